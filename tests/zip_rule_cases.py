"""Fixtures the two signature rules disagree on, for the rule-as-a-context-setting tests
(tests/test_zip_rule_seam_host.py on the CPU, tests/test_gpu_zip_rule.py on the device).  No GPU
here; deterministic; fixed-seed keys; every signature is over the real CanonicalVote sign-bytes.

Two ways to build a signature that ZIP-215 accepts and Go 1.18's Verify rejects, with the private key:

  torsion   R' = rB + T with T of order 8, k = H(R' || A || M), S = r + k a.  Then
            [S]B - [k]A = rB = R' - T: the encodings differ (Go rejects) and [8](-T) = O (ZIP-215 accepts).
  noncanon  a non-canonical encoding of a valid R.  The encodings that decode and are not canonical
            are y >= p (y < 19) and x = 0 with the sign bit set; to sign, the signer must know r with
            R = rB, and of those points only the small-order ones have one (r = 0) — no search over
            seeds finds another, the chance is 2^-250 a seed.  So R is the identity written as y = p + 1
            and S = k a: [S]B - [k]A = O, whose canonical encoding is not the 32 bytes of R.

Signatures that both rules reject, at the same index: one flipped bit, and S + L."""
import functools
import hashlib
import json
import os

import numpy as np

from oracle import commit as C
from oracle import ed25519_go as E
from oracle import zip215 as Z
from oracle.fixtures import make_block_id, make_commit, make_valset, seed_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN = "zip215-chain"
_T8 = [t for t in E.small_order_points() if not E.pt_equal(E.pt_mul(4, t), E.IDENTITY)][0]
NONCANON_IDENTITY = (E.P + 1).to_bytes(32, "little")


def _secret(seed):
    h = hashlib.sha512(seed).digest()
    return E._clamp(h[:32]) % E.L, h[32:]


def sign_torsion(seed, msg):
    a, prefix = _secret(seed)
    pub = E.encode(E.pt_mul(a, E.BASE))
    r = E.sc_reduce64(hashlib.sha512(prefix + msg).digest())
    rb = E.encode(E.pt_add(E.pt_mul(r, E.BASE), _T8))
    s = (r + E.hram(rb, pub, msg) * a) % E.L
    return rb + s.to_bytes(32, "little")


def sign_noncanon(seed, msg):
    a, _ = _secret(seed)
    pub = E.encode(E.pt_mul(a, E.BASE))
    s = E.hram(NONCANON_IDENTITY, pub, msg) * a % E.L
    return NONCANON_IDENTITY + s.to_bytes(32, "little")


def flipped(sig):
    b = bytearray(sig)
    b[40] ^= 4
    return bytes(b)


def s_plus_l(sig):
    s = int.from_bytes(sig[32:], "little") + E.L
    assert s < 1 << 256
    return sig[:32] + s.to_bytes(32, "little")


_CACHE = {}


def verify_zip(pub, msg, sig):
    """oracle.zip215.verify, cached (the same tuples come back request after request)."""
    k = (bytes(pub), bytes(msg), bytes(sig))
    if k not in _CACHE:
        _CACHE[k] = Z.verify(*k)
    return _CACHE[k]


_GO = {}


def verify_go(pub, msg, sig):
    k = (bytes(pub), bytes(msg), bytes(sig))
    if k not in _GO:
        _GO[k] = E.verify(*k)
    return _GO[k]


def zip_batch_verifier(pubs, sigs, lens, msgs, offs):
    """The batch callback of tmed_verify_commits_with / tmed_light_verify_with over oracle.zip215.verify."""
    out = np.zeros(len(lens), np.uint8)
    for i in range(len(lens)):
        out[i] = verify_zip(pubs[i].tobytes(), msgs[int(offs[i]):int(offs[i + 1])].tobytes(), sigs[i].tobytes()[:int(lens[i])])
    return out


@functools.lru_cache(maxsize=None)
def commit(n, kind, at, tag="zr", powers=None, flags=None, height=77):
    """(vs, seeds, bid, height, commit): n validators all for the block unless flags says otherwise,
    signature `at` rebuilt by `kind` ("torsion", "noncanon", "flip", "splusl", "flip_torsion" or None)."""
    powers = list(powers) if powers else [10] * n
    vs, seeds = make_valset([seed_of("%s%d" % (tag, n), i) for i in range(n)], powers)
    bid = make_block_id("%s%d" % (tag, n))
    cm = make_commit(vs, seeds, CHAIN, height, 1, bid, flags=list(flags) if flags else None)
    if kind is not None:
        msg = cm.vote_sign_bytes(CHAIN, at)
        good = cm.signatures[at].signature
        sig = {"torsion": lambda: sign_torsion(seeds[at], msg), "noncanon": lambda: sign_noncanon(seeds[at], msg),
               "flip": lambda: flipped(good), "splusl": lambda: s_plus_l(good),
               "flip_torsion": lambda: flipped(sign_torsion(seeds[at], msg))}[kind]()
        pub = vs.validators[at].pub_key
        want = {"torsion": (False, True), "noncanon": (False, True)}.get(kind, (False, False))
        assert (verify_go(pub, msg, sig), verify_zip(pub, msg, sig)) == want, kind
        cm.signatures[at].signature = sig
    return vs, seeds, bid, height, cm


def expected(mode, vs, bid, h, cm, num=1, den=3, rule="go"):
    fn = verify_go if rule == "go" else verify_zip
    if mode == 0:
        return C.verify_commit(vs, CHAIN, bid, h, cm, verify_fn=fn)
    if mode == 1:
        return C.verify_commit_light(vs, CHAIN, bid, h, cm, verify_fn=fn)
    return C.verify_commit_light_trusting(vs, CHAIN, cm, num, den, verify_fn=fn)


@functools.lru_cache(maxsize=None)
def corpus():
    """Both golden files' tuples with 32-byte keys -> (keys (distinct, (K, 32) uint8), idx, sigs (n, 64)
    zero-padded, lens, msgs, offs, valid_go, valid_zip215 by oracle.zip215.verify)."""
    vs = []
    for f in ("ed25519_vectors.json", "zip215_vectors.json"):
        with open(os.path.join(ROOT, "tests", "golden", f)) as fh:
            vs += json.load(fh)["vectors"]
    tup = [(bytes.fromhex(v["pub"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"]),
            int(v["valid_go"] if "valid_go" in v else v["valid"]), v.get("valid_zip215")) for v in vs]
    tup = [t for t in tup if len(t[0]) == 32]
    keys = sorted({t[0] for t in tup})
    pos = {k: i for i, k in enumerate(keys)}
    n = len(tup)
    idx = np.array([pos[t[0]] for t in tup], np.uint32)
    sigs = np.zeros((n, 64), np.uint8)
    lens = np.zeros(n, np.uint32)
    offs = np.zeros(n + 1, np.uint32)
    for i, (_, msg, sig, _, _) in enumerate(tup):
        lens[i] = len(sig)
        sigs[i, :min(len(sig), 64)] = np.frombuffer(sig[:64], np.uint8)
        offs[i + 1] = offs[i] + len(msg)
    msgs = np.frombuffer(b"".join(t[1] for t in tup) + bytes(16), np.uint8).copy()
    go = np.array([t[3] for t in tup], np.uint8)
    zp = np.array([Z.verify(t[0], t[1], t[2]) for t in tup], np.uint8)
    for i, t in enumerate(tup):  # the file's own column where it has one
        assert t[4] is None or int(t[4]) == zp[i]
    assert any(E.decode(k) is None for k in keys) and (lens != 64).any() and (go != zp).any()
    return np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), 32).copy(), idx, sigs, lens, msgs, offs, go, zp


# ---- light.Verify pairs ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def light_cases():
    """[adjacent, non-adjacent] light_cases.Case whose untrusted commit carries a torsion signature at
    its first index (in front of both loops' power crossings)."""
    import light_cases as LC
    chain = "zip215-light"
    keys = LC.gen_keys("ziplight", 4)
    vals = LC.to_validators(keys, 20, 10)
    trusted = LC.gen_signed_header(keys, chain, 1, LC.BTIME, vals, vals, 0, 4)
    out = []
    for name, height in (("adjacent", 2), ("non-adjacent", 5)):
        sh = LC.gen_signed_header(keys, chain, height, LC.time_add(LC.BTIME, LC.HOUR), vals, vals, 0, 4)
        seed = next(s for s, p in keys if p == vals.validators[0].pub_key)
        msg = sh.commit.vote_sign_bytes(chain, 0)
        sh.commit.signatures[0].signature = sign_torsion(seed, msg)
        out.append(LC.Case("zip rule/" + name, trusted, vals, sh, vals))
    return out


def light_expected(case, rule):
    """The restatement's error for the case under a rule (light_cases.verify with that rule's primitive)."""
    import light_cases as LC
    saved = LC.fast_verify
    LC.fast_verify = verify_go if rule == "go" else verify_zip
    try:
        return case.expected()
    finally:
        LC.fast_verify = saved
