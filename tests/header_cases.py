"""Header.Hash edge cases shared by the host and the device tests of header_hash_kernel (test helper):
every zero-omission of the 14 leaves, the lengths either side of the kernel's limits, and mixed batches."""
import random

from test_merkle_oracle import kat_header
from oracle import merkle as M

ZERO_TIME_SECONDS = -62135596800  # Go's zero time: a 10-byte varint


def fused_ok(h) -> bool:
    """The kernel's limits (include/tmed25519.h, tmed_header_hashes): every leaf within two SHA-256
    blocks.  Any other header takes the host-leaf route."""
    bh, _, ph = h["last_block_id"]
    return (len(h["chain_id"].encode()) <= 50 and all(len(h[k]) <= 64 for k in M.HEADER_HASH_FIELDS) and
            len(bh) <= 64 and len(ph) <= 64 and 1 + len(M.header_leaves(h)[4]) <= 119)


def with_(**kw):
    h = kat_header()
    h.update(kw)
    return h


def edge_headers():
    """The KAT, every zero-omission, chain-id lengths 0 / 1 / 50 / 51, AppHash lengths 0 / 1 / 20 / 32 /
    64 / 65, an empty ValidatorsHash, and the extremes of every varint."""
    rng = random.Random(11)
    hs = [kat_header(),
          with_(height=0), with_(version_block=0, version_app=0), with_(version_block=0), with_(version_app=0),
          with_(chain_id=""), with_(time=(ZERO_TIME_SECONDS, 0)), with_(time=(0, 0)), with_(time=(0, 7)),
          with_(time=(1700000000, 999999999)), with_(time=(253402300799, 999999999)), with_(time=(-1, 1)),
          with_(last_block_id=(b"", 6, bytes(32))), with_(last_block_id=(bytes(32), 0, bytes(32))),
          with_(last_block_id=(bytes(32), 6, b"")), with_(last_block_id=(b"", 0, b"")),
          with_(last_block_id=(rng.randbytes(32), 2**32 - 1, rng.randbytes(32))),
          with_(last_block_id=(rng.randbytes(32), 128, rng.randbytes(32))),
          with_(last_block_id=(rng.randbytes(64), 1, rng.randbytes(46))),   # the LastBlockID leaf at 118 bytes
          with_(last_block_id=(rng.randbytes(64), 1, rng.randbytes(47))),   # ... and past it: the host route
          with_(last_block_id=(rng.randbytes(64), 300, rng.randbytes(64))),
          with_(last_block_id=(rng.randbytes(65), 1, b"")),
          with_(height=2**63 - 1, version_block=2**64 - 1, version_app=2**64 - 1),
          with_(height=127), with_(height=128), with_(version_block=2**35, version_app=1)]
    for k in M.HEADER_HASH_FIELDS:
        hs.append(with_(**{k: b""}))
    for n in (0, 1, 50, 51):
        hs.append(with_(chain_id="c" * n))
    for n in (0, 1, 20, 32, 52, 53, 64, 65):  # 52 / 53: the one-block / two-block boundary of a bytes leaf
        hs.append(with_(app_hash=rng.randbytes(n)))
    hs.append(with_(chain_id="x" * 50, **{k: rng.randbytes(64) for k in M.HEADER_HASH_FIELDS}))
    hs.append(with_(**{k: b"" for k in M.HEADER_HASH_FIELDS}))
    for _ in range(40):
        h = kat_header()
        h["height"] = rng.choice([0, 1, 3, 2**40, 2**63 - 1])
        h["chain_id"] = rng.choice(["", "c", "test_chain_id", "x" * 50, "y" * 51])
        h["time"] = (rng.choice([0, ZERO_TIME_SECONDS, 1700000000]), rng.choice([0, 1, 999999999]))
        h["version_block"], h["version_app"] = rng.choice([0, 11]), rng.choice([0, 1, 2**33])
        h["last_block_id"] = (rng.choice([b"", rng.randbytes(32)]), rng.choice([0, 1, 6, 300]),
                              rng.choice([b"", rng.randbytes(32)]))
        for k in M.HEADER_HASH_FIELDS:
            r = rng.random()
            if r < 0.2:
                h[k] = b""
            elif r < 0.3:
                h[k] = rng.randbytes(rng.choice([1, 20, 33, 64, 65, 200]))
        hs.append(h)
    return hs


def batch(n, seed=5):
    """n headers, eligible and ineligible ones mixed, all different."""
    rng = random.Random(seed * 1000 + n)
    pool = edge_headers()
    out = []
    for i in range(n):
        h = dict(rng.choice(pool))
        h["height"] = i + 1 if h["height"] else 0
        h["data_hash"] = rng.randbytes(32)
        out.append(h)
    return out
