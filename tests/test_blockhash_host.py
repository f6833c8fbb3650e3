"""Commit.Hash / Data.Hash without a device: the Python restatement against the reference's pinned
CommitSig size, the exact leaf-encoder source (csrc/commitsig_leaf.h, csrc/sha256.h) compiled for
the host against that restatement, and the argument checks of the two C-ABI calls."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import blockhash_cases as B
from oracle import merkle as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tendermint-fork_amd", "csrc")


@pytest.fixture(scope="session")
def blockhash_host(tmp_path_factory):
    """tests/native/blockhash_host.cpp built into a temporary directory."""
    so = str(tmp_path_factory.mktemp("blockhash") / "libblockhash_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "blockhash_host.cpp"), "-o", so])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_restatement_pinned_size():
    """types/block_test.go:260-274 builds the largest CommitSig and asserts 109 bytes."""
    big = B.commitsig_bytes(3, bytes(range(20)), B.ZERO_TIME_SECONDS, 999999999, bytes(range(64)))
    assert len(big) == B.MAX_COMMIT_SIG_BYTES == 109
    assert B.commitsig_bytes(0, b"", 0, 0, b"") == bytes.fromhex("1a00")
    absent = B.commitsig_bytes(1, b"", B.ZERO_TIME_SECONDS, 0, b"")
    tenbyte = bytes.fromhex("8092b8c398feffffff01")
    assert sum((b & 0x7F) << (7 * k) for k, b in enumerate(tenbyte)) == B.ZERO_TIME_SECONDS % 2 ** 64
    assert absent == bytes.fromhex("0801" "1a0b" "08") + tenbyte
    assert B.commit_hash([]).hex() == B.EMPTY_HASH and B.txs_hash([]).hex() == B.EMPTY_HASH


def test_encoder_stream_bytes(blockhash_host):
    """The word stream itself (prefix, leaf, pad byte, bit length) for the extreme leaves."""
    out = (ctypes.c_uint8 * 112)()
    for flag, addr, sec, nan, sig in [(3, bytes(range(1, 21)), B.ZERO_TIME_SECONDS, 999999999, bytes(range(100, 164))),
                                      (0, b"", 0, 0, b""), (1, b"", B.ZERO_TIME_SECONDS, 0, b""),
                                      (255, bytes(20), -1, 1, b"\xff")]:
        n = blockhash_host.bh_commitsig_stream(ctypes.c_uint8(flag), len(addr), addr.ljust(20, b"\0"),
                                               ctypes.c_int64(sec), ctypes.c_int32(nan), sig.ljust(64, b"\xee"),
                                               len(sig), out)
        leaf = B.commitsig_bytes(flag, addr, sec, nan, sig)
        raw = bytes(out)
        assert n == len(leaf)
        assert raw[:n + 2] == b"\0" + leaf + b"\x80"
        if n + 1 <= 55:
            assert raw[n + 2:60] == bytes(58 - n) and raw[60:64] == (8 * (n + 1)).to_bytes(4, "big")
        else:
            assert raw[n + 2:] == bytes(110 - n)


def test_commitsig_encoder_sweep(blockhash_host):
    """flags x address lengths x signature lengths 0..64 x seconds x nanos, all of them: the leaf
    digest and the leaf length of the host-compiled encoder equal the restatement."""
    cases = list(B.full_sweep())
    n = len(cases)
    assert n == 7 * 2 * 65 * 9 * 7
    pc = B.packed_commit(cases)
    dig = np.zeros((n, 32), np.uint8)
    lens = np.zeros(n, np.uint32)
    blockhash_host.bh_commitsig_leaf_digests(ctypes.c_size_t(n), _p(pc.flags), _p(pc.address_lens), _p(pc.addresses),
                                             _p(pc.ts_seconds), _p(pc.ts_nanos), _p(pc.sigs), _p(pc.sig_lens),
                                             _p(dig), _p(lens))
    seen = set()
    for i, c in enumerate(cases):
        leaf = B.commitsig_bytes(*c)
        assert lens[i] == len(leaf), c
        assert bytes(dig[i]) == M.leaf_hash(leaf), c
        seen.add(len(leaf))
    assert {2, 54, 55, 109} <= seen  # the shortest, both sides of the block boundary, the longest


def test_tx_leaf_sweep(blockhash_host):
    """Transaction lengths 0..130 and 1000 (every padding position of both SHA-256 passes), at every
    dword misalignment."""
    out = (ctypes.c_uint8 * 32)()
    buf = np.frombuffer(B._pattern(1100, 9), np.uint8).copy()
    base = buf.ctypes.data
    for n in list(range(131)) + [1000]:
        for mis in range(4):
            start = (-base) % 4 + 4 + mis
            tx = bytes(buf[start:start + n])
            blockhash_host.bh_tx_leaf_digest(ctypes.c_void_p(base + start), n, out)
            assert bytes(out) == M.leaf_hash(hashlib.sha256(tx).digest()), (n, mis)


def test_null_context_and_empty_calls():
    from tmed.merkle import _bind
    from tmed._native import TMED_EINVAL, TMED_OK
    l = _bind()
    out = np.zeros(32, np.uint8)
    ok = np.zeros(1, np.uint8)
    from tmed.types import _CommitC
    commit = _CommitC()
    off64 = np.zeros(2, np.uint64)
    off32 = np.zeros(2, np.uint32)
    assert l.tmed_commit_hashes(None, ctypes.byref(commit), 1, _p(out), _p(ok)) == TMED_EINVAL
    assert l.tmed_txs_hashes(None, None, _p(off64), _p(off32), 1, _p(out)) == TMED_EINVAL
    # n == 0 returns before the context is looked at: any non-NULL pointer stands in for one here
    fake = np.zeros(64, np.uint8)
    assert l.tmed_commit_hashes(_p(fake), None, 0, None, None) == TMED_OK
    assert l.tmed_txs_hashes(_p(fake), None, None, None, 0, None) == TMED_OK


def test_compiled_host_marshal_matches_restatement():
    """shim/go_marshal.cpp gm_marshal_commitsigs (the host route bench_merkle.py times against the
    device encoder) writes the restatement's bytes."""
    from tmed import gomarshal as G
    cases = list(B.full_sweep())[::7]
    pc = B.packed_commit(cases)
    out, off = G.marshal_commitsigs(pc.flags, pc.addresses, pc.ts_seconds, pc.ts_nanos, pc.sigs, pc.sig_lens,
                                    pc.address_lens)
    for i, c in enumerate(cases):
        assert bytes(out[int(off[i]):int(off[i + 1])]) == B.commitsig_bytes(*c), c
