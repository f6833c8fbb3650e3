"""Python restatement of the block-integrity hashes Block.ValidateBasic recomputes
(types/block.go:55-106) and the case sweeps the CPU and GPU suites share.

  CommitSig leaf   cs.ToProto().Marshal(), proto/tendermint/types/types.pb.go:1563-1596 with
                   gogoproto StdTime: fields in ascending order,
                     08 varint(flag)     if flag != 0
                     12 len addr         if len(addr) > 0
                     1a len ts           always; ts = [08 varint(uint64(seconds))] if seconds != 0,
                                         then [10 varint(nanos)] if nanos != 0
                     22 len sig          if len(sig) > 0
  Commit.Hash      types/block.go:894-912: HashFromByteSlices over the marshalled CommitSigs
  Data.Hash        types/block.go:1004-1012 -> Txs.Hash, types/tx.go:47-55: HashFromByteSlices over
                   SHA-256(tx)

The reference holds no Commit.Hash known answer: the marshal rule is pinned by its size only
(MaxCommitSigBytes = 109, types/block.go:591, types/block_test.go:260-274)."""
import hashlib

from oracle.merkle import hash_from_byte_slices
from oracle.signbytes import uvarint

MAX_COMMIT_SIG_BYTES = 109
ZERO_TIME_SECONDS = -62135596800          # Go's time.Time{}.Unix()
MAX_SECONDS = 253402300800                # StdTimeMarshal accepts [ZERO_TIME_SECONDS, MAX_SECONDS)
EMPTY_HASH = "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"

FLAGS = (0, 1, 2, 3, 127, 128, 255)
ADDR_LENS = (0, 20)
SIG_LENS = tuple(range(65))
SECONDS = (0, 1, 127, 128, 2 ** 31, 1700000000, -1, ZERO_TIME_SECONDS, MAX_SECONDS - 1)
NANOS = (0, 1, 127, 128, 2 ** 28 - 1, 2 ** 28, 999999999)


def _u64(v: int) -> int:
    return v & 0xFFFFFFFFFFFFFFFF


def timestamp_bytes(seconds: int, nanos: int) -> bytes:
    out = b""
    if seconds != 0:
        out += b"\x08" + uvarint(_u64(seconds))
    if nanos != 0:
        out += b"\x10" + uvarint(_u64(nanos))
    return out


def commitsig_bytes(flag: int, address: bytes, seconds: int, nanos: int, signature: bytes) -> bytes:
    out = b""
    if flag != 0:
        out += b"\x08" + uvarint(flag)
    if len(address) > 0:
        out += b"\x12" + uvarint(len(address)) + bytes(address)
    ts = timestamp_bytes(seconds, nanos)
    out += b"\x1a" + uvarint(len(ts)) + ts
    if len(signature) > 0:
        out += b"\x22" + uvarint(len(signature)) + bytes(signature)
    return out


def commit_leaves(sigs) -> list:
    """sigs: (flag, address, seconds, nanos, signature) tuples."""
    return [commitsig_bytes(*s) for s in sigs]


def commit_hash(sigs) -> bytes:
    return hash_from_byte_slices(commit_leaves(sigs))


def txs_hash(txs) -> bytes:
    return hash_from_byte_slices([hashlib.sha256(bytes(t)).digest() for t in txs])


def _pattern(n: int, salt: int) -> bytes:
    return bytes((salt * 131 + 7 * k + (k * k >> 3)) & 0xFF for k in range(n))


def full_sweep():
    """The whole product of the sweep: (flag, address, seconds, nanos, signature) tuples."""
    i = 0
    for flag in FLAGS:
        for al in ADDR_LENS:
            for sl in SIG_LENS:
                sig, addr = _pattern(sl, i + 1000), _pattern(al, i)
                i += 1
                for sec in SECONDS:
                    for nan in NANOS:
                        yield (flag, addr, sec, nan, sig)


def cycle_sigs():
    """A walk through the sweep short enough for one GPU call: every signature length 0..64 meets
    every flag, seconds and nanos value and both address lengths (585 signatures; with the 5-byte
    seconds varints the leaf length crosses the 54/55 block boundary), deterministic."""
    out = []
    i = 0
    for sl in SIG_LENS:
        for k in range(max(len(FLAGS), len(SECONDS), len(NANOS))):
            flag = FLAGS[(k + sl) % len(FLAGS)]
            al = ADDR_LENS[(k + i) % 2]
            sec = SECONDS[(k + 2 * sl) % len(SECONDS)]
            nan = NANOS[(k + 3 * sl) % len(NANOS)]
            out.append((flag, _pattern(al, i), sec, nan, _pattern(sl, i + 1000)))
            i += 1
    return out


def packed_commit(sigs, address_lens="explicit"):
    """A tmed.types.PackedCommit of the sigs.  address_lens: "explicit" (u32 per signature) or None
    (every address must then be 20 bytes)."""
    import numpy as np
    from tmed.types import BlockID, PackedCommit
    n = len(sigs)
    flags = np.zeros(n, np.uint8)
    addrs = np.zeros((n, 20), np.uint8)
    sec = np.zeros(n, np.int64)
    nan = np.zeros(n, np.int32)
    sg = np.zeros((n, 64), np.uint8)
    sl = np.zeros(n, np.uint32)
    al = np.zeros(n, np.uint32)
    for i, (f, a, s, ns, sig) in enumerate(sigs):
        flags[i] = f
        al[i] = len(a)
        if len(a) == 20:
            addrs[i] = np.frombuffer(a, np.uint8)
        sec[i], nan[i] = s, ns
        sl[i] = len(sig)
        if 0 < len(sig) <= 64:
            sg[i, :len(sig)] = np.frombuffer(sig, np.uint8)
        # bytes of the slot past the signature are not part of it: the engine must ignore them
        sg[i, min(len(sig), 64):] = 0xA5
    if address_lens is None:
        assert (al == 20).all()
    return PackedCommit(1, 0, BlockID(), flags, addrs, sec, nan, sg, sl, None if address_lens is None else al)
