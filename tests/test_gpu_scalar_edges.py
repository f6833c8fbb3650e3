"""GPU: signatures whose S (and k) sit at the edges of the kernels' signed-digit recodings
(tests/scalar_edge_cases.py), as one batch through every route, bit for bit against the oracle.

S is the signer's to choose, and it is the B scalar of the key-cached throughput kernels (biased
radix 2^16; carry-free radix 2^24 read off the scalar on the device only), the key-cached latency
kernel (radix 256), the variant-5 main kernel (radix 2^16) and the ZIP-215 final comb; k's radix-2^12
digits index the key set's -A comb.  The batch is shuffled once with a fixed seed, so the edge lanes
share waves with ordinary ones."""
import numpy as np
import pytest

import scalar_edge_cases as SC
from conftest import engine_with_env
from oracle import port

pytestmark = pytest.mark.gpu

# context -> the routes it serves: generic batches above TMED_GLAT_MAX take the throughput kernels,
# key-cached batches above TMED_LAT_MAX the throughput kernels
CONTEXTS = {
    "default": dict(TMED_GLAT_MAX=0, TMED_LAT_MAX=0),
    "radix16": dict(TMED_GLAT_MAX=0, TMED_LAT_MAX=0, TMED_B26=0, TMED_B24=0),
    "v5_a8": dict(TMED_GLAT_MAX=0, TMED_LAT_MAX=0, TMED_MAIN_WAVES=5, TMED_KS_ACOMB=0),
    "latency": dict(TMED_GLAT_MAX=1 << 16, TMED_LAT_MAX=1 << 16),
}


@pytest.fixture(scope="module")
def batch():
    n = len(SC.cases())
    order = np.random.default_rng(0xED6E).permutation(n)
    pubs, sigs, msgs, offs, exp = SC.arrays(order=order)
    karr, idx = SC.keyed(pubs)
    tags = [SC.cases()[i]["tag"] for i in order]
    assert 0 < exp.sum() < n and n > 1024  # several blocks, accepts and rejects mixed
    return dict(pubs=pubs, sigs=sigs, msgs=msgs, offs=offs, exp=exp, karr=karr, idx=idx, tags=tags)


@pytest.fixture(scope="module")
def edge_engines():
    es = {name: engine_with_env(TMED_SLAB_SLOTS=4096, **env) for name, env in CONTEXTS.items()}
    yield es
    for e in es.values():
        e.close()


def _same(out, b, exp=None):
    exp = b["exp"] if exp is None else exp
    assert (out == exp).all(), [b["tags"][i] for i in np.nonzero(out != exp)[0]][:10]


@pytest.mark.parametrize("ctx,b_bits", [("default", 26), ("radix16", 16), ("v5_a8", 26), ("latency", 26)])
def test_generic_routes(edge_engines, batch, ctx, b_bits):
    """The half-size kernels on the radix-2^26 and the radix-2^16 B windows, the full-length variant 5
    (S in biased radix 2^16 on the 32769-row table) and the generic latency kernels."""
    eng = edge_engines[ctx]
    assert eng.b_window_bits() == b_bits
    _same(eng.verify_arrays(batch["pubs"], batch["sigs"], batch["msgs"], batch["offs"]), batch)


@pytest.mark.parametrize("ctx,ks_bits,a_bits", [("default", 24, 12), ("v5_a8", 24, 8), ("radix16", 16, 8),
                                                ("latency", 24, 8)])
def test_key_cached_routes(edge_engines, batch, ctx, ks_bits, a_bits):
    """keyset_straus_ab24 (the default: radix-2^12 -A comb from the second batch on, radix-2^24 B),
    keyset_straus_b24 (the first batch, and TMED_KS_ACOMB=0), keyset_straus_pf (TMED_B24=0) and the
    key-cached latency kernel (radix 256 of both scalars)."""
    eng = edge_engines[ctx]
    h = eng.keyset_load(batch["karr"])
    try:
        assert eng.keyset_b_window_bits() == ks_bits
        assert eng.keyset_a_window_bits(h) == 8
        for _ in range(2):
            _same(eng.verify_keyset_arrays(h, batch["idx"], batch["sigs"], batch["msgs"], batch["offs"]), batch)
            assert eng.keyset_a_window_bits(h) == a_bits
    finally:
        eng.keyset_free(h)


def test_zip215_route(edge_engines, batch):
    """The ZIP-215 rule (batch equation, bisection around the rejects, single checks) against the
    port's ZIP-215 bits; then the accepted ones alone, which one batch equation decides."""
    eng = edge_engines["default"]
    exp = port.verify_batch(batch["pubs"], batch["sigs"], batch["msgs"], batch["offs"].astype(np.uint64), 8,
                            zip215=True)
    _same(eng.verify_zip215_arrays(batch["pubs"], batch["sigs"], batch["msgs"], batch["offs"]), batch, exp)
    good = [i for i, c in enumerate(SC.cases()) if c["valid"]]
    pubs, sigs, msgs, offs, ones = SC.arrays(order=good)
    out = eng.verify_zip215_arrays(pubs, sigs, msgs, offs)
    assert ones.all() and out.all(), [SC.cases()[good[i]]["tag"] for i in np.nonzero(out == 0)[0]][:10]
