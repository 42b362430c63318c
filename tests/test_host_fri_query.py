"""Host side of the FRI query phase, no GPU: the tests' restatement of calculate_s (fri_query_ref) against the oracle's leaf layout, and the
shim's host arithmetic -- detail::pair_positions and detail::domain_index (hip/lpc.hpp) -- through tests/cpp/fri_query_test.cpp."""
import ctypes

import numpy as np
import pytest

import fri_query_ref as fq
import pasta_util  # noqa: F401  (adds Pallas and Vesta to util.CURVES)
import pyoracle as po
from harness import library
from util import CURVES, limbs


@pytest.fixture(scope="module")
def harness():
    return library("libfriquerytest.so")


def test_restated_walk_is_a_leaf_of_the_oracle():
    """Runs no product code: it validates the tests' own restatement (fri_query_ref, which the GPU tests hold the product against) against
    the oracle, and so passes with or without the feature.  log_domain 1-7, steps 1-5, every x: the values at calculate_s's indices are a
    permutation of leaf x mod (D >> step) of pyoracle.fri_leaves, in the leaf's own order when x < D >> step, and leaf_order restores that
    order for every x"""
    for log_d in range(1, 8):
        D = 1 << log_d
        polys = [[1000 * p + i for i in range(D)] for p in range(2)]
        for step in range(1, min(5, log_d) + 1):
            leaves = np.array(po.fri_leaves(polys, step)).reshape(D >> step, 2, 1 << (step - 1), 2)
            for x in range(D):
                got = np.array([[[f[a], f[b]] for a, b in fq.calculate_s(x, D, step)] for f in polys])
                leaf = leaves[x % (D >> step)]
                assert sorted(got.reshape(-1)) == sorted(leaf.reshape(-1)), (log_d, step, x)
                if x < D >> step:
                    assert np.array_equal(got, leaf), (log_d, step, x)
                assert np.array_equal(fq.leaf_order(got[..., None], x, D, step)[..., 0], leaf), (log_d, step, x)


def test_pair_positions_are_the_smaller_indices(harness):
    for log_d, step in [(1, 1), (3, 3), (5, 1), (5, 2), (5, 4), (7, 5), (12, 2)]:
        D = 1 << log_d
        out = np.zeros(1 << (step - 1), dtype=np.uint64)
        for x in list(range(min(D, 64))) + [D - 1, D // 2, D // 2 - 1]:
            harness.fq_pair_positions(ctypes.c_size_t(x), ctypes.c_size_t(log_d), ctypes.c_size_t(step), out.ctypes.data_as(ctypes.c_void_p))
            assert list(out) == [p[0] for p in fq.calculate_s(x, D, step)], (log_d, step, x)


@pytest.mark.parametrize("curve", [0, 1, 2, 3])
def test_domain_index_against_the_domain_table(harness, curve):
    """the walk down the 2-power subgroups finds the index the reference's scan finds: whole domains up to 2^6, edge and random elements up
    to 2^12 (1, -1, omega, omega^(D - 1)); 0 and an element of twice the order are refused"""
    C = CURVES[curve]
    r = C.r
    out = ctypes.c_uint64()

    def index(x, log_d):
        rc = harness.fq_domain_index(curve, limbs(x, 4).ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(log_d), ctypes.byref(out))
        assert rc in (0, 1)
        return out.value if rc == 0 else None

    rng = po.SplitMix64(40 + curve)
    for log_d in range(1, 13):
        D, w = 1 << log_d, C.root_of_unity(log_d)
        table = fq.domain_table(w, D, r)
        picks = range(D) if log_d <= 6 else [0, 1, D // 2, D - 1] + [rng.next_mod(D) for _ in range(12)]
        for i in picks:
            x = pow(w, i, r)
            assert index(x, log_d) == table[x] == i, (log_d, i)
        assert index(1, log_d) == 0 and index(r - 1, log_d) == D // 2
        assert index(0, log_d) is None
        assert index(C.root_of_unity(log_d + 1), log_d) is None
        # a challenge taken into the domain as the query phase does it
        c = rng.next_mod(r - 1) + 1
        x = pow(c, (r - 1) >> log_d, r)
        assert index(x, log_d) == table[x]
