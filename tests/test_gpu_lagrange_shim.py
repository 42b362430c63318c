"""The Lagrange-basis SRS of kimchi_pedersen_hip (crypto3-zk_amd/include/nil/crypto3/zk/hip/kimchi_pedersen.hpp: params_type::
add_lagrange_basis, lagrange_bases, commitment_evaluations) over the stand-in `pallas` / `vesta` types on the GPU, driven through
tests/cpp/lagrange_test.cpp -> liblagrangetest.so (a target of tests/cpp/Makefile).  |g| = 2^9 generators k_i G, domains of 2^9 and 2^5 points:
every entry of both bases against the oracle (its inverse NTT of the k_i in the exponent), no launch when a size is added again, what
throws, and the commitment of a column from its evaluations against the oracle's sum over the basis and against `commitment` of the
column's coefficients minus its blinding term."""
import numpy as np
import pytest

import arith_cases as ac
import cport as cp
import pasta_util as pu
from harness import library
from util import fr_arr, fr_ints, limbs, pt_from_limbs, pts_arr

pytestmark = pytest.mark.gpu
P = ac._ptr


@pytest.fixture(scope="module")
def harness():
    return library("liblagrangetest.so")


def basis(curve, ks, log_m):
    m, w = 1 << log_m, limbs(pu.CURVES[curve].root_of_unity(log_m), 4)
    pts, inf = cp.batch_mul(curve, 1, cp.ntt(curve, ks[:m].reshape(1, m, 4), log_m, w, inverse=True)[0])
    pts[inf != 0] = 0
    return pts, inf


@pytest.mark.parametrize("curve", [2, 3])
def test_lagrange_bases_and_commitment_from_evaluations(harness, curve):
    C = pu.CURVES[curve]
    r, n, log_big, log_small = C.r, 512, 9, 5
    big, small = 1 << log_big, 1 << log_small
    ks = cp.random_fr(curve, 9100, n)
    g_xy, _ = cp.batch_mul(curve, 1, ks)
    h = pu.random_points(curve, 9101, 1)[0]
    draws = fr_ints(cp.random_fr(curve, 9102, 4))
    evals = cp.random_fr(curve, 9103, big)
    evals[7] = 0
    w_big = limbs(C.root_of_unity(log_big), 4)
    coeffs = cp.ntt(curve, evals.reshape(1, big, 4), log_big, w_big, inverse=True)[0]
    omegas = np.concatenate([w_big, limbs(C.root_of_unity(log_small), 4)])
    sizes = np.array([n, big, small, len(draws)], dtype=np.uint64)
    out = dict(big_xy=np.zeros((big, 8), dtype=np.uint64), big_inf=np.zeros(big, dtype=np.uint8), small_xy=np.zeros((small, 8), dtype=np.uint64),
               small_inf=np.zeros(small, dtype=np.uint8), commit=np.zeros(20, dtype=np.uint64), counts=np.zeros(10, dtype=np.uint64))
    rc = harness.lagrange_run(curve, P(sizes), P(g_xy), P(pts_arr(curve, 1, [h])), P(omegas), P(evals), P(coeffs), P(fr_arr(draws)), P(out["big_xy"]),
                              P(out["big_inf"]), P(out["small_xy"]), P(out["small_inf"]), P(out["commit"]), P(out["counts"]))
    assert rc == 0, rc
    counts = [int(x) for x in out["counts"]]

    # lagrange_bases[n]: every entry of both sizes
    exp_big, exp_big_inf = basis(curve, ks, log_big)
    exp_small, exp_small_inf = basis(curve, ks, log_small)
    out["big_xy"][out["big_inf"] != 0] = 0
    out["small_xy"][out["small_inf"] != 0] = 0
    assert (out["big_inf"] == exp_big_inf).all() and (out["big_xy"] == exp_big).all()
    assert (out["small_inf"] == exp_small_inf).all() and (out["small_xy"] == exp_small).all()
    assert counts[0] > 0 and counts[1] == counts[0], "adding a size that is already there launched something"
    assert counts[2] == 2
    assert counts[3] == 1, "a domain larger than |g| did not throw"
    assert counts[4] == 1, "a domain that is no power of two did not throw"

    # commitment_evaluations = sum_j evals_j L_j, and = commitment(coefficients) - w h for the draw w
    exp, einf = cp.msm(curve, 1, exp_big, evals, inf=exp_big_inf)
    assert counts[5] == einf == 0 and (out["commit"][:8] == exp).all()
    by_evals = pt_from_limbs(curve, 1, out["commit"][:8], counts[5])
    hiding = pt_from_limbs(curve, 1, out["commit"][8:16], counts[6])
    assert fr_ints(out["commit"][16:20].reshape(1, 4))[0] == draws[0] and counts[7] == 2    # one draw per chunk, then one more
    assert hiding == C.g1.add(by_evals, C.g1.mul(h, draws[0]))
    assert counts[8] == 1, "a size that was not added did not throw"
    assert counts[9] == 0
