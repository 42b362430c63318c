"""The setup ceremonies of the shim over the stand-in `bls12_381` / `alt_bn128_254` types on the GPU, driven through
tests/cpp/ceremony_test.cpp -> libceremonytest.so (a target of tests/cpp/Makefile):

  transform_accumulator  (hip/powers_of_tau.hpp; powers_of_tau_accumulator::transform, accumulator.hpp:89-121) from the reference's initial
                         accumulator -- every entry the generator -- so that after one key the entries are tau^i G1, tau^i G2, alpha tau^i G1,
                         beta tau^i G1 and beta G2, and after a second key the exponents have multiplied;
  power_pairs / merge_pairs  (vector_pairs.hpp:30-71) with the random scalars given: both sums against the oracle's MSM over the two ranges;
  contribute_randomness  (hip/r1cs_gg_ppzksnark_mpc.hpp; crs_operations.hpp:109-129): H_query and L_query by delta^-1, the three delta points
                         by delta.

Every expected point is the oracle's multiple of the generator by the exponent computed here with Python integers."""
import ctypes

import numpy as np
import pytest

import arith_cases as ac
import cport as cp
from harness import library
from util import CURVES, FQ_LIMBS, fr_arr, fr_ints

pytestmark = pytest.mark.gpu
P = ac._ptr
Z = ctypes.c_size_t


@pytest.fixture(scope="module")
def harness():
    return library("libceremonytest.so")


def multiples(curve, group, exps):
    """rows and flags of e G for every exponent (Python integers, reduced here); rows at infinity zeroed"""
    r = CURVES[curve].r
    pts, inf = cp.batch_mul(curve, group, fr_arr([e % r for e in exps]))
    pts[inf != 0] = 0
    return pts, inf


class Output:
    """the harness's output: points of either group one after the other in one u64 buffer, one flag each"""

    def __init__(self, curve, n_g1, n_g2):
        self.L = FQ_LIMBS[curve]
        self.xy = np.zeros(2 * self.L * (n_g1 + 2 * n_g2), dtype=np.uint64)
        self.inf = np.full(n_g1 + n_g2, 7, dtype=np.uint8)
        self.at_xy = self.at_inf = 0

    def take(self, group, n):
        w = 2 * self.L * group
        pts = self.xy[self.at_xy:self.at_xy + n * w].reshape(n, w).copy()
        inf = self.inf[self.at_inf:self.at_inf + n].copy()
        self.at_xy += n * w
        self.at_inf += n
        pts[inf != 0] = 0
        return pts, inf


def same(got, exp):
    return (got[1] == exp[1]).all() and (got[0] == exp[0]).all()


@pytest.mark.parametrize("length", [8, 64])
@pytest.mark.parametrize("curve", [0, 1])
def test_transform_accumulator(harness, curve, length):
    """tau_powers_length 8 (15 / 8 / 8 / 8 points) and 64 (127 points: two waves of the ladder launch)"""
    r = CURVES[curve].r
    keys = [fr_ints(cp.random_fr(curve, 9950 + k, 3)) for k in range(2)]    # (tau, alpha, beta) of two participants
    gen1, gen2 = cp.batch_mul(curve, 1, fr_arr([1]))[0], cp.batch_mul(curve, 2, fr_arr([1]))[0]
    tau, alpha, beta = 1, 1, 1
    for nkeys in (1, 2):
        t, a, b = keys[nkeys - 1]
        tau, alpha, beta = tau * t % r, alpha * a % r, beta * b % r    # a second contribution multiplies the exponents
        out = Output(curve, 4 * length - 1, length + 1)
        flat = fr_arr([x for key in keys[:nkeys] for x in key])
        assert harness.ceremony_transform(curve, Z(length), P(gen1), P(gen2), P(flat), Z(nkeys), P(out.xy), P(out.inf)) == 0
        powers = [pow(tau, i, r) for i in range(2 * length - 1)]
        assert same(out.take(1, 2 * length - 1), multiples(curve, 1, powers)), "tau_powers_g1"
        assert same(out.take(2, length), multiples(curve, 2, powers[:length])), "tau_powers_g2"
        assert same(out.take(1, length), multiples(curve, 1, [alpha * p for p in powers[:length]])), "alpha_tau_powers_g1"
        assert same(out.take(1, length), multiples(curve, 1, [beta * p for p in powers[:length]])), "beta_tau_powers_g1"
        assert same(out.take(2, 1), multiples(curve, 2, [beta])), "beta_g2"


@pytest.mark.parametrize("curve,group", [(0, 1), (1, 1), (0, 2)])
def test_power_pairs_and_merge_pairs(harness, curve, group):
    r, n = CURVES[curve].r, 65
    tau = fr_ints(cp.random_fr(curve, 9960, 1))[0]
    rs = cp.random_fr(curve, 9961, n - 1)
    # a genuine powers vector: res1 = (sum r_i tau^i) G and res2 = tau res1, in the exponent
    exps = [pow(tau, i, r) for i in range(n)]
    s1 = sum(ri * e for ri, e in zip(fr_ints(rs), exps)) % r
    genuine = multiples(curve, group, [s1, tau * s1])
    assert not genuine[1].any()
    # and a vector with no structure, a point at infinity in it
    loose = fr_ints(cp.random_fr(curve, 9962, n))
    loose[9] = 0
    for exps_v, want in ((exps, genuine), (loose, None)):
        v, v_inf = multiples(curve, group, exps_v)
        for mode in range(4):
            out = Output(curve, 2 if group == 1 else 0, 2 if group == 2 else 0)
            assert harness.ceremony_pairs(curve, group, mode, Z(n), P(v), P(v_inf), P(rs), P(out.xy), P(out.inf)) == 0, mode
            got = out.take(group, 2)
            for k, (lo, hi) in enumerate(((0, n - 1), (1, n))):
                exp, einf = cp.msm(curve, group, v[lo:hi], rs, inf=v_inf[lo:hi])
                assert got[1][k] == einf and (got[0][k] == exp).all(), (mode, k)
            assert want is None or same(got, want), mode


@pytest.mark.parametrize("curve", [0, 1])
def test_contribute_randomness(harness, curve):
    r, nh, nl = CURVES[curve].r, 63, 9
    h = fr_ints(cp.random_fr(curve, 9970, nh))
    l = fr_ints(cp.random_fr(curve, 9971, nl))
    h[4] = 0    # a query entry at infinity
    d1, d2, delta = fr_ints(cp.random_fr(curve, 9972, 3))
    dinv = pow(delta, -1, r)
    (h_xy, h_inf), (l_xy, l_inf) = multiples(curve, 1, h), multiples(curve, 1, l)
    out = Output(curve, nh + nl + 1, 2)
    rc = harness.ceremony_mpc(curve, Z(nh), Z(nl), P(h_xy), P(h_inf), P(l_xy), P(l_inf), P(multiples(curve, 1, [d1])[0]), P(multiples(curve, 2, [d2])[0]),
                              P(fr_arr([delta])), P(out.xy), P(out.inf))
    assert rc == 0
    assert same(out.take(1, nh), multiples(curve, 1, [x * dinv for x in h])), "H_query"
    assert same(out.take(1, nl), multiples(curve, 1, [x * dinv for x in l])), "L_query"
    assert same(out.take(1, 1), multiples(curve, 1, [d1 * delta])), "delta_g1"
    assert same(out.take(2, 2), multiples(curve, 2, [d2 * delta] * 2)), "delta_g2 of the proving and the verification key"
