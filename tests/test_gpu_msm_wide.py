"""Level 2 of the MSM's two-level tail on the one-point-per-wave group law (csrc/fu_wide.hpp; msm_core.hpp msm_wide_weigh / msm_wide_tree /
msm_wide_final): the law itself against the one-lane formulas (tests/cpp/widetest.hip), and MSM results with it (msm_tail_quads = 1, the
default) against the same call on the lane quads (msm_tail_quads = 2) and against the oracle -- bit-exact after the conversion to affine.
msm_tail_fold is lowered so that 2^10 ... 2^13 points go through msm_fold and level 2; the profile tells which kernels ran."""
import subprocess

import numpy as np
import pytest

import cport as cp
import pasta_util  # noqa: F401  (ids 2 and 3 in util.CURVES)
from harness import program
from util import CURVES, fr_arr, jac_to_affine_py, pt_from_limbs

pytestmark = pytest.mark.gpu
WIDE, QUADS = 1, 2    # values of msm_tail_quads


def test_wide_group_law_unit(ctx):
    """product, sum, difference (limb for limb, at the limb bounds too), addition, doubling, small multiple, a chain of 64 operations, P + P,
    P + (-P), infinity on either side, coordinates 0 / 1 / p - 1, the load / store layout: BLS12-381, BN254, Pallas and Vesta base fields"""
    out = subprocess.run([program("widetest")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
    assert out.returncode == 0 and out.stdout.count("mismatch mask 0x0 ") == 4, out.stdout


def both_tails(ctx, bases, sc, tree=False):
    """the MSM with level 2 on the wide law and on the quads; the wide kernels must have run in the first and not in the second
    (tree: sets of more than 64 points, which need msm_wide_tree between the weighting and the final kernel)"""
    got = {}
    for mode in (WIDE, QUADS):
        ctx.set_option("msm_tail_quads", mode)
        ctx.profile_reset()
        ctx.profile(True)
        jac = ctx.msm(bases, sc)
        ctx.sync()
        ctx.profile(False)
        names = set(ctx.profile_dump())
        assert "msm_fold" in names, "the MSM did not take the two-level tail"
        assert ("msm_wide_weigh" in names) == ("msm_wide_final" in names) == (mode == WIDE), (mode, sorted(names))
        assert ("msm_wide_tree" in names) == (mode == WIDE and tree), (mode, sorted(names))
        dev_aff, dev_inf = ctx.jacobian_to_affine(bases.curve, bases.group, jac)
        got[mode] = (jac_to_affine_py(bases.curve, bases.group, jac), pt_from_limbs(bases.curve, bases.group, dev_aff, dev_inf))
        assert got[mode][0] == got[mode][1]
    assert got[WIDE] == got[QUADS]
    return got[WIDE][0]


def scalar_cases(curve, n, c):
    r = CURVES[curve].r
    half = 1 << ((c - 1 + 1) // 2)    # C of a set of 2^(c - 1) buckets: digits up to C stay in row 0 of the bucket index
    rng = np.random.default_rng(1234 + c)
    return {
        "random": cp.random_fr(curve, 900 + c, n),
        "one bucket": fr_arr([77] * n),                                          # one occupied bucket, the rest infinity
        "second set empty": fr_arr([int(v) for v in rng.integers(1, half + 1, n)]),   # ROW[h], h >= 1, all empty: the second level-2 set is infinity
        "top digits": fr_arr([r - 1 - int(v) for v in rng.integers(0, 50, n)]),
    }


# window bits c: 2^(c - 1) buckets, level-2 sets of C = 2^(c // 2) points, C / 8 partial sums per set after msm_wide_weigh; c = 15 is the
# smallest with more than 8 of them (16), which msm_wide_tree folds before the final kernel (and the partial sums change buffers)
@pytest.mark.parametrize("curve,log_n,c", [(0, 10, 11), (0, 12, 13), (1, 12, 12), (0, 13, 15), (2, 10, 11), (3, 12, 13), (3, 12, 12), (2, 13, 15),
                                           (3, 13, 15)])
def test_msm_wide_tail_equals_quads_and_oracle(ctx, curve, log_n, c):
    n = 1 << log_n
    try:
        ctx.set_option("msm_tail_fold", 8)
        ctx.set_option("msm_window_bits", c)
        bases = ctx.bases_from_scalars(curve, 1, cp.random_fr(curve, 800 + log_n, n))
        pts = bases.download()[0]
        for name, sc in scalar_cases(curve, n, c).items():
            exp, einf = cp.msm(curve, 1, pts, sc, chunks=4)
            assert both_tails(ctx, bases, sc, tree=c >= 15) == pt_from_limbs(curve, 1, exp, einf), (curve, log_n, name)
        bases.free()
    finally:
        for name, v in (("msm_window_bits", 0), ("msm_tail_fold", 16), ("msm_tail_quads", 1)):
            ctx.set_option(name, v)


def test_msm_wide_tail_result_at_infinity(ctx):
    """every base the same point, the scalars in pairs v, r - v: the buckets cancel in the trees and the result is the point at infinity;
    and scalars v alone over that base (every addition of the level-2 trees a doubling) against the oracle"""
    curve, n, c = 0, 1 << 10, 11
    r = CURVES[curve].r
    try:
        ctx.set_option("msm_tail_fold", 8)
        ctx.set_option("msm_window_bits", c)
        bases = ctx.bases_from_scalars(curve, 1, fr_arr([5] * n))
        pts = bases.download()[0]
        cancel = fr_arr([(v // 2) % 700 + 1 if v % 2 == 0 else r - ((v // 2) % 700 + 1) for v in range(n)])
        assert both_tails(ctx, bases, cancel) is None
        same = fr_arr([(v % 1023) + 1 for v in range(n)])
        exp, einf = cp.msm(curve, 1, pts, same, chunks=4)
        assert both_tails(ctx, bases, same) == pt_from_limbs(curve, 1, exp, einf)
        bases.free()
    finally:
        for name, v in (("msm_window_bits", 0), ("msm_tail_fold", 16), ("msm_tail_quads", 1)):
            ctx.set_option(name, v)


def test_batches_keep_their_lanes_and_a_batch_of_one_agrees(ctx, zk):
    """the wide level 2 is the lone MSM's: a batch of three members runs none of its kernels; a batch of ONE member (results through the
    array of output pointers) gives the lone MSM's point under either setting"""
    curve, n, c = 0, 1 << 12, 13
    try:
        ctx.set_option("msm_tail_fold", 8)
        ctx.set_option("msm_window_bits", c)
        bases = ctx.bases_from_scalars(curve, 1, cp.random_fr(curve, 811, n))
        sc = cp.random_fr(curve, 812, n)
        lone = both_tails(ctx, bases, sc)
        d_s = ctx.malloc(sc.nbytes)
        ctx.h2d(d_s, sc)
        L = zk.coord_limbs(curve, 1)
        d_o = [ctx.malloc(3 * L * 8) for _ in range(3)]
        for mode in (WIDE, QUADS):
            ctx.set_option("msm_tail_quads", mode)
            for members in (1, 3):
                ctx.profile_reset()
                ctx.profile(True)
                ctx.msm_batch_dev([bases] * members, [d_s] * members, d_o[:members])
                ctx.sync()
                ctx.profile(False)
                names = set(ctx.profile_dump())
                assert members == 1 or not any(k.startswith("msm_wide") for k in names), (mode, sorted(names))
                for k in range(members):
                    out = np.zeros((3, L), dtype=np.uint64)
                    ctx.d2h(out, d_o[k])
                    assert jac_to_affine_py(curve, 1, out) == lone, (mode, members, k)
        for d in [d_s] + d_o:
            ctx.free(d)
        bases.free()
    finally:
        for name, v in (("msm_window_bits", 0), ("msm_tail_fold", 16), ("msm_tail_quads", 1)):
            ctx.set_option(name, v)
