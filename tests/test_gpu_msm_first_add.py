"""The first real addition of a bucket runs as affine + affine (msm_bucket_acc.hpp, the per-lane `fresh` flag; curve.hpp xyzz_add_affine):
G1 MSMs on the four curves, window tables on and off, against the oracle -- small windows and tiny sizes, where the buckets of ONE wave
hold 0, 1, 2 and 3 or more entries (the fresh branch is mixed inside the wave), and crafted buckets whose second entry doubles the first,
cancels it (a new first entry and a fresh addition follow), or is the point at infinity.  One G2 case: the lane-pair kernel keeps the
general path.  Bit-exact (integer)."""
import itertools

import numpy as np
import pytest

import cport as cp
import pasta_util  # noqa: F401  (ids 2 and 3 in util.CURVES)
import pyoracle as po
from test_gpu_msm import gpu_affine
from util import CURVES, fr_arr, pt_from_limbs, pts_arr

pytestmark = pytest.mark.gpu
G1_CURVES = (0, 1, 2, 3)


def _restore(ctx):
    ctx.set_option("msm_precompute", 1)
    ctx.set_option("msm_window_bits", 0)


@pytest.mark.parametrize("tables", [1, 0])
@pytest.mark.parametrize("curve", G1_CURVES)
def test_small_windows_mix_the_fresh_branch_in_one_wave(ctx, curve, tables):
    sizes = (1, 2, 3, 65, 300)
    pts, _ = cp.batch_mul(curve, 1, cp.random_fr(curve, 810 + curve, max(sizes)))
    want = {}
    for n in sizes:
        sc = cp.random_fr(curve, 820 + n, n)
        exp, einf = cp.msm(curve, 1, pts[:n], sc, chunks=2)
        want[n] = (sc, pt_from_limbs(curve, 1, exp, einf))
    try:
        ctx.set_option("msm_precompute", tables)
        for c in (4, 7):
            ctx.set_option("msm_window_bits", c)
            b = ctx.upload_bases(curve, 1, pts)
            for n in sizes:
                sc, exp = want[n]
                assert gpu_affine(ctx, b, sc, n=n) == exp, (curve, tables, c, n)
            b.free()
    finally:
        _restore(ctx)


def _crafted(curve):
    """(points, scalars): scalar v < 2^6 puts a point into bucket v of window 0 at 7 window bits, so the points of one scalar are the entries
    of one bucket.  A bucket's entries are listed in every order, so whichever order the sort leaves them in, some bucket meets each case."""
    G = CURVES[curve].g1
    raw, _ = cp.batch_mul(curve, 1, cp.random_fr(curve, 830 + curve, 4))
    P, Q, R, S = (pt_from_limbs(curve, 1, raw[i]) for i in range(4))
    N = G.neg(P)
    buckets = [[P, P], [P, P, Q], [Q, P, P], [P, N], [P, N, Q], [Q, N, P], [N, P, Q, R, S]]
    buckets += [list(o) for o in itertools.permutations([P, N, Q, R])]       # cancellation, a new first entry, a fresh addition again
    buckets += [list(o) for o in itertools.permutations([P, P, Q])]          # doubling on the fresh path, then a general addition
    buckets += [[None, P], [P, None], [None, P, Q], [P, None, Q], [P, Q, None], [None, None, P, P], [None]]  # infinity bases
    assert len(buckets) < 63
    pts, sc = [], []
    for v, entries in enumerate(buckets, start=1):
        pts += entries
        sc += [v] * len(entries)
    return pts, sc


@pytest.mark.parametrize("tables", [1, 0])
@pytest.mark.parametrize("curve", G1_CURVES)
def test_crafted_buckets_double_cancel_and_skip_infinity(ctx, curve, tables):
    pts, sc = _crafted(curve)
    exp = po.msm_naive(CURVES[curve].g1, pts, sc)
    arr = pts_arr(curve, 1, pts)
    infs = np.array([1 if p is None else 0 for p in pts], dtype=np.uint8)
    try:
        ctx.set_option("msm_precompute", tables)
        for c in (7, 0):  # one bucket per scalar value; the default window
            ctx.set_option("msm_window_bits", c)
            b = ctx.upload_bases(curve, 1, arr, infs)
            assert gpu_affine(ctx, b, fr_arr(sc)) == exp, (curve, tables, c)
            b.free()
    finally:
        _restore(ctx)


@pytest.mark.parametrize("curve", G1_CURVES)
def test_4096_points_at_the_default_options(ctx, curve):
    n = 4096
    b = ctx.bases_from_scalars(curve, 1, cp.random_fr(curve, 840 + curve, n))
    pts, _ = b.download()
    sc = cp.random_fr(curve, 850 + curve, n)
    exp, einf = cp.msm(curve, 1, pts, sc, chunks=cp.num_threads())
    assert gpu_affine(ctx, b, sc) == pt_from_limbs(curve, 1, exp, einf)
    b.free()


def test_g2_lane_pairs_keep_the_general_path(ctx):
    n = 200
    pts, _ = cp.batch_mul(0, 2, cp.random_fr(0, 860, n))
    sc = cp.random_fr(0, 861, n)
    sc[:8] = fr_arr([3, 3, 5, 5, 5, 9, 0, 1])  # buckets with one, two and three entries
    exp, einf = cp.msm(0, 2, pts, sc, chunks=2)
    try:
        for c in (7, 0):
            ctx.set_option("msm_window_bits", c)
            b = ctx.upload_bases(0, 2, pts)
            assert gpu_affine(ctx, b, sc) == pt_from_limbs(0, 2, exp, einf), c
            b.free()
    finally:
        _restore(ctx)
