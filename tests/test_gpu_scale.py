"""zkhip_bases_scale_dev / zkhip_bases_scale_geometric: out[i] = s_i * b[offset + i] over resident points, a different full-width scalar per
point -- the scalars resident on the device, or the geometric sequence coeff * ratio^(first_exponent + i) (powers_of_tau_accumulator::transform,
accumulator.hpp:89-121; the delta^-1 scaling of crs_operations.hpp:116-123).  G1 of all four curve ids, G2 of the two pairing curves.

Inputs are P_i = a_i G (cport.batch_mul), so the expected row i is the oracle's (a_i s_i mod r) G: exact, affine limbs and infinity flags
compared directly.  The sizes sit around the boundaries the kernels have: the 64-lane wave of the ladder launch (63 / 64 / 65), 7 / 8 / 9 around
AFFINE_MAX_CHUNK, 16385 = the first size at which affine_chunk gives a lane two points to normalise with one inversion (csrc/curve.hpp), and a
run cut into launches of 64 lanes by "ec_ntt_table_lanes"."""
import ctypes

import numpy as np
import pytest

import arith_cases as ac
import cport as cp
import pasta_util as pu  # noqa: F401  (adds ids 2 and 3 to util.CURVES)
from util import CURVES, fr_arr, fr_ints, limbs

pytestmark = pytest.mark.gpu

P = ac._ptr
INVALID, RANGE = -2, -5
G1_CURVES, G2_CURVES = [0, 1, 2, 3], [0, 1]
# lambda of csrc/glv.hpp: (beta x, y) = lambda (x, y)
LAMBDA = {0: 0xac45a4010001a40200000000ffffffff,
          1: 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd,
          2: 0x397e65a7d7c1ad71aee24b27e308f0a61259527ec1d4752e619d1840af55f1b1,
          3: 0x12ccca834acdba712caad5dc57aab1b01d1f8bd237ad31491dad5ebdfdfe4ab9}


def expected(curve, group, a, s):
    """rows and flags of (a_i s_i mod r) G; rows at infinity are zero, as a download has them"""
    r = CURVES[curve].r
    pts, inf = cp.batch_mul(curve, group, fr_arr([x * y % r for x, y in zip(a, s)]))
    pts[inf != 0] = 0
    return pts, inf


def same(got, exp):
    (gp, gi), (ep, ei) = got, exp
    return (np.asarray(gi) == np.asarray(ei)).all() and (gp == ep).all()


def scale_dev(c, b, offset, n, s, flags=0):
    """zkhip_bases_scale_dev over host scalars (python ints below 2^256): upload, call, free"""
    d = c.malloc(32 * n)
    c.h2d(d, fr_arr(s))
    try:
        return c.bases_scale_dev(b, offset, n, d, flags)
    finally:
        c.free(d)


def taken(out):
    got = out.download()
    out.free()
    return got


def inputs(curve, seed, n, zero_at=5):
    a = fr_ints(cp.random_fr(curve, seed, n))
    if n > zero_at:
        a[zero_at] = 0    # an input at infinity
    return a


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 63, 64, 65, 200, 16385])
@pytest.mark.parametrize("curve", G1_CURVES)
def test_g1_sizes(ctx, curve, n):
    a, s = inputs(curve, 9100 + n, n), fr_ints(cp.random_fr(curve, 9150 + n, n))
    b = ctx.bases_from_scalars(curve, 1, fr_arr(a))
    out = scale_dev(ctx, b, 0, n, s)
    assert out.n == n and ctx.lib.zkhip_bases_size(out.h) == n
    assert same(taken(out), expected(curve, 1, a, s))
    b.free()


@pytest.mark.parametrize("n", [1, 9, 65])
@pytest.mark.parametrize("curve", G2_CURVES)
def test_g2_sizes(ctx, curve, n):
    a, s = inputs(curve, 9200 + n, n), fr_ints(cp.random_fr(curve, 9250 + n, n))
    b = ctx.bases_from_scalars(curve, 2, fr_arr(a))
    assert same(taken(scale_dev(ctx, b, 0, n, s)), expected(curve, 2, a, s))
    w = fr_ints(cp.random_fr(curve, 9260 + n, 2))
    r = CURVES[curve].r
    geo = ctx.bases_scale_geometric(b, 0, n, limbs(w[0], 4), limbs(w[1], 4), 3)
    assert same(taken(geo), expected(curve, 2, a, [w[1] * pow(w[0], 3 + i, r) % r for i in range(n)]))
    b.free()


@pytest.mark.parametrize("curve,group", [(0, 1), (2, 1), (1, 2)])
def test_several_launches(zk, curve, group):
    """option "ec_ntt_table_lanes" = 64 and 200 points: four launches, the last one partial, and the result of the default single launch"""
    n = 200
    a, s = inputs(curve, 9300, n), fr_ints(cp.random_fr(curve, 9301, n))
    c = zk.Context(0)
    try:
        b = c.bases_from_scalars(curve, group, fr_arr(a))
        c.profile(True)
        res, launches = [], []
        try:
            for lanes in (64, 0):
                c.set_option("ec_ntt_table_lanes", lanes)
                c.profile_reset()
                out = scale_dev(c, b, 0, n, s)
                launches.append(c.profile_get("bases_scale_pass")[1])
                res.append(taken(out))
        finally:
            c.set_option("ec_ntt_table_lanes", 0)
        c.profile(False)
        b.free()
    finally:
        c.close()
    assert launches == [4, 1]
    assert same(res[0], res[1]) and same(res[0], expected(curve, group, a, s))


def special_scalars(curve):
    r, lam = CURVES[curve].r, LAMBDA[curve]
    assert (lam * lam + lam + 1) % r == 0
    s = [0, 1, 2, 7, 8, 9, 15, 16, 17, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2,     # every nibble value and the recoding carry
         lam, lam + 1, lam - 1, r - lam,                                             # one GLV half zero, or flipping sign
         (1 << 128) - 1, 1 << 128, 1 << 129,
         r + 5, (1 << 256) - 1]                                                      # not canonical: taken mod r, as zkhip_msm_dev takes them
    return s + fr_ints(cp.random_fr(curve, 9400, 64))


@pytest.mark.parametrize("curve,group", [(c, 1) for c in G1_CURVES] + [(c, 2) for c in G2_CURVES])
def test_scalars_device_mode(ctx, curve, group):
    s = special_scalars(curve)
    n = len(s)
    a = fr_ints(cp.random_fr(curve, 9401, n))
    b = ctx.bases_from_scalars(curve, group, fr_arr(a))
    assert same(taken(scale_dev(ctx, b, 0, n, s)), expected(curve, group, a, s))    # expected() reduces a_i s_i mod r: non-canonical s_i included
    b.free()


@pytest.mark.parametrize("curve,group", [(c, 1) for c in G1_CURVES] + [(c, 2) for c in G2_CURVES])
def test_points(ctx, curve, group):
    """infinity among the inputs, the same point in every slot, P and -P adjacent"""
    r = CURVES[curve].r
    k = fr_ints(cp.random_fr(curve, 9500, 1))[0] | 1
    n = 66
    s = fr_ints(cp.random_fr(curve, 9501, n))
    for a in ([0 if i % 3 == 0 else k + i for i in range(n)], [k] * n, [k if i % 2 == 0 else r - k for i in range(n)], [0] * n):
        b = ctx.bases_from_scalars(curve, group, fr_arr(a))
        assert same(taken(scale_dev(ctx, b, 0, n, s)), expected(curve, group, a, s))
        assert same(taken(scale_dev(ctx, b, 0, n, [s[0]] * n)), expected(curve, group, a, [s[0]] * n))
        b.free()


@pytest.mark.parametrize("curve", G1_CURVES)
def test_geometric(ctx, curve):
    r = CURVES[curve].r
    n = 100
    a = inputs(curve, 9600, n)
    ratio, coeff = fr_ints(cp.random_fr(curve, 9601, 2))
    b = ctx.bases_from_scalars(curve, 1, fr_arr(a))

    def run(ratio, coeff, e0=0, offset=0, count=n):
        return taken(ctx.bases_scale_geometric(b, offset, count, limbs(ratio, 4), limbs(coeff, 4) if coeff is not None else None, e0))

    def exp(ratio, coeff, e0=0, offset=0, count=n):
        c = 1 if coeff is None else coeff
        return expected(curve, 1, a[offset:offset + count], [c * pow(ratio, e0 + i, r) % r for i in range(count)])    # pow(0, 0, r) = 1

    whole = run(ratio, coeff)
    assert same(whole, exp(ratio, coeff))
    assert same(run(ratio, None), exp(ratio, None))
    assert same(run(1, coeff), exp(1, coeff))                   # one scalar for every point
    got0 = run(0, coeff)                                        # s_0 = coeff, the rest zero
    assert same(got0, exp(0, coeff)) and got0[1][1:].all() and not got0[1][0]
    assert np.asarray(run(ratio, 0)[1]).all()                   # coeff = 0: all at infinity
    assert same(run(0, coeff, e0=5), exp(0, coeff, e0=5)) and same(run(ratio, coeff, e0=5), exp(ratio, coeff, e0=5))
    # slicing: rows k .. of the whole run are the run over the points from k with first_exponent = k
    k = 37
    part = run(ratio, coeff, e0=k, offset=k, count=n - k)
    assert same(part, (whole[0][k:], whole[1][k:]))
    # the largest exponents the entry takes: first_exponent + n = 2^32
    e0 = (1 << 32) - 4
    assert same(run(ratio, coeff, e0=e0, count=4), exp(ratio, coeff, e0=e0, count=4))
    b.free()


@pytest.mark.parametrize("curve,group", [(0, 1), (3, 1), (0, 2)])
def test_offset_into_a_larger_object(ctx, curve, group):
    total, off, n = 70, 3, 65
    a, s = inputs(curve, 9700, total), fr_ints(cp.random_fr(curve, 9701, n))
    b = ctx.bases_from_scalars(curve, group, fr_arr(a))
    before = b.download()
    assert same(taken(scale_dev(ctx, b, off, n, s)), expected(curve, group, a[off:off + n], s))
    after = b.download()
    assert before[0].tobytes() == after[0].tobytes() and np.asarray(before[1]).tobytes() == np.asarray(after[1]).tobytes()
    b.free()


@pytest.mark.parametrize("curve,group", [(0, 1), (2, 1), (1, 2)])
def test_window_tables(zk, curve, group):
    """with ZKHIP_SCALE_TABLES the result carries window tables as an upload would (64 points: above "msm_precompute_min"), without it none
    and an MSM over it takes the Horner path; either way the MSM equals the oracle's over the expected points"""
    n = 64
    a, s = inputs(curve, 9800, n), fr_ints(cp.random_fr(curve, 9801, n))
    e = cp.random_fr(curve, 9802, n)
    exp_pts, exp_inf = expected(curve, group, a, s)
    want = cp.msm(curve, group, exp_pts, e, inf=exp_inf)
    c = zk.Context(0)
    try:
        b = c.bases_from_scalars(curve, group, fr_arr(a))
        c.profile(True)
        for flags, builds in ((zk.zkhip.SCALE_TABLES, 1), (0, 0)):
            c.profile_reset()
            out = scale_dev(c, b, 0, n, s, flags)
            assert (c.profile_get("bases_precompute")[1] > 0) == bool(builds), flags
            geo = c.bases_scale_geometric(b, 0, n, limbs(1, 4), limbs(s[0], 4), 0, flags)
            aff, ainf = c.msm_affine(out, e)
            assert ainf == want[1] and (aff == want[0]).all(), flags
            assert same(out.download(), (exp_pts, exp_inf)) and same(geo.download(), expected(curve, group, a, [s[0]] * n))
            out.free()
            geo.free()
        c.profile(False)
        b.free()
    finally:
        c.close()


@pytest.mark.parametrize("curve", [0, 2])
def test_refusals(zk, curve):
    """every refusal with its code, *out null, no launch (the profiler has counted none), a clean device status and a context that works
    afterwards; a G2 object with a Pasta id cannot be made, so there is nothing of that kind to scale"""
    C = CURVES[curve]
    r, n = C.r, 10
    a = inputs(curve, 9900, n)
    c = zk.Context(0)
    try:
        L, h, z, u64 = c.lib, c.h, ctypes.c_size_t, ctypes.c_uint64
        b = c.bases_from_scalars(curve, 1, fr_arr(a))
        d = c.malloc(32 * n)
        s = fr_ints(cp.random_fr(curve, 9901, n))
        c.h2d(d, fr_arr(s))
        dp = ctypes.c_void_p(d)
        one, big = limbs(1, 4), limbs(r, 4)
        dev = lambda ch, bh, off, cnt, sp, fl, o: L.zkhip_bases_scale_dev(ch, bh, z(off), z(cnt), sp, fl, o)
        geo = lambda ch, bh, off, cnt, ra, co, e0, fl, o: L.zkhip_bases_scale_geometric(ch, bh, z(off), z(cnt), P(ra) if ra is not None else None,
                                                                                       P(co) if co is not None else None, u64(e0), fl, o)
        calls = [
            ("dev: null ctx", INVALID, lambda o: dev(None, b.h, 0, n, dp, 0, o)),
            ("dev: null bases", INVALID, lambda o: dev(h, None, 0, n, dp, 0, o)),
            ("dev: null scalars", INVALID, lambda o: dev(h, b.h, 0, n, None, 0, o)),
            ("dev: unknown flag", INVALID, lambda o: dev(h, b.h, 0, n, dp, 2, o)),
            ("dev: n = 0", RANGE, lambda o: dev(h, b.h, 0, 0, dp, 0, o)),
            ("dev: n = 2^31", RANGE, lambda o: dev(h, b.h, 0, 1 << 31, dp, 0, o)),
            ("dev: offset + n one past the size", RANGE, lambda o: dev(h, b.h, 1, n, dp, 0, o)),
            ("dev: offset past the size", RANGE, lambda o: dev(h, b.h, n + 1, 1, dp, 0, o)),
            ("geo: null ctx", INVALID, lambda o: geo(None, b.h, 0, n, one, None, 0, 0, o)),
            ("geo: null bases", INVALID, lambda o: geo(h, None, 0, n, one, None, 0, 0, o)),
            ("geo: null ratio", INVALID, lambda o: geo(h, b.h, 0, n, None, one, 0, 0, o)),
            ("geo: ratio = r", INVALID, lambda o: geo(h, b.h, 0, n, big, one, 0, 0, o)),
            ("geo: coeff = r", INVALID, lambda o: geo(h, b.h, 0, n, one, big, 0, 0, o)),
            ("geo: coeff = 2^256 - 1", INVALID, lambda o: geo(h, b.h, 0, n, one, limbs((1 << 256) - 1, 4), 0, 0, o)),
            ("geo: unknown flag", INVALID, lambda o: geo(h, b.h, 0, n, one, None, 0, 4, o)),
            ("geo: n = 0", RANGE, lambda o: geo(h, b.h, 0, 0, one, None, 0, 0, o)),
            ("geo: n = 2^31", RANGE, lambda o: geo(h, b.h, 0, 1 << 31, one, None, 0, 0, o)),
            ("geo: offset + n one past the size", RANGE, lambda o: geo(h, b.h, 1, n, one, None, 0, 0, o)),
            ("geo: first_exponent + n = 2^32 + 1", RANGE, lambda o: geo(h, b.h, 0, n, one, None, (1 << 32) - n + 1, 0, o)),
            ("geo: first_exponent = 2^64 - 1", RANGE, lambda o: geo(h, b.h, 0, n, one, None, (1 << 64) - 1, 0, o)),
        ]
        hdl = ctypes.c_void_p()
        c.profile(True)
        for name, code, call in calls:
            hdl.value = 1    # not a handle: the call must put null there
            assert call(ctypes.byref(hdl)) == code, name
            assert not hdl.value, name
        assert dev(h, b.h, 0, n, dp, 0, None) == INVALID and geo(h, b.h, 0, n, one, None, 0, 0, None) == INVALID
        for pasta in (2, 3):    # no G2 for the Pasta ids: such a bases object cannot exist
            hdl.value = 0
            assert L.zkhip_bases_from_scalars(h, pasta, 2, None, P(fr_arr(s)), z(n), ctypes.byref(hdl)) == INVALID and not hdl.value
        assert c.profile_get("")[1] == 0, "a refused call launched something"
        c.profile(False)
        assert c.device_status() == 0
        out = c.bases_scale_dev(b, 0, n, d)
        assert same(taken(out), expected(curve, 1, a, s))
        c.free(d)
        b.free()
    finally:
        c.close()
