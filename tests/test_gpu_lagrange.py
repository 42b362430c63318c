"""zkhip_bases_lagrange: the Lagrange basis of a range of a resident SRS, out[j] = (1/m) sum_i omega^(-i j) b[offset + i], as a new bases
object (kimchi_pedersen::params_type::add_lagrange_basis, kimchi_pedersen.hpp:92-105) -- G1 of all four curve ids, the twiddles split by the
curve's endomorphism (csrc/glv.hpp; the split itself against big integers: test_host_glv.py).

With inputs k_i G the expected rows are the oracle's inverse NTT of the k_i in the exponent (cport: zko_ntt, zko_batch_mul); with inputs of
unknown logarithm each row is the oracle's MSM of the inputs by the row omega^(-i j) / m.  Downloads (canonical affine + infinity flags)
are compared with the oracle's arrays directly."""
import ctypes

import numpy as np
import pytest

import arith_cases as ac
import cport as cp
import pasta_util as pu  # noqa: F401  (adds ids 2 and 3 to util.CURVES)
from util import CURVES, FQ_LIMBS, fr_arr, limbs, pts_arr

pytestmark = pytest.mark.gpu

P = ac._ptr
INVALID, RANGE = -2, -5


def scalars(curve, seed, m, zero_at=5):
    ks = cp.random_fr(curve, seed, m)
    if m > zero_at:
        ks[zero_at] = 0    # an input at infinity
    return ks


def expected_from_exponents(curve, ks, log_m, w):
    """rows and flags of the Lagrange basis of the points k_i G: the inverse NTT of the k_i, times G"""
    m = 1 << log_m
    e = cp.ntt(curve, ks.reshape(1, m, 4), log_m, limbs(w, 4), inverse=True)[0] if log_m else ks
    pts, inf = cp.batch_mul(curve, 1, e)
    pts[inf != 0] = 0
    return pts, inf


def same(got, exp):
    (gp, gi), (ep, ei) = got, exp
    return (np.asarray(gi) == np.asarray(ei)).all() and (gp == ep).all()


@pytest.mark.parametrize("log_m", [0, 1, 2, 3, 6, 7, 10])
@pytest.mark.parametrize("curve", [2, 3, 0, 1])
def test_definition_every_row(ctx, curve, log_m):
    """size 1 has no stage, 2 only the last stage with 1/m folded in, 64 is one wave of the multiplication pass, 128 the first size with two
    workgroups in the last stage"""
    m, w = 1 << log_m, CURVES[curve].root_of_unity(log_m)
    ks = scalars(curve, 8100 + log_m, m)
    b = ctx.bases_from_scalars(curve, 1, ks)
    out = ctx.bases_lagrange(b, 0, log_m, limbs(w, 4))
    assert out.n == m and ctx.lib.zkhip_bases_size(out.h) == m
    assert same(out.download(), expected_from_exponents(curve, ks, log_m, w))
    out.free()
    b.free()


@pytest.mark.parametrize("curve", [2, 3])
def test_sub_range_of_points_with_unknown_logarithms(ctx, curve):
    C = CURVES[curve]
    r, log_m, off = C.r, 4, 3
    m, w = 1 << log_m, C.root_of_unity(log_m)
    pts = pts_arr(curve, 1, pu.random_points(curve, 8200, off + m + 5))
    b = ctx.upload_bases(curve, 1, pts)
    out = ctx.bases_lagrange(b, off, log_m, limbs(w, 4))
    got, ginf = out.download()
    winv, minv = pow(w, -1, r), pow(m, -1, r)
    for j in range(m):
        row = fr_arr([pow(winv, i * j, r) * minv % r for i in range(m)])
        exp, einf = cp.msm(curve, 1, pts[off:off + m], row)
        assert ginf[j] == einf == 0 and (got[j] == exp).all(), j
    # the rows outside the range play no part, and b is left as it was
    after, ainf = b.download()
    assert (after == pts).all() and not ainf.any()
    other = pts.copy()
    other[:off] = pts[off + m:off + m + off]
    other[off + m:] = pts[1:6]
    b2 = ctx.upload_bases(curve, 1, other)
    out2 = ctx.bases_lagrange(b2, off, log_m, limbs(w, 4))
    assert same(out2.download(), (got, ginf))
    for x in (out, out2, b, b2):
        x.free()


@pytest.mark.parametrize("curve", [2, 3, 1])
def test_degenerate_inputs(ctx, curve):
    C = CURVES[curve]
    r, log_m = C.r, 6
    m, w = 1 << log_m, limbs(C.root_of_unity(log_m), 4)
    k = int(cp.random_fr(curve, 8300, 1)[0, 0]) | 1
    (pk,), _ = cp.batch_mul(curve, 1, fr_arr([k]))

    def run(ks):
        b = ctx.bases_from_scalars(curve, 1, fr_arr(ks))
        out = ctx.bases_lagrange(b, 0, log_m, w)
        got = out.download()
        out.free()
        b.free()
        return got

    def only(row):
        pts, inf = np.zeros((m, 2 * FQ_LIMBS[curve]), dtype=np.uint64), np.ones(m, dtype=np.uint8)
        if row is not None:
            pts[row], inf[row] = pk, 0
        return pts, inf

    # all inputs the same point: every first-stage butterfly is a doubling and a cancellation; out[0] = the point
    assert same(run([k] * m), only(0))
    assert same(run([0] * m), only(None))
    # g_i = (-1)^i P: only row m / 2 is finite, and it is P
    assert same(run([k if i % 2 == 0 else r - k for i in range(m)]), only(m // 2))


def test_several_launches_per_pass(zk):
    """option "ec_ntt_table_lanes": the multiplication pass over one table region in several launches gives the same result as in one"""
    curve, log_m = 2, 8
    m, w = 1 << log_m, CURVES[curve].root_of_unity(log_m)
    ks = scalars(curve, 8400, m)
    c = zk.Context(0)
    try:
        b = c.bases_from_scalars(curve, 1, ks)
        c.profile(True)
        res, launches = [], []
        try:
            for lanes in (64, 0):
                c.set_option("ec_ntt_table_lanes", lanes)
                c.profile_reset()
                out = c.bases_lagrange(b, 0, log_m, limbs(w, 4))
                launches.append(c.profile_get("ec_ntt_mul_pass")[1])
                res.append(out.download())
                out.free()
        finally:
            c.set_option("ec_ntt_table_lanes", 0)
        c.profile(False)
        b.free()
    finally:
        c.close()
    assert launches[0] > launches[1] > 0
    assert same(res[0], res[1]) and same(res[0], expected_from_exponents(curve, ks, log_m, w))


@pytest.mark.parametrize("curve", [2, 3])
def test_past_one_tile(ctx, curve):
    log_m = 13
    m, w = 1 << log_m, CURVES[curve].root_of_unity(log_m)
    ks = scalars(curve, 8500, m)
    b = ctx.bases_from_scalars(curve, 1, ks)
    out = ctx.bases_lagrange(b, 0, log_m, limbs(w, 4))
    assert same(out.download(), expected_from_exponents(curve, ks, log_m, w))
    out.free()
    b.free()


@pytest.mark.parametrize("curve,log_m", [(2, 15), (0, 15), (3, 17)])
def test_shared_inversion_chunks(ctx, curve, log_m):
    """ec_ntt_store_affine with more than one point per lane: 2^15 is the smallest size with two (the chunk is 1 up to 2^14 points), 2^17 has
    the full eight.  The OUTPUT exponents e_j are chosen first -- zeros at the first, the last and a middle row of a lane's chunk and over one
    whole chunk -- and the input is (NTT e) G, so the inverse transform must return e_j G, with infinity exactly at the chosen rows.  Rows are
    compared with bases_from_scalars(e), which test_gpu_msm.py::test_bases_from_scalars pins to the oracle."""
    m, w = 1 << log_m, limbs(CURVES[curve].root_of_unity(log_m), 4)
    chunk = m >> 14
    e = cp.random_fr(curve, 8900 + log_m, m)
    zero = [10 * chunk, 21 * chunk - 1, 30 * chunk + chunk // 2] + list(range(40 * chunk, 41 * chunk))
    e[zero] = 0
    ks = cp.ntt(curve, e.reshape(1, m, 4), log_m, w)[0]
    b = ctx.bases_from_scalars(curve, 1, ks)
    out = ctx.bases_lagrange(b, 0, log_m, w)
    ref = ctx.bases_from_scalars(curve, 1, e)
    (got, ginf), (exp, einf) = out.download(), ref.download()
    assert sorted(np.flatnonzero(einf).tolist()) == sorted(set(zero))
    assert (np.asarray(ginf) == np.asarray(einf)).all() and (got == exp).all()
    for x in (out, ref, b):
        x.free()


@pytest.mark.parametrize("curve", [2, 3])
def test_result_is_a_first_class_bases_object(zk, curve):
    """window tables as an upload would build them under the context's options: the MSM over the object equals the oracle's MSM over its
    downloaded points, and MSM(lagrange, e) = MSM(g[0 .. m), inverse NTT of e) -- what commitment_evaluations rests on"""
    log_m = 10
    m, w = 1 << log_m, limbs(CURVES[curve].root_of_unity(log_m), 4)
    ks = scalars(curve, 8600, m)
    g_pts, g_inf = cp.batch_mul(curve, 1, ks)
    e = cp.random_fr(curve, 8601, m)
    coeffs = cp.ntt(curve, e.reshape(1, m, 4), log_m, w, inverse=True)[0]
    commit = cp.msm(curve, 1, g_pts, coeffs, inf=g_inf)
    c = zk.Context(0)
    try:
        b = c.bases_from_scalars(curve, 1, ks)
        try:
            for pre in (1, 0):
                for bits in (0, 9):
                    c.set_option("msm_precompute", pre)
                    c.set_option("msm_window_bits", bits)
                    lagr = c.bases_lagrange(b, 0, log_m, w)
                    pts, inf = lagr.download()
                    aff, ainf = c.msm_affine(lagr, e)
                    exp, einf = cp.msm(curve, 1, pts, e, inf=inf)
                    assert ainf == einf and (aff == exp).all(), (pre, bits)
                    assert ainf == commit[1] and (aff == commit[0]).all(), (pre, bits)
                    lagr.free()
        finally:
            c.set_option("msm_precompute", 1)
            c.set_option("msm_window_bits", 0)
        b.free()
    finally:
        c.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_agrees_with_ec_ntt_dev(ctx, curve):
    """the two boundary forms around one stage network: canonical Jacobians in place (zkhip_ec_ntt_dev, inverse) and bases objects"""
    log_m = 8
    m, w, L = 1 << log_m, limbs(CURVES[curve].root_of_unity(log_m), 4), FQ_LIMBS[curve]
    ks = scalars(curve, 8700, m)
    b = ctx.bases_from_scalars(curve, 1, ks)
    pts, inf = b.download()
    out = ctx.bases_lagrange(b, 0, log_m, w)
    got, ginf = out.download()
    jac = np.zeros((m, 3 * L), dtype=np.uint64)
    jac[:, :2 * L] = pts
    jac[:, 2 * L] = 1
    jac[inf != 0] = 0
    d = ctx.malloc(jac.nbytes)
    ctx.h2d(d, jac)
    ctx.ec_ntt_dev(curve, 1, d, log_m, w, inverse=True)
    ctx.d2h(jac, d)
    ctx.free(d)
    for j in range(m):
        exp, einf = cp.jac_to_affine(curve, 1, jac[j])
        assert ginf[j] == einf and (einf or (got[j] == exp).all()), j
    out.free()
    b.free()


@pytest.mark.parametrize("curve", [2, 3, 0])
def test_refusals(zk, curve):
    """every refusal with its code, *out null, no launch (the profiler has counted none), a clean device status and a context that works
    afterwards; zkhip_ec_ntt_dev still refuses the two Pasta ids"""
    C = CURVES[curve]
    log_m = 3
    m = 1 << log_m
    ks = scalars(curve, 8800, m + 2)
    c = zk.Context(0)
    try:
        L, h, z = c.lib, c.h, ctypes.c_size_t
        b = c.bases_from_scalars(curve, 1, ks)
        g2 = c.bases_from_scalars(curve, 2, ks) if curve in (0, 1) else None
        d = c.malloc(1 << 12)
        c.h2d(d, np.zeros(1 << 9, dtype=np.uint64))
        root = lambda k: limbs(C.root_of_unity(k), 4)
        w = root(log_m)
        hdl = ctypes.c_void_p()
        lag = lambda ctx_h, bh, off, lg, om, out: L.zkhip_bases_lagrange(ctx_h, bh, z(off), z(lg), P(om) if om is not None else None, out)
        calls = [
            ("omega of order 2m", INVALID, lambda o: lag(h, b.h, 0, log_m, root(log_m + 1), o)),
            ("omega of order m/2", INVALID, lambda o: lag(h, b.h, 0, log_m, root(log_m - 1), o)),
            ("omega = 1", INVALID, lambda o: lag(h, b.h, 0, log_m, limbs(1, 4), o)),
            ("omega = r", INVALID, lambda o: lag(h, b.h, 0, log_m, limbs(C.r, 4), o)),
            ("omega = r + w", INVALID, lambda o: lag(h, b.h, 0, log_m, limbs(C.r + C.root_of_unity(log_m), 4), o)),
            ("log_m = 27", RANGE, lambda o: lag(h, b.h, 0, 27, root(27), o)),
            ("offset + m one past the size", RANGE, lambda o: lag(h, b.h, 3, log_m, w, o)),
            ("offset past the size", RANGE, lambda o: lag(h, b.h, m + 3, 0, limbs(1, 4), o)),
            ("null ctx", INVALID, lambda o: lag(None, b.h, 0, log_m, w, o)),
            ("null bases", INVALID, lambda o: lag(h, None, 0, log_m, w, o)),
            ("null omega", INVALID, lambda o: lag(h, b.h, 0, log_m, None, o)),
        ]
        if g2 is not None:
            calls.append(("G2 bases", INVALID, lambda o: lag(h, g2.h, 0, log_m, w, o)))
        c.profile(True)
        for name, code, call in calls:
            hdl.value = 1    # not a handle: the call must put null there
            assert call(ctypes.byref(hdl)) == code, name
            assert not hdl.value, name
        assert lag(h, b.h, 0, log_m, w, None) == INVALID
        if curve in (2, 3):    # the Jacobian entry point keeps to the pairing curves
            for group in (1, 2):
                assert L.zkhip_ec_ntt_dev(h, curve, group, ctypes.c_void_p(d), z(2), P(root(2)), 0) == INVALID
        assert c.profile_get("")[1] == 0, "a refused call launched something"
        c.profile(False)
        assert c.device_status() == 0
        out = c.bases_lagrange(b, 2, log_m, w)
        assert same(out.download(), expected_from_exponents(curve, ks[2:], log_m, C.root_of_unity(log_m)))
        out.free()
        c.free(d)
        if g2 is not None:
            g2.free()
        b.free()
    finally:
        c.close()
