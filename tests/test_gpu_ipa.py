"""The inner-product-argument primitives of include/zkhip.h on the GPU -- zkhip_bases_fold, zkhip_fr_inner_product_dev,
zkhip_fr_powers_lincomb_dev, zkhip_fr_challenge_products_dev -- against the Python model (tests/ipa_model.py, pyoracle's group law),
on Pallas and Vesta (ids 2, 3) and, where a bullet says so, BLS12-381 and BN254 (ids 0, 1: the 14-limb coordinates are where registers
run out)."""
import ctypes
import random

import numpy as np
import pytest

import ipa_model as im
import pasta_util as pu  # registers ids 2 and 3 in util.CURVES
import util
from util import fr_arr, fr_ints, limbs, pt_from_limbs, pts_arr

pytestmark = pytest.mark.gpu

INVALID, RANGE = -2, -5
HI = 520          # offset of the `hi` range in the fixture's bases; `lo` starts at 0
NPTS = HI + 520
# rows (relative to the start of a range) the fixture makes special
LO_INF, HI_INF, BOTH_INF = 1, 2, 5
DBL2, NEG2 = 7, 8       # lo = 2 hi, lo = -2 hi: with c = 2 the last addition is a doubling / cancels
DBLC, NEGC = 9, 10      # the same for the fixture's random c


class World:
    """1040 points of one curve (python and resident, with window tables), a random scalar c and c * hi[i] for the first 500 rows"""

    def __init__(self, ctx, zk, curve, n_mul):
        C = util.CURVES[curve]
        self.curve, self.G, self.r = curve, C.g1, C.r
        rng = random.Random(1000 + curve)
        G, r = self.G, self.r
        pts = G.batch_mul_gen([rng.randrange(1, r) for _ in range(NPTS)])
        self.c = rng.randrange(r >> 1, r)
        for i in (LO_INF, BOTH_INF, HI + HI_INF, HI + BOTH_INF):
            pts[i] = None
        pts[DBL2] = G.mul(pts[HI + DBL2], 2)
        pts[NEG2] = G.neg(G.mul(pts[HI + NEG2], 2))
        self.c_hi = [G.mul(pts[HI + i], self.c) for i in range(n_mul)]
        if n_mul > NEGC:
            pts[DBLC] = self.c_hi[DBLC]
            pts[NEGC] = G.neg(self.c_hi[NEGC])
        self.pts = pts
        inf = np.array([p is None for p in pts], dtype=np.uint8)
        self.bases = ctx.upload_bases(curve, zk.G1, pts_arr(curve, 1, pts), inf)

    def expect(self, c, lo, hi, half):
        G, r, p = self.G, self.r, self.pts
        out = []
        for i in range(half):
            h, l = p[hi + i], p[lo + i]
            if c == 0:
                m = None
            elif c == 1:
                m = h
            elif c == 2:
                m = G.add(h, h)
            elif c == r - 1:
                m = G.neg(h)
            else:
                assert c == self.c and hi == HI
                m = self.c_hi[i]
            out.append(G.add(m, l))
        return out

    def fold(self, ctx, c, lo, hi, half):
        out = ctx.bases_fold(self.bases, lo, hi, half, limbs(c, 4))
        xy, inf = out.download()
        out.free()
        return [pt_from_limbs(self.curve, 1, xy[i], inf[i]) for i in range(half)]


_WORLDS = {}


@pytest.fixture
def world(ctx, zk, request):
    curve = request.param
    if curve not in _WORLDS:
        _WORLDS[curve] = World(ctx, zk, curve, 500 if curve >= 2 else 0)
    return _WORLDS[curve]


@pytest.mark.parametrize("half", [1, 2, 3, 63, 64, 65, 500, 513])
@pytest.mark.parametrize("world", [2, 3], indirect=True)
def test_bases_fold_matches_model(ctx, world, half):
    """out[i] = c hi[i] + lo[i] for c in {0, 1, 2, r - 1, random}; rows with hi, lo or both at infinity, rows whose last addition is a doubling
    or cancels (c = 2 and the random c); 513 crosses a workgroup of 64 lanes x 8 points, were the chunk 8 (at these sizes it is 1)"""
    w = world
    for c in (0, 1, 2, w.r - 1) + ((w.c,) if half <= 500 else ()):
        got = w.fold(ctx, c, 0, HI, half)
        assert got == w.expect(c, 0, HI, half), (w.curve, half, hex(c))
    if half > NEGC:
        assert w.fold(ctx, 2, 0, HI, half)[NEG2] is None and w.fold(ctx, w.c, 0, HI, min(half, 500))[NEGC] is None


@pytest.mark.parametrize("half", [3, 65])
@pytest.mark.parametrize("world", [0, 1], indirect=True)
def test_bases_fold_on_the_pairing_curves(ctx, world, half):
    """ids 0 and 1 (BLS12-381: 14-limb coordinates) with the special scalars"""
    w = world
    for c in (0, 1, 2, w.r - 1):
        assert w.fold(ctx, c, 0, HI, half) == w.expect(c, 0, HI, half), (w.curve, half, hex(c))
    assert w.fold(ctx, 1, HI, HI, half) == [w.G.add(p, p) for p in w.pts[HI:HI + half]]
    assert w.fold(ctx, w.r - 1, HI, HI, half) == [None] * half


@pytest.mark.parametrize("world", [2, 3], indirect=True)
def test_bases_fold_coinciding_and_overlapping_ranges(ctx, world):
    w = world
    G = w.G
    assert w.fold(ctx, 1, HI, HI, 65) == [G.add(p, p) for p in w.pts[HI:HI + 65]]        # every lane doubles
    assert w.fold(ctx, w.r - 1, HI, HI, 65) == [None] * 65                              # every result is infinity
    assert w.fold(ctx, 2, 0, 3, 10) == w.expect(2, 0, 3, 10)                            # overlapping ranges
    assert w.fold(ctx, 2, 4, 0, 10) == w.expect(2, 4, 0, 10)
    assert w.fold(ctx, w.c, NPTS - 1, HI, 1) == [G.add(w.c_hi[0], w.pts[NPTS - 1])]     # the last row of the object
    empty = ctx.bases_fold(w.bases, 0, HI, 0, limbs(3, 4))
    assert empty.n == 0 and ctx.lib.zkhip_bases_size(empty.h) == 0
    empty.free()
    assert ctx.device_status() == 0


@pytest.mark.parametrize("half", [1 << 15, 1 << 16, (1 << 17) + 3])
def test_bases_fold_many_workgroups(ctx, zk, half):
    """Sizes at which the grid has many workgroups and a lane takes 2, 4 and 8 points (the last with a partial chunk).  The model would
    take minutes: for random r_i the library's own MSM (pinned to the oracle elsewhere) must give MSM(out, r) = c MSM(hi, r) + MSM(lo, r)."""
    curve = pu.PALLAS_ID
    G, r = pu.PALLAS.g1, pu.PALLAS.r
    rng = np.random.default_rng(half)
    ks = rng.integers(0, 1 << 62, size=(2 * half, 4), dtype=np.uint64)
    ks[:, 3] >>= np.uint64(4)
    ks[[5, half + 9, 77, half + 77]] = 0                      # points at infinity in lo, in hi and in both
    bases = ctx.bases_from_scalars(curve, zk.G1, ks)
    c = random.Random(half).randrange(r >> 1, r)
    out = ctx.bases_fold(bases, 0, half, half, limbs(c, 4))
    rs = rng.integers(0, 1 << 62, size=(half, 4), dtype=np.uint64)
    rs[:, 3] >>= np.uint64(4)
    aff = lambda a: pt_from_limbs(curve, 1, a[0], a[1])
    got = aff(ctx.msm_affine(out, rs))
    lo, hi = aff(ctx.msm_affine(bases, rs, 0, half)), aff(ctx.msm_affine(bases, rs, half, half))
    assert got is not None and got == G.add(G.mul(hi, c), lo)
    xy, inf = out.download(0, 100)
    assert list(np.nonzero(inf)[0]) == [77] and not xy[77].any()
    out.free()
    bases.free()
    assert ctx.device_status() == 0


def _dev(ctx, arr):
    d = ctx.malloc(max(32, arr.nbytes))
    if arr.nbytes:
        ctx.h2d(d, arr)
    return d


@pytest.mark.parametrize("curve", [0, 1, 2, 3])
def test_fr_inner_product(ctx, curve):
    r = util.CURVES[curve].r
    rng = random.Random(curve)
    nmax = (1 << 16) + 3
    a, b = [rng.randrange(r) for _ in range(nmax)], [rng.randrange(r) for _ in range(nmax)]
    top = [r - 1] * nmax
    d_a, d_b, d_top, d_out = _dev(ctx, fr_arr(a)), _dev(ctx, fr_arr(b)), _dev(ctx, fr_arr(top)), ctx.malloc(64)
    out = np.zeros((2, 4), dtype=np.uint64)
    for n in [0, 1, 63, 64, 65, 4097, nmax]:
        ctx.fr_inner_product_dev(curve, d_a, d_b, n, d_out)
        ctx.fr_inner_product_dev(curve, d_top, d_a, n, d_out + 32)
        ctx.d2h(out, d_out)
        assert fr_ints(out) == [im.inner_product(a[:n], b[:n], r), im.inner_product(top[:n], a[:n], r)], (curve, n)
    ctx.fr_inner_product_dev(curve, d_top, d_top, nmax, d_out)
    ctx.fr_inner_product_dev(curve, 0, 0, 0, d_out + 32)     # nothing to read: the pointers may be null
    ctx.d2h(out, d_out)
    assert fr_ints(out) == [nmax % r, 0]
    for d in (d_a, d_b, d_top, d_out):
        ctx.free(d)


@pytest.mark.parametrize("curve", [0, 2, 3])
def test_fr_powers_lincomb(ctx, curve):
    r = util.CURVES[curve].r
    rng = random.Random(10 + curve)
    x, y = rng.randrange(2, r), rng.randrange(2, r)
    d_out = ctx.malloc(8300 * 32)
    for points in ([x], [0], [1], [0, x], [r - 1, y], [1, x, 0], [x, y, x]):
        scales = [rng.randrange(r) for _ in points]
        for n in (1, 8, 1000, 8300):                        # 8300: a second workgroup of 256 lanes x 32 exponents
            ctx.fr_powers_lincomb_dev(curve, fr_arr(points), fr_arr(scales), d_out, n)
            got = np.zeros((n, 4), dtype=np.uint64)
            ctx.d2h(got, d_out)
            assert fr_ints(got) == im.powers_lincomb(points, scales, n, r), (curve, points, n)
    ctx.fr_powers_lincomb_dev(curve, np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64), d_out, 8)
    got = np.ones((8, 4), dtype=np.uint64)
    ctx.d2h(got, d_out)
    assert not got.any()                                    # the empty sum
    ctx.free(d_out)


@pytest.mark.parametrize("curve", [1, 2, 3])
@pytest.mark.parametrize("rounds", [0, 1, 5, 12])
def test_fr_challenge_products(ctx, curve, rounds):
    r = util.CURVES[curve].r
    rng = random.Random(20 + curve + rounds)
    chals = [rng.randrange(r) for _ in range(rounds)]
    if rounds == 5:
        chals[2] = r - 1
    d_out = ctx.malloc(32 << rounds)
    ctx.fr_challenge_products_dev(curve, fr_arr(chals) if rounds else np.zeros((0, 4), dtype=np.uint64), d_out)
    got = np.zeros((1 << rounds, 4), dtype=np.uint64)
    ctx.d2h(got, d_out)
    assert fr_ints(got) == im.b_poly_coefficients(chals, r)
    ctx.free(d_out)


@pytest.mark.parametrize("world", [2], indirect=True)
def test_documented_error_returns(ctx, zk, world):
    lib, h, b = ctx.lib, ctx.h, world.bases.h
    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    c = limbs(3, 4)
    cp = c.ctypes.data_as(vp)
    out = vp()
    fold = lambda ctx_h, bases, lo, hi, half, cptr, o: lib.zkhip_bases_fold(ctx_h, bases, sz(lo), sz(hi), sz(half), cptr, o)
    ok = ctypes.byref(out)
    assert fold(None, b, 0, HI, 4, cp, ok) == INVALID
    assert fold(h, None, 0, HI, 4, cp, ok) == INVALID
    assert fold(h, b, 0, HI, 4, None, ok) == INVALID
    assert fold(h, b, 0, HI, 4, cp, None) == INVALID
    for bad in (world.r, (1 << 256) - 1):                   # c is not a canonical Fr element
        assert fold(h, b, 0, HI, 4, limbs(bad, 4).ctypes.data_as(vp), ok) == INVALID
    g2 = ctx.bases_from_scalars(zk.BLS12_381, zk.G2, fr_arr([1, 2, 3, 4]))
    assert fold(h, g2.h, 0, 2, 2, cp, ok) == INVALID         # ZKHIP_G2
    g2.free()
    for lo, hi, half in ((NPTS - 3, 0, 4), (0, NPTS - 3, 4), (NPTS + 1, 0, 0), (0, NPTS + 1, 0), (0, 0, 1 << 40), (1 << 63, 0, 1 << 63)):
        assert fold(h, b, lo, hi, half, cp, ok) == RANGE, (lo, hi, half)
    assert not out.value                                     # no object came out of a refused call
    d = ctx.malloc(4096)
    dp = vp(d)
    ip = lambda ctx_h, curve, a, bb, n, o: lib.zkhip_fr_inner_product_dev(ctx_h, curve, a, bb, sz(n), o)
    assert ip(None, 2, dp, dp, 4, dp) == INVALID
    assert ip(h, 4, dp, dp, 4, dp) == INVALID and ip(h, -1, dp, dp, 4, dp) == INVALID
    assert ip(h, 2, None, dp, 4, dp) == INVALID and ip(h, 2, dp, None, 4, dp) == INVALID and ip(h, 2, dp, dp, 4, None) == INVALID
    assert ip(h, 2, dp, dp, 1 << 39, dp) == RANGE
    pw = lambda ctx_h, curve, p, s, k, o, n: lib.zkhip_fr_powers_lincomb_dev(ctx_h, curve, p, s, sz(k), o, sz(n))
    assert pw(None, 2, cp, cp, 1, dp, 4) == INVALID and pw(h, 7, cp, cp, 1, dp, 4) == INVALID
    assert pw(h, 2, None, cp, 1, dp, 4) == INVALID and pw(h, 2, cp, None, 1, dp, 4) == INVALID and pw(h, 2, cp, cp, 1, None, 4) == INVALID
    assert pw(h, 2, cp, cp, 65536, dp, 4) == RANGE and pw(h, 2, cp, cp, 1, dp, 1 << 39) == RANGE
    ch = lambda ctx_h, curve, p, k, o: lib.zkhip_fr_challenge_products_dev(ctx_h, curve, p, sz(k), o)
    assert ch(None, 2, cp, 1, dp) == INVALID and ch(h, 9, cp, 1, dp) == INVALID
    assert ch(h, 2, None, 1, dp) == INVALID and ch(h, 2, cp, 1, None) == INVALID
    assert ch(h, 2, cp, 32, dp) == RANGE
    ctx.free(d)
    assert ctx.device_status() == 0
