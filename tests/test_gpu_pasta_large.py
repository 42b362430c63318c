"""Pallas (id 2) and Vesta (id 3) kernels at the shapes where they change: more than one workgroup, sort tile and pass, split buckets, the
two-level tail on every lane shape, the cross-workgroup scan of the grand products, the generator fold with 2, 4 and 8 points per lane.
Every result is compared bit for bit with the C++ oracle (oracle/cport.py), which tests/test_oracle_pasta.py pins to the big-integer model
for both ids.  Where a case names a path, the launch labels of the profile (and the planner's thresholds, restated here) say that it ran:
a moved threshold fails the test instead of shrinking what it covers.

The curve-generic tests of test_gpu_msm.py, test_gpu_msm_wide.py, test_gpu_ntt.py and test_gpu_poly.py carry ids 2 and 3 in their own
parametrisations; this file holds the shapes that differ."""
import ctypes

import numpy as np
import pytest

import cport as cp
import pasta_util as pu
from util import CURVES, fr_arr, fr_ints, jac_to_affine_py, limbs, pt_from_limbs

pytestmark = pytest.mark.gpu
IDS = [pu.PALLAS_ID, pu.VESTA_ID]

# thresholds of the library restated (csrc/msm_core.hpp, perm.hip, ipa.hip): the tests assert against the profile that they still hold
MSM_LARGE_CHUNK = 4096
MSM_TAIL_THREADS = 256
MSM_WIDE_WAVES = 8
PERM_THREADS, PERM_CHUNK = 256, 8
FOLD_MAX_CHUNK, FOLD_TARGET_LANES = 8, 16384
MSM_OPTIONS = (("msm_precompute", 1), ("msm_window_bits", 0), ("msm_sets", 0), ("msm_sort_tile_log", 14), ("msm_segment_log", -1), ("msm_tail_fold", 16),
               ("msm_fold_run", 0), ("msm_tail_fold_g2", 1), ("msm_tail_quads", 1))


def reset_msm_options(ctx):
    for name, v in MSM_OPTIONS:
        ctx.set_option(name, v)


def profiled(ctx, call):
    """call() with the profiler on -> (its result, the set of launch labels)"""
    ctx.profile_reset()
    ctx.profile(True)
    try:
        out = call()
        ctx.sync()
    finally:
        ctx.profile(False)
    return out, set(ctx.profile_dump())


def affine(ctx, curve, jac):
    """Jacobian limbs -> python affine point by big integers, and the same through the device conversion"""
    P = jac_to_affine_py(curve, 1, jac)
    dev_aff, dev_inf = ctx.jacobian_to_affine(curve, 1, jac)
    assert pt_from_limbs(curve, 1, dev_aff, dev_inf) == P
    return P


def oracle_msm(curve, pts, sc, inf=None):
    exp, einf = cp.msm(curve, 1, pts, sc, inf=inf, chunks=4)
    return pt_from_limbs(curve, 1, exp, einf)


# ---- MSM ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", IDS)
def test_msm_random_scalars_past_one_sort_tile(ctx, curve):
    """uploaded bases, n = 4097 (one point past 2^12), 16385 (one past the 2^14-entry sort tile) and 20000, and a sub-range that starts and
    ends inside tiles"""
    nmax = 20000
    pts, _ = cp.batch_mul(curve, 1, cp.random_fr(curve, 3100, nmax))
    bases = ctx.upload_bases(curve, 1, pts)
    try:
        for n in (4097, 16385, 20000):
            sc = cp.random_fr(curve, 3200 + n, n)
            assert affine(ctx, curve, ctx.msm(bases, sc, n=n)) == oracle_msm(curve, pts[:n], sc), (curve, n)
        sc = cp.random_fr(curve, 3300, 9001)
        assert affine(ctx, curve, ctx.msm(bases, sc, offset=5003, n=9001)) == oracle_msm(curve, pts[5003:14004], sc)
    finally:
        bases.free()


@pytest.mark.parametrize("curve", IDS)
def test_msm_skewed_scalars_split_buckets(ctx, curve):
    """three quarters of 9000 scalars equal: in every window one bucket holds 6750 entries, more than MSM_LARGE_CHUNK, and is cut into tasks
    (msm_plan_large, msm_bucket_large) whose partial sums are combined and merged (msm_bucket_merge); a second skew towards r - 1 (the top
    window's largest digit, the tiny range above 2^254 next to it)"""
    n = 9000
    r = CURVES[curve].r
    bases = ctx.bases_from_scalars(curve, 1, cp.random_fr(curve, 21, n))
    pts, _ = bases.download()
    try:
        for hot in (None, r - 1, (1 << 254) + 5):
            sc = cp.random_fr(curve, 22, n)
            sc[: (3 * n) // 4] = sc[0] if hot is None else limbs(hot, 4)
            assert (3 * n) // 4 > MSM_LARGE_CHUNK
            jac, names = profiled(ctx, lambda: ctx.msm(bases, sc))
            assert {"msm_plan_large", "msm_bucket_large", "msm_bucket_merge", "msm_bucket_acc"} <= names, sorted(names)
            assert affine(ctx, curve, jac) == oracle_msm(curve, pts, sc), (curve, hot)
        assert ctx.device_status() == 0
    finally:
        bases.free()


@pytest.mark.parametrize("curve", IDS)
def test_msm_random_configurations(ctx, curve):
    """the loop of test_gpu_msm.py::test_msm_random_configurations (window size, bucket sets, sort tile, tail segment, tables on / off, two-level
    tail threshold and run, sub-range) at n = 3000 over a Pasta id"""
    rng = np.random.default_rng(2024 + curve)
    n = 3000
    pts, _ = cp.batch_mul(curve, 1, cp.random_fr(curve, 300 + n, n))
    sc = cp.random_fr(curve, 301 + n, n)
    sc[::9] = 0
    sc[1::17] = fr_arr([1])[0]
    sc[2::19] = fr_arr([CURVES[curve].r - 1])[0]
    try:
        for _ in range(10):
            c = int(rng.integers(2, 22))
            tables = bool(rng.integers(0, 4))
            ctx.set_option("msm_precompute", 1 if tables else 0)
            ctx.set_option("msm_window_bits", c)
            b = ctx.upload_bases(curve, 1, pts)
            ctx.set_option("msm_sets", int(rng.integers(0, 9)))
            ctx.set_option("msm_sort_tile_log", int(rng.choice([12, 14])))
            ctx.set_option("msm_segment_log", int(rng.integers(-1, 6)))
            ctx.set_option("msm_tail_fold", int(rng.choice([0, 8, 12, 16])))
            ctx.set_option("msm_fold_run", int(rng.choice([0, 1, 2, 4, 8, 16])))
            ctx.set_option("msm_tail_quads", int(rng.integers(0, 3)))
            lo = int(rng.integers(0, n // 2))
            cnt = int(rng.integers(1, n - lo + 1))
            exp, einf = cp.msm(curve, 1, pts[lo:lo + cnt], sc[lo:lo + cnt], chunks=4)
            got, ginf = ctx.msm_affine(b, sc[lo:lo + cnt], lo, cnt)
            assert ginf == einf and (got == exp).all(), (curve, c, tables, lo, cnt)
            b.free()
    finally:
        reset_msm_options(ctx)


# ---- the two-level tail ------------------------------------------------------------------------------------------------------------------------
def fold_plan(c, fold, run_opt, quads):
    """msm_fold_applies / msm_fold_geom / msm_tail_wide_applies of csrc/msm_core.hpp for a lone G1 MSM with window tables of c bits (2^(c - 1)
    buckets in its one set) -> (two-level tail taken, wide level 2 taken, msm_wide_tree needed)"""
    B = 1 << (c - 1)
    if fold <= 0 or B < (1 << fold):
        return False, False, False
    lb = (B - 1).bit_length()
    log_c = (lb + 1) // 2
    C, R = 1 << log_c, B >> log_c
    run = run_opt if run_opt > 0 else (8 if B >= (1 << 18) else 4)
    run = max(1, min(run, R))
    m_row, m_col = C // run, R // run
    sa = MSM_TAIL_THREADS
    applies = m_col >= 1 and m_row <= sa and m_col <= sa and B >= sa * run and m_row * run == C and m_col * run == R
    wide = applies and quads == 1 and C >= MSM_WIDE_WAVES
    return applies, wide, wide and C // MSM_WIDE_WAVES > MSM_WIDE_WAVES


def tail_grid(ctx, bases, sc, c, settings, want):
    """the MSM under every (msm_tail_fold, msm_fold_run, msm_tail_quads) of `settings`: each result is `want`, each profile shows the kernels
    fold_plan predicts; -> the set of (folded, wide, tree) plans seen"""
    seen = set()
    curve = bases.curve
    for fold, run, quads in settings:
        ctx.set_option("msm_tail_fold", fold)
        ctx.set_option("msm_fold_run", run)
        ctx.set_option("msm_tail_quads", quads)
        jac, names = profiled(ctx, lambda: ctx.msm(bases, sc))
        folded, wide, tree = fold_plan(c, fold, run, quads)
        key = (c, fold, run, quads, sorted(n_ for n_ in names if n_.startswith("msm_")))
        assert ("msm_fold" in names) == folded, key
        assert ("msm_wide_weigh" in names) == ("msm_wide_final" in names) == wide, key
        assert ("msm_wide_tree" in names) == tree, key
        assert affine(ctx, curve, jac) == want, key
        seen.add((folded, wide, tree))
    return seen


GRID = [(fold, run, quads) for fold in (0, 8) for run in (0, 1, 2, 8) for quads in (0, 1, 2)]


@pytest.mark.parametrize("curve", IDS)
@pytest.mark.parametrize("c", [9, 11, 12, 13, 15, 17])
def test_two_level_tail_every_setting(ctx, curve, c):
    """n = 2^13 points under window sizes that give the tail 2^8 ... 2^16 buckets (square and 2 : 1 splits of the bucket index), the two
    levels off and on, every run length, level 2 on one lane, on the wide law and on the quads: all 24 settings give the oracle's point.
    msm_wide_weigh / msm_wide_final run exactly where the two levels apply and msm_tail_quads = 1, msm_wide_tree exactly from c = 15 on
    (sets of 128 points and more: over 8 partial sums per set)."""
    n = 1 << 13
    r = CURVES[curve].r
    try:
        ctx.set_option("msm_window_bits", c)
        bases = ctx.bases_from_scalars(curve, 1, cp.random_fr(curve, 800 + c, n))
        pts, _ = bases.download()
        sc = cp.random_fr(curve, 900 + c, n)
        sc[::7] = 0
        sc[3::11] = limbs(r - 1, 4)
        sc[5::13] = limbs(1 << 254, 4)
        seen = tail_grid(ctx, bases, sc, c, GRID, oracle_msm(curve, pts, sc))
        assert (False, False, False) in seen and (True, True, c >= 15) in seen and (True, False, False) in seen, (c, seen)
        assert all(tree == (c >= 15) for folded, wide, tree in seen if wide)
        bases.free()
    finally:
        reset_msm_options(ctx)


@pytest.mark.parametrize("curve", IDS)
def test_two_level_tail_degenerate_sets_on_every_lane_shape(ctx, curve):
    """n = 6000, c = 13, every base the same point: buckets that hold one point (every addition of the runs and the trees a doubling), its
    negative (rows cancel to infinity), and a handful of entries in 2^12 buckets -- level 2 on one lane, the wide law and the quads"""
    r = CURVES[curve].r
    n, c = 6000, 13
    cases = {
        "doublings": fr_arr([(v % 4095) + 1 for v in range(n)]),
        "cancellations": fr_arr([(v % 2000) + 1 if v % 2 == 0 else r - ((v - 1) % 2000) - 1 for v in range(n)]),
        "sparse": fr_arr([0] * (n - 5) + [1, 4096, r - 4096, 77, 2 ** 40 + 3]),
    }
    try:
        ctx.set_option("msm_window_bits", c)
        bases = ctx.bases_from_scalars(curve, 1, fr_arr([5] * n))
        pts, _ = bases.download()
        for name, sc in cases.items():
            seen = tail_grid(ctx, bases, sc, c, [(0, 0, 1), (8, 0, 0), (8, 0, 1), (8, 2, 2), (8, 8, 1)], oracle_msm(curve, pts, sc))
            assert (True, True, False) in seen, name
        bases.free()
    finally:
        reset_msm_options(ctx)


@pytest.mark.parametrize("curve", IDS)
def test_two_level_tail_result_at_infinity(ctx, curve):
    """every base the same point, the scalars in pairs v, r - v: the buckets cancel in the trees and the result is the point at infinity,
    under both level-2 laws; then scalars v alone against the oracle"""
    n, c = 1 << 10, 11
    r = CURVES[curve].r
    try:
        ctx.set_option("msm_window_bits", c)
        bases = ctx.bases_from_scalars(curve, 1, fr_arr([5] * n))
        pts, _ = bases.download()
        cancel = fr_arr([(v // 2) % 700 + 1 if v % 2 == 0 else r - ((v // 2) % 700 + 1) for v in range(n)])
        same = fr_arr([(v % 1023) + 1 for v in range(n)])
        assert oracle_msm(curve, pts, cancel) is None
        for sc, want in ((cancel, None), (same, oracle_msm(curve, pts, same))):
            seen = tail_grid(ctx, bases, sc, c, [(8, 0, 1), (8, 0, 2), (8, 0, 0), (0, 0, 1)], want)
            assert (True, True, False) in seen and (True, False, False) in seen
        bases.free()
    finally:
        reset_msm_options(ctx)


# ---- the grand products across workgroups ----------------------------------------------------------------------------------------------------
def _dev(ctx, arr):
    d = ctx.malloc(max(32, arr.nbytes))
    ctx.h2d(d, arr)
    return d


def _host(ctx, d, n):
    out = np.zeros((n, 4), dtype=np.uint64)
    ctx.d2h(out, d)
    return out


@pytest.mark.parametrize("curve", IDS)
@pytest.mark.parametrize("n", [700, 2049, 4100])
def test_permutation_grand_product_across_workgroups(ctx, curve, n):
    """one workgroup of the scan covers PERM_THREADS * PERM_CHUNK = 2048 rows: n = 2049 (one row in the second block) and 4100 (three blocks,
    the last partial) make gp_top combine several blocks; n = 700 stays in one.  k = 2 columns of random values with h = 0 forced at two
    rows (the first decides: V_P is zero behind it) in the LAST block, so the zero crosses every block boundary before it; then without
    the zeros.  g, h, V_P and the factor products against the oracle's row-by-row recurrence."""
    r = CURVES[curve].r
    k = 2
    nblk = -(-(-(-n // PERM_CHUNK)) // PERM_THREADS)
    assert nblk == {700: 1, 2049: 2, 4100: 3}[n]
    beta, gamma = fr_ints(cp.random_fr(curve, 4400 + n, 2))
    cols, sid, ssig = (cp.random_fr(curve, 4410 + i, k * n).reshape(k, n, 4) for i in range(3))
    cols[0, 0] = limbs(r - 1, 4)
    cols[1, n - 1] = 0
    d_g, d_h, d_v = ctx.malloc(k * n * 32), ctx.malloc(k * n * 32), ctx.malloc(n * 32)
    z0, z1 = {700: (333, 520), 2049: (2048, 2048), 4100: (4097, 4099)}[n]
    for variant in ("zero denominators", "plain"):
        if variant == "plain":
            cols = cols.copy()
            cols[1, z0], cols[1, z1] = limbs(7, 4), limbs(9, 4)
        else:
            for z in (z0, z1):
                s = fr_ints(ssig[1, z])[0]
                cols[1, z] = limbs((-(beta * s + gamma)) % r, 4)            # h_1[z] = 0
        eg, eh, ev = cp.permutation_grand_product(curve, list(cols), list(sid), list(ssig), beta, gamma)
        if variant == "plain":
            assert ev[n - 1].any()
        else:
            assert ev[z0].any() and not ev[z0 + 1:].any() and not eh[1, z0].any()
        ptrs = [_dev(ctx, np.ascontiguousarray(v)) for v in list(cols) + list(sid) + list(ssig)]
        _, names = profiled(ctx, lambda: ctx.perm_grand_product_dev(curve, ptrs[:k], ptrs[k:2 * k], ptrs[2 * k:], n, limbs(beta, 4), limbs(gamma, 4), d_g, d_h, d_v))
        assert "perm_grand_product" in names
        assert (_host(ctx, d_v, n) == ev).all(), (variant, n)
        assert (_host(ctx, d_g, k * n) == eg.reshape(-1, 4)).all() and (_host(ctx, d_h, k * n) == eh.reshape(-1, 4)).all(), variant
        arr = lambda ps: (ctypes.c_void_p * k)(*ps)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = ctx.lib.zkhip_perm_factor_products_dev(ctx.h, curve, ctypes.c_size_t(k), arr(ptrs[:k]), arr(ptrs[k:2 * k]), arr(ptrs[2 * k:]), ctypes.c_size_t(n),
                                                    P(limbs(beta, 4)), P(limbs(gamma, 4)), ctypes.c_void_p(d_g), ctypes.c_void_p(d_h))
        assert rc == 0
        assert (_host(ctx, d_g, n) == cp.fr_vec(curve, 2, eg[0], eg[1])).all() and (_host(ctx, d_h, n) == cp.fr_vec(curve, 2, eh[0], eh[1])).all(), variant
        for p_ in ptrs:
            ctx.free(p_)
    for p_ in (d_g, d_h, d_v):
        ctx.free(p_)
    assert ctx.device_status() == 0


# ---- the generator fold of the inner-product argument ----------------------------------------------------------------------------------------
def fold_chunk(half):
    """points per lane of ipa_bases_fold (csrc/ipa.hip)"""
    chunk = 1
    while chunk < FOLD_MAX_CHUNK and -(-half // chunk) > FOLD_TARGET_LANES:
        chunk <<= 1
    return chunk


HALVES = [1 << 15, 1 << 16, (1 << 16) + 3, (1 << 17) + 3]


def test_fold_sizes_cover_every_chunk():
    """2, 4 and 8 points per lane.  2^16 + 3 is one lane over the target at 4 points per lane and so takes 8 like 2^17 + 3; 2^16 is the size
    with 4."""
    assert [fold_chunk(h) for h in HALVES] == [2, 4, 8, 8]


@pytest.mark.parametrize("curve", IDS)
@pytest.mark.parametrize("half", HALVES)
def test_bases_fold_every_row(ctx, zk, curve, half):
    """out[i] = c hi[i] + lo[i] at sizes where a lane takes 2, 4 and 8 points that share one inversion, every row against the oracle.  The
    inputs are multiples k_i G made on the device, chosen so that each case holds: the first and the last row of a chunk at infinity (lo and
    hi both infinite; lo = -c hi), a whole chunk of eight consecutive infinite results (nothing enters its inversion), infinity in lo alone
    and in hi alone, a row where lo = -c hi cancels and one where lo = c hi doubles inside an otherwise ordinary chunk, the same in the last
    chunk (partial when half is no multiple of 8).  And, as in test_gpu_ipa.py, MSM(out, s) = c MSM(hi, s) + MSM(lo, s) through the
    library's own MSM."""
    C = CURVES[curve]
    G, r = C.g1, C.r
    rng = np.random.default_rng(half + curve)
    ks = rng.integers(0, 1 << 62, size=(2 * half, 4), dtype=np.uint64)
    ks[:, 3] >>= np.uint64(4)
    c = int(rng.integers(1 << 40, 1 << 62)) * int(rng.integers(1 << 40, 1 << 62)) * int(rng.integers(1 << 40, 1 << 62)) * int(rng.integers(1 << 40, 1 << 62)) % r
    k_hi = lambda i: fr_ints(ks[half + i])[0]
    lo_is = lambda i, f: ks.__setitem__(i, limbs(f * k_hi(i) % r, 4))
    cancel = [16, 23, 200, half - 2] + list(range(64, 72))             # first / last of a chunk of 8; a lone row; the last chunk; a whole chunk
    double = [201, 4097, half - 1]
    for i in cancel:
        lo_is(i, r - c)
    for i in double:
        lo_is(i, c)
    ks[[24, half + 24, 31, half + 31]] = 0                             # both at infinity: first and last row of a chunk
    ks[[5, 8191]] = 0                                                  # lo alone
    ks[[half + 9, half + 12345]] = 0                                   # hi alone
    want_inf = sorted(cancel + [24, 31])
    assert fold_chunk(half) in (2, 4, 8)
    bases = ctx.bases_from_scalars(curve, zk.G1, ks)
    pts, inf = bases.download()
    assert sorted(np.nonzero(inf)[0]) == sorted([24, half + 24, 31, half + 31, 5, 8191, half + 9, half + 12345])
    out, names = profiled(ctx, lambda: ctx.bases_fold(bases, 0, half, half, limbs(c, 4)))
    assert "ipa_bases_fold" in names
    got, ginf = out.download()
    exp, einf = cp.bases_fold(curve, pts[:half], pts[half:], limbs(c, 4), inf[:half], inf[half:])
    assert sorted(np.nonzero(einf)[0]) == want_inf
    bad = np.nonzero((np.asarray(ginf) != einf) | (got != exp).any(axis=1))[0]
    assert bad.size == 0, (half, bad[:10], [i % 8 for i in bad[:10]])
    assert not got[einf != 0].any()
    assert (got[201] == cp.batch_mul(curve, 1, fr_arr([2 * c * k_hi(201) % r]))[0][0]).all()          # the doubled row, from its scalar
    # the MSM identity, through the library's own MSM
    rs = rng.integers(0, 1 << 62, size=(half, 4), dtype=np.uint64)
    rs[:, 3] >>= np.uint64(4)
    aff = lambda a: pt_from_limbs(curve, 1, a[0], a[1])
    res = aff(ctx.msm_affine(out, rs))
    lo, hi = aff(ctx.msm_affine(bases, rs, 0, half)), aff(ctx.msm_affine(bases, rs, half, half))
    assert res is not None and res == G.add(G.mul(hi, c), lo)
    out.free()
    bases.free()
    assert ctx.device_status() == 0
