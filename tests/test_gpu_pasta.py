"""Pallas (id 2) and Vesta (id 3) through the C ABI on the GPU: the device arithmetic of their lazy field types at its bounds, the MSM with
every option, NTT and evaluation domains, the polynomial / FRI / argument kernels, and what is refused -- bit-exact against pyoracle's generic
classes (tests/pasta_util.py), hashlib (tests/merkle_ref.py) and, for the arithmetic, limb for limb against the host build.
A curve id names a group and ITS scalar field: "Fr" of id 2 is F_q, of id 3 F_p (include/zkhip.h)."""
import ctypes
import os
import random

import numpy as np
import pytest

import arith_cases as ac
import merkle_ref as mr
import pasta_util as pu
import pyoracle as po
from harness import library
from test_host_pasta import check_chains, check_recoding
from util import fr_arr, fr_ints, jac_to_affine_py, limbs, lookup_instance, permutation_instance, pt_from_limbs, pt_limbs, pts_arr, qap_domains

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SO = os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_hosttest.so")
RECODE_STRIDE = 130
P = ac._ptr
INVALID = -2


@pytest.fixture(scope="module")
def dev():
    return library("libarithdev_pasta.so")


@pytest.fixture(scope="module")
def host():
    assert os.path.exists(HOST_SO), "crypto3-zk_amd/libzkhip_hosttest.so is missing: python -c 'import __graft_entry__ as g; g.build()'"
    return ctypes.CDLL(HOST_SO)


def _u32(v, n32=8):
    return np.array([(v >> (32 * i)) & 0xFFFFFFFF for i in range(n32)], dtype=np.uint32)


def _int(a):
    return sum(int(x) << (32 * i) for i, x in enumerate(a))


# ---- 1. device arithmetic at its bounds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [16, 17, 18, 19])
def test_raw_fu_ops_match_oracle_and_host_bodies(dev, host, t):
    """every raw Fu op of the four new lazy types on the device (inline-asm products, -O3): the oracle residue, the written postcondition,
    and the C++ body's limbs bit for bit.  The moduli's zero limbs 5 - 7, limb 0 = 1 and the 64 p spread limit of L = 9 are all in play:
    arith_cases' edges include p - 1, p - 2^k, R mod p and operands that fill the column accumulators."""
    for op, k, cases in ac.raw_suite(t, seed=1):
        ops = list(zip(*cases))
        rc, got = ac.run_raw(dev.zkdp_fu_raw, t, op, *ops, size_t=False)
        assert rc == 0, (t, op, rc)
        rc, ref = ac.run_raw(host.zkt_fu_raw, t, op, *ops)
        assert rc == 0
        for case, r, h in zip(cases, got, ref):
            err = ac.check_raw(t, op, *case, r, k=k)
            assert err is None, (t, op, k, err, [hex(ac.value(x)) for x in case], r)
            assert r == h, ("device limbs differ from the C++ body", t, op, k, [hex(ac.value(x)) for x in case], r, h)
    z = [[0] * ac.TYPES[t][1]]
    assert ac.run_raw(dev.zkdp_fu_raw, t, 11, z, size_t=False)[0] == -1
    if t in (18, 19):
        assert ac.run_raw(dev.zkdp_fu_raw, t, ac.op_sub(128), z, size_t=False)[0] == -1


@pytest.mark.parametrize("field", [16, 17, 18, 19])
def test_field_op_table_on_device(dev, host, field):
    p = ac.TYPES[field][0]
    rng = random.Random(field)
    vals = ac.canonical_edges(field) + [rng.randrange(p) for _ in range(8)]
    pairs = [(a, vals[(i * 7 + 3) % len(vals)]) for i, a in enumerate(vals)]

    def expect(op, a, b):
        X = (a * a - a * b - 2 * b * b) % p
        return {0: a * b, 1: a + b, 2: a - b, 3: pow(a, -1, p) if a else 0, 4: a * a, 5: -a, 6: 2 * a, 7: a - b, 8: (a * b - X) * (b * b - X),
                9: (a + b) ** 2, 10: a * (a + b) + b * b, 11: pow(a, -1, p) if a else 0}[op] % p

    for op in range(12):
        cases = [(a, b) for a, b in pairs if op not in (3, 11) or a]
        A, Bv = np.stack([_u32(a) for a, _ in cases]), np.stack([_u32(b) for _, b in cases])
        out = np.zeros_like(A)
        assert dev.zkdp_field_op(field, op, len(cases), P(A), P(Bv), P(out)) == 0
        h = np.zeros(8, dtype=np.uint32)
        for i, (a, b) in enumerate(cases):
            assert _int(out[i]) == expect(op, a, b), (field, op, hex(a), hex(b))
            assert host.zkt_field_op(field, op, P(A[i]), P(Bv[i]), P(h)) == 0
            assert (h == out[i]).all()
    assert dev.zkdp_field_op(field, 12, 1, P(A), P(Bv), P(out)) == -1


def _chain_dev(dev, field, curve, pts, infs, negs, mode, k=0):
    arr = pts_arr(curve, 1, pts).view(np.uint32).reshape(len(pts), -1) if len(pts) else np.zeros((0, 1), dtype=np.uint32)
    arr = np.ascontiguousarray(arr)
    out = np.zeros((3 if mode == 3 else 2) * 8, dtype=np.uint32)
    oinf = np.zeros(1, dtype=np.uint8)
    infa, nega = np.array(infs + [0], dtype=np.uint8), np.array(negs + [0], dtype=np.uint8)
    assert dev.zkdp_point_chain(field, P(arr), P(infa), P(nega), ctypes.c_size_t(len(pts)), mode, ctypes.c_uint32(k), P(out), P(oinf)) == 0
    return out.view(np.uint64), int(oinf[0])


@pytest.mark.parametrize("curve", [2, 3])
def test_point_chains_on_device(dev, curve):
    """the group-law cases of the host suite (P + P, P + (-P), infinity operands, restart after infinity, the generator (-1, 2) and its
    negative) on the device, modes 0 - 4"""
    check_chains(lambda *a: _chain_dev(dev, *a), pu.LAZY_FQ[curve], curve, 107)


@pytest.mark.parametrize("curve", [2, 3])
def test_parked_points_share_one_inversion_on_device(dev, host, curve):
    """xyzz_park / xyzz_parked_to_affine (curve.hpp) on one lane: parked_cases.py's chains -- every prefix against big integers, both
    layouts -- and limb for limb what the host build of the same code gives"""
    import parked_cases
    G, base = pu.CURVES[curve].g1, pu.random_points(curve, 307, 4)
    got = parked_cases.check(dev.zkdp_parked_affine, pu.LAZY_FQ[curve], curve, 1, G, base)
    ref = parked_cases.check(host.zkt_parked_affine, pu.LAZY_FQ[curve], curve, 1, G, base)
    for (o, i), (ho, hi) in zip(got, ref):
        assert (o == ho).all() and (i == hi).all()


@pytest.mark.parametrize("curve", [2, 3])
def test_recode_on_device(dev, host, curve):
    r = pu.CURVES[curve].r
    for c in range(2, 22):
        rng = random.Random(c)
        vals = ac.scalar_edges(r, c, rng) + [1 << 254, r - 2, 3 * r + 1] + [rng.randrange(1 << 254, r) for _ in range(3)]
        S = np.stack([_u32(v) for v in vals])
        dig = np.zeros((len(vals), RECODE_STRIDE), dtype=np.int32)
        assert dev.zkdp_recode_folded(curve, c, len(vals), P(S), P(dig)) == 0
        rows = {v: d for v, d in zip(vals, dig)}
        assert all(d[129] == 0 for d in dig)
        check_recoding(lambda v: (int(rows[v][128]), rows[v]), r, c, vals)
        ref = np.zeros(140, dtype=np.int32)
        for v, d in zip(vals, dig):
            W = host.zkt_recode_folded(curve, P(_u32(v)), c, P(ref))
            assert (d[:W] == ref[:W]).all(), (c, hex(v))
    assert dev.zkdp_recode_folded(curve, 22, 1, P(S), P(dig)) == -1


# ---- 2. MSM -------------------------------------------------------------------------------------------------------------------------------
def gpu_affine(ctx, bases, scalars, **kw):
    """MSM on the GPU -> affine point via the checker's big-int inversion, and the same through the device conversion"""
    jac = ctx.msm(bases, scalars, **kw)
    Pt = jac_to_affine_py(bases.curve, 1, jac)
    dev_aff, dev_inf = ctx.jacobian_to_affine(bases.curve, 1, jac)
    assert pt_from_limbs(bases.curve, 1, dev_aff, dev_inf) == Pt
    return Pt


_POINTS = {}


def points(curve, n):
    """the first n of 2048 multiples of the generator, computed once per curve"""
    if curve not in _POINTS:
        _POINTS[curve] = pu.random_points(curve, 11, 2048)
    return _POINTS[curve][:n]


@pytest.mark.parametrize("curve", [2, 3])
def test_msm_matches_oracle(ctx, curve):
    G = pu.CURVES[curve].g1
    pts = points(curve, 2048)
    arr = pts_arr(curve, 1, pts)
    bases = ctx.upload_bases(curve, 1, arr)
    dl, dinf = bases.download()                         # the round trip through the Montgomery device form
    assert (dl == arr).all() and not dinf.any()
    for n in (1, 2, 17, 300, 2048):
        sc = fr_ints(pu.random_fr(curve, 200 + n, n))
        exp = po.msm_pippenger(G, pts[:n], sc)
        if n <= 256:
            assert exp == po.msm_naive(G, pts[:n], sc)
        assert gpu_affine(ctx, bases, fr_arr(sc), n=n) == exp, (curve, n)
    # a sub-range, as the reference's iterator pairs give
    sc = fr_ints(pu.random_fr(curve, 777, 30))
    assert gpu_affine(ctx, bases, fr_arr(sc), offset=20, n=30) == po.msm_naive(G, pts[20:50], sc)
    with pytest.raises(Exception):
        ctx.msm(bases, fr_arr(sc), offset=2040, n=30)
    bases.free()


@pytest.mark.parametrize("curve", [2, 3])
def test_msm_edge_cases_and_every_option(ctx, curve):
    """n = 64 with duplicate, negated and infinity bases; scalars 0, 1, r - 1, (r +- 1) / 2, 2^254 and the tiny range [2^254, r); every window
    size with window tables (all windows in one bucket set, a few sets, one set per window; both sort tiles) and without (the Horner
    pass); non-canonical scalars r, r + 1 and 2^256 - 1 = 3 r + ... are taken mod r"""
    C = pu.CURVES[curve]
    G, r = C.g1, C.r
    n = 64
    Pts = list(points(curve, n))
    Pts[1] = Pts[0]
    Pts[2] = G.neg(Pts[0])
    Pts[3] = None
    Pts[10] = Pts[11]
    Pts[20] = G.gen
    Pts[21] = G.neg(G.gen)
    arr = pts_arr(curve, 1, Pts)
    infs = np.array([1 if p is None else 0 for p in Pts], dtype=np.uint8)
    rng = random.Random(curve)
    sc = fr_ints(pu.random_fr(curve, 6, n))
    sc[0] = sc[1] = sc[2] = 12345
    sc[4:10] = [0, 1, r - 1, (r - 1) // 2, (r + 1) // 2, 1 << 254]
    sc[10], sc[11] = 77, r - 77
    sc[12:16] = [(1 << 254) + 1, r - 2] + [rng.randrange(1 << 254, r) for _ in range(2)]
    sc[20] = sc[21] = r - 1
    exp = po.msm_naive(G, Pts, sc)
    bases = ctx.upload_bases(curve, 1, arr, infs)
    assert gpu_affine(ctx, bases, fr_arr(sc)) == exp
    try:
        for c in (2, 3, 5, 7, 12, 15, 16, 17, 20):          # 3, 5, 15, 17 divide 255: the top window is full
            ctx.set_option("msm_window_bits", c)
            tb = ctx.upload_bases(curve, 1, arr, infs)
            for sets, tile_log in ((0, 14), (1, 12), (5, 14), (64, 12)):
                ctx.set_option("msm_sets", sets)
                ctx.set_option("msm_sort_tile_log", tile_log)
                assert gpu_affine(ctx, tb, fr_arr(sc)) == exp, (c, sets, tile_log)
            ctx.set_option("msm_sets", 0)
            ctx.set_option("msm_sort_tile_log", 14)
            if c == 16:                                      # the two-level tail off, and the pair-only tail
                for opt in ("msm_tail_fold", "msm_tail_quads"):
                    keep = ctx.get_option(opt)
                    ctx.set_option(opt, 0)
                    assert gpu_affine(ctx, tb, fr_arr(sc)) == exp, opt
                    ctx.set_option(opt, keep)
            tb.free()
        ctx.set_option("msm_precompute", 0)
        ctx.set_option("msm_window_bits", 0)
        plain = ctx.upload_bases(curve, 1, arr, infs)
        ctx.set_option("msm_precompute", 1)
        for c in (0, 2, 3, 5, 7, 12, 15, 16, 17, 20):
            ctx.set_option("msm_window_bits", c)
            assert gpu_affine(ctx, plain, fr_arr(sc)) == exp, c
        nc = list(sc)
        nc[8], nc[9], nc[30] = r, r + 1, (1 << 256) - 1
        red = [v % r for v in nc]
        assert nc[30] // r == 3
        exp_nc = po.msm_naive(G, Pts, red)
        for c, b in ((0, bases), (15, plain), (16, bases)):
            ctx.set_option("msm_window_bits", c)
            assert gpu_affine(ctx, b, fr_arr(nc)) == exp_nc, c
        ctx.set_option("msm_window_bits", 0)
        zero = np.zeros((n, 4), dtype=np.uint64)
        assert gpu_affine(ctx, bases, zero) is None
        assert gpu_affine(ctx, bases, zero[:0], n=0) is None
        plain.free()
    finally:
        for name, v in (("msm_window_bits", 0), ("msm_sets", 0), ("msm_sort_tile_log", 14), ("msm_precompute", 1)):
            ctx.set_option(name, v)
        bases.free()


@pytest.mark.parametrize("curve,n", [(2, 300), (3, 300), (2, 4101), (3, 4101)])
def test_bases_from_scalars_default_generator(ctx, curve, n):
    """k_i (p - 1, 2) on the device: the double-and-add kernel (n < 4096) and the fixed-base table (n = 4101: past the switch, a short last
    chunk), zero scalars included; then an MSM over the device-generated (lazily reduced) points"""
    C = pu.CURVES[curve]
    ks = fr_ints(pu.random_fr(curve, 42, n))
    ks[0], ks[1], ks[2] = 0, 1, C.r - 1
    if n > 4096:
        ks[80] = ks[167] = ks[4098] = 0
        ks[320:328] = [0] * 8
    exp = C.g1.batch_mul_gen(ks)
    b = ctx.bases_from_scalars(curve, 1, fr_arr(ks))
    got, ginf = b.download()
    assert [pt_from_limbs(curve, 1, g, i) for g, i in zip(got, ginf)] == exp
    if n == 300:
        sc = fr_ints(pu.random_fr(curve, 43, n))
        assert gpu_affine(ctx, b, fr_arr(sc)) == po.msm_pippenger(C.g1, exp, sc)
        # an explicit base: another point
        base = points(curve, 1)[0]
        b2 = ctx.bases_from_scalars(curve, 1, fr_arr(ks[:40]), base=pt_limbs(curve, 1, base))
        got, ginf = b2.download()
        assert [pt_from_limbs(curve, 1, g, i) for g, i in zip(got, ginf)] == [C.g1.mul(base, k) for k in ks[:40]]
        b2.free()
    b.free()


@pytest.mark.parametrize("curve", [2, 3])
def test_msm_batch_of_three_sharing_scalars(ctx, zk, curve):
    """zkhip_msm_batch_dev: three table-backed members over ONE scalar vector (they share the digit extraction and the sort), with the
    sharing on and off; the Jacobian sum of the three results on the device"""
    G = pu.CURVES[curve].g1
    n = 300
    allp = points(curve, 3 * n)
    members = [allp[i * n:(i + 1) * n] for i in range(3)]
    bs = [ctx.upload_bases(curve, 1, pts_arr(curve, 1, m)) for m in members]
    sc = fr_ints(pu.random_fr(curve, 91, n))
    exp = [po.msm_pippenger(G, m, sc) for m in members]
    jac = 3 * zk.coord_limbs(curve, 1) * 8
    d_s, d_o = ctx.malloc(n * 32), ctx.malloc(4 * jac)
    ctx.h2d(d_s, fr_arr(sc))
    res = np.zeros((4, jac // 8), dtype=np.uint64)
    try:
        for share in (1, 0):
            ctx.set_option("msm_share_sort", share)
            ctx.h2d(d_o, res * 0)
            ctx.msm_batch_dev(bs, [d_s] * 3, [d_o + i * jac for i in range(3)])
            ctx.jacobian_sum_dev(curve, 1, d_o, 3, d_o + 3 * jac)
            ctx.d2h(res, d_o)
            assert [jac_to_affine_py(curve, 1, res[i]) for i in range(3)] == exp, share
            total = None
            for e in exp:
                total = G.add(total, e)
            assert jac_to_affine_py(curve, 1, res[3]) == total
    finally:
        ctx.set_option("msm_share_sort", 1)
        ctx.free(d_s)
        ctx.free(d_o)
        for b in bs:
            b.free()


# ---- 7 (and the refusals of 2). what is refused ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [2, 3])
def test_refusals(zk, curve):
    """G2 with a Pasta id, a coordinate >= p, and the entry points that need a pairing-friendly curve -- the Groth16 constraint-system upload
    (every other zkhip_r1cs_* / zkhip_groth16_* call takes its handle), the compressed wire format, the EC-NTT: ZKHIP_ERR_INVALID from the
    entry preamble, no launch (the profiler has counted none), a clean device status and a context that works afterwards"""
    C = pu.CURVES[curve]
    c = zk.Context(0)
    try:
        L, h, z = c.lib, c.h, ctypes.c_size_t
        d = c.malloc(1 << 12)
        c.h2d(d, np.zeros(1 << 9, dtype=np.uint64))
        vp = ctypes.c_void_p(d)
        out = np.zeros(64, dtype=np.uint64)
        one = pt_limbs(curve, 1, C.g1.gen)
        rp = np.zeros(2, dtype=np.uint32)
        w4 = limbs(C.root_of_unity(2), 4)
        hdl = ctypes.c_void_p()
        c.profile(True)
        calls = [
            ("bases_upload G2", lambda: L.zkhip_bases_upload(h, curve, 2, P(out), None, z(1), ctypes.byref(hdl))),
            ("bases_from_scalars G2", lambda: L.zkhip_bases_from_scalars(h, curve, 2, None, P(out), z(1), ctypes.byref(hdl))),
            ("jacobian_sum G2", lambda: L.zkhip_jacobian_sum_dev(h, curve, 2, vp, z(1), vp)),
            ("jacobian_to_affine G2", lambda: L.zkhip_jacobian_to_affine(h, curve, 2, P(out), P(out), P(out))),
            ("r1cs_upload", lambda: L.zkhip_r1cs_upload(h, curve, z(1), z(0), z(1), P(rp), None, None, P(rp), None, None, P(rp), None, None, ctypes.byref(hdl))),
            ("bases_upload_compressed", lambda: L.zkhip_bases_upload_compressed(h, curve, 1, P(out), z(1), ctypes.byref(hdl))),
            ("ec_ntt G1", lambda: L.zkhip_ec_ntt_dev(h, curve, 1, vp, z(2), P(w4), 0)),
            ("ec_ntt G2", lambda: L.zkhip_ec_ntt_dev(h, curve, 2, vp, z(2), P(w4), 0)),
        ]
        for name, call in calls:
            assert call() == INVALID, name
            assert not hdl.value, name
        # a coordinate that is not below the base-field modulus: p itself, p + 1, 2^256 - 1, in x and in y; a flagged point is not looked at
        good = np.concatenate([one, pt_limbs(curve, 1, C.g1.mul(C.g1.gen, 2))]).reshape(2, 8)
        for bad in (C.p, C.p + 1, (1 << 256) - 1):
            for col in (0, 4):
                a = good.copy()
                a[1, col:col + 4] = limbs(bad, 4)
                assert L.zkhip_bases_upload(h, curve, 1, P(a), None, z(2), ctypes.byref(hdl)) == INVALID, (hex(bad), col)
                assert not hdl.value
                b = c.upload_bases(curve, 1, a, np.array([0, 1], dtype=np.uint8))
                b.free()
        assert c.profile_get("bases_to_mont")[1] == 6 and c.profile_get("msm")[1] == 0    # only the six accepted uploads launched anything
        c.profile(False)
        assert c.device_status() == 0
        b = c.upload_bases(curve, 1, good)                   # p - 1 is a coordinate of the generator: the largest accepted value
        assert jac_to_affine_py(curve, 1, c.msm(b, fr_arr([1, 1]))) == C.g1.mul(C.g1.gen, 3)
        b.free()
        c.free(d)
    finally:
        c.close()


# ---- 3. NTT and domains -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [2, 3])
@pytest.mark.parametrize("log_m", [1, 2, 5, 10, 13])
def test_ntt_matches_oracle(ctx, curve, log_m):
    C = pu.CURVES[curve]
    r, m, batch = C.r, 1 << log_m, 3
    w, g = C.root_of_unity(log_m), C.fr_generator
    a = pu.random_fr(curve, 300 + log_m, batch * m).reshape(batch, m, 4)
    a[0, 0] = limbs(r - 1, 4)
    a[1, m - 1] = 0
    rows = [fr_ints(a[b]) for b in range(batch)]
    got = ctx.ntt(curve, a, log_m, limbs(w, 4))
    assert [fr_ints(got[b]) for b in range(batch)] == [po.ntt(x, w, r) for x in rows]
    back = ctx.ntt(curve, got, log_m, limbs(w, 4), inverse=True)
    assert (back == a).all() and [fr_ints(back[b]) for b in range(batch)] == [po.intt(po.ntt(x, w, r), w, r) for x in rows]
    gotc = ctx.ntt(curve, a, log_m, limbs(w, 4), coset=limbs(g, 4))
    assert [fr_ints(gotc[b]) for b in range(batch)] == [po.ntt(po.multiply_by_coset(x, g, r), w, r) for x in rows]
    inv = ctx.ntt(curve, a, log_m, limbs(w, 4), inverse=True, coset=limbs(g, 4))
    assert [fr_ints(inv[b]) for b in range(batch)] == [po.multiply_by_coset(po.intt(x, w, r), pow(g, -1, r), r) for x in rows]


@pytest.mark.parametrize("curve", [2, 3])
def test_ntt_rejects_a_root_of_the_wrong_order_and_keys_its_tables_on_the_curve(zk, ctx, curve):
    C, other = pu.CURVES[curve], pu.CURVES[5 - curve]
    log_m = 8
    a = pu.random_fr(curve, 3, 1 << log_m).reshape(1, -1, 4)
    w = C.root_of_unity(log_m)
    for bad in (w * w % C.r, 1, C.root_of_unity(log_m + 1), C.r - 1, other.root_of_unity(log_m)):
        with pytest.raises(zk.ZkhipError):
            ctx.ntt(curve, a, log_m, limbs(bad, 4))
    # the same size over the two fields, alternating: a table cached under one id must not serve the other
    for cv in (curve, 5 - curve, curve):
        Cc = pu.CURVES[cv]
        x = fr_ints(a[0])
        x = [v % Cc.r for v in x]
        got = ctx.ntt(cv, fr_arr(x).reshape(1, -1, 4), log_m, limbs(Cc.root_of_unity(log_m), 4))
        assert fr_ints(got[0]) == po.ntt(x, Cc.root_of_unity(log_m), Cc.r), cv


@pytest.mark.parametrize("curve", [2, 3])
def test_domains(ctx, zk, curve):
    """make_evaluation_domain's choice (two-adicity 32), and the transforms and Lagrange evaluations of a step radix-2 domain of 2^6 + 2^3
    points and of a basic one, against po.EvaluationDomain"""
    C = pu.CURVES[curve]
    Z = zk.zkhip
    assert Z.domain_choice(curve, (1 << 10) + 11)[0] == Z.DOMAIN_STEP
    assert Z.domain_choice(curve, 1 << 10) == (Z.DOMAIN_BASIC, 1 << 10)
    assert po.evaluation_domain_choice((1 << 10) + 11, 32) == Z.domain_choice(curve, (1 << 10) + 11)
    rng = po.SplitMix64(400 + curve)
    for min_size, kind in ((72, Z.DOMAIN_STEP), (64, Z.DOMAIN_BASIC)):
        dom, zd = qap_domains(zk, curve, min_size)
        assert (dom.kind, dom.m) == (kind, min_size)
        a = pu.random_fr(curve, 500 + min_size, 2 * dom.m).reshape(2, dom.m, 4)
        got = ctx.domain_fft(curve, zd, a)
        assert [fr_ints(got[b]) for b in range(2)] == [dom.fft(fr_ints(a[b])) for b in range(2)], dom.describe()
        assert (ctx.domain_fft(curve, zd, got, inverse=True) == a).all()
        assert fr_ints(ctx.domain_fft(curve, zd, a, inverse=True)[1]) == dom.inverse_fft(fr_ints(a[1]))
        g = C.fr_generator
        gotc = ctx.domain_fft(curve, zd, a, coset=limbs(g, 4))
        xs = [x * g % C.r for x in dom.elements()]
        coeffs = fr_ints(a[0])
        assert fr_ints(gotc[0]) == [po.poly_eval(coeffs, x, C.r) for x in xs], dom.describe()
        assert (ctx.domain_fft(curve, zd, gotc, inverse=True, coset=limbs(g, 4)) == a).all()
        t = rng.next_mod(C.r)
        assert fr_ints(ctx.domain_lagrange(curve, zd, limbs(t, 4))) == dom.evaluate_all_lagrange_polynomials(t), dom.describe()
        with pytest.raises(zk.ZkhipError):
            ctx.domain_lagrange(curve, zd, limbs(dom.elements()[7], 4))


# ---- 4. polynomial, FRI and argument kernels -----------------------------------------------------------------------------------------------
def _up(ctx, vals):
    d = ctx.malloc(max(1, len(vals)) * 32)
    ctx.h2d(d, fr_arr(vals))
    return d


def _down(ctx, d, n):
    a = np.zeros((n, 4), dtype=np.uint64)
    ctx.d2h(a, d)
    return fr_ints(a)


@pytest.mark.parametrize("curve", [3, 2])
def test_poly_resize_fold_and_leaves(ctx, curve):
    """polynomial_dfs::resize 2^6 -> 2^8 with both poly_coset_extend settings, fold_polynomial at 2^8, the FRI leaf layout of 3 x 2^8 with
    steps 1 and 3"""
    C = pu.CURVES[curve]
    r, batch = C.r, 3
    evals = [fr_ints(pu.random_fr(curve, 600 + b, 64)) for b in range(batch)]
    evals[0][0], evals[0][1] = r - 1, 0
    exp = [po.dfs_resize(e, 256, C.root_of_unity, r) for e in evals]
    d_in, d_out = ctx.malloc(batch * 64 * 32), ctx.malloc(batch * 256 * 32)
    try:
        for mode in (1, 0):
            ctx.set_option("poly_coset_extend", mode)
            ctx.h2d(d_in, fr_arr([x for e in evals for x in e]))
            ctx.h2d(d_out, fr_arr([7] * (batch * 256)))
            ctx.poly_resize_dev(curve, d_in, 6, batch, limbs(C.root_of_unity(6), 4), d_out, 8, limbs(C.root_of_unity(8), 4))
            assert _down(ctx, d_out, batch * 256) == [x for e in exp for x in e], mode
    finally:
        ctx.set_option("poly_coset_extend", 1)
    alpha = po.SplitMix64(5 + curve).next_mod(r)
    d_f = ctx.malloc(128 * 32)
    rc = ctx.lib.zkhip_fri_fold_dev(ctx.h, curve, ctypes.c_void_p(d_out), ctypes.c_size_t(8), P(limbs(alpha, 4)), P(limbs(C.root_of_unity(8), 4)), ctypes.c_void_p(d_f))
    assert rc == 0
    assert _down(ctx, d_f, 128) == po.fold_polynomial_dfs(exp[0], alpha, C.root_of_unity(8), r)
    d_l = ctx.malloc(batch * 256 * 32)
    for step in (1, 3):
        ctx.fri_leaves_dev(d_out, 8, batch, step, d_l)
        leaves = po.fri_leaves(exp, step)
        assert _down(ctx, d_l, batch * 256) == leaves, step
        # and the tree over them, hashed on the device straight from the evaluations: 32-byte big-endian elements of a 255-bit field
        t = ctx.merkle_build_fri(d_out, 8, batch, step)
        assert t.root() == bytes(mr.tree(fr_arr(leaves), 256 >> step)[-1]), step
        t.free()
    for p_ in (d_in, d_out, d_f, d_l):
        ctx.free(p_)


@pytest.mark.parametrize("curve", [3, 2])
def test_poly_eval_div_and_lincomb(ctx, curve):
    r = pu.CURVES[curve].r
    rng = po.SplitMix64(700 + curve)
    n, batch = 300, 3
    polys = [[rng.next_mod(r) for _ in range(n)] for _ in range(batch)]
    polys[1][-1] = 0
    polys[2][0] = r - 1
    pts = [0, 1, r - 1, rng.next_mod(r)]
    d = _up(ctx, [c for p_ in polys for c in p_])
    got = ctx.poly_eval_dev(curve, d, n, batch, fr_arr(pts))
    assert [fr_ints(got[b]) for b in range(batch)] == [[po.poly_eval(p_, z, r) for z in pts] for p_ in polys]
    d_q = ctx.malloc(n * 32)
    for z in (pts[3], 0, r - 1):
        rem = ctx.poly_div_linear_dev(curve, d, n, limbs(z, 4), d_q)
        g = _down(ctx, d_q, n)
        q, rm = po.poly_divmod(polys[0], [(-z) % r, 1], r)
        assert po.from_limbs(rem) == g[0] == po.poly_eval(polys[0], z, r) == (rm[0] if po.poly_trim(rm) else 0)
        assert g[1:] == (list(q) + [0] * n)[:n - 1]
    # exact division by X^16 - 1, and a remainder that is counted
    nv = 16
    quot = [rng.next_mod(r) for _ in range(37)]
    f = po.poly_mul(quot, [r - 1] + [0] * (nv - 1) + [1], r)
    d_f, d_o = _up(ctx, f), ctx.malloc(len(quot) * 32)
    assert ctx.poly_div_vanishing_dev(curve, d_f, len(f), nv, d_o) == 0
    assert _down(ctx, d_o, len(quot)) == quot
    f[3] = (f[3] + 1) % r
    ctx.h2d(d_f, fr_arr(f))
    assert ctx.poly_div_vanishing_dev(curve, d_f, len(f), nv, d_o) == 1
    # f += sum_i sum_t c[i][t] X^t poly_i over ragged lengths
    lens, taps, acc_len = [300, 256, 1, 299], 3, 302
    ps = [[rng.next_mod(r) for _ in range(ln)] for ln in lens]
    cs = [[rng.next_mod(r) for _ in range(taps)] for _ in lens]
    cs[1][2], cs[3] = 0, [r - 1, 0, 1]
    exp = [0] * acc_len
    for p_, c in zip(ps, cs):
        for t in range(taps):
            for j, x in enumerate(p_):
                if j + t < acc_len:
                    exp[j + t] = (exp[j + t] + c[t] * x) % r
    ds = [_up(ctx, p_) for p_ in ps]
    d_acc = ctx.malloc(acc_len * 32)
    ctx.poly_lincomb_dev(curve, ds, lens, fr_arr([x for c in cs for x in c]), taps, d_acc, acc_len, False)
    assert _down(ctx, d_acc, acc_len) == exp
    ctx.poly_lincomb_dev(curve, ds, lens, fr_arr([x for c in cs for x in c]), taps, d_acc, acc_len, True)
    assert _down(ctx, d_acc, acc_len) == [2 * x % r for x in exp]
    # pointwise vectors: a + b, a - b, a b, a x + b y + c, a b / c
    a, b = polys[0], polys[1]
    d_a, d_b, d_c = _up(ctx, a), _up(ctx, b), _up(ctx, [v or 1 for v in polys[2]])
    for op, fn in ((0, lambda x, y: (x + y) % r), (1, lambda x, y: (x - y) % r), (2, lambda x, y: x * y % r)):
        ctx.fr_vec_op_dev(curve, op, d_a, d_b, d_q, n)
        assert _down(ctx, d_q, n) == [fn(x, y) for x, y in zip(a, b)], op
    ctx.fr_vec_affine_dev(curve, d_a, d_b, limbs(r - 1, 4), limbs(5, 4), limbs(r - 2, 4), d_q, n)
    assert _down(ctx, d_q, n) == [((r - 1) * x + 5 * y + r - 2) % r for x, y in zip(a, b)]
    ctx.fr_vec_mul_div_dev(curve, d_a, d_b, d_c, d_q, n)
    assert _down(ctx, d_q, n) == [x * y * pow(w or 1, -1, r) % r for x, y, w in zip(a, b, polys[2])]
    for p_ in [d, d_q, d_f, d_o, d_acc, d_a, d_b, d_c] + ds:
        ctx.free(p_)


@pytest.mark.parametrize("curve", [3, 2])
def test_permutation_grand_product_and_factor_products(ctx, curve):
    """3 columns x 2^6 rows of a genuine copy-constraint instance (V_P closes at usable_rows), the g / h vectors, the factor products; then a
    zero denominator: the row's ratio is 0, V_P is zero behind it"""
    C = pu.CURVES[curve]
    r, n, k, usable = C.r, 64, 3, 61
    rng = po.SplitMix64(800 + curve)
    cols, sid, ssig = permutation_instance(C, rng, 6, k, usable)
    beta, gamma = rng.next_mod(r), rng.next_mod(r)
    d_g, d_h, d_v = ctx.malloc(k * n * 32), ctx.malloc(k * n * 32), ctx.malloc(n * 32)
    ptrs = []
    for variant in (0, 1):
        if variant:
            cols[1][40] = (-(beta * ssig[1][40] + gamma)) % r        # h_1[40] = 0
        g, h, V = po.permutation_grand_product(cols, sid, ssig, beta, gamma, r)
        assert (V[usable] == 1) if not variant else (V[40] != 0 and V[41:] == [0] * (n - 41))
        ptrs = [_up(ctx, v) for v in cols + sid + ssig]
        ctx.perm_grand_product_dev(curve, ptrs[:k], ptrs[k:2 * k], ptrs[2 * k:], n, limbs(beta, 4), limbs(gamma, 4), d_g, d_h, d_v)
        assert _down(ctx, d_v, n) == V, variant
        assert _down(ctx, d_g, k * n) == [x for v in g for x in v] and _down(ctx, d_h, k * n) == [x for v in h for x in v]
        arr = lambda ps: (ctypes.c_void_p * k)(*ps)
        rc = ctx.lib.zkhip_perm_factor_products_dev(ctx.h, curve, ctypes.c_size_t(k), arr(ptrs[:k]), arr(ptrs[k:2 * k]), arr(ptrs[2 * k:]), ctypes.c_size_t(n),
                                                    P(limbs(beta, 4)), P(limbs(gamma, 4)), ctypes.c_void_p(d_g), ctypes.c_void_p(d_h))
        assert rc == 0
        assert _down(ctx, d_g, n) == [g[0][j] * g[1][j] * g[2][j] % r for j in range(n)]
        assert _down(ctx, d_h, n) == [h[0][j] * h[1][j] * h[2][j] % r for j in range(n)]
        for p_ in ptrs:
            ctx.free(p_)
    for p_ in (d_g, d_h, d_v):
        ctx.free(p_)


@pytest.mark.parametrize("curve", [3, 2])
def test_lookup_sort_and_grand_product(ctx, curve):
    C = pu.CURVES[curve]
    r, n = C.r, 64
    rng = po.SplitMix64(900 + curve)
    inputs, values, usable = lookup_instance(C, rng, 6, 2, 1)
    exp = po.lookup_sort_polynomials(inputs, values, n, usable)
    ptrs = [_up(ctx, v) for v in inputs + values]
    outs = [_up(ctx, [5] * n) for _ in range(3)]
    ctx.lookup_sort_dev(ptrs[:2], ptrs[2:], n, usable, outs)
    assert [_down(ctx, d, n) for d in outs] == exp
    assert ctx.device_status() == 0
    beta, gamma = rng.next_mod(r), rng.next_mod(r)
    d_v = ctx.malloc(n * 32)
    ctx.lookup_grand_product_dev(curve, ptrs[:2], ptrs[2:], outs, n, usable, limbs(beta, 4), limbs(gamma, 4), d_v)
    VL = po.lookup_grand_product(inputs, values, exp, beta, gamma, usable, r)
    assert VL[usable] == 1 and _down(ctx, d_v, n) == VL
    for p_ in ptrs + outs + [d_v]:
        ctx.free(p_)


@pytest.mark.parametrize("curve", [3, 2])
def test_gate_eval_flat_program(ctx, zk, curve):
    """the flat program shape of tests/test_gpu_poly.py at 2^6 rows: gates with and without a selector, shared factors, rotations +-2 (and
    others) that wrap, a constant term, 37 terms in one gate, an empty gate; with mask, in two accumulating pieces -- every row from big
    integers"""
    from functools import reduce
    r, log_size = pu.CURVES[curve].r, 6
    size, n_slots = 1 << log_size, 6
    cols = [fr_ints(pu.random_fr(curve, 1000 + s, size)) for s in range(n_slots)]
    cols[5][::3] = [0] * len(cols[5][::3])
    rng = po.SplitMix64(55 + curve)
    big_gate = (None, [(rng.next_mod(r), [(t % 5, (t % 7) - 3), ((t + 1) % 5, 0)]) for t in range(37)])
    gates = [((5, 0), [(rng.next_mod(r), [(0, 0), (1, 1)]), (r - 1, [(2, -1)])]),
             ((5, 2), [(rng.next_mod(r), [(0, 2), (0, 0), (3, -2)]), (7, [])]),
             (None, [(rng.next_mod(r), [(4, 1), (4, 1), (4, size - 1)])]),
             big_gate, (None, []), ((3, -5), [(1, [])])]
    mask = fr_ints(pu.random_fr(curve, 1099, size))
    mask[-5:] = [0] * 5

    def expect(gs, with_mask):
        out = []
        for j in range(size):
            tot = 0
            for sel, terms in gs:
                g = sum(c * reduce(lambda a, b: a * b % r, [cols[sl][(j + rot) % size] for sl, rot in fs], 1) for c, fs in terms) % r
                tot += g * (cols[sel[0]][(j + sel[1]) % size] if sel is not None else 1)
            out.append(tot * (mask[j] if with_mask else 1) % r)
        return out

    d_slots = [_up(ctx, c) for c in cols]
    d_mask, d_out = _up(ctx, mask), ctx.malloc(size * 32)
    ctx.gate_eval_dev(curve, gates, d_slots, log_size, d_out, d_mask)
    want = expect(gates, True)
    assert _down(ctx, d_out, size) == want
    ctx.gate_eval_dev(curve, gates[:2], d_slots, log_size, d_out)
    assert _down(ctx, d_out, size) == expect(gates[:2], False)
    ctx.gate_eval_dev(curve, gates[2:], d_slots, log_size, d_out, d_mask, accumulate=True)
    assert _down(ctx, d_out, size) == want
    with pytest.raises(zk.ZkhipError):
        ctx.gate_eval_dev(curve, [(None, [(1, [(n_slots, 0)])])], d_slots, log_size, d_out)
    for p_ in d_slots + [d_mask, d_out]:
        ctx.free(p_)


# ---- 6 (second half). a device group of two members on one GPU ------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [2, 3])
def test_group_msm_and_ntt_equal_the_single_context(zk, ctx, curve):
    C = pu.CURVES[curve]
    n = 1 << 10
    pts = points(curve, n)
    arr = pts_arr(curve, 1, pts)
    sc = pu.random_fr(curve, 1200, n)
    single = ctx.upload_bases(curve, 1, arr)
    want = ctx.msm_affine(single, sc)
    single.free()
    assert pt_from_limbs(curve, 1, want[0], want[1]) == po.msm_pippenger(C.g1, pts, fr_ints(sc))
    grp = zk.DeviceGroup([0, 0])
    try:
        gb = grp.upload_bases(curve, 1, arr)
        got = grp.msm_affine(gb, sc)
        assert got[1] == want[1] and (got[0] == want[0]).all()
        gb.free()
        log_m, batch = 10, 4
        w = limbs(C.root_of_unity(log_m), 4)
        a = pu.random_fr(curve, 1201, batch << log_m).reshape(batch, 1 << log_m, 4)
        assert (grp.ntt(curve, a, log_m, w) == ctx.ntt(curve, a, log_m, w)).all()
        g = limbs(C.fr_generator, 4)
        assert (grp.ntt(curve, a, log_m, w, inverse=True, coset=g) == ctx.ntt(curve, a, log_m, w, inverse=True, coset=g)).all()
    finally:
        grp.close()
