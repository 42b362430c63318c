"""Pallas (id 2) and Vesta (id 3) in the C++ oracle, pinned before the GPU suite trusts it: every cport function the Pasta GPU tests
compare against is held here to pyoracle's generic Group / Fq classes and big-integer polynomial arithmetic (tests/pasta_util.py), the same
classes tests/test_host_pasta.py leans on.  Bit-exact, CPU only.  The inputs go after what is particular to the cycle: both primes are
2^254 + a 126-bit tail (zero middle limbs), [2^254, r) is a tiny range, and one prime is the coordinate field of one id and the scalar
field of the other -- so a swapped table shows in every test."""
import numpy as np
import pytest

import cport as cp
import pasta_util as pu
import pyoracle as po
from util import fr_arr, fr_ints, limbs, lookup_instance, permutation_instance, pt_from_limbs, pt_limbs, pts_arr

IDS = [pu.PALLAS_ID, pu.VESTA_ID]
_PTS = {}


def points(curve, n):
    if curve not in _PTS:
        _PTS[curve] = pu.random_points(curve, 21, 2048)
    return _PTS[curve][:n]


def _aff(curve, out):
    return pt_from_limbs(curve, 1, out[0], out[1])


def _edge_instance(curve, n, seed):
    """n points and scalars with the edges in: scalars 0, 1, r - 1, 2^254 and the range above it; duplicate, negated and infinity bases"""
    C = pu.CURVES[curve]
    G, r = C.g1, C.r
    pts = list(points(curve, n))
    sc = fr_ints(pu.random_fr(curve, seed, n))
    if n >= 16:
        pts[1] = pts[0]
        pts[2] = G.neg(pts[0])
        pts[3] = None
        pts[9] = G.gen
        pts[10] = G.neg(G.gen)
        sc[0] = sc[1] = sc[2] = 0x1234567
        sc[4:9] = [0, 1, r - 1, 1 << 254, (1 << 254) + 1]
        sc[9] = sc[10] = r - 1
        sc[11] = r - 2
    return pts, sc


@pytest.mark.parametrize("curve", IDS)
@pytest.mark.parametrize("n", [1, 2, 16, 65, 256])
def test_msm_against_the_definition(curve, n):
    G = pu.CURVES[curve].g1
    pts, sc = _edge_instance(curve, n, 100 + n)
    want = po.msm_naive(G, pts, sc)
    arr = pts_arr(curve, 1, pts)
    inf = np.array([p is None for p in pts], dtype=np.uint8)
    for chunks in (1, 4):
        assert _aff(curve, cp.msm(curve, 1, arr, fr_arr(sc), inf, chunks=chunks)) == want, chunks
    assert _aff(curve, cp.msm(curve, 1, arr, fr_arr(sc), inf, naive=True)) == want
    b = cp.Bases(curve, 1, arr, inf)
    assert _aff(curve, b.msm(fr_arr(sc), chunks=4)) == want
    if n >= 16:
        assert _aff(curve, b.msm(fr_arr(sc[3:12]), off=3, n=9)) == po.msm_naive(G, pts[3:12], sc[3:12])


@pytest.mark.parametrize("curve", IDS)
def test_msm_2048_and_a_result_at_infinity(curve):
    C = pu.CURVES[curve]
    G, r = C.g1, C.r
    pts, sc = _edge_instance(curve, 2048, 7)
    want = po.msm_pippenger(G, pts, sc)
    arr = pts_arr(curve, 1, pts)
    inf = np.array([p is None for p in pts], dtype=np.uint8)
    for chunks in (1, 4):
        assert _aff(curve, cp.msm(curve, 1, arr, fr_arr(sc), inf, chunks=chunks)) == want
    # s P + (r - s) P + t Q + t (-Q) + 0 R + k inf = infinity
    p4 = [pts[5], pts[5], pts[6], G.neg(pts[6]), pts[7], None]
    s4 = [sc[20], r - sc[20], sc[21], sc[21], 0, sc[22]]
    for chunks in (1, 4):
        out = cp.msm(curve, 1, pts_arr(curve, 1, p4), fr_arr(s4), np.array([0, 0, 0, 0, 0, 1], dtype=np.uint8), chunks=chunks)
        assert out[1] == 1 and not out[0].any()
    assert po.msm_naive(G, p4, s4) is None


@pytest.mark.parametrize("curve", IDS)
def test_batch_mul_point_add_and_jac_to_affine(curve):
    C = pu.CURVES[curve]
    G, r, p = C.g1, C.r, C.p
    ks = fr_ints(pu.random_fr(curve, 31, 40)) + [0, 1, 2, r - 1, r - 2, 1 << 254, (1 << 254) + 1]
    got, ginf = cp.batch_mul(curve, 1, fr_arr(ks))
    assert [pt_from_limbs(curve, 1, g, i) for g, i in zip(got, ginf)] == G.batch_mul_gen(ks)
    assert pt_from_limbs(curve, 1, got[-6], 0) == (p - 1, 2)                    # 1 * generator: the largest coordinate there is
    base = points(curve, 3)[2]
    got, ginf = cp.batch_mul(curve, 1, fr_arr(ks), base=pt_limbs(curve, 1, base))
    assert [pt_from_limbs(curve, 1, g, i) for g, i in zip(got, ginf)] == [G.mul(base, k) for k in ks]
    A, B = points(curve, 2)
    L = lambda P_: pt_limbs(curve, 1, P_)
    cases = [(A, B), (A, A), (A, G.neg(A)), (None, B), (A, None), (None, None), (G.gen, G.gen), (G.gen, G.neg(G.gen))]
    for X, Y in cases:
        assert _aff(curve, cp.point_add(curve, 1, L(X), X is None, L(Y), Y is None)) == G.add(X, Y), (X, Y)
    rng = po.SplitMix64(33 + curve)
    for Pt in (A, G.gen, None):
        z = rng.next_mod(p - 1) + 1
        jac = [1, 1, 0] if Pt is None else [Pt[0] * z * z % p, Pt[1] * z * z * z % p, z]
        assert _aff(curve, cp.jac_to_affine(curve, 1, np.concatenate([limbs(v, 4) for v in jac]))) == Pt


@pytest.mark.parametrize("curve", IDS)
def test_bases_fold(curve):
    """out[i] = c hi[i] + lo[i]: generic rows, a row that doubles (lo = c hi), rows that cancel (lo = -c hi), infinity in lo, in hi and in
    both; c random, 0, 1, r - 1 and 2^254"""
    C = pu.CURVES[curve]
    G, r = C.g1, C.r
    n = 12
    base = points(curve, 2 * n)
    for c in (pu.random_fr(curve, 41, 1)[0], 0, 1, r - 1, 1 << 254):
        c = c if isinstance(c, int) else fr_ints(c)[0]
        lo, hi = list(base[:n]), list(base[n:])
        lo[1] = G.mul(hi[1], c)                                   # doubles
        lo[2] = G.neg(G.mul(hi[2], c)) if c else None             # cancels (c = 0: infinity + infinity)
        lo[3] = G.neg(G.mul(hi[3], c)) if c else None
        lo[4] = None
        hi[5] = None
        lo[6] = hi[6] = None
        hi[7] = lo[7]
        hi[8] = G.neg(lo[8])
        want = [G.add(G.mul(h, c), l) for l, h in zip(lo, hi)]
        if c:
            assert want[2] is None and want[3] is None and want[1] == G.mul(hi[1], 2 * c)
        inf = lambda ps: np.array([p_ is None for p_ in ps], dtype=np.uint8)
        got, ginf = cp.bases_fold(curve, pts_arr(curve, 1, lo), pts_arr(curve, 1, hi), limbs(c, 4), inf(lo), inf(hi))
        assert [pt_from_limbs(curve, 1, g, i) for g, i in zip(got, ginf)] == want, hex(c)
        assert not got[ginf != 0].any()
    # without flags every row is a point
    got, ginf = cp.bases_fold(curve, pts_arr(curve, 1, base[:n]), pts_arr(curve, 1, base[n:]), limbs(3, 4))
    assert [pt_from_limbs(curve, 1, g, i) for g, i in zip(got, ginf)] == [G.add(G.mul(h, 3), l) for l, h in zip(base[:n], base[n:])]


# ---- the scalar field ------------------------------------------------------------------------------------------------------------------------
def _vec(curve, seed, n):
    r = pu.CURVES[curve].r
    v = fr_ints(pu.random_fr(curve, seed, n))
    for i, e in enumerate([r - 1, 0, 1, 1 << 254, r - 2][:n]):
        v[(i * 7 + 1) % n] = e
    return v


@pytest.mark.parametrize("curve", IDS)
@pytest.mark.parametrize("log_m", [0, 1, 2, 3, 6, 10])
def test_ntt(curve, log_m):
    C = pu.CURVES[curve]
    r, m, batch = C.r, 1 << log_m, 3
    w, g = C.root_of_unity(log_m), C.fr_generator
    assert fr_ints(cp.fr_root(curve, log_m)) == [w] and pow(w, m, r) == 1 and (m == 1 or pow(w, m // 2, r) == r - 1)
    rows = [_vec(curve, 200 + log_m + b, m) for b in range(batch)]
    ref = (lambda x, w_: po.dft_naive(x, w_, r)) if log_m <= 6 else (lambda x, w_: po.ntt(x, w_, r))
    a = np.stack([fr_arr(x) for x in rows])
    W, Gc = limbs(w, 4), limbs(g, 4)
    ginv, winv, minv = pow(g, -1, r), pow(w, -1, r), pow(m, -1, r)
    fwd = cp.ntt(curve, a, log_m, W)
    assert [fr_ints(fwd[b]) for b in range(batch)] == [ref(x, w) for x in rows]
    inv = cp.ntt(curve, a, log_m, W, inverse=True)
    assert [fr_ints(inv[b]) for b in range(batch)] == [[v * minv % r for v in ref(x, winv)] for x in rows]
    assert (cp.ntt(curve, fwd, log_m, W, inverse=True) == a).all()
    cos = cp.ntt(curve, a, log_m, W, coset=Gc)
    assert [fr_ints(cos[b]) for b in range(batch)] == [ref(po.multiply_by_coset(x, g, r), w) for x in rows]
    icos = cp.ntt(curve, a, log_m, W, inverse=True, coset=Gc)
    assert [fr_ints(icos[b]) for b in range(batch)] == [po.multiply_by_coset([v * minv % r for v in ref(x, winv)], ginv, r) for x in rows]
    if log_m:
        assert fr_ints(cp.ntt_wide(curve, a[0])) == ref(rows[0], w)
        assert (cp.ntt_wide(curve, fwd[0], inverse=True) == a[0]).all()


@pytest.mark.parametrize("curve", IDS)
def test_domain_fft(curve):
    C = pu.CURVES[curve]
    for min_size, kind in ((72, 2), (64, 0)):
        dom = po.make_evaluation_domain(C, min_size)
        assert (dom.kind, dom.m) == (kind, min_size) == cp.domain_choice(min_size, 32)
        x = _vec(curve, 300 + min_size, dom.m)
        om, sh = limbs(dom.omega, 4), limbs(dom.shift, 4)
        got = cp.domain_fft(curve, dom.kind, fr_arr(x), om, sh)
        assert fr_ints(got) == dom.fft(x) == [po.poly_eval(x, e, C.r) for e in dom.elements()]
        assert fr_ints(cp.domain_fft(curve, dom.kind, fr_arr(x), om, sh, inverse=True)) == dom.inverse_fft(x)
        assert fr_ints(cp.domain_fft(curve, dom.kind, got, om, sh, inverse=True)) == x


@pytest.mark.parametrize("curve", IDS)
def test_fr_vec_horner_and_poly_mul(curve):
    r = pu.CURVES[curve].r
    n = 67
    a, b, c = _vec(curve, 400, n), _vec(curve, 401, n)[::-1], _vec(curve, 402, n)
    c[5] = c[6] = 0                                                  # a zero divisor: the quotient is 0, as the argument loops take it
    A = fr_arr
    ops = {0: lambda x, y, z: x + y, 1: lambda x, y, z: x - y, 2: lambda x, y, z: x * y, 3: lambda x, y, z: x * b[0], 4: lambda x, y, z: x * y * po.inv0(z, r)}
    for op, fn in ops.items():
        got = cp.fr_vec(curve, op, A(a), A(b[:1]) if op == 3 else A(b), A(c) if op == 4 else None)
        assert fr_ints(got) == [fn(x, y, z) % r for x, y, z in zip(a, b, c)], op
    assert fr_ints(cp.fr_mul(curve, limbs(r - 1, 4), limbs(r - 1, 4))) == [1]
    assert fr_ints(cp.fr_mul(curve, limbs(a[0], 4), limbs(1 << 254, 4))) == [a[0] * (1 << 254) % r]
    for z in (0, 1, r - 1, a[3], 1 << 254):
        assert cp.poly_eval(curve, A(a), z) == po.poly_eval(a, z, r)
    big = _vec(curve, 403, 1500)                                     # more coefficients than threads x a few: every partial sum in play
    assert cp.poly_eval(curve, A(big), a[9]) == po.poly_eval(big, a[9], r)
    for la, lb in ((1, 1), (1, 67), (33, 32), (67, 62), (67, 63)):   # 128 and 129 output coefficients: either side of a transform size
        assert fr_ints(cp.poly_mul(curve, A(a[:la]), A(b[:lb]))) == po.poly_mul(a[:la], b[:lb], r), (la, lb)
    assert fr_ints(cp.poly_sub(curve, A(a), A(b[:9]))) == po.poly_sub(a, b[:9], r)
    assert fr_ints(cp.poly_scale(curve, A(a), r - 1)) == po.poly_scale(a, r - 1, r)
    # the random stream of the id: the 256-bit draws reduced by ITS r
    rng = po.SplitMix64(77)
    assert fr_ints(cp.random_fr(curve, 77, 50)) == [rng.next_mod(r) for _ in range(50)]


@pytest.mark.parametrize("curve", IDS)
def test_fri_fold_and_divisions(curve):
    C = pu.CURVES[curve]
    r = C.r
    A = fr_arr
    for log_size in (1, 4, 8):
        f = _vec(curve, 500 + log_size, 1 << log_size)
        w = C.root_of_unity(log_size)
        for alpha in (0, 1, r - 1, f[0] or 5):
            assert fr_ints(cp.fold_polynomial_dfs(curve, A(f), alpha, w)) == po.fold_polynomial_dfs(f, alpha, w, r), (log_size, alpha)
    f = _vec(curve, 510, 301)
    for z in (0, 1, r - 1, f[7], 1 << 254):
        q, rem = cp.poly_div_linear(curve, A(f), z)
        wq, wr = po.poly_divmod(f, [(-z) % r, 1], r)
        assert rem == po.poly_eval(f, z, r) == (wr[0] if po.poly_trim(wr) else 0)
        assert fr_ints(q) == (list(wq) + [0] * 300)[:300]
    exact = po.poly_mul(f, [(-f[7]) % r, 1], r)
    q, rem = cp.poly_div_linear(curve, A(exact), f[7])
    assert rem == 0 and fr_ints(q) == f
    assert fr_ints(cp.poly_div_exact_by_roots(curve, A(po.poly_mul(exact, [(-3) % r, 1], r)), [3, f[7]])) == f
    # by X^n - 1: exact (through quotient_polynomial, weights included) and with a remainder that is refused
    n = 16
    quot = _vec(curve, 511, 37)
    F0 = po.poly_mul(quot, [r - 1] + [0] * (n - 1) + [1], r)
    F1 = po.poly_mul(quot[:5], [r - 1] + [0] * (n - 1) + [1], r)
    a0, a1 = f[1], f[2]
    want = po.poly_trim(po.poly_add(po.poly_scale(quot, a0, r), po.poly_scale(quot[:5], a1, r), r))
    assert fr_ints(cp.quotient_polynomial(curve, [A(F0), A(F1)], [a0, a1], n)) == want
    F0[3] = (F0[3] + 1) % r
    with pytest.raises(AssertionError):
        cp.quotient_polynomial(curve, [A(F0)], [1], n)


@pytest.mark.parametrize("curve,log_n,k", [(2, 6, 3), (3, 8, 2)])
def test_permutation_grand_product(curve, log_n, k):
    C = pu.CURVES[curve]
    r, n = C.r, 1 << log_n
    usable = n - 3
    rng = po.SplitMix64(600 + curve)
    cols, sid, ssig = permutation_instance(C, rng, log_n, k, usable)
    beta, gamma = rng.next_mod(r), rng.next_mod(r)
    A = fr_arr
    for variant in (0, 1):
        if variant:
            cols[1][40] = (-(beta * ssig[1][40] + gamma)) % r        # h_1[40] = 0: the row's ratio is 0
        g, h, V = po.permutation_grand_product(cols, sid, ssig, beta, gamma, r)
        assert (V[usable] == 1) if not variant else (V[40] != 0 and V[41:] == [0] * (n - 41))
        gg, gh, gv = cp.permutation_grand_product(curve, [A(c) for c in cols], [A(c) for c in sid], [A(c) for c in ssig], beta, gamma)
        assert fr_ints(gv) == V, variant
        assert [fr_ints(x) for x in gg] == g and [fr_ints(x) for x in gh] == h
    cols, sid, ssig = permutation_instance(C, rng, log_n, k, usable)
    q_last = [1 if j == usable else 0 for j in range(n)]
    q_blind = [1 if j > usable else 0 for j in range(n)]
    L0 = [1] + [0] * (n - 1)
    if log_n <= 6:                                                   # the whole argument over the id's transforms, the dense way
        want = po.permutation_argument(cols, sid, ssig, q_last, q_blind, L0, beta, gamma, C.root_of_unity, r)
        got = cp.permutation_argument(curve, [A(c) for c in cols], [A(c) for c in sid], [A(c) for c in ssig], A(q_last), A(q_blind), A(L0), beta, gamma)
        assert fr_ints(got[0]) == want[0] and [fr_ints(f) for f in got[1]] == want[1]


@pytest.mark.parametrize("curve,log_n,k_in,k_val", [(3, 6, 2, 1), (2, 8, 1, 2)])
def test_lookup_grand_product(curve, log_n, k_in, k_val):
    C = pu.CURVES[curve]
    r, n = C.r, 1 << log_n
    rng = po.SplitMix64(700 + curve)
    inputs, values, usable = lookup_instance(C, rng, log_n, k_in, k_val)
    sorted_ = po.lookup_sort_polynomials(inputs, values, n, usable)
    A = fr_arr
    s2 = cp.lookup_sort_polynomials([A(x) for x in inputs], [A(x) for x in values], n, usable)
    assert [fr_ints(x) for x in s2] == sorted_
    beta, gamma = rng.next_mod(r), rng.next_mod(r)
    V = po.lookup_grand_product(inputs, values, sorted_, beta, gamma, usable, r)
    assert V[usable] == 1
    assert fr_ints(cp.lookup_grand_product(curve, [A(x) for x in inputs], [A(x) for x in values], s2, beta, gamma, usable)) == V
    if curve == 2:
        return
    # a sorted column that is no permutation of the rest (the product does not close) and a zero in h at row 20
    part1 = (1 + beta) * gamma % r
    bad = [list(x) for x in sorted_]
    bad[0][20] = (-(part1 + beta * bad[0][21])) % r
    V = po.lookup_grand_product(inputs, values, bad, beta, gamma, usable, r)
    assert V[20] != 0 and V[21:] == [0] * (n - 21)
    assert fr_ints(cp.lookup_grand_product(curve, [A(x) for x in inputs], [A(x) for x in values], [A(x) for x in bad], beta, gamma, usable)) == V


# ---- what is refused -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [4, 7, -1, 1 << 20])
def test_an_unknown_id_raises(curve):
    z4 = np.zeros((2, 4), dtype=np.uint64)
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    pts = np.zeros((2, 8), dtype=np.uint64)
    calls = [lambda: cp.random_fr(curve, 1, 2), lambda: cp.fr_mul(curve, one, one), lambda: cp.fr_horner(curve, z4, one), lambda: cp.ntt(curve, z4.reshape(1, 2, 4), 1, one),
             lambda: cp.ntt_wide(curve, z4), lambda: cp.fr_vec(curve, 0, z4, z4), lambda: cp.poly_mul(curve, z4 + 1, z4 + 1), lambda: cp.fold_polynomial_dfs(curve, z4, 1, 1),
             lambda: cp.poly_div_linear(curve, z4, 1), lambda: cp.toy_root(curve)(z4, 1), lambda: cp.domain_fft(curve, 0, z4, one),
             lambda: cp.permutation_grand_product(curve, [z4], [z4], [z4], 1, 1), lambda: cp.lookup_grand_product(curve, [z4], [z4], [z4, z4], 1, 1, 1),
             lambda: cp.quotient_polynomial(curve, [np.ones((5, 4), dtype=np.uint64)], [1], 2),
             lambda: cp.msm(curve, 1, pts, z4), lambda: cp.msm(curve, 1, pts, z4, naive=True), lambda: cp.batch_mul(curve, 1, z4), lambda: cp.Bases(curve, 1, pts),
             lambda: cp.point_add(curve, 1, pts[0], 1, pts[1], 1), lambda: cp.jac_to_affine(curve, 1, np.zeros(12, dtype=np.uint64)),
             lambda: cp.bases_fold(curve, pts, pts, one), lambda: cp.Groth16(curve, 4, 1, 1)]
    for i, call in enumerate(calls):
        with pytest.raises(Exception):
            call()
            pytest.fail(f"call {i} accepted curve id {curve}")


def test_the_library_itself_refuses():
    """below cport's own tables: every exported entry point that takes a curve id answers -1 (a null handle) for one it does not know, and
    leaves its output alone"""
    import ctypes
    L = cp.lib()
    buf = np.full(64, 0xAB, dtype=np.uint64)
    p, z = cp._p(buf), ctypes.c_size_t
    for curve in (4, -1):
        assert L.zko_random_fr(curve, ctypes.c_uint64(1), z(2), p) == -1
        assert L.zko_fr_mul(curve, p, p, p) == -1
        assert L.zko_fr_horner(curve, p, z(2), p, p) == -1
        assert L.zko_ntt(curve, p, z(1), z(1), p, 0, None) == -1
        assert L.zko_msm(curve, 1, p, None, p, z(1), 1, p, p) == -1
        assert L.zko_bases_fold(curve, p, None, p, None, p, z(1), p, p) == -1
        assert not L.zko_bases_new(curve, 1, p, None, z(1))
        assert not L.zko_g16_new(curve, z(4), z(1), ctypes.c_uint64(1))
        assert (buf == 0xAB).all()
    for curve in (2, 3):
        assert L.zko_msm(curve, 2, p, None, p, z(1), 1, p, p) == -1
        assert L.zko_batch_mul(curve, 2, None, p, z(1), p, p) == -1
        assert not L.zko_bases_new(curve, 2, p, None, z(1))
        assert not L.zko_g16_new(curve, z(4), z(1), ctypes.c_uint64(1))
        assert (buf == 0xAB).all()


@pytest.mark.parametrize("curve", IDS)
def test_g2_and_groth16_raise_on_a_pasta_id(curve):
    z4 = np.zeros((2, 4), dtype=np.uint64)
    pts = np.zeros((2, 16), dtype=np.uint64)
    for call in (lambda: cp.msm(curve, 2, pts, z4), lambda: cp.batch_mul(curve, 2, z4), lambda: cp.Bases(curve, 2, pts), lambda: cp.point_add(curve, 2, pts[0], 0, pts[1], 0),
                 lambda: cp.jac_to_affine(curve, 2, np.zeros(24, dtype=np.uint64)), lambda: cp.Groth16(curve, 4, 1, 1)):
        with pytest.raises(ValueError):
            call()
