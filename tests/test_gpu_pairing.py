"""zkhip_pairing_products on the GPU: out[k] = final_exponentiation(prod miller(P_i, Q_i)) over the terms naming k (include/zkhip.h, "pairing
products"; csrc/pairing.hip).

Checked against the reference's own vectors (tests/golden/ref_ipp2_kat.json: kzg_ipp2::single as 2 terms / 2 outputs, ::pair as 4 terms /
2 outputs), against the big-integer model (tests/pairing_ref.py) on unstructured pairs, and at larger sizes by structure: with
P_i = a_i G1 and Q_i = b_i G2 built on the device, the product is the model's e(G1, G2)^(sum a_i b_i mod r) -- one exponentiation on the
oracle side whatever n is.  Sizes: 63 / 64 / 65 around the 64-lane workgroup of the Miller kernel (one pair per lane), 257 (several
workgroups, not a power of two), 1100 (more than the 16 tiles one workgroup of the product kernel takes: two partials for one output),
1024 / 1025 (exactly 16 tiles and one more), and more than 64 partials -- 70 one-pair terms into three outputs, one term of 65537 pairs --
where a lane of the final kernel multiplies several (tests/THRESHOLDS.md)."""
import ctypes
import json
import random

import numpy as np
import pytest

import pairing_ref as pr
import pyoracle as po
from test_host_pairing import SO, host_products
from test_pairing_ref import KAT, load_kat

pytestmark = pytest.mark.gpu

BLS, G1, G2 = 0, 1, 2
INVALID, RANGE = -2, -5
R = pr.R
ONE = pr.to_canonical(pr.ONE)
g1, g2 = po.BLS12_381.g1, po.BLS12_381.g2


def fr_arr(vals):
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def gt_ints(row):
    return [sum(int(x) << (64 * i) for i, x in enumerate(row[k * 6:(k + 1) * 6])) for k in range(12)]


def fq_limbs(v):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]


def upload_g1(ctx, pts):
    arr = np.array([fq_limbs(p[0]) + fq_limbs(p[1]) if p is not None else [0] * 12 for p in pts], dtype=np.uint64)
    return ctx.upload_bases(BLS, G1, arr, np.array([p is None for p in pts], dtype=np.uint8))


def upload_g2(ctx, pts):
    arr = np.array([fq_limbs(q[0][0]) + fq_limbs(q[0][1]) + fq_limbs(q[1][0]) + fq_limbs(q[1][1]) if q is not None else [0] * 24 for q in pts], dtype=np.uint64)
    return ctx.upload_bases(BLS, G2, arr, np.array([q is None for q in pts], dtype=np.uint8))


def structured(ctx, seed, n, zero_a=(), zero_b=()):
    """(bases of a_i G1, bases of b_i G2, a, b); a zero scalar is a point at infinity"""
    rnd = random.Random(seed)
    a = [0 if i in zero_a else rnd.randrange(1, R) for i in range(n)]
    b = [0 if i in zero_b else rnd.randrange(1, R) for i in range(n)]
    return ctx.bases_from_scalars(BLS, G1, fr_arr(a)), ctx.bases_from_scalars(BLS, G2, fr_arr(b)), a, b


def dot(a, b):
    return sum(x * y for x, y in zip(a, b)) % R


@pytest.fixture(scope="module")
def kat(ctx):
    a, b, v1, v2, w1, w2, exp = load_kat()
    k = dict(a=upload_g1(ctx, a), b=upload_g2(ctx, b), v1=upload_g2(ctx, v1), v2=upload_g2(ctx, v2), w1=upload_g1(ctx, w1), w2=upload_g1(ctx, w2), exp=exp)
    yield k
    for name in ("a", "b", "v1", "v2", "w1", "w2"):
        k[name].free()


def test_single_equals_the_reference_vectors(ctx, kat):
    out = ctx.pairing_products([(kat["a"], 0, kat["v1"], 0, 10, 0), (kat["a"], 0, kat["v2"], 0, 10, 1)], 2)
    assert gt_ints(out[0]) == kat["exp"]["single_first"] and gt_ints(out[1]) == kat["exp"]["single_second"]


def test_pair_equals_the_reference_vectors(ctx, kat):
    out = ctx.pairing_products([(kat["a"], 0, kat["v1"], 0, 10, 0), (kat["w1"], 0, kat["b"], 0, 10, 0),
                                (kat["a"], 0, kat["v2"], 0, 10, 1), (kat["w2"], 0, kat["b"], 0, 10, 1)], 2)
    assert gt_ints(out[0]) == kat["exp"]["pair_first"] and gt_ints(out[1]) == kat["exp"]["pair_second"]


def test_keys_built_on_the_device_give_the_same_commitment(ctx, kat):
    u = int(json.load(open(KAT))["u"], 16)
    v1 = ctx.bases_from_scalars(BLS, G2, fr_arr([pow(u, i, R) for i in range(10)]))
    try:
        out = ctx.pairing_products([(kat["a"], 0, v1, 0, 10, 0)], 1)
        assert gt_ints(out[0]) == kat["exp"]["single_first"]
    finally:
        v1.free()


@pytest.mark.parametrize("n", [1, 2, 3])
def test_unstructured_pairs_against_the_model(ctx, n):
    rnd = random.Random(40 + n)
    pairs = [(g1.mul(g1.gen, rnd.randrange(1, R)), g2.mul(g2.gen, rnd.randrange(1, R))) for _ in range(n)]
    p, q = upload_g1(ctx, [x for x, _ in pairs]), upload_g2(ctx, [y for _, y in pairs])
    try:
        assert gt_ints(ctx.pairing_products([(p, 0, q, 0, n, 0)], 1)[0]) == pr.pairing_product(pairs)
    finally:
        p.free(), q.free()


@pytest.mark.parametrize("n", [63, 64, 65, 257, 1100])
def test_structured_products(ctx, n):
    p, q, a, b = structured(ctx, 50 + n, n)
    try:
        assert gt_ints(ctx.pairing_products([(p, 0, q, 0, n, 0)], 1)[0]) == pr.structured_expectation(dot(a, b))
    finally:
        p.free(), q.free()


@pytest.mark.parametrize("n", [1024, 1025])
def test_structured_products_at_the_product_workgroup_boundary(ctx, n):
    """a workgroup of pairing_product_blocks takes PROD_TILES = 16 tiles of 64 pairs: 1024 pairs fill one exactly, the 1025th opens a second
    workgroup with one tile of one live lane"""
    p, q, a, b = structured(ctx, 50 + n, n)
    try:
        assert gt_ints(ctx.pairing_products([(p, 0, q, 0, n, 0)], 1)[0]) == pr.structured_expectation(dot(a, b))
    finally:
        p.free(), q.free()


def test_seventy_terms_into_three_outputs_with_empty_terms_in_the_table(ctx):
    """70 terms of one pair each, term t into output t mod 3 of 4, with a zero-length term in front of them and one in the middle of the
    table (find_term walks past a term without tiles to the one that owns the workgroup).  70 partials reach pairing_product_final: more
    than its 64 lanes, so lanes 0 .. 5 take two each (the stride loop), and every lane skips the partials of the other outputs.  Output k is
    e(G1, G2)^(sum of a_t b_t over its terms); output 3, which only an empty term names, is one."""
    n = 70
    p, q, a, b = structured(ctx, 170, n)
    terms = [(p, t, q, t, 1, t % 3) for t in range(n)]
    terms.insert(0, (p, 0, q, 0, 0, 3))
    terms.insert(35, (p, 7, q, 9, 0, 1))
    assert len(terms) == 72 and terms[0][4] == 0 and terms[35][4] == 0 and sum(t[4] for t in terms) == n
    try:
        out = ctx.pairing_products(terms, 4)
        for k in range(3):
            assert gt_ints(out[k]) == pr.structured_expectation(dot(a[k::3], b[k::3])) != ONE, k
        assert gt_ints(out[3]) == ONE
    finally:
        p.free(), q.free()


def test_one_term_of_65537_pairs(ctx):
    """1025 tiles, 65 partials of ONE output: lane 0 of pairing_product_final multiplies two.  Then with infinity at pair 65536 -- the only
    pair of the last tile, workgroup and partial, which is then one."""
    n = 65537
    p, q, a, b = structured(ctx, 171, n)
    a2 = a[:n - 1] + [0]
    p2 = ctx.bases_from_scalars(BLS, G1, fr_arr(a2))
    try:
        assert gt_ints(ctx.pairing_products([(p, 0, q, 0, n, 0)], 1)[0]) == pr.structured_expectation(dot(a, b))
        got = gt_ints(ctx.pairing_products([(p2, 0, q, 0, n, 0)], 1)[0])
        assert got == pr.structured_expectation(dot(a2, b)) == pr.structured_expectation(dot(a[:n - 1], b[:n - 1]))
    finally:
        p.free(), q.free(), p2.free()


def test_structured_product_that_cancels(ctx):
    """n = 65 with b[64] chosen so that sum a_i b_i = 0 mod r: the pair that cancels the first workgroup's 64 sits in the second"""
    n = 65
    rnd = random.Random(55)
    a = [rnd.randrange(1, R) for _ in range(n)]
    b = [rnd.randrange(1, R) for _ in range(n - 1)]
    b.append((-dot(a[:64], b)) * pow(a[64], -1, R) % R)
    assert b[64] != 0 and dot(a, b) == 0 and dot(a[:64], b[:64]) != 0
    p, q = ctx.bases_from_scalars(BLS, G1, fr_arr(a)), ctx.bases_from_scalars(BLS, G2, fr_arr(b))
    try:
        out = ctx.pairing_products([(p, 0, q, 0, n, 0), (p, 0, q, 0, 64, 1)], 2)
        assert gt_ints(out[0]) == ONE
        assert gt_ints(out[1]) == pr.structured_expectation(dot(a[:64], b[:64])) != ONE
    finally:
        p.free(), q.free()


def test_explicit_pairs_that_cancel_and_a_repeated_pair(ctx):
    """e(P, Q) e(-P, Q) = e(P, Q) e(P, -Q) = 1 with the negations made by hand on the coordinates (y, respectively y.c0 and y.c1), and
    e(P, Q)^2 from the same pair twice"""
    rnd = random.Random(56)
    Pt, Q = g1.mul(g1.gen, rnd.randrange(1, R)), g2.mul(g2.gen, rnd.randrange(1, R))
    neg_P = (Pt[0], pr.P - Pt[1])
    neg_Q = (Q[0], (pr.P - Q[1][0], pr.P - Q[1][1]))
    assert g1.on_curve(neg_P) and g2.on_curve(neg_Q) and g1.add(Pt, neg_P) is None and g2.add(Q, neg_Q) is None
    p, q = upload_g1(ctx, [Pt, neg_P, Pt, Pt]), upload_g2(ctx, [Q, Q, neg_Q])
    try:
        # [(P, Q), (-P, Q)], [(P, Q), (P, -Q)], [(P, Q), (P, Q)], [(P, Q)]
        out = ctx.pairing_products([(p, 0, q, 0, 2, 0), (p, 2, q, 1, 2, 1), (p, 2, q, 0, 2, 2), (p, 0, q, 0, 1, 3)], 4)
        assert gt_ints(out[0]) == ONE and gt_ints(out[1]) == ONE
        single = pr.pairing_product([(Pt, Q)])
        assert gt_ints(out[3]) == single != ONE
        assert gt_ints(out[2]) == pr.pairing_product([(Pt, Q), (Pt, Q)])
        e = pr.from_canonical(single)
        assert gt_ints(out[2]) == pr.to_canonical(pr.f12_mul(e, e))
    finally:
        p.free(), q.free()


def test_infinity_placement(ctx):
    """infinity at the first, last and a middle index in G1, in G2, and in both at one index; an output whose pairs are all at infinity and
    one that no term names are one"""
    n = 70
    p, q, a, b = structured(ctx, 60, n, zero_a=(0, 33, 69, 7), zero_b=(1, 34, 68, 7))
    pz, qz, _, _ = structured(ctx, 61, 3, zero_a=(0, 1), zero_b=(2,))
    try:
        out = ctx.pairing_products([(p, 0, q, 0, n, 0), (pz, 0, qz, 0, 3, 2)], 4)
        assert gt_ints(out[0]) == pr.structured_expectation(dot(a, b))
        assert gt_ints(out[1]) == ONE and gt_ints(out[2]) == ONE and gt_ints(out[3]) == ONE
    finally:
        for x in (p, q, pz, qz):
            x.free()


def test_offsets_and_two_terms_of_different_length_into_one_output(ctx):
    p, q, a, b = structured(ctx, 70, 150)
    try:
        out = ctx.pairing_products([(p, 5, q, 40, 66, 1), (p, 100, q, 3, 9, 1), (p, 149, q, 0, 1, 0), (p, 0, q, 0, 0, 0)], 2)
        assert gt_ints(out[1]) == pr.structured_expectation(dot(a[5:71], b[40:106]) + dot(a[100:109], b[3:12]))
        assert gt_ints(out[0]) == pr.structured_expectation(a[149] * b[0])
    finally:
        p.free(), q.free()


def test_equals_the_host_twin_bit_for_bit(ctx):
    n = 65
    p, q, a, b = structured(ctx, 80, n, zero_a=(64,))
    try:
        got = gt_ints(ctx.pairing_products([(p, 0, q, 0, n, 0)], 1)[0])
        (P1, i1), (P2, i2) = p.download(), q.download()
    finally:
        p.free(), q.free()
    ints = lambda row, k: tuple(sum(int(x) << (64 * i) for i, x in enumerate(row[j * 6:(j + 1) * 6])) for j in range(k))
    pts1 = [None if f else ints(r, 2) for r, f in zip(P1, i1)]
    pts2 = [None if f else (lambda c: ((c[0], c[1]), (c[2], c[3])))(ints(r, 4)) for r, f in zip(P2, i2)]
    assert host_products(ctypes.CDLL(SO), [list(zip(pts1, pts2))], [0], 1) == [got]


def test_refusals(zk, ctx):
    """every error row of the header, before anything is launched: the profiler has counted no launch and the context works afterwards"""
    p, q, a, b = structured(ctx, 90, 10)
    pn = ctx.bases_from_scalars(1, G1, fr_arr([1, 2]))  # BN254
    L, h, z = ctx.lib, ctx.h, ctypes.c_size_t
    out = np.zeros((2, 72), dtype=np.uint64)
    op = out.ctypes.data_as(ctypes.c_void_p)

    def terms(*rows):
        arr = (zk.PairingTerm * len(rows))()
        for t, (x, o1, y, o2, n, k) in zip(arr, rows):
            t.g1, t.g1_offset, t.g2, t.g2_offset, t.n, t.out = (x.h.value if x else None), o1, (y.h.value if y else None), o2, n, k
        return arr

    ok = terms((p, 0, q, 0, 10, 0))
    call = lambda ch, curve, t, nt, no, o: L.zkhip_pairing_products(ch, curve, t, z(nt), z(no), o)
    rows = [
        ("null ctx", INVALID, lambda: call(None, BLS, ok, 1, 1, op)),
        ("null out", INVALID, lambda: call(h, BLS, ok, 1, 1, None)),
        ("null terms", INVALID, lambda: call(h, BLS, None, 1, 1, op)),
        ("null g1", INVALID, lambda: call(h, BLS, terms((None, 0, q, 0, 10, 0)), 1, 1, op)),
        ("null g2", INVALID, lambda: call(h, BLS, terms((p, 0, None, 0, 10, 0)), 1, 1, op)),
        ("unknown curve", INVALID, lambda: call(h, 7, ok, 1, 1, op)),
        ("BN254", INVALID, lambda: call(h, 1, ok, 1, 1, op)),
        ("Pallas", INVALID, lambda: call(h, 2, ok, 1, 1, op)),
        ("Vesta", INVALID, lambda: call(h, 3, ok, 1, 1, op)),
        ("G2 bases in the G1 slot", INVALID, lambda: call(h, BLS, terms((q, 0, q, 0, 10, 0)), 1, 1, op)),
        ("G1 bases in the G2 slot", INVALID, lambda: call(h, BLS, terms((p, 0, p, 0, 10, 0)), 1, 1, op)),
        ("bases of another curve", INVALID, lambda: call(h, BLS, terms((pn, 0, q, 0, 2, 0)), 1, 1, op)),
        ("g1 range one past the size", RANGE, lambda: call(h, BLS, terms((p, 1, q, 0, 10, 0)), 1, 1, op)),
        ("g2 range one past the size", RANGE, lambda: call(h, BLS, terms((p, 0, q, 1, 10, 0)), 1, 1, op)),
        ("g1 offset past the size", RANGE, lambda: call(h, BLS, terms((p, 11, q, 0, 0, 0)), 1, 1, op)),
        ("n wraps", RANGE, lambda: call(h, BLS, terms((p, 2, q, 0, (1 << 64) - 1, 0)), 1, 1, op)),
        ("out = n_out", RANGE, lambda: call(h, BLS, terms((p, 0, q, 0, 10, 2)), 1, 2, op)),
        ("n_out = 0", RANGE, lambda: call(h, BLS, ok, 1, 0, op)),
    ]
    try:
        L.zkhip_profile_enable(h, 1)
        L.zkhip_profile_reset(h)
        for name, code, fn in rows:
            assert fn() == code, name
        ms, launches = ctypes.c_double(), ctypes.c_uint64()
        assert L.zkhip_profile_get(h, b"", ctypes.byref(ms), ctypes.byref(launches)) == 0 and launches.value == 0
        L.zkhip_profile_enable(h, 0)
        assert gt_ints(ctx.pairing_products([(p, 0, q, 0, 10, 0)], 1)[0]) == pr.structured_expectation(dot(a, b))
        assert gt_ints(ctx.pairing_products([], 1)[0]) == ONE
    finally:
        L.zkhip_profile_enable(h, 0)
        for x in (p, q, pn):
            x.free()


def test_two_to_the_37_pairs_in_all_are_refused(ctx):
    """the header's last RANGE row: 2^20 terms of 2^17 pairs each over ONE pair of bases objects are 2^37 pairs (2^31 Miller workgroups); refused
    before anything is launched.  The term table is a 48-byte record per term, written here as one numpy array of the struct's layout."""
    n = 1 << 17
    rnd = random.Random(95)
    p = ctx.bases_from_scalars(BLS, G1, fr_arr([rnd.randrange(1, R) for _ in range(n)]))
    q = ctx.bases_from_scalars(BLS, G2, fr_arr([rnd.randrange(1, R) for _ in range(n)]))
    try:
        rec = np.dtype([("g1", "<u8"), ("g1_offset", "<u8"), ("g2", "<u8"), ("g2_offset", "<u8"), ("n", "<u8"), ("out", "<u4"), ("pad", "<u4")])
        assert rec.itemsize == ctypes.sizeof(__import__("crypto3_zk_amd").PairingTerm) == 48
        terms = np.zeros(1 << 20, dtype=rec)
        terms["g1"], terms["g2"], terms["n"] = p.h.value, q.h.value, n
        out = np.zeros(72, dtype=np.uint64)
        L, z = ctx.lib, ctypes.c_size_t
        call = lambda nt: L.zkhip_pairing_products(ctx.h, BLS, terms.ctypes.data_as(ctypes.c_void_p), z(nt), z(1), out.ctypes.data_as(ctypes.c_void_p))
        L.zkhip_profile_enable(ctx.h, 1)
        L.zkhip_profile_reset(ctx.h)
        assert call(1 << 20) == RANGE
        ms, launches = ctypes.c_double(), ctypes.c_uint64()
        assert L.zkhip_profile_get(ctx.h, b"", ctypes.byref(ms), ctypes.byref(launches)) == 0 and launches.value == 0
    finally:
        L.zkhip_profile_enable(ctx.h, 0)
        p.free(), q.free()
