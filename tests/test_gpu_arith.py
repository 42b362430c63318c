"""The arithmetic core as the kernels run it -- inline-asm Montgomery products at -O3 on gfx950, the lane-pair Fq2 type of the G2 bucket
kernel, the signed-digit recoding, the XYZZ group law -- through tests/cpp/libarithdev.so, against the oracle and, limb for limb,
against the C++ bodies built for the CPU (libzkhip_hosttest.so).  Operands sit at the edges of fu.hpp's written contract
(tests/arith_cases.py), where end-to-end tests on random residues never go."""
import ctypes
import os
import random

import numpy as np
import pytest

import arith_cases as ac
import pyoracle as po
from harness import library
from util import CURVES, FQ_LIMBS, jac_to_affine_py, pt_from_limbs, pts_arr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SO = os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_hosttest.so")
RECODE_STRIDE = 130
P = ac._ptr


@pytest.fixture(scope="module")
def dev():
    return library("libarithdev.so")


@pytest.fixture(scope="module")
def host():
    assert os.path.exists(HOST_SO), "crypto3-zk_amd/libzkhip_hosttest.so is missing: python -c 'import __graft_entry__ as g; g.build()'"
    return ctypes.CDLL(HOST_SO)


def _u32(v, n32):
    return np.array([(v >> (32 * i)) & 0xFFFFFFFF for i in range(n32)], dtype=np.uint32)


def _int(a):
    return sum(int(x) << (32 * i) for i, x in enumerate(a))


@pytest.mark.parametrize("t", [6, 7, 8, 9])
def test_raw_fu_ops_match_oracle_and_host_bodies(dev, host, t):
    """every raw Fu op on the device: (i) the oracle residue, (ii) the written postcondition (exact a + b and a + K p - b, normalised
    limbs, products < 2p), (iii) the C++ body's limbs bit for bit (fu.hpp: the asm blocks claim bit-identical results)"""
    for op, k, cases in ac.raw_suite(t, seed=1):
        ops = list(zip(*cases))
        rc, got = ac.run_raw(dev.zkd_fu_raw, t, op, *ops, size_t=False)
        assert rc == 0, (t, op, rc)
        rc, ref = ac.run_raw(host.zkt_fu_raw, t, op, *ops)
        assert rc == 0
        for case, r, h in zip(cases, got, ref):
            err = ac.check_raw(t, op, *case, r, k=k)
            assert err is None, (t, op, k, err, [hex(ac.value(x)) for x in case], r)
            assert r == h, ("device limbs differ from the C++ body", t, op, k, [hex(ac.value(x)) for x in case], r, h)
    z = [[0] * ac.TYPES[t][1]]
    assert ac.run_raw(dev.zkd_fu_raw, t, 11, z, size_t=False)[0] == -1


FIELDS = {6: (po.BLS12_381.p, 12, 1), 7: (po.BN254.p, 8, 1), 8: (po.BLS12_381.r, 8, 1), 9: (po.BN254.r, 8, 1),
          10: (po.BLS12_381.p, 12, 2), 11: (po.BN254.p, 8, 2)}


@pytest.mark.parametrize("field", [6, 7, 8, 9, 10, 11])
def test_field_op_table_on_device(dev, host, field):
    """zkt_field_op's table (op 8: the deepest lazy chain of the group law, every operand at its bound) on the device, single-lane Fu2
    included, against the oracle and the host build"""
    p, nl, deg = FIELDS[field]
    F = po.Fq2(p) if deg == 2 else None
    rng = random.Random(field)
    t = {6: 6, 7: 7, 8: 8, 9: 9, 10: 6, 11: 7}[field]
    edges = ac.canonical_edges(t)
    if deg == 1:
        vals = edges + [rng.randrange(p) for _ in range(8)]
    else:
        vals = [(0, 0), (1, 0), (0, 1), (p - 1, p - 1)] + [(edges[i], edges[-1 - i]) for i in range(len(edges))] + \
               [(rng.randrange(p), rng.randrange(p)) for _ in range(6)]
    pairs = [(a, vals[(i * 7 + 3) % len(vals)]) for i, a in enumerate(vals)]
    cw = nl * deg
    enc = (lambda x: _u32(x, nl)) if deg == 1 else (lambda x: np.concatenate([_u32(x[0], nl), _u32(x[1], nl)]))
    dec = (lambda o: _int(o)) if deg == 1 else (lambda o: (_int(o[:nl]), _int(o[nl:])))
    if deg == 1:
        mul, add, sub, sqr, neg = (lambda a, b: a * b % p), (lambda a, b: (a + b) % p), (lambda a, b: (a - b) % p), (lambda a: a * a % p), (lambda a: -a % p)
        inv, zero = (lambda a: pow(a, -1, p)), (lambda a: a == 0)
    else:
        mul, add, sub, sqr, neg, inv, zero = F.mul, F.add, F.sub, F.sqr, F.neg, F.inv, F.is_zero

    def expect(op, a, b):
        X = sub(sqr(a), add(mul(a, b), add(sqr(b), sqr(b))))
        return {0: lambda: mul(a, b), 1: lambda: add(a, b), 2: lambda: sub(a, b), 3: lambda: inv(a), 4: lambda: sqr(a), 5: lambda: neg(a),
                6: lambda: add(a, a), 7: lambda: sub(a, b), 8: lambda: mul(sub(mul(a, b), X), sub(sqr(b), X)),
                9: lambda: sqr(add(a, b)), 10: lambda: add(mul(a, add(a, b)), sqr(b)), 11: lambda: inv(a)}[op]()

    for op in range(12):
        cases = [(a, b) for a, b in pairs if op not in (3, 11) or not zero(a)]
        A = np.stack([enc(a) for a, _ in cases])
        Bv = np.stack([enc(b) for _, b in cases])
        out = np.zeros_like(A)
        assert dev.zkd_field_op(field, op, len(cases), P(A), P(Bv), P(out)) == 0
        h = np.zeros(cw, dtype=np.uint32)
        for i, (a, b) in enumerate(cases):
            assert dec(out[i]) == expect(op, a, b), (field, op, a, b)
            assert host.zkt_field_op(field, op, P(A[i]), P(Bv[i]), P(h)) == 0
            assert (h == out[i]).all()
    assert dev.zkd_field_op(field, 12, 1, P(A), P(Bv), P(out)) == -1


def _fq2_components(p, rng):
    """component values for the lane-pair Fq2 operands: fu2_pair.hpp's bounds -- affine inputs < 10p, stored X / Y < 18p, product
    operands < 34p -- at and below each, plus 0, p and random residues"""
    vals = [0, 1, p - 1, p, 2 * p - 1, 10 * p - 1, 18 * p - 1, 34 * p - 1] + [rng.randrange(34 * p) for _ in range(4)]
    return vals


@pytest.mark.parametrize("curve", [0, 1])
def test_fu2h_lane_pairs(dev, host, curve):
    """FieldOps<Fu2h> (one Fq2 component per lane of a pair, the G2 bucket kernel's type): every op against the oracle and against the
    same terms composed from the host's C++ bodies (zkt_fu_raw), limb for limb; the zero tests' pair exchange (both lanes agree)"""
    t = 6 if curve == 0 else 7
    p, L, NL = ac.TYPES[t][0], ac.TYPES[t][1], ac.TYPES[t][2]
    R = 1 << (29 * L)
    Ri = pow(R, -1, p)
    rng = random.Random(40 + curve)
    comp = _fq2_components(p, rng)
    xs = [(a, b) for a in comp for b in comp[::3]]
    pairs = [(x, xs[(i * 5 + 7) % len(xs)]) for i, x in enumerate(xs)]
    sp = lambda v: ac.split(v, L)  # noqa: E731
    for a, b in pairs:  # operand contract of the lane-pair product: both components < 34p
        assert max(a + b) < 34 * p

    def run(op, A, Bv=None, C=None, D=None):
        n = len(A)
        arrs = []
        for X in (A, Bv, C, D):
            X = X if X is not None else [(0, 0)] * n
            arrs.append(np.array([sp(x0) + sp(x1) for x0, x1 in X], dtype=np.uint32).reshape(n, 2 * L))
        out = np.zeros((n, 2 * L), dtype=np.uint32)
        assert dev.zkd_fu2h(curve, op, n, *[P(x) for x in arrs], P(out)) == 0
        return [(list(map(int, r[:L])), list(map(int, r[L:]))) for r in out]

    def raw(op, *ops):
        rc, out = ac.run_raw(host.zkt_fu_raw, t, op, *[[sp(v) for v in o] for o in ops])
        assert rc == 0
        return out

    A = [a for a, _ in pairs]
    Bv = [b for _, b in pairs]
    a0, a1 = [x[0] for x in A], [x[1] for x in A]
    b0, b1 = [x[0] for x in Bv], [x[1] for x in Bv]
    neg = lambda v: [ac.value(x) for x in raw(ac.op_sub(128), [0] * len(v), v)]  # noqa: E731
    # mul: even lane REDC(a0 b0 + (128p - a1) b1), odd lane REDC(a1 b0 + a0 b1)
    got = run(0, A, Bv)
    e0 = raw(ac.OP_MUL2, a0, b0, neg(a1), b1)
    e1 = raw(ac.OP_MUL2, a1, b0, a0, b1)
    for (x, y), g, h0, h1 in zip(pairs, got, e0, e1):
        assert g == (h0, h1), ("mul", x, y)
        c0, c1 = ac.value(g[0]), ac.value(g[1])
        assert c0 % p == (x[0] * y[0] - x[1] * y[1]) * Ri % p and c1 % p == (x[0] * y[1] + x[1] * y[0]) * Ri % p
        assert c0 < 2 * p and c1 < 2 * p and ac.normalised(g[0]) and ac.normalised(g[1])
    # sqr: even (a0 + a1)(a0 + 128p - a1), odd (2 a1) a0
    got = run(1, A)
    s = [ac.value(x) for x in raw(ac.OP_ADD, a0, a1)]
    d = [ac.value(x) for x in raw(ac.op_sub(128), a0, a1)]
    e0 = raw(ac.OP_MUL, s, d)
    e1 = raw(ac.OP_MUL, [2 * v for v in a1], a0)
    for x, g, h0, h1 in zip(A, got, e0, e1):
        assert g == (h0, h1), ("sqr", x)
        assert ac.value(g[0]) % p == (x[0] * x[0] - x[1] * x[1]) * Ri % p and ac.value(g[1]) % p == 2 * x[0] * x[1] * Ri % p
    # add, sub<K1 | K2 | K3> = sub<16 | 32 | 64>: exact per component
    got = run(2, A, Bv)
    assert all(ac.value(g[0]) == x[0] + y[0] and ac.value(g[1]) == x[1] + y[1] for (x, y), g in zip(pairs, got))
    for op, k in ((3, 16), (4, 32), (5, 64)):
        cs = [(x, y) for x, y in pairs if max(y) <= (k - 1) * p]
        got = run(op, [x for x, _ in cs], [y for _, y in cs])
        for (x, y), g in zip(cs, got):
            assert ac.value(g[0]) == x[0] + k * p - y[0] and ac.value(g[1]) == x[1] + k * p - y[1], (k, x, y)
            assert ac.normalised(g[0]) and ac.normalised(g[1])
    # mul_sub<K1>(a, b, c, d) = sub<16>(mul(a, b), mul(c, d))
    C = A[::-1]
    D = Bv[3:] + Bv[:3]
    got = run(6, A, Bv, C, D)
    m1, m2 = run(0, A, Bv), run(0, C, D)
    for g, u, v in zip(got, m1, m2):
        assert ac.value(g[0]) == ac.value(u[0]) + 16 * p - ac.value(v[0]) and ac.value(g[1]) == ac.value(u[1]) + 16 * p - ac.value(v[1])
    # zero tests: each lane writes the pair's verdict; both lanes must agree
    zs = [(0, 0), (p, 0), (0, p), (p, p), (0, 1), (1, 0), (p - 1, 1), (2 * p, 34 * p), (34 * p, 0), (0, 2 * p - 1)]
    for op, fn, cs in ((7, lambda x: x[0] % p == 0 and x[1] % p == 0, zs),
                       (8, lambda x: x[0] % p == 0 and x[1] % p == 0, [x for x in zs if max(x) < 2 * p]),
                       (9, lambda x: x == (0, 0), zs)):
        got = run(op, cs)
        for x, g in zip(cs, got):
            want = 1 if fn(x) else 0
            assert g[0] == [want] + [0] * (L - 1) and g[1] == [want] + [0] * (L - 1), (op, x, g)
    # to_canonical: each lane its component's canonical form (x R^-1 mod p), NL saturated words at c0 | c1
    got = run(10, A)
    for x, g in zip(A, got):
        flat = g[0] + g[1]
        assert _int(flat[:NL]) == x[0] * Ri % p and _int(flat[NL:2 * NL]) == x[1] * Ri % p, x
    # store / load through the device-buffer layout
    got = run(11, A)
    assert all(g == (sp(x[0]), sp(x[1])) for x, g in zip(A, got))
    assert dev.zkd_fu2h(curve, 12, 0, None, None, None, None, None) == -1


@pytest.mark.parametrize("curve_id,curve", [(0, po.BLS12_381), (1, po.BN254)])
def test_recode_on_device(dev, host, curve_id, curve):
    """msm_fold_scalar + msm_recode as msm_digits_only runs them, every window size from 2 to ZK_MSM_MAX_C = 21: the host twin's digits,
    the scalar back mod r, |digit| <= 2^(width - 1), no carry out of the top window"""
    r = curve.r
    tb = r.bit_length()
    for c in range(2, 22):
        rng = random.Random(c)
        vals = ac.scalar_edges(r, c, rng)
        S = np.stack([_u32(v, 8) for v in vals])
        dig = np.zeros((len(vals), RECODE_STRIDE), dtype=np.int32)
        assert dev.zkd_recode_folded(curve_id, c, len(vals), P(S), P(dig)) == 0
        W = (tb + c - 1) // c
        off = [w * tb // W for w in range(W + 1)]
        ref = np.zeros(140, dtype=np.int32)
        for v, d in zip(vals, dig):
            assert d[128] == W and d[129] == 0, (c, hex(v))
            assert host.zkt_recode_folded(curve_id, P(_u32(v, 8)), c, P(ref)) == W
            assert (d[:W] == ref[:W]).all(), (c, hex(v))
            assert all(abs(int(x)) <= 1 << (off[w + 1] - off[w] - 1) for w, x in enumerate(d[:W])), (c, hex(v))
            got = sum(int(x) << off[w] for w, x in enumerate(d[:W]))
            assert got % r == v % r and abs(got) <= (r - 1) // 2, (c, hex(v))
    assert dev.zkd_recode_folded(0, 22, 1, P(S), P(dig)) == -1


def _chain(fn, field, curve, group, pts, infs, negs, mode, k=0):
    arr = pts_arr(curve, group, pts).view(np.uint32).reshape(len(pts), -1) if len(pts) else np.zeros((0, 1), dtype=np.uint32)
    arr = np.ascontiguousarray(arr)
    out = np.zeros((3 if mode == 3 else 2) * FQ_LIMBS[curve] * group * 2, dtype=np.uint32)
    oinf = np.zeros(1, dtype=np.uint8)
    infa = np.array(infs + [0], dtype=np.uint8)
    nega = np.array(negs + [0], dtype=np.uint8)
    assert fn(field, P(arr), P(infa), P(nega), ctypes.c_size_t(len(pts)), mode, ctypes.c_uint32(k), P(out), P(oinf)) == 0
    return out.view(np.uint64), int(oinf[0])


@pytest.mark.parametrize("curve,group,field", [(0, 1, 6), (0, 2, 10), (1, 1, 7), (1, 2, 11)])
def test_point_chains_on_device(dev, curve, group, field):
    """test_xyzz_group_law's cases (P + P, P + (-P), infinity operands, restart after infinity) on the device: modes 0 - 4 on one lane,
    and for G2 the madd chain over Fu2h lane pairs as the bucket kernel runs it (mode 5)"""
    C = CURVES[curve]
    G = C.g1 if group == 1 else C.g2
    rng = po.SplitMix64(curve * 10 + group + 100)
    base = G.batch_mul_gen([rng.next_mod(C.r) for _ in range(6)])
    P0, P1, P2 = base[0], base[1], base[2]
    cases = [
        ([P0, P1, P2, base[3], base[4], base[5]], [0] * 6, [0, 1, 0, 1, 1, 0]),
        ([P0, P0], [0, 0], [0, 0]),
        ([P0, P0, P0, P0], [0] * 4, [0] * 4),
        ([P0, P0], [0, 0], [0, 1]),
        ([P0, P0, P1], [0, 0, 0], [0, 1, 0]),
        ([P0, P1], [1, 0], [0, 0]),
        ([], [], []),
    ]
    sgn = lambda Pt, n: G.neg(Pt) if n else Pt  # noqa: E731
    f = dev.zkd_point_chain
    for pts, infs, negs in cases:
        exp = None
        for Pt, i, n in zip(pts, infs, negs):
            if not i:
                exp = G.add(exp, sgn(Pt, n))
        for mode in ([0, 4, 5] if group == 2 else [0, 4]):
            out, oinf = _chain(f, field, curve, group, pts, infs, negs, mode)
            assert pt_from_limbs(curve, group, out, oinf) == exp, (mode, len(pts))
        if len(pts) >= 2:
            out, oinf = _chain(f, field, curve, group, pts, infs, negs, 1)
            assert pt_from_limbs(curve, group, out, oinf) == exp
            for k in (0, 1, 2, 37, 65535):
                out, oinf = _chain(f, field, curve, group, pts, infs, negs, 2, k)
                assert pt_from_limbs(curve, group, out, oinf) == G.mul(exp, k)
        out, oinf = _chain(f, field, curve, group, pts, infs, negs, 3)
        L = FQ_LIMBS[curve] * group
        if exp is None:
            assert oinf == 1 and po.from_limbs(out[2 * L:3 * L]) == 0
        else:
            assert jac_to_affine_py(curve, group, out.reshape(3, L)) == exp
    pts = [P0, P1, P0, P1]
    out, oinf = _chain(f, field, curve, group, pts, [0] * 4, [0] * 4, 1)
    assert pt_from_limbs(curve, group, out, oinf) == G.mul(G.add(P0, P1), 2)
    out, oinf = _chain(f, field, curve, group, pts, [0] * 4, [0, 0, 1, 1], 1)
    assert oinf == 1


@pytest.mark.parametrize("curve,group,field", [(0, 1, 6), (0, 2, 10), (1, 1, 7), (1, 2, 11)])
def test_parked_points_share_one_inversion_on_device(dev, host, curve, group, field):
    """xyzz_park / xyzz_parked_to_affine (curve.hpp) on one lane: parked_cases.py's chains -- every prefix against big integers, both
    layouts -- and limb for limb what the host build of the same code gives"""
    import parked_cases
    C = CURVES[curve]
    G = C.g1 if group == 1 else C.g2
    rng = po.SplitMix64(curve * 10 + group + 300)
    base = G.batch_mul_gen([rng.next_mod(C.r) for _ in range(4)])
    got = parked_cases.check(dev.zkd_parked_affine, field, curve, group, G, base)
    ref = parked_cases.check(host.zkt_parked_affine, field, curve, group, G, base)
    for (o, i), (ho, hi) in zip(got, ref):
        assert (o == ho).all() and (i == hi).all()
