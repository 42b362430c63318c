"""Pallas and Vesta without a GPU: the generated field constants, the __host__ __device__ arithmetic of their four lazy types at the edges of
fu.hpp's contract (libzkhip_hosttest.so, tests/arith_cases.py), the group law over their coordinate fields, the scalar recoding, and the
shim's host algebra over `pallas` / `vesta` (tests/cpp/pasta_test.cpp -> libpastatest.so) -- each against pyoracle's generic classes."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import arith_cases as ac
import pasta_util as pu
import pyoracle as po
from harness import library
from util import fr_arr, jac_to_affine_py, limbs, pt_from_limbs, pt_limbs, pts_arr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_hosttest.so")
P = ac._ptr


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run __graft_entry__.build()")
    return ctypes.CDLL(SO)


@pytest.fixture(scope="module")
def harness():
    return library("libpastatest.so")


def _u32(v, n32=8):
    return np.array([(v >> (32 * i)) & 0xFFFFFFFF for i in range(n32)], dtype=np.uint32)


def _int(a):
    return sum(int(x) << (32 * i) for i, x in enumerate(a))


def test_field_constants_are_what_the_generator_writes(tmp_path):
    """tools/gen_field_consts.py reproduces the committed csrc/field_consts.hpp byte for byte (run on a copy of the tree's two files)"""
    tool = tmp_path / "tools"
    dst = tmp_path / "crypto3-zk_amd" / "csrc"
    tool.mkdir()
    dst.mkdir(parents=True)
    src = open(os.path.join(ROOT, "tools", "gen_field_consts.py")).read()
    (tool / "gen_field_consts.py").write_text(src)
    subprocess.check_call([sys.executable, str(tool / "gen_field_consts.py")], stdout=subprocess.DEVNULL)
    committed = open(os.path.join(ROOT, "crypto3-zk_amd", "csrc", "field_consts.hpp")).read()
    assert (dst / "field_consts.hpp").read_text() == committed
    for name in ("PallasFq", "PallasFr", "VestaFq", "VestaFr"):
        assert f"struct {name} {{" in committed and f"struct {name}U {{" in committed


def test_modulus_limbs_have_the_shape_the_reduction_meets():
    """in 29-bit limbs both primes have limb 0 = 1, limbs 5 - 7 = 0 and a top limb of 2^22 (L = 9): the constants the unrolled reduction folds"""
    for p in (pu.P, pu.Q):
        assert po.Fq(p) and pow(2, p - 1, p) == 1 and p.bit_length() == 255
        v = ac.split(p, 9)
        assert v[0] == 1 and v[5:8] == [0, 0, 0] and v[8] == 1 << 22
        assert ac.split(p, 10)[:9] == v and ac.split(p, 10)[9] == 0
        assert 65 * p < 1 << 261 < 129 * p      # 64 p is the largest spread constant of the scalar role


@pytest.mark.parametrize("t", [16, 17, 18, 19])
def test_raw_limbs_at_the_contract_bounds(shim, t):
    """zkt_fu_raw over arith_cases' contract-edge suites -- mul, sqr, mul2, add, every sub<K> the type has, canon, both inverses, pack / unpack --
    against Python integers and the written postconditions"""
    L = ac.TYPES[t][1]
    counted = 0
    subs = []
    for op, k, cases in ac.raw_suite(t):
        rc, out = ac.run_raw(shim.zkt_fu_raw, t, op, *zip(*cases))
        assert rc == 0, (t, op)
        for case, r in zip(cases, out):
            err = ac.check_raw(t, op, *case, r, k=k)
            assert err is None, (t, op, k, err, [hex(ac.value(x)) for x in case], r)
        counted += len(cases)
        if k:
            subs.append(k)
    assert counted > 700
    assert subs == ([2, 4, 8, 16, 32, 64, 128] if t in (16, 17) else [2, 4, 8, 16, 32, 64])
    z = [[0] * L]
    assert ac.run_raw(shim.zkt_fu_raw, t, 11, z)[0] == -1     # no such op
    assert ac.run_raw(shim.zkt_fu_raw, 12, 0, z)[0] == -1     # a saturated type has no raw limbs
    if t in (18, 19):                                         # the scalar role has no 128 p spread constant
        assert ac.run_raw(shim.zkt_fu_raw, t, ac.op_sub(128), z)[0] == -1
    # fu_reduce_small is sized for the 9-limb scalar role: there it ran above over every value of its quotient estimate's input
    assert (ac.OP_REDUCE_SMALL in [op for op, _, _ in ac.raw_suite(t)]) == (L == 9) == (ac.run_raw(shim.zkt_fu_raw, t, ac.OP_REDUCE_SMALL, z)[0] == 0)


FIELDS = {12: pu.P, 13: pu.Q, 14: pu.Q, 15: pu.P, 16: pu.P, 17: pu.Q, 18: pu.Q, 19: pu.P}


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_field_op_table(shim, field):
    """zkt_field_op's table (op 8: the deepest lazy chain of the group law) for the saturated and the lazy types of both primes in both roles"""
    p = FIELDS[field]
    rng = random.Random(field)
    edges = ac.canonical_edges(field) if field >= 16 else [0, 1, 2, p - 1, p - 2, (1 << 254) % p, (p + 1) // 2, (1 << 254) - 1, p - (1 << 29)]
    vals = edges + [rng.randrange(p) for _ in range(30)]
    out = np.zeros(8, dtype=np.uint32)
    for i, a in enumerate(vals):
        b = vals[(i * 7 + 3) % len(vals)]
        A, B = _u32(a), _u32(b)
        X = (a * a - a * b - 2 * b * b) % p
        for op, want in ((0, a * b % p), (1, (a + b) % p), (2, (a - b) % p), (4, a * a % p), (5, (-a) % p), (6, 2 * a % p), (7, (a - b) % p),
                         (8, (a * b - X) * (b * b - X) % p), (9, (a + b) * (a + b) % p), (10, (a * (a + b) + b * b) % p)):
            assert shim.zkt_field_op(field, op, P(A), P(B), P(out)) == 0
            assert _int(out) == want, (field, op, hex(a), hex(b))
        if a and i < 16:
            for op in ((3, 11) if field >= 16 else (3,)):
                assert shim.zkt_field_op(field, op, P(A), None, P(out)) == 0
                assert _int(out) == pow(a, -1, p), (field, op, hex(a))
    assert shim.zkt_field_op(20, 0, P(A), P(B), P(out)) == -1


def _chain(shim, field, curve, pts, infs, negs, mode, k=0):
    arr = pts_arr(curve, 1, pts).view(np.uint32).reshape(len(pts), -1) if len(pts) else np.zeros((0, 1), dtype=np.uint32)
    arr = np.ascontiguousarray(arr)
    out = np.zeros((3 if mode == 3 else 2) * 8, dtype=np.uint32)
    oinf = np.zeros(1, dtype=np.uint8)
    infa, nega = np.array(infs + [0], dtype=np.uint8), np.array(negs + [0], dtype=np.uint8)
    assert shim.zkt_point_chain(field, P(arr), P(infa), P(nega), ctypes.c_size_t(len(pts)), mode, ctypes.c_uint32(k), P(out), P(oinf)) == 0
    return out.view(np.uint64), int(oinf[0])


def chain_cases(curve, seed):
    """the cases of test_host_arith.py's group-law test: P + P, P + (-P), infinity operands, restart after infinity; with what each must give"""
    C = pu.CURVES[curve]
    G = C.g1
    base = pu.random_points(curve, seed, 6)
    P0, P1, P2 = base[0], base[1], base[2]
    cases = [([P0, P1, P2, base[3], base[4], base[5]], [0] * 6, [0, 1, 0, 1, 1, 0]), ([P0, P0], [0, 0], [0, 0]), ([P0, P0, P0, P0], [0] * 4, [0] * 4),
             ([P0, P0], [0, 0], [0, 1]), ([P0, P0, P1], [0, 0, 0], [0, 1, 0]), ([P0, P1], [1, 0], [0, 0]), ([G.gen, G.neg(G.gen), G.gen], [0] * 3, [0] * 3),
             ([], [], [])]
    out = []
    for pts, infs, negs in cases:
        exp = None
        for Pt, i, n in zip(pts, infs, negs):
            if not i:
                exp = G.add(exp, G.neg(Pt) if n else Pt)
        out.append((pts, infs, negs, exp))
    return out, (P0, P1)


def check_chains(fn, field, curve, seed, modes=(0, 4)):
    G = pu.CURVES[curve].g1
    cases, (P0, P1) = chain_cases(curve, seed)
    for pts, infs, negs, exp in cases:
        for mode in modes:
            out, oinf = fn(field, curve, pts, infs, negs, mode)
            assert pt_from_limbs(curve, 1, out, oinf) == exp, (mode, len(pts))
        if len(pts) >= 2:
            out, oinf = fn(field, curve, pts, infs, negs, 1)
            assert pt_from_limbs(curve, 1, out, oinf) == exp
            for k in (0, 1, 2, 37, 65535):
                out, oinf = fn(field, curve, pts, infs, negs, 2, k)
                assert pt_from_limbs(curve, 1, out, oinf) == G.mul(exp, k)
        out, oinf = fn(field, curve, pts, infs, negs, 3)
        if exp is None:
            assert oinf == 1 and po.from_limbs(out[8:12]) == 0
        else:
            assert jac_to_affine_py(curve, 1, out.reshape(3, 4)) == exp
    pts = [P0, P1, P0, P1]
    out, oinf = fn(field, curve, pts, [0] * 4, [0] * 4, 1)          # xyzz_add's doubling branch
    assert pt_from_limbs(curve, 1, out, oinf) == G.mul(G.add(P0, P1), 2)
    assert fn(field, curve, pts, [0] * 4, [0, 0, 1, 1], 1)[1] == 1   # and the cancelling one


@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("curve", [2, 3])
def test_xyzz_group_law(shim, curve, lazy):
    field = (pu.LAZY_FQ if lazy else pu.SAT_FQ)[curve]
    check_chains(lambda *a: _chain(shim, *a), field, curve, 7)
    arr = np.zeros((1, 16), dtype=np.uint32)
    for scalar_field in (pu.SAT_FR[curve], pu.LAZY_FR[curve]):
        assert shim.zkt_point_chain(scalar_field, P(arr), P(arr), P(arr), ctypes.c_size_t(0), 0, ctypes.c_uint32(0), P(arr), P(arr)) == -1


@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("curve", [2, 3])
def test_parked_points_share_one_inversion(shim, curve, lazy):
    """xyzz_park / xyzz_parked_to_affine over the Pasta coordinate fields: every prefix sum of parked_cases.py's chains against big
    integers, both layouts"""
    import parked_cases
    field = (pu.LAZY_FQ if lazy else pu.SAT_FQ)[curve]
    parked_cases.check(shim.zkt_parked_affine, field, curve, 1, pu.CURVES[curve].g1, pu.random_points(curve, 207, 4))


def check_recoding(digits_of, r, c, vals):
    tb = r.bit_length()
    W = (tb + c - 1) // c
    off = [w * tb // W for w in range(W + 1)]
    assert all(1 <= off[w + 1] - off[w] <= c for w in range(W))
    for v in vals:
        Wg, dig = digits_of(v)
        assert Wg == W, (c, hex(v))
        assert all(abs(int(d)) <= (1 << (off[w + 1] - off[w] - 1)) for w, d in enumerate(dig[:W])), (c, hex(v))
        got = sum(int(d) << off[w] for w, d in enumerate(dig[:W]))
        assert got % r == v % r and abs(got) <= (r - 1) // 2, (c, hex(v))


@pytest.mark.parametrize("curve", [2, 3])
def test_folded_recoding(shim, curve):
    """msm_fold_scalar + msm_recode over arith_cases' scalar edges for every window size; r, r + 1 and 2^256 - 1 = 3 r + ... are taken mod r
    (three subtractions), and [2^254, r) -- a range of about 2^125 values -- folds to small negatives"""
    r = pu.CURVES[curve].r
    assert (1 << 256) - 1 > 3 * r and (1 << 256) - 1 < 4 * r
    dig = np.zeros(140, dtype=np.int32)

    def digits_of(v):
        W = shim.zkt_recode_folded(curve, P(_u32(v)), c, P(dig))
        return W, dig.copy()

    for c in range(2, 22):
        rng = random.Random(c)
        vals = ac.scalar_edges(r, c, rng) + [1 << 254, (1 << 254) + 1, r - 2, 3 * r, 3 * r + 1] + [rng.randrange(1 << 254, r) for _ in range(4)]
        check_recoding(digits_of, r, c, vals)
    assert shim.zkt_recode_folded(7, P(_u32(1)), 5, P(dig)) == -1


# ---- the shim's host algebra ------------------------------------------------------------------------------------------------------------
def _fr(h, curve, op, a, b=0):
    out = np.zeros(4, dtype=np.uint64)
    assert h.pasta_fr_op(curve, op, P(limbs(a, 4)), P(limbs(b, 4)), P(out)) == 0
    return po.from_limbs(out)


def _g1(h, curve, op, Pt, Qt=None, k=0):
    out, oinf = np.zeros(8, dtype=np.uint64), ctypes.c_int()
    rc = h.pasta_g1_op(curve, op, P(pt_limbs(curve, 1, Pt)), int(Pt is None), P(pt_limbs(curve, 1, Qt)), int(Qt is None), P(limbs(k, 4)), P(out), ctypes.byref(oinf))
    assert rc == 0
    return oinf.value if op == 3 else pt_from_limbs(curve, 1, out, oinf.value)


@pytest.mark.parametrize("curve", [2, 3])
def test_shim_host_algebra(harness, curve):
    """fr_value product, inverse, sum and difference; group_value sum and difference; scalar multiples by 0, 1, r - 1, 2^254 and a random scalar"""
    C = pu.CURVES[curve]
    r, G = C.r, C.g1
    rng = random.Random(curve)
    vals = [0, 1, r - 1, (r + 1) // 2, 1 << 254, (1 << 254) - 1] + [rng.randrange(r) for _ in range(12)]
    for i, a in enumerate(vals):
        b = vals[(5 * i + 2) % len(vals)]
        assert _fr(harness, curve, 0, a, b) == a * b % r
        assert _fr(harness, curve, 2, a, b) == (a + b) % r and _fr(harness, curve, 3, a, b) == (a - b) % r
        if a:
            assert _fr(harness, curve, 1, a) == pow(a, -1, r)
    pts = pu.random_points(curve, 3, 4)
    for Pt, Qt in ((pts[0], pts[1]), (pts[0], pts[0]), (pts[0], G.neg(pts[0])), (None, pts[2]), (pts[3], None), (None, None), (G.gen, pts[1])):
        assert _g1(harness, curve, 0, Pt, Qt) == G.add(Pt, Qt)
        assert _g1(harness, curve, 2, Pt, Qt) == G.add(Pt, G.neg(Qt))
        assert _g1(harness, curve, 3, Pt, Qt) == int(Pt == Qt)
    for k in (0, 1, r - 1, 1 << 254, rng.randrange(r)):
        for Pt in (G.gen, pts[0]):
            assert _g1(harness, curve, 1, Pt, None, k) == G.mul(Pt, k), hex(k)
    assert _g1(harness, curve, 1, None, None, 5) is None
    assert harness.pasta_fr_op(0, 0, None, None, None) == -2    # the harness is for ids 2 and 3


@pytest.mark.parametrize("curve", [2, 3])
def test_shim_field_constants(harness, curve):
    """root_of_unity(n) = 5^((r - 1) / 2^n) for n = 1, 16, 32 and the throw at 33; generator 5; the modulus"""
    C = pu.CURVES[curve]
    out, gen, mod = (np.zeros(4, dtype=np.uint64) for _ in range(3))
    for n in (1, 16, 32):
        assert harness.pasta_root_of_unity(curve, ctypes.c_size_t(n), P(out), P(gen), P(mod)) == 0
        w = po.from_limbs(out)
        assert w == C.root_of_unity(n) and pow(w, 1 << (n - 1), C.r) == C.r - 1
        assert po.from_limbs(gen) == 5 == C.fr_generator and po.from_limbs(mod) == C.r
    assert harness.pasta_root_of_unity(curve, ctypes.c_size_t(33), P(out), P(gen), P(mod)) == 1
    assert harness.pasta_root_of_unity(curve, ctypes.c_size_t(0), P(out), P(gen), P(mod)) == 0 and po.from_limbs(out) == 1
