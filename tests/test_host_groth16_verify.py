"""The Groth16 verifier's bodies (crypto3-zk_amd/csrc/groth16_verify.hpp, miller_loop3 and the prepared lines of pairing.hpp, the
cyclotomic squaring of fq12.hpp), compiled for the CPU into libzkhip_hosttest.so (zkt_groth16_verify), against the reference's eight
bellperson proofs (tests/golden/ref_groth16_verify_kat.json) and the model (tests/groth16_verify_ref.py, tests/pairing_ref.py).
These are the bodies the kernels of groth16_verify.hip run."""
import ctypes
import random

import numpy as np
import pytest

import groth16_verify_ref as gr
import pairing_ref as pr
from test_host_pairing import ONE, fq12_op, host_products, ptr, shim  # noqa: F401  (shim: the fixture)

G1, G2, R, P = gr.G1, gr.G2, gr.R, gr.P


def u64(vals, limbs):
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for v in vals for i in range(limbs)], dtype=np.uint64)


def u32(vals, limbs):
    return np.array([(v >> (32 * i)) & 0xFFFFFFFF for v in vals for i in range(limbs)], dtype=np.uint32)


def ints(a, limbs, bits):
    a = np.asarray(a).reshape(-1, limbs)
    return [sum(int(x) << (bits * i) for i, x in enumerate(row)) for row in a]


def g1_flat(pts):
    return [c for p in pts for c in (p if p is not None else (0, 0))]


def g2_flat(pts):
    return [c for q in pts for xy in (q if q is not None else ((0, 0), (0, 0))) for c in xy]


def flags(pts):
    return np.array([p is None for p in pts], dtype=np.uint8)


def host_verify(shim, alpha_beta, gamma, delta, ic, proofs, xs):
    """zkt_groth16_verify -> (ok, [gt as 12 ints], [-acc as a point or None]); None is the point at infinity, xs one list per proof"""
    n, n_inputs = len(proofs), len(xs[0])
    assert all(len(x) == n_inputs for x in xs)
    A, B, C = ([pf[k] for pf in proofs] for k in range(3))
    ok, gt, nacc = np.zeros(n, dtype=np.uint8), np.zeros(n * 144, dtype=np.uint32), np.zeros(n * 24, dtype=np.uint32)
    inputs = u32([x for row in xs for x in row], 8)
    rc = shim.zkt_groth16_verify(ptr(u64(alpha_beta, 6)), ptr(u64(g2_flat([gamma]), 6)), ptr(u64(g2_flat([delta]), 6)), ptr(u64(g1_flat(ic), 6)), ptr(flags(ic)),
                                 ctypes.c_size_t(len(ic)), ptr(u32(g1_flat(A), 12)), ptr(flags(A)), ptr(u32(g2_flat(B), 12)), ptr(flags(B)), ptr(u32(g1_flat(C), 12)),
                                 ptr(flags(C)), ctypes.c_size_t(n), ptr(inputs) if n_inputs else None, ctypes.c_size_t(n_inputs), ptr(ok), ptr(gt), ptr(nacc))
    assert rc == 0
    acc = [None if not any(row) else tuple(row) for row in np.array(ints(nacc, 12, 32), dtype=object).reshape(n, 2)]
    return [int(v) for v in ok], [ints(gt[k * 144:(k + 1) * 144], 12, 32) for k in range(n)], acc


@pytest.fixture(scope="module")
def kat():
    return gr.load_kat()


def kat_verify(shim, kat, proofs, xs):
    return host_verify(shim, kat["alpha_beta"], kat["gamma"], kat["delta"], kat["ic"], proofs, xs)


def test_fixture_is_well_formed(kat):
    assert len(kat["ic"]) == 12 and len(kat["proofs"]) == 8 and all(len(s) == 11 for s in kat["statements"])
    assert all(G1.on_curve(p) for p in kat["ic"]) and G2.on_curve(kat["gamma"]) and G2.on_curve(kat["delta"])
    assert all(G1.on_curve(a) and G2.on_curve(b) and G1.on_curve(c) for a, b, c in kat["proofs"])


def test_the_eight_reference_proofs_are_accepted(shim, kat):
    ok, gt, _ = kat_verify(shim, kat, kat["proofs"], kat["statements"])
    assert ok == [1] * 8
    assert all(g == kat["alpha_beta"] for g in gt)


def test_swapped_points_and_a_changed_statement_are_rejected(shim, kat):
    (a0, b0, c0), (a1, b1, c1) = kat["proofs"][:2]
    st = kat["statements"][0]
    changed = st[:10] + [st[10] + 1]
    ok, gt, _ = kat_verify(shim, kat, [(a1, b0, c0), (a0, b1, c0), (a0, b0, c1), (a0, b0, c0), (a0, b0, c0)], [st, st, st, changed, st])
    assert ok == [0, 0, 0, 0, 1]
    assert all(g != kat["alpha_beta"] for g in gt[:4])


@pytest.mark.parametrize("k", [0, 1])
def test_the_model_accepts_the_reference_proofs(kat, k):
    assert gr.compared_value(kat["gamma"], kat["delta"], kat["ic"], kat["proofs"][k], kat["statements"][k]) == kat["alpha_beta"]


def test_the_model_and_the_twin_agree_on_a_rejected_proof(shim, kat):
    (a0, b0, c0), (a1, _, _) = kat["proofs"][:2]
    _, gt, _ = kat_verify(shim, kat, [(a1, b0, c0)], [kat["statements"][0]])
    assert gt[0] == gr.compared_value(kat["gamma"], kat["delta"], kat["ic"], (a1, b0, c0), kat["statements"][0]) != kat["alpha_beta"]


def cyclotomic(shim, a):
    """a^((p^6 - 1)(p^2 + 1)) by the tower's own operations"""
    t = fq12_op(shim, 0, fq12_op(shim, 4, a), fq12_op(shim, 2, a))
    return fq12_op(shim, 0, fq12_op(shim, 3, fq12_op(shim, 3, t)), t)


def test_cyclotomic_squaring(shim):
    random.seed(21)
    for _ in range(4):
        a = [random.randrange(P) for _ in range(12)]
        c = cyclotomic(shim, a)
        assert fq12_op(shim, 0, c, fq12_op(shim, 4, c)) == ONE  # in the cyclotomic subgroup the conjugate is the inverse
        sq = fq12_op(shim, 7, c)
        C = pr.from_canonical(c)
        assert sq == fq12_op(shim, 1, c) == pr.to_canonical(pr.f12_mul(C, C))
        # and only there
        assert fq12_op(shim, 7, a) != fq12_op(shim, 1, a)
    assert fq12_op(shim, 7, ONE) == ONE


@pytest.mark.parametrize("seed", [14, 15])
def test_final_exponentiation_is_unchanged(shim, seed):
    """exp_by_x squares by Granger and Scott now: the same value as the model's plain power"""
    random.seed(seed)
    a = [random.randrange(P) for _ in range(12)]
    assert fq12_op(shim, 6, a) == pr.to_canonical(pr.final_exponentiation(pr.from_canonical(a)))


def test_prepared_lines_give_the_walked_pairing(shim, kat):
    """with A at infinity the compared value is e(-acc, gamma) e(-C, delta); with C at infinity too, e(-acc, gamma) alone, and with abc[0] at
    infinity (a key of no inputs) e(-C, delta) alone: each equals the walked Miller loop of pairing.hpp after the final exponentiation"""
    _, b0, c0 = kat["proofs"][0]
    ic0 = kat["ic"][0]
    ab = kat["alpha_beta"]
    _, gt, acc = host_verify(shim, ab, kat["gamma"], kat["delta"], [ic0], [(None, b0, None), (None, None, c0)], [[], []])
    assert acc == [G1.neg(ic0)] * 2
    assert gt[0] == host_products(shim, [[(G1.neg(ic0), kat["gamma"])]], [0], 1)[0] != ONE
    assert gt[1] == host_products(shim, [[(G1.neg(ic0), kat["gamma"]), (G1.neg(c0), kat["delta"])]], [0], 1)[0]
    _, gt, acc = host_verify(shim, ab, kat["gamma"], kat["delta"], [None], [(None, b0, c0), (None, None, None)], [[], []])
    assert acc == [None, None]
    assert gt[0] == host_products(shim, [[(G1.neg(c0), kat["delta"])]], [0], 1)[0] != ONE
    assert gt[1] == ONE


def test_accumulation_edge_scalars(shim):
    """scalars 0, 1 and r - 1 (and 2^256 - 1: every window digit maximal), acc at infinity (x_1 = -u_0 / u_1), fewer inputs than the key has"""
    key = gr.Key(31, 3)
    gamma, delta, ic = key.points()
    x_inf = (-key.u[0]) * pow(key.u[1], -1, R) % R
    rows = [[0, 0, 0], [1, 1, 1], [R - 1, R - 1, R - 1], [(1 << 256) - 1, 0, 1], [x_inf, 0, 0], [0x123456789ABCDEF << 190, R - 2, 16]]
    pf = (None, None, None)
    _, _, acc = host_verify(shim, key.alpha_beta(), gamma, delta, ic, [pf] * len(rows), rows)
    for row, got in zip(rows, acc):
        exp = gr.accumulate(ic, row)
        assert got == (None if exp is None else G1.neg(exp)), row
    assert acc[4] is None and acc[0] == G1.neg(ic[0])
    _, _, acc = host_verify(shim, key.alpha_beta(), gamma, delta, ic, [pf], [[5]])
    assert acc[0] == G1.neg(gr.accumulate(ic, [5, 0, 0]))


def test_synthetic_proofs_against_the_model(shim):
    """a key from trapdoor scalars: an accepted proof, one with a wrong input, one with c off by one, A at infinity, and an abc point at infinity"""
    key = gr.Key(32, 2, u=[random.Random(1).randrange(1, R), 0, random.Random(2).randrange(1, R)])
    gamma, delta, ic = key.points()
    assert ic[1] is None
    xs = [7, R - 3]
    good = key.prove(xs)
    cases = [(good, xs), (good, [7, R - 4]), ((good[0], good[1], (good[2] + 1) % R), xs), ((0, good[1], good[2]), xs), (good, [8, R - 3])]
    pts = [(G1.mul(G1.gen, a) if a else None, G2.mul(G2.gen, b) if b else None, G1.mul(G1.gen, c) if c else None) for (a, b, c), _ in cases]
    ok, gt, _ = host_verify(shim, key.alpha_beta(), gamma, delta, ic, pts, [x for _, x in cases])
    assert ok == [int(key.accepts(abc, x)) for abc, x in cases] == [1, 0, 0, 0, 1]  # abc[1] is at infinity: x_1 does not matter
    assert gt[0] == key.alpha_beta() == gt[4]
    for k in (1, 2, 3):
        assert gt[k] == key.expected_gt(*cases[k])


def test_a_point_off_its_curve_is_rejected_whatever_the_value(shim, kat):
    a0, b0, c0 = kat["proofs"][0]
    st = kat["statements"][0]
    bad_a, bad_c = (a0[0], (a0[1] + 1) % P), (c0[0], (c0[1] + 1) % P)
    bad_b = (b0[0], ((b0[1][0] + 1) % P, b0[1][1]))
    ok, _, _ = kat_verify(shim, kat, [(bad_a, b0, c0), (a0, bad_b, c0), (a0, b0, bad_c), (a0, b0, c0)], [st] * 4)
    assert ok == [0, 0, 0, 1]
