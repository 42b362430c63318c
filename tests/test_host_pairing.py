"""The Fq12 tower and the pairing of crypto3-zk_amd/csrc (fq12.hpp, pairing.hpp), compiled for the CPU into libzkhip_hosttest.so, against
the big-integer model (tests/pairing_ref.py) and the reference's vectors.  These are the bodies the Miller kernel and the host final
exponentiation of zkhip_pairing_products run."""
import ctypes
import os
import random

import numpy as np
import pytest

import pairing_ref as pr
import pyoracle as po
from test_pairing_ref import load_kat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_hosttest.so")
G1, G2 = po.BLS12_381.g1, po.BLS12_381.g2
P = pr.P
ONE = pr.to_canonical(pr.ONE)


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run __graft_entry__.build()")
    return ctypes.CDLL(SO)


def u32(vals):
    return np.array([(v >> (32 * i)) & 0xFFFFFFFF for v in vals for i in range(12)], dtype=np.uint32)


def ints(a):
    a = np.asarray(a).reshape(-1, 12)
    return [sum(int(x) << (32 * i) for i, x in enumerate(row)) for row in a]


ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def fq12_op(shim, op, a, b=None):
    out = np.zeros(144, dtype=np.uint32)
    assert shim.zkt_fq12_op(op, ptr(u32(a)), ptr(u32(b)) if b is not None else None, ptr(out)) == 0
    return ints(out)


def host_products(shim, pairs_per_term, outs, n_out):
    """zkt_pairing_products over lists of (P, Q) pairs (None = infinity), one list per term"""
    flat = [pq for term in pairs_per_term for pq in term]
    g1 = u32([c for p, _ in flat for c in (p if p is not None else (0, 0))])
    g2 = u32([c for _, q in flat for xy in (q if q is not None else ((0, 0), (0, 0))) for c in xy])
    i1 = np.array([p is None for p, _ in flat], dtype=np.uint8)
    i2 = np.array([q is None for _, q in flat], dtype=np.uint8)
    n = np.array([len(t) for t in pairs_per_term], dtype=np.uint64)
    start = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.uint64) if len(n) else np.zeros(0, dtype=np.uint64)
    o = np.array(outs, dtype=np.uint32)
    out = np.zeros(n_out * 144, dtype=np.uint32)
    pad = lambda a, dt: a if a.size else np.zeros(1, dtype=dt)
    rc = shim.zkt_pairing_products(ptr(pad(g1, np.uint32)), ptr(pad(i1, np.uint8)), ptr(pad(g2, np.uint32)), ptr(pad(i2, np.uint8)), ptr(pad(start, np.uint64)),
                                   ptr(pad(n, np.uint64)), ptr(pad(o, np.uint32)), ctypes.c_size_t(len(pairs_per_term)), ctypes.c_size_t(n_out), ptr(out))
    assert rc == 0
    return [ints(out[k * 144:(k + 1) * 144]) for k in range(n_out)]


def test_fq12_ops_against_the_model(shim):
    random.seed(11)
    single = lambda k, v: [v if i == k else 0 for i in range(12)]
    edge = [single(k, v) for k in (0, 5, 11) for v in (1, P - 1)] + [[0] * 12, [P - 1] * 12]
    vals = edge + [[random.randrange(P) for _ in range(12)] for _ in range(6)]
    for i, a in enumerate(vals):
        b = vals[(i * 5 + 3) % len(vals)]
        A, B = pr.from_canonical(a), pr.from_canonical(b)
        assert fq12_op(shim, 0, a, b) == pr.to_canonical(pr.f12_mul(A, B)), i
        assert fq12_op(shim, 1, a) == pr.to_canonical(pr.f12_mul(A, A)), i
        assert fq12_op(shim, 4, a) == pr.to_canonical(pr.f12_conj(A)), i
        # the sparse product: b's slots 0, 1 and 4 as the line value l0 + l1 v + l4 v w
        line = [b[0], b[1], b[2], b[3], b[8], b[9]]
        sparse = pr.from_canonical(b[:4] + [0] * 4 + b[8:10] + [0] * 2)
        out = np.zeros(144, dtype=np.uint32)
        assert shim.zkt_fq12_op(5, ptr(u32(a)), ptr(u32(line)), ptr(out)) == 0
        assert ints(out) == pr.to_canonical(pr.f12_mul(A, sparse)), i


def test_fq12_frobenius_and_inverse(shim):
    random.seed(12)
    for a in ([1] + [0] * 11, [0] * 11 + [P - 1], [random.randrange(P) for _ in range(12)], [random.randrange(P) for _ in range(12)]):
        A = pr.from_canonical(a)
        assert fq12_op(shim, 3, a) == pr.to_canonical(pr.f12_frobenius(A))
        inv = fq12_op(shim, 2, a)
        assert inv == pr.to_canonical(pr.f12_inv(A))
        assert fq12_op(shim, 0, inv, a) == ONE


def test_final_exponentiation_against_the_model(shim):
    random.seed(13)
    a = [random.randrange(P) for _ in range(12)]
    assert fq12_op(shim, 6, a) == pr.to_canonical(pr.final_exponentiation(pr.from_canonical(a)))


def test_pairing_products_equal_the_reference_vectors(shim):
    a, b, v1, v2, w1, w2, exp = load_kat()
    za = lambda x, y: list(zip(x, y))
    assert host_products(shim, [za(a, v1), za(a, v2)], [0, 1], 2) == [exp["single_first"], exp["single_second"]]
    got = host_products(shim, [za(a, v1), za(w1, b), za(a, v2), za(w2, b)], [0, 0, 1, 1], 2)
    assert got == [exp["pair_first"], exp["pair_second"]]


def random_pairs(seed, n):
    random.seed(seed)
    return [(G1.mul(G1.gen, random.randrange(1, pr.R)), G2.mul(G2.gen, random.randrange(1, pr.R))) for _ in range(n)]


@pytest.mark.parametrize("n", [1, 2, 3])
def test_pairing_products_against_the_model(shim, n):
    pairs = random_pairs(20 + n, n)
    assert host_products(shim, [pairs], [0], 1) == [pr.pairing_product(pairs)]


def test_infinity_gives_one(shim):
    (p, q), = random_pairs(30, 1)
    assert host_products(shim, [[(None, q)], [(p, None)], [(None, None)]], [0, 1, 2], 4) == [ONE] * 4
    assert host_products(shim, [[(p, q), (None, q), (p, None)]], [0], 1) == [pr.pairing_product([(p, q)])]
