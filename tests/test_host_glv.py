"""The GLV split of the group DFT's twiddles (crypto3-zk_amd/csrc/glv.hpp: glv_split and the constants of the four curves), compiled for the
CPU into libzkhip_hosttest.so, against big integers.  The kernel that builds the twiddle records (ecntt.hip: ec_ntt_records) calls the same
function, and the ladder multiplies X by the same beta.

For every curve id: k1 + k2 lambda = k (mod r) with both magnitudes below 2^131 (what the records' 33 signed nibbles hold), over the corners,
the rounding boundaries of c1 and c2 and 10^5 seeded random scalars; beta and lambda belong together, (beta x, y) = lambda (x, y); and for the
two pairing curves, whose split ran inside the kernel before it moved to the header, the arithmetic restated here from the constants
they had then gives the same words."""
import ctypes
import os
import random

import numpy as np
import pytest

import pasta_util as pu
import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_hosttest.so")
CURVES = {0: po.BLS12_381, 1: po.BN254, 2: pu.PALLAS, 3: pu.VESTA}
NAMES = ("g1", "g2", "a1", "a2", "b1", "b2")


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run __graft_entry__.build()")
    return ctypes.CDLL(SO)


def _int(words):
    return sum(int(w) << (32 * i) for i, w in enumerate(words))


def consts(shim, curve):
    """the constants the library was compiled with, as integers (magnitudes), and lambda = |a1| / |b1| mod r  (a1 > 0 > b1, a1 + b1 lambda = 0)"""
    out = np.zeros(42, dtype=np.uint32)
    assert shim.zkt_glv_consts(curve, out.ctypes.data_as(ctypes.c_void_p)) == 0
    c = {name: _int(out[5 * i:5 * i + 5]) for i, name in enumerate(NAMES)}
    c["beta"] = _int(out[30:42])
    r = CURVES[curve].r
    c["lambda"] = c["a1"] * pow(c["b1"], -1, r) % r
    return c


def split(shim, curve, k):
    kw = np.array([(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)], dtype=np.uint32)
    k1, k2, signs = np.zeros(6, dtype=np.uint32), np.zeros(6, dtype=np.uint32), ctypes.c_uint32()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert shim.zkt_glv_split(curve, P(kw), P(k1), P(k2), ctypes.byref(signs)) == 0
    return _int(k1), _int(k2), signs.value


def scalars(curve, c):
    r = CURVES[curve].r
    lam = c["lambda"]
    ks = [0, 1, r - 1, lam, r - lam, 1 << 254, (1 << 254) - 1, r - 2]
    for q in (c["b1"], c["b2"]):    # c1 = floor(k |b2| / r) and c2 = floor(k |b1| / r) step at the multiples of r / |b|: those nearest 2^200
        j = ((q << 200) + r // 2) // r
        for jj in (j, j + 1):
            k0 = jj * r // q
            ks += [k0 + d for d in range(-2, 3)]
    rng = random.Random(7700 + curve)
    ks += [rng.randrange(r) for _ in range(100000)]
    return [k for k in ks if 0 <= k < r]


@pytest.mark.parametrize("curve", [0, 1, 2, 3])
def test_constants_are_a_basis_with_the_kernel_signs(shim, curve):
    """a1 > 0 > b1, a2, b2 > 0 (magnitudes stored): both vectors in the lattice, determinant r, g = floor(2^256 |b| / r), everything in 5 words"""
    c, r = consts(shim, curve), CURVES[curve].r
    lam = c["lambda"]
    assert (lam * lam + lam + 1) % r == 0 and lam != 1
    assert (c["a1"] - c["b1"] * lam) % r == 0 and (c["a2"] + c["b2"] * lam) % r == 0
    assert c["a1"] * c["b2"] + c["a2"] * c["b1"] == r
    assert c["g1"] == (c["b2"] << 256) // r and c["g2"] == (c["b1"] << 256) // r
    assert all(0 < c[n] < 1 << 160 for n in NAMES)


@pytest.mark.parametrize("curve", [0, 1, 2, 3])
def test_beta_and_lambda_belong_together(shim, curve):
    c, C = consts(shim, curve), CURVES[curve]
    p, g = C.p, C.g1
    beta = c["beta"]
    assert 1 < beta < p and (beta * beta + beta + 1) % p == 0
    x, y = g.gen
    assert g.mul(g.gen, c["lambda"]) == (beta * x % p, y), "phi(G) = (beta x, y) is not lambda G: lambda is the other cube root of unity"


@pytest.mark.parametrize("curve", [0, 1, 2, 3])
def test_split_recombines_and_fits_the_record(shim, curve):
    c, r = consts(shim, curve), CURVES[curve].r
    lam, worst = c["lambda"], 0
    for k in scalars(curve, c):
        m1, m2, signs = split(shim, curve, k)
        assert signs < 4
        k1, k2 = (-m1 if signs & 1 else m1), (-m2 if signs & 2 else m2)
        assert (k1 + k2 * lam - k) % r == 0, hex(k)
        assert m1 < 1 << 131 and m2 < 1 << 131, hex(k)
        worst = max(worst, m1.bit_length(), m2.bit_length())
    print(f"curve {curve}: largest half {worst} bits")
    # c = floor(k g / 2^256) with g = floor(2^256 |b| / r) lies in (k |b| / r - 2, k |b| / r]: the remainder is x1 v1 + x2 v2 with x1, x2 in [0, 2),
    # so a half stays below 2 (|a1| + |a2|) resp. 2 (|b1| + |b2|) < 2^130 for components of at most 128 bits -- room to spare in the record
    assert worst <= 130


# the two pairing curves' constants as ec_ntt_records had them (u32 words, low first) before the split moved to glv.hpp
OLD = {
    0: dict(g1=[0xf6cfee30, 0x63f6e522, 0xe01faadd, 0x7c6becf1, 1], g2=[2, 0, 0, 0, 0], a1=[0xffffffff, 0, 0x0001a402, 0xac45a401, 0], a2=[1, 0, 0, 0, 0],
            b1=[1, 0, 0, 0, 0], b2=[0, 1, 0x0001a402, 0xac45a401, 0]),
    1: dict(g1=[0xc7e0b3d7, 0xd91d232e, 2, 0, 0], g2=[0x391eb18d, 0x7a7bd9d4, 0xa773d2cf, 0x4ccef014, 2], a1=[0x94d213e3, 0x89d32568, 0, 0, 0],
            a2=[0x1221250b, 0x0be4e154, 0xeeb859fd, 0x6f4d8248, 0], b1=[0x7d4f1128, 0x8211bbeb, 0xeeb859fc, 0x6f4d8248, 0], b2=[0x94d213e3, 0x89d32568, 0, 0, 0]),
}


def old_split(curve, k):
    """the in-kernel arithmetic: c = words 8..12 of k g, the halves modulo 2^192 in two's complement, then sign and magnitude"""
    o = {n: _int(w) for n, w in OLD[curve].items()}
    M160, M192 = (1 << 160) - 1, (1 << 192) - 1
    c1, c2 = (k * o["g1"] >> 256) & M160, (k * o["g2"] >> 256) & M160
    k1 = (k - c1 * o["a1"] - c2 * o["a2"]) & M192
    k2 = (c1 * o["b1"] - c2 * o["b2"]) & M192
    signs = 0
    if k1 >> 191:
        k1, signs = (-k1) & M192, signs | 1
    if k2 >> 191:
        k2, signs = (-k2) & M192, signs | 2
    return k1, k2, signs


@pytest.mark.parametrize("curve", [0, 1])
def test_pairing_curves_split_as_before(shim, curve):
    c = consts(shim, curve)
    assert all(c[n] == _int(OLD[curve][n]) for n in NAMES)
    for k in scalars(curve, c)[:20000]:
        assert split(shim, curve, k) == old_split(curve, k), hex(k)
