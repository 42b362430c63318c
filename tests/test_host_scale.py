"""The window records of zkhip_bases_scale_dev's scalars (crypto3-zk_amd/csrc/glv.hpp: scalar_record, recode_nibbles; fu.hpp: fu_reduce), compiled
for the CPU into libzkhip_hosttest.so, against big integers.  The kernel that builds the records (ecntt.hip: scale_records_from_scalars) calls
the same functions on the same words.

For every curve id and both record forms (GLV: 33 signed nibbles per half and a sign word, the G1 ladder; plain: 65 signed nibbles, the G2
ladder): the scalar is reduced mod r -- non-canonical values included, as zkhip_msm_dev takes them --, every nibble is a digit in [-8, 7],
and the digits sum back to the scalar: sum_w d_w 16^w = k, or (+-sum_w d1_w 16^w) + (+-sum_w d2_w 16^w) lambda = k (mod r)."""
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
LAMBDA = {0: 0xac45a4010001a40200000000ffffffff,
          1: 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd,
          2: 0x397e65a7d7c1ad71aee24b27e308f0a61259527ec1d4752e619d1840af55f1b1,
          3: 0x12ccca834acdba712caad5dc57aab1b01d1f8bd237ad31491dad5ebdfdfe4ab9}
REC_WORDS = 12


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run __graft_entry__.build()")
    return ctypes.CDLL(SO)


def record(shim, curve, glv, s):
    sw = np.array([(s >> (32 * i)) & 0xFFFFFFFF for i in range(8)], dtype=np.uint32)
    k, rec = np.zeros(8, dtype=np.uint32), np.full(REC_WORDS, 0xDEADBEEF, dtype=np.uint32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert shim.zkt_scale_record(curve, glv, P(sw), P(k), P(rec)) == 0
    return sum(int(w) << (32 * i) for i, w in enumerate(k)), [int(w) for w in rec]


def digits(words, windows):
    """the signed value of `windows` two's-complement nibbles, low first"""
    total = 0
    for w in range(windows):
        d = (words[w >> 3] >> ((w & 7) * 4)) & 15
        total += (d - 16 if d >= 8 else d) << (4 * w)
    return total


def scalars(curve):
    r, lam = CURVES[curve].r, LAMBDA[curve]
    s = [0, 1, 2, 7, 8, 9, 15, 16, 17, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2, lam, lam + 1, lam - 1, r - lam,
         (1 << 128) - 1, 1 << 128, 1 << 129, 0x8888888888888888888888888888888, 0x7777777777777777777777777777777,
         r, r + 1, r + 5, 2 * r - 1, 2 * r, (1 << 256) - 1, 1 << 255]
    rng = random.Random(9900 + curve)
    return s + [rng.randrange(r) for _ in range(20000)] + [rng.randrange(1 << 256) for _ in range(2000)]


@pytest.mark.parametrize("curve", [0, 1, 2, 3])
def test_plain_record_sums_back_to_the_scalar(shim, curve):
    r = CURVES[curve].r
    for s in scalars(curve):
        k, rec = record(shim, curve, 0, s)
        assert k == s % r, hex(s)
        assert digits(rec[:9], 65) == k, hex(s)
        assert rec[8] >> 4 == 0 and rec[9:] == [0, 0, 0], hex(s)    # 65 nibbles: nothing above nibble 64, no sign word


@pytest.mark.parametrize("curve", [0, 1, 2, 3])
def test_glv_record_sums_back_to_the_scalar(shim, curve):
    r, lam = CURVES[curve].r, LAMBDA[curve]
    assert (lam * lam + lam + 1) % r == 0
    for s in scalars(curve):
        k, rec = record(shim, curve, 1, s)
        assert k == s % r, hex(s)
        m1, m2, signs = digits(rec[0:5], 33), digits(rec[5:10], 33), rec[10]
        assert m1 >= 0 and m2 >= 0 and signs < 4 and rec[11] == 0, hex(s)    # magnitudes; the top nibble absorbs the last carry
        assert rec[4] >> 4 == 0 and rec[9] >> 4 == 0, hex(s)                 # 33 nibbles per half
        k1, k2 = (-m1 if signs & 1 else m1), (-m2 if signs & 2 else m2)
        assert (k1 + k2 * lam - k) % r == 0, hex(s)
