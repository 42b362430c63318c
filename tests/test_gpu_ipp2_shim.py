"""The inner pairing product commitments of the shim (hip/kzg_ipp2.hpp) over the stand-in `bls12_381` types on the GPU, driven through
tests/cpp/ipp2_test.cpp -> libipp2test.so (a target of tests/cpp/Makefile):

  kzg_ipp2_hip::single / ::pair  reproduce the reference's vectors (tests/golden/ref_ipp2_kat.json) through the shim's types -- keys built from
                                 the scalar powers on the device or from host values, the committed vectors as host values and as resident bases;
  pairing_inner_product_hip      n = 8 resident pairs a_i G1, b_i G2 against the model's e(G1, G2)^(sum a_i b_i); all a_i = 0 gives gt_value::one();
  has_correct_len                every length mismatch throws std::invalid_argument, matching lengths do not."""
import ctypes
import json
import random

import numpy as np
import pytest

import pairing_ref as pr
from harness import library
from test_gpu_pairing import fq_limbs, fr_arr, gt_ints
from test_pairing_ref import KAT

pytestmark = pytest.mark.gpu
Z = ctypes.c_size_t
ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
H = lambda s: int(s, 16)


@pytest.fixture(scope="module")
def harness():
    return library("libipp2test.so")


@pytest.fixture(scope="module")
def kat():
    k = json.load(open(KAT))
    a = np.array([fq_limbs(H(x)) + fq_limbs(H(y)) for x, y in k["a"]], dtype=np.uint64)
    b = np.array([fq_limbs(H(x[0])) + fq_limbs(H(x[1])) + fq_limbs(H(y[0])) + fq_limbs(H(y[1])) for x, y in k["b"]], dtype=np.uint64)
    exp = {name: [H(x) for x in k[name]] for name in ("single_first", "single_second", "pair_first", "pair_second")}
    return fr_arr([H(k["u"])]), fr_arr([H(k["v"])]), a, b, exp


@pytest.mark.parametrize("resident", [0, 1])
def test_single_reproduces_the_reference_vectors(harness, kat, resident):
    u, v, a, _, exp = kat
    out = np.zeros((2, 72), dtype=np.uint64)
    assert harness.ipp2_single(ptr(u), ptr(v), Z(10), ptr(a), resident, ptr(out)) == 0
    assert gt_ints(out[0]) == exp["single_first"] and gt_ints(out[1]) == exp["single_second"]


@pytest.mark.parametrize("resident", [0, 1])
def test_pair_reproduces_the_reference_vectors(harness, kat, resident):
    u, v, a, b, exp = kat
    out = np.zeros((2, 72), dtype=np.uint64)
    assert harness.ipp2_pair(ptr(u), ptr(v), Z(10), ptr(a), ptr(b), resident, ptr(out)) == 0
    assert gt_ints(out[0]) == exp["pair_first"] and gt_ints(out[1]) == exp["pair_second"]


def test_inner_product_against_the_structured_expectation(harness):
    rnd = random.Random(8)
    a, b = [rnd.randrange(1, pr.R) for _ in range(8)], [rnd.randrange(1, pr.R) for _ in range(8)]
    out = np.zeros(72, dtype=np.uint64)
    assert harness.ipp2_inner_product(ptr(fr_arr(a)), ptr(fr_arr(b)), Z(8), ptr(out)) == 0    # 0: not one
    assert gt_ints(out) == pr.structured_expectation(sum(x * y for x, y in zip(a, b)))
    # every G1 point at infinity: the value is gt_value::one(), and == / != say so
    assert harness.ipp2_inner_product(ptr(fr_arr([0] * 8)), ptr(fr_arr(b)), Z(8), ptr(out)) == 1
    assert gt_ints(out) == pr.to_canonical(pr.ONE)


@pytest.mark.parametrize("which", [0, 1, 2, 3, 4, 5])
def test_length_mismatches_throw(harness, which):
    assert harness.ipp2_length_mismatch(which) == 1


def test_matching_lengths_do_not_throw(harness):
    assert harness.ipp2_length_mismatch(6) == 0
