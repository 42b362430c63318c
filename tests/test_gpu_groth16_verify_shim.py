"""The shim's Groth16 verifier (hip/r1cs_gg_ppzksnark_verifier.hpp) and the generator's verification key
(hip/r1cs_gg_ppzksnark_generator.hpp) through libzkhip_bench.so (bench/groth16_verify_bench.cpp): a key WITH its verification key for the
2^10-constraint, 10-input system of smoke(), proofs made on the device, verified on the device.  This is what pins the generator against
the verifier: the same swap_AB_if_beneficial, the division by gamma, alpha_g1_beta_g2 from the device's pairing.  The reference's eight
bellperson proofs go through the same classes from host values."""
import ctypes
import os

import numpy as np
import pytest

import groth16_verify_ref as gr
from test_gpu_pairing import fq_limbs, fr_arr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_bench.so")
R, GEN = gr.R, 7
M, N_IN = 1 << 10, 10


def lim(v):
    return np.array([(v >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run __graft_entry__.build()")
    return ctypes.CDLL(SO)


def roundtrip(lib, seed, zero_inputs):
    m = 1
    while m < M + N_IN + 1:
        m <<= 1
    omega, coset = lim(pow(GEN, (R - 1) // m, R)), lim(GEN)
    out = np.full(12, -1, dtype=np.int32)
    rc = lib.zkhip_bench_groth16_verify_roundtrip(0, ctypes.c_size_t(M), ctypes.c_size_t(N_IN), ctypes.c_uint64(seed), zero_inputs,
                                                  omega.ctypes.data_as(ctypes.c_void_p), coset.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return [int(v) for v in out]


@pytest.fixture(scope="module")
def verdicts(lib):
    return roundtrip(lib, 3, 0)


def test_a_generated_key_verifies_its_proof(verdicts):
    assert verdicts[0] == 1 and verdicts[2] == 1


def test_a_wrong_public_input_is_rejected(verdicts):
    assert verdicts[1] == 0


def test_strong_refuses_a_missing_input_and_weak_takes_it_as_zero(lib, verdicts):
    """the random statement's last input is not zero: weak rejects the shorter statement; in the all-zero statement it is, and weak accepts,
    while strong answers false on the size alone both times"""
    assert verdicts[3] == 0 and verdicts[4] == 0
    zero = roundtrip(lib, 4, 1)
    assert zero[0] == 1 and zero[2] == 1
    assert zero[3] == 0 and zero[4] == 1
    assert zero[5:8] == [1, 0, 1]


def test_the_batch_form_with_the_middle_proof_spoiled(verdicts):
    assert verdicts[5:8] == [1, 0, 1]
    assert verdicts[8:11] == [1, 0, 0]  # strong: the last statement is one input short


def test_more_inputs_than_the_key_has_throw(verdicts):
    assert verdicts[11] == 1


def test_the_reference_proofs_through_the_shim_classes(lib):
    k = gr.load_kat()
    g1 = lambda p: fq_limbs(p[0]) + fq_limbs(p[1])
    g2 = lambda q: fq_limbs(q[0][0]) + fq_limbs(q[0][1]) + fq_limbs(q[1][0]) + fq_limbs(q[1][1])
    arr = lambda rows: np.array(rows, dtype=np.uint64).reshape(-1)
    ab = arr([l for v in k["alpha_beta"] for l in fq_limbs(v)])
    abc = arr([g1(p) for p in k["ic"]])
    a, b, c = (arr([f(p[i]) for p in k["proofs"]]) for i, f in ((0, g1), (1, g2), (2, g1)))
    st = [list(s) for s in k["statements"]]
    st[3][0] += 1
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)

    def run(inputs, n_inputs, strong):
        ok = np.full(8, 7, dtype=np.uint8)
        inp = fr_arr([x for row in inputs for x in row])
        rc = lib.zkhip_bench_groth16_verify_points(0, ptr(ab), ptr(arr(g2(k["gamma"]))), ptr(arr(g2(k["delta"]))), ptr(abc), ctypes.c_size_t(12), ptr(a), ptr(b), ptr(c),
                                                   ctypes.c_size_t(8), ptr(inp), ctypes.c_size_t(n_inputs), strong, ptr(ok))
        assert rc == 0
        return list(ok)

    assert run(k["statements"], 11, 0) == [1] * 8 == run(k["statements"], 11, 1)
    assert run(st, 11, 1) == [1, 1, 1, 0, 1, 1, 1, 1]
    assert run([s[:10] for s in k["statements"]], 10, 1) == [0] * 8
    assert run([s[:10] for s in k["statements"]], 10, 0) == [0] * 8  # the eleventh input of every statement is not zero
