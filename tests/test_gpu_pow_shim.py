"""The shim's side of FRI's proof of work: sha256_transcript (hip/transcript.hpp), proof_of_work_hip (hip/proof_of_work.hpp) and
lpc_commitment_scheme_hip::proof_eval with and without fri_params.use_grinding, against hashlib: Python replays every transcript from the
roots a run returns.  Harness: tests/cpp/pow_test.cpp -> libpowtest.so (a target of tests/cpp/Makefile)."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import cport as cp
import pyoracle as po
from harness import library
from pow_ref import cand, first_hit
from util import fr_arr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = po.BLS12_381.r
H = lambda b: hashlib.sha256(b).digest()  # noqa: E731


@pytest.fixture(scope="module")
def harness():
    return library("libpowtest.so")


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def limbs_int(a):
    return sum(int(v) << (64 * i) for i, v in enumerate(a))


@pytest.mark.parametrize("init,msg", [(b"", b""), (b"zkhip", b"\x01\x02\x03\x04"), (bytes(range(70)), bytes(range(200, 255)) * 3)])
def test_sha256_transcript_against_hashlib(harness, init, msg):
    """needs no GPU: the transcript hashes on the host"""
    digest = H(b"a root")
    s = [H(b"\x00"), H(init)]
    s.append(H(s[-1] + msg))
    s.append(H(s[-1] + digest))
    s.append(H(s[-1]))  # challenge
    s.append(H(s[-1]))  # int_challenge
    s.append(H(s[-1] + msg))
    states, chal, ic = np.zeros((7, 32), dtype=np.uint8), np.zeros(4, dtype=np.uint64), ctypes.c_uint32()
    rc = harness.pow_transcript_run(P(u8(init) if init else np.zeros(1, dtype=np.uint8)), ctypes.c_size_t(len(init)),
                                    P(u8(msg) if msg else np.zeros(1, dtype=np.uint8)), ctypes.c_size_t(len(msg)), P(u8(digest)), P(u8(b"".join(s))), P(states), P(chal),
                                    ctypes.byref(ic))
    assert rc == 0, f"state after step {-rc - 1} differs"
    assert states.tobytes() == b"".join(s)
    assert limbs_int(chal) == int.from_bytes(s[4], "big") % R
    assert ic.value == int.from_bytes(s[5][28:], "big")


@pytest.mark.gpu
@pytest.mark.parametrize("init,mask,start", [(b"zkhip-pow-shim", 0xFFFF, 1), (b"another transcript", 0xFFF, 0xFFFFFF00)])
def test_generate_and_verify(harness, init, mask, start):
    hosttest = ctypes.CDLL(os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_hosttest.so"))
    state = H(init)
    k = first_hit(state, start, mask)
    want = (start + k) & 0xFFFFFFFF
    assert cand(state, want ^ 1) & mask != 0, "choose a start whose neighbour does not pass as well"
    nonce, flags = ctypes.c_uint32(), ctypes.c_uint32()
    before, after = np.zeros(32, dtype=np.uint8), np.zeros(32, dtype=np.uint8)
    assert harness.pow_generate_verify(P(u8(init)), ctypes.c_size_t(len(init)), ctypes.c_uint32(mask), ctypes.c_uint32(start), ctypes.byref(nonce), P(before), P(after),
                                       ctypes.byref(flags)) == 0
    cpu_nonce, cpu_tried = ctypes.c_uint32(), ctypes.c_uint64()
    assert hosttest.zkt_pow_grind_cpu(state, ctypes.c_uint32(start), ctypes.c_uint32(mask), ctypes.c_uint64(0), ctypes.byref(cpu_nonce), ctypes.byref(cpu_tried)) == 0
    assert nonce.value == cpu_nonce.value == want and cpu_tried.value == k + 1
    assert before.tobytes() == state
    assert after.tobytes() == H(H(state + want.to_bytes(4, "big")))  # absorb the four big-endian bytes, then the int_challenge
    assert flags.value == 0b011  # verify accepts, both transcripts end alike, nonce ^ 1 is rejected


@pytest.mark.gpu
def test_lpc_proof_eval_with_and_without_grinding(harness):
    """runs 0..2 (grinding off: default-initialised params, the fields spelled out, a transcript without state()) must be one and the same
    proof and leave the transcript where hashlib's replay of the returned roots leaves it; run 3 (mask 0xFFF) adds the nonce and nothing else"""
    mask, init = 0xFFF, b"lpc grinding"
    evals = np.concatenate([cp.random_fr(0, 4300 + i, 1 << 7).reshape(-1, 4) for i in range(2)])
    point = fr_arr([po.SplitMix64(4301).next_mod(R)])
    commit, fri, final = np.zeros((4, 32), dtype=np.uint8), np.zeros((4, 3, 32), dtype=np.uint8), np.zeros((4, 32, 4), dtype=np.uint64)
    states, nonces, counts, flags = np.zeros((4, 32), dtype=np.uint8), np.zeros(4, dtype=np.uint32), np.zeros(2, dtype=np.uint64), ctypes.c_uint32()
    rc = harness.pow_lpc_run(P(evals), P(point), P(u8(init)), ctypes.c_size_t(len(init)), ctypes.c_uint32(mask), P(commit), P(fri), P(final), P(states), P(nonces),
                             P(counts), ctypes.byref(flags))
    assert rc == 0
    assert commit.any() and fri.any() and final.any()
    for k in (1, 2, 3):  # roots and the final polynomial never depend on grinding or on the transcript's type
        assert np.array_equal(commit[k], commit[0]) and np.array_equal(fri[k], fri[0]) and np.array_equal(final[k], final[0]), k
    # the transcript's path, replayed with hashlib: the commit root, theta, then per FRI round its root and its alpha
    s = H(H(init) + commit[0].tobytes())
    s = H(s)
    for i in range(3):
        s = H(H(s + fri[0][i].tobytes()))
    for k in (0, 1, 2):
        assert states[k].tobytes() == s and nonces[k] == 0, k  # grinding off: exactly these calls, no nonce
    assert list(counts) == [4, 4]
    nonce = int(nonces[3])
    assert cand(s, nonce) & mask == 0
    assert states[3].tobytes() == H(H(s + nonce.to_bytes(4, "big")))
    assert flags.value == 0b111  # verify() on the C++ replay accepts and ends in the same state; grinding without state() threw
