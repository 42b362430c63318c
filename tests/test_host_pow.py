"""The proof-of-work candidate function of the grinding kernel (crypto3-zk_amd/csrc/pow.hpp: candidate, the reference's search loop, the
byte-string SHA2-256 behind zkhip_sha256_host) compiled for the CPU into libzkhip_hosttest.so, against hashlib.  The kernel of pow.hip calls
the same functions.  The checker (hashlib) is tests/pow_ref.py."""
import ctypes
import hashlib
import os
import random

import pytest

from pow_ref import M32, cand, first_hit, st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_hosttest.so")


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(SO)
    lib.zkt_pow_candidate.restype = ctypes.c_uint32
    lib.zkt_pow_candidate.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    lib.zkt_pow_grind_cpu.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32),
                                      ctypes.POINTER(ctypes.c_uint64)]
    lib.zkt_sha256_bytes.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    return lib


def grind_cpu(lib, state, start, mask, max_tries=0):
    nonce, tried = ctypes.c_uint32(), ctypes.c_uint64()
    rc = lib.zkt_pow_grind_cpu(state, start, mask, max_tries, ctypes.byref(nonce), ctypes.byref(tried))
    return rc, nonce.value, tried.value


EDGE_NONCES = [0, 1, 0x80000000, 0xFFFFFFFF, 0x01020304]  # 0x01020304: four different bytes, a byte-order slip shows


def test_candidate_against_hashlib_random(shim):
    rng = random.Random(4100)
    for _ in range(200):
        state, n = rng.randbytes(32), rng.randrange(1 << 32)
        assert shim.zkt_pow_candidate(state, n) == cand(state, n), (state.hex(), n)


@pytest.mark.parametrize("state", [bytes(32), b"\xff" * 32, st(0), bytes(range(32))], ids=["zeros", "ones", "st0", "counting"])
def test_candidate_edge_nonces_and_states(shim, state):
    for n in EDGE_NONCES:
        assert shim.zkt_pow_candidate(state, n) == cand(state, n), hex(n)


@pytest.mark.parametrize("i,start,mask", [(0, 12345, 0xFFFF), (5, 0, 0xFFFF), (0, 7, 0xFF), (6, 0xFFFFFF00, 0xFF), (3, 7, 0x80000001)])
def test_cpu_loop_against_python_loop(shim, i, start, mask):
    k = first_hit(st(i), start, mask)
    assert grind_cpu(shim, st(i), start, mask) == (0, (start + k) & M32, k + 1)
    if (i, start, mask) == (0, 12345, 0xFFFF):
        assert (start + k, k) == (28018, 15673)


def test_cpu_loop_wraps_past_2_32(shim):
    start, mask = 0xFFFFFFF0, 0xFF
    k = first_hit(st(0), start, mask)
    assert (start + k) & M32 < start and ((start + k) & M32, k) == (0x93, 163)
    assert grind_cpu(shim, st(0), start, mask) == (0, 0x93, 164)


def test_cpu_loop_respects_max_tries(shim):
    state, start, mask = st(0), 12345, 0xFFFF
    k = first_hit(state, start, mask)
    assert k % 256 != 0
    rc, _, tried = grind_cpu(shim, state, start, mask, k)  # the hit is the first offset NOT tried
    assert (rc, tried) == (1, k)
    assert grind_cpu(shim, state, start, mask, k + 1) == (0, start + k, k + 1)
    assert grind_cpu(shim, state, start, 0, 1) == (0, start, 1)  # mask 0 accepts the first nonce
    assert grind_cpu(shim, state, start, mask, (1 << 32) + 1)[0] == -1


def test_host_hash_against_hashlib(shim):
    """lengths 0..130: every padding shape (55 / 56 / 63 / 64 / 119 / 120 bytes: the length field fits, or takes a block of its own)"""
    rng = random.Random(4200)
    out = ctypes.create_string_buffer(32)
    for n in range(131):
        msg = rng.randbytes(n)
        assert shim.zkt_sha256_bytes(msg, n, out) == 0
        assert out.raw == hashlib.sha256(msg).digest(), n
    assert shim.zkt_sha256_bytes(None, 1, out) == -1 and shim.zkt_sha256_bytes(b"", 0, None) == -1


def test_library_host_hash_needs_no_gpu(zk):
    """zkhip_sha256_host, the exported twin: no context"""
    for msg in (b"", b"\x00", b"abc", bytes(range(200))):
        assert zk.sha256_host(msg) == hashlib.sha256(msg).digest()
    lib = zk.load_library()
    assert lib.zkhip_sha256_host(None, 1, ctypes.create_string_buffer(32)) == -2
    assert lib.zkhip_strerror(zk.ERR_NOT_FOUND) == b"search ended without a result"
