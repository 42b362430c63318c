"""zkhip_pow_grind (crypto3-zk_amd/csrc/pow.hip): the device's search for FRI's proof of work must return what the reference's loop returns
from the same starting value -- the FIRST accepted nonce, not any accepted nonce -- whatever the chunking.  Every expected value is
computed here by the Python loop over hashlib (tests/pow_ref.py)."""
import ctypes

import pytest

from pow_ref import M32, cand, first_hit, st

pytestmark = pytest.mark.gpu


def expect(state, start, mask, max_tries=1 << 32):
    k = first_hit(state, start, mask, max_tries)
    return ((start + k) & M32, k + 1)


def test_mask_zero_accepts_the_start(ctx):
    for start in (0, 12345, 0xFFFFFFFF):
        for chunk_log in (0, 8, 16):
            assert ctx.pow_grind(st(0), start, 0, chunk_log=chunk_log) == (start, 1)


@pytest.mark.parametrize("i,start,mask,nonce,offset", [(0, 12345, 0xFFFF, 28018, 15673), (2, 7, 0xFF000000, 171, 164), (3, 7, 0x80000001, 7, 0),
                                                      (4, 0, 0x000FF000, 233, 233)])
def test_mask_shapes(ctx, i, start, mask, nonce, offset):
    assert expect(st(i), start, mask) == (nonce, offset + 1)  # the quoted values are the loop's
    assert ctx.pow_grind(st(i), start, mask) == (nonce, offset + 1)


def test_twenty_bit_mask(ctx):
    """~2^20 candidates: the hit lies behind the first chunks at every chunk size below 2^20"""
    state, start, mask = st(1), 0x89ABCDEF, 0xFFFFF
    want = expect(state, start, mask)
    assert want == (2310692188, 954221 + 1)
    assert ctx.pow_grind(state, start, mask) == want
    assert ctx.pow_grind(state, start, mask, chunk_log=16) == want


@pytest.mark.parametrize("i", [0, 1, 2, 3, 4, 5, 6, 7])
def test_many_hits_in_one_launch_first_one_wins(ctx, i):
    """mask 3: a quarter of the 2^16 offsets of the one launch are hits; the smallest must come back"""
    start = (0x9E3779B9 * (i + 1)) & M32
    want = expect(st(i), start, 0x3)
    assert ctx.pow_grind(st(i), start, 0x3, chunk_log=16) == want
    assert cand(st(i), want[0]) & 0x3 == 0 and all(cand(st(i), (start + k) & M32) & 0x3 for k in range(want[1] - 1))


def test_chunk_boundaries(ctx):
    """starts that put the hit on the last offset of a 256-chunk, on the first of the next, and around; Python recomputes every expectation
    (an earlier hit may intervene).  The chunk size never changes the answer."""
    state, mask = st(0), 0xFFF
    h = (12345 + first_hit(state, 12345, mask)) & M32
    for start in (h, h - 1, h - 255, h - 256, h - 257):
        start &= M32
        want = expect(state, start, mask)
        for chunk_log in (8, 12, 0):
            assert ctx.pow_grind(state, start, mask, chunk_log=chunk_log) == want, (hex(start), chunk_log)
    state, start, mask = st(5), 99, 0xFFFF  # a hit many 256-chunks in
    want = expect(state, start, mask)
    for chunk_log in (8, 12, 0):
        assert ctx.pow_grind(state, start, mask, chunk_log=chunk_log) == want


def test_wrap_around(ctx):
    state, start, mask = st(0), 0xFFFFFFF0, 0xFF
    nonce, tried = expect(state, start, mask)
    assert nonce < start and (nonce, tried) == (0x93, 164)  # the search crosses 2^32
    for chunk_log in (8, 0):
        assert ctx.pow_grind(state, start, mask, chunk_log=chunk_log) == (nonce, tried)


def test_max_tries(ctx):
    state, start, mask = st(0), 12345, 0xFFFF
    k = first_hit(state, start, mask)
    assert k % 256 != 0
    for chunk_log in (8, 0):
        assert ctx.pow_grind(state, start, mask, max_tries=k, chunk_log=chunk_log) == (None, k)  # ZKHIP_ERR_NOT_FOUND: the hit is the first offset not tried
        assert ctx.pow_grind(state, start, mask, max_tries=k + 1, chunk_log=chunk_log) == ((start + k) & M32, k + 1)
    assert ctx.pow_grind(state, start, mask, max_tries=1, chunk_log=8) == (None, 1)


def test_argument_errors_leave_the_context_usable(zk, ctx):
    lib = ctx.lib
    nonce, tried = ctypes.c_uint32(), ctypes.c_uint64()
    N, T = ctypes.byref(nonce), ctypes.byref(tried)
    state = st(0)
    INVALID, RANGE = -2, -5
    assert lib.zkhip_pow_grind(None, zk.HASH_SHA2_256, state, 0, 0xFF, 0, 0, N, T) == INVALID
    assert lib.zkhip_pow_grind(ctx.h, zk.HASH_SHA2_256, None, 0, 0xFF, 0, 0, N, T) == INVALID
    assert lib.zkhip_pow_grind(ctx.h, zk.HASH_SHA2_256, state, 0, 0xFF, 0, 0, None, T) == INVALID
    assert lib.zkhip_pow_grind(ctx.h, zk.HASH_SHA2_256 + 1, state, 0, 0xFF, 0, 0, N, T) == INVALID
    for chunk_log in (1, 7, 33, 64):
        assert lib.zkhip_pow_grind(ctx.h, zk.HASH_SHA2_256, state, 0, 0xFF, 0, chunk_log, N, T) == RANGE
    assert lib.zkhip_pow_grind(ctx.h, zk.HASH_SHA2_256, state, 0, 0xFF, (1 << 32) + 1, 0, N, T) == RANGE
    assert lib.zkhip_pow_grind(ctx.h, zk.HASH_SHA2_256, state, 7, 0xFF, 1 << 20, 32, N, None) == 0  # `tried` may be null; 32 is the largest chunk (clipped to max_tries)
    assert nonce.value == expect(state, 7, 0xFF)[0]
    assert lib.zkhip_strerror(zk.ERR_NOT_FOUND) == b"search ended without a result"
    assert ctx.pow_grind(state, 12345, 0xFFFF) == (28018, 15674)
