"""The checker of the proof-of-work tests: the candidate function and the reference's search loop over hashlib (nothing of the project)."""
import hashlib

M32 = 0xFFFFFFFF


def cand(state, n):
    """the checker: int_challenge<uint32_t> of the sequential SHA2-256 transcript after absorbing the nonce's four big-endian bytes"""
    return int.from_bytes(hashlib.sha256(hashlib.sha256(state + n.to_bytes(4, "big")).digest()).digest()[28:], "big")


def st(i):
    return hashlib.sha256(b"zkhip-pow-%d" % i).digest()


def first_hit(state, start, mask, max_tries=1 << 32):
    """the reference's loop: the offset k of the first accepted nonce start + k (mod 2^32), or None below max_tries"""
    for k in range(max_tries):
        if cand(state, (start + k) & M32) & mask == 0:
            return k
    return None
