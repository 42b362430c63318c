"""The Merkle-tree convention of include/zkhip.h ("Merkle trees") restated with hashlib, for the tests: independent of the product.
An element is the 32-byte big-endian encoding of its canonical integer; a leaf digest is SHA2-256 of the leaf's elements in order; an inner
node is SHA2-256(left || right); the digest array holds the L leaf digests, then each level above, the root last."""
import hashlib

import numpy as np


def element_bytes(limbs) -> bytes:
    """(..., 4) canonical little-endian u64 limbs -> the elements' big-endian encodings, concatenated"""
    a = np.asarray(limbs, dtype=np.uint64).reshape(-1, 4)
    return np.ascontiguousarray(a[:, ::-1]).astype(">u8").tobytes()


def tree(leaves, n_leaves: int) -> np.ndarray:
    """leaves: n_leaves x per_leaf x 4 u64 limbs (any shape with that element count) -> (2 n_leaves - 1, 32) u8"""
    assert n_leaves >= 1 and n_leaves & (n_leaves - 1) == 0
    raw = element_bytes(leaves)
    per = len(raw) // n_leaves
    assert per * n_leaves == len(raw) and per % 32 == 0 and per > 0
    level = [hashlib.sha256(raw[i * per:(i + 1) * per]).digest() for i in range(n_leaves)]
    out = list(level)
    while len(level) > 1:
        level = [hashlib.sha256(level[2 * j] + level[2 * j + 1]).digest() for j in range(len(level) // 2)]
        out += level
    return np.frombuffer(b"".join(out), dtype=np.uint8).reshape(2 * n_leaves - 1, 32)


def level_offset(n_leaves: int, level: int) -> int:
    return 2 * n_leaves - ((2 * n_leaves) >> level)


def path_from_digests(digests, n_leaves: int, index: int) -> np.ndarray:
    """the sibling digests of leaf `index`, leaf level first, read from a digest array"""
    depth = n_leaves.bit_length() - 1
    return np.stack([digests[level_offset(n_leaves, l) + ((index >> l) ^ 1)] for l in range(depth)]) if depth else np.zeros((0, 32), dtype=np.uint8)


def root_from_path(leaf_bytes: bytes, index: int, path) -> bytes:
    """recompute the root from a leaf's bytes and its authentication path"""
    d = hashlib.sha256(leaf_bytes).digest()
    for l, sib in enumerate(path):
        sib = bytes(bytearray(sib))
        d = hashlib.sha256(sib + d if (index >> l) & 1 else d + sib).digest()
    return d
