"""The SHA2-256 core of the device Merkle trees (crypto3-zk_amd/csrc/sha256.hpp: compression function, element-to-words step, padding,
inner-node hash) compiled for the CPU into libzkhip_hosttest.so, against hashlib.  The kernels of merkle.hip call the same functions."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

import merkle_ref as mr
import pyoracle as po
from util import fr_arr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_hosttest.so")
ALL_ONES = (1 << 256) - 1  # not a field element: the hash takes the limbs as they are


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run __graft_entry__.build()")
    return ctypes.CDLL(SO)


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _values(rng, r, n):
    """n elements cycling through the edge values and random ones"""
    edge = [0, 1, r - 1, ALL_ONES]
    return [edge[i % 4] if (i // 4) % 2 == 0 else rng.randrange(r) for i in range(n)]


def test_element_bytes_are_the_big_endian_integer():
    """the checker's own encoding, against int.to_bytes"""
    v = [0, 1, po.BN254.r - 1, ALL_ONES, 0x0102030405060708090A0B0C0D0E0F101112131415161718191A1B1C1D1E1F20]
    assert mr.element_bytes(fr_arr(v)) == b"".join(x.to_bytes(32, "big") for x in v)


@pytest.mark.parametrize("curve", [0, 1])
def test_hash_elements_against_hashlib(shim, curve):
    """messages of 1 to 70 elements (32 to 2240 bytes): both padding shapes (bytes = 0 and 32 mod 64), one block to 35 blocks"""
    r = (po.BLS12_381, po.BN254)[curve].r
    rng = random.Random(900 + curve)
    out = np.zeros(32, dtype=np.uint8)
    for n in range(1, 71):
        for shift in range(3):  # rotate which edge value lands where
            vals = _values(rng, r, n + shift)[shift:]
            a = fr_arr(vals)
            assert shim.zkt_sha256_elements(P(a), ctypes.c_size_t(n), P(out)) == 0
            want = hashlib.sha256(b"".join(v.to_bytes(32, "big") for v in vals)).digest()
            assert out.tobytes() == want, (n, shift)
    assert shim.zkt_sha256_elements(P(a), ctypes.c_size_t(0), P(out)) == -1


@pytest.mark.parametrize("single", [0, 1, po.BLS12_381.r - 1, po.BN254.r - 1, ALL_ONES])
def test_single_edge_elements(shim, single):
    out = np.zeros(32, dtype=np.uint8)
    for n in (1, 2, 3):
        a = fr_arr([single] * n)
        assert shim.zkt_sha256_elements(P(a), ctypes.c_size_t(n), P(out)) == 0
        assert out.tobytes() == hashlib.sha256(single.to_bytes(32, "big") * n).digest()


@pytest.mark.parametrize("n_leaves", [1, 2, 8, 1024])
@pytest.mark.parametrize("per_leaf", [1, 2, 5])
def test_cpu_tree_against_python_tree(shim, n_leaves, per_leaf):
    """every digest of the tree -- leaf digests, every level, the root -- in the external layout"""
    rng = random.Random(n_leaves * 10 + per_leaf)
    leaves = fr_arr(_values(rng, po.BLS12_381.r, n_leaves * per_leaf))
    out = np.zeros((2 * n_leaves - 1, 32), dtype=np.uint8)
    assert shim.zkt_merkle_tree(P(leaves), ctypes.c_size_t(n_leaves), ctypes.c_size_t(per_leaf), P(out)) == 0
    want = mr.tree(leaves, n_leaves)
    assert np.array_equal(out, want)
    if n_leaves == 1:
        assert out[0].tobytes() == hashlib.sha256(mr.element_bytes(leaves)).digest()  # one leaf: the root is its digest
    for i in {0, n_leaves - 1, n_leaves // 3}:
        leaf = mr.element_bytes(leaves[i * per_leaf:(i + 1) * per_leaf])
        assert mr.root_from_path(leaf, i, mr.path_from_digests(out, n_leaves, i)) == out[-1].tobytes()


def test_cpu_tree_refuses_bad_shapes(shim):
    a, out = fr_arr([1, 2, 3]), np.zeros((8, 32), dtype=np.uint8)
    assert shim.zkt_merkle_tree(P(a), ctypes.c_size_t(3), ctypes.c_size_t(1), P(out)) == -1
    assert shim.zkt_merkle_tree(P(a), ctypes.c_size_t(0), ctypes.c_size_t(1), P(out)) == -1
    assert shim.zkt_merkle_tree(P(a), ctypes.c_size_t(2), ctypes.c_size_t(0), P(out)) == -1
