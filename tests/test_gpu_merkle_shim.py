"""lpc_commitment_scheme_hip with the device tree builder (hip/merkle.hpp: device_merkle_builder, SHA2-256 on the GPU) against the same
scheme with a host builder that keeps the leaves it is handed: Python hashes the captured leaves with hashlib, and the commit roots and every
FRI round root must be those; the evaluations, the FRI alphas and the final polynomial must not depend on who hashes.
Harness: tests/cpp/merkle_test.cpp -> libmerkletest.so (a target of tests/cpp/Makefile)."""
import ctypes

import numpy as np
import pytest

import cport as cp
import merkle_ref as mr
import pyoracle as po
from harness import library
from util import CURVES, fr_arr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness():
    lib = library("libmerkletest.so")
    for f in (lib.merkle_captured_count, lib.merkle_captured_elements, lib.merkle_captured_per_leaf):
        f.restype = ctypes.c_size_t
    lib.merkle_captured_elements.argtypes = lib.merkle_captured_per_leaf.argtypes = [ctypes.c_size_t]
    lib.merkle_captured_copy.argtypes = [ctypes.c_size_t, ctypes.c_void_p]
    return lib


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _run(lib, curve, device, evals, logs, log_domain, steps, points, challenges):
    nfinal, rounds = 1 << (log_domain - sum(steps)), sum(steps)
    out = dict(roots=np.zeros((2, 32), dtype=np.uint8), fri=np.zeros((len(steps), 32), dtype=np.uint8), z=np.zeros((6, 4), dtype=np.uint64),
               alphas=np.zeros((rounds, 4), dtype=np.uint64), final=np.zeros((nfinal, 4), dtype=np.uint64), counts=np.zeros(6, dtype=np.uint64))
    lg, st = np.array(logs, dtype=np.uint64), np.array(steps, dtype=np.uint64)
    rc = lib.merkle_lpc_run(curve, device, P(evals), ctypes.c_size_t(len(logs)), P(lg), ctypes.c_size_t(log_domain), P(st), ctypes.c_size_t(len(steps)),
                            P(points), P(challenges), ctypes.c_size_t(len(challenges)), P(out["roots"]), P(out["fri"]), P(out["z"]), P(out["alphas"]),
                            P(out["final"]), P(out["counts"]))
    assert rc == 0, (rc, "device" if device else "host")
    return out


@pytest.mark.parametrize("steps", [[1], [1, 1, 2], [3, 2]])
@pytest.mark.parametrize("curve,log_rows", [(0, 6), (1, 7), (0, 9), (1, 12), (0, 14), (0, 16)])
def test_lpc_device_builder_roots_are_the_hashed_leaves(harness, curve, log_rows, steps):
    """four polynomials of up to 2^log_rows rows in two batches (the first fixed), domain 2^(log_rows + 1), ragged point sets"""
    lib = harness
    r = CURVES[curve].r
    log_domain = log_rows + 1
    logs = [log_rows - 1, log_rows - 1, log_rows, log_rows - 1]
    evals = np.concatenate([cp.random_fr(curve, 1500 + i, 1 << l).reshape(-1, 4) for i, l in enumerate(logs)])
    rng = po.SplitMix64(77 + curve + log_rows)
    points = fr_arr([rng.next_mod(r) for _ in range(3)])
    etha, theta = rng.next_mod(r), rng.next_mod(r)
    alphas = [rng.next_mod(r) for _ in range(sum(steps))]
    challenges = fr_arr([etha, etha, theta] + alphas)

    dev = _run(lib, curve, 1, evals, logs, log_domain, steps, points, challenges)
    host = _run(lib, curve, 0, evals, logs, log_domain, steps, points, challenges)
    try:
        # the trees the host run built, in order: commit(0), commit(1), then one per FRI round
        assert lib.merkle_captured_count() == 2 + len(steps)
        expect = []
        for i in range(2 + len(steps)):
            n, per = lib.merkle_captured_elements(i), lib.merkle_captured_per_leaf(i)
            leaves = np.zeros((n, 4), dtype=np.uint64)
            assert lib.merkle_captured_copy(i, P(leaves)) == 0
            step = steps[0] if i < 3 else steps[i - 2]
            assert per == (2 if i < 2 else 1) << step and n % per == 0
            expect.append(mr.tree(leaves, n // per)[-1])
        assert np.array_equal(dev["roots"], np.stack(expect[:2]))
        assert np.array_equal(dev["fri"], np.stack(expect[2:]))
    finally:
        lib.merkle_captured_clear()
    # who hashes changes nothing else
    for k in ("z", "alphas", "final", "counts"):
        assert np.array_equal(dev[k], host[k]), k
    assert list(dev["counts"]) == [6, len(steps), 1 << (log_domain - sum(steps)), len(challenges), 2 + len(steps), sum(steps)]
    assert np.array_equal(dev["alphas"], fr_arr(alphas))
