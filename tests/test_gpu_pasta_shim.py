"""The header-only shim over `pallas` / `vesta` on the GPU (tests/cpp/pasta_test.cpp -> libpastatest.so, a target of tests/cpp/Makefile):
lpc_commitment_scheme_hip over a sha256_transcript with grinding -- device tree builder, streaming and vector host builders -- against
po.lpc_proof_eval with the transcript replayed by hashlib, every Merkle root against tests/merkle_ref.py and the nonce against
tests/pow_ref.py; multiexp<multiexp_method_hip> on G1 against the oracle.
A placeholder instance over pallas::base_field_type (= F_p) binds to `vesta`, id 3: the id names the group whose SCALAR field that is."""
import ctypes
import hashlib

import numpy as np
import pytest

import merkle_ref as mr
import pasta_util as pu
import pyoracle as po
from pow_ref import cand, first_hit
from test_host_pasta import P, harness  # noqa: F401  (the fixture that builds and loads libpastatest.so)
from util import fr_arr, fr_ints, limbs, pt_from_limbs, pts_arr

pytestmark = pytest.mark.gpu
H = lambda b: hashlib.sha256(b).digest()  # noqa: E731
LOG_ROWS, LOG_DOMAIN, MASK = 8, 10, 0xFF


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def lpc_run(lib, curve, builder, evals, steps, point, init):
    npolys = len(evals) >> LOG_ROWS
    rounds, nfinal = sum(steps), 1 << (LOG_DOMAIN - sum(steps))
    out = dict(commit=np.zeros(32, dtype=np.uint8), fri=np.zeros((len(steps), 32), dtype=np.uint8), final=np.zeros((nfinal, 4), dtype=np.uint64),
               alphas=np.zeros((rounds, 4), dtype=np.uint64), z=np.zeros((npolys, 4), dtype=np.uint64), state=np.zeros(32, dtype=np.uint8),
               counts=np.zeros(4, dtype=np.uint64))
    nonce = ctypes.c_uint32()
    st = np.array(steps, dtype=np.uint64)
    rc = lib.pasta_lpc_run(curve, builder, P(evals), ctypes.c_size_t(npolys), ctypes.c_size_t(LOG_ROWS), ctypes.c_size_t(LOG_DOMAIN), P(st), ctypes.c_size_t(len(steps)),
                           P(point), P(u8(init)), ctypes.c_size_t(len(init)), ctypes.c_uint32(MASK), P(out["commit"]), P(out["fri"]), P(out["final"]), P(out["alphas"]),
                           P(out["z"]), P(out["state"]), ctypes.byref(nonce), P(out["counts"]))
    assert rc == 0, (rc, builder)
    assert list(out["counts"][:3]) == [npolys, nfinal, rounds]
    out["nonce"], out["start"] = nonce.value, int(out["counts"][3])
    return out


@pytest.mark.parametrize("curve,npolys,steps", [(3, 4, [1, 2]), (3, 1, [3]), (3, 4, [3]), (3, 1, [1, 2]), (2, 4, [1, 2])])
def test_lpc_commit_and_fri_commit_phase(harness, curve, npolys, steps):  # noqa: F811
    """batches of 4 and 1 polynomials x 2^8 rows on a 2^10-point domain, step lists [1, 2] and [3], an 8-bit grinding mask"""
    C = pu.CURVES[curve]
    r = C.r
    evals = pu.random_fr(curve, 2000 + npolys, npolys << LOG_ROWS)
    evals[0], evals[1] = limbs(r - 1, 4), 0
    rng = po.SplitMix64(2100 + curve)
    point = rng.next_mod(r)
    init = b"pasta lpc %d" % curve
    dev = lpc_run(harness, curve, 0, evals, steps, fr_arr([point]), init)
    # the transcript, replayed with hashlib from the roots the run returned: the commit root, theta, then per round its root and its alphas
    s = H(H(init) + dev["commit"].tobytes())
    s = H(s)
    theta = int.from_bytes(s, "big") % r
    alphas = []
    for i, step in enumerate(steps):
        s = H(s + dev["fri"][i].tobytes())
        for _ in range(step):
            s = H(s)
            alphas.append(int.from_bytes(s, "big") % r)
    assert fr_ints(dev["alphas"]) == alphas
    # the proof of work: the reference's loop finds the same nonce; the transcript ends behind it
    k = first_hit(s, dev["start"], MASK)      # from the start the scheme drew (std::rand(), pinned by the harness)
    assert dev["nonce"] == (dev["start"] + k) & 0xFFFFFFFF and cand(s, dev["nonce"]) & MASK == 0
    assert dev["state"].tobytes() == H(H(s + dev["nonce"].to_bytes(4, "big")))
    # the oracle's commit phase under those challenges, its trees hashed by hashlib
    polys = [fr_ints(evals[p << LOG_ROWS:(p + 1) << LOG_ROWS]) for p in range(npolys)]
    tree_root = lambda leaves, per_leaf: bytes(mr.tree(fr_arr(leaves), len(leaves) // per_leaf)[-1])  # noqa: E731
    roots, z, fri_roots, final = po.lpc_proof_eval(r, {0: polys}, {0: [[point]] * npolys}, [], LOG_DOMAIN, steps, C.root_of_unity, [0, 0, theta] + alphas, tree_root)
    assert dev["commit"].tobytes() == roots[0]
    assert [bytes(x) for x in dev["fri"]] == fri_roots
    assert fr_ints(dev["z"]) == [v[0] for v in z[0]]
    final = list(final) + [0] * (len(dev["final"]) - len(final))
    assert fr_ints(dev["final"]) == final
    # the same commit through host tree builders (leaves downloaded in slices / at once, hashed with the library's SHA2-256 on the host)
    for builder in (1, 2):
        host = lpc_run(harness, curve, builder, evals, steps, fr_arr([point]), init)
        for key in ("commit", "fri", "final", "alphas", "z", "state"):
            assert np.array_equal(host[key], dev[key]), (builder, key)
        assert host["nonce"] == dev["nonce"]


@pytest.mark.parametrize("curve", [2, 3])
def test_multiexp_of_300_points(harness, curve):  # noqa: F811
    """multiexp<multiexp_method_hip> in the reference's arity (bases uploaded for the call): the Pedersen / kimchi commitment shape"""
    C = pu.CURVES[curve]
    n = 300
    pts = pu.random_points(curve, 31, n)
    pts[5] = None
    pts[7] = pts[6]
    sc = fr_ints(pu.random_fr(curve, 32, n))
    sc[0], sc[1], sc[2] = 0, 1, C.r - 1
    inf = np.array([1 if p is None else 0 for p in pts], dtype=np.uint8)
    out, oinf = np.zeros(8, dtype=np.uint64), ctypes.c_int()
    assert harness.pasta_multiexp(curve, P(pts_arr(curve, 1, pts)), P(inf), P(fr_arr(sc)), ctypes.c_size_t(n), P(out), ctypes.byref(oinf)) == 0
    assert pt_from_limbs(curve, 1, out, oinf.value) == po.msm_pippenger(C.g1, pts, sc)
    # a sum that cancels
    two = [pts[0], pts[0]]
    assert harness.pasta_multiexp(curve, P(pts_arr(curve, 1, two)), None, P(fr_arr([5, C.r - 5])), ctypes.c_size_t(2), P(out), ctypes.byref(oinf)) == 0
    assert oinf.value == 1


def test_eval_polys_shared_case_lpc_pallas(harness):  # noqa: F811
    """the eval_polys case tests/test_gpu_shim.py runs through KZG and LPC (tests/cpp/eval_polys_case.hpp), through LPC over Pallas: proof.z
    equals po.poly_eval entry by entry"""
    from util import eval_polys_case
    evals, points, want = eval_polys_case(pu.CURVES[pu.PALLAS_ID], 8802)
    out = np.zeros((len(want), 4), dtype=np.uint64)
    assert harness.pasta_eval_polys_case(pu.PALLAS_ID, P(evals), P(points), P(out)) == 0
    assert fr_ints(out) == want


@pytest.mark.parametrize("n", [1, 5, 257])
def test_fr_vector_layer(harness, n):  # noqa: F811
    """the fr_vector cases tests/test_gpu_shim.py runs over BLS12-381 and BN254 (tests/cpp/fr_vector_case.hpp), over Pallas's scalar field"""
    from util import run_fr_vector_cases
    run_fr_vector_cases(harness.pasta_fr_vector, pu.PALLAS_ID, pu.CURVES[pu.PALLAS_ID].r, n, 9940 + n)
