"""Whole LPC opening proofs from the shim: lpc_commitment_scheme_hip::proof_eval_full (proof_eval, then the query phase answered on the
device) and verify_eval, through tests/cpp/fri_query_test.cpp -> libfriquerytest.so (a target of tests/cpp/Makefile).

Held against things the product does not compute: the query indices against a table of the domain, the initial values against the committed
polynomials extended with the oracle's NTT (cport.ntt) at the restated calculate_s indices (fri_query_ref), every y against the round
polynomial the commit phase kept, the last y against big-integer Horner over the final polynomial, and every path -- values put into leaf
order, hashed with hashlib -- against the batch root or the round's root.  Every comparison is bit-exact."""
import ctypes

import numpy as np
import pytest

import cport as cp
import fri_query_ref as fq
import merkle_ref as mr
import pasta_util  # noqa: F401  (adds Pallas and Vesta to util.CURVES)
import pyoracle as po
from harness import library
from util import CURVES, fr_arr, fr_ints, limbs

pytestmark = pytest.mark.gpu
LAMBDA = 5
DEVICE, HOST, HOST_GROUP = 0, 1, 2


@pytest.fixture(scope="module")
def harness():
    return library("libfriquerytest.so")


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _inputs(curve, log_rows, steps, lam=LAMBDA):
    """four polynomials of mixed sizes in two batches (one already of D[0]'s size), three opening points, and the script of a transcript:
    etha twice, theta, the alphas, the query challenges"""
    r = CURVES[curve].r
    log_domain = log_rows + 1
    logs = [log_rows - 1, log_rows, log_domain, log_rows - 1]
    evals = [cp.random_fr(curve, 5200 + 10 * log_rows + i, 1 << l).reshape(-1, 4) for i, l in enumerate(logs)]
    rng = po.SplitMix64(91 + 7 * curve + log_rows + 100 * len(steps) + steps[0])
    points = fr_arr([rng.next_mod(r) for _ in range(3)])
    etha = rng.next_mod(r)
    script = [etha, etha] + [rng.next_mod(r) for _ in range(1 + sum(steps))] + [rng.next_mod(r - 1) + 1 for _ in range(lam)]
    return dict(curve=curve, log_domain=log_domain, logs=logs, evals=evals, steps=list(steps), points=points, script=script, lam=lam)


def _run(lib, inp, mode, grind_mask=0, scripted=True):
    steps, lam, n, logs = inp["steps"], inp["lam"], inp["log_domain"], inp["logs"]
    R, r_total = len(steps), sum(steps)
    pairs0, depth0 = 1 << (steps[0] - 1), n - steps[0]
    t_of = [sum(steps[:i]) for i in range(R)]
    y_sizes = [(1 << (steps[i + 1] - 1)) if i + 1 < R else 1 for i in range(R)]
    depths = [n - t_of[i] - steps[i] for i in range(R)]
    out = dict(roots=np.zeros((2, 32), dtype=np.uint8), fri=np.zeros((R, 32), dtype=np.uint8), z=np.zeros((6, 4), dtype=np.uint64),
               final=np.zeros((1 << (n - r_total), 4), dtype=np.uint64), nonce=ctypes.c_uint32(), counts=np.zeros(8, dtype=np.uint64),
               drawn=np.zeros((64, 4), dtype=np.uint64), init_values=np.zeros((lam * 4 * pairs0 * 2, 4), dtype=np.uint64),
               init_leaf=np.zeros((2, lam), dtype=np.uint64), init_paths=np.zeros((2, lam, depth0, 32), dtype=np.uint8),
               y=np.zeros((lam * sum(y_sizes) * 2, 4), dtype=np.uint64), round_leaf=np.zeros((R, lam), dtype=np.uint64),
               round_paths=np.zeros(lam * sum(depths) * 32 + 1, dtype=np.uint8),
               round_polys=np.zeros((sum(1 << (n - t) for t in t_of), 4), dtype=np.uint64), flags=ctypes.c_uint32())
    ev = np.concatenate(inp["evals"])
    lg, st = np.array(logs, dtype=np.uint64), np.array(steps, dtype=np.uint64)
    script = fr_arr(inp["script"]) if scripted else np.zeros((0, 4), dtype=np.uint64)
    seed = np.frombuffer(b"fri query test", dtype=np.uint8)
    sz = ctypes.c_size_t
    rc = lib.fq_lpc_run(inp["curve"], mode, P(ev), sz(len(logs)), P(lg), sz(n), P(st), sz(R), P(inp["points"]), P(script), sz(len(script)), sz(lam),
                        ctypes.c_uint32(grind_mask), P(seed), sz(len(seed)), P(out["roots"]), P(out["fri"]), P(out["z"]), P(out["final"]),
                        ctypes.byref(out["nonce"]), P(out["counts"]), P(out["drawn"]), P(out["init_values"]), P(out["init_leaf"]), P(out["init_paths"]),
                        P(out["y"]), P(out["round_leaf"]), P(out["round_paths"]), P(out["round_polys"]), ctypes.byref(out["flags"]))
    assert rc == 0, (rc, mode)
    # the flat buffers as the proof's parts
    iv, at = out["init_values"], 0
    out["initial"] = []
    for count in (2, 2):
        size = lam * count * pairs0 * 2
        out["initial"].append(iv[at:at + size].reshape(lam, count, pairs0, 2, 4))
        at += size
    out["ys"], out["paths"], out["polys"] = [], [], []
    at = pat = fat = 0
    for i in range(R):
        out["ys"].append(out["y"][at:at + lam * y_sizes[i] * 2].reshape(lam, 1, y_sizes[i], 2, 4))
        at += lam * y_sizes[i] * 2
        out["paths"].append(out["round_paths"][pat:pat + lam * depths[i] * 32].reshape(lam, depths[i], 32))
        pat += lam * depths[i] * 32
        out["polys"].append(out["round_polys"][fat:fat + (1 << (n - t_of[i]))])
        fat += 1 << (n - t_of[i])
    out["flags"], out["nonce"] = out["flags"].value, out["nonce"].value
    return out


def _check_proof(inp, out, scripted=True):
    """everything a whole proof holds, against the oracle, big integers and hashlib; -> the query indices"""
    curve, steps, lam, n = inp["curve"], inp["steps"], inp["lam"], inp["log_domain"]
    C = CURVES[curve]
    r, R, D0 = C.r, len(steps), 1 << n
    total = int(out["counts"][1])
    # etha (twice from a script, once from the hashing transcript: preprocess draws it from a copy), theta, the alphas, the query challenges
    assert total == (3 if scripted else 2) + sum(steps) + lam and int(out["counts"][3]) == total - lam
    # the query indices, from the challenges the transcript handed out last, against a table of the domain
    table = fq.domain_table(C.root_of_unity(n), D0, r)
    xs = [table[pow(c, (r - 1) >> n, r)] for c in fr_ints(out["drawn"][total - lam:total])]
    # initial proofs: the committed polynomials on D[0] (inverse NTT, zero padding, NTT: the oracle's) at the restated indices
    w0 = limbs(C.root_of_unity(n), 4)
    ext = []
    for e, l in zip(inp["evals"], inp["logs"]):
        coeffs = cp.ntt(curve, e.reshape(1, -1, 4), l, limbs(C.root_of_unity(l), 4), inverse=True)[0]
        padded = np.zeros((1, D0, 4), dtype=np.uint64)
        padded[0, :len(coeffs)] = coeffs
        ext.append(cp.ntt(curve, padded, n, w0)[0])
    leaves0 = D0 >> steps[0]
    for k, polys in enumerate((ext[:2], ext[2:])):
        assert np.array_equal(out["initial"][k], fq.expected_answers(np.stack(polys), steps[0], xs)), k
        for q, x in enumerate(xs):
            assert int(out["init_leaf"][k][q]) == x % leaves0
            leaf = mr.element_bytes(fq.leaf_order(out["initial"][k][q], x, D0, steps[0]))
            assert mr.root_from_path(leaf, x % leaves0, out["init_paths"][k][q]) == out["roots"][k].tobytes(), (k, q)
    # round proofs: the leaf of round i is fs[i] at the pairs walked from x, y of round i is fs[i + 1] at the next round's pairs
    t = 0
    for i in range(R):
        N = 1 << (n - t)
        leaves = N >> steps[i]
        f = out["polys"][i].reshape(1, N, 4)
        for q, x in enumerate(xs):
            assert int(out["round_leaf"][i][q]) == x % leaves
            values = fq.expected_answers(f, steps[i], [x % N])[0]
            leaf = mr.element_bytes(fq.leaf_order(values, x % N, N, steps[i]))
            assert mr.root_from_path(leaf, x % leaves, out["paths"][i][q]) == out["fri"][i].tobytes(), (i, q)
        t += steps[i]
        if i + 1 < R:
            nxt = out["polys"][i + 1].reshape(1, 1 << (n - t), 4)
            assert np.array_equal(out["ys"][i], fq.expected_answers(nxt, steps[i + 1], [x % (1 << (n - t)) for x in xs])), i
    # the last y: the final polynomial at x^2 and -x^2 (x over the last round's domain), by big-integer Horner
    final = fr_ints(out["final"])
    horner = lambda v: sum(c * pow(v, k, r) for k, c in enumerate(final)) % r
    N = 1 << (n - (sum(steps) - 1))
    for q, x in enumerate(xs):
        xl = x % N
        x2 = pow(C.root_of_unity(n - (sum(steps) - 1)), 2 * xl, r)
        ind = 0 if xl % (N // 2) < N // 4 else 1
        got = fr_ints(out["ys"][R - 1][q])
        assert got[ind] == horner(x2) and got[1 - ind] == horner(r - x2), q
    return xs


ALL_REJECTED = sum(1 << b for b in range(1, 7))


@pytest.mark.parametrize("steps", [[1], [1, 1, 1], [2, 1], [3, 1, 1]])
@pytest.mark.parametrize("curve,log_rows", [(0, 4), (1, 4), (2, 4), (3, 4), (0, 9), (2, 9), (0, 12), (2, 12)])
def test_whole_proofs_device_builder(harness, curve, log_rows, steps):
    """the proof against the oracle; verify_eval -- on a scheme object of its own that only knows what a verifier knows, max_degree + 1 =
    |D[0]| / 2 -- accepts it, rejects it after each single change, rejects it under half that max_degree (the final polynomial is of full
    degree: one committed vector is as long as D[0]) and refuses to run with max_degree unset"""
    inp = _inputs(curve, log_rows, steps)
    out = _run(harness, inp, DEVICE)
    _check_proof(inp, out)
    flags = out["flags"]
    assert flags & 1, "verify_eval rejects the proof"
    assert flags & ALL_REJECTED == ALL_REJECTED, f"verify_eval accepts a changed proof: {flags:#x}"
    assert flags & (1 << 8), "proof_eval on a second scheme object gives another z / roots / final polynomial / nonce / transcript traffic"
    assert flags & (1 << 9), "proof_eval filled query_proofs"
    assert flags & (1 << 10), "a verifier whose max_degree is half of what the committed vectors need accepts their full-degree final polynomial"
    assert flags & (1 << 11), "verify_eval runs without a degree bound (fri_params.max_degree unset)"
    assert out["nonce"] == 0 and int(out["counts"][4]) == int(out["counts"][3])


def test_whole_proof_with_grinding(harness):
    """the SHA2-256 transcript itself (no script), 8 bits of proof of work between the commit and the query phase"""
    inp = _inputs(0, 4, [1, 1, 1])
    out = _run(harness, inp, DEVICE, grind_mask=0xFF, scripted=False)
    _check_proof(inp, out, scripted=False)
    flags = out["flags"]
    assert flags & 1 and flags & (1 << 8) and flags & (1 << 9) and flags & (1 << 10) and flags & (1 << 11)
    assert flags & (ALL_REJECTED | 1 << 7) == ALL_REJECTED | 1 << 7, f"verify_eval accepts a changed proof: {flags:#x}"


def test_host_builder_and_device_group(harness):
    """a host tree builder (the tree answers through proof(i)), on one context and over a device group of two members on one GPU: the same
    proof"""
    inp = _inputs(0, 6, [2, 1])
    one = _run(harness, inp, HOST)
    xs = _check_proof(inp, one)
    grp = _run(harness, inp, HOST_GROUP)
    assert _check_proof(inp, grp) == xs
    assert int(grp["counts"][5]) == 2 and int(one["counts"][5]) == 0
    for k in ("roots", "fri", "z", "final", "init_values", "init_leaf", "init_paths", "y", "round_leaf", "round_paths"):
        assert np.array_equal(one[k], grp[k]), k
    dev = _run(harness, inp, DEVICE)
    for k in ("roots", "fri", "z", "final", "init_values", "init_leaf", "init_paths", "y", "round_leaf", "round_paths"):
        assert np.array_equal(one[k], dev[k]), k


def test_query_phase_refusals(harness):
    """lambda = 0, a step list that does not end in 1, query_phase before proof_eval: std::invalid_argument, the transcript untouched"""
    inp = _inputs(0, 4, [1, 2])
    ev = np.concatenate(inp["evals"])
    lg = np.array(inp["logs"], dtype=np.uint64)
    script = fr_arr(inp["script"])
    flags = ctypes.c_uint32()
    sz = ctypes.c_size_t
    rc = harness.fq_refusals(0, P(ev), sz(4), P(lg), sz(inp["log_domain"]), P(inp["points"]), P(script), sz(len(script)), sz(LAMBDA), ctypes.byref(flags))
    assert rc == 0
    assert flags.value == 0b111, f"{flags.value:#b}"


@pytest.mark.parametrize("curve", [0, 1, 2, 3])
def test_domain_index_is_the_scan_s_index(harness, curve):
    """detail::domain_index against a table of the domain, log_domain <= 12: 1, -1, omega, omega^(D - 1) and random elements; a zero challenge
    (which maps to 0, outside every domain) is refused (the whole domains and the other fields' edge cases: tests/test_host_fri_query.py)"""
    C = CURVES[curve]
    r, out = C.r, ctypes.c_uint64()
    index = lambda x, n: (harness.fq_domain_index(curve, P(limbs(x, 4)), ctypes.c_size_t(n), ctypes.byref(out)), out.value)
    rng = po.SplitMix64(300 + curve)
    for n in range(1, 13):
        D, w = 1 << n, C.root_of_unity(n)
        table = fq.domain_table(w, D, r)
        for x in [1, r - 1, w, pow(w, D - 1, r)] + [pow(rng.next_mod(r - 1) + 1, (r - 1) >> n, r) for _ in range(6)]:
            assert index(x, n) == (0, table[x]), (n, x)
        assert index(pow(0, (r - 1) >> n, r), n)[0] == 1
