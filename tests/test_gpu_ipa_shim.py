"""kimchi_pedersen_hip (crypto3-zk_amd/include/nil/crypto3/zk/hip/kimchi_pedersen.hpp) over the stand-in `pallas` / `vesta` types on the
GPU, driven through tests/cpp/ipa_test.cpp -> libipatest.so (a target of tests/cpp/Makefile) with a sponge that answers from a list, a fixed group map
and a list of draws: commitments, blinders and every part of the opening proof against the Python model (tests/ipa_model.py), the sponge
calls and the draws in the model's number and order, the device's proof in the model's verifier equation, and the shim's own verify_eval
on the proof and on three changed copies of it."""
import numpy as np
import pytest

import arith_cases as ac
import ipa_model as im
import pasta_util as pu
from harness import library
from util import fr_arr, fr_ints, limbs, pt_from_limbs, pts_arr

pytestmark = pytest.mark.gpu
P = ac._ptr
KINDS = {0: "absorb_fr", 1: "challenge_fq", 2: "absorb_g", 3: "squeeze_challenge"}
ENDO_R = 5


@pytest.fixture(scope="module")
def harness():
    return library("libipatest.so")


def u64(n, *shape):
    return np.zeros((n,) + shape, dtype=np.uint64)


def run_device(lib, curve, pp, polys, points, xi, rr, draws, answers):
    n, npolys, npts = len(pp.g), len(polys), len(points)
    r = pp.r
    chunks = [(len(c) + n - 1) // n for c, _ in polys]
    slots, rounds = sum(chunks) + npolys, max(0, (n - 1).bit_length())
    evals = [v for c, _ in polys for per_point in im.chunk_evaluations(c, n, points, r) for v in per_point]
    coeffs = [v for c, _ in polys for v in c]
    log_cap = 4 * (4 + 3 * rounds) + 8
    sizes = np.array([n, npolys, npts, len(draws), len(answers), log_cap], dtype=np.uint64)
    out = dict(comm_xy=u64(slots, 8), comm_inf=u64(slots), comm_count=u64(npolys), blind=u64(slots, 4), lr_xy=u64(max(1, 2 * rounds), 8),
               lr_inf=u64(max(1, 2 * rounds)), tail_xy=u64(2, 8), tail_inf=u64(2), z=u64(2, 4), log=u64(log_cap, 10), counts=u64(11))
    g_inf = np.array([p is None for p in pp.g], dtype=np.uint8)
    rc = lib.ipa_run(curve, P(sizes), P(pts_arr(curve, 1, pp.g)), P(g_inf), P(pts_arr(curve, 1, [pp.h])), P(pts_arr(curve, 1, [pp.u_point])), P(limbs(pp.endo_r, 4)),
                     P(np.array([len(c) for c, _ in polys], dtype=np.uint64)), P(np.array([b for _, b in polys], dtype=np.int64)), P(fr_arr(coeffs)),
                     P(fr_arr(points)), P(fr_arr([xi, rr])), P(fr_arr(evals)), P(fr_arr(draws)), P(fr_arr(answers)), P(out["comm_xy"]), P(out["comm_inf"]),
                     P(out["comm_count"]), P(out["blind"]), P(out["lr_xy"]), P(out["lr_inf"]), P(out["tail_xy"]), P(out["tail_inf"]), P(out["z"]), P(out["log"]),
                     P(out["counts"]))
    assert rc == 0, rc
    assert list(out["comm_count"]) == chunks and int(out["counts"][10]) == rounds
    pt = lambda xy, inf: pt_from_limbs(curve, 1, xy, int(inf))
    commits, blinds, slot = [], [], 0
    for k in chunks:
        pts = [pt(out["comm_xy"][slot + i], out["comm_inf"][slot + i]) for i in range(k + 1)]
        bl = fr_ints(out["blind"][slot:slot + k + 1])
        commits.append((pts[:k], pts[k]))
        blinds.append((bl[:k], bl[k] if pts[k] is not None else None))
        slot += k + 1
    proof = {"lr": [(pt(out["lr_xy"][2 * i], out["lr_inf"][2 * i]), pt(out["lr_xy"][2 * i + 1], out["lr_inf"][2 * i + 1])) for i in range(rounds)],
             "delta": pt(out["tail_xy"][0], out["tail_inf"][0]), "sg": pt(out["tail_xy"][1], out["tail_inf"][1]), "z1": fr_ints(out["z"])[0], "z2": fr_ints(out["z"])[1]}
    logs, at = [], 0
    for count in out["counts"][:2]:
        log = []
        for e in out["log"][at:at + int(count)]:
            kind = KINDS[int(e[0])]
            arg = pt(e[2:], e[1]) if kind == "absorb_g" else (None if kind == "challenge_fq" else fr_ints(e[2:6])[0])
            log.append((kind, arg))
        logs.append(log)
        at += int(count)
    return commits, blinds, proof, logs, [int(x) for x in out["counts"]]


CASES = [
    # curve, |g|, [(length, bound)], evaluation points
    (2, 1, [(1, -1), (4, -1)], 1),                 # no round at all; a polynomial three chunks longer than g
    (3, 2, [(1, -1), (7, 7)], 2),                  # shorter than g; 3 chunks + a shifted tail of one coefficient
    (2, 5, [(5, -1), (18, 18)], 1),                # g padded to 8 with infinity; equal to g; 3 chunks + 3 with a bound
    (3, 8, [(3, 3), (32, -1)], 2),                 # a bound below |g| (the whole polynomial is the shifted part too); three chunks longer, no bound
    (2, 8, [(8, 16)], 1),                          # a bound that ends a chunk, above the length: no shifted part
    (2, 64, [(64, -1), (224, 224)], 2),
    (3, 512, [(512, -1)], 1),                      # ~3 s of model: the largest size of the routine suite
]


@pytest.mark.parametrize("curve,n,shapes,npoints", CASES)
def test_commit_open_verify_against_the_model(harness, curve, n, shapes, npoints):
    C = pu.CURVES[curve]
    r = C.r
    pts = pu.random_points(curve, 40 + n, n + 1)
    pp = im.Params(C.g1, r, pts[:n], pts[n], endo_r=ENDO_R)
    polys = [(im.splitmix_scalars(50 + 7 * i + n, length, r), bound) for i, (length, bound) in enumerate(shapes)]
    if n == 8 and len(polys) == 2:
        polys[1][0][5] = 0                         # a zero coefficient and the largest one
        polys[1][0][6] = r - 1
    points = im.splitmix_scalars(60 + n, npoints, r)
    xi, rr = im.splitmix_scalars(61 + n, 2, r)
    draws = im.splitmix_scalars(62 + n, 64 + 8, r)
    answers = im.splitmix_scalars(63 + n, 16, r)

    # the model
    md = im.Draws(draws)
    plms, evaluation, m_commits, m_blinds = [], [], [], []
    for coeffs, bound in polys:
        commit, blind = im.commitment(pp, coeffs, bound, md)
        m_commits.append(commit), m_blinds.append(blind)
        plms.append((coeffs, bound, blind))
        evaluation.append((commit, im.chunk_evaluations(coeffs, n, points, r), bound))
    after_commit = md.pos
    m_sponge = im.Transcript(answers)
    m_proof = im.proof_eval(pp, plms, points, xi, rr, m_sponge, md)
    after_proof = md.pos

    commits, blinds, proof, (prover_log, verifier_log), counts = run_device(harness, curve, pp, polys, points, xi, rr, draws, answers)
    assert commits == m_commits and blinds == m_blinds
    assert any(c[1] is not None for c in commits) == any(0 <= b and b % n and b <= length for length, b in shapes)
    for key in ("lr", "delta", "z1", "z2", "sg"):
        assert proof[key] == m_proof[key], key
    assert prover_log == m_sponge.log                                  # the sponge calls, their order and their arguments
    assert counts[2:5] == [after_commit, after_proof, after_proof + 2]   # the draws: per chunk + 1, 2 per round + 2, rand_base and sg_rand_base

    # the device's proof in the model's verifier equation, and the sponge calls the shim's verifier made
    v_sponge = im.Transcript(answers)
    batch = {"sponge": v_sponge, "evaluation": [(c, e[1], e[2]) for c, e in zip(commits, evaluation)], "evaluation_points": points, "xi": xi, "r": rr,
             "opening": proof}
    assert im.verify_eval(pp, [batch], im.Draws(draws[after_proof:]))
    assert verifier_log == v_sponge.log
    # the shim's verify_eval accepts it and rejects it with z2, the first L or sg changed
    assert counts[5] == 1
    assert counts[6] == 0 and counts[7] == (0 if n > 1 else 2) and counts[8] == 0
    assert counts[9] == 0                                              # zkhip_device_status
