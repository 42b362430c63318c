"""The Python model of kimchi_pedersen (tests/ipa_model.py) against itself, without a GPU: a proof it makes satisfies the verifier's
equation it restates, a tampered one does not, and b_poly is the polynomial whose coefficients b_poly_coefficents lists.  The GPU tests
(test_gpu_ipa.py, test_gpu_ipa_shim.py) hold the library against this model."""
import pytest

import ipa_model as im
import pasta_util as pu
import pyoracle as po


def make_params(curve, n, seed=1):
    C = pu.CURVES[curve]
    pts = pu.random_points(curve, seed, n + 1)
    return im.Params(C.g1, C.r, pts[:n], pts[n], endo_r=5)


def open_and_check(curve, n, polys, points, seed=3):
    """commit to `polys` = [(coefficients, bound)], open at `points`, build the verifier's batch -> (params, batch, proof)"""
    pp = make_params(curve, n)
    r = pp.r
    draws = im.Draws(im.splitmix_scalars(seed, 4 * len(polys) * 8 + 2 * 12 + 8, r))
    answers = im.splitmix_scalars(seed + 100, 16, r)
    plms, evaluation = [], []
    for coeffs, bound in polys:
        commit, blind = im.commitment(pp, coeffs, bound, draws)
        plms.append((coeffs, bound, blind))
        evaluation.append((commit, im.chunk_evaluations(coeffs, n, points, r), bound))
    xi, rr = im.splitmix_scalars(seed + 200, 2, r)
    proof = im.proof_eval(pp, plms, points, xi, rr, im.Transcript(answers), draws)
    batch = {"sponge": im.Transcript(answers), "evaluation": evaluation, "evaluation_points": points, "xi": xi, "r": rr, "opening": proof}
    return pp, batch, proof


def rand_poly(curve, seed, n):
    return im.splitmix_scalars(seed * 7 + curve, n, pu.CURVES[curve].r)


@pytest.mark.parametrize("n", [1, 2, 5, 8, 64])
def test_model_proof_satisfies_the_verifier_equation(n):
    curve = pu.PALLAS_ID if n != 5 else pu.VESTA_ID
    r = pu.CURVES[curve].r
    points = im.splitmix_scalars(11, 2, r)
    # one polynomial with a degree bound that ends inside the last of its chunks (so it has a shifted part whenever n > 1), one without a bound
    length = 2 * n + max(1, n // 2) if n > 1 else 3
    polys = [(rand_poly(curve, 1, length), length), (rand_poly(curve, 2, n), -1)]
    pp, batch, proof = open_and_check(curve, n, polys, points)
    assert len(proof["lr"]) == max(0, (n - 1).bit_length())
    assert (batch["evaluation"][0][0][1] is not None) == (n > 1)
    assert im.verify_eval(pp, [batch], im.Draws(im.splitmix_scalars(9, 2, r)))
    # the prover's and the verifier's sponge saw the same calls after the first absorb (whose argument they compute differently)
    assert len(batch["sponge"].log) == 2 + 3 * len(proof["lr"]) + 2


@pytest.mark.parametrize("field", ["z1", "z2"])
def test_model_rejects_a_changed_proof(field):
    curve, n = pu.PALLAS_ID, 8
    r = pu.CURVES[curve].r
    pp, batch, proof = open_and_check(curve, n, [(rand_poly(curve, 3, 11), 11)], im.splitmix_scalars(12, 1, r))
    proof[field] = (proof[field] + 1) % r
    assert not im.verify_eval(pp, [batch], im.Draws(im.splitmix_scalars(9, 2, r)))


def test_two_batches_share_one_equation():
    curve, n = pu.VESTA_ID, 4
    r = pu.CURVES[curve].r
    pp, b1, _ = open_and_check(curve, n, [(rand_poly(curve, 4, 4), -1)], im.splitmix_scalars(13, 1, r), seed=5)
    _, b2, _ = open_and_check(curve, n, [(rand_poly(curve, 5, 7), 7)], im.splitmix_scalars(14, 2, r), seed=6)
    assert im.verify_eval(pp, [b1, b2], im.Draws(im.splitmix_scalars(10, 2, r)))


@pytest.mark.parametrize("rounds", [0, 1, 5])
def test_b_poly_is_the_polynomial_of_its_coefficients(rounds):
    r = pu.PALLAS.r
    chals = im.splitmix_scalars(21, rounds, r)
    s = im.b_poly_coefficients(chals, r)
    assert len(s) == 1 << rounds
    for x in [0, 1] + im.splitmix_scalars(22, 2, r):
        assert im.b_poly(chals, x, r) == im.poly_eval(s, x, r) if rounds else s == [1]
    # the closed form the device kernel computes: the product of the challenges selected by the bits of i
    for i, v in enumerate(s):
        e = 1
        for t in range(rounds):
            if (i >> t) & 1:
                e = e * chals[rounds - 1 - t] % r
        assert v == e
