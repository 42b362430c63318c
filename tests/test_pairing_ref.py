"""The big-integer pairing model (tests/pairing_ref.py) against the reference's own vectors of the inner pairing product commitments
(tests/golden/ref_ipp2_kat.json: bls381_commitment_test, bellperson-generated), and its algebraic properties.  The model is what the
host and device pairing code is checked against; this file is what pins the model -- and with it the power of the Miller value that
`final_exponentiation` means."""
import json
import os
import random

import pytest

import pairing_ref as pr
import pyoracle as po

G1, G2 = po.BLS12_381.g1, po.BLS12_381.g2
KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_ipp2_kat.json")
H = lambda s: int(s, 16)


def load_kat():
    """(a, b, v1, v2, w1, w2, expected): the fixture's points, the keys g^(u^i), g^(v^i), i < 10, and the four expected values"""
    k = json.load(open(KAT))
    n, u, v = k["n"], H(k["u"]), H(k["v"])
    a = [(H(x), H(y)) for x, y in k["a"]]
    b = [((H(x[0]), H(x[1])), (H(y[0]), H(y[1]))) for x, y in k["b"]]
    pu, pv = [pow(u, i, pr.R) for i in range(n)], [pow(v, i, pr.R) for i in range(n)]
    keys = [[G.mul(G.gen, e) for e in pw] for G, pw in ((G2, pu), (G2, pv), (G1, pu), (G1, pv))]
    exp = {name: [H(x) for x in k[name]] for name in ("single_first", "single_second", "pair_first", "pair_second")}
    return a, b, keys[0], keys[1], keys[2], keys[3], exp


@pytest.fixture(scope="module")
def kat():
    return load_kat()


def test_fixture_points_are_on_the_curves(kat):
    a, b = kat[0], kat[1]
    assert all(G1.on_curve(p) for p in a) and all(G2.on_curve(q) for q in b)


def test_model_reproduces_single(kat):
    a, _, v1, v2, _, _, exp = kat
    assert pr.pairing_product(list(zip(a, v1))) == exp["single_first"]
    assert pr.pairing_product(list(zip(a, v2))) == exp["single_second"]


def test_model_reproduces_pair(kat):
    a, b, v1, v2, w1, w2, exp = kat
    assert pr.pairing_product(list(zip(a, v1)) + list(zip(w1, b))) == exp["pair_first"]
    assert pr.pairing_product(list(zip(a, v2)) + list(zip(w2, b))) == exp["pair_second"]


def test_the_plain_exponent_is_not_the_references(kat):
    """(p^12 - 1)/r gives another value (its cube is the reference's): the multiple 3 is part of the convention."""
    a, _, v1, _, _, _, exp = kat
    plain = pr.pairing_product(list(zip(a, v1)), pr.PLAIN_EXP)
    assert plain != exp["single_first"]
    assert pr.to_canonical(pr.f12_pow(pr.from_canonical(plain), 3)) == exp["single_first"]


def test_bilinearity_and_infinity():
    random.seed(5)
    x, y = random.randrange(1, pr.R), random.randrange(1, pr.R)
    lhs = pr.pairing_product([(G1.mul(G1.gen, x), G2.mul(G2.gen, y))])
    assert lhs == pr.structured_expectation(x * y)
    assert lhs != pr.to_canonical(pr.ONE)
    assert pr.pairing_product([(G1.gen, None)]) == pr.to_canonical(pr.ONE)
    assert pr.pairing_product([(None, G2.gen)]) == pr.to_canonical(pr.ONE)
    # the value has order r
    assert pr.f12_pow(pr.from_canonical(lhs), pr.R) == pr.ONE
