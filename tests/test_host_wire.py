"""The definition-level model of the wire encoding (tests/wire_cases.py) on the CPU: it accepts the reference's literal vectors
(tests/golden/ref_kat.json, serialisation_test) with the points the reference states, and pyoracle's bls12_381_compress /
bls12_381_decompress -- the complex-method square root with the same arms as the kernel -- agree with it on random subgroup points of both
signs, on infinity and on every constructed case: the arms where x^3 + 4 (1 + u) has no imaginary part, y.c1 at (p -+ 1)/2, small and large
x, and every refusal class.  A disagreement between the oracle and the definition shows here first, without a GPU."""
import json
import os

import pytest

import cport as cp
import pyoracle as po
import wire_cases as wc
from util import pt_from_limbs

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_kat.json")))["serialisation_test"]


def test_model_accepts_the_reference_vectors():
    g1 = (int(KAT["g1"][0], 16), int(KAT["g1"][1], 16))
    g2 = tuple((int(c[0], 16), int(c[1], 16)) for c in KAT["g2"])
    for group, point, enc in ((1, g1, bytes(KAT["g1_bytes"])), (2, g2, bytes(KAT["g2_bytes"]))):
        c = wc.classify(group, enc)
        assert c[0] == "point" and c[1] == point[0] and wc.on_curve(group, c[1])
        wc.check_decoded(group, enc, point)
        G = po.BLS12_381.g1 if group == 1 else po.BLS12_381.g2
        with pytest.raises(AssertionError):  # the other root does not pass
            wc.check_decoded(group, enc, G.neg(point))


@pytest.mark.parametrize("group", [1, 2])
def test_oracle_agrees_with_the_model_on_random_points(group):
    G = po.BLS12_381.g1 if group == 1 else po.BLS12_381.g2
    n = 200
    pts, inf = cp.batch_mul(0, group, cp.random_fr(0, 95, n))
    flags = set()
    for i in range(n):
        pt = pt_from_limbs(0, group, pts[i], inf[i])
        for q in (pt, G.neg(pt)):
            enc = po.bls12_381_compress(group, q)
            c = wc.classify(group, enc)
            assert c[:2] == ("point", q[0])
            flags.add(c[2])
            got = po.bls12_381_decompress(group, enc)
            wc.check_decoded(group, enc, got)
            assert got == q and po.bls12_381_compress(group, got) == enc
    assert flags == {True, False}
    assert po.bls12_381_compress(group, None) == wc.INFINITY[group]
    wc.check_decoded(group, wc.INFINITY[group], po.bls12_381_decompress(group, wc.INFINITY[group]))


@pytest.mark.parametrize("group", [1, 2])
def test_oracle_agrees_with_the_model_on_every_constructed_case(group):
    for name, encs in wc.valid_classes(group).items():
        for enc in encs:
            got = po.bls12_381_decompress(group, enc)
            wc.check_decoded(group, enc, got)
            assert po.bls12_381_compress(group, got) == enc, name
    encs, _ = wc.mixed_batch(group)
    for enc in encs:
        wc.check_decoded(group, enc, po.bls12_381_decompress(group, enc))
    for enc, reason in wc.refusals(group):
        with pytest.raises(ValueError):
            po.bls12_381_decompress(group, enc)


def test_constructed_cases_are_what_they_claim():
    """the shapes of y in the special arms, stated from the definition: y^2 = a with a in Fq"""
    square, non_square = wc.g2_imaginary_part_vanishes()
    assert len(square) == len(non_square) == 2
    for x in square + non_square:
        y = po.bls12_381_decompress(2, wc.encode(2, x, False))[1]
        assert (y[1] == 0) == (x in square) and (y[0] == 0) == (x in non_square)
    x, y = wc.g2_boundary_y()
    assert po.bls12_381_decompress(2, wc.encode(2, x, False)) == (x, y)
    assert po.bls12_381_decompress(2, wc.encode(2, x, True)) == (x, wc.f2_neg(y))
    first, second = wc.g2_generic_by_arm(3)
    assert len(first) == len(second) == 3 and not set(first) & set(second)
    assert po.bls12_381_decompress(1, wc.encode(1, 0, False)) == (0, 2)
    assert po.bls12_381_decompress(1, wc.encode(1, 0, True)) == (0, wc.P - 2)


def test_model_refuses_what_it_should():
    """check_decoded is not vacuous: a wrong x, a y off the curve and the wrong root each fail"""
    G = po.BLS12_381.g2
    pt = G.mul(G.gen, 5)
    enc = po.bls12_381_compress(2, pt)
    wc.check_decoded(2, enc, pt)
    for wrong in (G.neg(pt), (G.mul(G.gen, 6)[0], pt[1]), (pt[0], (pt[1][1], pt[1][0])), None):
        with pytest.raises(AssertionError):
            wc.check_decoded(2, enc, wrong)
    with pytest.raises(AssertionError):
        wc.check_decoded(2, wc.INFINITY[2], pt)
