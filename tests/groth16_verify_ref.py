"""The model the Groth16 verifier (host twin and device) is checked against, and the reference's vectors.

Keys and proofs are built from trapdoor scalars, with no circuit: a key has alpha, beta, gamma, delta and u_0 .. u_l with
abc[j] = u_j G1; a proof for the inputs x has random a and b and c = (a b - alpha beta - s gamma) / delta, s = u_0 + sum x_j u_j.
The value the verifier compares, final_exponentiation(miller(A, B) miller(-acc, gamma) miller(-C, delta)), is then
e(G1, G2)^(a b - s gamma - c delta) for ANY scalars (a, b, c): one exponentiation in pairing_ref, whatever the key's size; the
key's alpha_beta is e(G1, G2)^(alpha beta).  verify() is the equation itself over pairing_ref's big-integer pairing, for the
reference's vectors (tests/golden/ref_groth16_verify_kat.json: bls381_verification, eight bellperson proofs)."""
import json
import os
import random

import pairing_ref as pr
import pyoracle as po

G1, G2 = po.BLS12_381.g1, po.BLS12_381.g2
R, P = pr.R, pr.P
KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_groth16_verify_kat.json")
H = lambda s: int(s, 16)


def load_kat():
    """dict: alpha_beta (12 ints), gamma, delta (G2), ic (12 G1 points), proofs [(A, B, C)] and statements [[11 ints]]"""
    k = json.load(open(KAT))
    q = lambda v: ((H(v[0][0]), H(v[0][1])), (H(v[1][0]), H(v[1][1])))
    p = lambda v: (H(v[0]), H(v[1]))
    return dict(alpha_beta=[H(x) for x in k["alpha_g1_beta_g2"]], gamma=q(k["gamma_g2"]), delta=q(k["delta_g2"]), ic=[p(v) for v in k["ic"]],
                proofs=[(p(f["a"]), q(f["b"]), p(f["c"])) for f in k["proofs"]], statements=[[H(x) for x in st] for st in k["statements"]])


def accumulate(ic, xs):
    """ic[0] + sum x_j ic[j + 1] (None: infinity)"""
    acc = ic[0]
    for x, pt in zip(xs, ic[1:]):
        acc = G1.add(acc, G1.mul(pt, x % R)) if pt is not None else acc
    return acc


def compared_value(gamma, delta, ic, proof, xs):
    """final_exponentiation(miller(A, B) miller(-acc, gamma) miller(-C, delta)) as 12 canonical integers"""
    A, B, C = proof
    neg = lambda pt: None if pt is None else G1.neg(pt)
    return pr.pairing_product([(A, B), (neg(accumulate(ic, xs)), gamma), (neg(C), delta)])


class Key:
    """a key from trapdoor scalars, l inputs"""

    def __init__(self, seed, l, u=None):
        rnd = random.Random(seed)
        self.alpha, self.beta, self.gamma, self.delta = (rnd.randrange(1, R) for _ in range(4))
        self.u = list(u) if u is not None else [rnd.randrange(1, R) for _ in range(l + 1)]
        self.l = len(self.u) - 1
        self.rnd = rnd

    def points(self):
        """(gamma G2, delta G2, [u_j G1])"""
        return G2.mul(G2.gen, self.gamma), G2.mul(G2.gen, self.delta), [G1.mul(G1.gen, u) if u else None for u in self.u]

    def alpha_beta(self):
        return pr.structured_expectation(self.alpha * self.beta)

    def s(self, xs):
        return (self.u[0] + sum(x * u for x, u in zip(xs, self.u[1:]))) % R

    def prove(self, xs):
        """(a, b, c): the scalars of an accepted proof for xs"""
        a, b = self.rnd.randrange(1, R), self.rnd.randrange(1, R)
        return a, b, (a * b - self.alpha * self.beta - self.s(xs) * self.gamma) * pow(self.delta, -1, R) % R

    def exponent(self, abc, xs):
        a, b, c = abc
        return (a * b - self.s(xs) * self.gamma - c * self.delta) % R

    def expected_gt(self, abc, xs):
        """the compared value of the proof (a G1, b G2, c G1), a zero scalar being the point at infinity"""
        return pr.structured_expectation(self.exponent(abc, xs))

    def accepts(self, abc, xs):
        return self.exponent(abc, xs) == self.alpha * self.beta % R
