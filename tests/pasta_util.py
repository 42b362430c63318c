"""The Pasta cycle for the tests: the two Curve objects over pyoracle's generic Fq / Group classes, the curve and type ids of the library,
and their entries in the tables the shared helpers read (util.CURVES / FQ_LIMBS, arith_cases.TYPES), added at import time.

A curve id names a group and ITS scalar field (include/zkhip.h): PALLAS (id 2) has coordinates in F_p and scalars in F_q, VESTA (id 3)
the other way round.  Neither has a G2."""
import arith_cases as ac
import pyoracle as po
import util

P = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001    # Pallas base field = Vesta scalar field
Q = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001    # Pallas scalar field = Vesta base field
PALLAS_ID, VESTA_ID = 2, 3

PALLAS = po.Curve("pallas", P, Q, po.Group(po.Fq(P), 5, (P - 1, 2), Q, "pallas_g1"), None, 5, 32)
VESTA = po.Curve("vesta", Q, P, po.Group(po.Fq(Q), 5, (Q - 1, 2), P, "vesta_g1"), None, 5, 32)
CURVES = {PALLAS_ID: PALLAS, VESTA_ID: VESTA}

# type ids of csrc/hosttest.hip: saturated reference types, lazy 29-bit-limb compute types
SAT_FQ = {PALLAS_ID: 12, VESTA_ID: 14}
SAT_FR = {PALLAS_ID: 13, VESTA_ID: 15}
LAZY_FQ = {PALLAS_ID: 16, VESTA_ID: 17}
LAZY_FR = {PALLAS_ID: 18, VESTA_ID: 19}
# lazy types as arith_cases describes them: modulus, limbs L, saturated words NL, largest spread constant K.  In the coordinate role a
# prime takes 10 limbs (2^290 / p is huge: every spread up to 128 p exists), in the scalar role 9 (2^261 / p ~ 128: 64 p is the last)
LAZY_TYPES = {16: (P, 10, 8, 128), 17: (Q, 10, 8, 128), 18: (Q, 9, 8, 64), 19: (P, 9, 8, 64)}

util.CURVES.update(CURVES)
util.FQ_LIMBS.update({PALLAS_ID: 4, VESTA_ID: 4})
ac.TYPES.update(LAZY_TYPES)


def random_fr(curve, seed, n):
    """n scalars below the curve's r, (n, 4) canonical u64 limbs, from the oracle's SplitMix64"""
    rng = po.SplitMix64(seed * 4 + curve)
    return util.fr_arr([rng.next_mod(CURVES[curve].r) for _ in range(n)])


def random_points(curve, seed, n):
    """n multiples of the generator (python affine points)"""
    rng = po.SplitMix64(seed * 4 + curve + 1000)
    C = CURVES[curve]
    return C.g1.batch_mul_gen([rng.next_mod(C.r - 1) + 1 for _ in range(n)])
