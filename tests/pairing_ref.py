"""A big-integer BLS12-381 ate pairing: the model the host and device pairing code is checked against.

Independent of csrc/fq12.hpp and csrc/pairing.hpp on purpose: Fq12 is the flat extension
Fq2[w]/(w^6 - (u + 1)) with schoolbook products (no tower), the Miller loop walks the twist in affine
coordinates with one Fq2 inversion per step, and the final exponentiation is one `pow`.  The exponent is
3 (p^12 - 1)/r: the reference's vectors (bellperson's) are that power -- the x-chain formulas for the hard
part compute it to the fixed multiple 3 -- and not the plain one (tests/test_pairing_ref.py holds both facts).  Only the field and curve arithmetic of oracle/pyoracle.py is shared.

Canonical order of an Fq12 value (the reference's fq12(fq6(fq2, fq2, fq2), fq6(fq2, fq2, fq2)), with
v = w^2): Fq2 coefficients of w^0, w^2, w^4, w^1, w^3, w^5, each as (c0, c1) -- 12 integers.
"""
import pyoracle as po

C = po.BLS12_381
P = C.p
R = C.r
F2 = C.g2.F
X_ABS = 0xD201000000010000          # |x|; x itself is negative
XI = (1, 1)                          # w^6 = u + 1
PLAIN_EXP = (P ** 12 - 1) // R
FINAL_EXP = 3 * PLAIN_EXP
ONE = ((1, 0),) + ((0, 0),) * 5
TOWER_ORDER = (0, 2, 4, 1, 3, 5)    # canonical slot k holds the coefficient of w^TOWER_ORDER[k]


def f12_mul(a, b):
    acc = [(0, 0)] * 11
    for i, x in enumerate(a):
        if x == (0, 0):
            continue
        for j, y in enumerate(b):
            acc[i + j] = F2.add(acc[i + j], F2.mul(x, y))
    return tuple(F2.add(acc[k], F2.mul(acc[k + 6], XI)) if k < 5 else acc[k] for k in range(6))


def f12_pow(a, e):
    r = ONE
    for bit in bin(e)[2:]:
        r = f12_mul(r, r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def f12_conj(a):
    """w -> -w (the p^6 Frobenius)."""
    return tuple(c if k % 2 == 0 else F2.neg(c) for k, c in enumerate(a))


def f12_frobenius(a, k=1):
    return f12_pow(a, P ** k)


def f12_inv(a):
    return f12_pow(a, P ** 12 - 2)


def to_canonical(a):
    """12 integers in the canonical order."""
    out = []
    for k in TOWER_ORDER:
        out += [a[k][0] % P, a[k][1] % P]
    return out


def from_canonical(v):
    a = [None] * 6
    for slot, k in enumerate(TOWER_ORDER):
        a[k] = (v[2 * slot] % P, v[2 * slot + 1] % P)
    return tuple(a)


def _line(T, lam, Pt):
    """The line through the twist point T with slope lam, at the G1 point Pt, scaled by w^3 (a factor of
    a proper subfield, which the final exponentiation removes): (lam x_T - y_T) - lam x_P w^2 + y_P w^3."""
    xp, yp = Pt
    c0 = F2.sub(F2.mul(lam, T[0]), T[1])
    c2 = F2.neg((lam[0] * xp % P, lam[1] * xp % P))
    return (c0, (0, 0), c2, (yp % P, 0), (0, 0), (0, 0))


def miller_loop(Pt, Q):
    """f_{|x|, Q}(P), conjugated because x is negative.  None is the point at infinity: the value is one."""
    if Pt is None or Q is None:
        return ONE
    f = ONE
    T = Q
    for bit in bin(X_ABS)[3:]:
        lam = F2.mul(F2.mul((3, 0), F2.sqr(T[0])), F2.inv(F2.add(T[1], T[1])))
        f = f12_mul(f12_mul(f, f), _line(T, lam, Pt))
        x3 = F2.sub(F2.sqr(lam), F2.add(T[0], T[0]))
        T = (x3, F2.sub(F2.mul(lam, F2.sub(T[0], x3)), T[1]))
        if bit == "1":
            lam = F2.mul(F2.sub(T[1], Q[1]), F2.inv(F2.sub(T[0], Q[0])))
            f = f12_mul(f, _line(T, lam, Pt))
            x3 = F2.sub(F2.sub(F2.sqr(lam), T[0]), Q[0])
            T = (x3, F2.sub(F2.mul(lam, F2.sub(T[0], x3)), T[1]))
    return f12_conj(f)


def final_exponentiation(f, exponent=FINAL_EXP):
    return f12_pow(f, exponent)


def pairing_product(pairs, exponent=FINAL_EXP):
    """final_exponentiation(prod miller(P_i, Q_i)) as 12 canonical integers."""
    f = ONE
    for Pt, Q in pairs:
        f = f12_mul(f, miller_loop(Pt, Q))
    return to_canonical(final_exponentiation(f, exponent))


_E_GEN = None


def structured_expectation(k):
    """e(G1, G2)^k as 12 canonical integers: what prod e(a_i G1, b_i G2) is for k = sum a_i b_i mod r."""
    global _E_GEN
    if _E_GEN is None:
        _E_GEN = final_exponentiation(miller_loop(C.g1.gen, C.g2.gen))
    return to_canonical(f12_pow(_E_GEN, k % R))
