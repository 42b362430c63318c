// The ate pairing of BLS12-381: one Miller loop per (G1, G2) pair and the final exponentiation, over fq12.hpp.
//
//   miller_loop(fs, P, Q)      f_{|x|, Q}(P), conjugated because x = -0xd201000000010000 is negative.  The running value f lives
//                              behind `fs` (load / store of a whole Fp12): registers on the host, an LDS slot per lane in the
//                              Miller kernel (pairing.hip), which keeps only the running twist point and the line in registers.
//   prepare_lines(out, Q)      the 68 line triples of a FIXED Q (a verification key's gamma, delta), computed once per key
//   miller_loop3(fs, ...)      the product of three Miller values, the shape of a Groth16 verification (groth16_verify.hpp): one walked
//                              pair and two pairs over prepared lines, with one squaring of f per step for all three
//   final_exponentiation(f)    f^(3 (p^12 - 1) / r): the x-chain of Hayashida, Hayasaka and Teruya (eprint 2020/875) computes the
//                              hard part to the fixed multiple 3, and that is the power the reference's values are (its vectors
//                              come from bellperson; tests/test_pairing_ref.py settles it against (p^12 - 1)/r and its triple).
//
// The twist is E': y^2 = x^3 + 4 (u + 1), a point (x', y') of it standing for (x' / w^2, y' / w^3) on E(Fq12).  The running point
// T is Jacobian.  A line through T with slope lambda, at the affine G1 point (xP, yP) and scaled by w^3 and by factors of Fq2 -- all
// of a proper subfield, which the final exponentiation removes -- is
//      (lambda x_T - y_T)  -  lambda xP w^2  +  yP w^3        =  l0 + l1 v + l4 v w   (fq12_mul_by_014).
// Inputs are points of the order-r subgroups (the bases objects hold nothing else), so T never meets +-Q or a 2-torsion point
// inside the loop; a pair with a point at infinity is answered before the loop (its value is one).
//
// Replaces algebra::pair<curve_type> / algebra::final_exponentiation<curve_type> of crypto3-algebra as the reference's
// commitments/polynomial/kzg_ipp2.hpp:216-283 uses them.
#pragma once
#include "fq12.hpp"

namespace zkhip {
namespace pairing {

static constexpr uint64_t BLS_X_ABS = 0xd201000000010000ull;

typedef bls_fq Fq;
typedef bls_fq2 Fq2;
typedef bls_fq12 Fq12;

struct TwistPoint {  // Jacobian: (X / Z^2, Y / Z^3)
    Fq2 x, y, z;
};
struct Line {
    Fq2 l0, l1, l4;
};

// T <- 2T and the tangent at (the old) T.  dbl-2009-l: 6 squarings + 5 products in Fq2, 4 products in Fq for the G1 point.
ZK_HD Line doubling_step(TwistPoint &t, const Fq &xp, const Fq &yp) {
    const Fq2 a = fp_sqr(t.x), b = fp_sqr(t.y), c = fp_sqr(b), zz = fp_sqr(t.z);
    Fq2 d = fp_sqr(t.x + b) - a - c;
    d = fp_dbl(d);
    const Fq2 e = fp_dbl(a) + a;  // 3 X^2; the slope is e / Z3
    const Fq2 z3 = fp_dbl(t.y * t.z);
    Line l;
    l.l0 = e * t.x - fp_dbl(b);                 // (3 X^3 - 2 Y^2)          = Z3 Z^2 (lambda x_T - y_T)
    l.l1 = fp_neg(fq2_scale(e * zz, xp));       // -3 X^2 Z^2 xP            = Z3 Z^2 (-lambda xP)
    l.l4 = fq2_scale(z3 * zz, yp);              //  Z3 Z^2 yP
    const Fq2 x3 = fp_sqr(e) - fp_dbl(d);
    const Fq2 c8 = fp_dbl(fp_dbl(fp_dbl(c)));
    t.y = e * (d - x3) - c8;
    t.x = x3;
    t.z = z3;
    return l;
}

// T <- T + Q (Q affine) and the chord through them.  madd: 3 squarings + 9 products in Fq2, 4 products in Fq.
ZK_HD Line addition_step(TwistPoint &t, const Fq2 &xq, const Fq2 &yq, const Fq &xp, const Fq &yp) {
    const Fq2 zz = fp_sqr(t.z);
    const Fq2 h = xq * zz - t.x;
    const Fq2 r = yq * (t.z * zz) - t.y;  // the slope is r / Z3
    const Fq2 hh = fp_sqr(h), hhh = h * hh, v = t.x * hh;
    const Fq2 z3 = t.z * h;
    Line l;
    l.l0 = r * xq - z3 * yq;                    // Z3 (lambda x_Q - y_Q)
    l.l1 = fp_neg(fq2_scale(r, xp));
    l.l4 = fq2_scale(z3, yp);
    const Fq2 x3 = fp_sqr(r) - hhh - fp_dbl(v);
    t.y = r * (v - x3) - t.y * hhh;
    t.x = x3;
    t.z = z3;
    return l;
}

// an Fp12 behind load() / store(): the host's (and the product kernels') plain value
struct RegStore {
    Fq12 f;
    ZK_HD Fq12 load() const { return f; }
    ZK_HD void store(const Fq12 &a) { f = a; }
};

// fs <- the Miller value of (P, Q); both points affine, Montgomery form, not at infinity
template <class FStore>
ZK_HD void miller_loop(FStore &fs, const Fq &xp, const Fq &yp, const Fq2 &xq, const Fq2 &yq) {
    TwistPoint t = {xq, yq, Fq2::one()};
    fs.store(Fq12::one());
    for (int i = 62; i >= 0; --i) {  // below the top bit of |x|
        const Line l = doubling_step(t, xp, yp);
        fs.store(fq12_mul_by_014(fp_sqr(fs.load()), l.l0, l.l1, l.l4));
        if ((BLS_X_ABS >> i) & 1) {
            const Line m = addition_step(t, xq, yq, xp, yp);
            fs.store(fq12_mul_by_014(fs.load(), m.l0, m.l1, m.l4));
        }
    }
    fs.store(fq12_conj(fs.load()));
}

// The lines of a FIXED G2 point (a verification key's gamma and delta), walked once when the key is made: per step l0 and the factors
// of xP and of yP in l1 and l4, so a Miller loop over such a point keeps no twist point and only scales by its G1 point.
static constexpr int PREPARED_LINES = 63 + 5;  // one doubling per bit below the top of |x|, one addition per set bit among them
ZK_HD void prepare_lines(Line *out, const Fq2 &xq, const Fq2 &yq) {
    TwistPoint t = {xq, yq, Fq2::one()};
    const Fq one = Fq::one();
    for (int i = 62; i >= 0; --i) {
        *out++ = doubling_step(t, one, one);
        if ((BLS_X_ABS >> i) & 1) *out++ = addition_step(t, xq, yq, one, one);
    }
}

// The pairs of miller_loop3.  A pair that is not `live` (one of its points is at infinity) contributes one.
struct WalkedPair {  // a G1 point and a G2 point whose multiples the loop walks
    bool live;
    Fq xp, yp;
    Fq2 xq, yq;
};
struct PreparedPair {  // a G1 point and the prepared lines of a fixed G2 point
    bool live;
    Fq xp, yp;
    const Line *lines;
};

// fs <- miller(P0, Q0) miller(P1, Q1) miller(P2, Q2), the shape of a Groth16 verification (Q1, Q2: the key's gamma and delta): one
// squaring of f per step serves all three pairs, and only Q0's multiples are computed.
template <class FStore>
ZK_HD void miller_loop3(FStore &fs, const WalkedPair &w, const PreparedPair &p1, const PreparedPair &p2) {
    TwistPoint t = {w.xq, w.yq, Fq2::one()};
    const Line *n1 = p1.lines, *n2 = p2.lines;
    const auto prepared = [&fs](const PreparedPair &p, const Line *&next) {
        const Line &l = *next++;
        if (p.live) fs.store(fq12_mul_by_014(fs.load(), l.l0, fq2_scale(l.l1, p.xp), fq2_scale(l.l4, p.yp)));
    };
    fs.store(Fq12::one());
    for (int i = 62; i >= 0; --i) {
        fs.store(fp_sqr(fs.load()));
        if (w.live) {
            const Line l = doubling_step(t, w.xp, w.yp);
            fs.store(fq12_mul_by_014(fs.load(), l.l0, l.l1, l.l4));
        }
        prepared(p1, n1);
        prepared(p2, n2);
        if ((BLS_X_ABS >> i) & 1) {
            if (w.live) {
                const Line m = addition_step(t, w.xq, w.yq, w.xp, w.yp);
                fs.store(fq12_mul_by_014(fs.load(), m.l0, m.l1, m.l4));
            }
            prepared(p1, n1);
            prepared(p2, n2);
        }
    }
    fs.store(fq12_conj(fs.load()));
}

// a^x for a in the cyclotomic subgroup (where the inverse is the conjugate, and the squaring is Granger and Scott's)
ZK_HD Fq12 exp_by_x(const Fq12 &a) {
    Fq12 r = a;
    for (int i = 62; i >= 0; --i) {
        r = fq12_cyclotomic_sqr(r);
        if ((BLS_X_ABS >> i) & 1) r = r * a;
    }
    return fq12_conj(r);
}

ZK_HD Fq12 final_exponentiation(const Fq12 &f) {
    // easy part: f^((p^6 - 1)(p^2 + 1))
    Fq12 t2 = fq12_conj(f) * fp_inv(f);
    t2 = fq12_frobenius(fq12_frobenius(t2)) * t2;
    // hard part, to the multiple 3: t2^(3 (p^4 - p^2 + 1) / r)
    Fq12 t1 = fq12_conj(fp_sqr(t2));
    Fq12 t3 = exp_by_x(t2);
    Fq12 t4 = fp_sqr(t3);
    Fq12 t5 = t1 * t3;
    t1 = exp_by_x(t5);
    const Fq12 t0 = exp_by_x(t1);
    Fq12 t6 = exp_by_x(t0) * t4;
    t4 = exp_by_x(t6);
    t5 = fq12_conj(t5);
    t4 = t4 * t5 * t2;
    t5 = fq12_conj(t2);
    t1 = t1 * t2;
    t1 = fq12_frobenius(fq12_frobenius(fq12_frobenius(t1)));
    t6 = fq12_frobenius(t6 * t5);
    t3 = fq12_frobenius(fq12_frobenius(t3 * t0));
    return t3 * t1 * t6 * t4;
}

}  // namespace pairing
}  // namespace zkhip
