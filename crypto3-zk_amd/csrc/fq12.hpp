// The degree-12 extension of the BLS12-381 base field, as the tower the reference's fq12 value is built from:
//   Fq2  = Fq[u]  / (u^2 + 1)          (fp.hpp)
//   Fq6  = Fq2[v] / (v^3 - (u + 1))
//   Fq12 = Fq6[w] / (w^2 - v)
// over the saturated Montgomery type Fp<BlsFq> (why not the lazy type: DESIGN.md, "Inner pairing products").
//
// Canonical layout of an element (include/zkhip.h, out_gt): 12 Fq values in the order of the reference's constructor
// fq12(fq6(fq2, fq2, fq2), fq6(fq2, fq2, fq2)), c0 before c1 at every level, 6 u64 limbs each -- the member order of the structs
// below, so an Fp12 in memory IS that layout once its Fq values are taken out of Montgomery form.
//
// Everything is __host__ __device__: the Miller kernel (pairing.hip), the final exponentiation on the host and the CPU test
// twin (hosttest.hip) run these very bodies.  Replaces what the reference reaches through crypto3-algebra's
// fields/detail/element/fp6_3over2.hpp and fp12_2over3over2.hpp.
#pragma once
#include "fp.hpp"

// Translation units that call the base-field product out of line (ZK_NOINLINE_MUL: the kernels) call the Fq6 products out of line too:
// a Miller step inlines five of them, and hipcc needs a quarter of an hour to schedule that as one body.
#ifdef ZK_NOINLINE_MUL
#define ZK_FQ6_HD ZK_NOINLINE_HD
#else
#define ZK_FQ6_HD ZK_HD
#endif

namespace zkhip {

// a * (u + 1): the non-residue of the cubic step
template <class P>
ZK_HD Fp2<P> fq2_mul_xi(const Fp2<P> &a) {
    return {a.c0 - a.c1, a.c0 + a.c1};
}
template <class P>
ZK_HD Fp2<P> fq2_conj(const Fp2<P> &a) {
    return {a.c0, fp_neg(a.c1)};
}
template <class P>
ZK_HD Fp2<P> fq2_scale(const Fp2<P> &a, const Fp<P> &k) {
    return {a.c0 * k, a.c1 * k};
}

template <class P>
struct Fp6 {
    Fp2<P> c0, c1, c2;
    ZK_HD static Fp6 zero() { return {Fp2<P>::zero(), Fp2<P>::zero(), Fp2<P>::zero()}; }
    ZK_HD static Fp6 one() { return {Fp2<P>::one(), Fp2<P>::zero(), Fp2<P>::zero()}; }
    ZK_HD bool is_zero() const { return c0.is_zero() && c1.is_zero() && c2.is_zero(); }
    ZK_HD bool operator==(const Fp6 &b) const { return c0 == b.c0 && c1 == b.c1 && c2 == b.c2; }
};
template <class P>
ZK_HD Fp6<P> operator+(const Fp6<P> &a, const Fp6<P> &b) {
    return {a.c0 + b.c0, a.c1 + b.c1, a.c2 + b.c2};
}
template <class P>
ZK_HD Fp6<P> operator-(const Fp6<P> &a, const Fp6<P> &b) {
    return {a.c0 - b.c0, a.c1 - b.c1, a.c2 - b.c2};
}
template <class P>
ZK_HD Fp6<P> fp_neg(const Fp6<P> &a) {
    return {fp_neg(a.c0), fp_neg(a.c1), fp_neg(a.c2)};
}
template <class P>
ZK_HD Fp6<P> fq6_mul_v(const Fp6<P> &a) {  // a * v
    return {fq2_mul_xi(a.c2), a.c0, a.c1};
}
// Karatsuba over the three coefficients: 6 Fq2 products
template <class P>
ZK_FQ6_HD Fp6<P> operator*(const Fp6<P> &a, const Fp6<P> &b) {
    const Fp2<P> v0 = a.c0 * b.c0, v1 = a.c1 * b.c1, v2 = a.c2 * b.c2;
    const Fp2<P> t0 = (a.c1 + a.c2) * (b.c1 + b.c2) - v1 - v2;
    const Fp2<P> t1 = (a.c0 + a.c1) * (b.c0 + b.c1) - v0 - v1;
    const Fp2<P> t2 = (a.c0 + a.c2) * (b.c0 + b.c2) - v0 - v2;
    return {fq2_mul_xi(t0) + v0, t1 + fq2_mul_xi(v2), t2 + v1};
}
// a * (b0 + b1 v): 5 Fq2 products
template <class P>
ZK_FQ6_HD Fp6<P> fq6_mul_by_01(const Fp6<P> &a, const Fp2<P> &b0, const Fp2<P> &b1) {
    const Fp2<P> v0 = a.c0 * b0, v1 = a.c1 * b1;
    const Fp2<P> t0 = (a.c1 + a.c2) * b1 - v1;
    const Fp2<P> t1 = (a.c0 + a.c1) * (b0 + b1) - v0 - v1;
    const Fp2<P> t2 = (a.c0 + a.c2) * b0 - v0;
    return {fq2_mul_xi(t0) + v0, t1, t2 + v1};
}
// a * (b1 v): 3 Fq2 products
template <class P>
ZK_HD Fp6<P> fq6_mul_by_1(const Fp6<P> &a, const Fp2<P> &b1) {
    return {fq2_mul_xi(a.c2 * b1), a.c0 * b1, a.c1 * b1};
}
template <class P>
ZK_HD Fp6<P> fp_inv(const Fp6<P> &a) {
    const Fp2<P> t0 = fp_sqr(a.c0) - fq2_mul_xi(a.c1 * a.c2);
    const Fp2<P> t1 = fq2_mul_xi(fp_sqr(a.c2)) - a.c0 * a.c1;
    const Fp2<P> t2 = fp_sqr(a.c1) - a.c0 * a.c2;
    const Fp2<P> n = fp_inv(a.c0 * t0 + fq2_mul_xi(a.c2 * t1 + a.c1 * t2));
    return {t0 * n, t1 * n, t2 * n};
}

template <class P>
struct Fp12 {
    Fp6<P> c0, c1;
    ZK_HD static Fp12 one() { return {Fp6<P>::one(), Fp6<P>::zero()}; }
    ZK_HD bool operator==(const Fp12 &b) const { return c0 == b.c0 && c1 == b.c1; }
    ZK_HD bool operator!=(const Fp12 &b) const { return !(*this == b); }
};
// Karatsuba: 3 Fq6 products = 54 Fq products
template <class P>
ZK_HD Fp12<P> operator*(const Fp12<P> &a, const Fp12<P> &b) {
    const Fp6<P> aa = a.c0 * b.c0, bb = a.c1 * b.c1;
    const Fp6<P> m = (a.c0 + a.c1) * (b.c0 + b.c1);
    return {aa + fq6_mul_v(bb), m - aa - bb};
}
// complex squaring: 2 Fq6 products = 36 Fq products
template <class P>
ZK_HD Fp12<P> fp_sqr(const Fp12<P> &a) {
    const Fp6<P> ab = a.c0 * a.c1;
    const Fp6<P> t = (a.c0 + a.c1) * (a.c0 + fq6_mul_v(a.c1));
    return {t - ab - fq6_mul_v(ab), ab + ab};
}
// (a + b s)^2 in Fq4 = Fq2[s] / (s^2 - (u + 1)): 3 Fq2 squarings
template <class P>
ZK_HD void fq4_sqr(Fp2<P> &c0, Fp2<P> &c1, const Fp2<P> &a, const Fp2<P> &b) {
    const Fp2<P> t0 = fp_sqr(a), t1 = fp_sqr(b);
    c0 = fq2_mul_xi(t1) + t0;
    c1 = fp_sqr(a + b) - t0 - t1;
}
// a^2 for a in the cyclotomic subgroup (a^(p^6 + 1) = 1 after the easy part of the final exponentiation), by Granger and Scott
// (eprint 2009/565, section 3.2): three Fq4 squarings = 18 Fq products instead of 36.  The same value as fp_sqr there, and only there.
template <class P>
ZK_FQ6_HD Fp12<P> fq12_cyclotomic_sqr(const Fp12<P> &a) {
    Fp2<P> t0, t1, t2, t3, t4, t5;
    fq4_sqr(t0, t1, a.c0.c0, a.c1.c1);
    fq4_sqr(t2, t3, a.c1.c0, a.c0.c2);
    fq4_sqr(t4, t5, a.c0.c1, a.c1.c2);
    const Fp2<P> t5x = fq2_mul_xi(t5);
    Fp12<P> r;
    r.c0.c0 = fp_dbl(t0 - a.c0.c0) + t0;
    r.c0.c1 = fp_dbl(t2 - a.c0.c1) + t2;
    r.c0.c2 = fp_dbl(t4 - a.c0.c2) + t4;
    r.c1.c0 = fp_dbl(t5x + a.c1.c0) + t5x;
    r.c1.c1 = fp_dbl(t1 + a.c1.c1) + t1;
    r.c1.c2 = fp_dbl(t3 + a.c1.c2) + t3;
    return r;
}
// a * (l0 + l1 v + l4 v w), the shape of a line value (pairing.hpp): 13 Fq2 products = 39 Fq products
template <class P>
ZK_HD Fp12<P> fq12_mul_by_014(const Fp12<P> &a, const Fp2<P> &l0, const Fp2<P> &l1, const Fp2<P> &l4) {
    const Fp6<P> aa = fq6_mul_by_01(a.c0, l0, l1);
    const Fp6<P> bb = fq6_mul_by_1(a.c1, l4);
    const Fp6<P> m = fq6_mul_by_01(a.c0 + a.c1, l0, l1 + l4);
    return {aa + fq6_mul_v(bb), m - aa - bb};
}
// w -> -w: the p^6-th power, and the inverse of an element of the cyclotomic subgroup
template <class P>
ZK_HD Fp12<P> fq12_conj(const Fp12<P> &a) {
    return {a.c0, fp_neg(a.c1)};
}
template <class P>
ZK_HD Fp12<P> fp_inv(const Fp12<P> &a) {
    const Fp6<P> n = fp_inv(a.c0 * a.c0 - fq6_mul_v(a.c1 * a.c1));
    return {a.c0 * n, fp_neg(a.c1 * n)};
}

// gamma_i = (u + 1)^(i (p - 1) / 6), i = 1..5, Montgomery form: (sum c_i w^i)^p = sum conj(c_i) gamma_i w^i.
// Values: tests/test_host_pairing.py checks the map against a plain p-th power.
ZK_HD Fp2<BlsFq> fq12_frobenius_gamma(int i) {
    constexpr uint32_t t[5][2][12] = {
        {{0xb319d465u, 0x07089552u, 0xb50a8313u, 0xc6695f92u, 0xd117228fu, 0x97e83cccu, 0xb2dc29eeu, 0xa35baecau, 0x5daace4du, 0x1ce393eau, 0xb0fb66ebu, 0x08f2220fu},
         {0x4ce5d646u, 0xb2f66aadu, 0xfc497cecu, 0x5842a06bu, 0x2599d394u, 0xcf4895d4u, 0x40a8e8d0u, 0xc11b9cbau, 0xe5a0de89u, 0x2e3813cbu, 0x88847fafu, 0x110eefdau}},
        {{0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
         {0x8671f071u, 0xcd03c9e4u, 0x1fcda5d2u, 0x5dab2246u, 0xd3851b95u, 0x587042afu, 0x01bacb9eu, 0x8eb60ebeu, 0x83d050d2u, 0x03f97d6eu, 0x54638741u, 0x18f02065u}},
        {{0x5aa30fdau, 0x7bcfa7a2u, 0x2a927e7cu, 0xdc17dec1u, 0x6b4ebef1u, 0x2f088dd8u, 0xda74d4a7u, 0xd1ca2087u, 0x96cebc1du, 0x2da25966u, 0xbbfd87d2u, 0x0e2b7eedu},
         {0x5aa30fdau, 0x7bcfa7a2u, 0x2a927e7cu, 0xdc17dec1u, 0x6b4ebef1u, 0x2f088dd8u, 0xda74d4a7u, 0xd1ca2087u, 0x96cebc1du, 0x2da25966u, 0xbbfd87d2u, 0x0e2b7eedu}},
        {{0x867545c3u, 0x890dc9e4u, 0x3285a5d5u, 0x2af32253u, 0x309b7e2cu, 0x50880866u, 0x7e881024u, 0xa20d1b8cu, 0xe2db9068u, 0x14e4f04fu, 0x1564853au, 0x14e56d3fu},
         {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}},
        {{0x0dbce43fu, 0x82d83cf5u, 0xdf9d018fu, 0xa2813e53u, 0x3c65e181u, 0xc6f0caa5u, 0x8d50fe95u, 0x7525cf52u, 0xf4798a6bu, 0x4a85ed50u, 0x6cf8eebdu, 0x171da0fdu},
         {0xf242c66cu, 0x3726c30au, 0xd1b6fe70u, 0x7c2ac1aau, 0xba4b14a2u, 0xa04007fbu, 0x66341429u, 0xef517c32u, 0x4ed2226bu, 0x0095ba65u, 0xcc86f7ddu, 0x02e370ecu}},
    };
    Fp2<BlsFq> r;
    for (int k = 0; k < 12; ++k) {
        r.c0.v[k] = t[i - 1][0][k];
        r.c1.v[k] = t[i - 1][1][k];
    }
    return r;
}
// a^p.  The coefficient of w^i sits at c(i & 1).c(i >> 1).
ZK_HD Fp12<BlsFq> fq12_frobenius(const Fp12<BlsFq> &a) {
    Fp12<BlsFq> r;
    r.c0.c0 = fq2_conj(a.c0.c0);
    r.c1.c0 = fq2_conj(a.c1.c0) * fq12_frobenius_gamma(1);
    r.c0.c1 = fq2_conj(a.c0.c1) * fq12_frobenius_gamma(2);
    r.c1.c1 = fq2_conj(a.c1.c1) * fq12_frobenius_gamma(3);
    r.c0.c2 = fq2_conj(a.c0.c2) * fq12_frobenius_gamma(4);
    r.c1.c2 = fq2_conj(a.c1.c2) * fq12_frobenius_gamma(5);
    return r;
}

// canonical u64 limbs (72 per element, as 144 u32) <-> Montgomery form
static_assert(sizeof(Fp12<BlsFq>) == 12 * sizeof(Fp<BlsFq>), "the conversions below walk an Fp12 as its 12 packed Fq values");
template <class P>
ZK_HD Fp12<P> fq12_from_canonical(const uint32_t *p) {
    Fp12<P> r;
    Fp<P> *f = reinterpret_cast<Fp<P> *>(&r);
    for (int k = 0; k < 12; ++k) {
        Fp<P> c;
        for (int i = 0; i < P::NL; ++i) c.v[i] = p[k * P::NL + i];
        f[k] = fp_to_mont(c);
    }
    return r;
}
template <class P>
ZK_HD void fq12_to_canonical(uint32_t *p, const Fp12<P> &a) {
    const Fp<P> *f = reinterpret_cast<const Fp<P> *>(&a);
    for (int k = 0; k < 12; ++k) {
        const Fp<P> c = fp_from_mont(f[k]);
        for (int i = 0; i < P::NL; ++i) p[k * P::NL + i] = c.v[i];
    }
}

typedef Fp6<BlsFq> bls_fq6;
typedef Fp12<BlsFq> bls_fq12;

}  // namespace zkhip
