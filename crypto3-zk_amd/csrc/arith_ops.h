// TEST-ONLY op tables over the field / curve code (never included by the product path).  One source for the two builds that
// run them: csrc/hosttest.hip (the C++ bodies on the CPU, libzkhip_hosttest.so) and tests/cpp/arithdev.hip (the code the
// kernels run: inline-asm products, -O3, gfx950).  Everything here is __host__ __device__ and writes its results with plain
// stores.  (Named .h rather than .hpp: it is not part of what the kernels are built from.)
#pragma once
#include "curve.hpp"
#include "fu_safegcd.hpp"

namespace zkhip {
namespace arith {

// ---- raw Fu limbs --------------------------------------------------------------------------------------------------------
// op: 0 fu_mul(a, b), 1 fu_sqr(a), 2 fu_mul2(a, b, c, d), 3 fu_add(a, b), 4 fu_cond_sub_p(a), 5 fu_canon(a),
//     6 fu_is_zero_lt2p(a) (out[0] = 0 / 1), 7 fu_inv(a), 8 fu_inv_gcd(a), 9 fu_pack(a) (NL saturated words out),
//     10 fu_unpack(first NL words of a), 20 + j: fu_sub<2^j>(a, b) for j = 1 .. 7 where field_consts.hpp defines 2^j p.
//     The element layer of the scalar-field kernels: 30 fu_mulm(a, b), 31 fu_addm(a, b), 32 fu_from_mont(a), 33 fu_pow(a, e),
//     34 fu_pow_onto(c, a, e) -- e the 64-bit integer in b's first two words -- and, where NL = 8, 35 fu_store8 / fu_load8 of a through
//     element 1 of a 16-byte aligned three-element buffer (out: the element read back, or all-ones limbs if a neighbour changed) and
//     36 a^e for the 256-bit e in b's first 8 words: fu_pow_onto word by word from the top, fu_pow(r, 2^32) between.
//     Where L = 9 (the scalar fields' compute form): 37 fu_reduce_small(a), the product-free reduction of an NTT's last store.
// L u32 in per operand and L u32 out per case, exactly as a kernel holds them (no normalisation on the way in).
template <class U>
struct MaxSpread {  // largest K with a spread constant: every lazy type has 128 except the 255-bit scalar fields
    static constexpr int K = 128;
};
template <>
struct MaxSpread<BlsFrU> {
    static constexpr int K = 64;
};
template <>
struct MaxSpread<PallasFrU> {  // the Pasta primes in the scalar role: 2^261 / p ~ 128, as tight as BLS12-381's r
    static constexpr int K = 64;
};
template <>
struct MaxSpread<VestaFrU> {
    static constexpr int K = 64;
};

template <class U>
ZK_HD bool fu_raw_valid(int op) {
    if ((op >= 0 && op <= 10) || (op >= 30 && op <= 34)) return true;
    if (op == 35 || op == 36) return U::NL == 8;
    if (op == 37) return U::L == 9;
    return op >= 21 && op <= 27 && (1 << (op - 20)) <= MaxSpread<U>::K;
}

template <int K, class U>
ZK_HD Fu<U> sub_k(const Fu<U> &a, const Fu<U> &b) {
    if constexpr (K <= MaxSpread<U>::K) return fu_sub<K>(a, b);
    return Fu<U>::zero();
}

// ops 35 and 36, which only the 8-word types have
template <class U>
ZK_HD Fu<U> fu_raw_words8(int op, const Fu<U> &x, const uint32_t *b) {
    Fu<U> r = Fu<U>::zero();
    if constexpr (U::NL == 8) {
        if (op == 35) {
            alignas(16) uint32_t buf[24];
            for (int i = 0; i < 24; ++i) buf[i] = 0xA5A5A5A5u + i;
            fu_store8<U>(buf, 1, x);
            r = fu_load8<U>(buf, 1);
            bool kept = true;
            for (int i = 0; i < 8; ++i) kept = kept && buf[i] == 0xA5A5A5A5u + i && buf[16 + i] == 0xA5A5A5A5u + 16 + i;
            if (!kept)  // no element reads back as this
                for (int i = 0; i < U::L; ++i) r.v[i] = 0xFFFFFFFFu;
        } else {
            r = Fu<U>::one();
            for (int w = 7; w >= 0; --w) r = fu_pow_onto(fu_pow(r, (uint64_t)1 << 32), x, b[w]);
        }
    }
    return r;
}

// op 37, which only the 9-limb types have
template <class U>
ZK_HD Fu<U> fu_raw_limbs9(const Fu<U> &x) {
    if constexpr (U::L == 9) return fu_reduce_small(x);
    return Fu<U>::zero();
}

template <class U>
ZK_HD void fu_raw_one(int op, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out) {
    constexpr int L = U::L;
    Fu<U> x, y, z, w, r = Fu<U>::zero();
    for (int i = 0; i < L; ++i) x.v[i] = a[i], y.v[i] = b[i], z.v[i] = c[i], w.v[i] = d[i];
    switch (op) {
        case 0: r = fu_mul(x, y); break;
        case 1: r = fu_sqr(x); break;
        case 2: r = fu_mul2(x, y, z, w); break;
        case 3: r = fu_add(x, y); break;
        case 4: r = fu_cond_sub_p(x); break;
        case 5: r = fu_canon(x); break;
        case 6: r.v[0] = fu_is_zero_lt2p(x) ? 1u : 0u; break;
        case 7: r = fu_inv(x); break;
        case 8: r = fu_inv_gcd(x); break;
        case 9: {
            uint32_t s[U::NL];
            fu_pack<U>(s, x);
            for (int i = 0; i < U::NL; ++i) r.v[i] = s[i];
            break;
        }
        case 10: r = fu_unpack<U>(a); break;
        case 30: r = fu_mulm(x, y); break;
        case 31: r = fu_addm(x, y); break;
        case 32: r = fu_from_mont(x); break;
        case 33: r = fu_pow(x, (uint64_t)b[0] | ((uint64_t)b[1] << 32)); break;
        case 34: r = fu_pow_onto(z, x, (uint64_t)b[0] | ((uint64_t)b[1] << 32)); break;
        case 35:
        case 36: r = fu_raw_words8(op, x, b); break;
        case 37: r = fu_raw_limbs9(x); break;
        case 21: r = sub_k<2>(x, y); break;
        case 22: r = sub_k<4>(x, y); break;
        case 23: r = sub_k<8>(x, y); break;
        case 24: r = sub_k<16>(x, y); break;
        case 25: r = sub_k<32>(x, y); break;
        case 26: r = sub_k<64>(x, y); break;
        case 27: r = sub_k<128>(x, y); break;
        default: break;
    }
    for (int i = 0; i < L; ++i) out[i] = r.v[i];
}

// ---- FieldOps on canonical values (zkt_field_op / zkd_field_op) ------------------------------------------------------------
// op: 0 mul, 1 add, 2 sub<K1>, 3 inv(a), 4 sqr(a), 5 neg(a) = sub<K1>(0, a), 6 dbl(a), 7 sub<K2>, 9 fu_sqr(a + b),
//     10 mul_sub<K2>(a, a + b, sub<K1>(0, b), b) = a (a + b) + b^2  (one shared reduction for the lazy base field),
//     8 bound stress: mul(sub<K2>(mul(a,b), X), sub<K2>(sqr(b), X)),  X = sub<K1>(sqr(a), ab + 2 b^2)
//       -- the deepest lazy chain of the group law, with every operand at its contract bound
//     11 the safegcd inverse the grand products take once per call (fu_safegcd.hpp); the saturated types have none of their own
// the dedicated Montgomery square the kernels inline (FieldOps::sqr routes to the out-of-line product in the host shim's build)
template <class F>
ZK_HD F sqr_direct(const F &x) { return FieldOps<F>::sqr(x); }
template <class U>
ZK_HD Fu<U> sqr_direct(const Fu<U> &x) { return fu_sqr(x); }

template <class F>
ZK_HD F inv_gcd(const F &x) { return FieldOps<F>::inv(x); }
template <class U>
ZK_HD Fu<U> inv_gcd(const Fu<U> &x) { return fu_inv_gcd(fu_canon(x)); }

ZK_HD bool field_op_valid(int op) { return op >= 0 && op <= 11; }

template <class F>
ZK_HD void field_op(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    typedef FieldOps<F> O;
    F x = O::from_canonical(a), y = b ? O::from_canonical(b) : F::zero(), r = F::zero();
    switch (op) {
        case 0: r = O::mul(x, y); break;
        case 1: r = O::add(x, y); break;
        case 2: r = O::template sub<O::K1>(x, y); break;
        case 3: r = O::inv(x); break;
        case 4: r = O::sqr(x); break;
        case 5: r = O::template sub<O::K1>(F::zero(), x); break;
        case 6: r = O::add(x, x); break;
        case 7: r = O::template sub<O::K2>(x, y); break;
        case 9: r = sqr_direct(O::add(x, y)); break;  // (a + b)^2 through fu_sqr, operand not reduced
        case 10: r = O::template mul_sub<O::K2>(x, O::add(x, y), O::template sub<O::K1>(F::zero(), y), y); break;
        case 11: r = inv_gcd(x); break;
        case 8: {
            F ab = O::mul(x, y), bb = O::sqr(y);
            F X = O::template sub<O::K1>(O::sqr(x), O::add(ab, O::add(bb, bb)));
            r = O::mul(O::template sub<O::K2>(ab, X), O::template sub<O::K2>(bb, X));
            break;
        }
        default: break;
    }
    O::to_canonical(out, r);
}

// ---- madd chains (zkt_point_chain / zkd_point_chain) ------------------------------------------------------------------------
template <class F>
ZK_HD Affine<F> load_aff(const uint32_t *p, int inf) {
    typedef FieldOps<F> O;
    if (inf) return Affine<F>::infinity();
    return {O::from_canonical(p), O::from_canonical(p + O::CANON_WORDS)};
}
template <class F>
ZK_HD void store_aff(uint32_t *p, uint8_t *inf, const XYZZ<F> &a) {
    typedef FieldOps<F> O;
    Affine<F> r = xyzz_to_affine(a);
    *inf = a.is_inf() ? 1 : 0;
    O::to_canonical(p, r.x);
    O::to_canonical(p + O::CANON_WORDS, r.y);
}

// sum_i (+/-) pts[i] accumulated with xyzz_madd in order; result affine canonical.
// mode: 0 = madd chain; 1 = xyzz_add of the chains over the two halves; 2 = chain then xyzz_mul_small(acc, k);
//       3 = chain, xyzz_to_jacobian -> canonical Jacobian out (3 coords); 4 = like 0 but every partial sum goes
//       through the device-buffer store/load round trip (xyzz_store / xyzz_load, affine_store / affine_load)
template <class F>
ZK_HD void point_chain(const uint32_t *pts, const uint8_t *inf, const uint8_t *neg, size_t n, int mode, uint32_t k, uint32_t *out,
                       uint8_t *out_inf) {
    typedef FieldOps<F> O;
    constexpr int CW = O::CANON_WORDS;
    size_t split = mode == 1 ? n / 2 : n;
    XYZZ<F> acc = XYZZ<F>::infinity(), acc2 = XYZZ<F>::infinity();
    alignas(16) uint32_t b16[4 * O::WORDS];
    for (size_t i = 0; i < split; ++i) {
        Affine<F> p = load_aff<F>(pts + i * 2 * CW, inf ? inf[i] : 0);
        if (mode == 4) {
            affine_store<F>(b16, p);
            p = affine_load<F>(b16);
        }
        acc = xyzz_madd(acc, p, neg ? neg[i] != 0 : false);
        if (mode == 4) {
            xyzz_store<F>(b16, acc);
            acc = xyzz_load<F>(b16);
        }
    }
    for (size_t i = split; i < n; ++i) acc2 = xyzz_madd(acc2, load_aff<F>(pts + i * 2 * CW, inf ? inf[i] : 0), neg ? neg[i] != 0 : false);
    if (mode == 1) acc = xyzz_add(acc, acc2);
    if (mode == 2) acc = xyzz_mul_small(acc, k);
    if (mode == 3) {
        xyzz_store_canonical_jacobian<F>(out, acc);
        *out_inf = acc.is_inf() ? 1 : 0;
        return;
    }
    store_aff<F>(out, out_inf, acc);
}

// ---- the shared inversion (zkt_parked_affine / zkd_parked_affine) ----------------------------------------------------------------
// Entry k = the xyzz_madd chain over pts[0..k] (inf / neg as point_chain's).  All n entries are parked with xyzz_park, then
// xyzz_parked_to_affine turns them into n affine points: out = n canonical (x | y), out_inf = n flags.  layout 0: interleaved entries of 5
// field elements (X, Y, ZZ, ZZZ, prefix product); 1: the points in one array, the prefixes in another.  work: 7 n WORDS words (5 n for the
// parked entries, 2 n for the affine results in device form).
template <class F>
ZK_HD void parked_affine(const uint32_t *pts, const uint8_t *inf, const uint8_t *neg, size_t n, int layout, uint32_t *work, uint32_t *out,
                         uint8_t *out_inf) {
    typedef FieldOps<F> O;
    constexpr int CW = O::CANON_WORDS, NL = O::WORDS;
    auto pt = [&](uint32_t k) { return work + (size_t)k * (layout ? 4 : 5) * NL; };
    auto pre = [&](uint32_t k) { return layout ? work + (4 * n + k) * NL : work + ((size_t)k * 5 + 4) * NL; };
    XYZZ<F> acc = XYZZ<F>::infinity();
    F prod = F::one();
    for (size_t i = 0; i < n; ++i) {
        acc = xyzz_madd(acc, load_aff<F>(pts + i * 2 * CW, inf ? inf[i] : 0), neg ? neg[i] != 0 : false);
        xyzz_park(pt((uint32_t)i), pre((uint32_t)i), acc, prod);
    }
    xyzz_parked_to_affine(prod, (uint32_t)n, pt, pre, [&](uint32_t k) { return work + (5 * n + 2 * k) * NL; });
    for (size_t i = 0; i < n; ++i) store_aff<F>(out + i * 2 * CW, out_inf + i, XYZZ<F>::from_affine(affine_load<F>(work + (5 * n + 2 * i) * NL)));
}

}  // namespace arith
}  // namespace zkhip
