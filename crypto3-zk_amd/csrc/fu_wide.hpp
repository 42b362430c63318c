// G1 group law with ONE POINT PER WAVE, for dependent chains that leave most of the chip idle (device only).
//
// fu_quad.hpp shortens a tail operation by letting four lanes compute four different products of the formula; every lane still runs a whole
// Montgomery product (~460 instructions), and a lone wave issues one instruction per ~5 cycles whatever it is.  Here the product itself is spread
// over lanes: a field element lives ONE 29-bit limb per lane in a DPP row of 16 lanes (limb j in lane j of the row, lanes L .. 15 hold 0; L <= 15:
// lane 15 stays empty so that no carry of the normalisation crosses into the next row -- BLS12-381 has 14 limbs, BN254 and the Pasta fields 10),
// and the four rows of a wave compute the four products of a quad step at once.  A point is ONE register: row 0 = X, row 1 = Y, row 2 = ZZ,
// row 3 = ZZZ -- the order of the device-buffer layout, so a point's 4 * SL words load and store with one coalesced access.
//
// The product is operand scanning over the row, carry-save.  For step i = 0 .. L-1 lane j holds a column t_j:
//     t_j += a_i b_j              a_i: row broadcast of lane i (DPP row_newbcast)
//     q    = (t_0 QINV) mod 2^29  t_0: row broadcast of lane 0
//     t_j += q p_j                (now t_0 = 0 mod 2^29)
//     t_j  = (t_j >> 29) + (t_(j+1) mod 2^29)       one lane down (DPP row_shl:1); a lane keeps its own carry, whose weight is the next position
// Bounds: t_j enters a step below 2^32, gains two products of limbs below 2^30 (< 2^60 + 2^59), so t_j < 2^61, its carry < 2^32 and the next
// t_j < 2^32 again: the column is one 64-bit multiply-add target and the state between steps one 32-bit register.  After step L-1 the columns ARE
// the result's limbs, each below 2^31; wide_norm brings them to the unique normalised form.
//
// Contract -- fu.hpp's, limb for limb:
//   wide_mul   : limbs < 2^30 on both inputs, values a b < R p   ->  normalised limbs (< 2^29, the top limb keeps the rest), value < 2p
//   wide_add   : normalised inputs                                ->  normalised limbs, value = a + b
//   wide_sub<K>: b normalised with value(b) <= (K - 1) p          ->  normalised limbs, value = a + K p - b
// Every result is normalised EXACTLY (one neighbour round, then the remaining 0/1 carries resolved wave-wide from two ballots: generate = limb
// above 2^29 - 1, propagate = limb equal to it, carries = ((G | P) + G) ^ P), so a wide value has the very limbs the one-lane code computes for
// the same formula: the group law below is fu_quad.hpp's, product for product and K for K, and its results are bit-identical to the quad's.
//
// Rows meet through ds_bpermute (wide_rows); the schedules below place products so that most operands are already in their row: an addition
// takes 7 permutes, a doubling 4.  Every DPP result is pinned in a register of its own (see quad_bcast in fu_quad.hpp).
// Branches are uniform -- the wave holds one point: infinity and equal x (doubling / cancellation) gather the limbs and run the quad code.
// ALL 64 LANES of the wave must be active in every function of this header.
#pragma once
#include <utility>

#include "fu_quad.hpp"

namespace zkhip {

template <class U>
struct FuW {  // tag of the wide representation of Fu<U>
    typedef U params;
};

ZK_D uint32_t wide_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
ZK_D uint32_t wide_row() { return wide_lane() >> 4; }

// a point: row r of w is coordinate r (X, Y, ZZ, ZZZ)
template <class U>
struct XYZZ<FuW<U>> {
    uint32_t w;
    ZK_D bool is_inf() const { return ((uint32_t)(__builtin_amdgcn_ballot_w64(w == 0) >> 32) & 0xffffu) == 0xffffu; }  // ZZ = 0, exactly
    ZK_D static XYZZ infinity() { return {0u}; }
};

// per-lane constant: f(j) in lane j of every row, 0 in lanes L .. 15
template <class U, class Fn>
ZK_D uint32_t wide_const(Fn f) {
    const uint32_t j = wide_lane() & 15u;
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < U::L; ++i) r = j == (uint32_t)i ? f(i) : r;
    return r;
}
template <class U>
ZK_D uint32_t wide_mod() { return wide_const<U>([](int i) { return U::mod(i); }); }

template <int CTRL>
ZK_D uint32_t wide_dpp(uint32_t x) {
    uint32_t r = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
    asm volatile("" : "+v"(r));
    return r;
}
template <int I>
ZK_D uint32_t wide_bcast(uint32_t x) { return wide_dpp<0x150 + I>(x); }  // row_newbcast:I -- lane I of the row, on all its lanes
ZK_D uint32_t wide_down(uint32_t x) { return wide_dpp<0x101>(x); }       // row_shl:1 -- lane j takes lane j + 1, lane 15 takes 0
ZK_D uint32_t wide_up(uint32_t x) { return wide_dpp<0x111>(x); }         // row_shr:1 -- lane j takes lane j - 1, lane 0 takes 0

// row r of the result = row S_r of x
template <int S0, int S1, int S2, int S3>
ZK_D uint32_t wide_rows(uint32_t x) {
    constexpr uint32_t PACK = (uint32_t)(S0 | (S1 << 2) | (S2 << 4) | (S3 << 6));
    const uint32_t lane = wide_lane();
    const uint32_t src = (((PACK >> (2 * (lane >> 4))) & 3u) << 4) | (lane & 15u);
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)x);
}
// row 0 ? x0 : row 1 ? x1 : row 2 ? x2 : x3
ZK_D uint32_t wide_pick(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
    const uint32_t lane = wide_lane();
    const bool b0 = (lane & 16u) != 0, b1 = (lane & 32u) != 0;
    return b1 ? (b0 ? x3 : x2) : (b0 ? x1 : x0);
}

// limbs < 2^32 (the top limb, which keeps what the value leaves it, < 2^31) -> the normalised limbs of the same value
template <class U>
ZK_D uint32_t wide_norm(uint32_t v) {
    constexpr int L = U::L, B = U::B;
    constexpr uint32_t MASK = Fu<U>::MASK;
    static_assert(L <= 15, "lane 15 of a row ends the carry chain");
    constexpr uint64_t LOW = (((uint64_t)1 << (L - 1)) - 1) * 0x0001000100010001ull;  // the lanes of the limbs below the top one: they pass their carries on
    const bool low = (wide_lane() & 15u) < (uint32_t)(L - 1);
    const uint32_t lm = low ? MASK : 0xffffffffu;
    const uint32_t v1 = (v & lm) + wide_up(v >> (low ? B : 31));  // <= 2^29 - 1 + 7: what is left to pass is 0 or 1 per limb
    const uint64_t G = __builtin_amdgcn_ballot_w64(v1 > MASK) & LOW, P = __builtin_amdgcn_ballot_w64(v1 == MASK) & LOW;
    const uint64_t cin = ((G | P) + G) ^ P;  // bit = carry INTO that lane; G = P = 0 in lanes L-1 .. 15, so no carry crosses a row
    uint32_t r;
    uint64_t cout;
    asm("v_addc_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(r), "=s"(cout) : "v"(v1), "s"(cin));  // v1 + the lane's bit of cin
    return r & lm;
}

template <class U>
ZK_D uint32_t wide_add(uint32_t a, uint32_t b) { return wide_norm<U>(a + b); }
template <int K, class U>
ZK_D uint32_t wide_sub(uint32_t a, uint32_t b) {
    const uint32_t s = wide_const<U>([](int i) { return U::template spread<K>(i); });
    return wide_norm<U>(a + (s - b));
}

template <int L, int... I>
ZK_D void wide_bcast_all(uint32_t a, uint32_t (&ai)[L], std::integer_sequence<int, I...>) {
    ((ai[I] = wide_bcast<I>(a)), ...);
}
// row-wise Montgomery product: row r of the result = (row r of a) (row r of b) / R
template <class U>
ZK_D uint32_t wide_mul(uint32_t a, uint32_t b) {
    constexpr int L = U::L, B = U::B;
    constexpr uint32_t MASK = Fu<U>::MASK;
    static_assert(B == 29, "the column bounds are those of 29-bit limbs");
    const uint32_t p = wide_mod<U>();
    uint32_t ai[L];
    wide_bcast_all(a, ai, std::make_integer_sequence<int, L>());
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < L; ++i) {
        uint64_t acc = (uint64_t)ai[i] * b + t;
        const uint32_t q = (wide_bcast<0>((uint32_t)acc) * U::QINV) & MASK;
        acc += (uint64_t)q * p;
        t = (uint32_t)(acc >> B) + wide_down((uint32_t)acc & MASK);
    }
    return wide_norm<U>(t);
}

// ---- between the wide form and whole coordinates (rare branches, tests) ------------------------------------------------------------------
template <class U>
ZK_D XYZZ<FuQ<U>> wide_gather(const XYZZ<FuW<U>> &a) {  // the point, whole, on every lane
    XYZZ<FuQ<U>> r;
    Fu<U> *c[4] = {&r.X.v, &r.Y.v, &r.ZZ.v, &r.ZZZ.v};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int i = 0; i < U::L; ++i) c[k]->v[i] = (uint32_t)__builtin_amdgcn_readlane((int)a.w, 16 * k + i);
    }
    return r;
}
template <class U>
ZK_D XYZZ<FuW<U>> wide_scatter(const XYZZ<FuQ<U>> &a) {  // a: the same on every lane
    const Fu<U> *c[4] = {&a.X.v, &a.Y.v, &a.ZZ.v, &a.ZZZ.v};
    uint32_t x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = wide_const<U>([&](int i) { return c[k]->v[i]; });
    return {wide_pick(x[0], x[1], x[2], x[3])};
}

// a point's 4 * SL contiguous words <-> the wave, one access.  A row has 16 lanes, so SL <= 16; the load takes the L limbs and leaves lanes
// L .. 15 at 0 whatever the padding words hold, the store writes the padding words as 0 (lanes L .. 15 of every wide value are 0).
template <class U>
ZK_D XYZZ<FuW<U>> wide_load(const uint32_t *p) {
    static_assert(U::L <= 15 && U::SL <= 16 && U::L <= U::SL, "a coordinate is one DPP row");
    const uint32_t lane = wide_lane(), j = lane & 15u;
    return {j < (uint32_t)U::L ? p[(lane >> 4) * U::SL + j] : 0u};
}
template <class U>
ZK_D void wide_store(uint32_t *p, const XYZZ<FuW<U>> &a) {
    static_assert(U::L <= 15 && U::SL <= 16 && U::L <= U::SL, "a coordinate is one DPP row");
    const uint32_t lane = wide_lane(), j = lane & 15u;
    if (j < (uint32_t)U::SL) p[(lane >> 4) * U::SL + j] = a.w;
}

// the rare branches, out of line: gather, run the quad law (all lanes hold the same operands, as its quads do), scatter
template <class U>
__device__ __noinline__ uint32_t wide_add_whole(uint32_t a, uint32_t b) {
    return wide_scatter<U>(xyzz_add(wide_gather<U>(XYZZ<FuW<U>>{a}), wide_gather<U>(XYZZ<FuW<U>>{b}))).w;
}

// 2 a: fu_quad.hpp's three product steps.  Rows:  s1 = X^2 | U^2 | U^2 | U^2,  s2 = M^2 | U V | ZZ V | X V,  s3 = M D | W Y | - | ZZZ W
template <class U>
ZK_D XYZZ<FuW<U>> xyzz_dbl(const XYZZ<FuW<U>> &a) {
    typedef FieldOps<Fu<U>> O;
    if (a.is_inf()) return XYZZ<FuW<U>>::infinity();
    const uint32_t row = wide_row();
    const uint32_t a2 = wide_add<U>(a.w, a.w);                                  // row 1: U = 2 Y
    const uint32_t o1 = row == 0 ? a.w : wide_rows<1, 1, 1, 1>(a2);
    const uint32_t s1 = wide_mul<U>(o1, o1);                                    // XX | V | V | V
    const uint32_t M = wide_norm<U>(s1 + s1 + s1);                              // row 0: M = 3 XX
    const uint32_t s2 = wide_mul<U>(wide_pick(M, a2, a.w, wide_rows<0, 0, 0, 0>(a.w)), row == 0 ? M : s1);  // MM | W | ZZ3 | S
    const uint32_t sw = wide_rows<3, 1, 1, 1>(s2);                              // row 0: S, row 3: W
    const uint32_t X3 = wide_sub<O::K1, U>(s2, wide_add<U>(sw, sw));            // row 0
    const uint32_t D = wide_sub<O::K2, U>(sw, X3);                              // row 0
    const uint32_t s3 = wide_mul<U>(row == 0 ? M : (row == 1 ? s2 : a.w), wide_pick(D, a.w, a.w, sw));  // MD | WY | - | ZZZ3
    const uint32_t Y3 = wide_sub<O::K1, U>(wide_rows<0, 0, 0, 0>(s3), s3);      // row 1
    return {wide_pick(X3, Y3, s2, s3)};
}

// a + b: fu_quad.hpp's four product steps.
// Rows:  s1 = U1 | S1 | U2 | S2,  s2 = Pd^2 | R^2 | ZZa ZZb | ZZZa ZZZb,  s3 = Pd PP | U1 PP | ZZab PP | -,  s4 = S1 PPP | D R | - | ZZZab PPP
template <class U>
ZK_D XYZZ<FuW<U>> xyzz_add(const XYZZ<FuW<U>> &a, const XYZZ<FuW<U>> &b) {
    typedef FieldOps<Fu<U>> O;
    if (a.is_inf()) return b;
    if (b.is_inf()) return a;
    const uint32_t row = wide_row();
    const uint32_t s1 = wide_mul<U>(a.w, wide_rows<2, 3, 0, 1>(b.w));           // Xa ZZb | Ya ZZZb | ZZa Xb | ZZZa Yb
    const uint32_t T = wide_sub<O::K1, U>(wide_rows<2, 3, 2, 3>(s1), s1);       // rows 0, 1: Pd = U2 - U1, R = S2 - S1
    const uint32_t s2 = wide_mul<U>(row < 2 ? T : a.w, row < 2 ? T : b.w);      // PP | RR | ZZab | ZZZab
    {
        const uint32_t z = (uint32_t)__builtin_amdgcn_ballot_w64(s2 == 0) & 0xffffu, e = (uint32_t)__builtin_amdgcn_ballot_w64(s2 == wide_mod<U>()) & 0xffffu;
        if (z == 0xffffu || e == 0xffffu) return {wide_add_whole<U>(a.w, b.w)};  // PP = 0 mod p (PP < 2p): same x, doubling or cancellation (rare)
    }
    const uint32_t sx = wide_rows<1, 0, 0, 0>(s1);                              // row 0: S1, row 1: U1
    const uint32_t s3 = wide_mul<U>(wide_pick(T, sx, s2, s2), wide_rows<0, 0, 0, 0>(s2));  // PPP | Q | ZZ3 | -
    const uint32_t PPP = wide_rows<0, 0, 0, 0>(s3);
    const uint32_t X3 = wide_sub<O::K1, U>(s2, wide_norm<U>(PPP + s3 + s3));     // row 1: RR - (PPP + 2 Q)
    const uint32_t D = wide_sub<O::K2, U>(s3, X3);                              // row 1
    const uint32_t s4 = wide_mul<U>(wide_pick(sx, D, s2, s2), row == 1 ? T : PPP);         // S1 PPP | D R | - | ZZZ3
    const uint32_t Y3 = wide_sub<O::K1, U>(s4, wide_rows<0, 0, 0, 0>(s4));      // row 1
    return {wide_pick(wide_rows<1, 1, 1, 1>(X3), Y3, s3, s4)};
}

// k * a, bit by bit (as the quad's)
template <class U>
ZK_D XYZZ<FuW<U>> xyzz_mul_small(const XYZZ<FuW<U>> &a, uint32_t k) {
    XYZZ<FuW<U>> r = XYZZ<FuW<U>>::infinity();
    if (k == 0 || a.is_inf()) return r;
    int top = 31;
    while (!((k >> top) & 1)) --top;
    r = a;
    for (int i = top - 1; i >= 0; --i) {
        r = xyzz_dbl(r);
        if ((k >> i) & 1) r = xyzz_add(r, a);
    }
    return r;
}

// the wide type of a bucket coordinate field, where one exists (G1)
template <class F>
struct WideLane {
    static constexpr bool AVAILABLE = false;
    typedef typename TailLane<F>::type type;
    static constexpr int LANES = TailLane<F>::LANES;
};
template <class U>
struct WideLane<Fu<U>> {
    static constexpr bool AVAILABLE = true;
    typedef FuW<U> type;
    static constexpr int LANES = 64;
    ZK_D static XYZZ<type> xyzz_load(const uint32_t *p) { return wide_load<U>(p); }
    ZK_D static void xyzz_store(uint32_t *p, const XYZZ<type> &a) { wide_store<U>(p, a); }
    ZK_D static XYZZ<type> xyzz_add(const XYZZ<type> &a, const XYZZ<type> &b) { return zkhip::xyzz_add(a, b); }
    ZK_D static XYZZ<type> xyzz_dbl(const XYZZ<type> &a) { return zkhip::xyzz_dbl(a); }
    ZK_D static XYZZ<type> xyzz_mul_small(const XYZZ<type> &a, uint32_t k) { return zkhip::xyzz_mul_small(a, k); }
};

}  // namespace zkhip
