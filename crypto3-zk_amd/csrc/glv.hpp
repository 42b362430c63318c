// The GLV split of a scalar for the j = 0 curves (y^2 = x^3 + b, p = r = 1 mod 3): phi(x, y) = (beta x, y) = lambda P with
// lambda^2 + lambda + 1 = 0 (mod r), beta^2 + beta + 1 = 0 (mod p), so k P = k1 P + k2 phi(P) with k = k1 + k2 lambda (mod r) and both
// halves about half as long as k.  The EC-NTT's twiddle records (ecntt.hip) are built from it; __host__ __device__, so the no-GPU
// suite runs the very same code against big integers (hosttest.hip: zkt_glv_split).
//
// Constants of a curve: the lattice basis (a1, b1), (a2, b2) of {(a, b) : a + b lambda = 0 (mod r)} from the extended Euclid on (r, lambda),
// with the signs  a1 > 0, b1 < 0, a2 > 0, b2 > 0  (so a1 b2 - a2 b1 = r) and stored as magnitudes; g1 = floor(2^256 |b2| / r),
// g2 = floor(2^256 |b1| / r).  With c1 = floor(k g1 / 2^256), c2 = floor(k g2 / 2^256)
//   k1 = k - c1 |a1| - c2 |a2|,  k2 = + c1 |b1| - c2 |b2|
// Any (c1, c2) gives k1 + k2 lambda = k (mod r); these keep |k1|, |k2| at or below 2^128 (tests/test_host_glv.py).  All constants fit 5 words,
// both halves 6 words in two's complement, 33 signed nibbles each.  Of the two cube roots of unity mod r, lambda is the one that
// belongs to beta: (beta x, y) = lambda (x, y) on the curve's group.
#pragma once
#include "zk_defs.hpp"

namespace zkhip {

struct NoGlv {
    static constexpr bool ENABLED = false;
};
struct BlsGlv {  // lambda = z^2 - 1 = 0xac45a4010001a40200000000ffffffff; basis (lambda, -1), (1, lambda + 1)
    static constexpr bool ENABLED = true;
    ZK_HD static uint32_t g1(int i) { constexpr uint32_t t[5] = {0xf6cfee30u, 0x63f6e522u, 0xe01faaddu, 0x7c6becf1u, 0x00000001u}; return t[i]; }
    ZK_HD static uint32_t g2(int i) { constexpr uint32_t t[5] = {0x00000002u, 0, 0, 0, 0}; return t[i]; }
    ZK_HD static uint32_t a1(int i) { constexpr uint32_t t[5] = {0xffffffffu, 0x00000000u, 0x0001a402u, 0xac45a401u, 0}; return t[i]; }
    ZK_HD static uint32_t a2(int i) { constexpr uint32_t t[5] = {0x00000001u, 0, 0, 0, 0}; return t[i]; }
    ZK_HD static uint32_t b1(int i) { constexpr uint32_t t[5] = {0x00000001u, 0, 0, 0, 0}; return t[i]; }
    ZK_HD static uint32_t b2(int i) { constexpr uint32_t t[5] = {0x00000000u, 0x00000001u, 0x0001a402u, 0xac45a401u, 0}; return t[i]; }
    static constexpr int BETA_WORDS = 12;
    ZK_HD static uint32_t beta(int i) {  // canonical
        constexpr uint32_t t[12] = {0x0000aaacu, 0x8bfd0000u, 0x4f49fffdu, 0x409427ebu, 0x0fb85f9bu, 0x897d2965u,
                                    0x89759ad4u, 0xaa0d857du, 0x63d4de85u, 0xec024086u, 0x397fe699u, 0x1a0111eau};
        return t[i];
    }
};
struct BnGlv {  // lambda = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd; basis (a1, -b1), (a2, b2) from the extended Euclid on (r, lambda)
    static constexpr bool ENABLED = true;
    ZK_HD static uint32_t g1(int i) { constexpr uint32_t t[5] = {0xc7e0b3d7u, 0xd91d232eu, 0x00000002u, 0, 0}; return t[i]; }
    ZK_HD static uint32_t g2(int i) { constexpr uint32_t t[5] = {0x391eb18du, 0x7a7bd9d4u, 0xa773d2cfu, 0x4ccef014u, 0x00000002u}; return t[i]; }
    ZK_HD static uint32_t a1(int i) { constexpr uint32_t t[5] = {0x94d213e3u, 0x89d32568u, 0, 0, 0}; return t[i]; }
    ZK_HD static uint32_t a2(int i) { constexpr uint32_t t[5] = {0x1221250bu, 0x0be4e154u, 0xeeb859fdu, 0x6f4d8248u, 0}; return t[i]; }
    ZK_HD static uint32_t b1(int i) { constexpr uint32_t t[5] = {0x7d4f1128u, 0x8211bbebu, 0xeeb859fcu, 0x6f4d8248u, 0}; return t[i]; }
    ZK_HD static uint32_t b2(int i) { constexpr uint32_t t[5] = {0x94d213e3u, 0x89d32568u, 0, 0, 0}; return t[i]; }
    static constexpr int BETA_WORDS = 8;
    ZK_HD static uint32_t beta(int i) {  // canonical
        constexpr uint32_t t[8] = {0x77fffffeu, 0x57634731u, 0xacdb5c4fu, 0xd4f263f1u, 0xa0d48bacu, 0x59e26bceu, 0, 0};
        return t[i];
    }
};
// Pallas and Vesta: beta = 2^((p - 1) / 3) mod p, lambda the cube root of unity mod r that belongs to it, the basis as above
struct PallasGlv {  // lambda = 0x397e65a7d7c1ad71aee24b27e308f0a61259527ec1d4752e619d1840af55f1b1
    static constexpr bool ENABLED = true;
    ZK_HD static uint32_t g1(int i) { constexpr uint32_t t[5] = {0xffffffffu, 0x32c49e4bu, 0x02a2654eu, 0x279a7459u, 0x00000001u}; return t[i]; }
    ZK_HD static uint32_t g2(int i) { constexpr uint32_t t[5] = {0x00000003u, 0xff2b871cu, 0x03c12455u, 0x279a7459u, 0x00000001u}; return t[i]; }
    ZK_HD static uint32_t a1(int i) { constexpr uint32_t t[5] = {0x00000000u, 0x8cb12793u, 0x40a89953u, 0x49e69d16u, 0}; return t[i]; }
    ZK_HD static uint32_t a2(int i) { constexpr uint32_t t[5] = {0x00000001u, 0x0c7c095au, 0x8198e269u, 0x93cd3a2cu, 0}; return t[i]; }
    ZK_HD static uint32_t b1(int i) { constexpr uint32_t t[5] = {0x00000001u, 0x7fcae1c7u, 0x40f04915u, 0x49e69d16u, 0}; return t[i]; }
    ZK_HD static uint32_t b2(int i) { constexpr uint32_t t[5] = {0x00000000u, 0x8cb12793u, 0x40a89953u, 0x49e69d16u, 0}; return t[i]; }
    static constexpr int BETA_WORDS = 8;
    ZK_HD static uint32_t beta(int i) {  // canonical
        constexpr uint32_t t[8] = {0x0201b547u, 0x7b7fd22fu, 0xd19fc7d2u, 0x05270d29u, 0xa8554e50u, 0xd3552a23u, 0xb532458eu, 0x2d33357cu};
        return t[i];
    }
};
struct VestaGlv {  // lambda = 0x12ccca834acdba712caad5dc57aab1b01d1f8bd237ad31491dad5ebdfdfe4ab9
    static constexpr bool ENABLED = true;
    ZK_HD static uint32_t g1(int i) { constexpr uint32_t t[5] = {0x00000002u, 0x31f02568u, 0x066389a4u, 0x4f34e8b2u, 0x00000002u}; return t[i]; }
    ZK_HD static uint32_t g2(int i) { constexpr uint32_t t[5] = {0x00000003u, 0x32c49e4cu, 0x02a2654eu, 0x279a7459u, 0x00000001u}; return t[i]; }
    ZK_HD static uint32_t a1(int i) { constexpr uint32_t t[5] = {0x00000000u, 0x7fcae1c7u, 0x40f04915u, 0x49e69d16u, 0}; return t[i]; }
    ZK_HD static uint32_t a2(int i) { constexpr uint32_t t[5] = {0x00000001u, 0x8cb12793u, 0x40a89953u, 0x49e69d16u, 0}; return t[i]; }
    ZK_HD static uint32_t b1(int i) { constexpr uint32_t t[5] = {0x00000001u, 0x8cb12793u, 0x40a89953u, 0x49e69d16u, 0}; return t[i]; }
    ZK_HD static uint32_t b2(int i) { constexpr uint32_t t[5] = {0x00000001u, 0x0c7c095au, 0x8198e269u, 0x93cd3a2cu, 0}; return t[i]; }
    static constexpr int BETA_WORDS = 8;
    ZK_HD static uint32_t beta(int i) {  // canonical
        constexpr uint32_t t[8] = {0x50aa0e4fu, 0x2aa9d2e0u, 0x47c033afu, 0x0fed467du, 0x1cf70f5au, 0x511db4d8u, 0x283e528eu, 0x06819a58u};
        return t[i];
    }
};

// t (6 words) +/-= a (5 words) * b (5 words)   modulo 2^192
ZK_HD void glv_acc_mul_192(uint32_t *t, const uint32_t *a, const uint32_t *b, bool subtract) {
    uint32_t prod[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 5; ++i) {
        uint64_t carry = 0;
        for (int j = 0; i + j < 6 && j < 5; ++j) {
            const uint64_t cur = (uint64_t)prod[i + j] + (uint64_t)a[i] * b[j] + carry;
            prod[i + j] = (uint32_t)cur;
            carry = cur >> 32;
        }
        if (i + 5 < 6) prod[i + 5] = (uint32_t)carry;
    }
    uint64_t c = subtract ? 1 : 0;  // t - prod = t + ~prod + 1
    for (int i = 0; i < 6; ++i) {
        const uint64_t cur = (uint64_t)t[i] + (subtract ? (uint32_t)~prod[i] : prod[i]) + c;
        t[i] = (uint32_t)cur;
        c = cur >> 32;
    }
}

// words 8..12 of k (8 words) * g (5 words)
ZK_HD void glv_mul_hi_256(uint32_t *out5, const uint32_t *k, const uint32_t *g) {
    uint32_t t[13];
    for (int i = 0; i < 13; ++i) t[i] = 0;
    for (int i = 0; i < 8; ++i) {
        uint64_t carry = 0;
        for (int j = 0; j < 5; ++j) {
            const uint64_t cur = (uint64_t)t[i + j] + (uint64_t)k[i] * g[j] + carry;
            t[i + j] = (uint32_t)cur;
            carry = cur >> 32;
        }
        t[i + 5] = (uint32_t)carry;
    }
    for (int i = 0; i < 5; ++i) out5[i] = t[8 + i];
}

// k (8 words, below r) -> the MAGNITUDES of k1 and k2 (6 words each); bit h of the result: half h is negative
template <class G>
ZK_HD uint32_t glv_split(const uint32_t *k, uint32_t *k1, uint32_t *k2) {
    uint32_t c1[5], c2[5], cst[5];
    for (int i = 0; i < 5; ++i) cst[i] = G::g1(i);
    glv_mul_hi_256(c1, k, cst);
    for (int i = 0; i < 5; ++i) cst[i] = G::g2(i);
    glv_mul_hi_256(c2, k, cst);
    for (int i = 0; i < 6; ++i) k1[i] = k[i], k2[i] = 0;  // k modulo 2^192: k1 and k2 are small, the arithmetic is exact in two's complement
    for (int i = 0; i < 5; ++i) cst[i] = G::a1(i);
    glv_acc_mul_192(k1, c1, cst, true);
    for (int i = 0; i < 5; ++i) cst[i] = G::a2(i);
    glv_acc_mul_192(k1, c2, cst, true);
    for (int i = 0; i < 5; ++i) cst[i] = G::b1(i);
    glv_acc_mul_192(k2, c1, cst, false);
    for (int i = 0; i < 5; ++i) cst[i] = G::b2(i);
    glv_acc_mul_192(k2, c2, cst, true);
    uint32_t signs = 0;
    uint32_t *half[2] = {k1, k2};
    for (int h = 0; h < 2; ++h) {
        if (half[h][5] >> 31) {  // negative: take the magnitude
            signs |= 1u << h;
            uint64_t c = 1;
            for (int i = 0; i < 6; ++i) {
                const uint64_t cur = (uint64_t)(uint32_t)~half[h][i] + c;
                half[h][i] = (uint32_t)cur;
                c = cur >> 32;
            }
        }
    }
    return signs;
}

// ---- the window record of a scalar: what the fixed 4-bit ladder of ecntt.hip reads (the group DFT's twiddles, zkhip_bases_scale_*'s scalars)
constexpr int REC_WORDS = 12;  // GLV  [0..4] nibbles of |k1|, [5..9] nibbles of |k2|, [10] bit h = half h negative
                               // plain [0..8] nibbles of k (65 used), [10] = 0

// signed 4-bit windows of an unsigned magnitude: digit w in [-8, 7] as a two's-complement nibble, sum_w d_w 16^w = mag
ZK_HD void recode_nibbles(uint32_t *out, int out_words, const uint32_t *mag, int mag_words, int windows) {
    for (int i = 0; i < out_words; ++i) out[i] = 0;
    uint32_t carry = 0;
    for (int w = 0; w < windows; ++w) {
        const int word = w >> 3;
        uint32_t d = (word < mag_words ? (mag[word] >> ((w & 7) * 4)) & 15u : 0u) + carry;
        carry = d >= 8 ? 1 : 0;  // d - 16 in [-8, 0]: the nibble (d & 15) read as two's complement
        out[word] |= (d & 15u) << ((w & 7) * 4);
    }
}

// k (8 words, below r) -> its record: the GLV split (G1) and the signed-nibble recoding
template <class G>
ZK_HD void scalar_record(uint32_t *out, const uint32_t *k) {
    if constexpr (G::ENABLED) {
        uint32_t k1[6], k2[6];
        const uint32_t signs = glv_split<G>(k, k1, k2);
        recode_nibbles(out, 5, k1, 6, 33);
        recode_nibbles(out + 5, 5, k2, 6, 33);
        out[10] = signs;
        out[11] = 0;
    } else {
        recode_nibbles(out, 9, k, 8, 65);
        out[9] = out[10] = out[11] = 0;
    }
}

}  // namespace zkhip
