// What the pairing kernels (pairing.hip, groth16_verify.hip) share on the device: the word-major LDS / workspace slot of an Fq12 value
// and the way a coordinate of a bases object becomes a value of the tower.
#pragma once
#include "fu.hpp"
#include "pairing.hpp"

namespace zkhip {
namespace pairing_dev {

constexpr unsigned PAIR_LANES = 64;    // lanes per workgroup of the pairing kernels: one wave
constexpr unsigned F12_WORDS = 144;    // u32 words of an Fq12 value
constexpr unsigned COORD_WORDS = BlsFqU::SL;  // a bases object holds its coordinates in the lazy form of the curve kernels: 16 words per Fq
constexpr unsigned G1_WORDS = 2 * COORD_WORDS, G2_WORDS = 4 * COORD_WORDS;

// an Fq12 value in a word-major slot: word k at base[k * stride]
struct StridedStore {
    uint32_t *base;
    ZK_D pairing::Fq12 load() const {
        pairing::Fq12 r;
        uint32_t *w = reinterpret_cast<uint32_t *>(&r);
ZK_UNROLL
        for (unsigned k = 0; k < F12_WORDS; ++k) w[k] = base[k * PAIR_LANES];
        return r;
    }
    ZK_D void store(const pairing::Fq12 &a) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(&a);
ZK_UNROLL
        for (unsigned k = 0; k < F12_WORDS; ++k) base[k * PAIR_LANES] = w[k];
    }
};
static_assert(sizeof(pairing::Fq12) == F12_WORDS * 4, "an Fq12 value is 144 packed words");

ZK_D bool words_all_zero(const uint32_t *p, unsigned count) {
    uint32_t o = 0;
    for (unsigned i = 0; i < count; i += 4) {
        const uint4 t = *reinterpret_cast<const uint4 *>(p + i);
        o |= t.x | t.y | t.z | t.w;
    }
    return o == 0;
}

// a coordinate of a bases object (lazy 29-bit limbs, R = 2^406) as the saturated Montgomery value the tower computes on: two products
ZK_D pairing::Fq load_coord(const uint32_t *p) {
    uint32_t sat[BlsFq::NL];
    fu_to_canonical<BlsFqU>(sat, fu_load<BlsFqU>(p));
    pairing::Fq c;
ZK_UNROLL
    for (int i = 0; i < BlsFq::NL; ++i) c.v[i] = sat[i];
    return fp_to_mont(c);
}

}  // namespace pairing_dev
}  // namespace zkhip
