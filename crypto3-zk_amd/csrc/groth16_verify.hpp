// The Groth16 verifier's bodies (zkhip_groth16_verify_batch; include/zkhip.h, "Groth16 verification"), __host__ __device__: the kernels of
// groth16_verify.hip and the CPU twin of hosttest.hip run them.  Per proof, r1cs_gg_ppzksnark_verifier_weak_input_consistency::process
// of the reference (systems/ppzksnark/r1cs_gg_ppzksnark/verifier.hpp:150-186):
//     acc = abc[0] + sum_j x_j abc[j + 1]
//     ok  = A, B, C on their curves  &&  final_exponentiation(miller(A, B) miller(-acc, gamma) miller(-C, delta)) == alpha_beta
//
// A prepared key (Groth16Key) holds alpha_beta in Montgomery form, the prepared lines of gamma and delta (pairing.hpp), abc[0], and per
// further abc point a fixed-base window table: windows of ACC_WINDOW_BITS = 4 bits, for window w the 15 affine points d 16^w abc[j],
// d = 1 .. 15.  A lane adds one table entry per non-zero nibble of x_j (mixed additions, no doublings): at most 64 additions per input.
// G1 arithmetic here is over the saturated Montgomery type of the tower, not the lazy type of the MSM kernels: the accumulation's result
// feeds the Miller loop, and 64 additions per input do not pay for a conversion layer.
#pragma once
#include <algorithm>
#include <vector>

#include "pairing.hpp"

namespace zkhip {
namespace groth16v {

using pairing::Fq;
using pairing::Fq12;
using pairing::Fq2;
using pairing::Line;

constexpr int ACC_WINDOW_BITS = 4, ACC_WINDOWS = 64, ACC_ENTRIES = 15;           // 64 nibbles cover any 256-bit scalar
constexpr unsigned FQ_WORDS = 12, AFFINE_WORDS = 2 * FQ_WORDS;                   // an affine G1 point in Montgomery form; all words zero: infinity
constexpr size_t ACC_TABLE_WORDS = (size_t)ACC_WINDOWS * ACC_ENTRIES * AFFINE_WORDS;  // per input: 960 points = 92160 bytes
constexpr unsigned LINE_WORDS = 6 * FQ_WORDS;
static_assert(sizeof(Line) == LINE_WORDS * 4 && sizeof(Fq) == FQ_WORDS * 4, "lines and coordinates are stored as their packed words");

// the words of a prepared key, in this order (device memory for the kernels, a host vector for the twin)
struct Groth16Key {
    const uint32_t *alpha_beta;    // 144
    const Line *gamma, *delta;     // PREPARED_LINES each
    const uint32_t *abc0;          // AFFINE_WORDS
    const uint32_t *tables;        // (n_abc - 1) x ACC_TABLE_WORDS
};
constexpr size_t KEY_FIXED_WORDS = 144 + 2 * (size_t)pairing::PREPARED_LINES * LINE_WORDS + AFFINE_WORDS;
ZK_HD Groth16Key key_at(const uint32_t *p) {
    const uint32_t *g = p + 144, *d = g + pairing::PREPARED_LINES * LINE_WORDS, *a = d + pairing::PREPARED_LINES * LINE_WORDS;
    return {p, reinterpret_cast<const Line *>(g), reinterpret_cast<const Line *>(d), a, a + AFFINE_WORDS};
}

ZK_HD Fq fq_at(const uint32_t *p) {
    Fq r;
ZK_UNROLL
    for (unsigned i = 0; i < FQ_WORDS; ++i) r.v[i] = p[i];
    return r;
}
ZK_HD void fq_put(uint32_t *p, const Fq &a) {
ZK_UNROLL
    for (unsigned i = 0; i < FQ_WORDS; ++i) p[i] = a.v[i];
}
ZK_HD bool affine_is_infinity(const uint32_t *p) {
    uint32_t o = 0;
    for (unsigned i = 0; i < AFFINE_WORDS; ++i) o |= p[i];
    return o == 0;
}

ZK_HD Fq fq_four() { return fp_dbl(fp_dbl(Fq::one())); }
// y^2 = x^3 + 4 and, on the twist, y^2 = x^3 + 4 (u + 1): what the reference's is_well_formed() asks of a point that is not at infinity
ZK_HD bool g1_on_curve(const Fq &x, const Fq &y) { return fp_sqr(y) == fp_sqr(x) * x + fq_four(); }
ZK_HD bool g2_on_curve(const Fq2 &x, const Fq2 &y) {
    const Fq2 b = {fq_four(), fq_four()};
    return fp_sqr(y) == fp_sqr(x) * x + b;
}

struct G1Jac {  // (X / Z^2, Y / Z^3); Z = 0: infinity
    Fq x, y, z;
    ZK_HD static G1Jac infinity() { return {Fq::one(), Fq::one(), Fq::zero()}; }
    ZK_HD bool is_infinity() const { return z.is_zero(); }
};
ZK_HD G1Jac g1_from_affine(const uint32_t *p) {
    if (affine_is_infinity(p)) return G1Jac::infinity();
    return {fq_at(p), fq_at(p + FQ_WORDS), Fq::one()};
}
// dbl-2009-l (a = 0): 5 squarings + 2 products
ZK_HD G1Jac g1_dbl(const G1Jac &t) {
    const Fq a = fp_sqr(t.x), b = fp_sqr(t.y), c = fp_sqr(b);
    const Fq d = fp_dbl(fp_sqr(t.x + b) - a - c), e = fp_dbl(a) + a;
    G1Jac r;
    r.x = fp_sqr(e) - fp_dbl(d);
    r.y = e * (d - r.x) - fp_dbl(fp_dbl(fp_dbl(c)));
    r.z = fp_dbl(t.y * t.z);
    return r;
}
// t + (xq, yq), the affine point not at infinity; complete: t at infinity, t = +-(xq, yq).  3 squarings + 8 products.
ZK_HD G1Jac g1_madd(const G1Jac &t, const Fq &xq, const Fq &yq) {
    if (t.is_infinity()) return {xq, yq, Fq::one()};
    const Fq zz = fp_sqr(t.z);
    const Fq h = xq * zz - t.x, r = yq * (t.z * zz) - t.y;
    if (h.is_zero()) return r.is_zero() ? g1_dbl(t) : G1Jac::infinity();
    const Fq hh = fp_sqr(h), hhh = h * hh, v = t.x * hh;
    G1Jac o;
    o.x = fp_sqr(r) - hhh - fp_dbl(v);
    o.y = r * (v - o.x) - t.y * hhh;
    o.z = t.z * h;
    return o;
}

// acc = abc[0] + sum_{j < n_inputs} x_j abc[j + 1] from the key's tables; x: n_inputs scalars of 8 words, any 256-bit values
ZK_HD G1Jac accumulate(const Groth16Key &key, const uint32_t *x, size_t n_inputs) {
    G1Jac acc = g1_from_affine(key.abc0);
    for (size_t j = 0; j < n_inputs; ++j) {
        const uint32_t *tab = key.tables + j * ACC_TABLE_WORDS;
        for (int w = 0; w < ACC_WINDOWS; ++w) {
            const uint32_t d = (x[j * 8 + (w >> 3)] >> ((w & 7) * ACC_WINDOW_BITS)) & 15u;
            if (d == 0) continue;
            const uint32_t *e = tab + ((size_t)w * ACC_ENTRIES + (d - 1)) * AFFINE_WORDS;
            if (affine_is_infinity(e)) continue;  // only a key point outside the order-r subgroup, or at infinity, has such entries
            acc = g1_madd(acc, fq_at(e), fq_at(e + FQ_WORDS));
        }
    }
    return acc;
}
// out (AFFINE_WORDS) <- -acc, affine: one inversion
ZK_HD void neg_affine(uint32_t *out, const G1Jac &acc) {
    if (acc.is_infinity()) {
        for (unsigned i = 0; i < AFFINE_WORDS; ++i) out[i] = 0;
        return;
    }
    const Fq zi = fp_inv(acc.z), zi2 = fp_sqr(zi);
    fq_put(out, acc.x * zi2);
    fq_put(out + FQ_WORDS, fp_neg(acc.y * (zi2 * zi)));
}

// One proof's points as the Miller stage takes them: Montgomery form, infinity flags apart
struct ProofPoints {
    bool a_inf, b_inf, c_inf;
    Fq ax, ay, cx, cy;
    Fq2 bx, by;
    ZK_HD bool well_formed() const { return (a_inf || g1_on_curve(ax, ay)) && (b_inf || g2_on_curve(bx, by)) && (c_inf || g1_on_curve(cx, cy)); }
};
// fs <- miller(A, B) miller(-acc, gamma) miller(-C, delta); neg_acc: what neg_affine wrote
template <class FStore>
ZK_HD void miller3(FStore &fs, const Groth16Key &key, const ProofPoints &p, const uint32_t *neg_acc) {
    const pairing::WalkedPair w = {!p.a_inf && !p.b_inf, p.ax, p.ay, p.bx, p.by};
    const pairing::PreparedPair g = {!affine_is_infinity(neg_acc), fq_at(neg_acc), fq_at(neg_acc + FQ_WORDS), key.gamma};
    const pairing::PreparedPair d = {!p.c_inf, p.cx, fp_neg(p.cy), key.delta};
    pairing::miller_loop3(fs, w, g, d);
}
ZK_HD bool equals_alpha_beta(const Groth16Key &key, const Fq12 &v) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(&v);
    uint32_t o = 0;
    for (unsigned k = 0; k < 144; ++k) o |= w[k] ^ key.alpha_beta[k];
    return o == 0;
}

// ---- making a key (host only; once per key) ----------------------------------------------------------------------------------------

// the affine forms of `pts` (AFFINE_WORDS each) with ONE inversion (Montgomery's trick); infinity becomes all zero words
inline void batch_to_affine(uint32_t *out, const std::vector<G1Jac> &pts) {
    std::vector<Fq> prefix(pts.size());
    Fq run = Fq::one();
    for (size_t i = 0; i < pts.size(); ++i) {
        prefix[i] = run;
        if (!pts[i].is_infinity()) run = run * pts[i].z;
    }
    Fq inv = fp_inv(run);
    for (size_t i = pts.size(); i-- > 0;) {
        uint32_t *o = out + i * AFFINE_WORDS;
        if (pts[i].is_infinity()) {
            std::fill(o, o + AFFINE_WORDS, 0u);
            continue;
        }
        const Fq zi = inv * prefix[i], zi2 = fp_sqr(zi);
        inv = inv * pts[i].z;
        fq_put(o, pts[i].x * zi2);
        fq_put(o + FQ_WORDS, pts[i].y * (zi2 * zi));
    }
}

inline Fq fq_from_canonical(const uint64_t *limbs) {
    Fq c;
    for (unsigned i = 0; i < FQ_WORDS; ++i) c.v[i] = (uint32_t)(limbs[i / 2] >> (32 * (i & 1)));
    return fp_to_mont(c);
}

// The words of a prepared key from the canonical values of zkhip_groth16_vk_upload (n_abc >= 1).  The tables cost, per input, 64 x 4
// doublings and 64 x 14 mixed additions and two inversions on one host thread (~1 ms); the key's input count is bounded by memory alone.
inline std::vector<uint32_t> make_key(const uint64_t *alpha_beta, const uint64_t *gamma_g2, const uint64_t *delta_g2, const uint64_t *abc_xy,
                                      const uint8_t *abc_inf, size_t n_abc) {
    std::vector<uint32_t> words(KEY_FIXED_WORDS + (n_abc - 1) * ACC_TABLE_WORDS, 0u);
    for (unsigned k = 0; k < 12; ++k) fq_put(words.data() + k * FQ_WORDS, fq_from_canonical(alpha_beta + 6 * k));
    const uint64_t *g2[2] = {gamma_g2, delta_g2};
    for (int s = 0; s < 2; ++s) {
        const Fq2 x = {fq_from_canonical(g2[s]), fq_from_canonical(g2[s] + 6)}, y = {fq_from_canonical(g2[s] + 12), fq_from_canonical(g2[s] + 18)};
        pairing::prepare_lines(reinterpret_cast<Line *>(words.data() + 144 + s * pairing::PREPARED_LINES * LINE_WORDS), x, y);
    }
    uint32_t *abc0 = words.data() + KEY_FIXED_WORDS - AFFINE_WORDS;
    std::vector<G1Jac> win(ACC_WINDOWS), ent((size_t)ACC_WINDOWS * ACC_ENTRIES);
    std::vector<uint32_t> win_affine(ACC_WINDOWS * AFFINE_WORDS);
    for (size_t j = 0; j < n_abc; ++j) {
        if (abc_inf && abc_inf[j]) continue;  // the words are zero already: infinity, in abc0 and in every table entry
        const Fq x = fq_from_canonical(abc_xy + 12 * j), y = fq_from_canonical(abc_xy + 12 * j + 6);
        if (j == 0) {
            fq_put(abc0, x);
            fq_put(abc0 + FQ_WORDS, y);
            continue;
        }
        win[0] = {x, y, Fq::one()};
        for (int w = 1; w < ACC_WINDOWS; ++w) {
            win[w] = win[w - 1];
            for (int k = 0; k < ACC_WINDOW_BITS; ++k) win[w] = win[w].is_infinity() ? win[w] : g1_dbl(win[w]);
        }
        batch_to_affine(win_affine.data(), win);
        for (int w = 0; w < ACC_WINDOWS; ++w) {
            const uint32_t *b = win_affine.data() + w * AFFINE_WORDS;
            G1Jac e = G1Jac::infinity();
            for (int d = 0; d < ACC_ENTRIES; ++d) {
                if (!affine_is_infinity(b)) e = g1_madd(e, fq_at(b), fq_at(b + FQ_WORDS));
                ent[(size_t)w * ACC_ENTRIES + d] = e;
            }
        }
        batch_to_affine(words.data() + KEY_FIXED_WORDS + (j - 1) * ACC_TABLE_WORDS, ent);
    }
    return words;
}

}  // namespace groth16v
}  // namespace zkhip
