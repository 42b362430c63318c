// TEST SHIM (never loaded by the product path): runs the __host__ __device__ field / curve / recoding
// code of fp.hpp, fu.hpp, curve.hpp, msm_recode.hpp and glv.hpp on the CPU so the no-GPU test-suite can compare the
// exact device arithmetic against the oracle, and the SHA2-256 core of sha256.hpp (the Merkle kernels' hash) and the proof-of-work
// candidate function of pow.hpp (the grinding kernel's) against hashlib.
// Built with --offload-host-only into libzkhip_hosttest.so.
#include <cstring>
#include <vector>

#define ZK_NOINLINE_MUL 1  // keeps this shim's build time short; fu_sqr is reached through op 9
#include "arith_ops.h"
#include "glv.hpp"
#include "groth16_verify.hpp"
#include "msm_recode.hpp"
#include "ntt_plan.hpp"
#include "pairing.hpp"
#include "pow.hpp"
#include "sha256.hpp"

using namespace zkhip;
using namespace zkhip::arith;

#define FIELD_SWITCH(field, ...)                             \
    switch (field) {                                         \
        case 0: { typedef bls_fq F; __VA_ARGS__; } break;    \
        case 1: { typedef bls_fr F; __VA_ARGS__; } break;    \
        case 2: { typedef bn_fq F; __VA_ARGS__; } break;     \
        case 3: { typedef bn_fr F; __VA_ARGS__; } break;     \
        case 4: { typedef bls_fq2 F; __VA_ARGS__; } break;   \
        case 5: { typedef bn_fq2 F; __VA_ARGS__; } break;    \
        case 6: { typedef bls_fqu F; __VA_ARGS__; } break;   \
        case 7: { typedef bn_fqu F; __VA_ARGS__; } break;    \
        case 8: { typedef bls_fru F; __VA_ARGS__; } break;   \
        case 9: { typedef bn_fru F; __VA_ARGS__; } break;    \
        case 10: { typedef bls_fqu2 F; __VA_ARGS__; } break; \
        case 11: { typedef bn_fqu2 F; __VA_ARGS__; } break;  \
        case 12: { typedef pallas_fq F; __VA_ARGS__; } break; \
        case 13: { typedef pallas_fr F; __VA_ARGS__; } break; \
        case 14: { typedef vesta_fq F; __VA_ARGS__; } break;  \
        case 15: { typedef vesta_fr F; __VA_ARGS__; } break;  \
        case 16: { typedef pallas_fqu F; __VA_ARGS__; } break; \
        case 17: { typedef vesta_fqu F; __VA_ARGS__; } break; \
        case 18: { typedef pallas_fru F; __VA_ARGS__; } break; \
        case 19: { typedef vesta_fru F; __VA_ARGS__; } break; \
        default: return -1;                                  \
    }

extern "C" {

// field: 0 BLS Fq, 1 BLS Fr, 2 BN Fq, 3 BN Fr, 4 BLS Fq2, 5 BN Fq2 (saturated reference types);
//        6 BLS Fq, 7 BN Fq, 8 BLS Fr, 9 BN Fr, 10 BLS Fq2, 11 BN Fq2 (lazy 29-bit-limb compute types);
//        12 Pallas Fq, 13 Pallas Fr, 14 Vesta Fq, 15 Vesta Fr (saturated), 16 Pallas Fq, 17 Vesta Fq, 18 Pallas Fr, 19 Vesta Fr (lazy).
// canonical u32 limbs in and out
int zkt_field_op(int field, int op, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    if (!field_op_valid(op)) return -1;
    FIELD_SWITCH(field, field_op<F>(op, a, b, out); return 0);
    return -1;
}

// raw Fu limbs in and out (arith_ops.h, fu_raw_one): type 6 BLS Fq, 7 BN Fq, 8 BLS Fr, 9 BN Fr, 16 Pallas Fq, 17 Vesta Fq, 18 Pallas Fr, 19 Vesta Fr; a, b, c, d and out hold n cases of
// L u32 limbs each.  The host twin of tests/cpp/arithdev.hip's zkd_fu_raw: the C++ bodies here, the inline-asm products there.
int zkt_fu_raw(int type, int op, size_t n, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out) {
#define FU_RAW(U)                                                                                                       \
    {                                                                                                                   \
        if (!fu_raw_valid<U>(op)) return -1;                                                                            \
        for (size_t i = 0; i < n; ++i) fu_raw_one<U>(op, a + i * U::L, b + i * U::L, c + i * U::L, d + i * U::L, out + i * U::L); \
        return 0;                                                                                                       \
    }
    switch (type) {
        case 6: FU_RAW(BlsFqU)
        case 7: FU_RAW(BnFqU)
        case 8: FU_RAW(BlsFrU)
        case 9: FU_RAW(BnFrU)
        case 16: FU_RAW(PallasFqU)
        case 17: FU_RAW(VestaFqU)
        case 18: FU_RAW(PallasFrU)
        case 19: FU_RAW(VestaFrU)
        default: return -1;
    }
#undef FU_RAW
}

// The radix plan ntt.hip runs a 2^log_m transform with under the options ntt_radix_log = smax (1 .. 10) and ntt_tile_log (ntt_plan.hpp):
// returns the number of passes, sv[i] and log_t[i] (NTT_MAX_PASSES ints each) the stages and the tile width of pass i; -1 for bad arguments
int zkt_ntt_plan(size_t log_m, int smax, int tile_log, int *sv, int *log_t) {
    if (!sv || !log_t || log_m == 0 || log_m > 32 || smax < 1 || smax > 10) return -1;
    const NttPlan pl = ntt_plan(log_m, smax, tile_log);
    for (int i = 0; i < pl.np; ++i) sv[i] = pl.sv[i], log_t[i] = pl.log_t[i];
    return pl.np;
}
// the shape ntt_run_t launches a pass of s stages and a planned tile width with, over `count` polynomials of which pb (1, 2, 4) are wanted
// per workgroup: out = {polynomials per workgroup, log2 of the tile width, bytes of LDS}
int zkt_ntt_launch(int s, int log_t, int pb, size_t count, uint64_t *out) {
    if (!out || s < 1 || s > 10 || log_t < 0 || log_t > 12 || (pb != 1 && pb != 2 && pb != 4) || count == 0) return -1;
    const NttLaunchShape sh = ntt_launch_shape((uint32_t)s, (uint32_t)log_t, pb, count);
    out[0] = (uint64_t)sh.pb, out[1] = sh.log_t, out[2] = sh.lds;
    return 0;
}

// the scalar fields have no curve over them here
static bool is_coord_field(int field) { return !(field == 1 || field == 3 || field == 8 || field == 9 || field == 13 || field == 15 || field == 18 || field == 19); }
// coordinate field id as above (0/2/4/5/12/14 saturated, 6/7/10/11/16/17 lazy)
int zkt_point_chain(int field, const uint32_t *pts, const uint8_t *inf, const uint8_t *neg, size_t n, int mode, uint32_t k,
                    uint32_t *out, uint8_t *out_inf) {
    if (!is_coord_field(field)) return -1;
    FIELD_SWITCH(field, point_chain<F>(pts, inf, neg, n, mode, k, out, out_inf); return 0);
    return -1;
}

// arith_ops.h's parked_affine: the n partial sums of the madd chain, parked and normalised with ONE inversion (curve.hpp: xyzz_park,
// xyzz_parked_to_affine).  layout 0 / 1; out: n canonical affine points, out_inf: n flags.  Coordinate field ids as zkt_point_chain's.
int zkt_parked_affine(int field, const uint32_t *pts, const uint8_t *inf, const uint8_t *neg, size_t n, int layout, uint32_t *out, uint8_t *out_inf) {
    if (!is_coord_field(field) || (layout != 0 && layout != 1)) return -1;
    FIELD_SWITCH(field, std::vector<uint32_t> work(7 * n * FieldOps<F>::WORDS + 1); parked_affine<F>(pts, inf, neg, n, layout, work.data(), out, out_inf); return 0);
    return -1;
}

// digits[w] for one scalar: value = sum_w digit_w * 2^off(w), digit as signed int32 (0 when none); returns the carry
// out of the top window
static int recode_windows(const uint32_t *scalar, MsmWindows win, int32_t *digits) {
    uint32_t carry = 0;
    for (int w = 0; w < win.W; ++w) {
        uint32_t d = msm_recode(scalar, win.off(w), win.width(w), carry);
        if (d == DIG_NONE) digits[w] = 0;
        else {
            int32_t mag = (int32_t)(d & 0x7FFFFFFFu) + 1;
            digits[w] = (d >> 31) ? -mag : mag;
        }
    }
    return (int)carry;
}

// W uniform windows of c bits (off(w) = c w)
int zkt_recode(const uint32_t *scalar, int c, int W, int32_t *digits) { return recode_windows(scalar, msm_make_windows(c * W, W), digits); }

// the recoding msm_digits_only performs: fold to |s| <= (r - 1) / 2, then signed digits over the balanced windows
// MsmWindows{bitlen(r), ceil(bitlen(r) / c)}: value = sum_w digit_w * 2^floor(w * bitlen(r) / W).
// Returns the window count, or -1 if a carry left the top window (must not happen).  curve: 0 BLS12-381, 1 BN254, 2 Pallas, 3 Vesta.
int zkt_recode_folded(int curve, const uint32_t *scalar, int c, int32_t *digits) {
    uint32_t s[8];
    bool flip = false;
    if (fr_sat_dispatch(curve, [&](auto fr) -> int {
            flip = msm_fold_scalar<typename decltype(fr)::type>(scalar, s);
            return 0;
        }) != 0)
        return -1;
    const int tb = curve == CURVE_BN254 ? 254 : 255, W = msm_windows(tb, c);
    if (recode_windows(s, msm_make_windows(tb, W), digits) != 0) return -1;
    if (flip)
        for (int w = 0; w < W; ++w) digits[w] = -digits[w];
    return W;
}

// SHA2-256 of n >= 1 field elements (canonical little-endian limbs, hashed as their 32-byte big-endian encodings): merkle.hip's leaf digest
int zkt_sha256_elements(const uint64_t *elems, size_t n, uint8_t *digest) {
    if (!elems || !digest || n == 0) return -1;
    sha256::hash_elements(elems, n, digest);
    return 0;
}

// the whole tree over n_leaves x per_leaf elements, as zkhip_merkle_build_dev lays it out: (2 n_leaves - 1) x 32 bytes, leaf digests first, root last
int zkt_merkle_tree(const uint64_t *leaves, size_t n_leaves, size_t per_leaf, uint8_t *digests) {
    if (!leaves || !digests || n_leaves == 0 || (n_leaves & (n_leaves - 1)) || per_leaf == 0) return -1;
    for (size_t x = 0; x < n_leaves; ++x) sha256::hash_elements(leaves + 4 * x * per_leaf, per_leaf, digests + 32 * x);
    uint8_t *level = digests;
    for (size_t n = n_leaves / 2; n >= 1; n /= 2) {
        uint8_t *up = level + 64 * n;
        for (size_t j = 0; j < n; ++j) sha256::hash_node(level + 64 * j, level + 64 * j + 32, up + 32 * j);
        level = up;
    }
    return 0;
}

// candidate(state, nonce) of the proof of work (pow.hpp): the low 32 bits of SHA256(SHA256(state || be32(nonce))) as a big-endian integer
uint32_t zkt_pow_candidate(const uint8_t *state, uint32_t nonce) { return pow::candidate(pow::prepare(state), nonce); }

// the reference's grinding loop on one host thread: the first nonce start + k, k < max_tries (0: the whole 2^32 space), the mask accepts.
// 0 with *nonce and *tried = k + 1; 1 with *tried = max_tries when there is none; -1 for bad arguments
int zkt_pow_grind_cpu(const uint8_t *state, uint32_t start, uint32_t mask, uint64_t max_tries, uint32_t *nonce, uint64_t *tried) {
    if (!state || !nonce || !tried || max_tries > ((uint64_t)1 << 32)) return -1;
    const uint64_t total = max_tries ? max_tries : (uint64_t)1 << 32, k = pow::first_hit(pow::prepare(state), start, mask, total);
    *tried = k < total ? k + 1 : total;
    if (k == total) return 1;
    *nonce = start + (uint32_t)k;
    return 0;
}

// The GLV split of the EC-NTT's twiddle records (glv.hpp), curve 0 BLS12-381, 1 BN254, 2 Pallas, 3 Vesta: k (8 words, below r) -> the
// magnitudes of k1 and k2 (6 words each) and *signs (bit h: half h is negative).
int zkt_glv_split(int curve, const uint32_t *k, uint32_t *k1, uint32_t *k2, uint32_t *signs) {
    if (!k || !k1 || !k2 || !signs) return -1;
    return g1_dispatch(curve, [&](auto c) -> int { *signs = glv_split<typename decltype(c)::Glv>(k, k1, k2); return 0; }) == 0 ? 0 : -1;
}
// the constants the split and the ladder were compiled with: g1, g2, a1, a2, b1, b2 (5 words each, magnitudes), then beta (12 words, canonical)
int zkt_glv_consts(int curve, uint32_t *out42) {
    if (!out42) return -1;
    return g1_dispatch(curve, [&](auto c) -> int {
        using G = typename decltype(c)::Glv;
        for (int i = 0; i < 5; ++i) {
            out42[i] = G::g1(i), out42[5 + i] = G::g2(i), out42[10 + i] = G::a1(i);
            out42[15 + i] = G::a2(i), out42[20 + i] = G::b1(i), out42[25 + i] = G::b2(i);
        }
        for (int i = 0; i < 12; ++i) out42[30 + i] = i < G::BETA_WORDS ? G::beta(i) : 0;
        return 0;
    }) == 0 ? 0 : -1;
}

// The window record the scaling ladder reads (glv.hpp: scalar_record) of ANY 8-word scalar, as ecntt.hip's scale_records_from_scalars builds it: the
// scalar reduced mod r (fu_reduce; k_out, 8 words), then -- glv != 0 -- split by the curve's endomorphism and recoded into 33 signed nibbles per half,
// or -- glv = 0, the G2 ladder -- recoded into 65 signed nibbles.  rec: REC_WORDS words.
int zkt_scale_record(int curve, int glv, const uint32_t *scalar, uint32_t *k_out, uint32_t *rec) {
    if (!scalar || !k_out || !rec) return -1;
    return g1_dispatch(curve, [&](auto c) -> int {
        using C = decltype(c);
        fu_pack<typename C::U>(k_out, fu_reduce(fu_unpack<typename C::U>(scalar)));
        if (glv) scalar_record<typename C::Glv>(rec, k_out);
        else scalar_record<NoGlv>(rec, k_out);
        return 0;
    }) == 0 ? 0 : -1;
}

// SHA2-256 of a byte string: what zkhip_sha256_host computes
int zkt_sha256_bytes(const uint8_t *msg, size_t len, uint8_t *digest) {
    if (!digest || (!msg && len)) return -1;
    pow::hash_bytes(msg, len, digest);
    return 0;
}

// Fq12 tower (fq12.hpp) on canonical limbs (72 u64 = 144 u32 per element).  op: 0 a * b, 1 a^2, 2 1 / a, 3 a^p (Frobenius), 4 conjugate,
// 5 a * (l0 + l1 v + l4 v w) with the three Fq2 values l0, l1, l4 in b (72 u32), 6 final exponentiation, 7 cyclotomic squaring (the square
// of a only where a^(p^6 + 1) = 1)
int zkt_fq12_op(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    if (!a || !out || ((op == 0 || op == 5) && !b)) return -1;
    const bls_fq12 x = fq12_from_canonical<BlsFq>(a);
    bls_fq12 r;
    switch (op) {
    case 0: r = x * fq12_from_canonical<BlsFq>(b); break;
    case 1: r = fp_sqr(x); break;
    case 2: r = fp_inv(x); break;
    case 3: r = fq12_frobenius(x); break;
    case 4: r = fq12_conj(x); break;
    case 5: {
        bls_fq2 l[3];
        for (int k = 0; k < 3; ++k) {
            bls_fq2 c;
            for (int i = 0; i < 12; ++i) c.c0.v[i] = b[k * 24 + i], c.c1.v[i] = b[k * 24 + 12 + i];
            l[k] = fp_to_mont(c);
        }
        r = fq12_mul_by_014(x, l[0], l[1], l[2]);
        break;
    }
    case 6: r = pairing::final_exponentiation(x); break;
    case 7: r = fq12_cyclotomic_sqr(x); break;
    default: return -1;
    }
    fq12_to_canonical(out, r);
    return 0;
}

// zkhip_pairing_products on the CPU: the same pairing.hpp bodies over canonical affine points (G1: 24 u32, G2: 48 u32 per point)
// with infinity flags; term t covers pairs [start[t], start[t] + n[t]) of both arrays and is multiplied into output out[t].
// Unlike the entry, a term indexes BOTH arrays from the same start, so this twin says nothing about the entry's separate offsets (the structured
// expectation of tests/test_gpu_pairing.py covers those); like the entry, it checks neither that a point is on its curve nor in the order-r subgroup.
int zkt_pairing_products(const uint32_t *g1, const uint8_t *g1_inf, const uint32_t *g2, const uint8_t *g2_inf, const uint64_t *start, const uint64_t *n,
                         const uint32_t *out, size_t n_terms, size_t n_out, uint32_t *out_gt) {
    if (!g1 || !g1_inf || !g2 || !g2_inf || !start || !n || !out || !out_gt || n_out == 0) return -1;
    std::vector<bls_fq12> acc(n_out, bls_fq12::one());
    for (size_t t = 0; t < n_terms; ++t) {
        if (out[t] >= n_out) return -2;
        for (uint64_t i = start[t]; i < start[t] + n[t]; ++i) {
            if (g1_inf[i] || g2_inf[i]) continue;
            bls_fq c[6];
            for (int k = 0; k < 6; ++k) {
                const uint32_t *src = k < 2 ? g1 + i * 24 + k * 12 : g2 + i * 48 + (k - 2) * 12;
                bls_fq v;
                for (int j = 0; j < 12; ++j) v.v[j] = src[j];
                c[k] = fp_to_mont(v);
            }
            pairing::RegStore fs;
            pairing::miller_loop(fs, c[0], c[1], bls_fq2{c[2], c[3]}, bls_fq2{c[4], c[5]});
            acc[out[t]] = acc[out[t]] * fs.f;
        }
    }
    for (size_t k = 0; k < n_out; ++k) fq12_to_canonical(out_gt + k * 144, pairing::final_exponentiation(acc[k]));
    return 0;
}

// zkhip_groth16_verify_batch on the CPU: the same groth16_verify.hpp / pairing.hpp bodies (make_key, accumulate, miller_loop3 over the prepared
// lines, final_exponentiation, the comparison).  The key as zkhip_groth16_vk_upload takes it; a, c: n canonical affine G1 points (24 u32), b: G2
// (48 u32), with infinity flags; inputs: n x n_inputs scalars of 8 u32.  out_gt (n x 144 u32) and out_neg_acc (n x 24 u32: -acc, canonical, all
// zero = infinity) are nullable.
int zkt_groth16_verify(const uint64_t *alpha_beta, const uint64_t *gamma_g2, const uint64_t *delta_g2, const uint64_t *abc_xy, const uint8_t *abc_inf, size_t n_abc,
                       const uint32_t *a, const uint8_t *a_inf, const uint32_t *b, const uint8_t *b_inf, const uint32_t *c, const uint8_t *c_inf, size_t n,
                       const uint32_t *inputs, size_t n_inputs, uint8_t *ok, uint32_t *out_gt, uint32_t *out_neg_acc) {
    using namespace groth16v;
    if (!alpha_beta || !gamma_g2 || !delta_g2 || !abc_xy || n_abc == 0 || !a || !a_inf || !b || !b_inf || !c || !c_inf || !ok || (n_inputs && !inputs)) return -1;
    if (n_inputs > n_abc - 1) return -2;
    const std::vector<uint32_t> words = make_key(alpha_beta, gamma_g2, delta_g2, abc_xy, abc_inf, n_abc);
    const Groth16Key key = key_at(words.data());
    const auto coord = [](const uint32_t *p) {
        bls_fq v;
        for (int j = 0; j < 12; ++j) v.v[j] = p[j];
        return fp_to_mont(v);
    };
    for (size_t i = 0; i < n; ++i) {
        uint32_t neg_acc[AFFINE_WORDS];
        neg_affine(neg_acc, accumulate(key, inputs + i * n_inputs * 8, n_inputs));
        if (out_neg_acc)
            for (int k = 0; k < 2; ++k) {
                const bls_fq v = fp_from_mont(fq_at(neg_acc + k * FQ_WORDS));
                for (int j = 0; j < 12; ++j) out_neg_acc[i * 24 + k * 12 + j] = v.v[j];
            }
        ProofPoints p;
        p.a_inf = a_inf[i], p.b_inf = b_inf[i], p.c_inf = c_inf[i];
        p.ax = coord(a + i * 24), p.ay = coord(a + i * 24 + 12);
        p.cx = coord(c + i * 24), p.cy = coord(c + i * 24 + 12);
        p.bx = {coord(b + i * 48), coord(b + i * 48 + 12)}, p.by = {coord(b + i * 48 + 24), coord(b + i * 48 + 36)};
        pairing::RegStore fs;
        miller3(fs, key, p, neg_acc);
        const bls_fq12 v = pairing::final_exponentiation(fs.f);
        ok[i] = p.well_formed() && equals_alpha_beta(key, v);
        if (out_gt) fq12_to_canonical(out_gt + i * 144, v);
    }
    return 0;
}

}  // extern "C"
