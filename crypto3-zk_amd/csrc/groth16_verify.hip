// Groth16 verification of a batch of proofs on the device, up to and including the final exponentiation (zkhip_groth16_verify_batch;
// conventions: include/zkhip.h, "Groth16 verification"; bodies: groth16_verify.hpp, pairing.hpp, fq12.hpp).  Where the reference checks
// one proof after another on one host thread (systems/ppzksnark/r1cs_gg_ppzksnark/verifier.hpp:150-186), here a lane checks a proof.
// Three launches per call, whatever n is, each of 64-lane workgroups with proof offset + blockIdx.x * 64 + lane in lane `lane`:
//
//   groth16_accumulate   acc = abc[0] + sum_j x_j abc[j + 1] by lookups in the key's fixed-base window tables and mixed additions (no
//                        doublings), then -acc in affine form (one Fermat inversion per lane) into the workspace.
//   groth16_miller3      loads A, B, C from the three bases objects, checks that each lies on its curve, and runs miller_loop3: B is
//                        walked, gamma and delta come as the key's prepared lines (every lane reads the same address: scalar loads), one
//                        squaring of f per step for the three pairs.  f lives in the word-major LDS slot of the pairing kernels (36 KiB
//                        per workgroup); the value goes to the workspace in the same shape, a tile of 64 per workgroup.
//   groth16_final_exp    per lane: final_exponentiation of its value, compared with the key's alpha_beta; writes ok, and the value in
//                        canonical form when the caller asked for it.
// The final exponentiation is a kernel of its own, not the tail of groth16_miller3: its seven live Fq12 temporaries (4 KiB per lane) do
// not fit beside the Miller loop's twist point and line, and apart the two are timed apart ("Groth16 verification").
//
// The key's tables and lines are made on the host at upload (groth16_verify.hpp: make_key) and lie in one device allocation.
#define ZK_NOINLINE_MUL
#include <memory>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "groth16_verify.hpp"
#include "pairing_dev.hpp"

using namespace zkhip;
using namespace zkhip::groth16v;
using namespace zkhip::pairing_dev;

struct zkhip_groth16_vk {
    int device = 0;
    size_t n_abc = 0;
    DevBuf d;  // the words of make_key
};

namespace {

__global__ __launch_bounds__(PAIR_LANES) void groth16_accumulate(const uint32_t *__restrict__ key_words, const uint32_t *__restrict__ inputs, uint32_t n_inputs,
                                                                 size_t n, uint32_t *__restrict__ neg_acc) {
    const size_t i = (size_t)blockIdx.x * PAIR_LANES + threadIdx.x;
    if (i >= n) return;
    const Groth16Key key = key_at(key_words);
    neg_affine(neg_acc + i * AFFINE_WORDS, accumulate(key, inputs + i * n_inputs * 8, n_inputs));
}

__global__ __launch_bounds__(PAIR_LANES) void groth16_miller3(const uint32_t *__restrict__ key_words, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                              const uint32_t *__restrict__ c, const uint32_t *__restrict__ neg_acc, size_t n,
                                                              uint32_t *__restrict__ mill, uint8_t *__restrict__ well_formed) {
    __shared__ uint32_t slots[F12_WORDS * PAIR_LANES];
    const uint32_t lane = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * PAIR_LANES + lane;
    StridedStore fs = {slots + lane};
    if (i < n) {
        const uint32_t *pa = a + i * G1_WORDS, *pb = b + i * G2_WORDS, *pc = c + i * G1_WORDS;
        ProofPoints p;
        p.a_inf = words_all_zero(pa, G1_WORDS), p.b_inf = words_all_zero(pb, G2_WORDS), p.c_inf = words_all_zero(pc, G1_WORDS);
        p.ax = load_coord(pa), p.ay = load_coord(pa + COORD_WORDS);
        p.cx = load_coord(pc), p.cy = load_coord(pc + COORD_WORDS);
        p.bx = {load_coord(pb), load_coord(pb + COORD_WORDS)}, p.by = {load_coord(pb + 2 * COORD_WORDS), load_coord(pb + 3 * COORD_WORDS)};
        well_formed[i] = p.well_formed();
        miller3(fs, key_at(key_words), p, neg_acc + i * AFFINE_WORDS);
    } else {
        fs.store(pairing::Fq12::one());
    }
    // the lane's own slot, word-major, into the tile of the workspace (no other lane touches the slot: no barrier)
    uint32_t *dst = mill + (size_t)blockIdx.x * F12_WORDS * PAIR_LANES + lane;
    for (unsigned k = 0; k < F12_WORDS; ++k) dst[k * PAIR_LANES] = slots[k * PAIR_LANES + lane];
}

__global__ __launch_bounds__(PAIR_LANES) void groth16_final_exp(const uint32_t *__restrict__ key_words, const uint32_t *__restrict__ mill,
                                                                const uint8_t *__restrict__ well_formed, size_t n, uint8_t *__restrict__ ok, uint32_t *__restrict__ gt) {
    const uint32_t lane = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * PAIR_LANES + lane;
    if (i >= n) return;
    const StridedStore src = {const_cast<uint32_t *>(mill) + (size_t)blockIdx.x * F12_WORDS * PAIR_LANES + lane};
    const pairing::Fq12 v = pairing::final_exponentiation(src.load());
    ok[i] = well_formed[i] && equals_alpha_beta(key_at(key_words), v);
    if (gt) fq12_to_canonical(gt + i * F12_WORDS, v);
}

struct VerifyBuffers {  // the per-call workspace, in the order it lies in memory
    size_t n, n_inputs, tiles;
    bool want_gt;
    uint32_t *inputs;    // n x n_inputs x 8: the public inputs, canonical
    uint32_t *neg_acc;   // n x 24: -acc, affine, Montgomery form; all zero = infinity
    uint32_t *mill;      // tiles x 144 x 64: the Miller values, word-major per tile
    uint32_t *gt;        // n x 144: the compared values, canonical (want_gt)
    uint8_t *well_formed, *ok;  // n each
    template <class Arena>
    void layout(Arena &a) {
        a.take(inputs, std::max<size_t>(1, n * n_inputs * 8));
        a.take(neg_acc, n * AFFINE_WORDS);
        a.take(mill, tiles * F12_WORDS * PAIR_LANES);
        a.take(gt, want_gt ? n * F12_WORDS : 1);
        a.take(well_formed, n);
        a.take(ok, n);
    }
};

bool bases_fit(const zkhip_bases *b, int group, unsigned words) { return b->curve == CURVE_BLS12_381 && b->group == group && b->stride_u32 == words; }

}  // namespace

extern "C" {

int zkhip_groth16_vk_upload(zkhip_ctx *ctx, int curve, const uint64_t *alpha_beta, const uint64_t *gamma_g2, const uint64_t *delta_g2, const uint64_t *gamma_abc_xy,
                            const uint8_t *gamma_abc_inf, size_t n_abc, zkhip_groth16_vk **out) {
    ZK_ARGS(ctx, curve);
    if (curve != CURVE_BLS12_381 || !alpha_beta || !gamma_g2 || !delta_g2 || !out || (n_abc && !gamma_abc_xy)) return ZKHIP_ERR_INVALID;
    if (n_abc == 0 || n_abc - 1 > ZKHIP_GROTH16_VK_MAX_INPUTS) return ZKHIP_ERR_RANGE;
    ZK_ENTER(ctx);
    std::unique_ptr<zkhip_groth16_vk> vk(new (std::nothrow) zkhip_groth16_vk);
    if (!vk) return ZKHIP_ERR_OOM;
    vk->device = ctx->device;
    vk->n_abc = n_abc;
    std::vector<uint32_t> words;
    try {  // up to 2.8 GiB of host memory: a failed allocation is the call's error, not an exception across the C ABI
        words = make_key(alpha_beta, gamma_g2, delta_g2, gamma_abc_xy, gamma_abc_inf, n_abc);
    } catch (const std::bad_alloc &) {
        ctx->last_error = "zkhip_groth16_vk_upload: no host memory for the tables of " + std::to_string(n_abc - 1) + " inputs";
        return ZKHIP_ERR_OOM;
    }
    ZK_TRY(vk->d.alloc(ctx, words.size() * 4));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(vk->d, words.data(), words.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *out = vk.release();
    return ZKHIP_OK;
}

size_t zkhip_groth16_vk_inputs(const zkhip_groth16_vk *vk) { return vk ? vk->n_abc - 1 : 0; }

void zkhip_groth16_vk_free(zkhip_ctx *ctx, zkhip_groth16_vk *vk) {
    if (!vk) return;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    delete vk;
}

int zkhip_groth16_verify_batch(zkhip_ctx *ctx, const zkhip_groth16_vk *vk, const zkhip_bases *a, const zkhip_bases *b, const zkhip_bases *c, size_t offset, size_t n,
                               const uint64_t *inputs, size_t n_inputs, uint8_t *ok, uint64_t *out_gt) {
    if (!ctx || !vk || !a || !b || !c || !ok || (n_inputs && !inputs)) return ZKHIP_ERR_INVALID;
    if (!bases_fit(a, GROUP_G1, G1_WORDS) || !bases_fit(b, GROUP_G2, G2_WORDS) || !bases_fit(c, GROUP_G1, G1_WORDS) || vk->device != ctx->device)
        return ZKHIP_ERR_INVALID;
    for (const zkhip_bases *o : {a, b, c})
        if (offset > o->n || n > o->n - offset) return ZKHIP_ERR_RANGE;
    if (n_inputs > vk->n_abc - 1 || n >= ((size_t)1 << 37)) return ZKHIP_ERR_RANGE;  // 2^37: the grid's guard; no bases object is that long
    if (n == 0) return ZKHIP_OK;
    ZK_ENTER(ctx);
    const size_t tiles = (n + PAIR_LANES - 1) / PAIR_LANES;
    VerifyBuffers w = {n, n_inputs, tiles, out_gt != nullptr};
    ZK_TRY(ws_place(ctx, w));
    if (n_inputs) ZK_TRY(ws_upload(ctx, w.inputs, inputs, n * n_inputs * 32));
    const dim3 grid((unsigned)tiles), block(PAIR_LANES);
    // slot 0 of a bases object holds the points themselves, whatever window tables it carries
    ZK_LAUNCH(ctx, "groth16_accumulate", groth16_accumulate, grid, block, 0, vk->d.p, w.inputs, (uint32_t)n_inputs, n, w.neg_acc);
    ZK_LAUNCH(ctx, "groth16_miller3", groth16_miller3, grid, block, 0, vk->d.p, a->d.p + offset * G1_WORDS, b->d.p + offset * G2_WORDS, c->d.p + offset * G1_WORDS,
              w.neg_acc, n, w.mill, w.well_formed);
    ZK_LAUNCH(ctx, "groth16_final_exp", groth16_final_exp, grid, block, 0, vk->d.p, w.mill, w.well_formed, n, w.ok, out_gt ? w.gt : nullptr);
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(ok, w.ok, n, hipMemcpyDeviceToHost, ctx->stream));
    if (out_gt) ZK_HIP_CHECK(ctx, hipMemcpyAsync(out_gt, w.gt, n * F12_WORDS * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ZKHIP_OK;
}

}  // extern "C"
