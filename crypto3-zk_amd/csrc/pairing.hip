// Inner pairing products on the device: out[k] = final_exponentiation(prod miller(P_i, Q_i)) over the pairs of the terms that name output k
// (zkhip_pairing_products; conventions: include/zkhip.h, "Pairing products").  The commitments and GIPA rounds of the reference's Groth16
// aggregation are such products (commitments/polynomial/kzg_ipp2.hpp:216-283, systems/.../ipp2/prover.hpp:360-381, 584-593), where the
// reference runs one pairing after another on one host thread.
//
//   pairing_miller           one pair per lane, 64-lane workgroups.  The running value f (12 Fq = 144 words) lives in LDS, one word-major slot per
//                            lane (word k of lane l at k * 64 + l: a wave's access to one word covers the 64 banks once), the running twist
//                            point, the two input points and the line in registers.  36 KiB of LDS per workgroup: four workgroups per CU,
//                            one wave per SIMD, which is also what the register budget of the Fq12 squaring allows.  A lane past
//                            its term's end, or whose pair holds a point at infinity, leaves one.  Values go to the workspace in the same
//                            word-major shape, a tile of 64 per workgroup.
//   pairing_product_blocks   a workgroup takes PROD_TILES consecutive tiles of ONE term: lane l multiplies the l-th values of its tiles in
//                            order, then the 64 lanes multiply in a fixed tree through LDS.  One partial product per workgroup, with the
//                            output it belongs to.
//   pairing_product_final    one workgroup: per output, lane l multiplies the partials l, l + 64, ... of that output, then the same tree.
// No atomics anywhere: the order of every multiplication is fixed by the term list alone.
//
// The final exponentiation runs on the host, once per output, on the n_out x 576 bytes copied back: ~10^4 strictly dependent Fq products
// by the same pairing.hpp body.  Nothing proportional to the pair count runs on the host (the term table is one small upload).
#define ZK_NOINLINE_MUL
#include <vector>

#include "ctx.hpp"
#include "pairing_dev.hpp"

using namespace zkhip;
using namespace zkhip::pairing_dev;
using pairing::Fq;
using pairing::Fq12;
using pairing::Fq2;

namespace {

constexpr unsigned PROD_TILES = 16;    // Miller tiles (of 64 values) per workgroup of pairing_product_blocks

struct PairingTerm {  // device copy of a zkhip_pairing_term
    const uint32_t *g1, *g2;  // first point of the term (affine, lazy Montgomery form, all words zero = infinity)
    uint64_t n;
    uint32_t out;
    uint32_t tile_start, tiles;    // its Miller workgroups: ceil(n / 64) from tile_start
    uint32_t block_start;          // its product workgroups: ceil(tiles / PROD_TILES) from block_start
};

// the term a workgroup index belongs to, by its `start` / `count` members.  A linear walk of the term table by every workgroup: priced for the
// two to four terms of a commitment or a GIPA round (zkhip.h says so); a caller with thousands of small terms pays O(n_terms) per workgroup.
template <uint32_t PairingTerm::*Start, class Count>
ZK_D uint32_t find_term(const PairingTerm *terms, uint32_t n_terms, uint32_t idx, Count count) {
    uint32_t t = 0;
    while (t + 1 < n_terms && idx >= terms[t].*Start + count(terms[t])) ++t;
    return t;
}

__global__ __launch_bounds__(PAIR_LANES) void pairing_miller(const PairingTerm *__restrict__ terms, uint32_t n_terms, uint32_t *__restrict__ mill) {
    __shared__ uint32_t slots[F12_WORDS * PAIR_LANES];
    const uint32_t lane = threadIdx.x, tile = blockIdx.x;
    const PairingTerm tm = terms[find_term<&PairingTerm::tile_start>(terms, n_terms, tile, [](const PairingTerm &t) { return t.tiles; })];
    const uint64_t i = (uint64_t)(tile - tm.tile_start) * PAIR_LANES + lane;
    StridedStore fs = {slots + lane};
    bool live = i < tm.n;
    if (live) {
        const uint32_t *p = tm.g1 + i * G1_WORDS, *q = tm.g2 + i * G2_WORDS;
        live = !words_all_zero(p, G1_WORDS) && !words_all_zero(q, G2_WORDS);
        if (live) {
            const Fq xp = load_coord(p), yp = load_coord(p + COORD_WORDS);
            const Fq2 xq = {load_coord(q), load_coord(q + COORD_WORDS)}, yq = {load_coord(q + 2 * COORD_WORDS), load_coord(q + 3 * COORD_WORDS)};
            pairing::miller_loop(fs, xp, yp, xq, yq);
        }
    }
    if (!live) fs.store(Fq12::one());
    // the lane's own slot, word-major, into the tile of the workspace (no other lane touches the slot: no barrier)
    uint32_t *dst = mill + (size_t)tile * F12_WORDS * PAIR_LANES + lane;
    for (unsigned k = 0; k < F12_WORDS; ++k) dst[k * PAIR_LANES] = slots[k * PAIR_LANES + lane];
}

// the product of the 64 lanes' values, in lane 0: a fixed tree through LDS
ZK_D Fq12 workgroup_product(uint32_t *slots, Fq12 f) {
    const uint32_t lane = threadIdx.x;
    StridedStore mine = {slots + lane};
    mine.store(f);
    for (unsigned s = PAIR_LANES / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (lane < s) {
            const StridedStore other = {slots + lane + s};
            f = f * other.load();
            mine.store(f);
        }
    }
    return f;
}

__global__ __launch_bounds__(PAIR_LANES) void pairing_product_blocks(const PairingTerm *__restrict__ terms, uint32_t n_terms, const uint32_t *__restrict__ mill,
                                                                     uint32_t *__restrict__ part, uint32_t *__restrict__ part_out) {
    __shared__ uint32_t slots[F12_WORDS * PAIR_LANES];
    const uint32_t lane = threadIdx.x, block = blockIdx.x;
    const PairingTerm tm =
        terms[find_term<&PairingTerm::block_start>(terms, n_terms, block, [](const PairingTerm &t) { return (t.tiles + PROD_TILES - 1) / PROD_TILES; })];
    const uint32_t first = (block - tm.block_start) * PROD_TILES;
    const uint32_t last = first + PROD_TILES < tm.tiles ? first + PROD_TILES : tm.tiles;
    Fq12 f = Fq12::one();
    for (uint32_t t = first; t < last; ++t) {
        const StridedStore v = {const_cast<uint32_t *>(mill) + (size_t)(tm.tile_start + t) * F12_WORDS * PAIR_LANES + lane};
        f = f * v.load();
    }
    f = workgroup_product(slots, f);
    if (lane == 0) {
        uint32_t *dst = part + (size_t)block * F12_WORDS;
        const uint32_t *w = reinterpret_cast<const uint32_t *>(&f);
        for (unsigned k = 0; k < F12_WORDS; ++k) dst[k] = w[k];
        part_out[block] = tm.out;
    }
}

__global__ __launch_bounds__(PAIR_LANES) void pairing_product_final(const uint32_t *__restrict__ part, const uint32_t *__restrict__ part_out, uint32_t n_part,
                                                                    uint32_t n_out, uint32_t *__restrict__ out) {
    __shared__ uint32_t slots[F12_WORDS * PAIR_LANES];
    const uint32_t lane = threadIdx.x;
    for (uint32_t k = 0; k < n_out; ++k) {
        Fq12 f = Fq12::one();
        for (uint32_t j = lane; j < n_part; j += PAIR_LANES) {
            if (part_out[j] != k) continue;
            Fq12 v;
            uint32_t *w = reinterpret_cast<uint32_t *>(&v);
            const uint32_t *src = part + (size_t)j * F12_WORDS;
            for (unsigned i = 0; i < F12_WORDS; ++i) w[i] = src[i];
            f = f * v;
        }
        f = workgroup_product(slots, f);
        if (lane == 0) {
            uint32_t *dst = out + (size_t)k * F12_WORDS;
            const uint32_t *w = reinterpret_cast<const uint32_t *>(&f);
            for (unsigned i = 0; i < F12_WORDS; ++i) dst[i] = w[i];
        }
        __syncthreads();  // the slots are rewritten for the next output
    }
}

struct PairingBuffers {  // the per-call workspace, in the order it lies in memory
    size_t n_terms, tiles, blocks, n_out;
    PairingTerm *terms;
    uint32_t *mill;      // tiles x 144 x 64: the Miller values, word-major per tile
    uint32_t *part;      // blocks x 144: one partial product per workgroup of pairing_product_blocks
    uint32_t *part_out;  // blocks: the output each partial belongs to
    uint32_t *out;       // n_out x 144: the products, Montgomery form
    template <class Arena>
    void layout(Arena &a) {
        a.take(terms, std::max<size_t>(1, n_terms));
        a.take(mill, std::max<size_t>(1, tiles) * F12_WORDS * PAIR_LANES);
        a.take(part, std::max<size_t>(1, blocks) * F12_WORDS);
        a.take(part_out, std::max<size_t>(1, blocks));
        a.take(out, n_out * F12_WORDS);
    }
};

}  // namespace

extern "C" {

int zkhip_pairing_products(zkhip_ctx *ctx, int curve, const zkhip_pairing_term *terms, size_t n_terms, size_t n_out, uint64_t *out_gt) {
    ZK_ARGS(ctx, curve);
    if (curve != CURVE_BLS12_381 || !out_gt || (n_terms && !terms)) return ZKHIP_ERR_INVALID;
    for (size_t t = 0; t < n_terms; ++t) {
        const zkhip_pairing_term &tm = terms[t];
        if (!tm.g1 || !tm.g2 || tm.g1->curve != curve || tm.g2->curve != curve || tm.g1->group != GROUP_G1 || tm.g2->group != GROUP_G2 ||
            tm.g1->stride_u32 != G1_WORDS || tm.g2->stride_u32 != G2_WORDS)  // the kernel reads the lazy form of BLS12-381's bases
            return ZKHIP_ERR_INVALID;
    }
    if (n_out == 0 || n_out > 0xFFFFFFFFu || n_terms > 0xFFFFFFFFu) return ZKHIP_ERR_RANGE;
    std::vector<PairingTerm> dev(n_terms);
    size_t tiles = 0, blocks = 0;
    for (size_t t = 0; t < n_terms; ++t) {
        const zkhip_pairing_term &tm = terms[t];
        if (tm.g1_offset > tm.g1->n || tm.n > tm.g1->n - tm.g1_offset || tm.g2_offset > tm.g2->n || tm.n > tm.g2->n - tm.g2_offset || tm.out >= n_out)
            return ZKHIP_ERR_RANGE;
        const size_t nt = (tm.n + PAIR_LANES - 1) / PAIR_LANES;
        if (tiles + nt >= ((size_t)1 << 31)) return ZKHIP_ERR_RANGE;
        // slot 0 of a bases object holds the points themselves, whatever window tables it carries
        dev[t] = {tm.g1->d.p + tm.g1_offset * tm.g1->stride_u32, tm.g2->d.p + tm.g2_offset * tm.g2->stride_u32, tm.n, tm.out, (uint32_t)tiles, (uint32_t)nt,
                  (uint32_t)blocks};
        tiles += nt;
        blocks += (nt + PROD_TILES - 1) / PROD_TILES;
    }
    ZK_ENTER(ctx);
    PairingBuffers w = {n_terms, tiles, blocks, n_out};
    ZK_TRY(ws_place(ctx, w));
    if (n_terms) ZK_TRY(ws_upload(ctx, w.terms, dev.data(), n_terms * sizeof(PairingTerm)));
    if (tiles) {
        ZK_LAUNCH(ctx, "pairing_miller", pairing_miller, dim3((unsigned)tiles), dim3(PAIR_LANES), 0, w.terms, (uint32_t)n_terms, w.mill);
        ZK_LAUNCH(ctx, "pairing_product_blocks", pairing_product_blocks, dim3((unsigned)blocks), dim3(PAIR_LANES), 0, w.terms, (uint32_t)n_terms, w.mill, w.part,
                  w.part_out);
    }
    ZK_LAUNCH(ctx, "pairing_product_final", pairing_product_final, dim3(1), dim3(PAIR_LANES), 0, w.part, w.part_out, (uint32_t)blocks, (uint32_t)n_out, w.out);
    std::vector<Fq12> host(n_out);
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(host.data(), w.out, n_out * sizeof(Fq12), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; k < n_out; ++k) fq12_to_canonical(reinterpret_cast<uint32_t *>(out_gt + k * 72), pairing::final_exponentiation(host[k]));
    return ZKHIP_OK;
}

}  // extern "C"
