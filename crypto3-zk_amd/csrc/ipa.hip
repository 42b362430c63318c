// Primitives of the Pedersen / inner-product-argument polynomial commitment (zk/commitments/polynomial/kimchi_pedersen.hpp) that the MSM
// and polynomial layers do not already offer ("inner-product argument" of include/zkhip.h):
//
//   zkhip_bases_fold                g = g_high * u + g_low, the generator fold of proof_eval (:524-534): one variable-base scalar
//                                   multiplication by the SAME scalar and one mixed addition per point               <- the hot kernel
//   zkhip_fr_inner_product_dev      algebra::inner_product over two resident vectors (:472-475, :500-506)
//   zkhip_fr_powers_lincomb_dev     b[i] = sum_e scale_e * point_e^i, the evaluation-point vector of proof_eval (:460-470)
//   zkhip_fr_challenge_products_dev b_poly_coefficents (:629-643)
//
// Scalars in HBM are canonical 8-word integers (fu.hpp: fu_mul(plain, Montgomery) is the plain product); points are the bases objects'
// Montgomery affine form.
#include <algorithm>
#include <memory>

#include "ctx.hpp"
#include "curve.hpp"
#include "field_consts.hpp"
#include "fu.hpp"

using namespace zkhip;

namespace {

// ---- the generator fold ---------------------------------------------------------------------------------------------------------------
// The scalar of a fold, recoded once on the host and passed by value: its words and the index of its top set bit (-1: the scalar is zero).
// Every lane multiplies by the same scalar, so the double-and-add schedule is uniform over the wave: no lane waits for another's addition.
struct FoldScalar {
    uint32_t w[8];
    int top;
};
// word i of the scalar without indexing the argument dynamically (which would move it to scratch): a chain of uniform selects
ZK_D uint32_t fold_word(const FoldScalar &c, int i) {
    uint32_t v = c.w[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) v = i == k ? c.w[k] : v;
    return v;
}

// out[i] = c * hi[i] + lo[i].  A lane takes `chunk` consecutive points (affine_chunk): double-and-add from the top bit over the affine hi point,
// a mixed addition of lo (complete: doubling, cancellation and either operand at infinity), the XYZZ sums parked in `tmp` (5 field elements
// per entry: X, Y, ZZ, ZZZ, prefix product) and ONE inversion for the chunk (curve.hpp: xyzz_parked_to_affine).
template <class F>
__global__ __launch_bounds__(64) void ipa_bases_fold(const uint32_t *__restrict__ lo_pts, const uint32_t *__restrict__ hi_pts, uint32_t half, uint32_t chunk,
                                                     FoldScalar c, uint32_t *__restrict__ out, uint32_t *__restrict__ tmp) {
    typedef FieldOps<F> O;
    constexpr int NL = O::WORDS;
    const size_t first = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * chunk;
    if (first >= half) return;
    const uint32_t cnt = half - first < chunk ? (uint32_t)(half - first) : chunk;
    F pre = F::one();
    for (uint32_t k = 0; k < cnt; ++k) {
        const size_t i = first + k;
        const Affine<F> h = affine_load<F>(hi_pts + i * (2 * NL));
        XYZZ<F> acc = c.top >= 0 ? XYZZ<F>::from_affine(h) : XYZZ<F>::infinity();
        uint32_t word = c.top >= 0 ? fold_word(c, c.top >> 5) : 0;
        for (int b = c.top - 1; b >= 0; --b) {
            if ((b & 31) == 31) word = fold_word(c, b >> 5);
            acc = xyzz_dbl(acc);
            if ((word >> (b & 31)) & 1) acc = xyzz_madd(acc, h);
        }
        acc = xyzz_madd(acc, affine_load<F>(lo_pts + i * (2 * NL)));
        uint32_t *slot = tmp + i * (5 * NL);
        xyzz_park(slot, slot + 4 * NL, acc, pre);
    }
    xyzz_parked_to_affine(
        pre, cnt, [&](uint32_t k) { return tmp + (first + k) * (5 * NL); }, [&](uint32_t k) { return tmp + (first + k) * (5 * NL) + 4 * NL; },
        [&](uint32_t k) { return out + (first + k) * (2 * NL); });
}

// ---- scalar-field kernels -------------------------------------------------------------------------------------------------------------
constexpr uint32_t IP_THREADS = 256, IP_MAX_BLOCKS = 1024;

// The sum of one value per lane over the workgroup, in a fixed order: down the wave by lane shuffles, the waves' sums through LDS, added up
// by lane 0 (which alone holds the result).  Every lane of the workgroup calls it.
template <class U>
ZK_D Fu<U> ip_block_sum(Fu<U> v, uint32_t *lds) {
    constexpr int L = U::L;
    for (int off = 32; off > 0; off >>= 1) {
        Fu<U> o;
#pragma unroll
        for (int l = 0; l < L; ++l) o.v[l] = (uint32_t)__shfl_down((int)v.v[l], off, 64);
        v = fu_addm(v, o);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) fu_store<U>(lds + (size_t)wave * U::SL, v);
    __syncthreads();
    if (threadIdx.x == 0)
        for (uint32_t w = 1; w < IP_THREADS / 64; ++w) v = fu_addm(v, fu_load<U>(lds + (size_t)w * U::SL));
    return v;
}

// part[block] = sum over the workgroup's grid-strided elements of a[i] b[i] / R (canonical representative, limb form)
template <class U>
__global__ __launch_bounds__(IP_THREADS) void ipa_inner_product_blocks(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, size_t n,
                                                                       uint32_t *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[(IP_THREADS / 64) * U::SL];
    Fu<U> acc = Fu<U>::zero();
    for (size_t i = (size_t)blockIdx.x * IP_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * IP_THREADS)
        acc = fu_addm(acc, fu_mulm(fu_unpack<U>(a + i * U::NL), fu_unpack<U>(b + i * U::NL)));
    acc = ip_block_sum<U>(acc, lds);
    if (threadIdx.x == 0) fu_store<U>(part + (size_t)blockIdx.x * U::SL, acc);
}

// out = R^2 / R * sum of the partials = sum a[i] b[i], one canonical element; a single workgroup
template <class U>
__global__ __launch_bounds__(IP_THREADS) void ipa_inner_product_final(const uint32_t *__restrict__ part, uint32_t nparts, uint32_t *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[(IP_THREADS / 64) * U::SL];
    Fu<U> acc = Fu<U>::zero();
    for (uint32_t i = threadIdx.x; i < nparts; i += IP_THREADS) acc = fu_addm(acc, fu_load<U>(part + (size_t)i * U::SL));
    acc = ip_block_sum<U>(acc, lds);
    if (threadIdx.x == 0) fu_pack<U>(out, fu_mulm(acc, Fu<U>::r2()));
}

constexpr uint32_t POWERS_CHUNK = 32;  // consecutive exponents per lane: one power by square-and-multiply, then a running product

// out[i] = sum_e scales[e] * points[e]^i.  pts: points then scales, canonical.  A lane walks its exponents once per point and adds into what
// the points before left there (its own elements: no other lane touches them).
template <class U>
__global__ __launch_bounds__(256) void ipa_powers_lincomb(const uint32_t *__restrict__ pts, uint32_t npoints, size_t n, uint32_t *__restrict__ out) {
    const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * POWERS_CHUNK;
    if (i0 >= n) return;
    const size_t hi = n - i0 < POWERS_CHUNK ? n : i0 + POWERS_CHUNK;
    for (uint32_t e = 0; e < npoints; ++e) {
        const Fu<U> x = fu_cond_sub_p(fu_from_canonical<U>(pts + (size_t)e * U::NL));  // Montgomery
        Fu<U> pw = fu_pow_onto(fu_unpack<U>(pts + (size_t)(npoints + e) * U::NL), x, i0);  // plain: scale * x^i0
        for (size_t i = i0; i < hi; ++i) {
            Fu<U> v = fu_cond_sub_p(pw);
            if (e) v = fu_addm(v, fu_unpack<U>(out + i * U::NL));
            fu_pack<U>(out + i * U::NL, v);
            pw = fu_mul(pw, x);
        }
    }
}

// out[i] = prod over the set bits t of i of chal[rounds - 1 - t], i < 2^rounds; chal in Montgomery form
template <class U>
__global__ __launch_bounds__(256) void ipa_challenge_products(const uint32_t *__restrict__ chal, uint32_t rounds, uint32_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >> rounds) return;
    Fu<U> acc = Fu<U>::plain_one();  // products with Montgomery factors stay plain
    for (uint32_t t = 0; t < rounds; ++t)
        if ((i >> t) & 1) acc = fu_mul(acc, fu_load<U>(chal + (size_t)(rounds - 1 - t) * U::SL));
    fu_pack<U>(out + i * U::NL, fu_cond_sub_p(acc));
}

struct PowersBuffers {  // zkhip_fr_powers_lincomb_dev: the points, then the scales, as uploaded
    size_t npoints;
    uint32_t *pts;
    template <class Arena>
    void layout(Arena &a) { a.take(pts, 2 * npoints * 8); }
};
struct ChallengeBuffers {  // zkhip_fr_challenge_products_dev: the challenges as uploaded and in Montgomery form (16-word slots)
    size_t rounds;
    uint32_t *c, *m;
    template <class Arena>
    void layout(Arena &a) {
        a.take(c, rounds * 8);
        a.take(m, rounds * 16);
    }
};

}  // namespace

bool zk_fr_canonical(int curve, const uint64_t *c) {
    return fr_sat_dispatch(curve, [&](auto fr) -> int {
               using P = typename decltype(fr)::type;
               for (int j = 3; j >= 0; --j) {
                   const uint64_t m = (uint64_t)P::mod(2 * j) | ((uint64_t)P::mod(2 * j + 1) << 32);
                   if (c[j] != m) return c[j] < m ? 1 : 0;
               }
               return 0;
           }) == 1;
}

extern "C" {

int zkhip_bases_fold(zkhip_ctx *ctx, const zkhip_bases *b, size_t offset_lo, size_t offset_hi, size_t half, const uint64_t *c, zkhip_bases **out) {
    if (!b || !c || !out) return ZKHIP_ERR_INVALID;
    ZK_ARGS(ctx, b->curve);
    *out = nullptr;
    if (b->group != GROUP_G1 || !zk_fr_canonical(b->curve, c)) return ZKHIP_ERR_INVALID;
    if (offset_lo > b->n || half > b->n - offset_lo || offset_hi > b->n || half > b->n - offset_hi || half >= ((size_t)1 << 31)) return ZKHIP_ERR_RANGE;
    ZK_ENTER(ctx);
    // the result: the points alone (slot 0), no window tables -- it feeds two MSMs and the next fold
    std::unique_ptr<zkhip_bases> r(new zkhip_bases());
    r->curve = b->curve;
    r->group = b->group;
    r->n = half;
    r->stride_u32 = b->stride_u32;
    ZK_TRY(r->d.alloc(ctx, std::max<size_t>(1, half) * r->stride_u32 * 4));
    if (half) {
        FoldScalar s;
        memcpy(s.w, c, 32);
        s.top = -1;
        for (int i = 255; i >= 0 && s.top < 0; --i)
            if ((s.w[i >> 5] >> (i & 31)) & 1) s.top = i;
        const uint32_t chunk = affine_chunk(half);
        WsOne<uint32_t> w = {half * 5 * r->stride_u32 / 2};
        ZK_TRY(ws_place(ctx, w));
        const uint32_t *pts = b->d;  // slot 0: the points themselves, whatever tables the object carries
        ZK_TRY(g1_dispatch(b->curve, [&](auto g) -> int {
            using F = typename decltype(g)::F;
            ZK_LAUNCH(ctx, "ipa_bases_fold", ipa_bases_fold<F>, grid_1d((half + chunk - 1) / chunk, 64), dim3(64), 0, pts + offset_lo * b->stride_u32,
                      pts + offset_hi * b->stride_u32, (uint32_t)half, chunk, s, r->d.p, w.p);
            return ZKHIP_OK;
        }));
    }
    // drained like every constructor of bases: the workspace may be handed to the next call, and the handle is usable at once
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *out = r.release();
    return ZKHIP_OK;
}

int zkhip_fr_inner_product_dev(zkhip_ctx *ctx, int curve, const void *d_a, const void *d_b, size_t n, void *d_out) {
    ZK_ARGS(ctx, curve);
    if (!d_out || (n && (!d_a || !d_b))) return ZKHIP_ERR_INVALID;
    if (n >= ((size_t)1 << 39)) return ZKHIP_ERR_RANGE;
    ZK_ENTER(ctx);
    const uint32_t nblk = (uint32_t)std::min<size_t>(IP_MAX_BLOCKS, (n + IP_THREADS - 1) / IP_THREADS);
    WsOne<uint32_t> w = {(size_t)std::max(1u, nblk) * 16};
    ZK_TRY(ws_place(ctx, w));
    return fr_dispatch(curve, [&](auto u) -> int {
        using U = typename decltype(u)::type;
        static_assert(U::SL <= 16, "partial-sum slot");
        if (nblk) ZK_LAUNCH(ctx, "ipa_inner_product_blocks", ipa_inner_product_blocks<U>, dim3(nblk), dim3(IP_THREADS), 0, (const uint32_t *)d_a, (const uint32_t *)d_b, n, w.p);
        ZK_LAUNCH(ctx, "ipa_inner_product_final", ipa_inner_product_final<U>, dim3(1), dim3(IP_THREADS), 0, w.p, nblk, (uint32_t *)d_out);
        return ZKHIP_OK;
    });
}

int zkhip_fr_powers_lincomb_dev(zkhip_ctx *ctx, int curve, const uint64_t *points, const uint64_t *scales, size_t npoints, void *d_out, size_t n) {
    ZK_ARGS(ctx, curve);
    if ((n && !d_out) || (npoints && (!points || !scales))) return ZKHIP_ERR_INVALID;
    if (npoints >= 65536 || n >= ((size_t)1 << 39)) return ZKHIP_ERR_RANGE;
    if (n == 0) return ZKHIP_OK;
    ZK_ENTER(ctx);
    if (npoints == 0) {  // the empty sum
        ZK_HIP_CHECK(ctx, hipMemsetAsync(d_out, 0, n * 32, ctx->stream));
        return ZKHIP_OK;
    }
    PowersBuffers w = {npoints};
    ZK_TRY(ws_place(ctx, w));
    ZK_TRY(ws_upload(ctx, w.pts, points, npoints * 32));
    ZK_TRY(ws_upload(ctx, w.pts + npoints * 8, scales, npoints * 32));
    const size_t lanes = (n + POWERS_CHUNK - 1) / POWERS_CHUNK;
    return fr_dispatch(curve, [&](auto u) -> int {
        using U = typename decltype(u)::type;
        ZK_LAUNCH(ctx, "ipa_powers_lincomb", ipa_powers_lincomb<U>, grid_1d(lanes), dim3(256), 0, w.pts, (uint32_t)npoints, n, (uint32_t *)d_out);
        return ZKHIP_OK;
    });
}

int zkhip_fr_challenge_products_dev(zkhip_ctx *ctx, int curve, const uint64_t *chals, size_t rounds, void *d_out) {
    ZK_ARGS(ctx, curve);
    if (!d_out || (rounds && !chals)) return ZKHIP_ERR_INVALID;
    if (rounds > 31) return ZKHIP_ERR_RANGE;
    ZK_ENTER(ctx);
    ChallengeBuffers w = {std::max<size_t>(1, rounds)};
    ZK_TRY(ws_place(ctx, w));
    if (rounds) ZK_TRY(ws_upload(ctx, w.c, chals, rounds * 32));
    return fr_dispatch(curve, [&](auto u) -> int {
        using U = typename decltype(u)::type;
        static_assert(U::SL <= 16, "challenge slot");
        if (rounds) ZK_LAUNCH(ctx, "ipa_challenge_setup", fr_table_to_mont<U>, grid_1d(rounds, 64), dim3(64), 0, w.c, (uint32_t)rounds, w.m);
        ZK_LAUNCH(ctx, "ipa_challenge_products", ipa_challenge_products<U>, grid_1d((size_t)1 << rounds), dim3(256), 0, w.m, (uint32_t)rounds, (uint32_t *)d_out);
        return ZKHIP_OK;
    });
}

}  // extern "C"
