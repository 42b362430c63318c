// Pippenger multi-scalar multiplication for gfx950 (MI355X): the kernels that touch coordinates and the per-(curve, group) host logic.
// Included by one translation unit per (curve, group) -- msm_bls_g1.hip, msm_bls_g2.hip, msm_bn_g1.hip, msm_bn_g2.hip, msm_pallas_g1.hip, msm_vesta_g1.hip --
// so that the six instantiations compile in parallel.  The stage that needs no field -- digits, sort, size order, large-bucket plan -- is compiled once,
// in msm_entries.hip (interface: msm_entries.hpp); msm.hip holds the curve-independent host side.
//
// Replaces algebra::multiexp<multiexp_method_BDLO12> / multiexp_with_mixed_addition as called at
//   zk/snark/systems/ppzksnark/r1cs_gg_ppzksnark/prover.hpp:108-139   (A, B, H, L queries)
//   zk/commitments/polynomial/kzg.hpp:143-148, 409-435                  (KZG commit)
//   zk/commitments/polynomial/knowledge_commitment_multiexp.hpp:107     (sparse (G2,G1) query)
//
// Algorithm.  Scalars are folded to |s| <= (r - 1) / 2 and cut into W signed digits of ~c bits (msm_recode.hpp).  With
// WINDOW TABLES (table w holds 2^off(w) P_i for every point, built once at upload) every (point, window) pair is an
// addition of equal weight: all W n pairs are sorted by |digit| into ONE set of B = 2^(c-1) buckets -- or, when that
// leaves too few buckets to fill the chip, into S sets (pair (i, w) goes to set w mod S) that are folded bucket-wise
// afterwards.  One lane per bucket accumulates its entries with XYZZ mixed additions; sum_b (b + 1) bucket[b] follows.
// Merging the windows lets c grow to ~log2(n) + 0..1 (c = 20 at 2^20 points: 13 windows instead of the 16 of c = 16,
// 19 % fewer additions) with the same number of lanes (2^19 buckets of ~26 entries against 16 x 2^15 of ~32).
// Without tables (fewer than 32 points, or tables that do not fit) the sets are the windows themselves and the
// final kernel combines them by a Horner pass.
//
// Data layout in HBM
//   bases    : nslots tables x n x {x, y}  lazy Montgomery limbs (fu.hpp), 16 words per coordinate, AoS, (0,0) = infinity
//   scalars  : n x 8 u32             canonical little-endian
//   dig      : W x n u32             signed digit of scalar i in (local) window w: (|d|-1) | sign<<31, NONE if d = 0
//   offs     : nb + 1 u32            exclusive prefix of the bucket sizes, nb = S * B
//   idx      : (#non-zero digits) u32  entry = (table slot * bases_n + point index) | sign<<31, grouped by (set, bucket)
//   order    : nb u32                bucket ids by descending size
//   buckets  : nb XYZZ               bucket sums
//   segsum / winsum                  per-workgroup weighted sums of the bucket reduction / per-set sums
//
// Kernels (all integer VALU; no MFMA -- this is modular arithmetic, not a dense contraction):
//   (msm_entries.hip: msm_digits_only, msm_sort_*, msm_scan_*, msm_size_* -- dig, offs, idx, order and the large-bucket plan)
//   msm_bucket_acc_lds  one lane per bucket (G1) or one even / odd lane pair per bucket (G2, fu2_pair.hpp): gather affine
//                     points, XYZZ mixed additions, accumulator coordinates in LDS; on G1 the first addition of a bucket is
//                     affine + affine (xyzz_add_affine: no products by ZZ = ZZZ = one)                       <- dominant
//   msm_bucket_large / msm_large_combine   buckets far above the mean (the plan: msm_size_scatter), one workgroup per 4096-entry task
//   msm_bucket_merge  S > 1: fold the S equal-weight sets bucket by bucket (radix-4 tree)
//   msm_fold          (round 5, table-backed sets of >= 2^16 buckets) row and column sums of the bucket index b = h C + l: the reduction
//                     sum_b (b + 1) bucket[b] becomes sum_l (l + 1) COL[l] + C sum_h h ROW[h], i.e. the three kernels below over 2 sets of
//                     C ~ sqrt(B) buckets instead of one of B
//   msm_bucket_red    running sums over segments of L buckets + (seg L) * segment sum per lane, LDS tree per workgroup
//   msm_window_sum    LDS tree over the per-workgroup partials of a set
//   msm_final         (Horner over the windows when there are no tables,) XYZZ -> Jacobian, Montgomery -> canonical
//   msm_final_fold    the same after msm_fold: COL sum + 2^log2(C) ROW sum
//   msm_final_batch   the same for every member of a batch
//   msm_wide_weigh / msm_wide_tree / msm_wide_final   level 2 after msm_fold for G1, one point per wave (fu_wide.hpp), in place of the four above
// (msm_final, msm_final_fold and msm_write_infinity store through curve.hpp's xyzz_store_canonical_jacobian.  msm_final_batch and jac_sum_k keep the three
// stores spelled out, msm_bucket_large its own copy of block_tree_sum's loop, and the three batch inversions their walk back from the inversion, which is
// curve.hpp's xyzz_parked_to_affine written in place: through the shared helper an instance of each compiled worse or measured slower -- EXPERIMENTS 14, 22.)
// Point order inside a bucket depends on LDS-atomic arrival order; the group law is exact, so the sum
// (compared in affine) does not.
#pragma once
#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#ifndef ZK_NOINLINE_MUL2
#define ZK_NOINLINE_MUL2 1  // G2 (Fq2) products stay out of line; G1 products are inlined (out of line measured 27 % slower)
#endif
#include "ctx.hpp"
#include "curve.hpp"
#include "msm_entries.hpp"
#include "msm_ops.hpp"
#include "msm_recode.hpp"
#include "msm_bucket_acc.hpp"
#include "fu_pair.hpp"
#include "fu_quad.hpp"
#include "fu_wide.hpp"

namespace {

using namespace zkhip;

#ifndef MSM_G1_THREADS
#define MSM_G1_THREADS 64  // lanes per bucket-accumulation workgroup: 64 measured 5 % faster than 128 / 256 (finer refill)
#endif
#ifndef MSM_G2_THREADS
#define MSM_G2_THREADS 256
#endif
#ifndef MSM_G2_WAVES
#define MSM_G2_WAVES 2
#endif

// (all kernels below: F is the type a lane holds, LPB lanes share one point -- fu2_pair.hpp; `t` is the point slot)
template <class F, int LPB>
__global__ __launch_bounds__(128) void msm_bucket_large(const uint32_t *__restrict__ bases, const uint32_t *__restrict__ idx,
                                                        const uint32_t *__restrict__ plan, const uint32_t *__restrict__ tasks,
                                                        uint32_t *__restrict__ partials) {
    constexpr int NL = FieldOps<F>::WORDS;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t ntasks = plan[0];
    for (uint32_t task = blockIdx.x; task < ntasks; task += gridDim.x) {
        const uint32_t lo = tasks[3 * task + 1], hi = tasks[3 * task + 2], t = threadIdx.x / LPB;
        XYZZ<F> acc = XYZZ<F>::infinity();
        for (uint32_t k = lo + t; k < hi; k += blockDim.x / LPB) {
            uint32_t e = idx[k];
            Affine<F> p = affine_load<F>(bases + (size_t)(e & 0x7FFFFFFFu) * (2 * NL));
            acc = xyzz_madd(acc, p, (e >> 31) != 0);
        }
        xyzz_store<F>(lds + (size_t)t * (4 * NL), acc);
        __syncthreads();
        for (uint32_t d = blockDim.x / LPB / 2; d >= 1; d >>= 1) {
            if (t < d) {
                acc = xyzz_add(xyzz_load<F>(lds + (size_t)t * (4 * NL)), xyzz_load<F>(lds + (size_t)(t + d) * (4 * NL)));
                xyzz_store<F>(lds + (size_t)t * (4 * NL), acc);
            }
            __syncthreads();
        }
        if (t == 0) xyzz_store<F>(partials + (size_t)task * (4 * NL), acc);
        __syncthreads();
    }
}

// one wave per large bucket: lanes fold the bucket's task partials in strides, then an LDS tree
template <class F, int LPB>
__global__ __launch_bounds__(64) void msm_large_combine(const uint32_t *__restrict__ plan, const uint32_t *__restrict__ large,
                                                        const uint32_t *__restrict__ partials, uint32_t *__restrict__ buckets) {
    constexpr int NL = FieldOps<F>::WORDS;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t nlarge = plan[1], t = threadIdx.x / LPB;
    for (uint32_t j = blockIdx.x; j < nlarge; j += gridDim.x) {
        const uint32_t g = large[3 * j], first = large[3 * j + 1], nt = large[3 * j + 2];
        XYZZ<F> acc = XYZZ<F>::infinity();
        for (uint32_t k = t; k < nt; k += 64 / LPB) acc = xyzz_add(acc, xyzz_load<F>(partials + (size_t)(first + k) * (4 * NL)));
        if (nt > 1) {  // uniform over the wave
            xyzz_store<F>(lds + (size_t)t * (4 * NL), acc);
            __syncthreads();
            for (uint32_t d = 32 / LPB; d >= 1; d >>= 1) {
                if (t < d && t + d < nt) {
                    acc = xyzz_add(xyzz_load<F>(lds + (size_t)t * (4 * NL)), xyzz_load<F>(lds + (size_t)(t + d) * (4 * NL)));
                    xyzz_store<F>(lds + (size_t)t * (4 * NL), acc);
                }
                __syncthreads();
            }
        }
        if (t == 0) xyzz_store<F>(buckets + (size_t)g * (4 * NL), acc);
        __syncthreads();
    }
}

// buckets[s][b] += buckets[s + q][b] + buckets[s + 2q][b] + buckets[s + 3q][b] for s < q (sets >= cur do not exist):
// one radix-4 level of the tree that folds the equal-weight sets
template <class F, int LPB>
__global__ __launch_bounds__(256) void msm_bucket_merge(uint32_t *__restrict__ buckets, uint32_t B, uint32_t q, uint32_t cur) {
    constexpr int NL = FieldOps<F>::WORDS;
    uint32_t g = (blockIdx.x * blockDim.x + threadIdx.x) / LPB;  // = s * B + b
    if (g >= q * B) return;
    const uint32_t s = g / B;
    uint32_t *dst = buckets + (size_t)g * (4 * NL);
    XYZZ<F> acc = xyzz_load<F>(dst);
    for (uint32_t k = 1; k < 4; ++k)
        if (s + k * q < cur) acc = xyzz_add(acc, xyzz_load<F>(buckets + ((size_t)g + (size_t)k * q * B) * (4 * NL)));
    xyzz_store<F>(dst, acc);
}

// ---- tail: sum_b (b + 1) * bucket[b] per set -----------------------------------------------------------
// Every operation here is a full (projective) addition or doubling, a few thousand dependent instructions that a
// lone wave issues at one per ~4 cycles: the tail is bound by the LENGTH of its dependency chain as long as its lanes
// fit the chip.  Stage 1 gives every lane one segment of L buckets and folds the lanes of a workgroup in an LDS tree;
// stage 2 folds the per-workgroup partials of a set (one more tree).
// segment `seg` covers buckets [seg*L, seg*L + L) (bucket b holds digit value b + 1):
//   sum_b (b + 1) * bucket[b]  restricted to the segment
//       = sum_b (b - seg*L + 1) * bucket[b]  +  (seg*L) * sum_b bucket[b]
constexpr int MSM_TAIL_THREADS = 256;

template <class F>
ZK_D XYZZ<F> block_tree_sum(uint32_t *lds, XYZZ<F> acc, uint32_t t, uint32_t nthreads) {
    constexpr int NL = FieldOps<F>::WORDS;
    xyzz_store<F>(lds + (size_t)t * (4 * NL), acc);
    __syncthreads();
    for (uint32_t d = nthreads / 2; d >= 1; d >>= 1) {
        if (t < d) {
            acc = xyzz_add(xyzz_load<F>(lds + (size_t)t * (4 * NL)), xyzz_load<F>(lds + (size_t)(t + d) * (4 * NL)));
            xyzz_store<F>(lds + (size_t)t * (4 * NL), acc);
        }
        __syncthreads();
    }
    return acc;  // lane 0: the sum
}

// grid = sets x nblk workgroups; partial[s * nblk + j] = weighted sum of segments [SLOTS j, SLOTS j + SLOTS) of set s.
// Two waves per SIMD: the G1 kernels then spill (pairs 154 registers, one lane 765); bound 1 has no spills (330 / 446 VGPRs) and
// measures the same for a single MSM (0.699 against 0.716 ms at 2^19 buckets) but worse for batches, whose many waves want
// the second slot (50 x 2^19 buckets: 17.4 against 13.7 ms).
template <class F, int LPB>
#ifndef ZK_TAIL_WAVES
#define ZK_TAIL_WAVES 2  // workgroups of the reduction per CU the register allocation leaves room for (1: no spills; measured)
#endif
__global__ __launch_bounds__(MSM_TAIL_THREADS, ZK_TAIL_WAVES) void msm_bucket_red(const uint32_t *__restrict__ buckets, uint32_t B, uint32_t L, uint32_t nseg,
                                                                   uint32_t nblk, uint32_t *__restrict__ partial) {
    constexpr int NL = FieldOps<F>::WORDS;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    constexpr uint32_t SLOTS = MSM_TAIL_THREADS / LPB;
    const uint32_t t = threadIdx.x / LPB, w = blockIdx.x / nblk, seg = (blockIdx.x % nblk) * SLOTS + t;
    XYZZ<F> sum = XYZZ<F>::infinity();
    if (seg < nseg) {
        const uint32_t *base = buckets + ((size_t)w * B + (size_t)seg * L) * (4 * NL);
        if (L == 1) {
            sum = xyzz_mul_small(xyzz_load<F>(base), seg + 1);
        } else {
            XYZZ<F> run = XYZZ<F>::infinity();
            for (int b = (int)L - 1; b >= 0; --b) {
                run = xyzz_add(run, xyzz_load<F>(base + (size_t)b * (4 * NL)));
                sum = xyzz_add(sum, run);
            }
            if (seg != 0) sum = xyzz_add(sum, xyzz_mul_small(run, seg * L));
        }
    }
    sum = block_tree_sum<F>(lds, sum, t, SLOTS);
    if (t == 0) xyzz_store<F>(partial + (size_t)blockIdx.x * (4 * NL), sum);
}

// one workgroup (64 or 256 lanes: msm_window_threads) per set: winsum[s] = sum_j partial[s][j]
template <class F, int LPB>
__global__ __launch_bounds__(256) void msm_window_sum(const uint32_t *__restrict__ partial, uint32_t nblk, uint32_t *__restrict__ winsum) {
    constexpr int NL = FieldOps<F>::WORDS;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t w = blockIdx.x, t = threadIdx.x / LPB, slots = blockDim.x / LPB;
    XYZZ<F> acc = XYZZ<F>::infinity();
    for (uint32_t j = t; j < nblk; j += slots) acc = xyzz_add(acc, xyzz_load<F>(partial + ((size_t)w * nblk + j) * (4 * NL)));
    if (nblk > 1) acc = block_tree_sum<F>(lds, acc, t, slots);
    if (t == 0) xyzz_store<F>(winsum + (size_t)w * (4 * NL), acc);
}
// every operation is ~10 us of one wave: a tree level more (256 lanes) is cheaper than three more serial additions per lane
inline uint32_t msm_window_threads(uint32_t nblk, int lanes_per_point) { return (size_t)nblk * lanes_per_point > 128 ? 256u : 64u; }

// ---- two-level tail (round 5) -----------------------------------------------------------------------------------------------
// The running sums above are a DEPENDENT chain of 2 L additions per lane plus the (seg L) multiple: at 2^19 buckets ~76 operations of
// ~9 us each, 0.8 ms of a 2.85-ms MSM with one wave per SIMD.  Split the bucket index instead: bucket b = h C + l (l < C, h < R,
// B = R C) holds digit value b + 1 = h C + (l + 1), so
//     sum_b (b + 1) bucket[b]  =  sum_l (l + 1) COL[l]  +  C sum_h h ROW[h],     COL[l] = sum_h bucket[h C + l],   ROW[h] = sum_l bucket[h C + l]
// -- 2 B additions like the running sums, but every one of them sits in an independent SUM, and what is left for the dependent chain is the old
// tail over 2 sets of C = 2^ceil(log2(B) / 2) buckets (COL as it is, ROW[h] in bucket h - 1, the rest empty) and log2(C) doublings of the second
// set's sum.  (The "split the windows" step of bucket-method MSMs on GPUs, applied to the ONE merged bucket set the window tables leave.)
struct MsmFold {
    uint32_t B, C, R, log_c;
    uint32_t run;           // buckets a lane sums before the workgroup's tree takes over
    uint32_t m_row, m_col;  // runs (= LDS partial sums) per row: C / run, per column: R / run
};
inline MsmFold msm_fold_geom(const zkhip_ctx *ctx, uint32_t B) {
    MsmFold g;
    int lb = 0;
    while ((1u << lb) < B) ++lb;
    g.B = B;
    g.log_c = (uint32_t)((lb + 1) / 2);
    g.C = 1u << g.log_c;
    g.R = B >> g.log_c;
    // measured (tools/msm_profile.py, G1): 2^19 buckets: 8 and 16 the same (0.31 ms), 32 slower (0.52: half the SIMDs idle); 2^16 buckets: 8: 0.150,
    // 4: 0.108, 2: 0.094 ms
    g.run = ctx->opt_msm_fold_run > 0 ? (uint32_t)ctx->opt_msm_fold_run : (B >= (1u << 18) ? 8u : 4u);
    g.run = std::max(1u, std::min(g.run, g.R));
    g.m_row = g.C / g.run;
    g.m_col = g.R / g.run;
    return g;
}

// grid = sets x B / (RUN SA) workgroups, SA = threads / LA points: the first half of a set's workgroups sum ROWS (SA / m_row whole rows each), the second
// half COLUMNS (SA / m_col whole columns each).
//   phase 1, bound by WORK: every point slot sums RUN buckets of its row / column with the lane shape FA (one lane per point for G1: an addition
//            in the fewest issue slots), interleaved so that adjacent lanes read adjacent buckets, and leaves the sum in LDS;
//   phase 2, bound by LATENCY: binary trees over the m partial sums of each row / column in LDS with the lane shape FT (G1: lane quads);
//   level2[2 set][l] = COL[l], level2[2 set + 1][h - 1] = ROW[h] (row 0 has weight 0: dropped; entries R - 1 ... C - 1 of the second set are
//   empty: the row half's workgroups zero them, dealt out among themselves, so every word of level2 is written here and the caller clears nothing).
template <class FA, int LA, class FT, int LT>
__global__ __launch_bounds__(MSM_TAIL_THREADS, ZK_TAIL_WAVES) void msm_fold(const uint32_t *__restrict__ buckets, MsmFold g, uint32_t *__restrict__ level2) {
    constexpr int NL = FieldOps<FA>::WORDS;
    constexpr uint32_t SA = MSM_TAIL_THREADS / LA, ST = MSM_TAIL_THREADS / LT, PW = 4 * NL;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t half_wgs = g.B / (SA * g.run);
    const uint32_t w = blockIdx.x / (2 * half_wgs), k = blockIdx.x % (2 * half_wgs);
    const bool col = k >= half_wgs;
    const uint32_t wg = col ? k - half_wgs : k, s = threadIdx.x / LA;
    const uint32_t m = col ? g.m_col : g.m_row, G = SA / m;  // partial sums per output, outputs of this workgroup
    uint32_t first, stride, slot;
    if (!col) {  // slot (r, j): buckets h C + j + i m_row of row h = wg G + r
        first = (wg * G + s / m) * g.C + s % m;
        stride = m;
        slot = s;
    } else {  // slot (j, ll), ll fastest: buckets (j + i m_col) C + l of column l = wg G + ll; its sum goes to LDS slot ll m_col + j
        const uint32_t j = s / G, ll = s % G;
        first = j * g.C + wg * G + ll;
        stride = m * g.C;
        slot = ll * m + j;
    }
    {
        const uint32_t *src = buckets + ((size_t)w * g.B + first) * PW;
        XYZZ<FA> acc = xyzz_load<FA>(src);
        for (uint32_t i = 1; i < g.run; ++i) acc = xyzz_add(acc, xyzz_load<FA>(src + (size_t)i * stride * PW));
        xyzz_store<FA>(lds + (size_t)slot * PW, acc);
    }
    __syncthreads();
    const uint32_t t = threadIdx.x / LT;
    for (uint32_t half = m / 2; half >= 1; half >>= 1) {
        const uint32_t adds = G * half;
        for (uint32_t idx = t; idx < adds; idx += ST) {
            uint32_t *p = lds + (size_t)((idx / half) * m + idx % half) * PW;
            xyzz_store<FT>(p, xyzz_add(xyzz_load<FT>(p), xyzz_load<FT>(p + (size_t)half * PW)));
        }
        __syncthreads();
    }
    for (uint32_t i = t; i < G; i += ST) {
        const uint32_t o = wg * G + i;  // row h / column l
        if (col || o != 0)
            xyzz_store<FT>(level2 + (((size_t)2 * w + (col ? 0 : 1)) * g.C + (col ? o : o - 1)) * PW, xyzz_load<FT>(lds + (size_t)i * m * PW));
    }
    if (!col) {  // the empty entries of the second set
        for (uint32_t e = g.R - 1 + wg; e < g.C; e += half_wgs) {
            uint32_t *z = level2 + (((size_t)2 * w + 1) * g.C + e) * PW;
            for (uint32_t i = threadIdx.x; i < PW; i += MSM_TAIL_THREADS) z[i] = 0u;
        }
    }
}

// out[i] = winsum[2 i] + 2^shift winsum[2 i + 1] as canonical Jacobian; outs == nullptr: the single output `out`
template <class F, int LPB>
__global__ __launch_bounds__(64) void msm_final_fold(const uint32_t *__restrict__ winsum, uint32_t count, uint32_t shift, uint32_t *const *__restrict__ outs,
                                                     uint32_t *__restrict__ out) {
    constexpr int NL = FieldOps<F>::WORDS;
    if (blockIdx.x >= count || threadIdx.x >= LPB) return;
    XYZZ<F> acc = xyzz_load<F>(winsum + ((size_t)2 * blockIdx.x + 1) * (4 * NL));
    if (!acc.is_inf())
        for (uint32_t i = 0; i < shift; ++i) acc = xyzz_dbl(acc);
    acc = xyzz_add(acc, xyzz_load<F>(winsum + (size_t)2 * blockIdx.x * (4 * NL)));
    xyzz_store_canonical_jacobian<F>(outs ? outs[blockIdx.x] : out, acc);
}

// ---- level 2 of the two-level tail with one point per wave (fu_wide.hpp) ---------------------------------------------------------------
// The same sums in the same shape -- every point times its digit value, a binary tree over each set, log2(C) doublings of the second set's sum,
// one addition, the canonical store -- but an operation is ~2.4 us of a wave instead of the quad's ~6.8, and the launches are cut so that a SIMD
// holds at most two waves while the chain runs.  Workgroups of MSM_WIDE_WAVES waves, a point per wave, LDS trees between them:
//   msm_wide_weigh   point b of a set times (b + 1), then the tree over the workgroup's MSM_WIDE_WAVES points   C / MSM_WIDE_WAVES partials per set
//   msm_wide_tree    2 MSM_WIDE_WAVES consecutive partials to one (launched while a set has more than MSM_WIDE_WAVES partials)
//   msm_wide_final   one workgroup per MSM, half its waves per set: the last tree levels, the doublings, the addition, the canonical store
constexpr uint32_t MSM_WIDE_WAVES = 8;  // 512 lanes: two waves per SIMD while every wave of a workgroup works, one from the first tree level on

// tree over the nw (power of two) waves of a group that starts at LDS slot 0 of `lds`; wave 0 of the group returns the sum
template <class U>
ZK_D XYZZ<FuW<U>> wide_tree_sum(uint32_t *lds, XYZZ<FuW<U>> acc, uint32_t w, uint32_t nw) {
    constexpr uint32_t PW = 4 * U::SL;
    wide_store<U>(lds + w * PW, acc);
    __syncthreads();
    for (uint32_t d = nw / 2; d >= 1; d >>= 1) {
        if (w < d) {
            acc = xyzz_add(wide_load<U>(lds + w * PW), wide_load<U>(lds + (w + d) * PW));
            wide_store<U>(lds + w * PW, acc);
        }
        __syncthreads();
    }
    return acc;
}

// grid = points / MSM_WIDE_WAVES; point s C + b is bucket b of set s (C a power of two and a multiple of MSM_WIDE_WAVES: a workgroup stays inside a set)
template <class U>
__global__ __launch_bounds__(MSM_WIDE_WAVES * 64) void msm_wide_weigh(const uint32_t *__restrict__ points, uint32_t C, uint32_t *__restrict__ partial) {
    constexpr uint32_t PW = 4 * U::SL;
    __shared__ uint32_t lds[MSM_WIDE_WAVES * PW];
    const uint32_t w = threadIdx.x >> 6, i = blockIdx.x * MSM_WIDE_WAVES + w;
    XYZZ<FuW<U>> acc = xyzz_mul_small(wide_load<U>(points + (size_t)i * PW), (i & (C - 1)) + 1);
    acc = wide_tree_sum<U>(lds, acc, w, MSM_WIDE_WAVES);
    if (w == 0) wide_store<U>(partial + (size_t)blockIdx.x * PW, acc);
}

// grid = points / (2 MSM_WIDE_WAVES): out[j] = in[2 W j] + ... + in[2 W j + 2 W - 1], W = MSM_WIDE_WAVES
template <class U>
__global__ __launch_bounds__(MSM_WIDE_WAVES * 64) void msm_wide_tree(const uint32_t *__restrict__ in, uint32_t *__restrict__ out) {
    constexpr uint32_t PW = 4 * U::SL;
    __shared__ uint32_t lds[MSM_WIDE_WAVES * PW];
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t *src = in + ((size_t)blockIdx.x * 2 * MSM_WIDE_WAVES + w) * PW;
    XYZZ<FuW<U>> acc = xyzz_add(wide_load<U>(src), wide_load<U>(src + (size_t)MSM_WIDE_WAVES * PW));
    acc = wide_tree_sum<U>(lds, acc, w, MSM_WIDE_WAVES);
    if (w == 0) wide_store<U>(out + (size_t)blockIdx.x * PW, acc);
}

// grid = MSMs; partial[(2 i + k) m + j], j < m (a power of two): out[i] = sum_j partial[2 i][j] + 2^shift sum_j partial[2 i + 1][j] as canonical Jacobian;
// outs == nullptr: the single output `out`.  The first half of the waves takes the second set (whose sum the doublings wait for).
template <class U>
__global__ __launch_bounds__(MSM_WIDE_WAVES * 64) void msm_wide_final(const uint32_t *__restrict__ partial, uint32_t m, uint32_t shift, uint32_t *const *__restrict__ outs,
                                                                      uint32_t *__restrict__ out) {
    constexpr uint32_t PW = 4 * U::SL, HALF = MSM_WIDE_WAVES / 2;
    __shared__ uint32_t lds[MSM_WIDE_WAVES * PW];
    const uint32_t w = threadIdx.x >> 6, half = w / HALF, q = w % HALF;
    const uint32_t *src = partial + ((size_t)2 * blockIdx.x + (1 - half)) * m * PW;
    XYZZ<FuW<U>> acc = XYZZ<FuW<U>>::infinity();
    for (uint32_t j = q; j < m; j += HALF) acc = xyzz_add(acc, wide_load<U>(src + (size_t)j * PW));
    acc = wide_tree_sum<U>(lds + half * HALF * PW, acc, q, HALF);
    if (w != 0) return;
    if (!acc.is_inf())
        for (uint32_t i = 0; i < shift; ++i) acc = xyzz_dbl(acc);
    acc = xyzz_add(acc, wide_load<U>(lds + HALF * PW));
    const XYZZ<FuQ<U>> whole = wide_gather<U>(acc);
    if (wide_lane() < 4) xyzz_store_canonical_jacobian<FuQ<U>>(outs ? outs[blockIdx.x] : out, whole);  // one quad: the conversion is the quad tail's
}

// result = sum_w 2^off(w) winsum[w]  (Horner from the top window; a single set with tables), emitted as canonical Jacobian
template <class F, int LPB>
__global__ __launch_bounds__(64) void msm_final(const uint32_t *__restrict__ winsum, int W, MsmWindows win, uint32_t *__restrict__ out_jac) {
    constexpr int NL = FieldOps<F>::WORDS;
    if (blockIdx.x != 0 || threadIdx.x >= LPB) return;
    XYZZ<F> acc = XYZZ<F>::infinity();
    for (int w = W - 1; w >= 0; --w) {
        if (!acc.is_inf())
            for (int i = 0; i < win.width(w); ++i) acc = xyzz_dbl(acc);
        acc = xyzz_add(acc, xyzz_load<F>(winsum + (size_t)w * (4 * NL)));
    }
    xyzz_store_canonical_jacobian<F>(out_jac, acc);
}

// ---- bases maintenance ----------------------------------------------------------------------------
// canonical affine (x | y, CANON_WORDS each) -> device form (Montgomery, WORDS each); flagged points -> (0, 0)
template <class F>
__global__ __launch_bounds__(256) void bases_to_mont(const uint32_t *__restrict__ canon, const uint8_t *__restrict__ inf, uint32_t n,
                                                     uint32_t *__restrict__ pts) {
    typedef FieldOps<F> O;
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *c = canon + (size_t)i * (2 * O::CANON_WORDS);
    Affine<F> a;
    if (inf != nullptr && inf[i]) a = Affine<F>::infinity();
    else a = {O::from_canonical(c), O::from_canonical(c + O::CANON_WORDS)};
    affine_store<F>(pts + (size_t)i * (2 * O::WORDS), a);
}

template <class F>
__global__ __launch_bounds__(256) void bases_from_mont(const uint32_t *__restrict__ pts, uint32_t n, uint32_t *__restrict__ out,
                                                       uint8_t *__restrict__ inf) {
    typedef FieldOps<F> O;
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<F> a = affine_load<F>(pts + (size_t)i * (2 * O::WORDS));
    inf[i] = a.is_inf() ? 1 : 0;
    uint32_t *o = out + (size_t)i * (2 * O::CANON_WORDS);
    O::to_canonical(o, a.x);
    O::to_canonical(o + O::CANON_WORDS, a.y);
}

// pts[i] = scalars[i] * base, double-and-add from the top bit, then one inversion per point
template <class F>
__global__ __launch_bounds__(64) void bases_mul(uint32_t *__restrict__ pts, const uint32_t *__restrict__ base_canonical,
                                                const uint32_t *__restrict__ scalars, uint32_t n) {
    constexpr int NL = FieldOps<F>::WORDS;
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<F> g = {FieldOps<F>::from_canonical(base_canonical), FieldOps<F>::from_canonical(base_canonical + FieldOps<F>::CANON_WORDS)};
    const uint32_t *s = scalars + (size_t)i * 8;
    XYZZ<F> acc = XYZZ<F>::infinity();
    for (int b = 255; b >= 0; --b) {
        acc = xyzz_dbl(acc);
        if ((s[b >> 5] >> (b & 31)) & 1) acc = xyzz_madd(acc, g);
    }
    affine_store<F>(pts + (size_t)i * (2 * NL), xyzz_to_affine(acc));
}

// ---- fixed-base batch exponentiation (batch_exp of generator.hpp:187-214: every point is a multiple of ONE base) --------------------
// tab[(w << 8) + d] = d 2^(8 w) base, affine, d in [1, 256), w < 32.  One lane per window: 8 w doublings, 254 mixed additions in
// XYZZ parked in `tmp` (5 field elements per entry: X, Y, ZZ, ZZZ, prefix product), ONE inversion (Montgomery's trick), back down.
constexpr int FIXED_WBITS = 8, FIXED_NW = 32, FIXED_ROW = 1 << FIXED_WBITS;
template <class F>
__global__ __launch_bounds__(64) void bases_fixed_table(const uint32_t *__restrict__ base_canonical, uint32_t *__restrict__ tab, uint32_t *__restrict__ tmp) {
    typedef FieldOps<F> O;
    constexpr int NL = O::WORDS;
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= FIXED_NW) return;
    Affine<F> g = {O::from_canonical(base_canonical), O::from_canonical(base_canonical + O::CANON_WORDS)};
    XYZZ<F> P = XYZZ<F>::from_affine(g);
    for (uint32_t k = 0; k < w * FIXED_WBITS; ++k) P = xyzz_dbl(P);
    uint32_t *mine = tmp + (size_t)w * FIXED_ROW * (5 * NL);
    XYZZ<F> acc = P;
    F pre = F::one();
    for (uint32_t d = 1; d < FIXED_ROW; ++d) {  // entry d: d P (P is not affine: full additions; the table is built once per call)
        if (d > 1) acc = xyzz_add(acc, P);
        uint32_t *slot = mine + (size_t)d * (5 * NL);
        xyzz_store<F>(slot, acc);
        pre = O::mul(pre, O::mul(acc.ZZ, acc.ZZZ));
        O::store(slot + 4 * NL, pre);
    }
    F inv = O::inv(pre);
    for (uint32_t d = FIXED_ROW; d-- > 1;) {
        const uint32_t *slot = mine + (size_t)d * (5 * NL);
        XYZZ<F> q = xyzz_load<F>(slot);
        F before = d > 1 ? O::load(mine + (size_t)(d - 1) * (5 * NL) + 4 * NL) : F::one();
        F dinv = O::mul(inv, before);
        inv = O::mul(inv, O::mul(q.ZZ, q.ZZZ));
        Affine<F> a = {O::mul(q.X, O::mul(dinv, q.ZZZ)), O::mul(q.Y, O::mul(dinv, q.ZZ))};
        affine_store<F>(tab + ((size_t)w * FIXED_ROW + d) * (2 * NL), a);
    }
}
// pts[i] = scalars[i] * base = sum_w tab[w][byte w of the scalar]: at most 32 mixed additions per point instead of 256 doublings + ~128
// additions.  A lane takes FIXED_CHUNK consecutive points, parks their XYZZ sums in `tmp` and shares ONE inversion among them.
constexpr uint32_t FIXED_CHUNK = AFFINE_MAX_CHUNK;
template <class F>
__global__ __launch_bounds__(64) void bases_mul_fixed(uint32_t *__restrict__ pts, const uint32_t *__restrict__ tab, const uint32_t *__restrict__ scalars,
                                                      uint32_t n, uint32_t *__restrict__ tmp) {
    typedef FieldOps<F> O;
    constexpr int NL = O::WORDS;
    const uint32_t lo = (blockIdx.x * blockDim.x + threadIdx.x) * FIXED_CHUNK;
    if (lo >= n) return;
    const uint32_t cnt = n - lo < FIXED_CHUNK ? n - lo : FIXED_CHUNK;
    F pre = F::one();
    for (uint32_t k = 0; k < cnt; ++k) {
        const uint32_t *s = scalars + (size_t)(lo + k) * 8;
        XYZZ<F> acc = XYZZ<F>::infinity();
        for (uint32_t w = 0; w < FIXED_NW; ++w) {
            const uint32_t d = (s[w >> 2] >> ((w & 3) * 8)) & 0xFFu;
            if (d) acc = xyzz_madd(acc, affine_load<F>(tab + ((size_t)w * FIXED_ROW + d) * (2 * NL)));
        }
        uint32_t *slot = tmp + (size_t)(lo + k) * (5 * NL);
        xyzz_store<F>(slot, acc);
        if (!acc.is_inf()) pre = O::mul(pre, O::mul(acc.ZZ, acc.ZZZ));
        O::store(slot + 4 * NL, pre);
    }
    F inv = O::inv(pre);
    for (uint32_t k = cnt; k-- > 0;) {
        const uint32_t *slot = tmp + (size_t)(lo + k) * (5 * NL);
        XYZZ<F> q = xyzz_load<F>(slot);
        if (q.is_inf()) {
            affine_store<F>(pts + (size_t)(lo + k) * (2 * NL), Affine<F>::infinity());
            continue;
        }
        F before = k > 0 ? O::load(tmp + (size_t)(lo + k - 1) * (5 * NL) + 4 * NL) : F::one();
        F dinv = O::mul(inv, before);
        inv = O::mul(inv, O::mul(q.ZZ, q.ZZZ));
        Affine<F> a = {O::mul(q.X, O::mul(dinv, q.ZZZ)), O::mul(q.Y, O::mul(dinv, q.ZZ))};
        affine_store<F>(pts + (size_t)(lo + k) * (2 * NL), a);
    }
}

// Window tables: the table of window w holds 2^off(w) P_i in affine form.  One lane per point: width(w - 1) doublings
// per window in XYZZ, the intermediate points of the windows THIS object keeps parked in `tmp`, one shared inversion
// (Montgomery's trick over the lane's own denominators ZZ*ZZZ), then the affine results are written to their slots.
// Window partition (wrank of wworld): only windows w = wrank + k wworld are kept, in slot k + (wrank != 0); slot 0 holds
// the points themselves (= window 0, rank 0's).  tmp: kept x cnt entries of 5 field elements (X, Y, ZZ, ZZZ, prefix product).
template <class F>
__global__ __launch_bounds__(64) void bases_precompute_range(uint32_t *__restrict__ pts, uint32_t n, uint32_t lo, uint32_t cnt, MsmWindows win,
                                                             uint32_t wrank, uint32_t wworld, uint32_t *__restrict__ tmp) {
    const int W = win.W;
    typedef FieldOps<F> O;
    constexpr int NL = O::WORDS;
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;  // index inside the chunk
    if (j >= cnt) return;
    const uint32_t i = lo + j;
    const uint32_t extra = wrank != 0 ? 1u : 0u;
    auto slot_ptr = [&](uint32_t w) { return pts + ((size_t)(w / wworld + extra) * n + i) * (2 * NL); };  // w mod wworld == wrank
    Affine<F> p = affine_load<F>(pts + (size_t)i * (2 * NL));
    if (p.is_inf()) {
        for (uint32_t w = (wrank != 0 ? wrank : wworld); w < (uint32_t)W; w += wworld) affine_store<F>(slot_ptr(w), Affine<F>::infinity());
        return;
    }
    XYZZ<F> acc = XYZZ<F>::from_affine(p);
    F pre = F::one();
    uint32_t kept = 0;
    for (int w = 1; w < W; ++w) {
        for (int k = 0; k < win.width(w - 1); ++k) acc = xyzz_dbl(acc);  // now 2^off(w) P
        if ((uint32_t)w % wworld != wrank) continue;
        uint32_t *slot = tmp + ((size_t)kept * cnt + j) * (5 * NL);
        xyzz_store<F>(slot, acc);
        pre = O::mul(pre, O::mul(acc.ZZ, acc.ZZZ));
        O::store(slot + 4 * NL, pre);
        ++kept;
    }
    if (kept == 0) return;
    F inv = O::inv(pre);  // 1 / prod (ZZ_w ZZZ_w) over the kept windows
    uint32_t w = ((uint32_t)(W - 1) - wrank) / wworld * wworld + wrank;  // the last kept window (kept > 0: it is >= 1)
    for (uint32_t k = kept; k-- > 0; w -= wworld) {
        const uint32_t *slot = tmp + ((size_t)k * cnt + j) * (5 * NL);
        XYZZ<F> q = xyzz_load<F>(slot);
        F before = k > 0 ? O::load(tmp + ((size_t)(k - 1) * cnt + j) * (5 * NL) + 4 * NL) : F::one();
        F dinv = O::mul(inv, before);            // 1 / (ZZ_w ZZZ_w)
        inv = O::mul(inv, O::mul(q.ZZ, q.ZZZ));  // drop this factor
        Affine<F> a = {O::mul(q.X, O::mul(dinv, q.ZZZ)), O::mul(q.Y, O::mul(dinv, q.ZZ))};
        affine_store<F>(slot_ptr(w), a);
    }
}

template <class F>
__global__ void jac_to_affine_k(const uint32_t *__restrict__ jac, uint32_t *__restrict__ aff, uint8_t *__restrict__ inf) {
    typedef FieldOps<F> O;
    constexpr int CW = O::CANON_WORDS;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Jacobian<F> j = {O::from_canonical(jac), O::from_canonical(jac + CW), O::from_canonical(jac + 2 * CW)};
    XYZZ<F> q = xyzz_from_jacobian(j);
    inf[0] = q.is_inf() ? 1 : 0;
    Affine<F> a = xyzz_to_affine(q);
    O::to_canonical(aff, a.x);
    O::to_canonical(aff + CW, a.y);
}

// out = sum_i jac[i] (canonical Jacobian in and out); one lane, `count` is the number of GPUs
template <class F>
__global__ void jac_sum_k(const uint32_t *__restrict__ jac, uint32_t count, uint32_t *__restrict__ out) {
    typedef FieldOps<F> O;
    constexpr int CW = O::CANON_WORDS;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    XYZZ<F> acc = XYZZ<F>::infinity();
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t *p = jac + (size_t)i * 3 * CW;
        Jacobian<F> j = {O::from_canonical(p), O::from_canonical(p + CW), O::from_canonical(p + 2 * CW)};
        acc = xyzz_add(acc, xyzz_from_jacobian(j));
    }
    Jacobian<F> r = xyzz_to_jacobian(acc);
    O::to_canonical(out, r.X);
    O::to_canonical(out + CW, r.Y);
    O::to_canonical(out + 2 * CW, r.Z);
}

template <class F>
__global__ void msm_write_infinity(uint32_t *out_jac) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    xyzz_store_canonical_jacobian<F>(out_jac, XYZZ<F>::infinity());
}

// one workgroup per MSM of a batch: set sum -> canonical Jacobian at that MSM's output pointer
template <class F, int LPB>
__global__ __launch_bounds__(64) void msm_final_batch(const uint32_t *__restrict__ winsum, uint32_t count, uint32_t *const *__restrict__ outs) {
    constexpr int NL = FieldOps<F>::WORDS;
    constexpr int CW = FieldOps<F>::CANON_WORDS;
    if (blockIdx.x >= count || threadIdx.x >= LPB) return;
    Jacobian<F> j = xyzz_to_jacobian(xyzz_load<F>(winsum + (size_t)blockIdx.x * (4 * NL)));
    uint32_t *out = outs[blockIdx.x];
    FieldOps<F>::to_canonical(out, j.X);
    FieldOps<F>::to_canonical(out + CW, j.Y);
    FieldOps<F>::to_canonical(out + 2 * CW, j.Z);
}

// ---- host side ------------------------------------------------------------------------------------
// Each fact has one home.  msm_call_plan settles a call before its first launch (MsmCall) and touches nothing; MsmBuffers, MsmFoldBuffers,
// MsmBatchArea, FixedMulBuffers and BasesTmp each declare a workspace ONCE as layout(arena), walked by ws_bytes to size it and by ws_place
// (ctx.hpp) to hand it out and check the walk against the reservation; msm_stages enqueues an MSM up to its merged buckets for both entries
// (msm_run_t, msm_batch_member); msm_tail is the only place that launches msm_bucket_red and msm_window_sum, with the shape msm_tail_geom gives
// and the final kernel of its caller.

// Buckets per tail lane (segment length L).  Every operation of the tail is a full addition or doubling on a chain: a
// segment costs 2 L (running sums) + ~38 (the multiple seg L, a 20-bit double-and-add whose additions run on every step of
// a diverged wave) + 8 (LDS tree) dependent operations, each ~13.6 us on one lane, 9.2 us on a lane pair (fu_pair.hpp).
// Measured (tools/msm_profile.py, 2^19 buckets, G1): one lane per bucket L = 8: 0.84 ms, 16: 1.06, 4: 1.38; lane pairs
// L = 16: 0.72, 8: 0.92 (two waves per SIMD: the operations slow down more than the chain shortens).
inline uint32_t msm_tail_segment(const zkhip_ctx *ctx, uint32_t B, size_t sets, int lanes_per_point) {
    uint32_t L = 1;
    if (ctx->opt_msm_segment_log >= 0) L = 1u << std::min(ctx->opt_msm_segment_log, 8);
    else {
        const size_t lanes = sets * B * (size_t)lanes_per_point;
        // one wave per SIMD (2^16 lanes) is where an operation is fastest -- the lane-pair group law (fu_pair.hpp: 9.2 us per
        // operation alone on a SIMD, 14.8 us when two waves share it), G2's pair-split Fq2 likewise: L doubles up to 16 to get
        // there, and beyond only when the lanes would otherwise exceed ~4 waves per SIMD (batches of many MSMs)
        while (L < 16 && lanes / L > 65536) L <<= 1;
        while (L < 64 && lanes / L > 262144) L <<= 1;
    }
    return std::min(B, L);
}

// The launch shape of the tail over `sets` sets of B buckets.  Lane (TailLane<F>, QuadLane<F> or BucketLane<F>): what a lane holds and how
// many lanes share a point.
struct MsmTailGeom {
    uint32_t L, nseg;       // buckets per segment (= per point slot), segments per set
    uint32_t slots, nblk;   // point slots per msm_bucket_red workgroup, workgroups per set
    uint32_t wthreads;      // lanes of a msm_window_sum workgroup
    size_t lds_red, lds_win;  // dynamic LDS of the two kernels: one XYZZ point per slot
};
template <class Lane>
MsmTailGeom msm_tail_geom(const zkhip_ctx *ctx, uint32_t B, size_t sets) {
    constexpr size_t point_bytes = (size_t)4 * FieldOps<typename Lane::type>::WORDS * 4;
    constexpr int XL = Lane::LANES;
    MsmTailGeom t;
    t.L = msm_tail_segment(ctx, B, sets, XL);
    t.nseg = B / t.L;
    t.slots = MSM_TAIL_THREADS / XL;
    t.nblk = (t.nseg + t.slots - 1) / t.slots;
    t.wthreads = msm_window_threads(t.nblk, XL);
    t.lds_red = t.slots * point_bytes;  // 256 XYZZ points with one lane each: 56 KiB for G1, 128 KiB for BLS12-381 G2
    t.lds_win = t.wthreads / XL * point_bytes;
    return t;
}

// The tail, for every caller: sets[nsets][B] buckets -> segsum (room for segsum_blocks workgroup partials) -> winsum[nsets], then `final`,
// which launches the kernel that turns the set sums into results.
// (a variant of msm_bucket_red compiled for one-bucket segments only spills 37 instead of 173 registers and measures the same: 0.156 ms)
template <class Lane, class Final>
int msm_tail(zkhip_ctx *ctx, const uint32_t *sets, size_t nsets, uint32_t B, uint32_t *segsum, size_t segsum_blocks, uint32_t *winsum, Final final) {
    typedef typename Lane::type TX;
    constexpr int XL = Lane::LANES;
    const MsmTailGeom t = msm_tail_geom<Lane>(ctx, B, nsets);
    if (nsets * t.nblk > segsum_blocks) {
        ctx->last_error = "MSM tail of " + std::to_string(nsets * t.nblk) + " workgroups over a partial-sum buffer for " + std::to_string(segsum_blocks);
        return ZKHIP_ERR_RANGE;
    }
    ZK_MAX_LDS(ctx, (msm_bucket_red<TX, XL>), t.lds_red);
    ZK_LAUNCH(ctx, "msm_bucket_red", (msm_bucket_red<TX, XL>), dim3((unsigned)(nsets * t.nblk)), dim3(MSM_TAIL_THREADS), t.lds_red, sets, B, t.L, t.nseg, t.nblk,
              segsum);
    ZK_LAUNCH(ctx, "msm_window_sum", (msm_window_sum<TX, XL>), dim3((unsigned)nsets), dim3(t.wthreads), t.lds_win, segsum, t.nblk, winsum);
    return final();
}

// ---- the two-level tail on the host: buffers and launches --------------------------------------------------------------------
// Applies to merged bucket sets with window tables (ONE set per MSM) of at least 2^opt_msm_tail_fold buckets whose rows and columns fit a workgroup.
// G2 (lane pairs throughout): a lone 2^20-point MSM measures the same either way (tail 1.94 against 1.97 ms), but the two levels are HALF the
// additions, and a Groth16 proof runs its G2 MSM under the G1 MSMs, which take the issue slots (50.7-51.0 -> 51.9-52.4 M constraints/s, A/B on
// one box, three times interleaved): on by default, with its own switch msm_tail_fold_g2.
template <class F>
bool msm_fold_applies(const zkhip_ctx *ctx, uint32_t B, bool tables) {
    if (FieldOps<F>::WORDS > 16 && !ctx->opt_msm_tail_fold_g2) return false;
    if (!tables || ctx->opt_msm_tail_fold <= 0 || B < (1u << std::min(ctx->opt_msm_tail_fold, 30))) return false;
    const MsmFold g = msm_fold_geom(ctx, B);
    const uint32_t sa = MSM_TAIL_THREADS / BucketLane<F>::LANES;
    return g.m_col >= 1 && g.m_row <= sa && g.m_col <= sa && B >= sa * g.run && g.m_row * g.run == g.C && g.m_col * g.run == g.R;
}
template <class F>
struct MsmFoldBuffers {
    static constexpr size_t PW = (size_t)4 * FieldOps<F>::WORDS;  // words per XYZZ point
    MsmFold g{};
    size_t nsets = 0;
    uint32_t *level2 = nullptr, *segsum = nullptr, *winsum = nullptr;
    MsmFoldBuffers() = default;
    MsmFoldBuffers(const zkhip_ctx *ctx, uint32_t B, size_t nsets_) : g(msm_fold_geom(ctx, B)), nsets(nsets_) {}
    size_t level2_words() const { return nsets * 2 * g.C * PW; }
    // segments of >= 1 bucket, >= 64 of them per workgroup; the wide tail (lone MSM): a partial per MSM_WIDE_WAVES points
    size_t segsum_blocks() const { return nsets * 2 * std::max<size_t>((g.C + 63) / 64, WideLane<F>::AVAILABLE && nsets == 1 ? g.C / MSM_WIDE_WAVES : 0); }
    template <class Arena>
    void layout(Arena &a) {
        a.take(level2, level2_words());
        a.take(segsum, segsum_blocks() * PW);
        a.take(winsum, nsets * 2 * PW);
    }
};

// Level 2 on the wide lane: level2[2 nsets][C] -> nsets canonical Jacobian results.  The partial sums alternate between segsum and level2 (whose
// points msm_wide_weigh has read by then).  Applies to the LONE MSM (2 C waves: two per SIMD at C = 2^10) where a set holds at least a workgroup's
// points.  A batch keeps the quads / pairs: its level 2 has waves enough to fill the chip, and there an operation's issue slots count, not its latency.
template <class F>
bool msm_tail_wide_applies(const zkhip_ctx *ctx, size_t nsets, uint32_t C) {
    return WideLane<F>::AVAILABLE && ctx->opt_msm_tail_quads == 1 && nsets == 1 && C >= MSM_WIDE_WAVES;
}
template <class F>
int msm_tail_wide(zkhip_ctx *ctx, const MsmFoldBuffers<F> &fb, uint32_t *const *d_outs, uint32_t *d_out) {
    if constexpr (WideLane<F>::AVAILABLE) {
        typedef typename F::params U;
        const uint32_t C = fb.g.C;
        const size_t sets = 2 * fb.nsets;
        uint32_t m = C / MSM_WIDE_WAVES;  // partials per set
        if (sets * m > fb.segsum_blocks()) {
            ctx->last_error = "wide MSM tail of " + std::to_string(sets * m) + " workgroups over a partial-sum buffer for " + std::to_string(fb.segsum_blocks());
            return ZKHIP_ERR_RANGE;
        }
        uint32_t *from = fb.segsum, *to = fb.level2;
        ZK_LAUNCH(ctx, "msm_wide_weigh", (msm_wide_weigh<U>), dim3((unsigned)(sets * m)), dim3(MSM_WIDE_WAVES * 64), 0, fb.level2, C, from);
        while (m > MSM_WIDE_WAVES) {
            m /= 2 * MSM_WIDE_WAVES;
            ZK_LAUNCH(ctx, "msm_wide_tree", (msm_wide_tree<U>), dim3((unsigned)(sets * m)), dim3(MSM_WIDE_WAVES * 64), 0, from, to);
            std::swap(from, to);
        }
        ZK_LAUNCH(ctx, "msm_wide_final", (msm_wide_final<U>), dim3((unsigned)fb.nsets), dim3(MSM_WIDE_WAVES * 64), 0, from, m, fb.g.log_c, d_outs, d_out);
        return 0;
    } else {
        (void)fb, (void)d_outs, (void)d_out;
        ctx->last_error = "no wide lane for this field";
        return ZKHIP_ERR_INVALID;
    }
}

// sets[nsets][B] merged buckets -> nsets canonical Jacobian results (d_outs: device array of output pointers, or the one output d_out):
// msm_fold, then the tail over the 2 nsets level-2 sets.  Lane: the lane shape of that tail when the quads do not apply.
template <class F, class Lane>
int msm_fold_tail(zkhip_ctx *ctx, const uint32_t *sets, const MsmFoldBuffers<F> &fb, uint32_t *const *d_outs, uint32_t *d_out) {
    constexpr int NL = FieldOps<F>::WORDS;
    typedef typename BucketLane<F>::type FL;
    constexpr int LPB = BucketLane<F>::LANES;
    typedef typename QuadLane<F>::type TQ;  // the trees are latency: quads where the field has them (else this IS the tail lane)
    constexpr int QL = QuadLane<F>::LANES;
    const MsmFold &g = fb.g;
    const size_t nsets = fb.nsets;
    const size_t lds = (size_t)MSM_TAIL_THREADS / LPB * 4 * NL * 4;
    ZK_MAX_LDS(ctx, (msm_fold<FL, LPB, TQ, QL>), lds);
    ZK_LAUNCH(ctx, "msm_fold", (msm_fold<FL, LPB, TQ, QL>), dim3((unsigned)(nsets * (g.B / (MSM_TAIL_THREADS / LPB * g.run)) * 2)), dim3(MSM_TAIL_THREADS), lds,
              sets, g, fb.level2);
    auto level2 = [&](auto lane) -> int {  // the tail over the level-2 sets with one lane shape
        typedef decltype(lane) X;
        return msm_tail<X>(ctx, fb.level2, 2 * nsets, g.C, fb.segsum, fb.segsum_blocks(), fb.winsum, [&]() -> int {
            ZK_LAUNCH(ctx, "msm_final", (msm_final_fold<typename X::type, X::LANES>), dim3((unsigned)nsets), dim3(64), 0, fb.winsum, (uint32_t)nsets, g.log_c, d_outs, d_out);
            return 0;
        });
    };
    if (msm_tail_wide_applies<F>(ctx, nsets, g.C)) return msm_tail_wide<F>(ctx, fb, d_outs, d_out);
    if (QuadLane<F>::AVAILABLE && ctx->opt_msm_tail_quads && 2 * nsets * g.C <= ((size_t)1 << 18)) return level2(QuadLane<F>());
    return level2(Lane());
}

// Everything one MSM call settles before its first launch.  msm_call_plan fills it from the context's options and the bases object and
// touches neither; the workspace (MsmBuffers) and every grid below are functions of it.
// The entries' part (msm_entries.hpp: window geometry MsmPlan, SortGeom, the sort's and the large-bucket plan's sizes) needs no field; the tail's does.
struct MsmCall : MsmEntriesCall {
    int Sr;                       // sets left after the equal-weight merge = sets the tail sees
    uint32_t segsum_blocks;       // msm_bucket_red workgroups per set, the most over the lane shapes the tail may take
    bool fold;                    // the two-level tail applies (never to a batch member: batches fold once, for all members -- msm_batch_tail)
};

template <class F>
int msm_call_plan(const zkhip_ctx *ctx, const zkhip_bases *bases, size_t offset, size_t n, bool batch_member, MsmCall &c, std::string &error) {
    ZK_TRY(zk_msm_entries_plan(ctx, bases, offset, n, c, error));
    const MsmPlan &P = c.P;
    c.Sr = P.tables ? 1 : P.W;
    // the quad variant of the tail (msm_run_t) may cut the set into more workgroups than the default one: the partial-sum buffer holds either
    c.segsum_blocks = std::max(msm_tail_geom<TailLane<F>>(ctx, P.B, c.Sr).nblk, msm_tail_geom<QuadLane<F>>(ctx, P.B, c.Sr).nblk);
    c.fold = !batch_member && msm_fold_applies<F>(ctx, P.B, P.tables);
    return 0;
}

// The per-call workspace of one MSM, in the order it lies in memory.  The buffers of the entries stage are the MsmEntriesBuffers sub-object.
template <class F>
struct MsmBuffers : MsmEntriesBuffers {
    static constexpr size_t PW = (size_t)4 * FieldOps<F>::WORDS;  // words per XYZZ point
    const MsmCall &c;
    uint32_t *buckets;
    uint32_t *segsum, *winsum;
    MsmFoldBuffers<F> fb;
    uint32_t *partials;  // large buckets: the tasks' partial sums
    MsmBuffers(const zkhip_ctx *ctx, const MsmCall &call) : c(call) {
        if (c.fold) fb = MsmFoldBuffers<F>(ctx, c.P.B, 1);
    }
    template <class Arena>
    void layout(Arena &a) {
        a.take(dig, c.entries());
        a.take(bh, c.nbh);
        a.take(bo, (size_t)c.nbh + 1);
        a.take(bsums, (c.nbh + 1023) / 1024);
        a.take(tmp_idx, c.entries());
        a.take(tmp_key, c.entries());
        a.take(offs, (size_t)c.P.nb + 1);
        a.take(idx, c.entries());
        a.take(buckets, c.P.nb * PW);
        a.take(sh, (size_t)c.nsh + 1);
        a.take(so, (size_t)c.nsh + 1);
        a.take(ssums, (c.nsh + 1023) / 1024);
        a.take(order, c.P.nb);
        a.take(segsum, (size_t)c.Sr * c.segsum_blocks * PW);
        a.take(winsum, (size_t)std::max(1, c.Sr) * PW);
        if (c.fold) fb.layout(a);
        a.take(plan, 4);
        a.take(tasks, (size_t)c.task_cap * 3);
        a.take(large, (size_t)c.large_cap * 3);
        a.take(partials, c.task_cap * PW);
    }
};

// The stages of one MSM up to the merged buckets: digits, sort, size order, accumulation, large buckets, merge of the equal-weight sets.
// reuse_sort (batches: the previous member had the SAME scalars over an entry-compatible bases object -- msm_same_entries): the
// sorted entries, bucket offsets, size order and large-bucket plan in the workspace are this member's too (same sizes, so the same
// addresses); only the gathers read another table
template <class F>
int msm_stages(zkhip_ctx *ctx, const zkhip_bases *bases, const MsmCall &c, const MsmBuffers<F> &w, const uint32_t *d_scalars, bool reuse_sort) {
    constexpr int NL = FieldOps<F>::WORDS;
    typedef typename BucketLane<F>::type FL;   // what a lane holds in the bucket kernels
    constexpr int LPB = BucketLane<F>::LANES;  // lanes per point (2 for G2: fu2_pair.hpp)
    const MsmPlan &P = c.P;
    const uint32_t nb = P.nb;
    const uint32_t *d_b = bases->d;  // entries address table rows from the start of the bases object
    if (!reuse_sort) ZK_TRY(zk_msm_entries(ctx, bases->curve, c, w, d_scalars));  // digits, sort, buckets by descending size
    if constexpr (FieldOps<F>::WORDS <= 16) {
        // G1: accumulator coordinates in LDS, three waves per SIMD
        constexpr int NT = MSM_G1_THREADS;
        size_t lds_acc = LdsAcc<F, NT>::BYTES;
        ZK_MAX_LDS(ctx, (msm_bucket_acc_lds<F, NT, 3>), lds_acc);
        ZK_LAUNCH(ctx, "msm_bucket_acc", (msm_bucket_acc_lds<F, NT, 3>), dim3((nb + NT - 1) / NT), dim3(NT), lds_acc, d_b, w.offs, w.idx, nb, c.large_thresh,
                  w.order, w.buckets);
    } else {
        // G2: every bucket is an even / odd lane pair, each lane holding one component of the Fq2 coordinates
        // (fu2_pair.hpp): a lane then carries what a G1 lane carries -- two waves per SIMD instead of one.
        constexpr int NT = MSM_G2_THREADS, WAVES = MSM_G2_WAVES;
        size_t lds_acc = LdsAcc<FL, NT>::BYTES;
        ZK_MAX_LDS(ctx, (msm_bucket_acc_lds<FL, NT, WAVES, LPB>), lds_acc);
        ZK_LAUNCH(ctx, "msm_bucket_acc", (msm_bucket_acc_lds<FL, NT, WAVES, LPB>), dim3((unsigned)(((size_t)nb * LPB + NT - 1) / NT)), dim3(NT), lds_acc, d_b,
                  w.offs, w.idx, nb, c.large_thresh, w.order, w.buckets);
    }
    // large buckets: plan on the device (no host round trip), then fixed-size grids that read the plan
    if (!reuse_sort) ZK_TRY(zk_msm_large_plan(ctx, c, w));
    {
        size_t lds_large = (size_t)128 / LPB * 4 * NL * 4;
        if (lds_large > 48 * 1024) ZK_MAX_LDS(ctx, (msm_bucket_large<FL, LPB>), lds_large);
        unsigned grid_large = (unsigned)std::min<size_t>(c.task_cap, 512);  // persistent: workgroups loop over the task list
        ZK_LAUNCH(ctx, "msm_bucket_large", (msm_bucket_large<FL, LPB>), dim3(grid_large), dim3(128), lds_large, d_b, w.idx, w.plan, w.tasks, w.partials);
        ZK_LAUNCH(ctx, "msm_bucket_large", (msm_large_combine<FL, LPB>), dim3((unsigned)std::min<uint32_t>(c.large_cap, 256)), dim3(64),
                  (size_t)64 / LPB * 4 * NL * 4, w.plan, w.large, w.partials, w.buckets);
    }
    if (P.tables) {
        for (uint32_t cur = P.S; cur > 1;) {
            const uint32_t q = (cur + 3) / 4;
            ZK_LAUNCH(ctx, "msm_bucket_merge", (msm_bucket_merge<FL, LPB>), grid_1d((size_t)q * P.B * LPB), dim3(256), 0, w.buckets, P.B, q,
                      cur);
            cur = q;
        }
    }
    return 0;
}

// one MSM: plan, workspace, stages, tail
template <class F>
int msm_run_t(zkhip_ctx *ctx, const zkhip_bases *bases, size_t offset, size_t n, const uint32_t *d_scalars, uint32_t *d_out_jac) {
    MsmCall c;
    ZK_TRY(msm_call_plan<F>(ctx, bases, offset, n, false, c, ctx->last_error));
    MsmBuffers<F> w(ctx, c);
    ZK_TRY(ws_place(ctx, w));
    ZK_TRY(msm_stages<F>(ctx, bases, c, w, d_scalars, false));
    if (c.fold) return msm_fold_tail<F, TailLane<F>>(ctx, w.buckets, w.fb, nullptr, d_out_jac);
    // without tables the sets are the windows: Horner over them in msm_final
    auto tail = [&](auto lane) -> int {  // (in the tail a G1 lane holds half a point: the group law over a lane pair, fu_pair.hpp)
        typedef decltype(lane) X;
        return msm_tail<X>(ctx, w.buckets, (size_t)c.Sr, c.P.B, w.segsum, (size_t)c.Sr * c.segsum_blocks, w.winsum, [&]() -> int {
            ZK_LAUNCH(ctx, "msm_final", (msm_final<typename X::type, X::LANES>), dim3(1), dim3(64), 0, w.winsum, c.Sr, c.P.win, d_out_jac);
            return 0;
        });
    };
    // Small bucket sets leave lanes to spare even as pairs: the group law then runs over lane QUADS (fu_quad.hpp: 4 product steps per
    // addition instead of 7) with segments twice as long -- from 2^18 buckets down; at 2^19 the longer segments eat the gain.
    if (QuadLane<F>::AVAILABLE && ctx->opt_msm_tail_quads && (size_t)c.Sr * c.P.B <= ((size_t)1 << 18)) return tail(QuadLane<F>());
    return tail(TailLane<F>());
}

// one member of a batch: the stages into `slot` (B buckets of the batch area); the tail runs once for the whole batch.
template <class F>
int msm_batch_member(zkhip_ctx *ctx, const zkhip_bases *bases, size_t offset, size_t n, const uint32_t *d_scalars, uint32_t *slot, bool reuse_sort) {
    MsmCall c;
    ZK_TRY(msm_call_plan<F>(ctx, bases, offset, n, true, c, ctx->last_error));
    MsmBuffers<F> w(ctx, c);
    ZK_TRY(ws_place(ctx, w));
    if (c.P.S == 1) w.buckets = slot;  // ONE set: accumulate straight into the slot (no copy of 2^19 buckets = 117 MB)
    ZK_TRY(msm_stages<F>(ctx, bases, c, w, d_scalars, reuse_sort));
    if (w.buckets != slot) ZK_HIP_CHECK(ctx, hipMemcpyAsync(slot, w.buckets, c.P.B * MsmBuffers<F>::PW * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

struct BasesTmp {  // bases_precompute_range's parked points: 5 field elements per (kept window, point of the largest chunk)
    size_t words;
    uint32_t *tmp;
    template <class Arena>
    void layout(Arena &a) { a.take(tmp, words); }
};

// Build the window tables of a bases object whose slot 0 (the points) is filled (called once at upload).
template <class F>
int bases_precompute_t(zkhip_ctx *ctx, zkhip_bases *b) {
    constexpr int NL = FieldOps<F>::WORDS;
    if (!b->tables() || b->n == 0) return 0;
    const size_t chunk = 1u << 18;  // bounds the temporary to kept * 2^18 * 5 field elements
    const int kept = b->local_windows() - (b->win_rank == 0 ? 1 : 0);  // window 0 is the points themselves
    if (kept <= 0) return 0;
    BasesTmp w = {(size_t)kept * 5 * NL * std::min(chunk, b->n), nullptr};  // every chunk parks its points in the same place
    ZK_TRY(ws_place(ctx, w));
    uint32_t *tmp = w.tmp;
    for (size_t lo = 0; lo < b->n; lo += chunk) {
        size_t cnt = std::min(chunk, b->n - lo);
        ZK_LAUNCH(ctx, "bases_precompute", bases_precompute_range<F>, grid_1d(cnt, 64), dim3(64), 0, b->d, (uint32_t)b->n,
                  (uint32_t)lo, (uint32_t)cnt, msm_make_windows(zk_scalar_bits(b->curve), b->ntab), (uint32_t)b->win_rank, (uint32_t)b->win_world, tmp);
    }
    return 0;
}

// Do two members of a batch produce the same sorted entries?  An entry is (bucket of the digit, table row of the point): the same
// scalars, range and table geometry give the same list whatever the points are -- the queries of one Groth16 proof that run over the
// same assignment vector (A, the dense B.h, the padded L) then share one digit extraction, sort, size order and large-bucket plan.
inline bool msm_same_entries(const zkhip_bases *a, size_t off_a, size_t n_a, const uint32_t *s_a, const zkhip_bases *b, size_t off_b, size_t n_b,
                             const uint32_t *s_b) {
    return s_a == s_b && n_a == n_b && off_a == off_b && a->curve == b->curve && a->n == b->n && a->c_tab == b->c_tab && a->ntab == b->ntab &&
           a->win_rank == b->win_rank && a->win_world == b->win_world && a->nslots == b->nslots && a->tables() && b->tables();
}

template <class F>
struct MsmBatchArea {  // below the members' workspaces: a bucket set per member, the shared tail's sums, the output pointers
    static constexpr size_t PW = MsmBuffers<F>::PW;
    size_t count, slot_words, segsum_blocks;
    bool fold;
    uint32_t *slots, *segsum, *winsum, **d_ptrs;
    MsmFoldBuffers<F> fb;
    template <class Arena>
    void layout(Arena &a) {
        a.take(slots, count * slot_words);
        a.take(segsum, segsum_blocks * PW);
        a.take(winsum, count * PW);
        a.take(d_ptrs, count);
        if (fold) fb.layout(a);
    }
};

// Several MSMs over table-backed bases of one group with one window size: per MSM digits / sort / accumulate /
// merge as usual, then ONE bucket reduction, set sum and output conversion for the whole batch.
// Lane: what a lane of the shared tail holds.  A few members: the latency-bound shape of a single MSM (G1: the group law over
// lane pairs).  Many members (50 KZG columns x 2^19 buckets) have lanes to spare and are bound by WORK: one lane per point then
// does the same additions without the pair's selects and DPP swaps (measured: msm_bucket_red of a 50-column 2^20-row commit
// 16.2 -> 13.7 ms).
template <class F, class Lane>
int msm_batch_tail(zkhip_ctx *ctx, size_t count, const zkhip_bases *const *bases, const size_t *offsets, const size_t *ns,
                   const uint32_t *const *d_scalars, uint32_t *const *d_outs) {
    const uint32_t B = 1u << (bases[0]->c_tab - 1);
    // the members' own workspaces follow the batch area, one after the other in the same place.  Each is sized as the lone call it would be (the
    // fold buffers of one set more than a member takes), which keeps the reservation, and so every address, where it has always been
    size_t max_need = 0;
    for (size_t i = 0; i < count; ++i) {
        if (ns[i] == 0 || bases[i]->local_windows() == 0) continue;
        MsmCall c;
        ZK_TRY(msm_call_plan<F>(ctx, bases[i], offsets[i], ns[i], false, c, ctx->last_error));
        MsmBuffers<F> w(ctx, c);
        max_need = std::max(max_need, ws_bytes(w));
    }
    MsmBatchArea<F> area;
    area.count = count;
    area.slot_words = B * area.PW;
    area.segsum_blocks = count * msm_tail_geom<Lane>(ctx, B, count).nblk;
    area.fold = msm_fold_applies<F>(ctx, B, true);
    if (area.fold) area.fb = MsmFoldBuffers<F>(ctx, B, count);
    ctx->ws_floor = 0;
    ZK_TRY(ws_place(ctx, area, max_need));
    uint32_t *const slots = area.slots;
    const size_t slot_words = area.slot_words;
    uint32_t **d_ptrs = area.d_ptrs;
    ctx->ws_floor = ctx->ws_off;  // the per-MSM stages bump-allocate above the batch area
    int rc = 0;
    size_t prev = (size_t)-1;  // the member whose sort the workspace holds
    for (size_t i = 0; i < count && rc == 0; ++i) {
        if (ns[i] == 0 || bases[i]->local_windows() == 0) {
            hipError_t e = hipMemsetAsync(slots + i * slot_words, 0, slot_words * 4, ctx->stream);  // all buckets at infinity
            if (e != hipSuccess) rc = ZKHIP_ERR_HIP;
        } else {
            const bool reuse = ctx->opt_msm_share_sort && prev != (size_t)-1 &&
                               msm_same_entries(bases[prev], offsets[prev], ns[prev], d_scalars[prev], bases[i], offsets[i], ns[i], d_scalars[i]);
            rc = msm_batch_member<F>(ctx, bases[i], offsets[i], ns[i], d_scalars[i], slots + i * slot_words, reuse);
            prev = i;
        }
    }
    ctx->ws_floor = 0;
    if (rc) return rc;
    if (ctx->batch_dptrs_override) {  // graph capture: the output pointers already sit in a device array owned by the graph
        d_ptrs = static_cast<uint32_t **>(ctx->batch_dptrs_override);
    } else {
        ZK_TRY(ws_upload(ctx, d_ptrs, d_outs, count * sizeof(void *)));
    }
    if (area.fold) return msm_fold_tail<F, Lane>(ctx, slots, area.fb, d_ptrs, nullptr);
    return msm_tail<Lane>(ctx, slots, count, B, area.segsum, area.segsum_blocks, area.winsum, [&]() -> int {
        ZK_LAUNCH(ctx, "msm_final", (msm_final_batch<typename Lane::type, Lane::LANES>), dim3((unsigned)count), dim3(64), 0, area.winsum, (uint32_t)count, d_ptrs);
        return 0;
    });
}

template <class F>
int msm_batch_t(zkhip_ctx *ctx, size_t count, const zkhip_bases *const *bases, const size_t *offsets, const size_t *ns,
                const uint32_t *const *d_scalars, uint32_t *const *d_outs) {
    const size_t buckets = count << (bases[0]->c_tab - 1);
    // >= 2^21 buckets in all (the four G1 multiexps of a proof: msm_bucket_red 2.16 -> 1.87 ms; 50 KZG columns: 16.2 -> 13.7):
    // the one-lane shape keeps every SIMD busy by itself -- work-bound
    if (!std::is_same<typename BucketLane<F>::type, typename TailLane<F>::type>::value && buckets >= ((size_t)1 << 21))
        return msm_batch_tail<F, BucketLane<F>>(ctx, count, bases, offsets, ns, d_scalars, d_outs);
    return msm_batch_tail<F, TailLane<F>>(ctx, count, bases, offsets, ns, d_scalars, d_outs);
}

// ---- the per-(curve, group) operation table ----------------------------------------------------------------------
template <class F>
int op_to_mont(zkhip_ctx *ctx, zkhip_bases *b, const uint32_t *d_canonical, const uint8_t *d_inf) {
    ZK_LAUNCH(ctx, "bases_to_mont", bases_to_mont<F>, grid_1d(b->n), dim3(256), 0, d_canonical, d_inf, (uint32_t)b->n, b->d);
    return 0;
}
template <class F>
int op_from_mont(zkhip_ctx *ctx, const zkhip_bases *b, size_t offset, size_t n, uint32_t *d_out, uint8_t *d_inf) {
    const uint32_t *src = b->d + offset * b->stride_u32;
    ZK_LAUNCH(ctx, "bases_from_mont", bases_from_mont<F>, grid_1d(n), dim3(256), 0, src, (uint32_t)n, d_out, d_inf);
    return 0;
}
template <class F>
struct FixedMulBuffers {  // the table, and five field elements per table entry (while it is built) or per point (afterwards)
    size_t n;
    uint32_t *tab, *tmp;
    template <class Arena>
    void layout(Arena &a) {
        a.take(tab, (size_t)FIXED_NW * FIXED_ROW * 2 * FieldOps<F>::WORDS);
        a.take(tmp, std::max<size_t>((size_t)FIXED_NW * FIXED_ROW, n) * 5 * FieldOps<F>::WORDS);
    }
};
template <class F>
int op_mul(zkhip_ctx *ctx, zkhip_bases *b, const uint32_t *d_base_canonical, const uint32_t *d_scalars) {
    if (b->n < 4096) {  // a handful of points: the table would cost more than it saves
        ZK_LAUNCH(ctx, "bases_mul", bases_mul<F>, grid_1d(b->n, 64), dim3(64), 0, b->d, d_base_canonical, d_scalars, (uint32_t)b->n);
        return 0;
    }
    // fixed-base windows: a 32 x 256-entry affine table of the base, then <= 32 mixed additions per point (round 4: a 2^20-constraint
    // key's batch exponentiations were 256 doublings + ~128 additions + one Fermat inversion PER POINT)
    FixedMulBuffers<F> w = {b->n, nullptr, nullptr};
    ZK_TRY(ws_place(ctx, w));
    uint32_t *tab = w.tab, *tmp = w.tmp;
    ZK_LAUNCH(ctx, "bases_mul", bases_fixed_table<F>, dim3(1), dim3(64), 0, d_base_canonical, tab, tmp);
    const size_t lanes = (b->n + FIXED_CHUNK - 1) / FIXED_CHUNK;
    ZK_LAUNCH(ctx, "bases_mul", bases_mul_fixed<F>, grid_1d(lanes, 64), dim3(64), 0, b->d, tab, d_scalars, (uint32_t)b->n, tmp);
    return 0;
}
template <class F>
int op_jac_to_affine(zkhip_ctx *ctx, const uint32_t *d_jac, uint32_t *d_aff, uint8_t *d_inf) {
    ZK_LAUNCH(ctx, "jac_to_affine", jac_to_affine_k<F>, dim3(1), dim3(64), 0, d_jac, d_aff, d_inf);
    return 0;
}
template <class F>
int op_jac_sum(zkhip_ctx *ctx, const uint32_t *d_pts, size_t count, uint32_t *d_out) {
    ZK_LAUNCH(ctx, "jac_sum", jac_sum_k<F>, dim3(1), dim3(64), 0, d_pts, (uint32_t)count, d_out);
    return 0;
}
template <class F>
int op_write_infinity(zkhip_ctx *ctx, uint32_t *d_out_jac) {
    ZK_LAUNCH(ctx, "msm_write_infinity", msm_write_infinity<F>, dim3(1), dim3(64), 0, d_out_jac);
    return 0;
}

template <class F>
const MsmOps *msm_make_ops() {
    static const MsmOps ops = {msm_run_t<F>,        msm_batch_t<F>,      bases_precompute_t<F>, op_to_mont<F>,        op_from_mont<F>, op_mul<F>,
                               op_jac_to_affine<F>, op_jac_sum<F>, op_write_infinity<F>, (size_t)2 * FieldOps<F>::WORDS};
    return &ops;
}

}  // namespace
