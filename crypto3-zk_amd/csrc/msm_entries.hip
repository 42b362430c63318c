// The field-free first stage of every MSM, compiled once (interface: msm_entries.hpp; the per-(curve, group) units call it from msm_core.hpp's
// msm_stages).  No kernel here looks at a coordinate.
//   msm_digits_only   scalar -> signed digits                           (streams 32 B/scalar, coalesced)
//   msm_sort_*        two-level counting sort of the entries by (set, bucket), counters in LDS only, tiles staged in LDS
//   msm_scan_*        exclusive prefix (local scan, top scan, add-back), shared by both sorts; every LDS scan is block_inclusive_scan
//   msm_size_*        order of the buckets by descending size
//   msm_plan_large    buckets far above the mean, cut into 4096-entry tasks for msm_bucket_large / msm_large_combine (msm_core.hpp)
// Point order inside a bucket depends on LDS-atomic arrival order; nothing else about the buffers does.
#include <algorithm>
#include <string>

#include "ctx.hpp"
#include "fu.hpp"
#include "msm_entries.hpp"
#include "msm_ops.hpp"
#include "msm_recode.hpp"

namespace {

using namespace zkhip;

constexpr uint32_t MSM_LARGE_BUCKET = 128;  // buckets above this many entries (and 4 x the mean) are split across workgroups
constexpr uint32_t MSM_LARGE_CHUNK = 4096;  // entries per task of a split bucket

// Hillis-Steele inclusive scan over one LDS word per lane, in place; every lane has written its own word
template <uint32_t THREADS>
ZK_D void block_inclusive_scan(uint32_t *scratch) {
    const uint32_t t = threadIdx.x;
    __syncthreads();
    for (uint32_t d = 1; d < THREADS; d <<= 1) {
        uint32_t x = t >= d ? scratch[t - d] : 0;
        __syncthreads();
        scratch[t] += x;
        __syncthreads();
    }
}

// exclusive scan of `count` u32 counters in three launches: per-block (1024 counters) local scan + block
// totals, scan of the totals by one workgroup, add-back.  offs[count] = total; cursor = copy of offs.
__global__ __launch_bounds__(256) void msm_scan_local(const uint32_t *__restrict__ hist, uint32_t count, uint32_t *__restrict__ offs,
                                                      uint32_t *__restrict__ block_sums) {
    __shared__ uint32_t part[256];
    const uint32_t t = threadIdx.x, base = blockIdx.x * 1024 + t * 4;
    uint32_t v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = base + k < count ? hist[base + k] : 0;
        s += v[k];
    }
    part[t] = s;
    block_inclusive_scan<256>(part);
    uint32_t run = part[t] - s;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < count) offs[base + k] = run;
        run += v[k];
    }
    if (t == 255) block_sums[blockIdx.x] = part[255];
}

__global__ __launch_bounds__(1024) void msm_scan_top(uint32_t *__restrict__ block_sums, uint32_t nblocks, uint32_t *__restrict__ total) {
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nblocks + 1023) / 1024;
    const uint32_t lo = min(nblocks, t * per), hi = min(nblocks, lo + per);
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += block_sums[i];
    part[t] = s;
    block_inclusive_scan<1024>(part);
    uint32_t run = part[t] - s;
    for (uint32_t i = lo; i < hi; ++i) {
        uint32_t x = block_sums[i];
        block_sums[i] = run;
        run += x;
    }
    if (t == 1023) *total = part[1023];
}

__global__ __launch_bounds__(256) void msm_scan_add(uint32_t *__restrict__ offs, uint32_t count, const uint32_t *__restrict__ block_sums,
                                                    uint32_t *__restrict__ cursor) {
    const uint32_t base = blockIdx.x * 1024 + threadIdx.x * 4;
    const uint32_t add = block_sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < count) {
            uint32_t x = offs[base + k] + add;
            offs[base + k] = x;
            cursor[base + k] = x;
        }
    }
}

// the same three steps in ONE launch for short arrays (small MSMs are bound by launch gaps, not by work): one workgroup walks the
// array in 1024-counter strips, carrying the running total
__global__ __launch_bounds__(1024) void msm_scan_single(const uint32_t *__restrict__ hist, uint32_t count, uint32_t *__restrict__ offs,
                                                        uint32_t *__restrict__ cursor) {
    __shared__ uint32_t part[1024];
    __shared__ uint32_t carry;
    const uint32_t t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < count; base += 1024) {
        const uint32_t v = base + t < count ? hist[base + t] : 0;
        part[t] = v;
        block_inclusive_scan<1024>(part);
        const uint32_t excl = carry + part[t] - v;
        if (base + t < count) {
            offs[base + t] = excl;
            if (cursor != offs) cursor[base + t] = excl;
        }
        __syncthreads();
        if (t == 1023) carry += part[1023];
        __syncthreads();
    }
    if (t == 0) offs[count] = carry;
}
constexpr uint32_t MSM_SCAN_SINGLE_MAX = 1u << 16;

// exclusive scan of hist[0 .. count) into offs[0 .. count], offs[count] = total (bsums: scratch for the three-launch form)
inline int msm_scan(zkhip_ctx *ctx, const char *name, const uint32_t *hist, uint32_t count, uint32_t *offs, uint32_t *bsums) {
    if (count <= MSM_SCAN_SINGLE_MAX) {
        ZK_LAUNCH(ctx, name, msm_scan_single, dim3(1), dim3(1024), 0, hist, count, offs, offs);
        return 0;
    }
    const uint32_t nblk = (count + 1023) / 1024;
    ZK_LAUNCH(ctx, name, msm_scan_local, dim3(nblk), dim3(256), 0, hist, count, offs, bsums);
    ZK_LAUNCH(ctx, name, msm_scan_top, dim3(1), dim3(1024), 0, bsums, nblk, offs + count);
    ZK_LAUNCH(ctx, name, msm_scan_add, dim3(nblk), dim3(256), 0, offs, count, bsums, offs);
    return 0;
}

// Window partition (wrank of wworld): the carry chain runs over all windows, only the digits of windows
// w = wrank + k wworld are kept, as local window k.
template <class FR>
__global__ __launch_bounds__(256) void msm_digits_only(const uint32_t *__restrict__ scalars, uint32_t n, MsmWindows win, uint32_t wrank,
                                                       uint32_t wworld, uint32_t *__restrict__ dig) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t s[8];
    const uint32_t flip = msm_fold_scalar<FR>(scalars + (size_t)i * 8, s) ? 0x80000000u : 0u;  // |s| <= (r - 1) / 2
    uint32_t carry = 0, next = wrank, lw = 0;
    for (int w = 0; w < win.W; ++w) {
        uint32_t d = msm_recode(s, win.off(w), win.width(w), carry);
        if ((uint32_t)w != next) continue;
        dig[(size_t)lw * n + i] = d == DIG_NONE ? d : d ^ flip;
        next += wworld;
        ++lw;
    }
}

// ---- bucket sort without global atomics ------------------------------------------------------------------
// Random global atomics top out near 11 G/s on this chip (1.5 ms for the 16.8 M digits of a 2^20 MSM), so the
// (set, bucket) counting sort is done as a two-level partition whose counters all live in LDS:
//   pass 1  split the key range into "super-buckets" by the high bits of key = set * B + bucket: per-tile LDS
//           histogram -> global exclusive scan over (super-bucket, window, tile) -> per-tile LDS ranks;
//   pass 2  one workgroup per super-bucket: LDS counting sort over the low bits (<= 10), which also yields the final
//           bucket offsets.
// Both passes stage their tile / chunk in LDS first and write it out in runs per destination (one 4-byte store per
// entry straight to its slot cost 7x write amplification: PMC 619 MB written for 84 MB of output): with 2^14-entry
// tiles and <= 2^10 destinations per pass a run is >= 16 entries.
// Two tile shapes: 2^14 entries staged by 1024 lanes (~140 KiB of LDS: the workgroup owns its CU) when the MSM has the GPU
// to itself, and 2^12 entries by 256 lanes (~40 KiB) when another context's kernels share the chip (option
// "msm_sort_tile_log" = 12: the Groth16 shim's G2 multiexp on a second stream keeps ~98 KiB of every CU's LDS busy, a
// 140-KiB workgroup would wait for a CU to drain completely -- measured 7.8 ms for a 0.09-ms kernel).
struct SortBig {
    static constexpr uint32_t TILE = 16384, THREADS = 1024;
};
struct SortSmall {
    static constexpr uint32_t TILE = 4096, THREADS = 256;
};
constexpr uint32_t SORT_MAX_LOW = 10;   // <= 1024 destinations in pass 2
constexpr uint32_t SORT_MAX_SUPER = 1024;  // LDS: 3 counters per super-bucket next to the 128 KiB staged tile

ZK_D uint32_t sort_key(const SortGeom &g, uint32_t w, uint32_t d) { return (w % g.S) * g.B + (d & 0x7FFFFFFFu); }
ZK_D uint32_t sort_entry(const SortGeom &g, uint32_t w, uint32_t i, uint32_t d) {
    return ((g.tables ? (g.slot0 + w) * g.bases_n : 0u) + g.base_off + i) | (d & 0x80000000u);
}

// bh[sb * (W * ntile) + w * ntile + tile] = number of entries of window w, tile `tile`, in super-bucket sb
template <class SZ>
__global__ __launch_bounds__(SZ::THREADS) void msm_sort_hist(const uint32_t *__restrict__ dig, SortGeom g, uint32_t *__restrict__ bh) {
    constexpr uint32_t SORT_TILE = SZ::TILE, SORT_THREADS = SZ::THREADS;
    extern __shared__ uint32_t lh[];  // nsuper
    const uint32_t tile = blockIdx.x, w = blockIdx.y, t = threadIdx.x;
    for (uint32_t k = t; k < g.nsuper; k += SORT_THREADS) lh[k] = 0;
    __syncthreads();
    const uint32_t lo = tile * SORT_TILE, hi = min(g.n, lo + SORT_TILE);
    for (uint32_t i = lo + t; i < hi; i += SORT_THREADS) {
        uint32_t d = dig[(size_t)w * g.n + i];
        if (d != DIG_NONE) atomicAdd(&lh[sort_key(g, w, d) >> g.lowb], 1u);
    }
    __syncthreads();
    const size_t col = (size_t)w * g.ntile + tile, stride = (size_t)g.W * g.ntile;
    for (uint32_t k = t; k < g.nsuper; k += SORT_THREADS) bh[(size_t)k * stride + col] = lh[k];
}

// block-wide exclusive scan of `count` (<= SORT_MAX_SUPER) LDS counters in place; returns the total
template <uint32_t SORT_THREADS>
ZK_D uint32_t block_excl_scan(uint32_t *v, uint32_t count, uint32_t *scratch /* SORT_THREADS */) {
    const uint32_t t = threadIdx.x, per = (count + SORT_THREADS - 1) / SORT_THREADS;
    const uint32_t lo = min(count, t * per), hi = min(count, lo + per);
    uint32_t s = 0;
    for (uint32_t k = lo; k < hi; ++k) s += v[k];
    scratch[t] = s;
    block_inclusive_scan<SORT_THREADS>(scratch);
    const uint32_t total = scratch[SORT_THREADS - 1];
    uint32_t run = scratch[t] - s;
    for (uint32_t k = lo; k < hi; ++k) {
        uint32_t x = v[k];
        v[k] = run;
        run += x;
    }
    __syncthreads();
    return total;
}

// tmp_idx / tmp_key: entries grouped by super-bucket; order inside a group is arbitrary.
template <class SZ>
__global__ __launch_bounds__(SZ::THREADS) void msm_sort_split(const uint32_t *__restrict__ dig, SortGeom g, const uint32_t *__restrict__ bo,
                                                              uint32_t *__restrict__ tmp_idx, uint16_t *__restrict__ tmp_key) {
    constexpr uint32_t SORT_TILE = SZ::TILE, SORT_THREADS = SZ::THREADS;
    extern __shared__ uint32_t sm[];
    uint32_t *loff = sm;                      // nsuper + 1: local exclusive offsets
    uint32_t *cur = loff + g.nsuper + 1;      // nsuper
    uint32_t *gbase = cur + g.nsuper;         // nsuper
    uint32_t *scratch = gbase + g.nsuper;     // SORT_THREADS
    uint32_t *sidx = scratch + SORT_THREADS;  // SORT_TILE
    uint32_t *skey = sidx + SORT_TILE;        // SORT_TILE full keys
    const uint32_t tile = blockIdx.x, w = blockIdx.y, t = threadIdx.x;
    const size_t col = (size_t)w * g.ntile + tile, stride = (size_t)g.W * g.ntile;
    for (uint32_t k = t; k < g.nsuper; k += SORT_THREADS) {
        loff[k] = 0;
        gbase[k] = bo[(size_t)k * stride + col];
    }
    __syncthreads();
    const uint32_t lo = tile * SORT_TILE, hi = min(g.n, lo + SORT_TILE);
    for (uint32_t i = lo + t; i < hi; i += SORT_THREADS) {  // this tile's histogram again (cheaper than reloading it)
        uint32_t d = dig[(size_t)w * g.n + i];
        if (d != DIG_NONE) atomicAdd(&loff[sort_key(g, w, d) >> g.lowb], 1u);
    }
    __syncthreads();
    const uint32_t total = block_excl_scan<SORT_THREADS>(loff, g.nsuper, scratch);
    if (t == 0) loff[g.nsuper] = total;
    for (uint32_t k = t; k < g.nsuper; k += SORT_THREADS) cur[k] = loff[k];
    __syncthreads();
    for (uint32_t i = lo + t; i < hi; i += SORT_THREADS) {
        uint32_t d = dig[(size_t)w * g.n + i];
        if (d == DIG_NONE) continue;
        const uint32_t key = sort_key(g, w, d);
        const uint32_t r = atomicAdd(&cur[key >> g.lowb], 1u);
        sidx[r] = sort_entry(g, w, i, d);
        skey[r] = key;
    }
    __syncthreads();
    const uint32_t lmask = (1u << g.lowb) - 1;
    for (uint32_t s = t; s < total; s += SORT_THREADS) {
        const uint32_t key = skey[s], bin = key >> g.lowb, pos = gbase[bin] + (s - loff[bin]);
        tmp_idx[pos] = sidx[s];
        tmp_key[pos] = (uint16_t)(key & lmask);
    }
}

// one workgroup per super-bucket: final order + bucket offsets offs[sb * 2^lowb + low].
// The group is sorted chunk by chunk inside LDS and written out in runs per key (same reason as above).
// NLOW = 2^lowb <= 1024 counters, CPT = NLOW / THREADS of them per lane.
constexpr uint32_t SORT_NLOW_MAX = 1u << SORT_MAX_LOW;

template <uint32_t THREADS>
ZK_D void block_scan_counts(const uint32_t *cnt, uint32_t *excl, uint32_t *scratch) {  // excl[k] = sum_{j < k} cnt[j], k < SORT_NLOW_MAX
    constexpr uint32_t CPT = SORT_NLOW_MAX / THREADS;
    const uint32_t t = threadIdx.x;
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < CPT; ++k) s += cnt[t * CPT + k];
    scratch[t] = s;
    block_inclusive_scan<THREADS>(scratch);
    uint32_t run = scratch[t] - s;
#pragma unroll
    for (uint32_t k = 0; k < CPT; ++k) {
        excl[t * CPT + k] = run;
        run += cnt[t * CPT + k];
    }
    __syncthreads();
}

template <class SZ>
__global__ __launch_bounds__(SZ::THREADS) void msm_sort_final(const uint32_t *__restrict__ tmp_idx, const uint16_t *__restrict__ tmp_key, SortGeom g,
                                                              uint32_t nb, const uint32_t *__restrict__ bo, uint32_t *__restrict__ offs,
                                                              uint32_t *__restrict__ idx) {
    constexpr uint32_t SORT_TILE = SZ::TILE, SORT_THREADS = SZ::THREADS;
    __shared__ uint32_t cnt[SORT_NLOW_MAX], cursor[SORT_NLOW_MAX], loff[SORT_NLOW_MAX], cur[SORT_NLOW_MAX], scratch[SORT_THREADS];
    extern __shared__ uint32_t sm[];
    uint32_t *sidx = sm;                                            // SORT_TILE
    uint16_t *skey = reinterpret_cast<uint16_t *>(sidx + SORT_TILE);  // SORT_TILE
    const uint32_t grp = blockIdx.x, t = threadIdx.x;
    const size_t stride = (size_t)g.W * g.ntile;
    const uint32_t start = bo[(size_t)grp * stride];
    const uint32_t end = bo[(size_t)(grp + 1) * stride];  // bo has one trailing entry = total (grp + 1 == nsuper)
    const uint32_t nlow = 1u << g.lowb;                   // <= SORT_NLOW_MAX
    for (uint32_t k = t; k < SORT_NLOW_MAX; k += SORT_THREADS) cnt[k] = 0;
    __syncthreads();
    for (uint32_t k = start + t; k < end; k += SORT_THREADS) atomicAdd(&cnt[tmp_key[k]], 1u);
    __syncthreads();
    block_scan_counts<SORT_THREADS>(cnt, cursor, scratch);  // cursor[key] = offset of key inside the group
    for (uint32_t k = t; k < nlow; k += SORT_THREADS) {
        const uint32_t bucket = grp * nlow + k;
        cursor[k] += start;  // next free slot of key k
        if (bucket < nb) offs[bucket] = cursor[k];
    }
    if (grp + 1 == g.nsuper && t == 0) offs[nb] = end;
    __syncthreads();
    for (uint32_t c0 = start; c0 < end; c0 += SORT_TILE) {
        const uint32_t c1 = min(end, c0 + SORT_TILE);
        for (uint32_t k = t; k < SORT_NLOW_MAX; k += SORT_THREADS) cnt[k] = 0;
        __syncthreads();
        for (uint32_t k = c0 + t; k < c1; k += SORT_THREADS) atomicAdd(&cnt[tmp_key[k]], 1u);
        __syncthreads();
        block_scan_counts<SORT_THREADS>(cnt, loff, scratch);
        for (uint32_t k = t; k < SORT_NLOW_MAX; k += SORT_THREADS) cur[k] = loff[k];
        __syncthreads();
        for (uint32_t k = c0 + t; k < c1; k += SORT_THREADS) {
            const uint32_t key = tmp_key[k];
            const uint32_t r = atomicAdd(&cur[key], 1u);
            sidx[r] = tmp_idx[k];
            skey[r] = (uint16_t)key;
        }
        __syncthreads();
        for (uint32_t s = t; s < c1 - c0; s += SORT_THREADS) {
            const uint32_t key = skey[s];
            idx[cursor[key] + (s - loff[key])] = sidx[s];
        }
        __syncthreads();
        for (uint32_t k = t; k < SORT_NLOW_MAX; k += SORT_THREADS) cursor[k] += cnt[k];
        __syncthreads();
    }
}

// ---- order of buckets by descending size (counting sort, counters in LDS) --------------------------------------
// Lanes of a wave run in lockstep (a wave costs the largest bucket among its 64) and a workgroup holds its
// registers until its last wave retires, so buckets are handed out in globally sorted order: every wave and every
// workgroup sees near-equal trip counts, long buckets start first, empty and large (split elsewhere) buckets
// collect at the end.  `large` is the split threshold of this MSM (max(MSM_LARGE_BUCKET, 4 x mean bucket size)).
// bin 0: MSM_LARGE_BUCKET < size <= large; bin 1 + MSM_LARGE_BUCKET - size for 1 <= size <= MSM_LARGE_BUCKET; last bin:
// empty or split.
constexpr uint32_t SIZE_BINS = MSM_LARGE_BUCKET + 2;

ZK_HD uint32_t size_bin(uint32_t size, uint32_t large) {
    if (size == 0 || size > large) return SIZE_BINS - 1;
    return size > MSM_LARGE_BUCKET ? 0 : 1 + MSM_LARGE_BUCKET - size;
}

__global__ __launch_bounds__(256) void msm_size_hist(const uint32_t *__restrict__ offs, uint32_t nbuckets, uint32_t nblocks,
                                                     uint32_t large, uint32_t *__restrict__ bh) {
    __shared__ uint32_t lh[SIZE_BINS];
    const uint32_t t = threadIdx.x;
    if (t < SIZE_BINS) lh[t] = 0;
    __syncthreads();
    for (uint32_t g = blockIdx.x * 1024 + t; g < min(nbuckets, (blockIdx.x + 1) * 1024); g += 256)
        atomicAdd(&lh[size_bin(offs[g + 1] - offs[g], large)], 1u);
    __syncthreads();
    if (t < SIZE_BINS) bh[(size_t)t * nblocks + blockIdx.x] = lh[t];
}

__global__ __launch_bounds__(256) void msm_size_scatter(const uint32_t *__restrict__ offs, uint32_t nbuckets, uint32_t nblocks,
                                                        uint32_t large, const uint32_t *__restrict__ bo, uint32_t *__restrict__ order) {
    __shared__ uint32_t cur[SIZE_BINS];
    const uint32_t t = threadIdx.x;
    if (t < SIZE_BINS) cur[t] = bo[(size_t)t * nblocks + blockIdx.x];
    __syncthreads();
    for (uint32_t g = blockIdx.x * 1024 + t; g < min(nbuckets, (blockIdx.x + 1) * 1024); g += 256)
        order[atomicAdd(&cur[size_bin(offs[g + 1] - offs[g], large)], 1u)] = g;
}

// ---- large buckets ---------------------------------------------------------------------------------------
// Skewed scalars (Groth16 witnesses full of 0/1 values, a top window with only a few significant bits)
// put thousands of points into single buckets; one lane per bucket would serialise them.  Buckets above
// the threshold are cut into tasks of MSM_LARGE_CHUNK entries, one workgroup per task
// (strided mixed additions + LDS tree), and the per-task partial sums of a bucket are folded afterwards.
// plan[0] = number of tasks, plan[1] = number of large buckets; tasks[t] = {bucket, lo, hi};
// large[j] = {bucket, first task, task count}.
__global__ __launch_bounds__(256) void msm_plan_large(const uint32_t *__restrict__ offs, uint32_t nbuckets, uint32_t *__restrict__ plan,
                                                      uint32_t *__restrict__ tasks, uint32_t *__restrict__ large, uint32_t task_cap,
                                                      uint32_t large_cap, uint32_t thresh, uint32_t *__restrict__ status) {
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nbuckets) return;
    uint32_t lo = offs[g], hi = offs[g + 1], size = hi - lo;
    if (size <= thresh) return;
    uint32_t nt = (size + MSM_LARGE_CHUNK - 1) / MSM_LARGE_CHUNK;
    uint32_t first = atomicAdd(&plan[0], nt);
    uint32_t slot = atomicAdd(&plan[1], 1u);
    if (first + nt > task_cap || slot >= large_cap) {  // capacities are worst-case (see host): never expected, but never silent
        atomicOr(status, ZK_STATUS_MSM_PLAN_OVERFLOW);
        return;
    }
    for (uint32_t t = 0; t < nt; ++t) {
        tasks[3 * (first + t)] = g;
        tasks[3 * (first + t) + 1] = lo + t * MSM_LARGE_CHUNK;
        tasks[3 * (first + t) + 2] = min(hi, lo + (t + 1) * MSM_LARGE_CHUNK);
    }
    large[3 * slot] = g;
    large[3 * slot + 1] = first;
    large[3 * slot + 2] = nt;
}

inline MsmPlan msm_plan(const zkhip_ctx *ctx, const zkhip_bases *bases, size_t n) {
    MsmPlan p;
    p.tables = bases->tables();
    int c = p.tables ? bases->c_tab : ctx->opt_msm_window_bits;
    if (c <= 0) c = zk_msm_auto_window(n);
    p.c = std::max(2, std::min(ZK_MSM_MAX_C, c));
    if (!p.tables) p.c = std::min(p.c, 16);  // one bucket set PER WINDOW there (W 2^(c-1) buckets): stay within the sort's key range
    p.W_all = msm_windows(zk_scalar_bits(bases->curve), p.c);  // scalars are folded to |s| <= (r - 1) / 2: no carry out of the top window
    p.win = msm_make_windows(zk_scalar_bits(bases->curve), p.W_all);
    // window partition over GPUs: this call handles the windows {w : w mod win_world == win_rank} only (all equal-weight
    // thanks to the tables)
    p.wrank = p.tables ? (uint32_t)bases->win_rank : 0u;
    p.wworld = p.tables ? (uint32_t)bases->win_world : 1u;
    p.W = p.tables ? bases->local_windows() : p.W_all;
    p.B = 1u << (p.c - 1);
    // sets: without tables the windows keep their own buckets (different weights: Horner in msm_final); with tables all
    // windows share ONE set unless that leaves too few buckets (= lanes) to fill the chip
    if (!p.tables) p.S = (uint32_t)p.W;
    else {
        int s = ctx->opt_msm_sets;
        if (s <= 0) s = (int)((zk_msm_target_lanes() + p.B - 1) / p.B);
        p.S = (uint32_t)std::max(1, std::min(p.W, s));
        while (p.S > 1 && (uint64_t)p.S * p.B > ((uint64_t)SORT_MAX_SUPER << SORT_MAX_LOW)) --p.S;
    }
    p.nb = p.S * p.B;
    return p;
}

// the sort's launch sequence for one tile shape (bh / bo: g.nsuper x g.W x g.ntile counters and their scan)
template <class SZ>
int msm_sort_run(zkhip_ctx *ctx, const SortGeom &g, uint32_t nbh, const uint32_t *dig, uint32_t *bh, uint32_t *bo, uint32_t *bsums, uint32_t *tmp_idx,
                 uint16_t *tmp_key, uint32_t *offs, uint32_t *idx) {
    const size_t lds_hist = (size_t)g.nsuper * 4;
    const size_t lds_split = ((size_t)3 * g.nsuper + 1 + SZ::THREADS + 2 * SZ::TILE) * 4;
    const size_t lds_final = (size_t)SZ::TILE * 6;
    if (lds_split > 48 * 1024) ZK_MAX_LDS(ctx, msm_sort_split<SZ>, 160 * 1024 - 256);
    if (lds_final > 40 * 1024) ZK_MAX_LDS(ctx, msm_sort_final<SZ>, 160 * 1024 - (4 * SORT_NLOW_MAX + SZ::THREADS) * 4 - 256);
    ZK_LAUNCH(ctx, "msm_sort_hist", msm_sort_hist<SZ>, dim3(g.ntile, g.W), dim3(SZ::THREADS), lds_hist, dig, g, bh);
    ZK_TRY(msm_scan(ctx, "msm_scan", bh, nbh, bo, bsums));
    ZK_LAUNCH(ctx, "msm_sort_split", msm_sort_split<SZ>, dim3(g.ntile, g.W), dim3(SZ::THREADS), lds_split, dig, g, bo, tmp_idx, tmp_key);
    ZK_LAUNCH(ctx, "msm_sort_final", msm_sort_final<SZ>, dim3(g.nsuper), dim3(SZ::THREADS), lds_final, tmp_idx, tmp_key, g, g.S * g.B, bo, offs, idx);
    return 0;
}

}  // namespace

int zk_msm_entries_plan(const zkhip_ctx *ctx, const zkhip_bases *bases, size_t offset, size_t n, MsmEntriesCall &c, std::string &error) {
    const MsmPlan &P = c.P = msm_plan(ctx, bases, n);
    // every sort offset / prefix sum / idx position is a u32 over the W * n entries, and an entry addresses a table row
    if ((uint64_t)P.W * n >= (1ull << 32) || (uint64_t)bases->nslots * bases->n >= (1ull << 31)) {
        error = "MSM of " + std::to_string(n) + " points x " + std::to_string(P.W) + " windows exceeds the 32-bit entry index (split the range)";
        return ZKHIP_ERR_RANGE;
    }
    // two-level LDS counting sort (see msm_sort_*): the low bits inside a super-bucket, the rest across super-buckets
    SortGeom &g = c.g;
    g.n = (uint32_t)n;
    g.W = (uint32_t)P.W;
    g.B = P.B;
    g.S = P.S;
    g.lowb = (uint32_t)std::min<int>(SORT_MAX_LOW, P.c - 1);
    g.nsuper = (P.nb + (1u << g.lowb) - 1) >> g.lowb;
    c.big_tiles = ctx->opt_msm_sort_tile_log >= 14;
    g.tile = c.big_tiles ? SortBig::TILE : SortSmall::TILE;
    g.ntile = (uint32_t)((n + g.tile - 1) / g.tile);
    g.tables = P.tables ? 1u : 0u;
    g.slot0 = P.tables ? (uint32_t)bases->slot_of_local(0) : 0u;
    g.bases_n = (uint32_t)bases->n;
    g.base_off = (uint32_t)offset;
    if (g.nsuper > SORT_MAX_SUPER) return ZKHIP_ERR_RANGE;
    const size_t nbh64 = (size_t)g.nsuper * g.W * g.ntile;
    if (nbh64 >= (1ull << 31)) return ZKHIP_ERR_RANGE;
    c.nbh = (uint32_t)nbh64;
    c.sblk = (P.nb + 1023) / 1024;
    c.nsh = SIZE_BINS * c.sblk;
    c.large_thresh = (uint32_t)std::max<size_t>(MSM_LARGE_BUCKET, 4 * ((c.entries() + P.nb - 1) / P.nb));
    c.large_cap = (uint32_t)(c.entries() / c.large_thresh + 1);
    c.task_cap = (uint32_t)(c.entries() / MSM_LARGE_CHUNK + c.large_cap + 1);
    return 0;
}

int zk_msm_entries(zkhip_ctx *ctx, int curve, const MsmEntriesCall &c, const MsmEntriesBuffers &w, const uint32_t *d_scalars) {
    const MsmPlan &P = c.P;
    const uint32_t n = c.g.n, nb = P.nb;
    ZK_TRY(fr_sat_dispatch(curve, [&](auto fr) -> int {
        typedef typename decltype(fr)::type FR;
        ZK_LAUNCH(ctx, "msm_digits", msm_digits_only<FR>, grid_1d(n), dim3(256), 0, d_scalars, n, P.win, P.wrank, P.wworld, w.dig);
        return 0;
    }));
    ZK_TRY((c.big_tiles ? msm_sort_run<SortBig> : msm_sort_run<SortSmall>)(ctx, c.g, c.nbh, w.dig, w.bh, w.bo, w.bsums, w.tmp_idx, w.tmp_key, w.offs, w.idx));
    // buckets by descending size
    ZK_LAUNCH(ctx, "msm_size_sort", msm_size_hist, dim3(c.sblk), dim3(256), 0, w.offs, nb, c.sblk, c.large_thresh, w.sh);
    ZK_TRY(msm_scan(ctx, "msm_size_sort", w.sh, c.nsh, w.so, w.ssums));
    ZK_LAUNCH(ctx, "msm_size_sort", msm_size_scatter, dim3(c.sblk), dim3(256), 0, w.offs, nb, c.sblk, c.large_thresh, w.so, w.order);
    return 0;
}

// large buckets: plan on the device (no host round trip), then fixed-size grids that read the plan
int zk_msm_large_plan(zkhip_ctx *ctx, const MsmEntriesCall &c, const MsmEntriesBuffers &w) {
    const uint32_t nb = c.P.nb;
    ZK_HIP_CHECK(ctx, hipMemsetAsync(w.plan, 0, 16, ctx->stream));
    ZK_LAUNCH(ctx, "msm_plan_large", msm_plan_large, grid_1d(nb), dim3(256), 0, w.offs, nb, w.plan, w.tasks, w.large, c.task_cap, c.large_cap,
              c.large_thresh, ctx->d_status);
    return 0;
}

uint32_t zk_msm_size_bin(uint32_t size, uint32_t large) { return size_bin(size, large); }
