// The field-free first stage of every MSM, compiled once (interface: msm_entries.hpp; the per-(curve, group) units call it from msm_core.hpp's
// msm_stages).  No kernel here looks at a coordinate.
//   msm_digits_only   scalar -> signed digits                           (streams 32 B/scalar, coalesced); clears the plan's counters
//   msm_sort_*        two-level counting sort of the entries by (set, bucket), counters in LDS only, tiles staged in LDS
//   msm_scan_*        exclusive prefix (one workgroup, or local scan + add-back), shared by both sorts; every LDS scan is block_inclusive_scan
//   msm_size_*        order of the buckets by descending size
//   msm_plan_bucket   buckets far above the mean, cut into 4096-entry tasks for msm_bucket_large / msm_large_combine (msm_core.hpp)
// Launch sequence of a 2^20-point MSM (nine launches): msm_digits_only, msm_sort_hist, msm_scan_local, msm_scan_add, msm_sort_split,
// msm_sort_final (which also counts the size sort's histogram), msm_scan_local, msm_scan_add, msm_size_scatter (order and large-bucket plan).
// Short counter arrays take msm_scan_single instead of a scan pair; geometries whose super-buckets are not 1024 buckets wide launch
// msm_size_hist after msm_sort_final.
// Point order inside a bucket depends on LDS-atomic arrival order; nothing else about the buffers does.
#include <algorithm>
#include <string>

#include "ctx.hpp"
#include "fu.hpp"
#include "msm_block_scan.hpp"
#include "msm_entries.hpp"
#include "msm_ops.hpp"
#include "msm_recode.hpp"

namespace {

using namespace zkhip;

constexpr uint32_t MSM_LARGE_BUCKET = 128;  // buckets above this many entries (and 4 x the mean) are split across workgroups
constexpr uint32_t MSM_LARGE_CHUNK = 4096;  // entries per task of a split bucket

// exclusive scan of `count` u32 counters in two launches: per-block (1024 counters) local scan + block totals, then the add-back,
// in which every workgroup sums the block totals below its own (a few hundred words at 2^20 points; no workgroup waits for
// another one).  offs[count] = total.
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

__global__ __launch_bounds__(256) void msm_scan_add(uint32_t *__restrict__ offs, uint32_t count, const uint32_t *__restrict__ block_sums) {
    __shared__ uint32_t wave_total[4];
    const uint32_t t = threadIdx.x, blk = blockIdx.x, base = blk * 1024 + t * 4;
    uint32_t s = 0;
    for (uint32_t i = t; i < blk; i += 256) s += block_sums[i];
    s = wave_sum(s);
    if ((t & 63) == 0) wave_total[t >> 6] = s;
    __syncthreads();
    const uint32_t add = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (base + k < count) offs[base + k] += add;
    if (blk + 1 == gridDim.x && t == 0) offs[count] = add + block_sums[blk];
}

// the same in ONE launch for short arrays (small MSMs are bound by launch gaps, not by work): one workgroup walks the
// array in 1024-counter strips, carrying the running total
__global__ __launch_bounds__(1024) void msm_scan_single(const uint32_t *__restrict__ hist, uint32_t count, uint32_t *__restrict__ offs) {
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < count; base += 1024) {
        const uint32_t v = base + t < count ? hist[base + t] : 0;
        part[t] = v;
        block_inclusive_scan<1024>(part);
        if (base + t < count) offs[base + t] = carry + part[t] - v;
        carry += part[1023];
        __syncthreads();
    }
    if (t == 0) offs[count] = carry;
}
constexpr uint32_t MSM_SCAN_SINGLE_MAX = 1u << 16;

// exclusive scan of hist[0 .. count) into offs[0 .. count], offs[count] = total (bsums: the block totals of the two-launch form)
inline int msm_scan(zkhip_ctx *ctx, const char *name, const uint32_t *hist, uint32_t count, uint32_t *offs, uint32_t *bsums) {
    if (count <= MSM_SCAN_SINGLE_MAX) {
        ZK_LAUNCH(ctx, name, msm_scan_single, dim3(1), dim3(1024), 0, hist, count, offs);
        return 0;
    }
    const uint32_t nblk = (count + 1023) / 1024;
    ZK_LAUNCH(ctx, name, msm_scan_local, dim3(nblk), dim3(256), 0, hist, count, offs, bsums);
    ZK_LAUNCH(ctx, name, msm_scan_add, dim3(nblk), dim3(256), 0, offs, count, bsums);
    return 0;
}

// Window partition (wrank of wworld): the carry chain runs over all windows, only the digits of windows
// w = wrank + k wworld are kept, as local window k.
template <class FR>
__global__ __launch_bounds__(256) void msm_digits_only(const uint32_t *__restrict__ scalars, uint32_t n, MsmWindows win, uint32_t wrank,
                                                       uint32_t wworld, uint32_t *__restrict__ dig, uint32_t *__restrict__ plan) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == 0) plan[0] = plan[1] = 0;  // the large-bucket counters, for msm_size_scatter at the end of the stage
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
// A third shape in between, 2^13 entries by 512 lanes (~70 KiB: two workgroups per CU, runs still >= 16 entries at 512
// super-buckets), is option value 13.
// Every shape gives a lane 16 entries of a tile, which the split and the final pass hold in registers between their histogram and
// their ranking.
struct SortBig {
    static constexpr uint32_t TILE = 16384, THREADS = 1024;
};
struct SortMid {
    static constexpr uint32_t TILE = 8192, THREADS = 512;
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
    constexpr uint32_t SORT_TILE = SZ::TILE, SORT_THREADS = SZ::THREADS, ITEMS = SORT_TILE / SORT_THREADS;
    extern __shared__ uint32_t sm[];
    uint32_t *loff = sm;                      // nsuper + 1: local exclusive offsets
    uint32_t *cur = loff + g.nsuper + 1;      // nsuper
    uint32_t *gbase = cur + g.nsuper;         // nsuper
    uint32_t *scratch = gbase + g.nsuper;     // SORT_THREADS
    uint32_t *sidx = scratch + SORT_THREADS;  // SORT_TILE
    uint32_t *skey = sidx + SORT_TILE;        // SORT_TILE full keys
    const uint32_t tile = blockIdx.x, w = blockIdx.y, t = threadIdx.x;
    const size_t col = (size_t)w * g.ntile + tile, stride = (size_t)g.W * g.ntile;
    const uint32_t lo = tile * SORT_TILE, hi = min(g.n, lo + SORT_TILE);
    uint32_t d[ITEMS];  // the lane's digits of this tile, read once (the tile's histogram is counted again: cheaper than reloading it)
#pragma unroll
    for (uint32_t j = 0; j < ITEMS; ++j) {
        const uint32_t i = lo + j * SORT_THREADS + t;
        d[j] = i < hi ? dig[(size_t)w * g.n + i] : DIG_NONE;
    }
    for (uint32_t k = t; k < g.nsuper; k += SORT_THREADS) {
        loff[k] = 0;
        gbase[k] = bo[(size_t)k * stride + col];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < ITEMS; ++j)
        if (d[j] != DIG_NONE) atomicAdd(&loff[sort_key(g, w, d[j]) >> g.lowb], 1u);
    __syncthreads();
    const uint32_t total = block_excl_scan<SORT_THREADS>(loff, g.nsuper, scratch);
    if (t == 0) loff[g.nsuper] = total;
    for (uint32_t k = t; k < g.nsuper; k += SORT_THREADS) cur[k] = loff[k];
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < ITEMS; ++j) {
        if (d[j] == DIG_NONE) continue;
        const uint32_t key = sort_key(g, w, d[j]);
        const uint32_t r = atomicAdd(&cur[key >> g.lowb], 1u);
        sidx[r] = sort_entry(g, w, lo + j * SORT_THREADS + t, d[j]);
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

// one chunk of the final pass, after its keys are counted in cnt: cur[k] = rank of key k's first entry inside the chunk, dst[k] + rank = its
// slot in idx; cursor moves past the chunk and cnt is cleared for the next one
template <uint32_t THREADS>
ZK_D void block_scan_chunk(uint32_t *cnt, uint32_t *cursor, uint32_t *cur, uint32_t *dst, uint32_t *scratch) {
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
        const uint32_t i = t * CPT + k, c = cnt[i];
        cur[i] = run;
        dst[i] = cursor[i] - run;
        cursor[i] += c;
        cnt[i] = 0;
        run += c;
    }
    __syncthreads();
}

// sh (or null): with 2^lowb == 1024 a super-bucket is one 1024-bucket workgroup of the size sort, whose column of the (bin, workgroup)
// histogram is counted here, from the bucket sizes in LDS, instead of by msm_size_hist from offs
template <class SZ>
__global__ __launch_bounds__(SZ::THREADS) void msm_sort_final(const uint32_t *__restrict__ tmp_idx, const uint16_t *__restrict__ tmp_key, SortGeom g,
                                                              uint32_t nb, const uint32_t *__restrict__ bo, uint32_t *__restrict__ offs,
                                                              uint32_t *__restrict__ idx, uint32_t large, uint32_t *__restrict__ sh) {
    constexpr uint32_t SORT_TILE = SZ::TILE, SORT_THREADS = SZ::THREADS, ITEMS = SORT_TILE / SORT_THREADS;
    constexpr uint32_t NO_KEY = 0xFFFFu;  // keys are below SORT_NLOW_MAX
    static_assert(SORT_THREADS >= SIZE_BINS, "one lane per size bin");
    __shared__ uint32_t cnt[SORT_NLOW_MAX], cursor[SORT_NLOW_MAX], dst[SORT_NLOW_MAX], cur[SORT_NLOW_MAX], scratch[SORT_THREADS];
    extern __shared__ uint32_t sm[];
    uint32_t *sidx = sm;                                            // SORT_TILE
    uint16_t *skey = reinterpret_cast<uint16_t *>(sidx + SORT_TILE);  // SORT_TILE
    const uint32_t grp = blockIdx.x, t = threadIdx.x;
    const size_t stride = (size_t)g.W * g.ntile;
    const uint32_t start = bo[(size_t)grp * stride];
    const uint32_t end = bo[(size_t)(grp + 1) * stride];  // bo has one trailing entry = total (grp + 1 == nsuper)
    const uint32_t nlow = 1u << g.lowb;                   // <= SORT_NLOW_MAX
    for (uint32_t k = t; k < SORT_NLOW_MAX; k += SORT_THREADS) cnt[k] = 0;
    if (t < SIZE_BINS) cur[t] = 0;  // the size bins, until the first chunk
    __syncthreads();
    for (uint32_t k = start + t; k < end; k += SORT_THREADS) atomicAdd(&cnt[tmp_key[k]], 1u);
    __syncthreads();
    block_scan_counts<SORT_THREADS>(cnt, cursor, scratch);  // cursor[key] = offset of key inside the group
    for (uint32_t k = t; k < SORT_NLOW_MAX; k += SORT_THREADS) {
        const uint32_t bucket = grp * nlow + k;
        cursor[k] += start;  // next free slot of key k
        if (k < nlow && bucket < nb) {
            offs[bucket] = cursor[k];
            if (sh) atomicAdd(&cur[size_bin(cnt[k], large)], 1u);
        }
        cnt[k] = 0;
    }
    if (grp + 1 == g.nsuper && t == 0) offs[nb] = end;
    __syncthreads();
    if (sh && t < SIZE_BINS) sh[(size_t)t * g.nsuper + grp] = cur[t];
    for (uint32_t c0 = start; c0 < end; c0 += SORT_TILE) {
        const uint32_t c1 = min(end, c0 + SORT_TILE);
        uint32_t key[ITEMS], entry[ITEMS];  // the lane's part of the chunk, read once
#pragma unroll
        for (uint32_t j = 0; j < ITEMS; ++j) {
            const uint32_t k = c0 + j * SORT_THREADS + t;
            key[j] = k < c1 ? tmp_key[k] : NO_KEY;
            entry[j] = k < c1 ? tmp_idx[k] : 0u;
        }
#pragma unroll
        for (uint32_t j = 0; j < ITEMS; ++j)
            if (key[j] != NO_KEY) atomicAdd(&cnt[key[j]], 1u);
        __syncthreads();
        block_scan_chunk<SORT_THREADS>(cnt, cursor, cur, dst, scratch);
#pragma unroll
        for (uint32_t j = 0; j < ITEMS; ++j) {
            if (key[j] == NO_KEY) continue;
            const uint32_t r = atomicAdd(&cur[key[j]], 1u);
            sidx[r] = entry[j];
            skey[r] = (uint16_t)key[j];
        }
        __syncthreads();
        for (uint32_t s = t; s < c1 - c0; s += SORT_THREADS) idx[dst[skey[s]] + s] = sidx[s];
        // (the next chunk writes sidx / skey / dst only after two barriers, cnt is clear since block_scan_chunk)
    }
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

// ---- large buckets ---------------------------------------------------------------------------------------
// Skewed scalars (Groth16 witnesses full of 0/1 values, a top window with only a few significant bits)
// put thousands of points into single buckets; one lane per bucket would serialise them.  Buckets above
// the threshold are cut into tasks of MSM_LARGE_CHUNK entries, one workgroup per task
// (strided mixed additions + LDS tree), and the per-task partial sums of a bucket are folded afterwards.
// plan[0] = number of tasks, plan[1] = number of large buckets; tasks[t] = {bucket, lo, hi};
// large[j] = {bucket, first task, task count}.
// The plan is written by the last kernel of the stage, msm_size_scatter, which reads every bucket's size anyway; the first kernel
// (msm_digits_only) clears the two counters.
struct LargePlan {
    uint32_t *plan, *tasks, *large;
    uint32_t task_cap, large_cap;
    uint32_t *status;
};

ZK_D void msm_plan_bucket(const LargePlan &p, uint32_t g, uint32_t lo, uint32_t hi) {  // bucket g = entries lo .. hi is above the threshold
    const uint32_t nt = (hi - lo + MSM_LARGE_CHUNK - 1) / MSM_LARGE_CHUNK;
    const uint32_t first = atomicAdd(&p.plan[0], nt);
    const uint32_t slot = atomicAdd(&p.plan[1], 1u);
    if (first + nt > p.task_cap || slot >= p.large_cap) {  // capacities are worst-case (see host): never expected, but never silent
        atomicOr(p.status, ZK_STATUS_MSM_PLAN_OVERFLOW);
        return;
    }
    for (uint32_t t = 0; t < nt; ++t) {
        p.tasks[3 * (first + t)] = g;
        p.tasks[3 * (first + t) + 1] = lo + t * MSM_LARGE_CHUNK;
        p.tasks[3 * (first + t) + 2] = min(hi, lo + (t + 1) * MSM_LARGE_CHUNK);
    }
    p.large[3 * slot] = g;
    p.large[3 * slot + 1] = first;
    p.large[3 * slot + 2] = nt;
}

__global__ __launch_bounds__(256) void msm_size_scatter(const uint32_t *__restrict__ offs, uint32_t nbuckets, uint32_t nblocks,
                                                        uint32_t large, const uint32_t *__restrict__ bo, uint32_t *__restrict__ order, LargePlan plan) {
    // The same input gives the same order: the workgroup's 1024 buckets are 16 segments of 64, each ranked by ONE wave instruction
    // (LDS atomics of different waves arrive in any order, those of one instruction do not), and the segments of a bin follow one another.
    constexpr uint32_t SEGS = 16;
    __shared__ uint32_t seg[SEGS * SIZE_BINS];
    const uint32_t t = threadIdx.x, first = blockIdx.x * 1024, last = min(nbuckets, first + 1024);
    for (uint32_t k = t; k < SEGS * SIZE_BINS; k += 256) seg[k] = 0;
    __syncthreads();
    uint32_t slot[4], rank[4];  // slot: (segment, bin) of the lane's j-th bucket
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t g = first + j * 256 + t;
        if (g >= last) continue;
        const uint32_t lo = offs[g], hi = offs[g + 1];
        slot[j] = (j * 4 + (t >> 6)) * SIZE_BINS + size_bin(hi - lo, large);
        rank[j] = atomicAdd(&seg[slot[j]], 1u);
        if (hi - lo > large) msm_plan_bucket(plan, g, lo, hi);
    }
    __syncthreads();
    if (t < SIZE_BINS) {
        uint32_t run = bo[(size_t)t * nblocks + blockIdx.x];
        for (uint32_t s = 0; s < SEGS; ++s) {
            const uint32_t x = seg[s * SIZE_BINS + t];
            seg[s * SIZE_BINS + t] = run;
            run += x;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t g = first + j * 256 + t;
        if (g < last) order[seg[slot[j]] + rank[j]] = g;
    }
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

// the sort's launch sequence for one tile shape (bh / bo: g.nsuper x g.W x g.ntile counters and their scan); sh: see msm_sort_final
template <class SZ>
int msm_sort_run(zkhip_ctx *ctx, const SortGeom &g, uint32_t nbh, const MsmEntriesBuffers &w, uint32_t large, uint32_t *sh) {
    const size_t lds_hist = (size_t)g.nsuper * 4;
    const size_t lds_split = ((size_t)3 * g.nsuper + 1 + SZ::THREADS + 2 * SZ::TILE) * 4;
    const size_t lds_final = (size_t)SZ::TILE * 6;
    if (lds_split > 48 * 1024) ZK_MAX_LDS(ctx, msm_sort_split<SZ>, 160 * 1024 - 256);
    if (lds_final > 40 * 1024) ZK_MAX_LDS(ctx, msm_sort_final<SZ>, 160 * 1024 - (4 * SORT_NLOW_MAX + SZ::THREADS) * 4 - 256);
    ZK_LAUNCH(ctx, "msm_sort_hist", msm_sort_hist<SZ>, dim3(g.ntile, g.W), dim3(SZ::THREADS), lds_hist, w.dig, g, w.bh);
    ZK_TRY(msm_scan(ctx, "msm_scan", w.bh, nbh, w.bo, w.bsums));
    ZK_LAUNCH(ctx, "msm_sort_split", msm_sort_split<SZ>, dim3(g.ntile, g.W), dim3(SZ::THREADS), lds_split, w.dig, g, w.bo, w.tmp_idx, w.tmp_key);
    ZK_LAUNCH(ctx, "msm_sort_final", msm_sort_final<SZ>, dim3(g.nsuper), dim3(SZ::THREADS), lds_final, w.tmp_idx, w.tmp_key, g, g.S * g.B, w.bo, w.offs, w.idx,
              large, sh);
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
    const int tile_log = ctx->opt_msm_sort_tile_log;
    g.tile = tile_log >= 14 ? SortBig::TILE : tile_log == 13 ? SortMid::TILE : SortSmall::TILE;
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
        ZK_LAUNCH(ctx, "msm_digits", msm_digits_only<FR>, grid_1d(n), dim3(256), 0, d_scalars, n, P.win, P.wrank, P.wworld, w.dig, w.plan);
        return 0;
    }));
    // buckets by descending size: the final pass of the sort counts the (bin, workgroup) histogram where its groups are the size sort's workgroups
    const bool final_counts_sizes = (1u << c.g.lowb) == 1024;
    uint32_t *sh = final_counts_sizes ? w.sh : nullptr;
    ZK_TRY((c.g.tile == SortBig::TILE   ? msm_sort_run<SortBig>
            : c.g.tile == SortMid::TILE ? msm_sort_run<SortMid>
                                        : msm_sort_run<SortSmall>)(ctx, c.g, c.nbh, w, c.large_thresh, sh));
    if (!final_counts_sizes) ZK_LAUNCH(ctx, "msm_size_sort", msm_size_hist, dim3(c.sblk), dim3(256), 0, w.offs, nb, c.sblk, c.large_thresh, w.sh);
    ZK_TRY(msm_scan(ctx, "msm_size_sort", w.sh, c.nsh, w.so, w.ssums));
    const LargePlan plan = {w.plan, w.tasks, w.large, c.task_cap, c.large_cap, ctx->d_status};
    // (profiled under the name the plan always had: the launch that writes plan, tasks and large)
    ZK_LAUNCH(ctx, "msm_plan_large", msm_size_scatter, dim3(c.sblk), dim3(256), 0, w.offs, nb, c.sblk, c.large_thresh, w.so, w.order, plan);
    return 0;
}

// The plan of the large buckets is part of zk_msm_entries (msm_size_scatter writes it): nothing is left to enqueue here.
int zk_msm_large_plan(zkhip_ctx *, const MsmEntriesCall &, const MsmEntriesBuffers &) { return 0; }

uint32_t zk_msm_size_bin(uint32_t size, uint32_t large) { return size_bin(size, large); }
