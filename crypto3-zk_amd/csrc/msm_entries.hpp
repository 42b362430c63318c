// The field-free first stage of an MSM (msm_entries.hip): scalars -> signed digits -> entries sorted by (set, bucket) -> bucket ids by
// descending size -> the plan of the large buckets.  It never looks at a coordinate, so it is compiled once and called by every
// per-(curve, group) unit (msm_core.hpp) -- and by tests/cpp/entriestest.hip, which checks its buffers by themselves.
#pragma once
#include <string>

#include "ctx.hpp"
#include "msm_recode.hpp"

namespace zkhip {

// The geometry of one MSM call: window size, windows, sets, buckets.
struct MsmPlan {
    int c, W_all, W;      // window bits; windows of the scalar; windows this call handles (window partition: a subset)
    uint32_t B, S, nb;    // buckets per set, sets, S * B
    MsmWindows win;
    uint32_t wrank, wworld;
    bool tables;
};

// A window-w tile covers points [tile * SORT_TILE, ...) of that window; the entry it emits for point i is
// (slot(w) * bases_n + base_off + i) | sign, the index of the table row the accumulation kernel gathers.
struct SortGeom {
    uint32_t n;           // points
    uint32_t W;           // (local) windows
    uint32_t B;           // buckets per set
    uint32_t S;           // sets: set(w) = w % S
    uint32_t lowb;        // low key bits (pass 2)
    uint32_t nsuper;      // ceil(S * B / 2^lowb)
    uint32_t tile;        // entries per tile: names the sort's tile shape (option "msm_sort_tile_log": 12, 13 or 14)
    uint32_t ntile;       // tiles per window
    uint32_t slot0;       // table slot of local window 0 (slot(lw) = slot0 + lw); all windows share slot 0 without tables
    uint32_t tables;      // 1: window lw reads table slot0 + lw; 0: every window reads the points themselves
    uint32_t bases_n;     // points per table
    uint32_t base_off;    // first point of this MSM inside the table
};

// What the stage settles before its first launch: zk_msm_entries_plan fills it from the context's options and the bases object and touches
// neither; the sizes of MsmEntriesBuffers and every grid of the stage are functions of it.
struct MsmEntriesCall {
    MsmPlan P;
    SortGeom g;
    uint32_t nbh;                // counters of the sort's (super-bucket, window, tile) histogram
    uint32_t sblk, nsh;           // size sort: workgroups of 1024 buckets, counters of its (bin, workgroup) histogram
    // large buckets: split threshold, and the worst-case plan (every entry in a large bucket)
    uint32_t large_thresh, large_cap, task_cap;
    size_t entries() const { return (size_t)P.W * g.n; }
};

// The stage's device buffers; counts in u32 words unless said (MsmBuffers::layout in msm_core.hpp is the one place that sizes them for an MSM).
struct MsmEntriesBuffers {
    uint32_t *dig, *bh, *bo, *bsums, *tmp_idx;  // digits; the sort's histogram, its exclusive scan, the scan's block sums
    uint16_t *tmp_key;
    uint32_t *offs, *idx;
    uint32_t *sh, *so, *ssums, *order;  // size sort: histogram, its scan, block sums; bucket ids by descending size
    uint32_t *plan, *tasks, *large;     // large buckets: counters, tasks and buckets of the plan (written by msm_size_scatter)
};

}  // namespace zkhip

// the geometry of the MSM over points offset .. offset + n of `bases`; ZKHIP_ERR_RANGE (with `error` set where the entries outgrow 32 bits)
int zk_msm_entries_plan(const zkhip_ctx *ctx, const zkhip_bases *bases, size_t offset, size_t n, zkhip::MsmEntriesCall &c, std::string &error);
// enqueue digits, sort, size order and the plan of the buckets above c.large_thresh: dig, offs, idx, order, plan, tasks and large are final when
// the stream reaches the end of it; a plan beyond its capacities raises ZK_STATUS_MSM_PLAN_OVERFLOW
int zk_msm_entries(zkhip_ctx *ctx, int curve, const zkhip::MsmEntriesCall &c, const zkhip::MsmEntriesBuffers &w, const uint32_t *d_scalars);
// the point of the sequence from which callers read plan, tasks and large; enqueues nothing (the plan is the last kernel of zk_msm_entries)
int zk_msm_large_plan(zkhip_ctx *ctx, const zkhip::MsmEntriesCall &c, const zkhip::MsmEntriesBuffers &w);
// the size sort's bin of a bucket of `size` entries under the split threshold `large`: order lists the buckets by ascending bin
uint32_t zk_msm_size_bin(uint32_t size, uint32_t large);
