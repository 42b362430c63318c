// Host-side context shared by the kernel families: stream, workspace arena, per-kernel HIP-event profiler.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../include/zkhip.h"
#include "ntt_plan.hpp"
#include "options.hpp"
#include "table_cache.hpp"
#include "zk_defs.hpp"

#define ZK_HIP_CHECK(ctx, expr)                                                                  \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess) {                                                                 \
            (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(e__);              \
            return e__ == hipErrorOutOfMemory ? ZKHIP_ERR_OOM : ZKHIP_ERR_HIP;                   \
        }                                                                                        \
    } while (0)

#define ZK_TRY(expr)              \
    do {                          \
        int rc__ = (expr);        \
        if (rc__ != 0) return rc__; \
    } while (0)

// The head of an entry point, in two halves: ZK_ARGS refuses a null context or an unknown curve id before any HIP call, ZK_ENTER selects the
// context's device.  A function's own argument and range checks and its "nothing to do" return sit between the two, so argument errors
// never depend on the device and an empty call does not touch it.
inline bool zk_curve_known(int curve) { return curve >= zkhip::CURVE_BLS12_381 && curve <= zkhip::CURVE_VESTA; }
// The pairing-friendly curves: the only ones with a G2, and the only ones the Groth16, wire-format and EC-NTT entry points take (ZK_ARGS_PAIRING).
inline bool zk_curve_pairing(int curve) { return curve == zkhip::CURVE_BLS12_381 || curve == zkhip::CURVE_BN254; }
inline bool zk_group_known(int group) { return group == zkhip::GROUP_G1 || group == zkhip::GROUP_G2; }
inline bool zk_curve_group_known(int curve, int group) { return zk_curve_known(curve) && (group == zkhip::GROUP_G1 || (group == zkhip::GROUP_G2 && zk_curve_pairing(curve))); }
#define ZK_ARGS(ctx, curve) if (!(ctx) || !zk_curve_known(curve)) return ZKHIP_ERR_INVALID
#define ZK_ARGS_PAIRING(ctx, curve) if (!(ctx) || !zk_curve_pairing(curve)) return ZKHIP_ERR_INVALID
#define ZK_ENTER(ctx) ZK_HIP_CHECK(ctx, hipSetDevice((ctx)->device))
inline bool zk_any_null(const void *const *p, size_t count) {  // a host table of device pointers with a hole in it
    return std::any_of(p, p + count, [](const void *q) { return !q; });
}

// The 1-D grid of one lane per element, `threads` lanes per workgroup.  A grid holds fewer than 2^31 workgroups: the entry points' documented
// limits (count < 2^39 at 256 lanes, log_size <= 31, ...) all lie below that, which is asserted here and at no call site.
inline dim3 grid_1d(size_t count, unsigned threads = 256) {
    const size_t groups = (count + threads - 1) / threads;
    assert(groups < ((size_t)1 << 31));
    return dim3((unsigned)groups);
}

static constexpr int ZK_MSM_MAX_C = 21;  // largest Pippenger window (bits); 2^(c-1) buckets per set (the sort handles <= 2^20 x sets / 1024 super-buckets)

// bits of the sticky device status word (kernels atomicOr them in; zkhip_device_status reports and clears)
enum : uint32_t { ZK_STATUS_GATHER_RANGE = 1u, ZK_STATUS_MSM_PLAN_OVERFLOW = 2u, ZK_STATUS_LOOKUP_NOT_IN_TABLE = 4u, ZK_STATUS_LOOKUP_SORT_OVERFLOW = 8u };

struct zkhip_ctx;

// Owners of what the host holds on the device (last paragraph).  Each releases its resource when it goes out of scope, so a
// handle or a table set frees itself and a function that returns early leaks nothing.
// A device allocation:
struct DevBuf {
    uint32_t *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p = o.p;
            o.p = nullptr;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    int alloc(zkhip_ctx *ctx, size_t bytes);  // 0, or ZKHIP_ERR_OOM with ctx->last_error set
    operator uint32_t *() const { return p; }
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p); }
};
// A buffer in device (or page-locked host) memory that is kept across calls and only grows:
template <bool Pinned = false>
struct GrowBuf {
    void *p = nullptr;
    size_t cap = 0;
    GrowBuf() = default;
    GrowBuf(const GrowBuf &) = delete;
    GrowBuf &operator=(const GrowBuf &) = delete;
    GrowBuf(GrowBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    ~GrowBuf() { reset(); }
    void reset() {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    // room for `bytes`; a buffer that is too small is replaced by one of bytes + slack once ctx's stream has drained
    int reserve(zkhip_ctx *ctx, size_t bytes, size_t slack = 0);
    template <class T>
    T *as() const { return static_cast<T *>(p); }
};
// Events, a stream the context created itself, an instantiated graph:
struct ZkHipDelete {
    void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
    void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
    void operator()(hipGraphExec_t g) const { (void)hipGraphExecDestroy(g); }
};
using EventOwner = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, ZkHipDelete>;
using StreamOwner = std::unique_ptr<std::remove_pointer_t<hipStream_t>, ZkHipDelete>;
using GraphExecOwner = std::unique_ptr<std::remove_pointer_t<hipGraphExec_t>, ZkHipDelete>;
inline hipError_t zk_event_create(EventOwner &e, unsigned flags = hipEventDefault) {
    hipEvent_t raw = nullptr;
    const hipError_t rc = hipEventCreateWithFlags(&raw, flags);
    e.reset(raw);
    return rc;
}

struct zkhip_bases {
    int curve, group;
    size_t n;
    size_t stride_u32;  // u32 words per affine point (2 * coordinate limbs)
    DevBuf d;           // nslots tables of n Montgomery-form affine points each, (0,0) = infinity;
                        // the table of window w holds 2^off(w) P_i ("window tables": no Horner pass over the windows)
    int c_tab = 0, ntab = 1;  // window size the tables were built for (0: no tables) and the number of windows W
    // Window partition over GPUs: this object holds the tables of windows {w : w mod win_world == win_rank}
    // only, for ALL n points; an MSM over it yields the partial sum of those windows.  Slot 0 always holds the points
    // themselves (window 0, which belongs to rank 0; other ranks keep it as the source of their doubling chains).
    int win_rank = 0, win_world = 1;
    int nslots = 1;
    bool tables() const { return c_tab > 0; }
    int local_windows() const { return win_rank < ntab ? (ntab - win_rank + win_world - 1) / win_world : 0; }
    int slot_of_local(int lw) const { return lw + (win_rank != 0 ? 1 : 0); }  // local window lw = window win_rank + lw * win_world
};

struct ZkEventPair {
    EventOwner a, b;
};

struct ZkProfile {
    bool on = false;
    bool last_recorded = false;  // prof_begin recorded an event pair for the launch in flight
    std::string filter;          // non-empty: only kernels whose name starts with it are timed (fewer events in a timed region)
    std::vector<std::pair<std::string, ZkEventPair>> pending;
    std::vector<ZkEventPair> pool;
    std::map<std::string, std::pair<double, uint64_t>> acc;
};

// The device tables a context keeps across calls (the caches at the end of zkhip_ctx; protocol: table_cache.hpp)
struct NttTables {  // one radix-2 transform (ntt.hip: ntt_get_tables)
    int curve;
    size_t log_m;
    int inverse;
    bool has_coset;
    int smax, tile_log;  // the radix plan the per-pass tables were built for
    uint64_t omega[4], coset[4];
    int lo_bits;
    DevBuf d_tw[NTT_MAX_PASSES];     // store factors of pass i (i < passes - 1): m x 8 u32, Montgomery, saturated limbs
    DevBuf d_stage[NTT_MAX_PASSES];  // omega_R^q, q < R/2, Fu form (SL words)
    DevBuf d_prepost;                // coset: g^i (forward) or (1/m) g^-i (inverse), m x 8 u32
    DevBuf d_lo, d_hi;               // omega^i, omega^(i << lo_bits)          (Montgomery, SL words each)
    DevBuf d_clo, d_chi;             // g^i, g^(i << lo_bits), g = coset or coset^-1
    DevBuf d_scale;                  // [0] = 1/m (inverse) or 1 (forward), Montgomery
    DevBuf d_base;                   // [omega_eff, g_eff] (Montgomery)
};
struct NttExtTables {  // the coset factors of an n -> K n extension (ntt.hip: ntt_extend_t)
    int curve;
    size_t log_m, log_k;
    uint64_t omega_big[4];
    DevBuf d_pre;
};
struct DomTables {  // a step / extended radix-2 domain, or the 1 / Z entry of a basic domain's coset (domain.hip)
    int curve, kind;
    size_t m, n0, n1;
    uint64_t omega[4], shift[4], coset[4];
    bool has_coset;
    DevBuf d_T;       // step: (omega g)^i, i < big        (Montgomery, 8 words each)
    DevBuf d_Tinv;    // step: (omega g)^-i, i < small
    DevBuf d_consts;  // DC_* entries, Montgomery, 8 words each
    DevBuf d_zinv;    // has_coset: 1 / Z(g x_i) for part 0 by i mod nz, then one entry for part 1
    size_t nz = 1;
    uint64_t w0[4], w1[4];  // roots of the two sub-transforms
    uint64_t coset1[4];     // extended: g shift (the coset of the second sub-transform)
};

// a captured launch sequence (HIP graph) of one MSM / MSM batch, replayed when the same call comes again
struct ZkGraph {
    GraphExecOwner exec;
    uint64_t ws_epoch = 0;  // the workspace allocation the graph's addresses refer to
    DevBuf d_ptrs;          // batch: device array of the output pointers (kept with the graph)
};

struct zkhip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    StreamOwner own_stream;  // holds `stream` while it is the one the context created; empty on a borrowed stream (zkhip_set_stream)
    EventOwner order_event;  // zkhip_stream_wait: marks this context's stream for another context to wait on
    std::string last_error;
    // zkhip_malloc / zkhip_free keep freed blocks for reuse (sizes rounded to 64 KiB; a request takes a cached block up to 1/8 larger):
    // the polynomial-layer chains allocate the same GB-class temporaries again and again, and a raw hipMalloc / hipFree pair costs
    // milliseconds -- at times hundreds (measured: a 20-ms quotient chain with 170-230 ms outliers every third run).  "alloc_cache_mb"
    // caps what is kept (default 16 GiB of the 288; 0 turns the cache off); everything goes back at zkhip_destroy or when hipMalloc fails.
    std::multimap<size_t, void *> alloc_free;
    std::unordered_map<void *, size_t> alloc_live;
    size_t alloc_cached_bytes = 0, opt_alloc_cache_bytes = (size_t)16 << 30;
    std::mutex alloc_mutex;
    DevBuf d_status;  // sticky device-side error flags (ZK_STATUS_*), read and cleared by zkhip_device_status
    // bump-allocated workspace, grown on demand, reused across calls
    GrowBuf<> ws;
    size_t ws_off = 0, ws_floor = 0;  // ws_floor: start of the per-call region (a batch parks data below it)
    std::unordered_set<const void *> lds_configured;  // kernels whose dynamic-LDS limit was raised on this context's device
    // HIP graphs of repeated MSM calls (msm.hip: zk_graph_run)
    std::unordered_map<std::string, ZkGraph> graphs;
    std::unordered_map<std::string, int> graph_seen;
    uint64_t ws_epoch = 0;
    bool capturing = false;
    void *batch_dptrs_override = nullptr;  // during a batch capture: the graph-owned output-pointer array
    int opt_msm_graphs = 0;  // off: replaying the captured launch sequence measured no faster than issuing it
    GrowBuf<> msm_host_buf;  // zkhip_msm (scalars in host memory): result + scalars on the device, kept across calls
    // options (each is a row of options.hpp)
    int opt_msm_window_bits = 0;
    int opt_msm_sets = 0;          // bucket sets S with window tables (entry (i, w) -> set w mod S); 0: from the lane target
    int opt_msm_sort_tile_log = 14;  // 14: 2^14-entry sort tiles (the MSM owns the GPU); 13: 2^13; 12: 2^12 (kernels of another context run alongside)
    int opt_ec_ntt_table_lanes = 0;  // EC-NTT: lanes per multiplication launch = window tables held at once (0: as many as fit 1 GiB)
    int opt_msm_share_sort = 1;    // batches: consecutive members over the same scalars and table geometry share one sort (msm_same_entries)
    int opt_msm_tail_quads = 1;    // the tail's latency-bound group law.  0: lane pairs everywhere; 1: lane quads in the tail of small bucket sets (fu_quad.hpp) and one point per wave in level 2 of a lone MSM's two-level tail (fu_wide.hpp); any other value: the quads alone
    int opt_msm_tail_fold = 16;    // two-level tail (msm_core.hpp: row / column sums of the bucket index, then the old tail over 2 sets of ~sqrt(B) buckets) for table-backed sets of >= 2^k buckets; 0: off
    int opt_msm_tail_fold_g2 = 1;  // the two-level tail for G2 sets too (same threshold): a lone G2 MSM measures the same either way, a proof whose G2 MSM runs under its G1 MSMs gains the issue slots the shorter tail frees (Groth16 +2.6 %)
    int opt_msm_fold_run = 0;      // two-level tail: buckets a lane sums before the workgroup's tree (a power of two; 0: auto)
    int opt_msm_segment_log = -1;  // tail segments of 2^k buckets per lane; < 0: chosen from the lane count
    int opt_ntt_radix_log = 8;
    int opt_ntt_tile_log = 3;
    int opt_poly_coset_extend = 1;  // zkhip_poly_resize_dev n -> K n (K <= 16): the K - 1 new cosets by n-point transforms, the n known values copied (0: inverse + K n-point transform)
    int opt_ntt_pair = 1;  // log2 of the polynomials of a batch one NTT workgroup carries (1: pairs share indices, twiddles, factor-table reads)
    int opt_msm_precompute = 1;       // build window tables at upload for bases of >= opt_msm_precompute_min points
    int opt_msm_shard_rank = 0, opt_msm_shard_world = 1;  // window partition applied to bases uploaded from now on
    int opt_stream_priority = 0;      // < 0: the own stream was recreated with the highest priority, > 0: the lowest
    int opt_msm_precompute_min = 32;  // without tables the windows are combined by a serial Horner pass (~255 doublings on one lane: 3.8 ms)
    ZkProfile prof;
    // the per-index tables are m x 32 B each: the caches hold a few entries per size (a prover alternates between a handful of
    // (direction, coset) variants of one or two sizes), oldest out first
    TableCache<NttTables> ntt_tables{24};
    TableCache<NttExtTables> ntt_ext_tables{16};
    TableCache<DomTables> dom_tables{8};  // step / extended radix-2 domains and the basic domains' 1 / Z entries
    GrowBuf<> dom_ws;                     // scratch of zkhip_domain_fft_dev (the NTTs inside it use `ws`)

    zkhip_ctx() = default;
    ~zkhip_ctx();  // zkhip.hip: the release order of everything above

    int ws_reserve(size_t bytes) {
        if (bytes <= ws.cap) return 0;
        if (capturing) {  // growing means a synchronisation and new addresses: not inside a stream capture
            last_error = "workspace growth during graph capture";
            return ZKHIP_ERR_HIP;
        }
        ++ws_epoch;
        return ws.reserve(this, bytes, (bytes >> 3) + (1 << 20));
    }
    void ws_reset() { ws_off = ws_floor; }
    static size_t ws_round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    // the `drain` of the table caches' publish(): nothing enqueued may still read the entry that is about to go
    int stream_drain() {
        ZK_HIP_CHECK(this, hipStreamSynchronize(stream));
        return 0;
    }

    // ---- profiler
    void prof_begin(const char *name) {
        prof.last_recorded = false;
        if (!prof.on) return;
        if (!prof.filter.empty() && strncmp(name, prof.filter.c_str(), prof.filter.size()) != 0) return;
        prof.last_recorded = true;
        ZkEventPair ev;
        if (!prof.pool.empty()) {
            ev = std::move(prof.pool.back());
            prof.pool.pop_back();
        } else {
            (void)zk_event_create(ev.a);
            (void)zk_event_create(ev.b);
        }
        (void)hipEventRecord(ev.a.get(), stream);
        prof.pending.emplace_back(name, std::move(ev));
    }
    void prof_end() {
        if (!prof.on || !prof.last_recorded) return;
        (void)hipEventRecord(prof.pending.back().second.b.get(), stream);
    }
    void prof_collect() {
        if (prof.pending.empty()) return;
        (void)hipStreamSynchronize(stream);
        for (auto &p : prof.pending) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, p.second.a.get(), p.second.b.get());
            auto &a = prof.acc[p.first];
            a.first += ms;
            a.second += 1;
            prof.pool.push_back(std::move(p.second));
        }
        prof.pending.clear();
    }
};

inline int DevBuf::alloc(zkhip_ctx *ctx, size_t bytes) {
    reset();
    const hipError_t e = hipMalloc((void **)&p, bytes);
    if (e == hipSuccess) return 0;
    (void)hipGetLastError();
    ctx->last_error = "hipMalloc(" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e);
    return ZKHIP_ERR_OOM;
}
template <bool Pinned>
int GrowBuf<Pinned>::reserve(zkhip_ctx *ctx, size_t bytes, size_t slack) {
    if (bytes <= cap) return 0;
    if (p) ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // nothing enqueued may still use the old buffer
    reset();
    const hipError_t e = Pinned ? hipHostMalloc(&p, bytes + slack, hipHostMallocPortable) : hipMalloc(&p, bytes + slack);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        ctx->last_error = std::string(Pinned ? "hipHostMalloc(" : "hipMalloc(") + std::to_string(bytes + slack) + " bytes): " + hipGetErrorString(e);
        return ZKHIP_ERR_OOM;
    }
    cap = bytes + slack;
    return 0;
}

// Workspace layouts.  A call declares its buffers ONCE, as an object with a member
//     template <class Arena> void layout(Arena &a) { a.take(first, count); a.take(second, count); ... }
// which is walked twice: by WsCount to size the reservation, and by WsBump to hand the pointers out in the same order.
struct WsCount {
    size_t bytes = 0;
    template <class T>
    void take(T *&, size_t count) { bytes += zkhip_ctx::ws_round(count * sizeof(T)); }
};
struct WsBump {
    zkhip_ctx *ctx;
    template <class T>
    void take(T *&p, size_t count) {
        p = reinterpret_cast<T *>(ctx->ws.as<char>() + ctx->ws_off);
        ctx->ws_off += zkhip_ctx::ws_round(count * sizeof(T));
    }
};
template <class T>
struct WsOne {  // the layout of a call with a single buffer
    size_t count;
    T *p;
    template <class Arena>
    void layout(Arena &a) { a.take(p, count); }
};
template <class Layout>
size_t ws_bytes(Layout &l) {
    WsCount a;
    l.layout(a);
    return a.bytes;
}
// reserve the layout's bytes (+ `above`: room the caller hands out later) over ws_floor, place the buffers there and check that the
// walk stayed inside what was reserved
template <class Layout>
int ws_place(zkhip_ctx *ctx, Layout &l, size_t above = 0) {
    const size_t end = ctx->ws_floor + ws_bytes(l);
    ZK_TRY(ctx->ws_reserve(end + above));
    ctx->ws_reset();
    WsBump a{ctx};
    l.layout(a);
    if (ctx->ws_off > end || end + above > ctx->ws.cap) {
        ctx->last_error = "workspace layout took " + std::to_string(ctx->ws_off - ctx->ws_floor) + " bytes of " + std::to_string(end - ctx->ws_floor) + " reserved";
        return ZKHIP_ERR_RANGE;
    }
    return 0;
}

// How a small per-call table (pointers, challenges, a program image) gets to the device: this one route.  Its source is the caller's array or
// a function-local vector, and either may die when the call returns: by the runtime's own rule (hip_runtime_api.h, the note on hipMemcpyAsync:
// "if host or dest are not pinned, the memcpy will be performed synchronously") a source that is not page-locked has been consumed when
// hipMemcpyAsync returns.  That rule is also why a stream capture cannot take such a copy: inside one, a table must already sit in device
// memory the capture owns (msm.hip: ZkGraph::d_ptrs, handed over as batch_dptrs_override), so there is nothing to upload and the helper refuses.
inline int ws_upload(zkhip_ctx *ctx, void *d_dst, const void *src, size_t bytes) {
    if (ctx->capturing) {
        ctx->last_error = "host table upload during graph capture";
        return ZKHIP_ERR_HIP;
    }
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

// raise a kernel's dynamic-LDS limit once per context (the attribute is per device: a process may hold contexts on
// several GPUs, so a process-wide flag would skip it on the second device)
#define ZK_MAX_LDS(ctx, kernel, bytes)                                                                                              \
    do {                                                                                                                            \
        const void *fn__ = reinterpret_cast<const void *>(&kernel);                                                                 \
        if ((ctx)->lds_configured.insert(fn__).second)                                                                              \
            ZK_HIP_CHECK(ctx, hipFuncSetAttribute(fn__, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)));                 \
    } while (0)

// launch + profile wrapper: ZK_LAUNCH(ctx, "name", kernel, grid, block, lds, args...)
#define ZK_LAUNCH(ctx, name, kernel, grid, block, lds, ...)                        \
    do {                                                                           \
        (ctx)->prof_begin(name);                                                   \
        hipLaunchKernelGGL(kernel, grid, block, lds, (ctx)->stream, __VA_ARGS__);  \
        (ctx)->prof_end();                                                         \
        ZK_HIP_CHECK(ctx, hipGetLastError());                                      \
    } while (0)

// implemented in msm.hip / ntt.hip
int zk_msm_run(zkhip_ctx *ctx, const zkhip_bases *bases, size_t offset, size_t n, const uint32_t *d_scalars, uint32_t *d_out_jac);
int zk_msm_run_batch(zkhip_ctx *ctx, size_t count, const zkhip_bases *const *bases, const size_t *offsets, const size_t *ns,
                     const uint32_t *const *d_scalars, uint32_t *const *d_outs);
size_t zk_coord_limbs64(int curve, int group);  // u64 limbs per coordinate (Fq: 6/4, Fq2: 12/8)
int zk_bases_to_mont(zkhip_ctx *ctx, zkhip_bases *b, const uint32_t *d_canonical, const uint8_t *d_inf);
size_t zk_point_words(int curve, int group);
int zk_msm_auto_window(size_t n);
int zk_scalar_bits(int curve);  // bit length of the scalar-field modulus
int zk_bases_decompress(zkhip_ctx *ctx, zkhip_bases *b, const uint8_t *d_octets, uint32_t *d_err);  // wire.hip
void zk_graphs_clear(zkhip_ctx *ctx);  // destroy the cached MSM graphs
int zk_bases_precompute(zkhip_ctx *ctx, zkhip_bases *b);  // u32 words per affine point in device buffers
int zk_bases_from_mont(zkhip_ctx *ctx, const zkhip_bases *b, size_t offset, size_t n, uint32_t *d_out, uint8_t *d_inf);
int zk_bases_mul(zkhip_ctx *ctx, zkhip_bases *b, const uint32_t *d_base_canonical /* nullable: generator */, const uint32_t *d_scalars);
int zk_jac_sum(zkhip_ctx *ctx, int curve, int group, const uint32_t *d_pts, size_t count, uint32_t *d_out);
int zk_jac_to_affine(zkhip_ctx *ctx, int curve, int group, const uint32_t *d_jac, uint32_t *d_aff, uint8_t *d_inf);
int zk_ntt_run(zkhip_ctx *ctx, int curve, uint32_t *d_data, size_t log_m, size_t batch, const uint64_t *omega, int inverse,
               const uint64_t *coset);
int zk_ntt_extend(zkhip_ctx *ctx, int curve, uint32_t *d_coeffs, size_t log_m, size_t batch, const uint64_t *omega, uint32_t *d_out, size_t log_k,
                  const uint64_t *omega_big);
int zk_msm_host_reserve(zkhip_ctx *ctx, size_t n);  // zkhip.hip: ctx->msm_host_buf holds 512 B of result + n scalars
bool zk_fr_canonical(int curve, const uint64_t *c);  // ipa.hip: c (4 limbs) below the modulus of the curve's scalar field?
// ecntt.hip: slot 0 of dst (2^log_m G1 points, allocated) <- the inverse group DFT of src's points offset .. offset + 2^log_m; arguments checked by the caller.
// glv = false takes the plain 65-window ladder (the measurement's other arm)
int zk_bases_lagrange(zkhip_ctx *ctx, const zkhip_bases *src, size_t offset, size_t log_m, const uint64_t *omega, bool glv, zkhip_bases *dst);
// ecntt.hip: slot 0 of dst (n points of src's curve and group, allocated) <- s_i * (src's point offset + i); the scalars are the n resident 8-word values at
// d_scalars or, when that is null, coeff * ratio^(e0 + i) (coeff nullable: 1).  Arguments checked by the caller.
int zk_bases_scale(zkhip_ctx *ctx, const zkhip_bases *src, size_t offset, size_t n, const uint32_t *d_scalars, const uint64_t *ratio, const uint64_t *coeff,
                   uint32_t e0, zkhip_bases *dst);
