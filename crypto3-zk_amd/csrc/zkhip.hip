// extern "C" surface of libzkhip.so (declared in include/zkhip.h).  No torch types, no CPU fallback:
// if no HIP device is usable, zkhip_init fails and nothing else can be called.
#include <algorithm>
#include <cstdlib>

#include "ctx.hpp"
#include "domain.hpp"
#include "field_consts.hpp"
#include "msm_recode.hpp"
#include "zk_defs.hpp"

using namespace zkhip;

static int check_device(zkhip_ctx *ctx) {
    ZK_ENTER(ctx);
    return 0;
}

struct DownloadBuffers {  // zkhip_bases_download: n affine points of `words` u32 each and their infinity flags
    size_t n, words;
    uint32_t *xy;
    uint8_t *inf;
    template <class Arena>
    void layout(Arena &a) {
        a.take(xy, n * words);
        a.take(inf, n);
    }
};
struct ToAffineBuffers {  // zkhip_jacobian_to_affine: one point in, one out; cw = u32 words per coordinate
    size_t cw;
    uint32_t *jac, *aff;
    uint8_t *inf;
    template <class Arena>
    void layout(Arena &a) {
        a.take(jac, 3 * cw);
        a.take(aff, 2 * cw);
        a.take(inf, 16);
    }
};

extern "C" {

const char *zkhip_strerror(int status) {
    switch (status) {
        case ZKHIP_OK: return "ok";
        case ZKHIP_ERR_NO_DEVICE: return "no usable HIP device (zkhip has no CPU fallback)";
        case ZKHIP_ERR_INVALID: return "invalid argument";
        case ZKHIP_ERR_HIP: return "HIP runtime error (see zkhip_last_error)";
        case ZKHIP_ERR_OOM: return "out of device memory";
        case ZKHIP_ERR_RANGE: return "size or offset out of range";
        case ZKHIP_ERR_NOT_FOUND: return "search ended without a result";
        default: return "unknown status";
    }
}

// Process-wide view of the block caches: which context a live block of zkhip_malloc belongs to -- so that zkhip_free through
// ANOTHER context of the process settles the block with its owner instead of leaving a stale entry there --, and which contexts exist,
// so that an out-of-memory in one of them can empty its siblings' caches on the same device.  Lock order: g_alloc_mutex, then a
// context's alloc_mutex; never the other way round.
static std::mutex g_alloc_mutex;
static std::unordered_map<void *, zkhip_ctx *> g_block_owner;
static std::unordered_set<zkhip_ctx *> g_contexts;

int zkhip_init(int device_id, zkhip_ctx **out) {
    if (!out) return ZKHIP_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return ZKHIP_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= count) return ZKHIP_ERR_INVALID;
    if (hipSetDevice(device_id) != hipSuccess) return ZKHIP_ERR_NO_DEVICE;
    std::unique_ptr<zkhip_ctx> ctx(new zkhip_ctx());
    ctx->device = device_id;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) return ZKHIP_ERR_HIP;
    ctx->own_stream.reset(ctx->stream);
    if (ctx->d_status.alloc(ctx.get(), 4) != 0 || hipMemset(ctx->d_status, 0, 4) != hipSuccess) return ZKHIP_ERR_OOM;
    {
        std::lock_guard<std::mutex> g(g_alloc_mutex);
        g_contexts.insert(ctx.get());
    }
    // A/B runs of programs that create their own contexts (the bench library, the shim's default context): ZKHIP_OPTIONS="name=value,name=value"
    // is applied to every new context; an unknown name or a malformed entry is ignored (the variable is for measurements, not for deployments)
    if (const char *env = getenv("ZKHIP_OPTIONS"))
        zk_options_parse(env, [&](const char *name, int64_t value) { (void)zkhip_set_option(ctx.get(), name, value); });
    *out = ctx.release();
    return ZKHIP_OK;
}

static void alloc_cache_flush(zkhip_ctx *ctx);

}  // extern "C"

// Everything the context holds goes here, in this order: the stream drains first, the tables, events and graphs go while it still exists,
// the buffers after the allocator cache, the stream -- if the context created it -- last.
zkhip_ctx::~zkhip_ctx() {
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);
    ntt_tables.clear();
    ntt_ext_tables.clear();
    dom_tables.clear();
    dom_ws.reset();
    prof.pending.clear();
    prof.pool.clear();
    zk_graphs_clear(this);
    order_event.reset();
    {
        /* the cached blocks go back to the driver; blocks the caller still HOLDS (a shared_ptr handle of the shim that outlives its context)
           are left alone and lose their owner: a later zkhip_free through any context hands them to hipFree (they used to be
           freed here, under the handle) */
        std::lock_guard<std::mutex> g(g_alloc_mutex);
        std::lock_guard<std::mutex> lock(alloc_mutex);
        alloc_cache_flush(this);
        for (auto &e : alloc_live) g_block_owner.erase(e.first);
        alloc_live.clear();
        g_contexts.erase(this);
    }
    msm_host_buf.reset();
    ws.reset();
    d_status.reset();
    own_stream.reset();
}

extern "C" {

void zkhip_destroy(zkhip_ctx *ctx) {
    if (ctx) delete ctx;
}

int zkhip_device(const zkhip_ctx *ctx) { return ctx ? ctx->device : -1; }

int zkhip_stream_wait(zkhip_ctx *waiter, zkhip_ctx *signal) {
    if (!waiter || !signal || waiter->device != signal->device) return ZKHIP_ERR_INVALID;
    if (waiter == signal) return ZKHIP_OK;
    ZK_HIP_CHECK(waiter, hipSetDevice(waiter->device));
    if (!signal->order_event) ZK_HIP_CHECK(waiter, zk_event_create(signal->order_event, hipEventDisableTiming));
    ZK_HIP_CHECK(waiter, hipEventRecord(signal->order_event.get(), signal->stream));
    ZK_HIP_CHECK(waiter, hipStreamWaitEvent(waiter->stream, signal->order_event.get(), 0));
    return ZKHIP_OK;
}

const char *zkhip_last_error(const zkhip_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int zkhip_set_stream(zkhip_ctx *ctx, void *hip_stream) {
    if (!ctx) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->own_stream.reset();
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    return ZKHIP_OK;
}

int zkhip_sync(zkhip_ctx *ctx) {
    if (!ctx) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ZKHIP_OK;
}

int zkhip_device_status(zkhip_ctx *ctx, uint32_t *flags) {
    if (!ctx) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    uint32_t f = 0;
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(&f, ctx->d_status, 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (f) ZK_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_status, 0, 4, ctx->stream));
    if (flags) *flags = f;
    if (f) {
        ctx->last_error = std::string("device status:") + ((f & ZK_STATUS_GATHER_RANGE) ? " gather index out of range;" : "") +
                          ((f & ZK_STATUS_MSM_PLAN_OVERFLOW) ? " MSM large-bucket plan overflow;" : "");
        return ZKHIP_ERR_RANGE;
    }
    return ZKHIP_OK;
}

int zkhip_set_option(zkhip_ctx *ctx, const char *name, int64_t value) {
    if (!ctx || !name) return ZKHIP_ERR_INVALID;
    const OptRow<zkhip_ctx> *row = zk_option_find<zkhip_ctx>(name);
    if (!row) return ZKHIP_ERR_INVALID;
    if (row->admit != OPT_CUSTOM) {
        zk_option_store(*ctx, *row, value);
    } else if (!row->member) {  // alloc_cache_mb
        if (value < 0) return ZKHIP_ERR_RANGE;
        std::lock_guard<std::mutex> g(g_alloc_mutex);
        std::lock_guard<std::mutex> lock(ctx->alloc_mutex);
        ctx->opt_alloc_cache_bytes = (size_t)value << 20;
        if (ctx->alloc_cached_bytes > ctx->opt_alloc_cache_bytes) alloc_cache_flush(ctx);
    } else if (row->member == &zkhip_ctx::opt_msm_shard_world) {
        if (value < 1 || value > 64) return ZKHIP_ERR_RANGE;
        ctx->opt_msm_shard_world = (int)value;
        if (ctx->opt_msm_shard_rank >= ctx->opt_msm_shard_world) ctx->opt_msm_shard_rank = 0;
    } else if (row->member == &zkhip_ctx::opt_msm_shard_rank) {
        if (value < 0 || value >= ctx->opt_msm_shard_world) return ZKHIP_ERR_RANGE;
        ctx->opt_msm_shard_rank = (int)value;
    } else if (row->member == &zkhip_ctx::opt_stream_priority) {
        // the context's OWN stream is recreated with a scheduling priority: < 0 the highest the device offers, > 0 the
        // lowest, 0 the default.  Two contexts on one GPU (the Groth16 shim's main and G2 streams) can so decide whose workgroups go first.
        if (!ctx->own_stream) return ZKHIP_ERR_INVALID;
        ZK_ENTER(ctx);
        int least = 0, greatest = 0;
        ZK_HIP_CHECK(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
        ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        hipStream_t s = nullptr;
        ZK_HIP_CHECK(ctx, hipStreamCreateWithPriority(&s, hipStreamNonBlocking, value < 0 ? greatest : (value > 0 ? least : 0)));
        ctx->own_stream.reset(s);
        ctx->stream = s;
        ctx->opt_stream_priority = (int)value;
        zk_graphs_clear(ctx);
    } else {
        return ZKHIP_ERR_INVALID;  // an OPT_CUSTOM row without its code above
    }
    return ZKHIP_OK;
}

int zkhip_get_option(const zkhip_ctx *ctx, const char *name, int64_t *value) {
    if (!ctx || !name || !value) return ZKHIP_ERR_INVALID;
    const OptRow<zkhip_ctx> *row = zk_option_find<zkhip_ctx>(name);
    if (!row) return ZKHIP_ERR_INVALID;
    *value = row->member ? ctx->*row->member : (int64_t)(ctx->opt_alloc_cache_bytes >> 20);
    return ZKHIP_OK;
}

// give every cached block back to the driver; the caller holds g_alloc_mutex and ctx->alloc_mutex
static void alloc_cache_flush(zkhip_ctx *ctx) {
    for (auto &e : ctx->alloc_free) {
        g_block_owner.erase(e.second);
        (void)hipFree(e.second);
    }
    ctx->alloc_free.clear();
    ctx->alloc_cached_bytes = 0;
}
int zkhip_malloc(zkhip_ctx *ctx, size_t bytes, void **dptr) {
    if (!ctx || !dptr) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    const size_t want = ((bytes ? bytes : 1) + 0xFFFF) & ~(size_t)0xFFFF;
    {
        std::lock_guard<std::mutex> lock(ctx->alloc_mutex);
        auto it = ctx->alloc_free.lower_bound(want);
        if (it != ctx->alloc_free.end() && it->first <= want + (want >> 3)) {  // a cached block of this size class (blocks enter the cache after a device sync)
            *dptr = it->second;
            ctx->alloc_cached_bytes -= it->first;
            ctx->alloc_live[*dptr] = it->first;
            ctx->alloc_free.erase(it);
            return ZKHIP_OK;  // its owner entry was kept while it sat in the cache
        }
    }
    hipError_t e = hipMalloc(dptr, want);
    if (e != hipSuccess) {  // out of memory: the caches of EVERY context on this device go back to the driver (a shim process holds several), then once more
        (void)hipGetLastError();
        std::lock_guard<std::mutex> g(g_alloc_mutex);
        for (zkhip_ctx *c : g_contexts)
            if (c->device == ctx->device) {
                std::lock_guard<std::mutex> lock(c->alloc_mutex);
                alloc_cache_flush(c);
            }
        e = hipMalloc(dptr, want);
    }
    ZK_HIP_CHECK(ctx, e);
    std::lock_guard<std::mutex> g(g_alloc_mutex);
    std::lock_guard<std::mutex> lock(ctx->alloc_mutex);
    ctx->alloc_live[*dptr] = want;
    g_block_owner[*dptr] = ctx;
    return ZKHIP_OK;
}
int zkhip_free(zkhip_ctx *ctx, void *dptr) {
    if (!ctx) return ZKHIP_ERR_INVALID;
    if (!dptr) return ZKHIP_OK;
    // hipFree used to synchronise the whole device before the block could be handed out again; a block entering the cache gets the same
    // guarantee -- no stream of ANY context (a scheme's upload stream, the prover's G2 stream) still reads or writes it.  The device
    // that is drained is the one the BLOCK lives on (its owner's; ADVICE r5: a free through a context on another GPU used to drain that
    // GPU instead), ctx's own for a block no context owns.
    int block_device = ctx->device;
    {
        std::lock_guard<std::mutex> g(g_alloc_mutex);
        auto own = g_block_owner.find(dptr);
        if (own != g_block_owner.end()) block_device = own->second->device;
    }
    ZK_HIP_CHECK(ctx, hipSetDevice(block_device));
    ZK_HIP_CHECK(ctx, hipDeviceSynchronize());
    std::lock_guard<std::mutex> g(g_alloc_mutex);
    auto own = g_block_owner.find(dptr);
    if (own == g_block_owner.end()) {  // not a live block of any context's zkhip_malloc (or its context is gone): the driver's
        ZK_HIP_CHECK(ctx, hipFree(dptr));
        return ZKHIP_OK;
    }
    zkhip_ctx *owner = own->second;  // the block is settled with the context that allocated it, whichever context it is freed through
    std::lock_guard<std::mutex> lock(owner->alloc_mutex);
    auto it = owner->alloc_live.find(dptr);
    if (it == owner->alloc_live.end()) return ZKHIP_ERR_INVALID;  // a double free: the block already sits in the owner's cache
    const size_t sz = it->second;
    owner->alloc_live.erase(it);
    if (sz <= owner->opt_alloc_cache_bytes && owner->alloc_cached_bytes + sz <= owner->opt_alloc_cache_bytes) {
        owner->alloc_free.emplace(sz, dptr);
        owner->alloc_cached_bytes += sz;
        return ZKHIP_OK;
    }
    g_block_owner.erase(own);
    ZK_HIP_CHECK(ctx, hipFree(dptr));
    return ZKHIP_OK;
}
int zkhip_memcpy_h2d(zkhip_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ZKHIP_OK;
}
int zkhip_memcpy_h2d_async(zkhip_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return ZKHIP_OK;
}
int zkhip_host_alloc(zkhip_ctx *ctx, size_t bytes, void **hptr) {
    if (!ctx || !hptr) return ZKHIP_ERR_INVALID;
    ZK_ENTER(ctx);
    ZK_HIP_CHECK(ctx, hipHostMalloc(hptr, bytes ? bytes : 1, hipHostMallocPortable));  // page-locked for EVERY device: a group's members upload from one staging buffer
    return ZKHIP_OK;
}
int zkhip_host_free(zkhip_ctx *ctx, void *hptr) {
    if (!ctx) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    ZK_HIP_CHECK(ctx, hipHostFree(hptr));
    return ZKHIP_OK;
}
int zkhip_memcpy_d2h(zkhip_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ZKHIP_OK;
}

int zkhip_memcpy_d2h_async(zkhip_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return ZKHIP_OK;
}

int zkhip_memcpy_d2d_async(zkhip_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return ZKHIP_OK;
}

int zkhip_memcpy_2d_d2d_async(zkhip_ctx *ctx, void *dst, size_t dst_pitch, const void *src, size_t src_pitch, size_t width, size_t rows) {
    if (!ctx) return ZKHIP_ERR_INVALID;
    if (width == 0 || rows == 0) return ZKHIP_OK;
    if (!dst || !src || width > dst_pitch || width > src_pitch) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    if (dst_pitch >= ((size_t)1 << 31) || src_pitch >= ((size_t)1 << 31)) {  // beyond the 2D engine's pitch range (a 2^27-point domain at step 1): row by row
        for (size_t r = 0; r < rows; ++r)
            ZK_HIP_CHECK(ctx, hipMemcpyAsync(static_cast<char *>(dst) + r * dst_pitch, static_cast<const char *>(src) + r * src_pitch, width, hipMemcpyDeviceToDevice,
                                             ctx->stream));
        return ZKHIP_OK;
    }
    ZK_HIP_CHECK(ctx, hipMemcpy2DAsync(dst, dst_pitch, src, src_pitch, width, rows, hipMemcpyDeviceToDevice, ctx->stream));
    return ZKHIP_OK;
}

// ---- bases ------------------------------------------------------------------------------------------
static int bases_alloc(zkhip_ctx *ctx, int curve, int group, size_t n, std::unique_ptr<zkhip_bases> &out, bool tables = true) {
    if (!zk_curve_group_known(curve, group)) return ZKHIP_ERR_INVALID;
    std::unique_ptr<zkhip_bases> b(new zkhip_bases());
    b->curve = curve;
    b->group = group;
    b->n = n;
    b->stride_u32 = zk_point_words(curve, group);
    const bool shard = ctx->opt_msm_shard_world > 1;
    if (tables && ctx->opt_msm_precompute && n >= (size_t)ctx->opt_msm_precompute_min) {
        b->c_tab = ctx->opt_msm_window_bits > 0 ? std::max(2, std::min(ZK_MSM_MAX_C, ctx->opt_msm_window_bits)) : zk_msm_auto_window(n);
        b->ntab = msm_windows(zk_scalar_bits(curve), b->c_tab);
        if (shard) {
            b->win_rank = ctx->opt_msm_shard_rank;
            b->win_world = ctx->opt_msm_shard_world;
        }
        b->nslots = shard ? b->local_windows() + (b->win_rank != 0 ? 1 : 0) : b->ntab;
        if (b->nslots < 1) b->nslots = 1;
    } else if (shard) {
        // too few points for tables: the whole (tiny) MSM is rank 0's, the other ranks contribute the point at infinity
        b->win_rank = ctx->opt_msm_shard_rank;
        b->win_world = ctx->opt_msm_shard_world;
    }
    int rc = b->d.alloc(ctx, std::max<size_t>(1, n) * b->nslots * b->stride_u32 * 4);
    if (rc && b->tables() && !shard) {
        // the window tables do not fit (ntab x n points): keep the points alone; the MSM then folds the windows by the
        // Horner pass of msm_final instead of bucket-wise
        b->ntab = 1;
        b->c_tab = 0;
        b->nslots = 1;
        rc = b->d.alloc(ctx, std::max<size_t>(1, n) * b->stride_u32 * 4);
    }
    ZK_TRY(rc);
    out = std::move(b);
    return 0;
}

// the end of every constructor of bases: the window tables, the stream drained (the caller's temporaries go when it returns), the handle handed over
static int bases_finish(zkhip_ctx *ctx, std::unique_ptr<zkhip_bases> &b, zkhip_bases **out) {
    ZK_TRY(zk_bases_precompute(ctx, b.get()));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *out = b.release();
    return ZKHIP_OK;
}

}  // extern "C"

// Every coordinate of the n affine points (4 u64 limbs each; flagged points skipped) below the modulus of P?
template <class P>
static bool coords_canonical(const uint64_t *xy, const uint8_t *inf, size_t n) {
    uint64_t m[4];
    for (int i = 0; i < 4; ++i) m[i] = (uint64_t)P::mod(2 * i) | ((uint64_t)P::mod(2 * i + 1) << 32);
    for (size_t i = 0; i < n; ++i) {
        if (inf && inf[i]) continue;
        for (int k = 0; k < 2; ++k) {
            const uint64_t *c = xy + (2 * i + k) * 4;
            int j = 3;
            while (j > 0 && c[j] == m[j]) --j;
            if (c[j] >= m[j]) return false;
        }
    }
    return true;
}

extern "C" {

int zkhip_bases_upload(zkhip_ctx *ctx, int curve, int group, const uint64_t *affine_xy, const uint8_t *is_infinity, size_t n,
                       zkhip_bases **out) {
    if (!ctx || !out || (n && !affine_xy)) return ZKHIP_ERR_INVALID;
    // Pallas and Vesta: a 255-bit modulus in 256-bit words leaves room for values in [p, 2^256).  They are refused here, on the host, before
    // anything is allocated (the two older ids keep what they have always done with such a coordinate: it is taken mod p).
    if (group == GROUP_G1 && ((curve == CURVE_PALLAS && !coords_canonical<PallasFq>(affine_xy, is_infinity, n)) ||
                              (curve == CURVE_VESTA && !coords_canonical<VestaFq>(affine_xy, is_infinity, n)))) {
        ctx->last_error = "zkhip_bases_upload: a coordinate is not below the base-field modulus";
        return ZKHIP_ERR_INVALID;
    }
    ZK_TRY(check_device(ctx));
    std::unique_ptr<zkhip_bases> b;
    ZK_TRY(bases_alloc(ctx, curve, group, n, b));
    DevBuf d_canon, d_inf;
    if (n) {
        const size_t cbytes = n * 2 * zk_coord_limbs64(curve, group) * 8;
        ZK_TRY(d_canon.alloc(ctx, cbytes));
        ZK_HIP_CHECK(ctx, hipMemcpyAsync(d_canon, affine_xy, cbytes, hipMemcpyHostToDevice, ctx->stream));
        if (is_infinity) {
            ZK_TRY(d_inf.alloc(ctx, n));
            ZK_HIP_CHECK(ctx, hipMemcpyAsync(d_inf, is_infinity, n, hipMemcpyHostToDevice, ctx->stream));
        }
        ZK_TRY(zk_bases_to_mont(ctx, b.get(), d_canon, d_inf.as<uint8_t>()));
    }
    return bases_finish(ctx, b, out);
}

int zkhip_bases_upload_compressed(zkhip_ctx *ctx, int curve, int group, const uint8_t *octets, size_t n, zkhip_bases **out) {
    ZK_ARGS_PAIRING(ctx, curve);
    if (!out || (n && !octets)) return ZKHIP_ERR_INVALID;
    if (curve != CURVE_BLS12_381) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    std::unique_ptr<zkhip_bases> b;
    ZK_TRY(bases_alloc(ctx, curve, group, n, b));
    DevBuf d_oct;
    if (n) {
        const size_t bytes = n * (group == GROUP_G2 ? 96 : 48);
        ZK_TRY(d_oct.alloc(ctx, bytes + 16));
        uint32_t *d_err = reinterpret_cast<uint32_t *>(d_oct.as<uint8_t>() + ((bytes + 3) & ~(size_t)3));
        ZK_HIP_CHECK(ctx, hipMemcpyAsync(d_oct, octets, bytes, hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP_CHECK(ctx, hipMemsetAsync(d_err, 0, 4, ctx->stream));
        ZK_TRY(zk_bases_decompress(ctx, b.get(), d_oct.as<uint8_t>(), d_err));
        uint32_t rejected = 0;
        ZK_HIP_CHECK(ctx, hipMemcpyAsync(&rejected, d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (rejected) {
            ctx->last_error = std::to_string(rejected) + " point encoding(s) rejected (flags, x >= p, or x not on the curve)";
            return ZKHIP_ERR_INVALID;
        }
    }
    return bases_finish(ctx, b, out);
}

// standard generators, canonical u32 limbs (x | y)
static const uint64_t GEN_BLS_G1[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL,
                                        0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL, 0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL,
                                        0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL, 0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
static const uint64_t GEN_BLS_G2[24] = {
    0xd48056c8c121bdb8ULL, 0x0bac0326a805bbefULL, 0xb4510b647ae3d177ULL, 0xc6e47ad4fa403b02ULL, 0x260805272dc51051ULL, 0x024aa2b2f08f0a91ULL,
    0xe5ac7d055d042b7eULL, 0x334cf11213945d57ULL, 0xb5da61bbdc7f5049ULL, 0x596bd0d09920b61aULL, 0x7dacd3a088274f65ULL, 0x13e02b6052719f60ULL,
    0xe193548608b82801ULL, 0x923ac9cc3baca289ULL, 0x6d429a695160d12cULL, 0xadfd9baa8cbdd3a7ULL, 0x8cc9cdc6da2e351aULL, 0x0ce5d527727d6e11ULL,
    0xaaa9075ff05f79beULL, 0x3f370d275cec1da1ULL, 0x267492ab572e99abULL, 0xcb3e287e85a763afULL, 0x32acd2b02bc28b99ULL, 0x0606c4a02ea734ccULL};
static const uint64_t GEN_BN_G1[8] = {1, 0, 0, 0, 2, 0, 0, 0};
// Pallas (p - 1, 2) and Vesta (q - 1, 2): the point (-1, 2) of y^2 = x^3 + 5
static const uint64_t GEN_PALLAS_G1[8] = {0x992d30ed00000000ULL, 0x224698fc094cf91bULL, 0, 0x4000000000000000ULL, 2, 0, 0, 0};
static const uint64_t GEN_VESTA_G1[8] = {0x8c46eb2100000000ULL, 0x224698fc0994a8ddULL, 0, 0x4000000000000000ULL, 2, 0, 0, 0};
static const uint64_t GEN_BN_G2[16] = {0x46debd5cd992f6edULL, 0x674322d4f75edaddULL, 0x426a00665e5c4479ULL, 0x1800deef121f1e76ULL,
                                       0x97e485b7aef312c2ULL, 0xf1aa493335a9e712ULL, 0x7260bfb731fb5d25ULL, 0x198e9393920d483aULL,
                                       0x4ce6cc0166fa7daaULL, 0xe3d1e7690c43d37bULL, 0x4aab71808dcb408fULL, 0x12c85ea5db8c6debULL,
                                       0x55acdadcd122975bULL, 0xbc4b313370b38ef3ULL, 0xec9e99ad690c3395ULL, 0x090689d0585ff075ULL};

int zkhip_bases_from_scalars(zkhip_ctx *ctx, int curve, int group, const uint64_t *base_affine_xy, const uint64_t *scalars, size_t n,
                             zkhip_bases **out) {
    if (!ctx || !out || (n && !scalars)) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    std::unique_ptr<zkhip_bases> b;
    ZK_TRY(bases_alloc(ctx, curve, group, n, b));
    const uint64_t *gen = base_affine_xy;
    if (!gen)
        gen = curve == CURVE_PALLAS  ? GEN_PALLAS_G1
              : curve == CURVE_VESTA ? GEN_VESTA_G1
              : curve == CURVE_BLS12_381 ? (group == GROUP_G1 ? GEN_BLS_G1 : GEN_BLS_G2)
                                         : (group == GROUP_G1 ? GEN_BN_G1 : GEN_BN_G2);
    DevBuf d_s, d_g;
    if (n) {
        const size_t gbytes = 2 * zk_coord_limbs64(curve, group) * 8;
        ZK_TRY(d_s.alloc(ctx, n * 32));
        ZK_TRY(d_g.alloc(ctx, gbytes));
        ZK_HIP_CHECK(ctx, hipMemcpyAsync(d_s, scalars, n * 32, hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP_CHECK(ctx, hipMemcpyAsync(d_g, gen, gbytes, hipMemcpyHostToDevice, ctx->stream));
        ZK_TRY(zk_bases_mul(ctx, b.get(), d_g, d_s));
    }
    return bases_finish(ctx, b, out);
}

// out row d_rows[j] (or first + j) <- src row j; a row is `stride` words
__global__ void bases_spread_rows(const uint32_t *__restrict__ src, size_t count, uint32_t stride, const uint32_t *__restrict__ d_rows, uint32_t first,
                                  uint32_t n_total, uint32_t *__restrict__ out, uint32_t *__restrict__ status) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count * stride) return;
    const size_t j = g / stride;
    const uint32_t w = (uint32_t)(g % stride), row = d_rows ? d_rows[j] : first + (uint32_t)j;
    // rows must be in range AND strictly increasing (the sparse B query's index list, r1cs_gg_ppzksnark.hpp check_b_indices): a
    // repeated row would silently overwrite a point, so it raises the same sticky flag as a row beyond the end
    if (row >= n_total || (d_rows && j + 1 < count && d_rows[j + 1] <= row)) {
        if (w == 0) atomicOr(status, ZK_STATUS_GATHER_RANGE);
        if (row >= n_total) return;
    }
    out[(size_t)row * stride + w] = src[g];
}

int zkhip_bases_spread(zkhip_ctx *ctx, const zkhip_bases *src, const uint32_t *d_rows, size_t first, size_t n_total, zkhip_bases **out) {
    if (!ctx || !src || !out) return ZKHIP_ERR_INVALID;
    if (n_total >= ((size_t)1 << 32) || (!d_rows && first + src->n > n_total)) return ZKHIP_ERR_RANGE;
    if (src->n * src->stride_u32 >= ((size_t)1 << 39)) return ZKHIP_ERR_RANGE;  // one lane per word: the grid must fit 32 bits
    ZK_TRY(check_device(ctx));
    std::unique_ptr<zkhip_bases> b;
    ZK_TRY(bases_alloc(ctx, src->curve, src->group, n_total, b));
    if (n_total) {
        ZK_HIP_CHECK(ctx, hipMemsetAsync(b->d, 0, n_total * b->stride_u32 * 4, ctx->stream));  // (0, 0): the point at infinity
        if (src->n) {
            const size_t lanes = src->n * src->stride_u32;
            ZK_LAUNCH(ctx, "bases_spread_rows", bases_spread_rows, grid_1d(lanes), dim3(256), 0, src->d, src->n,
                      (uint32_t)src->stride_u32, d_rows, (uint32_t)first, (uint32_t)n_total, b->d, ctx->d_status);
        }
    }
    return bases_finish(ctx, b, out);
}

// The Lagrange basis of a range of an SRS (include/zkhip.h): every refusal before any launch, the transform into slot 0 of a new object (ecntt.hip),
// then the window tables as every constructor builds them.
static int bases_lagrange(zkhip_ctx *ctx, const zkhip_bases *b, size_t offset, size_t log_m, const uint64_t *omega, bool glv, zkhip_bases **out) {
    if (out) *out = nullptr;
    if (!b || !omega || !out) return ZKHIP_ERR_INVALID;
    ZK_ARGS(ctx, b->curve);
    if (b->group != GROUP_G1 || !zk_fr_canonical(b->curve, omega)) return ZKHIP_ERR_INVALID;
    if (log_m > 26 || offset > b->n || ((size_t)1 << log_m) > b->n - offset) return ZKHIP_ERR_RANGE;
    if (!zk_dom_primitive_root(b->curve, omega, log_m)) {
        ctx->last_error = "zkhip_bases_lagrange: omega is not a primitive 2^" + std::to_string(log_m) + "-th root of unity";
        return ZKHIP_ERR_INVALID;
    }
    ZK_TRY(check_device(ctx));
    std::unique_ptr<zkhip_bases> r;
    ZK_TRY(bases_alloc(ctx, b->curve, b->group, (size_t)1 << log_m, r));
    ZK_TRY(zk_bases_lagrange(ctx, b, offset, log_m, omega, glv, r.get()));
    return bases_finish(ctx, r, out);
}

int zkhip_bases_lagrange(zkhip_ctx *ctx, const zkhip_bases *b, size_t offset, size_t log_m, const uint64_t *omega, zkhip_bases **out) {
    return bases_lagrange(ctx, b, offset, log_m, omega, true, out);
}
// Not part of the ABI (no declaration in include/zkhip.h): the same constructor over the plain 65-window ladder, Pallas and Vesta only --
// the other arm of the measurement that chose GLV (tools/bench_lagrange.py, DESIGN.md section on the IPA).
int zkhip_bench_bases_lagrange_plain(zkhip_ctx *ctx, const zkhip_bases *b, size_t offset, size_t log_m, const uint64_t *omega, zkhip_bases **out) {
    return bases_lagrange(ctx, b, offset, log_m, omega, false, out);
}

// out[i] = s_i * b[offset + i] (include/zkhip.h): every refusal before any launch, the products into slot 0 of a new object (ecntt.hip), then the
// window tables when the caller asked for them.  d_scalars null: the geometric scalars coeff ratio^(e0 + i).
static int bases_scale(zkhip_ctx *ctx, const zkhip_bases *b, size_t offset, size_t n, const void *d_scalars, const uint64_t *ratio, const uint64_t *coeff,
                       uint64_t e0, int flags, zkhip_bases **out) {
    if (out) *out = nullptr;
    if (!b || !out || (!d_scalars && !ratio)) return ZKHIP_ERR_INVALID;
    ZK_ARGS(ctx, b->curve);
    if (!zk_curve_group_known(b->curve, b->group) || (flags & ~ZKHIP_SCALE_TABLES)) return ZKHIP_ERR_INVALID;
    if (!d_scalars && (!zk_fr_canonical(b->curve, ratio) || (coeff && !zk_fr_canonical(b->curve, coeff)))) return ZKHIP_ERR_INVALID;
    if (n == 0 || n >= ((size_t)1 << 31) || offset > b->n || n > b->n - offset) return ZKHIP_ERR_RANGE;
    if (!d_scalars && (e0 > ((uint64_t)1 << 32) || n > ((uint64_t)1 << 32) - e0)) return ZKHIP_ERR_RANGE;
    ZK_TRY(check_device(ctx));
    std::unique_ptr<zkhip_bases> r;
    ZK_TRY(bases_alloc(ctx, b->curve, b->group, n, r, (flags & ZKHIP_SCALE_TABLES) != 0));
    ZK_TRY(zk_bases_scale(ctx, b, offset, n, (const uint32_t *)d_scalars, ratio, coeff, (uint32_t)e0, r.get()));
    return bases_finish(ctx, r, out);
}

int zkhip_bases_scale_dev(zkhip_ctx *ctx, const zkhip_bases *b, size_t offset, size_t n, const void *d_scalars, int flags, zkhip_bases **out) {
    if (out) *out = nullptr;
    if (!d_scalars) return ZKHIP_ERR_INVALID;
    return bases_scale(ctx, b, offset, n, d_scalars, nullptr, nullptr, 0, flags, out);
}
int zkhip_bases_scale_geometric(zkhip_ctx *ctx, const zkhip_bases *b, size_t offset, size_t n, const uint64_t *ratio, const uint64_t *coeff, uint64_t first_exponent,
                                int flags, zkhip_bases **out) {
    if (out) *out = nullptr;
    if (!ratio) return ZKHIP_ERR_INVALID;
    return bases_scale(ctx, b, offset, n, nullptr, ratio, coeff, first_exponent, flags, out);
}

int zkhip_bases_download(zkhip_ctx *ctx, const zkhip_bases *b, size_t offset, size_t n, uint64_t *affine_xy, uint8_t *is_infinity) {
    if (!ctx || !b || (n && (!affine_xy || !is_infinity))) return ZKHIP_ERR_INVALID;
    if (offset + n > b->n) return ZKHIP_ERR_RANGE;
    if (n == 0) return ZKHIP_OK;
    ZK_TRY(check_device(ctx));
    size_t pbytes = n * 2 * zk_coord_limbs64(b->curve, b->group) * 8;
    DownloadBuffers w = {n, 4 * zk_coord_limbs64(b->curve, b->group)};
    ZK_TRY(ws_place(ctx, w));
    uint32_t *d_out = w.xy;
    uint8_t *d_inf = w.inf;
    ZK_TRY(zk_bases_from_mont(ctx, b, offset, n, d_out, d_inf));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(affine_xy, d_out, pbytes, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(is_infinity, d_inf, n, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ZKHIP_OK;
}

size_t zkhip_bases_size(const zkhip_bases *b) { return b ? b->n : 0; }

void zkhip_bases_free(zkhip_ctx *ctx, zkhip_bases *b) {
    if (!b) return;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    delete b;
}

// ---- MSM ----------------------------------------------------------------------------------------------
int zkhip_msm_dev(zkhip_ctx *ctx, const zkhip_bases *bases, size_t offset, size_t n, const void *d_scalars, void *d_out_jacobian) {
    if (!ctx || !bases || !d_out_jacobian || (n && !d_scalars)) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    return zk_msm_run(ctx, bases, offset, n, (const uint32_t *)d_scalars, (uint32_t *)d_out_jacobian);
}

int zkhip_msm_batch_dev(zkhip_ctx *ctx, size_t count, const zkhip_bases *const *bases, const size_t *offsets, const size_t *ns,
                        const void *const *d_scalars, void *const *d_out_jacobian) {
    if (!ctx || (count && (!bases || !offsets || !ns || !d_scalars || !d_out_jacobian))) return ZKHIP_ERR_INVALID;
    for (size_t i = 0; i < count; ++i)
        if (!bases[i] || !d_out_jacobian[i] || (ns[i] && !d_scalars[i])) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    return zk_msm_run_batch(ctx, count, bases, offsets, ns, (const uint32_t *const *)d_scalars, (uint32_t *const *)d_out_jacobian);
}

}  // extern "C"

// The device buffer zkhip_msm / zkhip_group_msm stage host scalars in: result in the first 512 bytes, scalars behind it.  The context keeps it
// (grow-only, freed with the context): no hipMalloc / hipFree per call (the free is a device synchronisation), and the SAME device addresses
// call after call, so the launch sequence replays as a HIP graph like the resident path's.
int zk_msm_host_reserve(zkhip_ctx *ctx, size_t n) {
    const size_t want = std::max<size_t>(1, n) * 32 + 512;
    if (ctx->msm_host_buf.cap >= want) return 0;
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // on a first allocation too: a graph may still be replaying
    zk_graphs_clear(ctx);                                  // graphs over the old buffer
    return ctx->msm_host_buf.reserve(ctx, want);
}

extern "C" {

int zkhip_msm(zkhip_ctx *ctx, const zkhip_bases *bases, size_t offset, size_t n, const uint64_t *scalars, uint64_t *out_jacobian) {
    if (!ctx || !bases || !out_jacobian || (n && !scalars)) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    const size_t obytes = 3 * zk_coord_limbs64(bases->curve, bases->group) * 8;
    ZK_TRY(zk_msm_host_reserve(ctx, n));
    uint32_t *d_o = ctx->msm_host_buf.as<uint32_t>(), *d_s = d_o + 128;
    if (n) ZK_HIP_CHECK(ctx, hipMemcpyAsync(d_s, scalars, n * 32, hipMemcpyHostToDevice, ctx->stream));
    ZK_TRY(zk_msm_run(ctx, bases, offset, n, d_s, d_o));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(out_jacobian, d_o, obytes, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ZKHIP_OK;
}

int zkhip_jacobian_sum_dev(zkhip_ctx *ctx, int curve, int group, const void *d_points, size_t count, void *d_out_jacobian) {
    if (!ctx || !d_points || !d_out_jacobian) return ZKHIP_ERR_INVALID;
    if (!zk_curve_group_known(curve, group)) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    return zk_jac_sum(ctx, curve, group, (const uint32_t *)d_points, count, (uint32_t *)d_out_jacobian);
}

int zkhip_jacobian_to_affine(zkhip_ctx *ctx, int curve, int group, const uint64_t *jacobian, uint64_t *affine_xy, uint8_t *is_infinity) {
    if (!ctx || !jacobian || !affine_xy || !is_infinity) return ZKHIP_ERR_INVALID;
    if (!zk_curve_group_known(curve, group)) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    size_t cl = zk_coord_limbs64(curve, group) * 8;
    ToAffineBuffers w = {cl / 4};
    ZK_TRY(ws_place(ctx, w));
    uint32_t *d_j = w.jac, *d_a = w.aff;
    uint8_t *d_i = w.inf;
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(d_j, jacobian, 3 * cl, hipMemcpyHostToDevice, ctx->stream));
    ZK_TRY(zk_jac_to_affine(ctx, curve, group, d_j, d_a, d_i));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(affine_xy, d_a, 2 * cl, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(is_infinity, d_i, 1, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ZKHIP_OK;
}

// ---- NTT ----------------------------------------------------------------------------------------------
int zkhip_ntt_dev(zkhip_ctx *ctx, int curve, void *d_data, size_t log_m, size_t batch, const uint64_t *omega, int inverse,
                  const uint64_t *coset_gen) {
    if (!ctx || !omega || (batch && !d_data)) return ZKHIP_ERR_INVALID;
    ZK_TRY(check_device(ctx));
    return zk_ntt_run(ctx, curve, (uint32_t *)d_data, log_m, batch, omega, inverse ? 1 : 0, coset_gen);
}

int zkhip_ntt(zkhip_ctx *ctx, int curve, uint64_t *data, size_t log_m, size_t batch, const uint64_t *omega, int inverse,
              const uint64_t *coset_gen) {
    if (!ctx || !omega || (batch && !data)) return ZKHIP_ERR_INVALID;
    if (log_m > 32) return ZKHIP_ERR_RANGE;
    if (batch == 0) return ZKHIP_OK;
    ZK_TRY(check_device(ctx));
    size_t bytes = (batch << log_m) * 32;
    DevBuf d;
    ZK_TRY(d.alloc(ctx, bytes));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(d, data, bytes, hipMemcpyHostToDevice, ctx->stream));
    ZK_TRY(zk_ntt_run(ctx, curve, d, log_m, batch, omega, inverse ? 1 : 0, coset_gen));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(data, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ZKHIP_OK;
}

// ---- profiling ----------------------------------------------------------------------------------------
int zkhip_profile_enable(zkhip_ctx *ctx, int on) {
    if (!ctx) return ZKHIP_ERR_INVALID;
    ctx->prof_collect();
    ctx->prof.on = on != 0;
    return ZKHIP_OK;
}
int zkhip_profile_filter(zkhip_ctx *ctx, const char *prefix) {
    if (!ctx) return ZKHIP_ERR_INVALID;
    ctx->prof_collect();
    ctx->prof.filter = prefix ? prefix : "";
    return ZKHIP_OK;
}
int zkhip_profile_reset(zkhip_ctx *ctx) {
    if (!ctx) return ZKHIP_ERR_INVALID;
    ctx->prof_collect();
    ctx->prof.acc.clear();
    return ZKHIP_OK;
}
int zkhip_profile_get(zkhip_ctx *ctx, const char *prefix, double *total_ms, uint64_t *launches) {
    if (!ctx || !prefix) return ZKHIP_ERR_INVALID;
    ctx->prof_collect();
    double ms = 0;
    uint64_t cnt = 0;
    size_t pl = strlen(prefix);
    for (auto &kv : ctx->prof.acc) {
        if (kv.first.compare(0, pl, prefix) == 0) {
            ms += kv.second.first;
            cnt += kv.second.second;
        }
    }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = cnt;
    return ZKHIP_OK;
}
size_t zkhip_profile_dump(zkhip_ctx *ctx, char *buf, size_t cap) {
    if (!ctx) return 0;
    ctx->prof_collect();
    std::string s;
    char line[256];
    for (auto &kv : ctx->prof.acc) {
        snprintf(line, sizeof(line), "%s %.6f %llu\n", kv.first.c_str(), kv.second.first, (unsigned long long)kv.second.second);
        s += line;
    }
    if (buf && cap) {
        size_t k = std::min(cap - 1, s.size());
        memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return s.size() + 1;
}

}  // extern "C"
