// The MSM's entries stage (csrc/msm_entries.hpp: zk_msm_entries_plan, zk_msm_entries, zk_msm_large_plan) by itself: every buffer it leaves is
// compared with a plain host restatement -- digits by msm_fold_scalar / msm_recode, the (set, bucket) histogram and its prefix, the entries of
// every bucket as a sorted list (arrival order inside a bucket is free, nothing else is), the size order as a permutation with non-decreasing
// bins, the large-bucket plan as an exact tiling.  Context, options and bases come through the public ABI; the fifteen buffers are the
// program's own allocations, sized as MsmBuffers::layout (csrc/msm_core.hpp) sizes them.
// Exit code 0 and "ok" on every line = pass.  Device only: run on the GPU box (tests/test_gpu_msm_entries.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "fu.hpp"
#include "msm_entries.hpp"

using namespace zkhip;

namespace {

constexpr uint32_t LARGE_CHUNK = 4096;  // entries per task of a split bucket, restated (msm_entries.hip: MSM_LARGE_CHUNK)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <class T>
struct Dev {  // a device array of `count` elements, prefilled with 0xff bytes so that a word the stage never wrote shows
    T *p = nullptr;
    size_t count;
    explicit Dev(size_t n) : count(std::max<size_t>(n, 1)) {
        if (hipMalloc((void **)&p, count * sizeof(T)) != hipSuccess) p = nullptr;
        else (void)hipMemset(p, 0xff, count * sizeof(T));
    }
    ~Dev() { (void)hipFree(p); }
    std::vector<T> host() const {
        std::vector<T> h(count);
        if (hipMemcpy(h.data(), p, count * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) h.clear();
        return h;
    }
};

struct Case {
    const char *name;
    int curve;
    int window_bits, tile_log, precompute, shard_world, shard_rank;
    size_t bases_n, offset, n;
    enum Scalars { RANDOM, EQUAL_NONZERO_DIGITS, ZERO } scalars;
};

// the digits of the n scalars as msm_digits_only leaves them: window-partitioned runs keep the windows of their rank, as local windows
template <class FR>
void host_digits(const std::vector<uint32_t> &sc, size_t n, const MsmPlan &P, std::vector<uint32_t> &dig) {
    for (size_t i = 0; i < n; ++i) {
        uint32_t s[8];
        const uint32_t flip = msm_fold_scalar<FR>(sc.data() + i * 8, s) ? 0x80000000u : 0u;
        uint32_t carry = 0, next = P.wrank, lw = 0;
        for (int w = 0; w < P.W_all; ++w) {
            const uint32_t d = msm_recode(s, P.win.off(w), P.win.width(w), carry);
            if ((uint32_t)w != next) continue;
            dig[(size_t)lw * n + i] = d == DIG_NONE ? d : d ^ flip;
            next += P.wworld;
            ++lw;
        }
    }
}

#define FAIL(...)                       \
    do {                                \
        printf("%s: ", k.name);         \
        printf(__VA_ARGS__);            \
        printf("\n");                   \
        return 1;                       \
    } while (0)

int run_case(zkhip_ctx *ctx, const Case &k) {
    const std::pair<const char *, int64_t> opts[] = {{"msm_window_bits", k.window_bits}, {"msm_sort_tile_log", k.tile_log}, {"msm_precompute", k.precompute},
                                                     {"msm_shard_world", k.shard_world}, {"msm_shard_rank", k.shard_rank}};
    for (const auto &o : opts)
        if (zkhip_set_option(ctx, o.first, o.second) != ZKHIP_OK) FAIL("option %s refused", o.first);
    std::vector<uint64_t> ks(k.bases_n * 4, 0);
    for (size_t i = 0; i < k.bases_n; ++i) ks[i * 4] = i + 1;
    zkhip_bases *bases = nullptr;
    if (zkhip_bases_from_scalars(ctx, k.curve, ZKHIP_G1, nullptr, ks.data(), k.bases_n, &bases) != ZKHIP_OK) FAIL("bases: %s", zkhip_last_error(ctx));
    struct Free {
        zkhip_ctx *ctx;
        zkhip_bases *b;
        ~Free() { zkhip_bases_free(ctx, b); }
    } free_bases{ctx, bases};
    const size_t n = k.n;

    MsmEntriesCall c;
    std::string error;
    if (zk_msm_entries_plan(ctx, bases, k.offset, n, c, error) != 0) FAIL("plan: %s", error.c_str());
    const MsmPlan &P = c.P;
    const SortGeom &g = c.g;
    const uint32_t nb = P.nb;
    if ((P.tables ? 1 : 0) != k.precompute || g.base_off != k.offset || g.n != n || (size_t)P.W * n != c.entries()) FAIL("the plan is not this case's");

    // scalars: 8 u32 words each; the random ones use all 256 bits (some are not below r: the digits are those of the value mod r)
    std::vector<uint32_t> sc(n * 8, 0);
    if (k.scalars == Case::RANDOM) {
        for (auto &x : sc) x = (uint32_t)rnd();
    } else if (k.scalars == Case::EQUAL_NONZERO_DIGITS) {
        std::vector<uint32_t> one(8), d1((size_t)P.W);
        for (bool found = false; !found;) {
            for (auto &x : one) x = (uint32_t)rnd();
            one[7] >>= 3;  // below every r here
            fr_sat_dispatch(k.curve, [&](auto fr) -> int { return host_digits<typename decltype(fr)::type>(one, 1, P, d1), 0; });
            found = std::none_of(d1.begin(), d1.end(), [](uint32_t d) { return d == DIG_NONE; });
        }
        for (size_t i = 0; i < n; ++i) std::copy(one.begin(), one.end(), sc.begin() + i * 8);
    }
    const size_t E = c.entries();
    std::vector<uint32_t> hdig(E, 0);
    if (fr_sat_dispatch(k.curve, [&](auto fr) -> int { return host_digits<typename decltype(fr)::type>(sc, n, P, hdig), 0; }) != 0) FAIL("unknown curve");

    Dev<uint32_t> d_sc(n * 8), dig(E), bh(c.nbh), bo((size_t)c.nbh + 1), bsums((c.nbh + 1023) / 1024), tmp_idx(E), offs((size_t)nb + 1), idx(E), sh((size_t)c.nsh + 1),
        so((size_t)c.nsh + 1), ssums((c.nsh + 1023) / 1024), order(nb), plan(4), tasks((size_t)c.task_cap * 3), large((size_t)c.large_cap * 3);
    Dev<uint16_t> tmp_key(E);
    for (const void *p : {(void *)d_sc.p, (void *)dig.p, (void *)bh.p, (void *)bo.p, (void *)bsums.p, (void *)tmp_idx.p, (void *)offs.p, (void *)idx.p, (void *)sh.p,
                          (void *)so.p, (void *)ssums.p, (void *)order.p, (void *)plan.p, (void *)tasks.p, (void *)large.p, (void *)tmp_key.p})
        if (!p) FAIL("hipMalloc failed");
    if (hipMemcpy(d_sc.p, sc.data(), n * 32, hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) FAIL("upload failed");
    MsmEntriesBuffers w;
    w.dig = dig.p, w.bh = bh.p, w.bo = bo.p, w.bsums = bsums.p, w.tmp_idx = tmp_idx.p, w.tmp_key = tmp_key.p, w.offs = offs.p, w.idx = idx.p;
    w.sh = sh.p, w.so = so.p, w.ssums = ssums.p, w.order = order.p, w.plan = plan.p, w.tasks = tasks.p, w.large = large.p;
    if (zk_msm_entries(ctx, k.curve, c, w, d_sc.p) != 0) FAIL("zk_msm_entries: %s", zkhip_last_error(ctx));
    if (zk_msm_large_plan(ctx, c, w) != 0) FAIL("zk_msm_large_plan: %s", zkhip_last_error(ctx));
    uint32_t flags = 0;
    const int status = zkhip_device_status(ctx, &flags);  // synchronises the stream
    if (status != ZKHIP_OK || (flags & ZK_STATUS_MSM_PLAN_OVERFLOW)) FAIL("device status %d, flags 0x%x", status, flags);
    const std::vector<uint32_t> ddig = dig.host(), doffs = offs.host(), didx_raw = idx.host(), dorder = order.host(), dplan = plan.host(), dtasks = tasks.host(),
                                dlarge = large.host();
    if (ddig.empty() || doffs.empty() || didx_raw.empty() || dorder.empty() || dplan.empty() || dtasks.empty() || dlarge.empty()) FAIL("download failed");

    // dig
    for (size_t e = 0; e < E; ++e)
        if (ddig[e] != hdig[e]) FAIL("dig[%zu] (window %zu, point %zu) = 0x%x, host 0x%x", e, e / n, e % n, ddig[e], hdig[e]);
    // offs: the exclusive prefix of the (set, bucket) histogram; offs[nb] = the number of non-zero digits
    std::vector<uint32_t> hoffs((size_t)nb + 1, 0);
    auto key_of = [&](size_t lw, uint32_t d) { return (uint32_t)(lw % P.S) * P.B + (d & 0x7FFFFFFFu); };
    for (size_t e = 0; e < E; ++e)
        if (hdig[e] != DIG_NONE) ++hoffs[key_of(e / n, hdig[e]) + 1];
    for (uint32_t b = 0; b < nb; ++b) hoffs[b + 1] += hoffs[b];
    for (uint32_t b = 0; b <= nb; ++b)
        if (doffs[b] != hoffs[b]) FAIL("offs[%u] = %u, host %u", b, doffs[b], hoffs[b]);
    const uint32_t total = hoffs[nb];
    // idx: bucket by bucket as a sorted list
    std::vector<uint32_t> hidx(total), cursor(hoffs.begin(), hoffs.end() - 1), didx(didx_raw.begin(), didx_raw.begin() + total);
    for (size_t e = 0; e < E; ++e) {
        const uint32_t d = hdig[e];
        if (d == DIG_NONE) continue;
        const size_t lw = e / n, i = e % n;
        hidx[cursor[key_of(lw, d)]++] = (uint32_t)((P.tables ? (g.slot0 + lw) * g.bases_n : 0) + k.offset + i) | (d & 0x80000000u);
    }
    for (uint32_t b = 0; b < nb; ++b) {
        std::sort(hidx.begin() + hoffs[b], hidx.begin() + hoffs[b + 1]);
        std::sort(didx.begin() + hoffs[b], didx.begin() + hoffs[b + 1]);
    }
    for (uint32_t b = 0; b < nb; ++b)
        for (uint32_t e = hoffs[b]; e < hoffs[b + 1]; ++e)
            if (didx[e] != hidx[e]) FAIL("bucket %u: sorted entry %u = 0x%x, host 0x%x", b, e - hoffs[b], didx[e], hidx[e]);
    // order: a permutation of the buckets, bins never decreasing
    std::vector<uint8_t> seen(nb, 0);
    uint32_t last_bin = 0;
    for (uint32_t j = 0; j < nb; ++j) {
        const uint32_t b = dorder[j];
        if (b >= nb || seen[b]) FAIL("order[%u] = %u is out of range or repeated", j, b);
        seen[b] = 1;
        const uint32_t bin = zk_msm_size_bin(hoffs[b + 1] - hoffs[b], c.large_thresh);
        if (bin < last_bin) FAIL("order[%u] = %u: bin %u after bin %u", j, b, bin, last_bin);
        last_bin = bin;
    }
    // plan, tasks, large: every bucket above the threshold once, its tasks tiling its entries in chunks; nothing else
    uint32_t want_large = 0, want_tasks = 0;
    for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t size = hoffs[b + 1] - hoffs[b];
        if (size > c.large_thresh) ++want_large, want_tasks += (size + LARGE_CHUNK - 1) / LARGE_CHUNK;
    }
    if (dplan[0] != want_tasks || dplan[1] != want_large) FAIL("plan = {%u tasks, %u large}, host {%u, %u}", dplan[0], dplan[1], want_tasks, want_large);
    if (want_tasks > c.task_cap || want_large > c.large_cap) FAIL("the plan's capacities (%u, %u) are below the plan", c.task_cap, c.large_cap);
    std::fill(seen.begin(), seen.end(), 0);
    std::vector<uint8_t> task_used(want_tasks, 0);
    for (uint32_t j = 0; j < want_large; ++j) {
        const uint32_t b = dlarge[3 * j], first = dlarge[3 * j + 1], nt = dlarge[3 * j + 2];
        if (b >= nb || seen[b] || hoffs[b + 1] - hoffs[b] <= c.large_thresh) FAIL("large[%u]: bucket %u is out of range, repeated or not large", j, b);
        seen[b] = 1;
        if (nt != (hoffs[b + 1] - hoffs[b] + LARGE_CHUNK - 1) / LARGE_CHUNK || first > want_tasks || nt > want_tasks - first)
            FAIL("large[%u]: bucket %u of %u entries has tasks %u + %u of %u", j, b, hoffs[b + 1] - hoffs[b], first, nt, want_tasks);
        for (uint32_t t = 0; t < nt; ++t) {
            const uint32_t *task = &dtasks[3 * (size_t)(first + t)];
            const uint32_t lo = hoffs[b] + t * LARGE_CHUNK, hi = std::min(hoffs[b + 1], lo + LARGE_CHUNK);
            if (task_used[first + t]++) FAIL("task %u belongs to two buckets", first + t);
            if (task[0] != b || task[1] != lo || task[2] != hi) FAIL("task %u = {%u, %u, %u}, host {%u, %u, %u}", first + t, task[0], task[1], task[2], b, lo, hi);
        }
    }
    printf("%s: ok (%d windows of %d, %u sets x %u buckets, %u super-buckets, %u tiles, %u entries, %u large buckets in %u tasks)\n", k.name, P.W, P.W_all, P.S, P.B,
           g.nsuper, g.ntile, total, want_large, want_tasks);
    return 0;
}

}  // namespace

int main() {
    zkhip_ctx *ctx = nullptr;
    if (zkhip_init(0, &ctx) != ZKHIP_OK) {
        printf("no device\n");
        return 1;
    }
    const int BLS = ZKHIP_BLS12_381;
    const Case cases[] = {
        // name, curve, window bits, tile log, tables, shard world / rank, points of the bases object, offset, n, scalars
        {"a: c = 21, small tiles: three-launch scans, 1024 super-buckets, a last tile of one entry", BLS, 21, 12, 1, 1, 0, 20481, 0, 20481, Case::RANDOM},
        {"b: c = 21, big tiles: two tiles, the raised LDS limit", BLS, 21, 14, 1, 1, 0, 20481, 0, 20481, Case::RANDOM},
        {"c: c = 8, equal scalars: three tasks per large bucket in every window", BLS, 8, 14, 1, 1, 0, 8193, 0, 8193, Case::EQUAL_NONZERO_DIGITS},
        {"d: c = 8, zero scalars: no entry at all", BLS, 8, 14, 1, 1, 0, 8193, 0, 8193, Case::ZERO},
        {"e: no tables, 31 points from offset 7", BLS, 21, 14, 0, 1, 0, 64, 7, 31, Case::RANDOM},
        {"e: no tables, 1 point from offset 63", BLS, 21, 14, 0, 1, 0, 64, 63, 1, Case::RANDOM},
        {"f: window partition, rank 1 of 2", BLS, 0, 14, 1, 2, 1, 4097, 0, 4097, Case::RANDOM},
        {"g: BN254 (254-bit r)", ZKHIP_BN254, 0, 14, 1, 1, 0, 4097, 0, 4097, Case::RANDOM},
        {"g: Pallas", ZKHIP_PALLAS, 0, 14, 1, 1, 0, 4097, 0, 4097, Case::RANDOM},
        {"g: Vesta, window partition, rank 1 of 2", ZKHIP_VESTA, 0, 12, 1, 2, 1, 4097, 0, 4097, Case::RANDOM},
    };
    int bad = 0;
    for (const Case &k : cases) bad |= run_case(ctx, k);
    zkhip_destroy(ctx);
    return bad;
}
