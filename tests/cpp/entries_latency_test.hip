// More cases of the MSM's entries stage (csrc/msm_entries.hpp), checked by entriestest.hip's own run_case -- its host restatement of dig, offs,
// idx, order and the large-bucket plan is compiled into this program, not restated a second time: wave, workgroup and tile boundaries of the
// three sort tile shapes, the two-launch scan beyond one strip, the large-bucket plan written by the size sort's last kernel, geometries whose
// super-buckets are narrower than 1024 buckets, and two runs of one input side by side.
// Exit code 0 and "ok" on every line = pass.  Device only: run on the GPU box (tests/test_gpu_msm_entries_latency.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "fu.hpp"
#include "msm_entries.hpp"

#define main entriestest_main
#include "entriestest.hip"
#undef main

namespace {

// The stage twice over one input, into two sets of buffers: what does not depend on arrival order -- offs, order, plan[0 .. 1] -- must agree word for word.
int run_twice(zkhip_ctx *ctx, const Case &k) {
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
    const uint32_t nb = c.P.nb;
    const size_t E = c.entries();
    std::vector<uint32_t> sc(n * 8, 0);
    if (k.scalars == Case::RANDOM) {
        for (auto &x : sc) x = (uint32_t)rnd();
    } else if (k.scalars == Case::EQUAL_NONZERO_DIGITS) {
        for (size_t i = 0; i < n; ++i)
            for (int j = 0; j < 8; ++j) sc[i * 8 + j] = 0x12345678u >> (j == 7 ? 4 : 0);  // one value below every r here; some digits may be zero
    }
    Dev<uint32_t> d_sc(n * 8);
    if (!d_sc.p || hipMemcpy(d_sc.p, sc.data(), n * 32, hipMemcpyHostToDevice) != hipSuccess) FAIL("upload failed");
    std::vector<uint32_t> offs[2], order[2], plan[2];
    for (int run = 0; run < 2; ++run) {
        Dev<uint32_t> dig(E), bh(c.nbh), bo((size_t)c.nbh + 1), bsums((c.nbh + 1023) / 1024), tmp_idx(E), d_offs((size_t)nb + 1), idx(E), sh((size_t)c.nsh + 1),
            so((size_t)c.nsh + 1), ssums((c.nsh + 1023) / 1024), d_order(nb), d_plan(4), tasks((size_t)c.task_cap * 3), large((size_t)c.large_cap * 3);
        Dev<uint16_t> tmp_key(E);
        for (const void *p : {(void *)dig.p, (void *)bh.p, (void *)bo.p, (void *)bsums.p, (void *)tmp_idx.p, (void *)d_offs.p, (void *)idx.p, (void *)sh.p, (void *)so.p,
                              (void *)ssums.p, (void *)d_order.p, (void *)d_plan.p, (void *)tasks.p, (void *)large.p, (void *)tmp_key.p})
            if (!p) FAIL("hipMalloc failed");
        if (hipDeviceSynchronize() != hipSuccess) FAIL("fill failed");
        MsmEntriesBuffers w;
        w.dig = dig.p, w.bh = bh.p, w.bo = bo.p, w.bsums = bsums.p, w.tmp_idx = tmp_idx.p, w.tmp_key = tmp_key.p, w.offs = d_offs.p, w.idx = idx.p;
        w.sh = sh.p, w.so = so.p, w.ssums = ssums.p, w.order = d_order.p, w.plan = d_plan.p, w.tasks = tasks.p, w.large = large.p;
        if (zk_msm_entries(ctx, k.curve, c, w, d_sc.p) != 0) FAIL("zk_msm_entries: %s", zkhip_last_error(ctx));
        if (zk_msm_large_plan(ctx, c, w) != 0) FAIL("zk_msm_large_plan: %s", zkhip_last_error(ctx));
        uint32_t flags = 0;
        const int status = zkhip_device_status(ctx, &flags);  // synchronises the stream
        if (status != ZKHIP_OK || flags) FAIL("device status %d, flags 0x%x", status, flags);
        offs[run] = d_offs.host(), order[run] = d_order.host(), plan[run] = d_plan.host();
        if (offs[run].empty() || order[run].empty() || plan[run].empty()) FAIL("download failed");
    }
    for (uint32_t b = 0; b <= nb; ++b)
        if (offs[0][b] != offs[1][b]) FAIL("offs[%u] = %u, then %u", b, offs[0][b], offs[1][b]);
    for (uint32_t j = 0; j < nb; ++j)
        if (order[0][j] != order[1][j]) FAIL("order[%u] = %u, then %u", j, order[0][j], order[1][j]);
    for (int j = 0; j < 2; ++j)
        if (plan[0][j] != plan[1][j]) FAIL("plan[%d] = %u, then %u", j, plan[0][j], plan[1][j]);
    printf("%s: ok (%u buckets, %u entries, %u tasks, %u large buckets, twice)\n", k.name, nb, offs[0][nb], plan[0][0], plan[0][1]);
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
    int bad = 0;
    // wave, workgroup and tile boundaries of the three tile shapes; c = 11: super-buckets of 1024 buckets, the final pass counts the size histogram
    std::vector<std::string> names;
    names.reserve(64);
    for (int tile_log : {12, 13, 14})
        for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)1023, (size_t)1025, (size_t)8191, (size_t)8193, (size_t)16385}) {
            names.push_back("sizes: n = " + std::to_string(n) + ", tile log " + std::to_string(tile_log));
            bad |= run_case(ctx, Case{names.back().c_str(), BLS, 11, tile_log, 1, 1, 0, std::max<size_t>(n, 64), 0, n, Case::RANDOM});  // (one point has no tables)
        }
    const Case more[] = {
        // name, curve, window bits, tile log, tables, shard world / rank, points of the bases object, offset, n, scalars
        {"scan: 512 x 13 x 11 = 73216 sort counters and 130 x 512 = 66560 size counters, both beyond one launch", BLS, 20, 12, 1, 1, 0, 45056, 0, 45056, Case::RANDOM},
        {"plan: c = 11, equal scalars, the final pass counts the sizes", BLS, 11, 13, 1, 1, 0, 9000, 0, 9000, Case::EQUAL_NONZERO_DIGITS},
        {"plan: c = 11, zero scalars", BLS, 11, 13, 1, 1, 0, 9000, 0, 9000, Case::ZERO},
        {"plan: c = 20, equal scalars, two-launch scans", BLS, 20, 14, 1, 1, 0, 9000, 0, 9000, Case::EQUAL_NONZERO_DIGITS},
        {"plan: c = 8, equal scalars, msm_size_hist counts the sizes", BLS, 8, 13, 1, 1, 0, 9000, 0, 9000, Case::EQUAL_NONZERO_DIGITS},
        {"narrow: c = 8 (128-bucket super-buckets), tile log 12", BLS, 8, 12, 1, 1, 0, 5000, 0, 5000, Case::RANDOM},
        {"narrow: c = 8, tile log 13", BLS, 8, 13, 1, 1, 0, 5000, 0, 5000, Case::RANDOM},
        {"narrow: c = 5 (16-bucket super-buckets), tile log 14", BLS, 5, 14, 1, 1, 0, 5000, 0, 5000, Case::RANDOM},
        {"narrow: c = 10 (512-bucket super-buckets), no tables", BLS, 10, 13, 0, 1, 0, 5000, 0, 5000, Case::RANDOM},
    };
    for (const Case &k : more) bad |= run_case(ctx, k);
    const Case twice[] = {
        {"twice: c = 11, random scalars, tile log 13", BLS, 11, 13, 1, 1, 0, 16385, 0, 16385, Case::RANDOM},
        {"twice: c = 20, random scalars, tile log 14", BLS, 20, 14, 1, 1, 0, 16385, 0, 16385, Case::RANDOM},
        {"twice: c = 8, equal scalars, tile log 12", BLS, 8, 12, 1, 1, 0, 9000, 0, 9000, Case::EQUAL_NONZERO_DIGITS},
    };
    for (const Case &k : twice) bad |= run_twice(ctx, k);
    zkhip_destroy(ctx);
    return bad;
}
