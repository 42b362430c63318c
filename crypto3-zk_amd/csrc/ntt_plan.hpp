// The host-side geometry of a radix-2 transform (ntt.hip): the radix plan of a size and the shape of one pass's launch -- polynomials per
// workgroup, tile width, bytes of LDS.  Pure functions of integers: ntt_run_t and ntt_get_tables walk them, and the host test-suite walks
// them over every size and option value (csrc/hosttest.hip: zkt_ntt_plan, zkt_ntt_launch).  No HIP here.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "zk_defs.hpp"

static constexpr int NTT_MAX_PASSES = 32;           // log_m <= 32 at radix 2
static constexpr uint32_t NTT_PAD = 0;              // extra elements per LDS row (see ntt.hip: lds_get)
static constexpr size_t NTT_MAX_LDS = 160 * 1024;   // what a workgroup of ntt_pass may ask for (gfx950: 160 KiB per CU)
static constexpr size_t NTT_SHARE_LDS = 80 * 1024;  // polynomials share a workgroup only while a second workgroup still fits on the CU

ZK_HD uint32_t ntt_tile_u4(uint32_t slots) { return 2 * slots + (slots + 3) / 4; }  // uint4 units of one tile's three planes

// LDS of one workgroup of a pass of s stages over pb tiles of 2^log_t columns: the tiles, then the stage twiddles omega_R^q, q < R/2
inline size_t ntt_lds_bytes(uint32_t s, uint32_t log_t, int pb) {
    const size_t nhalf = std::max<size_t>(1, ((size_t)1 << s) / 2);
    const size_t slots = ((size_t)1 << s) * (((size_t)1 << log_t) + NTT_PAD);
    return ((size_t)pb * ntt_tile_u4((uint32_t)slots) + ntt_tile_u4((uint32_t)nhalf)) * 16;
}

// the radix plan: log_m split into np nearly equal radices (larger first), tile widths
struct NttPlan {
    int np;
    int sv[NTT_MAX_PASSES], log_t[NTT_MAX_PASSES];
};
inline NttPlan ntt_plan(size_t log_m, int smax, int tile_log) {
    NttPlan pl;
    pl.np = (int)((log_m + smax - 1) / smax);
    for (int i = 0; i < pl.np; ++i) {
        pl.sv[i] = (int)(log_m / pl.np) + (i < (int)(log_m % pl.np) ? 1 : 0);
        const int log_cols = (int)log_m - pl.sv[i];  // log2(m / R)
        pl.log_t[i] = std::min(std::max(0, tile_log), log_cols);
        while (pl.sv[i] + pl.log_t[i] > 12 && pl.log_t[i] > 0) --pl.log_t[i];  // LDS budget: R * T * 36 B <= 144 KiB
        // ... and the stage twiddles behind the tile: a 10-stage pass brings 18 KiB of them, which a 2^12-element tile leaves no room for
        while (pl.log_t[i] > 0 && ntt_lds_bytes((uint32_t)pl.sv[i], (uint32_t)pl.log_t[i], 1) > NTT_MAX_LDS) --pl.log_t[i];
    }
    return pl;
}

// One launch of a pass over `count` polynomials, `pb` of them wanted per workgroup (1, 2 or 4; option "ntt_pair").  A narrower tile that
// lets the polynomials share a workgroup beats a wider one that does not (measured); what still does not fit
// beside a second workgroup, or a count that pb does not divide, halves pb.
struct NttLaunchShape {
    int pb;
    uint32_t log_t;
    size_t lds;
};
inline NttLaunchShape ntt_launch_shape(uint32_t s, uint32_t log_t, int pb, size_t count) {
    while (pb > 1 && log_t > 2 && ntt_lds_bytes(s, log_t, pb) > NTT_SHARE_LDS) --log_t;
    while (pb > 1 && (ntt_lds_bytes(s, log_t, pb) > NTT_SHARE_LDS || count % pb != 0)) pb >>= 1;
    return {pb, log_t, ntt_lds_bytes(s, log_t, pb)};
}
