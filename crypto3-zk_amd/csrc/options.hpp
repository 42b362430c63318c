// The context's integer options, each named ONCE: zkhip_set_option, zkhip_get_option, the ZKHIP_OPTIONS variable and the key of the MSM
// graph cache (msm.hip: key_begin) all walk this table.  A row is the option's name, the `int` member of the context that holds it,
// how a value is admitted, and whether the option shapes an MSM's launch sequence -- such an option is part of the graph key, so a
// captured graph is never replayed under another setting.  The members keep their defaults and comments where they are declared.
// No HIP here, and the context is a template parameter: the host test-suite walks the table over a plain struct.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

enum OptAdmit {
    OPT_INT,     // truncated to int
    OPT_FLAG,    // stored as value != 0
    OPT_LANES,   // clamped to [0, 2^24]
    OPT_CUSTOM,  // zkhip_set_option admits it by hand: a range that depends on another option, or a side effect
};

template <class Ctx>
struct OptRow {
    const char *name;
    int Ctx::*member;  // null: the option is not held in an int (alloc_cache_mb: a byte count)
    OptAdmit admit;
    bool msm_graph_key;
};

template <class Ctx>
constexpr OptRow<Ctx> zk_options[] = {
    {"msm_window_bits", &Ctx::opt_msm_window_bits, OPT_INT, true},
    {"msm_segment_log", &Ctx::opt_msm_segment_log, OPT_INT, true},
    {"msm_sets", &Ctx::opt_msm_sets, OPT_INT, true},
    {"msm_tail_quads", &Ctx::opt_msm_tail_quads, OPT_INT, true},
    {"msm_tail_fold", &Ctx::opt_msm_tail_fold, OPT_INT, true},
    {"msm_fold_run", &Ctx::opt_msm_fold_run, OPT_INT, true},
    {"msm_tail_fold_g2", &Ctx::opt_msm_tail_fold_g2, OPT_INT, true},
    {"msm_share_sort", &Ctx::opt_msm_share_sort, OPT_INT, true},
    {"msm_sort_tile_log", &Ctx::opt_msm_sort_tile_log, OPT_INT, true},  // the captured launch sequence depends on the sort's tile shape
    {"ec_ntt_table_lanes", &Ctx::opt_ec_ntt_table_lanes, OPT_LANES, false},
    {"ntt_radix_log", &Ctx::opt_ntt_radix_log, OPT_INT, false},
    {"ntt_tile_log", &Ctx::opt_ntt_tile_log, OPT_INT, false},
    {"ntt_pair", &Ctx::opt_ntt_pair, OPT_INT, false},
    {"poly_coset_extend", &Ctx::opt_poly_coset_extend, OPT_FLAG, false},
    {"msm_precompute", &Ctx::opt_msm_precompute, OPT_INT, false},
    {"msm_precompute_min", &Ctx::opt_msm_precompute_min, OPT_INT, false},
    {"msm_graphs", &Ctx::opt_msm_graphs, OPT_INT, false},
    {"msm_shard_world", &Ctx::opt_msm_shard_world, OPT_CUSTOM, false},
    {"msm_shard_rank", &Ctx::opt_msm_shard_rank, OPT_CUSTOM, false},
    {"stream_priority", &Ctx::opt_stream_priority, OPT_CUSTOM, false},
    {"alloc_cache_mb", nullptr, OPT_CUSTOM, false},
};

template <class Ctx>
const OptRow<Ctx> *zk_option_find(const char *name) {
    for (const OptRow<Ctx> &r : zk_options<Ctx>)
        if (strcmp(r.name, name) == 0) return &r;
    return nullptr;
}

// store `value` as the row admits it (not for OPT_CUSTOM rows)
template <class Ctx>
void zk_option_store(Ctx &c, const OptRow<Ctx> &r, int64_t value) {
    if (r.admit == OPT_FLAG) c.*r.member = value != 0;
    else if (r.admit == OPT_LANES) c.*r.member = (int)std::min<int64_t>(std::max<int64_t>(value, 0), 1 << 24);
    else c.*r.member = (int)value;
}

// "name=value,name=value" (the ZKHIP_OPTIONS variable): set(name, value) for every entry with a name and an '='; the rest is skipped
template <class Set>
void zk_options_parse(const char *text, Set set) {
    const std::string all(text);
    size_t at = 0;
    while (at < all.size()) {
        const size_t end = all.find(',', at);
        const std::string item = all.substr(at, end == std::string::npos ? std::string::npos : end - at);
        const size_t eq = item.find('=');
        if (eq != std::string::npos && eq > 0) set(item.substr(0, eq).c_str(), (int64_t)atoll(item.c_str() + eq + 1));
        if (end == std::string::npos) break;
        at = end + 1;
    }
}
