// SHA2-256 Merkle trees of the LPC / FRI commitments, built on the device (the hashing side of precommit<FRI>,
// zk/commitments/detail/polynomial/basic_fri.hpp:375-409, 461-496: make_merkle_tree<Hash, 2> over the coset-ordered leaves).
//
//   zkhip_merkle_build_fri_dev   the tree straight from the resident evaluations: one lane per leaf gathers the leaf's elements with
//                                fri_leaf_gather's index arithmetic (poly.hip) and hashes them as it goes -- the leaf layout is never written
//   zkhip_merkle_build_dev       the tree over a leaf layout that already lies on the device
//   zkhip_merkle_root / _digests / _paths   what a transcript and a query phase read
//   zkhip_fri_query_dev / zkhip_merkle_paths_multi   the FRI query phase's answers (basic_fri.hpp:747-930): the evaluation pairs calculate_s walks
//                                from every query index over several sets of resident polynomials, and the paths of every query in several
//                                trees -- each one launch and one copy to the host
//
// Conventions: include/zkhip.h ("Merkle trees") and sha256.hpp.  The tree is one array of (2L - 1) digests of 32 bytes in their external
// byte order: the L leaf digests, then every level above, the root last; level l starts at digest 2L - (2L >> l).
#include <algorithm>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "sha256.hpp"

using namespace zkhip;

struct zkhip_merkle {
    int hash = 0;
    size_t leaves = 0, depth = 0;
    uint32_t *d = nullptr;  // (2 leaves - 1) x 8 words
};

static __host__ __device__ inline size_t merkle_level_offset(size_t leaves, size_t level) { return 2 * leaves - ((2 * leaves) >> level); }

// One lane per leaf x < D / 2^step.  The leaf is, for every polynomial in turn, the pairs (f[s_i], f[s_i + D/2]), i < 2^step / 2, with
// s_0 = x and s_(2^l + j) = s_j + D / (4 * 2^l) mod D (fri_leaf_gather): every pair is one 64-byte compression block, and neighbouring lanes
// read neighbouring 32-byte elements.
__global__ __launch_bounds__(256) void merkle_fri_leaf_hash(const uint4 *__restrict__ polys, uint32_t log_d, uint32_t batch, uint32_t step, size_t n_leaves,
                                                            uint32_t *__restrict__ digests) {
    const size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_leaves) return;
    const uint32_t half_log = step - 1, half = 1u << half_log;
    const size_t D = (size_t)1 << log_d;
    uint32_t h[8], w[16];
    sha256::init(h);
    for (uint32_t p = 0; p < batch; ++p) {
        const uint4 *f = polys + 2 * ((size_t)p << log_d);
        for (uint32_t i = 0; i < half; ++i) {
            size_t s = x;
            for (uint32_t l = 0; l < half_log; ++l)
                if ((i >> l) & 1) s += D >> (2 + l);
            s &= D - 1;
            const size_t s2 = (s + (D >> 1)) & (D - 1);
            sha256::element_words(f + 2 * s, w);
            sha256::element_words(f + 2 * s2, w + 8);
            sha256::compress(h, w);
        }
    }
    sha256::pad_words(w, 0, ((uint64_t)batch << step) * 32);
    sha256::compress(h, w);
    sha256::store_digest(digests + 8 * x, h);
}

// one lane per leaf of a materialised layout: n_leaves x per_leaf elements
__global__ __launch_bounds__(256) void merkle_leaf_hash(const uint4 *__restrict__ leaves, size_t per_leaf, size_t n_leaves, uint32_t *__restrict__ digests) {
    const size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_leaves) return;
    sha256::hash_elements(leaves + 2 * x * per_leaf, per_leaf, digests + 8 * x);
}

// one lane per parent: parents[j] = H(children[2j] || children[2j + 1])
__global__ __launch_bounds__(256) void merkle_level_hash(const uint32_t *__restrict__ children, size_t n_parents, uint32_t *__restrict__ parents) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_parents) return;
    sha256::hash_node(children + 16 * j, children + 16 * j + 8, parents + 8 * j);
}

// one lane per 16 bytes of the output: out[(k * depth + l)] = the sibling of leaf indices[k]'s ancestor on level l
__global__ __launch_bounds__(256) void merkle_path_gather(const uint4 *__restrict__ tree, size_t leaves, uint32_t depth, const uint64_t *__restrict__ indices,
                                                          size_t total, uint4 *__restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // ((k * depth + l) * 2 + half)
    if (t >= total) return;
    const size_t node = t >> 1, k = node / depth, l = node % depth;
    const size_t sibling = (indices[k] >> l) ^ 1;
    out[t] = tree[2 * (merkle_level_offset(leaves, l) + sibling) + (t & 1)];
}

// zkhip_fri_query_dev: one set of resident evaluations as the gather sees it; `end` closes the set's range of output elements
struct FriQuerySet {
    const uint4 *polys;
    uint32_t log_d, batch, step;
    size_t end;
};

// One lane per 16 bytes of the output (neighbouring lanes write neighbouring halves of an element).  Element e of set t is
// [q][p][i][side]: with x = indices[q] mod D, s_0 = x and s_(2^l + j) = s_j + D / (4 * 2^l) mod D as in merkle_fri_leaf_hash, the pair i is
// (f[min(s_i, s_i + D/2 mod D)], f[max(...)]) (calculate_s and the ind0 / ind1 rule, basic_fri.hpp:585-614, 815-818).
__global__ __launch_bounds__(256) void fri_query_gather(const FriQuerySet *__restrict__ sets, uint32_t n_sets, const uint64_t *__restrict__ indices, size_t total,
                                                        uint4 *__restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t e = t >> 1;
    uint32_t u = 0;
    while (u + 1 < n_sets && e >= sets[u].end) ++u;
    const FriQuerySet set = sets[u];
    const size_t local = e - (u ? sets[u - 1].end : 0), per_query = (size_t)set.batch << set.step;
    const size_t q = local / per_query, rem = local % per_query;
    const size_t p = rem >> set.step, i = (rem & (((size_t)1 << set.step) - 1)) >> 1, side = rem & 1;
    const size_t D = (size_t)1 << set.log_d;
    size_t s = (size_t)indices[q] & (D - 1);
    for (uint32_t l = 0; l + 1 < set.step; ++l)
        if ((i >> l) & 1) s += D >> (2 + l);
    s &= D - 1;
    const size_t s2 = (s + (D >> 1)) & (D - 1);
    const size_t src = side ? max(s, s2) : min(s, s2);
    out[t] = set.polys[2 * ((p << set.log_d) + src) + (t & 1)];
}

// zkhip_merkle_paths_multi: one tree as the gather sees it; `end` closes the tree's range of output digests
struct PathTree {
    const uint4 *d;
    size_t leaves, depth, end;
};

// one lane per 16 bytes of the output: digest (k * depth + l) of tree t is the sibling of leaf (indices[k] mod leaves)'s ancestor on level l
__global__ __launch_bounds__(256) void merkle_path_gather_multi(const PathTree *__restrict__ trees, uint32_t n_trees, const uint64_t *__restrict__ indices,
                                                                size_t total, uint4 *__restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t node = t >> 1;
    uint32_t u = 0;
    while (u + 1 < n_trees && node >= trees[u].end) ++u;  // a one-leaf tree has an empty range and is stepped over
    const PathTree tree = trees[u];
    const size_t local = node - (u ? trees[u - 1].end : 0), k = local / tree.depth, l = local % tree.depth;
    const size_t sibling = (((size_t)indices[k] & (tree.leaves - 1)) >> l) ^ 1;
    out[t] = tree.d[2 * (merkle_level_offset(tree.leaves, l) + sibling) + (t & 1)];
}

// the levels above the leaf digests, bottom up
static int merkle_levels(zkhip_ctx *ctx, zkhip_merkle *t) {
    for (size_t l = 1; l <= t->depth; ++l) {
        const size_t n = t->leaves >> l;
        ZK_LAUNCH(ctx, "merkle_level_hash", merkle_level_hash, grid_1d(n), dim3(256), 0,
                  t->d + 8 * merkle_level_offset(t->leaves, l - 1), n, t->d + 8 * merkle_level_offset(t->leaves, l));
    }
    return ZKHIP_OK;
}

static int merkle_alloc(zkhip_ctx *ctx, int hash, size_t leaves, zkhip_merkle **out) {
    zkhip_merkle *t = new (std::nothrow) zkhip_merkle;
    if (!t) return ZKHIP_ERR_OOM;
    t->hash = hash;
    t->leaves = leaves;
    while (((size_t)1 << t->depth) < leaves) ++t->depth;
    void *d = nullptr;
    const int rc = zkhip_malloc(ctx, (2 * leaves - 1) * 32, &d);
    if (rc != ZKHIP_OK) {
        delete t;
        return rc;
    }
    t->d = static_cast<uint32_t *>(d);
    *out = t;
    return ZKHIP_OK;
}

// a build's last step: the tree to the caller, or back to the allocator when a launch failed
static int merkle_done(zkhip_ctx *ctx, zkhip_merkle *t, int rc, zkhip_merkle **out) {
    if (rc != ZKHIP_OK) {
        zkhip_merkle_free(ctx, t);
        return rc;
    }
    *out = t;
    return ZKHIP_OK;
}

static int merkle_hash_leaves(zkhip_ctx *ctx, zkhip_merkle *t, const void *d_leaves, size_t per_leaf) {
    ZK_LAUNCH(ctx, "merkle_leaf_hash", merkle_leaf_hash, grid_1d(t->leaves), dim3(256), 0, (const uint4 *)d_leaves, per_leaf, t->leaves,
              t->d);
    return merkle_levels(ctx, t);
}

static int merkle_hash_fri_leaves(zkhip_ctx *ctx, zkhip_merkle *t, const void *d_polys, size_t log_domain, size_t batch, size_t fri_step) {
    ZK_LAUNCH(ctx, "merkle_fri_leaf_hash", merkle_fri_leaf_hash, grid_1d(t->leaves), dim3(256), 0, (const uint4 *)d_polys,
              (uint32_t)log_domain, (uint32_t)batch, (uint32_t)fri_step, t->leaves, t->d);
    return merkle_levels(ctx, t);
}

struct PathBuffers {  // zkhip_merkle_paths: the leaf indices and the gathered digests (two uint4 each)
    size_t count, nodes;
    uint64_t *idx;
    uint4 *out;
    template <class Arena>
    void layout(Arena &a) {
        a.take(idx, count);
        a.take(out, nodes * 2);
    }
};

struct QueryBuffers {  // zkhip_fri_query_dev: the set table, the query indices and the gathered elements (two uint4 each)
    size_t n_sets, count, elements;
    FriQuerySet *sets;
    uint64_t *idx;
    uint4 *out;
    template <class Arena>
    void layout(Arena &a) {
        a.take(sets, n_sets);
        a.take(idx, count);
        a.take(out, elements * 2);
    }
};

struct MultiPathBuffers {  // zkhip_merkle_paths_multi: the tree table, the query indices and the gathered digests (two uint4 each)
    size_t n_trees, count, nodes;
    PathTree *trees;
    uint64_t *idx;
    uint4 *out;
    template <class Arena>
    void layout(Arena &a) {
        a.take(trees, n_trees);
        a.take(idx, count);
        a.take(out, nodes * 2);
    }
};

extern "C" {

int zkhip_merkle_build_dev(zkhip_ctx *ctx, int hash, const void *d_leaves, size_t n_leaves, size_t elements_per_leaf, zkhip_merkle **out) {
    if (!ctx || !out || !d_leaves || hash != ZKHIP_HASH_SHA2_256) return ZKHIP_ERR_INVALID;
    if (n_leaves == 0 || (n_leaves & (n_leaves - 1)) || elements_per_leaf == 0) return ZKHIP_ERR_INVALID;
    if (n_leaves > ((size_t)1 << 32) || elements_per_leaf >= ((size_t)1 << 32)) return ZKHIP_ERR_RANGE;
    ZK_ENTER(ctx);
    zkhip_merkle *t = nullptr;
    ZK_TRY(merkle_alloc(ctx, hash, n_leaves, &t));
    return merkle_done(ctx, t, merkle_hash_leaves(ctx, t, d_leaves, elements_per_leaf), out);
}

int zkhip_merkle_build_fri_dev(zkhip_ctx *ctx, int hash, const void *d_polys, size_t log_domain, size_t batch, size_t fri_step, zkhip_merkle **out) {
    if (!ctx || !out || !d_polys || hash != ZKHIP_HASH_SHA2_256 || batch == 0) return ZKHIP_ERR_INVALID;
    if (fri_step < 1 || fri_step > log_domain || log_domain > 32 || batch >= ((size_t)1 << 31)) return ZKHIP_ERR_RANGE;
    ZK_ENTER(ctx);
    zkhip_merkle *t = nullptr;
    ZK_TRY(merkle_alloc(ctx, hash, (size_t)1 << (log_domain - fri_step), &t));
    return merkle_done(ctx, t, merkle_hash_fri_leaves(ctx, t, d_polys, log_domain, batch, fri_step), out);
}

size_t zkhip_merkle_leaves(const zkhip_merkle *t) { return t ? t->leaves : 0; }
size_t zkhip_merkle_depth(const zkhip_merkle *t) { return t ? t->depth : 0; }

int zkhip_merkle_digests(zkhip_ctx *ctx, const zkhip_merkle *t, uint8_t *out) {
    if (!ctx || !t || !out) return ZKHIP_ERR_INVALID;
    ZK_ENTER(ctx);
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(out, t->d, (2 * t->leaves - 1) * 32, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ZKHIP_OK;
}

int zkhip_merkle_root(zkhip_ctx *ctx, const zkhip_merkle *t, uint8_t out[32]) {
    if (!ctx || !t || !out) return ZKHIP_ERR_INVALID;
    ZK_ENTER(ctx);
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(out, t->d + 8 * (2 * t->leaves - 2), 32, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ZKHIP_OK;
}

int zkhip_merkle_paths(zkhip_ctx *ctx, const zkhip_merkle *t, const uint64_t *leaf_indices, size_t count, uint8_t *out) {
    if (!ctx || !t || (count && (!leaf_indices || !out))) return ZKHIP_ERR_INVALID;
    if (count >= ((size_t)1 << 32)) return ZKHIP_ERR_RANGE;
    for (size_t k = 0; k < count; ++k)
        if (leaf_indices[k] >= t->leaves) return ZKHIP_ERR_RANGE;
    if (count == 0 || t->depth == 0) return ZKHIP_OK;
    ZK_ENTER(ctx);
    const size_t nodes = count * t->depth;
    PathBuffers w = {count, nodes};
    ZK_TRY(ws_place(ctx, w));
    ZK_TRY(ws_upload(ctx, w.idx, leaf_indices, count * 8));
    ZK_LAUNCH(ctx, "merkle_path_gather", merkle_path_gather, grid_1d(nodes * 2), dim3(256), 0, (const uint4 *)t->d, t->leaves, (uint32_t)t->depth, w.idx, nodes * 2,
              w.out);
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(out, w.out, nodes * 32, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // the digests are in `out` when the call returns
    return ZKHIP_OK;
}

int zkhip_fri_query_dev(zkhip_ctx *ctx, const zkhip_fri_query_set *sets, size_t n_sets, const uint64_t *x_indices, size_t count, uint64_t *out) {
    if (!ctx) return ZKHIP_ERR_INVALID;
    if (count == 0 || n_sets == 0) return ZKHIP_OK;
    if (!sets || !x_indices || !out) return ZKHIP_ERR_INVALID;
    for (size_t t = 0; t < n_sets; ++t)
        if (!sets[t].d_polys || sets[t].batch == 0) return ZKHIP_ERR_INVALID;
    if (count >= ((size_t)1 << 32) || n_sets >= ((size_t)1 << 32)) return ZKHIP_ERR_RANGE;
    size_t max_log = 0, elements = 0;
    std::vector<FriQuerySet> table(n_sets);
    for (size_t t = 0; t < n_sets; ++t) {
        const zkhip_fri_query_set &s = sets[t];
        if (s.fri_step < 1 || s.fri_step > s.log_domain || s.log_domain > 32 || s.batch >= ((size_t)1 << 31)) return ZKHIP_ERR_RANGE;
        max_log = std::max(max_log, s.log_domain);
        // the answers are a few elements per query: 2^38 of them and more is not a query phase.  Held against what is left of that bound before
        // the product is formed (batch < 2^31 and fri_step <= 32 keep the shift below 2^63; times count it could wrap)
        const size_t per_query = s.batch << s.fri_step, limit = (size_t)1 << 38;
        if (per_query > (limit - 1 - elements) / count) return ZKHIP_ERR_RANGE;
        elements += count * per_query;
        table[t] = {(const uint4 *)s.d_polys, (uint32_t)s.log_domain, (uint32_t)s.batch, (uint32_t)s.fri_step, elements};
    }
    for (size_t q = 0; q < count; ++q)
        if (x_indices[q] >> max_log) return ZKHIP_ERR_RANGE;
    ZK_ENTER(ctx);
    QueryBuffers w = {n_sets, count, elements};
    ZK_TRY(ws_place(ctx, w));
    ZK_TRY(ws_upload(ctx, w.sets, table.data(), n_sets * sizeof(FriQuerySet)));
    ZK_TRY(ws_upload(ctx, w.idx, x_indices, count * 8));
    ZK_LAUNCH(ctx, "fri_query_gather", fri_query_gather, grid_1d(elements * 2), dim3(256), 0, w.sets, (uint32_t)n_sets, w.idx, elements * 2, w.out);
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(out, w.out, elements * 32, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // the answers are in `out`, and `table` has been read, when the call returns
    return ZKHIP_OK;
}

int zkhip_merkle_paths_multi(zkhip_ctx *ctx, const zkhip_merkle *const *trees, size_t n_trees, const uint64_t *x_indices, size_t count, uint8_t *out) {
    if (!ctx || (n_trees && !trees)) return ZKHIP_ERR_INVALID;
    for (size_t t = 0; t < n_trees; ++t)
        if (!trees[t]) return ZKHIP_ERR_INVALID;
    if (count == 0 || n_trees == 0) return ZKHIP_OK;
    if (!x_indices) return ZKHIP_ERR_INVALID;
    if (count >= ((size_t)1 << 32) || n_trees >= ((size_t)1 << 32)) return ZKHIP_ERR_RANGE;
    size_t nodes = 0;
    std::vector<PathTree> table(n_trees);
    for (size_t t = 0; t < n_trees; ++t) {
        nodes += count * trees[t]->depth;
        table[t] = {(const uint4 *)trees[t]->d, trees[t]->leaves, trees[t]->depth, nodes};
    }
    if (nodes == 0) return ZKHIP_OK;  // one-leaf trees only: no bytes
    if (!out) return ZKHIP_ERR_INVALID;
    ZK_ENTER(ctx);
    MultiPathBuffers w = {n_trees, count, nodes};
    ZK_TRY(ws_place(ctx, w));
    ZK_TRY(ws_upload(ctx, w.trees, table.data(), n_trees * sizeof(PathTree)));
    ZK_TRY(ws_upload(ctx, w.idx, x_indices, count * 8));
    ZK_LAUNCH(ctx, "merkle_path_gather_multi", merkle_path_gather_multi, grid_1d(nodes * 2), dim3(256), 0, w.trees, (uint32_t)n_trees, w.idx, nodes * 2, w.out);
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(out, w.out, nodes * 32, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // the digests are in `out`, and `table` has been read, when the call returns
    return ZKHIP_OK;
}

void zkhip_merkle_free(zkhip_ctx *ctx, zkhip_merkle *t) {
    if (!t) return;
    if (ctx && t->d) (void)zkhip_free(ctx, t->d);
    delete t;
}

}  // extern "C"
