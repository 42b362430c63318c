// C++ shim test harness (test-only) of the device Merkle builder: lpc_commitment_scheme_hip driven twice over the same inputs and the same
// scripted challenges -- once with device_merkle_builder (hip/merkle.hpp: every tree hashed on the GPU), once with a host builder that keeps
// the leaves it is handed -- so that Python can hash the captured leaves (hashlib) and hold the device roots against them.
// Built into libmerkletest.so by tests/cpp/Makefile; driven by tests/test_gpu_merkle_shim.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include <nil/crypto3/zk/hip/lpc.hpp>
#include <nil/crypto3/zk/hip/merkle.hpp>

#include "harness_common.hpp"

using namespace nil::crypto3::zk::hip;

namespace {

/// hands out the caller's challenges, counts what it absorbed (roots of either type)
template <typename Curve>
struct scripted_transcript {
    typedef curve_adapter<Curve> A;
    std::vector<typename A::scalar_value_type> challenges;
    std::size_t next = 0, absorbed = 0;
    template <typename T>
    void operator()(const T &) { ++absorbed; }
    typename A::scalar_value_type challenge() { return challenges.at(next++); }
};

/// the leaves of every tree a host run built, in build order
struct captured_tree {
    std::size_t per_leaf = 0;
    std::vector<std::uint64_t> limbs;    // total elements x 4
};
std::vector<captured_tree> g_captured;

struct capture_root {
    std::uint64_t ordinal = 0;
    const std::uint64_t &root() const { return ordinal; }
};
/// vector-shaped host builder: keeps the leaves, the "root" is the tree's ordinal
template <typename Curve>
struct capture_builder {
    typedef curve_adapter<Curve> A;
    capture_root operator()(const std::vector<typename A::scalar_value_type> &leaves, std::size_t per_leaf) const {
        captured_tree t;
        t.per_leaf = per_leaf;
        t.limbs.resize(4 * leaves.size());
        for (std::size_t i = 0; i < leaves.size(); ++i) A::scalar_to_limbs(leaves[i], &t.limbs[4 * i]);
        g_captured.push_back(std::move(t));
        return capture_root {g_captured.size() - 1};
    }
};

void put_root(const device_merkle_tree::digest_type &d, std::uint8_t *out) { std::memcpy(out, d.data(), 32); }
void put_root(const std::uint64_t &, std::uint8_t *out) { std::memset(out, 0, 32); }

/// the tree of a device run, checked against itself: paths of the first, the last and a middle leaf equal the siblings in the digest array
int check_paths(const device_merkle_tree &t) {
    const std::size_t L = t.leaves(), depth = t.depth();
    if (((std::size_t)1 << depth) != L) return -30;
    const auto all = t.digests();
    if (all.size() != 2 * L - 1 || all.back() != t.root()) return -31;
    const std::vector<std::size_t> idx = {0, L - 1, L / 3};
    const auto ps = t.proofs(idx);
    for (std::size_t k = 0; k < idx.size(); ++k) {
        if (ps[k].size() != depth || ps[k] != t.proof(idx[k])) return -32;
        for (std::size_t l = 0; l < depth; ++l)
            if (ps[k][l] != all[2 * L - ((2 * L) >> l) + ((idx[k] >> l) ^ 1)]) return -33;
    }
    return 0;
}
int check_paths(const capture_root &) { return 0; }

/// batch 0 (fixed) = polys[0..1], batch 1 = polys[2..]: commit both, open at ragged point sets, run proof_eval
template <typename Curve, typename Builder>
int lpc_run(const uint64_t *evals, size_t npolys, const uint64_t *log_n, size_t log_domain, const uint64_t *steps, size_t nsteps, const uint64_t *points,
            const uint64_t *challenges, size_t nchallenges, uint8_t *out_roots, uint8_t *out_fri_roots, uint64_t *out_z, uint64_t *out_alphas,
            uint64_t *out_final, uint64_t *out_counts) {
    typedef curve_adapter<Curve> A;
    typedef typename A::scalar_value_type Fr;
    typedef lpc_commitment_scheme_hip<Curve, scripted_transcript<Curve>, Builder> scheme_type;
    context ctx(0);
    std::vector<std::size_t> step_list(steps, steps + nsteps);
    scheme_type scheme(ctx, fri_params_hip<Curve>::standard(log_domain, step_list), Builder());
    std::vector<polynomial_dfs<Curve>> polys(npolys);
    size_t at = 0;
    for (size_t p = 0; p < npolys; ++p)
        for (size_t i = 0; i < ((size_t)1 << log_n[p]); ++i) polys[p].values.push_back(A::scalar_from_limbs(evals + 4 * at++));
    scripted_transcript<Curve> tr;
    for (size_t i = 0; i < nchallenges; ++i) tr.challenges.push_back(A::scalar_from_limbs(challenges + 4 * i));
    const std::vector<Fr> pts = {A::scalar_from_limbs(points), A::scalar_from_limbs(points + 4), A::scalar_from_limbs(points + 8)};

    scheme.append_to_batch(0, std::vector<polynomial_dfs<Curve>>(polys.begin(), polys.begin() + 2));
    put_root(scheme.commit(0), out_roots);
    scheme.mark_batch_as_fixed(0);
    auto prep = scheme.preprocess(tr);
    scheme.setup(tr, prep);
    scheme.append_to_batch(1, std::vector<polynomial_dfs<Curve>>(polys.begin() + 2, polys.end()));
    put_root(scheme.commit(1), out_roots + 32);
    scheme.append_eval_point(0, pts[0]);
    scheme.append_eval_point(1, pts[0]);
    scheme.append_eval_point(1, 0, pts[1]);
    scheme.append_eval_points(0, 1, std::vector<Fr> {pts[2]});
    auto proof = scheme.proof_eval(tr);

    size_t zi = 0;
    for (std::size_t k : proof.z.get_batches())
        for (std::size_t i = 0; i < proof.z.get_batch_size(k); ++i)
            for (std::size_t q = 0; q < proof.z.get_poly_points_number(k, i); ++q) A::scalar_to_limbs(proof.z.get(k, i, q), out_z + 4 * zi++);
    for (size_t i = 0; i < proof.fri_proof.fri_roots.size(); ++i) put_root(proof.fri_proof.fri_roots[i], out_fri_roots + 32 * i);
    for (size_t i = 0; i < scheme.fri_alphas().size(); ++i) A::scalar_to_limbs(scheme.fri_alphas()[i], out_alphas + 4 * i);
    for (size_t i = 0; i < proof.fri_proof.final_polynomial.size(); ++i) A::scalar_to_limbs(proof.fri_proof.final_polynomial[i], out_final + 4 * i);
    out_counts[0] = zi;
    out_counts[1] = proof.fri_proof.fri_roots.size();
    out_counts[2] = proof.fri_proof.final_polynomial.size();
    out_counts[3] = tr.next;
    out_counts[4] = tr.absorbed;
    out_counts[5] = scheme.fri_alphas().size();
    /* the trees the query phase reads are kept, and the roots handed out are theirs */
    if (scheme.trees().size() != 2 || scheme.fri_trees().size() != nsteps) return -10;
    for (const auto &it : scheme.trees())
        if (int rc = check_paths(it.second)) return rc;
    for (size_t i = 0; i < nsteps; ++i) {
        if (int rc = check_paths(scheme.fri_trees()[i])) return rc;
        std::uint8_t r[32];
        put_root(scheme.fri_trees()[i].root(), r);
        if (std::memcmp(r, out_fri_roots + 32 * i, 32) != 0) return -11;
    }
    return 0;
}

template <typename Curve>
int lpc_run_t(int device, const uint64_t *evals, size_t npolys, const uint64_t *log_n, size_t log_domain, const uint64_t *steps, size_t nsteps,
              const uint64_t *points, const uint64_t *challenges, size_t nchallenges, uint8_t *out_roots, uint8_t *out_fri_roots, uint64_t *out_z,
              uint64_t *out_alphas, uint64_t *out_final, uint64_t *out_counts) {
    typedef scripted_transcript<Curve> T;
    typedef device_merkle_builder<ZKHIP_HASH_SHA2_256> D;
    /* the new kind is the device builder's alone; a host builder is classified as before */
    static_assert(lpc_commitment_scheme_hip<Curve, T, D>::builder_kind == detail::tree_builder_kind::device, "device builder");
    static_assert(lpc_commitment_scheme_hip<Curve, T, capture_builder<Curve>>::builder_kind == detail::tree_builder_kind::vector, "vector builder");
    static_assert(std::is_same<typename lpc_commitment_scheme_hip<Curve, T, D>::precommitment_type, device_merkle_tree>::value, "the tree is the precommitment");
    static_assert(std::is_same<typename lpc_commitment_scheme_hip<Curve, T, D>::commitment_type, std::array<std::uint8_t, 32>>::value, "the root is 32 bytes");
    if (device)
        return lpc_run<Curve, D>(evals, npolys, log_n, log_domain, steps, nsteps, points, challenges, nchallenges, out_roots, out_fri_roots, out_z, out_alphas,
                                 out_final, out_counts);
    g_captured.clear();
    return lpc_run<Curve, capture_builder<Curve>>(evals, npolys, log_n, log_domain, steps, nsteps, points, challenges, nchallenges, out_roots, out_fri_roots,
                                                  out_z, out_alphas, out_final, out_counts);
}

}    // namespace

extern "C" {

/// device != 0: the scheme with device_merkle_builder, roots out; device == 0: with the leaf-capturing host builder (roots zeroed, leaves kept
/// for merkle_captured_*)
int merkle_lpc_run(int curve, int device, const uint64_t *evals, size_t npolys, const uint64_t *log_n, size_t log_domain, const uint64_t *steps, size_t nsteps,
                   const uint64_t *points, const uint64_t *challenges, size_t nchallenges, uint8_t *out_roots, uint8_t *out_fri_roots, uint64_t *out_z,
                   uint64_t *out_alphas, uint64_t *out_final, uint64_t *out_counts) {
    return harness::guarded(__func__, [&] {
        if (curve == ZKHIP_BLS12_381)
            return lpc_run_t<bls12_381>(device, evals, npolys, log_n, log_domain, steps, nsteps, points, challenges, nchallenges, out_roots, out_fri_roots, out_z,
                                        out_alphas, out_final, out_counts);
        return lpc_run_t<alt_bn128_254>(device, evals, npolys, log_n, log_domain, steps, nsteps, points, challenges, nchallenges, out_roots, out_fri_roots, out_z,
                                        out_alphas, out_final, out_counts);
    });
}

size_t merkle_captured_count() { return g_captured.size(); }
size_t merkle_captured_elements(size_t i) { return i < g_captured.size() ? g_captured[i].limbs.size() / 4 : 0; }
size_t merkle_captured_per_leaf(size_t i) { return i < g_captured.size() ? g_captured[i].per_leaf : 0; }
int merkle_captured_copy(size_t i, uint64_t *out) {
    if (i >= g_captured.size()) return -1;
    std::memcpy(out, g_captured[i].limbs.data(), g_captured[i].limbs.size() * 8);
    return 0;
}
void merkle_captured_clear() { g_captured.clear(); }

}    // extern "C"
