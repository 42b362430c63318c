//---------------------------------------------------------------------------//
// zkhip shim: the Merkle trees of the LPC / FRI commitments, built and kept on the MI355X.
//
// Stands where containers::merkle_tree<hashes::sha2<256>, 2> stands in precommit<FRI> (zk/commitments/detail/polynomial/basic_fri.hpp:375-409,
// 461-496): `device_merkle_tree` is the tree -- root(), the authentication paths the query phase reads --, `device_merkle_builder` the tree
// builder lpc_commitment_scheme_hip takes (hip/lpc.hpp, tree_builder_kind::device): it is handed the evaluations where they lie on the device
// and hashes the coset-ordered leaves straight out of them.
//
// Conventions (include/zkhip.h, "Merkle trees"): an element is the 32-byte big-endian encoding of its canonical integer, a leaf digest the
// SHA2-256 of the leaf's elements in leaf order, an inner node SHA2-256(left || right), arity 2, a power-of-two leaf count.
//
// This header is the only one of the shim that refers to the zkhip_merkle_* entry points: code that never names a device tree builder does
// not need them at link time.
//---------------------------------------------------------------------------//
#ifndef ZKHIP_SHIM_MERKLE_HPP
#define ZKHIP_SHIM_MERKLE_HPP

#include <algorithm>
#include <array>
#include <cstdint>
#include <memory>
#include <vector>

#include "backend.hpp"

namespace nil {
namespace crypto3 {
namespace zk {
namespace hip {

/// The authentication path of one leaf as a query proof carries it (merkle_proof in basic_fri.hpp's initial_proof_type / round_proof_type)
struct device_merkle_path {
    std::size_t leaf_index = 0;
    std::vector<std::array<std::uint8_t, 32>> siblings;    // leaf level first
    /// the root this path leads to from a leaf's digest: the node convention of include/zkhip.h, hashed on the host
    std::array<std::uint8_t, 32> root_from(std::array<std::uint8_t, 32> digest) const {
        std::uint8_t node[64];
        for (std::size_t l = 0; l < siblings.size(); ++l) {
            const bool right = (leaf_index >> l) & 1;
            std::copy_n(digest.begin(), 32, node + (right ? 32 : 0));
            std::copy_n(siblings[l].begin(), 32, node + (right ? 0 : 32));
            check(zkhip_sha256_host(node, 64, digest.data()), "zkhip_sha256_host");
        }
        return digest;
    }
};

/// A Merkle tree resident on the device (RAII over zkhip_merkle; copies share the tree).  The context must outlive it.
class device_merkle_tree {
public:
    typedef std::array<std::uint8_t, 32> digest_type;
    typedef std::vector<digest_type> proof_type;    // the sibling digests of a leaf's ancestors, leaf level first
    typedef device_merkle_path path_type;

    /// the paths of every query index in every tree (the trees of one context), tree t answering leaf x mod leaves(t): one device pass and one
    /// copy for all of them (zkhip_merkle_paths_multi); out[t][q]
    static std::vector<std::vector<device_merkle_path>> paths_multi(const context &ctx, const std::vector<const device_merkle_tree *> &trees,
                                                                    const std::vector<std::uint64_t> &x_indices) {
        std::vector<const zkhip_merkle *> handles;
        std::size_t bytes = 0;
        for (const device_merkle_tree *t : trees) {
            handles.push_back(t->get());
            bytes += x_indices.size() * t->depth() * 32;
        }
        std::vector<std::uint8_t> flat(bytes);
        ZKHIP_CALL(ctx, zkhip_merkle_paths_multi, handles.data(), handles.size(), x_indices.data(), x_indices.size(), flat.data());
        std::vector<std::vector<device_merkle_path>> out(trees.size());
        const std::uint8_t *at = flat.data();
        for (std::size_t t = 0; t < trees.size(); ++t) {
            const std::size_t d = trees[t]->depth(), L = trees[t]->leaves();
            out[t].resize(x_indices.size());
            for (std::size_t q = 0; q < x_indices.size(); ++q) {
                out[t][q].leaf_index = x_indices[q] % L;
                out[t][q].siblings.resize(d);
                for (std::size_t l = 0; l < d; ++l, at += 32) std::copy_n(at, 32, out[t][q].siblings[l].begin());
            }
        }
        return out;
    }

    device_merkle_tree() = default;
    /// takes the handle over; the root is fetched here, once
    device_merkle_tree(const context &ctx, zkhip_merkle *tree) : ctx_(&ctx) {
        zkhip_ctx *c = ctx.get();
        tree_ = std::shared_ptr<zkhip_merkle>(tree, [c](zkhip_merkle *t) { zkhip_merkle_free(c, t); });
        ZKHIP_CALL(ctx, zkhip_merkle_root, tree, root_.data());
    }
    /// the tree over `batch` polynomials resident as evaluations over the 2^log_domain-point domain, leaves as precommit<FRI> lays them out
    static device_merkle_tree from_evaluations(const context &ctx, int hash, const void *d_evals, std::size_t batch, std::size_t log_domain,
                                               std::size_t fri_step) {
        zkhip_merkle *t = nullptr;
        ZKHIP_CALL(ctx, zkhip_merkle_build_fri_dev, hash, d_evals, log_domain, batch, fri_step, &t);
        return device_merkle_tree(ctx, t);
    }
    /// the tree over a leaf layout on the device: n_leaves leaves of elements_per_leaf elements
    static device_merkle_tree from_leaves(const context &ctx, int hash, const void *d_leaves, std::size_t n_leaves, std::size_t elements_per_leaf) {
        zkhip_merkle *t = nullptr;
        ZKHIP_CALL(ctx, zkhip_merkle_build_dev, hash, d_leaves, n_leaves, elements_per_leaf, &t);
        return device_merkle_tree(ctx, t);
    }

    const digest_type &root() const { return root_; }
    std::size_t leaves() const { return zkhip_merkle_leaves(tree_.get()); }
    std::size_t depth() const { return zkhip_merkle_depth(tree_.get()); }
    const zkhip_merkle *get() const { return tree_.get(); }

    /// the authentication path of one leaf: depth() sibling digests
    proof_type proof(std::size_t leaf_index) const { return proofs(std::vector<std::size_t> {leaf_index}).front(); }
    /// the paths of many leaves in one device pass and one copy (the query phase's lambda openings of a round)
    std::vector<proof_type> proofs(const std::vector<std::size_t> &leaf_indices) const {
        const std::size_t d = depth();
        std::vector<std::uint64_t> idx(leaf_indices.begin(), leaf_indices.end());
        std::vector<std::uint8_t> flat(idx.size() * d * 32);
        ZKHIP_CALL(*ctx_, zkhip_merkle_paths, tree_.get(), idx.data(), idx.size(), flat.data());
        std::vector<proof_type> out(idx.size(), proof_type(d));
        for (std::size_t k = 0; k < idx.size(); ++k)
            for (std::size_t l = 0; l < d; ++l) std::copy_n(flat.data() + (k * d + l) * 32, 32, out[k][l].begin());
        return out;
    }
    /// every digest: the leaves() leaf digests, then each level above, the root last
    std::vector<digest_type> digests() const {
        std::vector<digest_type> out(2 * leaves() - 1);
        ZKHIP_CALL(*ctx_, zkhip_merkle_digests, tree_.get(), out.front().data());
        return out;
    }

private:
    const context *ctx_ = nullptr;
    std::shared_ptr<zkhip_merkle> tree_;
    digest_type root_ {};
};

/// The tree builder that keeps lpc_commitment_scheme_hip's hashing on the device.  `Hash`: a ZKHIP_HASH_* id.
template <int Hash = ZKHIP_HASH_SHA2_256>
struct device_merkle_builder {
    static_assert(Hash == ZKHIP_HASH_SHA2_256, "device_merkle_builder: SHA2-256 is the only hash built for the device");
    device_merkle_tree operator()(const context &ctx, const void *d_evals, std::size_t batch, std::size_t log_domain, std::size_t fri_step) const {
        return device_merkle_tree::from_evaluations(ctx, Hash, d_evals, batch, log_domain, fri_step);
    }
};

}    // namespace hip
}    // namespace zk
}    // namespace crypto3
}    // namespace nil

#endif    // ZKHIP_SHIM_MERKLE_HPP
