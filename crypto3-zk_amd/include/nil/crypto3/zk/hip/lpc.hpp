//---------------------------------------------------------------------------//
// zkhip shim: the LPC (list polynomial commitment, FRI-based) scheme placeholder plugs in as `commitment_scheme_type`,
// with every polynomial-sized step on the MI355X.
//
// Mirrors zk/commitments/polynomial/lpc.hpp (class lpc_commitment_scheme, :50-300) on top of the polys_evaluator of
// polys_evaluator.hpp (batched_commitment.hpp:58-249, shared with the KZG schemes of kzg_v2.hpp) and the commit phase of
// algorithms::proof_eval<FRI> (zk/commitments/detail/polynomial/basic_fri.hpp:666-742) -- same member names, same call
// order: append_to_batch / commit(batch) / append_eval_point[s] / set_batch_size / mark_batch_as_fixed /
// preprocess / setup / proof_eval(transcript), public `_z`, `is_lpc()`.
//
// What runs where
//   device  commit: the batch's inverse NTTs (the coefficient forms stay resident: the reference re-derives them per use,
//           lpc.hpp:150,173), the extension of every polynomial to D[0] and the coset-ordered leaf layout
//           (basic_fri.hpp:433-496); proof_eval: eval_polys (block-Horner), the combined quotient
//           Q = sum_points (sum_k theta^k (g_k - z_k)) / (X - point)  (lpc.hpp:139-186; one pass over the resident
//           coefficients + one synthetic division per point), its extension, and the FRI commit phase
//           (fold_polynomial rounds + per-round leaf layouts, basic_fri.hpp:705-742).
//           hashing, WITH A DEVICE TREE BUILDER (tree_builder_kind::device; hip/merkle.hpp's device_merkle_builder: SHA2-256): the builder is
//           handed the resident evaluations -- b(ctx, d_evals, batch, log_domain, fri_step) -- and builds the Merkle tree of commit(batch), of
//           the combined quotient and of every FRI round on the GPU, leaf hashing fused with the leaf gather: no leaf layout is written and
//           no leaf crosses PCIe; the tree stays resident for the query phase's paths and only its 32-byte root comes back.
//   caller  hashing, with a host tree builder: the TreeBuilder builds the Merkle tree of a precommitment and exposes .root()
//           (containers::merkle_tree + the scheme's hash).  Three host shapes, best first (see tree_builder_kind):
//             streaming  b.begin(total_elements, elements_per_leaf); b.absorb(ptr, first_element, count) ...; b.finish()
//                        -- the leaves arrive in slices of whole leaves through two page-locked buffers: slice k + 1 crosses
//                        PCIe while the caller hashes slice k, nothing is materialised;
//             span       b(ptr, total_elements, elements_per_leaf) over a page-locked buffer the scheme keeps (one copy at link speed);
//             vector     b(const std::vector<value_type> &leaves, elements_per_leaf), as round 2 (a vector the scheme keeps).
//           transcript:
//           duck-typed on VALUES like the KZG schemes' (transcript(root), transcript.challenge()).
//   device  the QUERY phase of proof_eval<FRI> (basic_fri.hpp:747-930: fri_params.lambda openings at transcript-derived indices), behind names of
//           its own -- proof_eval keeps its statements, its transcript traffic and its result:
//             query_phase(transcript, proof)   after proof_eval on the same object; fills proof.fri_proof.query_proofs.  Everything it reads is
//                        resident -- the coefficient forms of every batch, every round polynomial, every tree -- and only the answers cross PCIe:
//                        per batch its polynomials are re-extended to D[0] into the commit's scratch and ONE zkhip_fri_query_dev gathers the
//                        pairs calculate_s walks from every query index; one more gathers y of every round; zkhip_merkle_paths_multi opens
//                        all batch trees, and all round trees, in one pass each (a host tree answers through its proof(i)).  The host keeps
//                        the domain indices (detail::domain_index: a walk down the 2-power subgroups, not the reference's scan of D[0]) and
//                        the final polynomial at +-x^2.
//             proof_eval_full(transcript)      proof_eval, then query_phase: a proof a verifier can check.
//             verify_eval(proof, commitments, transcript)   lpc.hpp:202-300 over basic_fri.hpp:933-1154, host only; for the device builder,
//                        whose leaf and node hashing include/zkhip.h states.
//           A caller that runs its own query phase still finds what it needs through trees() / fri_trees() / fri_round_polynomial(i) /
//           coefficients(batch, i) / fri_alphas().
//   device  grinding (basic_fri.hpp:743-745), when fri_params.use_grinding is set: the proof of work between the commit and the query phase
//           is searched on the GPU (hip/proof_of_work.hpp: proof_of_work_hip over the transcript's state()) and returned in
//           fri_proof.proof_of_work.  It needs the SHA2-256 sequential transcript (hip/transcript.hpp, or any type with its state()); without
//           use_grinding nothing is launched and the transcript sees the calls it always saw.
//
// Over a device group (constructor taking a device_group): commit(batch) deals the batch's polynomials over the members -- uploads over
// their own PCIe links, extensions on their own GPUs --, then the path's one exchange: the leaf range of every LEAF OWNER (the first 2^k
// members) is made of 2^fri_step segments of every polynomial, which the members pack and push to the owners; each owner lays out ITS
// leaves and sends them to the host over ITS link while the caller hashes.  Same leaves, same order, same roots as on one device; the
// coefficient forms are gathered on member 0, where proof_eval runs as before.  See commit_group.  A device tree builder over a group is
// not supported (the leaf owners would each hold a subtree): the group constructor refuses it at compile time.
// Lone or over a group, what a commit keeps across calls exists once per member -- its upload stream (polys_evaluator.hpp) and its scratch
// (member_scratch; entry 0 is the lone context's) -- and a host builder gets its leaves through one function, deliver_leaves, over blocks of
// laid-out leaves: one block on one context, or the owners' blocks on theirs.
//---------------------------------------------------------------------------//
#ifndef ZKHIP_SHIM_LPC_HPP
#define ZKHIP_SHIM_LPC_HPP

#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstdio>
#include <chrono>
#include <functional>
#include <map>
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

#include "fri.hpp"
#include "polys_evaluator.hpp"
#include "proof_of_work.hpp"

namespace nil {
namespace crypto3 {
namespace zk {
namespace hip {

/// What the scheme reads of basic_fri::params_type (basic_fri.hpp:86-140): the domains D[t] (size 2^(log_domain - t),
/// generator root_of_unity(log_domain - t)) and the step list; r = sum(step_list) folding rounds.
template <typename CurveType>
struct fri_params_hip {
    typedef typename curve_adapter<CurveType>::scalar_value_type value_type;
    std::size_t log_domain = 0;
    std::vector<std::size_t> step_list;
    std::function<value_type(std::size_t log_n)> root_of_unity;
    /// basic_fri.hpp:123-124, defaults as :156-157 (trailing, so that aggregate initialisation of the members above stays as it was)
    bool use_grinding = false;
    std::uint32_t grinding_parameter = 0xFFFF;    // the mask a nonce's int_challenge must clear
    /// the number of queries (basic_fri.hpp:122); 0: the scheme stops after the commit phase (proof_eval), query_phase refuses.  Trailing too.
    std::size_t lambda = 0;
    /// the degree bound the proof is about (basic_fri.hpp:228: every committed polynomial has degree <= max_degree); read by verify_eval
    /// alone, which refuses to run without it (0: unset).  Trailing too.
    std::size_t max_degree = 0;
    /// the roots the reference's domains D[i] = make_evaluation_domain(2^(log_domain - i)) carry (fri params, basic_fri.hpp:84-118),
    /// from the curve adapter's field constants
    static fri_params_hip standard(std::size_t log_domain, std::vector<std::size_t> step_list) {
        return {log_domain, std::move(step_list), [](std::size_t log_n) { return curve_adapter<CurveType>::root_of_unity(log_n); }};
    }
};

namespace detail {
    /// which of the tree-builder shapes a type offers (see the header comment): three that hash on the host, one that hashes on the device
    enum class tree_builder_kind { streaming, span, vector, device };
    template <typename B, typename V, typename = void>
    struct is_streaming_builder : std::false_type { };
    template <typename B, typename V>
    struct is_streaming_builder<B, V,
                                std::void_t<decltype(std::declval<B &>().begin(std::size_t(), std::size_t())),
                                            decltype(std::declval<B &>().absorb(static_cast<const V *>(nullptr), std::size_t(), std::size_t())),
                                            decltype(std::declval<B &>().finish())>> : std::true_type { };
    template <typename B, typename V, typename = void>
    struct is_span_builder : std::false_type { };
    template <typename B, typename V>
    struct is_span_builder<B, V, std::void_t<decltype(std::declval<B &>()(static_cast<const V *>(nullptr), std::size_t(), std::size_t()))>> : std::true_type { };
    template <typename B, typename = void>
    struct is_device_builder : std::false_type { };
    template <typename B>
    struct is_device_builder<B, std::void_t<decltype(std::declval<B &>()(std::declval<const context &>(), static_cast<const void *>(nullptr), std::size_t(),
                                                                         std::size_t(), std::size_t()))>> : std::true_type { };
    /// a transcript that shows its state(): what the device's proof-of-work search starts from
    template <typename T, typename = void>
    struct has_state : std::false_type { };
    template <typename T>
    struct has_state<T, std::void_t<decltype(std::declval<const T &>().state())>> : std::true_type { };
    template <typename B, typename V, tree_builder_kind K>
    struct tree_builder_result;
    template <typename B, typename V>
    struct tree_builder_result<B, V, tree_builder_kind::device> {
        typedef typename std::decay<decltype(std::declval<B &>()(std::declval<const context &>(), static_cast<const void *>(nullptr), std::size_t(), std::size_t(),
                                                                  std::size_t()))>::type type;
    };
    template <typename B, typename V>
    struct tree_builder_result<B, V, tree_builder_kind::streaming> {
        typedef typename std::decay<decltype(std::declval<B &>().finish())>::type type;
    };
    template <typename B, typename V>
    struct tree_builder_result<B, V, tree_builder_kind::span> {
        typedef typename std::decay<decltype(std::declval<B &>()(static_cast<const V *>(nullptr), std::size_t(), std::size_t()))>::type type;
    };
    template <typename B, typename V>
    struct tree_builder_result<B, V, tree_builder_kind::vector> {
        typedef typename std::decay<decltype(std::declval<B &>()(std::declval<const std::vector<V> &>(), std::size_t()))>::type type;
    };

    // ---- the query phase (basic_fri.hpp:747-930) ----
    /// a host tree that can open a leaf: proof(std::size_t)
    template <typename Tree, typename = void>
    struct has_proof : std::false_type { };
    template <typename Tree>
    struct has_proof<Tree, std::void_t<decltype(std::declval<const Tree &>().proof(std::size_t()))>> : std::true_type { };
    /// what stands for the path of a host tree that cannot open a leaf (query_phase does not compile for it)
    struct no_merkle_path { };
    /// the path a query proof carries: the device tree's path_type (hip/merkle.hpp's device_merkle_path), or whatever a host tree's proof(i) returns
    template <typename Tree, bool Device, bool HasProof>
    struct merkle_path_of {
        typedef no_merkle_path type;
    };
    template <typename Tree, bool HasProof>
    struct merkle_path_of<Tree, true, HasProof> {
        typedef typename Tree::path_type type;
    };
    template <typename Tree>
    struct merkle_path_of<Tree, false, true> {
        typedef typename std::decay<decltype(std::declval<const Tree &>().proof(std::size_t()))>::type type;
    };

    /// base^e, e as four little-endian 64-bit limbs
    template <typename V>
    V pow_limbs(const V &base, const std::uint64_t *e) {
        V acc = V::one();
        for (int bit = 255; bit >= 0; --bit) {
            acc = acc * acc;
            if ((e[bit / 64] >> (bit % 64)) & 1) acc = acc * base;
        }
        return acc;
    }
    template <typename V>
    V pow_index(const V &base, std::size_t e) {
        const std::uint64_t limbs[4] = {e, 0, 0, 0};
        return pow_limbs(base, limbs);
    }
    /// The index of x in the domain of 2^log_domain points: the e with omega^e = x, omega = root_of_unity(log_domain).  Where the reference scans
    /// the whole domain (basic_fri.hpp:781-786), this walks down the tower of 2-power subgroups: x^(2^j) lies in the subgroup of order
    /// 2^(log_domain - j), so from j = log_domain - 1 down to 0 each level fixes one more bit of e, lowest first -- log_domain squarings of x and of
    /// omega, then a product of at most log_domain known powers per bit.  Same index as the scan's.  An x outside the domain (0, or an element of
    /// larger order: the reference's scan would run off the domain's end) throws.
    template <typename V, typename RootFn>
    std::size_t domain_index(const V &x, std::size_t log_domain, const RootFn &root_of_unity) {
        std::vector<V> xs(log_domain + 1), ws(log_domain + 1);    // xs[j] = x^(2^j), ws[j] = omega^(2^j)
        xs[0] = x;
        ws[0] = root_of_unity(log_domain);
        for (std::size_t j = 0; j < log_domain; ++j) {
            xs[j + 1] = xs[j] * xs[j];
            ws[j + 1] = ws[j] * ws[j];
        }
        if (!(xs[log_domain] == V::one())) throw std::runtime_error("lpc query phase: the challenge does not map into the domain");
        std::size_t e = 0;
        for (std::size_t k = 0; k < log_domain; ++k) {    // bit k of e, read off x^(2^j) = omega^(2^j e) with j = log_domain - 1 - k
            const std::size_t j = log_domain - 1 - k;
            V low = V::one();    // omega^(2^j (e mod 2^k))
            for (std::size_t b = 0; b < k; ++b)
                if ((e >> b) & 1) low = low * ws[j + b];
            if (xs[j] == low) continue;
            if (!(xs[j] == low * ws[j + k])) throw std::runtime_error("lpc query phase: the challenge does not map into the domain");
            e |= (std::size_t)1 << k;
        }
        return e;
    }
    /// calculate_s's walk (basic_fri.hpp:585-614) as positions: pair j of the 2^(fri_step - 1) pairs read from x over the 2^log_n-point domain is
    /// (f[p_j], f[p_j + N/2]) with p_j = (x + the offsets N/4, N/8, ... picked by the bits of j) mod N/2 -- the smaller index of the pair
    inline std::vector<std::size_t> pair_positions(std::size_t x, std::size_t log_n, std::size_t fri_step) {
        const std::size_t N = (std::size_t)1 << log_n, half = (std::size_t)1 << (fri_step - 1);
        std::vector<std::size_t> pos(half);
        for (std::size_t j = 0; j < half; ++j) {
            std::size_t s = x;
            for (std::size_t l = 0; l + 1 < fri_step; ++l)
                if ((j >> l) & 1) s += N >> (2 + l);
            pos[j] = s & ((N >> 1) - 1);
        }
        return pos;
    }
}    // namespace detail

/// The batches, the points, `_z` and eval_polys: polys_evaluator.hpp.  Host polynomials only: commit reads every one through its pointer.
/// `PolynomialType`: as for the KZG schemes (batched_commitment.hpp:56-64) -- size() and operator[] over contiguous scalars.
template <typename CurveType, typename TranscriptType, typename TreeBuilder, typename PolynomialType = polynomial_dfs<CurveType>>
class lpc_commitment_scheme_hip : public polys_evaluator_hip<CurveType, PolynomialType> {
    typedef polys_evaluator_hip<CurveType, PolynomialType> base;

public:
    static constexpr bool is_lpc() { return true; }

    typedef typename base::adapter adapter;
    typedef fr_vector<CurveType> fv;
    typedef CurveType curve_type;
    typedef typename base::scalar_value_type value_type;
    typedef fri_params_hip<CurveType> params_type;
    typedef TranscriptType transcript_type;
    typedef typename base::poly_type poly_type;
    typedef typename base::eval_storage_type eval_storage_type;
    static constexpr detail::tree_builder_kind builder_kind =
        detail::is_device_builder<TreeBuilder>::value
            ? detail::tree_builder_kind::device
            : detail::is_streaming_builder<TreeBuilder, value_type>::value
                  ? detail::tree_builder_kind::streaming
                  : (detail::is_span_builder<TreeBuilder, value_type>::value ? detail::tree_builder_kind::span : detail::tree_builder_kind::vector);
    typedef typename detail::tree_builder_result<TreeBuilder, value_type, builder_kind>::type precommitment_type;
    typedef typename std::decay<decltype(std::declval<const precommitment_type &>().root())>::type commitment_type;
    typedef std::map<std::size_t, std::vector<value_type>> preprocessed_data_type;
    /// the path a query proof carries (basic_fri.hpp:228-290): device_merkle_path with the device builder, a host tree's proof(i) otherwise
    typedef typename detail::merkle_path_of<precommitment_type, builder_kind == detail::tree_builder_kind::device,
                                            detail::has_proof<precommitment_type>::value>::type merkle_path_type;
    struct initial_proof_type {
        std::vector<std::vector<std::array<value_type, 2>>> values;    // [polynomial][pair], in calculate_s's order from the query's x
        merkle_path_type p;
    };
    struct round_proof_type {
        std::vector<std::array<value_type, 2>> y;
        merkle_path_type p;
    };
    struct query_proof_type {
        std::map<std::size_t, initial_proof_type> initial_proof;
        std::vector<round_proof_type> round_proofs;
    };
    struct fri_proof_type {
        std::vector<commitment_type> fri_roots;
        std::vector<value_type> final_polynomial;    // coefficients (math::polynomial(f.coefficients()), basic_fri.hpp:736-742)
        std::uint32_t proof_of_work = 0;             // the grinding nonce (basic_fri.hpp:296, 743-745); 0 without use_grinding
        std::vector<query_proof_type> query_proofs;  // lambda of them after query_phase / proof_eval_full; proof_eval leaves it empty
    };
    struct proof_type {
        eval_storage_type z;
        fri_proof_type fri_proof;
    };

    using base::_z;

    lpc_commitment_scheme_hip(const context &ctx, const params_type &fri_params, TreeBuilder builder) :
        lpc_commitment_scheme_hip(ctx, 1, fri_params, std::move(builder)) { }

    /// the scheme over a device group: commit(batch) spreads over the members (commit_group), everything else runs on member 0
    lpc_commitment_scheme_hip(const device_group &group, const params_type &fri_params, TreeBuilder builder) :
        lpc_commitment_scheme_hip(group.root(), group.size(), fri_params, std::move(builder)) {
        static_assert(builder_kind != detail::tree_builder_kind::device,
                      "lpc over a device group takes a host tree builder: a device tree builder (hip/merkle.hpp) works on one context only");
        _group = &group;
    }

    const params_type &get_commitment_params() const { return _fri_params; }

    /// lpc.hpp:82-96: the fixed batches' polynomials evaluated at etha
    preprocessed_data_type preprocess(transcript_type &transcript) const {
        const value_type etha = transcript.challenge();
        preprocessed_data_type result;
        for (const auto &it : _batch_fixed) {
            if (!it.second) continue;
            result[it.first] = this->evaluate_batch_at(it.first, etha);
        }
        return result;
    }
    void setup(transcript_type &transcript, const preprocessed_data_type &preprocessed_data) {
        _etha = transcript.challenge();
        _fixed_polys_values = preprocessed_data;
    }
    /// Should be done after commitment (lpc.hpp:109-111)
    void mark_batch_as_fixed(std::size_t index) { _batch_fixed[index] = true; }

    /// commit(index) (lpc.hpp:101-106): precommit<FRI>(polys, D[0], step_list.front()) -> the tree's root
    commitment_type commit(std::size_t index) {
        ZKHIP_PROFILE_SCOPE("Basic FRI Precommit time");    // commit = precommit<FRI> + root (lpc.hpp:101-106; the scope of basic_fri.hpp:449)
        const std::vector<const poly_type *> &polys = this->_polys[index];
        device_batch db;
        for (const poly_type *p : polys) {
            if (p->size() == 0 || (p->size() & (p->size() - 1)) || p->size() > domain_size(0)) throw std::runtime_error("lpc commit: bad polynomial size");
            db.append(p->size());
        }
        db.data = _ctx.alloc(std::max<std::size_t>(1, db.total) * 32);
        const std::size_t D = domain_size(0), count = polys.size();
        root_map roots;    // D[0]'s root first, then one per distinct size
        roots[_fri_params.log_domain] = limbs_of<adapter>(_fri_params.root_of_unity(_fri_params.log_domain));
        detail::add_roots<adapter>(roots, db, _fri_params.root_of_unity);
        if (_group && _group->size() > 1 && count) {
            /* host builders only: the group constructor, which alone sets _group, does not compile for a device builder */
            if constexpr (builder_kind != detail::tree_builder_kind::device) commit_group(index, polys, db, roots);
        } else {
            char *d_ext = static_cast<char *>(_scratch[0].ext.reserve(_ctx, std::max<std::size_t>(1, count) * D * 32));    // kept across commits: no GB-sized hipMalloc per batch
            extend_columns(polys, db, 0, count, static_cast<char *>(db.data.get()), _ctx, 0, d_ext, roots);
            _trees.erase(index);
            _trees.emplace(index, build_tree(d_ext, count, _fri_params.log_domain, _fri_params.step_list.front()));
        }
        this->state_commited(index, std::move(db));
        return _trees.at(index).root();
    }

    /// commits that ran over the device group, and over how many leaf owners the last one cut its leaves (tests and logs)
    std::size_t group_commits() const { return _group_commits; }
    std::size_t last_leaf_owners() const { return _last_owners; }

    /// polynomials per upload chunk of commit() (0: the whole batch in one transfer)
    std::size_t upload_chunk = 4;
    /// elements per slice handed to a streaming tree builder (rounded up to whole leaves)
    std::size_t leaf_slice_elements = (std::size_t)1 << 21;

protected:
    typedef typename base::device_batch device_batch;
    typedef typename base::root_map root_map;
    using base::_ctx;
    using base::_points;
    using base::_dev;

    /// poly.resize(D[0]->size()) (basic_fri.hpp:452-455) for polys [lo, hi) of a batch on `ctx`, one call per chunk of equally sized
    /// polynomials: uploaded into `base` (polynomial p at base + 32 (offset[p] - offset[lo])), where the call leaves the COEFFICIENTS proof_eval
    /// reads later, and extended to d_ext + 32 (p - lo) D.  The chunks go up on member `k`'s upload stream (upload_context: a second in-order
    /// stream of ctx's GPU): chunk c + 1 crosses PCIe while chunk c is transformed.  Enqueued only.
    void extend_columns(const std::vector<const poly_type *> &polys, const device_batch &db, std::size_t lo, std::size_t hi, char *base, const context &ctx,
                        std::size_t k, char *d_ext, const root_map &roots) const {
        const std::size_t D = domain_size(0);
        const bool pipelined = upload_chunk != 0 && hi - lo > upload_chunk;
        const context &upc = pipelined ? this->upload_context(k, ctx) : ctx;
        auto at = [&](std::size_t p) { return base + 32 * (db.offset[p] - db.offset[lo]); };
        db.for_each_run(lo, hi, upload_chunk, upload_chunk, [&](std::size_t i, std::size_t j) {
            for (std::size_t p = i; p < j; ++p) upload_scalars<adapter>(upc, at(p), detail::poly_data<adapter>(*polys[p]), polys[p]->size());
            if (pipelined) ctx.wait_for(upc);
            const std::size_t log_n = detail::ceil_log2(db.len[i]);
            ZKHIP_CALL(ctx, zkhip_poly_resize_dev, adapter::id, at(i), log_n, j - i, roots.at(log_n).data(), d_ext + 32 * (i - lo) * D, _fri_params.log_domain,
                       roots.at(_fri_params.log_domain).data());    // the roots are packed once per batch (root_map), not per call
        });
    }

    /// commit(index) over the device group.  Member k takes the k-th contiguous range of the batch's polynomials: its host thread uploads them
    /// over the member's own link and extends them to D[0] on the member's GPU (extend_columns, as on one device).  The
    /// leaves are then cut by RANGE over the first 2^k members (the leaf owners): leaf x reads, of every polynomial, the positions
    /// x + j D / 2^step (fri_leaf_gather, poly.hip), so an owner's L = D / 2^step / owners consecutive leaves read 2^step segments of L
    /// consecutive evaluations per polynomial -- packed side by side they ARE the evaluations over a domain of D / owners points as far as the
    /// leaf layout is concerned (segment j of the small domain is segment j of the large one), and the owner runs the ordinary leaf kernel on
    /// them.  The exchange: every member packs, per owner, the segments of its polynomials (one strided copy) and pushes the block into the
    /// owner's buffer (zkhip_group_copy: ordered after the extension on the source's stream, on the owner's stream); owners x members
    /// copies of count / members x D / owners elements each.  Each owner then sends its leaves to the host over its own link while the
    /// caller hashes.  The coefficient forms the extension leaves behind are gathered on member 0 for proof_eval.
    void commit_group(std::size_t index, const std::vector<const poly_type *> &polys, const device_batch &db, const root_map &roots) {
        const device_group &group = *_group;
        const std::size_t D = domain_size(0), count = polys.size(), world = group.size(), step = _fri_params.step_list.front();
        std::size_t log_owners = 0;    // owners: a power of two (the compact domain is one), every owner with at least one leaf
        while (((std::size_t)2 << log_owners) <= world && _fri_params.log_domain >= step + log_owners + 1) ++log_owners;
        const std::size_t owners = (std::size_t)1 << log_owners, Ds = D >> log_owners, seg = Ds >> step, rows_per_poly = (std::size_t)1 << step;
        std::vector<detail::group_part> parts(world);
        for (std::size_t k = 0; k < world; ++k) {
            member_scratch &gs = _scratch[k];
            if (k < owners) {
                gs.cmp.reserve(group[k], count * Ds * 32);
                gs.leaves.reserve(group[k], count * Ds * 32);
            }
            const detail::group_part &pt = parts[k] = detail::deal_columns(db, group, k);
            if (pt.empty()) continue;
            gs.ext.reserve(group[k], (pt.hi - pt.lo) * D * 32);
            gs.send.reserve(group[k], (pt.hi - pt.lo) * D * 32);    // owners blocks of (hi - lo) * Ds
        }
        group.for_each_member([&](std::size_t k) {
            const detail::group_part &pt = parts[k];
            if (pt.empty()) return;
            const context &ctx = group[k];
            member_scratch &gs = _scratch[k];
            const std::size_t mine = pt.hi - pt.lo;
            char *d_ext = static_cast<char *>(gs.ext.get());
            extend_columns(polys, db, pt.lo, pt.hi, pt.base, ctx, k, d_ext, roots);
            /* per owner: the 2^step segments [d seg + j D / 2^step, + seg) of each of my polynomials, side by side (rows of seg elements at a
               pitch of D / 2^step in, seg out) -- straight into my own buffer where I am the owner */
            for (std::size_t d = 0; d < owners; ++d) {
                char *dst = d == k ? static_cast<char *>(gs.cmp.get()) + 32 * pt.lo * Ds : static_cast<char *>(gs.send.get()) + 32 * d * mine * Ds;
                ZKHIP_CALL(ctx, zkhip_memcpy_2d_d2d_async, dst, seg * 32, d_ext + 32 * d * seg, (D >> step) * 32, seg * 32, mine * rows_per_poly);
            }
        });
        /* the exchange, from this thread: blocks to their owners, coefficient forms to member 0 */
        for (std::size_t k = 0; k < world; ++k) {
            const detail::group_part &pt = parts[k];
            if (pt.empty()) continue;
            const std::size_t mine = pt.hi - pt.lo;
            for (std::size_t d = 0; d < owners; ++d)
                if (d != k)
                    group.copy(d, static_cast<char *>(_scratch[d].cmp.get()) + 32 * pt.lo * Ds, k, static_cast<const char *>(_scratch[k].send.get()) + 32 * d * mine * Ds,
                               mine * Ds * 32);
            detail::gather_form(db, group, k, pt);
        }
        std::vector<leaf_block> blocks;
        for (std::size_t d = 0; d < owners; ++d) {
            ZKHIP_CALL(group[d], zkhip_fri_leaves_dev, _scratch[d].cmp.get(), _fri_params.log_domain - log_owners, count, step, _scratch[d].leaves.get());
            blocks.push_back({group[d], _scratch[d].leaves.get(), _scratch[d]});
        }
        _trees.erase(index);
        _trees.emplace(index, deliver_leaves(blocks, count * Ds, count * rows_per_poly));
        group.sync();    // the members' own coefficient buffers go with `parts`: every copy out of them has finished
        ++_group_commits;
        _last_owners = owners;
    }

public:
    /// proof_eval (lpc.hpp:113-200) up to and including the FRI commit phase (basic_fri.hpp:705-742) and the grinding behind it (:743-745)
    proof_type proof_eval(transcript_type &transcript) {
        /* ZKHIP_LPC_PHASES=1: host wall time of the phases on stderr */
        const bool phases = std::getenv("ZKHIP_LPC_PHASES") != nullptr;
        auto tp = std::chrono::steady_clock::now();
        auto lap = [&](const char *what) {
            if (!phases) return;
            _ctx.sync();
            const auto now = std::chrono::steady_clock::now();
            std::fprintf(stderr, "lpc proof_eval phase %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - tp).count());
            tp = now;
        };
        this->eval_polys();
        lap("eval_polys");
        for (const auto &it : _trees) transcript(it.second.root());

        /* Prepare z-s and combined_Q (lpc.hpp:124-186), coefficient form, resident */
        const value_type theta = transcript.challenge();
        value_type theta_acc = value_type::one();
        std::size_t max_len = 1;
        for (const auto &it : _dev)
            for (std::size_t l : it.second.len) max_len = std::max(max_len, l);
        auto d_combined = _ctx.alloc(max_len * 32), d_q = _ctx.alloc(max_len * 32);
        bool have_combined = false;
        auto add_quotient = [&](const std::vector<const void *> &ptrs, const std::vector<std::size_t> &lens, const std::vector<value_type> &coeffs,
                                const value_type &constant, const value_type &point) {
            if (ptrs.empty()) return;
            /* Q_normal = sum theta_acc g - sum theta_acc z;  Q_normal /= (X - point);  combined_Q_normal += Q_normal */
            fv::lincomb(_ctx, ptrs, lens, coeffs, 1, d_q.get(), max_len, false);
            auto d_c = _ctx.alloc(32);
            _ctx.h2d(d_c.get(), limbs_of<adapter>(value_type::zero() - constant).data(), 32);
            fv::pointwise(_ctx, fr_op::add, d_q.get(), d_c.get(), d_q.get(), 1);
            if (!(fv::div_linear(_ctx, d_q.get(), max_len, point, d_q.get()) == value_type::zero()))
                throw std::runtime_error("lpc proof_eval: a quotient does not divide (evaluation / point mismatch)");
            /* the quotient's max_len - 1 coefficients sit at d_q + 1; slot 0 held the (zero) remainder */
            void *q = static_cast<char *>(d_q.get()) + 32;
            if (!have_combined) {
                fv::copy(_ctx, d_combined.get(), q, max_len - 1);
                have_combined = true;
            } else if (max_len > 1) {
                fv::pointwise(_ctx, fr_op::add, d_combined.get(), q, d_combined.get(), max_len - 1);
            }
            _ctx.sync();    // d_c is released on return
        };
        for (const auto &point : this->unique_points()) {
            std::vector<const void *> ptrs;
            std::vector<std::size_t> lens;
            std::vector<value_type> coeffs;
            value_type constant = value_type::zero();
            for (std::size_t i : _z.get_batches()) {
                for (std::size_t j = 0; j < _z.get_batch_size(i); ++j) {
                    const auto &pts = _points.at(i)[j];
                    auto it = std::find(pts.begin(), pts.end(), point);
                    if (it == pts.end()) continue;
                    ptrs.push_back(_dev.at(i).at(j));
                    lens.push_back(_dev.at(i).len[j]);
                    coeffs.push_back(theta_acc);
                    constant = constant + _z.get(i, j, it - pts.begin()) * theta_acc;
                    theta_acc = theta_acc * theta;
                }
            }
            add_quotient(ptrs, lens, coeffs, constant, point);
        }
        for (std::size_t i : _z.get_batches()) {    // the fixed batches at etha (lpc.hpp:164-186)
            auto fx = _batch_fixed.find(i);
            if (fx == _batch_fixed.end() || !fx->second) continue;
            std::vector<const void *> ptrs;
            std::vector<std::size_t> lens;
            std::vector<value_type> coeffs;
            value_type constant = value_type::zero();
            for (std::size_t j = 0; j < _z.get_batch_size(i); ++j) {
                ptrs.push_back(_dev.at(i).at(j));
                lens.push_back(_dev.at(i).len[j]);
                coeffs.push_back(theta_acc);
                constant = constant + _fixed_polys_values.at(i).at(j) * theta_acc;
                theta_acc = theta_acc * theta;
            }
            add_quotient(ptrs, lens, coeffs, constant, _etha);
        }
        if (!have_combined) throw std::runtime_error("lpc proof_eval: nothing to open");
        lap("combined quotient");

        /* combined_Q.from_coefficients + precommit(combined_Q, D[0], step_list.front()) (lpc.hpp:188-198): the extension to
           D[0] is the NTT of the zero-padded coefficients */
        const std::size_t D0 = domain_size(0);
        device_polynomial_dfs<CurveType> f(_ctx, D0);
        /* the zero-padded copy in one pass on the device: f[j] = 1 * combined[j] below max_len - 1, zero behind (one term even when
           max_len - 1 == 0, which zero_padded_copy would pass as none) */
        fv::add_scaled(_ctx, d_combined.get(), max_len - 1, value_type::one(), f.data(), D0, false);
        fv::ntt(_ctx, f.data(), _fri_params.log_domain, 1, _fri_params.root_of_unity(_fri_params.log_domain), false);
        lap("extension to D[0]");
        precommitment_type precommitment = [&]() {
            ZKHIP_PROFILE_SCOPE("Basic FRI Precommit time");    // precommit(combined_Q, ...), lpc.hpp:196-198
            return build_tree(f.data(), 1, _fri_params.log_domain, _fri_params.step_list.front());
        }();

        lap("precommit (leaves of round 0)");
        /* Commit phase (basic_fri.hpp:705-742) */
        proof_type proof;
        _fri_trees.clear();
        _fs.clear();
        _alphas.clear();
        std::size_t t = 0;
        for (std::size_t i = 0; i < _fri_params.step_list.size(); ++i) {
            _fs.push_back(f);
            _fri_trees.push_back(precommitment);
            proof.fri_proof.fri_roots.push_back(precommitment.root());
            transcript(precommitment.root());
            for (std::size_t step_i = 0; step_i < _fri_params.step_list[i]; ++step_i, ++t) {
                _alphas.push_back(transcript.challenge());
                f = fold_polynomial<CurveType>(f, _alphas[t], _fri_params.root_of_unity(_fri_params.log_domain - t));
            }
            if (i != _fri_params.step_list.size() - 1)
                precommitment = build_tree(f.data(), 1, _fri_params.log_domain - t, _fri_params.step_list[i + 1]);
        }
        _fs.push_back(f);
        lap("fold rounds + their leaves");
        {
            auto d_c = f.coefficients(_fri_params.root_of_unity);
            std::vector<std::uint64_t> h(4 * f.size());
            _ctx.d2h(h.data(), d_c.get(), h.size() * 8);
            for (std::size_t k = 0; k < f.size(); ++k) proof.fri_proof.final_polynomial.push_back(adapter::scalar_from_limbs(&h[4 * k]));
        }
        if (_fri_params.use_grinding) {    // Grinding (basic_fri.hpp:743-745); over a device group _ctx is member 0
            if constexpr (detail::has_state<transcript_type>::value) {
                proof.fri_proof.proof_of_work = proof_of_work_hip<transcript_type>::generate(_ctx, transcript, _fri_params.grinding_parameter);
                lap("grinding");
            } else {
                throw std::invalid_argument("lpc proof_eval: use_grinding needs a transcript with state() (hip/transcript.hpp)");
            }
        }
        proof.z = _z;
        return proof;
    }

    /// The query phase of proof_eval<FRI> (basic_fri.hpp:747-930), after proof_eval on this object (which still holds the round polynomials,
    /// the trees and the coefficient forms): fills proof.fri_proof.query_proofs with fri_params.lambda query proofs.  All lambda challenges
    /// are drawn first -- the reference draws one per query and absorbs nothing in between, so the transcript sees the same calls in the same
    /// order -- and the device answers all queries together:
    ///   per committed batch, in map order: its polynomials re-extended to D[0] from the resident coefficient forms into the commit's scratch
    ///     (a zero-padded copy per polynomial, one batched NTT), then ONE zkhip_fri_query_dev over them;
    ///   ONE zkhip_merkle_paths_multi over the batch trees;  ONE zkhip_fri_query_dev over fs[i + 1] of every round but the last;  ONE
    ///     zkhip_merkle_paths_multi over the round trees (a host tree answers through proof(i) instead);
    ///   the last round's y: the final polynomial at +-x^2, on the host.
    /// Refuses (std::invalid_argument, the transcript untouched): lambda == 0, a step list that does not end in 1 (check_step_list, :566), no
    /// proof_eval before.  A challenge that does not map into D[0] (c = 0) throws std::runtime_error.
    void query_phase(transcript_type &transcript, proof_type &proof) {
        static_assert(builder_kind == detail::tree_builder_kind::device || detail::has_proof<precommitment_type>::value,
                      "lpc query_phase: the host tree builder's tree has no proof(std::size_t) to open a leaf with");
        const std::vector<std::size_t> &steps = _fri_params.step_list;
        const std::size_t lambda = _fri_params.lambda, n = _fri_params.log_domain, R = steps.size();
        if (lambda == 0) throw std::invalid_argument("lpc query_phase: fri_params.lambda is 0");
        if (steps.empty() || steps.back() != 1) throw std::invalid_argument("lpc query_phase: the step list must end in 1");
        if (_fs.size() != R + 1 || _fri_trees.size() != R || proof.fri_proof.final_polynomial.empty())
            throw std::invalid_argument("lpc query_phase: proof_eval has not run on this scheme object");
        typedef std::chrono::steady_clock clock;
        query_phase_times times;
        auto tp = clock::now();
        auto lap = [&](double &slot) {
            if (!_time_query_phase) return;
            const auto now = clock::now();
            slot += std::chrono::duration<double, std::milli>(now - tp).count();
            tp = now;
        };

        /* x = challenge^((r - 1) / |D[0]|) and its index in D[0] (basic_fri.hpp:779-786) */
        std::uint64_t e[4];
        cofactor_exponent(e);
        std::vector<std::uint64_t> xi(lambda);
        for (std::size_t q = 0; q < lambda; ++q) xi[q] = detail::domain_index(detail::pow_limbs(transcript.challenge(), e), n, _fri_params.root_of_unity);
        std::vector<query_proof_type> &qps = proof.fri_proof.query_proofs;
        qps.assign(lambda, query_proof_type());
        lap(times.host_ms);

        /* Initial proofs (:793-861): the values of every committed polynomial over D[0] at the pairs calculate_s walks from x */
        const std::size_t D0 = domain_size(0), pairs0 = (std::size_t)1 << (steps[0] - 1);
        const value_type w0 = _fri_params.root_of_unity(n);
        std::vector<std::uint64_t> answers;
        for (const auto &it : _dev) {
            const device_batch &db = it.second;
            const std::size_t count = db.len.size();
            for (std::size_t q = 0; q < lambda; ++q) qps[q].initial_proof[it.first].values.assign(count, std::vector<std::array<value_type, 2>>(pairs0));
            if (count == 0) continue;
            /* member 0's extension buffer, which commit_group fills too: both on member 0's stream, and reserve() drains it before it reallocates */
            char *d_ext = static_cast<char *>(_scratch[0].ext.reserve(_ctx, count * D0 * 32));
            for (std::size_t p = 0; p < count; ++p) fv::zero_padded_copy(_ctx, db.at(p), db.len[p], d_ext + 32 * p * D0, D0);    // len >= 1: commit refuses less
            fv::ntt(_ctx, d_ext, n, count, w0, false);
            if (_time_query_phase) _ctx.sync();
            lap(times.reextend_ms);
            const zkhip_fri_query_set set = {d_ext, n, count, steps[0]};
            answers.resize(4 * lambda * (count << steps[0]));
            ZKHIP_CALL(_ctx, zkhip_fri_query_dev, &set, 1, xi.data(), lambda, answers.data());
            lap(times.gather_ms);
            const std::uint64_t *at = answers.data();
            for (std::size_t q = 0; q < lambda; ++q) {
                auto &values = qps[q].initial_proof[it.first].values;
                for (std::size_t p = 0; p < count; ++p)
                    for (std::size_t j = 0; j < pairs0; ++j, at += 8) values[p][j] = {adapter::scalar_from_limbs(at), adapter::scalar_from_limbs(at + 4)};
            }
            lap(times.host_ms);
        }
        {    /* the paths of leaf x mod (|D[0]| / 2^step_list[0]) in every batch tree (:857-860) */
            std::vector<const precommitment_type *> trees;
            for (const auto &it : _trees) trees.push_back(&it.second);
            auto paths = open_paths(trees, std::vector<std::size_t>(trees.size(), n - steps[0]), xi);
            std::size_t t = 0;
            for (const auto &it : _trees) {
                for (std::size_t q = 0; q < lambda; ++q) qps[q].initial_proof[it.first].p = std::move(paths[t][q]);
                ++t;
            }
            lap(times.paths_ms);
        }

        /* Round proofs (:863-920): y of round i is fs[i + 1] at the pairs walked from x mod |D[t_(i+1)]| */
        for (std::size_t q = 0; q < lambda; ++q) qps[q].round_proofs.assign(R, round_proof_type());
        if (R > 1) {
            std::vector<zkhip_fri_query_set> sets;
            std::size_t t = steps[0], elements = 0;
            const std::size_t log_first = n - t;    // the largest domain among the sets: the indices go in reduced to it
            for (std::size_t i = 0; i + 1 < R; ++i) {
                sets.push_back({_fs[i + 1].data(), n - t, 1, steps[i + 1]});
                elements += (std::size_t)1 << steps[i + 1];
                t += steps[i + 1];
            }
            std::vector<std::uint64_t> xr(lambda);
            for (std::size_t q = 0; q < lambda; ++q) xr[q] = xi[q] & (((std::uint64_t)1 << log_first) - 1);
            answers.resize(4 * lambda * elements);
            ZKHIP_CALL(_ctx, zkhip_fri_query_dev, sets.data(), sets.size(), xr.data(), lambda, answers.data());
            lap(times.gather_ms);
            const std::uint64_t *at = answers.data();
            for (std::size_t i = 0; i + 1 < R; ++i)
                for (std::size_t q = 0; q < lambda; ++q) {
                    auto &y = qps[q].round_proofs[i].y;
                    y.resize((std::size_t)1 << (steps[i + 1] - 1));
                    for (auto &pair : y) {
                        pair = {adapter::scalar_from_limbs(at), adapter::scalar_from_limbs(at + 4)};
                        at += 8;
                    }
                }
            lap(times.host_ms);
        }
        {    /* the paths of leaf x mod (|D[t_i]| / 2^step_list[i]) in the tree of round i (:868-874) */
            std::vector<const precommitment_type *> trees;
            std::vector<std::size_t> log_leaves;
            std::size_t t = 0;
            for (std::size_t i = 0; i < R; t += steps[i], ++i) {
                trees.push_back(&_fri_trees[i]);
                log_leaves.push_back(n - t - steps[i]);
            }
            auto paths = open_paths(trees, log_leaves, xi);
            for (std::size_t i = 0; i < R; ++i)
                for (std::size_t q = 0; q < lambda; ++q) qps[q].round_proofs[i].p = std::move(paths[i][q]);
            lap(times.paths_ms);
        }
        {    /* the last round (:904-918): the final polynomial at x^2 and -x^2, x over the last round's domain, in the order the next round
                -- of step 1 -- would hold them */
            std::size_t r = 0;
            for (std::size_t s : steps) r += s;
            const std::size_t log_last = n - (r - 1), N = (std::size_t)1 << log_last;
            const value_type w = _fri_params.root_of_unity(log_last);
            for (std::size_t q = 0; q < lambda; ++q) {
                const std::size_t x_index = xi[q] & (N - 1);
                const value_type x = detail::pow_index(w, x_index), x2 = x * x;
                const std::size_t ind = (x_index % (N / 2) < N / 4) ? 0 : 1;
                auto &y = qps[q].round_proofs[R - 1].y;
                y.resize(1);
                y[0][ind] = horner(proof.fri_proof.final_polynomial, x2);
                y[0][1 - ind] = horner(proof.fri_proof.final_polynomial, value_type::zero() - x2);
            }
            lap(times.host_ms);
        }
        _last_query_times = times;
    }

    /// a whole opening proof: proof_eval, then query_phase
    proof_type proof_eval_full(transcript_type &transcript) {
        proof_type proof = proof_eval(transcript);
        query_phase(transcript, proof);
        return proof;
    }

    /// verify_eval (lpc.hpp:202-300 over basic_fri.hpp:933-1154), in this shim's own words; host only, nothing is launched.  The verifier's
    /// scheme object knows what the prover's knew: the evaluation points of every polynomial (set_batch_size + append_eval_point[s]), the fixed
    /// batches (mark_batch_as_fixed) and their values at etha (setup).  Per query it checks
    ///   the initial values against the batch roots (the leaf is the answered pairs in leaf order, hashed by include/zkhip.h's convention),
    ///   the combined quotient they imply -- sum over the opening points of (sum theta^k g_k - U) / (X - point), as proof_eval builds it --
    ///     against the first round's root,
    ///   every round: the y values against the round's root, their fold with the round's alphas against the next round's y,
    ///   the last y against the final polynomial at +-x^2;
    /// before that the shape of the proof, the low-degree bound on the final polynomial (basic_fri.hpp:949-952: its degree, trailing zero
    /// coefficients aside, is at most 2^(log2(max_degree + 1) - r + 1) - 1 -- without it a final polynomial as long as the last domain would
    /// interpolate anything) and, with use_grinding, the proof of work.  Refuses (std::invalid_argument, before the transcript is touched)
    /// lambda == 0, a step list that does not end in 1, and an unset fri_params.max_degree: there is no verifying without a degree bound.
    /// It reads what a verifier has -- the parameters, the points, etha and the fixed values -- and nothing the prover's calls left behind.
    /// Built for the device builder's instantiation: its leaf and node convention is the one include/zkhip.h states.
    bool verify_eval(const proof_type &proof, const std::map<std::size_t, commitment_type> &commitments, transcript_type &transcript) const {
        static_assert(builder_kind == detail::tree_builder_kind::device,
                      "lpc verify_eval: built for the device tree builder, whose leaf and node hashing include/zkhip.h states");
        const std::vector<std::size_t> &steps = _fri_params.step_list;
        const std::size_t lambda = _fri_params.lambda, n = _fri_params.log_domain, R = steps.size();
        if (lambda == 0) throw std::invalid_argument("lpc verify_eval: fri_params.lambda is 0");
        if (steps.empty() || steps.back() != 1) throw std::invalid_argument("lpc verify_eval: the step list must end in 1");
        if (_fri_params.max_degree == 0) throw std::invalid_argument("lpc verify_eval: fri_params.max_degree is not set: there is no degree bound to verify against");
        std::size_t r = 0;
        for (std::size_t s : steps) r += s;
        const eval_storage_type &z = proof.z;
        const fri_proof_type &fp = proof.fri_proof;

        for (const auto &it : commitments) transcript(it.second);
        const value_type theta = transcript.challenge();

        /* what is opened where (lpc.hpp:212-252): per opening point the polynomials that have it, and U = sum theta^k z_k */
        struct opening {
            value_type point, U, theta0;    // theta0: the running power of theta at the opening's first polynomial
            std::vector<std::pair<std::size_t, std::size_t>> polys;
        };
        std::vector<opening> openings;
        value_type theta_acc = value_type::one();
        for (std::size_t i : z.get_batches()) {
            auto pt = _points.find(i);
            if (!commitments.count(i) || pt == _points.end() || pt->second.size() != z.get_batch_size(i)) return false;
            for (std::size_t j = 0; j < z.get_batch_size(i); ++j)
                if (z.get_poly_points_number(i, j) != pt->second[j].size()) return false;
        }
        for (const auto &point : this->unique_points()) {
            opening o {point, value_type::zero(), theta_acc, {}};
            for (std::size_t i : z.get_batches())
                for (std::size_t j = 0; j < z.get_batch_size(i); ++j) {
                    const auto &pts = _points.at(i)[j];
                    auto it = std::find(pts.begin(), pts.end(), point);
                    if (it == pts.end()) continue;
                    o.U = o.U + z.get(i, j, it - pts.begin()) * theta_acc;
                    o.polys.emplace_back(i, j);
                    theta_acc = theta_acc * theta;
                }
            if (!o.polys.empty()) openings.push_back(std::move(o));
        }
        for (std::size_t i : z.get_batches()) {    // the fixed batches at etha (lpc.hpp:241-252), batch by batch as proof_eval adds them
            auto fx = _batch_fixed.find(i);
            if (fx == _batch_fixed.end() || !fx->second) continue;
            auto fv = _fixed_polys_values.find(i);
            if (fv == _fixed_polys_values.end() || fv->second.size() != z.get_batch_size(i)) return false;
            opening o {_etha, value_type::zero(), theta_acc, {}};
            for (std::size_t j = 0; j < z.get_batch_size(i); ++j) {
                o.U = o.U + fv->second[j] * theta_acc;
                o.polys.emplace_back(i, j);
                theta_acc = theta_acc * theta;
            }
            if (!o.polys.empty()) openings.push_back(std::move(o));
        }
        if (openings.empty()) return false;

        /* the shape of the FRI proof, its roots and alphas (basic_fri.hpp:949-962), the proof of work (:964-966) */
        if (fp.fri_roots.size() != R || fp.query_proofs.size() != lambda || fp.final_polynomial.empty() ||
            fp.final_polynomial.size() > ((std::size_t)1 << (n - r)))
            return false;
        {   /* the low-degree bound (basic_fri.hpp:949-952): degree(final) <= 2^(log2(max_degree + 1) - r + 1) - 1, that is
               (degree + 1) 2^r <= 2 (max_degree + 1); the degree is that of the highest non-zero coefficient */
            std::size_t degree = fp.final_polynomial.size() - 1;
            while (degree > 0 && fp.final_polynomial[degree] == value_type::zero()) --degree;
            if (degree + 1 > ((_fri_params.max_degree + 1) >> (r - 1))) return false;    // r >= 1: the step list is not empty
        }
        std::vector<value_type> alphas;
        for (std::size_t i = 0; i < R; ++i) {
            transcript(fp.fri_roots[i]);
            for (std::size_t s = 0; s < steps[i]; ++s) alphas.push_back(transcript.challenge());
        }
        if (_fri_params.use_grinding) {
            if constexpr (detail::has_state<transcript_type>::value) {
                if (!proof_of_work_hip<transcript_type>::verify(transcript, fp.proof_of_work, _fri_params.grinding_parameter)) return false;
            } else {
                throw std::invalid_argument("lpc verify_eval: use_grinding needs a transcript with state() (hip/transcript.hpp)");
            }
        }

        std::uint64_t e[4];
        cofactor_exponent(e);
        const value_type w0 = _fri_params.root_of_unity(n), half = (value_type::one() + value_type::one()).inversed();
        for (std::size_t q = 0; q < lambda; ++q) {
            const query_proof_type &qp = fp.query_proofs[q];
            const std::size_t x_index = detail::domain_index(detail::pow_limbs(transcript.challenge(), e), n, _fri_params.root_of_unity);
            if (qp.round_proofs.size() != R || qp.initial_proof.size() != commitments.size()) return false;

            /* initial proofs (:987-1006) */
            const std::size_t pairs0 = (std::size_t)1 << (steps[0] - 1);
            const std::vector<std::size_t> pos0 = detail::pair_positions(x_index, n, steps[0]);
            for (const auto &it : qp.initial_proof) {
                auto root = commitments.find(it.first);
                if (root == commitments.end()) return false;
                const initial_proof_type &ip = it.second;
                for (const auto &v : ip.values)
                    if (v.size() != pairs0) return false;
                std::vector<const std::vector<std::array<value_type, 2>> *> rows;
                for (const auto &v : ip.values) rows.push_back(&v);
                if (!leaf_opens(rows, x_index, n, steps[0], ip.p, root->second)) return false;
            }
            /* the combined quotient at the same pairs (:1008-1038) */
            std::vector<std::array<value_type, 2>> y(pairs0, {value_type::zero(), value_type::zero()});
            for (const opening &o : openings)
                for (std::size_t j = 0; j < pairs0; ++j)
                    for (std::size_t side = 0; side < 2; ++side) {
                        value_type acc = value_type::zero(), th = o.theta0;
                        for (std::size_t k = 0; k < o.polys.size(); ++k) {
                            auto ip = qp.initial_proof.find(o.polys[k].first);
                            if (ip == qp.initial_proof.end() || o.polys[k].second >= ip->second.values.size()) return false;
                            acc = acc + ip->second.values[o.polys[k].second][j][side] * th;
                            th = th * theta;
                        }
                        const value_type denominator = detail::pow_index(w0, pos0[j] + side * (domain_size(0) / 2)) - o.point;
                        if (denominator == value_type::zero()) return false;
                        y[j][side] = y[j][side] + (acc - o.U) * denominator.inversed();
                    }

            /* round proofs (:1039-1139): the y of round i open its tree, fold to one value, and that value stands in the next y */
            std::size_t t = 0;
            for (std::size_t i = 0; i < R; ++i) {
                const std::size_t log_n = n - t, N = (std::size_t)1 << log_n, xr = x_index & (N - 1);
                if (y.size() != ((std::size_t)1 << (steps[i] - 1))) return false;
                if (!leaf_opens({&y}, xr, log_n, steps[i], qp.round_proofs[i].p, fp.fri_roots[i])) return false;
                std::map<std::size_t, value_type> cur;    // position in the current domain -> value
                const std::vector<std::size_t> pos = detail::pair_positions(xr, log_n, steps[i]);
                for (std::size_t j = 0; j < y.size(); ++j) {
                    cur[pos[j]] = y[j][0];
                    cur[pos[j] + N / 2] = y[j][1];
                }
                for (std::size_t s = 0; s < steps[i]; ++s, ++t) {    // fold_polynomial (fold_polynomial.hpp:68-93) on the positions held
                    const std::size_t M = (std::size_t)1 << (n - t);
                    const value_type w = _fri_params.root_of_unity(n - t);
                    std::map<std::size_t, value_type> next;
                    for (const auto &pv : cur) {
                        if (pv.first >= M / 2) break;
                        auto hi = cur.find(pv.first + M / 2);
                        if (hi == cur.end()) return false;
                        const value_type aw = alphas[t] * detail::pow_index(w, (M - pv.first) & (M - 1));    // alpha w^-p
                        next[pv.first] = half * ((value_type::one() + aw) * pv.second + (value_type::one() - aw) * hi->second);
                    }
                    cur.swap(next);
                }
                if (cur.size() != 1) return false;
                const std::size_t Nn = (std::size_t)1 << (n - t), xn = x_index & (Nn - 1);    // the next domain and x's index in it
                if (cur.begin()->first != (xn & ((N >> steps[i]) - 1))) return false;
                y = qp.round_proofs[i].y;
                const std::size_t expect = i + 1 < R ? (std::size_t)1 << (steps[i + 1] - 1) : 1;
                if (y.size() != expect) return false;
                if (!(y[0][xn < Nn / 2 ? 0 : 1] == cur.begin()->second)) return false;
            }
            /* the final polynomial (:1141-1151) */
            {
                const std::size_t log_last = n - (r - 1), N = (std::size_t)1 << log_last, xl = x_index & (N - 1);
                const value_type x = detail::pow_index(_fri_params.root_of_unity(log_last), xl), x2 = x * x;
                const std::size_t ind = (xl % (N / 2) < N / 4) ? 0 : 1;
                if (!(y[0][ind] == horner(fp.final_polynomial, x2))) return false;
                if (!(y[0][1 - ind] == horner(fp.final_polynomial, value_type::zero() - x2))) return false;
            }
        }
        return true;
    }

    // ---- what the caller's query phase reads (basic_fri.hpp:747-930) ----
    const std::map<std::size_t, precommitment_type> &trees() const { return _trees; }
    const std::vector<precommitment_type> &fri_trees() const { return _fri_trees; }
    const std::vector<value_type> &fri_alphas() const { return _alphas; }
    /// fs[i] of the commit phase (i <= step_list.size()): the round polynomials, evaluations over their domains
    polynomial_dfs<CurveType> fri_round_polynomial(std::size_t i) const { return _fs.at(i).to_host(); }
    /// coefficient form of committed polynomial (batch, index): `g_coeffs` of the query phase (basic_fri.hpp:753-771)
    std::vector<value_type> coefficients(std::size_t batch, std::size_t index) const {
        const device_batch &db = _dev.at(batch);
        std::vector<value_type> out;
        download_scalars<adapter>(_ctx, db.at(index), db.len.at(index), out);
        return out;
    }

protected:
    std::size_t domain_size(std::size_t t) const { return (std::size_t)1 << (_fri_params.log_domain - t); }
    /// (r - 1) / |D[0]|, the exponent that takes a challenge into D[0] (basic_fri.hpp:780, 973); r is odd and |D[0]| divides r - 1
    void cofactor_exponent(std::uint64_t *e) const {
        adapter::scalar_modulus(e);
        e[0] -= 1;
        const std::size_t n = _fri_params.log_domain, limbs = n / 64, bits = n % 64;
        for (std::size_t k = 0; k < 4; ++k) {
            const std::uint64_t lo = k + limbs < 4 ? e[k + limbs] : 0, hi = k + limbs + 1 < 4 ? e[k + limbs + 1] : 0;
            e[k] = bits ? (lo >> bits) | (hi << (64 - bits)) : lo;
        }
    }
    /// math::polynomial::evaluate over a coefficient vector
    static value_type horner(const std::vector<value_type> &coefficients, const value_type &x) {
        value_type acc = value_type::zero();
        for (std::size_t k = coefficients.size(); k-- > 0;) acc = acc * x + coefficients[k];
        return acc;
    }
    /// the paths of leaf (x mod 2^log_leaves[t]) of tree t for every query: out[t][q].  Device trees answer all of it in one pass
    /// (zkhip_merkle_paths_multi reduces the index by the tree's own leaf count, which is 2^log_leaves[t]); a host tree is asked leaf by leaf.
    std::vector<std::vector<merkle_path_type>> open_paths(const std::vector<const precommitment_type *> &trees, const std::vector<std::size_t> &log_leaves,
                                                          const std::vector<std::uint64_t> &xi) const {
        if constexpr (builder_kind == detail::tree_builder_kind::device) {
            return precommitment_type::paths_multi(_ctx, trees, xi);
        } else {
            std::vector<std::vector<merkle_path_type>> out(trees.size());
            for (std::size_t t = 0; t < trees.size(); ++t)
                for (std::uint64_t x : xi) out[t].push_back(trees[t]->proof((std::size_t)(x & (((std::uint64_t)1 << log_leaves[t]) - 1))));
            return out;
        }
    }
    /// verify_eval's Merkle check: `rows` (one per polynomial) hold the pairs answered for x over the 2^log_n-point domain in calculate_s's
    /// order; put into the leaf's own order (get_correct_order, basic_fri.hpp:616-663: the walk from the leaf index instead of x), encoded and
    /// hashed as include/zkhip.h states, they must lead to `root` along `path`
    bool leaf_opens(const std::vector<const std::vector<std::array<value_type, 2>> *> &rows, std::size_t x, std::size_t log_n, std::size_t fri_step,
                    const merkle_path_type &path, const commitment_type &root) const {
        const std::size_t leaf = x & (((std::size_t)1 << (log_n - fri_step)) - 1);
        if (path.leaf_index != leaf || path.siblings.size() != log_n - fri_step) return false;
        const std::vector<std::size_t> asked = detail::pair_positions(x, log_n, fri_step), ordered = detail::pair_positions(leaf, log_n, fri_step);
        std::vector<std::uint8_t> bytes;
        for (const auto *row : rows) {
            if (row->size() != asked.size()) return false;
            for (std::size_t position : ordered) {
                const std::size_t j = std::find(asked.begin(), asked.end(), position) - asked.begin();
                if (j == asked.size()) return false;
                for (const value_type &v : (*row)[j]) {
                    std::uint64_t limbs[4];
                    adapter::scalar_to_limbs(v, limbs);
                    for (int k = 3; k >= 0; --k)
                        for (int b = 7; b >= 0; --b) bytes.push_back(std::uint8_t(limbs[k] >> (8 * b)));    // the canonical integer, big-endian
                }
            }
        }
        commitment_type digest;
        check(zkhip_sha256_host(bytes.data(), bytes.size(), digest.data()), "zkhip_sha256_host");
        return path.root_from(digest) == root;
    }
    /// What a member keeps across commits: the extensions of its columns, the blocks it sends, an owner's compact evaluations and its leaves,
    /// and the two page-locked buffers its leaves cross PCIe through.  Entry 0 is the lone context's (over a group: member 0's) and serves the
    /// lone commit, proof_eval's round trees and query_phase's re-extension too: outside commit_group's member lambda every use of it is
    /// enqueued on that context's stream from the calling thread, commit_group ends in group.sync(), and device_scratch::reserve drains the
    /// stream before it reallocates.
    struct member_scratch {
        device_scratch ext, send, cmp, leaves;
        pinned_buffer pin[2];
    };
    /// `block` laid-out leaf elements at `d_leaves` on `ctx`, the scratch entry of that member
    struct leaf_block {
        const context &ctx;
        const void *d_leaves;
        member_scratch &scratch;
    };
    /// the leaf layout of `batch` polynomials resident as evaluations over the 2^log_domain-point domain -> the caller's tree; a device
    /// builder takes the evaluations as they lie: no leaf layout, no copy to the host
    precommitment_type build_tree(const void *d_evals, std::size_t batch, std::size_t log_domain, std::size_t fri_step) const {
        if constexpr (builder_kind == detail::tree_builder_kind::device) return _builder(_ctx, d_evals, batch, log_domain, fri_step);
        else {
            const std::size_t total = batch << log_domain;
            void *d_leaves = _scratch[0].leaves.reserve(_ctx, std::max<std::size_t>(1, total) * 32);
            ZKHIP_CALL(_ctx, zkhip_fri_leaves_dev, d_evals, log_domain, batch, fri_step, d_leaves);
            return deliver_leaves({{_ctx, d_leaves, _scratch[0]}}, total, batch << fri_step);
        }
    }
    /// The host builder's tree from leaves that lie in consecutive blocks of `block` elements (`per_leaf` to a leaf), block d on blocks[d].ctx:
    /// the one block of a lone context, or the leaf owners' of a group.  Nothing below depends on which.
    precommitment_type deliver_leaves(const std::vector<leaf_block> &blocks, std::size_t block, std::size_t per_leaf) const {
        const std::size_t total = blocks.size() * block;
        if constexpr (builder_kind == detail::tree_builder_kind::streaming) {
            /* slices of whole leaves through two page-locked buffers per block: every block's first slice is requested at once, then the blocks
               are absorbed in leaf order, the copy of a block's slice k + 1 in flight on its own link while the caller absorbs slice k */
            const std::size_t leaf = std::max<std::size_t>(1, per_leaf), slice = std::max<std::size_t>(1, (leaf_slice_elements + leaf - 1) / leaf) * leaf;
            const std::size_t first = std::min(slice, block);
            _builder.begin(total, per_leaf);
            if (total != 0) {
                for (const leaf_block &b : blocks) {
                    void *p0 = b.scratch.pin[0].reserve(b.ctx, first * 32);
                    b.scratch.pin[1].reserve(b.ctx, first * 32);
                    b.ctx.d2h_async(p0, b.d_leaves, first * 32);
                }
                for (std::size_t d = 0; d < blocks.size(); ++d) {
                    const leaf_block &b = blocks[d];
                    const char *src = static_cast<const char *>(b.d_leaves);
                    void *pin[2] = {b.scratch.pin[0].get(), b.scratch.pin[1].get()};
                    b.ctx.sync();
                    for (std::size_t at = 0, k = 0; at < block; at += slice, ++k) {
                        const std::size_t cnt = std::min(slice, block - at), next = at + slice;
                        if (next < block) b.ctx.d2h_async(pin[(k + 1) & 1], src + 32 * next, std::min(slice, block - next) * 32);
                        _builder.absorb(host_values(pin[k & 1], cnt), d * block + at, cnt);
                        b.ctx.sync();
                    }
                }
            }
            return _builder.finish();
        } else {
            if constexpr (builder_kind == detail::tree_builder_kind::vector)
                if (blocks.size() == 1) {    // straight into the vector: one copy for canonical-limb scalar types (backend.hpp)
                    _leaf_vec.clear();       // keeps its capacity: after the first commit no page of it is touched for the first time
                    download_scalars<adapter>(blocks[0].ctx, blocks[0].d_leaves, total, _leaf_vec);
                    return _builder(_leaf_vec, per_leaf);
                }
            /* one page-locked buffer for all leaves (portable: every member's copy engine may write it), the blocks' downloads side by side.  The
               vector builder goes through it only with several blocks: a pageable vector cannot be the target of several members' copy engines */
            char *pin = static_cast<char *>(blocks[0].scratch.pin[0].reserve(blocks[0].ctx, std::max<std::size_t>(1, total) * 32));
            if (total != 0) {
                for (std::size_t d = 0; d < blocks.size(); ++d) blocks[d].ctx.d2h_async(pin + 32 * d * block, blocks[d].d_leaves, block * 32);
                for (const leaf_block &b : blocks) b.ctx.sync();
            }
            const value_type *values = host_values(pin, total);
            if constexpr (builder_kind == detail::tree_builder_kind::span) return _builder(values, total, per_leaf);
            else {
                _leaf_vec.assign(values, values + total);
                return _builder(_leaf_vec, per_leaf);
            }
        }
    }
    /// `count` canonical 32-byte elements in host memory as scalar-field values: in place when the scalar type IS four canonical
    /// limbs, through a converted copy (host threads) otherwise
    const value_type *host_values(const void *limbs, std::size_t count) const {
        if constexpr (detail::canonical_scalars<adapter>::value) {
            static_assert(sizeof(value_type) == 32, "canonical-limb scalars are 4 x u64");
            return static_cast<const value_type *>(limbs);
        } else {
            _conv.resize(count);
            const std::uint64_t *h = static_cast<const std::uint64_t *>(limbs);
            detail::host_parallel_for(count, (std::size_t)1 << 16, 8, [&](std::size_t lo, std::size_t hi) {
                for (std::size_t i = lo; i < hi; ++i) _conv[i] = adapter::scalar_from_limbs(h + 4 * i);
            });
            return _conv.data();
        }
    }
    /// what both public constructors come to: `members` upload streams (polys_evaluator.hpp) and scratch entries
    lpc_commitment_scheme_hip(const context &ctx, std::size_t members, const params_type &fri_params, TreeBuilder &&builder) :
        base(ctx, members), _scratch(new member_scratch[std::max<std::size_t>(1, members)]), _fri_params(fri_params), _builder(std::move(builder)),
        _etha(value_type::zero()) {
        std::size_t r = 0;
        for (std::size_t s : fri_params.step_list) r += s;
        if (fri_params.step_list.empty() || r > fri_params.log_domain) throw std::invalid_argument("lpc: step_list does not fit the domain");
    }
    /// host wall time of the last query_phase by part, for a measuring subclass (the bench driver's): filled while _time_query_phase is set,
    /// which costs a stream synchronisation per batch.  Not part of the scheme's interface.
    struct query_phase_times {
        double reextend_ms = 0, gather_ms = 0, paths_ms = 0, host_ms = 0;
    };
    bool _time_query_phase = false;
    query_phase_times _last_query_times;
    const device_group *_group = nullptr;
    std::size_t _group_commits = 0, _last_owners = 0;
    mutable std::unique_ptr<member_scratch[]> _scratch;    // max(1, world) entries; an array: the page-locked buffers neither copy nor move
    params_type _fri_params;
    mutable TreeBuilder _builder;
    value_type _etha;
    mutable std::vector<value_type> _leaf_vec, _conv;
    std::map<std::size_t, bool> _batch_fixed;
    std::map<std::size_t, precommitment_type> _trees;
    preprocessed_data_type _fixed_polys_values;
    std::vector<precommitment_type> _fri_trees;
    std::vector<device_polynomial_dfs<CurveType>> _fs;
    std::vector<value_type> _alphas;
};

}    // namespace hip
}    // namespace zk
}    // namespace crypto3
}    // namespace nil

#endif    // ZKHIP_SHIM_LPC_HPP
