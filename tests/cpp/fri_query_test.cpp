// C++ shim test harness (test-only) of the FRI query phase: lpc_commitment_scheme_hip::query_phase / proof_eval_full / verify_eval and
// detail::domain_index.  A run commits two batches, opens them at ragged point sets and produces a whole proof; everything in it -- values,
// paths, leaf indices, the challenges the transcript handed out -- goes back to the Python driver, which holds it against the oracle and
// hashlib.  The verifier is run here, on a scheme object of its own that has only what a verifier has, on the proof and on copies with one
// thing changed each.
// Built into libfriquerytest.so by tests/cpp/Makefile; driven by tests/test_gpu_fri_query_shim.py and tests/test_host_fri_query.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <vector>

#include <nil/crypto3/zk/hip/lpc.hpp>
#include <nil/crypto3/zk/hip/merkle.hpp>
#include <nil/crypto3/zk/hip/transcript.hpp>

#include "harness_common.hpp"

using namespace nil::crypto3::zk::hip;

namespace {

typedef std::array<std::uint8_t, 32> digest;

/// The SHA2-256 transcript, counted; with a script the challenges come from the caller instead (absorbing still hashes).  Keeps every
/// challenge it handed out.
template <typename Curve>
struct harness_transcript {
    typedef curve_adapter<Curve> A;
    typedef typename A::scalar_value_type Fr;
    sha256_transcript<Curve> inner;
    std::vector<Fr> script, drawn;
    bool scripted = false;
    std::size_t next = 0, absorbed = 0;
    explicit harness_transcript(const std::vector<std::uint8_t> &seed) : inner(seed) { }
    template <typename T>
    void operator()(const T &r) {
        ++absorbed;
        inner(r);
    }
    Fr challenge() {
        const Fr c = scripted ? script.at(next) : inner.challenge();
        ++next;
        drawn.push_back(c);
        return c;
    }
    template <typename Integral>
    Integral int_challenge() {
        return inner.template int_challenge<Integral>();
    }
    const digest &state() const { return inner.state(); }
};

/// a host Merkle tree by the convention of include/zkhip.h, with root() and proof(i): what a host tree builder's result looks like
struct host_path {
    std::size_t leaf_index = 0;
    std::vector<digest> siblings;
};
struct host_tree {
    std::size_t leaves = 0;
    std::vector<digest> nodes;    // the leaf digests, then each level above, the root last
    const digest &root() const { return nodes.back(); }
    host_path proof(std::size_t i) const {
        host_path p;
        p.leaf_index = i;
        for (std::size_t l = 0; ((std::size_t)1 << l) < leaves; ++l) p.siblings.push_back(nodes[2 * leaves - ((2 * leaves) >> l) + ((i >> l) ^ 1)]);
        return p;
    }
};
template <typename Curve>
struct host_builder {
    typedef curve_adapter<Curve> A;
    host_tree operator()(const std::vector<typename A::scalar_value_type> &elements, std::size_t per_leaf) const {
        host_tree t;
        t.leaves = elements.size() / per_leaf;
        std::vector<std::uint8_t> bytes(32 * per_leaf);
        for (std::size_t x = 0; x < t.leaves; ++x) {
            for (std::size_t k = 0; k < per_leaf; ++k) {
                std::uint64_t limbs[4];
                A::scalar_to_limbs(elements[x * per_leaf + k], limbs);
                for (int j = 0; j < 32; ++j) bytes[32 * k + j] = std::uint8_t(limbs[3 - j / 8] >> (8 * (7 - j % 8)));
            }
            digest d;
            check(zkhip_sha256_host(bytes.data(), bytes.size(), d.data()), "zkhip_sha256_host");
            t.nodes.push_back(d);
        }
        for (std::size_t at = 0, n = t.leaves; n > 1; at += n, n /= 2)
            for (std::size_t j = 0; j < n / 2; ++j) {
                std::uint8_t pair[64];
                std::memcpy(pair, t.nodes[at + 2 * j].data(), 32);
                std::memcpy(pair + 32, t.nodes[at + 2 * j + 1].data(), 32);
                digest d;
                check(zkhip_sha256_host(pair, 64, d.data()), "zkhip_sha256_host");
                t.nodes.push_back(d);
            }
        return t;
    }
};
/// a host tree that cannot open a leaf: the scheme still compiles with it (proof_eval), only query_phase would not
struct rootless_tree {
    digest d {};
    const digest &root() const { return d; }
};
template <typename Curve>
struct rootless_builder {
    rootless_tree operator()(const std::vector<typename curve_adapter<Curve>::scalar_value_type> &, std::size_t) const { return rootless_tree(); }
};

struct run_io {
    const std::uint64_t *evals;
    std::size_t npolys;
    const std::uint64_t *log_n;
    std::size_t log_domain;
    const std::uint64_t *steps;
    std::size_t nsteps;
    const std::uint64_t *points;
    const std::uint64_t *script;
    std::size_t nscript, lambda;
    std::uint32_t grind_mask;
    const std::uint8_t *seed;
    std::size_t seed_len;
    std::uint8_t *roots, *fri_roots;
    std::uint64_t *z, *final_poly;
    std::uint32_t *nonce;
    std::uint64_t *counts, *drawn, *init_values, *init_leaf;
    std::uint8_t *init_paths;
    std::uint64_t *y, *round_leaf;
    std::uint8_t *round_paths;
    std::uint64_t *round_polys;    // fs[0 .. nsteps - 1] of the commit phase, one after the other
    std::uint32_t *flags;
};

template <typename Curve>
fri_params_hip<Curve> make_params(const run_io &io, std::size_t lambda) {
    fri_params_hip<Curve> params = fri_params_hip<Curve>::standard(io.log_domain, std::vector<std::size_t>(io.steps, io.steps + io.nsteps));
    params.lambda = lambda;
    params.max_degree = ((std::size_t)1 << (io.log_domain - 1)) - 1;    // D[0] is twice as long as the longest admissible polynomial
    if (io.grind_mask) {
        params.use_grinding = true;
        params.grinding_parameter = io.grind_mask;
    }
    return params;
}

template <typename Curve>
harness_transcript<Curve> make_transcript(const run_io &io) {
    typedef curve_adapter<Curve> A;
    harness_transcript<Curve> tr(std::vector<std::uint8_t>(io.seed, io.seed + io.seed_len));
    tr.scripted = io.nscript != 0;
    for (std::size_t i = 0; i < io.nscript; ++i) tr.script.push_back(A::scalar_from_limbs(io.script + 4 * i));
    return tr;
}

/// the ragged point sets: what prover and verifier both know
template <typename Curve, typename Scheme>
void set_points(Scheme &scheme, const run_io &io) {
    typedef curve_adapter<Curve> A;
    typedef typename A::scalar_value_type Fr;
    const std::vector<Fr> pts = {A::scalar_from_limbs(io.points), A::scalar_from_limbs(io.points + 4), A::scalar_from_limbs(io.points + 8)};
    scheme.append_eval_point(0, pts[0]);
    scheme.append_eval_point(1, pts[0]);
    scheme.append_eval_point(1, 0, pts[1]);
    scheme.append_eval_points(0, 1, std::vector<Fr> {pts[2]});
}

/// what a verifier is handed besides the proof and the roots: the transcript as it stood when etha was drawn, the fixed batches' values there
template <typename Curve>
struct verifier_data {
    harness_transcript<Curve> at_setup;
    std::map<std::size_t, std::vector<typename curve_adapter<Curve>::scalar_value_type>> fixed_values;
};

/// batch 0 (fixed) = polys[0..1], batch 1 = polys[2..]: commit both, set the ragged point sets; leaves `tr` where proof_eval starts
template <typename Curve, typename Scheme>
void commit_and_open(Scheme &scheme, const run_io &io, harness_transcript<Curve> &tr, std::uint8_t *out_roots, verifier_data<Curve> *public_data = nullptr) {
    typedef curve_adapter<Curve> A;
    typedef typename A::scalar_value_type Fr;
    std::vector<polynomial_dfs<Curve>> polys(io.npolys);
    std::size_t at = 0;
    for (std::size_t p = 0; p < io.npolys; ++p)
        for (std::size_t i = 0; i < ((std::size_t)1 << io.log_n[p]); ++i) polys[p].values.push_back(A::scalar_from_limbs(io.evals + 4 * at++));
    scheme.append_to_batch(0, std::vector<polynomial_dfs<Curve>>(polys.begin(), polys.begin() + 2));
    const digest r0 = scheme.commit(0);
    scheme.mark_batch_as_fixed(0);
    /* preprocess and setup must draw the same etha: a script names it twice, the hashing transcript is asked from the same state twice */
    harness_transcript<Curve> pre = tr;
    auto prep = scheme.preprocess(tr.scripted ? tr : pre);
    pre = tr;    // setup draws etha from here
    scheme.setup(tr, prep);
    scheme.append_to_batch(1, std::vector<polynomial_dfs<Curve>>(polys.begin() + 2, polys.end()));
    const digest r1 = scheme.commit(1);
    if (out_roots) {
        std::memcpy(out_roots, r0.data(), 32);
        std::memcpy(out_roots + 32, r1.data(), 32);
    }
    set_points<Curve>(scheme, io);
    if (public_data) *public_data = {pre, prep};
}

template <typename Curve, typename Proof>
void put_proof(const Proof &proof, const run_io &io) {
    typedef curve_adapter<Curve> A;
    std::size_t zi = 0;
    for (std::size_t k : proof.z.get_batches())
        for (std::size_t i = 0; i < proof.z.get_batch_size(k); ++i)
            for (std::size_t q = 0; q < proof.z.get_poly_points_number(k, i); ++q) A::scalar_to_limbs(proof.z.get(k, i, q), io.z + 4 * zi++);
    io.counts[0] = zi;
    const auto &fp = proof.fri_proof;
    for (std::size_t i = 0; i < fp.fri_roots.size(); ++i) std::memcpy(io.fri_roots + 32 * i, fp.fri_roots[i].data(), 32);
    for (std::size_t i = 0; i < fp.final_polynomial.size(); ++i) A::scalar_to_limbs(fp.final_polynomial[i], io.final_poly + 4 * i);
    *io.nonce = fp.proof_of_work;
    /* initial proofs: per batch [q][p][pair][2] values, [q] leaf indices, [q][depth] siblings */
    std::uint64_t *v = io.init_values, *leaf = io.init_leaf;
    std::uint8_t *path = io.init_paths;
    for (std::size_t k = 0; k < 2; ++k)
        for (const auto &qp : fp.query_proofs) {
            const auto &ip = qp.initial_proof.at(k);
            for (const auto &poly : ip.values)
                for (const auto &pair : poly)
                    for (const auto &value : pair) {
                        A::scalar_to_limbs(value, v);
                        v += 4;
                    }
            *leaf++ = ip.p.leaf_index;
            for (const auto &s : ip.p.siblings) {
                std::memcpy(path, s.data(), 32);
                path += 32;
            }
        }
    /* round proofs: per round [q][pair][2] values, [q] leaf indices, [q][depth] siblings */
    v = io.y;
    leaf = io.round_leaf;
    path = io.round_paths;
    for (std::size_t i = 0; i < io.nsteps; ++i)
        for (const auto &qp : fp.query_proofs) {
            const auto &rp = qp.round_proofs.at(i);
            for (const auto &pair : rp.y)
                for (const auto &value : pair) {
                    A::scalar_to_limbs(value, v);
                    v += 4;
                }
            *leaf++ = rp.p.leaf_index;
            for (const auto &s : rp.p.siblings) {
                std::memcpy(path, s.data(), 32);
                path += 32;
            }
        }
}

/// mode 0: device builder, one context (with verification);  1: host builder, one context;  2: host builder over a device group of two
template <typename Curve, typename Builder, bool Group>
int lpc_run(const run_io &io) {
    typedef curve_adapter<Curve> A;
    typedef harness_transcript<Curve> T;
    typedef lpc_commitment_scheme_hip<Curve, T, Builder> scheme_type;
    typedef typename scheme_type::proof_type proof_type;
    constexpr bool device = scheme_type::builder_kind == detail::tree_builder_kind::device;
    static_assert(std::is_same<typename scheme_type::merkle_path_type, typename std::conditional<device, device_merkle_path, host_path>::type>::value,
                  "the path type follows the builder");
    static_assert(std::is_same<typename lpc_commitment_scheme_hip<Curve, T, rootless_builder<Curve>>::merkle_path_type, detail::no_merkle_path>::value,
                  "a host tree without proof(i) has no path type");
    context ctx(0);
    std::unique_ptr<device_group> grp;
    std::unique_ptr<scheme_type> holder;
    if constexpr (Group) {
        grp.reset(new device_group(std::vector<int> {0, 0}));
        holder.reset(new scheme_type(*grp, make_params<Curve>(io, io.lambda), Builder()));
    } else {
        holder.reset(new scheme_type(ctx, make_params<Curve>(io, io.lambda), Builder()));
    }
    scheme_type &scheme = *holder;
    T tr = make_transcript<Curve>(io);
    verifier_data<Curve> pub {make_transcript<Curve>(io), {}};
    commit_and_open<Curve>(scheme, io, tr, io.roots, &pub);
    std::srand(1);          // the first nonce tried by the grinding: the same in every run
    proof_type proof = scheme.proof_eval_full(tr);
    put_proof<Curve>(proof, io);
    {
        std::uint64_t *at = io.round_polys;
        for (std::size_t i = 0; i < io.nsteps; ++i)
            for (const auto &value : scheme.fri_round_polynomial(i).values) {
                A::scalar_to_limbs(value, at);
                at += 4;
            }
    }
    io.counts[1] = tr.next;
    io.counts[2] = tr.absorbed;
    io.counts[3] = tr.next - io.lambda;
    io.counts[5] = scheme.group_commits();
    for (std::size_t i = 0; i < tr.drawn.size() && i < 64; ++i) A::scalar_to_limbs(tr.drawn[i], io.drawn + 4 * i);
    std::uint32_t flags = 0;
    if (proof.fri_proof.query_proofs.size() != io.lambda) return -20;

    {    /* a plain proof_eval on a second scheme object over the same inputs: the same z, roots, final polynomial, nonce and transcript traffic */
        scheme_type second(ctx, make_params<Curve>(io, 0), Builder());
        T tr2 = make_transcript<Curve>(io);
        commit_and_open<Curve>(second, io, tr2, nullptr);
        std::srand(1);
        const proof_type plain = second.proof_eval(tr2);
        io.counts[4] = tr2.next;
        if (plain.fri_proof.query_proofs.empty()) flags |= 1u << 9;
        if (plain.z == proof.z && plain.fri_proof.fri_roots == proof.fri_proof.fri_roots && plain.fri_proof.final_polynomial == proof.fri_proof.final_polynomial &&
            plain.fri_proof.proof_of_work == proof.fri_proof.proof_of_work && tr2.next == io.counts[3] && tr2.absorbed == tr.absorbed)
            flags |= 1u << 8;
    }

    if constexpr (device) {
        typedef typename A::scalar_value_type Fr;
        std::map<std::size_t, digest> commitments;
        std::memcpy(commitments[0].data(), io.roots, 32);
        std::memcpy(commitments[1].data(), io.roots + 32, 32);
        /* the verifier's side: a scheme object of its own that is told the batch sizes, the points, which batch is fixed and -- through setup
           over the transcript as it stood there -- etha and the fixed values.  It never commits and never runs proof_eval. */
        T start = pub.at_setup;    // after make_verifier: where verify_eval starts
        auto make_verifier = [&](std::size_t max_degree) {
            fri_params_hip<Curve> params = make_params<Curve>(io, io.lambda);
            params.max_degree = max_degree;
            std::unique_ptr<scheme_type> v(new scheme_type(ctx, params, Builder()));
            v->set_batch_size(0, 2);
            v->set_batch_size(1, io.npolys - 2);
            v->mark_batch_as_fixed(0);
            start = pub.at_setup;
            v->setup(start, pub.fixed_values);
            set_points<Curve>(*v, io);
            return v;
        };
        const std::size_t max_degree = make_params<Curve>(io, io.lambda).max_degree;
        const std::unique_ptr<scheme_type> verifier = make_verifier(max_degree);
        auto verify = [&](const proof_type &p, const std::map<std::size_t, digest> &c) {
            T v = start;
            return verifier->verify_eval(p, c, v);
        };
        if (verify(proof, commitments)) flags |= 1u;
        auto rejected = [&](unsigned bit, const proof_type &p, const std::map<std::size_t, digest> &c) {
            if (!verify(p, c)) flags |= 1u << bit;
        };
        const std::size_t q = io.lambda - 1;
        const Fr one = Fr::one();
        {    // one initial value: the last polynomial of batch 1, its last pair, second element
            proof_type p = proof;
            auto &values = p.fri_proof.query_proofs[q].initial_proof.at(1).values;
            values.back().back()[1] = values.back().back()[1] + one;
            rejected(1, p, commitments);
        }
        {    // one y: the first round's, in query 0
            proof_type p = proof;
            auto &y = p.fri_proof.query_proofs[0].round_proofs[0].y;
            y.back()[0] = y.back()[0] + one;
            rejected(2, p, commitments);
        }
        {    // one sibling byte: a round path's top sibling where there is one, a batch path's otherwise
            proof_type p = proof;
            auto &round_path = p.fri_proof.query_proofs[q].round_proofs.back().p.siblings;
            auto &batch_path = p.fri_proof.query_proofs[q].initial_proof.at(0).p.siblings;
            (round_path.empty() ? batch_path : round_path).back()[31] ^= 1;
            rejected(3, p, commitments);
        }
        {    // one coefficient of the final polynomial
            proof_type p = proof;
            p.fri_proof.final_polynomial[0] = p.fri_proof.final_polynomial[0] + one;
            rejected(4, p, commitments);
        }
        {    // one root in `commitments`
            auto c = commitments;
            c[1][0] ^= 0x80;
            rejected(5, proof, c);
        }
        {    // one z value
            proof_type p = proof;
            p.z.set(1, 0, 1, p.z.get(1, 0, 1) + one);
            rejected(6, p, commitments);
        }
        {    // the degree bound: batch 1 holds a vector as long as D[0], so the honest final polynomial has as many coefficients as the last
             // domain has points -- admissible for max_degree + 1 = |D[0]| / 2 (the reference's bound is that loose at this rate), not for half of it
            const std::unique_ptr<scheme_type> tight = make_verifier((max_degree + 1) / 2 - 1);
            T v = start;
            if (!tight->verify_eval(proof, commitments, v)) flags |= 1u << 10;
        }
        {    // no degree bound, no verification: refused before the transcript is touched
            const std::unique_ptr<scheme_type> unset = make_verifier(0);
            T v = start;
            try {
                (void)unset->verify_eval(proof, commitments, v);
            } catch (const std::invalid_argument &) {
                if (v.next == start.next && v.absorbed == start.absorbed) flags |= 1u << 11;
            }
        }
        if (io.grind_mask) {    // the nonce
            proof_type p = proof;
            p.fri_proof.proof_of_work ^= 1;
            rejected(7, p, commitments);
        }
    }
    *io.flags = flags;
    return 0;
}

template <typename Curve>
int lpc_run_mode(int mode, const run_io &io) {
    if (mode == 0) return lpc_run<Curve, device_merkle_builder<ZKHIP_HASH_SHA2_256>, false>(io);
    if (mode == 1) return lpc_run<Curve, host_builder<Curve>, false>(io);
    return lpc_run<Curve, host_builder<Curve>, true>(io);
}

/// query_phase refused: bit 0 lambda == 0, bit 1 step list {1, 2}, bit 2 before proof_eval; each with the transcript's counters untouched
template <typename Curve>
int refusals(const run_io &io, std::uint32_t *flags) {
    typedef harness_transcript<Curve> T;
    typedef lpc_commitment_scheme_hip<Curve, T, device_merkle_builder<ZKHIP_HASH_SHA2_256>> scheme_type;
    context ctx(0);
    *flags = 0;
    for (unsigned k = 0; k < 3; ++k) {
        fri_params_hip<Curve> params = make_params<Curve>(io, k == 0 ? 0 : io.lambda);
        if (k == 1) params.step_list = {1, 2};
        scheme_type scheme(ctx, params, device_merkle_builder<ZKHIP_HASH_SHA2_256>());
        T tr = make_transcript<Curve>(io);
        commit_and_open<Curve>(scheme, io, tr, nullptr);
        typename scheme_type::proof_type proof;
        if (k != 2) proof = scheme.proof_eval(tr);
        const std::size_t next = tr.next, absorbed = tr.absorbed;
        try {
            scheme.query_phase(tr, proof);
        } catch (const std::invalid_argument &) {
            if (tr.next == next && tr.absorbed == absorbed && proof.fri_proof.query_proofs.empty()) *flags |= 1u << k;
        }
    }
    return 0;
}

template <typename Curve>
int domain_index_of(const std::uint64_t *x, std::size_t log_domain, std::uint64_t *out) {
    typedef curve_adapter<Curve> A;
    try {
        *out = detail::domain_index(A::scalar_from_limbs(x), log_domain, [](std::size_t log_n) { return A::root_of_unity(log_n); });
        return 0;
    } catch (const std::runtime_error &) {
        return 1;
    }
}

#define FQ_DISPATCH(curve, call)                \
    do {                                        \
        if (curve == ZKHIP_BLS12_381) return call(bls12_381); \
        if (curve == ZKHIP_BN254) return call(alt_bn128_254); \
        if (curve == ZKHIP_PALLAS) return call(pallas);       \
        if (curve == ZKHIP_VESTA) return call(vesta);         \
        return -2;                              \
    } while (0)

}    // namespace

extern "C" {

/// host arithmetic only: the index of x in the 2^log_domain-point domain; 0 and the index, or 1 when x is not in the domain
int fq_domain_index(int curve, const std::uint64_t *x, std::size_t log_domain, std::uint64_t *out) {
#define CALL(C) domain_index_of<C>(x, log_domain, out)
    FQ_DISPATCH(curve, CALL);
#undef CALL
}

/// host arithmetic only: pair j of detail::pair_positions(x, log_n, fri_step) in out[j]
void fq_pair_positions(std::size_t x, std::size_t log_n, std::size_t fri_step, std::uint64_t *out) {
    const auto pos = detail::pair_positions(x, log_n, fri_step);
    for (std::size_t j = 0; j < pos.size(); ++j) out[j] = pos[j];
}

int fq_lpc_run(int curve, int mode, const std::uint64_t *evals, std::size_t npolys, const std::uint64_t *log_n, std::size_t log_domain, const std::uint64_t *steps,
               std::size_t nsteps, const std::uint64_t *points, const std::uint64_t *script, std::size_t nscript, std::size_t lambda, std::uint32_t grind_mask,
               const std::uint8_t *seed, std::size_t seed_len, std::uint8_t *roots, std::uint8_t *fri_roots, std::uint64_t *z, std::uint64_t *final_poly,
               std::uint32_t *nonce, std::uint64_t *counts, std::uint64_t *drawn, std::uint64_t *init_values, std::uint64_t *init_leaf, std::uint8_t *init_paths,
               std::uint64_t *y, std::uint64_t *round_leaf, std::uint8_t *round_paths, std::uint64_t *round_polys, std::uint32_t *flags) {
    const run_io io = {evals, npolys, log_n, log_domain, steps, nsteps, points, script, nscript, lambda, grind_mask, seed, seed_len, roots, fri_roots, z, final_poly,
                       nonce, counts, drawn, init_values, init_leaf, init_paths, y, round_leaf, round_paths, round_polys, flags};
    return harness::guarded(__func__, [&]() -> int {
#define CALL(C) lpc_run_mode<C>(mode, io)
        FQ_DISPATCH(curve, CALL);
#undef CALL
    });
}

int fq_refusals(int curve, const std::uint64_t *evals, std::size_t npolys, const std::uint64_t *log_n, std::size_t log_domain, const std::uint64_t *points,
                const std::uint64_t *script, std::size_t nscript, std::size_t lambda, std::uint32_t *flags) {
    const std::uint64_t steps[2] = {1, 1};
    const std::uint8_t seed = 7;
    run_io io = {};
    io.evals = evals, io.npolys = npolys, io.log_n = log_n, io.log_domain = log_domain, io.steps = steps, io.nsteps = 2, io.points = points, io.script = script,
    io.nscript = nscript, io.lambda = lambda, io.seed = &seed, io.seed_len = 1;
    return harness::guarded(__func__, [&]() -> int {
#define CALL(C) refusals<C>(io, flags)
        FQ_DISPATCH(curve, CALL);
#undef CALL
    });
}

}    // extern "C"
