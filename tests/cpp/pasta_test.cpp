// C++ shim test harness (test-only) of the Pasta curves: the host algebra of hip/algebra.hpp over `pallas` / `vesta`, multiexp<multiexp_method_hip>
// on their G1, and lpc_commitment_scheme_hip over a sha256_transcript with grinding -- with the device tree builder and with two host builders
// (streaming and vector shaped) that hash with the library's own SHA2-256.  Everything a run produces goes back to the Python driver, which
// holds it against the oracle and hashlib.  The placeholder argument classes are instantiated in full for both curves (compile coverage; their
// kernels are driven through the C ABI by tests/test_gpu_pasta.py).
// Built into libpastatest.so by tests/cpp/Makefile; driven by tests/test_host_pasta.py and tests/test_gpu_pasta_shim.py.
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include <nil/crypto3/zk/hip/lpc.hpp>
#include <nil/crypto3/zk/hip/merkle.hpp>
#include <nil/crypto3/zk/hip/multiexp.hpp>
#include <nil/crypto3/zk/hip/placeholder_lookup.hpp>
#include <nil/crypto3/zk/hip/placeholder_permutation.hpp>
#include <nil/crypto3/zk/hip/placeholder_quotient.hpp>
#include <nil/crypto3/zk/hip/proof_of_work.hpp>
#include <nil/crypto3/zk/hip/transcript.hpp>

#include "eval_polys_case.hpp"
#include "fr_vector_case.hpp"

using namespace nil::crypto3::zk::hip;

// every member of the placeholder classes, for both curves
template struct nil::crypto3::zk::hip::placeholder_permutation_hip<pallas>;
template struct nil::crypto3::zk::hip::placeholder_permutation_hip<vesta>;
template struct nil::crypto3::zk::hip::placeholder_lookup_hip<pallas>;
template struct nil::crypto3::zk::hip::placeholder_lookup_hip<vesta>;
template struct nil::crypto3::zk::hip::placeholder_quotient_hip<pallas>;
template struct nil::crypto3::zk::hip::placeholder_quotient_hip<vesta>;

namespace {

static_assert(curve_adapter<pallas>::id == ZKHIP_PALLAS && curve_adapter<vesta>::id == ZKHIP_VESTA, "ids");
static_assert(!curve_adapter<pallas>::has_g2 && !curve_adapter<vesta>::has_g2 && curve_adapter<bls12_381>::has_g2, "only the pairing curves have a G2");
static_assert(curve_adapter<pallas>::g1_coord_limbs == 4 && curve_adapter<vesta>::g2_coord_limbs == 0, "4-limb Fq, no G2");
static_assert(curve_adapter<pallas>::two_adicity == 32 && curve_adapter<vesta>::two_adicity == 32, "two-adicity");

typedef std::array<std::uint8_t, 32> digest;

/// what a host builder returns: the root is all the scheme asks for
struct host_tree {
    digest r {};
    const digest &root() const { return r; }
};

digest sha(const std::uint8_t *msg, std::size_t len) {
    digest d;
    if (zkhip_sha256_host(msg, len, d.data()) != 0) throw std::runtime_error("zkhip_sha256_host");
    return d;
}

/// leaf digests of `count` elements (whole leaves of per_leaf elements, each hashed as its 32-byte big-endian encoding), appended to `level`
template <typename A>
void hash_leaves(const typename A::scalar_value_type *v, std::size_t count, std::size_t per_leaf, std::vector<digest> &level) {
    std::vector<std::uint8_t> buf(32 * per_leaf);
    for (std::size_t at = 0; at < count; at += per_leaf) {
        for (std::size_t e = 0; e < per_leaf; ++e) {
            std::uint64_t l[4];
            A::scalar_to_limbs(v[at + e], l);
            for (int b = 0; b < 32; ++b) buf[32 * e + b] = (std::uint8_t)(l[3 - b / 8] >> (8 * (7 - b % 8)));
        }
        level.push_back(sha(buf.data(), buf.size()));
    }
}
host_tree reduce(std::vector<digest> level) {
    while (level.size() > 1) {
        std::vector<digest> up(level.size() / 2);
        for (std::size_t j = 0; j < up.size(); ++j) {
            std::uint8_t pair[64];
            std::memcpy(pair, level[2 * j].data(), 32);
            std::memcpy(pair + 32, level[2 * j + 1].data(), 32);
            up[j] = sha(pair, 64);
        }
        level.swap(up);
    }
    return host_tree {level.at(0)};
}

template <typename Curve>
struct streaming_builder {
    typedef curve_adapter<Curve> A;
    std::size_t total = 0, per = 0, seen = 0;
    std::vector<digest> level;
    void begin(std::size_t total_elements, std::size_t per_leaf) { total = total_elements, per = per_leaf, seen = 0, level.clear(); }
    void absorb(const typename A::scalar_value_type *v, std::size_t first, std::size_t count) {
        if (first != seen || count % per != 0) throw std::logic_error("streaming_builder: slices must be whole leaves, in order");
        hash_leaves<A>(v, count, per, level);
        seen += count;
    }
    host_tree finish() {
        if (seen != total) throw std::logic_error("streaming_builder: leaves missing");
        return reduce(level);
    }
};
template <typename Curve>
struct vector_builder {
    typedef curve_adapter<Curve> A;
    host_tree operator()(const std::vector<typename A::scalar_value_type> &leaves, std::size_t per_leaf) const {
        std::vector<digest> level;
        hash_leaves<A>(leaves.data(), leaves.size(), per_leaf, level);
        return reduce(level);
    }
};

struct lpc_out {
    std::uint8_t *commit_root, *fri_roots, *state;
    std::uint64_t *final_poly, *alphas, *z, *counts;
    std::uint32_t *nonce;
};

/// npolys polynomials of 2^log_rows evaluations in one batch, opened at one point, over the 2^log_domain-point domain; grinding with `mask`
template <typename Curve, typename Builder>
int lpc_run(const std::uint64_t *evals, std::size_t npolys, std::size_t log_rows, std::size_t log_domain, const std::uint64_t *steps, std::size_t nsteps,
            const std::uint64_t *point, const std::uint8_t *init, std::size_t init_len, std::uint32_t mask, const lpc_out &out) {
    typedef curve_adapter<Curve> A;
    typedef sha256_transcript<Curve> transcript_type;
    typedef lpc_commitment_scheme_hip<Curve, transcript_type, Builder> scheme_type;
    context ctx(0);
    fri_params_hip<Curve> params = fri_params_hip<Curve>::standard(log_domain, std::vector<std::size_t>(steps, steps + nsteps));
    params.use_grinding = true;
    params.grinding_parameter = mask;
    scheme_type scheme(ctx, params, Builder());
    std::vector<polynomial_dfs<Curve>> polys(npolys);
    for (std::size_t p = 0; p < npolys; ++p)
        for (std::size_t i = 0; i < ((std::size_t)1 << log_rows); ++i) polys[p].values.push_back(A::scalar_from_limbs(evals + 4 * ((p << log_rows) + i)));
    scheme.append_to_batch(0, polys);
    std::memcpy(out.commit_root, scheme.commit(0).data(), 32);
    scheme.append_eval_point(0, A::scalar_from_limbs(point));
    transcript_type tr(std::vector<std::uint8_t>(init, init + init_len));
    /* the search starts at std::rand(), as the reference's does: pin the generator so that the driver knows the start (counts[3]) */
    std::srand(950);
    out.counts[3] = (std::uint32_t)std::rand();
    std::srand(950);
    auto proof = scheme.proof_eval(tr);
    std::memcpy(out.state, tr.state().data(), 32);
    std::size_t zi = 0;
    for (std::size_t k : proof.z.get_batches())
        for (std::size_t i = 0; i < proof.z.get_batch_size(k); ++i)
            for (std::size_t q = 0; q < proof.z.get_poly_points_number(k, i); ++q) A::scalar_to_limbs(proof.z.get(k, i, q), out.z + 4 * zi++);
    if (proof.fri_proof.fri_roots.size() != nsteps) return -20;
    for (std::size_t i = 0; i < nsteps; ++i) std::memcpy(out.fri_roots + 32 * i, proof.fri_proof.fri_roots[i].data(), 32);
    for (std::size_t i = 0; i < proof.fri_proof.final_polynomial.size(); ++i) A::scalar_to_limbs(proof.fri_proof.final_polynomial[i], out.final_poly + 4 * i);
    for (std::size_t i = 0; i < scheme.fri_alphas().size(); ++i) A::scalar_to_limbs(scheme.fri_alphas()[i], out.alphas + 4 * i);
    out.counts[0] = zi;
    out.counts[1] = proof.fri_proof.final_polynomial.size();
    out.counts[2] = scheme.fri_alphas().size();
    *out.nonce = proof.fri_proof.proof_of_work;
    return 0;
}

template <typename Curve>
int lpc_run_t(int builder, const std::uint64_t *evals, std::size_t npolys, std::size_t log_rows, std::size_t log_domain, const std::uint64_t *steps,
              std::size_t nsteps, const std::uint64_t *point, const std::uint8_t *init, std::size_t init_len, std::uint32_t mask, const lpc_out &out) {
    typedef sha256_transcript<Curve> T;
    typedef device_merkle_builder<ZKHIP_HASH_SHA2_256> D;
    static_assert(lpc_commitment_scheme_hip<Curve, T, D>::builder_kind == detail::tree_builder_kind::device, "device builder");
    static_assert(lpc_commitment_scheme_hip<Curve, T, streaming_builder<Curve>>::builder_kind == detail::tree_builder_kind::streaming, "streaming builder");
    static_assert(lpc_commitment_scheme_hip<Curve, T, vector_builder<Curve>>::builder_kind == detail::tree_builder_kind::vector, "vector builder");
    switch (builder) {
        case 0: return lpc_run<Curve, D>(evals, npolys, log_rows, log_domain, steps, nsteps, point, init, init_len, mask, out);
        case 1: return lpc_run<Curve, streaming_builder<Curve>>(evals, npolys, log_rows, log_domain, steps, nsteps, point, init, init_len, mask, out);
        case 2: return lpc_run<Curve, vector_builder<Curve>>(evals, npolys, log_rows, log_domain, steps, nsteps, point, init, init_len, mask, out);
        default: return -2;
    }
}

/// host algebra.  op: 0 fr a * b, 1 fr a^-1, 2 fr a + b, 3 fr a - b  (4 limbs in and out)
template <typename Curve>
int fr_op_t(int op, const std::uint64_t *a, const std::uint64_t *b, std::uint64_t *out) {
    typedef curve_adapter<Curve> A;
    const auto x = A::scalar_from_limbs(a), y = A::scalar_from_limbs(b);
    switch (op) {
        case 0: A::scalar_to_limbs(x * y, out); return 0;
        case 1: A::scalar_to_limbs(x.inversed(), out); return 0;
        case 2: A::scalar_to_limbs(x + y, out); return 0;
        case 3: A::scalar_to_limbs(x - y, out); return 0;
        default: return -2;
    }
}
/// op: 0 P + Q, 1 k P, 2 P - Q, 3 (P == Q) into out_inf; affine limbs x | y and an infinity flag each
template <typename Curve>
int g1_op_t(int op, const std::uint64_t *p, int p_inf, const std::uint64_t *q, int q_inf, const std::uint64_t *k, std::uint64_t *out, int *out_inf) {
    typedef curve_adapter<Curve> A;
    typedef typename A::g1_value_type G;
    const G P = G::from_affine(p, p_inf != 0), Q = G::from_affine(q, q_inf != 0);
    G R;
    switch (op) {
        case 0: R = P + Q; break;
        case 1: R = P * A::scalar_from_limbs(k); break;
        case 2: R = P - Q; break;
        case 3: *out_inf = P == Q ? 1 : 0; return 0;
        default: return -2;
    }
    *out_inf = A::point_to_affine_limbs(R, out) ? 0 : 1;
    return 0;
}
template <typename Curve>
int root_t(std::size_t log_n, std::uint64_t *out, std::uint64_t *generator, std::uint64_t *modulus) {
    typedef curve_adapter<Curve> A;
    A::scalar_to_limbs(A::multiplicative_generator(), generator);
    A::scalar_modulus(modulus);
    try {
        A::scalar_to_limbs(A::root_of_unity(log_n), out);
    } catch (const std::invalid_argument &) {
        return 1;
    }
    return 0;
}
template <typename Curve>
int multiexp_t(const std::uint64_t *pts, const std::uint8_t *inf, const std::uint64_t *scalars, std::size_t n, std::uint64_t *out, int *out_inf) {
    typedef curve_adapter<Curve> A;
    typedef typename A::g1_value_type G;
    std::vector<G> bases;
    std::vector<typename A::scalar_value_type> sc;
    for (std::size_t i = 0; i < n; ++i) {
        bases.push_back(G::from_affine(pts + 8 * i, inf && inf[i]));
        sc.push_back(A::scalar_from_limbs(scalars + 4 * i));
    }
    const G r = multiexp<multiexp_method_hip>(bases.begin(), bases.end(), sc.begin(), sc.end(), 1);
    *out_inf = A::point_to_affine_limbs(r, out) ? 0 : 1;
    return 0;
}

/// eval_polys_case.hpp through lpc_commitment_scheme_hip (vector host builder, 2^6-point domain, step list {1, 1}, no grinding)
template <typename Curve>
int eval_polys_case_t(const std::uint64_t *evals, const std::uint64_t *points, std::uint64_t *out_z) {
    typedef sha256_transcript<Curve> transcript_type;
    context ctx(0);
    lpc_commitment_scheme_hip<Curve, transcript_type, vector_builder<Curve>> scheme(ctx, fri_params_hip<Curve>::standard(6, {1, 1}), vector_builder<Curve>());
    transcript_type tr(std::vector<std::uint8_t> {'e', 'v', 'a', 'l'});
    return eval_polys_case::run(scheme, tr, evals, points, out_z);
}

/// one case of fr_vector_case.hpp on a context of its own
template <typename Curve>
int fr_vector_t(int what, const std::uint64_t *a, const std::uint64_t *b, std::size_t n, const std::uint64_t *s, std::size_t m, int flag, std::uint64_t *out) {
    context ctx(0);
    return fr_vector_case::run<Curve>(ctx, what, a, b, n, s, m, flag, out);
}

}    // namespace

#define PASTA_DISPATCH(curve, call)                     \
    try {                                               \
        if (curve == ZKHIP_PALLAS) return call(pallas); \
        if (curve == ZKHIP_VESTA) return call(vesta);   \
        return -2;                                      \
    } catch (const std::exception &e) {                 \
        fprintf(stderr, "%s: %s\n", __func__, e.what()); \
        return -100;                                    \
    }

extern "C" {

int pasta_fr_op(int curve, int op, const std::uint64_t *a, const std::uint64_t *b, std::uint64_t *out) {
#define CALL(C) fr_op_t<C>(op, a, b, out)
    PASTA_DISPATCH(curve, CALL)
#undef CALL
}
int pasta_g1_op(int curve, int op, const std::uint64_t *p, int p_inf, const std::uint64_t *q, int q_inf, const std::uint64_t *k, std::uint64_t *out, int *out_inf) {
#define CALL(C) g1_op_t<C>(op, p, p_inf, q, q_inf, k, out, out_inf)
    PASTA_DISPATCH(curve, CALL)
#undef CALL
}
/// 0 with the root, 1 if root_of_unity threw std::invalid_argument; the generator and the modulus always
int pasta_root_of_unity(int curve, std::size_t log_n, std::uint64_t *out, std::uint64_t *generator, std::uint64_t *modulus) {
#define CALL(C) root_t<C>(log_n, out, generator, modulus)
    PASTA_DISPATCH(curve, CALL)
#undef CALL
}
/// multiexp<multiexp_method_hip> of n G1 points (the context-less arity of the reference: bases uploaded for this call)
int pasta_multiexp(int curve, const std::uint64_t *pts, const std::uint8_t *inf, const std::uint64_t *scalars, std::size_t n, std::uint64_t *out, int *out_inf) {
#define CALL(C) multiexp_t<C>(pts, inf, scalars, n, out, out_inf)
    PASTA_DISPATCH(curve, CALL)
#undef CALL
}
/// builder: 0 device_merkle_builder, 1 streaming host builder, 2 vector host builder.  counts: evaluations, final coefficients, alphas, the first nonce the search tried
int pasta_lpc_run(int curve, int builder, const std::uint64_t *evals, std::size_t npolys, std::size_t log_rows, std::size_t log_domain, const std::uint64_t *steps,
                  std::size_t nsteps, const std::uint64_t *point, const std::uint8_t *init, std::size_t init_len, std::uint32_t mask, std::uint8_t *commit_root,
                  std::uint8_t *fri_roots, std::uint64_t *final_poly, std::uint64_t *alphas, std::uint64_t *z, std::uint8_t *state, std::uint32_t *nonce,
                  std::uint64_t *counts) {
    const lpc_out out = {commit_root, fri_roots, state, final_poly, alphas, z, counts, nonce};
#define CALL(C) lpc_run_t<C>(builder, evals, npolys, log_rows, log_domain, steps, nsteps, point, init, init_len, mask, out)
    PASTA_DISPATCH(curve, CALL)
#undef CALL
}

/// the shared eval_polys case (eval_polys_case.hpp) through the LPC scheme: proof.z, 9 elements
int pasta_eval_polys_case(int curve, const std::uint64_t *evals, const std::uint64_t *points, std::uint64_t *out_z) {
#define CALL(C) eval_polys_case_t<C>(evals, points, out_z)
    PASTA_DISPATCH(curve, CALL)
#undef CALL
}

/// fr_vector (hip/fr_vector.hpp) member by member: the cases and their buffers are fr_vector_case.hpp's
int pasta_fr_vector(int curve, int what, const std::uint64_t *a, const std::uint64_t *b, std::size_t n, const std::uint64_t *s, std::size_t m, int flag, std::uint64_t *out) {
#define CALL(C) fr_vector_t<C>(what, a, b, n, s, m, flag, out)
    PASTA_DISPATCH(curve, CALL)
#undef CALL
}

}    // extern "C"
