// C++ shim test harness (test-only) of the proof of work: hip/transcript.hpp's sha256_transcript, hip/proof_of_work.hpp's proof_of_work_hip
// and lpc_commitment_scheme_hip::proof_eval with and without fri_params.use_grinding.  Everything a run produces goes back to the Python
// driver, which holds it against hashlib.  Built into libpowtest.so by tests/cpp/Makefile; driven by tests/test_gpu_pow_shim.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include <nil/crypto3/zk/hip/lpc.hpp>
#include <nil/crypto3/zk/hip/merkle.hpp>
#include <nil/crypto3/zk/hip/proof_of_work.hpp>
#include <nil/crypto3/zk/hip/transcript.hpp>

using namespace nil::crypto3::zk::hip;

namespace {

typedef bls12_381 Curve;
typedef curve_adapter<Curve> A;
typedef A::scalar_value_type Fr;
typedef sha256_transcript<Curve> transcript_type;
typedef device_merkle_builder<ZKHIP_HASH_SHA2_256> builder_type;

/// hashes like sha256_transcript, counts its calls, and does NOT show its state: what every transcript type looked like before grinding
struct counting_transcript {
    transcript_type inner;
    std::size_t absorbed = 0, challenges = 0;
    explicit counting_transcript(const std::vector<std::uint8_t> &init) : inner(init) { }
    template <typename T>
    void operator()(const T &r) {
        ++absorbed;
        inner(r);
    }
    Fr challenge() {
        ++challenges;
        return inner.challenge();
    }
};
static_assert(detail::has_state<transcript_type>::value, "sha256_transcript shows its state");
static_assert(!detail::has_state<counting_transcript>::value, "the counting transcript does not");

struct lpc_out {
    std::uint8_t *commit_root, *fri_roots, *state;    // 32, 3 x 32, 32 bytes
    std::uint64_t *final_poly;                        // 32 x 4 limbs
    std::uint32_t *nonce;
};

constexpr std::size_t LOG_DOMAIN = 8;

/// two polynomials of 2^7 evaluations in one batch, opened at one point, over the 2^8-point domain with step_list {1, 1, 1}
template <typename Transcript>
int lpc_run(const context &ctx, const fri_params_hip<Curve> &params, const std::uint64_t *evals, const std::uint64_t *point, Transcript &tr, const lpc_out &out) {
    typedef lpc_commitment_scheme_hip<Curve, Transcript, builder_type> scheme_type;
    scheme_type scheme(ctx, params, builder_type());
    std::vector<polynomial_dfs<Curve>> polys(2);
    for (std::size_t p = 0; p < 2; ++p)
        for (std::size_t i = 0; i < ((std::size_t)1 << (LOG_DOMAIN - 1)); ++i) polys[p].values.push_back(A::scalar_from_limbs(evals + 4 * ((p << (LOG_DOMAIN - 1)) + i)));
    scheme.append_to_batch(0, polys);
    std::memcpy(out.commit_root, scheme.commit(0).data(), 32);
    scheme.append_eval_point(0, A::scalar_from_limbs(point));
    auto proof = scheme.proof_eval(tr);
    if (proof.fri_proof.fri_roots.size() != 3 || proof.fri_proof.final_polynomial.size() != ((std::size_t)1 << (LOG_DOMAIN - 3))) return -20;
    for (std::size_t i = 0; i < 3; ++i) std::memcpy(out.fri_roots + 32 * i, proof.fri_proof.fri_roots[i].data(), 32);
    for (std::size_t i = 0; i < proof.fri_proof.final_polynomial.size(); ++i) A::scalar_to_limbs(proof.fri_proof.final_polynomial[i], out.final_poly + 4 * i);
    *out.nonce = proof.fri_proof.proof_of_work;
    return 0;
}

lpc_out slot(std::uint8_t *commit_roots, std::uint8_t *fri_roots, std::uint64_t *final_polys, std::uint8_t *states, std::uint32_t *nonces, std::size_t k) {
    return lpc_out {commit_roots + 32 * k, fri_roots + 96 * k, states + 32 * k, final_polys + 4 * 32 * k, nonces + k};
}

}    // namespace

extern "C" {

/// sha256_transcript step by step; states[k] after step k:
///   0 default construction   1 construction from `init`   2 absorb `msg`   3 absorb a 32-byte digest (std::array)   4 challenge()
///   5 int_challenge<uint32_t>()   6 absorb through iterators
/// Compared here with `expected` (7 x 32 bytes, the driver's hashlib): returns -(k + 1) for the first step that differs.
int pow_transcript_run(const std::uint8_t *init, std::size_t init_len, const std::uint8_t *msg, std::size_t msg_len, const std::uint8_t *digest,
                       const std::uint8_t *expected, std::uint8_t *states, std::uint64_t *challenge, std::uint32_t *int_challenge) {
    try {
        std::size_t k = 0;
        auto put = [&](const transcript_type &t) { std::memcpy(states + 32 * k++, t.state().data(), 32); };
        transcript_type t0;
        put(t0);
        transcript_type t(std::vector<std::uint8_t>(init, init + init_len));
        put(t);
        t(std::vector<std::uint8_t>(msg, msg + msg_len));
        put(t);
        std::array<std::uint8_t, 32> d;
        std::memcpy(d.data(), digest, 32);
        t(d);
        put(t);
        A::scalar_to_limbs(t.challenge(), challenge);
        put(t);
        *int_challenge = t.int_challenge<std::uint32_t>();
        put(t);
        t(msg, msg + msg_len);
        put(t);
        for (std::size_t i = 0; i < k; ++i)
            if (std::memcmp(states + 32 * i, expected + 32 * i, 32) != 0) return -(int)(i + 1);
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "pow_transcript_run: %s\n", e.what());
        return -100;
    }
}

/// generate() from `start` over the transcript built from `init`, verify() on a copy taken before.  flags: bit 0 verify accepted the nonce,
/// bit 1 both transcripts ended in the same state, bit 2 verify accepted nonce ^ 1 on another copy
int pow_generate_verify(const std::uint8_t *init, std::size_t init_len, std::uint32_t mask, std::uint32_t start, std::uint32_t *nonce, std::uint8_t *state_before,
                        std::uint8_t *state_after, std::uint32_t *flags) {
    try {
        typedef proof_of_work_hip<transcript_type> pow_type;
        context ctx(0);
        transcript_type tr(std::vector<std::uint8_t>(init, init + init_len));
        transcript_type copy = tr, other = tr;
        std::memcpy(state_before, tr.state().data(), 32);
        *nonce = pow_type::generate(ctx, tr, mask, start);
        std::memcpy(state_after, tr.state().data(), 32);
        *flags = 0;
        if (pow_type::verify(copy, *nonce, mask)) *flags |= 1;
        if (copy.state() == tr.state()) *flags |= 2;
        if (pow_type::verify(other, *nonce ^ 1, mask)) *flags |= 4;
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "pow_generate_verify: %s\n", e.what());
        return -100;
    }
}

/// lpc_commitment_scheme_hip::proof_eval, every run from a transcript built from `init`; slot k of every output belongs to run k:
///   0 params as standard() leaves them (a caller that predates the grinding fields)   1 use_grinding = false spelled out, another mask
///   2 run 0's params over the counting transcript (no state())                        3 use_grinding = true, mask `mask`
/// counts: absorbed and challenges of run 2.  flags: bit 0 run 3's nonce verifies against a replay of the transcript up to the end of the
/// commit phase, bit 1 that replay ends in run 3's final state, bit 2 grinding over the counting transcript threw std::invalid_argument
int pow_lpc_run(const std::uint64_t *evals, const std::uint64_t *point, const std::uint8_t *init, std::size_t init_len, std::uint32_t mask,
                std::uint8_t *commit_roots, std::uint8_t *fri_roots, std::uint64_t *final_polys, std::uint8_t *states, std::uint32_t *nonces, std::uint64_t *counts,
                std::uint32_t *flags) {
    try {
        context ctx(0);
        const std::vector<std::uint8_t> seed(init, init + init_len);
        const fri_params_hip<Curve> plain = fri_params_hip<Curve>::standard(LOG_DOMAIN, {1, 1, 1});
        if (plain.use_grinding || plain.grinding_parameter != 0xFFFF) return -10;
        fri_params_hip<Curve> off = plain, on = plain;
        off.use_grinding = false;
        off.grinding_parameter = 0xF;
        on.use_grinding = true;
        on.grinding_parameter = mask;
        *flags = 0;
        for (std::size_t k = 0; k < 4; ++k) {
            const lpc_out out = slot(commit_roots, fri_roots, final_polys, states, nonces, k);
            int rc = 0;
            if (k == 2) {
                counting_transcript tr(seed);
                rc = lpc_run(ctx, plain, evals, point, tr, out);
                std::memcpy(out.state, tr.inner.state().data(), 32);
                counts[0] = tr.absorbed;
                counts[1] = tr.challenges;
            } else {
                transcript_type tr(seed);
                rc = lpc_run(ctx, k == 0 ? plain : (k == 1 ? off : on), evals, point, tr, out);
                std::memcpy(out.state, tr.state().data(), 32);
            }
            if (rc != 0) return rc - (int)k;
        }
        {    // replay run 3's transcript up to the end of the commit phase: the commit root, theta, then per round its root and its alpha
            const lpc_out r3 = slot(commit_roots, fri_roots, final_polys, states, nonces, 3);
            transcript_type replay(seed);
            std::array<std::uint8_t, 32> d;
            std::memcpy(d.data(), r3.commit_root, 32);
            replay(d);
            replay.challenge();
            for (std::size_t i = 0; i < 3; ++i) {
                std::memcpy(d.data(), r3.fri_roots + 32 * i, 32);
                replay(d);
                replay.challenge();
            }
            if (proof_of_work_hip<transcript_type>::verify(replay, *r3.nonce, mask)) *flags |= 1;
            if (std::memcmp(replay.state().data(), r3.state, 32) == 0) *flags |= 2;
        }
        try {
            counting_transcript tr(seed);
            std::uint8_t root[32], fri[96], state[32];
            std::uint64_t fin[4 * 32];
            std::uint32_t nonce = 0;
            lpc_run(ctx, on, evals, point, tr, lpc_out {root, fri, state, fin, &nonce});
        } catch (const std::invalid_argument &) {
            *flags |= 4;
        }
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "pow_lpc_run: %s\n", e.what());
        return -100;
    }
}

}    // extern "C"
