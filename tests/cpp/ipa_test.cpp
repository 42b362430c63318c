// C++ shim test harness (test-only) of kimchi_pedersen_hip over the stand-in `pallas` / `vesta` types: one call commits to a list of
// polynomials, opens them, verifies the opening and then three tampered copies of it -- with a sponge that answers from a list and records
// every call, a group map that returns a fixed point and a random source that hands out a list, all given by the Python driver, which
// holds everything that comes back against tests/ipa_model.py.
// Built into libipatest.so by tests/cpp/Makefile; driven by tests/test_gpu_ipa_shim.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include <nil/crypto3/zk/hip/kimchi_pedersen.hpp>

#include "harness_common.hpp"

using namespace nil::crypto3::zk::hip;
using harness::list_random;

namespace {

enum : std::uint64_t { LOG_ABSORB_FR = 0, LOG_CHALLENGE_FQ = 1, LOG_ABSORB_G = 2, LOG_SQUEEZE = 3 };
struct log_entry {
    std::uint64_t kind, inf, data[8];
};

template <typename Curve>
struct list_sponge {
    typedef curve_adapter<Curve> A;
    typedef typename A::scalar_value_type Fr;
    const std::uint64_t *answers = nullptr;
    std::size_t count = 0, pos = 0;
    std::vector<log_entry> *log = nullptr;

    static Fr shift_scalar(const Fr &x) { return x + Fr::one(); }    // the model's stand-in for kimchi_functions::shift_scalar
    void record(std::uint64_t kind, const Fr *x) {
        log_entry e = {kind, 0, {}};
        if (x) A::scalar_to_limbs(*x, e.data);
        log->push_back(e);
    }
    Fr answer() {
        if (pos >= count) throw std::out_of_range("list_sponge: out of answers");
        return A::scalar_from_limbs(answers + 4 * pos++);
    }
    void absorb_fr(const Fr &x) { record(LOG_ABSORB_FR, &x); }
    void absorb_g(const typename A::g1_value_type &p) {
        log_entry e = {LOG_ABSORB_G, 0, {}};
        e.inf = A::point_to_affine_limbs(p, e.data) ? 0 : 1;
        log->push_back(e);
    }
    Fr challenge_fq() {
        record(LOG_CHALLENGE_FQ, nullptr);
        return answer();
    }
    Fr squeeze_challenge(const Fr &endo_r) {
        record(LOG_SQUEEZE, &endo_r);
        return answer();
    }
};

template <typename Curve>
struct fixed_group_map {
    typename curve_adapter<Curve>::g1_value_type u;
    template <typename T>
    typename curve_adapter<Curve>::g1_value_type to_group(const T &) const { return u; }
};

struct ipa_io {
    // in
    std::size_t n;
    const std::uint64_t *g_xy;
    const std::uint8_t *g_inf;
    const std::uint64_t *h_xy, *u_xy, *endo_r;
    std::size_t npolys;
    const std::uint64_t *poly_len;
    const std::int64_t *poly_bound;
    const std::uint64_t *coeffs;
    std::size_t npoints;
    const std::uint64_t *elm, *scales /* polyscale, evalscale */, *evals /* [poly][point][chunk] */;
    const std::uint64_t *draws;
    std::size_t ndraws;
    const std::uint64_t *answers;
    std::size_t nanswers;
    // out
    std::uint64_t *comm_xy, *comm_inf, *comm_count, *blind;    // per polynomial: its unshifted chunks, then the shifted slot
    std::uint64_t *lr_xy, *lr_inf, *tail_xy /* delta, sg */, *tail_inf, *z /* z1, z2 */;
    std::uint64_t *log, *counts;
    std::size_t log_cap;
};

template <typename Curve>
int ipa_run_t(const ipa_io &io) {
    typedef curve_adapter<Curve> A;
    typedef typename A::scalar_value_type Fr;
    typedef typename A::g1_value_type G;
    typedef kimchi_pedersen_hip<Curve, list_sponge<Curve>, fixed_group_map<Curve>, list_random<Curve>> scheme;
    context ctx(0);
    list_random<Curve> random = {io.draws, io.ndraws};
    std::vector<G> g;
    for (std::size_t i = 0; i < io.n; ++i) g.push_back(G::from_affine(io.g_xy + 8 * i, io.g_inf[i] != 0));
    typename scheme::params_type params(ctx, random, g.begin(), g.end(), G::from_affine(io.h_xy), A::scalar_from_limbs(io.endo_r));
    fixed_group_map<Curve> group_map = {G::from_affine(io.u_xy)};

    // commitments
    typename scheme::poly_type plms;
    std::vector<typename scheme::evaluation_type> evaluation;
    std::size_t at = 0, slot = 0, ev = 0;
    for (std::size_t p = 0; p < io.npolys; ++p) {
        std::vector<Fr> coeffs;
        for (std::size_t i = 0; i < io.poly_len[p]; ++i) coeffs.push_back(A::scalar_from_limbs(io.coeffs + 4 * (at + i)));
        at += io.poly_len[p];
        const auto [commit, blind] = scheme::commitment(params, coeffs, (int)io.poly_bound[p]);
        io.comm_count[p] = commit.unshifted.size();
        for (std::size_t k = 0; k <= commit.unshifted.size(); ++k, ++slot) {
            const bool shifted = k == commit.unshifted.size();
            io.comm_inf[slot] = A::point_to_affine_limbs(shifted ? commit.shifted : commit.unshifted[k], io.comm_xy + 8 * slot) ? 0 : 1;
            A::scalar_to_limbs(shifted ? blind.shifted : blind.unshifted[k], io.blind + 4 * slot);
        }
        plms.emplace_back(coeffs, (int)io.poly_bound[p], blind);
        std::vector<std::vector<Fr>> evals(io.npoints);
        for (std::size_t j = 0; j < io.npoints; ++j)
            for (std::size_t k = 0; k < commit.unshifted.size(); ++k) evals[j].push_back(A::scalar_from_limbs(io.evals + 4 * ev++));
        evaluation.emplace_back(commit, evals, (int)io.poly_bound[p]);
    }
    io.counts[2] = random.pos;

    // the opening
    std::vector<Fr> elm;
    for (std::size_t j = 0; j < io.npoints; ++j) elm.push_back(A::scalar_from_limbs(io.elm + 4 * j));
    const Fr polyscale = A::scalar_from_limbs(io.scales), evalscale = A::scalar_from_limbs(io.scales + 4);
    std::vector<log_entry> prover_log, verifier_log, scratch_log;
    list_sponge<Curve> fresh;
    fresh.answers = io.answers, fresh.count = io.nanswers;
    list_sponge<Curve> sponge = fresh;
    sponge.log = &prover_log;
    const typename scheme::proof_type proof = scheme::proof_eval(params, group_map, plms, elm, polyscale, evalscale, sponge);
    io.counts[3] = random.pos;
    for (std::size_t i = 0; i < proof.lr.size(); ++i) {
        io.lr_inf[2 * i] = A::point_to_affine_limbs(std::get<0>(proof.lr[i]), io.lr_xy + 16 * i) ? 0 : 1;
        io.lr_inf[2 * i + 1] = A::point_to_affine_limbs(std::get<1>(proof.lr[i]), io.lr_xy + 16 * i + 8) ? 0 : 1;
    }
    io.counts[10] = proof.lr.size();
    io.tail_inf[0] = A::point_to_affine_limbs(proof.delta, io.tail_xy) ? 0 : 1;
    io.tail_inf[1] = A::point_to_affine_limbs(proof.sg, io.tail_xy + 8) ? 0 : 1;
    A::scalar_to_limbs(proof.z1, io.z);
    A::scalar_to_limbs(proof.z2, io.z + 4);

    // verify_eval: the proof as it is, then with z2, the first L and sg changed
    auto verify = [&](const typename scheme::proof_type &opening, std::vector<log_entry> &log) {
        typename scheme::batchproof_type batch = {fresh, evaluation, elm, polyscale, evalscale, opening};
        batch.sponge.log = &log;
        std::vector<typename scheme::batchproof_type> batches = {batch};
        return scheme::verify_eval(params, group_map, batches) ? 1u : 0u;
    };
    io.counts[5] = verify(proof, verifier_log);
    io.counts[4] = random.pos;
    typename scheme::proof_type bad = proof;
    bad.z2 = bad.z2 + Fr::one();
    io.counts[6] = verify(bad, scratch_log);
    bad = proof;
    if (!bad.lr.empty()) {
        std::get<0>(bad.lr[0]) = std::get<0>(bad.lr[0]) + params.h;
        io.counts[7] = verify(bad, scratch_log);
    } else {
        io.counts[7] = 2;    // no round, no L
    }
    bad = proof;
    bad.sg = bad.sg + params.h;
    io.counts[8] = verify(bad, scratch_log);
    io.counts[9] = ctx.device_status();

    io.counts[0] = prover_log.size();
    io.counts[1] = verifier_log.size();
    if (prover_log.size() + verifier_log.size() > io.log_cap) return -30;
    std::size_t w = 0;
    for (const auto *log : {&prover_log, &verifier_log})
        for (const log_entry &e : *log) {
            io.log[10 * w] = e.kind;
            io.log[10 * w + 1] = e.inf;
            std::memcpy(io.log + 10 * w + 2, e.data, 64);
            ++w;
        }
    return 0;
}

}    // namespace

extern "C" {

/// sizes: n, npolys, npoints, ndraws, nanswers, log_cap.  counts (11): prover log entries, verifier log entries, draws consumed after the
/// commitments / after proof_eval / after the first verify_eval, verify_eval of the proof, of the proof with z2 / L_0 / sg changed (2: no L),
/// zkhip_device_status, rounds
int ipa_run(int curve, const std::uint64_t *sizes, const std::uint64_t *g_xy, const std::uint8_t *g_inf, const std::uint64_t *h_xy, const std::uint64_t *u_xy,
            const std::uint64_t *endo_r, const std::uint64_t *poly_len, const std::int64_t *poly_bound, const std::uint64_t *coeffs, const std::uint64_t *elm,
            const std::uint64_t *scales, const std::uint64_t *evals, const std::uint64_t *draws, const std::uint64_t *answers, std::uint64_t *comm_xy,
            std::uint64_t *comm_inf, std::uint64_t *comm_count, std::uint64_t *blind, std::uint64_t *lr_xy, std::uint64_t *lr_inf, std::uint64_t *tail_xy,
            std::uint64_t *tail_inf, std::uint64_t *z, std::uint64_t *log, std::uint64_t *counts) {
    const ipa_io io = {sizes[0], g_xy,   g_inf,  h_xy,     u_xy,     endo_r,   sizes[1],   poly_len, poly_bound, coeffs, sizes[2], elm,    scales,  evals,
                       draws,    sizes[3], answers, sizes[4], comm_xy, comm_inf, comm_count, blind,    lr_xy,      lr_inf, tail_xy,  tail_inf, z,     log,
                       counts,   sizes[5]};
    return harness::guarded(__func__, [&] {
        if (curve == ZKHIP_PALLAS) return ipa_run_t<pallas>(io);
        if (curve == ZKHIP_VESTA) return ipa_run_t<vesta>(io);
        return -2;
    }, -100);
}

}    // extern "C"
