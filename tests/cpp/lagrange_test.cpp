// C++ shim test harness (test-only) of the Lagrange-basis SRS of kimchi_pedersen_hip over the stand-in `pallas` / `vesta` types:
// params_type::add_lagrange_basis for two domain sizes (an evaluation_domain_hip and a plain struct with size() and omega, as the
// reference's basic_radix2_domain offers them), lagrange_bases[n] handed back whole, the launches a repeated call makes, what throws, and
// commitment_evaluations next to commitment over the coefficients the Python driver computed for the same column.
// Built into liblagrangetest.so by tests/cpp/Makefile; driven by tests/test_gpu_lagrange_shim.py.
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include <nil/crypto3/zk/hip/evaluation_domain.hpp>
#include <nil/crypto3/zk/hip/kimchi_pedersen.hpp>

#include "harness_common.hpp"

using namespace nil::crypto3::zk::hip;
using harness::list_random;
using harness::throws_invalid;

namespace {

struct no_sponge { };
struct no_group_map { };

/// what add_lagrange_basis reads of a domain, and nothing else
template <typename Fr>
struct plain_domain {
    std::size_t m;
    Fr omega;
    std::size_t size() const { return m; }
};

std::uint64_t launches(const context &ctx) {
    double ms = 0;
    std::uint64_t count = 0;
    check(zkhip_profile_get(ctx.get(), "", &ms, &count), "zkhip_profile_get", ctx.get());
    return count;
}

template <typename Curve>
int lagrange_run_t(const std::uint64_t *sizes, const std::uint64_t *g_xy, const std::uint64_t *h_xy, const std::uint64_t *omegas, const std::uint64_t *evals,
                   const std::uint64_t *coeffs, const std::uint64_t *draws, std::uint64_t *big_xy, std::uint8_t *big_inf, std::uint64_t *small_xy,
                   std::uint8_t *small_inf, std::uint64_t *commit_xy, std::uint64_t *counts) {
    typedef curve_adapter<Curve> A;
    typedef typename A::scalar_value_type Fr;
    typedef typename A::g1_value_type G;
    typedef kimchi_pedersen_hip<Curve, no_sponge, no_group_map, list_random<Curve>> scheme;
    const std::size_t n = sizes[0], big = sizes[1], small = sizes[2], ndraws = sizes[3];
    context ctx(0);
    list_random<Curve> random = {draws, ndraws};
    std::vector<G> g;
    for (std::size_t i = 0; i < n; ++i) g.push_back(G::from_affine(g_xy + 8 * i, false));
    typename scheme::params_type params(ctx, random, g.begin(), g.end(), G::from_affine(h_xy), Fr::one());

    check(zkhip_profile_enable(ctx.get(), 1), "zkhip_profile_enable", ctx.get());
    const evaluation_domain_hip<Curve> big_domain(ZKHIP_DOMAIN_BASIC_RADIX2, big, A::scalar_from_limbs(omegas));
    const plain_domain<Fr> small_domain = {small, A::scalar_from_limbs(omegas + 4)};
    params.add_lagrange_basis(big_domain);
    params.add_lagrange_basis(small_domain);
    counts[0] = launches(ctx);
    params.add_lagrange_basis(big_domain);    // already there: nothing is launched
    params.add_lagrange_basis(small_domain);
    counts[1] = launches(ctx);
    check(zkhip_profile_enable(ctx.get(), 0), "zkhip_profile_enable", ctx.get());
    counts[2] = params.lagrange_bases.size();

    const std::vector<G> &lb = params.lagrange_bases.at(big), &ls = params.lagrange_bases.at(small);
    if (lb.size() != big || ls.size() != small) return -31;
    for (std::size_t i = 0; i < big; ++i) big_inf[i] = A::point_to_affine_limbs(lb[i], big_xy + 8 * i) ? 0 : 1;
    for (std::size_t i = 0; i < small; ++i) small_inf[i] = A::point_to_affine_limbs(ls[i], small_xy + 8 * i) ? 0 : 1;

    // a domain larger than |g|, and one that is not a power of two: both throw and add nothing
    counts[3] = throws_invalid([&] { params.add_lagrange_basis(plain_domain<Fr> {2 * params.padded, A::scalar_from_limbs(omegas + 4)}); });
    counts[4] = throws_invalid([&] { params.add_lagrange_basis(plain_domain<Fr> {small + 1, A::scalar_from_limbs(omegas + 4)}); });
    if (params.lagrange_bases.size() != 2) return -32;

    // the column: its evaluations over the big domain through the Lagrange bases, its coefficients through commitment (hiding: + w h)
    std::vector<Fr> ev, co;
    for (std::size_t i = 0; i < big; ++i) ev.push_back(A::scalar_from_limbs(evals + 4 * i)), co.push_back(A::scalar_from_limbs(coeffs + 4 * i));
    const typename scheme::commitment_type by_evals = scheme::commitment_evaluations(params, ev);
    if (by_evals.unshifted.size() != 1 || !by_evals.shifted.is_zero()) return -33;
    counts[5] = A::point_to_affine_limbs(by_evals.unshifted[0], commit_xy) ? 0 : 1;
    const auto [hiding, blind] = scheme::commitment(params, co, -1);
    if (hiding.unshifted.size() != 1 || blind.unshifted.size() != 1) return -34;
    counts[6] = A::point_to_affine_limbs(hiding.unshifted[0], commit_xy + 8) ? 0 : 1;
    A::scalar_to_limbs(blind.unshifted[0], commit_xy + 16);
    counts[7] = random.pos;
    // a size that was not added
    counts[8] = throws_invalid([&] { (void)scheme::commitment_evaluations(params, std::vector<Fr>(2 * small, Fr::one())); });
    counts[9] = ctx.device_status();
    return 0;
}

}    // namespace

extern "C" {

/// sizes: |g|, the two domain sizes, the number of draws.  omegas: the roots of the two domains.
/// commit_xy: commitment_evaluations' point, commitment's unshifted[0], its blinder (4 limbs).  counts (10): launches after the two
/// bases were added / after both were added again, lagrange_bases.size(), threw for a domain larger than |g| / not a power of two,
/// the two points' infinity flags, draws consumed, threw for a size that was not added, zkhip_device_status
int lagrange_run(int curve, const std::uint64_t *sizes, const std::uint64_t *g_xy, const std::uint64_t *h_xy, const std::uint64_t *omegas, const std::uint64_t *evals,
                 const std::uint64_t *coeffs, const std::uint64_t *draws, std::uint64_t *big_xy, std::uint8_t *big_inf, std::uint64_t *small_xy, std::uint8_t *small_inf,
                 std::uint64_t *commit_xy, std::uint64_t *counts) {
    return harness::guarded(__func__, [&] {
        if (curve == ZKHIP_PALLAS) return lagrange_run_t<pallas>(sizes, g_xy, h_xy, omegas, evals, coeffs, draws, big_xy, big_inf, small_xy, small_inf, commit_xy, counts);
        if (curve == ZKHIP_VESTA) return lagrange_run_t<vesta>(sizes, g_xy, h_xy, omegas, evals, coeffs, draws, big_xy, big_inf, small_xy, small_inf, commit_xy, counts);
        return -2;
    }, -100);
}

}    // extern "C"
