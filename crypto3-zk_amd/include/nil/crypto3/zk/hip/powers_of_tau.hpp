//---------------------------------------------------------------------------//
// zkhip shim: the Lagrange-basis transform of a powers-of-tau accumulator, on the MI355X.
//
// Mirrors evaluation_domain<Fr, G>::evaluate_all_lagrange_polynomials(powers_begin, powers_end) as
// powers_of_tau_result::from_accumulator calls it for coeffs_g1 / coeffs_g2 / alpha_coeffs_g1 / beta_coeffs_g1
// (zk/commitments/detail/polynomial/powers_of_tau/result.hpp:81-94): given P_i = tau^i G for i < m (m a power of two)
// it returns L_j(tau) G for every Lagrange polynomial of the m-point domain -- an inverse DFT over group elements.
// `omega` is the primitive m-th root of unity of that domain (math::make_evaluation_domain's choice).
//
// The step BEFORE it, a participant's contribution: transform_accumulator does what powers_of_tau_accumulator::transform does
// (powers_of_tau/accumulator.hpp:89-121) -- every entry of tau_powers_g1 / tau_powers_g2 / alpha_tau_powers_g1 / beta_tau_powers_g1
// multiplied by tau^i, tau^i, alpha tau^i, beta tau^i -- with one scalar multiplication per point on the device
// (zkhip_bases_scale_geometric) instead of the reference's loop on one host thread.  merge_pairs / power_pairs are the two multiexps of
// the contribution check (detail/polynomial/vector_pairs.hpp:30-71) as ONE zkhip_msm_batch_dev over the same resident scalars; the pairing
// comparison that follows them stays the caller's.
//---------------------------------------------------------------------------//
#ifndef ZKHIP_SHIM_POWERS_OF_TAU_HPP
#define ZKHIP_SHIM_POWERS_OF_TAU_HPP

#include <iterator>
#include <stdexcept>
#include <utility>
#include <vector>

#include "fr_vector.hpp"
#include "multiexp.hpp"

namespace nil {
namespace crypto3 {
namespace zk {
namespace hip {

template <typename CurveType, int Group, typename InputIt>
std::vector<typename detail::jac_result<CurveType, Group>::type>
    evaluate_all_lagrange_polynomials(const context &ctx, InputIt powers_begin, InputIt powers_end,
                                      const typename curve_adapter<CurveType>::scalar_value_type &omega) {
    typedef curve_adapter<CurveType> adapter;
    typedef detail::jac_result<CurveType, Group> R;
    const std::size_t m = std::distance(powers_begin, powers_end), cl = R::limbs / 3;
    const std::size_t log_m = detail::ceil_log2(m);
    if (m == 0 || ((std::size_t)1 << log_m) != m) throw std::runtime_error("evaluate_all_lagrange_polynomials: the domain size must be a power of two");
    /* canonical Jacobian (x, y, 1) of every power; (0, 0, 0) for the point at infinity */
    std::vector<std::uint64_t> jac(m * R::limbs, 0);
    std::size_t i = 0;
    for (InputIt it = powers_begin; it != powers_end; ++it, ++i)
        if (adapter::point_to_affine_limbs(*it, &jac[i * R::limbs])) jac[i * R::limbs + 2 * cl] = 1;
    auto d = ctx.alloc(jac.size() * 8);
    ctx.h2d(d.get(), jac.data(), jac.size() * 8);
    ZKHIP_CALL(ctx, zkhip_ec_ntt_dev, adapter::id, Group, d.get(), log_m, limbs_of<adapter>(omega).data(), 1);
    ctx.d2h(jac.data(), d.get(), jac.size() * 8);
    std::vector<typename R::type> out;
    for (i = 0; i < m; ++i) out.push_back(R::make(&jac[i * R::limbs]));
    return out;
}

namespace detail {
    /// v[i] <- coeff * ratio^i * v[i] (coeff == nullptr: 1): one upload, one zkhip_bases_scale_geometric, one download.  The upload carries no
    /// window tables ("msm_precompute" off for its duration): the points are multiplied once, not summed.
    template <typename CurveType, int Group, typename G>
    void scale_geometric_in_place(const context &ctx, std::vector<G> &v, const typename curve_adapter<CurveType>::scalar_value_type &ratio,
                                  const typename curve_adapter<CurveType>::scalar_value_type *coeff) {
        if (v.empty()) return;
        struct no_tables {
            const context &ctx;
            std::int64_t was;
            explicit no_tables(const context &c) : ctx(c), was(c.get_option("msm_precompute")) { ctx.set_option("msm_precompute", 0); }
            ~no_tables() { zkhip_set_option(ctx.get(), "msm_precompute", was); }
        };
        device_bases<CurveType, Group> out;
        {
            no_tables guard(ctx);
            const device_bases<CurveType, Group> in(ctx, v.begin(), v.end());
            out = in.scale_geometric(0, v.size(), ratio, coeff);
        }
        v = out.download();
    }
    /// the two sums of a pair check over scalars that are on the device already: one zkhip_msm_batch_dev, one download
    template <typename CurveType, int Group>
    std::pair<typename jac_result<CurveType, Group>::type, typename jac_result<CurveType, Group>::type>
        pair_sums(const context &ctx, const device_bases<CurveType, Group> &b1, std::size_t off1, const device_bases<CurveType, Group> &b2, std::size_t off2,
                  std::size_t n, const void *d_scalars) {
        typedef jac_result<CurveType, Group> R;
        auto d_out = ctx.alloc(2 * R::limbs * 8);
        const zkhip_bases *bases[2] = {b1.get(), b2.get()};
        const std::size_t offsets[2] = {off1, off2}, ns[2] = {n, n};
        const void *scalars[2] = {d_scalars, d_scalars};
        void *outs[2] = {d_out.get(), static_cast<char *>(d_out.get()) + R::limbs * 8};
        ZKHIP_CALL(ctx, zkhip_msm_batch_dev, 2, bases, offsets, ns, scalars, outs);
        std::uint64_t jac[2 * R::limbs];
        ctx.d2h(jac, d_out.get(), sizeof(jac));
        return std::make_pair(R::make(jac), R::make(jac + R::limbs));
    }
    /// `count` draws of a random source (a callable returning a scalar, as kimchi_pedersen_hip's RandomSource)
    template <typename Fr, typename RandomSource>
    std::vector<Fr> draw_scalars(RandomSource &random, std::size_t count) {
        std::vector<Fr> r;
        r.reserve(count);
        for (std::size_t i = 0; i < count; ++i) r.push_back(random());
        return r;
    }
}    // namespace detail

/// powers_of_tau_accumulator::transform(key) (powers_of_tau/accumulator.hpp:89-121).  Duck-typed: `acc` has the reference accumulator's five
/// public members (tau_powers_g1, tau_powers_g2, alpha_tau_powers_g1, beta_tau_powers_g1: vectors of group values; beta_g2), `key` has tau,
/// alpha and beta.  Four uploads, four scalings on the device (the exponents tau^i are built there too), four downloads; beta_g2 * beta is
/// one scalar multiplication and stays on the host.
template <typename Accumulator, typename PrivateKey>
void transform_accumulator(const context &ctx, Accumulator &acc, const PrivateKey &key) {
    typedef typename std::decay<decltype(acc.tau_powers_g1)>::type::value_type g1_value_type;
    typedef typename group_traits<g1_value_type>::curve_type curve_type;
    ZKHIP_REQUIRE_PAIRING(curve_type, "powers_of_tau_accumulator");
    typedef typename curve_adapter<curve_type>::scalar_value_type Fr;
    const Fr tau = key.tau, alpha = key.alpha, beta = key.beta;
    detail::scale_geometric_in_place<curve_type, ZKHIP_G1>(ctx, acc.tau_powers_g1, tau, nullptr);
    detail::scale_geometric_in_place<curve_type, ZKHIP_G2>(ctx, acc.tau_powers_g2, tau, nullptr);
    detail::scale_geometric_in_place<curve_type, ZKHIP_G1>(ctx, acc.alpha_tau_powers_g1, tau, &alpha);
    detail::scale_geometric_in_place<curve_type, ZKHIP_G1>(ctx, acc.beta_tau_powers_g1, tau, &beta);
    acc.beta_g2 = acc.beta_g2 * beta;
}

/// detail::merge_pairs (vector_pairs.hpp:30-63) with the random scalars given by the caller: (sum r_i v1[i], sum r_i v2[i]).  The reference
/// draws the r_i itself (algebra::random_element); here they are an argument -- a vector, or below a random source (anything callable without arguments that returns a scalar) -- so that a test can
/// replay them.  Two uploads, one scalar upload, both sums in one zkhip_msm_batch_dev.
template <typename CurveType, int Group, typename PointIt>
std::pair<typename detail::jac_result<CurveType, Group>::type, typename detail::jac_result<CurveType, Group>::type>
    merge_pairs(const context &ctx, PointIt v1_begin, PointIt v1_end, PointIt v2_begin, PointIt v2_end,
                const std::vector<typename curve_adapter<CurveType>::scalar_value_type> &random_scalars) {
    const std::size_t n = std::distance(v1_begin, v1_end);
    if ((std::size_t)std::distance(v2_begin, v2_end) != n || random_scalars.size() != n)
        throw std::invalid_argument("merge_pairs: the two vectors and the random scalars must have one length");
    if (n == 0) return {};
    const device_bases<CurveType, Group> b1(ctx, v1_begin, v1_end), b2(ctx, v2_begin, v2_end);
    auto d_r = ctx.alloc(n * 32);
    upload_scalars<curve_adapter<CurveType>>(ctx, d_r.get(), random_scalars.data(), n);
    return detail::pair_sums<CurveType, Group>(ctx, b1, 0, b2, 0, n, d_r.get());
}
template <typename CurveType, int Group, typename PointIt, typename RandomSource, typename = decltype(std::declval<RandomSource &>()())>
std::pair<typename detail::jac_result<CurveType, Group>::type, typename detail::jac_result<CurveType, Group>::type>
    merge_pairs(const context &ctx, PointIt v1_begin, PointIt v1_end, PointIt v2_begin, PointIt v2_end, RandomSource &random) {
    typedef typename curve_adapter<CurveType>::scalar_value_type Fr;
    return merge_pairs<CurveType, Group>(ctx, v1_begin, v1_end, v2_begin, v2_end, detail::draw_scalars<Fr>(random, std::distance(v1_begin, v1_end)));
}

/// detail::power_pairs (vector_pairs.hpp:65-71): the pair (s, s^x) of a vector of the form [1, x, x^2, ...] -- merge_pairs over v[0 .. n - 1)
/// and v[1 .. n).  Both ranges lie in ONE resident object: one upload of v, one scalar upload, one zkhip_msm_batch_dev.
template <typename CurveType, int Group>
std::pair<typename detail::jac_result<CurveType, Group>::type, typename detail::jac_result<CurveType, Group>::type>
    power_pairs(const context &ctx, const std::vector<typename detail::jac_result<CurveType, Group>::type> &v,
                const std::vector<typename curve_adapter<CurveType>::scalar_value_type> &random_scalars) {
    if (v.empty() || random_scalars.size() != v.size() - 1) throw std::invalid_argument("power_pairs: one random scalar per point but the last");
    const std::size_t n = v.size() - 1;
    if (n == 0) return {};
    const device_bases<CurveType, Group> b(ctx, v.begin(), v.end());
    auto d_r = ctx.alloc(n * 32);
    upload_scalars<curve_adapter<CurveType>>(ctx, d_r.get(), random_scalars.data(), n);
    return detail::pair_sums<CurveType, Group>(ctx, b, 0, b, 1, n, d_r.get());
}
template <typename CurveType, int Group, typename RandomSource, typename = decltype(std::declval<RandomSource &>()())>
std::pair<typename detail::jac_result<CurveType, Group>::type, typename detail::jac_result<CurveType, Group>::type>
    power_pairs(const context &ctx, const std::vector<typename detail::jac_result<CurveType, Group>::type> &v, RandomSource &random) {
    typedef typename curve_adapter<CurveType>::scalar_value_type Fr;
    if (v.empty()) throw std::invalid_argument("power_pairs: an empty vector");
    return power_pairs<CurveType, Group>(ctx, v, detail::draw_scalars<Fr>(random, v.size() - 1));
}

}    // namespace hip
}    // namespace zk
}    // namespace crypto3
}    // namespace nil

#endif    // ZKHIP_SHIM_POWERS_OF_TAU_HPP
