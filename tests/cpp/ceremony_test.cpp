// C++ shim test harness (test-only) of the setup ceremonies over the stand-in `bls12_381` / `alt_bn128_254` types: transform_accumulator
// (powers_of_tau.hpp) on an accumulator with the reference's five members, starting from the reference's initial one (every entry the
// generator) and applying one key after the other; power_pairs / merge_pairs with the caller's random scalars as a vector and as a random
// source; contribute_randomness (r1cs_gg_ppzksnark_mpc.hpp) on a keypair with the members transform_keypair touches.
// Built into libceremonytest.so by tests/cpp/Makefile; driven by tests/test_gpu_ceremony_shim.py.
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <utility>
#include <vector>

#include <nil/crypto3/zk/hip/powers_of_tau.hpp>
#include <nil/crypto3/zk/hip/r1cs_gg_ppzksnark_mpc.hpp>

#include "harness_common.hpp"

using namespace nil::crypto3::zk::hip;
using harness::list_random;
using harness::read_points;
using harness::write_points;

namespace {

// what transform_accumulator reads of powers_of_tau_accumulator and powers_of_tau_private_key, and nothing else
template <typename Curve>
struct accumulator {
    typedef typename curve_adapter<Curve>::g1_value_type g1_value_type;
    typedef typename curve_adapter<Curve>::g2_value_type g2_value_type;
    std::vector<g1_value_type> tau_powers_g1;
    std::vector<g2_value_type> tau_powers_g2;
    std::vector<g1_value_type> alpha_tau_powers_g1;
    std::vector<g1_value_type> beta_tau_powers_g1;
    g2_value_type beta_g2;
    accumulator(std::size_t length, const g1_value_type &one1, const g2_value_type &one2) :
        tau_powers_g1(2 * length - 1, one1), tau_powers_g2(length, one2), alpha_tau_powers_g1(length, one1), beta_tau_powers_g1(length, one1), beta_g2(one2) { }
};
template <typename Curve>
struct tau_private_key {
    typename curve_adapter<Curve>::scalar_value_type tau, alpha, beta;
};
// what contribute_randomness reads of r1cs_gg_ppzksnark's keypair and the mpc private key
template <typename Curve>
struct proving_key {
    typename curve_adapter<Curve>::g1_value_type delta_g1;
    typename curve_adapter<Curve>::g2_value_type delta_g2;
    std::vector<typename curve_adapter<Curve>::g1_value_type> H_query, L_query;
};
template <typename Curve>
struct verification_key {
    typename curve_adapter<Curve>::g2_value_type delta_g2;
};
template <typename Curve>
struct mpc_private_key {
    typename curve_adapter<Curve>::scalar_value_type delta;
};

template <typename Curve>
int transform_t(std::size_t length, const std::uint64_t *gen1, const std::uint64_t *gen2, const std::uint64_t *keys, std::size_t nkeys, std::uint64_t *xy,
                std::uint8_t *inf) {
    typedef curve_adapter<Curve> A;
    typedef typename A::g2_value_type G2;
    context ctx(0);
    accumulator<Curve> acc(length, A::g1_value_type::from_affine(gen1), G2::from_affine(gen2));
    for (std::size_t k = 0; k < nkeys; ++k) {
        const tau_private_key<Curve> key = {A::scalar_from_limbs(keys + 12 * k), A::scalar_from_limbs(keys + 12 * k + 4), A::scalar_from_limbs(keys + 12 * k + 8)};
        transform_accumulator(ctx, acc, key);
    }
    if (acc.tau_powers_g1.size() != 2 * length - 1 || acc.tau_powers_g2.size() != length || acc.alpha_tau_powers_g1.size() != length ||
        acc.beta_tau_powers_g1.size() != length)
        return -31;
    write_points(acc.tau_powers_g1, xy, inf);
    write_points(acc.tau_powers_g2, xy, inf);
    write_points(acc.alpha_tau_powers_g1, xy, inf);
    write_points(acc.beta_tau_powers_g1, xy, inf);
    write_points(std::vector<G2> {acc.beta_g2}, xy, inf);
    return ctx.device_status() == 0 ? 0 : -32;
}

template <typename Curve, int Group>
int pairs_t(int mode, std::size_t n, const std::uint64_t *v_xy, const std::uint8_t *v_inf, const std::uint64_t *scalars, std::uint64_t *xy, std::uint8_t *inf) {
    typedef curve_adapter<Curve> A;
    typedef typename detail::jac_result<Curve, Group>::type G;
    context ctx(0);
    const std::vector<G> v = read_points<G>(v_xy, v_inf, n);
    std::vector<typename A::scalar_value_type> r;
    for (std::size_t i = 0; i + 1 < n; ++i) r.push_back(A::scalar_from_limbs(scalars + 4 * i));
    list_random<Curve> random = {scalars, n - 1};
    std::pair<G, G> res;
    if (mode == 0) res = power_pairs<Curve, Group>(ctx, v, r);
    else if (mode == 1) res = power_pairs<Curve, Group>(ctx, v, random);
    else if (mode == 2) res = merge_pairs<Curve, Group>(ctx, v.begin(), v.end() - 1, v.begin() + 1, v.end(), r);
    else res = merge_pairs<Curve, Group>(ctx, v.begin(), v.end() - 1, v.begin() + 1, v.end(), random);
    if ((mode == 1 || mode == 3) && random.pos != n - 1) return -41;
    write_points(std::vector<G> {res.first, res.second}, xy, inf);
    // lengths that do not belong together throw
    r.pop_back();
    if (!harness::throws_invalid([&] { (void)power_pairs<Curve, Group>(ctx, v, r); })) return -42;
    return ctx.device_status() == 0 ? 0 : -43;
}

template <typename Curve>
int mpc_t(std::size_t nh, std::size_t nl, const std::uint64_t *h_xy, const std::uint8_t *h_inf, const std::uint64_t *l_xy, const std::uint8_t *l_inf,
          const std::uint64_t *delta_g1, const std::uint64_t *delta_g2, const std::uint64_t *delta, std::uint64_t *xy, std::uint8_t *inf) {
    typedef curve_adapter<Curve> A;
    typedef typename A::g1_value_type G1;
    typedef typename A::g2_value_type G2;
    context ctx(0);
    std::pair<proving_key<Curve>, verification_key<Curve>> keypair;
    keypair.first.delta_g1 = G1::from_affine(delta_g1);
    keypair.first.delta_g2 = keypair.second.delta_g2 = G2::from_affine(delta_g2);
    keypair.first.H_query = read_points<G1>(h_xy, h_inf, nh);
    keypair.first.L_query = read_points<G1>(l_xy, l_inf, nl);
    const mpc_private_key<Curve> key = {A::scalar_from_limbs(delta)};
    contribute_randomness(ctx, keypair, key);
    if (keypair.first.H_query.size() != nh || keypair.first.L_query.size() != nl) return -51;
    write_points(keypair.first.H_query, xy, inf);
    write_points(keypair.first.L_query, xy, inf);
    write_points(std::vector<G1> {keypair.first.delta_g1}, xy, inf);
    write_points(std::vector<G2> {keypair.first.delta_g2, keypair.second.delta_g2}, xy, inf);
    return ctx.device_status() == 0 ? 0 : -52;
}

}    // namespace

extern "C" {

/// the reference's initial accumulator of `length` powers (gen1 / gen2: the generators, canonical affine) after `nkeys` contributions in turn
/// (keys: tau | alpha | beta per key, 4 limbs each).  xy / inf: tau_powers_g1 (2 length - 1 points), tau_powers_g2 (length),
/// alpha_tau_powers_g1, beta_tau_powers_g1 (length each), beta_g2, one after the other (a G2 point takes twice the limbs of a G1 point)
int ceremony_transform(int curve, std::size_t length, const std::uint64_t *gen1, const std::uint64_t *gen2, const std::uint64_t *keys, std::size_t nkeys,
                       std::uint64_t *xy, std::uint8_t *inf) {
    return harness::guarded(__func__, [&] {
        if (curve == ZKHIP_BLS12_381) return transform_t<bls12_381>(length, gen1, gen2, keys, nkeys, xy, inf);
        if (curve == ZKHIP_BN254) return transform_t<alt_bn128_254>(length, gen1, gen2, keys, nkeys, xy, inf);
        return -2;
    }, -100);
}

/// mode 0 / 1: power_pairs over the n points with the n - 1 scalars as a vector / drawn from a random source; 2 / 3: merge_pairs over the
/// ranges [0, n - 1) and [1, n) likewise.  xy / inf: the two sums
int ceremony_pairs(int curve, int group, int mode, std::size_t n, const std::uint64_t *v_xy, const std::uint8_t *v_inf, const std::uint64_t *scalars,
                   std::uint64_t *xy, std::uint8_t *inf) {
    return harness::guarded(__func__, [&] {
        if (curve == ZKHIP_BLS12_381 && group == ZKHIP_G1) return pairs_t<bls12_381, ZKHIP_G1>(mode, n, v_xy, v_inf, scalars, xy, inf);
        if (curve == ZKHIP_BLS12_381 && group == ZKHIP_G2) return pairs_t<bls12_381, ZKHIP_G2>(mode, n, v_xy, v_inf, scalars, xy, inf);
        if (curve == ZKHIP_BN254 && group == ZKHIP_G1) return pairs_t<alt_bn128_254, ZKHIP_G1>(mode, n, v_xy, v_inf, scalars, xy, inf);
        if (curve == ZKHIP_BN254 && group == ZKHIP_G2) return pairs_t<alt_bn128_254, ZKHIP_G2>(mode, n, v_xy, v_inf, scalars, xy, inf);
        return -2;
    }, -100);
}

/// contribute_randomness on a keypair with H_query (nh points), L_query (nl points), delta_g1 and delta_g2 (the proving key's and the
/// verification key's copy start equal).  xy / inf: H_query, L_query, delta_g1, the proving key's delta_g2, the verification key's delta_g2
int ceremony_mpc(int curve, std::size_t nh, std::size_t nl, const std::uint64_t *h_xy, const std::uint8_t *h_inf, const std::uint64_t *l_xy, const std::uint8_t *l_inf,
                 const std::uint64_t *delta_g1, const std::uint64_t *delta_g2, const std::uint64_t *delta, std::uint64_t *xy, std::uint8_t *inf) {
    return harness::guarded(__func__, [&] {
        if (curve == ZKHIP_BLS12_381) return mpc_t<bls12_381>(nh, nl, h_xy, h_inf, l_xy, l_inf, delta_g1, delta_g2, delta, xy, inf);
        if (curve == ZKHIP_BN254) return mpc_t<alt_bn128_254>(nh, nl, h_xy, h_inf, l_xy, l_inf, delta_g1, delta_g2, delta, xy, inf);
        return -2;
    }, -100);
}

}    // extern "C"
