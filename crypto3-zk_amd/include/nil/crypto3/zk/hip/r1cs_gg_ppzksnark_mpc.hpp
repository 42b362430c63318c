//---------------------------------------------------------------------------//
// zkhip shim: a participant's contribution to the circuit-specific phase of the Groth16 setup ceremony, on the MI355X.
//
// Mirrors detail::transform_keypair (zk/commitments/detail/polynomial/r1cs_gg_ppzksnark_mpc/crs_operations.hpp:109-129): every point of
// H_query and L_query is multiplied by delta^-1, delta_g1 and both copies of delta_g2 by delta.  The two queries are the cost -- one
// scalar multiplication per point, a loop on one host thread in the reference -- and go through zkhip_bases_scale_geometric with
// ratio = 1, coeff = delta^-1 (every point by the same scalar); the three single points stay on the host.
//---------------------------------------------------------------------------//
#ifndef ZKHIP_SHIM_R1CS_GG_PPZKSNARK_MPC_HPP
#define ZKHIP_SHIM_R1CS_GG_PPZKSNARK_MPC_HPP

#include "powers_of_tau.hpp"

namespace nil {
namespace crypto3 {
namespace zk {
namespace hip {

/// Duck-typed on the reference's types: keypair.first is the proving key (H_query, L_query: vectors of G1 values; delta_g1, delta_g2),
/// keypair.second the verification key (delta_g2); private_key.delta is a scalar with inversed().
template <typename Keypair, typename PrivateKey>
void contribute_randomness(const context &ctx, Keypair &keypair, const PrivateKey &private_key) {
    typedef typename std::decay<decltype(keypair.first.H_query)>::type::value_type g1_value_type;
    typedef typename group_traits<g1_value_type>::curve_type curve_type;
    ZKHIP_REQUIRE_PAIRING(curve_type, "r1cs_gg_ppzksnark_mpc");
    typedef typename curve_adapter<curve_type>::scalar_value_type Fr;
    const Fr delta = private_key.delta, delta_inv = delta.inversed(), one = Fr::one();
    detail::scale_geometric_in_place<curve_type, ZKHIP_G1>(ctx, keypair.first.H_query, one, &delta_inv);
    detail::scale_geometric_in_place<curve_type, ZKHIP_G1>(ctx, keypair.first.L_query, one, &delta_inv);
    keypair.first.delta_g1 = delta * keypair.first.delta_g1;
    keypair.first.delta_g2 = delta * keypair.first.delta_g2;
    keypair.second.delta_g2 = delta * keypair.second.delta_g2;
}

}    // namespace hip
}    // namespace zk
}    // namespace crypto3
}    // namespace nil

#endif    // ZKHIP_SHIM_R1CS_GG_PPZKSNARK_MPC_HPP
