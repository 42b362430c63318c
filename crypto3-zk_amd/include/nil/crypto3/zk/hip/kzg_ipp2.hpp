//---------------------------------------------------------------------------//
// zkhip shim: the inner pairing product commitments of Groth16 aggregation (SnarkPack / TIPP-MIPP), on the MI355X.
//
// Mirrors commitments::kzg_ipp2<CurveType> (zk/commitments/polynomial/kzg_ipp2.hpp:100-283) with the reference's names --
// commitment_key (a, b, has_correct_len), vkey_type, wkey_type, output_type, pair, single -- and gives the product shape of the GIPA
// rounds (ipp2/prover.hpp:360-381 zab_l / zab_r, :584-593 ip_ab) as the free function pairing_inner_product_hip.  Every product is
// final_exponentiation(prod_i miller(A_i, B_i)) computed by ONE zkhip_pairing_products call: `pair` is four terms into two outputs,
// `single` two terms into two outputs, an inner product one term.
//
// Keys are RESIDENT: a commitment_key holds two device_bases, built from the powers of the key scalars on the device
// (from_scalar_powers: what structured_generators_scalar_power computes on the host, ipp2/srs.hpp:44-56) or uploaded from host values.
// The committed vectors are taken as host values (iterators of the adapter's point types: uploaded, used, freed) or as resident
// device_bases (the next round's folded vectors).  Where the reference asserts a length (BOOST_ASSERT), this throws std::invalid_argument.
// Values of the target group come back through curve_adapter::gt_from_limbs (algebra.hpp).  BLS12-381 only, as the entry is.
//---------------------------------------------------------------------------//
#ifndef ZKHIP_SHIM_KZG_IPP2_HPP
#define ZKHIP_SHIM_KZG_IPP2_HPP

#include <iterator>
#include <stdexcept>
#include <utility>
#include <vector>

#include "backend.hpp"

namespace nil {
namespace crypto3 {
namespace zk {
namespace hip {

namespace detail {
    /// one zkhip_pairing_products call; the outputs as the adapter's target-group values
    template <typename CurveType>
    std::vector<typename curve_adapter<CurveType>::gt_value_type> pairing_products(const context &ctx, const std::vector<zkhip_pairing_term> &terms,
                                                                                   std::size_t n_out) {
        typedef curve_adapter<CurveType> adapter;
        std::vector<std::uint64_t> limbs(n_out * 72);
        ZKHIP_CALL(ctx, zkhip_pairing_products, adapter::id, terms.data(), terms.size(), n_out, limbs.data());
        std::vector<typename adapter::gt_value_type> out;
        out.reserve(n_out);
        for (std::size_t k = 0; k < n_out; ++k) out.push_back(adapter::gt_from_limbs(&limbs[k * 72]));
        return out;
    }
    template <typename CurveType>
    zkhip_pairing_term pairing_term(const device_bases<CurveType, ZKHIP_G1> &g1, const device_bases<CurveType, ZKHIP_G2> &g2, std::size_t n, std::uint32_t out) {
        zkhip_pairing_term t;
        t.g1 = g1.get(), t.g1_offset = 0;
        t.g2 = g2.get(), t.g2_offset = 0;
        t.n = n, t.out = out;
        return t;
    }
}    // namespace detail

/// final_exponentiation(prod_i miller(a_i, b_i)) over two resident vectors of the same length: ip_ab, zab_l, zab_r
template <typename CurveType>
typename curve_adapter<CurveType>::gt_value_type pairing_inner_product_hip(const context &ctx, const device_bases<CurveType, ZKHIP_G1> &a,
                                                                           const device_bases<CurveType, ZKHIP_G2> &b) {
    ZKHIP_REQUIRE_PAIRING(CurveType, "pairing_inner_product_hip");
    if (a.size() != b.size()) throw std::invalid_argument("pairing_inner_product_hip: the two vectors differ in length");
    return detail::pairing_products<CurveType>(ctx, {detail::pairing_term<CurveType>(a, b, a.size(), 0)}, 1)[0];
}

template <typename CurveType>
class kzg_ipp2_hip {
    ZKHIP_REQUIRE_PAIRING(CurveType, "kzg_ipp2_hip");

public:
    typedef CurveType curve_type;
    typedef curve_adapter<CurveType> adapter;
    typedef typename adapter::scalar_value_type field_value_type;
    typedef typename adapter::g1_value_type g1_value_type;
    typedef typename adapter::g2_value_type g2_value_type;
    typedef typename adapter::gt_value_type gt_value_type;

    /// the two vectors of a key, resident (commitment_key<group_type>, kzg_ipp2.hpp:72-178)
    template <int Group>
    struct commitment_key {
        device_bases<CurveType, Group> a, b;

        commitment_key() = default;
        /// from host values, as the reference's key holds them
        template <typename InputIt>
        commitment_key(const context &ctx, InputIt a_first, InputIt a_last, InputIt b_first, InputIt b_last) : a(ctx, a_first, a_last), b(ctx, b_first, b_last) { }
        /// a_i = s_a^i G, b_i = s_b^i G for i < n, the multiples computed on the device (structured_generators_scalar_power, srs.hpp:44-56)
        static commitment_key from_scalar_powers(const context &ctx, std::size_t n, const field_value_type &s_a, const field_value_type &s_b) {
            commitment_key k;
            k.a = powers(ctx, n, s_a);
            k.b = powers(ctx, n, s_b);
            return k;
        }
        bool has_correct_len(std::size_t n) const { return a.size() == n && n == b.size(); }

    private:
        static device_bases<CurveType, Group> powers(const context &ctx, std::size_t n, const field_value_type &s) {
            std::vector<field_value_type> e;
            e.reserve(n);
            field_value_type acc = field_value_type::one();
            for (std::size_t i = 0; i < n; ++i, acc = acc * s) e.push_back(acc);
            return device_bases<CurveType, Group>::from_scalars(ctx, e.begin(), e.end());
        }
    };
    typedef commitment_key<ZKHIP_G2> vkey_type;
    typedef commitment_key<ZKHIP_G1> wkey_type;
    typedef std::pair<gt_value_type, gt_value_type> output_type;

    /// T = prod e(A_i, v1_i) e(w1_i, B_i), U = prod e(A_i, v2_i) e(w2_i, B_i) over resident vectors (kzg_ipp2.hpp:216-255)
    static output_type pair(const vkey_type &vkey, const wkey_type &wkey, const device_bases<CurveType, ZKHIP_G1> &a, const device_bases<CurveType, ZKHIP_G2> &b) {
        if (!vkey.has_correct_len(a.size())) throw std::invalid_argument("kzg_ipp2_hip::pair: vkey and the G1 vector differ in length");
        if (!wkey.has_correct_len(b.size())) throw std::invalid_argument("kzg_ipp2_hip::pair: wkey and the G2 vector differ in length");
        if (a.size() != b.size()) throw std::invalid_argument("kzg_ipp2_hip::pair: the two vectors differ in length");
        const std::size_t n = a.size();
        const auto out = detail::pairing_products<CurveType>(context_of(a), {detail::pairing_term<CurveType>(a, vkey.a, n, 0), detail::pairing_term<CurveType>(wkey.a, b, n, 0),
                                                                            detail::pairing_term<CurveType>(a, vkey.b, n, 1), detail::pairing_term<CurveType>(wkey.b, b, n, 1)},
                                                             2);
        return std::make_pair(out[0], out[1]);
    }
    /// the same over host values: both vectors are uploaded to the keys' context for the call
    template <typename InputG1Iterator, typename InputG2Iterator>
    static output_type pair(const vkey_type &vkey, const wkey_type &wkey, InputG1Iterator a_first, InputG1Iterator a_last, InputG2Iterator b_first,
                            InputG2Iterator b_last) {
        if (!vkey.has_correct_len((std::size_t)std::distance(a_first, a_last))) throw std::invalid_argument("kzg_ipp2_hip::pair: vkey and the G1 vector differ in length");
        if (!wkey.has_correct_len((std::size_t)std::distance(b_first, b_last))) throw std::invalid_argument("kzg_ipp2_hip::pair: wkey and the G2 vector differ in length");
        const context &ctx = context_of(vkey.a);
        const device_bases<CurveType, ZKHIP_G1> a(ctx, a_first, a_last);
        const device_bases<CurveType, ZKHIP_G2> b(ctx, b_first, b_last);
        return pair(vkey, wkey, a, b);
    }

    /// T = prod e(A_i, v1_i), U = prod e(A_i, v2_i) over a resident vector (kzg_ipp2.hpp:264-283)
    static output_type single(const vkey_type &vkey, const device_bases<CurveType, ZKHIP_G1> &a) {
        if (!vkey.has_correct_len(a.size())) throw std::invalid_argument("kzg_ipp2_hip::single: vkey and the G1 vector differ in length");
        const auto out = detail::pairing_products<CurveType>(
            context_of(a), {detail::pairing_term<CurveType>(a, vkey.a, a.size(), 0), detail::pairing_term<CurveType>(a, vkey.b, a.size(), 1)}, 2);
        return std::make_pair(out[0], out[1]);
    }
    template <typename InputG1Iterator>
    static output_type single(const vkey_type &vkey, InputG1Iterator a_first, InputG1Iterator a_last) {
        if (!vkey.has_correct_len((std::size_t)std::distance(a_first, a_last))) throw std::invalid_argument("kzg_ipp2_hip::single: vkey and the G1 vector differ in length");
        const device_bases<CurveType, ZKHIP_G1> a(context_of(vkey.a), a_first, a_last);
        return single(vkey, a);
    }

private:
    template <int Group>
    static const context &context_of(const device_bases<CurveType, Group> &b) {
        if (!b.owner_context()) throw std::invalid_argument("kzg_ipp2_hip: a key or vector that holds no resident points");
        return *b.owner_context();
    }
};

}    // namespace hip
}    // namespace zk
}    // namespace crypto3
}    // namespace nil

#endif    // ZKHIP_SHIM_KZG_IPP2_HPP
