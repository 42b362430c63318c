//---------------------------------------------------------------------------//
// zkhip shim: the Groth16 verifier on the device (replaces, for BLS12-381,
// zk/snark/systems/ppzksnark/r1cs_gg_ppzksnark/verification_key.hpp and verifier.hpp:56-226).
//
// The reference checks one proof on one host thread: an accumulation over the public inputs, a Miller loop, a double
// Miller loop and a final exponentiation (verifier.hpp:150-186).  Here a processed key is RESIDENT (zkhip_groth16_vk: the
// prepared lines of gamma and delta and fixed-base tables of gamma_ABC_g1, include/zkhip.h "Groth16 verification") and
// proofs are checked by the batch, a proof per lane, with zkhip_groth16_verify_batch.  The names are the reference's with
// the suffix _hip; the batch form process(pvk, inputs, proofs) has no counterpart there.
//
// Weak input consistency: a primary input shorter than the key's is padded with zeros (verifier.hpp:150-155); a longer
// one, which the reference only asserts against, throws std::invalid_argument.  Strong input consistency answers false
// on a size mismatch without a launch (verifier.hpp:216-226).
//---------------------------------------------------------------------------//
#ifndef ZKHIP_SHIM_R1CS_GG_PPZKSNARK_VERIFIER_HPP
#define ZKHIP_SHIM_R1CS_GG_PPZKSNARK_VERIFIER_HPP

#include <stdexcept>
#include <utility>
#include <vector>

#include "r1cs_gg_ppzksnark.hpp"

namespace nil {
namespace crypto3 {
namespace zk {
namespace hip {

/// accumulation_vector<g1_type> as the verification key holds it (container/accumulation_vector.hpp): first, then rest
template <typename CurveType>
struct g1_accumulation_vector {
    typename curve_adapter<CurveType>::g1_value_type first;
    std::vector<typename curve_adapter<CurveType>::g1_value_type> rest;
    std::size_t size() const { return rest.size(); }
};

/// r1cs_gg_ppzksnark_verification_key (verification_key.hpp:46-90)
template <typename CurveType>
struct r1cs_gg_ppzksnark_verification_key {
    ZKHIP_REQUIRE_PAIRING(CurveType, "Groth16");
    typedef curve_adapter<CurveType> adapter;
    typename adapter::gt_value_type alpha_g1_beta_g2;
    typename adapter::g2_value_type gamma_g2, delta_g2;
    g1_accumulation_vector<CurveType> gamma_ABC_g1;
    std::size_t num_inputs() const { return gamma_ABC_g1.size(); }
};

/// The processed key: a resident zkhip_groth16_vk on `ctx` (one owner, move-only)
template <typename CurveType>
class r1cs_gg_ppzksnark_processed_verification_key_hip {
public:
    r1cs_gg_ppzksnark_processed_verification_key_hip() = default;
    r1cs_gg_ppzksnark_processed_verification_key_hip(const context &ctx, const r1cs_gg_ppzksnark_verification_key<CurveType> &vk) : ctx_(&ctx) {
        typedef curve_adapter<CurveType> adapter;
        std::uint64_t g2[2][4 * adapter::g1_coord_limbs];
        if (!adapter::point_to_affine_limbs(vk.gamma_g2, g2[0]) || !adapter::point_to_affine_limbs(vk.delta_g2, g2[1]))
            throw std::invalid_argument("r1cs_gg_ppzksnark_process_verification_key_hip: gamma_g2 or delta_g2 is the point at infinity");
        const std::size_t n_abc = vk.gamma_ABC_g1.rest.size() + 1, cl = 2 * adapter::g1_coord_limbs;
        std::vector<std::uint64_t> xy(n_abc * cl);
        std::vector<std::uint8_t> inf(n_abc);
        for (std::size_t i = 0; i < n_abc; ++i)
            inf[i] = adapter::point_to_affine_limbs(i ? vk.gamma_ABC_g1.rest[i - 1] : vk.gamma_ABC_g1.first, xy.data() + i * cl) ? 0 : 1;
        ZKHIP_CALL(ctx, zkhip_groth16_vk_upload, adapter::id, vk.alpha_g1_beta_g2.limbs.data(), g2[0], g2[1], xy.data(), inf.data(), n_abc, &vk_);
    }
    ~r1cs_gg_ppzksnark_processed_verification_key_hip() { reset(); }
    r1cs_gg_ppzksnark_processed_verification_key_hip(r1cs_gg_ppzksnark_processed_verification_key_hip &&o) noexcept : ctx_(o.ctx_), vk_(o.vk_) { o.vk_ = nullptr; }
    r1cs_gg_ppzksnark_processed_verification_key_hip &operator=(r1cs_gg_ppzksnark_processed_verification_key_hip &&o) noexcept {
        if (this != &o) {
            reset();
            ctx_ = o.ctx_, vk_ = o.vk_;
            o.vk_ = nullptr;
        }
        return *this;
    }
    r1cs_gg_ppzksnark_processed_verification_key_hip(const r1cs_gg_ppzksnark_processed_verification_key_hip &) = delete;
    r1cs_gg_ppzksnark_processed_verification_key_hip &operator=(const r1cs_gg_ppzksnark_processed_verification_key_hip &) = delete;

    const zkhip_groth16_vk *get() const { return vk_; }
    const context &owner_context() const {
        if (!ctx_ || !vk_) throw std::invalid_argument("r1cs_gg_ppzksnark_processed_verification_key_hip: an empty key");
        return *ctx_;
    }
    std::size_t num_inputs() const { return zkhip_groth16_vk_inputs(vk_); }

private:
    void reset() {
        if (vk_) zkhip_groth16_vk_free(ctx_ ? ctx_->get() : nullptr, vk_);
        vk_ = nullptr;
    }
    const context *ctx_ = nullptr;
    zkhip_groth16_vk *vk_ = nullptr;
};

/// r1cs_gg_ppzksnark_process_verification_key::process (verifier.hpp:56-72)
template <typename CurveType>
struct r1cs_gg_ppzksnark_process_verification_key_hip {
    typedef r1cs_gg_ppzksnark_verification_key<CurveType> verification_key_type;
    typedef r1cs_gg_ppzksnark_processed_verification_key_hip<CurveType> processed_verification_key_type;
    static processed_verification_key_type process(const context &ctx, const verification_key_type &vk) { return processed_verification_key_type(ctx, vk); }
};

/// r1cs_gg_ppzksnark_verifier_weak_input_consistency (verifier.hpp:120-186)
template <typename CurveType>
class r1cs_gg_ppzksnark_verifier_weak_input_consistency_hip {
    typedef curve_adapter<CurveType> adapter;

public:
    typedef r1cs_gg_ppzksnark_verification_key<CurveType> verification_key_type;
    typedef r1cs_gg_ppzksnark_processed_verification_key_hip<CurveType> processed_verification_key_type;
    typedef std::vector<typename adapter::scalar_value_type> primary_input_type;
    typedef r1cs_gg_ppzksnark_proof<CurveType> proof_type;

    /// the batch form: verdict i is process(pvk, primary_inputs[i], proofs[i]); one zkhip_groth16_verify_batch call
    static std::vector<bool> process(const processed_verification_key_type &pvk, const std::vector<primary_input_type> &primary_inputs,
                                     const std::vector<proof_type> &proofs) {
        if (primary_inputs.size() != proofs.size()) throw std::invalid_argument("r1cs_gg_ppzksnark_verifier_hip: one primary input per proof");
        const context &ctx = pvk.owner_context();
        const std::size_t n = proofs.size();
        std::size_t width = 0;
        for (const auto &p : primary_inputs) width = std::max(width, p.size());
        if (width > pvk.num_inputs()) throw std::invalid_argument("r1cs_gg_ppzksnark_verifier_hip: more primary inputs than the key has");
        if (n == 0) return {};
        std::vector<std::uint64_t> inputs(n * width * 4, 0);    // shorter statements are padded with zeros, which is what weak consistency means
        for (std::size_t i = 0; i < n; ++i)
            for (std::size_t j = 0; j < primary_inputs[i].size(); ++j) adapter::scalar_to_limbs(primary_inputs[i][j], &inputs[(i * width + j) * 4]);
        std::vector<typename adapter::g1_value_type> a, c;
        std::vector<typename adapter::g2_value_type> b;
        for (const auto &p : proofs) a.push_back(p.g_A), b.push_back(p.g_B), c.push_back(p.g_C);
        const device_bases<CurveType, ZKHIP_G1> da(ctx, a.begin(), a.end()), dc(ctx, c.begin(), c.end());
        const device_bases<CurveType, ZKHIP_G2> db(ctx, b.begin(), b.end());
        std::vector<std::uint8_t> ok(n);
        ZKHIP_CALL(ctx, zkhip_groth16_verify_batch, pvk.get(), da.get(), db.get(), dc.get(), 0, n, width ? inputs.data() : nullptr, width, ok.data(), nullptr);
        return std::vector<bool>(ok.begin(), ok.end());
    }
    static bool process(const processed_verification_key_type &pvk, const primary_input_type &primary_input, const proof_type &proof) {
        return process(pvk, std::vector<primary_input_type> {primary_input}, std::vector<proof_type> {proof})[0];
    }
    static bool process(const context &ctx, const verification_key_type &vk, const primary_input_type &primary_input, const proof_type &proof) {
        return process(processed_verification_key_type(ctx, vk), primary_input, proof);
    }
    /// the reference's argument list: the calling thread's default context
    static bool process(const verification_key_type &vk, const primary_input_type &primary_input, const proof_type &proof) {
        return process(default_context(), vk, primary_input, proof);
    }
};

/// r1cs_gg_ppzksnark_verifier_strong_input_consistency (verifier.hpp:190-226)
template <typename CurveType>
class r1cs_gg_ppzksnark_verifier_strong_input_consistency_hip {
    typedef r1cs_gg_ppzksnark_verifier_weak_input_consistency_hip<CurveType> weak;

public:
    typedef typename weak::verification_key_type verification_key_type;
    typedef typename weak::processed_verification_key_type processed_verification_key_type;
    typedef typename weak::primary_input_type primary_input_type;
    typedef typename weak::proof_type proof_type;

    /// the batch form: a statement of another size than the key's is false, the others go to the device in one call
    static std::vector<bool> process(const processed_verification_key_type &pvk, const std::vector<primary_input_type> &primary_inputs,
                                     const std::vector<proof_type> &proofs) {
        if (primary_inputs.size() != proofs.size()) throw std::invalid_argument("r1cs_gg_ppzksnark_verifier_hip: one primary input per proof");
        std::vector<primary_input_type> in;
        std::vector<proof_type> pf;
        std::vector<std::size_t> at;
        for (std::size_t i = 0; i < proofs.size(); ++i)
            if (primary_inputs[i].size() == pvk.num_inputs()) in.push_back(primary_inputs[i]), pf.push_back(proofs[i]), at.push_back(i);
        std::vector<bool> out(proofs.size(), false);
        const std::vector<bool> ok = weak::process(pvk, in, pf);
        for (std::size_t k = 0; k < at.size(); ++k) out[at[k]] = ok[k];
        return out;
    }
    static bool process(const processed_verification_key_type &pvk, const primary_input_type &primary_input, const proof_type &proof) {
        return primary_input.size() == pvk.num_inputs() && weak::process(pvk, primary_input, proof);
    }
    static bool process(const context &ctx, const verification_key_type &vk, const primary_input_type &primary_input, const proof_type &proof) {
        return primary_input.size() == vk.num_inputs() && weak::process(ctx, vk, primary_input, proof);
    }
    static bool process(const verification_key_type &vk, const primary_input_type &primary_input, const proof_type &proof) {
        return process(default_context(), vk, primary_input, proof);
    }
};

}    // namespace hip
}    // namespace zk
}    // namespace crypto3
}    // namespace nil

#endif    // ZKHIP_SHIM_R1CS_GG_PPZKSNARK_VERIFIER_HPP
