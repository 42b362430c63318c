// Groth16 verification through the header-only shim (r1cs_gg_ppzksnark_verifier.hpp), for tests/test_gpu_groth16_verify_shim.py and
// tools: generate a key WITH its verification key, prove on the device, verify on the device; and the batch verification of given
// points.  Host compiler only; links libzkhip.so.
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

#include <nil/crypto3/zk/hip/r1cs_gg_ppzksnark_generator.hpp>
#include <nil/crypto3/zk/hip/r1cs_gg_ppzksnark_verifier.hpp>

#include "bench_instance.hpp"

using namespace nil::crypto3::zk::hip;
using zkhip_bench::SplitMix;

extern "C" {

// BLS12-381.  The synthetic instance of zkhip_bench_groth16 (M constraints, n >= 2 public inputs; zero_inputs: the satisfying assignment whose
// public inputs are all zero), a key and its verification key from a trapdoor fixed by the seed, two proofs of the same statement under different
// blinders, and the shim's verdicts:
//   out[0]  weak, process(ctx, vk, primary, proof)                      out[1]  weak, process(pvk, primary with the last input + 1, proof)
//   out[2]  strong, process(pvk, primary, proof)                        out[3]  strong, process(pvk, primary without its last input, proof)
//   out[4]  weak, process(pvk, primary without its last input, proof): accepted exactly when that input is zero
//   out[5..7]  weak, the batch form over (proof, proof with g_C replaced by g_A, second proof)
//   out[8..10] strong, the batch form over the same proofs with the LAST statement one input short
//   out[11] 1 when a primary input longer than the key's threw std::invalid_argument
// Returns 0, or -1 with nothing written when an exception escaped.
int zkhip_bench_groth16_verify_roundtrip(int device, size_t M, size_t n, uint64_t seed, int zero_inputs, const uint64_t *omega, const uint64_t *coset, int *out) {
    typedef native_curve<ZKHIP_BLS12_381> Curve;
    typedef curve_adapter<Curve> A;
    typedef A::scalar_value_type Fr;
    try {
        r1cs_constraint_system<Curve> cs;
        std::vector<Fr> full;
        SplitMix rng = zkhip_bench::build_instance<Curve>(M, n, seed, cs, full, zero_inputs != 0);
        auto rnd = [&]() {
            uint64_t w[4] = {rng.next(), rng.next(), rng.next(), rng.next() & 0x0fffffffffffffffULL};
            return A::scalar_from_limbs(w);
        };
        const std::vector<Fr> primary(full.begin(), full.begin() + n), auxiliary(full.begin() + n, full.end());
        context ctx(device);
        const domain_params<Curve> dom {A::scalar_from_limbs(omega), A::scalar_from_limbs(coset)};
        const Fr t = rnd(), alpha = rnd(), beta = rnd(), gamma = rnd(), delta = rnd();
        r1cs_gg_ppzksnark_verification_key<Curve> vk;
        auto key = r1cs_gg_ppzksnark_generator_hip<Curve>::deterministic_basic_process(ctx, cs, dom, t, alpha, beta, gamma, delta, 0, 1, &vk);
        typedef r1cs_gg_ppzksnark_prover_hip<Curve> prover;
        const Fr r1 = rnd(), s1 = rnd(), r2 = rnd(), s2 = rnd();
        const prover::proof_type proof = prover::process(*key->device, primary, auxiliary, r1, s1), second = prover::process(*key->device, primary, auxiliary, r2, s2);
        prover::proof_type spoiled = proof;
        spoiled.g_C = proof.g_A;

        typedef r1cs_gg_ppzksnark_verifier_weak_input_consistency_hip<Curve> weak;
        typedef r1cs_gg_ppzksnark_verifier_strong_input_consistency_hip<Curve> strong;
        const auto pvk = r1cs_gg_ppzksnark_process_verification_key_hip<Curve>::process(ctx, vk);
        std::vector<Fr> wrong = primary, shorter(primary.begin(), primary.end() - 1), longer = primary;
        wrong.back() = wrong.back() + Fr::one();
        longer.push_back(Fr::one());
        int res[12];
        res[0] = weak::process(ctx, vk, primary, proof);
        res[1] = weak::process(pvk, wrong, proof);
        res[2] = strong::process(pvk, primary, proof);
        res[3] = strong::process(pvk, shorter, proof);
        res[4] = weak::process(pvk, shorter, proof);
        const std::vector<bool> wb = weak::process(pvk, {primary, primary, primary}, {proof, spoiled, second});
        const std::vector<bool> sb = strong::process(pvk, {primary, primary, shorter}, {proof, spoiled, second});
        for (int k = 0; k < 3; ++k) res[5 + k] = wb[k], res[8 + k] = sb[k];
        res[11] = 0;
        try {
            (void)weak::process(pvk, longer, proof);
        } catch (const std::invalid_argument &) {
            res[11] = 1;
        }
        std::memcpy(out, res, sizeof(res));
        return 0;
    } catch (const std::exception &) {
        return -1;
    }
}

// The batch form over GIVEN values (canonical limbs as zkhip_groth16_vk_upload and zkhip_bases_upload take them; no point at infinity):
// ok[i] = weak (strong_consistency = 0) or strong verdict of proof i under inputs row i (n x n_inputs x 4 u64).  Returns 0, or -1 on an exception.
int zkhip_bench_groth16_verify_points(int device, const uint64_t *alpha_beta, const uint64_t *gamma_g2, const uint64_t *delta_g2, const uint64_t *abc_xy, size_t n_abc,
                                      const uint64_t *a_xy, const uint64_t *b_xy, const uint64_t *c_xy, size_t n, const uint64_t *inputs, size_t n_inputs,
                                      int strong_consistency, uint8_t *ok) {
    typedef native_curve<ZKHIP_BLS12_381> Curve;
    typedef curve_adapter<Curve> A;
    try {
        if (n_abc == 0) return -1;
        context ctx(device);
        r1cs_gg_ppzksnark_verification_key<Curve> vk;
        vk.alpha_g1_beta_g2 = A::gt_from_limbs(alpha_beta);
        vk.gamma_g2 = A::g2_value_type::from_affine(gamma_g2);
        vk.delta_g2 = A::g2_value_type::from_affine(delta_g2);
        vk.gamma_ABC_g1.first = A::g1_value_type::from_affine(abc_xy);
        for (size_t i = 1; i < n_abc; ++i) vk.gamma_ABC_g1.rest.push_back(A::g1_value_type::from_affine(abc_xy + 12 * i));
        const auto pvk = r1cs_gg_ppzksnark_process_verification_key_hip<Curve>::process(ctx, vk);
        std::vector<r1cs_gg_ppzksnark_proof<Curve>> proofs(n);
        std::vector<std::vector<A::scalar_value_type>> statements(n);
        for (size_t i = 0; i < n; ++i) {
            proofs[i].g_A = A::g1_value_type::from_affine(a_xy + 12 * i);
            proofs[i].g_B = A::g2_value_type::from_affine(b_xy + 24 * i);
            proofs[i].g_C = A::g1_value_type::from_affine(c_xy + 12 * i);
            for (size_t j = 0; j < n_inputs; ++j) statements[i].push_back(A::scalar_from_limbs(inputs + (i * n_inputs + j) * 4));
        }
        const std::vector<bool> res = strong_consistency ? r1cs_gg_ppzksnark_verifier_strong_input_consistency_hip<Curve>::process(pvk, statements, proofs)
                                                         : r1cs_gg_ppzksnark_verifier_weak_input_consistency_hip<Curve>::process(pvk, statements, proofs);
        for (size_t i = 0; i < n; ++i) ok[i] = res[i];
        return 0;
    } catch (const std::exception &) {
        return -1;
    }
}

}    // extern "C"
