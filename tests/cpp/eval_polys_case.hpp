// Test-only: ONE set of polynomials and evaluation points through whichever commitment scheme of the shim is handed in -- the case of the
// polys_evaluator's eval_polys that tests/test_gpu_shim.py (KZG v2 and LPC over BLS12-381 / BN254) and tests/test_gpu_pasta_shim.py (LPC
// over Pallas) hold against the oracle's Horner.
//   batch 0: four polynomials of 2^3, 2^3, 2^5, 2^3 evaluations (a run of two equal lengths, broken by another length, resumed), opened
//            at {a, b}, {b}, {a, b, c}, {c, a}: the union differs from every single set, the order from the union's;
//   batch 2: one polynomial of 2^4 evaluations opened at a (batch ids with a gap, a point shared across batches).
#ifndef ZKHIP_TEST_EVAL_POLYS_CASE_HPP
#define ZKHIP_TEST_EVAL_POLYS_CASE_HPP

#include <cstdint>
#include <vector>

#include <nil/crypto3/zk/hip/fri.hpp>

namespace eval_polys_case {

constexpr std::size_t log_len[5] = {3, 3, 5, 3, 4};
constexpr std::size_t evaluations = 2 + 1 + 3 + 2 + 1;

/// evals: the five polynomials' evaluations, one behind the other; points: a | b | c.  out_z: proof.z in (batch, polynomial, point) order,
/// `evaluations` elements.  0, or a negative code when proof.z does not have the case's shape
template <typename Scheme>
int run(Scheme &scheme, typename Scheme::transcript_type &transcript, const std::uint64_t *evals, const std::uint64_t *points, std::uint64_t *out_z) {
    typedef typename Scheme::adapter A;
    typedef typename A::scalar_value_type Fr;
    typedef nil::crypto3::zk::hip::polynomial_dfs<typename Scheme::curve_type> poly;
    std::vector<poly> polys(5);
    for (std::size_t p = 0, at = 0; p < 5; ++p)
        for (std::size_t i = 0; i < ((std::size_t)1 << log_len[p]); ++i) polys[p].values.push_back(A::scalar_from_limbs(evals + 4 * at++));
    const Fr a = A::scalar_from_limbs(points), b = A::scalar_from_limbs(points + 4), c = A::scalar_from_limbs(points + 8);
    scheme.append_to_batch(0, std::vector<poly>(polys.begin(), polys.begin() + 4));
    scheme.append_to_batch(2, polys[4]);
    (void)scheme.commit(0);
    (void)scheme.commit(2);
    const std::vector<std::vector<Fr>> sets = {{a, b}, {b}, {a, b, c}, {c, a}};
    for (std::size_t i = 0; i < sets.size(); ++i) scheme.append_eval_points(0, i, sets[i]);
    scheme.append_eval_point(2, a);
    const auto proof = scheme.proof_eval(transcript);
    if (proof.z.get_batches() != std::vector<std::size_t> {0, 2}) return -30;
    if (proof.z.get_batch_size(0) != 4 || proof.z.get_batch_size(2) != 1) return -31;
    std::size_t zi = 0;
    for (std::size_t k : proof.z.get_batches())
        for (std::size_t i = 0; i < proof.z.get_batch_size(k); ++i) {
            if (proof.z.get_poly_points_number(k, i) != (k == 0 ? sets[i].size() : 1)) return -32;
            for (std::size_t q = 0; q < proof.z.get_poly_points_number(k, i); ++q) A::scalar_to_limbs(proof.z.get(k, i, q), out_z + 4 * zi++);
        }
    return zi == evaluations ? 0 : -33;
}

}    // namespace eval_polys_case

#endif    // ZKHIP_TEST_EVAL_POLYS_CASE_HPP
