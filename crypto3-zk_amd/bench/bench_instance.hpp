// The synthetic Groth16 instance the bench entry points share (groth16_bench.cpp, groth16_verify_bench.cpp).
#pragma once
#include <cstdint>
#include <vector>

#include <nil/crypto3/zk/hip/r1cs_gg_ppzksnark_generator.hpp>

namespace zkhip_bench {

using namespace nil::crypto3::zk::hip;

struct SplitMix {
    uint64_t s;
    uint64_t next() {
        s += 0x9E3779B97F4A7C15ULL;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    }
};

/// the reference's generate_r1cs_example_with_field_input family (r1cs_examples.hpp:77-140), M constraints, n public inputs,
/// N = M + 2 variables; returns the generator state for (r, s).  zero_start: the two free values are zero instead of random, and with
/// them every value of the chain (a satisfying assignment whose public inputs are all zero)
template <typename Curve>
SplitMix build_instance(size_t M, size_t n, uint64_t seed, r1cs_constraint_system<Curve> &cs, std::vector<typename curve_adapter<Curve>::scalar_value_type> &full,
                        bool zero_start = false) {
    typedef curve_adapter<Curve> A;
    typedef typename A::scalar_value_type Fr;
    SplitMix rng {seed};
    auto rnd = [&]() {    // < 2^252 < r for both curves: canonical
        uint64_t w[4] = {rng.next(), rng.next(), rng.next(), rng.next() & 0x0fffffffffffffffULL};
        return A::scalar_from_limbs(w);
    };
    cs.primary_input_size = n;
    cs.auxiliary_input_size = 2 + M - n;
    Fr a = rnd(), b = rnd();
    if (zero_start) a = b = Fr::zero();
    full.push_back(a);
    full.push_back(b);
    cs.constraints.reserve(M);
    for (size_t i = 0; i + 1 < M; ++i) {
        r1cs_constraint<Curve> c;
        Fr tmp;
        if (i % 2) {
            c.a.add_term(i + 1, 1);
            c.b.add_term(i + 2, 1);
            tmp = a * b;
        } else {
            c.b.add_term(0, 1);
            c.a.add_term(i + 1, 1);
            c.a.add_term(i + 2, 1);
            tmp = a + b;
        }
        c.c.add_term(i + 3, 1);
        full.push_back(tmp);
        a = b;
        b = tmp;
        cs.add_constraint(c);
    }
    {
        r1cs_constraint<Curve> c;
        Fr fin = Fr::zero();
        for (size_t i = 1; i < cs.num_variables(); ++i) {
            c.a.add_term(i, 1);
            c.b.add_term(i, 1);
            fin = fin + full[i - 1];
        }
        c.c.add_term(cs.num_variables(), 1);
        cs.add_constraint(c);
        full.push_back(fin * fin);
    }
    return rng;
}

}    // namespace zkhip_bench
