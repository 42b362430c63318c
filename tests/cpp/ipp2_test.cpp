// C++ shim test harness (test-only) of the inner pairing product commitments over the stand-in `bls12_381` types: kzg_ipp2_hip::single and
// ::pair with keys built from scalar powers on the device and the committed vectors given as host values or as resident bases,
// pairing_inner_product_hip over resident vectors, and the length checks (has_correct_len mismatches throw).
// Built into libipp2test.so by tests/cpp/Makefile; driven by tests/test_gpu_ipp2_shim.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include <nil/crypto3/zk/hip/kzg_ipp2.hpp>

#include "harness_common.hpp"

using namespace nil::crypto3::zk::hip;
using harness::throws_invalid;

namespace {

typedef bls12_381 curve;
typedef kzg_ipp2_hip<curve> scheme;
typedef curve_adapter<curve> A;

void put(std::uint64_t *out, const scheme::output_type &c) {
    std::memcpy(out, c.first.limbs.data(), 72 * 8);
    std::memcpy(out + 72, c.second.limbs.data(), 72 * 8);
}

}    // namespace

extern "C" {

// out (2 x 72 limbs) = single(vkey, a) with vkey = (u^i G2, v^i G2), i < n; resident != 0: a is uploaded by the caller and passed as bases
int ipp2_single(const std::uint64_t *u, const std::uint64_t *v, std::size_t n, const std::uint64_t *a_xy, int resident, std::uint64_t *out) {
    return harness::guarded(__func__, [&] {
        context ctx(0);
        const auto vkey = scheme::vkey_type::from_scalar_powers(ctx, n, A::scalar_from_limbs(u), A::scalar_from_limbs(v));
        const auto a = harness::read_points<A::g1_value_type>(a_xy, nullptr, n);
        if (resident) {
            const device_bases<curve, ZKHIP_G1> da(ctx, a.begin(), a.end());
            put(out, scheme::single(vkey, da));
        } else {
            put(out, scheme::single(vkey, a.begin(), a.end()));
        }
        return 0;
    });
}

// out = pair(vkey, wkey, a, b), wkey = (u^i G1, v^i G1); the wkey is built from HOST values here (the other constructor of a key)
int ipp2_pair(const std::uint64_t *u, const std::uint64_t *v, std::size_t n, const std::uint64_t *a_xy, const std::uint64_t *b_xy, int resident, std::uint64_t *out) {
    return harness::guarded(__func__, [&] {
        context ctx(0);
        const auto us = A::scalar_from_limbs(u), vs = A::scalar_from_limbs(v);
        const auto vkey = scheme::vkey_type::from_scalar_powers(ctx, n, us, vs);
        const auto dev_w = scheme::wkey_type::from_scalar_powers(ctx, n, us, vs);
        const auto w1 = dev_w.a.download(), w2 = dev_w.b.download();
        const scheme::wkey_type wkey(ctx, w1.begin(), w1.end(), w2.begin(), w2.end());
        const auto a = harness::read_points<A::g1_value_type>(a_xy, nullptr, n);
        const auto b = harness::read_points<A::g2_value_type>(b_xy, nullptr, n);
        if (resident) {
            const device_bases<curve, ZKHIP_G1> da(ctx, a.begin(), a.end());
            const device_bases<curve, ZKHIP_G2> db(ctx, b.begin(), b.end());
            put(out, scheme::pair(vkey, wkey, da, db));
        } else {
            put(out, scheme::pair(vkey, wkey, a.begin(), a.end(), b.begin(), b.end()));
        }
        return 0;
    });
}

// out (72 limbs) = pairing_inner_product_hip over a_i G1 and b_i G2, i < n; returns 1 when the value is gt_value::one(), 0 when it is not
int ipp2_inner_product(const std::uint64_t *sa, const std::uint64_t *sb, std::size_t n, std::uint64_t *out) {
    return harness::guarded(__func__, [&] {
        context ctx(0);
        std::vector<A::scalar_value_type> ea, eb;
        for (std::size_t i = 0; i < n; ++i) ea.push_back(A::scalar_from_limbs(sa + 4 * i)), eb.push_back(A::scalar_from_limbs(sb + 4 * i));
        const auto a = device_bases<curve, ZKHIP_G1>::from_scalars(ctx, ea.begin(), ea.end());
        const auto b = device_bases<curve, ZKHIP_G2>::from_scalars(ctx, eb.begin(), eb.end());
        const A::gt_value_type z = pairing_inner_product_hip<curve>(ctx, a, b);
        std::memcpy(out, z.limbs.data(), 72 * 8);
        const bool is_one = z == A::gt_value_type::one();
        if (is_one == (z != A::gt_value_type::one())) return -1;    // == and != disagree
        return is_one ? 1 : 0;
    });
}

// the length checks: keys of n = 4; which = 0 single over 3 points, 1 pair with 3 G2 points, 2 pair with 3 G1 points, 3 a vkey whose halves
// differ (4 and 3), 4 inner product over 4 and 3, 5 single over resident 5 points, 6 every length right (must NOT throw)
int ipp2_length_mismatch(int which) {
    return harness::guarded(__func__, [&]() -> int {
        context ctx(0);
        const std::size_t n = 4;
        const A::scalar_value_type s(3), t(5);
        const auto vkey = scheme::vkey_type::from_scalar_powers(ctx, n, s, t);
        const auto wkey = scheme::wkey_type::from_scalar_powers(ctx, n, s, t);
        const auto a = wkey.a.download();
        const auto b = vkey.a.download();
        switch (which) {
        case 0: return throws_invalid([&] { scheme::single(vkey, a.begin(), a.begin() + 3); });
        case 1: return throws_invalid([&] { scheme::pair(vkey, wkey, a.begin(), a.end(), b.begin(), b.begin() + 3); });
        case 2: return throws_invalid([&] { scheme::pair(vkey, wkey, a.begin(), a.begin() + 3, b.begin(), b.end()); });
        case 3: {
            const scheme::vkey_type bad(ctx, b.begin(), b.end(), b.begin(), b.begin() + 3);
            if (bad.has_correct_len(4) || bad.has_correct_len(3) || !vkey.has_correct_len(4)) return -1;
            return throws_invalid([&] { scheme::single(bad, a.begin(), a.end()); });
        }
        case 4: {
            const device_bases<curve, ZKHIP_G2> short_b(ctx, b.begin(), b.begin() + 3);
            return throws_invalid([&] { pairing_inner_product_hip<curve>(ctx, wkey.a, short_b); });
        }
        case 5: {
            std::vector<A::g1_value_type> five(a);
            five.push_back(a[0]);
            const device_bases<curve, ZKHIP_G1> da(ctx, five.begin(), five.end());
            return throws_invalid([&] { scheme::single(vkey, da); });
        }
        case 6: return throws_invalid([&] { scheme::pair(vkey, wkey, a.begin(), a.end(), b.begin(), b.end()); });
        default: return -1;
        }
    });
}

}    // extern "C"
