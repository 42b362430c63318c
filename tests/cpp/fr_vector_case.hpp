// Test-only: every member of fr_vector (hip/fr_vector.hpp) the dfs arithmetic does not already pin, one call per case, over buffers the test
// fills and reads back -- what tests/test_gpu_shim.py (BLS12-381 / BN254) and tests/test_gpu_pasta_shim.py (Pallas) hold against Python
// integers.  All sizes are in elements of four limbs.
//   a: n elements, b: what the case needs besides (see below), s: up to three scalars, out: the case's result
#ifndef ZKHIP_TEST_FR_VECTOR_CASE_HPP
#define ZKHIP_TEST_FR_VECTOR_CASE_HPP

#include <algorithm>
#include <cstdint>
#include <memory>

#include <nil/crypto3/zk/hip/fri.hpp>

namespace fr_vector_case {

enum what_type {
    pointwise_add = 0,       // b: n           out[n] = a + b      (1: a - b, 2: a * b)
    pointwise_sub = 1,
    pointwise_mul = 2,
    affine = 3,              // b: n           out[n] = s0 a + s1 b + s2; flag == 0: without y, s0 a + s2
    scale = 4,               //                out[n] = s0 a
    zero_padded_copy = 5,    // b: m           out[m] = a below n, zero behind, over a destination pre-filled with b; n == 0: a null source
    add_scaled = 6,          // b: m           out[m] = (flag ? b : 0) + s0 a (a zero behind n)
    subsample = 7,           // a: 2^n         out[2^m] = every 2^(n - m)-th element; through the dfs form, which answers m == n itself
    div_linear = 8,          //                out[n + 1] = f(s0), the n - 1 quotient coefficients of a / (X - s0), then the RETURNED remainder
    copy = 9                 // b: n + 1       out[n + 1] = a, then b[n]: a destination of n + 1 elements pre-filled with b
};

template <typename Curve>
int run(const nil::crypto3::zk::hip::context &ctx, int what, const std::uint64_t *a, const std::uint64_t *b, std::size_t n, const std::uint64_t *s, std::size_t m,
        int flag, std::uint64_t *out) {
    using namespace nil::crypto3::zk::hip;
    typedef fr_vector<Curve> fv;
    typedef curve_adapter<Curve> A;
    typedef typename A::scalar_value_type Fr;
    auto up = [&ctx](const std::uint64_t *h, std::size_t count) {
        std::shared_ptr<void> d = ctx.alloc(std::max<std::size_t>(1, count) * 32);
        if (count) ctx.h2d(d.get(), h, count * 32);
        return d;
    };
    auto scalar = [s](std::size_t k) { return A::scalar_from_limbs(s + 4 * k); };
    switch (what) {
    case pointwise_add:
    case pointwise_sub:
    case pointwise_mul: {
        auto d_a = up(a, n), d_b = up(b, n), d_out = ctx.alloc(n * 32);
        fv::pointwise(ctx, what == pointwise_add ? fr_op::add : what == pointwise_sub ? fr_op::sub : fr_op::mul, d_a.get(), d_b.get(), d_out.get(), n);
        ctx.d2h(out, d_out.get(), n * 32);
        return 0;
    }
    case affine: {
        auto d_a = up(a, n), d_b = up(b, n), d_out = ctx.alloc(n * 32);
        fv::affine(ctx, d_a.get(), flag ? d_b.get() : nullptr, scalar(0), scalar(1), scalar(2), d_out.get(), n);
        ctx.d2h(out, d_out.get(), n * 32);
        return 0;
    }
    case scale: {
        auto d_a = up(a, n), d_out = ctx.alloc(n * 32);
        fv::scale(ctx, d_a.get(), scalar(0), d_out.get(), n);
        ctx.d2h(out, d_out.get(), n * 32);
        return 0;
    }
    case zero_padded_copy: {
        auto d_a = up(a, n), d_out = up(b, m);
        fv::zero_padded_copy(ctx, n ? d_a.get() : nullptr, n, d_out.get(), m);
        ctx.d2h(out, d_out.get(), m * 32);
        return 0;
    }
    case add_scaled: {
        auto d_a = up(a, n), d_out = up(b, m);
        fv::add_scaled(ctx, d_a.get(), n, scalar(0), d_out.get(), m, flag != 0);
        ctx.d2h(out, d_out.get(), m * 32);
        return 0;
    }
    case subsample: {
        device_polynomial_dfs<Curve> p(ctx, (std::size_t)1 << n);
        ctx.h2d(p.data(), a, p.size() * 32);
        const device_polynomial_dfs<Curve> q = nil::crypto3::zk::hip::subsample(p, (std::size_t)1 << m);    // fv::subsample when m < n, p itself when m == n
        ctx.d2h(out, q.data(), q.size() * 32);
        return 0;
    }
    case div_linear: {
        auto d_a = up(a, n), d_out = ctx.alloc(n * 32);
        const Fr remainder = fv::div_linear(ctx, d_a.get(), n, scalar(0), d_out.get());
        ctx.d2h(out, d_out.get(), n * 32);
        A::scalar_to_limbs(remainder, out + 4 * n);
        return 0;
    }
    case copy: {
        auto d_a = up(a, n), d_out = up(b, n + 1);
        fv::copy(ctx, d_out.get(), d_a.get(), n);
        ctx.d2h(out, d_out.get(), (n + 1) * 32);
        return 0;
    }
    }
    return -2;
}

}    // namespace fr_vector_case

#endif    // ZKHIP_TEST_FR_VECTOR_CASE_HPP
