//---------------------------------------------------------------------------//
// zkhip shim: the typed layer between the schemes' scalar-field values and the Fr-vector entry points of the C ABI
// (include/zkhip.h: zkhip_fr_vec_*, zkhip_poly_*, zkhip_ntt_dev, zkhip_fri_fold_dev, the 32-byte-element device copy).
// Every member converts its scalar arguments to canonical limbs, calls ONE entry point and checks it under that entry
// point's own name.  No state, no allocation, no synchronisation: buffers, their lifetimes and every sync() stay with the
// caller.  Counts and lengths are in ELEMENTS (32 bytes each), never in bytes.
//---------------------------------------------------------------------------//
#ifndef ZKHIP_SHIM_FR_VECTOR_HPP
#define ZKHIP_SHIM_FR_VECTOR_HPP

#include <array>
#include <cstdint>
#include <vector>

#include "backend.hpp"

namespace nil {
namespace crypto3 {
namespace zk {
namespace hip {

/// the pointwise operation of zkhip_fr_vec_op_dev (zkhip.h: "op 0 add, 1 sub, 2 mul")
enum class fr_op : int { add = 0, sub = 1, mul = 2 };

/// a scalar as the ABI reads it, for the few places that keep one packed (zkhip_domain, root maps, query tables)
template <typename Adapter>
std::array<std::uint64_t, 4> limbs_of(const typename Adapter::scalar_value_type &v) {
    std::array<std::uint64_t, 4> l;
    Adapter::scalar_to_limbs(v, l.data());
    return l;
}

template <typename CurveType>
struct fr_vector {
    typedef curve_adapter<CurveType> adapter;
    typedef typename adapter::scalar_value_type value_type;

    /// out[i] = a[i] op b[i], i < n; in place allowed
    static void pointwise(const context &ctx, fr_op op, const void *a, const void *b, void *out, std::size_t n) {
        ZKHIP_CALL(ctx, zkhip_fr_vec_op_dev, adapter::id, (int)op, a, b, out, n);
    }
    /// out[i] = a x[i] + b y[i] + c, i < n; y may be null (then b is not passed either): a x[i] + c
    static void affine(const context &ctx, const void *x, const void *y, const value_type &a, const value_type &b, const value_type &c, void *out, std::size_t n) {
        ZKHIP_CALL(ctx, zkhip_fr_vec_affine_dev, adapter::id, x, y, limbs(a).data(), y ? limbs(b).data() : nullptr, limbs(c).data(), out, n);
    }
    /// out[i] = c x[i], i < n
    static void scale(const context &ctx, const void *x, const value_type &c, void *out, std::size_t n) {
        affine(ctx, x, nullptr, c, value_type::zero(), value_type::zero(), out, n);
    }
    /// out[i] = a[i] b[i] / c[i], i < n (entries from n on are not touched)
    static void mul_div(const context &ctx, const void *a, const void *b, const void *c, void *out, std::size_t n) {
        ZKHIP_CALL(ctx, zkhip_fr_vec_mul_div_dev, adapter::id, a, b, c, out, n);
    }
    /// out[i] = prod_k ptrs[k][i], i < n; out may be one of the factors
    static void product(const context &ctx, const std::vector<const void *> &ptrs, void *out, std::size_t n) {
        ZKHIP_CALL(ctx, zkhip_fr_vec_prod_dev, adapter::id, ptrs.size(), ptrs.data(), out, n);
    }
    /// acc[j] (+)= sum_i sum_{t < taps} coeffs[i * taps + t] ptrs[i][j - t], j < acc_len; ptrs[i] holds lens[i] elements.  The coefficients
    /// as canonical limbs already packed (4 per coefficient) ...
    static void lincomb(const context &ctx, const std::vector<const void *> &ptrs, const std::vector<std::size_t> &lens, const std::vector<std::uint64_t> &coeffs,
                        std::size_t taps, void *acc, std::size_t acc_len, bool accumulate) {
        ZKHIP_CALL(ctx, zkhip_poly_lincomb_dev, adapter::id, ptrs.size(), ptrs.data(), lens.data(), coeffs.data(), taps, acc, acc_len, accumulate ? 1 : 0);
    }
    /// ... or as scalar values
    static void lincomb(const context &ctx, const std::vector<const void *> &ptrs, const std::vector<std::size_t> &lens, const std::vector<value_type> &coeffs,
                        std::size_t taps, void *acc, std::size_t acc_len, bool accumulate) {
        std::vector<std::uint64_t> packed(4 * coeffs.size());
        for (std::size_t i = 0; i < coeffs.size(); ++i) adapter::scalar_to_limbs(coeffs[i], &packed[4 * i]);
        lincomb(ctx, ptrs, lens, packed, taps, acc, acc_len, accumulate);
    }
    /// acc[j] (+)= c src[j] for j < len, (+)= 0 for len <= j < acc_len
    static void add_scaled(const context &ctx, const void *src, std::size_t len, const value_type &c, void *acc, std::size_t acc_len, bool accumulate) {
        ZKHIP_CALL(ctx, zkhip_poly_lincomb_dev, adapter::id, 1, &src, &len, limbs(c).data(), 1, acc, acc_len, accumulate ? 1 : 0);
    }
    /// dst[j] = src[j] for j < len, zero for len <= j < dst_len; an empty source (len == 0) is not read and may be null
    static void zero_padded_copy(const context &ctx, const void *src, std::size_t len, void *dst, std::size_t dst_len) {
        if (!len) src = nullptr;
        ZKHIP_CALL(ctx, zkhip_poly_lincomb_dev, adapter::id, len ? 1 : 0, &src, &len, limbs(value_type::one()).data(), 1, dst, dst_len, 0);
    }
    /// in-place transform of `batch` vectors of 2^log_n elements over the domain `root` generates
    static void ntt(const context &ctx, void *data, std::size_t log_n, std::size_t batch, const value_type &root, bool inverse) {
        ZKHIP_CALL(ctx, zkhip_ntt_dev, adapter::id, data, log_n, batch, limbs(root).data(), inverse ? 1 : 0, nullptr);
    }
    /// `batch` vectors of 2^log_n evaluations at `in` (CONSUMED when the domain grows) -> 2^log_out evaluations each at `out`
    static void resize(const context &ctx, void *in, std::size_t log_n, std::size_t batch, const value_type &root_n, void *out, std::size_t log_out,
                       const value_type &root_out) {
        ZKHIP_CALL(ctx, zkhip_poly_resize_dev, adapter::id, in, log_n, batch, limbs(root_n).data(), out, log_out, limbs(root_out).data());
    }
    /// out[i] = in[i 2^(log_n - log_out)], i < 2^log_out < 2^log_n: the shrinking form of the call above, which reads neither root and
    /// leaves `in` untouched.  Equal sizes are no subsampling (the entry point would take them for a resize and check the roots): the
    /// dfs-level subsample (fri.hpp) answers them with the polynomial itself.
    static void subsample(const context &ctx, const void *in, std::size_t log_n, void *out, std::size_t log_out) {
        const std::uint64_t unused[4] = {1, 0, 0, 0};
        ZKHIP_CALL(ctx, zkhip_poly_resize_dev, adapter::id, const_cast<void *>(in), log_n, 1, unused, out, log_out, unused);
    }
    /// out[i] = in[(i + rotation) mod 2^log_size]; out must not alias in
    static void shift(const context &ctx, const void *in, std::size_t log_size, std::int64_t rotation, void *out) {
        ZKHIP_CALL(ctx, zkhip_poly_shift_dev, in, log_size, rotation, out);
    }
    /// FRI's fold of the 2^log_size evaluations at f over the domain omega generates -> 2^(log_size - 1) elements at out
    static void fold(const context &ctx, const void *f, std::size_t log_size, const value_type &alpha, const value_type &omega, void *out) {
        ZKHIP_CALL(ctx, zkhip_fri_fold_dev, adapter::id, f, log_size, limbs(alpha).data(), limbs(omega).data(), out);
    }
    /// out[0] = f(z), out[1 .. n) = the n - 1 coefficients of f / (X - z); out may equal f.  Returns f(z), which synchronises the stream.
    static value_type div_linear(const context &ctx, const void *f, std::size_t n, const value_type &z, void *out) {
        std::uint64_t remainder[4];
        ZKHIP_CALL(ctx, zkhip_poly_div_linear_dev, adapter::id, f, n, limbs(z).data(), out, remainder);
        return adapter::scalar_from_limbs(remainder);
    }
    /// `elements` elements from src to dst, in stream order
    static void copy(const context &ctx, void *dst, const void *src, std::size_t elements) { ZKHIP_CALL(ctx, zkhip_memcpy_d2d_async, dst, src, elements * 32); }

private:
    static std::array<std::uint64_t, 4> limbs(const value_type &v) { return limbs_of<adapter>(v); }
};

}    // namespace hip
}    // namespace zk
}    // namespace crypto3
}    // namespace nil

#endif    // ZKHIP_SHIM_FR_VECTOR_HPP
