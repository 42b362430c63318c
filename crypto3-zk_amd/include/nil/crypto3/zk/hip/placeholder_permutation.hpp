//---------------------------------------------------------------------------//
// zkhip shim: placeholder's permutation argument, prover side, on the device --
//   placeholder_permutation_argument::prove_eval   zk/snark/systems/plonk/placeholder/permutation_argument.hpp:70-224
// both forms: permutation_parts == 1 (common_data.max_quotient_chunks == 0) and the multi-part one the reference's tests also run
// (test/systems/plonk/placeholder/placeholder.cpp:1245, 1287-1291: max_quotient_poly_chunks = 8, 10, 30, 50).
//   :103-124  g_v[i] = column_i + beta S_id[i] + gamma,  h_v[i] = column_i + beta S_sigma[i] + gamma
//   :126-136  V_P[0] = 1, V_P[j] = V_P[j - 1] prod_i g_v[i][j - 1] / prod_i h_v[i][j - 1]    -- zkhip_perm_grand_product_dev: a serial loop with
//             one inversion per row in the reference; chunks sharing an inversion + a three-level prefix-product scan here
//   :140-160  g = polynomial_product(g_v), h = polynomial_product(h_v)
//   :163-218  F_dfs[0] = lagrange_0 (1 - V_P),  F_dfs[1] = (1 - (q_last + q_blind)) (V_P(omega X) h - V_P g),  F_dfs[2] = q_last V_P (V_P - 1)
//   :147-160, 188-207  max_quotient_chunks = c != 0: the factors in groups of c - 1; every group but the last gives an intermediate polynomial
//             current[j] = previous[j] g_i[j] / h_i[j] over the usable rows (zkhip_fr_vec_mul_div_dev: chunks sharing an inversion; one inversion per
//             row in the reference), appended to PERMUTATION_BATCH after V_P, and
//             F_dfs[1] = ((q_last + q_blind) - 1)(sum_i alpha_i (previous_i g_i - current_i h_i) + previous_last g_last - V_P(omega X) h_last)
// What the caller keeps: the transcript (beta, gamma are arguments) and `commitment_scheme.append_to_batch(PERMUTATION_BATCH, V_P)` --
// the returned V_P is a device_polynomial_dfs, which the KZG scheme takes where it lies.
// Domain sizes of the three F polynomials follow their degrees (the smallest power of two that holds them), as polynomial_dfs's
// operator*= does; quotient_polynomial (placeholder_quotient.hpp) brings all parts to one domain anyway.
//---------------------------------------------------------------------------//
#ifndef ZKHIP_SHIM_PLACEHOLDER_PERMUTATION_HPP
#define ZKHIP_SHIM_PLACEHOLDER_PERMUTATION_HPP

#include <array>
#include <functional>
#include <stdexcept>
#include <vector>

#include "fri.hpp"

namespace nil {
namespace crypto3 {
namespace zk {
namespace hip {

/// The loop both multi-part arguments run over all parts but the last (ph/permutation_argument.hpp:188-207, lookup_argument.hpp:252-276): part p
/// gives the intermediate polynomial current_p = previous g_p / h_p over the usable rows (multiplied_up; `fill`'s values behind them), handed
/// to `on_part` where the reference appends it to its batch, and the term alpha_p (previous g_p - current_p h_p) of the sum.  `previous_ext`:
/// `previous` on the domain every current is extended to ONCE -- for current h_p and, as the next previous, for previous g_(p + 1).
template <typename CurveType>
struct multi_part_sum {
    typedef device_polynomial_dfs<CurveType> dfs_type;
    std::vector<dfs_type> parts;    // one per alpha, in batch order
    dfs_type sum;                   // sum_p alpha_p (previous_p g_p - current_p h_p); a one-element placeholder without alphas
    dfs_type last_ext;              // the last current (without alphas: previous) on previous_ext's domain, for the caller's last part

    static multi_part_sum run(dfs_type previous, dfs_type previous_ext, const dfs_type &fill, const std::vector<dfs_type> &gs, const std::vector<dfs_type> &hs,
                              const std::vector<typename dfs_type::value_type> &alphas, std::size_t n, std::size_t usable_rows,
                              const std::function<void(const dfs_type &)> &on_part, const typename dfs_type::root_of_unity_type &root) {
        std::vector<dfs_type> parts;
        dfs_type sum(previous.ctx(), 1);
        const std::size_t ext_size = previous_ext.size();
        for (std::size_t p = 0; p < alphas.size(); ++p) {
            dfs_type current = multiplied_up(previous, fill, gs[p], hs[p], n, usable_rows);
            parts.push_back(current);
            if (on_part) on_part(current);
            const dfs_type current_ext = current.extension(ext_size, root);
            dfs_type part = minus(polynomial_product<CurveType>({previous_ext, gs[p]}, root), polynomial_product<CurveType>({current_ext, hs[p]}, root), root);
            scale(part, alphas[p]);
            sum = p == 0 ? part : plus(sum, part, root);
            previous = current;
            previous_ext = current_ext;
        }
        return {std::move(parts), std::move(sum), std::move(previous_ext)};
    }
};

template <typename CurveType>
struct placeholder_permutation_hip {
    typedef curve_adapter<CurveType> adapter;
    typedef typename adapter::scalar_value_type value_type;
    typedef device_polynomial_dfs<CurveType> dfs_type;
    typedef typename dfs_type::root_of_unity_type root_of_unity_type;
    typedef fr_vector<CurveType> fv;

    struct prover_result_type {
        std::array<dfs_type, 3> F_dfs;
        dfs_type permutation_polynomial_dfs;    // V_P
        std::vector<dfs_type> parts_dfs;        // the intermediate polynomials of the multi-part form, in PERMUTATION_BATCH order behind V_P
    };

    /// what the reference does BETWEEN the numeric steps (placeholder_arguments.hpp drives them from the transcript and the commitment scheme):
    /// on_V_P: V_P is final (:139 append_to_batch); draw_alphas(permutation_parts): the parts' challenges (:181-183); on_part: an intermediate
    /// polynomial is final (:200 append_to_batch).  Any of them may be empty.
    struct hooks_type {
        std::function<void(const dfs_type &)> on_V_P, on_part;
        std::function<std::vector<value_type>(std::size_t parts)> draw_alphas;
    };

    /// `columns[i]`: the i-th permuted column (column_polynomials[global_indices[i]], :93-97), S_id / S_sigma the preprocessed identity /
    /// permutation polynomials, all over the n-row basic domain.  max_quotient_chunks / alphas / usable_rows: the multi-part form
    /// (alphas: permutation_parts - 1 challenges in drawing order, :181-183).
    static prover_result_type prove_eval(const context &ctx, const std::vector<dfs_type> &columns, const std::vector<dfs_type> &S_id,
                                         const std::vector<dfs_type> &S_sigma, const dfs_type &q_last, const dfs_type &q_blind, const dfs_type &lagrange_0,
                                         const value_type &beta, const value_type &gamma, const root_of_unity_type &root, std::size_t max_quotient_chunks = 0,
                                         const std::vector<value_type> &alphas = {}, std::size_t usable_rows = 0) {
        hooks_type hooks;
        hooks.draw_alphas = [&alphas](std::size_t parts) {
            if (alphas.size() + 1 != parts) throw std::invalid_argument("permutation argument: permutation_parts - 1 alphas");
            return alphas;
        };
        return prove_eval_hooked(ctx, columns, S_id, S_sigma, q_last, q_blind, lagrange_0, beta, gamma, root, max_quotient_chunks, usable_rows, hooks);
    }

    /// the same with the challenges of the parts and the batch appends handed to the caller's hooks, each at the point of the reference's flow
    static prover_result_type prove_eval_hooked(const context &ctx, const std::vector<dfs_type> &columns, const std::vector<dfs_type> &S_id,
                                                const std::vector<dfs_type> &S_sigma, const dfs_type &q_last, const dfs_type &q_blind, const dfs_type &lagrange_0,
                                                const value_type &beta, const value_type &gamma, const root_of_unity_type &root, std::size_t max_quotient_chunks,
                                                std::size_t usable_rows, const hooks_type &hooks) {
        const std::size_t k = columns.size();
        if (k == 0 || S_id.size() != k || S_sigma.size() != k) throw std::invalid_argument("permutation argument: one S_id / S_sigma per permuted column");
        const std::size_t n = columns[0].size();
        for (std::size_t i = 0; i < k; ++i)
            if (columns[i].size() != n || S_id[i].size() != n || S_sigma[i].size() != n) throw std::invalid_argument("permutation argument: sizes differ from the basic domain's");
        if (q_last.size() != n || q_blind.size() != n || lagrange_0.size() != n) throw std::invalid_argument("permutation argument: selector sizes differ from the basic domain's");
        if (max_quotient_chunks == 1) throw std::invalid_argument("permutation argument: max_quotient_chunks = 1 leaves no factor per part");
        const std::size_t step = max_quotient_chunks ? max_quotient_chunks - 1 : k, parts = (k + step - 1) / step;    // preprocessor.hpp:80-87
        if (parts > 1 && (usable_rows == 0 || usable_rows >= n)) throw std::invalid_argument("permutation argument: the multi-part form needs usable_rows");
        /* Round 5: with extension caches on S_id / S_sigma (preprocessed, the same in every proof) the factors g_v, h_v are formed ON the products'
           domain from ONE extension per column -- ext(column) + beta ext(S) + gamma, a pointwise pass -- instead of being extended one by one (2 k
           transforms); a column's extension is shared with whatever else extended it (the gate argument) when the column's cache is on as well. */
        bool factors_from_columns = true;
        for (std::size_t i = 0; i < k; ++i) factors_from_columns = factors_from_columns && S_id[i].extension_cache_enabled() && S_sigma[i].extension_cache_enabled();
        /* 2.-3.: g_v, h_v and V_P in one device call */
        std::shared_ptr<void> d_g, d_h;
        if (!factors_from_columns) {
            d_g = ctx.alloc(k * n * 32);
            d_h = ctx.alloc(k * n * 32);
        }
        dfs_type V_P(ctx, n);
        std::vector<const void *> pc, pi, ps;
        for (std::size_t i = 0; i < k; ++i) {
            pc.push_back(columns[i].data());
            pi.push_back(S_id[i].data());
            ps.push_back(S_sigma[i].data());
        }
        const auto bl = limbs_of<adapter>(beta), gl = limbs_of<adapter>(gamma);
        ZKHIP_CALL(ctx, zkhip_perm_grand_product_dev, adapter::id, k, pc.data(), pi.data(), ps.data(), n, bl.data(), gl.data(), d_g.get(), d_h.get(), V_P.data());
        V_P.set_degree(n - 1);
        if (hooks.on_V_P) hooks.on_V_P(V_P);    // 4. (:139)
        /* 5.: gs[p] = prod of the p-th group's g_v, hs[p] likewise */
        std::vector<dfs_type> gs, hs;
        for (std::size_t lo = 0; lo < k; lo += step) {
            std::vector<dfs_type> g_v, h_v;
            const std::size_t hi = std::min(k, lo + step), size = pow2_holding((hi - lo) * (n - 1));
            if (factors_from_columns) {
                /* the group's g and h on their domain in ONE pass over the extended columns and (cached) permutation polynomials */
                std::vector<dfs_type> ext;    // alive until the pass ran
                std::vector<const void *> ec, ei, es;
                for (std::size_t i = lo; i < hi; ++i) {
                    ext.push_back(columns[i].extension(size, root));
                    ec.push_back(ext.back().data());
                    ext.push_back(S_id[i].extension(size, root));
                    ei.push_back(ext.back().data());
                    ext.push_back(S_sigma[i].extension(size, root));
                    es.push_back(ext.back().data());
                }
                dfs_type g(ctx, size), h(ctx, size);
                g.set_degree((hi - lo) * (n - 1));
                h.set_degree((hi - lo) * (n - 1));
                ZKHIP_CALL(ctx, zkhip_perm_factor_products_dev, adapter::id, hi - lo, ec.data(), ei.data(), es.data(), size, bl.data(), gl.data(), g.data(), h.data());
                gs.push_back(std::move(g));
                hs.push_back(std::move(h));
                continue;
            }
            for (std::size_t i = lo; i < hi; ++i) {
                g_v.emplace_back(ctx, n);
                h_v.emplace_back(ctx, n);
                fv::copy(ctx, g_v.back().data(), static_cast<const char *>(d_g.get()) + i * n * 32, n);
                fv::copy(ctx, h_v.back().data(), static_cast<const char *>(d_h.get()) + i * n * 32, n);
            }
            gs.push_back(polynomial_product<CurveType>(std::move(g_v), root));
            hs.push_back(polynomial_product<CurveType>(std::move(h_v), root));
        }
        /* V_P takes part in five products on three domains: it is extended ONCE, to the largest of them (that of V_P g), and subsampled for the
           others inside polynomial_product; V_P(omega X) is a rotation of that extension; likewise lagrange_0 and q_last */
        std::size_t deg_g = 0;
        for (const auto &g : gs) deg_g = std::max(deg_g, g.degree());
        const dfs_type V = V_P.extension(pow2_holding(V_P.degree() + deg_g), root);
        const dfs_type V_shifted = polynomial_shift(V, 1, n);
        const dfs_type L0 = lagrange_0.extension(2 * n, root), QL = q_last.extension(4 * n, root);
        prover_result_type res {{dfs_type(ctx, 1), dfs_type(ctx, 1), dfs_type(ctx, 1)}, V_P, {}};
        /* F_dfs[0] = lagrange_0 (1 - V_P) = lagrange_0 - lagrange_0 V_P */
        res.F_dfs[0] = minus(L0, polynomial_product<CurveType>({L0, V}, root, L0.size()), root);
        const std::vector<value_type> alphas = hooks.draw_alphas ? hooks.draw_alphas(parts) : std::vector<value_type>();    // :181-183
        if (alphas.size() + 1 != parts) throw std::invalid_argument("permutation argument: permutation_parts - 1 alphas");
        const dfs_type q = selector_sum(q_last, q_blind, pow2_holding(n - 1 + V_P.degree() + deg_g), root);    // q_last + q_blind
        if (parts == 1) {
            /* F_dfs[1] = (1 - q)(V_P_shifted h - V_P g) = T - q T,  q = q_last + q_blind */
            dfs_type T = minus(polynomial_product<CurveType>({V_shifted, hs[0]}, root), polynomial_product<CurveType>({V, gs[0]}, root), root);
            res.F_dfs[1] = minus(T, polynomial_product<CurveType>({q, T}, root), root);
        } else {
            /* F_dfs[1] = (q - 1)(sum_i alpha_i (previous g_i - current h_i) + previous g_last - V_P_shifted h_last) = q S - S */
            multi_part_sum<CurveType> m = multi_part_sum<CurveType>::run(V_P, V, V_P, gs, hs, alphas, n, usable_rows, hooks.on_part, root);    // on_part: :200
            res.parts_dfs = m.parts;
            dfs_type last = minus(polynomial_product<CurveType>({m.last_ext, gs[parts - 1]}, root), polynomial_product<CurveType>({V_shifted, hs[parts - 1]}, root), root);
            dfs_type S = std::move(m.sum);
            S = plus(S, last, root);
            res.F_dfs[1] = minus(polynomial_product<CurveType>({q, S}, root), S, root);
        }
        /* F_dfs[2] = q_last V_P (V_P - 1) = q_last V_P V_P - q_last V_P, both products on the first one's domain */
        res.F_dfs[2] = minus(polynomial_product<CurveType>({QL, V, V}, root), polynomial_product<CurveType>({QL, V}, root, QL.size()), root);
        ctx.sync();
        return res;
    }

    /// p *= c, in place (fri.hpp: scale)
    static void scale(dfs_type &p, const value_type &c) { nil::crypto3::zk::hip::scale<CurveType>(p, c); }
};

}    // namespace hip
}    // namespace zk
}    // namespace crypto3
}    // namespace nil

#endif    // ZKHIP_SHIM_PLACEHOLDER_PERMUTATION_HPP
