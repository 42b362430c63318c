//---------------------------------------------------------------------------//
// zkhip shim: the Pedersen / inner-product-argument polynomial commitment of the pairing-less curves, on the MI355X.
//
// Mirrors commitments::kimchi_pedersen<CurveType> (zk/commitments/polynomial/kimchi_pedersen.hpp), statement for statement:
//   commitment(params, poly, bound)                                          (:334-383)  one MSM per chunk over sub-ranges of the resident g
//   proof_eval(params, group_map, plms, elm, polyscale, evalscale, sponge)   (:385-559)  a, b, g stay on the device for the whole opening
//   verify_eval(params, group_map, batches)                                  (:645-755)  one MSM over the resident [g ..., h] + one small one
//   params.add_lagrange_basis(domain)                                        (:92-105)   the inverse DFT over group elements of g[0 .. n) on the
//                                                                                        device; the result stays resident and is downloaded once
//   commitment_evaluations(params, evals)                                    (no counterpart) one MSM of a column's evaluations over that basis
// What stays the CALLER's, as the transcript does for the KZG and LPC shims (duck-typed template parameters):
//   SpongeType    copyable;  absorb_fr(scalar), absorb_g(g1 value), challenge_fq() -> whatever GroupMapType::to_group takes,
//                 squeeze_challenge(endo_r) -> scalar (never zero: it is inverted), and shift_scalar(scalar) -> scalar -- kimchi_functions'
//                 (pickles/detail/kimchi_functions.hpp:13-21), which the reference reaches through its `functions` typedef; the shim
//                 calls it on the sponge object (a static member serves).  The reference's sponge is Poseidon over the Mina policy.
//   GroupMapType  to_group(t) -> g1 value
//   RandomSource  scalar operator()(): every algebra::random_element<scalar_field_type>() of the reference, in the reference's order --
//                 commitment: one per unshifted chunk, then one more whether or not a shifted part exists; proof_eval: rand_l, rand_r
//                 per round, then d, r_delta; verify_eval: rand_base, sg_rand_base.
// Neither Poseidon nor the group map run on the device, and there is one context (no device group).
//---------------------------------------------------------------------------//
#ifndef ZKHIP_SHIM_KIMCHI_PEDERSEN_HPP
#define ZKHIP_SHIM_KIMCHI_PEDERSEN_HPP

#include <memory>
#include <stdexcept>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "fr_vector.hpp"
#include "multiexp.hpp"

namespace nil {
namespace crypto3 {
namespace zk {
namespace hip {

template <typename CurveType, typename SpongeType, typename GroupMapType, typename RandomSource>
struct kimchi_pedersen_hip {
    typedef curve_adapter<CurveType> adapter;
    typedef typename adapter::scalar_value_type scalar_value_type;
    typedef typename adapter::g1_value_type group_value_type;
    typedef multiexp_method_hip multiexp_method;
    typedef SpongeType sponge_type;
    typedef GroupMapType group_map_type;
    static constexpr std::size_t jac_limbs = 3 * adapter::g1_coord_limbs;
    typedef fr_vector<CurveType> fv;

    /// params_type with the generators resident: ONE object [g_0 .. g_(n-1), infinity up to the next power of two, h] with window
    /// tables -- commitment reads sub-ranges of g, the opening's first round the padded g, verify_eval all of it.
    struct params_type {
        template <typename InputIt>
        params_type(const context &ctx, RandomSource &random, InputIt g_first, InputIt g_last, const group_value_type &h, const scalar_value_type &endo_r) :
            ctx(ctx), random(random), g(g_first, g_last), h(h), endo_r(endo_r) {
            for (padded = 1; padded < g.size(); padded <<= 1) { }
            std::vector<group_value_type> all(g);
            all.resize(padded, group_value_type::zero());
            all.push_back(h);
            srs = device_bases<CurveType, ZKHIP_G1>(ctx, all.begin(), all.end());
        }
        const context &ctx;
        RandomSource &random;
        std::vector<group_value_type> g;
        group_value_type h;
        scalar_value_type endo_r;
        std::size_t padded = 1;                       ///< |g| rounded up to a power of two
        device_bases<CurveType, ZKHIP_G1> srs;        ///< h is its row `padded`: the one-point range (padded, 1) is the resident h
        /// the reference's member (:71): the Lagrange-basis SRS per domain size, a host copy downloaded once (pickles/verifier.hpp:78-79 reads it)
        std::unordered_map<std::size_t, std::vector<group_value_type>> lagrange_bases;
        /// the same bases resident, with window tables: what commitment_evaluations multiplies against
        std::unordered_map<std::size_t, device_bases<CurveType, ZKHIP_G1>> lagrange_resident;

        /// :92-105: lagrange_bases[n] = inverse_fft over group elements of g[0 .. n), on the device (zkhip_bases_lagrange).  Domain: size() and
        /// omega -- evaluation_domain_hip of the basic kind, or the reference's basic_radix2_domain.  A size that is already there returns at
        /// once (no launch); throws where the reference asserts (n > |g|), and for a size that is not a power of two.
        template <typename Domain>
        void add_lagrange_basis(const Domain &domain) {
            const std::size_t n = domain.size();
            if (lagrange_bases.find(n) != lagrange_bases.end()) return;
            if (n == 0 || (n & (n - 1)) != 0) throw std::invalid_argument("kimchi_pedersen: add_lagrange_basis needs a radix-2 domain");
            if (n > g.size()) throw std::invalid_argument("kimchi_pedersen: add_lagrange_basis: the domain is larger than the SRS");
            std::size_t log_n = 0;
            while (((std::size_t)1 << log_n) < n) ++log_n;
            const auto at = lagrange_resident.emplace(n, srs.lagrange(0, log_n, domain.omega)).first;
            lagrange_bases[n] = at->second.download();
        }
    };

    template <typename value_type>
    struct poly_comm {
        std::vector<value_type> unshifted;
        value_type shifted {};
        poly_comm() = default;
        poly_comm(const std::vector<value_type> &unshifted, const value_type &shifted) : unshifted(unshifted), shifted(shifted) { }
    };
    typedef poly_comm<group_value_type> commitment_type;
    typedef poly_comm<scalar_value_type> blinding_type;
    typedef std::tuple<commitment_type, blinding_type> blinded_commitment_type;

    struct poly_type_single {
        std::vector<scalar_value_type> coeffs;
        std::size_t bound = -1;    ///< as in the reference: a size_t, so "no bound" is the largest value
        blinding_type commit;
        poly_type_single(const std::vector<scalar_value_type> &coeffs, int bound, const blinding_type &commit) : coeffs(coeffs), bound(bound), commit(commit) { }
    };
    typedef std::vector<poly_type_single> poly_type;

    struct proof_type {
        std::vector<std::tuple<group_value_type, group_value_type>> lr;
        group_value_type delta;
        scalar_value_type z1, z2;
        group_value_type sg;
        std::tuple<std::vector<scalar_value_type>, std::vector<scalar_value_type>> challenges(const scalar_value_type &endo_r, sponge_type &sponge) const {
            std::vector<scalar_value_type> chal, chal_invs;
            for (const auto &[l, r] : lr) {
                sponge.absorb_g(l);
                sponge.absorb_g(r);
                chal.push_back(sponge.squeeze_challenge(endo_r));
                chal_invs.push_back(chal.back().inversed());
            }
            return std::make_tuple(chal, chal_invs);
        }
    };

    struct evaluation_type {
        commitment_type commit;
        std::vector<std::vector<scalar_value_type>> evaluations;    ///< [evaluation point][chunk]
        int bound = -1;
        evaluation_type(const commitment_type &commit, const std::vector<std::vector<scalar_value_type>> &evaluations, int bound) :
            commit(commit), evaluations(evaluations), bound(bound) { }
    };

    struct batchproof_type {
        sponge_type sponge;
        std::vector<evaluation_type> evaluation;
        std::vector<scalar_value_type> evaluation_points;
        scalar_value_type xi, r;
        proof_type opening;
    };

    /// :334-383
    static blinded_commitment_type commitment(const params_type &params, const std::vector<scalar_value_type> &poly, int bound) {
        const context &ctx = params.ctx;
        commitment_type res;
        blinding_type blind_res;
        const std::size_t g_len = params.g.size();
        /* every multiexp of the non-hiding part as one batch over sub-ranges of the resident g: the chunks, then the shifted part */
        std::vector<std::size_t> offs, ns, at;
        for (std::size_t left = 0, len = poly.size(); len > 0;) {
            const std::size_t take = std::min(len, g_len);
            offs.push_back(0), ns.push_back(take), at.push_back(left);
            left += take, len -= take;
        }
        const std::size_t chunks = ns.size();
        bool has_shifted = false, nonzero = false;
        for (const auto &c : poly) nonzero = nonzero || !c.is_zero();
        if (bound >= 0) {
            const std::size_t start = (std::size_t)bound - (std::size_t)bound % g_len;
            const std::size_t tail = (std::size_t)bound % g_len;    // bases g.end() - bound % g_len .. g.end(): none when the bound ends a chunk
            if (nonzero && start < poly.size() && tail > 0) {
                has_shifted = true;
                offs.push_back(g_len - tail), ns.push_back(std::min(tail, poly.size() - start)), at.push_back(start);
            }
        }
        std::vector<group_value_type> sums;
        if (!ns.empty()) {
            auto d_poly = ctx.alloc(std::max<std::size_t>(1, poly.size()) * 32);
            upload_scalars<adapter>(ctx, d_poly.get(), poly.data(), poly.size());
            sums = msm_batch(ctx, std::vector<const zkhip_bases *>(ns.size(), params.srs.get()), offs, ns, d_poly.get(), at);
        }
        res.unshifted.assign(sums.begin(), sums.begin() + chunks);
        if (has_shifted) res.shifted = sums.back();
        /* masking part */
        for (auto &i : res.unshifted) {
            const scalar_value_type w = params.random();
            i = i + w * params.h;
            blind_res.unshifted.push_back(w);
        }
        const scalar_value_type w = params.random();
        if (!res.shifted.is_zero()) {
            res.shifted = res.shifted + w * params.h;
            blind_res.shifted = w;
        }
        return blinded_commitment_type(res, blind_res);
    }

    /// The NON-HIDING commitment of the polynomial whose evaluations over the domain of size evals.size() are given: one MSM over the
    /// resident Lagrange bases of that size into unshifted[0], no inverse NTT.  No blinding, no degree bound and no chunking (the domain is
    /// no larger than the SRS); the hiding variant is `commitment`'s masking loop, unshifted[0] + w h, and is the caller's one line.
    /// Throws if add_lagrange_basis was not called for that size.
    static commitment_type commitment_evaluations(const params_type &params, const std::vector<scalar_value_type> &evals) {
        const auto at = params.lagrange_resident.find(evals.size());
        if (at == params.lagrange_resident.end()) throw std::invalid_argument("kimchi_pedersen: commitment_evaluations: no Lagrange basis of this size was added");
        commitment_type res;
        res.unshifted.push_back(multiexp<CurveType, ZKHIP_G1>(params.ctx, at->second, 0, evals.begin(), evals.end()));
        return res;
    }

    /// :385-559
    static proof_type proof_eval(const params_type &params, group_map_type &group_map, const poly_type &plms, const std::vector<scalar_value_type> &elm,
                                 const scalar_value_type &polyscale, const scalar_value_type &evalscale, sponge_type &sponge) {
        const context &ctx = params.ctx;
        proof_type res;
        std::vector<std::tuple<scalar_value_type, scalar_value_type>> blinders;
        const std::size_t n = params.g.size();
        std::size_t power_of_two = params.padded;

        /* a = sum scale_k segment_k on the device: the unshifted segments land at 0, a shifted one at n - |segment| */
        auto d_a = ctx.alloc(power_of_two * 32), d_b = ctx.alloc(power_of_two * 32);
        std::vector<std::shared_ptr<void>> d_coeffs;
        std::vector<const void *> lo_ptr;
        std::vector<std::size_t> lo_len;
        std::vector<scalar_value_type> lo_scale;
        struct shifted_term {
            const void *ptr;
            std::size_t len;
            scalar_value_type scale;
        };
        std::vector<shifted_term> shifted;
        scalar_value_type blinding_factor = scalar_value_type::zero(), scale = scalar_value_type::one();
        for (const auto &polynom : plms) {
            d_coeffs.push_back(ctx.alloc(std::max<std::size_t>(1, polynom.coeffs.size()) * 32));
            upload_scalars<adapter>(ctx, d_coeffs.back().get(), polynom.coeffs.data(), polynom.coeffs.size());
            std::size_t offset = 0, j = 0;
            /* polynom.bound is unsigned: the reference's `bound >= 0` branch is the only one ever taken */
            while (j < polynom.commit.unshifted.size()) {
                const std::size_t end = std::min(offset + n, polynom.coeffs.size());
                const std::size_t seg = end > offset ? end - offset : 0;
                const void *seg_ptr = static_cast<const char *>(d_coeffs.back().get()) + 32 * offset;
                lo_ptr.push_back(seg_ptr), lo_len.push_back(seg);
                lo_scale.push_back(scale);
                blinding_factor = blinding_factor + polynom.commit.unshifted[j] * scale;
                j += 1;
                scale = scale * polyscale;
                offset += n;
                if (offset > polynom.bound) {
                    shifted.push_back({seg_ptr, seg, scale});
                    blinding_factor = blinding_factor + polynom.commit.shifted * scale;
                    scale = scale * polyscale;
                }
            }
        }
        fv::lincomb(ctx, lo_ptr, lo_len, lo_scale, 1, d_a.get(), power_of_two, false);
        for (const shifted_term &t : shifted)
            if (t.len) fv::add_scaled(ctx, t.ptr, t.len, t.scale, static_cast<char *>(d_a.get()) + 32 * (n - t.len), t.len, true);

        /* b[i] = sum_e evalscale^e elm[e]^i */
        std::vector<std::uint64_t> pts(4 * elm.size()), scl(4 * elm.size());
        scale = scalar_value_type::one();
        for (std::size_t e = 0; e < elm.size(); ++e) {
            adapter::scalar_to_limbs(elm[e], &pts[4 * e]);
            adapter::scalar_to_limbs(scale, &scl[4 * e]);
            scale = scale * evalscale;
        }
        ZKHIP_CALL(ctx, zkhip_fr_powers_lincomb_dev, adapter::id, pts.data(), scl.data(), elm.size(), d_b.get(), power_of_two);

        /* per-round scalars [rand_l, <a_hi, b_lo>, rand_r, <a_lo, b_hi>] and the four partial sums of L and R */
        auto d_sc = ctx.alloc(4 * 32), d_jac = ctx.alloc(6 * jac_limbs * 8);
        char *sc = static_cast<char *>(d_sc.get());
        std::uint64_t *jac = static_cast<std::uint64_t *>(d_jac.get());
        ZKHIP_CALL(ctx, zkhip_fr_inner_product_dev, adapter::id, d_a.get(), d_b.get(), power_of_two, sc);
        sponge.absorb_fr(sponge.shift_scalar(download_scalar(ctx, sc)));
        const group_value_type u = group_map.to_group(sponge.challenge_fq());
        /* [h, u] for the two-point sums rand h + <., .> u of every round, padded with infinity to the size from which an upload builds window
           tables: without them every one of those sums would pay the serial Horner pass over the windows (measured: 1.6 ms each, DESIGN) */
        std::vector<group_value_type> hu(32, group_value_type::zero());
        hu[0] = params.h, hu[1] = u;
        const device_bases<CurveType, ZKHIP_G1> hu_dev(ctx, hu.begin(), hu.end());

        std::vector<scalar_value_type> chals, chal_invs;
        bases_handle folded;                           // g of the current round; empty: the resident (padded) g itself
        const zkhip_bases *g_cur = params.srs.get();
        char *a = static_cast<char *>(d_a.get()), *b = static_cast<char *>(d_b.get());
        while (power_of_two > 1) {
            power_of_two >>= 1;
            const std::size_t half = power_of_two;
            const scalar_value_type rand_l = params.random();
            const scalar_value_type rand_r = params.random();
            upload_scalars<adapter>(ctx, sc, &rand_l, 1);
            upload_scalars<adapter>(ctx, sc + 64, &rand_r, 1);
            ZKHIP_CALL(ctx, zkhip_fr_inner_product_dev, adapter::id, a + 32 * half, b, half, sc + 32);
            ZKHIP_CALL(ctx, zkhip_fr_inner_product_dev, adapter::id, a, b + 32 * half, half, sc + 96);
            /* l = <g_low, a_high> + rand_l h + <a_high, b_low> u,   r = <g_high, a_low> + rand_r h + <a_low, b_high> u */
            const zkhip_bases *qb[4] = {g_cur, hu_dev.get(), g_cur, hu_dev.get()};
            const std::size_t qo[4] = {0, 0, half, 0}, qn[4] = {half, 2, half, 2};
            const void *qs[4] = {a + 32 * half, sc, a, sc + 64};
            void *qr[4] = {jac, jac + jac_limbs, jac + 2 * jac_limbs, jac + 3 * jac_limbs};
            ZKHIP_CALL(ctx, zkhip_msm_batch_dev, 4, qb, qo, qn, qs, qr);
            ZKHIP_CALL(ctx, zkhip_jacobian_sum_dev, adapter::id, ZKHIP_G1, jac, 2, jac + 4 * jac_limbs);
            ZKHIP_CALL(ctx, zkhip_jacobian_sum_dev, adapter::id, ZKHIP_G1, jac + 2 * jac_limbs, 2, jac + 5 * jac_limbs);
            std::uint64_t lr_host[2 * jac_limbs];
            ctx.d2h(lr_host, jac + 4 * jac_limbs, sizeof(lr_host));
            const group_value_type l = normalised(adapter::g1_from_jacobian(lr_host)), r = normalised(adapter::g1_from_jacobian(lr_host + jac_limbs));
            res.lr.emplace_back(l, r);
            blinders.emplace_back(rand_l, rand_r);

            sponge.absorb_g(l);
            sponge.absorb_g(r);
            const scalar_value_type u_scalar = sponge.squeeze_challenge(params.endo_r);
            const scalar_value_type u_scalar_inv = u_scalar.inversed();
            chals.push_back(u_scalar);
            chal_invs.push_back(u_scalar_inv);

            /* a = a_high u^-1 + a_low,  b = b_high u + b_low,  g = g_high u + g_low */
            fv::affine(ctx, a + 32 * half, a, u_scalar_inv, scalar_value_type::one(), scalar_value_type::zero(), a, half);
            fv::affine(ctx, b + 32 * half, b, u_scalar, scalar_value_type::one(), scalar_value_type::zero(), b, half);
            zkhip_bases *next = nullptr;
            ZKHIP_CALL(ctx, zkhip_bases_fold, g_cur, 0, half, half, limbs_of<adapter>(u_scalar).data(), &next);
            folded = bases_handle(next, bases_free {ctx.get()});
            g_cur = next;
        }
        const scalar_value_type a0 = download_scalar(ctx, a), b0 = download_scalar(ctx, b);
        group_value_type g0;
        {
            std::uint64_t xy[2 * adapter::g1_coord_limbs];
            std::uint8_t inf = 0;
            ZKHIP_CALL(ctx, zkhip_bases_download, g_cur, 0, 1, xy, &inf);
            g0 = group_value_type::from_affine(xy, inf != 0);
        }

        scalar_value_type r_prime = blinding_factor;
        for (std::size_t i = 0; i < blinders.size(); ++i) {
            const auto &[l, r] = blinders[i];
            r_prime = r_prime + (l * chal_invs[i] + r * chals[i]);
        }
        const scalar_value_type d = params.random();
        const scalar_value_type r_delta = params.random();

        const group_value_type delta = normalised((g0 + u * b0) * d + params.h * r_delta);
        sponge.absorb_g(delta);
        const scalar_value_type cc = sponge.squeeze_challenge(params.endo_r);

        res.delta = delta;
        res.z1 = a0 * cc + d;
        res.z2 = cc * r_prime + r_delta;
        res.sg = g0;
        return res;
    }

    /// :561-609
    static scalar_value_type combined_inner_product(const std::vector<scalar_value_type> &evaluation_points, const scalar_value_type &xi,
                                                    const scalar_value_type &r, const std::vector<std::tuple<evaluation_type, int>> &polys, std::size_t g_size) {
        scalar_value_type res = scalar_value_type::zero(), xi_i = scalar_value_type::one();
        for (const auto &[evals_tr, bound] : polys) {
            std::vector<std::vector<scalar_value_type>> evals;
            if (!evals_tr.evaluations.empty())
                for (std::size_t i = 0; i < evals_tr.evaluations[0].size(); ++i) {
                    std::vector<scalar_value_type> ev;
                    for (std::size_t j = 0; j < evals_tr.evaluations.size(); ++j) ev.push_back(evals_tr.evaluations[j][i]);
                    evals.push_back(ev);
                }
            for (const auto &eval : evals) {
                res = res + xi_i * evaluate(eval, r);
                xi_i = xi_i * xi;
            }
            if (bound != -1) {
                std::vector<scalar_value_type> last_evals(evaluation_points.size(), scalar_value_type::zero());
                if ((std::size_t)bound <= evals.size() * g_size) last_evals = evals[evals.size() - 1];
                std::vector<scalar_value_type> shifted_evals;
                for (std::size_t i = 0; i < last_evals.size(); ++i) shifted_evals.push_back(pow(evaluation_points[i], g_size - (std::size_t)bound % g_size) * last_evals[i]);
                res = res + xi_i * evaluate(shifted_evals, r);
                xi_i = xi_i * xi;
            }
        }
        return res;
    }

    /// :611-627
    static scalar_value_type b_poly(const std::vector<scalar_value_type> &chals, const scalar_value_type &x) {
        const std::size_t k = chals.size();
        std::vector<scalar_value_type> pow_twos = {x};
        for (std::size_t i = 1; i < k; ++i) pow_twos.push_back(pow_twos.back() * pow_twos.back());
        scalar_value_type res = scalar_value_type::one();
        for (std::size_t i = 0; i < k; ++i) res = res * (scalar_value_type::one() + chals[i] * pow_twos[k - 1 - i]);
        return res;
    }

    /// :645-755.  The scalars of [g ..., h] are assembled on the device (every batch's s vector comes from
    /// zkhip_fr_challenge_products_dev and is scaled and added in place), those of the per-proof points on the host.
    static bool verify_eval(params_type &params, group_map_type &group_map, std::vector<batchproof_type> &batches) {
        const context &ctx = params.ctx;
        const std::size_t power_of_two = params.padded;
        std::vector<group_value_type> points;      // behind the resident ones
        std::vector<scalar_value_type> scalars;
        scalar_value_type h_scalar = scalar_value_type::zero();
        auto d_scalars = ctx.alloc((power_of_two + 1) * 32), d_s = ctx.alloc(power_of_two * 32);
        bool first = true;

        const scalar_value_type rand_base = params.random();
        const scalar_value_type sg_rand_base = params.random();
        scalar_value_type rand_base_i = scalar_value_type::one(), sg_rand_base_i = scalar_value_type::one();

        for (auto &batch : batches) {
            std::vector<std::tuple<evaluation_type, int>> es;
            for (const auto &eval : batch.evaluation) es.emplace_back(eval, eval.commit.shifted.is_zero() ? -1 : eval.bound);
            const scalar_value_type combined_inner_product0 = combined_inner_product(batch.evaluation_points, batch.xi, batch.r, es, params.g.size());

            batch.sponge.absorb_fr(batch.sponge.shift_scalar(combined_inner_product0));
            const group_value_type u = group_map.to_group(batch.sponge.challenge_fq());
            const auto [chals, chal_invs] = batch.opening.challenges(params.endo_r, batch.sponge);
            batch.sponge.absorb_g(batch.opening.delta);
            const scalar_value_type cc = batch.sponge.squeeze_challenge(params.endo_r);

            scalar_value_type scale = scalar_value_type::one(), b0 = scalar_value_type::zero();
            for (const auto &e : batch.evaluation_points) {
                b0 = b0 + scale * b_poly(chals, e);
                scale = scale * batch.r;
            }

            /* scalars[1 + i] += sg_rand_base_i * s[i] over the generators, s = b_poly_coefficents(chals) */
            if (((std::size_t)1 << chals.size()) != power_of_two) return false;    // an opening of another size than this SRS
            std::vector<std::uint64_t> ch(4 * std::max<std::size_t>(1, chals.size()));
            for (std::size_t i = 0; i < chals.size(); ++i) adapter::scalar_to_limbs(chals[i], &ch[4 * i]);
            ZKHIP_CALL(ctx, zkhip_fr_challenge_products_dev, adapter::id, ch.data(), chals.size(), d_s.get());
            fv::affine(ctx, d_s.get(), first ? nullptr : d_scalars.get(), sg_rand_base_i, scalar_value_type::one(), scalar_value_type::zero(), d_scalars.get(), power_of_two);
            first = false;

            const scalar_value_type neg_rand_base_i = scalar_value_type::zero() - rand_base_i;
            points.push_back(batch.opening.sg);
            scalars.push_back(neg_rand_base_i * batch.opening.z1 - sg_rand_base_i);
            h_scalar = h_scalar - rand_base_i * batch.opening.z2;
            scalars.push_back(neg_rand_base_i * batch.opening.z1 * b0);
            points.push_back(u);

            const scalar_value_type rand_base_i_c_i = cc * rand_base_i;
            for (std::size_t i = 0; i < batch.opening.lr.size(); ++i) {
                const auto &[l, r] = batch.opening.lr[i];
                points.push_back(l);
                scalars.push_back(rand_base_i_c_i * chal_invs[i]);
                points.push_back(r);
                scalars.push_back(rand_base_i_c_i * chals[i]);
            }

            scalar_value_type xi_i = scalar_value_type::one();
            for (const auto &eval : batch.evaluation) {
                for (const auto &comm : eval.commit.unshifted) {
                    scalars.push_back(rand_base_i_c_i * xi_i);
                    points.push_back(comm);
                    xi_i = xi_i * batch.xi;
                }
                if (eval.bound >= 0 && !eval.commit.shifted.is_zero()) {
                    scalars.push_back(rand_base_i_c_i * xi_i);
                    points.push_back(eval.commit.shifted);
                    xi_i = xi_i * batch.xi;
                }
            }

            scalars.push_back(rand_base_i_c_i * combined_inner_product0);
            points.push_back(u);
            scalars.push_back(rand_base_i);
            points.push_back(batch.opening.delta);

            rand_base_i = rand_base_i * rand_base;
            sg_rand_base_i = sg_rand_base_i * sg_rand_base;
        }

        group_value_type sum = group_value_type::zero();
        if (!first) {    // the resident part: [g ..., padding, h] against what the batches left in d_scalars, h's scalar behind them
            upload_scalars<adapter>(ctx, static_cast<char *>(d_scalars.get()) + 32 * power_of_two, &h_scalar, 1);
            sum = multiexp_dev<CurveType, ZKHIP_G1>(ctx, params.srs, 0, power_of_two + 1, d_scalars.get());
        }
        if (!points.empty()) sum = sum + multiexp<multiexp_method_hip, CurveType, ZKHIP_G1>(ctx, points.begin(), points.end(), scalars.begin(), scalars.end(), 1);
        return sum.is_zero();
    }

private:
    struct bases_free {
        zkhip_ctx *ctx;
        void operator()(zkhip_bases *b) const { zkhip_bases_free(ctx, b); }
    };
    typedef std::unique_ptr<zkhip_bases, bases_free> bases_handle;

    static scalar_value_type download_scalar(const context &ctx, const void *d_src) {
        std::vector<scalar_value_type> v;
        download_scalars<adapter>(ctx, d_src, 1, v);
        return v[0];
    }
    /// the same group element with Z = 1: what a sponge absorbs (and a proof carries) is the affine point
    static group_value_type normalised(const group_value_type &p) {
        std::uint64_t xy[2 * adapter::g1_coord_limbs];
        const bool finite = adapter::point_to_affine_limbs(p, xy);
        return group_value_type::from_affine(xy, !finite);
    }
    static scalar_value_type evaluate(const std::vector<scalar_value_type> &coeffs, const scalar_value_type &x) {
        scalar_value_type acc = scalar_value_type::zero();
        for (std::size_t i = coeffs.size(); i-- > 0;) acc = acc * x + coeffs[i];
        return acc;
    }
    static scalar_value_type pow(const scalar_value_type &x, std::size_t e) {
        scalar_value_type acc = scalar_value_type::one(), sq = x;
        for (; e; e >>= 1) {
            if (e & 1) acc = acc * sq;
            sq = sq * sq;
        }
        return acc;
    }
    /// sum_i scalars[at[k] + i] * bases[k][offs[k] + i], i < ns[k], for every k in one zkhip_msm_batch_dev; the scalars are resident at d_scalars
    static std::vector<group_value_type> msm_batch(const context &ctx, const std::vector<const zkhip_bases *> &bases, const std::vector<std::size_t> &offs,
                                                   const std::vector<std::size_t> &ns, const void *d_scalars, const std::vector<std::size_t> &at) {
        const std::size_t count = ns.size();
        auto d_res = ctx.alloc(count * jac_limbs * 8);
        std::vector<const void *> qs(count);
        std::vector<void *> qr(count);
        for (std::size_t k = 0; k < count; ++k) {
            qs[k] = static_cast<const char *>(d_scalars) + 32 * at[k];
            qr[k] = static_cast<std::uint64_t *>(d_res.get()) + k * jac_limbs;
        }
        ZKHIP_CALL(ctx, zkhip_msm_batch_dev, count, bases.data(), offs.data(), ns.data(), qs.data(), qr.data());
        std::vector<std::uint64_t> res(count * jac_limbs);
        ctx.d2h(res.data(), d_res.get(), res.size() * 8);
        std::vector<group_value_type> out;
        for (std::size_t k = 0; k < count; ++k) out.push_back(adapter::g1_from_jacobian(&res[k * jac_limbs]));
        return out;
    }
};

}    // namespace hip
}    // namespace zk
}    // namespace crypto3
}    // namespace nil

#endif    // ZKHIP_SHIM_KIMCHI_PEDERSEN_HPP
