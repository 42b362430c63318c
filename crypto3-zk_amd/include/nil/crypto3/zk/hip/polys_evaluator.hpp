//---------------------------------------------------------------------------//
// zkhip shim: the polys_evaluator under the KZG schemes (kzg_v2.hpp) and the LPC scheme (lpc.hpp).
//
// Mirrors zk/commitments/batched_commitment.hpp (class polys_evaluator, :58-249) and zk/commitments/detail/polynomial/eval_storage.hpp:36-95:
// the batches, their lock flags, the evaluation points, `_z`, eval_polys, get_unique_points.  The batch rules live here alone:
//   * a batch that is committed, or sized by set_batch_size, refuses appends;
//   * copies and handed-over polynomials are kept; lent ones (std::cref) are read where they lie, their pointers dropped by state_commited;
//   * a committed batch is its coefficient forms, resident, one behind the other (detail::device_batch);
//   * the caller's root-of-unity function is called from the calling thread only, once per distinct size (detail::add_roots).
// A scheme adds its commit(batch) and its proof_eval.  Over a device group both deal the columns alike (detail::deal_columns) and gather the
// coefficient forms on member 0 (detail::gather_form).  No transcript parameter and no pairing requirement: LPC runs on Pallas and Vesta.
//---------------------------------------------------------------------------//
#ifndef ZKHIP_SHIM_POLYS_EVALUATOR_HPP
#define ZKHIP_SHIM_POLYS_EVALUATOR_HPP

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <tuple>
#include <vector>

#include "fri.hpp"

namespace nil {
namespace crypto3 {
namespace zk {
namespace hip {

/// eval_storage (eval_storage.hpp:36-95)
template <typename CurveType>
class eval_storage_hip {
    typedef typename curve_adapter<CurveType>::scalar_value_type value_type;
    std::map<std::size_t, std::vector<std::vector<value_type>>> z;

public:
    bool operator==(const eval_storage_hip &other) const { return z == other.z; }
    std::vector<std::size_t> get_batches() const {
        std::vector<std::size_t> b;
        for (const auto &it : z) b.push_back(it.first);
        return b;
    }
    std::size_t get_batches_num() const { return z.size(); }
    std::size_t get_batch_size(std::size_t batch_id) const { return z.at(batch_id).size(); }
    std::size_t get_poly_points_number(std::size_t batch_id, std::size_t poly_id) const { return z.at(batch_id)[poly_id].size(); }
    const std::vector<std::vector<value_type>> &get(std::size_t batch_id) const { return z.at(batch_id); }
    const std::vector<value_type> &get(std::size_t batch_id, std::size_t poly_id) const { return z.at(batch_id)[poly_id]; }
    const value_type &get(std::size_t batch_id, std::size_t poly_id, std::size_t point_id) const { return z.at(batch_id)[poly_id][point_id]; }
    void set_batch_size(std::size_t batch_id, std::size_t batch_size) { z[batch_id].assign(batch_size, {}); }
    void set_poly_points_number(std::size_t batch_id, std::size_t poly_id, std::size_t n) { z[batch_id][poly_id].assign(n, value_type::zero()); }
    void set(std::size_t batch_id, std::size_t poly_id, std::size_t point_id, const value_type &v) { z[batch_id][poly_id][point_id] = v; }
};

namespace detail {
    template <bool Value>
    struct constant_predicate {    // the default of the optional predicates below
        template <typename... Args> bool operator()(Args...) const { return Value; }
    };
    /// a committed batch on the device: the coefficient forms of its polynomials (its columns), one behind the other
    struct device_batch {
        std::shared_ptr<void> data;
        std::vector<std::size_t> offset, len;    // in elements
        std::size_t total = 0;                   // elements of all columns
        void *at(std::size_t i) const { return static_cast<char *>(data.get()) + 32 * offset[i]; }
        std::size_t size() const { return len.size(); }
        void append(std::size_t elements) {
            offset.push_back(total);
            len.push_back(elements);
            total += elements;
        }
        /// the elements of columns [lo, hi): one contiguous piece of the buffer
        std::size_t elements(std::size_t lo, std::size_t hi) const { return (hi < len.size() ? offset[hi] : total) - offset[lo]; }
        /// fn(i, j) for the maximal runs [i, j) of columns of equal length in [lo, hi), in order.  A run also ends after first_limit columns
        /// (the run that starts at lo) or limit columns (0: no limit), and where same(i, j) says that columns i and j are not of one kind.
        template <typename Fn, typename Same = constant_predicate<true>>
        void for_each_run(std::size_t lo, std::size_t hi, std::size_t first_limit, std::size_t limit, Fn fn, Same same = Same()) const {
            for (std::size_t i = lo; i < hi;) {
                const std::size_t lim = i == lo ? first_limit : limit;
                std::size_t j = i + 1;
                while (j < hi && len[j] == len[i] && same(i, j) && (lim == 0 || j - i < lim)) ++j;
                fn(i, j);
                i = j;
            }
        }
    };

    typedef std::map<std::size_t, std::array<std::uint64_t, 4>> root_map;    // log_n -> the limbs of the primitive 2^log_n-th root
    /// One root per distinct ceil_log2(len) of the batch's columns (those skip(i) names aside) that `roots` does not hold yet.  The caller's
    /// root-of-unity function is called from THIS thread only (it need not be thread-safe), once per size, before any member thread starts.
    template <typename Adapter, typename RootFn, typename Skip = constant_predicate<false>>
    void add_roots(root_map &roots, const device_batch &db, const RootFn &root_of_unity, Skip skip = Skip()) {
        for (std::size_t i = 0; i < db.size(); ++i) {
            const std::size_t log_n = ceil_log2(db.len[i]);
            if (!skip(i) && !roots.count(log_n)) roots[log_n] = limbs_of<Adapter>(root_of_unity(log_n));
        }
    }

    /// commit(batch) over a device group, member k's share: columns [lo, hi), a contiguous range, so their coefficient forms are ONE piece of
    /// `elems` elements of the batch buffer.  Member 0 works in the batch buffer itself, every other member in a buffer of its own (`data`).
    struct group_part {
        std::size_t lo = 0, hi = 0, elems = 0;
        std::shared_ptr<void> data;
        char *base = nullptr;
        bool empty() const { return hi == lo; }
    };
    inline group_part deal_columns(const device_batch &db, const device_group &group, std::size_t k) {
        group_part pt;
        std::tie(pt.lo, pt.hi) = even_range(db.size(), group.size(), k);
        if (pt.empty()) return pt;
        pt.elems = db.elements(pt.lo, pt.hi);
        if (k == 0) pt.base = static_cast<char *>(db.at(pt.lo));
        else {
            pt.data = group[k].alloc(pt.elems * 32);
            pt.base = static_cast<char *>(pt.data.get());
        }
        return pt;
    }
    /// member k's coefficient forms join the batch on member 0 (a peer copy; proof_eval reads them there)
    inline void gather_form(const device_batch &db, const device_group &group, std::size_t k, const group_part &pt) {
        if (k != 0 && !pt.empty()) group.copy(0, db.at(pt.lo), k, pt.base, pt.elems * 32);
    }
}    // namespace detail

/// polys_evaluator (batched_commitment.hpp:58-249).  `ctx`: where the coefficient forms live (over a device group: member 0).
/// `PolynomialType` as in the reference (:56-64; default: the shim's own polynomial_dfs): anything with size() and operator[] over contiguous
/// scalar_value_type -- math::polynomial_dfs as placeholder_prover hands it over (prover.hpp:137-138, 316) included.
template <typename CurveType, typename PolynomialType = polynomial_dfs<CurveType>>
class polys_evaluator_hip {
public:
    typedef curve_adapter<CurveType> adapter;
    typedef CurveType curve_type;
    typedef typename adapter::scalar_value_type scalar_value_type;
    typedef PolynomialType poly_type;
    typedef eval_storage_hip<CurveType> eval_storage_type;

    eval_storage_type _z;

    /// `members`: how many devices commit(batch) spreads over (a device group's world; 1: `ctx` alone)
    explicit polys_evaluator_hip(const context &ctx, std::size_t members = 1) : _ctx(ctx), _upload(std::max<std::size_t>(1, members)) { }

    // ---- batched_commitment.hpp:197-247 ----
    /// as the reference: the scheme keeps a COPY of the polynomial (batched_commitment.hpp:197-206)
    void append_to_batch(std::size_t index, const poly_type &poly) { own(index, poly_type(poly)); }
    template <typename ContainerType>
    void append_to_batch(std::size_t index, const ContainerType &polys) {
        for (const auto &p : polys) append_one(index, p);
    }
    /// a caller that is done with the polynomials hands them over instead (50 x 2^20 rows: 340 ms of host copying saved) ...
    void append_to_batch(std::size_t index, poly_type &&poly) { own(index, std::move(poly)); }
    void append_to_batch(std::size_t index, std::vector<poly_type> &&polys) {
        for (auto &p : polys) own(index, std::move(p));
        polys.clear();
    }
    /// ... and one that keeps them alive until commit(index) returns LENDS them: std::cref(poly), or a container of
    /// std::reference_wrapper<const poly_type> -- nothing is copied on the host, commit reads the caller's vectors where they lie
    void append_to_batch(std::size_t index, std::reference_wrapper<const poly_type> poly) {
        if (_locked[index]) throw std::runtime_error("append_to_batch: batch already committed");
        _polys[index].push_back(&poly.get());
    }
    void append_eval_point(std::size_t batch_id, const scalar_value_type &point) {
        for (auto &pts : _points.at(batch_id)) pts.push_back(point);
    }
    void append_eval_point(std::size_t batch_id, std::size_t poly_id, const scalar_value_type &point) { _points.at(batch_id).at(poly_id).push_back(point); }
    void append_eval_points(std::size_t batch_id, const std::vector<scalar_value_type> &points) {
        for (auto &pts : _points.at(batch_id)) pts.insert(pts.end(), points.begin(), points.end());
    }
    void append_eval_points(std::size_t batch_id, std::size_t poly_id, const std::vector<scalar_value_type> &points) {
        auto &pts = _points.at(batch_id).at(poly_id);
        pts.insert(pts.end(), points.begin(), points.end());
    }
    void set_batch_size(std::size_t batch_id, std::size_t batch_size) {
        _points[batch_id].resize(batch_size);
        _locked[batch_id] = true;
    }

protected:
    typedef detail::device_batch device_batch;
    typedef detail::root_map root_map;

    void own(std::size_t index, poly_type &&poly) {
        if (_locked[index]) throw std::runtime_error("append_to_batch: batch already committed");
        _owned[index].push_back(std::move(poly));
        _polys[index].push_back(&_owned[index].back());
    }
    void append_one(std::size_t index, const poly_type &p) { own(index, poly_type(p)); }
    void append_one(std::size_t index, std::reference_wrapper<const poly_type> p) { append_to_batch(index, p); }

    /// state_commited (batched_commitment.hpp:163-166).  The host polynomials are not read again: lent ones may go; copies and
    /// handed-over ones are released with the scheme (freeing gigabytes of host memory here costs ~100 ms: more than the upload)
    void state_commited(std::size_t index, device_batch &&db) {
        _locked[index] = true;
        _points[index].resize(db.size());
        _dev[index] = std::move(db);
        _polys[index].clear();    // no pointer to a lent polynomial outlives the call
    }

    /// eval_polys (batched_commitment.hpp:168-183): every polynomial of a batch at the union of the batch's points
    void eval_polys() {
        for (const auto &it : _dev) {
            const std::size_t k = it.first;
            const device_batch &db = it.second;
            const auto &point = _points.at(k);
            _z.set_batch_size(k, db.size());
            std::vector<scalar_value_type> uni;
            add_unique(uni, point);
            std::vector<std::uint64_t> pts(4 * uni.size());
            for (std::size_t j = 0; j < uni.size(); ++j) adapter::scalar_to_limbs(uni[j], &pts[4 * j]);
            const std::vector<std::uint64_t> vals = evaluate_runs(db, pts.data(), uni.size());
            for (std::size_t p = 0; p < db.size(); ++p) {
                _z.set_poly_points_number(k, p, point[p].size());
                for (std::size_t q = 0; q < point[p].size(); ++q) {
                    const std::size_t u = std::find(uni.begin(), uni.end(), point[p][q]) - uni.begin();
                    _z.set(k, p, q, adapter::scalar_from_limbs(&vals[4 * (p * uni.size() + u)]));
                }
            }
        }
    }
    /// every polynomial of committed batch k at x
    std::vector<scalar_value_type> evaluate_batch_at(std::size_t k, const scalar_value_type &x) const {
        const device_batch &db = _dev.at(k);
        const std::vector<std::uint64_t> vals = evaluate_runs(db, limbs_of<adapter>(x).data(), 1);
        std::vector<scalar_value_type> out(db.size());
        for (std::size_t p = 0; p < db.size(); ++p) out[p] = adapter::scalar_from_limbs(&vals[4 * p]);
        return out;
    }
    /// get_unique_points (batched_commitment.hpp:113-129): first-seen order over batches, polynomials, points
    std::vector<scalar_value_type> unique_points() const {
        std::vector<scalar_value_type> result;
        for (const auto &it : _points) add_unique(result, it.second);
        return result;
    }

    /// Member k's upload stream: the second in-order stream the uploads of commit() ride on, on the GPU of `on` (member k's context), created
    /// on first use.  The slots are sized in the constructor and never resized: the member threads of for_each_member each touch their own
    /// slot only, and none of them may see the vector move.
    const context &upload_context(std::size_t k, const context &on) const {
        std::unique_ptr<context> &up = _upload.at(k);
        if (!up) up.reset(new context(on.device()));
        return *up;
    }

    const context &_ctx;
    std::map<std::size_t, std::vector<const poly_type *>> _polys;    // in append order: copies held in _owned, or the caller's (lent)
    std::map<std::size_t, std::deque<poly_type>> _owned;             // a deque: references stay valid as it grows
    std::map<std::size_t, bool> _locked;
    std::map<std::size_t, std::vector<std::vector<scalar_value_type>>> _points;
    std::map<std::size_t, device_batch> _dev;

private:
    mutable std::vector<std::unique_ptr<context>> _upload;    // one slot per member, see upload_context

    static void add_unique(std::vector<scalar_value_type> &out, const std::vector<std::vector<scalar_value_type>> &point_sets) {
        for (const auto &point_set : point_sets)
            for (const auto &point : point_set)
                if (std::find(out.begin(), out.end(), point) == out.end()) out.push_back(point);
    }
    /// every polynomial of `db` at `count` points (canonical limbs): the value of polynomial p at point u at [4 (p count + u)]; one
    /// zkhip_poly_eval_dev per run of polynomials of equal length
    std::vector<std::uint64_t> evaluate_runs(const device_batch &db, const std::uint64_t *pts, std::size_t count) const {
        std::vector<std::uint64_t> vals(4 * db.size() * count);
        if (count != 0)
            db.for_each_run(0, db.size(), 0, 0, [&](std::size_t i, std::size_t j) {
                ZKHIP_CALL(_ctx, zkhip_poly_eval_dev, adapter::id, db.at(i), db.len[i], db.len[i], j - i, pts, count, &vals[4 * i * count]);
            });
        return vals;
    }
};

}    // namespace hip
}    // namespace zk
}    // namespace crypto3
}    // namespace nil

#endif    // ZKHIP_SHIM_POLYS_EVALUATOR_HPP
