// What more than one C++ shim test harness needs (test-only): the wrapper of an extern "C" entry, the check that a call throws
// std::invalid_argument, a random source that hands out a list, and the conversion between affine limbs and the shim's point values.
#pragma once
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include <nil/crypto3/zk/hip/algebra.hpp>

namespace harness {

/// fn(), or `code` after printing "name: what()" when it throws: no exception crosses the C boundary
template <typename Fn>
int guarded(const char *name, Fn &&fn, int code = -1) {
    try {
        return fn();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s: %s\n", name, e.what());
        return code;
    }
}

/// whether fn() threw std::invalid_argument; anything else it throws goes on to the caller (to `guarded`)
template <typename Fn>
bool throws_invalid(Fn &&fn) {
    try {
        fn();
        return false;
    } catch (const std::invalid_argument &) {
        return true;
    }
}

/// a random source that hands out the caller's scalars (4 limbs each) in order
template <typename Curve>
struct list_random {
    typedef nil::crypto3::zk::hip::curve_adapter<Curve> A;
    const std::uint64_t *values;
    std::size_t count, pos = 0;
    typename A::scalar_value_type operator()() {
        if (pos >= count) throw std::out_of_range("list_random: out of draws");
        return A::scalar_from_limbs(values + 4 * pos++);
    }
};

/// n points of type G from canonical affine coordinates (2 G::coord_limbs limbs per point); inf: one flag per point, or none at all
template <typename G>
std::vector<G> read_points(const std::uint64_t *xy, const std::uint8_t *inf, std::size_t n) {
    std::vector<G> v;
    for (std::size_t i = 0; i < n; ++i) v.push_back(G::from_affine(xy + i * 2 * G::coord_limbs, inf && inf[i]));
    return v;
}
/// -> the position behind what was written: 2 coordinates per point into xy, one flag into inf
template <typename G>
void write_points(const std::vector<G> &v, std::uint64_t *&xy, std::uint8_t *&inf) {
    for (const G &g : v) {
        *inf++ = g.to_affine(xy) ? 0 : 1;
        xy += 2 * G::coord_limbs;
    }
}

}    // namespace harness
