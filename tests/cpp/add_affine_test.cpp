// xyzz_add_affine(a, b) against xyzz_madd(from_affine(a), b) on the host build of curve.hpp (test-only, stands alone: no libzkhip.so, no GPU).
// Per coordinate field (BLS12-381, BN254, Pallas, Vesta Fq): X, Y, ZZ, ZZZ of both formulas agree after canonicalisation over
//   - 1 000 random pairs, each with y as loaded and with y negated through sub<K1>(0, y) on either side (what the bucket kernel feeds it);
//   - b = a (the doubling branch) and b = -a (infinity), -a as the canonical p - y and as sub<K1>(0, y);
//   - every a, b whose coordinates run over {0, 1, p - 1, two random values}, (0, 0) = the point at infinity among them.
// The formulas are algebraic identities, so the points need not lie on the curve.  Prints one line per field, exits 0 when all agree.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "curve.hpp"

using namespace zkhip;

template <class U>
struct Case {
    typedef Fu<U> F;
    typedef FieldOps<F> O;
    static constexpr int NL = U::NL;
    std::mt19937_64 rng;
    long checked = 0, failed = 0;

    explicit Case(uint64_t seed) : rng(seed) {}

    // canonical limbs of a value below p: random limbs, the top one reduced below the modulus' top limb
    F random() {
        uint32_t w[NL];
        for (int i = 0; i < NL; ++i) w[i] = (uint32_t)rng();
        w[NL - 1] %= U::sat::mod(NL - 1);
        return O::from_canonical(w);
    }
    static F small(uint32_t v) {
        uint32_t w[NL] = {v};
        return O::from_canonical(w);
    }
    static F p_minus(uint32_t v) {  // p - v, v small
        uint32_t w[NL];
        uint64_t borrow = v;
        for (int i = 0; i < NL; ++i) {
            uint64_t t = (uint64_t)U::sat::mod(i) - borrow;
            w[i] = (uint32_t)t;
            borrow = (t >> 32) & 1;
        }
        return O::from_canonical(w);
    }
    static F neg_canonical(const F &y) {  // the canonical p - y (0 stays 0)
        uint32_t c[NL], w[NL];
        O::to_canonical(c, y);
        bool zero = true;
        uint64_t borrow = 0;
        for (int i = 0; i < NL; ++i) {
            zero = zero && c[i] == 0;
            uint64_t t = (uint64_t)U::sat::mod(i) - c[i] - borrow;
            w[i] = (uint32_t)t;
            borrow = (t >> 32) & 1;
        }
        return zero ? y : O::from_canonical(w);
    }
    static F neg_lazy(const F &y) { return O::template sub<O::K1>(F::zero(), y); }

    static bool same(const F &x, const F &y) {
        uint32_t a[NL], b[NL];
        O::to_canonical(a, x);
        O::to_canonical(b, y);
        return std::memcmp(a, b, sizeof a) == 0;
    }
    void check(const Affine<F> &a, const Affine<F> &b, const char *what) {
        const XYZZ<F> got = xyzz_add_affine(a, b), want = xyzz_madd(XYZZ<F>::from_affine(a), b);
        ++checked;
        if (got.is_inf() != want.is_inf() || !same(got.X, want.X) || !same(got.Y, want.Y) || !same(got.ZZ, want.ZZ) || !same(got.ZZZ, want.ZZZ)) {
            if (failed++ < 5) std::fprintf(stderr, "  mismatch (%s), check %ld\n", what, checked);
        }
    }
    // a + b with y as given and negated the kernel's way on either side
    void check_signs(const Affine<F> &a, const Affine<F> &b, const char *what) {
        check(a, b, what);
        if (!a.is_inf()) check({a.x, neg_lazy(a.y)}, b, what);
        if (!b.is_inf()) check(a, {b.x, neg_lazy(b.y)}, what);
        if (!a.is_inf() && !b.is_inf()) check({a.x, neg_lazy(a.y)}, {b.x, neg_lazy(b.y)}, what);
    }
    bool run(const char *name) {
        for (int i = 0; i < 1000; ++i) {
            const Affine<F> a = {random(), random()}, b = {random(), random()};
            check_signs(a, b, "random pair");
            if (i < 100) {
                check_signs(a, a, "b = a");
                check(a, {a.x, neg_canonical(a.y)}, "b = -a, canonical");
                check(a, {a.x, neg_lazy(a.y)}, "b = -a, sub<K1>(0, y)");
                check({a.x, neg_lazy(a.y)}, a, "a = -b, sub<K1>(0, y)");
                check({a.x, neg_lazy(a.y)}, {a.x, neg_lazy(a.y)}, "b = a, both negated");
            }
        }
        const std::vector<F> edge = {F::zero(), small(1), p_minus(1), random(), random()};
        for (const F &ax : edge)
            for (const F &ay : edge)
                for (const F &bx : edge)
                    for (const F &by : edge) check_signs({ax, ay}, {bx, by}, "edge coordinates");
        std::printf("%s: %ld checks, %ld mismatches\n", name, checked, failed);
        return failed == 0;
    }
};

int main() {
    bool ok = true;
    ok = Case<BlsFqU>(1).run("BLS12-381 Fq") && ok;
    ok = Case<BnFqU>(2).run("BN254 Fq") && ok;
    ok = Case<PallasFqU>(3).run("Pallas Fq") && ok;
    ok = Case<VestaFqU>(4).run("Vesta Fq") && ok;
    return ok ? 0 : 1;
}
