// The one-point-per-wave group law (csrc/fu_wide.hpp) against the one-lane formulas of csrc/curve.hpp and the one-lane product of csrc/fu.hpp, on
// arbitrary field elements (the formulas are algebraic identities; no curve membership needed): BLS12-381, BN254, Pallas and Vesta base fields.
// One wave per case; every lane computes the one-lane reference, the wave computes the wide result, coordinates compared after canonicalisation
// (products: limb for limb too -- fu_wide.hpp promises the very limbs of fu_mul).  Cases by wave: random operands; P + P; P + (-P); infinity on
// either side; coordinates 0, 1 and p - 1; in every wave the product at the limb bound of the contract (all limbs 2^30 - 1), a chain of 64
// dependent additions / doublings, the small multiple and the load / store round trip.
// Exit code 0 and "mismatch mask 0x0" on every line = pass.  Device only: run on the GPU box (tests/test_gpu_msm_wide.py).
#include <hip/hip_runtime.h>

#include <cstdio>

#include "fu_wide.hpp"

using namespace zkhip;

enum { BAD_ADD = 1, BAD_DBL = 2, BAD_MULTIPLE = 4, BAD_PRODUCT = 8, BAD_BOUND = 16, BAD_CHAIN = 32, BAD_MEMORY = 64 };
constexpr int CASES = 64;

template <class U>
__device__ bool same(const Fu<U> &x, const Fu<U> &y) { return fu_canon(x).limbs_equal(fu_canon(y)); }
template <class U>
__device__ bool same_point(const XYZZ<Fu<U>> &p, const XYZZ<FuW<U>> &w) {
    const XYZZ<FuQ<U>> g = wide_gather<U>(w);
    return same(p.X, g.X.v) && same(p.Y, g.Y.v) && same(p.ZZ, g.ZZ.v) && same(p.ZZZ, g.ZZZ.v);
}
template <class U>
__device__ XYZZ<FuW<U>> widen(const XYZZ<Fu<U>> &p) { return wide_scatter<U>(XYZZ<FuQ<U>>{{p.X}, {p.Y}, {p.ZZ}, {p.ZZZ}}); }

// one wave per block; mem: CASES points in device-buffer layout (4 * SL words), written here by the wide store and read back by the next launch
template <class U>
__global__ __launch_bounds__(64) void k(const uint32_t *in, uint32_t *mem, uint32_t *bad) {
    constexpr int L = U::L;
    const int w = blockIdx.x;
    const uint32_t lane = wide_lane();
    XYZZ<Fu<U>> a, b;
    Fu<U> *fa[4] = {&a.X, &a.Y, &a.ZZ, &a.ZZZ}, *fb[4] = {&b.X, &b.Y, &b.ZZ, &b.ZZZ};
    for (int c = 0; c < 4; ++c) {
        for (int i = 0; i < L; ++i) {
            fa[c]->v[i] = in[(w * 97 + c * 31 + i) & 4095] & Fu<U>::MASK;
            fb[c]->v[i] = in[(w * 89 + c * 37 + i + 1000) & 4095] & Fu<U>::MASK;
        }
        // below p (top limb: 0 where the modulus reaches into it, the last value limb cut where it does not), then one product: < 2p like real coordinates
        const int top = U::mod(L - 1) ? L - 1 : L - 2;
        fa[c]->v[L - 1] = 0, fb[c]->v[L - 1] = 0;
        fa[c]->v[top] &= U::mod(top) >> 1, fb[c]->v[top] &= U::mod(top) >> 1;
        *fa[c] = fu_mul(*fa[c], Fu<U>::r2());
        *fb[c] = fu_mul(*fb[c], Fu<U>::r2());
    }
    Fu<U> pm1 = Fu<U>::modulus();
    pm1.v[0] -= 1;  // p is odd
    const int mode = w & 7;
    if (mode == 3) b = a;                                                                        // P + P
    if (mode == 4) b = {a.X, fu_sub<FieldOps<Fu<U>>::K1>(Fu<U>::zero(), a.Y), a.ZZ, a.ZZZ};      // P + (-P)
    if (mode == 5) a = XYZZ<Fu<U>>::infinity();
    if (mode == 6) b = XYZZ<Fu<U>>::infinity();
    if (mode == 7) {                                                                             // 0, 1 and p - 1 as coordinates
        a.X = Fu<U>::zero(), a.Y = Fu<U>::one(), a.ZZ = pm1;
        b.X = pm1, b.Y = Fu<U>::zero(), b.ZZZ = Fu<U>::one();
        if (w & 8) b.ZZ = Fu<U>::plain_one(), a.ZZZ = pm1;
    }
    const XYZZ<FuW<U>> aw = widen(a), bw = widen(b);
    unsigned m = 0;

    // products, row by row: X X', Y Y', ZZ ZZ', ZZZ ZZZ' -- the very limbs of fu_mul
    {
        const XYZZ<FuQ<U>> g = wide_gather<U>(XYZZ<FuW<U>>{wide_mul<U>(aw.w, bw.w)});
        if (!g.X.v.limbs_equal(fu_mul(a.X, b.X)) || !g.Y.v.limbs_equal(fu_mul(a.Y, b.Y)) || !g.ZZ.v.limbs_equal(fu_mul(a.ZZ, b.ZZ)) ||
            !g.ZZZ.v.limbs_equal(fu_mul(a.ZZZ, b.ZZZ)))
            m |= BAD_PRODUCT;
    }
    // at the bound of the contract: every limb 2^30 - 1 below the top one (x x < R p for all three fields), squared and against a coordinate
    {
        Fu<U> x;
        for (int i = 0; i < L; ++i) x.v[i] = i < L - 1 ? 0x3fffffffu : 0u;
        const uint32_t xw = (lane & 15u) < (uint32_t)(L - 1) ? 0x3fffffffu : 0u;
        const XYZZ<FuQ<U>> g = wide_gather<U>(XYZZ<FuW<U>>{wide_mul<U>(xw, wide_pick(xw, bw.w, xw, bw.w))});
        if (!g.X.v.limbs_equal(fu_mul(x, x)) || !g.Y.v.limbs_equal(fu_mul(x, b.Y)) || !g.ZZ.v.limbs_equal(fu_mul(x, x)) || !g.ZZZ.v.limbs_equal(fu_mul(x, b.ZZZ)))
            m |= BAD_BOUND;
        // sums and differences at theirs: normalised limbs all 2^29 - 1
        Fu<U> y;
        for (int i = 0; i < L; ++i) y.v[i] = i < L - 1 ? Fu<U>::MASK : 0u;
        const uint32_t yw = (lane & 15u) < (uint32_t)(L - 1) ? Fu<U>::MASK : 0u;
        const XYZZ<FuQ<U>> s = wide_gather<U>(XYZZ<FuW<U>>{wide_add<U>(yw, wide_pick(yw, aw.w, 1u & (uint32_t)((lane & 15u) == 0), bw.w))});
        Fu<U> one_limb = Fu<U>::zero();
        one_limb.v[0] = 1;
        if (!s.X.v.limbs_equal(fu_add(y, y)) || !s.Y.v.limbs_equal(fu_add(y, a.Y)) || !s.ZZ.v.limbs_equal(fu_add(y, one_limb)) || !s.ZZZ.v.limbs_equal(fu_add(y, b.ZZZ)))
            m |= BAD_BOUND;
        const XYZZ<FuQ<U>> d = wide_gather<U>(XYZZ<FuW<U>>{wide_sub<8, U>(aw.w, bw.w)});
        if (!d.X.v.limbs_equal(fu_sub<8>(a.X, b.X)) || !d.Y.v.limbs_equal(fu_sub<8>(a.Y, b.Y)) || !d.ZZ.v.limbs_equal(fu_sub<8>(a.ZZ, b.ZZ)) ||
            !d.ZZZ.v.limbs_equal(fu_sub<8>(a.ZZZ, b.ZZZ)))
            m |= BAD_BOUND;
    }
    if (!same_point(xyzz_add(a, b), xyzz_add(aw, bw))) m |= BAD_ADD;
    if (!same_point(xyzz_add(b, a), xyzz_add(bw, aw))) m |= BAD_ADD;
    if (!same_point(xyzz_dbl(a), xyzz_dbl(aw))) m |= BAD_DBL;
    if (!same_point(xyzz_dbl(b), xyzz_dbl(bw))) m |= BAD_DBL;
    // the multiple by the wide code's own chain (double, then add where the bit is set): off the curve two DIFFERENT addition chains need not
    // meet, so the one-lane reference follows the same one
    {
        const uint32_t kk = (w & 16) ? 1 + (in[w & 4095] & 0x3ff) : (uint32_t)(w >> 5);  // 0 and 1 among them
        XYZZ<Fu<U>> m1 = kk ? a : XYZZ<Fu<U>>::infinity();
        for (int i = 31 - __builtin_clz(kk | 1) - 1; i >= 0; --i) {
            m1 = xyzz_dbl(m1);
            if ((kk >> i) & 1) m1 = xyzz_add(m1, a);
        }
        if (!same_point(m1, xyzz_mul_small(aw, kk))) m |= BAD_MULTIPLE;
    }
    // 64 dependent operations: the limb bounds as they compound
    {
        XYZZ<Fu<U>> r = a;
        XYZZ<FuW<U>> rw = aw;
        for (int i = 0; i < 64; ++i) {
            if (i % 3 == 2) r = xyzz_dbl(r), rw = xyzz_dbl(rw);
            else r = xyzz_add(r, b), rw = xyzz_add(rw, bw);
        }
        if (!same_point(r, rw)) m |= BAD_CHAIN;
    }
    // memory: what the previous launch's wide store left is what the one-lane load reads, and the wide load of it is the point again
    {
        const XYZZ<FuW<U>> sum = xyzz_add(aw, bw);
        uint32_t *slot = mem + (size_t)w * 4 * U::SL;
        if (in[4096]) {  // second launch
            const XYZZ<Fu<U>> back = xyzz_load<Fu<U>>(slot);
            const XYZZ<FuQ<U>> g = wide_gather<U>(sum), h = wide_gather<U>(wide_load<U>(slot));
            if (!back.X.limbs_equal(g.X.v) || !back.Y.limbs_equal(g.Y.v) || !back.ZZ.limbs_equal(g.ZZ.v) || !back.ZZZ.limbs_equal(g.ZZZ.v)) m |= BAD_MEMORY;
            if (!back.X.limbs_equal(h.X.v) || !back.Y.limbs_equal(h.Y.v) || !back.ZZ.limbs_equal(h.ZZ.v) || !back.ZZZ.limbs_equal(h.ZZZ.v)) m |= BAD_MEMORY;
            for (int i = L; i < U::SL; ++i)
                if (slot[i] | slot[U::SL + i] | slot[2 * U::SL + i] | slot[3 * U::SL + i]) m |= BAD_MEMORY;  // the padding words stay 0
        } else {
            wide_store<U>(slot, sum);
        }
    }
    if (m) atomicOr(bad, m);
}

template <class U>
unsigned run(const char *name) {
    static uint32_t h[4097];
    uint32_t *din, *dmem, *dbad, bad = 0xffffffffu;
    for (int i = 0; i < 4096; ++i) h[i] = i * 2654435761u + 977;
    const size_t mem_bytes = (size_t)CASES * 4 * U::SL * 4;
    if (hipMalloc(&din, sizeof(h)) != hipSuccess || hipMalloc(&dmem, mem_bytes) != hipSuccess || hipMalloc(&dbad, 4) != hipSuccess) return bad;
    (void)hipMemset(dbad, 0, 4), (void)hipMemset(dmem, 0xff, mem_bytes);
    for (uint32_t pass = 0; pass < 2; ++pass) {
        h[4096] = pass;
        (void)hipMemcpy(din, h, sizeof(h), hipMemcpyHostToDevice);
        hipLaunchKernelGGL(k<U>, dim3(CASES), dim3(64), 0, 0, din, dmem, dbad);
        if (hipDeviceSynchronize() != hipSuccess) break;
    }
    if (hipMemcpy(&bad, dbad, 4, hipMemcpyDeviceToHost) != hipSuccess) bad = 0xffffffffu;
    printf("%s: mismatch mask 0x%x (add / dbl / multiple / product / at the bounds / chain of 64 / load-store = 1 / 2 / 4 / 8 / 16 / 32 / 64)\n", name, bad);
    (void)hipFree(din), (void)hipFree(dmem), (void)hipFree(dbad);
    return bad;
}

int main() {
    const unsigned a = run<BlsFqU>("BLS12-381 Fq"), b = run<BnFqU>("BN254 Fq"), c = run<PallasFqU>("Pallas Fq"), d = run<VestaFqU>("Vesta Fq");
    return (a | b | c | d) ? 1 : 0;
}
