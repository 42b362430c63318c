// Latency of ONE dependent group operation for a wave that has its SIMD (nearly) to itself: the one-point-per-wave law (csrc/fu_wide.hpp) against
// the lane-quad law (csrc/fu_quad.hpp) under the same harness -- a chain of N additions (doublings) per wave, 1 or 2 waves per SIMD on 256 CUs.
// Operands are arbitrary field elements (the formulas are algebraic identities); the time is the slowest wave's, by the constant 100 MHz counter.
//   make -C tools widebench && tools/widebench        (EXPERIMENTS.md has the figures)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "fu_wide.hpp"

using namespace zkhip;
constexpr int N = 256;

template <class U, int WIDE, int DBL>
__global__ __launch_bounds__(512) void k(const uint32_t *in, uint32_t *out, uint64_t *ticks) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    uint64_t t0, t1;
    if constexpr (WIDE) {
        XYZZ<FuW<U>> r = wide_load<U>(in), b = wide_load<U>(in + 4 * U::SL);
        t0 = wall_clock64();
#pragma unroll 1
        for (int i = 0; i < N; ++i) r = DBL ? xyzz_dbl(r) : xyzz_add(r, b);
        t1 = wall_clock64();
        wide_store<U>(out + (size_t)wave * 4 * U::SL, r);
    } else {
        XYZZ<FuQ<U>> r = xyzz_load<FuQ<U>>(in), b = xyzz_load<FuQ<U>>(in + 4 * U::SL);
        t0 = wall_clock64();
#pragma unroll 1
        for (int i = 0; i < N; ++i) r = DBL ? xyzz_dbl(r) : xyzz_add(r, b);
        t1 = wall_clock64();
        if ((threadIdx.x & 63) == 0) xyzz_store<FuQ<U>>(out + (size_t)wave * 4 * U::SL, r);
    }
    if ((threadIdx.x & 63) == 0) ticks[wave] = t1 - t0;
}

template <class U, int WIDE, int DBL>
double run(int waves_per_simd) {
    const int blocks = 256, threads = 256 * waves_per_simd, waves = blocks * threads / 64;
    std::vector<uint32_t> h(8 * U::SL, 0);
    for (int c = 0; c < 8; ++c)
        for (int i = 0; i < U::L - 1; ++i) h[c * U::SL + i] = ((c * 131 + i) * 2654435761u + 12345) & ((1u << 28) - 1);  // below p, normalised limbs
    uint32_t *din, *dout;
    uint64_t *dt;
    if (hipMalloc(&din, h.size() * 4) != hipSuccess || hipMalloc(&dout, (size_t)waves * 4 * U::SL * 4) != hipSuccess || hipMalloc(&dt, waves * 8) != hipSuccess) return -1;
    (void)hipMemcpy(din, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    std::vector<uint64_t> t(waves);
    for (int rep = 0; rep < 2; ++rep) {  // the second launch counts (code in the instruction cache)
        hipLaunchKernelGGL((k<U, WIDE, DBL>), dim3(blocks), dim3(threads), 0, 0, din, dout, dt);
        if (hipDeviceSynchronize() != hipSuccess) return -1;
    }
    (void)hipMemcpy(t.data(), dt, waves * 8, hipMemcpyDeviceToHost);
    (void)hipFree(din), (void)hipFree(dout), (void)hipFree(dt);
    return (double)*std::max_element(t.begin(), t.end()) * 0.01 / N;  // us per operation
}

template <class U>
void field(const char *name) {
    for (int wps : {1, 2}) {
        const double qa = run<U, 0, 0>(wps), wa = run<U, 1, 0>(wps), qd = run<U, 0, 1>(wps), wd = run<U, 1, 1>(wps);
        printf("%s  %d wave(s) per SIMD   addition: quad %.2f us  wide %.2f us  (x%.2f)   doubling: quad %.2f us  wide %.2f us  (x%.2f)\n", name, wps, qa, wa, qa / wa,
               qd, wd, qd / wd);
    }
}

int main() {
    field<BlsFqU>("BLS12-381 Fq (14 limbs)");
    field<BnFqU>("BN254 Fq     (10 limbs)");
    return 0;
}
