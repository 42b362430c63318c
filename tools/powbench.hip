// Micro-benchmark of the proof-of-work candidate function (crypto3-zk_amd/csrc/pow.hpp) on the device: the kernel shape of pow.hip
// (16 offsets per lane, one chunk of 2^28 offsets, no hit expected under the full mask) over two forms of candidate():
//   plain     two calls of sha256::compress, as the definition reads (the compiler folds the constant block words and drops what h[7]
//             of the second hash does not depend on by itself)
//   shipped   pow::candidate: the first block from the host-computed state after rounds 0..7 and schedule words 16..22
// Prints one JSON line per form: candidates/s, median and spread of `runs` timed launches (HIP events) after two warm-up launches, and checks
// every form against the host's plain form on 4096 nonces first.     make -C tools powbench && tools/powbench [runs]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../crypto3-zk_amd/csrc/pow.hpp"

using namespace zkhip;

#define CHECK(expr)                                                                     \
    do {                                                                                \
        hipError_t e__ = (expr);                                                        \
        if (e__ != hipSuccess) {                                                        \
            fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e__));                 \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

template <int Form>
__host__ __device__ inline uint32_t candidate_form(const pow::Search &s, uint32_t n) {
    if (Form == 1) return pow::candidate(s, n);
    uint32_t h[8], w[16];
    sha256::init(h);
    for (int k = 0; k < 8; ++k) w[k] = s.st[k];
    pow::first_block_tail(w, n);
    sha256::compress(h, w);
    for (int k = 0; k < 8; ++k) w[k] = h[k];
    sha256::pad_words(w, 8, 32);
    sha256::init(h);
    sha256::compress(h, w);
    return h[7];
}

template <int Form>
__global__ __launch_bounds__(256) void grind(pow::Search s, uint32_t first, uint64_t count, uint32_t mask, unsigned long long *hit) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        if ((candidate_form<Form>(s, first + (uint32_t)i) & mask) != 0) continue;
        if (i < *(volatile unsigned long long *)hit) atomicMin(hit, (unsigned long long)i);
        return;
    }
}

template <int Form>
__global__ void values(pow::Search s, uint32_t first, uint32_t count, uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = candidate_form<Form>(s, first + i);
}

template <int Form>
int run(const char *name, const pow::Search &s, int runs, unsigned long long *d_hit, uint32_t *d_out) {
    const uint32_t first = 0xFFFFF800u, n = 4096;  // across the wrap
    std::vector<uint32_t> got(n);
    values<Form><<<n / 256, 256>>>(s, first, n, d_out);
    CHECK(hipMemcpy(got.data(), d_out, n * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i)
        if (got[i] != candidate_form<0>(s, first + i)) {
            fprintf(stderr, "%s: candidate %u differs from the host's plain form\n", name, i);
            return 1;
        }
    const uint64_t count = (uint64_t)1 << 28;
    const unsigned blocks = (unsigned)(count / (256 * 16));
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    std::vector<double> rate;
    for (int r = -2; r < runs; ++r) {
        CHECK(hipMemset(d_hit, 0xFF, 8));
        CHECK(hipEventRecord(a));
        grind<Form><<<blocks, 256>>>(s, 12345u, count, 0xFFFFFFFFu, d_hit);
        CHECK(hipEventRecord(b));
        CHECK(hipEventSynchronize(b));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, a, b));
        if (r >= 0) rate.push_back((double)count / (ms * 1e-3));
    }
    std::sort(rate.begin(), rate.end());
    printf("{\"form\": \"%s\", \"candidates\": %llu, \"runs\": %d, \"candidates_per_s_median\": %.4g, \"min\": %.4g, \"max\": %.4g}\n", name,
           (unsigned long long)count, runs, rate[rate.size() / 2], rate.front(), rate.back());
    CHECK(hipEventDestroy(a));
    CHECK(hipEventDestroy(b));
    return 0;
}

int main(int argc, char **argv) {
    const int runs = argc > 1 ? std::max(1, atoi(argv[1])) : 10;
    uint8_t state[32];
    for (int k = 0; k < 32; ++k) state[k] = (uint8_t)(37 * k + 11);
    const pow::Search s = pow::prepare(state);
    unsigned long long *d_hit = nullptr;
    uint32_t *d_out = nullptr;
    CHECK(hipMalloc(&d_hit, 8));
    CHECK(hipMalloc(&d_out, 4096 * 4));
    if (run<0>("plain", s, runs, d_hit, d_out) || run<1>("shipped", s, runs, d_hit, d_out)) return 1;
    CHECK(hipFree(d_hit));
    CHECK(hipFree(d_out));
    return 0;
}
