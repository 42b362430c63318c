// The LDS scan of the MSM's entries stage (csrc/msm_block_scan.hpp: block_inclusive_scan) by itself, on workgroups of 256 and of 1024 lanes,
// against a serial prefix sum on the host: all zeros, all ones, one non-zero word in the last lane, values whose total is 2^32 - 1, and
// random words whose sums wrap.  The kernel scans twice over the same LDS words, as the stage's callers do, so that a word left over from
// the first scan would show in the second.
// Exit code 0 and "ok" on every line = pass.  Device only: run on the GPU box (tests/test_gpu_msm_entries_latency.py).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "msm_block_scan.hpp"

using namespace zkhip;

template <uint32_t THREADS>
__global__ __launch_bounds__(THREADS) void scan_twice(const uint32_t *__restrict__ in, uint32_t *__restrict__ out) {
    __shared__ uint32_t part[THREADS];
    const uint32_t t = threadIdx.x, base = blockIdx.x * 2 * THREADS;
    for (uint32_t half = 0; half < 2; ++half) {
        part[t] = in[base + half * THREADS + t];
        block_inclusive_scan<THREADS>(part);
        out[base + half * THREADS + t] = part[t];
        __syncthreads();
    }
}

template <uint32_t THREADS>
int run(const char *name, const std::vector<uint32_t> &first, const std::vector<uint32_t> &second) {
    constexpr uint32_t GROUPS = 3;  // the same input in three workgroups
    std::vector<uint32_t> in, want(2 * THREADS), got(GROUPS * 2 * THREADS);
    for (uint32_t g = 0; g < GROUPS; ++g) {
        in.insert(in.end(), first.begin(), first.end());
        in.insert(in.end(), second.begin(), second.end());
    }
    for (uint32_t half = 0; half < 2; ++half) {
        uint32_t run = 0;
        for (uint32_t t = 0; t < THREADS; ++t) want[half * THREADS + t] = run += in[half * THREADS + t];
    }
    uint32_t *d_in = nullptr, *d_out = nullptr;
    const size_t bytes = in.size() * 4;
    bool ok = hipMalloc((void **)&d_in, bytes) == hipSuccess && hipMalloc((void **)&d_out, bytes) == hipSuccess &&
              hipMemcpy(d_in, in.data(), bytes, hipMemcpyHostToDevice) == hipSuccess && hipMemset(d_out, 0xff, bytes) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(scan_twice<THREADS>, dim3(GROUPS), dim3(THREADS), 0, 0, d_in, d_out);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(got.data(), d_out, bytes, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    if (!ok) {
        printf("%s, %u lanes: HIP error\n", name, THREADS);
        return 1;
    }
    for (size_t i = 0; i < got.size(); ++i)
        if (got[i] != want[i % (2 * THREADS)]) {
            printf("%s, %u lanes: workgroup %zu, scan %zu, lane %zu = %u, host %u\n", name, THREADS, i / (2 * THREADS), i / THREADS % 2, i % THREADS, got[i],
                   want[i % (2 * THREADS)]);
            return 1;
        }
    printf("%s, %u lanes: ok (total %u, then %u)\n", name, THREADS, want[THREADS - 1], want[2 * THREADS - 1]);
    return 0;
}

template <uint32_t THREADS>
int run_all() {
    const std::vector<uint32_t> zeros(THREADS, 0), ones(THREADS, 1);
    std::vector<uint32_t> last(THREADS, 0), full(THREADS, 0xFFFFFFFFu / THREADS), rnd(THREADS), lanes(THREADS);
    last[THREADS - 1] = 0x80000001u;
    full[0] += 0xFFFFFFFFu % THREADS;  // the total is 2^32 - 1 exactly
    uint64_t z = 0x9E3779B97F4A7C15ull;
    for (uint32_t t = 0; t < THREADS; ++t) {
        z = z * 6364136223846793005ull + 1442695040888963407ull;
        rnd[t] = (uint32_t)(z >> 32);
        lanes[t] = t;
    }
    int bad = 0;
    bad |= run<THREADS>("all zeros, then all ones", zeros, ones);
    bad |= run<THREADS>("all ones, then all zeros", ones, zeros);
    bad |= run<THREADS>("one word in the last lane, then the lane numbers", last, lanes);
    bad |= run<THREADS>("a total of 2^32 - 1, then one word in the last lane", full, last);
    bad |= run<THREADS>("random words (sums wrap), then a total of 2^32 - 1", rnd, full);
    return bad;
}

int main() {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
        printf("no device\n");
        return 1;
    }
    return run_all<256>() | run_all<1024>();
}
