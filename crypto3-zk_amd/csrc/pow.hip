// FRI's proof of work (grinding) on the device: proof_of_work<sha2<256>, std::uint32_t>::generate's search
// (zk/commitments/detail/polynomial/proof_of_work.hpp:47-68) over a SHA2-256 sequential transcript's state.
//
//   zkhip_pow_grind     the first nonce in the reference's search order start, start + 1, ... (mod 2^32) that the mask accepts
//   zkhip_sha256_host   SHA2-256 of a byte string on the host, over the same core (the shim's transcript hashes with it)
//
// Conventions: include/zkhip.h ("Proof of work") and pow.hpp.  The search is cut into chunks of 2^chunk_log consecutive offsets, one launch
// each; every lane tries POW_PER_LANE offsets of its chunk and folds a hit into one device word with atomicMin on the OFFSET, so the word
// holds the chunk's first hit whichever lane got there first.  The host reads the word after each chunk and stops at the first chunk that
// holds a hit: the answer is the reference's, never a lucky lane's.  Every launch is bounded by its chunk; no lane waits on another.
#include "ctx.hpp"
#include "pow.hpp"

using namespace zkhip;

static constexpr unsigned POW_PER_LANE = 16;       // offsets a lane tries (at a stride of the grid): the launch's fixed cost over more work
static constexpr size_t POW_DEFAULT_CHUNK_LOG = 20;  // DESIGN.md ("Proof of work"): the best 16-to-20-bit latency of tools/bench_pow.py
static constexpr unsigned long long POW_NO_HIT = ~0ull;

// offsets [base, base + count) of the search; nonce of offset k = first + (k - base) (mod 2^32), first = start + base
__global__ __launch_bounds__(256) void pow_grind_chunk(pow::Search s, uint32_t first, uint64_t base, uint64_t count, uint32_t mask,
                                                       unsigned long long *__restrict__ hit) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        if ((pow::candidate(s, first + (uint32_t)i) & mask) != 0) continue;
        // a lane's later offsets are larger: its first hit is its only contribution.  The plain read spares the atomic when a smaller
        // offset is already in (mask 0: every lane hits); a stale read only costs the atomic it would have spared.
        if (base + i < *(volatile unsigned long long *)hit) atomicMin(hit, (unsigned long long)(base + i));
        return;
    }
}

extern "C" {

int zkhip_pow_grind(zkhip_ctx *ctx, int hash, const uint8_t state[32], uint32_t start, uint32_t mask, uint64_t max_tries, size_t chunk_log, uint32_t *nonce,
                    uint64_t *tried) {
    if (!ctx || !state || !nonce || hash != ZKHIP_HASH_SHA2_256) return ZKHIP_ERR_INVALID;
    if (chunk_log == 0) chunk_log = POW_DEFAULT_CHUNK_LOG;
    const uint64_t space = (uint64_t)1 << 32;
    if (chunk_log < 8 || chunk_log > 32 || max_tries > space) return ZKHIP_ERR_RANGE;
    const uint64_t total = max_tries ? max_tries : space, chunk = (uint64_t)1 << chunk_log;
    ZK_ENTER(ctx);
    WsOne<unsigned long long> word = {1};
    ZK_TRY(ws_place(ctx, word));
    ZK_HIP_CHECK(ctx, hipMemsetAsync(word.p, 0xFF, sizeof(unsigned long long), ctx->stream));  // POW_NO_HIT
    const pow::Search s = pow::prepare(state);
    for (uint64_t base = 0; base < total; base += chunk) {
        const uint64_t count = total - base < chunk ? total - base : chunk;
        const uint64_t per_block = 256 * (uint64_t)POW_PER_LANE;
        ZK_LAUNCH(ctx, "pow_grind_chunk", pow_grind_chunk, dim3((unsigned)((count + per_block - 1) / per_block)), dim3(256), 0, s, start + (uint32_t)base, base,
                  count, mask, word.p);
        unsigned long long k = POW_NO_HIT;
        ZK_HIP_CHECK(ctx, hipMemcpyAsync(&k, word.p, sizeof k, hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (k != POW_NO_HIT) {
            *nonce = start + (uint32_t)k;
            if (tried) *tried = k + 1;
            return ZKHIP_OK;
        }
    }
    if (tried) *tried = total;
    return ZKHIP_ERR_NOT_FOUND;
}

int zkhip_sha256_host(const uint8_t *msg, size_t len, uint8_t out[32]) {
    if (!out || (!msg && len)) return ZKHIP_ERR_INVALID;
    pow::hash_bytes(msg, len, out);
    return ZKHIP_OK;
}

}  // extern "C"
