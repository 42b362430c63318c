// SHA2-256 over field elements: the hash core of the Merkle trees (merkle.hip), __host__ __device__ so the no-GPU suite runs the very
// same code on the CPU (hosttest.hip) against hashlib.
//
// Conventions (include/zkhip.h, "Merkle trees"): a field element is the 32-byte BIG-ENDIAN encoding of its canonical integer.  Elements lie
// in memory as canonical little-endian limbs, so the eight big-endian 32-bit words SHA reads of an element are its u32 limbs taken from the
// top down -- no byte swap on input.  Two elements fill one 64-byte compression block.  Digests are kept in memory in their EXTERNAL byte
// order (the 32 bytes a caller reads), i.e. every state word byte-swapped on store and on load.
#pragma once
#include <cstring>

#include "zk_defs.hpp"

namespace zkhip {
namespace sha256 {

struct RoundTable {
    uint32_t v[64];
};

static constexpr RoundTable K = {{
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
    0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
    0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
    0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
    0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
    0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u}};

// written so that the device compiler emits v_alignbit_b32 for the rotates and v_bfi_b32 for Ch / Maj
constexpr ZK_HD uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
constexpr ZK_HD uint32_t ch(uint32_t x, uint32_t y, uint32_t z) { return (x & y) | (~x & z); }
constexpr ZK_HD uint32_t maj(uint32_t x, uint32_t y, uint32_t z) { return ((x ^ y) & z) | (~(x ^ y) & y); }
constexpr ZK_HD uint32_t big0(uint32_t x) { return rotr(x, 2) ^ rotr(x, 13) ^ rotr(x, 22); }
constexpr ZK_HD uint32_t big1(uint32_t x) { return rotr(x, 6) ^ rotr(x, 11) ^ rotr(x, 25); }
constexpr ZK_HD uint32_t small0(uint32_t x) { return rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3); }
constexpr ZK_HD uint32_t small1(uint32_t x) { return rotr(x, 17) ^ rotr(x, 19) ^ (x >> 10); }

// K[i] + W[i] of the one block that pads a 64-byte message (0x80, zeros, bit length 512): what every inner node hashes second
constexpr RoundTable pad64_rounds() {
    uint32_t w[64] = {};
    w[0] = 0x80000000u;
    w[15] = 512;
    for (int i = 16; i < 64; ++i) w[i] = w[i - 16] + small0(w[i - 15]) + w[i - 7] + small1(w[i - 2]);
    RoundTable t = {};
    for (int i = 0; i < 64; ++i) t.v[i] = K.v[i] + w[i];
    return t;
}
static constexpr RoundTable PAD64 = pad64_rounds();

ZK_HD void init(uint32_t h[8]) {
    h[0] = 0x6a09e667u, h[1] = 0xbb67ae85u, h[2] = 0x3c6ef372u, h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu, h[5] = 0x9b05688cu, h[6] = 0x1f83d9abu, h[7] = 0x5be0cd19u;
}

#define ZK_SHA_ROUND(kw)                                        \
    {                                                           \
        const uint32_t t1 = hh + big1(e) + ch(e, f, g) + (kw);  \
        const uint32_t t2 = big0(a) + maj(a, b, c);             \
        hh = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2; \
    }

// one compression: h <- h + F(h, w); w is the block's sixteen big-endian words and is consumed (the rolling message schedule lives in it)
ZK_HD void compress(uint32_t h[8], uint32_t w[16]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    ZK_UNROLL
    for (int i = 0; i < 64; ++i) {
        if (i >= 16) w[i & 15] += small0(w[(i + 1) & 15]) + w[(i + 9) & 15] + small1(w[(i + 14) & 15]);
        ZK_SHA_ROUND(K.v[i] + w[i & 15])
    }
    h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
}

// the compression of the constant padding block of a 64-byte message: no schedule to run
ZK_HD void compress_pad64(uint32_t h[8]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    ZK_UNROLL
    for (int i = 0; i < 64; ++i) ZK_SHA_ROUND(PAD64.v[i])
    h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
}
#undef ZK_SHA_ROUND

// eight u32 from 32 bytes (16-byte aligned on the device: two 128-bit loads)
ZK_HD void load8(const void *p, uint32_t v[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 lo = static_cast<const uint4 *>(p)[0], hi = static_cast<const uint4 *>(p)[1];
    v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w, v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
#else
    memcpy(v, p, 32);
#endif
}
ZK_HD void store8(void *p, const uint32_t v[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_cast<uint4 *>(p)[0] = make_uint4(v[0], v[1], v[2], v[3]);
    static_cast<uint4 *>(p)[1] = make_uint4(v[4], v[5], v[6], v[7]);
#else
    memcpy(p, v, 32);
#endif
}

// the eight block words of the element at `elem` (canonical little-endian limbs): its u32 limbs from the top down
ZK_HD void element_words(const void *elem, uint32_t w[8]) {
    uint32_t v[8];
    load8(elem, v);
    ZK_UNROLL
    for (int k = 0; k < 8; ++k) w[k] = v[7 - k];
}

// the tail of the last block of a message of `bytes` bytes, from word `from` (0: a block of padding only, 8: behind one element)
ZK_HD void pad_words(uint32_t w[16], int from, uint64_t bytes) {
    w[from] = 0x80000000u;
    ZK_UNROLL
    for (int k = from + 1; k < 14; ++k) w[k] = 0;
    w[14] = (uint32_t)(bytes >> 29);
    w[15] = (uint32_t)(bytes << 3);
}

// state -> the digest's 32 bytes in memory, and back
ZK_HD void store_digest(void *out, const uint32_t h[8]) {
    uint32_t v[8];
    ZK_UNROLL
    for (int k = 0; k < 8; ++k) v[k] = __builtin_bswap32(h[k]);
    store8(out, v);
}
ZK_HD void digest_words(const void *digest, uint32_t w[8]) {
    load8(digest, w);
    ZK_UNROLL
    for (int k = 0; k < 8; ++k) w[k] = __builtin_bswap32(w[k]);
}

// SHA2-256 of n contiguous elements (n >= 1): n / 2 blocks of two elements, then the padding block -- alone when n is even (bytes = 0 mod
// 64), behind the last element when n is odd (bytes = 32 mod 64)
ZK_HD void hash_elements(const void *elems, size_t n, void *digest) {
    const char *e = static_cast<const char *>(elems);
    uint32_t h[8], w[16];
    init(h);
    size_t i = 0;
    for (; i + 2 <= n; i += 2) {
        element_words(e + 32 * i, w);
        element_words(e + 32 * i + 32, w + 8);
        compress(h, w);
    }
    if (i < n) {
        element_words(e + 32 * i, w);
        pad_words(w, 8, (uint64_t)n * 32);
    } else {
        pad_words(w, 0, (uint64_t)n * 32);
    }
    compress(h, w);
    store_digest(digest, h);
}

// inner node: SHA2-256(left digest || right digest)
ZK_HD void hash_node(const void *left, const void *right, void *digest) {
    uint32_t h[8], w[16];
    init(h);
    digest_words(left, w);
    digest_words(right, w + 8);
    compress(h, w);
    compress_pad64(h);
    store_digest(digest, h);
}

}  // namespace sha256
}  // namespace zkhip
