// FRI's proof of work (grinding) over the SHA2-256 sequential transcript: proof_of_work<sha2<256>, std::uint32_t>
// (zk/commitments/detail/polynomial/proof_of_work.hpp:47-79) over fiat_shamir_heuristic_sequential (zk/transcript/fiat_shamir.hpp:134-199).
// __host__ __device__ on top of sha256.hpp, so the kernel of pow.hip and the no-GPU suite (hosttest.hip, against hashlib) run the same code.
//
// Conventions (include/zkhip.h, "Proof of work").  A candidate nonce n is tried by absorbing its four BIG-ENDIAN bytes into a copy of the
// transcript and drawing int_challenge<uint32_t>:
//     candidate(state, n) = the low 32 bits of the big-endian integer of SHA256( SHA256( state || be32(n) ) )
// i.e. bytes 28..31 of the second digest read big-endian = state word h[7] of the second hash; n is accepted when (candidate & mask) == 0.
// Both messages are one block:
//     first   36 bytes: words 0..7 the state (its bytes read as big-endian words), word 8 = n (a big-endian word of be32(n) is n: no byte
//             swap), word 9 = 0x80000000, words 10..14 = 0, word 15 = 288;
//     second  32 bytes: words 0..7 the first digest's state words, word 8 = 0x80000000, words 9..14 = 0, word 15 = 256.
#pragma once
#include "sha256.hpp"

namespace zkhip {
namespace pow {

// What a search computes once, on the host: everything of the first block that does not depend on the nonce.  The nonce is block word 8, so
// rounds 0..7 read none of it, and neither do schedule words 16..22 (word 16 + j reads words j, j + 1, j + 9 and j + 14).
struct Search {
    uint32_t st[8];     // the transcript state as block words 0..7
    uint32_t mid[8];    // a..h after rounds 0..7 of the first block
    uint32_t sched[7];  // schedule words 16..22 of the first block
};

#define ZK_POW_ROUND(kw)                                                          \
    {                                                                             \
        const uint32_t t1 = hh + sha256::big1(e) + sha256::ch(e, f, g) + (kw);    \
        const uint32_t t2 = sha256::big0(a) + sha256::maj(a, b, c);               \
        hh = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;       \
    }

// the first block's words behind the state
ZK_HD void first_block_tail(uint32_t w[16], uint32_t n) {
    w[8] = n;
    sha256::pad_words(w, 9, 36);
}

ZK_HD Search prepare(const uint8_t state[32]) {
    Search s;
    for (int k = 0; k < 8; ++k)
        s.st[k] = (uint32_t)state[4 * k] << 24 | (uint32_t)state[4 * k + 1] << 16 | (uint32_t)state[4 * k + 2] << 8 | (uint32_t)state[4 * k + 3];
    uint32_t iv[8], w[23] = {};
    sha256::init(iv);
    uint32_t a = iv[0], b = iv[1], c = iv[2], d = iv[3], e = iv[4], f = iv[5], g = iv[6], hh = iv[7];
    for (int i = 0; i < 8; ++i) {
        w[i] = s.st[i];
        ZK_POW_ROUND(sha256::K.v[i] + w[i])
    }
    s.mid[0] = a, s.mid[1] = b, s.mid[2] = c, s.mid[3] = d, s.mid[4] = e, s.mid[5] = f, s.mid[6] = g, s.mid[7] = hh;
    uint32_t tail[16];
    first_block_tail(tail, 0);  // word 8 (the nonce) is not read below
    for (int i = 9; i < 16; ++i) w[i] = tail[i];
    for (int i = 16; i < 23; ++i) s.sched[i - 16] = w[i] = w[i - 16] + sha256::small0(w[i - 15]) + w[i - 7] + sha256::small1(w[i - 2]);
    return s;
}

// candidate(state, n).  Hoisted: the first block starts at round 8 from Search::mid and takes schedule words 16..22 from Search::sched; the
// template exists so that tools/powbench.hip can time the plain form against it (EXPERIMENTS.md).  The second block is an ordinary
// compression of which only h[7] is read: the compiler drops rounds 61..63 and everything else that word does not depend on by itself, and
// folds the constant block words of both messages into the round constants.
template <bool Hoisted>
ZK_HD uint32_t candidate_as(const Search &s, uint32_t n) {
    uint32_t iv[8], w[16];
    sha256::init(iv);
    ZK_UNROLL
    for (int k = 0; k < 8; ++k) w[k] = s.st[k];
    first_block_tail(w, n);
    uint32_t a, b, c, d, e, f, g, hh;
    if (Hoisted) a = s.mid[0], b = s.mid[1], c = s.mid[2], d = s.mid[3], e = s.mid[4], f = s.mid[5], g = s.mid[6], hh = s.mid[7];
    else a = iv[0], b = iv[1], c = iv[2], d = iv[3], e = iv[4], f = iv[5], g = iv[6], hh = iv[7];
    ZK_UNROLL
    for (int i = Hoisted ? 8 : 0; i < 64; ++i) {
        if (i >= 16) {
            if (Hoisted && i < 23) w[i & 15] = s.sched[i - 16];
            else w[i & 15] += sha256::small0(w[(i + 1) & 15]) + w[(i + 9) & 15] + sha256::small1(w[(i + 14) & 15]);
        }
        ZK_POW_ROUND(sha256::K.v[i] + w[i & 15])
    }
    // the second block: the first digest (never stored: its state words are the block words) and constant padding
    w[0] = iv[0] + a, w[1] = iv[1] + b, w[2] = iv[2] + c, w[3] = iv[3] + d, w[4] = iv[4] + e, w[5] = iv[5] + f, w[6] = iv[6] + g, w[7] = iv[7] + hh;
    sha256::pad_words(w, 8, 32);
    sha256::compress(iv, w);
    return iv[7];
}
#undef ZK_POW_ROUND

ZK_HD uint32_t candidate(const Search &s, uint32_t n) { return candidate_as<true>(s, n); }

// the reference's loop (proof_of_work.hpp:52-64) over at most max_tries <= 2^32 nonces start, start + 1, ... (mod 2^32): the offset of the
// first accepted one, or max_tries when there is none
ZK_HD uint64_t first_hit(const Search &s, uint32_t start, uint32_t mask, uint64_t max_tries) {
    for (uint64_t k = 0; k < max_tries; ++k)
        if ((candidate(s, start + (uint32_t)k) & mask) == 0) return k;
    return max_tries;
}

// SHA2-256 of a byte string (the transcript's own hashing in the shim: zkhip_sha256_host)
ZK_HD void hash_bytes(const uint8_t *msg, size_t len, uint8_t out[32]) {
    uint32_t h[8], w[16];
    sha256::init(h);
    uint8_t block[64];
    size_t at = 0;
    bool padded = false, done = false;  // the 0x80 byte is out; the length is out
    while (!done) {
        const size_t take = len - at < 64 ? len - at : 64;
        for (size_t k = 0; k < take; ++k) block[k] = msg[at + k];
        at += take;
        size_t fill = take;
        if (fill < 64 && !padded) block[fill++] = 0x80, padded = true;
        for (size_t k = fill; k < 64; ++k) block[k] = 0;
        if (padded && fill <= 56) {
            const uint64_t bits = (uint64_t)len << 3;
            for (int k = 0; k < 8; ++k) block[56 + k] = (uint8_t)(bits >> (56 - 8 * k));
            done = true;
        }
        for (int k = 0; k < 16; ++k)
            w[k] = (uint32_t)block[4 * k] << 24 | (uint32_t)block[4 * k + 1] << 16 | (uint32_t)block[4 * k + 2] << 8 | (uint32_t)block[4 * k + 3];
        sha256::compress(h, w);
    }
    for (int k = 0; k < 8; ++k)
        for (int j = 0; j < 4; ++j) out[4 * k + j] = (uint8_t)(h[k] >> (24 - 8 * j));
}

}  // namespace pow
}  // namespace zkhip
