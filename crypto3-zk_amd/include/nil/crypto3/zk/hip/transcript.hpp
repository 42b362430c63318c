//---------------------------------------------------------------------------//
// zkhip shim: the SHA2-256 sequential Fiat-Shamir transcript, restated for the scheme classes of this shim.
//
// Stands where transcript::fiat_shamir_heuristic_sequential<hashes::sha2<256>> stands (zk/transcript/fiat_shamir.hpp:134-199): the state is
// one digest; absorbing makes it H(state || bytes), a challenge makes it H(state) and reads the state as a big-endian integer.  It is the
// transcript the device's proof-of-work search is defined over (hip/proof_of_work.hpp; include/zkhip.h, "Proof of work"), and -- unlike the
// duck-typed transcripts the scheme classes otherwise take -- exposes its state(), which is what that search starts from.
//
// All hashing goes through zkhip_sha256_host (the library's own SHA2-256 core on the host): the shim carries no second implementation.
// The byte conventions are checked against an independent SHA2-256, not pinned to a crypto3 vector (crypto3-hash and crypto3-marshalling
// were not at hand): a digest is absorbed as its 32 bytes, a challenge is the state's big-endian integer reduced mod r.
//---------------------------------------------------------------------------//
#ifndef ZKHIP_SHIM_TRANSCRIPT_HPP
#define ZKHIP_SHIM_TRANSCRIPT_HPP

#include <array>
#include <cstdint>
#include <iterator>
#include <vector>

#include "backend.hpp"

namespace nil {
namespace crypto3 {
namespace zk {
namespace hip {

template <typename CurveType>
class sha256_transcript {
public:
    typedef curve_adapter<CurveType> adapter;
    typedef typename adapter::scalar_value_type value_type;
    typedef std::array<std::uint8_t, 32> digest_type;

    /// fiat_shamir.hpp:139: hash({0}), one zero byte
    sha256_transcript() {
        const std::uint8_t zero = 0;
        hash(&zero, 1);
    }
    /// fiat_shamir.hpp:142-144: the hash of a byte range
    template <typename InputRange, typename = decltype(std::begin(std::declval<const InputRange &>()))>
    explicit sha256_transcript(const InputRange &r) {
        const std::vector<std::uint8_t> bytes(std::begin(r), std::end(r));
        hash(bytes.data(), bytes.size());
    }
    /// absorb a byte range -- a Merkle root (device_merkle_tree::digest_type), marshalled bytes: state = H(state || bytes)
    template <typename InputRange>
    void operator()(const InputRange &r) {
        (*this)(std::begin(r), std::end(r));
    }
    template <typename InputIterator>
    void operator()(InputIterator first, InputIterator last) {
        std::vector<std::uint8_t> bytes(state_.begin(), state_.end());
        bytes.insert(bytes.end(), first, last);
        hash(bytes.data(), bytes.size());
    }
    /// challenge<Field>() (fiat_shamir.hpp:168-188): state = H(state), read as a big-endian integer, as a scalar (reduced mod r)
    value_type challenge() {
        hash(state_.data(), state_.size());
        /* the integer is hi 2^128 + lo with both halves below 2^128 < r: canonical values the adapter takes as limbs */
        std::uint64_t word[4];    // little-endian u64 limbs of the big-endian bytes
        for (int k = 0; k < 4; ++k) {
            word[k] = 0;
            for (int j = 0; j < 8; ++j) word[k] = word[k] << 8 | state_[8 * (3 - k) + j];
        }
        const std::uint64_t lo[4] = {word[0], word[1], 0, 0}, hi[4] = {word[2], word[3], 0, 0}, two128[4] = {0, 0, 1, 0};
        return adapter::scalar_from_limbs(lo) + adapter::scalar_from_limbs(hi) * adapter::scalar_from_limbs(two128);
    }
    /// int_challenge<Integral>() (fiat_shamir.hpp:190-199): state = H(state), the low bits of its big-endian integer
    template <typename Integral>
    Integral int_challenge() {
        static_assert(sizeof(Integral) <= 8, "int_challenge: at most 64 bits");
        hash(state_.data(), state_.size());
        std::uint64_t v = 0;
        for (std::size_t j = 32 - sizeof(Integral); j < 32; ++j) v = v << 8 | state_[j];
        return static_cast<Integral>(v);
    }
    const digest_type &state() const { return state_; }

private:
    void hash(const std::uint8_t *msg, std::size_t len) {
        digest_type out;
        check(zkhip_sha256_host(msg, len, out.data()), "zkhip_sha256_host");
        state_ = out;
    }
    digest_type state_ {};
};

}    // namespace hip
}    // namespace zk
}    // namespace crypto3
}    // namespace nil

#endif    // ZKHIP_SHIM_TRANSCRIPT_HPP
