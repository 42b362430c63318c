//---------------------------------------------------------------------------//
// zkhip shim: FRI's proof of work (grinding), searched on the MI355X.
//
// Stands where commitments::proof_of_work<hashes::sha2<256>, std::uint32_t> stands (zk/commitments/detail/polynomial/proof_of_work.hpp:41-80),
// with the reference's two members.  generate() hands the transcript's state to zkhip_pow_grind, which returns the FIRST nonce the
// reference's loop would accept from the same starting value, and then does to the transcript what the reference does (:65-67): absorb the
// nonce's four big-endian bytes, draw the int_challenge.  verify() is host only (two hashes).
//
// `TranscriptType` is the SHA2-256 sequential transcript: hip/transcript.hpp's sha256_transcript, or any type with its state() (32 bytes),
// operator()(byte range) and int_challenge<std::uint32_t>() and its byte conventions (include/zkhip.h, "Proof of work").  generate() holds
// the transcript against the device's answer: a transcript that hashes differently is reported, not silently ground for.
//
// This header and hip/transcript.hpp are the only ones of the shim that refer to zkhip_pow_grind / zkhip_sha256_host: code that never
// asks for grinding over a transcript with state() does not need them at link time.
//---------------------------------------------------------------------------//
#ifndef ZKHIP_SHIM_PROOF_OF_WORK_HPP
#define ZKHIP_SHIM_PROOF_OF_WORK_HPP

#include <array>
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <type_traits>

#include "backend.hpp"

namespace nil {
namespace crypto3 {
namespace zk {
namespace hip {

template <typename TranscriptType, typename OutType = std::uint32_t>
class proof_of_work_hip {
    static_assert(std::is_same<OutType, std::uint32_t>::value, "proof_of_work_hip: the device search is built for 32-bit nonces");

public:
    typedef TranscriptType transcript_type;
    typedef OutType output_type;

    /// proof_of_work.hpp:47-68.  `start`: the first nonce tried (the reference draws it with std::rand() inside)
    static OutType generate(const context &ctx, transcript_type &transcript, OutType mask = 0xFFFF, OutType start = (OutType)std::rand()) {
        const auto &state = transcript.state();
        if (state.size() != 32) throw std::invalid_argument("proof_of_work_hip: the transcript's state is not a 32-byte digest");
        OutType proof_of_work = 0;
        /* nothing found in the whole 2^32 space (where the reference loops forever): ZKHIP_ERR_NOT_FOUND, thrown by check */
        ZKHIP_CALL(ctx, zkhip_pow_grind, ZKHIP_HASH_SHA2_256, state.data(), start, mask, 0, 0, &proof_of_work, nullptr);
        if (!verify(transcript, proof_of_work, mask))
            throw std::logic_error("proof_of_work_hip: the transcript rejects the device's nonce (it is not the SHA2-256 sequential transcript)");
        return proof_of_work;
    }

    /// proof_of_work.hpp:70-79
    static bool verify(transcript_type &transcript, OutType proof_of_work, OutType mask = 0xFFFF) {
        const std::array<std::uint8_t, 4> bytes = {std::uint8_t(proof_of_work >> 24), std::uint8_t(proof_of_work >> 16), std::uint8_t(proof_of_work >> 8),
                                                   std::uint8_t(proof_of_work)};
        transcript(bytes);
        const OutType result = transcript.template int_challenge<OutType>();
        return (result & mask) == 0;
    }
};

}    // namespace hip
}    // namespace zk
}    // namespace crypto3
}    // namespace nil

#endif    // ZKHIP_SHIM_PROOF_OF_WORK_HPP
