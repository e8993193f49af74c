// chunk_sign.hpp -- the SigV4 chunk-signing context shared by the CPU chain (cpu/lib_chunk_sign.cpp,
// which creates it) and the device launch (chunk_sign.cpp, which copies its midstates and tail
// templates into the kernels' argument blocks).  HIP-free.
//
// Every chunk's string to sign is  P || hex(prev) '\n' hex(sha256("")) '\n' hex(sha256(chunk)),
// P the constant prefix.  HMAC's inner hash runs over  ipad-block || P || 194 bytes: the context
// holds the state after the ipad block and P's whole 64-byte blocks, and a template of what is
// left -- P's last r bytes, the 194 bytes with the two variable hex fields zeroed, 0x80, zeros
// and the bit length -- as bytes (CPU chain) and as big-endian words (chain kernel).
//
// The trailer signature (...-PAYLOAD-TRAILER) signs  P' || hex(sig_last) '\n' hex(sha256(line)),
// P' being P under the name AWS4-HMAC-SHA256-TRAILER: as long as P, so r is shared, but wherever
// |P| >= 64 the name sits in a block hashed once -- a second inner midstate and a second tail
// template (P's last r bytes, 129 bytes with both hex fields zeroed, padding).
#pragma once
#include <stdint.h>

#include "kernel_abi.hpp"

struct s3h_chunk_sign_ctx_s {
  uint32_t istate[8];               // native words: after ipad-block || P[0 : 64 * floor(|P| / 64))
  uint32_t ostate[8];               // after the opad block
  uint32_t prefix_len;              // |P|
  uint32_t r;                       // |P| mod 64
  uint32_t nblk;                    // compressions of the inner tail: ceil((r + 203) / 64), 4 or 5
  uint8_t tail[s3h::kChunkTailWords * 4];   // nblk * 64 bytes used
  uint32_t tail_words[s3h::kChunkTailWords]; // the same as big-endian words
  char prefix[256];
  // the trailer signature's
  uint32_t trailer_istate[8];       // after ipad-block || P'[0 : 64 * floor(|P| / 64))
  uint32_t trailer_nblk;            // ceil((r + 138) / 64), 3 or 4
  uint8_t trailer_tail[s3h::kTrailerTailWords * 4];
  uint32_t trailer_tail_words[s3h::kTrailerTailWords];
};

namespace s3h {

// The trailing header line of a checksum kind (enum s3h_trailer_checksum): `name ":"`, then
// `text_len` base64 characters of the value's `value_len` big-endian bytes, then "\n".
struct TrailerKind {
  const char* name;
  uint32_t value_len;
  uint32_t text_len;
};
// Null for an unknown kind.
const TrailerKind* trailer_kind(int checksum);

}  // namespace s3h
