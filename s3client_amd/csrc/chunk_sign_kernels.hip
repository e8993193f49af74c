// chunk_sign_kernels.hip -- the SigV4 chunk-signature chain (aws-chunked uploads signed with
// STREAMING-AWS4-HMAC-SHA256-PAYLOAD) for MI355X (gfx950).
//
// An upload part is cut into chunks that are hashed independently (an ordinary SHA-256 plan whose
// parts are the chunks); what links them is one HMAC per chunk over a short string:
//   sig_i = HMAC-SHA256(signing_key, P || hex(sig_{i-1}) '\n' hex(sha256("")) '\n' hex(sha256(chunk_i)))
// with P constant.  The chain of one part is serial, the chains of different parts are
// independent: one lane per part, one wave per workgroup, so the waves of a batch spread over
// CUs and each has a SIMD to itself (the chain is latency-bound: a lone wave issues one VALU
// every ~4 cycles whatever its neighbours do).
//
// Per link a lane compresses the inner tail -- P's last r bytes, the 194 variable bytes, the
// padding: 4 blocks for r <= 53, 5 above -- from the context's inner midstate, then one outer
// block from the outer midstate.  The tail lives in LDS as a column [word][lane] (consecutive
// lanes on consecutive banks): the kernel's arguments carry it as big-endian words with the two
// variable hex fields zeroed, each lane copies it once and per link rewrites the 17 words each
// field touches.  r is uniform over the launch, so the fields' word offsets and byte shifts are
// scalars.  Rounds and schedule are sha256_device.hpp's.
//
// The kernel lives in a text section of its own, so the machine code of the kernels pinned in
// s3client_amd/kernel_isa_counts.json stays as it is.
#pragma once
#include "sha256_device.hpp"

namespace s3h {

#define S3H_CHUNK_TEXT __attribute__((section(".text.s3h_chunk_sign")))

// Lowercase hex of the 4 nibbles of x[15:0] as a big-endian word of 4 characters: the nibbles
// spread to bytes, then '0' + v, plus 39 ('a' - '0' - 10) where v >= 10 (bit 4 of v + 6).
__device__ __forceinline__ uint32_t hex4(uint32_t x) {
  const uint32_t v = ((x << 12) & 0x0F000000u) | ((x << 8) & 0x000F0000u) | ((x << 4) & 0x00000F00u) |
                     (x & 0x0000000Fu);
  return v + 0x30303030u + (((v + 0x06060606u) >> 4) & 0x01010101u) * 39u;
}

// Writes the 64 hex characters of h[0..7] (native words) at byte offset 4 * word + shift of the
// lane's column.  The 17 words the field touches are rewritten whole: `lo` and `hi` are the
// template's first and last of them (P's bytes or a '\n' around the field), the 15 between hold
// field bytes only.
__device__ __forceinline__ void put_hex_field(uint32_t (*col)[kChunkChainThreads], uint32_t lane,
                                              uint32_t word, uint32_t shift, uint32_t lo, uint32_t hi,
                                              const uint32_t h[8]) {
  uint32_t x[18];
  x[0] = 0;
  x[17] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    x[2 * i + 1] = hex4(h[i] >> 16);
    x[2 * i + 2] = hex4(h[i]);
  }
  const uint32_t bits = 8 * shift;  // alignbit(hi, lo, 0) == lo: an aligned field is copied
#pragma unroll
  for (int k = 0; k < 17; ++k) {
    uint32_t v = __builtin_amdgcn_alignbit(x[k], x[k + 1], bits);
    if (k == 0) v |= lo;
    if (k == 16) v |= hi;
    col[word + k][lane] = v;
  }
}

// One compression of w into st.
__device__ __forceinline__ void chunk_compress(uint32_t st[8], const uint32_t w[16]) {
  uint32_t wk[64], t[8];
  schedule_wk(w, wk);
#pragma unroll
  for (int i = 0; i < 8; ++i) t[i] = st[i];
  rounds_wk(t, wk);
#pragma unroll
  for (int i = 0; i < 8; ++i) st[i] += t[i];
}

S3H_CHUNK_TEXT __global__ __launch_bounds__(kChunkChainThreads) void sigv4_chunk_chain_kernel(ChunkChainArgs A) {
  __shared__ uint32_t col[kChunkTailWords][kChunkChainThreads];  // 20 KiB

  const uint32_t lane = threadIdx.x;
  const uint64_t part = uint64_t(blockIdx.x) * kChunkChainThreads + lane;
  if (part >= A.n) return;  // (no barrier below: a lane touches its own column only)
  const ChunkChainPart pt = A.parts[part];

#pragma unroll
  for (int j = 0; j < kChunkTailWords; ++j) col[j][lane] = A.tail[j];
  // the two hex fields: bytes [r, r + 64) and [r + 130, r + 194) of the tail
  const uint32_t word0 = A.r >> 2, shift0 = A.r & 3u;
  const uint32_t word1 = (A.r + 130u) >> 2, shift1 = (A.r + 130u) & 3u;
  const uint32_t lo0 = col[word0][lane], hi0 = col[word0 + 16][lane];
  const uint32_t lo1 = col[word1][lane], hi1 = col[word1 + 16][lane];

  uint32_t prev[8];
  {
    const uint4* s = reinterpret_cast<const uint4*>(A.seeds + 8 * part);
    const uint4 a = s[0], b = s[1];
    prev[0] = bswap(a.x); prev[1] = bswap(a.y); prev[2] = bswap(a.z); prev[3] = bswap(a.w);
    prev[4] = bswap(b.x); prev[5] = bswap(b.y); prev[6] = bswap(b.z); prev[7] = bswap(b.w);
  }
  const uint4* dig = reinterpret_cast<const uint4*>(A.digests + 8 * pt.first);
  uint4* out = reinterpret_cast<uint4*>(A.signatures + 8 * pt.sig);

#pragma unroll 1
  for (uint32_t c = 0; c <= pt.count; ++c) {
    // this link's chunk digest; the final link signs the empty chunk, sha256("")
    uint32_t d[8] = {0xe3b0c442u, 0x98fc1c14u, 0x9afbf4c8u, 0x996fb924u,
                     0x27ae41e4u, 0x649b934cu, 0xa495991bu, 0x7852b855u};
    if (c < pt.count) {
      const uint4 a = dig[2 * uint64_t(c)], b = dig[2 * uint64_t(c) + 1];
      d[0] = bswap(a.x); d[1] = bswap(a.y); d[2] = bswap(a.z); d[3] = bswap(a.w);
      d[4] = bswap(b.x); d[5] = bswap(b.y); d[6] = bswap(b.z); d[7] = bswap(b.w);
    }
    put_hex_field(col, lane, word0, shift0, lo0, hi0, prev);
    put_hex_field(col, lane, word1, shift1, lo1, hi1, d);

    uint32_t st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = A.istate[i];
#pragma unroll 1
    for (uint32_t b = 0; b < A.nblk; ++b) {
      uint32_t w[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) w[j] = col[16 * b + j][lane];
      chunk_compress(st, w);
    }
    // outer hash: opad midstate, then the inner digest, 0x80, zeros, (64 + 32) * 8 bits
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = st[i];
    w[8] = 0x80000000u;
#pragma unroll
    for (int i = 9; i < 15; ++i) w[i] = 0;
    w[15] = 768;
#pragma unroll
    for (int i = 0; i < 8; ++i) prev[i] = A.ostate[i];
    chunk_compress(prev, w);

    out[2 * uint64_t(c)] = make_uint4(bswap(prev[0]), bswap(prev[1]), bswap(prev[2]), bswap(prev[3]));
    out[2 * uint64_t(c) + 1] = make_uint4(bswap(prev[4]), bswap(prev[5]), bswap(prev[6]), bswap(prev[7]));
  }
}

}  // namespace s3h
