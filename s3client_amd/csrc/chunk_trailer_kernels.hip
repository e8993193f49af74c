// chunk_trailer_kernels.hip -- the trailer signature of a chunk-signed upload that carries a
// trailing checksum header (STREAMING-AWS4-HMAC-SHA256-PAYLOAD-TRAILER) for MI355X (gfx950).
//
// After the chain's last signature sig_last (the final 0-byte chunk's) a part is closed by
//   line        = name ":" base64(crc) "\n"                  e.g. "x-amz-checksum-crc32c:sOO8/Q==\n"
//   trailer_sig = HMAC-SHA256(signing_key, P' || hex(sig_last) '\n' hex(sha256(line)))
// with P' the chain's prefix under the name AWS4-HMAC-SHA256-TRAILER: the same length, so the
// same remainder r, but a midstate and a tail template of its own.  One link per part, the parts
// independent: one lane per part, one wave per workgroup, as the chain kernel.
//
// Per lane: the CRC to base64 on packed bytes, the text into the line's one block (a column
// [word][lane] in LDS, the template from the kernel's arguments, the value's byte offset uniform
// over the launch), one compression from the IV; then the two hex fields into the trailer tail
// (the same LDS column, put_hex_field of the chain kernel), 3 or 4 compressions from the trailer
// midstate and the outer block.  The second field starts 65 bytes behind the first, so its first
// word may be the first field's last: it is read back after the first field is in place.
//
// The kernel lives in a text section of its own, so the machine code of the kernels pinned in
// s3client_amd/kernel_isa_counts.json stays as it is.
#pragma once
#include "chunk_sign_kernels.hip"

namespace s3h {

#define S3H_TRAILER_TEXT __attribute__((section(".text.s3h_chunk_trailer")))

// The 4 sextets of x[23:0] as the bytes of a big-endian word, first sextet first.
__device__ __forceinline__ uint32_t sextets4(uint32_t x) {
  return ((x << 6) & 0x3F000000u) | ((x << 4) & 0x003F0000u) | ((x << 2) & 0x00003F00u) | (x & 0x0000003Fu);
}

// Base64 characters of 4 sextets (one per byte): 'A' + v, plus 6 from 26 ('a' - 'Z' - 1), minus
// 75 from 52 ('0' - 'z' - 1), minus 15 from 62 ('+' - '9' - 1), plus 3 at 63 ('/' - '+' - 1).
// v + (64 - k) carries into bit 6 of its byte where v >= k; a byte's sum stays within the byte.
__device__ __forceinline__ uint32_t base64_4(uint32_t v) {
  const uint32_t ge26 = ((v + 0x26262626u) >> 6) & 0x01010101u;
  const uint32_t ge52 = ((v + 0x0C0C0C0Cu) >> 6) & 0x01010101u;
  const uint32_t ge62 = ((v + 0x02020202u) >> 6) & 0x01010101u;
  const uint32_t ge63 = ((v + 0x01010101u) >> 6) & 0x01010101u;
  return v + 0x41414141u + ge26 * 6u - ge52 * 75u - ge62 * 15u + ge63 * 3u;
}

S3H_TRAILER_TEXT __global__ __launch_bounds__(kChunkChainThreads) void sigv4_trailer_kernel(ChunkTrailerArgs A) {
  __shared__ uint32_t col[kTrailerTailWords][kChunkChainThreads];  // 16 KiB

  const uint32_t lane = threadIdx.x;
  const uint64_t part = uint64_t(blockIdx.x) * kChunkChainThreads + lane;
  if (part >= A.n) return;  // (no barrier below: a lane touches its own column only)
  const ChunkChainPart pt = A.parts[part];

  // the value's big-endian bytes, 32-bit values in the upper half: 24 bits give 4 characters
  uint32_t hi, lo = 0;
  if (A.wide) {
    const uint64_t v = static_cast<const uint64_t*>(A.checksums)[part];
    hi = uint32_t(v >> 32);
    lo = uint32_t(v);
  } else {
    hi = static_cast<const uint32_t*>(A.checksums)[part];
  }
  uint32_t x[5];
  x[0] = 0;
  x[1] = base64_4(sextets4(hi >> 8));
  x[2] = base64_4(sextets4(((hi & 0xFFu) << 16) | (lo >> 16)));
  x[3] = base64_4(sextets4((lo & 0xFFFFu) << 8));
  x[4] = 0;
  // padding: 4 bytes end in "==" (6 characters of text), 8 bytes in "=" (11)
  if (A.wide) {
    x[3] = (x[3] & 0xFFFFFF00u) | 0x3Du;
  } else {
    x[2] = (x[2] & 0xFFFF0000u) | 0x3D3Du;
    x[3] = 0;
  }

  // the header line: its text at byte value_at of the one-block template
#pragma unroll
  for (int j = 0; j < 16; ++j) col[j][lane] = A.line[j];
  {
    const uint32_t word = A.value_at >> 2, bits = 8 * (A.value_at & 3u);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      col[word + k][lane] |= __builtin_amdgcn_alignbit(x[k], x[k + 1], bits);
  }
  uint32_t d[8];
  init_state(d);
  {
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = col[j][lane];
    chunk_compress(d, w);
  }

  uint32_t prev[8];
  {
    const uint4* s = reinterpret_cast<const uint4*>(A.signatures + 8 * (pt.sig + pt.count));
    const uint4 a = s[0], b = s[1];
    prev[0] = bswap(a.x); prev[1] = bswap(a.y); prev[2] = bswap(a.z); prev[3] = bswap(a.w);
    prev[4] = bswap(b.x); prev[5] = bswap(b.y); prev[6] = bswap(b.z); prev[7] = bswap(b.w);
  }

  // the trailer tail: hex fields at bytes [r, r + 64) and [r + 65, r + 129)
#pragma unroll
  for (int j = 0; j < kTrailerTailWords; ++j) col[j][lane] = A.tail[j];
  const uint32_t word0 = A.r >> 2, shift0 = A.r & 3u;
  const uint32_t word1 = (A.r + 65u) >> 2, shift1 = (A.r + 65u) & 3u;
  put_hex_field(col, lane, word0, shift0, col[word0][lane], col[word0 + 16][lane], prev);
  put_hex_field(col, lane, word1, shift1, col[word1][lane], col[word1 + 16][lane], d);

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
  for (int i = 0; i < 8; ++i) st[i] = A.ostate[i];
  chunk_compress(st, w);

  uint4* out = reinterpret_cast<uint4*>(A.trailer + 8 * part);
  out[0] = make_uint4(bswap(st[0]), bswap(st[1]), bswap(st[2]), bswap(st[3]));
  out[1] = make_uint4(bswap(st[4]), bswap(st[5]), bswap(st[6]), bswap(st[7]));
}

}  // namespace s3h
