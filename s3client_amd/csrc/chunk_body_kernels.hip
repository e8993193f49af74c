// chunk_body_kernels.hip -- the wire form of a chunk-signed upload (an aws-chunked body) for
// MI355X (gfx950): the parts' bytes gathered into framed bodies, ready for one copy to the host.
//
//   body = { hex(k) ";chunk-signature=" hex(sig_i) "\r\n" chunk_i "\r\n" }   k bytes each
//          "0;chunk-signature=" hex(sig_last) "\r\n"
//          "\r\n"   |   name ":" base64(crc) "\r\nx-amz-trailer-signature:" hex(trailer_sig) "\r\n\r\n"
//
// One work item per piece of a data chunk (at most kChunkBodyPiece contiguous bytes) and one per
// part for its final line and ending; one wave per item, the items of a launch taken in grid
// stride.  An item finds its part by bisection over the parts' first items, and its place in the
// body in closed form (every full chunk of a plan has the same wire length).  The wave of a
// chunk's first piece writes the framing line, the wave of its last piece the "\r\n" behind it.
//
// The copy.  A piece's destination starts at any byte, and the source's shift against it,
// (src - dst) mod 16, is uniform over the piece and differs from chunk to chunk.  The bytes up to
// the destination's first 16-byte boundary and from its last go out as byte stores, one lane
// each; between them lane l writes the aligned line l of a 64-line tile as one dwordx4, funnel-
// shifted (v_alignbyte_b32) out of the two aligned source lines that hold its bytes.  Of the
// payload only aligned lines holding a byte of the piece are loaded (crc32_kernels.hip's rule):
// the second line only where the shift is not zero, and then it holds bytes of the same
// destination line.  Nothing is read back from the output and every byte of a body is written
// once.  The text -- lengths, signatures, checksum -- is rendered a character per lane with hex4
// and base64_4 of the chain and trailer kernels and stored as bytes.
//
// A lane loads its second source line itself: taking it from the neighbour lane's first (a
// cross-lane move, lane 63 alone loading) measured 4 % slower on C2 and needs 14 more VGPRs
// (profiles/chunk_body_c2.json).
//
// The kernel lives in a text section of its own, so the machine code of the kernels pinned in
// s3client_amd/kernel_isa_counts.json stays as it is.
#pragma once
#include "chunk_trailer_kernels.hip"

namespace s3h {

#define S3H_BODY_TEXT __attribute__((section(".text.s3h_chunk_body")))

namespace bodydev {

// The aligned line that holds absolute address `addr`, as an offset from the base pointer (not a
// cast of the address: the loads stay global loads).
__device__ __forceinline__ const uint4* line_at(const uint8_t* base, uint64_t addr) {
  return reinterpret_cast<const uint4*>(base + ((addr & ~uint64_t(15)) - reinterpret_cast<uint64_t>(base)));
}

__device__ __forceinline__ uint32_t line_byte(const uint4& v, uint32_t k) {
  // (shifts, not a select among the four words: the compiler turns that into an array in LDS)
  const uint64_t h = k & 8u ? uint64_t(v.w) << 32 | v.z : uint64_t(v.y) << 32 | v.x;
  return uint32_t(h >> (8 * (k & 7u))) & 0xFFu;
}

// count <= 15 bytes from absolute source address `src`, a lane each.
__device__ __forceinline__ void copy_edge(const uint8_t* base, uint64_t src, uint8_t* dst, uint32_t count,
                                          uint32_t lane) {
  if (lane < count) {
    const uint64_t a = src + lane;
    const uint4 v = *line_at(base, a);
    dst[lane] = uint8_t(line_byte(v, uint32_t(a) & 15u));
  }
}

// Bytes [4 * Q + r, 4 * Q + r + 16) of the 32 bytes lo ++ hi.
template <int Q>
__device__ __forceinline__ uint4 realign(const uint4& lo, const uint4& hi, uint32_t r) {
  const uint32_t x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return make_uint4(__builtin_amdgcn_alignbyte(x[Q + 1], x[Q], r), __builtin_amdgcn_alignbyte(x[Q + 2], x[Q + 1], r),
                    __builtin_amdgcn_alignbyte(x[Q + 3], x[Q + 2], r), __builtin_amdgcn_alignbyte(x[Q + 4], x[Q + 3], r));
}

// Destination lines q[0 .. nb) from source lines p[0 .. nb] at byte shift 4 * Q + r; `two`: the
// shift is not zero, so line i also takes bytes of p[i + 1].
template <int Q>
__device__ __forceinline__ void copy_lines(const uint4* p, uint4* q, uint32_t nb, uint32_t r, bool two,
                                           uint32_t lane) {
  uint32_t t = 0;
  for (; t + 256 <= nb; t += 256) {  // whole tiles, four in flight per lane
    const uint32_t i = t + lane;
    const uint4 a0 = p[i], a1 = p[i + 64], a2 = p[i + 128], a3 = p[i + 192];
    uint4 b0 = a0, b1 = a1, b2 = a2, b3 = a3;
    if (two) b0 = p[i + 1], b1 = p[i + 65], b2 = p[i + 129], b3 = p[i + 193];
    q[i] = realign<Q>(a0, b0, r);
    q[i + 64] = realign<Q>(a1, b1, r);
    q[i + 128] = realign<Q>(a2, b2, r);
    q[i + 192] = realign<Q>(a3, b3, r);
  }
  for (; t < nb; t += 64) {
    const uint32_t i = t + lane;
    if (i < nb) {
      const uint4 a = p[i];
      const uint4 b = two ? p[i + 1] : a;
      q[i] = realign<Q>(a, b, r);
    }
  }
}

// 1 <= `len` <= kChunkBodyPiece bytes from absolute source address `src` to body + dst_off (any
// alignment): the offsets are 64-bit, what counts lines within the piece is not.
__device__ __forceinline__ void copy_run(const uint8_t* base, uint64_t src, uint8_t* body, uint64_t dst_off,
                                         uint32_t len, uint32_t lane) {
  const uint32_t to_line = uint32_t(0 - (reinterpret_cast<uint64_t>(body) + dst_off)) & 15u;
  const uint32_t head = len < to_line ? len : to_line;
  const uint32_t nb = (len - head) >> 4;
  const uint32_t tail = (len - head) & 15u;
  copy_edge(base, src, body + dst_off, head, lane);
  copy_edge(base, src + head + 16 * nb, body + dst_off + head + 16 * nb, tail, lane);
  if (nb == 0) return;
  const uint64_t s = src + head;
  const uint32_t shift = __builtin_amdgcn_readfirstlane(uint32_t(s) & 15u);
  const uint4* p = line_at(base, s);
  uint4* q = reinterpret_cast<uint4*>(body + dst_off + head);
  const uint32_t r = shift & 3u;
  switch (shift >> 2) {
    case 0: copy_lines<0>(p, q, nb, r, shift != 0, lane); break;
    case 1: copy_lines<1>(p, q, nb, r, true, lane); break;
    case 2: copy_lines<2>(p, q, nb, r, true, lane); break;
    default: copy_lines<3>(p, q, nb, r, true, lane); break;
  }
}

// Character j (0 .. 63) of the lowercase hex of a signature row (8 words, word i = bswap32(H_i):
// the digest's bytes in memory order).
__device__ __forceinline__ uint32_t hex_char(const uint32_t* row, uint32_t j) {
  const uint32_t byte = (row[j >> 3] >> (8 * ((j >> 1) & 3u))) & 0xFFu;
  return hex4((byte >> (4 * (~j & 1u))) & 15u) & 0xFFu;
}

__device__ __forceinline__ uint32_t hexlen(uint64_t k) {
  return k == 0 ? 1u : uint32_t(64 - __builtin_clzll(k) + 3) >> 2;
}

// The framing line of a chunk of k bytes, hl = hexlen(k): hl + 83 bytes at out.
__device__ __forceinline__ void put_header(uint8_t* out, uint64_t k, uint32_t hl, const uint32_t* row,
                                           const uint8_t* text, uint32_t lane) {
  for (uint32_t i = lane; i < hl + 83u; i += 64) {
    uint32_t ch;
    if (i < hl) ch = hex4(uint32_t(k >> (4 * (hl - 1 - i))) & 15u) & 0xFFu;
    else if (i < hl + 17u) ch = text[i - hl];
    else if (i < hl + 81u) ch = hex_char(row, i - hl - 17u);
    else ch = i == hl + 81u ? '\r' : '\n';
    out[i] = uint8_t(ch);
  }
}

}  // namespace bodydev

S3H_BODY_TEXT __global__ __launch_bounds__(kChunkBodyThreads) void chunk_body_kernel(ChunkBodyArgs A) {
  using namespace bodydev;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr uint32_t kWaves = kChunkBodyThreads / 64;
  const uint64_t c = A.chunk_bytes, stride = A.head_len + c + 2;
  for (uint64_t item = uint64_t(blockIdx.x) * kWaves + wave; item < A.items; item += uint64_t(gridDim.x) * kWaves) {
    // the item's part: the last one whose first item is not behind it
    uint64_t lo = 0, hi = A.n;
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if (A.parts[mid].item0 <= item) lo = mid; else hi = mid;
    }
    const ChunkBodyPart pt = A.parts[lo];
    const uint64_t body = A.body_offs[lo];
    const uint64_t j = item - pt.item0, rem = pt.len - pt.full * c;
    const uint64_t full_items = pt.full * A.pieces_per_chunk;
    const uint64_t rem_items = (rem + kChunkBodyPiece - 1) / kChunkBodyPiece;
    if (j < full_items + rem_items) {  // a piece of a data chunk
      uint64_t chunk = pt.full, piece = j - full_items, k = rem;
      if (j < full_items) {
        chunk = A.pieces_per_chunk == 1 ? j : j / A.pieces_per_chunk;
        piece = j - chunk * A.pieces_per_chunk;
        k = c;
      }
      const uint32_t hl = k == c ? A.head_len - 83u : hexlen(k);
      const uint64_t at = body + chunk * stride, data = at + hl + 83u;
      const uint64_t begin = piece * kChunkBodyPiece;
      const uint32_t len = k - begin < kChunkBodyPiece ? uint32_t(k - begin) : kChunkBodyPiece;
      if (piece == 0) put_header(A.body + at, k, hl, A.signatures + 8 * (pt.sig + chunk), A.text, lane);
      if (begin + len == k && lane < 2) A.body[data + k + lane] = lane == 0 ? '\r' : '\n';
      copy_run(A.base, reinterpret_cast<uint64_t>(A.base) + pt.off + chunk * c + begin, A.body, data + begin, len, lane);
      continue;
    }
    // the final line and the ending
    const uint64_t chunks = pt.full + (rem != 0);
    const uint64_t at = body + pt.full * stride + (rem ? hexlen(rem) + 85u + rem : 0);
    put_header(A.body + at, 0, 1, A.signatures + 8 * (pt.sig + chunks), A.text, lane);
    uint8_t* out = A.body + at + 84;
    if (!A.checksums) {
      if (lane < 2) out[lane] = lane == 0 ? '\r' : '\n';
      continue;
    }
    // the value's big-endian bytes as base64, as sigv4_trailer_kernel renders them
    uint32_t vhi, vlo = 0;
    if (A.wide) {
      const uint64_t v = static_cast<const uint64_t*>(A.checksums)[lo];
      vhi = uint32_t(v >> 32);
      vlo = uint32_t(v);
    } else {
      vhi = static_cast<const uint32_t*>(A.checksums)[lo];
    }
    const uint32_t x0 = base64_4(sextets4(vhi >> 8));
    uint32_t x1 = base64_4(sextets4(((vhi & 0xFFu) << 16) | (vlo >> 16)));
    uint32_t x2 = base64_4(sextets4((vlo & 0xFFFFu) << 8));
    if (A.wide) x2 = (x2 & 0xFFFFFF00u) | 0x3Du;
    else x1 = (x1 & 0xFFFF0000u) | 0x3D3Du;
    const uint32_t text_len = A.wide ? 12u : 8u;
    const uint32_t sig_at = A.name_len + text_len, hex_at = sig_at + 26u, total = hex_at + 68u;
    const uint32_t* row = A.trailer + 8 * lo;
    for (uint32_t i = lane; i < total; i += 64) {
      uint32_t ch;
      if (i < A.name_len) {
        ch = A.text[kChunkBodyNameAt + i];
      } else if (i < sig_at) {
        const uint32_t m = i - A.name_len, w = m < 4 ? x0 : m < 8 ? x1 : x2;
        ch = (w >> (8 * (~m & 3u))) & 0xFFu;
      } else if (i < hex_at) {
        ch = A.text[kChunkBodySigAt + i - sig_at];
      } else if (i < hex_at + 64u) {
        ch = hex_char(row, i - hex_at);
      } else {
        ch = (i - hex_at) & 1u ? '\n' : '\r';
      }
      out[i] = uint8_t(ch);
    }
  }
}

}  // namespace s3h
