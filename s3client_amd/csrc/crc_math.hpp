// crc_math.hpp -- the GF(2) arithmetic of the reflected 32-bit CRCs (CRC-32C, CRC-32) that the
// gfx950 kernels (crc32_kernels.hip), the plan builder (crc.cpp) and the CPU functions
// (cpu/lib_crc.cpp) share: compiled into all three, so the tables a kernel reads and the
// constants the host hands it come from the same code.  Header-only, no dependencies.
//
// Representation.  A 32-bit value is a polynomial over GF(2) of degree < 32 in the reflected bit
// order every table-driven CRC uses: bit 31 is the coefficient of x^0, bit 0 of x^31, so
// 0x80000000 is 1 and multiplying by x is a right shift (reduced by `poly`, the reflected
// generator without its x^32 term: 0x82F63B78 Castagnoli, 0xEDB88320 ISO-HDLC).
//
// The RAW value of a message M is M(x) * x^32 mod P: the CRC register after feeding M with
// init 0 and no xor-out.  It is linear, so
//     raw(A || B) = raw(A) * x^(8|B|)  ^  raw(B)              (segment fold)
//     raw(0...0 || B) = raw(B)                                (leading zeros are free)
//     raw(B) = raw(B || k zero bytes) * x^(-8k)               (un-shift; x is a unit: P(0) = 1)
// and the finalised CRC (init and xor-out 0xFFFFFFFF) is
//     crc(M) = 0xFFFFFFFF ^ 0xFFFFFFFF * x^(8|M|) ^ raw(M)
//     crc(A || B) = crc(A) * x^(8|B|) ^ crc(B)                (combine, on finalised values)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define S3H_CRC_HD __host__ __device__ inline
#else
#define S3H_CRC_HD inline
#endif

namespace s3h::crc {

constexpr uint32_t kPolyCrc32c = 0x82F63B78u;  // Castagnoli, reflected
constexpr uint32_t kPolyCrc32 = 0xEDB88320u;   // ISO-HDLC (zlib), reflected
constexpr uint32_t kOne = 0x80000000u;         // the polynomial 1

// Device tables, in 32-bit words (one block per polynomial, built by build_device_tables):
//   [0, 4096)     slicing-by-16: table k (k = 0..15), entry b = raw(byte b || k zero bytes)
//   [4096, 5120)  tile shift: table j (j = 0..3), entry b = (b << 8j) * x^(8 * kTileBytes)
//   [5120, 5136)  x^(-8k), k = 0..15 (un-shift of the masked tail of a segment's last line)
//   [5136, 5142)  x^(8 * 16 * 2^k), k = 0..5 (the lane tree of a tile: 16-byte lines)
constexpr uint32_t kLineBytes = 16;    // one lane's load (dwordx4)
constexpr uint32_t kTileBytes = 1024;  // one wave-instruction: 64 lanes x 16 bytes
constexpr uint32_t kSliceWords = 16 * 256;
constexpr uint32_t kShiftAt = kSliceWords, kShiftWords = 4 * 256;
constexpr uint32_t kInvAt = kShiftAt + kShiftWords, kInvWords = 16;
constexpr uint32_t kTreeAt = kInvAt + kInvWords, kTreeWords = 6;
constexpr uint32_t kTableWords = kTreeAt + kTreeWords + 2;  // padded to a multiple of 4 words

// a * x mod P
S3H_CRC_HD constexpr uint32_t mulx(uint32_t a, uint32_t poly) {
  return (a >> 1) ^ ((a & 1u) ? poly : 0u);
}

// a * x^-1 mod P: the x^0 coefficient (bit 31) of a product by x is set exactly when the
// reduction added P, whose constant term is 1.
S3H_CRC_HD constexpr uint32_t divx(uint32_t a, uint32_t poly) {
  return (a & kOne) ? (((a ^ poly) << 1) | 1u) : (a << 1);
}

// a * b mod P (32 shift-and-add steps, no table)
S3H_CRC_HD constexpr uint32_t mulmod(uint32_t a, uint32_t b, uint32_t poly) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= (a & kOne) ? b : 0u;
    a <<= 1;
    b = mulx(b, poly);
  }
  return p;
}

// x^(8 * bytes) mod P by square-and-multiply on the 64-bit byte count
S3H_CRC_HD constexpr uint32_t xpow8(uint64_t bytes, uint32_t poly) {
  uint32_t r = kOne, sq = kOne >> 8;  // x^8
  while (bytes) {
    if (bytes & 1u) r = mulmod(r, sq, poly);
    bytes >>= 1;
    if (bytes) sq = mulmod(sq, sq, poly);
  }
  return r;
}

// x^(-8k) mod P for the k < 16 zero bytes a masked last line appends
S3H_CRC_HD constexpr uint32_t xinv8(uint32_t k, uint32_t poly) {
  uint32_t r = kOne;
  for (uint32_t i = 0; i < 8 * k; ++i) r = divx(r, poly);
  return r;
}

// raw(A || B) from raw(A), raw(B) and x^(8|B|); the same on finalised CRCs (combine)
S3H_CRC_HD constexpr uint32_t fold(uint32_t a, uint32_t b, uint32_t xpow_b, uint32_t poly) {
  return mulmod(a, xpow_b, poly) ^ b;
}

// crc(A || B) from the finalised crc(A), crc(B) and |B|
S3H_CRC_HD constexpr uint32_t combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b, uint32_t poly) {
  return fold(crc_a, crc_b, xpow8(len_b, poly), poly);
}

// the finalised CRC (init / xor-out 0xFFFFFFFF) of a message of `len` bytes from its raw value
S3H_CRC_HD constexpr uint32_t finalise(uint32_t raw, uint64_t len, uint32_t poly) {
  return 0xFFFFFFFFu ^ mulmod(0xFFFFFFFFu, xpow8(len, poly), poly) ^ raw;
}

// raw value after one more byte (bitwise; what the tables are generated from)
S3H_CRC_HD constexpr uint32_t raw_byte(uint32_t raw, uint8_t byte, uint32_t poly) {
  raw ^= byte;
  for (int i = 0; i < 8; ++i) raw = mulx(raw, poly);
  return raw;
}

// Slicing tables: t[k * 256 + b] = raw(byte b || k zero bytes), k = 0..slices-1.  One step over
// `slices` bytes d[0..slices) from state s (s xored into d[0..3]) is the xor of
// t[(slices - 1 - i) * 256 + d[i]].
S3H_CRC_HD constexpr void build_slicing_tables(uint32_t poly, uint32_t slices, uint32_t* t) {
  for (uint32_t b = 0; b < 256; ++b) t[b] = raw_byte(0, uint8_t(b), poly);
  for (uint32_t k = 1; k < slices; ++k)
    for (uint32_t b = 0; b < 256; ++b) {
      const uint32_t prev = t[(k - 1) * 256 + b];
      t[k * 256 + b] = (prev >> 8) ^ t[prev & 0xFFu];
    }
}

// Multiplication by the constant `m` as four byte tables: t[j * 256 + b] = (b << 8j) * m, so
// a * m = t[a & 255] ^ t[256 + (a >> 8 & 255)] ^ t[512 + (a >> 16 & 255)] ^ t[768 + (a >> 24)].
S3H_CRC_HD constexpr void build_mul_tables(uint32_t m, uint32_t poly, uint32_t* t) {
  for (uint32_t j = 0; j < 4; ++j) {
    uint32_t* tj = t + j * 256;
    tj[0] = 0;
    for (uint32_t bit = 0; bit < 8; ++bit) tj[1u << bit] = mulmod(1u << (8 * j + bit), m, poly);
    for (uint32_t b = 1; b < 256; ++b)
      if (b & (b - 1)) tj[b] = tj[b & (b - 1)] ^ tj[b & (0u - b)];  // linear in b
  }
}

// The kTableWords words a CRC kernel copies to LDS (layout above).
S3H_CRC_HD constexpr void build_device_tables(uint32_t poly, uint32_t* t) {
  build_slicing_tables(poly, 16, t);
  build_mul_tables(xpow8(kTileBytes, poly), poly, t + kShiftAt);
  for (uint32_t k = 0; k < kInvWords; ++k) t[kInvAt + k] = xinv8(k, poly);
  for (uint32_t k = 0; k < kTreeWords; ++k) t[kTreeAt + k] = xpow8(uint64_t(kLineBytes) << k, poly);
  for (uint32_t k = kTreeAt + kTreeWords; k < kTableWords; ++k) t[k] = 0;
}

// ---------------------------------------------------------------- the kernels' decomposition
// What stage 1 computes for one segment and stage 2 for one part, as plain loops over the same
// table lookups and folds: the kernels follow these line by line, and the host model
// (tests/cpp/crc_model.cpp) runs them against the CPU functions.

// One 16-byte line (bytes outside the segment already zero) from state 0.
S3H_CRC_HD uint32_t line_raw(const uint32_t* slicing, const uint32_t w[4]) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < 4; ++i)
    for (uint32_t b = 0; b < 4; ++b)
      r ^= slicing[(15 - (4 * i + b)) * 256 + ((w[i] >> (8 * b)) & 0xFFu)];
  return r;
}

S3H_CRC_HD uint32_t mul_by_table(const uint32_t* t, uint32_t a) {
  return t[a & 0xFFu] ^ t[256 + ((a >> 8) & 0xFFu)] ^ t[512 + ((a >> 16) & 0xFFu)] ^ t[768 + (a >> 24)];
}

// Keeps bytes [lead, 16 - trail) of line word i (memory order: byte 0 is the lowest address).
S3H_CRC_HD uint32_t line_mask(uint32_t i, uint32_t lead, uint32_t trail) {
  const uint32_t lo = lead > 4 * i ? lead - 4 * i : 0, hi = trail > 4 * (3 - i) ? trail - 4 * (3 - i) : 0;
  const uint32_t ml = lo >= 4 ? 0u : 0xFFFFFFFFu << (8 * lo), mh = hi >= 4 ? 0u : 0xFFFFFFFFu >> (8 * hi);
  return ml & mh;
}

// The geometry of one segment: bytes [addr, addr + len), len >= 1, cut into 16-byte-aligned
// lines and padded in FRONT with virtual zero lines to whole tiles of 64 lines.
struct SegGeom {
  uint64_t first;   // index (address / 16) of the line holding the first byte
  uint32_t lines;   // lines holding at least one byte of the segment
  uint32_t tiles;   // ceil(lines / 64)
  uint32_t pad;     // virtual zero lines in front: tiles * 64 - lines
  uint32_t lead;    // bytes of the first line in front of the segment
  uint32_t trail;   // bytes of the last line behind the segment
};
S3H_CRC_HD SegGeom seg_geom(uint64_t addr, uint64_t len) {
  SegGeom g;
  const uint64_t last = (addr + len - 1) >> 4;
  g.first = addr >> 4;
  g.lines = uint32_t(last - g.first) + 1;
  g.tiles = (g.lines + 63) >> 6;
  g.pad = g.tiles * 64 - g.lines;
  g.lead = uint32_t(addr & 15);
  g.trail = 15 - uint32_t((addr + len - 1) & 15);
  return g;
}

// ---------------------------------------------------------------- ranged (resumable) launches
// A ranged launch covers bytes [begin, end) of every part.  Its pieces are cut on the plan's
// segment grid (S = 2^log2s bytes, counted from each part's byte 0): piece k of a part of `len`
// bytes is [k * S, (k + 1) * S) & [begin, end) & [0, len).  Stage 1 runs one wave per
// (part, k) with k in [range_first_piece, + range_pieces) and leaves piece k's raw value in the
// part's k-th slot of the partials buffer; stage 2 folds the part's pieces into its running
// value.  The kernels (crc_range_pieces_kernel, crc_range_parts_kernel) and the host model
// (tests/cpp/crc_range_model.cpp) both call these functions.

S3H_CRC_HD uint64_t range_first_piece(uint64_t begin, uint32_t log2s) { return begin >> log2s; }
// pieces per part of a launch (begin < end)
S3H_CRC_HD uint64_t range_pieces(uint64_t begin, uint64_t end, uint32_t log2s) {
  return ((end - 1) >> log2s) - (begin >> log2s) + 1;
}

struct Piece {
  uint64_t lo, hi;  // bytes [lo, hi) of the part; empty when lo >= hi
};
S3H_CRC_HD Piece piece_of(uint64_t k, uint32_t log2s, uint64_t begin, uint64_t end, uint64_t len) {
  const uint64_t a = k << log2s, b = a + (uint64_t(1) << log2s), e = end < len ? end : len;
  Piece p;
  p.lo = a > begin ? a : begin;
  p.hi = b < e ? b : e;
  return p;
}

// What stage 2 does for one part of `len` bytes in a launch over [begin, end).
struct PartRange {
  uint64_t bytes;   // m: bytes of the part inside the range (0: the part is not touched, unless
                    // it is empty and begin == 0, when its CRC is written)
  uint64_t first;   // k of the part's first non-empty piece
  uint64_t front;   // pieces in front of the last one; all but the first of them hold S bytes,
                    // and the first folds like a whole one (its missing front is leading zeros)
  uint64_t tail;    // bytes of the last piece (1..S)
  bool emits;       // the range holds the part's last byte (or the part is empty, begin == 0)
};
S3H_CRC_HD PartRange part_range(uint64_t len, uint64_t begin, uint64_t end, uint32_t log2s) {
  PartRange r;
  const uint64_t e = end < len ? end : len;
  r.bytes = e > begin ? e - begin : 0;
  r.first = begin >> log2s;
  r.front = 0;
  r.tail = 0;
  r.emits = r.bytes ? e == len : (len == 0 && begin == 0);
  if (r.bytes) {
    const uint64_t last = (e - 1) >> log2s, a = last << log2s;
    r.front = last - r.first;
    r.tail = e - (a > begin ? a : begin);
  }
  return r;
}

// The part's running raw value after a launch: `fresh` is the raw value of the range's bytes.
// At begin == 0 the old value is ignored (a new pass starts).
S3H_CRC_HD uint32_t range_state(uint32_t old, uint32_t fresh, uint64_t begin, uint64_t bytes, uint32_t poly) {
  return begin == 0 ? fresh : fold(old, fresh, xpow8(bytes, poly), poly);
}
// finalise() of a finished part, written out: a second device caller of finalise() itself
// stops the compiler from inlining it into crc_parts_kernel, whose machine code is pinned
// (s3client_amd/kernel_isa_counts.json).  tests/cpp/crc_range_model.cpp checks the two agree.
S3H_CRC_HD uint32_t range_emit(uint32_t state, uint64_t len, uint32_t poly) {
  return ~state ^ mulmod(0xFFFFFFFFu, xpow8(len, poly), poly);
}

}  // namespace s3h::crc
