// crc64_math.hpp -- the GF(2) arithmetic of the reflected 64-bit CRC S3 uses (CRC-64/NVME),
// the 64-bit counterpart of crc_math.hpp: shared by the gfx950 kernels (crc64_kernels.hip), the
// plan builder (crc.cpp) and the CPU functions (cpu/lib_crc64.cpp).  Header-only.
//
// Representation.  A 64-bit value is a polynomial over GF(2) of degree < 64 in reflected bit
// order: bit 63 is the coefficient of x^0, so 0x8000000000000000 is 1 and multiplying by x is a
// right shift, reduced by `poly`, the reflected generator without its x^64 term
// (0x9A6C9329AC4BC9B5 for the NVMe polynomial 0xAD93D23594C93659).  The RAW value of a message
// M is M(x) * x^64 mod P, and the identities at the top of crc_math.hpp (segment fold, free
// leading zeros, un-shift, finalise, combine) hold with x^64 in place of x^32 and all-ones
// 64-bit init / xor-out.
//
// The width-independent geometry -- seg_geom, line_mask, range_first_piece, range_pieces,
// piece_of, part_range -- is crc_math.hpp's, used as it is.
#pragma once
#include <stdint.h>

#include "crc_math.hpp"

namespace s3h::crc64 {

using s3h::crc::kLineBytes;
using s3h::crc::kTileBytes;

constexpr uint64_t kPolyNvme = 0x9A6C9329AC4BC9B5ull;  // CRC-64/NVME, reflected
constexpr uint64_t kOne = 0x8000000000000000ull;       // the polynomial 1
constexpr uint64_t kAllOnes = ~uint64_t(0);

// Device tables, in 64-bit words (built by build_device_tables):
//   [0, 4096)     slicing-by-16: table k (k = 0..15), entry b = raw(byte b || k zero bytes)
//   [4096, 6144)  tile shift: table j (j = 0..7), entry b = (b << 8j) * x^(8 * kTileBytes)
//   [6144, 6160)  x^(-8k), k = 0..15 (un-shift of the masked tail of a segment's last line)
//   [6160, 6224)  x^(8 * 16 * (63 - l)), l = 0..63: what follows lane l's line in the last tile.
//                 (A 64-bit mulmod costs about four times a 32-bit one, so the lanes are joined
//                 by one multiplication each and an xor reduction, not by the 32-bit kernels'
//                 6-step tree of multiplications.)
constexpr uint32_t kSliceWords = 16 * 256;
constexpr uint32_t kShiftAt = kSliceWords, kShiftWords = 8 * 256;
constexpr uint32_t kInvAt = kShiftAt + kShiftWords, kInvWords = 16;
constexpr uint32_t kLaneAt = kInvAt + kInvWords, kLaneWords = 64;
constexpr uint32_t kTableWords = kLaneAt + kLaneWords;  // 6224 words = 49,792 B, a multiple of 16 B
static_assert(kTableWords % 2 == 0, "the kernels copy the tables in 16-byte pieces");

// a * x mod P
S3H_CRC_HD constexpr uint64_t mulx(uint64_t a, uint64_t poly) {
  return (a >> 1) ^ ((a & 1u) ? poly : 0u);
}

// a * x^-1 mod P (P's constant term is 1: bit 63 of a product by x is set exactly when the
// reduction added P)
S3H_CRC_HD constexpr uint64_t divx(uint64_t a, uint64_t poly) {
  return (a & kOne) ? (((a ^ poly) << 1) | 1u) : (a << 1);
}

// a * b mod P (64 shift-and-add steps, no table)
S3H_CRC_HD constexpr uint64_t mulmod(uint64_t a, uint64_t b, uint64_t poly) {
  uint64_t p = 0;
  for (int i = 0; i < 64; ++i) {
    p ^= (a & kOne) ? b : 0u;
    a <<= 1;
    b = mulx(b, poly);
  }
  return p;
}

// x^(8 * bytes) mod P by square-and-multiply on the 64-bit byte count
S3H_CRC_HD constexpr uint64_t xpow8(uint64_t bytes, uint64_t poly) {
  uint64_t r = kOne, sq = kOne >> 8;  // x^8
  while (bytes) {
    if (bytes & 1u) r = mulmod(r, sq, poly);
    bytes >>= 1;
    if (bytes) sq = mulmod(sq, sq, poly);
  }
  return r;
}

// x^(-8k) mod P for the k < 16 zero bytes a masked last line appends
S3H_CRC_HD constexpr uint64_t xinv8(uint32_t k, uint64_t poly) {
  uint64_t r = kOne;
  for (uint32_t i = 0; i < 8 * k; ++i) r = divx(r, poly);
  return r;
}

// raw(A || B) from raw(A), raw(B) and x^(8|B|); the same on finalised CRCs (combine)
S3H_CRC_HD constexpr uint64_t fold(uint64_t a, uint64_t b, uint64_t xpow_b, uint64_t poly) {
  return mulmod(a, xpow_b, poly) ^ b;
}

// crc(A || B) from the finalised crc(A), crc(B) and |B|
S3H_CRC_HD constexpr uint64_t combine(uint64_t crc_a, uint64_t crc_b, uint64_t len_b, uint64_t poly) {
  return fold(crc_a, crc_b, xpow8(len_b, poly), poly);
}

// the finalised CRC (init / xor-out all ones) of a message of `len` bytes from its raw value
S3H_CRC_HD constexpr uint64_t finalise(uint64_t raw, uint64_t len, uint64_t poly) {
  return kAllOnes ^ mulmod(kAllOnes, xpow8(len, poly), poly) ^ raw;
}

// raw value after one more byte (bitwise; what the tables are generated from)
S3H_CRC_HD constexpr uint64_t raw_byte(uint64_t raw, uint8_t byte, uint64_t poly) {
  raw ^= byte;
  for (int i = 0; i < 8; ++i) raw = mulx(raw, poly);
  return raw;
}

// Slicing tables: t[k * 256 + b] = raw(byte b || k zero bytes), k = 0..slices-1.  One step over
// `slices` >= 8 bytes d[0..slices) from state s (s xored into d[0..7]) is the xor of
// t[(slices - 1 - i) * 256 + d[i]].
S3H_CRC_HD constexpr void build_slicing_tables(uint64_t poly, uint32_t slices, uint64_t* t) {
  for (uint32_t b = 0; b < 256; ++b) t[b] = raw_byte(0, uint8_t(b), poly);
  for (uint32_t k = 1; k < slices; ++k)
    for (uint32_t b = 0; b < 256; ++b) {
      const uint64_t prev = t[(k - 1) * 256 + b];
      t[k * 256 + b] = (prev >> 8) ^ t[prev & 0xFFu];
    }
}

// Multiplication by the constant `m` as eight byte tables: t[j * 256 + b] = (b << 8j) * m, so
// a * m is the xor over j of t[j * 256 + (a >> 8j & 255)].
S3H_CRC_HD constexpr void build_mul_tables(uint64_t m, uint64_t poly, uint64_t* t) {
  for (uint32_t j = 0; j < 8; ++j) {
    uint64_t* tj = t + j * 256;
    tj[0] = 0;
    for (uint32_t bit = 0; bit < 8; ++bit) tj[1u << bit] = mulmod(uint64_t(1) << (8 * j + bit), m, poly);
    for (uint32_t b = 1; b < 256; ++b)
      if (b & (b - 1)) tj[b] = tj[b & (b - 1)] ^ tj[b & (0u - b)];  // linear in b
  }
}

// The kTableWords words a CRC-64 kernel copies to LDS (layout above).
S3H_CRC_HD constexpr void build_device_tables(uint64_t poly, uint64_t* t) {
  build_slicing_tables(poly, 16, t);
  build_mul_tables(xpow8(kTileBytes, poly), poly, t + kShiftAt);
  for (uint32_t k = 0; k < kInvWords; ++k) t[kInvAt + k] = xinv8(k, poly);
  for (uint32_t l = 0; l < kLaneWords; ++l) t[kLaneAt + l] = xpow8(uint64_t(kLineBytes) * (63 - l), poly);
}

// ---------------------------------------------------------------- the kernels' decomposition
// As in crc_math.hpp: what the kernels do per line and per shift, as plain functions the host
// model (tests/cpp/crc64_model.cpp) runs over the same tables.

// One 16-byte line (bytes outside the segment already zero) from state 0.
S3H_CRC_HD uint64_t line_raw(const uint64_t* slicing, const uint32_t w[4]) {
  uint64_t r = 0;
  for (uint32_t i = 0; i < 4; ++i)
    for (uint32_t b = 0; b < 4; ++b)
      r ^= slicing[(15 - (4 * i + b)) * 256 + ((w[i] >> (8 * b)) & 0xFFu)];
  return r;
}

S3H_CRC_HD uint64_t mul_by_table(const uint64_t* t, uint64_t a) {
  const uint32_t lo = uint32_t(a), hi = uint32_t(a >> 32);
  return t[lo & 0xFFu] ^ t[256 + ((lo >> 8) & 0xFFu)] ^ t[512 + ((lo >> 16) & 0xFFu)] ^ t[768 + (lo >> 24)] ^
         t[1024 + (hi & 0xFFu)] ^ t[1280 + ((hi >> 8) & 0xFFu)] ^ t[1536 + ((hi >> 16) & 0xFFu)] ^
         t[1792 + (hi >> 24)];
}

// The part's running raw value after a ranged launch: `fresh` is the raw value of the range's
// bytes.  At begin == 0 the old value is ignored (a new pass starts).
S3H_CRC_HD uint64_t range_state(uint64_t old, uint64_t fresh, uint64_t begin, uint64_t bytes, uint64_t poly) {
  return begin == 0 ? fresh : fold(old, fresh, xpow8(bytes, poly), poly);
}

}  // namespace s3h::crc64
