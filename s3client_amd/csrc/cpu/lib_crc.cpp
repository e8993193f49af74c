// lib_crc.cpp -- CPU side of the CRC-32C / CRC-32 checksums (include/s3hash.h): the
// single-message function, the combine / full-object fold over part checksums and the header
// text forms S3's "additional checksums" use.  HIP-free.
//
// Single message: slicing-by-8 on tables from the generator the GPU tables come from
// (crc_math.hpp); on x86 with SSE4.2 the `crc32` instruction for CRC-32C, chosen at load time
// like the SHA extensions in lib_hash.cpp.  S3H_CPU_SCALAR=1 forces the table path.
#if defined(__x86_64__)
#include <cpuid.h>
#include <nmmintrin.h>
#endif

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../../include/s3hash.h"
#include "../crc_math.hpp"
#include "../status.hpp"

namespace {

using s3h::host::fail;
namespace gf = s3h::crc;

struct Tables {
  uint32_t t[2][8 * 256];
  Tables() {
    gf::build_slicing_tables(gf::kPolyCrc32c, 8, t[S3H_CRC32C]);
    gf::build_slicing_tables(gf::kPolyCrc32, 8, t[S3H_CRC32]);
  }
};
const Tables g_tables;

bool known(int crc) { return crc == S3H_CRC32C || crc == S3H_CRC32; }
uint32_t poly_of(int crc) { return crc == S3H_CRC32C ? gf::kPolyCrc32c : gf::kPolyCrc32; }

// register value in, register value out (the caller applies init / xor-out)
uint32_t update_table(const uint32_t *t, uint32_t c, const uint8_t *p, uint64_t n) {
  for (; n >= 8; n -= 8, p += 8) {
    uint32_t a, b;
    std::memcpy(&a, p, 4);
    std::memcpy(&b, p + 4, 4);
    a ^= c;
    c = t[7 * 256 + (a & 0xFFu)] ^ t[6 * 256 + ((a >> 8) & 0xFFu)] ^ t[5 * 256 + ((a >> 16) & 0xFFu)] ^
        t[4 * 256 + (a >> 24)] ^ t[3 * 256 + (b & 0xFFu)] ^ t[2 * 256 + ((b >> 8) & 0xFFu)] ^
        t[1 * 256 + ((b >> 16) & 0xFFu)] ^ t[b >> 24];
  }
  for (; n; --n, ++p) c = t[(c ^ *p) & 0xFFu] ^ (c >> 8);
  return c;
}

#if defined(__x86_64__)
__attribute__((target("sse4.2")))
uint32_t update_crc32c_sse42(uint32_t c, const uint8_t *p, uint64_t n) {
  uint64_t c64 = c;
  for (; n >= 8; n -= 8, p += 8) {
    uint64_t v;
    std::memcpy(&v, p, 8);
    c64 = _mm_crc32_u64(c64, v);
  }
  c = uint32_t(c64);
  for (; n; --n, ++p) c = _mm_crc32_u8(c, *p);
  return c;
}

bool pick_sse42() {
  const char *force = std::getenv("S3H_CPU_SCALAR");
  if (force && force[0] == '1') return false;
  unsigned a, b, c, d;
  if (!__get_cpuid(1, &a, &b, &c, &d)) return false;
  return (c & (1u << 20)) != 0;
}
const bool g_sse42 = pick_sse42();
#endif

void base64(const uint8_t *in, size_t n, char *out) {
  static const char *const a = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  size_t o = 0;
  for (size_t i = 0; i < n; i += 3) {
    const uint32_t v = uint32_t(in[i]) << 16 | (i + 1 < n ? uint32_t(in[i + 1]) << 8 : 0) |
                       (i + 2 < n ? uint32_t(in[i + 2]) : 0);
    out[o++] = a[v >> 18];
    out[o++] = a[(v >> 12) & 63];
    out[o++] = i + 1 < n ? a[(v >> 6) & 63] : '=';
    out[o++] = i + 2 < n ? a[v & 63] : '=';
  }
  out[o] = '\0';
}

void big_endian(uint32_t v, uint8_t *out) {
  out[0] = uint8_t(v >> 24);
  out[1] = uint8_t(v >> 16);
  out[2] = uint8_t(v >> 8);
  out[3] = uint8_t(v);
}

}  // namespace

extern "C" {

uint32_t s3h_cpu_crc(int crc, const uint8_t *data, uint64_t length, uint32_t seed_crc) {
  if (!known(crc) || (!data && length)) {
    fail(S3H_EINVAL, "cpu crc: unknown checksum %d or null data", crc);
    return 0;
  }
  uint32_t c = seed_crc ^ 0xFFFFFFFFu;
#if defined(__x86_64__)
  if (crc == S3H_CRC32C && g_sse42) return update_crc32c_sse42(c, data, length) ^ 0xFFFFFFFFu;
#endif
  return update_table(g_tables.t[crc], c, data, length) ^ 0xFFFFFFFFu;
}

int s3h_crc_combine(int crc, uint32_t crc_a, uint32_t crc_b, uint64_t len_b, uint32_t *out) {
  if (!known(crc)) return fail(S3H_EINVAL, "crc combine: unknown checksum %d", crc);
  if (!out) return fail(S3H_EINVAL, "crc combine: null out-pointer");
  *out = gf::combine(crc_a, crc_b, len_b, poly_of(crc));
  return S3H_OK;
}

int s3h_crc_object(int crc, const uint32_t *part_crcs, const uint64_t *lengths, uint64_t n,
                   uint32_t *out) {
  if (!known(crc)) return fail(S3H_EINVAL, "crc object: unknown checksum %d", crc);
  if (!part_crcs || !lengths || !out || n == 0)
    return fail(S3H_EINVAL, "crc object: null argument or no parts");
  const uint32_t poly = poly_of(crc);
  uint32_t acc = part_crcs[0];
  for (uint64_t i = 1; i < n; ++i) acc = gf::combine(acc, part_crcs[i], lengths[i], poly);
  *out = acc;
  return S3H_OK;
}

int s3h_checksum_text(int crc, const uint32_t *part_crcs, uint64_t n, int composite, char *out,
                      uint64_t out_len) {
  if (out && out_len) out[0] = '\0';
  if (!known(crc)) return fail(S3H_EINVAL, "checksum text: unknown checksum %d", crc);
  if (!out || out_len < S3H_CHECKSUM_MAX)
    return fail(S3H_EINVAL, "checksum text: need %d output bytes", S3H_CHECKSUM_MAX);
  if (!part_crcs || n == 0) return fail(S3H_EINVAL, "checksum text: no part checksums");
  if (composite != 0 && composite != 1) return fail(S3H_EINVAL, "checksum text: composite must be 0 or 1");
  uint8_t be[4];
  if (!composite) {
    if (n != 1) return fail(S3H_EINVAL, "checksum text: the plain form takes one checksum (n=%llu)",
                            static_cast<unsigned long long>(n));
    big_endian(part_crcs[0], be);
    base64(be, 4, out);
    return S3H_OK;
  }
  // composite: the checksum of the parts' big-endian checksums concatenated, then "-n"
  uint32_t c = 0;
  for (uint64_t i = 0; i < n; ++i) {
    big_endian(part_crcs[i], be);
    c = s3h_cpu_crc(crc, be, 4, c);
  }
  big_endian(c, be);
  base64(be, 4, out);
  std::snprintf(out + 8, size_t(out_len - 8), "-%llu", static_cast<unsigned long long>(n));
  return S3H_OK;
}

}  // extern "C"
