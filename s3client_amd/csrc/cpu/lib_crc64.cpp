// lib_crc64.cpp -- CPU side of the CRC-64/NVME checksum (include/s3hash.h): the single-message
// function (slicing-by-8 on tables from the generator the GPU tables come from, crc64_math.hpp),
// the combine / full-object fold over part checksums and the header text of
// x-amz-checksum-crc64nvme.  HIP-free.
#include <cstdint>
#include <cstring>

#include "../../../include/s3hash.h"
#include "../crc64_math.hpp"
#include "../status.hpp"

namespace {

using s3h::host::fail;
namespace gf = s3h::crc64;

struct Tables {
  uint64_t t[8 * 256];
  Tables() { gf::build_slicing_tables(gf::kPolyNvme, 8, t); }
};
const Tables g_tables;

// register value in, register value out (the caller applies init / xor-out)
uint64_t update_table(const uint64_t *t, uint64_t c, const uint8_t *p, uint64_t n) {
  for (; n >= 8; n -= 8, p += 8) {
    uint8_t d[8];
    std::memcpy(d, p, 8);
    // (bytes in memory order, so the loop is the same on either endianness)
    c = t[7 * 256 + (d[0] ^ (c & 0xFFu))] ^ t[6 * 256 + (d[1] ^ ((c >> 8) & 0xFFu))] ^
        t[5 * 256 + (d[2] ^ ((c >> 16) & 0xFFu))] ^ t[4 * 256 + (d[3] ^ ((c >> 24) & 0xFFu))] ^
        t[3 * 256 + (d[4] ^ ((c >> 32) & 0xFFu))] ^ t[2 * 256 + (d[5] ^ ((c >> 40) & 0xFFu))] ^
        t[1 * 256 + (d[6] ^ ((c >> 48) & 0xFFu))] ^ t[d[7] ^ (c >> 56)];
  }
  for (; n; --n, ++p) c = t[(c ^ *p) & 0xFFu] ^ (c >> 8);
  return c;
}

}  // namespace

extern "C" {

uint64_t s3h_cpu_crc64nvme(const uint8_t *data, uint64_t length, uint64_t seed_crc) {
  if (!data && length) {
    fail(S3H_EINVAL, "cpu crc64nvme: null data");
    return 0;
  }
  return update_table(g_tables.t, seed_crc ^ gf::kAllOnes, data, length) ^ gf::kAllOnes;
}

int s3h_crc64nvme_combine(uint64_t crc_a, uint64_t crc_b, uint64_t len_b, uint64_t *out) {
  if (!out) return fail(S3H_EINVAL, "crc64nvme combine: null out-pointer");
  *out = gf::combine(crc_a, crc_b, len_b, gf::kPolyNvme);
  return S3H_OK;
}

int s3h_crc64nvme_object(const uint64_t *part_crcs, const uint64_t *lengths, uint64_t n, uint64_t *out) {
  if (!part_crcs || !lengths || !out || n == 0)
    return fail(S3H_EINVAL, "crc64nvme object: null argument or no parts");
  uint64_t acc = part_crcs[0];
  for (uint64_t i = 1; i < n; ++i) acc = gf::combine(acc, part_crcs[i], lengths[i], gf::kPolyNvme);
  *out = acc;
  return S3H_OK;
}

int s3h_checksum64_text(uint64_t crc, char *out, uint64_t out_len) {
  if (out && out_len) out[0] = '\0';
  if (!out || out_len < S3H_CHECKSUM_MAX)
    return fail(S3H_EINVAL, "checksum64 text: need %d output bytes", S3H_CHECKSUM_MAX);
  static const char *const a = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  uint8_t be[9] = {};
  for (int i = 0; i < 8; ++i) be[i] = uint8_t(crc >> (56 - 8 * i));
  size_t o = 0;
  for (int i = 0; i < 9; i += 3) {
    const uint32_t v = uint32_t(be[i]) << 16 | uint32_t(be[i + 1]) << 8 | be[i + 2];
    out[o++] = a[v >> 18];
    out[o++] = a[(v >> 12) & 63];
    out[o++] = a[(v >> 6) & 63];
    out[o++] = a[v & 63];
  }
  out[11] = '=';  // 8 bytes: two whole groups and one of two bytes
  out[12] = '\0';
  return S3H_OK;
}

}  // extern "C"
