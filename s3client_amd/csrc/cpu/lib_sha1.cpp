// lib_sha1.cpp -- CPU SHA-1 (FIPS 180-4 6.1) for x-amz-checksum-sha1: s3h_cpu_sha1, and the
// header text of the digest checksums (s3h_digest_checksum_text: x-amz-checksum-sha1 /
// -sha256 values and S3's COMPOSITE form).  Digest words follow the device's and SHA-256's
// convention: hash[i] = bswap32(H_i), so the 20 bytes in memory are the canonical digest.
//
// Two compressions, chosen at load time as lib_hash.cpp chooses SHA-256's: the x86 SHA
// extensions (sha1rnds4 / sha1nexte / sha1msg1 / sha1msg2) when the CPU has them, else a
// portable scalar loop.  S3H_CPU_SCALAR=1 in the environment forces the scalar loop.
#include <cpuid.h>
#include <immintrin.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../../include/s3hash.h"
#include "../status.hpp"

namespace {

using s3h::host::fail;

inline uint32_t rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

void compress_scalar(uint32_t st[5], const uint8_t *p, uint64_t nblk) {
  for (; nblk; --nblk, p += 64) {
    uint32_t w[80];
    for (int t = 0; t < 16; ++t) {
      uint32_t x;
      std::memcpy(&x, p + 4 * t, 4);
      w[t] = __builtin_bswap32(x);
    }
    for (int t = 16; t < 80; ++t) w[t] = rotl(w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16], 1);
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4];
    for (int t = 0; t < 80; ++t) {
      const uint32_t f = t < 20 ? (b & c) | (~b & d) : t < 40 ? b ^ c ^ d
                         : t < 60 ? (b & c) | (b & d) | (c & d) : b ^ c ^ d;
      const uint32_t k = t < 20 ? 0x5a827999u : t < 40 ? 0x6ed9eba1u : t < 60 ? 0x8f1bbcdcu : 0xca62c1d6u;
      const uint32_t tmp = rotl(a, 5) + f + e + k + w[t];
      e = d; d = c; c = rotl(b, 30); b = a; a = tmp;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e;
  }
}

// Four rounds of group G (rounds 4G .. 4G+3; the round function is G / 5) in the rolling form:
// m[G & 3] holds W[4G .. 4G+3] once sha1msg2 has finished it from the previous group's words;
// `esave` is ABCD from before the previous group (its rotated a is this group's e).
#define S3H_SHA1_GROUP(G)                                                                   \
  do {                                                                                      \
    if ((G) >= 4) m[(G) & 3] = _mm_sha1msg2_epu32(m[(G) & 3], m[((G) + 3) & 3]);            \
    const __m128i ecur = (G) == 0 ? _mm_add_epi32(e, m[0]) : _mm_sha1nexte_epu32(esave, m[(G) & 3]); \
    esave = abcd;                                                                           \
    abcd = _mm_sha1rnds4_epu32(abcd, ecur, (G) / 5);                                        \
    if ((G) >= 1 && (G) <= 16) m[((G) + 3) & 3] = _mm_sha1msg1_epu32(m[((G) + 3) & 3], m[(G) & 3]); \
    if ((G) >= 2 && (G) <= 17) m[((G) + 2) & 3] = _mm_xor_si128(m[((G) + 2) & 3], m[(G) & 3]); \
  } while (0)

__attribute__((target("sha,sse4.1,ssse3")))
void compress_shani(uint32_t st[5], const uint8_t *p, uint64_t nblk) {
  const __m128i bswap_mask = _mm_set_epi64x(0x0001020304050607ll, 0x08090a0b0c0d0e0fll);
  __m128i abcd = _mm_shuffle_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i *>(st)), 0x1B);
  __m128i e = _mm_set_epi32(int(st[4]), 0, 0, 0);
  for (; nblk; --nblk, p += 64) {
    const __m128i abcd_save = abcd, e_save = e;
    __m128i m[4], esave = abcd;
    for (int g = 0; g < 4; ++g)
      m[g] = _mm_shuffle_epi8(_mm_loadu_si128(reinterpret_cast<const __m128i *>(p + 16 * g)), bswap_mask);
    S3H_SHA1_GROUP(0);  S3H_SHA1_GROUP(1);  S3H_SHA1_GROUP(2);  S3H_SHA1_GROUP(3);
    S3H_SHA1_GROUP(4);  S3H_SHA1_GROUP(5);  S3H_SHA1_GROUP(6);  S3H_SHA1_GROUP(7);
    S3H_SHA1_GROUP(8);  S3H_SHA1_GROUP(9);  S3H_SHA1_GROUP(10); S3H_SHA1_GROUP(11);
    S3H_SHA1_GROUP(12); S3H_SHA1_GROUP(13); S3H_SHA1_GROUP(14); S3H_SHA1_GROUP(15);
    S3H_SHA1_GROUP(16); S3H_SHA1_GROUP(17); S3H_SHA1_GROUP(18); S3H_SHA1_GROUP(19);
    e = _mm_sha1nexte_epu32(esave, e_save);
    abcd = _mm_add_epi32(abcd, abcd_save);
  }
  _mm_storeu_si128(reinterpret_cast<__m128i *>(st), _mm_shuffle_epi32(abcd, 0x1B));
  st[4] = uint32_t(_mm_extract_epi32(e, 3));
}
#undef S3H_SHA1_GROUP

using CompressFn = void (*)(uint32_t *, const uint8_t *, uint64_t);

CompressFn pick_compress() {
  const char *force = std::getenv("S3H_CPU_SCALAR");
  if (force && force[0] == '1') return compress_scalar;
  unsigned a, b, c, d;
  if (!__get_cpuid(1, &a, &b, &c, &d)) return compress_scalar;
  const bool sse41 = c & (1u << 19), ssse3 = c & (1u << 9);
  if (!__get_cpuid_count(7, 0, &a, &b, &c, &d)) return compress_scalar;
  const bool sha = b & (1u << 29);
  return (sha && sse41 && ssse3) ? compress_shani : compress_scalar;
}

const CompressFn g_compress = pick_compress();

// RFC 4648 base64 with padding; writes 4 * ceil(n / 3) characters and a NUL.
void base64(const uint8_t *in, size_t n, char *out) {
  static const char tab[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  size_t o = 0;
  for (size_t i = 0; i < n; i += 3) {
    const uint32_t b0 = in[i], b1 = i + 1 < n ? in[i + 1] : 0, b2 = i + 2 < n ? in[i + 2] : 0;
    const uint32_t v = b0 << 16 | b1 << 8 | b2;
    out[o++] = tab[v >> 18];
    out[o++] = tab[(v >> 12) & 63];
    out[o++] = i + 1 < n ? tab[(v >> 6) & 63] : '=';
    out[o++] = i + 2 < n ? tab[v & 63] : '=';
  }
  out[o] = '\0';
}

}  // namespace

extern "C" {

void s3h_cpu_sha1(const uint8_t *data, uint64_t length, uint32_t hash[5]) {
  uint32_t st[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u};
  // whole blocks straight from the caller's buffer, then the one or two padded tail blocks
  const uint64_t whole = length / 64;
  g_compress(st, data, whole);
  uint8_t tail[128] = {0};
  const uint64_t rem = length - whole * 64;
  if (rem) std::memcpy(tail, data + whole * 64, rem);
  tail[rem] = 0x80;
  const uint64_t tb = rem < 56 ? 64 : 128;
  const uint64_t be = __builtin_bswap64(8 * length);
  std::memcpy(tail + tb - 8, &be, 8);
  g_compress(st, tail, tb / 64);
  for (int i = 0; i < 5; ++i) hash[i] = __builtin_bswap32(st[i]);
}

int s3h_digest_checksum_text(int algo, const uint32_t *digests, uint64_t n, int composite,
                             char *out, uint64_t out_len) {
  if (out && out_len) out[0] = '\0';
  if (algo != S3H_ALGO_SHA1 && algo != S3H_ALGO_SHA256)
    return fail(S3H_EINVAL, "digest checksum text: algorithm %d (SHA-1 and SHA-256 only; MD5 has "
                "s3h_multipart_etag)", algo);
  if (!out || out_len < S3H_DIGEST_CHECKSUM_MAX)
    return fail(S3H_EINVAL, "digest checksum text: need %d output bytes", S3H_DIGEST_CHECKSUM_MAX);
  if (!digests || n == 0) return fail(S3H_EINVAL, "digest checksum text: no digests");
  if (composite != 0 && composite != 1)
    return fail(S3H_EINVAL, "digest checksum text: composite must be 0 or 1");
  const size_t bytes = algo == S3H_ALGO_SHA1 ? 20 : 32;
  if (!composite) {
    if (n != 1) return fail(S3H_EINVAL, "digest checksum text: the plain form takes one digest (n=%llu)",
                            static_cast<unsigned long long>(n));
    base64(reinterpret_cast<const uint8_t *>(digests), bytes, out);
    return S3H_OK;
  }
  // composite: the same hash over the parts' raw digests concatenated (they are contiguous in
  // the batch entry points' output), then "-n"
  uint32_t h[8];
  const uint8_t *raw = reinterpret_cast<const uint8_t *>(digests);
  if (algo == S3H_ALGO_SHA1) s3h_cpu_sha1(raw, n * bytes, h);
  else s3h_cpu_sha256(raw, n * bytes, h);
  base64(reinterpret_cast<const uint8_t *>(h), bytes, out);
  const size_t len = std::strlen(out);  // 28 or 44 characters (S3 allows n <= 10,000: 6 more)
  std::snprintf(out + len, size_t(out_len - len), "-%llu", static_cast<unsigned long long>(n));
  return S3H_OK;
}

}  // extern "C"
