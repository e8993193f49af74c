// lib_chunk_sign.cpp -- CPU side of SigV4 chunk-signed uploads (aws-chunked bodies under
// x-amz-content-sha256: STREAMING-AWS4-HMAC-SHA256-PAYLOAD): the signing key, the chunk-signing
// context, the signature chain over ready chunk digests and the framing line of a chunk.
//
//   string_i = "AWS4-HMAC-SHA256-PAYLOAD\n" timestamp "\n" date/region/service/aws4_request "\n"
//              hex(sig_{i-1}) "\n" hex(sha256("")) "\n" hex(sha256(chunk_i))
//   sig_i    = HMAC-SHA256(signing_key, string_i),   sig_0 = the request's seed signature
//
// Everything before hex(sig_{i-1}) is constant (the prefix P), so the context hashes the key's
// ipad block and P's whole blocks once; a link is the 4 or 5 blocks that remain plus one outer
// block.  The compression is the drop-in's (SHA-NI or scalar, s3h_cpu_backend).
//
// The trailer variant (...-PAYLOAD-TRAILER) closes a part with a trailing checksum header and
//   trailer_sig = HMAC-SHA256(signing_key, P' hex(sig_last) "\n" hex(sha256(name ":" base64 "\n")))
// P' being P under the name AWS4-HMAC-SHA256-TRAILER: one more link, 3 or 4 inner blocks, from a
// midstate and a tail template of its own (chunk_sign.hpp).
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <new>
#include <thread>
#include <vector>

#include "../../../include/s3hash.h"
#include "../../../include/sha256.h"
#include "../chunk_sign.hpp"
#include "../status.hpp"
#include "cpu_hash.hpp"

namespace {

using s3h::host::fail;

// sha256("")
const uint8_t kEmptyDigest[32] = {0xe3, 0xb0, 0xc4, 0x42, 0x98, 0xfc, 0x1c, 0x14, 0x9a, 0xfb, 0xf4,
                                  0xc8, 0x99, 0x6f, 0xb9, 0x24, 0x27, 0xae, 0x41, 0xe4, 0x64, 0x9b,
                                  0x93, 0x4c, 0xa4, 0x95, 0x99, 0x1b, 0x78, 0x52, 0xb8, 0x55};

inline void put_hex(const uint8_t *bytes, size_t n, uint8_t *out) {
  static const char digits[] = "0123456789abcdef";
  for (size_t i = 0; i < n; ++i) {
    out[2 * i] = uint8_t(digits[bytes[i] >> 4]);
    out[2 * i + 1] = uint8_t(digits[bytes[i] & 15]);
  }
}

// HMAC from the midstates: `nblk` blocks of `tail` from the inner one, then the outer block.
void finish(const uint32_t istate[8], const uint32_t ostate[8], const uint8_t *tail, uint32_t nblk,
            uint8_t *sig) {
  uint32_t st[8];
  std::memcpy(st, istate, sizeof st);
  s3h::cpu::sha256_blocks(st, tail, nblk);
  uint8_t outer[64] = {0};
  for (int i = 0; i < 8; ++i) {
    const uint32_t be = __builtin_bswap32(st[i]);
    std::memcpy(outer + 4 * i, &be, 4);
  }
  outer[32] = 0x80;
  outer[62] = 0x03;  // (64 + 32) * 8 = 768 bits
  std::memcpy(st, ostate, sizeof st);
  s3h::cpu::sha256_blocks(st, outer, 1);
  for (int i = 0; i < 8; ++i) {
    const uint32_t be = __builtin_bswap32(st[i]);
    std::memcpy(sig + 4 * i, &be, 4);
  }
}

// One link: prev (32 raw bytes) and the chunk digest (32 raw bytes) -> sig (32 raw bytes).
void link(const s3h_chunk_sign_ctx_s *C, const uint8_t *prev, const uint8_t *digest, uint8_t *sig) {
  uint8_t tail[sizeof C->tail];
  std::memcpy(tail, C->tail, 64 * C->nblk);
  put_hex(prev, 32, tail + C->r);
  put_hex(digest, 32, tail + C->r + 130);
  finish(C->istate, C->ostate, tail, C->nblk, sig);
}

const s3h::TrailerKind kTrailerKinds[] = {{"x-amz-checksum-crc32c", 4, 8},
                                          {"x-amz-checksum-crc32", 4, 8},
                                          {"x-amz-checksum-crc64nvme", 8, 12},
                                          {"x-amz-checksum-sha1", 20, 28},
                                          {"x-amz-checksum-sha256", 32, 44}};
constexpr size_t kTrailerLineMax = 24 + 1 + 44 + 1;  // the longest name, ':', the longest text, '\n'

size_t base64(const uint8_t *in, size_t n, char *out) {
  static const char *const a = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  size_t o = 0;
  for (size_t i = 0; i < n; i += 3) {
    const size_t left = n - i;
    const uint32_t v = uint32_t(in[i]) << 16 | (left > 1 ? uint32_t(in[i + 1]) << 8 : 0) | (left > 2 ? in[i + 2] : 0);
    out[o++] = a[v >> 18];
    out[o++] = a[(v >> 12) & 63];
    out[o++] = left > 1 ? a[(v >> 6) & 63] : '=';
    out[o++] = left > 2 ? a[v & 63] : '=';
  }
  return o;
}

// "name:base64" of entry `at` of a values array (no line end, no NUL); returns its length.
// CRC values are numbers, sent as big-endian bytes; digest words are the digest's bytes in memory.
size_t trailer_line(const s3h::TrailerKind &K, const void *values, uint64_t at, char *out) {
  uint8_t be[32];
  if (K.value_len == 4) {
    const uint32_t v = __builtin_bswap32(static_cast<const uint32_t *>(values)[at]);
    std::memcpy(be, &v, 4);
  } else if (K.value_len == 8) {
    const uint64_t v = __builtin_bswap64(static_cast<const uint64_t *>(values)[at]);
    std::memcpy(be, &v, 8);
  } else {
    std::memcpy(be, static_cast<const uint8_t *>(values) + K.value_len * at, K.value_len);
  }
  const size_t name = std::strlen(K.name);
  std::memcpy(out, K.name, name);
  out[name] = ':';
  return name + 1 + base64(be, K.value_len, out + name + 1);
}

// The trailer link of one part: its checksum line hashed, then the HMAC over the trailer string.
void trailer_link(const s3h_chunk_sign_ctx_s *C, const s3h::TrailerKind &K, const void *values, uint64_t at,
                  const uint8_t *last, uint8_t *sig) {
  uint8_t line[128] = {0};  // one block, or two for a SHA-256 checksum
  size_t len = trailer_line(K, values, at, reinterpret_cast<char *>(line));
  line[len++] = '\n';
  line[len] = 0x80;
  const size_t blocks = (len + 9 + 63) / 64;
  line[64 * blocks - 2] = uint8_t((8 * len) >> 8);
  line[64 * blocks - 1] = uint8_t(8 * len);
  uint32_t st[8];
  sha256::init_hash(st);
  s3h::cpu::sha256_blocks(st, line, blocks);
  uint8_t digest[32];
  for (int i = 0; i < 8; ++i) {
    const uint32_t be = __builtin_bswap32(st[i]);
    std::memcpy(digest + 4 * i, &be, 4);
  }
  uint8_t tail[sizeof C->trailer_tail];
  std::memcpy(tail, C->trailer_tail, 64 * C->trailer_nblk);
  put_hex(last, 32, tail + C->r);
  put_hex(digest, 32, tail + C->r + 65);
  finish(C->trailer_istate, C->ostate, tail, C->trailer_nblk, sig);
}

inline uint64_t hexlen(uint64_t k) { return k == 0 ? 1 : uint64_t(64 - __builtin_clzll(k) + 3) / 4; }

// Wire length of the body of a part of `len` bytes: its framed data chunks, the final line and
// `ending` bytes ("\r\n" or the trailer text).
inline uint64_t body_length(uint64_t len, uint64_t chunk_bytes, uint64_t ending) {
  const uint64_t full = len / chunk_bytes, rem = len % chunk_bytes;
  return full * (hexlen(chunk_bytes) + 85 + chunk_bytes) + (rem ? hexlen(rem) + 85 + rem : 0) + 84 + ending;
}

// "<hex len>;chunk-signature=<64 hex>\r\n" at out (no NUL); returns its length.
size_t frame_line(uint64_t chunk_len, const uint8_t *sig, uint8_t *out) {
  char head[40];
  const int at = std::snprintf(head, sizeof head, "%llx;chunk-signature=", static_cast<unsigned long long>(chunk_len));
  std::memcpy(out, head, size_t(at));
  put_hex(sig, 32, out + at);
  out[at + 64] = '\r';
  out[at + 65] = '\n';
  return size_t(at) + 66;
}

// One part's body at out: `sigs` its data-chunk signatures and the final chunk's behind them.
void write_body(const uint8_t *part, uint64_t len, uint64_t chunk_bytes, const uint8_t *sigs,
                const s3h::TrailerKind *K, const void *values, uint64_t at, const uint8_t *trailer_sig,
                uint8_t *out) {
  uint64_t c = 0;
  for (uint64_t done = 0; done < len; ++c) {
    const uint64_t k = std::min(chunk_bytes, len - done);
    out += frame_line(k, sigs + 32 * c, out);
    std::memcpy(out, part + done, k);
    out[k] = '\r';
    out[k + 1] = '\n';
    out += k + 2;
    done += k;
  }
  out += frame_line(0, sigs + 32 * c, out);
  if (K) {
    out += trailer_line(*K, values, at, reinterpret_cast<char *>(out));
    std::memcpy(out, "\r\nx-amz-trailer-signature:", 26);
    put_hex(trailer_sig, 32, out + 26);
    out += 90;
  }
  std::memcpy(out, K ? "\r\n\r\n" : "\r\n", K ? 4 : 2);
}

void chain(const s3h_chunk_sign_ctx_s *C, const uint8_t *digests, uint64_t chunks, const uint8_t *seed,
           uint8_t *sigs) {
  const uint8_t *prev = seed;
  for (uint64_t c = 0; c <= chunks; ++c) {
    link(C, prev, c < chunks ? digests + 32 * c : kEmptyDigest, sigs + 32 * c);
    prev = sigs + 32 * c;
  }
}

}  // namespace

const s3h::TrailerKind *s3h::trailer_kind(int checksum) {
  return checksum >= 0 && checksum < int(sizeof kTrailerKinds / sizeof kTrailerKinds[0]) ? &kTrailerKinds[checksum]
                                                                                         : nullptr;
}

extern "C" {

int s3h_sigv4_signing_key(const char *secret, const char *date, const char *region,
                          const char *service, uint8_t key[32]) {
  if (!secret || !date || !region || !service || !key)
    return fail(S3H_EINVAL, "signing key: null argument");
  std::vector<uint8_t> k0(4 + std::strlen(secret));
  std::memcpy(k0.data(), "AWS4", 4);
  std::memcpy(k0.data() + 4, secret, k0.size() - 4);
  uint8_t a[32], b[32];
  s3h_cpu_hmac256(reinterpret_cast<const uint8_t *>(date), std::strlen(date), k0.data(), k0.size(), a);
  s3h_cpu_hmac256(reinterpret_cast<const uint8_t *>(region), std::strlen(region), a, 32, b);
  s3h_cpu_hmac256(reinterpret_cast<const uint8_t *>(service), std::strlen(service), b, 32, a);
  s3h_cpu_hmac256(reinterpret_cast<const uint8_t *>("aws4_request"), 12, a, 32, key);
  return S3H_OK;
}

int s3h_chunk_sign_ctx_create(const uint8_t key[32], const char *timestamp, const char *date,
                              const char *region, const char *service, s3h_chunk_sign_ctx_t *out) {
  if (!out) return fail(S3H_EINVAL, "chunk sign context: null out-pointer");
  *out = nullptr;
  if (!key || !timestamp || !date || !region || !service)
    return fail(S3H_EINVAL, "chunk sign context: null argument");
  const size_t nr = std::strlen(region), ns = std::strlen(service);
  if (std::strlen(timestamp) != 16) return fail(S3H_EINVAL, "chunk sign context: timestamp must be 16 bytes (YYYYMMDDThhmmssZ)");
  if (std::strlen(date) != 8) return fail(S3H_EINVAL, "chunk sign context: date must be 8 bytes (YYYYMMDD)");
  if (nr == 0 || ns == 0) return fail(S3H_EINVAL, "chunk sign context: empty region or service");
  if (66 + nr + ns > 256)
    return fail(S3H_EINVAL, "chunk sign context: prefix of %zu bytes (at most 256)", 66 + nr + ns);
  auto *C = new (std::nothrow) s3h_chunk_sign_ctx_s();
  if (!C) return fail(S3H_ENOMEM, "chunk sign context: out of memory");
  const int plen = std::snprintf(C->prefix, sizeof C->prefix, "AWS4-HMAC-SHA256-PAYLOAD\n%s\n%s/%s/%s/aws4_request",
                                 timestamp, date, region, service);
  C->prefix[plen] = '\n';  // |P| <= 256: the 256th byte has no room for snprintf's NUL
  C->prefix_len = uint32_t(plen) + 1;
  C->r = C->prefix_len % 64;
  C->nblk = (C->r + 203 + 63) / 64;

  // P': the same prefix under the trailer's algorithm name, 7 letters for 7 at byte 17
  char tprefix[sizeof C->prefix];
  std::memcpy(tprefix, C->prefix, C->prefix_len);
  std::memcpy(tprefix + 17, "TRAILER", 7);
  C->trailer_nblk = (C->r + 138 + 63) / 64;

  uint8_t pad[64];
  for (int i = 0; i < 64; ++i) pad[i] = uint8_t((i < 32 ? key[i] : 0) ^ 0x36);
  sha256::init_hash(C->istate);
  s3h::cpu::sha256_blocks(C->istate, pad, 1);
  std::memcpy(C->trailer_istate, C->istate, sizeof C->istate);
  s3h::cpu::sha256_blocks(C->istate, reinterpret_cast<const uint8_t *>(C->prefix), C->prefix_len / 64);
  s3h::cpu::sha256_blocks(C->trailer_istate, reinterpret_cast<const uint8_t *>(tprefix), C->prefix_len / 64);
  for (int i = 0; i < 64; ++i) pad[i] = uint8_t((i < 32 ? key[i] : 0) ^ 0x5c);
  sha256::init_hash(C->ostate);
  s3h::cpu::sha256_blocks(C->ostate, pad, 1);

  // the tail: P's last r bytes, [64 hex] '\n' hex(sha256("")) '\n' [64 hex], 0x80, zeros, bit length
  uint8_t *t = C->tail;
  std::memcpy(t, C->prefix + C->prefix_len - C->r, C->r);
  t[C->r + 64] = '\n';
  put_hex(kEmptyDigest, 32, t + C->r + 65);
  t[C->r + 129] = '\n';
  t[C->r + 194] = 0x80;
  const uint64_t be = __builtin_bswap64(8ull * (64 + C->prefix_len + 194));
  std::memcpy(t + 64 * C->nblk - 8, &be, 8);
  for (int j = 0; j < s3h::kChunkTailWords; ++j) {
    uint32_t w;
    std::memcpy(&w, t + 4 * j, 4);
    C->tail_words[j] = __builtin_bswap32(w);
  }
  // the trailer tail: its prefix's last r bytes, [64 hex] '\n' [64 hex], 0x80, zeros, bit length
  t = C->trailer_tail;
  std::memcpy(t, tprefix + C->prefix_len - C->r, C->r);
  t[C->r + 64] = '\n';
  t[C->r + 129] = 0x80;
  const uint64_t tbe = __builtin_bswap64(8ull * (64 + C->prefix_len + 129));
  std::memcpy(t + 64 * C->trailer_nblk - 8, &tbe, 8);
  for (int j = 0; j < s3h::kTrailerTailWords; ++j) {
    uint32_t w;
    std::memcpy(&w, t + 4 * j, 4);
    C->trailer_tail_words[j] = __builtin_bswap32(w);
  }
  *out = C;
  return S3H_OK;
}

int s3h_chunk_sign_ctx_destroy(s3h_chunk_sign_ctx_t ctx) {
  delete ctx;
  return S3H_OK;
}

int s3h_chunk_geometry(const uint64_t *lengths, uint64_t n, uint64_t chunk_bytes,
                       uint64_t *data_chunks_per_part, uint64_t *signature_offsets,
                       uint64_t *data_chunks, uint64_t *signatures, uint64_t *max_chunks_per_part) {
  if (!lengths || n == 0 || n > (1ull << 31)) return fail(S3H_EINVAL, "chunk geometry: need 1 .. 2^31 parts");
  if (chunk_bytes == 0) return fail(S3H_EINVAL, "chunk geometry: chunk_bytes must be at least 1");
  uint64_t total = 0, longest = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t c = lengths[i] / chunk_bytes + (lengths[i] % chunk_bytes != 0);
    if (c > (1ull << 31) || total + c > (1ull << 31))
      return fail(S3H_EINVAL, "chunk geometry: more than 2^31 data chunks");
    if (data_chunks_per_part) data_chunks_per_part[i] = c;
    if (signature_offsets) signature_offsets[i] = total + i;
    total += c;
    longest = std::max(longest, c);
  }
  if (data_chunks) *data_chunks = total;
  if (signatures) *signatures = total + n;
  if (max_chunks_per_part) *max_chunks_per_part = longest;
  return S3H_OK;
}

int s3h_cpu_chunk_signatures(s3h_chunk_sign_ctx_t ctx, const uint32_t *chunk_digests,
                             const uint64_t *data_chunks_per_part, uint64_t n, const uint32_t *seeds,
                             uint32_t *signatures) {
  if (!ctx || !data_chunks_per_part || !seeds || !signatures || n == 0)
    return fail(S3H_EINVAL, "chunk signatures: null argument or no parts");
  std::vector<uint64_t> first(n + 1, 0);
  for (uint64_t i = 0; i < n; ++i) first[i + 1] = first[i] + data_chunks_per_part[i];
  if (first[n] != 0 && !chunk_digests) return fail(S3H_EINVAL, "chunk signatures: null chunk digests");
  const uint8_t *dig = reinterpret_cast<const uint8_t *>(chunk_digests);
  const uint8_t *seed = reinterpret_cast<const uint8_t *>(seeds);
  uint8_t *sig = reinterpret_cast<uint8_t *>(signatures);
  std::atomic<uint64_t> next{0};
  auto work = [&] {
    for (uint64_t i; (i = next.fetch_add(1)) < n;)
      chain(ctx, dig + 32 * first[i], data_chunks_per_part[i], seed + 32 * i, sig + 32 * (first[i] + i));
  };
  int cpus = 1;
  s3h_host_threads(1, &cpus);
  // a thread per 64 links at least: starting one costs about as much as that many links
  const uint64_t links = first[n] + n;
  const unsigned t = unsigned(std::min<uint64_t>({uint64_t(std::max(1, cpus)), n, (links + 63) / 64}));
  std::vector<std::thread> pool;
  try {
    for (unsigned k = 1; k < t; ++k) pool.emplace_back(work);
  } catch (const std::exception &) {  // fewer threads: the ones started and this one finish
  }
  work();
  for (auto &th : pool) th.join();
  return S3H_OK;
}

int s3h_chunk_header_text(uint64_t chunk_len, const uint32_t sig[8], char *out, uint64_t out_len) {
  if (out && out_len) out[0] = '\0';
  if (!sig || !out || out_len < S3H_CHUNK_HEADER_MAX)
    return fail(S3H_EINVAL, "chunk header text: need a signature and %d output bytes", S3H_CHUNK_HEADER_MAX);
  int at = std::snprintf(out, size_t(out_len), "%llx;chunk-signature=", static_cast<unsigned long long>(chunk_len));
  put_hex(reinterpret_cast<const uint8_t *>(sig), 32, reinterpret_cast<uint8_t *>(out) + at);
  std::memcpy(out + at + 64, "\r\n", 3);
  return S3H_OK;
}

int s3h_chunk_body_geometry(const uint64_t *lengths, uint64_t n, uint64_t chunk_bytes, int checksum,
                            uint64_t *body_lengths, uint64_t *body_offsets, uint64_t *total) {
  const s3h::TrailerKind *K = s3h::trailer_kind(checksum);
  if (checksum != -1 && !K) return fail(S3H_EINVAL, "chunk body geometry: unknown checksum %d", checksum);
  if (int rc = s3h_chunk_geometry(lengths, n, chunk_bytes, nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
  // the ending: "\r\n", or the trailer text (name ':' text, 26 + 64 bytes of signature line, two line ends)
  const uint64_t ending = K ? std::strlen(K->name) + 1 + K->text_len + 94 : 2;
  uint64_t sum = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t b = body_length(lengths[i], chunk_bytes, ending);
    if (body_lengths) body_lengths[i] = b;
    if (body_offsets) body_offsets[i] = sum;
    sum += b;
  }
  if (total) *total = sum;
  return S3H_OK;
}

int s3h_cpu_chunk_body(const uint8_t *const *parts, const uint64_t *lengths, uint64_t n, uint64_t chunk_bytes,
                       const uint32_t *signatures, int checksum, const void *values,
                       const uint32_t *trailer_signatures, uint8_t *body, const uint64_t *body_offsets) {
  const s3h::TrailerKind *K = s3h::trailer_kind(checksum);
  if (checksum != -1 && !K) return fail(S3H_EINVAL, "chunk body: unknown checksum %d", checksum);
  if (!parts || !lengths || !signatures || !body) return fail(S3H_EINVAL, "chunk body: null argument");
  if ((K != nullptr) != (values != nullptr) || (K != nullptr) != (trailer_signatures != nullptr))
    return fail(S3H_EINVAL, "chunk body: checksum values and trailer signatures go with a checksum kind, and only with one");
  std::vector<uint64_t> sig(n ? n : 1), packed(n ? n : 1);
  uint64_t total = 0;
  if (int rc = s3h_chunk_geometry(lengths, n, chunk_bytes, nullptr, sig.data(), nullptr, nullptr, nullptr)) return rc;
  if (int rc = s3h_chunk_body_geometry(lengths, n, chunk_bytes, checksum, nullptr, packed.data(), &total)) return rc;
  for (uint64_t i = 0; i < n; ++i)
    if (lengths[i] && !parts[i]) return fail(S3H_EINVAL, "chunk body: part %llu is null", (unsigned long long)i);
  const uint64_t *at = body_offsets ? body_offsets : packed.data();
  const uint8_t *sigs = reinterpret_cast<const uint8_t *>(signatures);
  const uint8_t *tsig = reinterpret_cast<const uint8_t *>(trailer_signatures);
  std::atomic<uint64_t> next{0};
  auto work = [&] {
    for (uint64_t i; (i = next.fetch_add(1)) < n;)
      write_body(parts[i], lengths[i], chunk_bytes, sigs + 32 * sig[i], K, values, i, K ? tsig + 32 * i : nullptr,
                 body + at[i]);
  };
  int cpus = 1;
  s3h_host_threads(1, &cpus);
  // a thread per MiB at least: starting one costs about as much as copying that
  const unsigned t = unsigned(std::min<uint64_t>({uint64_t(std::max(1, cpus)), n, (total >> 20) + 1}));
  std::vector<std::thread> pool;
  try {
    for (unsigned k = 1; k < t; ++k) pool.emplace_back(work);
  } catch (const std::exception &) {  // fewer threads: the ones started and this one finish
  }
  work();
  for (auto &th : pool) th.join();
  return S3H_OK;
}

int s3h_cpu_trailer_signatures(s3h_chunk_sign_ctx_t ctx, int checksum, const void *values,
                               const uint32_t *last_signatures, uint64_t n, uint32_t *trailer_signatures) {
  const s3h::TrailerKind *K = s3h::trailer_kind(checksum);
  if (!K) return fail(S3H_EINVAL, "trailer signatures: unknown checksum %d", checksum);
  if (!ctx || !values || !last_signatures || !trailer_signatures || n == 0)
    return fail(S3H_EINVAL, "trailer signatures: null argument or no parts");
  const uint8_t *last = reinterpret_cast<const uint8_t *>(last_signatures);
  uint8_t *sig = reinterpret_cast<uint8_t *>(trailer_signatures);
  std::atomic<uint64_t> next{0};
  auto work = [&] {  // 64 parts a turn: one link each
    for (uint64_t i; (i = next.fetch_add(64)) < n;)
      for (uint64_t k = i; k < std::min(n, i + 64); ++k) trailer_link(ctx, *K, values, k, last + 32 * k, sig + 32 * k);
  };
  int cpus = 1;
  s3h_host_threads(1, &cpus);
  const unsigned t = unsigned(std::min<uint64_t>(uint64_t(std::max(1, cpus)), (n + 63) / 64));
  std::vector<std::thread> pool;
  try {
    for (unsigned k = 1; k < t; ++k) pool.emplace_back(work);
  } catch (const std::exception &) {  // fewer threads: the ones started and this one finish
  }
  work();
  for (auto &th : pool) th.join();
  return S3H_OK;
}

int s3h_trailer_line_text(int checksum, const void *value, char *out, uint64_t out_len) {
  if (out && out_len) out[0] = '\0';
  const s3h::TrailerKind *K = s3h::trailer_kind(checksum);
  if (!K) return fail(S3H_EINVAL, "trailer line text: unknown checksum %d", checksum);
  if (!value || !out || out_len < S3H_TRAILER_LINE_MAX)
    return fail(S3H_EINVAL, "trailer line text: need a value and %d output bytes", S3H_TRAILER_LINE_MAX);
  static_assert(kTrailerLineMax < S3H_TRAILER_LINE_MAX, "the longest line and its NUL fit");
  out[trailer_line(*K, value, 0, out)] = '\0';
  return S3H_OK;
}

int s3h_chunk_trailer_text(int checksum, const void *value, const uint32_t trailer_sig[8], char *out,
                           uint64_t out_len) {
  if (out && out_len) out[0] = '\0';
  const s3h::TrailerKind *K = s3h::trailer_kind(checksum);
  if (!K) return fail(S3H_EINVAL, "chunk trailer text: unknown checksum %d", checksum);
  if (!value || !trailer_sig || !out || out_len < S3H_CHUNK_TRAILER_MAX)
    return fail(S3H_EINVAL, "chunk trailer text: need a value, a signature and %d output bytes",
                S3H_CHUNK_TRAILER_MAX);
  static_assert(kTrailerLineMax + 2 + 24 + 64 + 2 + 2 < S3H_CHUNK_TRAILER_MAX, "the longest trailer and its NUL fit");
  size_t at = trailer_line(*K, value, 0, out);
  std::memcpy(out + at, "\r\nx-amz-trailer-signature:", 26);
  at += 26;
  put_hex(reinterpret_cast<const uint8_t *>(trailer_sig), 32, reinterpret_cast<uint8_t *>(out) + at);
  std::memcpy(out + at + 64, "\r\n\r\n", 5);
  return S3H_OK;
}

}  // extern "C"
