// include/s3hash_batch.hpp -- C++ convenience layer over the C-ABI (include/s3hash.h) in the
// same `namespace sha256` as the lib/hash drop-in, for C++ callers such as the parallel
// upload (the reference's lib/src/upload.cpp:89-110 insertion point).  Header-only; every
// call goes to the GPU through libs3hash.so and throws on error (no CPU fallback) -- unless
// the caller passes Route::cpu or Route::automatic to payload_hashes / file_part_hashes.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "s3hash.h"
#include "sha256.h"

namespace sha256 {

struct batch_error : std::runtime_error {
  int code;
  batch_error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

inline void batch_check(int rc) {
  if (rc != S3H_OK) throw batch_error(rc, std::string("s3hash: ") + s3h_last_error());
}

// Digests of host-resident parts on the GPUs (0 = all visible devices), one uint32_t[8] per
// part in lib/hash's layout (hash[i] = bswap32(H_i)).
inline std::vector<uint32_t> sha256_batch(const std::vector<const uint8_t*>& parts,
                                          const std::vector<uint64_t>& lengths,
                                          int ndevices = 0, uint64_t slice_bytes = 0) {
  if (parts.size() != lengths.size()) throw std::invalid_argument("parts/lengths size mismatch");
  std::vector<uint32_t> out(8 * parts.size());
  if (!parts.empty())
    batch_check(s3h_sha256_batch_host(parts.data(), lengths.data(), parts.size(), out.data(),
                                      ndevices, slice_bytes));
  return out;
}

// Parts already in device memory at d_base + offsets[i]; digests written to d_digests.
inline void sha256_batch_device(int device, const void* d_base,
                                const std::vector<uint64_t>& offsets,
                                const std::vector<uint64_t>& lengths, uint32_t* d_digests,
                                void* stream = nullptr) {
  batch_check(s3h_sha256_batch_device(device, d_base, offsets.data(), lengths.data(),
                                      offsets.size(), d_digests, stream));
}

// Where a host batch is hashed (include/s3hash.h "size-aware routing"): gpu = the batched GPU
// path (default), cpu = the lib/hash drop-in on host threads, split = both at once (the
// longest parts on the CPU, the rest on the GPU), automatic = whichever a model measured once
// per process estimates to finish first (needs a GPU; never a fallback).
enum class Route { gpu = S3H_ROUTE_GPU, cpu = S3H_ROUTE_CPU, automatic = S3H_ROUTE_AUTO, split = S3H_ROUTE_SPLIT };

inline std::vector<std::string> to_hex(const std::vector<uint32_t>& d) {
  std::vector<std::string> out(d.size() / 8);
  for (size_t i = 0; i < out.size(); ++i) {
    char t[65];
    hash_to_text(const_cast<uint32_t*>(&d[8 * i]), t);
    out[i] = t;
  }
  return out;
}

// AUTO's decision for a batch of parts of `lengths` without running it (s3h_route_rates,
// measured on first use and kept current by routed calls, + s3h_route_choose): Route::gpu,
// Route::cpu or Route::split, and the GPU / CPU estimates.  `digests` is what the caller will
// compute (S3H_DIGESTS_SHA256, or S3H_DIGESTS_BOTH for Content-MD5 + x-amz-content-sha256: the
// CPU side is then priced at the MD5 + SHA-256 rate), `source` where the parts are
// (S3H_SOURCE_PINNED / _PAGEABLE / _FILE).  An uploader that hashes per job decides once for
// the whole upload with this, then hashes each job's parts on that route.
inline Route choose_route(const std::vector<uint64_t>& lengths, int ndevices = 0,
                          double* gpu_s = nullptr, double* cpu_s = nullptr,
                          int digests = S3H_DIGESTS_SHA256, int source = S3H_SOURCE_PINNED) {
  if (lengths.empty()) throw std::invalid_argument("choose_route: no parts");
  s3h_route_rates_t r{};
  r.size = sizeof r;
  batch_check(s3h_route_rates(&r));
  s3h_route_choice_t c{};
  batch_check(s3h_route_choose(&r, digests, lengths.data(), lengths.size(), ndevices, source, &c));
  if (gpu_s) *gpu_s = c.gpu_s;
  if (cpu_s) *cpu_s = c.cpu_s;
  return Route(c.route);
}

// 64-char lowercase hex per part: the `payloadHash` strings S3Api::UploadFilePart takes
// (lib/include/s3-api.h:447-452).  *taken (if non-null) receives the route that ran.
inline std::vector<std::string> payload_hashes(const std::vector<const uint8_t*>& parts,
                                               const std::vector<uint64_t>& lengths,
                                               int ndevices = 0, Route route = Route::gpu,
                                               Route* taken = nullptr) {
  if (parts.size() != lengths.size()) throw std::invalid_argument("parts/lengths size mismatch");
  if (route == Route::gpu) {
    if (taken) *taken = Route::gpu;
    return to_hex(sha256_batch(parts, lengths, ndevices));
  }
  std::vector<uint32_t> d(8 * parts.size());
  int t = S3H_ROUTE_GPU;
  if (!parts.empty())
    batch_check(s3h_sha256_batch_routed(parts.data(), lengths.data(), parts.size(), d.data(),
                                        ndevices, int(route), &t));
  if (taken) *taken = Route(t);
  return to_hex(d);
}

// Digests of byte ranges of a file -- the (file, offset, size) parts UploadFilePart sends --
// read by host threads straight into pinned staging (s3h_sha256_file_parts), as hex.
inline std::vector<std::string> file_part_hashes(const std::string& path,
                                                 const std::vector<uint64_t>& offsets,
                                                 const std::vector<uint64_t>& lengths,
                                                 int ndevices = 0, Route route = Route::gpu,
                                                 Route* taken = nullptr) {
  if (offsets.size() != lengths.size()) throw std::invalid_argument("offsets/lengths size mismatch");
  std::vector<uint32_t> d(8 * offsets.size());
  int t = S3H_ROUTE_GPU;
  if (!offsets.empty() && route == Route::gpu)
    batch_check(s3h_sha256_file_parts(path.c_str(), offsets.data(), lengths.data(), offsets.size(),
                                      d.data(), ndevices, 0));
  else if (!offsets.empty())
    batch_check(s3h_sha256_file_parts_routed(path.c_str(), offsets.data(), lengths.data(),
                                             offsets.size(), d.data(), ndevices, int(route), &t));
  if (taken) *taken = Route(t);
  return to_hex(d);
}

// Release the host path's cached per-device buffers (s3h_trim).
inline void trim() { batch_check(s3h_trim()); }

// Both upload headers per part from one pass (s3h_sha256_md5_batch_host): `sha256` gets the
// x-amz-content-sha256 hex, `md5` the 16 digest bytes of Content-MD5 (base64 them for the
// header) -- the replacement for one sha256::sha256 + one md5::md5 call per part.
struct DualDigests {
  std::vector<uint32_t> sha256;  // 8 words per part, lib/hash layout
  std::vector<uint32_t> md5;     // 4 words per part, digest bytes in memory order
};
inline DualDigests sha256_md5_batch(const std::vector<const uint8_t*>& parts,
                                    const std::vector<uint64_t>& lengths, int ndevices = 0,
                                    uint64_t slice_bytes = 0) {
  if (parts.size() != lengths.size()) throw std::invalid_argument("parts/lengths size mismatch");
  DualDigests d{std::vector<uint32_t>(8 * parts.size()), std::vector<uint32_t>(4 * parts.size())};
  if (!parts.empty())
    batch_check(s3h_sha256_md5_batch_host(parts.data(), lengths.data(), parts.size(),
                                          d.sha256.data(), d.md5.data(), ndevices, slice_bytes));
  return d;
}

// The same for (file, offset, size) parts (s3h_sha256_md5_file_parts): each slice is read once.
inline DualDigests file_part_sha256_md5(const std::string& path, const std::vector<uint64_t>& offsets,
                                        const std::vector<uint64_t>& lengths, int ndevices = 0) {
  if (offsets.size() != lengths.size()) throw std::invalid_argument("offsets/lengths size mismatch");
  DualDigests d{std::vector<uint32_t>(8 * offsets.size()), std::vector<uint32_t>(4 * offsets.size())};
  if (!offsets.empty())
    batch_check(s3h_sha256_md5_file_parts(path.c_str(), offsets.data(), lengths.data(),
                                          offsets.size(), d.sha256.data(), d.md5.data(), ndevices, 0));
  return d;
}

// Both digests on a route (s3h_sha256_md5_batch_routed / s3h_sha256_md5_file_parts_routed):
// Route::gpu = the one-grid dual pass, Route::cpu = SHA-256 + MD5 per part in one pass over
// memory on the host threads, Route::split = the longest parts on the CPU while the GPU hashes
// the rest, Route::automatic = the model's pick for both digests.  *taken: the route that ran.
inline DualDigests sha256_md5_routed(const std::vector<const uint8_t*>& parts,
                                     const std::vector<uint64_t>& lengths, int ndevices = 0,
                                     Route route = Route::automatic, Route* taken = nullptr) {
  if (parts.size() != lengths.size()) throw std::invalid_argument("parts/lengths size mismatch");
  DualDigests d{std::vector<uint32_t>(8 * parts.size()), std::vector<uint32_t>(4 * parts.size())};
  int t = int(route);
  if (!parts.empty())
    batch_check(s3h_sha256_md5_batch_routed(parts.data(), lengths.data(), parts.size(), d.sha256.data(),
                                            d.md5.data(), ndevices, int(route), &t));
  if (taken) *taken = Route(t);
  return d;
}
inline DualDigests file_part_sha256_md5_routed(const std::string& path, const std::vector<uint64_t>& offsets,
                                               const std::vector<uint64_t>& lengths, int ndevices = 0,
                                               Route route = Route::automatic, Route* taken = nullptr) {
  if (offsets.size() != lengths.size()) throw std::invalid_argument("offsets/lengths size mismatch");
  DualDigests d{std::vector<uint32_t>(8 * offsets.size()), std::vector<uint32_t>(4 * offsets.size())};
  int t = int(route);
  if (!offsets.empty())
    batch_check(s3h_sha256_md5_file_parts_routed(path.c_str(), offsets.data(), lengths.data(), offsets.size(),
                                                 d.sha256.data(), d.md5.data(), ndevices, int(route), &t));
  if (taken) *taken = Route(t);
  return d;
}

// Download-side check (s3h_verify_batch_host): true for every part whose SHA-256 differs from
// the expected hex digest (the x-amz-content-sha256 it was uploaded with).
inline std::vector<bool> verify_payloads(const std::vector<const uint8_t*>& parts,
                                         const std::vector<uint64_t>& lengths,
                                         const std::vector<std::string>& expected_hex,
                                         int ndevices = 0) {
  if (parts.size() != lengths.size() || parts.size() != expected_hex.size())
    throw std::invalid_argument("parts/lengths/expected size mismatch");
  std::vector<uint32_t> want(8 * parts.size());
  auto nibble = [](char c) -> int {
    return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10
           : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
  };
  for (size_t i = 0; i < parts.size(); ++i) {
    const std::string& h = expected_hex[i];
    // exactly 64 hex digits: no sign, whitespace or prefix is accepted
    bool ok = h.size() == 64;
    for (size_t k = 0; ok && k < 64; ++k) ok = nibble(h[k]) >= 0;
    if (!ok)
      throw std::invalid_argument("verify_payloads: expected digest of part " + std::to_string(i) +
                                  " is not 64 hex digits: \"" + h + "\"");
    uint8_t* w = reinterpret_cast<uint8_t*>(&want[8 * i]);
    for (int b = 0; b < 32; ++b) w[b] = uint8_t(nibble(h[2 * b]) << 4 | nibble(h[2 * b + 1]));
  }
  std::vector<uint8_t> bad(parts.size());
  uint64_t count = 0;
  if (!parts.empty())
    batch_check(s3h_verify_batch_host(S3H_ALGO_SHA256, parts.data(), lengths.data(), parts.size(),
                                      want.data(), bad.data(), &count, ndevices));
  return std::vector<bool>(bad.begin(), bad.end());
}

// n objects hashed as their bodies arrive (s3h_stream_*): append() one chunk per object
// (any length, 0 allowed), finish() -> n digests of everything appended since the last
// finish(), after which the object restarts with n empty messages.  The batched, on-device
// form of sha256_stream + the documented sha256_next contract (sha256.h:73-97).
class stream_batch {
 public:
  explicit stream_batch(uint64_t n, int device = 0, int algo = S3H_ALGO_SHA256)
      : n_(n), words_(algo == S3H_ALGO_MD5 ? 4 : 8) {
    batch_check(s3h_stream_create(device, algo, n, S3H_KERNEL_AUTO, &s_));
  }
  ~stream_batch() { s3h_stream_destroy(s_); }
  stream_batch(const stream_batch&) = delete;
  stream_batch& operator=(const stream_batch&) = delete;

  void append(const std::vector<const uint8_t*>& chunks, const std::vector<uint64_t>& lengths) {
    if (chunks.size() != n_ || lengths.size() != n_)
      throw std::invalid_argument("stream_batch: one chunk per object");
    batch_check(s3h_stream_update_host(s_, chunks.data(), lengths.data()));
  }
  std::vector<uint32_t> finish() {
    std::vector<uint32_t> out(words_ * n_);
    batch_check(s3h_stream_final_host(s_, out.data()));
    return out;
  }
  std::vector<std::string> finish_hex() {
    const std::vector<uint32_t> d = finish();
    std::vector<std::string> out(n_);
    static const char* hexd = "0123456789abcdef";
    for (uint64_t i = 0; i < n_; ++i) {
      const uint8_t* b = reinterpret_cast<const uint8_t*>(&d[words_ * i]);
      for (uint32_t k = 0; k < 4 * words_; ++k) {
        out[i] += hexd[b[k] >> 4];
        out[i] += hexd[b[k] & 15];
      }
    }
    return out;
  }
  uint64_t size() const { return n_; }

 private:
  s3h_stream_t s_ = nullptr;
  uint64_t n_;
  uint32_t words_;
};

}  // namespace sha256

namespace md5 {

// The multipart ETag an S3 endpoint returns from CompleteMultipartUpload
// (lib/src/api/multipart_upload.cpp:162-183), from the parts' MD5 digests in part order
// (4 words per part, as DualDigests::md5 / s3h_md5_batch_* return them): s3h_multipart_etag.
inline std::string multipart_etag(const std::vector<uint32_t>& part_md5s) {
  if (part_md5s.empty() || part_md5s.size() % 4)
    throw std::invalid_argument("multipart_etag: need 4 words per part and at least one part");
  char out[S3H_ETAG_MAX];
  sha256::batch_check(s3h_multipart_etag(part_md5s.data(), part_md5s.size() / 4, out, sizeof out));
  return out;
}

}  // namespace md5

// S3 "additional checksums" (x-amz-checksum-crc32c / x-amz-checksum-crc32): `algo` is
// S3H_CRC32C or S3H_CRC32, every value the CRC's number (one uint32_t per part).
namespace crc {

// Parts already in device memory at d_base + offsets[i] (any alignment); n CRCs to d_crcs.
inline void crc_batch_device(int device, int algo, const void* d_base,
                             const std::vector<uint64_t>& offsets,
                             const std::vector<uint64_t>& lengths, uint32_t* d_crcs,
                             void* stream = nullptr) {
  if (offsets.size() != lengths.size()) throw std::invalid_argument("offsets/lengths size mismatch");
  sha256::batch_check(s3h_crc_batch_device(device, algo, d_base, offsets.data(), lengths.data(),
                                           offsets.size(), d_crcs, stream));
}

// Host-resident parts on the GPUs (s3h_crc_batch_host): one CRC per part.
inline std::vector<uint32_t> crc_batch(int algo, const std::vector<const uint8_t*>& parts,
                                       const std::vector<uint64_t>& lengths, int ndevices = 0,
                                       uint64_t slice_bytes = 0) {
  if (parts.size() != lengths.size()) throw std::invalid_argument("parts/lengths size mismatch");
  std::vector<uint32_t> crcs(parts.size());
  if (!parts.empty())
    sha256::batch_check(s3h_crc_batch_host(algo, parts.data(), lengths.data(), parts.size(), crcs.data(),
                                           ndevices, slice_bytes));
  return crcs;
}

// x-amz-content-sha256 and x-amz-checksum-crc32c / -crc32 per part from one pass over the host
// link (s3h_sha256_crc_batch_host / s3h_sha256_crc_file_parts).
struct Sha256Crc {
  std::vector<uint32_t> sha256;  // 8 words per part, lib/hash layout
  std::vector<uint32_t> crc;     // one value per part
};
inline Sha256Crc sha256_crc_batch(int algo, const std::vector<const uint8_t*>& parts,
                                  const std::vector<uint64_t>& lengths, int ndevices = 0,
                                  uint64_t slice_bytes = 0) {
  if (parts.size() != lengths.size()) throw std::invalid_argument("parts/lengths size mismatch");
  Sha256Crc d{std::vector<uint32_t>(8 * parts.size()), std::vector<uint32_t>(parts.size())};
  if (!parts.empty())
    sha256::batch_check(s3h_sha256_crc_batch_host(algo, parts.data(), lengths.data(), parts.size(),
                                                  d.sha256.data(), d.crc.data(), ndevices, slice_bytes));
  return d;
}

inline Sha256Crc file_part_sha256_crc(int algo, const std::string& path,
                                      const std::vector<uint64_t>& offsets,
                                      const std::vector<uint64_t>& lengths, int ndevices = 0) {
  if (offsets.size() != lengths.size()) throw std::invalid_argument("offsets/lengths size mismatch");
  Sha256Crc d{std::vector<uint32_t>(8 * offsets.size()), std::vector<uint32_t>(offsets.size())};
  if (!offsets.empty())
    sha256::batch_check(s3h_sha256_crc_file_parts(algo, path.c_str(), offsets.data(), lengths.data(),
                                                  offsets.size(), d.sha256.data(), d.crc.data(), ndevices, 0));
  return d;
}

// One message on the CPU; `seed` = a previous call's result (chunks chain like zlib's).
inline uint32_t crc(int algo, const uint8_t* data, uint64_t length, uint32_t seed = 0) {
  if (algo != S3H_CRC32C && algo != S3H_CRC32) throw std::invalid_argument("crc: unknown checksum");
  return s3h_cpu_crc(algo, data, length, seed);
}

inline uint32_t combine(int algo, uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  uint32_t out = 0;
  sha256::batch_check(s3h_crc_combine(algo, crc_a, crc_b, len_b, &out));
  return out;
}

// The FULL_OBJECT checksum of a multipart upload from its parts' CRCs and lengths.
inline uint32_t object_crc(int algo, const std::vector<uint32_t>& part_crcs,
                           const std::vector<uint64_t>& lengths) {
  if (part_crcs.size() != lengths.size()) throw std::invalid_argument("crcs/lengths size mismatch");
  uint32_t out = 0;
  sha256::batch_check(s3h_crc_object(algo, part_crcs.data(), lengths.data(), part_crcs.size(), &out));
  return out;
}

// Header value of one CRC (a part's, or object_crc's result): base64 of its big-endian bytes.
inline std::string checksum_text(int algo, uint32_t value) {
  char out[S3H_CHECKSUM_MAX];
  sha256::batch_check(s3h_checksum_text(algo, &value, 1, 0, out, sizeof out));
  return out;
}

// The COMPOSITE checksum of a multipart upload: "<base64>-<parts>".
inline std::string composite_checksum_text(int algo, const std::vector<uint32_t>& part_crcs) {
  char out[S3H_CHECKSUM_MAX];
  sha256::batch_check(s3h_checksum_text(algo, part_crcs.data(), part_crcs.size(), 1, out, sizeof out));
  return out;
}

}  // namespace crc

// x-amz-checksum-crc64nvme (CRC-64/NVME): every value the CRC's number, one uint64_t per part.
// S3 offers this checksum as FULL_OBJECT only: fold the parts' values with object_crc.
namespace crc64 {

// Parts already in device memory at d_base + offsets[i] (any alignment); n CRCs to d_crcs.
inline void crc_batch_device(int device, const void* d_base, const std::vector<uint64_t>& offsets,
                             const std::vector<uint64_t>& lengths, uint64_t* d_crcs,
                             void* stream = nullptr) {
  if (offsets.size() != lengths.size()) throw std::invalid_argument("offsets/lengths size mismatch");
  sha256::batch_check(s3h_crc64nvme_batch_device(device, d_base, offsets.data(), lengths.data(),
                                                 offsets.size(), d_crcs, stream));
}

// Host-resident parts on the GPUs (s3h_crc64nvme_batch_host): one CRC per part.
inline std::vector<uint64_t> crc_batch(const std::vector<const uint8_t*>& parts,
                                       const std::vector<uint64_t>& lengths, int ndevices = 0,
                                       uint64_t slice_bytes = 0) {
  if (parts.size() != lengths.size()) throw std::invalid_argument("parts/lengths size mismatch");
  std::vector<uint64_t> crcs(parts.size());
  if (!parts.empty())
    sha256::batch_check(s3h_crc64nvme_batch_host(parts.data(), lengths.data(), parts.size(), crcs.data(),
                                                 ndevices, slice_bytes));
  return crcs;
}

// x-amz-content-sha256 and x-amz-checksum-crc64nvme per part from one pass over the host link.
struct Sha256Crc64 {
  std::vector<uint32_t> sha256;  // 8 words per part, lib/hash layout
  std::vector<uint64_t> crc;     // one value per part
};
inline Sha256Crc64 sha256_crc_batch(const std::vector<const uint8_t*>& parts,
                                    const std::vector<uint64_t>& lengths, int ndevices = 0,
                                    uint64_t slice_bytes = 0) {
  if (parts.size() != lengths.size()) throw std::invalid_argument("parts/lengths size mismatch");
  Sha256Crc64 d{std::vector<uint32_t>(8 * parts.size()), std::vector<uint64_t>(parts.size())};
  if (!parts.empty())
    sha256::batch_check(s3h_sha256_crc64nvme_batch_host(parts.data(), lengths.data(), parts.size(),
                                                        d.sha256.data(), d.crc.data(), ndevices,
                                                        slice_bytes));
  return d;
}

inline Sha256Crc64 file_part_sha256_crc(const std::string& path, const std::vector<uint64_t>& offsets,
                                        const std::vector<uint64_t>& lengths, int ndevices = 0) {
  if (offsets.size() != lengths.size()) throw std::invalid_argument("offsets/lengths size mismatch");
  Sha256Crc64 d{std::vector<uint32_t>(8 * offsets.size()), std::vector<uint64_t>(offsets.size())};
  if (!offsets.empty())
    sha256::batch_check(s3h_sha256_crc64nvme_file_parts(path.c_str(), offsets.data(), lengths.data(),
                                                        offsets.size(), d.sha256.data(), d.crc.data(),
                                                        ndevices, 0));
  return d;
}

// One message on the CPU; `seed` = a previous call's result (chunks chain).
inline uint64_t crc(const uint8_t* data, uint64_t length, uint64_t seed = 0) {
  if (!data && length) throw std::invalid_argument("crc64: null data");
  return s3h_cpu_crc64nvme(data, length, seed);
}

inline uint64_t combine(uint64_t crc_a, uint64_t crc_b, uint64_t len_b) {
  uint64_t out = 0;
  sha256::batch_check(s3h_crc64nvme_combine(crc_a, crc_b, len_b, &out));
  return out;
}

// The FULL_OBJECT checksum of a multipart upload from its parts' CRCs and lengths.
inline uint64_t object_crc(const std::vector<uint64_t>& part_crcs, const std::vector<uint64_t>& lengths) {
  if (part_crcs.size() != lengths.size()) throw std::invalid_argument("crcs/lengths size mismatch");
  uint64_t out = 0;
  sha256::batch_check(s3h_crc64nvme_object(part_crcs.data(), lengths.data(), part_crcs.size(), &out));
  return out;
}

// Header value of one CRC (a part's, or object_crc's result): base64 of its big-endian bytes.
inline std::string checksum_text(uint64_t value) {
  char out[S3H_CHECKSUM_MAX];
  sha256::batch_check(s3h_checksum64_text(value, out, sizeof out));
  return out;
}

}  // namespace crc64

// x-amz-checksum-sha1 (SHA-1): 5 words per part with word i = bswap32(H_i), so the 20 bytes in
// memory are the canonical digest (the convention of the SHA-256 digests).
namespace sha1 {

// Parts already in device memory at d_base + offsets[i] (any alignment); n x 5 words to d_digests.
inline void sha1_batch_device(int device, const void* d_base, const std::vector<uint64_t>& offsets,
                              const std::vector<uint64_t>& lengths, uint32_t* d_digests,
                              void* stream = nullptr) {
  if (offsets.size() != lengths.size()) throw std::invalid_argument("offsets/lengths size mismatch");
  sha256::batch_check(s3h_sha1_batch_device(device, d_base, offsets.data(), lengths.data(),
                                            offsets.size(), d_digests, stream));
}

// Host-resident parts on the GPUs (s3h_sha1_batch_host): 5 words per part.
inline std::vector<uint32_t> sha1_batch(const std::vector<const uint8_t*>& parts,
                                        const std::vector<uint64_t>& lengths, int ndevices = 0,
                                        uint64_t slice_bytes = 0) {
  if (parts.size() != lengths.size()) throw std::invalid_argument("parts/lengths size mismatch");
  std::vector<uint32_t> d(5 * parts.size());
  if (!parts.empty())
    sha256::batch_check(s3h_sha1_batch_host(parts.data(), lengths.data(), parts.size(), d.data(),
                                            ndevices, slice_bytes));
  return d;
}

// (file, offset, size) parts (s3h_sha1_file_parts).
inline std::vector<uint32_t> file_part_sha1(const std::string& path, const std::vector<uint64_t>& offsets,
                                            const std::vector<uint64_t>& lengths, int ndevices = 0) {
  if (offsets.size() != lengths.size()) throw std::invalid_argument("offsets/lengths size mismatch");
  std::vector<uint32_t> d(5 * offsets.size());
  if (!offsets.empty())
    sha256::batch_check(s3h_sha1_file_parts(path.c_str(), offsets.data(), lengths.data(),
                                            offsets.size(), d.data(), ndevices, 0));
  return d;
}

// x-amz-content-sha256 and x-amz-checksum-sha1 per part from one pass over the host link.
struct Sha256Sha1 {
  std::vector<uint32_t> sha256;  // 8 words per part, lib/hash layout
  std::vector<uint32_t> sha1;    // 5 words per part
};
inline Sha256Sha1 sha256_sha1_batch(const std::vector<const uint8_t*>& parts,
                                    const std::vector<uint64_t>& lengths, int ndevices = 0,
                                    uint64_t slice_bytes = 0) {
  if (parts.size() != lengths.size()) throw std::invalid_argument("parts/lengths size mismatch");
  Sha256Sha1 d{std::vector<uint32_t>(8 * parts.size()), std::vector<uint32_t>(5 * parts.size())};
  if (!parts.empty())
    sha256::batch_check(s3h_sha256_sha1_batch_host(parts.data(), lengths.data(), parts.size(),
                                                   d.sha256.data(), d.sha1.data(), ndevices,
                                                   slice_bytes));
  return d;
}

inline Sha256Sha1 file_part_sha256_sha1(const std::string& path, const std::vector<uint64_t>& offsets,
                                        const std::vector<uint64_t>& lengths, int ndevices = 0) {
  if (offsets.size() != lengths.size()) throw std::invalid_argument("offsets/lengths size mismatch");
  Sha256Sha1 d{std::vector<uint32_t>(8 * offsets.size()), std::vector<uint32_t>(5 * offsets.size())};
  if (!offsets.empty())
    sha256::batch_check(s3h_sha256_sha1_file_parts(path.c_str(), offsets.data(), lengths.data(),
                                                   offsets.size(), d.sha256.data(), d.sha1.data(),
                                                   ndevices, 0));
  return d;
}

// One message on the CPU: 5 words.
inline std::vector<uint32_t> sha1(const uint8_t* data, uint64_t length) {
  if (!data && length) throw std::invalid_argument("sha1: null data");
  std::vector<uint32_t> h(5);
  s3h_cpu_sha1(data, length, h.data());
  return h;
}

// Header value of one digest (`algo`: S3H_ALGO_SHA1, 5 words, or S3H_ALGO_SHA256, 8 words):
// base64 of its bytes -- x-amz-checksum-sha1 / -sha256 of a part or a single-PUT object.
inline std::string checksum_text(const std::vector<uint32_t>& digest, int algo = S3H_ALGO_SHA1) {
  const size_t words = algo == S3H_ALGO_SHA256 ? 8 : 5;
  if (digest.size() != words) throw std::invalid_argument("checksum_text: one digest expected");
  char out[S3H_DIGEST_CHECKSUM_MAX];
  sha256::batch_check(s3h_digest_checksum_text(algo, digest.data(), 1, 0, out, sizeof out));
  return out;
}

// S3's COMPOSITE checksum of a multipart object from its parts' digests in part order:
// base64 of the same hash over the raw digests concatenated, then "-n".
inline std::string composite_checksum_text(const std::vector<uint32_t>& part_digests,
                                           int algo = S3H_ALGO_SHA1) {
  const size_t words = algo == S3H_ALGO_SHA256 ? 8 : 5;
  if (part_digests.empty() || part_digests.size() % words)
    throw std::invalid_argument("composite_checksum_text: need n x digest words");
  char out[S3H_DIGEST_CHECKSUM_MAX];
  sha256::batch_check(s3h_digest_checksum_text(algo, part_digests.data(), part_digests.size() / words,
                                               1, out, sizeof out));
  return out;
}

}  // namespace sha1

// SigV4 chunk-signed uploads (aws-chunked bodies, STREAMING-AWS4-HMAC-SHA256-PAYLOAD): each part
// cut into chunks, each chunk hashed on its own, one HMAC per chunk chained from the request's
// seed signature.  Signatures and seeds are 8 words each in the SHA-256 digest layout (the 32
// raw bytes in memory), part-major: a part's data-chunk signatures, then its final 0-byte
// chunk's.
namespace s3h {

// SigV4 signing key of `secret` for a date "YYYYMMDD", a region and a service.
inline std::vector<uint8_t> sigv4_signing_key(const std::string& secret, const std::string& date,
                                              const std::string& region, const std::string& service = "s3") {
  std::vector<uint8_t> key(32);
  sha256::batch_check(s3h_sigv4_signing_key(secret.c_str(), date.c_str(), region.c_str(), service.c_str(),
                                            key.data()));
  return key;
}

// The constant part of every chunk's string to sign, hashed once (s3h_chunk_sign_ctx_create).
class ChunkSignContext {
 public:
  ChunkSignContext(const std::vector<uint8_t>& key, const std::string& timestamp, const std::string& date,
                   const std::string& region, const std::string& service = "s3") {
    if (key.size() != 32) throw std::invalid_argument("ChunkSignContext: the signing key is 32 bytes");
    sha256::batch_check(s3h_chunk_sign_ctx_create(key.data(), timestamp.c_str(), date.c_str(),
                                                  region.c_str(), service.c_str(), &c_));
  }
  ~ChunkSignContext() { s3h_chunk_sign_ctx_destroy(c_); }
  ChunkSignContext(const ChunkSignContext&) = delete;
  ChunkSignContext& operator=(const ChunkSignContext&) = delete;
  s3h_chunk_sign_ctx_t get() const { return c_; }

  // The chains on the CPU over ready chunk digests (s3h_cpu_chunk_signatures): 8 words per data
  // chunk, part-major, data_chunks_per_part[p] of them for part p; seeds 8 words per part.
  std::vector<uint32_t> signatures(const std::vector<uint32_t>& chunk_digests,
                                   const std::vector<uint64_t>& data_chunks_per_part,
                                   const std::vector<uint32_t>& seeds) const {
    uint64_t chunks = 0;
    for (uint64_t c : data_chunks_per_part) chunks += c;
    if (chunk_digests.size() != 8 * chunks || seeds.size() != 8 * data_chunks_per_part.size())
      throw std::invalid_argument("ChunkSignContext: 8 words per data chunk and per seed");
    std::vector<uint32_t> out(8 * (chunks + data_chunks_per_part.size()));
    sha256::batch_check(s3h_cpu_chunk_signatures(c_, chunk_digests.data(), data_chunks_per_part.data(),
                                                 data_chunks_per_part.size(), seeds.data(), out.data()));
    return out;
  }

 private:
  s3h_chunk_sign_ctx_t c_ = nullptr;
};

// Device-resident parts (at d_base + offsets[i]) cut into chunks of chunk_bytes: the chunk
// hashes and the chains run on `stream` (s3h_chunk_plan_*).  One plan on one stream at a time.
class ChunkSignPlan {
 public:
  ChunkSignPlan(int device, const std::vector<uint64_t>& offsets, const std::vector<uint64_t>& lengths,
                uint64_t chunk_bytes) {
    if (offsets.size() != lengths.size()) throw std::invalid_argument("offsets/lengths size mismatch");
    sha256::batch_check(s3h_chunk_plan_create(device, offsets.data(), lengths.data(), offsets.size(),
                                              chunk_bytes, &p_));
    signature_offsets_.resize(lengths.size());
    sha256::batch_check(s3h_chunk_geometry(lengths.data(), lengths.size(), chunk_bytes, nullptr,
                                           signature_offsets_.data(), nullptr, &signatures_, nullptr));
  }
  ~ChunkSignPlan() { s3h_chunk_plan_destroy(p_); }
  ChunkSignPlan(const ChunkSignPlan&) = delete;
  ChunkSignPlan& operator=(const ChunkSignPlan&) = delete;

  // Asynchronous: d_seeds (n x 8 words) and d_signatures (signatures() x 8 words) are device
  // pointers, 16-byte aligned.  Call status() before using the signatures.
  void launch(const ChunkSignContext& ctx, const void* d_base, const uint32_t* d_seeds,
              uint32_t* d_signatures, void* stream = nullptr) {
    sha256::batch_check(s3h_chunk_plan_launch(p_, ctx.get(), d_base, d_seeds, d_signatures, stream));
  }
  // The chain alone over chunk digests the caller hashed itself (device, the plan's geometry).
  void chain(const ChunkSignContext& ctx, const uint32_t* d_chunk_digests, const uint32_t* d_seeds,
             uint32_t* d_signatures, void* stream = nullptr) {
    sha256::batch_check(s3h_chunk_plan_chain(p_, ctx.get(), d_chunk_digests, d_seeds, d_signatures, stream));
  }
  // Asynchronous, behind launch() on the same stream: part p's aws-chunked body at
  // d_body + body_offsets[p] (host array; null: packed back to back) (s3h_chunk_plan_body).
  void body(const void* d_base, const uint32_t* d_signatures, void* d_body, const uint64_t* body_offsets = nullptr,
            void* stream = nullptr) {
    sha256::batch_check(s3h_chunk_plan_body(p_, d_base, d_signatures, nullptr, nullptr, d_body, body_offsets, stream));
  }
  // The plan's body lengths (Content-Length of each part's request) and their sum.
  std::vector<uint64_t> body_lengths(uint64_t* total = nullptr) const {
    std::vector<uint64_t> out(signature_offsets_.size());
    sha256::batch_check(s3h_chunk_plan_body_info(p_, out.data(), total, nullptr, nullptr, nullptr));
    return out;
  }
  void status(void* stream = nullptr) { sha256::batch_check(s3h_chunk_plan_status(p_, stream)); }
  uint64_t signatures() const { return signatures_; }
  // Row of part p's first signature.
  const std::vector<uint64_t>& signature_offsets() const { return signature_offsets_; }
  std::string kernel() const {
    char name[16];
    sha256::batch_check(s3h_chunk_plan_info(p_, nullptr, nullptr, nullptr, nullptr, name, sizeof name));
    return name;
  }

 private:
  s3h_chunk_plan_t p_ = nullptr;
  uint64_t signatures_ = 0;
  std::vector<uint64_t> signature_offsets_;
};

// Host-resident parts: chunk digests on the GPUs, the chains on the CPU (s3h_chunk_sign_batch_host).
inline std::vector<uint32_t> chunk_signatures_host(const ChunkSignContext& ctx,
                                                   const std::vector<const uint8_t*>& parts,
                                                   const std::vector<uint64_t>& lengths, uint64_t chunk_bytes,
                                                   const std::vector<uint32_t>& seeds) {
  if (parts.size() != lengths.size() || seeds.size() != 8 * parts.size())
    throw std::invalid_argument("chunk_signatures_host: one length and one 8-word seed per part");
  uint64_t signatures = 0;
  sha256::batch_check(s3h_chunk_geometry(lengths.data(), lengths.size(), chunk_bytes, nullptr, nullptr,
                                         nullptr, &signatures, nullptr));
  std::vector<uint32_t> out(8 * signatures);
  sha256::batch_check(s3h_chunk_sign_batch_host(ctx.get(), parts.data(), lengths.data(), parts.size(),
                                                chunk_bytes, seeds.data(), out.data()));
  return out;
}

// The framing line before a chunk's bytes: "<hex len>;chunk-signature=<64 hex>\r\n".
inline std::string chunk_header_text(uint64_t chunk_len, const uint32_t* signature) {
  char out[S3H_CHUNK_HEADER_MAX];
  sha256::batch_check(s3h_chunk_header_text(chunk_len, signature, out, sizeof out));
  return out;
}

// ---- trailer signatures (STREAMING-AWS4-HMAC-SHA256-PAYLOAD-TRAILER): the same bodies closed by
// one trailing checksum header and a signature over it.  `checksum` is an s3h_trailer_checksum;
// values are uint32_t (CRC-32C, CRC-32) or uint64_t (CRC-64/NVME) per part, or 5 / 8 words per
// part for the SHA-1 / SHA-256 digests (CPU and host-resident forms only).

// The trailer link on the CPU (s3h_cpu_trailer_signatures): one value and one last chunk
// signature (8 words) per part -> 8 words per part.
template <class Value>
inline std::vector<uint32_t> trailer_signatures(const ChunkSignContext& ctx, int checksum,
                                                const std::vector<Value>& values,
                                                const std::vector<uint32_t>& last_signatures) {
  static_assert(sizeof(Value) == 4 || sizeof(Value) == 8, "uint32_t values or words, or uint64_t values");
  const uint64_t n = last_signatures.size() / 8;
  const uint64_t per = checksum == S3H_TRAILER_SHA1 ? 5 : checksum == S3H_TRAILER_SHA256 ? 8 : 1;
  const bool wide = checksum == S3H_TRAILER_CRC64NVME;
  if (last_signatures.size() != 8 * n || values.size() != per * n || (sizeof(Value) == 8) != wide)
    throw std::invalid_argument("trailer_signatures: one value of the checksum's type and 8 signature words per part");
  std::vector<uint32_t> out(8 * n);
  sha256::batch_check(s3h_cpu_trailer_signatures(ctx.get(), checksum, values.data(), last_signatures.data(), n,
                                                 out.data()));
  return out;
}

// "name:base64" of one value (s3h_trailer_line_text).
inline std::string trailer_line_text(int checksum, const void* value) {
  char out[S3H_TRAILER_LINE_MAX];
  sha256::batch_check(s3h_trailer_line_text(checksum, value, out, sizeof out));
  return out;
}

// What follows the "0;chunk-signature=...\r\n" line: the trailing header, the
// x-amz-trailer-signature line and the empty line (s3h_chunk_trailer_text).
inline std::string chunk_trailer_text(int checksum, const void* value, const uint32_t* trailer_signature) {
  char out[S3H_CHUNK_TRAILER_MAX];
  sha256::batch_check(s3h_chunk_trailer_text(checksum, value, trailer_signature, out, sizeof out));
  return out;
}

// A ChunkSignPlan that also owns a CRC plan over the whole parts (s3h_chunk_plan_create_trailer):
// checksum S3H_TRAILER_CRC32C, _CRC32 or _CRC64NVME.
class ChunkTrailerPlan {
 public:
  ChunkTrailerPlan(int device, int checksum, const std::vector<uint64_t>& offsets,
                   const std::vector<uint64_t>& lengths, uint64_t chunk_bytes)
      : checksum_(checksum) {
    if (offsets.size() != lengths.size()) throw std::invalid_argument("offsets/lengths size mismatch");
    sha256::batch_check(s3h_chunk_plan_create_trailer(device, checksum, offsets.data(), lengths.data(),
                                                      offsets.size(), chunk_bytes, &p_));
    signature_offsets_.resize(lengths.size());
    sha256::batch_check(s3h_chunk_geometry(lengths.data(), lengths.size(), chunk_bytes, nullptr,
                                           signature_offsets_.data(), nullptr, &signatures_, nullptr));
  }
  ~ChunkTrailerPlan() { s3h_chunk_plan_destroy(p_); }
  ChunkTrailerPlan(const ChunkTrailerPlan&) = delete;
  ChunkTrailerPlan& operator=(const ChunkTrailerPlan&) = delete;

  // Asynchronous: chunk hashes, chain, CRCs, trailer kernel on `stream`.  Device pointers:
  // d_seeds n x 8 words, d_signatures signatures() x 8 words, d_checksums n values,
  // d_trailer_signatures n x 8 words.  Call status() before using the outputs.
  void launch(const ChunkSignContext& ctx, const void* d_base, const uint32_t* d_seeds, uint32_t* d_signatures,
              void* d_checksums, uint32_t* d_trailer_signatures, void* stream = nullptr) {
    sha256::batch_check(s3h_chunk_plan_launch_trailer(p_, ctx.get(), d_base, d_seeds, d_signatures, d_checksums,
                                                      d_trailer_signatures, stream));
  }
  // The trailer kernel alone over chunk signatures and checksum values already on the device.
  void trailer(const ChunkSignContext& ctx, const uint32_t* d_signatures, const void* d_checksums,
               uint32_t* d_trailer_signatures, void* stream = nullptr) {
    sha256::batch_check(s3h_chunk_plan_trailer(p_, ctx.get(), d_signatures, d_checksums, d_trailer_signatures,
                                               stream));
  }
  // Asynchronous, behind launch() on the same stream: part p's body in the trailer form at
  // d_body + body_offsets[p] (host array; null: packed back to back) (s3h_chunk_plan_body).
  void body(const void* d_base, const uint32_t* d_signatures, const void* d_checksums,
            const uint32_t* d_trailer_signatures, void* d_body, const uint64_t* body_offsets = nullptr,
            void* stream = nullptr) {
    sha256::batch_check(s3h_chunk_plan_body(p_, d_base, d_signatures, d_checksums, d_trailer_signatures, d_body,
                                            body_offsets, stream));
  }
  // The plan's body lengths (Content-Length of each part's request) and their sum.
  std::vector<uint64_t> body_lengths(uint64_t* total = nullptr) const {
    std::vector<uint64_t> out(signature_offsets_.size());
    sha256::batch_check(s3h_chunk_plan_body_info(p_, out.data(), total, nullptr, nullptr, nullptr));
    return out;
  }
  void status(void* stream = nullptr) { sha256::batch_check(s3h_chunk_plan_status(p_, stream)); }
  int checksum() const { return checksum_; }
  uint64_t signatures() const { return signatures_; }
  const std::vector<uint64_t>& signature_offsets() const { return signature_offsets_; }
  s3h_chunk_plan_t get() const { return p_; }

 private:
  s3h_chunk_plan_t p_ = nullptr;
  int checksum_;
  uint64_t signatures_ = 0;
  std::vector<uint64_t> signature_offsets_;
};

// Host-resident parts (s3h_chunk_sign_trailer_batch_host): the chunk signatures, the checksums
// (as bytes in the kind's layout: 4, 8, 20 or 32 per part) and the trailer signatures.
struct ChunkTrailerResult {
  std::vector<uint32_t> signatures;
  std::vector<uint8_t> checksums;
  std::vector<uint32_t> trailer_signatures;
};
inline ChunkTrailerResult chunk_trailer_signatures_host(const ChunkSignContext& ctx, int checksum,
                                                        const std::vector<const uint8_t*>& parts,
                                                        const std::vector<uint64_t>& lengths,
                                                        uint64_t chunk_bytes, const std::vector<uint32_t>& seeds) {
  if (parts.size() != lengths.size() || seeds.size() != 8 * parts.size())
    throw std::invalid_argument("chunk_trailer_signatures_host: one length and one 8-word seed per part");
  uint64_t signatures = 0;
  sha256::batch_check(s3h_chunk_geometry(lengths.data(), lengths.size(), chunk_bytes, nullptr, nullptr,
                                         nullptr, &signatures, nullptr));
  ChunkTrailerResult r;
  r.signatures.resize(8 * signatures);
  r.checksums.resize(32 * parts.size());  // room for the widest kind
  r.trailer_signatures.resize(8 * parts.size());
  sha256::batch_check(s3h_chunk_sign_trailer_batch_host(ctx.get(), checksum, parts.data(), lengths.data(),
                                                        parts.size(), chunk_bytes, seeds.data(),
                                                        r.signatures.data(), r.checksums.data(),
                                                        r.trailer_signatures.data()));
  const uint64_t per = checksum == S3H_TRAILER_CRC64NVME ? 8 : checksum == S3H_TRAILER_SHA1 ? 20
                       : checksum == S3H_TRAILER_SHA256 ? 32 : 4;
  r.checksums.resize(per * parts.size());
  return r;
}

// ---- the bodies themselves: the framed bytes of a chunk-signed part.  `checksum` is -1 (no
// trailer) or an s3h_trailer_checksum.

// Wire length of each part's body (its request's Content-Length), where each starts when they are
// packed back to back, and their sum (s3h_chunk_body_geometry; no device).
struct ChunkBodyGeometry {
  std::vector<uint64_t> lengths, offsets;
  uint64_t total = 0;
};
inline ChunkBodyGeometry chunk_body_geometry(const std::vector<uint64_t>& lengths, uint64_t chunk_bytes,
                                             int checksum = -1) {
  ChunkBodyGeometry g;
  g.lengths.resize(lengths.size());
  g.offsets.resize(lengths.size());
  sha256::batch_check(s3h_chunk_body_geometry(lengths.data(), lengths.size(), chunk_bytes, checksum,
                                              g.lengths.data(), g.offsets.data(), &g.total));
  return g;
}

// Host-resident parts -> their bodies packed back to back (s3h_cpu_chunk_body).  `signatures` as
// ChunkSignContext::signatures returns them; with a checksum, `values` (one per part in the kind's
// layout) and `trailer_signatures` (8 words per part).
inline std::vector<uint8_t> chunk_body_host(const std::vector<const uint8_t*>& parts,
                                            const std::vector<uint64_t>& lengths, uint64_t chunk_bytes,
                                            const std::vector<uint32_t>& signatures, int checksum = -1,
                                            const void* values = nullptr,
                                            const std::vector<uint32_t>& trailer_signatures = {}) {
  uint64_t rows = 0;
  if (parts.size() != lengths.size()) throw std::invalid_argument("chunk_body_host: one length per part");
  sha256::batch_check(s3h_chunk_geometry(lengths.data(), lengths.size(), chunk_bytes, nullptr, nullptr, nullptr,
                                         &rows, nullptr));
  if (signatures.size() != 8 * rows || (checksum != -1 && trailer_signatures.size() != 8 * parts.size()))
    throw std::invalid_argument("chunk_body_host: 8 words per signature and per trailer signature");
  const ChunkBodyGeometry g = chunk_body_geometry(lengths, chunk_bytes, checksum);
  std::vector<uint8_t> out(g.total);
  sha256::batch_check(s3h_cpu_chunk_body(parts.data(), lengths.data(), parts.size(), chunk_bytes, signatures.data(),
                                         checksum, values, checksum == -1 ? nullptr : trailer_signatures.data(),
                                         out.data(), nullptr));
  return out;
}

// Device-resident parts, one-shot and blocking: signed and framed on the device, the packed bodies
// copied back (s3h_chunk_body_batch_device).  checksum -1, or a CRC kind.
inline std::vector<uint8_t> chunk_body_batch_device(int device, const ChunkSignContext& ctx, int checksum,
                                                    const void* d_base, const std::vector<uint64_t>& offsets,
                                                    const std::vector<uint64_t>& lengths, uint64_t chunk_bytes,
                                                    const std::vector<uint32_t>& seeds) {
  if (offsets.size() != lengths.size() || seeds.size() != 8 * lengths.size())
    throw std::invalid_argument("chunk_body_batch_device: one offset, one length and one 8-word seed per part");
  const ChunkBodyGeometry g = chunk_body_geometry(lengths, chunk_bytes, checksum);
  std::vector<uint8_t> out(g.total);
  sha256::batch_check(s3h_chunk_body_batch_device(device, ctx.get(), checksum, d_base, offsets.data(), lengths.data(),
                                                  lengths.size(), chunk_bytes, seeds.data(), out.data(), nullptr));
  return out;
}

}  // namespace s3h
