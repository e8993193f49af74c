// chunk_sign.cpp -- SigV4 chunk-signed uploads on the device and from host memory
// (s3h_chunk_plan_*, s3h_chunk_sign_batch_device, s3h_chunk_sign_batch_host).
//
// A chunk plan is an ordinary SHA-256 plan whose parts are the chunks (AUTO picks its kernel by
// the chunk count) plus one chain record per part; a launch is the hash launch followed by the
// chain kernel on the same stream, which reads the plan-owned chunk digests.  The context and
// the CPU chain are cpu/lib_chunk_sign.cpp; the host-resident form hashes the chunks through the
// host pipeline and chains on the CPU.
//
// A trailer plan (s3h_chunk_plan_create_trailer) also owns a CRC plan over the whole parts: its
// launch is the chunk launch, the CRC launch and sigv4_trailer_kernel, all on the caller's stream.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "chunk_sign.hpp"
#include "internal.hpp"

using namespace s3h::host;

struct s3h_chunk_plan_s {
  int device = 0;
  uint64_t n = 0;
  uint64_t chunks = 0;          // data chunks in all
  uint64_t max_chunks = 0;      // of one part
  s3h_plan_s* hash = nullptr;   // the chunks as parts (null: no data chunk)
  uint32_t* d_digests = nullptr;          // chunks x 8 words
  s3h::ChunkChainPart* d_parts = nullptr; // n records
  int trailer = -1;                       // enum s3h_trailer_checksum of a trailer plan
  s3h_crc_plan_t crc = nullptr;           // ... its CRC plan over the whole parts: 32-bit kinds
  s3h_crc64nvme_plan_t crc64 = nullptr;   // ... or CRC-64/NVME
};

namespace {

// Offsets and lengths of every data chunk, part-major.
void cut_chunks(const uint64_t* offsets, const uint64_t* lengths, uint64_t n, uint64_t chunk_bytes,
                std::vector<uint64_t>& co, std::vector<uint64_t>& cl) {
  for (uint64_t i = 0; i < n; ++i)
    for (uint64_t at = 0; at < lengths[i]; at += chunk_bytes) {
      co.push_back((offsets ? offsets[i] : 0) + at);
      cl.push_back(std::min(chunk_bytes, lengths[i] - at));
    }
}

// `trailer`: -1, or the CRC kind whose plan over the whole parts the chunk plan owns.
int chunk_plan_build(int device, const uint64_t* offsets, const uint64_t* lengths, uint64_t n,
                     uint64_t chunk_bytes, int trailer, s3h_chunk_plan_s** out) {
  *out = nullptr;
  if (!offsets || !lengths) return fail(S3H_EINVAL, "chunk plan: need offsets and lengths");
  if (trailer == S3H_TRAILER_SHA1 || trailer == S3H_TRAILER_SHA256)
    return fail(S3H_EINVAL, "chunk plan: a digest checksum is a whole-part chain, not offered on the device");
  if (trailer != -1 && !s3h::trailer_kind(trailer)) return fail(S3H_EINVAL, "chunk plan: unknown checksum %d", trailer);
  std::vector<uint64_t> counts(n ? n : 1), sig(n ? n : 1);
  uint64_t chunks = 0, longest = 0;
  if (int rc = s3h_chunk_geometry(lengths, n, chunk_bytes, counts.data(), sig.data(), &chunks, nullptr,
                                  &longest))
    return rc;
  if (int rc = check_device(device)) return rc;
  auto* P = new s3h_chunk_plan_s;
  struct Guard {
    s3h_chunk_plan_s* P;
    ~Guard() { if (P) s3h_chunk_plan_destroy(P); }
  } guard{P};
  P->device = device;
  P->n = n;
  P->chunks = chunks;
  P->max_chunks = longest;
  if (chunks) {
    std::vector<uint64_t> co, cl;
    co.reserve(chunks);
    cl.reserve(chunks);
    cut_chunks(offsets, lengths, n, chunk_bytes, co, cl);
    if (int rc = plan_build(device, S3H_ALGO_SHA256, co.data(), cl.data(), chunks, S3H_KERNEL_AUTO, &P->hash))
      return rc;
  }
  std::vector<s3h::ChunkChainPart> parts(n);
  for (uint64_t i = 0; i < n; ++i) parts[i] = {sig[i] - i, sig[i], uint32_t(counts[i]), 0};
  DeviceGuard g(device);
  if (chunks) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&P->d_digests), chunks * 8 * sizeof(uint32_t)));
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&P->d_parts), n * sizeof(s3h::ChunkChainPart)));
  HIP_TRY(hipMemcpy(P->d_parts, parts.data(), n * sizeof(s3h::ChunkChainPart), hipMemcpyHostToDevice));
  P->trailer = trailer;
  if (trailer == S3H_TRAILER_CRC64NVME) {
    if (int rc = s3h_crc64nvme_plan_create(device, offsets, lengths, n, &P->crc64)) return rc;
  } else if (trailer != -1) {
    const int crc = trailer == S3H_TRAILER_CRC32C ? S3H_CRC32C : S3H_CRC32;
    if (int rc = s3h_crc_plan_create(device, crc, offsets, lengths, n, &P->crc)) return rc;
  }
  guard.P = nullptr;
  *out = P;
  return S3H_OK;
}

// The chain kernel over `d_digests` (the plan's own, or the caller's in the plan's geometry).
int chunk_plan_chain(s3h_chunk_plan_s* P, const s3h_chunk_sign_ctx_s* C, const uint32_t* d_digests,
                     const uint32_t* d_seeds, uint32_t* d_signatures, hipStream_t s) {
  if ((reinterpret_cast<uintptr_t>(d_digests) | reinterpret_cast<uintptr_t>(d_seeds) |
       reinterpret_cast<uintptr_t>(d_signatures)) & 15)
    return fail(S3H_EINVAL, "chunk launch: digests, seeds and signatures must be 16-byte aligned");
  s3h::ChunkChainArgs A;
  A.digests = d_digests;
  A.parts = P->d_parts;
  A.seeds = d_seeds;
  A.signatures = d_signatures;
  A.n = P->n;
  A.r = C->r;
  A.nblk = C->nblk;
  std::memcpy(A.istate, C->istate, sizeof A.istate);
  std::memcpy(A.ostate, C->ostate, sizeof A.ostate);
  static_assert(sizeof A.tail == sizeof C->tail_words, "one tail template");
  std::memcpy(A.tail, C->tail_words, sizeof A.tail);
  DeviceGuard g(P->device);
  (void)hipGetLastError();
  HIP_TRY(launch_chunk_chain(A, s));
  return S3H_OK;
}

int chunk_plan_launch(s3h_chunk_plan_s* P, const s3h_chunk_sign_ctx_s* C, const void* d_base,
                      const uint32_t* d_seeds, uint32_t* d_signatures, hipStream_t s) {
  if ((reinterpret_cast<uintptr_t>(d_seeds) | reinterpret_cast<uintptr_t>(d_signatures)) & 15)
    return fail(S3H_EINVAL, "chunk launch: seeds and signatures must be 16-byte aligned");
  if (P->hash)
    if (int rc = plan_launch(P->hash, d_base, P->d_digests, 0, P->hash->max_blocks, 0, s, false)) return rc;
  return chunk_plan_chain(P, C, P->d_digests, d_seeds, d_signatures, s);
}

// The trailer kernel over chunk signatures and checksum values on the device.
int chunk_plan_trailer(s3h_chunk_plan_s* P, const s3h_chunk_sign_ctx_s* C, const uint32_t* d_signatures,
                       const void* d_checksums, uint32_t* d_trailer, hipStream_t s) {
  if (P->trailer == -1) return fail(S3H_EINVAL, "chunk trailer: the plan was created without a trailer checksum");
  const s3h::TrailerKind* K = s3h::trailer_kind(P->trailer);
  if ((reinterpret_cast<uintptr_t>(d_signatures) | reinterpret_cast<uintptr_t>(d_trailer)) & 15)
    return fail(S3H_EINVAL, "chunk trailer: signatures and trailer signatures must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_checksums) & (K->value_len - 1))
    return fail(S3H_EINVAL, "chunk trailer: checksums must be %u-byte aligned", K->value_len);
  s3h::ChunkTrailerArgs A;
  A.signatures = d_signatures;
  A.parts = P->d_parts;
  A.checksums = d_checksums;
  A.trailer = d_trailer;
  A.n = P->n;
  A.r = C->r;
  A.nblk = C->trailer_nblk;
  A.wide = K->value_len == 8;
  // the line's one block: name ':' [text] '\n' 0x80, zeros, the bit length
  const uint32_t name = uint32_t(std::strlen(K->name)), len = name + 1 + K->text_len + 1;
  uint8_t line[64] = {0};
  static_assert(sizeof line == sizeof A.line, "one block");
  std::memcpy(line, K->name, name);
  line[name] = ':';
  line[len - 1] = '\n';
  line[len] = 0x80;
  line[62] = uint8_t((8 * len) >> 8);
  line[63] = uint8_t(8 * len);
  A.value_at = name + 1;
  for (int j = 0; j < 16; ++j)
    A.line[j] = uint32_t(line[4 * j]) << 24 | uint32_t(line[4 * j + 1]) << 16 | uint32_t(line[4 * j + 2]) << 8 | line[4 * j + 3];
  std::memcpy(A.istate, C->trailer_istate, sizeof A.istate);
  std::memcpy(A.ostate, C->ostate, sizeof A.ostate);
  static_assert(sizeof A.tail == sizeof C->trailer_tail_words, "one tail template");
  std::memcpy(A.tail, C->trailer_tail_words, sizeof A.tail);
  DeviceGuard g(P->device);
  (void)hipGetLastError();
  HIP_TRY(launch_chunk_trailer(A, s));
  return S3H_OK;
}

int chunk_plan_launch_trailer(s3h_chunk_plan_s* P, const s3h_chunk_sign_ctx_s* C, const void* d_base,
                              const uint32_t* d_seeds, uint32_t* d_signatures, void* d_checksums,
                              uint32_t* d_trailer, hipStream_t s) {
  if (P->trailer == -1) return fail(S3H_EINVAL, "chunk trailer: the plan was created without a trailer checksum");
  // every argument check before the first launch
  if ((reinterpret_cast<uintptr_t>(d_seeds) | reinterpret_cast<uintptr_t>(d_signatures) |
       reinterpret_cast<uintptr_t>(d_trailer)) & 15)
    return fail(S3H_EINVAL, "chunk trailer: seeds, signatures and trailer signatures must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_checksums) & (s3h::trailer_kind(P->trailer)->value_len - 1))
    return fail(S3H_EINVAL, "chunk trailer: checksums must be %u-byte aligned", s3h::trailer_kind(P->trailer)->value_len);
  if (int rc = chunk_plan_launch(P, C, d_base, d_seeds, d_signatures, s)) return rc;
  if (P->crc64) {
    if (int rc = s3h_crc64nvme_plan_launch(P->crc64, d_base, static_cast<uint64_t*>(d_checksums), s)) return rc;
  } else {
    if (int rc = s3h_crc_plan_launch(P->crc, d_base, static_cast<uint32_t*>(d_checksums), s)) return rc;
  }
  return chunk_plan_trailer(P, C, d_signatures, d_checksums, d_trailer, s);
}

}  // namespace

extern "C" {

int s3h_chunk_plan_create(int device, const uint64_t* offsets, const uint64_t* lengths, uint64_t n,
                          uint64_t chunk_bytes, s3h_chunk_plan_t* out) {
  if (!out) return fail(S3H_EINVAL, "chunk plan: null plan out-pointer");
  return chunk_plan_build(device, offsets, lengths, n, chunk_bytes, -1, out);
}

int s3h_chunk_plan_create_trailer(int device, int checksum, const uint64_t* offsets, const uint64_t* lengths,
                                  uint64_t n, uint64_t chunk_bytes, s3h_chunk_plan_t* out) {
  if (!out) return fail(S3H_EINVAL, "chunk plan: null plan out-pointer");
  *out = nullptr;
  if (!s3h::trailer_kind(checksum)) return fail(S3H_EINVAL, "chunk plan: unknown checksum %d", checksum);
  return chunk_plan_build(device, offsets, lengths, n, chunk_bytes, checksum, out);
}

int s3h_chunk_plan_launch_trailer(s3h_chunk_plan_t P, s3h_chunk_sign_ctx_t ctx, const void* d_base,
                                  const uint32_t* d_seeds, uint32_t* d_signatures, void* d_checksums,
                                  uint32_t* d_trailer_signatures, void* stream) {
  if (!P || !ctx || !d_base || !d_seeds || !d_signatures || !d_checksums || !d_trailer_signatures)
    return fail(S3H_EINVAL, "chunk trailer launch: null argument");
  return chunk_plan_launch_trailer(P, ctx, d_base, d_seeds, d_signatures, d_checksums, d_trailer_signatures,
                                   static_cast<hipStream_t>(stream));
}

int s3h_chunk_plan_trailer(s3h_chunk_plan_t P, s3h_chunk_sign_ctx_t ctx, const uint32_t* d_signatures,
                           const void* d_checksums, uint32_t* d_trailer_signatures, void* stream) {
  if (!P || !ctx || !d_signatures || !d_checksums || !d_trailer_signatures)
    return fail(S3H_EINVAL, "chunk trailer: null argument");
  return chunk_plan_trailer(P, ctx, d_signatures, d_checksums, d_trailer_signatures,
                            static_cast<hipStream_t>(stream));
}

int s3h_chunk_plan_trailer_info(s3h_chunk_plan_t P, int* checksum) {
  if (!P || !checksum) return fail(S3H_EINVAL, "chunk plan: null argument");
  *checksum = P->trailer;
  return S3H_OK;
}

int s3h_chunk_plan_launch(s3h_chunk_plan_t P, s3h_chunk_sign_ctx_t ctx, const void* d_base,
                          const uint32_t* d_seeds, uint32_t* d_signatures, void* stream) {
  if (!P || !ctx || !d_base || !d_seeds || !d_signatures) return fail(S3H_EINVAL, "chunk launch: null argument");
  return chunk_plan_launch(P, ctx, d_base, d_seeds, d_signatures, static_cast<hipStream_t>(stream));
}

int s3h_chunk_plan_chain(s3h_chunk_plan_t P, s3h_chunk_sign_ctx_t ctx, const uint32_t* d_chunk_digests,
                         const uint32_t* d_seeds, uint32_t* d_signatures, void* stream) {
  if (!P || !ctx || !d_seeds || !d_signatures || (P->chunks && !d_chunk_digests))
    return fail(S3H_EINVAL, "chunk chain: null argument");
  return chunk_plan_chain(P, ctx, d_chunk_digests, d_seeds, d_signatures, static_cast<hipStream_t>(stream));
}

int s3h_chunk_plan_status(s3h_chunk_plan_t P, void* stream) {
  if (!P) return fail(S3H_EINVAL, "chunk plan: null plan");
  DeviceGuard g(P->device);
  if (P->hash) return plan_check(P->hash, static_cast<hipStream_t>(stream));
  HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return S3H_OK;
}

int s3h_chunk_plan_info(s3h_chunk_plan_t P, uint64_t* n, uint64_t* data_chunks, uint64_t* signatures,
                        uint64_t* max_chunks_per_part, char* kernel_name, int len) {
  if (!P) return fail(S3H_EINVAL, "chunk plan: null plan");
  if (n) *n = P->n;
  if (data_chunks) *data_chunks = P->chunks;
  if (signatures) *signatures = P->chunks + P->n;
  if (max_chunks_per_part) *max_chunks_per_part = P->max_chunks;
  if (kernel_name && len > 0) std::snprintf(kernel_name, size_t(len), "%s", P->hash ? plan_kernel_name(P->hash) : "none");
  return S3H_OK;
}

int s3h_chunk_plan_destroy(s3h_chunk_plan_t P) {
  if (!P) return S3H_OK;
  s3h_plan_destroy(P->hash);
  s3h_crc_plan_destroy(P->crc);
  s3h_crc64nvme_plan_destroy(P->crc64);
  DeviceGuard g(P->device);
  (void)hipFree(P->d_digests);
  (void)hipFree(P->d_parts);
  delete P;
  return S3H_OK;
}

int s3h_chunk_sign_batch_device(int device, s3h_chunk_sign_ctx_t ctx, const void* d_base,
                                const uint64_t* offsets, const uint64_t* lengths, uint64_t n,
                                uint64_t chunk_bytes, const uint32_t* seeds_host, uint32_t* signatures_host) {
  if (!ctx || !d_base || !seeds_host || !signatures_host) return fail(S3H_EINVAL, "chunk batch: null argument");
  s3h_chunk_plan_s* P = nullptr;
  if (int rc = chunk_plan_build(device, offsets, lengths, n, chunk_bytes, -1, &P)) return rc;
  struct Cleanup {
    s3h_chunk_plan_s* P;
    uint32_t* d = nullptr;
    ~Cleanup() {
      (void)hipFree(d);
      s3h_chunk_plan_destroy(P);
    }
  } c{P};
  DeviceGuard g(device);
  const uint64_t sigs = P->chunks + n;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c.d), (n + sigs) * 32));
  HIP_TRY(hipMemcpy(c.d, seeds_host, n * 32, hipMemcpyHostToDevice));
  uint32_t* d_sig = c.d + 8 * n;
  if (int rc = chunk_plan_launch(P, ctx, d_base, c.d, d_sig, nullptr)) return rc;
  if (int rc = s3h_chunk_plan_status(P, nullptr)) return rc;
  HIP_TRY(hipMemcpy(signatures_host, d_sig, sigs * 32, hipMemcpyDeviceToHost));
  return S3H_OK;
}

int s3h_chunk_sign_batch_host(s3h_chunk_sign_ctx_t ctx, const uint8_t* const* parts, const uint64_t* lengths,
                              uint64_t n, uint64_t chunk_bytes, const uint32_t* seeds, uint32_t* signatures) {
  if (!ctx || !parts || !lengths || !seeds || !signatures) return fail(S3H_EINVAL, "chunk host batch: null argument");
  std::vector<uint64_t> counts(n ? n : 1);
  uint64_t chunks = 0;
  if (int rc = s3h_chunk_geometry(lengths, n, chunk_bytes, counts.data(), nullptr, &chunks, nullptr, nullptr))
    return rc;
  std::vector<uint32_t> digests(chunks * 8);
  if (chunks) {
    std::vector<uint64_t> co, cl;
    co.reserve(chunks);
    cl.reserve(chunks);
    cut_chunks(nullptr, lengths, n, chunk_bytes, co, cl);
    std::vector<const uint8_t*> cp(chunks);
    for (uint64_t i = 0, k = 0; i < n; ++i) {
      if (counts[i] && !parts[i]) return fail(S3H_EINVAL, "chunk host batch: part %llu is null", (unsigned long long)i);
      for (uint64_t c = 0; c < counts[i]; ++c, ++k) cp[k] = parts[i] + co[k];
    }
    if (int rc = s3h_sha256_batch_host(cp.data(), cl.data(), chunks, digests.data(), 0, 0)) return rc;
  }
  return s3h_cpu_chunk_signatures(ctx, digests.data(), counts.data(), n, seeds, signatures);
}

int s3h_chunk_sign_trailer_batch_device(int device, s3h_chunk_sign_ctx_t ctx, int checksum, const void* d_base,
                                        const uint64_t* offsets, const uint64_t* lengths, uint64_t n,
                                        uint64_t chunk_bytes, const uint32_t* seeds_host,
                                        uint32_t* signatures_host, void* checksums_host,
                                        uint32_t* trailer_signatures_host) {
  if (!ctx || !d_base || !seeds_host || !signatures_host || !checksums_host || !trailer_signatures_host)
    return fail(S3H_EINVAL, "chunk trailer batch: null argument");
  const s3h::TrailerKind* K = s3h::trailer_kind(checksum);
  if (!K) return fail(S3H_EINVAL, "chunk trailer batch: unknown checksum %d", checksum);
  s3h_chunk_plan_s* P = nullptr;
  if (int rc = chunk_plan_build(device, offsets, lengths, n, chunk_bytes, checksum, &P)) return rc;
  struct Cleanup {
    s3h_chunk_plan_s* P;
    uint32_t* d = nullptr;
    ~Cleanup() {
      (void)hipFree(d);
      s3h_chunk_plan_destroy(P);
    }
  } c{P};
  DeviceGuard g(device);
  // seeds, signatures, trailer signatures (32 bytes each), then the values
  const uint64_t sigs = P->chunks + n;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c.d), (2 * n + sigs) * 32 + n * K->value_len));
  HIP_TRY(hipMemcpy(c.d, seeds_host, n * 32, hipMemcpyHostToDevice));
  uint32_t* d_sig = c.d + 8 * n;
  uint32_t* d_trailer = d_sig + 8 * sigs;
  uint32_t* d_values = d_trailer + 8 * n;
  if (int rc = chunk_plan_launch_trailer(P, ctx, d_base, c.d, d_sig, d_values, d_trailer, nullptr)) return rc;
  if (int rc = s3h_chunk_plan_status(P, nullptr)) return rc;
  HIP_TRY(hipMemcpy(signatures_host, d_sig, sigs * 32, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(trailer_signatures_host, d_trailer, n * 32, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(checksums_host, d_values, n * K->value_len, hipMemcpyDeviceToHost));
  return S3H_OK;
}

int s3h_chunk_sign_trailer_batch_host(s3h_chunk_sign_ctx_t ctx, int checksum, const uint8_t* const* parts,
                                      const uint64_t* lengths, uint64_t n, uint64_t chunk_bytes,
                                      const uint32_t* seeds, uint32_t* signatures, void* checksums,
                                      uint32_t* trailer_signatures) {
  if (!ctx || !parts || !lengths || !seeds || !signatures || !checksums || !trailer_signatures)
    return fail(S3H_EINVAL, "chunk trailer host batch: null argument");
  const s3h::TrailerKind* K = s3h::trailer_kind(checksum);
  if (!K) return fail(S3H_EINVAL, "chunk trailer host batch: unknown checksum %d", checksum);
  std::vector<uint64_t> counts(n ? n : 1), sig(n ? n : 1);
  uint64_t chunks = 0;
  if (int rc = s3h_chunk_geometry(lengths, n, chunk_bytes, counts.data(), sig.data(), &chunks, nullptr, nullptr))
    return rc;
  const bool digest = checksum == S3H_TRAILER_SHA1 || checksum == S3H_TRAILER_SHA256;
  const bool wide = checksum == S3H_TRAILER_CRC64NVME;
  std::vector<uint32_t> digests(chunks * 8);
  std::vector<uint64_t> co, cl;
  std::vector<uint32_t> crcs(digest || wide ? 0 : chunks);
  std::vector<uint64_t> crcs64(wide ? chunks : 0);
  if (chunks) {
    co.reserve(chunks);
    cl.reserve(chunks);
    cut_chunks(nullptr, lengths, n, chunk_bytes, co, cl);
    std::vector<const uint8_t*> cp(chunks);
    for (uint64_t i = 0, k = 0; i < n; ++i) {
      if (counts[i] && !parts[i])
        return fail(S3H_EINVAL, "chunk trailer host batch: part %llu is null", (unsigned long long)i);
      for (uint64_t c = 0; c < counts[i]; ++c, ++k) cp[k] = parts[i] + co[k];
    }
    // one pass over the data: each chunk's SHA-256 and CRC
    int rc;
    if (digest)
      rc = s3h_sha256_batch_host(cp.data(), cl.data(), chunks, digests.data(), 0, 0);
    else if (wide)
      rc = s3h_sha256_crc64nvme_batch_host(cp.data(), cl.data(), chunks, digests.data(), crcs64.data(), 0, 0);
    else
      rc = s3h_sha256_crc_batch_host(checksum == S3H_TRAILER_CRC32C ? S3H_CRC32C : S3H_CRC32, cp.data(), cl.data(),
                                     chunks, digests.data(), crcs.data(), 0, 0);
    if (rc) return rc;
  }
  if (digest) {  // a whole-part hash: a second pass
    if (int rc = checksum == S3H_TRAILER_SHA1
                     ? s3h_sha1_batch_host(parts, lengths, n, static_cast<uint32_t*>(checksums), 0, 0)
                     : s3h_sha256_batch_host(parts, lengths, n, static_cast<uint32_t*>(checksums), 0, 0))
      return rc;
  } else {  // a part's CRC from its chunks' (an empty part: 0)
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t first = sig[i] - i;
      if (wide) {
        uint64_t v = 0;
        if (counts[i])
          if (int rc = s3h_crc64nvme_object(crcs64.data() + first, cl.data() + first, counts[i], &v)) return rc;
        static_cast<uint64_t*>(checksums)[i] = v;
      } else {
        uint32_t v = 0;
        if (counts[i])
          if (int rc = s3h_crc_object(checksum == S3H_TRAILER_CRC32C ? S3H_CRC32C : S3H_CRC32, crcs.data() + first,
                                      cl.data() + first, counts[i], &v))
            return rc;
        static_cast<uint32_t*>(checksums)[i] = v;
      }
    }
  }
  if (int rc = s3h_cpu_chunk_signatures(ctx, digests.data(), counts.data(), n, seeds, signatures)) return rc;
  std::vector<uint32_t> last(8 * n);
  for (uint64_t i = 0; i < n; ++i) std::memcpy(&last[8 * i], signatures + 8 * (sig[i] + counts[i]), 32);
  return s3h_cpu_trailer_signatures(ctx, checksum, checksums, last.data(), n, trailer_signatures);
}

}  // extern "C"
