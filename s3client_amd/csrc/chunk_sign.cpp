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
//
// Every plan also keeps what the body kernel needs (s3h_chunk_plan_body): one record per part,
// the packed body offsets and the fixed text on the device, uploaded at creation; a launch with
// offsets of the caller's uploads them in stream order through pinned memory the plan owns.
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
  // the bodies (chunk_body_kernels.hip)
  uint64_t chunk_bytes = 0;
  uint64_t src_lo = 0, src_hi = 0;        // extent of the non-empty parts, relative to the base pointer
  std::vector<uint64_t> body_len, body_off;  // wire lengths; offsets of the packed bodies
  uint64_t body_total = 0, body_items = 0;
  uint8_t* d_body_block = nullptr;        // one allocation: the three below and the text
  s3h::ChunkBodyPart* d_body_parts = nullptr;
  uint64_t* d_body_packed = nullptr;      // n packed offsets
  uint64_t* d_body_offs = nullptr;        // n offsets of the latest launch that gave its own
  uint8_t* d_body_text = nullptr;
  uint64_t* h_body_offs = nullptr;        // pinned staging of d_body_offs ...
  hipEvent_t body_staged = nullptr;       // ... free again once this has passed
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

uint32_t body_hexlen(uint64_t k) { return k == 0 ? 1 : uint32_t(64 - __builtin_clzll(k) + 3) / 4; }
// Work items of one full chunk (the clamp: no device holds a full chunk of 2^46 bytes, and a part
// shorter than its chunk size is a remainder, counted from its own length).
uint32_t body_pieces(uint64_t chunk_bytes) {
  return uint32_t(std::min<uint64_t>((chunk_bytes - 1) / s3h::kChunkBodyPiece + 1, 0xFFFFFFFFu));
}
uint32_t body_grid(uint64_t items) {
  constexpr uint64_t per_wg = s3h::kChunkBodyThreads / 64;
  return uint32_t(std::min<uint64_t>((items + per_wg - 1) / per_wg, s3h::kChunkBodyMaxGrid));
}

// What the body kernel reads, uploaded once: the parts' records, the packed offsets, the text.
int chunk_plan_body_setup(s3h_chunk_plan_s* P, const uint64_t* offsets, const uint64_t* lengths,
                          const uint64_t* sig, uint64_t chunk_bytes) {
  const uint64_t n = P->n;
  P->chunk_bytes = chunk_bytes;
  P->body_len.resize(n);
  P->body_off.resize(n);
  if (int rc = s3h_chunk_body_geometry(lengths, n, chunk_bytes, P->trailer, P->body_len.data(), P->body_off.data(),
                                       &P->body_total))
    return rc;
  const uint64_t ppc = body_pieces(chunk_bytes);
  std::vector<s3h::ChunkBodyPart> parts(n);
  uint64_t items = 0;
  P->src_lo = ~uint64_t(0);
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t full = lengths[i] / chunk_bytes, rem = lengths[i] - full * chunk_bytes;
    parts[i] = {offsets[i], lengths[i], full, items, sig[i]};
    items += full * ppc + (rem + s3h::kChunkBodyPiece - 1) / s3h::kChunkBodyPiece + 1;
    if (lengths[i]) {
      P->src_lo = std::min(P->src_lo, offsets[i]);
      P->src_hi = std::max(P->src_hi, offsets[i] + lengths[i]);
    }
  }
  P->body_items = items;
  uint8_t text[s3h::kChunkBodyTextBytes] = {0};
  std::memcpy(text, ";chunk-signature=", 17);
  if (const s3h::TrailerKind* K = P->trailer == -1 ? nullptr : s3h::trailer_kind(P->trailer)) {
    static_assert(s3h::kChunkBodySigAt - s3h::kChunkBodyNameAt >= 25, "the longest name and ':'");
    std::memcpy(text + s3h::kChunkBodyNameAt, K->name, std::strlen(K->name));
    text[s3h::kChunkBodyNameAt + std::strlen(K->name)] = ':';
  }
  std::memcpy(text + s3h::kChunkBodySigAt, "\r\nx-amz-trailer-signature:", 26);
  DeviceGuard g(P->device);
  const uint64_t rec = n * sizeof(s3h::ChunkBodyPart), off = n * sizeof(uint64_t);
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&P->d_body_block), rec + 2 * off + sizeof text));
  P->d_body_parts = reinterpret_cast<s3h::ChunkBodyPart*>(P->d_body_block);
  P->d_body_packed = reinterpret_cast<uint64_t*>(P->d_body_block + rec);
  P->d_body_offs = P->d_body_packed + n;
  P->d_body_text = P->d_body_block + rec + 2 * off;
  HIP_TRY(hipMemcpy(P->d_body_parts, parts.data(), rec, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(P->d_body_packed, P->body_off.data(), off, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(P->d_body_text, text, sizeof text, hipMemcpyHostToDevice));
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&P->h_body_offs), off, hipHostMallocDefault));
  HIP_TRY(hipEventCreateWithFlags(&P->body_staged, hipEventDisableTiming));
  return S3H_OK;
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
  if (int rc = chunk_plan_body_setup(P, offsets, lengths, sig.data(), chunk_bytes)) return rc;
  guard.P = nullptr;
  *out = P;
  return S3H_OK;
}

// S3H_EINVAL when two of the n bodies (offs, lens) share a byte.
int check_disjoint(const uint64_t* offs, const uint64_t* lens, uint64_t n) {
  std::vector<uint64_t> order(n);
  for (uint64_t i = 0; i < n; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return offs[a] < offs[b]; });
  for (uint64_t i = 1; i < n; ++i)
    if (offs[order[i - 1]] + lens[order[i - 1]] > offs[order[i]])
      return fail(S3H_EINVAL, "chunk body: the bodies of parts %llu and %llu overlap",
                  (unsigned long long)order[i - 1], (unsigned long long)order[i]);
  return S3H_OK;
}

int chunk_plan_body(s3h_chunk_plan_s* P, const void* d_base, const uint32_t* d_signatures, const void* d_checksums,
                    const uint32_t* d_trailer, void* d_body, const uint64_t* body_offsets, hipStream_t s) {
  const s3h::TrailerKind* K = P->trailer == -1 ? nullptr : s3h::trailer_kind(P->trailer);
  if (!d_signatures || !d_body || (P->chunks && !d_base)) return fail(S3H_EINVAL, "chunk body: null argument");
  if (K ? !d_checksums || !d_trailer : d_checksums || d_trailer)
    return fail(S3H_EINVAL, K ? "chunk body: a trailer plan needs checksums and trailer signatures"
                              : "chunk body: the plan was created without a trailer checksum");
  if ((reinterpret_cast<uintptr_t>(d_signatures) | reinterpret_cast<uintptr_t>(d_trailer)) & 3)
    return fail(S3H_EINVAL, "chunk body: signatures must be 4-byte aligned");
  if (K && reinterpret_cast<uintptr_t>(d_checksums) & (K->value_len - 1))
    return fail(S3H_EINVAL, "chunk body: checksums must be %u-byte aligned", K->value_len);
  uint64_t lo = 0, hi = P->body_total;
  if (body_offsets) {
    if (int rc = check_disjoint(body_offsets, P->body_len.data(), P->n)) return rc;
    lo = ~uint64_t(0), hi = 0;
    for (uint64_t i = 0; i < P->n; ++i) {
      lo = std::min(lo, body_offsets[i]);
      hi = std::max(hi, body_offsets[i] + P->body_len[i]);
    }
  }
  const uintptr_t b0 = reinterpret_cast<uintptr_t>(d_body) + lo, b1 = reinterpret_cast<uintptr_t>(d_body) + hi;
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(d_base) + P->src_lo, p1 = reinterpret_cast<uintptr_t>(d_base) + P->src_hi;
  if (P->src_hi > P->src_lo && b0 < p1 && p0 < b1)
    return fail(S3H_EINVAL, "chunk body: the bodies' extent intersects the parts'");
  DeviceGuard g(P->device);
  if (body_offsets) {  // through the plan's pinned staging, once the upload before this one has read it
    HIP_TRY(hipEventSynchronize(P->body_staged));
    std::memcpy(P->h_body_offs, body_offsets, P->n * sizeof(uint64_t));
    HIP_TRY(hipMemcpyAsync(P->d_body_offs, P->h_body_offs, P->n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(P->body_staged, s));
  }
  s3h::ChunkBodyArgs A;
  A.base = static_cast<const uint8_t*>(d_base);
  A.parts = P->d_body_parts;
  A.body_offs = body_offsets ? P->d_body_offs : P->d_body_packed;
  A.signatures = d_signatures;
  A.checksums = d_checksums;
  A.trailer = d_trailer;
  A.text = P->d_body_text;
  A.body = static_cast<uint8_t*>(d_body);
  A.n = P->n;
  A.items = P->body_items;
  A.chunk_bytes = P->chunk_bytes;
  A.pieces_per_chunk = body_pieces(P->chunk_bytes);
  A.head_len = body_hexlen(P->chunk_bytes) + 83;
  A.wide = K && K->value_len == 8;
  A.name_len = K ? uint32_t(std::strlen(K->name)) + 1 : 0;
  (void)hipGetLastError();
  HIP_TRY(launch_chunk_body(A, body_grid(P->body_items), s));
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

int s3h_chunk_plan_body(s3h_chunk_plan_t P, const void* d_base, const uint32_t* d_signatures,
                        const void* d_checksums, const uint32_t* d_trailer_signatures, void* d_body,
                        const uint64_t* body_offsets, void* stream) {
  if (!P) return fail(S3H_EINVAL, "chunk body: null plan");
  return chunk_plan_body(P, d_base, d_signatures, d_checksums, d_trailer_signatures, d_body, body_offsets,
                         static_cast<hipStream_t>(stream));
}

int s3h_chunk_plan_body_info(s3h_chunk_plan_t P, uint64_t* body_lengths, uint64_t* total, uint64_t* items,
                             uint64_t* piece_bytes, uint64_t* grid) {
  if (!P) return fail(S3H_EINVAL, "chunk plan: null plan");
  if (body_lengths) std::memcpy(body_lengths, P->body_len.data(), P->n * sizeof(uint64_t));
  if (total) *total = P->body_total;
  if (items) *items = P->body_items;
  if (piece_bytes) *piece_bytes = s3h::kChunkBodyPiece;
  if (grid) *grid = body_grid(P->body_items);
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
  (void)hipFree(P->d_body_block);
  if (P->h_body_offs) (void)hipHostFree(P->h_body_offs);
  if (P->body_staged) (void)hipEventDestroy(P->body_staged);
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

int s3h_chunk_body_batch_device(int device, s3h_chunk_sign_ctx_t ctx, int checksum, const void* d_base,
                                const uint64_t* offsets, const uint64_t* lengths, uint64_t n, uint64_t chunk_bytes,
                                const uint32_t* seeds_host, uint8_t* body_host, const uint64_t* body_offsets) {
  if (!ctx || !d_base || !seeds_host || !body_host) return fail(S3H_EINVAL, "chunk body batch: null argument");
  const s3h::TrailerKind* K = s3h::trailer_kind(checksum);
  if (checksum != -1 && !K) return fail(S3H_EINVAL, "chunk body batch: unknown checksum %d", checksum);
  s3h_chunk_plan_s* P = nullptr;
  if (int rc = chunk_plan_build(device, offsets, lengths, n, chunk_bytes, checksum, &P)) return rc;
  struct Cleanup {
    s3h_chunk_plan_s* P;
    uint32_t* d = nullptr;
    uint8_t* body = nullptr;
    ~Cleanup() {
      (void)hipFree(d);
      (void)hipFree(body);
      s3h_chunk_plan_destroy(P);
    }
  } c{P};
  if (body_offsets)
    if (int rc = check_disjoint(body_offsets, P->body_len.data(), n)) return rc;
  DeviceGuard g(device);
  // seeds, signatures, trailer signatures (32 bytes each), then the values; the bodies packed
  const uint64_t sigs = P->chunks + n;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c.d), (2 * n + sigs) * 32 + n * 8));
  if (hipMalloc(reinterpret_cast<void**>(&c.body), P->body_total) != hipSuccess) {
    (void)hipGetLastError();
    return fail(S3H_ENOMEM, "chunk body batch: %llu bytes of device memory for the bodies", (unsigned long long)P->body_total);
  }
  HIP_TRY(hipMemcpy(c.d, seeds_host, n * 32, hipMemcpyHostToDevice));
  uint32_t* d_sig = c.d + 8 * n;
  uint32_t* d_trailer = d_sig + 8 * sigs;
  uint32_t* d_values = d_trailer + 8 * n;
  if (int rc = K ? chunk_plan_launch_trailer(P, ctx, d_base, c.d, d_sig, d_values, d_trailer, nullptr)
                 : chunk_plan_launch(P, ctx, d_base, c.d, d_sig, nullptr))
    return rc;
  if (int rc = chunk_plan_body(P, d_base, d_sig, K ? d_values : nullptr, K ? d_trailer : nullptr, c.body, nullptr, nullptr))
    return rc;
  if (int rc = s3h_chunk_plan_status(P, nullptr)) return rc;
  if (!body_offsets) {
    HIP_TRY(hipMemcpy(body_host, c.body, P->body_total, hipMemcpyDeviceToHost));
  } else {
    for (uint64_t i = 0; i < n; ++i)
      HIP_TRY(hipMemcpy(body_host + body_offsets[i], c.body + P->body_off[i], P->body_len[i], hipMemcpyDeviceToHost));
  }
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
