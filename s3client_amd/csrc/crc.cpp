// crc.cpp -- CRC-32C / CRC-32 / CRC-64/NVME of device-resident parts: the plan (per-part records and, for
// whole-part launches, a segment table, built on the host and uploaded once; per-polynomial
// lookup tables; the partials buffer the two stages hand segment values through; the per-part
// running values of ranged launches) and the s3h_crc_* / s3h_crc64nvme_* entry points of
// include/s3hash.h.  A 64-bit plan is the same plan with two words per value (words == 2) and
// the kernels of crc64_kernels.hip; everything about geometry is shared.  The
// host pipeline (host_path.cpp) reuses plans through crc_plan_alloc / _reserve / _refill.  The
// arithmetic is crc_math.hpp (shared with the kernels); the CPU functions are cpu/lib_crc.cpp.
#include <algorithm>
#include <vector>

#include "crc64_math.hpp"
#include "crc_math.hpp"
#include "internal.hpp"

using namespace s3h::host;
namespace gf = s3h::crc;
namespace gf64 = s3h::crc64;

namespace {

// Segment size: the largest power of two in [16 KiB, 256 KiB] that still cuts the batch into
// at least kMinSegments segments (one wave each: 256 CUs x 32 waves), so a few large parts
// fill the chip while many parts keep the per-segment work (a 6-step lane tree, ~10 tiles'
// worth of instructions) small beside the segment's 16-256 tiles.
constexpr uint32_t kLog2SegMin = 14, kLog2SegMax = 18;
constexpr uint64_t kMinSegments = 8192;
constexpr uint32_t kSegWaves = s3h::kCrcSegThreads / 64;
constexpr uint32_t kWgsPerCu = 4;  // 4 x 20.5 KiB of LDS, 32 waves: a full CU
static_assert(s3h::kCrc64SegThreads == s3h::kCrcSegThreads, "one grid rule for both widths");
constexpr uint32_t kWgsPerCu64 = 3;  // 3 x 48.6 KiB of LDS, 24 waves (6 per SIMD)

uint64_t count_segments(const uint64_t* lengths, uint64_t n, uint32_t log2s) {
  uint64_t s = 0;
  for (uint64_t i = 0; i < n; ++i) s += (lengths[i] + (uint64_t(1) << log2s) - 1) >> log2s;
  return s;
}

int check_batch_args(const void* a, const void* b, uint64_t n) {
  if (!a || !b) return fail(S3H_EINVAL, "crc: null offsets or lengths");
  if (n == 0 || n > kMaxParts)
    return fail(S3H_EINVAL, "crc: need 0 < n <= 2^31 (n=%llu)", (unsigned long long)n);
  return S3H_OK;
}

// the 32-bit entry points: enum s3h_crc only
int check_crc_args(int crc, const void* a, const void* b, uint64_t n) {
  if (crc != S3H_CRC32C && crc != S3H_CRC32) return fail(S3H_EINVAL, "crc: unknown checksum %d", crc);
  return check_batch_args(a, b, n);
}

uint32_t pick_log2_segment(const uint64_t* lengths, uint64_t n) {
  uint32_t log2s = kLog2SegMax;
  while (log2s > kLog2SegMin && count_segments(lengths, n, log2s) < kMinSegments) --log2s;
  return log2s;
}

uint32_t seg_grid(const s3h_crc_plan_s* P, uint64_t waves) {
  const uint64_t wgs = (waves + kSegWaves - 1) / kSegWaves;
  const uint32_t per_cu = P->words == 2 ? kWgsPerCu64 : kWgsPerCu;
  return uint32_t(std::min<uint64_t>(std::max<uint64_t>(wgs, 1), uint64_t(std::max(P->cus, 1)) * per_cu));
}

// The plan's geometry for these parts and its per-part records (n entries each).
void fill_records(s3h_crc_plan_s* P, const uint64_t* offsets, const uint64_t* lengths, uint64_t n,
                  s3h::CrcPart* parts, uint64_t* offs) {
  P->n = n;
  P->log2_segment = pick_log2_segment(lengths, n);
  P->longest = 0;
  P->range_end = 0;
  uint64_t k = 0;
  for (uint64_t i = 0; i < n; ++i) {
    parts[i] = {k, lengths[i]};
    offs[i] = offsets[i];
    k += (lengths[i] + (uint64_t(1) << P->log2_segment) - 1) >> P->log2_segment;
    P->longest = std::max(P->longest, lengths[i]);
  }
  P->nseg = k;
  P->grid = seg_grid(P, k);
}

template <class T>
hipError_t regrow(T** p, uint64_t count) {
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  return hipMalloc(reinterpret_cast<void**>(p), std::max<uint64_t>(count, 1) * sizeof(T));
}

int crc_plan_build(int device, int crc, const uint64_t* offsets, const uint64_t* lengths,
                   uint64_t n, s3h_crc_plan_s** out) {
  *out = nullptr;
  if (int rc = check_batch_args(offsets, lengths, n)) return rc;
  s3h_crc_plan_s* P = nullptr;
  if (int rc = crc_plan_alloc(device, crc, &P)) return rc;
  struct Guard {
    s3h_crc_plan_s* P;
    ~Guard() { if (P) s3h_crc_plan_destroy(P); }
  } guard{P};
  std::vector<s3h::CrcPart> parts(n);
  std::vector<uint64_t> offs(n);
  fill_records(P, offsets, lengths, n, parts.data(), offs.data());
  const uint64_t S = uint64_t(1) << P->log2_segment;
  std::vector<s3h::CrcSeg> segs(P->nseg);
  uint64_t k = 0;
  for (uint64_t i = 0; i < n; ++i)
    for (uint64_t done = 0; done < lengths[i]; done += S)
      segs[k++] = {offsets[i] + done, uint32_t(std::min(S, lengths[i] - done)), 0};

  if (int rc = crc_plan_reserve(P, n, P->nseg)) return rc;
  DeviceGuard g(device);
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&P->d_segs), std::max<uint64_t>(P->nseg, 1) * sizeof(s3h::CrcSeg)));
  HIP_TRY(hipMemcpy(P->d_parts, parts.data(), n * sizeof(s3h::CrcPart), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(P->d_offs, offs.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
  if (P->nseg)
    HIP_TRY(hipMemcpy(P->d_segs, segs.data(), P->nseg * sizeof(s3h::CrcSeg), hipMemcpyHostToDevice));
  guard.P = nullptr;
  *out = P;
  return S3H_OK;
}

s3h::Crc64Args crc64_args(const s3h_crc_plan_s* P, const void* d_base, void* d_crcs) {
  s3h::Crc64Args A;
  A.base = static_cast<const uint8_t*>(d_base);
  A.segs = P->d_segs;
  A.parts = P->d_parts;
  A.offs = P->d_offs;
  A.tables = reinterpret_cast<const uint64_t*>(P->d_tables);
  A.partials = reinterpret_cast<uint64_t*>(P->d_partials);
  A.state = reinterpret_cast<uint64_t*>(P->d_state);
  A.crcs = static_cast<uint64_t*>(d_crcs);
  A.n = P->n;
  A.nseg = P->nseg;
  A.begin = A.end = A.origin = 0;
  A.poly = P->poly64;
  A.x_segment = gf64::xpow8(uint64_t(1) << P->log2_segment, P->poly64);
  A.log2_segment = P->log2_segment;
  return A;
}

// d_crcs: n values of P->words words
int crc_plan_launch(s3h_crc_plan_s* P, const void* d_base, uint32_t* d_crcs, hipStream_t s) {
  if (P->words == 2) {
    const s3h::Crc64Args A64 = crc64_args(P, d_base, d_crcs);
    DeviceGuard g(P->device);
    (void)hipGetLastError();
    HIP_TRY(launch_crc64(A64, P->grid, s));
    P->range_end = 0;
    return S3H_OK;
  }
  s3h::CrcSegArgs A;
  A.base = static_cast<const uint8_t*>(d_base);
  A.segs = P->d_segs;
  A.tables = P->d_tables;
  A.partials = P->d_partials;
  A.nseg = P->nseg;
  A.poly = P->poly;
  s3h::CrcPartArgs B;
  B.parts = P->d_parts;
  B.partials = P->d_partials;
  B.crcs = d_crcs;
  B.n = P->n;
  B.poly = P->poly;
  B.x_segment = gf::xpow8(uint64_t(1) << P->log2_segment, P->poly);
  B.log2_segment = P->log2_segment;
  DeviceGuard g(P->device);
  (void)hipGetLastError();
  HIP_TRY(launch_crc(A, P->grid, B, s));
  P->range_end = 0;  // the partials are shared: a ranged pass cannot go on across this launch
  return S3H_OK;
}

}  // namespace

namespace s3h::host {

int crc_plan_alloc(int device, int crc, s3h_crc_plan_s** out) {
  *out = nullptr;
  if (crc != S3H_CRC32C && crc != S3H_CRC32 && crc != kCrcIdCrc64Nvme)
    return fail(S3H_EINVAL, "crc: unknown checksum %d", crc);
  if (int rc = check_device(device)) return rc;
  auto* P = new s3h_crc_plan_s;
  struct Guard {
    s3h_crc_plan_s* P;
    ~Guard() { if (P) s3h_crc_plan_destroy(P); }
  } guard{P};
  P->device = device;
  P->crc = crc;
  P->poly = crc == S3H_CRC32C ? gf::kPolyCrc32c : gf::kPolyCrc32;
  P->cus = device_cus(device);
  if (crc == kCrcIdCrc64Nvme) {
    P->poly = 0;
    P->poly64 = gf64::kPolyNvme;
    P->words = 2;
    std::vector<uint64_t> t64(gf64::kTableWords);
    gf64::build_device_tables(P->poly64, t64.data());
    DeviceGuard g(device);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&P->d_tables), gf64::kTableWords * 8));
    HIP_TRY(hipMemcpy(P->d_tables, t64.data(), gf64::kTableWords * 8, hipMemcpyHostToDevice));
    guard.P = nullptr;
    *out = P;
    return S3H_OK;
  }
  std::vector<uint32_t> tables(gf::kTableWords);
  gf::build_device_tables(P->poly, tables.data());
  DeviceGuard g(device);
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&P->d_tables), gf::kTableWords * 4));
  HIP_TRY(hipMemcpy(P->d_tables, tables.data(), gf::kTableWords * 4, hipMemcpyHostToDevice));
  guard.P = nullptr;
  *out = P;
  return S3H_OK;
}

uint64_t crc_max_segments(const uint64_t* lengths, uint64_t n) {
  return count_segments(lengths, n, kLog2SegMin);
}

int crc_plan_reserve(s3h_crc_plan_s* P, uint64_t parts, uint64_t segments) {
  DeviceGuard g(P->device);
  if (P->cap < parts) {
    P->cap = 0;
    HIP_TRY(regrow(&P->d_parts, parts));
    HIP_TRY(regrow(&P->d_offs, parts));
    HIP_TRY(regrow(&P->d_state, parts * P->words));
    P->cap = parts;
  }
  if (P->seg_cap < segments || !P->d_partials) {
    P->seg_cap = 0;
    HIP_TRY(regrow(&P->d_partials, segments * P->words));
    P->seg_cap = segments;
  }
  return S3H_OK;
}

int crc_plan_refill(s3h_crc_plan_s* P, const uint64_t* offsets, const uint64_t* lengths, uint64_t n,
                    s3h::CrcPart* h_parts, uint64_t* h_offs, hipStream_t s) {
  if (n == 0 || n > P->cap) return fail(S3H_EINVAL, "crc refill: %llu parts, room for %llu",
                                        (unsigned long long)n, (unsigned long long)P->cap);
  fill_records(P, offsets, lengths, n, h_parts, h_offs);
  if (P->nseg > P->seg_cap) return fail(S3H_EINVAL, "crc refill: %llu segments, room for %llu",
                                        (unsigned long long)P->nseg, (unsigned long long)P->seg_cap);
  DeviceGuard g(P->device);
  HIP_TRY(hipMemcpyAsync(P->d_parts, h_parts, n * sizeof(s3h::CrcPart), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(P->d_offs, h_offs, n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  return S3H_OK;
}

// No allocation, no synchronisation, no upload: two kernel launches.
int crc_plan_launch_range(s3h_crc_plan_s* P, const void* d_base, uint32_t* d_crcs, uint64_t begin,
                          uint64_t end, uint64_t origin, hipStream_t s) {
  if (begin >= end || origin > begin)
    return fail(S3H_EINVAL, "crc range: need byte_origin <= byte_begin < byte_end (%llu, %llu, %llu)",
                (unsigned long long)origin, (unsigned long long)begin, (unsigned long long)end);
  if (begin != 0 && begin != P->range_end)
    return fail(S3H_EINVAL, "crc range: byte_begin %llu does not continue the previous range (ended at %llu)",
                (unsigned long long)begin, (unsigned long long)P->range_end);
  if (P->words == 2) {
    s3h::Crc64Args A64 = crc64_args(P, d_base, d_crcs);
    A64.segs = nullptr;
    A64.begin = begin;
    A64.end = end;
    A64.origin = origin;
    DeviceGuard g(P->device);
    (void)hipGetLastError();
    HIP_TRY(launch_crc64_range(A64, seg_grid(P, P->n * gf::range_pieces(begin, end, P->log2_segment)), s));
    P->range_end = end;
    return S3H_OK;
  }
  s3h::CrcRangeArgs A;
  A.base = static_cast<const uint8_t*>(d_base);
  A.parts = P->d_parts;
  A.offs = P->d_offs;
  A.tables = P->d_tables;
  A.partials = P->d_partials;
  A.state = P->d_state;
  A.crcs = d_crcs;
  A.n = P->n;
  A.begin = begin;
  A.end = end;
  A.origin = origin;
  A.poly = P->poly;
  A.x_segment = gf::xpow8(uint64_t(1) << P->log2_segment, P->poly);
  A.log2_segment = P->log2_segment;
  DeviceGuard g(P->device);
  (void)hipGetLastError();
  HIP_TRY(launch_crc_range(A, seg_grid(P, P->n * gf::range_pieces(begin, end, P->log2_segment)), s));
  P->range_end = end;
  return S3H_OK;
}

}  // namespace s3h::host

extern "C" {

int s3h_crc_plan_create(int device, int crc, const uint64_t* offsets, const uint64_t* lengths,
                        uint64_t n, s3h_crc_plan_t* plan) {
  if (!plan) return fail(S3H_EINVAL, "crc: null plan out-pointer");
  *plan = nullptr;
  if (int rc = check_crc_args(crc, offsets, lengths, n)) return rc;
  return crc_plan_build(device, crc, offsets, lengths, n, plan);
}

int s3h_crc_plan_launch(s3h_crc_plan_t P, const void* d_base, uint32_t* d_crcs, void* stream) {
  if (!P || !d_base || !d_crcs) return fail(S3H_EINVAL, "crc launch: null argument");
  if (misaligned(d_crcs, 4)) return fail(S3H_EINVAL, "crc launch: crcs must be 4-byte aligned");
  return crc_plan_launch(P, d_base, d_crcs, static_cast<hipStream_t>(stream));
}

int s3h_crc_plan_launch_range(s3h_crc_plan_t P, const void* d_base, uint32_t* d_crcs,
                              uint64_t byte_begin, uint64_t byte_end, uint64_t byte_origin,
                              void* stream) {
  if (!P || !d_base || !d_crcs) return fail(S3H_EINVAL, "crc range launch: null argument");
  if (misaligned(d_crcs, 4)) return fail(S3H_EINVAL, "crc range launch: crcs must be 4-byte aligned");
  return crc_plan_launch_range(P, d_base, d_crcs, byte_begin, byte_end, byte_origin,
                               static_cast<hipStream_t>(stream));
}

int s3h_crc_plan_info(s3h_crc_plan_t P, uint64_t* n, uint64_t* segments, uint64_t* segment_bytes,
                      uint32_t* grid) {
  if (!P) return fail(S3H_EINVAL, "crc: null plan");
  if (n) *n = P->n;
  if (segments) *segments = P->nseg;
  if (segment_bytes) *segment_bytes = uint64_t(1) << P->log2_segment;
  if (grid) *grid = P->grid;
  return S3H_OK;
}

int s3h_crc_plan_destroy(s3h_crc_plan_t P) {
  if (!P) return S3H_OK;
  DeviceGuard g(P->device);
  (void)hipFree(P->d_segs);
  (void)hipFree(P->d_parts);
  (void)hipFree(P->d_tables);
  (void)hipFree(P->d_partials);
  (void)hipFree(P->d_offs);
  (void)hipFree(P->d_state);
  delete P;
  return S3H_OK;
}

int s3h_crc_batch_device(int device, int crc, const void* d_base, const uint64_t* offsets,
                         const uint64_t* lengths, uint64_t n, uint32_t* d_crcs, void* stream) {
  if (int rc = check_crc_args(crc, offsets, lengths, n)) return rc;
  if (!d_base || !d_crcs) return fail(S3H_EINVAL, "crc batch: null argument");
  if (misaligned(d_crcs, 4)) return fail(S3H_EINVAL, "crc batch: crcs must be 4-byte aligned");
  s3h_crc_plan_s* P = nullptr;
  if (int rc = crc_plan_build(device, crc, offsets, lengths, n, &P)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = crc_plan_launch(P, d_base, d_crcs, s);
  if (rc == S3H_OK) {
    DeviceGuard g(device);
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = fail(S3H_EHIP, "crc batch sync: %s", hipGetErrorString(e));
  }
  s3h_crc_plan_destroy(P);
  return rc;
}

int s3h_crc_verify_batch_device(int device, int crc, const void* d_base, const uint64_t* offsets,
                                const uint64_t* lengths, uint64_t n, const uint32_t* d_expected,
                                uint8_t* d_mismatch, uint64_t* mismatches, void* stream) {
  if (int rc = check_crc_args(crc, offsets, lengths, n)) return rc;
  if (!d_base || !d_expected || !d_mismatch || !mismatches)
    return fail(S3H_EINVAL, "crc verify: null argument");
  if (misaligned(d_expected, 4)) return fail(S3H_EINVAL, "crc verify: expected must be 4-byte aligned");
  s3h_crc_plan_s* P = nullptr;
  if (int rc = crc_plan_build(device, crc, offsets, lengths, n, &P)) return rc;
  struct Cleanup {
    s3h_crc_plan_s* P;
    ~Cleanup() { s3h_crc_plan_destroy(P); }
  } cleanup{P};
  DeviceGuard g(device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  VerifyScratch scratch(s);  // freed on every return below
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&scratch.values), n * 4, s));
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&scratch.count), 8, s));
  HIP_TRY(hipMemsetAsync(scratch.count, 0, 8, s));
  int rc = crc_plan_launch(P, d_base, scratch.values, s);
  if (rc == S3H_OK) {
    unsigned long long c = 0;
    hipError_t e = launch_compare_digests(scratch.values, d_expected, n, 1, d_mismatch, scratch.count, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&c, scratch.count, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = fail(S3H_EHIP, "crc verify: %s", hipGetErrorString(e));
    *mismatches = c;
  }
  return rc;
}

// ---------------------------------------------------------------- CRC-64/NVME
// The same plans with two words per value; d_crcs holds n 64-bit words.

int s3h_crc64nvme_plan_create(int device, const uint64_t* offsets, const uint64_t* lengths, uint64_t n,
                              s3h_crc64nvme_plan_t* plan) {
  if (!plan) return fail(S3H_EINVAL, "crc64nvme: null plan out-pointer");
  *plan = nullptr;
  s3h_crc_plan_s* P = nullptr;
  if (int rc = crc_plan_build(device, kCrcIdCrc64Nvme, offsets, lengths, n, &P)) return rc;
  *plan = new s3h_crc64nvme_plan_s{P};
  return S3H_OK;
}

int s3h_crc64nvme_plan_launch(s3h_crc64nvme_plan_t H, const void* d_base, uint64_t* d_crcs, void* stream) {
  if (!H || !d_base || !d_crcs) return fail(S3H_EINVAL, "crc64nvme launch: null argument");
  if (misaligned(d_crcs, 8)) return fail(S3H_EINVAL, "crc64nvme launch: crcs must be 8-byte aligned");
  return crc_plan_launch(H->p, d_base, reinterpret_cast<uint32_t*>(d_crcs), static_cast<hipStream_t>(stream));
}

int s3h_crc64nvme_plan_launch_range(s3h_crc64nvme_plan_t H, const void* d_base, uint64_t* d_crcs,
                                    uint64_t byte_begin, uint64_t byte_end, uint64_t byte_origin,
                                    void* stream) {
  if (!H || !d_base || !d_crcs) return fail(S3H_EINVAL, "crc64nvme range launch: null argument");
  if (misaligned(d_crcs, 8)) return fail(S3H_EINVAL, "crc64nvme range launch: crcs must be 8-byte aligned");
  return crc_plan_launch_range(H->p, d_base, reinterpret_cast<uint32_t*>(d_crcs), byte_begin, byte_end,
                               byte_origin, static_cast<hipStream_t>(stream));
}

int s3h_crc64nvme_plan_info(s3h_crc64nvme_plan_t H, uint64_t* n, uint64_t* segments,
                            uint64_t* segment_bytes, uint32_t* grid) {
  if (!H) return fail(S3H_EINVAL, "crc64nvme: null plan");
  return s3h_crc_plan_info(H->p, n, segments, segment_bytes, grid);
}

int s3h_crc64nvme_plan_destroy(s3h_crc64nvme_plan_t H) {
  if (!H) return S3H_OK;
  s3h_crc_plan_destroy(H->p);
  delete H;
  return S3H_OK;
}

int s3h_crc64nvme_batch_device(int device, const void* d_base, const uint64_t* offsets,
                               const uint64_t* lengths, uint64_t n, uint64_t* d_crcs, void* stream) {
  if (int rc = check_batch_args(offsets, lengths, n)) return rc;
  if (!d_base || !d_crcs) return fail(S3H_EINVAL, "crc64nvme batch: null argument");
  if (misaligned(d_crcs, 8)) return fail(S3H_EINVAL, "crc64nvme batch: crcs must be 8-byte aligned");
  s3h_crc_plan_s* P = nullptr;
  if (int rc = crc_plan_build(device, kCrcIdCrc64Nvme, offsets, lengths, n, &P)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = crc_plan_launch(P, d_base, reinterpret_cast<uint32_t*>(d_crcs), s);
  if (rc == S3H_OK) {
    DeviceGuard g(device);
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = fail(S3H_EHIP, "crc64nvme batch sync: %s", hipGetErrorString(e));
  }
  s3h_crc_plan_destroy(P);
  return rc;
}

int s3h_crc64nvme_verify_batch_device(int device, const void* d_base, const uint64_t* offsets,
                                      const uint64_t* lengths, uint64_t n, const uint64_t* d_expected,
                                      uint8_t* d_mismatch, uint64_t* mismatches, void* stream) {
  if (int rc = check_batch_args(offsets, lengths, n)) return rc;
  if (!d_base || !d_expected || !d_mismatch || !mismatches)
    return fail(S3H_EINVAL, "crc64nvme verify: null argument");
  if (misaligned(d_expected, 4)) return fail(S3H_EINVAL, "crc64nvme verify: expected must be 4-byte aligned");
  s3h_crc_plan_s* P = nullptr;
  if (int rc = crc_plan_build(device, kCrcIdCrc64Nvme, offsets, lengths, n, &P)) return rc;
  struct Cleanup {
    s3h_crc_plan_s* P;
    ~Cleanup() { s3h_crc_plan_destroy(P); }
  } cleanup{P};
  DeviceGuard g(device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  VerifyScratch scratch(s);  // freed on every return below
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&scratch.values), n * 8, s));
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&scratch.count), 8, s));
  HIP_TRY(hipMemsetAsync(scratch.count, 0, 8, s));
  int rc = crc_plan_launch(P, d_base, scratch.values, s);
  if (rc == S3H_OK) {
    unsigned long long c = 0;
    hipError_t e = launch_compare_digests(scratch.values, reinterpret_cast<const uint32_t*>(d_expected), n, 2,
                                          d_mismatch, scratch.count, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&c, scratch.count, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = fail(S3H_EHIP, "crc64nvme verify: %s", hipGetErrorString(e));
    *mismatches = c;
  }
  return rc;
}

}  // extern "C"
