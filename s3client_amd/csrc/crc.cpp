// crc.cpp -- CRC-32C / CRC-32 of device-resident parts: the plan (segment table built on the
// host and uploaded once, per-polynomial lookup tables, the partials buffer the two launches
// hand segment values through) and the s3h_crc_* entry points of include/s3hash.h.  The
// arithmetic is crc_math.hpp (shared with the kernels); the CPU functions are cpu/lib_crc.cpp.
#include <algorithm>
#include <vector>

#include "crc_math.hpp"
#include "internal.hpp"

struct s3h_crc_plan_s {
  int device = 0;
  int crc = S3H_CRC32C;
  uint32_t poly = 0;
  uint64_t n = 0;
  uint64_t nseg = 0;
  uint32_t log2_segment = 0;
  uint32_t grid = 0;               // workgroups of the segment launch
  s3h::CrcSeg* d_segs = nullptr;
  s3h::CrcPart* d_parts = nullptr;
  uint32_t* d_tables = nullptr;
  // One raw value per segment, written by stage 1 and read by stage 2 of the same launch:
  // plan-owned, so one plan runs on one stream at a time (include/s3hash.h).
  uint32_t* d_partials = nullptr;
};

using namespace s3h::host;
namespace gf = s3h::crc;

namespace {

// Segment size: the largest power of two in [16 KiB, 256 KiB] that still cuts the batch into
// at least kMinSegments segments (one wave each: 256 CUs x 32 waves), so a few large parts
// fill the chip while many parts keep the per-segment work (a 6-step lane tree, ~10 tiles'
// worth of instructions) small beside the segment's 16-256 tiles.
constexpr uint32_t kLog2SegMin = 14, kLog2SegMax = 18;
constexpr uint64_t kMinSegments = 8192;
constexpr uint32_t kSegWaves = s3h::kCrcSegThreads / 64;
constexpr uint32_t kWgsPerCu = 4;  // 4 x 20.5 KiB of LDS, 32 waves: a full CU

uint64_t count_segments(const uint64_t* lengths, uint64_t n, uint32_t log2s) {
  uint64_t s = 0;
  for (uint64_t i = 0; i < n; ++i) s += (lengths[i] + (uint64_t(1) << log2s) - 1) >> log2s;
  return s;
}

int check_crc_args(int crc, const void* a, const void* b, uint64_t n) {
  if (crc != S3H_CRC32C && crc != S3H_CRC32) return fail(S3H_EINVAL, "crc: unknown checksum %d", crc);
  if (!a || !b) return fail(S3H_EINVAL, "crc: null offsets or lengths");
  if (n == 0 || n > kMaxParts)
    return fail(S3H_EINVAL, "crc: need 0 < n <= 2^31 (n=%llu)", (unsigned long long)n);
  return S3H_OK;
}

int crc_plan_build(int device, int crc, const uint64_t* offsets, const uint64_t* lengths,
                   uint64_t n, s3h_crc_plan_s** out) {
  *out = nullptr;
  if (int rc = check_crc_args(crc, offsets, lengths, n)) return rc;
  if (int rc = check_device(device)) return rc;
  auto* P = new s3h_crc_plan_s;
  struct Guard {
    s3h_crc_plan_s* P;
    ~Guard() { if (P) s3h_crc_plan_destroy(P); }
  } guard{P};
  P->device = device;
  P->crc = crc;
  P->poly = crc == S3H_CRC32C ? gf::kPolyCrc32c : gf::kPolyCrc32;
  P->n = n;
  P->log2_segment = kLog2SegMax;
  while (P->log2_segment > kLog2SegMin && count_segments(lengths, n, P->log2_segment) < kMinSegments)
    --P->log2_segment;
  P->nseg = count_segments(lengths, n, P->log2_segment);
  const uint64_t S = uint64_t(1) << P->log2_segment;

  std::vector<s3h::CrcPart> parts(n);
  std::vector<s3h::CrcSeg> segs(P->nseg);
  uint64_t k = 0;
  for (uint64_t i = 0; i < n; ++i) {
    parts[i] = {k, lengths[i]};
    for (uint64_t done = 0; done < lengths[i]; done += S)
      segs[k++] = {offsets[i] + done, uint32_t(std::min(S, lengths[i] - done)), 0};
  }
  std::vector<uint32_t> tables(gf::kTableWords);
  gf::build_device_tables(P->poly, tables.data());

  const int cus = std::max(device_cus(device), 1);
  const uint64_t wgs = (P->nseg + kSegWaves - 1) / kSegWaves;
  P->grid = uint32_t(std::min<uint64_t>(std::max<uint64_t>(wgs, 1), uint64_t(cus) * kWgsPerCu));

  DeviceGuard g(device);
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&P->d_parts), n * sizeof(s3h::CrcPart)));
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&P->d_segs), std::max<uint64_t>(P->nseg, 1) * sizeof(s3h::CrcSeg)));
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&P->d_partials), std::max<uint64_t>(P->nseg, 1) * 4));
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&P->d_tables), gf::kTableWords * 4));
  HIP_TRY(hipMemcpy(P->d_parts, parts.data(), n * sizeof(s3h::CrcPart), hipMemcpyHostToDevice));
  if (P->nseg)
    HIP_TRY(hipMemcpy(P->d_segs, segs.data(), P->nseg * sizeof(s3h::CrcSeg), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(P->d_tables, tables.data(), gf::kTableWords * 4, hipMemcpyHostToDevice));
  guard.P = nullptr;
  *out = P;
  return S3H_OK;
}

int crc_plan_launch(s3h_crc_plan_s* P, const void* d_base, uint32_t* d_crcs, hipStream_t s) {
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
  return S3H_OK;
}

}  // namespace

extern "C" {

int s3h_crc_plan_create(int device, int crc, const uint64_t* offsets, const uint64_t* lengths,
                        uint64_t n, s3h_crc_plan_t* plan) {
  if (!plan) return fail(S3H_EINVAL, "crc: null plan out-pointer");
  return crc_plan_build(device, crc, offsets, lengths, n, plan);
}

int s3h_crc_plan_launch(s3h_crc_plan_t P, const void* d_base, uint32_t* d_crcs, void* stream) {
  if (!P || !d_base || !d_crcs) return fail(S3H_EINVAL, "crc launch: null argument");
  return crc_plan_launch(P, d_base, d_crcs, static_cast<hipStream_t>(stream));
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
  delete P;
  return S3H_OK;
}

int s3h_crc_batch_device(int device, int crc, const void* d_base, const uint64_t* offsets,
                         const uint64_t* lengths, uint64_t n, uint32_t* d_crcs, void* stream) {
  if (int rc = check_crc_args(crc, offsets, lengths, n)) return rc;
  if (!d_base || !d_crcs) return fail(S3H_EINVAL, "crc batch: null argument");
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
  s3h_crc_plan_s* P = nullptr;
  if (int rc = crc_plan_build(device, crc, offsets, lengths, n, &P)) return rc;
  struct Cleanup {
    s3h_crc_plan_s* P;
    ~Cleanup() { s3h_crc_plan_destroy(P); }
  } cleanup{P};
  DeviceGuard g(device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t* d_crcs = nullptr;
  unsigned long long* d_count = nullptr;
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&d_crcs), n * 4, s));
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&d_count), 8, s));
  HIP_TRY(hipMemsetAsync(d_count, 0, 8, s));
  int rc = crc_plan_launch(P, d_base, d_crcs, s);
  if (rc == S3H_OK) {
    unsigned long long c = 0;
    hipError_t e = launch_compare_digests(d_crcs, d_expected, n, 1, d_mismatch, d_count, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&c, d_count, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = fail(S3H_EHIP, "crc verify: %s", hipGetErrorString(e));
    *mismatches = c;
  }
  (void)hipFreeAsync(d_crcs, s);
  (void)hipFreeAsync(d_count, s);
  (void)hipStreamSynchronize(s);
  return rc;
}

}  // extern "C"
