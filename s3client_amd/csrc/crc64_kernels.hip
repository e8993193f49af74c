// crc64_kernels.hip -- batched CRC-64/NVME of device-resident parts (included by launch.hip).
// The decomposition is crc32_kernels.hip's with 64-bit values (crc64_math.hpp): a part is cut
// into segments, stage 1 gives each segment's raw value with one wave, stage 2 folds a part's
// values with one wave and finalises.
//
//   crc64_segments_kernel      stage 1 over a host-built segment table (whole-part launch)
//   crc64_parts_kernel         stage 2 of the whole-part launch
//   crc64_range_pieces_kernel  stage 1 of a ranged launch: one wave per (part, piece of the range)
//   crc64_range_parts_kernel   stage 2 of a ranged launch: folds into the part's running value
//
// LDS.  The tables are 64-bit: 16 x 256 slicing entries (32 KiB) + 8 x 256 tile-shift entries
// (16 KiB) + constants = 49,792 B per workgroup of 8 waves, so 3 workgroups (24 waves, 6 per
// SIMD) share a CU's 160 KiB.  A line costs 16 + 8 ds_read_b64 where the 32-bit kernel issues
// 16 + 4 ds_read_b32; a ds_read_b64 is serviced in the same two 32-lane groups over 64 banks as
// a ds_read_b32 over 32, so a random lookup conflicts alike in both and the expected price is
// the lookup count, 24 : 20.  The polynomial and every constant are data read from
// the plan.
//
// Every kernel here lives in a text section of its own and shares no device function with the
// 32-bit kernels, whose machine code is pinned (s3client_amd/kernel_isa_counts.json).
#pragma once
#include <hip/hip_runtime.h>

#include "crc64_math.hpp"
#include "kernel_abi.hpp"

namespace s3h {

namespace crc64dev {

using namespace s3h::crc64;
using s3h::crc::line_mask;
using s3h::crc::part_range;
using s3h::crc::PartRange;
using s3h::crc::Piece;
using s3h::crc::piece_of;
using s3h::crc::range_first_piece;
using s3h::crc::range_pieces;
using s3h::crc::seg_geom;
using s3h::crc::SegGeom;

// a 64-bit value from `delta` lanes up: two 32-bit shuffles
__device__ __forceinline__ uint64_t shfl_down64(uint64_t v, uint32_t delta) {
  const uint32_t lo = __shfl_down(uint32_t(v), delta, 64);
  const uint32_t hi = __shfl_down(uint32_t(v >> 32), delta, 64);
  return uint64_t(hi) << 32 | lo;
}

// One lane's 16-byte line: 16 lookups in the slicing tables (LDS), state 0.
__device__ __forceinline__ uint64_t line16(const uint64_t* T, uint32_t x, uint32_t y, uint32_t z,
                                           uint32_t w) {
  uint64_t r;
  r = T[15 * 256 + (x & 0xFFu)] ^ T[14 * 256 + ((x >> 8) & 0xFFu)];
  r ^= T[13 * 256 + ((x >> 16) & 0xFFu)] ^ T[12 * 256 + (x >> 24)];
  r ^= T[11 * 256 + (y & 0xFFu)] ^ T[10 * 256 + ((y >> 8) & 0xFFu)];
  r ^= T[9 * 256 + ((y >> 16) & 0xFFu)] ^ T[8 * 256 + (y >> 24)];
  r ^= T[7 * 256 + (z & 0xFFu)] ^ T[6 * 256 + ((z >> 8) & 0xFFu)];
  r ^= T[5 * 256 + ((z >> 16) & 0xFFu)] ^ T[4 * 256 + (z >> 24)];
  r ^= T[3 * 256 + (w & 0xFFu)] ^ T[2 * 256 + ((w >> 8) & 0xFFu)];
  r ^= T[1 * 256 + ((w >> 16) & 0xFFu)] ^ T[w >> 24];
  return r;
}

// The lane's running value moved one tile (1 KiB) on, plus the lane's line of that tile.
__device__ __forceinline__ uint64_t tile_step(const uint64_t* T, uint64_t r, const uint4& d) {
  return mul_by_table(T + kShiftAt, r) ^ line16(T, d.x, d.y, d.z, d.w);
}

__device__ __forceinline__ uint4 mask_line(uint4 d, uint32_t lead, uint32_t trail) {
  d.x &= line_mask(0, lead, trail);
  d.y &= line_mask(1, lead, trail);
  d.z &= line_mask(2, lead, trail);
  d.w &= line_mask(3, lead, trail);
  return d;
}

__device__ __forceinline__ void load_tables(uint64_t* T, const uint64_t* tables) {
  for (uint32_t i = threadIdx.x; i < kTableWords / 2; i += kCrc64SegThreads)
    reinterpret_cast<uint4*>(T)[i] = reinterpret_cast<const uint4*>(tables)[i];
  __syncthreads();
}

// Stage 1 of one wave: the raw value of bytes [base + off, base + off + len), len >= 1 (valid
// in lane 0).  The wave reads the 16-byte-aligned lines that hold at least one of the segment's
// bytes and nothing else: one dwordx4 per lane and tile, virtual zero lines in front of the
// first one (free with init 0), the bytes of the first and last line outside the segment
// masked to zero -- the k trailing zeros are undone by x^(-8k).
__device__ __forceinline__ uint64_t segment_raw(const uint64_t* T, const uint8_t* base, uint64_t off,
                                                uint64_t len, uint64_t poly, uint32_t lane) {
  const SegGeom g = seg_geom(reinterpret_cast<uint64_t>(base) + off, len);
  // the lane's line of tile t is p[64 * t]; in tile 0 the lanes below g.pad have none
  // (an offset from the base pointer, not a cast of the address: the loads stay global loads)
  const uint4* p = reinterpret_cast<const uint4*>(
      base + (((g.first - g.pad + lane) << 4) - reinterpret_cast<uint64_t>(base)));
  const uint32_t last = g.tiles - 1;
  uint4 d = make_uint4(0, 0, 0, 0);
  if (lane >= g.pad) d = p[0];
  if (lane == g.pad) d = mask_line(d, g.lead, 0);
  if (last == 0 && lane == 63) d = mask_line(d, 0, g.trail);
  uint64_t r = line16(T, d.x, d.y, d.z, d.w);
  uint32_t t = 1;
  for (; t + 4 <= last; t += 4) {  // whole tiles, four loads in flight per lane
    const uint4 d0 = p[64 * t], d1 = p[64 * t + 64], d2 = p[64 * t + 128], d3 = p[64 * t + 192];
    r = tile_step(T, r, d0);
    r = tile_step(T, r, d1);
    r = tile_step(T, r, d2);
    r = tile_step(T, r, d3);
  }
  for (; t < last; ++t) r = tile_step(T, r, p[64 * t]);
  if (last != 0) {
    d = p[64 * uint64_t(last)];
    if (lane == 63) d = mask_line(d, 0, g.trail);
    r = tile_step(T, r, d);
  }
  // lane l's lines are followed by 63 - l lines of the last tile: one multiplication per lane
  // moves its value there, an xor reduction joins the lanes
  r = mulmod(r, T[kLaneAt + lane], poly);
  for (uint32_t k = 0; k < 6; ++k) r ^= shfl_down64(r, 1u << k);
  return mulmod(r, T[kInvAt + g.trail], poly);
}

// Stage 2 of one wave: the part's `front` values v[0 .. front) of S = 2^log2s bytes each,
// padded in front with virtual zero values to 64 runs of c; lane l folds run l (Horner with
// x^(8S)) and a 6-step tree joins the runs (valid in lane 0; 0 when front == 0).
__device__ __forceinline__ uint64_t fold_front(const uint64_t* v, uint64_t front, uint32_t log2s,
                                               uint64_t x_segment, uint64_t poly, uint32_t lane) {
  const uint64_t S = uint64_t(1) << log2s;
  const uint64_t c = (front + 63) >> 6, pad = 64 * c - front;
  uint64_t r = 0;
  for (uint64_t i = 0; i < c; ++i) {
    const uint64_t j = lane * c + i;
    r = mulmod(r, x_segment, poly) ^ (j >= pad ? v[j - pad] : uint64_t(0));
  }
  if (c != 0) {
    uint64_t sh = xpow8(c * S, poly);
    for (uint32_t k = 0; k < 6; ++k) {
      const uint64_t o = shfl_down64(r, 1u << k);
      r = mulmod(r, sh, poly) ^ o;
      sh = mulmod(sh, sh, poly);
    }
  }
  return r;
}

}  // namespace crc64dev

#define S3H_CRC64_TEXT __attribute__((section(".text.s3h_crc64")))
// Stage 1 wants its 3 workgroups per CU resident at once: 6 waves per SIMD, at most 84 VGPRs.
#define S3H_CRC64_STAGE1 S3H_CRC64_TEXT __attribute__((amdgpu_waves_per_eu(6)))

// Stage 1, whole parts.  Workgroup = 8 waves; the tables are copied to LDS once per workgroup
// and each wave then takes segments blockIdx * 8 + wave, + gridDim * 8, ...
__global__ __launch_bounds__(kCrc64SegThreads) S3H_CRC64_STAGE1 void crc64_segments_kernel(Crc64Args A) {
  using namespace crc64dev;
  __shared__ uint64_t T[kTableWords];
  load_tables(T, A.tables);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr uint32_t kWaves = kCrc64SegThreads / 64;
  for (uint64_t s = uint64_t(blockIdx.x) * kWaves + wave; s < A.nseg; s += uint64_t(gridDim.x) * kWaves) {
    const CrcSeg seg = A.segs[s];
    const uint64_t r = segment_raw(T, A.base, seg.off, seg.len, A.poly, lane);
    if (lane == 0) A.partials[s] = r;
  }
}

// Stage 2, whole parts.  One wave per part: the full segments in front of the last one through
// fold_front, then lane 0 appends the last segment and finalises.
__global__ __launch_bounds__(kCrc64PartThreads) S3H_CRC64_TEXT void crc64_parts_kernel(Crc64Args A) {
  using namespace crc64dev;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t part = uint64_t(blockIdx.x) * (kCrc64PartThreads / 64) +
                        __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (part >= A.n) return;
  const CrcPart q = A.parts[part];
  if (q.len == 0) {
    if (lane == 0) A.crcs[part] = 0;
    return;
  }
  const uint64_t full = (q.len - 1) >> A.log2_segment;  // segments in front of the last one
  const uint64_t* v = A.partials + q.seg0;
  uint64_t r = fold_front(v, full, A.log2_segment, A.x_segment, A.poly, lane);
  if (lane == 0) {
    const uint64_t tail = q.len - (full << A.log2_segment);  // 1..S bytes
    const uint64_t xt = xpow8(tail, A.poly);
    // (a part of one segment -- most parts of a ragged batch -- has tail == len and r == 0:
    // one square-and-multiply instead of two)
    r = full ? mulmod(r, xt, A.poly) ^ v[full] : v[0];
    const uint64_t xl = full ? xpow8(q.len, A.poly) : xt;
    A.crcs[part] = kAllOnes ^ mulmod(kAllOnes, xl, A.poly) ^ r;  // finalise()
  }
}

// Ranged stage 1: the pieces derived on the device.  Wave w takes piece k0 + w % nk of part
// w / nk (grid-stride; k0, nk: the launch's pieces per part, crc_math.hpp) and goes on at once
// when the piece is empty -- the part ends in front of it.
__global__ __launch_bounds__(kCrc64SegThreads) S3H_CRC64_STAGE1 void crc64_range_pieces_kernel(Crc64Args A) {
  using namespace crc64dev;
  __shared__ uint64_t T[kTableWords];
  load_tables(T, A.tables);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr uint32_t kWaves = kCrc64SegThreads / 64;
  const uint64_t k0 = range_first_piece(A.begin, A.log2_segment);
  const uint64_t nk = range_pieces(A.begin, A.end, A.log2_segment);
  const uint64_t total = A.n * nk;
  for (uint64_t w = uint64_t(blockIdx.x) * kWaves + wave; w < total; w += uint64_t(gridDim.x) * kWaves) {
    const uint64_t part = nk == 1 ? w : w / nk, k = k0 + (w - part * nk);
    const CrcPart q = A.parts[part];
    const Piece pc = piece_of(k, A.log2_segment, A.begin, A.end, q.len);
    if (pc.lo >= pc.hi) continue;
    const uint64_t r = segment_raw(T, A.base, A.offs[part] + (pc.lo - A.origin), pc.hi - pc.lo, A.poly, lane);
    if (lane == 0) A.partials[q.seg0 + k] = r;
  }
}

// Ranged stage 2: one wave per part folds the part's pieces of this launch (the first may be
// short in front: leading zeros), moves the part's running value on by the bytes of the range
// and adds them, and finalises the parts whose last byte the range holds.  Parts with no byte
// in the range are left alone.
__global__ __launch_bounds__(kCrc64PartThreads) S3H_CRC64_TEXT void crc64_range_parts_kernel(Crc64Args A) {
  using namespace crc64dev;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t part = uint64_t(blockIdx.x) * (kCrc64PartThreads / 64) +
                        __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (part >= A.n) return;
  const CrcPart q = A.parts[part];
  const PartRange R = part_range(q.len, A.begin, A.end, A.log2_segment);
  if (R.bytes == 0) {
    if (R.emits && lane == 0) A.crcs[part] = 0;  // an empty part
    return;
  }
  const uint64_t* v = A.partials + q.seg0 + R.first;
  uint64_t r = fold_front(v, R.front, A.log2_segment, A.x_segment, A.poly, lane);
  if (lane == 0) {
    const uint64_t xt = xpow8(R.tail, A.poly);
    r = R.front ? mulmod(r, xt, A.poly) ^ v[R.front] : v[0];
    r = range_state(A.begin ? A.state[part] : uint64_t(0), r, A.begin, R.bytes, A.poly);
    A.state[part] = r;
    if (R.emits) {
      // (a whole part in one piece -- the host path's groups of small parts -- has tail == len)
      const uint64_t xl = R.front == 0 && A.begin == 0 ? xt : xpow8(q.len, A.poly);
      A.crcs[part] = kAllOnes ^ mulmod(kAllOnes, xl, A.poly) ^ r;  // finalise()
    }
  }
}

}  // namespace s3h
