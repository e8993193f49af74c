// crc32_kernels.hip -- batched CRC-32C / CRC-32 of device-resident parts (included by
// launch.hip).  A CRC is linear over GF(2) (crc_math.hpp), so a part is cut into segments that
// are checksummed independently and folded: the one S3 digest that uses the whole chip for a
// single part.  Two launches on the caller's stream, no inter-workgroup waits:
//
//   crc_segments_kernel  stage 1: one wave per segment (grid-stride), raw value (init 0, no
//                        xor-out) of the segment into the plan's partials buffer
//   crc_parts_kernel     stage 2: one wave per part folds the part's segment values in order
//                        and applies init / xor-out through the closed form
//
// A RANGED launch (bytes [begin, end) of every part, the running value kept per part between
// launches) is the same two stages over the pieces of that range, derived on the device:
//
//   crc_range_pieces_kernel  stage 1: one wave per (part, piece of the range)
//   crc_range_parts_kernel   stage 2: one wave per part folds its pieces into the part's state
//                            and finalises the parts that end in the range
//
// The polynomial is data: both kernels read it, the lookup tables and every constant from the
// plan (built by crc_math.hpp build_device_tables on the host).
#pragma once
#include <hip/hip_runtime.h>

#include "crc_math.hpp"
#include "kernel_abi.hpp"

namespace s3h {

namespace crcdev {

using namespace s3h::crc;

// One lane's 16-byte line: 16 lookups in the slicing tables (LDS), state 0.
__device__ __forceinline__ uint32_t line16(const uint32_t* T, uint32_t x, uint32_t y, uint32_t z,
                                           uint32_t w) {
  uint32_t r;
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
__device__ __forceinline__ uint32_t tile_step(const uint32_t* T, uint32_t r, const uint4& d) {
  return mul_by_table(T + kShiftAt, r) ^ line16(T, d.x, d.y, d.z, d.w);
}

__device__ __forceinline__ uint4 mask_line(uint4 d, uint32_t lead, uint32_t trail) {
  d.x &= line_mask(0, lead, trail);
  d.y &= line_mask(1, lead, trail);
  d.z &= line_mask(2, lead, trail);
  d.w &= line_mask(3, lead, trail);
  return d;
}

// The ranged kernels' stages as functions of one wave.  (crc_segments_kernel and
// crc_parts_kernel below keep their own text of the same steps: their machine code is the one
// the profiles were taken with, and sharing these functions with them changed it.)
//
// Stage 1: the raw value of bytes [base + off, base + off + len), len >= 1, as described at
// crc_segments_kernel (valid in lane 0).
__device__ __forceinline__ uint32_t segment_raw(const uint32_t* T, const uint8_t* base, uint64_t off,
                                                uint64_t len, uint32_t poly, uint32_t lane) {
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
  uint32_t r = line16(T, d.x, d.y, d.z, d.w);
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
  // lane l's lines are followed by 63 - l lines of the last tile: a 6-step tree, step k
  // moves the left value 2^k lines on
  for (uint32_t k = 0; k < 6; ++k) {
    const uint32_t o = __shfl_down(r, 1u << k, 64);
    r = mulmod(r, T[kTreeAt + k], poly) ^ o;  // (kept by lanes that are multiples of 2^(k+1))
  }
  return mulmod(r, T[kInvAt + g.trail], poly);
}

// Stage 2: the part's `front` values v[0 .. front) of S = 2^log2s bytes each, folded as
// described at crc_parts_kernel (valid in lane 0; 0 when front == 0).
__device__ __forceinline__ uint32_t fold_front(const uint32_t* v, uint64_t front, uint32_t log2s,
                                               uint32_t x_segment, uint32_t poly, uint32_t lane) {
  const uint64_t S = uint64_t(1) << log2s;
  const uint64_t c = (front + 63) >> 6, pad = 64 * c - front;
  uint32_t r = 0;
  for (uint64_t i = 0; i < c; ++i) {
    const uint64_t j = lane * c + i;
    r = mulmod(r, x_segment, poly) ^ (j >= pad ? v[j - pad] : 0u);
  }
  if (c != 0) {
    uint32_t sh = xpow8(c * S, poly);
    for (uint32_t k = 0; k < 6; ++k) {
      const uint32_t o = __shfl_down(r, 1u << k, 64);
      r = mulmod(r, sh, poly) ^ o;
      sh = mulmod(sh, sh, poly);
    }
  }
  return r;
}

}  // namespace crcdev

// Stage 1.  Workgroup = 8 waves; the tables (20.5 KiB) are copied to LDS once per workgroup and
// each wave then takes segments blockIdx * 8 + wave, + gridDim * 8, ...  Of a segment
// [addr, addr + len) the wave reads the 16-byte-aligned lines that hold at least one of its
// bytes and nothing else: one dwordx4 per lane, 1 KiB per wave-instruction, lines in front of
// the first one are virtual zeros (free with init 0), and the bytes of the first and last
// line outside the segment are masked to zero -- the k trailing zeros are undone by x^(-8k).
__global__ __launch_bounds__(kCrcSegThreads) void crc_segments_kernel(CrcSegArgs A) {
  using namespace crcdev;
  __shared__ uint32_t T[kTableWords];
  for (uint32_t i = threadIdx.x; i < kTableWords / 4; i += kCrcSegThreads)
    reinterpret_cast<uint4*>(T)[i] = reinterpret_cast<const uint4*>(A.tables)[i];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr uint32_t kWaves = kCrcSegThreads / 64;
  for (uint64_t s = uint64_t(blockIdx.x) * kWaves + wave; s < A.nseg; s += uint64_t(gridDim.x) * kWaves) {
    const CrcSeg seg = A.segs[s];
    const SegGeom g = seg_geom(reinterpret_cast<uint64_t>(A.base) + seg.off, seg.len);
    // the lane's line of tile t is p[64 * t]; in tile 0 the lanes below g.pad have none
    // (an offset from the base pointer, not a cast of the address: the loads stay global loads)
    const uint4* p = reinterpret_cast<const uint4*>(
        A.base + (((g.first - g.pad + lane) << 4) - reinterpret_cast<uint64_t>(A.base)));
    const uint32_t last = g.tiles - 1;
    uint4 d = make_uint4(0, 0, 0, 0);
    if (lane >= g.pad) d = p[0];
    if (lane == g.pad) d = mask_line(d, g.lead, 0);
    if (last == 0 && lane == 63) d = mask_line(d, 0, g.trail);
    uint32_t r = line16(T, d.x, d.y, d.z, d.w);
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
    // lane l's lines are followed by 63 - l lines of the last tile: a 6-step tree, step k
    // moves the left value 2^k lines on
    for (uint32_t k = 0; k < 6; ++k) {
      const uint32_t o = __shfl_down(r, 1u << k, 64);
      r = mulmod(r, T[kTreeAt + k], A.poly) ^ o;  // (kept by lanes that are multiples of 2^(k+1))
    }
    if (lane == 0) A.partials[s] = mulmod(r, T[kInvAt + g.trail], A.poly);
  }
}

// Stage 2.  One wave per part.  The part's full segments (all but the last) are padded in front
// with virtual zero values to 64 runs of c segments; lane l folds run l (Horner with x^(8S)),
// a 6-step tree joins the runs (step k moves the left value c * 2^k segments on), and lane 0
// appends the last segment (x^(8 * its length) by square-and-multiply) and finalises.
__global__ __launch_bounds__(kCrcPartThreads) void crc_parts_kernel(CrcPartArgs A) {
  using namespace s3h::crc;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t part = uint64_t(blockIdx.x) * (kCrcPartThreads / 64) +
                        __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (part >= A.n) return;
  const CrcPart q = A.parts[part];
  if (q.len == 0) {
    if (lane == 0) A.crcs[part] = 0;
    return;
  }
  const uint64_t S = uint64_t(1) << A.log2_segment;
  const uint64_t full = (q.len - 1) >> A.log2_segment;  // segments in front of the last one
  const uint64_t c = (full + 63) >> 6, pad = 64 * c - full;
  const uint32_t* v = A.partials + q.seg0;
  uint32_t r = 0;
  for (uint64_t i = 0; i < c; ++i) {
    const uint64_t j = lane * c + i;
    r = mulmod(r, A.x_segment, A.poly) ^ (j >= pad ? v[j - pad] : 0u);
  }
  if (c != 0) {
    uint32_t sh = xpow8(c * S, A.poly);
    for (uint32_t k = 0; k < 6; ++k) {
      const uint32_t o = __shfl_down(r, 1u << k, 64);
      r = mulmod(r, sh, A.poly) ^ o;
      sh = mulmod(sh, sh, A.poly);
    }
  }
  if (lane == 0) {
    const uint64_t tail = q.len - full * S;  // 1..S bytes
    r = mulmod(r, xpow8(tail, A.poly), A.poly) ^ v[full];
    A.crcs[part] = finalise(r, q.len, A.poly);
  }
}

// The ranged kernels live in a text section of their own, like the template kernels: the padding
// the assembler puts at the end of .text then still follows crc_parts_kernel, and that padding is
// part of the kernel's pinned code hash (tools/code_object.py hashes up to the next symbol).
#define S3H_CRC_RANGE_TEXT __attribute__((section(".text.s3h_crc_range")))

// Ranged stage 1: crc_segments_kernel with the pieces derived on the device.  Wave w takes
// piece k0 + w % nk of part w / nk (grid-stride; k0, nk: the launch's pieces per part,
// crc_math.hpp) and goes on at once when the piece is empty -- the part ends in front of it.
__global__ __launch_bounds__(kCrcSegThreads) S3H_CRC_RANGE_TEXT void crc_range_pieces_kernel(CrcRangeArgs A) {
  using namespace crcdev;
  __shared__ uint32_t T[kTableWords];
  for (uint32_t i = threadIdx.x; i < kTableWords / 4; i += kCrcSegThreads)
    reinterpret_cast<uint4*>(T)[i] = reinterpret_cast<const uint4*>(A.tables)[i];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr uint32_t kWaves = kCrcSegThreads / 64;
  const uint64_t k0 = range_first_piece(A.begin, A.log2_segment);
  const uint64_t nk = range_pieces(A.begin, A.end, A.log2_segment);
  const uint64_t total = A.n * nk;
  for (uint64_t w = uint64_t(blockIdx.x) * kWaves + wave; w < total; w += uint64_t(gridDim.x) * kWaves) {
    const uint64_t part = nk == 1 ? w : w / nk, k = k0 + (w - part * nk);
    const CrcPart q = A.parts[part];
    const Piece pc = piece_of(k, A.log2_segment, A.begin, A.end, q.len);
    if (pc.lo >= pc.hi) continue;
    const uint32_t r = segment_raw(T, A.base, A.offs[part] + (pc.lo - A.origin), pc.hi - pc.lo, A.poly, lane);
    if (lane == 0) A.partials[q.seg0 + k] = r;
  }
}

// Ranged stage 2: one wave per part folds the part's pieces of this launch as crc_parts_kernel
// folds segments (the first piece may be short in front: leading zeros), moves the part's
// running value on by the bytes of the range and adds them, and finalises the parts whose
// last byte the range holds.  Parts with no byte in the range are left alone.
__global__ __launch_bounds__(kCrcPartThreads) S3H_CRC_RANGE_TEXT void crc_range_parts_kernel(CrcRangeArgs A) {
  using namespace s3h::crc;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t part = uint64_t(blockIdx.x) * (kCrcPartThreads / 64) +
                        __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (part >= A.n) return;
  const CrcPart q = A.parts[part];
  const PartRange R = part_range(q.len, A.begin, A.end, A.log2_segment);
  if (R.bytes == 0) {
    if (R.emits && lane == 0) A.crcs[part] = 0;  // an empty part
    return;
  }
  const uint32_t* v = A.partials + q.seg0 + R.first;
  uint32_t r = crcdev::fold_front(v, R.front, A.log2_segment, A.x_segment, A.poly, lane);
  if (lane == 0) {
    r = mulmod(r, xpow8(R.tail, A.poly), A.poly) ^ v[R.front];
    r = range_state(A.begin ? A.state[part] : 0u, r, A.begin, R.bytes, A.poly);
    A.state[part] = r;
    if (R.emits) A.crcs[part] = range_emit(r, q.len, A.poly);
  }
}

}  // namespace s3h
