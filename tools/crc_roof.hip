// crc_roof.hip -- the read roof of the CRC segment kernel, for tools/crc_bench.py only (never
// part of libs3hash.so): the same grid, the same segment table and the same 16-byte-aligned
// dwordx4 loads as crc_segments_kernel (s3client_amd/csrc/crc32_kernels.hip), with the table
// lookups replaced by an XOR of the loaded words.  One word per segment is stored so the loads
// stay live.
//
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o tools/libcrc_roof.so tools/crc_roof.hip
#include <hip/hip_runtime.h>

#include "../s3client_amd/csrc/crc_math.hpp"
#include "../s3client_amd/csrc/kernel_abi.hpp"

namespace {

__global__ __launch_bounds__(s3h::kCrcSegThreads) void read_roof_kernel(const uint8_t* base,
                                                                        const s3h::CrcSeg* segs,
                                                                        uint64_t nseg, uint32_t* out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr uint32_t kWaves = s3h::kCrcSegThreads / 64;
  for (uint64_t s = uint64_t(blockIdx.x) * kWaves + wave; s < nseg; s += uint64_t(gridDim.x) * kWaves) {
    const s3h::CrcSeg seg = segs[s];
    const s3h::crc::SegGeom g = s3h::crc::seg_geom(reinterpret_cast<uint64_t>(base) + seg.off, seg.len);
    // (an offset from the base pointer, not a cast of the address: the loads stay global loads)
    const uint4* p = reinterpret_cast<const uint4*>(
        base + (((g.first - g.pad + lane) << 4) - reinterpret_cast<uint64_t>(base)));
    uint4 a = make_uint4(0, 0, 0, 0);
    if (lane >= g.pad) a = p[0];
    uint32_t t = 1;
    for (; t + 4 <= g.tiles; t += 4) {
      const uint4 d0 = p[64 * t], d1 = p[64 * t + 64], d2 = p[64 * t + 128], d3 = p[64 * t + 192];
      a.x ^= d0.x ^ d1.x ^ d2.x ^ d3.x;
      a.y ^= d0.y ^ d1.y ^ d2.y ^ d3.y;
      a.z ^= d0.z ^ d1.z ^ d2.z ^ d3.z;
      a.w ^= d0.w ^ d1.w ^ d2.w ^ d3.w;
    }
    for (; t < g.tiles; ++t) {
      const uint4 d = p[64 * t];
      a.x ^= d.x, a.y ^= d.y, a.z ^= d.z, a.w ^= d.w;
    }
    uint32_t r = a.x ^ a.y ^ a.z ^ a.w;
    for (uint32_t k = 1; k < 64; k <<= 1) r ^= __shfl_down(r, k, 64);
    if (lane == 0) out[s] = r;
  }
}

}  // namespace

extern "C" int crc_roof_launch(const void* d_base, const void* d_segs, uint64_t nseg, uint32_t grid,
                               uint32_t* d_out, void* stream) {
  hipLaunchKernelGGL(read_roof_kernel, dim3(grid), dim3(s3h::kCrcSegThreads), 0,
                     static_cast<hipStream_t>(stream), static_cast<const uint8_t*>(d_base),
                     static_cast<const s3h::CrcSeg*>(d_segs), nseg, d_out);
  return int(hipGetLastError());
}
