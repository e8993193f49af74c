// crc_model.cpp -- host model of the GPU CRC decomposition (s3client_amd/csrc/crc32_kernels.hip),
// built from the arithmetic header the kernels use (crc_math.hpp) and nothing else: 64 lanes as
// an array, the same tables, line masks, tile shifts, lane trees and segment folds.
// tests/test_crc_cpu.py compiles it (also with -fsanitize=address,undefined), feeds it ragged
// part lists at a reduced segment size and compares with s3h_cpu_crc.
//
//   crc_model CRC LOG2_SEGMENT DATA_FILE PARTS_FILE   (CRC: 0 = CRC-32C, 1 = CRC-32;
//   PARTS_FILE: "offset length" per line)  ->  one hex CRC per part on stdout
//
// The data is held in a 16-byte-aligned buffer of exactly ceil(size / 16) lines, so a model
// that read a line holding no byte of any part would run off the allocation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../s3client_amd/csrc/crc_math.hpp"

namespace gf = s3h::crc;

// Stage 1: one wave, one segment [addr, addr + len), len >= 1 (crc_segments_kernel).
static uint32_t segment_raw(const uint32_t* T, uint32_t poly, uint64_t addr, uint64_t len) {
  const gf::SegGeom g = gf::seg_geom(addr, len);
  uint32_t r[64] = {0};
  for (uint32_t t = 0; t < g.tiles; ++t)
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t j = 64 * t + lane;
      uint32_t w[4] = {0, 0, 0, 0};
      if (j >= g.pad) {
        std::memcpy(w, reinterpret_cast<const void*>((g.first - g.pad + j) << 4), 16);
        const uint32_t lead = j == g.pad ? g.lead : 0, trail = j == 64 * g.tiles - 1 ? g.trail : 0;
        for (uint32_t i = 0; i < 4; ++i) w[i] &= gf::line_mask(i, lead, trail);
      }
      r[lane] = (t ? gf::mul_by_table(T + gf::kShiftAt, r[lane]) : 0u) ^ gf::line_raw(T, w);
    }
  for (uint32_t k = 0; k < 6; ++k) {
    uint32_t next[64];
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t from = lane + (1u << k) < 64 ? lane + (1u << k) : lane;  // shuffle down
      next[lane] = gf::mulmod(r[lane], T[gf::kTreeAt + k], poly) ^ r[from];
    }
    std::memcpy(r, next, sizeof r);
  }
  return gf::mulmod(r[0], T[gf::kInvAt + g.trail], poly);
}

// Stage 2: one wave, one part of `len` bytes whose segment values are v[] (crc_parts_kernel).
static uint32_t part_crc(const uint32_t* v, uint64_t len, uint32_t log2s, uint32_t poly) {
  if (len == 0) return 0;
  const uint64_t S = uint64_t(1) << log2s, full = (len - 1) >> log2s;
  const uint64_t c = (full + 63) >> 6, pad = 64 * c - full;
  const uint32_t xs = gf::xpow8(S, poly);
  uint32_t r[64] = {0};
  for (uint64_t lane = 0; lane < 64; ++lane)
    for (uint64_t i = 0; i < c; ++i) {
      const uint64_t j = lane * c + i;
      r[lane] = gf::mulmod(r[lane], xs, poly) ^ (j >= pad ? v[j - pad] : 0u);
    }
  if (c != 0) {
    uint32_t sh = gf::xpow8(c * S, poly);
    for (uint32_t k = 0; k < 6; ++k) {
      uint32_t next[64];
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t from = lane + (1u << k) < 64 ? lane + (1u << k) : lane;
        next[lane] = gf::mulmod(r[lane], sh, poly) ^ r[from];
      }
      std::memcpy(r, next, sizeof r);
      sh = gf::mulmod(sh, sh, poly);
    }
  }
  const uint32_t raw = gf::mulmod(r[0], gf::xpow8(len - full * S, poly), poly) ^ v[full];
  return gf::finalise(raw, len, poly);
}

int main(int argc, char** argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: crc_model CRC LOG2_SEGMENT DATA_FILE PARTS_FILE\n");
    return 2;
  }
  const uint32_t poly = std::atoi(argv[1]) == 0 ? gf::kPolyCrc32c : gf::kPolyCrc32;
  const uint32_t log2s = uint32_t(std::atoi(argv[2]));
  if (log2s < 4 || log2s > 30) return 2;
  FILE* f = std::fopen(argv[3], "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  const uint64_t size = uint64_t(std::ftell(f));
  std::fseek(f, 0, SEEK_SET);
  const uint64_t alloc = ((size + 15) / 16) * 16;
  uint8_t* data = static_cast<uint8_t*>(std::aligned_alloc(16, alloc ? alloc : 16));
  if (!data || std::fread(data, 1, size, f) != size) return 2;
  std::fclose(f);
  std::memset(data + size, 0xA5, alloc - size);  // (masked out, never part of a CRC)

  std::vector<uint32_t> T(gf::kTableWords);
  gf::build_device_tables(poly, T.data());

  FILE* pf = std::fopen(argv[4], "r");
  if (!pf) return 2;
  unsigned long long off, len;
  const uint64_t S = uint64_t(1) << log2s;
  std::vector<uint32_t> v;
  while (std::fscanf(pf, "%llu %llu", &off, &len) == 2) {
    if (off + len > size) return 2;
    v.clear();
    for (uint64_t done = 0; done < len; done += S)
      v.push_back(segment_raw(T.data(), poly, reinterpret_cast<uint64_t>(data) + off + done,
                              len - done < S ? len - done : S));
    std::printf("%08x\n", part_crc(v.data(), len, log2s, poly));
  }
  std::fclose(pf);
  std::free(data);
  return 0;
}
