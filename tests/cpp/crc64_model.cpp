// crc64_model.cpp -- host model of the GPU CRC-64/NVME decomposition
// (s3client_amd/csrc/crc64_kernels.hip), built from the arithmetic headers the kernels use
// (crc64_math.hpp and the geometry of crc_math.hpp) and nothing else: 64 lanes as an array, the
// same tables, line masks, tile shifts, lane joins and segment folds, for whole-part launches
// and for ranged ones.  tests/test_crc64_cpu.py compiles it (also with
// -fsanitize=address,undefined) and compares with s3h_cpu_crc64nvme.
//
//   crc64_model LOG2_SEGMENT DATA_FILE PARTS_FILE            whole parts: one hex CRC per part
//   crc64_model LOG2_SEGMENT DATA_FILE PARTS_FILE CUT...     ranged: ascending range ends
//       (ranges [0, c1), [c1, c2), ...); per part "crc range", the hex CRC and the index of the
//       range that wrote it (-1: never written)
//   PARTS_FILE: "offset length" per line.
//
// Whole parts are read from a 16-byte-aligned buffer of exactly ceil(size / 16) lines; a
// range's bytes are first moved into a slot buffer (part j at j * slot, byte_origin =
// byte_begin) of exactly the lines copied: a model that read a line holding no byte of a part
// or range would run off the allocation.  A piece value is overwritten with garbage once
// stage 2 has folded it: a range may only read the piece values it wrote itself.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../s3client_amd/csrc/crc64_math.hpp"

namespace gf = s3h::crc64;
namespace geo = s3h::crc;
constexpr uint64_t kPoly = gf::kPolyNvme;

// Stage 1: one wave, one segment or piece [addr, addr + len), len >= 1 (crc64dev::segment_raw).
static uint64_t segment_raw(const uint64_t* T, uint64_t addr, uint64_t len) {
  const geo::SegGeom g = geo::seg_geom(addr, len);
  uint64_t r[64] = {0};
  for (uint32_t t = 0; t < g.tiles; ++t)
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t j = 64 * t + lane;
      uint32_t w[4] = {0, 0, 0, 0};
      if (j >= g.pad) {
        std::memcpy(w, reinterpret_cast<const void*>((g.first - g.pad + j) << 4), 16);
        const uint32_t lead = j == g.pad ? g.lead : 0, trail = j == 64 * g.tiles - 1 ? g.trail : 0;
        for (uint32_t i = 0; i < 4; ++i) w[i] &= geo::line_mask(i, lead, trail);
      }
      r[lane] = (t ? gf::mul_by_table(T + gf::kShiftAt, r[lane]) : uint64_t(0)) ^ gf::line_raw(T, w);
    }
  for (uint32_t lane = 0; lane < 64; ++lane) r[lane] = gf::mulmod(r[lane], T[gf::kLaneAt + lane], kPoly);
  for (uint32_t k = 0; k < 6; ++k) {
    uint64_t next[64];
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t from = lane + (1u << k) < 64 ? lane + (1u << k) : lane;  // shuffle down
      next[lane] = r[lane] ^ r[from];
    }
    std::memcpy(r, next, sizeof r);
  }
  return gf::mulmod(r[0], T[gf::kInvAt + g.trail], kPoly);
}

// Stage 2, the values in front of the last one (crc64dev::fold_front): lane 0's result.
static uint64_t fold_front(const uint64_t* v, uint64_t front, uint32_t log2s) {
  const uint64_t S = uint64_t(1) << log2s, c = (front + 63) >> 6, pad = 64 * c - front;
  const uint64_t xs = gf::xpow8(S, kPoly);
  uint64_t r[64] = {0};
  for (uint64_t lane = 0; lane < 64; ++lane)
    for (uint64_t i = 0; i < c; ++i) {
      const uint64_t j = lane * c + i;
      r[lane] = gf::mulmod(r[lane], xs, kPoly) ^ (j >= pad ? v[j - pad] : uint64_t(0));
    }
  if (c != 0) {
    uint64_t sh = gf::xpow8(c * S, kPoly);
    for (uint32_t k = 0; k < 6; ++k) {
      uint64_t next[64];
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t from = lane + (1u << k) < 64 ? lane + (1u << k) : lane;
        next[lane] = gf::mulmod(r[lane], sh, kPoly) ^ r[from];
      }
      std::memcpy(r, next, sizeof r);
      sh = gf::mulmod(sh, sh, kPoly);
    }
  }
  return r[0];
}

// Stage 2 of a whole-part launch (crc64_parts_kernel).
static uint64_t part_crc(const uint64_t* v, uint64_t len, uint32_t log2s) {
  if (len == 0) return 0;
  const uint64_t full = (len - 1) >> log2s;
  uint64_t r = fold_front(v, full, log2s);
  const uint64_t xt = gf::xpow8(len - (full << log2s), kPoly);
  r = full ? gf::mulmod(r, xt, kPoly) ^ v[full] : v[0];  // (one segment: tail == len, r == 0)
  const uint64_t xl = full ? gf::xpow8(len, kPoly) : xt;
  const uint64_t crc = gf::kAllOnes ^ gf::mulmod(gf::kAllOnes, xl, kPoly) ^ r;
  if (crc != gf::finalise(r, len, kPoly)) std::exit(5);  // the written-out form is finalise()
  return crc;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: crc64_model LOG2_SEGMENT DATA_FILE PARTS_FILE [CUT...]\n");
    return 2;
  }
  const uint32_t log2s = uint32_t(std::atoi(argv[1]));
  if (log2s < 4 || log2s > 30) return 2;
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  const uint64_t size = uint64_t(std::ftell(f));
  std::fseek(f, 0, SEEK_SET);
  const uint64_t alloc = ((size + 15) / 16) * 16;
  uint8_t* data = static_cast<uint8_t*>(std::aligned_alloc(16, alloc ? alloc : 16));
  if (!data || std::fread(data, 1, size, f) != size) return 2;
  std::fclose(f);
  std::memset(data + size, 0xA5, alloc - size);  // (masked out, never part of a CRC)

  std::vector<uint64_t> offs, lens, seg0;
  FILE* pf = std::fopen(argv[3], "r");
  if (!pf) return 2;
  unsigned long long off, len;
  uint64_t nseg = 0;
  const uint64_t S = uint64_t(1) << log2s;
  while (std::fscanf(pf, "%llu %llu", &off, &len) == 2) {
    if (off + len > size) return 2;
    offs.push_back(off);
    lens.push_back(len);
    seg0.push_back(nseg);
    nseg += (len + S - 1) >> log2s;
  }
  std::fclose(pf);
  const uint64_t n = lens.size();

  std::vector<uint64_t> T(gf::kTableWords);
  gf::build_device_tables(kPoly, T.data());
  std::vector<uint64_t> partials(nseg + 1, 0x5EED5EED5EED5EEDull);

  if (argc == 4) {  // whole parts
    for (uint64_t p = 0; p < n; ++p) {
      uint64_t* v = partials.data() + seg0[p];
      uint64_t k = 0;
      for (uint64_t done = 0; done < lens[p]; done += S)
        v[k++] = segment_raw(T.data(), reinterpret_cast<uint64_t>(data) + offs[p] + done,
                             lens[p] - done < S ? lens[p] - done : S);
      std::printf("%016llx\n", static_cast<unsigned long long>(part_crc(v, lens[p], log2s)));
    }
    std::free(data);
    return 0;
  }

  std::vector<uint64_t> cuts;
  for (int i = 4; i < argc; ++i) cuts.push_back(std::strtoull(argv[i], nullptr, 10));
  std::vector<uint64_t> state(n, 0xDEADBEEFDEADBEEFull), crcs(n, 0);
  std::vector<int> wrote(n, -1);
  uint64_t begin = 0;
  for (size_t ri = 0; ri < cuts.size(); begin = cuts[ri], ++ri) {
    const uint64_t end = cuts[ri];
    if (end <= begin) return 2;
    // the slot buffer of this range: part j's bytes [begin, min(end, len)) at j * slot
    const uint64_t slot = end - begin;
    uint64_t used = 0;
    for (uint64_t j = 0; j < n; ++j)
      if (lens[j] > begin) used = j * slot + ((end < lens[j] ? end : lens[j]) - begin);
    const uint64_t balloc = ((used + 15) / 16) * 16;
    uint8_t* buf = static_cast<uint8_t*>(std::aligned_alloc(16, balloc ? balloc : 16));
    if (!buf) return 2;
    std::memset(buf, 0xA5, balloc ? balloc : 16);
    for (uint64_t j = 0; j < n; ++j)
      if (lens[j] > begin)
        std::memcpy(buf + j * slot, data + offs[j] + begin, (end < lens[j] ? end : lens[j]) - begin);
    const uint64_t base = reinterpret_cast<uint64_t>(buf), origin = begin;

    // stage 1: wave w = piece k0 + w % nk of part w / nk
    const uint64_t k0 = geo::range_first_piece(begin, log2s), nk = geo::range_pieces(begin, end, log2s);
    for (uint64_t w = 0; w < n * nk; ++w) {
      const uint64_t part = w / nk, k = k0 + (w - part * nk);
      const geo::Piece pc = geo::piece_of(k, log2s, begin, end, lens[part]);
      if (pc.lo >= pc.hi) continue;
      if (seg0[part] + k >= nseg) return 3;  // (the kernel's store would leave the buffer)
      partials[seg0[part] + k] = segment_raw(T.data(), base + part * slot + (pc.lo - origin), pc.hi - pc.lo);
    }
    // stage 2: one wave per part
    for (uint64_t part = 0; part < n; ++part) {
      const geo::PartRange R = geo::part_range(lens[part], begin, end, log2s);
      if (R.bytes == 0) {
        if (R.emits) {
          if (wrote[part] >= 0) return 4;
          crcs[part] = 0;
          wrote[part] = int(ri);
        }
        continue;
      }
      uint64_t* v = partials.data() + seg0[part] + R.first;
      uint64_t r = fold_front(v, R.front, log2s);
      const uint64_t xt = gf::xpow8(R.tail, kPoly);
      r = R.front ? gf::mulmod(r, xt, kPoly) ^ v[R.front] : v[0];
      for (uint64_t i = 0; i <= R.front; ++i) v[i] = 0x5EED000000000000ull + ri;  // used up
      r = gf::range_state(begin ? state[part] : uint64_t(0), r, begin, R.bytes, kPoly);
      state[part] = r;
      if (R.emits) {
        if (wrote[part] >= 0) return 4;  // written twice
        const uint64_t xl = R.front == 0 && begin == 0 ? xt : gf::xpow8(lens[part], kPoly);
        crcs[part] = gf::kAllOnes ^ gf::mulmod(gf::kAllOnes, xl, kPoly) ^ r;
        if (crcs[part] != gf::finalise(r, lens[part], kPoly)) return 5;  // the written-out form is finalise()
        wrote[part] = int(ri);
      }
    }
    std::free(buf);
  }
  for (uint64_t part = 0; part < n; ++part)
    std::printf("%016llx %d\n", static_cast<unsigned long long>(crcs[part]), wrote[part]);
  std::free(data);
  return 0;
}
