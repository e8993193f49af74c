// crc_range_model.cpp -- host model of the RANGED CRC launches (crc_range_pieces_kernel,
// crc_range_parts_kernel in s3client_amd/csrc/crc32_kernels.hip), built from crc_math.hpp alone:
// the piece geometry the kernels call (range_first_piece, range_pieces, piece_of, part_range,
// range_state, range_emit), 64 lanes as an array, the same tables and folds.  It walks a list of
// ranges as a caller of s3h_crc_plan_launch_range would: pieces of each range into the part's
// slots of the partials buffer, fold into the part's running value, CRC written by the range
// that holds the part's last byte.  tests/test_crc_range_cpu.py compiles it (also with
// -fsanitize=address,undefined) and compares with s3h_cpu_crc / zlib.
//
//   crc_range_model CRC LOG2_SEGMENT DATA_FILE PARTS_FILE CUT...
//     CRC: 0 = CRC-32C, 1 = CRC-32; PARTS_FILE: "offset length" per line; CUT...: ascending
//     range ends (ranges [0, c1), [c1, c2), ...), or the one word every:STEP:END
//   ->  per part "crc range" on stdout: the hex CRC and the index of the range that wrote it
//       (-1: never written)
//
// Each range's bytes are first moved into a scratch buffer the way the host pipeline lays out a
// ring slot -- part j at j * slot, read with byte_origin = byte_begin -- held in 16-byte lines of
// exactly the bytes copied, so a model that read a line holding no byte of the range would run
// off the allocation.  A piece value is overwritten with garbage once stage 2 has folded it: a
// range may only read the piece values it wrote itself.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../s3client_amd/csrc/crc_math.hpp"

namespace gf = s3h::crc;

// Stage 1: one wave, one piece [addr, addr + len), len >= 1 (crcdev::segment_raw).
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

// Stage 2, the values in front of the last one (crcdev::fold_front): lane 0's result.
static uint32_t fold_front(const uint32_t* v, uint64_t front, uint32_t log2s, uint32_t poly) {
  const uint64_t S = uint64_t(1) << log2s, c = (front + 63) >> 6, pad = 64 * c - front;
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
  return r[0];
}

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: crc_range_model CRC LOG2_SEGMENT DATA_FILE PARTS_FILE CUT...\n");
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
  std::vector<uint8_t> data(size);
  if (std::fread(data.data(), 1, size, f) != size) return 2;
  std::fclose(f);

  std::vector<uint64_t> offs, lens, seg0;
  FILE* pf = std::fopen(argv[4], "r");
  if (!pf) return 2;
  unsigned long long off, len;
  uint64_t nseg = 0;
  while (std::fscanf(pf, "%llu %llu", &off, &len) == 2) {
    if (off + len > size) return 2;
    offs.push_back(off);
    lens.push_back(len);
    seg0.push_back(nseg);
    nseg += (len + (uint64_t(1) << log2s) - 1) >> log2s;
  }
  std::fclose(pf);
  const uint64_t n = lens.size();

  std::vector<uint64_t> cuts;
  if (std::strncmp(argv[5], "every:", 6) == 0) {
    unsigned long long step = 0, end = 0;
    if (std::sscanf(argv[5], "every:%llu:%llu", &step, &end) != 2 || step == 0) return 2;
    for (uint64_t c = step; c < end; c += step) cuts.push_back(c);
    cuts.push_back(end);
  } else {
    for (int i = 5; i < argc; ++i) cuts.push_back(std::strtoull(argv[i], nullptr, 10));
  }

  std::vector<uint32_t> T(gf::kTableWords);
  gf::build_device_tables(poly, T.data());
  std::vector<uint32_t> partials(nseg + 1, 0x5EED5EEDu), state(n, 0xDEADBEEFu), crcs(n, 0);
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
    const uint64_t alloc = ((used + 15) / 16) * 16;
    uint8_t* buf = static_cast<uint8_t*>(std::aligned_alloc(16, alloc ? alloc : 16));
    if (!buf) return 2;
    std::memset(buf, 0xA5, alloc ? alloc : 16);
    for (uint64_t j = 0; j < n; ++j)
      if (lens[j] > begin)
        std::memcpy(buf + j * slot, data.data() + offs[j] + begin, (end < lens[j] ? end : lens[j]) - begin);
    const uint64_t base = reinterpret_cast<uint64_t>(buf), origin = begin;

    // stage 1: wave w = piece k0 + w % nk of part w / nk
    const uint64_t k0 = gf::range_first_piece(begin, log2s), nk = gf::range_pieces(begin, end, log2s);
    for (uint64_t w = 0; w < n * nk; ++w) {
      const uint64_t part = w / nk, k = k0 + (w - part * nk);
      const gf::Piece pc = gf::piece_of(k, log2s, begin, end, lens[part]);
      if (pc.lo >= pc.hi) continue;
      if (seg0[part] + k >= nseg) return 3;  // (the kernel's store would leave the buffer)
      partials[seg0[part] + k] = segment_raw(T.data(), poly, base + part * slot + (pc.lo - origin), pc.hi - pc.lo);
    }
    // stage 2: one wave per part
    for (uint64_t part = 0; part < n; ++part) {
      const gf::PartRange R = gf::part_range(lens[part], begin, end, log2s);
      if (R.bytes == 0) {
        if (R.emits) {
          if (wrote[part] >= 0) return 4;
          crcs[part] = 0;
          wrote[part] = int(ri);
        }
        continue;
      }
      uint32_t* v = partials.data() + seg0[part] + R.first;
      uint32_t r = fold_front(v, R.front, log2s, poly);
      r = gf::mulmod(r, gf::xpow8(R.tail, poly), poly) ^ v[R.front];
      for (uint64_t i = 0; i <= R.front; ++i) v[i] = 0x5EED0000u + uint32_t(ri);  // used up
      r = gf::range_state(begin ? state[part] : 0u, r, begin, R.bytes, poly);
      state[part] = r;
      if (R.emits) {
        if (wrote[part] >= 0) return 4;  // written twice
        if (gf::range_emit(r, lens[part], poly) != gf::finalise(r, lens[part], poly)) return 5;
        crcs[part] = gf::range_emit(r, lens[part], poly);
        wrote[part] = int(ri);
      }
    }
    std::free(buf);
  }
  for (uint64_t part = 0; part < n; ++part) std::printf("%08x %d\n", crcs[part], wrote[part]);
  return 0;
}
