// sha1_kernels.hip -- batched SHA-1 (x-amz-checksum-sha1) for MI355X (gfx950).
//
// SHA-1 (FIPS 180-4 6.1) is a serial Merkle-Damgard chain like SHA-256 and MD5 and pads exactly
// as SHA-256 does (0x80, zeros, 64-bit big-endian bit length), so the plan, the ranged /
// unpadded / stream launch forms and every decode helper of sha256_kernels.hip serve unchanged.
// One kernel, in the shape of sha256_pc_kernel / md5_pc_kernel: 128-thread workgroups, wave 0
// the consumer with one lane per chain (64 parts per workgroup), wave 1 the producer.  Slots are
// sorted by block count, so the workgroup's first slot bounds the loop and both waves execute
// the same number of s_barrier.  No flag waits: nothing reports into the device error word.
//
// Producer: fetches one step ahead into two named register sets, decodes (one v_perm per word),
// pads, expands W[16..79] = rotl1(W[t-3] ^ W[t-8] ^ W[t-14] ^ W[t-16]) (one bitop3, one xor, one
// alignbit per word) and writes the 80 words W[t] + K[t] as 20 rows of uint4[64] into an LDS
// double buffer: 20 KiB per block per buffer, one or two blocks per step (sha1_pc_kernel).
// Consumer: 20 ds_read_b128 per block, streamed in beside the rounds (sha1_block_streamed), and
// 5 VALU per round in rotating names --
//   f = bitop3(b, c, d); e = add3(e, f, wk); e += rotl5(a); b = rotl30(b)
// -- 400 VALU per block.  The chaining state uses words 0-4 of the plan's 8-word state slots;
// the digest is 5 words per part, word i = bswap32(H_i) (the 20 bytes in memory are the
// canonical digest, as for SHA-256), written with plain dword stores at a 20-byte stride.
//
// Every kernel here lives in a text section of its own, so the machine code of the kernels
// pinned in s3client_amd/kernel_isa_counts.json stays as it is.
#pragma once
#include "sha256_device.hpp"

namespace s3h {

#define S3H_SHA1_TEXT __attribute__((section(".text.s3h_sha1")))

__device__ __forceinline__ constexpr uint32_t sha1_k(int t) {
  return t < 20 ? 0x5a827999u : t < 40 ? 0x6ed9eba1u : t < 60 ? 0x8f1bbcdcu : 0xca62c1d6u;
}

// Ch, parity, Maj, parity as single v_bitop3_b32 (truth table index = b<<2 | c<<1 | d).  Written
// as builtins: the compiler otherwise splits Ch and Maj into and/or terms (md5_f).
template <int T>
__device__ __forceinline__ uint32_t sha1_f(uint32_t b, uint32_t c, uint32_t d) {
  if constexpr (T < 20) return __builtin_amdgcn_bitop3_b32(b, c, d, 0xCA);
  else if constexpr (T < 40) return __builtin_amdgcn_bitop3_b32(b, c, d, 0x96);
  else if constexpr (T < 60) return __builtin_amdgcn_bitop3_b32(b, c, d, 0xE8);
  else return __builtin_amdgcn_bitop3_b32(b, c, d, 0x96);
}

// One round in rotating names: the new a lands in `e`, b is rotated in place.
template <int T>
__device__ __forceinline__ void sha1_round(uint32_t a, uint32_t& b, uint32_t c, uint32_t d,
                                           uint32_t& e, uint32_t wk) {
  e = e + sha1_f<T>(b, c, d) + wk;
  e += __builtin_amdgcn_alignbit(a, a, 27);
  b = __builtin_amdgcn_alignbit(b, b, 2);
}

// Four rounds from one row (W+K of rounds 4Q .. 4Q+3).  The names come back to their places
// after five rows, so the caller passes row Q's names rotated by 4 * Q mod 5.
template <int Q>
__device__ __forceinline__ void sha1_row(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d,
                                         uint32_t& e, const v4u32 r) {
  sha1_round<4 * Q + 0>(a, b, c, d, e, r.x);
  sha1_round<4 * Q + 1>(e, a, b, c, d, r.y);
  sha1_round<4 * Q + 2>(d, e, a, b, c, r.z);
  sha1_round<4 * Q + 3>(c, d, e, a, b, r.w);
}

// The 80 rounds of one block with its rows streamed in.  The reads and their waits are asm
// statements: the compiler, left to itself, reads all 20 rows and waits for every one before
// the first round (20 KiB per wave at 128 B/clk of LDS plus the latency, exposed per block;
// md5_block_streamed).  LDS returns in order, so a wait for "at most N outstanding" releases
// the rows before them: 16 reads, rows 0-1 awaited (lgkmcnt holds 4 bits); then the last four
// reads and rows 2-6; rows 7-11; 12-15; 16-19.  Five s_waitcnt per block.  Each wait names the
// rows it releases and the chain's registers as read-write operands, so the rounds that use
// those rows stay behind it and the rounds before it stay in front.
// `ad`: this lane's LDS byte address of row 0 (rows are 1,024 B apart: Sha1Lds).
#define S3H_SHA1_LD(N, OFF) "ds_read_b128 %[" #N "], %[ad] offset:" #OFF "\n\t"
#define S3H_SHA1_CHAIN "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e)
__device__ __forceinline__ void sha1_block_streamed(uint32_t& a, uint32_t& b, uint32_t& c,
                                                    uint32_t& d, uint32_t& e, uint32_t ad) {
  v4u32 r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13, r14, r15, r16, r17, r18, r19;
  asm volatile(S3H_SHA1_LD(r0, 0) S3H_SHA1_LD(r1, 1024) S3H_SHA1_LD(r2, 2048) S3H_SHA1_LD(r3, 3072)
               S3H_SHA1_LD(r4, 4096) S3H_SHA1_LD(r5, 5120) S3H_SHA1_LD(r6, 6144) S3H_SHA1_LD(r7, 7168)
               S3H_SHA1_LD(r8, 8192) S3H_SHA1_LD(r9, 9216) S3H_SHA1_LD(r10, 10240)
               S3H_SHA1_LD(r11, 11264) S3H_SHA1_LD(r12, 12288) S3H_SHA1_LD(r13, 13312)
               S3H_SHA1_LD(r14, 14336) S3H_SHA1_LD(r15, 15360) "s_waitcnt lgkmcnt(14)"
               : [r0] "=&v"(r0), [r1] "=&v"(r1), [r2] "=&v"(r2), [r3] "=&v"(r3), [r4] "=&v"(r4),
                 [r5] "=&v"(r5), [r6] "=&v"(r6), [r7] "=&v"(r7), [r8] "=&v"(r8), [r9] "=&v"(r9),
                 [r10] "=&v"(r10), [r11] "=&v"(r11), [r12] "=&v"(r12), [r13] "=&v"(r13),
                 [r14] "=&v"(r14), [r15] "=&v"(r15)
               : [ad] "v"(ad)
               : "memory");
  sha1_row<0>(a, b, c, d, e, r0);
  sha1_row<1>(b, c, d, e, a, r1);
  asm volatile(S3H_SHA1_LD(r16, 16384) S3H_SHA1_LD(r17, 17408) S3H_SHA1_LD(r18, 18432)
               S3H_SHA1_LD(r19, 19456) "s_waitcnt lgkmcnt(13)"
               : [r16] "=&v"(r16), [r17] "=&v"(r17), [r18] "=&v"(r18), [r19] "=&v"(r19),
                 "+v"(r2), "+v"(r3), "+v"(r4), "+v"(r5), "+v"(r6), S3H_SHA1_CHAIN
               : [ad] "v"(ad)
               : "memory");
  sha1_row<2>(c, d, e, a, b, r2);
  sha1_row<3>(d, e, a, b, c, r3);
  sha1_row<4>(e, a, b, c, d, r4);
  sha1_row<5>(a, b, c, d, e, r5);
  sha1_row<6>(b, c, d, e, a, r6);
  asm volatile("s_waitcnt lgkmcnt(8)"
               : "+v"(r7), "+v"(r8), "+v"(r9), "+v"(r10), "+v"(r11), S3H_SHA1_CHAIN);
  sha1_row<7>(c, d, e, a, b, r7);
  sha1_row<8>(d, e, a, b, c, r8);
  sha1_row<9>(e, a, b, c, d, r9);
  sha1_row<10>(a, b, c, d, e, r10);
  sha1_row<11>(b, c, d, e, a, r11);
  asm volatile("s_waitcnt lgkmcnt(4)"
               : "+v"(r12), "+v"(r13), "+v"(r14), "+v"(r15), S3H_SHA1_CHAIN);
  sha1_row<12>(c, d, e, a, b, r12);
  sha1_row<13>(d, e, a, b, c, r13);
  sha1_row<14>(e, a, b, c, d, r14);
  sha1_row<15>(a, b, c, d, e, r15);
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(r16), "+v"(r17), "+v"(r18), "+v"(r19), S3H_SHA1_CHAIN);
  sha1_row<16>(b, c, d, e, a, r16);
  sha1_row<17>(c, d, e, a, b, r17);
  sha1_row<18>(d, e, a, b, c, r18);
  sha1_row<19>(e, a, b, c, d, r19);
}
#undef S3H_SHA1_LD
#undef S3H_SHA1_CHAIN

// Rows Q.. of W[t] + K[t] written to LDS, the schedule expanded on the way in a 16-word window
// (w[t & 15] is W[t - 16] until it is overwritten with W[t]); unrolled by recursion (md5_km_rows).
template <int T>
__device__ __forceinline__ uint32_t sha1_w(uint32_t w[16]) {
  if constexpr (T >= 16) {
    const uint32_t x = xor3(w[(T - 3) & 15], w[(T - 8) & 15], w[(T - 14) & 15]) ^ w[T & 15];
    w[T & 15] = __builtin_amdgcn_alignbit(x, x, 31);
  }
  return w[T & 15] + sha1_k(T);
}
template <int Q>
__device__ __forceinline__ void sha1_wk_rows(uint32_t w[16], uint4 (*buf)[64], uint32_t lane) {
  if constexpr (Q < 20) {
    const uint32_t x = sha1_w<4 * Q + 0>(w), y = sha1_w<4 * Q + 1>(w);
    const uint32_t z = sha1_w<4 * Q + 2>(w), u = sha1_w<4 * Q + 3>(w);
    buf[Q][lane] = make_uint4(x, y, z, u);
    sha1_wk_rows<Q + 1>(w, buf, lane);
  }
}

// kFull: the block is a whole data block of every lane's part (the producer's fast steps), so
// only the v_perm decode is emitted, not the padding path's predicated byte loads (md5_produce).
template <bool kFull>
__device__ __forceinline__ void sha1_produce(const RawBlock& r, uint32_t sel, const uint8_t* bp,
                                             uint64_t len, uint64_t bits, uint64_t blk,
                                             uint64_t limit, uint4 (*buf)[64], uint32_t lane) {
  uint32_t w[16];
  if constexpr (kFull) decode_full(r, sel, w);
  else make_block(r, sel, bp, len, bits, blk, limit, w);
  sha1_wk_rows<0>(w, buf, lane);
}

template <int kBps>
struct Sha1Lds {
  uint4 wk[2][kBps][20][64];  // [buffer][block of the step][row][lane]: kBps x 40 KiB
};

template <int kBps>
__device__ __forceinline__ void sha1_pc_body(const LaunchArgs& A, const uint32_t group,
                                             const uint32_t role, Sha1Lds<kBps>& L) {
  auto& lds_wk = L.wk;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t slot0 = group * 64u;
  const uint32_t slot = slot0 + lane;
  const bool valid = slot < A.n;
  const uint32_t last = (slot0 + 64u <= A.n ? slot0 + 64u : A.n) - 1;  // the shortest part's slot
  Slot s = {0, 0};
  if (valid) s = A.slots[slot];
  const uint64_t nb = valid ? slot_blocks(A, s.len) : 0;
  // Slots are sorted by block count, so the workgroup's first slot bounds the loop; the step
  // count is the same in both waves, so their s_barrier counts match.
  const uint64_t wg_nb = slot_blocks(A, A.slots[slot0].len);
  const uint64_t wg_end = wg_nb < A.blk_end ? wg_nb : A.blk_end;
  if (wg_end <= A.blk_begin) return;  // whole workgroup done in earlier launches
  const uint64_t iters = wg_end - A.blk_begin;
  const uint64_t nsteps = (iters + kBps - 1) / kBps;

  if (role == 1) {
    // ---------------------------------------------------------------- producer
    // Step k's blocks are fetched one step before they are decoded: two named register sets
    // alternate (no dynamic indexing -> no scratch).
    const uint64_t b0 = A.blk_begin;
    const uint8_t* p = A.base + s.off + 64ull * (b0 - A.blk_origin);
    const uint32_t sel = be_selector(uint32_t(reinterpret_cast<uintptr_t>(p) & 3));
    const uint64_t fend = fetch_end(s.len, A.blk_end);
    const uint64_t bits = valid ? msg_bits(A, slot, s.len) : 0;
    const uint64_t dl = decode_len(valid, s.len);
    // Blocks past this lane's last one (its padding included) or past the launch's range are
    // never consumed: written as zeros without touching memory (md5_pc_body's `lim`).
    const uint64_t lim = nb < A.blk_end ? nb : A.blk_end;
    RawBlock ra[kBps], rb[kBps];
#define S3H_SHA1_FETCH(R, K)                                                                 \
    _Pragma("unroll") for (int h = 0; h < kBps; ++h)                                        \
      fetch_full(p + 64 * ((K) * kBps + h), b0 + (K) * kBps + h < fend, A.zero, R[h]);
#define S3H_SHA1_MAKE_T(R, K, FULL)                                                          \
    _Pragma("unroll") for (int h = 0; h < kBps; ++h)                                        \
      sha1_produce<FULL>(R[h], sel, p + 64 * ((K) * kBps + h), dl, bits, b0 + (K) * kBps + h, \
                         lim, lds_wk[(K) & 1][h], lane);
#define S3H_SHA1_MAKE(R, K) S3H_SHA1_MAKE_T(R, K, false)
    // Steps below `full_steps` hold whole data blocks of every lane's part (the group's last
    // valid slot is the shortest; lanes past n decode_len past everything): a compact loop
    // with the perm-only decode runs them in pairs.
    const uint64_t lfull = A.slots[last].len >> 6;
    const uint64_t fabs = lfull < A.blk_end ? lfull : A.blk_end;
    const uint64_t full_steps = fabs > b0 ? (fabs - b0) / kBps : 0;
    S3H_SHA1_FETCH(ra, 0)
    S3H_SHA1_FETCH(rb, 1)
    S3H_SHA1_MAKE(ra, 0)
    __syncthreads();
    uint64_t k = 1;
    for (; k + 1 < full_steps; k += 2) {  // steps k and k + 1: whole blocks, both produced
      S3H_SHA1_FETCH(ra, k + 1)
      S3H_SHA1_MAKE_T(rb, k, true)
      __syncthreads();
      S3H_SHA1_FETCH(rb, k + 2)
      S3H_SHA1_MAKE_T(ra, k + 1, true)
      __syncthreads();
    }
    // k odd: the same register roles.  One barrier per step k = 1 .. nsteps, as the consumer's
    // (one after each of its nsteps steps, the first after its state load).
    for (;; k += 2) {
      if (k < nsteps) {
        S3H_SHA1_FETCH(ra, k + 1)
        S3H_SHA1_MAKE(rb, k)
      }
      __syncthreads();
      if (k + 1 > nsteps) break;
      if (k + 1 < nsteps) {
        S3H_SHA1_FETCH(rb, k + 2)
        S3H_SHA1_MAKE(ra, k + 1)
      }
      __syncthreads();
      if (k + 2 > nsteps) break;
    }
#undef S3H_SHA1_FETCH
#undef S3H_SHA1_MAKE
#undef S3H_SHA1_MAKE_T
  } else {
    // ---------------------------------------------------------------- consumer
    __builtin_amdgcn_s_setprio(3);
    uint32_t st[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u};
    if (valid && resumes(A)) {
      const uint32_t* sp = A.state + 8ull * A.out_idx[slot];
      const uint4 v = reinterpret_cast<const uint4*>(sp)[0];
      st[0] = v.x; st[1] = v.y; st[2] = v.z; st[3] = v.w;
      st[4] = sp[4];
    }
    __syncthreads();
    // slots are sorted by length: every chain of the group is live below the last one's end
    const uint64_t live_end = slot_blocks(A, A.slots[last].len);
    uint64_t clk0 = 0, rt0 = 0;  // clock probe (s3h_plan_set_clock_probe), as in md5_pc_body
    if (A.clocks) {
      clk0 = __builtin_amdgcn_s_memtime();
      rt0 = __builtin_amdgcn_s_memrealtime();
    }
    // One step: its kBps blocks back to back, then the step's barrier.  Steps whose every block
    // lies below live_end -- every chain live -- run in their own loop with an unconditional
    // feed-forward (the loop tools/isa_counts.py counts); the ragged tail selects per lane and
    // skips the blocks past the launch's range.
    typedef __attribute__((address_space(3))) uint4 lds_u4;
    auto row_addr = [&](uint32_t buf, int h) {
      return uint32_t(reinterpret_cast<uintptr_t>((const lds_u4*)&lds_wk[buf][h][0][lane]));
    };
    const uint64_t fast = live_end > A.blk_begin ? (live_end - A.blk_begin < iters
                                                    ? live_end - A.blk_begin : iters) : 0;
    uint64_t j = 0;
    for (; j < fast / kBps; ++j) {
      const uint32_t buf = uint32_t(j & 1);
#pragma unroll
      for (int h = 0; h < kBps; ++h) {
        uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4];
        sha1_block_streamed(a, b, c, d, e, row_addr(buf, h));
        st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e;
      }
      __syncthreads();
    }
    for (; j < nsteps; ++j) {
      const uint32_t buf = uint32_t(j & 1);
#pragma unroll
      for (int h = 0; h < kBps; ++h) {
        const uint64_t i = j * kBps + h;
        if (i >= iters) break;  // uniform: the launch's last step may be partial
        uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4];
        sha1_block_streamed(a, b, c, d, e, row_addr(buf, h));
        const bool live = (A.blk_begin + i) < nb;
        st[0] = live ? st[0] + a : st[0];
        st[1] = live ? st[1] + b : st[1];
        st[2] = live ? st[2] + c : st[2];
        st[3] = live ? st[3] + d : st[3];
        st[4] = live ? st[4] + e : st[4];
      }
      __syncthreads();
    }
    if (A.clocks) {
      const uint64_t clk1 = __builtin_amdgcn_s_memtime(), rt1 = __builtin_amdgcn_s_memrealtime();
      if (lane == 0) {
        uint64_t* c = A.clocks + 4ull * group;
        c[0] = clk0; c[1] = clk1; c[2] = rt0; c[3] = rt1;
      }
    }
    if (valid && nb > A.blk_begin) {
      if (emits(A, nb)) {
        // 20-byte stride: only 4-byte aligned, so five dword stores and nothing behind them
        uint32_t* o = A.digests + 5ull * A.out_idx[slot];
#pragma unroll
        for (int i = 0; i < 5; ++i) o[i] = bswap(st[i]);
      } else if (A.state) {
        uint32_t* sp = A.state + 8ull * A.out_idx[slot];
        reinterpret_cast<uint4*>(sp)[0] = make_uint4(st[0], st[1], st[2], st[3]);
        sp[4] = st[4];
      }
    }
  }
}

// kBps = kSha1Bps (80 KiB of LDS) while the grid fits one workgroup per CU (<= 64 x CUs parts):
// half the barriers per block; kBps = 1 (40 KiB, up to four workgroups per CU) for larger
// batches (launch.hip).  C2: 74.0 against 71.0 GiB/s in one run (profiles/sha1_c2.json).
template <int kBps>
__global__ __launch_bounds__(kPcThreads) S3H_SHA1_TEXT void sha1_pc_kernel(LaunchArgs A) {
  __shared__ Sha1Lds<kBps> L;
  sha1_pc_body<kBps>(A, blockIdx.x, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), L);
}

}  // namespace s3h
