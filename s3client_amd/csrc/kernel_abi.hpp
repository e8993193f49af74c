// kernel_abi.hpp -- what the host side and the gfx950 kernels share: the launch argument block,
// the plan's part slots, the stream splice jobs, the generator's part records and the
// workgroup-shape constants the host sizes grids with.  Plain structs and constants: the
// host translation units (g++) and the kernel translation unit (launch.hip, hipcc) both include
// it, so a plan built on the host and the kernel that reads it agree by construction.
#pragma once
#include <stdint.h>

#include "exp_config.hpp"

#if defined(__HIPCC__)
#define S3H_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define S3H_HOST_DEVICE inline
#endif

namespace s3h {

struct Slot {        // one upload part in a plan, slots sorted by block count (descending)
  uint64_t off;      // byte offset of the part relative to the launch's base pointer
  uint64_t len;      // part length in bytes (the full part, also for resumed launches)
};

// Number of 64-byte compressions for a message of `len` bytes: ceil((len + 9) / 64)
// (lib/hash/utility.cpp:42-56 alloc_padded: 0x80, zeros, 64-bit big-endian bit length).
S3H_HOST_DEVICE uint64_t nblocks(uint64_t len) { return (len + 72) >> 6; }

// LaunchArgs::flags
constexpr uint32_t kNoPad = 1;   // hash only the slot's whole 64-B blocks; never pad or emit
constexpr uint32_t kResume = 2;  // load the chaining state even at blk_begin == 0

// Bits of the device error word (LaunchArgs::err).  Every host entry point reads the word
// after its launches complete and fails the call when it is non-zero (plan.cpp plan_check):
// a launch whose digests may be wrong never returns S3H_OK.
constexpr uint32_t kErrSyncTimeout = 1;  // a producer/consumer flag wait timed out

struct LaunchArgs {
  const uint8_t* base;       // part p's block b is at base + slots[p].off + 64*(b - blk_origin)
  const Slot* slots;         // sorted by nblocks descending
  const uint32_t* out_idx;   // slot -> output part (message) index
  uint32_t* state;           // n*8 words (message order); may be null for single-launch plans
  uint32_t* digests;         // n*8 words (part order), bswap32(H_i) like lib/hash to_little
  const uint8_t* zero;       // 256 zero bytes: target of the loads of out-of-range lanes
  const uint64_t* bits;      // per-message bit length for the padding (null: 8 * slot length)
  uint64_t blk_begin, blk_end, blk_origin;
  uint32_t n;
  uint32_t flags;
  // Clock probe (s3h_plan_set_clock_probe; skew kernel): per consumer wave, shader-clock and
  // 100 MHz real-time counters at the start and end of its chain loop.  Null: off.
  uint64_t* clocks;
  // sha256_skew_pairs_kernel: the first `solo` workgroups run one group each (the longest
  // parts, on a CU of their own), the rest two.  0 elsewhere.
  uint32_t solo;
  // Device error word of the plan (kErr* bits OR-ed in by global atomics; cleared by the host).
  uint32_t* err;
};

// MD5 is paced by a SHA-256 producer only inside a workgroup (through LDS).  Pacing the MD5
// workgroups of the split dual grid and of the mixed grid's apart form by the skew groups of
// their XCD, through step counts in global memory, was measured and dropped: C2 dual traffic
// 2x -> 1.04-1.22x at -0.3 %, C3 dual 1.25x -> 1.18x at -3 to -4 %
// (profiles/r06_dual_xcd_pace_ab.json).

// sha256_md5_group_mixed_kernel, apart form: the MD5 workgroups of the F skew groups' 8F
// chains, 64 chains each.
S3H_HOST_DEVICE uint32_t mixed_lead_wgs(uint64_t F) { return uint32_t((8 * F + 63) / 64); }

// sha256_md5_dual_kernel (the split dual grid): MD5 workgroups after the skew workgroups, one
// per 64 of the n parts.
S3H_HOST_DEVICE uint32_t split_md5_wgs(uint64_t n) { return uint32_t((n + 63) / 64); }

// Workgroup shapes (sha256_kernels.hip).
constexpr int kPcThreads = 128;          // producer/consumer: wave 0 consumer, wave 1 producer; 64 parts
constexpr int kPairThreads = 128;        // lane-pair kernel: 32 parts per workgroup
constexpr int kPairParts = 32;
constexpr int kQuadChainsPerWave = 8;    // skew / quad: 8 chains per consumer wave
// MD5 kernel: kMd5Bps-block producer steps (128 KiB of LDS, one workgroup per CU) while the
// grid fits one workgroup per CU (<= 64 x CUs parts); 1-block steps (32 KiB) beyond.
constexpr int kMd5Bps = 4;
// SHA-1 kernel: kSha1Bps-block producer steps (80 KiB of LDS) while the grid fits one workgroup
// per CU (<= 64 x CUs parts); 1-block steps (40 KiB, up to four workgroups per CU) beyond.
constexpr int kSha1Bps = S3H_EXP_SHA1_BPS;
static_assert(kSha1Bps >= 1 && kSha1Bps <= 3, "SHA-1 steps: 40 KiB of LDS per block, 160 KiB per CU");

// ------------------------------------------------------------- multi-object streams
// Carry bookkeeping of one s3h_stream update, one thread per message (<= 127 bytes moved):
//   kSpliceHead : head[i] = carry[i][0:c] ++ chunk[0:h]   (c + h == 64: the block that
//                 straddles the previous update and this one, hashed by the head launch)
//   kSpliceGrow : carry[i][c:c+h] = chunk[0:h]           (still < 64 B buffered)
//   kSpliceReset: carry[i][0:r] = chunk[tail:tail+r]     (the new < 64-B remainder)
struct SpliceJob {
  uint64_t src, tail;  // chunk start / new-remainder start, offsets from the update's base
  uint32_t c, h, r, mode;
};
constexpr uint32_t kSpliceHead = 1, kSpliceGrow = 2, kSpliceReset = 4;

// ------------------------------------------------------------- CRC-32C / CRC-32 (crc32_kernels.hip)
// Stage 1 (crc_segments_kernel): one record per segment of a non-empty part, in part order.
struct CrcSeg {
  uint64_t off;   // byte offset of the segment relative to the launch's base pointer
  uint32_t len;   // 1..segment_bytes
  uint32_t pad_;
};
// Stage 2 (crc_parts_kernel): part p's ceil(len / segment_bytes) values start at partials[seg0].
struct CrcPart {
  uint64_t seg0;
  uint64_t len;
};
struct CrcSegArgs {
  const uint8_t* base;
  const CrcSeg* segs;
  const uint32_t* tables;  // crc_math.hpp build_device_tables (kTableWords words, 16-B aligned)
  uint32_t* partials;      // one raw value per segment
  uint64_t nseg;
  uint32_t poly;
};
struct CrcPartArgs {
  const CrcPart* parts;
  const uint32_t* partials;
  uint32_t* crcs;          // one finalised CRC per part, part order
  uint64_t n;
  uint32_t poly;
  uint32_t x_segment;      // x^(8 * segment_bytes) mod P
  uint32_t log2_segment;
};
// Ranged launches (crc_range_pieces_kernel, crc_range_parts_kernel): bytes [begin, end) of every
// part, part p's byte b at base + offs[p] + (b - origin).  Both stages derive their pieces on
// the device (crc_math.hpp piece_of / part_range) from the per-part records, so a launch
// uploads nothing.  Piece k of part p goes through partials[parts[p].seg0 + k].
struct CrcRangeArgs {
  const uint8_t* base;
  const CrcPart* parts;
  const uint64_t* offs;    // byte offset of each part relative to the launch's base pointer
  const uint32_t* tables;
  uint32_t* partials;
  uint32_t* state;         // one running raw value (init 0) per part, kept between launches
  uint32_t* crcs;          // written only for parts whose last byte lies in the range
  uint64_t n;
  uint64_t begin, end, origin;
  uint32_t poly;
  uint32_t x_segment;
  uint32_t log2_segment;
};
constexpr int kCrcSegThreads = 512;   // 8 waves share one copy of the tables in LDS
constexpr int kCrcPartThreads = 256;  // 4 parts per workgroup

// ------------------------------------------------------------- CRC-64/NVME (crc64_kernels.hip)
// The same two stages and the same per-segment / per-part records (CrcSeg, CrcPart) with 64-bit
// values: tables (crc64_math.hpp build_device_tables), partials, running values and outputs are
// 64-bit words.  One argument block serves the whole-part launch (segs set; begin, end, origin,
// offs and state unused) and the ranged launch (segs null).
struct Crc64Args {
  const uint8_t* base;
  const CrcSeg* segs;      // whole-part launch: one record per segment
  const CrcPart* parts;
  const uint64_t* offs;    // ranged launch: byte offset of each part relative to `base`
  const uint64_t* tables;  // crc64_math.hpp kTableWords words, 16-B aligned
  uint64_t* partials;      // one raw value per segment / piece
  uint64_t* state;         // ranged launch: one running raw value per part
  uint64_t* crcs;          // one finalised CRC per part, part order
  uint64_t n, nseg;
  uint64_t begin, end, origin;
  uint64_t poly;
  uint64_t x_segment;      // x^(8 * segment_bytes) mod P
  uint32_t log2_segment;
};
constexpr int kCrc64SegThreads = 512;   // 8 waves share one copy of the tables (48.6 KiB of LDS)
constexpr int kCrc64PartThreads = 256;  // 4 parts per workgroup

// ------------------------------------------------------------- SigV4 chunk signatures (chunk_sign_kernels.hip)
// One record per part: its data chunks' digests are digests[8 * first ...] (count of them), its
// count + 1 signatures go to signatures[8 * sig ...].
struct ChunkChainPart {
  uint64_t first;
  uint64_t sig;
  uint32_t count;
  uint32_t pad_;
};
constexpr int kChunkTailWords = 80;  // the inner tail: at most 5 blocks (r + 194 + 9 <= 266 bytes)
// The context's midstates and tail template travel in the argument block (chunk_sign.hpp): a
// launch uploads nothing.  `r` and `nblk` are uniform over the launch.
struct ChunkChainArgs {
  const uint32_t* digests;     // chunk digests, word i = bswap32(H_i)
  const ChunkChainPart* parts;
  const uint32_t* seeds;       // n x 8 words, the same convention
  uint32_t* signatures;
  uint64_t n;
  uint32_t r;                  // |P| mod 64: the first hex field starts at tail byte r
  uint32_t nblk;               // compressions of the inner tail (4 or 5)
  uint32_t istate[8];
  uint32_t ostate[8];
  uint32_t tail[kChunkTailWords];  // big-endian words, the two 64-byte hex fields zeroed
};
constexpr int kChunkChainThreads = 64;  // one wave per workgroup, one lane per part

// ------------------------------------------------------------- SigV4 trailer signatures (chunk_trailer_kernels.hip)
// The last link of a chunk-signed upload with a trailing checksum header
// (STREAMING-AWS4-HMAC-SHA256-PAYLOAD-TRAILER): per part, the CRC as base64 in the header line,
// the line's SHA-256, and the HMAC over the trailer string.  The parts are the chain kernel's
// records: a part's last chunk signature is signatures[8 * (sig + count) ...].
constexpr int kTrailerTailWords = 64;  // the inner tail: at most 4 blocks (r + 129 + 9 <= 201 bytes)
struct ChunkTrailerArgs {
  const uint32_t* signatures;  // the chunk signatures of the chain kernel
  const ChunkChainPart* parts;
  const void* checksums;       // n values in part order: uint32_t, or uint64_t when `wide`
  uint32_t* trailer;           // n x 8 words, word i = bswap32(H_i)
  uint64_t n;
  uint32_t r;                  // |P| mod 64: the first hex field starts at tail byte r
  uint32_t nblk;               // compressions of the inner tail (3 or 4)
  uint32_t wide;               // 0: 32-bit values (8 characters), 1: 64-bit values (12)
  uint32_t value_at;           // byte offset of the base64 text in the line
  uint32_t istate[8];          // the trailer string's inner midstate
  uint32_t ostate[8];
  uint32_t line[16];           // the header line's one block, big-endian words, the value zeroed
  uint32_t tail[kTrailerTailWords];  // big-endian words, the two 64-byte hex fields zeroed
};

// ------------------------------------------------------------- aws-chunked bodies (chunk_body_kernels.hip)
// The wire form of a chunk-signed upload: per data chunk of k bytes
//   hex(k) ";chunk-signature=" hex(sig) "\r\n" data "\r\n"          hexlen(k) + 85 + k bytes
// then the line of the final 0-byte chunk (84 bytes) and "\r\n" or the trailer text.  One work
// item (one wave) per piece of a data chunk -- at most kChunkBodyPiece contiguous bytes -- and one
// per part for its final line and ending.  Every full chunk of a plan has the same wire length,
// so chunk i of a part starts at  body offset + i * (head_len + chunk_bytes + 2).
struct ChunkBodyPart {
  uint64_t off;     // byte offset of the part relative to the launch's base pointer
  uint64_t len;
  uint64_t full;    // floor(len / chunk_bytes)
  uint64_t item0;   // the part's first work item: full * pieces_per_chunk data items, the
                    // remainder chunk's ceil(rem / kChunkBodyPiece), then the final item
  uint64_t sig;     // row of the part's first signature
};
constexpr int kChunkBodyThreads = 256;         // 4 waves, one item each per grid pass
constexpr uint32_t kChunkBodyPiece = 16384;    // 16 tiles of 64 lanes x 16 bytes
constexpr uint32_t kChunkBodyMaxGrid = 2048;   // 32 waves on each of 256 CUs; more items: grid stride
// The fixed text the kernel copies, uploaded with the plan: ";chunk-signature=" at byte 0, the
// checksum's name and ':' at kChunkBodyNameAt, "\r\nx-amz-trailer-signature:" at kChunkBodySigAt.
constexpr uint32_t kChunkBodyNameAt = 32, kChunkBodySigAt = 64, kChunkBodyTextBytes = 96;
struct ChunkBodyArgs {
  const uint8_t* base;
  const ChunkBodyPart* parts;
  const uint64_t* body_offs;   // n byte offsets of the bodies relative to `body`
  const uint32_t* signatures;  // the chain kernel's
  const void* checksums;       // trailer form: n values, uint32_t, or uint64_t when `wide`; else null
  const uint32_t* trailer;     // trailer form: n x 8 words
  const uint8_t* text;         // kChunkBodyTextBytes
  uint8_t* body;
  uint64_t n, items, chunk_bytes;
  uint32_t pieces_per_chunk;   // ceil(chunk_bytes / kChunkBodyPiece)
  uint32_t head_len;           // hexlen(chunk_bytes) + 83: a full chunk's bytes in front of its data
  uint32_t wide;               // 0: 32-bit values (8 characters), 1: 64-bit values (12)
  uint32_t name_len;           // the checksum's name and ':'
};

// ------------------------------------------------------------- synthetic input generator
// G(seed, p, L) of SURVEY.md 8(d): one record per part (byte offset, length, generator id).
struct GenPart { uint64_t off, len, id; };

}  // namespace s3h
