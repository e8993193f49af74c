// host_limits.hpp -- sizes and thresholds of the host-resident path that more than one unit
// uses (the pipeline in host_path.cpp, the split planner in route_plan.cpp).  HIP-free.
#pragma once
#include <cstdint>

#include "../../include/s3hash.h"

namespace s3h::host {

// The host pipeline's algorithm ids: enum s3h_algo, and beside it (internal, never part of the
// public enum) one id per enum s3h_crc and one for CRC-64/NVME (a CRC plan's id 2, internal.hpp
// kCrcIdCrc64Nvme).  A merged batch is keyed on the id array.
constexpr int kAlgoCrcBase = 0x100;
constexpr int kAlgoCrc32c = kAlgoCrcBase + S3H_CRC32C, kAlgoCrc32 = kAlgoCrcBase + S3H_CRC32;
constexpr int kAlgoCrc64Nvme = kAlgoCrcBase + 2;
inline bool is_crc(int algo) { return algo == kAlgoCrc32c || algo == kAlgoCrc32 || algo == kAlgoCrc64Nvme; }
inline int crc_of(int algo) { return algo - kAlgoCrcBase; }  // the CRC plan's id of a CRC algorithm

// digest words per part: SHA-256 8, MD5 4, SHA-1 5, a 32-bit CRC 1, CRC-64/NVME 2
inline uint32_t digest_words(int algo) {
  return algo == S3H_ALGO_MD5 ? 4u : algo == S3H_ALGO_SHA1 ? 5u : algo == kAlgoCrc64Nvme ? 2u
         : is_crc(algo) ? 1u : 8u;
}

// algorithms one host-path call computes: SHA-256, MD5, SHA-1 or a CRC alone, or two of them
constexpr int kHostMaxAlgo = 2;
constexpr int kHostRing = 3;     // HBM ring slots / pinned staging slots

// Group mode (host_path.cpp run_host_groups) for many small parts: parts of at most
// kGroupMaxPart bytes go in groups of whole parts instead of slices of every part.
constexpr uint64_t kGroupMaxPart = 1ull << 20;
// Beyond this many ragged pinned parts the slice pipeline stages them (memcpy + one DMA per
// slice) instead of one DMA per part per slice.
constexpr uint64_t kPinnedStageMin = 256;

}  // namespace s3h::host
