/* include/s3hash.h -- C-ABI of the MI355X batched SHA-256 path (libs3hash.so).
 *
 * This is the boundary the S3 client links against for PAYLOAD hashing: plain pointers and
 * sizes, int status codes, no C++ or HIP types, no exceptions.  It sits beside the C++
 * drop-in of lib/hash (include/sha256.h, include/utility.h), whose single-message calls stay
 * on the CPU exactly as in the reference.
 *
 * Reference interfaces each entry point serves (paths under /root/reference):
 *   s3h_sha256_batch_device / s3h_plan_*  -- batched form of sha256::sha256
 *       (lib/hash/sha256.h:70, lib/hash/sha256.cpp:147-160), applied to the parts that
 *       lib/src/upload.cpp:89-110 (UploadParts) slices, before each part's digest is passed
 *       as `payloadHash` to S3Api::UploadFilePart (lib/include/s3-api.h:447-452).
 *   s3h_sha256_batch_host  -- the same starting and ending in host memory (file chunks
 *       staged for upload -> 32-byte digests handed back to the SigV4 signer,
 *       lib/src/aws_sign.cpp:236-237 x-amz-content-sha256).
 *   s3h_plan_launch_range  -- resumable chaining state: sha256::sha256_stream semantics
 *       (lib/hash/sha256.h:97, sha256.cpp:84-144) for many parts at once.
 *   s3h_sha1_batch_device / _batch_host / _file_parts, s3h_sha256_sha1_batch_host /
 *       _file_parts, S3H_ALGO_SHA1 in s3h_plan_create_ex / s3h_stream_create / s3h_verify_*,
 *       s3h_cpu_sha1, s3h_digest_checksum_text  -- x-amz-checksum-sha1 (lib/hash has no SHA-1;
 *       FIPS 180-4): 5 words per part in the same word convention.
 *   s3h_sigv4_signing_key, s3h_chunk_sign_ctx_*, s3h_chunk_plan_*, s3h_chunk_sign_batch_device /
 *       _host, s3h_cpu_chunk_signatures, s3h_chunk_header_text  -- aws-chunked bodies signed per
 *       chunk (STREAMING-AWS4-HMAC-SHA256-PAYLOAD), which the reference's signer does not
 *       produce (lib/src/aws_sign.cpp signs whole payloads): chunk hashes and the HMAC chain.
 *   s3h_chunk_plan_create_trailer / _launch_trailer / _trailer, s3h_chunk_sign_trailer_batch_*,
 *       s3h_cpu_trailer_signatures, s3h_chunk_trailer_text  -- the same bodies closed by a trailing
 *       checksum header and its signature (STREAMING-AWS4-HMAC-SHA256-PAYLOAD-TRAILER).
 *   s3h_chunk_body_geometry, s3h_cpu_chunk_body, s3h_chunk_plan_body / _body_info,
 *       s3h_chunk_body_batch_device  -- those bodies themselves: the framed bytes an uploader
 *       sends and their lengths (Content-Length), on the device or the CPU.
 *
 * Digest layout (every entry point): 8 uint32 words per part with word i = bswap32(H_i),
 * exactly lib/hash's `to_little` output (sha256.h:103-106); on little-endian hosts the 32
 * bytes in memory are the canonical SHA-256 digest, and sha256::hash_to_text prints them.
 */
#ifndef S3HASH_H
#define S3HASH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: s3h_route_rates_t / s3h_route_choose (size-carrying, digest sets), s3h_host_plan,
 * s3h_host_alloc_ex, MD5 and dual routed entry points.  s3h_route_model_t keeps its round-5
 * layout (8 fields) for good: new rates go to s3h_route_rates_t, which carries its size.
 * Added within version 2 (new symbols only, nothing changed): the CRC-32C / CRC-32 entry
 * points (s3h_crc_*, s3h_cpu_crc, s3h_checksum_text), then s3h_crc_plan_launch_range and the
 * host-resident forms s3h_crc_batch_host, s3h_sha256_crc_batch_host, s3h_sha256_crc_file_parts,
 * then CRC-64/NVME (s3h_crc64nvme_*, s3h_cpu_crc64nvme, s3h_checksum64_text,
 * s3h_sha256_crc64nvme_*), then SHA-1 (S3H_ALGO_SHA1 for plans, streams and verification,
 * s3h_sha1_batch_device, s3h_sha1_batch_host, s3h_sha1_file_parts, s3h_sha256_sha1_batch_host,
 * s3h_sha256_sha1_file_parts, s3h_cpu_sha1, s3h_digest_checksum_text), then SigV4 chunk-signed
 * uploads (s3h_sigv4_signing_key, s3h_chunk_sign_ctx_*, s3h_cpu_chunk_signatures,
 * s3h_chunk_header_text, s3h_chunk_geometry, s3h_chunk_plan_*, s3h_chunk_sign_batch_device / _host),
 * then their trailer signatures (s3h_cpu_trailer_signatures, s3h_trailer_line_text,
 * s3h_chunk_trailer_text, s3h_chunk_plan_create_trailer, s3h_chunk_plan_launch_trailer,
 * s3h_chunk_plan_trailer, s3h_chunk_plan_trailer_info, s3h_chunk_sign_trailer_batch_device / _host),
 * then the bodies (s3h_chunk_body_geometry, s3h_cpu_chunk_body, s3h_chunk_plan_body,
 * s3h_chunk_plan_body_info, s3h_chunk_body_batch_device). */
#define S3H_API_VERSION 2

enum s3h_status {
  S3H_OK = 0,
  S3H_EINVAL = -1,   /* bad argument (null pointer, bad device, n too large, ...) */
  S3H_ENODEV = -2,   /* no HIP device visible: the GPU path never falls back to the CPU */
  S3H_EHIP = -3,     /* HIP runtime error (message in s3h_last_error) */
  S3H_ENOMEM = -4    /* device or pinned host allocation failed */
};

enum s3h_kernel {
  S3H_KERNEL_AUTO = 0, /* choose by part count */
  S3H_KERNEL_LANE = 1, /* fused: one lane = schedule + rounds of one part */
  S3H_KERNEL_PC = 2,   /* producer/consumer: producer wave stages W+K through LDS */
  S3H_KERNEL_PAIR = 3, /* producer/consumer with each chain split over a lane pair (DPP) */
  S3H_KERNEL_QUAD = 4, /* as PAIR, each half-state on a lane quad: 9 instead of 10 VALU/round */
  S3H_KERNEL_SKEW = 5, /* lane quads with the a-quad two rounds behind: 8 VALU/round */
  S3H_KERNEL_SKEWP = 6, /* the same skewed schedule on lane pairs: 9 VALU/round, 32 chains/wave */
  S3H_KERNEL_SKEWS = 7  /* SKEW with each producer on its consumer's SIMD: 32 chains per CU */
};

enum s3h_algo {
  S3H_ALGO_SHA256 = 0, /* payload SHA-256 (x-amz-content-sha256), digests n x 8 words */
  S3H_ALGO_MD5 = 1,    /* MD5 (Content-MD5, multipart ETags), digests n x 4 words */
  S3H_ALGO_SHA1 = 2    /* SHA-1 (x-amz-checksum-sha1), digests n x 5 words, word i = bswap32(H_i) */
};

/* What AUTO optimises when several kernels fit a batch (s3h_kernel_policy).  They differ only
 * for 4,097 - 32 x CUs parts (8,192 on MI355X: the C4 shard), where the shared-SIMD SKEWS
 * kernel is ~5 % faster than SKEWP but draws 1.26-1.34 kW against 0.77 kW (2.57 vs 1.65 J/GiB):
 * S3H_POLICY_THROUGHPUT -- SKEWS; S3H_POLICY_EFFICIENCY -- SKEWP (the lower energy-delay
 * product); S3H_POLICY_POWER (default since API 2) -- SKEWS only when the device's board power
 * cap (sysfs hwmon power1_cap, s3h_device_power_cap) lets it hold its full clock (>= 1,500 W:
 * consumers and producers together need ~1.52 kW, more than MI355X's 1,400 W cap), SKEWP
 * otherwise.  Initial value from the environment: S3H_KERNEL_POLICY=throughput|efficiency|power
 * (S3H_PREFER_EFFICIENCY=1 = efficiency). */
enum s3h_policy { S3H_POLICY_THROUGHPUT = 0, S3H_POLICY_EFFICIENCY = 1, S3H_POLICY_POWER = 2 };

/* Last error message of the calling thread ("" if none). */
const char *s3h_last_error(void);
int s3h_api_version(void);
/* Free the host path's cached per-device contexts.  Between s3h_*_batch_host /
 * s3h_sha256_file_parts / s3h_verify_batch_host calls each device keeps one context:
 * streams, plans, digest buffers, copy threads, at most 1 GiB of HBM ring (larger rings are
 * freed when the call returns) and its pinned staging (96 MiB, up to 384 MiB after a
 * file-range call with thousands of parts).  Concurrent host calls on one device are merged
 * into one batch (their digests are the same as from separate calls).  s3h_trim releases the
 * contexts of idle devices. */
int s3h_trim(void);
/* Set AUTO's kernel policy for plans created afterwards (initially S3H_POLICY_POWER, see
 * above); *previous receives the old one.  No GPU. */
int s3h_kernel_policy(int policy, int *previous);
/* Board power cap of HIP device `device` in watts as the POWER policy reads it (0: unknown). */
int s3h_device_power_cap(int device, double *watts);
/* Host threads (the calling thread included) the host path uses per device to stage
 * pageable parts and file ranges when `ndevices` device shards run at once: the CPUs this
 * process may use -- its sched_getaffinity mask, capped by the cgroup CPU quota (cpu.max, or
 * cfs_quota_us / cfs_period_us) -- split evenly over the devices, at least 1 and at most 16.
 * *cpus (if non-null) receives that CPU count.  Needs no GPU.  The reference's jobs run on
 * the cores the host grants (lib/src/upload.cpp:136-140, std::async). */
int s3h_host_threads(int ndevices, int *cpus);
/* The host path's thread plan for a call over `ndevices` devices at PCI addresses
 * pci_bus_ids[k] (null entries or a null array: no NUMA record), with the CPUs of
 * `affinity_cpulist` ("0-63,128-191"; null: this process's affinity) under a cgroup quota of
 * `cpu_quota` CPUs (0: none; < 0: this process's quota) -- pure host arithmetic over sysfs
 * (S3H_SYSFS_ROOT replaces /sys), the rules the host pipeline and the split route apply, so an
 * N-GPU host can be checked before it runs:
 *   staging threads per device = min(16, max(1, cpus / ndevices)), each device's threads bound
 *   to its node's CPUs within the affinity; the split route from pinned parts gives the CPU side
 *   every thread, from staged sources each device tg of its share (1, 4, 6, 8, 9 twelfths) and
 *   the CPU side the rest.  devices (if non-null) receives ndevices records. */
typedef struct {
  int cpus;                       /* affinity capped by ceil(quota) */
  int affinity_cpus;
  double cpu_quota;               /* the quota applied (0: none) */
  int devices;
  int staging_threads_per_device; /* host threads staging one device's pageable parts / files */
  int threads;                    /* staging threads of the whole call */
  int oversubscribed;             /* threads > cpus (ndevices > cpus: one thread each anyway) */
  int below_saturation;           /* per-device staging < 6 threads: pageable sources below the
                                     H2D rate of one device (profiles/r05_stage_threads_sweep.json) */
  int node_oversubscribed;        /* some node's bound threads exceed its bindable CPUs */
  int split_cpu_threads_pinned;   /* split route, pinned parts: the CPU side's threads */
  int split_candidates;           /* split route, staged sources: staging-thread choices (0: none fits) */
  int split_stage_min, split_stage_max;            /* per device */
  int split_cpu_threads_min, split_cpu_threads_max; /* the CPU side's threads at those choices */
} s3h_host_plan_t;
typedef struct {
  int node;            /* sysfs numa_node (-1: unknown) */
  int bind_node;       /* node its threads and staging go to (-1: unbound) */
  int bind_cpus;       /* CPUs its shard / copy threads bind to (0: unbound) */
  int bind_first_cpu;  /* lowest and highest of them (-1: none) */
  int bind_last_cpu;
  int staging_threads;
} s3h_host_plan_device_t;
int s3h_host_plan(const char *const *pci_bus_ids, int ndevices, const char *affinity_cpulist,
                  double cpu_quota, s3h_host_plan_t *plan, s3h_host_plan_device_t *devices);
/* Number of visible HIP devices; S3H_ENODEV (and *count = 0) when there is none. */
int s3h_device_count(int *count);
/* PCI address of HIP device `device` as "dddd:bb:dd.f" (lowercase, NUL-terminated; len >= 13):
 * which physical GPU a device index names, so a multi-GPU run can show that its N ranks
 * hashed on N distinct devices.  S3H_ENODEV / S3H_EINVAL as s3h_plan_create. */
int s3h_device_pci_bus_id(int device, char *out, int len);

/* ---------------------------------------------------------------- NUMA placement
 * MI355X hosts are dual-socket with four GPUs behind each socket.  The host path puts each
 * device's pinned staging (pageable parts, file ranges, stream bookkeeping) on the device's
 * NUMA node and binds its copy threads -- and, for multi-device calls, each device's shard
 * thread -- to that node's CPUs within the process's affinity mask.  The reference's upload
 * jobs run wherever the host schedules them (lib/src/upload.cpp:136-140, std::async; bytes
 * read by ReadFile, lib/src/webclient.cpp:105-116).  None of these needs a GPU except where
 * stated; S3H_SYSFS_ROOT (tests) replaces /sys.
 *
 * NUMA record of a PCI function "dddd:bb:dd.f": sysfs numa_node (-1 when the platform gives
 * none), local_cpulist (into cpulist, NUL-terminated, truncated to len) and how many of those
 * CPUs this thread's affinity mask allows.  S3H_EINVAL when the function has no sysfs entry. */
int s3h_pci_numa(const char *pci_bus_id, int *node, char *cpulist, int len, int *usable_cpus);
/* The same for HIP device `device` (needs the device: its PCI address). */
int s3h_device_numa_node(int device, int *node, char *cpulist, int len);
/* Board power cap of the PCI function in watts (sysfs hwmon<k>/power1_cap; 0 when the platform
 * does not report one): what S3H_POLICY_POWER reads for a device.  No GPU needed. */
int s3h_pci_power_cap(const char *pci_bus_id, double *watts);
/* Placement policy of the host path: S3H_NUMA_LOCAL (default: each device's own node),
 * S3H_NUMA_OFF (no binding: the runtime's placement, unbound threads) or a node >= 0 (every
 * device's staging and threads on that node -- for local/remote measurements).  Initial value
 * from the environment: S3H_HOST_NUMA=local|off|<node>.  Idle cached contexts are released
 * so the next call re-places them.  *previous (if non-null) receives the old mode. */
#define S3H_NUMA_LOCAL (-1)
#define S3H_NUMA_OFF (-2)
int s3h_host_numa(int mode, int *previous);
typedef struct {
  int device_node;  /* sysfs numa_node of the device (-1: unknown) */
  int target_node;  /* node the policy places its staging on (-1: none) */
  int bound_cpus;   /* CPUs its copy / shard threads bind to (0: unbound) */
  int staging_node; /* measured node of the cached context's staging ring (-1: none yet) */
  int threads_node; /* node the cached context's copy threads are bound to (-1: unbound/none) */
  int copy_threads; /* copy threads of the cached context (0: none yet) */
} s3h_host_numa_t;
/* Placement of device `device` under the current policy, plus what its cached host context
 * actually holds (needs the device). */
int s3h_host_numa_info(int device, s3h_host_numa_t *info);
/* Pinned (page-locked, DMA-able) host memory whose pages are bound to NUMA node `node`
 * (-1: the runtime's placement): an uploader's read buffers on its device's node.  Needs a
 * HIP device.  Free with s3h_host_free. */
int s3h_host_alloc(int node, uint64_t bytes, void **out);
/* The same with flags.  Default (and s3h_host_alloc): the node is PREFERRED -- when it is short
 * of free memory the pages go to another node instead of the process being OOM-killed within
 * the node.  S3H_HOST_ALLOC_STRICT binds the pages to the node (MPOL_BIND) after checking that
 * the node has the bytes free (S3H_ENOMEM otherwise). */
#define S3H_HOST_ALLOC_STRICT 1
int s3h_host_alloc_ex(int node, uint64_t bytes, int flags, void **out);
int s3h_host_free(void *p);
/* NUMA node of the page holding host address p (get_mempolicy). */
int s3h_mem_node(const void *p, int *node);

/* ---------------------------------------------------------------- device-resident path
 * A plan captures the part geometry (byte offsets relative to a base pointer, lengths) of
 * one batch, sorted on the host by block count and uploaded once to `device`.  Launching it
 * hashes every part of a device buffer laid out that way; the same plan can be launched on
 * many buffers with that layout.  `stream` is a hipStream_t (NULL = the null stream). */
typedef struct s3h_plan_s *s3h_plan_t;

int s3h_plan_create(int device, const uint64_t *offsets, const uint64_t *lengths, uint64_t n,
                    int kernel, s3h_plan_t *plan);
/* Same for any algorithm (s3h_algo); digests are 8 (SHA-256), 4 (MD5) or 5 (SHA-1) words per
 * part.  MD5 and SHA-1 have one kernel each: S3H_KERNEL_AUTO or S3H_KERNEL_PC, any other is
 * S3H_EINVAL. */
int s3h_plan_create_ex(int device, int algo, const uint64_t *offsets, const uint64_t *lengths,
                       uint64_t n, int kernel, s3h_plan_t *plan);
int s3h_plan_algo(s3h_plan_t plan);
int s3h_plan_destroy(s3h_plan_t plan);
/* Asynchronous on `stream`: d_base and d_digests (n*8 uint32) are device pointers.  The
 * launch's success is known only after it has run: call s3h_plan_status before using the
 * digests.
 * Alignment of d_digests, here and in every device entry point that takes SHA-256 or MD5
 * digests (s3h_plan_launch / _launch_range, s3h_sha256_batch_device, s3h_md5_batch_device,
 * d_sha256 and d_md5 of s3h_sha256_md5_batch_device, s3h_stream_final_device): 16 bytes, the
 * kernels store a digest as one or two 16-byte words.  SHA-1 digests (5 words): 4 bytes.
 * d_base and the offsets may have any byte alignment.  A pointer that misses its alignment is
 * S3H_EINVAL, before anything is allocated or launched. */
int s3h_plan_launch(s3h_plan_t plan, const void *d_base, uint32_t *d_digests, void *stream);
/* Waits for `stream`, then reads and clears the plan's device error word, which every launch
 * of the plan (s3h_plan_launch / _range) ORs its faults into.  S3H_OK: the digests of every
 * launch since the last status call are valid.  S3H_EHIP ("synchronisation timeout"): a
 * flag-synchronised kernel (the two-group skew, shared-SIMD skew and dual-digest group
 * kernels pair a producer and a consumer wave through LDS step counters) gave up a bounded
 * wait, so the grid drained instead of hanging and those digests are NOT the parts' digests.
 * The one-shot, host, dual, verification and stream entry points check this word themselves
 * and fail the call; lib/hash's sha256() (sha256.cpp:147-160) never returns a wrong digest. */
int s3h_plan_status(s3h_plan_t plan, void *stream);
/* Resumable form: process blocks [blk_begin, blk_end) of every part, where part p's block b
 * lives at d_base + offsets[p] + 64*(b - blk_origin).  Chaining state is kept in the plan
 * between launches (same stream order required); a part's digest is written by the launch
 * that processes its final (padding) block. */
int s3h_plan_launch_range(s3h_plan_t plan, const void *d_base, uint32_t *d_digests,
                          uint64_t blk_begin, uint64_t blk_end, uint64_t blk_origin,
                          void *stream);
/* Introspection: total 64-B compressions, max blocks of any part, chosen kernel, grid size. */
int s3h_plan_info(s3h_plan_t plan, uint64_t *n, uint64_t *total_blocks, uint64_t *max_blocks,
                  int *kernel, uint32_t *grid);
/* Workgroup layout: consumer groups of the grid (skew/skewp kernels; 0 for the others) and how
 * many leading workgroups of the two-group skew kernel run one group on a CU of their own
 * (the groups of the longest parts of a ragged batch). */
int s3h_plan_groups(s3h_plan_t plan, uint32_t *groups, uint32_t *solo);
/* SHA-256 + MD5 of a SHA-256 plan's parts (s3h_sha256_md5_batch_*): how many leading
 * workgroups of the one-grid dual kernel run the longest parts as 8-part skew groups (a
 * ragged batch of 2,049 - 32 x CUs parts); 0 when the dual pass uses another form. */
int s3h_plan_dual_solo(s3h_plan_t plan, uint32_t *solo);
/* The same plus which form of that mixed grid runs: *apart = 1 when the skew groups' MD5
 * chains run on workgroups of their own (round 4, each skew group at the SHA-256-alone rate),
 * 0 when each skew group carries its MD5 wave (round 3; used when the apart grid would exceed
 * one workgroup per CU). */
int s3h_plan_dual_layout(s3h_plan_t plan, uint32_t *solo, int *apart);
/* That choice for a batch of `lengths` on a device of `cus` CUs, without a device (pure host
 * arithmetic, the rule the plan applies). */
int s3h_dual_layout(const uint64_t *lengths, uint64_t n, int cus, uint32_t *solo, int *apart);

/* Measurement hook (not part of the lib/hash surface): while d_clocks (device memory,
 * 4 x *waves uint64) is set, every launch of a plan on the skew kernel records, per consumer
 * wave, the shader-clock counter (s_memtime) and the 100 MHz real-time counter
 * (s_memrealtime) at the start and end of its chain loop: {clk0, clk1, rt0, rt1}.  *waves
 * receives the number of consumer waves (0: the plan's kernel does not record).  NULL turns
 * the probe off.  bench.py uses it to report cycles per block and the live shader clock. */
int s3h_plan_set_clock_probe(s3h_plan_t plan, uint64_t *d_clocks, uint32_t *waves);

/* One-shot convenience: plan + launch + wait.  Returns when d_digests (16-byte aligned) is
 * complete. */
int s3h_sha256_batch_device(int device, const void *d_base, const uint64_t *offsets,
                            const uint64_t *lengths, uint64_t n, uint32_t *d_digests,
                            void *stream);

/* Batched MD5 (lib/hash/md5.cpp semantics with md5_file's padding): n x 4 words, the
 * digest bytes in memory order (md5::hash_to_text prints them).  d_digests: 16-byte aligned. */
int s3h_md5_batch_device(int device, const void *d_base, const uint64_t *offsets,
                         const uint64_t *lengths, uint64_t n, uint32_t *d_digests, void *stream);

/* ---------------------------------------------------------------- host-resident path
 * parts[i] (host memory, pinned or pageable) of lengths[i] bytes -> digests (host, n*8).
 * Parts are sharded round-robin over `ndevices` GPUs (0 = all visible), part i on device
 * i % ndevices; each device streams its parts through HBM in slices of `slice_bytes` per
 * part with copies overlapped with hashing.  slice_bytes 0 = auto: pinned parts are DMA'd
 * directly (256 KiB slices and one 2-D copy per slice when they are equal-length chunks at a
 * constant host stride, 2 MiB per-part copies otherwise); pageable parts (e.g. an mmap'd
 * file) are first copied by host threads into a pinned staging ring (at most 32 MiB per
 * slot: slices of 32 MiB / n bytes, down to 64 B) and DMA'd from there; beyond 524,288
 * pageable parts, or when pinned memory is unavailable, each part is DMA'd from pageable memory.
 * Everything is cached per device between calls (s3h_trim).  Safe to call from concurrent
 * threads (concurrent calls on a device are merged into one batch, see
 * s3h_sha256_batch_host_on).  Blocking. */
int s3h_sha256_batch_host(const uint8_t *const *parts, const uint64_t *lengths, uint64_t n,
                          uint32_t *digests, int ndevices, uint64_t slice_bytes);

int s3h_md5_batch_host(const uint8_t *const *parts, const uint64_t *lengths, uint64_t n,
                       uint32_t *digests, int ndevices, uint64_t slice_bytes);

/* The same over an explicit device list: shard k = parts i with i % ndevices == k, hashed on
 * devices[k].  A device may be listed more than once: its shards then meet in that device's
 * queue like concurrent callers (below) and run merged into one batch, or one after another
 * when they arrive apart -- the digests are the same either way (this is how the sharding is
 * exercised on a one-GPU host).  Concurrent host calls on one device are merged in its queue:
 * the first caller runs every pending request with the same algorithms and slice size as one
 * batch; if that batch fails, each request is re-run on its own, so each caller gets its own
 * status.  Staging threads per device: s3h_host_threads(number of shards). */
int s3h_sha256_batch_host_on(const uint8_t *const *parts, const uint64_t *lengths, uint64_t n,
                             uint32_t *digests, const int *devices, int ndevices,
                             uint64_t slice_bytes);

/* Parts given as byte ranges of a file: part i = [offsets[i], offsets[i] + lengths[i]) of
 * `path` -- the (file, offset, size) parts that S3Api::UploadFilePart sends
 * (lib/src/api/multipart_upload.cpp:216-223 -> WebClient::UploadFile, webclient.cpp:331-355),
 * i.e. a batched sha256::sha256_file (lib/hash/sha256.cpp:183-233) over ranges.  Host threads
 * pread each slice straight into the pinned staging ring (no intermediate copy); its slots
 * are 128 MiB (32 KiB slices up to 4,096 parts per device), so the per-slice syscall does not
 * dominate.
 * S3H_EINVAL when the file cannot be opened or is shorter than a part.  Blocking. */
int s3h_sha256_file_parts(const char *path, const uint64_t *offsets, const uint64_t *lengths,
                          uint64_t n, uint32_t *digests, int ndevices, uint64_t slice_bytes);

/* ---------------------------------------------------------------- dual digest
 * x-amz-content-sha256 AND Content-MD5 of every part in one call (an upload that sends both
 * headers; the MD5s also give the multipart ETag).  Replaces a sha256::sha256 plus an
 * md5::md5 call per part (lib/hash/sha256.cpp:147-160, lib/hash/md5.cpp:71-180).
 * Both forms launch ONE grid whose workgroups run either the SHA-256 or the MD5 chain
 * (sha256_md5_dual_kernel) while it fits one workgroup per CU, so both digests take the
 * SHA-256 time; larger batches (> 32 x CUs parts, where each kernel fills the chip) run the
 * two kernels one after the other.  Host form: each slice
 * crosses PCIe ONCE for both digests (the host path is PCIe-bound).  Blocking.
 * sha256_digests: n x 8 words (lib/hash layout); md5_digests: n x 4 words (memory order). */
int s3h_sha256_md5_batch_host(const uint8_t *const *parts, const uint64_t *lengths, uint64_t n,
                              uint32_t *sha256_digests, uint32_t *md5_digests, int ndevices,
                              uint64_t slice_bytes);
/* Both digests of (file, offset, size) parts, each slice read once (pread into pinned
 * staging) and crossing PCIe once: s3h_sha256_file_parts for uploads that also send
 * Content-MD5.  Same arguments and errors as s3h_sha256_file_parts. */
/* Content-MD5 of (file, offset, size) parts, as s3h_sha256_file_parts. */
int s3h_md5_file_parts(const char *path, const uint64_t *offsets, const uint64_t *lengths,
                       uint64_t n, uint32_t *digests, int ndevices, uint64_t slice_bytes);
int s3h_sha256_md5_file_parts(const char *path, const uint64_t *offsets, const uint64_t *lengths,
                              uint64_t n, uint32_t *sha256_digests, uint32_t *md5_digests,
                              int ndevices, uint64_t slice_bytes);
/* Device form: d_sha256 and d_md5 are device pointers, each 16-byte aligned (S3H_EINVAL if
 * not).  The work runs on `stream`; the call returns when both are complete. */
int s3h_sha256_md5_batch_device(int device, const void *d_base, const uint64_t *offsets,
                                const uint64_t *lengths, uint64_t n, uint32_t *d_sha256,
                                uint32_t *d_md5, void *stream);

/* ---------------------------------------------------------------- size-aware routing
 * One part's chain runs at ~69 MB/s on the GPU and ~2.5 GB/s on one SHA-NI core, so a batch
 * of a few large parts -- the per-job batches of lib/src/upload.cpp:89-110, 136-140 -- is
 * faster on the CPU drop-in, and a batch of hundreds is faster on the GPU.  The routed entry
 * points take a route: S3H_ROUTE_GPU = the batched host path unchanged (the default
 * everywhere); S3H_ROUTE_CPU = the lib/hash drop-in (sha256::sha256, md5::md5, both digests in
 * one pass over each part) on s3h_host_threads' CPU count, parts longest first; S3H_ROUTE_AUTO
 * = whichever the model below estimates to finish first; S3H_ROUTE_SPLIT = both at once: the
 * CPU drop-in hashes the m longest parts on its threads while the GPU host path hashes the rest
 * (m from the model; a single part goes to the GPU; for pageable parts and file ranges the host
 * threads are divided between the GPU side's staging and the CPU side).  AUTO also splits when
 * the split is estimated at least 5 % faster than the better single route.  AUTO needs a
 * visible GPU (S3H_ENODEV otherwise): it chooses between paths with identical digests and is
 * never a fallback for a missing device.  *taken (if non-null) receives the route that ran.
 *   gpu_s = call_s + max(longest part / chain rate, bytes per device / feed rate)
 *           feed = h2d (pinned parts), min(h2d, staged memcpy) (pageable parts) or
 *                  min(h2d, staged pread) (file ranges)
 *   cpu_s = (longest-first schedule of the parts on k = min(n, threads) threads) / (rate(k) / k)
 *           rate(k) = min(k x one-thread rate, all-threads rate)
 * each for the digest set the call computes (SHA-256, MD5, or both), times the observed /
 * predicted ratio of earlier routed calls (the model is measured lazily per digest set and per
 * device, re-measured when a call diverges from its prediction by more than 25 % and every
 * s3h_route_refresh_calls calls). */
enum s3h_route { S3H_ROUTE_GPU = 0, S3H_ROUTE_CPU = 1, S3H_ROUTE_AUTO = 2, S3H_ROUTE_SPLIT = 3 };
/* Digest sets of the routing model: rate arrays are indexed by (set - 1). */
enum s3h_digests { S3H_DIGESTS_SHA256 = 1, S3H_DIGESTS_MD5 = 2, S3H_DIGESTS_BOTH = 3 };
/* The SHA-256 model (layout frozen at API version 1 + round 5's two trailing doubles). */
typedef struct {
  double cpu_bytes_per_s;   /* one host thread on the lib/hash drop-in (s3h_cpu_backend) */
  double chain_bytes_per_s; /* one part's chain on the GPU (the slowest visible device) */
  double h2d_bytes_per_s;   /* pinned host -> device copy (the slowest visible device) */
  double call_s;            /* fixed cost of one host-path GPU call (setup, launch, sync) */
  int cpu_threads;          /* host threads of the CPU route (affinity and cgroup quota) */
  int devices;              /* visible HIP devices */
  double cpu_all_bytes_per_s; /* all cpu_threads threads at once, aggregate: the CPU route on k
                               * threads runs at min(k x cpu_bytes_per_s, this) -- not linear
                               * (memory bandwidth, SMT siblings, the cgroup quota) */
  double staged_bytes_per_s;  /* pageable sources: cpu_threads threads' memcpy into pinned
                               * staging, aggregate; the GPU route is fed at min(h2d, this) */
} s3h_route_model_t;
/* The measured model (measures it on first use).  S3H_ENODEV without a GPU (cpu fields set). */
int s3h_route_model(s3h_route_model_t *m);
/* AUTO's choice for `lengths` under model *m (any model, e.g. a recorded one; pure host
 * arithmetic): returns S3H_ROUTE_GPU or S3H_ROUTE_CPU and both time estimates in seconds. */
int s3h_route_estimate(const s3h_route_model_t *m, const uint64_t *lengths, uint64_t n,
                       int ndevices, double *gpu_s, double *cpu_s);
/* The same for parts of a given source: S3H_SOURCE_PINNED (as s3h_route_estimate),
 * S3H_SOURCE_PAGEABLE (staged through pinned memory) or S3H_SOURCE_FILE (file ranges). */
enum s3h_source { S3H_SOURCE_PINNED = 0, S3H_SOURCE_PAGEABLE = 1, S3H_SOURCE_FILE = 2 };
int s3h_route_estimate_ex(const s3h_route_model_t *m, const uint64_t *lengths, uint64_t n,
                          int ndevices, int source, double *gpu_s, double *cpu_s);
/* The split route's plan under model *m (pure host arithmetic): with the parts ordered by length
 * (descending, ties by index), the first *cpu_parts go to the CPU and the rest to the GPU, and
 *   split_s(m) = max(gpu_s(the n - m shorter parts), cpu_s(the m longest)),  m = 1 .. n-1
 * (gpu_s / cpu_s as above on each side's parts); of the m with split_s(m) within 0.5 % of the
 * minimum (the GPU side's longest chain makes ranges of m tie), *cpu_parts = the one with the
 * smallest max(GPU side's bytes / devices / feed, cpu_s(m)), and *split_s = split_s(it)
 * (*cpu_parts = 0 when n == 1).  Pinned parts: the CPU side gets all cpu_threads threads
 * (*stage_threads = 0).  Pageable parts / file ranges: each GPU shard stages with
 * *stage_threads = tg threads, fed at min(H2D, staged rate x tg / threads), and the CPU side
 * gets the rest at the all-threads rate per thread; tg is the best of (threads / devices) x
 * {1, 4, 6, 8, 9} / 12 (env S3H_SPLIT_STAGE_THREADS fixes it). */
int s3h_route_split_estimate(const s3h_route_model_t *m, const uint64_t *lengths, uint64_t n,
                             int ndevices, int source, uint64_t *cpu_parts, int *stage_threads,
                             double *split_s);
/* The whole model, every digest set, with the observed corrections.  The caller sets `size`
 * (sizeof(s3h_route_rates_t) as it was compiled); the library writes at most that many bytes,
 * so a caller built against an older, shorter struct keeps working. */
typedef struct {
  uint32_t size;                  /* in: the struct size the caller knows; out: bytes written */
  uint32_t version;               /* out: the library's S3H_API_VERSION */
  int cpu_threads;                /* host threads of the CPU route */
  int devices;                    /* visible HIP devices */
  double cpu_bytes_per_s[3];      /* one host thread, per digest set (index = set - 1) */
  double cpu_all_bytes_per_s[3];  /* all cpu_threads threads, aggregate */
  double chain_bytes_per_s[3];    /* one GPU chain (the slowest device); [2]: both digests from one grid */
  double h2d_bytes_per_s;         /* pinned host -> device (the slowest device) */
  double staged_bytes_per_s;      /* staging memcpy of all cpu_threads threads */
  double call_s;                  /* fixed cost of one host-path GPU call */
  double gpu_factor[3];           /* observed / predicted wall time of routed calls, per digest */
  double cpu_factor[3];           /* set (EWMA; 1: none; 0 = 1 in s3h_route_choose) */
  uint64_t measurements;          /* times the model was (re)measured */
  uint64_t routed_calls;          /* AUTO / SPLIT calls observed */
  uint64_t divergences;           /* calls that differed from their prediction by > 25 % */
  double age_s;                   /* seconds since the last measurement */
  double staged_file_bytes_per_s; /* file ranges: cpu_threads threads' pread from the page cache
                                   * (0: price them at staged_bytes_per_s) */
} s3h_route_rates_t;
int s3h_route_rates(s3h_route_rates_t *r);
/* AUTO's decision for digest set `digests` under rates *r (pure host arithmetic; reads at most
 * r->size bytes, missing fields = 0, factors 0 = 1; the digest set's own factors apply). */
typedef struct {
  int route;           /* S3H_ROUTE_GPU, _CPU or _SPLIT */
  int stage_threads;   /* split: staging threads per GPU shard (0: pinned parts / no split) */
  uint64_t cpu_parts;  /* split: the longest parts on the CPU (0: no split plan) */
  double gpu_s, cpu_s; /* estimates with the observed factors */
  double split_s;      /* the split plan's estimate (0: none) */
} s3h_route_choice_t;
int s3h_route_choose(const s3h_route_rates_t *r, int digests, const uint64_t *lengths, uint64_t n,
                     int ndevices, int source, s3h_route_choice_t *out);
/* One device's lone-chain rate for a digest set and its pinned H2D rate (measured on first use). */
int s3h_route_device_rates(int device, int digests, double *chain_bytes_per_s,
                           double *h2d_bytes_per_s);
/* Re-measure the model after this many AUTO / SPLIT calls (default 64, env
 * S3H_ROUTE_REFRESH_CALLS; 0: only on divergence).  *previous (if non-null) gets the old value. */
int s3h_route_refresh_calls(int calls, int *previous);
/* Measurement / test hook: multiply one measured rate by `factor` until the model is next
 * measured -- a model taken while the GPU or the host was busy (tests/test_gpu_route_adapt.py). */
enum s3h_rate { S3H_RATE_CHAIN = 0, S3H_RATE_H2D = 1, S3H_RATE_CPU = 2, S3H_RATE_STAGED = 3 };
int s3h_route_scale(int which, double factor);
int s3h_sha256_batch_routed(const uint8_t *const *parts, const uint64_t *lengths, uint64_t n,
                            uint32_t *digests, int ndevices, int route, int *taken);
int s3h_sha256_file_parts_routed(const char *path, const uint64_t *offsets,
                                 const uint64_t *lengths, uint64_t n, uint32_t *digests,
                                 int ndevices, int route, int *taken);
/* Content-MD5 of host parts on a route (the CPU side: md5::md5). */
int s3h_md5_batch_routed(const uint8_t *const *parts, const uint64_t *lengths, uint64_t n,
                         uint32_t *digests, int ndevices, int route, int *taken);
/* Both upload headers on a route: the GPU side is s3h_sha256_md5_batch_host /
 * _file_parts (one grid, one PCIe pass), the CPU side hashes each part with SHA-256 and MD5 in
 * one pass over memory (64 KiB chunks while they sit in cache); the model prices both digests
 * (a CPU MD5 runs at ~1.0 GB/s per thread, both digests at ~0.7: the dual CPU route is ~3.5x
 * slower per thread than SHA-256 alone, so the GPU wins at far fewer parts). */
int s3h_sha256_md5_batch_routed(const uint8_t *const *parts, const uint64_t *lengths, uint64_t n,
                                uint32_t *sha256_digests, uint32_t *md5_digests, int ndevices,
                                int route, int *taken);
int s3h_sha256_md5_file_parts_routed(const char *path, const uint64_t *offsets,
                                     const uint64_t *lengths, uint64_t n, uint32_t *sha256_digests,
                                     uint32_t *md5_digests, int ndevices, int route, int *taken);

/* ---------------------------------------------------------------- verification
 * Download-side check of parts against known digests (ranged GETs of
 * lib/src/download.cpp:88-103; expected = the uploader's x-amz-content-sha256 / Content-MD5 /
 * x-amz-checksum-sha1).  `expected` holds n x words 32-bit words in the layout the batch calls
 * write: 8 per part for S3H_ALGO_SHA256, 4 for S3H_ALGO_MD5, 5 for S3H_ALGO_SHA1; every word is
 * compared.  A successful call writes all n bytes of `mismatch`, whatever they held: mismatch[i]
 * = 1 when part i differs, 0 when it matches (an empty part matches the digest of the empty
 * message); no byte behind mismatch[n - 1] is touched; *mismatches is stored (not added to) and
 * equals the sum of the n bytes.  The CRC forms (s3h_crc_verify_batch_device,
 * s3h_crc64nvme_verify_batch_device) keep the same contract with 1 and 2 words per value.
 * Blocking.  Device form: d_expected (n x words, 4-byte aligned) and d_mismatch (n bytes) are
 * device pointers; the comparison runs on `stream`, behind work queued there earlier (such as
 * a launch that is still writing d_expected). */
int s3h_verify_batch_device(int device, int algo, const void *d_base, const uint64_t *offsets,
                            const uint64_t *lengths, uint64_t n, const uint32_t *d_expected,
                            uint8_t *d_mismatch, uint64_t *mismatches, void *stream);
int s3h_verify_batch_host(int algo, const uint8_t *const *parts, const uint64_t *lengths,
                          uint64_t n, const uint32_t *expected, uint8_t *mismatch,
                          uint64_t *mismatches, int ndevices);
/* The host form on a route (size-aware routing above): S3H_ROUTE_GPU = s3h_verify_batch_host;
 * CPU / SPLIT / AUTO hash as s3h_sha256_batch_routed / s3h_md5_batch_routed do (either
 * algorithm, priced by its own rates), then compare.  *taken (if non-null) receives the route
 * that ran. */
int s3h_verify_batch_routed(int algo, const uint8_t *const *parts, const uint64_t *lengths,
                            uint64_t n, const uint32_t *expected, uint8_t *mismatch,
                            uint64_t *mismatches, int ndevices, int route, int *taken);

/* ---------------------------------------------------------------- multi-object streams
 * n messages (objects) hashed incrementally as their bytes arrive in chunks: the batched,
 * device-resident form of lib/hash's chunked API -- sha256_stream (sha256.cpp:84-144) for the
 * appends, and the DOCUMENTED contract of sha256_next (sha256.h:73-89: chunks of one buffer,
 * the last one padded with the buffer's TOTAL length) for the finish.  (The reference's
 * sha256_next pads with the chunk length and hashes unpadded data)
 *   update: appends chunk i (lengths[i] bytes, any alignment, 0 allowed) to message i.
 *           Whole 64-B blocks are compressed on the GPU; each message's < 64-B remainder is
 *           carried on the device into the next update.  Asynchronous on `stream`; the host
 *           arrays may be reused on return, the device chunks must stay valid until the
 *           stream reaches this point.  An object's calls run on the device in call order,
 *           whichever stream each is given (each waits for the previous call's work).
 *   final:  pads every message with its total length, writes n digests (words as in the
 *           batch API) and resets the object to n empty messages.  d_digests of the device
 *           form is 16-byte aligned for SHA-256 and MD5, 4-byte for SHA-1 (S3H_EINVAL if not).
 * The chaining state, carries and total lengths live on the device (n x 104 B); one object
 * may be driven from one host thread at a time.  MD5 (algo 1) follows md5_stream/md5_file. */
typedef struct s3h_stream_s *s3h_stream_t;
int s3h_stream_create(int device, int algo, uint64_t n, int kernel, s3h_stream_t *out);
int s3h_stream_update_device(s3h_stream_t s, const void *d_base, const uint64_t *offsets,
                             const uint64_t *lengths, void *stream);
int s3h_stream_final_device(s3h_stream_t s, uint32_t *d_digests, void *stream);
/* Host-memory forms: chunks[i] may be null when lengths[i] == 0.  update_host returns once
 * the chunks have been copied out of the caller's memory (they may be reused on return); its
 * hash runs on the device while the caller prepares the next update, whose copy overlaps it.
 * Page-locked chunks are DMA'd directly; pageable ones go through pinned pieces filled by copy
 * threads on the device's NUMA node.  final_host waits for every update and checks the
 * launches' device error words like s3h_plan_status (a fault of any update fails it). */
int s3h_stream_update_host(s3h_stream_t s, const uint8_t *const *chunks, const uint64_t *lengths);
int s3h_stream_final_host(s3h_stream_t s, uint32_t *digests);
/* Device forms: waits for `stream` and reports (and clears) a fault of any update / final
 * launch since the last check, as s3h_plan_status does for a plan. */
int s3h_stream_status(s3h_stream_t s, void *stream);
/* Update launches that found their plan's device slots in place (equal chunk lengths at
 * offsets moved by one constant: the base pointer moves, no re-sort, no copies) and those
 * that re-sorted and uploaded the slots.  Host counters, no device sync.  A call that fails
 * after queueing work leaves the object failed: later calls return S3H_EINVAL (destroy it). */
int s3h_stream_stats(s3h_stream_t s, uint64_t *slot_reuses, uint64_t *slot_refills);
/* Bytes appended so far to message i (host bookkeeping; no device sync). */
int s3h_stream_total(s3h_stream_t s, uint64_t i, uint64_t *total);
int s3h_stream_destroy(s3h_stream_t s);

/* ---------------------------------------------------------------- CRC-32C / CRC-32 checksums
 * S3's "additional checksums" (x-amz-checksum-crc32c / x-amz-checksum-crc32 on UploadPart, the
 * full-object or composite value on CompleteMultipartUpload; <ChecksumAlgorithm> in
 * lib/src/api/xml_parser.cpp:94) for device-resident parts.  Both are reflected 32-bit CRCs
 * with init and xor-out 0xFFFFFFFF: CRC-32C = Castagnoli (0x82F63B78), CRC-32 = ISO-HDLC /
 * zlib (0xEDB88320).  Output layout (every entry point): one uint32 per part, in part order,
 * holding the CRC's numeric value (what zlib.crc32 returns); a part of length 0 gives 0.
 *
 * A CRC is linear, so each part is cut into segments (s3h_crc_plan_info: segment_bytes, chosen
 * by the plan from the batch) that are checksummed independently -- one wave each -- and folded
 * per part by a second launch: a single large part uses the whole GPU.  Offsets may have any
 * byte alignment.  The segment values live in a buffer the plan owns: launch one plan on ONE
 * stream at a time (as for s3h_plan_launch); launches on one stream may follow each other
 * without a sync.  Host-resident data: s3h_sha256_crc_batch_host / s3h_sha256_crc_file_parts
 * below give the CRC out of the SHA-256 pass (each part crosses the host link once), and
 * s3h_crc_batch_host the CRC alone; s3h_cpu_crc is the CPU function (a CRC alone from host
 * memory is bounded by the host link, which a few cores match for CRC-32C but not for CRC-32,
 * which has no CPU instruction).  Added within API version 2. */
enum s3h_crc { S3H_CRC32C = 0, S3H_CRC32 = 1 };
typedef struct s3h_crc_plan_s *s3h_crc_plan_t;
int s3h_crc_plan_create(int device, int crc, const uint64_t *offsets, const uint64_t *lengths,
                        uint64_t n, s3h_crc_plan_t *plan);
/* Asynchronous on `stream`: d_crcs (n words, device, 4-byte aligned) is complete when the
 * stream reaches it. */
int s3h_crc_plan_launch(s3h_crc_plan_t plan, const void *d_base, uint32_t *d_crcs, void *stream);
/* Resumable form (as s3h_plan_launch_range, in bytes): process bytes [byte_begin, byte_end) of
 * every part, where part p's byte b lives at d_base + offsets[p] + (b - byte_origin).  Each
 * part's running value is kept in the plan between launches (same stream order required).
 * A part's CRC is written to d_crcs[p] by the launch whose range holds its last byte.
 * A part of length 0 is written by a launch with byte_begin == 0.  No other entry of d_crcs
 * is touched.  A launch with byte_begin == 0 starts over.  Otherwise byte_begin must equal
 * the previous ranged launch's byte_end (S3H_EINVAL if not, or if byte_begin >= byte_end or
 * byte_origin > byte_begin).  Any byte values: no alignment is required of the range, the
 * offsets or the base.  A launch allocates nothing, uploads nothing and does not wait for
 * the device.  s3h_crc_plan_launch leaves the running values unspecified: the next ranged
 * launch after one must begin at 0.  Asynchronous on `stream`. */
int s3h_crc_plan_launch_range(s3h_crc_plan_t plan, const void *d_base, uint32_t *d_crcs,
                              uint64_t byte_begin, uint64_t byte_end, uint64_t byte_origin,
                              void *stream);
/* n parts, segments in all, bytes per segment, workgroups of the segment launch (any may be null). */
int s3h_crc_plan_info(s3h_crc_plan_t plan, uint64_t *n, uint64_t *segments, uint64_t *segment_bytes,
                      uint32_t *grid);
int s3h_crc_plan_destroy(s3h_crc_plan_t plan);
/* One-shot, blocking: plan + launch + sync. */
int s3h_crc_batch_device(int device, int crc, const void *d_base, const uint64_t *offsets,
                         const uint64_t *lengths, uint64_t n, uint32_t *d_crcs, void *stream);
/* As s3h_verify_batch_device, against n expected CRCs (device).  Blocking. */
int s3h_crc_verify_batch_device(int device, int crc, const void *d_base, const uint64_t *offsets,
                                const uint64_t *lengths, uint64_t n, const uint32_t *d_expected,
                                uint8_t *d_mismatch, uint64_t *mismatches, void *stream);
/* Host-resident parts (pinned or pageable memory, or byte ranges of a file), arguments as for
 * s3h_sha256_batch_host / s3h_sha256_md5_batch_host / s3h_sha256_md5_file_parts: every slice
 * crosses the host link once and is hashed from the HBM ring by SHA-256 and by a ranged CRC
 * launch on streams of their own.  `crc` is an enum s3h_crc; `crcs` receives n words in part
 * order.  The route is the GPU (never a CPU fallback: no visible device is S3H_ENODEV); an
 * unknown `crc` or a null pointer is S3H_EINVAL.  Blocking.  Concurrent callers that ask for
 * the same digests are merged into one batch, as for the SHA-256 forms. */
int s3h_crc_batch_host(int crc, const uint8_t *const *parts, const uint64_t *lengths, uint64_t n,
                       uint32_t *crcs, int ndevices, uint64_t slice_bytes);
int s3h_sha256_crc_batch_host(int crc, const uint8_t *const *parts, const uint64_t *lengths,
                              uint64_t n, uint32_t *sha256_digests, uint32_t *crcs,
                              int ndevices, uint64_t slice_bytes);
int s3h_sha256_crc_file_parts(int crc, const char *path, const uint64_t *offsets,
                              const uint64_t *lengths, uint64_t n, uint32_t *sha256_digests,
                              uint32_t *crcs, int ndevices, uint64_t slice_bytes);
/* CPU, one message.  seed_crc: 0, or a previous call's result, so chunks chain like zlib's
 * crc32(data, seed).  CRC-32C uses the SSE4.2 instruction where the CPU has it
 * (S3H_CPU_SCALAR=1 forces the table path).  Unknown `crc`: returns 0 and sets s3h_last_error. */
uint32_t s3h_cpu_crc(int crc, const uint8_t *data, uint64_t length, uint32_t seed_crc);
/* crc(A || B) from crc(A), crc(B) and |B| (zlib's crc32_combine), without the data. */
int s3h_crc_combine(int crc, uint32_t crc_a, uint32_t crc_b, uint64_t len_b, uint32_t *out);
/* FULL_OBJECT checksum: the CRC of the n parts' concatenation from their CRCs and lengths. */
int s3h_crc_object(int crc, const uint32_t *part_crcs, const uint64_t *lengths, uint64_t n,
                   uint32_t *out);
/* Header text, NUL-terminated, out_len >= S3H_CHECKSUM_MAX.  composite = 0: n must be 1, the
 * value of x-amz-checksum-crc32c / -crc32 (base64 of the CRC's 4 bytes, big-endian) -- of a
 * part, or of s3h_crc_object's result for the FULL_OBJECT form.  composite = 1: the COMPOSITE
 * form, base64 of the CRC of the n big-endian part CRCs concatenated, then "-n". */
#define S3H_CHECKSUM_MAX 32
int s3h_checksum_text(int crc, const uint32_t *part_crcs, uint64_t n, int composite, char *out,
                      uint64_t out_len);

/* ---------------------------------------------------------------- CRC-64/NVME checksum
 * x-amz-checksum-crc64nvme, the checksum S3 computes for every new object and current SDKs
 * send by default: the reflected 64-bit CRC of the NVMe specification (polynomial
 * 0xAD93D23594C93659, reflected 0x9A6C9329AC4BC9B5, init and xor-out all ones;
 * "123456789" gives 0xAE8B14860A799888).  Values are uint64_t holding the CRC's numeric value;
 * a part of length 0 gives 0.  S3 offers this checksum as FULL_OBJECT only: a multipart
 * uploader sends each part's value with UploadPart and folds them with s3h_crc64nvme_object for
 * CompleteMultipartUpload; there is no COMPOSITE form.
 *
 * The plan calls have the contracts of their s3h_crc_* namesakes above -- segments, one plan
 * on one stream at a time, which ranged launch writes which d_crcs[p], byte_begin 0 or the
 * previous byte_end -- with d_crcs holding n 64-bit words (8-byte aligned).  The enum s3h_crc
 * entry points do not accept this checksum.  Added within API version 2. */
typedef struct s3h_crc64nvme_plan_s *s3h_crc64nvme_plan_t;
int s3h_crc64nvme_plan_create(int device, const uint64_t *offsets, const uint64_t *lengths,
                              uint64_t n, s3h_crc64nvme_plan_t *plan);
int s3h_crc64nvme_plan_launch(s3h_crc64nvme_plan_t plan, const void *d_base, uint64_t *d_crcs,
                              void *stream);
int s3h_crc64nvme_plan_launch_range(s3h_crc64nvme_plan_t plan, const void *d_base,
                                    uint64_t *d_crcs, uint64_t byte_begin, uint64_t byte_end,
                                    uint64_t byte_origin, void *stream);
int s3h_crc64nvme_plan_info(s3h_crc64nvme_plan_t plan, uint64_t *n, uint64_t *segments,
                            uint64_t *segment_bytes, uint32_t *grid);
int s3h_crc64nvme_plan_destroy(s3h_crc64nvme_plan_t plan);
/* One-shot, blocking: plan + launch + sync. */
int s3h_crc64nvme_batch_device(int device, const void *d_base, const uint64_t *offsets,
                               const uint64_t *lengths, uint64_t n, uint64_t *d_crcs,
                               void *stream);
/* As s3h_crc_verify_batch_device, against n expected 64-bit values (device).  Blocking. */
int s3h_crc64nvme_verify_batch_device(int device, const void *d_base, const uint64_t *offsets,
                                      const uint64_t *lengths, uint64_t n,
                                      const uint64_t *d_expected, uint8_t *d_mismatch,
                                      uint64_t *mismatches, void *stream);
/* Host-resident parts, as s3h_crc_batch_host / s3h_sha256_crc_batch_host /
 * s3h_sha256_crc_file_parts: `crcs` receives n 64-bit values in part order. */
int s3h_crc64nvme_batch_host(const uint8_t *const *parts, const uint64_t *lengths, uint64_t n,
                             uint64_t *crcs, int ndevices, uint64_t slice_bytes);
int s3h_sha256_crc64nvme_batch_host(const uint8_t *const *parts, const uint64_t *lengths,
                                    uint64_t n, uint32_t *sha256_digests, uint64_t *crcs,
                                    int ndevices, uint64_t slice_bytes);
int s3h_sha256_crc64nvme_file_parts(const char *path, const uint64_t *offsets,
                                    const uint64_t *lengths, uint64_t n, uint32_t *sha256_digests,
                                    uint64_t *crcs, int ndevices, uint64_t slice_bytes);
/* CPU, one message (slicing-by-8 tables).  seed_crc: 0, or a previous call's result, so chunks
 * chain.  Null data with length > 0: returns 0 and sets s3h_last_error. */
uint64_t s3h_cpu_crc64nvme(const uint8_t *data, uint64_t length, uint64_t seed_crc);
/* crc(A || B) from crc(A), crc(B) and |B|, without the data. */
int s3h_crc64nvme_combine(uint64_t crc_a, uint64_t crc_b, uint64_t len_b, uint64_t *out);
/* FULL_OBJECT checksum: the CRC of the n parts' concatenation from their CRCs and lengths. */
int s3h_crc64nvme_object(const uint64_t *part_crcs, const uint64_t *lengths, uint64_t n,
                         uint64_t *out);
/* Header text of a 64-bit checksum, NUL-terminated, out_len >= S3H_CHECKSUM_MAX: the value of
 * x-amz-checksum-crc64nvme, base64 of the CRC's 8 bytes, big-endian (12 characters) -- of a
 * part, or of s3h_crc64nvme_object's result. */
int s3h_checksum64_text(uint64_t crc, char *out, uint64_t out_len);

/* ---------------------------------------------------------------- SHA-1 checksum
 * x-amz-checksum-sha1 (objects stored with ChecksumAlgorithm=SHA1).  Digests are 5 uint32 words
 * per part with word i = bswap32(H_i): the 20 bytes in memory are the canonical digest, the
 * convention of SHA-256.  Plans (s3h_plan_create_ex with S3H_ALGO_SHA1: whole and ranged
 * launches, status, info), streams (s3h_stream_create) and s3h_verify_batch_device /
 * s3h_verify_batch_host take the algorithm id; the entry points below have the arguments and
 * errors of their MD5 namesakes.  The routed calls (AUTO / CPU / SPLIT) do not take SHA-1:
 * S3H_EINVAL.  Added within API version 2. */
/* One-shot, blocking: plan + launch + sync.  d_digests: n x 5 words (4-byte aligned). */
int s3h_sha1_batch_device(int device, const void *d_base, const uint64_t *offsets,
                          const uint64_t *lengths, uint64_t n, uint32_t *d_digests, void *stream);
int s3h_sha1_batch_host(const uint8_t *const *parts, const uint64_t *lengths, uint64_t n,
                        uint32_t *digests, int ndevices, uint64_t slice_bytes);
int s3h_sha1_file_parts(const char *path, const uint64_t *offsets, const uint64_t *lengths,
                        uint64_t n, uint32_t *digests, int ndevices, uint64_t slice_bytes);
/* x-amz-content-sha256 AND x-amz-checksum-sha1 of every part from one pass over the host link
 * (two kernels on two hash streams per slice or group).  sha256_digests: n x 8 words;
 * sha1_digests: n x 5 words. */
int s3h_sha256_sha1_batch_host(const uint8_t *const *parts, const uint64_t *lengths, uint64_t n,
                               uint32_t *sha256_digests, uint32_t *sha1_digests, int ndevices,
                               uint64_t slice_bytes);
int s3h_sha256_sha1_file_parts(const char *path, const uint64_t *offsets, const uint64_t *lengths,
                               uint64_t n, uint32_t *sha256_digests, uint32_t *sha1_digests,
                               int ndevices, uint64_t slice_bytes);
/* CPU, one message: SHA-NI when the CPU has it, else portable scalar code (S3H_CPU_SCALAR=1
 * forces the scalar path; s3h_cpu_backend names the choice).  Same word convention. */
void s3h_cpu_sha1(const uint8_t *data, uint64_t length, uint32_t hash[5]);
/* Header text of a digest checksum, NUL-terminated, out_len >= S3H_DIGEST_CHECKSUM_MAX.
 * algo: S3H_ALGO_SHA1 or S3H_ALGO_SHA256 (MD5: S3H_EINVAL, see s3h_multipart_etag); digests:
 * n x 5 or n x 8 words as the batch entry points return them.  composite = 0: n must be 1, the
 * value of x-amz-checksum-sha1 / -sha256 of a part or a single-PUT object (base64 of the 20 or
 * 32 digest bytes).  composite = 1: the COMPOSITE checksum of a multipart object, base64 of
 * the same hash over the n raw digests concatenated, then "-n".  CPU only. */
#define S3H_DIGEST_CHECKSUM_MAX 64
int s3h_digest_checksum_text(int algo, const uint32_t *digests, uint64_t n, int composite,
                             char *out, uint64_t out_len);

/* ---------------------------------------------------------------- SigV4 chunk-signed uploads
 * An aws-chunked body under x-amz-content-sha256: STREAMING-AWS4-HMAC-SHA256-PAYLOAD (what the
 * AWS SDKs send when they stream a body over plain HTTP) needs no whole-part SHA-256: the part is
 * cut into chunks of chunk_bytes (the last may be short; the server asks for >= 8 KiB, the SDKs
 * use 64 KiB), each chunk is hashed on its own, and a chain of HMACs links them:
 *   sig_i = HMAC-SHA256(signing_key, "AWS4-HMAC-SHA256-PAYLOAD\n" timestamp "\n"
 *             date "/" region "/" service "/aws4_request\n" hex(sig_{i-1}) "\n"
 *             hex(sha256("")) "\n" hex(sha256(chunk_i)))
 * sig_0 being the seed: the signature of the request's headers (computed with the payload hash
 * "STREAMING-AWS4-HMAC-SHA256-PAYLOAD").  A final chunk of 0 bytes closes the body, so a part of
 * L bytes has ceil(L / chunk_bytes) data chunks and one signature more (an empty part: one).
 * Signatures are stored like SHA-256 digests: 8 words each, word i = bswap32(H_i), the 32 raw
 * bytes in memory; seeds likewise, one per part.  `signatures` arrays are part-major: part p's
 * signatures follow part p-1's.  The chunk hashes are independent, so one large part fills the
 * GPU; the chain of a part is serial and ~6 compressions per chunk.  Device-resident plans run
 * it on the device behind the hash launch (stream-ordered, no host work between); the
 * host-resident entry point runs it on the CPU, where the digests land anyway.  A device caller
 * with a few long parts is better off hashing the chunks with an ordinary SHA-256 plan and
 * calling s3h_cpu_chunk_signatures: one GPU lane walks a chain ~100x slower than one CPU core.
 * The trailer variant (...-PAYLOAD-TRAILER): the section after this one.  Added within API
 * version 2. */
typedef struct s3h_chunk_sign_ctx_s *s3h_chunk_sign_ctx_t;
typedef struct s3h_chunk_plan_s *s3h_chunk_plan_t;
/* signing_key = HMAC(HMAC(HMAC(HMAC("AWS4" + secret, date), region), service), "aws4_request")
 * (NUL-terminated strings).  CPU. */
int s3h_sigv4_signing_key(const char *secret, const char *date, const char *region,
                          const char *service, uint8_t key[32]);
/* The constant part of every chunk's string to sign, hashed once: timestamp "YYYYMMDDThhmmssZ"
 * (16 bytes), date "YYYYMMDD" (8 bytes), region and service non-empty and together at most 190
 * bytes (the prefix is 66 + |region| + |service| <= 256 bytes); S3H_EINVAL otherwise.  CPU; a
 * context is immutable and may be used from any number of threads and launches at once. */
int s3h_chunk_sign_ctx_create(const uint8_t key[32], const char *timestamp, const char *date,
                              const char *region, const char *service, s3h_chunk_sign_ctx_t *out);
int s3h_chunk_sign_ctx_destroy(s3h_chunk_sign_ctx_t ctx);
/* The chain on the CPU over ready chunk digests: chunk_digests holds the data chunks' SHA-256
 * digests (8 words each), part-major, data_chunks_per_part[p] of them for part p (the final
 * chunk's hash is implied; chunk_digests may be null when there is no data chunk); seeds n x 8
 * words; signatures receives sum(data_chunks_per_part[p] + 1) x 8 words.  Parts are spread over
 * the host threads s3h_host_threads(1) reports. */
int s3h_cpu_chunk_signatures(s3h_chunk_sign_ctx_t ctx, const uint32_t *chunk_digests,
                             const uint64_t *data_chunks_per_part, uint64_t n, const uint32_t *seeds,
                             uint32_t *signatures);
/* The framing line an uploader writes before a chunk's bytes (and "\r\n" after them):
 * "<chunk_len in hex>;chunk-signature=<64 hex>\r\n", NUL-terminated, out_len >=
 * S3H_CHUNK_HEADER_MAX.  The body ends with the line of chunk_len 0 and a last "\r\n". */
#define S3H_CHUNK_HEADER_MAX 104
int s3h_chunk_header_text(uint64_t chunk_len, const uint32_t sig[8], char *out, uint64_t out_len);
/* The chunk geometry of parts of `lengths` at chunk_bytes >= 1, without a device (pure host
 * arithmetic, the rule the plans and the batch calls apply): per part its data chunks,
 * ceil(length / chunk_bytes), and the index of its first signature in a part-major signatures
 * array (n entries each), and for the batch the data chunks, the signatures (data chunks + n) and
 * the longest part's data chunks.  Any output may be null.  S3H_EINVAL for chunk_bytes == 0,
 * n == 0 or more than 2^31 parts or data chunks. */
int s3h_chunk_geometry(const uint64_t *lengths, uint64_t n, uint64_t chunk_bytes,
                       uint64_t *data_chunks_per_part, uint64_t *signature_offsets,
                       uint64_t *data_chunks, uint64_t *signatures, uint64_t *max_chunks_per_part);
/* Device-resident parts (offsets relative to a base pointer, as s3h_plan_create) cut into chunks
 * of chunk_bytes >= 1: an S3H_ALGO_SHA256 plan over the chunks (S3H_KERNEL_AUTO) plus each part's
 * chain record.  At most 2^31 data chunks in all; a batch without one (every part empty) is
 * valid.  The plan owns the chunk digests: launch one plan on ONE stream at a time. */
int s3h_chunk_plan_create(int device, const uint64_t *offsets, const uint64_t *lengths, uint64_t n,
                          uint64_t chunk_bytes, s3h_chunk_plan_t *out);
/* Asynchronous on `stream`: the chunk-hash launch, then the chain kernel.  d_seeds (n x 8 words)
 * and d_signatures (signatures x 8 words, s3h_chunk_plan_info) are device pointers, 16-byte
 * aligned; nothing behind the last signature is written.  The context is read during the call
 * only.  As for s3h_plan_launch, call s3h_chunk_plan_status before using the signatures. */
int s3h_chunk_plan_launch(s3h_chunk_plan_t plan, s3h_chunk_sign_ctx_t ctx, const void *d_base,
                          const uint32_t *d_seeds, uint32_t *d_signatures, void *stream);
/* The chain kernel alone, over data-chunk digests already on the device (d_chunk_digests: data
 * chunks x 8 words, part-major in the plan's geometry, 16-byte aligned; may be null for a plan
 * without a data chunk) -- for a caller that hashed the chunks itself.  Asynchronous on `stream`;
 * it does not touch the plan's own digests, so it may run beside a launch of the plan. */
int s3h_chunk_plan_chain(s3h_chunk_plan_t plan, s3h_chunk_sign_ctx_t ctx,
                         const uint32_t *d_chunk_digests, const uint32_t *d_seeds,
                         uint32_t *d_signatures, void *stream);
/* s3h_plan_status of the chunk-hash plan (waits for `stream`): S3H_OK means the chunk digests,
 * and so the signatures, of every launch since the last call were produced. */
int s3h_chunk_plan_status(s3h_chunk_plan_t plan, void *stream);
/* n parts, data chunks and signatures in all, the longest chain's data chunks, and the name of
 * the chunk-hash kernel ("lane", "skew", ...; "none" without a data chunk) into kernel_name
 * (NUL-terminated, truncated to len).  Any pointer may be null. */
int s3h_chunk_plan_info(s3h_chunk_plan_t plan, uint64_t *n, uint64_t *data_chunks,
                        uint64_t *signatures, uint64_t *max_chunks_per_part, char *kernel_name,
                        int len);
int s3h_chunk_plan_destroy(s3h_chunk_plan_t plan);
/* One-shot, blocking: plan + launch + status + copy back.  d_base is a device pointer; seeds_host
 * (n x 8 words) and signatures_host (sum(ceil(lengths[p] / chunk_bytes) + 1) x 8 words) are host
 * memory. */
int s3h_chunk_sign_batch_device(int device, s3h_chunk_sign_ctx_t ctx, const void *d_base,
                                const uint64_t *offsets, const uint64_t *lengths, uint64_t n,
                                uint64_t chunk_bytes, const uint32_t *seeds_host,
                                uint32_t *signatures_host);
/* Host-resident parts: the chunks go through s3h_sha256_batch_host as its parts (all visible
 * devices, automatic slices), then the chain runs on the CPU.  Blocking. */
int s3h_chunk_sign_batch_host(s3h_chunk_sign_ctx_t ctx, const uint8_t *const *parts,
                              const uint64_t *lengths, uint64_t n, uint64_t chunk_bytes,
                              const uint32_t *seeds, uint32_t *signatures);

/* ---------------------------------------------------------------- SigV4 trailer signatures
 * x-amz-content-sha256: STREAMING-AWS4-HMAC-SHA256-PAYLOAD-TRAILER, the form current SDKs send:
 * the chunk-signed body above (the chunk strings keep AWS4-HMAC-SHA256-PAYLOAD; only the seed,
 * signed over other headers, differs), closed by one trailing checksum header and a signature
 * over it.  With sig_last the signature of the part's final 0-byte chunk:
 *   line        = name ":" base64(value) "\n"         e.g. "x-amz-checksum-crc32c:sOO8/Q==\n"
 *   trailer_sig = HMAC-SHA256(signing_key, "AWS4-HMAC-SHA256-TRAILER\n" timestamp "\n"
 *                   date "/" region "/" service "/aws4_request\n" hex(sig_last) "\n"
 *                   hex(sha256(line)))
 * `value` is the checksum's big-endian bytes: 4 (CRC-32C, CRC-32), 8 (CRC-64/NVME), 20 (SHA-1)
 * or 32 (SHA-256); the hashed line ends in "\n" (not "\r\n", which is only the framing).  Value
 * arrays have the layouts the library returns elsewhere: one uint32_t per part for the 32-bit
 * CRCs, one uint64_t for CRC-64/NVME, 5 or 8 words per part for the digests; trailer signatures
 * are 8 words per part like every signature.  A CRC plan cuts a part into segments as the chunk
 * plan cuts it into chunks, so neither half is a serial chain per part and one large part still
 * fills the GPU.  The digest checksums are accepted by the CPU functions and the host-resident
 * entry point only: a part's SHA-1 or SHA-256 is a whole-part chain, which is what chunk signing
 * exists to avoid, so the device entry points return S3H_EINVAL for them.
 * The framing s3h_chunk_trailer_text writes follows the AWS documentation; the tests pin it, as
 * part of whole bodies, against an independent decoder (the section after this one), but no real
 * server has seen it (the tests' mock endpoint does not decode aws-chunked bodies).
 * Added within API version 2. */
enum s3h_trailer_checksum {
  S3H_TRAILER_CRC32C = 0,
  S3H_TRAILER_CRC32 = 1,
  S3H_TRAILER_CRC64NVME = 2,
  S3H_TRAILER_SHA1 = 3,
  S3H_TRAILER_SHA256 = 4
};
/* The trailer link on the CPU, from the context's midstates: values (n entries in the kind's
 * layout), last_signatures (n x 8 words: each part's last chunk signature, gathered) ->
 * trailer_signatures (n x 8 words).  Every kind.  Parts are spread over the host threads. */
int s3h_cpu_trailer_signatures(s3h_chunk_sign_ctx_t ctx, int checksum, const void *values,
                               const uint32_t *last_signatures, uint64_t n,
                               uint32_t *trailer_signatures);
/* "name:base64" of one value (no line end), NUL-terminated, out_len >= S3H_TRAILER_LINE_MAX. */
#define S3H_TRAILER_LINE_MAX 80
int s3h_trailer_line_text(int checksum, const void *value, char *out, uint64_t out_len);
/* What an uploader writes after the "0;chunk-signature=...\r\n" line of s3h_chunk_header_text:
 *   name:base64\r\n
 *   x-amz-trailer-signature:<64 hex>\r\n
 *   \r\n
 * NUL-terminated, out_len >= S3H_CHUNK_TRAILER_MAX. */
#define S3H_CHUNK_TRAILER_MAX 192
int s3h_chunk_trailer_text(int checksum, const void *value, const uint32_t trailer_sig[8],
                           char *out, uint64_t out_len);
/* s3h_chunk_plan_create plus a CRC plan over the whole parts (s3h_crc_plan_* or
 * s3h_crc64nvme_plan_*, owned by the chunk plan).  checksum: S3H_TRAILER_CRC32C, _CRC32 or
 * _CRC64NVME (the digests: S3H_EINVAL, above).  The plan serves every s3h_chunk_plan_* call. */
int s3h_chunk_plan_create_trailer(int device, int checksum, const uint64_t *offsets,
                                  const uint64_t *lengths, uint64_t n, uint64_t chunk_bytes,
                                  s3h_chunk_plan_t *out);
/* Asynchronous on `stream`, in stream order with no host work between: the chunk hashes, the
 * chain, the CRC launch, the trailer kernel.  d_seeds and d_signatures as for
 * s3h_chunk_plan_launch; d_checksums receives n values (4-byte aligned words, or 8-byte aligned
 * 64-bit words for CRC-64/NVME: the uploader needs them for the trailer text; an empty part
 * gives 0); d_trailer_signatures n x 8 words, 16-byte aligned.  Nothing behind the last entry of
 * an output is written.  S3H_EINVAL for a plan made by s3h_chunk_plan_create. */
int s3h_chunk_plan_launch_trailer(s3h_chunk_plan_t plan, s3h_chunk_sign_ctx_t ctx,
                                  const void *d_base, const uint32_t *d_seeds,
                                  uint32_t *d_signatures, void *d_checksums,
                                  uint32_t *d_trailer_signatures, void *stream);
/* The trailer kernel alone, over chunk signatures (the plan's geometry) and checksum values
 * already on the device: the counterpart of s3h_chunk_plan_chain.  Asynchronous on `stream`. */
int s3h_chunk_plan_trailer(s3h_chunk_plan_t plan, s3h_chunk_sign_ctx_t ctx,
                           const uint32_t *d_signatures, const void *d_checksums,
                           uint32_t *d_trailer_signatures, void *stream);
/* The plan's checksum kind (enum s3h_trailer_checksum), or -1 for a plan without a trailer. */
int s3h_chunk_plan_trailer_info(s3h_chunk_plan_t plan, int *checksum);
/* One-shot, blocking: plan + launch + status + copy back.  d_base is a device pointer; seeds_host,
 * signatures_host (as s3h_chunk_sign_batch_device), checksums_host (n values) and
 * trailer_signatures_host (n x 8 words) are host memory. */
int s3h_chunk_sign_trailer_batch_device(int device, s3h_chunk_sign_ctx_t ctx, int checksum,
                                        const void *d_base, const uint64_t *offsets,
                                        const uint64_t *lengths, uint64_t n, uint64_t chunk_bytes,
                                        const uint32_t *seeds_host, uint32_t *signatures_host,
                                        void *checksums_host, uint32_t *trailer_signatures_host);
/* Host-resident parts.  CRC kinds: the chunks go once through s3h_sha256_crc_batch_host /
 * s3h_sha256_crc64nvme_batch_host as its parts, each part's chunk CRCs are folded
 * (s3h_crc_object / s3h_crc64nvme_object: no second read of the data), then the chain and the
 * trailer link run on the CPU.  Digest kinds: the chunks through s3h_sha256_batch_host and the
 * whole parts through s3h_sha1_batch_host / s3h_sha256_batch_host.  Blocking. */
int s3h_chunk_sign_trailer_batch_host(s3h_chunk_sign_ctx_t ctx, int checksum,
                                      const uint8_t *const *parts, const uint64_t *lengths,
                                      uint64_t n, uint64_t chunk_bytes, const uint32_t *seeds,
                                      uint32_t *signatures, void *checksums,
                                      uint32_t *trailer_signatures);

/* ---------------------------------------------------------------- aws-chunked bodies
 * The bytes an uploader sends for a chunk-signed part, from the signatures of the two sections
 * above.  For a part of L bytes at chunk_bytes c: floor(L / c) chunks of c bytes and one of
 * L mod c bytes if that is not zero, each framed as s3h_chunk_header_text frames it,
 *   hex(k) ";chunk-signature=" <64 hex> "\r\n" <k bytes> "\r\n"        hexlen(k) + 85 + k bytes
 * then the line of the final chunk, "0;chunk-signature=" <64 hex> "\r\n" (84 bytes), then "\r\n",
 * or with a trailing checksum the text of s3h_chunk_trailer_text (name ":" base64 + 94 bytes).
 * Chunk i of part p carries signature row signature_offsets[p] + i (s3h_chunk_geometry), the
 * final line the part's last row.  The body's length is the request's Content-Length, the
 * part's own length its x-amz-decoded-content-length.  The AWS documentation's example (66,560
 * bytes at 65,536-byte chunks) gives 66,824 bytes, 66,946 with a CRC-32C trailer.
 * Added within API version 2. */
/* Pure host arithmetic, no device.  checksum: -1 (no trailer) or any enum s3h_trailer_checksum.
 * body_lengths[p]: the wire length of part p's body; body_offsets[p]: where it starts when the
 * bodies are packed back to back; *total: their sum.  Any output may be null.  Errors as
 * s3h_chunk_geometry, and S3H_EINVAL for an unknown checksum. */
int s3h_chunk_body_geometry(const uint64_t *lengths, uint64_t n, uint64_t chunk_bytes,
                            int checksum, uint64_t *body_lengths, uint64_t *body_offsets,
                            uint64_t *total);
/* Host-resident parts: part p's body at body + body_offsets[p] (null: packed, as
 * s3h_chunk_body_geometry packs them), exactly its bytes and nothing else.  signatures as
 * s3h_cpu_chunk_signatures returns them.  checksum -1: values and trailer_signatures null; any
 * enum s3h_trailer_checksum: values (n entries in the kind's layout) and trailer_signatures
 * (n x 8 words), both needed.  parts[p] may be null for an empty part.  Parts are spread over
 * the host threads. */
int s3h_cpu_chunk_body(const uint8_t *const *parts, const uint64_t *lengths, uint64_t n,
                       uint64_t chunk_bytes, const uint32_t *signatures, int checksum,
                       const void *values, const uint32_t *trailer_signatures, uint8_t *body,
                       const uint64_t *body_offsets);
/* Device-resident parts of a chunk plan, asynchronous on `stream`: part p's body at
 * d_body + body_offsets[p] (a host array of n byte offsets, any values, reusable on return;
 * null: packed).  d_body needs no alignment.  d_signatures as s3h_chunk_plan_launch wrote them;
 * a trailer plan writes the trailer form and needs d_checksums and d_trailer_signatures as
 * s3h_chunk_plan_launch_trailer wrote them, a plain plan needs both null.  Queued behind those
 * launches on the same stream it needs no host synchronisation in between.  The kernel reads the
 * parts and the three inputs and writes every byte of every body once, nothing else.
 * S3H_EINVAL, with nothing started: two bodies overlap, the bodies' extent intersects the
 * parts' (d_base + their offsets), a pointer is null where one is needed or given where none is,
 * d_signatures is not 4-byte aligned or d_checksums not aligned to its values. */
int s3h_chunk_plan_body(s3h_chunk_plan_t plan, const void *d_base, const uint32_t *d_signatures,
                        const void *d_checksums, const uint32_t *d_trailer_signatures,
                        void *d_body, const uint64_t *body_offsets, void *stream);
/* The plan's body lengths (n entries) and their sum, and the body kernel's shape: its work items
 * (one wave each: the pieces of the data chunks and one per part), the most bytes of one chunk
 * that one item copies, and its grid (workgroups).  Any output may be null. */
int s3h_chunk_plan_body_info(s3h_chunk_plan_t plan, uint64_t *body_lengths, uint64_t *total,
                             uint64_t *items, uint64_t *piece_bytes, uint64_t *grid);
/* One-shot, blocking: plan + launch (checksum -1) or trailer launch (a CRC kind) + body + status
 * + copy back.  body_host receives part p's body at body_offsets[p] (null: packed; the packed
 * bodies come back in one copy).  S3H_ENOMEM when the device buffer for the bodies cannot be
 * allocated. */
int s3h_chunk_body_batch_device(int device, s3h_chunk_sign_ctx_t ctx, int checksum,
                                const void *d_base, const uint64_t *offsets,
                                const uint64_t *lengths, uint64_t n, uint64_t chunk_bytes,
                                const uint32_t *seeds_host, uint8_t *body_host,
                                const uint64_t *body_offsets);

/* ---------------------------------------------------------------- synthetic inputs
 * Fill part i (at d_base + offsets[i], 8-B aligned, lengths[i] bytes) with generator
 * G(seed, part_ids[i], lengths[i]) of SURVEY.md 8(d).  Asynchronous on `stream`. */
int s3h_generate_parts(int device, void *d_base, const uint64_t *offsets,
                       const uint64_t *lengths, const uint64_t *part_ids, uint64_t n,
                       uint64_t seed, void *stream);

/* ---------------------------------------------------------------- CPU drop-in (C view)
 * C entry points of the lib/hash drop-in that the same library exports in C++ form
 * (namespace sha256, include/sha256.h).  Single messages: CPU, never the GPU. */
void s3h_cpu_sha256(const uint8_t *data, uint64_t length, uint32_t hash[8]);
void s3h_cpu_hmac256(const uint8_t *data, uint64_t length, const uint8_t *key,
                     uint64_t key_length, uint8_t mac[32]);
/* MD5 drop-in (md5::md5, include/md5.h): hash[0..3], digest bytes = words in LE order. */
void s3h_cpu_md5(const uint8_t *data, uint64_t length, uint32_t hash[4]);
/* S3 multipart ETag of an object from its parts' MD5 digests (n x 4 words, as the MD5 batch
 * entry points return them, in part order): lowercase hex of MD5(the n 16-byte digests
 * concatenated) + "-" + n, NUL-terminated, into out (out_len >= S3H_ETAG_MAX).  This is the
 * ETag CompleteMultipartUpload returns (lib/src/api/multipart_upload.cpp:162-183); an
 * uploader compares it with the server's.  CPU (16 B per part).  S3H_EINVAL for n == 0. */
#define S3H_ETAG_MAX 56
int s3h_multipart_etag(const uint32_t *md5_digests, uint64_t n, char *out, uint64_t out_len);
/* lowercase hex of the 32 digest bytes + NUL (sha256::hash_to_text). */
void s3h_hash_to_text(const uint32_t hash[8], char text[65]);
/* "sha-ni" or "scalar": which compression the CPU drop-in dispatched to. */
const char *s3h_cpu_backend(void);

#ifdef __cplusplus
}
#endif
#endif /* S3HASH_H */
