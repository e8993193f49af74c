"""ctypes binding of libs3hash.so (the C-ABI declared in include/s3hash.h).

The library is built in-tree (``make`` at the repo root, or ``__graft_entry__.build()``) to
``s3client_amd/lib/libs3hash.so``.  There is no fallback: if the library is missing, every
entry point raises, and the batched GPU entry points raise when no HIP device is visible.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libs3hash.so")
# Kernel experiments only (`make exp` builds variants under tools/exp/): S3H_LIBRARY points the
# Python layer at one of them.  Unset in every test, smoke and default bench run.
LIB_PATH = os.environ.get("S3H_LIBRARY", LIB_PATH)

S3H_OK, S3H_EINVAL, S3H_ENODEV, S3H_EHIP, S3H_ENOMEM = 0, -1, -2, -3, -4
KERNEL_AUTO, KERNEL_LANE, KERNEL_PC, KERNEL_PAIR, KERNEL_QUAD, KERNEL_SKEW, KERNEL_SKEWP = 0, 1, 2, 3, 4, 5, 6
KERNEL_SKEWS = 7
KERNEL_NAMES = {KERNEL_AUTO: "auto", KERNEL_LANE: "lane", KERNEL_PC: "pc", KERNEL_PAIR: "pair",
                KERNEL_QUAD: "quad", KERNEL_SKEW: "skew", KERNEL_SKEWP: "skewp", KERNEL_SKEWS: "skews"}
KERNEL_IDS = {v: k for k, v in KERNEL_NAMES.items()}

# every symbol include/s3hash.h declares (tests check the library exports all of them)
C_ABI_SYMBOLS = (
    "s3h_last_error", "s3h_api_version", "s3h_device_count",
    "s3h_plan_create", "s3h_plan_destroy", "s3h_plan_launch", "s3h_plan_launch_range",
    "s3h_plan_info", "s3h_sha256_batch_device", "s3h_sha256_batch_host",
    "s3h_generate_parts", "s3h_cpu_sha256", "s3h_cpu_hmac256", "s3h_hash_to_text",
    "s3h_cpu_backend", "s3h_cpu_md5", "s3h_plan_create_ex", "s3h_plan_algo",
    "s3h_md5_batch_device", "s3h_md5_batch_host", "s3h_verify_batch_device",
    "s3h_verify_batch_host", "s3h_stream_create", "s3h_stream_update_device",
    "s3h_stream_final_device", "s3h_stream_update_host", "s3h_stream_final_host",
    "s3h_stream_total", "s3h_stream_destroy", "s3h_plan_set_clock_probe",
    "s3h_sha256_md5_batch_host", "s3h_sha256_md5_batch_device", "s3h_trim",
    "s3h_sha256_file_parts", "s3h_sha256_batch_host_on", "s3h_plan_groups",
    "s3h_sha256_md5_file_parts", "s3h_plan_status", "s3h_stream_status", "s3h_host_threads",
    "s3h_plan_dual_solo", "s3h_device_pci_bus_id", "s3h_multipart_etag",
    "s3h_route_model", "s3h_route_estimate", "s3h_sha256_batch_routed",
    "s3h_sha256_file_parts_routed", "s3h_pci_numa", "s3h_device_numa_node", "s3h_host_numa",
    "s3h_host_numa_info", "s3h_host_alloc", "s3h_host_free", "s3h_mem_node",
    "s3h_route_estimate_ex", "s3h_kernel_policy", "s3h_stream_stats", "s3h_plan_dual_layout",
    "s3h_dual_layout", "s3h_route_split_estimate", "s3h_verify_batch_routed",
    # round 6: digest-set routing, adaptive model, host thread plan, strict pinned allocation
    "s3h_route_rates", "s3h_route_choose", "s3h_route_device_rates", "s3h_route_refresh_calls",
    "s3h_route_scale", "s3h_md5_batch_routed", "s3h_sha256_md5_batch_routed",
    "s3h_sha256_md5_file_parts_routed", "s3h_md5_file_parts", "s3h_host_plan",
    "s3h_host_alloc_ex", "s3h_device_power_cap", "s3h_pci_power_cap",
    # CRC-32C / CRC-32 checksums (added within API version 2)
    "s3h_crc_plan_create", "s3h_crc_plan_launch", "s3h_crc_plan_info", "s3h_crc_plan_destroy",
    "s3h_crc_batch_device", "s3h_crc_verify_batch_device", "s3h_cpu_crc", "s3h_crc_combine",
    "s3h_crc_object", "s3h_checksum_text",
    # ranged CRC launches, SHA-256 + CRC of host-resident parts in one pass
    "s3h_crc_plan_launch_range", "s3h_crc_batch_host", "s3h_sha256_crc_batch_host",
    "s3h_sha256_crc_file_parts",
    # CRC-64/NVME
    "s3h_crc64nvme_plan_create", "s3h_crc64nvme_plan_launch", "s3h_crc64nvme_plan_launch_range",
    "s3h_crc64nvme_plan_info", "s3h_crc64nvme_plan_destroy", "s3h_crc64nvme_batch_device",
    "s3h_crc64nvme_verify_batch_device", "s3h_cpu_crc64nvme", "s3h_crc64nvme_combine",
    "s3h_crc64nvme_object", "s3h_checksum64_text", "s3h_crc64nvme_batch_host",
    "s3h_sha256_crc64nvme_batch_host", "s3h_sha256_crc64nvme_file_parts",
    # SHA-1
    "s3h_sha1_batch_device", "s3h_sha1_batch_host", "s3h_sha1_file_parts",
    "s3h_sha256_sha1_batch_host", "s3h_sha256_sha1_file_parts", "s3h_cpu_sha1",
    "s3h_digest_checksum_text",
    # SigV4 chunk-signed uploads
    "s3h_sigv4_signing_key", "s3h_chunk_sign_ctx_create", "s3h_chunk_sign_ctx_destroy",
    "s3h_cpu_chunk_signatures", "s3h_chunk_header_text", "s3h_chunk_geometry",
    "s3h_chunk_plan_create", "s3h_chunk_plan_launch", "s3h_chunk_plan_chain", "s3h_chunk_plan_status",
    "s3h_chunk_plan_info", "s3h_chunk_plan_destroy", "s3h_chunk_sign_batch_device",
    "s3h_chunk_sign_batch_host",
    # SigV4 trailer signatures (chunk-signed uploads with a trailing checksum header)
    "s3h_cpu_trailer_signatures", "s3h_trailer_line_text", "s3h_chunk_trailer_text",
    "s3h_chunk_plan_create_trailer", "s3h_chunk_plan_launch_trailer", "s3h_chunk_plan_trailer",
    "s3h_chunk_plan_trailer_info", "s3h_chunk_sign_trailer_batch_device",
    "s3h_chunk_sign_trailer_batch_host",
    # aws-chunked bodies
    "s3h_chunk_body_geometry", "s3h_cpu_chunk_body", "s3h_chunk_plan_body", "s3h_chunk_plan_body_info",
    "s3h_chunk_body_batch_device",
)
# enum s3h_trailer_checksum, and the numpy layout of one value of each kind
TRAILER_IDS = {"crc32c": 0, "crc32": 1, "crc64nvme": 2, "sha1": 3, "sha256": 4}
TRAILER_VALUE = {0: ("<u4", 1), 1: ("<u4", 1), 2: ("<u8", 1), 3: ("<u4", 5), 4: ("<u4", 8)}
TRAILER_LINE_MAX = 80
CHUNK_TRAILER_MAX = 192
CRC32C, CRC32 = 0, 1
CRC64NVME = "crc64nvme"  # not an enum s3h_crc: the checksum has entry points of its own
CRC_IDS = {"crc32c": CRC32C, "crc32": CRC32}
CHECKSUM_MAX = 32
DIGEST_CHECKSUM_MAX = 64
CHUNK_HEADER_MAX = 104
POLICY_IDS = {"throughput": 0, "efficiency": 1, "power": 2}
POLICY_NAMES = {v: k for k, v in POLICY_IDS.items()}
SOURCE_IDS = {"pinned": 0, "pageable": 1, "file": 2}
NUMA_LOCAL, NUMA_OFF = -1, -2
ROUTE_GPU, ROUTE_CPU, ROUTE_AUTO, ROUTE_SPLIT = 0, 1, 2, 3
ROUTE_IDS = {"gpu": ROUTE_GPU, "cpu": ROUTE_CPU, "auto": ROUTE_AUTO, "split": ROUTE_SPLIT}
ROUTE_NAMES = {v: k for k, v in ROUTE_IDS.items()}


class RouteModel(ctypes.Structure):
    """s3h_route_model_t (include/s3hash.h)."""
    _fields_ = [("cpu_bytes_per_s", ctypes.c_double), ("chain_bytes_per_s", ctypes.c_double),
                ("h2d_bytes_per_s", ctypes.c_double), ("call_s", ctypes.c_double),
                ("cpu_threads", ctypes.c_int), ("devices", ctypes.c_int),
                ("cpu_all_bytes_per_s", ctypes.c_double), ("staged_bytes_per_s", ctypes.c_double)]


DIGESTS_SHA256, DIGESTS_MD5, DIGESTS_BOTH = 1, 2, 3
DIGESTS_IDS = {"sha256": DIGESTS_SHA256, "md5": DIGESTS_MD5, "both": DIGESTS_BOTH}
RATE_IDS = {"chain": 0, "h2d": 1, "cpu": 2, "staged": 3}
HOST_ALLOC_STRICT = 1


class RouteRates(ctypes.Structure):
    """s3h_route_rates_t (include/s3hash.h): size-carrying, every digest set."""
    _fields_ = [("size", ctypes.c_uint32), ("version", ctypes.c_uint32),
                ("cpu_threads", ctypes.c_int), ("devices", ctypes.c_int),
                ("cpu_bytes_per_s", ctypes.c_double * 3),
                ("cpu_all_bytes_per_s", ctypes.c_double * 3),
                ("chain_bytes_per_s", ctypes.c_double * 3),
                ("h2d_bytes_per_s", ctypes.c_double), ("staged_bytes_per_s", ctypes.c_double),
                ("call_s", ctypes.c_double), ("gpu_factor", ctypes.c_double * 3),
                ("cpu_factor", ctypes.c_double * 3), ("measurements", ctypes.c_uint64),
                ("routed_calls", ctypes.c_uint64), ("divergences", ctypes.c_uint64),
                ("age_s", ctypes.c_double), ("staged_file_bytes_per_s", ctypes.c_double)]


class RouteChoice(ctypes.Structure):
    """s3h_route_choice_t (include/s3hash.h)."""
    _fields_ = [("route", ctypes.c_int), ("stage_threads", ctypes.c_int),
                ("cpu_parts", ctypes.c_uint64), ("gpu_s", ctypes.c_double),
                ("cpu_s", ctypes.c_double), ("split_s", ctypes.c_double)]


class HostPlan(ctypes.Structure):
    """s3h_host_plan_t (include/s3hash.h)."""
    _fields_ = [("cpus", ctypes.c_int), ("affinity_cpus", ctypes.c_int),
                ("cpu_quota", ctypes.c_double), ("devices", ctypes.c_int),
                ("staging_threads_per_device", ctypes.c_int), ("threads", ctypes.c_int),
                ("oversubscribed", ctypes.c_int), ("below_saturation", ctypes.c_int),
                ("node_oversubscribed", ctypes.c_int), ("split_cpu_threads_pinned", ctypes.c_int),
                ("split_candidates", ctypes.c_int), ("split_stage_min", ctypes.c_int),
                ("split_stage_max", ctypes.c_int), ("split_cpu_threads_min", ctypes.c_int),
                ("split_cpu_threads_max", ctypes.c_int)]


class HostPlanDevice(ctypes.Structure):
    """s3h_host_plan_device_t (include/s3hash.h)."""
    _fields_ = [("node", ctypes.c_int), ("bind_node", ctypes.c_int), ("bind_cpus", ctypes.c_int),
                ("bind_first_cpu", ctypes.c_int), ("bind_last_cpu", ctypes.c_int),
                ("staging_threads", ctypes.c_int)]


class HostNuma(ctypes.Structure):
    """s3h_host_numa_t (include/s3hash.h)."""
    _fields_ = [("device_node", ctypes.c_int), ("target_node", ctypes.c_int),
                ("bound_cpus", ctypes.c_int), ("staging_node", ctypes.c_int),
                ("threads_node", ctypes.c_int), ("copy_threads", ctypes.c_int)]


ALGO_SHA256, ALGO_MD5, ALGO_SHA1 = 0, 1, 2
ALGO_IDS = {"sha256": ALGO_SHA256, "md5": ALGO_MD5, "sha1": ALGO_SHA1}
DIGEST_WORDS = {ALGO_SHA256: 8, ALGO_MD5: 4, ALGO_SHA1: 5}
# the lib/hash drop-in (C++ mangled names identical to the reference's libs3client.a)
CXX_DROPIN_SYMBOLS = (
    "_ZN6sha2566sha256EPKhmPj",          # sha256::sha256(const uint8_t*, size_t, uint32_t*)
    "_ZN6sha25613sha256_streamEPjPKhm",  # sha256::sha256_stream(uint32_t*, const uint8_t*, uint64_t)
    "_ZN6sha25611sha256_nextEPKhjPjmPh", # sha256::sha256_next(...)
    "_ZN6sha25610print_hashEPj",         # sha256::print_hash(uint32_t*)
    "_ZN6sha25611sha256_fileEPKcPj",     # sha256::sha256_file(const char*, uint32_t*)
    "_Z7hmac256PKhmS0_mPh",              # hmac256(...)
    "_Z12alloc_paddedmmPmPh",            # alloc_padded(...)
    "_ZN3md510md5_streamEPjPKhm",        # md5::md5_stream(uint32_t*, const uint8_t*, uint64_t)
    "_ZN3md53md5EPKhmPj",                # md5::md5(const uint8_t*, size_t, uint32_t*)
    "_ZN3md510print_hashEPj",            # md5::print_hash(uint32_t*)
    "_ZN3md58md5_fileEPKcPj",            # md5::md5_file(const char*, uint32_t*)
)


class S3HashError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"s3hash error {code}: {msg}")
        self.code = code


_lib = None
_lock = threading.Lock()

u64p = ctypes.POINTER(ctypes.c_uint64)
u32p = ctypes.POINTER(ctypes.c_uint32)


def lib() -> ctypes.CDLL:
    """Load libs3hash.so once; raise loudly if it has not been built."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise S3HashError(S3H_EINVAL, f"{LIB_PATH} missing: run `make` (or "
                                  "__graft_entry__.build()) -- there is no fallback path")
            # One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64 and
            # libhsa-runtime64 (SONAME libamdhip64.so.7, like /opt/rocm's), but torch's own
            # libraries NEED the unversioned names: loaded AFTER this library, torch maps a
            # second HIP + ROCr instance and this library's runtime loses the device ("no HIP
            # device visible" on its first GPU call after torch.cuda.init(); tools/
            # cpu_route_context_probe.py on the box).  With torch loaded first this library's
            # NEEDED libamdhip64.so.7 resolves to torch's runtime by SONAME.
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
            L = ctypes.CDLL(LIB_PATH)
            L.s3h_last_error.restype = ctypes.c_char_p
            L.s3h_device_count.argtypes = [ctypes.POINTER(ctypes.c_int)]
            L.s3h_device_pci_bus_id.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
            L.s3h_pci_numa.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int),
                                       ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
            L.s3h_device_numa_node.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                               ctypes.c_char_p, ctypes.c_int]
            L.s3h_host_numa.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
            L.s3h_host_numa_info.argtypes = [ctypes.c_int, ctypes.POINTER(HostNuma)]
            L.s3h_host_alloc.argtypes = [ctypes.c_int, ctypes.c_uint64,
                                         ctypes.POINTER(ctypes.c_void_p)]
            L.s3h_host_free.argtypes = [ctypes.c_void_p]
            L.s3h_kernel_policy.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
            L.s3h_device_power_cap.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
            L.s3h_pci_power_cap.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double)]
            L.s3h_stream_stats.argtypes = [ctypes.c_void_p, u64p, u64p]
            L.s3h_plan_dual_layout.argtypes = [ctypes.c_void_p, u32p, ctypes.POINTER(ctypes.c_int)]
            L.s3h_dual_layout.argtypes = [u64p, ctypes.c_uint64, ctypes.c_int, u32p,
                                          ctypes.POINTER(ctypes.c_int)]
            L.s3h_mem_node.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
            L.s3h_plan_create.argtypes = [ctypes.c_int, u64p, u64p, ctypes.c_uint64, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_void_p)]
            L.s3h_plan_create_ex.argtypes = [ctypes.c_int, ctypes.c_int, u64p, u64p,
                                             ctypes.c_uint64, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_void_p)]
            L.s3h_plan_algo.argtypes = [ctypes.c_void_p]
            L.s3h_plan_destroy.argtypes = [ctypes.c_void_p]
            L.s3h_plan_launch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p]
            L.s3h_plan_launch_range.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                                ctypes.c_void_p]
            L.s3h_plan_status.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            L.s3h_stream_status.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            L.s3h_host_threads.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
            L.s3h_plan_set_clock_probe.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.POINTER(ctypes.c_uint32)]
            L.s3h_plan_info.argtypes = [ctypes.c_void_p, u64p, u64p, u64p,
                                        ctypes.POINTER(ctypes.c_int), u32p]
            L.s3h_plan_groups.argtypes = [ctypes.c_void_p, u32p, u32p]
            L.s3h_plan_dual_solo.argtypes = [ctypes.c_void_p, u32p]
            L.s3h_sha256_batch_device.argtypes = [ctypes.c_int, ctypes.c_void_p, u64p, u64p,
                                                  ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
            for name in ("s3h_sha256_batch_host", "s3h_md5_batch_host", "s3h_sha1_batch_host"):
                getattr(L, name).argtypes = [ctypes.POINTER(ctypes.c_void_p), u64p,
                                             ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_uint64]
            L.s3h_sha256_batch_host_on.argtypes = [ctypes.POINTER(ctypes.c_void_p), u64p,
                                                   ctypes.c_uint64, ctypes.c_void_p,
                                                   ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                                   ctypes.c_uint64]
            L.s3h_sha256_file_parts.argtypes = [ctypes.c_char_p, u64p, u64p, ctypes.c_uint64,
                                                ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64]
            L.s3h_sha256_md5_file_parts.argtypes = [ctypes.c_char_p, u64p, u64p, ctypes.c_uint64,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                    ctypes.c_uint64]
            L.s3h_sha256_md5_batch_host.argtypes = [ctypes.POINTER(ctypes.c_void_p), u64p,
                                                    ctypes.c_uint64, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_int,
                                                    ctypes.c_uint64]
            L.s3h_sha256_md5_batch_device.argtypes = [ctypes.c_int, ctypes.c_void_p, u64p, u64p,
                                                      ctypes.c_uint64, ctypes.c_void_p,
                                                      ctypes.c_void_p, ctypes.c_void_p]
            L.s3h_verify_batch_host.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), u64p,
                                                ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                                u64p, ctypes.c_int]
            L.s3h_verify_batch_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, u64p,
                                                  u64p, ctypes.c_uint64, ctypes.c_void_p,
                                                  ctypes.c_void_p, u64p, ctypes.c_void_p]
            L.s3h_md5_batch_device.argtypes = [ctypes.c_int, ctypes.c_void_p, u64p, u64p,
                                               ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
            L.s3h_generate_parts.argtypes = [ctypes.c_int, ctypes.c_void_p, u64p, u64p, u64p,
                                             ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
            L.s3h_cpu_sha256.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
            L.s3h_cpu_sha256.restype = None
            L.s3h_cpu_hmac256.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                          ctypes.c_uint64, ctypes.c_void_p]
            L.s3h_cpu_hmac256.restype = None
            L.s3h_hash_to_text.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
            L.s3h_hash_to_text.restype = None
            L.s3h_cpu_backend.restype = ctypes.c_char_p
            L.s3h_cpu_md5.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
            L.s3h_cpu_md5.restype = None
            L.s3h_route_model.argtypes = [ctypes.POINTER(RouteModel)]
            L.s3h_route_estimate.argtypes = [ctypes.POINTER(RouteModel), u64p, ctypes.c_uint64,
                                             ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                             ctypes.POINTER(ctypes.c_double)]
            L.s3h_route_estimate_ex.argtypes = [ctypes.POINTER(RouteModel), u64p, ctypes.c_uint64,
                                                ctypes.c_int, ctypes.c_int,
                                                ctypes.POINTER(ctypes.c_double),
                                                ctypes.POINTER(ctypes.c_double)]
            L.s3h_route_split_estimate.argtypes = [ctypes.POINTER(RouteModel), u64p, ctypes.c_uint64,
                                                   ctypes.c_int, ctypes.c_int,
                                                   ctypes.POINTER(ctypes.c_uint64),
                                                   ctypes.POINTER(ctypes.c_int),
                                                   ctypes.POINTER(ctypes.c_double)]
            L.s3h_verify_batch_routed.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), u64p,
                                                  ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.POINTER(ctypes.c_uint64), ctypes.c_int,
                                                  ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
            L.s3h_sha256_batch_routed.argtypes = [ctypes.POINTER(ctypes.c_void_p), u64p,
                                                  ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                                  ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
            L.s3h_sha256_file_parts_routed.argtypes = [ctypes.c_char_p, u64p, u64p,
                                                       ctypes.c_uint64, ctypes.c_void_p,
                                                       ctypes.c_int, ctypes.c_int,
                                                       ctypes.POINTER(ctypes.c_int)]
            L.s3h_route_rates.argtypes = [ctypes.POINTER(RouteRates)]
            L.s3h_route_choose.argtypes = [ctypes.POINTER(RouteRates), ctypes.c_int, u64p,
                                           ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                           ctypes.POINTER(RouteChoice)]
            L.s3h_route_device_rates.argtypes = [ctypes.c_int, ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_double),
                                                 ctypes.POINTER(ctypes.c_double)]
            L.s3h_route_refresh_calls.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
            L.s3h_route_scale.argtypes = [ctypes.c_int, ctypes.c_double]
            L.s3h_md5_batch_routed.argtypes = L.s3h_sha256_batch_routed.argtypes
            L.s3h_sha256_md5_batch_routed.argtypes = [ctypes.POINTER(ctypes.c_void_p), u64p,
                                                      ctypes.c_uint64, ctypes.c_void_p,
                                                      ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                      ctypes.POINTER(ctypes.c_int)]
            L.s3h_sha256_md5_file_parts_routed.argtypes = [ctypes.c_char_p, u64p, u64p,
                                                           ctypes.c_uint64, ctypes.c_void_p,
                                                           ctypes.c_void_p, ctypes.c_int,
                                                           ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
            L.s3h_md5_file_parts.argtypes = L.s3h_sha256_file_parts.argtypes
            L.s3h_host_plan.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.c_int,
                                        ctypes.c_char_p, ctypes.c_double,
                                        ctypes.POINTER(HostPlan), ctypes.POINTER(HostPlanDevice)]
            L.s3h_host_alloc_ex.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_void_p)]
            L.s3h_multipart_etag.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p,
                                             ctypes.c_uint64]
            L.s3h_stream_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                            ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
            L.s3h_stream_update_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u64p, u64p,
                                                   ctypes.c_void_p]
            L.s3h_stream_final_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p]
            L.s3h_stream_update_host.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                                 u64p]
            L.s3h_stream_final_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            L.s3h_stream_total.argtypes = [ctypes.c_void_p, ctypes.c_uint64, u64p]
            L.s3h_stream_destroy.argtypes = [ctypes.c_void_p]
            L.s3h_crc_plan_create.argtypes = [ctypes.c_int, ctypes.c_int, u64p, u64p,
                                              ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]
            L.s3h_crc_plan_launch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p]
            L.s3h_crc_plan_info.argtypes = [ctypes.c_void_p, u64p, u64p, u64p, u32p]
            L.s3h_crc_plan_launch_range.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_uint64,
                                                    ctypes.c_uint64, ctypes.c_uint64,
                                                    ctypes.c_void_p]
            L.s3h_crc_batch_host.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), u64p,
                                             ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_uint64]
            L.s3h_sha256_crc_batch_host.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                                    u64p, ctypes.c_uint64, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64]
            L.s3h_sha256_crc_file_parts.argtypes = [ctypes.c_int, ctypes.c_char_p, u64p, u64p,
                                                    ctypes.c_uint64, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64]
            L.s3h_crc_plan_destroy.argtypes = [ctypes.c_void_p]
            L.s3h_crc64nvme_plan_create.argtypes = [ctypes.c_int, u64p, u64p, ctypes.c_uint64,
                                                    ctypes.POINTER(ctypes.c_void_p)]
            L.s3h_crc64nvme_plan_launch.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_void_p]
            L.s3h_crc64nvme_plan_launch_range.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                                          ctypes.c_void_p, ctypes.c_uint64,
                                                          ctypes.c_uint64, ctypes.c_uint64,
                                                          ctypes.c_void_p]
            L.s3h_crc64nvme_plan_info.argtypes = [ctypes.c_void_p, u64p, u64p, u64p, u32p]
            L.s3h_crc64nvme_plan_destroy.argtypes = [ctypes.c_void_p]
            L.s3h_crc64nvme_batch_device.argtypes = [ctypes.c_int, ctypes.c_void_p, u64p, u64p,
                                                     ctypes.c_uint64, ctypes.c_void_p,
                                                     ctypes.c_void_p]
            L.s3h_crc64nvme_verify_batch_device.argtypes = [ctypes.c_int, ctypes.c_void_p, u64p,
                                                            u64p, ctypes.c_uint64, ctypes.c_void_p,
                                                            ctypes.c_void_p, u64p, ctypes.c_void_p]
            L.s3h_crc64nvme_batch_host.argtypes = [ctypes.POINTER(ctypes.c_void_p), u64p,
                                                   ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                                   ctypes.c_uint64]
            L.s3h_sha256_crc64nvme_batch_host.argtypes = [ctypes.POINTER(ctypes.c_void_p), u64p,
                                                          ctypes.c_uint64, ctypes.c_void_p,
                                                          ctypes.c_void_p, ctypes.c_int,
                                                          ctypes.c_uint64]
            L.s3h_sha256_crc64nvme_file_parts.argtypes = [ctypes.c_char_p, u64p, u64p,
                                                          ctypes.c_uint64, ctypes.c_void_p,
                                                          ctypes.c_void_p, ctypes.c_int,
                                                          ctypes.c_uint64]
            L.s3h_cpu_crc64nvme.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
            L.s3h_cpu_crc64nvme.restype = ctypes.c_uint64
            L.s3h_crc64nvme_combine.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                                u64p]
            L.s3h_crc64nvme_object.argtypes = [ctypes.c_void_p, u64p, ctypes.c_uint64, u64p]
            L.s3h_checksum64_text.argtypes = [ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64]
            L.s3h_crc_batch_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, u64p,
                                               u64p, ctypes.c_uint64, ctypes.c_void_p,
                                               ctypes.c_void_p]
            L.s3h_crc_verify_batch_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                      u64p, u64p, ctypes.c_uint64, ctypes.c_void_p,
                                                      ctypes.c_void_p, u64p, ctypes.c_void_p]
            L.s3h_cpu_crc.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                      ctypes.c_uint32]
            L.s3h_cpu_crc.restype = ctypes.c_uint32
            L.s3h_crc_combine.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.c_uint64, u32p]
            L.s3h_crc_object.argtypes = [ctypes.c_int, ctypes.c_void_p, u64p, ctypes.c_uint64,
                                         u32p]
            L.s3h_checksum_text.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                            ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64]
            L.s3h_sha1_batch_device.argtypes = L.s3h_md5_batch_device.argtypes
            L.s3h_sha1_file_parts.argtypes = L.s3h_sha256_file_parts.argtypes
            L.s3h_sha256_sha1_batch_host.argtypes = L.s3h_sha256_md5_batch_host.argtypes
            L.s3h_sha256_sha1_file_parts.argtypes = L.s3h_sha256_md5_file_parts.argtypes
            L.s3h_cpu_sha1.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
            L.s3h_cpu_sha1.restype = None
            L.s3h_digest_checksum_text.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                                   ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64]
            L.s3h_sigv4_signing_key.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                                ctypes.c_char_p, ctypes.c_void_p]
            L.s3h_chunk_sign_ctx_create.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p,
                                                    ctypes.c_char_p, ctypes.c_char_p,
                                                    ctypes.POINTER(ctypes.c_void_p)]
            L.s3h_chunk_sign_ctx_destroy.argtypes = [ctypes.c_void_p]
            L.s3h_cpu_chunk_signatures.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u64p,
                                                   ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
            L.s3h_chunk_header_text.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_char_p,
                                                ctypes.c_uint64]
            L.s3h_chunk_geometry.argtypes = [u64p, ctypes.c_uint64, ctypes.c_uint64, u64p, u64p,
                                             u64p, u64p, u64p]
            L.s3h_chunk_plan_create.argtypes = [ctypes.c_int, u64p, u64p, ctypes.c_uint64,
                                                ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]
            L.s3h_chunk_plan_launch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
            L.s3h_chunk_plan_chain.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
            L.s3h_chunk_plan_status.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            L.s3h_chunk_plan_info.argtypes = [ctypes.c_void_p, u64p, u64p, u64p, u64p,
                                              ctypes.c_char_p, ctypes.c_int]
            L.s3h_chunk_plan_destroy.argtypes = [ctypes.c_void_p]
            L.s3h_chunk_sign_batch_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                      u64p, u64p, ctypes.c_uint64, ctypes.c_uint64,
                                                      ctypes.c_void_p, ctypes.c_void_p]
            L.s3h_chunk_sign_batch_host.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                                    u64p, ctypes.c_uint64, ctypes.c_uint64,
                                                    ctypes.c_void_p, ctypes.c_void_p]
            L.s3h_cpu_trailer_signatures.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
            L.s3h_trailer_line_text.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p,
                                                ctypes.c_uint64]
            L.s3h_chunk_trailer_text.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_char_p, ctypes.c_uint64]
            L.s3h_chunk_plan_create_trailer.argtypes = [ctypes.c_int, ctypes.c_int, u64p, u64p,
                                                        ctypes.c_uint64, ctypes.c_uint64,
                                                        ctypes.POINTER(ctypes.c_void_p)]
            L.s3h_chunk_plan_launch_trailer.argtypes = [ctypes.c_void_p] * 8
            L.s3h_chunk_plan_trailer.argtypes = [ctypes.c_void_p] * 6
            L.s3h_chunk_plan_trailer_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
            L.s3h_chunk_sign_trailer_batch_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                              ctypes.c_void_p, u64p, u64p,
                                                              ctypes.c_uint64, ctypes.c_uint64,
                                                              ctypes.c_void_p, ctypes.c_void_p,
                                                              ctypes.c_void_p, ctypes.c_void_p]
            L.s3h_chunk_sign_trailer_batch_host.argtypes = [ctypes.c_void_p, ctypes.c_int,
                                                            ctypes.POINTER(ctypes.c_void_p), u64p,
                                                            ctypes.c_uint64, ctypes.c_uint64,
                                                            ctypes.c_void_p, ctypes.c_void_p,
                                                            ctypes.c_void_p, ctypes.c_void_p]
            L.s3h_chunk_body_geometry.argtypes = [u64p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                                  u64p, u64p, u64p]
            L.s3h_cpu_chunk_body.argtypes = [ctypes.POINTER(ctypes.c_void_p), u64p, ctypes.c_uint64,
                                             ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, u64p]
            L.s3h_chunk_plan_body.argtypes = [ctypes.c_void_p] * 6 + [u64p, ctypes.c_void_p]
            L.s3h_chunk_plan_body_info.argtypes = [ctypes.c_void_p, u64p, u64p, u64p, u64p, u64p]
            L.s3h_chunk_body_batch_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                      ctypes.c_void_p, u64p, u64p, ctypes.c_uint64,
                                                      ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                                      u64p]
            _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != S3H_OK:
        raise S3HashError(rc, lib().s3h_last_error().decode(errors="replace"))
