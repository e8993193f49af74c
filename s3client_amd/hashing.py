"""Python view of the MI355X batched SHA-256 path (over the C-ABI, include/s3hash.h).

Mirrors lib/hash's interface (/root/reference/lib/hash/sha256.h):
  * ``sha256(data)``        -> 8 digest words, ``hash[i] = bswap32(H_i)`` (sha256.h:70, CPU)
  * ``hmac256(data, key)``  -> 32-byte MAC (hmac256.cpp:60-95, CPU)
  * ``hash_to_text(words)`` -> 64 lowercase hex chars (sha256.h:113-119)
and adds the batched GPU entry points that the parallel upload uses for per-part payload
hashes (lib/src/upload.cpp:89-110 -> S3Api::UploadFilePart(..., payloadHash)):
  * ``Plan`` / ``sha256_batch_device``  -- parts already resident in HBM (torch tensors)
  * ``sha256_batch_host``               -- parts in host memory, sharded over GPUs
  * ``sha256_md5_batch_{host,device}``  -- both digests (x-amz-content-sha256 + Content-MD5)
                                           from one pass over the parts
  * ``sha1_batch_{device,host}``, ``sha256_sha1_batch_host``, ``Plan(..., algo="sha1")``,
    ``Stream(algo="sha1")``             -- SHA-1 (x-amz-checksum-sha1), 5 words per part

Device memory, streams and events come from PyTorch (plumbing only); all hashing is done by
the HIP kernels in s3client_amd/csrc.  Nothing here falls back to the CPU for a batch.
"""
from __future__ import annotations

import ctypes
import os
from typing import Iterable, Sequence

import numpy as np

from . import _native
from ._native import check, lib

DIGEST_WORDS = 8


def _u64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


def _p64(a: np.ndarray):
    return a.ctypes.data_as(_native.u64p)


def device_count() -> int:
    c = ctypes.c_int(0)
    rc = lib().s3h_device_count(ctypes.byref(c))
    return c.value if rc == 0 else 0


def device_pci_bus_id(device: int) -> str:
    """PCI address "dddd:bb:dd.f" of HIP device ``device`` (s3h_device_pci_bus_id)."""
    buf = ctypes.create_string_buffer(64)
    check(lib().s3h_device_pci_bus_id(device, buf, len(buf)))
    return buf.value.decode()


def nblocks(length: int) -> int:
    """64-byte compressions SHA-256 performs on a message of ``length`` bytes."""
    return (int(length) + 72) // 64


def _stream_handle(stream) -> int | None:
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    return getattr(stream, "cuda_stream", stream)


def _device_buffer(name: str, t, need: int, device: int | None = None, align: int = 1,
                   raw: bool = False) -> ctypes.c_void_p:
    """The one gate between a caller's tensor and a device pointer handed to the library: every
    device wrapper below passes each of its tensors through here and gives ``lib()`` only what
    this returns.  The kernels read and write ``need`` contiguous bytes from ``data_ptr()``, so
    anything else would give wrong digests with status OK.  Raises ValueError naming ``name``
    when ``t``
      * is not a device tensor (a host tensor, a numpy array),
      * is on another device than ``device`` (the plan's, stream object's or ``device=``),
      * is not contiguous (``buf[::2]``, a transposed tensor, a column slice ``pool[:, :8]``),
      * holds fewer than ``need`` bytes,
      * starts at an address that misses ``align``, the alignment include/s3hash.h states for
        that argument (16 B for SHA-256 / MD5 digests, seeds and signatures; 8 B for 64-bit
        values; 4 B for SHA-1 digests, 32-bit values and expected words; data: any).
    The element type does not matter (bytes are bytes), nor does a storage offset.  With
    ``raw`` a plain int is taken as a raw device pointer the caller vouches for: the library
    itself checks its alignment.  O(1): no device work, no synchronisation."""
    if raw and isinstance(t, int):
        return ctypes.c_void_p(t)
    if not getattr(t, "is_cuda", False):
        raise ValueError(f"{name} must be a device tensor")
    if device is not None and t.device.index != device:
        raise ValueError(f"{name} is on device {t.device.index}, the call runs on device {device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous: the kernels address {need} consecutive "
                         "bytes from data_ptr(), not the tensor's strides")
    have = t.numel() * t.element_size()
    if have < need:
        raise ValueError(f"{name} buffer too small ({have} B, need {need} B)")
    ptr = t.data_ptr()
    if align > 1 and ptr % align:
        raise ValueError(f"{name} must be {align}-byte aligned (data_ptr() % {align} = {ptr % align})")
    return ctypes.c_void_p(ptr)


def _digest_align(algo: int) -> int:
    # the SHA-256 and MD5 kernels store a digest as 16-byte words, SHA-1 as dwords
    return 4 if algo == _native.ALGO_IDS["sha1"] else 16


def _extent(offs: np.ndarray, lens: np.ndarray) -> int:
    """Bytes of the data buffer that parts (offs, lens) reach."""
    return int((offs + lens).max()) if offs.size else 0


class Plan:
    """Geometry of one batch of parts, uploaded once (s3h_plan_create)."""

    def __init__(self, offsets: Sequence[int], lengths: Sequence[int], device: int = 0,
                 kernel: str | int = "auto", algo: str = "sha256"):
        k = kernel if isinstance(kernel, int) else _native.KERNEL_IDS[kernel]
        self.algo = _native.ALGO_IDS[algo]
        self.words = _native.DIGEST_WORDS[self.algo]
        self.offsets, self.lengths = _u64(offsets), _u64(lengths)
        if self.offsets.shape != self.lengths.shape or self.offsets.ndim != 1:
            raise ValueError("offsets and lengths must be 1-D and of equal length")
        self.n = int(self.lengths.size)
        self.device = device
        h = ctypes.c_void_p()
        check(lib().s3h_plan_create_ex(device, self.algo, _p64(self.offsets), _p64(self.lengths),
                                       self.n, k, ctypes.byref(h)))
        self._h = h

    def info(self) -> dict:
        n, tb, mb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        k, g = ctypes.c_int(), ctypes.c_uint32()
        check(lib().s3h_plan_info(self._h, ctypes.byref(n), ctypes.byref(tb), ctypes.byref(mb),
                                  ctypes.byref(k), ctypes.byref(g)))
        groups, solo = ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().s3h_plan_groups(self._h, ctypes.byref(groups), ctypes.byref(solo)))
        dual_solo, apart = ctypes.c_uint32(), ctypes.c_int()
        check(lib().s3h_plan_dual_layout(self._h, ctypes.byref(dual_solo), ctypes.byref(apart)))
        return {"n": n.value, "total_blocks": tb.value, "max_blocks": mb.value,
                "kernel": _native.KERNEL_NAMES[k.value], "grid": g.value,
                "groups": groups.value, "solo": solo.value, "dual_solo": dual_solo.value,
                "dual_apart": bool(apart.value)}

    def set_clock_probe(self, clocks=None) -> int:
        """Record per-consumer-wave clock counters on later launches (skew kernel only):
        ``clocks`` is a device int64 tensor of >= 4 x waves entries ({clk0, clk1, rt0, rt1}
        per wave, s_memtime / s_memrealtime); None switches the probe off.  Returns the
        number of consumer waves that record (0 if the plan's kernel does not)."""
        w = ctypes.c_uint32()
        ptr = (None if clocks is None else
               _device_buffer("clock buffer", clocks, 0, self.device, align=8))
        check(lib().s3h_plan_set_clock_probe(self._h, ptr, ctypes.byref(w)))
        if clocks is not None and clocks.numel() * clocks.element_size() < 32 * w.value:
            lib().s3h_plan_set_clock_probe(self._h, None, None)
            raise ValueError(f"clock buffer needs {4 * w.value} int64 entries")
        return w.value

    def _digests_ptr(self, digests) -> ctypes.c_void_p:
        return _device_buffer("digests", digests, 4 * self.words * self.n, self.device,
                              align=_digest_align(self.algo))

    def launch(self, data, digests, stream=None) -> None:
        """Hash every part of ``data`` (device tensor) into ``digests`` (n*8 words; contiguous,
        16-byte aligned for SHA-256 and MD5, 4-byte for SHA-1).  Asynchronous on ``stream``."""
        d_base = _device_buffer("data", data, _extent(self.offsets, self.lengths), self.device)
        check(lib().s3h_plan_launch(self._h, d_base, self._digests_ptr(digests),
                                    ctypes.c_void_p(_stream_handle(stream))))

    def status(self, stream=None) -> None:
        """Wait for ``stream`` and raise S3HashError (S3H_EHIP, "synchronisation timeout") if a
        launch since the last check reported a fault through the plan's device error word --
        its digests are then invalid (s3h_plan_status).  Clears the word."""
        check(lib().s3h_plan_status(self._h, ctypes.c_void_p(_stream_handle(stream))))

    def launch_range(self, data_ptr: int, digests, blk_begin: int, blk_end: int,
                     blk_origin: int, stream=None) -> None:
        check(lib().s3h_plan_launch_range(self._h, ctypes.c_void_p(data_ptr),
                                          self._digests_ptr(digests), blk_begin,
                                          blk_end, blk_origin,
                                          ctypes.c_void_p(_stream_handle(stream))))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().s3h_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def sha256_batch_device(data, offsets, lengths, device: int | None = None, kernel="auto",
                        stream=None, algo: str = "sha256"):
    """Digest every part [offsets[i], offsets[i]+lengths[i]) of the device tensor ``data``.

    Returns an (n, 8) int32 device tensor holding the uint32 digest words (lib/hash layout);
    (n, 4) for algo="md5"."""
    import torch
    _device_buffer("data", data, 0, device)  # (a host tensor has no device to plan for)
    dev = data.device.index if device is None else device
    with Plan(offsets, lengths, device=dev, kernel=kernel, algo=algo) as plan:
        out = torch.empty((plan.n, plan.words), dtype=torch.int32, device=data.device)
        plan.launch(data, out, stream)
        plan.status(stream)  # waits for the launch; raises if it reported a fault
    return out


def md5_batch_device(data, offsets, lengths, device: int | None = None, stream=None):
    """Batched MD5 of device-resident parts: (n, 4) int32 device tensor (LE digest words)."""
    return sha256_batch_device(data, offsets, lengths, device, "auto", stream, algo="md5")


def _as_bytes(p) -> np.ndarray:
    if type(p) is np.ndarray and p.dtype == np.uint8 and p.ndim == 1 and p.flags.c_contiguous:
        return p
    if isinstance(p, (bytes, bytearray, memoryview)):
        return np.frombuffer(p, dtype=np.uint8)
    return np.ascontiguousarray(p, dtype=np.uint8).reshape(-1)


def _addr(a: np.ndarray) -> int:
    # c_char.from_buffer is ~3x cheaper than a.ctypes.data / __array_interface__ (which build
    # objects per part: ~2 ms of a 1,024-part call); it needs a writable, non-empty buffer
    if not a.size:
        return 0
    if a.flags.writeable:
        return ctypes.addressof(ctypes.c_char.from_buffer(a))
    return a.__array_interface__["data"][0]


class BufferParts:
    """Host parts given as (offset, length) ranges of ONE host buffer -- a numpy uint8 array or
    a CPU torch tensor (pinned or pageable) -- usable wherever the host entry points take a
    sequence of parts.  The part pointers are formed in numpy, with no Python object per part
    (a 1,024-part call marshals in ~0.02 ms instead of ~0.5 ms for a list of views)."""

    def __init__(self, buf, offsets, lengths):
        if hasattr(buf, "data_ptr"):  # torch tensor
            if buf.is_cuda:
                raise ValueError("BufferParts takes host memory (use the *_device calls for HBM)")
            if not buf.is_contiguous():
                raise ValueError("BufferParts needs a contiguous buffer")
            base, size = buf.data_ptr(), buf.numel() * buf.element_size()
        else:
            buf = _as_bytes(buf)
            base, size = (buf.ctypes.data if buf.size else 0), int(buf.size)
        self._keep = buf
        offs, lens = _u64(offsets), _u64(lengths)
        if offs.shape != lens.shape or offs.ndim != 1:
            raise ValueError("offsets and lengths must be 1-D and of equal length")
        sz = np.uint64(size)
        if bool(((lens > 0) & ((offs > sz) | (lens > sz - np.minimum(offs, sz)))).any()):
            raise ValueError("a part extends past the end of the buffer")
        self.lens = lens
        self.addrs = np.where(lens > 0, offs + np.uint64(base), np.uint64(0)).astype(np.uint64)
        self.ptrs = self.addrs.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p))

    def __len__(self) -> int:
        return int(self.lens.size)


def _host_parts(parts):
    if isinstance(parts, BufferParts):
        return parts, parts.ptrs, parts.lens
    arrs = [_as_bytes(p) for p in parts]
    n = len(arrs)
    ptrs = (ctypes.c_void_p * n)(*[_addr(a) for a in arrs])
    return arrs, ptrs, np.fromiter((a.size for a in arrs), dtype=np.uint64, count=n)


def _host_batch(fn, words, parts, ndevices, slice_bytes):
    arrs, ptrs, lens = _host_parts(parts)
    n = len(arrs)
    out = np.zeros((n, words), dtype=np.uint32)
    check(fn(ptrs, _p64(lens), n, out.ctypes.data, ndevices, slice_bytes))
    return out


def sha256_md5_batch_host(parts: Sequence, ndevices: int = 0,
                          slice_bytes: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """SHA-256 (n, 8) and MD5 (n, 4) uint32 digests of host-resident parts, each part crossing
    PCIe once (s3h_sha256_md5_batch_host)."""
    arrs, ptrs, lens = _host_parts(parts)
    n = len(arrs)
    sha = np.zeros((n, 8), dtype=np.uint32)
    m5 = np.zeros((n, 4), dtype=np.uint32)
    check(lib().s3h_sha256_md5_batch_host(ptrs, _p64(lens), n, sha.ctypes.data, m5.ctypes.data,
                                          ndevices, slice_bytes))
    return sha, m5


def sha256_md5_batch_device(data, offsets, lengths, device: int | None = None, stream=None):
    """SHA-256 (n, 8) and MD5 (n, 4) int32 device tensors of device-resident parts
    (s3h_sha256_md5_batch_device): one grid running both chains while the batch fits one
    workgroup per CU, above that the two kernels one after the other on ``stream``."""
    import torch
    _device_buffer("data", data, 0, device)
    dev = data.device.index if device is None else device
    offs, lens = _u64(offsets), _u64(lengths)
    if offs.shape != lens.shape:
        raise ValueError("offsets and lengths differ in length")
    n = int(lens.size)
    d_base = _device_buffer("data", data, _extent(offs, lens), dev)
    sha = torch.empty((n, 8), dtype=torch.int32, device=data.device)
    m5 = torch.empty((n, 4), dtype=torch.int32, device=data.device)
    check(lib().s3h_sha256_md5_batch_device(dev, d_base, _p64(offs), _p64(lens), n,
                                            _device_buffer("sha256 digests", sha, 32 * n, dev, align=16),
                                            _device_buffer("md5 digests", m5, 16 * n, dev, align=16),
                                            _stream_handle(stream)))
    return sha, m5


def md5_batch_host(parts: Sequence, ndevices: int = 0, slice_bytes: int = 0) -> np.ndarray:
    """Batched MD5 of host-resident parts on the GPUs: (n, 4) uint32."""
    return _host_batch(lib().s3h_md5_batch_host, 4, parts, ndevices, slice_bytes)


def verify_batch_host(parts: Sequence, expected, algo: str = "sha256",
                      ndevices: int = 0) -> np.ndarray:
    """Download-side verification: bool mask of parts whose digest differs from ``expected``
    ((n, 8) uint32 SHA-256, (n, 4) MD5 or (n, 5) SHA-1 words for ``algo`` "sha256" / "md5" /
    "sha1", or a list of hex strings).  Every word is compared.  The library writes all n mask
    bytes, 0 or 1, nothing behind them, and a count equal to their sum (s3h_verify_batch_host)."""
    a = _native.ALGO_IDS[algo]
    words = _native.DIGEST_WORDS[a]
    if len(expected) and isinstance(expected[0], str):
        expected = np.stack([np.frombuffer(bytes.fromhex(h), dtype=np.uint32) for h in expected])
    exp = np.ascontiguousarray(expected, dtype=np.uint32).reshape(-1, words)
    arrs, ptrs, lens = _host_parts(parts)
    n = len(arrs)
    if exp.shape[0] != n:
        raise ValueError("expected digest count differs from part count")
    mism = np.zeros(n, dtype=np.uint8)
    cnt = ctypes.c_uint64(0)
    check(lib().s3h_verify_batch_host(a, ptrs, _p64(lens), n, exp.ctypes.data, mism.ctypes.data,
                                      ctypes.byref(cnt), ndevices))
    assert cnt.value == int(mism.sum())
    return mism.astype(bool)


def verify_batch_routed(parts: Sequence, expected, algo: str = "sha256", ndevices: int = 0,
                        route: str = "auto") -> tuple[np.ndarray, str]:
    """verify_batch_host on a route (s3h_verify_batch_routed): "gpu", "cpu", "split" or "auto"
    as sha256_batch_routed / md5_batch_routed, for either algorithm.  Returns (bool mismatch
    mask, route taken)."""
    a = _native.ALGO_IDS[algo]
    words = _native.DIGEST_WORDS[a]
    if len(expected) and isinstance(expected[0], str):
        expected = np.stack([np.frombuffer(bytes.fromhex(h), dtype=np.uint32) for h in expected])
    exp = np.ascontiguousarray(expected, dtype=np.uint32).reshape(-1, words)
    arrs, ptrs, lens = _host_parts(parts)
    n = len(arrs)
    if exp.shape[0] != n:
        raise ValueError("expected digest count differs from part count")
    mism = np.zeros(n, dtype=np.uint8)
    cnt = ctypes.c_uint64(0)
    taken = ctypes.c_int(-1)
    check(lib().s3h_verify_batch_routed(a, ptrs, _p64(lens), n, exp.ctypes.data, mism.ctypes.data,
                                        ctypes.byref(cnt), ndevices, _native.ROUTE_IDS[route],
                                        ctypes.byref(taken)))
    assert cnt.value == int(mism.sum())
    return mism.astype(bool), _native.ROUTE_NAMES[taken.value]


def verify_batch_device(data, offsets, lengths, expected, algo: str = "sha256", stream=None):
    """Device-resident verification: returns (mismatch count, bool mask on the device)."""
    import torch
    a = _native.ALGO_IDS[algo]
    offs, lens = _u64(offsets), _u64(lengths)
    d_base = _device_buffer("data", data, _extent(offs, lens))
    dev = data.device.index
    d_exp = _device_buffer("expected", expected, 4 * _native.DIGEST_WORDS[a] * offs.size, dev, align=4)
    mism = torch.zeros(offs.size, dtype=torch.uint8, device=data.device)
    cnt = ctypes.c_uint64(0)
    check(lib().s3h_verify_batch_device(dev, a, d_base, _p64(offs), _p64(lens), offs.size, d_exp,
                                        _device_buffer("mask", mism, offs.size, dev),
                                        ctypes.byref(cnt), ctypes.c_void_p(_stream_handle(stream))))
    return cnt.value, mism.bool()


# ------------------------------------------------------------------ CRC-32C / CRC-32 checksums
def _crc_id(algo) -> int:
    return algo if isinstance(algo, int) else _native.CRC_IDS[algo]


class CrcPlan:
    """Segment geometry of one batch of device-resident parts for CRC-32C / CRC-32
    (s3h_crc_plan_create).  One plan runs on one stream at a time: its segment values pass
    through a buffer the plan owns.  ``launch`` checksums whole parts; ``launch_range`` a byte
    range of every part, resumable (after a ``launch`` the next range must begin at 0)."""

    _prefix = "s3h_crc_plan_"   # the C entry points of this plan type
    _value_bytes = 4            # bytes per value in ``crcs``

    def _create(self, h) -> int:
        return lib().s3h_crc_plan_create(self.device, self.crc, _p64(self.offsets),
                                         _p64(self.lengths), self.n, ctypes.byref(h))

    def __init__(self, offsets: Sequence[int], lengths: Sequence[int], device: int = 0,
                 algo: str | int = "crc32c"):
        self.crc = _crc_id(algo)
        self.offsets, self.lengths = _u64(offsets), _u64(lengths)
        if self.offsets.shape != self.lengths.shape or self.offsets.ndim != 1:
            raise ValueError("offsets and lengths must be 1-D and of equal length")
        self.n = int(self.lengths.size)
        self.device = device
        h = ctypes.c_void_p()
        check(self._create(h))
        self._h = h

    def info(self) -> dict:
        n, segs, sb, g = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
        check(getattr(lib(), self._prefix + "info")(self._h, ctypes.byref(n), ctypes.byref(segs),
                                                    ctypes.byref(sb), ctypes.byref(g)))
        return {"n": n.value, "segments": segs.value, "segment_bytes": sb.value, "grid": g.value}

    def _crcs_ptr(self, crcs) -> ctypes.c_void_p:
        return _device_buffer("crcs", crcs, self._value_bytes * self.n, self.device,
                              align=self._value_bytes)

    def launch(self, data, crcs, stream=None) -> None:
        """CRC of every part of ``data`` (device tensor) into ``crcs`` (n 32-bit words, device).
        Asynchronous on ``stream``."""
        d_base = _device_buffer("data", data, _extent(self.offsets, self.lengths), self.device)
        check(getattr(lib(), self._prefix + "launch")(self._h, d_base, self._crcs_ptr(crcs),
                                                      ctypes.c_void_p(_stream_handle(stream))))

    def launch_range(self, data, crcs, byte_begin: int, byte_end: int, byte_origin: int = 0,
                     stream=None) -> None:
        """Resumable form (s3h_crc_plan_launch_range): bytes [byte_begin, byte_end) of every
        part, part p's byte b at ``data + offsets[p] + (b - byte_origin)``; the running values
        stay in the plan.  ``crcs[p]`` is written by the launch whose range holds part p's last
        byte (an empty part's by a launch with byte_begin == 0), no other entry is touched.
        byte_begin is 0 (a new pass) or the previous ranged launch's byte_end."""
        end = 0
        if byte_origin <= byte_begin < byte_end and self.n:  # (the library rejects the rest)
            top = np.minimum(self.lengths, np.uint64(byte_end))
            live = top > np.uint64(byte_begin)
            end = int((self.offsets[live] + top[live]).max()) - byte_origin if live.any() else 0
        d_base = _device_buffer("data", data, end, self.device)
        check(getattr(lib(), self._prefix + "launch_range")(
            self._h, d_base, self._crcs_ptr(crcs), byte_begin, byte_end, byte_origin,
            ctypes.c_void_p(_stream_handle(stream))))

    def close(self) -> None:
        if getattr(self, "_h", None):
            getattr(lib(), self._prefix + "destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def crc_batch_device(data, offsets, lengths, algo: str | int = "crc32c", stream=None):
    """CRC-32C / CRC-32 of every part [offsets[i], offsets[i]+lengths[i]) of the device tensor
    ``data`` (any byte alignment): an (n,) int32 device tensor holding the uint32 values
    (``.cpu().numpy().view(np.uint32)``), what zlib.crc32 returns for CRC-32.  Blocking."""
    import torch
    offs, lens = _u64(offsets), _u64(lengths)
    d_base = _device_buffer("data", data, _extent(offs, lens))
    dev = data.device.index
    out = torch.empty(offs.size, dtype=torch.int32, device=data.device)
    check(lib().s3h_crc_batch_device(dev, _crc_id(algo), d_base, _p64(offs), _p64(lens),
                                     offs.size, _device_buffer("crcs", out, 4 * offs.size, dev, align=4),
                                     ctypes.c_void_p(_stream_handle(stream))))
    return out


def crc_batch_host(parts: Sequence, algo: str | int = "crc32c", ndevices: int = 0,
                   slice_bytes: int = 0) -> np.ndarray:
    """CRC-32C / CRC-32 of host-resident parts on the GPUs (s3h_crc_batch_host): (n,) uint32."""
    arrs, ptrs, lens = _host_parts(parts)
    n = len(arrs)
    out = np.zeros(n, dtype=np.uint32)
    check(lib().s3h_crc_batch_host(_crc_id(algo), ptrs, _p64(lens), n, out.ctypes.data, ndevices,
                                   slice_bytes))
    return out


def sha256_crc_batch_host(parts: Sequence, algo: str | int = "crc32c", ndevices: int = 0,
                          slice_bytes: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """SHA-256 (n, 8) digests and CRC-32C / CRC-32 values (n,) of host-resident parts, each part
    crossing PCIe once (s3h_sha256_crc_batch_host): x-amz-content-sha256 and
    x-amz-checksum-crc32c / -crc32 of UploadPart."""
    arrs, ptrs, lens = _host_parts(parts)
    n = len(arrs)
    sha = np.zeros((n, DIGEST_WORDS), dtype=np.uint32)
    out = np.zeros(n, dtype=np.uint32)
    check(lib().s3h_sha256_crc_batch_host(_crc_id(algo), ptrs, _p64(lens), n, sha.ctypes.data,
                                          out.ctypes.data, ndevices, slice_bytes))
    return sha, out


def sha256_crc_file_parts(path: str, offsets, lengths, algo: str | int = "crc32c",
                          ndevices: int = 0, slice_bytes: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """SHA-256 (n, 8) digests and CRC values (n,) of file ranges, each slice read once
    (s3h_sha256_crc_file_parts)."""
    offs, lens = _u64(offsets), _u64(lengths)
    if offs.shape != lens.shape or offs.ndim != 1 or offs.size == 0:
        raise ValueError("offsets and lengths must be 1-D, equal length and non-empty")
    sha = np.zeros((offs.size, DIGEST_WORDS), dtype=np.uint32)
    out = np.zeros(offs.size, dtype=np.uint32)
    check(lib().s3h_sha256_crc_file_parts(_crc_id(algo), os.fsencode(path), _p64(offs), _p64(lens),
                                          offs.size, sha.ctypes.data, out.ctypes.data, ndevices,
                                          slice_bytes))
    return sha, out


def crc_verify_batch_device(data, offsets, lengths, expected, algo: str | int = "crc32c",
                            stream=None):
    """Device-resident verification against ``expected`` (n 32-bit words, device): returns
    (mismatch count, bool mask on the device)."""
    import torch
    offs, lens = _u64(offsets), _u64(lengths)
    d_base = _device_buffer("data", data, _extent(offs, lens))
    dev = data.device.index
    d_exp = _device_buffer("expected", expected, 4 * offs.size, dev, align=4)
    mism = torch.zeros(offs.size, dtype=torch.uint8, device=data.device)
    cnt = ctypes.c_uint64(0)
    check(lib().s3h_crc_verify_batch_device(dev, _crc_id(algo), d_base, _p64(offs), _p64(lens),
                                            offs.size, d_exp,
                                            _device_buffer("mask", mism, offs.size, dev),
                                            ctypes.byref(cnt),
                                            ctypes.c_void_p(_stream_handle(stream))))
    return cnt.value, mism.bool()


def crc(data, algo: str | int = "crc32c", seed: int = 0) -> int:
    """CPU CRC of one message (s3h_cpu_crc); ``seed`` = a previous call's result, so chunks
    chain like zlib.crc32(data, seed)."""
    a = _as_bytes(data) if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), dtype=np.uint8)
    return int(lib().s3h_cpu_crc(_crc_id(algo), ctypes.c_void_p(a.ctypes.data if a.size else None),
                                 a.size, seed & 0xFFFFFFFF))


def crc_combine(crc_a: int, crc_b: int, len_b: int, algo: str | int = "crc32c") -> int:
    """crc(A || B) from crc(A), crc(B) and len(B) (s3h_crc_combine)."""
    out = ctypes.c_uint32()
    check(lib().s3h_crc_combine(_crc_id(algo), crc_a & 0xFFFFFFFF, crc_b & 0xFFFFFFFF,
                                int(len_b), ctypes.byref(out)))
    return out.value


def crc_object(part_crcs, lengths, algo: str | int = "crc32c") -> int:
    """FULL_OBJECT checksum of the parts' concatenation from their CRCs and lengths."""
    w = np.ascontiguousarray(part_crcs).astype(np.uint32, copy=False).reshape(-1)
    lens = _u64(lengths)
    if lens.shape != w.shape:
        raise ValueError("one length per part checksum")
    out = ctypes.c_uint32()
    check(lib().s3h_crc_object(_crc_id(algo), ctypes.c_void_p(w.ctypes.data), _p64(lens), w.size,
                               ctypes.byref(out)))
    return out.value


def checksum_text(part_crcs, algo: str | int = "crc32c", composite: bool = False) -> str:
    """Header text of a checksum (s3h_checksum_text): base64 of one CRC's big-endian bytes, or
    with ``composite`` the S3 composite form of the parts' CRCs, "<base64>-<n>"."""
    w = np.ascontiguousarray(np.atleast_1d(part_crcs)).astype(np.uint32, copy=False).reshape(-1)
    out = ctypes.create_string_buffer(_native.CHECKSUM_MAX)
    check(lib().s3h_checksum_text(_crc_id(algo), ctypes.c_void_p(w.ctypes.data), w.size,
                                  int(bool(composite)), out, len(out)))
    return out.value.decode()


# ------------------------------------------------------------------ SHA-1 checksum
def sha1_batch_device(data, offsets, lengths, device: int | None = None, stream=None):
    """Batched SHA-1 (x-amz-checksum-sha1) of device-resident parts: (n, 5) int32 device tensor,
    word i = bswap32(H_i) (the 20 bytes of a row are the canonical digest)."""
    return sha256_batch_device(data, offsets, lengths, device, "auto", stream, algo="sha1")


def sha1_batch_host(parts: Sequence, ndevices: int = 0, slice_bytes: int = 0) -> np.ndarray:
    """Batched SHA-1 of host-resident parts on the GPUs (s3h_sha1_batch_host): (n, 5) uint32."""
    return _host_batch(lib().s3h_sha1_batch_host, 5, parts, ndevices, slice_bytes)


def sha256_sha1_batch_host(parts: Sequence, ndevices: int = 0,
                           slice_bytes: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """SHA-256 (n, 8) and SHA-1 (n, 5) uint32 digests of host-resident parts, each part crossing
    PCIe once (s3h_sha256_sha1_batch_host)."""
    arrs, ptrs, lens = _host_parts(parts)
    n = len(arrs)
    sha = np.zeros((n, DIGEST_WORDS), dtype=np.uint32)
    s1 = np.zeros((n, 5), dtype=np.uint32)
    check(lib().s3h_sha256_sha1_batch_host(ptrs, _p64(lens), n, sha.ctypes.data, s1.ctypes.data,
                                           ndevices, slice_bytes))
    return sha, s1


def sha1_file_parts(path: str, offsets, lengths, ndevices: int = 0, slice_bytes: int = 0) -> np.ndarray:
    """SHA-1 of file ranges on the GPU (s3h_sha1_file_parts): (n, 5) uint32."""
    offs, lens = _u64(offsets), _u64(lengths)
    if offs.shape != lens.shape or offs.ndim != 1 or offs.size == 0:
        raise ValueError("offsets and lengths must be 1-D, equal length and non-empty")
    out = np.zeros((offs.size, 5), dtype=np.uint32)
    check(lib().s3h_sha1_file_parts(os.fsencode(path), _p64(offs), _p64(lens), offs.size,
                                    out.ctypes.data, ndevices, slice_bytes))
    return out


def sha256_sha1_file_parts(path: str, offsets, lengths, ndevices: int = 0,
                           slice_bytes: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """SHA-256 (n, 8) and SHA-1 (n, 5) uint32 digests of file ranges, each slice read once
    (s3h_sha256_sha1_file_parts)."""
    offs, lens = _u64(offsets), _u64(lengths)
    if offs.shape != lens.shape or offs.ndim != 1 or offs.size == 0:
        raise ValueError("offsets and lengths must be 1-D, equal length and non-empty")
    sha = np.zeros((offs.size, DIGEST_WORDS), dtype=np.uint32)
    s1 = np.zeros((offs.size, 5), dtype=np.uint32)
    check(lib().s3h_sha256_sha1_file_parts(os.fsencode(path), _p64(offs), _p64(lens), offs.size,
                                           sha.ctypes.data, s1.ctypes.data, ndevices, slice_bytes))
    return sha, s1


def sha1(data: bytes) -> np.ndarray:
    """SHA-1 on the CPU (s3h_cpu_sha1, single message): 5 words, hash[i] = bswap32(H_i)."""
    b = bytes(data)
    out = np.zeros(5, dtype=np.uint32)
    lib().s3h_cpu_sha1(b, len(b), out.ctypes.data)
    return out


def digest_checksum_text(digests, algo: str = "sha1", composite: bool = False) -> str:
    """Header text of a digest checksum (s3h_digest_checksum_text), ``algo`` "sha1" or "sha256":
    base64 of one digest (x-amz-checksum-sha1 / -sha256 of a part or a single-PUT object), or
    with ``composite`` S3's COMPOSITE form of the parts' digests, "<base64>-<n>"."""
    a = _native.ALGO_IDS[algo]
    w = np.ascontiguousarray(digests).astype(np.uint32, copy=False).reshape(-1, _native.DIGEST_WORDS[a])
    out = ctypes.create_string_buffer(_native.DIGEST_CHECKSUM_MAX)
    check(lib().s3h_digest_checksum_text(a, ctypes.c_void_p(w.ctypes.data), w.shape[0],
                                         int(bool(composite)), out, len(out)))
    return out.value.decode()


# ------------------------------------------------------------------ CRC-64/NVME checksum
# ---------------------------------------------------------------- SigV4 chunk-signed uploads
def sigv4_signing_key(secret: str, date: str, region: str, service: str = "s3") -> bytes:
    """The SigV4 signing key (32 bytes) of ``secret`` for a date "YYYYMMDD", region and service
    (s3h_sigv4_signing_key, CPU)."""
    key = ctypes.create_string_buffer(32)
    check(lib().s3h_sigv4_signing_key(secret.encode(), date.encode(), region.encode(),
                                      service.encode(), key))
    return key.raw


class ChunkSignContext:
    """The constant part of every chunk's string to sign of one aws-chunked request, hashed once
    (s3h_chunk_sign_ctx_create): signing key, timestamp "YYYYMMDDThhmmssZ", date, region,
    service.  Immutable; CPU."""

    def __init__(self, key: bytes, timestamp: str, date: str, region: str, service: str = "s3"):
        if len(key) != 32:
            raise ValueError("the signing key is 32 bytes")
        h = ctypes.c_void_p()
        check(lib().s3h_chunk_sign_ctx_create(bytes(key), timestamp.encode(), date.encode(),
                                              region.encode(), service.encode(), ctypes.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().s3h_chunk_sign_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def chunk_geometry(lengths, chunk_bytes: int) -> dict:
    """Chunk geometry of parts of ``lengths`` cut at ``chunk_bytes`` (s3h_chunk_geometry, no
    GPU): per part its data chunks and the index of its first signature, and the totals."""
    lens = _u64(lengths)
    n = int(lens.size)
    counts, sig = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    chunks, sigs, longest = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    check(lib().s3h_chunk_geometry(_p64(lens), n, int(chunk_bytes), _p64(counts), _p64(sig),
                                   ctypes.byref(chunks), ctypes.byref(sigs), ctypes.byref(longest)))
    return {"n": n, "data_chunks_per_part": counts, "signature_offsets": sig,
            "data_chunks": chunks.value, "signatures": sigs.value,
            "max_chunks_per_part": longest.value}


def _words(a, rows: int | None, what: str) -> np.ndarray:
    """(rows, 8) uint32 view of signatures / digests given as words or raw bytes."""
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(a, dtype=np.uint8)
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8).view(np.uint32).reshape(-1, 8)
    if rows is not None and a.shape[0] != rows:
        raise ValueError(f"{what}: {a.shape[0]} rows of 8 words, expected {rows}")
    return a


def cpu_chunk_signatures(ctx: ChunkSignContext, chunk_digests, data_chunks_per_part,
                         seeds) -> np.ndarray:
    """The signature chains on the CPU over ready chunk digests (s3h_cpu_chunk_signatures):
    ``chunk_digests`` (data chunks, 8) words part-major, ``data_chunks_per_part`` n counts,
    ``seeds`` (n, 8).  Returns (data chunks + n, 8) uint32, part-major: each part's data-chunk
    signatures, then the signature of its final 0-byte chunk."""
    counts = _u64(data_chunks_per_part)
    n, total = int(counts.size), int(counts.sum())
    dig = _words(chunk_digests, total, "chunk digests") if total else None
    sd = _words(seeds, n, "seeds")
    out = np.zeros((total + n, 8), dtype=np.uint32)
    check(lib().s3h_cpu_chunk_signatures(ctx._h, dig.ctypes.data if total else None, _p64(counts),
                                         n, sd.ctypes.data, out.ctypes.data))
    return out


def chunk_header_text(chunk_len: int, signature) -> str:
    """The framing line before a chunk: "<hex len>;chunk-signature=<64 hex>\r\n"."""
    sig = _words(signature, 1, "signature")
    buf = ctypes.create_string_buffer(_native.CHUNK_HEADER_MAX)
    check(lib().s3h_chunk_header_text(int(chunk_len), sig.ctypes.data, buf, len(buf)))
    return buf.value.decode()


class ChunkSignPlan:
    """Device-resident parts cut into chunks of ``chunk_bytes``: a SHA-256 plan over the chunks
    plus each part's chain record (s3h_chunk_plan_create).  ``signature_offsets[p]`` is the row
    of part p's first signature; part p has ``data_chunks_per_part[p] + 1`` of them.

    ``trailer`` = "crc32c", "crc32" or "crc64nvme" makes it a trailer plan
    (s3h_chunk_plan_create_trailer, STREAMING-AWS4-HMAC-SHA256-PAYLOAD-TRAILER): it also owns a
    CRC plan over the whole parts, and ``launch_trailer`` / ``trailer`` give each part's
    checksum and trailer signature."""

    def __init__(self, offsets: Sequence[int], lengths: Sequence[int], chunk_bytes: int,
                 device: int = 0, trailer: str | None = None):
        self.offsets, self.lengths = _u64(offsets), _u64(lengths)
        if self.offsets.shape != self.lengths.shape or self.offsets.ndim != 1:
            raise ValueError("offsets and lengths must be 1-D and of equal length")
        self.n = int(self.lengths.size)
        self.chunk_bytes = int(chunk_bytes)
        self.device = device
        g = chunk_geometry(self.lengths, self.chunk_bytes)
        self.data_chunks_per_part = g["data_chunks_per_part"]
        self.signature_offsets = g["signature_offsets"]
        self.signatures = g["signatures"]
        self.trailer_kind = trailer
        h = ctypes.c_void_p()
        if trailer is None:
            check(lib().s3h_chunk_plan_create(device, _p64(self.offsets), _p64(self.lengths), self.n,
                                              self.chunk_bytes, ctypes.byref(h)))
        else:
            check(lib().s3h_chunk_plan_create_trailer(device, _trailer_id(trailer), _p64(self.offsets),
                                                      _p64(self.lengths), self.n, self.chunk_bytes,
                                                      ctypes.byref(h)))
        self._h = h
        self._body_lengths = None  # of the first body launch (s3h_chunk_plan_body_info)

    def info(self) -> dict:
        n, c, s, m = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        name = ctypes.create_string_buffer(16)
        check(lib().s3h_chunk_plan_info(self._h, ctypes.byref(n), ctypes.byref(c), ctypes.byref(s),
                                        ctypes.byref(m), name, len(name)))
        return {"n": n.value, "data_chunks": c.value, "signatures": s.value,
                "max_chunks_per_part": m.value, "kernel": name.value.decode()}

    def _ptrs(self, *args) -> list:
        # (name, tensor or raw device pointer, bytes needed, alignment) -> validated pointers
        return [_device_buffer(name, t, need, self.device, align, raw=True)
                for name, t, need, align in args]

    def launch(self, data, ctx: ChunkSignContext, seeds, out, stream=None) -> None:
        """Hash every chunk of ``data`` and chain the signatures into ``out`` (signatures x 8
        words) from ``seeds`` (n x 8 words).  Device tensors, or raw device pointers (ints)."""
        ptrs = self._ptrs(("data", data, _extent(self.offsets, self.lengths), 1),
                          ("seeds", seeds, 32 * self.n, 16), ("out", out, 32 * self.signatures, 16))
        check(lib().s3h_chunk_plan_launch(self._h, ctx._h, *ptrs,
                                          ctypes.c_void_p(_stream_handle(stream))))

    def chain(self, ctx: ChunkSignContext, chunk_digests, seeds, out, stream=None) -> None:
        """The chain kernel alone over ``chunk_digests`` (device tensor, data chunks x 8 words in
        this plan's geometry) that the caller hashed itself (s3h_chunk_plan_chain)."""
        chunks = int(self.data_chunks_per_part.sum())
        ptrs = self._ptrs(("chunk_digests", chunk_digests, 32 * chunks, 16),
                          ("seeds", seeds, 32 * self.n, 16), ("out", out, 32 * self.signatures, 16))
        check(lib().s3h_chunk_plan_chain(self._h, ctx._h, *ptrs,
                                         ctypes.c_void_p(_stream_handle(stream))))

    def _value_bytes(self) -> int:
        if self.trailer_kind is None:
            return 4  # (the library refuses the launch)
        return np.dtype(_native.TRAILER_VALUE[_trailer_id(self.trailer_kind)][0]).itemsize

    def launch_trailer(self, data, ctx: ChunkSignContext, seeds, out, checksums, trailer_out,
                       stream=None) -> None:
        """``launch``, then each part's CRC into ``checksums`` (n 32-bit words, or 64-bit for
        crc64nvme) and its trailer signature into ``trailer_out`` (n x 8 words), all on
        ``stream`` (s3h_chunk_plan_launch_trailer).  Device tensors, or raw device pointers."""
        vb = self._value_bytes()
        ptrs = self._ptrs(("data", data, _extent(self.offsets, self.lengths), 1),
                          ("seeds", seeds, 32 * self.n, 16), ("out", out, 32 * self.signatures, 16),
                          ("checksums", checksums, vb * self.n, vb),
                          ("trailer_out", trailer_out, 32 * self.n, 16))
        check(lib().s3h_chunk_plan_launch_trailer(self._h, ctx._h, *ptrs,
                                                  ctypes.c_void_p(_stream_handle(stream))))

    def trailer(self, ctx: ChunkSignContext, signatures, checksums, trailer_out, stream=None) -> None:
        """The trailer kernel alone over chunk ``signatures`` (this plan's geometry) and
        ``checksums`` already on the device (s3h_chunk_plan_trailer)."""
        vb = self._value_bytes()
        ptrs = self._ptrs(("signatures", signatures, 32 * self.signatures, 16),
                          ("checksums", checksums, vb * self.n, vb),
                          ("trailer_out", trailer_out, 32 * self.n, 16))
        check(lib().s3h_chunk_plan_trailer(self._h, ctx._h, *ptrs,
                                           ctypes.c_void_p(_stream_handle(stream))))

    def body_info(self) -> dict:
        """The plan's body lengths (each part's Content-Length) and their sum, and the body
        kernel's shape: work items, the most bytes of a chunk one item copies, workgroups
        (s3h_chunk_plan_body_info)."""
        lens = np.zeros(self.n, dtype=np.uint64)
        total, items, piece, grid = (ctypes.c_uint64() for _ in range(4))
        check(lib().s3h_chunk_plan_body_info(self._h, _p64(lens), ctypes.byref(total), ctypes.byref(items),
                                             ctypes.byref(piece), ctypes.byref(grid)))
        return {"body_lengths": lens, "total": total.value, "items": items.value,
                "piece_bytes": piece.value, "grid": grid.value}

    def body(self, data, signatures, body, checksums=None, trailer_signatures=None, body_offsets=None,
             stream=None) -> None:
        """Write every part's aws-chunked body into ``body`` on ``stream`` (s3h_chunk_plan_body):
        part p's at byte ``body_offsets[p]`` (host values; None: packed back to back), framed
        with ``signatures`` as ``launch`` wrote them.  A trailer plan also takes ``checksums``
        and ``trailer_signatures`` as ``launch_trailer`` wrote them and writes the trailer form.
        Queued behind those launches on the same stream it needs no synchronisation in between.
        Device tensors, or raw device pointers; ``body`` needs no alignment."""
        if self._body_lengths is None:
            self._body_lengths = self.body_info()["body_lengths"]
        lens = self._body_lengths
        offs = None if body_offsets is None else _u64(body_offsets)
        if offs is not None and offs.shape != lens.shape:
            raise ValueError("body_offsets: one offset per part")
        need = int(lens.sum()) if offs is None else int((offs + lens).max())
        vb = self._value_bytes()
        args = [("data", data, _extent(self.offsets, self.lengths), 1),
                ("signatures", signatures, 32 * self.signatures, 4)]
        opt = [("checksums", checksums, vb * self.n, vb), ("trailer_signatures", trailer_signatures, 32 * self.n, 4)]
        ptrs = self._ptrs(*args) + [None if a[1] is None else self._ptrs(a)[0] for a in opt] + \
            self._ptrs(("body", body, need, 1))
        check(lib().s3h_chunk_plan_body(self._h, *ptrs, None if offs is None else _p64(offs),
                                        ctypes.c_void_p(_stream_handle(stream))))

    def status(self, stream=None) -> None:
        """Wait for ``stream``; raise if a chunk-hash launch since the last check reported a
        fault (s3h_chunk_plan_status)."""
        check(lib().s3h_chunk_plan_status(self._h, ctypes.c_void_p(_stream_handle(stream))))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().s3h_chunk_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def chunk_sign_batch_device(data, offsets, lengths, chunk_bytes: int, ctx: ChunkSignContext,
                            seeds) -> np.ndarray:
    """One-shot: plan, launch, copy back (s3h_chunk_sign_batch_device).  ``data`` is a device
    tensor, ``seeds`` host (n, 8) words; returns host (signatures, 8) uint32."""
    offs, lens = _u64(offsets), _u64(lengths)
    n = int(lens.size)
    sd = _words(seeds, n, "seeds")
    out = np.zeros((chunk_geometry(lens, chunk_bytes)["signatures"], 8), dtype=np.uint32)
    d_base = _device_buffer("data", data, _extent(offs, lens))
    check(lib().s3h_chunk_sign_batch_device(data.device.index or 0, ctx._h, d_base, _p64(offs), _p64(lens),
                                            n, int(chunk_bytes), sd.ctypes.data, out.ctypes.data))
    return out


def chunk_sign_host(parts: Sequence, chunk_bytes: int, ctx: ChunkSignContext, seeds) -> np.ndarray:
    """Host-resident parts: chunk digests through the host pipeline, the chain on the CPU
    (s3h_chunk_sign_batch_host).  Returns (signatures, 8) uint32, part-major."""
    arrs, ptrs, lens = _host_parts(parts)
    n = len(arrs)
    sd = _words(seeds, n, "seeds")
    out = np.zeros((chunk_geometry(lens, chunk_bytes)["signatures"], 8), dtype=np.uint32)
    check(lib().s3h_chunk_sign_batch_host(ctx._h, ptrs, _p64(lens), n, int(chunk_bytes),
                                          sd.ctypes.data, out.ctypes.data))
    return out


def _trailer_id(kind) -> int:
    if isinstance(kind, str):
        if kind not in _native.TRAILER_IDS:
            raise ValueError(f"unknown trailer checksum {kind!r} (one of {sorted(_native.TRAILER_IDS)})")
        return _native.TRAILER_IDS[kind]
    return int(kind)


def _trailer_values(kind, values, rows: int | None) -> np.ndarray:
    """(rows,) or (rows, words) array of checksum values in the layout of ``kind``."""
    dt, words = _native.TRAILER_VALUE[_trailer_id(kind)]
    if isinstance(values, (bytes, bytearray, memoryview)):
        values = np.frombuffer(values, dtype=np.uint8).view(dt)
    a = np.ascontiguousarray(np.atleast_1d(values)).astype(dt, copy=False).reshape(-1, words)
    if rows is not None and a.shape[0] != rows:
        raise ValueError(f"checksum values: {a.shape[0]} entries, expected {rows}")
    return a


def cpu_trailer_signatures(ctx: ChunkSignContext, checksum, values, last_signatures) -> np.ndarray:
    """The trailer link on the CPU (s3h_cpu_trailer_signatures): ``checksum`` "crc32c", "crc32",
    "crc64nvme", "sha1" or "sha256", ``values`` n checksums in that kind's layout (numbers for
    the CRCs, (n, 5) / (n, 8) words for the digests), ``last_signatures`` (n, 8): each part's
    last chunk signature.  Returns (n, 8) uint32."""
    last = _words(last_signatures, None, "last signatures")
    n = last.shape[0]
    vals = _trailer_values(checksum, values, n)
    out = np.zeros((n, 8), dtype=np.uint32)
    check(lib().s3h_cpu_trailer_signatures(ctx._h, _trailer_id(checksum), vals.ctypes.data,
                                           last.ctypes.data, n, out.ctypes.data))
    return out


def trailer_line_text(checksum, value) -> str:
    """The trailing header of one checksum value, "name:base64", no line end
    (s3h_trailer_line_text)."""
    vals = _trailer_values(checksum, value, 1)
    buf = ctypes.create_string_buffer(_native.TRAILER_LINE_MAX)
    check(lib().s3h_trailer_line_text(_trailer_id(checksum), vals.ctypes.data, buf, len(buf)))
    return buf.value.decode()


def chunk_trailer_text(checksum, value, trailer_signature) -> str:
    """What follows the "0;chunk-signature=...\r\n" line: the trailing header, the
    x-amz-trailer-signature line and the empty line (s3h_chunk_trailer_text)."""
    vals = _trailer_values(checksum, value, 1)
    sig = _words(trailer_signature, 1, "trailer signature")
    buf = ctypes.create_string_buffer(_native.CHUNK_TRAILER_MAX)
    check(lib().s3h_chunk_trailer_text(_trailer_id(checksum), vals.ctypes.data, sig.ctypes.data, buf,
                                       len(buf)))
    return buf.value.decode()


def _trailer_outputs(kind, lens, chunk_bytes: int):
    dt, words = _native.TRAILER_VALUE[_trailer_id(kind)]
    n = int(lens.size)
    sigs = np.zeros((chunk_geometry(lens, chunk_bytes)["signatures"], 8), dtype=np.uint32)
    vals = np.zeros(n if words == 1 else (n, words), dtype=dt)
    return sigs, vals, np.zeros((n, 8), dtype=np.uint32)


def chunk_sign_trailer_batch_device(data, offsets, lengths, chunk_bytes: int, ctx: ChunkSignContext,
                                    seeds, trailer: str = "crc32c"):
    """One-shot: trailer plan, launch, copy back (s3h_chunk_sign_trailer_batch_device).  Returns
    host (signatures, 8) uint32, the n checksums and (n, 8) uint32 trailer signatures."""
    offs, lens = _u64(offsets), _u64(lengths)
    n = int(lens.size)
    sd = _words(seeds, n, "seeds")
    sigs, vals, tsig = _trailer_outputs(trailer, lens, chunk_bytes)
    d_base = _device_buffer("data", data, _extent(offs, lens))
    check(lib().s3h_chunk_sign_trailer_batch_device(data.device.index or 0, ctx._h, _trailer_id(trailer),
                                                    d_base, _p64(offs),
                                                    _p64(lens), n, int(chunk_bytes), sd.ctypes.data,
                                                    sigs.ctypes.data, vals.ctypes.data, tsig.ctypes.data))
    return sigs, vals, tsig


def chunk_sign_trailer_host(parts: Sequence, chunk_bytes: int, ctx: ChunkSignContext, seeds,
                            trailer: str = "crc32c"):
    """Host-resident parts: chunk digests and chunk CRCs from one pass through the host pipeline,
    the CRCs folded per part, the chain and the trailer link on the CPU
    (s3h_chunk_sign_trailer_batch_host; "sha1" / "sha256" hash the whole parts in a second
    pass).  Returns (signatures, 8) uint32, the n checksums and (n, 8) trailer signatures."""
    arrs, ptrs, lens = _host_parts(parts)
    n = len(arrs)
    sd = _words(seeds, n, "seeds")
    sigs, vals, tsig = _trailer_outputs(trailer, lens, chunk_bytes)
    check(lib().s3h_chunk_sign_trailer_batch_host(ctx._h, _trailer_id(trailer), ptrs, _p64(lens), n,
                                                  int(chunk_bytes), sd.ctypes.data, sigs.ctypes.data,
                                                  vals.ctypes.data, tsig.ctypes.data))
    return sigs, vals, tsig


def _body_kind(checksum) -> int:
    return -1 if checksum is None else _trailer_id(checksum)


def chunk_body_geometry(lengths, chunk_bytes: int, checksum=None) -> dict:
    """Wire lengths of the aws-chunked bodies of parts of ``lengths`` cut at ``chunk_bytes``
    (s3h_chunk_body_geometry, no GPU): ``body_lengths[p]`` is the Content-Length of part p's
    request, ``body_offsets[p]`` where its body starts when they are packed back to back,
    ``total`` their sum.  ``checksum`` None, or the trailer's kind."""
    lens = _u64(lengths)
    n = int(lens.size)
    blen, boff = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    total = ctypes.c_uint64()
    check(lib().s3h_chunk_body_geometry(_p64(lens), n, int(chunk_bytes), _body_kind(checksum), _p64(blen),
                                        _p64(boff), ctypes.byref(total)))
    return {"n": n, "body_lengths": blen, "body_offsets": boff, "total": total.value}


def cpu_chunk_body(parts: Sequence, chunk_bytes: int, signatures, checksum=None, values=None,
                   trailer_signatures=None, out=None, body_offsets=None) -> np.ndarray:
    """The aws-chunked bodies of host-resident parts on the CPU (s3h_cpu_chunk_body):
    ``signatures`` as ``cpu_chunk_signatures`` returns them; with ``checksum`` also ``values``
    (n checksums in the kind's layout) and ``trailer_signatures`` (n, 8).  Part p's body goes to
    ``out[body_offsets[p]:]`` (a uint8 array; None: a new one) -- ``body_offsets`` None: packed
    back to back.  Returns ``out``."""
    arrs, ptrs, lens = _host_parts(parts)
    n = len(arrs)
    kind = _body_kind(checksum)
    sig = _words(signatures, None, "signatures")
    # (values without a kind: the library refuses them)
    vals = None if values is None else _trailer_values(kind, values, None) if kind >= 0 else np.ascontiguousarray(values)
    tsig = None if trailer_signatures is None else _words(trailer_signatures, None, "trailer signatures")
    offs = None if body_offsets is None else _u64(body_offsets)
    g = chunk_body_geometry(lens, chunk_bytes, checksum)
    need = g["total"] if offs is None else int((offs + g["body_lengths"]).max())
    if out is None:
        out = np.zeros(need, dtype=np.uint8)
    if out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < need:
        raise ValueError(f"out must be a contiguous uint8 array of at least {need} bytes")
    if sig.shape[0] != chunk_geometry(lens, chunk_bytes)["signatures"]:
        raise ValueError("signatures: one row per data chunk and one more per part")
    check(lib().s3h_cpu_chunk_body(ptrs, _p64(lens), n, int(chunk_bytes), sig.ctypes.data, kind,
                                   None if vals is None else vals.ctypes.data,
                                   None if tsig is None else tsig.ctypes.data, out.ctypes.data,
                                   None if offs is None else _p64(offs)))
    return out


def chunk_body_batch_device(data, offsets, lengths, chunk_bytes: int, ctx: ChunkSignContext, seeds,
                            trailer: str | None = None, out=None, body_offsets=None) -> np.ndarray:
    """One-shot: sign the chunks of device-resident parts and frame them on the device, then copy
    the bodies back (s3h_chunk_body_batch_device).  ``trailer`` None for the plain form, or
    "crc32c", "crc32", "crc64nvme".  Returns host uint8: the bodies packed back to back, or at
    ``body_offsets`` in ``out``."""
    offs, lens = _u64(offsets), _u64(lengths)
    n = int(lens.size)
    sd = _words(seeds, n, "seeds")
    boffs = None if body_offsets is None else _u64(body_offsets)
    g = chunk_body_geometry(lens, chunk_bytes, trailer)
    need = g["total"] if boffs is None else int((boffs + g["body_lengths"]).max())
    if out is None:
        out = np.zeros(need, dtype=np.uint8)
    if out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < need:
        raise ValueError(f"out must be a contiguous uint8 array of at least {need} bytes")
    d_base = _device_buffer("data", data, _extent(offs, lens))
    check(lib().s3h_chunk_body_batch_device(data.device.index or 0, ctx._h, _body_kind(trailer), d_base,
                                            _p64(offs), _p64(lens), n, int(chunk_bytes), sd.ctypes.data,
                                            out.ctypes.data, None if boffs is None else _p64(boffs)))
    return out


class Crc64Plan(CrcPlan):
    """CrcPlan for CRC-64/NVME (x-amz-checksum-crc64nvme; s3h_crc64nvme_plan_create): the same
    ``launch`` / ``launch_range`` / ``info``, with ``crcs`` holding n 64-bit words."""

    _prefix = "s3h_crc64nvme_plan_"
    _value_bytes = 8

    def _create(self, h) -> int:
        return lib().s3h_crc64nvme_plan_create(self.device, _p64(self.offsets), _p64(self.lengths),
                                               self.n, ctypes.byref(h))

    def __init__(self, offsets: Sequence[int], lengths: Sequence[int], device: int = 0):
        self.crc = _native.CRC64NVME
        self.offsets, self.lengths = _u64(offsets), _u64(lengths)
        if self.offsets.shape != self.lengths.shape or self.offsets.ndim != 1:
            raise ValueError("offsets and lengths must be 1-D and of equal length")
        self.n = int(self.lengths.size)
        self.device = device
        h = ctypes.c_void_p()
        check(self._create(h))
        self._h = h


def crc64_batch_device(data, offsets, lengths, stream=None):
    """CRC-64/NVME of every part [offsets[i], offsets[i]+lengths[i]) of the device tensor
    ``data`` (any byte alignment): an (n,) int64 device tensor holding the uint64 values
    (``.cpu().numpy().view(np.uint64)``).  Blocking."""
    import torch
    offs, lens = _u64(offsets), _u64(lengths)
    d_base = _device_buffer("data", data, _extent(offs, lens))
    dev = data.device.index
    out = torch.empty(offs.size, dtype=torch.int64, device=data.device)
    check(lib().s3h_crc64nvme_batch_device(dev, d_base, _p64(offs), _p64(lens), offs.size,
                                           _device_buffer("crcs", out, 8 * offs.size, dev, align=8),
                                           ctypes.c_void_p(_stream_handle(stream))))
    return out


def crc64_verify_batch_device(data, offsets, lengths, expected, stream=None):
    """Device-resident verification against ``expected`` (n 64-bit words, device): returns
    (mismatch count, bool mask on the device)."""
    import torch
    offs, lens = _u64(offsets), _u64(lengths)
    d_base = _device_buffer("data", data, _extent(offs, lens))
    dev = data.device.index
    d_exp = _device_buffer("expected", expected, 8 * offs.size, dev, align=4)
    mism = torch.zeros(offs.size, dtype=torch.uint8, device=data.device)
    cnt = ctypes.c_uint64(0)
    check(lib().s3h_crc64nvme_verify_batch_device(dev, d_base, _p64(offs), _p64(lens), offs.size,
                                                  d_exp,
                                                  _device_buffer("mask", mism, offs.size, dev),
                                                  ctypes.byref(cnt),
                                                  ctypes.c_void_p(_stream_handle(stream))))
    return cnt.value, mism.bool()


def crc64_batch_host(parts: Sequence, ndevices: int = 0, slice_bytes: int = 0) -> np.ndarray:
    """CRC-64/NVME of host-resident parts on the GPUs (s3h_crc64nvme_batch_host): (n,) uint64."""
    arrs, ptrs, lens = _host_parts(parts)
    n = len(arrs)
    out = np.zeros(n, dtype=np.uint64)
    check(lib().s3h_crc64nvme_batch_host(ptrs, _p64(lens), n, out.ctypes.data, ndevices, slice_bytes))
    return out


def sha256_crc64_batch_host(parts: Sequence, ndevices: int = 0,
                            slice_bytes: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """SHA-256 (n, 8) digests and CRC-64/NVME values (n,) uint64 of host-resident parts, each
    part crossing PCIe once (s3h_sha256_crc64nvme_batch_host)."""
    arrs, ptrs, lens = _host_parts(parts)
    n = len(arrs)
    sha = np.zeros((n, DIGEST_WORDS), dtype=np.uint32)
    out = np.zeros(n, dtype=np.uint64)
    check(lib().s3h_sha256_crc64nvme_batch_host(ptrs, _p64(lens), n, sha.ctypes.data,
                                                out.ctypes.data, ndevices, slice_bytes))
    return sha, out


def sha256_crc64_file_parts(path: str, offsets, lengths, ndevices: int = 0,
                            slice_bytes: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """SHA-256 (n, 8) digests and CRC-64/NVME values (n,) of file ranges, each slice read once
    (s3h_sha256_crc64nvme_file_parts)."""
    offs, lens = _u64(offsets), _u64(lengths)
    if offs.shape != lens.shape or offs.ndim != 1 or offs.size == 0:
        raise ValueError("offsets and lengths must be 1-D, equal length and non-empty")
    sha = np.zeros((offs.size, DIGEST_WORDS), dtype=np.uint32)
    out = np.zeros(offs.size, dtype=np.uint64)
    check(lib().s3h_sha256_crc64nvme_file_parts(os.fsencode(path), _p64(offs), _p64(lens), offs.size,
                                                sha.ctypes.data, out.ctypes.data, ndevices,
                                                slice_bytes))
    return sha, out


_M64 = 0xFFFFFFFFFFFFFFFF


def crc64(data, seed: int = 0) -> int:
    """CPU CRC-64/NVME of one message (s3h_cpu_crc64nvme); ``seed`` = a previous call's result,
    so chunks chain."""
    a = _as_bytes(data) if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), dtype=np.uint8)
    return int(lib().s3h_cpu_crc64nvme(ctypes.c_void_p(a.ctypes.data if a.size else None), a.size,
                                       seed & _M64))


def crc64_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """crc(A || B) from crc(A), crc(B) and len(B) (s3h_crc64nvme_combine)."""
    out = ctypes.c_uint64()
    check(lib().s3h_crc64nvme_combine(crc_a & _M64, crc_b & _M64, int(len_b), ctypes.byref(out)))
    return out.value


def crc64_object(part_crcs, lengths) -> int:
    """FULL_OBJECT x-amz-checksum-crc64nvme value of the parts' concatenation from their CRCs
    and lengths (s3h_crc64nvme_object)."""
    if isinstance(part_crcs, np.ndarray) and part_crcs.dtype == np.int64:
        part_crcs = part_crcs.view(np.uint64)  # (the int64 view of a device tensor's values)
    w = np.ascontiguousarray(np.asarray(part_crcs, dtype=np.uint64)).reshape(-1)
    lens = _u64(lengths)
    if lens.shape != w.shape:
        raise ValueError("one length per part checksum")
    out = ctypes.c_uint64()
    check(lib().s3h_crc64nvme_object(ctypes.c_void_p(w.ctypes.data), _p64(lens), w.size,
                                     ctypes.byref(out)))
    return out.value


def checksum64_text(crc: int) -> str:
    """Header text of a 64-bit checksum (s3h_checksum64_text): base64 of its 8 big-endian bytes."""
    out = ctypes.create_string_buffer(_native.CHECKSUM_MAX)
    check(lib().s3h_checksum64_text(int(crc) & _M64, out, len(out)))
    return out.value.decode()


def multipart_etag(part_md5s) -> str:
    """S3 multipart ETag: hex(MD5(concatenated binary part MD5s)) + "-" + part count
    (s3h_multipart_etag; the outer MD5, 16 B per part, runs on the lib/hash MD5 drop-in)."""
    w = np.ascontiguousarray(part_md5s, dtype=np.uint32).reshape(-1, 4)
    out = ctypes.create_string_buffer(56)
    check(lib().s3h_multipart_etag(w.ctypes.data, w.shape[0], out, len(out)))
    return out.value.decode()


class Stream:
    """n messages (objects) hashed incrementally on the GPU as chunks arrive
    (s3h_stream_*, include/s3hash.h): sha256_stream semantics per append and the documented
    sha256_next contract (lib/hash/sha256.h:73-89) at ``final()`` -- the digest of the
    concatenation of every chunk appended since the previous ``final()``.

    ``update(chunks)`` takes one chunk per message: host ``bytes``/numpy arrays or
    ``BufferParts`` (returns once the chunks are copied; the hash overlaps the next update and
    ``final()`` reports a device fault of any of them), or, with ``update_device``, a device
    tensor plus offsets/lengths (asynchronous)."""

    def __init__(self, n: int, device: int = 0, algo: str = "sha256", kernel: str | int = "auto"):
        k = kernel if isinstance(kernel, int) else _native.KERNEL_IDS[kernel]
        self.algo = _native.ALGO_IDS[algo]
        self.words = _native.DIGEST_WORDS[self.algo]
        self.n, self.device = int(n), device
        h = ctypes.c_void_p()
        check(lib().s3h_stream_create(device, self.algo, self.n, k, ctypes.byref(h)))
        self._h = h

    def update(self, chunks: Sequence) -> None:
        if len(chunks) != self.n:
            raise ValueError(f"need one chunk per message ({self.n})")
        arrs, ptrs, lens = _host_parts(chunks)
        check(lib().s3h_stream_update_host(self._h, ptrs, _p64(lens)))

    def update_device(self, data, offsets, lengths, stream=None) -> None:
        offs, lens = _u64(offsets), _u64(lengths)
        if offs.size != self.n or lens.size != self.n:
            raise ValueError(f"need one chunk per message ({self.n})")
        end = int((offs + lens)[lens > 0].max()) if lens.any() else 0
        check(lib().s3h_stream_update_device(self._h, _device_buffer("data", data, end, self.device),
                                             _p64(offs), _p64(lens),
                                             ctypes.c_void_p(_stream_handle(stream))))

    def final(self) -> np.ndarray:
        """(n, words) uint32 digests; the object restarts with n empty messages."""
        out = np.zeros((self.n, self.words), dtype=np.uint32)
        check(lib().s3h_stream_final_host(self._h, out.ctypes.data))
        return out

    def final_device(self, digests, stream=None) -> None:
        d_dig = _device_buffer("digests", digests, 4 * self.words * self.n, self.device,
                               align=_digest_align(self.algo))
        check(lib().s3h_stream_final_device(self._h, d_dig,
                                            ctypes.c_void_p(_stream_handle(stream))))

    def status(self, stream=None) -> None:
        """Wait for ``stream``; raise if an update/final launch reported a fault
        (s3h_stream_status).  The host forms check by themselves."""
        check(lib().s3h_stream_status(self._h, ctypes.c_void_p(_stream_handle(stream))))

    def stats(self) -> dict:
        """How updates found their plans' device slots (s3h_stream_stats): reused in place
        (equal chunks appended at a moved base) or re-sorted and uploaded."""
        r, f = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().s3h_stream_stats(self._h, ctypes.byref(r), ctypes.byref(f)))
        return {"slot_reuses": r.value, "slot_refills": f.value}

    def total(self, i: int) -> int:
        t = ctypes.c_uint64()
        check(lib().s3h_stream_total(self._h, i, ctypes.byref(t)))
        return t.value

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().s3h_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def sha256_batch_host(parts: Sequence, ndevices: int = 0, slice_bytes: int = 0) -> np.ndarray:
    """Digest host-resident parts (bytes / numpy uint8 arrays) on the GPUs: (n, 8) uint32."""
    return _host_batch(lib().s3h_sha256_batch_host, DIGEST_WORDS, parts, ndevices, slice_bytes)


def sha256_batch_host_on(parts: Sequence, devices: Sequence[int], slice_bytes: int = 0) -> np.ndarray:
    """sha256_batch_host over an explicit device list (shard k = parts i % len(devices) == k on
    devices[k]; repeats allowed): s3h_sha256_batch_host_on."""
    arrs, ptrs, lens = _host_parts(parts)
    n = len(arrs)
    out = np.zeros((n, DIGEST_WORDS), dtype=np.uint32)
    devs = (ctypes.c_int * len(devices))(*devices)
    check(lib().s3h_sha256_batch_host_on(ptrs, _p64(lens), n, out.ctypes.data, devs, len(devices),
                                         slice_bytes))
    return out


def sha256_file_parts(path: str, offsets, lengths, ndevices: int = 0,
                      slice_bytes: int = 0) -> np.ndarray:
    """Digests of byte ranges [offsets[i], offsets[i]+lengths[i]) of a file, read by host
    threads straight into the pinned staging ring (s3h_sha256_file_parts): the (file, offset,
    size) parts of S3Api::UploadFilePart.  (n, 8) uint32."""
    offs, lens = _u64(offsets), _u64(lengths)
    if offs.shape != lens.shape or offs.ndim != 1 or offs.size == 0:
        raise ValueError("offsets and lengths must be 1-D, equal length and non-empty")
    out = np.zeros((offs.size, DIGEST_WORDS), dtype=np.uint32)
    check(lib().s3h_sha256_file_parts(os.fsencode(path), _p64(offs), _p64(lens), offs.size,
                                      out.ctypes.data, ndevices, slice_bytes))
    return out


def sha256_md5_file_parts(path: str, offsets, lengths, ndevices: int = 0,
                          slice_bytes: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """SHA-256 (n, 8) and MD5 (n, 4) uint32 digests of file ranges, each slice read once
    (s3h_sha256_md5_file_parts): x-amz-content-sha256 and Content-MD5 of UploadFilePart parts."""
    offs, lens = _u64(offsets), _u64(lengths)
    if offs.shape != lens.shape or offs.ndim != 1 or offs.size == 0:
        raise ValueError("offsets and lengths must be 1-D, equal length and non-empty")
    sha = np.zeros((offs.size, DIGEST_WORDS), dtype=np.uint32)
    m5 = np.zeros((offs.size, 4), dtype=np.uint32)
    check(lib().s3h_sha256_md5_file_parts(os.fsencode(path), _p64(offs), _p64(lens), offs.size,
                                          sha.ctypes.data, m5.ctypes.data, ndevices, slice_bytes))
    return sha, m5


def route_model() -> dict:
    """The size-aware routing model's rates, measured once per process on this host and GPU
    (s3h_route_model): per-thread CPU drop-in rate, one GPU chain's rate, pinned H2D rate,
    fixed GPU call cost, CPU threads, devices.  Raises S3HashError without a GPU."""
    m = _native.RouteModel()
    check(lib().s3h_route_model(ctypes.byref(m)))
    return {f: getattr(m, f) for f, _ in m._fields_}


def route_estimate(lengths, model: dict, ndevices: int = 0, pinned: bool = True,
                   source: str | None = None) -> tuple[str, float, float]:
    """AUTO's choice for a batch of parts of ``lengths`` under ``model`` (any dict with
    route_model()'s fields; pure host arithmetic, s3h_route_estimate_ex): (route, gpu_s,
    cpu_s).  ``source``: "pinned", "pageable" or "file" (default: pinned or pageable by
    ``pinned``) -- pageable parts and file ranges feed the GPU at min(h2d, staged)."""
    m = _native.RouteModel(**model)
    lens = _u64(lengths)
    src = _native.SOURCE_IDS[source or ("pinned" if pinned else "pageable")]
    g, c = ctypes.c_double(), ctypes.c_double()
    r = lib().s3h_route_estimate_ex(ctypes.byref(m), _p64(lens), lens.size, ndevices, src,
                                    ctypes.byref(g), ctypes.byref(c))
    if r < 0:
        check(r)
    return _native.ROUTE_NAMES[r], g.value, c.value


def route_split_estimate(lengths, model: dict, ndevices: int = 0,
                         source: str = "pinned") -> tuple[int, int, float]:
    """The split route's plan under ``model`` (s3h_route_split_estimate, pure host arithmetic):
    (m, tg, split_s) -- the m longest parts on the CPU, the rest on the GPU with tg staging
    threads per device (0 for pinned parts), estimated split_s seconds."""
    m = _native.RouteModel(**model)
    lens = _u64(lengths)
    k, tg, t = ctypes.c_uint64(), ctypes.c_int(), ctypes.c_double()
    check(lib().s3h_route_split_estimate(ctypes.byref(m), _p64(lens), lens.size, ndevices,
                                         _native.SOURCE_IDS[source], ctypes.byref(k), ctypes.byref(tg),
                                         ctypes.byref(t)))
    return k.value, tg.value, t.value


def sha256_batch_routed(parts: Sequence, ndevices: int = 0, route: str = "auto") -> tuple[np.ndarray, str]:
    """Host-resident parts hashed on the route given -- "gpu" (= sha256_batch_host), "cpu" (the
    lib/hash drop-in on host threads), "split" (the longest parts on the CPU, the rest on the
    GPU, at once) or "auto" (whichever the measured model says finishes first; needs a GPU) --
    s3h_sha256_batch_routed.  Returns ((n, 8) uint32, route taken)."""
    arrs, ptrs, lens = _host_parts(parts)
    out = np.zeros((len(arrs), DIGEST_WORDS), dtype=np.uint32)
    taken = ctypes.c_int(-1)
    check(lib().s3h_sha256_batch_routed(ptrs, _p64(lens), len(arrs), out.ctypes.data, ndevices,
                                        _native.ROUTE_IDS[route], ctypes.byref(taken)))
    return out, _native.ROUTE_NAMES[taken.value]


def sha256_file_parts_routed(path: str, offsets, lengths, ndevices: int = 0,
                             route: str = "auto") -> tuple[np.ndarray, str]:
    """File ranges on the route given (s3h_sha256_file_parts_routed): ((n, 8) uint32, taken)."""
    offs, lens = _u64(offsets), _u64(lengths)
    if offs.shape != lens.shape or offs.ndim != 1 or offs.size == 0:
        raise ValueError("offsets and lengths must be 1-D, equal length and non-empty")
    out = np.zeros((offs.size, DIGEST_WORDS), dtype=np.uint32)
    taken = ctypes.c_int(-1)
    check(lib().s3h_sha256_file_parts_routed(os.fsencode(path), _p64(offs), _p64(lens), offs.size,
                                             out.ctypes.data, ndevices, _native.ROUTE_IDS[route],
                                             ctypes.byref(taken)))
    return out, _native.ROUTE_NAMES[taken.value]


def md5_batch_routed(parts: Sequence, ndevices: int = 0, route: str = "auto") -> tuple[np.ndarray, str]:
    """Content-MD5 of host parts on a route (s3h_md5_batch_routed): ((n, 4) uint32, taken)."""
    arrs, ptrs, lens = _host_parts(parts)
    out = np.zeros((len(arrs), 4), dtype=np.uint32)
    taken = ctypes.c_int(-1)
    check(lib().s3h_md5_batch_routed(ptrs, _p64(lens), len(arrs), out.ctypes.data, ndevices,
                                     _native.ROUTE_IDS[route], ctypes.byref(taken)))
    return out, _native.ROUTE_NAMES[taken.value]


def sha256_md5_batch_routed(parts: Sequence, ndevices: int = 0,
                            route: str = "auto") -> tuple[np.ndarray, np.ndarray, str]:
    """x-amz-content-sha256 AND Content-MD5 of host parts on a route -- "gpu" (one grid, one
    PCIe pass: sha256_md5_batch_host), "cpu" (both digests per part in one pass over memory),
    "split" or "auto" (priced with the dual rates) -- s3h_sha256_md5_batch_routed.  Returns
    ((n, 8) SHA-256 words, (n, 4) MD5 words, route taken)."""
    arrs, ptrs, lens = _host_parts(parts)
    sha = np.zeros((len(arrs), DIGEST_WORDS), dtype=np.uint32)
    m5 = np.zeros((len(arrs), 4), dtype=np.uint32)
    taken = ctypes.c_int(-1)
    check(lib().s3h_sha256_md5_batch_routed(ptrs, _p64(lens), len(arrs), sha.ctypes.data,
                                            m5.ctypes.data, ndevices, _native.ROUTE_IDS[route],
                                            ctypes.byref(taken)))
    return sha, m5, _native.ROUTE_NAMES[taken.value]


def sha256_md5_file_parts_routed(path: str, offsets, lengths, ndevices: int = 0,
                                 route: str = "auto") -> tuple[np.ndarray, np.ndarray, str]:
    """Both digests of file ranges on a route (s3h_sha256_md5_file_parts_routed)."""
    offs, lens = _u64(offsets), _u64(lengths)
    if offs.shape != lens.shape or offs.ndim != 1 or offs.size == 0:
        raise ValueError("offsets and lengths must be 1-D, equal length and non-empty")
    sha = np.zeros((offs.size, DIGEST_WORDS), dtype=np.uint32)
    m5 = np.zeros((offs.size, 4), dtype=np.uint32)
    taken = ctypes.c_int(-1)
    check(lib().s3h_sha256_md5_file_parts_routed(os.fsencode(path), _p64(offs), _p64(lens),
                                                 offs.size, sha.ctypes.data, m5.ctypes.data,
                                                 ndevices, _native.ROUTE_IDS[route],
                                                 ctypes.byref(taken)))
    return sha, m5, _native.ROUTE_NAMES[taken.value]


def md5_file_parts(path: str, offsets, lengths, ndevices: int = 0, slice_bytes: int = 0) -> np.ndarray:
    """Content-MD5 of file ranges on the GPU (s3h_md5_file_parts): (n, 4) uint32."""
    offs, lens = _u64(offsets), _u64(lengths)
    if offs.shape != lens.shape or offs.ndim != 1 or offs.size == 0:
        raise ValueError("offsets and lengths must be 1-D, equal length and non-empty")
    out = np.zeros((offs.size, 4), dtype=np.uint32)
    check(lib().s3h_md5_file_parts(os.fsencode(path), _p64(offs), _p64(lens), offs.size,
                                   out.ctypes.data, ndevices, slice_bytes))
    return out


def route_rates() -> dict:
    """The whole routing model -- per digest set (index 0 SHA-256, 1 MD5, 2 both) the one-thread
    and all-threads CPU rates and the GPU chain rate, H2D / staging rates, call cost, the
    observed GPU / CPU factors, measurement and divergence counters (s3h_route_rates; measures
    what is missing).  Lists for the per-digest-set arrays."""
    r = _native.RouteRates()
    r.size = ctypes.sizeof(r)
    check(lib().s3h_route_rates(ctypes.byref(r)))
    out = {}
    for f, _ in r._fields_:
        v = getattr(r, f)
        out[f] = list(v) if isinstance(v, ctypes.Array) else v
    return out


def route_choose(lengths, rates: dict, digests: str = "sha256", ndevices: int = 0,
                 source: str = "pinned") -> dict:
    """AUTO's decision under ``rates`` (route_rates()'s dict, possibly edited; pure host
    arithmetic, s3h_route_choose): route, gpu_s, cpu_s, split_s, cpu_parts, stage_threads."""
    r = _native.RouteRates()
    for f, _ in r._fields_:
        if f in rates:
            v = rates[f]
            if isinstance(v, (list, tuple)):
                arr = getattr(r, f)
                for i, x in enumerate(v):
                    arr[i] = x
            else:
                setattr(r, f, v)
    r.size = ctypes.sizeof(r)
    lens = _u64(lengths)
    c = _native.RouteChoice()
    check(lib().s3h_route_choose(ctypes.byref(r), _native.DIGESTS_IDS[digests], _p64(lens), lens.size,
                                 ndevices, _native.SOURCE_IDS[source], ctypes.byref(c)))
    return {"route": _native.ROUTE_NAMES[c.route], "gpu_s": c.gpu_s, "cpu_s": c.cpu_s,
            "split_s": c.split_s, "cpu_parts": c.cpu_parts, "stage_threads": c.stage_threads}


def route_device_rates(device: int, digests: str = "sha256") -> tuple[float, float]:
    """(lone-chain bytes/s, pinned H2D bytes/s) of one device (s3h_route_device_rates)."""
    ch, h = ctypes.c_double(), ctypes.c_double()
    check(lib().s3h_route_device_rates(device, _native.DIGESTS_IDS[digests], ctypes.byref(ch),
                                       ctypes.byref(h)))
    return ch.value, h.value


def route_refresh_calls(calls: int) -> int:
    """Re-measure the routing model every ``calls`` AUTO/SPLIT calls (0: only on divergence);
    returns the previous setting (s3h_route_refresh_calls)."""
    prev = ctypes.c_int(0)
    check(lib().s3h_route_refresh_calls(int(calls), ctypes.byref(prev)))
    return prev.value


def route_scale(rate: str, factor: float) -> None:
    """Test hook: multiply one measured rate ("chain", "h2d", "cpu", "staged") by ``factor``
    until the model is next measured (s3h_route_scale)."""
    check(lib().s3h_route_scale(_native.RATE_IDS[rate], float(factor)))


def host_plan(pci_bus_ids, affinity: str | None = None, cpu_quota: float = -1.0) -> dict:
    """The host path's thread plan for a call over the devices at ``pci_bus_ids`` (None
    entries: no NUMA record) -- per-device staging threads, bind node and CPUs, split-route
    thread shares, oversubscription flags -- with the CPUs of ``affinity`` (a cpulist; None:
    this process) under a ``cpu_quota`` (0: none; < 0: this process's cgroup): s3h_host_plan,
    pure host arithmetic over sysfs (S3H_SYSFS_ROOT)."""
    n = len(pci_bus_ids)
    ids = (ctypes.c_char_p * n)(*[None if b is None else b.encode() for b in pci_bus_ids])
    plan = _native.HostPlan()
    devs = (_native.HostPlanDevice * n)()
    check(lib().s3h_host_plan(ids, n, None if affinity is None else affinity.encode(),
                              float(cpu_quota), ctypes.byref(plan), devs))
    out = {f: getattr(plan, f) for f, _ in plan._fields_}
    out["per_device"] = [{f: getattr(d, f) for f, _ in d._fields_} for d in devs]
    return out


def host_threads(ndevices: int = 1) -> tuple[int, int]:
    """(staging threads per device when ``ndevices`` device shards run at once, CPUs this
    process may use: affinity capped by the cgroup quota) -- s3h_host_threads."""
    cpus = ctypes.c_int(0)
    per = lib().s3h_host_threads(ndevices, ctypes.byref(cpus))
    return per, cpus.value


def pci_numa(pci_bus_id: str) -> dict:
    """sysfs NUMA record of a PCI function (s3h_pci_numa; no GPU needed): node, local CPU
    list and how many of those CPUs this thread may run on."""
    node, usable = ctypes.c_int(-1), ctypes.c_int(0)
    buf = ctypes.create_string_buffer(4096)
    check(lib().s3h_pci_numa(pci_bus_id.encode(), ctypes.byref(node), buf, len(buf),
                             ctypes.byref(usable)))
    return {"node": node.value, "local_cpulist": buf.value.decode(), "usable_cpus": usable.value}


def device_numa(device: int) -> dict:
    """NUMA node and local CPU list of HIP device ``device`` (s3h_device_numa_node)."""
    node = ctypes.c_int(-1)
    buf = ctypes.create_string_buffer(4096)
    check(lib().s3h_device_numa_node(device, ctypes.byref(node), buf, len(buf)))
    return {"node": node.value, "local_cpulist": buf.value.decode()}


def host_numa(mode) -> int:
    """Set the host path's placement policy -- "local" (each device's node, the default), "off"
    (runtime placement, unbound threads) or a node number -- and return the previous mode
    (-1 local, -2 off, else a node): s3h_host_numa."""
    m = {"local": _native.NUMA_LOCAL, "off": _native.NUMA_OFF}.get(mode, mode)
    prev = ctypes.c_int(0)
    check(lib().s3h_host_numa(int(m), ctypes.byref(prev)))
    return prev.value


def host_numa_info(device: int) -> dict:
    """Where the host path places device ``device``'s staging and copy threads, and what its
    cached context holds (s3h_host_numa_info)."""
    info = _native.HostNuma()
    check(lib().s3h_host_numa_info(device, ctypes.byref(info)))
    return {f: getattr(info, f) for f, _ in info._fields_}


def mem_node(buf) -> int:
    """NUMA node of the page holding the start of ``buf`` (numpy array, CPU torch tensor or an
    address): s3h_mem_node."""
    addr = buf if isinstance(buf, int) else (buf.data_ptr() if hasattr(buf, "data_ptr")
                                             else _as_bytes(buf).ctypes.data)
    node = ctypes.c_int(-1)
    check(lib().s3h_mem_node(ctypes.c_void_p(addr), ctypes.byref(node)))
    return node.value


class PinnedBuffer:
    """Pinned host memory on a NUMA node (s3h_host_alloc; node -1 = the runtime's placement),
    e.g. an uploader's read buffer on its device's node.  ``array`` is a uint8 numpy view (it
    keeps the buffer alive); the memory is freed when the last view is gone or on close()."""

    def __init__(self, nbytes: int, node: int = -1, strict: bool = False):
        import weakref
        p = ctypes.c_void_p()
        flags = _native.HOST_ALLOC_STRICT if strict else 0
        check(lib().s3h_host_alloc_ex(int(node), int(nbytes), flags, ctypes.byref(p)))
        self.ptr, self.nbytes, self.node = p.value, int(nbytes), int(node)
        raw = (ctypes.c_uint8 * self.nbytes).from_address(self.ptr)
        # freed once the ctypes array -- held by this object and by every numpy view -- is gone
        self._free = weakref.finalize(raw, lib().s3h_host_free, ctypes.c_void_p(self.ptr))
        self.array = np.frombuffer(raw, dtype=np.uint8)

    def close(self) -> None:
        """Free now (no view of ``array`` may be used afterwards)."""
        self.array = None
        self._free()


def dual_layout(lengths, cus: int = 256) -> tuple[int, bool]:
    """(skew groups of the SHA-256 + MD5 mixed grid, MD5 apart?) for a batch of ``lengths`` on
    a device of ``cus`` CUs -- the rule a plan applies, on the host (s3h_dual_layout)."""
    lens = _u64(lengths)
    solo, apart = ctypes.c_uint32(), ctypes.c_int()
    check(lib().s3h_dual_layout(_p64(lens), lens.size, cus, ctypes.byref(solo), ctypes.byref(apart)))
    return solo.value, bool(apart.value)


def kernel_policy(policy: str) -> str:
    """AUTO's kernel policy for plans created afterwards -- "throughput" (skews for 4,097 -
    32 x CUs parts), "efficiency" (skewp there: ~5 % slower, ~36 % fewer joules per GiB) or
    "power" (the default: skews only when the board's power cap lets it hold its clock) --
    returns the previous one (s3h_kernel_policy)."""
    prev = ctypes.c_int(0)
    check(lib().s3h_kernel_policy(_native.POLICY_IDS[policy], ctypes.byref(prev)))
    return _native.POLICY_NAMES[prev.value]


def device_power_cap(device: int = 0) -> float:
    """Board power cap of ``device`` in watts as the "power" kernel policy reads it (sysfs hwmon
    power1_cap; 0.0 when the platform does not say): s3h_device_power_cap."""
    w = ctypes.c_double(0)
    check(lib().s3h_device_power_cap(device, ctypes.byref(w)))
    return w.value


def pci_power_cap(pci_bus_id: str) -> float:
    """Board power cap in watts of the PCI function (sysfs hwmon power1_cap; 0.0 when absent;
    no GPU needed): s3h_pci_power_cap."""
    w = ctypes.c_double(0)
    check(lib().s3h_pci_power_cap(pci_bus_id.encode(), ctypes.byref(w)))
    return w.value


def trim() -> None:
    """Free the host path's cached per-device buffers (HBM ring, pinned staging, plans):
    s3h_trim.  A process that shares the GPU with other work calls this when it is done."""
    check(lib().s3h_trim())


def generate_parts(data, offsets, lengths, part_ids, seed: int, stream=None) -> None:
    """Fill parts of device tensor ``data`` with generator G(seed, part_id, length)."""
    offs, lens, ids = _u64(offsets), _u64(lengths), _u64(part_ids)
    d_base = _device_buffer("data", data, _extent(offs, lens), align=8)
    dev = data.device.index
    for s in range(0, offs.size, 65535):
        e = min(offs.size, s + 65535)
        check(lib().s3h_generate_parts(dev, d_base, _p64(offs[s:e]),
                                       _p64(lens[s:e]), _p64(ids[s:e]), e - s, seed,
                                       ctypes.c_void_p(_stream_handle(stream))))


# ------------------------------------------------------------------ CPU drop-in (lib/hash)
def sha256(data: bytes) -> np.ndarray:
    """lib/hash sha256::sha256 (CPU, single message): 8 words, hash[i] = bswap32(H_i)."""
    b = bytes(data)
    out = np.zeros(DIGEST_WORDS, dtype=np.uint32)
    lib().s3h_cpu_sha256(b, len(b), out.ctypes.data)
    return out


def md5(data: bytes) -> np.ndarray:
    """lib/hash md5 drop-in (CPU, single message, padded): 4 words, LE digest bytes."""
    b = bytes(data)
    out = np.zeros(4, dtype=np.uint32)
    lib().s3h_cpu_md5(b, len(b), out.ctypes.data)
    return out


def hmac256(data: bytes, key: bytes) -> bytes:
    out = ctypes.create_string_buffer(32)
    d, k = bytes(data), bytes(key)
    lib().s3h_cpu_hmac256(d, len(d), k, len(k), out)
    return out.raw


def hash_to_text(words) -> str:
    """sha256::hash_to_text / md5::hash_to_text: lowercase hex of the digest bytes in memory."""
    return np.ascontiguousarray(words, dtype=np.uint32).reshape(-1).tobytes().hex()


def digests_to_text(words, nwords: int = DIGEST_WORDS) -> list[str]:
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, nwords)
    return [row.tobytes().hex() for row in w]


def cpu_backend() -> str:
    return lib().s3h_cpu_backend().decode()
