"""SHA-256 + CRC-64/NVME (and the CRC alone) of host-resident parts from one pass through the host
pipeline (s3h_sha256_crc64nvme_batch_host, s3h_crc64nvme_batch_host,
s3h_sha256_crc64nvme_file_parts): every copy mode of the slice and group pipelines, at the sizes
of tests/test_gpu_crc_host.py.  Expected values: s3h_cpu_crc64nvme (pinned by
tests/test_crc64_cpu.py) and hashlib.sha256 (the 32 digest bytes in memory)."""
import hashlib
import threading

import numpy as np
import pytest

import s3client_amd as s3

pytestmark = pytest.mark.gpu
MIB = 1 << 20


class Batch:
    """Parts of one buffer (a numpy view of it, offsets, lengths) and their expected values."""

    def __init__(self, host, offs, lens):
        self.host = host
        self.offs = np.asarray(offs, dtype=np.uint64)
        self.lens = np.asarray(lens, dtype=np.uint64)
        views = [host[int(o):int(o) + int(n)] for o, n in zip(self.offs, self.lens)]
        self.sha = np.frombuffer(b"".join(hashlib.sha256(v.tobytes()).digest() for v in views),
                                 dtype=np.uint32).reshape(-1, 8)
        self.crc = np.array([s3.crc64(v) for v in views], dtype=np.uint64)

    def parts(self, buf=None, k=None):
        return s3.BufferParts(self.host if buf is None else buf, self.offs[:k], self.lens[:k])

    def check(self, sha, crcs, k=None):
        want = self.crc[:k]
        assert crcs.dtype == np.uint64 and crcs.shape == want.shape
        bad = np.flatnonzero(crcs != want)
        assert bad.size == 0, [(int(i), int(self.lens[i]), hex(crcs[i]), hex(want[i])) for i in bad[:8]]
        if sha is not None:
            bad = np.flatnonzero((sha != self.sha[:k]).any(axis=1))
            assert bad.size == 0, ("sha256", [(int(i), int(self.lens[i])) for i in bad[:8]])

    def check_dual(self, parts, k=None, **kw):
        sha, crcs = s3.sha256_crc64_batch_host(parts, **kw)
        self.check(sha, crcs, k)


def _ragged(lens, gap=0):
    lens = np.asarray(lens, dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens + np.uint64(gap))[:-1]]).astype(np.uint64)
    return offs, lens, int(offs[-1] + lens[-1]) + 64


def _pinned(torch, size, rng):
    t = torch.empty(size, dtype=torch.uint8, pin_memory=True)
    t.numpy()[:] = rng.integers(0, 256, size, dtype=np.uint8)
    return t


@pytest.fixture(scope="module")
def pageable_ragged():
    rng = np.random.default_rng(31)
    offs, lens, size = _ragged(rng.integers(0, 600 << 10, 100))
    return Batch(rng.integers(0, 256, size, dtype=np.uint8), offs, lens)


def test_pinned_constant_stride(torch_cuda):
    """2-D copies: 24 parts of 300,007 B at stride 300,032 in one pinned buffer."""
    rng = np.random.default_rng(30)
    n, L, stride = 24, 300007, 300032
    t = _pinned(torch_cuda, n * stride, rng)
    b = Batch(t.numpy(), np.arange(n) * stride, np.full(n, L))
    b.check_dual(b.parts(t))


def test_pinned_ragged(torch_cuda):
    """Per-part copies (<= 64 pinned parts), lengths around the 64-byte block."""
    rng = np.random.default_rng(32)
    lens = [0, 1, 63, 64, 65, 5 * MIB + 9] + list(rng.integers(0, 3 * MIB, 6))
    offs, lens, size = _ragged(lens, gap=5)
    t = _pinned(torch_cuda, size, rng)
    b = Batch(t.numpy(), offs, lens)
    b.check_dual(b.parts(t))


def test_pageable_ragged_staged(torch_cuda, pageable_ragged):
    b = pageable_ragged
    b.check_dual(b.parts())
    b.check_dual(b.parts(), slice_bytes=4096)
    b.check_dual(b.parts(k=12), k=12, slice_bytes=64)


def test_crc_alone(torch_cuda, pageable_ragged):
    b = pageable_ragged
    b.check(None, s3.crc64_batch_host(b.parts()))
    b.check(None, s3.crc64_batch_host(b.parts(), slice_bytes=4096))


def test_sha256_words_equal_the_single_digest_call(torch_cuda, pageable_ragged):
    b = pageable_ragged
    sha, _ = s3.sha256_crc64_batch_host(b.parts())
    assert np.array_equal(sha, s3.sha256_batch_host(b.parts()))


def test_groups_then_slices(torch_cuda):
    """3,000 small pageable parts run in groups of whole parts; with two parts of 3 MiB + 1
    beside them the groups run first and the slice pipeline afterwards."""
    rng = np.random.default_rng(33)
    small = list(rng.integers(0, 3000, 3000))
    offs, lens, size = _ragged(small + [3 * MIB + 1, 3 * MIB + 1], gap=1)
    b = Batch(rng.integers(0, 256, size, dtype=np.uint8), offs, lens)
    b.check_dual(b.parts(k=3000), k=3000)
    b.check_dual(b.parts())
    b.check(None, s3.crc64_batch_host(b.parts()))


def test_file_ranges(torch_cuda, tmp_path):
    rng = np.random.default_rng(34)
    size = 6 * MIB
    host = rng.integers(0, 256, size, dtype=np.uint8)
    path = str(tmp_path / "object.bin")
    host.tofile(path)
    cuts = np.sort(rng.choice(np.arange(1, size), 35, replace=False))
    cuts = np.concatenate([[0], cuts, [size]])
    offs, lens = list(cuts[:-1]), list(np.diff(cuts))
    offs.insert(10, offs[10])  # an empty range
    lens.insert(10, 0)
    assert len(offs) == 37 and any(o % 16 for o in offs)
    b = Batch(host, offs, lens)
    sha, crcs = s3.sha256_crc64_file_parts(path, b.offs, b.lens)
    b.check(sha, crcs)
    # the FULL_OBJECT value of the file from its ranges' values
    keep = b.lens > 0
    assert s3.crc64_object(crcs[keep], b.lens[keep]) == s3.crc64(host)


def test_concurrent_callers_are_merged_by_digest_set(torch_cuda):
    """8 threads at once with four different digest sets, a 32-bit CRC among them: the merge
    key keeps them apart, and every caller gets its own results."""
    rng = np.random.default_rng(35)
    L, n = 256 * 1024 + 5, 16
    jobs = ["sha+crc64"] * 3 + ["sha+crc32c"] * 2 + ["sha"] + ["crc64"] * 2
    batches = []
    for _ in jobs:
        offs, lens, size = _ragged(np.full(n, L))
        batches.append(Batch(rng.integers(0, 256, size, dtype=np.uint8), offs, lens))
    results, errors = [None] * len(jobs), []
    gate = threading.Barrier(len(jobs))

    def run(i):
        try:
            b, job = batches[i], jobs[i]
            gate.wait()
            if job == "sha":
                results[i] = (s3.sha256_batch_host(b.parts()), None)
            elif job == "crc64":
                results[i] = (None, s3.crc64_batch_host(b.parts()))
            elif job == "sha+crc64":
                results[i] = s3.sha256_crc64_batch_host(b.parts())
            else:
                results[i] = s3.sha256_crc_batch_host(b.parts(), "crc32c")
        except Exception as e:  # noqa: BLE001
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, job in enumerate(jobs):
        sha, crcs = results[i]
        b = batches[i]
        if job == "sha":
            assert np.array_equal(sha, b.sha), i
        elif job == "sha+crc32c":
            assert np.array_equal(sha, b.sha), i
            want = np.array([s3.crc(b.host[int(o):int(o) + int(m)], "crc32c")
                             for o, m in zip(b.offs, b.lens)], dtype=np.uint32)
            assert np.array_equal(crcs, want), i
        else:
            b.check(sha, crcs)
