"""SHA-256 + CRC-32C / CRC-32 (and a CRC alone) of host-resident parts from one pass through the
host pipeline (s3h_sha256_crc_batch_host, s3h_crc_batch_host, s3h_sha256_crc_file_parts): every
copy mode of the slice and group pipelines.  Expected values: zlib.crc32, s3h_cpu_crc for
CRC-32C (pinned by tests/test_crc_cpu.py), hashlib.sha256 (the 32 digest bytes in memory)."""
import hashlib
import subprocess
import threading
import zlib

import numpy as np
import pytest

import s3client_amd as s3
from tests.test_crc_range_cpu import build_host_wrappers_test

pytestmark = pytest.mark.gpu
ALGOS = ("crc32c", "crc32")
MIB = 1 << 20


def _crc(buf, algo):
    b = buf.tobytes()
    return zlib.crc32(b) if algo == "crc32" else s3.crc(b, "crc32c")


class Batch:
    """Parts of one buffer (a numpy view of it, offsets, lengths) and their expected values."""

    def __init__(self, host, offs, lens):
        self.host = host
        self.offs = np.asarray(offs, dtype=np.uint64)
        self.lens = np.asarray(lens, dtype=np.uint64)
        views = [host[int(o):int(o) + int(n)] for o, n in zip(self.offs, self.lens)]
        self.sha = np.frombuffer(b"".join(hashlib.sha256(v.tobytes()).digest() for v in views),
                                 dtype=np.uint32).reshape(-1, 8)
        self.crc = {a: np.array([_crc(v, a) for v in views], dtype=np.uint32) for a in ALGOS}

    def parts(self, buf=None, k=None):
        return s3.BufferParts(self.host if buf is None else buf, self.offs[:k], self.lens[:k])

    def check(self, sha, crcs, algo, k=None):
        want = self.crc[algo][:k]
        bad = np.flatnonzero(crcs != want)
        assert bad.size == 0, (algo, [(int(i), int(self.lens[i]), hex(crcs[i]), hex(want[i])) for i in bad[:8]])
        if sha is not None:
            bad = np.flatnonzero((sha != self.sha[:k]).any(axis=1))
            assert bad.size == 0, ("sha256", [(int(i), int(self.lens[i])) for i in bad[:8]])

    def check_dual(self, parts, k=None, **kw):
        for algo in ALGOS:
            sha, crcs = s3.sha256_crc_batch_host(parts, algo, **kw)
            self.check(sha, crcs, algo, k)


def _ragged(rng, lens, gap=0):
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
    offs, lens, size = _ragged(rng, rng.integers(0, 600 << 10, 100))
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
    offs, lens, size = _ragged(rng, lens, gap=5)
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
    for algo in ALGOS:
        b.check(None, s3.crc_batch_host(b.parts(), algo), algo)
        b.check(None, s3.crc_batch_host(b.parts(), algo, slice_bytes=4096), algo)


def test_sha256_words_equal_the_single_digest_call(torch_cuda, pageable_ragged):
    b = pageable_ragged
    alone = s3.sha256_batch_host(b.parts())
    for algo in ALGOS:
        sha, _ = s3.sha256_crc_batch_host(b.parts(), algo)
        assert np.array_equal(sha, alone)


def test_groups_then_slices(torch_cuda):
    """3,000 small pageable parts run in groups of whole parts; with two parts of 3 MiB + 1
    beside them the groups run first and the slice pipeline afterwards."""
    rng = np.random.default_rng(33)
    small = list(rng.integers(0, 3000, 3000))
    offs, lens, size = _ragged(rng, small + [3 * MIB + 1, 3 * MIB + 1], gap=1)
    b = Batch(rng.integers(0, 256, size, dtype=np.uint8), offs, lens)
    b.check_dual(b.parts(k=3000), k=3000)
    b.check_dual(b.parts())
    for algo in ALGOS:
        b.check(None, s3.crc_batch_host(b.parts(), algo), algo)


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
    for algo in ALGOS:
        sha, crcs = s3.sha256_crc_file_parts(path, b.offs, b.lens, algo)
        b.check(sha, crcs, algo)


def test_concurrent_callers_are_merged_by_digest_set(torch_cuda):
    """8 threads at once with four different digest sets: the merge key keeps them apart, and
    every caller gets its own results."""
    rng = np.random.default_rng(35)
    L, n = 256 * 1024 + 5, 16
    jobs = ["sha+crc32c"] * 3 + ["sha+crc32"] * 2 + ["sha"] * 2 + ["crc32c"]
    batches = []
    for _ in jobs:
        offs, lens, size = _ragged(rng, np.full(n, L))
        batches.append(Batch(rng.integers(0, 256, size, dtype=np.uint8), offs, lens))
    results, errors = [None] * len(jobs), []
    gate = threading.Barrier(len(jobs))

    def run(i):
        try:
            b, job = batches[i], jobs[i]
            gate.wait()
            if job == "sha":
                results[i] = (s3.sha256_batch_host(b.parts()), None)
            elif job == "crc32c":
                results[i] = (None, s3.crc_batch_host(b.parts(), "crc32c"))
            else:
                results[i] = s3.sha256_crc_batch_host(b.parts(), job.split("+")[1])
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
        if job == "sha":
            assert np.array_equal(sha, batches[i].sha), i
        else:
            batches[i].check(sha, crcs, job.split("+")[-1])


def test_argument_errors_with_a_device(torch_cuda, tmp_path):
    exe = build_host_wrappers_test(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
