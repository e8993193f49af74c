"""SHA-1, and SHA-256 + SHA-1 from one pass over the host link, of host-resident parts
(s3h_sha1_batch_host, s3h_sha256_sha1_batch_host, s3h_sha1_file_parts,
s3h_sha256_sha1_file_parts, s3h_verify_batch_host): the group and the slice pipeline, pinned and
pageable sources, file ranges, concurrent callers with different digest sets.

Expected digests: hashlib.sha1 / hashlib.sha256 (the digest bytes in memory); in every
two-digest call the SHA-256 half also equals sha256_batch_host of the same parts."""
import hashlib
import subprocess
import threading

import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests.test_sha1_cpu import build_sha1_wrappers_test

pytestmark = pytest.mark.gpu
KIB, MIB = 1 << 10, 1 << 20
GROUP_MAX_PART = 1 << 20  # host_limits.hpp kGroupMaxPart
_CACHE = {}


class Batch:
    """Parts of one buffer (offsets, lengths) and their expected digests."""

    def __init__(self, host, offs, lens):
        self.host = host
        self.offs = np.asarray(offs, dtype=np.uint64)
        self.lens = np.asarray(lens, dtype=np.uint64)
        views = [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(self.offs, self.lens)]
        self.sha1 = np.frombuffer(b"".join(hashlib.sha1(v).digest() for v in views),
                                  dtype=np.uint32).reshape(-1, 5)
        self.sha256 = np.frombuffer(b"".join(hashlib.sha256(v).digest() for v in views),
                                    dtype=np.uint32).reshape(-1, 8)
        self._alone = None

    def parts(self, buf=None):
        return s3.BufferParts(self.host if buf is None else buf, self.offs, self.lens)

    def pinned(self, torch):
        t = torch.empty(self.host.size, dtype=torch.uint8, pin_memory=True)
        t.numpy()[:] = self.host
        return t

    def sha256_alone(self):
        if self._alone is None:
            self._alone = s3.sha256_batch_host(self.parts())
            assert np.array_equal(self._alone, self.sha256)
        return self._alone

    def bad(self, got, want):
        rows = np.flatnonzero((got != want).any(axis=1))
        return [(int(i), int(self.lens[i])) for i in rows[:8]]

    def check(self, parts, **kw):
        s1 = s3.sha1_batch_host(parts, **kw)
        assert s1.shape == self.sha1.shape and np.array_equal(s1, self.sha1), self.bad(s1, self.sha1)
        sha, s1 = s3.sha256_sha1_batch_host(parts, **kw)
        assert np.array_equal(s1, self.sha1), self.bad(s1, self.sha1)
        assert np.array_equal(sha, self.sha256_alone()), self.bad(sha, self.sha256)


def _ragged(seed, lens, gap=5):
    lens = np.asarray(lens, dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens + np.uint64(gap))[:-1]]).astype(np.uint64)
    host = np.random.default_rng(seed).integers(0, 256, int(offs[-1] + lens[-1]) + 64, dtype=np.uint8)
    return Batch(host, offs, lens)


def _groups():
    """Group mode: 300 parts of U[1, 128] KiB."""
    if "groups" not in _CACHE:
        _CACHE["groups"] = _ragged(231, np.random.default_rng(230).integers(1 * KIB, 128 * KIB + 1, 300))
    return _CACHE["groups"]


def _slices():
    """Slice mode: 6 parts of U[2, 3] MiB and one of 1 byte beyond kGroupMaxPart."""
    if "slices" not in _CACHE:
        lens = list(np.random.default_rng(232).integers(2 * MIB, 3 * MIB + 1, 6)) + [GROUP_MAX_PART + 1]
        _CACHE["slices"] = _ragged(233, lens)
    return _CACHE["slices"]


@pytest.mark.parametrize("source", ("pageable", "pinned"))
def test_group_mode(torch_cuda, source):
    b = _groups()
    assert int(b.lens.max()) <= GROUP_MAX_PART
    b.check(b.parts(b.pinned(torch_cuda)) if source == "pinned" else b.parts())


@pytest.mark.parametrize("source", ("pageable", "pinned"))
def test_slice_mode(torch_cuda, source):
    """An explicit slice of 192 KiB: 16 slices over the longest part, with the geometric tail."""
    b = _slices()
    assert int(b.lens.min()) > GROUP_MAX_PART
    b.check(b.parts(b.pinned(torch_cuda)) if source == "pinned" else b.parts(), slice_bytes=192 * KIB)


def test_slice_mode_default_slice(torch_cuda):
    b = _slices()
    b.check(b.parts())


def test_file_ranges(torch_cuda, tmp_path):
    rng = np.random.default_rng(234)
    size = 5 * MIB
    host = rng.integers(0, 256, size, dtype=np.uint8)
    path = str(tmp_path / "object.bin")
    host.tofile(path)
    cuts = np.concatenate([[0], np.sort(rng.choice(np.arange(1, size), 30, replace=False)), [size]])
    offs, lens = list(cuts[:-1]), list(np.diff(cuts))
    offs.insert(7, offs[7])  # an empty range
    lens.insert(7, 0)
    b = Batch(host, offs, lens)
    s1 = s3.sha1_file_parts(path, b.offs, b.lens)
    assert np.array_equal(s1, b.sha1), b.bad(s1, b.sha1)
    sha, s1 = s3.sha256_sha1_file_parts(path, b.offs, b.lens)
    assert np.array_equal(s1, b.sha1), b.bad(s1, b.sha1)
    assert np.array_equal(sha, b.sha256_alone())
    # a range past the end of the file
    for call in (s3.sha1_file_parts, s3.sha256_sha1_file_parts):
        with pytest.raises(s3.S3HashError) as e:
            call(path, [size - 10], [11])
        assert e.value.code == _native.S3H_EINVAL


def test_verify_batch_host(torch_cuda):
    b = _groups()
    assert not s3.verify_batch_host(b.parts(), b.sha1, algo="sha1").any()
    host = b.host.copy()
    host[int(b.offs[123]) + 17] ^= 1
    mism = s3.verify_batch_host(s3.BufferParts(host, b.offs, b.lens), b.sha1, algo="sha1")
    assert np.flatnonzero(mism).tolist() == [123]
    with pytest.raises(s3.S3HashError) as e:
        s3.verify_batch_routed(b.parts(), b.sha1, algo="sha1", route="gpu")
    assert e.value.code == _native.S3H_EINVAL


def test_concurrent_callers_with_different_digest_sets(torch_cuda):
    """Two threads at once, one asking for SHA-256 + SHA-1 and one for SHA-256 + MD5: the merge
    key is the id array, so the calls are not merged and both get their own digests."""
    a = _ragged(235, np.random.default_rng(236).integers(1, 300 * KIB, 40))
    b = _ragged(237, np.random.default_rng(238).integers(1, 300 * KIB, 40))
    md5 = np.frombuffer(b"".join(hashlib.md5(b.host[int(o):int(o) + int(n)].tobytes()).digest()
                                 for o, n in zip(b.offs, b.lens)), dtype=np.uint32).reshape(-1, 4)
    results, errors = {}, []
    gate = threading.Barrier(2)

    def run(name, fn, batch):
        try:
            gate.wait()
            results[name] = fn(batch.parts())
        except Exception as e:  # noqa: BLE001
            errors.append((name, repr(e)))

    threads = [threading.Thread(target=run, args=("sha1", s3.sha256_sha1_batch_host, a)),
               threading.Thread(target=run, args=("md5", s3.sha256_md5_batch_host, b))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert np.array_equal(results["sha1"][0], a.sha256) and np.array_equal(results["sha1"][1], a.sha1)
    assert np.array_equal(results["md5"][0], b.sha256) and np.array_equal(results["md5"][1], md5)


def test_cpp_wrappers_with_a_device(torch_cuda, tmp_path):
    exe = build_sha1_wrappers_test(tmp_path)
    path = str(tmp_path / "bytes.bin")
    (np.arange(3 * MIB, dtype=np.uint32) & 255).astype(np.uint8).tofile(path)
    r = subprocess.run([exe, "gpu", path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
