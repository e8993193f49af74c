"""SHA-1 without a GPU: the CPU function s3h_cpu_sha1 (SHA-NI and scalar paths) against the FIPS
180 vectors and hashlib.sha1, the header text of the digest checksums against base64 + hashlib,
the argument errors that are reported before any device is looked for, the SHA-1 kernel's
entry in kernel_isa_counts.json, and the C++ wrappers (tests/cpp/sha1_wrappers_test.cpp)."""
import base64
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests import range_shapes as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# FIPS 180 example messages (one-block, two-block, 448- and 896-bit, one million "a")
FIPS = [
    (b"", "da39a3ee5e6b4b0d3255bfef95601890afd80709"),
    (b"abc", "a9993e364706816aba3e25717850c26c9cd0d89d"),
    (b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq",
     "84983e441c3bd26ebaae4aa1f95129e5e54670f1"),
    (b"abcdefghbcdefghicdefghijdefghijkefghijklfghijklmghijklmnhijklmnoijklmnopjklmnopqklmnopqr"
     b"lmnopqrsmnopqrstnopqrstu", "a49b2446a02c645bf419f995b67091253a04a259"),
    (b"a" * 1_000_000, "34aa973cd4c4daa4f61eeb2bdbad27316534016f"),
]
LENGTHS = sorted(set(range(201)) | set(rs.SHORT_LENGTHS + rs.LONG_LENGTHS))


def _text(words) -> str:
    return np.asarray(words, dtype=np.uint32).tobytes().hex()


def test_fips_vectors():
    assert len(FIPS[2][0]) * 8 == 448 and len(FIPS[3][0]) * 8 == 896
    for msg, digest in FIPS:
        assert hashlib.sha1(msg).hexdigest() == digest
        assert _text(s3.sha1(msg)) == digest, len(msg)


def test_every_length_against_hashlib():
    data = np.random.default_rng(41).integers(0, 256, max(LENGTHS), dtype=np.uint8).tobytes()
    bad = [L for L in LENGTHS if _text(s3.sha1(data[:L])) != hashlib.sha1(data[:L]).hexdigest()]
    assert not bad, bad


def test_scalar_path_in_a_child_process():
    """The compression is chosen at load time, so S3H_CPU_SCALAR=1 needs a process of its own
    (as tests/test_dropin_cpu.py test_cpu_sha256_golden runs SHA-256's)."""
    code = ("import sys,hashlib,numpy as np;import s3client_amd as s;"
            "from tests.test_sha1_cpu import FIPS,LENGTHS;"
            "assert s.cpu_backend()=='scalar';"
            "t=lambda w:np.asarray(w,dtype=np.uint32).tobytes().hex();"
            "d=np.random.default_rng(41).integers(0,256,max(LENGTHS),dtype=np.uint8).tobytes();"
            "bad=[len(m) for m,h in FIPS if t(s.sha1(m))!=h];"
            "bad+=[L for L in LENGTHS if t(s.sha1(d[:L]))!=hashlib.sha1(d[:L]).hexdigest()];"
            "print(bad);sys.exit(1 if bad else 0)")
    r = subprocess.run(["python", "-c", code], env={**os.environ, "S3H_CPU_SCALAR": "1"},
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr


# ------------------------------------------------------------------ header text
def _digests(algo, n):
    h = getattr(hashlib, algo)
    raw = b"".join(h(b"part %d" % i).digest() for i in range(n))
    return raw, np.frombuffer(raw, dtype=np.uint32).reshape(n, -1)


@pytest.mark.parametrize("algo", ("sha1", "sha256"))
def test_digest_checksum_text(algo):
    h = getattr(hashlib, algo)
    raw, words = _digests(algo, 1)
    assert words.shape[1] == (5 if algo == "sha1" else 8)
    assert s3.digest_checksum_text(words, algo) == base64.b64encode(raw).decode()
    assert s3.digest_checksum_text(s3.sha1(b"abc") if algo == "sha1" else s3.sha256(b"abc"), algo) == \
        base64.b64encode(h(b"abc").digest()).decode()
    for n in (1, 2, 10_000):
        raw, words = _digests(algo, n)
        want = base64.b64encode(h(raw).digest()).decode() + "-%d" % n
        assert s3.digest_checksum_text(words, algo, composite=True) == want, n
        assert len(want) < _native.DIGEST_CHECKSUM_MAX


def test_digest_checksum_text_errors():
    L = _native.lib()
    _, two = _digests("sha1", 2)
    two = np.ascontiguousarray(two)
    out = ctypes.create_string_buffer(_native.DIGEST_CHECKSUM_MAX)
    call = lambda algo, n, comp, buf, size: L.s3h_digest_checksum_text(  # noqa: E731
        algo, ctypes.c_void_p(two.ctypes.data), n, comp, buf, size)
    assert call(_native.ALGO_SHA1, 1, 0, out, len(out)) == _native.S3H_OK
    assert call(_native.ALGO_SHA1, 2, 0, out, len(out)) == _native.S3H_EINVAL   # plain form, n != 1
    assert call(_native.ALGO_SHA1, 0, 1, out, len(out)) == _native.S3H_EINVAL
    assert call(_native.ALGO_MD5, 1, 0, out, len(out)) == _native.S3H_EINVAL    # MD5: multipart_etag
    assert call(3, 1, 0, out, len(out)) == _native.S3H_EINVAL
    assert call(_native.ALGO_SHA1, 1, 2, out, len(out)) == _native.S3H_EINVAL
    short = ctypes.create_string_buffer(_native.DIGEST_CHECKSUM_MAX - 1)
    short.raw = b"x" * len(short)
    assert call(_native.ALGO_SHA256, 1, 0, short, len(short)) == _native.S3H_EINVAL
    assert short.raw[0:1] == b"\0" and short.raw[1:] == b"x" * (len(short) - 1)
    with pytest.raises(s3.S3HashError):
        s3.digest_checksum_text(two, "sha1")
    with pytest.raises(s3.S3HashError):
        s3.digest_checksum_text(np.zeros(4, dtype=np.uint32), "md5")


# ------------------------------------------------------------------ argument errors, no device
def test_einval_before_any_device():
    L = _native.lib()
    one = (ctypes.c_uint64 * 1)(0)
    h = ctypes.c_void_p()
    assert L.s3h_plan_create_ex(0, 3, one, one, 1, _native.KERNEL_AUTO, ctypes.byref(h)) == _native.S3H_EINVAL
    assert b"unknown algorithm" in L.s3h_last_error()
    for k in (_native.KERNEL_LANE, _native.KERNEL_PAIR, _native.KERNEL_QUAD, _native.KERNEL_SKEW,
              _native.KERNEL_SKEWP, _native.KERNEL_SKEWS):
        assert L.s3h_plan_create_ex(0, _native.ALGO_SHA1, one, one, 1, k, ctypes.byref(h)) == _native.S3H_EINVAL
        assert b"SHA-1" in L.s3h_last_error()
    assert not h.value
    part = np.zeros(4, dtype=np.uint8)
    with pytest.raises(s3.S3HashError) as e:
        s3.verify_batch_routed([part], np.zeros((1, 5), dtype=np.uint32), algo="sha1")
    assert e.value.code == _native.S3H_EINVAL
    assert _native.ALGO_IDS["sha1"] == 2 and _native.DIGEST_WORDS[2] == 5
    assert "sha1" not in _native.DIGESTS_IDS


# ------------------------------------------------------------------ instruction count
def test_kernel_isa_counts_entry():
    """The consumer's fast loop: 400 round instructions + 20 LDS reads + 5 feed-forward adds,
    plus waits, barrier and loop overhead; a sixth VALU per round would be 480."""
    with open(os.path.join(ROOT, "s3client_amd", "kernel_isa_counts.json")) as f:
        isa = json.load(f)
    for key, bps in (("sha1-pc", 2), ("sha1-pc1", 1)):  # the two step forms launch.hip picks from
        assert len(isa["code_hash"][key]) >= 16
        k = isa["kernels"][key]
        assert k["blocks_per_step"] == bps
        assert k["per_block"]["lds"] == 20
        assert k["instr_per_block"] <= 440, k


# ------------------------------------------------------------------ C++ wrappers
def build_sha1_wrappers_test(tmp_path) -> str:
    exe = str(tmp_path / "sha1_wrappers_test")
    libdir = os.path.dirname(_native.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1",
                        "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "sha1_wrappers_test.cpp"),
                        "-L" + libdir, "-ls3hash", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_cpp_wrappers(tmp_path):
    """include/s3hash_batch.hpp namespace sha1, compiled with -Wall -Wextra and linked against
    the built library: the CPU-only part."""
    exe = build_sha1_wrappers_test(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
