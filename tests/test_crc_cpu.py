"""CRC-32C / CRC-32 on the CPU (no GPU): s3h_cpu_crc on both backends, combine / full-object /
header text, argument errors, and a host model of the GPU kernels' decomposition
(tests/cpp/crc_model.cpp, built from crc_math.hpp) over the ragged shapes the GPU tests use."""
import base64
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests import crc_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGOS = ("crc32c", "crc32")
POLY = crc_shapes.POLY
KAT_CRC32C = [(b"123456789", 0xE3069283), (bytes(32), 0x8A9136AA), (b"\xff" * 32, 0x62A8AB43),
              (bytes(range(32)), 0x46DD794E), (bytes(range(31, -1, -1)), 0x113FDB5C), (b"", 0)]


def bitwise_crc(data: bytes, poly: int) -> int:
    """Reference: one bit at a time, reflected, init and xor-out 0xFFFFFFFF."""
    c = 0xFFFFFFFF
    for byte in data:
        c ^= byte
        for _ in range(8):
            c = (c >> 1) ^ (poly if c & 1 else 0)
    return c ^ 0xFFFFFFFF


def test_known_answers():
    for msg, want in KAT_CRC32C:
        assert s3.crc(msg, "crc32c") == want, msg
    assert s3.crc(b"123456789", "crc32") == 0xCBF43926
    assert s3.crc(b"", "crc32") == 0
    rng = np.random.default_rng(5)
    for n in (1, 7, 8, 9, 63, 4096, 100001):
        buf = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert s3.crc(buf, "crc32") == zlib.crc32(buf), n


def test_known_answers_on_the_table_path():
    """S3H_CPU_SCALAR=1 forces slicing-by-8 for CRC-32C too: same answers in a child process,
    and the same values as this process's backend on random buffers."""
    code = ("import sys,zlib,numpy as np;import s3client_amd as s;"
            "from tests.test_crc_cpu import KAT_CRC32C;"
            "assert s.cpu_backend()=='scalar';"
            "bad=[m for m,w in KAT_CRC32C if s.crc(m,'crc32c')!=w];"
            "assert not bad,bad;assert s.crc(b'123456789','crc32')==0xCBF43926;"
            "r=np.random.default_rng(6);"
            "print(*[s.crc(r.integers(0,256,n,dtype=np.uint8),a) for n in (1,8,9,300,65537) "
            "for a in ('crc32c','crc32')])")
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "S3H_CPU_SCALAR": "1"},
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    rng = np.random.default_rng(6)
    here = [s3.crc(rng.integers(0, 256, n, dtype=np.uint8), a) for n in (1, 8, 9, 300, 65537)
            for a in ALGOS]
    assert [int(x) for x in r.stdout.split()] == here


def test_crc32c_against_the_bitwise_reference_at_every_alignment():
    rng = np.random.default_rng(7)
    for L in list(range(301)) + [65537]:
        msg = rng.integers(0, 256, L, dtype=np.uint8)
        want = bitwise_crc(msg.tobytes(), POLY["crc32c"])
        raw = np.empty(L + 48, dtype=np.uint8)
        base = (-raw.ctypes.data) % 16
        for a in range(16):
            view = raw[base + a: base + a + L]
            view[:] = msg
            assert view.size == 0 or view.ctypes.data % 16 == a
            assert s3.crc(view, "crc32c") == want, (L, a)


@pytest.mark.parametrize("algo", ALGOS)
def test_seeded_chaining_equals_one_shot(algo):
    rng = np.random.default_rng(8)
    buf = rng.integers(0, 256, 20000, dtype=np.uint8).tobytes()
    want = s3.crc(buf, algo)
    for _ in range(20):
        cuts = sorted(rng.integers(0, len(buf) + 1, int(rng.integers(1, 6))))
        c, prev = 0, 0
        for cut in list(cuts) + [len(buf)]:
            c = s3.crc(buf[prev:cut], algo, c)
            prev = cut
        assert c == want, cuts


@pytest.mark.parametrize("algo", ALGOS)
def test_checksum_text(algo):
    assert s3.checksum_text(s3.crc(b"123456789", "crc32c"), "crc32c") == "4waSgw=="
    rng = np.random.default_rng(9)
    for n in (1, 2, 7, 1000):
        parts = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        cat = b"".join(int(p).to_bytes(4, "big") for p in parts)
        want = base64.b64encode(s3.crc(cat, algo).to_bytes(4, "big")).decode() + f"-{n}"
        assert s3.checksum_text(parts, algo, composite=True) == want
        single = base64.b64encode(int(parts[0]).to_bytes(4, "big")).decode()
        assert s3.checksum_text(parts[:1], algo) == single


@pytest.mark.parametrize("algo", ALGOS)
def test_combine_and_object_on_ragged_parts(algo):
    rng = np.random.default_rng(10)
    for lens in ([5, 0, 1, 300], [0, 0, 7], [1], [0], [4096, 1, 0, 65537, 3], [0, 1, 0]):
        chunks = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in lens]
        crcs = [s3.crc(c, algo) for c in chunks]
        whole = s3.crc(b"".join(chunks), algo)
        assert s3.crc_object(crcs, lens, algo) == whole, lens
        acc = crcs[0]
        for c, L in zip(crcs[1:], lens[1:]):
            acc = s3.crc_combine(acc, c, L, algo)
        assert acc == whole, lens


def test_combine_with_a_64_bit_length():
    """len_b = 2^32 + 5: crc32(A || zeros(L)) from crc(A) and crc(zeros(L)), both sides by zlib."""
    L = (1 << 32) + 5
    a = b"additional checksums"
    chunk = bytes(64 << 20)
    zeros_crc, cont = 0, zlib.crc32(a)
    done = 0
    while done < L:
        piece = chunk if L - done >= len(chunk) else chunk[:L - done]
        zeros_crc = zlib.crc32(piece, zeros_crc)
        cont = zlib.crc32(piece, cont)
        done += len(piece)
    assert s3.crc_combine(zlib.crc32(a), zeros_crc, L, "crc32") == cont
    assert s3.crc_object([zlib.crc32(a), zeros_crc], [len(a), L], "crc32") == cont


# ------------------------------------------------------------------ host model of the kernels
def _build_model(tmp, sanitize):
    exe = os.path.join(tmp, "crc_model_san" if sanitize else "crc_model")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"] if sanitize else ["-O2"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "crc_model.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("crc_model"))
    return {"plain": _build_model(tmp, False), "san": _build_model(tmp, True), "tmp": tmp}


def _run_model(model, which, algo, log2s, data, offs, lens, tag):
    dpath = os.path.join(model["tmp"], f"{tag}.bin")
    ppath = os.path.join(model["tmp"], f"{tag}.parts")
    data.tofile(dpath)
    with open(ppath, "w") as f:
        f.writelines(f"{int(o)} {int(n)}\n" for o, n in zip(offs, lens))
    r = subprocess.run([model[which], str(_native.CRC_IDS[algo]), str(log2s), dpath, ppath],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [int(x, 16) for x in r.stdout.split()]
    want = [s3.crc(data[int(o):int(o) + int(n)], algo) for o, n in zip(offs, lens)]
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (tag, [(i, int(offs[i]), int(lens[i])) for i in bad[:8]])


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("log2s", (10, 12))
def test_model_boundary_batch(model, algo, log2s):
    """The boundary lengths at every start alignment, under the sanitizers: a line read outside
    the parts' own lines runs off the model's allocation."""
    offs, lens, size = crc_shapes.boundary_layout(1 << log2s)
    for kind in ("random", "zeros", "ones"):
        _run_model(model, "san", algo, log2s, crc_shapes.fill(kind, size), offs, lens,
                   f"b_{algo}_{log2s}_{kind}")


@pytest.mark.parametrize("algo", ALGOS)
def test_model_ragged_batches(model, algo):
    """Many segments of one part (the run / tree fold of stage 2), 4,200 small parts, mixed
    segment counts -- at 4 KiB segments."""
    for name, (offs, lens, size) in (("fold", crc_shapes.segment_fold()),
                                     ("small", crc_shapes.many_small()),
                                     ("mixed", crc_shapes.mixed())):
        _run_model(model, "plain", algo, 12, crc_shapes.fill("random", size + 64, 3), offs, lens,
                   f"r_{algo}_{name}")


def test_model_segment_fold_under_sanitizers(model):
    offs, lens, size = crc_shapes.segment_fold()
    _run_model(model, "san", "crc32c", 12, crc_shapes.fill("random", size, 4), offs, lens, "san_fold")


def test_cpp_wrappers(tmp_path):
    """include/s3hash_batch.hpp namespace crc, linked against the built library."""
    exe = str(tmp_path / "crc_wrappers_test")
    libdir = os.path.dirname(_native.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-O1", "-I" + os.path.join(ROOT, "include"),
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "crc_wrappers_test.cpp"),
                        "-L" + libdir, "-ls3hash", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ------------------------------------------------------------------ argument errors
def test_argument_errors():
    L = _native.lib()
    one = (ctypes.c_uint64 * 1)(0)
    h = ctypes.c_void_p()
    out = (ctypes.c_uint32 * 1)()
    dummy = ctypes.c_void_p(16)
    E = _native.S3H_EINVAL
    # plan / batch: unknown checksum, null pointers, n == 0, n > 2^31 -- all before any device use
    assert L.s3h_crc_plan_create(0, 2, one, one, 1, ctypes.byref(h)) == E
    assert L.s3h_crc_plan_create(0, -1, one, one, 1, ctypes.byref(h)) == E
    assert L.s3h_crc_plan_create(0, 0, None, one, 1, ctypes.byref(h)) == E
    assert L.s3h_crc_plan_create(0, 0, one, None, 1, ctypes.byref(h)) == E
    assert L.s3h_crc_plan_create(0, 0, one, one, 1, None) == E
    assert L.s3h_crc_plan_create(0, 0, one, one, 0, ctypes.byref(h)) == E
    assert L.s3h_crc_plan_create(0, 0, one, one, (1 << 31) + 1, ctypes.byref(h)) == E
    assert L.s3h_crc_plan_launch(None, dummy, dummy, None) == E
    assert L.s3h_crc_plan_info(None, None, None, None, None) == E
    assert L.s3h_crc_batch_device(0, 7, dummy, one, one, 1, dummy, None) == E
    assert L.s3h_crc_batch_device(0, 0, None, one, one, 1, dummy, None) == E
    assert L.s3h_crc_batch_device(0, 0, dummy, None, one, 1, dummy, None) == E
    assert L.s3h_crc_batch_device(0, 0, dummy, one, one, 1, None, None) == E
    assert L.s3h_crc_batch_device(0, 0, dummy, one, one, 0, dummy, None) == E
    assert L.s3h_crc_batch_device(0, 0, dummy, one, one, (1 << 31) + 1, dummy, None) == E
    cnt = ctypes.c_uint64()
    assert L.s3h_crc_verify_batch_device(0, 2, dummy, one, one, 1, dummy, dummy, ctypes.byref(cnt), None) == E
    assert L.s3h_crc_verify_batch_device(0, 0, dummy, one, one, 1, None, dummy, ctypes.byref(cnt), None) == E
    assert L.s3h_crc_verify_batch_device(0, 0, dummy, one, one, 1, dummy, None, ctypes.byref(cnt), None) == E
    assert L.s3h_crc_verify_batch_device(0, 0, dummy, one, one, 1, dummy, dummy, None, None) == E
    assert L.s3h_crc_verify_batch_device(0, 0, dummy, one, one, 0, dummy, dummy, ctypes.byref(cnt), None) == E
    assert b"crc" in L.s3h_last_error()
    if s3.device_count() == 0:  # valid arguments and no device: never a CPU fallback
        assert L.s3h_crc_plan_create(0, 0, one, one, 1, ctypes.byref(h)) == _native.S3H_ENODEV
        assert L.s3h_crc_batch_device(0, 0, dummy, one, one, 1, dummy, None) == _native.S3H_ENODEV
    # host arithmetic
    assert L.s3h_crc_combine(2, 0, 0, 0, out) == E
    assert L.s3h_crc_combine(0, 0, 0, 0, None) == E
    assert L.s3h_crc_object(2, out, one, 1, out) == E
    assert L.s3h_crc_object(0, None, one, 1, out) == E
    assert L.s3h_crc_object(0, out, None, 1, out) == E
    assert L.s3h_crc_object(0, out, one, 1, None) == E
    assert L.s3h_crc_object(0, out, one, 0, out) == E
    buf = ctypes.create_string_buffer(_native.CHECKSUM_MAX)
    assert L.s3h_checksum_text(2, out, 1, 0, buf, len(buf)) == E
    assert L.s3h_checksum_text(0, None, 1, 0, buf, len(buf)) == E
    assert L.s3h_checksum_text(0, out, 0, 1, buf, len(buf)) == E
    assert L.s3h_checksum_text(0, out, 1, 0, None, len(buf)) == E
    assert L.s3h_checksum_text(0, out, 1, 0, buf, _native.CHECKSUM_MAX - 1) == E
    assert L.s3h_checksum_text(0, (ctypes.c_uint32 * 2)(), 2, 0, buf, len(buf)) == E  # plain form: one CRC
    assert L.s3h_cpu_crc(2, b"abc", 3, 0) == 0 and b"unknown checksum" in L.s3h_last_error()
    assert L.s3h_api_version() == 2
