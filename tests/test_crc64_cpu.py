"""CRC-64/NVME on the CPU (no GPU): s3h_cpu_crc64nvme against the known answers and a bitwise
reference, combine / full-object / header text, argument errors of every new entry point, the
C++ wrappers, and a host model of the GPU kernels' decomposition (tests/cpp/crc64_model.cpp,
built from crc64_math.hpp and crc_math.hpp) over the ragged shapes the GPU tests use, for
whole-part and ranged launches."""
import base64
import ctypes
import os
import subprocess

import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests import crc_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLY = 0x9A6C9329AC4BC9B5
M64 = (1 << 64) - 1
# the issue's table; the four 4 KiB vectors are the NVMe specification's
KAT = [(b"123456789", 0xAE8B14860A799888), (b"", 0), (bytes(32), 0xCF3473434D4ECF3B),
       (b"\xff" * 32, 0xA0A06974C34D63C4), (bytes(range(32)), 0xB9D9D4A8492CBD7F),
       (b"hello world", 0x8D29D5C3F6EA8EBE), (bytes(4096), 0x6482D367EB22B64E),
       (b"\xff" * 4096, 0xC0DDBA7302ECA3AC), (bytes(i & 255 for i in range(4096)), 0x3E729F5F6750449C),
       (bytes(255 - (i & 255) for i in range(4096)), 0x9A2DF64B8E9E517E)]


def bitwise_crc64(data: bytes) -> int:
    """Reference: one bit at a time, reflected, init and xor-out all ones."""
    c = M64
    for byte in data:
        c ^= byte
        for _ in range(8):
            c = (c >> 1) ^ (POLY if c & 1 else 0)
    return c ^ M64


def test_known_answers():
    for msg, want in KAT:
        assert s3.crc64(msg) == want, msg[:16]
        assert bitwise_crc64(msg) == want, msg[:16]  # (the reference itself)


def test_against_the_bitwise_reference_at_shifting_alignments():
    rng = np.random.default_rng(7)
    for L in list(range(301)) + [65537]:
        msg = rng.integers(0, 256, L, dtype=np.uint8)
        raw = np.empty(L + 48, dtype=np.uint8)
        a = L % 16
        start = (-raw.ctypes.data) % 16 + a
        view = raw[start: start + L]
        view[:] = msg
        assert view.size == 0 or view.ctypes.data % 16 == a
        assert s3.crc64(view) == bitwise_crc64(msg.tobytes()), L


def test_seeded_chaining_equals_one_shot():
    rng = np.random.default_rng(8)
    buf = rng.integers(0, 256, 20000, dtype=np.uint8).tobytes()
    want = s3.crc64(buf)
    assert want == bitwise_crc64(buf)
    for fixed in ([0], [1], [7, 8, 9], [len(buf)], [len(buf) - 1]):
        c, prev = 0, 0
        for cut in fixed + [len(buf)]:
            c = s3.crc64(buf[prev:cut], c)
            prev = cut
        assert c == want, fixed
    for _ in range(20):
        cuts = sorted(rng.integers(0, len(buf) + 1, int(rng.integers(1, 6))))
        c, prev = 0, 0
        for cut in list(cuts) + [len(buf)]:
            c = s3.crc64(buf[prev:cut], c)
            prev = cut
        assert c == want, cuts


def test_combine_and_object_on_ragged_parts():
    rng = np.random.default_rng(10)
    for lens in ([5, 0, 1, 300], [0, 0, 7], [1], [0], [4096, 1, 0, 65537, 3], [0, 1, 0]):
        chunks = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in lens]
        crcs = [s3.crc64(c) for c in chunks]
        whole = s3.crc64(b"".join(chunks))
        assert s3.crc64_object(crcs, lens) == whole, lens
        acc = crcs[0]
        for c, L in zip(crcs[1:], lens[1:]):
            acc = s3.crc64_combine(acc, c, L)
        assert acc == whole, lens


def test_combine_with_a_64_bit_length():
    """len_b = 2^32 + 5 in one combine equals the same fold chained in two halves whose lengths
    fit 32 bits: a length cut to 32 bits would fold by 5 bytes."""
    L, L1 = (1 << 32) + 5, (1 << 31) + 2
    L2 = L - L1
    z = {1 << 20: s3.crc64(bytes(1 << 20))}  # crc of m zero bytes, doubled up to 2^31
    m = 1 << 20
    while m < 1 << 31:
        z[2 * m] = s3.crc64_combine(z[m], z[m], m)
        m *= 2
    assert z[1 << 21] == s3.crc64(bytes(1 << 21))
    z1 = s3.crc64_combine(z[1 << 31], s3.crc64(bytes(2)), 2)        # zeros(L1)
    z2 = s3.crc64_combine(z[1 << 31], s3.crc64(bytes(3)), 3)        # zeros(L2)
    assert L2 == (1 << 31) + 3
    zl = s3.crc64_combine(z1, z2, L2)                                # zeros(L), lengths < 2^32
    a = s3.crc64(b"additional checksums")
    halves = s3.crc64_combine(s3.crc64_combine(a, z1, L1), z2, L2)
    assert s3.crc64_combine(a, zl, L) == halves
    assert s3.crc64_object([a, zl], [20, L]) == halves
    assert s3.crc64_combine(a, zl, 5) != halves


def test_checksum_text():
    assert s3.checksum64_text(s3.crc64(b"123456789")) == "rosUhgp5mIg="
    assert s3.checksum64_text(0) == "AAAAAAAAAAA="
    assert s3.checksum64_text(s3.crc64(b"hello world")) == "jSnVw/bqjr4="
    rng = np.random.default_rng(9)
    for v in rng.integers(0, 1 << 63, 50, dtype=np.uint64):
        v = (int(v) << 1 | 1) & M64
        assert s3.checksum64_text(v) == base64.b64encode(v.to_bytes(8, "big")).decode()


def test_existing_crc_ids_are_unchanged():
    assert _native.CRC_IDS == {"crc32c": 0, "crc32": 1}


# ------------------------------------------------------------------ host model of the kernels
def _build_model(tmp, sanitize):
    exe = os.path.join(tmp, "crc64_model_san" if sanitize else "crc64_model")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"] if sanitize else ["-O2"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "crc64_model.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("crc64_model"))
    return {"plain": _build_model(tmp, False), "san": _build_model(tmp, True), "tmp": tmp}


def _write(model, tag, data, offs, lens):
    dpath = os.path.join(model["tmp"], f"{tag}.bin")
    ppath = os.path.join(model["tmp"], f"{tag}.parts")
    data.tofile(dpath)
    with open(ppath, "w") as f:
        f.writelines(f"{int(o)} {int(n)}\n" for o, n in zip(offs, lens))
    return dpath, ppath


def _expected(data, offs, lens):
    return [s3.crc64(data[int(o):int(o) + int(n)]) for o, n in zip(offs, lens)]


def _run_model(model, which, log2s, data, offs, lens, tag):
    dpath, ppath = _write(model, tag, data, offs, lens)
    r = subprocess.run([model[which], str(log2s), dpath, ppath], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [int(x, 16) for x in r.stdout.split()]
    want = _expected(data, offs, lens)
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (tag, [(i, int(offs[i]), int(lens[i])) for i in bad[:8]])


@pytest.mark.parametrize("log2s", (10, 12))
def test_model_boundary_batch_under_sanitizers(model, log2s):
    """The boundary lengths at every start alignment, under ASan + UBSan: a line read outside
    the parts' own lines runs off the model's allocation."""
    offs, lens, size = crc_shapes.boundary_layout(1 << log2s)
    for kind in ("random", "zeros", "ones"):
        _run_model(model, "san", log2s, crc_shapes.fill(kind, size), offs, lens, f"b_{log2s}_{kind}")


def test_model_ragged_batches(model):
    """Many segments of one part (the run / tree fold of stage 2), 4,200 small parts, mixed
    segment counts -- at 4 KiB segments."""
    for name, (offs, lens, size) in (("fold", crc_shapes.segment_fold()),
                                     ("small", crc_shapes.many_small()),
                                     ("mixed", crc_shapes.mixed())):
        _run_model(model, "plain", 12, crc_shapes.fill("random", size + 64, 3), offs, lens, f"r_{name}")


def cut_list(S: int, longest: int):
    """Range ends at byte 1, mid-line (17), one byte either side of a segment boundary and on
    it, inside later segments, at the longest part's end and past it (ranges past the longest
    part must change nothing)."""
    return sorted({1, 17, S - 1, S, S + 1, 2 * S + 5, 4096, 65539, longest, longest + 100})


def writer_of(lens, cuts):
    ends = np.asarray(cuts, dtype=np.uint64)
    return [0 if n == 0 else int(np.searchsorted(ends, n, side="left")) for n in lens]


@pytest.mark.parametrize("name,which", (("mixed", "plain"), ("boundary", "plain"), ("boundary", "san")))
def test_model_ranged_launches(model, name, which):
    """Ranged stages over a cut list: the value of each part equals the CPU value and is written
    by the range that holds the part's last byte, once."""
    log2s = 8
    offs, lens, size = crc_shapes.mixed() if name == "mixed" else crc_shapes.boundary_layout(1 << log2s)
    data = crc_shapes.fill("random", size, 3)
    dpath, ppath = _write(model, f"rg_{name}_{which}", data, offs, lens)
    cuts = cut_list(1 << log2s, int(lens.max()))
    r = subprocess.run([model[which], str(log2s), dpath, ppath, *[str(c) for c in cuts]],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    rows = [l.split() for l in r.stdout.splitlines()]
    got = [int(c, 16) for c, _ in rows]
    want = _expected(data, offs, lens)
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (name, [(i, int(lens[i])) for i in bad[:8]])
    assert [int(w) for _, w in rows] == writer_of([int(n) for n in lens], cuts)


def test_cpp_wrappers(tmp_path):
    """include/s3hash_batch.hpp namespace crc64, compiled with -Wall -Wextra and linked against
    the built library."""
    exe = str(tmp_path / "crc64_wrappers_test")
    libdir = os.path.dirname(_native.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1",
                        "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "crc64_wrappers_test.cpp"),
                        "-L" + libdir, "-ls3hash", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ------------------------------------------------------------------ argument errors
def test_argument_errors():
    L = _native.lib()
    one = (ctypes.c_uint64 * 1)(0)
    h = ctypes.c_void_p()
    out = (ctypes.c_uint64 * 1)()
    dummy = ctypes.c_void_p(16)
    E = _native.S3H_EINVAL
    # plan / batch: null pointers, n == 0, n > 2^31 -- all before any device use
    assert L.s3h_crc64nvme_plan_create(0, None, one, 1, ctypes.byref(h)) == E
    assert L.s3h_crc64nvme_plan_create(0, one, None, 1, ctypes.byref(h)) == E
    assert L.s3h_crc64nvme_plan_create(0, one, one, 1, None) == E
    assert L.s3h_crc64nvme_plan_create(0, one, one, 0, ctypes.byref(h)) == E
    assert L.s3h_crc64nvme_plan_create(0, one, one, (1 << 31) + 1, ctypes.byref(h)) == E
    assert L.s3h_crc64nvme_plan_launch(None, dummy, dummy, None) == E
    assert L.s3h_crc64nvme_plan_launch_range(None, dummy, dummy, 0, 64, 0, None) == E
    assert L.s3h_crc64nvme_plan_info(None, None, None, None, None) == E
    assert L.s3h_crc64nvme_plan_destroy(None) == _native.S3H_OK
    assert L.s3h_crc64nvme_batch_device(0, None, one, one, 1, dummy, None) == E
    assert L.s3h_crc64nvme_batch_device(0, dummy, None, one, 1, dummy, None) == E
    assert L.s3h_crc64nvme_batch_device(0, dummy, one, None, 1, dummy, None) == E
    assert L.s3h_crc64nvme_batch_device(0, dummy, one, one, 1, None, None) == E
    assert L.s3h_crc64nvme_batch_device(0, dummy, one, one, 0, dummy, None) == E
    assert L.s3h_crc64nvme_batch_device(0, dummy, one, one, (1 << 31) + 1, dummy, None) == E
    cnt = ctypes.c_uint64()
    V = L.s3h_crc64nvme_verify_batch_device
    assert V(0, None, one, one, 1, dummy, dummy, ctypes.byref(cnt), None) == E
    assert V(0, dummy, None, one, 1, dummy, dummy, ctypes.byref(cnt), None) == E
    assert V(0, dummy, one, one, 1, None, dummy, ctypes.byref(cnt), None) == E
    assert V(0, dummy, one, one, 1, dummy, None, ctypes.byref(cnt), None) == E
    assert V(0, dummy, one, one, 1, dummy, dummy, None, None) == E
    assert V(0, dummy, one, one, 0, dummy, dummy, ctypes.byref(cnt), None) == E
    assert b"crc" in L.s3h_last_error()
    if s3.device_count() == 0:  # valid arguments and no device: never a CPU fallback
        assert L.s3h_crc64nvme_plan_create(0, one, one, 1, ctypes.byref(h)) == _native.S3H_ENODEV
        assert L.s3h_crc64nvme_batch_device(0, dummy, one, one, 1, dummy, None) == _native.S3H_ENODEV
    # the 32-bit entry points still refuse every other id
    assert L.s3h_crc_plan_create(0, 2, one, one, 1, ctypes.byref(h)) == E
    assert L.s3h_crc_batch_device(0, 2, dummy, one, one, 1, dummy, None) == E
    # host arithmetic
    assert L.s3h_crc64nvme_combine(0, 0, 0, None) == E
    assert L.s3h_crc64nvme_object(None, one, 1, out) == E
    assert L.s3h_crc64nvme_object(out, None, 1, out) == E
    assert L.s3h_crc64nvme_object(out, one, 1, None) == E
    assert L.s3h_crc64nvme_object(out, one, 0, out) == E
    buf = ctypes.create_string_buffer(_native.CHECKSUM_MAX)
    assert L.s3h_checksum64_text(1, None, len(buf)) == E
    assert L.s3h_checksum64_text(1, buf, _native.CHECKSUM_MAX - 1) == E
    assert L.s3h_cpu_crc64nvme(None, 3, 0) == 0 and b"null data" in L.s3h_last_error()
    # host-resident forms
    ptrs = (ctypes.c_void_p * 1)(16)
    sha = (ctypes.c_uint32 * 8)()
    assert L.s3h_crc64nvme_batch_host(None, one, 1, out, 0, 0) == E
    assert L.s3h_crc64nvme_batch_host(ptrs, None, 1, out, 0, 0) == E
    assert L.s3h_crc64nvme_batch_host(ptrs, one, 1, None, 0, 0) == E
    assert L.s3h_crc64nvme_batch_host(ptrs, one, 0, out, 0, 0) == E
    assert L.s3h_sha256_crc64nvme_batch_host(None, one, 1, sha, out, 0, 0) == E
    assert L.s3h_sha256_crc64nvme_batch_host(ptrs, one, 1, None, out, 0, 0) == E
    assert L.s3h_sha256_crc64nvme_batch_host(ptrs, one, 1, sha, None, 0, 0) == E
    assert L.s3h_sha256_crc64nvme_file_parts(None, one, one, 1, sha, out, 0, 0) == E
    assert L.s3h_sha256_crc64nvme_file_parts(b"/dev/null", None, one, 1, sha, out, 0, 0) == E
    assert L.s3h_sha256_crc64nvme_file_parts(b"/dev/null", one, one, 1, None, out, 0, 0) == E
    assert L.s3h_sha256_crc64nvme_file_parts(b"/dev/null", one, one, 1, sha, None, 0, 0) == E
    assert L.s3h_api_version() == 2
