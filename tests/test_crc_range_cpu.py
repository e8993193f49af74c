"""Ranged (resumable) CRC launches and the host-resident CRC entry points, on the CPU (no GPU):
a host model of the ranged decomposition (tests/cpp/crc_range_model.cpp, built from the
crc_math.hpp functions the kernels call) walked over cut lists on the shapes the GPU tests use,
and the argument errors of s3h_crc_batch_host / s3h_sha256_crc_batch_host /
s3h_sha256_crc_file_parts through the C++ wrappers (tests/cpp/crc_host_wrappers_test.cpp)."""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests import crc_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGOS = ("crc32c", "crc32")


def expected_crcs(data, offs, lens, algo):
    """zlib for CRC-32, s3.crc (pinned by tests/test_crc_cpu.py) for CRC-32C."""
    one = (lambda b: zlib.crc32(b)) if algo == "crc32" else (lambda b: s3.crc(b, "crc32c"))
    return [one(data[int(o):int(o) + int(n)].tobytes()) for o, n in zip(offs, lens)]


def cut_list(S: int, longest: int):
    """Range ends 1, 17, S-1, S, S+1, 2S+5, 4096, 65539 and the longest part, ascending (ranges
    past the longest part stay in: they must change nothing)."""
    return sorted({1, 17, S - 1, S, S + 1, 2 * S + 5, 4096, 65539, longest})


def writer_of(lens, cuts):
    """Index of the range (begin, end] = (cuts[i-1], cuts[i]] that holds each part's last byte;
    an empty part is written by range 0."""
    ends = np.asarray(cuts, dtype=np.uint64)
    return [0 if n == 0 else int(np.searchsorted(ends, n, side="left")) for n in lens]


def _build(tmp, sanitize):
    exe = os.path.join(tmp, "crc_range_model_san" if sanitize else "crc_range_model")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"] if sanitize else ["-O2"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "crc_range_model.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("crc_range_model"))
    return {"plain": _build(tmp, False), "san": _build(tmp, True), "tmp": tmp}


@pytest.fixture(scope="module")
def shapes():
    """name -> (log2 S, data, offsets, lengths); the expected CRCs are computed once per algo."""
    out = {}
    offs, lens, size = crc_shapes.mixed()
    out["mixed"] = (8, crc_shapes.fill("random", size, 3), offs, lens)
    offs, lens, size = crc_shapes.boundary_layout(1 << 8)
    out["boundary"] = (8, crc_shapes.fill("random", size, 4), offs, lens)
    return out


@pytest.fixture(scope="module")
def expected(shapes):
    return {(name, algo): expected_crcs(d, o, n, algo)
            for name, (_, d, o, n) in shapes.items() for algo in ALGOS}


def _run(model, which, algo, shape, name, cuts, cut_args, expected):
    log2s, data, offs, lens = shape
    dpath = os.path.join(model["tmp"], f"{name}.bin")
    ppath = os.path.join(model["tmp"], f"{name}.parts")
    if not os.path.exists(dpath):
        data.tofile(dpath)
        with open(ppath, "w") as f:
            f.writelines(f"{int(o)} {int(n)}\n" for o, n in zip(offs, lens))
    r = subprocess.run([model[which], str(_native.CRC_IDS[algo]), str(log2s), dpath, ppath, *cut_args],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    rows = [l.split() for l in r.stdout.splitlines()]
    got = [int(c, 16) for c, _ in rows]
    wrote = [int(w) for _, w in rows]
    want = expected[(name, algo)]
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (name, [(i, int(lens[i])) for i in bad[:8]])
    assert wrote == writer_of([int(n) for n in lens], cuts), name


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", ("mixed", "boundary"))
def test_model_cut_list(model, shapes, expected, algo, name):
    """Cuts at 1, 17, S-1, S, S+1, 2S+5, 4096, 65539 and the longest part: range ends inside
    pieces, on the segment grid and one byte off it."""
    shape = shapes[name]
    cuts = cut_list(1 << shape[0], int(shape[3].max()))
    _run(model, "plain", algo, shape, name, cuts, [str(c) for c in cuts], expected)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", ("mixed", "boundary"))
def test_model_every_64_bytes(model, shapes, expected, algo, name):
    """The host pipeline's smallest slices: a range per 64 bytes."""
    shape = shapes[name]
    longest = int(shape[3].max())
    cuts = list(range(64, longest, 64)) + [longest]
    _run(model, "plain", algo, shape, name, cuts, [f"every:64:{longest}"], expected)


@pytest.mark.parametrize("algo", ALGOS)
def test_model_under_sanitizers(model, shapes, expected, algo):
    """The same program as a stand-alone binary under ASan + UBSan: every start alignment and
    boundary length, both cut lists; a line read outside a range's own lines runs off the
    model's slot buffer."""
    shape = shapes["boundary"]
    longest = int(shape[3].max())
    cuts = cut_list(1 << shape[0], longest)
    _run(model, "san", algo, shape, "boundary", cuts, [str(c) for c in cuts], expected)
    cuts = list(range(64, longest, 64)) + [longest]
    _run(model, "san", algo, shape, "boundary", cuts, [f"every:64:{longest}"], expected)


def build_host_wrappers_test(tmp_path) -> str:
    exe = str(tmp_path / "crc_host_wrappers_test")
    libdir = os.path.dirname(_native.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-O1", "-I" + os.path.join(ROOT, "include"),
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "crc_host_wrappers_test.cpp"),
                        "-L" + libdir, "-ls3hash", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_host_entry_point_argument_errors(tmp_path):
    """Unknown checksum / null pointers -> S3H_EINVAL from the three host entry points and
    their C++ wrappers, before any device is looked for."""
    exe = build_host_wrappers_test(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_ranged_launch_argument_errors():
    L = _native.lib()
    dummy = ctypes.c_void_p(16)
    assert L.s3h_crc_plan_launch_range(None, dummy, dummy, 0, 64, 0, None) == _native.S3H_EINVAL
    assert b"crc" in L.s3h_last_error()
