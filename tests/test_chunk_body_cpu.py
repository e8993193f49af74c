"""aws-chunked bodies on the CPU: s3h_chunk_body_geometry and s3h_cpu_chunk_body against the
plain-Python rule and its independent decoder (tests/chunk_body_ref.py).  Bit-exact; no GPU.

The assembler only renders signatures, checksums and trailer signatures, so the tests feed it
random ones."""
import ctypes

import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests import chunk_body_ref as bref
from tests import chunk_sign_ref as ref
from tests import chunk_trailer_ref as tref
from tests.chunk_body_ref import CHUNK_BYTES, KINDS, grid_case, grid_lengths, grid_parts

SENTINEL = 0xA5


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", CHUNK_BYTES)
def test_geometry_equals_the_framed_length(c, kind):
    bodies = grid_case(c, kind)[3]
    g = s3.chunk_body_geometry(grid_lengths(c), c, kind)
    want = [len(b) for b in bodies]
    assert g["body_lengths"].tolist() == want
    assert want == [bref.body_length(n, c, kind) for n in grid_lengths(c)]
    assert g["body_offsets"].tolist() == [sum(want[:i]) for i in range(len(want))]
    assert g["total"] == sum(want)


def test_known_totals():
    # the AWS documentation's example: Content-Length 66824; with the CRC-32C trailer 66946
    assert s3.chunk_body_geometry([66560], 65536)["total"] == 65626 + 1112 + 86 == 66824
    assert s3.chunk_body_geometry([66560], 65536, "crc32c")["total"] == 66946
    # any output may be null
    lens = np.array([66560], dtype=np.uint64)
    total = ctypes.c_uint64()
    L = _native.lib()
    _native.check(L.s3h_chunk_body_geometry(lens.ctypes.data_as(_native.u64p), 1, 65536, -1, None, None,
                                            ctypes.byref(total)))
    assert total.value == 66824
    _native.check(L.s3h_chunk_body_geometry(lens.ctypes.data_as(_native.u64p), 1, 65536, -1, None, None, None))


def _image(bodies, offsets, size):
    img = np.full(size, SENTINEL, dtype=np.uint8)
    for b, o in zip(bodies, offsets):
        img[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return img


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "offsets"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", CHUNK_BYTES)
def test_cpu_body_equals_the_rule(c, kind, packed):
    parts = grid_parts(c)
    sigs, values, tsigs, bodies = grid_case(c, kind)
    arr = None if kind is None else tref.to_array(kind, values)
    margin = 64
    if packed:
        # null offsets: back to back, from the start of the buffer handed over
        offsets = np.cumsum([0] + [len(b) for b in bodies[:-1]]) + margin
        size = int(offsets[-1]) + len(bodies[-1]) + margin
        buf = np.full(size, SENTINEL, dtype=np.uint8)
        s3.cpu_chunk_body(parts, c, sigs, kind, arr, tsigs, out=buf[margin:])
    else:
        # gaps of 1, 2, ... bytes, and the bodies in reverse order
        offsets = np.zeros(len(bodies), dtype=np.int64)
        at = margin
        for i in reversed(range(len(bodies))):
            offsets[i] = at
            at += len(bodies[i]) + 1 + i
        size = at + margin
        buf = np.full(size, SENTINEL, dtype=np.uint8)
        s3.cpu_chunk_body(parts, c, sigs, kind, arr, tsigs, out=buf, body_offsets=offsets)
    want = _image(bodies, offsets, size)
    bad = np.flatnonzero(buf != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8].tolist()}"
    # the decoder gives the input back
    for p, o, b, v, i in zip(parts, offsets, bodies, values or [None] * len(parts), range(len(parts))):
        got = bref.parse(buf[o:o + len(b)].tobytes())
        assert b"".join(got["chunks"]) == p and [len(x) for x in got["chunks"]] == [len(x) for x in ref.cut(p, c)]
        first = sum(len(ref.cut(q, c)) + 1 for q in parts[:i])
        assert got["signatures"] == [r.tobytes().hex() for r in sigs[first:first + len(got["chunks"]) + 1]]
        if kind is None:
            assert got["trailer_line"] is None and got["trailer_signature"] is None
        else:
            assert got["trailer_line"] == tref.line_text(kind, v)
            assert got["trailer_signature"] == tsigs[i].tobytes().hex()


def test_the_decoder_rejects_malformed_bodies():
    body = bref.frame([b"x" * 20], 16, np.arange(16, dtype=np.uint32).reshape(2, 8).repeat(2, axis=0)[:3])[0]
    assert bref.parse(body)["chunks"] == [b"x" * 16, b"x" * 4]
    for bad in (body[:-1], body + b"\r", body.replace(b"10;", b"010;"), body.replace(b";chunk-sig", b";Chunk-sig"),
                body.replace(b"\r\n4;", b"\n4;"), body[:30] + b"A" + body[31:], body.replace(b"4;chunk", b"5;chunk")):
        with pytest.raises(ValueError):
            bref.parse(bad)


def _call(parts, lens, n, c, sigs, kind, values, tsigs, body):
    ptrs = (ctypes.c_void_p * max(1, len(parts)))(*[p.ctypes.data if p is not None else None for p in parts])
    return _native.lib().s3h_cpu_chunk_body(
        ptrs if parts else None, None if lens is None else lens.ctypes.data_as(_native.u64p), n, c,
        None if sigs is None else sigs.ctypes.data, kind, None if values is None else values.ctypes.data,
        None if tsigs is None else tsigs.ctypes.data, None if body is None else body.ctypes.data, None)


def test_argument_errors():
    part = np.zeros(100, dtype=np.uint8)
    lens = np.array([100], dtype=np.uint64)
    sigs = np.zeros((3, 8), dtype=np.uint32)
    vals, tsig = np.zeros(1, dtype=np.uint32), np.zeros((1, 8), dtype=np.uint32)
    body = np.full(1024, SENTINEL, dtype=np.uint8)
    E = _native.S3H_EINVAL
    assert _call([part], lens, 1, 64, sigs, -1, None, None, body) == _native.S3H_OK
    body[:] = SENTINEL
    assert _call([], lens, 1, 64, sigs, -1, None, None, body) == E            # null parts
    assert _call([part], None, 1, 64, sigs, -1, None, None, body) == E        # null lengths
    assert _call([part], lens, 1, 64, None, -1, None, None, body) == E        # null signatures
    assert _call([part], lens, 1, 64, sigs, -1, None, None, None) == E        # null body
    assert _call([None], lens, 1, 64, sigs, -1, None, None, body) == E        # a null part that is not empty
    assert _call([part], lens, 0, 64, sigs, -1, None, None, body) == E        # no parts
    assert _call([part], lens, 1, 0, sigs, -1, None, None, body) == E         # chunk_bytes 0
    assert _call([part], lens, 1, 64, sigs, -1, vals, None, body) == E        # values without a kind
    assert _call([part], lens, 1, 64, sigs, -1, None, tsig, body) == E
    assert _call([part], lens, 1, 64, sigs, 0, None, tsig, body) == E         # a kind without values
    assert _call([part], lens, 1, 64, sigs, 0, vals, None, body) == E         # ... without trailer signatures
    for kind in (-2, 5, 99):                                                  # unknown kinds
        assert _call([part], lens, 1, 64, sigs, kind, vals, tsig, body) == E
        assert _native.lib().s3h_chunk_body_geometry(lens.ctypes.data_as(_native.u64p), 1, 64, kind, None, None,
                                                     None) == E
    assert (body == SENTINEL).all(), "a refused call wrote"
    # the wrapper hands both mismatches to the library
    with pytest.raises(s3.S3HashError) as e:
        s3.cpu_chunk_body([part], 64, sigs, None, vals, None)
    assert e.value.code == E
    with pytest.raises(s3.S3HashError) as e:
        s3.cpu_chunk_body([part], 64, sigs, "crc32c", None, tsig)
    assert e.value.code == E
    with pytest.raises(s3.S3HashError) as e:
        s3.chunk_body_geometry([100], 0)
    assert e.value.code == E
    # an empty part may be null
    assert _call([None], np.array([0], dtype=np.uint64), 1, 64, sigs, -1, None, None, body) == _native.S3H_OK
    assert bref.parse(body[:86].tobytes())["chunks"] == []


@pytest.mark.parametrize("kind", tref.KINDS)
def test_the_text_functions_sit_where_the_rule_says(kind):
    # s3h_chunk_header_text / s3h_chunk_trailer_text and the assembler cannot drift apart
    c = 4096
    parts = grid_parts(c)
    sigs, values, tsigs, _ = grid_case(c, kind)
    arr = tref.to_array(kind, values)
    body = s3.cpu_chunk_body(parts, c, sigs, kind, arr, tsigs).tobytes()
    offs = s3.chunk_body_geometry([len(p) for p in parts], c, kind)["body_offsets"]
    row = 0
    for i, p in enumerate(parts):
        at = int(offs[i])
        for chunk in ref.cut(p, c) + [b""]:
            head = s3.chunk_header_text(len(chunk), sigs[row]).encode()
            assert len(head) == bref.hexlen(len(chunk)) + 83
            assert body[at:at + len(head)] == head
            at += len(head) + (len(chunk) + 2 if chunk else 0)
            row += 1
        text = s3.chunk_trailer_text(kind, arr[i], tsigs[i]).encode()
        assert len(text) == len(tref.line_text(kind, values[i])) + 94
        assert body[at:at + len(text)] == text
        assert at + len(text) == (int(offs[i + 1]) if i + 1 < len(parts) else len(body))
