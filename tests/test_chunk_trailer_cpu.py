"""SigV4 trailer signatures on the CPU (no GPU): the context's trailer midstate and tail template
through s3h_cpu_trailer_signatures, the header line and the trailer framing.  Expected values:
hashlib + hmac + base64 from the definition (tests/chunk_trailer_ref.py) and the known answer in
the AWS documentation's setting.  Bit-exact."""
import ctypes
import hashlib

import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests import chunk_sign_ref as ref
from tests import chunk_trailer_ref as tref


def _ctx(region="us-east-1", service="s3"):
    key = ref.signing_key(ref.SECRET, ref.DATE, region, service)
    return key, s3.ChunkSignContext(key, ref.TIMESTAMP, ref.DATE, region, service)


def test_symbols_are_exported():
    L = _native.lib()
    for name in _native.C_ABI_SYMBOLS:
        if "trailer" in name:
            assert hasattr(L, name), name
    assert sum("trailer" in name for name in _native.C_ABI_SYMBOLS) == 9
    assert L.s3h_api_version() == 2


def test_reference_crcs():
    assert tref.crc64nvme(b"123456789") == 0xAE8B14860A799888
    assert tref.crc32c(b"123456789") == 0xE3069283
    assert tref.crc32c(b"") == 0 and tref.crc64nvme(b"") == 0


def test_known_answer():
    key, ctx = _ctx()
    body = b"a" * 66560
    digs = b"".join(hashlib.sha256(c).digest() for c in ref.cut(body, 65536))
    sig = s3.cpu_chunk_signatures(ctx, digs, [2], bytes.fromhex(tref.KNOWN_SEED))
    assert tuple(row.tobytes().hex() for row in sig) == tref.KNOWN_SIGNATURES
    crc = s3.crc(body, "crc32c")
    assert crc == tref.crc32c(body)
    assert s3.trailer_line_text("crc32c", crc) == tref.KNOWN_LINE
    got = s3.cpu_trailer_signatures(ctx, "crc32c", [crc], sig[2])
    assert got.shape == (1, 8) and got.dtype == np.uint32
    assert got.tobytes().hex() == tref.KNOWN_TRAILER_SIGNATURE
    # the hmac reference reproduces the value too
    want = tref.trailer_signature(key, "us-east-1", "s3", sig[2].tobytes(), "crc32c", crc.to_bytes(4, "big"))
    assert want.hex() == tref.KNOWN_TRAILER_SIGNATURE


@pytest.mark.parametrize("kind", tref.KINDS)
@pytest.mark.parametrize("r", ref.REMAINDERS)
def test_prefix_remainders(r, kind):
    region, service = ref.names_for(r)
    assert (66 + len(region) + len(service)) % 64 == r
    key, ctx = _ctx(region, service)
    rng = np.random.default_rng(2000 + r)
    parts = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (0, 1, 9, 64, 300)]
    values = [tref.value_bytes(kind, p) for p in parts]
    lasts = rng.integers(0, 2**32, (5, 8), dtype=np.uint32)
    got = s3.cpu_trailer_signatures(ctx, kind, tref.to_array(kind, values), lasts)
    assert np.array_equal(got, tref.trailer_signatures(key, region, service, lasts, kind, values))
    for p, v in zip(parts, values):
        assert s3.trailer_line_text(kind, tref.to_array(kind, [v])) == tref.line_text(kind, v)


def test_many_parts_over_the_host_threads():
    key, ctx = _ctx()
    rng = np.random.default_rng(8)
    n = 1000
    values = [bytes(v) for v in rng.integers(0, 256, (n, 8), dtype=np.uint8)]
    lasts = rng.integers(0, 2**32, (n, 8), dtype=np.uint32)
    got = s3.cpu_trailer_signatures(ctx, "crc64nvme", tref.to_array("crc64nvme", values), lasts)
    assert np.array_equal(got, tref.trailer_signatures(key, "us-east-1", "s3", lasts, "crc64nvme", values))


def test_empty_values_text():
    assert s3.trailer_line_text("crc32", 0) == "x-amz-checksum-crc32:AAAAAA=="
    assert s3.trailer_line_text("crc64nvme", 0) == "x-amz-checksum-crc64nvme:AAAAAAAAAAA="
    assert s3.trailer_line_text("crc32c", 0xFFFFFFFF) == "x-amz-checksum-crc32c://///w=="
    assert s3.trailer_line_text("crc64nvme", 2**64 - 1) == "x-amz-checksum-crc64nvme://////////8="


@pytest.mark.parametrize("kind", tref.KINDS)
def test_trailer_text(kind):
    value = tref.value_bytes(kind, b"trailer")
    sig = bytes.fromhex(tref.KNOWN_TRAILER_SIGNATURE)
    text = s3.chunk_trailer_text(kind, tref.to_array(kind, [value]), sig)
    assert text == (tref.line_text(kind, value) + "\r\nx-amz-trailer-signature:" +
                    tref.KNOWN_TRAILER_SIGNATURE + "\r\n\r\n")
    assert len(text) < _native.CHUNK_TRAILER_MAX
    assert len(tref.line_text(kind, value)) < _native.TRAILER_LINE_MAX


def test_arguments():
    _, ctx = _ctx()
    L = _native.lib()
    EINVAL = _native.S3H_EINVAL
    vals = (ctypes.c_uint64 * 8)()
    words = (ctypes.c_uint32 * 8)()
    out = (ctypes.c_uint32 * 8)()
    assert L.s3h_cpu_trailer_signatures(ctx._h, 0, vals, words, 1, out) == _native.S3H_OK
    for kind in (-1, 5, 99):
        assert L.s3h_cpu_trailer_signatures(ctx._h, kind, vals, words, 1, out) == EINVAL
        assert L.s3h_trailer_line_text(kind, vals, ctypes.create_string_buffer(128), 128) == EINVAL
        assert L.s3h_chunk_trailer_text(kind, vals, words, ctypes.create_string_buffer(256), 256) == EINVAL
    assert L.s3h_cpu_trailer_signatures(None, 0, vals, words, 1, out) == EINVAL
    assert L.s3h_cpu_trailer_signatures(ctx._h, 0, None, words, 1, out) == EINVAL
    assert L.s3h_cpu_trailer_signatures(ctx._h, 0, vals, None, 1, out) == EINVAL
    assert L.s3h_cpu_trailer_signatures(ctx._h, 0, vals, words, 1, None) == EINVAL
    assert L.s3h_cpu_trailer_signatures(ctx._h, 0, vals, words, 0, out) == EINVAL
    buf = ctypes.create_string_buffer(256)
    assert L.s3h_trailer_line_text(0, None, buf, 256) == EINVAL
    assert L.s3h_trailer_line_text(0, vals, None, 256) == EINVAL
    assert L.s3h_trailer_line_text(0, vals, buf, _native.TRAILER_LINE_MAX - 1) == EINVAL
    assert L.s3h_trailer_line_text(0, vals, buf, _native.TRAILER_LINE_MAX) == _native.S3H_OK
    assert L.s3h_chunk_trailer_text(0, None, words, buf, 256) == EINVAL
    assert L.s3h_chunk_trailer_text(0, vals, None, buf, 256) == EINVAL
    assert L.s3h_chunk_trailer_text(0, vals, words, None, 256) == EINVAL
    assert L.s3h_chunk_trailer_text(0, vals, words, buf, _native.CHUNK_TRAILER_MAX - 1) == EINVAL
    assert L.s3h_chunk_trailer_text(0, vals, words, buf, _native.CHUNK_TRAILER_MAX) == _native.S3H_OK
    with pytest.raises(ValueError):
        s3.trailer_line_text("md5", 0)
    # the plan and the batch calls refuse a digest or unknown kind before they look for a device
    one = (ctypes.c_uint64 * 1)(10)
    h = ctypes.c_void_p()
    for kind in (3, 4, 5, -1):
        assert L.s3h_chunk_plan_create_trailer(0, kind, one, one, 1, 64, ctypes.byref(h)) == EINVAL
        assert not h.value
    assert L.s3h_chunk_plan_create_trailer(0, 0, one, one, 1, 64, None) == EINVAL
    assert L.s3h_chunk_plan_create_trailer(0, 0, one, one, 1, 0, ctypes.byref(h)) == EINVAL
    assert L.s3h_chunk_plan_trailer_info(None, None) == EINVAL
