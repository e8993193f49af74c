"""SigV4 chunk-signed uploads on the CPU (no GPU): the signing key, the chunk-signing context, the
signature chain over ready digests (s3h_cpu_chunk_signatures), the chunk geometry and the framing
line.  Expected values: hashlib + hmac from the definition (tests/chunk_sign_ref.py) and the AWS
documentation's example.  Bit-exact."""
import ctypes

import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests import chunk_sign_ref as ref


def _ctx(region="us-east-1", service="s3", key=None):
    key = ref.signing_key(ref.SECRET, ref.DATE, region, service) if key is None else key
    return key, s3.ChunkSignContext(key, ref.TIMESTAMP, ref.DATE, region, service)


def test_symbols_are_exported():
    L = _native.lib()
    for name in _native.C_ABI_SYMBOLS:
        if "chunk" in name or "sigv4" in name:
            assert hasattr(L, name), name
    assert L.s3h_api_version() == 2


def test_known_answer():
    key = s3.sigv4_signing_key(ref.SECRET, ref.DATE, "us-east-1", "s3")
    assert key.hex() == ref.KNOWN_KEY
    assert ref.signing_key(ref.SECRET, ref.DATE, "us-east-1", "s3") == key
    body = b"a" * 66560
    import hashlib
    digs = b"".join(hashlib.sha256(c).digest() for c in ref.cut(body, 65536))
    with s3.ChunkSignContext(key, ref.TIMESTAMP, ref.DATE, "us-east-1", "s3") as ctx:
        sig = s3.cpu_chunk_signatures(ctx, digs, [2], bytes.fromhex(ref.KNOWN_SEED))
    assert sig.shape == (3, 8) and sig.dtype == np.uint32
    assert tuple(row.tobytes().hex() for row in sig) == ref.KNOWN_SIGNATURES
    # the hmac reference reproduces the documentation's values too
    want = ref.signatures(key, "us-east-1", "s3", np.frombuffer(bytes.fromhex(ref.KNOWN_SEED), np.uint32),
                          [body], 65536)
    assert np.array_equal(sig, want)


@pytest.mark.parametrize("r", ref.REMAINDERS)
def test_prefix_remainders(r):
    region, service = ref.names_for(r)
    assert (66 + len(region) + len(service)) % 64 == r
    key, ctx = _ctx(region, service)
    rng = np.random.default_rng(1000 + r)
    counts = [0, 1, 5]
    digs = rng.integers(0, 256, (sum(counts), 32), dtype=np.uint8)
    seeds = rng.integers(0, 2**32, (3, 8), dtype=np.uint32)
    assert len({s.tobytes() for s in seeds}) == 3
    got = s3.cpu_chunk_signatures(ctx, digs, counts, seeds)
    want, at = [], 0
    for c, seed in zip(counts, seeds):
        want += ref.chain(key, region, service, seed.tobytes(), digs[at:at + c])
        at += c
    assert got.shape == (sum(counts) + 3, 8)
    assert got.tobytes() == b"".join(want)


def test_many_parts_over_the_host_threads():
    # more parts and links than one thread takes: every part's chain is its own
    key, ctx = _ctx()
    rng = np.random.default_rng(7)
    counts = rng.integers(0, 40, 97)
    digs = rng.integers(0, 256, (int(counts.sum()), 32), dtype=np.uint8)
    seeds = rng.integers(0, 2**32, (97, 8), dtype=np.uint32)
    got = s3.cpu_chunk_signatures(ctx, digs, counts, seeds)
    want, at = [], 0
    for c, seed in zip(counts, seeds):
        want += ref.chain(key, "us-east-1", "s3", seed.tobytes(), digs[at:at + int(c)])
        at += int(c)
    assert got.tobytes() == b"".join(want)


def test_geometry():
    c = 4096
    lens = [0, c - 1, c, c + 1, 3 * c]
    g = s3.chunk_geometry(lens, c)
    assert g["data_chunks_per_part"].tolist() == [0, 1, 1, 2, 3]
    # every part has one signature more than data chunks: a full last chunk is still followed
    # by the final 0-byte chunk, and an empty part has that one alone
    assert g["signature_offsets"].tolist() == [0, 1, 3, 5, 8]
    assert (g["data_chunks"], g["signatures"], g["max_chunks_per_part"]) == (7, 12, 3)
    for L, want in ((0, 0), (c - 1, 1), (c, 1), (c + 1, 2), (3 * c, 3)):
        one = s3.chunk_geometry([L], c)
        assert (one["data_chunks"], one["signatures"]) == (want, want + 1), L
    assert s3.chunk_geometry([5], 1)["signatures"] == 6  # any chunk_bytes >= 1 is ours to accept


def test_geometry_arguments():
    with pytest.raises(s3.S3HashError) as e:
        s3.chunk_geometry([10], 0)
    assert e.value.code == _native.S3H_EINVAL
    L = _native.lib()
    one = (ctypes.c_uint64 * 1)(10)
    assert L.s3h_chunk_geometry(None, 1, 64, None, None, None, None, None) == _native.S3H_EINVAL
    assert L.s3h_chunk_geometry(one, 0, 64, None, None, None, None, None) == _native.S3H_EINVAL
    assert L.s3h_chunk_geometry(one, 1, 64, None, None, None, None, None) == _native.S3H_OK
    big = (ctypes.c_uint64 * 1)(2**31 + 1)  # 2^31 + 1 one-byte chunks
    assert L.s3h_chunk_geometry(big, 1, 1, None, None, None, None, None) == _native.S3H_EINVAL
    # the plan and the batch calls refuse chunk_bytes = 0 before they look for a device
    h = ctypes.c_void_p()
    assert L.s3h_chunk_plan_create(0, one, one, 1, 0, ctypes.byref(h)) == _native.S3H_EINVAL
    assert not h.value
    assert L.s3h_chunk_plan_create(0, one, one, 1, 64, None) == _native.S3H_EINVAL
    assert L.s3h_chunk_plan_create(0, None, one, 1, 64, ctypes.byref(h)) == _native.S3H_EINVAL


@pytest.mark.parametrize("timestamp,date,region,service", [
    ("20130524T000000", ref.DATE, "us-east-1", "s3"),     # 15 bytes
    ("20130524T000000ZZ", ref.DATE, "us-east-1", "s3"),   # 17 bytes
    (ref.TIMESTAMP, "2013052", "us-east-1", "s3"),
    (ref.TIMESTAMP, "201305240", "us-east-1", "s3"),
    (ref.TIMESTAMP, ref.DATE, "", "s3"),
    (ref.TIMESTAMP, ref.DATE, "us-east-1", ""),
    (ref.TIMESTAMP, ref.DATE, "r" * 189, "s3"),           # prefix of 257 bytes
])
def test_context_arguments(timestamp, date, region, service):
    with pytest.raises(s3.S3HashError) as e:
        s3.ChunkSignContext(bytes(32), timestamp, date, region, service)
    assert e.value.code == _native.S3H_EINVAL


def test_longest_prefix_and_null_pointers():
    # 256 bytes is accepted (and signs like hmac does)
    region = "r" * 188
    key, ctx = _ctx(region, "s3")
    seed = np.arange(8, dtype=np.uint32)
    dig = np.arange(32, dtype=np.uint8)
    got = s3.cpu_chunk_signatures(ctx, dig, [1], seed)
    assert got.tobytes() == b"".join(ref.chain(key, region, "s3", seed.tobytes(), [dig.tobytes()]))
    L = _native.lib()
    h = ctypes.c_void_p()
    k = bytes(32)
    args = (ref.TIMESTAMP.encode(), ref.DATE.encode(), b"us-east-1", b"s3")
    assert L.s3h_chunk_sign_ctx_create(None, *args, ctypes.byref(h)) == _native.S3H_EINVAL
    assert L.s3h_chunk_sign_ctx_create(k, *args, None) == _native.S3H_EINVAL
    for i in range(4):
        bad = list(args)
        bad[i] = None
        assert L.s3h_chunk_sign_ctx_create(k, *bad, ctypes.byref(h)) == _native.S3H_EINVAL
        assert not h.value
    assert L.s3h_sigv4_signing_key(None, b"20130524", b"us-east-1", b"s3", ctypes.create_string_buffer(32)) \
        == _native.S3H_EINVAL
    counts = (ctypes.c_uint64 * 1)(1)
    buf = (ctypes.c_uint32 * 16)()
    assert L.s3h_cpu_chunk_signatures(None, buf, counts, 1, buf, buf) == _native.S3H_EINVAL
    assert L.s3h_cpu_chunk_signatures(ctx._h, None, counts, 1, buf, buf) == _native.S3H_EINVAL
    assert L.s3h_cpu_chunk_signatures(ctx._h, buf, None, 1, buf, buf) == _native.S3H_EINVAL
    assert L.s3h_cpu_chunk_signatures(ctx._h, buf, counts, 1, None, buf) == _native.S3H_EINVAL
    assert L.s3h_cpu_chunk_signatures(ctx._h, buf, counts, 1, buf, None) == _native.S3H_EINVAL
    assert L.s3h_chunk_sign_ctx_destroy(None) == _native.S3H_OK


def test_header_text():
    sig = bytes.fromhex(ref.KNOWN_SIGNATURES[0])
    assert s3.chunk_header_text(65536, sig) == "10000;chunk-signature=" + ref.KNOWN_SIGNATURES[0] + "\r\n"
    last = bytes.fromhex(ref.KNOWN_SIGNATURES[2])
    assert s3.chunk_header_text(0, last) == "0;chunk-signature=" + ref.KNOWN_SIGNATURES[2] + "\r\n"
    assert s3.chunk_header_text(2**64 - 1, sig).startswith("ffffffffffffffff;chunk-signature=")
    L = _native.lib()
    words = (ctypes.c_uint32 * 8)()
    small = ctypes.create_string_buffer(_native.CHUNK_HEADER_MAX - 1)
    assert L.s3h_chunk_header_text(1, words, small, len(small)) == _native.S3H_EINVAL
    assert L.s3h_chunk_header_text(1, None, ctypes.create_string_buffer(128), 128) == _native.S3H_EINVAL
