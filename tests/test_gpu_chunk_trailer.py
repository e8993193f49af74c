"""SigV4 trailer signatures on the device: a trailer plan's launch (chunk hashes, chain, CRC plan,
sigv4_trailer_kernel), the trailer kernel alone, the one-shot call and the host-resident entry
point (s3h_chunk_plan_create_trailer / _launch_trailer / _trailer, s3h_chunk_sign_trailer_batch_*).

Expected values: hashlib + hmac + base64 and table CRCs from the definition
(tests/chunk_trailer_ref.py).  Bit-exact."""
import ctypes
import functools

import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests import chunk_sign_ref as ref
from tests import chunk_trailer_ref as tref

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5AA5A5
MARGIN = 64  # sentinel words behind every output


def _batch(seed, lens, gap=3):
    lens = np.asarray(lens, dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens + np.uint64(gap))[:-1]]).astype(np.uint64)
    rng = np.random.default_rng(seed)
    host = rng.integers(0, 256, int(offs[-1] + lens[-1]) + 64, dtype=np.uint8)
    seeds = rng.integers(0, 2**32, (len(lens), 8), dtype=np.uint32)
    return {"offs": offs, "lens": lens, "host": host, "seeds": seeds}


def _parts(b):
    return [b["host"][int(o):int(o) + int(n)].tobytes() for o, n in zip(b["offs"], b["lens"])]


def _words_per_value(kind):
    return 2 if kind == "crc64nvme" else 1


def _outputs(torch, plan, kind):
    """Signatures, checksums and trailer signatures, each followed by a sentinel margin."""
    sizes = (8 * plan.signatures, _words_per_value(kind) * plan.n, 8 * plan.n)
    return [torch.full((s + MARGIN,), SENTINEL, dtype=torch.int32, device="cuda") for s in sizes]


def _read(outs, plan, kind):
    """The three outputs as host arrays in the library's layout; the margins must be untouched."""
    got = []
    for t, words in zip(outs, (8 * plan.signatures, _words_per_value(kind) * plan.n, 8 * plan.n)):
        w = t.cpu().numpy().view(np.uint32)
        assert (w[words:] == SENTINEL).all(), "words behind an output were written"
        got.append(w[:words].copy())
    vals = got[1].view(np.uint64) if kind == "crc64nvme" else got[1]
    return got[0].reshape(-1, 8), vals, got[2].reshape(-1, 8)


def _check(got, want):
    for name, g, w in zip(("signatures", "checksums", "trailer signatures"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, name
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))
        assert bad.size == 0, f"{bad.size} of {len(w)} {name} differ, first rows {bad[:8].tolist()}"


def _launch(torch, b, chunk_bytes, kind, region="us-east-1", service="s3", seeds=None, plan=None, want=None):
    """One trailer launch: status OK, the three outputs equal to the reference's, margins
    untouched.  Returns the outputs."""
    key = ref.signing_key(ref.SECRET, ref.DATE, region, service)
    seeds = b["seeds"] if seeds is None else seeds
    if want is None:
        want = tref.expected(key, region, service, seeds, _parts(b), chunk_bytes, kind)
    data = torch.from_numpy(b["host"]).cuda()
    d_seeds = torch.from_numpy(seeds.view(np.int32)).cuda()
    own = plan is None
    plan = s3.ChunkSignPlan(b["offs"], b["lens"], chunk_bytes, trailer=kind) if own else plan
    try:
        assert plan.signatures == len(want[0])
        outs = _outputs(torch, plan, kind)
        with s3.ChunkSignContext(key, ref.TIMESTAMP, ref.DATE, region, service) as ctx:
            plan.launch_trailer(data, ctx, d_seeds, *outs)
            plan.status()
        got = _read(outs, plan, kind)
    finally:
        if own:
            plan.close()
    _check(got, want)
    return got


def test_known_answer(torch_cuda):
    b = {"offs": np.array([0], dtype=np.uint64), "lens": np.array([66560], dtype=np.uint64),
         "host": np.full(66560, ord("a"), dtype=np.uint8),
         "seeds": np.frombuffer(bytes.fromhex(tref.KNOWN_SEED), dtype=np.uint32).reshape(1, 8).copy()}
    sigs, vals, tsig = _launch(torch_cuda, b, 65536, "crc32c")
    assert tuple(r.tobytes().hex() for r in sigs) == tref.KNOWN_SIGNATURES
    assert s3.trailer_line_text("crc32c", vals[0]) == tref.KNOWN_LINE
    assert tsig.tobytes().hex() == tref.KNOWN_TRAILER_SIGNATURE


# 70 parts: the second workgroup is partial; 0-11 data chunks, some parts empty.  One batch for
# every case: the chunk signatures depend on the remainder alone, the checksums on the kind alone.
@functools.lru_cache(maxsize=None)
def _remainder_batch():
    lens = np.random.default_rng(70).integers(0, 701, 70)
    lens[:3] = [0, 64, 65]
    b = _batch(370, lens)
    return b, _parts(b)


@functools.lru_cache(maxsize=None)
def _remainder_signatures(r):
    region, service = ref.names_for(r)
    b, parts = _remainder_batch()
    return ref.signatures(ref.signing_key(ref.SECRET, ref.DATE, region, service), region, service,
                          b["seeds"], parts, 64)


@functools.lru_cache(maxsize=None)
def _remainder_values(kind):
    return tuple(tref.value_bytes(kind, p) for p in _remainder_batch()[1])


@pytest.mark.parametrize("kind", tref.CRC_KINDS)
@pytest.mark.parametrize("r", ref.REMAINDERS)
def test_prefix_remainders(torch_cuda, r, kind):
    region, service = ref.names_for(r)
    key = ref.signing_key(ref.SECRET, ref.DATE, region, service)
    b, parts = _remainder_batch()
    sigs, values = _remainder_signatures(r), _remainder_values(kind)
    ends = np.cumsum([len(ref.cut(p, 64)) + 1 for p in parts]) - 1
    want = (sigs, tref.to_array(kind, values),
            tref.trailer_signatures(key, region, service, sigs[ends], kind, values))
    _launch(torch_cuda, b, 64, kind, region, service, want=want)


def _sextet_values(bits):
    """Value k puts sextet k in every base64 character position (the last character holds the
    sextet's upper 2 bits of a 32-bit value, its upper 4 of a 64-bit one), then 0 and all ones."""
    vals = []
    for k in range(64):
        v = 0
        for sh in range(bits - 6, -6, -6):
            v |= k << sh if sh >= 0 else k >> -sh
        vals.append(v)
    return vals + [0, 2**bits - 1]


@pytest.mark.parametrize("kind", tref.CRC_KINDS)
def test_base64_alphabet(torch_cuda, kind):
    # the trailer kernel alone over caller-made values: 66 empty parts, so part p's last chunk
    # signature is row p
    torch = torch_cuda
    bits = 64 if kind == "crc64nvme" else 32
    ints = _sextet_values(bits)
    values = [v.to_bytes(bits // 8, "big") for v in ints]
    text = "".join(tref.line_text(kind, v).split(":")[1] for v in values)
    assert set(text) == set("ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/=")
    n = len(values)
    arr = tref.to_array(kind, values)
    lasts = np.random.default_rng(bits).integers(0, 2**32, (n, 8), dtype=np.uint32)
    key = ref.signing_key(ref.SECRET, ref.DATE, "us-east-1", "s3")
    d_sigs = torch.from_numpy(lasts.view(np.int32)).cuda()
    d_vals = torch.from_numpy(arr.view(np.int32)).cuda()
    out = torch.full((8 * n + MARGIN,), SENTINEL, dtype=torch.int32, device="cuda")
    with s3.ChunkSignPlan(np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), 64, trailer=kind) as plan, \
            s3.ChunkSignContext(key, ref.TIMESTAMP, ref.DATE, "us-east-1", "s3") as ctx:
        assert plan.signatures == n
        plan.trailer(ctx, d_sigs, d_vals, out)
        plan.status()
        cpu = s3.cpu_trailer_signatures(ctx, kind, arr, lasts)
    got = out.cpu().numpy().view(np.uint32)
    assert (got[8 * n:] == SENTINEL).all()
    got = got[:8 * n].reshape(-1, 8)
    bad = np.flatnonzero((got != cpu).any(axis=1))
    assert bad.size == 0, f"values {[hex(ints[i]) for i in bad[:8]]} sign differently on the CPU"
    assert np.array_equal(got, tref.trailer_signatures(key, "us-east-1", "s3", lasts, kind, values))


@pytest.mark.parametrize("n,kind", [(1, "crc32c"), (64, "crc32"), (65, "crc64nvme")])
def test_part_counts(torch_cuda, n, kind):
    # chunk size 100: chunks start at every alignment
    lens = np.random.default_rng(n).integers(0, 1200, n)
    _launch(torch_cuda, _batch(40 + n, lens), 100, kind)


@pytest.mark.parametrize("kind", tref.CRC_KINDS)
def test_only_empty_parts(torch_cuda, kind):
    _, vals, _ = _launch(torch_cuda, _batch(6, [0, 0, 0]), 64, kind)
    assert not vals.any()
    assert s3.trailer_line_text(kind, vals[0]).endswith(":AAAAAAAAAAA=" if kind == "crc64nvme" else ":AAAAAA==")


def test_one_shot_and_relaunch(torch_cuda):
    lens = np.random.default_rng(9).integers(0, 3000, 33)
    b = _batch(10, lens)
    key = ref.signing_key(ref.SECRET, ref.DATE, "us-east-1", "s3")
    other = np.random.default_rng(11).integers(0, 2**32, b["seeds"].shape, dtype=np.uint32)
    with s3.ChunkSignPlan(b["offs"], b["lens"], 256, trailer="crc64nvme") as plan:
        first = _launch(torch_cuda, b, 256, "crc64nvme", plan=plan)
        second = _launch(torch_cuda, b, 256, "crc64nvme", seeds=other, plan=plan)  # its own chains
        again = _launch(torch_cuda, b, 256, "crc64nvme", plan=plan)
    assert not np.array_equal(first[2], second[2]) and np.array_equal(first[1], second[1])
    _check(again, first)
    data = torch_cuda.from_numpy(b["host"]).cuda()
    with s3.ChunkSignContext(key, ref.TIMESTAMP, ref.DATE, "us-east-1", "s3") as ctx:
        shot = s3.chunk_sign_trailer_batch_device(data, b["offs"], b["lens"], 256, ctx, b["seeds"], "crc64nvme")
    _check(shot, first)


@pytest.mark.parametrize("kind", tref.CRC_KINDS)
def test_host_form_equals_device_form(torch_cuda, kind):
    # 33 pageable parts of 0-3,000 bytes at 256-byte chunks: the chunk CRCs are folded per part,
    # most last chunks are short
    rng = np.random.default_rng(13)
    lens = rng.integers(0, 3001, 33)
    lens[:3] = [0, 256, 257]
    b = _batch(14, lens, gap=0)
    device = _launch(torch_cuda, b, 256, kind)
    parts = [np.frombuffer(p, dtype=np.uint8) for p in _parts(b)]
    key = ref.signing_key(ref.SECRET, ref.DATE, "us-east-1", "s3")
    with s3.ChunkSignContext(key, ref.TIMESTAMP, ref.DATE, "us-east-1", "s3") as ctx:
        host = s3.chunk_sign_trailer_host(parts, 256, ctx, b["seeds"], kind)
    _check(host, device)


@pytest.mark.parametrize("kind", ["sha1", "sha256"])
def test_host_form_digest_checksums(torch_cuda, kind):
    # whole-part digests are the host form's alone (two-block line for SHA-256)
    rng = np.random.default_rng(15)
    parts = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in (0, 1, 255, 256, 1000)]
    seeds = rng.integers(0, 2**32, (5, 8), dtype=np.uint32)
    key = ref.signing_key(ref.SECRET, ref.DATE, "us-east-1", "s3")
    with s3.ChunkSignContext(key, ref.TIMESTAMP, ref.DATE, "us-east-1", "s3") as ctx:
        host = s3.chunk_sign_trailer_host(parts, 256, ctx, seeds, kind)
    _check(host, tref.expected(key, "us-east-1", "s3", seeds, [p.tobytes() for p in parts], 256, kind))


def test_plain_plan_refuses_and_trailer_plan_launches_plainly(torch_cuda):
    torch = torch_cuda
    b = _batch(12, [100, 200, 0])
    key = ref.signing_key(ref.SECRET, ref.DATE, "us-east-1", "s3")
    want = ref.signatures(key, "us-east-1", "s3", b["seeds"], _parts(b), 64)
    data = torch.from_numpy(b["host"]).cuda()
    d_seeds = torch.from_numpy(b["seeds"].view(np.int32)).cuda()
    kind = ctypes.c_int(-2)
    with s3.ChunkSignContext(key, ref.TIMESTAMP, ref.DATE, "us-east-1", "s3") as ctx:
        with s3.ChunkSignPlan(b["offs"], b["lens"], 64) as plain:
            outs = _outputs(torch, plain, "crc32c")
            with pytest.raises(s3.S3HashError) as e:
                plain.launch_trailer(data, ctx, d_seeds, *outs)
            assert e.value.code == _native.S3H_EINVAL
            with pytest.raises(s3.S3HashError) as e:
                plain.trailer(ctx, outs[0], outs[1], outs[2])
            assert e.value.code == _native.S3H_EINVAL
            plain.status()
            assert all((t.cpu().numpy().view(np.uint32) == SENTINEL).all() for t in outs)
            _native.check(_native.lib().s3h_chunk_plan_trailer_info(plain._h, ctypes.byref(kind)))
            assert kind.value == -1
        # a trailer plan's ordinary launch: the chunk signatures of a plain plan
        with s3.ChunkSignPlan(b["offs"], b["lens"], 64, trailer="crc32") as plan:
            out = torch.full((8 * plan.signatures + MARGIN,), SENTINEL, dtype=torch.int32, device="cuda")
            plan.launch(data, ctx, d_seeds, out)
            plan.status()
            _native.check(_native.lib().s3h_chunk_plan_trailer_info(plan._h, ctypes.byref(kind)))
            assert kind.value == _native.TRAILER_IDS["crc32"]
            assert plan.info()["signatures"] == len(want)
    got = out.cpu().numpy().view(np.uint32)
    assert (got[8 * len(want):] == SENTINEL).all()
    assert np.array_equal(got[:8 * len(want)].reshape(-1, 8), want)


@pytest.mark.parametrize("kind", ["sha1", "sha256"])
def test_digest_checksums_are_refused_on_the_device(torch_cuda, kind):
    b = _batch(16, [100, 200])
    with pytest.raises(s3.S3HashError) as e:
        s3.ChunkSignPlan(b["offs"], b["lens"], 64, trailer=kind)
    assert e.value.code == _native.S3H_EINVAL
    data = torch_cuda.from_numpy(b["host"]).cuda()
    with s3.ChunkSignContext(bytes(32), ref.TIMESTAMP, ref.DATE, "us-east-1", "s3") as ctx:
        with pytest.raises(s3.S3HashError) as e:
            s3.chunk_sign_trailer_batch_device(data, b["offs"], b["lens"], 64, ctx, b["seeds"], kind)
    assert e.value.code == _native.S3H_EINVAL


def test_launch_arguments(torch_cuda):
    torch = torch_cuda
    b = _batch(17, [100, 200])
    data = torch.from_numpy(b["host"]).cuda()
    seeds = torch.zeros(16, dtype=torch.int32, device="cuda")
    with s3.ChunkSignPlan(b["offs"], b["lens"], 64, trailer="crc64nvme") as plan, \
            s3.ChunkSignContext(bytes(32), ref.TIMESTAMP, ref.DATE, "us-east-1", "s3") as ctx:
        sigs, vals, tsig = _outputs(torch, plan, "crc64nvme")
        with pytest.raises(ValueError):
            plan.launch_trailer(data, ctx, seeds, sigs, vals[:3], tsig)  # 12 bytes for two 64-bit values
        with pytest.raises(ValueError):
            plan.launch_trailer(data, ctx, seeds, sigs, vals, tsig[:15])
        with pytest.raises(s3.S3HashError):
            plan.launch_trailer(data, ctx, seeds, sigs, vals.data_ptr() + 4, tsig)  # not 8-byte aligned
        with pytest.raises(s3.S3HashError):
            plan.launch_trailer(data, ctx, seeds, sigs, vals, tsig.data_ptr() + 4)  # not 16-byte aligned
        plan.status()
        # a refused launch starts nothing
        assert all((t.cpu().numpy().view(np.uint32) == SENTINEL).all() for t in (sigs, vals, tsig))
