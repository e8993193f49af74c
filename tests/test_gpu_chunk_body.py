"""aws-chunked bodies on the device: chunk_body_kernel behind a chunk plan's launches
(s3h_chunk_plan_body / _body_info, s3h_chunk_body_batch_device).

Expected values: tests/chunk_body_ref.py, the rule in plain Python and its independent decoder.
The kernel only renders signatures, checksums and trailer signatures, so most tests feed it random
ones; the end-to-end tests run the signing launches in front of it on the same stream.  The output
buffer is pre-filled with 0xA5 and compared whole -- bodies, gaps and 256-byte margins -- with the
reference image.  Bit-exact."""
import base64
import functools

import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests import chunk_body_ref as bref
from tests import chunk_sign_ref as ref
from tests import chunk_trailer_ref as tref

pytestmark = pytest.mark.gpu
FILL = 0xA5
MARGIN = 256
FORMS = (None,) + tref.CRC_KINDS


def _batch(seed, lens, gap=3):
    lens = np.asarray(lens, dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens + np.uint64(gap))[:-1]]).astype(np.uint64)
    rng = np.random.default_rng(seed)
    host = rng.integers(0, 256, int(offs[-1] + lens[-1]) + 64, dtype=np.uint8)
    seeds = rng.integers(0, 2**32, (len(lens), 8), dtype=np.uint32)
    return {"offs": offs, "lens": lens, "host": host, "seeds": seeds}


def _parts(b):
    return [b["host"][int(o):int(o) + int(n)].tobytes() for o, n in zip(b["offs"], b["lens"])]


def _gapped(lengths, start=0, gap=5):
    """Body offsets with gaps between the bodies, the bodies in reverse order."""
    offs, at = np.zeros(len(lengths), dtype=np.uint64), start
    for i in reversed(range(len(lengths))):
        offs[i] = at
        at += int(lengths[i]) + gap + i % 7
    return offs, at


def _image(bodies, offsets, size):
    img = np.full(size, FILL, dtype=np.uint8)
    for b, o in zip(bodies, offsets):
        img[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return img


def _compare(buf, want):
    got = buf.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{bad.size} of {want.size} bytes differ, first at {bad[:8].tolist()}: "
                           f"got {got[bad[:8]].tolist()}, want {want[bad[:8]].tolist()}")


def _device_inputs(torch, kind, sigs, values, tsigs):
    d_sigs = torch.from_numpy(sigs.view(np.int32)).cuda()
    if kind is None:
        return d_sigs, None, None
    return (d_sigs, torch.from_numpy(tref.to_array(kind, values).view(np.int32)).cuda(),
            torch.from_numpy(tsigs.view(np.int32)).cuda())


def _render(torch, plan, data, kind, sigs, values, tsigs, bodies, offsets=None, shift=0, buf=None):
    """One body launch over given signatures into a 0xA5 buffer (bodies from byte MARGIN + shift,
    packed or at `offsets`), the whole buffer compared with the reference image."""
    lens = [len(b) for b in bodies]
    info = plan.body_info()
    assert info["body_lengths"].tolist() == lens and info["total"] == sum(lens)
    at = np.cumsum([0] + lens[:-1]) if offsets is None else np.asarray(offsets)
    extent = int(max(int(o) + n for o, n in zip(at, lens)))
    size = MARGIN + shift + extent + MARGIN
    if buf is None:
        buf = torch.empty(size, dtype=torch.uint8, device="cuda")
    assert buf.numel() >= size
    buf.fill_(FILL)
    d_sigs, d_vals, d_tsig = _device_inputs(torch, kind, sigs, values, tsigs)
    plan.body(data, d_sigs, buf[MARGIN + shift:], d_vals, d_tsig, body_offsets=offsets)
    plan.status()
    _compare(buf, _image(bodies, at + MARGIN + shift, buf.numel()))
    return buf


def _random_case(torch, seed, b, c, kind, offsets=None, shift=0):
    parts = _parts(b)
    sigs, values, tsigs = bref.random_inputs(np.random.default_rng(seed), parts, c, kind)
    bodies = bref.frame(parts, c, sigs, kind, values, tsigs)
    data = torch.from_numpy(b["host"]).cuda()
    with s3.ChunkSignPlan(b["offs"], b["lens"], c, trailer=kind) as plan:
        _render(torch, plan, data, kind, sigs, values, tsigs, bodies, offsets, shift)
    return bodies


# ---- 1. the AWS documentation's example
def _known(kind):
    b = {"offs": np.array([0], dtype=np.uint64), "lens": np.array([66560], dtype=np.uint64),
         "host": np.full(66560, ord("a"), dtype=np.uint8)}
    if kind is None:
        b["seeds"] = np.frombuffer(bytes.fromhex(ref.KNOWN_SEED), dtype=np.uint32).reshape(1, 8).copy()
        sigs = [bytes.fromhex(s) for s in ref.KNOWN_SIGNATURES]
        return b, bref.frame(_parts(b), 65536, sigs)[0]
    b["seeds"] = np.frombuffer(bytes.fromhex(tref.KNOWN_SEED), dtype=np.uint32).reshape(1, 8).copy()
    sigs = [bytes.fromhex(s) for s in tref.KNOWN_SIGNATURES]
    value = base64.b64decode(tref.KNOWN_LINE.split(":")[1])
    return b, bref.frame(_parts(b), 65536, sigs, "crc32c", [value], [bytes.fromhex(tref.KNOWN_TRAILER_SIGNATURE)])[0]


def _sign_and_frame(torch, b, c, kind, key, region="us-east-1", service="s3", offsets=None, extent=None):
    """launch / launch_trailer -> body on one stream with no synchronisation between, then status.
    Returns the 0xA5-filled buffer (bodies from byte MARGIN on)."""
    data = torch.from_numpy(b["host"]).cuda()
    d_seeds = torch.from_numpy(b["seeds"].view(np.int32)).cuda()
    with s3.ChunkSignPlan(b["offs"], b["lens"], c, trailer=kind) as plan, \
            s3.ChunkSignContext(key, ref.TIMESTAMP, ref.DATE, region, service) as ctx:
        total = plan.body_info()["total"] if extent is None else extent
        buf = torch.full((MARGIN + total + MARGIN,), FILL, dtype=torch.uint8, device="cuda")
        d_sigs = torch.zeros(8 * plan.signatures, dtype=torch.int32, device="cuda")
        if kind is None:
            plan.launch(data, ctx, d_seeds, d_sigs)
            plan.body(data, d_sigs, buf[MARGIN:], body_offsets=offsets)
        else:
            words = 2 if kind == "crc64nvme" else 1
            d_vals = torch.zeros(words * plan.n, dtype=torch.int32, device="cuda")
            d_tsig = torch.zeros(8 * plan.n, dtype=torch.int32, device="cuda")
            plan.launch_trailer(data, ctx, d_seeds, d_sigs, d_vals, d_tsig)
            plan.body(data, d_sigs, buf[MARGIN:], d_vals, d_tsig, body_offsets=offsets)
        plan.status()
    return buf


@pytest.mark.parametrize("kind,length", [("crc32c", 66946), (None, 66824)])
def test_known_answer(torch_cuda, kind, length):
    b, body = _known(kind)
    assert len(body) == length
    key = ref.signing_key(ref.SECRET, ref.DATE, "us-east-1", "s3")
    assert key.hex() == ref.KNOWN_KEY
    buf = _sign_and_frame(torch_cuda, b, 65536, kind, key)
    _compare(buf, _image([body], [MARGIN], buf.numel()))
    assert body.startswith(b"10000;chunk-signature=" + (tref if kind else ref).KNOWN_SIGNATURES[0].encode())


# ---- 2. every source alignment x every body alignment
def _aligned_batch(seed, lens):
    """256 parts: part 16 a + d starts at source offset a (mod 16); its body goes to offset d (mod 16)."""
    lens = np.asarray(lens, dtype=np.uint64)
    offs, at = [], 0
    for p, n in enumerate(lens):
        at = (at + 15) // 16 * 16 + p // 16
        offs.append(at)
        at += int(n) + 1
    rng = np.random.default_rng(seed)
    host = rng.integers(0, 256, at + 64, dtype=np.uint8)
    return {"offs": np.array(offs, dtype=np.uint64), "lens": lens, "host": host,
            "seeds": rng.integers(0, 2**32, (len(lens), 8), dtype=np.uint32)}


def _aligned_body_offsets(body_lengths):
    offs, at = [], 0
    for p, n in enumerate(body_lengths):
        at = (at + 15) // 16 * 16 + p % 16
        offs.append(at)
        at += int(n) + 1
    return np.array(offs, dtype=np.uint64)


@pytest.mark.parametrize("c,kind", [(64, None), (64, "crc32c"), (4099, None), (4099, "crc64nvme")])
def test_every_relative_alignment(torch_cuda, c, kind):
    rng = np.random.default_rng(c)
    # 64: 0-200 bytes, runs of every short length; 4099: the bulk path and its tile loop at every shift
    lens = rng.integers(0, 201, 256) if c == 64 else 3 * 4099 + rng.integers(0, 4099, 256)
    b = _aligned_batch(c + 1, lens)
    assert sorted(set((b["offs"] % 16).tolist())) == list(range(16))
    boffs = _aligned_body_offsets(s3.chunk_body_geometry(lens, c, kind)["body_lengths"])
    assert {(int(s) % 16, int(d) % 16) for s, d in zip(b["offs"], boffs)} == {(a, d) for a in range(16) for d in range(16)}
    _random_case(torch_cuda, c + 2, b, c, kind, offsets=boffs)


# ---- 3. the digits of the length: remainders whose hex length differs from the chunk's
@pytest.mark.parametrize("c", bref.CHUNK_BYTES)
def test_length_digit_edges(torch_cuda, c):
    torch = torch_cuda
    parts = bref.grid_parts(c)
    lens = np.array(bref.grid_lengths(c), dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens + np.uint64(3))[:-1]]).astype(np.uint64)
    host = np.zeros(int(offs[-1] + lens[-1]) + 64, dtype=np.uint8)
    for o, p in zip(offs, parts):
        host[int(o):int(o) + len(p)] = np.frombuffer(p, dtype=np.uint8)
    data = torch.from_numpy(host).cuda()
    for kind in FORMS:
        sigs, values, tsigs, bodies = bref.grid_case(c, kind)
        with s3.ChunkSignPlan(offs, lens, c, trailer=kind) as plan:
            offsets, _ = _gapped([len(x) for x in bodies])
            _render(torch, plan, data, kind, sigs, values, tsigs, bodies, offsets, shift=c % 16)


# ---- 4. the ends of a piece
def test_piece_edges(torch_cuda):
    with s3.ChunkSignPlan([0], [1], 1) as plan:
        P = plan.body_info()["piece_bytes"]
    assert P >= 1024
    for i, c in enumerate((P - 1, P, P + 1, 2 * P + 1)):
        # one chunk; two chunks and a last chunk of 1 byte; less than a chunk
        b = _batch(40 + i, [c, 2 * c + 1, P // 2 + 7, 1])
        with s3.ChunkSignPlan(b["offs"], b["lens"], c) as plan:
            per = -(-c // P)
            assert plan.body_info()["items"] == per + (2 * per + 1) + 1 + 1 + 4
        _random_case(torch_cuda, 50 + i, b, c, FORMS[i], shift=i + 1)


# ---- 5. more items than one pass of the grid
def test_more_items_than_one_grid_pass(torch_cuda):
    lens = np.zeros(5001, dtype=np.uint64)
    lens[2500] = 70000
    b = _batch(60, lens, gap=0)
    with s3.ChunkSignPlan(b["offs"], b["lens"], 1) as plan:
        info = plan.body_info()
        assert info["items"] == 70001 + 5000 and info["items"] > 4 * info["grid"]
        assert info["total"] == 70000 * 87 + 5001 * 86
    _random_case(torch_cuda, 61, b, 1, None)


# ---- 6. a plan without a data chunk
@pytest.mark.parametrize("kind", FORMS)
def test_only_empty_parts(torch_cuda, kind):
    bodies = _random_case(torch_cuda, 62, _batch(6, [0, 0, 0]), 64, kind, shift=3)
    assert all(bref.parse(x)["chunks"] == [] for x in bodies)


# ---- 7. offsets past 2^32
def test_past_4_gib(torch_cuda):
    torch = torch_cuda
    big = 2**32 + 4096
    rng = np.random.default_rng(63)
    # 3,000 bytes at 1,021-byte chunks: the body and its margins end inside the 4,096 bytes past 2^32
    part = rng.integers(0, 256, 3000, dtype=np.uint8)
    sigs, values, tsigs = bref.random_inputs(rng, [part.tobytes()], 1021, "crc32")
    body = bref.frame([part.tobytes()], 1021, sigs, "crc32", values, tsigs)[0]
    inputs = _device_inputs(torch, "crc32", sigs, values, tsigs)
    space = torch.empty(big, dtype=torch.uint8, device="cuda")  # never filled: only the touched ranges
    small = torch.from_numpy(part).cuda()
    # the body at 2^32 - 40 of the output
    at = 2**32 - 40
    lo, hi = at - MARGIN, at + len(body) + MARGIN
    assert hi <= big
    space[lo:hi] = FILL
    with s3.ChunkSignPlan([0], [3000], 1021, trailer="crc32") as plan:
        plan.body(small, inputs[0], space, inputs[1], inputs[2], body_offsets=[at])
        plan.status()
    _compare(space[lo:hi], _image([body], [MARGIN], hi - lo))
    # the part at 2^32 - 100 of the source
    src = 2**32 - 100
    space[src:src + 3000] = small
    out = torch.full((MARGIN + len(body) + MARGIN,), FILL, dtype=torch.uint8, device="cuda")
    with s3.ChunkSignPlan([src], [3000], 1021, trailer="crc32") as plan:
        plan.body(space, inputs[0], out[MARGIN:], inputs[1], inputs[2])
        plan.status()
    _compare(out, _image([body], [MARGIN], out.numel()))


# ---- 8. end to end: sign, frame, decode
@functools.lru_cache(maxsize=None)
def _ragged_batch():
    # 70 parts of 0-700 bytes at 64-byte chunks: 0-11 data chunks, some parts empty
    lens = np.random.default_rng(70).integers(0, 701, 70)
    lens[:3] = [0, 64, 65]
    b = _batch(370, lens)
    return b, _parts(b)


@functools.lru_cache(maxsize=None)
def _ragged_expected(kind):
    """From the definition: the signatures, and with a kind the checksum bytes and trailer
    signatures, and the bodies they frame."""
    b, parts = _ragged_batch()
    key = ref.signing_key(ref.SECRET, ref.DATE, "us-east-1", "s3")
    sigs = ref.signatures(key, "us-east-1", "s3", b["seeds"], parts, 64)
    if kind is None:
        return sigs, None, None, bref.frame(parts, 64, sigs)
    values = [tref.value_bytes(kind, p) for p in parts]
    ends = np.cumsum([len(ref.cut(p, 64)) + 1 for p in parts]) - 1
    tsigs = tref.trailer_signatures(key, "us-east-1", "s3", sigs[ends], kind, values)
    return sigs, values, tsigs, bref.frame(parts, 64, sigs, kind, values, tsigs)


@pytest.mark.parametrize("kind", FORMS)
def test_end_to_end(torch_cuda, kind):
    b, parts = _ragged_batch()
    sigs, values, tsigs, bodies = _ragged_expected(kind)
    key = ref.signing_key(ref.SECRET, ref.DATE, "us-east-1", "s3")
    offsets, extent = _gapped([len(x) for x in bodies])
    buf = _sign_and_frame(torch_cuda, b, 64, kind, key, offsets=offsets, extent=extent)
    host = buf.cpu().numpy()
    row = 0
    for i, (p, o, body) in enumerate(zip(parts, offsets, bodies)):
        got = bref.parse(host[MARGIN + int(o):MARGIN + int(o) + len(body)].tobytes())
        assert b"".join(got["chunks"]) == p
        assert got["signatures"] == [r.tobytes().hex() for r in sigs[row:row + len(got["signatures"])]]
        row += len(got["signatures"])
        if kind is not None:
            assert got["trailer_line"] == tref.line_text(kind, values[i])
            assert got["trailer_signature"] == tsigs[i].tobytes().hex()
    assert row == len(sigs)
    _compare(buf, _image(bodies, offsets + np.uint64(MARGIN), buf.numel()))


# ---- 9. nothing kept from a launch to the next
def test_same_plan_second_launch(torch_cuda):
    torch = torch_cuda
    b, parts = _ragged_batch()
    data = torch.from_numpy(b["host"]).cuda()
    with s3.ChunkSignPlan(b["offs"], b["lens"], 64, trailer="crc64nvme") as plan:
        lens = plan.body_info()["body_lengths"]
        first_offs, e1 = _gapped(lens, gap=5)
        second_offs, e2 = _gapped(lens, start=11, gap=9)
        buf = torch.empty(MARGIN + max(e1, e2) + MARGIN, dtype=torch.uint8, device="cuda")
        for seed, offsets in ((81, first_offs), (82, second_offs), (83, None)):
            sigs, values, tsigs = bref.random_inputs(np.random.default_rng(seed), parts, 64, "crc64nvme")
            bodies = bref.frame(parts, 64, sigs, "crc64nvme", values, tsigs)
            _render(torch, plan, data, "crc64nvme", sigs, values, tsigs, bodies, offsets, buf=buf)


# ---- 10. what a launch refuses, with nothing started
def test_refusals(torch_cuda):
    torch = torch_cuda
    b = _batch(90, [100, 200, 0])
    data = torch.from_numpy(b["host"]).cuda()
    buf = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    words = torch.zeros(8 * 16, dtype=torch.int32, device="cuda")

    def refused(call):
        with pytest.raises(s3.S3HashError) as e:
            call()
        assert e.value.code == _native.S3H_EINVAL
        torch.cuda.synchronize()
        assert bool((buf == FILL).all()) and bool((data.cpu() == torch.from_numpy(b["host"])).all())

    with s3.ChunkSignPlan(b["offs"], b["lens"], 64) as plain, \
            s3.ChunkSignPlan(b["offs"], b["lens"], 64, trailer="crc32c") as trailer:
        lens = plain.body_info()["body_lengths"]
        assert lens.tolist() == [151 + 123 + 86, 3 * 151 + 94 + 86, 86]
        # overlapping bodies: the second starts on the first's last byte; two at one place
        refused(lambda: plain.body(data, words, buf, body_offsets=[0, int(lens[0]) - 1, 2000]))
        refused(lambda: plain.body(data, words, buf, body_offsets=[0, 1000, 1000]))
        # the bodies' extent inside the parts' extent, and reaching into it from below
        refused(lambda: plain.body(data, words, data.data_ptr() + 10))
        refused(lambda: plain.body(buf.data_ptr() + 64, words, buf))
        # trailer inputs on a plain plan, none or one on a trailer plan
        refused(lambda: plain.body(data, words, buf, words, words))
        refused(lambda: plain.body(data, words, buf, words, None))
        refused(lambda: trailer.body(data, words, buf))
        refused(lambda: trailer.body(data, words, buf, words, None))
        refused(lambda: trailer.body(data, words, buf, None, words))
        # null pointers
        refused(lambda: plain.body(data, words, 0))
        refused(lambda: plain.body(data, 0, buf))
        refused(lambda: plain.body(0, words, buf))
        # the plans still work
        trailer.body(data, words, buf, words, words)
        plain.body(data, words, buf)
        plain.status()
    assert bref.parse(buf[:int(lens[0])].cpu().numpy().tobytes())["chunks"] == ref.cut(_parts(b)[0], 64)


# ---- 11. the one-shot call
@pytest.mark.parametrize("kind", FORMS)
def test_one_shot_call(torch_cuda, kind):
    b, parts = _ragged_batch()
    bodies = _ragged_expected(kind)[3]
    data = torch_cuda.from_numpy(b["host"]).cuda()
    key = ref.signing_key(ref.SECRET, ref.DATE, "us-east-1", "s3")
    with s3.ChunkSignContext(key, ref.TIMESTAMP, ref.DATE, "us-east-1", "s3") as ctx:
        packed = s3.chunk_body_batch_device(data, b["offs"], b["lens"], 64, ctx, b["seeds"], kind)
        assert packed.tobytes() == b"".join(bodies)
        offsets, extent = _gapped([len(x) for x in bodies], start=MARGIN)
        out = np.full(extent + MARGIN, FILL, dtype=np.uint8)
        s3.chunk_body_batch_device(data, b["offs"], b["lens"], 64, ctx, b["seeds"], kind, out=out, body_offsets=offsets)
        assert np.array_equal(out, _image(bodies, offsets, out.size))
        with pytest.raises(s3.S3HashError) as e:
            s3.chunk_body_batch_device(data, b["offs"], b["lens"], 64, ctx, b["seeds"], kind, out=out,
                                       body_offsets=np.zeros(len(bodies), dtype=np.uint64))
        assert e.value.code == _native.S3H_EINVAL
