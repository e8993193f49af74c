"""Ranged (resumable) CRC launches on the GPU (s3h_crc_plan_launch_range: crc_range_pieces_kernel
and crc_range_parts_kernel) against whole-part values.  Expected values: CRC-32 from zlib.crc32,
CRC-32C from s3h_cpu_crc (pinned by tests/test_crc_cpu.py)."""
import zlib

import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests import crc_shapes

pytestmark = pytest.mark.gpu
ALGOS = ("crc32c", "crc32")
SENTINEL = 0x5A5AA5A5


def _expected(host, offs, lens, algo):
    one = (lambda b: zlib.crc32(b)) if algo == "crc32" else (lambda b: s3.crc(b, "crc32c"))
    return np.array([one(host[int(o):int(o) + int(n)].tobytes()) for o, n in zip(offs, lens)],
                    dtype=np.uint32)


def _check(got, want, lens):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(i), int(lens[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]


def _sentinels(torch, n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")


def _words(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def mixed_batch():
    """crc_shapes.mixed() with two fills (buffers A and B) and their expected CRCs."""
    offs, lens, size = crc_shapes.mixed()
    a, b = crc_shapes.fill("random", size + 64, 21), crc_shapes.fill("random", size + 64, 22)
    return {"offs": offs, "lens": lens, "a": a, "b": b,
            "want_a": {g: _expected(a, offs, lens, g) for g in ALGOS},
            "want_b": {g: _expected(b, offs, lens, g) for g in ALGOS}}


def _ranges(cuts):
    return list(zip([0] + list(cuts[:-1]), cuts))


@pytest.mark.parametrize("algo", ALGOS)
def test_ranged_equals_whole_on_resident_data(torch_cuda, mixed_batch, algo):
    """Origin 0, cuts inside pieces, on the segment grid and one byte off it.  After every
    launch exactly the parts that end in the range (and the empty part at begin 0) changed, and
    no later launch rewrites them."""
    torch = torch_cuda
    offs, lens, want = mixed_batch["offs"], mixed_batch["lens"], mixed_batch["want_a"][algo]
    data = torch.from_numpy(mixed_batch["a"]).cuda()
    with s3.CrcPlan(offs, lens, algo=algo) as plan:
        S = plan.info()["segment_bytes"]
        cuts = sorted({1, 17, 4096, S - 1, S, S + 1, 2 * S + 5, 65539, (1 << 20) + 3, int(lens.max())})
        out = _sentinels(torch, len(lens))
        for begin, end in _ranges(cuts):
            plan.launch_range(data, out, begin, end)
            torch.cuda.synchronize()
            got = _words(out)
            due = ((lens > begin) & (lens <= end)) | ((lens == 0) & (begin == 0))
            changed = got != SENTINEL
            assert np.array_equal(changed, due), (begin, end, np.flatnonzero(changed != due)[:8])
            _check(got[due], want[due], lens[due])
            out[torch.from_numpy(np.flatnonzero(due)).cuda()] = SENTINEL
        assert np.all(_words(out) == SENTINEL)  # nothing was rewritten after its own launch


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("slice_bytes", (4096, 262144))
def test_ranged_equals_whole_through_a_slot_buffer(torch_cuda, mixed_batch, algo, slice_bytes):
    """The host pipeline's layout: each range's bytes of part j at j * slice of a separate
    buffer, a plan on those offsets, byte_origin = byte_begin.  The 8 MiB part is cut 11 bytes
    short, so the last range is shorter than a slice and no multiple of 16."""
    torch = torch_cuda
    offs, lens, want = mixed_batch["offs"], mixed_batch["lens"].copy(), mixed_batch["want_a"][algo].copy()
    host, n = mixed_batch["a"], len(lens)
    big = int(np.argmax(lens))
    lens[big] -= 11
    want[big] = _expected(host, offs[big:big + 1], lens[big:big + 1], algo)[0]
    longest = int(lens.max())
    assert 0 < longest % slice_bytes and longest % slice_bytes % 16 != 0
    slot_offs = (np.arange(n, dtype=np.uint64) * np.uint64(slice_bytes))
    out = _sentinels(torch, n)
    with s3.CrcPlan(slot_offs, lens, algo=algo) as plan:
        for begin in range(0, longest, slice_bytes):
            end = min(begin + slice_bytes, longest)
            slot = np.full(n * slice_bytes + 64, 0xEE, dtype=np.uint8)
            for j in np.flatnonzero(lens > begin):
                cnt = min(end, int(lens[j])) - begin
                slot[j * slice_bytes: j * slice_bytes + cnt] = host[int(offs[j]) + begin: int(offs[j]) + begin + cnt]
            plan.launch_range(torch.from_numpy(slot).cuda(), out, begin, end, byte_origin=begin)
        torch.cuda.synchronize()
    _check(_words(out), want, lens)


@pytest.mark.parametrize("algo", ALGOS)
def test_restart_after_an_abandoned_pass(torch_cuda, mixed_batch, algo):
    torch = torch_cuda
    offs, lens = mixed_batch["offs"], mixed_batch["lens"]
    A, B = torch.from_numpy(mixed_batch["a"]).cuda(), torch.from_numpy(mixed_batch["b"]).cuda()
    cuts = [5000, 30000, 70001, int(lens.max())]
    with s3.CrcPlan(offs, lens, algo=algo) as plan:
        def full_pass(data):
            out = _sentinels(torch, len(lens))
            for begin, end in _ranges(cuts):
                plan.launch_range(data, out, begin, end)
            torch.cuda.synchronize()
            return _words(out)
        _check(full_pass(A), mixed_batch["want_a"][algo], lens)
        scratch = _sentinels(torch, len(lens))
        for begin, end in _ranges(cuts)[:2]:  # a pass on B, abandoned after two ranges
            plan.launch_range(B, scratch, begin, end)
        _check(full_pass(A), mixed_batch["want_a"][algo], lens)
        _check(full_pass(B), mixed_batch["want_b"][algo], lens)
        # a whole-part launch between passes: the next ranged launch must begin at 0, and does
        whole = torch.empty(len(lens), dtype=torch.int32, device="cuda")
        plan.launch(A, whole)
        _check(_words(whole), mixed_batch["want_a"][algo], lens)
        _check(full_pass(B), mixed_batch["want_b"][algo], lens)


@pytest.mark.parametrize("algo", ALGOS)
def test_order_errors_launch_nothing(torch_cuda, mixed_batch, algo):
    torch = torch_cuda
    offs, lens, want = mixed_batch["offs"], mixed_batch["lens"], mixed_batch["want_a"][algo]
    data = torch.from_numpy(mixed_batch["a"]).cuda()
    longest = int(lens.max())
    with s3.CrcPlan(offs, lens, algo=algo) as plan:
        out = _sentinels(torch, len(lens))
        plan.launch_range(data, out, 0, 100)
        torch.cuda.synchronize()
        before = _words(out).copy()
        for begin, end, origin in ((200, 300, 0),      # does not continue the previous range
                                   (100, 100, 0),      # empty
                                   (100, 50, 0),       # backwards
                                   (100, 200, 101)):   # origin past the range's first byte
            with pytest.raises(s3.S3HashError) as e:
                plan.launch_range(data, out, begin, end, origin)
            assert e.value.code == _native.S3H_EINVAL
        torch.cuda.synchronize()
        assert np.array_equal(_words(out), before)
        plan.launch_range(data, out, 100, longest)  # the pass goes on where it was
        torch.cuda.synchronize()
    _check(_words(out), want, lens)


@pytest.mark.parametrize("algo", ALGOS)
def test_one_large_part_in_ranges_of_many_pieces(torch_cuda, algo):
    torch = torch_cuda
    offs, lens, size = crc_shapes.segment_fold()
    host = crc_shapes.fill("random", size, 23)
    data = torch.from_numpy(host).cuda()
    step, L = (1 << 20) + 1, int(lens[0])
    out = _sentinels(torch, 1)
    with s3.CrcPlan(offs, lens, algo=algo) as plan:
        assert step > 2 * plan.info()["segment_bytes"]
        for begin in range(0, L, step):
            plan.launch_range(data, out, begin, min(begin + step, L))
        torch.cuda.synchronize()
    _check(_words(out), _expected(host, offs, lens, algo), lens)


@pytest.mark.parametrize("algo", ALGOS)
def test_many_small_parts_in_two_ranges(torch_cuda, algo):
    """4,200 parts (a partial last stage-2 workgroup), about half ending in each range."""
    torch = torch_cuda
    offs, lens, size = crc_shapes.many_small()
    host = crc_shapes.fill("random", size + 64, 24)
    data = torch.from_numpy(host).cuda()
    want = _expected(host, offs, lens, algo)
    out = _sentinels(torch, len(lens))
    with s3.CrcPlan(offs, lens, algo=algo) as plan:
        plan.launch_range(data, out, 0, 1500)
        torch.cuda.synchronize()
        got = _words(out)
        first = lens <= 1500
        assert 1500 < int(first.sum()) < 2700
        assert np.all(got[~first] == SENTINEL)
        _check(got[first], want[first], lens[first])
        plan.launch_range(data, out, 1500, 3000)
        torch.cuda.synchronize()
    _check(_words(out), want, lens)
