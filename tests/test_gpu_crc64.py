"""Batched CRC-64/NVME of device-resident parts on the GPU (crc64_kernels.hip through the C-ABI):
whole-part launches and ranged ones.  Expected values come from s3h_cpu_crc64nvme (s3.crc64),
which tests/test_crc64_cpu.py pins to the NVMe vectors and a bitwise reference."""
import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests import crc_shapes

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5AA5A5C3C33C3C


def _expected(host, offs, lens):
    return np.array([s3.crc64(host[int(o):int(o) + int(n)]) for o, n in zip(offs, lens)], dtype=np.uint64)


def _words(t):
    return t.cpu().numpy().view(np.uint64)


def _gpu(torch, host, offs, lens):
    out = s3.crc64_batch_device(torch.from_numpy(host).cuda(), offs, lens)
    assert out.dtype == torch.int64 and tuple(out.shape) == (len(lens),)
    return _words(out)


def _check(got, want, offs, lens):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(i), int(offs[i]), int(lens[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]


def _sentinels(torch, n):
    return torch.from_numpy(np.full(n, SENTINEL, dtype=np.uint64).view(np.int64)).cuda()


def _ranges(cuts):
    return list(zip([0] + list(cuts[:-1]), cuts))


@pytest.fixture(scope="module")
def mixed_batch():
    """crc_shapes.mixed() with two fills (buffers A and B) and their expected CRCs."""
    offs, lens, size = crc_shapes.mixed()
    a, b = crc_shapes.fill("random", size + 64, 11), crc_shapes.fill("random", size + 64, 15)
    return {"offs": offs, "lens": lens, "a": a, "b": b,
            "want_a": _expected(a, offs, lens), "want_b": _expected(b, offs, lens)}


def test_boundary_batch(torch_cuda):
    """Every boundary length, and those around multiples of the plan's segment size, at each
    start alignment 0-15; all-zero and all-0xFF data expose a wrong init or length term."""
    S = 1 << 14
    # this batch is far below 8,192 segments at any size, so the plan always yields 16 KiB here
    # and the loop ends at once; the other sizes are pinned in tests/test_gpu_crc_sizes.py
    for _ in range(4):
        offs, lens, size = crc_shapes.boundary_layout(S)
        with s3.Crc64Plan(offs, lens) as plan:
            picked = plan.info()["segment_bytes"]
        if picked == S:
            break
        S = picked
    with s3.Crc64Plan(offs, lens) as plan:
        info = plan.info()
        assert info["segment_bytes"] == S and info["n"] == len(lens)
        assert info["segments"] == int(((lens + (S - 1)) // S).sum())
        for kind in ("random", "zeros", "ones"):
            host = crc_shapes.fill(kind, size, 12)
            data = torch_cuda.from_numpy(host).cuda()
            out = torch_cuda.empty(len(lens), dtype=torch_cuda.int64, device="cuda")
            plan.launch(data, out)
            torch_cuda.cuda.synchronize()
            _check(_words(out), _expected(host, offs, lens), offs, lens)


def test_segment_fold_of_one_large_part(torch_cuda):
    offs, lens, size = crc_shapes.segment_fold()
    host = crc_shapes.fill("random", size, 13)
    with s3.Crc64Plan(offs, lens) as plan:
        assert plan.info()["segments"] > 64  # more than one segment per stage-2 lane
    _check(_gpu(torch_cuda, host, offs, lens), _expected(host, offs, lens), offs, lens)


def test_many_small_parts(torch_cuda):
    """4,200 parts with 1-byte gaps: many stage-2 workgroups and a partial last one."""
    offs, lens, size = crc_shapes.many_small()
    host = crc_shapes.fill("random", size + 64, 14)
    _check(_gpu(torch_cuda, host, offs, lens), _expected(host, offs, lens), offs, lens)


def test_mixed_segment_counts(torch_cuda, mixed_batch):
    m = mixed_batch
    _check(_gpu(torch_cuda, m["a"], m["offs"], m["lens"]), m["want_a"], m["offs"], m["lens"])


def test_no_stale_partials(torch_cuda, mixed_batch):
    """One plan launched on buffer A, on B with the same layout, on A again: each result
    follows its own buffer."""
    m = mixed_batch
    offs, lens = m["offs"], m["lens"]
    a, b = torch_cuda.from_numpy(m["a"]).cuda(), torch_cuda.from_numpy(m["b"]).cuda()
    outs = [torch_cuda.empty(len(lens), dtype=torch_cuda.int64, device="cuda") for _ in range(3)]
    with s3.Crc64Plan(offs, lens) as plan:
        for buf, out in zip((a, b, a), outs):
            plan.launch(buf, out)
        torch_cuda.cuda.synchronize()
    for out, w in zip(outs, (m["want_a"], m["want_b"], m["want_a"])):
        _check(_words(out), w, offs, lens)


def test_verify_flags_exactly_the_flipped_part(torch_cuda, mixed_batch):
    m = mixed_batch
    host, offs, lens = m["a"], m["offs"], m["lens"]
    expected = torch_cuda.from_numpy(m["want_a"].view(np.int64)).cuda()
    data = torch_cuda.from_numpy(host).cuda()
    count, mask = s3.crc64_verify_batch_device(data, offs, lens, expected)
    assert count == 0 and not bool(mask.any())
    k = 137
    assert lens[k] > 0
    flipped = host.copy()
    flipped[int(offs[k]) + int(lens[k]) // 2] ^= 0x40
    count, mask = s3.crc64_verify_batch_device(torch_cuda.from_numpy(flipped).cuda(), offs, lens, expected)
    assert count == 1
    assert np.flatnonzero(mask.cpu().numpy()).tolist() == [k]


def test_offsets_past_4_gib(torch_cuda):
    """Parts that straddle and lie beyond byte 2^32 of the buffer (64-bit segment offsets); only
    the bytes the parts cover are initialised."""
    top = 1 << 32
    data = torch_cuda.empty(top + (1 << 20), dtype=torch_cuda.uint8, device="cuda")
    offs = np.array([top - 100_003, top + 7, top + 300_001], dtype=np.uint64)
    lens = np.array([200_005, 250_000, 70_001], dtype=np.uint64)
    lo, hi = int(offs[0]), int(offs[-1] + lens[-1])
    host = crc_shapes.fill("random", hi - lo, 17)
    data[lo:hi] = torch_cuda.from_numpy(host).cuda()
    got = _words(s3.crc64_batch_device(data, offs, lens))
    _check(got, _expected(host, offs - np.uint64(lo), lens), offs, lens)


def test_object_checksum_from_gpu_part_crcs(torch_cuda):
    """crc64_object of the GPU's part CRCs (5 ragged parts of the 8 MiB + 5 buffer, one empty)
    equals the CPU CRC of the whole buffer: the FULL_OBJECT x-amz-checksum-crc64nvme value."""
    _, _, size = crc_shapes.segment_fold()
    host = crc_shapes.fill("random", size, 16)
    total = size - 3
    cuts = [0, 1, 1 + (3 << 20) + 7, (5 << 20) + 123, (5 << 20) + 123, total]  # one empty part
    lens = np.diff(cuts).astype(np.uint64)
    offs = (3 + np.array(cuts[:-1])).astype(np.uint64)
    got = _gpu(torch_cuda, host, offs, lens)
    assert s3.crc64_object(got, lens) == s3.crc64(host[3:])
    assert s3.crc64_object(got.view(np.int64), lens) == s3.crc64(host[3:])


# ------------------------------------------------------------------ ranged launches
def test_ranged_equals_whole_and_writes_each_part_once(torch_cuda, mixed_batch):
    """Unequal ranges that do not align with segments: cuts inside pieces, on the segment grid
    and one byte off it.  After every launch exactly the parts that end in the range (and the
    empty part at begin 0) changed from the sentinel, and no later launch rewrites them."""
    torch = torch_cuda
    m = mixed_batch
    offs, lens, want = m["offs"], m["lens"], m["want_a"]
    data = torch.from_numpy(m["a"]).cuda()
    with s3.Crc64Plan(offs, lens) as plan:
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
            _check(got[due], want[due], offs[due], lens[due])
            out[torch.from_numpy(np.flatnonzero(due)).cuda()] = int(np.uint64(SENTINEL).view(np.int64))
        assert np.all(_words(out) == SENTINEL)  # nothing was rewritten after its own launch


def test_ranged_through_a_slot_buffer(torch_cuda, mixed_batch):
    """The host pipeline's layout: each range's bytes of part j at j * slice of a separate
    buffer, a plan on those offsets, byte_origin = byte_begin.  The 8 MiB part is cut 11 bytes
    short, so the last range is shorter than a slice and no multiple of 16."""
    torch = torch_cuda
    m = mixed_batch
    slice_bytes = 262144
    keep = 40  # the first parts of the batch, the 8 MiB one among them: a 10 MiB slot buffer
    offs, lens, want, host = m["offs"][:keep], m["lens"][:keep].copy(), m["want_a"][:keep].copy(), m["a"]
    n = len(lens)
    big = int(np.argmax(lens))
    lens[big] -= 11
    want[big] = _expected(host, offs[big:big + 1], lens[big:big + 1])[0]
    longest = int(lens.max())
    assert longest > 30 * slice_bytes and 0 < longest % slice_bytes and longest % slice_bytes % 16 != 0
    slot_offs = (np.arange(n, dtype=np.uint64) * np.uint64(slice_bytes))
    out = _sentinels(torch, n)
    with s3.Crc64Plan(slot_offs, lens) as plan:
        for begin in range(0, longest, slice_bytes):
            end = min(begin + slice_bytes, longest)
            slot = np.full(n * slice_bytes + 64, 0xEE, dtype=np.uint8)
            for j in np.flatnonzero(lens > begin):
                cnt = min(end, int(lens[j])) - begin
                slot[j * slice_bytes: j * slice_bytes + cnt] = host[int(offs[j]) + begin: int(offs[j]) + begin + cnt]
            plan.launch_range(torch.from_numpy(slot).cuda(), out, begin, end, byte_origin=begin)
        torch.cuda.synchronize()
    _check(_words(out), want, offs, lens)


def test_a_new_pass_from_zero_starts_clean(torch_cuda, mixed_batch):
    torch = torch_cuda
    m = mixed_batch
    offs, lens = m["offs"], m["lens"]
    A, B = torch.from_numpy(m["a"]).cuda(), torch.from_numpy(m["b"]).cuda()
    cuts = [5000, 30000, 70001, int(lens.max())]
    with s3.Crc64Plan(offs, lens) as plan:
        def full_pass(data):
            out = _sentinels(torch, len(lens))
            for begin, end in _ranges(cuts):
                plan.launch_range(data, out, begin, end)
            torch.cuda.synchronize()
            return _words(out)
        _check(full_pass(A), m["want_a"], offs, lens)
        _check(full_pass(B), m["want_b"], offs, lens)  # after a finished pass
        scratch = _sentinels(torch, len(lens))
        for begin, end in _ranges(cuts)[:2]:  # a pass on B, abandoned after two ranges
            plan.launch_range(B, scratch, begin, end)
        _check(full_pass(A), m["want_a"], offs, lens)
        # a whole-part launch between passes: the next ranged launch must begin at 0, and does
        whole = torch.empty(len(lens), dtype=torch.int64, device="cuda")
        plan.launch(A, whole)
        _check(_words(whole), m["want_a"], offs, lens)
        _check(full_pass(B), m["want_b"], offs, lens)


def test_order_errors_launch_nothing(torch_cuda, mixed_batch):
    torch = torch_cuda
    m = mixed_batch
    offs, lens = m["offs"], m["lens"]
    data = torch.from_numpy(m["a"]).cuda()
    with s3.Crc64Plan(offs, lens) as plan:
        out = _sentinels(torch, len(lens))
        plan.launch_range(data, out, 0, 100)
        torch.cuda.synchronize()
        before = _words(out).copy()
        for begin, end, origin in ((200, 300, 0), (100, 100, 0), (100, 50, 0), (100, 200, 101)):
            with pytest.raises(s3.S3HashError) as e:
                plan.launch_range(data, out, begin, end, origin)
            assert e.value.code == _native.S3H_EINVAL
        torch.cuda.synchronize()
        assert np.array_equal(_words(out), before)
        plan.launch_range(data, out, 100, int(lens.max()))  # the pass goes on where it was
        torch.cuda.synchronize()
    _check(_words(out), m["want_a"], offs, lens)


def test_many_small_parts_in_two_ranges(torch_cuda):
    """4,200 parts (a partial last stage-2 workgroup), about half ending in each range."""
    torch = torch_cuda
    offs, lens, size = crc_shapes.many_small()
    host = crc_shapes.fill("random", size + 64, 24)
    data = torch.from_numpy(host).cuda()
    want = _expected(host, offs, lens)
    out = _sentinels(torch, len(lens))
    with s3.Crc64Plan(offs, lens) as plan:
        plan.launch_range(data, out, 0, 1500)
        torch.cuda.synchronize()
        got = _words(out)
        first = lens <= 1500
        assert np.all(got[~first] == SENTINEL)
        _check(got[first], want[first], offs[first], lens[first])
        plan.launch_range(data, out, 1500, 3000)
        torch.cuda.synchronize()
    _check(_words(out), want, offs, lens)
