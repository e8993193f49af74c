"""CRC launches at each of the plan's five segment sizes and past one grid pass of stage 1, for
CRC-32C, CRC-32 and CRC-64/NVME, whole-part and ranged.  The plan picks its geometry from the
batch (crc.cpp: pick_log2_segment, seg_grid), so each geometry is reached by composing the batch:
crc_shapes.sized_layout(14..18) lands on 16-256 KiB, two_pass_16k() on 16 KiB with 12,100
segments, many_small(n=20000) on 256 KiB with 20,000 one-tile segments; every test asserts the
plan's own segment_bytes / segments / grid first (tests/test_crc_sizes_cpu.py holds the layouts'
arithmetic).  Expected values: CRC-32 from zlib.crc32, CRC-32C and CRC-64/NVME from s3.crc /
s3.crc64, which tests/test_crc_cpu.py and test_crc64_cpu.py pin to known answers and bitwise
references.  Every comparison is bit-exact and covers every part."""
import zlib

import numpy as np
import pytest

import s3client_amd as s3
from tests import crc_shapes
from tests.crc_shapes import sized_cuts

pytestmark = pytest.mark.gpu
ALGOS = ("crc32c", "crc32", "crc64nvme")
LOG2S = (14, 15, 16, 17, 18)
SENTINEL = {4: 0x5A5AA5A5, 8: 0x5A5AA5A5C3C33C3C}


def _wide(algo):
    return algo == "crc64nvme"


def _plan(offs, lens, algo):
    return s3.Crc64Plan(offs, lens) if _wide(algo) else s3.CrcPlan(offs, lens, algo=algo)


def _np_type(algo):
    return np.uint64 if _wide(algo) else np.uint32


def _words(t, algo):
    return t.cpu().numpy().view(_np_type(algo))


def _signed(a):
    """The same words as torch's signed type of that width."""
    return a.view(np.int64 if a.itemsize == 8 else np.int32)


def _out(torch, n, algo, sentinel=False):
    """n result words on the device, filled with the sentinel when asked."""
    if not sentinel:
        return torch.empty(n, dtype=torch.int64 if _wide(algo) else torch.int32, device="cuda")
    dt = _np_type(algo)
    return torch.from_numpy(_signed(np.full(n, SENTINEL[np.dtype(dt).itemsize], dtype=dt))).cuda()


def _expected(host, offs, lens, algo):
    one = {"crc32": zlib.crc32, "crc32c": lambda b: s3.crc(b, "crc32c"), "crc64nvme": s3.crc64}[algo]
    return np.array([one(host[int(o):int(o) + int(n)]) for o, n in zip(offs, lens)], dtype=_np_type(algo))


def _check(got, want, offs, lens):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(i), int(offs[i]), int(lens[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]


class _Batch:
    """One layout: its random and all-0xFF fills and, per (fill, algo), the expected values --
    each made once, on first use."""

    def __init__(self, layout, seed):
        self.offs, self.lens, self.size = layout
        self.seed = seed
        self._host, self._want = {}, {}

    def host(self, kind="random"):
        if kind not in self._host:
            self._host[kind] = crc_shapes.fill(kind, self.size + 64, self.seed)
        return self._host[kind]

    def want(self, algo, kind="random"):
        if (algo, kind) not in self._want:
            self._want[algo, kind] = _expected(self.host(kind), self.offs, self.lens, algo)
        return self._want[algo, kind]

    def segments(self, S):
        return crc_shapes.segment_count(self.lens, S)


@pytest.fixture(scope="module")
def batches():
    """name -> _Batch, laid out on first use: 14..18 = sized_layout, "two_pass", "small"."""
    cache = {}

    def get(name):
        if name not in cache:
            if name == "two_pass":
                cache[name] = _Batch(crc_shapes.two_pass_16k(), 41)
            elif name == "small":
                cache[name] = _Batch(crc_shapes.many_small(n=20000), 42)
            else:
                cache[name] = _Batch(crc_shapes.sized_layout(name), 30 + name)
        return cache[name]
    return get


def _ranged_pass(torch, plan, data, b, algo, cuts, shifted=False):
    """Ranges [0, c1), [c1, c2), ... on one plan.  After every launch exactly the parts that
    end in the range (and the empty ones at begin 0) left the sentinel, with their whole-part
    values, and no later launch rewrites them.  `shifted`: byte_origin = byte_begin with the
    view data[begin:] as the base -- the same bytes through a base pointer of another
    alignment at every cut."""
    offs, lens, want = b.offs, b.lens, b.want(algo)
    sentinel = np.array(SENTINEL[want.itemsize], dtype=want.dtype)
    out = _out(torch, len(lens), algo, sentinel=True)
    for begin, end in zip([0] + list(cuts[:-1]), cuts):
        if shifted:
            plan.launch_range(data[begin:], out, begin, end, byte_origin=begin)
        else:
            plan.launch_range(data, out, begin, end)
        torch.cuda.synchronize()
        got = _words(out, algo)
        due = ((lens > begin) & (lens <= end)) | ((lens == 0) & (begin == 0))
        changed = got != sentinel
        assert np.array_equal(changed, due), (begin, end, np.flatnonzero(changed != due)[:8])
        _check(got[due], want[due], offs[due], lens[due])
        out[torch.from_numpy(np.flatnonzero(due)).cuda()] = int(_signed(sentinel))
    assert np.all(_words(out, algo) == sentinel)  # nothing was rewritten after its own launch
    assert int(cuts[-1]) >= int(lens.max())       # (the pass covered every part)


def _whole_launch(torch, plan, data, b, algo, kind="random"):
    """A whole-part launch over the `kind` fill, checked.  It also leaves that fill's segment
    values in the plan's partials: run over "ones" ahead of a ranged pass over the random
    data, a piece value the pass fails to write cannot be right by being left over."""
    out = _out(torch, len(b.lens), algo)
    plan.launch(data, out)
    torch.cuda.synchronize()
    _check(_words(out, algo), b.want(algo, kind), b.offs, b.lens)


@pytest.mark.parametrize("log2s", LOG2S)
@pytest.mark.parametrize("algo", ALGOS)
def test_whole_launch_at_each_segment_size(torch_cuda, batches, algo, log2s):
    """x^(8S) in stage 2, 16..257 tiles per segment in stage 1, and (from 32 KiB up) a second
    grid pass; all-0xFF data and random (each launch finds the other fill's segment values in
    the plan's partials, or another plan's: a segment that is not written shows)."""
    torch = torch_cuda
    b = batches(log2s)
    with _plan(b.offs, b.lens, algo) as plan:
        info = plan.info()
        assert info["segment_bytes"] == 1 << log2s and info["n"] == len(b.lens)
        assert info["segments"] == b.segments(1 << log2s)
        if log2s >= 15:
            assert info["segments"] > 8 * info["grid"]
        for kind in ("ones", "random"):
            _whole_launch(torch, plan, torch.from_numpy(b.host(kind)).cuda(), b, algo, kind)


@pytest.mark.parametrize("log2s", LOG2S)
@pytest.mark.parametrize("algo", ALGOS)
def test_ranged_at_each_segment_size(torch_cuda, batches, algo, log2s):
    """piece_of / part_range / range_pieces at each segment size: cuts on the segment grid, one
    byte off it and deep inside the 67-segment part (up to 62 pieces per part in one launch,
    most of them empty), with origin 0 and then with byte_origin = byte_begin.  No launch of
    that cut list holds more than 64 pieces of a part, so stage 2 never multiplies by x^(8S)
    there; a third pass cut at byte 1 alone does: 67 pieces of the long part in one launch, the
    first short in front, folded in runs of two."""
    torch = torch_cuda
    b = batches(log2s)
    S = 1 << log2s
    data, ones = torch.from_numpy(b.host()).cuda(), torch.from_numpy(b.host("ones")).cuda()
    with _plan(b.offs, b.lens, algo) as plan:
        assert plan.info()["segment_bytes"] == S
        _whole_launch(torch, plan, ones, b, algo, "ones")
        _ranged_pass(torch, plan, data, b, algo, sized_cuts(S))
        _whole_launch(torch, plan, ones, b, algo, "ones")
        _ranged_pass(torch, plan, data, b, algo, sized_cuts(S), shifted=True)
        _whole_launch(torch, plan, ones, b, algo, "ones")
        _ranged_pass(torch, plan, data, b, algo, [1, 66 * S + 5])


@pytest.mark.parametrize("algo", ALGOS)
def test_second_grid_pass_at_16_kib(torch_cuda, batches, algo):
    """12,100 segments of 16 KiB: 3,900 and more of them are a wave's second item."""
    torch = torch_cuda
    b = batches("two_pass")
    data = torch.from_numpy(b.host()).cuda()
    with _plan(b.offs, b.lens, algo) as plan:
        info = plan.info()
        assert info["segment_bytes"] == 16384 and info["segments"] == b.segments(16384)
        assert info["segments"] > 8 * info["grid"] + 1000
        _whole_launch(torch, plan, data, b, algo)
        _whole_launch(torch, plan, torch.from_numpy(b.host("ones")).cuda(), b, algo, "ones")
        _ranged_pass(torch, plan, data, b, algo, [20000, int(b.lens.max())])


@pytest.mark.parametrize("algo", ALGOS)
def test_three_grid_passes_of_tiny_segments(torch_cuda, batches, algo):
    """20,000 parts of one short segment each at 256 KiB: a wave's tables serve three items
    (four for CRC-64), and the ranged form takes one piece per part."""
    torch = torch_cuda
    b = batches("small")
    data = torch.from_numpy(b.host()).cuda()
    with _plan(b.offs, b.lens, algo) as plan:
        info = plan.info()
        assert info["segment_bytes"] == 262144 and info["segments"] == b.segments(262144)
        assert info["segments"] > 16 * info["grid"]
        _whole_launch(torch, plan, data, b, algo)
        _whole_launch(torch, plan, torch.from_numpy(b.host("ones")).cuda(), b, algo, "ones")
        _ranged_pass(torch, plan, data, b, algo, [1500, 3000])


@pytest.mark.parametrize("algo", ALGOS)
def test_verify_at_256_kib(torch_cuda, batches, algo):
    torch = torch_cuda
    b = batches(18)
    S, big = 1 << 18, crc_shapes.SIZED_BIG_PART
    want = b.want(algo)
    expected = torch.from_numpy(_signed(want)).cuda()
    data = torch.from_numpy(b.host()).cuda()

    def verify():
        if _wide(algo):
            return s3.crc64_verify_batch_device(data, b.offs, b.lens, expected)
        return s3.crc_verify_batch_device(data, b.offs, b.lens, expected, algo)
    count, mask = verify()
    assert count == 0 and not bool(mask.any())
    assert int(b.lens[big]) == 66 * S + 5
    data[int(b.offs[big]) + 65 * S + 100] ^= 0x40  # the second-to-last of the part's 67 segments
    count, mask = verify()
    assert count == 1
    assert np.flatnonzero(mask.cpu().numpy()).tolist() == [big]


@pytest.mark.parametrize("algo", ALGOS)
def test_no_stale_partials_across_sizes(torch_cuda, batches, algo):
    """A 256 KiB plan, a 16 KiB plan and the first again, on one stream without a wait between
    them: each plan owns its partials, whatever the segment sizes."""
    torch = torch_cuda
    big, small = batches(18), batches(14)
    d_big, d_small = torch.from_numpy(big.host()).cuda(), torch.from_numpy(small.host()).cuda()
    with _plan(big.offs, big.lens, algo) as p_big, _plan(small.offs, small.lens, algo) as p_small:
        assert p_big.info()["segment_bytes"] == 1 << 18 and p_small.info()["segment_bytes"] == 1 << 14
        runs = [(p_big, d_big, big), (p_small, d_small, small), (p_big, d_big, big)]
        outs = [_out(torch, len(b.lens), algo) for _, _, b in runs]
        for (plan, data, _), out in zip(runs, outs):
            plan.launch(data, out)
        torch.cuda.synchronize()
    for (_, _, b), out in zip(runs, outs):
        _check(_words(out, algo), b.want(algo), b.offs, b.lens)
