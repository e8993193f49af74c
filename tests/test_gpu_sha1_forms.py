"""Both instantiations of the SHA-1 kernel on the device, on the layouts of tests/sha1_shapes.py:
sha1_pc_kernel<1> (plans with more workgroups than CUs: more than 64 x CUs parts) through whole,
ranged, host-pipeline, verification and stream launches; resumes into the long loops of
sha1_pc_kernel<2> at odd and even blocks and with partial last steps; ranges of 2^31 blocks or
more and ranges that launch nothing on both forms; random batch shapes; offsets past 4 GiB
(SHA-1 and MD5).

Expected digests: hashlib (sha1_shapes.sha1_ref / md5_ref / sha256_ref), the digest bytes as
stored, bit-exact."""
import hashlib

import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests import range_shapes as rs
from tests import sha1_shapes as sh
from tests.test_gpu_shapes import BUF, _draws

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5AA5A5
MARGIN = 64  # sentinel words behind the digest words of a whole launch
HUGE = 2 ** 31


class Batch:
    """Parts of one buffer, their SHA-1 digests and the buffer on the device."""

    def __init__(self, torch, offs, lens, host):
        self.offs, self.lens, self.host = offs, lens, host
        self.n = len(lens)
        self.nb = sh.nb(lens)
        self.want = sh.sha1_ref(host, offs, lens)
        for a in (self.want, self.offs, self.lens, self.nb):
            a.setflags(write=False)
        self.data = torch.from_numpy(host).cuda()
        self.grid = (self.n + 63) // 64
        self._sha256 = None

    def sha256(self):
        if self._sha256 is None:
            self._sha256 = sh.sha256_ref(self.host, self.offs, self.lens)
        return self._sha256


@pytest.fixture(scope="module")
def cus(torch_cuda):
    return torch_cuda.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def many(torch_cuda, cus):
    b = Batch(torch_cuda, *sh.many(cus, seed=301))
    assert b.grid == cus + 2 > cus
    return b


@pytest.fixture(scope="module")
def long70(torch_cuda, cus):
    b = Batch(torch_cuda, *sh.long70(seed=302))
    assert b.grid == 2 <= cus
    return b


@pytest.fixture(scope="module")
def tile(torch_cuda, cus):
    b = Batch(torch_cuda, *rs.tiles(1, seed=303))
    assert b.grid == 2 <= cus and int(b.nb.max()) == rs.LONG_BLOCKS
    return b


@pytest.fixture
def layout(request, tile, many):
    return {"tile": tile, "many": many}[request.param]


LAYOUTS = pytest.mark.parametrize("layout", ("tile", "many"), indirect=True)


def _plan(b, algo="sha1"):
    plan = s3.Plan(b.offs, b.lens, algo=algo)
    info = plan.info()
    assert info["kernel"] == "pc" and info["grid"] == b.grid, info
    assert info["max_blocks"] == int(b.nb.max()), info
    return plan, info


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _sentinels(torch, n, words=5):
    return torch.full((n, words), SENTINEL, dtype=torch.int32, device="cuda")


def _bad(got, want, lens):
    rows = np.flatnonzero((got != want).any(axis=1))
    return [(int(i), int(lens[i])) for i in rows[:8]]


def _whole_launch(torch, b, algo="sha1", want=None):
    """One whole launch into n x words words followed by a sentinel margin: digests right,
    margin untouched."""
    want = b.want if want is None else want
    plan, _ = _plan(b, algo)
    with plan:
        w = plan.words
        out = torch.full((w * b.n + MARGIN,), SENTINEL, dtype=torch.int32, device="cuda")
        plan.launch(b.data, out)
        plan.status()
    got = _words(out)
    assert np.all(got[w * b.n:] == SENTINEL), "words behind the digests were written"
    got = got[:w * b.n].reshape(b.n, w)
    assert np.array_equal(got, want), _bad(got, want, b.lens)


def _launch_checked(torch, plan, b, out, b0, b1, want=None):
    """One ranged launch at origin 0: exactly the parts whose final block lies in [b0, b1) are
    written, with the right digest; they are reset to the sentinel afterwards."""
    want = b.want if want is None else want
    plan.launch_range(b.data.data_ptr(), out, b0, b1, 0)
    plan.status()
    got = _words(out)
    changed = (got != SENTINEL).any(axis=1)
    due = sh.due(b.nb, b0, b1)
    wrong = np.flatnonzero(changed != due)
    assert wrong.size == 0, ((b0, b1), [(int(i), int(b.lens[i]), bool(due[i])) for i in wrong[:8]])
    assert np.array_equal(got[due], want[due]), ((b0, b1), _bad(got[due], want[due], b.lens[due]))
    out[torch.from_numpy(np.flatnonzero(due)).cuda()] = SENTINEL


def _pass(torch, plan, b, out, ranges):
    for b0, b1 in ranges:
        _launch_checked(torch, plan, b, out, b0, b1)
    assert np.all(_words(out) == SENTINEL), ranges


# ------------------------------------------------------------------ a. the many-part form
def test_many_whole_launch(torch_cuda, many):
    _whole_launch(torch_cuda, many)
    got = _words(s3.sha1_batch_device(many.data, many.offs, many.lens))
    assert got.shape == (many.n, 5) and np.array_equal(got, many.want), _bad(got, many.want, many.lens)


def test_many_schedule_twice_on_one_plan(torch_cuda, many):
    """MANY_SCHEDULE at blk_origin 0, the state carried in the plan: after each launch exactly
    the due parts differ from the sentinel and equal hashlib; a second pass follows an
    abandoned first range [0, 9), whose state must not be carried over.  The schedule's ranges
    from odd blocks are one block long, so a last pass cuts at 37 and 74: whole-block steps in
    pairs from an odd block, as the host pipeline's 37-block slices run them."""
    b = many
    plan, info = _plan(b)
    end = info["max_blocks"]
    ranges = sh.schedule(sh.MANY_SCHEDULE, end)
    out = _sentinels(torch_cuda, b.n)
    with plan:
        _pass(torch_cuda, plan, b, out, ranges)
        _launch_checked(torch_cuda, plan, b, out, 0, 9)
        _pass(torch_cuda, plan, b, out, ranges)
        _pass(torch_cuda, plan, b, out, [(0, 37), (37, 74), (74, end)])


@pytest.mark.parametrize("slice_blocks", (37, 101, 0))
def test_many_through_the_host_pipeline(torch_cuda, many, slice_blocks):
    """One device, so the plan keeps all 64 x CUs + 70 parts; an explicit slice keeps the slice
    pipeline (host_path.cpp run_host_shard): ranged launches with blk_origin = blk_begin, 37
    blocks each (resumes at blocks 37 and 74), or 96 and the rest (101 blocks exceed the longest
    part: the slice is cut to its 6,144 bytes); 0 selects whole parts in groups."""
    b = many
    parts = s3.BufferParts(b.host, b.offs, b.lens)
    s1 = s3.sha1_batch_host(parts, ndevices=1, slice_bytes=64 * slice_blocks)
    assert s1.shape == b.want.shape and np.array_equal(s1, b.want), _bad(s1, b.want, b.lens)
    sha, s1 = s3.sha256_sha1_batch_host(parts, ndevices=1, slice_bytes=64 * slice_blocks)
    assert np.array_equal(s1, b.want), _bad(s1, b.want, b.lens)
    want256 = b.sha256()
    assert np.array_equal(sha, want256), _bad(sha, want256, b.lens)


def test_many_verify_flags_exactly_the_flipped_part(torch_cuda, many, cus):
    torch, b = torch_cuda, many
    expected = torch.from_numpy(b.want.view(np.int32).copy()).cuda()
    count, mask = s3.verify_batch_device(b.data, b.offs, b.lens, expected, algo="sha1")
    assert count == 0 and not mask.any().item()
    # a 17-block part in a workgroup past the first `cus` (sha1_shapes.slot_order)
    late = sh.slot_order(b.lens)[64 * cus:]
    j = int(late[b.lens[late] == 1024][0])
    at = int(b.offs[j]) + 512
    b.data[at] ^= 0x10
    try:
        count, mask = s3.verify_batch_device(b.data, b.offs, b.lens, expected, algo="sha1")
    finally:
        b.data[at] ^= 0x10
    assert count == 1 and np.flatnonzero(mask.cpu().numpy()).tolist() == [j]


CHUNKS = (0, 1, 63, 64, 65, 1000, 4096)


def _stream_rounds(seed, n, rounds):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(rounds):
        lens = rng.choice(CHUNKS, n).astype(np.uint64)
        offs = np.concatenate([[0], np.cumsum(lens + np.uint64(1))[:-1]]).astype(np.uint64)
        out.append((offs, lens, rng.integers(0, 256, int(offs[-1] + lens[-1]) + 64, dtype=np.uint8)))
    return out


def _stream_want(rounds, n):
    """hashlib.sha1 of every message: its chunks of all rounds concatenated."""
    total = sum(r[1] for r in rounds)
    offs = np.concatenate([[0], np.cumsum(total)[:-1]]).astype(np.uint64)
    msgs = np.empty(int(total.sum()) + 1, dtype=np.uint8)
    at = offs.copy()
    for ro, rl, host in rounds:
        for i in np.flatnonzero(rl):
            msgs[int(at[i]):int(at[i] + rl[i])] = host[int(ro[i]):int(ro[i] + rl[i])]
        at += rl
    return sh.sha1_ref(msgs, offs, total)


@pytest.mark.parametrize("form", ("device", "host"))
def test_many_messages_in_one_stream(torch_cuda, cus, form):
    """64 x CUs + 70 messages fed in chunks of lengths drawn from CHUNKS, three rounds and a
    final, twice on one object; a final with nothing appended gives sha1(b"") in every row."""
    torch = torch_cuda
    n = 64 * cus + 70
    with s3.Stream(n, algo="sha1") as st:
        assert st.words == 5
        for seed in (310, 311):
            rounds = _stream_rounds(seed, n, 3)
            keep = []
            for offs, lens, host in rounds:
                if form == "device":
                    keep.append(torch.from_numpy(host).cuda())
                    st.update_device(keep[-1], offs, lens)
                else:
                    st.update(s3.BufferParts(host, offs, lens))
            if form == "device":
                out = _sentinels(torch, n)
                st.final_device(out)
                st.status()
                got = _words(out)
            else:
                got = st.final()
            want = _stream_want(rounds, n)
            assert np.array_equal(got, want), (seed, _bad(got, want, sum(r[1] for r in rounds)))
        empty = st.final()
        assert empty.shape == (n, 5)
        assert np.all(empty == np.frombuffer(hashlib.sha1(b"").digest(), dtype=np.uint32))


# ------------------------------------------------------------------ b. resumed long loops
def test_long_schedule_resumes_into_the_fast_loops(torch_cuda, long70):
    """70 parts of 641-769 blocks on sha1_pc_kernel<2>: ranges that start at odd blocks, have odd
    lengths (a partial last step) and resume into hundreds of steps with every chain live."""
    b = long70
    plan, info = _plan(b)
    out = _sentinels(torch_cuda, b.n)
    with plan:
        _pass(torch_cuda, plan, b, out, sh.schedule(sh.LONG_SCHEDULE, info["max_blocks"]))


def test_long_parts_in_launches_of_37_blocks(torch_cuda, long70):
    """Starts alternate between even and odd blocks; every launch ends on half a step."""
    b = long70
    plan, info = _plan(b)
    out = _sentinels(torch_cuda, b.n)
    with plan:
        _pass(torch_cuda, plan, b, out, [(b0, b0 + 37) for b0 in range(0, info["max_blocks"], 37)])


# ------------------------------------------------------------------ c. range edges
@LAYOUTS
def test_ranges_of_2_31_blocks_or_more(torch_cuda, layout):
    torch, b = torch_cuda, layout
    plan, _ = _plan(b)
    with plan:
        out = _sentinels(torch, b.n)
        plan.launch_range(b.data.data_ptr(), out, 0, HUGE + 5, 0)
        plan.status()
        got = _words(out)
        assert np.array_equal(got, b.want), _bad(got, b.want, b.lens)
        for c in (1, 8, 9):
            out = _sentinels(torch, b.n)
            plan.launch_range(b.data.data_ptr(), out, 0, c, 0)
            plan.launch_range(b.data.data_ptr(), out, c, c + HUGE, 0)
            plan.status()
            got = _words(out)
            assert np.array_equal(got, b.want), (c, _bad(got, b.want, b.lens))


@LAYOUTS
def test_blk_end_far_beyond_max_blocks(torch_cuda, layout):
    """blk_end far past the longest part but below 2^31 behaves as max_blocks does, for a whole
    pass and for a pass's last range."""
    torch, b = torch_cuda, layout
    plan, _ = _plan(b)
    out = _sentinels(torch, b.n)
    with plan:
        plan.launch_range(b.data.data_ptr(), out, 0, HUGE - 1, 0)
        plan.status()
        got = _words(out)
        assert np.array_equal(got, b.want), _bad(got, b.want, b.lens)
        out = _sentinels(torch, b.n)
        _launch_checked(torch, plan, b, out, 0, 9)
        plan.launch_range(b.data.data_ptr(), out, 9, HUGE - 1, 0)
        plan.status()
        got = _words(out)
        late = b.nb > 9
        assert np.array_equal(got[late], b.want[late]) and np.all(got[~late] == SENTINEL)


@LAYOUTS
def test_ranges_that_launch_nothing(torch_cuda, layout):
    """blk_end <= blk_begin returns OK, blk_origin > blk_begin S3H_EINVAL; neither launches
    anything: sentinels and the chaining state stay, and the pass continues to the right
    digests."""
    torch, b = torch_cuda, layout
    plan, info = _plan(b)
    end = info["max_blocks"]
    out = _sentinels(torch, b.n)
    with plan:
        _launch_checked(torch, plan, b, out, 0, 9)
        for b0, b1 in ((9, 9), (9, 3), (20, 20), (0, 0)):
            plan.launch_range(b.data.data_ptr(), out, b0, b1, 0)
        for b0, b1, origin in ((9, end, 10), (0, end, 1), (9, 9, 10)):
            with pytest.raises(s3.S3HashError) as e:
                plan.launch_range(b.data.data_ptr(), out, b0, b1, origin)
            assert e.value.code == _native.S3H_EINVAL
        plan.status()
        assert np.all(_words(out) == SENTINEL)
        _launch_checked(torch, plan, b, out, 9, end)
        assert np.all(_words(out) == SENTINEL)


# ------------------------------------------------------------------ d. random shapes
@pytest.fixture(scope="module")
def device_bytes(torch_cuda):
    host = np.random.default_rng(778).integers(0, 256, BUF, dtype=np.uint8)
    return host, torch_cuda.from_numpy(host).cuda()


@pytest.fixture(scope="module")
def draws():
    return _draws(6, 8)  # one draw per part-count range, every length shape


@pytest.mark.parametrize("i", range(8))
def test_random_shapes(torch_cuda, device_bytes, draws, i):
    """Part counts across every AUTO range with one giant part among tiny ones, two sizes, a
    heavy tail, runs of empty parts and block-edge lengths: the sort, the out_idx scatter and
    the 20-byte digest stride."""
    host, dev = device_bytes
    n, shape, offs, lens = draws[i]
    got = _words(s3.sha1_batch_device(dev, offs, lens))
    want = sh.sha1_ref(host, offs, lens)
    rows = np.flatnonzero((got != want).any(axis=1))
    assert rows.size == 0, (n, shape, rows[:8], lens[rows[:8]])


# ------------------------------------------------------------------ e. offsets past 4 GiB
@pytest.mark.parametrize("algo", ("sha1", "md5"))
def test_offsets_past_4_gib(torch_cuda, algo):
    """Parts that straddle and lie beyond byte 2^32 of the buffer (sha1_pc_body and md5_pc_body
    form base + offset + 64 x block themselves); only the bytes the parts cover are
    initialised.  A whole launch, and one pass cut at block 37."""
    torch = torch_cuda
    top = 1 << 32
    data = torch.empty(top + (1 << 20), dtype=torch.uint8, device="cuda")
    offs = np.array([top - 100_003, top + 7, top + 300_001], dtype=np.uint64)
    lens = np.array([200_005, 250_000, 70_001], dtype=np.uint64)
    lo, hi = int(offs[0]), int(offs[-1] + lens[-1])
    host = np.random.default_rng(320).integers(0, 256, hi - lo, dtype=np.uint8)
    data[lo:hi] = torch.from_numpy(host).cuda()
    ref = sh.sha1_ref if algo == "sha1" else sh.md5_ref
    want = ref(host, offs - np.uint64(lo), lens)
    with s3.Plan(offs, lens, algo=algo) as plan:
        info = plan.info()
        assert info["kernel"] == "pc" and info["grid"] == 1, info
        w = plan.words
        out = torch.full((3 * w + MARGIN,), SENTINEL, dtype=torch.int32, device="cuda")
        plan.launch(data, out)
        plan.status()
        got = _words(out)
        assert np.all(got[3 * w:] == SENTINEL), "words behind the digests were written"
        assert np.array_equal(got[:3 * w].reshape(3, w), want), _bad(got[:3 * w].reshape(3, w), want, lens)
        out = _sentinels(torch, 3, w)
        plan.launch_range(data.data_ptr(), out, 0, 37, 0)
        plan.status()
        assert np.all(_words(out) == SENTINEL)  # every part is open at block 37
        plan.launch_range(data.data_ptr(), out, 37, info["max_blocks"], 0)
        plan.status()
        got = _words(out)
        assert np.array_equal(got, want), _bad(got, want, lens)
    del data
    torch.cuda.empty_cache()
