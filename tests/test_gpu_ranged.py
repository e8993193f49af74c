"""Ranged (resumable) launches of the hash plans (s3h_plan_launch_range) on every kernel: cuts
around each part's final block, which launch writes which digest, the host ring's slot-buffer
form (blk_origin = blk_begin), the dual grids through one-block slices, and ranges of 2^31
blocks or more (launch.hip's 64-bit-counter fallbacks).  Layouts: tests/range_shapes.py.

Expected digests: the oracle (tests/oracle_lib.py, pinned to the lib/hash goldens by
tests/test_oracle.py); SHA-256 also against hashlib.  Bit-exact."""
import hashlib

import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests import range_shapes as rs

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5AA5A5
SHA_KERNELS = ["lane", "pc", "pair", "quad", "skew", "skewp", "skews"]
# (id, kernel, algo, tiles): every SHA-256 kernel forced at one tile, the two-group skew kernel
# (sha256_skew_pairs_kernel: 2,049-4,096 parts) at 17 tiles, MD5 at one tile
CASES = [pytest.param(k, "sha256", 1, id=k) for k in SHA_KERNELS] + [
    pytest.param("skew", "sha256", 17, id="skew-pairs"), pytest.param("auto", "md5", 1, id="md5")]
_BATCHES = {}


def _batch(oracle, count):
    """``count`` tiles and both digests of every part, computed once per module run."""
    if count not in _BATCHES:
        offs, lens, host = rs.tiles(count, seed=100 + count)
        sha = oracle.batch(host, offs, lens, threads=16)
        for j in range(0, len(lens), 7 if count > 1 else 1):  # the oracle against hashlib
            b = host[int(offs[j]):int(offs[j] + lens[j])].tobytes()
            assert sha[j].tobytes() == hashlib.sha256(b).digest(), j
        md5 = oracle.md5_batch(host, offs, lens, threads=16)
        for a in (sha, md5, offs, lens):  # (torch.from_numpy wants the bytes writable)
            a.setflags(write=False)
        _BATCHES[count] = {"offs": offs, "lens": lens, "host": host, "sha256": sha, "md5": md5,
                           "nb": np.array([rs.nb(L) for L in lens])}
    return _BATCHES[count]


def _plan(batch, kernel, algo, offs=None):
    plan = s3.Plan(batch["offs"] if offs is None else offs, batch["lens"], kernel=kernel, algo=algo)
    info = plan.info()
    if algo == "sha256":
        assert info["kernel"] == kernel, info
    return plan, info


def _assert_two_group_skew(info, n):
    """2,049-4,096 parts: sha256_skew_pairs_kernel, two 8-part groups per workgroup except the
    plan's solo ones (plan.cpp plan_geometry).  17 tiles get solo workgroups on 256 CUs (43:
    the groups of the 34- and 35-block parts, plan_solo), so grid == ceil(groups / 2) holds
    only for batches without them."""
    groups = (n + 7) // 8
    assert info["groups"] == groups > 256, info
    assert info["grid"] == info["solo"] + (groups - info["solo"] + 1) // 2, info


def _sentinels(torch, n, words):
    return torch.full((n, words), SENTINEL, dtype=torch.int32, device="cuda")


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _bad(got, want, lens):
    rows = np.flatnonzero((got != want).any(axis=1))
    return [(int(i), int(lens[i])) for i in rows[:8]]


def _launch_checked(torch, plan, data, out, b0, b1, batch, want):
    """One ranged launch at origin 0: exactly the parts whose final block lies in [b0, b1) are
    written, with the right digest; they are reset to the sentinel afterwards."""
    plan.launch_range(data.data_ptr(), out, b0, b1, 0)
    plan.status()
    got = _words(out)
    changed = (got != SENTINEL).any(axis=1)
    due = (batch["nb"] > b0) & (batch["nb"] <= b1)
    wrong = np.flatnonzero(changed != due)
    assert wrong.size == 0, ((b0, b1), [(int(i), int(batch["lens"][i]), bool(due[i])) for i in wrong[:8]])
    assert np.array_equal(got[due], want[due]), ((b0, b1), _bad(got[due], want[due], batch["lens"][due]))
    out[torch.from_numpy(np.flatnonzero(due)).cuda()] = SENTINEL


@pytest.mark.parametrize("kernel,algo,count", CASES)
def test_cut_tail_matrix_writes_each_digest_once(torch_cuda, oracle, kernel, algo, count):
    """Every schedule of both families on one plan, blk_origin 0.  After each launch exactly
    the parts with b0 < nb(L) <= b1 differ from the sentinel and equal the oracle; after a
    pass the buffer is all sentinel again (no later launch rewrote a digest).  Each pass from
    block 0 follows a finished or an unfinished one on the same plan: the short passes end at
    block 4 with every long part open, and one pass is abandoned after its first range [0, 9)."""
    torch = torch_cuda
    batch = _batch(oracle, count)
    want, n = batch[algo], len(batch["lens"])
    data = torch.from_numpy(batch["host"]).cuda()
    plan, info = _plan(batch, kernel, algo)
    if count > 1:
        _assert_two_group_skew(info, n)
    out = _sentinels(torch, n, plan.words)
    with plan:
        for schedule in rs.SHORT_SCHEDULES + [[(0, 9)]] + rs.LONG_SCHEDULES:
            for b0, b1 in schedule:
                _launch_checked(torch, plan, data, out, b0, b1, batch, want)
            assert np.all(_words(out) == SENTINEL), schedule


@pytest.mark.parametrize("kernel,algo,count", CASES)
def test_two_range_passes_through_a_slot_buffer(torch_cuda, oracle, kernel, algo, count):
    """The host ring's form: each range's bytes of part j at j * slot + (offset mod 4) of a
    buffer of its own, everything else 0xEE (behind a part's end, the slot of a part with only
    its padding-only block in the range, the slack), one plan on the slot offsets, blk_origin =
    blk_begin.  Long-family two-range cuts; digests after each pass equal the oracle's."""
    torch = torch_cuda
    batch = _batch(oracle, count)
    want, n = batch[algo], len(batch["lens"])
    slot = 64 * rs.LONG_BLOCKS + 64
    slot_offs = None
    for c in rs.LONG_CUTS:
        bufs = []
        for b0, b1 in ((0, c), (c, rs.LONG_BLOCKS)):
            slot_offs, buf = rs.slot_buffer(batch["host"], batch["offs"], batch["lens"], b0, b1, slot)
            bufs.append((b0, b1, torch.from_numpy(buf).cuda()))
        if c == rs.LONG_CUTS[0]:
            plan, info = _plan(batch, kernel, algo, offs=slot_offs)
            if count > 1:
                _assert_two_group_skew(info, n)
        out = _sentinels(torch, n, plan.words)
        for b0, b1, dev in bufs:
            plan.launch_range(dev.data_ptr(), out, b0, b1, b0)
        plan.status()
        got = _words(out)
        assert np.array_equal(got, want), (c, _bad(got, want, batch["lens"]))
    plan.close()


@pytest.mark.parametrize("count", (1, 15, 17, 66))
def test_dual_digests_through_one_block_slices(torch_cuda, oracle, count):
    """sha256_md5_batch_host with 64-byte slices on one device: every ranged launch of the dual
    grid is one block, so each cut of the matrix above falls in every part.  The form each count
    selects on 256 CUs (plan.cpp dual_mode; the host plan has the tile's lengths):
      124 parts    split grid (16 skew workgroups + their MD5 workgroups fit one per CU);
      1,860 parts  skew groups each with a self-fed MD5 wave (233 workgroups: the split grid
                   would need more than 256);
      2,108 parts  the mixed grid (dual_mixed_solo > 0: the 34/35-block parts in skew groups,
                   the rest in skewp groups);
      8,184 parts  the group kernel (256 workgroups of 32 parts; a mixed grid would not fit)."""
    torch = torch_cuda
    batch = _batch(oracle, count)
    offs, lens, n = batch["offs"], batch["lens"], len(batch["lens"])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = (n + 7) // 8
    solo, _ = s3.dual_layout(lens, cus)
    if count == 1:
        assert groups + 8 * ((groups + 63) // 64) <= cus
    elif count == 15:
        assert n <= 2048 and groups <= cus < groups + (n + 63) // 64
    elif count == 17:
        assert n > 2048 and solo > 0
    else:
        assert (n + 31) // 32 <= cus and solo == 0
    parts = [batch["host"][int(o):int(o + L)] for o, L in zip(offs, lens)]
    sha, m5 = s3.sha256_md5_batch_host(parts, ndevices=1, slice_bytes=64)
    assert np.array_equal(sha, batch["sha256"]), _bad(sha, batch["sha256"], lens)
    assert np.array_equal(m5, batch["md5"]), _bad(m5, batch["md5"], lens)


# ------------------------------------------------------------------ ranges of 2^31 blocks or more
def _ragged_top(seed, n, top, top_len, rest_len):
    rng = np.random.default_rng(seed)
    lens = rng.integers(*rest_len, n)
    lens[:top] = rng.integers(*top_len, top)
    rng.shuffle(lens)
    offs = np.concatenate([[0], np.cumsum(lens + 3)[:-1]]).astype(np.uint64)  # misaligned
    host = rng.integers(0, 256, int(offs[-1] + lens[-1]) + 64, dtype=np.uint8)
    return {"offs": offs, "lens": lens.astype(np.uint64), "host": host}


def _equal_parts(seed, n, length):
    offs = np.arange(n, dtype=np.uint64) * np.uint64(length + 3)
    host = np.random.default_rng(seed).integers(0, 256, n * (length + 3) + 64, dtype=np.uint8)
    return {"offs": offs, "lens": np.full(n, length, dtype=np.uint64), "host": host}


HUGE = 2 ** 31
HUGE_CASES = [pytest.param("skew", "sha256", "tile1", id="skew-one-group"),
              pytest.param("skew", "sha256", "tile17", id="skew-pairs-tile"),
              pytest.param("skew", "sha256", "equal", id="skew-pairs-no-solo"),
              pytest.param("skew", "sha256", "solo", id="skew-pairs-solo"),
              pytest.param("skews", "sha256", "tile1", id="skews"),
              pytest.param("skewp", "sha256", "tile1", id="skewp"),
              pytest.param("quad", "sha256", "tile1", id="quad"),
              pytest.param("pair", "sha256", "tile1", id="pair"),
              pytest.param("pc", "sha256", "tile1", id="pc"),
              pytest.param("lane", "sha256", "tile1", id="lane"),
              pytest.param("auto", "md5", "tile1", id="md5")]


@pytest.mark.parametrize("kernel,algo,shape", HUGE_CASES)
def test_ranges_of_2_31_blocks_or_more(torch_cuda, oracle, kernel, algo, shape):
    """A range of >= 2^31 blocks sends skew / skews / skewp plans to the quad / pair kernels
    (launch.hip launch_plan_kernel); every kernel clamps its loop to the parts' blocks, so
    small parts run a few.  (i) one launch [0, 2^31 + 5); (ii) the hand-over: [0, c) on the
    plan's own kernel, then [c, c + 2^31) on the fallback, which resumes from the state the
    plan's kernel stored, c in {1, 8, 9}.
    skew-pairs-solo (2,600 parts, 40 of them ~110 KB: test_two_group_solo_grid's shape) is the
    plan whose grid, solo + ceil((groups - solo) / 2), exceeds the ceil(n / 16) workgroups that
    sha256_quad_kernel<2>'s slot mapping covers: the fallback must launch the latter.  The
    17-tile batch gets solo workgroups as well (its 34/35-block parts); skew-pairs-no-solo is
    2,108 equal parts, where the two grids agree."""
    torch = torch_cuda
    if shape == "solo":
        batch = _ragged_top(505, 2600, 40, (110_000, 112_000), (1, 5_000))
    elif shape == "equal":
        batch = _equal_parts(506, 2108, 64 * 17 + 56)
    else:
        batch = _batch(oracle, int(shape[4:]))
    offs, lens, n = batch["offs"], batch["lens"], len(batch["lens"])
    if algo in batch:
        want = batch[algo]
    else:
        want = oracle.batch(batch["host"], offs, lens, threads=16)
    data = torch.from_numpy(batch["host"]).cuda()
    plan, info = _plan(batch, kernel, algo)
    with plan:
        if shape in ("tile17", "equal", "solo"):
            _assert_two_group_skew(info, n)
        if shape == "solo":
            assert info["solo"] > 0 and info["grid"] > (n + 15) // 16, info
        if shape == "equal":
            assert info["solo"] == 0 and info["grid"] == (n + 15) // 16, info
        out = _sentinels(torch, n, plan.words)
        plan.launch_range(data.data_ptr(), out, 0, HUGE + 5, 0)
        plan.status()
        got = _words(out)
        assert np.array_equal(got, want), _bad(got, want, lens)
        for c in (1, 8, 9):
            out = _sentinels(torch, n, plan.words)
            plan.launch_range(data.data_ptr(), out, 0, c, 0)
            plan.launch_range(data.data_ptr(), out, c, c + HUGE, 0)
            plan.status()
            got = _words(out)
            assert np.array_equal(got, want), (c, _bad(got, want, lens))


# ------------------------------------------------------------------ small things
@pytest.mark.parametrize("kernel,algo", [(k, "sha256") for k in SHA_KERNELS] + [("auto", "md5")])
def test_ranges_that_launch_nothing(torch_cuda, oracle, kernel, algo):
    """blk_end <= blk_begin returns OK, blk_origin > blk_begin S3H_EINVAL; neither launches
    anything: sentinels and the chaining state stay, and the pass continues to the right
    digests."""
    torch = torch_cuda
    batch = _batch(oracle, 1)
    want, n = batch[algo], len(batch["lens"])
    data = torch.from_numpy(batch["host"]).cuda()
    plan, _ = _plan(batch, kernel, algo)
    out = _sentinels(torch, n, plan.words)
    with plan:
        _launch_checked(torch, plan, data, out, 0, 9, batch, want)
        for b0, b1 in ((9, 9), (9, 3), (20, 20), (0, 0)):
            plan.launch_range(data.data_ptr(), out, b0, b1, 0)
        for b0, b1, origin in ((9, 35, 10), (0, 35, 1), (9, 9, 10)):
            with pytest.raises(s3.S3HashError) as e:
                plan.launch_range(data.data_ptr(), out, b0, b1, origin)
            assert e.value.code == _native.S3H_EINVAL
        plan.status()
        assert np.all(_words(out) == SENTINEL)
        _launch_checked(torch, plan, data, out, 9, 35, batch, want)
        assert np.all(_words(out) == SENTINEL)


@pytest.mark.parametrize("kernel,algo", [(k, "sha256") for k in SHA_KERNELS] + [("auto", "md5")])
def test_blk_end_far_beyond_max_blocks(torch_cuda, oracle, kernel, algo):
    """blk_end far past the longest part but below 2^31 (the plan's own kernel) behaves as
    max_blocks does, for a whole pass and for a pass's last range."""
    torch = torch_cuda
    batch = _batch(oracle, 1)
    want, n = batch[algo], len(batch["lens"])
    data = torch.from_numpy(batch["host"]).cuda()
    plan, info = _plan(batch, kernel, algo)
    assert info["max_blocks"] == rs.LONG_BLOCKS
    out = _sentinels(torch, n, plan.words)
    with plan:
        plan.launch_range(data.data_ptr(), out, 0, HUGE - 1, 0)
        plan.status()
        got = _words(out)
        assert np.array_equal(got, want), _bad(got, want, batch["lens"])
        out = _sentinels(torch, n, plan.words)
        _launch_checked(torch, plan, data, out, 0, 9, batch, want)
        plan.launch_range(data.data_ptr(), out, 9, HUGE - 1, 0)
        plan.status()
        got = _words(out)
        late = batch["nb"] > 9
        assert np.array_equal(got[late], want[late]) and np.all(got[~late] == SENTINEL)
