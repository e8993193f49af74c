"""Batched SHA-1 (x-amz-checksum-sha1) of device-resident parts: whole launches, ranged
launches with the state carried in the plan, verification and streams (sha1_pc_kernel through
s3h_plan_*, s3h_verify_batch_device, s3h_stream_*).  Layouts: tests/range_shapes.py.

Expected digests: hashlib.sha1 (the 20 digest bytes in memory, 5 words per part).  Bit-exact."""
import hashlib

import numpy as np
import pytest

import s3client_amd as s3
from tests import range_shapes as rs

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5AA5A5
MARGIN = 64  # sentinel words behind the n x 5 digest words
_CACHE = {}


def _sha1(host, offs, lens):
    raw = b"".join(hashlib.sha1(host[int(o):int(o) + int(n)].tobytes()).digest() for o, n in zip(offs, lens))
    return np.frombuffer(raw, dtype=np.uint32).reshape(len(lens), 5)


def _tile(fill=None):
    """The 124-part tile (random bytes, or every byte ``fill``) and its digests, computed once."""
    if fill not in _CACHE:
        offs, lens, host = rs.tiles(1, seed=211)
        if fill is not None:
            host = np.full_like(host, fill)
        want = _sha1(host, offs, lens)
        for a in (want, offs, lens):
            a.setflags(write=False)
        _CACHE[fill] = {"offs": offs, "lens": lens, "host": host, "want": want,
                        "nb": np.array([rs.nb(L) for L in lens])}
    return _CACHE[fill]


def _ragged(seed, lens, gap=3):
    lens = np.asarray(lens, dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens + np.uint64(gap))[:-1]]).astype(np.uint64)
    host = np.random.default_rng(seed).integers(0, 256, int(offs[-1] + lens[-1]) + 64, dtype=np.uint8)
    return {"offs": offs, "lens": lens, "host": host}


def _bad(got, want, lens):
    rows = np.flatnonzero((got != want).any(axis=1))
    return [(int(i), int(lens[i])) for i in rows[:8]]


def _whole_launch(torch, batch, want=None):
    """One whole launch into n x 5 words followed by a sentinel margin: digests right, margin
    untouched.  Returns the plan's info."""
    offs, lens = batch["offs"], batch["lens"]
    n = len(lens)
    want = _sha1(batch["host"], offs, lens) if want is None else want
    data = torch.from_numpy(batch["host"]).cuda()
    out = torch.full((5 * n + MARGIN,), SENTINEL, dtype=torch.int32, device="cuda")
    with s3.Plan(offs, lens, algo="sha1") as plan:
        assert plan.words == 5
        info = plan.info()
        assert info["kernel"] == "pc" and info["grid"] == (n + 63) // 64, info
        plan.launch(data, out)
        plan.status()
    got = out.cpu().numpy().view(np.uint32)
    assert np.all(got[5 * n:] == SENTINEL), "words behind the digests were written"
    got = got[:5 * n].reshape(n, 5)
    assert np.array_equal(got, want), _bad(got, want, lens)
    return info


# ------------------------------------------------------------------ whole launches
@pytest.mark.parametrize("fill", (None, 0x00, 0xFF), ids=("random", "zeros", "ones"))
def test_tile_of_padding_boundaries(torch_cuda, fill):
    """124 parts: every length around the padding boundaries at start misalignments 0-3; two
    workgroups, the second partial."""
    b = _tile(fill)
    assert len(b["lens"]) == rs.TILE_PARTS == 124
    _whole_launch(torch_cuda, b, b["want"])


@pytest.mark.parametrize("n", (1, 64, 65))
def test_part_counts_around_one_workgroup(torch_cuda, n):
    rng = np.random.default_rng(212 + n)
    _whole_launch(torch_cuda, _ragged(213 + n, rng.integers(0, 700, n)))


def test_lone_empty_part(torch_cuda):
    info = _whole_launch(torch_cuda, {"offs": np.zeros(1, dtype=np.uint64), "lens": np.zeros(1, dtype=np.uint64),
                                      "host": np.zeros(64, dtype=np.uint8)})
    assert info["max_blocks"] == 1


def test_many_fast_steps_then_a_ragged_tail(torch_cuda):
    """70 parts of U[200, 260] KiB: thousands of fast-loop steps while every chain of a
    workgroup is live, then a tail in which the chains end on different blocks."""
    rng = np.random.default_rng(214)
    _whole_launch(torch_cuda, _ragged(215, rng.integers(200 << 10, (260 << 10) + 1, 70)))


def test_more_workgroups_than_cus(torch_cuda):
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    n = 64 * cus + 64
    rng = np.random.default_rng(216)
    info = _whole_launch(torch_cuda, _ragged(217, rng.integers(0, 301, n), gap=1))
    assert info["grid"] == cus + 1


def test_one_shot_entry_point(torch_cuda):
    b = _tile()
    data = torch_cuda.from_numpy(b["host"]).cuda()
    got = s3.sha1_batch_device(data, b["offs"], b["lens"]).cpu().numpy().view(np.uint32)
    assert got.shape == (124, 5) and np.array_equal(got, b["want"])


# ------------------------------------------------------------------ ranged launches
def _sentinels(torch, n):
    return torch.full((n, 5), SENTINEL, dtype=torch.int32, device="cuda")


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def test_ranged_schedules_write_each_digest_once(torch_cuda):
    """Every schedule of both families on one plan, blk_origin 0, the state carried in the
    plan.  After each launch exactly the parts for which range_shapes.due holds differ from the
    sentinel and equal hashlib's digest; after a pass the buffer is all sentinel again."""
    torch = torch_cuda
    b = _tile()
    lens, want, n = b["lens"], b["want"], len(b["lens"])
    data = torch.from_numpy(b["host"]).cuda()
    out = _sentinels(torch, n)
    with s3.Plan(b["offs"], lens, algo="sha1") as plan:
        for _, schedules in rs.FAMILIES.values():
            for schedule in schedules:
                for b0, b1 in schedule:
                    plan.launch_range(data.data_ptr(), out, b0, b1, 0)
                    plan.status()
                    got = _words(out)
                    changed = (got != SENTINEL).any(axis=1)
                    due = np.array([rs.due(L, b0, b1) for L in lens])
                    wrong = np.flatnonzero(changed != due)
                    assert wrong.size == 0, ((b0, b1), [(int(i), int(lens[i]), bool(due[i])) for i in wrong[:8]])
                    assert np.array_equal(got[due], want[due]), ((b0, b1), _bad(got[due], want[due], lens[due]))
                    out[torch.from_numpy(np.flatnonzero(due)).cuda()] = SENTINEL
                # the short passes end at block 4 with every long part open: those stay sentinel
                assert np.all(_words(out) == SENTINEL), schedule


def test_ranged_passes_through_a_slot_buffer(torch_cuda):
    """The host ring's form on the long family's two-range cuts: each range's bytes of part j at
    j * slot + (offset mod 4) of a buffer of its own, 0xEE behind each part's end, one plan on
    the slot offsets, blk_origin = blk_begin."""
    torch = torch_cuda
    b = _tile()
    lens, want, n = b["lens"], b["want"], len(b["lens"])
    slot = 64 * rs.LONG_BLOCKS + 64
    plan = None
    for c in rs.LONG_CUTS:
        bufs = []
        for b0, b1 in ((0, c), (c, rs.LONG_BLOCKS)):
            slot_offs, buf = rs.slot_buffer(b["host"], b["offs"], lens, b0, b1, slot)
            bufs.append((b0, b1, torch.from_numpy(buf).cuda()))
        if plan is None:
            plan = s3.Plan(slot_offs, lens, algo="sha1")
        out = _sentinels(torch, n)
        for b0, b1, dev in bufs:
            plan.launch_range(dev.data_ptr(), out, b0, b1, b0)
        plan.status()
        got = _words(out)
        assert np.array_equal(got, want), (c, _bad(got, want, lens))
    plan.close()


# ------------------------------------------------------------------ verification
def test_verify_flags_exactly_the_flipped_part(torch_cuda):
    torch = torch_cuda
    b = _tile()
    expected = torch.from_numpy(b["want"].view(np.int32).copy()).cuda()
    data = torch.from_numpy(b["host"]).cuda()
    count, mask = s3.verify_batch_device(data, b["offs"], b["lens"], expected, algo="sha1")
    assert count == 0 and not mask.any().item()
    j = int(np.flatnonzero(b["lens"] == 64 * 17 + 56)[1])
    host = b["host"].copy()
    host[int(b["offs"][j]) + 700] ^= 0x10
    data = torch.from_numpy(host).cuda()
    count, mask = s3.verify_batch_device(data, b["offs"], b["lens"], expected, algo="sha1")
    assert count == 1 and np.flatnonzero(mask.cpu().numpy()).tolist() == [j]


# ------------------------------------------------------------------ streams
CHUNKS = (0, 1, 63, 64, 65, 1000, 4096)


def _stream_rounds(seed, n, rounds):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(rounds):
        lens = rng.choice(CHUNKS, n).astype(np.uint64)
        out.append(_ragged(int(rng.integers(1 << 30)), lens, gap=1))
    return out


def _stream_want(rounds, n):
    msgs = [b"".join(r["host"][int(r["offs"][i]):int(r["offs"][i] + r["lens"][i])].tobytes() for r in rounds)
            for i in range(n)]
    return np.frombuffer(b"".join(hashlib.sha1(m).digest() for m in msgs), dtype=np.uint32).reshape(n, 5)


@pytest.mark.parametrize("form", ("device", "host"))
def test_stream_of_130_messages(torch_cuda, form):
    """130 messages fed in chunks of lengths drawn from CHUNKS; final digests equal hashlib's,
    and after ``final`` the object starts over with empty messages."""
    torch = torch_cuda
    n = 130
    with s3.Stream(n, algo="sha1") as st:
        assert st.words == 5
        for seed, nrounds in ((220, 7), (221, 3)):
            rounds = _stream_rounds(seed, n, nrounds)
            keep = []
            for r in rounds:
                if form == "device":
                    dev = torch.from_numpy(r["host"]).cuda()
                    keep.append(dev)
                    st.update_device(dev, r["offs"], r["lens"])
                else:
                    st.update(s3.BufferParts(r["host"], r["offs"], r["lens"]))
            if form == "device":
                out = torch.full((n, 5), SENTINEL, dtype=torch.int32, device="cuda")
                st.final_device(out)
                st.status()
                got = _words(out)
            else:
                got = st.final()
            want = _stream_want(rounds, n)
            assert np.array_equal(got, want), (seed, _bad(got, want, np.zeros(n)))
        # nothing appended: n empty messages
        empty = st.final()
        assert all(row.tobytes() == hashlib.sha1(b"").digest() for row in empty)
