"""The layouts and schedules of tests/sha1_shapes.py keep what they exist for: which kernel form
a batch selects, how long the loops with every chain live run, where the ranges start and end.
No GPU: tests/test_gpu_sha1_forms.py runs them on one."""
import hashlib

import numpy as np
import pytest

import s3client_amd as s3
from tests import range_shapes as rs
from tests import sha1_shapes as sh

CUS = (120, 256, 304)


def _workgroups(lens):
    """Block counts of the plan's workgroups: slots in descending order, 64 per workgroup."""
    nblocks = sh.nb(lens)[sh.slot_order(lens)]
    assert np.all(np.diff(nblocks.astype(np.int64)) <= 0)
    return [nblocks[i:i + 64] for i in range(0, len(nblocks), 64)]


@pytest.mark.parametrize("cus", CUS)
def test_many_selects_the_many_part_form(cus):
    offs, lens, host = sh.many(cus, seed=cus)
    n = len(lens)
    assert n == 64 * cus + 70 > 64 * cus
    assert host.size >= int(offs[-1] + lens[-1]) + 64
    assert np.all(offs[1:] >= offs[:-1] + lens[:-1])  # no part overlaps the next
    groups = _workgroups(lens)
    assert len(groups) == cus + 2
    # fast loops of >= 65 steps: 64 x cus - 58 long parts fill cus - 1 whole workgroups
    assert sum(int(g.min()) >= 65 for g in groups) >= cus - 1
    assert all(int(g.min()) >= 65 for g in groups[:cus - 1])
    assert int(sh.nb(lens).max()) <= 97
    # one workgroup mixes long and short parts: fast steps, then a long ragged tail
    mixed = [g for g in groups if int(g.max()) >= 65 and int(g.min()) <= rs.LONG_BLOCKS]
    assert len(mixed) >= 1
    assert len(groups[-1]) == 6  # the last workgroup is partial
    assert set((offs % np.uint64(4)).tolist()) == {0, 1, 2, 3}
    assert len(set((offs % np.uint64(64)).tolist())) >= 32
    assert (lens == 0).any()
    # every padding-edge length of the tile occurs
    assert set(rs.SHORT_LENGTHS + rs.LONG_LENGTHS) <= set(lens.tolist())
    # the part whose flip the verification test looks for: a 1,024-byte part (17 blocks) in a
    # workgroup past the first `cus`
    order = sh.slot_order(lens)
    assert (lens[order[64 * cus:]] == 1024).any()


def test_long70_keeps_every_chain_live_for_641_blocks():
    offs, lens, host = sh.long70()
    assert len(lens) == 70 and np.all(np.diff(offs.astype(np.int64)) == lens[:-1].astype(np.int64) + 3)
    groups = _workgroups(lens)
    assert len(groups) == 2 and len(groups[0]) == 64 and len(groups[1]) == 6
    assert int(groups[0].min()) >= 641 and int(sh.nb(lens).min()) >= 641
    assert int(sh.nb(lens).max()) <= 769
    # every part is open across the schedule's first six cuts
    cuts = [b1 for _, b1 in sh.LONG_SCHEDULE[:-1]]
    assert len(cuts) >= 5 and all(c < int(sh.nb(lens).min()) for c in cuts)


@pytest.mark.parametrize("name,max_blocks", [("MANY_SCHEDULE", 97), ("LONG_SCHEDULE", 769)])
def test_schedules(name, max_blocks):
    sched = sh.schedule(getattr(sh, name), max_blocks)
    assert sched[0][0] == 0 and sched[-1][1] == max_blocks
    assert all(a[1] == b[0] for a, b in zip(sched, sched[1:]))  # contiguous
    assert all(b1 > b0 for b0, b1 in sched)
    assert sum(b0 % 2 == 1 for b0, _ in sched) >= 2          # starts at odd blocks
    assert sum(b0 % 2 == 0 for b0, _ in sched[1:]) >= 2      # resumes at even blocks
    assert sum((b1 - b0) % 2 == 1 for b0, b1 in sched) >= 2  # a partial 2-block last step
    assert any(b0 % 2 == 1 and (b1 - b0) % 2 == 1 for b0, b1 in sched)
    assert any((b1 - b0) % 2 == 1 and b1 - b0 > 2 for b0, b1 in sched)  # whole steps, then half a one
    # a resume into tens of steps with every chain live (the parts' shortest: 65 / 641 blocks)
    live = 65 if name == "MANY_SCHEDULE" else 641
    assert any(b0 > 0 and min(b1, live) - b0 >= 24 for b0, b1 in sched)


def test_vectorised_due_and_nb_agree_with_range_shapes():
    _, lens, _ = rs.tiles(1)
    lens = np.concatenate([lens, [4096, 6135, 6136, 6144, 40 << 10, 48 << 10]])
    assert sh.nb(lens).tolist() == [rs.nb(L) for L in lens]
    for sched in (sh.schedule(sh.MANY_SCHEDULE, 97), sh.schedule(sh.LONG_SCHEDULE, 769),
                  rs.LONG_SINGLE_BLOCKS, [(9, 9), (9, 3), (0, 0), (0, 2 ** 31 + 5), (9, 9 + 2 ** 31)]):
        for b0, b1 in sched:
            assert sh.due(sh.nb(lens), b0, b1).tolist() == [rs.due(L, b0, b1) for L in lens], (b0, b1)


def test_references_and_the_cpu_sha1_on_sampled_parts():
    """sha1_shapes.sha1_ref is hashlib.sha1 part by part, and the library's CPU SHA-1 (s3.sha1
    = s3h_cpu_sha1) agrees with it on 200 parts of many(256)."""
    offs, lens, host = sh.many(256, seed=5)
    pick = np.random.default_rng(6).choice(len(lens), 200, replace=False)
    pick[:3] = [np.flatnonzero(lens == L)[0] for L in (0, 55, 56)]
    want = sh.sha1_ref(host, offs[pick], lens[pick])
    assert want.shape == (200, 5)
    for row, j in zip(want, pick):
        part = host[int(offs[j]):int(offs[j] + lens[j])].tobytes()
        assert row.tobytes() == hashlib.sha1(part).digest(), int(j)
        assert s3.sha1(part).tobytes() == row.tobytes(), (int(j), int(lens[j]))
    assert sh.md5_ref(host, offs[pick[:5]], lens[pick[:5]]).tobytes() == b"".join(
        hashlib.md5(host[int(offs[j]):int(offs[j] + lens[j])].tobytes()).digest() for j in pick[:5])
    assert sh.sha256_ref(host, offs[pick[:5]], lens[pick[:5]]).tobytes() == b"".join(
        hashlib.sha256(host[int(offs[j]):int(offs[j] + lens[j])].tobytes()).digest() for j in pick[:5])
