"""The ranged-launch matrix of tests/range_shapes.py keeps the cases it exists for: for every
length, a launch of the final block alone, a cut directly in front of it, and (long family) a
cut one block earlier -- between the last data block and the tail of a part whose padding has a
block of its own, in front of the tail block of one whose has not."""
import numpy as np
import pytest

from tests import range_shapes as rs


def _cuts(schedule):
    """Block indices where one launch of the pass ends and the next begins."""
    return {a1 for (_, a1), (b0, _) in zip(schedule, schedule[1:]) if a1 == b0}


def test_block_counts_and_due_predicate():
    assert [rs.nb(L) for L in (0, 55, 56, 63, 64, 119, 120, 183, 184, 192)] == [1, 1, 2, 2, 2, 2, 3, 3, 4, 4]
    assert {rs.nb(L) for L in rs.SHORT_LENGTHS} == {1, 2, 3, 4}
    assert {rs.nb(L) for L in rs.LONG_LENGTHS} == {17, 18, 19, 34, 35}
    assert max(rs.nb(L) for L in rs.SHORT_LENGTHS) == rs.SHORT_BLOCKS
    assert max(rs.nb(L) for L in rs.LONG_LENGTHS) == rs.LONG_BLOCKS
    # b0 < nb(L) <= b1, by hand: L = 55 -> 1 block, 56 -> 2, 119 -> 2, 120 -> 3
    assert rs.due(55, 0, 1) and not rs.due(55, 1, 2)
    assert not rs.due(56, 0, 1) and rs.due(56, 1, 2) and rs.due(56, 0, 2) and not rs.due(56, 2, 3)
    assert not rs.due(119, 0, 1) and rs.due(119, 1, 2) and not rs.due(119, 2, 4)
    assert not rs.due(120, 1, 2) and rs.due(120, 2, 3) and rs.due(120, 0, 4) and not rs.due(120, 3, 4)
    assert rs.due(0, 0, 1) and not rs.due(0, 1, 4)


def test_schedules_are_contiguous_passes_from_block_zero():
    assert len(rs.SHORT_SCHEDULES) == 8 and sum(map(len, rs.SHORT_SCHEDULES)) == 20
    assert len({tuple(s) for s in rs.SHORT_SCHEDULES}) == 8
    assert len(rs.LONG_SCHEDULES) == 13 and sum(map(len, rs.LONG_SCHEDULES)) == 24 + 35
    for blocks, schedules in ((rs.SHORT_BLOCKS, rs.SHORT_SCHEDULES), (rs.LONG_BLOCKS, rs.LONG_SCHEDULES)):
        for s in schedules:
            assert s[0][0] == 0 and s[-1][1] == blocks
            assert all(b0 < b1 for b0, b1 in s)
            assert all(a[1] == b[0] for a, b in zip(s, s[1:]))


@pytest.mark.parametrize("family", ("short", "long"))
def test_every_length_meets_its_cuts(family):
    lengths, schedules = rs.FAMILIES[family]
    launches = {r for s in schedules for r in s}
    cuts = set().union(*(_cuts(s) for s in schedules))
    for L in lengths:
        n = rs.nb(L)
        assert (n - 1, n) in launches, L           # the final block alone
        if n > 1:
            assert n - 1 in cuts, L                # a cut directly in front of the final block
        if family == "long":
            assert n - 2 in cuts, L                # and one block earlier
        # every pass writes the digest exactly once
        for s in schedules:
            assert sum(rs.due(L, b0, b1) for b0, b1 in s) == 1, (L, s)
    # both kinds of tail: padding in a block of its own, and beside the last data bytes
    assert {L % 64 >= 56 for L in lengths} == {True, False}


def test_tile_layout():
    offs, lens, host = rs.tiles(2, seed=5)
    assert len(lens) == 2 * rs.TILE_PARTS == 248 and rs.TILE_PARTS == 124
    assert sorted(lens[:124].tolist()) == sorted((rs.SHORT_LENGTHS + rs.LONG_LENGTHS) * 4)
    for L in rs.SHORT_LENGTHS + rs.LONG_LENGTHS:  # each length once at each misalignment
        assert sorted((offs[:124][lens[:124] == L] % 64).tolist()) == [0, 1, 2, 3]
    ends = offs + lens
    assert np.all(ends[:-1] <= offs[1:]) and int(ends[-1]) + 64 == host.size
    a, b = host[int(offs[0]):int(ends[123])], host[int(offs[124]):int(ends[247])]
    assert not np.array_equal(a[:4096], b[:4096])  # fresh bytes per tile


def test_slot_buffer_holds_the_range_and_poison_elsewhere():
    offs, lens, host = rs.tiles(1, seed=6)
    slot = 64 * rs.LONG_BLOCKS + 64
    for b0, b1 in ((0, 17), (17, 35), (34, 35)):
        slot_offs, buf = rs.slot_buffer(host, offs, lens, b0, b1, slot)
        assert buf.size == len(lens) * slot + 256
        mask = np.ones(buf.size, dtype=bool)
        for j, (o, L) in enumerate(zip(offs.tolist(), lens.tolist())):
            assert slot_offs[j] == j * slot + o % 4
            cnt = max(0, min(64 * b1, L) - 64 * b0)
            at = int(slot_offs[j])
            assert np.array_equal(buf[at:at + cnt], host[o + 64 * b0:o + 64 * b0 + cnt])
            mask[at:at + cnt] = False
            if rs.nb(L) > b0 and L <= 64 * b0:  # only its padding-only block in the range
                assert cnt == 0
        assert np.all(buf[mask] == 0xEE)
