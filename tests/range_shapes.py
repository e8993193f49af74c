"""Part layouts and launch schedules shared by the ranged-launch tests of the hash plans
(s3h_plan_launch_range): tests/test_range_shapes_cpu.py checks that the schedules keep the
cuts they exist for, tests/test_gpu_ranged.py runs them on the GPU.

A schedule is a list of block ranges [b0, b1) launched in order on one plan.  The cuts that
matter for a resumable kernel fall around a part's final block: between its last data block and
a padding-only block (len % 64 >= 56), directly in front of the block that holds the tail, and
a launch of that one block alone."""
from itertools import combinations

import numpy as np


def nb(length: int) -> int:
    """64-byte blocks of a padded message of ``length`` bytes (kernel_abi.hpp nblocks)."""
    return (int(length) + 72) >> 6


def due(length: int, b0: int, b1: int) -> bool:
    """A part's digest is written by the launch [b0, b1) that processes its final block."""
    return b0 < nb(length) <= b1


# Short family: nb = 1..4, every way to cut [0, 4) into contiguous ranges (8 passes, 20 launches).
SHORT_LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 183, 184, 191, 192]
SHORT_BLOCKS = 4
SHORT_SCHEDULES = [list(zip((0,) + cuts, cuts + (SHORT_BLOCKS,)))
                   for k in range(SHORT_BLOCKS) for cuts in combinations(range(1, SHORT_BLOCKS), k)]

# Long family: nb in {17, 18, 19, 34, 35}: the skew kernels' unrolled fast steps run before the
# checked tail.  Two-range passes cut at LONG_CUTS, and one pass of single-block launches.
LONG_LENGTHS = [64 * k + r for k in (16, 17, 33) for r in (0, 1, 55, 56, 63)]
LONG_BLOCKS = 35
LONG_CUTS = [1, 7, 8, 9, 15, 16, 17, 18, 31, 32, 33, 34]
LONG_TWO_RANGE = [[(0, c), (c, LONG_BLOCKS)] for c in LONG_CUTS]
LONG_SINGLE_BLOCKS = [(b, b + 1) for b in range(LONG_BLOCKS)]
LONG_SCHEDULES = LONG_TWO_RANGE + [LONG_SINGLE_BLOCKS]

FAMILIES = {"short": (SHORT_LENGTHS, SHORT_SCHEDULES), "long": (LONG_LENGTHS, LONG_SCHEDULES)}
MISALIGNMENTS = (0, 1, 2, 3)
TILE_PARTS = (len(SHORT_LENGTHS) + len(LONG_LENGTHS)) * len(MISALIGNMENTS)  # 124


def tiles(count: int = 1, seed: int = 1):
    """``count`` tiles: every length of both families once at each start misalignment 0-3
    (offset mod 64 = the misalignment), random bytes, fresh for every tile.  Returns (offsets,
    lengths, host buffer); the buffer has 64 bytes of slack behind the last part."""
    offs, lens, pos = [], [], 0
    for _ in range(count):
        for mis in MISALIGNMENTS:
            for L in SHORT_LENGTHS + LONG_LENGTHS:
                pos += (-pos) % 64 + mis
                offs.append(pos)
                lens.append(L)
                pos += L
    host = np.random.default_rng(seed).integers(0, 256, pos + 64, dtype=np.uint8)
    return np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint64), host


def slot_buffer(host, offs, lens, b0: int, b1: int, slot: int, fill: int = 0xEE, slack: int = 256):
    """The host ring's form of range [b0, b1): part j's bytes of the range at j * slot + (its
    offset mod 4) of a separate buffer, every other byte ``fill`` -- the bytes behind a part's
    end inside its slot, the whole slot of a part with nothing (or only its padding-only block)
    in the range, and ``slack`` bytes at the end.  Returns (slot offsets for the plan, buffer);
    launch with blk_origin = b0."""
    n = len(lens)
    assert slot >= 64 * (b1 - b0) + 64
    buf = np.full(n * slot + slack, fill, dtype=np.uint8)
    mis = np.asarray(offs, dtype=np.uint64) % np.uint64(4)
    slot_offs = np.arange(n, dtype=np.uint64) * np.uint64(slot) + mis
    for j in range(n):
        lo, hi = 64 * b0, min(64 * b1, int(lens[j]))
        if hi > lo:
            at = int(slot_offs[j])
            buf[at:at + hi - lo] = host[int(offs[j]) + lo:int(offs[j]) + hi]
    return slot_offs, buf
