"""Part layouts shared by the CRC tests: tests/test_crc_cpu.py runs them through the host model
of the kernels' decomposition (tests/cpp/crc_model.cpp) at a reduced segment size, and
tests/test_gpu_crc.py through the GPU at the plan's own.  sized_layout, two_pass_16k and
many_small(n=20000) steer the plan to each of its segment sizes and past one grid pass
(tests/test_crc_sizes_cpu.py, tests/test_gpu_crc_sizes.py)."""
import numpy as np

POLY = {"crc32c": 0x82F63B78, "crc32": 0xEDB88320}
BOUNDARY_LENGTHS = [0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025,
                    4095, 4096, 4097]


def boundary_layout(S: int):
    """Every boundary length (and those around multiples of the segment size S) once at each
    start alignment 0-15: (offsets, lengths, buffer size)."""
    lengths = BOUNDARY_LENGTHS + [S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S + 17]
    offs, lens, cur = [], [], 0
    for L in lengths:
        for a in range(16):
            cur = (cur + 15) // 16 * 16 + a
            offs.append(cur)
            lens.append(L)
            cur += L
    return np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint64), cur


def fill(kind: str, size: int, seed: int = 1) -> np.ndarray:
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)
    return np.full(size, 0 if kind == "zeros" else 0xFF, dtype=np.uint8)


def segment_fold():
    """One part of 8 MiB + 5 bytes at offset 3: many segments of one part."""
    L = (8 << 20) + 5
    return np.array([3], dtype=np.uint64), np.array([L], dtype=np.uint64), 3 + L


def many_small(seed: int = 2, n: int = 4200):
    """n parts of U[0, 3000) bytes with 1-byte gaps.  At n = 20,000 a plan has more than 16,384
    one-tile segments: it picks 256 KiB and stage 1 takes three grid passes of 8,192 waves (four
    of CRC-64's 6,144)."""
    lens = np.random.default_rng(seed).integers(0, 3000, n).astype(np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens + 1)[:-1]]).astype(np.uint64)
    return offs, lens, int(offs[-1] + lens[-1])


# The plan's segment rule (s3client_amd/csrc/crc.cpp: kLog2SegMin, kLog2SegMax, kMinSegments):
# the largest S = 2^log2s, log2s in 14..18, that still cuts the batch into 8,192 segments.
LOG2S_MIN, LOG2S_MAX, MIN_SEGMENTS = 14, 18, 8192
SIZED_SLACK = 100     # segments between a sized layout's counts at S and 2S and the threshold
SIZED_BIG_PART = 0    # index of the 66 S + 5 part in sized_layout()
SIZED_RAMP = 72       # parts of S+1 .. S+72 bytes in sized_layout()


def segment_count(lens, S: int) -> int:
    return int(((np.asarray(lens, dtype=np.uint64) + np.uint64(S - 1)) // np.uint64(S)).sum())


def _fillers(rng, count: int, start: int):
    """count parts of U[1, 3000) bytes with 1-byte gaps from `start`: one segment each at every
    segment size."""
    lens = rng.integers(1, 3000, count).astype(np.uint64)
    offs = (np.uint64(start) + np.concatenate([[0], np.cumsum(lens + 1)[:-1]])).astype(np.uint64)
    return offs, lens, int(offs[-1] + lens[-1])


def sized_layout(log2s: int):
    """A batch for which the plan picks S = 2^log2s (log2s in 14..18), with at least SIZED_SLACK
    segments to spare on either side: (offsets, lengths, buffer size).
      * part 0: 66 S + 5 bytes at offset 3 -- 67 segments, stage 2 with c = 2 and 62 virtual
        zero values in front; it comes first so that it has the lowest index (the host models
        lay a range's bytes out at index * range length);
      * boundary_layout(S), moved up by a multiple of 16 (every start alignment kept);
      * SIZED_RAMP parts of S+1 .. S+72 bytes at start alignments 0-15 in turn.  Each is two
        segments at S and one at 2 S: with the parts above alone the two counts lie 129 apart,
        which leaves no room for the slack on both sides;
      * fillers, as many as put the count at S at MIN_SEGMENTS + SIZED_SLACK.  The count at 2 S
        is then at most MIN_SEGMENTS - SIZED_SLACK (asserted)."""
    assert LOG2S_MIN <= log2s <= LOG2S_MAX
    S = 1 << log2s
    offs, lens = [3], [66 * S + 5]
    cur = 3 + lens[0]
    base = (cur + 15) // 16 * 16
    b_offs, b_lens, b_size = boundary_layout(S)
    offs += [base + int(o) for o in b_offs]
    lens += [int(n) for n in b_lens]
    cur = base + b_size
    for i in range(SIZED_RAMP):
        cur = (cur + 15) // 16 * 16 + i % 16
        offs.append(cur)
        lens.append(S + 1 + i)
        cur += lens[-1]
    count = MIN_SEGMENTS + SIZED_SLACK - segment_count(lens, S)
    assert segment_count(lens, 2 * S) + count <= MIN_SEGMENTS - SIZED_SLACK
    f_offs, f_lens, size = _fillers(np.random.default_rng(100 + log2s), count, cur + 1)
    return (np.concatenate([np.array(offs, dtype=np.uint64), f_offs]),
            np.concatenate([np.array(lens, dtype=np.uint64), f_lens]), size)


def sized_cuts(S: int):
    """Range ends for sized_layout at segment size S: byte 1, either side of the first segment
    boundary and on it, inside later segments, the end of the 3S + 17 parts and one byte short
    of it, deep inside the 66S + 5 part (on the segment grid and one byte off it) and its end."""
    return [1, S - 1, S, S + 1, 2 * S + 5, 3 * S + 16, 3 * S + 17, 64 * S, 65 * S + 1, 66 * S + 5]


def two_pass_16k(seed: int = 5):
    """4,000 parts of U(16 KiB, 24 KiB] bytes with 1-byte gaps and 4,100 fillers: 8,100 segments
    at 32 KiB, so the plan stays at 16 KiB, and 12,100 segments there -- more than one grid pass
    of 8,192 waves.  About 84 MB."""
    rng = np.random.default_rng(seed)
    lens = rng.integers((16 << 10) + 1, (24 << 10) + 1, 4000).astype(np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens + 1)[:-1]]).astype(np.uint64)
    f_offs, f_lens, size = _fillers(rng, 4100, int(offs[-1] + lens[-1]) + 1)
    return np.concatenate([offs, f_offs]), np.concatenate([lens, f_lens]), size


def mixed(seed: int = 0):
    """300 parts of U[0, 70000) and one of 8 MiB, 3-byte gaps (the smoke run's shape)."""
    lens = np.random.default_rng(seed).integers(0, 70000, 300)
    lens[:4] = [0, 55, 56, 8 << 20]
    offs = np.concatenate([[0], np.cumsum(lens + 3)[:-1]])
    return offs.astype(np.uint64), lens.astype(np.uint64), int(offs[-1] + lens[-1])

