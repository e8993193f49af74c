"""Part layouts shared by the CRC tests: tests/test_crc_cpu.py runs them through the host model
of the kernels' decomposition (tests/cpp/crc_model.cpp) at a reduced segment size, and
tests/test_gpu_crc.py through the GPU at the plan's own."""
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


def many_small(seed: int = 2):
    """4,200 parts of U[0, 3000) bytes with 1-byte gaps."""
    lens = np.random.default_rng(seed).integers(0, 3000, 4200).astype(np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens + 1)[:-1]]).astype(np.uint64)
    return offs, lens, int(offs[-1] + lens[-1])


def mixed(seed: int = 0):
    """300 parts of U[0, 70000) and one of 8 MiB, 3-byte gaps (the smoke run's shape)."""
    lens = np.random.default_rng(seed).integers(0, 70000, 300)
    lens[:4] = [0, 55, 56, 8 << 20]
    offs = np.concatenate([[0], np.cumsum(lens + 3)[:-1]])
    return offs.astype(np.uint64), lens.astype(np.uint64), int(offs[-1] + lens[-1])

