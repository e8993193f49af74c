"""Layouts, reference values and corruption sets shared by the verification tests
(tests/test_verify_shapes_cpu.py, tests/test_verify_cpu.py, tests/test_gpu_verify.py).  Pure numpy
and the standard library: nothing here calls the library under test.

A verification call hashes n parts and compares each value, word by word, with an expected one.
The sets below exist to make every word of every value type, and every row at an edge of the
compare kernel's grid (256 threads per block), the ONLY thing that differs in some case."""
import hashlib
import zlib

import numpy as np

from tests import chunk_trailer_ref

ALGOS = ("sha256", "sha1", "md5", "crc32c", "crc32", "crc64nvme")
DIGESTS = ALGOS[:3]
# 32-bit words per value as stored; a CRC-64 value is two words, low half first (little-endian)
WORDS = {"sha256": 8, "sha1": 5, "md5": 4, "crc32c": 1, "crc32": 1, "crc64nvme": 2}
LENGTHS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 200)  # empty, and around both padding boundaries
GAP = 3
TAIL = 64  # bytes behind the last part, so that every part pointer lies inside the buffer
N_DEVICE = 513  # three blocks of the compare kernel, the last one with a single row
N_HOST = 70
HOST_ROWS = (0, 1, 63, 64, 69)
GRID_EDGE_N = (1, 255, 256, 257)


def batch(n: int, seed: int):
    """n parts with lengths drawn from LENGTHS -- part 0 empty, part n - 1 of 200 bytes (the one
    part of n = 1 has 200) -- 3-byte gaps, random bytes: (data uint8, offsets, lengths)."""
    rng = np.random.default_rng(seed)
    lens = rng.choice(np.array(LENGTHS, dtype=np.uint64), n)
    lens[0] = 0
    lens[n - 1] = 200
    offs = np.concatenate([[0], np.cumsum(lens + np.uint64(GAP))[:-1]]).astype(np.uint64)
    data = rng.integers(0, 256, int(offs[-1] + lens[-1]) + TAIL, dtype=np.uint8)
    return data, offs, lens


def parts_of(data: np.ndarray, offs, lens) -> list:
    return [data[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)]


def expected(algo: str, parts) -> np.ndarray:
    """(n, WORDS[algo]) uint32, the layout the library compares: hashlib for the digests,
    zlib.crc32 for CRC-32, the table CRCs of tests/chunk_trailer_ref.py for the other two."""
    if algo in DIGESTS:
        raw = b"".join(hashlib.new(algo, p).digest() for p in parts)
        return np.frombuffer(raw, dtype="<u4").reshape(len(parts), WORDS[algo]).copy()
    if algo == "crc64nvme":
        v = np.array([chunk_trailer_ref.crc64nvme(p) for p in parts], dtype="<u8")
        return v.view("<u4").reshape(len(parts), 2).copy()
    f = zlib.crc32 if algo == "crc32" else chunk_trailer_ref.crc32c
    return np.array([f(p) for p in parts], dtype="<u4").reshape(len(parts), 1)


def EDGE_ROWS(n: int) -> list:
    """Rows at the edges of the compare kernel's blocks and of the batch."""
    return sorted({r for r in (0, 1, 63, 64, 255, 256, 257, 511, 512) if r < n} | {n - 1})


def bit(row: int, word: int) -> int:
    return (7 * int(row) + 5 * int(word)) % 32


def corrupt(exp: np.ndarray, rows, word) -> np.ndarray:
    """A copy of exp with one bit of one word flipped in every row of `rows`:
    exp[r, w] ^= 1 << ((7 r + 5 w) % 32), w = `word` (an int, or one word index per row)."""
    out = exp.copy()
    rows = [int(r) for r in rows]
    words = [int(word)] * len(rows) if np.ndim(word) == 0 else [int(w) for w in word]
    assert len(words) == len(rows) and len(set(rows)) == len(rows)
    for r, w in zip(rows, words):
        out[r, w] ^= np.uint32(1 << bit(r, w))
    return out


def word_alone_cases(algo: str, n: int, rows=None) -> list:
    """One case per word of the value: (rows, word), the same rows corrupted in that word only."""
    rows = EDGE_ROWS(n) if rows is None else list(rows)
    return [(rows, w) for w in range(WORDS[algo])]


def every_row_case(algo: str, n: int):
    """Every row corrupted, row r in word r % WORDS: (rows, one word per row)."""
    rows = np.arange(n)
    return rows, rows % WORDS[algo]


def first_nonempty(lens, start: int) -> int:
    """The first row >= start that holds at least one byte (a data byte can be flipped there)."""
    return start + int(np.flatnonzero(np.asarray(lens[start:]) > 0)[0])
