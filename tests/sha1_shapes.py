"""Part layouts and launch schedules for the two instantiations of the SHA-1 kernel
(sha1_pc_kernel<1> for plans with more workgroups than CUs, sha1_pc_kernel<2> otherwise) and the
hashlib reference they are compared with: tests/test_sha1_shapes_cpu.py checks that the layouts
keep what they exist for, tests/test_gpu_sha1_forms.py runs them on the GPU.

A schedule is a list of block ranges [b0, b1) launched in order on one plan, as in
tests/range_shapes.py; END stands for the plan's max_blocks."""
import hashlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests import range_shapes as rs

END = None
# Starts at odd and even blocks, ranges of odd length (a partial 2-block step at the end of a
# launch) and resumes in the middle of the loops in which every chain of a workgroup is live.
MANY_SCHEDULE = [(0, 1), (1, 2), (2, 37), (37, 38), (38, 63), (63, 64), (64, END)]
LONG_SCHEDULE = [(0, 1), (1, 2), (2, 37), (37, 138), (138, 139), (139, 640), (640, END)]
EDGE_PARTS = 128           # padding-edge lengths among the parts of many()
MANY_LONG = (4096, 6144)   # bytes of the other parts: 65-97 blocks
LONG70 = (40 << 10, 48 << 10)  # 641-769 blocks
REF_THREADS = 16


def schedule(sched, max_blocks: int):
    """``sched`` with END replaced by the plan's max_blocks."""
    return [(b0, max_blocks if b1 is END else b1) for b0, b1 in sched]


def nb(lens) -> np.ndarray:
    """range_shapes.nb over an array of lengths."""
    return (np.asarray(lens, dtype=np.uint64) + np.uint64(72)) >> np.uint64(6)


def due(nblocks, b0: int, b1: int) -> np.ndarray:
    """range_shapes.due over an array of block counts: the parts whose digest launch [b0, b1)
    writes."""
    nblocks = np.asarray(nblocks)
    return (nblocks > b0) & (nblocks <= b1)


def slot_order(lens) -> np.ndarray:
    """Part index of each slot: descending length, equal lengths in part order (plan.cpp
    sort_slots).  Workgroup g runs slots [64 g, 64 g + 64)."""
    return np.argsort(-np.asarray(lens, dtype=np.int64), kind="stable")


def _layout(rng, lens, gaps):
    lens = np.asarray(lens, dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens + gaps.astype(np.uint64))[:-1]]).astype(np.uint64)
    host = rng.integers(0, 256, int(offs[-1] + lens[-1]) + 64, dtype=np.uint8)
    return offs, lens, host


def many(cus: int, seed: int = 1):
    """64 x cus + 70 parts: a grid of cus + 2 workgroups, the last of 6 parts.  128 parts have
    the tile's padding-edge lengths, the others U[4096, 6144] bytes; shuffled; U[0, 8] bytes
    between parts, so the start alignments cover 0-63.  Returns (offsets, lengths, host buffer)
    with 64 bytes of slack behind the last part."""
    rng = np.random.default_rng(seed)
    n = 64 * cus + 70
    edge = rs.SHORT_LENGTHS + rs.LONG_LENGTHS
    edge = (edge * (EDGE_PARTS // len(edge) + 1))[:EDGE_PARTS]
    lens = np.concatenate([edge, rng.integers(MANY_LONG[0], MANY_LONG[1] + 1, n - EDGE_PARTS)])
    rng.shuffle(lens)
    return _layout(rng, lens, rng.integers(0, 9, n))


def long70(seed: int = 2):
    """70 parts of U[40, 48] KiB, 3 bytes apart: one full workgroup whose shortest part has at
    least 641 blocks, and a partial one."""
    rng = np.random.default_rng(seed)
    return _layout(rng, rng.integers(LONG70[0], LONG70[1] + 1, 70), np.full(70, 3))


def _digests(name, words, host, offs, lens):
    mv = memoryview(np.ascontiguousarray(host))
    offs, lens = [int(o) for o in offs], [int(n) for n in lens]
    new = getattr(hashlib, name)

    def run(lo, hi):
        return b"".join(new(mv[offs[i]:offs[i] + lens[i]]).digest() for i in range(lo, hi))

    n = len(lens)
    step = max(1, min(512, (n + REF_THREADS - 1) // REF_THREADS))
    with ThreadPoolExecutor(REF_THREADS) as pool:
        raw = b"".join(pool.map(lambda lo: run(lo, min(lo + step, n)), range(0, n, step)))
    return np.frombuffer(raw, dtype=np.uint32).reshape(n, words)


def sha1_ref(host, offs, lens) -> np.ndarray:
    """hashlib.sha1 of every part: (n, 5) uint32, the digest bytes as stored."""
    return _digests("sha1", 5, host, offs, lens)


def md5_ref(host, offs, lens) -> np.ndarray:
    return _digests("md5", 4, host, offs, lens)


def sha256_ref(host, offs, lens) -> np.ndarray:
    return _digests("sha256", 8, host, offs, lens)
