"""Helpers shared by the caller-contract tests (tests/test_gpu_stream_order.py,
tests/test_gpu_buffer_contract.py, tests/test_buffer_contract_cpu.py): reference values from
hashlib / zlib / the table CRCs (tests/verify_shapes.py) and the chunk-signing references, the
"sandwich" that makes a launch's stream order observable, and a tensor stand-in for the CPU
tests.  Nothing here computes a reference with the library under test.  torch is only touched
through the module a test hands in."""
import functools
import hashlib

import numpy as np

import s3client_amd as s3
from tests import verify_shapes as vs

SENTINEL = 0x5A5AA5A5   # what every output holds before a launch, and its margin for ever
CONSUMED = 0x3C3CC3C3   # what the consumer writes over an output once it has read it
MARGIN = 64             # sentinel words behind every output
DELAY_BYTES = 4 << 20   # one SHA-256 part of this size: a serial chain of tens of milliseconds


def i32(word: int) -> int:
    """A 32-bit pattern as the Python int torch takes for an int32 fill."""
    return int(np.array([word], dtype=np.uint32).view(np.int32)[0])


# ------------------------------------------------------------------ batches and references
def ragged(n: int, seed: int, hi: int = 300, gap: int = 3, lo: int = 0):
    """n parts of lo .. hi bytes (part 0 of lo bytes, part 1 of hi bytes), `gap`-byte gaps,
    random bytes: (data uint8, offsets, lengths), as tests/verify_shapes.batch lays its parts out."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, n).astype(np.uint64)
    lens[0] = lo
    if n > 1:
        lens[1] = hi
    offs = np.concatenate([[0], np.cumsum(lens + np.uint64(gap))[:-1]]).astype(np.uint64)
    data = rng.integers(0, 256, int(offs[-1] + lens[-1]) + vs.TAIL, dtype=np.uint8)
    return data, offs, lens


def poison_of(host: np.ndarray) -> np.ndarray:
    return host ^ np.uint8(0xFF)


class Refs:
    """Reference values of one layout over its good bytes, computed once per value type and left
    unchanged.  ref() also proves that a launch reading the bytes too early cannot pass: the
    poison's values differ from the good bytes' in every row that holds a byte."""

    def __init__(self, host, offs, lens):
        self.host, self.offs, self.lens = host, offs, lens
        self.n = int(lens.size)
        self._ref = {}

    def ref(self, algo: str) -> np.ndarray:
        if algo not in self._ref:
            r = vs.expected(algo, vs.parts_of(self.host, self.offs, self.lens))
            bad = vs.expected(algo, vs.parts_of(poison_of(self.host), self.offs, self.lens))
            differ = (r != bad).any(axis=1)
            assert differ[self.lens > 0].all(), "poison and good bytes must differ in every non-empty row"
            r.flags.writeable = False
            self._ref[algo] = r
        return self._ref[algo]


@functools.lru_cache(maxsize=None)
def vs_refs(n: int, seed: int) -> Refs:
    return Refs(*vs.batch(n, seed))


@functools.lru_cache(maxsize=None)
def ragged_refs(n: int, seed: int, hi: int = 300, gap: int = 3, lo: int = 0) -> Refs:
    return Refs(*ragged(n, seed, hi, gap, lo))


def rows_differ(got: np.ndarray, want: np.ndarray) -> str:
    """'' when equal, otherwise a short description of the rows that differ."""
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
    return "" if bad.size == 0 else f"{bad.size} of {len(want)} rows differ, first {bad[:8].tolist()}"


# ------------------------------------------------------------------ the sandwich
_delay_cache = {}


def _delay(torch):
    """The delay launch's plan, part and scratch output, made once (one part of DELAY_BYTES)."""
    if "d" not in _delay_cache:
        part = torch.from_numpy(np.random.default_rng(4).integers(0, 256, DELAY_BYTES, dtype=np.uint8)).cuda()
        plan = s3.Plan([0], [DELAY_BYTES], algo="sha256")
        out = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
        _delay_cache["d"] = (plan, part, out)
    return _delay_cache["d"]


class Sandwich:
    """delay -> producer -> [the launch under test] -> consumer, all on one fresh side stream S
    with no host synchronisation in between.

    `data` holds poison (good ^ 0xFF) when the launch is enqueued; the good bytes arrive by a
    copy on S that cannot have run yet, because S is still busy with the delay launch (one
    SHA-256 part of 4 MiB, a serial chain of tens of milliseconds).  Behind the launch, still on
    S, every output is snapshotted and then overwritten.  A launch, or one kernel / memset /
    copy of a multi-step launch, that is not ordered on S therefore reads poison, or writes
    after the consumer, and the snapshot differs from the reference.  Scheduling can hide such
    a bug (the stray kernel may happen to run late enough) but can never invent one."""

    def __init__(self, torch, good_host: np.ndarray):
        self.torch = torch
        self.good = torch.from_numpy(np.array(good_host, order="C")).cuda()  # (a writable copy)
        self.data = ~self.good  # poison: every bit flipped (bytes ^ 0xFF; words likewise)
        self.S = torch.cuda.Stream()
        self.outs = []
        self.delay = _delay(torch)

    def output(self, words: int):
        """A sentinel-filled int32 output of `words` words plus the margin (256-byte aligned)."""
        t = self.torch.full((words + MARGIN,), i32(SENTINEL), dtype=self.torch.int32, device="cuda")
        snap = self.torch.zeros_like(t)
        self.outs.append((t, snap, words))
        return t

    def open(self, produce: bool = True):
        """Everything set up so far is made visible; from here on only S is used."""
        self.torch.cuda.synchronize()
        plan, part, out = self.delay
        plan.launch(part, out, stream=self.S)
        if produce:
            with self.torch.cuda.stream(self.S):
                self.data.copy_(self.good, non_blocking=True)
        return self.S

    def close(self, *plans) -> list:
        """Consumer and end: the snapshots' payload words as uint32 arrays, in output() order.
        The margin of every snapshot and every overwritten output are checked here."""
        with self.torch.cuda.stream(self.S):
            for t, snap, _ in self.outs:
                snap.copy_(t, non_blocking=True)
                t.fill_(i32(CONSUMED))
        self.S.synchronize()
        for p in plans:
            p.status(self.S)
        self.delay[0].status(self.S)
        got = []
        for t, snap, words in self.outs:
            w = snap.cpu().numpy().view(np.uint32)
            assert (w[words:] == SENTINEL).all(), "words behind an output were written"
            assert (t.cpu().numpy().view(np.uint32) == CONSUMED).all(), \
                "an output was written after the consumer had overwritten it"
            got.append(w[:words].copy())
        return got


# ------------------------------------------------------------------ tensor stand-in (CPU tests)
class FakeDevice:
    def __init__(self, index):
        self.index = index


class FakeTensor:
    """What the buffer validator looks at, without torch or a device."""

    def __init__(self, nbytes: int = 4096, ptr: int = 0x7F0000001000, cuda: bool = True,
                 device: int = 0, contiguous: bool = True, itemsize: int = 1):
        assert nbytes % itemsize == 0
        self.is_cuda = cuda
        self.device = FakeDevice(device if cuda else None)
        self._contiguous, self._ptr, self._n, self._item = contiguous, ptr, nbytes // itemsize, itemsize

    def is_contiguous(self) -> bool:
        return self._contiguous

    def data_ptr(self) -> int:
        return self._ptr if self._n else 0  # torch: an empty tensor has a null data_ptr()

    def numel(self) -> int:
        return self._n

    def element_size(self) -> int:
        return self._item


def sha256_words(parts) -> np.ndarray:
    raw = b"".join(hashlib.sha256(p).digest() for p in parts)
    return np.frombuffer(raw, dtype="<u4").reshape(len(parts), 8).copy()
