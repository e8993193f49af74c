"""s3h_verify_batch_routed on the CPU route, through the raw C ABI and with no GPU: every word of
a digest, corrupted alone in the expected values, flags exactly the corrupted parts; all n mask
bytes are written (0 or 1) into a buffer the test pre-fills, nothing behind them is touched, and
*mismatches is their sum.  Reference digests: hashlib (tests/verify_shapes.py).

The helpers here also serve the host cases of tests/test_gpu_verify.py."""
import ctypes

import numpy as np
import pytest

from s3client_amd import _native
from tests import verify_shapes as vs

FILL = 0xA5
MARGIN = 64
STALE = 0xDEADBEEFDEADBEEF  # *mismatches before the call: a call that adds instead of storing shows


class HostBatch:
    """vs.batch(n, seed) as pageable host parts: one pointer per part, every one of them inside
    the buffer (an empty part's too), with the reference digests of each algorithm asked for."""

    def __init__(self, n: int, seed: int, algos):
        self.data, self.offs, self.lens = vs.batch(n, seed)
        self.n = n
        parts = vs.parts_of(self.data, self.offs, self.lens)
        self.ref = {a: vs.expected(a, parts) for a in algos}
        self.addrs = (self.offs + np.uint64(self.data.ctypes.data)).astype(np.uint64)
        self.ptrs = self.addrs.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p))
        self.lens_p = self.lens.ctypes.data_as(_native.u64p)


def check_mask(mask: np.ndarray, n: int, count: int) -> np.ndarray:
    """The contract of every verification call; returns the n mask bytes."""
    assert set(np.unique(mask[:n]).tolist()) <= {0, 1}, np.unique(mask[:n])
    assert (mask[n:] == FILL).all(), "the call wrote behind mask byte n"
    assert count == int(mask[:n].sum())
    return mask[:n]


def verify_host(b: HostBatch, algo: str, exp: np.ndarray, route: str | None = None):
    """s3h_verify_batch_host (route None) or s3h_verify_batch_routed: (flagged rows, route taken)."""
    exp = np.ascontiguousarray(exp, dtype=np.uint32)
    assert exp.shape == (b.n, vs.WORDS[algo]) and exp.ctypes.data % 4 == 0
    mask = np.full(b.n + MARGIN, FILL, dtype=np.uint8)
    cnt = ctypes.c_uint64(STALE)
    taken = ctypes.c_int(-7)
    L = _native.lib()
    a = _native.ALGO_IDS[algo]
    if route is None:
        rc = L.s3h_verify_batch_host(a, b.ptrs, b.lens_p, b.n, exp.ctypes.data, mask.ctypes.data,
                                     ctypes.byref(cnt), 0)
    else:
        rc = L.s3h_verify_batch_routed(a, b.ptrs, b.lens_p, b.n, exp.ctypes.data, mask.ctypes.data,
                                       ctypes.byref(cnt), 0, _native.ROUTE_IDS[route],
                                       ctypes.byref(taken))
    _native.check(rc)
    got = check_mask(mask, b.n, cnt.value)
    return np.flatnonzero(got).tolist(), _native.ROUTE_NAMES.get(taken.value)


def check_each_word_alone(b: HostBatch, algo: str, word: int, route: str | None):
    """Rows HOST_ROWS corrupted in `word` only: the mask is exactly those rows."""
    rows, w = vs.word_alone_cases(algo, b.n, vs.HOST_ROWS)[word]
    flagged, taken = verify_host(b, algo, vs.corrupt(b.ref[algo], rows, w), route)
    assert flagged == sorted(rows), (algo, word, route)
    if route in ("gpu", "cpu", "split"):  # a forced route runs; AUTO may pick any
        assert taken == route


@pytest.fixture(scope="module")
def host_batch():
    return HostBatch(vs.N_HOST, 70, ("sha256", "md5"))


@pytest.mark.parametrize("algo, word", [(a, w) for a in ("sha256", "md5") for w in range(vs.WORDS[a])])
def test_cpu_route_each_word_alone(host_batch, algo, word):
    check_each_word_alone(host_batch, algo, word, "cpu")


@pytest.mark.parametrize("algo", ["sha256", "md5"])
def test_cpu_route_clean_and_every_row(host_batch, algo):
    """Reference values: every mask byte becomes 0 (the empty part 0 included) and the count is
    stored, not added to.  Every row corrupted in word r % words: all ones, count n."""
    b = host_batch
    assert verify_host(b, algo, b.ref[algo], "cpu") == ([], "cpu")
    rows, words = vs.every_row_case(algo, b.n)
    flagged, _ = verify_host(b, algo, vs.corrupt(b.ref[algo], rows, words), "cpu")
    assert flagged == list(range(b.n))
