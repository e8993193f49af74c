"""The comparison at the end of every verification call, on the GPU: the device forms
(s3h_verify_batch_device, s3h_crc_verify_batch_device, s3h_crc64nvme_verify_batch_device -- all
end in compare_digests_kernel) and the host forms (s3h_verify_batch_host, s3h_verify_batch_routed),
through the raw C ABI with a mask buffer of the test's own: n + 64 bytes of 0xA5.

The other GPU tests flip a DATA byte, which changes every word of a value; here the EXPECTED
values are wrong, in one bit of one word, so a compare that looks at too few words, too few rows,
writes the mask only on a mismatch, writes behind it or keeps an old count fails.  Reference
values come from hashlib / zlib / table CRCs (tests/verify_shapes.py), never from the library."""
import ctypes
import hashlib

import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests import verify_shapes as vs
from tests.test_verify_cpu import FILL, MARGIN, STALE, HostBatch, check_each_word_alone, check_mask, verify_host

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ device forms
class DeviceBatch:
    """vs.batch(n, seed) in HBM, with the reference values of each value type on demand."""

    def __init__(self, torch, n: int, seed: int):
        self.torch = torch
        self.host, self.offs, self.lens = vs.batch(n, seed)
        self.n = n
        self.parts = vs.parts_of(self.host, self.offs, self.lens)
        self.data = torch.from_numpy(self.host).cuda()
        self._ref = {}

    def ref(self, algo: str) -> np.ndarray:
        if algo not in self._ref:
            self._ref[algo] = vs.expected(algo, self.parts)
            self._ref[algo].flags.writeable = False  # shared among the tests: left unchanged
        return self._ref[algo]


def _to_device(torch, exp: np.ndarray):
    """Expected values as a device tensor of their own (torch aligns it to >= 256 bytes)."""
    t = torch.from_numpy(np.ascontiguousarray(exp, dtype=np.uint32).view(np.int32).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _new_mask(torch, n: int):
    return torch.full((n + MARGIN,), FILL, dtype=torch.uint8, device="cuda")


def _verify(torch, algo, data, offs, lens, d_exp, d_mask=None, stream: int = 0):
    """One raw verification call of the value type's entry point on `stream` (a hipStream_t;
    0 = the null stream).  Checks the mask contract and returns the flagged rows."""
    n = int(lens.size)
    assert d_exp.numel() * d_exp.element_size() == 4 * vs.WORDS[algo] * n
    if d_mask is None:
        d_mask = _new_mask(torch, n)
        torch.cuda.synchronize()  # the fill ran on torch's stream, the call may run on another
    assert d_mask.numel() == n + MARGIN
    cnt = ctypes.c_uint64(STALE)
    L = _native.lib()
    dev = data.device.index
    args = (ctypes.c_void_p(data.data_ptr()), offs.ctypes.data_as(_native.u64p),
            lens.ctypes.data_as(_native.u64p), n, ctypes.c_void_p(d_exp.data_ptr()),
            ctypes.c_void_p(d_mask.data_ptr()), ctypes.byref(cnt), ctypes.c_void_p(stream))
    if algo in vs.DIGESTS:
        rc = L.s3h_verify_batch_device(dev, _native.ALGO_IDS[algo], *args)
    elif algo == "crc64nvme":
        rc = L.s3h_crc64nvme_verify_batch_device(dev, *args)
    else:
        rc = L.s3h_crc_verify_batch_device(dev, _native.CRC_IDS[algo], *args)
    _native.check(rc)  # blocking: `stream` has drained
    mask = check_mask(d_mask.cpu().numpy(), n, cnt.value)
    return np.flatnonzero(mask).tolist()


@pytest.fixture(scope="module")
def dev513(torch_cuda):
    return DeviceBatch(torch_cuda, vs.N_DEVICE, 513)


@pytest.mark.parametrize("algo", vs.ALGOS)
def test_clean_batch_clears_every_mask_byte(dev513, algo):
    """Reference values as expected: count 0 and all n bytes 0 although the buffer held 0xA5
    (check_mask: bytes [0, n) are 0 or 1); the empty part 0 is not flagged."""
    b = dev513
    assert b.lens[0] == 0
    assert _verify(b.torch, algo, b.data, b.offs, b.lens, _to_device(b.torch, b.ref(algo))) == []


@pytest.mark.parametrize("algo, word", [(a, w) for a in vs.ALGOS for w in range(vs.WORDS[a])])
def test_each_word_alone(dev513, algo, word):
    """Rows 0, 1, 63, 64, 255, 256, 257, 511, 512 of 513 differ in one bit of `word` and in
    nothing else: the mask is 1 exactly there."""
    b = dev513
    rows, w = vs.word_alone_cases(algo, b.n)[word]
    d_exp = _to_device(b.torch, vs.corrupt(b.ref(algo), rows, w))
    assert _verify(b.torch, algo, b.data, b.offs, b.lens, d_exp) == rows


@pytest.mark.parametrize("n", vs.GRID_EDGE_N)
@pytest.mark.parametrize("algo", ["sha256", "sha1", "crc64nvme"])
def test_grid_edges(torch_cuda, algo, n):
    """n % 256 in {1, 255, 0, 1}: only row n - 1 differs, in its last word."""
    b = DeviceBatch(torch_cuda, n, 1000 + n)
    d_exp = _to_device(b.torch, vs.corrupt(b.ref(algo), [n - 1], vs.WORDS[algo] - 1))
    assert _verify(b.torch, algo, b.data, b.offs, b.lens, d_exp) == [n - 1]


@pytest.mark.parametrize("algo", vs.ALGOS)
def test_every_row(dev513, algo):
    """Every row differs, row r in word r % words: three blocks add to one counter."""
    b = dev513
    rows, words = vs.every_row_case(algo, b.n)
    d_exp = _to_device(b.torch, vs.corrupt(b.ref(algo), rows, words))
    assert _verify(b.torch, algo, b.data, b.offs, b.lens, d_exp) == list(range(b.n))


@pytest.mark.parametrize("algo", vs.ALGOS)
def test_data_and_expected_together(dev513, algo):
    """A data byte flipped in row i, an expected last word corrupted in row j: exactly {i, j}.
    Then row k with both its data and its expected value changed (it still differs): flagged
    once, the count is 3."""
    b = dev513
    last = vs.WORDS[algo] - 1
    i, j, k = vs.first_nonempty(b.lens, 256), 511, vs.first_nonempty(b.lens, 63)
    assert len({i, j, k}) == 3
    host = b.host.copy()
    host[int(b.offs[i]) + int(b.lens[i]) - 1] ^= 0x10
    data = b.torch.from_numpy(host).cuda()
    d_exp = _to_device(b.torch, vs.corrupt(b.ref(algo), [j], last))
    assert _verify(b.torch, algo, data, b.offs, b.lens, d_exp) == sorted([i, j])
    host[int(b.offs[k])] ^= 0x01
    data = b.torch.from_numpy(host).cuda()
    d_exp = _to_device(b.torch, vs.corrupt(b.ref(algo), [j, k], last))
    assert _verify(b.torch, algo, data, b.offs, b.lens, d_exp) == sorted([i, j, k])


@pytest.mark.parametrize("algo", vs.ALGOS)
def test_no_carry_over_between_calls(dev513, algo):
    """The same mask buffer, not re-filled: a corrupted call (count k), then a clean one, which
    reports 0 and clears the k bytes."""
    b = dev513
    rows = vs.EDGE_ROWS(b.n)
    mask = _new_mask(b.torch, b.n)
    b.torch.cuda.synchronize()
    d_bad = _to_device(b.torch, vs.corrupt(b.ref(algo), rows, vs.WORDS[algo] - 1))
    assert _verify(b.torch, algo, b.data, b.offs, b.lens, d_bad, mask) == rows
    assert int(mask[:b.n].sum().item()) == len(rows)
    assert _verify(b.torch, algo, b.data, b.offs, b.lens, _to_device(b.torch, b.ref(algo)), mask) == []


def test_stream_order(dev513):
    """The compare runs in stream order behind whatever wrote `expected` on the same stream.

    A SHA-256 plan over the 513 small parts and one of 4 MiB (a serial chain of tens of
    milliseconds) is launched on a side stream into `expected`, which holds a sentinel; with no
    host synchronisation in between, the verification call on that stream must read the finished
    digests (count 0).  One word is then corrupted by a torch op issued on the stream, and the
    next call must see it (count 1, that row).

    Scheduling could hide an ordering bug here -- the plan may happen to finish before the
    compare starts -- but it can never invent one: a failure of this test is a real defect."""
    torch, b = dev513.torch, dev513
    big = np.random.default_rng(4).integers(0, 256, (4 << 20) + vs.TAIL, dtype=np.uint8)
    host = np.concatenate([b.host, big])
    offs = np.concatenate([b.offs, [b.host.size]]).astype(np.uint64)
    lens = np.concatenate([b.lens, [4 << 20]]).astype(np.uint64)
    n = b.n + 1
    ref = np.concatenate([b.ref("sha256"),
                          np.frombuffer(hashlib.sha256(big[:4 << 20].tobytes()).digest(), dtype="<u4")[None]])
    data = torch.from_numpy(host).cuda()
    expected = torch.full((n, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    mask = _new_mask(torch, n)
    side = torch.cuda.Stream()
    row = 256
    flip = int(np.array([1 << vs.bit(row, 7)], dtype=np.uint32).view(np.int32)[0])
    with s3.Plan(offs, lens, algo="sha256") as plan:
        torch.cuda.synchronize()  # uploads and fills done; from here on only `side` is used
        plan.launch(data, expected, stream=side)
        assert _verify(torch, "sha256", data, offs, lens, expected, mask, side.cuda_stream) == []
        with torch.cuda.stream(side):
            expected[row, 7] ^= flip
        assert _verify(torch, "sha256", data, offs, lens, expected, mask, side.cuda_stream) == [row]
        plan.status(side)
    assert np.array_equal(expected.cpu().numpy().view(np.uint32), vs.corrupt(ref, [row], 7))


# ------------------------------------------------------------------ host forms
@pytest.fixture(scope="module")
def host70(torch_cuda):
    return HostBatch(vs.N_HOST, 70, vs.DIGESTS)  # the parts of tests/test_verify_cpu.py


@pytest.mark.parametrize("algo", vs.DIGESTS)
def test_host_each_word_alone(host70, algo):
    """s3h_verify_batch_host, pageable parts: rows 0, 1, 63, 64, 69 differ in one word only."""
    assert verify_host(host70, algo, host70.ref[algo]) == ([], None)
    for word in range(vs.WORDS[algo]):
        check_each_word_alone(host70, algo, word, None)


@pytest.mark.parametrize("route", ["gpu", "cpu", "split", "auto"])
@pytest.mark.parametrize("algo", ["sha256", "md5"])
def test_routed_each_word_alone(host70, algo, route):
    """s3h_verify_batch_routed on every route (SHA-1 stays refused there:
    tests/test_sha1_cpu.py); a forced route reports itself as taken."""
    flagged, _ = verify_host(host70, algo, host70.ref[algo], route)
    assert flagged == []
    for word in range(vs.WORDS[algo]):
        check_each_word_alone(host70, algo, word, route)


def test_hex_string_path_of_the_wrapper(host70):
    """verify_batch_host given hex strings, one differing in its last character (the top of the
    last word's last byte as stored): exactly that part is flagged."""
    b = host70
    views = [b.data[int(o):int(o) + int(n)] for o, n in zip(b.offs, b.lens) if n]
    for algo, row in (("sha256", len(views) - 1), ("md5", len(views) // 2), ("sha1", 0)):
        hexes = [hashlib.new(algo, v.tobytes()).hexdigest() for v in views]
        assert not s3.verify_batch_host(views, hexes, algo=algo).any()
        hexes[row] = hexes[row][:-1] + ("0" if hexes[row][-1] != "0" else "1")
        assert np.flatnonzero(s3.verify_batch_host(views, hexes, algo=algo)).tolist() == [row]
