"""tests/verify_shapes.py keeps what it exists for (no GPU, no library call): every word of every
value type is the only differing word in some case, the flipped bits reach all four bytes of a
word, the rows sit on the compare kernel's block edges, and the reference values equal the known
answers the repository commits.

This is also the argument that the device cases of tests/test_gpu_verify.py catch a compare
kernel that looks at fewer words or rows than it should: a kernel comparing `words - 1` words sees
no difference in the case that flips only the last word; one that stops at row 255, or skips row
n - 1, misses the rows below."""
import numpy as np
import pytest

from tests import verify_shapes as vs


def _diff(algo, n, rows, word):
    base = np.zeros((n, vs.WORDS[algo]), dtype=np.uint32)
    return vs.corrupt(base, rows, word) ^ base


def _popcount(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8)).reshape(a.shape[0], -1).sum(axis=1)


@pytest.mark.parametrize("algo", vs.ALGOS)
@pytest.mark.parametrize("n, rows", [(vs.N_DEVICE, None), (vs.N_HOST, vs.HOST_ROWS)])
def test_each_word_is_the_only_differing_word_once(algo, n, rows):
    cases = vs.word_alone_cases(algo, n, rows)
    assert [w for _, w in cases] == list(range(vs.WORDS[algo]))  # the last word / high half too
    for case_rows, w in cases:
        d = _diff(algo, n, case_rows, w)
        assert sorted(np.flatnonzero(d.any(axis=1))) == sorted(case_rows)
        assert set(np.flatnonzero(d.any(axis=0))) == {w}
        assert (_popcount(d)[list(case_rows)] == 1).all()  # one bit per corrupted row


@pytest.mark.parametrize("algo", vs.ALGOS)
def test_every_row_case_hits_each_row_once_and_each_word(algo):
    rows, words = vs.every_row_case(algo, vs.N_DEVICE)
    d = _diff(algo, vs.N_DEVICE, rows, words)
    assert (_popcount(d) == 1).all()
    assert set(np.flatnonzero(d.any(axis=0))) == set(range(vs.WORDS[algo]))
    assert np.array_equal(np.argmax(d != 0, axis=1), np.arange(vs.N_DEVICE) % vs.WORDS[algo])


def _bytes_hit(pairs):
    return {vs.bit(r, w) // 8 for r, w in pairs}


@pytest.mark.parametrize("algo", vs.ALGOS)
def test_bits_cover_all_four_bytes_of_a_word(algo):
    """Per value type over the device cases (each word alone + every row); the each-word-alone
    cases by themselves do for the digests and, taken over all value types, for any word."""
    alone = [(r, w) for rows, w in vs.word_alone_cases(algo, vs.N_DEVICE) for r in rows]
    rows, words = vs.every_row_case(algo, vs.N_DEVICE)
    assert _bytes_hit(alone + list(zip(rows, words))) == {0, 1, 2, 3}
    if algo in vs.DIGESTS:
        assert _bytes_hit(alone) == {0, 1, 2, 3}
        host = [(r, w) for rows, w in vs.word_alone_cases(algo, vs.N_HOST, vs.HOST_ROWS) for r in rows]
        assert _bytes_hit(host) == {0, 1, 2, 3}
    union = [(r, w) for a in vs.ALGOS for rows, w in vs.word_alone_cases(a, vs.N_DEVICE) for r in rows]
    assert _bytes_hit(union) == {0, 1, 2, 3}


def test_edge_rows():
    assert {255, 256, 512} <= set(vs.EDGE_ROWS(513))
    assert vs.EDGE_ROWS(513) == [0, 1, 63, 64, 255, 256, 257, 511, 512]
    assert vs.EDGE_ROWS(1) == [0]
    for n in vs.GRID_EDGE_N + (vs.N_HOST,):
        rows = vs.EDGE_ROWS(n)
        assert n - 1 in rows and max(rows) == n - 1 and len(set(rows)) == len(rows)
    assert {n % 256 for n in vs.GRID_EDGE_N + (vs.N_DEVICE,)} == {0, 1, 255}
    assert set(vs.HOST_ROWS) == set(vs.EDGE_ROWS(vs.N_HOST))


def test_batch_layout():
    data, offs, lens = vs.batch(vs.N_DEVICE, 3)
    assert lens[0] == 0 and lens[-1] == 200 and set(lens.tolist()) == set(vs.LENGTHS)
    assert np.array_equal(offs[1:], (offs + lens)[:-1] + vs.GAP)
    assert data.size == int(offs[-1] + lens[-1]) + vs.TAIL and 20 << 10 < data.size < 64 << 10
    again = vs.batch(vs.N_DEVICE, 3)
    assert all(np.array_equal(a, b) for a, b in zip((data, offs, lens), again))
    assert not np.array_equal(vs.batch(vs.N_DEVICE, 4)[0][:64], data[:64])
    for n in vs.GRID_EDGE_N:
        _, o, l = vs.batch(n, n)
        assert l.size == n and l[-1] == 200 and (n == 1 or l[0] == 0)


def test_corrupt_leaves_its_input_alone():
    exp = vs.expected("sha1", [b"a", b"b"])
    keep = exp.copy()
    out = vs.corrupt(exp, [1], 4)
    assert np.array_equal(exp, keep) and out[1, 4] == keep[1, 4] ^ np.uint32(1 << vs.bit(1, 4))


def test_expected_matches_the_committed_known_answers(golden):
    t = golden["transfer"]
    blob = (np.arange(t["size"], dtype=np.uint64) % 128).astype(np.uint8)
    parts = [blob[p["offset"]:p["offset"] + p["size"]].tobytes() for p in t["parts"]]
    assert vs.expected("sha256", parts).tobytes().hex() == "".join(p["digest"] for p in t["parts"])
    assert vs.expected("md5", parts).tobytes().hex() == "".join(p["digest"] for p in golden["md5"]["transfer"])
    assert vs.expected("sha256", [b""]).tobytes().hex() == golden["edge"][0]["digest"]
    m = [b"123456789", b""]
    assert vs.expected("crc32c", m).tolist() == [[0xE3069283], [0]]
    assert vs.expected("crc32", m).tolist() == [[0xCBF43926], [0]]
    # the 64-bit value 0xAE8B14860A799888 as stored: low half, then high half
    assert vs.expected("crc64nvme", m).tolist() == [[0x0A799888, 0xAE8B1486], [0, 0]]
    assert vs.expected("sha1", [b"abc"]).tobytes().hex() == "a9993e364706816aba3e25717850c26c9cd0d89d"
    for algo in vs.ALGOS:
        e = vs.expected(algo, m)
        assert e.dtype == np.uint32 and e.shape == (2, vs.WORDS[algo]) and e.flags.writeable
