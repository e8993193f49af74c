"""The CRC layouts that reach each of the plan's five segment sizes (crc_shapes.sized_layout,
two_pass_16k, many_small(n=20000)), on the CPU (no GPU): the properties tests/test_gpu_crc_sizes.py
relies on, and the host models of the kernels' decomposition (tests/cpp/crc_model.cpp,
crc_range_model.cpp, crc64_model.cpp) run at the real segment sizes 16-256 KiB -- crc_math.hpp
and crc64_math.hpp at x^(8S), tile counts and piece geometry no other test uses.  The models are
built and run by the functions of tests/test_crc_cpu.py, test_crc_range_cpu.py and
test_crc64_cpu.py."""
import subprocess

import numpy as np
import pytest

from tests import crc_shapes
from tests import test_crc64_cpu as whole64
from tests import test_crc_cpu as whole32
from tests import test_crc_range_cpu as ranged32

ALGOS32 = ("crc32c", "crc32")
LOG2S = tuple(range(crc_shapes.LOG2S_MIN, crc_shapes.LOG2S_MAX + 1))
# the plan's rule, s3client_amd/csrc/crc.cpp: kLog2SegMin = 14, kLog2SegMax = 18 and
# kMinSegments = 8192 (restated in crc_shapes; the GPU tests assert the plan's own segment_bytes)
assert (crc_shapes.LOG2S_MIN, crc_shapes.LOG2S_MAX, crc_shapes.MIN_SEGMENTS) == (14, 18, 8192)
THRESHOLD, SLACK = crc_shapes.MIN_SEGMENTS, 100


@pytest.fixture(scope="module")
def batches():
    """log2s -> (data, offsets, lengths) of sized_layout(log2s) with one random fill, made on
    first use."""
    cache = {}

    def get(log2s):
        if log2s not in cache:
            offs, lens, size = crc_shapes.sized_layout(log2s)
            cache[log2s] = (crc_shapes.fill("random", size, 30 + log2s), offs, lens)
        return cache[log2s]
    return get


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """The three models as the files named above build them; the sanitizer builds are the
    stand-alone ones of the whole-part models."""
    tmp = str(tmp_path_factory.mktemp("crc_sizes"))
    return {"whole32": {"plain": whole32._build_model(tmp, False), "san": whole32._build_model(tmp, True), "tmp": tmp},
            "ranged32": {"plain": ranged32._build(tmp, False), "tmp": tmp},
            "whole64": {"plain": whole64._build_model(tmp, False), "san": whole64._build_model(tmp, True), "tmp": tmp}}


# ------------------------------------------------------------------ the layouts
@pytest.mark.parametrize("log2s", LOG2S)
def test_sized_layout_lands_on_its_segment_size(log2s):
    S = 1 << log2s
    offs, lens, size = crc_shapes.sized_layout(log2s)
    at_s, at_2s = crc_shapes.segment_count(lens, S), crc_shapes.segment_count(lens, 2 * S)
    if log2s > crc_shapes.LOG2S_MIN:
        assert at_s >= THRESHOLD + SLACK
    if log2s < crc_shapes.LOG2S_MAX:
        assert at_2s <= THRESHOLD - SLACK
    # the core: every boundary length at each start alignment, and the 67-segment part
    for L in crc_shapes.BOUNDARY_LENGTHS + [S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S + 17]:
        assert {int(a) for a in offs[lens == L] % 16} == set(range(16)), L
    big = crc_shapes.SIZED_BIG_PART
    assert int(lens[big]) == 66 * S + 5 == int(lens.max()) and int(offs[big]) % 16 == 3
    assert int((lens == lens[big]).sum()) == 1
    # the fillers are one segment at every size
    small = (lens >= 1) & (lens < 3000)
    assert int(small.sum()) >= 7000 and crc_shapes.segment_count(lens[small], 1 << 14) == int(small.sum())
    # no two parts overlap and all lie inside the buffer
    order = np.argsort(offs, kind="stable")
    ends = offs[order] + lens[order]
    assert np.all(ends[:-1] <= offs[order][1:]) and int(ends.max()) <= size
    assert size <= 96 << 20


def test_two_pass_layout_stays_at_16_kib_with_more_than_one_pass():
    offs, lens, size = crc_shapes.two_pass_16k()
    assert crc_shapes.segment_count(lens, 1 << 15) <= THRESHOLD - 90
    assert crc_shapes.segment_count(lens, 1 << 14) >= THRESHOLD + 1000 + 90
    assert np.all(offs[1:] == offs[:-1] + lens[:-1] + 1) and int(offs[-1] + lens[-1]) == size
    assert size <= 96 << 20


def test_many_small_keeps_its_default_and_reaches_256_kib_at_20000():
    offs, lens, size = crc_shapes.many_small()
    assert len(lens) == 4200 and crc_shapes.segment_count(lens, 1 << 15) < THRESHOLD  # 16 KiB, as before
    again = crc_shapes.many_small(2, 4200)
    assert np.array_equal(again[0], offs) and np.array_equal(again[1], lens) and again[2] == size
    offs, lens, size = crc_shapes.many_small(n=20000)
    assert len(lens) == 20000 and int((lens == 0).sum()) > 0
    assert crc_shapes.segment_count(lens, 1 << 18) >= 16 * 1024 + 90  # 16 x (256 CUs x 4 workgroups)


# ------------------------------------------------------------------ the models at the real sizes
@pytest.mark.parametrize("algo", ALGOS32)
@pytest.mark.parametrize("log2s", LOG2S)
def test_model_whole_parts_at_each_segment_size(models, batches, algo, log2s):
    data, offs, lens = batches(log2s)
    whole32._run_model(models["whole32"], "plain", algo, log2s, data, offs, lens, f"w_{algo}_{log2s}")


@pytest.mark.parametrize("algo", ALGOS32)
@pytest.mark.parametrize("log2s", LOG2S)
def test_model_ranged_at_each_segment_size(models, batches, algo, log2s):
    data, offs, lens = batches(log2s)
    cuts = crc_shapes.sized_cuts(1 << log2s)
    name = f"sized_{log2s}"
    want = {(name, algo): ranged32.expected_crcs(data, offs, lens, algo)}
    ranged32._run(models["ranged32"], "plain", algo, (log2s, data, offs, lens), name, cuts,
                  [str(c) for c in cuts], want)


@pytest.mark.parametrize("log2s", LOG2S)
def test_model_crc64_whole_parts_at_each_segment_size(models, batches, log2s):
    data, offs, lens = batches(log2s)
    whole64._run_model(models["whole64"], "plain", log2s, data, offs, lens, f"w64_{log2s}")


@pytest.mark.parametrize("log2s", LOG2S)
def test_model_crc64_ranged_at_each_segment_size(models, batches, log2s):
    data, offs, lens = batches(log2s)
    cuts = crc_shapes.sized_cuts(1 << log2s)
    dpath, ppath = whole64._write(models["whole64"], f"r64_{log2s}", data, offs, lens)
    r = subprocess.run([models["whole64"]["plain"], str(log2s), dpath, ppath, *[str(c) for c in cuts]],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    rows = [l.split() for l in r.stdout.splitlines()]
    got = [int(c, 16) for c, _ in rows]
    want = whole64._expected(data, offs, lens)
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, [(i, int(offs[i]), int(lens[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
    assert [int(w) for _, w in rows] == whole64.writer_of([int(n) for n in lens], cuts)


def test_models_at_256_kib_under_sanitizers(models, batches):
    """The stand-alone ASan + UBSan builds of the whole-part models, once per width, at
    256 KiB: 256- and 257-tile segments read no line outside the parts' own."""
    data, offs, lens = batches(18)
    whole32._run_model(models["whole32"], "san", "crc32c", 18, data, offs, lens, "san_18")
    whole64._run_model(models["whole64"], "san", 18, data, offs, lens, "san64_18")
