"""Batched CRC-32C / CRC-32 of device-resident parts on the GPU (crc32_kernels.hip through the
C-ABI).  Expected values: CRC-32 from zlib.crc32 (independent); CRC-32C from s3h_cpu_crc, which
tests/test_crc_cpu.py pins to known answers and a bitwise reference."""
import zlib

import numpy as np
import pytest

import s3client_amd as s3
from tests import crc_shapes

pytestmark = pytest.mark.gpu
ALGOS = ("crc32c", "crc32")


def _expected(host, offs, lens, algo):
    if algo == "crc32":
        return np.array([zlib.crc32(host[int(o):int(o) + int(n)].tobytes()) for o, n in zip(offs, lens)],
                        dtype=np.uint32)
    return np.array([s3.crc(host[int(o):int(o) + int(n)], algo) for o, n in zip(offs, lens)],
                    dtype=np.uint32)


def _gpu(torch, host, offs, lens, algo):
    data = torch.from_numpy(host).cuda()
    return s3.crc_batch_device(data, offs, lens, algo).cpu().numpy().view(np.uint32)


def _check(got, want, offs, lens):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(i), int(offs[i]), int(lens[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]


@pytest.fixture(scope="module")
def mixed_batch():
    offs, lens, size = crc_shapes.mixed()
    host = crc_shapes.fill("random", size + 64, 11)
    return host, offs, lens, {a: _expected(host, offs, lens, a) for a in ALGOS}


@pytest.mark.parametrize("algo", ALGOS)
def test_boundary_batch(torch_cuda, algo):
    """Every boundary length, and those around multiples of the plan's segment size, at each
    start alignment 0-15; all-zero and all-0xFF data expose a wrong init or length term."""
    S = 1 << 14
    # this batch is far below 8,192 segments at any size, so the plan always yields 16 KiB here
    # and the loop ends at once; the other sizes are pinned in tests/test_gpu_crc_sizes.py
    for _ in range(4):
        offs, lens, size = crc_shapes.boundary_layout(S)
        with s3.CrcPlan(offs, lens, algo=algo) as plan:
            picked = plan.info()["segment_bytes"]
        if picked == S:
            break
        S = picked
    with s3.CrcPlan(offs, lens, algo=algo) as plan:
        info = plan.info()
        assert info["segment_bytes"] == S and info["n"] == len(lens)
        assert info["segments"] == int(((lens + (S - 1)) // S).sum())
        for kind in ("random", "zeros", "ones"):
            host = crc_shapes.fill(kind, size, 12)
            data = torch_cuda.from_numpy(host).cuda()
            out = torch_cuda.empty(len(lens), dtype=torch_cuda.int32, device="cuda")
            plan.launch(data, out)
            torch_cuda.cuda.synchronize()
            _check(out.cpu().numpy().view(np.uint32), _expected(host, offs, lens, algo), offs, lens)


@pytest.mark.parametrize("algo", ALGOS)
def test_segment_fold_of_one_large_part(torch_cuda, algo):
    offs, lens, size = crc_shapes.segment_fold()
    host = crc_shapes.fill("random", size, 13)
    with s3.CrcPlan(offs, lens, algo=algo) as plan:
        assert plan.info()["segments"] > 64  # more than one segment per stage-2 lane
    _check(_gpu(torch_cuda, host, offs, lens, algo), _expected(host, offs, lens, algo), offs, lens)


@pytest.mark.parametrize("algo", ALGOS)
def test_many_small_parts(torch_cuda, algo):
    """4,200 parts with 1-byte gaps: many stage-2 workgroups and a partial last one."""
    offs, lens, size = crc_shapes.many_small()
    host = crc_shapes.fill("random", size + 64, 14)
    _check(_gpu(torch_cuda, host, offs, lens, algo), _expected(host, offs, lens, algo), offs, lens)


@pytest.mark.parametrize("algo", ALGOS)
def test_mixed_segment_counts(torch_cuda, mixed_batch, algo):
    host, offs, lens, want = mixed_batch
    _check(_gpu(torch_cuda, host, offs, lens, algo), want[algo], offs, lens)


@pytest.mark.parametrize("algo", ALGOS)
def test_no_stale_partials(torch_cuda, mixed_batch, algo):
    """One plan launched on buffer A, on B with the same layout, on A again: each result
    follows its own buffer."""
    host_a, offs, lens, want = mixed_batch
    host_b = crc_shapes.fill("random", host_a.size, 15)
    want_b = _expected(host_b, offs, lens, algo)
    a, b = torch_cuda.from_numpy(host_a).cuda(), torch_cuda.from_numpy(host_b).cuda()
    outs = [torch_cuda.empty(len(lens), dtype=torch_cuda.int32, device="cuda") for _ in range(3)]
    with s3.CrcPlan(offs, lens, algo=algo) as plan:
        for buf, out in zip((a, b, a), outs):
            plan.launch(buf, out)
        torch_cuda.cuda.synchronize()
    for out, w in zip(outs, (want[algo], want_b, want[algo])):
        _check(out.cpu().numpy().view(np.uint32), w, offs, lens)


@pytest.mark.parametrize("algo", ALGOS)
def test_verify_flags_exactly_the_flipped_part(torch_cuda, mixed_batch, algo):
    host, offs, lens, want = mixed_batch
    expected = torch_cuda.from_numpy(want[algo].view(np.int32)).cuda()
    data = torch_cuda.from_numpy(host).cuda()
    count, mask = s3.crc_verify_batch_device(data, offs, lens, expected, algo)
    assert count == 0 and not bool(mask.any())
    k = 137
    assert lens[k] > 0
    flipped = host.copy()
    flipped[int(offs[k]) + int(lens[k]) // 2] ^= 0x40
    count, mask = s3.crc_verify_batch_device(torch_cuda.from_numpy(flipped).cuda(), offs, lens,
                                             expected, algo)
    assert count == 1
    assert np.flatnonzero(mask.cpu().numpy()).tolist() == [k]


def test_offsets_past_4_gib(torch_cuda):
    """Parts that straddle and lie beyond byte 2^32 of the buffer (64-bit segment offsets); only
    the bytes the parts cover are initialised."""
    top = 1 << 32
    data = torch_cuda.empty(top + (1 << 20), dtype=torch_cuda.uint8, device="cuda")
    offs = np.array([top - 100_003, top + 7, top + 300_001], dtype=np.uint64)
    lens = np.array([200_005, 250_000, 70_001], dtype=np.uint64)
    lo, hi = int(offs[0]), int(offs[-1] + lens[-1])
    host = crc_shapes.fill("random", hi - lo, 17)
    data[lo:hi] = torch_cuda.from_numpy(host).cuda()
    got = s3.crc_batch_device(data, offs, lens, "crc32").cpu().numpy().view(np.uint32)
    _check(got, _expected(host, offs - np.uint64(lo), lens, "crc32"), offs, lens)


@pytest.mark.parametrize("algo", ALGOS)
def test_object_checksum_from_gpu_part_crcs(torch_cuda, algo):
    """crc_object of the GPU's part CRCs (5 ragged parts of the 8 MiB + 5 buffer) equals the CPU
    CRC of the whole buffer."""
    _, _, size = crc_shapes.segment_fold()
    host = crc_shapes.fill("random", size, 16)
    total = size - 3
    cuts = [0, 1, 1 + (3 << 20) + 7, (5 << 20) + 123, (5 << 20) + 123, total]  # one empty part
    lens = np.diff(cuts).astype(np.uint64)
    offs = (3 + np.array(cuts[:-1])).astype(np.uint64)
    got = _gpu(torch_cuda, host, offs, lens, algo)
    whole = zlib.crc32(host[3:].tobytes()) if algo == "crc32" else s3.crc(host[3:], algo)
    assert s3.crc_object(got, lens, algo) == whole
