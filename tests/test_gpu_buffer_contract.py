"""The buffers a device launch is handed: what the Python wrappers refuse before anything is
launched (non-contiguous views, host tensors, another device's tensors), the unusual but valid
buffers that must still give bit-exact values (data at odd storage offsets, int32-typed 2-D
data, digests as a row slice of a larger pool), and the C-ABI's own rejection (S3H_EINVAL) of a
digest pointer that misses the alignment include/s3hash.h states.

The misaligned-pointer tests assert the rejection and that nothing was written; they are not
about what a misaligned store would do.  References: tests/verify_shapes.py expected (hashlib,
zlib, table CRCs), never the library."""
import ctypes

import numpy as np
import pytest

import s3client_amd as s3
from s3client_amd import _native
from tests import launch_contract as lc
from tests import verify_shapes as vs

pytestmark = pytest.mark.gpu
ALGOS = ("sha256", "md5", "sha1", "crc32c", "crc64nvme")
N = vs.N_DEVICE
ROW = 4  # rows of sentinel before and after the digests inside a pool


@pytest.fixture(scope="module")
def batch(torch_cuda):
    return lc.vs_refs(N, 513)


def _plan(r, algo):
    if algo == "crc64nvme":
        return s3.Crc64Plan(r.offs, r.lens)
    if algo.startswith("crc"):
        return s3.CrcPlan(r.offs, r.lens, algo=algo)
    return s3.Plan(r.offs, r.lens, algo=algo)


def _status(plan):
    if hasattr(plan, "status"):
        plan.status()  # OK: a refused launch left no fault behind


def _pool(torch, words: int, rows: int = N + 2 * ROW):
    return torch.full((rows, words), lc.i32(lc.SENTINEL), dtype=torch.int32, device="cuda")


def _all_sentinel(t) -> bool:
    return bool((t.cpu().numpy().view(np.uint32) == lc.SENTINEL).all())


# ------------------------------------------------------------------ refused before any launch
@pytest.mark.parametrize("algo", ALGOS)
def test_rejects_strided_data(torch_cuda, batch, algo):
    """buf[::2] and a transposed 2-D tensor hold enough elements and are device tensors: the
    kernel would hash the storage's bytes, not the tensor's."""
    torch, r = torch_cuda, batch
    need = r.host.size
    flat = torch.zeros(2 * need, dtype=torch.uint8, device="cuda")
    side = 1 << int(np.ceil(np.log2(need) / 2))
    square = torch.zeros((side, side), dtype=torch.uint8, device="cuda")
    assert square.numel() >= need
    with _plan(r, algo) as plan:
        out = _pool(torch, vs.WORDS[algo])
        for data in (flat[::2], square.t()):
            assert data.is_cuda and data.numel() >= need and not data.is_contiguous()
            with pytest.raises(ValueError, match="data must be contiguous"):
                plan.launch(data, out)
        torch.cuda.synchronize()
        assert _all_sentinel(out)
        _status(plan)


@pytest.mark.parametrize("algo", ALGOS)
def test_rejects_column_slice_as_digests(torch_cuda, batch, algo):
    """pool[:, :words] of an (n, 2 * words) tensor: n * words elements, a device tensor, and
    rows that are not consecutive in memory."""
    torch, r = torch_cuda, batch
    words = vs.WORDS[algo]
    data = torch.from_numpy(r.host).cuda()
    pool = _pool(torch, 2 * words, N)
    view = pool[:, :words]
    assert view.numel() == N * words and not view.is_contiguous()
    with _plan(r, algo) as plan:
        with pytest.raises(ValueError, match="(digests|crcs) must be contiguous"):
            plan.launch(data, view)
        if algo in ("sha256", "md5", "sha1"):
            with pytest.raises(ValueError, match="digests must be contiguous"):
                plan.launch_range(data.data_ptr(), view, 0, 1, 0)
        else:
            with pytest.raises(ValueError, match="crcs must be contiguous"):
                plan.launch_range(data, view, 0, 64, 0)
        torch.cuda.synchronize()
        assert _all_sentinel(pool)
        _status(plan)


def test_rejects_misaligned_digest_tensor(torch_cuda, batch):
    """A contiguous view one word into a pool: 4-byte aligned, which SHA-1 and CRC-32 accept and
    SHA-256, MD5 (16) and CRC-64 (8) do not."""
    torch, r = torch_cuda, batch
    data = torch.from_numpy(r.host).cuda()
    for algo in ALGOS:
        words = vs.WORDS[algo]
        flat = _pool(torch, 1, (N + 2 * ROW) * words + 1).reshape(-1)
        view = flat[1:1 + N * words]
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        with _plan(r, algo) as plan:
            if algo in ("sha1", "crc32c"):
                plan.launch(data, view)
                _status(plan)
                torch.cuda.synchronize()
                got = view.cpu().numpy().view(np.uint32).reshape(N, words)
                assert lc.rows_differ(got, r.ref(algo)) == ""
                assert _all_sentinel(flat[:1]) and _all_sentinel(flat[1 + N * words:])
            else:
                with pytest.raises(ValueError, match="-byte aligned"):
                    plan.launch(data, view)
                torch.cuda.synchronize()
                assert _all_sentinel(flat)
                _status(plan)


@pytest.mark.parametrize("algo", ["sha256", "md5", "sha1"])
def test_stream_object_rejects_host_and_strided_tensors(torch_cuda, algo):
    """Stream.update_device and Stream.final_device tested nothing but sizes before."""
    torch = torch_cuda
    n = 130
    r = lc.ragged_refs(n, 131)
    words = vs.WORDS[algo]
    host_data = torch.from_numpy(r.host)
    data = host_data.cuda()
    out = _pool(torch, words, n + ROW)
    with s3.Stream(n, algo=algo) as st:
        with pytest.raises(ValueError, match="data must be a device tensor"):
            st.update_device(host_data, r.offs, r.lens)
        with pytest.raises(ValueError, match="data must be a device tensor"):
            st.update_device(r.host, r.offs, r.lens)
        with pytest.raises(ValueError, match="data must be contiguous"):
            st.update_device(torch.zeros(2 * r.host.size, dtype=torch.uint8, device="cuda")[::2], r.offs, r.lens)
        with pytest.raises(ValueError, match="digests must be a device tensor"):
            st.final_device(torch.zeros((n, words), dtype=torch.int32))
        with pytest.raises(ValueError, match="digests must be contiguous"):
            st.final_device(_pool(torch, 2 * words, n)[:, :words])
        assert all(st.total(i) == 0 for i in (0, 1, n - 1))  # no refused update was counted
        # the object still works: one update, one final, exact digests, nothing behind them
        st.update_device(data, r.offs, r.lens)
        st.final_device(out)
        st.status()
    got = out.cpu().numpy().view(np.uint32)
    assert lc.rows_differ(got[:n], r.ref(algo)) == ""
    assert (got[n:] == lc.SENTINEL).all()


def test_one_shots_reject_host_and_strided_data(torch_cuda, batch):
    torch, r = torch_cuda, batch
    host_t = torch.from_numpy(r.host)
    strided = torch.zeros(2 * r.host.size, dtype=torch.uint8, device="cuda")[::2]
    exp = torch.zeros((N, 8), dtype=torch.int32, device="cuda")
    calls = [lambda d: s3.sha256_batch_device(d, r.offs, r.lens),
             lambda d: s3.md5_batch_device(d, r.offs, r.lens),
             lambda d: s3.sha1_batch_device(d, r.offs, r.lens),
             lambda d: s3.sha256_md5_batch_device(d, r.offs, r.lens),
             lambda d: s3.crc_batch_device(d, r.offs, r.lens),
             lambda d: s3.crc64_batch_device(d, r.offs, r.lens),
             lambda d: s3.verify_batch_device(d, r.offs, r.lens, exp),
             lambda d: s3.crc_verify_batch_device(d, r.offs, r.lens, exp),
             lambda d: s3.crc64_verify_batch_device(d, r.offs, r.lens, exp),
             lambda d: s3.generate_parts(d, r.offs // 8 * 8, r.lens, np.arange(N), 1)]
    for call in calls:
        with pytest.raises(ValueError, match="data must be a device tensor"):
            call(host_t)
        with pytest.raises(ValueError, match="data must be contiguous"):
            call(strided)
    data = torch.from_numpy(r.host).cuda()
    with pytest.raises(ValueError, match="expected must be contiguous"):
        s3.verify_batch_device(data, r.offs, r.lens, torch.zeros((N, 16), dtype=torch.int32, device="cuda")[:, :8])
    with pytest.raises(ValueError, match="expected must be a device tensor"):
        s3.crc_verify_batch_device(data, r.offs, r.lens, torch.zeros(N, dtype=torch.int32))


def test_rejects_tensor_of_another_device(torch_cuda, batch):
    """Runs where there are two devices; tests/test_buffer_contract_cpu.py covers the check
    everywhere."""
    torch, r = torch_cuda, batch
    if torch.cuda.device_count() < 2:
        return
    data0 = torch.from_numpy(r.host).cuda()
    data1 = torch.from_numpy(r.host).to("cuda:1")
    out0 = _pool(torch, 8)
    with s3.Plan(r.offs, r.lens) as plan:
        with pytest.raises(ValueError, match="data is on device 1"):
            plan.launch(data1, out0)
        with pytest.raises(ValueError, match="digests is on device 1"):
            plan.launch(data0, out0.to("cuda:1"))
        torch.cuda.synchronize()
        assert _all_sentinel(out0)
        plan.status()


# ------------------------------------------------------------------ unusual but valid buffers
def _run_into_pool(torch, r, algo, data, base_ptr=None):
    """One launch into the row slice pool[ROW:ROW + n]; returns the digests, having checked the
    sentinel rows on both sides."""
    words = vs.WORDS[algo]
    pool = _pool(torch, words)
    view = pool[ROW:ROW + N]
    align = {"sha256": 16, "md5": 16, "sha1": 4, "crc32c": 4, "crc64nvme": 8}[algo]
    off = view.data_ptr() - pool.data_ptr()
    assert view.is_contiguous() and off == 4 * words * ROW and off % align == 0 and off % 256 != 0
    with _plan(r, algo) as plan:
        plan.launch(data, view)
        _status(plan)
    torch.cuda.synchronize()
    got = pool.cpu().numpy().view(np.uint32)
    assert (got[:ROW] == lc.SENTINEL).all() and (got[ROW + N:] == lc.SENTINEL).all()
    return got[ROW:ROW + N]


@pytest.mark.parametrize("shift", [1, 3, 13])
@pytest.mark.parametrize("algo", ALGOS)
def test_data_view_at_storage_offset(torch_cuda, batch, algo, shift):
    """The parts inside a larger tensor, the view beginning 1, 3 or 13 bytes into it; the digests
    go to a row slice of a larger pool whose offset is no multiple of 256."""
    torch, r = torch_cuda, batch
    big = torch.full((r.host.size + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    view = big[shift:shift + r.host.size]
    view.copy_(torch.from_numpy(r.host))
    assert view.data_ptr() - big.data_ptr() == shift and view.is_contiguous()
    assert lc.rows_differ(_run_into_pool(torch, r, algo, view), r.ref(algo)) == ""


@pytest.mark.parametrize("algo", ALGOS)
def test_data_typed_int32_and_2d(torch_cuda, batch, algo):
    """The same bytes as an (rows, 64) int32 tensor: element type and shape do not matter."""
    torch, r = torch_cuda, batch
    padded = np.zeros((r.host.size + 255) // 256 * 256, dtype=np.uint8)
    padded[:r.host.size] = r.host
    data = torch.from_numpy(padded.view(np.int32).reshape(-1, 64)).cuda()
    assert data.dim() == 2 and data.element_size() == 4 and data.is_contiguous()
    assert lc.rows_differ(_run_into_pool(torch, r, algo, data), r.ref(algo)) == ""


# ------------------------------------------------------------------ the C-ABI's own check
def _p(x: int):
    return ctypes.c_void_p(x)


def _expect_einval(rc: int):
    assert rc == _native.S3H_EINVAL, rc


def test_c_abi_rejects_misaligned_digest_pointer(torch_cuda, batch):
    """digests.data_ptr() + 4 straight through the C ABI (the Python validator would intercept
    first): S3H_EINVAL from every device entry point that stores 16-byte words, nothing written,
    nothing launched.  For the dual call only d_md5 is off."""
    torch, r = torch_cuda, batch
    L = _native.lib()
    data = torch.from_numpy(r.host).cuda()
    offs, lens = r.offs.ctypes.data_as(_native.u64p), r.lens.ctypes.data_as(_native.u64p)
    out = _pool(torch, 8)
    sha = _pool(torch, 8)
    torch.cuda.synchronize()
    bad, dptr = out.data_ptr() + 4, data.data_ptr()
    for algo in ("sha256", "md5"):
        with s3.Plan(r.offs, r.lens, algo=algo) as plan:
            _expect_einval(L.s3h_plan_launch(plan._h, _p(dptr), _p(bad), None))
            _expect_einval(L.s3h_plan_launch_range(plan._h, _p(dptr), _p(bad), 0, 1, 0, None))
            plan.status()
        with s3.Stream(N, algo=algo) as st:
            _expect_einval(L.s3h_stream_final_device(st._h, _p(bad), None))
            st.status()
    _expect_einval(L.s3h_sha256_batch_device(0, _p(dptr), offs, lens, N, _p(bad), None))
    _expect_einval(L.s3h_md5_batch_device(0, _p(dptr), offs, lens, N, _p(bad), None))
    _expect_einval(L.s3h_sha256_md5_batch_device(0, _p(dptr), offs, lens, N, _p(sha.data_ptr()), _p(bad), None))
    # 64-bit values: 8-byte aligned
    with s3.Crc64Plan(r.offs, r.lens) as plan:
        _expect_einval(L.s3h_crc64nvme_plan_launch(plan._h, _p(dptr), _p(bad), None))
        _expect_einval(L.s3h_crc64nvme_plan_launch_range(plan._h, _p(dptr), _p(bad), 0, 64, 0, None))
    _expect_einval(L.s3h_crc64nvme_batch_device(0, _p(dptr), offs, lens, N, _p(bad), None))
    torch.cuda.synchronize()
    assert _all_sentinel(out) and _all_sentinel(sha)
    # SHA-1 stays at 4 bytes: the same pointer is accepted and gives exact digests
    with s3.Plan(r.offs, r.lens, algo="sha1") as plan:
        assert L.s3h_plan_launch(plan._h, _p(dptr), _p(bad), None) == 0
        plan.status()
    got = out.cpu().numpy().view(np.uint32).reshape(-1)
    assert lc.rows_differ(got[1:1 + 5 * N].reshape(N, 5), r.ref("sha1")) == ""
    assert got[0] == lc.SENTINEL and (got[1 + 5 * N:] == lc.SENTINEL).all()
    # ... and 2 bytes off is refused for SHA-1 and the 32-bit values
    out2 = _pool(torch, 8)
    torch.cuda.synchronize()
    odd = out2.data_ptr() + 2
    with s3.Plan(r.offs, r.lens, algo="sha1") as plan:
        _expect_einval(L.s3h_plan_launch(plan._h, _p(dptr), _p(odd), None))
    _expect_einval(L.s3h_sha1_batch_device(0, _p(dptr), offs, lens, N, _p(odd), None))
    with s3.CrcPlan(r.offs, r.lens) as plan:
        _expect_einval(L.s3h_crc_plan_launch(plan._h, _p(dptr), _p(odd), None))
    torch.cuda.synchronize()
    assert _all_sentinel(out2)
