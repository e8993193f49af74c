"""Stream order of every asynchronous launch of the library, and of the blocking device calls'
use of the caller's stream: each launch sits in a "sandwich" on a fresh side stream S
(tests/launch_contract.py Sandwich) -- a delay launch, a producer copy that fills the parts, the
launch under test, a consumer that snapshots and overwrites the outputs -- with no host
synchronisation until the end.  Torch's side streams do not block on the null stream, so a
kernel, memset or copy that the library put on another stream than S reads the poison the data
held before, or writes behind the consumer, and the snapshot differs from the reference.

Scheduling can hide such an ordering bug -- the stray work may happen to run late enough -- but
it can never invent one: a failure here is a real defect in launch.hip or in the launch path of
the entry point.

References: hashlib, zlib and the table CRCs (tests/verify_shapes.py expected), hashlib + hmac
(tests/chunk_sign_ref.py, tests/chunk_trailer_ref.py); nothing is computed by the library."""
import numpy as np
import pytest

import s3client_amd as s3
from tests import chunk_sign_ref as ref
from tests import chunk_trailer_ref as tref
from tests import launch_contract as lc
from tests import verify_shapes as vs

pytestmark = pytest.mark.gpu


def _cus(torch) -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _launch_on(torch, S, via_current: bool, fn):
    """fn(stream) with stream=S, or with stream=None under `with torch.cuda.stream(S)`."""
    if via_current:
        with torch.cuda.stream(S):
            return fn(None)
    return fn(S)


def _plan_case(torch, r: lc.Refs, algo: str, kernel="auto", via_current=False, check_plan=None):
    """One whole-batch plan launch inside the sandwich; returns nothing, asserts bit-exactness."""
    words = vs.WORDS[algo]
    with s3.Plan(r.offs, r.lens, kernel=kernel, algo=algo) as plan:
        if check_plan is not None:
            check_plan(plan.info())
        sw = lc.Sandwich(torch, r.host)
        out = sw.output(words * r.n)
        S = sw.open()
        _launch_on(torch, S, via_current, lambda st: plan.launch(sw.data, out, stream=st))
        got, = sw.close(plan)
    assert lc.rows_differ(got.reshape(r.n, words), r.ref(algo)) == ""


# ------------------------------------------------------------------ s3h_plan_launch
@pytest.mark.parametrize("kernel, via_current",
                         [(k, False) for k in ("lane", "pc", "pair", "quad", "skew", "skewp", "skews")]
                         + [("skew", True)])
def test_plan_launch_sha256_each_kernel(torch_cuda, kernel, via_current):
    """Each forced SHA-256 kernel at 513 parts; `skew` also through the current stream."""
    r = lc.vs_refs(vs.N_DEVICE, 513)

    def is_kernel(info):
        assert info["kernel"] == kernel

    _plan_case(torch_cuda, r, "sha256", kernel, via_current, is_kernel)


def test_plan_launch_sha256_two_group_skew(torch_cuda):
    """3,000 parts: the skew plan runs two flag-synchronised groups per workgroup."""
    n = 3000
    with s3.Plan([0] * n, [1] * n, kernel="skew") as eq:
        assert eq.info()["grid"] == (n + 15) // 16
    r = lc.ragged_refs(n, 3000)

    def two_groups(info):
        assert info["kernel"] == "skew" and info["groups"] == (n + 7) // 8

    _plan_case(torch_cuda, r, "sha256", "skew", False, two_groups)


@pytest.mark.parametrize("form", ["grid<=CUs", "grid>CUs"])
@pytest.mark.parametrize("algo", ["md5", "sha1"])
def test_plan_launch_md5_sha1_both_forms(torch_cuda, algo, form):
    """md5_pc_kernel / sha1_pc_kernel: the one-workgroup-per-CU form (513 parts, grid 9) and the
    several-per-CU form (one part more than 64 x CUs, 0-64 B each)."""
    cus = _cus(torch_cuda)
    if form == "grid<=CUs":
        r = lc.vs_refs(vs.N_DEVICE, 513)
        want_grid = (vs.N_DEVICE + 63) // 64
        assert want_grid <= cus
    else:
        r = lc.ragged_refs(64 * cus + 1, 64, hi=64)
        want_grid = cus + 1

    def grid(info):
        assert info["kernel"] == "pc" and info["grid"] == want_grid

    _plan_case(torch_cuda, r, algo, "auto", False, grid)


def test_plan_launch_md5_current_stream(torch_cuda):
    _plan_case(torch_cuda, lc.vs_refs(vs.N_DEVICE, 513), "md5", "auto", True)


# ------------------------------------------------------------------ s3h_plan_launch_range
def _prime_ranged(torch, plan, r):
    """A first ranged launch on the default stream, waited for: the plan allocates its chaining
    state there and not in the middle of the sandwich."""
    tmp = torch.zeros(r.host.size, dtype=torch.uint8, device="cuda")
    out = torch.zeros((r.n, 8), dtype=torch.int32, device="cuda")
    plan.launch_range(tmp.data_ptr(), out, 0, 1, 0)
    plan.status()


def _ranged(plan, data, out, max_blocks, stream):
    plan.launch_range(data.data_ptr(), out, 0, 2, 0, stream=stream)
    plan.launch_range(data.data_ptr(), out, 2, max_blocks, 0, stream=stream)


@pytest.mark.parametrize("algo, kernel, via_current",
                         [("sha256", "skew", False), ("sha256", "skewp", False), ("md5", "auto", False),
                          ("sha256", "skew", True)])
def test_plan_launch_range_state_in_stream_order(torch_cuda, algo, kernel, via_current):
    """Blocks [0, 2) then [2, max_blocks) back to back on S: the chaining state the first launch
    leaves in the plan is read by the second in stream order."""
    torch = torch_cuda
    r = lc.vs_refs(vs.N_DEVICE, 513)
    words = vs.WORDS[algo]
    with s3.Plan(r.offs, r.lens, kernel=kernel, algo=algo) as plan:
        mb = plan.info()["max_blocks"]
        assert mb == 4  # the 200-byte part: two launches of two blocks
        _prime_ranged(torch, plan, r)
        sw = lc.Sandwich(torch, r.host)
        out = sw.output(words * r.n)
        S = sw.open()
        _launch_on(torch, S, via_current, lambda st: _ranged(plan, sw.data, out, mb, st))
        got, = sw.close(plan)
    assert lc.rows_differ(got.reshape(r.n, words), r.ref(algo)) == ""


# ------------------------------------------------------------------ blocking device calls on S
def _blocking(torch, r: lc.Refs, call, via_current=False):
    """Delay and producer on S, then a blocking call given S (or None with S current): returns
    what the call returned."""
    sw = lc.Sandwich(torch, r.host)
    S = sw.open()
    res = _launch_on(torch, S, via_current, lambda st: call(sw.data, st))
    sw.close()
    return res


def _u32(t, shape):
    return t.cpu().numpy().view(np.uint32).reshape(shape)


# (parts, shortest part, form).  With 0-300 B parts a 2,500-part batch has skew groups of its own
# (the mixed grid: its longest parts have 5 blocks, most have fewer), so the plain group kernel is
# reached with 248-300 B parts, which all have 5 blocks.
DUAL_FORMS = [(300, 0, "split"), (2000, 0, "group-skew"), (2500, 248, "group"), (2500, 0, "mixed"),
              (9000, 0, "two-kernels")]


@pytest.mark.parametrize("n, lo, form", DUAL_FORMS, ids=[f for _, _, f in DUAL_FORMS])
def test_dual_digest_device_on_stream(torch_cuda, n, lo, form):
    """sha256_md5_batch_device(stream=S): the one-grid forms and the two-kernel fallback (0-300 B
    parts; counts of test_dual_digest_device_fallback_and_fused_ragged).  The form follows from
    the plan (plan.cpp dual_mode): its kernel, grid and skew groups are asserted."""
    cus = _cus(torch_cuda)
    r = lc.ragged_refs(n, 7000 + n, lo=lo)
    with s3.Plan(r.offs, r.lens) as p:
        info = p.info()
    assert (info["dual_solo"] > 0) == (form == "mixed")
    if form in ("split", "group-skew"):
        assert info["kernel"] == "skew" and info["grid"] == (n + 7) // 8 <= cus
        # the split grid adds its MD5 workgroups (kernel_abi.hpp split_md5_wgs: one per 64
        # parts); the cases keep the same side of the limit with that count rounded up to 8s
        for md5_wgs in (8 * ((info["grid"] + 63) // 64), (n + 63) // 64):
            assert (info["grid"] + md5_wgs <= cus) == (form == "split")
    elif form == "two-kernels":
        assert (n + 31) // 32 > cus
    else:
        assert n > 2048 and (n + 31) // 32 <= cus
    sha, m5 = _blocking(torch_cuda, r, lambda d, S: s3.sha256_md5_batch_device(d, r.offs, r.lens, stream=S))
    assert lc.rows_differ(_u32(sha, (n, 8)), r.ref("sha256")) == ""
    assert lc.rows_differ(_u32(m5, (n, 4)), r.ref("md5")) == ""


@pytest.mark.parametrize("via_current", [False, True], ids=["stream=S", "current"])
def test_dual_digest_mixed_grid_on_stream(torch_cuda, via_current):
    """The fourth one-grid form: 2,100 ragged parts of 80-1,024 B have skew groups of their own
    (dual_solo > 0: test_dual_mixed_grid_ragged scaled down by 64)."""
    torch = torch_cuda
    n = 2100
    rng = np.random.default_rng(n)
    lens = (80 + rng.integers(0, 945, n)).astype(np.uint64)
    lens[:5] = [1024, 1023, 80, 135, 1024]
    offs = np.concatenate([[0], np.cumsum(lens + np.uint64(7))[:-1]]).astype(np.uint64)
    host = rng.integers(0, 256, int(offs[-1] + lens[-1]) + 64, dtype=np.uint8)
    r = lc.Refs(host, offs, lens)
    solo, apart = s3.dual_layout(lens, _cus(torch))
    assert solo > 0 and 8 * solo < n
    with s3.Plan(offs, lens) as p:
        info = p.info()
        assert (info["dual_solo"], info["dual_apart"]) == (solo, apart)

    sha, m5 = _blocking(torch, r, lambda d, S: s3.sha256_md5_batch_device(d, offs, lens, stream=S), via_current)
    assert lc.rows_differ(_u32(sha, (n, 8)), r.ref("sha256")) == ""
    assert lc.rows_differ(_u32(m5, (n, 4)), r.ref("md5")) == ""


@pytest.mark.parametrize("via_current", [False, True], ids=["stream=S", "current"])
@pytest.mark.parametrize("algo", ["sha1", "md5", "crc32c", "crc32", "crc64nvme"])
def test_one_shot_batch_device_on_stream(torch_cuda, algo, via_current):
    """sha1_ / md5_ / crc_ / crc64_batch_device(stream=S), and with S as the current stream."""
    r = lc.vs_refs(vs.N_DEVICE, 513)
    call = {"sha1": lambda d, S: s3.sha1_batch_device(d, r.offs, r.lens, stream=S),
            "md5": lambda d, S: s3.md5_batch_device(d, r.offs, r.lens, stream=S),
            "crc32c": lambda d, S: s3.crc_batch_device(d, r.offs, r.lens, "crc32c", stream=S),
            "crc32": lambda d, S: s3.crc_batch_device(d, r.offs, r.lens, "crc32", stream=S),
            "crc64nvme": lambda d, S: s3.crc64_batch_device(d, r.offs, r.lens, stream=S)}[algo]
    got = _blocking(torch_cuda, r, call, via_current)
    assert lc.rows_differ(_u32(got, (r.n, vs.WORDS[algo])), r.ref(algo)) == ""


@pytest.mark.parametrize("algo, via_current", [(a, False) for a in vs.ALGOS]
                         + [("sha256", True), ("crc32c", True), ("crc64nvme", True)])
def test_verify_batch_device_on_stream(torch_cuda, algo, via_current):
    """verify_ / crc_verify_ / crc64_verify_batch_device(stream=S) against the reference of the
    good bytes: no row is flagged; read too early, every non-empty row would be.  Then one
    expected word is corrupted by a torch op on S and exactly that row is flagged."""
    torch = torch_cuda
    r = lc.vs_refs(vs.N_DEVICE, 513)
    exp = torch.from_numpy(r.ref(algo).view(np.int32).copy()).cuda()
    verify = {"crc64nvme": lambda d, S: s3.crc64_verify_batch_device(d, r.offs, r.lens, exp, stream=S),
              "crc32c": lambda d, S: s3.crc_verify_batch_device(d, r.offs, r.lens, exp, "crc32c", stream=S),
              "crc32": lambda d, S: s3.crc_verify_batch_device(d, r.offs, r.lens, exp, "crc32", stream=S)
              }.get(algo, lambda d, S: s3.verify_batch_device(d, r.offs, r.lens, exp, algo, stream=S))
    sw = lc.Sandwich(torch, r.host)
    S = sw.open()
    cnt, mask = _launch_on(torch, S, via_current, lambda st: verify(sw.data, st))
    assert cnt == 0 and not mask.any().item()
    row, word = 256, vs.WORDS[algo] - 1
    with torch.cuda.stream(S):
        exp[row, word] ^= lc.i32(1 << vs.bit(row, word))
    cnt, mask = _launch_on(torch, S, via_current, lambda st: verify(sw.data, st))
    assert cnt == 1 and torch.nonzero(mask).flatten().tolist() == [row]
    sw.close()


# ------------------------------------------------------------------ CRC plans
SEGMENT = 16384  # the segment size of a batch of fewer than 8,192 segments (crc.cpp)


@pytest.fixture(scope="module")
def crc_batch(torch_cuda):
    """513 small parts and one of 3 segments + 17 B, so that both kernels of a launch matter."""
    host, offs, lens = vs.batch(vs.N_DEVICE, 515)
    long_len = 3 * SEGMENT + 17
    big = np.random.default_rng(6).integers(0, 256, long_len + vs.TAIL, dtype=np.uint8)
    offs = np.concatenate([offs, [host.size]]).astype(np.uint64)
    lens = np.concatenate([lens, [long_len]]).astype(np.uint64)
    return lc.Refs(np.concatenate([host, big]), offs, lens), SEGMENT


CRC_CASES = [("crc32c", False), ("crc32", False), ("crc64nvme", False)]


@pytest.mark.parametrize("algo, via_current", CRC_CASES + [("crc32c", True)])
def test_crc_plan_launch(torch_cuda, crc_batch, algo, via_current):
    """CrcPlan.launch: the segment kernel, then the parts kernel, through plan-owned partials."""
    torch = torch_cuda
    r, seg = crc_batch
    words = vs.WORDS[algo]
    plan = s3.Crc64Plan(r.offs, r.lens) if algo == "crc64nvme" else s3.CrcPlan(r.offs, r.lens, algo=algo)
    with plan:
        info = plan.info()
        assert info["segment_bytes"] == seg and info["segments"] >= 4
        sw = lc.Sandwich(torch, r.host)
        out = sw.output(words * r.n)
        S = sw.open()
        _launch_on(torch, S, via_current, lambda st: plan.launch(sw.data, out, stream=st))
        got, = sw.close()
    assert lc.rows_differ(got.reshape(r.n, words), r.ref(algo)) == ""


@pytest.mark.parametrize("algo, via_current", CRC_CASES + [("crc64nvme", True)])
def test_crc_plan_launch_range(torch_cuda, crc_batch, algo, via_current):
    """CrcPlan.launch_range: bytes [0, cut) then [cut, longest) on S, the cut inside the long
    part's second segment; the running values stay in the plan between the two launches."""
    torch = torch_cuda
    r, seg = crc_batch
    words = vs.WORDS[algo]
    longest = int(r.lens.max())
    cut = seg + 100
    plan = s3.Crc64Plan(r.offs, r.lens) if algo == "crc64nvme" else s3.CrcPlan(r.offs, r.lens, algo=algo)

    def two(st):
        plan.launch_range(sw.data, out, 0, cut, 0, stream=st)
        plan.launch_range(sw.data, out, cut, longest, 0, stream=st)

    with plan:
        sw = lc.Sandwich(torch, r.host)
        out = sw.output(words * r.n)
        S = sw.open()
        _launch_on(torch, S, via_current, two)
        got, = sw.close()
    assert lc.rows_differ(got.reshape(r.n, words), r.ref(algo)) == ""


# ------------------------------------------------------------------ chunk-signing plans
REGION, SERVICE = "us-east-1", "s3"
KEY = ref.signing_key(ref.SECRET, ref.DATE, REGION, SERVICE)


def _chunk_host(seed: int):
    """70 parts of 0-700 B at 3-byte gaps (chunk size 64: 0-11 data chunks), and their seeds."""
    lens = np.random.default_rng(70).integers(0, 701, 70).astype(np.uint64)
    lens[:3] = [0, 64, 65]
    offs = np.concatenate([[0], np.cumsum(lens + np.uint64(3))[:-1]]).astype(np.uint64)
    rng = np.random.default_rng(seed)
    host = rng.integers(0, 256, int(offs[-1] + lens[-1]) + 64, dtype=np.uint8)
    seeds = rng.integers(0, 2**32, (70, 8), dtype=np.uint32)
    return host, offs, lens, seeds


class ChunkBatch:
    def __init__(self, seed: int):
        self.host, self.offs, self.lens, self.seeds = _chunk_host(seed)
        self.n = 70
        self.parts = vs.parts_of(self.host, self.offs, self.lens)
        self._want = {}

    def want(self, kind: str):
        """(signatures, checksums, trailer signatures) of the good bytes for a trailer kind."""
        if kind not in self._want:
            self._want[kind] = tref.expected(KEY, REGION, SERVICE, self.seeds, self.parts, 64, kind)
        return self._want[kind]


@pytest.fixture(scope="module")
def chunks(torch_cuda):
    return ChunkBatch(370), ChunkBatch(371)


def _ctx():
    return s3.ChunkSignContext(KEY, ref.TIMESTAMP, ref.DATE, REGION, SERVICE)


def _vwords(kind):
    return 2 if kind == "crc64nvme" else 1


def _check_trailer(got, want, kind, n):
    sigs, vals, tsig = got
    assert lc.rows_differ(sigs.reshape(-1, 8), want[0]) == "", "signatures"
    assert lc.rows_differ(vals.reshape(n, _vwords(kind)),
                          want[1].view(np.uint32).reshape(n, _vwords(kind))) == "", "checksums"
    assert lc.rows_differ(tsig.reshape(n, 8), want[2]) == "", "trailer signatures"


@pytest.mark.parametrize("via_current", [False, True], ids=["stream=S", "current"])
def test_chunk_plan_launch(torch_cuda, chunks, via_current):
    """ChunkSignPlan.launch: the chunk hash plan into plan-owned digests, then the chain kernel."""
    torch, b = torch_cuda, chunks[0]
    seeds = torch.from_numpy(b.seeds.view(np.int32)).cuda()
    with s3.ChunkSignPlan(b.offs, b.lens, 64) as plan, _ctx() as ctx:
        sw = lc.Sandwich(torch, b.host)
        out = sw.output(8 * plan.signatures)
        S = sw.open()
        _launch_on(torch, S, via_current, lambda st: plan.launch(sw.data, ctx, seeds, out, stream=st))
        got, = sw.close(plan)
    assert lc.rows_differ(got.reshape(-1, 8), b.want("crc32c")[0]) == ""


@pytest.mark.parametrize("via_current", [False, True], ids=["stream=S", "current"])
def test_chunk_plan_chain(torch_cuda, chunks, via_current):
    """ChunkSignPlan.chain over chunk digests that a copy on S delivers."""
    torch, b = torch_cuda, chunks[0]
    digs = lc.sha256_words([c for p in b.parts for c in ref.cut(p, 64)])
    seeds = torch.from_numpy(b.seeds.view(np.int32)).cuda()
    with s3.ChunkSignPlan(b.offs, b.lens, 64) as plan, _ctx() as ctx:
        assert len(digs) == int(plan.data_chunks_per_part.sum())
        sw = lc.Sandwich(torch, digs.view(np.int32))
        out = sw.output(8 * plan.signatures)
        S = sw.open()
        _launch_on(torch, S, via_current, lambda st: plan.chain(ctx, sw.data, seeds, out, stream=st))
        got, = sw.close(plan)
    assert lc.rows_differ(got.reshape(-1, 8), b.want("crc32c")[0]) == ""


TRAILER_CASES = [("crc32c", False), ("crc64nvme", False), ("crc64nvme", True)]


@pytest.mark.parametrize("kind, via_current", TRAILER_CASES)
def test_chunk_plan_launch_trailer(torch_cuda, chunks, kind, via_current):
    """launch_trailer: chunk hash plan, chain, CRC plan (two kernels), trailer kernel -- all on S."""
    torch, b = torch_cuda, chunks[0]
    seeds = torch.from_numpy(b.seeds.view(np.int32)).cuda()
    with s3.ChunkSignPlan(b.offs, b.lens, 64, trailer=kind) as plan, _ctx() as ctx:
        sw = lc.Sandwich(torch, b.host)
        outs = [sw.output(w) for w in (8 * plan.signatures, _vwords(kind) * b.n, 8 * b.n)]
        S = sw.open()
        _launch_on(torch, S, via_current,
                   lambda st: plan.launch_trailer(sw.data, ctx, seeds, *outs, stream=st))
        got = sw.close(plan)
    _check_trailer(got, b.want(kind), kind, b.n)


@pytest.mark.parametrize("kind, via_current", TRAILER_CASES)
def test_chunk_plan_trailer_alone(torch_cuda, chunks, kind, via_current):
    """ChunkSignPlan.trailer over signatures that a copy on S delivers."""
    torch, b = torch_cuda, chunks[0]
    sigs, vals, tsig = b.want(kind)
    checks = torch.from_numpy(np.ascontiguousarray(vals).view(np.int32).copy()).cuda()
    with s3.ChunkSignPlan(b.offs, b.lens, 64, trailer=kind) as plan, _ctx() as ctx:
        sw = lc.Sandwich(torch, np.ascontiguousarray(sigs).view(np.int32))
        out = sw.output(8 * b.n)
        S = sw.open()
        _launch_on(torch, S, via_current, lambda st: plan.trailer(ctx, sw.data, checks, out, stream=st))
        got, = sw.close(plan)
    assert lc.rows_differ(got.reshape(b.n, 8), tsig) == ""


# ------------------------------------------------------------------ multi-object streams
@pytest.mark.parametrize("algo, via_current", [("sha256", False), ("md5", False), ("sha1", False), ("sha256", True)])
def test_stream_updates_and_final_on_stream(torch_cuda, algo, via_current):
    """Stream.update_device twice, then final_device, all on S: 130 messages of two ragged chunks
    (carries of every size); the digests are those of each message's two chunks joined."""
    torch = torch_cuda
    n = 130
    r1, r2 = lc.ragged_refs(n, 131), lc.ragged_refs(n, 132)
    host = np.concatenate([r1.host, r2.host])
    offs2 = r2.offs + np.uint64(r1.host.size)
    msgs = [a + b for a, b in zip(vs.parts_of(r1.host, r1.offs, r1.lens), vs.parts_of(r2.host, r2.offs, r2.lens))]
    want = vs.expected(algo, msgs)
    words = vs.WORDS[algo]
    with s3.Stream(n, algo=algo) as st:
        sw = lc.Sandwich(torch, host)
        out = sw.output(words * n)
        S = sw.open()
        def run(on):
            st.update_device(sw.data, r1.offs, r1.lens, stream=on)
            st.update_device(sw.data, offs2, r2.lens, stream=on)
            st.final_device(out, stream=on)

        _launch_on(torch, S, via_current, run)
        got, = sw.close(st)
    assert lc.rows_differ(got.reshape(n, words), want) == ""


# ------------------------------------------------------------------ generator
@pytest.mark.parametrize("via_current", [False, True], ids=["stream=S", "current"])
def test_generate_parts_then_plan_on_stream(torch_cuda, oracle, via_current):
    """generate_parts(stream=S) fills the parts behind the delay launch, a plan launch on S
    hashes them: the digests are those of the oracle's generator output."""
    torch = torch_cuda
    n, seed = 257, 11
    lens = np.random.default_rng(9).integers(0, 301, n).astype(np.uint64)
    lens[:2] = [0, 300]
    offs = np.concatenate([[0], np.cumsum((lens + np.uint64(15)) // np.uint64(8) * np.uint64(8))[:-1]]).astype(np.uint64)
    ids = np.arange(n, dtype=np.uint64) + np.uint64(1000)
    total = int(offs[-1] + lens[-1]) + 64
    want = lc.sha256_words([oracle.generate(int(p), int(L), seed) for p, L in zip(ids, lens)])
    with s3.Plan(offs, lens) as plan:
        sw = lc.Sandwich(torch, np.zeros(total, dtype=np.uint8))  # `data` starts as 0xFF bytes
        out = sw.output(8 * n)
        S = sw.open(produce=False)
        def run(on):
            s3.generate_parts(sw.data, offs, lens, ids, seed, stream=on)
            plan.launch(sw.data, out, stream=on)

        _launch_on(torch, S, via_current, run)
        got, = sw.close(plan)
    assert lc.rows_differ(got.reshape(n, 8), want) == ""


# ------------------------------------------------------------------ plan-owned scratch, no host sync
def _other_bytes(host: np.ndarray) -> np.ndarray:
    """Buffer B: the same layout, other bytes."""
    return np.random.default_rng(host.size).integers(0, 256, host.size, dtype=np.uint8)


def _aba(torch, host_a, host_b, words, launch, *plans):
    """launch(data, out, S) on buffer A, on buffer B, on A again, all on S behind the delay
    launch with no synchronisation or status() in between: the three outputs' payloads."""
    sw = lc.Sandwich(torch, host_a)
    d_b = torch.from_numpy(host_b).cuda()
    outs = [[sw.output(w) for w in words] for _ in range(3)]
    S = sw.open()
    for data, o in zip((sw.data, d_b, sw.data), outs):
        launch(data, o, S)
    got = sw.close(*plans)
    k = len(words)
    return [got[i * k:(i + 1) * k] for i in range(3)]


def test_scratch_reuse_sha256_ranged_plan(torch_cuda):
    """d_state of a ranged SHA-256 plan, reused by three passes of two ranges each."""
    ra = lc.vs_refs(vs.N_DEVICE, 513)
    rb = lc.Refs(_other_bytes(ra.host), ra.offs, ra.lens)
    with s3.Plan(ra.offs, ra.lens, kernel="skew") as plan:
        mb = plan.info()["max_blocks"]
        _prime_ranged(torch_cuda, plan, ra)
        got = _aba(torch_cuda, ra.host, rb.host, [8 * ra.n],
                   lambda d, o, S: _ranged(plan, d, o[0], mb, S), plan)
    for (g,), r in zip(got, (ra, rb, ra)):
        assert lc.rows_differ(g.reshape(r.n, 8), r.ref("sha256")) == ""


def test_scratch_reuse_crc64_plan(torch_cuda, crc_batch):
    """d_partials of a CRC-64/NVME plan (segment values of the long part), three launches."""
    ra, _ = crc_batch
    rb = lc.Refs(_other_bytes(ra.host), ra.offs, ra.lens)
    with s3.Crc64Plan(ra.offs, ra.lens) as plan:
        got = _aba(torch_cuda, ra.host, rb.host, [2 * ra.n],
                   lambda d, o, S: plan.launch(d, o[0], stream=S))
    for (g,), r in zip(got, (ra, rb, ra)):
        assert lc.rows_differ(g.reshape(r.n, 2), r.ref("crc64nvme")) == ""


def test_scratch_reuse_trailer_plan(torch_cuda, chunks):
    """A trailer plan's chunk digests, CRC partials and error word, three launches."""
    torch = torch_cuda
    a, b = chunks
    kind = "crc32c"
    seeds_a = torch.from_numpy(a.seeds.view(np.int32)).cuda()
    seeds_b = torch.from_numpy(b.seeds.view(np.int32)).cuda()
    with s3.ChunkSignPlan(a.offs, a.lens, 64, trailer=kind) as plan, _ctx() as ctx:
        words = [8 * plan.signatures, a.n, 8 * a.n]
        seq = iter((seeds_a, seeds_b, seeds_a))
        got = _aba(torch, a.host, b.host, words,
                   lambda d, o, S: plan.launch_trailer(d, ctx, next(seq), *o, stream=S), plan)
    for g, x in zip(got, (a, b, a)):
        _check_trailer(g, x.want(kind), kind, x.n)
