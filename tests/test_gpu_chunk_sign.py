"""SigV4 chunk-signed uploads on the device: chunk hashes through a SHA-256 plan over the chunks,
then the signature chains in sigv4_chunk_chain_kernel (s3h_chunk_plan_*,
s3h_chunk_sign_batch_device), and the host-resident entry point (s3h_chunk_sign_batch_host).

Expected signatures: hashlib + hmac from the definition (tests/chunk_sign_ref.py).  Bit-exact."""
import hashlib

import numpy as np
import pytest

import s3client_amd as s3
from tests import chunk_sign_ref as ref

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5AA5A5
MARGIN = 64  # sentinel words behind the signatures


def _batch(seed, lens, gap=3):
    lens = np.asarray(lens, dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens + np.uint64(gap))[:-1]]).astype(np.uint64)
    rng = np.random.default_rng(seed)
    host = rng.integers(0, 256, int(offs[-1] + lens[-1]) + 64, dtype=np.uint8)
    seeds = rng.integers(0, 2**32, (len(lens), 8), dtype=np.uint32)
    return {"offs": offs, "lens": lens, "host": host, "seeds": seeds}


def _parts(b):
    return [b["host"][int(o):int(o) + int(n)].tobytes() for o, n in zip(b["offs"], b["lens"])]


def _launch(torch, b, chunk_bytes, region="us-east-1", service="s3", seeds=None, plan=None):
    """One launch into the signatures followed by a sentinel margin: status OK, signatures equal
    to hmac's, margin untouched.  Returns (signatures, plan info)."""
    key = ref.signing_key(ref.SECRET, ref.DATE, region, service)
    seeds = b["seeds"] if seeds is None else seeds
    want = ref.signatures(key, region, service, seeds, _parts(b), chunk_bytes)
    data = torch.from_numpy(b["host"]).cuda()
    d_seeds = torch.from_numpy(seeds.view(np.int32)).cuda()
    own = plan is None
    plan = s3.ChunkSignPlan(b["offs"], b["lens"], chunk_bytes) if own else plan
    try:
        assert plan.signatures == len(want)
        out = torch.full((8 * plan.signatures + MARGIN,), SENTINEL, dtype=torch.int32, device="cuda")
        with s3.ChunkSignContext(key, ref.TIMESTAMP, ref.DATE, region, service) as ctx:
            plan.launch(data, ctx, d_seeds, out)
            plan.status()
        info = plan.info()
    finally:
        if own:
            plan.close()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[8 * len(want):] == SENTINEL).all(), "words behind the signatures were written"
    got = got[:8 * len(want)].reshape(-1, 8)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {len(want)} signatures differ, first rows {bad[:8].tolist()}"
    return got, info


def test_known_answer(torch_cuda):
    b = {"offs": np.array([0], dtype=np.uint64), "lens": np.array([66560], dtype=np.uint64),
         "host": np.full(66560, ord("a"), dtype=np.uint8),
         "seeds": np.frombuffer(bytes.fromhex(ref.KNOWN_SEED), dtype=np.uint32).reshape(1, 8).copy()}
    got, info = _launch(torch_cuda, b, 65536)
    assert tuple(r.tobytes().hex() for r in got) == ref.KNOWN_SIGNATURES
    assert info["n"] == 1 and info["data_chunks"] == 2 and info["signatures"] == 3
    assert info["max_chunks_per_part"] == 2


@pytest.mark.parametrize("r", ref.REMAINDERS)
def test_prefix_remainders(torch_cuda, r):
    # 70 parts: the second workgroup is partial; 0-11 data chunks, some parts empty, last chunks
    # of 1-64 bytes
    region, service = ref.names_for(r)
    lens = np.random.default_rng(r).integers(0, 701, 70)
    lens[:3] = [0, 64, 65]
    _, info = _launch(torch_cuda, _batch(300 + r, lens), 64, region, service)
    assert info["n"] == 70 and info["max_chunks_per_part"] == int(-(-lens.max() // 64))


@pytest.mark.parametrize("n", [1, 64, 65])
def test_part_counts(torch_cuda, n):
    # chunk size 100: chunks start at every alignment
    lens = np.random.default_rng(n).integers(0, 1200, n)
    _launch(torch_cuda, _batch(40 + n, lens), 100)


def test_mixed_chain_lengths(torch_cuda):
    # one chain of 300 data chunks beside 63 of one: lanes that finished idle beside a long one
    lens = [300 * 64] + [64] * 63
    _, info = _launch(torch_cuda, _batch(5, lens), 64)
    assert info["max_chunks_per_part"] == 300 and info["data_chunks"] == 363


def test_only_empty_parts(torch_cuda):
    _, info = _launch(torch_cuda, _batch(6, [0, 0, 0]), 64)
    assert info["data_chunks"] == 0 and info["signatures"] == 3 and info["kernel"] == "none"


def test_other_hash_kernel(torch_cuda):
    # 5,000 chunks: AUTO takes the chunk hashes to another kernel than the small batches' skew
    lens = np.full(50, 100 * 64)
    _, info = _launch(torch_cuda, _batch(8, lens), 64)
    assert info["data_chunks"] == 5000
    assert info["kernel"] in ("skewp", "skews"), info
    small = s3.ChunkSignPlan([0], [640], 64)
    assert small.info()["kernel"] == "skew"
    small.close()


def test_one_shot_and_relaunch(torch_cuda):
    lens = np.random.default_rng(9).integers(0, 3000, 33)
    b = _batch(10, lens)
    key = ref.signing_key(ref.SECRET, ref.DATE, "us-east-1", "s3")
    other = np.random.default_rng(11).integers(0, 2**32, b["seeds"].shape, dtype=np.uint32)
    with s3.ChunkSignPlan(b["offs"], b["lens"], 256) as plan:
        first, _ = _launch(torch_cuda, b, 256, plan=plan)
        second, _ = _launch(torch_cuda, b, 256, seeds=other, plan=plan)  # its own chain
        again, _ = _launch(torch_cuda, b, 256, plan=plan)
    assert not np.array_equal(first, second) and np.array_equal(first, again)
    data = torch_cuda.from_numpy(b["host"]).cuda()
    with s3.ChunkSignContext(key, ref.TIMESTAMP, ref.DATE, "us-east-1", "s3") as ctx:
        shot = s3.chunk_sign_batch_device(data, b["offs"], b["lens"], 256, ctx, b["seeds"])
    assert np.array_equal(shot, first)


def test_chain_alone(torch_cuda):
    # the chain kernel over digests the caller hashed with an ordinary plan over the chunks
    lens = np.random.default_rng(14).integers(0, 2000, 20)
    b = _batch(15, lens)
    key = ref.signing_key(ref.SECRET, ref.DATE, "us-east-1", "s3")
    want = ref.signatures(key, "us-east-1", "s3", b["seeds"], _parts(b), 128)
    co = [int(o) + at for o, n in zip(b["offs"], b["lens"]) for at in range(0, int(n), 128)]
    cl = [min(128, int(n) - at) for n in b["lens"] for at in range(0, int(n), 128)]
    data = torch_cuda.from_numpy(b["host"]).cuda()
    digs = s3.sha256_batch_device(data, co, cl)
    d_seeds = torch_cuda.from_numpy(b["seeds"].view(np.int32)).cuda()
    with s3.ChunkSignPlan(b["offs"], b["lens"], 128) as plan, \
            s3.ChunkSignContext(key, ref.TIMESTAMP, ref.DATE, "us-east-1", "s3") as ctx:
        out = torch_cuda.full((8 * plan.signatures + MARGIN,), SENTINEL, dtype=torch_cuda.int32, device="cuda")
        plan.chain(ctx, digs, d_seeds, out)
        plan.status()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[8 * len(want):] == SENTINEL).all()
    assert np.array_equal(got[:8 * len(want)].reshape(-1, 8), want)


def test_launch_arguments(torch_cuda):
    b = _batch(12, [100, 200])
    data = torch_cuda.from_numpy(b["host"]).cuda()
    seeds = torch_cuda.zeros(16, dtype=torch_cuda.int32, device="cuda")
    with s3.ChunkSignPlan(b["offs"], b["lens"], 64) as plan, \
            s3.ChunkSignContext(bytes(32), ref.TIMESTAMP, ref.DATE, "us-east-1", "s3") as ctx:
        out = torch_cuda.zeros(8 * plan.signatures, dtype=torch_cuda.int32, device="cuda")
        with pytest.raises(ValueError):
            plan.launch(data, ctx, seeds, out[8:])  # too small
        with pytest.raises(s3.S3HashError):
            plan.launch(data, ctx, seeds, out.data_ptr() + 4)  # not 16-byte aligned
        plan.status()


def test_host_entry(torch_cuda):
    rng = np.random.default_rng(13)
    lens = rng.integers(0, 5001, 40)
    lens[:2] = [0, 1024]
    parts = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in lens]
    seeds = rng.integers(0, 2**32, (40, 8), dtype=np.uint32)
    key = ref.signing_key(ref.SECRET, ref.DATE, "us-east-1", "s3")
    counts = [len(ref.cut(p.tobytes(), 1024)) for p in parts]
    digs = b"".join(hashlib.sha256(c).digest() for p in parts for c in ref.cut(p.tobytes(), 1024))
    with s3.ChunkSignContext(key, ref.TIMESTAMP, ref.DATE, "us-east-1", "s3") as ctx:
        got = s3.chunk_sign_host(parts, 1024, ctx, seeds)
        want = s3.cpu_chunk_signatures(ctx, digs, counts, seeds)
    assert np.array_equal(got, want)
    assert np.array_equal(got, ref.signatures(key, "us-east-1", "s3", seeds, [p.tobytes() for p in parts], 1024))
