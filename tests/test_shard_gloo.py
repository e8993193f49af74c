"""Multi-rank sharding on CPU with the gloo backend, world_size 2.

Each rank takes parts p % world == rank, digests them locally (CPU drop-in here; the GPU
path on the box), and the digest table is reassembled only for verification.  Checks: the
shards partition the batch, the reassembled table equals the oracle's, and bench.py's
workload() uses the same partition."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from s3client_amd.shard import gather_digests, pack_offsets, shard_ids


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, n_total, lens, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import s3client_amd as s3
    from tests.oracle_lib import Oracle
    orc = Oracle()
    ids = shard_ids(n_total, rank, world)
    local = np.stack([s3.sha256(orc.generate(int(p), int(lens[int(p)]))) for p in ids])
    t = __import__("torch").tensor([float(rank + 1)])
    dist.all_reduce(t, op=dist.ReduceOp.MAX)          # bench.py's max-over-ranks timing
    full = gather_digests(local, ids, n_total)
    if rank == 0:
        q.put((full, float(t)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_round_robin_shards_reassemble_to_oracle(oracle, world):
    n_total = 37
    lens = np.random.default_rng(world).integers(0, 3000, n_total)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_total, lens, q))
             for r in range(world)]
    for p in procs:
        p.start()
    full, tmax = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert tmax == float(world)
    want = np.stack([oracle.sha256(oracle.generate(p, int(lens[p]))) for p in range(n_total)])
    assert np.array_equal(full, want)


def test_shards_partition_and_bench_workload_matches():
    import bench
    for world in (1, 2, 4, 8):
        allids = np.concatenate([shard_ids(1000, r, world) for r in range(world)])
        assert sorted(allids.tolist()) == list(range(1000))
        for r in range(world):
            ids, lens, offs, _ = bench.workload("c2", r, world, 0)
            assert np.array_equal(ids, shard_ids(1024 * world, r, world))
            assert np.all(offs % 256 == 0) and np.all(lens == 8 << 20)
    ids, lens, offs, _ = bench.workload("c3", 1, 2, 0)
    assert ids.size == 2048 and int(ids[0]) == 1


def test_pack_offsets_alignment():
    offs = pack_offsets([0, 1, 255, 256, 257])
    assert offs.tolist() == [0, 0, 256, 512, 768]


def test_every_rank_checks_its_own_fixtures():
    """bench.py's parity check on every rank of an N-GPU run (N = 2, 4, 8; the C2 weak-scaling
    job and C4) finds at least four lib/hash fixtures inside that rank's shard."""
    import bench
    from s3client_amd.shard import shard_ids
    for cfg, per in (("c2", 1024), ("c4", 8192)):
        fx = bench.golden_fixtures(cfg, "sha256")
        for world in (2, 4, 8):
            for r in range(world):
                ids = shard_ids(per * world, r, world)
                assert sum(int(p) in fx for p in ids) >= 4, (cfg, world, r)


def _per_rank_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench
    got = bench.per_rank(dist, world, [rank, 10 + rank, 7])
    if rank == 0:
        q.put(got)
    dist.barrier()
    dist.destroy_process_group()


def test_bench_per_rank_gather_gloo():
    """The gloo all_gather bench.py uses for per-rank parity and C4 timings (world size 2)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_per_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got == [[0, 10, 7], [1, 11, 7]]


def test_bench_gloo_init_keeps_stdout_clean():
    """gloo prints "[Gloo] Rank r is connected ..." on stdout from C++ in every rank; bench.py's
    init_gloo keeps it off stdout, which must carry only rank 0's JSON line (world size 2)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, torch.distributed as dist; sys.path.insert(0, %r); import bench; "
            "bench.init_gloo(dist); dist.barrier(); "
            "print('{}') if dist.get_rank() == 0 else None; dist.destroy_process_group()" % root)
    port = _free_port()
    procs = [subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True,
                              env={**os.environ, "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                                   "RANK": str(r), "WORLD_SIZE": "2"})
             for r in range(2)]
    outs = [p.communicate(timeout=120) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-500:] for o in outs]
    assert outs[0][0] == "{}\n" and outs[1][0] == ""
    assert all("[Gloo]" in o[1] for o in outs)  # still printed, on stderr


def test_bench_guard_reports_a_failed_sub_measurement():
    """A sub-measurement that raises becomes {"error": ...} in the line AND an entry of the
    line's top-level errors (bench then exits non-zero); the metric survives."""
    import bench
    from s3client_amd import S3HashError
    errors = []
    assert bench._guard(errors, "x", lambda a, b: a + b, 2, 3) == 5 and errors == []
    got = bench._guard(errors, "y", lambda: 1 / 0)
    assert got == {"error": "ZeroDivisionError: division by zero"}

    def fault():
        raise S3HashError(-3, "synchronisation timeout")
    bench._guard(errors, "z", fault)
    assert [e["where"] for e in errors] == ["y", "z"]
    assert [e["device_fault"] for e in errors] == [False, True]


def test_bench_parity_failures_scan_the_whole_line():
    import bench
    line = {"parity": {"mismatches": 0, "per_rank": [{"mismatches": 0}, {"mismatches": 2}]},
            "configs": {"c4": {"kernels": {"skewp": {"parity": {"mismatches": 1}},
                                           "skews": {"digests_match_auto": True}}},
                        "c3": {"sha256_md5": {"sha256_equals_sha256_only_run": False}}},
            "host_resident": {"fixture_mismatches": 0, "digests_match_device_run": False}}
    got = sorted(e["where"] for e in bench.parity_failures(line))
    assert got == ["configs.c3.sha256_md5.sha256_equals_sha256_only_run",
                   "configs.c4.kernels.skewp.parity.mismatches",
                   "host_resident.digests_match_device_run", "parity.per_rank[1].mismatches"]
    assert bench.parity_failures({"parity": {"mismatches": 0}}) == []


def test_bench_launcher_command_touches_no_gpu():
    """`python bench.py --gpus N` with no launcher: the parent builds one torch.distributed.run
    child (N ranks, rendezvous on 127.0.0.1, the same arguments) without importing torch --
    no GPU call can precede the child."""
    import bench
    cmd, env = bench.launch_command(8, ["--gpus", "8", "--steps", "3"], 29999)
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    assert "--master-addr=127.0.0.1" in cmd and "--master-port=29999" in cmd
    assert cmd[-4:] == ["--gpus", "8", "--steps", "3"] and cmd[-5].endswith("bench.py")
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and env["S3H_BENCH_LAUNCHED"] == "1"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--no-c4",
                        "--print-launch"], capture_output=True, text=True, timeout=120,
                       env={k: v for k, v in os.environ.items() if k != "WORLD_SIZE"})
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout)
    assert got["torch_imported"] is False
    assert "--nproc-per-node=4" in got["cmd"]
    assert got["cmd"][-4:] == ["--gpus", "4", "--no-c4", "--print-launch"]


def test_bench_full_and_dump_options(tmp_path):
    """--full is off by default; --dump-outputs writes each array of 32-bit digest words as
    float64 (exact), rank 0 under the plain name and the other ranks under <name>_rank<r>."""
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    a = bench.parse(["--full", "--dump-outputs", str(tmp_path)])
    assert a.full is True and a.dump_outputs == str(tmp_path)
    words = np.array([[0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 5, 6, 7]], dtype=np.uint32)
    bench.dump_outputs(str(tmp_path / "d"), 0, digests=words.view(np.int32), md5=None)
    bench.dump_outputs(str(tmp_path / "d"), 1, digests=words)
    assert sorted(os.listdir(tmp_path / "d")) == ["digests.npy", "digests_rank1.npy"]
    for f in ("digests.npy", "digests_rank1.npy"):
        got = np.load(tmp_path / "d" / f)
        assert got.dtype == np.float64 and got.shape == (1, 8)
        assert np.array_equal(got.astype(np.uint32), words)


def test_bench_self_launch_runs_n_ranks_on_cpu():
    """The whole self-launch on a CPU host: `bench.py --gpus 2 --rank-dry-run` starts the child
    launcher, both ranks join gloo, and the parent's stdout carries ONE line from rank 0 that
    lists two distinct processes started by the bench's launcher."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2",
                        "--rank-dry-run"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    got = json.loads(lines[0])
    assert got["n_gpus"] == 2 and [x["rank"] for x in got["ranks"]] == [0, 1]
    assert len({x["pid"] for x in got["ranks"]}) == 2
    assert all(x["launched_by_bench"] for x in got["ranks"])


def _status_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench

    def check():
        if rank == 1:
            raise RuntimeError("s3hash error -3: synchronisation timeout")
    try:
        bench.status_all(dist, world, check)
        q.put((rank, "no raise"))
    except bench.DeviceFault as e:
        q.put((rank, str(e)))
    dist.barrier()  # every rank still reaches the next collective
    dist.destroy_process_group()


def test_bench_status_fault_on_one_rank_fails_every_rank():
    """A device fault reported on rank 1 raises on rank 0 too (gathered first), so no rank is
    left blocked in a collective (world size 2, gloo)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_status_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got[0] == got[1] == "rank 1: RuntimeError: s3hash error -3: synchronisation timeout"


def test_host_resident_multi_views_give_every_device_the_whole_buffer():
    """bench.host_resident_multi over N devices reads ONE bounded pinned buffer: with the host
    path's split (part i on device i % N) device k gets buffer parts 0..per-1 in order, at a
    constant stride (the 2-D copy form), whatever N."""
    import bench
    per, L = 16, 64
    h = np.arange(per * L, dtype=np.uint8)
    for ndev in (1, 2, 3, 8):
        views = bench.shared_buffer_views(h, per, ndev, L)
        assert len(views) == per * ndev
        for k in range(ndev):
            mine = views[k::ndev]
            assert [v.ctypes.data - h.ctypes.data for v in mine] == [j * L for j in range(per)]
            assert all(v.size == L for v in mine)


def test_host_resident_multi_views_read_each_devices_own_node_buffer():
    """With one pinned buffer per NUMA node (round 5), device k reads the buffer on its own
    node -- e.g. devices 0-3 on node 0 and 4-7 on node 1 -- parts 0..per-1 in order at the
    buffer's stride, and never a byte of the other node's buffer."""
    import bench
    per, L, ndev = 16, 64, 8
    node_buf = {0: np.arange(per * L, dtype=np.uint8), 1: np.arange(per * L, dtype=np.uint8)}
    dev_nodes = [0, 0, 0, 0, 1, 1, 1, 1]
    views = bench.shared_buffer_views([node_buf[dev_nodes[d]] for d in range(ndev)], per, ndev, L)
    assert len(views) == per * ndev
    for k in range(ndev):
        h = node_buf[dev_nodes[k]]
        mine = views[k::ndev]
        assert [v.ctypes.data - h.ctypes.data for v in mine] == [j * L for j in range(per)]
