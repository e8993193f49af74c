"""bench.py's multi-GPU plumbing on the GPU box (pytest -m gpu): `python bench.py --gpus 2`
with NO external launcher starts its two ranks itself (a child torch.distributed.run), and
rank 0's single JSON line carries both ranks' devices, per-rank fixture parity and no errors.
On a one-GPU box the two ranks share the device (S3H_BENCH_SHARE_GPU=1, the rehearsal mode);
the driver's N-GPU runs use the same code with one device per rank."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_self_launches_two_ranks(torch_cuda):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["S3H_BENCH_SHARE_GPU"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2",
                        "--warmup", "1", "--full", "--no-c4", "--no-host-resident"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and "errors" not in line, line.get("errors")
    assert [d["rank"] for d in line["devices"]] == [0, 1]
    assert all(d["pci_bus_id"].count(":") == 2 and d["arch"].startswith("gfx950") for d in line["devices"])
    assert line["distinct_devices"] == 1  # shared on purpose here
    per = line["parity"]["per_rank"]
    assert [p["rank"] for p in per] == [0, 1] and all(p["fixtures_checked"] >= 4 for p in per)
    assert line["parity"]["mismatches"] == 0
    assert "timed 2 steps" in line["phases_s"]
    assert "[bench rank 0] timed 2 steps" in r.stderr


def test_plain_run_is_lean_and_dumps_its_digests(torch_cuda, golden, tmp_path):
    """A plain run (no --full) times exactly --steps launches, prints the headline line without
    any sub-measurement, and --dump-outputs writes the last step's digest table: float64 words,
    one row per part, equal to the lib/hash fixtures of the parts that have one (64 parts keep
    the run short; C2 fixture ids 0..15 are among them)."""
    import numpy as np
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--parts-per-gpu", "64", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and "timed 3 steps" in line["phases_s"]
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    assert line["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region: 64 x 8 MiB = 0.5 GiB per step
    assert abs(line["value"] - 0.5 / (line["ms_per_step"] / 1e3)) <= 0.01 * line["value"]
    assert line["full"] is False and "errors" not in line
    for k in ("parity", "roofline", "issue", "power", "library", "cpu_baseline", "host_resident",
              "c5_loopback", "f_rows", "configs"):
        assert k not in line, k
    assert sorted(p.name for p in out.iterdir()) == ["digests.npy"]
    d = np.load(out / "digests.npy")
    assert d.dtype == np.float64 and d.shape == (64, 8)
    words = d.astype(np.uint32)
    assert np.array_equal(words.astype(np.float64), d)
    fx = {e["p"]: e["digest"] for e in golden["c2_parts"] if e["p"] < 64}
    assert len(fx) >= 16
    import s3client_amd as s3
    for p, want in fx.items():
        assert s3.hash_to_text(words[p]) == want, p
