#!/usr/bin/env python3
"""SHA-256 + CRC-32C of host-resident parts from one pass over the host link, beside SHA-256
alone and the CRC alone (not the product benchmark: bench.py is untouched).  One process,
profiler off, wall time around the blocking calls.  Data: C2 (1,024 x 8 MiB) in one pinned
buffer.  Three items, alternated round by round until each has at least --seconds:

  * sha256_batch_host
  * sha256_crc_batch_host with CRC-32C
  * crc_batch_host (CRC-32C)

With --crc64 two more items run in the same alternating rounds -- sha256_crc64_batch_host and
crc64_batch_host (CRC-64/NVME) -- the ranged-against-whole comparison is repeated on a CRC-64
plan, and the document goes to profiles/crc64_host_c2.json: the one-pass SHA-256 + CRC-64/NVME
rate is held to the same bar, >= 0.95 of SHA-256 alone in the same run.

Every result is checked against the CPU before its rate is recorded.  Also recorded, with HIP
events and no bar: a device-resident C2 pass in ranged launches of 256 KiB against one whole
launch of the same plan.  Writes one JSON document (default profiles/crc_host_c2.json) with
every round's times.

    python tools/crc_host_bench.py [--out profiles/crc_host_c2.json] [--git-head SHA]
    python tools/crc_host_bench.py --crc64 [--out profiles/crc64_host_c2.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
BAR = 0.95  # SHA-256 + CRC-32C over SHA-256 alone, same run
RANGE_BYTES = 256 << 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--crc64", action="store_true",
                    help="also time CRC-64/NVME; default output profiles/crc64_host_c2.json")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--parts", type=int, default=1024)
    ap.add_argument("--part-mib", type=int, default=8)
    ap.add_argument("--git-head", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "crc64_host_c2.json" if args.crc64 else "crc_host_c2.json")
    import torch

    import s3client_amd as s3
    from bench import SEED
    from code_object import file_sha256
    from s3client_amd import _native

    n, L = args.parts, args.part_mib << 20
    offs = np.arange(n, dtype=np.uint64) * np.uint64(L)
    lens = np.full(n, L, dtype=np.uint64)
    data = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    s3.generate_parts(data, offs, lens, np.arange(n, dtype=np.uint64), SEED)
    torch.cuda.synchronize()
    pinned = torch.empty(n * L, dtype=torch.uint8, pin_memory=True)
    pinned.copy_(data)
    torch.cuda.synchronize()
    host = pinned.numpy()
    parts = s3.BufferParts(pinned, offs, lens)

    pool = ThreadPoolExecutor(16)  # (the ctypes calls release the GIL)
    views = [host[int(o):int(o) + int(m)] for o, m in zip(offs, lens)]
    want_sha = np.array(list(pool.map(s3.sha256, views)), dtype=np.uint32).reshape(n, 8)
    want_crc = np.array(list(pool.map(lambda b: s3.crc(b, "crc32c"), views)), dtype=np.uint32)

    def run_sha():
        return np.array_equal(s3.sha256_batch_host(parts), want_sha)

    def run_dual():
        sha, crcs = s3.sha256_crc_batch_host(parts, "crc32c")
        return np.array_equal(sha, want_sha) and np.array_equal(crcs, want_crc)

    def run_crc():
        return np.array_equal(s3.crc_batch_host(parts, "crc32c"), want_crc)

    items = {"sha256": run_sha, "sha256_crc32c": run_dual, "crc32c": run_crc}
    if args.crc64:
        want_crc64 = np.array(list(pool.map(s3.crc64, views)), dtype=np.uint64)

        def run_dual64():
            sha, crcs = s3.sha256_crc64_batch_host(parts)
            return np.array_equal(sha, want_sha) and np.array_equal(crcs, want_crc64)

        def run_crc64():
            return np.array_equal(s3.crc64_batch_host(parts), want_crc64)

        items.update({"sha256_crc64nvme": run_dual64, "crc64nvme": run_crc64})
    for name, fn in items.items():  # warm-up: contexts, rings, plans
        for _ in range(2):
            if not fn():
                sys.exit(f"{name}: GPU result differs from the CPU value -- nothing recorded")
    rounds = {name: [] for name in items}
    while min(sum(t) for t in rounds.values()) < args.seconds:
        for name, fn in items.items():
            t0 = time.perf_counter()
            ok = fn()  # (the comparison with the CPU values is inside the timed span: ~1 ms)
            dt = time.perf_counter() - t0
            if not ok:
                sys.exit(f"{name}: GPU result differs from the CPU value -- nothing recorded")
            rounds[name].append(dt)
    gib = n * L / 2**30
    rates = {name: gib * len(t) / sum(t) for name, t in rounds.items()}

    # device-resident: one whole launch against the same pass in ranged launches (informational)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def resident_pass(kind, plan, tdt, ndt, want):
        stream_out = torch.empty(n, dtype=tdt, device="cuda")
        device = {}

        def whole():
            plan.launch(data, stream_out)

        def ranged():
            for b in range(0, L, RANGE_BYTES):
                plan.launch_range(data, stream_out, b, min(b + RANGE_BYTES, L))

        for name, fn in (("whole_launch", whole), ("ranged_256KiB", ranged)):
            ms = []
            for i in range(6):
                stream_out.zero_()
                ev0.record()
                fn()
                ev1.record()
                ev1.synchronize()
                if not np.array_equal(stream_out.cpu().numpy().view(ndt), want):
                    sys.exit(f"{kind} {name}: GPU result differs from the CPU value -- nothing recorded")
                if i:  # the first run is the warm-up
                    ms.append(ev0.elapsed_time(ev1))
            device[name] = {"ms": [round(x, 3) for x in ms],
                            "GiB_per_s": round(gib * len(ms) / (sum(ms) * 1e-3), 1)}
        device["segment_bytes"] = plan.info()["segment_bytes"]
        device["launches_per_ranged_pass"] = (L + RANGE_BYTES - 1) // RANGE_BYTES
        return device

    resident = {}
    with s3.CrcPlan(offs, lens, algo="crc32c") as plan:
        resident["crc32c"] = resident_pass("crc32c", plan, torch.int32, np.uint32, want_crc)
    if args.crc64:
        with s3.Crc64Plan(offs, lens) as plan:
            resident["crc64nvme"] = resident_pass("crc64nvme", plan, torch.int64, np.uint64, want_crc64)

    with open(os.path.join(ROOT, "s3client_amd", "kernel_isa_counts.json")) as f:
        hashes = json.load(f)["code_hash"]
    head = args.git_head
    if head is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        head = r.stdout.strip() if r.returncode == 0 else "unknown"
    ratio = rates["sha256_crc32c"] / rates["sha256"]
    doc = {
        "tool": "tools/crc_host_bench.py", "device": torch.cuda.get_device_name(0),
        "config": {"c2": f"{n} x {args.part_mib} MiB, one pinned buffer", "seconds_per_item": args.seconds,
                   "timing": "wall time around the blocking calls, items alternated per round"},
        "GiB_per_s": {k: round(v, 2) for k, v in rates.items()},
        "GiB_per_s_min_max": {k: [round(gib / max(t), 2), round(gib / min(t), 2)] for k, t in rounds.items()},
        "round_seconds": {k: [round(x, 5) for x in t] for k, t in rounds.items()},
        "sha256_crc32c_over_sha256": round(ratio, 4), "bar": BAR, "bar_met": bool(ratio >= BAR),
        "device_resident_crc32c": resident["crc32c"],
        **({"sha256_crc64nvme_over_sha256": round(rates["sha256_crc64nvme"] / rates["sha256"], 4),
            "bar_met_crc64nvme": bool(rates["sha256_crc64nvme"] / rates["sha256"] >= BAR),
            "sha256_crc64nvme_over_sha256_crc32c": round(rates["sha256_crc64nvme"] / rates["sha256_crc32c"], 4),
            "device_resident_crc64nvme": resident["crc64nvme"]} if args.crc64 else {}),
        "checked_against_cpu": sorted(items) + ["whole_launch", "ranged_256KiB"],
        "kernel_code_hash": {k: hashes.get(k) for k in ("crc_segments", "crc_parts", "crc_range_pieces",
                                                         "crc_range_parts", "skew", "skew_nc2", "skewp", "skews") +
                             (("crc64_segments", "crc64_parts", "crc64_range_pieces", "crc64_range_parts")
                              if args.crc64 else ())},
        "library_sha256": file_sha256(_native.LIB_PATH), "git_head": head,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
