#!/usr/bin/env python3
"""CRC-32C / CRC-32 throughput beside the project's other digests and the read roof (not the
product benchmark: bench.py is untouched).  One process, profiler off, device-resident data:

  * CRC-32C and CRC-32 plan launches on C2 (1,024 x 8 MiB) and on one part of 1 GiB;
  * MD5-alone and SHA-256 plan launches on the same C2 buffer, alternated with the CRC launches;
  * a read-roof kernel (tools/crc_roof.hip, this tool's own): the CRC segment kernel's grid,
    segment table and dwordx4 loads, XOR-reduced.

With --crc64 the same run also times CRC-64/NVME (crc64_kernels.hip) on both shapes and, beside
CRC-32C, on a ragged batch (one 64 MiB part plus 4,096 parts of U[1, 128] KiB), and writes
profiles/crc64_c2.json instead: its rate, its ratio to the read roof and to CRC-32C of the run.

Every item is warmed up, then timed with HIP events in rounds that alternate between the items
until each has at least --seconds of GPU time.  Every digest timed is checked against the CPU
value before its rate is recorded.  Writes one JSON document (default profiles/crc_c2.json).

    make crcbench && python tools/crc_bench.py [--out profiles/crc_c2.json] [--git-head SHA]
    make crcbench && python tools/crc_bench.py --crc64 [--out profiles/crc64_c2.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ROOF_LIB = os.path.join(ROOT, "tools", "libcrc_roof.so")
BAR = 8.0  # CRC-32C over MD5-alone on C2, same run


def segment_table(offs, lens, S):
    """The plan's stage-1 table (kernel_abi.hpp CrcSeg: u64 offset, u32 length, u32 pad)."""
    rows = []
    for o, n in zip(offs, lens):
        for done in range(0, int(n), S):
            rows.append((int(o) + done, min(S, int(n) - done), 0))
    return np.array(rows, dtype=np.dtype([("off", "<u8"), ("len", "<u4"), ("pad", "<u4")]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--crc64", action="store_true",
                    help="also time CRC-64/NVME and the ragged batch; default output profiles/crc64_c2.json")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--parts", type=int, default=1024)
    ap.add_argument("--part-mib", type=int, default=8)
    ap.add_argument("--big-mib", type=int, default=1024)
    ap.add_argument("--git-head", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "crc64_c2.json" if args.crc64 else "crc_c2.json")
    import torch

    import s3client_amd as s3
    from bench import SEED
    from code_object import file_sha256
    from s3client_amd import _native

    if not os.path.exists(ROOF_LIB):
        sys.exit(f"{ROOF_LIB} missing: run `make crcbench`")
    roof = ctypes.CDLL(ROOF_LIB)
    roof.crc_roof_launch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                     ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]

    n, L = args.parts, args.part_mib << 20
    big = args.big_mib << 20
    assert big <= n * L
    data = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    offs = np.arange(n, dtype=np.uint64) * np.uint64(L)
    lens = np.full(n, L, dtype=np.uint64)
    s3.generate_parts(data, offs, lens, np.arange(n, dtype=np.uint64), SEED)
    torch.cuda.synchronize()
    host = data.cpu().numpy()
    shapes = {"c2": (offs, lens), "one_part": (np.zeros(1, np.uint64), np.array([big], np.uint64))}
    stream = torch.cuda.current_stream().cuda_stream
    pool = ThreadPoolExecutor(16)

    def cpu(fn, o, l):  # the ctypes calls release the GIL
        return list(pool.map(lambda ol: fn(host[int(ol[0]):int(ol[0]) + int(ol[1])]), zip(o, l)))

    items, keep = {}, []
    for shape, (o, l) in shapes.items():
        for algo in ("crc32c", "crc32"):
            plan = s3.CrcPlan(o, l, algo=algo)
            out = torch.empty(len(l), dtype=torch.int32, device="cuda")
            want = np.array(cpu(lambda b: s3.crc(b, algo), o, l), dtype=np.uint32)
            info = plan.info()
            items[f"{algo}_{shape}"] = {
                "launch": (lambda p=plan, out=out: p.launch(data, out)), "bytes": int(l.sum()),
                "check": (lambda out=out, want=want: np.array_equal(out.cpu().numpy().view(np.uint32), want)),
                "info": info}
            keep.append(plan)
        if args.crc64:
            plan = s3.Crc64Plan(o, l)
            out = torch.empty(len(l), dtype=torch.int64, device="cuda")
            want = np.array(cpu(s3.crc64, o, l), dtype=np.uint64)
            items[f"crc64nvme_{shape}"] = {
                "launch": (lambda p=plan, out=out: p.launch(data, out)), "bytes": int(l.sum()),
                "check": (lambda out=out, want=want: np.array_equal(out.cpu().numpy().view(np.uint64), want)),
                "info": plan.info()}
            assert plan.info()["segment_bytes"] == info["segment_bytes"]
            keep.append(plan)
        segs = segment_table(o, l, info["segment_bytes"])
        assert len(segs) == info["segments"]
        d_segs = torch.from_numpy(segs.view(np.uint8)).cuda()
        d_out = torch.empty(len(segs), dtype=torch.int32, device="cuda")
        want = np.bitwise_xor.reduce(host[:int(l.sum())].view(np.uint32).reshape(len(segs), -1), axis=1)
        items[f"roof_{shape}"] = {
            "launch": (lambda d_segs=d_segs, d_out=d_out, k=len(segs), g=info["grid"]:
                       roof.crc_roof_launch(data.data_ptr(), d_segs.data_ptr(), k, g, d_out.data_ptr(), stream)),
            "bytes": int(l.sum()), "info": {"grid": info["grid"], "segments": len(segs)},
            "check": (lambda d_out=d_out, want=want: np.array_equal(d_out.cpu().numpy().view(np.uint32), want))}
    if args.crc64:  # ragged: one 64 MiB part, then 4,096 parts of U[1, 128] KiB, back to back
        rl = np.concatenate([[64 << 20], np.random.default_rng(SEED).integers(1, (128 << 10) + 1, 4096)]).astype(np.uint64)
        ro = np.concatenate([[0], np.cumsum(rl)[:-1]]).astype(np.uint64)
        assert int(rl.sum()) <= n * L
        shapes["ragged"] = (ro, rl)
        for name, mk, dt, fn in (("crc32c", lambda: s3.CrcPlan(ro, rl, algo="crc32c"), np.uint32,
                                  lambda b: s3.crc(b, "crc32c")),
                                 ("crc64nvme", lambda: s3.Crc64Plan(ro, rl), np.uint64, s3.crc64)):
            plan = mk()
            out = torch.empty(len(rl), dtype=torch.int32 if dt is np.uint32 else torch.int64, device="cuda")
            want = np.array(cpu(fn, ro, rl), dtype=dt)
            items[f"{name}_ragged"] = {
                "launch": (lambda p=plan, out=out: p.launch(data, out)), "bytes": int(rl.sum()),
                "check": (lambda out=out, want=want, dt=dt: np.array_equal(out.cpu().numpy().view(dt), want)),
                "info": plan.info()}
            keep.append(plan)
    for algo, words, fn in (("md5", 4, s3.md5), ("sha256", 8, s3.sha256)):
        plan = s3.Plan(offs, lens, algo=algo)
        out = torch.empty((n, words), dtype=torch.int32, device="cuda")
        want = np.array(cpu(fn, offs, lens), dtype=np.uint32)
        items[f"{algo}_c2"] = {
            "launch": (lambda p=plan, out=out: p.launch(data, out)), "bytes": n * L,
            "check": (lambda p=plan, out=out, want=want:
                      (p.status(), np.array_equal(out.cpu().numpy().view(np.uint32), want))[1]),
            "info": {k: plan.info()[k] for k in ("kernel", "grid")}}
        keep.append(plan)

    # warm-up, and every digest against the CPU before anything is recorded
    for name, it in items.items():
        for _ in range(3):
            it["launch"]()
        torch.cuda.synchronize()
        if not it["check"]():
            sys.exit(f"{name}: GPU result differs from the CPU value -- nothing recorded")
    # one launch's time -> launches per round (~50 ms of GPU time)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in items.values():
        ev0.record()
        it["launch"]()
        ev1.record()
        ev1.synchronize()
        it["reps"] = max(1, int(50.0 / max(ev0.elapsed_time(ev1), 1e-3)))
        it["ms"], it["launches"] = 0.0, 0
    while min(it["ms"] for it in items.values()) < args.seconds * 1e3:
        for it in items.values():  # alternate: CRC, roof, MD5, SHA-256 in every round
            ev0.record()
            for _ in range(it["reps"]):
                it["launch"]()
            ev1.record()
            ev1.synchronize()
            it["ms"] += ev0.elapsed_time(ev1)
            it["launches"] += it["reps"]
    torch.cuda.synchronize()
    for name, it in items.items():
        if not it["check"]():
            sys.exit(f"{name}: GPU result differs from the CPU value after timing")

    rates = {name: it["bytes"] * it["launches"] / (it["ms"] * 1e-3) / 2**30 for name, it in items.items()}
    with open(os.path.join(ROOT, "s3client_amd", "kernel_isa_counts.json")) as f:
        hashes = json.load(f)["code_hash"]
    head = args.git_head
    if head is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        head = r.stdout.strip() if r.returncode == 0 else "unknown"
    md5 = rates["md5_c2"]
    doc = {
        "tool": "tools/crc_bench.py", "device": torch.cuda.get_device_name(0),
        "config": {"c2": f"{n} x {args.part_mib} MiB", "one_part": f"1 x {args.big_mib} MiB",
                   **({"ragged": "1 x 64 MiB + 4096 x U[1, 128] KiB"} if args.crc64 else {}),
                   "seconds_per_item": args.seconds, "timing": "HIP events, items alternated per round"},
        "GiB_per_s": {k: round(v, 1) for k, v in rates.items()},
        "launches": {k: it["launches"] for k, it in items.items()},
        "ms_per_launch": {k: round(it["ms"] / it["launches"], 4) for k, it in items.items()},
        "plans": {k: it["info"] for k, it in items.items()},
        "segment_bytes": {s: items[f"crc32c_{s}"]["info"]["segment_bytes"] for s in shapes},
        "crc_over_read_roof": {f"{a}_{s}": round(rates[f"{a}_{s}"] / rates[f"roof_{s}"], 3)
                               for a in ("crc32c", "crc32") + (("crc64nvme",) if args.crc64 else ())
                               for s in ("c2", "one_part")},
        "crc32c_over_md5_c2": {s: round(rates[f"crc32c_{s}"] / md5, 2) for s in ("c2", "one_part")},
        "bar": BAR, "bar_met": all(rates[f"crc32c_{s}"] >= BAR * md5 for s in ("c2", "one_part")),
        **({"crc64nvme_over_crc32c": {s: round(rates[f"crc64nvme_{s}"] / rates[f"crc32c_{s}"], 3) for s in shapes},
            "ragged_ms_per_launch": {a: round(items[f"{a}_ragged"]["ms"] / items[f"{a}_ragged"]["launches"], 4)
                                     for a in ("crc32c", "crc64nvme")}} if args.crc64 else {}),
        "checked_against_cpu": sorted(items),
        "kernel_code_hash": {k: hashes.get(k) for k in ("crc_segments", "crc_parts", "md5-pc", "md5-pc1",
                                                         "skew", "skew_nc2", "skewp", "skews") +
                             (("crc64_segments", "crc64_parts") if args.crc64 else ())},
        "library_sha256": file_sha256(_native.LIB_PATH), "git_head": head,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
