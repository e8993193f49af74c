#!/usr/bin/env python3
"""SHA-1 throughput beside the project's other digests (not the product benchmark: bench.py is
untouched).  One process, profiler off.

Device-resident part (default output profiles/sha1_c2.json), HIP events, C2 (1,024 x 8 MiB):
  * SHA-1, MD5 and SHA-256 plan launches on the same buffer, alternated round by round until
    each has at least --seconds of GPU time;
  * with --exp-lib NAME=PATH (repeatable) the SHA-1 plan of an experiment build of the library
    (`make exp TAG=sha1bps1 EXPFLAGS=-DS3H_EXP_SHA1_BPS=1`: 1-block producer steps; name it
    bps1, bps3, ...) as one more item of the same alternating rounds, driven through its C-ABI;
  * SHA-256 and SHA-1 of the same buffer launched at once on two streams (what the host
    pipeline's hash streams do with every slice), beside each alone;
  * cycles per block of the SHA-1 and MD5 consumer waves from the clock probe
    (s3h_plan_set_clock_probe), and cycles / (4 x instructions per block of the shipped loop).

Host part (default output profiles/sha1_host_c2.json), wall time around the blocking calls, the
same C2 in one pinned buffer: sha256_batch_host, sha1_batch_host and sha256_sha1_batch_host,
alternated; the one-pass SHA-256 + SHA-1 rate is held to >= 0.95 of SHA-256 alone in the same run.

Every result timed is checked against hashlib before its rate is recorded.

    python tools/sha1_bench.py [--skip-host] [--skip-device] [--exp-lib bps1=tools/exp/libs3hash_sha1bps1.so]
"""
import argparse
import ctypes
import hashlib
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
HOST_BAR = 0.95   # SHA-256 + SHA-1 over SHA-256 alone, same run
BPS_BAR = 1.03    # a multi-block step form is kept only if this much faster than the 1-block form
ALGO_SHA1 = 2
u64p = ctypes.POINTER(ctypes.c_uint64)


class ExpPlan:
    """A SHA-1 plan of another build of the library, through its C-ABI (the same process and
    HIP runtime, so its launches alternate with the product's)."""

    def __init__(self, path, offs, lens):
        L = ctypes.CDLL(path)
        L.s3h_last_error.restype = ctypes.c_char_p
        L.s3h_plan_create_ex.argtypes = [ctypes.c_int, ctypes.c_int, u64p, u64p, ctypes.c_uint64,
                                         ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.s3h_plan_launch.argtypes = [ctypes.c_void_p] * 4
        L.s3h_plan_status.argtypes = [ctypes.c_void_p] * 2
        L.s3h_plan_set_clock_probe.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.POINTER(ctypes.c_uint32)]
        L.s3h_plan_destroy.argtypes = [ctypes.c_void_p]
        self.L, self.h = L, ctypes.c_void_p()
        self.check(L.s3h_plan_create_ex(0, ALGO_SHA1, offs.ctypes.data_as(u64p), lens.ctypes.data_as(u64p),
                                        len(lens), 0, ctypes.byref(self.h)))

    def check(self, rc):
        if rc:
            sys.exit(f"experiment library: {self.L.s3h_last_error().decode()}")

    def launch(self, data, out, stream=None):
        self.check(self.L.s3h_plan_launch(self.h, data.data_ptr(), out.data_ptr(), stream))

    def status(self):
        self.check(self.L.s3h_plan_status(self.h, None))

    def set_clock_probe(self, clocks):
        w = ctypes.c_uint32()
        self.check(self.L.s3h_plan_set_clock_probe(self.h, clocks.data_ptr() if clocks is not None else None,
                                                   ctypes.byref(w)))
        return w.value


def cycles_per_block(torch, plan, data, out, blocks):
    """Median over consumer waves of (clk1 - clk0) / blocks from one probed launch, and the
    shader clock in GHz from the 100 MHz real-time counter."""
    waves = plan.set_clock_probe(None)
    clocks = torch.zeros(4 * waves, dtype=torch.int64, device="cuda")
    plan.set_clock_probe(clocks)
    plan.launch(data, out)
    plan.status()
    plan.set_clock_probe(None)
    c = clocks.cpu().numpy().reshape(waves, 4)
    cyc = (c[:, 1] - c[:, 0]) / blocks
    ghz = (c[:, 1] - c[:, 0]) / np.maximum(c[:, 3] - c[:, 2], 1) * 0.1
    return {"waves": int(waves), "cycles_per_block_median": round(float(np.median(cyc)), 1),
            "cycles_per_block_max": round(float(cyc.max()), 1), "shader_GHz_median": round(float(np.median(ghz)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sha1_c2.json"))
    ap.add_argument("--host-out", default=os.path.join(ROOT, "profiles", "sha1_host_c2.json"))
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--parts", type=int, default=1024)
    ap.add_argument("--part-mib", type=int, default=8)
    ap.add_argument("--exp-lib", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-device", action="store_true")
    ap.add_argument("--git-head", default=None)
    args = ap.parse_args()
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
    views = [host[int(o):int(o) + int(m)] for o, m in zip(offs, lens)]
    pool = ThreadPoolExecutor(16)  # (hashlib releases the GIL on large buffers)

    def reference(name, words):
        raw = b"".join(pool.map(lambda v: hashlib.new(name, v).digest(), views))
        return np.frombuffer(raw, dtype=np.uint32).reshape(n, words)

    want = {"sha1": reference("sha1", 5), "md5": reference("md5", 4), "sha256": reference("sha256", 8)}
    with open(os.path.join(ROOT, "s3client_amd", "kernel_isa_counts.json")) as f:
        isa = json.load(f)
    head = args.git_head
    if head is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        head = r.stdout.strip() if r.returncode == 0 else "unknown"
    common = {"tool": "tools/sha1_bench.py", "device": torch.cuda.get_device_name(0),
              "library_sha256": file_sha256(_native.LIB_PATH), "git_head": head,
              "kernel_code_hash": {k: isa["code_hash"].get(k) for k in ("sha1-pc", "sha1-pc1", "md5-pc", "md5-pc1", "skew")}}

    if not args.skip_device:
        items, keep = {}, []
        for algo, words in (("sha1", 5), ("md5", 4), ("sha256", 8)):
            plan = s3.Plan(offs, lens, algo=algo)
            out = torch.empty((n, words), dtype=torch.int32, device="cuda")
            items[f"{algo}_c2"] = {"plan": plan, "out": out, "want": want[algo],
                                   "info": {k: plan.info()[k] for k in ("kernel", "grid")}}
        for spec in args.exp_lib:
            name, path = spec.split("=", 1)
            plan = ExpPlan(os.path.abspath(path), offs, lens)
            out = torch.empty((n, 5), dtype=torch.int32, device="cuda")
            items[f"sha1_{name}_c2"] = {"plan": plan, "out": out, "want": want["sha1"],
                                        "info": {"library": path, "library_sha256": file_sha256(path)}}
        for it in items.values():
            it["launch"] = (lambda p=it["plan"], o=it["out"]: p.launch(data, o))
            it["check"] = (lambda p=it["plan"], o=it["out"], w=it["want"]:
                           (p.status(), np.array_equal(o.cpu().numpy().view(np.uint32), w))[1])
        for name, it in items.items():  # warm-up, and every digest against hashlib first
            for _ in range(3):
                it["launch"]()
            torch.cuda.synchronize()
            if not it["check"]():
                sys.exit(f"{name}: GPU result differs from hashlib -- nothing recorded")
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for it in items.values():
            it["ms"] = []
        while min(sum(it["ms"]) for it in items.values()) < args.seconds * 1e3:
            for it in items.values():  # alternate the items in every round
                ev0.record()
                it["launch"]()
                ev1.record()
                ev1.synchronize()
                it["ms"].append(ev0.elapsed_time(ev1))
        for name, it in items.items():
            if not it["check"]():
                sys.exit(f"{name}: GPU result differs from hashlib after timing")
        gib = n * L / 2**30
        rates = {k: gib * len(it["ms"]) / (sum(it["ms"]) * 1e-3) for k, it in items.items()}
        base = "sha1_bps1_c2" if "sha1_bps1_c2" in items else "sha1_c2"  # the 1-block form
        # SHA-256 and SHA-1 at once on two streams, launched in either order: each stream's time
        # from a common start, beside the item's time alone
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        two = {"alone_ms": {k: round(sum(items[k]["ms"]) / len(items[k]["ms"]), 3) for k in ("sha256_c2", "sha1_c2")}}
        for first in ("sha256", "sha1"):
            order = [("sha256_c2", sa), ("sha1_c2", sb)]
            if first == "sha1":
                order.reverse()
            t = {"sha256_ms": [], "sha1_ms": []}
            for i in range(6):
                ev0.record()
                sa.wait_event(ev0)
                sb.wait_event(ev0)
                for k, st in order:
                    items[k]["plan"].launch(data, items[k]["out"], st)
                ea.record(sa)
                eb.record(sb)
                ea.synchronize()
                eb.synchronize()
                if i:  # the first run is the warm-up
                    t["sha256_ms"].append(round(ev0.elapsed_time(ea), 3))
                    t["sha1_ms"].append(round(ev0.elapsed_time(eb), 3))
            for k in ("sha256_c2", "sha1_c2"):
                if not items[k]["check"]():
                    sys.exit(f"{k}: GPU result differs from hashlib after the two-stream launches")
            t["both_GiB_per_s"] = round(gib * len(t["sha1_ms"]) /
                                        (sum(max(x, y) for x, y in zip(t["sha256_ms"], t["sha1_ms"])) * 1e-3), 1)
            two[f"{first}_launched_first"] = t
        blocks = (L + 72) >> 6
        probe = {}
        for k, isa_key in [("sha1_c2", "sha1-pc"), ("md5_c2", "md5-pc")] + \
                          [(f"sha1_{s.split('=', 1)[0]}_c2", {"bps1": "sha1-pc1"}.get(s.split("=", 1)[0]))
                           for s in args.exp_lib]:
            p = cycles_per_block(torch, items[k]["plan"], data, items[k]["out"], blocks)
            if isa_key:
                ipb = isa["kernels"][isa_key]["instr_per_block"]
                p["instr_per_block"] = ipb
                p["cycles_over_4x_instr"] = round(p["cycles_per_block_median"] / (4 * ipb), 3)
            probe[k] = p
        doc = {**common,
               "config": {"c2": f"{n} x {args.part_mib} MiB, device-resident", "seconds_per_item": args.seconds,
                          "timing": "HIP events, one launch per item per round, items alternated"},
               "GiB_per_s": {k: round(v, 1) for k, v in rates.items()},
               "GiB_per_s_min_max": {k: [round(gib / (max(it["ms"]) * 1e-3), 1), round(gib / (min(it["ms"]) * 1e-3), 1)]
                                     for k, it in items.items()},
               "launches": {k: len(it["ms"]) for k, it in items.items()},
               "plans": {k: it["info"] for k, it in items.items()},
               "clock_probe": probe,
               "sha1_over_sha256_c2": round(rates["sha1_c2"] / rates["sha256_c2"], 3),
               "bar": "sha1_c2 >= sha256_c2", "bar_met": bool(rates["sha1_c2"] >= rates["sha256_c2"]),
               "step_forms": {k: {"GiB_per_s": round(rates[k], 1), "over_1_block_form": round(rates[k] / rates[base], 4),
                                  "at_least_the_bar": bool(rates[k] >= BPS_BAR * rates[base])}
                              for k in items if k.startswith("sha1_")},
               "step_form_product": f"sha1_c2 = sha1_pc_kernel<{isa['kernels']['sha1-pc']['blocks_per_step']}>",
               "step_form_bar": BPS_BAR, "two_streams": two,
               "checked_against_hashlib": sorted(items)}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(doc, sort_keys=True))
        del items, keep

    if not args.skip_host:
        parts = s3.BufferParts(pinned, offs, lens)

        def run_sha():
            return np.array_equal(s3.sha256_batch_host(parts), want["sha256"])

        def run_sha1():
            return np.array_equal(s3.sha1_batch_host(parts), want["sha1"])

        def run_dual():
            sha, s1 = s3.sha256_sha1_batch_host(parts)
            return np.array_equal(sha, want["sha256"]) and np.array_equal(s1, want["sha1"])

        hitems = {"sha256": run_sha, "sha1": run_sha1, "sha256_sha1": run_dual}
        for name, fn in hitems.items():  # warm-up: contexts, rings, plans
            for _ in range(2):
                if not fn():
                    sys.exit(f"{name}: GPU result differs from hashlib -- nothing recorded")
        rounds = {name: [] for name in hitems}
        while min(sum(t) for t in rounds.values()) < args.seconds:
            for name, fn in hitems.items():
                t0 = time.perf_counter()
                ok = fn()  # (the comparison with the reference is inside the timed span: ~1 ms)
                dt = time.perf_counter() - t0
                if not ok:
                    sys.exit(f"{name}: GPU result differs from hashlib -- nothing recorded")
                rounds[name].append(dt)
        gib = n * L / 2**30
        rates = {name: gib * len(t) / sum(t) for name, t in rounds.items()}
        ratio = rates["sha256_sha1"] / rates["sha256"]
        doc = {**common,
               "config": {"c2": f"{n} x {args.part_mib} MiB, one pinned buffer", "seconds_per_item": args.seconds,
                          "timing": "wall time around the blocking calls, items alternated per round"},
               "GiB_per_s": {k: round(v, 2) for k, v in rates.items()},
               "GiB_per_s_min_max": {k: [round(gib / max(t), 2), round(gib / min(t), 2)] for k, t in rounds.items()},
               "round_seconds": {k: [round(x, 5) for x in t] for k, t in rounds.items()},
               "sha256_sha1_over_sha256": round(ratio, 4), "bar": HOST_BAR, "bar_met": bool(ratio >= HOST_BAR),
               "checked_against_hashlib": sorted(hitems)}
        os.makedirs(os.path.dirname(os.path.abspath(args.host_out)), exist_ok=True)
        with open(args.host_out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
