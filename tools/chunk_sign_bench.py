#!/usr/bin/env python3
"""SigV4 chunk-signed uploads beside the whole-part SHA-256 they replace (not the product
benchmark: bench.py is untouched).  One process, profiler off, device-resident data, 64 KiB
chunks.  Three shapes out of one buffer: C2 (1,024 x 8 MiB), 8 x 8 MiB and one part of 1 GiB.
Per shape, alternated round by round and timed with HIP events:
  * whole  -- the whole-part SHA-256 plan (the yardstick: what an upload without chunk signing
              hashes; one launch only for the 1 GiB part, a 15 s chain);
  * chunk  -- the chunk plan: chunk hashes + signature chains (s3h_chunk_plan_launch);
  * hash   -- an ordinary SHA-256 plan over the same chunks (the chunk plan's first launch alone);
  * chain  -- the chain kernel alone on ready digests (s3h_chunk_plan_chain);
and s3h_cpu_chunk_signatures on the same digests (host wall time).

Checked before anything is recorded: the chunk plan's signatures equal the CPU chain's over the
GPU's chunk digests for every part, equal hashlib + hmac from the bytes for sampled parts, and
the whole-part digests equal hashlib for sampled parts.

The one bar: on C2 the chunk plan's payload rate is above the whole-part SHA-256 rate.

    python tools/chunk_sign_bench.py [--out profiles/chunk_sign_c2.json]
"""
import argparse
import hashlib
import hmac
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SECRET, DATE, TIMESTAMP, REGION, SERVICE = "wJalrXUtnFEMI/K7MDENG/bPxRfiCYEXAMPLEKEY", "20130524", "20130524T000000Z", "us-east-1", "s3"
EMPTY = hashlib.sha256(b"").hexdigest()


def hmac_chain(key, seed, part, chunk):
    """Signatures of one part from its bytes, by the definition (hashlib + hmac)."""
    prefix = f"AWS4-HMAC-SHA256-PAYLOAD\n{TIMESTAMP}\n{DATE}/{REGION}/{SERVICE}/aws4_request\n"
    prev, out = seed, []
    for d in [hashlib.sha256(part[i:i + chunk]).digest() for i in range(0, len(part), chunk)] + \
             [hashlib.sha256(b"").digest()]:
        prev = hmac.new(key, (prefix + prev.hex() + "\n" + EMPTY + "\n" + d.hex()).encode(), hashlib.sha256).digest()
        out.append(prev)
    return b"".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_sign_c2.json"))
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--chunk-kib", type=int, default=64)
    ap.add_argument("--git-head", default=None)
    args = ap.parse_args()
    import torch

    import s3client_amd as s3
    from bench import SEED
    from code_object import file_sha256
    from s3client_amd import _native

    chunk = args.chunk_kib << 10
    n, L = 1024, 8 << 20
    offs = np.arange(n, dtype=np.uint64) * np.uint64(L)
    lens = np.full(n, L, dtype=np.uint64)
    data = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    s3.generate_parts(data, offs, lens, np.arange(n, dtype=np.uint64), SEED)
    torch.cuda.synchronize()
    key = s3.sigv4_signing_key(SECRET, DATE, REGION, SERVICE)
    ctx = s3.ChunkSignContext(key, TIMESTAMP, DATE, REGION, SERVICE)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def shape(name, o, m, rounds, whole_rounds, samples):
        o, m = np.asarray(o, dtype=np.uint64), np.asarray(m, dtype=np.uint64)
        parts = len(m)
        seeds = np.random.default_rng(parts).integers(0, 2**32, (parts, 8), dtype=np.uint32)
        d_seeds = torch.from_numpy(seeds.view(np.int32)).cuda()
        cplan = s3.ChunkSignPlan(o, m, chunk)
        counts = cplan.data_chunks_per_part
        co = np.concatenate([oo + np.arange(c, dtype=np.uint64) * np.uint64(chunk) for oo, c in zip(o, counts)])
        cl = np.concatenate([np.minimum(np.uint64(chunk), mm - np.arange(c, dtype=np.uint64) * np.uint64(chunk))
                             for mm, c in zip(m, counts)])
        hplan = s3.Plan(co, cl)
        wplan = s3.Plan(o, m)
        d_dig = torch.empty((len(cl), 8), dtype=torch.int32, device="cuda")
        d_whole = torch.empty((parts, 8), dtype=torch.int32, device="cuda")
        d_sig = torch.empty((cplan.signatures, 8), dtype=torch.int32, device="cuda")
        d_sig2 = torch.empty((cplan.signatures, 8), dtype=torch.int32, device="cuda")
        items = {"whole": lambda: wplan.launch(data, d_whole),
                 "chunk": lambda: cplan.launch(data, ctx, d_seeds, d_sig),
                 "hash": lambda: hplan.launch(data, d_dig),
                 "chain": lambda: cplan.chain(ctx, d_dig, d_seeds, d_sig2)}
        # warm-up and checks (the whole-part launch of a lone 1 GiB chain runs once, timed)
        ms = {k: [] for k in items}
        for k in ("chunk", "hash", "chain") + (("whole",) if whole_rounds > 1 else ()):
            items[k]()
        cplan.status(), hplan.status(), wplan.status()
        digs = d_dig.cpu().numpy().view(np.uint32)
        t0 = time.perf_counter()
        cpu_sig = s3.cpu_chunk_signatures(ctx, digs, counts, seeds)
        cpu_s = [time.perf_counter() - t0]
        for _ in range(4):
            t0 = time.perf_counter()
            s3.cpu_chunk_signatures(ctx, digs, counts, seeds)
            cpu_s.append(time.perf_counter() - t0)
        for buf, what in ((d_sig, "chunk plan"), (d_sig2, "chain alone")):
            if not np.array_equal(buf.cpu().numpy().view(np.uint32), cpu_sig):
                sys.exit(f"{name}: {what} signatures differ from the CPU chain -- nothing recorded")
        for p in samples:  # from the bytes, by the definition
            raw = data[int(o[p]):int(o[p] + m[p])].cpu().numpy().tobytes()
            at = int(cplan.signature_offsets[p])
            if hmac_chain(key, seeds[p].tobytes(), raw, chunk) != cpu_sig[at:at + int(counts[p]) + 1].tobytes():
                sys.exit(f"{name}: part {p} differs from hashlib + hmac -- nothing recorded")
        for r in range(rounds):
            for k, fn in items.items():
                if k == "whole" and r >= whole_rounds:
                    continue
                ev0.record()
                fn()
                ev1.record()
                ev1.synchronize()
                ms[k].append(ev0.elapsed_time(ev1))
        cplan.status(), hplan.status(), wplan.status()
        whole = d_whole.cpu().numpy().view(np.uint32)
        for p in samples:
            raw = data[int(o[p]):int(o[p] + m[p])].cpu().numpy().tobytes()
            if hashlib.sha256(raw).digest() != whole[p].tobytes():
                sys.exit(f"{name}: whole-part digest of part {p} differs from hashlib -- nothing recorded")
        if not np.array_equal(d_sig.cpu().numpy().view(np.uint32), cpu_sig):
            sys.exit(f"{name}: chunk plan signatures differ after timing")
        gib = float(m.sum()) / 2**30
        mean = {k: sum(v) / len(v) for k, v in ms.items()}
        row = {"parts": parts, "part_bytes": int(m[0]), "chunk_bytes": chunk, "data_chunks": int(len(cl)),
               "signatures": int(cplan.signatures), "max_chunks_per_part": int(counts.max()),
               "chunk_hash_kernel": cplan.info()["kernel"], "whole_part_kernel": wplan.info()["kernel"],
               "launches": {k: len(v) for k, v in ms.items()},
               "ms_mean": {k: round(v, 3) for k, v in mean.items()},
               "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
               "GiB_per_s": {k: round(gib / (mean[k] * 1e-3), 1) for k in ("whole", "chunk", "hash")},
               "chunk_over_whole": round(mean["whole"] / mean["chunk"], 2),
               "chain_share_of_chunk_plan": round(mean["chain"] / mean["chunk"], 3),
               "chain_us_per_link": round(mean["chain"] * 1e3 / (int(counts.max()) + 1), 2),
               "cpu_chain_ms_min": round(min(cpu_s) * 1e3, 3), "cpu_chain_ms_mean": round(sum(cpu_s) / len(cpu_s) * 1e3, 3),
               "cpu_chain_over_gpu_chain": round(mean["chain"] / (min(cpu_s) * 1e3), 2),
               "checked_against_hmac_parts": [int(p) for p in samples]}
        print(name, json.dumps(row, sort_keys=True), flush=True)
        for pl in (cplan, hplan, wplan):
            pl.close()
        return row

    rows = {"c2": shape("c2", offs, lens, args.rounds, args.rounds, (0, 511, 1023)),
            "8x8MiB": shape("8x8MiB", offs[:8], lens[:8], args.rounds, args.rounds, (0, 7)),
            "1x1GiB": shape("1x1GiB", [0], [1 << 30], 3, 1, (0,))}
    with open(os.path.join(ROOT, "s3client_amd", "kernel_isa_counts.json")) as f:
        isa = json.load(f)
    head = args.git_head
    if head is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        head = r.stdout.strip() if r.returncode == 0 else "unknown"
    per, cpus = s3.host_threads(1)
    doc = {"tool": "tools/chunk_sign_bench.py", "device": torch.cuda.get_device_name(0),
           "library_sha256": file_sha256(_native.LIB_PATH), "git_head": head,
           "kernel_code_hash": {k: isa["code_hash"].get(k) for k in ("chunk-chain", "lane", "skew", "skew_nc2", "pc")},
           "config": {"timing": "HIP events, one launch per item per round, items alternated; CPU chain: wall time, 5 calls",
                      "prefix_bytes": 66 + len(REGION) + len(SERVICE), "cpu_backend": s3.cpu_backend(),
                      "cpu_chain_threads": per, "cpus": cpus},
           "shapes": rows,
           "bar": "c2: chunk plan GiB/s > whole-part SHA-256 GiB/s of the same run",
           "bar_met": bool(rows["c2"]["GiB_per_s"]["chunk"] > rows["c2"]["GiB_per_s"]["whole"])}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
