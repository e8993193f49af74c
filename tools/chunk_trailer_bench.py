#!/usr/bin/env python3
"""SigV4 trailer signatures beside the two launches they are made of (not the product benchmark:
bench.py is untouched).  One process, profiler off, device-resident data, 64 KiB chunks.  Three
shapes out of one buffer: C2 (1,024 x 8 MiB), 8 x 8 MiB and one part of 1 GiB.  Per shape and per
trailing checksum (CRC-32C, CRC-32, CRC-64/NVME), alternated round by round and timed with HIP
events:
  * trailer -- the trailer plan: chunk hashes, chains, CRCs, trailer kernel
               (s3h_chunk_plan_launch_trailer);
  * chunk   -- the plain chunk plan: chunk hashes + chains (s3h_chunk_plan_launch);
  * crc     -- the CRC plan over the whole parts alone (s3h_crc_plan_launch / s3h_crc64nvme_...);
  * link    -- the trailer kernel alone on ready signatures and checksums (s3h_chunk_plan_trailer).

Checked before anything is recorded, and again after the timed rounds: the trailer plan's chunk
signatures equal the CPU chain's over the GPU's chunk digests, its checksums equal the CRC plan's
for every part and the CPU function's for sampled parts, and its trailer signatures -- and the
kernel-alone ones -- equal s3h_cpu_trailer_signatures for every part.

The one bar: on C2, for each checksum, trailer <= 1.05 x (chunk + crc) of the same run.

    python tools/chunk_trailer_bench.py [--out profiles/chunk_trailer_c2.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SECRET, DATE, TIMESTAMP, REGION, SERVICE = "wJalrXUtnFEMI/K7MDENG/bPxRfiCYEXAMPLEKEY", "20130524", "20130524T000000Z", "us-east-1", "s3"
KINDS = ("crc32c", "crc32", "crc64nvme")
BAR = 1.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_trailer_c2.json"))
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

    def shape(name, o, m, rounds, samples):
        o, m = np.asarray(o, dtype=np.uint64), np.asarray(m, dtype=np.uint64)
        parts = len(m)
        seeds = np.random.default_rng(parts).integers(0, 2**32, (parts, 8), dtype=np.uint32)
        d_seeds = torch.from_numpy(seeds.view(np.int32)).cuda()
        cplan = s3.ChunkSignPlan(o, m, chunk)
        counts = cplan.data_chunks_per_part
        ends = (cplan.signature_offsets + counts).astype(np.int64)  # row of each part's last signature
        # the CPU chain over the GPU's chunk digests: what every chunk signature is checked against
        co = np.concatenate([oo + np.arange(c, dtype=np.uint64) * np.uint64(chunk) for oo, c in zip(o, counts)])
        cl = np.concatenate([np.minimum(np.uint64(chunk), mm - np.arange(c, dtype=np.uint64) * np.uint64(chunk))
                             for mm, c in zip(m, counts)])
        d_dig = torch.empty((len(cl), 8), dtype=torch.int32, device="cuda")
        with s3.Plan(co, cl) as hplan:
            hplan.launch(data, d_dig)
            hplan.status()
        cpu_sig = s3.cpu_chunk_signatures(ctx, d_dig.cpu().numpy().view(np.uint32), counts, seeds)
        del d_dig
        d_sig = torch.empty((cplan.signatures, 8), dtype=torch.int32, device="cuda")
        d_sig_t = torch.empty((cplan.signatures, 8), dtype=torch.int32, device="cuda")
        raw = {p: data[int(o[p]):int(o[p] + m[p])].cpu().numpy() for p in samples}
        rows = {}
        for kind in KINDS:
            wide = kind == "crc64nvme"
            vt, vn = (torch.int64, np.uint64) if wide else (torch.int32, np.uint32)
            tplan = s3.ChunkSignPlan(o, m, chunk, trailer=kind)
            rplan = s3.Crc64Plan(o, m) if wide else s3.CrcPlan(o, m, algo=kind)
            d_val, d_crc = (torch.empty(parts, dtype=vt, device="cuda") for _ in range(2))
            d_tsig, d_link = (torch.empty((parts, 8), dtype=torch.int32, device="cuda") for _ in range(2))
            items = {"trailer": lambda: tplan.launch_trailer(data, ctx, d_seeds, d_sig_t, d_val, d_tsig),
                     "chunk": lambda: cplan.launch(data, ctx, d_seeds, d_sig),
                     "crc": lambda: rplan.launch(data, d_crc),
                     "link": lambda: tplan.trailer(ctx, d_sig, d_crc, d_link)}

            def check(when):
                sig_t = d_sig_t.cpu().numpy().view(np.uint32)
                if not (np.array_equal(sig_t, cpu_sig) and np.array_equal(d_sig.cpu().numpy().view(np.uint32), cpu_sig)):
                    sys.exit(f"{name} {kind}: chunk signatures differ from the CPU chain {when} -- nothing recorded")
                vals = d_val.cpu().numpy().view(vn)
                if not np.array_equal(vals, d_crc.cpu().numpy().view(vn)):
                    sys.exit(f"{name} {kind}: the trailer plan's checksums differ from the CRC plan's {when}")
                for p in samples:
                    want = s3.crc64(raw[p]) if wide else s3.crc(raw[p], kind)
                    if int(vals[p]) != want:
                        sys.exit(f"{name} {kind}: checksum of part {p} differs from the CPU function {when}")
                cpu_t = s3.cpu_trailer_signatures(ctx, kind, vals, cpu_sig[ends])
                for buf, what in ((d_tsig, "trailer plan"), (d_link, "trailer kernel alone")):
                    if not np.array_equal(buf.cpu().numpy().view(np.uint32), cpu_t):
                        sys.exit(f"{name} {kind}: {what} signatures differ from the CPU link {when}")

            ms = {k: [] for k in items}
            for k in ("trailer", "chunk", "crc", "link"):  # warm-up; link reads chunk's and crc's outputs
                items[k]()
            tplan.status(), cplan.status()
            torch.cuda.synchronize()
            check("before timing")
            for _ in range(rounds):
                for k, fn in items.items():
                    ev0.record()
                    fn()
                    ev1.record()
                    ev1.synchronize()
                    ms[k].append(ev0.elapsed_time(ev1))
            tplan.status(), cplan.status()
            check("after timing")
            mean = {k: sum(v) / len(v) for k, v in ms.items()}
            gib = float(m.sum()) / 2**30
            rows[kind] = {"launches": {k: len(v) for k, v in ms.items()},
                          "ms_mean": {k: round(v, 4) for k, v in mean.items()},
                          "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
                          "GiB_per_s": {k: round(gib / (mean[k] * 1e-3), 1) for k in ("trailer", "chunk", "crc")},
                          "trailer_over_chunk_plus_crc": round(mean["trailer"] / (mean["chunk"] + mean["crc"]), 4),
                          "link_us": round(mean["link"] * 1e3, 2),
                          "crc_segment_bytes": int(rplan.info()["segment_bytes"])}
            print(name, kind, json.dumps(rows[kind], sort_keys=True), flush=True)
            tplan.close()
            rplan.close()
        row = {"parts": parts, "part_bytes": int(m[0]), "chunk_bytes": chunk, "data_chunks": int(len(cl)),
               "signatures": int(cplan.signatures), "max_chunks_per_part": int(counts.max()),
               "chunk_hash_kernel": cplan.info()["kernel"], "checksums": rows,
               "checked_against_cpu_crc_parts": [int(p) for p in samples]}
        cplan.close()
        return row

    rows = {"c2": shape("c2", offs, lens, args.rounds, (0, 511, 1023)),
            "8x8MiB": shape("8x8MiB", offs[:8], lens[:8], args.rounds, (0, 7)),
            "1x1GiB": shape("1x1GiB", [0], [1 << 30], 3, (0,))}
    with open(os.path.join(ROOT, "s3client_amd", "kernel_isa_counts.json")) as f:
        isa = json.load(f)
    head = args.git_head
    if head is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        head = r.stdout.strip() if r.returncode == 0 else "unknown"
    ratios = {k: rows["c2"]["checksums"][k]["trailer_over_chunk_plus_crc"] for k in KINDS}
    doc = {"tool": "tools/chunk_trailer_bench.py", "device": torch.cuda.get_device_name(0),
           "library_sha256": file_sha256(_native.LIB_PATH), "git_head": head,
           "kernel_code_hash": {k: isa["code_hash"].get(k)
                                for k in ("chunk-trailer", "chunk-chain", "crc_segments", "crc_parts",
                                          "crc64_segments", "crc64_parts", "skew", "skewp", "skews")},
           "config": {"timing": "HIP events, one launch per item per round, items alternated",
                      "prefix_bytes": 66 + len(REGION) + len(SERVICE), "cpu_backend": s3.cpu_backend()},
           "shapes": rows,
           "bar": f"c2, each checksum: trailer ms <= {BAR} x (chunk ms + crc ms) of the same run",
           "c2_trailer_over_chunk_plus_crc": ratios,
           "bar_met": bool(all(v <= BAR for v in ratios.values()))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
