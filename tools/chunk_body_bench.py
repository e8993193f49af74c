#!/usr/bin/env python3
"""The aws-chunked body launch beside the signing launches it follows and a plain copy of the same
bytes (not the product benchmark: bench.py is untouched).  One process, profiler off,
device-resident data, 64 KiB chunks, CRC-32C trailer.  Three shapes out of one buffer: C2
(1,024 x 8 MiB), 8 x 8 MiB and one part of 1 GiB.  Per shape four items, alternated round by round
and timed with HIP events:
  * body    -- the body launch alone on ready signatures (s3h_chunk_plan_body);
  * trailer -- the trailer plan: chunk hashes, chains, CRCs, trailer kernel
               (s3h_chunk_plan_launch_trailer);
  * copy    -- a device-to-device copy of the parts' bytes into a second buffer (the runtime's
               memcpy through torch.Tensor.copy_): the same payload read and written once;
  * both    -- trailer + body queued together on the stream, nothing in between.

Checked before anything is recorded, and again after the timed rounds: for sampled parts the whole
body equals s3h_cpu_chunk_body over the same part and the device's signatures, checksum and trailer
signature; for every part the final line and the trailer text equal s3h_chunk_header_text +
s3h_chunk_trailer_text; the copy equals its source.

The bars, on C2: body <= trailer of the same run, and both <= 1.05 x (body + trailer).

    python tools/chunk_body_bench.py [--out profiles/chunk_body_c2.json]
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
KIND = "crc32c"
BAR = 1.05
ITEMS = ("body", "trailer", "copy", "both")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_body_c2.json"))
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--chunk-kib", type=int, default=64)
    ap.add_argument("--shapes", default="c2,8x8MiB,1x1GiB")
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
        parts, payload = len(m), int(m.sum())
        seeds = np.random.default_rng(parts).integers(0, 2**32, (parts, 8), dtype=np.uint32)
        d_seeds = torch.from_numpy(seeds.view(np.int32)).cuda()
        plan = s3.ChunkSignPlan(o, m, chunk, trailer=KIND)
        info = plan.body_info()
        geo = s3.chunk_body_geometry(m, chunk, KIND)
        blen, boff = geo["body_lengths"].astype(np.int64), geo["body_offsets"].astype(np.int64)
        if not (np.array_equal(info["body_lengths"], geo["body_lengths"]) and info["total"] == geo["total"]):
            sys.exit(f"{name}: the plan's body lengths differ from s3h_chunk_body_geometry -- nothing recorded")
        counts, first = plan.data_chunks_per_part.astype(np.int64), plan.signature_offsets.astype(np.int64)
        d_sig = torch.empty((plan.signatures, 8), dtype=torch.int32, device="cuda")
        d_val = torch.empty(parts, dtype=torch.int32, device="cuda")
        d_tsig = torch.empty((parts, 8), dtype=torch.int32, device="cuda")
        d_body = torch.empty(info["total"], dtype=torch.uint8, device="cuda")
        d_copy = torch.empty(payload, dtype=torch.uint8, device="cuda")
        src = data[:payload]  # (every shape's parts lie back to back from byte 0)
        tail = 84 + len(s3.chunk_trailer_text(KIND, np.zeros(1, dtype=np.uint32), np.zeros(8, dtype=np.uint32)))
        d_tail_at = torch.from_numpy((boff + blen - tail)[:, None] + np.arange(tail)[None, :]).cuda()

        def sign():
            plan.launch_trailer(data, ctx, d_seeds, d_sig, d_val, d_tsig)

        def frame():
            plan.body(data, d_sig, d_body, d_val, d_tsig)

        items = {"body": frame, "trailer": sign, "copy": lambda: d_copy.copy_(src, non_blocking=True),
                 "both": lambda: (sign(), frame())}

        def check(when):
            sig = d_sig.cpu().numpy().view(np.uint32)
            val = d_val.cpu().numpy().view(np.uint32)
            tsig = d_tsig.cpu().numpy().view(np.uint32)
            for p in samples:
                part = data[int(o[p]):int(o[p] + m[p])].cpu().numpy()
                want = s3.cpu_chunk_body([part], chunk, sig[first[p]:first[p] + counts[p] + 1], KIND, val[p:p + 1],
                                         tsig[p:p + 1])
                got = d_body[int(boff[p]):int(boff[p] + blen[p])].cpu().numpy()
                if not np.array_equal(got, want):
                    sys.exit(f"{name}: the body of part {p} differs from s3h_cpu_chunk_body {when} -- nothing recorded")
            tails = d_body[d_tail_at].cpu().numpy()
            for p in range(parts):
                text = s3.chunk_header_text(0, sig[first[p] + counts[p]]) + s3.chunk_trailer_text(KIND, val[p], tsig[p])
                if tails[p].tobytes() != text.encode():
                    sys.exit(f"{name}: the ending of part {p}'s body differs from the text functions {when}")
            if not torch.equal(d_copy, src):
                sys.exit(f"{name}: the copy differs from its source {when}")

        ms = {k: [] for k in ITEMS}
        for k in ("trailer", "body", "copy", "both"):  # warm-up; body reads trailer's outputs
            items[k]()
        plan.status()
        torch.cuda.synchronize()
        check("before timing")
        d_body.fill_(0)
        for _ in range(rounds):
            for k in ITEMS:
                ev0.record()
                items[k]()
                ev1.record()
                ev1.synchronize()
                ms[k].append(ev0.elapsed_time(ev1))
        plan.status()
        check("after timing")
        mean = {k: sum(v) / len(v) for k, v in ms.items()}
        gib = payload / 2**30
        row = {"parts": parts, "part_bytes": int(m[0]), "chunk_bytes": chunk, "payload_bytes": payload,
               "body_bytes": int(info["total"]), "body_over_payload": round(info["total"] / payload, 6),
               "items": int(info["items"]), "piece_bytes": int(info["piece_bytes"]), "grid": int(info["grid"]),
               "chunk_hash_kernel": plan.info()["kernel"],
               "launches": {k: len(v) for k, v in ms.items()},
               "ms_mean": {k: round(v, 4) for k, v in mean.items()},
               "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
               "payload_GiB_per_s": {k: round(gib / (mean[k] * 1e-3), 1) for k in ITEMS},
               "body_over_copy": round(mean["body"] / mean["copy"], 4),
               "body_over_trailer": round(mean["body"] / mean["trailer"], 4),
               "both_over_body_plus_trailer": round(mean["both"] / (mean["body"] + mean["trailer"]), 4),
               "checked_whole_bodies_of_parts": [int(p) for p in samples]}
        print(name, json.dumps(row, sort_keys=True), flush=True)
        plan.close()
        return row

    all_shapes = {"c2": lambda: shape("c2", offs, lens, args.rounds, (0, 511, 1023)),
                  "8x8MiB": lambda: shape("8x8MiB", offs[:8], lens[:8], args.rounds, (0, 7)),
                  "1x1GiB": lambda: shape("1x1GiB", [0], [1 << 30], 3, (0,))}
    rows = {k: all_shapes[k]() for k in args.shapes.split(",")}
    with open(os.path.join(ROOT, "s3client_amd", "kernel_isa_counts.json")) as f:
        isa = json.load(f)
    head = args.git_head
    if head is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        head = r.stdout.strip() if r.returncode == 0 else "unknown"
    doc = {"tool": "tools/chunk_body_bench.py", "device": torch.cuda.get_device_name(0),
           "library": os.path.relpath(_native.LIB_PATH, ROOT), "library_sha256": file_sha256(_native.LIB_PATH),
           "git_head": head,
           "kernel_code_hash": {k: isa["code_hash"].get(k)
                                for k in ("chunk-body", "chunk-trailer", "chunk-chain", "crc_segments", "crc_parts",
                                          "skew", "skewp", "skews")},
           "config": {"timing": "HIP events, one launch per item per round, items alternated",
                      "checksum": KIND, "copy": "torch.Tensor.copy_ between two device buffers",
                      "cpu_backend": s3.cpu_backend()},
           "shapes": rows,
           "bars": f"c2: body ms <= trailer ms of the same run; both ms <= {BAR} x (body ms + trailer ms)"}
    if "c2" in rows:
        doc["c2_body_over_copy"] = rows["c2"]["body_over_copy"]
        doc["c2_body_payload_GiB_per_s"] = rows["c2"]["payload_GiB_per_s"]["body"]
        doc["bars_met"] = {"body_le_trailer": bool(rows["c2"]["body_over_trailer"] <= 1.0),
                           "both_le_1.05_sum": bool(rows["c2"]["both_over_body_plus_trailer"] <= BAR)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
