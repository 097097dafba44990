#!/usr/bin/env python3
"""Batched zstd encoder against the loop of stream calls it replaces -> profiles/zstd_batch.md.

For 4096 items each of 4 KiB, 16 KiB, 64 KiB and 128 KiB of text-zipf, resident in HBM, at level 3:
  * the batch call, from HIP events (first kernel start -> last kernel end, mean of five after one warm-up);
  * the same items as 4096 stream calls (gc_zstd_compress_device + gc_zstd_finish) on the same context: wall time around the loop with a final synchronise.
The loop of stream calls is what the engine offered for this job before the batch calls existed: it is the baseline.

Every size is measured by a child process of its own under a time limit; the first child that fails or runs out of time ends the run (nothing more is started on
the device).  The parent never opens the GPU.  The figures replace everything above the line "## Compiler figures" of the output file; what stands from that line on
(the cross-compiled kernels' registers, LDS and scratch) is kept.

    python tools/zstd_batch_rate.py [--out profiles/zstd_batch.md] [--items 4096] [--limit 240]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4 << 10, 16 << 10, 64 << 10, 128 << 10)
CORPUS_CAP = 64 << 20           # text generated per size; items are cut from it at a fixed stride and overlap where 4096 of them do not fit side by side
KEEP_FROM = "## Compiler figures"


def child(size, n_items, level):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import __graft_entry__ as g
    pkg, O = g.load_package(), g.load_oracle()
    corpus_bytes = min(CORPUS_CAP, n_items * size)
    x = O.corpus("text-zipf", corpus_bytes)
    stride = (corpus_bytes - size) // max(1, n_items - 1) if n_items > 1 else 0
    items = [(i * stride, size) for i in range(n_items)]
    d_src = torch.from_numpy(x).to("cuda:0")
    enc = pkg.ZstdEncoder(device=0, level=level)
    cap = enc.batch_bound([size] * n_items)
    d_dst = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    table = (pkg.BatchItem * n_items)()
    for i, (o, n) in enumerate(items):
        table[i].src_off, table[i].src_size = o, n
    batch_ms, total = [], 0
    for rep in range(6):                                   # one warm-up (the workspace grows), five measured
        enc.code_batch_device(d_src.data_ptr(), x.size, table, d_dst.data_ptr(), cap)
        results, total = enc.finish_batch(n_items)
        if rep:
            batch_ms.append(enc.batch_timing_ms()["total"])
    first = d_dst[results[0].dst_off:results[0].dst_off + results[0].dst_size].cpu().numpy().tobytes()
    # the same items as stream calls on the same context
    one_cap = enc.compress_bound(size)
    d_one = torch.empty(one_cap, dtype=torch.uint8, device="cuda:0")
    stream_total = 0
    for rep in range(2):                                   # one warm-up loop, one measured
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stream_total = 0
        for o, n in items:
            enc.code_device(d_src.data_ptr() + o, n, d_one.data_ptr(), one_cap)
            stream_total += enc.finish()
        torch.cuda.synchronize()
        loop_ms = (time.perf_counter() - t0) * 1e3
    enc.code_device(d_src.data_ptr(), size, d_one.data_ptr(), one_cap)
    k = enc.finish()
    same = d_one[:k].cpu().numpy().tobytes() == first and stream_total == total
    out = dict(size=size, items=n_items, input_bytes=n_items * size, output_bytes=total, batch_ms=sum(batch_ms) / len(batch_ms), batch_ms_all=batch_ms, loop_ms=loop_ms,
               round_items=enc.batch_round_items(), same_bytes=bool(same), device=torch.cuda.get_device_name(0))
    enc.close()
    print("RESULT " + json.dumps(out))
    return 0 if same else 1


def write(path, rows, note):
    kept = ""
    for p in (path, os.path.join(ROOT, "profiles", "zstd_batch.md")):
        if os.path.exists(p):
            text = open(p).read()
            if KEEP_FROM in text:
                kept = text[text.index(KEEP_FROM):]
                break
    lines = ["# Batched zstd encoder: one launch set against a loop of stream calls", "",
             "Written by `tools/zstd_batch_rate.py`.  Level 3, items of text-zipf resident in HBM.  batch = HIP events, first kernel start to last kernel end, mean of five calls",
             "after one warm-up; loop = the same items as stream calls (`gc_zstd_compress_device` + `gc_zstd_finish`) on the same context, wall time with a final synchronise.",
             "The loop is the baseline: before the batch calls it was the only way to do this job.  No rate is promised.", ""]
    if rows:
        r0 = rows[0]
        lines += ["Device: %s.  R (items per round) = %d." % (r0["device"], r0["round_items"]), "",
                  "| item | items | input | output | batch ms | batch GB/s | loop ms | loop GB/s | loop / batch | same bytes |", "|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append("| %d KiB | %d | %.1f MB | %.1f MB | %.3f | %.2f | %.1f | %.3f | %.0f x | %s |" % (
                r["size"] >> 10, r["items"], r["input_bytes"] / 1e6, r["output_bytes"] / 1e6, r["batch_ms"], r["input_bytes"] / r["batch_ms"] / 1e6, r["loop_ms"],
                r["input_bytes"] / r["loop_ms"] / 1e6, r["loop_ms"] / r["batch_ms"], "yes" if r["same_bytes"] else "NO"))
        lines += ["", "Items of a size are cut from %d MiB of text at a fixed stride, so the larger sizes overlap; \"same bytes\": the totals of both ways agree and the first item's frame is" % (CORPUS_CAP >> 20),
                  "the stream call's."]
    else:
        lines += ["not measured"]
    if note:
        lines += ["", note]
    lines += ["", kept.rstrip("\n") if kept else KEEP_FROM + "\n\nnot recorded", ""]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zstd_batch.md"))
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a size may take")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.items, a.level)
    rows, note = [], ""
    for size in SIZES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(size), "--items", str(a.items), "--level", str(a.level)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if got:
            rows.append(json.loads(got[-1][7:]))
            print(got[-1], flush=True)
        if r.returncode != 0 or not got:
            note = "The run ended at %d KiB items: exit status %d.  %s" % (size >> 10, r.returncode, (r.stderr or "").strip().splitlines()[-1] if (r.stderr or "").strip() else "")
            print(note, flush=True)
            break                                          # nothing more is started on the device
    write(a.out, rows, note)
    return 1 if note else 0


if __name__ == "__main__":
    sys.exit(main())
