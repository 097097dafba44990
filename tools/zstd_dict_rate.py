#!/usr/bin/env python3
"""Batched zstd encoder and decoder with and without a raw-content dictionary -> appended to profiles/zstd_dict.md.

For 4096 items each of 4 KiB and of 128 KiB of text-zipf, resident in HBM, at level 3, with a 112 KiB dictionary (text-zipf of another seed) and without one:
  * the batch call: the four entries of gc_zstd_batch_timing (HIP events; finder, entropy stages, plan + emit, first kernel start -> last kernel end), mean / min / max
    of --repeats calls after one warm-up call of the same shape;
  * gc_zstd_set_dictionary itself: wall time around the call (it copies, digests and synchronises), same repeats;
  * the decode of both outputs in one gc_zstd_decompress_device call each: gc_zstd_decompress_timing (HIP events), same repeats.
--parent-lib PATH (a libgpucodec.so built from the parent commit) adds the one comparison that is a condition: the batch call WITHOUT a dictionary must not be slower
than the parent's.  Both libraries run in the same process on the same buffers, alternating call by call; the verdict allows the spread of the parent's own repeats
(this build's mean against the parent's slowest repeat) and nothing more.

Every size is measured by a child process of its own under a time limit; the first child that fails or runs out of time ends the run (nothing more is started on the
device).  The parent process never opens the GPU.  No rate is promised for the dictionary path.

    python tools/zstd_dict_rate.py [--out profiles/zstd_dict.md] [--items 4096] [--repeats 10] [--parent-lib PATH] [--limit 300]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4 << 10, 128 << 10)
DICT_BYTES = 112 << 10
CORPUS_CAP = 64 << 20           # text generated per size; items are cut from it at a fixed stride and overlap where 4096 of them do not fit side by side
MARK = "## Rates on the device"


def stats(v):
    return dict(mean=sum(v) / len(v), min=min(v), max=max(v))


def child(size, n_items, level, repeats, parent_lib):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import __graft_entry__ as g
    pkg, O = g.load_package(), g.load_oracle()
    corpus_bytes = min(CORPUS_CAP, n_items * size)
    x = O.corpus("text-zipf", corpus_bytes)
    dictionary = np.ascontiguousarray(O.corpus("text-zipf", DICT_BYTES, seed=20260922))
    stride = (corpus_bytes - size) // max(1, n_items - 1) if n_items > 1 else 0
    items = [(i * stride, size) for i in range(n_items)]
    content = n_items * size
    d_src = torch.from_numpy(x).to("cuda:0")
    table = (pkg.BatchItem * n_items)()
    for i, (o, n) in enumerate(items):
        table[i].src_off, table[i].src_size = o, n
    enc, dec = pkg.ZstdEncoder(device=0, level=level), pkg.ZstdDecoder(device=0)
    old = pkg.ZstdEncoder(device=0, level=level, lib_path=parent_lib) if parent_lib else None
    cap = enc.batch_bound([size] * n_items)
    d_dst = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    d_old = torch.empty(cap, dtype=torch.uint8, device="cuda:0") if old else None
    d_out = torch.empty(content + 64, dtype=torch.uint8, device="cuda:0")
    want = torch.cat([d_src[o:o + n] for o, n in items]) if content <= (1 << 30) else None
    torch.cuda.synchronize()

    def batch(e, dst):
        e.code_batch_device(d_src.data_ptr(), x.size, table, dst.data_ptr(), cap)
        _, total = e.finish_batch(n_items)
        return total, e.batch_timing_ms()

    def decode(total):
        frames, nf, stated = dec.scan(d_dst[:total].cpu().numpy())
        assert nf == n_items and stated == content
        ms = []
        for rep in range(repeats + 1):
            got = dec.code_device(d_dst.data_ptr(), total, d_out.data_ptr(), content, frames, nf)
            assert got == content
            if rep:
                ms.append(dec.last_timing_ms())
        ok = bool(torch.equal(d_out[:content], want)) if want is not None else None
        return stats(ms), ok

    out = dict(size=size, items=n_items, input_bytes=content, device=torch.cuda.get_device_name(0), repeats=repeats)
    # ---- without a dictionary; the parent's library alternating with this one
    batch(enc, d_dst)
    if old:
        batch(old, d_old)
    mine, theirs, total = [], [], 0
    for rep in range(repeats):
        total, ms = batch(enc, d_dst)
        mine.append(ms)
        if old:
            t_old, ms = batch(old, d_old)
            theirs.append(ms)
            assert t_old == total
    out["plain"] = dict(output_bytes=total, **{k: stats([m[k] for m in mine]) for k in enc.BATCH_KERNELS})
    if old:
        out["parent_plain"] = {k: stats([m[k] for m in theirs]) for k in enc.BATCH_KERNELS}
        out["same_bytes_as_parent"] = bool(torch.equal(d_dst[:total], d_old[:total]))
        old.close()
    out["plain"]["decode_ms"], out["plain"]["decode_ok"] = decode(total)
    # ---- set_dictionary itself
    wall = []
    for rep in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc.set_dictionary(dictionary)
        if rep:
            wall.append((time.perf_counter() - t0) * 1e3)
    out["set_dictionary_ms"] = stats(wall)
    dec.set_dictionary(dictionary)
    # ---- with the dictionary
    batch(enc, d_dst)
    mine = []
    for rep in range(repeats):
        total, ms = batch(enc, d_dst)
        mine.append(ms)
    out["dict"] = dict(output_bytes=total, **{k: stats([m[k] for m in mine]) for k in enc.BATCH_KERNELS})
    out["dict"]["decode_ms"], out["dict"]["decode_ok"] = decode(total)
    enc.close(); dec.close()
    print("RESULT " + json.dumps(out))
    bad = out["plain"]["decode_ok"] is False or out["dict"]["decode_ok"] is False or out.get("same_bytes_as_parent") is False
    return 1 if bad else 0


def fmt(s):
    return "%.3f (%.3f .. %.3f)" % (s["mean"], s["min"], s["max"])


def write(path, rows, note, parent_lib):
    head = ""
    if os.path.exists(path):
        head = open(path).read()
        if MARK in head:
            head = head[:head.index(MARK)]
    lines = [MARK, "",
             "Written by `tools/zstd_dict_rate.py`.  Level 3, items of text-zipf resident in HBM, dictionary: %d KiB of text-zipf of another seed.  Times in ms: mean (min .. max) of the" % (DICT_BYTES >> 10),
             "repeats after one warm-up call of the same shape.  Batch columns: `gc_zstd_batch_timing` (finder K1b, entropy stages, plan + emit, first kernel start -> last kernel end);",
             "decode: `gc_zstd_decompress_timing` of one call over all frames; set_dictionary: wall time around the call.  No rate is promised for the dictionary path.", ""]
    if rows:
        lines += ["Device: %s.  %d items per size, %d repeats." % (rows[0]["device"], rows[0]["items"], rows[0]["repeats"]), "",
                  "| item | dictionary | output | lz | entropy | frame | total | total GB/s | decode | decode GB/s | decoded right |", "|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            for key, label in (("plain", "none"), ("dict", "%d KiB" % (DICT_BYTES >> 10))):
                e = r[key]
                lines.append("| %d KiB | %s | %.1f MB | %s | %s | %s | %s | %.2f | %s | %.2f | %s |" % (
                    r["size"] >> 10, label, e["output_bytes"] / 1e6, fmt(e["lz"]), fmt(e["entropy"]), fmt(e["frame"]), fmt(e["total"]), r["input_bytes"] / e["total"]["mean"] / 1e6,
                    fmt(e["decode_ms"]), r["input_bytes"] / e["decode_ms"]["mean"] / 1e6, {True: "yes", False: "NO", None: "not compared"}[e["decode_ok"]]))
        lines += ["", "| item | set_dictionary ms |", "|---|---|"]
        lines += ["| %d KiB | %s |" % (r["size"] >> 10, fmt(r["set_dictionary_ms"])) for r in rows]
        if any("parent_plain" in r for r in rows):
            lines += ["", "### The batch call without a dictionary against the parent commit", "",
                      "Both libraries in one process on the same buffers, alternating call by call (`--parent-lib`).  The condition: this build's mean is no slower than the parent's",
                      "slowest repeat -- the parent's own run-to-run spread and nothing more.", "",
                      "| item | parent total | this build total | parent lz | this build lz | same bytes | verdict |", "|---|---|---|---|---|---|---|"]
            for r in rows:
                if "parent_plain" in r:
                    p, m = r["parent_plain"], r["plain"]
                    ok = m["total"]["mean"] <= p["total"]["max"]
                    lines.append("| %d KiB | %s | %s | %s | %s | %s | %s |" % (r["size"] >> 10, fmt(p["total"]), fmt(m["total"]), fmt(p["lz"]), fmt(m["lz"]),
                                                                         "yes" if r["same_bytes_as_parent"] else "NO", "not slower" if ok else "SLOWER"))
        elif not parent_lib:
            lines += ["", "The comparison with the parent commit was not measured in this run (no `--parent-lib`)."]
    else:
        lines += ["not measured"]
    if note:
        lines += ["", note]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write(head.rstrip("\n") + ("\n\n" if head.strip() else "") + "\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zstd_dict.md"))
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--parent-lib", default="", help="libgpucodec.so of the parent commit, for the no-dictionary comparison")
    ap.add_argument("--limit", type=int, default=300, help="seconds a size may take")
    ap.add_argument("--json", default="", help="also write the raw results here")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.items, a.level, a.repeats, a.parent_lib)
    rows, note = [], ""
    for size in SIZES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(size), "--items", str(a.items), "--level", str(a.level),
               "--repeats", str(a.repeats)] + (["--parent-lib", os.path.abspath(a.parent_lib)] if a.parent_lib else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if got:
            rows.append(json.loads(got[-1][7:]))
            print(got[-1], flush=True)
        if r.returncode != 0 or not got:
            note = "The run ended at %d KiB items: exit status %d.  %s" % (size >> 10, r.returncode, (r.stderr or "").strip().splitlines()[-1] if (r.stderr or "").strip() else "")
            print(note, flush=True)
            break                                          # nothing more is started on the device
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)
    write(a.out, rows, note, a.parent_lib)
    return 1 if note else 0


if __name__ == "__main__":
    sys.exit(main())
