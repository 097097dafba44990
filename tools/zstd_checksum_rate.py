"""What the zstd content checksums (GC_OPT_ZSTD_CHECKSUM) cost on the MI355X: the hash kernel alone and beside the encoder.

    python tools/zstd_checksum_rate.py [--quick] [--parent-tree DIR] [--out profiles/zstd_checksum.md]

Steps, each a fresh child process under a time limit of its own; the first one that fails ends the run (what has been measured so far is still written):
  enc:<bytes>   zstd level 3 on the enwik9 stand-in (`text-zipf`) at 1 GB, 64 MiB and one 8 MiB frame, input and output resident in HBM: calls alternate between option
                off and option on; gc_zstd_checksum_timing and ms[5] of gc_zstd_last_timing (first kernel start -> last kernel end), medians after a warm-up pair
  xxh:<bytes>   gc_xxh64_device on 8 MiB and 256 MiB of the same text (one "frame": ONE workgroup), wall clock of the synchronous call, GB/s
  bench         bench.py --gpus 1 of this tree (option off) and of the parent commit's tree (--parent-tree, built there beforehand), three runs each, alternating
Without a GPU (or with --resources-only) the file holds the compiler's register / LDS figures and "not measured" for every rate.
--quick: 64 MiB in place of 1 GB and three calls per side (a check of the tool itself, not a measurement)."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
MiB = 1 << 20
KERNEL = "gc_zstd_xxh64_kernel"


def kernel_resources(g):
    """VGPR / SGPR / LDS / scratch of the hash kernel: hipcc's resource remarks for gc_zstd_frame.hip (the unit that includes gc_xxh64.h)."""
    csrc = os.path.join(ROOT, "7-zip-zstd_amd", "csrc")
    cmd = [g._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "gc_zstd_frame.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    out, cur = {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            cur = m.group(1) if m.group(1) == KERNEL else None
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|AGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur:
            out[m.group(1).split(" [")[0]] = int(m.group(2))
    return out


# ------------------------------------------------------------------------------------------------ steps (child processes)
def step_enc(n, calls):
    import torch
    import __graft_entry__ as g
    import oracle as O
    pkg = g.load_package()
    x = O.corpus("text-zipf", n)
    enc = pkg.ZstdEncoder(device=0, level=3)
    d_src = torch.from_numpy(x).to("cuda:0")
    cap = enc.compress_bound(n)
    d_dst = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    total = {0: [], 1: []}; hash_ms = []; size = {}
    for i in range(calls + 1):                                        # the first pair warms up
        for on in (0, 1):
            enc.set_option(enc.OPT_ZSTD_CHECKSUM, on)
            enc.code_device(d_src.data_ptr(), n, d_dst.data_ptr(), cap)
            size[on] = enc.finish()
            if i:
                total[on].append(enc.last_timing_ms()["total"])
                if on:
                    hash_ms.append(enc.checksum_ms())
    frames = -(-n // (64 * 128 * 1024))
    assert size[1] == size[0] + 4 * frames
    dec = pkg.ZstdDecoder(device=0)                                    # the checksummed stream verifies on the device
    fr, nf, tot = dec.scan(d_dst[:size[1]].cpu().numpy())
    d_out = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    assert nf == frames and dec.code_device(d_dst.data_ptr(), size[1], d_out.data_ptr(), n, fr, nf) == n and torch.equal(d_out[:n], d_src)
    dec.close(); enc.close()
    return {"bytes": n, "frames": frames, "off_ms": statistics.median(total[0]), "on_ms": statistics.median(total[1]), "hash_ms": statistics.median(hash_ms),
            "off_spread": [min(total[0]), max(total[0])], "on_spread": [min(total[1]), max(total[1])], "calls": calls}


def step_xxh(n, calls):
    import torch
    import __graft_entry__ as g
    import oracle as O
    pkg = g.load_package()
    x = O.corpus("text-zipf", n)
    d = torch.from_numpy(x).to("cuda:0")
    torch.cuda.synchronize()
    want = O.port().gco_xxh64(x.ctypes.data, n, 0)
    secs = []
    for i in range(calls + 1):
        t0 = time.perf_counter()
        got = pkg.xxh64_device(d.data_ptr(), n)
        if i:
            secs.append(time.perf_counter() - t0)
        assert got == want
    s = statistics.median(secs)
    return {"bytes": n, "ms": s * 1e3, "gbps": n / 1e9 / s, "calls": calls}


def step_bench(tree):
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"], capture_output=True, text=True, cwd=tree)
    if r.returncode != 0:
        raise RuntimeError("bench.py failed in %s:\n%s" % (tree, (r.stdout + r.stderr)[-2000:]))
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    return {"tree": tree, "value": json.loads(line)["value"]}


def run_step(spec, limit, quick):
    """one step in a fresh child under `limit` seconds; -> its result, or None (failed / timed out: the caller stops)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--step", spec] + (["--quick"] if quick else [])
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print("step %s: no result after %d s -- stopping" % (spec, limit), flush=True)
        return None
    if r.returncode != 0:
        print("step %s failed (exit %d) -- stopping\n%s" % (spec, r.returncode, (r.stdout + r.stderr)[-2000:]), flush=True)
        return None
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print("step %s: %s" % (spec, res), flush=True)
    return res


# ------------------------------------------------------------------------------------------------ report
def write_report(path, res, enc_rows, xxh_rows, bench_rows, quick):
    nm = "not measured"
    lines = ["# zstd content checksums: XXH64 per frame on the MI355X", "",
             "Written by `tools/zstd_checksum_rate.py`%s.  The hash kernel (`%s`, K0x) takes one workgroup of 320 threads per zstd frame: wave 0 runs the four accumulator"
             % (" --quick" if quick else "", KERNEL),
             "chains on lanes 0..3, waves 1..4 stage the next 8 KiB tile -- coalesced loads, the products `x * P2` into LDS.  It runs on a stream of its own beside the match",
             "finder and the entropy stages and joins in front of the plan kernel.", "",
             "## Kernel resources (hipcc --offload-arch=gfx950 -O3)", "", "| kernel | VGPRs | SGPRs | LDS bytes | scratch bytes / lane | waves / SIMD |", "|---|---:|---:|---:|---:|---:|"]
    lines.append("| %s | %d | %d | %d | %d | %d |" % (KERNEL, res.get("VGPRs", -1), res.get("TotalSGPRs", -1), res.get("LDS Size", -1), res.get("ScratchSize", -1), res.get("Occupancy", -1))
                 if res else "| %s | (not collected) | | | | |" % KERNEL)
    lines += ["", "## Beside the encoder (zstd level 3, `text-zipf`, input and output in HBM; calls alternate option off / on)", "",
              "| input | frames | hash kernel ms | first kernel -> last kernel, option off ms (min..max) | option on ms (min..max) | on - off ms |", "|---|---:|---:|---:|---:|---:|"]
    for tag, n in (("1 GB", 1_000_000_000), ("64 MiB", 64 * MiB), ("one 8 MiB frame", 8 * MiB)):
        r = enc_rows.get(n)
        lines.append("| %s | %d | %.3f | %.3f (%.3f..%.3f) | %.3f (%.3f..%.3f) | %+.3f |" % (tag, r["frames"], r["hash_ms"], r["off_ms"], r["off_spread"][0], r["off_spread"][1], r["on_ms"],
                                                                                      r["on_spread"][0], r["on_spread"][1], r["on_ms"] - r["off_ms"])
                     if r else "| %s | | %s | %s | %s | %s |" % (tag, nm, nm, nm, nm))
    lines += ["", "## `gc_xxh64_device` (one frame = one workgroup; wall clock of the synchronous call)", "", "| input | ms | GB/s |", "|---|---:|---:|"]
    for tag, n in (("8 MiB", 8 * MiB), ("256 MiB", 256 * MiB)):
        r = xxh_rows.get(n)
        lines.append("| %s | %.3f | %.3f |" % (tag, r["ms"], r["gbps"]) if r else "| %s | %s | %s |" % (tag, nm, nm))
    lines += ["", "## `bench.py --gpus 1` headline with the option off, against the parent commit (MB/s, runs alternating)", ""]
    if bench_rows:
        for name in ("parent", "this"):
            v = [b["value"] for b in bench_rows if b["name"] == name]
            lines.append("- %s: %s (min %.1f, max %.1f)" % (name, ", ".join("%.1f" % t for t in v), min(v), max(v)))
    else:
        lines.append(nm)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zstd_checksum.md"))
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit, for the bench.py comparison")
    ap.add_argument("--resources-only", action="store_true", help="no GPU steps: the compiler's figures and 'not measured'")
    ap.add_argument("--no-resources", action="store_true", help="skip the hipcc run for the register / LDS figures")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    calls = 3 if a.quick else 7
    if a.step:                                                        # child: one step, one JSON line
        kind, _, arg = a.step.partition(":")
        res = step_enc(int(arg), calls) if kind == "enc" else step_xxh(int(arg), calls) if kind == "xxh" else step_bench(arg)
        print(json.dumps(res), flush=True)
        return
    import __graft_entry__ as g
    res = {} if a.no_resources else kernel_resources(g)
    enc_rows, xxh_rows, bench_rows = {}, {}, []
    gpu = False
    if not a.resources_only:
        import torch
        gpu = torch.cuda.is_available()
    if gpu:
        big = 64 * MiB if a.quick else 1_000_000_000
        steps = [("enc:%d" % n, 420) for n in dict.fromkeys((8 * MiB, 64 * MiB, big))] + [("xxh:%d" % (8 * MiB), 120), ("xxh:%d" % (256 * MiB), 180)]
        ok = True
        for spec, limit in steps:
            r = run_step(spec, limit, a.quick)
            if r is None:
                ok = False
                break
            (enc_rows if spec.startswith("enc") else xxh_rows)[r["bytes"]] = r
        if ok and a.parent_tree:
            for i in range(3):
                for name, tree in (("parent", os.path.abspath(a.parent_tree)), ("this", ROOT)):
                    r = run_step("bench:" + tree, 600, a.quick) if ok else None
                    if r is None:
                        ok = False
                        break
                    r["name"] = name
                    bench_rows.append(r)
            if not ok:
                bench_rows = []
    write_report(a.out, res, enc_rows, xxh_rows, bench_rows, a.quick)


if __name__ == "__main__":
    main()
