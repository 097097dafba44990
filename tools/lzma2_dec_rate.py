"""What one wave of gfx950 does with LZMA's decode loop, and from how many units the device is ahead of one host thread.

    python tools/lzma2_dec_rate.py [--quick] [--out profiles/lzma2_dec.md]

On the GPU, for (a) one unit of 8 MiB content, (b) 64 and (c) 1 024 units of 1 MiB, each on `text-zipf` and `silesia-like`, and (d) the FLZMA2 level-5 stream of
211.9 MB `silesia-like` written as 16 MiB shards (the level's grain): content MB/s from gc_lzma2_decompress_timing -- the median of at least five calls after a warm-up,
compressed input and output resident in HBM -- beside the reference's Lzma2Dec.c (oracle ref_lzma2_decode) on ONE host thread on the same stream on the same box.
Writes the figures, with the kernels' register / LDS numbers and the waves per CU they give, to profiles/lzma2_dec.md.  Needs the MI355X and oracle/_ref.
--quick: 64 MiB for (d) and three calls (a check of the tool itself, not a measurement)."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
MiB = 1 << 20


def kernel_resources(g):
    """VGPR / SGPR / LDS / scratch of the two kernel instances: hipcc's resource remarks for gc_lzma2_frame.hip (the unit that includes gc_lzma2_dec.h)."""
    csrc = os.path.join(ROOT, "7-zip-zstd_amd", "csrc")
    cmd = [g._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "gc_lzma2_frame.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    out, cur = {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            cur = m.group(1) if m.group(1).startswith("gc_lzma2_dec_kernel") else None
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|AGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            out.setdefault(cur, {})[m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lzma2_dec.md"))
    ap.add_argument("--no-resources", action="store_true", help="skip the hipcc run for the register / LDS figures")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    import oracle as O
    if not torch.cuda.is_available():
        sys.exit("needs the MI355X")
    if O.ref("flzma2") is None:
        sys.exit("needs oracle/_ref (the reference's Lzma2Dec.c for the host column)")
    pkg = g.load_package()
    dec = pkg.Lzma2Decoder(device=0)
    calls = 3 if a.quick else 5
    rows = []

    def measure(tag, comp, prop, x):
        comp = np.ascontiguousarray(comp)
        units, nu, total, used, ended = dec.scan(comp)
        assert ended and total == x.size
        d_src = torch.from_numpy(comp).to("cuda:0")
        d_out = torch.empty(total + 64, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ms = []
        for i in range(calls + 1):                                # the first call warms up
            assert dec.code_device(d_src.data_ptr(), used, d_out.data_ptr(), total, prop, units, nu) == total
            if i:
                ms.append(dec.last_timing_ms())
        assert torch.equal(d_out[:total].cpu(), torch.from_numpy(x)), tag
        hs = []
        for i in range(4):                                        # the host thread alike: a warm-up, then the median of three
            t0 = time.perf_counter()
            y = O.ref_lzma2_decode(comp, x.size, prop)
            if i:
                hs.append(time.perf_counter() - t0)
        host = statistics.median(hs)
        assert y.tobytes() == x.tobytes()
        gpu = statistics.median(ms) / 1e3
        rows.append((tag, nu, x.size, comp.size, x.size / 1e6 / gpu, x.size / 1e6 / host))
        print("%-44s units %5d  GPU %9.1f MB/s  one host thread %7.1f MB/s" % (tag, nu, rows[-1][4], rows[-1][5]), flush=True)

    for kind in ("text-zipf", "silesia-like"):
        x = O.corpus(kind, 8 * MiB)
        c, prop = O.ref_fl2_compress(x, 5)
        measure("(a) one unit of 8 MiB, %s" % kind, c, prop, x)
        x1 = O.corpus(kind, MiB)
        c1, prop = O.ref_fl2_compress(x1, 5)
        for tag, k in (("(b) 64", 64), ("(c) 1 024", 1024)):
            measure("%s units of 1 MiB, %s" % (tag, kind), np.concatenate([c1[:-1]] * k + [np.zeros(1, np.uint8)]), prop, np.tile(x1, k))
    n = 64 * MiB if a.quick else 211_900_000
    x = O.corpus("silesia-like", n)
    enc = pkg.Flzma2Encoder(device=0, level=5)
    grain = pkg.codec_grain("flzma2", 5)
    c = np.concatenate([enc.code(x[i:i + grain], flags=enc.NO_END_MARK) for i in range(0, n, grain)] + [np.zeros(1, np.uint8)])
    prop = enc.coder_props()[0]
    enc.close()
    measure("(d) FLZMA2-L5 of %.1f MB silesia-like, %d MiB shards" % (n / 1e6, grain // MiB), c, prop, x)
    dec.close()

    res = {} if a.no_resources else kernel_resources(g)
    lines = ["# LZMA2 decoder: one wave per unit on the MI355X", "",
             "Written by `tools/lzma2_dec_rate.py`%s.  Content MB/s from `gc_lzma2_decompress_timing` (median of %d calls after a warm-up; input and output resident in HBM) beside"
             % (" --quick" if a.quick else "", calls),
             "the reference's `Lzma2Dec.c` on one host thread, same stream, same box.  Streams (a)-(c): the reference's Fast-LZMA2 level 5; (d): this engine's encoder.", "",
             "| case | units | content MB | compressed MB | GPU MB/s | one host thread MB/s | GPU / host |", "|---|---:|---:|---:|---:|---:|---:|"]
    for tag, nu, size, csize, gm, hm in rows:
        lines.append("| %s | %d | %.1f | %.1f | %.1f | %.1f | %.2f |" % (tag, nu, size / 1e6, csize / 1e6, gm, hm, gm / hm))
    one = {r[0].split(", ")[-1]: r for r in rows if r[0].startswith("(a)")}
    lines += ["", "Per wave (case a): " + "; ".join("%s %.1f MB/s against %.1f MB/s of the host thread, so the device is ahead from %d units" % (k, r[4], r[5], int(np.ceil(r[5] / r[4])))
                                                   for k, r in one.items()) + " (while every unit has a wave of its own).", ""]
    lines += ["## Kernel resources (hipcc --offload-arch=gfx950 -O3)", "", "| kernel | VGPRs | SGPRs | SGPRs spilled to VGPR lanes | LDS bytes | scratch bytes / lane | waves per CU (LDS, 160 KiB) |", "|---|---:|---:|---:|---:|---:|---:|"]
    for k in sorted(res):
        r = res[k]
        lds = r.get("LDS Size", 0)
        lines.append("| %s | %d | %d | %d | %d | %d | %d |" % (k, r.get("VGPRs", -1), r.get("TotalSGPRs", -1), r.get("SGPRs Spill", -1), lds, r.get("ScratchSize", -1), (160 * 1024) // lds if lds else 0))
    if not res:
        lines.append("| (not collected) | | | | | | |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
