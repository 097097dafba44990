"""The .xz container on the MI355X: what the check kernel does per second, and what the number of blocks does to the decode rate.

    python tools/xz_rate.py [--quick] [--out profiles/xz.md]

(1) GB/s of gc_crc64_device on 1 GiB in HBM beside gc_crc32_device on the same bytes in the same run (wall time of the synchronous calls, median of five after a warm-up).
(2) The same content (256 MiB of `silesia-like`) written by this engine's encoder as 1, 16 and 256 blocks, decoded with input and output resident in HBM: content MB/s
    from gc_xz_timing (LZMA2 kernels, check kernel), median of five calls after a warm-up, with the launch counts of the last call.
Writes profiles/xz.md.  Needs the MI355X.  --quick: 64 MiB / 32 MiB and three calls (a check of the tool itself, not a measurement)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
MiB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xz.md"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    import oracle as O
    if not torch.cuda.is_available():
        sys.exit("needs the MI355X")
    pkg = g.load_package()
    calls = 3 if a.quick else 5

    # (1) the raw checksums
    n = (64 if a.quick else 1024) * MiB
    d = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    crc_rows = []
    for name, f in (("gc_crc64_device", pkg.crc64_device), ("gc_crc32_device", pkg.crc32_device)):
        ts = []
        for i in range(calls + 1):
            t0 = time.perf_counter(); v = f(d.data_ptr(), n); t = time.perf_counter() - t0
            if i:
                ts.append(t)
        crc_rows.append((name, v, n / 1e9 / statistics.median(ts)))
        print("%-16s %016x  %.1f GB/s" % (name, v, crc_rows[-1][2]), flush=True)
    del d

    # (2) decode rate against the number of blocks
    total = (32 if a.quick else 256) * MiB
    x = O.corpus("silesia-like", total)
    d_x = torch.from_numpy(x).to("cuda:0")
    dec = pkg.XzDecoder(device=0)
    rows = []
    for nb in (1, 16, 256):
        enc = pkg.XzEncoder(device=0, level=5, block_bytes=total // nb, check="crc64")
        cap = enc.compress_bound(total)
        d_c = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        size = enc.code_device(d_x.data_ptr(), total, d_c.data_ptr(), cap)
        enc_ms = enc.last_timing_ms()
        enc.close()
        blocks, nblocks, units, nu, tot = dec.scan(d_c[:size].cpu().numpy())
        assert nblocks == nb and tot == total
        d_o = torch.empty(total + 64, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ms = []
        for i in range(calls + 1):
            assert dec.code_device(d_c.data_ptr(), size, d_o.data_ptr(), total, blocks, nblocks, units, nu) == total
            if i:
                ms.append(dec.last_timing_ms())
        assert torch.equal(d_o[:total], d_x)
        l2 = statistics.median(m["lzma2"] for m in ms); ck = statistics.median(m["check"] for m in ms)
        rows.append((nb, nu, size, total / 1e3 / l2, total / 1e3 / ck, dec.launch_counts(), enc_ms))
        print("%4d blocks, %5d units: LZMA2 %.1f MB/s, check %.1f MB/s, launches %s" % (nb, nu, rows[-1][3], rows[-1][4], rows[-1][5]), flush=True)
        del d_c, d_o
    dec.close()

    lines = ["# The .xz container on the MI355X", "",
             "Written by `tools/xz_rate.py`%s (median of %d calls after a warm-up; data resident in HBM)." % (" --quick" if a.quick else "", calls), "",
             "## Checksums of %.0f MiB (wall time of the synchronous call)" % (n / MiB), "", "| entry point | value | GB/s |", "|---|---|---:|"]
    lines += ["| `%s` | %x | %.1f |" % r for r in crc_rows]
    lines += ["", "## Decode rate against the number of blocks (%.0f MiB of `silesia-like`, this engine's encoder at level 5, CRC-64)" % (total / MiB), "",
              "| blocks | units | compressed MB | LZMA2 kernels MB/s | check kernel MB/s | decode launch sets, units, check launches | encoder: LZMA2 ms, check ms |", "|---:|---:|---:|---:|---:|---|---|"]
    lines += ["| %d | %d | %.1f | %.1f | %.1f | %s | %.1f, %.2f |" % (nb, nu, size / 1e6, l2, ck, counts, e["lzma2"], e["check"]) for nb, nu, size, l2, ck, counts, e in rows]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
