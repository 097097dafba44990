#!/usr/bin/env python3
"""Records tests/golden/seq_rounds/streams.npz: the streams of tests/test_seq_rounds.py's cases from an emulator build.
usage: python tools/record_seq_rounds.py --lib <checkout of the commit to record>/tests/emu/_build/libgpucodec_emu.so
Per case: sha_<name> = SHA-256 of the whole stream, tail_<name> = the stream behind its first 128 KiB (block 0 of every case is 128 KiB of random bytes, stored raw:
the file would be 10 MB with them).  The committed file was recorded from the emulator build of commit eeb9b4c, the parent of the change that gives a thread of the
sequence stage several sequences per round."""
import argparse, hashlib, importlib.util, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
import __graft_entry__ as g

ap = argparse.ArgumentParser()
ap.add_argument("--lib", required=True, help="libgpucodec_emu.so of the commit whose streams are recorded")
a = ap.parse_args()
spec = importlib.util.spec_from_file_location("seq_rounds_cases", os.path.join(ROOT, "tests", "test_seq_rounds.py"))
T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
pkg = g.load_package()
os.makedirs(os.path.dirname(T.GOLDEN), exist_ok=True)
out = {}
for name in sorted(T.CASES):
    s = T.emu_stream(pkg, os.path.abspath(a.lib), name)
    out["sha_" + name] = np.frombuffer(hashlib.sha256(s).digest(), dtype=np.uint8)
    out["tail_" + name] = np.frombuffer(s[T.BLOCK:], dtype=np.uint8)
    print(name, len(s), len(s) - T.BLOCK)
np.savez_compressed(T.GOLDEN, **out)
print("%d cases, %d bytes" % (len(T.CASES), os.path.getsize(T.GOLDEN)))
