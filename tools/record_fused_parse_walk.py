#!/usr/bin/env python3
"""Records tests/golden/fused_parse_walk/<codec>.npz: the streams of tests/test_fused_parse_walk.py's inputs from an emulator build.
usage: python tools/record_fused_parse_walk.py --lib <checkout of the commit to record>/tests/emu/_build/libgpucodec_emu.so
The committed files were recorded from the emulator build of commit 3d52408, the parent of the change that walks the parse path per lane."""
import argparse, importlib.util, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
import __graft_entry__ as g
import oracle as O

ap = argparse.ArgumentParser()
ap.add_argument("--lib", required=True, help="libgpucodec_emu.so of the commit whose streams are recorded")
a = ap.parse_args()
spec = importlib.util.spec_from_file_location("fused_parse_walk_cases", os.path.join(ROOT, "tests", "test_fused_parse_walk.py"))
T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
pkg = g.load_package()
os.makedirs(T.GOLDEN, exist_ok=True)
for name in sorted(T.CODECS):
    streams, _ = T.encode_all(pkg, O, name, lib_path=os.path.abspath(a.lib))
    np.savez_compressed(os.path.join(T.GOLDEN, name + ".npz"), **streams)
    print(name, {k: int(v.size) for k, v in streams.items()})
