#!/usr/bin/env python3
"""Record tests/golden/scatter_stable_sha256.json: SHA-256 of the compressed stream of every case of tests/scatter_cases.py, as ANOTHER
checkout of this repository compresses it -- the commit whose bytes are the yardstick of tests/test_scatter_stable.py.

    git worktree add ../parent <sha> && python ../parent/__graft_entry__.py          # build that commit (libraries + tests/emu)
    python tools/gen_scatter_golden.py --tree ../parent --emu [--jobs N]              # every case through that tree's CPU emulator
    python tools/gen_scatter_golden.py --tree ../parent --gpu                         # every case through that tree's library, on device 0

The case list is this tree's; the package, the emulator library and the corpus generators are --tree's.  The commit is read from
--tree's git (or given with --commit where the tree is an export without one).  Both modes merge into --out (default: the fixture's place
in this tree): a case recorded twice must hash the same (emulator bytes == device bytes), anything else is an error.  --only SUBSTRING
limits the run to the cases whose id contains it.  The frame-sized cases take the emulator minutes each."""
import argparse
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _one(arg):
    tree, case, emu = arg
    S = _load("scatter_cases", os.path.join(ROOT, "tests", "scatter_cases.py"))
    g = _load("graft_entry_of_tree", os.path.join(tree, "__graft_entry__.py"))
    O = g.load_oracle()
    kw = {"lib_path": os.path.join(tree, "tests", "emu", "_build", "libgpucodec_emu.so")} if emu else {"device": 0}
    return S.case_id(case), S.stream_sha256(g.load_package(), O.corpus, case, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="built checkout of the commit to record")
    ap.add_argument("--commit", default="", help="its full hash, where --tree has no git of its own")
    ap.add_argument("--emu", action="store_true")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "scatter_stable_sha256.json"))
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    commit = args.commit or subprocess.run(["git", "-C", tree, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    if args.emu == args.gpu or len(commit) != 40 or tree == ROOT:
        raise SystemExit("one of --emu / --gpu, a --tree other than this one, and its full commit hash")
    S = _load("scatter_cases", os.path.join(ROOT, "tests", "scatter_cases.py"))
    work = [(tree, c, args.emu) for c in S.cases() if args.only in S.case_id(c)]
    if args.emu and args.jobs > 1:
        from multiprocessing import Pool
        with Pool(args.jobs) as pool:
            got = pool.map(_one, sorted(work, key=lambda w: -w[1][3]), chunksize=1)
    else:
        got = [_one(w) for w in work]
    doc = {"_parent_commit": commit, "sha256": {}}
    if os.path.exists(args.out):
        doc = json.load(open(args.out))
        if doc["_parent_commit"] != commit:
            raise SystemExit("%s was recorded at %s" % (args.out, doc["_parent_commit"]))
    doc["_note"] = "SHA-256 of the compressed stream of each case of tests/scatter_cases.py (<codec>-<level>/<corpus>/<bytes>), recorded by tools/gen_scatter_golden.py at _parent_commit"
    for cid, h in got:
        if doc["sha256"].setdefault(cid, h) != h:
            raise SystemExit("case %s: %s here, %s in %s" % (cid, h, doc["sha256"][cid], args.out))
    doc["sha256"] = dict(sorted(doc["sha256"].items()))
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("%d cases hashed, %d in %s" % (len(got), len(doc["sha256"]), args.out))


if __name__ == "__main__":
    main()
