#!/usr/bin/env python3
"""Record tests/golden/mf_keys_sha256.json: SHA-256 of the compressed stream of every case of tests/mf_keys_cases.py, as the EMULATOR build of another checkout of
this repository compresses it under frames of two blocks (test hook GC_FRAME_BLOCKS) -- the commit whose bytes are the yardstick of tests/test_mf_keys.py.

    git worktree add ../parent <sha> && python ../parent/__graft_entry__.py          # build that commit (libraries + tests/emu)
    python tools/record_mf_keys.py --tree ../parent [--jobs N]

The case list and the inputs are this tree's; the package and the emulator library are --tree's.  The commit is read from --tree's git (or given with --commit where
the tree is an export without one).  Merges into --out: a case recorded twice must hash the same.  --only SUBSTRING limits the run."""
import argparse
import importlib.util
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _one(arg):
    tree, case = arg
    K = _load("mf_keys_cases", os.path.join(ROOT, "tests", "mf_keys_cases.py"))
    g = _load("graft_entry_of_tree", os.path.join(tree, "__graft_entry__.py"))
    os.environ["GC_FRAME_BLOCKS"] = str(K.FRAME_BLOCKS)
    return K.case_id(case), K.stream_sha256(g.load_package(), case, lib_path=os.path.join(tree, "tests", "emu", "_build", "libgpucodec_emu.so"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="built checkout of the commit to record")
    ap.add_argument("--commit", default="", help="its full hash, where --tree has no git of its own")
    ap.add_argument("--only", default="")
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mf_keys_sha256.json"))
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    commit = args.commit or subprocess.run(["git", "-C", tree, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    if len(commit) != 40 or tree == ROOT:
        raise SystemExit("a --tree other than this one, and its full commit hash")
    K = _load("mf_keys_cases", os.path.join(ROOT, "tests", "mf_keys_cases.py"))
    work = [(tree, c) for c in K.cases() if args.only in K.case_id(c)]
    if args.jobs > 1:
        from multiprocessing import Pool
        with Pool(args.jobs) as pool:
            got = pool.map(_one, work, chunksize=1)
    else:
        got = [_one(w) for w in work]
    doc = {"_parent_commit": commit, "sha256": {}}
    if os.path.exists(args.out):
        doc = json.load(open(args.out))
        if doc["_parent_commit"] != commit:
            raise SystemExit("%s was recorded at %s" % (args.out, doc["_parent_commit"]))
    doc["_note"] = "SHA-256 of the compressed stream of each case of tests/mf_keys_cases.py (<codec>-<level>/<name>) under GC_FRAME_BLOCKS=2, recorded by tools/record_mf_keys.py from the emulator build of _parent_commit"
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
