"""Writes tests/golden/zstd_dict_sizes.json: the totals tests/test_zstd_dict.py asserts, measured under the emulator (it runs the kernels' own source and the
encoder is deterministic, so the device must give the same).  Needs the emulator library (tests/emu) and the reference library (oracle/_ref/libzstd_ref.so, for
the reference's level-3 totals with and without the dictionary).  Run from the repository root: python tests/golden/make_zstd_dict_sizes.py"""
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    import __graft_entry__ as g
    import oracle
    spec = importlib.util.spec_from_file_location("zstd_dict_cases", os.path.join(ROOT, "tests", "zstd_dict_cases.py"))
    D = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(D)
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "emu"), "-j8"], check=True, capture_output=True)
    if oracle.ref("zstd") is None:
        raise SystemExit("the reference library is not built (make -C oracle all)")
    B = D.K.Backend("emu", dict(lib_path=os.path.join(ROOT, "tests", "emu", "_build", "libgpucodec_emu.so")))
    sizes = D.measure_sizes(g.load_package(), B, D.Ref(oracle.ref("zstd")))
    with open(D.SIZES_PATH, "w") as f:
        json.dump(sizes, f, indent=1, sort_keys=True)
        f.write("\n")
    for name in D.SIZE_BATCHES:
        e = sizes[name]
        print("%s: %s  R0 %.4f  R1 %.4f" % (name, e, e["engine_plain"] / e["ref_plain"], e["engine_dict"] / e["ref_dict"]))
    print("sweep:", sizes["sweep"])


if __name__ == "__main__":
    main()
