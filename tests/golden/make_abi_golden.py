"""Writes tests/golden/reference_abi.json: the layout of the reference's zero_latency::Detection (src/common/types.h) and the values of
its zero_latency::ErrorCode (src/common/result.h), as the compiler sees them -- tests/cpp/abi_reference_probe.cpp built twice against
the reference's own headers and run.  tests/test_abi.py then checks include/zly.h against this record with the compiler, so the suite
needs no reference tree.  Re-run when the reference's headers change:
    python tests/golden/make_abi_golden.py --reference <reference checkout>"""
import argparse
import json
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def probe(reference: str) -> dict:
    src = os.path.join(ROOT, "tests", "cpp", "abi_reference_probe.cpp")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, defs in (("types", []), ("result", ["-DPROBE_RESULT"])):
            exe = os.path.join(tmp, name)
            subprocess.run(["g++", "-std=c++17", *defs, "-I", os.path.join(reference, "src", "common"), src, "-o", exe], check=True)
            out.update(json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True, help="root of a zero-latency-yolo checkout (the one holding src/common/types.h)")
    a = ap.parse_args()
    dst = os.path.join(ROOT, "tests", "golden", "reference_abi.json")
    with open(dst, "w") as f:
        json.dump(probe(a.reference), f, indent=1, sort_keys=True)
        f.write("\n")
    print(dst)
