"""Register budget of the c2f_kernel instantiations that the default plans select (YOLOv8n 416 / 640: model.2, model.4 front and back, model.15;
YOLOv8-s 640: model.2).  The 16-wave builds sit at the 128-VGPR cap, and what keeps them out of scratch reaches the compiler only indirectly
(kernels_pair.hip: a compiler-level fence that keeps conv B's weight fragments in LDS, opaque copies of the lane indices per phase), so a compiler
or source change can undo it without any other sign.  This compiles kernels_pair.hip for the device with the Makefile's flags and reads the
compiler's own resource remarks: no scratch, and the waves per SIMD a workgroup of that size needs (4 for 16 waves, 2 for 8).  No GPU is used."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# <C, MODE, NW, NLD, NK1> as mangled template arguments -> (what runs it, waves per SIMD it needs)
DEFAULT_PLAN = {
    "ILi16ELi3ELi16ELi4ELi1EE": ("model.2 of YOLOv8n", 4),
    "ILi32ELi1ELi8ELi4ELi2EE": ("model.4 front half of YOLOv8n", 2),
    "ILi32ELi2ELi16ELi4ELi1EE": ("model.4 back half of YOLOv8n", 4),
    "ILi32ELi3ELi16ELi4ELi6EE": ("model.15 of YOLOv8n", 4),
    "ILi32ELi3ELi16ELi4ELi2EE": ("model.2 of YOLOv8-s", 4),
}


def test_default_plan_c2f_kernels_have_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Iinclude", "-Izero-latency-yolo_amd/csrc", "--cuda-device-only", "-c",
           "zero-latency-yolo_amd/csrc/kernels_pair.hip", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: .*?(Function Name|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = usage.setdefault(m.group(2), {})
        elif cur is not None:
            cur.setdefault(m.group(1), int(m.group(2)))
    for args, (what, need) in DEFAULT_PLAN.items():
        hit = [u for name, u in usage.items() if "c2f_kernel" + args in name]
        assert len(hit) == 1, (what, args, len(hit))
        u = hit[0]
        print(what, u)
        assert u["ScratchSize [bytes/lane]"] == 0, (what, u)
        assert u["Occupancy [waves/SIMD]"] >= need, (what, u)
