"""Host-side helpers of tests/test_gpu_batch_sweep.py.  TEST INFRASTRUCTURE (imported by tests/ only; not a conftest); no GPU, no engine:
everything here works on kernel-name strings, slab records and detection arrays, and tests/test_batch_sweep_ref.py checks it on the CPU."""
import re

import numpy as np

from oracle_lib import det_fields_equal

TAIL_BOX_NOTE = "(computed in the Detect tail at surviving anchors)"


# ---------------------------------------------------------------------------------------------------
# what a launch table (zly_op_kernel_name of every op at one batch size) says
# ---------------------------------------------------------------------------------------------------
def c2f_shape(kernel_name):
    """'c2f_kernel<C=32,NW=16,bottleneck+cv2,13x26 tiles>' -> (C, NW or None, TH, TW); None for any other launch"""
    if not kernel_name.startswith("c2f_kernel<"):
        return None
    c = re.search(r"<C=(\d+)", kernel_name)
    nw = re.search(r",NW=(\d+),", kernel_name)
    t = re.search(r",(\d+)x(\d+) tiles>", kernel_name)
    assert c and t, kernel_name
    return int(c.group(1)), int(nw.group(1)) if nw else None, int(t.group(1)), int(t.group(2))


def pixel_tiles_per_wave(kernel_name):
    """(16-pixel MFMA tiles of one workgroup tile, NW) of a C = 32 launch that carries conv B's results to cv2 in registers: a wave carries
    ceil(tiles / NW) of them"""
    c, nw, th, tw = c2f_shape(kernel_name)
    assert c == 32 and nw, kernel_name
    return -(-th * tw // 16), nw


def carries_to_cv2(kernel_name):
    """the back half of a C = 32 block, or the whole block: conv B's epilogue hands its result to cv2 in registers"""
    return kernel_name.startswith("c2f_kernel<C=32") and "bottleneck+cv2" in kernel_name


def table_ids(tables):
    """{n: tuple of kernel names} -> ({n: id}, number of distinct tables); ids count up from 0 in order of first appearance over ascending n"""
    seen, out = {}, {}
    for n in sorted(tables):
        out[n] = seen.setdefault(tuple(tables[n]), len(seen))
    return out, len(seen)


def fused_block_names(op_names, tables):
    """{lead op of a fused C2f block: {n: its kernel name}} over every n at which that op launches c2f_kernel"""
    out = {}
    for n, kern in tables.items():
        assert len(kern) == len(op_names)
        for name, k in zip(op_names, kern):
            if k.startswith("c2f_kernel<"):
                out.setdefault(name, {})[n] = k
    return out


def count_launches(kern, prefix):
    return sum(k.startswith(prefix) for k in kern)


def tail_box_levels(op_names, kern):
    """Detect levels whose second box conv (model.22.cv2.L.1) the tail computes itself at this batch size"""
    by = {nm.split("+")[0]: k for nm, k in zip(op_names, kern)}
    return [l for l in range(3) if by.get(f"model.22.cv2.{l}.1") == TAIL_BOX_NOTE]


# ---------------------------------------------------------------------------------------------------
# slabs and detections
# ---------------------------------------------------------------------------------------------------
def slab_key(hdr, dets, with_tag=True):
    """what two runs of the same frame must agree on, as bytes: the header (without frame_tag where the frame sits at another position) and the kept
    detections with the wall-clock timestamp field zeroed"""
    d = np.array(dets, copy=True)
    d["timestamp"] = 0
    h = (int(hdr["n_kept"]), int(hdr["n_candidates"]), int(hdr["flags"])) + ((int(hdr["frame_tag"]),) if with_tag else ())
    return h, d.tobytes()


def same_slab(a, b):
    """header fields n_kept, n_candidates, frame_tag and det_fields_equal on the detections of two (header, detections) records"""
    (ha, da), (hb, db) = a, b
    return all(int(ha[k]) == int(hb[k]) for k in ("n_kept", "n_candidates", "frame_tag")) and det_fields_equal(da, db)


def same_result(a, b):
    """two (detections, n) results as detect / detect_batch / wait return them: the count and every field but the timestamp, bit for bit"""
    return int(a[1]) == int(b[1]) and det_fields_equal(a[0], b[0])


def matching_batch_sizes(result, entries):
    """batch sizes n whose table entry entries[n] (the frame's result inside a batch of n) equals `result`"""
    return [n for n in sorted(entries) if same_result(result, entries[n])]


def check_membership(results, table):
    """results: [(frame index, (detections, n))] of a pipelined run; table[frame][n] = that frame's result inside a batch of n.
    -> the batch sizes matched per result; raises AssertionError naming every result that equals none of ITS frame's entries"""
    matched, bad = [], []
    for i, (k, res) in enumerate(results):
        m = matching_batch_sizes(res, table[k])
        matched.append(m)
        if not m:
            other = sorted(j for j in table if j != k and matching_batch_sizes(res, table[j]))
            bad.append(f"result {i} of frame {k} ({int(res[1])} detections) equals no batch size's entry" +
                       (f"; it equals an entry of frame(s) {other}" if other else ""))
    assert not bad, "\n  ".join(["pipelined results outside the table:"] + bad)
    return matched
