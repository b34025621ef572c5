"""float64 reference of the SPPF block's two 1x1 convs with closed_loop_ref's bf16 bound.  TEST INFRASTRUCTURE (imported by
tests/test_sppf_cases.py and tests/test_gpu_sppf.py).  The bound, its constants and the float64 conv are closed_loop_ref's own: nothing is
copied here, and C_ACC's CPU floor on the fused kernel's inputs is asserted in tests/test_sppf_cases.py."""
import numpy as np
import torch

import closed_loop_ref as cl
import sppf_cases as sc


class _Conv1x1:
    name, k, stride, act = "sppf", 1, 1, 1


def nchw64(bits, H, W):
    """bf16 bit patterns [n, H*W, C] -> float64 [n, C, H, W]"""
    n, hw, c = bits.shape
    return np.ascontiguousarray(sc.to_f64(bits, sc.BF16).reshape(n, H, W, c).transpose(0, 3, 1, 2))


def conv64(x_bits, w, b, H, W):
    """-> (y = SiLU(b + sum w x), B = |b| + sum |w| |x|) in float64, [n, cout, H, W]"""
    wt = torch.from_numpy(np.asarray(w, dtype=np.float64))[:, :, None, None]
    p, a = cl.conv64(_Conv1x1, wt, torch.from_numpy(np.asarray(b, dtype=np.float64)), torch.from_numpy(nchw64(x_bits, H, W)))
    return cl._finish(_Conv1x1, p, a, None)


def bound_ratio(g_bits, y, bb, H, W):
    """closed_loop_ref's bf16 bound |g - y| <= 2^-8 |y| + C_ACC 2^-24 B -> (largest |g - y| / bound, largest (|g - y| - 2^-8 |y|)^+ / (2^-24 B))"""
    g = nchw64(g_bits, H, W)
    assert np.isfinite(g).all()
    err, rnd = np.abs(g - y), cl.EPS_BF16 * np.abs(y)
    bound = rnd + cl.C_ACC * cl.EPS_F32 * bb
    assert (bound > 0).all()
    return float((err / bound).max()), float((np.clip(err - rnd, 0, None) / (cl.EPS_F32 * bb)).max())
