// head_skip.h -- the Detect tail's early-out bound (kernels_head.hip: HeadArgs::skip_logit), host arithmetic only: no HIP dependency, so that
// tests/cpp/test_head_skip.cpp compiles it with the host compiler and tests/test_head_skip.py scans the fp32 logits below it.
#pragma once
#include <math.h>

namespace zly {

// The class logit below which NO score can reach conf_thr, whichever of the tail's two arithmetics computes it:
//     score = fl(1 / fl(1 + e')),   e' = the computed exp(-z) = e (1 + d),  |d| <= 2^-18
// (fp32 engine: expf and an IEEE divide; bf16 engine: v_exp_f32 of the rounded product z * log2(e), v_rcp_f32, 1 ulp each).
// fl(1 + e') >= (1 + e')(1 - 2^-24), and the quotient / reciprocal is within one ulp, i.e. within 2^-23 relative.  So
//     score >= thr   only if   1 + e' <= (1 + 2^-23) / (thr (1 - 2^-24))   i.e.   e' <= (1 - thr) / thr + 3 * 2^-24 / thr   (to first order).
// The bound is  -log((1 - thr) / thr + C * 2^-24) - 1e-2  with C = 4:
//   * thr near 1: (1 - thr) / thr is itself a few units of 2^-24 and the ABSOLUTE roundings of 1 + e' and of the quotient decide -- the C
//     term (3 / thr <= 3.0000004 there, against C e^0.01 = 4.04).  logit(thr) - 1e-2 alone is wrong from thr = 1 - 34 * 2^-24 up: at
//     thr = 1 - 2^-23 the lowest passing logit is 15.54, logit(thr) - 1e-2 is 15.93;
//   * elsewhere the errors are RELATIVE to e (d above, and 3 * 2^-24 / thr against (1 - thr) / thr), and the 1e-2 covers them: one per cent
//     of e, against 2^-18 + 3 * 2^-24 / (1 - thr) < 0.01 wherever 1 - thr > 2e-5.  At thr = 0.5 the C term moves the bound by 2.4e-7.
//   * thr >= 1 is no special case: (1 - thr) / thr = 0 leaves -log(C 2^-24) - 1e-2 = 15.24, and a score of 1.0f needs e' <= 2^-24, z >= 16.6.
// thr <= 0 keeps everything (and a class of score exactly 0 is refused by cls >= 0, not by the threshold).
inline float head_skip_logit(float conf_thr)
{
    const double C = 4.0, U = 5.9604644775390625e-8;      // 2^-24
    if (!(conf_thr > 0.0f)) return -3.0e38f;
    const double thr = conf_thr < 1.0f ? (double)conf_thr : 1.0;
    return (float)(-log((1.0 - thr) / thr + C * U) - 1e-2);
}

}  // namespace zly
