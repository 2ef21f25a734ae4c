// crf_exact_div.h -- the correctly rounded fp32 quotient through one reciprocal per denominator, and its per-voxel guard,
// as the Pearson-type kernels use them (crf_device.h includes this header).  Plain C++, usable from host code
// (tests/native/division_edges.cpp evaluates both on vectors at the guard's edges against the plain division).
// Compile with -ffp-contract=off: every operation below is one IEEE operation, fmaf included.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define CRF_HDI __host__ __device__ __forceinline__
#else
#define CRF_HDI inline
#endif

namespace crf {

// Correctly rounded fp32 quotients a/b for MANY numerators and ONE denominator (the voxel's standard deviation) without
// the ~10-instruction IEEE division expansion per element: with rcp = RN(1/b) (one true division),
//     q0 = RN(a * rcp);  rem = fma(-q0, b, a) (exact);  q = fma(rem, rcp, q0)
// is the correctly rounded a/b (Markstein's theorem; checked against `/` on 2.4e9 operand pairs including every
// significand of b) PROVIDED rem is exactly representable, i.e. no underflow: |a| >= 2^-100 or a == 0, b in
// [2^-60, 2^60].  In the Pearson tail a = y_e - mean: a non-zero difference of two floats is at least half an ulp of
// the mean, so |mean| >= 2^-70 guarantees the bound on every a.  exact_div_guard() is that per-voxel test; when it
// fails for any lane of the wave the kernels take the plain-division path.
CRF_HDI bool exact_div_guard(float mean, float sd) {
    return fabsf(mean) >= 0x1p-70f && sd >= 0x1p-60f && sd <= 0x1p60f;  // false for NaN, 0, inf, tiny
}
CRF_HDI float exact_div(float a, float b, float rcp) {
    const float q0 = a * rcp;
    const float rem = fmaf(-q0, b, a);
    return fmaf(rem, rcp, q0);
}

}  // namespace crf
