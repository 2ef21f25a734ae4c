// crf_binned_bins.h -- the bin of one sample of binned mutual information, as the binned kernels compute it on the query
// side.  Plain C++, usable from host code (tests/native/narrow_bins.cpp evaluates it for every code of the narrow member
// formats against the reference's lines written out step by step).
//
// A sample y becomes  q = (y - min) / (max - min)  (CorrelationCalculator.cpp:1061-1062) and then the bin
// clamp(int(double(q) * numBins), 0, numBins - 1)  (MutualInformation.cpp:64-67); a sample whose q is NaN is skipped.
// Two forms of q, which the launchers choose between per evaluation (range = max - min is the same for every sample):
//   division     q = d / range,  d = y - min;  the sample counts iff q is not NaN
//   reciprocal   rcp = RN(1 / range) once;  q0 = RN(d * rcp);  q = fma(fma(-q0, range, d), rcp, q0);  counts iff d == d
// The reciprocal form is the correctly rounded d / range whenever the remainder is exact (Markstein; crf_exact_div.h:
// exact_div).  Where it is not -- |d| < 2^-100, or a quotient that leaves the normal range -- the quotient is below 2^-40
// or infinite either way and lands in the same bin (0) as the division's; for d = +-inf (or an overflowing q0) the chain
// yields NaN where the division yields +-inf: both convert to bin 0 (bin_index_x86), and whether the sample counts is
// decided from d itself (with finite min and range the division is NaN iff the sample is).  A launcher may pick the
// reciprocal form only for range inside [2^-60, 2^60] (binned_range_takes_rcp).
// Compile with -ffp-contract=off: every operation below is one IEEE operation, fmaf included.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define CRF_HDI __host__ __device__ __forceinline__
#else
#define CRF_HDI inline
#endif

namespace crf {

// what the marker-returning forms below give for a skipped sample: no bin, num_bins being at most 255
constexpr uint32_t kSkippedSampleBin = 0xFFu;

// int(t) the way the reference's x86-64 build evaluates a bin index before clamping it to [0, numBins - 1]
// (MutualInformation.cpp:66-67): cvttsd2si yields INT_MIN for NaN and for every t outside the int range -- so a POSITIVE
// overflow (t >= 2^31: caller-supplied extrema far narrower than the data, or +inf data) lands in bin 0, where the
// GPU's saturating conversion would give INT_MAX and bin numBins - 1.  On the device negative overflow and NaN saturate
// to values that clamp to bin 0 either way, so one compare suffices (and 0 stands for INT_MIN); on the host the
// conversion of an out-of-range value is undefined, so the instruction's result is written out.
CRF_HDI int bin_index_x86(double t) {
#if defined(__HIP_DEVICE_COMPILE__)
    return t < 2147483648.0 ? int(t) : 0;
#else
    return (t > -2147483649.0 && t < 2147483648.0) ? int(t) : INT_MIN;
#endif
}

CRF_HDI int clamp_bin(int b, int nb) { return b < 0 ? 0 : (b > nb - 1 ? nb - 1 : b); }

// the bin of a normalised value; nbd = double(nb)
CRF_HDI int bin_of_normalised(float q01, double nbd, int nb) {
    return clamp_bin(bin_index_x86(double(q01) * nbd), nb);
}

// the rule of launch_binned_n / launch_mi_binned_narrow: range is the fp32 difference max - min the kernels form
CRF_HDI bool binned_range_takes_rcp(float range) { return range >= 0x1p-60f && range <= 0x1p60f; }

// division form: the bin of y, *counts = the sample is not skipped
CRF_HDI int query_bin_div(float y, float min_q, float range_q, double nbd, int nb, bool* counts) {
    const float q01 = (y - min_q) / range_q;  // CorrelationCalculator.cpp:1061-1062
    *counts = q01 == q01;
    return bin_of_normalised(q01, nbd, nb);
}

// reciprocal form: rcp_q = 1.0f / range_q
CRF_HDI int query_bin_rcp(float y, float min_q, float range_q, float rcp_q, double nbd, int nb, bool* counts) {
    const float d = y - min_q;
    const float q0 = d * rcp_q;
    const float q01 = fmaf(fmaf(-q0, range_q, d), rcp_q, q0);
    *counts = d == d;  // min and range are finite here: the division is NaN iff the sample (and so d) is
    return bin_of_normalised(q01, nbd, nb);
}

// the same with the skipped sample folded into the result: a bin in [0, nb) or kSkippedSampleBin
CRF_HDI uint32_t query_bin_or_skip_div(float y, float min_q, float range_q, double nbd, int nb) {
    bool counts;
    const int b = query_bin_div(y, min_q, range_q, nbd, nb, &counts);
    return counts ? uint32_t(b) : kSkippedSampleBin;
}
CRF_HDI uint32_t query_bin_or_skip_rcp(float y, float min_q, float range_q, float rcp_q, double nbd, int nb) {
    bool counts;
    const int b = query_bin_rcp(y, min_q, range_q, rcp_q, nbd, nb, &counts);
    return counts ? uint32_t(b) : kSkippedSampleBin;
}

}  // namespace crf
