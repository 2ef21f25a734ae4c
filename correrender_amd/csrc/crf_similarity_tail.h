// crf_similarity_tail.h -- the host half of crf_field_similarity's binned measures: from the joint histogram's integer
// counts to the mutual information; and of the Kendall calls: from four integers to tau-b.  Plain C++, no HIP: api.cpp
// calls it on the counts similarity_histogram_kernel and kernels_kendall_similarity.hip leave,
// tests/native/similarity_tail.cpp and tests/native/kendall_tail.cpp run it without a GPU.
//
// The reference (computeMutualInformationBinned<double>, MutualInformation.cpp:45-143) adds 1.0 per sample into an fp64
// histogram -- exact integers, so the histogram does not depend on the order the samples arrive in -- and everything
// after that is restated here operation by operation in its loop order: the total (:72-77), the division (:78-82), the
// marginals (:106-111), the two epsilon tests and the three entropy sums (:120-140), all in fp64 with the host's log.
// Compile with -ffp-contract=off: `mi -= p * log(p)` is a product and a difference, as in the reference's x86-64 build.
//
// `samples` is the reference's `es`: the pairs handed to the function (Similarity.cpp:128, every pair without a NaN
// value), which may exceed the histogram's total -- a pair whose NORMALISED value is NaN (inf / inf under infinite
// extrema) is counted in es and left out of the histogram (:64).
//
// One deliberate deviation: the reference forms EPSILON_2D = 0.5 / Real(es * es) with an int product (:121), which
// overflows from 46 341 samples on (its object code then returns NaN at 46 341 and H(x) + H(y) without the joint term
// at 65 536).  Here the product is formed in fp64: bit-identical to the object code up to 46 340 samples, well defined
// beyond.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace crf {

inline float similarity_mi_from_counts(const uint64_t* counts, int num_bins, uint64_t samples) {
    const size_t nb = size_t(num_bins);
    std::vector<double> h2d(nb * nb), h0(nb, 0.0), h1(nb, 0.0);
    for (size_t i = 0; i < nb * nb; i++) h2d[i] = double(counts[i]);
    double total = 0.0;
    for (size_t i = 0; i < nb * nb; i++) total += h2d[i];
    for (size_t i = 0; i < nb * nb; i++) h2d[i] /= total;  // no sample: 0 / 0 = NaN, which fails every test below
    for (size_t b0 = 0; b0 < nb; b0++) {
        for (size_t b1 = 0; b1 < nb; b1++) {
            h0[b0] += h2d[b0 * nb + b1];
            h1[b1] += h2d[b0 * nb + b1];
        }
    }
    const double es = double(samples);
    const double epsilon_1d = 0.5 / es;
    const double epsilon_2d = 0.5 / (es * es);  // the deviation: an fp64 product
    double mi = 0.0;
    for (size_t b = 0; b < nb; b++) {
        const double p_x = h0[b], p_y = h1[b];
        if (p_x > epsilon_1d) mi -= p_x * std::log(p_x);
        if (p_y > epsilon_1d) mi -= p_y * std::log(p_y);
    }
    for (size_t i = 0; i < nb * nb; i++) {
        const double p_xy = h2d[i];
        if (p_xy > epsilon_2d) mi += p_xy * std::log(p_xy);
    }
    return float(mi);
}

// Kendall's tau-b from its integers, computeKendall<int64_t> (Correlation.cpp:439-453) verbatim: n pairs, n1 and n2 the
// tie sums of x and of y (joint ties n3 stay 0, as there), S the strict inversions.  Exact integers, three IEEE double
// operations and a cast; no special cases: no pair or one gives 0 / 0 = NaN, a constant side NaN or +-inf.  counts (may be
// null) receives n0, n1, n2, S.
inline float similarity_kendall_from_counts(int64_t n, int64_t n1, int64_t n2, int64_t s, long long* counts) {
    const int64_t n0 = (n * (n - 1)) / 2;
    const int64_t numerator = n0 - n1 - n2 - 2 * s;
    // volatile: the division runs on the machine even where the compiler knows its operands (no pair: 0 / 0).  The
    // reference's is a run-time division, and the x86-64 instruction gives the NaN with the sign bit set where a compiler
    // that folds 0.0 / 0.0 gives the one without.
    volatile double dividend = double(numerator);
    volatile double denominator = std::sqrt(double(n0 - n1)) * std::sqrt(double(n0 - n2));
    if (counts) counts[0] = n0, counts[1] = n1, counts[2] = n2, counts[3] = s;
    return float(dividend / denominator);
}

// sqrt(1 - exp(-2 MI)) in fp32 with the host's expf (Similarity.cpp:165-167; on the device: crf_mi_device.h, mi_to_cc)
inline float similarity_mi_to_cc(float mi) { return std::sqrt(1.0f - std::exp(-2.0f * mi)); }

}  // namespace crf
