/*
 * ref_mi_driver.cpp -- TEST INFRASTRUCTURE.  A thin C-ABI driver around the REFERENCE's own MutualInformation.cpp and
 * DKL.cpp, <double> instantiations.
 *
 * oracle/Makefile compiles it together with those two files *where they lie* (never copied) into
 * oracle/_ref/libref_mi.so, with oracle/standins/ on the include path in place of boost, sgl and glm.  So:
 *   PINNED (the reference's object code):  everything the two files do themselves -- bin indices and their int()
 *     conversion, the histogram normalisation and summation order, the epsilon thresholds, how the noise is applied, the
 *     range counts of averageDigamma (`<` versus `<=`), the window descent of the DKL k-NN search, clamps and casts.
 *   STAND-INS (this repository's code, oracle/standins/): digamma at integers, the exact Chebyshev k-NN search (which
 *     REPLACES its output vectors -- see KdTreed.hpp), the xorshift32 noise stream (not sgl's), PI / TWO_PI / sqr / iceil.
 *   DRIVER CODE, NOT PINNED: the loops below (ref_mi_field, ref_mi_symmetric_field, ref_mi_pair_requests, ref_dkl_field).
 *     Their NaN rule, cs == 1 rule, binned normalisation and MI-CC map are written here after CorrelationCalculator.cpp:
 *     1026-1142, HEBChartCorrelation.cpp:543-590 and DKLCalculator.cpp:170-250, files that cannot be compiled (sgl::vk,
 *     ImGui, VolumeData).  The symmetric loop follows this project's own definition of that mode (corr_oracle.cpp).
 *
 * A std::domain_error of the stand-in digamma (a pole: KSG-2 with a marginal count of 1 evaluates digamma(0)) is caught
 * at the C boundary and answered with NaN.
 */
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <vector>

#include "DKL.hpp"                // -I$(REFERENCE)/src/Calculators
#include "MutualInformation.hpp"  // pulls <Utils/SearchStructures/KdTreed.hpp> from -Istandins

namespace {

const float QNAN = std::numeric_limits<float>::quiet_NaN();

struct BinnedScratch {
    std::vector<double> h0, h1, h2d;
    void ensure(int numBins) {
        h0.resize(size_t(numBins));
        h1.resize(size_t(numBins));
        h2d.resize(size_t(numBins) * size_t(numBins));
    }
};

float binned(const float* x01, const float* y01, int numBins, int n, BinnedScratch& s) {
    s.ensure(numBins);
    return computeMutualInformationBinned<double>(x01, y01, numBins, n, s.h0.data(), s.h1.data(), s.h2d.data());
}

float kraskov(const float* x, const float* y, int k, int n, int estimator, KraskovEstimatorCache<double>& cache) {
    try {
        return estimator == 2 ? computeMutualInformationKraskov2<double>(x, y, k, n, cache)
                              : computeMutualInformationKraskov<double>(x, y, k, n, cache);
    } catch (const std::domain_error&) {
        return QNAN;
    }
}

inline float mi_to_cc(float mi) {  // driver code
    return std::sqrt(1.0f - std::exp(-2.0f * mi));
}

// driver code: one voxel of the binned / Kraskov branch of calculateCpu.  ref01 is already normalised for the binned
// measures; q is scratch of cs floats.
float mi_voxel(int measure, const float* const* fields, int cs, size_t idx, const float* ref, int k, int estimator,
               int numBins, float minQuery, float maxQuery, float* q, BinnedScratch& bs,
               KraskovEstimatorCache<double>& cache) {
    if (cs == 1) return 1.0f;
    const bool isBinned = measure == 3 || measure == 5;
    for (int c = 0; c < cs; c++) {
        q[c] = fields[c][idx];
        if (std::isnan(q[c])) return QNAN;
        if (isBinned) q[c] = (q[c] - minQuery) / (maxQuery - minQuery);
    }
    float mi = isBinned ? binned(ref, q, numBins, cs, bs) : kraskov(ref, q, k, cs, estimator, cache);
    if (measure == 5 || measure == 6) mi = mi_to_cc(mi);
    return mi;
}

}  // namespace

extern "C" {

// --- the reference's functions, one call each --------------------------------------------------------------------
float ref_mi_binned(const float* x01, const float* y01, int numBins, int n) {
    BinnedScratch s;
    return binned(x01, y01, numBins, n, s);
}

float ref_mi_kraskov(const float* x, const float* y, int k, int n, int estimator) {
    KraskovEstimatorCache<double> cache;
    return kraskov(x, y, k, n, estimator, cache);
}

float ref_kraskov_max(int k, int n) {
    try {
        return computeMaximumMutualInformationKraskov(k, n);
    } catch (const std::domain_error&) {
        return QNAN;
    }
}

// both DKL estimators overwrite their input: the driver hands them a copy
float ref_dkl_binned(const float* values, int numBins, int n) {
    std::vector<float> v(values, values + n);
    std::vector<double> hist((size_t)numBins);
    return computeDKLBinned<double>(v.data(), numBins, n, hist.data());
}

float ref_dkl_knn(const float* values, int k, int n) {
    std::vector<float> v(values, values + n);
    try {
        return computeDKLKNNEstimate<double>(v.data(), k, n);
    } catch (const std::domain_error&) {
        return QNAN;
    }
}

// --- driver loops (NOT PINNED, see the header) --------------------------------------------------------------------
// measure: 3 binned MI, 4 Kraskov MI, 5 binned MI-CC, 6 Kraskov MI-CC (the numbering of corr_oracle.cpp)
int ref_mi_field(int measure, const float* const* fields, int cs, size_t voxelBegin, size_t voxelEnd,
                 const float* referenceValues, int k, int estimator, int numBins, float minRef, float maxRef,
                 float minQuery, float maxQuery, float* out) {
    if (measure < 3 || measure > 6 || cs < 1 || voxelEnd < voxelBegin) return 1;
    std::vector<float> ref(referenceValues, referenceValues + cs);
    if (measure == 3 || measure == 5) {
        for (int c = 0; c < cs; c++) ref[size_t(c)] = (ref[size_t(c)] - minRef) / (maxRef - minRef);
    }
    const long long n = (long long)(voxelEnd - voxelBegin);
#pragma omp parallel
    {
        std::vector<float> q((size_t)cs);
        BinnedScratch bs;
        KraskovEstimatorCache<double> cache;   // one per thread and reused from voxel to voxel, as in the reference
#pragma omp for
        for (long long i = 0; i < n; i++) {
            out[i] = mi_voxel(measure, fields, cs, voxelBegin + size_t(i), ref.data(), k, estimator, numBins, minQuery,
                              maxQuery, q.data(), bs, cache);
        }
    }
    return 0;
}

// this project's definition of the symmetric mode: the one-reference computation with the reference vector read from
// fieldsRef at the same voxel; a NaN there gives NaN; KSG-1 only
int ref_mi_symmetric_field(int measure, const float* const* fieldsRef, const float* const* fieldsQuery, int cs,
                           size_t voxelBegin, size_t voxelEnd, int k, int numBins, float minRef, float maxRef,
                           float minQuery, float maxQuery, float* out) {
    if (measure < 3 || measure > 6 || cs < 1 || voxelEnd < voxelBegin) return 1;
    const long long n = (long long)(voxelEnd - voxelBegin);
#pragma omp parallel
    {
        std::vector<float> ref((size_t)cs), q((size_t)cs);
        BinnedScratch bs;
        KraskovEstimatorCache<double> cache;
#pragma omp for
        for (long long i = 0; i < n; i++) {
            const size_t v = voxelBegin + size_t(i);
            bool isNan = false;
            for (int c = 0; c < cs; c++) {
                ref[size_t(c)] = fieldsRef[c][v];
                isNan = isNan || std::isnan(ref[size_t(c)]);
            }
            if (isNan && cs > 1) {
                out[i] = QNAN;
                continue;
            }
            if (measure == 3 || measure == 5) {
                for (int c = 0; c < cs; c++) ref[size_t(c)] = (ref[size_t(c)] - minRef) / (maxRef - minRef);
            }
            out[i] = mi_voxel(measure, fieldsQuery, cs, v, ref.data(), k, 1, numBins, minQuery, maxQuery, q.data(), bs,
                              cache);
        }
    }
    return 0;
}

// the per-pair body of the diagram's correlation computation: binned MI normalises both vectors with the extrema over
// the two of them; Kraskov is KSG-1
int ref_mi_pair_requests(int measure, const float* const* fields, int cs, const size_t* idxI, const size_t* idxJ,
                         size_t numRequests, int k, int numBins, int useAbs, float* out) {
    if (measure < 3 || measure > 6 || cs < 1) return 1;
    std::vector<float> X((size_t)cs), Y((size_t)cs);
    BinnedScratch bs;
    KraskovEstimatorCache<double> cache;
    for (size_t r = 0; r < numRequests; r++) {
        bool isNan = false;
        for (int c = 0; c < cs; c++) {
            X[size_t(c)] = fields[c][idxI[r]];
            Y[size_t(c)] = fields[c][idxJ[r]];
            isNan = isNan || std::isnan(X[size_t(c)]) || std::isnan(Y[size_t(c)]);
        }
        if (isNan) {
            out[r] = QNAN;
            continue;
        }
        if (cs == 1) {
            out[r] = 1.0f;
            continue;
        }
        float v;
        if (measure == 3 || measure == 5) {
            float mn = std::numeric_limits<float>::max(), mx = std::numeric_limits<float>::lowest();
            for (int c = 0; c < cs; c++) {
                mn = std::min(mn, X[size_t(c)]);
                mx = std::max(mx, X[size_t(c)]);
            }
            for (int c = 0; c < cs; c++) {
                mn = std::min(mn, Y[size_t(c)]);
                mx = std::max(mx, Y[size_t(c)]);
            }
            for (int c = 0; c < cs; c++) {
                X[size_t(c)] = (X[size_t(c)] - mn) / (mx - mn);
                Y[size_t(c)] = (Y[size_t(c)] - mn) / (mx - mn);
            }
            v = binned(X.data(), Y.data(), numBins, cs, bs);
        } else {
            v = kraskov(X.data(), Y.data(), k, cs, 1, cache);
        }
        if (measure == 5 || measure == 6) v = mi_to_cc(v);
        if (useAbs) v = std::abs(v);
        out[r] = v;
    }
    return 0;
}

// estimator 0 = binned (numBins), 1 = entropy k-NN (k); cs == 1 -> 1; a NaN member value -> NaN
int ref_dkl_field(int estimator, const float* const* fields, int cs, size_t numPoints, int numBins, int k, float* out) {
    if (cs < 1 || (estimator != 0 && estimator != 1)) return 1;
    if (estimator == 1 && cs > 1 && (k < 1 || k >= cs)) return 1;
    if (estimator == 0 && numBins < 1) return 1;
#pragma omp parallel
    {
        std::vector<float> vals((size_t)cs);
        std::vector<double> hist((size_t)std::max(numBins, 1));
#pragma omp for
        for (long long p = 0; p < (long long)numPoints; p++) {
            if (cs == 1) {
                out[p] = 1.0f;
                continue;
            }
            bool isNan = false;
            for (int c = 0; c < cs; c++) {
                vals[size_t(c)] = fields[c][p];
                isNan = isNan || std::isnan(vals[size_t(c)]);
            }
            if (isNan) {
                out[p] = QNAN;
                continue;
            }
            try {
                out[p] = estimator == 0 ? computeDKLBinned<double>(vals.data(), numBins, cs, hist.data())
                                        : computeDKLKNNEstimate<double>(vals.data(), k, cs);
            } catch (const std::domain_error&) {
                out[p] = QNAN;
            }
        }
    }
    return 0;
}

}  // extern "C"
