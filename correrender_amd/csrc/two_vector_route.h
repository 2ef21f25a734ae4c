// two_vector_route.h -- which kernel evaluates a measure between two member vectors per item: the symmetric field mode
// (CRF_FLAG_SYMMETRIC: item v = voxel v of the primary and of the secondary field) and pair requests
// (crf_compute_requests*: item r = request {xi,yi,zi,i,xj,yj,zj,j}).  Plain C++17 without HIP types, like kraskov_plan.h,
// so that the table is testable on a machine without a GPU (tests/test_two_vector_route.py).  api.cpp (run_two_vector)
// asks it once per evaluation and calls the one launcher; the launchers are strict -- hipErrorInvalidValue outside the
// domain stated here.
#pragma once
#include "../../include/corrfield.h"
#include "kraskov_plan.h"

namespace crf {

// Largest member count supported at all by the sort-based estimators (LDS / register budgets).
constexpr int kMaxSortMembers = 128;
// Largest member count of the two-vector Pearson kernel (both vectors resident in registers).
constexpr int kMaxSymmetricRegisterMembers = 128;

enum class TwoVectorKernel {
    Fill,             // one member: every result is 1 (fill_kernel)
    PearsonRegister,  // pearson_symmetric_kernel (kernels_pearson.hip)
    KraskovDirect,    // kraskov_direct_kernel<K, TI, SYM = true> (kernels_kraskov.hip)
    Sorted,           // spearman_ / kendall_ / binned_symmetric_kernel (kernels_symmetric.hip, kernels_symmetric_binned.hip)
    DirectSymmetric,  // direct_symmetric_kernel (kernels_generic.hip): field mode, any member count
    PairRequest,      // pair_request_kernel (kernels_generic.hip): every measure, any member count
};

// the domain of the sort-based kernels: Spearman, Kendall, and the binned measures with bin codes of one byte
inline bool two_vector_sortable(int measure, int cs, int num_bins) {
    if (cs < 2 || cs > kMaxSortMembers) return false;
    if (measure == CRF_SPEARMAN || measure == CRF_KENDALL) return true;
    return (measure == CRF_MI_BINNED || measure == CRF_BINNED_MI_CC) && num_bins >= 1 && num_bins <= 255;
}

// requests: request mode, else symmetric field mode.  force_counting: CRF_SYMMETRIC_DIRECT=1 (field mode: the sort-based
// kernels are skipped, nothing else) or CRF_REQUESTS_GENERIC=1 (request mode: pair_request_kernel for everything).
// items_fit_u32: fewer than 2^32 items (the Pearson kernel indexes them with 32 bits; field mode always does, a grid
// beyond that is evaluated in windows).
inline TwoVectorKernel two_vector_route(bool requests, int measure, int cs, int k, int num_bins, bool force_counting,
                                        bool items_fit_u32 = true) {
    if (requests) {
        if (force_counting) return TwoVectorKernel::PairRequest;
        if (measure == CRF_PEARSON)
            return cs >= 2 && cs <= kMaxSymmetricRegisterMembers && items_fit_u32 ? TwoVectorKernel::PearsonRegister
                                                                                  : TwoVectorKernel::PairRequest;
        return two_vector_sortable(measure, cs, num_bins) ? TwoVectorKernel::Sorted : TwoVectorKernel::PairRequest;
    }
    switch (measure) {
        case CRF_PEARSON:
            if (cs == 1) return TwoVectorKernel::Fill;
            return cs <= kMaxSymmetricRegisterMembers ? TwoVectorKernel::PearsonRegister : TwoVectorKernel::PairRequest;
        case CRF_MI_KRASKOV:
        case CRF_KMI_CC: {
            if (cs == 1) return TwoVectorKernel::Fill;
            KraskovPlan plan;
            return kraskov_symmetric_plan(cs, k, &plan) ? TwoVectorKernel::KraskovDirect : TwoVectorKernel::PairRequest;
        }
        case CRF_SPEARMAN:
        case CRF_KENDALL:
        case CRF_MI_BINNED:
        case CRF_BINNED_MI_CC:
            return !force_counting && two_vector_sortable(measure, cs, num_bins) ? TwoVectorKernel::Sorted
                                                                                 : TwoVectorKernel::DirectSymmetric;
        default: return TwoVectorKernel::PairRequest;  // no such measure (check_params turns it away first)
    }
}

// what crf_last_kernel_name reports for a route: the kernel family, by mode; the fill reports the kernel it stands in for
inline const char* two_vector_kernel_name(TwoVectorKernel kernel, bool requests, int measure) {
    switch (kernel) {
        case TwoVectorKernel::Fill: return measure == CRF_PEARSON ? "pearson_symmetric_kernel" : "kraskov_direct_kernel";
        case TwoVectorKernel::PearsonRegister: return requests ? "pearson_request_kernel" : "pearson_symmetric_kernel";
        case TwoVectorKernel::KraskovDirect: return "kraskov_direct_kernel";
        case TwoVectorKernel::Sorted: return requests ? "sorted_request_kernel" : "sorted_symmetric_kernel";
        case TwoVectorKernel::DirectSymmetric: return "direct_symmetric_kernel";
        default: return "pair_request_kernel";
    }
}

}  // namespace crf
