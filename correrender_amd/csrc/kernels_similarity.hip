// kernels_similarity.hip -- whole-field similarity of two scalar fields (crf_field_similarity; reference:
// computeFieldSimilarity<double>, src/Calculators/Similarity.cpp:36-180): ONE value over the samples
// (x[m][v], y[m][v]) of every voxel v of `members` member volumes of both fields, pairs with a NaN left out.
//
// Both measures stream the two fields once per pass from HBM and keep nothing, so the kernels are judged against the
// algorithmic bytes (8 per sample and pass).  Work is cut into CHUNKS of threads x 16 consecutive voxels of one member;
// a capped, persistent grid strides over the chunks.  Inside a chunk lane t owns, for u = 0..3, the four voxels
// base + (u * threads + t) * 4 .. + 3: one 16-byte load per field and u when every member of both fields is 16-byte
// aligned (a wave then reads 1 KiB contiguous per load instruction), four dword loads otherwise (borrowed members may
// be only 4-byte aligned).  Ownership and order of accumulation are the same in both forms, so the two give the same
// bits.  All 8 loads of a chunk are issued before the first value is used.
//
//   similarity_moments_kernel   pass 1: N, sum x, sum y;  pass 2: Sxx, Syy, Sxy about the means, which it reads from
//                               device memory (no host round trip in between).  fp64 accumulators per lane (four per
//                               quantity, one per voxel of the lane's quadruple, combined in a fixed order), a butterfly
//                               over the wave, the waves of a block in order, ONE partial record per block.
//   similarity_finish_kernel    one block: adds the partial records in index order, leaves the means (pass 1) or the
//                               moments and the value (pass 2).  No floating-point atomics anywhere: the value is
//                               bitwise reproducible from call to call (the grid size depends on the device and the
//                               sample count only).
//   similarity_histogram_kernel the joint histogram of binned mutual information: num_bins^2 32-bit counters in
//                               dynamic LDS per block (64 KiB at 128 bins: two blocks of 512 threads per CU), flushed
//                               to a global 64-bit histogram with integer atomics, non-zero counters only.  Counts are
//                               integers: any order of accumulation gives the same histogram.  Real fields put most
//                               samples into a few cells; every lane therefore carries a RUN (cell, count) through
//                               all its samples and issues one LDS atomic per change of cell -- a field in one cell
//                               costs one atomic per lane, a uniform one an atomic per sample on spread addresses.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>

#include "crf_binned_bins.h"
#include "crf_internal.h"
#include "crf_similarity_chunks.h"

namespace crf {
namespace {

using namespace chunks;  // Samples, load_chunk, make_samples, grid_blocks (crf_similarity_chunks.h)

constexpr int kMomentThreads = 256;
constexpr int kHistogramThreads = 512;
// the one-block finishing kernel holds every partial record in LDS (4 doubles each)
constexpr int kMaxMomentBlocks = 1024;
constexpr uint32_t kNoCell = 0xFFFFFFFFu;

__device__ __forceinline__ double wave_sum(double v) {  // butterfly: the same value, in the same order, on every lane
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// stats (doubles): [0] N  [1] mean x  [2] mean y  [3] Sxx  [4] Syy  [5] Sxy  [6] the value
template <int PASS, bool VEC>
__global__ __launch_bounds__(kMomentThreads) void similarity_moments_kernel(Samples s, const double* __restrict__ stats,
                                                                            double* __restrict__ partials) {
    double a[3][4] = {};  // pass 1: sum x, sum y, N;  pass 2: Sxx, Syy, Sxy
    double mean_x = 0.0, mean_y = 0.0;
    if constexpr (PASS == 2) mean_x = stats[1], mean_y = stats[2];
    for (uint32_t chunk = blockIdx.x; chunk < s.chunks; chunk += gridDim.x) {
        const uint32_t m = chunk / s.chunks_per_member;
        const uint32_t base = (chunk - m * s.chunks_per_member) * uint32_t(kMomentThreads * kLaneVoxels);
        float x[kLaneVoxels], y[kLaneVoxels];
        load_chunk<VEC, kMomentThreads, false>(s.x[m], s.y[m], base, s.voxels, x, y);
#pragma unroll
        for (int e = 0; e < kLaneVoxels; e++) {
            const bool ok = x[e] == x[e] && y[e] == y[e];
            const int j = e & 3;
            if constexpr (PASS == 1) {
                a[0][j] += ok ? double(x[e]) : 0.0;
                a[1][j] += ok ? double(y[e]) : 0.0;
                a[2][j] += ok ? 1.0 : 0.0;  // exact: N stays below 2^31
            } else {
                const double dx = ok ? double(x[e]) - mean_x : 0.0;
                const double dy = ok ? double(y[e]) - mean_y : 0.0;
                a[0][j] += dx * dx;
                a[1][j] += dy * dy;
                a[2][j] += dx * dy;
            }
        }
    }
    __shared__ double waves[3][kMomentThreads / 64];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const double lane = (a[q][0] + a[q][1]) + (a[q][2] + a[q][3]);
        const double w = wave_sum(lane);
        if ((threadIdx.x & 63) == 0) waves[q][threadIdx.x >> 6] = w;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = waves[threadIdx.x][0];
        for (int w = 1; w < kMomentThreads / 64; w++) t += waves[threadIdx.x][w];
        partials[size_t(blockIdx.x) * 4 + threadIdx.x] = t;
    }
}

template <int PASS>
__global__ __launch_bounds__(256) void similarity_finish_kernel(const double* __restrict__ partials, int blocks,
                                                                double* __restrict__ stats) {
    __shared__ double rec[kMaxMomentBlocks * 4];
    __shared__ double total[3];
    for (int i = threadIdx.x; i < blocks * 4; i += 256) rec[i] = partials[i];
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = 0.0;
        for (int b = 0; b < blocks; b++) t += rec[b * 4 + threadIdx.x];  // index order
        total[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if constexpr (PASS == 1) {  // sum x, sum y, N
        const double n = total[2];
        stats[0] = n;
        stats[1] = total[0] / n;
        stats[2] = total[1] / n;
    } else {  // Sxx, Syy, Sxy
        const double sxx = total[0], syy = total[1], sxy = total[2];
        stats[3] = sxx;
        stats[4] = syy;
        stats[5] = sxy;
        // N = 0: 0 (the reference's empty loops);  N = 1 or a constant side: 0 / 0 = NaN, as the reference's division
        // by a zero standard deviation
        const float r = stats[0] == 0.0 ? 0.0f : float(sxy / (sqrt(sxx) * sqrt(syy)));
        stats[6] = double(r);
    }
}

struct Bins {
    int nb;
    double nbd;
    float min_x, range_x, rcp_x, min_y, range_y, rcp_y;
};

// RCP: both ranges lie inside [2^-60, 2^60] and both minima are finite, so the reciprocal form of the normalisation
// gives the division's bin and a sample's normalised value is NaN iff the sample is (crf_binned_bins.h)
template <bool VEC, bool RCP>
__global__ __launch_bounds__(kHistogramThreads) void similarity_histogram_kernel(Samples s, Bins b,
                                                                                 unsigned long long* __restrict__ hist,
                                                                                 unsigned long long* __restrict__ samples) {
    extern __shared__ uint32_t cells[];  // nb * nb counters
    const uint32_t num_cells = uint32_t(b.nb * b.nb);
    for (uint32_t i = threadIdx.x; i < num_cells; i += kHistogramThreads) cells[i] = 0u;
    __syncthreads();
    uint32_t run_cell = kNoCell, run_count = 0u, pairs = 0u;
    for (uint32_t chunk = blockIdx.x; chunk < s.chunks; chunk += gridDim.x) {
        const uint32_t m = chunk / s.chunks_per_member;
        const uint32_t base = (chunk - m * s.chunks_per_member) * uint32_t(kHistogramThreads * kLaneVoxels);
        float x[kLaneVoxels], y[kLaneVoxels];
        load_chunk<VEC, kHistogramThreads, true>(s.x[m], s.y[m], base, s.voxels, x, y);
#pragma unroll
        for (int e = 0; e < kLaneVoxels; e++) {
            const bool pair = x[e] == x[e] && y[e] == y[e];  // what the reference hands to the estimator: its `es`
            bool cx, cy;
            int bx, by;
            if constexpr (RCP) {
                bx = query_bin_rcp(x[e], b.min_x, b.range_x, b.rcp_x, b.nbd, b.nb, &cx);
                by = query_bin_rcp(y[e], b.min_y, b.range_y, b.rcp_y, b.nbd, b.nb, &cy);
            } else {
                bx = query_bin_div(x[e], b.min_x, b.range_x, b.nbd, b.nb, &cx);
                by = query_bin_div(y[e], b.min_y, b.range_y, b.nbd, b.nb, &cy);
            }
            pairs += pair ? 1u : 0u;
            // a pair whose normalised value is NaN counts as a sample and enters no cell (MutualInformation.cpp:64)
            const uint32_t cell = (pair && cx && cy) ? uint32_t(bx * b.nb + by) : kNoCell;
            if (cell != run_cell) {
                if (run_count != 0u) atomicAdd(&cells[run_cell], run_count);
                run_cell = cell;
                run_count = 0u;
            }
            run_count += cell != kNoCell ? 1u : 0u;
        }
    }
    if (run_count != 0u) atomicAdd(&cells[run_cell], run_count);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) pairs += __shfl_xor(pairs, off);
    if ((threadIdx.x & 63) == 0 && pairs != 0u) atomicAdd(samples, (unsigned long long)pairs);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < num_cells; i += kHistogramThreads) {
        const uint32_t v = cells[i];
        if (v != 0u) atomicAdd(&hist[i], (unsigned long long)v);
    }
}

bool job_ok(const SimilarityJob& job) {
    // 32-bit voxel indices, a chunk past the end included; the sample count fits the reference's int
    return job.members >= 1 && job.num_voxels >= 1 && job.num_voxels < (size_t(1) << 30) &&
           size_t(job.members) * job.num_voxels <= size_t(0x7FFFFFFF) && job.workspace != nullptr;
}

// workspace layout
constexpr size_t kStatsOffset = 0;                                               // 8 doubles
constexpr size_t kSamplesOffset = 64;                                            // one 64-bit counter
constexpr size_t kHistOffset = 128;                                              // kSimilarityMaxBins^2 64-bit counters
constexpr size_t kHistBytes = size_t(kSimilarityMaxBins) * kSimilarityMaxBins * 8;
constexpr size_t kPartialsOffset = kHistOffset + kHistBytes;                     // kMaxMomentBlocks records of 4 doubles
constexpr size_t kWorkspaceBytes = kPartialsOffset + size_t(kMaxMomentBlocks) * 4 * sizeof(double);

}  // namespace

size_t similarity_workspace_bytes() { return kWorkspaceBytes; }
const double* similarity_stats(const unsigned char* workspace) {
    return reinterpret_cast<const double*>(workspace + kStatsOffset);
}
const unsigned long long* similarity_samples(const unsigned char* workspace) {
    return reinterpret_cast<const unsigned long long*>(workspace + kSamplesOffset);
}
const unsigned long long* similarity_histogram(const unsigned char* workspace) {
    return reinterpret_cast<const unsigned long long*>(workspace + kHistOffset);
}

hipError_t launch_similarity_moments(const SimilarityJob& job, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end,
                                     LaunchInfo* info) {
    if (info) info->kernel_name = "similarity_moments_kernel";
    if (!job_ok(job)) return hipErrorInvalidValue;
    int cus = 0;
    if (hipError_t e = compute_units(&cus); e != hipSuccess) return e;
    const Samples smp = make_samples(job, kMomentThreads);
    // four blocks of four waves per CU: 16 waves with 8 x 16 B in flight each
    const uint32_t blocks = grid_blocks(smp.chunks, std::min(4 * cus, kMaxMomentBlocks));
    double* stats = reinterpret_cast<double*>(job.workspace + kStatsOffset);
    double* partials = reinterpret_cast<double*>(job.workspace + kPartialsOffset);
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    if (job.vec16) {
        hipLaunchKernelGGL((similarity_moments_kernel<1, true>), dim3(blocks), dim3(kMomentThreads), 0, s, smp, stats, partials);
        hipLaunchKernelGGL((similarity_finish_kernel<1>), dim3(1), dim3(256), 0, s, partials, int(blocks), stats);
        hipLaunchKernelGGL((similarity_moments_kernel<2, true>), dim3(blocks), dim3(kMomentThreads), 0, s, smp, stats, partials);
    } else {
        hipLaunchKernelGGL((similarity_moments_kernel<1, false>), dim3(blocks), dim3(kMomentThreads), 0, s, smp, stats, partials);
        hipLaunchKernelGGL((similarity_finish_kernel<1>), dim3(1), dim3(256), 0, s, partials, int(blocks), stats);
        hipLaunchKernelGGL((similarity_moments_kernel<2, false>), dim3(blocks), dim3(kMomentThreads), 0, s, smp, stats, partials);
    }
    hipLaunchKernelGGL((similarity_finish_kernel<2>), dim3(1), dim3(256), 0, s, partials, int(blocks), stats);
    if (ev_end) (void)hipEventRecord(ev_end, s);
    return hipGetLastError();
}

hipError_t launch_similarity_histogram(const SimilarityJob& job, int num_bins, float min_x, float max_x, float min_y,
                                       float max_y, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end,
                                       LaunchInfo* info) {
    if (info) info->kernel_name = "similarity_histogram_kernel";
    if (!job_ok(job) || num_bins < 1 || num_bins > kSimilarityMaxBins) return hipErrorInvalidValue;
    int cus = 0;
    if (hipError_t e = compute_units(&cus); e != hipSuccess) return e;
    const Samples smp = make_samples(job, kHistogramThreads);
    Bins b;
    b.nb = num_bins;
    b.nbd = double(num_bins);
    b.min_x = min_x, b.range_x = max_x - min_x, b.rcp_x = 1.0f / b.range_x;
    b.min_y = min_y, b.range_y = max_y - min_y, b.rcp_y = 1.0f / b.range_y;
    const bool rcp = binned_range_takes_rcp(b.range_x) && binned_range_takes_rcp(b.range_y) && std::isfinite(min_x) &&
                     std::isfinite(min_y);
    // two blocks of eight waves per CU at every bin count: 128 bins take 64 KiB of the CU's 160 KiB per block
    const size_t lds = size_t(num_bins) * size_t(num_bins) * sizeof(uint32_t);
    const uint32_t blocks = grid_blocks(smp.chunks, 2 * cus);
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(job.workspace + kHistOffset);
    unsigned long long* samples = reinterpret_cast<unsigned long long*>(job.workspace + kSamplesOffset);
    if (hipError_t e = hipMemsetAsync(job.workspace + kSamplesOffset, 0, kHistOffset - kSamplesOffset + size_t(num_bins) * num_bins * 8, s);
        e != hipSuccess)
        return e;
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    if (job.vec16 && rcp)
        hipLaunchKernelGGL((similarity_histogram_kernel<true, true>), dim3(blocks), dim3(kHistogramThreads), lds, s, smp, b, hist, samples);
    else if (job.vec16)
        hipLaunchKernelGGL((similarity_histogram_kernel<true, false>), dim3(blocks), dim3(kHistogramThreads), lds, s, smp, b, hist, samples);
    else if (rcp)
        hipLaunchKernelGGL((similarity_histogram_kernel<false, true>), dim3(blocks), dim3(kHistogramThreads), lds, s, smp, b, hist, samples);
    else
        hipLaunchKernelGGL((similarity_histogram_kernel<false, false>), dim3(blocks), dim3(kHistogramThreads), lds, s, smp, b, hist, samples);
    if (ev_end) (void)hipEventRecord(ev_end, s);
    return hipGetLastError();
}

}  // namespace crf
