// crf_dkl_device.h -- the parts of dkl_kernel<FMT, NS> (kernels_dkl.hip) that stand on their own: tile and table sizes
// (host and device) and the window descent of the k-NN estimator.  Nothing here depends on how the members are stored.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "crf_device.h"
#include "crf_internal.h"

namespace crf {

namespace {
constexpr int kDklBlocks = 1024;
constexpr size_t kDklLdsLimit = 60 * 1024;

// ln(h) for the h = 0..cs samples a bin can hold (binned estimator), rounded up to 16 bytes; 0 for the k-NN estimator
__host__ __device__ inline size_t dkl_log_table_bytes(int cs, int estimator) {
    return estimator == 0 ? ((size_t(cs) + 1) * sizeof(double) + 15) & ~size_t(15) : 0;
}

// in_place: the k-NN estimator's network sort holds the whole column in registers and writes the sorted values back
// over it -- one column instead of two (twice the resident blocks per CU for this latency-bound kernel)
__host__ __device__ inline size_t dkl_tile_bytes(int cs, int estimator, int num_bins, bool in_place = false) {
    const size_t column = size_t(cs) * 64 * sizeof(float);
    return estimator == 0 ? column + size_t(num_bins) * 64 * sizeof(uint16_t) : (in_place ? column : 2 * column);
}

// sgl's Math.hpp declares PI and TWO_PI as float (see oracle/corr_oracle.cpp for the pinning note)
constexpr float kSglPi = 3.1415926535897932f;
constexpr float kSglTwoPi = kSglPi * 2.0f;

// Sorts the lane's column (stride 64 floats, cs <= N values) into `sorted` with the N-input min/max network: keys that
// order like the floats (crf_device.h: orderable_key), pads = 0xFFFFFFFF behind every real value, keys mapped back.
template <int N>
__device__ __forceinline__ void sort_column(const float* vals, float* sorted, int cs) {
    uint32_t a[N];
#pragma unroll
    for (int e = 0; e < N; e++) a[e] = e < cs ? orderable_key(vals[(e < cs ? e : 0) * 64]) : 0xFFFFFFFFu;
    __builtin_amdgcn_sched_barrier(0);  // the network is straight-line code: left to the scheduler it is interleaved
    SortNet32<N>::sort(a);              // with the loads and stores around it and runs out of registers
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < N; p++) {
        const uint32_t key = a[p];
        const uint32_t bits = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
        if (p < cs) sorted[p * 64] = __uint_as_float(bits);
    }
}

// Distance from sorted element i to its k-th nearest neighbour as the reference's heuristic finds it
// (findKNearestNeighbors<float>, DKL.cpp:98-130): NOT an exact k-NN query but a descent over windows of k + 1 consecutive
// sorted elements that hold element i, whose outcome -- including where it stalls -- is part of the estimator's
// definition.  Restated here as a descent on a window COST: the window [lo, lo + k] costs the larger of the two gaps
// from element i to its ends, an end that leaves the column or passes element i costs FLT_MAX.  Each round compares
// the windows `step` to the left and to the right, moves towards the cheaper one unless the current window is
// strictly cheaper than both, then halves the step (rounding up) until a round with step 1 has been played.  `col` is
// the lane's ascending column (stride 64 floats).
struct KnnWindow {
    const float* col;
    int n, k, i;
    float centre;
    __device__ float left_gap(int lo) const { return (lo >= 0 && lo <= i) ? centre - col[lo * 64] : 3.402823466e+38f; }
    __device__ float right_gap(int hi) const { return (hi >= i && hi < n) ? col[hi * 64] - centre : 3.402823466e+38f; }
    __device__ float cost(int lo) const { return fmaxf(left_gap(lo), right_gap(lo + k)); }
};

// The same descent for E sorted elements at once (e0 .. e0 + E - 1, clamped to the column): the step sequence depends
// on k only, so the rounds are the outer loop and the E x 6 column reads of a round are independent -- one element after
// the other, every round was a dependent LDS round trip (r02: the kernel is bound by exactly that latency).
template <int E>
__device__ __forceinline__ void dkl_window_distances(const float* data, int N, int k, int e0, float (&dist)[E]) {
    KnnWindow w[E];
    int lo[E];
    const int first_step = (k + 1) / 2;
#pragma unroll
    for (int u = 0; u < E; u++) {
        const int i = e0 + u < N ? e0 + u : N - 1;
        w[u] = KnnWindow{data, N, k, i, data[i * 64]};
        lo[u] = i - first_step > 0 ? i - first_step : 0;
        lo[u] = lo[u] + k >= N ? N - k - 1 : lo[u];
    }
    int step = first_step;
#pragma unroll 1
    for (bool last = false; !last; step = (step + 1) / 2) {
        last = step == 1;
        float here[E], left[E], right[E];
#pragma unroll
        for (int u = 0; u < E; u++) {
            here[u] = w[u].cost(lo[u]);
            left[u] = w[u].cost(lo[u] - step);
            right[u] = w[u].cost(lo[u] + step);
        }
#pragma unroll
        for (int u = 0; u < E; u++) {
            const int towards = (left[u] > right[u]) - (left[u] < right[u]);
            lo[u] += (here[u] < left[u] && here[u] < right[u]) ? 0 : towards * step;
        }
    }
#pragma unroll
    for (int u = 0; u < E; u++) dist[u] = w[u].cost(lo[u]);
}

__device__ float dkl_window_distance(const float* data, int N, int k, int i) {
    const KnnWindow w{data, N, k, i, data[i * 64]};
    int step = (k + 1) / 2;
    // start: element i sits `step` from the left end, clamped into the column
    int lo = i - step > 0 ? i - step : 0;
    lo = lo + k >= N ? N - k - 1 : lo;
#pragma unroll 1
    for (bool last = false; !last; step = (step + 1) / 2) {
        last = step == 1;
        const float here = w.cost(lo), left = w.cost(lo - step), right = w.cost(lo + step);
        const int towards = (left > right) - (left < right);  // +1: the right window is cheaper; 0: a draw
        lo += (here < left && here < right) ? 0 : towards * step;
    }
    return w.cost(lo);
}

}  // namespace

}  // namespace crf
