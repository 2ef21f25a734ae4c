// crf_two_vector_device.h -- what the two-vector kernels (kernels_symmetric.hip, kernels_symmetric_binned.hip, the
// two-vector kernel of kernels_pearson.hip) share: the guarded-slot scheme, the item -> byte offset arithmetic of the two
// modes, and the choice between the unguarded and the guarded instantiation.
#pragma once
#include "crf_device.h"
#include "crf_internal.h"

namespace crf {

// An instantiation holds N slots per vector, N the smallest multiple of 16 that holds cs: the first N - 16 slots are
// members whatever cs is, the last 16 are guarded -- unless the instantiation is EXACT (cs == N, no guards at all).
template <int N>
constexpr int sure_slots() {
    return N - 16;
}
// Is slot e a member?  A macro, spelled in place like the expression it replaces: as a function it leaves
// kendall_symmetric_kernel, which uses it inside `&&`, with another register allocation (up to 24 VGPRs more at 112 and
// 128 slots) although the instructions are the same.
#define CRF_SLOT_IS_MEMBER(N, EXACT, e, cs) ((EXACT) || (e) < ::crf::sure_slots<N>() || (e) < (cs))

// What a lane works on.  Field mode (REQ = false): voxel `item` of both fields.  Request mode: pair request `item`
// (layout {xi, yi, zi, i, xj, yj, zj, j}, HEBChart.hpp:166-168): X = the members at voxel i, Y = the members at voxel j.
struct RequestArgs {
    const uint32_t* requests;
    int xs, ys;
    int use_abs;
};
inline RequestArgs request_args(const TwoVectorJob& job) { return RequestArgs{job.requests, job.xs, job.ys, job.use_abs}; }

template <bool REQ, class Index>
__device__ __forceinline__ void lane_offsets(const RequestArgs& ra, Index item, Index num_items, uint32_t& offset_x,
                                             uint32_t& offset_y) {
    if constexpr (REQ) {
        offset_x = offset_y = kOutOfRangeOffset;  // lanes past the end read 0 and store nothing
        if (item < num_items) {
            const uint32_t* q = ra.requests + size_t(item) * 8;
            offset_x = ((q[2] * uint32_t(ra.ys) + q[1]) * uint32_t(ra.xs) + q[0]) * 4u;  // IDXS
            offset_y = ((q[6] * uint32_t(ra.ys) + q[5]) * uint32_t(ra.xs) + q[4]) * 4u;
        }
    } else {
        offset_x = offset_y = uint32_t(item) * 4u;
    }
}

// Launcher<N, EXACT, WAVES>::launch(job, s) for the instantiation that serves the job: the unguarded one in field mode
// at cs == N; request mode builds the guarded instantiations only.
template <template <int, bool, int> class Launcher, int N, int WAVES>
void launch_exact_or_guarded(const TwoVectorJob& job, hipStream_t s) {
    if (!job.requests && job.cs == N)
        Launcher<N, true, WAVES>::launch(job, s);
    else
        Launcher<N, false, WAVES>::launch(job, s);
}

}  // namespace crf
