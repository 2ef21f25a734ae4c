// symmetric_narrow_route.h -- at which (member format, member count) the symmetric Pearson field reads two narrow fields as
// stored (kernels_pearson.hip: pearson_symmetric_narrow_kernel) instead of running pearson_symmetric_kernel on their fp32
// copies.  Plain C++17 without HIP types, like two_vector_route.h, so that the table is testable on a machine without a GPU
// (tests/test_symmetric_narrow_route.py).  api.cpp (native_field) adds what only the context knows: both fields in the
// same narrow format, both sets 4-byte aligned, the grid not windowed.
#pragma once
#include "../../include/corrfield.h"

namespace crf {

// Largest member count of the native kernel: 2 x 128 raw dwords per lane plus the working set of a dword's voxels fit the
// 512-entry register file at one wave per SIMD.
constexpr int kSymmetricNarrowMaxMembers = 128;

// 2..64 members: every narrow format (the kernel moves 2 cs e + 4 bytes per voxel where the copy route moves 8 cs + 4).
// 65..128 members: where the native kernel was measured no slower than pearson_symmetric_kernel on the copies, per format
// and N = cs rounded up to 16 (profiles/narrow_symmetric_ab.md): every format at every N.  (No instantiation needs scratch.)
constexpr bool symmetric_narrow_routed(int format, int cs) {
    if (format != CRF_MEMBER_U8 && format != CRF_MEMBER_U16 && format != CRF_MEMBER_F16) return false;
    if (cs < 2 || cs > kSymmetricNarrowMaxMembers) return false;
    return true;
}

}  // namespace crf
