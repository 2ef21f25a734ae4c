// crf_similarity_chunks.h -- how the whole-field similarity kernels (kernels_similarity.hip, kernels_rank_similarity.hip)
// cut two fields into work: CHUNKS of threads x 16 consecutive voxels of one member, and a capped, persistent grid that
// strides over them.  Inside a chunk lane t owns, for u = 0..3, the four voxels base + (u * threads + t) * 4 .. + 3: one
// 16-byte load per field and u when every member of both fields is 16-byte aligned, four dword loads otherwise.
// Ownership is the same in both forms.  Device and launcher code; internal to libcorrfield.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <limits>

#include "crf_internal.h"

namespace crf {
namespace chunks {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kLaneVoxels = 16;  // per chunk: 4 quadruples

struct Samples {
    const float* const* x;
    const float* const* y;
    uint32_t voxels;             // per member, below 2^30
    uint32_t chunks_per_member;  // ceil(voxels / (threads * kLaneVoxels))
    uint32_t chunks;             // members * chunks_per_member
};

// the lane's 16 voxels of both fields; voxels past the end of the member read as NaN (a pair that is left out)
template <bool VEC, int THREADS, bool NT>
__device__ __forceinline__ void load_chunk(const float* __restrict__ px, const float* __restrict__ py, uint32_t base,
                                           uint32_t voxels, float (&x)[kLaneVoxels], float (&y)[kLaneVoxels]) {
    const uint32_t first = base + threadIdx.x * 4;
    if (base + uint32_t(THREADS * kLaneVoxels) <= voxels) {  // block-uniform: a whole chunk
        if constexpr (VEC) {
            f4 a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const f4* qx = reinterpret_cast<const f4*>(px + first + u * THREADS * 4);
                const f4* qy = reinterpret_cast<const f4*>(py + first + u * THREADS * 4);
                a[u] = NT ? __builtin_nontemporal_load(qx) : *qx;
                b[u] = NT ? __builtin_nontemporal_load(qy) : *qy;
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int j = 0; j < 4; j++) x[4 * u + j] = a[u][j], y[4 * u + j] = b[u][j];
        } else {
#pragma unroll
            for (int e = 0; e < kLaneVoxels; e++) {
                const uint32_t i = first + (e >> 2) * THREADS * 4 + (e & 3);
                x[e] = NT ? __builtin_nontemporal_load(px + i) : px[i];
                y[e] = NT ? __builtin_nontemporal_load(py + i) : py[i];
            }
        }
    } else {  // the ragged last chunk of a member
        const float nan = std::numeric_limits<float>::quiet_NaN();
#pragma unroll
        for (int e = 0; e < kLaneVoxels; e++) {
            const uint32_t i = first + (e >> 2) * THREADS * 4 + (e & 3);
            x[e] = i < voxels ? px[i] : nan;
            y[e] = i < voxels ? py[i] : nan;
        }
    }
}

inline Samples make_samples(const SimilarityJob& job, int threads) {
    Samples s;
    s.x = job.x;
    s.y = job.y;
    s.voxels = uint32_t(job.num_voxels);
    s.chunks_per_member = uint32_t((job.num_voxels + size_t(threads * kLaneVoxels) - 1) / size_t(threads * kLaneVoxels));
    s.chunks = s.chunks_per_member * uint32_t(job.members);
    return s;
}

inline hipError_t compute_units(int* cus) {
    int device = 0;
    if (hipError_t e = hipGetDevice(&device); e != hipSuccess) return e;
    return hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, device);
}

// The persistent grid: at most `wanted` blocks, one per chunk if there are fewer.  CRF_SIMILARITY_MAX_BLOCKS (tests): a
// smaller cap, so that a small field takes several grid-stride rounds.
inline uint32_t grid_blocks(uint32_t chunks, int wanted) {
    const char* v = getenv("CRF_SIMILARITY_MAX_BLOCKS");
    const int cap = (v && *v) ? atoi(v) : 0;
    if (cap > 0) wanted = std::min(wanted, cap);
    return std::min<uint32_t>(chunks, uint32_t(wanted));
}

}  // namespace chunks
}  // namespace crf
