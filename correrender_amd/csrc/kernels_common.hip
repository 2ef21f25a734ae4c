// kernels_common.hip -- small gfx950 helper kernels around the per-voxel estimators:
//   * reference-vector gather      (referenceValues[c] = fields[c][IDXS(ref)], CorrelationCalculator.cpp:802,815-817)
//   * member min/max reduction     (getMinMaxScalarFieldValue per member + min/max over members,
//                                   VolumeData.cpp:1632-1670, CorrelationCalculator.cpp:822-829)
//   * synthetic box-ensemble fill  (recipe of scripts/generate_synth_box_ensembles.py:57-136; input generation only)
#include <algorithm>
#include <type_traits>

#include "crf_device.h"
#include "crf_internal.h"

namespace crf {

// ---------------------------------------------------------------------------------------------------------
__global__ void gather_reference_kernel(const float* const* __restrict__ members, int cs, size_t voxel,
                                        float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < cs) out[c] = members[c][voxel];
}

hipError_t launch_gather_reference(const float* const* d_members, int cs, size_t voxel, float* d_out, hipStream_t s) {
    const int block = 64;
    hipLaunchKernelGGL(gather_reference_kernel, dim3((cs + block - 1) / block), dim3(block), 0, s, d_members, cs,
                       voxel, d_out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// Narrow member formats (crf_internal.h): the gather above with the conversion, and the fp32 copy of the members that
// every kernel but the native Pearson field reads.  The copy is written once per set of members; plain loads and stores.
template <int FMT>
__global__ void gather_reference_narrow_kernel(const void* const* __restrict__ members, int cs, size_t voxel,
                                               float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < cs) out[c] = narrow_value<FMT>(members[c], voxel);
}

hipError_t launch_gather_reference_narrow(const void* const* d_narrow, int format, int cs, size_t voxel, float* d_out,
                                          hipStream_t s) {
    const dim3 grid((cs + 63) / 64), block(64);
    switch (format) {
        case CRF_MEMBER_U8:
            hipLaunchKernelGGL(gather_reference_narrow_kernel<CRF_MEMBER_U8>, grid, block, 0, s, d_narrow, cs, voxel, d_out);
            break;
        case CRF_MEMBER_U16:
            hipLaunchKernelGGL(gather_reference_narrow_kernel<CRF_MEMBER_U16>, grid, block, 0, s, d_narrow, cs, voxel, d_out);
            break;
        case CRF_MEMBER_F16:
            hipLaunchKernelGGL(gather_reference_narrow_kernel<CRF_MEMBER_F16>, grid, block, 0, s, d_narrow, cs, voxel, d_out);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int FMT>
__global__ __launch_bounds__(256) void widen_members_kernel(const void* const* __restrict__ members, size_t num_voxels,
                                                            float* __restrict__ block, size_t stride) {
    const void* src = members[blockIdx.y];
    float* dst = block + size_t(blockIdx.y) * stride;
    for (size_t i = size_t(blockIdx.x) * 256 + threadIdx.x; i < num_voxels; i += size_t(gridDim.x) * 256)
        dst[i] = narrow_value<FMT>(src, i);
}

hipError_t launch_widen_members(const void* const* d_narrow, int format, int cs, size_t num_voxels, float* d_block,
                                size_t stride, hipStream_t s) {
    if (cs <= 0 || num_voxels == 0) return hipErrorInvalidValue;
    const size_t blocks = std::min<size_t>((num_voxels + 255) / 256, 8192);
    const dim3 grid{unsigned(blocks), unsigned(cs)}, block(256);
    switch (format) {
        case CRF_MEMBER_U8:
            hipLaunchKernelGGL(widen_members_kernel<CRF_MEMBER_U8>, grid, block, 0, s, d_narrow, num_voxels, d_block, stride);
            break;
        case CRF_MEMBER_U16:
            hipLaunchKernelGGL(widen_members_kernel<CRF_MEMBER_U16>, grid, block, 0, s, d_narrow, num_voxels, d_block, stride);
            break;
        case CRF_MEMBER_F16:
            hipLaunchKernelGGL(widen_members_kernel<CRF_MEMBER_F16>, grid, block, 0, s, d_narrow, num_voxels, d_block, stride);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// Rows of a batched reference-vector exchange (multi-GPU: one collective per several evaluations): row r receives the
// reference values of voxel[r], or zeros when voxel[r] == kNoVoxel (a point whose slice another rank owns) -- one
// launch instead of a memset plus one gather per owned row.
__global__ void gather_reference_rows_kernel(const float* const* __restrict__ members, int cs, GatherRows rows,
                                             float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (c < cs) {
        const size_t voxel = rows.voxel[r];
        out[size_t(r) * size_t(cs) + c] = voxel == kNoVoxel ? 0.0f : members[c][voxel];
    }
}

hipError_t launch_gather_reference_rows(const float* const* d_members, int cs, const GatherRows& rows, int num_rows,
                                        float* d_out, hipStream_t s) {
    if (num_rows <= 0) return hipSuccess;
    const int block = 64;
    hipLaunchKernelGGL(gather_reference_rows_kernel, dim3((cs + block - 1) / block, num_rows), dim3(block), 0, s,
                       d_members, cs, rows, d_out);
    return hipGetLastError();
}

template <int FMT>
__global__ void gather_reference_rows_narrow_kernel(const void* const* __restrict__ members, int cs, GatherRows rows,
                                                    float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (c < cs) {
        const size_t voxel = rows.voxel[r];
        out[size_t(r) * size_t(cs) + c] = voxel == kNoVoxel ? 0.0f : narrow_value<FMT>(members[c], voxel);
    }
}

hipError_t launch_gather_reference_rows_narrow(const void* const* d_narrow, int format, int cs, const GatherRows& rows,
                                               int num_rows, float* d_out, hipStream_t s) {
    if (num_rows <= 0) return hipSuccess;
    if (num_rows > kMaxGatherRows) return hipErrorInvalidValue;
    const dim3 grid((cs + 63) / 64, num_rows), block(64);
    switch (format) {
        case CRF_MEMBER_U8:
            hipLaunchKernelGGL(gather_reference_rows_narrow_kernel<CRF_MEMBER_U8>, grid, block, 0, s, d_narrow, cs, rows, d_out);
            break;
        case CRF_MEMBER_U16:
            hipLaunchKernelGGL(gather_reference_rows_narrow_kernel<CRF_MEMBER_U16>, grid, block, 0, s, d_narrow, cs, rows, d_out);
            break;
        case CRF_MEMBER_F16:
            hipLaunchKernelGGL(gather_reference_rows_narrow_kernel<CRF_MEMBER_F16>, grid, block, 0, s, d_narrow, cs, rows, d_out);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// Order-preserving float -> uint32 key so that unsigned atomicMin/atomicMax order like the floats do.
__device__ __forceinline__ uint32_t float_to_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
float minmax_key_to_float(uint32_t key) {
    const uint32_t b = (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
}

// grid = (blocks_per_member, cs).  Each block strides over one member with 16-byte loads; NaNs are skipped
// (fminf/fmaxf), one pair of atomics per wave.
__global__ __launch_bounds__(256) void minmax_kernel(const float* const* __restrict__ members, size_t num_voxels,
                                                     uint32_t* __restrict__ keys) {
    const float* __restrict__ p = members[blockIdx.y];
    float mn = INFINITY, mx = -INFINITY;
    const size_t n4 = num_voxels / 4;
    const bool aligned = (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
    const size_t stride = size_t(gridDim.x) * blockDim.x;
    const size_t t = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (aligned) {
        const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p);
        for (size_t i = t; i < n4; i += stride) {
            const float4 v = p4[i];
            mn = fminf(fminf(mn, v.x), fminf(v.y, fminf(v.z, v.w)));
            mx = fmaxf(fmaxf(mx, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
        }
        for (size_t i = n4 * 4 + t; i < num_voxels; i += stride) {
            mn = fminf(mn, p[i]);
            mx = fmaxf(mx, p[i]);
        }
    } else {
        for (size_t i = t; i < num_voxels; i += stride) {
            mn = fminf(mn, p[i]);
            mx = fmaxf(mx, p[i]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off, 64));
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (mn <= mx) {  // false only when every value seen was NaN / nothing was seen
            atomicMin(&keys[0], float_to_key(mn));
            atomicMax(&keys[1], float_to_key(mx));
        }
    }
}

__global__ void minmax_init_kernel(uint32_t* keys) {
    keys[0] = 0xFFFFFFFFu;
    keys[1] = 0u;
}

hipError_t launch_minmax(const float* const* d_members, int cs, size_t num_voxels, uint32_t* d_keys, hipStream_t s) {
    hipLaunchKernelGGL(minmax_init_kernel, dim3(1), dim3(1), 0, s, d_keys);
    size_t blocks = (num_voxels / 4 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 64) blocks = 64;  // 64 blocks x cs members >> 256 CUs
    hipLaunchKernelGGL(minmax_kernel, dim3(unsigned(blocks), unsigned(cs)), dim3(256), 0, s, d_members, num_voxels,
                       d_keys);
    return hipGetLastError();
}

// The extrema of members in a narrow native format, read as stored: the keys launch_minmax leaves for the converted
// values.  u8 / u16 reduce the integer codes and convert the two winners (the conversion is strictly increasing);
// float16 converts first, skips NaNs and reduces the fp32 kernel's keys, in which -0 orders below +0 exactly as in its
// fminf / fmaxf.  Same grid and atomics scheme as minmax_kernel.  Nothing is asked of the pointers beyond the element's
// own alignment: the elements before the first 16-byte boundary and behind the last whole 16 bytes are read one by one.
template <int FMT>
__global__ __launch_bounds__(256) void minmax_narrow_kernel(const void* const* __restrict__ members, size_t num_voxels,
                                                            uint32_t* __restrict__ keys) {
    typedef typename std::conditional<FMT == CRF_MEMBER_U8, uint8_t, uint16_t>::type elem_t;
    constexpr size_t kPerVector = 16 / sizeof(elem_t);
    const elem_t* __restrict__ p = static_cast<const elem_t*>(members[blockIdx.y]);
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;
    const auto see = [&mn, &mx](uint32_t code) {
        uint32_t k = code;
        if constexpr (FMT == CRF_MEMBER_F16) {
            const float f = float(__builtin_bit_cast(_Float16, uint16_t(code)));
            if (f != f) return;
            k = float_to_key(f);
        }
        mn = k < mn ? k : mn;
        mx = k > mx ? k : mx;
    };
    const uintptr_t address = reinterpret_cast<uintptr_t>(p);
    size_t head = ((16u - (address & 15u)) & 15u) / sizeof(elem_t);
    if (address % sizeof(elem_t) != 0 || head > num_voxels) head = num_voxels;  // (no 16-byte boundary to reach)
    const size_t vectors = (num_voxels - head) / kPerVector;
    const size_t stride = size_t(gridDim.x) * blockDim.x;
    const size_t t = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    for (size_t i = t; i < head; i += stride) see(p[i]);
    const uint4* __restrict__ p4 = reinterpret_cast<const uint4*>(p + head);
    for (size_t i = t; i < vectors; i += stride) {
        const uint4 v = p4[i];
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if constexpr (FMT == CRF_MEMBER_U8) {
                see(d[j] & 0xFFu);
                see((d[j] >> 8) & 0xFFu);
                see((d[j] >> 16) & 0xFFu);
                see(d[j] >> 24);
            } else {
                see(d[j] & 0xFFFFu);
                see(d[j] >> 16);
            }
        }
    }
    for (size_t i = head + vectors * kPerVector + t; i < num_voxels; i += stride) see(p[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t omn = __shfl_xor(mn, off, 64), omx = __shfl_xor(mx, off, 64);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
    }
    if ((threadIdx.x & 63) == 0 && mn <= mx) {  // false only when every value seen was NaN / nothing was seen
        if constexpr (FMT != CRF_MEMBER_F16) {
            const elem_t lo = elem_t(mn), hi = elem_t(mx);
            mn = float_to_key(narrow_value<FMT>(&lo, 0));
            mx = float_to_key(narrow_value<FMT>(&hi, 0));
        }
        atomicMin(&keys[0], mn);
        atomicMax(&keys[1], mx);
    }
}

hipError_t launch_minmax_narrow(const void* const* d_narrow, int format, int cs, size_t num_voxels, uint32_t* d_keys,
                                hipStream_t s) {
    if (cs <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(minmax_init_kernel, dim3(1), dim3(1), 0, s, d_keys);
    size_t blocks = (num_voxels * member_format_bytes(format) / 16 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 64) blocks = 64;
    const dim3 grid{unsigned(blocks), unsigned(cs)}, block(256);
    switch (format) {
        case CRF_MEMBER_U8: hipLaunchKernelGGL(minmax_narrow_kernel<CRF_MEMBER_U8>, grid, block, 0, s, d_narrow, num_voxels, d_keys); break;
        case CRF_MEMBER_U16: hipLaunchKernelGGL(minmax_narrow_kernel<CRF_MEMBER_U16>, grid, block, 0, s, d_narrow, num_voxels, d_keys); break;
        case CRF_MEMBER_F16: hipLaunchKernelGGL(minmax_narrow_kernel<CRF_MEMBER_F16>, grid, block, 0, s, d_narrow, num_voxels, d_keys); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// One member: every estimator's field is 1 by the reference's convention (CorrelationCalculator.cpp:882-885).
hipError_t launch_single_member(const RefSource& ref, float* d_out, size_t num_voxels, hipStream_t s,
                                hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info) {
    if (!ref.run()) return hipSuccess;
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    hipError_t e = launch_fill(d_out, num_voxels, 1.0f, s);
    if (ev_end) (void)hipEventRecord(ev_end, s);
    if (info) info->kernel_name = "fill_kernel";
    return e;
}

// ---------------------------------------------------------------------------------------------------------
// Synthetic "box ensemble".  lambda(x,y,z) = sum over 10 boxes of peak(chebyshev((x,y,z)-(cx,cy,zs/2)) / (size/2)),
// peak(u) = 0 for u >= 1 else 1 - max(0, 2|u|-1)^2  (generate_synth_box_ensembles.py:57-61,70-102, with g = xs/8
// for our grids; the original uses xs=ys=128, zs=32, g=16).  Sample of member c at a voxel:
// lambda*s1[c] + (1-lambda)*N(0,1) with s1 = 2*linspace(0,1,cs)-1 (:113-136).  The normal deviate comes from a
// counter-based hash of (seed, global voxel, member), so a z-slab generated on one rank equals the same slab of
// the whole grid generated elsewhere.
__device__ __forceinline__ float peak_fun(float u) {
    if (u >= 1.0f) return 0.0f;
    const float t = fmaxf(0.0f, fabsf(u) * 2.0f - 1.0f);
    return 1.0f - t * t;
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void synth_box_kernel(float* __restrict__ out, int xs, int ys, int zs_local,
                                                        int z_begin, int zs_global, int c, int cs, uint64_t seed) {
    const size_t n = size_t(xs) * ys * zs_local;
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int x = int(i % size_t(xs));
    const int y = int((i / size_t(xs)) % size_t(ys));
    const int z = int(i / (size_t(xs) * ys)) + z_begin;
    const float g = float(xs) / 8.0f;
    const float cz = float(zs_global / 2);
    // (cx, cy, size) in units of g
    const float boxes[10][3] = {{1.0f, 1.0f, 2.0f}, {7.0f, 7.0f, 2.0f}, {2.5f, 0.5f, 1.0f}, {2.5f, 1.5f, 1.0f},
                                {5.5f, 6.5f, 1.0f}, {5.5f, 7.5f, 1.0f}, {0.5f, 2.5f, 1.0f}, {1.5f, 2.5f, 1.0f},
                                {6.5f, 5.5f, 1.0f}, {7.5f, 5.5f, 1.0f}};
    float lambda = 0.0f;
#pragma unroll
    for (int b = 0; b < 10; b++) {
        const float dx = fabsf(float(x) - boxes[b][0] * g);
        const float dy = fabsf(float(y) - boxes[b][1] * g);
        const float dz = fabsf(float(z) - cz);
        const float dist = fmaxf(dx, fmaxf(dy, dz)) / (boxes[b][2] * g * 0.5f);
        lambda += peak_fun(dist);
    }
    lambda = fminf(lambda, 1.0f);
    const size_t gvoxel = (size_t(z) * ys + y) * size_t(xs) + x;
    const uint64_t h = mix64(seed ^ mix64(gvoxel * uint64_t(cs) + uint64_t(c)));
    const float u1 = (float(uint32_t(h >> 40)) + 0.5f) * (1.0f / 16777216.0f);          // (0,1)
    const float u2 = (float(uint32_t(h >> 8) & 0xFFFFFFu) + 0.5f) * (1.0f / 16777216.0f);  // (0,1)
    const float normal = sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
    const float s1 = cs > 1 ? 2.0f * (float(c) / float(cs - 1)) - 1.0f : -1.0f;
    out[i] = lambda * s1 + (1.0f - lambda) * normal;
}

hipError_t launch_synth_box_member(float* d_out, int xs, int ys, int zs_local, int z_begin, int zs_global, int c,
                                   int cs, uint64_t seed, hipStream_t s) {
    const size_t n = size_t(xs) * ys * zs_local;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(synth_box_kernel, dim3(unsigned(blocks)), dim3(256), 0, s, d_out, xs, ys, zs_local, z_begin,
                       zs_global, c, cs, seed);
    return hipGetLastError();
}

}  // namespace crf
