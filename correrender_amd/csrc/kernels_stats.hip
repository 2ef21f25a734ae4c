// kernels_stats.hip -- the sibling per-voxel ensemble reductions of the correlation path:
//   ensemble mean    EnsembleMeanCalculator::calculateCpu   (src/Calculators/EnsembleMeanCalculator.cpp:94-138)
//   ensemble spread  EnsembleSpreadCalculator::calculateCpu (src/Calculators/EnsembleSpreadCalculator.cpp:94-149)
//   set predicate    SetPredicateCalculator::calculateCpu   (src/Calculators/SetPredicateCalculator.cpp:154-210)
// plus the linear -> 8x8x4-tiled re-layout of a result field (VolumeData.cpp:1581-1621).
// Same access pattern and roofline as Pearson (cs member streams in, one float per voxel out, 4*cs + 4 bytes/voxel),
// same loader (buffer descriptors, shared 32-bit offset, non-temporal).  fp32, NaN values skipped, sums in member order
// exactly like the reference:  mean = (sum of valid) / numValid (NaN if none);  spread = sqrt( sum (mean - v)^2 /
// (numValid - 1) ) (NaN if fewer than two valid values).
#include <algorithm>

#include "crf_device.h"
#include "crf_internal.h"

namespace crf {

// kind 0: mean, 1: spread.  Members resident in registers (one voxel per lane), loops fully unrolled to CS_PAD.
template <int CS_PAD, int KIND>
__global__ __launch_bounds__(256) void ensemble_stat_reg_kernel(const float* const* __restrict__ members,
                                                                float* __restrict__ out, uint32_t num_voxels, int cs) {
    const uint32_t v0 = blockIdx.x * 256u + threadIdx.x;
    const uint32_t byte_offset = v0 * 4u, bytes = num_voxels * 4u;
    float y[CS_PAD];
#pragma unroll
    for (int e = 0; e < CS_PAD; e++)
        y[e] = load_member_nt(members[e < cs ? e : cs - 1], bytes, byte_offset);  // slots past cs re-read a valid member
    int num_valid = 0;
    float mean = 0.0f;
#pragma unroll
    for (int e = 0; e < CS_PAD; e++) {
        const bool ok = e < cs && !(y[e] != y[e]);
        mean = ok ? mean + y[e] : mean;
        num_valid += ok ? 1 : 0;
    }
    float res;
    if (KIND == 0) {
        res = num_valid >= 1 ? mean / float(num_valid) : __uint_as_float(0x7FC00000u);
    } else {
        mean = mean / float(num_valid);
        float var_sum = 0.0f;
#pragma unroll
        for (int e = 0; e < CS_PAD; e++) {
            const bool ok = e < cs && !(y[e] != y[e]);
            const float diff = mean - y[e];
            var_sum = ok ? var_sum + diff * diff : var_sum;
        }
        res = num_valid > 1 ? sqrtf(var_sum / float(num_valid - 1)) : __uint_as_float(0x7FC00000u);
    }
    if (v0 < num_voxels) store_result_nt(out + v0, res);
}

// Any member count: streaming passes (the spread re-reads the members once; mostly served by L2 / Infinity Cache).
template <int KIND>
__global__ __launch_bounds__(256) void ensemble_stat_stream_kernel(const float* const* __restrict__ members,
                                                                   float* __restrict__ out, uint32_t num_voxels, int cs) {
    const uint32_t v0 = blockIdx.x * 256u + threadIdx.x;
    const uint32_t byte_offset = v0 * 4u, bytes = num_voxels * 4u;
    int num_valid = 0;
    float mean = 0.0f;
#pragma unroll 16
    for (int e = 0; e < cs; e++) {
        const float v = load_member_nt(members[e], bytes, byte_offset);
        const bool ok = !(v != v);
        mean = ok ? mean + v : mean;
        num_valid += ok ? 1 : 0;
    }
    float res;
    if (KIND == 0) {
        res = num_valid >= 1 ? mean / float(num_valid) : __uint_as_float(0x7FC00000u);
    } else {
        mean = mean / float(num_valid);
        float var_sum = 0.0f;
#pragma unroll 16
        for (int e = 0; e < cs; e++) {
            const float v = load_member_nt(members[e], bytes, byte_offset);
            const float diff = mean - v;
            var_sum = !(v != v) ? var_sum + diff * diff : var_sum;
        }
        res = num_valid > 1 ? sqrtf(var_sum / float(num_valid - 1)) : __uint_as_float(0x7FC00000u);
    }
    if (v0 < num_voxels) store_result_nt(out + v0, res);
}

// Set predicate (SetPredicateCalculator::calculateCpu, src/Calculators/SetPredicateCalculator.cpp:154-210): count the
// members whose value satisfies `value OP comparison_value`, map the count to [0, 1] between countLower and
// countUpper.  One streaming pass, nothing to hold: 4*cs + 4 bytes per voxel.
template <int OP>
__device__ __forceinline__ bool set_predicate_compare(float a, float b) {
    if constexpr (OP == 0) return a > b;
    else if constexpr (OP == 1) return a >= b;
    else if constexpr (OP == 2) return a < b;
    else if constexpr (OP == 3) return a <= b;
    else if constexpr (OP == 4) return a == b;
    else return a != b;
}

template <int OP>
__global__ __launch_bounds__(256) void set_predicate_kernel(const float* const* __restrict__ members,
                                                            float* __restrict__ out, uint32_t num_voxels, int cs,
                                                            float comparison_value, int count_lower, int count_upper) {
    const uint32_t v0 = blockIdx.x * 256u + threadIdx.x;
    const uint32_t byte_offset = v0 * 4u, bytes = num_voxels * 4u;
    int count = 0;
#pragma unroll 16
    for (int e = 0; e < cs; e++)
        count += set_predicate_compare<OP>(load_member_nt(members[e], bytes, byte_offset), comparison_value) ? 1 : 0;
    float res = float(count) - float(count_lower);
    if (count_lower != count_upper) res = res / (float(count_upper) - float(count_lower));
    res = res < 0.0f ? 0.0f : (1.0f < res ? 1.0f : res);  // std::clamp: -0.0 stays -0.0
    if (v0 < num_voxels) store_result_nt(out + v0, res);
}

hipError_t launch_set_predicate(const float* const* d_members, int cs, size_t num_voxels, int op, float comparison_value,
                                int count_lower, int count_upper, float* d_out, hipStream_t s, hipEvent_t ev_begin,
                                hipEvent_t ev_end, LaunchInfo* info) {
    const unsigned blocks = unsigned((num_voxels + 255) / 256);
    const uint32_t n = uint32_t(num_voxels);
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
#define CRF_SETPRED(OP)                                                                                       \
    case OP:                                                                                                  \
        hipLaunchKernelGGL((set_predicate_kernel<OP>), dim3(blocks), dim3(256), 0, s, d_members, d_out, n, cs, \
                           comparison_value, count_lower, count_upper);                                       \
        break;
    switch (op) {
        CRF_SETPRED(0)
        CRF_SETPRED(1)
        CRF_SETPRED(2)
        CRF_SETPRED(3)
        CRF_SETPRED(4)
        CRF_SETPRED(5)
        default: return hipErrorInvalidValue;
    }
#undef CRF_SETPRED
    if (ev_end) (void)hipEventRecord(ev_end, s);
    if (info) info->kernel_name = "set_predicate_kernel";
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// Members in a narrow native format (crf_internal.h: u8, u16, f16), read as they are stored: element x cs + 4 bytes per
// voxel instead of 4 cs + 4, and no fp32 copy of the ensemble.  The scheme is pearson_narrow_kernel's
// (kernels_pearson.hip): one lane owns the VPL = 4 (8-bit) or 2 (16-bit) consecutive voxels of one dword, so a wave's
// load of one member is 256 contiguous bytes through a raw descriptor bounded to covered / VPL * 4 bytes (lanes past the
// end read 0 and store nothing), non-temporal; the caller passes `covered`, a multiple of VPL, and gives the up to
// VPL - 1 voxels behind the last whole dword to a one-wave tail kernel.  The arithmetic and its order are those of the
// fp32 kernels above on the converted values (crf_device.h: narrow_pair == narrow_value), two voxels at a time in packed
// fp32 -- the same IEEE operation per element, contraction off -- so every result equals the fp32 kernels' bit for bit.
// Only float16 can hold a NaN: the integer formats carry no valid-count.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t load_narrow_dword_nt(const void* base, uint32_t bytes, uint32_t byte_offset) {
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), short(0), int(bytes), 0x00020000);
    return __builtin_amdgcn_raw_buffer_load_b32(rsrc, int(byte_offset), 0, kAuxNonTemporal);
}

// a lane's VPL results: one vector store where `out` is aligned for it
template <int VPL>
__device__ __forceinline__ void store_lane_results(float* __restrict__ out, uint32_t v0, const float (&res)[VPL],
                                                   int out_vector) {
    if (out_vector) {
        typedef float fv __attribute__((ext_vector_type(VPL)));
        fv v;
#pragma unroll
        for (int i = 0; i < VPL; i++) v[i] = res[i];
        __builtin_nontemporal_store(v, reinterpret_cast<fv*>(out + v0));
    } else {
#pragma unroll
        for (int i = 0; i < VPL; i++) store_result_nt(out + v0 + i, res[i]);
    }
}

// the running sums of a lane's voxels (mean: the values; spread: the squared deviations) and their valid-counts
template <int FMT>
struct NarrowSums {
    static constexpr int VPL = narrow_vpl<FMT>(), P = VPL / 2;
    static constexpr bool kNaN = FMT == CRF_MEMBER_F16;
    f2 sum[P];
    int valid[VPL];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int p = 0; p < P; p++) sum[p] = f2{0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < VPL; i++) valid[i] = 0;
    }
    // sum += term for the voxels whose value y is no NaN
    __device__ __forceinline__ void add(int p, f2 y, f2 term, bool count) {
        const f2 t = sum[p] + term;
        if constexpr (kNaN) {
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const bool ok = !(y[i] != y[i]);
                sum[p][i] = ok ? t[i] : sum[p][i];
                if (count) valid[2 * p + i] += ok ? 1 : 0;
            }
        } else {
            sum[p] = t;
        }
    }
    __device__ __forceinline__ int num_valid(int i, int cs) const { return kNaN ? valid[i] : cs; }
};

// kind 0: mean, 1: spread.  CS_PAD > 0 (the spread up to 128 members): the cs raw dwords stay in registers across both
// passes and are converted on use -- CS_PAD registers for 2 or 4 voxels where ensemble_stat_reg_kernel holds cs per
// voxel; slots from CS_PAD - 16 on (all slots of the smallest instantiation) are stepped over in uniform branches, loads
// included.  CS_PAD == 0: streaming passes
// at any member count (the spread re-reads the members, the mean does not).
// The smallest register-resident instantiation of a format; every slot of it is guarded.  u8 starts at 48: its 16- and
// 32-slot instantiations come out of the compiler at 214 and 229 + 192 registers (one wave per SIMD), or with scratch
// under an occupancy request, where the 48-slot one takes 61 (tools/resource_usage.py).
constexpr int stat_narrow_smallest_pad(int format) { return format == CRF_MEMBER_U8 ? 48 : 16; }

template <int FMT, int CS_PAD, int KIND>
__global__ __launch_bounds__(256) void ensemble_stat_narrow_kernel(const void* const* __restrict__ members,
                                                                   float* __restrict__ out, uint32_t covered, int cs,
                                                                   int out_vector) {
    static_assert(CS_PAD == 0 || KIND == 1, "the mean needs one pass only: no reason to hold the dwords");
    constexpr int VPL = narrow_vpl<FMT>(), P = VPL / 2;
    constexpr int W = CS_PAD > 0 ? CS_PAD : 1;
    constexpr int kFirstGuarded = CS_PAD == stat_narrow_smallest_pad(FMT) ? 0 : CS_PAD - 16;
    const uint32_t dword = blockIdx.x * 256 + threadIdx.x;
    const uint32_t v0 = dword * VPL;
    const uint32_t byte_offset = dword * 4u;
    const uint32_t bytes = covered / VPL * 4u;
    int mine = cs;  // slot e is a member iff e < mine (laundered with the dwords, see pearson_narrow_kernel)
    const auto is_member = [&mine](int e) { return e < kFirstGuarded || e < mine; };
    uint32_t w[W];
    NarrowSums<FMT> acc;
    acc.clear();
    // pass 1: the sum of the valid values, in member order
    if constexpr (CS_PAD > 0) {
#pragma unroll
        for (int e = 0; e < CS_PAD; e++) {
            w[e] = 0u;
            if (is_member(e)) w[e] = load_narrow_dword_nt(members[e], bytes, byte_offset);  // uniform
        }
#pragma unroll
        for (int e = 0; e < CS_PAD; e++) {
#pragma unroll
            for (int p = 0; p < P; p++) {
                if (!is_member(e)) continue;  // uniform
                const f2 y = narrow_pair<FMT>(w[e], p);
                acc.add(p, y, y, true);
            }
            if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // (else the conversions of many slots run ahead)
        }
        // Laundered: left alone the compiler keeps the converted values of pass 1 for pass 2 -- cs x VPL registers,
        // the fp32 kernel's footprint, which is what this kernel exists to avoid.
#pragma unroll
        for (int e = 0; e < CS_PAD; e++) asm volatile("" : "+v"(w[e]));
        asm volatile("" : "+s"(mine));
    } else {
#pragma unroll 16
        for (int e = 0; e < cs; e++) {
            const uint32_t we = load_narrow_dword_nt(members[e], bytes, byte_offset);
#pragma unroll
            for (int p = 0; p < P; p++) {
                const f2 y = narrow_pair<FMT>(we, p);
                acc.add(p, y, y, true);
            }
        }
    }
    float res[VPL];
    f2 mean[P];
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const int nv = acc.num_valid(i, cs);
        const float m = acc.sum[i / 2][i % 2] / float(nv);
        mean[i / 2][i % 2] = m;
        res[i] = nv >= 1 ? m : __uint_as_float(0x7FC00000u);
    }
    if constexpr (KIND == 1) {
        // pass 2: the sum of (mean - v)^2 over the valid values, in member order
        NarrowSums<FMT> var;
        var.clear();
        if constexpr (CS_PAD > 0) {
#pragma unroll
            for (int e = 0; e < CS_PAD; e++) {
#pragma unroll
                for (int p = 0; p < P; p++) {
                    if (!is_member(e)) continue;  // uniform
                    const f2 y = narrow_pair<FMT>(w[e], p);
                    const f2 diff = mean[p] - y;
                    var.add(p, y, diff * diff, false);
                }
                if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll 16
            for (int e = 0; e < cs; e++) {
                const uint32_t we = load_narrow_dword_nt(members[e], bytes, byte_offset);
#pragma unroll
                for (int p = 0; p < P; p++) {
                    const f2 y = narrow_pair<FMT>(we, p);
                    const f2 diff = mean[p] - y;
                    var.add(p, y, diff * diff, false);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < VPL; i++) {
            const int nv = acc.num_valid(i, cs);
            res[i] = nv > 1 ? sqrtf(var.sum[i / 2][i % 2] / float(nv - 1)) : __uint_as_float(0x7FC00000u);
        }
    }
    if (v0 + VPL <= covered) store_lane_results<VPL>(out, v0, res, out_vector);
}

// the up to VPL - 1 voxels behind the last whole dword: ensemble_stat_stream_kernel on the converted values
template <int FMT, int KIND>
__global__ __launch_bounds__(64) void ensemble_stat_narrow_tail_kernel(const void* const* __restrict__ members,
                                                                       float* __restrict__ out, size_t voxel_offset,
                                                                       size_t voxel_end, int cs) {
    const size_t v0 = voxel_offset + threadIdx.x;
    if (v0 >= voxel_end) return;
    int num_valid = 0;
    float mean = 0.0f;
    for (int e = 0; e < cs; e++) {
        const float v = narrow_value<FMT>(members[e], v0);
        const bool ok = !(v != v);
        mean = ok ? mean + v : mean;
        num_valid += ok ? 1 : 0;
    }
    float res;
    if (KIND == 0) {
        res = num_valid >= 1 ? mean / float(num_valid) : __uint_as_float(0x7FC00000u);
    } else {
        mean = mean / float(num_valid);
        float var_sum = 0.0f;
        for (int e = 0; e < cs; e++) {
            const float v = narrow_value<FMT>(members[e], v0);
            const float diff = mean - v;
            var_sum = !(v != v) ? var_sum + diff * diff : var_sum;
        }
        res = num_valid > 1 ? sqrtf(var_sum / float(num_valid - 1)) : __uint_as_float(0x7FC00000u);
    }
    store_result_nt(out + v0, res);
}

__device__ __forceinline__ float set_predicate_result(int count, int count_lower, int count_upper) {
    float res = float(count) - float(count_lower);
    if (count_lower != count_upper) res = res / (float(count_upper) - float(count_lower));
    return res < 0.0f ? 0.0f : (1.0f < res ? 1.0f : res);  // std::clamp: -0.0 stays -0.0
}

template <int FMT, int OP>
__global__ __launch_bounds__(256) void set_predicate_narrow_kernel(const void* const* __restrict__ members,
                                                                   float* __restrict__ out, uint32_t covered, int cs,
                                                                   float comparison_value, int count_lower,
                                                                   int count_upper, int out_vector) {
    constexpr int VPL = narrow_vpl<FMT>(), P = VPL / 2;
    const uint32_t dword = blockIdx.x * 256 + threadIdx.x;
    const uint32_t v0 = dword * VPL;
    const uint32_t byte_offset = dword * 4u;
    const uint32_t bytes = covered / VPL * 4u;
    int count[VPL];
#pragma unroll
    for (int i = 0; i < VPL; i++) count[i] = 0;
#pragma unroll 16
    for (int e = 0; e < cs; e++) {
        const uint32_t we = load_narrow_dword_nt(members[e], bytes, byte_offset);
#pragma unroll
        for (int p = 0; p < P; p++) {
            const f2 y = narrow_pair<FMT>(we, p);
#pragma unroll
            for (int i = 0; i < 2; i++) count[2 * p + i] += set_predicate_compare<OP>(y[i], comparison_value) ? 1 : 0;
        }
    }
    float res[VPL];
#pragma unroll
    for (int i = 0; i < VPL; i++) res[i] = set_predicate_result(count[i], count_lower, count_upper);
    if (v0 + VPL <= covered) store_lane_results<VPL>(out, v0, res, out_vector);
}

template <int FMT, int OP>
__global__ __launch_bounds__(64) void set_predicate_narrow_tail_kernel(const void* const* __restrict__ members,
                                                                       float* __restrict__ out, size_t voxel_offset,
                                                                       size_t voxel_end, int cs, float comparison_value,
                                                                       int count_lower, int count_upper) {
    const size_t v0 = voxel_offset + threadIdx.x;
    if (v0 >= voxel_end) return;
    int count = 0;
    for (int e = 0; e < cs; e++)
        count += set_predicate_compare<OP>(narrow_value<FMT>(members[e], v0), comparison_value) ? 1 : 0;
    store_result_nt(out + v0, set_predicate_result(count, count_lower, count_upper));
}

namespace {
template <int FMT, int CS_PAD, int KIND>
void launch_stat_narrow_main(const void* const* d_narrow, float* d_out, size_t covered, int cs, bool out_vector,
                             hipStream_t s) {
    const size_t per_block = size_t(256) * narrow_vpl<FMT>();
    hipLaunchKernelGGL((ensemble_stat_narrow_kernel<FMT, CS_PAD, KIND>), dim3(unsigned((covered + per_block - 1) / per_block)),
                       dim3(256), 0, s, d_narrow, d_out, uint32_t(covered), cs, out_vector ? 1 : 0);
}

template <int FMT>
void launch_stat_narrow_format(int kind, const void* const* d_narrow, float* d_out, size_t num_voxels, int cs,
                               hipStream_t s) {
    constexpr int VPL = narrow_vpl<FMT>();
    const size_t covered = num_voxels / VPL * VPL;
    const bool out_vector = reinterpret_cast<uintptr_t>(d_out) % (VPL * sizeof(float)) == 0;
    if (covered > 0) {
        if (kind == 0) {
            launch_stat_narrow_main<FMT, 0, 0>(d_narrow, d_out, covered, cs, out_vector, s);
        } else if (cs > kNarrowMaxMembers) {
            launch_stat_narrow_main<FMT, 0, 1>(d_narrow, d_out, covered, cs, out_vector, s);
        } else {
            constexpr int kSmallest = stat_narrow_smallest_pad(FMT);
            switch (std::max((cs + 15) / 16 * 16, kSmallest)) {
                case 16: launch_stat_narrow_main<FMT, kSmallest, 1>(d_narrow, d_out, covered, cs, out_vector, s); break;
                case 32: launch_stat_narrow_main<FMT, kSmallest < 32 ? 32 : kSmallest, 1>(d_narrow, d_out, covered, cs, out_vector, s); break;
                case 48: launch_stat_narrow_main<FMT, 48, 1>(d_narrow, d_out, covered, cs, out_vector, s); break;
                case 64: launch_stat_narrow_main<FMT, 64, 1>(d_narrow, d_out, covered, cs, out_vector, s); break;
                case 80: launch_stat_narrow_main<FMT, 80, 1>(d_narrow, d_out, covered, cs, out_vector, s); break;
                case 96: launch_stat_narrow_main<FMT, 96, 1>(d_narrow, d_out, covered, cs, out_vector, s); break;
                case 112: launch_stat_narrow_main<FMT, 112, 1>(d_narrow, d_out, covered, cs, out_vector, s); break;
                default: launch_stat_narrow_main<FMT, 128, 1>(d_narrow, d_out, covered, cs, out_vector, s); break;
            }
        }
    }
    if (covered < num_voxels) {
        if (kind == 0)
            hipLaunchKernelGGL((ensemble_stat_narrow_tail_kernel<FMT, 0>), dim3(1), dim3(64), 0, s, d_narrow, d_out, covered,
                               num_voxels, cs);
        else
            hipLaunchKernelGGL((ensemble_stat_narrow_tail_kernel<FMT, 1>), dim3(1), dim3(64), 0, s, d_narrow, d_out, covered,
                               num_voxels, cs);
    }
}

template <int FMT, int OP>
void launch_predicate_narrow_op(const void* const* d_narrow, float* d_out, size_t num_voxels, int cs, float comparison_value,
                                int count_lower, int count_upper, hipStream_t s) {
    constexpr int VPL = narrow_vpl<FMT>();
    const size_t covered = num_voxels / VPL * VPL, per_block = size_t(256) * VPL;
    const bool out_vector = reinterpret_cast<uintptr_t>(d_out) % (VPL * sizeof(float)) == 0;
    if (covered > 0)
        hipLaunchKernelGGL((set_predicate_narrow_kernel<FMT, OP>), dim3(unsigned((covered + per_block - 1) / per_block)),
                           dim3(256), 0, s, d_narrow, d_out, uint32_t(covered), cs, comparison_value, count_lower,
                           count_upper, out_vector ? 1 : 0);
    if (covered < num_voxels)
        hipLaunchKernelGGL((set_predicate_narrow_tail_kernel<FMT, OP>), dim3(1), dim3(64), 0, s, d_narrow, d_out, covered,
                           num_voxels, cs, comparison_value, count_lower, count_upper);
}

template <int FMT>
bool launch_predicate_narrow_format(int op, const void* const* d_narrow, float* d_out, size_t num_voxels, int cs,
                                    float comparison_value, int count_lower, int count_upper, hipStream_t s) {
#define CRF_SETPRED(OP)                                                                                              \
    case OP:                                                                                                         \
        launch_predicate_narrow_op<FMT, OP>(d_narrow, d_out, num_voxels, cs, comparison_value, count_lower, count_upper, s); \
        return true;
    switch (op) {
        CRF_SETPRED(0)
        CRF_SETPRED(1)
        CRF_SETPRED(2)
        CRF_SETPRED(3)
        CRF_SETPRED(4)
        CRF_SETPRED(5)
        default: return false;
    }
#undef CRF_SETPRED
}

bool narrow_launchable(int format, int cs, size_t num_voxels) {
    return cs >= 1 && num_voxels > 0 && (format == CRF_MEMBER_U8 || format == CRF_MEMBER_U16 || format == CRF_MEMBER_F16) &&
           num_voxels * member_format_bytes(format) < kNarrowMaxBytes;
}
}  // namespace

hipError_t launch_ensemble_stat_narrow(int kind, const void* const* d_narrow, int format, int cs, size_t num_voxels,
                                       float* d_out, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end,
                                       LaunchInfo* info) {
    if (!narrow_launchable(format, cs, num_voxels) || (kind != 0 && kind != 1)) return hipErrorInvalidValue;
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    switch (format) {
        case CRF_MEMBER_U8: launch_stat_narrow_format<CRF_MEMBER_U8>(kind, d_narrow, d_out, num_voxels, cs, s); break;
        case CRF_MEMBER_U16: launch_stat_narrow_format<CRF_MEMBER_U16>(kind, d_narrow, d_out, num_voxels, cs, s); break;
        default: launch_stat_narrow_format<CRF_MEMBER_F16>(kind, d_narrow, d_out, num_voxels, cs, s); break;
    }
    if (ev_end) (void)hipEventRecord(ev_end, s);
    if (info) info->kernel_name = "ensemble_stat_narrow_kernel";
    return hipGetLastError();
}

hipError_t launch_set_predicate_narrow(const void* const* d_narrow, int format, int cs, size_t num_voxels, int op,
                                       float comparison_value, int count_lower, int count_upper, float* d_out,
                                       hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info) {
    if (!narrow_launchable(format, cs, num_voxels) || op < 0 || op > 5) return hipErrorInvalidValue;
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    switch (format) {
        case CRF_MEMBER_U8:
            launch_predicate_narrow_format<CRF_MEMBER_U8>(op, d_narrow, d_out, num_voxels, cs, comparison_value, count_lower, count_upper, s);
            break;
        case CRF_MEMBER_U16:
            launch_predicate_narrow_format<CRF_MEMBER_U16>(op, d_narrow, d_out, num_voxels, cs, comparison_value, count_lower, count_upper, s);
            break;
        default:
            launch_predicate_narrow_format<CRF_MEMBER_F16>(op, d_narrow, d_out, num_voxels, cs, comparison_value, count_lower, count_upper, s);
            break;
    }
    if (ev_end) (void)hipEventRecord(ev_end, s);
    if (info) info->kernel_name = "set_predicate_narrow_kernel";
    return hipGetLastError();
}

// Linear IDXS order -> the 8x8x4-tiled buffer layout of the reference's device field cache (VolumeData.cpp:1581-1621,
// IDXS of Data/Shaders/Correlation/ScalarFields.glsl:32-50): tiles in x-fastest tile order, x-fastest inside a tile,
// the grid padded up to whole tiles with zeros.  One wave writes one 256-B row of 64 tiled elements.
__global__ __launch_bounds__(256) void tile_field_kernel(const float* __restrict__ linear, float* __restrict__ tiled,
                                                         uint32_t xs, uint32_t ys, uint32_t zs, uint32_t xst,
                                                         uint32_t yst, size_t num_tiled) {
    const size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= num_tiled) return;
    const uint32_t tile = uint32_t(i >> 8), voxel = uint32_t(i & 255u);
    const uint32_t xt = tile % xst, yt = (tile / xst) % yst, zt = tile / (xst * yst);
    const uint32_t x = (voxel & 7u) + xt * 8u, y = ((voxel >> 3) & 7u) + yt * 8u, z = (voxel >> 6) + zt * 4u;
    float value = 0.0f;
    if (x < xs && y < ys && z < zs) value = linear[(size_t(z) * ys + y) * xs + x];
    tiled[i] = value;
}

hipError_t launch_tile_field(const float* d_linear, float* d_tiled, int xs, int ys, int zs, hipStream_t s) {
    const uint32_t xst = (uint32_t(xs) + 7u) / 8u, yst = (uint32_t(ys) + 7u) / 8u, zst = (uint32_t(zs) + 3u) / 4u;
    const size_t num_tiled = size_t(xst) * yst * zst * 256;
    hipLaunchKernelGGL(tile_field_kernel, dim3(unsigned((num_tiled + 255) / 256)), dim3(256), 0, s, d_linear, d_tiled,
                       uint32_t(xs), uint32_t(ys), uint32_t(zs), xst, yst, num_tiled);
    return hipGetLastError();
}

hipError_t launch_ensemble_stat(int kind, const float* const* d_members, int cs, size_t num_voxels, float* d_out,
                                hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info) {
    const unsigned blocks = unsigned((num_voxels + 255) / 256);
    const uint32_t n = uint32_t(num_voxels);
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
#define CRF_STAT(CSP)                                                                                              \
    if (kind == 0)                                                                                                 \
        hipLaunchKernelGGL((ensemble_stat_reg_kernel<CSP, 0>), dim3(blocks), dim3(256), 0, s, d_members, d_out, n, cs); \
    else                                                                                                           \
        hipLaunchKernelGGL((ensemble_stat_reg_kernel<CSP, 1>), dim3(blocks), dim3(256), 0, s, d_members, d_out, n, cs);
    if (kind == 0 || cs > 128) {  // the mean needs one pass only: no reason to hold the values
        if (kind == 0)
            hipLaunchKernelGGL((ensemble_stat_stream_kernel<0>), dim3(blocks), dim3(256), 0, s, d_members, d_out, n, cs);
        else
            hipLaunchKernelGGL((ensemble_stat_stream_kernel<1>), dim3(blocks), dim3(256), 0, s, d_members, d_out, n, cs);
        if (info) info->kernel_name = "ensemble_stat_stream_kernel";
    } else {
        if (cs <= 16) {
            CRF_STAT(16)
        } else if (cs <= 32) {
            CRF_STAT(32)
        } else if (cs <= 64) {
            CRF_STAT(64)
        } else {
            CRF_STAT(128)
        }
        if (info) info->kernel_name = "ensemble_stat_reg_kernel";
    }
#undef CRF_STAT
    if (ev_end) (void)hipEventRecord(ev_end, s);
    return hipGetLastError();
}

}  // namespace crf
