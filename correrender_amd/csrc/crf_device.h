// crf_device.h -- device-side building blocks shared by the gfx950 estimator kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "crf_binned_bins.h"  // bin_index_x86 and the per-sample bin of binned MI (host-usable)
#include "crf_exact_div.h"    // exact_div, exact_div_guard (host-usable)
#include "crf_internal.h"

namespace crf {

// Streaming member loads through buffer descriptors.  Member base pointers come out of a pointer table, so plain
// loads are flat/global loads with a 64-bit VGPR address each (two VGPRs + a 64-bit VALU add per load in flight).  A
// raw buffer load takes the wave-uniform base in a 128-bit SGPR descriptor and ONE shared 32-bit VGPR byte offset, and
// the hardware bounds check (num_records) makes lanes past the end of the volume read 0 instead of faulting, so the
// ragged tail needs no separate kernel.  aux = 2 is the non-temporal (`nt`) policy: every member value is read exactly
// once per evaluation and the ensemble dwarfs the 256 MiB Infinity Cache.  A member volume (or slab) is < 4 GiB
// (checked in crf_set_grid), so the 32-bit offset and num_records suffice.
typedef int32_t __attribute__((ext_vector_type(4))) buffer_rsrc_t;
#ifndef CRF_LOAD_AUX
#define CRF_LOAD_AUX 2
#endif
constexpr int kAuxNonTemporal = CRF_LOAD_AUX;  // buffer-load cache-policy bits: 1 = sc0, 2 = nt, 16 = sc1
__device__ __forceinline__ auto make_member_rsrc(const float* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), /*stride*/ short(0), int(bytes), 0x00020000);
}
template <class RSRC>
__device__ __forceinline__ float buffer_load_f32_nt(RSRC rsrc, uint32_t byte_offset) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, int(byte_offset), 0, kAuxNonTemporal));
}
// default cache policy through the same descriptor path: for values that are read again soon (kernels that re-read
// a voxel's members from L2 / Infinity Cache)
__device__ __forceinline__ float load_member_cached(const float* base, uint32_t bytes, uint32_t byte_offset) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(make_member_rsrc(base, bytes), int(byte_offset), 0, 0));
}
__device__ __forceinline__ float load_member_nt(const float* base, uint32_t bytes, uint32_t byte_offset) {
    return buffer_load_f32_nt(make_member_rsrc(base, bytes), byte_offset);
}
// One stored element of a member in a narrow native format, zero-extended: a byte / short buffer load (non-temporal like
// load_member_nt; the hardware bounds check makes an offset at or past `bytes` read 0 without a memory request).
// Sub-dword loads ask for nothing but the element's own alignment.
template <int FMT>
__device__ __forceinline__ uint32_t load_code_nt(const void* base, uint32_t bytes, uint32_t byte_offset) {
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), /*stride*/ short(0), int(bytes), 0x00020000);
    if constexpr (FMT == CRF_MEMBER_U8)
        return __builtin_amdgcn_raw_buffer_load_b8(rsrc, int(byte_offset), 0, kAuxNonTemporal);
    else
        return __builtin_amdgcn_raw_buffer_load_b16(rsrc, int(byte_offset), 0, kAuxNonTemporal);
}
// Result stores of the bandwidth-bound kernels: written once, never re-read by the kernel (non-temporal)
__device__ __forceinline__ void store_result_nt(float* p, float v) { __builtin_nontemporal_store(v, p); }

// Offset that is out of range for every member descriptor (num_records <= 4 * 2^30): a load through it returns 0
// without a memory request.  Padded slots of the guarded kernels select it (wave-uniform condition, one v_cndmask)
// instead of branching around the load or re-reading a valid member.
constexpr uint32_t kOutOfRangeOffset = 0xFFFFFFF0u;

// plain (cacheable) gather of one value: pair requests re-use voxels, so the default cache policy is kept
__device__ __forceinline__ float load_member(const float* base, uint32_t byte_offset) {
    typedef const float __attribute__((address_space(1)))* gptr;
    typedef const char __attribute__((address_space(1)))* gcptr;
    return *(gptr)((gcptr)base + byte_offset);
}

// One element of a member in a narrow native format as the value the calculators see (crf_internal.h; reference:
// HostCacheEntry.cpp:107-176).  `/` is the correctly rounded IEEE quotient (Makefile).
template <int FMT>
__device__ __forceinline__ float narrow_value(const void* base, size_t i) {
    static_assert(FMT == CRF_MEMBER_U8 || FMT == CRF_MEMBER_U16 || FMT == CRF_MEMBER_F16, "a narrow format");
    if constexpr (FMT == CRF_MEMBER_U8) {
        return float(static_cast<const uint8_t*>(base)[i]) / 255.0f;
    } else if constexpr (FMT == CRF_MEMBER_U16) {
        return float(static_cast<const uint16_t*>(base)[i]) / 65535.0f;
    } else {
        return float(static_cast<const _Float16*>(base)[i]);  // half denormals are fp32 normals: exact
    }
}

// The same values out of a member's dword, for the kernels whose lanes own the VPL = 4 (8-bit) or 2 (16-bit)
// consecutive voxels of one dword (kernels_pearson.hip: pearson_narrow_kernel, kernels_stats.hip): two voxels at a
// time in packed fp32.  The integer formats' x / 255.0f, x / 65535.0f is exact_div (below) with a compile-time
// reciprocal: x is an integer below 2^16 and the denominator a constant inside [2^-60, 2^60], its preconditions.
typedef float f2 __attribute__((ext_vector_type(2)));

template <int FMT>
constexpr int narrow_vpl() {
    return FMT == CRF_MEMBER_U8 ? 4 : 2;
}

// voxels 2 h and 2 h + 1 of the lane out of a member's dword
template <int FMT>
__device__ __forceinline__ f2 narrow_pair(uint32_t w, int h) {
    if constexpr (FMT == CRF_MEMBER_F16) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const h2 v = __builtin_bit_cast(h2, w);
        return f2{float(v[0]), float(v[1])};
    } else {
        constexpr float kDen = FMT == CRF_MEMBER_U8 ? 255.0f : 65535.0f;
        constexpr float kRcp = 1.0f / kDen;
        f2 x;
        if constexpr (FMT == CRF_MEMBER_U8) {
            x = f2{float((w >> (16 * h)) & 0xFFu), float((w >> (16 * h + 8)) & 0xFFu)};
        } else {
            x = f2{float(w & 0xFFFFu), float(w >> 16)};
        }
        const f2 rcp2 = {kRcp, kRcp}, den2 = {kDen, kDen};
        const f2 q0 = x * rcp2;
        const f2 rem = __builtin_elementwise_fma(-q0, den2, x);
        return __builtin_elementwise_fma(rem, rcp2, q0);
    }
}

__device__ __forceinline__ float load_ref(const RefSource& r, const float* const* __restrict__ members, int c) {
    if (r.values) return r.values[c];
    return (r.table ? r.table : members)[c][r.voxel];
}

// Compiler ordering fence on VALUES: an empty asm that "modifies" a and b makes everything computed from them
// afterwards wait for both, which pins phase order in the fully unrolled straight-line kernels (the machine
// scheduler otherwise hoists hundreds of independent address/mask computations and runs out of registers;
// __builtin_amdgcn_sched_barrier does not stop IR-level and DAG-level reordering of pure register code).
template <class A, class B>
__device__ __forceinline__ void order_after(A& a, B& b) {
    asm volatile("" : "+v"(a), "+v"(b));
}

// Order-preserving map float -> uint32 (a < b  <=>  key(a) < key(b) for non-NaN a, b; -0.0 must have been
// canonicalised to +0.0 by the caller with `y + 0.0f` so that key equality == float equality).
__device__ __forceinline__ uint32_t orderable_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u);
}

// Per-lane sorting networks over 64-bit (key, slot) composites held in registers (static indices only).
//
// A composite is built so that it is a POSITIVE NORMAL fp64 number whose numeric order equals the lexicographic
// (key, slot) order:   bits = 0x4000000000000000 | (uint64(key32) << 29) | low        (low < 2^29; slot in bits 0..7)
// bit 62 set and bit 61 clear keep the exponent field away from 0 (denormal) and 0x7FF (inf/NaN).  A compare-exchange
// is then exactly two VALU instructions, v_min_f64 + v_max_f64 (they return one of their operands bit for bit),
// instead of a 64-bit integer compare plus four conditional moves.  Inline asm because fmin()/fmax() add a
// canonicalising v_max_f64 x, x per operand.
typedef double composite_t;
__device__ __forceinline__ composite_t make_composite(uint32_t key32, uint32_t low) {
    const uint64_t bits = 0x4000000000000000ull | (uint64_t(key32) << 29) | uint64_t(low);
    return __longlong_as_double((long long)bits);
}
__device__ __forceinline__ uint32_t composite_key(composite_t c) {
    return uint32_t(uint64_t(__double_as_longlong(c)) >> 29);
}
__device__ __forceinline__ uint32_t composite_low(composite_t c) {
    return uint32_t(uint64_t(__double_as_longlong(c))) & 0x1FFFFFFFu;
}
__device__ __forceinline__ composite_t composite_or_low(composite_t c, uint32_t bits) {
    return __longlong_as_double(__double_as_longlong(c) | (long long)bits);
}

#define CRF_CE(i, j)                                                               \
    {                                                                              \
        composite_t lo_, hi_;                                                      \
        asm("v_min_f64 %0, %1, %2" : "=v"(lo_) : "v"(a[i]), "v"(a[j]));            \
        asm("v_max_f64 %0, %1, %2" : "=v"(hi_) : "v"(a[i]), "v"(a[j]));            \
        a[i] = lo_;                                                                \
        a[j] = hi_;                                                                \
    }
template <int N>
struct SortNet;
template <>
struct SortNet<8> {
    static __device__ __forceinline__ void sort(composite_t (&a)[8]) {
#define CRF_SORTNET_N 8
#include "sortnet.inc"
    }
};
template <>
struct SortNet<16> {
    static __device__ __forceinline__ void sort(composite_t (&a)[16]) {
#define CRF_SORTNET_N 16
#include "sortnet.inc"
    }
};
template <>
struct SortNet<32> {
    static __device__ __forceinline__ void sort(composite_t (&a)[32]) {
#define CRF_SORTNET_N 32
#include "sortnet.inc"
    }
};
template <>
struct SortNet<24> {
    static __device__ __forceinline__ void sort(composite_t (&a)[24]) {
#define CRF_SORTNET_N 24
#include "sortnet.inc"
    }
};
template <>
struct SortNet<40> {
    static __device__ __forceinline__ void sort(composite_t (&a)[40]) {
#define CRF_SORTNET_N 40
#include "sortnet.inc"
    }
};
template <>
struct SortNet<48> {
    static __device__ __forceinline__ void sort(composite_t (&a)[48]) {
#define CRF_SORTNET_N 48
#include "sortnet.inc"
    }
};
template <>
struct SortNet<56> {
    static __device__ __forceinline__ void sort(composite_t (&a)[56]) {
#define CRF_SORTNET_N 56
#include "sortnet.inc"
    }
};
template <>
struct SortNet<64> {
    static __device__ __forceinline__ void sort(composite_t (&a)[64]) {
#define CRF_SORTNET_N 64
#include "sortnet.inc"
    }
};
template <>
struct SortNet<80> {
    static __device__ __forceinline__ void sort(composite_t (&a)[80]) {
#define CRF_SORTNET_N 80
#include "sortnet.inc"
    }
};
template <>
struct SortNet<96> {
    static __device__ __forceinline__ void sort(composite_t (&a)[96]) {
#define CRF_SORTNET_N 96
#include "sortnet.inc"
    }
};
template <>
struct SortNet<112> {
    static __device__ __forceinline__ void sort(composite_t (&a)[112]) {
#define CRF_SORTNET_N 112
#include "sortnet.inc"
    }
};
template <>
struct SortNet<128> {
    static __device__ __forceinline__ void sort(composite_t (&a)[128]) {
#define CRF_SORTNET_N 128
#include "sortnet.inc"
    }
};
#undef CRF_CE

// Same networks over plain 32-bit keys (min/max: 2 VALU per exchange).
#define CRF_CE(i, j)                      \
    {                                     \
        const uint32_t lo_ = a[i], hi_ = a[j]; \
        a[i] = lo_ < hi_ ? lo_ : hi_;     \
        a[j] = lo_ < hi_ ? hi_ : lo_;     \
    }
template <int N>
struct SortNet32;
template <>
struct SortNet32<16> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[16]) {
#define CRF_SORTNET_N 16
#include "sortnet.inc"
    }
};
template <>
struct SortNet32<32> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[32]) {
#define CRF_SORTNET_N 32
#include "sortnet.inc"
    }
};
template <>
struct SortNet32<64> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[64]) {
#define CRF_SORTNET_N 64
#include "sortnet.inc"
    }
};
template <>
struct SortNet32<48> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[48]) {
#define CRF_SORTNET_N 48
#include "sortnet.inc"
    }
};
template <>
struct SortNet32<80> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[80]) {
#define CRF_SORTNET_N 80
#include "sortnet.inc"
    }
};
template <>
struct SortNet32<96> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[96]) {
#define CRF_SORTNET_N 96
#include "sortnet.inc"
    }
};
template <>
struct SortNet32<112> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[112]) {
#define CRF_SORTNET_N 112
#include "sortnet.inc"
    }
};
template <>
struct SortNet32<128> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[128]) {
#define CRF_SORTNET_N 128
#include "sortnet.inc"
    }
};
template <>
struct SortNet32<8> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[8]) {
#define CRF_SORTNET_N 8
#include "sortnet.inc"
    }
};
template <>
struct SortNet32<24> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[24]) {
#define CRF_SORTNET_N 24
#include "sortnet.inc"
    }
};
template <>
struct SortNet32<40> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[40]) {
#define CRF_SORTNET_N 40
#include "sortnet.inc"
    }
};
template <>
struct SortNet32<56> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[56]) {
#define CRF_SORTNET_N 56
#include "sortnet.inc"
    }
};
template <>
struct SortNet32<72> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[72]) {
#define CRF_SORTNET_N 72
#include "sortnet.inc"
    }
};
template <>
struct SortNet32<88> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[88]) {
#define CRF_SORTNET_N 88
#include "sortnet.inc"
    }
};
template <>
struct SortNet32<104> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[104]) {
#define CRF_SORTNET_N 104
#include "sortnet.inc"
    }
};
template <>
struct SortNet32<120> {
    static __device__ __forceinline__ void sort(uint32_t (&a)[120]) {
#define CRF_SORTNET_N 120
#include "sortnet.inc"
    }
};
#undef CRF_CE

// Ends a sorting network for the compiler: an empty asm "modifies" every element, so nothing that follows is mixed into the
// network's last stages.  Left alone the compiler starts the scans / searches that consume the sorted array while the last
// exchanges are still pending, the live ranges of both overlap, and a network over N values needs ~2N registers
// (spearman_u32_kernel: 116 B of scratch per lane at 128 members, 25.1 -> 21.5 ms at 512^3 x 128 once they were gone;
// mi_binned_kernel: 40 B of scratch at 64 / 128 members gone, three waves per SIMD instead of two at 96 members: 2.33 ->
// 2.15 ms at 256^3).  Measured neutral for the other rank kernels, slightly negative (+2 %) for the two-field kernels of
// kernels_symmetric*.hip, which therefore do without it.
template <class T, int N>
__device__ __forceinline__ void pin_array(T (&a)[N]) {
#pragma unroll
    for (int i = 0; i < N; i++) asm volatile("" : "+v"(a[i]));
}

// exact_div / exact_div_guard: crf_exact_div.h

// The value the calculators see of ONE stored code that a kernel holds in a register (load_code_nt): narrow_value's
// operations, the integer formats' quotient through exact_div with a compile-time reciprocal (an integer below 2^16 over
// a constant denominator: its preconditions).
template <int FMT>
__device__ __forceinline__ float narrow_code_value(uint32_t code) {
    if constexpr (FMT == CRF_MEMBER_F16) {
        return float(__builtin_bit_cast(_Float16, uint16_t(code)));
    } else {
        constexpr float kDen = FMT == CRF_MEMBER_U8 ? 255.0f : 65535.0f;
        return exact_div(float(code), kDen, 1.0f / kDen);  // == float(code) / kDen
    }
}

// One element of a member of ANY stored format, streamed once, as the value the calculators see: the front end of the
// kernels that are one template for all four formats (dkl_kernel, mi_kraskov_kernel) and the only place in them that knows
// how a member is stored, besides the element size (member_format_bytes(FMT)) behind their byte offsets.
template <int FMT>
__device__ __forceinline__ float member_value_nt(const void* base, uint32_t bytes, uint32_t byte_offset) {
    if constexpr (FMT == CRF_MEMBER_F32)
        return load_member_nt(static_cast<const float*>(base), bytes, byte_offset);
    else
        return narrow_code_value<FMT>(load_code_nt<FMT>(base, bytes, byte_offset));
}

// The voxel side of computePearson2<float> (Correlation.cpp:141-174) for one lane: y[0..cs) in registers, a_e =
// invNm1 * ((x_e - meanX) / sdX) prepared once per evaluation.  Sequential fp32, no contraction.
// SURE: slots 0..SURE-1 are members whatever cs is (the caller's contract), so only the slots behind them are guarded.
template <int N, bool EXACT, int SURE = 0>
__device__ __forceinline__ float pearson_tail(float (&y)[N], const float* __restrict__ prep_a, int cs) {
    const float n = float(cs);
    const float invN = 1.0f / n;
    const float invNm1 = 1.0f / (n - 1.0f);
    // Guarded use (cs < N), branch free: the caller passes y[e] = 0 and prep_a[e] = 0 for e >= cs and the deviation
    // of those slots is forced to 0, so every pass adds +0 for them (see pearson_reg_kernel).
    float meanY = 0.0f;
#pragma unroll
    for (int e = 0; e < N; e++) meanY += invN * y[e];
    float varY = 0.0f;
#pragma unroll
    for (int e = 0; e < N; e++) {
        const float d = (EXACT || e < SURE || e < cs) ? y[e] - meanY : 0.0f;
        y[e] = d;
        varY += invNm1 * d * d;
    }
    const float sdY = sqrtf(varY);
    float r = 0.0f;
    if (__all(exact_div_guard(meanY, sdY))) {
        const float rcp = 1.0f / sdY;
#pragma unroll
        for (int e = 0; e < N; e++) r += prep_a[e] * exact_div(y[e], sdY, rcp);
    } else {
#pragma unroll
        for (int e = 0; e < N; e++) r += prep_a[e] * ((EXACT || e < SURE || e < cs) ? y[e] / sdY : 0.0f);
    }
    return r;
}

}  // namespace crf
