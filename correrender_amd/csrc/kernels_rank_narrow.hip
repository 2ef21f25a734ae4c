// kernels_rank_narrow.hip -- the two rank estimators, Kendall tau-b (2..128 members) and Spearman (33..128), on members
// stored as uint8, uint16 or float16, read as stored.
//
// The fp32 kernels (kernels_rank.hip) sort 64-bit (key, slot) composites, and from 17 members on they run a tie-free first
// pass that defers every voxel with two equal values to a one-wave-per-SIMD list kernel.  Quantised members are exactly
// the data that ties (u8 at 64 members: every voxel), and they need far fewer bits: the rank estimators use only the order
// and the ties of a voxel's values, and an order-preserving key of the stored CODE has 17 bits (crf_narrow_keys.h).  Key
// above a 7-bit slot is one uint32_t with nothing dropped -- no close-pair repair as in spearman_u32_kernel -- so ONE
// Batcher network over u32 min / max sorts the voxel in N registers, and kendall_kernel's walk, or spearman_kernel's two
// tie-run scans, handle ties in line.  One kernel per estimator, one pass, no todo list, no workspace, no fp32 copy of the
// members.
//
// Mapping as in kernels_rank.hip: one lane per voxel, a wave load = 64 consecutive elements of one member; the reference
// side is fp32 with any values.  Kendall loads the members in reference-sorted order (kendall_prep_kernel's permutation),
// Spearman in member order: its ranks go through the lane's LDS column back into member order for the Pearson tail.
// Results are bit-identical to kendall_kernel / spearman_kernel on the converted values: the integer counts and ranks are
// the same and the fp32 tail is the same code.
#include "crf_device.h"
#include "crf_internal.h"
#include "crf_narrow_keys.h"

namespace crf {

// (one stored element per load: load_code_nt, crf_device.h)
// The front end a rank kernel over narrow members needs: a[p] = the voxel's (key, slot) composites in ascending order.
// Slot e holds member perm[e] (PERMUTED) or member e.  N - 8 < cs <= N: the first N - 8 slots are members whatever cs is
// and carry no guard; a slot past cs loads at kOutOfRangeOffset and gets the pad key, so the pads end up behind the cs
// real elements in slot order.  All loads are issued before the first use.
template <int FMT, int N, bool PERMUTED>
__device__ __forceinline__ void narrow_sorted_composites(uint32_t (&a)[N], const void* const* __restrict__ members,
                                                         const int* __restrict__ perm, int cs, uint32_t bytes,
                                                         uint32_t byte_offset) {
    constexpr int SURE = N - 8;
#pragma unroll
    for (int e = 0; e < N; e++) {
        const bool real = e < SURE || e < cs;
        const int member = PERMUTED ? perm[e] : (real ? e : cs - 1);  // (perm of a pad: member 0)
        a[e] = load_code_nt<FMT>(members[member], bytes, real ? byte_offset : kOutOfRangeOffset);
    }
#pragma unroll
    for (int e = 0; e < N; e++)
        a[e] = narrow_composite((e < SURE || e < cs) ? narrow_key<FMT>(a[e]) : kNarrowPadKey, uint32_t(e));
    __builtin_amdgcn_sched_barrier(0);
    SortNet32<N>::sort(a);
    pin_array(a);  // the network ends here (crf_device.h)
    __builtin_amdgcn_sched_barrier(0);
}

// a NaN among the voxel's values: the smallest key, or the largest REAL key (position cs - 1, one of the last 8)
template <int FMT, int N>
__device__ __forceinline__ bool narrow_sorted_hold_nan(const uint32_t (&a)[N], int cs) {
    bool is_nan = narrow_key_is_nan<FMT>(narrow_composite_key(a[0]));
    if constexpr (FMT == CRF_MEMBER_F16) {
#pragma unroll
        for (int p = (N > 8 ? N - 8 : 1); p < N; p++)
            is_nan |= p == cs - 1 && narrow_key_is_nan<FMT>(narrow_composite_key(a[p]));
    }
    return is_nan;
}

// waves per SIMD the register budget is set for: N composites plus ~40 registers of the walk, no scratch in any
// instantiation (tools/resource_usage.py; table in profiles/narrow_kendall_ab.md)
constexpr int kendall_narrow_waves(int n) {
    return n <= 32 ? 8 : n == 40 ? 7 : n == 48 ? 4 : n == 56 ? 5 : n <= 72 ? 4 : n <= 88 ? 3 : 2;  // (48 needs more than 56)
}

// N - 8 < cs <= N; the prep tables (kendall_prep_kernel) have the stride NPAD = pad_pow2(cs) = pad_pow2(N)
template <int FMT, int N>
__global__ __launch_bounds__(64, kendall_narrow_waves(N)) void kendall_narrow_kernel(
    const void* const* __restrict__ members, const int* __restrict__ prep, float* __restrict__ out, size_t num_voxels,
    int cs) {
    static_assert(N % 8 == 0 && N <= (1 << kNarrowSlotBits), "slots are 7 bits");
    constexpr int NPAD = pad_pow2(N);
    constexpr uint32_t kElement = FMT == CRF_MEMBER_U8 ? 1u : 2u;
    __shared__ uint8_t gend_lds[N];
    const int lane = threadIdx.x;
    const bool x_ties = prep[2 * NPAD + 1] != 0;  // wave-uniform
    if (x_ties) {
        for (int i = lane; i < N; i += 64) gend_lds[i] = uint8_t(prep[NPAD + i]);
        __syncthreads();
    }
    const size_t v = size_t(blockIdx.x) * 64 + lane;
    const bool active = v < num_voxels;  // inactive lanes are out of range: they read 0 and store nothing
    const uint32_t bytes = uint32_t(num_voxels) * kElement, byte_offset = uint32_t(v) * kElement;

    uint32_t a[N];
    narrow_sorted_composites<FMT, N, true>(a, members, prep, cs, bytes, byte_offset);
    const bool is_nan = narrow_sorted_hold_nan<FMT, N>(a, cs);

    // kendall_kernel's walk.  The pads sort behind the cs real elements in slot order, so when one is visited every seen
    // slot is below it -- it adds no discordant pair; its tie run is masked out of n2.
    constexpr int SURE = N - 8;
    constexpr int W = (N + 63) / 64;
    constexpr bool SMALL = N <= 32;  // slots 0..31: a 32-bit set (one shift, and, popcount, or each)
    uint64_t seen[W];
#pragma unroll
    for (int w = 0; w < W; w++) seen[w] = 0ull;
    uint32_t seen32 = 0u;
    int32_t discordant = 0, n2 = 0, run = 0;
    constexpr int G = 8;  // positions per group: their x-tie group ends are read from LDS together, then consumed
#pragma unroll
    for (int p0 = 0; p0 < N; p0 += G) {
        uint32_t slot[G], g[G];  // g: last slot with the same x (pads: themselves)
#pragma unroll
        for (int i = 0; i < G; i++) slot[i] = g[i] = narrow_composite_slot(a[p0 + i]);
        if (x_ties) {
#pragma unroll
            for (int i = 0; i < G; i++) g[i] = uint32_t(gend_lds[slot[i]]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < G; i++) {
            const int p = p0 + i;
            // ties in y: a run of t equal values contributes 0+1+...+(t-1) = t(t-1)/2
            if (p > 0) {
                const bool same = (a[p] ^ a[p - 1]) < (1u << kNarrowSlotBits);
                run = ((p < SURE || p < cs) && same) ? run + 1 : 0;
                n2 += run;
            }
            // already-seen slots (smaller y, or equal y and smaller slot) with strictly larger x: slot' > g
            if constexpr (SMALL) {
                discordant += __popc(seen32 & (0xFFFFFFFEu << g[i]));
                seen32 |= 1u << slot[i];
            } else if constexpr (W == 1) {
                discordant += __popcll(seen[0] & (0xFFFFFFFFFFFFFFFEull << g[i]));
                seen[0] |= 1ull << slot[i];
            } else {
                const uint64_t gm = 0xFFFFFFFFFFFFFFFEull << (g[i] & 63u);
                const uint64_t sbit = 1ull << (slot[i] & 63u);
#pragma unroll
                for (int w = 0; w < W; w++) {
                    const uint64_t mask = (uint32_t(w) > (g[i] >> 6)) ? ~0ull : ((uint32_t(w) == (g[i] >> 6)) ? gm : 0ull);
                    discordant += __popcll(seen[w] & mask);
                    seen[w] |= (uint32_t(w) == (slot[i] >> 6)) ? sbit : 0ull;
                }
            }
        }
        // the group ends here for the compiler: left alone it forms the seen sets of every position first and counts
        // afterwards, one live set per position (0.5-2.4 KB of scratch per lane)
        if constexpr (SMALL) {
            order_after(discordant, seen32);
        } else {
#pragma unroll
            for (int w = 0; w < W; w++) order_after(discordant, seen[w]);
        }
        order_after(n2, run);
        __builtin_amdgcn_sched_barrier(0);
    }
    const int32_t n = cs;
    const int32_t n0 = (n * (n - 1)) / 2;
    const int32_t n1 = prep[2 * NPAD];
    const int32_t numerator = n0 - n1 - n2 - 2 * discordant;
    const float denominator = sqrtf(float(n0 - n1)) * sqrtf(float(n0 - n2));
    float res = float(numerator) / denominator;
    if (is_nan) res = __uint_as_float(0x7FC00000u);
    if (active) store_result_nt(out + v, res);
}

namespace {

using NarrowKendallKernel = void (*)(const void* const*, const int*, float*, size_t, int);

template <int FMT>
NarrowKendallKernel kendall_narrow_for(int cs) {
    switch ((cs + 7) / 8 * 8) {
        case 8: return kendall_narrow_kernel<FMT, 8>;
        case 16: return kendall_narrow_kernel<FMT, 16>;
        case 24: return kendall_narrow_kernel<FMT, 24>;
        case 32: return kendall_narrow_kernel<FMT, 32>;
        case 40: return kendall_narrow_kernel<FMT, 40>;
        case 48: return kendall_narrow_kernel<FMT, 48>;
        case 56: return kendall_narrow_kernel<FMT, 56>;
        case 64: return kendall_narrow_kernel<FMT, 64>;
        case 72: return kendall_narrow_kernel<FMT, 72>;
        case 80: return kendall_narrow_kernel<FMT, 80>;
        case 88: return kendall_narrow_kernel<FMT, 88>;
        case 96: return kendall_narrow_kernel<FMT, 96>;
        case 104: return kendall_narrow_kernel<FMT, 104>;
        case 112: return kendall_narrow_kernel<FMT, 112>;
        case 120: return kendall_narrow_kernel<FMT, 120>;
        default: return kendall_narrow_kernel<FMT, 128>;
    }
}

}  // namespace

hipError_t launch_kendall_narrow(const void* const* d_narrow, int format, int cs, size_t num_voxels, const RefSource& ref,
                                 float* d_prep, float* d_out, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end,
                                 LaunchInfo* info) {
    if (cs < 2 || cs > kNarrowMaxMembers || format == CRF_MEMBER_F32 ||
        num_voxels * member_format_bytes(format) >= kNarrowMaxBytes || (ref.prepare() && !ref.values))
        return hipErrorInvalidValue;
    int* prep = reinterpret_cast<int*>(d_prep);
    if (ref.prepare()) launch_kendall_prep(ref, nullptr, cs, pad_pow2(cs), prep, s);
    if (!ref.run()) return hipGetLastError();
    const NarrowKendallKernel k = format == CRF_MEMBER_U8    ? kendall_narrow_for<CRF_MEMBER_U8>(cs)
                                  : format == CRF_MEMBER_U16 ? kendall_narrow_for<CRF_MEMBER_U16>(cs)
                                                             : kendall_narrow_for<CRF_MEMBER_F16>(cs);
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    hipLaunchKernelGGL(k, dim3(unsigned((num_voxels + 63) / 64)), dim3(64), 0, s, d_narrow, prep, d_out, num_voxels, cs);
    if (ev_end) (void)hipEventRecord(ev_end, s);
    if (info) info->kernel_name = "kendall_narrow_kernel";
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// Spearman
// ---------------------------------------------------------------------------------------------------------
// waves per SIMD the register budget is set for: N composites, then N ranks, plus ~30 registers; no scratch in any
// instantiation (tools/resource_usage.py; table in profiles/narrow_spearman_ab.md; N = 88 at three waves spilled 12 B).
// The byte column in LDS (N * 64 bytes per wave) never sets the occupancy: 4 SIMDs x waves x N x 64 B is 80 KB at most
// (N = 64 where its 96 registers allow five waves) of the CU's 160 KB.
constexpr int spearman_narrow_waves(int n) {
    return n == 40 ? 7 : n == 48 ? 4 : n == 56 ? 5 : n <= 72 ? 4 : n == 80 ? 3 : 2;  // (48: its network needs more than 56's)
}

// 33..128 members, N - 8 < cs <= N, members in member order (the tail runs in member order); prep is
// spearman_prep_kernel's table (0 behind cs).  spearman_kernel's two scans over the sorted registers, its arithmetic and
// its tail: bit-identical to it on the converted values.  The composite has 24 significant bits, so the forward scan parks
// a position's run start in the byte above them, and "the run of p + 1 started before it" tells the backward scan that p
// and p + 1 hold equal keys without another comparison.
template <int FMT, int N>
__global__ __launch_bounds__(64, spearman_narrow_waves(N)) void spearman_narrow_kernel(
    const void* const* __restrict__ members, const float* __restrict__ prep, float* __restrict__ out, size_t num_voxels,
    int cs) {
    static_assert(N % 8 == 0 && N >= 40 && N <= (1 << kNarrowSlotBits), "slots are 7 bits; up to 32 members: the fp32 copy");
    static_assert(kNarrowSlotBits + 17 <= 24 && 2 * (N - 1) <= 255, "run start above the composite; start + end in a byte");
    constexpr int SURE = N - 8;
    constexpr uint32_t kElement = FMT == CRF_MEMBER_U8 ? 1u : 2u;
    // [slot][lane]: start + end of the member's tie run (2 * rank - 2).  Column = lane: private to the lane, no barrier.
    __shared__ uint8_t run_sum[N * 64];
    const int lane = threadIdx.x;
    const size_t v = size_t(blockIdx.x) * 64 + lane;
    const bool active = v < num_voxels;  // inactive lanes are out of range: they read 0 and store nothing
    const uint32_t bytes = uint32_t(num_voxels) * kElement, byte_offset = uint32_t(v) * kElement;

    uint32_t a[N];
    narrow_sorted_composites<FMT, N, false>(a, members, nullptr, cs, bytes, byte_offset);
    bool is_nan;
    {   // pinned here (see spearman_u32_kernel): the scans below overwrite the registers it reads
        uint32_t nan_flag = narrow_sorted_hold_nan<FMT, N>(a, cs) ? 1u : 0u;
        asm volatile("" : "+v"(nan_flag));
        is_nan = nan_flag != 0u;
    }
    // (the pads form a tie run of their own behind the cs real elements -- the pad key equals no real key -- and their
    // rows are masked when the ranks are read back: scanning them too keeps the kernel free of branches)
    // forward scan: first position of the tie run each sorted position belongs to, parked in bits 24..30
    {
        uint32_t run_start = 0u, prev = a[0];
#pragma unroll
        for (int p = 1; p < N; p++) {
            const uint32_t cur = a[p];
            const bool same = (cur ^ prev) < (1u << kNarrowSlotBits);  // equal keys
            run_start = same ? run_start : uint32_t(p);
            a[p] = cur | (run_start << 24);
            prev = cur;
            if ((p & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // bound the scheduler's window: register pressure
        }
    }
    pin_array(a);  // the scatter's address arithmetic stays behind the scan (see spearman_u32_kernel)
    __builtin_amdgcn_sched_barrier(0);
    // backward scan: last position of the run; start + end to the member's LDS row
    {
        uint32_t run_end = uint32_t(N - 1);
        bool next_same = false;  // positions p and p + 1 hold equal keys
#pragma unroll
        for (int p = N - 1; p >= 0; p--) {
            run_end = next_same ? run_end : uint32_t(p);
            const uint32_t start = a[p] >> 24;
            run_sum[narrow_composite_slot(a[p]) * 64 + lane] = uint8_t(start + run_end);
            next_same = start != uint32_t(p);  // the run of p started before it
            if ((p & 3) == 0) __builtin_amdgcn_sched_barrier(0);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    // ranks back in member order (same lane wrote them: program order suffices); all reads first, then the conversions
    // (see spearman_kernel)
    float r[N];
#pragma unroll
    for (int e = 0; e < N; e++) a[e] = run_sum[e * 64 + lane];
#pragma unroll
    for (int e = 0; e < N; e++) r[e] = (e < SURE || e < cs) ? 0.5f * float(a[e] + 2u) : 0.0f;
    float res = pearson_tail<N, false, SURE>(r, prep, cs);
    if (is_nan) res = __uint_as_float(0x7FC00000u);
    if (active) store_result_nt(out + v, res);
}

namespace {

using NarrowSpearmanKernel = void (*)(const void* const*, const float*, float*, size_t, int);

template <int FMT>
NarrowSpearmanKernel spearman_narrow_for(int cs) {
    switch ((cs + 7) / 8 * 8) {
        case 40: return spearman_narrow_kernel<FMT, 40>;
        case 48: return spearman_narrow_kernel<FMT, 48>;
        case 56: return spearman_narrow_kernel<FMT, 56>;
        case 64: return spearman_narrow_kernel<FMT, 64>;
        case 72: return spearman_narrow_kernel<FMT, 72>;
        case 80: return spearman_narrow_kernel<FMT, 80>;
        case 88: return spearman_narrow_kernel<FMT, 88>;
        case 96: return spearman_narrow_kernel<FMT, 96>;
        case 104: return spearman_narrow_kernel<FMT, 104>;
        case 112: return spearman_narrow_kernel<FMT, 112>;
        case 120: return spearman_narrow_kernel<FMT, 120>;
        default: return spearman_narrow_kernel<FMT, 128>;
    }
}

}  // namespace

hipError_t launch_spearman_narrow(const void* const* d_narrow, int format, int cs, size_t num_voxels, const RefSource& ref,
                                  float* d_prep, float* d_out, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end,
                                  LaunchInfo* info) {
    if (cs < 33 || cs > kNarrowMaxMembers || format == CRF_MEMBER_F32 || !spearman_narrow_routed(format, cs) ||
        num_voxels * member_format_bytes(format) >= kNarrowMaxBytes || (ref.prepare() && !ref.values))
        return hipErrorInvalidValue;
    if (ref.prepare()) launch_spearman_prep(ref, nullptr, cs, d_prep, s);
    if (!ref.run()) return hipGetLastError();
    const NarrowSpearmanKernel k = format == CRF_MEMBER_U8    ? spearman_narrow_for<CRF_MEMBER_U8>(cs)
                                   : format == CRF_MEMBER_U16 ? spearman_narrow_for<CRF_MEMBER_U16>(cs)
                                                              : spearman_narrow_for<CRF_MEMBER_F16>(cs);
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    hipLaunchKernelGGL(k, dim3(unsigned((num_voxels + 63) / 64)), dim3(64), 0, s, d_narrow, d_prep, d_out, num_voxels, cs);
    if (ev_end) (void)hipEventRecord(ev_end, s);
    if (info) info->kernel_name = "spearman_narrow_kernel";
    return hipGetLastError();
}

}  // namespace crf
