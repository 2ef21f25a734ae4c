// kernels_binned_narrow.hip -- binned mutual information on members stored as uint8, uint16 or float16, read as stored.
//
// mi_binned_kernel (kernels_binned.hip) spends most of its time per sample: subtract, divide (or the Markstein chain),
// fp32 -> fp64, an fp64 multiply, truncate, clamp -- the member loads are the smaller part.  Here a lane reads one byte /
// short per member instead of a dword, and what happens to the code depends on the format:
//   TABLE  (u8)         a uint8 member has 256 codes and num_bins is at most 255, so the whole per-sample chain is a
//                       256-byte table in LDS that the block fills once: four codes per lane through the division form of
//                       crf_binned_bins.h on float(code) / 255.0f.  Per sample: one ds_read_u8.  A byte read banks at
//                       (address / 4) mod 32 and the table spans 64 dwords, so two distinct dwords share a bank: at most
//                       2-way per 32-lane group (equal addresses broadcast).
//   RCP / DIV (u16, f16; measured against the table for u8 and 21-27 % slower there, so u8 has the table only)
//                       the code becomes the value the calculators see in registers (crf_device.h's conversions: the
//                       compile-time exact_div by 65535, float(h)), then the reciprocal or the division form of
//                       crf_binned_bins.h, chosen by the launcher with launch_binned_n's rule on max_query - min_query.
// Everything behind the bins -- the cell codes b1 << 8 | b0, the LDS column of the slow path, the sort, the run-length scan,
// the recount, the NaN store -- is mi_binned_kernel's (binned_mi_of_codes below), and the reference side is
// binned_prep_kernel's on fp32 values.  The bins are those of mi_binned_kernel on the converted values (the table holds the
// division form, which the reciprocal form equals for every non-NaN sample), so the results are bit-identical to it.
// One lane per voxel, 64-lane blocks, no fp32 copy of the members, members aligned to their element only.
#include <cstdlib>

#include "crf_device.h"
#include "crf_internal.h"
#include "crf_mi_device.h"

namespace crf {

enum BinnedNarrowMode { kBinTable = 0, kBinRcp = 1, kBinDiv = 2 };

// Everything behind the cell codes, for one lane = one voxel: mi_binned_kernel's lines (kernels_binned.hip), copied -- with
// both kernels calling one function the fp32 kernel's instantiations come out with other register counts (-6 .. +5 VGPRs),
// so its text stays as it is (profiles/narrow_binned_ab.md).  a[e] = b1 << 8 | b0 of slot e, kPadCode for a pad or a skipped
// sample (low 16 bits all ones also where the reference sample is skipped: b0 = kInvalidBin); `total` samples count; slots
// from FIRST_GUARDED on are members only below cs.  T (LDS): T[c] = (c/cs) ln(c/cs), 0 behind cs; codes (LDS): the lane's
// column at codes[e * 64 + lane], written and read here only.  Returns the voxel's result, NaN for is_nan.
template <int N, int FIRST_GUARDED>
__device__ __forceinline__ float binned_mi_of_codes(uint32_t (&a)[N], const double* T, uint16_t* codes, int lane, int cs,
                                                    int total, bool is_nan, bool ref_all_valid, double sx, int to_cc) {
    const auto is_member = [cs](int e) { return e < FIRST_GUARDED || e < cs; };  // folds in the unrolled loops
    // (a lane with a NaN member stores NaN whatever the histogram says: it must not drag itself -- and with it its wave,
    // for cs^2 steps -- onto the recount; missing values come in whole regions: 256^3 x 128 with 30 % NaN voxels 75.8 ms)
    const bool slow = !is_nan && ((total != cs) || !ref_all_valid);
    const bool any_slow = __any(slow);
    if (any_slow) {
#pragma unroll
        for (int e = 0; e < N; e++)
            if (is_member(e)) codes[e * 64 + lane] = uint16_t(a[e] & 0xFFFFu);  // pad -> 0xFFFF
    }

    __builtin_amdgcn_sched_barrier(0);
    SortNet32<N>::sort(a);
    pin_array(a);  // the network ends here (crf_device.h)
    __builtin_amdgcn_sched_barrier(0);
    double mi_y = -sx, joint = 0.0;
    uint32_t cell_len = 0, col_len = 0;
#pragma unroll
    for (int p = 0; p < N; p++) {
        if (p % 8 == 0) __builtin_amdgcn_sched_barrier(0);  // bounds the table look-ups hoisted ahead of the sums
        // guarded instantiation: the cs - total .. pads (kPadCode, the largest code) sort behind the real samples;
        // a pad position contributes T[0] = 0
        const bool member = is_member(p);
        uint32_t next = kPadCode;
        if (p + 1 < N) next = is_member(p + 1) ? a[p + 1] : kPadCode;
        cell_len++;
        col_len++;
        const bool end_cell = member && next != a[p];
        const bool end_col = member && (next >> 8) != (a[p] >> 8);
        joint += T[end_cell ? cell_len : 0u];
        mi_y -= T[end_col ? col_len : 0u];
        cell_len = end_cell ? 0u : cell_len;
        col_len = end_col ? 0u : col_len;
    }
    double mi = mi_y + joint;

    if (any_slow && slow) {
        // Samples were skipped: probabilities are c/total with total < cs.  Direct O(cs^2) evaluation over the
        // lane's LDS column; first occurrence of each bin/cell contributes its term.
        mi = 0.0;
        int counted = 0;  // samples with a query bin AND a reference bin
#pragma unroll 1
        for (int i = 0; i < cs; i++) counted += codes[i * 64 + lane] != 0xFFFFu;
        if (counted > 0) {
            const double tot = double(counted);
            const double eps1 = 0.5 / double(cs);
            const double eps2 = 0.5 / double(cs * cs);
#pragma unroll 1
            for (int i = 0; i < cs; i++) {
                const uint32_t ci = codes[i * 64 + lane];
                if (ci == 0xFFFFu) continue;
                int cx = 0, cy = 0, cxy = 0;
                bool fx = true, fy = true, fxy = true;
#pragma unroll 1
                for (int j = 0; j < cs; j++) {
                    const uint32_t cj = codes[j * 64 + lane];
                    if (cj == 0xFFFFu) continue;
                    const bool ex = (cj & 0xFFu) == (ci & 0xFFu);
                    const bool ey = (cj >> 8) == (ci >> 8);
                    cx += ex;
                    cy += ey;
                    cxy += (ex && ey);
                    if (j < i) {
                        fx = fx && !ex;
                        fy = fy && !ey;
                        fxy = fxy && !(ex && ey);
                    }
                }
                if (fx) {
                    const double p = double(cx) / tot;
                    if (p > eps1) mi -= p * log(p);
                }
                if (fy) {
                    const double p = double(cy) / tot;
                    if (p > eps1) mi -= p * log(p);
                }
                if (fxy) {
                    const double p = double(cxy) / tot;
                    if (p > eps2) mi += p * log(p);
                }
            }
        }
    }
    float res = float(mi);
    if (to_cc) res = mi_to_cc(res);
    if (is_nan) res = __uint_as_float(0x7FC00000u);
    return res;
}

// N - 16 < cs <= N (launch_mi_binned_narrow pads cs to the next multiple of 16): the first N - 16 slots are members
// whatever cs is; a slot past cs loads at kOutOfRangeOffset (0, no memory request) and gets kPadCode.
// LC: slots loaded per batch, all of them before the batch's first use (mi_binned_kernel).
template <int FMT, int N, int MIN_WAVES, int LC, int MODE>
__global__ __launch_bounds__(64, MIN_WAVES) void mi_binned_narrow_kernel(const void* const* __restrict__ members,
                                                                         const int* __restrict__ prep,
                                                                         const double* __restrict__ tableT,
                                                                         float* __restrict__ out, size_t num_voxels, int cs,
                                                                         int nb, float min_q, float max_q, int to_cc) {
    static_assert(MODE != kBinTable || FMT == CRF_MEMBER_U8, "the table has one entry per 8-bit code");
    static_assert(N % 16 == 0 && N % LC == 0, "whole batches");
    constexpr uint32_t kElement = FMT == CRF_MEMBER_U8 ? 1u : 2u;
    constexpr int kFirstGuarded = N - 16;
    __shared__ double T[N + 1];
    __shared__ uint16_t codes[N * 64];
    __shared__ uint8_t bin_of_code[MODE == kBinTable ? 256 : 1];
    const int lane = threadIdx.x;
    const float range_q = max_q - min_q;
    const double nbd = double(nb);
    for (int i = lane; i <= N; i += 64) T[i] = i <= cs ? tableT[i] : 0.0;
    if constexpr (MODE == kBinTable) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t code = uint32_t(lane) + 64u * uint32_t(i);
            bin_of_code[code] = uint8_t(query_bin_or_skip_div(float(code) / 255.0f, min_q, range_q, nbd, nb));
        }
    }
    __syncthreads();
    const size_t v = size_t(blockIdx.x) * 64 + lane;
    // lanes past the end read 0 (num_voxels x element size is below kNarrowMaxBytes: nothing wraps)
    const uint32_t byte_offset = uint32_t(v) * kElement, bytes = uint32_t(num_voxels) * kElement;
    const bool ref_all_valid = prep[N] != 0;
    const double sx = *reinterpret_cast<const double*>(reinterpret_cast<const char*>(prep) + kBinnedSxOffset);

    const auto is_member = [cs](int e) { return e < kFirstGuarded || e < cs; };  // folds in the unrolled loops
    uint32_t a[N];
    bool is_nan = false;
    int total = 0;
    const float rcp_q = MODE == kBinRcp ? 1.0f / range_q : 0.0f;
#pragma unroll
    for (int base = 0; base < N; base += LC) {
        uint32_t c[LC];
#pragma unroll
        for (int i = 0; i < LC; i++) {
            const int e = base + i;
            c[i] = load_code_nt<FMT>(members[is_member(e) ? e : cs - 1], bytes,
                                     is_member(e) ? byte_offset : kOutOfRangeOffset);
        }
#pragma unroll
        for (int i = 0; i < LC; i++) {
            const int e = base + i;
            const bool member = is_member(e);
            // reference bin of the member; kInvalidBin = 0xFFFF for a skipped reference sample (and for pads), see
            // mi_binned_kernel
            const int b0 = prep[e];
            uint32_t b1;
            bool valid;
            if constexpr (MODE == kBinTable) {
                b1 = bin_of_code[c[i]];
                valid = member && b1 != kSkippedSampleBin;
            } else {
                const float y = narrow_code_value<FMT>(c[i]);
                if constexpr (FMT == CRF_MEMBER_F16) is_nan |= member && (y != y);  // the integer formats have no NaN
                bool counts;
                if constexpr (MODE == kBinRcp)
                    b1 = uint32_t(query_bin_rcp(y, min_q, range_q, rcp_q, nbd, nb, &counts));
                else
                    b1 = uint32_t(query_bin_div(y, min_q, range_q, nbd, nb, &counts));
                valid = member && counts;
            }
            a[e] = valid ? (b1 << 8) | uint32_t(b0) : kPadCode;
            total += valid ? 1 : 0;
        }
        if (LC < N) __builtin_amdgcn_sched_barrier(0);  // the next batch is not hoisted above this one's conversion
        if constexpr (FMT == CRF_MEMBER_F16) {
            // pin the NaN flag per batch, as mi_binned_kernel does: left alone the compiler sinks the compares to the end
            // of the kernel and keeps all N samples alive across the sort
            uint32_t nan_flag = is_nan ? 1u : 0u;
            asm volatile("" : "+v"(nan_flag));
            is_nan = nan_flag != 0u;
        }
    }
    const float res = binned_mi_of_codes<N, kFirstGuarded>(a, T, codes, lane, cs, total, is_nan, ref_all_valid, sx, to_cc);
    if (v < num_voxels) store_result_nt(out + v, res);
}

namespace {

using BinnedNarrowKernel = void (*)(const void* const*, const int*, const double*, float*, size_t, int, int, float, float,
                                    int);

// waves per SIMD as launch_mi_binned's table (the kernel holds the same N codes and the same tail)
template <int FMT, int MODE>
BinnedNarrowKernel binned_narrow_for(int n_pad) {
    switch (n_pad) {
        case 16: return mi_binned_narrow_kernel<FMT, 16, 4, 16, MODE>;
        case 32: return mi_binned_narrow_kernel<FMT, 32, 4, 32, MODE>;
        case 48: return mi_binned_narrow_kernel<FMT, 48, 3, 48, MODE>;
        case 64: return mi_binned_narrow_kernel<FMT, 64, 4, 64, MODE>;
        case 80: return mi_binned_narrow_kernel<FMT, 80, 3, 80, MODE>;
        case 96: return mi_binned_narrow_kernel<FMT, 96, 2, 96, MODE>;
        case 112: return mi_binned_narrow_kernel<FMT, 112, 2, 112, MODE>;
        default: return mi_binned_narrow_kernel<FMT, 128, 2, 128, MODE>;
    }
}

// the 16-bit formats: only what binned_narrow_routed (crf_internal.h) routes here is built; null otherwise
template <int FMT>
BinnedNarrowKernel binned_narrow_arith_for(int n_pad, bool rcp) {
    if (n_pad == 64)
        return rcp ? mi_binned_narrow_kernel<FMT, 64, 4, 64, kBinRcp> : mi_binned_narrow_kernel<FMT, 64, 4, 64, kBinDiv>;
    if constexpr (FMT == CRF_MEMBER_U16) {
        if (n_pad == 32)
            return rcp ? mi_binned_narrow_kernel<FMT, 32, 4, 32, kBinRcp> : mi_binned_narrow_kernel<FMT, 32, 4, 32, kBinDiv>;
    }
    return nullptr;
}

}  // namespace

hipError_t launch_mi_binned_narrow(const void* const* d_narrow, int format, int cs, size_t num_voxels, const RefSource& ref,
                                   const BinnedArgs& a, const double* d_tables, float* d_prep, float* d_out, hipStream_t s,
                                   hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info) {
    if (cs < 2 || cs > kNarrowMaxMembers || format == CRF_MEMBER_F32 ||
        num_voxels * member_format_bytes(format) >= kNarrowMaxBytes || (ref.prepare() && !ref.values))
        return hipErrorInvalidValue;
    const int n_pad = (cs + 15) / 16 * 16;
    int* prep = reinterpret_cast<int*>(d_prep);
    const double* tableT = d_tables + (cs + 1);
    if (ref.prepare()) launch_binned_prep(ref, nullptr, cs, n_pad, a, tableT, prep, s);
    if (!ref.run()) return hipGetLastError();
    const float range = a.max_query - a.min_query;  // the same fp32 subtraction the kernel performs
    const char* plain = getenv("CRF_BINNED_PLAIN_DIV");  // tuning / tests: always the per-sample division
    const bool rcp = binned_range_takes_rcp(range) && !(plain && *plain == '1');
    const BinnedNarrowKernel k = format == CRF_MEMBER_U8    ? binned_narrow_for<CRF_MEMBER_U8, kBinTable>(n_pad)
                                 : format == CRF_MEMBER_U16 ? binned_narrow_arith_for<CRF_MEMBER_U16>(n_pad, rcp)
                                                            : binned_narrow_arith_for<CRF_MEMBER_F16>(n_pad, rcp);
    if (!k) return hipErrorInvalidValue;  // not routed here (binned_narrow_routed)
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    hipLaunchKernelGGL(k, dim3(unsigned((num_voxels + 63) / 64)), dim3(64), 0, s, d_narrow, prep, tableT, d_out, num_voxels,
                       cs, a.num_bins, a.min_query, a.max_query, int(a.to_cc));
    if (ev_end) (void)hipEventRecord(ev_end, s);
    if (info) info->kernel_name = "mi_binned_narrow_kernel";
    return hipGetLastError();
}

}  // namespace crf
