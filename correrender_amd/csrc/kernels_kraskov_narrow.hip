// kernels_kraskov_narrow.hip -- Kraskov (KSG) mutual information on members stored as uint8, uint16 or float16, read as
// stored: the launch of both kernel families, and kraskov_direct_narrow_kernel, the sibling of kraskov_direct_kernel
// (kernels_kraskov.hip).
//
// A lane owns one voxel and loads one byte / short per member (load_code_nt, the element's own alignment); the code
// becomes the value the calculators see through narrow_code_value (crf_device.h: the correctly rounded float(b) / 255.0f,
// float(s) / 65535.0f, float(h)), and from there on every operation is the fp32 kernel's, in its order: the plan
// (kraskov_field_plan) fixes family, K, TI and the x-distance table, and with them the order in which the fp64 partial
// sums are added, so the results are bit-identical to the fp32 kernel of the same plan on the converted values.
//
// The column kernel is not here: mi_kraskov_kernel<FMT, K, TI, DXT> (kernels_kraskov.hip) is one text for every stored
// format, and this file launches its uint8 instantiations (kraskov_column_narrow_kernel).  The tile-free kernel below is a
// text of its own, and not a copy of kraskov_direct_kernel's: it always stages the tile, it has PARK, and it leaves out
// the symmetric form and the share == 0 path that the fp32 kernel keeps.  Its arithmetic and the order of its sums are
// those of kraskov_direct_kernel's share = 1 path, which a change there has to keep in mind:
// tests/test_gpu_narrow_kraskov.py compares the two bit for bit at every routed plan.
//
// Where a value lives between its one load and its uses is not arithmetic.  The column kernel parks converted floats; the
// tile-free kernel has PARK:
//   kParkFloats   the converted floats in LDS -- the staged tile of kraskov_direct_kernel;
//                 one conversion per value and voxel, the fp32 kernel's LDS footprint
//   kParkCodes    the raw codes in LDS, converted at every fetch: a quarter (u8) or half of the footprint, so the tile-free
//                 kernel can stage a tile at every member count up to 128 (8 / 16 KB beside the tables)
// profiles/narrow_kraskov_ab.md has what was measured and which (format, family, member count) is routed here
// (kraskov_plan.h: kraskov_narrow_plan).  The reference side (kraskov_prep_kernel, the x-distance table) is fp32.
#include <type_traits>

#include "crf_device.h"
#include "crf_internal.h"
#include "crf_kraskov_device.h"
#include "crf_mi_device.h"
#include "kraskov_plan.h"

namespace crf {

static_assert(kKraskovNarrowMaxMembers == kNarrowMaxMembers, "kraskov_plan.h cannot include crf_internal.h");

enum KraskovNarrowPark { kParkFloats = 0, kParkCodes = 1 };

template <int FMT, int PARK>
using kraskov_parked_t =
    std::conditional_t<PARK == kParkFloats, float, std::conditional_t<FMT == CRF_MEMBER_U8, uint8_t, uint16_t>>;

template <int FMT, int PARK>
__device__ __forceinline__ kraskov_parked_t<FMT, PARK> kraskov_park(uint32_t code) {
    if constexpr (PARK == kParkFloats) return narrow_code_value<FMT>(code);
    else return kraskov_parked_t<FMT, PARK>(code);
}
template <int FMT, int PARK>
__device__ __forceinline__ float kraskov_parked_value(kraskov_parked_t<FMT, PARK> parked) {
    if constexpr (PARK == kParkFloats) return parked;
    else return narrow_code_value<FMT>(uint32_t(parked));
}

// kraskov_direct_kernel (field mode, the four waves of a block sharing a voxel tile) on narrow members.  The block always
// stages the tile in LDS -- floats or codes -- whatever the plan's `stage` says: staging changes where a value is fetched
// from, not what is added to what.  The work split, and with it the order of the partial sums, is the fp32 kernel's.
template <int FMT, int PARK, int K, int TI, bool DXT = false>
__global__ __launch_bounds__(256, direct_min_waves(K, TI, false)) void kraskov_direct_narrow_kernel(
    const void* const* __restrict__ members, const double* __restrict__ prep_px, const double* __restrict__ table_psi,
    const double* __restrict__ noise_query, float* __restrict__ out, size_t num_voxels, int cs, int k, int estimator,
    int to_cc, double c_term) {
    using parked_t = kraskov_parked_t<FMT, PARK>;
    constexpr uint32_t kElement = FMT == CRF_MEMBER_U8 ? 1u : 2u;
    extern __shared__ __align__(16) unsigned char smem[];
    double* s_px = reinterpret_cast<double*>(smem);  // member order
    double* s_spx = s_px + cs;                       // ascending
    double* s_nq = s_spx + cs;
    parked_t* s_tile = reinterpret_cast<parked_t*>(s_nq + cs);  // [cs][64], the current tile
    // partial sums of the block's 4 tiles, one slot per (tile, wave): [16][64] x (sum_x, sum_y, NaN flag)
    __shared__ double s_sum_x[16 * 64];
    __shared__ double s_sum_y[16 * 64];
    __shared__ int s_nan[16 * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));  // uniform: i0 below stays in SGPRs
    const double* __restrict__ dxt = prep_px + dxt_offset(cs);  // DXT only
    const int dxt_cols = (cs + 7) / 8 * 8;
    for (int i = threadIdx.x; i < cs; i += 256) {
        s_px[i] = prep_px[i];
        s_spx[i] = prep_px[cs + i];
        s_nq[i] = noise_query[i];
    }
    __syncthreads();
    constexpr int JB = 16;  // member values fetched per batch of the sweeps
    const uint32_t bytes = uint32_t(num_voxels) * kElement;
    const int kk = k < cs - 1 ? k : cs - 1;
    int top = 1;
    while (top * 2 <= cs) top *= 2;
    const double factor = 1.0 / double(cs);
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    const size_t tiles = (num_voxels + 63) / 64;
    const size_t groups = (tiles + 3) / 4;
    const int passes = (cs + TI - 1) / TI;
#pragma unroll 1
    for (size_t group = blockIdx.x; group < groups; group += gridDim.x) {
#pragma unroll
      for (int t4 = 0; t4 < 4; t4++) {
          s_sum_x[(t4 * 4 + wave) * 64 + lane] = 0.0;
          s_sum_y[(t4 * 4 + wave) * 64 + lane] = 0.0;
          s_nan[(t4 * 4 + wave) * 64 + lane] = 0;
      }
#pragma unroll 1
      for (int t4 = 0; t4 < 4; t4++) {
        const size_t tile = group * 4 + size_t(t4);
        if (tile >= tiles) continue;  // block-uniform
        const size_t v = tile * 64 + lane;
        const uint32_t off = v < num_voxels ? uint32_t(v) * kElement : kOutOfRangeOffset;
        __syncthreads();  // every wave has finished reading the previous tile
#pragma unroll 1
        for (int m0 = wave; m0 < cs; m0 += 4 * 8) {
            uint32_t stage[8];
#pragma unroll
            for (int q = 0; q < 8; q++) stage[q] = load_code_nt<FMT>(members[m0 + 4 * q < cs ? m0 + 4 * q : cs - 1], bytes, off);
#pragma unroll
            for (int q = 0; q < 8; q++)
                if (m0 + 4 * q < cs) s_tile[(m0 + 4 * q) * 64 + lane] = kraskov_park<FMT, PARK>(stage[q]);
        }
        __syncthreads();
        const auto value_of = [&](int m) -> float { return kraskov_parked_value<FMT, PARK>(s_tile[m * 64 + lane]); };
        bool is_nan = false;
        double sum_x = 0.0, sum_y = 0.0;
        // the 4 * passes items (tile, TI points) of the group are dealt to the waves round-robin
        const int first = (wave - t4 * passes) & 3;
#pragma unroll 1
        for (int i0 = first * TI; i0 < cs; i0 += 4 * TI) {
            double pxi[TI], pyi[TI], dk[TI], rx[TI], ry[TI];
            double best[TI][K];
#pragma unroll
            for (int t = 0; t < TI; t++) {
                const int ii = (i0 + t < cs) ? i0 + t : cs - 1;
                const float y = value_of(ii);
                if constexpr (FMT == CRF_MEMBER_F16) is_nan |= y != y;  // the integer formats have no NaN
                pxi[t] = s_px[ii];
                pyi[t] = double(y) + s_nq[ii];
#pragma unroll
                for (int q = 0; q < K; q++) best[t][q] = inf;
            }
            // ---- sweep A: the K smallest Chebyshev distances to OTHER points (kraskov_direct_kernel)
#pragma unroll 1
            for (int j0 = 0; j0 < cs; j0 += JB) {
                float yb[JB];
#pragma unroll
                for (int u = 0; u < JB; u++) yb[u] = value_of(j0 + u < cs ? j0 + u : cs - 1);
                auto candidate_a = [&](int u) {
                    const int j = j0 + u;
                    const int jc = j < cs ? j : cs - 1;
                    const double pxj = j < cs ? s_px[jc] : inf;
                    const double pyj = (DXT || j < cs) ? double(yb[u]) + s_nq[jc] : inf;
                    const double* dx_row = DXT ? dxt + size_t(j) * size_t(dxt_cols) + i0 : nullptr;
#pragma unroll
                    for (int t = 0; t < TI; t++) {
                        double d;
                        if constexpr (DXT) {
                            d = chebyshev_f64_sx(pyi[t] - pyj, dx_row[t]);
                        } else {
                            d = chebyshev_f64(pxi[t] - pxj, pyi[t] - pyj);
                            const uint64_t bits = uint64_t(__double_as_longlong(d));
                            const uint32_t hi = (j == i0 + t) ? 0x7FEFFFFFu : uint32_t(bits >> 32);
                            d = __longlong_as_double((long long)((uint64_t(hi) << 32) | uint32_t(bits)));
                        }
#pragma unroll
                        for (int q = 0; q < K; q++) {
                            const double lo = min_f64(best[t][q], d);
                            if (q + 1 < K) d = max_f64(best[t][q], d);
                            best[t][q] = lo;
                        }
                    }
                };
#pragma unroll
                for (int u = 0; u < JB / 2; u++) candidate_a(u);
                if (j0 + JB / 2 < cs) {
#pragma unroll
                    for (int u = JB / 2; u < JB; u++) candidate_a(u);
                }
            }
#pragma unroll
            for (int t = 0; t < TI; t++) {
                double sel = best[t][0];
#pragma unroll
                for (int q = 1; q < K; q++) sel = (q == kk - 1) ? best[t][q] : sel;
                dk[t] = sel;
            }
            if (estimator == 1) {
#pragma unroll
                for (int t = 0; t < TI; t++) rx[t] = ry[t] = dk[t] - kCountSlack;
            } else {
                double ex[TI], ey[TI];
#pragma unroll
                for (int t = 0; t < TI; t++) ex[t] = ey[t] = 0.0;
#pragma unroll 2
                for (int j = 0; j < cs; j++) {
                    const double pxj = s_px[j];
                    const double pyj = double(value_of(j)) + s_nq[j];
#pragma unroll
                    for (int t = 0; t < TI; t++) {
                        const double ax = fabs(pxi[t] - pxj), ay = fabs(pyi[t] - pyj);
                        const bool in = fmax(ax, ay) <= dk[t];
                        ex[t] = in ? fmax(ex[t], ax) : ex[t];
                        ey[t] = in ? fmax(ey[t], ay) : ey[t];
                    }
                }
#pragma unroll
                for (int t = 0; t < TI; t++) {
                    rx[t] = ex[t] + kCountSlack;
                    ry[t] = ey[t] + kCountSlack;
                }
            }
            // ---- sweep C: marginal counts
            double loy[TI], hiy[TI], lox[TI], hix[TI];
            int cx[TI], cy[TI];
#pragma unroll
            for (int t = 0; t < TI; t++) {
                lox[t] = pxi[t] - rx[t];
                hix[t] = pxi[t] + rx[t];
                loy[t] = pyi[t] - ry[t];
                hiy[t] = pyi[t] + ry[t];
                cx[t] = cy[t] = 0;
            }
            {
                int less[TI];
                count_less_batch<TI>(s_spx, cs, top, hix, cx);
                count_less_batch<TI>(s_spx, cs, top, lox, less);
#pragma unroll
                for (int t = 0; t < TI; t++) cx[t] -= less[t];
            }
#pragma unroll 1
            for (int j0 = 0; j0 < cs; j0 += JB) {
                float yb[JB];
#pragma unroll
                for (int u = 0; u < JB; u++) yb[u] = value_of(j0 + u < cs ? j0 + u : cs - 1);
                auto candidate_c = [&](int u) {
                    const int jc = j0 + u < cs ? j0 + u : cs - 1;
                    const double pyj = j0 + u < cs ? double(yb[u]) + s_nq[jc] : inf;  // past the end: inside no [lo, hi)
#pragma unroll
                    for (int t = 0; t < TI; t++) cy[t] += (pyj >= loy[t] && pyj < hiy[t]) ? 1 : 0;
                };
#pragma unroll
                for (int u = 0; u < JB / 2; u++) candidate_c(u);
                if (j0 + JB / 2 < cs) {
#pragma unroll
                    for (int u = JB / 2; u < JB; u++) candidate_c(u);
                }
            }
#pragma unroll
            for (int t = 0; t < TI; t++) {
                if (i0 + t < cs) {
                    int nx = cx[t] > 1 ? cx[t] : 1;
                    int ny = cy[t] > 1 ? cy[t] : 1;
                    if (estimator != 1) {
                        nx -= 1;  // psi(n - 1), psi(0) = NaN (pole)
                        ny -= 1;
                    }
                    sum_x += factor * table_psi[nx];
                    sum_y += factor * table_psi[ny];
                }
            }
        }
        const int slot = (t4 * 4 + wave) * 64 + lane;
        s_sum_x[slot] = sum_x;
        s_sum_y[slot] = sum_y;
        s_nan[slot] = is_nan ? 1 : 0;
      }
      __syncthreads();
      {   // wave w finishes tile w of the group
        double sum_x = 0.0, sum_y = 0.0;
        int is_nan = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            sum_x += s_sum_x[(wave * 4 + w) * 64 + lane];
            sum_y += s_sum_y[(wave * 4 + w) * 64 + lane];
            is_nan |= s_nan[(wave * 4 + w) * 64 + lane];
        }
        const size_t v = (group * 4 + size_t(wave)) * 64 + lane;
        const double mi = -sum_x - sum_y + c_term + table_psi[cs];
        float res = float(mi);
        res = (res < 0.0f) ? 0.0f : res;
        if (to_cc) res = mi_to_cc(res);
        if (is_nan) res = __uint_as_float(0x7FC00000u);
        if (v < num_voxels) store_result_nt(out + v, res);
      }
      __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Host side: the plan of kraskov_narrow_plan (kraskov_plan.h) -> kernel pointer, as kernels_kraskov.hip does for fp32.
// ---------------------------------------------------------------------------------------------------------------
namespace {

using NarrowKernel = KraskovColumnKernel;  // the tile-free kernel takes the column kernel's arguments

// Where the values are parked, by measurement (profiles/narrow_kraskov_ab.md).  The LDS column: floats (codes cost 1-3 %
// at k = 1 and 3 and gained 6 % only at k = 2; that form is not kept).  The tile of the tile-free kernel: floats up to 64
// members -- where the fp32 plan stages floats too, and where it does not (k <= 2, k > 4) floats were 2-4 % faster than
// codes -- and codes above, where a tile of floats costs occupancy (11-25 % slower than the fp32 kernel at 80..128 members).
constexpr int kFloatTileMaxMembers = 64;

// Only what kraskov_narrow_plan routes is built.  Tile-free: K = 2, 3, 4 and 8 (K = 1 is routed nowhere).  (Column:
// kraskov_column_narrow_kernel, kernels_kraskov.hip.)
template <int FMT, int PARK, int K>
NarrowKernel direct_narrow_table_kernel(const KraskovPlan& p) {
    return p.TI == 4 ? kraskov_direct_narrow_kernel<FMT, PARK, K, 4, true> : kraskov_direct_narrow_kernel<FMT, PARK, K, 8, true>;
}

template <int FMT, int PARK>
NarrowKernel direct_narrow_kernel(const KraskovPlan& p) {
    if (p.dxt) {
        switch (p.K) {
            case 2: return direct_narrow_table_kernel<FMT, PARK, 2>(p);
            case 3: return direct_narrow_table_kernel<FMT, PARK, 3>(p);
            case 4: return direct_narrow_table_kernel<FMT, PARK, 4>(p);
            default: return nullptr;
        }
    }
    if (p.K == 3 && p.TI == 4) return kraskov_direct_narrow_kernel<FMT, PARK, 3, 4>;
    if (p.K == 4 && p.TI == 4) return kraskov_direct_narrow_kernel<FMT, PARK, 4, 4>;
    switch (p.K) {
        case 2: return kraskov_direct_narrow_kernel<FMT, PARK, 2, 8>;
        case 3: return kraskov_direct_narrow_kernel<FMT, PARK, 3, 8>;
        case 4: return kraskov_direct_narrow_kernel<FMT, PARK, 4, 8>;
        case 8: return kraskov_direct_narrow_kernel<FMT, PARK, 8, 4>;
        default: return nullptr;  // K = 1; K = 16 (it spills to scratch), 32, 64, 128: not routed (kraskov_narrow_plan)
    }
}

constexpr size_t parked_bytes(int format, int park) {
    return park == kParkFloats ? sizeof(float) : (format == CRF_MEMBER_U8 ? 1 : 2);
}

template <int FMT>
hipError_t launch_narrow(const KraskovPlan& p, const void* const* d_narrow, int cs, size_t num_voxels, const KraskovArgs& a,
                         const KraskovTables& t, const double* prep, float* d_out, hipStream_t s, hipEvent_t ev_begin,
                         hipEvent_t ev_end, LaunchInfo* info) {
    const size_t tiles = (num_voxels + 63) / 64;
    NarrowKernel kernel = nullptr;
    size_t lds = 0;
    unsigned blocks = 0, threads = 0;
    if (p.family == KraskovFamily::Column) {
        kernel = kraskov_column_narrow_kernel(FMT, p);
        lds = kraskov_column_lds_bytes(cs);
        blocks = unsigned(tiles);
        threads = 64;
    } else {
        const int park = p.stage || cs <= kFloatTileMaxMembers ? kParkFloats : kParkCodes;
        kernel = park == kParkFloats ? direct_narrow_kernel<FMT, kParkFloats>(p) : direct_narrow_kernel<FMT, kParkCodes>(p);
        lds = kraskov_table_bytes(cs) + size_t(cs) * 64 * parked_bytes(FMT, park);
        const size_t groups = (tiles + 3) / 4;
        blocks = unsigned(groups < 65536 ? groups : 65536);
        threads = 256;
    }
    if (!kernel) return hipErrorInvalidValue;
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds, s, d_narrow, prep, t.psi, t.noise_query, d_out, num_voxels,
                       cs, a.k, a.estimator, int(a.to_cc), a.c_term);
    if (ev_end) (void)hipEventRecord(ev_end, s);
    if (info) info->kernel_name = p.family == KraskovFamily::Column ? "mi_kraskov_narrow_kernel" : "kraskov_direct_narrow_kernel";
    return hipGetLastError();
}

}  // namespace

bool kraskov_narrow_routed(int format, int cs, int k) {
    KraskovPlan plan;
    return kraskov_narrow_plan(format, cs, k, read_switches(), &plan);
}

hipError_t launch_mi_kraskov_narrow(const void* const* d_narrow, int format, int cs, size_t num_voxels, const RefSource& ref,
                                    const KraskovArgs& a, const double* d_tables, float* d_prep, float* d_out, hipStream_t s,
                                    hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info) {
    KraskovPlan plan;
    if (num_voxels * member_format_bytes(format) >= kNarrowMaxBytes || (ref.prepare() && !ref.values) ||
        !kraskov_narrow_plan(format, cs, a.k, read_switches(), &plan))
        return hipErrorInvalidValue;  // not routed here
    const KraskovTables t = kraskov_tables(d_tables, cs);
    double* prep = reinterpret_cast<double*>(d_prep);
    if (ref.prepare()) launch_kraskov_prep(ref, nullptr, cs, t.noise_ref, prep, s);
    if (!ref.run()) return hipGetLastError();
    switch (format) {
        case CRF_MEMBER_U8:
            return launch_narrow<CRF_MEMBER_U8>(plan, d_narrow, cs, num_voxels, a, t, prep, d_out, s, ev_begin, ev_end, info);
        case CRF_MEMBER_U16:
            return launch_narrow<CRF_MEMBER_U16>(plan, d_narrow, cs, num_voxels, a, t, prep, d_out, s, ev_begin, ev_end, info);
        default:
            return launch_narrow<CRF_MEMBER_F16>(plan, d_narrow, cs, num_voxels, a, t, prep, d_out, s, ev_begin, ev_end, info);
    }
}

}  // namespace crf
