// kernels_generic.hip -- the counting kernels: Spearman / Kendall / binned MI / Kraskov MI for ANY member count (cs up to
// kMaxGenericMembers).
//
// The register-resident kernels (kernels_rank.hip, kernels_binned.hip, kernels_kraskov.hip) are instantiated for cs <= 128; the reference has
// no such limit (its own synthetic data set has 1000 members, scripts/generate_synth_box_ensembles.py:47).  These
// kernels keep the same mapping -- one lane = one voxel (or one pair request) -- and use O(cs^2) counting formulations
// with runtime loops:
//   Spearman  2*rank_e = 1 + sum_j (2 [v_j < v_e] + [v_j == v_e])           (mid-ranks, Correlation.cpp:277-303)
//   Kendall   S_y = #{ a < b in x order, not in the same x-tie group : y_a > y_b },  n2 = #{ a < b : y_a == y_b }
//   binned    first-occurrence scan over the voxel's cell codes (the skipped-sample path of mi_binned_kernel)
//   Kraskov   the same brute-force k-select as mi_kraskov_kernel, tile pointer instead of LDS
// Where the values live:
//   direct_rank_kernel       field mode, Spearman / Kendall: reads the member volumes in place (16 rows per sweep)
//   direct_symmetric_kernel  symmetric field mode, Spearman / Kendall / binned MI: the same with two member tables
//   generic_kernel           field mode, binned MI / Kraskov (measures 3, 4, 5, 6): the voxel's cs values in a per-lane
//                            column [member][lane] of a tile that lives in LDS when it fits and otherwise in a global
//                            workspace slice owned by the block (persistent blocks, grid-stride over 64-voxel tiles)
//   pair_request_kernel      all seven measures between two arbitrary voxels per request, same tile scheme
// The arithmetic the kernels share is written once, in the helpers below; they take loaders, so the kernels that read
// member volumes and the ones that read tile columns run the same body.
// Integer cores are exact; fp32 tails use the reference's operation order; fp64 sums of the MI estimators differ from
// the reference's order at the 1e-16 level (see kernels_binned.hip).  Throughput is secondary here: at cs = 1000 the
// pair loops are ~10^6 compares per voxel, ~20 ms for the reference's 128x128x32 data set.
#include <cstdlib>

#include "crf_device.h"
#include "crf_internal.h"
#include "crf_mi_device.h"

namespace crf {

namespace {
constexpr int kGenericBlocks = 1024;        // persistent blocks (4 per CU)
constexpr int kDirectBlocks = 4096;
constexpr int kDirectRows = 16;
constexpr size_t kLdsTileLimit = 60 * 1024;  // use LDS for the tile when it fits under the default 64 KB limit
constexpr uint32_t kSkippedCell = 0xFFFFu;   // cell code of a skipped sample (num_bins <= 255: no valid code equals it)

__host__ __device__ inline size_t tile_bytes(int cs) { return size_t(cs) * 64 * (sizeof(float) + sizeof(uint16_t)); }
__host__ __device__ inline size_t pair_tile_bytes(int cs) {
    return size_t(cs) * 64 * (2 * sizeof(float) + 2 * sizeof(uint16_t));
}

// grid of a persistent kernel: one block per 64-item tile, at most max_blocks (the blocks stride over the tiles)
inline size_t persistent_blocks(size_t items, size_t max_blocks) {
    const size_t tiles = (items + 63) / 64;
    return tiles < max_blocks ? tiles : max_blocks;
}
}  // namespace

size_t direct_rank_workspace_bytes(int cs, size_t num_voxels, int measure) {
    if (measure != 1) return 0;  // Spearman's doubled ranks; Kendall keeps nothing per voxel
    return size_t(cs) * 64 * sizeof(uint16_t) * persistent_blocks(num_voxels, kDirectBlocks);
}

// the larger of generic_kernel's tile workspace and direct_rank_kernel's rank workspace (api.cpp sizes one buffer)
size_t generic_workspace_bytes(int cs, size_t num_voxels) {
    const size_t generic =
        tile_bytes(cs) <= kLdsTileLimit ? 0 : tile_bytes(cs) * persistent_blocks(num_voxels, kGenericBlocks);
    const size_t direct = direct_rank_workspace_bytes(cs, num_voxels, 1);
    return generic > direct ? generic : direct;
}

size_t direct_symmetric_workspace_bytes(int cs, size_t num_voxels, int measure) {
    if (measure == 2) return 0;  // Kendall keeps nothing per voxel
    return size_t(cs) * 64 * 2 * sizeof(uint16_t) * persistent_blocks(num_voxels, kDirectBlocks);
}

size_t pair_workspace_bytes(int cs, size_t num_requests) {
    if (pair_tile_bytes(cs) <= kLdsTileLimit) return 0;
    return pair_tile_bytes(cs) * persistent_blocks(num_requests, kGenericBlocks);
}

// ---- the shared arithmetic: loaders map an element index to its value; columns have a stride of 64 elements ---------
// (callers pass lambdas that capture by value: by reference direct_symmetric_kernel<1> took 4 VGPRs more and lost a wave)

// Doubled mid-ranks by counting, 2 * rank_e = 1 + sum_j (2 [v_j < v_e] + [v_j == v_e]), into column r2.  T elements
// are ranked per sweep, so every value read serves T comparisons.  Returns whether a value was NaN.
template <int T, class Load>
__device__ __forceinline__ bool doubled_ranks(int cs, Load load, uint16_t* r2) {
    bool is_nan = false;
#pragma unroll 1
    for (int e0 = 0; e0 < cs; e0 += T) {
        float ve[T];
        uint32_t sc[T];
#pragma unroll
        for (int r = 0; r < T; r++) {
            ve[r] = load(e0 + r < cs ? e0 + r : cs - 1);
            is_nan |= ve[r] != ve[r];
            sc[r] = 0u;
        }
#pragma unroll 4
        for (int j = 0; j < cs; j++) {
            const float vj = load(j);
#pragma unroll
            for (int r = 0; r < T; r++) sc[r] += (vj < ve[r]) ? 2u : ((vj == ve[r]) ? 1u : 0u);
        }
#pragma unroll
        for (int r = 0; r < T; r++)
            if (e0 + r < cs) r2[size_t(e0 + r) * 64] = uint16_t(sc[r] + 1u);  // self contributes the +1 of [v_e == v_e]
    }
    return is_nan;
}

// the half-integer rank behind a doubled rank
__device__ __forceinline__ float half_rank(const uint16_t* r2, int e) { return 0.5f * float(r2[size_t(e) * 64]); }

// computePearson2<float>(X, Y, cs) in member order (Correlation.cpp:141-174)
template <int UNROLL, class LoadX, class LoadY>
__device__ __forceinline__ float pearson2(int cs, LoadX X, LoadY Y) {
    const float n = float(cs);
    const float invN = 1.0f / n;
    const float invNm1 = 1.0f / (n - 1.0f);
    float meanX = 0.0f, meanY = 0.0f;
#pragma unroll UNROLL
    for (int e = 0; e < cs; e++) {
        meanX += invN * X(e);
        meanY += invN * Y(e);
    }
    float varX = 0.0f, varY = 0.0f;
#pragma unroll UNROLL
    for (int e = 0; e < cs; e++) {
        const float dx = X(e) - meanX, dy = Y(e) - meanY;
        varX += invNm1 * dx * dx;
        varY += invNm1 * dy * dy;
    }
    const float sdX = sqrtf(varX), sdY = sqrtf(varY);
    float r = 0.0f;
#pragma unroll UNROLL
    for (int e = 0; e < cs; e++) r += invNm1 * ((X(e) - meanX) / sdX) * ((Y(e) - meanY) / sdY);
    return r;
}

// The same with the reference side prepared: prep_a[e] = invNm1 * (x_e - meanX) / sdX (launch_spearman_prep)
template <int UNROLL, class LoadY>
__device__ __forceinline__ float pearson2_prepared(int cs, const float* __restrict__ prep_a, LoadY Y) {
    const float n = float(cs);
    const float invN = 1.0f / n;
    const float invNm1 = 1.0f / (n - 1.0f);
    float meanY = 0.0f;
#pragma unroll UNROLL
    for (int e = 0; e < cs; e++) meanY += invN * Y(e);
    float varY = 0.0f;
#pragma unroll UNROLL
    for (int e = 0; e < cs; e++) {
        const float d = Y(e) - meanY;
        varY += invNm1 * d * d;
    }
    const float sdY = sqrtf(varY);
    float r = 0.0f;
#pragma unroll UNROLL
    for (int e = 0; e < cs; e++) r += prep_a[e] * ((Y(e) - meanY) / sdY);
    return r;
}

// Kendall's tau-b from the tied pairs in x (n1), in y (n2) and the discordant pairs (Correlation.cpp:423-455)
__device__ __forceinline__ float tau_b(int cs, int32_t n1, int32_t n2, int32_t discordant) {
    const int32_t n = cs;
    const int32_t n0 = (n * (n - 1)) / 2;
    const int32_t numerator = n0 - n1 - n2 - 2 * discordant;
    const float denominator = sqrtf(float(n0 - n1)) * sqrtf(float(n0 - n2));
    return float(numerator) / denominator;
}

__device__ __forceinline__ int clamped_bin(float v01, int num_bins) {
    const int b = bin_index_x86(double(v01) * double(num_bins));
    return b < 0 ? 0 : (b > num_bins - 1 ? num_bins - 1 : b);
}

// Cell code b1 << 8 | b0 of a sample normalised to [0, 1] on both sides, kSkippedCell when either side is NaN (as in
// mi_binned_kernel).  cell_code_prepared: b0 comes from the prepared table of the reference side (kInvalidBin = skip).
__device__ __forceinline__ uint16_t cell_code(float x01, float y01, int num_bins) {
    const bool valid = (x01 == x01) && (y01 == y01);
    const int b0 = clamped_bin(x01, num_bins), b1 = clamped_bin(y01, num_bins);
    return valid ? uint16_t((b1 << 8) | b0) : uint16_t(kSkippedCell);
}
__device__ __forceinline__ uint16_t cell_code_prepared(int b0, float y01, int num_bins) {
    const bool valid = (y01 == y01) && b0 != kInvalidBin;
    const int b1 = clamped_bin(y01, num_bins);
    return valid ? uint16_t((b1 << 8) | b0) : uint16_t(kSkippedCell);
}

// Binned MI: what one sample adds to mi, given the counts of its x bin, y bin and cell over the voxel's valid samples
// and whether it is the first sample of each.  table_ok (every sample valid): p = c / cs, p ln p from the host-built table.
__device__ __forceinline__ double binned_mi_term(double mi, int cx, int cy, int cxy, bool first_x, bool first_y,
                                                 bool first_xy, bool table_ok, const double* __restrict__ tableT,
                                                 double tot, double eps1, double eps2) {
    if (table_ok) {
        if (first_x) mi -= tableT[cx];
        if (first_y) mi -= tableT[cy];
        if (first_xy) mi += tableT[cxy];
    } else {
        if (first_x) {
            const double p = double(cx) / tot;
            if (p > eps1) mi -= p * log(p);
        }
        if (first_y) {
            const double p = double(cy) / tot;
            if (p > eps1) mi -= p * log(p);
        }
        if (first_xy) {
            const double p = double(cxy) / tot;
            if (p > eps2) mi += p * log(p);
        }
    }
    return mi;
}

constexpr int kPivotSelectMinK = 16;  // more neighbours than this: selection by pivots instead of kk minimum passes

// The same value as the minimum passes below give, the kk-th smallest distance counted with multiplicity (infinity when
// fewer than kk distances are numbers), by partitioning: the answer lies in (lo, hi), a pass counts the distances of
// that interval below and at the pivot p and picks the next pivot on either side (the candidate with the smallest hash
// of its index, so the member order does not matter): about 2 ln(cs) passes whatever kk is.
template <class LoadX, class LoadY>
__device__ __forceinline__ double kth_chebyshev_distance_by_pivots(int cs, int kk, int i, double pxi, double pyi,
                                                                   LoadX px, LoadY py) {
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double p = -1.0;  // distances are >= 0: -1 stands for "none"
    for (int j = 0; j < cs && p < 0.0; j++) {
        const double d = fmax(fabs(pxi - px(j)), fabs(pyi - py(j)));
        if (j != i && d == d) p = d;
    }
    if (p < 0.0) return inf;
    double lo = -1.0, hi = inf;
    bool has_hi = false;
    int need = kk;  // the answer is the need-th smallest distance above lo
#pragma unroll 1
    for (uint32_t pass = 1;; pass++) {
        int c_lt = 0, c_eq = 0;
        double a = -1.0, b = -1.0;
        uint32_t ha = 0xFFFFFFFFu, hb = 0xFFFFFFFFu;
#pragma unroll 4
        for (int j = 0; j < cs; j++) {
            const double d = fmax(fabs(pxi - px(j)), fabs(pyi - py(j)));
            const bool in = j != i && d > lo && (!has_hi || d < hi);
            const bool lt = in && d < p, gt = in && d > p;
            c_lt += lt ? 1 : 0;
            c_eq += (in && d == p) ? 1 : 0;
            const uint32_t h = (uint32_t(j) + pass * 7919u) * 2654435761u;
            if (lt && h <= ha) {
                a = d;
                ha = h;
            }
            if (gt && h <= hb) {
                b = d;
                hb = h;
            }
        }
        if (need <= c_lt) {  // c_lt >= 1: a exists
            hi = p;
            has_hi = true;
            p = a;
        } else if (need <= c_lt + c_eq) {
            return p;
        } else {
            if (b < 0.0) return inf;  // nothing above p: fewer than kk numbers (only without an upper bound)
            need -= c_lt + c_eq;
            lo = p;
            p = b;
        }
    }
}

// Kraskov: Chebyshev distance from sample i = (pxi, pyi) to its kk-th neighbour, by repeated minimum passes (each pass
// finds the smallest distance above the previous one and how many samples sit at it); many neighbours: by pivots
template <class LoadX, class LoadY>
__device__ __forceinline__ double kth_chebyshev_distance(int cs, int kk, int i, double pxi, double pyi, LoadX px,
                                                         LoadY py) {
    if (kk > kPivotSelectMinK) return kth_chebyshev_distance_by_pivots(cs, kk, i, pxi, pyi, px, py);
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double cur = -1.0, m = 0.0;
    int cnt = 0;
#pragma unroll 1
    for (int pass = 0; pass < kk; pass++) {
        m = inf;
        int c = 0;
#pragma unroll 2
        for (int j = 0; j < cs; j++) {
            const double d = fmax(fabs(pxi - px(j)), fabs(pyi - py(j)));
            if (d > cur && j != i) {
                c = (d < m) ? 1 : (d == m ? c + 1 : c);
                m = fmin(m, d);
            }
        }
        cnt += c;
        if (cnt >= kk) break;
        cur = m;
    }
    return m;
}

// ---- per-voxel evaluators of the tile kernels: `vals` / `aux` point at this lane's column -------------------------

// Binned MI from the voxel's cell codes in aux.
__device__ float binned_voxel(const uint16_t* aux, int total, bool table_ok, const double* __restrict__ tableT, int cs) {
    double mi = 0.0;
    if (total > 0) {
        const double tot = double(total);
        const double eps1 = 0.5 / double(cs);
        const double eps2 = 0.5 / double(cs * cs);
#pragma unroll 1
        for (int i = 0; i < cs; i++) {
            const uint32_t ci = aux[i * 64];
            if (ci == kSkippedCell) continue;
            int cx = 0, cy = 0, cxy = 0;
            bool fx = true, fy = true, fxy = true;
#pragma unroll 2
            for (int j = 0; j < cs; j++) {
                const uint32_t cj = aux[j * 64];
                const bool ok = cj != kSkippedCell;
                const bool ex = ok && (cj & 0xFFu) == (ci & 0xFFu);
                const bool ey = ok && (cj >> 8) == (ci >> 8);
                cx += ex;
                cy += ey;
                cxy += (ex && ey);
                if (j < i) {
                    fx = fx && !ex;
                    fy = fy && !ey;
                    fxy = fxy && !(ex && ey);
                }
            }
            mi = binned_mi_term(mi, cx, cy, cxy, fx, fy, fxy, table_ok, tableT, tot, eps1, eps2);
        }
    }
    return float(mi);
}

__device__ __forceinline__ int count_less_generic(const double* tab, int n, int top, double v) {
    int pos = 0;
    for (int step = top; step >= 1; step >>= 1) {
        const int idx = pos + step;
        const int probe = idx <= n ? idx : n;
        pos = (idx <= n && tab[probe - 1] < v) ? idx : pos;
    }
    return pos;
}

// Kraskov KSG-1 / KSG-2, any k.
__device__ float kraskov_voxel(const float* vals, const double* __restrict__ px, const double* __restrict__ spx,
                               const double* __restrict__ nq, const double* __restrict__ psi, int cs, int k,
                               int estimator, double c_term) {
    const int kk = k < cs - 1 ? k : cs - 1;
    int top = 1;
    while (top * 2 <= cs) top *= 2;
    const double factor = 1.0 / double(cs);
    const double slack = 1e-15;
    double sum_x = 0.0, sum_y = 0.0;
#pragma unroll 1
    for (int i = 0; i < cs; i++) {
        const double pxi = px[i];
        const double pyi = double(vals[i * 64]) + nq[i];
        const double m = kth_chebyshev_distance(
            cs, kk, i, pxi, pyi, [=](int j) { return px[j]; }, [=](int j) { return double(vals[j * 64]) + nq[j]; });
        double rx, ry;
        if (estimator == 1) {
            rx = ry = m - slack;
        } else {
            double ex = 0.0, ey = 0.0;
#pragma unroll 2
            for (int j = 0; j < cs; j++) {
                const double ax = fabs(pxi - px[j]), ay = fabs(pyi - (double(vals[j * 64]) + nq[j]));
                const bool in = fmax(ax, ay) <= m;
                ex = in ? fmax(ex, ax) : ex;
                ey = in ? fmax(ey, ay) : ey;
            }
            rx = ex + slack;
            ry = ey + slack;
        }
        int cx = count_less_generic(spx, cs, top, pxi + rx) - count_less_generic(spx, cs, top, pxi - rx);
        const double loy = pyi - ry, hiy = pyi + ry;
        int cy = 0;
#pragma unroll 4
        for (int j = 0; j < cs; j++) {
            const double pyj = double(vals[j * 64]) + nq[j];
            cy += (pyj >= loy && pyj < hiy) ? 1 : 0;
        }
        cx = cx > 1 ? cx : 1;
        cy = cy > 1 ? cy : 1;
        if (estimator != 1) {
            cx -= 1;
            cy -= 1;
        }
        sum_x += factor * psi[cx];
        sum_y += factor * psi[cy];
    }
    const double mi = -sum_x - sum_y + c_term + psi[cs];
    const float res = float(mi);
    return (res < 0.0f) ? 0.0f : res;
}

// ---------------------------------------------------------------------------------------------------------------
// Spearman / Kendall beyond the register kernels (cs > 128; an LDS-tile kernel measured 3.8x slower at 130
// members because a 50 KB tile per wave leaves one wave per SIMD): the O(cs^2) sweeps read the
// values straight from the member volumes (a wave's read of one member is the same coalesced 256 B as a read of a
// workspace copy would be, and with 16 rows per sweep there are 16 comparisons per value read), so no per-block copy of
// the values exists, the grid is not limited by workspace size (the old scheme ran one wave per SIMD) and only
// Spearman keeps a per-voxel column: the 16-bit doubled ranks, in a global workspace slice per block.
// ---------------------------------------------------------------------------------------------------------------

// MEASURE 1: Spearman (prep = float a_e), 2: Kendall (prep = int perm / gend / n1 with stride cs)
// LIST: the voxels are those of a todo list {count, voxel indices...} (the ones a sort-based kernel deferred: ties)
template <int MEASURE, bool LIST = false>
__global__ __launch_bounds__(64) void direct_rank_kernel(const float* const* __restrict__ members,
                                                         const void* __restrict__ prep, float* __restrict__ out,
                                                         size_t num_voxels, int cs, uint16_t* __restrict__ workspace,
                                                         const uint32_t* __restrict__ todo) {
    constexpr int measure = MEASURE;
    constexpr int T = kDirectRows;
    const int lane = threadIdx.x;
    const uint32_t bytes = uint32_t(num_voxels) * 4u;
    const int* prep_i = static_cast<const int*>(prep);
    const float* prep_a = static_cast<const float*>(prep);
    uint16_t* aux = workspace ? workspace + size_t(blockIdx.x) * size_t(cs) * 64 + lane : nullptr;
    const size_t listed = LIST ? size_t(todo[0]) : 0;
    const size_t tiles = ((LIST ? listed : num_voxels) + 63) / 64;
#pragma unroll 1
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        size_t v = t * 64 + lane;
        if constexpr (LIST) v = v < listed ? size_t(todo[1 + v]) : num_voxels;  // a lane past the end of the list: idle
        const uint32_t off = v < num_voxels ? uint32_t(v) * 4u : kOutOfRangeOffset;
        float res;
        bool is_nan = false;
        if constexpr (measure == 1) {
            is_nan = doubled_ranks<T>(cs, [=](int e) { return load_member_cached(members[e], bytes, off); }, aux);
            res = pearson2_prepared<4>(cs, prep_a, [=](int e) { return half_rank(aux, e); });
        } else {
            const int* gend = prep_i + cs;  // slot -> last slot of its x-tie group (slots = reference-sorted order)
            int32_t discordant = 0, n2 = 0;
#pragma unroll 1
            for (int i0 = 0; i0 < cs; i0 += T) {
                float yi[T];
                int gi[T];
#pragma unroll
                for (int r = 0; r < T; r++) {
                    const int i = i0 + r < cs ? i0 + r : cs - 1;
                    yi[r] = load_member_cached(members[prep_i[i]], bytes, off);
                    is_nan |= yi[r] != yi[r];
                    gi[r] = i0 + r < cs ? gend[i] : cs;
                    if (i0 + r >= cs) yi[r] = __uint_as_float(0x7FC00000u);  // a row past the end matches nothing
                }
                // the block's own columns: row r only counts j > i0 + r
#pragma unroll 1
                for (int j = i0 + 1; j < i0 + T && j < cs; j++) {
                    const float yj = load_member_cached(members[prep_i[j]], bytes, off);
#pragma unroll
                    for (int r = 0; r < T; r++) {
                        const bool after = j > i0 + r;
                        n2 += (after && yj == yi[r]) ? 1 : 0;
                        discordant += (after && j > gi[r] && yi[r] > yj) ? 1 : 0;
                    }
                }
                // every later column counts for all rows of the block
#pragma unroll 4
                for (int j = i0 + T; j < cs; j++) {
                    const float yj = load_member_cached(members[prep_i[j]], bytes, off);
#pragma unroll
                    for (int r = 0; r < T; r++) {
                        n2 += (yj == yi[r]) ? 1 : 0;
                        discordant += (j > gi[r] && yi[r] > yj) ? 1 : 0;
                    }
                }
            }
            res = tau_b(cs, prep_i[2 * cs], n2, discordant);
        }
        if (is_nan) res = __uint_as_float(0x7FC00000u);
        if (v < num_voxels) store_result_nt(out + v, res);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Symmetric field mode (CRF_FLAG_SYMMETRIC), Spearman and Kendall, any member count: both vectors of a voxel are voxel
// dependent, so nothing is prepared; same direct-read scheme as direct_rank_kernel with two member tables.
//   Spearman: doubled ranks of X and of Y by counting (two 16-bit columns per voxel in the block's workspace slice),
//             then computePearson2<float> on the two rank vectors in member order.
//   Kendall : tau-b in pair form -- S_y = #{x_a < x_b, y_a > y_b}, n1 = #{x_a == x_b}, n2 = #{y_a == y_b} over
//             unordered pairs (the sort of computeKendall orders equal x by y, so x-tied pairs add no inversion;
//             Correlation.cpp:423-455).
// ---------------------------------------------------------------------------------------------------------------
struct SymmetricBinnedArgs {
    int num_bins;  // <= 255: the code 0xFFFF of a skipped sample can then never equal a valid bin pair
    float min_x, max_x, min_y, max_y;
    int to_cc;
};

// measure 1: Spearman, 2: Kendall, 3 / 5: binned MI / its correlation coefficient (cell codes b1 << 8 | b0 in the
// voxel's 16-bit workspace column, then counts of equal bins / cells by 16-row sweeps; the first occurrence of a bin
// or cell contributes its term, exactly like the skipped-sample path of mi_binned_kernel)
// (one instantiation per measure: sharing one kernel cost Kendall 60 % through register allocation)
template <int MEASURE>
__global__ __launch_bounds__(64) void direct_symmetric_kernel(const float* const* __restrict__ members_x,
                                                              const float* const* __restrict__ members_y,
                                                              float* __restrict__ out, size_t num_voxels, int cs,
                                                              uint16_t* __restrict__ workspace, SymmetricBinnedArgs ba,
                                                              const double* __restrict__ tableT) {
    constexpr int measure = MEASURE;
    constexpr int T = kDirectRows;
    const int lane = threadIdx.x;
    const uint32_t bytes = uint32_t(num_voxels) * 4u;
    uint16_t* rx = workspace ? workspace + size_t(blockIdx.x) * size_t(cs) * 128 + lane : nullptr;
    uint16_t* ry = rx ? rx + size_t(cs) * 64 : nullptr;
    const size_t tiles = (num_voxels + 63) / 64;
#pragma unroll 1
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t v = t * 64 + lane;
        const uint32_t off = v < num_voxels ? uint32_t(v) * 4u : kOutOfRangeOffset;
        float res;
        bool is_nan = false;
        if constexpr (measure == 1) {
#pragma unroll 1
            for (int side = 0; side < 2; side++) {
                const float* const* __restrict__ m = side == 0 ? members_x : members_y;
                is_nan |= doubled_ranks<T>(cs, [=](int e) { return load_member_cached(m[e], bytes, off); },
                                           side == 0 ? rx : ry);
            }
            res = pearson2<4>(cs, [=](int e) { return half_rank(rx, e); }, [=](int e) { return half_rank(ry, e); });
        } else if constexpr (measure == 3 || measure == 5) {
            uint16_t* codes = rx;
            const float range_x = ba.max_x - ba.min_x, range_y = ba.max_y - ba.min_y;
            int total = 0;
#pragma unroll 4
            for (int e = 0; e < cs; e++) {
                const float xv = load_member_cached(members_x[e], bytes, off);
                const float yv = load_member_cached(members_y[e], bytes, off);
                is_nan |= xv != xv || yv != yv;
                const uint16_t code = cell_code((xv - ba.min_x) / range_x, (yv - ba.min_y) / range_y, ba.num_bins);
                codes[size_t(e) * 64] = code;
                total += code != kSkippedCell ? 1 : 0;
            }
            double mi = 0.0;
            const bool table_ok = total == cs;
            const double tot = double(total);
            const double eps1 = 0.5 / double(cs), eps2 = 0.5 / double(cs * cs);
#pragma unroll 1
            for (int i0 = 0; i0 < cs && total > 0; i0 += T) {
                uint32_t ci[T];
                int cx[T], cy[T], cxy[T], bx[T], by[T], bxy[T];  // counts over all j / over j < i
#pragma unroll
                for (int r = 0; r < T; r++) {
                    ci[r] = i0 + r < cs ? uint32_t(codes[size_t(i0 + r) * 64]) : kSkippedCell;
                    cx[r] = cy[r] = cxy[r] = bx[r] = by[r] = bxy[r] = 0;
                }
#pragma unroll 2
                for (int j = 0; j < cs; j++) {
                    const uint32_t cj = codes[size_t(j) * 64];
#pragma unroll
                    for (int r = 0; r < T; r++) {
                        const int ex = ((cj ^ ci[r]) & 0xFFu) == 0u ? 1 : 0;
                        const int ey = ((cj ^ ci[r]) >> 8) == 0u ? 1 : 0;
                        const int exy = cj == ci[r] ? 1 : 0;
                        const int before = j < i0 + r ? 1 : 0;
                        cx[r] += ex;
                        cy[r] += ey;
                        cxy[r] += exy;
                        bx[r] += ex & before;
                        by[r] += ey & before;
                        bxy[r] += exy & before;
                    }
                }
#pragma unroll
                for (int r = 0; r < T; r++) {
                    if (ci[r] == kSkippedCell) continue;  // skipped sample (or a row past the end)
                    mi = binned_mi_term(mi, cx[r], cy[r], cxy[r], bx[r] == 0, by[r] == 0, bxy[r] == 0, table_ok, tableT,
                                        tot, eps1, eps2);
                }
            }
            res = float(mi);
            if (measure == 5) res = mi_to_cc(res);
        } else {
            int32_t discordant = 0, n1 = 0, n2 = 0;
#pragma unroll 1
            for (int i0 = 0; i0 < cs; i0 += T) {
                float xi[T], yi[T];
#pragma unroll
                for (int r = 0; r < T; r++) {
                    const int i = i0 + r < cs ? i0 + r : cs - 1;
                    xi[r] = load_member_cached(members_x[i], bytes, off);
                    yi[r] = load_member_cached(members_y[i], bytes, off);
                    is_nan |= xi[r] != xi[r] || yi[r] != yi[r];
                }
#pragma unroll 2
                for (int j = i0 + 1; j < cs; j++) {
                    const float xj = load_member_cached(members_x[j], bytes, off);
                    const float yj = load_member_cached(members_y[j], bytes, off);
#pragma unroll
                    for (int r = 0; r < T; r++) {
                        const bool after = j > i0 + r && i0 + r < cs;
                        n1 += (after && xi[r] == xj) ? 1 : 0;
                        n2 += (after && yi[r] == yj) ? 1 : 0;
                        discordant += (after && ((xi[r] < xj && yi[r] > yj) || (xj < xi[r] && yj > yi[r]))) ? 1 : 0;
                    }
                }
            }
            res = tau_b(cs, n1, n2, discordant);
        }
        if (is_nan) res = __uint_as_float(0x7FC00000u);
        if (cs == 1) res = 1.0f;
        if (v < num_voxels) store_result_nt(out + v, res);
    }
}

// field mode only; which evaluations arrive here: two_vector_route.h
hipError_t launch_direct_symmetric(const TwoVectorJob& job, hipStream_t s) {
    const int measure = job.measure;
    if (job.requests || (measure != 1 && measure != 2 && measure != 3 && measure != 5)) return hipErrorInvalidValue;
    if (measure != 2 && !job.workspace) return hipErrorInvalidValue;
    const unsigned blocks = unsigned(persistent_blocks(job.num_voxels, kDirectBlocks));
    const SymmetricBinnedArgs ba{job.num_bins, job.min_x, job.max_x, job.min_y, job.max_y, measure == 5};
    uint16_t* ws = reinterpret_cast<uint16_t*>(job.workspace);
    const double* tableT = job.tables + (job.cs + 1);
#define CRF_LAUNCH_SYMMETRIC(M)                                                                                        \
    hipLaunchKernelGGL((direct_symmetric_kernel<M>), dim3(blocks), dim3(64), 0, s, job.members_x, job.members_y, job.out, \
                       job.num_voxels, job.cs, ws, ba, tableT)
    switch (measure) {
        case 1: CRF_LAUNCH_SYMMETRIC(1); break;
        case 2: CRF_LAUNCH_SYMMETRIC(2); break;
        case 3: CRF_LAUNCH_SYMMETRIC(3); break;
        default: CRF_LAUNCH_SYMMETRIC(5); break;
    }
#undef CRF_LAUNCH_SYMMETRIC
    return hipGetLastError();
}

// Field mode, binned MI / its correlation coefficient (measures 3, 5) and Kraskov MI / KMI-CC (4, 6) only: Spearman
// and Kendall go through direct_rank_kernel (launch_generic).  prep: the reference side's bins (int b0[cs], then
// whether every reference sample is valid) for the binned measures, px / sorted px (double) for Kraskov.
__global__ __launch_bounds__(64) void generic_kernel(const float* const* __restrict__ members,
                                                     const void* __restrict__ prep, const double* __restrict__ tables,
                                                     float* __restrict__ out, size_t num_voxels, int cs, GenericArgs a,
                                                     unsigned char* __restrict__ workspace) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* tile = workspace ? workspace + size_t(blockIdx.x) * tile_bytes(cs) : smem;
    const int lane = threadIdx.x;
    float* vals = reinterpret_cast<float*>(tile) + lane;                                        // [cs][64]
    uint16_t* aux = reinterpret_cast<uint16_t*>(tile + size_t(cs) * 64 * sizeof(float)) + lane;  // [cs][64]
    const uint32_t bytes = uint32_t(num_voxels) * 4u;
    const int* prep_i = static_cast<const int*>(prep);
    const size_t tiles = (num_voxels + 63) / 64;
    const bool binned = a.measure == 3 || a.measure == 5;
#pragma unroll 1
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t v = t * 64 + lane;
        const uint32_t byte_offset = uint32_t(v) * 4u;  // lanes past the end read 0
        bool is_nan = false;
        int total = 0;
        const float range_q = a.max_query - a.min_query;
#pragma unroll 4
        for (int e = 0; e < cs; e++) {
            const float y = load_member_nt(members[e], bytes, byte_offset);
            is_nan |= (y != y);
            vals[e * 64] = y;
            if (binned) {
                const uint16_t code = cell_code_prepared(prep_i[e], (y - a.min_query) / range_q, a.num_bins);
                aux[e * 64] = code;
                total += code != kSkippedCell ? 1 : 0;
            }
        }
        float res;
        if (binned) {
            const bool table_ok = total == cs && prep_i[cs] != 0;
            res = binned_voxel(aux, total, table_ok, tables + (cs + 1), cs);
        } else {
            const double* prep_d = static_cast<const double*>(prep);
            res = kraskov_voxel(vals, prep_d, prep_d + cs, tables + 3 * cs + 2, tables, cs, a.k, a.estimator, a.kraskov_c);
        }
        if (a.measure == 5 || a.measure == 6) res = mi_to_cc(res);
        if (is_nan) res = __uint_as_float(0x7FC00000u);
        if (v < num_voxels) store_result_nt(out + v, res);
    }
}

// =========================================================================================================
// Pair-request mode: the estimator between the ensemble vectors of two arbitrary voxels per request -- the reference's
// CorrelationComputePass request mode (src/Calculators/CorrelationCalculator.hpp:250-258, request layout
// {xi,yi,zi,i,xj,yj,zj,j} src/Renderers/Diagram/HEBChart.hpp:166-168, Data/Shaders/Correlation/RequestsBuffer.glsl:22-36)
// with the semantics of its CPU twin HEBChart::computeCorrelations (src/Renderers/Diagram/HEBChartCorrelation.cpp:493-600):
// both vectors are voxel dependent (no shared reference side), binned MI normalises with the extrema of the two
// vectors of the pair (:556-566), Kraskov is KSG-1, NaN in either vector yields NaN (the CPU twin emits no entry).
// One lane = one request; 2*cs gathered loads per request; same tile scheme as above (x, y, two u16 columns).
// =========================================================================================================
__device__ float kendall_pair(const float* x, const float* y, int cs) {
    int32_t discordant = 0, n1 = 0, n2 = 0;
#pragma unroll 1
    for (int a = 0; a < cs; a++) {
        const float xa = x[a * 64], ya = y[a * 64];
#pragma unroll 4
        for (int b = a + 1; b < cs; b++) {
            const float xb = x[b * 64], yb = y[b * 64];
            n1 += (xa == xb) ? 1 : 0;
            n2 += (ya == yb) ? 1 : 0;
            discordant += ((xa < xb && ya > yb) || (xb < xa && yb > ya)) ? 1 : 0;
        }
    }
    return tau_b(cs, n1, n2, discordant);
}

__device__ float kraskov_pair(const float* x, const float* y, const double* __restrict__ nr,
                              const double* __restrict__ nq, const double* __restrict__ psi, int cs, int k,
                              double c_term) {
    const int kk = k < cs - 1 ? k : cs - 1;
    const double factor = 1.0 / double(cs);
    double sum_x = 0.0, sum_y = 0.0;
#pragma unroll 1
    for (int i = 0; i < cs; i++) {
        const double pxi = double(x[i * 64]) + nr[i], pyi = double(y[i * 64]) + nq[i];
        const double m = kth_chebyshev_distance(
            cs, kk, i, pxi, pyi, [=](int j) { return double(x[j * 64]) + nr[j]; },
            [=](int j) { return double(y[j * 64]) + nq[j]; });
        const double r = m - 1e-15;
        const double lox = pxi - r, hix = pxi + r, loy = pyi - r, hiy = pyi + r;
        int cx = 0, cy = 0;
#pragma unroll 2
        for (int j = 0; j < cs; j++) {
            const double pxj = double(x[j * 64]) + nr[j], pyj = double(y[j * 64]) + nq[j];
            cx += (pxj >= lox && pxj < hix) ? 1 : 0;
            cy += (pyj >= loy && pyj < hiy) ? 1 : 0;
        }
        sum_x += factor * psi[cx > 1 ? cx : 1];
        sum_y += factor * psi[cy > 1 ? cy : 1];
    }
    const double mi = -sum_x - sum_y + c_term + psi[cs];
    const float res = float(mi);
    return (res < 0.0f) ? 0.0f : res;
}

// members_i / members_j: the member sets the first / second voxel of a request is read from (the same table for the
// request mode; primary / secondary field for the symmetric field mode).  requests == nullptr: request r is the
// voxel pair (r, r) -- SEPARATE_SYMMETRIC, CorrelationMain.glsl:10-15; which evaluations arrive in either mode:
// two_vector_route.h.  Binned MI normalises with the pair's own extrema (HEBChart).
struct PairArgs {
    int measure, num_bins, k, use_abs;
    double kraskov_c;  // psi(k) (pair requests are KSG-1), host-evaluated like KraskovArgs::c_term
};
__global__ __launch_bounds__(64) void pair_request_kernel(const float* const* __restrict__ members_i,
                                                          const float* const* __restrict__ members_j,
                                                          const uint32_t* __restrict__ requests,
                                                          const double* __restrict__ tables, float* __restrict__ out,
                                                          size_t num_requests, size_t num_voxels, int xs, int ys, int cs,
                                                          PairArgs a, unsigned char* __restrict__ workspace) {
    const int measure = a.measure, num_bins = a.num_bins, k = a.k, use_abs = a.use_abs;
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* tile = workspace ? workspace + size_t(blockIdx.x) * pair_tile_bytes(cs) : smem;
    const int lane = threadIdx.x;
    float* x = reinterpret_cast<float*>(tile) + lane;
    float* y = x + size_t(cs) * 64;
    uint16_t* ax = reinterpret_cast<uint16_t*>(tile + size_t(cs) * 64 * 2 * sizeof(float)) + lane;
    uint16_t* ay = ax + size_t(cs) * 64;
    const size_t tiles = (num_requests + 63) / 64;
#pragma unroll 1
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t r = t * 64 + lane;
        const bool active = r < num_requests;
        uint32_t vi = 0, vj = 0;
        if (active) {
            if (requests) {
                const uint32_t* q = requests + r * 8;
                vi = (q[2] * uint32_t(ys) + q[1]) * uint32_t(xs) + q[0];  // IDXS
                vj = (q[6] * uint32_t(ys) + q[5]) * uint32_t(xs) + q[4];
            } else {
                vi = vj = uint32_t(r);
            }
        }
        bool is_nan = false;
        float mn = __uint_as_float(0x7F7FFFFFu), mx = __uint_as_float(0xFF7FFFFFu);
#pragma unroll 4
        for (int e = 0; e < cs; e++) {
            const float xv = load_member(members_i[e], vi * 4u);
            const float yv = load_member(members_j[e], vj * 4u);
            is_nan |= (xv != xv) || (yv != yv);
            x[e * 64] = xv;
            y[e * 64] = yv;
            mn = fminf(mn, fminf(xv, yv));
            mx = fmaxf(mx, fmaxf(xv, yv));
        }
        float res;
        switch (measure) {
            case 0: res = pearson2<1>(cs, [=](int e) { return x[e * 64]; }, [=](int e) { return y[e * 64]; }); break;
            case 1:
                (void)doubled_ranks<1>(cs, [=](int e) { return x[e * 64]; }, ax);
                (void)doubled_ranks<1>(cs, [=](int e) { return y[e * 64]; }, ay);
                res = pearson2<1>(cs, [=](int e) { return half_rank(ax, e); }, [=](int e) { return half_rank(ay, e); });
                break;
            case 2: res = kendall_pair(x, y, cs); break;
            case 3:
            case 5: {
                int total = 0;
                const float range = mx - mn;
#pragma unroll 2
                for (int e = 0; e < cs; e++) {
                    const uint16_t code = cell_code((x[e * 64] - mn) / range, (y[e * 64] - mn) / range, num_bins);
                    ax[e * 64] = code;
                    total += code != kSkippedCell ? 1 : 0;
                }
                res = binned_voxel(ax, total, total == cs, tables + (cs + 1), cs);
                break;
            }
            default: res = kraskov_pair(x, y, tables + 2 * (cs + 1), tables + 3 * cs + 2, tables, cs, k, a.kraskov_c); break;
        }
        if (measure == 5 || measure == 6) res = mi_to_cc(res);
        if (use_abs) res = fabsf(res);
        if (is_nan) res = __uint_as_float(0x7FC00000u);
        if (cs == 1) res = 1.0f;
        if (active) out[r] = res;
    }
}

hipError_t launch_pair_requests(const TwoVectorJob& job, hipStream_t s) {
    const unsigned blocks = unsigned(persistent_blocks(job.num_items, kGenericBlocks));
    const bool use_lds = pair_tile_bytes(job.cs) <= kLdsTileLimit;
    if (job.num_items == 0 || (!use_lds && !job.workspace)) return hipErrorInvalidValue;
    const PairArgs a{job.measure, job.num_bins, job.k, job.use_abs, job.kraskov_c};
    hipLaunchKernelGGL(pair_request_kernel, dim3(blocks), dim3(64), use_lds ? pair_tile_bytes(job.cs) : 0, s, job.members_x,
                       job.members_y, job.requests, job.tables, job.out, job.num_items, job.num_voxels, job.xs, job.ys, job.cs,
                       a, use_lds ? nullptr : job.workspace);
    return hipGetLastError();
}

hipError_t launch_generic(const float* const* d_members, int cs, size_t num_voxels, const RefSource& ref,
                          const GenericArgs& a, const double* d_tables, float* d_prep, unsigned char* d_workspace,
                          float* d_out, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info,
                          uint32_t* d_todo) {
    switch (ref.prepare() ? a.measure : -1) {
        case -1: break;
        case 1: launch_spearman_prep(ref, d_members, cs, d_prep, s); break;
        case 2: launch_kendall_prep(ref, d_members, cs, cs, reinterpret_cast<int*>(d_prep), s); break;
        case 3:
        case 5: {
            const BinnedArgs b{a.num_bins, a.min_ref, a.max_ref, a.min_query, a.max_query, a.measure == 5};
            launch_binned_prep(ref, d_members, cs, cs, b, d_tables + (cs + 1), reinterpret_cast<int*>(d_prep), s);
            break;
        }
        case 4:
        case 6:
            launch_kraskov_prep(ref, d_members, cs, d_tables + 2 * (cs + 1), reinterpret_cast<double*>(d_prep), s);
            break;
        default: return hipErrorInvalidValue;
    }
    if (!ref.run()) return hipGetLastError();
    if (a.measure == 1 || a.measure == 2) {
        // Spearman / Kendall: the direct-read counting kernel.  At 129..256 members the pair kernels go first (two sorted
        // chunks merged through LDS, kernels_rank.hip) and the counting kernel only walks the voxels they deferred
        // (ties); CRF_RANK_PAIR=0: the counting kernel for every voxel.
        if (a.measure == 1 && !d_workspace) return hipErrorInvalidValue;
        const char* pair_env = getenv("CRF_RANK_PAIR");
        const bool try_pair = !(pair_env && *pair_env == '0');
        if (ev_begin) (void)hipEventRecord(ev_begin, s);
        const bool paired =
            try_pair && (a.measure == 1 ? launch_spearman_pair(d_members, d_prep, d_out, num_voxels, cs, d_todo, s)
                                        : launch_kendall_pair(d_members, reinterpret_cast<const int*>(d_prep), d_out,
                                                              num_voxels, cs, d_todo, s));
        const auto kernel = a.measure == 1 ? (paired ? direct_rank_kernel<1, true> : direct_rank_kernel<1, false>)
                                           : (paired ? direct_rank_kernel<2, true> : direct_rank_kernel<2, false>);
        // the list is short: grid-stride over it
        const unsigned blocks = unsigned(persistent_blocks(num_voxels, paired ? 1024 : kDirectBlocks));
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), 0, s, d_members, static_cast<const void*>(d_prep), d_out,
                           num_voxels, cs, reinterpret_cast<uint16_t*>(d_workspace),
                           static_cast<const uint32_t*>(paired ? d_todo : nullptr));
        if (ev_end) (void)hipEventRecord(ev_end, s);
        if (info)
            info->kernel_name = !paired ? "direct_rank_kernel" : a.measure == 1 ? "spearman_pair_kernel" : "kendall_pair_kernel";
        return hipGetLastError();
    }
    const unsigned blocks = unsigned(persistent_blocks(num_voxels, kGenericBlocks));
    const bool use_lds = tile_bytes(cs) <= kLdsTileLimit;
    if (!use_lds && !d_workspace) return hipErrorInvalidValue;
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    hipLaunchKernelGGL(generic_kernel, dim3(blocks), dim3(64), use_lds ? tile_bytes(cs) : 0, s, d_members,
                       static_cast<const void*>(d_prep), d_tables, d_out, num_voxels, cs, a,
                       use_lds ? nullptr : d_workspace);
    if (ev_end) (void)hipEventRecord(ev_end, s);
    if (info) info->kernel_name = "generic_kernel";
    return hipGetLastError();
}

}  // namespace crf
