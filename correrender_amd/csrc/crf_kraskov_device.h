// crf_kraskov_device.h -- what the Kraskov kernels on fp32 members (kernels_kraskov.hip) and on narrow members
// (kernels_kraskov_narrow.hip) share: the layout of the preparation buffer, the fp64 single-instruction helpers, the
// batched binary search, the occupancy table of the tile-free kernel, and the host lookups of tables and switches.
#pragma once
#include <cstdlib>

#include "crf_device.h"
#include "crf_internal.h"
#include "kraskov_plan.h"

namespace crf {

// the distance table lies in the preparation buffer behind the two coordinate vectors (up to 128 members: 133 KB)
__host__ __device__ inline int dxt_offset(int cs) { return (2 * cs + 7) / 8 * 8; }  // in doubles
static_assert(size_t(((2 * kDxtMaxMembers + 7) / 8 * 8) + 128 * 128) * sizeof(double) <= kPrepBytes - 16, "prep buffer");

constexpr double kCountSlack = 1e-15;  // default_epsilon<double>::value, MutualInformation.cpp:163

// mi_kraskov_kernel<FMT, K, TI, DXT> (kernels_kraskov.hip), one wave per tile of 64 voxels, whatever FMT is:
// (members, prep, psi, noise_query, out, num_voxels, cs, k, estimator, to_cc, c_term).  Its dynamic LDS: four tables of
// doubles (px, sorted px, noise_query, psi(0..cs) padded to 16 bytes) and the cs x 64 column of converted floats.
using KraskovColumnKernel = void (*)(const void* const*, const double*, const double*, const double*, float*, size_t, int,
                                     int, int, int, double);
constexpr size_t kraskov_column_lds_bytes(int cs) {
    return size_t(4 * cs + 1 + ((cs + 1) & 1)) * sizeof(double) + size_t(cs) * 64 * sizeof(float);
}
// the instantiation for a Column plan on narrow members (kernels_kraskov.hip); nullptr where none is built
KraskovColumnKernel kraskov_column_narrow_kernel(int format, const KraskovPlan& p);

// fp64 min / max / Chebyshev distance as single instructions.  fmin()/fmax() make hipcc canonicalise each operand first
// (an extra v_max_f64 x, x); the operands here are never signalling NaNs and the k-select only needs "one of the two".
__device__ __forceinline__ double min_f64(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double max_f64(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double chebyshev_f64(double dx, double dy) {  // max(|dx|, |dy|)
    double r;
    asm("v_max_f64 %0, |%1|, |%2|" : "=v"(r) : "v"(dx), "v"(dy));
    return r;
}

__device__ __forceinline__ double chebyshev_f64_sx(double dy, double abs_dx_uniform) {  // max(|dy|, s): s in SGPRs
    double r;
    asm("v_max_f64 %0, |%1|, %2" : "=v"(r) : "v"(dy), "s"(abs_dx_uniform));
    return r;
}

// #{ t : tab[t] < v } for an ascending table of n entries; top = largest power of two <= n.  Branch-free binary search;
// the table is shared by the wave (LDS), the probe index is per lane.
__device__ __forceinline__ int count_less(const double* tab, int n, int top, double v) {
    int pos = 0;
    for (int step = top; step >= 1; step >>= 1) {
        const int idx = pos + step;
        const int probe = idx <= n ? idx : n;  // keep the read in range; the result is discarded when idx > n
        pos = (idx <= n && tab[probe - 1] < v) ? idx : pos;
    }
    return pos;
}

// The same search for NCH bounds at once: the steps are the outer loop, so a step issues NCH independent LDS reads before
// it waits (one search after the other is a chain of log2(n) dependent LDS round trips each -- and the && above
// compiles to exec-masked branches; at 8 points x 2 bounds per sweep that latency was as long as the k-select itself).
template <int NCH>
__device__ __forceinline__ void count_less_batch(const double* tab, int n, int top, const double (&v)[NCH],
                                                 int (&pos)[NCH]) {
#pragma unroll
    for (int c = 0; c < NCH; c++) pos[c] = 0;
#pragma unroll 1
    for (int step = top; step >= 1; step >>= 1) {
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const int idx = pos[c] + step;
            const bool ok = idx <= n;
            const double val = tab[(ok ? idx : n) - 1];
            pos[c] = (ok & (val < v[c])) ? idx : pos[c];
        }
    }
}

// Occupancy the register allocator is held to (waves per SIMD): what the instantiations reached before the work split
// below was added; left to itself the compiler now settles one step lower for K <= 2 and <8, 4>.
constexpr int direct_min_waves(int K, int TI, bool SYM) {
    if (SYM) return K <= 8 ? 2 : (K <= 32 ? 3 : 2);
    return K <= 2 ? 4 : (K == 3 ? 3 : (K == 4 ? 2 : (K <= 32 ? 3 : 1)));
}

struct KraskovTables {
    const double *psi, *noise_ref, *noise_query;
};
inline KraskovTables kraskov_tables(const double* d_tables, int cs) {
    const double* noise_ref = d_tables + 2 * (cs + 1);
    return {d_tables, noise_ref, noise_ref + cs};
}

inline KraskovSwitches read_switches() {  // at every call: the tests set them after the library is loaded
    auto first_char = [](const char* name) {
        const char* e = getenv(name);
        return !e ? -1 : *e == '0' ? 0 : *e == '1' ? 1 : 2;
    };
    return {first_char("CRF_KRASKOV_SORTED"), first_char("CRF_KRASKOV_DIRECT"), first_char("CRF_KRASKOV_TILE"),
            first_char("CRF_KRASKOV_DXT"),    first_char("CRF_KRASKOV_TI4"),    first_char("CRF_KRASKOV_STAGE")};
}

}  // namespace crf
