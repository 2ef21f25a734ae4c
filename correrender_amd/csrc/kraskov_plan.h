// kraskov_plan.h -- which Kraskov kernel instantiation runs for (members, k): plain C++17 without HIP types, so the
// selection is testable on a machine without a GPU (tests/test_kraskov_plan.py).  kernels_kraskov.hip turns a plan into
// a kernel pointer and launch parameters; DESIGN.md section 4 has the resulting table and the measurements behind it.
#pragma once
#include <cstddef>

namespace crf {

// CRF_KRASKOV_SORTED / _DIRECT / _TILE / _DXT / _TI4 / _STAGE by their first character:
// -1 unset, 0 '0', 1 '1', 2 anything else (which only counts as "set")
struct KraskovSwitches {
    int sorted = -1, direct = -1, tile = -1, dxt = -1, ti4 = -1, stage = -1;
};

enum class KraskovFamily { Column, Direct, Sorted };  // mi_kraskov_kernel, kraskov_direct_kernel, kraskov_sorted_kernel

struct KraskovPlan {
    KraskovFamily family;
    int K, TI;   // neighbours kept in registers (>= min(k, cs - 1)), points per sweep
    bool dxt;    // x distances from the prepared table
    bool stage;  // Direct: the voxel tile staged in LDS
    int NS;      // Sorted: padded column length (32, 48, 64), else 0
};

constexpr int kDxtMaxMembers = 128;  // the x-distance table exists up to here (it lies in the preparation buffer)
// LDS of kraskov_direct_kernel: three tables of cs doubles, the staged tile of cs x 64 floats, and its static partial
// sums -- 16 (tile, wave) slots x 64 lanes x (2 doubles + 1 int)
constexpr size_t kraskov_table_bytes(int cs) { return size_t(3 * cs) * sizeof(double); }
constexpr size_t kraskov_stage_bytes(int cs) { return size_t(cs) * 64 * sizeof(float); }
constexpr size_t kDirectSumBytes = 16 * 64 * (2 * sizeof(double) + sizeof(int));

inline bool kraskov_switch(int value, bool otherwise) { return value >= 0 ? value == 1 : otherwise; }
inline int kraskov_kk(int cs, int k) { return k < cs - 1 ? k : cs - 1; }  // neighbours besides the point itself

// K and TI of the tile-free kernel without the table; k beyond 4 rounds up to the next instantiated K
inline void kraskov_direct_wide(int kk, KraskovPlan* p) {
    p->K = kk <= 8 ? 8 : kk <= 16 ? 16 : kk <= 32 ? 32 : kk <= 64 ? 64 : 128;
    p->TI = kk <= 8 ? 4 : kk <= 16 ? 2 : 1;
}

// Tile-free kernel, 2 <= cs; false: k > 128 or the tables are beyond LDS.
inline bool kraskov_direct_plan(int cs, int k, const KraskovSwitches& sw, KraskovPlan* p) {
    const int kk = kraskov_kk(cs, k);
    if (kk > 128 || kraskov_table_bytes(cs) + kDirectSumBytes > 60 * 1024) return false;
    *p = {KraskovFamily::Direct, kk, 8, false, false, 0};  // K = k exactly for the small k
    if (kk > 4) {
        kraskov_direct_wide(kk, p);
        return true;
    }
    const bool table_pays = cs <= 112 || kk == 2 || kk == 4;
    p->dxt = cs <= kDxtMaxMembers && (sw.dxt == 1 || (table_pays && sw.dxt != 0));
    if (!p->dxt) {  // 4 points per sweep gain only at K = 4 here
        p->TI = kk >= 3 && kraskov_switch(sw.ti4, kk == 4) ? 4 : 8;
        return true;
    }
    const bool fits = kraskov_table_bytes(cs) + kraskov_stage_bytes(cs) + kDirectSumBytes <= 64 * 1024;
    p->stage = fits && kraskov_switch(sw.stage, cs <= 64 && kk >= 3);
    p->TI = p->stage || kraskov_switch(sw.ti4, kk >= 3) ? 4 : 8;
    return true;
}

// Field mode, 2 <= cs.  direct_only: the entry for more than 128 members, which has the tile-free kernel alone.
// false: not supported (the caller falls back to the generic kernel).
inline bool kraskov_field_plan(int cs, int k, bool direct_only, const KraskovSwitches& sw, KraskovPlan* p) {
    if (direct_only) return kraskov_direct_plan(cs, k, sw, p);
    const int kk = kraskov_kk(cs, k);
    if (sw.sorted == 1 && kk <= 4 && cs <= 64 && sw.direct != 1) {
        *p = {KraskovFamily::Sorted, kk, 8, false, false, cs <= 32 ? 32 : cs <= 48 ? 48 : 64};
        return true;
    }
    const bool prefer_direct = kk <= 2 ? cs > 44 : (kk == 3 ? cs > 40 : (cs > 36 || (cs > 28 && cs <= 32)));
    if (kk > 4 || cs > 80 || sw.direct == 1 || (prefer_direct && sw.tile != 1)) return kraskov_direct_plan(cs, k, sw, p);
    // LDS-column kernel: 16 points per sweep only where the column caps the occupancy at two waves per SIMD anyway
    // (more than 56 members) and the member count fills the last sweep well
    const bool wide = cs > 56 && (cs % 16 == 0 || cs % 16 > 8);
    const int ti = kk == 4 ? 4 : (kk == 1 || !wide) ? 8 : 16;
    const bool table = sw.dxt == 1 ? cs <= kDxtMaxMembers : (cs <= 32 && sw.dxt != 0);
    *p = {KraskovFamily::Column, kk, ti, table && ti <= 8, false, 0};
    return true;
}

// Members stored as uint8, uint16 or float16 (format 1, 2, 3 of crf_member_format; 0 is fp32): whether the field runs
// on them as stored (kernels_kraskov_narrow.hip) and, if so, with which plan -- the field plan's family, K, TI and dxt,
// so that the native call adds its fp64 partial sums in the fp32 call's order under every switch setting.  false: the
// call runs on the fp32 copy.  The routed set is the "within rule" column of profiles/narrow_kraskov_ab.md: a cell
// (format, family, member count rounded up to 16, K) is routed only where the native kernel's time was within the fp32
// kernel's on the copy plus its run-to-run spread at every measured member count of the cell -- for the tile-free kernel
// at one count whose sweeps divide evenly among the four waves of a block and at one where they do not.  Cells that were
// not measured stay on the copy, as does the Sorted family (CRF_KRASKOV_SORTED=1).  K = min(k, members - 1) up to 4, then
// 8 for 5..8.  The K = 16 instantiation spills to scratch on narrow members as it does on fp32 and is therefore not built;
// K = 32, 64, 128 were not measured.  What passed (member counts):
//   uint8     column kernel K = 2, 3: 33..48;  tile-free kernel K = 2: 49..64, K = 3: 49..96, K = 4: 113..128,
//             K = 8: 49..64 and 113..128
//   uint16    tile-free kernel K = 2, 3: 49..64, K = 4 and K = 8: 113..128
//   float16   tile-free kernel K = 2: 49..64, K = 3: 49..64 and 113..128, K = 4: 113..128, K = 8: 49..64 and 113..128
constexpr int kKraskovNarrowMaxMembers = 128;
struct KraskovNarrowCells {  // [K - 1] for K = 1..4, then K = 8; bit n - 1: member counts 16 n - 15 .. 16 n
    unsigned column[4], direct[5];
};
constexpr KraskovNarrowCells kKraskovNarrowCells[4] = {
    {{0, 0, 0, 0}, {0, 0, 0, 0, 0}},                    // fp32
    {{0, 0x04, 0x04, 0}, {0, 0x08, 0x38, 0x80, 0x88}},  // uint8
    {{0, 0, 0, 0}, {0, 0x08, 0x08, 0x80, 0x80}},        // uint16
    {{0, 0, 0, 0}, {0, 0x08, 0x88, 0x80, 0x88}},        // float16
};

inline bool kraskov_narrow_plan(int format, int cs, int k, const KraskovSwitches& sw, KraskovPlan* p) {
    if (format < 1 || format > 3 || cs < 2 || cs > kKraskovNarrowMaxMembers) return false;
    KraskovPlan plan;
    if (!kraskov_field_plan(cs, k, false, sw, &plan) || plan.family == KraskovFamily::Sorted) return false;
    if (plan.K > 8 || (plan.family == KraskovFamily::Column && plan.K > 4)) return false;
    const KraskovNarrowCells& cells = kKraskovNarrowCells[format];
    const unsigned mask = plan.family == KraskovFamily::Column ? cells.column[plan.K - 1]
                                                                : cells.direct[plan.K <= 4 ? plan.K - 1 : 4];
    if (!(mask >> ((cs + 15) / 16 - 1) & 1u)) return false;
    *p = plan;
    return true;
}

// Symmetric field mode (kraskov_direct_kernel<K, TI, SYM>), 2 <= cs; false: k > 64 or the tables are beyond LDS.
inline bool kraskov_symmetric_plan(int cs, int k, KraskovPlan* p) {
    const int kk = kraskov_kk(cs, k);
    if (kk > 64 || kraskov_table_bytes(cs) + kDirectSumBytes > 60 * 1024) return false;
    *p = {KraskovFamily::Direct, kk, 8, false, false, 0};
    if (kk > 4) kraskov_direct_wide(kk, p);
    return true;
}

}  // namespace crf
