// api.cpp -- the C ABI of libcorrfield.so (include/corrfield.h) over the gfx950 kernels.
//
// Host-side responsibilities, mirroring what CorrelationCalculator::calculateCpu does around its hot loop
// (reference: src/Calculators/CorrelationCalculator.cpp:781-866): hold the member volumes (resident in HBM), obtain
// the reference vector, pick the estimator, launch, hand back xs*ys*zs floats.  No CPU fallback exists: without a
// gfx950 device every entry point fails.
#include "../../include/corrfield.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <functional>
#include <immintrin.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <limits>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "crf_context.h"
#include "crf_host_copy.h"
#include "crf_internal.h"
#include "crf_similarity_tail.h"

namespace {
thread_local std::string g_create_error;

std::string fmt(const char* f, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

int fail(crf_context* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define CRF_HIP(ctx, call)                                                                                     \
    do {                                                                                                       \
        hipError_t e_ = (call);                                                                                \
        if (e_ != hipSuccess)                                                                                  \
            return fail(ctx, CRF_ERR_DEVICE, fmt("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                                                 __LINE__));                                                   \
    } while (0)

int bind_device(crf_context* c) {
    CRF_HIP(c, hipSetDevice(c->device));
    return CRF_OK;
}

int alignment_vpt(const void* p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    return (a & 15u) == 0 ? 4 : ((a & 7u) == 0 ? 2 : 1);
}

const char* format_name(int format) {
    return format == CRF_MEMBER_U8 ? "u8" : format == CRF_MEMBER_U16 ? "u16" : format == CRF_MEMBER_F16 ? "f16" : "f32";
}

// what a launch on the whole local grid reads
crf_launch_view whole_view(const crf_context* c) {
    const crf_grid_state& g = c->grid;
    return {g.members.f32_table(), g.secondary.f32_table(), g.narrow.table.get(), c->alloc_voxels, g.members.vpt, 0,
            g.secondary_narrow.table.get()};
}

// One scalar field's members as the context holds them (crf_context.h): the fp32 set, the narrow set, the format that
// says which of the two the caller gave, and the fp32 copy of narrow ones.  Non-owning.
struct FieldMembers {
    crf_member_set& f32;
    crf_member_set& narrow;
    int& format;
    crf::DeviceBuffer<float>& wide;
    const char* label;  // how a message names the field's members
    crf_member_set& current() const { return format == CRF_MEMBER_F32 ? f32 : narrow; }
};
FieldMembers field_members(crf_context* c, bool secondary) {
    crf_grid_state& g = c->grid;
    if (secondary) return {g.secondary, g.secondary_narrow, g.secondary_format, g.secondary_wide, "secondary members"};
    return {g.members, g.narrow, g.format, g.wide, "members"};
}

// ---- what is derived from the members, and what drops it ---------------------------------------------------------------
//   derived object                         built by             reads
//   min/max cache of a set                 member_minmax        the set's values
//   host range tables (chunk_tables)       ensure_host_ranges   the pointers of `members` or of `narrow`
//   window tables                          ensure_windows       the pointers of `members` and of `secondary`
//   packed copy                            ensure_packed        the values of `members`
//   wide copy (`members` of narrow ones)   ensure_wide          the values of `narrow`
//   secondary wide copy (`secondary` of    ensure_secondary_wide  the values of `secondary_narrow`
//     narrow secondary members)
// Each function below is the whole answer to "what goes when this changes"; crf_set_grid drops everything by replacing
// the grid state.

// the packed copy; decided again at the next Pearson field evaluation (also when the layout policy changes)
void drop_packed(crf_context* c) {
    c->grid.packed.reset();
    c->grid.pack_state = 0;
}

// The fp32 view of narrow members appeared (ensure_wide): tables built while it was missing do not point into it.  The
// min/max cache stays: it holds the extrema of the narrow values, and the copy holds the same values.
void fp32_view_appeared(crf_context* c) {
    c->grid.host_chunks = 0;
    c->grid.windows = 0;
}

// The primary members were replaced (upload, bind) or overwritten in place (crf_members_changed).
void primary_members_changed(crf_context* c) {
    crf_grid_state& g = c->grid;
    g.members.minmax_valid = g.narrow.minmax_valid = false;
    g.host_chunks = 0;
    g.windows = 0;
    drop_packed(c);
    if (g.format != CRF_MEMBER_F32) {  // the wide copy, and the fp32 pointers into it
        g.wide.reset();
        g.members.ptrs.clear();
    }
}

// The fp32 view of narrow secondary members appeared (ensure_secondary_wide): the window tables are the one derived object
// that reads the secondary's fp32 pointers.
void secondary_fp32_view_appeared(crf_context* c) { c->grid.windows = 0; }

// The secondary members were replaced or overwritten in place.  The one place that drops their wide copy.
void secondary_members_changed(crf_context* c) {
    crf_grid_state& g = c->grid;
    g.secondary.minmax_valid = g.secondary_narrow.minmax_valid = false;
    g.windows = 0;
    if (g.secondary_format != CRF_MEMBER_F32) {  // the wide copy, and the fp32 pointers into it
        g.secondary_wide.reset();
        g.secondary.ptrs.clear();
    }
}

// the set's alignment facts and its device table, from set.ptrs
int install_table(crf_context* c, crf_member_set& set) {
    const uintptr_t element_mask = crf::member_format_bytes(set.format) - 1;
    set.vpt = 4;
    set.dword_aligned = set.element_aligned = true;
    for (const void* p : set.ptrs) {
        set.vpt = std::min(set.vpt, alignment_vpt(p));
        set.dword_aligned = set.dword_aligned && (reinterpret_cast<uintptr_t>(p) & 3u) == 0;
        set.element_aligned = set.element_aligned && (reinterpret_cast<uintptr_t>(p) & element_mask) == 0;
    }
    CRF_HIP(c, set.table.reserve(size_t(c->cs)));
    CRF_HIP(c, hipMemcpyAsync(set.table.get(), set.ptrs.data(), sizeof(void*) * size_t(c->cs), hipMemcpyHostToDevice,
                              c->stream));
    CRF_HIP(c, hipStreamSynchronize(c->stream));
    c->view = whole_view(c);
    return CRF_OK;
}

// Replaces the primary members (secondary == false) or the secondary ones, in any format, by cs volumes uploaded from
// host memory into one owned block, or bound where they lie in device memory.  label: how the messages name a member.
int set_members(crf_context* c, bool secondary, int format, const void* const* members, bool upload, const char* label) {
    if (!c || !members) return fail(c, CRF_ERR_ARGUMENT, "null argument");
    if (format < CRF_MEMBER_F32 || format > CRF_MEMBER_F16)
        return fail(c, CRF_ERR_ARGUMENT, fmt("unknown member format %d", format));
    if (c->cs <= 0) return fail(c, CRF_ERR_STATE, "crf_set_grid has not been called");
    for (int i = 0; i < c->cs; i++)
        if (!members[i]) return fail(c, CRF_ERR_ARGUMENT, fmt("%s %d is a null pointer", label, i));
    // the native kernels address a member with 32-bit byte offsets (crf_internal.h: kNarrowMaxBytes, just under 4 GiB)
    if (format != CRF_MEMBER_F32 && c->alloc_voxels * crf::member_format_bytes(format) >= crf::kNarrowMaxBytes)
        return fail(c, CRF_ERR_UNSUPPORTED, fmt("%s members of 4 GiB or more are not supported (%zu voxels per member)",
                                                format_name(format), c->alloc_voxels));
    if (int r = bind_device(c)) return r;
    (secondary ? secondary_members_changed : primary_members_changed)(c);
    const FieldMembers field = field_members(c, secondary);
    field.f32.clear();
    field.narrow.clear();
    field.format = format;
    crf_member_set& set = field.current();
    set.format = format;
    if (!upload) {
        set.ptrs.assign(members, members + c->cs);
        return install_table(c, set);
    }
    // every member starts 256-byte aligned (wide vector loads)
    const size_t bytes = c->alloc_voxels * crf::member_format_bytes(format);
    const size_t stride = (bytes + 255) & ~size_t(255);
    CRF_HIP(c, set.owned.reserve(stride * size_t(c->cs)));
    for (int i = 0; i < c->cs; i++) {
        set.ptrs.push_back(set.owned.get() + stride * size_t(i));
        CRF_HIP(c, hipMemcpyAsync(set.owned.get() + stride * size_t(i), members[i], bytes, hipMemcpyHostToDevice,
                                  c->stream));
    }
    return install_table(c, set);
}

// The extrema of a set's values, computed once per set of values.
int member_minmax(crf_context* c, crf_member_set& set, float* out_min, float* out_max) {
    if (!out_min || !out_max) return fail(c, CRF_ERR_ARGUMENT, "null output");
    if (!set.minmax_valid) {
        if (int r = bind_device(c)) return r;
        uint32_t* d_keys = c->minmax.get();
        if (set.format != CRF_MEMBER_F32)  // the narrow members as stored: no fp32 copy
            CRF_HIP(c, crf::launch_minmax_narrow(set.table.get(), set.format, c->cs, c->alloc_voxels, d_keys, c->stream));
        else
            CRF_HIP(c, crf::launch_minmax(set.f32_table(), c->cs, c->alloc_voxels, d_keys, c->stream));
        uint32_t keys[2];
        CRF_HIP(c, hipMemcpyAsync(keys, d_keys, sizeof keys, hipMemcpyDeviceToHost, c->stream));
        CRF_HIP(c, hipStreamSynchronize(c->stream));
        set.min_v = crf::minmax_key_to_float(keys[0]);
        set.max_v = crf::minmax_key_to_float(keys[1]);
        set.minmax_valid = true;
    }
    *out_min = set.min_v;
    *out_max = set.max_v;
    return CRF_OK;
}

// Narrow members: the fp32 copy for every evaluation without a native route (native_field, native_reduction) -- one owned
// block that `members` points into, converted on stream s at the first call that needs it.  A caller that stays on the
// native routes, the extrema and the reference gathers never pays for it.  Dropped with the members it was made from.
// The same serves the secondary field: its copy is `secondary_wide`, its fp32 set `secondary` (ensure_secondary_wide).  A
// field that is not there, or is fp32, needs nothing.
int ensure_wide_of(crf_context* c, bool secondary, hipStream_t s) {
    const FieldMembers field = field_members(c, secondary);
    if (field.format == CRF_MEMBER_F32 || !field.f32.ptrs.empty() || field.narrow.ptrs.empty()) return CRF_OK;
    if (int r = bind_device(c)) return r;
    const size_t stride = (c->alloc_voxels + 63) & ~size_t(63);
    if (field.wide.reserve(stride * size_t(c->cs)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, CRF_ERR_DEVICE, fmt("no device memory for the fp32 copy of the %s %s (%zu bytes)",
                                           format_name(field.format), field.label, stride * sizeof(float) * size_t(c->cs)));
    }
    CRF_HIP(c, crf::launch_widen_members(field.narrow.table.get(), field.format, c->cs, c->alloc_voxels, field.wide.get(),
                                         stride, s));
    for (int i = 0; i < c->cs; i++) field.f32.ptrs.push_back(field.wide.get() + stride * size_t(i));
    field.f32.vpt = 4;
    CRF_HIP(c, field.f32.table.reserve(size_t(c->cs)));
    CRF_HIP(c, hipMemcpyAsync(field.f32.table.get(), field.f32.ptrs.data(), sizeof(void*) * size_t(c->cs),
                              hipMemcpyHostToDevice, s));
    CRF_HIP(c, hipStreamSynchronize(s));
    c->view = whole_view(c);
    (secondary ? secondary_fp32_view_appeared : fp32_view_appeared)(c);
    return CRF_OK;
}
int ensure_wide(crf_context* c, hipStream_t s) { return ensure_wide_of(c, false, s); }
int ensure_secondary_wide(crf_context* c, hipStream_t s) { return ensure_wide_of(c, true, s); }

// Whether the per-voxel kernel of this field evaluation reads the narrow members as they are (view.narrow), no fp32 copy.
// Everything else -- more than kNarrowMaxMembers members, the symmetric mode but for its Pearson route below, windowed
// grids, pair requests -- runs on the fp32 copy (ensure_wide).  Per measure:
//   Pearson    2..128 members, dword loads: every member 4-byte aligned (kernels_pearson.hip: pearson_narrow_kernel)
//   Kendall    2..128 members, element loads: the element's own alignment (kernels_rank_narrow.hip)
//   Spearman   33..128 members (kernels_rank_narrow.hip); up to 32 the fp32 kernels handle ties in line and the call stays
//              on the copy (crf_internal.h: spearman_narrow_routed; profiles/narrow_spearman_ab.md).  CRF_RANK_U32 selects
//              among the fp32 kernels only: it does not move a native call.
//   binned MI  2..128 members where measured faster than the copy route (crf_internal.h: binned_narrow_routed;
//              profiles/narrow_binned_ab.md); CRF_BINNED_HIST=1 asks for the histogram kernel, which reads fp32
//   Kraskov MI 2..128 members, element loads, where measured no slower than the copy route (kraskov_plan.h:
//              kraskov_narrow_plan; profiles/narrow_kraskov_ab.md).  The CRF_KRASKOV_* switches move a native call as they
//              move an fp32 call; CRF_KRASKOV_SORTED=1 asks for the sorted-column kernel, which reads fp32
// The symmetric mode (two fields per voxel) has one native route: the Pearson field over two fields in the SAME narrow format,
// both sets 4-byte aligned (dword loads), at the member counts of symmetric_narrow_routed (symmetric_narrow_route.h;
// profiles/narrow_symmetric_ab.md) -- kernels_pearson.hip: pearson_symmetric_narrow_kernel.  Every other symmetric
// evaluation reads fp32 views of both fields (ensure_wide, ensure_secondary_wide).
bool native_field(const crf_context* c, const crf_params* p) {
    const crf_grid_state& g = c->grid;
    if (g.format == CRF_MEMBER_F32 || c->cs > crf::kNarrowMaxMembers || c->windowed) return false;
    if (p->flags & CRF_FLAG_SYMMETRIC)
        return p->measure == CRF_PEARSON && g.secondary_format == g.format && !g.secondary_narrow.ptrs.empty() &&
               g.narrow.dword_aligned && g.secondary_narrow.dword_aligned && crf::symmetric_narrow_routed(g.format, c->cs);
    switch (p->measure) {
        case CRF_PEARSON: return c->cs >= 2 && g.narrow.dword_aligned;
        case CRF_KENDALL: return c->cs >= 2 && g.narrow.element_aligned;
        case CRF_SPEARMAN:
            return c->cs >= 33 && g.narrow.element_aligned && crf::spearman_narrow_routed(g.format, c->cs);
        case CRF_MI_BINNED:
        case CRF_BINNED_MI_CC:
            if (const char* hv = getenv("CRF_BINNED_HIST"); hv && *hv == '1') return false;
            return c->cs >= 2 && g.narrow.element_aligned && crf::binned_narrow_routed(g.format, c->cs);
        case CRF_MI_KRASKOV:
        case CRF_KMI_CC: return g.narrow.element_aligned && crf::kraskov_narrow_routed(g.format, c->cs, p->k);
        default: return false;
    }
}

// The sibling reductions (ensemble mean / spread, set predicate) read narrow members with dword loads
// (kernels_stats.hip: ensemble_stat_narrow_kernel, set_predicate_narrow_kernel), at any member count.  The extrema and the
// reference gathers read narrow members element by element and ask for nothing but a narrow format.
bool native_reduction(const crf_context* c) {
    return c->grid.format != CRF_MEMBER_F32 && c->grid.narrow.dword_aligned && !c->windowed;
}

// DKL reads narrow members element by element (kernels_dkl.hip: dkl_kernel at a narrow FMT, reported as dkl_narrow_kernel; the element's own alignment), at
// any member count, where that was measured to be no slower than dkl_kernel on the copy (crf_internal.h: dkl_narrow_routed;
// profiles/narrow_dkl_ab.md).  CRF_DKL_COUNTING_SORT and CRF_DKL_BLOCKS_PER_CU move a native call as they move an fp32 call.
bool native_dkl(const crf_context* c, int estimator, int k) {
    return c->grid.format != CRF_MEMBER_F32 && c->grid.narrow.element_aligned && !c->windowed &&
           crf::dkl_narrow_routed(c->grid.format, c->cs, estimator, k);
}

// Packs the members for the Pearson field if the layout policy asks for it (include/corrfield.h: crf_member_layout),
// once per set of members, on stream s.  *use: the packed copy is there for this evaluation.
int ensure_packed(crf_context* c, hipStream_t s, crf::PackedMembers* use) {
    *use = crf::PackedMembers{};
    const int cs = c->cs;
    if (c->grid.format != CRF_MEMBER_F32) return CRF_OK;  // the packed copy is an fp32 format
    if (c->member_layout == CRF_MEMBER_LAYOUT_RAW || cs < crf::kPackMinMembers || cs > crf::kPackMaxMembers ||
        c->windowed || c->view.num_voxels != c->alloc_voxels)
        return CRF_OK;
    const bool automatic = c->member_layout == CRF_MEMBER_LAYOUT_AUTO;
    const size_t tiles = (c->view.num_voxels + 63) / 64;
    const size_t header_bytes = (tiles * size_t(crf::pack_slots(cs)) + 255) & ~size_t(255);
    crf_grid_state& g = c->grid;
    if (g.pack_state == 0) {
        g.pack_state = -1;
        if (automatic && c->view.num_voxels < (size_t(1) << 20)) return CRF_OK;  // the one-time encode would not pay off
        // padded slots are stored and read: near the bottom of a 16-slot granule the copy moves more than the members
        if (automatic && crf::pack_voxel_bytes(cs) > crf::kPackAutoByteRatio * double(4 * cs + 4)) return CRF_OK;
        const size_t bytes = header_bytes + tiles * size_t(crf::pack_tile_bytes(crf::pack_slots(cs)));
        if (automatic) {
            size_t free_b = 0, total_b = 0;
            CRF_HIP(c, hipMemGetInfo(&free_b, &total_b));
            const size_t keep = std::max(size_t(8) << 30, total_b / 10);
            if (free_b < bytes || free_b - bytes < keep) return CRF_OK;
        }
        CRF_HIP(c, c->pack_fallbacks.reserve(1));
        if (g.packed.reserve(bytes) != hipSuccess) {
            (void)hipGetLastError();
            if (automatic) return CRF_OK;
            return fail(c, CRF_ERR_DEVICE, fmt("no device memory for the packed members (%zu bytes)", bytes));
        }
        uint32_t* d_fallbacks = c->pack_fallbacks.get();
        CRF_HIP(c, hipMemsetAsync(d_fallbacks, 0, sizeof(uint32_t), s));
        CRF_HIP(c, crf::launch_pack_members(c->view.members, cs, c->view.num_voxels, g.packed.get(),
                                            g.packed.get() + header_bytes, d_fallbacks, s));
        uint32_t fallbacks = 0;
        CRF_HIP(c, hipMemcpyAsync(&fallbacks, d_fallbacks, sizeof fallbacks, hipMemcpyDeviceToHost, s));
        CRF_HIP(c, hipStreamSynchronize(s));
        if (automatic && double(fallbacks) > 0.05 * double(tiles) * double(cs)) {
            drop_packed(c);
            g.pack_state = -1;
            return CRF_OK;
        }
        g.pack_state = 1;
    }
    if (g.pack_state == 1) *use = crf::PackedMembers{g.packed.get(), g.packed.get() + header_bytes};
    return CRF_OK;
}

// Host-built fp64 tables that depend on the member count only.
//   psi(n) at integers: the reference calls boost::math::digamma on positive integers only
//     (MutualInformation.cpp:235,237,438,439,503,504) = -gamma + H_{n-1}; accumulated in long double.
//   T[c] = p ln p, p = c/cs: the value computeMutualInformationBinned adds for a bin holding c of cs samples
//     (MutualInformation.cpp:120-140), evaluated with the host libm log like the reference.
//   noise: the 1e-10 tie-breaking jitter of the Kraskov estimator (MutualInformation.cpp:409-420).  sgl's
//     XorshiftRandomGenerator is not available (un-vendored, unpinned); this is the repo's documented stream:
//     Marsaglia xorshift32 (13,17,5), seeds 617406168 / 864730169, u = (state >> 8) * 2^-24.
std::vector<double> build_tables(int cs) {
    std::vector<double> t(size_t(4 * cs + 2));
    const long double gamma = 0.577215664901532860606512090082402431L;
    long double h = 0.0L;
    t[0] = std::numeric_limits<double>::quiet_NaN();
    for (int n = 1; n <= cs; n++) {
        t[size_t(n)] = double(h - gamma);
        h += 1.0L / (long double)n;
    }
    double* T = t.data() + (cs + 1);
    T[0] = 0.0;
    for (int c = 1; c <= cs; c++) {
        const double p = double(c) / double(cs);
        T[c] = p * std::log(p);
    }
    const uint32_t seeds[2] = {617406168u, 864730169u};
    for (int w = 0; w < 2; w++) {
        uint32_t s = seeds[w];
        double* dst = t.data() + 2 * (cs + 1) + w * cs;
        for (int e = 0; e < cs; e++) {
            s ^= s << 13;
            s ^= s >> 17;
            s ^= s << 5;
            dst[e] = double(float(s >> 8) * (1.0f / 16777216.0f)) * 1e-10;
        }
    }
    return t;
}

// psi(n) = -gamma + H_{n-1} at a positive integer, the same long-double accumulation as build_tables()
double psi_int(int n) {
    long double h = 0.0L;
    for (int i = 1; i < n; i++) h += 1.0L / (long double)i;
    return double(h - 0.577215664901532860606512090082402431L);
}
// the k-dependent constant of the KSG estimators: psi(k) (KSG-1, MutualInformation.cpp:438) or psi(k) - 1/k (KSG-2, :503)
double kraskov_c_term(int k, int estimator) {
    double c = psi_int(k);
    if (estimator != 1) c -= 1.0 / double(k);
    return c;
}

int check_ready(crf_context* c) {
    if (!c) return CRF_ERR_ARGUMENT;
    if (c->cs <= 0 || c->alloc_voxels == 0) return fail(c, CRF_ERR_STATE, "crf_set_grid has not been called");
    const crf_member_set& current = c->grid.format == CRF_MEMBER_F32 ? c->grid.members : c->grid.narrow;
    if (int(current.ptrs.size()) != c->cs)
        return fail(c, CRF_ERR_STATE, "no member volumes uploaded or bound");
    return CRF_OK;
}

crf::Event take_event(crf_context* c) {  // empty: none could be created
    crf::Event e;
    if (!c->ev_free.empty()) {
        e = std::move(c->ev_free.back());
        c->ev_free.pop_back();
    } else {
        (void)e.create();
    }
    return e;
}

hipStream_t stream_of(crf_context* c, void* stream) { return stream ? static_cast<hipStream_t>(stream) : c->stream; }

// a launcher's hipError_t as the ABI status
int launch_status(crf_context* c, hipError_t e) {
    if (e == hipSuccess) return CRF_OK;
    return fail(c, CRF_ERR_DEVICE, fmt("kernel launch failed: %s", hipGetErrorString(e)));
}

// One timed launch.  Takes an event pair when profiling is on, for the launcher to record around its per-voxel kernel;
// finish() names the kernel for crf_last_kernel_name, queues the pair for crf_take_kernel_time and maps the launcher's
// hipError_t to the ABI status.
struct TimedLaunch {
    crf_context* c;
    crf::Event e0, e1;
    crf::LaunchInfo info;
    explicit TimedLaunch(crf_context* ctx, bool timed = true) : c(ctx) {
        if (c->profiling && timed) {
            e0 = take_event(c);
            e1 = take_event(c);
        }
    }
    int finish(hipError_t e) {
        c->last_kernel = info.kernel_name ? info.kernel_name : "";
        if (e0 && e1) c->ev_pending.emplace_back(std::move(e0), std::move(e1));
        return launch_status(c, e);
    }
};

// The only place that validates a crf_params.  member_limit: the most members the mode's kernels take (0: any number);
// who: the mode as the member-limit message names it (null: field mode, which names the measure).
int check_params(crf_context* c, const crf_params* p, int member_limit, const char* who = nullptr) {
    if (!p) return fail(c, CRF_ERR_ARGUMENT, "null argument");
    if (p->measure < CRF_PEARSON || p->measure > CRF_KMI_CC)
        return fail(c, CRF_ERR_ARGUMENT, fmt("unknown measure %d", p->measure));
    for (int v : p->reserved)
        if (v != 0) return fail(c, CRF_ERR_ARGUMENT, "crf_params.reserved must be zero");
    if (member_limit > 0 && c->cs > member_limit)
        return fail(c, CRF_ERR_UNSUPPORTED,
                    who ? fmt("%s at most %d members", who, member_limit)
                        : fmt("measure %d supports at most %d members (got %d)", p->measure, member_limit, c->cs));
    if ((p->measure == CRF_MI_BINNED || p->measure == CRF_BINNED_MI_CC) && (p->num_bins < 1 || p->num_bins > 255))
        return fail(c, CRF_ERR_ARGUMENT, fmt("num_bins %d outside [1,255]", p->num_bins));
    // any k >= 1, like the reference (its k+1-nearest-neighbour query returns at most cs points; psi(k) itself is used)
    if ((p->measure == CRF_MI_KRASKOV || p->measure == CRF_KMI_CC) && p->k < 1)
        return fail(c, CRF_ERR_ARGUMENT, fmt("k=%d must be at least 1", p->k));
    return CRF_OK;
}

// prepared slots [first, first + count); one: the call takes the single slot `first` and says so
int check_slots(crf_context* c, int first, int count, bool one = false) {
    if (count >= 0 && first >= 0 && first + count <= CRF_PREPARED_SLOTS) return CRF_OK;
    return fail(c, CRF_ERR_ARGUMENT,
                one ? fmt("slot %d outside [0,%d)", first, CRF_PREPARED_SLOTS)
                    : fmt("slots [%d, %d) outside [0, %d)", first, first + count, CRF_PREPARED_SLOTS));
}

// Scratch that the per-voxel kernels write (crf_context.h: crf_scratch).  Both functions size every set that the
// evaluation being issued uses: set 0 alone, or both sets under the range pipeline of compute_to_host, whose ranges run on
// two streams and may not share a list or a workspace slice.  The pipeline issues its reference-side preparation through
// the same dispatch as its ranges, with pipeline_voxels = its largest range, before the first range is launched: that
// call sizes everything, and the calls for the ranges find it large enough (no growth, no synchronisation, between ranges).
// the most voxels one launch of the evaluation being issued covers: what its blockIdx-indexed workspace is sized for
size_t launch_voxels(const crf_context* c) { return c->pipeline_voxels ? c->pipeline_voxels : c->view.num_voxels; }

int ensure_workspace(crf_context* c, size_t need) {
    for (int set = 0; set < c->pipeline_sets; set++) {
        crf_scratch& sc = c->grid.scratch[set];
        if (need <= sc.workspace.count()) continue;
        CRF_HIP(c, hipDeviceSynchronize());  // an earlier evaluation on a caller stream may still use the old workspace
        CRF_HIP(c, sc.workspace.reserve(need));
    }
    return CRF_OK;
}

// The buffer of the device-wide sort (crf_context.h: rank_scratch).  Only synchronous calls on the context's own stream
// use it, so nothing can still be reading an old one.
int ensure_rank_scratch(crf_context* c, size_t need) {
    crf::DeviceBuffer<unsigned char>& buf = c->grid.rank_scratch;
    if (need <= buf.count()) return CRF_OK;
    if (buf.reserve(need) != hipSuccess) {
        (void)hipGetLastError();  // the failed allocation is reported here, not by the next launch
        return fail(c, CRF_ERR_DEVICE, fmt("the sort needs %zu bytes of device memory, which could not be allocated", need));
    }
    return CRF_OK;
}

// The sort-based rank kernels' list of deferred voxels.  Set 0 serves the device entry points as well: the whole local
// grid (num_voxels == alloc_voxels whenever no NarrowScope is active).  Set 1 only ever holds one range.
int ensure_todo(crf_context* c) {
    for (int set = 0; set < c->pipeline_sets; set++) {
        crf_scratch& sc = c->grid.scratch[set];
        const size_t need = set == 0 ? c->alloc_voxels : c->pipeline_voxels;
        if (need + 1 <= sc.todo.count()) continue;
        if (sc.todo) CRF_HIP(c, hipDeviceSynchronize());  // another range layout than the one it was sized for
        CRF_HIP(c, sc.todo.reserve(need + 1));  // a counter, then `need` indices
    }
    return CRF_OK;
}

int ensure_out(crf_context* c) {  // device result of the host-output calls
    CRF_HIP(c, c->grid.out.reserve(c->alloc_voxels));
    return CRF_OK;
}

// ---- member volumes of 4 GiB and more: evaluation in windows (the arithmetic: crf_windows.h) --------------------------
int ensure_windows(crf_context* c) {
    crf_grid_state& g = c->grid;
    if (g.windows > 0) return CRF_OK;
    const int windows = crf_window_count(c);
    const bool sec = !g.secondary.ptrs.empty();
    std::vector<const float*> table(size_t(windows) * size_t(c->cs) * (sec ? 2 : 1));
    for (int w = 0; w < windows; w++) {
        const size_t first = crf::window_first(size_t(w), c->window_voxels);
        for (int m = 0; m < c->cs; m++) {
            table[(size_t(w) * (sec ? 2 : 1)) * size_t(c->cs) + size_t(m)] = g.members.f32(m) + first;
            if (sec) table[(size_t(w) * 2 + 1) * size_t(c->cs) + size_t(m)] = g.secondary.f32(m) + first;
        }
    }
    CRF_HIP(c, g.window_tables.reserve(table.size()));
    CRF_HIP(c, hipMemcpy(g.window_tables.get(), table.data(), table.size() * sizeof(float*), hipMemcpyHostToDevice));
    g.windows = windows;
    g.window_has_secondary = sec;
    return CRF_OK;
}

// narrows the context to one window of a >= 4 GiB grid, or to one voxel range of a host-output evaluation, for the
// duration of a launch; restores it on every exit path
struct NarrowScope {
    crf_context* c;
    const crf_launch_view whole;
    explicit NarrowScope(crf_context* ctx) : c(ctx), whole(ctx->view) {}
    size_t select_window(int w) {  // returns the window's first voxel
        const crf_grid_state& g = c->grid;
        const size_t per = size_t(g.window_has_secondary ? 2 : 1) * size_t(c->cs);
        c->view.members = g.window_tables.get() + size_t(w) * per;
        if (g.window_has_secondary) c->view.secondary = g.window_tables.get() + size_t(w) * per + size_t(c->cs);
        c->view.num_voxels = crf::window_length(c->alloc_voxels, size_t(w), c->window_voxels);
        return crf::window_first(size_t(w), c->window_voxels);
    }
    void select_range(int j, int scratch_set) {  // range j of ensure_host_ranges, writing the scratch of its stream
        const crf_grid_state& g = c->grid;
        const void* const* range_table = g.chunk_tables.get() + size_t(j) * size_t(c->cs);
        if (g.chunk_native)
            c->view.narrow = range_table;
        else
            c->view.members = reinterpret_cast<const float* const*>(range_table);
        c->view.num_voxels = g.chunk_first[j + 1] - g.chunk_first[j];
        c->view.scratch_set = scratch_set;
    }
    ~NarrowScope() { c->view = whole; }
};

// runs launch(out + first voxel of the window) for every window of a >= 4 GiB grid, or once for an ordinary grid
template <class Launch>
int for_each_window(crf_context* c, float* out, Launch&& launch) {
    if (!c->windowed) return launch(out);
    if (int r = ensure_windows(c)) return r;
    NarrowScope scope(c);
    for (int w = 0; w < c->grid.windows; w++) {
        const size_t first = scope.select_window(w);
        if (int r = launch(out + first)) return r;
    }
    return CRF_OK;
}

// ---- two vectors per item: the symmetric field mode and pair requests -------------------------------------------------
bool env_is_one(const char* name) {
    const char* v = getenv(name);
    return v && *v == '1';
}

// what both modes take from the context and the parameters; the caller adds its items, members_y, use_abs and out
crf::TwoVectorJob two_vector_job(const crf_context* c, const crf_params* p) {
    crf::TwoVectorJob job{};
    job.members_x = job.members_y = c->view.members;
    job.cs = c->cs, job.xs = c->xs, job.ys = c->ys;
    job.num_voxels = c->view.num_voxels;
    job.measure = p->measure, job.num_bins = p->num_bins, job.k = p->k;
    job.min_x = p->min_ref, job.max_x = p->max_ref, job.min_y = p->min_query, job.max_y = p->max_query;
    job.kraskov_c = kraskov_c_term(p->k > 0 ? p->k : 1, 1);
    job.tables = c->grid.tables.get();
    return job;
}

// One two-vector evaluation: takes the route (two_vector_route.h), reserves the workspace that route needs, calls the one
// launcher.  *kernel: the name the route reports; *e: the launcher's status.  Returns non-zero only where the workspace
// could not be had.
int run_two_vector(crf_context* c, crf::TwoVectorJob job, bool force_counting, hipStream_t s, const char** kernel,
                   hipError_t* e) {
    using crf::TwoVectorKernel;
    const bool requests = job.requests || job.num_items == 0;  // field mode has voxels; an empty list may come as null
    const TwoVectorKernel route = crf::two_vector_route(requests, job.measure, job.cs, job.k, job.num_bins, force_counting,
                                                        job.num_items < (size_t(1) << 32));
    *kernel = crf::two_vector_kernel_name(route, requests, job.measure);
    *e = hipSuccess;
    if (job.num_items == 0) return CRF_OK;  // an empty request list
    const size_t need = route == TwoVectorKernel::DirectSymmetric
                            ? crf::direct_symmetric_workspace_bytes(job.cs, job.num_voxels, job.measure)
                        : route == TwoVectorKernel::PairRequest ? crf::pair_workspace_bytes(job.cs, job.num_items)
                                                                : 0;
    if (int r = ensure_workspace(c, need)) return r;
    job.workspace = c->grid.scratch[0].workspace.get();
    const bool binned = job.measure == CRF_MI_BINNED || job.measure == CRF_BINNED_MI_CC;
    switch (route) {
        case TwoVectorKernel::Fill: *e = crf::launch_fill(job.out, job.num_items, 1.0f, s); break;
        case TwoVectorKernel::PearsonRegister: *e = crf::launch_pearson_two_vector(job, s); break;
        case TwoVectorKernel::KraskovDirect: *e = crf::launch_mi_kraskov_symmetric(job, s); break;
        case TwoVectorKernel::Sorted: *e = binned ? crf::launch_sorted_binned(job, s) : crf::launch_sorted_rank(job, s); break;
        case TwoVectorKernel::DirectSymmetric: *e = crf::launch_direct_symmetric(job, s); break;
        case TwoVectorKernel::PairRequest: *e = crf::launch_pair_requests(job, s); break;
    }
    return CRF_OK;
}

// CRF_FLAG_SYMMETRIC: measure(primary members at v, secondary members at v) for every voxel v
int compute_symmetric(crf_context* c, const crf_params* p, float* out, hipStream_t s) {
    TimedLaunch launch(c);
    if (launch.e0) (void)hipEventRecord(launch.e0, s);
    crf::TwoVectorJob job = two_vector_job(c, p);
    job.members_y = c->view.secondary;
    job.num_items = c->view.num_voxels;
    job.out = out;
    hipError_t e;
    // CRF_SYMMETRIC_DIRECT=1 (tuning / tests): the any-member-count kernel instead of the sort-based ones
    if (int r = run_two_vector(c, job, env_is_one("CRF_SYMMETRIC_DIRECT"), s, &launch.info.kernel_name, &e)) return r;
    if (launch.e0 && launch.e1) (void)hipEventRecord(launch.e1, s);
    return launch.finish(e);
}

// ... and its native route (native_field): the Pearson field over two fields in one narrow format, read as stored
int compute_symmetric_narrow(crf_context* c, float* out, hipStream_t s) {
    TimedLaunch launch(c);
    const int format = c->grid.format;
    const uintptr_t vector_bytes = format == CRF_MEMBER_U8 ? 16 : 8;  // one lane's results
    return launch.finish(crf::launch_pearson_symmetric_narrow(c->view.narrow, c->view.secondary_narrow, format, c->cs,
                                                              c->view.num_voxels,
                                                              reinterpret_cast<uintptr_t>(out) % vector_bytes == 0, out, s,
                                                              launch.e0, launch.e1, &launch.info));
}

int ref_voxel(crf_context* c, int x, int y, int z, size_t* voxel) {
    if (x < 0 || y < 0 || z < 0 || x >= c->xs || y >= c->ys || z >= c->zs)
        return fail(c, CRF_ERR_ARGUMENT,
                    fmt("reference point (%d,%d,%d) outside the local grid %dx%dx%d", x, y, z, c->xs, c->ys, c->zs));
    *voxel = (size_t(z) * size_t(c->ys) + size_t(y)) * size_t(c->xs) + size_t(x);  // IDXS, DataSet.hpp:37
    return CRF_OK;
}

// device_out[m] = the value of secondary member m at `voxel`: narrow secondary members as stored (no fp32 copy, any alignment)
int gather_secondary_reference(crf_context* c, size_t voxel, float* device_out, hipStream_t s) {
    if (c->grid.secondary_format != CRF_MEMBER_F32)
        CRF_HIP(c, crf::launch_gather_reference_narrow(c->view.secondary_narrow, c->grid.secondary_format, c->cs, voxel,
                                                       device_out, s));
    else
        CRF_HIP(c, crf::launch_gather_reference(c->view.secondary, c->cs, voxel, device_out, s));
    return CRF_OK;
}

// ---- device result -> the caller's (pageable) host buffer -------------------------------------------------------------
// The caller of calculateCpu owns a freshly allocated `new float[xs*ys*zs]` (VolumeData.cpp:1222-1226): pageable and never
// touched.  Measured on MI355X hosts at 256^3 (67 MB, profiles/r03_host_boundary.md): one DMA into pinned memory 1.19 ms
// (56.5 GB/s, the PCIe floor); a kernel storing straight into device-mapped pinned memory 1.22 ms; 8 host threads move
// pinned -> resident pageable memory at 120 GB/s but only at 14 GB/s into never-touched pages (first-touch faults).
//
// So a host-output evaluation is a pipeline over a few voxel RANGES (ensure_host_ranges):
//   GPU     the per-voxel kernel of each range stores its results straight into a pinned, device-mapped staging buffer
//           (no device-side result buffer, no DMA engine: the stores cross PCIe while the kernel runs -- the kernel is
//           simply throttled to the link rate, which is the floor anyway);
//   host    a persistent pool of copier threads (crf_pool.h) moves each finished range from the staging buffer into
//           the caller's buffer, and while it waits for a range it faults the destination pages of the ranges ahead in
//           (MADV_POPULATE_WRITE batches the faults; transparent huge pages are requested for the buffer first).
// Range sizes are staggered over two streams so that kernel ends alternate and the last copy is small (ensure_host_ranges).
// CRF_HOST_PATH=dma keeps results in HBM and copies each range with the DMA engine instead (also used when a post-pass
// has to read the result back: CRF_FLAG_ABSOLUTE_VALUE).
// The host half -- range partition, thread shares, pre-faulting, the copier loop -- is crf_host_copy.h (no HIP in it:
// tests/native/host_copy.cpp runs it against a scripted producer).
int env_int_or(const char* name, int fallback) {
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : fallback;
}

int ensure_copy_pool(crf_context* c) {
    if (c->copy_pool) return CRF_OK;
    const unsigned hw = std::thread::hardware_concurrency();
    int cap = int(std::min<unsigned>(16u, std::max(1u, hw / 2)));
    if (c->copy_threads_cap > 0) cap = std::min(cap, c->copy_threads_cap);
    const int forced = env_int_or("CRF_COPY_THREADS", 0);
    if (forced >= 1) cap = std::min(forced, 64);
    // copier threads idle-spin for a short while only: back-to-back evaluations hand over within ~0.1 ms
    c->copy_pool = std::make_unique<crf::SpinPool>(cap, nullptr, 300e-6);
    c->copy_threads = cap;
    if (forced >= 1 || cap <= 2) return CRF_OK;
    // one-off calibration: how many of the pool's threads move pinned -> pageable memory fastest on this host
    const size_t bytes = std::min<size_t>(c->alloc_voxels * sizeof(float), size_t(16) << 20);
    std::vector<char> dst(bytes, 1);
    const char* src = reinterpret_cast<const char*>(c->grid.staging.host());
    double best = 1e30;
    for (int t : {2, 4, 8, 12, 16}) {
        if (t > cap) break;
        double fastest = 1e30;
        for (int rep = 0; rep < 3; rep++) {
            const auto t0 = std::chrono::steady_clock::now();
            c->copy_pool->run([&](int w) -> int {
                if (w >= t) return 0;
                size_t lo, hi;
                crf::thread_share(0, bytes, w, t, &lo, &hi);
                if (lo < hi) memcpy(dst.data() + lo, src + lo, hi - lo);
                return 0;
            });
            fastest = std::min(fastest, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        }
        if (fastest < best * 0.93) {  // more threads only for a real gain
            best = fastest;
            c->copy_threads = t;
        }
    }
    return CRF_OK;
}

// Plain form for small results and the sibling reductions: kernel into HBM, one copy.
int copy_result_to_host(crf_context* c, const float* d_src, float* host_out, size_t count) {
    CRF_HIP(c, hipMemcpyAsync(host_out, d_src, count * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    CRF_HIP(c, hipStreamSynchronize(c->stream));
    return CRF_OK;
}

// One evaluation of the field or symmetric mode on the context as it is narrowed right now.
// phase: bit 0 = reference-side preparation, bit 1 = per-voxel kernel (crf_internal.h RefSource::phase);
// slot < 0: the context's own preparation buffer
int compute_impl_one(crf_context* c, const crf_params* p, const void* device_reference_values, void* device_out,
                     void* stream, unsigned phase, int slot, const crf::RefOverride* ov) {
    if (int r = check_ready(c)) return r;
    const bool symmetric = p && (p->flags & CRF_FLAG_SYMMETRIC);
    const bool any_member_count = p && p->measure == CRF_PEARSON && !symmetric;  // the Pearson field kernel
    if (int r = check_params(c, p, any_member_count ? 0 : crf::kMaxGenericMembers,
                             symmetric ? "the symmetric mode supports" : nullptr))
        return r;
    if (!device_out && (phase & 2u)) return fail(c, CRF_ERR_ARGUMENT, "null argument");
    if (int r = bind_device(c)) return r;
    hipStream_t s = stream_of(c, stream);
    float* out = static_cast<float*>(device_out);
    const bool native = native_field(c, p);
    if (ov && c->grid.format != CRF_MEMBER_F32)
        return fail(c, CRF_ERR_UNSUPPORTED, "a direct reference read needs fp32 members");
    if (!native)
        if (int r = ensure_wide(c, s)) return r;
    if (phase & 2u) c->last_format = native ? c->grid.format : CRF_MEMBER_F32;
    if (symmetric) {
        if (phase != 3u) return fail(c, CRF_ERR_ARGUMENT, "the symmetric mode has no reference-side preparation");
        if (!c->grid.has_secondary())
            return fail(c, CRF_ERR_STATE, "CRF_FLAG_SYMMETRIC needs secondary members (crf_upload_secondary_members)");
        if (native) return compute_symmetric_narrow(c, out, s);
        if (int r = ensure_secondary_wide(c, s)) return r;
        return for_each_window(c, out, [&](float* o) { return compute_symmetric(c, p, o, s); });
    }
    float* prep = c->prep.get();
    if (slot >= 0) {
        CRF_HIP(c, c->prep_slots.reserve(size_t(CRF_PREPARED_SLOTS) * (crf::kPrepBytes / sizeof(float))));
        prep = c->prep_slots.get() + size_t(slot) * (crf::kPrepBytes / sizeof(float));
    }

    // 1. reference vector (CorrelationCalculator.cpp:802-818): a device array, a host array (copied stream-ordered),
    //    or the reference point -- then the gather is fused into the estimator's preparation kernel.
    crf::RefSource ref{static_cast<const float*>(device_reference_values), 0};
    ref.phase = phase;
    if (!(phase & 1u)) {
        ref.values = nullptr;  // prepared earlier: no reference vector is read
    } else if (!ref.values && ov) {
        // crf_group, direct exchange: the preparation kernel reads the values out of another context's members
        ref.table = ov->table;
        ref.voxel = ov->voxel;
    } else if (!ref.values && (p->flags & CRF_FLAG_REFERENCE_FROM_SECONDARY)) {
        if (!c->grid.has_secondary())
            return fail(c, CRF_ERR_STATE, "CRF_FLAG_REFERENCE_FROM_SECONDARY needs secondary members");
        size_t voxel;
        if (int r = ref_voxel(c, p->ref_x, p->ref_y, p->ref_z, &voxel)) return r;
        if (int r = gather_secondary_reference(c, voxel, c->grid.ref.get(), s)) return r;
        ref.values = c->grid.ref.get();
    }
    if ((phase & 1u) && !ref.values && !ref.table) {
        if (p->reference_values) {
            CRF_HIP(c, hipMemcpyAsync(c->grid.ref.get(), p->reference_values, sizeof(float) * size_t(c->cs),
                                      hipMemcpyHostToDevice, s));
            ref.values = c->grid.ref.get();
        } else {
            if (int r = ref_voxel(c, p->ref_x, p->ref_y, p->ref_z, &ref.voxel)) return r;
        }
    }

    // 2. estimator
    TimedLaunch launch(c, phase & 2u);
    const hipEvent_t e0 = launch.e0, e1 = launch.e1;
    crf::LaunchInfo* info = &launch.info;
    const bool binned = p->measure == CRF_MI_BINNED || p->measure == CRF_BINNED_MI_CC;
    const bool kraskov = p->measure == CRF_MI_KRASKOV || p->measure == CRF_KMI_CC;
    const int est = p->kraskov_estimator_index == 2 ? 2 : 1;  // clamp as CorrelationCalculator.cpp:765
    const crf::BinnedArgs ba{p->num_bins, p->min_ref, p->max_ref, p->min_query, p->max_query,
                             p->measure == CRF_BINNED_MI_CC};
    const crf_scratch& scratch = c->grid.scratch[c->view.scratch_set];  // filled in by ensure_todo / ensure_workspace below
    hipError_t e = hipErrorNotSupported;
    if (p->measure != CRF_PEARSON && c->cs > crf::kMaxSortMembers) {
        // any-member-count path: a specialised kernel where one applies, else kernels_generic.hip
        if (binned) {  // O(cs) histogram kernel, unless there are too many bins for the LDS rows
            e = crf::launch_mi_binned_hist(c->view.members, c->cs, c->view.num_voxels, ref, ba, c->grid.tables.get(), prep, out, s, e0,
                                           e1, info);
        } else if (kraskov) {  // tile-free single-sweep top-K kernel, unless k > 128 or the tables are beyond LDS
            const crf::KraskovArgs ka{p->k, est, p->measure == CRF_KMI_CC, kraskov_c_term(p->k, est)};
            e = crf::launch_mi_kraskov_direct(c->view.members, c->cs, c->view.num_voxels, ref, ka, c->grid.tables.get(), prep, out, s,
                                              e0, e1, info);
        }
        if (e == hipErrorNotSupported) {  // the O(cs^2) counting / repeated-minimum kernels
            if (int r = ensure_workspace(c, crf::generic_workspace_bytes(c->cs, launch_voxels(c)))) return r;
            const crf::GenericArgs ga{p->measure, p->num_bins, p->min_ref, p->max_ref, p->min_query, p->max_query, p->k,
                                      est, kraskov_c_term(p->k > 0 ? p->k : 1, est)};
            const bool rank_measure = p->measure == CRF_SPEARMAN || p->measure == CRF_KENDALL;
            if (rank_measure && c->cs <= 256)
                if (int r = ensure_todo(c)) return r;
            e = crf::launch_generic(c->view.members, c->cs, c->view.num_voxels, ref, ga, c->grid.tables.get(), prep, scratch.workspace.get(),
                                    out, s, e0, e1, info, rank_measure ? scratch.todo.get() : nullptr);
        }
        return launch.finish(e);
    }
    if (native && (phase & 1u) && !ref.values) {  // the reference point: its converted values (fp32), through grid.ref
        CRF_HIP(c, crf::launch_gather_reference_narrow(c->view.narrow, c->grid.format, c->cs, ref.voxel, c->grid.ref.get(), s));
        ref.values = c->grid.ref.get();
    }
    switch (p->measure) {
        case CRF_PEARSON: {
            if (native) {
                const uintptr_t vector_bytes = c->grid.format == CRF_MEMBER_U8 ? 16 : 8;  // one lane's results
                e = crf::launch_pearson_narrow(c->view.narrow, c->grid.format, c->cs, c->view.num_voxels,
                                               reinterpret_cast<uintptr_t>(out) % vector_bytes == 0, ref, prep, out, s, e0,
                                               e1, info);
                if (phase & 2u) c->last_layout = CRF_MEMBER_LAYOUT_RAW;
                break;
            }
            crf::PackedMembers packed;
            if (phase & 2u)
                if (int r = ensure_packed(c, s, &packed)) return r;
            e = crf::launch_pearson(c->view.members, c->cs, c->view.num_voxels, std::min(c->view.max_vpt, alignment_vpt(out)), ref,
                                    prep, out, s, e0, e1, info, packed);
            if (phase & 2u) c->last_layout = packed.header ? CRF_MEMBER_LAYOUT_PACKED : CRF_MEMBER_LAYOUT_RAW;
            break;
        }
        case CRF_SPEARMAN:
        case CRF_KENDALL:
            if (native) {  // on narrow members: one pass, no todo list; the reference side is fp32 as ever
                e = (p->measure == CRF_SPEARMAN ? crf::launch_spearman_narrow : crf::launch_kendall_narrow)(
                    c->view.narrow, c->grid.format, c->cs, c->view.num_voxels, ref, prep, out, s, e0, e1, info);
                break;
            }
            if (c->cs > 16)
                if (int r = ensure_todo(c)) return r;
            e = (p->measure == CRF_SPEARMAN ? crf::launch_spearman : crf::launch_kendall)(
                c->view.members, c->cs, c->view.num_voxels, ref, prep, scratch.todo.get(), out, s, e0, e1, info);
            break;
        case CRF_MI_BINNED:
        case CRF_BINNED_MI_CC:
            if (native) {  // binned MI on narrow members: the reference side is fp32 as ever
                e = crf::launch_mi_binned_narrow(c->view.narrow, c->grid.format, c->cs, c->view.num_voxels, ref, ba, c->grid.tables.get(),
                                                 prep, out, s, e0, e1, info);
                break;
            }
            if (const char* hv = getenv("CRF_BINNED_HIST"); hv && *hv == '1')  // tuning: histogram kernel for any cs
                e = crf::launch_mi_binned_hist(c->view.members, c->cs, c->view.num_voxels, ref, ba, c->grid.tables.get(), prep, out, s,
                                               e0, e1, info);
            if (e == hipErrorNotSupported)
                e = crf::launch_mi_binned(c->view.members, c->cs, c->view.num_voxels, ref, ba, c->grid.tables.get(), prep, out, s,
                                          e0, e1, info);
            break;
        case CRF_MI_KRASKOV:
        case CRF_KMI_CC: {
            const crf::KraskovArgs ka{p->k, est, p->measure == CRF_KMI_CC, kraskov_c_term(p->k, est)};
            if (native) {  // Kraskov MI on narrow members: the reference side is fp32 as ever
                e = crf::launch_mi_kraskov_narrow(c->view.narrow, c->grid.format, c->cs, c->view.num_voxels, ref, ka,
                                                  c->grid.tables.get(), prep, out, s, e0, e1, info);
                break;
            }
            e = crf::launch_mi_kraskov(c->view.members, c->cs, c->view.num_voxels, ref, ka, c->grid.tables.get(), prep, out, s,
                                       e0, e1, info);
            break;
        }
    }
    const int rc = launch.finish(e);
    if (e == hipErrorNotSupported)
        return fail(c, CRF_ERR_UNSUPPORTED, fmt("measure %d is not implemented by this build", p->measure));
    return rc;
}

// An ordinary grid: one call.  A grid whose members are 4 GiB or larger: the reference side once, from the whole grid
// (the reference point indexes it with 64 bits), then the per-voxel kernel window by window.
int compute_impl(crf_context* c, const crf_params* p, const void* device_reference_values, void* device_out,
                 void* stream, unsigned phase, int slot, const crf::RefOverride* ov = nullptr) {
    if (!c || !c->windowed || !p || (p->flags & CRF_FLAG_SYMMETRIC))
        return compute_impl_one(c, p, device_reference_values, device_out, stream, phase, slot, ov);
    if (int r = ensure_wide(c, stream_of(c, stream))) return r;  // the window tables point into the fp32 members
    if (phase & 1u)
        if (int r = compute_impl_one(c, p, device_reference_values, nullptr, stream, 1u, slot, ov)) return r;
    if (!(phase & 2u)) return CRF_OK;
    if (!device_out) return fail(c, CRF_ERR_ARGUMENT, "null argument");
    return for_each_window(c, static_cast<float*>(device_out), [&](float* o) {
        return compute_impl_one(c, p, nullptr, o, stream, 2u, slot, nullptr);
    });
}

// CRF_FLAG_ABSOLUTE_VALUE after a device evaluation (opt-in: what the reference's accelerator paths do)
int apply_abs(crf_context* c, const crf_params* p, void* device_out, void* stream) {
    if (p->flags & CRF_FLAG_ABSOLUTE_VALUE)
        CRF_HIP(c, crf::launch_abs(static_cast<float*>(device_out), c->view.num_voxels, stream_of(c, stream)));
    return CRF_OK;
}

// The voxel ranges of a host-output evaluation: one member-pointer table per range (pointers advanced by the range's
// first voxel), so that every per-voxel kernel can be launched on a range without knowing about ranges.  Range lengths
// are multiples of 1024 voxels (4 KiB: every range stays as aligned as the members themselves) and shrink towards the
// end: the copy of the last range into the caller's buffer is the only host work no kernel hides.
// native (the evaluation is a native_field one): the tables point into the narrow members, advanced by whole elements.
// A range starts at a multiple of 1024 voxels, so its pointers are as aligned as the members' own (the fact native_field
// asked about) and every range but the last is whole dwords.  Else they point into the fp32 members.
int ensure_host_ranges(crf_context* c, bool native) {
    crf_grid_state& g = c->grid;
    if (g.host_chunks > 0 && g.chunk_native == native) return CRF_OK;
    g.host_chunks = 0;
    const size_t n = c->alloc_voxels;
    // experiments: CRF_HOST_CHUNKS equal ranges, or CRF_HOST_SHARES comma-separated shares of 64
    const std::vector<size_t> first = crf::host_range_partition(n, env_int_or("CRF_HOST_CHUNKS", 0),
                                                                crf::parse_shares(getenv("CRF_HOST_SHARES")), kMaxHostChunks);
    const int ranges = int(first.size()) - 1;
    std::vector<const void*> table(size_t(ranges) * size_t(c->cs));
    const crf_member_set& set = native ? g.narrow : g.members;
    const size_t element = crf::member_format_bytes(set.format);
    for (int j = 0; j < ranges; j++)
        for (int m = 0; m < c->cs; m++)
            table[size_t(j) * size_t(c->cs) + size_t(m)] =
                static_cast<const char*>(set.ptrs[size_t(m)]) + first[size_t(j)] * element;
    CRF_HIP(c, g.chunk_tables.reserve(table.size()));
    CRF_HIP(c, hipMemcpy(g.chunk_tables.get(), table.data(), table.size() * sizeof(void*), hipMemcpyHostToDevice));
    CRF_HIP(c, c->copy_stream.create());
    for (int j = 0; j < ranges; j++) CRF_HIP(c, c->chunk_done[j].create(hipEventDisableTiming));
    for (int j = 0; j < ranges; j++) CRF_HIP(c, c->chunk_copied[j].create(hipEventDisableTiming));
    CRF_HIP(c, c->prep_done.create(hipEventDisableTiming));
    for (int j = 0; j <= ranges; j++) g.chunk_first[j] = first[size_t(j)];
    g.host_chunks = ranges;
    g.chunk_native = native;
    return CRF_OK;
}

// The ensemble-stat, set-predicate and DKL device calls: launch(out, stream, timed launch) once, or once per window of
// a >= 4 GiB grid (stopping at the first window that fails), as one timed launch.  native: the launch reads the members in
// their narrow format (native_reduction, and DKL where dkl_narrow_routed says so: never windowed), so no fp32 copy is built.
template <class Launch>
int run_windowed(crf_context* c, void* device_out, void* stream, bool native, Launch&& launch) {
    if (int r = bind_device(c)) return r;
    hipStream_t s = stream_of(c, stream);
    if (!native)
        if (int r = ensure_wide(c, s)) return r;
    TimedLaunch timed(c);
    hipError_t e = hipSuccess;
    const int rc = for_each_window(c, static_cast<float*>(device_out), [&](float* o) {
        e = launch(o, s, timed);
        return e == hipSuccess ? CRF_OK : CRF_ERR_DEVICE;
    });
    if (int r = timed.finish(e)) return r;
    return rc;  // not CRF_OK: the window tables could not be built
}

// ... and their host forms: device_call(device buffer) into the context's result buffer, one copy
template <class DeviceCall>
int to_host(crf_context* c, float* host_out, DeviceCall&& device_call) {
    if (int r = check_ready(c)) return r;
    if (!host_out) return fail(c, CRF_ERR_ARGUMENT, "null output");
    if (int r = bind_device(c)) return r;
    if (int r = ensure_out(c)) return r;
    if (int r = device_call(c->grid.out.get())) return r;
    return copy_result_to_host(c, c->grid.out.get(), host_out, c->alloc_voxels);
}

}  // namespace

extern "C" {

int crf_abi_version(void) { return 5; }

const char* crf_last_error(const crf_context* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int crf_create(int device_ordinal, crf_context** out_ctx) {
    if (!out_ctx) return CRF_ERR_ARGUMENT;
    *out_ctx = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        g_create_error = fmt("no HIP device available (%s); libcorrfield has no CPU fallback",
                             e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
        return CRF_ERR_DEVICE;
    }
    if (device_ordinal < 0 || device_ordinal >= count) {
        g_create_error = fmt("device ordinal %d out of range [0,%d)", device_ordinal, count);
        return CRF_ERR_ARGUMENT;
    }
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device_ordinal);
    if (e != hipSuccess) {
        g_create_error = fmt("hipGetDeviceProperties: %s", hipGetErrorString(e));
        return CRF_ERR_DEVICE;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = fmt("device %d is %s; libcorrfield is built for gfx950 (MI355X) only", device_ordinal,
                             prop.gcnArchName);
        return CRF_ERR_DEVICE;
    }
    auto* c = new crf_context();
    c->device = device_ordinal;
    auto bail = [&](const char* what, hipError_t err) {
        g_create_error = fmt("%s: %s", what, hipGetErrorString(err));
        crf_destroy(c);
        return CRF_ERR_DEVICE;
    };
    if ((e = hipSetDevice(device_ordinal)) != hipSuccess) return bail("hipSetDevice", e);
    if ((e = c->stream.create()) != hipSuccess) return bail("hipStreamCreate", e);
    if ((e = c->prep.reserve(crf::kPrepBytes / sizeof(float))) != hipSuccess) return bail("hipMalloc(prep)", e);
    if ((e = c->minmax.reserve(2)) != hipSuccess) return bail("hipMalloc(minmax)", e);
    *out_ctx = c;
    return CRF_OK;
}

// The owners in the context release everything, in the order crf_context.h states.
void crf_destroy(crf_context* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

int crf_set_grid(crf_context* c, int xs, int ys, int zs, int cs) {
    if (!c) return CRF_ERR_ARGUMENT;
    if (xs <= 0 || ys <= 0 || zs <= 0 || cs <= 0)
        return fail(c, CRF_ERR_ARGUMENT, fmt("invalid grid %dx%dx%d with %d members", xs, ys, zs, cs));
    const size_t n = size_t(xs) * size_t(ys) * size_t(zs);
    // CRF_WINDOW_VOXELS (tests): another window size, so that a small grid takes the windowed routes (crf_windows.h)
    // It is read here like CRF_HOST_CHUNKS and CRF_COPY_THREADS are read where they apply, but strictly: env_int_or's atoi
    // would take "1024abc" for 1024, and a value that does not count must fail, not fall back.
    const char* window_text = getenv("CRF_WINDOW_VOXELS");
    const long long window_override = crf::parse_window_override(window_text);
    if (window_override < 0)
        return fail(c, CRF_ERR_ARGUMENT, fmt("CRF_WINDOW_VOXELS=%.64s is neither 0 nor a positive multiple of %zu voxels up to %zu",
                                             window_text, crf::kWindowGranule, crf::kMaxWindowVoxels));
    if (int r = bind_device(c)) return r;
    CRF_HIP(c, hipDeviceSynchronize());  // evaluations the caller left in flight on its own streams still read the scratch
    c->grid = crf_grid_state{};  // the members, everything derived from them and everything sized for the old grid
    c->view = crf_launch_view{};
    c->xs = xs;
    c->ys = ys;
    c->zs = zs;
    c->cs = cs;
    c->alloc_voxels = n;
    // The kernels address a member with 32-bit byte offsets, and their out-of-range sentinel offset (crf_device.h
    // kOutOfRangeOffset = 0xFFFFFFF0) must lie beyond the end of every member: a member volume of 4 GiB or more (1024^3 is
    // exactly 4 GiB; the reference has no limit) is evaluated in WINDOWS of 2^29 voxels, one launch each, through
    // member-pointer tables advanced by the window's first voxel (ensure_windows above; the rule and the override:
    // crf_windows.h).  Both are captured here for the life of this grid.
    c->windowed = crf::grid_windowed(n, size_t(window_override));
    c->window_voxels = crf::window_voxels(size_t(window_override));
    CRF_HIP(c, c->grid.members.table.reserve(size_t(cs)));
    CRF_HIP(c, c->grid.narrow.table.reserve(size_t(cs)));
    CRF_HIP(c, c->grid.ref.reserve(size_t(cs)));
    const std::vector<double> tables = build_tables(cs);
    CRF_HIP(c, c->grid.tables.reserve(tables.size()));
    CRF_HIP(c, hipMemcpy(c->grid.tables.get(), tables.data(), tables.size() * sizeof(double), hipMemcpyHostToDevice));
    c->view = whole_view(c);
    return CRF_OK;
}

int crf_window_count(const crf_context* c) {
    if (!c) return 0;
    return c->windowed ? int(crf::windows_covering(c->alloc_voxels, c->window_voxels)) : 1;
}

int crf_set_kraskov_noise(crf_context* c, const double* ref_noise, const double* query_noise) {
    if (!c) return CRF_ERR_ARGUMENT;
    if (c->cs <= 0 || !c->grid.tables) return fail(c, CRF_ERR_STATE, "crf_set_grid has not been called");
    if ((ref_noise == nullptr) != (query_noise == nullptr))
        return fail(c, CRF_ERR_ARGUMENT, "crf_set_kraskov_noise: give both tables, or NULL for both (default stream)");
    if (int r = bind_device(c)) return r;
    const size_t cs = size_t(c->cs);
    std::vector<double> both(2 * cs);
    if (ref_noise) {
        for (size_t e = 0; e < cs; e++) {
            // the estimator's contract: a jitter far below the data's resolution, never negative
            if (!(ref_noise[e] >= 0.0 && ref_noise[e] < 1e-9) || !(query_noise[e] >= 0.0 && query_noise[e] < 1e-9))
                return fail(c, CRF_ERR_ARGUMENT, fmt("crf_set_kraskov_noise: entry %zu outside [0, 1e-9)", e));
            both[e] = ref_noise[e];
            both[cs + e] = query_noise[e];
        }
    } else {
        const std::vector<double> t = build_tables(c->cs);
        std::copy(t.begin() + 2 * (c->cs + 1), t.end(), both.begin());
    }
    CRF_HIP(c, hipStreamSynchronize(c->stream));
    CRF_HIP(c, hipMemcpy(c->grid.tables.get() + 2 * (cs + 1), both.data(), both.size() * sizeof(double), hipMemcpyHostToDevice));
    return CRF_OK;
}

int crf_upload_members(crf_context* c, const float* const* host_members) {
    return set_members(c, false, CRF_MEMBER_F32, reinterpret_cast<const void* const*>(host_members), true, "member");
}

int crf_bind_members_device(crf_context* c, const void* const* device_members) {
    return set_members(c, false, CRF_MEMBER_F32, device_members, false, "member");
}

int crf_upload_members_format(crf_context* c, int format, const void* const* host_members) {
    return set_members(c, false, format, host_members, true, "member");
}

int crf_bind_members_device_format(crf_context* c, int format, const void* const* device_members) {
    return set_members(c, false, format, device_members, false, "member");
}

int crf_member_format(const crf_context* c) { return c ? c->grid.format : CRF_MEMBER_F32; }

int crf_last_member_format(const crf_context* c) { return c ? c->last_format : CRF_MEMBER_F32; }

size_t crf_wide_copy_bytes(const crf_context* c) { return c ? c->grid.wide.count() * sizeof(float) : 0; }

int crf_member_minmax(crf_context* c, float* out_min, float* out_max) {
    if (int r = check_ready(c)) return r;
    return member_minmax(c, c->grid.format == CRF_MEMBER_F32 ? c->grid.members : c->grid.narrow, out_min, out_max);
}

int crf_member_minmax_divergent(crf_context* c, int secondary, float* out_min, float* out_max) {
    float mn = 0.f, mx = 0.f;
    if (int r = secondary ? crf_secondary_member_minmax(c, &mn, &mx) : crf_member_minmax(c, &mn, &mx)) return r;
    const float max_abs = std::max(std::abs(mn), std::abs(mx));  // VolumeData.cpp:1662-1666
    *out_min = -max_abs;
    *out_max = max_abs;
    return CRF_OK;
}

int crf_upload_secondary_members(crf_context* c, const float* const* host_members) {
    return set_members(c, true, CRF_MEMBER_F32, reinterpret_cast<const void* const*>(host_members), true,
                       "secondary member");
}

int crf_bind_secondary_members_device(crf_context* c, const void* const* device_members) {
    return set_members(c, true, CRF_MEMBER_F32, device_members, false, "secondary member");
}

int crf_upload_secondary_members_format(crf_context* c, int format, const void* const* host_members) {
    return set_members(c, true, format, host_members, true, "secondary member");
}

int crf_bind_secondary_members_device_format(crf_context* c, int format, const void* const* device_members) {
    return set_members(c, true, format, device_members, false, "secondary member");
}

int crf_secondary_member_format(const crf_context* c) { return c ? c->grid.secondary_format : CRF_MEMBER_F32; }

size_t crf_secondary_wide_copy_bytes(const crf_context* c) { return c ? c->grid.secondary_wide.count() * sizeof(float) : 0; }

int crf_secondary_member_minmax(crf_context* c, float* out_min, float* out_max) {
    if (int r = check_ready(c)) return r;
    if (!out_min || !out_max) return fail(c, CRF_ERR_ARGUMENT, "null output");
    if (!c->grid.has_secondary()) return fail(c, CRF_ERR_STATE, "no secondary members are bound");
    return member_minmax(c, field_members(c, true).current(), out_min, out_max);
}

int crf_gather_reference_device(crf_context* c, int x, int y, int z, void* device_out, void* stream) {
    if (int r = check_ready(c)) return r;
    if (!device_out) return fail(c, CRF_ERR_ARGUMENT, "null output");
    size_t voxel;
    if (int r = ref_voxel(c, x, y, z, &voxel)) return r;
    if (int r = bind_device(c)) return r;
    hipStream_t s = stream_of(c, stream);
    if (c->grid.format != CRF_MEMBER_F32)  // the converted values of the narrow members: no fp32 copy
        CRF_HIP(c, crf::launch_gather_reference_narrow(c->view.narrow, c->grid.format, c->cs, voxel,
                                                       static_cast<float*>(device_out), s));
    else
        CRF_HIP(c, crf::launch_gather_reference(c->view.members, c->cs, voxel, static_cast<float*>(device_out), s));
    return CRF_OK;
}

int crf_gather_reference_rows_device(crf_context* c, const int32_t* xyz, int num_rows, void* device_rows, void* stream) {
    if (int r = check_ready(c)) return r;
    if (!xyz || !device_rows) return fail(c, CRF_ERR_ARGUMENT, "null argument");
    if (num_rows < 0 || num_rows > crf::kMaxGatherRows)
        return fail(c, CRF_ERR_ARGUMENT, fmt("num_rows %d outside [0,%d]", num_rows, crf::kMaxGatherRows));
    crf::GatherRows rows;
    for (int r = 0; r < num_rows; r++) {
        rows.voxel[r] = crf::kNoVoxel;
        if (xyz[3 * r + 2] >= 0)
            if (int e = ref_voxel(c, xyz[3 * r], xyz[3 * r + 1], xyz[3 * r + 2], &rows.voxel[r])) return e;
    }
    if (int r = bind_device(c)) return r;
    hipStream_t s = stream_of(c, stream);
    if (c->grid.format != CRF_MEMBER_F32)
        CRF_HIP(c, crf::launch_gather_reference_rows_narrow(c->view.narrow, c->grid.format, c->cs, rows, num_rows,
                                                            static_cast<float*>(device_rows), s));
    else
        CRF_HIP(c, crf::launch_gather_reference_rows(c->view.members, c->cs, rows, num_rows,
                                                     static_cast<float*>(device_rows), s));
    return CRF_OK;
}

int crf_gather_reference(crf_context* c, int x, int y, int z, float* host_out) {
    if (!host_out) return fail(c, CRF_ERR_ARGUMENT, "null output");
    if (int r = crf_gather_reference_device(c, x, y, z, c ? c->grid.ref.get() : nullptr, nullptr)) return r;
    CRF_HIP(c, hipMemcpyAsync(host_out, c->grid.ref.get(), sizeof(float) * size_t(c->cs), hipMemcpyDeviceToHost, c->stream));
    CRF_HIP(c, hipStreamSynchronize(c->stream));
    return CRF_OK;
}

}  // extern "C"

namespace crf {

int gather_reference_to(crf_context* c, bool secondary, int x, int y, int z, float* device_out, hipStream_t s) {
    if (int r = check_ready(c)) return r;
    if (secondary && !c->grid.has_secondary()) return fail(c, CRF_ERR_STATE, "no secondary members are bound");
    size_t voxel;
    if (int r = ref_voxel(c, x, y, z, &voxel)) return r;
    if (int r = bind_device(c)) return r;
    if (secondary) return gather_secondary_reference(c, voxel, device_out, s);
    if (c->grid.format != CRF_MEMBER_F32)
        CRF_HIP(c, launch_gather_reference_narrow(c->view.narrow, c->grid.format, c->cs, voxel, device_out, s));
    else
        CRF_HIP(c, launch_gather_reference(c->view.members, c->cs, voxel, device_out, s));
    return CRF_OK;
}

int second_stream(crf_context* c, hipStream_t* out) {
    if (int r = bind_device(c)) return r;
    CRF_HIP(c, c->stream2.create());
    *out = c->stream2;
    return CRF_OK;
}

int reference_override(crf_context* owner, bool secondary, int x, int y, int z, RefOverride* out) {
    if (int r = check_ready(owner)) return r;
    if (secondary && !owner->grid.has_secondary()) return fail(owner, CRF_ERR_STATE, "no secondary members are bound");
    if (int r = ref_voxel(owner, x, y, z, &out->voxel)) return r;
    if ((secondary ? owner->grid.secondary_format : owner->grid.format) != CRF_MEMBER_F32)
        return fail(owner, CRF_ERR_UNSUPPORTED, "a direct reference read needs fp32 members");
    out->table = secondary ? owner->view.secondary : owner->view.members;
    return CRF_OK;
}

int compute_device_ex(crf_context* c, const crf_params* p, const void* device_reference_values, void* device_out,
                      void* stream, const RefOverride* ov) {
    if (!ov) return crf_compute_device(c, p, device_reference_values, device_out, stream);
    if (!p || p->prepared_slot != 0) return fail(c, CRF_ERR_ARGUMENT, "a direct reference read cannot use a prepared slot");
    if (int r = compute_impl(c, p, device_reference_values, device_out, stream, 3u, -1, ov)) return r;
    return apply_abs(c, p, device_out, stream);
}

int prepare_device_ex(crf_context* c, const crf_params* p, const void* device_reference_values, int slot, void* stream,
                      const RefOverride* ov) {
    if (int r = check_slots(c, slot, 1, true)) return r;
    return compute_impl(c, p, device_reference_values, nullptr, stream, 1u, slot, ov);
}

// What calculateCpu(t, e, buffer) does, into the caller's host buffer (Calculator.hpp:123-124, VolumeData.cpp:1222-1226):
// the pipeline described above copy_result_to_host.  The reference-side preparation runs once, from the whole-grid
// member table (the reference point indexes the whole grid); the per-voxel kernels run range by range.
int compute_to_host(crf_context* c, const crf_params* p, const void* device_reference_values, float* host_out,
                    const RefOverride* ov) {
    if (int r = check_ready(c)) return r;
    if (!host_out || !p) return fail(c, CRF_ERR_ARGUMENT, "null argument");
    if (int r = bind_device(c)) return r;
    const size_t bytes = c->alloc_voxels * sizeof(float);
    const bool ranged = !(p->flags & CRF_FLAG_SYMMETRIC) && p->prepared_slot == 0 && bytes >= (size_t(8) << 20) &&
                        !c->windowed && env_int_or("CRF_PLAIN_D2H", 0) != 1;
    if (!ranged) {
        if (int r = ensure_out(c)) return r;
        if (int r = compute_device_ex(c, p, device_reference_values, c->grid.out.get(), nullptr, ov)) return r;
        return copy_result_to_host(c, c->grid.out.get(), host_out, c->alloc_voxels);
    }
    const bool native = native_field(c, p);
    if (!native)
        if (int r = ensure_wide(c, c->stream)) return r;  // (the second stream is ordered behind the preparation below)
    if (int r = ensure_host_ranges(c, native)) return r;
    const int ranges = c->grid.host_chunks;
    // pinned, device-mapped staging for the whole local result
    CRF_HIP(c, c->grid.staging.allocate(c->alloc_voxels));
    if (int r = ensure_copy_pool(c)) return r;
    const char* path_env = getenv("CRF_HOST_PATH");
    const bool dma = (path_env && strcmp(path_env, "dma") == 0) || (p->flags & CRF_FLAG_ABSOLUTE_VALUE);
    if (dma)
        if (int r = ensure_out(c)) return r;
    {
        hipStream_t unused;
        if (int r = second_stream(c, &unused)) return r;
    }
    const bool two_streams = env_int_or("CRF_HOST_STREAMS", 2) == 2;
    const int fault_mode = env_int_or("CRF_HOST_FAULT", 2);           // 0 none, 1 touch, 2 MADV_POPULATE_WRITE
    const bool huge = env_int_or("CRF_HOST_HUGEPAGE", 1) == 1;        // ask for transparent huge pages first
    const bool trace = env_int_or("CRF_HOST_TRACE", 0) == 1;
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_call).count(); };

    // 0. host side first: the copier threads start faulting the destination in while the launches below are issued
    char* dst = reinterpret_cast<char*>(host_out);
    const char* src = reinterpret_cast<const char*>(c->grid.staging.host());
    if (huge && fault_mode != 0) {
        const uintptr_t a = (reinterpret_cast<uintptr_t>(dst) + (size_t(2) << 20) - 1) & ~((uintptr_t(2) << 20) - 1);
        const uintptr_t e = (reinterpret_cast<uintptr_t>(dst) + bytes) & ~((uintptr_t(2) << 20) - 1);
        if (e > a) (void)madvise(reinterpret_cast<void*>(a), e - a, MADV_HUGEPAGE);  // a hint; failure is harmless
    }
    for (int j = 0; j < ranges; j++) c->chunk_ready[j].store(0, std::memory_order_relaxed);
    const int threads = c->copy_threads;
    std::atomic<int>* ready = c->chunk_ready;
    const size_t* first = c->grid.chunk_first;
    const std::function<int(int)> copy_job = [=](int w) -> int {
        return crf::copy_ranges(dst, src, first, ranges, threads, ready, fault_mode, w);
    };
    c->copy_pool->start(copy_job);
    const double t_pool = trace ? since() : 0.0;
    // every exit below has to release the copier threads first
    auto abort_copy = [&](int rc) {
        for (int j = 0; j < ranges; j++) c->chunk_ready[j].store(-1, std::memory_order_release);
        c->copy_pool->wait();
        return rc;
    };

    // 1. reference-side tables, once.  The call goes through the dispatch the ranges go through, so it also sizes the
    //    scratch they write, for the largest range and one set per stream (ensure_todo): ranges in flight together are
    //    on different streams, so they write different lists, counters and workspace slices.
    struct PipelineScratch {
        crf_context* c;
        PipelineScratch(crf_context* ctx, int sets, size_t voxels) : c(ctx) {
            c->pipeline_sets = sets;
            c->pipeline_voxels = voxels;
        }
        ~PipelineScratch() {
            c->pipeline_sets = 1;
            c->pipeline_voxels = 0;
        }
    };
    size_t largest = 0;
    for (int j = 0; j < ranges; j++) largest = std::max(largest, c->grid.chunk_first[j + 1] - c->grid.chunk_first[j]);
    const PipelineScratch sized(c, two_streams ? 2 : 1, largest);
    if (int r = compute_impl(c, p, device_reference_values, nullptr, nullptr, 1u, -1, ov)) return abort_copy(r);
    const double t_prep = trace ? since() : 0.0;
    if (two_streams) {
        if (hipEventRecord(c->prep_done, c->stream) != hipSuccess || hipStreamWaitEvent(c->stream2, c->prep_done, 0) != hipSuccess)
            return abort_copy(fail(c, CRF_ERR_DEVICE, "ordering the second stream after the preparation failed"));
    }
    // 2. per-voxel kernels, range by range, alternating between two streams (the next range fills the GPU while the
    //    last waves of the previous one drain); results go straight to the mapped staging buffer, or to HBM + DMA
    float* out_base = dma ? c->grid.out.get() : c->grid.staging.device();
    {
        NarrowScope scope(c);
        for (int j = 0; j < ranges; j++) {
            const bool second = two_streams && !(j & 1);  // range 0 on the second stream
            scope.select_range(j, second ? 1 : 0);
            hipStream_t s = second ? c->stream2 : c->stream;
            float* out = out_base + c->grid.chunk_first[j];
            if (int r = compute_impl(c, p, nullptr, out, s, 2u, -1)) return abort_copy(r);
            if (p->flags & CRF_FLAG_ABSOLUTE_VALUE)
                if (launch_abs(out, c->view.num_voxels, s) != hipSuccess) return abort_copy(fail(c, CRF_ERR_DEVICE, "launch_abs failed"));
            if (hipEventRecord(c->chunk_done[j], s) != hipSuccess) return abort_copy(fail(c, CRF_ERR_DEVICE, "hipEventRecord failed"));
            if (dma) {
                const size_t off = c->grid.chunk_first[j], count = c->grid.chunk_first[j + 1] - off;
                if (hipStreamWaitEvent(c->copy_stream, c->chunk_done[j], 0) != hipSuccess ||
                    hipMemcpyAsync(c->grid.staging.host() + off, c->grid.out.get() + off, count * sizeof(float), hipMemcpyDeviceToHost,
                                   c->copy_stream) != hipSuccess ||
                    hipEventRecord(c->chunk_copied[j], c->copy_stream) != hipSuccess)
                    return abort_copy(fail(c, CRF_ERR_DEVICE, "enqueueing the copy of a result range failed"));
            }
        }
    }
    const double t_issued = trace ? since() : 0.0;
    // 3. release each range to the copier threads as it lands in the staging buffer
    for (int j = 0; j < ranges; j++) {
        const hipError_t e = crf::spin_on_event(dma ? c->chunk_copied[j] : c->chunk_done[j]);
        if (e != hipSuccess) return abort_copy(fail(c, CRF_ERR_DEVICE, fmt("waiting for result range %d failed: %s", j, hipGetErrorString(e))));
        c->chunk_ready[j].store(1, std::memory_order_release);
        if (trace) fprintf(stderr, "crf_compute: range %d (%zu voxels) landed at %.0f us\n", j, c->grid.chunk_first[j + 1] - c->grid.chunk_first[j], since());
    }
    c->copy_pool->wait();
    if (trace) fprintf(stderr, "crf_compute: copier pool started by %.0f us, preparation launched by %.0f us, launches issued by %.0f us, "
                               "copied out by %.0f us (%d ranges, %d copier threads)\n", t_pool, t_prep, t_issued, since(), ranges, threads);
    return CRF_OK;
}

}  // namespace crf

extern "C" {

// ---- field evaluation -------------------------------------------------------------------------------------------------
int crf_compute_device(crf_context* c, const crf_params* p, const void* device_reference_values, void* device_out,
                       void* stream) {
    if (p && p->prepared_slot != 0) {
        if (p->prepared_slot < 0 || p->prepared_slot > CRF_PREPARED_SLOTS)
            return fail(c, CRF_ERR_ARGUMENT, fmt("prepared_slot %d outside [0,%d]", p->prepared_slot, CRF_PREPARED_SLOTS));
        if (c && !c->prep_slots) return fail(c, CRF_ERR_STATE, "prepared_slot given but crf_prepare_device was never called");
        if (int r = compute_impl(c, p, nullptr, device_out, stream, 2u, p->prepared_slot - 1)) return r;
    } else {
        if (int r = compute_impl(c, p, device_reference_values, device_out, stream, 3u, -1)) return r;
    }
    return apply_abs(c, p, device_out, stream);
}

int crf_prepare_device(crf_context* c, const crf_params* p, const void* device_reference_values, int slot, void* stream) {
    return crf::prepare_device_ex(c, p, device_reference_values, slot, stream, nullptr);
}

int crf_prepare_rows_device(crf_context* c, const crf_params* p, const void* device_rows, int first_slot, int count,
                            void* stream) {
    if (!c || !p || !device_rows) return fail(c, CRF_ERR_ARGUMENT, "null argument");
    if (int r = check_slots(c, first_slot, count)) return r;
    crf_params local = *p;
    local.reference_values = nullptr;
    local.prepared_slot = 0;
    const float* rows = static_cast<const float*>(device_rows);
    for (int i = 0; i < count; i++)
        if (int r = crf_prepare_device(c, &local, rows + size_t(i) * size_t(c->cs), first_slot + i, stream)) return r;
    return CRF_OK;
}

int crf_compute_prepared_device(crf_context* c, const crf_params* p, int first_slot, int count, void* const* device_outs,
                                void* stream) {
    if (!c || !p || !device_outs) return fail(c, CRF_ERR_ARGUMENT, "null argument");
    if (int r = check_slots(c, first_slot, count)) return r;
    crf_params local = *p;
    for (int i = 0; i < count; i++) {
        local.prepared_slot = first_slot + i + 1;
        if (int r = crf_compute_device(c, &local, nullptr, device_outs[i], stream)) return r;
    }
    return CRF_OK;
}

int crf_compute(crf_context* c, const crf_params* p, float* host_out) {
    return crf::compute_to_host(c, p, nullptr, host_out, nullptr);
}

// ---- pair requests ----------------------------------------------------------------------------------------------------
int crf_compute_requests_device(crf_context* c, const crf_params* p, const void* device_requests, size_t num_requests,
                                void* device_out, void* stream) {
    if (int r = check_ready(c)) return r;
    if (int r = check_params(c, p, crf::kMaxGenericMembers, "pair requests support")) return r;
    if (num_requests && (!device_requests || !device_out)) return fail(c, CRF_ERR_ARGUMENT, "null argument");
    if (c->windowed)
        return fail(c, CRF_ERR_UNSUPPORTED, "pair requests address voxels with 32-bit byte offsets: member volumes of 4 GiB or more are not supported in request mode");
    if (int r = bind_device(c)) return r;
    hipStream_t s = stream_of(c, stream);
    if (int r = ensure_wide(c, s)) return r;
    crf::TwoVectorJob job = two_vector_job(c, p);
    // two-field request mode: the j side reads the secondary members (CRF_FLAG_QUERY_FROM_SECONDARY)
    if (p->flags & CRF_FLAG_QUERY_FROM_SECONDARY) {
        if (!c->grid.has_secondary())
            return fail(c, CRF_ERR_STATE, "CRF_FLAG_QUERY_FROM_SECONDARY needs secondary members (crf_upload_secondary_members)");
        if (int r = ensure_secondary_wide(c, s)) return r;
        job.members_y = c->view.secondary;
    }
    job.requests = static_cast<const uint32_t*>(device_requests);
    job.num_items = num_requests;
    job.use_abs = (p->flags & CRF_FLAG_ABSOLUTE_VALUE) ? 1 : 0;
    job.out = static_cast<float*>(device_out);
    // CRF_REQUESTS_GENERIC=1 (tuning / tests): the counting kernel for every measure.  A null list (legal only with no
    // requests) launches nothing and reports that kernel too.
    const bool force_counting = env_is_one("CRF_REQUESTS_GENERIC") || !job.requests;
    const char* kernel = "";
    hipError_t e;
    if (int r = run_two_vector(c, job, force_counting, s, &kernel, &e)) return r;
    c->last_kernel = kernel;
    return launch_status(c, e);
}

int crf_compute_requests(crf_context* c, const crf_params* p, const crf_request* host_requests, size_t num_requests,
                         float* host_out) {
    if (int r = check_ready(c)) return r;
    if (num_requests == 0) return CRF_OK;
    if (!host_requests || !host_out) return fail(c, CRF_ERR_ARGUMENT, "null argument");
    for (size_t r = 0; r < num_requests; r++) {
        const crf_request& q = host_requests[r];
        if (q.xi >= uint32_t(c->xs) || q.yi >= uint32_t(c->ys) || q.zi >= uint32_t(c->zs) || q.xj >= uint32_t(c->xs) ||
            q.yj >= uint32_t(c->ys) || q.zj >= uint32_t(c->zs))
            return fail(c, CRF_ERR_ARGUMENT, fmt("request %zu addresses a voxel outside the grid", r));
    }
    if (int r = bind_device(c)) return r;
    CRF_HIP(c, c->requests.reserve(num_requests));
    CRF_HIP(c, c->request_out.reserve(num_requests));
    CRF_HIP(c, hipMemcpyAsync(c->requests.get(), host_requests, num_requests * sizeof(crf_request), hipMemcpyHostToDevice,
                              c->stream));
    if (int r = crf_compute_requests_device(c, p, c->requests.get(), num_requests, c->request_out.get(), nullptr)) return r;
    CRF_HIP(c, hipMemcpyAsync(host_out, c->request_out.get(), num_requests * sizeof(float), hipMemcpyDeviceToHost,
                              c->stream));
    CRF_HIP(c, hipStreamSynchronize(c->stream));
    return CRF_OK;
}

// ---- ensemble statistics ----------------------------------------------------------------------------------------------
int crf_compute_ensemble_stat_device(crf_context* c, int stat, void* device_out, void* stream) {
    if (int r = check_ready(c)) return r;
    if (!device_out) return fail(c, CRF_ERR_ARGUMENT, "null output");
    if (stat != CRF_ENSEMBLE_MEAN && stat != CRF_ENSEMBLE_SPREAD)
        return fail(c, CRF_ERR_ARGUMENT, fmt("unknown ensemble statistic %d", stat));
    const bool native = native_reduction(c);
    return run_windowed(c, device_out, stream, native, [&](float* o, hipStream_t s, TimedLaunch& t) {
        if (native)
            return crf::launch_ensemble_stat_narrow(stat, c->view.narrow, c->grid.format, c->cs, c->view.num_voxels, o, s, t.e0,
                                                    t.e1, &t.info);
        return crf::launch_ensemble_stat(stat, c->view.members, c->cs, c->view.num_voxels, o, s, t.e0, t.e1, &t.info);
    });
}

int crf_compute_ensemble_stat(crf_context* c, int stat, float* host_out) {
    return to_host(c, host_out, [&](void* d) { return crf_compute_ensemble_stat_device(c, stat, d, nullptr); });
}

int crf_compute_set_predicate_device(crf_context* c, int op, float comparison_value, int count_lower, int count_upper,
                                     void* device_out, void* stream) {
    if (int r = check_ready(c)) return r;
    if (!device_out) return fail(c, CRF_ERR_ARGUMENT, "null output");
    if (op < CRF_CMP_GREATER || op > CRF_CMP_NOT_EQUAL)
        return fail(c, CRF_ERR_ARGUMENT, fmt("unknown comparison operator %d", op));
    const bool native = native_reduction(c);
    return run_windowed(c, device_out, stream, native, [&](float* o, hipStream_t s, TimedLaunch& t) {
        if (native)
            return crf::launch_set_predicate_narrow(c->view.narrow, c->grid.format, c->cs, c->view.num_voxels, op, comparison_value,
                                                    count_lower, count_upper, o, s, t.e0, t.e1, &t.info);
        return crf::launch_set_predicate(c->view.members, c->cs, c->view.num_voxels, op, comparison_value, count_lower,
                                         count_upper, o, s, t.e0, t.e1, &t.info);
    });
}

int crf_compute_set_predicate(crf_context* c, int op, float comparison_value, int count_lower, int count_upper,
                              float* host_out) {
    return to_host(c, host_out, [&](void* d) {
        return crf_compute_set_predicate_device(c, op, comparison_value, count_lower, count_upper, d, nullptr);
    });
}

int crf_compute_dkl_device(crf_context* c, int estimator, int num_bins, int k, void* device_out, void* stream) {
    if (int r = check_ready(c)) return r;
    if (!device_out) return fail(c, CRF_ERR_ARGUMENT, "null output");
    if (estimator != CRF_DKL_BINNED && estimator != CRF_DKL_ENTROPY_KNN)
        return fail(c, CRF_ERR_ARGUMENT, fmt("unknown DKL estimator %d", estimator));
    if (c->cs > crf::kMaxGenericMembers)
        return fail(c, CRF_ERR_UNSUPPORTED, fmt("DKL supports at most %d members", crf::kMaxGenericMembers));
    if (estimator == CRF_DKL_BINNED && (num_bins < 1 || num_bins > 1024))
        return fail(c, CRF_ERR_ARGUMENT, fmt("num_bins %d outside [1,1024]", num_bins));
    if (estimator == CRF_DKL_ENTROPY_KNN && c->cs > 1 && (k < 1 || k >= c->cs))
        return fail(c, CRF_ERR_ARGUMENT, fmt("k=%d must be in [1, cs-1=%d]", k, c->cs - 1));
    if (int r = bind_device(c)) return r;
    if (int r = ensure_workspace(c, crf::dkl_workspace_bytes(c->cs, estimator, num_bins, std::min(c->view.num_voxels, c->window_voxels)))) return r;
    // psi(n) = -gamma + H_{n-1} (boost::math::digamma at positive integers, DKL.cpp:156)
    const double knn_const =
        estimator == CRF_DKL_ENTROPY_KNN && c->cs > 1 ? psi_int(c->cs) - psi_int(k) + std::log(2.0) : 0.0;
    const bool native = native_dkl(c, estimator, k);
    return run_windowed(c, device_out, stream, native, [&](float* o, hipStream_t s, TimedLaunch& t) {
        if (native)
            return crf::launch_dkl_narrow(c->view.narrow, c->grid.format, c->cs, c->view.num_voxels, estimator, num_bins, k, knn_const,
                                          c->grid.scratch[0].workspace.get(), o, s, t.e0, t.e1, &t.info);
        return crf::launch_dkl(c->view.members, c->cs, c->view.num_voxels, estimator, num_bins, k, knn_const, c->grid.scratch[0].workspace.get(), o,
                               s, t.e0, t.e1, &t.info);
    });
}

int crf_compute_dkl(crf_context* c, int estimator, int num_bins, int k, float* host_out) {
    return to_host(c, host_out, [&](void* d) { return crf_compute_dkl_device(c, estimator, num_bins, k, d, nullptr); });
}

// ---- whole-field similarity of the primary and the secondary field -----------------------------------------------------
// computeFieldSimilarity<double> (Similarity.cpp:36-180) on two resident fields: Pearson in two streaming passes on the
// device, the binned measures as a joint histogram on the device and the reference's own arithmetic from the integer
// counts on the host (crf_similarity_tail.h).  Narrow members are read through their fp32 copies.
int crf_field_similarity(crf_context* c, int measure, int member, int num_bins, float min_x, float max_x, float min_y,
                         float max_y, float* out_value, unsigned long long* out_samples) {
    if (int r = check_ready(c)) return r;
    if (!out_value) return fail(c, CRF_ERR_ARGUMENT, "null output");
    if (!c->grid.has_secondary())
        return fail(c, CRF_ERR_STATE, "crf_field_similarity needs secondary members (crf_upload_secondary_members)");
    if (measure < CRF_PEARSON || measure > CRF_KMI_CC) return fail(c, CRF_ERR_ARGUMENT, fmt("unknown measure %d", measure));
    const bool binned = measure == CRF_MI_BINNED || measure == CRF_BINNED_MI_CC;
    if (measure != CRF_PEARSON && !binned)
        return fail(c, CRF_ERR_UNSUPPORTED,
                    fmt("crf_field_similarity: measure %d needs a global sort (Spearman, Kendall) or a k-nearest-neighbour search "
                        "(Kraskov MI) over all samples of the two fields, which is not implemented; Pearson and binned MI are",
                        measure));
    if (member < -1 || member >= c->cs)
        return fail(c, CRF_ERR_ARGUMENT, fmt("member %d outside [-1, %d)", member, c->cs));
    if (binned && (num_bins < 1 || num_bins > crf::kSimilarityMaxBins))
        return fail(c, CRF_ERR_ARGUMENT, fmt("num_bins %d outside [1,%d]", num_bins, crf::kSimilarityMaxBins));
    if (c->windowed)
        return fail(c, CRF_ERR_UNSUPPORTED, "crf_field_similarity does not evaluate windowed grids (member volumes of 4 GiB or more)");
    const int members = member < 0 ? c->cs : 1;
    if (size_t(members) * c->alloc_voxels > size_t(0x7FFFFFFF))
        return fail(c, CRF_ERR_UNSUPPORTED, fmt("%zu samples: the reference counts the samples of a field similarity in an int "
                                                "(at most 2147483647)", size_t(members) * c->alloc_voxels));
    if (int r = bind_device(c)) return r;
    hipStream_t s = c->stream;
    if (int r = ensure_wide(c, s)) return r;
    if (int r = ensure_secondary_wide(c, s)) return r;
    if (int r = ensure_workspace(c, crf::similarity_workspace_bytes())) return r;
    const crf_grid_state& g = c->grid;
    const int first = member < 0 ? 0 : member;
    crf::SimilarityJob job{c->view.members + first, c->view.secondary + first, members, c->alloc_voxels,
                           g.members.vpt == 4 && g.secondary.vpt == 4, g.scratch[0].workspace.get()};
    TimedLaunch launch(c);
    float value = 0.0f;
    unsigned long long samples = 0;
    if (!binned) {
        if (int r = launch.finish(crf::launch_similarity_moments(job, s, launch.e0, launch.e1, &launch.info))) return r;
        double stats[7];
        CRF_HIP(c, hipMemcpyAsync(stats, crf::similarity_stats(job.workspace), sizeof stats, hipMemcpyDeviceToHost, s));
        CRF_HIP(c, hipStreamSynchronize(s));
        samples = (unsigned long long)stats[0];
        value = float(stats[6]);
    } else {
        if (int r = launch.finish(crf::launch_similarity_histogram(job, num_bins, min_x, max_x, min_y, max_y, s, launch.e0,
                                                                   launch.e1, &launch.info)))
            return r;
        std::vector<uint64_t> counts(size_t(num_bins) * size_t(num_bins));
        CRF_HIP(c, hipMemcpyAsync(counts.data(), crf::similarity_histogram(job.workspace), counts.size() * sizeof(uint64_t),
                                  hipMemcpyDeviceToHost, s));
        CRF_HIP(c, hipMemcpyAsync(&samples, crf::similarity_samples(job.workspace), sizeof samples, hipMemcpyDeviceToHost, s));
        CRF_HIP(c, hipStreamSynchronize(s));
        value = crf::similarity_mi_from_counts(counts.data(), num_bins, samples);
        if (measure == CRF_BINNED_MI_CC) value = crf::similarity_mi_to_cc(value);
    }
    *out_value = value;
    if (out_samples) *out_samples = samples;
    return CRF_OK;
}

// ---- ranks over all samples: the device-wide sort ---------------------------------------------------------------------------
size_t crf_rank_scratch_bytes(const crf_context* c) { return c ? c->grid.rank_scratch.count() : 0; }

int crf_rank_values_device(crf_context* c, const void* device_values, size_t count, void* device_ranks,
                           unsigned long long* out_ranked) {
    if (!c) return CRF_ERR_ARGUMENT;
    if (out_ranked) *out_ranked = 0;
    if (count == 0) return CRF_OK;
    if (!device_values || !device_ranks) return fail(c, CRF_ERR_ARGUMENT, "null argument");
    if (count > size_t(0x7FFFFFFF))
        return fail(c, CRF_ERR_UNSUPPORTED, fmt("%zu values: the sort carries 32-bit payloads (at most 2147483647)", count));
    const char* in = static_cast<const char*>(device_values);
    const char* out = static_cast<const char*>(device_ranks);
    if (in < out + count * sizeof(float) && out < in + count * sizeof(float))
        return fail(c, CRF_ERR_ARGUMENT, "crf_rank_values_device: the ranks overlap the values");
    if (int r = bind_device(c)) return r;
    if (int r = ensure_rank_scratch(c, crf::rank_sort_scratch_bytes(count))) return r;
    TimedLaunch launch(c);
    if (int r = launch.finish(crf::launch_rank_values(static_cast<const float*>(device_values), count,
                                                      static_cast<float*>(device_ranks), c->grid.rank_scratch.get(),
                                                      c->stream, launch.e0, launch.e1, out_ranked, &launch.info)))
        return r;
    CRF_HIP(c, hipStreamSynchronize(c->stream));
    return CRF_OK;
}

// computeFieldSimilarity<double> with a rank measure (Similarity.cpp:134-143) on two resident fields.  An entry point of
// its own: crf_field_similarity keeps refusing the rank measures.
int crf_field_rank_similarity(crf_context* c, int measure, int member, float* out_value, unsigned long long* out_samples) {
    if (int r = check_ready(c)) return r;
    if (!out_value) return fail(c, CRF_ERR_ARGUMENT, "null output");
    if (!c->grid.has_secondary())
        return fail(c, CRF_ERR_STATE, "crf_field_rank_similarity needs secondary members (crf_upload_secondary_members)");
    if (measure == CRF_KENDALL)
        return fail(c, CRF_ERR_UNSUPPORTED, "crf_field_rank_similarity: Kendall needs an inversion count over all samples on top of "
                                            "the sort, which is not implemented; Spearman is");
    if (measure != CRF_SPEARMAN)
        return fail(c, CRF_ERR_ARGUMENT, fmt("crf_field_rank_similarity: measure %d is not a rank measure (crf_field_similarity "
                                             "serves Pearson and binned MI)", measure));
    if (member < -1 || member >= c->cs)
        return fail(c, CRF_ERR_ARGUMENT, fmt("member %d outside [-1, %d)", member, c->cs));
    if (c->windowed)
        return fail(c, CRF_ERR_UNSUPPORTED, "crf_field_rank_similarity does not evaluate windowed grids (member volumes of 4 GiB or more)");
    const int members = member < 0 ? c->cs : 1;
    if (size_t(members) * c->alloc_voxels > size_t(0x7FFFFFFF))
        return fail(c, CRF_ERR_UNSUPPORTED, fmt("%zu samples: the reference counts the samples of a field similarity in an int "
                                                "(at most 2147483647)", size_t(members) * c->alloc_voxels));
    if (int r = bind_device(c)) return r;
    hipStream_t s = c->stream;
    if (int r = ensure_wide(c, s)) return r;
    if (int r = ensure_secondary_wide(c, s)) return r;
    if (int r = ensure_workspace(c, crf::similarity_workspace_bytes())) return r;
    if (int r = ensure_rank_scratch(c, crf::rank_similarity_scratch_bytes(members, c->alloc_voxels))) return r;
    const crf_grid_state& g = c->grid;
    const int first = member < 0 ? 0 : member;
    crf::SimilarityJob job{c->view.members + first, c->view.secondary + first, members, c->alloc_voxels,
                           g.members.vpt == 4 && g.secondary.vpt == 4, g.scratch[0].workspace.get()};
    TimedLaunch launch(c);
    if (int r = launch.finish(crf::launch_rank_similarity(job, g.rank_scratch.get(), s, launch.e0, launch.e1, &launch.info)))
        return r;
    double stats[7];
    CRF_HIP(c, hipMemcpyAsync(stats, crf::similarity_stats(job.workspace), sizeof stats, hipMemcpyDeviceToHost, s));
    CRF_HIP(c, hipStreamSynchronize(s));
    *out_value = float(stats[6]);
    if (out_samples) *out_samples = (unsigned long long)stats[0];
    return CRF_OK;
}

// ---- Kendall's tau-b over all samples: two sorts and an inversion count ------------------------------------------------------
namespace {
// the tail shared by the two entry points: the launcher's integers to the value and the caller's outputs
void kendall_outputs(unsigned long long kept, const long long device_counts[3], float* out_value, long long* out_counts,
                     unsigned long long* out_kept) {
    *out_value = crf::similarity_kendall_from_counts(int64_t(kept), device_counts[0], device_counts[1], device_counts[2], out_counts);
    if (out_kept) *out_kept = kept;
}
}  // namespace

int crf_kendall_values_device(crf_context* c, const void* device_x, const void* device_y, size_t count, float* out_value,
                              long long* out_counts, unsigned long long* out_kept) {
    if (!c) return CRF_ERR_ARGUMENT;
    if (!out_value) return fail(c, CRF_ERR_ARGUMENT, "null output");
    const long long none[3] = {0, 0, 0};
    if (count == 0) {
        kendall_outputs(0, none, out_value, out_counts, out_kept);  // 0 / 0
        return CRF_OK;
    }
    if (!device_x || !device_y) return fail(c, CRF_ERR_ARGUMENT, "null argument");
    if (count > size_t(0x7FFFFFFF))
        return fail(c, CRF_ERR_UNSUPPORTED, fmt("%zu values: the sort carries 32-bit payloads (at most 2147483647)", count));
    if (int r = bind_device(c)) return r;
    if (int r = ensure_rank_scratch(c, crf::kendall_scratch_bytes(count))) return r;
    TimedLaunch launch(c);
    unsigned long long kept = 0;
    long long counts[3] = {0, 0, 0};
    if (int r = launch.finish(crf::launch_kendall_values(static_cast<const float*>(device_x), static_cast<const float*>(device_y),
                                                         count, c->grid.rank_scratch.get(), c->stream, launch.e0, launch.e1,
                                                         &kept, counts, &launch.info)))
        return r;
    kendall_outputs(kept, counts, out_value, out_counts, out_kept);
    return CRF_OK;
}

// computeFieldSimilarity<double> with CRF_KENDALL (Similarity.cpp:134-143) on two resident fields.  An entry point of its
// own: crf_field_similarity and crf_field_rank_similarity keep refusing Kendall.
int crf_field_kendall_similarity(crf_context* c, int member, float* out_value, long long* out_counts,
                                 unsigned long long* out_samples) {
    if (int r = check_ready(c)) return r;
    if (!out_value) return fail(c, CRF_ERR_ARGUMENT, "null output");
    if (!c->grid.has_secondary())
        return fail(c, CRF_ERR_STATE, "crf_field_kendall_similarity needs secondary members (crf_upload_secondary_members)");
    if (member < -1 || member >= c->cs)
        return fail(c, CRF_ERR_ARGUMENT, fmt("member %d outside [-1, %d)", member, c->cs));
    if (c->windowed)
        return fail(c, CRF_ERR_UNSUPPORTED, "crf_field_kendall_similarity does not evaluate windowed grids (member volumes of 4 GiB or more)");
    const int members = member < 0 ? c->cs : 1;
    if (size_t(members) * c->alloc_voxels > size_t(0x7FFFFFFF))
        return fail(c, CRF_ERR_UNSUPPORTED, fmt("%zu samples: the reference counts the samples of a field similarity in an int "
                                                "(at most 2147483647)", size_t(members) * c->alloc_voxels));
    if (int r = bind_device(c)) return r;
    hipStream_t s = c->stream;
    if (int r = ensure_wide(c, s)) return r;
    if (int r = ensure_secondary_wide(c, s)) return r;
    if (int r = ensure_rank_scratch(c, crf::kendall_scratch_bytes(size_t(members) * c->alloc_voxels))) return r;
    const crf_grid_state& g = c->grid;
    const int first = member < 0 ? 0 : member;
    crf::SimilarityJob job{c->view.members + first, c->view.secondary + first, members, c->alloc_voxels,
                           g.members.vpt == 4 && g.secondary.vpt == 4, nullptr};
    TimedLaunch launch(c);
    unsigned long long kept = 0;
    long long counts[3] = {0, 0, 0};
    if (int r = launch.finish(crf::launch_kendall_similarity(job, g.rank_scratch.get(), s, launch.e0, launch.e1, &kept, counts,
                                                             &launch.info)))
        return r;
    kendall_outputs(kept, counts, out_value, out_counts, out_samples);
    return CRF_OK;
}

// ---- helpers, instrumentation, synthetic data -------------------------------------------------------------------------
double crf_max_mutual_information_kraskov(int k, int cs) {
    if (k < 1 || cs < 1) return std::numeric_limits<double>::quiet_NaN();
    return psi_int(cs) - psi_int(k);
}

size_t crf_tiled_element_count(int xs, int ys, int zs) {
    if (xs <= 0 || ys <= 0 || zs <= 0) return 0;
    return size_t((xs + 7) / 8) * size_t((ys + 7) / 8) * size_t((zs + 3) / 4) * 256;
}

int crf_tile_field_device(crf_context* c, const void* device_linear, void* device_tiled, void* stream) {
    if (!c) return CRF_ERR_ARGUMENT;
    if (c->cs <= 0) return fail(c, CRF_ERR_STATE, "crf_set_grid has not been called");
    if (c->windowed) return fail(c, CRF_ERR_UNSUPPORTED, "re-tiling a field of 4 GiB or more is not supported");
    if (!device_linear || !device_tiled) return fail(c, CRF_ERR_ARGUMENT, "null argument");
    if (int r = bind_device(c)) return r;
    hipStream_t s = stream_of(c, stream);
    hipError_t e = crf::launch_tile_field(static_cast<const float*>(device_linear), static_cast<float*>(device_tiled),
                                          c->xs, c->ys, c->zs, s);
    return launch_status(c, e);
}

int crf_set_profiling(crf_context* c, int enabled) {
    if (!c) return CRF_ERR_ARGUMENT;
    c->profiling = enabled != 0;
    return CRF_OK;
}

int crf_take_kernel_time(crf_context* c, double* out_ms_sum, int* out_launches) {
    if (!c || !out_ms_sum || !out_launches) return fail(c, CRF_ERR_ARGUMENT, "null argument");
    if (int r = bind_device(c)) return r;
    double sum = 0.0;
    int n = 0;
    for (auto& p : c->ev_pending) {
        CRF_HIP(c, hipEventSynchronize(p.second));
        float ms = 0.f;
        CRF_HIP(c, hipEventElapsedTime(&ms, p.first, p.second));
        sum += double(ms);
        n++;
        c->ev_free.push_back(std::move(p.first));
        c->ev_free.push_back(std::move(p.second));
    }
    c->ev_pending.clear();
    *out_ms_sum = sum;
    *out_launches = n;
    return CRF_OK;
}

const char* crf_last_kernel_name(const crf_context* c) { return c ? c->last_kernel.c_str() : ""; }

int crf_set_member_layout(crf_context* c, int mode) {
    if (!c) return CRF_ERR_ARGUMENT;
    if (mode != CRF_MEMBER_LAYOUT_AUTO && mode != CRF_MEMBER_LAYOUT_RAW && mode != CRF_MEMBER_LAYOUT_PACKED)
        return fail(c, CRF_ERR_ARGUMENT, fmt("unknown member layout %d", mode));
    if (mode == c->member_layout) return CRF_OK;
    if (int r = bind_device(c)) return r;
    CRF_HIP(c, hipDeviceSynchronize());  // evaluations in flight may still read the packed copy
    drop_packed(c);
    c->member_layout = mode;
    return CRF_OK;
}

int crf_last_member_layout(const crf_context* c) { return c ? c->last_layout : CRF_MEMBER_LAYOUT_RAW; }

int crf_members_changed(crf_context* c) {
    if (!c) return CRF_ERR_ARGUMENT;
    if (int r = bind_device(c)) return r;
    CRF_HIP(c, hipDeviceSynchronize());  // evaluations in flight may still read what is dropped
    primary_members_changed(c);
    secondary_members_changed(c);
    return CRF_OK;
}

int crf_synth_box_member(crf_context* c, void* device_out, int xs, int ys, int zs_local, int z_begin, int zs_global,
                         int member, int cs, uint64_t seed, void* stream) {
    if (!c || !device_out) return fail(c, CRF_ERR_ARGUMENT, "null argument");
    if (xs <= 0 || ys <= 0 || zs_local <= 0 || zs_global <= 0 || z_begin < 0 || member < 0 || member >= cs)
        return fail(c, CRF_ERR_ARGUMENT, "invalid synthetic volume description");
    if (int r = bind_device(c)) return r;
    hipStream_t s = stream_of(c, stream);
    CRF_HIP(c, crf::launch_synth_box_member(static_cast<float*>(device_out), xs, ys, zs_local, z_begin, zs_global,
                                            member, cs, seed, s));
    return CRF_OK;
}

}  // extern "C"
