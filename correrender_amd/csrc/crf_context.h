// crf_context.h -- the state behind a crf_context (include/corrfield.h), shared by api.cpp and group.cpp.
// Internal to libcorrfield.so.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/corrfield.h"
#include "crf_host_copy.h"  // kMaxHostChunks
#include "crf_internal.h"
#include "crf_owned.h"
#include "crf_pool.h"
#include "crf_windows.h"

// Scratch that the per-voxel kernels WRITE.  Launches that share a set must be ordered on one stream.
struct crf_scratch {
    crf::DeviceBuffer<uint32_t> todo;  // deferred-voxel list of the split-sort rank kernels: a counter, then the indices
    crf::DeviceBuffer<unsigned char> workspace;  // blockIdx-indexed voxel tiles / rank columns of the generic kernels
};

// cs member volumes on the device, in one element format.
struct crf_member_set {
    crf::DeviceBuffer<unsigned char> owned;  // uploaded members: one block, 256-byte aligned each; empty for bound ones
    std::vector<const void*> ptrs;           // cs device pointers (into `owned`, the wide copy or the caller's memory);
                                             //   empty: the set is not there
    crf::DeviceBuffer<const void*> table;    // the same cs pointers on the device
    int format = CRF_MEMBER_F32;
    bool minmax_valid = false;  // min_v / max_v hold the extrema of the current values
    float min_v = 0.f, max_v = 0.f;
    // what the set's consumers ask about the pointers (api.cpp: install_table)
    int vpt = 1;                   // fp32: the widest vector load every member allows (4, 2 or 1 floats)
    bool dword_aligned = false;    // narrow: every member is 4-byte aligned (the kernels that load dwords)
    bool element_aligned = false;  // narrow: ... aligned to its element (the kernels that load single elements)
    const float* f32(int m) const { return static_cast<const float*>(ptrs[size_t(m)]); }
    const float* const* f32_table() const { return reinterpret_cast<const float* const*>(table.get()); }
    void clear() {
        owned.reset();
        ptrs.clear();
        minmax_valid = false;
    }
};

// Everything whose size depends on the grid or the member count.  crf_set_grid replaces it with a fresh value; what is
// derived from the members is dropped in one place (api.cpp: primary_members_changed and its siblings).
struct crf_grid_state {
    // The primary members are in `members` (format == CRF_MEMBER_F32) or in `narrow` (crf_upload_members_format /
    // crf_bind_members_device_format with a narrow format).  With narrow members, `members` stays empty until an
    // evaluation that has no native route needs fp32 values: then it points into `wide`, the converted copy
    // (api.cpp: ensure_wide; native_field and native_reduction say which evaluations read `narrow` as it is).
    crf_member_set members, narrow;
    int format = CRF_MEMBER_F32;
    crf::DeviceBuffer<float> wide;
    // The second scalar field of the SEPARATE / SEPARATE_SYMMETRIC modes, optional, held like the primary one: fp32 members
    // in `secondary`, narrow ones in `secondary_narrow`, and then `secondary` empty until an evaluation without a native
    // route needs fp32 values and points it into `secondary_wide` (api.cpp: ensure_secondary_wide).
    crf_member_set secondary, secondary_narrow;
    int secondary_format = CRF_MEMBER_F32;
    crf::DeviceBuffer<float> secondary_wide;
    bool has_secondary() const { return !(secondary_format == CRF_MEMBER_F32 ? secondary : secondary_narrow).ptrs.empty(); }
    // packed copy of fp32 members for the Pearson field (crf_internal.h), built at the first Pearson field evaluation
    // after the members change (api.cpp: ensure_packed)
    crf::DeviceBuffer<unsigned char> packed;  // header, then body
    int pack_state = 0;                       // 0: not decided for the current members, 1: packed, -1: declined
    crf::DeviceBuffer<float> ref;      // cs reference values
    crf::DeviceBuffer<float> out;      // the whole grid, lazily (host-output calls only)
    crf::DeviceBuffer<double> tables;  // psi / p ln p / noise tables for this member count (crf_internal.h)
    // [0]: every launch on the context's stream or a caller's; [1]: the ranges of a host-output evaluation that run on
    // stream2.  Lazily; sized before the first launch of an evaluation, never between its ranges (api.cpp: ensure_todo).
    crf_scratch scratch[2];
    // the device-wide sort of crf_rank_values_device / crf_field_rank_similarity (kernels_rank_similarity.hip) and of the
    // two Kendall calls (kernels_kendall_similarity.hip): keys, payloads, tables and rank arrays, grown on demand (api.cpp:
    // ensure_rank_scratch).  Not part of `scratch`: it is sized by the sample count, tens of GiB for a large field, and
    // only these four calls use it.
    crf::DeviceBuffer<unsigned char> rank_scratch;
    // host-output evaluations (crf_compute): the grid in up to kMaxHostChunks voxel ranges, one member-pointer table per
    // range; the per-voxel kernel of a range stores into the pinned, device-mapped staging buffer and a pool of host
    // threads moves finished ranges into the caller's buffer (api.cpp: compute_to_host)
    crf::DeviceBuffer<const void*> chunk_tables;  // host_chunks x cs pointers
    int host_chunks = 0;                          // 0: tables not built for the current members
    bool chunk_native = false;                    // the tables point into `narrow` (a native field), not into `members`
    size_t chunk_first[kMaxHostChunks + 1] = {};  // first voxel of every range; [host_chunks] = alloc_voxels
    crf::PinnedBuffer staging;                    // alloc_voxels floats, lazily
    // member volumes of 4 GiB or more: evaluated in windows (api.cpp: ensure_windows)
    crf::DeviceBuffer<const float*> window_tables;  // windows x (1 or 2) x cs pointers (primary [, secondary] members)
    int windows = 0;                                // 0: tables not built for the current members
    bool window_has_secondary = false;
};

// What a launch reads: the whole local grid (api.cpp: whole_view), or one window / one voxel range of it while a
// NarrowScope is active.  Non-owning; the owners above are never repointed.
struct crf_launch_view {
    const float* const* members = nullptr;    // fp32 primary members
    const float* const* secondary = nullptr;  // null: no secondary members
    const void* const* narrow = nullptr;      // primary members in their narrow format
    size_t num_voxels = 0;
    int max_vpt = 1;
    int scratch_set = 0;  // the crf_scratch the launch being issued writes
    const void* const* secondary_narrow = nullptr;  // secondary members in their narrow format
};

// Members are destroyed in reverse order of declaration, and crf_destroy relies on it: `stream` comes first because it
// goes last (everything else was used on it), and `copy_pool` comes after `grid` because the copier threads are joined
// before the staging buffer they read goes.  The device is bound before a context is deleted or re-gridded.
struct crf_context {
    int device = -1;
    crf::Stream stream;  // the context's own stream (used when the caller passes none)
    std::string err;
    int xs = 0, ys = 0, zs = 0, cs = 0;
    size_t alloc_voxels = 0;  // voxels of the whole local grid
    bool windowed = false;    // member volumes of 4 GiB or more (or more voxels than CRF_WINDOW_VOXELS): crf_windows.h
    size_t window_voxels = crf::kDefaultWindowVoxels;  // voxels of a full window, captured by crf_set_grid for this grid
    crf_grid_state grid;
    crf_launch_view view;
    int last_format = CRF_MEMBER_F32;  // what the per-voxel kernel of the last field evaluation read
    int member_layout = CRF_MEMBER_LAYOUT_AUTO;  // crf_set_member_layout
    int last_layout = CRF_MEMBER_LAYOUT_RAW;     // of the last Pearson field evaluation
    // context-lifetime device memory
    crf::DeviceBuffer<float> prep;        // crf::kPrepBytes
    crf::DeviceBuffer<float> prep_slots;  // CRF_PREPARED_SLOTS x crf::kPrepBytes, lazily (crf_prepare_device)
    crf::DeviceBuffer<uint32_t> minmax;   // the two keys of the extrema kernels
    crf::DeviceBuffer<uint32_t> pack_fallbacks;
    crf::DeviceBuffer<crf_request> requests;  // staging of host pair requests / their results, lazily
    crf::DeviceBuffer<float> request_out;
    int pipeline_sets = 1;       // while crf_compute runs its range pipeline: the streams it uses, and the voxels of
    size_t pipeline_voxels = 0;  //   its largest range (0: no pipeline, scratch is sized for the view's voxels)
    // profiling
    bool profiling = false;
    std::vector<crf::Event> ev_free;
    std::vector<std::pair<crf::Event, crf::Event>> ev_pending;
    std::string last_kernel;
    // the range pipeline of crf_compute (the range tables themselves are grid state)
    std::atomic<int> chunk_ready[kMaxHostChunks] = {};  // 1: range landed in the staging buffer, -1: evaluation failed
    crf::Stream stream2;      // odd ranges (the next range fills the GPU while the previous one drains)
    crf::Stream copy_stream;  // DMA form only (CRF_HOST_PATH=dma, CRF_FLAG_ABSOLUTE_VALUE)
    crf::Event prep_done;
    crf::Event chunk_done[kMaxHostChunks];    // range evaluated
    crf::Event chunk_copied[kMaxHostChunks];  // DMA form: range landed in the staging buffer (copy stream)
    std::unique_ptr<crf::SpinPool> copy_pool;  // copier threads, lazily
    int copy_threads = 0;                      // how many of them a copy uses (calibrated at first use)
    int copy_threads_cap = 0;                  // > 0: upper bound set by the owner (a device group shares the host)
};


// api.cpp internals used by the device group (group.cpp)
namespace crf {
// waits for an event by polling hipEventQuery (a render thread blocked in calculateCpu has nothing else to do, and the
// runtime's sleeping wait costs tens of microseconds per wake-up); falls back to hipEventSynchronize after 50 ms
inline hipError_t spin_on_event(hipEvent_t e) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned i = 1;; i++) {
        const hipError_t q = hipEventQuery(e);
        if (q != hipErrorNotReady) return q;
        if ((i & 1023u) == 0u && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 0.05)
            return hipEventSynchronize(e);
        _mm_pause();
    }
}
// One evaluation straight into a caller-owned HOST buffer of the local grid: reference-side preparation once, then the
// per-voxel kernel range by range with the D2H copies overlapped.  device_reference_values: device pointer to cs floats
// or null (then params->reference_values / the reference point are used).
// ref_override (crf_group, direct exchange): the reference-side preparation reads its cs values from table[c][voxel], the
// member table of ANOTHER context (the slab that holds the reference point), instead of a vector or the local members.
struct RefOverride {
    const float* const* table = nullptr;
    size_t voxel = 0;
};
int compute_to_host(crf_context* c, const crf_params* p, const void* device_reference_values, float* host_out,
                    const RefOverride* ref_override);
// crf_compute_device / crf_prepare_device with a direct reference read (ref_override may be null: the plain calls)
int compute_device_ex(crf_context* c, const crf_params* p, const void* device_reference_values, void* device_out,
                      void* stream, const RefOverride* ref_override);
int prepare_device_ex(crf_context* c, const crf_params* p, const void* device_reference_values, int slot, void* stream,
                      const RefOverride* ref_override);
// the context's second stream (created on first use)
int second_stream(crf_context* c, hipStream_t* out);
// the override that makes other contexts read the reference values of local point (x, y, z) out of `owner`'s members
int reference_override(crf_context* owner, bool secondary, int x, int y, int z, RefOverride* out);
// referenceValues[c] = (secondary ? secondary members : members)[c][IDXS(x,y,z)] into a device buffer, stream-ordered
int gather_reference_to(crf_context* c, bool secondary, int x, int y, int z, float* device_out, hipStream_t s);
}  // namespace crf
