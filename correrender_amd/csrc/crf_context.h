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
#include "crf_internal.h"
#include "crf_pool.h"

constexpr int kMaxHostChunks = 16;  // z-chunks of a host-output evaluation (kernel of chunk i+1 under the D2H of chunk i)

// Scratch that the per-voxel kernels WRITE.  Launches that share a set must be ordered on one stream.
struct crf_scratch {
    uint32_t* todo = nullptr;  // deferred-voxel list of the split-sort rank kernels: a counter, then todo_voxels indices
    size_t todo_voxels = 0;
    unsigned char* workspace = nullptr;  // blockIdx-indexed voxel tiles / rank columns of the generic (cs > 128) kernels
    size_t workspace_bytes = 0;
};

struct crf_context {
    int device = -1;
    hipStream_t stream = nullptr;  // the context's own stream (used when the caller passes none)
    std::string err;
    int xs = 0, ys = 0, zs = 0, cs = 0;
    size_t num_voxels = 0;
    // members
    void* owned_block = nullptr;  // one allocation holding every uploaded member (stride owned_stride floats)
    size_t owned_stride = 0;
    std::vector<const float*> members;  // cs device pointers (owned or borrowed)
    const float** d_member_table = nullptr;
    int max_vpt = 1;
    // primary members in a narrow native format (crf_upload_members_format / crf_bind_members_device_format): `narrow`
    // holds the cs device pointers and `members` stays empty until a call that needs fp32 members builds the widened
    // copy (api.cpp: ensure_wide), one owned block; the Pearson, the Kendall and (where routed: api.cpp native_binned) the binned-MI field at 2..128 members, the sibling
    // reductions, the extrema and the reference gathers read `narrow` directly
    int format = CRF_MEMBER_F32;
    void* narrow_owned_block = nullptr;
    std::vector<const void*> narrow;
    const void** d_narrow_table = nullptr;
    bool narrow_aligned = false;       // every narrow pointer is 4-byte aligned (the native Pearson kernel loads dwords)
    bool narrow_element_aligned = false;  // ... aligned to its element (the native Kendall and binned-MI kernels load elements)
    void* wide_block = nullptr;        // the widened copy, lazily
    int last_format = CRF_MEMBER_F32;  // what the per-voxel kernel of the last field evaluation read
    // secondary members (second scalar field of the SEPARATE / SEPARATE_SYMMETRIC modes), optional
    void* sec_owned_block = nullptr;
    std::vector<const float*> sec_members;
    const float** d_sec_table = nullptr;
    bool sec_minmax_valid = false;
    float sec_min_v = 0.f, sec_max_v = 0.f;
    // scratch
    float* d_ref = nullptr;    // cs reference values
    float* d_prep = nullptr;   // crf::kPrepBytes
    float* d_prep_slots = nullptr;  // CRF_PREPARED_SLOTS x crf::kPrepBytes, lazily (crf_prepare_device)
    float* d_out = nullptr;    // num_voxels floats, lazily (crf_compute only)
    double* d_tables = nullptr;  // psi / p ln p / noise tables for this member count (crf_internal.h)
    // [0]: every launch on the context's stream or a caller's; [1]: the ranges of a host-output evaluation that run on
    // stream2.  Lazily; sized before the first launch of an evaluation, never between its ranges (api.cpp: ensure_todo).
    crf_scratch scratch[2];
    int scratch_set = 0;         // the set the launch being issued uses (api.cpp: NarrowScope::select_range)
    int pipeline_sets = 1;       // while crf_compute runs its range pipeline: the streams it uses, and the voxels of
    size_t pipeline_voxels = 0;  //   its largest range (0: no pipeline, scratch is sized for num_voxels)
    uint32_t* d_requests = nullptr;  // staging of host pair requests / their results, lazily
    float* d_request_out = nullptr;
    size_t request_capacity = 0;
    uint32_t* d_minmax = nullptr;
    bool minmax_valid = false;
    // packed copy of the members for the Pearson field (crf_internal.h), built lazily at the first Pearson field
    // evaluation after the members change (api.cpp: ensure_packed)
    int member_layout = CRF_MEMBER_LAYOUT_AUTO;  // crf_set_member_layout
    int pack_state = 0;                          // 0: not decided for the current members, 1: packed, -1: declined
    unsigned char* d_packed = nullptr;           // header, then body (one allocation)
    size_t packed_bytes = 0;
    uint32_t* d_pack_fallbacks = nullptr;
    int last_layout = CRF_MEMBER_LAYOUT_RAW;     // of the last Pearson field evaluation
    float min_v = 0.f, max_v = 0.f;
    // profiling
    bool profiling = false;
    std::vector<hipEvent_t> ev_free;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending;
    std::string last_kernel;
    // host-output evaluations (crf_compute): the grid in up to kMaxHostChunks voxel ranges, one member-pointer table per
    // range; the per-voxel kernel of a range stores into the pinned, device-mapped staging buffer and a pool of host
    // threads moves finished ranges into the caller's buffer (api.cpp: compute_to_host)
    const float** d_chunk_tables = nullptr;  // host_chunks x cs pointers
    int host_chunks = 0;                     // 0: tables not built for the current members
    bool chunk_native = false;               // the tables hold the narrow pointers (native Pearson field), not fp32 ones
    size_t chunk_first[kMaxHostChunks + 1] = {};  // first voxel of every range; [host_chunks] = alloc_voxels
    std::atomic<int> chunk_ready[kMaxHostChunks] = {};  // 1: range landed in the staging buffer, -1: evaluation failed
    hipStream_t stream2 = nullptr;           // odd ranges (the next range fills the GPU while the previous one drains)
    hipStream_t copy_stream = nullptr;       // DMA form only (CRF_HOST_PATH=dma, CRF_FLAG_ABSOLUTE_VALUE)
    hipEvent_t prep_done = nullptr;
    hipEvent_t chunk_done[kMaxHostChunks] = {};    // range evaluated
    hipEvent_t chunk_copied[kMaxHostChunks] = {};  // DMA form: range landed in the staging buffer (copy stream)
    float* h_staging = nullptr;                    // pinned + mapped, alloc_voxels floats, lazily
    float* d_staging = nullptr;                    // its device address
    std::unique_ptr<crf::SpinPool> copy_pool;      // copier threads, lazily
    int copy_threads = 0;                          // how many of them a copy uses (calibrated at first use)
    int copy_threads_cap = 0;                      // > 0: upper bound set by the owner (a device group shares the host)
    // member volumes of 4 GiB or more: evaluated in windows (api.cpp: ensure_windows)
    bool windowed = false;
    const float** d_window_tables = nullptr;  // windows x (1 or 2) x cs pointers (primary [, secondary] members)
    int windows = 0;                          // 0: tables not built for the current members
    bool window_has_secondary = false;
    size_t alloc_voxels = 0;  // voxels of the whole local grid (num_voxels is narrowed while a chunk is being launched)
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
