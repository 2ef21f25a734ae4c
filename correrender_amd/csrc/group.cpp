// group.cpp -- several GPUs behind ONE caller thread: the crf_group part of the C ABI (include/corrfield.h).
//
// The reference is one process whose calculators are invoked from the render thread with a caller-owned host buffer
// (src/Volume/VolumeData.cpp:1214-1226, 1469-1472).  A renderer that links libcorrfield can therefore not use the
// one-process-per-GPU driver (correrender_amd/distributed.py); this is the same z-slab decomposition inside the library:
//   * the global grid is cut into z-slabs, one per device (the split of distributed.py:slab_bounds -- with x-fastest
//     volumes a slab of every member is one contiguous range and the result slabs concatenate in the caller's buffer);
//   * every device is one GroupSlot: its own crf_context (members resident in ITS HBM, its own streams), the buffers and
//     events of the exchange, which the slot owns (crf_owned.h), and a persistent worker thread bound to the device, so
//     the launches of the N devices are issued concurrently, not one device after the other;
//   * per evaluation there is ONE exchange: the cs values of the reference point live in the slab of one device (the
//     owner).  Its form (Exchange) is decided once, in crf_group_create.  Direct, whenever every pair of devices has peer
//     access (the xGMI-connected MI355X of a node; trivially when an ordinal repeats -- the rehearsal of an N-slab group
//     on fewer GPUs): every device's reference-side preparation kernel reads the cs values straight out of the owner's
//     member volumes -- no collective, no copy, no event, no rendezvous between the workers.  Rccl
//     (CRF_GROUP_EXCHANGE=rccl, and the default without peer access): the owner gathers and ncclBroadcast distributes
//     (one persistent single-process communicator from ncclCommInitAll, one rank per worker thread; RCCL refuses two
//     ranks on one device).  Staged (CRF_GROUP_EXCHANGE=copy): the owner gathers, the others hipMemcpyPeerAsync;
//   * crf_group_compute_batch[_device] evaluates MANY reference points per hand-off: the reference vectors of up to 32
//     points travel in one collective (owners fill their rows, one ncclAllReduce(sum)) or are read directly, the
//     reference-side preparations of a block run first into prepared slots and its per-voxel kernels follow back to
//     back; the workers synchronise once per call;
//   * each device then runs the ranged evaluation of api.cpp (crf::compute_to_host) straight into its part of the
//     caller's buffer: the D2H copies of the N devices run concurrently over their own PCIe links.
// librccl is loaded on first use (dlopen): a single-device process never needs it.
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "crf_context.h"
#include "crf_pool.h"

namespace {

// ---- the few RCCL entry points the exchange needs (rccl.h: ncclCommInitAll :236, ncclBroadcast :591) -------------
using ncclComm_t = void*;
constexpr int kNcclFloat32 = 7;  // ncclFloat32, rccl.h:466
constexpr int kNcclSum = 0;      // ncclSum, rccl.h (ncclRedOp_t)
struct Rccl {
    void* handle = nullptr;
    int (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    int (*CommDestroy)(ncclComm_t) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;  // rccl.h: ncclAllReduce
    const char* (*GetErrorString)(int) = nullptr;
    std::string error;
    bool load() {
        if (handle) return true;
        const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names)
            if ((handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;  // the copy the process already has (e.g. torch's)
        if (!handle)
            for (const char* n : names)
                if ((handle = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
        if (!handle) {
            error = std::string("librccl not found: ") + (dlerror() ? dlerror() : "");
            return false;
        }
        CommInitAll = reinterpret_cast<decltype(CommInitAll)>(dlsym(handle, "ncclCommInitAll"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(handle, "ncclCommDestroy"));
        Broadcast = reinterpret_cast<decltype(Broadcast)>(dlsym(handle, "ncclBroadcast"));
        AllReduce = reinterpret_cast<decltype(AllReduce)>(dlsym(handle, "ncclAllReduce"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(handle, "ncclGetErrorString"));
        if (!CommInitAll || !CommDestroy || !Broadcast || !AllReduce) {
            error = "librccl lacks ncclCommInitAll / ncclCommDestroy / ncclBroadcast / ncclAllReduce";
            return false;
        }
        return true;
    }
    const char* describe(int status) const { return GetErrorString ? GetErrorString(status) : "?"; }
};

std::string fmt(const char* f, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

thread_local std::string g_group_create_error;

constexpr int kBatchRows = crf::kMaxGatherRows;  // reference vectors exchanged per collective of a batch

// How the reference vector of an evaluation reaches the devices that do not hold the reference point.
enum class Exchange {
    None,    // one device: global == local coordinates, the context does it all itself
    Direct,  // every preparation kernel reads the owner's members (crf::RefOverride)
    Rccl,    // ncclBroadcast of one vector, ncclAllReduce of a batch's rows
    Staged,  // the owner gathers, the others hipMemcpyPeerAsync
};

bool forced_onto(const char* forced, const char* form) { return forced && strcmp(forced, form) == 0; }

// `forced`: CRF_GROUP_EXCHANGE ("peer" | "copy" | "rccl") or null.  By default the direct read whenever every pair of
// devices has peer access (all MI355X of a node do, over xGMI; trivially true when an ordinal repeats), else RCCL when
// the ordinals are distinct (RCCL refuses two ranks on one device), else staged peer copies.
Exchange choose_exchange(int num_devices, const char* forced, bool all_peers, bool distinct) {
    const bool rccl = forced_onto(forced, "rccl"), copy = forced_onto(forced, "copy"), peer = forced_onto(forced, "peer");
    if (num_devices == 1 && !rccl) return Exchange::None;
    if (!rccl && !copy && all_peers) return Exchange::Direct;
    if (rccl || (distinct && !copy && !peer)) return Exchange::Rccl;
    return Exchange::Staged;
}

// One device of the group.  The context is created first: events and buffers exist only next to one.
struct GroupSlot {
    int ordinal = -1;
    crf_context* ctx = nullptr;
    int z_begin = 0, z_count = 0;      // the slot's slab of the global grid
    ncclComm_t comm = nullptr;         // Exchange::Rccl: this rank's communicator (destroyed by the group, before any slot)
    crf::DeviceBuffer<float> refvec;   // the cs reference values of the current evaluation (Rccl, Staged)
    crf::DeviceBuffer<float> rows;     // kBatchRows x cs reference rows of a batch (Rccl)
    crf::Event owner_ready;            // Staged: recorded by the owner after its gather
    crf::Event prep_done[2], block_done[2], rows_ready;  // order a batch's preparation stream against its main stream
    crf::Event job_done;               // completion poll of a device-resident job
    // crf_destroy binds the slot's device and synchronises the context's stream: nothing is in flight when the events
    // and buffers go, after this body and with that device still bound
    ~GroupSlot() { crf_destroy(ctx); }
};

}  // namespace

struct crf_group {
    const int n;
    std::vector<GroupSlot> slots;
    Rccl rccl;
    Exchange exchange = Exchange::None;
    std::string exchange_text = "none";
    std::unique_ptr<crf::SpinPool> workers;
    int xs = 0, ys = 0, zs = 0, cs = 0;
    std::string err;
    explicit crf_group(int num_devices) : n(num_devices), slots(size_t(num_devices)) {}
    // also of a partly filled group (crf_group_create's failure paths): the workers stop, RCCL is torn down before the
    // contexts its communicators use, then the slots release what they hold
    ~crf_group() {
        workers.reset();
        for (GroupSlot& s : slots)
            if (s.comm) (void)rccl.CommDestroy(s.comm);
        slots.clear();
    }
};

namespace {

int gfail(crf_group* g, int code, const std::string& msg) {
    if (g) g->err = msg;
    return code;
}

// first failing rank's status and message -> the group's error
int collect(crf_group* g, int status, const char* where) {
    if (status == 0) return CRF_OK;
    for (int r = 0; r < g->n; r++) {
        const char* m = crf_last_error(g->slots[size_t(r)].ctx);
        if (m && *m) return gfail(g, status, fmt("%s (device slot %d): %s", where, r, m));
    }
    return gfail(g, status, fmt("%s failed with status %d", where, status));
}

void slab(int zs, int n, int r, int* z0, int* zn) {  // the split of distributed.py:slab_bounds
    const int base = zs / n, rem = zs % n;
    *z0 = r * base + std::min(r, rem);
    *zn = base + (r < rem ? 1 : 0);
}

// Enables peer access between every pair of distinct devices of the group; false when some pair has none.
bool enable_all_peers(const crf_group* g) {
    bool all_peers = true;
    for (const GroupSlot& a : g->slots) {
        (void)hipSetDevice(a.ordinal);
        for (const GroupSlot& b : g->slots) {
            if (a.ordinal == b.ordinal) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, a.ordinal, b.ordinal) == hipSuccess && can) {
                const hipError_t pe = hipDeviceEnablePeerAccess(b.ordinal, 0);
                if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) all_peers = false;
            } else {
                all_peers = false;
            }
        }
    }
    (void)hipGetLastError();
    return all_peers;
}

// one single-process communicator over the group's devices, one rank per slot
int init_rccl(crf_group* g, const int* device_ordinals) {
    if (!g->rccl.load()) {
        g_group_create_error = "crf_group_create: " + g->rccl.error;
        return CRF_ERR_DEVICE;
    }
    std::vector<ncclComm_t> comms(size_t(g->n), nullptr);
    if (const int status = g->rccl.CommInitAll(comms.data(), g->n, device_ordinals)) {
        g_group_create_error = fmt("crf_group_create: ncclCommInitAll failed: %s", g->rccl.describe(status));
        return CRF_ERR_DEVICE;
    }
    for (int r = 0; r < g->n; r++) g->slots[size_t(r)].comm = comms[size_t(r)];
    return CRF_OK;
}

}  // namespace

extern "C" {

const char* crf_group_last_error(const crf_group* g) { return g ? g->err.c_str() : g_group_create_error.c_str(); }

int crf_group_size(const crf_group* g) { return g ? g->n : 0; }

crf_context* crf_group_context(crf_group* g, int slot) {
    return (g && slot >= 0 && slot < g->n) ? g->slots[size_t(slot)].ctx : nullptr;
}

const char* crf_group_exchange(const crf_group* g) { return g ? g->exchange_text.c_str() : ""; }

void crf_group_destroy(crf_group* g) { delete g; }

int crf_group_create(const int* device_ordinals, int num_devices, crf_group** out_group) {
    if (!out_group) return CRF_ERR_ARGUMENT;
    *out_group = nullptr;
    if (!device_ordinals || num_devices < 1 || num_devices > 64) {
        g_group_create_error = "crf_group_create: need 1..64 device ordinals";
        return CRF_ERR_ARGUMENT;
    }
    auto g = std::make_unique<crf_group>(num_devices);  // every failure below deletes what exists of it
    for (int r = 0; r < num_devices; r++) {
        GroupSlot& s = g->slots[size_t(r)];
        s.ordinal = device_ordinals[r];
        if (const int rc = crf_create(s.ordinal, &s.ctx)) {
            g_group_create_error = fmt("crf_group_create: device ordinal %d: %s", s.ordinal, crf_last_error(nullptr));
            return rc;
        }
        // the devices of a group share the host: bound each context's copier threads (host-output evaluations)
        s.ctx->copy_threads_cap = std::max(2, 16 / num_devices);
        (void)hipSetDevice(s.ordinal);
        for (crf::Event* e : {&s.owner_ready, &s.prep_done[0], &s.prep_done[1], &s.block_done[0], &s.block_done[1],
                              &s.rows_ready, &s.job_done})
            if (e->create(hipEventDisableTiming) != hipSuccess) {
                g_group_create_error = "crf_group_create: hipEventCreate failed";
                return CRF_ERR_DEVICE;
            }
    }
    const bool distinct = std::set<int>(device_ordinals, device_ordinals + num_devices).size() == size_t(num_devices);
    const char* forced = getenv("CRF_GROUP_EXCHANGE");
    const bool all_peers = num_devices == 1 || forced_onto(forced, "rccl") || enable_all_peers(g.get());
    g->exchange = choose_exchange(num_devices, forced, all_peers, distinct);
    const char* why = forced      ? "CRF_GROUP_EXCHANGE"
                      : !all_peers ? "no peer access between some pair of devices"
                      : distinct   ? "every pair of devices has peer access"
                                   : "a device ordinal repeats: rehearsal";
    switch (g->exchange) {
        case Exchange::None: g->exchange_text = "none (one device)"; break;
        case Exchange::Direct: g->exchange_text = fmt("peer read (direct gather from the owner's members; %s)", why); break;
        case Exchange::Staged: g->exchange_text = fmt("peer copy (staged: owner gathers, the others copy; %s)", why); break;
        case Exchange::Rccl:
            if (const int rc = init_rccl(g.get(), device_ordinals)) return rc;
            g->exchange_text = fmt("rccl (ncclBroadcast / ncclAllReduce, single-process communicator; %s)", why);
            break;
    }
    // one persistent worker per device slot, bound to its device once
    crf_group* raw = g.get();
    g->workers = std::make_unique<crf::SpinPool>(num_devices, [raw](int r) { (void)hipSetDevice(raw->slots[size_t(r)].ordinal); });
    *out_group = g.release();
    return CRF_OK;
}

int crf_group_set_grid(crf_group* g, int xs, int ys, int zs, int cs) {
    if (!g) return CRF_ERR_ARGUMENT;
    if (xs <= 0 || ys <= 0 || zs <= 0 || cs <= 0)
        return gfail(g, CRF_ERR_ARGUMENT, fmt("invalid grid %dx%dx%d with %d members", xs, ys, zs, cs));
    if (zs < g->n)
        return gfail(g, CRF_ERR_ARGUMENT, fmt("%d devices cannot share a grid of %d z-slices: every device needs one", g->n, zs));
    g->xs = xs;
    g->ys = ys;
    g->zs = zs;
    g->cs = cs;
    for (int r = 0; r < g->n; r++) slab(zs, g->n, r, &g->slots[size_t(r)].z_begin, &g->slots[size_t(r)].z_count);
    // everything a job needs is allocated here (the buffers only grow): a worker that failed an allocation inside a job
    // would leave the collective of the other ranks unmatched
    const int status = g->workers->run([&](int r) -> int {
        GroupSlot& s = g->slots[size_t(r)];
        if (int rc = crf_set_grid(s.ctx, xs, ys, s.z_count, cs)) return rc;
        hipError_t e = s.refvec.reserve(size_t(cs));
        if (e == hipSuccess && g->exchange == Exchange::Rccl) e = s.rows.reserve(size_t(kBatchRows) * size_t(cs));
        if (e == hipSuccess) return CRF_OK;
        s.ctx->err = fmt("hipMalloc of the reference vector / the batch's reference rows failed: %s", hipGetErrorString(e));
        return CRF_ERR_DEVICE;
    });
    return collect(g, status, "crf_group_set_grid");
}

int crf_group_slab(const crf_group* g, int slot, int* z_begin, int* z_count) {
    if (!g || slot < 0 || slot >= g->n || g->cs <= 0) return CRF_ERR_ARGUMENT;
    if (z_begin) *z_begin = g->slots[size_t(slot)].z_begin;
    if (z_count) *z_count = g->slots[size_t(slot)].z_count;
    return CRF_OK;
}

static int upload_slabs(crf_group* g, const float* const* host_members, bool secondary) {
    if (!g || !host_members) return gfail(g, CRF_ERR_ARGUMENT, "null argument");
    if (g->cs <= 0) return gfail(g, CRF_ERR_STATE, "crf_group_set_grid has not been called");
    for (int c = 0; c < g->cs; c++)
        if (!host_members[c]) return gfail(g, CRF_ERR_ARGUMENT, fmt("member %d is a null pointer", c));
    const size_t slice = size_t(g->xs) * size_t(g->ys);
    const int status = g->workers->run([&](int r) -> int {
        const GroupSlot& s = g->slots[size_t(r)];
        std::vector<const float*> slabs(size_t(g->cs));
        for (int c = 0; c < g->cs; c++) slabs[size_t(c)] = host_members[c] + slice * size_t(s.z_begin);
        return secondary ? crf_upload_secondary_members(s.ctx, slabs.data()) : crf_upload_members(s.ctx, slabs.data());
    });
    return collect(g, status, secondary ? "crf_group_upload_secondary_members" : "crf_group_upload_members");
}

int crf_group_upload_members(crf_group* g, const float* const* host_members) { return upload_slabs(g, host_members, false); }

int crf_group_upload_secondary_members(crf_group* g, const float* const* host_members) {
    return upload_slabs(g, host_members, true);
}

static int group_minmax(crf_group* g, bool secondary, float* out_min, float* out_max) {
    if (!g || !out_min || !out_max) return gfail(g, CRF_ERR_ARGUMENT, "null argument");
    std::vector<float> mn(size_t(g->n)), mx(size_t(g->n));
    const int status = g->workers->run([&](int r) -> int {
        crf_context* c = g->slots[size_t(r)].ctx;
        return secondary ? crf_secondary_member_minmax(c, &mn[size_t(r)], &mx[size_t(r)])
                         : crf_member_minmax(c, &mn[size_t(r)], &mx[size_t(r)]);
    });
    if (int rc = collect(g, status, "crf_group_member_minmax")) return rc;
    *out_min = *std::min_element(mn.begin(), mn.end());
    *out_max = *std::max_element(mx.begin(), mx.end());
    return CRF_OK;
}

int crf_group_member_minmax(crf_group* g, float* out_min, float* out_max) { return group_minmax(g, false, out_min, out_max); }

int crf_group_secondary_member_minmax(crf_group* g, float* out_min, float* out_max) {
    return group_minmax(g, true, out_min, out_max);
}

int crf_group_set_kraskov_noise(crf_group* g, const double* ref_noise, const double* query_noise) {
    if (!g) return CRF_ERR_ARGUMENT;
    const int status = g->workers->run(
        [&](int r) -> int { return crf_set_kraskov_noise(g->slots[size_t(r)].ctx, ref_noise, query_noise); });
    return collect(g, status, "crf_group_set_kraskov_noise");
}

int crf_group_set_profiling(crf_group* g, int enabled) {
    if (!g) return CRF_ERR_ARGUMENT;
    for (GroupSlot& s : g->slots) crf_set_profiling(s.ctx, enabled);
    return CRF_OK;
}

int crf_group_take_kernel_time(crf_group* g, double* out_ms_max, int* out_launches) {
    if (!g || !out_ms_max || !out_launches) return gfail(g, CRF_ERR_ARGUMENT, "null argument");
    double worst = 0.0;
    int launches = 0;
    for (GroupSlot& s : g->slots) {
        double ms = 0.0;
        int n = 0;
        if (int rc = crf_take_kernel_time(s.ctx, &ms, &n)) return gfail(g, rc, crf_last_error(s.ctx));
        worst = std::max(worst, ms);
        launches = std::max(launches, n);
    }
    *out_ms_max = worst;
    *out_launches = launches;
    return CRF_OK;
}

}  // extern "C"

namespace {

// Where the reference vector of one evaluation comes from, resolved once on the caller thread.
struct RefPlan {
    bool exchange = false;    // the reference point's values have to travel (not symmetric, no host vector)
    int owner = -1;           // slot whose slab holds the reference point
    int local_z = 0;          // its z inside that slab
    crf::RefOverride direct;  // Exchange::Direct: the owner's member table + the voxel inside the owner's slab
};

int plan_reference(crf_group* g, const crf_params* p, RefPlan* plan) {
    if (p->prepared_slot != 0) return gfail(g, CRF_ERR_ARGUMENT, "prepared slots are per context, not per group");
    const bool symmetric = (p->flags & CRF_FLAG_SYMMETRIC) != 0;
    plan->exchange = !symmetric && p->reference_values == nullptr;
    if (!plan->exchange) return CRF_OK;
    if (p->ref_x < 0 || p->ref_y < 0 || p->ref_z < 0 || p->ref_x >= g->xs || p->ref_y >= g->ys || p->ref_z >= g->zs)
        return gfail(g, CRF_ERR_ARGUMENT, fmt("reference point (%d,%d,%d) outside the grid %dx%dx%d", p->ref_x, p->ref_y,
                                              p->ref_z, g->xs, g->ys, g->zs));
    for (int r = 0; r < g->n; r++)
        if (const GroupSlot& s = g->slots[size_t(r)]; p->ref_z >= s.z_begin && p->ref_z < s.z_begin + s.z_count) {
            plan->owner = r;
            plan->local_z = p->ref_z - s.z_begin;
        }
    if (g->exchange == Exchange::Direct) {
        crf_context* owner = g->slots[size_t(plan->owner)].ctx;
        const bool from_secondary = (p->flags & CRF_FLAG_REFERENCE_FROM_SECONDARY) != 0;
        if (int rc = crf::reference_override(owner, from_secondary, p->ref_x, p->ref_y, plan->local_z, &plan->direct))
            return gfail(g, rc, crf_last_error(owner));
    }
    return CRF_OK;
}

// One call as every worker sees it.  It is read-only while the job runs and the same for all workers.  THE invariant of
// the job: every worker enters every collective and every SpinPool::barrier the same number of times, whatever its
// local status -- so whether and how a block exchanges is decided from this (the plans, the count, the group's exchange
// form), never from anything slot-local such as an error or a pointer.
struct Call {
    crf_group* g;
    const crf_params* params;
    int count;
    float* const* host_outs;   // count host buffers of the whole grid, or null:
    void* const* device_outs;  //   count x n device buffers of a slab each, evaluation-major
    std::vector<RefPlan> plans;
};

// What a block's evaluations read their reference values from (null, null: the parameters say it).
struct BlockRef {
    const void* vec[kBatchRows] = {};               // a device vector of cs floats
    const crf::RefOverride* ov[kBatchRows] = {};    // a direct read out of the owner's members
};

// The job of slot r for one call.  `rc` is the slot's one error accumulator: the first error stays, later steps that
// would launch work are skipped, steps that other workers wait in (collectives, barriers) are not.
struct SlotJob {
    const Call& call;
    const int r;
    crf_group* const g;
    GroupSlot& s;
    crf_context* const c;
    int rc = CRF_OK;
    SlotJob(const Call& call, int r) : call(call), r(r), g(call.g), s(g->slots[size_t(r)]), c(s.ctx) {}
    void note(int e) {  // status of a call that has left its message in the context
        if (e != CRF_OK && rc == CRF_OK) rc = e;
    }
    void fail(const std::string& what) {  // a device error of the group's own
        if (rc != CRF_OK) return;
        c->err = what;
        rc = CRF_ERR_DEVICE;
    }
    void note_hip(hipError_t e, const char* what) {
        if (e != hipSuccess) fail(what);
    }
    bool from_secondary(int i) const { return (call.params[i].flags & CRF_FLAG_REFERENCE_FROM_SECONDARY) != 0; }
    // what the slot hands to its context for evaluation i: in every form but None the vector arrives / is read remotely
    crf_params local_params(int i) const {
        crf_params local = call.params[i];
        if (g->exchange != Exchange::None) local.flags &= ~CRF_FLAG_REFERENCE_FROM_SECONDARY;
        return local;
    }

    // Rccl / Staged exchange of the reference vector of evaluation i on the slot's stream; leaves it in s.refvec.
    void exchange_one(int i) {
        const crf_params& p = call.params[i];
        const RefPlan& plan = call.plans[size_t(i)];
        const GroupSlot& owner = g->slots[size_t(plan.owner)];
        float* mine = s.refvec.get();
        const bool own = r == plan.owner;
        if (own) note(crf::gather_reference_to(c, from_secondary(i), p.ref_x, p.ref_y, plan.local_z, mine, c->stream));
        if (g->exchange == Exchange::Rccl) {
            if (const int status = g->rccl.Broadcast(mine, mine, size_t(g->cs), kNcclFloat32, plan.owner, s.comm, c->stream))
                fail(fmt("ncclBroadcast failed: %s", g->rccl.describe(status)));
            return;
        }
        if (own && rc == CRF_OK && hipEventRecord(s.owner_ready, c->stream) != hipSuccess) note(CRF_ERR_DEVICE);
        g->workers->barrier();  // the owner's event is recorded: the others may wait on it
        if (!own) {
            // The first of the staged form's two drains.  hipMemcpyPeerAsync is NOT reliably ordered behind kernels
            // launched earlier on the same stream (measured with two slots on one device: in a batch the copy of
            // evaluation i + 1 overtook the preparation kernel of evaluation i, which then read the next vector --
            // tools/repro_group_batch.py): the stream is drained before the copy is issued.
            if (hipStreamSynchronize(c->stream) != hipSuccess) note(CRF_ERR_DEVICE);
            if (hipStreamWaitEvent(c->stream, owner.owner_ready, 0) != hipSuccess ||
                hipMemcpyPeerAsync(mine, s.ordinal, owner.refvec.get(), owner.ordinal, sizeof(float) * size_t(g->cs),
                                   c->stream) != hipSuccess)
                fail("peer copy of the reference vector failed");
            // The second.  The owner must not overwrite its vector (the next evaluation's gather, possibly within the
            // same batch job) before the others' copies have EXECUTED, not just been enqueued: every copier waits for
            // its copy before the rendezvous.
            if (hipStreamSynchronize(c->stream) != hipSuccess) note(CRF_ERR_DEVICE);
        }
        g->workers->barrier();
    }

    // Rccl, a batch: the owners fill their rows (zeros elsewhere), one all-reduce(sum) gives every device the block's rows
    void all_reduce_rows(int b0, int bn, BlockRef* ref) {
        float* rows = s.rows.get();
        int32_t xyz[3 * kBatchRows];
        bool secondary = false;
        for (int j = 0; j < bn; j++) {
            const RefPlan& pl = call.plans[size_t(b0 + j)];
            xyz[3 * j] = call.params[b0 + j].ref_x;
            xyz[3 * j + 1] = call.params[b0 + j].ref_y;
            xyz[3 * j + 2] = pl.exchange && pl.owner == r ? pl.local_z : -1;  // -1: not this slot's row
            secondary = secondary || (pl.exchange && from_secondary(b0 + j));
        }
        if (secondary) {  // rows from the secondary field: one gather per such row, the rest zero-filled first
            if (hipMemsetAsync(rows, 0, sizeof(float) * size_t(bn) * size_t(g->cs), c->stream) != hipSuccess) note(CRF_ERR_DEVICE);
            for (int j = 0; j < bn; j++) {
                const RefPlan& pl = call.plans[size_t(b0 + j)];
                if (!pl.exchange || pl.owner != r) continue;
                note(crf::gather_reference_to(c, from_secondary(b0 + j), call.params[b0 + j].ref_x, call.params[b0 + j].ref_y,
                                              pl.local_z, rows + size_t(j) * size_t(g->cs), c->stream));
            }
        } else {
            note(crf_gather_reference_rows_device(c, xyz, bn, rows, nullptr));
        }
        if (const int status = g->rccl.AllReduce(rows, rows, size_t(bn) * size_t(g->cs), kNcclFloat32, kNcclSum, s.comm, c->stream))
            fail(fmt("ncclAllReduce failed: %s", g->rccl.describe(status)));
        for (int j = 0; j < bn; j++)
            if (call.plans[size_t(b0 + j)].exchange) ref->vec[j] = rows + size_t(j) * size_t(g->cs);
    }

    // The reference of a block's evaluations, as far as it is settled per block: Direct and Rccl.  (None: the context
    // reads its own members.  Staged exchanges per evaluation, immediately before it: evaluate_each.)
    void block_reference(int b0, int bn, BlockRef* ref) {
        bool any = false;
        for (int j = 0; j < bn; j++) {
            const RefPlan& pl = call.plans[size_t(b0 + j)];
            any = any || pl.exchange;
            if (g->exchange == Exchange::Direct && pl.exchange) ref->ov[j] = &pl.direct;
        }
        if (g->exchange != Exchange::Rccl || !any) return;
        if (call.count > 1) return all_reduce_rows(b0, bn, ref);
        exchange_one(0);
        ref->vec[0] = s.refvec.get();
    }

    // One evaluation after the other, each complete in itself: into the slot's part of the caller's host buffers, or into
    // the caller's device buffers for a single call and for a Staged batch.
    void evaluate_each(int b0, int bn, const BlockRef& ref) {
        const size_t first = size_t(g->xs) * size_t(g->ys) * size_t(s.z_begin);  // of the slot's slab in a host buffer
        for (int j = 0; j < bn; j++) {
            const int i = b0 + j;
            const void* vec = ref.vec[j];
            if (g->exchange == Exchange::Staged && call.plans[size_t(i)].exchange) {
                exchange_one(i);
                vec = s.refvec.get();
            }
            if (rc != CRF_OK) continue;  // not break: the exchanges of the remaining evaluations have barriers in them
            const crf_params local = local_params(i);
            if (call.host_outs) note(crf::compute_to_host(c, &local, vec, call.host_outs[i] + first, ref.ov[j]));
            else note(crf::compute_device_ex(c, &local, vec, call.device_outs[size_t(i) * size_t(g->n) + size_t(r)], nullptr, ref.ov[j]));
        }
    }

    // A block of a device-resident batch.  The reference-side preparations of the block (tiny kernels) run on the
    // context's SECOND stream, one block ahead of the per-voxel kernels, which follow back to back on the main stream: the
    // main stream carries nothing but per-voxel kernels.  Blocks alternate between the two halves of the prepared-slot
    // table; events order a half's re-use after the kernels that read it.
    void evaluate_pipelined(int b0, int bn, const BlockRef& ref) {
        static_assert(2 * kBatchRows == CRF_PREPARED_SLOTS, "two blocks of a batch share the prepared-slot table");
        const char* const ordering = "ordering the preparation stream of a batch failed";
        const int parity = (b0 / kBatchRows) % 2;
        const int slot0 = parity * kBatchRows;
        hipStream_t aux = nullptr;
        note(crf::second_stream(c, &aux));
        if (rc == CRF_OK && b0 >= 2 * kBatchRows) note_hip(hipStreamWaitEvent(aux, s.block_done[parity], 0), ordering);
        bool has_rows = false;
        for (int j = 0; j < bn; j++) has_rows = has_rows || ref.vec[j] != nullptr;
        if (rc == CRF_OK && has_rows) {  // rows exchanged on the main stream (Rccl): the preparations read them
            note_hip(hipEventRecord(s.rows_ready, c->stream), ordering);
            if (rc == CRF_OK) note_hip(hipStreamWaitEvent(aux, s.rows_ready, 0), ordering);
        }
        for (int j = 0; j < bn && rc == CRF_OK; j++) {
            const crf_params local = local_params(b0 + j);
            if (local.flags & CRF_FLAG_SYMMETRIC) continue;  // no reference side
            note(crf::prepare_device_ex(c, &local, ref.vec[j], slot0 + j, aux, ref.ov[j]));
        }
        if (rc == CRF_OK) note_hip(hipEventRecord(s.prep_done[parity], aux), ordering);
        if (rc == CRF_OK) note_hip(hipStreamWaitEvent(c->stream, s.prep_done[parity], 0), ordering);
        for (int j = 0; j < bn && rc == CRF_OK; j++) {
            const int i = b0 + j;
            crf_params local = local_params(i);
            if (!(local.flags & CRF_FLAG_SYMMETRIC)) local.prepared_slot = slot0 + j + 1;
            note(crf_compute_device(c, &local, nullptr, call.device_outs[size_t(i) * size_t(g->n) + size_t(r)], nullptr));
        }
        if (rc == CRF_OK) note_hip(hipEventRecord(s.block_done[parity], c->stream), ordering);
    }

    // host outputs return synchronised; device-resident results: one synchronisation per job, polling the slot's event
    void finish() {
        if (call.host_outs) return;
        if (hipEventRecord(s.job_done, c->stream) != hipSuccess || crf::spin_on_event(s.job_done) != hipSuccess)
            fail("synchronisation failed after the evaluation");
    }
};

int check_call(crf_group* g, const crf_params* params, int count, float* const* host_outs, void* const* device_outs) {
    if (!g || !params || count < 1 || (!host_outs && !device_outs)) return gfail(g, CRF_ERR_ARGUMENT, "null argument");
    if (g->cs <= 0) return gfail(g, CRF_ERR_STATE, "crf_group_set_grid has not been called");
    for (int i = 0; i < count; i++) {
        if (host_outs && !host_outs[i]) return gfail(g, CRF_ERR_ARGUMENT, fmt("host output %d is a null pointer", i));
        if (device_outs)
            for (int r = 0; r < g->n; r++)
                if (!device_outs[size_t(i) * size_t(g->n) + size_t(r)])
                    return gfail(g, CRF_ERR_ARGUMENT, fmt("device output of evaluation %d, slot %d is a null pointer", i, r));
    }
    // the exchange reads another context's member table as fp32 (crf::RefOverride)
    for (int r = 0; r < g->n; r++)
        if (g->slots[size_t(r)].ctx->grid.format != CRF_MEMBER_F32 ||
            g->slots[size_t(r)].ctx->grid.secondary_format != CRF_MEMBER_F32)
            return gfail(g, CRF_ERR_UNSUPPORTED,
                         fmt("device groups evaluate fp32 members only: the context of slot %d holds members in a narrow "
                             "native format (crf_bind_members_device_format, crf_bind_secondary_members_device_format)", r));
    return CRF_OK;
}

// `count` evaluations over the whole grid, handed to the workers in ONE job: per block of up to kBatchRows evaluations
// the exchange of the reference vectors, then every device evaluates its slab -- into its part of the caller's HOST
// buffers (host_outs != null: calculateCpu(t, e, buffer)) or into the caller's per-device DEVICE buffers
// (device_outs[evaluation * n + slot] receives the slab of that slot: xs*ys*z_count floats, resident for a device-side
// consumer).  The workers synchronise once, at the end.
int group_compute(crf_group* g, const crf_params* params, int count, float* const* host_outs, void* const* device_outs) {
    if (int rc = check_call(g, params, count, host_outs, device_outs)) return rc;
    Call call{g, params, count, host_outs, device_outs, std::vector<RefPlan>(size_t(count))};
    for (int i = 0; i < count; i++)
        if (int rc = plan_reference(g, &params[i], &call.plans[size_t(i)])) return rc;
    const bool pipelined = count > 1 && !host_outs && g->exchange != Exchange::Staged;
    const char* trace_env = getenv("CRF_GROUP_TRACE");  // development: host-side phase times of slot 0 on stderr
    const bool trace = trace_env && *trace_env == '1';
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_call).count(); };
    const int status = g->workers->run([&](int r) -> int {
        const double t_start = since();
        SlotJob job{call, r};
        for (int b0 = 0; b0 < count; b0 += kBatchRows) {
            const int bn = std::min(kBatchRows, count - b0);
            BlockRef ref;
            job.block_reference(b0, bn, &ref);
            const double t_exchanged = since();
            if (pipelined) job.evaluate_pipelined(b0, bn, ref);
            else job.evaluate_each(b0, bn, ref);
            if (trace && r == 0)
                fprintf(stderr, "crf_group slot 0: job started %.0f us after the call, exchange of block %d issued by %.0f us, "
                                "evaluations issued by %.0f us\n", t_start, b0 / kBatchRows, t_exchanged, since());
        }
        job.finish();
        return job.rc;
    });
    if (trace) fprintf(stderr, "crf_group: returned to the caller after %.0f us\n", since());
    return collect(g, status, host_outs ? "crf_group_compute" : "crf_group_compute_device");
}

}  // namespace

extern "C" {

int crf_group_compute(crf_group* g, const crf_params* p, float* host_out) {
    if (!host_out) return gfail(g, CRF_ERR_ARGUMENT, "null output");
    return group_compute(g, p, 1, &host_out, nullptr);
}

int crf_group_compute_device(crf_group* g, const crf_params* p, void* const* device_outs) {
    if (!device_outs) return gfail(g, CRF_ERR_ARGUMENT, "null output table");
    return group_compute(g, p, 1, nullptr, device_outs);
}

int crf_group_compute_batch(crf_group* g, const crf_params* params, int count, float* const* host_outs) {
    if (!host_outs) return gfail(g, CRF_ERR_ARGUMENT, "null output table");
    if (count == 0) return CRF_OK;
    return group_compute(g, params, count, host_outs, nullptr);
}

int crf_group_compute_batch_device(crf_group* g, const crf_params* params, int count, void* const* device_outs) {
    if (!device_outs) return gfail(g, CRF_ERR_ARGUMENT, "null output table");
    if (count == 0) return CRF_OK;
    return group_compute(g, params, count, nullptr, device_outs);
}

}  // extern "C"
