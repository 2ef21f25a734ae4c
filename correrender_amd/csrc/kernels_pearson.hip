// kernels_pearson.hip -- Pearson correlation field on gfx950.
//
// Semantics: computePearson2<float>(referenceValues, fields, cs, voxel) of the reference
// (src/Calculators/Correlation.cpp:100-133, selected by FORMULA_2_FLOAT at CorrelationCalculator.cpp:887-893),
// reproduced operation for operation in fp32 with contraction off (built with -ffp-contract=off) so that results
// are bit-identical to the reference's x86-64 build (no FMA: CMakeLists.txt:34-36 sets no -march):
//     pass 1   meanY += invN * y_e                         (e = 0..cs-1, sequential)
//     pass 2   varY  += (invNm1 * (y_e - meanY)) * (y_e - meanY)
//     pass 3   r     += (invNm1 * ((x_e - meanX) / sdX)) * ((y_e - meanY) / sdY)
// Every reference-only term -- meanX, sdX and a_e = invNm1 * ((x_e - meanX) / sdX) -- is voxel independent and is
// computed once by pearson_prep_kernel with the same sequential fp32 arithmetic; the per-voxel kernel then needs
// only the cs a_e values (scalar loads -> SGPRs).
//
// Data movement (the bound): each voxel reads its cs member values exactly once from HBM (4*cs bytes) and writes
// 4 bytes.  One lane owns VPT consecutive voxels and keeps all cs values in VGPRs across the three passes; a wave
// load instruction covers 64*VPT consecutive floats of ONE member volume (256 B / 512 B / 1 KiB contiguous), all
// cs loads of a wave are issued back to back before the first use, so a wave has cs*256*VPT bytes in flight.
// No LDS, no MFMA: ~4 flop/byte, HBM-read bound.
#include "crf_device.h"
#include "crf_internal.h"
#include "crf_two_vector_device.h"

namespace crf {

constexpr int kPrepZeroFilled = 1280;  // a_e = 0 for cs <= e < this: the padded slots of the register and split kernels

// ---------------------------------------------------------------------------------------------------------
// Reference-side preparation: one wave.  d_prep[e] = a_e for e < cs.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pearson_prep_kernel(RefSource src, const float* const* __restrict__ members,
                                                           int cs, float* __restrict__ prep) {
    extern __shared__ float x[];  // cs reference values
    __shared__ float sh[2];
    for (int e = threadIdx.x; e < cs; e += blockDim.x) x[e] = load_ref(src, members, e);
    __syncthreads();
    const float n = float(cs);
    const float invN = 1.0f / n;
    const float invNm1 = 1.0f / (n - 1.0f);
    if (threadIdx.x == 0) {
        float meanX = 0.0f;
        for (int e = 0; e < cs; e++) meanX += invN * x[e];
        float varX = 0.0f;
        for (int e = 0; e < cs; e++) {
            const float d = x[e] - meanX;
            varX += invNm1 * d * d;
        }
        sh[0] = meanX;
        sh[1] = sqrtf(varX);
    }
    __syncthreads();
    const float meanX = sh[0], sdX = sh[1];
    for (int e = threadIdx.x; e < cs; e += blockDim.x) prep[e] = invNm1 * ((x[e] - meanX) / sdX);
    // padded slots of the guarded register kernels multiply by a_e = 0 (see pearson_reg_kernel)
    for (int e = cs + threadIdx.x; e < kPrepZeroFilled; e += blockDim.x) prep[e] = 0.0f;
}

// ---------------------------------------------------------------------------------------------------------
// Per-voxel kernel, members resident in registers.
//   CS_PAD  compile-time upper bound of cs (loops fully unrolled to it); EXACT: cs == CS_PAD, no guards; otherwise
//           CS_PAD - pad_granule(CS_PAD) < cs < CS_PAD and only the last granule is guarded.
//   VPT     voxels per lane (1 or 2) = width of each global load in dwords.
// ---------------------------------------------------------------------------------------------------------
template <int VPT>
struct VecT;
template <>
struct VecT<1> {
    using type = float;
};
template <>
struct VecT<2> {
    using type = float __attribute__((ext_vector_type(2)));
};

// VPT consecutive voxels of one member for this lane (see crf_device.h: buffer descriptor + shared 32-bit offset).
// Non-temporal loads: measured 0.753 -> 0.705 ms at 256^3 x 64 on MI355X against the default policy
// (profiles/tuning_r01.md).
template <int VPT>
__device__ __forceinline__ void load_vec(const float* base, uint32_t bytes, uint32_t byte_offset, float (&dst)[VPT]) {
    const auto rsrc = make_member_rsrc(base, bytes);
    if constexpr (VPT == 1) {
        dst[0] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, int(byte_offset), 0, kAuxNonTemporal));
    } else {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, int(byte_offset), 0, kAuxNonTemporal);
        dst[0] = __uint_as_float(v[0]);
        dst[1] = __uint_as_float(v[1]);
    }
}
template <int VPT>
__device__ __forceinline__ void store_vec(float* p, const float (&src)[VPT]) {
    using V = typename VecT<VPT>::type;
    V v;
    __builtin_memcpy(&v, src, sizeof(V));
    // non-temporal: the result is written once and not read by this kernel -- keeping it out of the caches' way measured
    // 0.692 -> 0.657 ms at 256^3 x 64 (78.9 -> 83.0 % of the HBM peak, same box, interleaved; profiles/tuning_r01.md)
    __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
}

// launch_pearson pads cs to the next multiple of this: only the last granule of a guarded instantiation can be padding
constexpr int pad_granule(int cs_pad) { return cs_pad <= 16 ? 8 : cs_pad <= 128 ? 16 : 32; }

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

template <int CS_PAD, bool EXACT>
__device__ __forceinline__ void pearson_packed_wave(const float* const* __restrict__ members,
                                                    const float* __restrict__ prep, float* __restrict__ out,
                                                    uint32_t num_voxels, int cs, const PackedMembers& packed);

// PACKED: the members come from their packed copy (crf_internal.h; pearson_packed_wave below), VPT = 1.
template <int CS_PAD, int VPT, bool EXACT, int MIN_WAVES, bool PACKED>
__global__ __launch_bounds__(256, MIN_WAVES) void pearson_reg_kernel(const float* const* __restrict__ members,
                                                                     const float* __restrict__ prep,
                                                                     float* __restrict__ out, uint32_t num_voxels,
                                                                     int cs, PackedMembers packed) {
    static_assert(CS_PAD <= kPrepZeroFilled, "a_e is zero-filled up to kPrepZeroFilled");
    if constexpr (PACKED) {
        static_assert(VPT == 1, "one voxel per lane: a wave is one 64-voxel tile of the packed copy");
        pearson_packed_wave<CS_PAD, EXACT>(members, prep, out, num_voxels, cs, packed);
        return;
    }
    constexpr int kFirstGuarded = EXACT ? CS_PAD : CS_PAD - pad_granule(CS_PAD);  // slots below are always members
    const auto is_member = [cs](int e) { return e < kFirstGuarded || e < cs; };      // folds in the unrolled loops
    const uint32_t v0 = (blockIdx.x * 256 + threadIdx.x) * VPT;
    const uint32_t byte_offset = v0 * 4u;       // one 32-bit offset serves all cs loads of the lane
    const uint32_t bytes = num_voxels * 4u;     // descriptor bound: lanes past the end read 0 and store nothing
    // Guarded instantiation (cs < CS_PAD), branch free: a padded slot loads at an out-of-range offset (the value is 0
    // and no memory request is made: crf_device.h kOutOfRangeOffset), its deviation is forced to 0 in pass 2 and its
    // a_e is 0 (pearson_prep_kernel), so each pass adds +0 for it -- an identity on the running sums, which start at
    // +0 and therefore are never -0.  In pass 3 exact_div(0, sd) = 0 on the fast path; the plain-division path (sd
    // may be 0 there: 0/0) selects 0 for the pads explicitly.
    float y[CS_PAD][VPT];
#pragma unroll
    for (int e = 0; e < CS_PAD; e++) {
        if (e < kFirstGuarded) {
            load_vec<VPT>(members[e], bytes, byte_offset, y[e]);
        } else if (CS_PAD >= 224) {
            // the widest kernels have no register to spare for per-slot offsets: a uniform branch around each of the
            // few guarded loads instead (they are the last loads issued)
#pragma unroll
            for (int v = 0; v < VPT; v++) y[e][v] = 0.0f;
            if (e < cs) load_vec<VPT>(members[e], bytes, byte_offset, y[e]);
        } else {
            load_vec<VPT>(members[e < cs ? e : cs - 1], bytes, e < cs ? byte_offset : kOutOfRangeOffset, y[e]);
        }
    }
    const float n = float(cs);
    const float invN = 1.0f / n;
    const float invNm1 = 1.0f / (n - 1.0f);

    float meanY[VPT];
#pragma unroll
    for (int v = 0; v < VPT; v++) meanY[v] = 0.0f;
#pragma unroll
    for (int e = 0; e < CS_PAD; e++) {
#pragma unroll
        for (int v = 0; v < VPT; v++) meanY[v] += invN * y[e][v];
    }
    float varY[VPT];
#pragma unroll
    for (int v = 0; v < VPT; v++) varY[v] = 0.0f;
#pragma unroll
    for (int e = 0; e < CS_PAD; e++) {
#pragma unroll
        for (int v = 0; v < VPT; v++) {
            const float d = is_member(e) ? y[e][v] - meanY[v] : 0.0f;
            y[e][v] = d;  // (y_e - meanY) is needed again, bit-identically, by pass 3
            varY[v] += invNm1 * d * d;
        }
    }
    float r[VPT];
    float sdY[VPT];
#pragma unroll
    for (int v = 0; v < VPT; v++) {
        sdY[v] = sqrtf(varY[v]);
        r[v] = 0.0f;
    }
    bool guard = true;
#pragma unroll
    for (int v = 0; v < VPT; v++) guard = guard && exact_div_guard(meanY[v], sdY[v]);
    if (__all(guard)) {  // exact quotients through one reciprocal per voxel (crf_exact_div.h: exact_div)
        float rcp[VPT];
#pragma unroll
        for (int v = 0; v < VPT; v++) rcp[v] = 1.0f / sdY[v];
#pragma unroll
        for (int e = 0; e < CS_PAD; e++) {
            const float a = prep[e];
#pragma unroll
            for (int v = 0; v < VPT; v++) r[v] += a * exact_div(y[e][v], sdY[v], rcp[v]);
        }
    } else {
#pragma unroll
        for (int e = 0; e < CS_PAD; e++) {
            const float a = prep[e];
#pragma unroll
            for (int v = 0; v < VPT; v++) r[v] += a * (is_member(e) ? y[e][v] / sdY[v] : 0.0f);
        }
    }
    if (v0 + VPT <= num_voxels) store_vec<VPT>(out + v0, r);
}

// ---------------------------------------------------------------------------------------------------------
// pearson_reg_kernel on the packed copy (crf_internal.h): one wave = one 64-voxel tile.  The wave reads the tile's
// CS_PAD base bytes with scalar loads and its 1 KiB runs with one dwordx4 buffer load each (all issued before the first
// use, as the cs member loads of the raw form), then decodes every value.  A tile with a segment that did not fit then
// reads that member from the member itself, in a uniform branch (the decode itself has no branches).  The arithmetic is the raw form's, operation for operation, with what
// is off the sequential sums done two slots at a time in packed fp32 (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32: the
// same IEEE operations per element, as in pearson_split_kernel) to make room for the decode.
// ---------------------------------------------------------------------------------------------------------
template <int CS_PAD, bool EXACT>
__device__ __forceinline__ void pearson_packed_wave(const float* const* __restrict__ members,
                                                    const float* __restrict__ prep, float* __restrict__ out,
                                                    uint32_t num_voxels, int cs, const PackedMembers& packed) {
    static_assert(CS_PAD % 16 == 0 && CS_PAD >= 32 && CS_PAD <= kPackMaxMembers, "pack_slots() of a packed cs");
    constexpr int kLo = CS_PAD / 8, kByte = CS_PAD / 16, kCode = (CS_PAD + 31) / 32;
    constexpr uint32_t kTileBytes = 1024u * uint32_t(kLo + kByte + kCode);
    constexpr int kFirstGuarded = EXACT ? CS_PAD : CS_PAD - 16;
    const auto is_member = [cs](int e) { return e < kFirstGuarded || e < cs; };
    const uint32_t tile = blockIdx.x * 4u + uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    if (tile >= (num_voxels + 63u) / 64u) return;  // the last block's surplus waves
    const uint32_t v0 = tile * 64u + (threadIdx.x & 63u);
    const uint32_t byte_offset = v0 * 4u, bytes = num_voxels * 4u;  // fallback members: lanes past the end read 0
    const uint32_t* header = reinterpret_cast<const uint32_t*>(packed.header + size_t(tile) * CS_PAD);
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(packed.body) + size_t(tile) * kTileBytes,
                                                        short(0), int(kTileBytes), 0x00020000);
    const int lane_bytes = int(threadIdx.x & 63u) * 16;
    u4 code[kCode], byte[kByte], lo[kLo];
    // issue order = order of first use (the first members need code run 0, byte run 0, lo run 0)
#pragma unroll
    for (int r = 0; r < kCode; r++)
        code[r] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane_bytes + 1024 * (kLo + kByte + r), 0, kAuxNonTemporal);
#pragma unroll
    for (int r = 0; r < kLo; r++) {
        if (r % 2 == 0)
            byte[r / 2] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane_bytes + 1024 * (kLo + r / 2), 0, kAuxNonTemporal);
        lo[r] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane_bytes + 1024 * r, 0, kAuxNonTemporal);
    }
    uint32_t hdr[CS_PAD / 4];  // base bytes, wave-uniform (SGPRs)
    uint32_t fallback = 0;     // non-zero: some segment of the tile is read from its member
#pragma unroll
    for (int i = 0; i < CS_PAD / 4; i++) {
        hdr[i] = header[i];
        const uint32_t t = ~hdr[i];  // a byte of kPackFallback is a zero byte of t
        fallback |= (t - 0x01010101u) & ~t & 0x80808080u;
    }
    f2 y[CS_PAD / 2];
#pragma unroll
    for (int e = 0; e < CS_PAD; e++)  // (a fallback segment decodes to 0 here: its planes hold zeros)
        y[e / 2][e % 2] = __uint_as_float(unpack_bits(lo[e / 8][(e % 8) / 2], e % 2, byte[e / 16][(e % 16) / 4], e % 4,
                                                      code[e / 32][(e % 32) / 8], e % 8, (hdr[e / 4] >> (8 * (e % 4))) & 0xFFu));
    if (fallback != 0u) {  // uniform; about a third of the tiles of the benchmark's ensemble, one or two members each
#pragma unroll
        for (int e = 0; e < CS_PAD; e++) {
            if (((hdr[e / 4] >> (8 * (e % 4))) & 0xFFu) == kPackFallback)  // never a padded slot (base 1)
                y[e / 2][e % 2] = load_member_nt(members[e < kFirstGuarded || e < cs ? e : cs - 1], bytes, byte_offset);
        }
    }
    const float n = float(cs);
    const float invN = 1.0f / n;
    const float invNm1 = 1.0f / (n - 1.0f);
    // pass 1: meanY += invN * y_e (a padded slot is +0 and adds +0)
    float meanY = 0.0f;
    {
        const f2 scale = {invN, invN};
#pragma unroll
        for (int k = 0; k < CS_PAD / 2; k++) {
            const f2 t = scale * y[k];
            meanY += t[0];
            meanY += t[1];
        }
    }
    // deviations in place (needed again, bit-identically, by pass 3); a padded slot's is forced to 0
    {
        const f2 mean2 = {meanY, meanY};
#pragma unroll
        for (int k = 0; k < CS_PAD / 2; k++) {
            f2 d = y[k] - mean2;
            if (2 * k >= kFirstGuarded) {
                if (!is_member(2 * k)) d[0] = 0.0f;
                if (!is_member(2 * k + 1)) d[1] = 0.0f;
            }
            y[k] = d;
        }
    }
    // pass 2: varY += (invNm1 * d_e) * d_e
    float varY = 0.0f;
    {
        const f2 scale = {invNm1, invNm1};
#pragma unroll
        for (int k = 0; k < CS_PAD / 2; k++) {
            const f2 t = (scale * y[k]) * y[k];
            varY += t[0];
            varY += t[1];
        }
    }
    const float sdY = sqrtf(varY);
    float r = 0.0f;
    if (__all(exact_div_guard(meanY, sdY))) {  // exact_div (crf_exact_div.h) two slots at a time, then r += a_e * q_e
        const float rcp = 1.0f / sdY;
        const f2 rcp2 = {rcp, rcp}, sd2 = {sdY, sdY};
#pragma unroll
        for (int k = 0; k < CS_PAD / 2; k++) {
            const f2 q0 = y[k] * rcp2;
            const f2 rem = __builtin_elementwise_fma(-q0, sd2, y[k]);
            const f2 q = __builtin_elementwise_fma(rem, rcp2, q0);
            const f2 a = {prep[2 * k], prep[2 * k + 1]};
            const f2 t = a * q;
            r += t[0];
            r += t[1];
        }
    } else {
#pragma unroll
        for (int e = 0; e < CS_PAD; e++) r += prep[e] * (is_member(e) ? y[e / 2][e % 2] / sdY : 0.0f);
    }
    if (v0 < num_voxels) store_result_nt(out + v0, r);
}

// The packed copy (crf_internal.h), built once per set of members: one wave per tile, one member at a time (the
// segment's exponent range is a wave reduction).  Plain loads and dword stores: this runs once, not per step.
__global__ __launch_bounds__(256) void pearson_encode_kernel(const float* const* __restrict__ members,
                                                             uint32_t num_voxels, int cs,
                                                             unsigned char* __restrict__ header,
                                                             unsigned char* __restrict__ body,
                                                             uint32_t* __restrict__ fallbacks) {
    const int slots = pack_slots(cs);
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= (num_voxels + 63u) / 64u) return;
    const int lane = int(threadIdx.x & 63u);
    const uint32_t v = tile * 64u + uint32_t(lane);
    // this lane's 16 B of run 0; dword k of run q is lane_words[256 q + k]
    uint32_t* lane_words = reinterpret_cast<uint32_t*>(body + size_t(tile) * pack_tile_bytes(slots) + 16 * lane);
    const int byte_run0 = pack_lo_runs(slots), code_run0 = byte_run0 + pack_byte_runs(slots);
    uint32_t lo_w = 0, byte_w = 0, code_w = 0, fell_back = 0;
#pragma unroll 1
    for (int e = 0; e < slots; e++) {
        const uint32_t bits = e < cs && v < num_voxels ? __float_as_uint(members[e][v]) : 0u;
        const uint32_t ex = (bits >> 23) & 0xFFu;
        uint32_t emin = ex != 0u ? ex : 256u, emax = ex;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            emin = min(emin, uint32_t(__shfl_xor(int(emin), o)));
            emax = max(emax, uint32_t(__shfl_xor(int(emax), o)));
        }
        const uint32_t base = pack_segment_base(emin, emax, emax == 255u);
        const uint32_t b = base == kPackFallback ? 0u : bits;  // a fallback segment's planes hold zeros
        lo_w |= pack_lo16(b) << (16 * (e & 1));
        byte_w |= pack_byte(b) << (8 * (e & 3));
        code_w |= pack_code(b, base) << (4 * (e & 7));
        if ((e & 1) == 1) {
            lane_words[256 * (e / 8) + (e % 8) / 2] = lo_w;
            lo_w = 0;
        }
        if ((e & 3) == 3) {
            lane_words[256 * (byte_run0 + e / 16) + (e % 16) / 4] = byte_w;
            byte_w = 0;
        }
        if ((e & 7) == 7) {
            lane_words[256 * (code_run0 + e / 32) + (e % 32) / 8] = code_w;
            code_w = 0;
        }
        if (lane == 0) header[size_t(tile) * size_t(slots) + size_t(e)] = static_cast<unsigned char>(base);
        fell_back += base == kPackFallback ? 1u : 0u;  // (padded slots always fit)
    }
    if (slots % 32 == 16) {  // the unused half of the last code run
        lane_words[256 * (code_run0 + slots / 32) + 2] = 0u;
        lane_words[256 * (code_run0 + slots / 32) + 3] = 0u;
    }
    if (lane == 0 && fell_back != 0u) atomicAdd(fallbacks, fell_back);
}

hipError_t launch_pack_members(const float* const* d_members, int cs, size_t num_voxels, unsigned char* header,
                               unsigned char* body, uint32_t* d_fallbacks, hipStream_t s) {
    if (cs < kPackMinMembers || cs > kPackMaxMembers || num_voxels == 0 || num_voxels >= (size_t(1) << 32))
        return hipErrorInvalidValue;
    const size_t tiles = (num_voxels + 63) / 64;
    hipLaunchKernelGGL(pearson_encode_kernel, dim3(unsigned((tiles + 3) / 4)), dim3(256), 0, s, d_members,
                       uint32_t(num_voxels), cs, header, body, d_fallbacks);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// R + up to L members: the first R values of a voxel in registers (always members: no guards), the remaining cs - R
// (1..L) in the lane's LDS column.  For member counts just above what fits two waves per SIMD in registers: 256
// register values spill 120 B - 1 KB under the 256-register cap, 240 + 16 in LDS do not (16 x 1 KB per block).
// The tail slots are handled in uniform branches (they are in LDS: no register live ranges to split).
// ---------------------------------------------------------------------------------------------------------
template <int R, int L, int MIN_WAVES>
__global__ __launch_bounds__(256, MIN_WAVES) void pearson_reg_lds_kernel(const float* const* __restrict__ members,
                                                                         const float* __restrict__ prep,
                                                                         float* __restrict__ out, uint32_t num_voxels,
                                                                         int cs) {
    extern __shared__ float tail_dyn[];  // L rows of 256 floats
    float(*tail)[256] = reinterpret_cast<float(*)[256]>(tail_dyn);
    const uint32_t v0 = blockIdx.x * 256u + threadIdx.x;
    const uint32_t byte_offset = v0 * 4u, bytes = num_voxels * 4u;
    const int nt = cs - R;  // members in the LDS tail, 1..L
    float y[R];
#pragma unroll
    for (int e = 0; e < R; e++) y[e] = load_member_nt(members[e], bytes, byte_offset);
    // the tail goes straight from memory to LDS (global_load_lds: no registers, issued back to back with the loads above;
    // the hardware writes lane l of a wave to lds_base + 4 l, i.e. the wave's own 64 consecutive floats of the row,
    // which only this wave reads again, so the only synchronisation is its own vmcnt wait).  Lanes past the end of the
    // grid read the last voxel instead (no descriptor bounds on this path); they store nothing.
    const int wave_first = int(threadIdx.x) & ~63;
    const uint32_t v_safe = v0 < num_voxels ? v0 : num_voxels - 1u;
#pragma unroll
    for (int t = 0; t < L; t++) {
        if (t < nt) {
            typedef const float __attribute__((address_space(1)))* gptr_t;
            typedef float __attribute__((address_space(3)))* lptr_t;
            __builtin_amdgcn_global_load_lds((gptr_t)(members[R + t] + v_safe), (lptr_t)&tail[t][wave_first], 4, 0,
                                             kAuxNonTemporal);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const float n = float(cs);
    const float invN = 1.0f / n;
    const float invNm1 = 1.0f / (n - 1.0f);
    float meanY = 0.0f;
#pragma unroll
    for (int e = 0; e < R; e++) meanY += invN * y[e];
#pragma unroll
    for (int t = 0; t < L; t++)
        if (t < nt) meanY += invN * tail[t][threadIdx.x];
    float varY = 0.0f;
#pragma unroll
    for (int e = 0; e < R; e++) {
        const float d = y[e] - meanY;
        y[e] = d;
        varY += invNm1 * d * d;
    }
#pragma unroll
    for (int t = 0; t < L; t++) {
        if (t < nt) {
            const float d = tail[t][threadIdx.x] - meanY;
            tail[t][threadIdx.x] = d;
            varY += invNm1 * d * d;
        }
    }
    const float sdY = sqrtf(varY);
    float r = 0.0f;
    if (__all(exact_div_guard(meanY, sdY))) {
        const float rcp = 1.0f / sdY;
#pragma unroll
        for (int e = 0; e < R; e++) r += prep[e] * exact_div(y[e], sdY, rcp);
#pragma unroll
        for (int t = 0; t < L; t++)
            if (t < nt) r += prep[R + t] * exact_div(tail[t][threadIdx.x], sdY, rcp);
    } else {
#pragma unroll
        for (int e = 0; e < R; e++) r += prep[e] * (y[e] / sdY);
#pragma unroll
        for (int t = 0; t < L; t++)
            if (t < nt) r += prep[R + t] * (tail[t][threadIdx.x] / sdY);
    }
    if (v0 < num_voxels) store_result_nt(out + v0, r);
}

// ---------------------------------------------------------------------------------------------------------
// 289..1216 members (r03): G = 2 or 4 LANES per voxel.  A wave owns 64 / G voxels; lane group g (lanes g * 64 / G ...)
// holds members [g * S, g * S + S) of them, S = R + L slots per lane: R in registers and L in the lane's LDS column,
// exactly the storage of the 176..288-member kernels above, which run at two waves per SIMD and 70-88 % of the HBM
// peak -- instead of one wave per SIMD with 384 values in VGPRs + AGPRs (37-56 %), an 8-wave relay through LDS
// (385..512 members, 37 %; r02, since removed) or three sweeps over the members (beyond 512: 3x the algorithmic bytes).
// The three passes of computePearson2<float> are sequential fp32 sums over the members, so each pass is a relay of
// G stages inside the wave: in stage gg every lane runs the chain over its own S slots, starting from the value that
// group gg - 1 handed over (ds_bpermute, no LDS memory), and only group gg's result is kept; the other groups compute
// throw-away values in that stage (no traps, nothing stored).  Same operations in the same order as the reference,
// every member value fetched once.  What does not lie on a chain -- products, deviations, quotients -- is done once
// and two slots at a time (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32: the same IEEE operations per element), which
// pays for the repeated chain stages: 12.9 vector instructions per slot at G = 2 against 12 per member in
// pearson_reg_kernel.  A load instruction is issued per member under the owning group's exec mask (the descriptor is
// wave-uniform), 256 / G bytes each.
//   PAD   cs lies in (G * S - PAD, G * S]: only the last PAD slots of the last group can be padding (they read 0, their
//         deviation is forced to 0 and a_e = 0 for e >= cs: every pass adds +0 for them, as in pearson_reg_kernel).
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float from_lane(float v, int src_lane) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(src_lane << 2, __float_as_int(v)));
}

constexpr int kSplitMaxMembers = 4 * 304;  // 1216

template <int R, int L, int G, int PAD, int MIN_WAVES>
__global__ __launch_bounds__(256, MIN_WAVES) void pearson_split_kernel(const float* const* __restrict__ members,
                                                                       const float* __restrict__ prep,
                                                                       float* __restrict__ out, uint32_t num_voxels,
                                                                       int cs) {
    static_assert(R % 2 == 0 && L % 2 == 0 && PAD % 2 == 0 && 64 % G == 0, "slots are handled in pairs");
    constexpr int S = R + L;        // slots per lane
    constexpr int VW = 64 / G;      // voxels per wave
    constexpr int kSure = S - PAD;  // slots below are members in every lane group
    static_assert(kSure >= 0 && G * S <= kPrepZeroFilled, "a_e is zero-filled up to kPrepZeroFilled");
    extern __shared__ float tail_dyn[];  // L rows of 256 floats: slot R + t of thread x is tail[t][x]
    float(*tail)[256] = reinterpret_cast<float(*)[256]>(tail_dyn);
    const int lane = int(threadIdx.x) & 63;
    const int g = lane / VW;
    const uint32_t v0 = (blockIdx.x * 4u + (threadIdx.x >> 6)) * uint32_t(VW) + uint32_t(lane % VW);
    const uint32_t byte_offset = v0 * 4u, bytes = num_voxels * 4u;  // lanes past the end read 0 and store nothing
    // slot i of this lane is a member iff i < mine.  (Laundered before each phase that tests it: left alone the compiler
    // evaluates all PAD tests once and keeps them as SGPR pairs across the kernel, which spill into VGPR lanes.)
    int mine = cs - g * S;
    const auto is_member = [&mine](int i) { return i < kSure || i < mine; };
    f2 y[R / 2];
    // the LDS tail first (global_load_lds: memory -> LDS without registers; lane l of the wave lands at row base + 4 l):
    // loads return in order, so by the time the register loads issued below have been waited for these are done too
    if constexpr (L > 0) {
        const int wave_first = int(threadIdx.x) & ~63;
        const uint32_t v_safe = v0 < num_voxels ? v0 : num_voxels - 1u;  // no descriptor bounds on this path
#pragma unroll
        for (int gg = 0; gg < G; gg++) {
            if (g == gg) {
#pragma unroll
                for (int t = 0; t < L; t++) {
                    const int e = gg * S + R + t;
                    if (gg < G - 1 || R + t < kSure || e < cs) {
                        typedef const float __attribute__((address_space(1)))* gptr_t;
                        typedef float __attribute__((address_space(3)))* lptr_t;
                        __builtin_amdgcn_global_load_lds((gptr_t)(members[e] + v_safe), (lptr_t)&tail[t][wave_first], 4, 0,
                                                         kAuxNonTemporal);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int gg = 0; gg < G; gg++) {
        if (g == gg) {  // this group's members, under its exec mask
#pragma unroll
            for (int i = 0; i < R; i++) {
                const int e = gg * S + i;
                float v = 0.0f;
                if (gg < G - 1 || i < kSure) {
                    v = load_member_nt(members[e], bytes, byte_offset);
                } else if (e < cs) {  // uniform branch around a load that may be padding
                    v = load_member_nt(members[e], bytes, byte_offset);
                }
                y[i / 2][i % 2] = v;
            }
        }
    }
    const float n = float(cs);
    const float invN = 1.0f / n;
    const float invNm1 = 1.0f / (n - 1.0f);
    const int last_group_lane = (G - 1) * VW + lane % VW;  // where a pass's result ends up for this lane's voxel
    // ---- pass 1: meanY += invN * y_e
    float m = 0.0f;
#pragma unroll
    for (int gg = 0; gg < G; gg++) {
        if (gg > 0) m = from_lane(m, lane - VW);
        // laundered per stage: left alone the compiler computes the products once and keeps all S of them for the
        // other stages (spills)
        f2 scale = {invN, invN};
        asm volatile("" : "+v"(scale));
#pragma unroll
        for (int k = 0; k < R / 2; k++) {
            const f2 t = scale * y[k];
            m += t[0];
            m += t[1];
            if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (L > 0) {
            if (gg == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the tail has landed (see above)
            asm volatile("" : "+v"(mine));
#pragma unroll
            for (int t = 0; t < L; t += 2) {
                f2 v = {tail[t][threadIdx.x], tail[t + 1][threadIdx.x]};
                if (R + t >= kSure) {  // a padded row was not loaded: whatever the row holds is not a member value
                    if (!is_member(R + t)) v[0] = 0.0f;
                    if (!is_member(R + t + 1)) v[1] = 0.0f;
                }
                const f2 p = scale * v;
                m += p[0];
                m += p[1];
                if ((t & 6) == 6) __builtin_amdgcn_sched_barrier(0);  // (else all L rows are read up front)
            }
        }
    }
    const float meanY = from_lane(m, last_group_lane);
    // ---- deviations in place (needed again, bit-identically, by pass 3)
    {
        const f2 mean2 = {meanY, meanY};
        asm volatile("" : "+v"(mine));
#pragma unroll
        for (int k = 0; k < R / 2; k++) {
            f2 d = y[k] - mean2;
            if (2 * k >= kSure) {
                if (!is_member(2 * k)) d[0] = 0.0f;
                if (!is_member(2 * k + 1)) d[1] = 0.0f;
            }
            y[k] = d;
            if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (L > 0) {
            asm volatile("" : "+v"(mine));
#pragma unroll
            for (int t = 0; t < L; t++) {
                float d = tail[t][threadIdx.x] - meanY;
                if (R + t >= kSure && !is_member(R + t)) d = 0.0f;
                tail[t][threadIdx.x] = d;
                if ((t & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    // ---- pass 2: varY += (invNm1 * d_e) * d_e
    float var = 0.0f;
#pragma unroll
    for (int gg = 0; gg < G; gg++) {
        if (gg > 0) var = from_lane(var, lane - VW);
        f2 scale = {invNm1, invNm1};
        asm volatile("" : "+v"(scale));
#pragma unroll
        for (int k = 0; k < R / 2; k++) {
            const f2 t = (scale * y[k]) * y[k];
            var += t[0];
            var += t[1];
            if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (L > 0) {
#pragma unroll
            for (int t = 0; t < L; t += 2) {
                const f2 d = {tail[t][threadIdx.x], tail[t + 1][threadIdx.x]};
                const f2 p = (scale * d) * d;
                var += p[0];
                var += p[1];
                if ((t & 6) == 6) __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    const float sdY = sqrtf(from_lane(var, last_group_lane));
    // ---- pass 3: r += a_e * (d_e / sdY)
    float r = 0.0f;
    // exact_div needs sd in [2^-60, 2^60] and every non-zero deviation >= 2^-100 in magnitude (crf_exact_div.h).
    // exact_div_guard() infers the latter from |mean| >= 2^-70; a wave in which that fails -- a mean that is exactly 0
    // is enough, and the benchmark's box ensemble has such voxels at 512 members -- looks at its deviations themselves
    // before it gives up the exact path, whose alternative is expensive here (see the else branch).
    bool exact = exact_div_guard(meanY, sdY);
    constexpr bool kSecondLook = R + L < 304;  // (in the 304-slot instantiation it costs 0.3 KB of scratch per lane)
    if (kSecondLook && !__all(exact)) {
        uint32_t smallest = 0xFFFFFFFFu;  // min over the slots of (bits of |d|) - 1: a zero wraps to the maximum
#pragma unroll
        for (int k = 0; k < R / 2; k++) {
            smallest = min(smallest, (__float_as_uint(y[k][0]) & 0x7FFFFFFFu) - 1u);
            smallest = min(smallest, (__float_as_uint(y[k][1]) & 0x7FFFFFFFu) - 1u);
            if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (L > 0) {
#pragma unroll
            for (int t = 0; t < L; t++) {
                smallest = min(smallest, (__float_as_uint(tail[t][threadIdx.x]) & 0x7FFFFFFFu) - 1u);
                if ((t & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
        }
        // (a NaN or infinite member makes the mean and therefore sd NaN: the range test fails)
        exact = sdY >= 0x1p-60f && sdY <= 0x1p60f && smallest >= __float_as_uint(0x1p-100f) - 1u;
        // Two kinds of voxels whose result is NaN on either path, so they need not drag their wave onto the slow one --
        // and they come in whole regions in real ensembles (missing values, masks): a NaN mean (some member is NaN:
        // every deviation is NaN), and sd = 0 with every deviation exactly 0 (all members equal, e.g. a zero mask:
        // the exact path computes 0 * (1 / 0) = NaN where the division gives 0 / 0 = NaN).
        exact = exact || meanY != meanY || (sdY == 0.0f && smallest == 0xFFFFFFFFu);
    }
    if (__all(exact)) {  // exact quotients through one reciprocal per voxel
        const float rcp = 1.0f / sdY;
        const f2 rcp2 = {rcp, rcp}, sd2 = {sdY, sdY};
#pragma unroll
        for (int k = 0; k < R / 2; k++) {  // exact_div in place, two slots at a time
            const f2 q0 = y[k] * rcp2;
            const f2 rem = __builtin_elementwise_fma(-q0, sd2, y[k]);
            y[k] = __builtin_elementwise_fma(rem, rcp2, q0);
            if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (L > 0) {
#pragma unroll
            for (int t = 0; t < L; t++) {
                tail[t][threadIdx.x] = exact_div(tail[t][threadIdx.x], sdY, rcp);
                if ((t & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int gg = 0; gg < G; gg++) {
            if (gg > 0) r = from_lane(r, lane - VW);
#pragma unroll
            for (int k = 0; k < R / 2; k++) {
                const f2 a = {prep[gg * S + 2 * k], prep[gg * S + 2 * k + 1]};  // the stage's group decides: wave-uniform
                const f2 t = a * y[k];
                r += t[0];
                r += t[1];
                if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (L > 0) {
#pragma unroll
                for (int t = 0; t < L; t += 2) {
                    const f2 a = {prep[gg * S + R + t], prep[gg * S + R + t + 1]};
                    const f2 q = {tail[t][threadIdx.x], tail[t + 1][threadIdx.x]};
                    const f2 p = a * q;
                    r += p[0];
                    r += p[1];
                    if ((t & 6) == 6) __builtin_amdgcn_sched_barrier(0);  // (else all L rows are read up front)
                }
            }
        }
    } else if (g == G - 1 && v0 < num_voxels) {
        // A constant voxel (sd = 0) or a tiny mean somewhere in the wave: plain divisions.  The storing lanes redo pass 3
        // from memory (the lines are still in L2), 16 or 8 members per step with their loads in flight together; y_e - meanY is
        // recomputed from the same operands: the same float.  (A second unrolled body over y[] -- quotients in place, or
        // taken on the fly per stage -- costs the whole kernel its register allocation: 0.9-2 KB of scratch per lane;
        // in groups of 8 slots under a uniform branch still 150-320 B.)
        constexpr int kStep = G == 2 ? 16 : 8;  // (16 live values cost the four-lane instantiations 0.1-0.4 KB of scratch)
        int e = 0;
#pragma unroll 1
        for (; e + kStep <= cs; e += kStep) {
            float v[kStep];
#pragma unroll
            for (int i = 0; i < kStep; i++) v[i] = load_member(members[e + i], byte_offset);
#pragma unroll
            for (int i = 0; i < kStep; i++) r += prep[e + i] * ((v[i] - meanY) / sdY);
        }
#pragma unroll 1
        for (; e < cs; e++) r += prep[e] * ((load_member(members[e], byte_offset) - meanY) / sdY);
    }
    if (g == G - 1 && v0 < num_voxels) store_result_nt(out + v0, r);
}

// ---------------------------------------------------------------------------------------------------------
// Members in a narrow native format (crf_internal.h: u8, u16, f16): pearson_reg_kernel with the members kept as they
// are in memory.  One lane owns the VPL = 4 (8-bit) or 2 (16-bit) consecutive voxels of one dword, so a wave's load of
// one member is still 256 contiguous bytes, all cs loads are issued before the first use, and the cs raw dwords stay in
// registers for the three passes: cs VGPRs for 2 or 4 voxels where the fp32 kernel needs cs per voxel.  Each pass
// converts on use -- y_e - meanY recomputed in pass 3 from the same operands is the same float as the one pass 2 saw.
// The integer formats' value x / 255.0f, x / 65535.0f is exact_div (crf_exact_div.h) with a compile-time reciprocal: x is
// an integer below 2^16 and the denominator a constant inside [2^-60, 2^60], its preconditions.  Everything is done
// two voxels at a time in packed fp32 (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32: the same IEEE operation per element,
// contraction off), as in pearson_split_kernel; the sequential sums are one chain per voxel, element-wise.
// The caller passes `covered`, a multiple of VPL: no dword straddles the descriptor's end (a raw descriptor returns 0
// for the WHOLE dword then); launch_pearson_narrow gives the up to VPL - 1 voxels behind it to the tail kernel.
// Guarded slots (the last granule of a guarded instantiation) are stepped over in uniform branches, loads included: a
// skipped slot is the +0 that pearson_reg_kernel adds for it in every pass.
// ---------------------------------------------------------------------------------------------------------
// (narrow_vpl and narrow_pair: crf_device.h, shared with the sibling reductions of kernels_stats.hip)
template <int FMT, int CS_PAD, bool EXACT, int MIN_WAVES>
__global__ __launch_bounds__(256, MIN_WAVES) void pearson_narrow_kernel(const void* const* __restrict__ members,
                                                                        const float* __restrict__ prep,
                                                                        float* __restrict__ out, uint32_t covered,
                                                                        int cs, int out_vector) {
    static_assert(CS_PAD <= kPrepZeroFilled, "a_e is zero-filled up to kPrepZeroFilled");
    constexpr int VPL = narrow_vpl<FMT>(), P = VPL / 2;  // voxels, and pairs of voxels, per lane
    constexpr int kFirstGuarded = EXACT ? CS_PAD : CS_PAD - pad_granule(CS_PAD);
    // slot e is a member iff e < mine.  (Laundered before each pass: left alone the compiler evaluates the guarded slots'
    // tests once and keeps them as SGPR pairs across the kernel, which spill into VGPR lanes; see pearson_split_kernel.)
    int mine = cs;
    const auto is_member = [&mine](int e) { return e < kFirstGuarded || e < mine; };
    const uint32_t dword = blockIdx.x * 256 + threadIdx.x;
    const uint32_t v0 = dword * VPL;
    const uint32_t byte_offset = dword * 4u;
    const uint32_t bytes = covered / VPL * 4u;  // descriptor bound: lanes past the end read 0 and store nothing
    uint32_t w[CS_PAD];
#pragma unroll
    for (int e = 0; e < CS_PAD; e++) {
        w[e] = 0u;
        if (is_member(e)) {  // a uniform branch around each of the few guarded loads (they are the last loads issued)
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(members[e]), short(0), int(bytes), 0x00020000);
            w[e] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, int(byte_offset), 0, kAuxNonTemporal);
        }
    }
    const float n = float(cs);
    const float invN = 1.0f / n;
    const float invNm1 = 1.0f / (n - 1.0f);
    const f2 zero2 = {0.0f, 0.0f};
    // pass 1: meanY += invN * y_e
    f2 meanY[P];
#pragma unroll
    for (int p = 0; p < P; p++) meanY[p] = zero2;
    {
        const f2 scale = {invN, invN};
#pragma unroll
        for (int e = 0; e < CS_PAD; e++) {
#pragma unroll
            for (int p = 0; p < P; p++) {
                if (!is_member(e)) continue;  // uniform
                meanY[p] += scale * narrow_pair<FMT>(w[e], p);
            }
            if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // (else the conversions of many slots run ahead)
        }
    }
    // Laundered before each pass: left alone the compiler keeps the converted values of pass 1 for the later passes --
    // cs x VPL registers, the fp32 kernel's footprint, which is what this kernel exists to avoid.
    const auto launder = [&w, &mine]() {
#pragma unroll
        for (int e = 0; e < CS_PAD; e++) asm volatile("" : "+v"(w[e]));
        asm volatile("" : "+s"(mine));
    };
    launder();
    // pass 2: varY += (invNm1 * d_e) * d_e, d_e = y_e - meanY
    f2 varY[P];
#pragma unroll
    for (int p = 0; p < P; p++) varY[p] = zero2;
    {
        const f2 scale = {invNm1, invNm1};
#pragma unroll
        for (int e = 0; e < CS_PAD; e++) {
#pragma unroll
            for (int p = 0; p < P; p++) {
                if (!is_member(e)) continue;  // uniform
                const f2 d = narrow_pair<FMT>(w[e], p) - meanY[p];
                varY[p] += (scale * d) * d;
            }
            if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
    }
    launder();
    f2 sdY[P], r[P];
    bool guard = true;
#pragma unroll
    for (int p = 0; p < P; p++) {
        sdY[p] = f2{sqrtf(varY[p][0]), sqrtf(varY[p][1])};
        r[p] = zero2;
        guard = guard && exact_div_guard(meanY[p][0], sdY[p][0]) && exact_div_guard(meanY[p][1], sdY[p][1]);
    }
    // pass 3: r += a_e * (d_e / sdY)
    if (__all(guard)) {  // exact quotients through one reciprocal per voxel (crf_exact_div.h: exact_div)
        f2 rcp[P];
#pragma unroll
        for (int p = 0; p < P; p++) rcp[p] = f2{1.0f / sdY[p][0], 1.0f / sdY[p][1]};
#pragma unroll
        for (int e = 0; e < CS_PAD; e++) {
            const float a = prep[e];
            const f2 a2 = {a, a};
#pragma unroll
            for (int p = 0; p < P; p++) {
                if (!is_member(e)) continue;  // uniform
                const f2 d = narrow_pair<FMT>(w[e], p) - meanY[p];
                const f2 q0 = d * rcp[p];
                const f2 rem = __builtin_elementwise_fma(-q0, sdY[p], d);
                r[p] += a2 * __builtin_elementwise_fma(rem, rcp[p], q0);
            }
            if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
    } else {
#pragma unroll
        for (int e = 0; e < CS_PAD; e++) {
            const float a = prep[e];
#pragma unroll
            for (int p = 0; p < P; p++) {
                if (!is_member(e)) continue;  // uniform
                const f2 y = narrow_pair<FMT>(w[e], p);
#pragma unroll
                for (int i = 0; i < 2; i++) r[p][i] += a * ((y[i] - meanY[p][i]) / sdY[p][i]);
            }
            if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (v0 + VPL <= covered) {
        if (out_vector) {
            typedef float fv __attribute__((ext_vector_type(VPL)));
            fv v;
#pragma unroll
            for (int i = 0; i < VPL; i++) v[i] = r[i / 2][i % 2];
            __builtin_nontemporal_store(v, reinterpret_cast<fv*>(out + v0));
        } else {
#pragma unroll
            for (int i = 0; i < VPL; i++) store_result_nt(out + v0 + i, r[i / 2][i % 2]);
        }
    }
}

// the up to VPL - 1 voxels behind the last whole dword of the narrow members: one voxel per lane, three passes
template <int FMT>
__global__ __launch_bounds__(64) void pearson_narrow_tail_kernel(const void* const* __restrict__ members,
                                                                 const float* __restrict__ prep,
                                                                 float* __restrict__ out, size_t voxel_offset,
                                                                 size_t voxel_end, int cs) {
    const size_t v0 = voxel_offset + size_t(blockIdx.x) * 64 + threadIdx.x;
    if (v0 >= voxel_end) return;
    const float n = float(cs);
    const float invN = 1.0f / n;
    const float invNm1 = 1.0f / (n - 1.0f);
    float meanY = 0.0f;
    for (int e = 0; e < cs; e++) meanY += invN * narrow_value<FMT>(members[e], v0);
    float varY = 0.0f;
    for (int e = 0; e < cs; e++) {
        const float d = narrow_value<FMT>(members[e], v0) - meanY;
        varY += invNm1 * d * d;
    }
    const float sdY = sqrtf(varY);
    float r = 0.0f;
    for (int e = 0; e < cs; e++) r += prep[e] * ((narrow_value<FMT>(members[e], v0) - meanY) / sdY);
    store_result_nt(out + v0, r);
}

// ---------------------------------------------------------------------------------------------------------
// Symmetric field mode (CorrelationFieldMode::SEPARATE_SYMMETRIC, CorrelationMain.glsl:10-15): voxel v correlates
// the reference field's members at v with the query field's members at v -- computePearson2 on two arrays
// (Correlation.cpp:141-174), nothing to hoist.  2*cs loads per voxel (8*cs + 4 algorithmic bytes), both sides in
// registers.  Same guarded-slot scheme as pearson_reg_kernel.
// ---------------------------------------------------------------------------------------------------------
// REQ: pair-request mode (crf_compute_requests): item r works on request r = {xi, yi, zi, i, xj, yj, zj, j}
// (HEBChart.hpp:166-168), X = the members at voxel i, Y = the members at voxel j; default cache policy (requests
// revisit voxels); `requests`, `xs`, `ys`, `use_abs` are unused in field mode, where num_items = num_voxels.
// Which evaluations arrive here: two_vector_route.h.
template <int CS_PAD, bool EXACT, int MIN_WAVES, bool REQ = false>
__global__ __launch_bounds__(256, MIN_WAVES) void pearson_symmetric_kernel(const float* const* __restrict__ members_x,
                                                                           const float* const* __restrict__ members_y,
                                                                           float* __restrict__ out,
                                                                           uint32_t num_voxels, int cs,
                                                                           const uint32_t* __restrict__ requests,
                                                                           uint32_t num_items, int xs, int ys,
                                                                           int use_abs) {
    const auto is_member = [cs](int e) { return CRF_SLOT_IS_MEMBER(CS_PAD, EXACT, e, cs); };
    const uint32_t v0 = blockIdx.x * 256 + threadIdx.x;
    uint32_t offset_x, offset_y;
    lane_offsets<REQ>(RequestArgs{requests, xs, ys, use_abs}, v0, num_items, offset_x, offset_y);
    const uint32_t bytes = num_voxels * 4u;
    float x[CS_PAD], y[CS_PAD];
#pragma unroll
    for (int e = 0; e < CS_PAD; e++) {
        const int slot = is_member(e) ? e : cs - 1;
        const uint32_t off_x = is_member(e) ? offset_x : kOutOfRangeOffset;
        const uint32_t off_y = is_member(e) ? offset_y : kOutOfRangeOffset;
        x[e] = REQ ? load_member_cached(members_x[slot], bytes, off_x) : load_member_nt(members_x[slot], bytes, off_x);
        y[e] = REQ ? load_member_cached(members_y[slot], bytes, off_y) : load_member_nt(members_y[slot], bytes, off_y);
    }
    const float n = float(cs);
    const float invN = 1.0f / n;
    const float invNm1 = 1.0f / (n - 1.0f);
    float meanX = 0.0f, meanY = 0.0f;
#pragma unroll
    for (int e = 0; e < CS_PAD; e++) {
        meanX += invN * x[e];
        meanY += invN * y[e];
    }
    float varX = 0.0f, varY = 0.0f;
#pragma unroll
    for (int e = 0; e < CS_PAD; e++) {
        const float dx = is_member(e) ? x[e] - meanX : 0.0f;
        const float dy = is_member(e) ? y[e] - meanY : 0.0f;
        x[e] = dx;
        y[e] = dy;
        varX += invNm1 * dx * dx;
        varY += invNm1 * dy * dy;
    }
    const float sdX = sqrtf(varX), sdY = sqrtf(varY);
    float r = 0.0f;
    if (__all(exact_div_guard(meanX, sdX) && exact_div_guard(meanY, sdY))) {
        const float rcpX = 1.0f / sdX, rcpY = 1.0f / sdY;
#pragma unroll
        for (int e = 0; e < CS_PAD; e++)
            r += (invNm1 * exact_div(x[e], sdX, rcpX)) * exact_div(y[e], sdY, rcpY);
    } else {
#pragma unroll
        for (int e = 0; e < CS_PAD; e++)
            r += (invNm1 * (is_member(e) ? x[e] / sdX : 0.0f)) * (is_member(e) ? y[e] / sdY : 0.0f);
    }
    if (REQ && use_abs) r = fabsf(r);
    if (v0 < num_items) store_result_nt(out + v0, r);
}

// ---------------------------------------------------------------------------------------------------------
// Symmetric field mode on two fields in ONE narrow native format: pearson_symmetric_kernel with both fields kept as they
// are in memory, in the register scheme of pearson_narrow_kernel.  One lane owns the VPL voxels of one dword of every
// member of both fields; all 2 cs raw-buffer dword loads are issued before the first use and the 2 cs raw dwords stay in
// registers for the three passes (2 cs VGPRs for 2 or 4 voxels where the fp32 kernel needs 2 cs per voxel); each pass
// converts on use, two voxels at a time in packed fp32, and the dwords are laundered between the passes so that the
// compiler does not keep converted values.  2 cs e + 4 algorithmic bytes per voxel (e = element size).  The arithmetic
// is pearson_symmetric_kernel's in its order; a skipped padded slot is the +0 that kernel adds for it in every pass (its
// sums start at +0 and can never become -0).  The division branch is taken per wave as there, over VPL times the voxels:
// exact_div equals the plain quotient wherever its guard holds, so which waves take which branch does not show.
// `covered` as for pearson_narrow_kernel; launch_pearson_symmetric_narrow gives the rest to the tail kernel.
// ---------------------------------------------------------------------------------------------------------
template <int FMT, int CS_PAD, bool EXACT, int MIN_WAVES>
__global__ __launch_bounds__(256, MIN_WAVES) void pearson_symmetric_narrow_kernel(
    const void* const* __restrict__ members_x, const void* const* __restrict__ members_y, float* __restrict__ out,
    uint32_t covered, int cs, int out_vector) {
    constexpr int VPL = narrow_vpl<FMT>(), P = VPL / 2;  // voxels, and pairs of voxels, per lane
    constexpr int kFirstGuarded = EXACT ? CS_PAD : CS_PAD - pad_granule(CS_PAD);
    // a scheduling region is 2 pairs of voxels of each field: one slot (8-bit) or two (16-bit).  (Four slots, as in
    // pearson_narrow_kernel, are 4 or 8 chains per field here, and the scheduler interleaves them all.)
    constexpr int kBarrierMask = P == 2 ? 0 : 1;
    int mine = cs;  // slot e is a member iff e < mine (laundered before each pass: see pearson_narrow_kernel)
    const auto is_member = [&mine](int e) { return e < kFirstGuarded || e < mine; };
    const uint32_t dword = blockIdx.x * 256 + threadIdx.x;
    const uint32_t v0 = dword * VPL;
    const uint32_t byte_offset = dword * 4u;
    const uint32_t bytes = covered / VPL * 4u;  // descriptor bound: lanes past the end read 0 and store nothing
    uint32_t wx[CS_PAD], wy[CS_PAD];
    // (unroll(full) on the slot loops: `#pragma unroll` gives up above a size that the 8-bit bodies reach at 112 slots, and a
    // loop left rolled indexes wx / wy dynamically, which moves them to scratch)
#pragma clang loop unroll(full)
    for (int e = 0; e < CS_PAD; e++) {
        wx[e] = wy[e] = 0u;
        if (is_member(e)) {  // a uniform branch around each of the few guarded loads (they are the last loads issued)
            const auto rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(members_x[e]), short(0), int(bytes), 0x00020000);
            const auto ry = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(members_y[e]), short(0), int(bytes), 0x00020000);
            wx[e] = __builtin_amdgcn_raw_buffer_load_b32(rx, int(byte_offset), 0, kAuxNonTemporal);
            wy[e] = __builtin_amdgcn_raw_buffer_load_b32(ry, int(byte_offset), 0, kAuxNonTemporal);
        }
    }
    const float n = float(cs);
    const float invN = 1.0f / n;
    const float invNm1 = 1.0f / (n - 1.0f);
    const f2 zero2 = {0.0f, 0.0f};
    // Laundered before each pass as in pearson_narrow_kernel.  The sums of the pass that ends are pinned first, so that the
    // pass is over before the first dword is laundered (a chain of it moved behind the launder would keep both
    // generations of the dwords alive).
    const auto launder = [&wx, &wy, &mine](f2 (&sum_x)[P], f2 (&sum_y)[P]) {
#pragma unroll
        for (int p = 0; p < P; p++) asm volatile("" : "+v"(sum_x[p]), "+v"(sum_y[p]));
#pragma clang loop unroll(full)
        for (int e = 0; e < CS_PAD; e++) {
            asm volatile("" : "+v"(wx[e]));
            asm volatile("" : "+v"(wy[e]));
        }
        asm volatile("" : "+s"(mine));
    };
    // pass 1: mean += invN * v_e
    f2 meanX[P], meanY[P];
#pragma unroll
    for (int p = 0; p < P; p++) meanX[p] = meanY[p] = zero2;
    {
        const f2 scale = {invN, invN};
#pragma clang loop unroll(full)
        for (int e = 0; e < CS_PAD; e++) {
#pragma unroll
            for (int p = 0; p < P; p++) {
                if (!is_member(e)) continue;  // uniform
                meanX[p] += scale * narrow_pair<FMT>(wx[e], p);
                meanY[p] += scale * narrow_pair<FMT>(wy[e], p);
            }
            if ((e & kBarrierMask) == kBarrierMask) __builtin_amdgcn_sched_barrier(0);  // (else the conversions of many slots run ahead)
        }
    }
    launder(meanX, meanY);
    // pass 2: var += (invNm1 * d_e) * d_e, d_e = v_e - mean
    f2 varX[P], varY[P];
#pragma unroll
    for (int p = 0; p < P; p++) varX[p] = varY[p] = zero2;
    {
        const f2 scale = {invNm1, invNm1};
#pragma clang loop unroll(full)
        for (int e = 0; e < CS_PAD; e++) {
#pragma unroll
            for (int p = 0; p < P; p++) {
                if (!is_member(e)) continue;  // uniform
                const f2 dx = narrow_pair<FMT>(wx[e], p) - meanX[p];
                const f2 dy = narrow_pair<FMT>(wy[e], p) - meanY[p];
                varX[p] += (scale * dx) * dx;
                varY[p] += (scale * dy) * dy;
            }
            if ((e & kBarrierMask) == kBarrierMask) __builtin_amdgcn_sched_barrier(0);
        }
    }
    launder(varX, varY);
    f2 sdX[P], sdY[P], r[P];
    int guard = 1;  // (no short circuit: nothing of a pass is to be sunk behind a branch)
#pragma unroll
    for (int p = 0; p < P; p++) {
        sdX[p] = f2{sqrtf(varX[p][0]), sqrtf(varX[p][1])};
        sdY[p] = f2{sqrtf(varY[p][0]), sqrtf(varY[p][1])};
        r[p] = zero2;
#pragma unroll
        for (int i = 0; i < 2; i++)
            guard &= int(exact_div_guard(meanX[p][i], sdX[p][i])) & int(exact_div_guard(meanY[p][i], sdY[p][i]));
    }
    // pass 3: r += (invNm1 * (dx_e / sdX)) * (dy_e / sdY).  The choice between the exact quotients through one reciprocal per
    // voxel and side (crf_exact_div.h: exact_div) and the plain divisions (a constant voxel, sd = 0, or a tiny mean somewhere
    // in the wave) is a uniform branch inside every slot, behind the conversions: written as two loops, both begin with the
    // same conversions, the compiler hoists them above the branch, all of them at once, and the kernel is back at the
    // fp32 kernel's footprint.  (The flag is laundered per slot so that the branches are not threaded into two loops again.)
    int exact = __builtin_amdgcn_readfirstlane(__all(guard) ? 1 : 0);
    f2 rcpX[P], rcpY[P];
#pragma unroll
    for (int p = 0; p < P; p++) {
        rcpX[p] = f2{1.0f / sdX[p][0], 1.0f / sdX[p][1]};
        rcpY[p] = f2{1.0f / sdY[p][0], 1.0f / sdY[p][1]};
    }
    const f2 scale3 = {invNm1, invNm1};
#pragma clang loop unroll(full)
    for (int e = 0; e < CS_PAD; e++) {
        if (!is_member(e)) continue;  // uniform
        f2 dx[P], dy[P];
#pragma unroll
        for (int p = 0; p < P; p++) {
            dx[p] = narrow_pair<FMT>(wx[e], p) - meanX[p];
            dy[p] = narrow_pair<FMT>(wy[e], p) - meanY[p];
        }
        asm volatile("" : "+s"(exact));
        if (exact) {
#pragma unroll
            for (int p = 0; p < P; p++) {
                const f2 qx0 = dx[p] * rcpX[p], qy0 = dy[p] * rcpY[p];
                const f2 remx = __builtin_elementwise_fma(-qx0, sdX[p], dx[p]);
                const f2 remy = __builtin_elementwise_fma(-qy0, sdY[p], dy[p]);
                const f2 qx = __builtin_elementwise_fma(remx, rcpX[p], qx0);
                const f2 qy = __builtin_elementwise_fma(remy, rcpY[p], qy0);
                r[p] += (scale3 * qx) * qy;
            }
        } else {
#pragma unroll
            for (int p = 0; p < P; p++)
#pragma unroll
                for (int i = 0; i < 2; i++) r[p][i] += (invNm1 * (dx[p][i] / sdX[p][i])) * (dy[p][i] / sdY[p][i]);
        }
        // (pinned per slot: the additions are common to both arms, and left alone the compiler moves them all behind the last
        // slot and keeps every slot's products until then)
#pragma unroll
        for (int p = 0; p < P; p++) asm volatile("" : "+v"(r[p]));
    }
    if (v0 + VPL <= covered) {
        if (out_vector) {
            typedef float fv __attribute__((ext_vector_type(VPL)));
            fv v;
#pragma unroll
            for (int i = 0; i < VPL; i++) v[i] = r[i / 2][i % 2];
            __builtin_nontemporal_store(v, reinterpret_cast<fv*>(out + v0));
        } else {
#pragma unroll
            for (int i = 0; i < VPL; i++) store_result_nt(out + v0 + i, r[i / 2][i % 2]);
        }
    }
}

// the up to VPL - 1 voxels behind the last whole dword of the two narrow fields: one voxel per lane, three passes
template <int FMT>
__global__ __launch_bounds__(64) void pearson_symmetric_narrow_tail_kernel(const void* const* __restrict__ members_x,
                                                                           const void* const* __restrict__ members_y,
                                                                           float* __restrict__ out, size_t voxel_offset,
                                                                           size_t voxel_end, int cs) {
    const size_t v0 = voxel_offset + size_t(blockIdx.x) * 64 + threadIdx.x;
    if (v0 >= voxel_end) return;
    const float n = float(cs);
    const float invN = 1.0f / n;
    const float invNm1 = 1.0f / (n - 1.0f);
    float meanX = 0.0f, meanY = 0.0f;
    for (int e = 0; e < cs; e++) {
        meanX += invN * narrow_value<FMT>(members_x[e], v0);
        meanY += invN * narrow_value<FMT>(members_y[e], v0);
    }
    float varX = 0.0f, varY = 0.0f;
    for (int e = 0; e < cs; e++) {
        const float dx = narrow_value<FMT>(members_x[e], v0) - meanX;
        const float dy = narrow_value<FMT>(members_y[e], v0) - meanY;
        varX += invNm1 * dx * dx;
        varY += invNm1 * dy * dy;
    }
    const float sdX = sqrtf(varX), sdY = sqrtf(varY);
    float r = 0.0f;
    for (int e = 0; e < cs; e++)
        r += (invNm1 * ((narrow_value<FMT>(members_x[e], v0) - meanX) / sdX)) *
             ((narrow_value<FMT>(members_y[e], v0) - meanY) / sdY);
    store_result_nt(out + v0, r);
}

// ---------------------------------------------------------------------------------------------------------
// Streaming fallback for any cs (three passes re-reading the members; the second and third mostly hit L2/MALL) and
// for the ragged tail of the grid.  One voxel per lane, bounds-checked.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pearson_stream_kernel(const float* const* __restrict__ members,
                                                             const float* __restrict__ prep,
                                                             float* __restrict__ out, size_t voxel_offset,
                                                             size_t voxel_end, int cs) {
    const size_t v0 = voxel_offset + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (v0 >= voxel_end) return;
    const float n = float(cs);
    const float invN = 1.0f / n;
    const float invNm1 = 1.0f / (n - 1.0f);
    float meanY = 0.0f;
    for (int e = 0; e < cs; e++) meanY += invN * members[e][v0];
    float varY = 0.0f;
    for (int e = 0; e < cs; e++) {
        const float d = members[e][v0] - meanY;
        varY += invNm1 * d * d;
    }
    const float sdY = sqrtf(varY);
    float r = 0.0f;
    for (int e = 0; e < cs; e++) r += prep[e] * ((members[e][v0] - meanY) / sdY);
    store_result_nt(out + v0, r);
}

// ---------------------------------------------------------------------------------------------------------
// Member counts beyond the register kernels (the reference's own synthetic data set has 1000 members): the three passes
// re-read the voxel's values, 3x the algorithmic bytes.  One wave owns 64 voxels at a time and walks the members in
// chunks of 64 with all 64 loads of a chunk in flight; measured at 128x128x64x1000: 2.12 ms = 5.9 TB/s moved (2.0 TB/s
// of algorithmic bytes), HBM-bound, vs 3.42 ms for the plain streaming kernel below.  A deliberately small persistent
// grid (512-1024 waves, so that the lines of pass 1 would still be in the 256 MiB Infinity Cache for passes 2 and 3)
// was measured too and is slower -- a wave moves only ~4 GB/s when it alternates load and compute phases, so the grid
// must fill the chip (3.6 ms at 1024 waves, 2.3 ms at 2048, flat from 4096; profiles/tuning_r01.md).
// Arithmetic: the same sequential fp32 passes as everywhere else.
// ---------------------------------------------------------------------------------------------------------
constexpr int kBigWaves = 8192;  // persistent beyond this many 64-voxel tiles

// One chunk = 64 members: the 64 member pointers are fetched by ONE coalesced vector load (lane l takes member e0 + l)
// and handed to the wave one at a time with v_readlane -- no dependent scalar-load chain in front of the 64 buffer
// loads, which all go out back to back (vmcnt allows 63 in flight).
__device__ __forceinline__ void load_chunk_64(const float* const* __restrict__ members, int e0, int cs, uint32_t bytes,
                                              uint32_t byte_offset, float (&buf)[64]) {
    const int mine = e0 + int(threadIdx.x) < cs ? e0 + int(threadIdx.x) : cs - 1;
    const uint64_t ptr = reinterpret_cast<uint64_t>(members[mine]);
    const uint32_t ptr_lo = uint32_t(ptr), ptr_hi = uint32_t(ptr >> 32);
#pragma unroll
    for (int i = 0; i < 64; i++) {
        const uint64_t base = (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(ptr_hi), i))) << 32) |
                              uint64_t(uint32_t(__builtin_amdgcn_readlane(int(ptr_lo), i)));
        buf[i] = load_member_cached(reinterpret_cast<const float*>(base), bytes,
                                    e0 + i < cs ? byte_offset : kOutOfRangeOffset);
    }
}

__global__ __launch_bounds__(64) void pearson_big_kernel(const float* const* __restrict__ members,
                                                         const float* __restrict__ prep, float* __restrict__ out,
                                                         uint32_t num_voxels, int cs) {
    const uint32_t bytes = num_voxels * 4u;
    const float n = float(cs);
    const float invN = 1.0f / n;
    const float invNm1 = 1.0f / (n - 1.0f);
    const uint32_t tiles = (num_voxels + 63u) / 64u;
#pragma unroll 1
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t v0 = t * 64u + threadIdx.x;
        const uint32_t byte_offset = v0 * 4u;  // lanes past the end read 0 and store nothing
        float buf[64];
        float meanY = 0.0f;
#pragma unroll 1
        for (int e0 = 0; e0 < cs; e0 += 64) {
            load_chunk_64(members, e0, cs, bytes, byte_offset, buf);
#pragma unroll
            for (int i = 0; i < 64; i++) meanY += invN * buf[i];  // a padded slot adds invN * 0 = +0
        }
        float varY = 0.0f;
#pragma unroll 1
        for (int e0 = 0; e0 < cs; e0 += 64) {
            load_chunk_64(members, e0, cs, bytes, byte_offset, buf);
#pragma unroll
            for (int i = 0; i < 64; i++) {
                const float d = e0 + i < cs ? buf[i] - meanY : 0.0f;
                varY += invNm1 * d * d;
            }
        }
        const float sdY = sqrtf(varY);
        float r = 0.0f;
#pragma unroll 1
        for (int e0 = 0; e0 < cs; e0 += 64) {
            load_chunk_64(members, e0, cs, bytes, byte_offset, buf);
            const float a_mine = e0 + int(threadIdx.x) < cs ? prep[e0 + threadIdx.x] : 0.0f;  // a_e, one per lane
#pragma unroll
            for (int i = 0; i < 64; i++) {
                const float a = __uint_as_float(uint32_t(__builtin_amdgcn_readlane(int(__float_as_uint(a_mine)), i)));
                if (e0 + i < cs) r += a * ((buf[i] - meanY) / sdY);
            }
        }
        if (v0 < num_voxels) store_result_nt(out + v0, r);
    }
}

__global__ void fill_kernel(float* __restrict__ out, size_t n, float value) {
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) out[i] = value;
}

namespace {

template <int CS_PAD, int VPT>
void launch_reg(const float* const* d_members, const float* d_prep, float* d_out, size_t blocks, size_t num_voxels,
                int cs, hipStream_t s) {
    // occupancy request: data registers are CS_PAD*VPT per lane; ask for the waves/SIMD that budget allows.
    // 161..224 values per lane: capped at 256 registers (two waves per SIMD) the kernel is 1.2x faster than with 256
    // VGPRs + AGPRs at one wave per SIMD, which cannot overlap its load and compute phases -- measured at 512x512x128:
    // 224 members 5.60 -> 4.63 ms (81 % of the HBM peak), 200 (guarded 224) 5.61 -> 4.53 ms.
    constexpr int kData = CS_PAD * VPT;
    constexpr int kMinWaves = kData <= 64 ? 4 : kData <= 128 ? 2 : kData <= 160 ? 1 : 2;
    if (cs == CS_PAD)
        hipLaunchKernelGGL((pearson_reg_kernel<CS_PAD, VPT, true, kMinWaves, false>), dim3(unsigned(blocks)), dim3(256),
                           0, s, d_members, d_prep, d_out, uint32_t(num_voxels), cs, PackedMembers{});
    else
        hipLaunchKernelGGL((pearson_reg_kernel<CS_PAD, VPT, false, kMinWaves, false>), dim3(unsigned(blocks)),
                           dim3(256), 0, s, d_members, d_prep, d_out, uint32_t(num_voxels), cs, PackedMembers{});
}

// the packed form: 17..128 members, one voxel per lane.  Up to 64 slots it is held to 96 VGPRs (five waves per SIMD,
// as the raw 64-member kernel's 93).
template <int CS_PAD>
void launch_reg_packed(const float* const* d_members, const float* d_prep, float* d_out, size_t num_voxels, int cs,
                       const PackedMembers& packed, hipStream_t s) {
    constexpr int kMinWaves = CS_PAD <= 64 ? 5 : 2;
    const unsigned blocks = unsigned((num_voxels + 255) / 256);
    if (cs == CS_PAD)
        hipLaunchKernelGGL((pearson_reg_kernel<CS_PAD, 1, true, kMinWaves, true>), dim3(blocks), dim3(256), 0, s,
                           d_members, d_prep, d_out, uint32_t(num_voxels), cs, packed);
    else
        hipLaunchKernelGGL((pearson_reg_kernel<CS_PAD, 1, false, kMinWaves, true>), dim3(blocks), dim3(256), 0, s,
                           d_members, d_prep, d_out, uint32_t(num_voxels), cs, packed);
}

template <int CS_PAD>
void launch_reg_vpt(int vpt, const float* const* d_members, const float* d_prep, float* d_out, size_t blocks,
                    size_t num_voxels, int cs, hipStream_t s) {
    if constexpr (CS_PAD <= 16) {
        if (vpt == 2) return launch_reg<CS_PAD, 2>(d_members, d_prep, d_out, blocks, num_voxels, cs, s);
    }
    return launch_reg<CS_PAD, 1>(d_members, d_prep, d_out, blocks, num_voxels, cs, s);
}

// A per-voxel kernel with `rows` rows of 256 floats of dynamic LDS per block (pearson_reg_lds_kernel,
// pearson_split_kernel).
struct LdsKernel {
    void (*kernel)(const float* const*, const float*, float*, uint32_t, int);
    int rows;
};

// pearson_split_kernel at two waves per SIMD; the slots per lane are rounded up to a multiple of 16, so up to 16 * G of
// them can be padding
template <int R, int L, int G>
LdsKernel split_kernel() {
    return {pearson_split_kernel<R, L, G, 16 * G, 2>, L};
}
template <int R, int L>
LdsKernel split_kernel(int lanes) {
    return lanes == 2 ? split_kernel<R, L, 2>() : split_kernel<R, L, 4>();
}

// pearson_split_kernel for `slots` register + LDS slots per lane (160..304)
LdsKernel split_kernel_for(int slots, int lanes) {
    switch (slots) {
        case 160: return split_kernel<160, 0>(lanes);  // 289..320 or 577..640 members
        case 176: return split_kernel<176, 0>(lanes);
        case 192: return split_kernel<192, 0>(lanes);
        case 208: return split_kernel<208, 0>(lanes);
        // beyond 208 slots the rest goes to LDS rows: with 224 register slots the allocation is at its edge and
        // whether 16 B or 0.5 KB of scratch come out depends on details of the rare path (measured: 448 members
        // 72 % of the peak without, 63 % with 52 B of scratch)
        case 224: return split_kernel<208, 16>(lanes);
        case 240: return split_kernel<216, 24>(lanes);
        case 256: return split_kernel<216, 40>(lanes);
        case 272: return split_kernel<216, 56>(lanes);
        case 288: return split_kernel<216, 72>(lanes);
        // 304 slots, four lanes only (1153..1216 members): 80 KB of LDS per block, still two blocks per CU
        // (320 slots = 224 + 96 LDS rows: one block per CU, 17-32 % of the peak -- not instantiated)
        default: return split_kernel<224, 80, 4>();
    }
}

hipError_t launch_lds(LdsKernel k, size_t blocks, const float* const* d_members, const float* d_prep, float* d_out,
                      size_t num_voxels, int cs, hipStream_t s) {
    const size_t bytes = size_t(k.rows) * 256 * sizeof(float);
    if (bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k.kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
        if (e != hipSuccess) return e;
    }
    if (blocks > 0)
        hipLaunchKernelGGL(k.kernel, dim3(unsigned(blocks)), dim3(256), bytes, s, d_members, d_prep, d_out,
                           uint32_t(num_voxels), cs);
    return hipSuccess;
}

}  // namespace

__global__ void abs_kernel(float* __restrict__ out, size_t n) {
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) out[i] = fabsf(out[i]);  // NaN stays NaN
}

hipError_t launch_abs(float* d_out, size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(abs_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, d_out, n);
    return hipGetLastError();
}

hipError_t launch_fill(float* d_out, size_t n, float value, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(fill_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, d_out, n, value);
    return hipGetLastError();
}

namespace {
template <int CS_PAD>
void launch_two_vector(const TwoVectorJob& j, hipStream_t s) {
    // 2 * CS_PAD values per lane.  Two waves under a 256-register cap pay off at 96 (90 members: 2.55 -> 2.04 ms) but
    // not with the 72-670 B of scratch of the 112 / 128 instantiations (128 members: 3.92 -> 5.09 ms); request mode
    // (cached loads, the guarded instantiations only) takes two waves at 80 as well
    constexpr int kFieldWaves = CS_PAD <= 32 ? 4 : (CS_PAD <= 64 || CS_PAD == 96 ? 2 : 1);
    constexpr int kRequestWaves = CS_PAD <= 32 ? 4 : (CS_PAD <= 96 ? 2 : 1);
    const auto kernel = j.requests       ? pearson_symmetric_kernel<CS_PAD, false, kRequestWaves, true>
                        : j.cs == CS_PAD ? pearson_symmetric_kernel<CS_PAD, true, kFieldWaves>
                                         : pearson_symmetric_kernel<CS_PAD, false, kFieldWaves>;
    hipLaunchKernelGGL(kernel, dim3(unsigned((j.num_items + 255) / 256)), dim3(256), 0, s, j.members_x, j.members_y, j.out,
                       uint32_t(j.num_voxels), j.cs, j.requests, uint32_t(j.num_items), j.xs, j.ys, j.use_abs);
}
}  // namespace

// Pearson between two vectors per item, both in registers: 2 <= cs <= kMaxSymmetricRegisterMembers, fewer than 2^32 items
hipError_t launch_pearson_two_vector(const TwoVectorJob& job, hipStream_t s) {
    if (job.measure != CRF_PEARSON || job.cs < 2 || job.cs > kMaxSymmetricRegisterMembers ||
        job.num_items >= (size_t(1) << 32))
        return hipErrorInvalidValue;
    switch ((job.cs + 15) / 16) {
        case 1: launch_two_vector<16>(job, s); break;
        case 2: launch_two_vector<32>(job, s); break;
        case 3: launch_two_vector<48>(job, s); break;
        case 4: launch_two_vector<64>(job, s); break;
        case 5: launch_two_vector<80>(job, s); break;
        case 6: launch_two_vector<96>(job, s); break;
        case 7: launch_two_vector<112>(job, s); break;
        default: launch_two_vector<128>(job, s); break;
    }
    return hipGetLastError();
}

namespace {
// occupancy request.  Registers: CS_PAD raw dwords + the working set of one pair of voxels (16-bit formats) or two
// (8-bit), each instantiation at the most waves per SIMD it reaches without scratch (tools/resource_usage.py).
constexpr int narrow_min_waves(int format, int cs_pad, bool exact) {
    if (format == CRF_MEMBER_U8) return cs_pad <= 32 ? 4 : cs_pad <= 48 || (cs_pad == 64 && exact) ? 3 : 2;
    return cs_pad <= 64 ? 4 : cs_pad <= 96 ? 3 : 2;
}

template <int FMT, int CS_PAD>
void launch_narrow(const void* const* d_narrow, const float* d_prep, float* d_out, size_t covered, int cs, bool out_vector,
                   hipStream_t s) {
    const size_t per_block = size_t(256) * narrow_vpl<FMT>();
    const dim3 grid(unsigned((covered + per_block - 1) / per_block)), block(256);
    if (cs == CS_PAD)
        hipLaunchKernelGGL((pearson_narrow_kernel<FMT, CS_PAD, true, narrow_min_waves(FMT, CS_PAD, true)>), grid, block, 0,
                           s, d_narrow, d_prep, d_out, uint32_t(covered), cs, out_vector ? 1 : 0);
    else
        hipLaunchKernelGGL((pearson_narrow_kernel<FMT, CS_PAD, false, narrow_min_waves(FMT, CS_PAD, false)>), grid, block,
                           0, s, d_narrow, d_prep, d_out, uint32_t(covered), cs, out_vector ? 1 : 0);
}

template <int FMT>
void launch_narrow_format(const void* const* d_narrow, const float* d_prep, float* d_out, size_t num_voxels, int cs,
                          bool out_vector, hipStream_t s) {
    const size_t covered = num_voxels / narrow_vpl<FMT>() * narrow_vpl<FMT>();
    if (covered > 0) {
        switch (cs <= 8 ? 8 : (cs + 15) / 16 * 16) {
            case 8: launch_narrow<FMT, 8>(d_narrow, d_prep, d_out, covered, cs, out_vector, s); break;
            case 16: launch_narrow<FMT, 16>(d_narrow, d_prep, d_out, covered, cs, out_vector, s); break;
            case 32: launch_narrow<FMT, 32>(d_narrow, d_prep, d_out, covered, cs, out_vector, s); break;
            case 48: launch_narrow<FMT, 48>(d_narrow, d_prep, d_out, covered, cs, out_vector, s); break;
            case 64: launch_narrow<FMT, 64>(d_narrow, d_prep, d_out, covered, cs, out_vector, s); break;
            case 80: launch_narrow<FMT, 80>(d_narrow, d_prep, d_out, covered, cs, out_vector, s); break;
            case 96: launch_narrow<FMT, 96>(d_narrow, d_prep, d_out, covered, cs, out_vector, s); break;
            case 112: launch_narrow<FMT, 112>(d_narrow, d_prep, d_out, covered, cs, out_vector, s); break;
            default: launch_narrow<FMT, 128>(d_narrow, d_prep, d_out, covered, cs, out_vector, s); break;
        }
    }
    if (covered < num_voxels)
        hipLaunchKernelGGL(pearson_narrow_tail_kernel<FMT>, dim3(1), dim3(64), 0, s, d_narrow, d_prep, d_out, covered,
                           num_voxels, cs);
}
}  // namespace

hipError_t launch_pearson_narrow(const void* const* d_narrow, int format, int cs, size_t num_voxels, bool out_vector,
                                 const RefSource& ref, float* d_prep, float* d_out, hipStream_t s, hipEvent_t ev_begin,
                                 hipEvent_t ev_end, LaunchInfo* info) {
    if (cs < 2 || cs > kNarrowMaxMembers || format == CRF_MEMBER_F32 ||
        num_voxels * member_format_bytes(format) >= kNarrowMaxBytes)
        return hipErrorInvalidValue;
    if (ref.prepare()) {
        if (!ref.values) return hipErrorInvalidValue;  // the caller gathers the converted reference values
        hipLaunchKernelGGL(pearson_prep_kernel, dim3(1), dim3(256), size_t(cs) * sizeof(float), s, ref, nullptr, cs, d_prep);
    }
    if (!ref.run()) return hipGetLastError();
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    switch (format) {
        case CRF_MEMBER_U8: launch_narrow_format<CRF_MEMBER_U8>(d_narrow, d_prep, d_out, num_voxels, cs, out_vector, s); break;
        case CRF_MEMBER_U16: launch_narrow_format<CRF_MEMBER_U16>(d_narrow, d_prep, d_out, num_voxels, cs, out_vector, s); break;
        case CRF_MEMBER_F16: launch_narrow_format<CRF_MEMBER_F16>(d_narrow, d_prep, d_out, num_voxels, cs, out_vector, s); break;
        default: return hipErrorInvalidValue;
    }
    if (info) info->kernel_name = "pearson_narrow_kernel";
    if (ev_end) (void)hipEventRecord(ev_end, s);
    return hipGetLastError();
}

namespace {
// occupancy request of pearson_symmetric_narrow_kernel.  Registers: 2 x CS_PAD raw dwords + the working set of one pair
// of voxels (16-bit formats) or two (8-bit) of both fields; each instantiation at the most waves per SIMD it reaches
// without scratch (tools/resource_usage.py; the table is in profiles/narrow_symmetric_ab.md).
constexpr int symmetric_narrow_min_waves(int format, int cs_pad, bool exact) {
    if (format == CRF_MEMBER_U8)
        return cs_pad == 8 ? (exact ? 8 : 6) : cs_pad == 16 ? 6 : cs_pad == 32 ? 4 : cs_pad == 48 ? 3 : cs_pad <= 96 ? 2 : 1;
    return cs_pad <= 16 ? 8 : cs_pad == 32 ? 5 : cs_pad == 48 ? 4 : cs_pad == 64 ? 3 : cs_pad <= 112 ? 2 : 1;
}

template <int FMT, int CS_PAD>
void launch_symmetric_narrow(const void* const* d_x, const void* const* d_y, float* d_out, size_t covered, int cs,
                             bool out_vector, hipStream_t s) {
    const size_t per_block = size_t(256) * narrow_vpl<FMT>();
    const dim3 grid(unsigned((covered + per_block - 1) / per_block)), block(256);
    if (cs == CS_PAD)
        hipLaunchKernelGGL((pearson_symmetric_narrow_kernel<FMT, CS_PAD, true, symmetric_narrow_min_waves(FMT, CS_PAD, true)>),
                           grid, block, 0, s, d_x, d_y, d_out, uint32_t(covered), cs, out_vector ? 1 : 0);
    else
        hipLaunchKernelGGL((pearson_symmetric_narrow_kernel<FMT, CS_PAD, false, symmetric_narrow_min_waves(FMT, CS_PAD, false)>),
                           grid, block, 0, s, d_x, d_y, d_out, uint32_t(covered), cs, out_vector ? 1 : 0);
}

template <int FMT>
void launch_symmetric_narrow_format(const void* const* d_x, const void* const* d_y, float* d_out, size_t num_voxels, int cs,
                                    bool out_vector, hipStream_t s) {
    const size_t covered = num_voxels / narrow_vpl<FMT>() * narrow_vpl<FMT>();
    if (covered > 0) {
        switch (cs <= 8 ? 8 : (cs + 15) / 16 * 16) {
            case 8: launch_symmetric_narrow<FMT, 8>(d_x, d_y, d_out, covered, cs, out_vector, s); break;
            case 16: launch_symmetric_narrow<FMT, 16>(d_x, d_y, d_out, covered, cs, out_vector, s); break;
            case 32: launch_symmetric_narrow<FMT, 32>(d_x, d_y, d_out, covered, cs, out_vector, s); break;
            case 48: launch_symmetric_narrow<FMT, 48>(d_x, d_y, d_out, covered, cs, out_vector, s); break;
            case 64: launch_symmetric_narrow<FMT, 64>(d_x, d_y, d_out, covered, cs, out_vector, s); break;
            case 80: launch_symmetric_narrow<FMT, 80>(d_x, d_y, d_out, covered, cs, out_vector, s); break;
            case 96: launch_symmetric_narrow<FMT, 96>(d_x, d_y, d_out, covered, cs, out_vector, s); break;
            case 112: launch_symmetric_narrow<FMT, 112>(d_x, d_y, d_out, covered, cs, out_vector, s); break;
            default: launch_symmetric_narrow<FMT, 128>(d_x, d_y, d_out, covered, cs, out_vector, s); break;
        }
    }
    if (covered < num_voxels)
        hipLaunchKernelGGL(pearson_symmetric_narrow_tail_kernel<FMT>, dim3(1), dim3(64), 0, s, d_x, d_y, d_out, covered,
                           num_voxels, cs);
}
}  // namespace

hipError_t launch_pearson_symmetric_narrow(const void* const* d_narrow_x, const void* const* d_narrow_y, int format, int cs,
                                           size_t num_voxels, bool out_vector, float* d_out, hipStream_t s,
                                           hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info) {
    if (!symmetric_narrow_routed(format, cs) || !d_narrow_x || !d_narrow_y || !d_out ||
        num_voxels * member_format_bytes(format) >= kNarrowMaxBytes)
        return hipErrorInvalidValue;
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    switch (format) {
        case CRF_MEMBER_U8:
            launch_symmetric_narrow_format<CRF_MEMBER_U8>(d_narrow_x, d_narrow_y, d_out, num_voxels, cs, out_vector, s);
            break;
        case CRF_MEMBER_U16:
            launch_symmetric_narrow_format<CRF_MEMBER_U16>(d_narrow_x, d_narrow_y, d_out, num_voxels, cs, out_vector, s);
            break;
        default:
            launch_symmetric_narrow_format<CRF_MEMBER_F16>(d_narrow_x, d_narrow_y, d_out, num_voxels, cs, out_vector, s);
            break;
    }
    if (info) info->kernel_name = "pearson_symmetric_narrow_kernel";
    if (ev_end) (void)hipEventRecord(ev_end, s);
    return hipGetLastError();
}

hipError_t launch_pearson(const float* const* d_members, int cs, size_t num_voxels, int max_vpt, const RefSource& ref,
                          float* d_prep, float* d_out, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end,
                          LaunchInfo* info, const PackedMembers& packed) {
    if (cs == 1)  // CorrelationCalculator.cpp:882-885
        return launch_single_member(ref, d_out, num_voxels, s, ev_begin, ev_end, info);
    if (ref.prepare())
        hipLaunchKernelGGL(pearson_prep_kernel, dim3(1), dim3(256), size_t(cs) * sizeof(float), s, ref, d_members, cs,
                           d_prep);
    if (!ref.run()) return hipGetLastError();

    size_t covered = num_voxels;  // voxels the per-voxel kernel below answers; pearson_stream_kernel takes the rest
    const char* name;
    hipError_t e = hipSuccess;
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    if (packed.header && cs >= kPackMinMembers && cs <= kPackMaxMembers && num_voxels > 0) {
        switch (pack_slots(cs)) {
            case 32: launch_reg_packed<32>(d_members, d_prep, d_out, num_voxels, cs, packed, s); break;
            case 48: launch_reg_packed<48>(d_members, d_prep, d_out, num_voxels, cs, packed, s); break;
            case 64: launch_reg_packed<64>(d_members, d_prep, d_out, num_voxels, cs, packed, s); break;
            case 80: launch_reg_packed<80>(d_members, d_prep, d_out, num_voxels, cs, packed, s); break;
            case 96: launch_reg_packed<96>(d_members, d_prep, d_out, num_voxels, cs, packed, s); break;
            case 112: launch_reg_packed<112>(d_members, d_prep, d_out, num_voxels, cs, packed, s); break;
            default: launch_reg_packed<128>(d_members, d_prep, d_out, num_voxels, cs, packed, s); break;
        }
        name = "pearson_reg_kernel";
    } else if (cs <= 224) {
        const int cs_pad = cs <= 8 ? 8 : cs <= 128 ? (cs + 15) / 16 * 16 : (cs + 31) / 32 * 32;
        // voxels per lane.  Measured on MI355X at 256^3 x 64 (profiles/): one voxel per lane (dword loads, 93 VGPRs,
        // 5 waves/SIMD) reaches 5.7 TB/s; 2 per lane (196 VGPRs, 2 waves/SIMD) 4.9 TB/s; 4 per lane 3.4 TB/s --
        // occupancy, not load width, is what keeps HBM busy here.
        const int vpt = cs_pad <= 16 && max_vpt >= 2 ? 2 : 1;
        covered = num_voxels / vpt * vpt;  // whole vectors; the descriptor bounds the last block
        const size_t per_block = size_t(256) * vpt;
        const size_t blocks = (covered + per_block - 1) / per_block;
        if (blocks > 0) {
            switch (cs_pad) {
                case 8: launch_reg_vpt<8>(vpt, d_members, d_prep, d_out, blocks, num_voxels, cs, s); break;
                case 16: launch_reg_vpt<16>(vpt, d_members, d_prep, d_out, blocks, num_voxels, cs, s); break;
                case 32: launch_reg_vpt<32>(vpt, d_members, d_prep, d_out, blocks, num_voxels, cs, s); break;
                case 48: launch_reg_vpt<48>(vpt, d_members, d_prep, d_out, blocks, num_voxels, cs, s); break;
                case 64: launch_reg_vpt<64>(vpt, d_members, d_prep, d_out, blocks, num_voxels, cs, s); break;
                case 80: launch_reg_vpt<80>(vpt, d_members, d_prep, d_out, blocks, num_voxels, cs, s); break;
                case 96: launch_reg_vpt<96>(vpt, d_members, d_prep, d_out, blocks, num_voxels, cs, s); break;
                case 112: launch_reg_vpt<112>(vpt, d_members, d_prep, d_out, blocks, num_voxels, cs, s); break;
                case 128: launch_reg_vpt<128>(vpt, d_members, d_prep, d_out, blocks, num_voxels, cs, s); break;
                case 160: launch_reg_vpt<160>(vpt, d_members, d_prep, d_out, blocks, num_voxels, cs, s); break;
                case 192: launch_reg_vpt<192>(vpt, d_members, d_prep, d_out, blocks, num_voxels, cs, s); break;
                default: launch_reg_vpt<224>(vpt, d_members, d_prep, d_out, blocks, num_voxels, cs, s); break;
            }
        }
        name = "pearson_reg_kernel";
    } else if (cs <= 288) {
        // 225..288 members: 224 or 240 values in registers + the rest in the lane's LDS column; measured at 512x512x128:
        // 256 members 85 % of the HBM peak (64 % with 256 register values under the two-wave cap, 53 % at one wave),
        // 272: 82 % (57 %), 288: 78 % (54 %).
        const LdsKernel k = cs <= 240   ? LdsKernel{pearson_reg_lds_kernel<224, 16, 2>, 16}
                            : cs <= 256 ? LdsKernel{pearson_reg_lds_kernel<240, 16, 2>, 16}
                                        : LdsKernel{pearson_reg_lds_kernel<240, 48, 2>, 48};
        e = launch_lds(k, (num_voxels + 255) / 256, d_members, d_prep, d_out, num_voxels, cs, s);
        name = "pearson_reg_lds_kernel";
    } else if (cs <= kSplitMaxMembers) {
        // 289..1216 members: two (up to 576) or four lanes per voxel.  From 289 members: measured at 512x512x128
        // against the one-lane kernels (registers + LDS rows), % of the HBM peak: 160 members 78 vs 83, 192: 76 vs 83,
        // 224: 75 vs 83, 256: 73 vs 87, 288: 74 vs 79, 320: 74 vs 71 (profiles/r03_pearson_two_lanes_from_129_members.txt).
        const int lanes = cs > 576 ? 4 : 2;  // (two lanes x 304 slots = 224 + 80 LDS rows: 0.5 KB of scratch per lane)
        const int slots = ((cs + lanes - 1) / lanes + 15) / 16 * 16;  // per lane, in steps of 16: 160 .. 304
        const size_t per_block = size_t(4) * (64 / lanes);
        e = launch_lds(split_kernel_for(slots, lanes), (num_voxels + per_block - 1) / per_block, d_members, d_prep,
                       d_out, num_voxels, cs, s);
        name = "pearson_split_kernel";
    } else {
        // chunked three-pass kernel (see pearson_big_kernel)
        const size_t tiles = (num_voxels + 63) / 64;
        const unsigned blocks = unsigned(tiles < size_t(kBigWaves) ? tiles : size_t(kBigWaves));
        hipLaunchKernelGGL(pearson_big_kernel, dim3(blocks), dim3(64), 0, s, d_members, d_prep, d_out,
                           uint32_t(num_voxels), cs);
        name = "pearson_big_kernel";
    }
    if (e != hipSuccess) return e;
    if (info) info->kernel_name = name;
    if (covered < num_voxels) {
        const size_t rest = num_voxels - covered;
        hipLaunchKernelGGL(pearson_stream_kernel, dim3(unsigned((rest + 255) / 256)), dim3(256), 0, s, d_members,
                           d_prep, d_out, covered, num_voxels, cs);
    }
    if (ev_end) (void)hipEventRecord(ev_end, s);
    return hipGetLastError();
}

}  // namespace crf
