// crf_internal.h -- declarations shared by the C-ABI (api.cpp) and the gfx950 kernel translation units.
// Everything here is internal to libcorrfield.so; the public surface is include/corrfield.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "../../include/corrfield.h"
#include "symmetric_narrow_route.h"  // symmetric_narrow_routed
#include "two_vector_route.h"        // kMaxSortMembers, kMaxSymmetricRegisterMembers

namespace crf {

// Largest member count the register-resident kernels are instantiated for; above it the streaming
// (re-reading) variants run.
constexpr int kMaxRegisterMembers = 384;  // 257..384: VGPRs + AGPRs + a little scratch at one wave per SIMD
// Prepared reference-derived table: floats (see each kernels_*.hip for its layout).
constexpr size_t kPrepBytes = 160 * 1024;  // (r02: room for the Kraskov x-distance table of 128 members, 133 KB)
// Largest member count of the generic (any-cs) kernels: bounded by the preparation scratch (2*cs ints / doubles).
constexpr int kMaxGenericMembers = 2048;
// where binned_prep_kernel leaves the reference-side entropy sum (fp64) inside the preparation scratch
constexpr size_t kBinnedSxOffset = kPrepBytes - 16;

// Where a preparation kernel takes the reference vector from: an explicit device array of cs floats (SEPARATE mode,
// or a vector received from another rank), or -- fused gather -- members[c][voxel]
// (referenceValues[c] = fields[c][IDXS(ref)], CorrelationCalculator.cpp:802,815-817).
struct RefSource {
    const float* values;  // non-null: use values[c]
    size_t voxel;         // else: members[c][voxel]
    // which halves of an evaluation a launcher performs: the reference-side preparation (into d_prep) and/or the
    // per-voxel kernel (reading d_prep).  Split so that a caller can prepare several evaluations ahead of time on
    // another stream (crf_prepare_device) and keep only the per-voxel kernels on the critical path.
    unsigned phase = 3;
    // non-null: the fused gather reads table[c][voxel] instead of the launcher's own member table -- the member table of
    // ANOTHER context whose slab holds the reference point (crf_group, direct exchange: same device, or a peer device
    // whose memory this one may read over xGMI)
    const float* const* table = nullptr;
    bool prepare() const { return (phase & 1u) != 0; }
    bool run() const { return (phase & 2u) != 0; }
};

struct LaunchInfo {
    const char* kernel_name = "";  // dominant per-voxel kernel (for rocprof row matching)
};

// ---- kernels_common.hip -----------------------------------------------------------------------------------
hipError_t launch_gather_reference(const float* const* d_members, int cs, size_t voxel, float* d_out, hipStream_t s);
constexpr int kMaxGatherRows = 32;
constexpr size_t kNoVoxel = ~size_t(0);
struct GatherRows {
    size_t voxel[kMaxGatherRows];  // kNoVoxel: the row is zero-filled
};
hipError_t launch_gather_reference_rows(const float* const* d_members, int cs, const GatherRows& rows, int num_rows,
                                        float* d_out, hipStream_t s);
hipError_t launch_minmax(const float* const* d_members, int cs, size_t num_voxels, uint32_t* d_keys /*[2]*/,
                         hipStream_t s);
float minmax_key_to_float(uint32_t key);
// the whole evaluation at one member: fills d_out with 1 (fill_kernel) if ref.run()
hipError_t launch_single_member(const RefSource& ref, float* d_out, size_t num_voxels, hipStream_t s,
                                hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info);
hipError_t launch_synth_box_member(float* d_out, int xs, int ys, int zs_local, int z_begin, int zs_global, int c,
                                   int cs, uint64_t seed, hipStream_t s);

// ---- packed members (kernels_pearson.hip: pearson_encode_kernel, pearson_reg_kernel<..., true>) -------------------
// A lossless 28-bit copy of the members for the Pearson field at kPackMinMembers..kPackMaxMembers members.  The grid is
// cut into tiles of 64 consecutive voxels (one wave of the field kernel); a SEGMENT is one member of one tile.  An fp32
// value (sign s, exponent field E, mantissa m) is stored as
//     lo16   m & 0xFFFF                                  (16 bits)
//     byte   s << 7 | m >> 16                            (8 bits)
//     code   0 if E == 0 (+-0, denormals), else E - base + 1 in 1..15   (4 bits)
// with one base byte per segment: the smallest non-zero E of the segment.  A segment fits if it holds no E == 255
// (NaN, +-Inf) and its non-zero exponents span at most 15 binades; one that does not gets the header byte
// kPackFallback and the field kernel reads it from the original member instead (its planes hold zeros).
//
// Memory: P = pack_slots(cs) slots per tile (cs rounded up to 16; slots cs..P-1 are padding: base 1, value +0).
//   header   tiles x P bytes, tile t at t * P: the P base bytes (read by the field kernel with scalar loads)
//   body     tiles x pack_tile_bytes(P), tile t at t * pack_tile_bytes(P), 1 KiB RUNS of 64 lanes x 16 B (lane l of the
//            wave = voxel 64 t + l owns bytes [16 l, 16 l + 16) of every run; one dwordx4 load per run and wave):
//     lo16 runs   P / 8       run r: member 8 r + i at bytes 2 i, 2 i + 1 of the lane's 16 B (little endian)
//     byte runs   P / 16      run r: member 16 r + i at byte i
//     code runs   (P + 31)/32 run r: member 32 r + i at bits 4 (i % 8) .. 4 (i % 8) + 3 of dword i / 8
//   in that order.  Lanes past the end of the grid hold zeros.  Every slot is stored and read, padding included:
//   pack_voxel_bytes(cs) = pack_tile_bytes(P) / 64 + P / 64 + 4 (result) per voxel against 4 cs + 4 from the members
//   themselves -- 229 against 260 B at 64 members, but 116.5 against 72 B at 17 (see kPackAutoByteRatio).
constexpr int kPackMinMembers = 17;
constexpr int kPackMaxMembers = 128;
constexpr uint32_t kPackFallback = 0xFFu;
__host__ __device__ inline int pack_slots(int cs) { return (cs + 15) / 16 * 16; }
__host__ __device__ inline int pack_lo_runs(int slots) { return slots / 8; }
__host__ __device__ inline int pack_byte_runs(int slots) { return slots / 16; }
__host__ __device__ inline int pack_code_runs(int slots) { return (slots + 31) / 32; }
__host__ __device__ inline uint32_t pack_tile_bytes(int slots) {
    return 1024u * uint32_t(pack_lo_runs(slots) + pack_byte_runs(slots) + pack_code_runs(slots));
}
// HBM bytes per voxel of one evaluation from the packed copy (members + base bytes + result)
inline double pack_voxel_bytes(int cs) {
    const int slots = pack_slots(cs);
    return double(pack_tile_bytes(slots) + uint32_t(slots)) / 64.0 + 4.0;
}
// AUTO packs only where pack_voxel_bytes(cs) <= this x (4 cs + 4).  Measured on MI355X at 256^3, kernel time packed / raw
// against the byte ratio (profiles/packed_members_layout_sweep.md): byte ratios of 0.88-0.92 gave 0.85-0.93 (7-15 %
// faster) at every count tried, 0.94 gave 0.93-1.00, about 1.0 gave 0.98-1.05, and above that up to 1.56.
constexpr double kPackAutoByteRatio = 0.925;
// base byte of a segment from the smallest and largest non-zero exponent field of its values (emin = 256 when every
// value is +-0 or denormal) and whether any value is NaN or +-Inf
__host__ __device__ inline uint32_t pack_segment_base(uint32_t emin, uint32_t emax, bool special) {
    if (special) return kPackFallback;
    if (emin > 254u) return 1u;
    return emax - emin <= 14u ? emin : kPackFallback;
}
__host__ __device__ inline uint32_t pack_lo16(uint32_t bits) { return bits & 0xFFFFu; }
__host__ __device__ inline uint32_t pack_byte(uint32_t bits) { return ((bits >> 24) & 0x80u) | ((bits >> 16) & 0x7Fu); }
__host__ __device__ inline uint32_t pack_code(uint32_t bits, uint32_t base) {
    const uint32_t e = (bits >> 23) & 0xFFu;
    return e == 0u ? 0u : e - base + 1u;
}
// v_perm_b32: byte i of the result is byte sel_i (0..7) of the 64-bit {hi, lo}
__host__ __device__ inline uint32_t perm_bytes(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t d = (uint64_t(hi) << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) r |= uint32_t((d >> (8 * ((sel >> (8 * i)) & 7u))) & 0xFFu) << (8 * i);
    return r;
#endif
}
// The value of a fitting segment from its three parts, each taken out of the word the field kernel loads: lo16 is half
// `h` of lo_word, the byte is byte `b` of byte_word, the code is nibble `n` of code_word.  In the field kernel the
// positions are compile-time constants: v_perm_b32 puts lo16 at the bottom and the byte twice above it (its top bit
// lands on the sign, its low 7 bits on the top of the mantissa), v_bfe_u32 takes the code, an add-shift and a select
// make the exponent field, v_bfi_b32 merges it -- 6 VALU per value.
__host__ __device__ inline uint32_t unpack_bits(uint32_t lo_word, int h, uint32_t byte_word, int b, uint32_t code_word,
                                                int n, uint32_t base) {
    const uint32_t sel = uint32_t(2 * h) | uint32_t(2 * h + 1) << 8 | uint32_t(4 + b) << 16 | uint32_t(4 + b) << 24;
    const uint32_t w = perm_bytes(byte_word, lo_word, sel);
    const uint32_t code = (code_word >> (4 * n)) & 0xFu;
    const uint32_t e = code != 0u ? (code + base - 1u) << 23 : 0u;
    return (w & 0x807FFFFFu) | e;
}

// ---- kernels_pearson.hip ----------------------------------------------------------------------------------
// The packed copy of a context's members (see above), or both null: the field kernel reads the members themselves.
struct PackedMembers {
    const unsigned char* header = nullptr;
    const unsigned char* body = nullptr;
};
// d_ref: cs reference values on the device.  d_prep: scratch of kPrepBytes.  Writes num_voxels floats to d_out.
// max_vpt: widest per-lane vector (1, 2 or 4 floats) the member/output pointers are aligned for.
// packed: a packed copy of d_members (header non-null) for kPackMinMembers <= cs <= kPackMaxMembers, else ignored.
hipError_t launch_pearson(const float* const* d_members, int cs, size_t num_voxels, int max_vpt, const RefSource& ref,
                          float* d_prep, float* d_out, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end,
                          LaunchInfo* info, const PackedMembers& packed = PackedMembers{});
// Builds the packed copy of d_members into header (tiles x pack_slots(cs) bytes) and body (tiles x pack_tile_bytes),
// tiles = ceil(num_voxels / 64), and adds the number of member segments that fall back to *d_fallbacks.
hipError_t launch_pack_members(const float* const* d_members, int cs, size_t num_voxels, unsigned char* header,
                               unsigned char* body, uint32_t* d_fallbacks, hipStream_t s);
// ---- narrow primary members (include/corrfield.h: crf_member_format) ---------------------------------------------
// The value the calculators see of a u8 / u16 / f16 element is float(b) / 255.0f, float(s) / 65535.0f, float(h)
// (reference: src/Volume/Cache/HostCacheEntry.cpp:107-176).  The Pearson, the Kendall and the binned-MI field at
// 2..kNarrowMaxMembers members read such members directly (kernels_pearson.hip: pearson_narrow_kernel;
// kernels_rank_narrow.hip: kendall_narrow_kernel; kernels_binned_narrow.hip: mi_binned_narrow_kernel), the Kraskov-MI field
// where kraskov_narrow_plan routes it (kernels_kraskov_narrow.hip), and so do the
// sibling reductions, the extrema and the gathers; everything else runs on an fp32 copy that launch_widen_members builds
// (kernels_common.hip).
constexpr int kNarrowMaxMembers = 128;
// A narrow member must be smaller than this: the native kernel's 32-bit voxel index and byte offset of the last block's
// surplus lanes (up to 1020 voxels past the end) must not wrap.
constexpr size_t kNarrowMaxBytes = size_t(0xFFFF0000u);
constexpr size_t member_format_bytes(int format) {
    return format == CRF_MEMBER_U8 ? 1 : format == CRF_MEMBER_F32 ? 4 : 2;
}
// d_narrow: cs device pointers to num_voxels elements of `format` each, every one 4-byte aligned; num_voxels x element
// size below kNarrowMaxBytes.  ref.values holds the cs (converted) reference values when ref.prepare().  out_vector: d_out is
// aligned for one vector store of a lane's 2 (16-bit) or 4 (8-bit) results.
hipError_t launch_pearson_narrow(const void* const* d_narrow, int format, int cs, size_t num_voxels, bool out_vector,
                                 const RefSource& ref, float* d_prep, float* d_out, hipStream_t s, hipEvent_t ev_begin,
                                 hipEvent_t ev_end, LaunchInfo* info);
// The symmetric Pearson field over two fields in one narrow format, read as stored (pearson_symmetric_narrow_kernel):
// out[v] = Pearson(d_narrow_x[.][v], d_narrow_y[.][v]), bit-identical to launch_pearson_two_vector in field mode on the
// converted values.  Both tables as d_narrow above (every pointer 4-byte aligned); symmetric_narrow_routed(format, cs)
// must hold, else hipErrorInvalidValue.  Main kernel and tail kernel are bracketed by one event pair.
hipError_t launch_pearson_symmetric_narrow(const void* const* d_narrow_x, const void* const* d_narrow_y, int format, int cs,
                                           size_t num_voxels, bool out_vector, float* d_out, hipStream_t s,
                                           hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info);
// member c of the fp32 copy = d_block + c * stride, num_voxels converted values each
hipError_t launch_widen_members(const void* const* d_narrow, int format, int cs, size_t num_voxels, float* d_block,
                                size_t stride, hipStream_t s);
// d_out[c] = converted value of d_narrow[c][voxel]
hipError_t launch_gather_reference_narrow(const void* const* d_narrow, int format, int cs, size_t voxel, float* d_out,
                                          hipStream_t s);
// launch_gather_reference_rows / launch_minmax on narrow members (no alignment asked of the pointers beyond the
// element's own): the rows hold converted values; the keys are those launch_minmax leaves for the converted values
hipError_t launch_gather_reference_rows_narrow(const void* const* d_narrow, int format, int cs, const GatherRows& rows,
                                               int num_rows, float* d_out, hipStream_t s);
hipError_t launch_minmax_narrow(const void* const* d_narrow, int format, int cs, size_t num_voxels, uint32_t* d_keys /*[2]*/,
                                hipStream_t s);
hipError_t launch_fill(float* d_out, size_t n, float value, hipStream_t s);
hipError_t launch_abs(float* d_out, size_t n, hipStream_t s);  // in place |.| (CRF_FLAG_ABSOLUTE_VALUE on a field)

// ---- kernels_rank.hip (Spearman, Kendall) ---------------------------------------------------------------
// d_todo: num_voxels + 1 uint32 (count, then voxel indices) through which the first-pass kernels (above 16 members)
// defer voxels that contain ties to the monolithic kernel; null above 16 members: hipErrorInvalidValue.
hipError_t launch_spearman(const float* const* d_members, int cs, size_t num_voxels, const RefSource& ref,
                           float* d_prep, uint32_t* d_todo, float* d_out, hipStream_t s, hipEvent_t ev_begin,
                           hipEvent_t ev_end, LaunchInfo* info);
hipError_t launch_kendall(const float* const* d_members, int cs, size_t num_voxels, const RefSource& ref,
                          float* d_prep, uint32_t* d_todo, float* d_out, hipStream_t s, hipEvent_t ev_begin,
                          hipEvent_t ev_end, LaunchInfo* info);
// stride of kendall_prep_kernel's tables at 2..128 members: the same for a preparation and any later evaluation from it
constexpr int pad_pow2(int cs) { return cs <= 8 ? 8 : cs <= 16 ? 16 : cs <= 32 ? 32 : cs <= 64 ? 64 : 128; }

// ---- kernels_rank_narrow.hip: Kendall on narrow members, read as stored ------------------------------------------------
// One kernel, one pass, ties included (no todo list): 2 <= cs <= kNarrowMaxMembers, bit-identical to launch_kendall on the
// converted values.  d_narrow: cs device pointers to num_voxels elements of `format`, each aligned to its element (no
// more); num_voxels x element size below kNarrowMaxBytes.  ref.values holds the cs reference values (fp32, any values)
// when ref.prepare(); d_prep gets launch_kendall_prep's tables with stride pad_pow2(cs).
hipError_t launch_kendall_narrow(const void* const* d_narrow, int format, int cs, size_t num_voxels, const RefSource& ref,
                                 float* d_prep, float* d_out, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end,
                                 LaunchInfo* info);
// Spearman the same way: one kernel, one pass, ties included (no todo list, no workspace), 33 <= cs <= kNarrowMaxMembers,
// bit-identical to launch_spearman on the converted values.  d_narrow as for launch_kendall_narrow (element alignment
// only).  ref.values holds the cs reference values (fp32, any values) when ref.prepare(); d_prep gets
// launch_spearman_prep's table.  Up to 32 members stay on the fp32 copy (the fp32 kernels handle ties in line there).
// Which (format, member count) the native kernel serves, by measurement (profiles/narrow_spearman_ab.md: native kernel
// time <= the fp32 kernels' on the copy + their run-to-run spread, per format and N = cs rounded up to 8): every format
// at every N from 40 to 128.  hipErrorInvalidValue for a combination that is not routed.
inline bool spearman_narrow_routed(int format, int cs) {
    return format != CRF_MEMBER_F32 && cs >= 33 && cs <= kNarrowMaxMembers;
}
hipError_t launch_spearman_narrow(const void* const* d_narrow, int format, int cs, size_t num_voxels, const RefSource& ref,
                                  float* d_prep, float* d_out, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end,
                                  LaunchInfo* info);

// ---- kernels_binned.hip / kernels_kraskov.hip -------------------------------------------------------------------
struct BinnedArgs {
    int num_bins;
    float min_ref, max_ref, min_query, max_query;
    bool to_cc;
};
// d_tables (fp64, built on the host per member count, see build_tables() in api.cpp):
//   [0, cs]            psi(n) = -gamma + H_{n-1}  (psi(0) = NaN)
//   [cs+1, 2cs+1]      T[c] = (c/cs) * ln(c/cs)   (T[0] = 0)
//   [2cs+2, 3cs+2)     noise_ref[e]   = double(u_e) * 1e-10, xorshift32 stream seeded 617406168
//   [3cs+2, 4cs+2)     noise_query[e] = double(u_e) * 1e-10, xorshift32 stream seeded 864730169
hipError_t launch_mi_binned(const float* const* d_members, int cs, size_t num_voxels, const RefSource& ref,
                            const BinnedArgs& a, const double* d_tables, float* d_prep, float* d_out, hipStream_t s,
                            hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info);
hipError_t launch_mi_binned_hist(const float* const* d_members, int cs, size_t num_voxels, const RefSource& ref,
                                 const BinnedArgs& a, const double* d_tables, float* d_prep, float* d_out, hipStream_t s,
                                 hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info);
// ---- kernels_binned_narrow.hip: binned MI on narrow members, read as stored ----------------------------------------
// 2 <= cs <= kNarrowMaxMembers, bit-identical to launch_mi_binned on the converted values.  d_narrow: cs device pointers to
// num_voxels elements of `format`, each aligned to its element (no more); num_voxels x element size below kNarrowMaxBytes.
// ref.values holds the cs reference values (fp32, any values) when ref.prepare(); d_prep gets launch_binned_prep's layout
// with the stride of launch_mi_binned (cs rounded up to 16).
// Which (format, member count) the native kernel serves, by measurement (profiles/narrow_binned_ab.md: native kernel time
// <= the fp32 kernel's on the copy + its run-to-run spread, per format and N = cs rounded up to 16): uint8 (table front
// end) at every N; uint16 at N = 32 and 64; float16 at N = 64.  The 16-bit formats at 100 and 128 members and float16 at 24
// were 2-4 % slower than the copy route and stay on it, as do the 16-bit N that were not measured (16, 48, 80, 96); only
// the routed instantiations are built.
inline bool binned_narrow_routed(int format, int cs) {
    const int n = (cs + 15) / 16 * 16;
    return format == CRF_MEMBER_U8 || (format == CRF_MEMBER_U16 && (n == 32 || n == 64)) ||
           (format == CRF_MEMBER_F16 && n == 64);
}
hipError_t launch_mi_binned_narrow(const void* const* d_narrow, int format, int cs, size_t num_voxels, const RefSource& ref,
                                   const BinnedArgs& a, const double* d_tables, float* d_prep, float* d_out, hipStream_t s,
                                   hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info);
struct KraskovArgs {
    int k;
    int estimator;  // 1 or 2
    bool to_cc;
    // psi(k) for KSG-1, psi(k) - 1/k for KSG-2 (MutualInformation.cpp:438,503), evaluated on the host: k may exceed the
    // member count (the reference accepts any k >= 1; its kd-tree just returns at most cs points), the device psi
    // table ends at cs
    double c_term;
};
hipError_t launch_mi_kraskov(const float* const* d_members, int cs, size_t num_voxels, const RefSource& ref,
                             const KraskovArgs& a, const double* d_tables, float* d_prep, float* d_out, hipStream_t s,
                             hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info);

// ---- kernels_kraskov_narrow.hip: Kraskov MI on narrow members, read as stored --------------------------------------
// 2 <= cs <= kNarrowMaxMembers where kraskov_narrow_plan (kraskov_plan.h) routes (format, cs, k) under the CRF_KRASKOV_*
// switches in force -- kraskov_narrow_routed is that question; bit-identical to launch_mi_kraskov on the converted values.
// d_narrow: cs device pointers to num_voxels elements of `format`, each aligned to its element (no more); num_voxels x
// element size below kNarrowMaxBytes.  ref.values holds the cs reference values (fp32, any values) when ref.prepare();
// d_prep gets launch_kraskov_prep's layout.  hipErrorInvalidValue for a combination that is not routed.
bool kraskov_narrow_routed(int format, int cs, int k);
hipError_t launch_mi_kraskov_narrow(const void* const* d_narrow, int format, int cs, size_t num_voxels, const RefSource& ref,
                                    const KraskovArgs& a, const double* d_tables, float* d_prep, float* d_out, hipStream_t s,
                                    hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info);

hipError_t launch_mi_kraskov_direct(const float* const* d_members, int cs, size_t num_voxels, const RefSource& ref,
                                    const KraskovArgs& a, const double* d_tables, float* d_prep, float* d_out,
                                    hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info);

// ---- kernels_generic.hip: any member count (O(cs^2) counting algorithms, runtime loops) ------------------
struct GenericArgs {
    int measure;  // crf_measure value
    int num_bins;
    float min_ref, max_ref, min_query, max_query;
    int k, estimator;
    double kraskov_c;  // KraskovArgs::c_term
};
// workspace: generic_workspace_bytes(cs, num_voxels) bytes of device memory (per-block voxel tiles)
size_t generic_workspace_bytes(int cs, size_t num_voxels);
// d_todo: num_voxels + 1 uint32, or null (Spearman / Kendall at 129..256 members defer voxels with ties through it)
hipError_t launch_generic(const float* const* d_members, int cs, size_t num_voxels, const RefSource& ref,
                          const GenericArgs& a, const double* d_tables, float* d_prep, unsigned char* d_workspace,
                          float* d_out, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info,
                          uint32_t* d_todo = nullptr);
// kernels_rank.hip: Spearman at 129..256 members (spearman_pair_kernel); false if it does not apply.  The caller runs the
// counting kernel over d_todo afterwards.
bool launch_spearman_pair(const float* const* d_members, const float* d_prep, float* d_out, size_t num_voxels, int cs,
                          uint32_t* d_todo, hipStream_t s);
bool launch_kendall_pair(const float* const* d_members, const int* d_prep, float* d_out, size_t num_voxels, int cs,
                         uint32_t* d_todo, hipStream_t s);
// ---- kernels_stats.hip: ensemble mean (kind 0) / spread (kind 1) ------------------------------------------
hipError_t launch_ensemble_stat(int kind, const float* const* d_members, int cs, size_t num_voxels, float* d_out,
                                hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info);

hipError_t launch_set_predicate(const float* const* d_members, int cs, size_t num_voxels, int op, float comparison_value,
                                int count_lower, int count_upper, float* d_out, hipStream_t s, hipEvent_t ev_begin,
                                hipEvent_t ev_end, LaunchInfo* info);
// The same on members in a narrow native format, read as stored (bit-identical to the fp32 launchers on the converted
// values).  d_narrow as for launch_pearson_narrow: every pointer 4-byte aligned, num_voxels x element size below
// kNarrowMaxBytes; any cs >= 1.  Main kernel and tail kernel are bracketed by one event pair.
hipError_t launch_ensemble_stat_narrow(int kind, const void* const* d_narrow, int format, int cs, size_t num_voxels,
                                       float* d_out, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end,
                                       LaunchInfo* info);
hipError_t launch_set_predicate_narrow(const void* const* d_narrow, int format, int cs, size_t num_voxels, int op,
                                       float comparison_value, int count_lower, int count_upper, float* d_out,
                                       hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info);
hipError_t launch_tile_field(const float* d_linear, float* d_tiled, int xs, int ys, int zs, hipStream_t s);

// ---- kernels_dkl.hip: DKLCalculator (estimator 0 = binned, 1 = entropy k-NN) --------------------------------
size_t dkl_workspace_bytes(int cs, int estimator, int num_bins, size_t num_voxels);
hipError_t launch_dkl(const float* const* d_members, int cs, size_t num_voxels, int estimator, int num_bins, int k,
                      double knn_const, unsigned char* d_workspace, float* d_out, hipStream_t s, hipEvent_t ev_begin,
                      hipEvent_t ev_end, LaunchInfo* info);
// ---- kernels_dkl.hip: DKL on narrow members, read as stored (dkl_kernel<FMT, NS> at a narrow FMT) --------------------
// Any cs in 1..kMaxGenericMembers, both estimators, bit-identical to launch_dkl on the converted values; the workspace is
// launch_dkl's (dkl_workspace_bytes: the columns hold converted floats).  d_narrow: cs device pointers to num_voxels
// elements of `format`, each aligned to its element (no more); num_voxels x element size below kNarrowMaxBytes.  One event
// pair around the one kernel, reported as "dkl_narrow_kernel".  hipErrorInvalidValue for CRF_MEMBER_F32 or an unknown format.
// Which (format, member count, estimator, k) the native kernel serves, by measurement (profiles/narrow_dkl_ab.md: native
// kernel time <= the fp32 kernel's on the copy + its run-to-run spread in every measured row of a class; a class is a
// format, an estimator and an instantiation -- N = the member count rounded up to 16, or the counting sort).  The network
// instantiations came out 1-5 % slower than dkl_kernel almost everywhere, the counting-sort ones 0-3 % faster:
//   binned   uint8 and uint16 at N = 32 (17..32 members); uint8 and float16 from 97 members on (counting sort)
//   k-NN     uint8 and uint16 at N = 64 (49..64 members) with k <= 2 (the register descent; larger k was not measured);
//            every format from 129 members on (counting sort)
// Everything else, the instantiations that were not measured (N = 16, 48, 80, 96) included, stays on the copy.
constexpr bool dkl_narrow_routed(int format, int cs, int estimator, int k) {
    if (format != CRF_MEMBER_U8 && format != CRF_MEMBER_U16 && format != CRF_MEMBER_F16) return false;
    const int n = (cs + 15) / 16 * 16;
    if (estimator == CRF_DKL_BINNED)
        return cs >= 97 ? format != CRF_MEMBER_U16 : (n == 32 && format != CRF_MEMBER_F16);
    return cs >= 129 || (n == 64 && k <= 2 && format != CRF_MEMBER_F16);
}
hipError_t launch_dkl_narrow(const void* const* d_narrow, int format, int cs, size_t num_voxels, int estimator, int num_bins,
                             int k, double knn_const, unsigned char* d_workspace, float* d_out, hipStream_t s,
                             hipEvent_t ev_begin, hipEvent_t ev_end, LaunchInfo* info);

// ---- kernels_similarity.hip: whole-field similarity of two fields (crf_field_similarity) ------------------------------
// ONE value over the samples (x[m][v], y[m][v]), m < members, v < num_voxels; a pair with a NaN on either side is left
// out.  x, y: device tables of `members` fp32 volumes; num_voxels below 2^30 and members x num_voxels at most 2^31 - 1
// (the reference counts samples in an int), else hipErrorInvalidValue.  vec16: every member of both tables is 16-byte
// aligned (16-byte loads; dword loads otherwise, same bits).  workspace: similarity_workspace_bytes() of device memory,
// 8-byte aligned, which also receives the results; both launchers are stream-ordered and leave reading them to the caller.
constexpr int kSimilarityMaxBins = 128;  // num_bins^2 32-bit counters in 64 KiB of LDS
struct SimilarityJob {
    const float* const* x;
    const float* const* y;
    int members;
    size_t num_voxels;
    bool vec16;
    unsigned char* workspace;
};
size_t similarity_workspace_bytes();
// where the launchers leave their results inside the workspace
const double* similarity_stats(const unsigned char* workspace);  // 7 doubles: N, mean x, mean y, Sxx, Syy, Sxy, value
const unsigned long long* similarity_samples(const unsigned char* workspace);    // pairs without a NaN
const unsigned long long* similarity_histogram(const unsigned char* workspace);  // num_bins^2 counts, x bin major
// Pearson: two passes of similarity_moments_kernel, each followed by the one-block similarity_finish_kernel; no
// floating-point atomics.  One event pair around the four launches.
hipError_t launch_similarity_moments(const SimilarityJob& job, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end,
                                     LaunchInfo* info);
// The joint histogram of binned MI over x01 = (x - min_x) / (max_x - min_x), y01 likewise, formed in fp32, bin =
// clamp(int(double(x01) * num_bins), 0, num_bins - 1) as compiled for x86-64 (crf_binned_bins.h).  1 <= num_bins <=
// kSimilarityMaxBins.  The counts-to-MI tail runs on the host (crf_similarity_tail.h).
hipError_t launch_similarity_histogram(const SimilarityJob& job, int num_bins, float min_x, float max_x, float min_y,
                                       float max_y, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end,
                                       LaunchInfo* info);

// ---- kernels_rank_similarity.hip: ranks over a device array, and the rank form of the field similarity ----------------
// Fractional ranks of `count` <= 2^31 - 1 fp32 values in input order (computeRanks, Correlation.cpp:277-303) by a
// device-wide LSD radix sort; a NaN gets rank NaN and is not ranked.  d_ranks may be d_values itself (the values are read
// once, before the first rank is stored) but must not overlap them otherwise.  scratch: rank_sort_scratch_bytes(count)
// of device memory, 256-byte aligned.  SYNCHRONISES the stream once (the host reads the digit histograms back and leaves
// out the passes that would move nothing); *ranked (may be null) is final on return, the ranks are stream-ordered.
size_t rank_sort_scratch_bytes(size_t count);
hipError_t launch_rank_values(const float* d_values, size_t count, float* d_ranks, unsigned char* scratch, hipStream_t s,
                              hipEvent_t ev_begin, hipEvent_t ev_end, unsigned long long* ranked, LaunchInfo* info);
// Spearman over the samples of a SimilarityJob: pairs with a NaN masked, ranks of x and of y, then
// launch_similarity_moments over the two rank arrays (the results are where that launcher leaves them, in job.workspace).
// scratch: rank_similarity_scratch_bytes(members, num_voxels).  One event pair around all launches.
size_t rank_similarity_scratch_bytes(int members, size_t num_voxels);
hipError_t launch_rank_similarity(const SimilarityJob& job, unsigned char* scratch, hipStream_t s, hipEvent_t ev_begin,
                                  hipEvent_t ev_end, LaunchInfo* info);

// ---- kernels_kendall_similarity.hip: Kendall's tau-b over all samples ---------------------------------------------------------
// The integers of computeKendall<int64_t> (Correlation.cpp:423-455) over the pairs (x[i], y[i]) without a NaN: *kept = n,
// counts = {n1, n2, S} (ties of x, ties of y, strict inversions of y in the order of x, then y); crf_similarity_tail.h makes
// the value of them.  Two sorts by the device-wide radix sort, then a tile kernel and merge levels that count inversions.
// count in [1, 2^31 - 1]; d_x and d_y are only read and may be one array.  scratch: kendall_scratch_bytes(count) of device
// memory, 256-byte aligned.  SYNCHRONISES the stream (the digit histograms, then the counts): everything is final on
// return.  One event pair around all launches.
size_t kendall_scratch_bytes(size_t count);
hipError_t launch_kendall_values(const float* d_x, const float* d_y, size_t count, unsigned char* scratch, hipStream_t s,
                                 hipEvent_t ev_begin, hipEvent_t ev_end, unsigned long long* kept, long long counts[3],
                                 LaunchInfo* info);
// The same over the samples of a SimilarityJob (job.workspace is not used); scratch: kendall_scratch_bytes(members x
// num_voxels).
hipError_t launch_kendall_similarity(const SimilarityJob& job, unsigned char* scratch, hipStream_t s, hipEvent_t ev_begin,
                                     hipEvent_t ev_end, unsigned long long* kept, long long counts[3], LaunchInfo* info);

// ---- two vectors per item: the symmetric field mode and pair requests --------------------------------------------------
// One evaluation of a measure between two member vectors per item.  Field mode (requests == nullptr): item v is voxel
// pair (v, v), X = members_x[.][v] (the primary field), Y = members_y[.][v] (the secondary field).  Request mode: item r
// is requests[8 r ..] = {xi,yi,zi,i,xj,yj,zj,j}, X = members_x at voxel i, Y = members_y at voxel j.  Which kernel serves
// a job is two_vector_route's decision (two_vector_route.h); a launcher called outside the domain that table gives it
// returns hipErrorInvalidValue.
struct TwoVectorJob {
    const float* const* members_x;
    const float* const* members_y;
    int cs, xs, ys;
    size_t num_voxels;         // of every member volume
    const uint32_t* requests;  // null: field mode
    size_t num_items;          // voxels (field mode) or requests
    int measure, num_bins;
    float min_x, max_x, min_y, max_y;  // binned measures in field mode; requests normalise with the pair's own extrema
    int k;
    double kraskov_c;  // psi(k) (two-vector Kraskov is KSG-1), host-evaluated like KraskovArgs::c_term
    int use_abs;       // request mode: |result|
    const double* tables;
    unsigned char* workspace;  // direct_symmetric_workspace_bytes / pair_workspace_bytes for the kernels that use one
    float* out;
};
size_t pair_workspace_bytes(int cs, size_t num_requests);
size_t direct_symmetric_workspace_bytes(int cs, size_t num_voxels, int measure);
hipError_t launch_pearson_two_vector(const TwoVectorJob& job, hipStream_t s);    // kernels_pearson.hip
hipError_t launch_sorted_rank(const TwoVectorJob& job, hipStream_t s);           // kernels_symmetric.hip: Spearman, Kendall
hipError_t launch_sorted_binned(const TwoVectorJob& job, hipStream_t s);         // kernels_symmetric_binned.hip
hipError_t launch_mi_kraskov_symmetric(const TwoVectorJob& job, hipStream_t s);  // kernels_kraskov.hip, field mode
hipError_t launch_direct_symmetric(const TwoVectorJob& job, hipStream_t s);      // kernels_generic.hip, field mode
hipError_t launch_pair_requests(const TwoVectorJob& job, hipStream_t s);         // kernels_generic.hip
// preparation launchers shared with the generic path (kernels_rank.hip / kernels_binned.hip / kernels_kraskov.hip); n_pad = table stride
void launch_spearman_prep(const RefSource& ref, const float* const* d_members, int cs, float* d_prep, hipStream_t s);
void launch_kendall_prep(const RefSource& ref, const float* const* d_members, int cs, int n_pad, int* d_prep,
                         hipStream_t s);
void launch_binned_prep(const RefSource& ref, const float* const* d_members, int cs, int n_pad, const BinnedArgs& a,
                        const double* tableT, int* d_prep, hipStream_t s);
void launch_kraskov_prep(const RefSource& ref, const float* const* d_members, int cs, const double* noise_ref,
                         double* d_prep, hipStream_t s);

}  // namespace crf
