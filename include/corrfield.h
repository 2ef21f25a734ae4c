/*
 * corrfield.h -- C ABI of libcorrfield.so, the MI355X (gfx950) correlation-field engine.
 *
 * Drop-in boundary for ONE path of chrismile/Correrender: the per-voxel ensemble correlation estimators evaluated
 * between one reference grid point and every voxel of a 3-D grid, i.e. what
 *     void CorrelationCalculator::calculateCpu(int timeStepIdx, int ensembleIdx, float* buffer)
 * (reference: src/Calculators/CorrelationCalculator.cpp:781-1154, declared src/Calculators/Calculator.hpp:123-124)
 * computes.  The reference has no C ABI (calculators are compiled-in C++ classes registered as factories,
 * src/Volume/VolumeData.cpp:198-232); these entry points are what a `Calculator` subclass living in the reference
 * tree would bind to hand the hot loop to the GPU -- see INTEGRATION.md for that subclass and
 * correrender_amd/csrc/host/ for this repo's mirror of the ICorrelationCalculator/VolumeData surface built on top.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ / torch types; every function returns 0 on success, non-zero on error
 *     (the reference reports errors through sgl::Logfile::throwError, e.g. VolumeData.cpp:1217-1221; the adapter
 *     maps a non-zero status + crf_last_error() onto that).
 *   - single caller thread per context (the reference calls calculators from the render thread only,
 *     VolumeData.cpp:1225,1469-1472); no re-entrancy.
 *   - the *_device entry points are asynchronous on the stream they are given, but a context owns ONE set of scratch
 *     buffers (reference vector, reference-side tables, deferred-voxel list, workspace): at most one evaluation per
 *     context may be in flight at a time unless consecutive calls are ordered on the same stream (or by events).  The
 *     only state meant for overlap across streams are the prepared slots of crf_prepare_device (given a reference
 *     VECTOR; a reference POINT on members in a narrow format is gathered through the one reference-vector buffer, so
 *     such preparations must be ordered like any other evaluation).  crf_set_grid and any
 *     call that has to grow a scratch buffer synchronise the device first.
 *   - crf_compute (host output) of a result of 8 MiB or more evaluates the grid in voxel ranges on TWO streams of the
 *     context, so the scratch that the per-voxel kernels write (deferred-voxel list with its counter, workspace) exists
 *     once per stream there: ranges in flight together never share it, ranges on one stream are ordered.  Both sets are
 *     sized for the largest range before the first range is launched; nothing is grown between ranges.
 *   - volumes are fp32, x fastest: voxel (x,y,z) at z*xs*ys + y*xs + x  (IDXS, src/Loaders/DataSet.hpp:37);
 *     the ensemble is member-major SoA: one contiguous volume per member
 *     (std::vector<const float*> fields, CorrelationCalculator.cpp:791-800).
 *   - outputs are caller-owned: exactly xs*ys*zs floats are written, nothing is retained
 *     (VolumeData.cpp:1222-1226 allocates the buffer and wraps it in a HostCacheEntry).
 *   - There is NO CPU fallback: every compute entry point fails with CRF_ERR_DEVICE if no gfx950 device is usable.
 */
#ifndef CORRFIELD_H
#define CORRFIELD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crf_context crf_context;

/* Same order and meaning as enum class CorrelationMeasureType (src/Calculators/CorrelationDefines.hpp:41-45);
 * the string ids are CORRELATION_MEASURE_TYPE_IDS (CorrelationDefines.hpp:54-57). */
typedef enum crf_measure {
    CRF_PEARSON = 0,                 /* "pearson"   computePearson2<float>, Correlation.cpp:100-133 */
    CRF_SPEARMAN = 1,                /* "spearman"  computeRanks + computePearson2<float>, :277-303,:141-174 */
    CRF_KENDALL = 2,                 /* "kendall"   computeKendall<int32_t> (tau-b), :423-455 */
    CRF_MI_BINNED = 3,               /* "mi_binned" computeMutualInformationBinned<double>, MutualInformation.cpp:45-143 */
    CRF_MI_KRASKOV = 4,              /* "mi_kraskov" computeMutualInformationKraskov[2]<double>, :399-509 */
    CRF_BINNED_MI_CC = 5,            /* "binned_mi_correlation_coefficient"  sqrt(1-exp(-2 MI)), CorrelationCalculator.cpp:1071-1073 */
    CRF_KMI_CC = 6                   /* "kmi_correlation_coefficient"        same map, :1130-1132 */
} crf_measure;

enum {
    CRF_OK = 0,
    CRF_ERR_ARGUMENT = 1,   /* bad pointer / size / enum */
    CRF_ERR_STATE = 2,      /* grid or members not set */
    CRF_ERR_DEVICE = 3,     /* HIP error or no usable gfx950 device */
    CRF_ERR_UNSUPPORTED = 4 /* configuration outside what the kernels implement (message says which) */
};

/* One evaluation = the state CorrelationCalculator holds when calculateCpu runs
 * (CorrelationCalculator.hpp:200-213 and ICorrelationCalculator members :120-140). */
typedef struct crf_params {
    int32_t measure;                 /* crf_measure */
    int32_t ref_x, ref_y, ref_z;     /* referencePointIndex in LOCAL grid coordinates; used when reference_values==NULL */
    int32_t k;                       /* kmi_neighbors (Kraskov); default max(ceil(3*cs/100),1), CorrelationCalculator.cpp:592-598 */
    int32_t kraskov_estimator_index; /* 1 = KSG-1 (default), 2 = KSG-2 */
    int32_t num_bins;                /* mi_bins, default 80 (CorrelationCalculator.hpp:209) */
    float min_ref, max_ref;          /* binned MI: extrema used to normalise the reference vector (:820-833) */
    float min_query, max_query;      /* binned MI: extrema used to normalise each voxel's vector (:834-846,:1061-1062) */
    const float* reference_values;   /* HOST pointer to cs floats, or NULL.  Non-NULL = CorrelationFieldMode::SEPARATE
                                        / time-lag (reference vector taken from another field, :804-813) or a vector
                                        received from another rank. */
    int32_t flags;                   /* CRF_FLAG_* */
    int32_t prepared_slot;           /* 0: the evaluation prepares its reference-side tables itself.  s+1: use the
                                        tables crf_prepare_device left in slot s (the reference vector arguments are
                                        then not read; the other fields must equal those given to crf_prepare_device) */
    int32_t reserved[2];             /* must be 0 */
} crf_params;

/* |.| of the result.  Pair requests: useAbsoluteCorrelationMeasure (HEBChartCorrelation.cpp:583-585).  Full-grid
 * evaluations: OPT-IN -- the reference's calculateCpu ignores calculate_absolute_value (it is a shader define of the
 * accelerator paths only, CorrelationCalculator.cpp:1662-1664), so the C++ adapter never sets the flag; a caller that
 * wants the accelerator paths' behaviour sets it and gets |value| (NaN stays NaN). */
#define CRF_FLAG_ABSOLUTE_VALUE 1
/* CorrelationFieldMode::SEPARATE_SYMMETRIC (CorrelationCalculator.hpp:59-64): crf_compute[_device] evaluate, at every
 * voxel v, the measure between X[c] = member_c[v] (the reference field = the primary members) and Y[c] =
 * secondary_member_c[v] (the query field) -- `#define referencePointIdx currentPointIdx`, CorrelationMain.glsl:10-15;
 * scalarFieldsRef = scalarFields, scalarFieldsQuery = scalarFieldsSecondary, ScalarFields.glsl:107-117.  The
 * reference implements this mode on its Vulkan path only (CorrelationCalculator.cpp:1182-1229; calculateCpu falls into
 * the SINGLE branch), so the arithmetic here is DEFINED as calculateCpu's per-voxel computation with the reference
 * vector taken from the primary field at the same voxel; a NaN in either vector gives NaN; Kraskov is KSG-1 (the
 * shaders ignore the estimator index).  Binned MI normalises X with min_ref/max_ref and Y with min_query/max_query.
 * The reference point / reference_values are not read. */
#define CRF_FLAG_SYMMETRIC 2
/* CorrelationFieldMode::SEPARATE on the device: the reference vector is gathered from the SECONDARY members at
 * (ref_x, ref_y, ref_z) -- referenceValues[c] = field2_c[IDXS(ref)], CorrelationCalculator.cpp:804-813 (for time-lag
 * correlations bind the secondary field's members of the lagged time step). */
#define CRF_FLAG_REFERENCE_FROM_SECONDARY 4
/* Pair requests over two fields (crf_compute_requests*): the i side of every request reads the primary members, the j
 * side the SECONDARY members -- the request mode with setUseSecondaryFields(true) / setFieldBuffersSecondary
 * (CorrelationCalculator.hpp:255-257, HEBChartCorrelation.cpp:1164-1169; scalarFieldsRef / scalarFieldsQuery in
 * Data/Shaders/Correlation/ScalarFields.glsl:105-120).  Both member sets share the local grid. */
#define CRF_FLAG_QUERY_FROM_SECONDARY 8

/* One pair request: the estimator between the ensemble vectors of voxel (xi,yi,zi) and voxel (xj,yj,zj).  Same layout
 * as struct CorrelationRequestData {xi,yi,zi,i,xj,yj,zj,j} (src/Renderers/Diagram/HEBChart.hpp:166-168,
 * Data/Shaders/Correlation/RequestsBuffer.glsl:22-36); i and j (linear indices) are carried along, not read. */
typedef struct crf_request {
    uint32_t xi, yi, zi, i, xj, yj, zj, j;
} crf_request;

/* ---- lifetime ------------------------------------------------------------------------------------------- */
/* Creates a context bound to HIP device `device_ordinal`.  Fails (CRF_ERR_DEVICE) when the device is absent or is
 * not gfx950.  *out_ctx is set to NULL on failure; crf_last_error(NULL) then holds the message. */
int crf_create(int device_ordinal, crf_context** out_ctx);
void crf_destroy(crf_context* ctx);
/* Last error message of this context (or of the calling thread's last failed crf_create when ctx==NULL). */
const char* crf_last_error(const crf_context* ctx);
/* ABI version of this header, bumped on incompatible change. */
int crf_abi_version(void);  /* 5: crf_group_compute_batch[_device], crf_member_minmax_divergent; added since, compatibly:
                                  crf_upload_members_format, crf_bind_members_device_format, crf_member_format,
                                  crf_last_member_format, crf_wide_copy_bytes, crf_window_count,
                                  crf_upload_secondary_members_format, crf_bind_secondary_members_device_format,
                                  crf_secondary_member_format, crf_secondary_wide_copy_bytes, crf_field_similarity,
                                  crf_rank_values_device, crf_field_rank_similarity, crf_rank_scratch_bytes,
                                  crf_kendall_values_device, crf_field_kendall_similarity;
                               4: crf_group_* (several devices behind one caller thread), crf_set_kraskov_noise;
                               3: crf_params.reserved[0] became prepared_slot (same layout; 0 keeps the old meaning) */

/* ---- the ensemble (replaces the fields[] gather of CorrelationCalculator.cpp:791-800) --------------------- */
/* Declares the LOCAL grid (a whole grid, or this process's z-slab of one) and member count; drops any members. */
int crf_set_grid(crf_context* ctx, int xs, int ys, int zs, int cs);
/* The launches a per-voxel evaluation of the current local grid takes: 1 for an ordinary grid; 2 or more for a grid
 * whose fp32 member volume is 4 GiB or more, which is evaluated in windows of 2^29 voxels (the slower path: no native
 * narrow-format route, no packed Pearson copy, no range pipeline of crf_compute; pair requests and crf_tile_field_device
 * are refused).  Valid right after crf_set_grid; 0 if ctx == NULL.  (Tests set CRF_WINDOW_VOXELS, read by crf_set_grid,
 * to a positive multiple of 1024 to window a small grid: it is then windowed iff it has more voxels than that.) */
int crf_window_count(const crf_context* ctx);
/* Copies cs host volumes (each xs*ys*zs floats) into HBM owned by the context (the role the reference's LRU
 * field cache plays across reference-point moves, VolumeData.cpp:1202-1226). */
int crf_upload_members(crf_context* ctx, const float* const* host_members);
/* Uses cs caller-owned DEVICE volumes in place (borrowed until the next set_grid/upload/bind/destroy). */
int crf_bind_members_device(crf_context* ctx, const void* const* device_members);
/* ---- members in a narrow native format ---------------------------------------------------------------------------
 * The reference keeps scalar fields as float, unsigned byte, unsigned short or float16 (format_cast,
 * src/Loaders/DataSetList.cpp:185-195) and its calculators see them through HostCacheEntry::data<float>()
 * (src/Volume/Cache/HostCacheEntry.cpp:107-176); the value of an element is given below.  Members in such a format
 * stay as narrow in HBM as they are on the host.  Every entry point that reads the primary members gives exactly the
 * result of the same call on fp32 members that hold those values.
 *   - The Pearson field (CRF_PEARSON without CRF_FLAG_SYMMETRIC) at 2..128 members reads the narrow members directly
 *     (pearson_narrow_kernel); crf_last_member_format then returns the narrow format and crf_last_member_layout RAW
 *     (crf_set_member_layout has no effect on narrow members: the packed copy is an fp32 format).
 *   - The Kendall field (CRF_KENDALL without CRF_FLAG_SYMMETRIC) at 2..128 members reads the narrow members directly
 *     (kendall_narrow_kernel: one pass that sorts order-preserving keys of the stored codes, ties handled in line, no
 *     list of deferred voxels); crf_last_member_format then returns the narrow format.  It loads single elements, so it
 *     asks for the element's own alignment only (2 bytes for the 16-bit formats, none for uint8).  The reference side
 *     -- a reference point, a caller's host or device vector, CRF_FLAG_REFERENCE_FROM_SECONDARY, prepared slots --
 *     stays fp32 with any values.
 *   - The Spearman field (CRF_SPEARMAN without CRF_FLAG_SYMMETRIC) at 33..128 members reads the narrow members directly
 *     (spearman_narrow_kernel: the same sorted keys, fractional ranks of tie runs in line, no list of deferred voxels,
 *     whatever CRF_RANK_U32 says); crf_last_member_format then returns the narrow format.  Alignment and reference side
 *     as for the Kendall field.  At 2..32 members it takes the fp32 copy.
 *   - The binned mutual-information field (CRF_MI_BINNED, CRF_BINNED_MI_CC without CRF_FLAG_SYMMETRIC) reads the narrow
 *     members directly where that was measured to be no slower than the copy route -- uint8 at 2..128 members, uint16 at
 *     17..32 and 49..64, float16 at 49..64; other counts take the fp32 copy -- (mi_binned_narrow_kernel: one byte / short load per member; a uint8 code
 *     becomes its bin through a 256-entry table that each block fills from min_query, max_query and num_bins, a 16-bit
 *     code through the arithmetic of the fp32 kernel on its value); crf_last_member_format then returns the narrow
 *     format.  Alignment and reference side as for the Kendall field.
 *   - The Kraskov mutual-information field (CRF_MI_KRASKOV, CRF_KMI_CC without CRF_FLAG_SYMMETRIC; KSG-1 and KSG-2) reads
 *     the narrow members directly where that was measured to be no slower than the copy route
 *     (mi_kraskov_narrow_kernel, kraskov_direct_narrow_kernel: one byte / short load per member, the converted values or
 *     the codes parked in LDS, every operation behind them the fp32 kernel's in the fp32 kernel's order):
 *       (K = min(k, members - 1); "column plan": the LDS-column kernel, by default k = 2 up to 44 members, k = 3 up to 40)
 *       uint8    K = 2, 3 at 33..48 members under a column plan; K = 2 at 49..64, K = 3 at 49..96, K = 4 at 113..128,
 *                k = 5..8 at 49..64 and 113..128 members;
 *       uint16   K = 2, 3 at 49..64 members; K = 4 and k = 5..8 at 113..128;
 *       float16  K = 2 at 49..64, K = 3 at 49..64 and 113..128, K = 4 at 113..128, k = 5..8 at 49..64 and 113..128 members;
 *     every other (format, member count, k) takes the fp32 copy, as does CRF_KRASKOV_SORTED=1 where it selects the
 *     sorted-column kernel; the other CRF_KRASKOV_* switches move a native call as they move an fp32 call.
 *     crf_last_member_format then returns the narrow format.  Alignment and reference side as for the Kendall field;
 *     crf_set_kraskov_noise applies as on fp32 members.
 *   - The sibling reductions (crf_compute_ensemble_stat[_device], crf_compute_set_predicate[_device]) read the narrow
 *     members directly at any member count (ensemble_stat_narrow_kernel, set_predicate_narrow_kernel, reported by
 *     crf_last_kernel_name; crf_last_member_format speaks of field evaluations only and is left alone).  Like the
 *     Pearson field they load whole dwords, so borrowed members that are not all 4-byte aligned take the fp32 copy.
 *   - DKL (crf_compute_dkl[_device]) reads the narrow members directly where that was measured to be no slower than the
 *     copy route (dkl_narrow_kernel, reported by crf_last_kernel_name: one byte / short load per member, every operation
 *     behind it the fp32 kernel's in the fp32 kernel's order, so the result is bit-identical to the copy route's):
 *       binned estimator   uint8 and uint16 at 17..32 members; uint8 and float16 at 97..2048 members;
 *       k-NN estimator     uint8 and uint16 at 49..64 members with k <= 2; every format at 129..2048 members;
 *     every other (format, member count, estimator, k) takes the fp32 copy.  It loads single elements, so it asks for the
 *     element's own alignment only, as the Kendall field does.  CRF_DKL_COUNTING_SORT and CRF_DKL_BLOCKS_PER_CU move a
 *     native call as they move an fp32 call.  Like the other sibling reductions it leaves crf_last_member_format alone.
 *   - crf_member_minmax and the reference gathers (crf_gather_reference, crf_gather_reference_device,
 *     crf_gather_reference_rows_device) read the narrow members directly, whatever their alignment.
 *   - Everything else -- Spearman at 2..32 members, symmetric evaluations (but for the Pearson field over two narrow fields
 *     described with the secondary members below) and pair-request evaluations, and the
 *     Pearson, Spearman, Kendall, binned-MI and Kraskov-MI fields above 128 members (binned MI, Kraskov MI and DKL also at
 *     the counts named above) -- runs on an fp32 copy of the members that the context builds on the compute stream at the first
 *     call that needs it (one owned block of cs x xs*ys*zs floats; CRF_ERR_DEVICE naming the copy and its size if it
 *     cannot be allocated) and drops in crf_set_grid, upload, bind and crf_members_changed; crf_last_member_format then
 *     returns CRF_MEMBER_F32.  So do the Pearson field and the sibling reductions over borrowed members that are not all
 *     4-byte aligned.  A context that only runs the entry points of the eight items above never builds the copy;
 *     crf_wide_copy_bytes tells.
 *   - A local grid whose narrow member is 4 GiB or more: CRF_ERR_UNSUPPORTED.
 *     crf_group_* evaluations on a context that holds narrow members, primary or secondary: CRF_ERR_UNSUPPORTED.
 * Secondary members (crf_upload_secondary_members_format, crf_bind_secondary_members_device_format) stay as narrow in HBM
 * too, and every entry point that reads them gives exactly the result of the same call on fp32 secondary members that
 * hold those values:
 *   - crf_secondary_member_minmax, crf_member_minmax_divergent(secondary = 1) and the reference vector of
 *     CRF_FLAG_REFERENCE_FROM_SECONDARY read them directly, whatever their alignment; the rest of such an evaluation is
 *     that of the primary members (their native routes included).
 *   - The symmetric Pearson field (CRF_PEARSON with CRF_FLAG_SYMMETRIC) at 2..128 members reads BOTH fields directly when
 *     they are in the same narrow format, all members of both are 4-byte aligned and the grid is not windowed
 *     (pearson_symmetric_narrow_kernel, reported by crf_last_kernel_name: one lane owns the voxels of one dword, 2 cs e + 4
 *     bytes per voxel for elements of e bytes where the fp32 kernel moves 8 cs + 4); crf_last_member_format then returns
 *     the narrow format and neither fp32 copy is built.
 *   - Every other reader -- the symmetric mode for the other measures, for fields in different formats, for borrowed
 *     members that are not all 4-byte aligned, above 128 members and on windowed grids; pair requests with
 *     CRF_FLAG_QUERY_FROM_SECONDARY -- takes fp32 views: of the secondary members through an fp32 copy of their own (built
 *     at the first call that needs it, dropped by crf_set_grid, a secondary upload or bind and crf_members_changed;
 *     crf_secondary_wide_copy_bytes tells), of narrow primary members through theirs.  crf_last_member_format then
 *     returns CRF_MEMBER_F32.
 * format == CRF_MEMBER_F32 behaves exactly like crf_upload_members / crf_bind_members_device (and their secondary
 * counterparts), which set the format to CRF_MEMBER_F32.  An unknown format: CRF_ERR_ARGUMENT. */
enum crf_member_format { /* a tag only: the function crf_member_format() below shares the name */
    CRF_MEMBER_F32 = 0,
    CRF_MEMBER_U8 = 1,   /* value = float(b) / 255.0f */
    CRF_MEMBER_U16 = 2,  /* value = float(s) / 65535.0f */
    CRF_MEMBER_F16 = 3   /* value = float(h), IEEE binary16 */
};
int crf_upload_members_format(crf_context* ctx, int format, const void* const* host_members);
int crf_bind_members_device_format(crf_context* ctx, int format, const void* const* device_members);
int crf_member_format(const crf_context* ctx);      /* format of the bound primary members */
/* format the per-voxel kernel of the last field evaluation read: the members' own after a native Pearson, Kendall,
 * Spearman, binned-MI or Kraskov-MI field, CRF_MEMBER_F32 after anything that ran on fp32 members or on the fp32 copy */
int crf_last_member_format(const crf_context* ctx);
/* bytes of the fp32 copy of narrow members held right now; 0 if none or ctx == NULL (the native Pearson, Kendall,
 * Spearman, binned-MI and Kraskov-MI fields, the sibling reductions, DKL where it is read natively, the extrema and the
 * gathers never build it) */
size_t crf_wide_copy_bytes(const crf_context* ctx);
/* min of per-member minima / max of per-member maxima over the local grid (CorrelationCalculator.cpp:822-829 on
 * top of VolumeData::getMinMaxScalarFieldValue, VolumeData.cpp:1632-1670); computed on the device, cached until
 * the members change. */
int crf_member_minmax(crf_context* ctx, float* out_min, float* out_max);
/* The same extrema for a field the reference flags as DIVERGENT (VolumeData::getIsScalarFieldDivergent,
 * VolumeData.cpp:616-621: the field named "Helicity"): getMinMaxScalarFieldValue centres its range at zero,
 * min = -max|.|, max = +max|.| (VolumeData.cpp:1661-1666), per member -- and the min of the mins / max of the maxes the
 * calculator takes (CorrelationCalculator.cpp:822-829) is then -A / +A with A = max(|min|, |max|) over all members.
 * secondary != 0: the secondary members.  The caller decides whether a field is divergent (it knows the field's name). */
int crf_member_minmax_divergent(crf_context* ctx, int secondary, float* out_min, float* out_max);
/* The second scalar field of the SEPARATE / SEPARATE_SYMMETRIC field modes (fieldIndex2Gui; fieldEntriesSecondary,
 * CorrelationCalculator.cpp:1182-1229): cs volumes of the same local grid, uploaded or borrowed like the primary
 * members; dropped by crf_set_grid.  Used by CRF_FLAG_SYMMETRIC / CRF_FLAG_REFERENCE_FROM_SECONDARY. */
int crf_upload_secondary_members(crf_context* ctx, const float* const* host_members);
int crf_bind_secondary_members_device(crf_context* ctx, const void* const* device_members);
int crf_secondary_member_minmax(crf_context* ctx, float* out_min, float* out_max);
/* ... in a narrow native format (see "members in a narrow native format" above) */
int crf_upload_secondary_members_format(crf_context* ctx, int format, const void* const* host_members);
int crf_bind_secondary_members_device_format(crf_context* ctx, int format, const void* const* device_members);
int crf_secondary_member_format(const crf_context* ctx);      /* format of the bound secondary members */
/* bytes of the fp32 copy of narrow secondary members held right now; 0 if none or ctx == NULL */
size_t crf_secondary_wide_copy_bytes(const crf_context* ctx);

/* ---- reference vector (CorrelationCalculator.cpp:802,815-817) --------------------------------------------- */
/* referenceValues[c] = member_c[IDXS(x,y,z)] -> cs floats to a host buffer (synchronous) ... */
int crf_gather_reference(crf_context* ctx, int x, int y, int z, float* host_out);
/* ... or to a device buffer, asynchronously on `stream` (a hipStream_t, NULL = the context's own stream). */
int crf_gather_reference_device(crf_context* ctx, int x, int y, int z, void* device_out, void* stream);

/* Batched form for the multi-GPU exchange: row r of device_rows (num_rows x cs floats, num_rows <= 32) receives the
 * reference values of LOCAL grid point (xyz[3r], xyz[3r+1], xyz[3r+2]), or zeros when xyz[3r+2] < 0 (a point whose
 * z-slice another process owns) -- so that one all-reduce(sum) over the processes yields every row everywhere. */
int crf_gather_reference_rows_device(crf_context* ctx, const int32_t* xyz, int num_rows, void* device_rows, void* stream);

/* ---- Kraskov tie-breaking noise ------------------------------------------------------------------------------------
 * The KSG estimators add `u * 1e-10`, u drawn per member from sgl::XorshiftRandomGenerator(617406168) for the reference
 * vector and (864730169) for every query vector, to break exact ties (MutualInformation.cpp:409-420, 167-185).  sgl is
 * not vendored by the reference and not available to this build, so the library's DEFAULT tables come from a
 * documented stand-in stream (Marsaglia xorshift32) -- results on exactly tied data then differ from a
 * reference build in the last digits.  An integrator who has sgl passes the real stream here: ref_noise[e] and
 * query_noise[e] are the noise VALUES (already multiplied by 1e-10, as double) of member e, cs of each; both NULL
 * restores the default.  Applies to every later Kraskov evaluation of this context (field, symmetric and pair-request
 * modes) until the next crf_set_grid.  Stream-ordered on the context's own stream; call it between evaluations. */
int crf_set_kraskov_noise(crf_context* ctx, const double* ref_noise, const double* query_noise);

/* ---- evaluation (replaces the hot loop CorrelationCalculator.cpp:868-1142) ------------------------------- */
/* Synchronous, host output: what calculateCpu(t, e, buffer) does.  host_out receives xs*ys*zs floats.
 * Member counts: the Pearson field (no CRF_FLAG_SYMMETRIC) takes any cs; every other measure and mode, here, in the
 * *_device forms and in crf_compute_requests, takes at most 2048 members and returns CRF_ERR_UNSUPPORTED beyond. */
int crf_compute(crf_context* ctx, const crf_params* params, float* host_out);
/* Asynchronous, device output, stream-ordered, no host synchronisation: the form the multi-GPU path and the
 * benchmark use.  device_reference_values: DEVICE pointer to cs floats or NULL (then params->reference_values or
 * the reference point are used).  device_out receives xs*ys*zs floats. */
int crf_compute_device(crf_context* ctx, const crf_params* params, const void* device_reference_values,
                       void* device_out, void* stream);

/* Two-phase form for pipelined callers (the multi-GPU driver): crf_prepare_device runs only the reference-side
 * preparation of an evaluation (the reference-derived tables: Pearson/Spearman a_e, Kendall's x order and tie groups,
 * binned reference bins, Kraskov's noisy reference coordinates) into slot `slot` (0 <= slot < CRF_PREPARED_SLOTS), e.g.
 * on a communication stream right after the reference vectors arrive; a later crf_compute_device with
 * params->prepared_slot = slot + 1 launches only the per-voxel kernel.  The caller orders the two calls (same stream
 * or an event) and must not re-prepare a slot before the evaluation that reads it has been launched and ordered. */
#define CRF_PREPARED_SLOTS 64
int crf_prepare_device(crf_context* ctx, const crf_params* params, const void* device_reference_values, int slot,
                       void* stream);

/* crf_prepare_device for `count` reference vectors with ONE call: row i of device_rows (cs floats each, contiguous rows --
 * e.g. the buffer crf_gather_reference_rows_device filled and an all-reduce completed) is prepared into slot
 * first_slot + i.  params: the evaluation's settings (reference point and reference_values are not read). */
int crf_prepare_rows_device(crf_context* ctx, const crf_params* params, const void* device_rows, int first_slot, int count,
                            void* stream);
/* Launches `count` prepared evaluations back to back with ONE call: evaluation i reads the tables crf_prepare_device left
 * in slot first_slot + i and writes device_outs[i] (params: as given to crf_prepare_device, prepared_slot is ignored).
 * The host-side cost of a pipelined driver then is one call per batch instead of one per evaluation -- at 8 GPUs a
 * 256^3 x 64 evaluation is 0.09 ms per device, the same order as a Python-level call. */
int crf_compute_prepared_device(crf_context* ctx, const crf_params* params, int first_slot, int count,
                                void* const* device_outs, void* stream);

/* ---- several GPUs behind ONE caller thread ------------------------------------------------------------------------
 * The reference is a single process that calls its calculators from the render thread with a caller-owned host buffer
 * (src/Volume/VolumeData.cpp:1214-1226, 1469-1472).  A crf_group gives such a caller N devices: the GLOBAL grid is cut
 * into z-slabs (the first zs % N slabs one slice longer -- with x-fastest volumes a slab of every member is contiguous
 * and the result slabs concatenate in the caller's buffer), each device keeps its slab of every member resident in its
 * own HBM and is driven by its own worker thread inside the library, and every evaluation has one exchange step: the
 * device whose slab holds the reference point (the owner) has the cs reference values
 * (CorrelationCalculator.cpp:802,815-817).  By default every other device READS them directly out of the owner's member
 * volumes -- peer access over xGMI, fused into its reference-side preparation kernel: no collective, no copy, no
 * rendezvous.  CRF_GROUP_EXCHANGE=rccl (and the default when some pair of devices lacks peer access): the owner gathers
 * and ncclBroadcast distributes them on a persistent single-process RCCL communicator.  CRF_GROUP_EXCHANGE=copy: staged
 * peer copies.  crf_group_exchange() names the form in use.  Each device then evaluates its slab and copies it straight
 * into its part
 * of the caller's buffer (the copies of the N devices run concurrently).  Results are bit-identical to a single
 * context's.  Same conventions as above: one caller thread, status codes, crf_group_last_error. */
typedef struct crf_group crf_group;
int crf_group_create(const int* device_ordinals, int num_devices, crf_group** out_group);
void crf_group_destroy(crf_group* group);
const char* crf_group_last_error(const crf_group* group);   /* group == NULL: last failed crf_group_create of this thread */
int crf_group_size(const crf_group* group);
/* "peer read (...)", "rccl (...)", "peer copy (...)" or "none (one device)": how the reference vector travels. */
const char* crf_group_exchange(const crf_group* group);
/* The context that drives device slot `slot` (its LOCAL grid is the slab): for per-device helpers such as
 * crf_bind_members_device or crf_last_kernel_name.  Owned by the group. */
crf_context* crf_group_context(crf_group* group, int slot);
/* Declares the GLOBAL grid and member count (zs >= number of devices); drops any members. */
int crf_group_set_grid(crf_group* group, int xs, int ys, int zs, int cs);
int crf_group_slab(const crf_group* group, int slot, int* z_begin, int* z_count);
/* cs host volumes of the WHOLE grid; every device uploads its slab of each (concurrently). */
int crf_group_upload_members(crf_group* group, const float* const* host_members);
int crf_group_upload_secondary_members(crf_group* group, const float* const* host_members);
/* Extrema over all slabs (binned-MI normalisation range, CorrelationCalculator.cpp:822-829). */
int crf_group_member_minmax(crf_group* group, float* out_min, float* out_max);
int crf_group_secondary_member_minmax(crf_group* group, float* out_min, float* out_max);
/* calculateCpu(t, e, buffer) on N devices: params as for crf_compute with the reference point in GLOBAL coordinates;
 * host_out receives xs*ys*zs floats.  Supports the reference point, a host reference vector (no exchange),
 * CRF_FLAG_REFERENCE_FROM_SECONDARY, CRF_FLAG_SYMMETRIC (no exchange) and CRF_FLAG_ABSOLUTE_VALUE. */
int crf_group_compute(crf_group* group, const crf_params* params, float* host_out);
/* The same evaluation with DEVICE-resident results (what crf_compute_device is to crf_compute): device_outs[slot] is a
 * buffer on the device of that slot and receives the slot's slab, xs*ys*z_count floats (crf_group_slab); returns when
 * every device has finished.  For consumers that keep the field on the GPUs. */
int crf_group_compute_device(crf_group* group, const crf_params* params, void* const* device_outs);
/* MANY reference points per call -- a diagram or an animation that evaluates a list of points (the reference's
 * HEBChart / time-series consumers call calculateCpu point after point from the same thread): params[i] as for
 * crf_group_compute, evaluation i writes host_outs[i] (xs*ys*zs floats each).  One hand-off to the device workers for
 * the whole list; the reference vectors of up to 32 points travel in ONE collective (owners fill their rows, one
 * ncclAllReduce(sum)) or are read directly from the owner's members (peer exchange). */
int crf_group_compute_batch(crf_group* group, const crf_params* params, int count, float* const* host_outs);
/* ... with device-resident results: device_outs[i * crf_group_size(group) + slot] receives the slab of slot `slot` of
 * evaluation i.  Per device the reference-side preparations of a block of evaluations run first, the per-voxel kernels
 * follow back to back and the workers synchronise once, at the end of the call. */
int crf_group_compute_batch_device(crf_group* group, const crf_params* params, int count, void* const* device_outs);
int crf_group_set_profiling(crf_group* group, int enabled);
/* Slowest device's summed kernel time (ms) and its launch count since the last call. */
int crf_group_take_kernel_time(crf_group* group, double* out_ms_max, int* out_launches);
/* crf_set_kraskov_noise on every device of the group. */
int crf_group_set_kraskov_noise(crf_group* group, const double* ref_noise, const double* query_noise);

/* ---- pair-request evaluation (CorrelationComputePass request mode, CorrelationCalculator.hpp:250-258; CPU twin
 * HEBChart::computeCorrelations, src/Renderers/Diagram/HEBChartCorrelation.cpp:493-600) ---------------------------- */
/* out[r] = measure(X_r, Y_r) with X_r[c] = member_c[IDXS(xi,yi,zi)], Y_r[c] = member_c[IDXS(xj,yj,zj)].  Semantics of the
 * CPU twin: Pearson/Spearman/Kendall as in the full-grid path but with both vectors per request; binned MI normalises
 * both vectors with the extrema of the pair (:556-566); Kraskov is KSG-1; MI-CC variants map sqrt(1-exp(-2 MI));
 * CRF_FLAG_ABSOLUTE_VALUE takes |.|; a NaN in either vector gives NaN (the CPU twin emits no entry for that pair).
 * CRF_FLAG_QUERY_FROM_SECONDARY: the j side reads the secondary members (two-field request mode).
 * Read from params: measure, k, num_bins, flags. */
int crf_compute_requests(crf_context* ctx, const crf_params* params, const crf_request* host_requests,
                         size_t num_requests, float* host_out);
int crf_compute_requests_device(crf_context* ctx, const crf_params* params, const void* device_requests,
                                size_t num_requests, void* device_out, void* stream);

/* ---- sibling per-voxel ensemble reductions (same access pattern) ------------------------------ */
typedef enum crf_ensemble_stat {
    CRF_ENSEMBLE_MEAN = 0,   /* EnsembleMeanCalculator::calculateCpu,   src/Calculators/EnsembleMeanCalculator.cpp:94-138 */
    CRF_ENSEMBLE_SPREAD = 1  /* EnsembleSpreadCalculator::calculateCpu, src/Calculators/EnsembleSpreadCalculator.cpp:94-149 */
} crf_ensemble_stat;
/* NaN-skipping mean / sample standard deviation over the cs members at every voxel; xs*ys*zs floats out. */
int crf_compute_ensemble_stat(crf_context* ctx, int stat, float* host_out);
int crf_compute_ensemble_stat_device(crf_context* ctx, int stat, void* device_out, void* stream);

/* SetPredicateCalculator::calculateCpu (src/Calculators/SetPredicateCalculator.cpp:154-210): count = number of members
 * with `value OP comparison_value`; out = clamp(count - count_lower, 0, 1) when count_lower == count_upper, else
 * clamp((count - count_lower) / (count_upper - count_lower), 0, 1), all in fp32.  Operator values follow
 * ComparisonOperatorType (SetPredicateCalculator.hpp:41-43); NaN compares as in C. */
typedef enum crf_comparison_operator {
    CRF_CMP_GREATER = 0, CRF_CMP_GREATER_EQUAL = 1, CRF_CMP_LESS = 2, CRF_CMP_LESS_EQUAL = 3, CRF_CMP_EQUAL = 4,
    CRF_CMP_NOT_EQUAL = 5
} crf_comparison_operator;
int crf_compute_set_predicate(crf_context* ctx, int comparison_operator, float comparison_value, int count_lower,
                              int count_upper, float* host_out);
int crf_compute_set_predicate_device(crf_context* ctx, int comparison_operator, float comparison_value, int count_lower,
                                     int count_upper, void* device_out, void* stream);

/* DKLCalculator::calculateCpu (src/Calculators/DKLCalculator.cpp:134-262): Kullback-Leibler divergence between the
 * normalised distribution of the cs member values of a voxel and N(0,1).  Estimators (DKLEstimatorType,
 * DKLCalculator.hpp:39-41): binned = computeDKLBinned<double> (DKL.cpp:38-84, num_bins in [1, 1024], default 80),
 * entropy k-NN = computeDKLKNNEstimate<double> (DKL.cpp:98-165, 1 <= k < cs, default max(ceil(3 cs / 100), 1),
 * DKLCalculator.cpp:94-101).  cs == 1 -> 1; a NaN member -> NaN; at most 2048 members. */
typedef enum crf_dkl_estimator { CRF_DKL_BINNED = 0, CRF_DKL_ENTROPY_KNN = 1 } crf_dkl_estimator;
int crf_compute_dkl(crf_context* ctx, int estimator, int num_bins, int k, float* host_out);
int crf_compute_dkl_device(crf_context* ctx, int estimator, int num_bins, int k, void* device_out, void* stream);

/* ---- whole-field similarity of two fields ------------------------------------------------------------------------------
 * Whole-field similarity (src/Calculators/Similarity.cpp:36-180, the <double> instantiation): one value of `measure`
 * over the samples (primary[c][v], secondary[c][v]) -- every voxel v of every member c (member == -1) or of member
 * `member` alone; a pair with a NaN on either side is left out.  *out_samples = the number of pairs kept.
 * It backs the reference's "Field Similarity" dialog (MainApp.cpp:1608-1618) and every cell of its correlation-matrix
 * chart (CorrelationMatrixRenderer.cpp:91-101); INTEGRATION.md maps useAllTimeSteps / useAllEnsembleMembers onto it.
 * Synchronous on the context's own stream; both fields stay where they are in HBM.
 *   CRF_PEARSON        computePearsonParallel<double> (Correlation.cpp:182-268): means, then centred second moments, all
 *                      accumulated in fp64, the result cast to float; here Sxy / (sqrt(Sxx) sqrt(Syy)) from two streaming
 *                      passes (similarity_moments_kernel).  The reference sums under an OpenMP reduction, so bit identity
 *                      with it is not defined; this library's value is bitwise reproducible from call to call (fixed
 *                      summation order, no floating-point atomics) and the same for 16-byte-aligned and merely 4-byte-
 *                      aligned borrowed members.  No pair kept: 0; one pair, or a constant side: NaN (a constant side
 *                      centres to exactly 0 while N x value is exact in fp64: up to 2^29 samples at least).
 *   CRF_MI_BINNED      computeMutualInformationBinned<double> (MutualInformation.cpp:45-143) on x01 = (x - min_x) /
 *                      (max_x - min_x), y01 likewise, formed in IEEE fp32; bin = clamp(int(double(x01) * num_bins), 0,
 *                      num_bins - 1) as the x86-64 build converts it (an out-of-range product lands in bin 0).  Ranges
 *                      (0, 1, 0, 1) are the reference's call verbatim (Similarity.cpp:163 passes raw values; it fixes 80
 *                      bins); the fields' extrema (crf_member_minmax, crf_secondary_member_minmax) give a meaningful
 *                      number.  The joint histogram (similarity_histogram_kernel) holds integer counts, so it does not
 *                      depend on the order of accumulation; everything after the counts is the reference's arithmetic in
 *                      the reference's loop order, in fp64 with the host's log.  num_bins in [1, 128] (read by the binned
 *                      measures only).
 *                      ONE DELIBERATE DEVIATION: the reference forms EPSILON_2D = 0.5 / Real(es * es) with an int product
 *                      (MutualInformation.cpp:121) that overflows from 46 341 samples on -- its object code returns NaN at
 *                      46 341 samples and H(x) + H(y), the joint term dropped, at 65 536, 262 144 and 2^20.  This library
 *                      forms the product in fp64: bit-identical to the object code up to 46 340 samples, well defined beyond.
 *   CRF_BINNED_MI_CC   sqrt(1 - exp(-2 MI)) of that float (Similarity.cpp:165-167).
 *   CRF_SPEARMAN, CRF_KENDALL, CRF_MI_KRASKOV, CRF_KMI_CC: CRF_ERR_UNSUPPORTED -- they need a global sort or a k-nearest-
 *                      neighbour search over all N samples.  Spearman and Kendall have entry points of their own:
 *                      crf_field_rank_similarity and crf_field_kendall_similarity below.  Kraskov MI over all samples is
 *                      not served.
 * Refusals (the context stays usable): no secondary members CRF_ERR_STATE; member outside [-1, cs) or num_bins outside
 * [1, 128] CRF_ERR_ARGUMENT; a windowed grid (crf_window_count > 1), or more than 2^31 - 1 candidate samples (the
 * reference counts samples in an int), CRF_ERR_UNSUPPORTED.  Members in a narrow format are read through their fp32
 * copies (crf_wide_copy_bytes, crf_secondary_wide_copy_bytes).  crf_last_kernel_name reports similarity_moments_kernel or
 * similarity_histogram_kernel; crf_set_profiling covers the call's launches with one event pair. */
int crf_field_similarity(crf_context* ctx, int measure, int member, int num_bins,
                         float min_x, float max_x, float min_y, float max_y,
                         float* out_value, unsigned long long* out_samples /* may be NULL */);

/* ---- ranks over all samples: a device-wide sort ----------------------------------------------------------------------------
 * crf_rank_values_device: fractional ranks of `count` fp32 values on the device, in input order -- computeRanks
 * (Correlation.cpp:277-303) -- by a device-wide radix sort (similarity_rank_sort_kernel and its siblings,
 * kernels_rank_similarity.hip).  count at most 2^31 - 1; device_ranks holds count floats and must not overlap the input.
 * Values compare as floats: -0 and +0 are equal, +-inf are ordinary values, the order among equal values does not matter.
 * A run of m equal values whose first 1-based position in sorted order is s gets fl32(float(s) + float(m - 1) * 0.5f): one
 * fp32 addition, no contraction.  That is the reference bit for bit up to 2^24 values (half ranks are rounded, not exact,
 * from 2^23 on, there as here).
 * ONE DELIBERATE DEVIATION: the reference carries s as an fp32 running sum (currentRank += float(numEqualValues)), which
 * stops counting runs of one at 2^24; beyond 2^24 values its ranks are wrong (first seen at 2^24 + 4096 values).  This
 * library forms s as an exact integer and rounds it once.
 * A NaN gets rank NaN and is not ranked (the reference never ranks one: its gather removes them first); *out_ranked = the
 * number of values ranked.  Synchronous on the context's own stream.
 *
 * crf_field_rank_similarity: the whole-field similarity by a rank measure (Similarity.cpp:134-143, the <double>
 * instantiation), over the samples crf_field_similarity takes: every voxel of every member (member == -1) or of member
 * `member`, pairs with a NaN on either side left out.
 *   CRF_SPEARMAN   ranks of the kept x and of the kept y separately (as above), then the Pearson value of the two rank
 *                  arrays by the moments path of crf_field_similarity: Sxy / (sqrt(Sxx) sqrt(Syy)) in fp64 with a fixed
 *                  order, cast to float; bitwise reproducible from call to call.  No pair kept: 0; one pair, or a constant
 *                  side: NaN.
 *   CRF_KENDALL    CRF_ERR_UNSUPPORTED: it needs an inversion count over all samples on top of the sort.  That is what
 *                  crf_field_kendall_similarity (below) does; this call keeps its refusal.
 *   every other measure: CRF_ERR_ARGUMENT (crf_field_similarity serves Pearson and binned MI).
 * Refusals as for crf_field_similarity (the context stays usable): no secondary members CRF_ERR_STATE; member outside
 * [-1, cs) CRF_ERR_ARGUMENT; a windowed grid, or more than 2^31 - 1 candidate samples, CRF_ERR_UNSUPPORTED.  Narrow
 * members are read through their fp32 copies.  crf_last_kernel_name reports similarity_rank_sort_kernel; crf_set_profiling
 * covers all launches of a call with one event pair.
 *
 * Scratch: the sort works in a buffer the context owns, grown on demand and released by crf_set_grid and crf_destroy
 * (it is not part of the grid workspace: it can be tens of GiB).  crf_rank_values_device takes 16 bytes per value (a
 * ping-pong of key and payload), crf_field_rank_similarity 24 bytes per candidate sample (the same, and the two rank
 * arrays, which first hold the masked samples: nothing is compacted, a pair with a NaN is carried as (NaN, NaN)), both
 * plus about 1 MiB of tables and count / 512 bytes.  A failed allocation gives CRF_ERR_DEVICE with the byte count in the
 * message.  crf_rank_scratch_bytes: what the buffer currently holds, 0 before first use. */
int crf_rank_values_device(crf_context* ctx, const void* device_values, size_t count,
                           void* device_ranks /* count floats, must not overlap the input */,
                           unsigned long long* out_ranked /* may be NULL */);
int crf_field_rank_similarity(crf_context* ctx, int measure, int member,
                              float* out_value, unsigned long long* out_samples /* may be NULL */);
size_t crf_rank_scratch_bytes(const crf_context* ctx);

/* ---- Kendall's tau-b over all samples: two sorts and an inversion count -----------------------------------------------------
 * computeKendall<int64_t> (Correlation.cpp:423-455), which computeFieldSimilarity<double> calls for CRF_KENDALL
 * (Similarity.cpp:134-143), bit for bit at every size.  Over the pairs (x_i, y_i) without a NaN on either side, n of them:
 *   n0 = n (n - 1) / 2
 *   n1 = the sum of m (m - 1) / 2 over the runs of m equal x;  n2 = the same over y.  Values compare as floats: -0 and +0
 *        are equal, +-inf are ordinary values.  Joint ties stay 0, as in the reference -- which is why the value differs
 *        from SciPy's tau-b on tied data.
 *   S  = the strict inversions of the y sequence in the order of std::sort on pair<float, float>: x ascending, y ascending
 *        among equal x; the pairs i < j of that order with y_j < y_i
 *   value = float(double(n0 - n1 - n2 - 2 S) / (sqrt(double(n0 - n1)) * sqrt(double(n0 - n2))))
 * evaluated as written on the host (crf_similarity_tail.h) from integers the device counts exactly
 * (kernels_kendall_similarity.hip: the device-wide radix sort by y, then by x, a tile kernel and merge levels that count
 * inversions; integer atomics only).  No tolerance is involved and the result is the same from call to call.  No special
 * cases: no pair kept or one gives 0 / 0 = NaN, a constant side NaN or +-inf, as IEEE gives them.  out_counts (may be
 * NULL) receives n0, n1, n2, S.
 *
 * crf_kendall_values_device: two fp32 device arrays of `count` values, count at most 2^31 - 1.  The inputs are only read
 * and may be the same array.  count == 0: NaN, 0 kept, no device work.  *out_kept = n.  Synchronous on the context's own
 * stream.
 *
 * crf_field_kendall_similarity: over the samples crf_field_similarity takes: every voxel of every member (member == -1) or
 * of member `member`.  Refusals as for crf_field_rank_similarity, with the same codes (the context stays usable): no
 * secondary members CRF_ERR_STATE; member outside [-1, cs) CRF_ERR_ARGUMENT; a windowed grid, or more than 2^31 - 1
 * candidate samples, CRF_ERR_UNSUPPORTED.  Narrow members are read through their fp32 copies.  *out_samples = n.
 *
 * Both: crf_last_kernel_name reports similarity_kendall_merge_kernel; crf_set_profiling covers all launches of a call with
 * one event pair.  Scratch is the sort's buffer (above: grown on demand, reported by crf_rank_scratch_bytes, released by
 * crf_set_grid and crf_destroy): 16 bytes per value or candidate sample (the ping-pong of key and payload, which also
 * holds the masked samples of the field call and the buffers of the merge levels: nothing is compacted), plus about
 * 1 MiB of tables and less than count / 64 bytes (the heads of the tiles, the cuts of the merge chunks). */
int crf_kendall_values_device(crf_context* ctx, const void* device_x, const void* device_y, size_t count,
                              float* out_value, long long* out_counts /* 4: n0, n1, n2, S; may be NULL */,
                              unsigned long long* out_kept /* may be NULL */);
int crf_field_kendall_similarity(crf_context* ctx, int member, float* out_value,
                                 long long* out_counts /* 4: n0, n1, n2, S; may be NULL */,
                                 unsigned long long* out_samples /* may be NULL */);

/* ---- result layout for the renderer -------------------------------------------------------------------------------- */
/* The reference keeps device fields in 8x8x4 tiles (bufferTileSize, VolumeData.cpp:1581-1621; addressed by IDXS of
 * Data/Shaders/Correlation/ScalarFields.glsl:32-50): tiles in x-fastest order, x-fastest inside a tile, grid padded up
 * to whole tiles with zeros.  crf_tiled_element_count = ceil(xs/8)*ceil(ys/8)*ceil(zs/4)*256 floats;
 * crf_tile_field_device re-lays a linear (IDXS) device field of the context's grid into that layout, stream-ordered. */
size_t crf_tiled_element_count(int xs, int ys, int zs);
int crf_tile_field_device(crf_context* ctx, const void* device_linear, void* device_tiled, void* stream);

/* Upper bound of the KSG estimate used for the colour range of the diagrams:
 * computeMaximumMutualInformationKraskov(k, es) = psi(es) - psi(k) (MutualInformation.cpp:526-528); psi(n) = -gamma + H_{n-1}.
 * Host-only helper, no context needed; NaN for k < 1 or cs < 1. */
double crf_max_mutual_information_kraskov(int k, int cs);

/* ---- member layout of the Pearson field ---------------------------------------------------------------------------
 * At 17..128 members the Pearson field can stream its members from a lossless packed copy in HBM (3.5 bytes per member
 * SLOT, the member count rounded up to 16, + 1 byte per slot and 64 voxels: 225 B per voxel at 64 members instead of 256,
 * but 112.5 B at 17 instead of 68; values whose 64-voxel segment does not fit the format are read from the members
 * themselves), built on the compute stream at the first Pearson field evaluation after the members change.  Results are
 * bit-identical.
 *   AUTO    (default) packs when 17 <= cs <= 128, the copy moves at most 92.5 % of the bytes of the members per
 *           evaluation (31-32, 48, 61-64, 79-80, 92-96, 109-112, 122-128 members), the grid has at least 2^20 voxels,
 *           no more than 5 % of the member segments fall back, and at least max(8 GiB, 10 % of the device memory)
 *           stays free; else RAW
 *   RAW     never packs
 *   PACKED  packs whenever the member count allows it (tests)
 * The copy is dropped by crf_set_grid, crf_upload_members, crf_bind_members_device and crf_set_member_layout.  The
 * library cannot see writes into BORROWED members (crf_bind_members_device): after changing their contents, call
 * crf_members_changed (or bind them again) before the next evaluation.  crf_members_changed drops everything derived
 * from the members (packed copy, cached extrema, pointer tables).  crf_last_member_layout: the layout the last Pearson
 * field evaluation read (CRF_MEMBER_LAYOUT_RAW or CRF_MEMBER_LAYOUT_PACKED). */
typedef enum crf_member_layout {
    CRF_MEMBER_LAYOUT_AUTO = 0,
    CRF_MEMBER_LAYOUT_RAW = 1,
    CRF_MEMBER_LAYOUT_PACKED = 2
} crf_member_layout;
int crf_set_member_layout(crf_context* ctx, int mode);
int crf_last_member_layout(const crf_context* ctx);
int crf_members_changed(crf_context* ctx);

/* ---- instrumentation --------------------------------------------------------------------------------------- */
/* When enabled, every crf_compute* brackets its dominant (per-voxel) kernel with HIP events on the launch stream. */
int crf_set_profiling(crf_context* ctx, int enabled);
/* Sum of the recorded kernel durations (ms) and their count since the last call; synchronises the events.  Resets. */
int crf_take_kernel_time(crf_context* ctx, double* out_ms_sum, int* out_launches);
/* Name of the dominant kernel of the last compute (for matching rocprofv3 rows), valid until the next call. */
const char* crf_last_kernel_name(const crf_context* ctx);
/* Fills device memory with a deterministic synthetic "box ensemble" member volume (recipe of the
 * reference's scripts/generate_synth_box_ensembles.py:57-136) for a z-slab [z_begin, z_begin+zs_local) of a global
 * xs*ys*zs_global grid: member `c` of `cs`.  Benchmark/test input generation only; not on the timed path. */
int crf_synth_box_member(crf_context* ctx, void* device_out, int xs, int ys, int zs_local, int z_begin, int zs_global,
                         int c, int cs, uint64_t seed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CORRFIELD_H */
