/*
 * swiftly_hip.h -- C ABI of libswiftly_hip.so, the MI355X (gfx950) native
 * implementation of the SwiFTly facet<->subgrid primitives.
 *
 * Drop-in boundary.  The reference (ska_sdp_exec_swiftly 1.0.0) reaches its
 * native backend through
 *     ska_sdp_func.fourier_transforms.swiftly.Swiftly(N, yN_size, xM_size, W)
 * (src/ska_sdp_exec_swiftly/fourier_transform/core.py:508-510) and then calls
 * one method per primitive on 2-D arrays, always along the LAST axis, passing
 * transposed views for axis 0 (core.py:577-630).  Every entry point below
 * replaces exactly one of those methods and keeps its contract: a batch of
 * `rows` independent 1-D problems along an axis with arbitrary element
 * strides (so "pass a .T view" becomes "swap the two strides"), overwrite
 * for the operations the reference allocates with numpy.empty and
 * ACCUMULATE for the ones it allocates with numpy.zeros (core.py:685, 714,
 * 743, 871, 896, 922).
 *
 * Conventions
 *  - plain C, no C++/torch types; all array pointers are DEVICE pointers
 *    (HIP), `stream` is a hipStream_t passed as void* (NULL = default stream);
 *    work is enqueued asynchronously on that stream.
 *  - dtype: SWIFTLY_C64 (interleaved float re,im) or SWIFTLY_C128.
 *  - element (r, i) of an array lives at base + r*row_stride + i*col_stride,
 *    strides counted in complex elements.  (transform length)*col_stride
 *    must be < 2^32.
 *  - offsets are in full-resolution pixels exactly as in the reference
 *    (facet_off a multiple of N/xM, subgrid_off a multiple of N/yN); they may
 *    be negative or >= N.
 *  - return value 0 = success; non-zero = failure, message available from
 *    swiftly_hip_last_error() (thread local).  Nothing throws across the ABI.
 *  - transform lengths (yN, xM, m = xM*yN/N): powers of two from 4 to 32768 run on native kernels in both
 *    precisions (complex128 up to 8192 along a unit-stride axis); 65536 is supported in complex64 for prepare_* /
 *    finish_* along a unit-stride axis and along the strided axis of contiguous rows.  Lengths Q * 2^k with
 *    Q in {3, 5, 7, 9} -- every other length of the reference's parameter catalogue, yN up to 57344 -- run natively
 *    too: one radix-Q pass in front of the power-of-two kernels (2^k <= 32768 in complex64, <= 8192 in complex128;
 *    rows * length < 2^32 per call).  Any other length goes through a Bluestein fallback on the power-of-two kernels
 *    (correct, ~10x the traffic) as long as 2^ceil(log2(2n-1)) <= 65536 (complex64) / 8192 (complex128); beyond
 *    that the call returns SWIFTLY_ERR_UNSUPPORTED (handle creation still succeeds).
 *  - a handle is immutable after creation and may be used concurrently from
 *    several host threads / streams (the reference scatters one core object
 *    to all Dask worker threads, api.py:145-147).  Handles may be created
 *    concurrently and on several devices of one process; every entry point
 *    makes the handle's device current for the duration of the call and
 *    restores the caller's current device afterwards (`stream` must belong to
 *    the handle's device).
 */
#ifndef SWIFTLY_HIP_H
#define SWIFTLY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct swiftly_hip swiftly_hip_t;

enum { SWIFTLY_C64 = 0, SWIFTLY_C128 = 1 };
enum {
    SWIFTLY_OK = 0,
    SWIFTLY_ERR_PARAM = 1,       /* -> ValueError in the Python mirror */
    SWIFTLY_ERR_UNSUPPORTED = 2, /* -> NotImplementedError */
    SWIFTLY_ERR_HIP = 3          /* -> RuntimeError */
};

const char* swiftly_hip_last_error(void);
int swiftly_hip_version(void);
/* Number of visible HIP devices (0 when there is no GPU; never fails). */
int swiftly_hip_device_count(void);
/* Identity of the build: the first 16 hex digits of the SHA-256 of the kernel sources (the headers and .hip files
 * of csrc, this header, the Makefile) the library was compiled from.  The per-kernel counter summaries under profiles/
 * record it and bench.py compares it with the running build. */
const char* swiftly_hip_build_id(void);

/*
 * Replaces Swiftly(N, yN_size, xM_size, W) (core.py:508-510) and the parameter
 * checks of core.py:55-74.  `pswf` is the length-yN host array
 * pro_ang1(0, 0, pi*W/2, 2*(k - yN/2)/yN) with pswf[0] = 0 (core.py:119-150);
 * the window constants Fb = 1/pswf[1:] and Fn = pswf[(yN/2)%(N/xM)::N/xM]
 * (core.py:104-117) are derived from it and uploaded in both precisions.
 */
int swiftly_hip_create(swiftly_hip_t** out, int64_t N, int64_t yN_size, int64_t xM_size, double W,
                       const double* pswf, int device);
void swiftly_hip_destroy(swiftly_hip_t* h);
int64_t swiftly_hip_contribution_size(const swiftly_hip_t* h); /* xM*yN/N, core.py:48 */
/* 1 when every transform length of the handle's configuration (yN_size, xM_size, contribution size) has a kernel in
 * `dtype` (SWIFTLY_C64 | SWIFTLY_C128), by the same gates the primitives apply: powers of two 8 .. 65536 in complex64 and
 * 8 .. 32768 in complex128; other lengths through Bluestein / Q * 2^k where their tables exist (complex128: convolution
 * and power-of-two sub-transform up to 8192).  0 otherwise (or for a null handle / unknown dtype).  Lets a caller pick
 * the precision before a pass instead of meeting SWIFTLY_ERR_UNSUPPORTED halfway through.  (complex64 at 65536 is
 * limited to the prepare_* / finish_* forms named by that error.) */
int swiftly_hip_supports_dtype(const swiftly_hip_t* h, int dtype);
/* Which pipelines exist for a configuration: the library's own capability table (csrc/swiftly_caps.h, the functions the
 * entry points refuse through), answered from the sizes alone -- no handle, no device.  1 = supported; 0 = not, and
 * swiftly_hip_last_error() says why (also for sizes swiftly_hip_create would reject).  `n_facets` <= 0: not given;
 * features that do not depend on `dtype` or `n_facets` ignore them. */
enum {
    SWIFTLY_FEATURE_FUSED_SUBGRID = 0,          /* transform_contributions + sum_finish_facets (dtype, n_facets) */
    SWIFTLY_FEATURE_BAND_PIPELINE = 1,          /* contiguous-axis-first forward kernels (dtype, n_facets) */
    SWIFTLY_FEATURE_BAND_PIPELINE_EXPLICIT = 2, /* ... when the caller asks for them: also answers for complex128 */
    SWIFTLY_FEATURE_BACKWARD_BAND = 3,          /* accumulate_facet_columns + finish_facet_band (dtype): complex64, yN_size a
                                                   power of two 64 .. 65536 or Q * 2^k; both entry points refuse other sizes through it */
    SWIFTLY_FEATURE_SPLIT_BAND = 4,             /* band buffers are parity-split and band-pruned (else whole axis, plain) */
    SWIFTLY_FEATURE_WINDOW_ROWS = 5,            /* prepare_facet_window_rows, size part (band / facets / windows: per call) */
    SWIFTLY_FEATURE_BACKWARD_BAND_EXPLICIT = 6, /* BACKWARD_BAND when the caller asks for the band schedule: complex64 as
                                                   BACKWARD_BAND; also answers for complex128 (xM, m powers of two, yN_size a
                                                   power of two 64 .. 32768, no Q * 2^k).  The gate accumulate_facet_columns
                                                   and finish_facet_band refuse through */
    SWIFTLY_FEATURE_SPLIT_PREPARE = 7,          /* split_prepare_facets + wave_split_subgrids (dtype, n_facets): complex64 as
                                                   FUSED_SUBGRID; complex128 for (m, xM) = (128, 256), (128, 1024), (256, 512),
                                                   (256, 1024), (512, 1024), up to 64 facets */
    SWIFTLY_FEATURE_REAL_FACETS = 8,            /* prepare_facet_band_real / prepare_facet_band_rows_real (dtype = the OUTPUT
                                                   type): the sizes of BAND_PIPELINE in complex64 with a power-of-two yN_size;
                                                   no complex128, no Q * 2^k.  The gate both entry points refuse through */
    SWIFTLY_FEATURE_REAL_FACETS_OUT = 9,        /* finish_facet_band_real (dtype = the INPUT type): the sizes of BACKWARD_BAND
                                                   in complex64 with a power-of-two yN_size; no complex128, no Q * 2^k.  The
                                                   gate the entry point refuses through */
    SWIFTLY_FEATURE_GROUP_FINISH = 10,          /* wave_group_finish_pieces (dtype, n_facets): FUSED_SUBGRID in complex64 with
                                                   (m, xM) = (128, 256) or (512, 1024) and n_facets * xM / m <= 64.  The gate
                                                   the entry point refuses through */
    SWIFTLY_FEATURE_REAL_WINDOW_ROWS = 11,      /* prepare_facet_window_rows_real (dtype = the OUTPUT type), size part: the
                                                   sizes of WINDOW_ROWS that are also sizes of REAL_FACETS in complex64.  The
                                                   gate the entry point refuses through ("real window rows: ...") */
    SWIFTLY_FEATURE_REAL_FACETS_RFFT = 12,      /* prepare_facet_band_rfft / prepare_facet_band_rows_rfft (dtype = the OUTPUT
                                                   type), size part: the sizes of REAL_FACETS with yN_size 32768.  The gate both
                                                   entry points refuse through ("real facets, half-length: ...") */
    SWIFTLY_FEATURE_REAL_FACETS_OUT_C2R = 13,   /* finish_facet_band_c2r (dtype = the INPUT type), size part: the sizes of
                                                   REAL_FACETS_OUT with yN_size 32768.  The gate the entry point refuses
                                                   through ("real facets out, half-length: ...") */
    SWIFTLY_FEATURE_REAL_FACETS_F64 = 14,       /* prepare_facet_band_real64 (dtype = the OUTPUT type): FLOAT64 facets into the
                                                   complex128 K1 -- the sizes of BAND_PIPELINE_EXPLICIT in complex128 (n_facets
                                                   not counted); complex64 is answered no (float32 facets: REAL_FACETS).  The
                                                   gate the entry point refuses through ("real facets, float64: ...") */
    SWIFTLY_FEATURE_REAL_FACETS_OUT_F64 = 15,   /* finish_facet_band_real64 (dtype = the INPUT type): FLOAT64 facets out of the
                                                   complex128 backward band -- the sizes of BACKWARD_BAND_EXPLICIT in
                                                   complex128; complex64 is answered no (float32 facets: REAL_FACETS_OUT).  The
                                                   gate the entry point refuses through ("real facet output, float64: ...") */
    SWIFTLY_FEATURE_REAL_FACETS_RFFT_64K = 16,  /* prepare_facet_band_rfft / prepare_facet_band_rows_rfft on 65536-point rows
                                                   (one 32768-point transform per row), size part: the sizes of REAL_FACETS with
                                                   yN_size 65536.  The entry points take a handle that REAL_FACETS_RFFT or this
                                                   feature supports ("real facets, half-length: ...") */
    SWIFTLY_FEATURE_REAL_FACETS_OUT_C2R_64K = 17, /* finish_facet_band_c2r on 65536-point band rows, size part: the sizes of
                                                   REAL_FACETS_OUT with yN_size 65536.  The entry point takes a handle that
                                                   REAL_FACETS_OUT_C2R or this feature supports ("real facets out, half-length: ...") */
    SWIFTLY_FEATURE_AXIS1_COLUMNS = 18          /* prepare_facet_columns_axis1 (dtype): complex64, the parity-split band layout,
                                                   (yN_size, m) = (32768, 512) or (16384, 256), a sum_finish instance for
                                                   (m, xM_size) and xM_size <= 2048.  The gate the entry point refuses through
                                                   ("axis-1 columns: ...") */
};
int swiftly_hip_supports(int feature, int dtype, int64_t N, int64_t yN_size, int64_t xM_size, int64_t n_facets);
enum {
    SWIFTLY_LIMIT_FUSED_FACETS = 0,              /* facets one sum_finish_facets call sums */
    SWIFTLY_LIMIT_WINDOW_ROWS_STAGE_COLUMNS = 1, /* physical band columns prepare_facet_window_rows can stage */
    SWIFTLY_LIMIT_WINDOW_ROWS_WINDOWS = 2        /* windows per prepare_facet_window_rows call */
};
int64_t swiftly_hip_limit(int which); /* -1 for an unknown limit */
/* 1 and (Q, k) when n = Q * 2^k with Q in {3, 5, 7, 9} and 2^k >= 8 (one radix-Q pass in front of the power-of-two
 * kernels), else 0 (powers of two included: they need no pass). */
int swiftly_hip_mixed_factor(int64_t n, int* Q, int* log2_rest);
/* Arithmetic of the column passes of the band pipelines on complex64 data (K2 = prepare_facet along the strided axis of
 * a wave, K3 = the m-point transform of add_to_subgrid behind it, and their backward mirrors): 32 (default) = float32
 * throughout; 64 = loads and stores in complex64, windows / butterflies / exchanges / four-step twiddles in float64.
 * These are the transforms whose rounding errors are amplified by BOTH facet windows (1/pswf, up to 90 per axis) before
 * anything cancels them; in float64 the end-to-end complex64 error against the numpy reference drops from 1.0e-5 to
 * 2.8e-6 forward and from 2.1e-5 to 5.1e-6 backward on the N = 65536 workload (storage floor 3.3e-6 on the probe
 * configuration of tests/accuracy_model.py), for 1.5x the pass time.  Initial value from the
 * environment variable SWIFTLY_COL_F64 (0 | 1).  (No reference counterpart: numpy computes in complex128 throughout,
 * core.py:212-222.) */
int swiftly_hip_set_column_precision(swiftly_hip_t* h, int bits);
int swiftly_hip_get_column_precision(const swiftly_hip_t* h);
/* Chained four-step launches (calling thread only; default 0).  A strided-axis transform whose intermediate exceeds
 * 256 MB runs in chunks on two internal streams of the handle; each call FORKS them behind everything queued on the
 * caller's stream and JOINS them back into it.  Between two such calls that follow each other on one stream the join /
 * fork pair is a full pipeline drain plus two cross-stream event hops (measured on the 64k workload: 40 us with nothing
 * running on the GPU, once per wave).  With chain = 1 the calling thread promises that the INPUTS of its next calls were
 * already complete when an earlier (forking) call on the same handle was queued, and that nobody else still uses the
 * output buffer: the fork is skipped, the chunk streams run on from the previous call's chunks, the join is unchanged
 * (the caller's stream still continues behind the whole transform).  SwiftlyForward's planned-wave prefetch (K2 of
 * consecutive waves read the same band buffers) sets it around the second and later calls of a pass.  (No reference
 * counterpart: scheduling of this implementation.) */
void swiftly_hip_chain_chunk_streams(int chain);

/* -- facet -> subgrid ------------------------------------------------------ */

/* Swiftly.prepare_facet(in[rows, facet_size], out[rows, yN], facet_off)
 * (core.py:686; numpy form core.py:212-222).  Overwrites out. */
int swiftly_hip_prepare_facet(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                              int64_t in_row_stride, int64_t in_col_stride, void* out, int64_t out_row_stride,
                              int64_t out_col_stride, int64_t facet_off, void* stream);

/* Swiftly.extract_from_facet(in[rows, yN], out[rows, m], subgrid_off)
 * (core.py:715; numpy form core.py:243-253).  Overwrites out.  Bit-exact. */
int swiftly_hip_extract_from_facet(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                   int64_t in_col_stride, void* out, int64_t out_row_stride, int64_t out_col_stride,
                                   int64_t subgrid_off, void* stream);

/* Swiftly.add_to_subgrid(in[rows, m], out[rows, xM], facet_off)
 * (core.py:744; numpy form core.py:274-285).  ACCUMULATES into out. */
int swiftly_hip_add_to_subgrid(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                               int64_t in_col_stride, void* out, int64_t out_row_stride, int64_t out_col_stride,
                               int64_t facet_off, void* stream);

/* Swiftly.add_to_subgrid_2d(in[m, m], out[xM, xM], facet_off0, facet_off1) (core.py:752-778): both axes in one call;
 * ACCUMULATES into out.  (Axis 0 into a stream-ordered [xM, m] intermediate, then axis 1 into out.) */
int swiftly_hip_add_to_subgrid_2d(swiftly_hip_t* h, int dtype, const void* in, int64_t in_row_stride,
                                  int64_t in_col_stride, void* out, int64_t out_row_stride, int64_t out_col_stride,
                                  int64_t facet_off0, int64_t facet_off1, void* stream);

/* Swiftly.finish_subgrid(in[rows, xM], out[rows, subgrid_size], subgrid_off)
 * (core.py:798-811; numpy form core.py:316-323), one axis per call.
 * `mask` (optional, device, real of matching precision, length subgrid_size)
 * folds the subgrid mask multiply of api_helper.py:107-112 into the store.
 * Overwrites out. */
int swiftly_hip_finish_subgrid(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                               int64_t in_col_stride, void* out, int64_t out_row_stride, int64_t out_col_stride,
                               int64_t subgrid_off, int64_t subgrid_size, const void* mask, void* stream);

/* -- subgrid -> facet ------------------------------------------------------ */

/* Swiftly.prepare_subgrid_inplace (core.py:837, 852; numpy form
 * core.py:357-366), one axis per call, out of place with the pad_mid of
 * core.py:836/849 folded in: in[rows, subgrid_size] -> out[rows, xM].
 * Overwrites out. */
int swiftly_hip_prepare_subgrid(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t subgrid_size,
                                int64_t in_row_stride, int64_t in_col_stride, void* out, int64_t out_row_stride,
                                int64_t out_col_stride, int64_t subgrid_off, void* stream);

/* Swiftly.prepare_subgrid_inplace(data[rows, xM], subgrid_off) (core.py:837-840): `data` already holds the subgrid
 * zero-padded to xM (pad_mid: centred); in place it becomes fft(roll(data, subgrid_off)) along the axis whose element
 * stride is col_stride.  ..._2d(data[xM, xM], off0, off1) (core.py:851-853) does both axes. */
int swiftly_hip_prepare_subgrid_inplace(swiftly_hip_t* h, int dtype, void* data, int64_t rows, int64_t row_stride,
                                        int64_t col_stride, int64_t subgrid_off, void* stream);
int swiftly_hip_prepare_subgrid_inplace_2d(swiftly_hip_t* h, int dtype, void* data, int64_t row_stride, int64_t col_stride,
                                           int64_t subgrid_off0, int64_t subgrid_off1, void* stream);

/* Swiftly.extract_from_subgrid(in[rows, xM], out[rows, m], facet_off)
 * (core.py:873; numpy form core.py:390-405).  Overwrites out. */
int swiftly_hip_extract_from_subgrid(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                     int64_t in_col_stride, void* out, int64_t out_row_stride,
                                     int64_t out_col_stride, int64_t facet_off, void* stream);

/* Swiftly.add_to_facet(in[rows, m], out[rows, yN], subgrid_off)
 * (core.py:897; numpy form core.py:430-446).  ACCUMULATES.  Exact adds. */
int swiftly_hip_add_to_facet(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                             int64_t in_col_stride, void* out, int64_t out_row_stride, int64_t out_col_stride,
                             int64_t subgrid_off, void* stream);

/* Swiftly.finish_facet(in[rows, yN], out[rows, facet_size], facet_off)
 * (core.py:923; numpy form core.py:475-483).  `mask` (optional) folds the
 * facet mask multiply of api_helper.py:175-176 / 195-196.  Overwrites out. */
int swiftly_hip_finish_facet(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                             int64_t in_col_stride, void* out, int64_t out_row_stride, int64_t out_col_stride,
                             int64_t facet_off, int64_t facet_size, const void* mask, void* stream);


/* -- fused / batched forms used by the streaming classes ---------------------
 *
 * *_batch: `nbatch` independent problems of identical shape; item b reads
 * in + b*in_batch_stride and writes out + b*out_batch_stride (strides in
 * complex elements; in_batch_stride = 0 shares one input; the ACCUMULATING
 * entry points add_to_subgrid_batch / add_to_facet_batch run the items
 * concurrently with plain read-modify-write, so items must not share output
 * elements: out_batch_stride = 0 with nbatch > 1 is SWIFTLY_ERR_PARAM).  `offs` is a HOST
 * array of nbatch per-item offsets, or NULL to use the scalar offset for all
 * items.  `mask` (finish_*): item b uses mask + b*mask_batch_stride (real
 * elements; 0 = one shared mask).  One launch covers up to 64 items. */

/* api_helper.extract_column (api_helper.py:200-210) as one kernel:
 * prepare_facet(extract_from_facet(BF_F, subgrid_off0, axis=0), facet_off1,
 * axis=1).  in = BF_F[yN, facet_size] (row stride in_row_stride), out =
 * NMBF_BF[m, yN].  The row gather is folded into the load. */
int swiftly_hip_extract_column(swiftly_hip_t* h, int dtype, const void* in, int64_t facet_size,
                               int64_t in_row_stride, int64_t in_col_stride, void* out, int64_t out_row_stride,
                               int64_t out_col_stride, int64_t subgrid_off0, int64_t facet_off1, void* stream);

/* Row-compacted BF_F (sparse subgrid sets): `rowmap` is a DEVICE int32 array of length yN; entry k is the
 * physical row of BF_F that holds logical row k, or negative when no requested subgrid column reads row k.
 * prepare_facet_rows = prepare_facet whose output index along the transform axis goes through the map
 * (unmapped rows are never written; rowmap may be NULL); extract_column_rows = extract_column reading such a
 * compacted BF_F.  fold_other_axis_window != 0 makes prepare_facet_rows also multiply row r of the call (= index r
 * along the OTHER axis, facet size `rows`) by 1/pswf -- the window the axis-1 prepare_facet of extract_column
 * applies; windows commute with transforms along the orthogonal axis, so extract_column_rows(prewindowed != 0)
 * then skips its window loads. */
int swiftly_hip_prepare_facet_rows(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                   int64_t in_row_stride, int64_t in_col_stride, void* out, int64_t out_row_stride,
                                   int64_t out_col_stride, int64_t facet_off, const int32_t* rowmap,
                                   int fold_other_axis_window, void* stream);
int swiftly_hip_extract_column_rows(swiftly_hip_t* h, int dtype, const void* in, int64_t facet_size,
                                    int64_t in_row_stride, int64_t in_col_stride, void* out, int64_t out_row_stride,
                                    int64_t out_col_stride, int64_t subgrid_off0, int64_t facet_off1,
                                    const int32_t* rowmap, int prewindowed, void* stream);

int swiftly_hip_extract_from_facet_batch(swiftly_hip_t* h, int dtype, const void* in, int64_t rows,
                                         int64_t in_row_stride, int64_t in_col_stride, void* out,
                                         int64_t out_row_stride, int64_t out_col_stride, int64_t subgrid_off,
                                         int64_t nbatch, int64_t in_batch_stride, int64_t out_batch_stride,
                                         const int64_t* subgrid_offs, void* stream);
int swiftly_hip_add_to_subgrid_batch(swiftly_hip_t* h, int dtype, const void* in, int64_t rows,
                                     int64_t in_row_stride, int64_t in_col_stride, void* out, int64_t out_row_stride,
                                     int64_t out_col_stride, int64_t facet_off, int64_t nbatch,
                                     int64_t in_batch_stride, int64_t out_batch_stride, const int64_t* facet_offs,
                                     void* stream);
int swiftly_hip_finish_subgrid_batch(swiftly_hip_t* h, int dtype, const void* in, int64_t rows,
                                     int64_t in_row_stride, int64_t in_col_stride, void* out, int64_t out_row_stride,
                                     int64_t out_col_stride, int64_t subgrid_off, int64_t subgrid_size,
                                     const void* mask, int64_t nbatch, int64_t in_batch_stride,
                                     int64_t out_batch_stride, const int64_t* subgrid_offs,
                                     int64_t mask_batch_stride, void* stream);
int swiftly_hip_prepare_subgrid_batch(swiftly_hip_t* h, int dtype, const void* in, int64_t rows,
                                      int64_t subgrid_size, int64_t in_row_stride, int64_t in_col_stride, void* out,
                                      int64_t out_row_stride, int64_t out_col_stride, int64_t subgrid_off,
                                      int64_t nbatch, int64_t in_batch_stride, int64_t out_batch_stride,
                                      const int64_t* subgrid_offs, void* stream);
int swiftly_hip_extract_from_subgrid_batch(swiftly_hip_t* h, int dtype, const void* in, int64_t rows,
                                           int64_t in_row_stride, int64_t in_col_stride, void* out,
                                           int64_t out_row_stride, int64_t out_col_stride, int64_t facet_off,
                                           int64_t nbatch, int64_t in_batch_stride, int64_t out_batch_stride,
                                           const int64_t* facet_offs, void* stream);
int swiftly_hip_add_to_facet_batch(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                   int64_t in_col_stride, void* out, int64_t out_row_stride, int64_t out_col_stride,
                                   int64_t subgrid_off, int64_t nbatch, int64_t in_batch_stride,
                                   int64_t out_batch_stride, const int64_t* subgrid_offs, void* stream);
int swiftly_hip_finish_facet_batch(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                   int64_t in_col_stride, void* out, int64_t out_row_stride, int64_t out_col_stride,
                                   int64_t facet_off, int64_t facet_size, const void* mask, int64_t nbatch,
                                   int64_t in_batch_stride, int64_t out_batch_stride, const int64_t* facet_offs,
                                   int64_t mask_batch_stride, void* stream);

/* Fused second half of api_helper.sum_and_finish_subgrid (api_helper.py:96-112) along the contiguous axis,
 * complex64: for every row of every subgrid b of a wave
 *     out[b][row, :] = mask_b * finish_subgrid_axis1( sum_g add_to_subgrid_axis1(in[g][b][row, :], group_facet_offs[g]) )
 * in[g][b] = [xM, m] (row stride in_row_stride), out[b] = [xM, subgrid_size].  Host arrays: group_facet_offs
 * (ngroups <= 8 facet off1 values), subgrid_offs (nbatch subgrid off1 values).  The [xM, xM] accumulator never
 * reaches HBM.  SWIFTLY_ERR_UNSUPPORTED for complex128 or (m, xM) pairs that are not instantiated. */
int swiftly_hip_sum_finish_rows(swiftly_hip_t* h, int dtype, const void* in, int64_t ngroups, int64_t in_group_stride,
                                int64_t in_batch_stride, int64_t in_row_stride, const int64_t* group_facet_offs,
                                void* out, int64_t out_batch_stride, int64_t out_row_stride,
                                const int64_t* subgrid_offs, int64_t subgrid_size, const void* mask,
                                int64_t mask_batch_stride, int64_t nbatch, void* stream);

/* K3 + K4a fused (complex64): for facet index f < nfacets and subgrid b < nsub
 *     out[f][b] (+)= add_to_subgrid_axis0( extract_from_facet_axis1(in[f], subgrid_off1s[b]), facet_off0 )
 * with in[f] = NMBF_BF [m, yN] at in + f*in_facet_stride (row stride in_row_stride) -- the output of
 * extract_column -- and out[f][b] = [xM, m] at out + (f*nsub + b)*out_batch_stride (element (r, c) at
 * r*out_col_stride + c).  The window gather of core.py:243-253 is folded into the load, so the [m, m]
 * contribution never goes through HBM (single-GPU path; the multi-GPU path materialises it for the
 * all-to-all).  All nfacets facets must share facet_off0.  ACCUMULATES. */
int swiftly_hip_add_to_subgrid_from_columns(swiftly_hip_t* h, int dtype, const void* in, int64_t in_row_stride,
                                            int64_t in_facet_stride, int64_t nfacets, void* out,
                                            int64_t out_col_stride, int64_t out_batch_stride, int64_t facet_off0,
                                            int64_t nsub, const int64_t* subgrid_off1s, void* stream);

/* -- contiguous-axis-first forward pipeline ----------------------------------------------------------------
 *
 * The 2-D transforms of the reference are separable, so the order in which api_helper.extract_column
 * (api_helper.py:200-210) visits the axes is free (it does axis 0 on the whole facet, then axis 1 per subgrid
 * column).  On a row-major facet the cheap order is the other one: the full-facet pass runs along the CONTIGUOUS
 * axis in ONE kernel (no four-step scratch), keeps only the output columns some planned subgrid reads, and the
 * strided-axis transform moves to the per-wave stage where it acts on m columns only.  complex64.
 *
 *   P_f   = prepare_facet_band(facet_f)                      once per facet       [yB, band]      K1
 *   Q_f   = prepare_facet_columns(P_f, wave off1)            per subgrid wave     [rows kept, m]  K2
 *   G_f,b = transform_contributions(Q_f, subgrid b)          per (facet, subgrid) [m, m]          K3+K4a
 *   T_b   = sum_finish_facets(G_.,b)                         per subgrid          [xM, xA]        K4b+K5a
 *   S_b   = finish_subgrid_batch(T_b, axis 0)                per subgrid          [xA, xA]        K5b
 */

/* Number of physical columns of a band buffer holding `band_len` logical columns (parity-split layout: the
 * logical column with cyclic distance d from band_start lives at (d & 1) * H + (d >> 1), H = swiftly_hip_band_columns / 2
 * = (band_len + 1) / 2 rounded up to a multiple of 16 columns, so that both parity runs start on a 128-byte line). */
int64_t swiftly_hip_band_columns(int64_t band_len);
/* The same for the band layout a HANDLE uses: parity-split as above for yN = 16384, 32768, 65536 (where the
 * two-workgroup long-row kernel produces the band); PLAIN for shorter padded facets (logical column d at physical
 * column d, band_columns = band_len; K1 is then the generic contiguous-axis transform and the band must be the
 * whole padded axis (0, yN)). */
int64_t swiftly_hip_band_columns_for(const swiftly_hip_t* h, int64_t band_len);

/* K1: Swiftly.prepare_facet(in[rows, facet_size], ., facet_off) (core.py:686; numpy form core.py:212-222) along
 * the contiguous axis for every row of a facet, keeping only the centred output indices in the cyclic range
 * [band_start, band_start + band_len) of [0, yN) (band_len = yN keeps everything), parity-split (see above);
 * out[rows, band_columns(band_len)], row stride out_row_stride.  fold_other_axis_window != 0 also multiplies row r
 * by 1/pswf of the OTHER axis (facet size `rows`) -- the window prepare_facet applies along that axis later;
 * windows commute with transforms along the orthogonal axis.  yN = 16384, 32768 or 65536 (SWIFTLY_ERR_UNSUPPORTED else). */
int swiftly_hip_prepare_facet_band(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                   int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                   int64_t band_start, int64_t band_len, int fold_other_axis_window, void* stream);
/* The same for a BLOCK OF ROWS [other_axis_row0, other_axis_row0 + rows) of a facet with other_axis_size rows (`in` points
 * at the first row of the block): the folded window of the other axis is that facet's 1/pswf at those rows, so that the
 * band rows of several blocks -- computed by different GPUs -- assemble to the band buffer of the whole facet
 * (distributed.py: cooperative facets when the facet count does not divide by the number of ranks).
 * other_axis_size = 0: no window of the other axis.  Split band layout only (yN_size 16384 .. 65536). */
int swiftly_hip_prepare_facet_band_rows(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                        int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                        int64_t band_start, int64_t band_len, int64_t other_axis_size,
                                        int64_t other_axis_row0, void* stream);
/* K1 of a REAL-VALUED facet (a Stokes image): the two entry points above with `in` pointing to FLOAT32, in_row_stride
 * counting real elements, and `dtype` the type of the OUTPUT (SWIFTLY_C64).  The row kernels load the reals (half the bytes
 * of the promoted facet) and set the imaginary parts to zero in registers; `out` holds the values the complex entry points
 * give for the same facet promoted to a contiguous complex64 copy (every operation on a zero imaginary part is exact), whatever
 * in_row_stride and the alignment of `in`: the transform is chosen as for that copy.  Sizes: SWIFTLY_FEATURE_REAL_FACETS
 * (complex64 band pipeline, power-of-two yN_size), SWIFTLY_ERR_UNSUPPORTED otherwise; every call the complex entry points
 * take at those sizes is taken.  At yN_size 32768 the 8-byte loads of the tuned instances need an even in_row_stride and an
 * 8-byte-aligned `in`; anything else fetches the same elements with 4-byte loads (same values, slower).
 * Exception to "the same values": at yN_size 32768 a facet_size above 23552 (the row can cover more than 24 of the 32 load
 * segments) runs all-segment instances that agree with the complex ones to the last bit or two, not bit for bit (the
 * compiler contracts their products differently); a caller that needs the bits of the complex path promotes such facets. */
int swiftly_hip_prepare_facet_band_real(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                        int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                        int64_t band_start, int64_t band_len, int fold_other_axis_window, void* stream);
int swiftly_hip_prepare_facet_band_rows_real(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                             int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                             int64_t band_start, int64_t band_len, int64_t other_axis_size,
                                             int64_t other_axis_row0, void* stream);
/* K1 of a real-valued FLOAT64 facet in complex128: the argument list of swiftly_hip_prepare_facet_band_real with `in`
 * pointing to FLOAT64, in_row_stride counting real elements, and `dtype` the type of the OUTPUT, which must be SWIFTLY_C128.
 * The complex128 row kernels (one workgroup per row up to 8192 points; pass A of the two-kernel long-row form at 16384 /
 * 32768) load the reals -- 8 bytes per pixel where the promoted facet holds 16 -- and set the imaginary parts to zero in
 * registers.  Value contract: `out` holds, bit for bit, what swiftly_hip_prepare_facet_band gives for the same facet promoted
 * to complex128 (the instances and their code after the load are the same, and every operation on a zero imaginary part is
 * exact), whatever in_row_stride; no instance is exempt.  The band must be (0, yN_size) as for every complex128 K1; there is
 * no _rows form (complex128 has no row blocks).  Sizes: SWIFTLY_FEATURE_REAL_FACETS_F64; a refusal is
 * SWIFTLY_ERR_UNSUPPORTED ("real facets, float64: ...") and nothing is written.  The _real, _rfft entry points above keep
 * refusing SWIFTLY_C128: this is a door of its own. */
int swiftly_hip_prepare_facet_band_real64(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                          int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                          int64_t band_start, int64_t band_len, int fold_other_axis_window, void* stream);
/* K1 of a real-valued facet as a HALF-LENGTH transform: the argument lists and the stored quantity of the two _real entry
 * points above (`in` float32, in_row_stride in reals, `dtype` the OUTPUT type; inverse-transform convention of prepare_facet,
 * 1 / yN_size, the folded window of the other axis; parity-split band), computed by ONE workgroup per row from one
 * yN_size / 2-point complex transform of z[n] = x[2n] + i x[2n+1] and the recombination
 * S[k] = E[k] + W^k O[k], S[k + yN_size/2] = E[k] - W^k O[k] (csrc/swiftly_rowreal.h).  The values ROUND DIFFERENTLY from
 * those of the _real entry points (same bound against the exact transform, not the same bits), which is why this is a door
 * of its own that nothing else routes to.  Sizes: SWIFTLY_FEATURE_REAL_FACETS_RFFT (REAL_FACETS with yN_size 32768) or
 * SWIFTLY_FEATURE_REAL_FACETS_RFFT_64K (REAL_FACETS with yN_size 65536: one 32768-point transform per row).  Per
 * call the adjacent reals are fetched with 8-byte loads, so an odd facet_size, an odd position of the facet in the padded
 * row (facet_off + yN_size/2 - facet_size/2 odd), an odd in_row_stride or an `in` that is not 8-byte aligned is REFUSED with
 * SWIFTLY_ERR_UNSUPPORTED ("real facets, half-length: ..."): nothing is written and no other kernel runs instead.  Parameter
 * errors as in the _real entry points.  swiftly_hip_last_band_instance does not count these calls. */
int swiftly_hip_prepare_facet_band_rfft(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                        int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                        int64_t band_start, int64_t band_len, int fold_other_axis_window, void* stream);
int swiftly_hip_prepare_facet_band_rows_rfft(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                             int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                             int64_t band_start, int64_t band_len, int64_t other_axis_size,
                                             int64_t other_axis_row0, void* stream);

/* K2: for every facet f < nfacets: extract_from_facet(P_f, subgrid_off1, axis=1) (core.py:715) folded into the load
 * of prepare_facet(., facet_off0s[f], axis=0) WITHOUT its window (pre-applied by prepare_facet_band).
 * in + f*in_facet_stride = band buffer P_f[rows, band], out + f*out_facet_stride = Q_f[., m] with row stride
 * out_row_stride; out_rowmap (device int32[yN], optional): physical output row of logical row k, negative = not
 * stored (the rows no subgrid of the plan reads).  facet_off0s is a HOST array. */
int swiftly_hip_prepare_facet_columns(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                      int64_t in_facet_stride, int64_t nfacets, const int64_t* facet_off0s,
                                      int64_t band_start, int64_t band_len, int64_t subgrid_off1, void* out,
                                      int64_t out_row_stride, int64_t out_facet_stride, const int32_t* out_rowmap,
                                      void* stream);

/* K2 for several waves at once (facet-major schedule: all waves of one facet right after its K1, on a second
 * stream, so that this bandwidth-bound work overlaps the issue-bound K1 of the next facet): item (f, w) is written at
 * out + f*out_facet_stride + w*out_wave_stride through the row map rowmaps + w*rowmap_stride (device int32[yN] each;
 * NULL = all rows).  workspace (optional, device, workspace_bytes >= 8*yN*m per (facet, wave) of a launch group):
 * the four-step scratch; with NULL it comes from the stream-ordered pool, whose reuse across streams is only
 * opportunistic.  wave_off1s / facet_off0s are HOST arrays. */
int swiftly_hip_prepare_facet_columns_waves(swiftly_hip_t* h, int dtype, const void* in, int64_t rows,
                                            int64_t in_row_stride, int64_t in_facet_stride, int64_t nfacets,
                                            const int64_t* facet_off0s, int64_t band_start, int64_t band_len,
                                            int64_t nwaves, const int64_t* wave_off1s, void* out, int64_t out_row_stride,
                                            int64_t out_facet_stride, int64_t out_wave_stride, const int32_t* rowmaps,
                                            int64_t rowmap_stride, void* workspace, int64_t workspace_bytes,
                                            void* stream);

/* K2 on a column range: prepare_facet_columns_waves for ONE wave, but only the positions [col_first, col_first + ncols)
 * of the m-wide window (both multiples of 16, 0 < ncols <= m): out keeps the [rows kept, m] layout and row stride, its
 * other columns are not touched.  SWIFTLY_ERR_PARAM when one of the requested columns lies outside the band
 * [band_start, band_start + band_len).  With subgrid_off1 = j*m*N/yN this fills (part of) column slab j of the padded
 * axis -- the columns (yN/2 - m/2 + j*m + [0, m)) mod yN at positions 0 .. m-1, the positions every wave's Q keeps them
 * at -- so that neighbouring waves, whose windows overlap, share it (transform_contributions_pieces).  Power-of-two
 * yN_size. */
int swiftly_hip_prepare_facet_columns_range(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                            int64_t in_facet_stride, int64_t nfacets, const int64_t* facet_off0s,
                                            int64_t band_start, int64_t band_len, int64_t subgrid_off1, int64_t col_first,
                                            int64_t ncols, void* out, int64_t out_row_stride, int64_t out_facet_stride,
                                            const int32_t* out_rowmap, void* workspace, int64_t workspace_bytes,
                                            void* stream);

/* K3 + K4a: out[f][b][k, j] = Fn[k] * cfft_m(C_{f,b}[:, j])[(k + s'0_f) mod m]  --  add_to_subgrid(axis 0)
 * (core.py:744, numpy form core.py:274-285) of the [m, m] contribution C_{f,b} WITHOUT its placement into the
 * padded subgrid (row k belongs to padded row (k + xM/2 - m/2 + s'0_f) mod xM; sum_finish_facets resolves that).
 * The contribution is gathered on load (extract_from_facet, core.py:243-253, never materialised):
 *   layout 0: in + f*in_facet_stride = NMBF_BF[m, yN or band] (output of extract_column[_rows]); window of
 *             subgrid_offs[b] (an off1) along the contiguous axis; band_len > 0: parity-split band columns.
 *   layout 1: in + f*in_facet_stride = Q_f[rows kept, m] (output of prepare_facet_columns); window of
 *             subgrid_offs[b] (an off0) along the strided axis through in_rowmap (device int32[yN] or NULL).
 *   layout 2: in + f*in_facet_stride + b*in_sub_stride = C_{f,b}[m, m] materialised (multi-GPU path).
 * out[f][b] at out + f*out_facet_stride + b*out_sub_stride, [m, m] row-major.  Overwrites.  Host offset arrays. */
int swiftly_hip_transform_contributions(swiftly_hip_t* h, int dtype, const void* in, int layout, int64_t in_row_stride,
                                        int64_t in_facet_stride, int64_t in_sub_stride, const int32_t* in_rowmap,
                                        int64_t band_start, int64_t band_len, int64_t nfacets,
                                        const int64_t* facet_off0s, int64_t nsub, const int64_t* subgrid_offs,
                                        void* out, int64_t out_facet_stride, int64_t out_sub_stride, void* stream);

/* transform_contributions, layout 1, for a wave whose window lies in up to two Q buffers (npieces <= 2; host arrays of
 * that length): piece i holds the window positions [first[i], first[i] + count[i]) (multiples of 16; together exactly
 * [0, m), disjoint) at the SAME positions of its rows: q[i] + f*q_facet_strides[i] = [n_rows[i] kept rows, m] with row map
 * rowmaps[i] (device int32[yN] or NULL; it may keep more rows than the subgrids read).  Column j of every output block
 * comes from the piece that holds position j; a piece with count 0 is skipped.  Output placement as wave_facet_side:
 * g_offsets / g_facet_strides (both or neither), else g_facet_stride / g_sub_stride.  Bit-identical to
 * transform_contributions on a Q assembled from the pieces.  Two non-empty pieces are read by ONE launch sequence over the
 * whole window (a single launch per batch of 32 facets x 64 subgrids), whose column tiles take each column from the piece
 * that holds it -- for complex64 with m = 128, 256 (float32 column arithmetic) and 512 (either column precision); any other
 * case, and every case after swiftly_hip_k3_one_launch(0), runs one launch sequence per piece, with the same bits. */
int swiftly_hip_transform_contributions_pieces(swiftly_hip_t* h, int dtype, int64_t npieces, const void* const* q,
                                               const int64_t* q_facet_strides, const int32_t* const* rowmaps,
                                               const int64_t* n_rows, const int64_t* first, const int64_t* count,
                                               int64_t nfacets, const int64_t* facet_off0s, int64_t nsub,
                                               const int64_t* sub_off0s, void* g_out, int64_t g_facet_stride,
                                               int64_t g_sub_stride, const int64_t* g_offsets,
                                               const int64_t* g_facet_strides, void* stream);
/* Process-wide switch of the one-launch form of transform_contributions_pieces (A/B runs and tests): sets it to on != 0
 * and returns the previous value; on < 0 only queries.  Initial value 1, or 0 with the environment variable
 * SWIFTLY_K3_ONE_LAUNCH=0.  (No reference counterpart: scheduling of this implementation.) */
int swiftly_hip_k3_one_launch(int on);

/* K4b + K5a: for every padded row r < xM of every subgrid b:
 *   out[b][r, :] = mask_b * finish_subgrid_axis1( sum_f add_to_subgrid_axis1( G[f][b][k_f(r), :], facet_off1s[f] ) )
 * over the facets whose axis-0 band covers r (k_f(r) = (r - (xM/2 - m/2 + s'0_f)) mod xM < m): the facet sums of
 * api_helper.sum_and_finish_subgrid (api_helper.py:81-99) re-associated so that no accumulator reaches HBM, plus
 * finish_subgrid along axis 1 and the mask (api_helper.py:101-111).  in = G from transform_contributions,
 * out[b] = [xM, subgrid_size].  Up to 64 facets. */
int swiftly_hip_sum_finish_facets(swiftly_hip_t* h, int dtype, const void* in, int64_t nfacets, int64_t in_facet_stride,
                                  int64_t in_sub_stride, int64_t in_row_stride, const int64_t* facet_off0s,
                                  const int64_t* facet_off1s, void* out, int64_t out_sub_stride, int64_t out_row_stride,
                                  const int64_t* subgrid_off1s, int64_t subgrid_size, const void* mask,
                                  int64_t mask_batch_stride, int64_t nsub, void* stream);

/* One forward wave as TWO native calls (per-wave host work = two ABI calls), for native callers.  The streaming classes
 * call K2 (prepare_facet_columns_waves / _range) and transform_contributions_pieces / wave_group_finish_pieces separately;
 * wave_facet_side is the same launch sequence as K2 followed by transform_contributions_pieces on one whole-window piece.
 *
 * wave_facet_side: K2 (prepare_facet_columns into the workspace q_work[nfacets][n_rows][m], facet stride
 *   q_facet_stride elements; skipped when compute_q == 0 and q_work still holds the wave's result -- e.g. a slice
 *   of what prepare_facet_columns_waves precomputed) followed by K3 + K4a (transform_contributions, layout 1)
 *   for the subgrids sub_off0s[nsub] of the wave.  Block (f, b) is written at
 *       g_out + g_offsets[b] + f * g_facet_strides[b]            when g_offsets != NULL
 *       g_out + f * g_facet_stride + b * g_sub_stride             otherwise
 *   (elements) -- the first form fills a rank-ordered all-to-all send buffer [dest][facet][subgrid of dest] in place.
 * wave_subgrid_side: K4b + K5a (sum_finish_facets into tmp_work[nsub][xM][subgrid_size]) and K5b
 *   (finish_subgrid along axis 0 with mask0) -> out[nsub][subgrid_size][subgrid_size] for the blocks g[f][b] of ALL
 *   facets (facet order = order of facet_off0s / facet_off1s, e.g. arrival order of the exchange).
 * Host arrays: facet / subgrid offsets, g_offsets, g_facet_strides.  masks: device, real, [nsub][subgrid_size] with
 * batch strides (0 = shared), or NULL.  scratch / scratch_bytes: optional device scratch for the four-step
 * intermediates (facet side: nfacets*yN*m*8 bytes, subgrid side: min(nsub, 64)*xM*subgrid_size*8 bytes); NULL or too
 * small = stream-ordered allocation, which costs ~2 ms of host time per call when the size changes between calls. */
int swiftly_hip_wave_facet_side(swiftly_hip_t* h, int dtype, const void* bands, int64_t rows, int64_t band_row_stride,
                                int64_t band_facet_stride, int64_t nfacets, const int64_t* facet_off0s,
                                int64_t band_start, int64_t band_len, int64_t wave_off1, const int32_t* rowmap,
                                int64_t n_rows, void* q_work, int64_t q_facet_stride, int compute_q, int64_t nsub,
                                const int64_t* sub_off0s, void* g_out, int64_t g_facet_stride, int64_t g_sub_stride,
                                const int64_t* g_offsets, const int64_t* g_facet_strides, void* scratch,
                                int64_t scratch_bytes, void* stream);
int swiftly_hip_wave_subgrid_side(swiftly_hip_t* h, int dtype, const void* g, int64_t nfacets, int64_t g_facet_stride,
                                  int64_t g_sub_stride, const int64_t* facet_off0s, const int64_t* facet_off1s,
                                  int64_t nsub, const int64_t* sub_off0s, const int64_t* sub_off1s, int64_t subgrid_size,
                                  const void* mask0, int64_t mask0_bs, const void* mask1, int64_t mask1_bs,
                                  void* tmp_work, void* out, void* scratch, int64_t scratch_bytes, void* stream);

/* The subgrid side of one forward wave with the STRIDED axis finished first, straight from the wave's K2 buffers (the
 * pieces of transform_contributions_pieces: same arguments, same checks), in two kernels instead of K3 + sum_finish_facets
 * + finish_subgrid(axis 0):
 *   stage 1 (group_finish): per facet off1 group g, subgrid b and column j of the m-wide window
 *       T[g][b][a, j] = mask0_b[a] * finish_subgrid_axis0( sum_{f in g} add_to_subgrid_axis0( C_f[:, j], facet_off0s[f] ) )[a]
 *     with C_f the window rows of facet f (extract_from_facet along axis 0 from Q), a < subgrid_size;
 *   stage 2 (sum_finish_facets over the rows of T): out[b][a, :] = mask1_b * finish_subgrid_axis1( sum_g
 *       add_to_subgrid_axis1( T[g][b][a, :], off1 of group g ) ).
 * The facet sums of api_helper.sum_and_finish_subgrid (api_helper.py:81-99) re-associated once more: the same subgrids as
 * transform_contributions_pieces + wave_subgrid_side up to float32 rounding, not the same bits, for 48.6 instead of 78.8 MB
 * of HBM traffic per subgrid on the N = 65536 workload.  Groups are numbered by ascending facet off1; within a group the
 * facets are summed in list order.  t_work: device scratch T[ngroups][nsub][xM][m] complex elements (t_work_elems >=
 * ngroups * nsub * xM * m; only subgrid_size of every xM rows are touched).  stages: 1 | 2 | 3 (both; a test may run
 * either kernel alone on a T of its own).  out[nsub][subgrid_size][subgrid_size].  complex64,
 * swiftly_hip_supports(SWIFTLY_FEATURE_GROUP_FINISH). */
int swiftly_hip_wave_group_finish_pieces(swiftly_hip_t* h, int dtype, int64_t npieces, const void* const* q,
                                         const int64_t* q_facet_strides, const int32_t* const* rowmaps,
                                         const int64_t* n_rows, const int64_t* first, const int64_t* count,
                                         int64_t nfacets, const int64_t* facet_off0s, const int64_t* facet_off1s,
                                         int64_t nsub, const int64_t* sub_off0s, const int64_t* sub_off1s,
                                         int64_t subgrid_size, const void* mask0, int64_t mask0_bs, const void* mask1,
                                         int64_t mask1_bs, void* t_work, int64_t t_work_elems, void* out, int stages,
                                         void* stream);
/* Process-wide switch between that form and K3 + wave_subgrid_side for the callers that own both halves (A/B runs and
 * tests): sets it to on != 0 and returns the previous value; on < 0 only queries.  Initial value 1, or 0 with the
 * environment variable SWIFTLY_GROUP_FINISH=0.  (No reference counterpart: scheduling of this implementation.) */
int swiftly_hip_group_finish(int on);
/* How stage 1 (group_finish) walks its tiles -- 16 columns x one subgrid x one facet group each: n = 0 launches one workgroup
 * per tile; n = 1 launches persistent workgroups, min(tiles, compute units of the handle's device) of them, each walking
 * the tiles w, w + grid, ... and requesting the next tile's first facet ahead of the inverse transform of the one it
 * finishes; n > 1 caps that grid at n workgroups (tests: a small problem then makes every workgroup walk many tiles).  The
 * same bits in every form.  Sets the process-wide value and returns the previous one; n = -1 only queries it; n = -2
 * returns the grid of the calling thread's last group_finish launch: 0 for the one-workgroup-per-tile kernel, else the
 * persistent kernel's workgroup count (-1 before the first launch).  Initial value 1, or the environment variable
 * SWIFTLY_GROUP_FINISH_PERSISTENT, read once.  (No reference counterpart: scheduling of this implementation.) */
int swiftly_hip_group_finish_persistent(int n);

/* AXIS-1-FIRST forward pipeline (r6; opt-in: the accuracy mode that replaces float64 column passes).  The transforms of
 * the two axes commute (api_helper.py:81-99, 200-210), so the contiguous-axis half of add_to_subgrid (core.py:255-285:
 * m-point transform x Fn, the step that takes the axis-1 facet window out again) can run on the K1 output BEFORE the
 * strided-axis transforms K2 / K3, which then work on data that carries ONE facet window instead of two: their float32
 * rounding reaches the subgrid an order of magnitude weaker.
 *
 * finish_axis1_rows: for every facet f and row r of its K1 band buffer (bands + f*band_facet_stride, [rows, band columns],
 *   parity-split) and the wave `wave_off1` (s = wave_off1 * yN / N):
 *       x[(i + s) mod m] = P_f[r, (yN/2 - m/2 + i + s) mod yN]            extract_from_facet(axis 1), core.py:243-253
 *       Z[k] = Fn[k] * cfft_m(x)[(k + s'1_f) mod m]                        add_to_subgrid(axis 1) without its placement
 *   out + f*out_facet_stride = [rows, m] in the parity-split layout of a band that is exactly the wave's window
 *   (band_start' = (yN/2 - m/2 + s) mod yN, band_len' = m; logical column i holds Z[(i + s) mod m]): pass it to
 *   prepare_facet_columns / wave_facet_side as `bands` with that band, and the contributions come out with Z along their
 *   contiguous axis.  facet_off1s: host array.  yN_size 16384 .. 65536, m 128 .. 1024, complex64.
 * wave_subgrid_side_placed: wave_subgrid_side for blocks produced that way -- sum_finish_facets places and sums the rows
 *   without its m-point transforms (xM <= 2048). */
int swiftly_hip_finish_axis1_rows(swiftly_hip_t* h, int dtype, const void* bands, int64_t rows, int64_t band_row_stride,
                                  int64_t band_facet_stride, int64_t nfacets, const int64_t* facet_off1s,
                                  int64_t band_start, int64_t band_len, int64_t wave_off1, void* out,
                                  int64_t out_row_stride, int64_t out_facet_stride, void* stream);
int swiftly_hip_wave_subgrid_side_placed(swiftly_hip_t* h, int dtype, const void* g, int64_t nfacets, int64_t g_facet_stride,
                                         int64_t g_sub_stride, const int64_t* facet_off0s, const int64_t* facet_off1s,
                                         int64_t nsub, const int64_t* sub_off0s, const int64_t* sub_off1s,
                                         int64_t subgrid_size, const void* mask0, int64_t mask0_bs, const void* mask1,
                                         int64_t mask1_bs, void* tmp_work, void* out, void* scratch, int64_t scratch_bytes,
                                         void* stream);
/* AXIS-1-FIRST pipeline with the contiguous-axis finish INSIDE K2 (SwiftlyConfig(axis1_first="k2")): finish_axis1_rows for
 * the wave `wave_off1` and prepare_facet_columns on its output, in one call that never writes the finished rows.  The
 * strided-axis transform of K2 is a four-step yN = n1 * n2 with n1 = 16384 / m; a workgroup of its first pass holds the n1
 * band-buffer rows {y1*n2 + y2} across the whole m-column window in LDS, finishes every row that lies inside the facet
 * along the contiguous axis (gather in window order, m-point transform, Fn, rotation by the facet's s'1 -- the rows of the
 * zero padding are neither read nor transformed), THEN does the n1-point step of the strided axis over them; the second
 * pass is the n2-point column pass of prepare_facet_columns, with its row map.
 *   out + f*out_facet_stride = [rows kept, m], element for element in meaning what prepare_facet_columns returns for
 *   `bands` = the output of finish_axis1_rows(wave_off1) and the band (window start, m) -- the same values up to float32
 *   rounding, not the same bits (another split of the strided axis).  out_rowmap as prepare_facet_columns: rows with a
 *   negative entry are not written (null: all yN rows, out_row_stride >= m).
 * bands: K1 band buffers [rows, band columns] per facet, parity-split; the window of wave_off1 has to lie inside the band
 * (SWIFTLY_ERR_PARAM).  facet_off0s, facet_off1s: host arrays, 1 .. 64 facets.  workspace: 8 * yN * m bytes per facet of a
 * group of up to 32 facets, else the stream-ordered pool (as prepare_facet_columns_waves); everything runs on `stream`.
 * float32 arithmetic whatever swiftly_hip_set_column_precision says.  complex64 and the sizes of
 * swiftly_hip_supports(SWIFTLY_FEATURE_AXIS1_COLUMNS); SWIFTLY_ERR_UNSUPPORTED with its text otherwise, nothing written.
 * (No reference counterpart: api_helper.py:81-99 allows either order of the axes.) */
int swiftly_hip_prepare_facet_columns_axis1(swiftly_hip_t* h, int dtype, const void* bands, int64_t rows,
                                            int64_t band_row_stride, int64_t band_facet_stride, int64_t nfacets,
                                            const int64_t* facet_off0s, const int64_t* facet_off1s, int64_t band_start,
                                            int64_t band_len, int64_t wave_off1, void* out, int64_t out_row_stride,
                                            int64_t out_facet_stride, const int32_t* out_rowmap, void* workspace,
                                            int64_t workspace_bytes, void* stream);

/* AXIS-1-FIRST pipeline with the contiguous-axis finish FUSED INTO THE FORWARD K1 (r6): prepare_facet_band_rows as one
 * persistent workgroup per CU that owns whole rows -- both output parities -- stages the band of a row in LDS (it never
 * reaches memory) and stores for each of the `nwindows` contribution windows of the plan (window w = the m columns from
 * logical column band_start + window_starts[w], all inside the band) exactly what finish_axis1_rows produces for wave w:
 *     out[row*out_row_stride + w*out_window_stride ..] = parity-split window band of  Fn[k] cfft_m(window w)[(k + s'1) mod m]
 * (wave-major [nwindows][rows][m]: out_row_stride = m, out_window_stride = rows*m -- what the pipeline uses: K2 of wave w then
 * reads one contiguous block; or side by side in a row: out_row_stride >= nwindows*m, out_window_stride = m)
 * so the rows of window w go to prepare_facet_columns / wave_facet_side with the band (window start, m) and the
 * blocks to wave_subgrid_side_placed.  No band buffer, no row pass per wave.  window_starts: DEVICE int32 table.
 * yN_size 32768, m = 512, even facet size / offset / row stride, a band of at most 12800 physical columns (the LDS stage);
 * SWIFTLY_ERR_UNSUPPORTED otherwise: use prepare_facet_band + finish_axis1_rows.  complex64. */
int swiftly_hip_prepare_facet_window_rows(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                          int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                          int64_t band_start, int64_t band_len, int64_t other_axis_size,
                                          int64_t other_axis_row0, const int32_t* window_starts, int64_t nwindows,
                                          int64_t out_window_stride, void* stream);
/* prepare_facet_window_rows for REAL-VALUED facets kept as float32: `in` points to float32, in_row_stride counts reals and
 * `dtype` is the OUTPUT type (SWIFTLY_C64); every other argument as above.  The whole-row kernel loads a lane's two
 * adjacent reals with one 8-byte load (half the bytes read, half the resident facet) and computes with a zero imaginary
 * part, so `out` holds the values prepare_facet_window_rows gives for the facet promoted to complex64 (at most the sign
 * of a zero differs).  Sizes: SWIFTLY_FEATURE_REAL_WINDOW_ROWS; per call what prepare_facet_window_rows needs, with an
 * even real row stride and an 8-byte-aligned `in` (there is no 4-byte-load form: SWIFTLY_ERR_UNSUPPORTED, nothing is
 * written -- promote the facet, or use prepare_facet_band_real + finish_axis1_rows).  swiftly_hip_last_band_instance
 * reports family 1 (whole row), st 3 and real 1 for it. */
int swiftly_hip_prepare_facet_window_rows_real(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                               int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                               int64_t band_start, int64_t band_len, int64_t other_axis_size,
                                               int64_t other_axis_row0, const int32_t* window_starts, int64_t nwindows,
                                               int64_t out_window_stride, void* stream);
/* Backward subgrid side for all facets at once (mirror of sum_finish_facets): in[b] = [xM, subgrid_size] =
 * prepare_subgrid of subgrid b along axis 0 ONLY (core.py:328-368); out[f][b] = [m, m] contiguous = the contribution
 * of subgrid b to facet f, i.e. api_helper.prepare_and_split_subgrid (api_helper.py:115-139): prepare_subgrid along
 * axis 1 and both extract_from_subgrid (core.py:396-439).  The prepared [xM, xM] subgrid and the per-off0
 * intermediates never reach HBM.  (m, xM) pairs of sum_finish_facets; up to 64 facets.  SWIFTLY_C128: complex128 in / out
 * for the pairs of SWIFTLY_FEATURE_SPLIT_PREPARE, the gate this entry point and wave_split_subgrids refuse through. */
int swiftly_hip_split_prepare_facets(swiftly_hip_t* h, int dtype, const void* in, int64_t in_sub_stride,
                                     int64_t in_row_stride, int64_t subgrid_size, int64_t nsub,
                                     const int64_t* subgrid_off1s, int64_t nfacets, const int64_t* facet_off0s,
                                     const int64_t* facet_off1s, void* out, int64_t out_facet_stride,
                                     int64_t out_sub_stride, void* stream);

/* The subgrid side of one backward wave in ONE native call without stream-ordered allocations: prepare_subgrid along
 * axis 0 of subgrids[nsub][subgrid_size][subgrid_size] (contiguous) followed by split_prepare_facets.  work: device
 * scratch of work_elems >= 2 * nsub * xM * subgrid_size complex elements of `dtype`. */
int swiftly_hip_wave_split_subgrids(swiftly_hip_t* h, int dtype, const void* subgrids, int64_t subgrid_size, int64_t nsub,
                                    const int64_t* subgrid_off0s, const int64_t* subgrid_off1s, int64_t nfacets,
                                    const int64_t* facet_off0s, const int64_t* facet_off1s, void* work,
                                    int64_t work_elems, void* out, int64_t out_facet_stride, int64_t out_sub_stride,
                                    void* stream);

/* Backward pass with the contiguous-axis transform LAST (mirror of prepare_facet_band / prepare_facet_columns;
 * waves = subgrids sharing off1).  Replaces, for all facets of a wave, api_helper.accumulate_column +
 * accumulate_facet (api_helper.py:142-179) with the two axes swapped (they commute):
 *
 * accumulate_facet_columns: for every facet f
 *     bands[f][r, d] += mask0_f[r] * finish_facet_axis0( sum_b add_to_facet_axis0( C[f][b], sub_off0[b] ), facet_off0s[f] )[r, j]
 *   where column j < m of the wave lands at band column d = (col(j, subgrid_off1) - band_start) mod yN of the padded
 *   facet (add_to_facet along axis 1, core.py:441-478).  The sum over the wave's subgrids is taken while LOADING:
 *   row_sources (device int32 [2][yN]) names for every padded row up to two source rows (negative = none), each
 *   encoded  chunk << 20 | row : read at parts + chunk_offsets[chunk] + f * chunk_facet_strides[chunk] + row *
 *   part_row_stride (elements; row = b*m + k for contiguous [m, m] blocks).  Chunks (<= 16) are the pieces of a
 *   multi-GPU receive buffer; a single-process caller passes one chunk.  masks: device float [nfacets][facet_size]
 *   (SWIFTLY_C128: double) or NULL.  bands[f] = [facet_size rows][band_len] plain column order, read-modify-written (zero it first).
 *   touched: optional device bytes [band_len], zero before the first call: band columns whose byte is 0 have not
 *   been written yet and are stored plainly (bands need no zero fill, no read of the old value); the call then marks
 *   its columns.  band_zero_untouched clears the columns no call has written (bands[rows][band_len], rows = all
 *   facets' rows when the facets are contiguous) -- call it before finish_facet_band.  NULL: always read-modify-write.
 *   workspace: optional device scratch (nfacets*yN*m*8 bytes used when large enough; SWIFTLY_C128: 16 bytes per
 *   element), else stream-ordered allocation.  SWIFTLY_C128: parts, bands and the workspace hold complex128, the
 *   arithmetic is float64 whatever swiftly_hip_set_column_precision says; sizes of SWIFTLY_FEATURE_BACKWARD_BAND_EXPLICIT.
 * finish_facet_band: finish_facet (core.py:481-510) along the contiguous axis of a band accumulator row:
 *     out[r, :] = mask * Fb * crop( FFT_yN( band row r placed at columns band_start + d, zero elsewhere ) ). */
int swiftly_hip_accumulate_facet_columns(swiftly_hip_t* h, int dtype, const void* parts, int64_t part_row_stride,
                                         int64_t nchunks, const int64_t* chunk_offsets,
                                         const int64_t* chunk_facet_strides, const int32_t* row_sources,
                                         int64_t nfacets, const int64_t* facet_off0s, int64_t facet_size,
                                         const void* masks, int64_t subgrid_off1, void* bands, int64_t band_row_stride,
                                         int64_t band_facet_stride, int64_t band_start, int64_t band_len,
                                         unsigned char* touched, void* workspace, int64_t workspace_bytes,
                                         void* stream);
int swiftly_hip_band_zero_untouched(swiftly_hip_t* h, int dtype, void* bands, int64_t rows, int64_t band_row_stride,
                                    int64_t band_len, const unsigned char* touched, void* stream);
int swiftly_hip_finish_facet_band(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                  int64_t band_start, int64_t band_len, void* out, int64_t out_row_stride,
                                  int64_t facet_off, int64_t facet_size, const void* mask, void* stream);
/* finish_facet_band for a REAL-VALUED facet (an image): the entry point above with `out` pointing to FLOAT32, out_row_stride
 * counting real elements, and `dtype` the type of the INPUT band rows (SWIFTLY_C64).  The row kernels compute what the complex
 * entry point computes and store the real part only (4 bytes per pixel; the arithmetic that only feeds the imaginary part is
 * not done): `out` holds, bit for bit, the real parts of what swiftly_hip_finish_facet_band gives for the same band rows,
 * whatever out_row_stride and the alignment of `out` -- the transform is chosen from the arguments both entry points share,
 * never from the destination.  Any out_row_stride >= facet_size (odd ones included) and any 4-byte-aligned `out` are taken;
 * out_row_stride < facet_size (overlapping rows) is SWIFTLY_ERR_PARAM.
 * Sizes: SWIFTLY_FEATURE_REAL_FACETS_OUT (complex64 backward band, power-of-two yN_size), SWIFTLY_ERR_UNSUPPORTED otherwise;
 * the checks of the arguments are those of swiftly_hip_finish_facet_band. */
int swiftly_hip_finish_facet_band_real(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                       int64_t band_start, int64_t band_len, void* out, int64_t out_row_stride,
                                       int64_t facet_off, int64_t facet_size, const void* mask, void* stream);
/* finish_facet_band for a real-valued FLOAT64 facet in complex128: the argument list of swiftly_hip_finish_facet_band_real
 * with `in` a COMPLEX128 band accumulator (`dtype` = SWIFTLY_C128, the type of the input) over any band the complex128
 * swiftly_hip_finish_facet_band takes, `out` pointing to FLOAT64, and out_row_stride counting real elements.  The complex128
 * row kernels (one workgroup per row up to 8192 points; pass B of the long-row form at 16384 / 32768) store the real part
 * only: 8 bytes per pixel, and no complex128 facet exists at any time.  Value contract: `out` holds, bit for bit, the real
 * parts of what swiftly_hip_finish_facet_band stores for the same band rows, whatever out_row_stride; no instance is exempt.
 * out_row_stride < facet_size (overlapping rows) is SWIFTLY_ERR_PARAM.  Sizes: SWIFTLY_FEATURE_REAL_FACETS_OUT_F64; a
 * refusal is SWIFTLY_ERR_UNSUPPORTED ("real facet output, float64: ...") and nothing is written.  The _real and _c2r entry
 * points keep refusing SWIFTLY_C128: this is a door of its own. */
int swiftly_hip_finish_facet_band_real64(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                         int64_t band_start, int64_t band_len, void* out, int64_t out_row_stride,
                                         int64_t facet_off, int64_t facet_size, const void* mask, void* stream);
/* finish_facet_band_real as ONE HALF-LENGTH transform per row (csrc/swiftly_rowc2r.h): only the real part of the 32768-point
 * transform of a band row is wanted, and that is the transform of the row's Hermitian part -- one 16384-point complex
 * transform of a recombination of the band elements k, k + yN/2 and their mirrors, in one workgroup per row, where the entry
 * point above runs the whole complex transform in two workgroups per row and drops the imaginary half.  Same arguments, same
 * quantity, the same error bound against the exact transform -- NOT the same bits: the rounding differs.  A kernel and a door
 * of its own that nothing else routes to (not an instance of the band row kernel: swiftly_hip_last_band_instance does not
 * count it).  Sizes: SWIFTLY_FEATURE_REAL_FACETS_OUT_C2R (REAL_FACETS_OUT with yN_size 32768) or
 * SWIFTLY_FEATURE_REAL_FACETS_OUT_C2R_64K (yN_size 65536: one 32768-point transform per row).  Per call, an odd facet_size, a
 * facet at an odd position of the padded row (yN_size / 2 - facet_size / 2 + facet_off odd), an odd out_row_stride or an `out`
 * that is not 8-byte aligned is SWIFTLY_ERR_UNSUPPORTED ("real facets out, half-length: ...") and nothing is written -- a
 * refusal is not a copy through the entry point above; out_row_stride < facet_size is SWIFTLY_ERR_PARAM as there.  The
 * other checks of the arguments are those of swiftly_hip_finish_facet_band. */
int swiftly_hip_finish_facet_band_c2r(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                      int64_t band_start, int64_t band_len, void* out, int64_t out_row_stride,
                                      int64_t facet_off, int64_t facet_size, const void* mask, void* stream);

/* -- point-source truths and RMSE checks on the device (handle-free; work is enqueued on `stream` of the current device).
 *    The reference checks itself with point sources: it builds facets with make_facet, and compares every subgrid with
 *    the direct Fourier sum of the sources and every finished facet with the scattered sources
 *    (fourier_algorithm.py:218-315, api_helper.py:15-70).  These entry points evaluate those truths natively, in float64
 *    arithmetic whatever `dtype` (of out / approx: SWIFTLY_C64 is rounded once on store, widened exactly on load).
 *    sources: device table of n_sources records { double re, im; int32_t c0, c1; } (24 bytes): complex intensity and
 *    the integer image coordinates relative to the image centre, reduced into [-image_size/2, image_size/2), no two
 *    records on one pixel (the caller merges them).  image_size <= 2^31.  n_sources = 0 is allowed (zeros).
 *    The subgrid phases exp(2 pi i c u / N) are evaluated from (c * u) mod N taken in 64-bit integers: the double
 *    formula of the reference carries a phase error that grows with c * u / N.
 *    Errors: SWIFTLY_ERR_PARAM for non-positive sizes, image_size > 2^31, a null pointer where one is needed, an
 *    unknown dtype.
 *
 * subgrids_from_sources: make_subgrid_from_sources (fourier_algorithm.py:267-315) / make_subgrid (api_helper.py:15-24)
 *   for n_subgrids subgrids of one `size` in ONE launch:
 *     out[b][i0, i1] = mask0s[b][i0] * mask1s[b][i1] * image_size^-2 *
 *                      sum_s I_s exp(2 pi i (c0_s (off0s[b] - size/2 + i0) + c1_s (off1s[b] - size/2 + i1)) / image_size)
 *   off0s / off1s: HOST arrays [n_subgrids]; mask0s / mask1s: device double [n_subgrids][size] or NULL (ones);
 *   out[b] at out + b * out_sub_stride, rows out_row_stride apart (complex elements), columns contiguous.
 * check_subgrids_from_sources: check_subgrid (api_helper.py:58-70) without storing the truth:
 *     result[b] = { sum |truth_b - approx_b|^2, sum |truth_b|^2 }   (device double [n_subgrids][2]);
 *   RMSE = sqrt(result[b][0]) / size.  Summed in a fixed order: bit-reproducible from run to run.
 * facet_from_sources: make_facet_from_sources (fourier_algorithm.py:218-264) / make_facet (api_helper.py:27-36): out is
 *   zeroed, then I_s * mask0[p0] * mask1[p1] stored at pixel p = (c_s - (off - size/2)) mod image_size of every
 *   source with p0, p1 < size.  mask0 / mask1: device double [size] or NULL.
 * check_facet_from_sources: check_facet (api_helper.py:39-48): result = { sum |truth - approx|^2, sum |truth|^2 }
 *   (device double [2]), every pixel of the facet differenced on its own.  The sources of facet row r are
 *   row_sources[row_start[r] .. row_start[r + 1]) (device int32; indices into the table, ascending in their facet column;
 *   row_start has size + 1 entries), built by the caller for these offsets.
 * facet_from_sources_real / check_facet_from_sources_real: the same two for a real-valued image, which never becomes
 *   complex: the arguments of their twins, but out / approx hold reals -- float for SWIFTLY_C64, double for SWIFTLY_C128
 *   -- and the row stride counts reals.  The store writes Re(I_s) * mask0[p0] * mask1[p1] (the caller refuses a table
 *   with a non-zero imaginary part); the check takes the truth's imaginary part as zero and sums in the order of the
 *   complex check: for approx with zero imaginary parts both give the same bits. */
int swiftly_hip_subgrids_from_sources(int dtype, const void* sources, int64_t n_sources, int64_t image_size,
                                      int64_t size, const int64_t* off0s, const int64_t* off1s, int64_t n_subgrids,
                                      const double* mask0s, const double* mask1s, void* out, int64_t out_sub_stride,
                                      int64_t out_row_stride, void* stream);
int swiftly_hip_check_subgrids_from_sources(int dtype, const void* sources, int64_t n_sources, int64_t image_size,
                                            int64_t size, const int64_t* off0s, const int64_t* off1s,
                                            int64_t n_subgrids, const double* mask0s, const double* mask1s,
                                            const void* approx, int64_t approx_sub_stride, int64_t approx_row_stride,
                                            double* result, void* stream);
int swiftly_hip_facet_from_sources(int dtype, const void* sources, int64_t n_sources, int64_t image_size, int64_t size,
                                   int64_t off0, int64_t off1, const double* mask0, const double* mask1, void* out,
                                   int64_t out_row_stride, void* stream);
int swiftly_hip_check_facet_from_sources(int dtype, const void* sources, int64_t n_sources, int64_t image_size,
                                         int64_t size, int64_t off0, int64_t off1, const double* mask0,
                                         const double* mask1, const void* approx, int64_t approx_row_stride,
                                         const int32_t* row_start, const int32_t* row_sources, double* result,
                                         void* stream);
int swiftly_hip_facet_from_sources_real(int dtype, const void* sources, int64_t n_sources, int64_t image_size,
                                        int64_t size, int64_t off0, int64_t off1, const double* mask0,
                                        const double* mask1, void* out, int64_t out_row_stride, void* stream);
int swiftly_hip_check_facet_from_sources_real(int dtype, const void* sources, int64_t n_sources, int64_t image_size,
                                              int64_t size, int64_t off0, int64_t off1, const double* mask0,
                                              const double* mask1, const void* approx, int64_t approx_row_stride,
                                              const int32_t* row_start, const int32_t* row_sources, double* result,
                                              void* stream);

/* -- device memory helpers for callers that do not bring their own allocator
 *    (the Python mirror uses torch for device memory and never calls these) -- */
int swiftly_hip_malloc(void** ptr, size_t bytes);
int swiftly_hip_free(void* ptr);
int swiftly_hip_memset_async(void* ptr, int value, size_t bytes, void* stream);
int swiftly_hip_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int swiftly_hip_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int swiftly_hip_stream_synchronize(void* stream);

/* -- CU-partitioned streams: two kernels of different character (the full-facet row transform: latency / issue bound;
 *    the per-wave column passes: bandwidth bound) can share the chip on disjoint sets of compute units.
 *    stream_create_cu_mask: a HIP stream whose kernels only run on the CUs whose bit is set in cu_mask (nwords 32-bit
 *    words, bit i of word i/32 = CU i in the runtime's enumeration; hipExtStreamCreateWithCUMask).  cu_census: launches
 *    `nblocks` one-wave workgroups on `stream` and writes per block  xcc_id << 16 | se_id << 8 | cu_id  to the device
 *    array out[nblocks] -- how a mask maps to XCDs is not documented, so callers measure it. */
int swiftly_hip_stream_create_cu_mask(void** stream, const uint32_t* cu_mask, int nwords);
int swiftly_hip_stream_destroy(void* stream);
int swiftly_hip_cu_census(int32_t* out, int nblocks, void* stream);

/* -- the kernels launched with dynamic LDS: how many instances the library registered when it was loaded (their
 *    per-device attribute is set by swiftly_hip_create) and the largest LDS size in bytes among them.  No device needed. */
int swiftly_hip_kernel_table(int64_t* count, int64_t* max_lds_bytes);

/* -- which instance of the band row kernel (the contiguous-axis kernel of prepare_facet_band / finish_facet_band and of
 *    prepare_facet / finish_facet on 32768 and 65536 points) the calling thread's last launch ran.  Writes the first
 *    min(n, 18) of: status (0 launched, -1 / -2 refused), family (0 two workgroups per row, 1 whole row), geometry, WIN,
 *    ST, PAIR, NSEG, CJ, W4, REAL, REAL_ST (the template arguments), seg_rot, ld_win4, twc (window table / compact twiddles
 *    in use), and the key of the window table (c, segments, n, segment length; segments = 0: none).  The record is taken
 *    after the fallback of a full window-table cache.  Returns the number of band row launches the calling thread has made
 *    so far (refused ones included, calls without rows not).  No device needed: before the first launch 0 and the default
 *    record. */
int64_t swiftly_hip_last_band_instance(int32_t* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* SWIFTLY_HIP_H */
