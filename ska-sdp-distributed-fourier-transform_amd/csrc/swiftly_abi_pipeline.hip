// C ABI of libswiftly_hip.so, part 2: the fused and per-wave entry points the streaming classes use
// (include/swiftly_hip.h, sections "fused kernels", "contiguous-axis-first forward pipeline" and "backward pass with
// band accumulators").  Each one is a short launch sequence over the column-tile passes (swiftly_colpass.h) and the
// row-wise fused kernels (swiftly_sumfinish.h).
#include "swiftly_abi_internal.h"
#include "swiftly_groupfinish.h"
#include "swiftly_colaxis1.h"

// touched[d] = 1 for the band columns d of one wave's window (see accumulate_facet_columns)
__global__ void mark_columns_kernel(unsigned char* __restrict__ touched, int m, int rot, int base, int yN, int band_start,
                                    int band_len) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= m) return;
    int scol = base + ((col + rot) & (m - 1));  // m a power of two, yN any length: base < yN
    if (scol >= yN) scol -= yN;
    int d = scol - band_start;
    if (d < 0) d += yN;
    if (d < band_len) touched[d] = 1;
}
// zero the band columns no wave has written (rows x band_len, row stride `pitch`)
template <typename R>
__global__ void zero_untouched_kernel(cx<R>* __restrict__ band, const unsigned char* __restrict__ touched, long long rows,
                                      long long pitch, int band_len) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= band_len || touched[d]) return;
    for (long long r = blockIdx.y; r < rows; r += gridDim.y) band[r * pitch + d] = cx<R>{(R)0, (R)0};
}


extern "C" {

int swiftly_hip_sum_finish_rows(swiftly_hip_t* h, int dtype, const void* in, int64_t ngroups, int64_t in_group_stride,
                                int64_t in_batch_stride, int64_t in_row_stride, const int64_t* group_facet_offs,
                                void* out, int64_t out_batch_stride, int64_t out_row_stride,
                                const int64_t* subgrid_offs, int64_t subgrid_size, const void* mask,
                                int64_t mask_batch_stride, int64_t nbatch, void* stream) {
    if (!h || !in || !out || !group_facet_offs || !subgrid_offs) return fail(SWIFTLY_ERR_PARAM, "null argument");
    DeviceGuard device_guard_(h->device);
    CHECK_SUBGRID_SIZE();
    if (dtype != SWIFTLY_C64) return fail(SWIFTLY_ERR_UNSUPPORTED, "sum_finish_rows: complex64 only");
    if (ngroups <= 0 || ngroups > kSumFinishMaxGroups)
        return fail(SWIFTLY_ERR_UNSUPPORTED, "sum_finish_rows: 1..%d facet groups supported", kSumFinishMaxGroups);
    if (!sum_finish_supported(h->log_m, h->log_xM))
        return fail(SWIFTLY_ERR_UNSUPPORTED, "sum_finish_rows: (m, xM) = (%lld, %lld) not instantiated", (long long)h->m,
                    (long long)h->xM);
    if (nbatch <= 0) return 0;
    const int xM = (int)h->xM, xA = (int)subgrid_size;
    SumFinishArgs a;
    std::memset(&a, 0, sizeof a);
    a.in_gs = in_group_stride;
    a.in_bs = in_batch_stride;
    a.in_rs = in_row_stride;
    a.out_bs = out_batch_stride;
    a.out_rs = out_row_stride;
    a.nrows = xM;
    a.ngroups = (int)ngroups;
    a.xA = xA;
    for (int g = 0; g < ngroups; g++) a.sp[g] = (int)facet_shift(*h, group_facet_offs[g]);
    a.mask_bs = mask ? mask_batch_stride : 0;
    if (int rc = fill_sum_finish_tables(h, false, &a.fn, &a.tw_m, &a.tw_x, nullptr, nullptr)) return rc;
    for (int64_t b0 = 0; b0 < nbatch; b0 += kSumFinishMaxBatch) {
        const int nb = (int)std::min<int64_t>(kSumFinishMaxBatch, nbatch - b0);
        a.in = (const cx<float>*)in + b0 * in_batch_stride;
        a.out = (cx<float>*)out + b0 * out_batch_stride;
        a.mask = mask ? (const float*)mask + b0 * mask_batch_stride : nullptr;
        for (int b = 0; b < nb; b++) a.st_a[b] = subgrid_in_padded_subgrid(*h, xA, subgrid_offs[b0 + b]).a;
        if (int rc = launch_status(launch_sum_finish_rows(h->log_m, h->log_xM, a, nb, (hipStream_t)stream))) return rc;
    }
    return 0;
}

int swiftly_hip_add_to_subgrid_from_columns(swiftly_hip_t* h, int dtype, const void* in, int64_t in_row_stride,
                                            int64_t in_facet_stride, int64_t nfacets, void* out,
                                            int64_t out_col_stride, int64_t out_batch_stride, int64_t facet_off0,
                                            int64_t nsub, const int64_t* subgrid_off1s, void* stream) {
    if (!h || !in || !out || !subgrid_off1s) return fail(SWIFTLY_ERR_PARAM, "null argument");
    DeviceGuard device_guard_(h->device);
    if (dtype != SWIFTLY_C64) return fail(SWIFTLY_ERR_UNSUPPORTED, "add_to_subgrid_from_columns: complex64 only");
    const int m = (int)h->m, xM = (int)h->xM, yN = (int)h->yN;
    if (h->log_m < kColPassMinLog || h->log_m > kColPassMaxLog || h->log_yN < 0)
        return fail(SWIFTLY_ERR_UNSUPPORTED, "add_to_subgrid_from_columns: contribution size %d not supported", m);
    if (nfacets <= 0 || nsub <= 0) return 0;
    CHECK_OFFSETS_32(offsets_fit_32(m, in_row_stride, yN) && offsets_fit_32(xM, out_col_stride, m));
    ColPassArgs c = col_pass_args(whole(m), contribution_in_padded_subgrid(*h, facet_off0));
    c.ncols = m;
    c.full_logn = h->log_m;
    c.in_pitch = (unsigned)in_row_stride;
    c.out_pitch = (unsigned)out_col_stride;
    c.st_win = h->fn_f;
    c.scale = 1.f;
    c.accumulate = 1;
    c.tw = twiddles<float>(h, h->log_m);
    if (!c.tw) return fail(SWIFTLY_ERR_HIP, "internal: missing twiddle table");
    c.cg_mod = m;
    c.cg_full = yN;
    c.in_bs_hi = in_facet_stride;
    c.in_bs = 0;
    c.out_bs = out_batch_stride;
    // batch item z = f*nb + b  (f: facet / group index, b: subgrid of this chunk); item (f, b) reads facet f's
    // column buffer and adds into out + (f*nsub + b0 + b) * out_batch_stride
    if (nfacets > kColZF) return fail(SWIFTLY_ERR_UNSUPPORTED, "add_to_subgrid_from_columns: too many facets per call");
    for (int64_t b0 = 0; b0 < nsub; b0 += kColZB) {
        const int nb = (int)std::min<int64_t>(kColZB, nsub - b0);
        ColZ cz = plain_colz();
        cz.flags = kZColGather;
        cz.nb = nb;
        for (int b = 0; b < nb; b++) {
            const Window w = window_of(*h, subgrid_off1s[b0 + b]);
            cz.b_rot[b] = w.rot;
            cz.b_base[b] = w.base;
        }
        c.in = (const cx<float>*)in;
        c.in_bdiv = nb;
        c.out = (cx<float>*)out + b0 * out_batch_stride;
        c.out_bdiv = nb;
        c.out_bs_hi = nsub * out_batch_stride;
        if (int rc = launch_col_checked(h->log_m, 2, c, cz, 1, (int)nfacets * nb, (hipStream_t)stream)) return rc;
    }
    return 0;
}


int64_t swiftly_hip_band_columns(int64_t band_len) { return 2 * band_half_columns(band_len); }
int64_t swiftly_hip_band_columns_for(const swiftly_hip_t* h, int64_t band_len) {
    if (!h) return -1;
    return band_is_split(h) ? 2 * band_half_columns(band_len) : band_len;
}

} // extern "C" (helpers follow)
// K2 for yN = Q * 2^k (swiftly_mixed.h): per wave, the radix-Q pass over the window columns of every facet (the
// generic pass kernel with lanes along the columns: window gather through the modular row map, zero padding and facet
// offset through the load map, one batch item per facet) into a scratch [facet][j][y2][column], then the Q
// power-of-two sub-transforms along the strided axis with the column-tile passes, whose store side carries the row
// map of the wave with plain output index Q*k + j.  PLAIN band layout only (the parity-split layout belongs to the
// power-of-two long-row kernel).
static int prepare_facet_columns_mixed(swiftly_hip_t* h, const void* in, int64_t rows, int64_t in_row_stride,
                                       int64_t in_facet_stride, int64_t nfacets, const int64_t* facet_off0s,
                                       int64_t band_start, int64_t band_len, int64_t nwaves, const int64_t* wave_off1s,
                                       void* out, int64_t out_row_stride, int64_t out_facet_stride,
                                       int64_t out_wave_stride, const int32_t* rowmaps, int64_t rowmap_stride,
                                       void* stream, void* ws, size_t ws_bytes) {
    const int yN = (int)h->yN, m = (int)h->m;
    auto it = h->mixed.find(h->yN);
    if (it == h->mixed.end() || !it->second.tw_f)
        return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_columns: padded facet size %d is neither a power of two nor Q * 2^k (Q = 3, 5, 7, 9)", yN);
    if (band_is_split(h)) return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_columns: internal: split band layout");
    const int Q = it->second.Q, logM = it->second.logM;
    const long long M = 1ll << logM;
    CHECK_OFFSETS_32(offsets_fit_32(rows, in_row_stride) && offsets_fit_32(yN, out_row_stride) && offsets_fit_32(yN, m));
    hipStream_t st = (hipStream_t)stream;
    MixedArgs<float> X = mixed_args<float>(it->second, yN);
    X.s_row = 1; X.s_y = m; X.s_j = M * m; X.s_b = (long long)yN * m;
    const int per_f_cap = (int)std::min<int64_t>(kMaxBatch, kColZF);
    for (int64_t f0 = 0; f0 < nfacets; f0 += per_f_cap) {
        const int nf = (int)std::min<int64_t>(per_f_cap, nfacets - f0);
        const MixedWorkspace part(nf, yN, M, m);
        ScratchLease lease;
        if (int rc = lease.acquire(ws, ws_bytes, part.bytes(), st, "hipMallocAsync(&own, radix_bytes + sub_bytes, st)")) return rc;
        X.scratch = (cx<float>*)lease.p;
        int rc = 0;
        for (int64_t w = 0; w < nwaves && !rc; w++) {
            const Window win = window_of(*h, wave_off1s[w]);
            RowsArgs<float> a;
            std::memset(&a, 0, sizeof a);
            a.in = (const cx<float>*)in + f0 * in_facet_stride;
            a.in_rs = 1;                            // "rows" of the pass = the m window columns (contiguous)
            a.in_cs = (unsigned)in_row_stride;      // transform index = facet row
            a.in_bs = in_facet_stride;
            a.nrows = m;
            a.nbatch = nf;
            a.rowfast = 1;
            a.ld = axis_map<float>(whole(rows));  // window already applied by prepare_facet_band
            a.conj_ld = 1;
            a.scale = 1.f;
            a.rm_mod = m;
            a.rm_inner = win.rot;
            a.rm_outer = pmod(win.base - band_start, yN);  // plain band: physical column = logical - band_start
            a.rm_full = yN;
            a.full_n = yN;
            OffTab tab;
            tab.use = 1;
            for (int f = 0; f < nf; f++) tab.ld_a[f] = facet_in_padded_facet(*h, rows, facet_off0s[f0 + f]).a;
            rc = radix_launch_status(launch_mixed_pass(Q, a, tab, X, nf, st), Q);
            if (rc) break;
            for (int j = 0; j < Q && !rc; j++) {
                ColPassArgs c = col_pass_args(Map{}, whole(yN));  // (plain load from the pass's scratch: no load map)
                c.ncols = m;
                c.in = X.scratch + (long long)j * X.s_j;
                c.in_pitch = (unsigned)m;
                c.in_bs = X.s_b;
                c.out = (cx<float>*)out + f0 * out_facet_stride + w * out_wave_stride;
                c.out_pitch = (unsigned)out_row_stride;
                c.out_bs = out_facet_stride;
                c.scale = (float)(1.0 / yN);
                c.conj_ld = 0; c.conj_st = 1;
                c.f64 = h->col_f64;  // (the sub-transforms only: the radix-Q pass is float32; as accumulate_facet_columns)
                c.st_rowmap = rowmaps ? rowmaps + w * rowmap_stride : nullptr;
                c.st_rowmap_bs = 0;
                const int r2 = col_transform(h, logM, c, plain_colz(), m, nf, st, part.sub(lease.p), part.sub_bytes, Q, j, yN);
                if (r2 == -1) rc = fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_columns: sub-transform length %lld not supported", M);
                else rc = r2;
            }
        }
        if ((rc = lease.release(rc))) return rc;
    }
    return 0;
}

// K2 for `nfacets` facets x `nwaves` waves: item (f, w) gathers the window of wave_off1s[w] from band buffer f and
// writes out + f*out_facet_stride + w*out_wave_stride through row map  rowmaps + w*rowmap_stride  (or none).
static int prepare_facet_columns_impl(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                      int64_t in_facet_stride, int64_t nfacets, const int64_t* facet_off0s,
                                      int64_t band_start, int64_t band_len, int64_t nwaves, const int64_t* wave_off1s,
                                      void* out, int64_t out_row_stride, int64_t out_facet_stride,
                                      int64_t out_wave_stride, const int32_t* rowmaps, int64_t rowmap_stride,
                                      void* stream, void* ws = nullptr, size_t ws_bytes = 0, int64_t col_first = 0,
                                      int64_t ncols = -1) {
    if (!h || !in || !out || !facet_off0s || !wave_off1s) return fail(SWIFTLY_ERR_PARAM, "null argument");
    const bool ranged = ncols >= 0;  // positions [col_first, col_first + ncols) of the window only, checked against the band
    if (!ranged) ncols = h->m;       // (the whole window, as ever)
    const bool c128 = dtype == SWIFTLY_C128;
    CHECK_DTYPE();
    if (c128 && !band_pipeline_c128_supported(h))
        return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_columns: complex128 needs a power-of-two yN_size of 64 .. 32768 and "
                    "(m, xM) with a complex128 sum_finish_facets instance, got yN_size %lld, m %lld, xM %lld",
                    (long long)h->yN, (long long)h->m, (long long)h->xM);
    const int yN = (int)h->yN, m = (int)h->m;
    if (h->log_m < kBandMinLog) return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_columns: sizes not supported");
    // (the yN range of swiftly_hip_supports(BAND_PIPELINE): refuse here, not at a missing twiddle table further down)
    if (!c128 && !band_yN_supported(*h, kBandMinLog, kBandMaxLogYN))
        return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_columns: padded facet size %d not supported (power of two %d .. %d, or "
                    "Q * 2^k with Q = 3, 5, 7, 9)", yN, 1 << kBandMinLog, 1 << kBandMaxLogYN);
    if (rows <= 0 || rows >= yN) return fail(SWIFTLY_ERR_PARAM, "facet size %lld must be in [1, yN_size - 1]", (long long)rows);
    CHECK_BAND();
    if (nfacets <= 0 || nwaves <= 0) return 0;
    if (ranged) {
        if (col_first < 0 || ncols <= 0 || col_first + ncols > m || col_first % 16 || ncols % 16)
            return fail(SWIFTLY_ERR_PARAM, "prepare_facet_columns: column range [%lld, +%lld) must be multiples of 16 inside [0, %d)",
                        (long long)col_first, (long long)ncols, m);
        if (h->log_yN < 0) return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_columns: a column range needs a power-of-two yN_size");
        // every requested column has to come from the band (the whole-window form maps a stray column to band column 0)
        for (int64_t w = 0; w < nwaves; w++)
            if (const int64_t q = window_in_band(*h, window_of(*h, wave_off1s[w]), col_first, ncols, band_start, band_len); q >= 0)
                return fail(SWIFTLY_ERR_PARAM, "prepare_facet_columns: position %lld of the window of off1 = %lld is outside the "
                            "band [%lld, +%lld)", (long long)q, (long long)wave_off1s[w], (long long)band_start, (long long)band_len);
    }
    if (h->log_yN < 0)
        return prepare_facet_columns_mixed(h, in, rows, in_row_stride, in_facet_stride, nfacets, facet_off0s, band_start,
                                           band_len, nwaves, wave_off1s, out, out_row_stride, out_facet_stride,
                                           out_wave_stride, rowmaps, rowmap_stride, stream, ws, ws_bytes);
    // only `rows` input rows are ever read (the rest of the padded axis is zero fill)
    CHECK_OFFSETS_32(offsets_fit_32(rows, in_row_stride) && offsets_fit_32(yN, out_row_stride));
    ColPassArgs c = col_pass_args(whole(rows), whole(yN));  // (load: window already applied by prepare_facet_band)
    c.ncols = (int)ncols;
    c.col0 = (int)col_first;  // the gather sees window position col_first + column; the output pointer is shifted below
    c.full_logn = h->log_yN;
    c.in_pitch = (unsigned)in_row_stride;
    c.out_pitch = (unsigned)out_row_stride;
    c.scale = (float)(1.0 / yN);
    c.conj_ld = c.conj_st = 1;
    c.cg_mod = m; c.cg_full = yN;
    // (complex128: plain band layout -- its K1 keeps the whole padded axis in plain column order)
    c.cg_band_start = (int)band_start; c.cg_band_len = (int)band_len; c.cg_band_half = c128 ? 0 : band_half_of(h, band_len);
    c.f64 = h->col_f64;  // (col_transform falls back to float32 where the instances do not exist)
    c.c128 = c128 ? 1 : 0;
    const int esz = c128 ? 16 : 8;
    const int per_f = kColZF;  // facets per launch group (smaller groups: no gain, r4)
    // keep the four-step scratch of one launch group below ~4 GB
    const int64_t group_cap = ws ? (int64_t)ws_bytes : (int64_t(4) << 30);
    const int64_t per_w_cap = std::max<int64_t>(1, group_cap / ((int64_t)yN * ncols * esz) / std::min<int64_t>(per_f, nfacets));
    const int per_w = (int)std::min<int64_t>(kColZB, per_w_cap);
    for (int64_t f0 = 0; f0 < nfacets; f0 += per_f) {
        const int nf = (int)std::min<int64_t>(per_f, nfacets - f0);
        for (int64_t w0 = 0; w0 < nwaves; w0 += per_w) {
            const int nw = (int)std::min<int64_t>(per_w, nwaves - w0);
            ColZ cz = plain_colz();
            cz.flags = kZColGather | kZLoadAF;
            cz.nb = nw;
            for (int w = 0; w < nw; w++) {
                const Window win = window_of(*h, wave_off1s[w0 + w]);
                cz.b_rot[w] = win.rot;
                cz.b_base[w] = win.base;
            }
            for (int f = 0; f < nf; f++) cz.f_lda[f] = facet_in_padded_facet(*h, rows, facet_off0s[f0 + f]).a;
            // item z = f*nw + w reads band buffer f, writes out[f][w]
            c.in = cx_at(in, f0 * in_facet_stride, c128);
            c.in_bdiv = nw; c.in_bs_hi = in_facet_stride; c.in_bs = 0;
            c.out = cx_at(out, f0 * out_facet_stride + w0 * out_wave_stride + col_first, c128);
            c.out_bdiv = nw; c.out_bs_hi = out_facet_stride; c.out_bs = out_wave_stride;
            c.st_rowmap = rowmaps ? rowmaps + w0 * rowmap_stride : nullptr;
            c.st_rowmap_bs = rowmaps ? rowmap_stride : 0;
            const int rc = col_transform(h, h->log_yN, c, cz, (int)ncols, nf * nw, (hipStream_t)stream, ws, ws_bytes);
            if (rc == -1) return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_columns: padded facet size %d not supported", yN);
            if (rc) return rc;
        }
    }
    return 0;
}

extern "C" {

int swiftly_hip_prepare_facet_columns(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                      int64_t in_facet_stride, int64_t nfacets, const int64_t* facet_off0s,
                                      int64_t band_start, int64_t band_len, int64_t subgrid_off1, void* out,
                                      int64_t out_row_stride, int64_t out_facet_stride, const int32_t* out_rowmap,
                                      void* stream) {
    if (!h) return fail(SWIFTLY_ERR_PARAM, "null argument");
    DeviceGuard device_guard_(h->device);
    return prepare_facet_columns_impl(h, dtype, in, rows, in_row_stride, in_facet_stride, nfacets, facet_off0s, band_start,
                                      band_len, 1, &subgrid_off1, out, out_row_stride, out_facet_stride, 0, out_rowmap, 0,
                                      stream);
}

int swiftly_hip_prepare_facet_columns_waves(swiftly_hip_t* h, int dtype, const void* in, int64_t rows,
                                            int64_t in_row_stride, int64_t in_facet_stride, int64_t nfacets,
                                            const int64_t* facet_off0s, int64_t band_start, int64_t band_len,
                                            int64_t nwaves, const int64_t* wave_off1s, void* out, int64_t out_row_stride,
                                            int64_t out_facet_stride, int64_t out_wave_stride, const int32_t* rowmaps,
                                            int64_t rowmap_stride, void* workspace, int64_t workspace_bytes,
                                            void* stream) {
    if (!h) return fail(SWIFTLY_ERR_PARAM, "null argument");
    DeviceGuard device_guard_(h->device);
    return prepare_facet_columns_impl(h, dtype, in, rows, in_row_stride, in_facet_stride, nfacets, facet_off0s, band_start,
                                      band_len, nwaves, wave_off1s, out, out_row_stride, out_facet_stride, out_wave_stride,
                                      rowmaps, rowmap_stride, stream, workspace, workspace ? (size_t)workspace_bytes : 0);
}

/* K2 on a column range: swiftly_hip_prepare_facet_columns_waves for one wave, positions [col_first, col_first + ncols) of
 * the m-wide window only (multiples of 16; the other columns of `out` are not touched).  Refused when a requested column
 * lies outside the band. */
int swiftly_hip_prepare_facet_columns_range(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                            int64_t in_facet_stride, int64_t nfacets, const int64_t* facet_off0s,
                                            int64_t band_start, int64_t band_len, int64_t subgrid_off1, int64_t col_first,
                                            int64_t ncols, void* out, int64_t out_row_stride, int64_t out_facet_stride,
                                            const int32_t* out_rowmap, void* workspace, int64_t workspace_bytes,
                                            void* stream) {
    if (!h) return fail(SWIFTLY_ERR_PARAM, "null argument");
    DeviceGuard device_guard_(h->device);
    if (ncols <= 0) return fail(SWIFTLY_ERR_PARAM, "prepare_facet_columns: empty column range");
    return prepare_facet_columns_impl(h, dtype, in, rows, in_row_stride, in_facet_stride, nfacets, facet_off0s, band_start,
                                      band_len, 1, &subgrid_off1, out, out_row_stride, out_facet_stride, 0, out_rowmap, 0,
                                      stream, workspace, workspace ? (size_t)workspace_bytes : 0, col_first, ncols);
}

} // extern "C" (helper follows)
// out_offs / out_fstrides (optional, per subgrid): item (f, b) is written at out + out_offs[b] + f*out_fstrides[b]
// instead of out + f*out_facet_stride + b*out_sub_stride
// in_b (optional, layout 1 on the whole window): a second source [rows kept, m] per facet with its own facet stride and row
// map, which holds the window positions below `split` (a multiple of 16); `in` holds the others.  One launch per batch reads
// both (ColPassSrc2); SWIFTLY_ERR_UNSUPPORTED before anything is launched when the case has no such instance.
struct SecondSource {
    const void* in;
    int64_t facet_stride;
    const int32_t* rowmap;
    int64_t split;
};
static int transform_contributions_impl(swiftly_hip_t* h, int dtype, const void* in, int layout, int64_t in_row_stride,
                                        int64_t in_facet_stride, int64_t in_sub_stride, const int32_t* in_rowmap,
                                        int64_t band_start, int64_t band_len, int64_t nfacets,
                                        const int64_t* facet_off0s, int64_t nsub, const int64_t* subgrid_offs,
                                        void* out, int64_t out_facet_stride, int64_t out_sub_stride,
                                        const int64_t* out_offs, const int64_t* out_fstrides, void* stream,
                                        int64_t col_first = 0, int64_t ncols = -1, const SecondSource* in_b = nullptr) {
    if (!h || !in || !out || !facet_off0s) return fail(SWIFTLY_ERR_PARAM, "null argument");
    // columns [col_first, col_first + ncols) of the blocks only (layout 1, whose columns are read where they are written):
    // both pointers are shifted, the other columns of `out` are not touched
    if (ncols < 0) ncols = h->m;
    if (col_first < 0 || ncols <= 0 || col_first + ncols > h->m || ((col_first || ncols != h->m) && layout != 1))
        return fail(SWIFTLY_ERR_PARAM, "transform_contributions: bad column range [%lld, +%lld)", (long long)col_first, (long long)ncols);
    if (in_b && (layout != 1 || col_first || ncols != h->m || !in_b->in || in_b->split <= 0 || in_b->split >= h->m || in_b->split % 16))
        return fail(SWIFTLY_ERR_PARAM, "transform_contributions: bad second source (split %lld)", (long long)(in_b ? in_b->split : 0));
    const bool c128 = dtype == SWIFTLY_C128;
    CHECK_DTYPE();
    if (layout < 0 || layout > 2) return fail(SWIFTLY_ERR_PARAM, "bad layout %d", layout);
    // complex128: the row-window layouts of the band pipeline (layout 0 gathers from the complex64-only column buffers)
    if (c128 && (layout == 0 || !band_pipeline_c128_supported(h)))
        return fail(SWIFTLY_ERR_UNSUPPORTED, "transform_contributions: complex128 takes layouts 1 and 2 and m = 32 .. 512 with a "
                    "complex128 sum_finish_facets instance, got layout %d, m %lld, xM %lld", layout, (long long)h->m,
                    (long long)h->xM);
    if (layout != 2 && !subgrid_offs) return fail(SWIFTLY_ERR_PARAM, "null argument");
    const int m = (int)h->m, yN = (int)h->yN;
    // (layout 0 gathers columns with masks of the padded facet size; the row-window layouts take any yN)
    if (h->log_m < kColPassMinLog || h->log_m > kColPassMaxLog || (layout == 0 && h->log_yN < 0))
        return fail(SWIFTLY_ERR_UNSUPPORTED, "transform_contributions: contribution size %d not supported", m);
    if (nfacets <= 0 || nsub <= 0) return 0;
    CHECK_OFFSETS_32(offsets_fit_32(yN, in_row_stride, yN));
    ColPassArgs c = col_pass_args(whole(m), whole(m));  // no placement: out[k] = Fn[k] * F[(k + s') mod m]
    c.ncols = (int)ncols;
    c.full_logn = h->log_m;
    c.in_pitch = (unsigned)in_row_stride;
    c.out_pitch = (unsigned)m;
    c.st_win = c128 ? (const float*)h->fn_d : h->fn_f;  // (complex128: the double table)
    c.scale = 1.f;
    c.tw = twiddles<float>(h, h->log_m);
    if (!c.tw) return fail(SWIFTLY_ERR_HIP, "internal: missing twiddle table");
    if (layout == 0) {  // in[f] = [m, yN] column buffers: window gather along the contiguous axis
        c.cg_mod = m; c.cg_full = yN;
        c.cg_band_start = (int)band_start; c.cg_band_len = (int)band_len; c.cg_band_half = band_half_of(h, band_len);
    } else if (layout == 1) {  // in[f] = [kept rows of yN, m]: window gather along the strided axis
        c.ld_mod = yN;
        c.ld_rowmap = in_rowmap;
        c.tile32 = 1;  // K3 of the band pipeline: runs next to K2 of the following waves (col_pass.hip)
    }
    for (int64_t f0 = 0; f0 < nfacets; f0 += kColZF) {
        const int nf = (int)std::min<int64_t>(kColZF, nfacets - f0);
        for (int64_t b0 = 0; b0 < nsub; b0 += kColZB) {
            const int nb = (int)std::min<int64_t>(kColZB, nsub - b0);
            ColZ cz = plain_colz();
            cz.nb = nb;
            cz.flags = kZStoreAF;
            for (int f = 0; f < nf; f++) cz.f_sta[f] = contribution_in_padded_subgrid(*h, facet_off0s[f0 + f]).a;
            for (int b = 0; b < nb && layout != 2; b++) {
                const Window w = window_of(*h, subgrid_offs[b0 + b]);
                if (layout == 0) {
                    cz.b_rot[b] = w.rot;
                    cz.b_base[b] = w.base;
                } else {
                    cz.b_lda[b] = w.rot;
                    cz.b_ldc[b] = w.base;
                }
            }
            if (layout == 0) cz.flags |= kZColGather;
            if (layout == 1) cz.flags |= kZLoadB;
            // item z = f*nb + b reads in + f*in_facet_stride (+ b*in_sub_stride for layout 2), writes out[f][b]
            c.in = cx_at(in, f0 * in_facet_stride + (layout == 2 ? b0 * in_sub_stride : 0) + col_first, c128);
            c.in_bdiv = nb; c.in_bs_hi = in_facet_stride; c.in_bs = layout == 2 ? in_sub_stride : 0;
            c.out = cx_at(out, f0 * out_facet_stride + b0 * out_sub_stride + col_first, c128);
            c.out_bdiv = nb; c.out_bs_hi = out_facet_stride; c.out_bs = out_sub_stride;
            if (out_offs) {
                cz.flags |= kZOutB;
                c.out = cx_at(out, col_first, c128);
                for (int b = 0; b < nb; b++) {
                    cz.b_out_fs[b] = out_fstrides[b0 + b];
                    cz.b_out_off[b] = out_offs[b0 + b] + f0 * out_fstrides[b0 + b];
                }
            }
            if (int rc = set_col_precision(h, c, h->log_m, c128)) return rc;
            ColPassSrc2 src2 = {};
            if (in_b) {
                if (!col_pass_pieces_supported(h->log_m, c))
                    return fail(SWIFTLY_ERR_UNSUPPORTED, "transform_contributions: no two-source instance for m = %d", m);
                src2.in = cx_at(in_b->in, f0 * in_b->facet_stride, c128);
                src2.in_bs_hi = in_b->facet_stride;
                src2.ld_rowmap = in_b->rowmap;
                src2.split = (int)in_b->split;
            }
            if (int rc = launch_col_checked(h->log_m, 2, c, cz, 1, nf * nb, (hipStream_t)stream, in_b ? &src2 : nullptr)) return rc;
        }
    }
    return 0;
}

// The pieces of a wave's window (transform_contributions_pieces, wave_group_finish_pieces): up to two, multiples of 16,
// disjoint, together exactly [0, m), each with rows enough behind its facet stride
static int check_window_pieces(const swiftly_hip_t* h, const char* who, int64_t npieces, const void* const* q,
                               const int64_t* q_facet_strides, const int64_t* n_rows, const int64_t* first,
                               const int64_t* count) {
    if (npieces < 0 || npieces > 2) return fail(SWIFTLY_ERR_PARAM, "%s: 0..2 pieces, got %lld", who, (long long)npieces);
    const int64_t m = h->m;
    int64_t covered = 0;
    for (int64_t i = 0; i < npieces; i++) {
        if (count[i] < 0 || first[i] < 0 || first[i] + count[i] > m || first[i] % 16 || count[i] % 16)
            return fail(SWIFTLY_ERR_PARAM, "%s: piece %lld = [%lld, +%lld) must be multiples of 16 "
                        "inside [0, %lld)", who, (long long)i, (long long)first[i], (long long)count[i], (long long)m);
        if (count[i] && (!q[i] || n_rows[i] <= 0 || n_rows[i] > h->yN || q_facet_strides[i] < n_rows[i] * m))
            return fail(SWIFTLY_ERR_PARAM, "bad row count %lld / facet stride %lld", (long long)n_rows[i], (long long)q_facet_strides[i]);
        covered += count[i];
    }
    if (npieces == 2 && count[0] && count[1] && first[0] < first[1] + count[1] && first[1] < first[0] + count[0])
        return fail(SWIFTLY_ERR_PARAM, "%s: the pieces overlap", who);
    if (covered != m) return fail(SWIFTLY_ERR_PARAM, "%s: the pieces hold %lld of %lld positions", who, (long long)covered, (long long)m);
    return 0;
}

// Who holds what of a checked window: piece *a the positions [split, m) -- or the whole window --, piece *b the positions
// [0, split), -1 where the window lies in one piece
static void window_piece_roles(int64_t m, int64_t npieces, const int64_t* first, const int64_t* count, int* a, int* b) {
    *a = *b = -1;
    for (int64_t i = 0; i < npieces; i++)
        if (count[i]) *(first[i] == 0 && count[i] < m ? b : a) = (int)i;
}

// SWIFTLY_K3_ONE_LAUNCH=0: K3 of a window in two pieces as one launch sequence per piece (A/B runs; swiftly_hip_k3_one_launch)
static std::atomic<int> g_k3_one_launch{getenv("SWIFTLY_K3_ONE_LAUNCH") ? atoi(getenv("SWIFTLY_K3_ONE_LAUNCH")) != 0 : 1};
// SWIFTLY_GROUP_FINISH=0: the callers that own K3 and the finish keep K3 + wave_subgrid_side (A/B runs; swiftly_hip_group_finish)
static std::atomic<int> g_group_finish{getenv("SWIFTLY_GROUP_FINISH") ? atoi(getenv("SWIFTLY_GROUP_FINISH")) != 0 : 1};
// SWIFTLY_GROUP_FINISH_PERSISTENT: 0 = group_finish on one workgroup per tile, 1 = persistent workgroups, one per compute
// unit, n > 1 = at most n of them (swiftly_hip_group_finish_persistent); and the grid of the calling thread's last launch
static std::atomic<int> g_group_finish_persistent{
    getenv("SWIFTLY_GROUP_FINISH_PERSISTENT") ? std::max(0, atoi(getenv("SWIFTLY_GROUP_FINISH_PERSISTENT"))) : 1};
static thread_local int t_group_finish_last_grid = -1;

extern "C" {
int swiftly_hip_k3_one_launch(int on) {
    return on < 0 ? g_k3_one_launch.load() : g_k3_one_launch.exchange(on ? 1 : 0);
}

int swiftly_hip_transform_contributions(swiftly_hip_t* h, int dtype, const void* in, int layout, int64_t in_row_stride,
                                        int64_t in_facet_stride, int64_t in_sub_stride, const int32_t* in_rowmap,
                                        int64_t band_start, int64_t band_len, int64_t nfacets,
                                        const int64_t* facet_off0s, int64_t nsub, const int64_t* subgrid_offs,
                                        void* out, int64_t out_facet_stride, int64_t out_sub_stride, void* stream) {
    if (!h) return fail(SWIFTLY_ERR_PARAM, "null argument");
    DeviceGuard device_guard_(h->device);
    return transform_contributions_impl(h, dtype, in, layout, in_row_stride, in_facet_stride, in_sub_stride, in_rowmap,
                                        band_start, band_len, nfacets, facet_off0s, nsub, subgrid_offs, out,
                                        out_facet_stride, out_sub_stride, nullptr, nullptr, stream);
}

/* K3 + K4a of one wave whose window lies in up to two Q buffers (column slabs of the padded axis): piece i holds the
 * positions [first[i], first[i] + count[i]) of the window, at the same positions of its rows, in q[i] (layout 1:
 * [F, rows kept, m], facet stride q_facet_strides[i], row map rowmaps[i] over n_rows[i] kept rows).  The output is that
 * of transform_contributions layout 1 (or, with g_offsets / g_facet_strides, of wave_facet_side with compute_q = 0) on a Q
 * assembled from the pieces.  Two non-empty pieces are read by ONE launch sequence over the whole window when the
 * column pass has a two-source instance for the case (col_pass_pieces_supported) and swiftly_hip_k3_one_launch is on;
 * otherwise one launch sequence per piece.  A piece with count 0 is skipped. */
int swiftly_hip_transform_contributions_pieces(swiftly_hip_t* h, int dtype, int64_t npieces, const void* const* q,
                                               const int64_t* q_facet_strides, const int32_t* const* rowmaps,
                                               const int64_t* n_rows, const int64_t* first, const int64_t* count,
                                               int64_t nfacets, const int64_t* facet_off0s, int64_t nsub,
                                               const int64_t* sub_off0s, void* g_out, int64_t g_facet_stride,
                                               int64_t g_sub_stride, const int64_t* g_offsets,
                                               const int64_t* g_facet_strides, void* stream) {
    if (!h || !q || !q_facet_strides || !rowmaps || !n_rows || !first || !count || !g_out || !facet_off0s || !sub_off0s)
        return fail(SWIFTLY_ERR_PARAM, "null argument");
    if (!g_offsets != !g_facet_strides) return fail(SWIFTLY_ERR_PARAM, "g_offsets and g_facet_strides go together");
    if (int rc = check_window_pieces(h, "transform_contributions_pieces", npieces, q, q_facet_strides, n_rows, first, count)) return rc;
    DeviceGuard device_guard_(h->device);
    const int64_t m = h->m;
    int a, b;
    window_piece_roles(m, npieces, first, count, &a, &b);
    if (b >= 0 && g_k3_one_launch.load()) {
        const SecondSource second = {q[b], q_facet_strides[b], rowmaps[b], count[b]};
        const int rc = transform_contributions_impl(h, dtype, q[a], 1, m, q_facet_strides[a], 0, rowmaps[a], 0, 0, nfacets,
                                                    facet_off0s, nsub, sub_off0s, g_out, g_facet_stride, g_sub_stride,
                                                    g_offsets, g_facet_strides, stream, 0, -1, &second);
        if (rc != SWIFTLY_ERR_UNSUPPORTED) return rc;  // (no instance: refused before its first launch -- once per piece)
    }
    for (int64_t i = 0; i < npieces; i++) {
        if (!count[i]) continue;
        if (int rc = transform_contributions_impl(h, dtype, q[i], 1, m, q_facet_strides[i], 0, rowmaps[i], 0, 0, nfacets,
                                                  facet_off0s, nsub, sub_off0s, g_out, g_facet_stride, g_sub_stride, g_offsets,
                                                  g_facet_strides, stream, first[i], count[i]))
            return rc;
    }
    return 0;
}

static int sum_finish_facets_impl(swiftly_hip_t* h, int dtype, const void* in, int64_t nfacets, int64_t in_facet_stride,
                                  int64_t in_sub_stride, int64_t in_row_stride, const int64_t* facet_off0s,
                                  const int64_t* facet_off1s, void* out, int64_t out_sub_stride, int64_t out_row_stride,
                                  const int64_t* subgrid_off1s, int64_t subgrid_size, const void* mask,
                                  int64_t mask_batch_stride, int64_t nsub, int placed, void* stream) {
    if (!h || !in || !out || !facet_off0s || !facet_off1s || !subgrid_off1s) return fail(SWIFTLY_ERR_PARAM, "null argument");
    DeviceGuard device_guard_(h->device);
    CHECK_SUBGRID_SIZE();
    const bool c128 = dtype == SWIFTLY_C128;
    CHECK_DTYPE();
    if (nfacets <= 0 || nfacets > kSumFinishMaxFacets)
        return fail(SWIFTLY_ERR_UNSUPPORTED, "sum_finish_facets: 1..%d facets supported", kSumFinishMaxFacets);
    if (c128 && (placed || !sum_finish_c128_supported(h->log_m, h->log_xM)))
        return fail(SWIFTLY_ERR_UNSUPPORTED, "sum_finish_facets: complex128 %s", placed ? "has no placed mode (axis-1-first pipeline)"
                    : ("instances exist for (m, xM) = " + sum_finish_c128_sizes()).c_str());
    if (!sum_finish_supported(h->log_m, h->log_xM))
        return fail(SWIFTLY_ERR_UNSUPPORTED, "sum_finish_facets: (m, xM) = (%lld, %lld) not instantiated", (long long)h->m,
                    (long long)h->xM);
    if (nsub <= 0) return 0;
    const int xM = (int)h->xM, xA = (int)subgrid_size;
    SumFinishFacetArgs a;
    std::memset(&a, 0, sizeof a);
    a.in_fs = in_facet_stride; a.in_bs = in_sub_stride; a.in_rs = in_row_stride;
    a.out_bs = out_sub_stride; a.out_rs = out_row_stride;
    a.nrows = xM;
    a.nfacets = (int)nfacets;
    a.xA = xA;
    fill_facet_groups(a, h, nfacets, facet_off0s, facet_off1s);
    fill_group_rounds(a, h);
    a.placed = placed ? 1 : 0;
    if (placed && h->log_xM > kPlacedMaxLogXM)
        return fail(SWIFTLY_ERR_UNSUPPORTED, "axis-1-first pipeline: rows of %lld points run the wave-parallel sum_finish form, "
                    "which has no placed mode", (long long)h->xM);
    a.mask_bs = mask ? mask_batch_stride : 0;
    // (the complex128 instances read no compact copies; the block carries them all the same)
    if (int rc = fill_sum_finish_tables(h, c128, &a.fn, &a.tw_m, &a.tw_x, &a.twc_m, &a.twc_x)) return rc;
    for (int64_t b0 = 0; b0 < nsub; b0 += kSumFinishMaxBatch) {
        const int nb = (int)std::min<int64_t>(kSumFinishMaxBatch, nsub - b0);
        a.in = cx_at(in, b0 * in_sub_stride, c128);
        a.out = cx_at(out, b0 * out_sub_stride, c128);
        // (mask: float, or double with complex128 data)
        a.mask = mask ? (const float*)((const char*)mask + b0 * mask_batch_stride * (c128 ? 8 : 4)) : nullptr;
        for (int b = 0; b < nb; b++) a.st_a[b] = subgrid_in_padded_subgrid(*h, xA, subgrid_off1s[b0 + b]).a;
        int e = c128 ? launch_sum_finish_facets_c128(h->log_m, h->log_xM, a, nb, (hipStream_t)stream)
                     : launch_sum_finish_facets(h->log_m, h->log_xM, a, nb, (hipStream_t)stream);
        if (int rc = launch_status(e)) return rc;
    }
    return 0;
}

int swiftly_hip_sum_finish_facets(swiftly_hip_t* h, int dtype, const void* in, int64_t nfacets, int64_t in_facet_stride,
                                  int64_t in_sub_stride, int64_t in_row_stride, const int64_t* facet_off0s,
                                  const int64_t* facet_off1s, void* out, int64_t out_sub_stride, int64_t out_row_stride,
                                  const int64_t* subgrid_off1s, int64_t subgrid_size, const void* mask,
                                  int64_t mask_batch_stride, int64_t nsub, void* stream) {
    return sum_finish_facets_impl(h, dtype, in, nfacets, in_facet_stride, in_sub_stride, in_row_stride, facet_off0s, facet_off1s,
                                  out, out_sub_stride, out_row_stride, subgrid_off1s, subgrid_size, mask, mask_batch_stride, nsub,
                                  0, stream);
}

/* AXIS-1-FIRST pipeline (r6), step R: the contiguous-axis half of add_to_subgrid (core.py:255-285) on the rows of the K1
 * band buffers of all facets, for the wave `wave_off1`, BEFORE the strided-axis transforms (swiftly_sumfinish.h,
 * axis1_rows_kernel).  out[f] = [rows, m] in the parity-split layout of a band that is exactly the wave's window
 * (start (yN/2 - m/2 + s) mod yN, length m): hand it to prepare_facet_columns / wave_facet_side with that band. */
int swiftly_hip_finish_axis1_rows(swiftly_hip_t* h, int dtype, const void* bands, int64_t rows, int64_t band_row_stride,
                                  int64_t band_facet_stride, int64_t nfacets, const int64_t* facet_off1s,
                                  int64_t band_start, int64_t band_len, int64_t wave_off1, void* out,
                                  int64_t out_row_stride, int64_t out_facet_stride, void* stream) {
    if (!h || !bands || !out || !facet_off1s) return fail(SWIFTLY_ERR_PARAM, "null argument");
    DeviceGuard device_guard_(h->device);
    if (dtype != SWIFTLY_C64) return fail(SWIFTLY_ERR_UNSUPPORTED, "finish_axis1_rows: complex64 only");
    if (!band_is_split(h) || h->log_m < 7 || h->log_m > 10)
        return fail(SWIFTLY_ERR_UNSUPPORTED, "finish_axis1_rows: needs the parity-split band layout (yN_size 16384 .. 65536) and "
                    "m = 128 .. 1024");
    if (nfacets <= 0 || nfacets > kSumFinishMaxFacets)
        return fail(SWIFTLY_ERR_UNSUPPORTED, "finish_axis1_rows: 1..%d facets supported", kSumFinishMaxFacets);
    const int yN = (int)h->yN, m = (int)h->m;
    CHECK_BAND();
    if (rows <= 0) return 0;
    Axis1RowsArgs a;
    std::memset(&a, 0, sizeof a);
    a.in = (const cx<float>*)bands; a.out = (cx<float>*)out;
    a.in_fs = band_facet_stride; a.in_rs = band_row_stride; a.out_fs = out_facet_stride; a.out_rs = out_row_stride;
    a.nrows = (int)rows; a.yN = yN;
    a.band_start = (int)band_start; a.band_len = (int)band_len; a.band_half = (int)band_half_columns(band_len);
    const Window w = window_of(*h, wave_off1);
    a.c0 = w.base;
    a.s = pmod(w.s, m);
    // every column of the window must lie inside the band
    if (window_in_band(*h, w, 0, m, band_start, band_len) >= 0)
        return fail(SWIFTLY_ERR_PARAM, "finish_axis1_rows: the window of off1 = %lld is not inside the band", (long long)wave_off1);
    for (int64_t f = 0; f < nfacets; f++) a.sp[f] = pmod(facet_shift(*h, facet_off1s[f]), m);
    if (int rc = fill_sum_finish_tables(h, false, &a.fn, &a.tw_m, nullptr, &a.twc_m, nullptr)) return rc;
    return launch_status(launch_axis1_rows(h->log_m, a, (int)nfacets, (hipStream_t)stream), nullptr, "no instance");
}

/* AXIS-1-FIRST pipeline, the finish inside K2: finish_axis1_rows + prepare_facet_columns for one wave in two launches that
 * never write the finished rows (swiftly_colaxis1.h: pass A' of the four-step; pass B is prepare_facet_columns' own).  The
 * argument checks of the two calls it replaces. */
int swiftly_hip_prepare_facet_columns_axis1(swiftly_hip_t* h, int dtype, const void* bands, int64_t rows,
                                            int64_t band_row_stride, int64_t band_facet_stride, int64_t nfacets,
                                            const int64_t* facet_off0s, const int64_t* facet_off1s, int64_t band_start,
                                            int64_t band_len, int64_t wave_off1, void* out, int64_t out_row_stride,
                                            int64_t out_facet_stride, const int32_t* out_rowmap, void* workspace,
                                            int64_t workspace_bytes, void* stream) {
    if (!h || !bands || !out || !facet_off0s || !facet_off1s) return fail(SWIFTLY_ERR_PARAM, "null argument");
    DeviceGuard device_guard_(h->device);
    CHECK_DTYPE();
    if (std::string why = why_not_axis1_columns(*h, dtype); !why.empty())
        return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_columns_axis1: %s", why.c_str());
    if (nfacets <= 0 || nfacets > kSumFinishMaxFacets)
        return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_columns_axis1: 1..%d facets supported", kSumFinishMaxFacets);
    const int yN = (int)h->yN, m = (int)h->m;
    if (rows <= 0 || rows >= yN) return fail(SWIFTLY_ERR_PARAM, "facet size %lld must be in [1, yN_size - 1]", (long long)rows);
    CHECK_BAND();
    const Window w = window_of(*h, wave_off1);
    if (window_in_band(*h, w, 0, m, band_start, band_len) >= 0)
        return fail(SWIFTLY_ERR_PARAM, "prepare_facet_columns_axis1: the window of off1 = %lld is not inside the band",
                    (long long)wave_off1);
    const int64_t band_half = band_half_columns(band_len);
    if (out_row_stride < m || band_row_stride < 2 * band_half)
        return fail(SWIFTLY_ERR_PARAM, "prepare_facet_columns_axis1: out_row_stride %lld below m = %d, or band_row_stride %lld "
                    "below the band's %lld physical columns", (long long)out_row_stride, m, (long long)band_row_stride,
                    (long long)(2 * band_half));
    CHECK_OFFSETS_32(offsets_fit_32(yN, out_row_stride) && offsets_fit_32(yN, m));
    // pass B: the store side of prepare_facet_columns (whole(yN), the wave's row map, 1 / yN, conjugated back)
    ColPassArgs c = col_pass_args(whole(rows), whole(yN));
    c.ncols = m;
    c.full_logn = h->log_yN;
    c.out_pitch = (unsigned)out_row_stride;
    c.scale = (float)(1.0 / yN);
    c.conj_ld = c.conj_st = 1;
    c.st_rowmap = out_rowmap;
    // pass A': the row finish of finish_axis1_rows behind the load map of prepare_facet_columns
    ColAxis1Args a;
    std::memset(&a, 0, sizeof a);
    a.in_fs = band_facet_stride; a.in_rs = band_row_stride;
    a.rows = (int)rows; a.yN = yN;
    a.band_start = (int)band_start; a.band_len = (int)band_len; a.band_half = (int)band_half;
    a.c0 = w.base;
    a.s = pmod(w.s, m);
    if (int rc = fill_sum_finish_tables(h, false, &a.fn, &a.tw_m, nullptr, &a.twc_m, nullptr)) return rc;
    const size_t ws_bytes = workspace ? (size_t)std::max<int64_t>(0, workspace_bytes) : 0;
    for (int64_t f0 = 0; f0 < nfacets; f0 += kColZF) {
        const int nf = (int)std::min<int64_t>(kColZF, nfacets - f0);
        for (int f = 0; f < nf; f++) {
            a.sp[f] = pmod(facet_shift(*h, facet_off1s[f0 + f]), m);
            a.ld_a[f] = facet_in_padded_facet(*h, rows, facet_off0s[f0 + f]).a;
        }
        a.in = (const cx<float>*)bands + f0 * band_facet_stride;
        // item z = facet: reads its slot of the scratch, writes out[f]
        c.out = (cx<float>*)out + f0 * out_facet_stride;
        c.out_bdiv = 1; c.out_bs_hi = out_facet_stride; c.out_bs = 0;
        const int rc = col_transform_axis1(h, c, plain_colz(), a, nf, (hipStream_t)stream, workspace, ws_bytes);
        if (rc == -1) return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_columns_axis1: no instance for yN %d, m %d", yN, m);
        if (rc) return rc;
    }
    return 0;
}

/* Backward subgrid side, contiguous-axis half + axis-0 remainder (see swiftly_sumfinish.h): in[b] = [xM, xA] =
 * prepare_subgrid(axis 0) of subgrid b; out[f][b] = [m, m] = the contribution of subgrid b to facet f
 * (api_helper.prepare_and_split_subgrid, api_helper.py:115-139). */
int swiftly_hip_split_prepare_facets(swiftly_hip_t* h, int dtype, const void* in, int64_t in_sub_stride,
                                     int64_t in_row_stride, int64_t subgrid_size, int64_t nsub,
                                     const int64_t* subgrid_off1s, int64_t nfacets, const int64_t* facet_off0s,
                                     const int64_t* facet_off1s, void* out, int64_t out_facet_stride,
                                     int64_t out_sub_stride, void* stream) {
    if (!h || !in || !out || !facet_off0s || !facet_off1s || !subgrid_off1s) return fail(SWIFTLY_ERR_PARAM, "null argument");
    DeviceGuard device_guard_(h->device);
    CHECK_SUBGRID_SIZE();
    const bool c128 = dtype == SWIFTLY_C128;
    CHECK_DTYPE();
    if (nfacets <= 0) return fail(SWIFTLY_ERR_UNSUPPORTED, "split_prepare_facets: 1..%d facets supported", kSumFinishMaxFacets);
    // (the gate of swiftly_hip_supports(SPLIT_PREPARE): a caller that asked it is never refused here)
    if (const std::string why = why_not_split_prepare(*h, dtype, nfacets); !why.empty())
        return fail(SWIFTLY_ERR_UNSUPPORTED, "split_prepare_facets: %s", why.c_str());
    if (nsub <= 0) return 0;
    const int xM = (int)h->xM, xA = (int)subgrid_size, m = (int)h->m;
    SplitFacetArgs a;
    std::memset(&a, 0, sizeof a);
    a.in_bs = in_sub_stride; a.in_rs = in_row_stride;
    a.out_fs = out_facet_stride; a.out_bs = out_sub_stride; a.out_rs = m;
    a.nrows = xM;
    a.nfacets = (int)nfacets;
    a.xA = xA;
    fill_facet_groups(a, h, nfacets, facet_off0s, facet_off1s);
    // (the complex128 instances read no compact copies)
    if (int rc = fill_sum_finish_tables(h, c128, &a.fn, &a.tw_m, &a.tw_x, c128 ? nullptr : &a.twc_m, c128 ? nullptr : &a.twc_x))
        return rc;
    for (int64_t b0 = 0; b0 < nsub; b0 += kSumFinishMaxBatch) {
        const int nb = (int)std::min<int64_t>(kSumFinishMaxBatch, nsub - b0);
        a.in = cx_at(in, b0 * in_sub_stride, c128);
        a.out = cx_at(out, b0 * out_sub_stride, c128);
        for (int b = 0; b < nb; b++) a.ld_a[b] = subgrid_in_padded_subgrid(*h, xA, subgrid_off1s[b0 + b]).a;
        int e = c128 ? launch_split_prepare_facets_c128(h->log_m, h->log_xM, a, nb, (hipStream_t)stream)
                     : launch_split_prepare_facets(h->log_m, h->log_xM, a, nb, (hipStream_t)stream);
        if (int rc = launch_status(e, nullptr, "no instance")) return rc;
    }
    // axis-0 remainder of extract_from_subgrid, in place: out[f][b][:, j] = cifft_m( Fn[k] * E[f][b][(k - s'0_f) ..., j] )
    ColPassArgs c = col_pass_args(whole(m), whole(m));
    c.ncols = m;
    c.full_logn = h->log_m;
    c.in_pitch = c.out_pitch = (unsigned)m;
    c.ld_win = c128 ? (const float*)h->fn_d : h->fn_f;  // (complex128: the double table)
    c.conj_ld = c.conj_st = 1;
    c.scale = 1.f / (float)m;  // (a power of two: exact in either precision)
    c.tw = twiddles<float>(h, h->log_m);
    for (int64_t f0 = 0; f0 < nfacets; f0 += kColZF) {
        const int nf = (int)std::min<int64_t>(kColZF, nfacets - f0);
        for (int64_t b0 = 0; b0 < nsub; b0 += kColZB) {
            const int nb = (int)std::min<int64_t>(kColZB, nsub - b0);
            ColZ cz = plain_colz();
            cz.nb = nb;
            cz.flags = kZLoadAF;
            for (int f = 0; f < nf; f++) cz.f_lda[f] = contribution_in_padded_subgrid(*h, facet_off0s[f0 + f]).a;
            c.in = cx_at((const void*)out, f0 * out_facet_stride + b0 * out_sub_stride, c128);
            c.in_bdiv = nb; c.in_bs_hi = out_facet_stride; c.in_bs = out_sub_stride;
            c.out = cx_at(out, f0 * out_facet_stride + b0 * out_sub_stride, c128);
            c.out_bdiv = nb; c.out_bs_hi = out_facet_stride; c.out_bs = out_sub_stride;
            if (int rc = set_col_precision(h, c, h->log_m, c128)) return rc;  // (complex128: m <= 512, one pass)
            if (int rc = launch_col_checked(h->log_m, 2, c, cz, 1, nf * nb, (hipStream_t)stream)) return rc;
        }
    }
    return 0;
}

/* The whole subgrid side of one backward wave natively, without stream-ordered allocations: prepare_subgrid along
 * axis 0 (four-step through `work`) + split_prepare_facets.  work: device scratch of >= 2 * nsub * xM * subgrid_size
 * complex elements of `dtype` (first half: tmp[nsub][xM][subgrid_size], second half: four-step scratch). */
int swiftly_hip_wave_split_subgrids(swiftly_hip_t* h, int dtype, const void* subgrids, int64_t subgrid_size, int64_t nsub,
                                    const int64_t* subgrid_off0s, const int64_t* subgrid_off1s, int64_t nfacets,
                                    const int64_t* facet_off0s, const int64_t* facet_off1s, void* work,
                                    int64_t work_elems, void* out, int64_t out_facet_stride, int64_t out_sub_stride,
                                    void* stream) {
    if (!h || !subgrids || !work || !out || !subgrid_off0s || !subgrid_off1s) return fail(SWIFTLY_ERR_PARAM, "null argument");
    DeviceGuard device_guard_(h->device);
    CHECK_SUBGRID_SIZE();
    const bool c128 = dtype == SWIFTLY_C128;
    CHECK_DTYPE();
    // (refused before the first launch: the gate of split_prepare_facets)
    if (const std::string why = why_not_split_prepare(*h, dtype, nfacets); !why.empty())
        return fail(SWIFTLY_ERR_UNSUPPORTED, "wave_split_subgrids: %s", why.c_str());
    if (nsub <= 0 || nfacets <= 0) return 0;
    const int xM = (int)h->xM, xA = (int)subgrid_size;
    const int64_t half = nsub * (int64_t)xM * xA;
    if (work_elems < 2 * half) return fail(SWIFTLY_ERR_PARAM, "work holds %lld elements, %lld needed", (long long)work_elems, (long long)(2 * half));
    void* tmp = work;
    const size_t esz = c128 ? sizeof(cx<double>) : sizeof(cx<float>);
    ColPassArgs c = col_pass_args(whole(xA), whole(xM));
    c.c128 = c128 ? 1 : 0;
    c.ncols = xA;
    c.full_logn = h->log_xM;
    c.in_pitch = c.out_pitch = (unsigned)xA;
    c.scale = 1.f;
    for (int64_t b0 = 0; b0 < nsub; b0 += kColZB) {
        const int nb = (int)std::min<int64_t>(kColZB, nsub - b0);
        ColZ cz = plain_colz();
        cz.nb = nb;
        cz.flags = kZLoadB;
        for (int b = 0; b < nb; b++) {
            cz.b_lda[b] = subgrid_in_padded_subgrid(*h, xA, subgrid_off0s[b0 + b]).a;
            cz.b_ldc[b] = 0;
        }
        c.in = cx_at(subgrids, b0 * (int64_t)xA * xA, c128);
        c.in_bs = (long long)xA * xA;
        c.out = cx_at(tmp, b0 * (int64_t)xM * xA, c128);
        c.out_bs = (long long)xM * xA;
        const int rc = col_transform(h, h->log_xM, c, cz, xA, nb, (hipStream_t)stream, cx_at(tmp, half, c128), (size_t)half * esz);
        if (rc == -1) return fail(SWIFTLY_ERR_UNSUPPORTED, "wave_split_subgrids: padded subgrid size %d not supported", xM);
        if (rc) return rc;
    }
    return swiftly_hip_split_prepare_facets(h, dtype, tmp, (int64_t)xM * xA, xA, subgrid_size, nsub, subgrid_off1s, nfacets,
                                            facet_off0s, facet_off1s, out, out_facet_stride, out_sub_stride, stream);
}


/* One forward wave in two calls (the whole launch sequence runs natively: per-wave host work is two ABI calls). */
int swiftly_hip_wave_facet_side(swiftly_hip_t* h, int dtype, const void* bands, int64_t rows, int64_t band_row_stride,
                                int64_t band_facet_stride, int64_t nfacets, const int64_t* facet_off0s,
                                int64_t band_start, int64_t band_len, int64_t wave_off1, const int32_t* rowmap,
                                int64_t n_rows, void* q_work, int64_t q_facet_stride, int compute_q, int64_t nsub,
                                const int64_t* sub_off0s, void* g_out,
                                int64_t g_facet_stride, int64_t g_sub_stride, const int64_t* g_offsets,
                                const int64_t* g_facet_strides, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!h || (!bands && compute_q) || !q_work || !g_out || !facet_off0s || !sub_off0s) return fail(SWIFTLY_ERR_PARAM, "null argument");
    if (nfacets <= 0 || nsub <= 0) return 0;
    const int64_t m = h->m;
    if (n_rows <= 0 || n_rows > h->yN || q_facet_stride < n_rows * m)
        return fail(SWIFTLY_ERR_PARAM, "bad row count %lld / facet stride %lld", (long long)n_rows, (long long)q_facet_stride);
    // K2: Q[f] = [n_rows, m] (skipped when the caller still holds the wave's Q: compute_q = 0)
    DeviceGuard device_guard_(h->device);
    if (compute_q) {
        int rc = prepare_facet_columns_impl(h, dtype, bands, rows, band_row_stride, band_facet_stride, nfacets, facet_off0s,
                                            band_start, band_len, 1, &wave_off1, q_work, m, q_facet_stride, 0, rowmap, 0,
                                            stream, scratch, scratch ? (size_t)scratch_bytes : 0);
        if (rc) return rc;
    }
    // K3 + K4a from Q (layout 1)
    return transform_contributions_impl(h, dtype, q_work, 1, m, q_facet_stride, 0, rowmap, 0, 0, nfacets, facet_off0s, nsub,
                                        sub_off0s, g_out, g_facet_stride, g_sub_stride, g_offsets, g_facet_strides, stream);
}

static int wave_subgrid_side_impl(swiftly_hip_t* h, int dtype, const void* g, int64_t nfacets, int64_t g_facet_stride,
                                  int64_t g_sub_stride, const int64_t* facet_off0s, const int64_t* facet_off1s,
                                  int64_t nsub, const int64_t* sub_off0s, const int64_t* sub_off1s, int64_t subgrid_size,
                                  const void* mask0, int64_t mask0_bs, const void* mask1, int64_t mask1_bs,
                                  void* tmp_work, void* out, void* scratch, int64_t scratch_bytes, int placed, void* stream) {
    if (!h || !g || !tmp_work || !out || !sub_off0s || !sub_off1s) return fail(SWIFTLY_ERR_PARAM, "null argument");
    if (nsub <= 0) return 0;
    const int64_t m = h->m, xM = h->xM, xA = subgrid_size;
    // K4b + K5a: tmp[b] = [xM, xA]
    int rc = sum_finish_facets_impl(h, dtype, g, nfacets, g_facet_stride, g_sub_stride, m, facet_off0s, facet_off1s,
                                    tmp_work, xM * xA, xA, sub_off1s, subgrid_size, mask1, mask1_bs, nsub, placed, stream);
    if (rc) return rc;
    // K5b: finish_subgrid along axis 0 (strided): rows of the op = xA columns
    CallWorkspace call_ws(scratch, scratch ? (size_t)scratch_bytes : 0);
    return swiftly_hip_finish_subgrid_batch(h, dtype, tmp_work, xA, 1, xA, out, 1, xA, 0, subgrid_size, mask0, nsub,
                                            xM * xA, xA * xA, sub_off0s, mask0 ? mask0_bs : 0, stream);
}

int swiftly_hip_wave_subgrid_side(swiftly_hip_t* h, int dtype, const void* g, int64_t nfacets, int64_t g_facet_stride,
                                  int64_t g_sub_stride, const int64_t* facet_off0s, const int64_t* facet_off1s,
                                  int64_t nsub, const int64_t* sub_off0s, const int64_t* sub_off1s, int64_t subgrid_size,
                                  const void* mask0, int64_t mask0_bs, const void* mask1, int64_t mask1_bs,
                                  void* tmp_work, void* out, void* scratch, int64_t scratch_bytes, void* stream) {
    return wave_subgrid_side_impl(h, dtype, g, nfacets, g_facet_stride, g_sub_stride, facet_off0s, facet_off1s, nsub, sub_off0s,
                                  sub_off1s, subgrid_size, mask0, mask0_bs, mask1, mask1_bs, tmp_work, out, scratch, scratch_bytes,
                                  0, stream);
}

/* wave_subgrid_side of the AXIS-1-FIRST pipeline: the blocks g[f][b] come from band buffers that went through
 * swiftly_hip_finish_axis1_rows, i.e. their rows already are Fn * cfft_m along the contiguous axis: sum_finish_facets
 * places and sums them without its m-point transforms. */
int swiftly_hip_wave_subgrid_side_placed(swiftly_hip_t* h, int dtype, const void* g, int64_t nfacets, int64_t g_facet_stride,
                                         int64_t g_sub_stride, const int64_t* facet_off0s, const int64_t* facet_off1s,
                                         int64_t nsub, const int64_t* sub_off0s, const int64_t* sub_off1s,
                                         int64_t subgrid_size, const void* mask0, int64_t mask0_bs, const void* mask1,
                                         int64_t mask1_bs, void* tmp_work, void* out, void* scratch, int64_t scratch_bytes,
                                         void* stream) {
    return wave_subgrid_side_impl(h, dtype, g, nfacets, g_facet_stride, g_sub_stride, facet_off0s, facet_off1s, nsub, sub_off0s,
                                  sub_off1s, subgrid_size, mask0, mask0_bs, mask1, mask1_bs, tmp_work, out, scratch, scratch_bytes,
                                  1, stream);
}


/* The subgrid side of a wave with the strided axis finished first (swiftly_groupfinish.h): group_finish from the K2 pieces
 * into T[g][b][xM rows, subgrid_size used][m], then sum_finish_facets over the rows of T.  The row kernel is the one
 * wave_subgrid_side runs, unchanged: a group's T[g][b] enters it as xM / m "facets" of m rows each (entry c = rows
 * [c m, (c + 1) m), band start c m), so every row is covered by exactly one entry per group and is read as it lies. */
int swiftly_hip_group_finish(int on) {
    return on < 0 ? g_group_finish.load() : g_group_finish.exchange(on ? 1 : 0);
}

int swiftly_hip_group_finish_persistent(int n) {
    if (n == -2) return t_group_finish_last_grid;
    return n < 0 ? g_group_finish_persistent.load() : g_group_finish_persistent.exchange(n);
}

int swiftly_hip_wave_group_finish_pieces(swiftly_hip_t* h, int dtype, int64_t npieces, const void* const* q,
                                         const int64_t* q_facet_strides, const int32_t* const* rowmaps,
                                         const int64_t* n_rows, const int64_t* first, const int64_t* count,
                                         int64_t nfacets, const int64_t* facet_off0s, const int64_t* facet_off1s,
                                         int64_t nsub, const int64_t* sub_off0s, const int64_t* sub_off1s,
                                         int64_t subgrid_size, const void* mask0, int64_t mask0_bs, const void* mask1,
                                         int64_t mask1_bs, void* t_work, int64_t t_work_elems, void* out, int stages,
                                         void* stream) {
    if (!h || !q || !q_facet_strides || !rowmaps || !n_rows || !first || !count || !t_work || !facet_off0s || !facet_off1s ||
        !sub_off0s || !sub_off1s || (!out && (stages & 2)))
        return fail(SWIFTLY_ERR_PARAM, "null argument");
    if (stages < 1 || stages > 3) return fail(SWIFTLY_ERR_PARAM, "wave_group_finish_pieces: stages must be 1, 2 or 3");
    CHECK_SUBGRID_SIZE();
    if (nfacets <= 0) return fail(SWIFTLY_ERR_UNSUPPORTED, "wave_group_finish_pieces: 1..%d facets supported", kGroupFinishMaxFacets);
    // (the gate of swiftly_hip_supports(GROUP_FINISH): a caller that asked it is never refused here)
    if (const std::string why = why_not_group_finish(*h, dtype, nfacets); !why.empty())
        return fail(SWIFTLY_ERR_UNSUPPORTED, "wave_group_finish_pieces: %s", why.c_str());
    if (h->col_f64)
        return fail(SWIFTLY_ERR_UNSUPPORTED, "wave_group_finish_pieces: float32 column arithmetic only (column precision is 64)");
    if (int rc = check_window_pieces(h, "wave_group_finish_pieces", npieces, q, q_facet_strides, n_rows, first, count)) return rc;
    if (nsub <= 0) return 0;
    DeviceGuard device_guard_(h->device);
    const int m = (int)h->m, xM = (int)h->xM, xA = (int)subgrid_size, yN = (int)h->yN, ratio = xM / m;
    CHECK_OFFSETS_32(offsets_fit_32(yN, m, yN));

    SumFinishFacetArgs r;  // stage 2; its facet tables first serve as the grouping of the real facets
    std::memset(&r, 0, sizeof r);
    fill_facet_groups(r, h, nfacets, facet_off0s, facet_off1s);
    const int ngroups = r.ngroups;
    if (t_work_elems < (int64_t)ngroups * nsub * xM * m)
        return fail(SWIFTLY_ERR_PARAM, "t_work holds %lld elements, %lld needed", (long long)t_work_elems,
                    (long long)((int64_t)ngroups * nsub * xM * m));
    GroupFinishArgs a;
    std::memset(&a, 0, sizeof a);
    for (int n = 0; n < nfacets; n++) {
        a.fidx[n] = r.fidx[n];
        a.sp0[n] = (int)facet_shift(*h, facet_off0s[r.fidx[n]]);
    }
    for (int g = 0; g <= ngroups; g++) a.gstart[g] = r.gstart[g];
    int pa, pb;
    window_piece_roles(m, npieces, first, count, &pa, &pb);
    a.in_a = (const cx<float>*)q[pa]; a.in_fs_a = q_facet_strides[pa]; a.rowmap_a = rowmaps[pa];
    if (pb >= 0) {
        a.in_b = (const cx<float>*)q[pb]; a.in_fs_b = q_facet_strides[pb]; a.rowmap_b = rowmaps[pb];
        a.split = (int)count[pb];
    }
    a.in_pitch = (unsigned)m;
    a.out_gs = (long long)nsub * xM * m; a.out_bs = (long long)xM * m;
    a.yN = yN; a.xA = xA; a.ncols = m;
    a.fn = h->fn_f;
    a.tw_m = twiddles<float>(h, h->log_m);
    a.tw_x = twiddles<float>(h, h->log_xM);
    if (!a.fn || !a.tw_m || !a.tw_x) return fail(SWIFTLY_ERR_HIP, "internal: missing twiddle tables");
    a.mask_bs = mask0 ? mask0_bs : 0;

    // the row kernel's view of T: xM / m entries of m rows per group
    for (int g = 0; g < ngroups; g++) {
        r.gstart[g] = g * ratio;
        for (int c = 0; c < ratio; c++) {
            r.fidx[g * ratio + c] = (int)((int64_t)g * nsub * ratio + c);
            r.base0[g * ratio + c] = c * m;
        }
    }
    r.gstart[ngroups] = ngroups * ratio;
    r.nfacets = ngroups * ratio;
    r.in_fs = (long long)m * m; r.in_bs = (long long)xM * m; r.in_rs = m;
    r.out_bs = (long long)xA * xA; r.out_rs = xA;
    r.nrows = xA;  // the rows group_finish kept
    r.xA = xA;
    fill_group_rounds(r, h);
    r.mask_bs = mask1 ? mask1_bs : 0;
    if (int rc = fill_sum_finish_tables(h, false, &r.fn, &r.tw_m, &r.tw_x, &r.twc_m, &r.twc_x)) return rc;

    static_assert(kGroupFinishMaxBatch == kSumFinishMaxBatch, "one batch loop");
    for (int64_t b0 = 0; b0 < nsub; b0 += kGroupFinishMaxBatch) {
        const int nb = (int)std::min<int64_t>(kGroupFinishMaxBatch, nsub - b0);
        if (stages & 1) {
            a.out = (cx<float>*)t_work + b0 * a.out_bs;
            a.mask = mask0 ? (const float*)mask0 + b0 * mask0_bs : nullptr;
            for (int b = 0; b < nb; b++) {
                const Window w = window_of(*h, sub_off0s[b0 + b]);
                a.lda[b] = w.rot;
                a.ldc[b] = w.base;
                a.st_a[b] = subgrid_in_padded_subgrid(*h, xA, sub_off0s[b0 + b]).a;
            }
            const int persistent = g_group_finish_persistent.load();
            const int grid_cap = persistent == 1 ? h->cu_count : persistent;
            if (int rc = launch_status(launch_group_finish(h->log_m, h->log_xM, a, nb, ngroups, grid_cap, (hipStream_t)stream),
                                       "group_finish", "no instance"))
                return rc;
            t_group_finish_last_grid = (int)std::min<int64_t>((int64_t)((m + 15) / 16) * nb * ngroups, grid_cap);
        }
        if (stages & 2) {
            r.in = (const cx<float>*)t_work + b0 * r.in_bs;
            r.out = (cx<float>*)out + b0 * r.out_bs;
            r.mask = mask1 ? (const float*)mask1 + b0 * mask1_bs : nullptr;
            for (int b = 0; b < nb; b++) r.st_a[b] = subgrid_in_padded_subgrid(*h, xA, sub_off1s[b0 + b]).a;
            if (int rc = launch_status(launch_sum_finish_facets(h->log_m, h->log_xM, r, nb, (hipStream_t)stream))) return rc;
        }
    }
    return 0;
}

int swiftly_hip_accumulate_facet_columns(swiftly_hip_t* h, int dtype, const void* parts, int64_t part_row_stride,
                                         int64_t nchunks, const int64_t* chunk_offsets,
                                         const int64_t* chunk_facet_strides, const int32_t* row_sources,
                                         int64_t nfacets, const int64_t* facet_off0s, int64_t facet_size,
                                         const void* masks, int64_t subgrid_off1, void* bands, int64_t band_row_stride,
                                         int64_t band_facet_stride, int64_t band_start, int64_t band_len,
                                         unsigned char* touched, void* workspace, int64_t workspace_bytes,
                                         void* stream) {
    if (!h || !parts || !bands || !chunk_offsets || !chunk_facet_strides || !row_sources || !facet_off0s)
        return fail(SWIFTLY_ERR_PARAM, "null argument");
    DeviceGuard device_guard_(h->device);
    const bool c128 = dtype == SWIFTLY_C128;
    CHECK_DTYPE();
    CHECK_FACET_SIZE();
    const int yN = (int)h->yN, m = (int)h->m;
    const swiftly_hip::Mixed* mx = nullptr;  // yN = Q * 2^k: radix-Q pass with the gather-sum load + sub-transforms
    if (h->log_yN < 0) {
        auto it = h->mixed.find(h->yN);
        if (it != h->mixed.end() && it->second.tw_f && !band_is_split(h)) mx = &it->second;
    }
    // (the gate of swiftly_hip_supports(BACKWARD_BAND_EXPLICIT), in complex64 identical to BACKWARD_BAND: a caller that asked
    // it is never refused here)
    if (const std::string why = why_not_backward_band(*h, dtype, true); !why.empty())
        return fail(SWIFTLY_ERR_UNSUPPORTED, "accumulate_facet_columns: %s", why.c_str());
    if (h->log_yN < 0 && !mx)
        return fail(SWIFTLY_ERR_UNSUPPORTED, "accumulate_facet_columns: yN %lld = Q * 2^k has no complex64 radix-Q table "
                    "(2^k above %d), or would need the split band layout", (long long)h->yN, 1 << kBandMixedMaxLog);
    if (nchunks <= 0 || nchunks > kColZC) return fail(SWIFTLY_ERR_PARAM, "1..%d source chunks", kColZC);
    CHECK_BAND();
    if (nfacets <= 0) return 0;
    // (ELEMENT offsets, of either storage type)
    CHECK_OFFSETS_32(offsets_fit_32(facet_size, band_row_stride) && offsets_fit_32(uint64_t(1) << kGsRowBits, part_row_stride));
    const int lo = facet_lo(*h, facet_size);
    ColPassArgs c = col_pass_args(whole(yN), whole(facet_size));
    c.ncols = m;
    c.full_logn = h->log_yN;
    c.in = (const cx<float>*)parts;
    c.in_pitch = (unsigned)part_row_stride;
    c.out_pitch = (unsigned)band_row_stride;
    c.ld_rowmap = row_sources; c.gs = 1;
    c.f64 = h->col_f64;  // (complex128 storage: always float64 arithmetic, the column_precision setting does not matter)
    c.c128 = c128 ? 1 : 0;
    // masks and 1/pswf: float tables, double ones with complex128 storage (the kernel reinterprets the pointers)
    const size_t rsz = c128 ? sizeof(double) : sizeof(float);
    c.st_win = (const float*)masks; c.st_win_bs = masks ? facet_size : 0;
    c.st_win2 = c128 ? (const float*)(h->invp_d + lo) : h->invp_f + lo;
    c.scale = 1.f;
    c.accumulate = 1;
    c.touched = touched;
    c.cg_mod = m; c.cg_full = yN;
    c.cg_band_start = (int)band_start; c.cg_band_len = (int)band_len; c.cg_band_half = 0;
    const int64_t cap = workspace ? workspace_bytes : (int64_t(4) << 30);
    const int64_t per_item = mx ? (int64_t)MixedWorkspace(1, yN, 1ll << mx->logM, m).bytes() : (int64_t)yN * m * (c128 ? 16 : 8);
    const int per_f = (int)std::max<int64_t>(1, std::min<int64_t>(kColZF, cap / per_item));
    const Window win = window_of(*h, subgrid_off1);
    for (int64_t f0 = 0; f0 < nfacets; f0 += per_f) {
        const int nf = (int)std::min<int64_t>(per_f, nfacets - f0);
        ColZ cz = plain_colz();
        cz.flags = kZColScatter | kZStoreAF;
        cz.nb = 1;
        cz.b_rot[0] = win.rot;
        cz.b_base[0] = win.base;
        for (int f = 0; f < nf; f++) cz.f_sta[f] = facet_in_padded_facet(*h, facet_size, facet_off0s[f0 + f]).a;
        for (int k = 0; k < nchunks; k++) {
            cz.c_base[k] = chunk_offsets[k] + f0 * chunk_facet_strides[k];
            cz.c_fs[k] = chunk_facet_strides[k];
        }
        c.out = cx_at(bands, f0 * band_facet_stride, c128);
        c.out_bs = band_facet_stride;
        if (masks) c.st_win = (const float*)((const char*)masks + (size_t)(f0 * facet_size) * rsz);
        int rc = 0;
        if (!mx) {
            rc = col_transform(h, h->log_yN, c, cz, m, nf, (hipStream_t)stream, workspace,
                               workspace ? (size_t)workspace_bytes : 0);
        } else {
            const int Q = mx->Q, logM = mx->logM;
            const long long M = 1ll << logM;
            const MixedWorkspace part(nf, yN, M, m);
            hipStream_t st = (hipStream_t)stream;
            ScratchLease lease;
            if ((rc = lease.acquire(workspace, (size_t)workspace_bytes, part.bytes(), st, "hipMallocAsync(&own, radix_bytes + sub_bytes, st)")))
                return rc;
            MixedGsArgs g;
            std::memset(&g, 0, sizeof g);
            g.in = (const cx<float>*)parts;
            g.in_pitch = (unsigned)part_row_stride;
            g.rowmap = row_sources;
            g.ncols = m;
            for (int k = 0; k < nchunks; k++) {
                g.c_base[k] = cz.c_base[k];
                g.c_fs[k] = cz.c_fs[k];
            }
            MixedArgs<float> X = mixed_args<float>(*mx, yN);
            X.scratch = (cx<float>*)lease.p;
            X.s_row = 1; X.s_y = m; X.s_j = M * m; X.s_b = (long long)yN * m;
            rc = radix_launch_status(launch_mixed_gs_pass(Q, g, X, nf, st), Q, "gather-sum pass");
            for (int j = 0; j < Q && !rc; j++) {
                ColPassArgs cs = c;  // the store side of the primitive; plain load from the pass's scratch
                cs.in = X.scratch + (long long)j * X.s_j;
                cs.in_pitch = (unsigned)m;
                cs.in_bs = X.s_b; cs.in_bdiv = 0; cs.in_bs_hi = 0;
                cs.ld_rowmap = nullptr; cs.gs = 0;
                rc = col_transform(h, logM, cs, cz, m, nf, st, part.sub(lease.p), part.sub_bytes, Q, j, yN);
            }
            rc = lease.release(rc);
        }
        if (rc == -1) return fail(SWIFTLY_ERR_UNSUPPORTED, "accumulate_facet_columns: padded facet size %d not supported", yN);
        if (rc) return rc;
    }
    if (touched) {
        hipLaunchKernelGGL(mark_columns_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, touched,
                           m, win.rot, win.base, yN, (int)band_start, (int)band_len);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int swiftly_hip_band_zero_untouched(swiftly_hip_t* h, int dtype, void* bands, int64_t rows, int64_t band_row_stride,
                                    int64_t band_len, const unsigned char* touched, void* stream) {
    if (!h || !bands || !touched) return fail(SWIFTLY_ERR_PARAM, "null argument");
    DeviceGuard device_guard_(h->device);
    CHECK_DTYPE();
    if (rows <= 0 || band_len <= 0) return 0;
    dim3 grid((unsigned)((band_len + 63) / 64), (unsigned)std::min<int64_t>(rows, 1024));
    if (dtype == SWIFTLY_C128)
        hipLaunchKernelGGL(zero_untouched_kernel<double>, grid, dim3(64), 0, (hipStream_t)stream, (cx<double>*)bands, touched,
                           (long long)rows, (long long)band_row_stride, (int)band_len);
    else
        hipLaunchKernelGGL(zero_untouched_kernel<float>, grid, dim3(64), 0, (hipStream_t)stream, (cx<float>*)bands, touched,
                           (long long)rows, (long long)band_row_stride, (int)band_len);
    HIP_TRY(hipGetLastError());
    return 0;
}


}  // extern "C"
