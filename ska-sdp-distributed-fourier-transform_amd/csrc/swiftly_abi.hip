// C ABI of libswiftly_hip.so (see include/swiftly_hip.h).
//
// Each primitive of the reference (fourier_transform/core.py:189-484) is
// expressed as ONE launch of the mapped row FFT kernel (swiftly_rows.h) or of
// the modular gather/scatter kernel below:
//
//   primitive             N    load map (q = (ci+a) mod N)          store map (d = (ci+a) mod N)        dir  scale
//   prepare_facet         yN   a=-(off+yN/2-yB//2) len=yB win=1/pswf  identity                          inv  1/yN
//   add_to_subgrid        m    identity                             a=-s' len=m c=xM/2-m/2+s' mod xM Fn  fwd  1   (+=)
//   finish_subgrid        xM   identity                             a=-(xM/2-xA//2+off) len=xA [mask]   inv  1/xM
//   prepare_subgrid       xM   a=-(xM/2-xA//2+off) len=xA           identity                            fwd  1
//   extract_from_subgrid  m    a=-s' len=m c=xM/2-m/2+s' mod xM Fn  identity                            inv  1/m
//   finish_facet          yN   identity                             a=-(yN/2-yB//2+off) len=yB 1/pswf   fwd  1
//   extract_from_facet / add_to_facet: pure modular gather / scatter-add (no FFT)
//
// with s = floor(subgrid_off*yN/N), s' = floor(facet_off*xM/N), all arrays
// centred (origin at index n//2).
#include <hip/hip_runtime.h>
#include "swiftly_abi_internal.h"

// ---------------------------------------------------------------------------
static thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int launch_status(int e, const char* what, const char* negative) {
    if (!e) return 0;
    const char* text = (e < 0 && negative) ? negative : hipGetErrorString((hipError_t)e);
    if (what) return fail(SWIFTLY_ERR_HIP, "kernel launch failed (%s): %s", what, text);
    return fail(SWIFTLY_ERR_HIP, "kernel launch failed: %s", text);
}
int radix_launch_status(int e, int Q, const char* pass) {
    if (!e) return 0;
    char what[48]; snprintf(what, sizeof what, "radix-%d %s", Q, pass);
    return launch_status(e, what);
}

template <typename T>
static int upload(swiftly_hip* h, T** dst, const std::vector<T>& v) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, v.size() * sizeof(T)));
    h->allocs.push_back(p);
    HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *dst = (T*)p;
    return 0;
}

static std::vector<cx<float>> host_twiddles_f(int logn) {
    const int n = 1 << logn;
    std::vector<cx<float>> t(n);
    for (int k = 0; k < n; k++) {
        // exact octant symmetry is not needed; evaluate in long double
        long double a = -2.0L * 3.14159265358979323846264338327950288L * k / n;
        t[k] = {(float)cosl(a), (float)sinl(a)};
    }
    return t;
}
// compact copy of the float table of length 2^logn for kernels with 2^logp points per lane (swiftly_fft.h)
static int make_compact_twiddles(swiftly_hip* h, int logn, int logp) {
    if (logn < 2 || logp < 1 || logn > kMaxLogNFloat + 1 || h->twc_f.count({logn, logp})) return 0;
    const std::vector<cx<float>> t = host_twiddles_f(logn);
    std::vector<cx<float>> c((size_t)compact_tw_entries(logn, logp));
    build_compact_twiddles(t.data(), logn, logp, c.data());
    cx<float>* d;
    if (int rc = upload(h, &d, c)) return rc;
    h->twc_f[{logn, logp}] = d;
    return 0;
}

static int make_twiddles(swiftly_hip* h, int logn) {
    if (logn < kMinLogN) return 0;
    const int n = 1 << logn;
    if (logn <= kMaxLogNFloat + 1 && !h->tw_f.count(logn)) {  // 2^16: only the band row kernel and the column passes use it
        const std::vector<cx<float>> t = host_twiddles_f(logn);
        cx<float>* d;
        if (int rc = upload(h, &d, t)) return rc;
        h->tw_f[logn] = d;
    }
    // (double tables up to 2^16: the float64-arithmetic column passes need the four-step twiddles of the whole length)
    if (logn <= kMaxLogNFloat + 1 && !h->tw_d.count(logn)) {
        std::vector<cx<double>> t(n);
        for (int k = 0; k < n; k++) {
            long double a = -2.0L * 3.14159265358979323846264338327950288L * k / n;
            t[k] = {(double)cosl(a), (double)sinl(a)};
        }
        cx<double>* d;
        if (int rc = upload(h, &d, t)) return rc;
        h->tw_d[logn] = d;
    }
    return 0;
}

// Bluestein tables for length n: chirp c[j] = exp(i pi j^2 / n) and the spectrum of the wrapped chirp filter of
// length L = 2^logL >= 2n - 1 (host radix-2 FFT in double precision; exact angles through j^2 mod 2n).
static int make_bluestein(swiftly_hip* h, int64_t n) {
    if (n <= 0 || ilog2_exact(n) >= 0 || h->blu.count(n)) return 0;
    int logL = 0;
    while ((int64_t(1) << logL) < 2 * n - 1) logL++;
    if (logL > kMaxLogNFloat + 1) return 0;  // no kernel for the convolution length: stays unsupported
    const int64_t L = int64_t(1) << logL;
    const long double pi = 3.14159265358979323846264338327950288L;
    std::vector<std::complex<double>> c(n), f(L, 0.0);
    for (int64_t j = 0; j < n; j++) {
        const long double ang = pi * (long double)((j * j) % (2 * n)) / (long double)n;
        c[j] = {(double)cosl(ang), (double)sinl(ang)};
    }
    f[0] = c[0];
    for (int64_t j = 1; j < n; j++) f[j] = f[L - j] = c[j];
    // iterative radix-2 decimation-in-time FFT (forward, exp(-2 pi i jk / L))
    for (int64_t i = 1, j = 0; i < L; i++) {
        int64_t bit = L >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(f[i], f[j]);
    }
    for (int64_t len = 2; len <= L; len <<= 1) {
        for (int64_t i = 0; i < L; i += len)
            for (int64_t k = 0; k < len / 2; k++) {
                const long double ang = -2.0L * pi * (long double)k / (long double)len;
                const std::complex<double> w((double)cosl(ang), (double)sinl(ang));
                const std::complex<double> u = f[i + k], v = f[i + k + len / 2] * w;
                f[i + k] = u + v;
                f[i + k + len / 2] = u - v;
            }
    }
    swiftly_hip::Blu t;
    t.logL = logL;
    std::vector<cx<float>> cf(n), sf(L);
    std::vector<cx<double>> cd(n), sd(L);
    for (int64_t j = 0; j < n; j++) {
        cd[j] = {c[j].real(), c[j].imag()};
        cf[j] = {(float)c[j].real(), (float)c[j].imag()};
    }
    for (int64_t j = 0; j < L; j++) {
        sd[j] = {f[j].real(), f[j].imag()};
        sf[j] = {(float)f[j].real(), (float)f[j].imag()};
    }
    int rc = upload(h, &t.chirp_f, cf);
    if (!rc) rc = upload(h, &t.spec_f, sf);
    if (!rc && logL <= kMaxLogNDouble) {
        rc = upload(h, &t.chirp_d, cd);
        if (!rc) rc = upload(h, &t.spec_d, sd);
    }
    if (!rc) rc = make_twiddles(h, logL);
    if (!rc && logL == 16) rc = make_twiddles(h, 15);
    if (!rc && logL == 15) {
        rc = make_twiddles(h, 14);
        if (!rc) rc = make_twiddles(h, 13);
    }
    if (!rc) h->blu[n] = t;
    return rc;
}

// Tables for a length n = Q * 2^k (swiftly_mixed.h): the full-length twiddles and the power-of-two tables of the
// sub-transforms (with the halves their strided four-step form uses).
static int make_mixed(swiftly_hip* h, int64_t n) {
    int Q = 0, logM = 0;
    if (!mixed_factor(n, &Q, &logM) || h->mixed.count(n)) return 0;
    if (logM > kMaxLogNFloat) return 0;  // stays with the fallbacks
    swiftly_hip::Mixed t;
    t.Q = Q;
    t.logM = logM;
    std::vector<cx<float>> tf((size_t)n);
    std::vector<cx<double>> td((size_t)n);
    for (int64_t k = 0; k < n; k++) {
        const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)n;
        td[(size_t)k] = {(double)cosl(a), (double)sinl(a)};
        tf[(size_t)k] = {(float)cosl(a), (float)sinl(a)};
    }
    int rc = upload(h, &t.tw_f, tf);
    if (!rc && logM <= kMaxLogNDouble) rc = upload(h, &t.tw_d, td);
    if (!rc) rc = make_twiddles(h, logM);
    if (!rc && logM >= kTwoPassMinLog) rc = make_twiddles(h, logM / 2);
    if (!rc && logM >= kTwoPassMinLog) rc = make_twiddles(h, logM - logM / 2);
    if (!rc && logM == 15) rc = make_twiddles(h, 14);
    if (!rc && logM == 15) rc = make_twiddles(h, 13);
    if (!rc) h->mixed[n] = t;
    return rc;
}

// Kernel attributes (max dynamic LDS; the table of swiftly_launch.h) and the memory-pool release threshold are per DEVICE
// state: they are set once for every device a handle is created on, under a lock (handles may be created from several
// host threads).
static std::mutex g_init_mutex;
static std::vector<char> g_device_inited;


extern "C" {

const char* swiftly_hip_last_error(void) { return g_err.c_str(); }
int swiftly_hip_version(void) { return 100; }
int swiftly_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int swiftly_hip_create(swiftly_hip_t** out, int64_t N, int64_t yN, int64_t xM, double W, const double* pswf,
                       int device) {
    if (!out || !pswf) return fail(SWIFTLY_ERR_PARAM, "null argument");
    *out = nullptr;
    if (const std::string bad = check_sizes(N, yN, xM); !bad.empty()) return fail(SWIFTLY_ERR_PARAM, "%s", bad.c_str());
    int ndev = swiftly_hip_device_count();
    if (ndev <= 0) return fail(SWIFTLY_ERR_HIP, "no HIP device visible: the SwiFTly HIP backend has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(SWIFTLY_ERR_PARAM, "invalid device %d", device);
    DeviceGuard guard(device);
    if (guard.rc) return fail(SWIFTLY_ERR_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString((hipError_t)guard.rc));
    std::lock_guard<std::mutex> init_lock(g_init_mutex);
    if ((int)g_device_inited.size() < ndev) g_device_inited.resize(ndev, 0);
    if (!g_device_inited[device]) {
        int lds = 0;
        if (int rc = set_registered_kernel_attributes(&lds))
            return fail(SWIFTLY_ERR_HIP, "kernel attribute setup failed (%d bytes of LDS): %d", lds, rc);
        // keep freed scratch (the four-step intermediate, up to yN*yB*8 bytes) in the stream-ordered pool instead of
        // returning it to the driver at every synchronisation point
        hipMemPool_t pool;
        if (hipDeviceGetDefaultMemPool(&pool, device) == hipSuccess) {
            uint64_t keep = UINT64_MAX;
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
        }
        (void)hipGetLastError();
        g_device_inited[device] = 1;
    }
    swiftly_hip* h = new (std::nothrow) swiftly_hip();
    if (!h) return fail(SWIFTLY_ERR_HIP, "out of host memory");
    static_cast<Sizes&>(*h) = make_sizes(N, yN, xM);
    h->W = W;
    h->device = device;
    if (hipDeviceGetAttribute(&h->cu_count, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h->cu_count <= 0) {
        delete h;
        return fail(SWIFTLY_ERR_HIP, "cannot query the compute unit count of device %d", device);
    }
    if (const char* e = getenv("SWIFTLY_COL_F64")) h->col_f64 = atoi(e) != 0;
    if (const char* e = getenv("SWIFTLY_COL_F64_STAGES")) h->col_f64_stages = atoi(e) & 7;
    // windows: 1/pswf (Fb, core.py:104-108) and Fn (core.py:110-117)
    std::vector<double> ip(yN);
    std::vector<float> ipf(yN);
    for (int64_t k = 0; k < yN; k++) {
        ip[k] = (k == 0 || pswf[k] == 0.0) ? 0.0 : 1.0 / pswf[k];
        ipf[k] = (float)ip[k];
    }
    const int64_t step = N / xM;
    std::vector<double> fn;
    for (int64_t k = (yN / 2) % step; k < yN; k += step) fn.push_back(pswf[k]);
    if ((int64_t)fn.size() != h->m) {
        delete h;
        return fail(SWIFTLY_ERR_PARAM, "internal: Fn length %zu != contribution size %lld", fn.size(), (long long)(xM * yN / N));
    }
    std::vector<float> fnf(fn.begin(), fn.end());
    int rc = 0;
    if (!rc) rc = upload(h, &h->invp_d, ip);
    if (!rc) rc = upload(h, &h->invp_f, ipf);
    if (!rc) rc = upload(h, &h->fn_d, fn);
    if (!rc) rc = upload(h, &h->fn_f, fnf);
    for (int l : {h->log_yN, h->log_xM, h->log_m})
        if (!rc && l >= 0) {
            rc = make_twiddles(h, l);
            if (!rc && l >= kTwoPassMinLog) rc = make_twiddles(h, l / 2);
            if (!rc && l >= kTwoPassMinLog) rc = make_twiddles(h, l - l / 2);
            if (!rc && l == 15) rc = make_twiddles(h, 14);  // multi-workgroup row kernels
            if (!rc && l == 15) rc = make_twiddles(h, 13);
            if (!rc && (l == 16 || l == 14)) rc = make_twiddles(h, l - 1);  // band row kernel halves
        }
    // compact copies for the contiguous-axis kernels whose lanes gather table values (swiftly_fft.h): the forward K1 / backward
    // finish of 32768-point rows (2 x 16384 points, 32 per lane) and the facet kernels of the subgrid side (64 lanes per transform)
    if (!rc && h->log_yN == 15) {
        rc = make_compact_twiddles(h, 14, 5);
        if (!rc) h->win4.twc = compact_twiddles(h, 14, 5);
    }
    // ... and of the 32768-point table for the half-length forms of 65536-point rows (RowRealGeo64k / RowC2RGeo64k)
    if (!rc && h->log_yN == 16) rc = make_compact_twiddles(h, 15, 5);
    if (!rc && sum_finish_supported(h->log_m, h->log_xM)) {
        rc = make_compact_twiddles(h, h->log_m, h->log_m - 6);
        if (!rc) rc = make_compact_twiddles(h, h->log_xM, h->log_xM - (h->log_xM >= 12 ? 8 : 6));
    }
    for (int64_t len : {yN, xM, h->m})
        if (!rc) rc = make_bluestein(h, len);
    for (int64_t len : {yN, xM, h->m})
        if (!rc) rc = make_mixed(h, len);
    if (rc) {
        swiftly_hip_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

void swiftly_hip_destroy(swiftly_hip_t* h) {
    if (!h) return;
    DeviceGuard guard(h->device);
    for (hipStream_t st : h->chunk_st)
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
    for (void* p : h->allocs) (void)hipFree(p);
    h->win4.clear();
    delete h;
}


int64_t swiftly_hip_contribution_size(const swiftly_hip_t* h) { return h ? h->m : -1; }

}  // extern "C"

// ---------------------------------------------------------------------------
// Batch descriptor shared by all *_batch entry points: nbatch independent
// problems of identical shape at in + b*in_bs / out + b*out_bs.  `offs`
// (host array, may be null) gives a per-item offset, otherwise `off` applies
// to every item.
struct Batch {
    int64_t n = 1, in_bs = 0, out_bs = 0;
    const int64_t* offs = nullptr;
    int64_t mask_bs = 0;
    int64_t off_of(int64_t b, int64_t off) const { return offs ? offs[b] : off; }
};

// modular gather / scatter-add (extract_from_facet / add_to_facet)
//   j < m ; i = (j - s) mod m ; big = (base + i + s) mod yN
//   gather : out[row, j]   = in[row, big]
//   scatter: out[row, big] += in[row, j]
struct ModTab {
    int s_m[kMaxBatch], base_s[kMaxBatch];
};

template <typename R, bool SCATTER>
__global__ void modcopy_kernel(const cx<R>* __restrict__ in, cx<R>* __restrict__ out, long long rows, int m, int yN,
                               const ModTab tab, long long in_rs, long long in_cs, long long out_rs,
                               long long out_cs, long long in_bs, long long out_bs, int rowfast) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= rows * m) return;
    const int b = blockIdx.y;
    in += (long long)b * in_bs;
    out += (long long)b * out_bs;
    long long row;
    int j;
    if (rowfast) {
        row = gid % rows;
        j = (int)(gid / rows);
    } else {
        j = (int)(gid % m);
        row = gid / m;
    }
    int i = j - tab.s_m[b];
    if (i < 0) i += m;
    int big = tab.base_s[b] + i;  // base_s = (yN/2 - m/2 + s) mod yN
    if (big >= yN) big -= yN;
    if (SCATTER) {
        cx<R> v = in[row * in_rs + (long long)j * in_cs];
        cx<R>* p = out + row * out_rs + (long long)big * out_cs;
        cx<R> o = *p;
        o.x += v.x;
        o.y += v.y;
        *p = o;
    } else {
        out[row * out_rs + (long long)j * out_cs] = in[row * in_rs + (long long)big * in_cs];
    }
}

template <typename R, bool SCATTER>
static int run_modcopy(swiftly_hip* h, const void* in, int64_t rows, int64_t in_rs, int64_t in_cs, void* out,
                       int64_t out_rs, int64_t out_cs, int64_t subgrid_off, const Batch& bt, hipStream_t st) {
    if (rows <= 0 || bt.n <= 0) return 0;
    const int m = (int)h->m, yN = (int)h->yN;
    const long long total = rows * (long long)m;
    const int rowfast = (in_rs == 1 && in_cs != 1) ? 1 : 0;
    for (int64_t b0 = 0; b0 < bt.n; b0 += kMaxBatch) {
        const int nb = (int)std::min<int64_t>(kMaxBatch, bt.n - b0);
        ModTab tab;
        for (int b = 0; b < nb; b++) {
            const Window w = window_of(*h, bt.off_of(b0 + b, subgrid_off));
            tab.s_m[b] = pmod(w.s, m);
            tab.base_s[b] = w.base;
        }
        dim3 grid((unsigned)((total + 255) / 256), nb);
        hipLaunchKernelGGL((modcopy_kernel<R, SCATTER>), grid, dim3(256), 0, st,
                           (const cx<R>*)in + b0 * bt.in_bs, (cx<R>*)out + b0 * bt.out_bs, (long long)rows, m, yN, tab,
                           (long long)in_rs, (long long)in_cs, (long long)out_rs, (long long)out_cs,
                           (long long)bt.in_bs, (long long)bt.out_bs, rowfast);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// ---------------------------------------------------------------------------
template <typename R>
static int launch_checked(int logn, const RowsArgs<R>& a, const OffTab& tab, hipStream_t st) {
    return launch_status(launch_fft_rows(logn, a, tab, st));
}

// Route ColPass (complex64 transforms along the strided axis of row-major arrays, columns contiguous: swiftly_colpass.h):
// the argument block of the call and, in `cz`, its per-item tables.
static ColPassArgs col_pass_of(int logn, const RowsArgs<float>& a, const OffTab& tab, ColZ& cz) {
    const int nb = a.nbatch > 0 ? a.nbatch : 1;
    ColPassArgs c = col_pass_args(Map{a.ld.a, a.ld.len, a.ld.c, a.ld.mod}, Map{a.st.a, a.st.len, a.st.c, a.st.mod});
    c.ncols = a.nrows;
    c.full_logn = logn;
    c.in = a.in; c.out = a.out;
    c.in_pitch = a.in_cs; c.out_pitch = a.out_cs;
    c.in_bs = a.in_bs;
    c.out_bs = a.out_bs;
    c.ld_win = a.ld.win; c.ld_win2 = a.ld.win2;
    c.st_win = a.st.win; c.st_win2 = a.st.win2; c.st_win_bs = a.st_win_bs;
    c.st_rowmap = a.st_rowmap;
    c.col_win = a.row_win;
    c.scale = a.scale;
    c.conj_ld = a.conj_ld; c.conj_st = a.conj_st; c.accumulate = a.accumulate;
    // per-item map offsets (OffTab) -> per-subgrid tables of the column pass (batch item z = b)
    cz = plain_colz();
    if (tab.use) {
        static_assert(kMaxBatch <= kColZB, "per-item tables");
        cz.nb = nb;
        if (tab.use & 3) {
            cz.flags |= kZLoadB;
            for (int b = 0; b < nb; b++) {
                cz.b_lda[b] = (tab.use & 1) ? tab.ld_a[b] : a.ld.a;
                cz.b_ldc[b] = (tab.use & 2) ? tab.ld_c[b] : a.ld.c;
            }
        }
        if (tab.use & 4) {
            cz.flags |= kZStoreAB;
            for (int b = 0; b < nb; b++) cz.b_sta[b] = tab.st_a[b];
        }
    }
    return c;
}


__global__ void mul_windows_kernel(float* __restrict__ out, const float* __restrict__ a, const float* __restrict__ b, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i] * b[i];
}

// The mapped-store form of the band row kernel takes ONE output window: fold st_win * st_win2 into a
// stream-ordered temporary (freed by the caller with hipFreeAsync after the launch is queued).
static int single_store_window(RowPassArgs& r, hipStream_t st, void** tmp) {
    *tmp = nullptr;
    if (r.st_win && r.st_win2) {
        HIP_TRY(hipMallocAsync(tmp, (size_t)r.st_len * sizeof(float), st));
        hipLaunchKernelGGL(mul_windows_kernel, dim3((unsigned)((r.st_len + 255) / 256)), dim3(256), 0, st, (float*)*tmp,
                           r.st_win, r.st_win2, r.st_len);
        HIP_TRY(hipGetLastError());
        r.st_win = (const float*)*tmp;
    } else if (r.st_win2) {
        r.st_win = r.st_win2;
    }
    r.st_win2 = nullptr;
    return 0;
}

// Routes Lean, Split32k and the three band routes (long complex64 transforms along the contiguous axis, one or two
// workgroups per row: swiftly_rowpass.h): the argument block of the call.  (These kernels take no st_rowmap, no second load
// window and no per-item window: choose_row_route sends such calls elsewhere.)
static RowPassArgs row_pass_of(const RowsArgs<float>& a) {
    RowPassArgs r;
    std::memset(&r, 0, sizeof r);
    r.in = a.in; r.out = a.out;
    r.in_pitch = a.in_rs; r.out_pitch = a.out_rs;
    r.nrows = a.nrows;
    r.rm_mod = a.rm_mod; r.rm_inner = a.rm_inner; r.rm_outer = a.rm_outer; r.rm_full = a.rm_full;
    r.in_rowmap = a.in_rowmap;
    r.in_real = a.real_in;
    r.out_real = a.real_out;
    r.row_win = a.row_win;
    r.ld_a = a.ld.a; r.ld_len = a.ld.len; r.ld_c = a.ld.c; r.ld_mod = a.ld.mod; r.ld_win = a.ld.win;
    r.st_a = a.st.a; r.st_len = a.st.len; r.st_c = a.st.c; r.st_mod = a.st.mod; r.st_win = a.st.win; r.st_win2 = a.st.win2;
    r.tw = a.tw;
    r.scale = a.scale; r.conj_ld = a.conj_ld; r.conj_st = a.conj_st; r.accumulate = a.accumulate;
    return r;
}
// Routes Band32kPlain, Band32kMapped and Band64k: the two-workgroup band kernel at 32768 / 65536 points, for the load map
// of a prepare_* primitive or -- mapped store, one window -- the store map of a finish_* primitive.
static int launch_band_route(swiftly_hip* h, const RowRoute& route, int logn, RowPassArgs r, hipStream_t st) {
    void* tmp = nullptr;
    if (route.single_store_window) {
        r.band_len = -1;  // selects the mapped-store variant
        if (int rc = single_store_window(r, st, &tmp)) return rc;
    }
    const int e = launch_row_pass_band_n(logn, r, twiddles<float>(h, logn - 1), r.tw, st,
                                         route.kind == kRouteBand32kMapped ? &h->win4 : nullptr);
    if (tmp) (void)hipFreeAsync(tmp, st);
    return launch_status(e);
}


// complex128 transform of 2^14 / 2^15 points along the CONTIGUOUS axis (swiftly_rowslong.h): pass A (mapped load, n1 =
// 128 points per column, lanes along y2, twiddle on store) into a stream-ordered scratch [rows][k1][y2], pass B =
// fft_rows_kernel at log2(n2) with raw load from the scratch and the primitive's store map (plain index k1 + n1*k2).  Rows
// run in chunks whose scratch stays under kLongChunkBytes (a whole 128k[1]-n32k-1k facet would need 14 GB), all chunks
// reuse one allocation.  SWIFTLY_LONG_ROWS_CHUNK_MB (read per call) lowers the bound (tests: many chunk boundaries).
static const size_t kLongChunkBytes = size_t(1) << 30;
static int run_rows_long(swiftly_hip* h, int logn, RowsArgs<double>& a, const OffTab& tab, hipStream_t st) {
    const int l1 = kLongLogN1, l2 = logn - l1;
    const int n1 = 1 << l1, n2 = 1 << l2;
    const long long n = 1ll << logn;
    if (n2 % LongAGeo::RB) return fail(SWIFTLY_ERR_UNSUPPORTED, "internal: no pass A tiling for 2^%d points", logn);
    const cx<double>* tw_full = twiddles<double>(h, logn);
    const cx<double>* tw1 = twiddles<double>(h, l1);
    const cx<double>* tw2 = twiddles<double>(h, l2);
    if (!tw_full || !tw1 || !tw2) return fail(SWIFTLY_ERR_HIP, "internal: missing twiddle tables for 2^%d = 2^%d * 2^%d", logn, l1, l2);
    const int nb = a.nbatch > 0 ? a.nbatch : 1;
    size_t budget = kLongChunkBytes;
    if (const char* e = getenv("SWIFTLY_LONG_ROWS_CHUNK_MB")) {
        const long long mb = atoll(e);
        if (mb > 0) budget = std::min(budget, (size_t)mb << 20);
    }
    const size_t row_bytes = (size_t)nb * (size_t)n * sizeof(cx<double>);
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)a.nrows, budget / row_bytes));
    void* scratch = nullptr;
    HIP_TRY(hipMallocAsync(&scratch, (size_t)chunk * row_bytes, st));
    RowsArgs<double> A = a;  // (real_in, float64 rows, is pass A's alone: pass B reads the complex scratch)
    A.real_out = 0;
    A.tw = tw1;
    A.full_logn = logn;
    A.full_n = 0;
    LongArgs<double> L;
    L.scratch = (cx<double>*)scratch;
    L.s_bs = (long long)chunk * n;
    L.log_n2 = l2;
    L.tw_full = tw_full;
    // pass B: rows of the chunk x outer index k1 = n1 sub-transforms of length n2 per row; the n1 workgroups of a row block
    // are enumerated next to each other on one XCD (outer_group), whose L2 merges their interleaved output elements
    RowsArgs<double> B = a;  // (real_out, float64 rows, is pass B's alone: pass A writes the complex scratch)
    B.real_in = 0;
    B.tw = tw2;
    B.in = (const cx<double>*)scratch;
    B.raw_ld = 1;
    B.conj_ld = 0;  // applied by pass A
    B.in_rs = n;
    B.in_cs = 1;
    B.in_os = n2;
    B.in_bs = (long long)chunk * n;
    B.rm_mod = 0;
    B.in_rowmap = nullptr;
    B.outer = n1;
    B.outer_group = 1;
    B.full_logn = logn;
    B.full_n = 0;
    B.ld_mul = 1;
    B.ld_addmul = 0;
    B.st_mul = n1;
    B.st_addmul = 1;
    B.st_add0 = 0;
    B.tw_full = nullptr;
    B.tw_on_store = 0;
    B.raw_st = 0;
    int rc = 0;
    for (int row0 = 0; row0 < a.nrows && !rc; row0 += chunk) {
        const int rows = std::min(chunk, a.nrows - row0);
        L.row0 = row0;
        L.nrows = rows;
        rc = launch_status(launch_fft_long_a(A, tab, L, st), "long-row pass A");
        if (rc) break;
        B.nrows = rows;
        // (out_rs counts reals when the rows are float64)
        B.out = a.real_out ? (cx<double>*)((double*)a.out + (long long)row0 * a.out_rs) : a.out + (long long)row0 * a.out_rs;
        B.row_win = a.row_win ? a.row_win + row0 : nullptr;
        rc = launch_checked(l2, B, tab, st);
    }
    hipError_t e = hipFreeAsync(scratch, st);
    if (!rc && e != hipSuccess) return fail(SWIFTLY_ERR_HIP, "hipFreeAsync: %s", hipGetErrorString(e));
    return rc;
}

// The four-step of a transform of length >= 2^kTwoPassMinLog along a strided axis (route FourStep), through a
// stream-ordered scratch.  Sub-transform form: see run_rows_chunk.
template <typename R>
static int run_rows_four_step(swiftly_hip* h, int logn, RowsArgs<R>& a, const OffTab& tab, hipStream_t st, int qmul, int qadd) {
    const bool sub = qmul > 1;
    // ---- four-step: N = n1 * n2, input index y = y1*n2 + y2, output index k = k1 + n1*k2
    //   pass A (length n1 over y1, one per y2): scratch[k1*n2 + y2] = W_N^(y2 k1) * sum_y1 x[y1 n2 + y2] W_n1^(y1 k1)
    //   pass B (length n2 over y2, one per k1): X[k1 + n1 k2]       = sum_y2 scratch[k1*n2 + y2] W_n2^(y2 k2)
    const uint64_t n = uint64_t(1) << logn;
    const int l1 = logn / 2, l2 = logn - l1;
    const int n1 = 1 << l1, n2 = 1 << l2;
    const cx<R>* tw1 = twiddles<R>(h, l1);
    const cx<R>* tw2 = twiddles<R>(h, l2);
    if (!tw1 || !tw2) return fail(SWIFTLY_ERR_HIP, "internal: missing twiddle tables for the two-pass transform");
    const long long W = a.nrows;  // scratch row width (rows of the op are contiguous in memory)
    if (n * (uint64_t)W >= (uint64_t(1) << 32))
        return fail(SWIFTLY_ERR_PARAM, "two-pass scratch exceeds 2^32 elements; split the call by columns");
    const int nb = a.nbatch > 0 ? a.nbatch : 1;
    void* scratch = nullptr;
    HIP_TRY(hipMallocAsync(&scratch, (size_t)nb * n * (size_t)W * sizeof(cx<R>), st));
    RowsArgs<R> A = a;
    A.tw = tw1;
    A.tw_full = a.tw;
    A.tw_on_store = 1;
    A.outer = n2;
    A.ld_mul = n2;
    A.ld_addmul = 1;
    if (sub) {  // raw input: element y1*n2 + y2 of the sub-transform, outer index y2
        if ((uint64_t)a.in_cs * n >= (uint64_t(1) << 32)) {
            (void)hipFreeAsync(scratch, st);
            return fail(SWIFTLY_ERR_PARAM, "transform length * column stride must be < 2^32");
        }
        A.in_cs = a.in_cs * (unsigned)n2;
        A.in_os = (long long)a.in_cs;
    }
    A.st_mul = 1;
    A.st_add0 = 0;
    A.raw_st = 1;
    A.out = (cx<R>*)scratch;
    A.out_rs = 1;
    A.out_cs = (unsigned)(n2 * W);
    A.out_os = W;
    A.out_bs = (long long)(n * W);
    A.conj_st = 0;
    A.scale = (R)1;
    A.accumulate = 0;
    A.st_rowmap = nullptr;  // output-side maps / windows belong to pass B
    A.row_win = nullptr;
    int rc = launch_checked(l1, A, tab, st);
    if (!rc) {
        RowsArgs<R> B = a;
        B.tw = tw2;
        B.in = (const cx<R>*)scratch;
        B.raw_ld = 1;
        B.in_rs = 1;
        B.in_cs = (unsigned)W;
        B.in_os = (long long)n2 * W;
        B.in_bs = (long long)(n * W);
        B.rm_mod = 0;
        B.in_rowmap = nullptr;  // the scratch is indexed by plain (k1, y2), never through the compaction map
        B.outer = n1;
        B.st_mul = qmul * n1;
        B.st_addmul = qmul;
        B.st_add0 = qadd;
        B.conj_ld = 0;
        rc = launch_checked(l2, B, tab, st);
    }
    hipError_t e = hipFreeAsync(scratch, st);
    if (!rc && e != hipSuccess) return fail(SWIFTLY_ERR_HIP, "hipFreeAsync: %s", hipGetErrorString(e));
    return rc;
}

template <typename R>
static int run_rows_chunk(swiftly_hip* h, int64_t nlen, int logn, RowsArgs<R>& a, const OffTab& tab, hipStream_t st, int qmul = 1,
                          int qadd = 0);

// Transform length n that is NOT a power of two: Bluestein through two power-of-two transforms of length
// L >= 2n - 1 on a stream-ordered work buffer (swiftly_bluestein.h).
template <typename R>
static int run_rows_bluestein(swiftly_hip* h, int64_t n, RowsArgs<R>& a, const OffTab& tab, hipStream_t st) {
    auto it = h->blu.find(n);
    const cx<R>* chirp = nullptr;
    const cx<R>* spec = nullptr;
    int logL = 0;
    if (it != h->blu.end()) {
        logL = it->second.logL;
        if constexpr (sizeof(R) == 4) {
            chirp = it->second.chirp_f;
            spec = it->second.spec_f;
        } else {
            chirp = it->second.chirp_d;
            spec = it->second.spec_d;
        }
    }
    if (!chirp || !spec) return fail(SWIFTLY_ERR_HIP, "internal: missing Bluestein tables");  // (the route has them)
    const int64_t L = int64_t(1) << logL;
    const int nb = a.nbatch > 0 ? a.nbatch : 1;
    const int64_t rows_total = (int64_t)nb * a.nrows;
    if (rows_total > 0x7fffffff) return fail(SWIFTLY_ERR_PARAM, "too many rows");
    void *w1 = nullptr, *w2 = nullptr;
    const size_t bytes = (size_t)rows_total * (size_t)L * sizeof(cx<R>);
    HIP_TRY(hipMallocAsync(&w1, bytes, st));
    hipError_t e2 = hipMallocAsync(&w2, bytes, st);
    if (e2 != hipSuccess) {
        (void)hipFreeAsync(w1, st);
        return fail(SWIFTLY_ERR_HIP, "hipMallocAsync(Bluestein work): %s", hipGetErrorString(e2));
    }
    BluArgs<R> B;
    B.a = a;
    B.n = (int)n;
    B.L = (int)L;
    B.chirp = chirp;
    B.work = (cx<R>*)w1;
    const unsigned gy = (unsigned)std::min<int64_t>(a.nrows, 65535);
    hipLaunchKernelGGL((blu_load_kernel<R>), dim3((unsigned)((L + 255) / 256), gy, (unsigned)nb), dim3(256), 0, st, B, tab);
    int rc = launch_status((int)hipGetLastError(), "blu_load");
    RowsArgs<R> f;
    OffTab none;
    none.use = 0;
    auto fft_L = [&](const void* src, void* dst, bool inverse) -> int {
        std::memset(&f, 0, sizeof f);
        f.in = (const cx<R>*)src;
        f.out = (cx<R>*)dst;
        f.in_rs = f.out_rs = L;
        f.in_cs = f.out_cs = 1;
        f.nrows = (int)rows_total;
        f.ld = axis_map<R>(whole(L));
        f.st = axis_map<R>(whole(L));
        f.scale = inverse ? (R)(1.0 / (double)L) : (R)1;
        f.conj_ld = f.conj_st = inverse ? 1 : 0;
        f.nbatch = 1;
        return run_rows_chunk(h, L, logL, f, none, st);
    };
    if (!rc) rc = fft_L(w1, w2, false);
    if (!rc) {
        const unsigned gy2 = (unsigned)std::min<int64_t>(rows_total, 65535);
        hipLaunchKernelGGL((blu_mul_kernel<R>), dim3((unsigned)((L + 255) / 256), gy2), dim3(256), 0, st, (cx<R>*)w2, spec,
                           (long long)rows_total, (int)L);
        rc = launch_status((int)hipGetLastError(), "blu_mul");
    }
    if (!rc) rc = fft_L(w2, w1, true);
    if (!rc) {
        hipLaunchKernelGGL((blu_store_kernel<R>), dim3((unsigned)((n + 255) / 256), gy, (unsigned)nb), dim3(256), 0, st, B, tab);
        rc = launch_status((int)hipGetLastError(), "blu_store");
    }
    (void)hipFreeAsync(w1, st);
    (void)hipFreeAsync(w2, st);
    return rc;
}

// Transform length n = Q * 2^k (Q in {3, 5, 7, 9}): one radix-Q pass (swiftly_mixed.h) into a stream-ordered scratch,
// then the Q power-of-two sub-transforms with the store map of the primitive.
template <typename R>
static int run_rows_mixed(swiftly_hip* h, int64_t n, const swiftly_hip::Mixed& mx, RowsArgs<R>& a, const OffTab& tab,
                          hipStream_t st) {
    MixedArgs<R> X = mixed_args<R>(mx, n);
    if (!X.tw_n) return fail(SWIFTLY_ERR_UNSUPPORTED, "transform length %lld: no %s tables", (long long)n, sizeof(R) == 8 ? "complex128" : "complex64");
    const int Q = mx.Q, logM = mx.logM;
    const long long M = 1ll << logM;
    const int nb = a.nbatch > 0 ? a.nbatch : 1;
    const long long W = a.nrows;
    if ((uint64_t)n * (uint64_t)W >= (uint64_t(1) << 32))
        return fail(SWIFTLY_ERR_PARAM, "rows * transform length must be < 2^32 for lengths that are not a power of two; split the call");
    ScratchLease lease;  // (no workspace reaches the batch primitives: always a stream-ordered allocation)
    if (int rc = lease.acquire(nullptr, 0, (size_t)nb * (size_t)n * (size_t)W * sizeof(cx<R>), st,
                               "hipMallocAsync(&scratch, (size_t)nb * (size_t)n * (size_t)W * sizeof(cx<R>), st)"))
        return rc;
    X.scratch = (cx<R>*)lease.p;
    X.s_b = (long long)n * W;
    if (a.rowfast) {  // rows are the contiguous direction: scratch[b][j][y2][row]
        X.s_row = 1; X.s_y = W; X.s_j = M * W;
    } else {          // scratch[b][row][j][y2]
        X.s_row = n; X.s_j = M; X.s_y = 1;
    }
    RowsArgs<R> P = a;
    P.full_n = (int)n;
    int rc = radix_launch_status(launch_mixed_pass(Q, P, tab, X, nb, st), Q);
    // the Q sub-transforms: ONE launch with j as the kernel's outer index when the sub-transform is a single pass
    // (qadd = -1), one four-step pair per j along a strided axis
    const bool one_launch = !(a.rowfast && logM >= kTwoPassMinLog);
    for (int j = 0; j < (one_launch ? 1 : Q) && !rc; j++) {
        RowsArgs<R> B = a;
        B.in = X.scratch + (long long)j * X.s_j;
        B.in_rs = X.s_row;
        B.in_cs = (unsigned)X.s_y;
        B.in_bs = X.s_b;
        B.raw_ld = 1;
        B.conj_ld = 0;        // applied by the pass
        B.rm_mod = 0;
        B.in_rowmap = nullptr;
        B.full_n = (int)n;
        B.in_os = X.s_j;      // (used by the one-launch form only)
        rc = run_rows_chunk(h, M, logM, B, tab, st, Q, one_launch ? -1 : j);
    }
    return lease.release(rc);
}

// The radix-Q tables of a length as run_rows picks them, and the Bluestein tables of the handle (which exist only where
// their kernels do): facts of choose_row_route, and with row_length_supported the gate of swiftly_hip_supports_dtype.
static bool use_mixed(const swiftly_hip* h, int64_t n, bool dbl) {
    const char* no_mixed = getenv("SWIFTLY_NO_MIXED");  // read per call: Bluestein for every such length (A/B, tests)
    auto it = h->mixed.find(n);
    const bool have = it != h->mixed.end() && (dbl ? it->second.tw_d != nullptr : it->second.tw_f != nullptr);
    return have && !(no_mixed && atoi(no_mixed));
}
static bool have_bluestein(const swiftly_hip* h, int64_t n, bool dbl) {
    auto it = h->blu.find(n);
    return it != h->blu.end() && (dbl ? it->second.chirp_d != nullptr : it->second.chirp_f != nullptr);
}

// What choose_row_route (swiftly_rowroute.h) reads of a call: `a` after run_rows_chunk has set its transform fields.
template <typename R>
static RowCall row_call_of(const swiftly_hip* h, int64_t nlen, int logn, const RowsArgs<R>& a, const OffTab& tab, int qmul, int qadd) {
    constexpr bool dbl = sizeof(R) == 8;
    RowCall c;
    c.dbl = dbl; c.n = nlen; c.logn = logn;
    c.sub = qmul > 1; c.all_j = c.sub && qadd < 0;
    c.rowfast = a.rowfast != 0; c.in_rs1 = a.in_rs == 1; c.out_rs1 = a.out_rs == 1;
    c.nrows = a.nrows; c.in_cs = a.in_cs; c.out_cs = a.out_cs;
    c.tab_use = tab.use; c.nbatch = a.nbatch; c.rm = a.rm_mod > 0;
    c.in_rowmap = a.in_rowmap != nullptr; c.st_rowmap = a.st_rowmap != nullptr; c.row_win = a.row_win != nullptr;
    c.ld_win = a.ld.win != nullptr; c.ld_win2 = a.ld.win2 != nullptr;
    c.st_win = a.st.win != nullptr; c.st_win2 = a.st.win2 != nullptr; c.st_win_bs = a.st_win_bs != 0;
    c.ld_a = a.ld.a; c.ld_len = a.ld.len; c.ld_c = a.ld.c; c.ld_mod = a.ld.mod;
    c.st_a = a.st.a; c.st_len = a.st.len; c.st_c = a.st.c; c.st_mod = a.st.mod;
    c.accumulate = a.accumulate != 0; c.real_in = a.real_in != 0; c.real_out = a.real_out != 0;
    c.raw_ld = a.raw_ld != 0; c.raw_st = a.raw_st != 0;
    if (logn >= 0) {
        c.tw = a.tw != nullptr;
        if (!dbl) {
            c.tw_m1 = twiddles<float>(h, logn - 1); c.tw_m2 = twiddles<float>(h, logn - 2);
            c.tw_h1 = twiddles<float>(h, logn / 2); c.tw_h2 = twiddles<float>(h, logn - logn / 2);
        }
    } else {
        c.mixed = use_mixed(h, nlen, dbl);
        c.blu = have_bluestein(h, nlen, dbl);
    }
    return c;  // (c.col stays empty: the primitives ask nothing of the column passes)
}

// The one place where a refused route becomes a status and a text.
static int refuse_route(int why, bool dbl, int64_t n, int logn) {
    switch (why) {
    case kRowLength:
        return fail(SWIFTLY_ERR_UNSUPPORTED,
                    "transform length %lld is not supported by the HIP backend (power of two in [8, %d], or a length "
                    "whose Bluestein convolution or Q * 2^k sub-transform fits, for %s)",
                    (long long)n, 1 << max_log_rows(dbl), dbl ? "complex128: Bluestein and Q * 2^k up to 8192" : "complex64");
    case kRowStride:
        return fail(SWIFTLY_ERR_PARAM, "transform length * column stride must be < 2^32");
    case kRowNoConvolution:
        return fail(SWIFTLY_ERR_UNSUPPORTED,
                    "transform length %lld (not a power of two) needs a convolution of length >= %lld, beyond the %s kernels",
                    (long long)n, (long long)(2 * n - 1), dbl ? "complex128 (8192; Q * 2^k lengths up to Q * 8192)" : "complex64 (65536)");
    case kRowNoTable:
        return fail(SWIFTLY_ERR_HIP, "internal: missing twiddle table for 2^%d", logn);
    case kRowRealInDecomposed:
        return fail(SWIFTLY_ERR_UNSUPPORTED, "internal: %s input reaches a decomposed transform of 2^%d points", dbl ? "float64" : "real", logn);
    case kRowRealOutNoStore:
        return fail(SWIFTLY_ERR_UNSUPPORTED, "internal: %s output reaches a transform of 2^%d points without a real store",
                    dbl ? "float64" : "real", logn);
    case kRow64kLeanOnly:
        return fail(SWIFTLY_ERR_UNSUPPORTED, "transform length 65536 is only supported for complex64 prepare_* / finish_* "
                    "calls with unit stride along the transform axis or along a strided axis of contiguous rows");
    case kRowLongMappedLoadOnly:
        return fail(SWIFTLY_ERR_UNSUPPORTED, "complex128 transform length %d along the contiguous axis: only the "
                    "mapped-load form of the primitives is supported (no raw / sub-transform input)", 1 << logn);
    case kRowNoGenericInstance:
        return launch_status(-1);  // the status of a launcher without an instance
    }
    return fail(SWIFTLY_ERR_HIP, "internal: refused route %d", why);
}

// Launch the mapped row FFT for `a` (batch of a.nbatch <= kMaxBatch items with per-item offsets in `tab`) on the route
// choose_row_route names for it.  `nlen` = transform length, `logn` = its log2 or -1.
// Sub-transform form (swiftly_mixed.h): qmul = Q > 1 says that `a` is sub-transform j = qadd of a length-Q*2^logn
// transform whose radix-Q pass has run: the input is the plain scratch of that pass (a.raw_ld set by the caller, element
// e at in + e*in_cs), the store map refers to the full length a.full_n with plain output index Q*e + j.
template <typename R>
static int run_rows_chunk(swiftly_hip* h, int64_t nlen, int logn, RowsArgs<R>& a, const OffTab& tab, hipStream_t st, int qmul, int qadd) {
    const bool sub = qmul > 1;
    const bool all_j = sub && qadd < 0;  // all Q sub-transforms in this launch: outer index = j, input at in + j*in_os
    if (logn >= 0) {
        a.tw = twiddles<R>(h, logn);
        a.full_logn = logn;
        if (!sub) a.full_n = 0;
        a.ld_mul = 1;
        a.st_mul = qmul;
        a.st_add0 = all_j ? 0 : qadd;
        a.ld_addmul = 0;
        a.st_addmul = all_j ? 1 : 0;
        a.outer = all_j ? qmul : 1;
        // the Q sub-transforms of a row write interleaved elements of the same lines: their workgroups are enumerated 8 block
        // ids apart = on one XCD, whose L2 merges the partial lines (K1 of 24k[1]-n12k-1k 1.52 -> 0.88 ms per facet, r3)
        a.outer_group = all_j ? 1 : 0;
        if (!all_j) a.in_os = 0;
        a.out_os = 0;
        a.tw_full = nullptr;
        a.tw_on_store = 0;
        a.raw_st = 0;
        if (!sub) a.raw_ld = 0;
    }
    const RowRoute route = choose_row_route(row_call_of(h, nlen, logn, a, tab, qmul, qadd));
    switch (route.kind) {
    case kRouteEmpty:
        return 0;
    case kRouteMixed:
        return run_rows_mixed(h, nlen, h->mixed.find(nlen)->second, a, tab, st);
    case kRouteBluestein:
        return run_rows_bluestein(h, nlen, a, tab, st);
    case kRouteLongRowsF64:
        if constexpr (sizeof(R) == 8) return run_rows_long(h, logn, a, tab, st);
        break;
    case kRouteGeneric:
        return launch_checked(logn, a, tab, st);
    case kRouteFourStep:
        return run_rows_four_step(h, logn, a, tab, st, qmul, qadd);
    case kRouteRefused:
        return refuse_route(route.refusal, sizeof(R) == 8, nlen, logn);
    default:
        break;
    }
    if constexpr (sizeof(R) == 4) {  // the lean complex64 routes
        switch (route.kind) {
        case kRouteColPass: {
            ColZ cz;
            const ColPassArgs c = col_pass_of(logn, a, tab, cz);
            const int rc = col_transform(h, logn, c, cz, a.nrows, a.nbatch > 0 ? a.nbatch : 1, st);
            return rc == -1 ? fail(SWIFTLY_ERR_HIP, "internal: the column passes refuse a call of their route") : rc;
        }
        case kRouteLean:
            return launch_status(launch_row_pass(logn, route.mode, row_pass_of(a), st));
        case kRouteSplit32k: {
            const RowPassArgs r = row_pass_of(a);
            return launch_status(launch_row_pass_split(r, twiddles<float>(h, 14), twiddles<float>(h, 13), r.tw, st));
        }
        case kRouteBand32kPlain:
        case kRouteBand32kMapped:
        case kRouteBand64k:
            return launch_band_route(h, route, logn, row_pass_of(a), st);
        default:
            break;
        }
    }
    return fail(SWIFTLY_ERR_HIP, "internal: route %d in the wrong precision", route.kind);
}

// `fill(b, tab_index)` sets the per-item offsets of batch item b into the
// OffTab; called once per item per chunk.  `nlen` = transform length, `logn` = its log2 or -1.
template <typename R, class Fill>
static int run_rows(swiftly_hip* h, int64_t nlen, int logn, RowsArgs<R>& a, const Batch& bt, int use_bits, Fill&& fill,
                    hipStream_t st) {
    const cx<R>* in0 = a.in;
    cx<R>* out0 = a.out;
    const R* win0 = a.st.win;
    for (int64_t b0 = 0; b0 == 0 || b0 < bt.n; b0 += kMaxBatch) {  // (an empty batch: one chunk without items, for the refusals)
        const int nb = (int)std::min<int64_t>(kMaxBatch, std::max<int64_t>(bt.n, 0) - b0);
        OffTab tab;
        tab.use = bt.offs ? use_bits : 0;
        if (tab.use)
            for (int b = 0; b < nb; b++) fill(b0 + b, b, tab);
        RowsArgs<R> c = a;
        c.in = in0 + b0 * bt.in_bs;
        c.out = out0 + b0 * bt.out_bs;
        c.in_bs = bt.in_bs;
        c.out_bs = bt.out_bs;
        c.nbatch = nb;
        c.st_win_bs = bt.mask_bs;
        if (win0) c.st.win = win0 + b0 * bt.mask_bs;
        if (int rc = run_rows_chunk(h, nlen, logn, c, tab, st)) return rc;
    }
    return 0;
}

template <typename R>
static void fill_io(RowsArgs<R>& a, const void* in, int64_t rows, int64_t in_rs, int64_t in_cs, void* out,
                    int64_t out_rs, int64_t out_cs) {
    std::memset(&a, 0, sizeof a);
    a.in = (const cx<R>*)in;
    a.out = (cx<R>*)out;
    a.in_rs = in_rs;
    a.in_cs = (unsigned)in_cs;
    a.out_rs = out_rs;
    a.out_cs = (unsigned)out_cs;
    a.nrows = (int)rows;
    a.scale = (R)1;
    // lanes run along rows when rows are the contiguous direction
    a.rowfast = (in_rs == 1 && in_cs != 1) ? 1 : 0;
}

static const auto kNoFill = [](int64_t, int, OffTab&) {};

// row_gather_off: when not INT64_MIN, the rows of `in` are gathered like
// extract_from_facet(subgrid_off = row_gather_off) would along the OTHER axis
// (fuses api_helper.extract_column, api_helper.py:200-210, into one kernel).
template <typename R>
static int do_prepare_facet(swiftly_hip* h, const void* in, int64_t rows, int64_t yB, int64_t in_rs, int64_t in_cs,
                            void* out, int64_t out_rs, int64_t out_cs, int64_t off, int64_t row_gather_off,
                            const int32_t* out_rowmap, const int32_t* in_rowmap, int fold_other, int no_window,
                            hipStream_t st, bool real_in = false) {
    const int yN = (int)h->yN;
    RowsArgs<R> a;
    fill_io(a, in, rows, in_rs, in_cs, out, out_rs, out_cs);
    a.real_in = real_in ? 1 : 0;  // `in` points to R, in_rs / in_cs count real elements
    a.ld = axis_map<R>(facet_in_padded_facet(*h, yB, off), invp<R>(h) + facet_lo(*h, yB));
    a.st = axis_map<R>(whole(yN));
    a.conj_ld = a.conj_st = 1;
    a.scale = (R)(1.0 / yN);
    a.st_rowmap = out_rowmap;
    a.in_rowmap = in_rowmap;
    if (no_window) a.ld.win = nullptr;
    if (fold_other) a.row_win = invp<R>(h) + facet_lo(*h, rows);  // the rows of this call are the other axis
    if (row_gather_off != INT64_MIN) {
        const Window w = window_of(*h, row_gather_off);
        a.rm_mod = (int)h->m;
        a.rm_inner = w.rot;
        a.rm_outer = w.base;
        a.rm_full = yN;
    }
    return run_rows(h, h->yN, h->log_yN, a, Batch{}, 0, kNoFill, st);
}

template <typename R>
static int do_add_to_subgrid(swiftly_hip* h, const void* in, int64_t rows, int64_t in_rs, int64_t in_cs, void* out,
                             int64_t out_rs, int64_t out_cs, int64_t off, const Batch& bt, hipStream_t st) {
    RowsArgs<R> a;
    fill_io(a, in, rows, in_rs, in_cs, out, out_rs, out_cs);
    a.ld = axis_map<R>(whole(h->m));
    a.st = axis_map<R>(contribution_in_padded_subgrid(*h, off), fnwin<R>(h));
    a.accumulate = 1;
    return run_rows(h, h->m, h->log_m, a, bt, 4 | 8, [&](int64_t gb, int b, OffTab& t) {
        const Map g = contribution_in_padded_subgrid(*h, bt.offs[gb]);
        t.st_a[b] = g.a; t.st_c[b] = g.c;
    }, st);
}

template <typename R>
static int do_finish_subgrid(swiftly_hip* h, const void* in, int64_t rows, int64_t in_rs, int64_t in_cs, void* out,
                             int64_t out_rs, int64_t out_cs, int64_t off, int64_t xA, const void* mask,
                             const Batch& bt, hipStream_t st) {
    const int xM = (int)h->xM;
    RowsArgs<R> a;
    fill_io(a, in, rows, in_rs, in_cs, out, out_rs, out_cs);
    a.ld = axis_map<R>(whole(xM));
    a.st = axis_map<R>(subgrid_in_padded_subgrid(*h, xA, off), (const R*)mask);
    a.conj_ld = a.conj_st = 1;
    a.scale = (R)(1.0 / xM);
    return run_rows(h, h->xM, h->log_xM, a, bt, 4,
                    [&](int64_t gb, int b, OffTab& t) { t.st_a[b] = subgrid_in_padded_subgrid(*h, xA, bt.offs[gb]).a; }, st);
}

template <typename R>
static int do_prepare_subgrid(swiftly_hip* h, const void* in, int64_t rows, int64_t xA, int64_t in_rs, int64_t in_cs,
                              void* out, int64_t out_rs, int64_t out_cs, int64_t off, const Batch& bt,
                              hipStream_t st) {
    const int xM = (int)h->xM;
    RowsArgs<R> a;
    fill_io(a, in, rows, in_rs, in_cs, out, out_rs, out_cs);
    a.ld = axis_map<R>(subgrid_in_padded_subgrid(*h, xA, off));
    a.st = axis_map<R>(whole(xM));
    return run_rows(h, h->xM, h->log_xM, a, bt, 1,
                    [&](int64_t gb, int b, OffTab& t) { t.ld_a[b] = subgrid_in_padded_subgrid(*h, xA, bt.offs[gb]).a; }, st);
}

template <typename R>
static int do_extract_from_subgrid(swiftly_hip* h, const void* in, int64_t rows, int64_t in_rs, int64_t in_cs,
                                   void* out, int64_t out_rs, int64_t out_cs, int64_t off, const Batch& bt,
                                   hipStream_t st) {
    RowsArgs<R> a;
    fill_io(a, in, rows, in_rs, in_cs, out, out_rs, out_cs);
    a.ld = axis_map<R>(contribution_in_padded_subgrid(*h, off), fnwin<R>(h));
    a.st = axis_map<R>(whole(h->m));
    a.conj_ld = a.conj_st = 1;
    a.scale = (R)(1.0 / (int)h->m);
    return run_rows(h, h->m, h->log_m, a, bt, 1 | 2, [&](int64_t gb, int b, OffTab& t) {
        const Map g = contribution_in_padded_subgrid(*h, bt.offs[gb]);
        t.ld_a[b] = g.a; t.ld_c[b] = g.c;
    }, st);
}

template <typename R>
static int do_finish_facet(swiftly_hip* h, const void* in, int64_t rows, int64_t in_rs, int64_t in_cs, void* out,
                           int64_t out_rs, int64_t out_cs, int64_t off, int64_t yB, const void* mask, const Batch& bt,
                           hipStream_t st, int64_t band_start = 0, int64_t band_len = -1, bool real_out = false) {
    const int yN = (int)h->yN;
    RowsArgs<R> a;
    fill_io(a, in, rows, in_rs, in_cs, out, out_rs, out_cs);
    a.real_out = real_out ? 1 : 0;  // `out` points to R, out_rs / out_cs count real elements
    a.ld = axis_map<R>(whole(yN));
    // band input: element d of a row is column (band_start + d) mod yN of the padded facet, the rest is zero
    if (band_len >= 0) a.ld = axis_map<R>(band_as_load_map(*h, band_start, band_len));
    // mask goes to `win` (it is the per-item one), the PSWF window to `win2`
    a.st = axis_map<R>(facet_in_padded_facet(*h, yB, off), (const R*)mask, invp<R>(h) + facet_lo(*h, yB));
    return run_rows(h, h->yN, h->log_yN, a, bt, 4,
                    [&](int64_t gb, int b, OffTab& t) { t.st_a[b] = facet_in_padded_facet(*h, yB, bt.offs[gb]).a; }, st);
}

extern "C" {

int swiftly_hip_supports_dtype(const swiftly_hip_t* h, int dtype) {
    if (!h || (dtype != SWIFTLY_C64 && dtype != SWIFTLY_C128)) return 0;
    for (const auto& [n, logn] : {std::pair<int64_t, int>{h->yN, h->log_yN}, {h->xM, h->log_xM}, {h->m, h->log_m}}) {
        const bool dbl = dtype == SWIFTLY_C128;
        const bool ok = row_length_supported(dbl, logn, use_mixed(h, n, dbl), have_bluestein(h, n, dbl));
        if (!ok) return 0;
    }
    return 1;
}

int swiftly_hip_prepare_facet(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                              int64_t in_rs, int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs,
                              int64_t facet_off, void* stream) {
    CHECK_COMMON();
    CHECK_FACET_SIZE();
    return DISPATCH(do_prepare_facet, h, in, rows, facet_size, in_rs, in_cs, out, out_rs, out_cs, facet_off, INT64_MIN,
                    nullptr, nullptr, 0, 0, (hipStream_t)stream);
}

int swiftly_hip_prepare_facet_rows(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                   int64_t in_rs, int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs,
                                   int64_t facet_off, const int32_t* out_rowmap, int fold_other_axis_window,
                                   void* stream) {
    CHECK_COMMON();
    CHECK_FACET_SIZE();
    if (fold_other_axis_window && (rows <= 0 || rows >= h->yN))
        return fail(SWIFTLY_ERR_PARAM, "other-axis facet size %lld must be in [1, yN_size - 1]", (long long)rows);
    return DISPATCH(do_prepare_facet, h, in, rows, facet_size, in_rs, in_cs, out, out_rs, out_cs, facet_off, INT64_MIN,
                    out_rowmap, nullptr, fold_other_axis_window, 0, (hipStream_t)stream);
}

int swiftly_hip_extract_column(swiftly_hip_t* h, int dtype, const void* in, int64_t facet_size, int64_t in_rs,
                               int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs, int64_t subgrid_off0,
                               int64_t facet_off1, void* stream) {
    const int64_t rows = h ? h->m : 0;
    CHECK_COMMON();
    CHECK_FACET_SIZE();
    return DISPATCH(do_prepare_facet, h, in, rows, facet_size, in_rs, in_cs, out, out_rs, out_cs, facet_off1,
                    subgrid_off0, nullptr, nullptr, 0, 0, (hipStream_t)stream);
}

int swiftly_hip_extract_column_rows(swiftly_hip_t* h, int dtype, const void* in, int64_t facet_size, int64_t in_rs,
                                    int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs, int64_t subgrid_off0,
                                    int64_t facet_off1, const int32_t* in_rowmap, int prewindowed, void* stream) {
    const int64_t rows = h ? h->m : 0;
    CHECK_COMMON();
    CHECK_FACET_SIZE();
    return DISPATCH(do_prepare_facet, h, in, rows, facet_size, in_rs, in_cs, out, out_rs, out_cs, facet_off1,
                    subgrid_off0, nullptr, in_rowmap, 0, prewindowed, (hipStream_t)stream);
}

int swiftly_hip_extract_from_facet_batch(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_rs,
                                         int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs,
                                         int64_t subgrid_off, int64_t nbatch, int64_t in_bs, int64_t out_bs,
                                         const int64_t* subgrid_offs, void* stream) {
    CHECK_COMMON();
    CHECK_BATCH();
    Batch bt{nbatch, in_bs, out_bs, subgrid_offs, 0};
    if (dtype == SWIFTLY_C64)
        return run_modcopy<float, false>(h, in, rows, in_rs, in_cs, out, out_rs, out_cs, subgrid_off, bt, (hipStream_t)stream);
    return run_modcopy<double, false>(h, in, rows, in_rs, in_cs, out, out_rs, out_cs, subgrid_off, bt, (hipStream_t)stream);
}
int swiftly_hip_extract_from_facet(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_rs,
                                   int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs, int64_t subgrid_off,
                                   void* stream) {
    return swiftly_hip_extract_from_facet_batch(h, dtype, in, rows, in_rs, in_cs, out, out_rs, out_cs, subgrid_off, 1,
                                                0, 0, nullptr, stream);
}

int swiftly_hip_add_to_subgrid_batch(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_rs,
                                     int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs, int64_t facet_off,
                                     int64_t nbatch, int64_t in_bs, int64_t out_bs, const int64_t* facet_offs,
                                     void* stream) {
    CHECK_COMMON();
    CHECK_BATCH();
    CHECK_ACCUMULATE_BATCH();
    Batch bt{nbatch, in_bs, out_bs, facet_offs, 0};
    return DISPATCH(do_add_to_subgrid, h, in, rows, in_rs, in_cs, out, out_rs, out_cs, facet_off, bt, (hipStream_t)stream);
}
int swiftly_hip_add_to_subgrid(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_rs,
                               int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs, int64_t facet_off,
                               void* stream) {
    return swiftly_hip_add_to_subgrid_batch(h, dtype, in, rows, in_rs, in_cs, out, out_rs, out_cs, facet_off, 1, 0, 0,
                                            nullptr, stream);
}

int swiftly_hip_finish_subgrid_batch(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_rs,
                                     int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs, int64_t subgrid_off,
                                     int64_t subgrid_size, const void* mask, int64_t nbatch, int64_t in_bs,
                                     int64_t out_bs, const int64_t* subgrid_offs, int64_t mask_bs, void* stream) {
    CHECK_COMMON();
    CHECK_BATCH();
    CHECK_SUBGRID_SIZE();
    Batch bt{nbatch, in_bs, out_bs, subgrid_offs, mask ? mask_bs : 0};
    return DISPATCH(do_finish_subgrid, h, in, rows, in_rs, in_cs, out, out_rs, out_cs, subgrid_off, subgrid_size, mask,
                    bt, (hipStream_t)stream);
}
int swiftly_hip_finish_subgrid(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_rs,
                               int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs, int64_t subgrid_off,
                               int64_t subgrid_size, const void* mask, void* stream) {
    return swiftly_hip_finish_subgrid_batch(h, dtype, in, rows, in_rs, in_cs, out, out_rs, out_cs, subgrid_off,
                                            subgrid_size, mask, 1, 0, 0, nullptr, 0, stream);
}

int swiftly_hip_prepare_subgrid_batch(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t subgrid_size,
                                      int64_t in_rs, int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs,
                                      int64_t subgrid_off, int64_t nbatch, int64_t in_bs, int64_t out_bs,
                                      const int64_t* subgrid_offs, void* stream) {
    CHECK_COMMON();
    CHECK_BATCH();
    CHECK_SUBGRID_SIZE();
    Batch bt{nbatch, in_bs, out_bs, subgrid_offs, 0};
    return DISPATCH(do_prepare_subgrid, h, in, rows, subgrid_size, in_rs, in_cs, out, out_rs, out_cs, subgrid_off, bt,
                    (hipStream_t)stream);
}
int swiftly_hip_prepare_subgrid(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t subgrid_size,
                                int64_t in_rs, int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs,
                                int64_t subgrid_off, void* stream) {
    return swiftly_hip_prepare_subgrid_batch(h, dtype, in, rows, subgrid_size, in_rs, in_cs, out, out_rs, out_cs,
                                             subgrid_off, 1, 0, 0, nullptr, stream);
}

// Swiftly.prepare_subgrid_inplace(data[rows, xM], subgrid_off) (core.py:837-840): `data` holds the subgrid already
// zero-padded to xM (pad_mid: centred); in place it becomes fft(roll(data, subgrid_off)) along the strided/contiguous
// axis given by the two strides.  = prepare_subgrid with subgrid_size = xM_size and in == out: every kernel reads all
// of a row (column tile) before it writes any of it, and the four-step passes go through their own scratch.
int swiftly_hip_prepare_subgrid_inplace(swiftly_hip_t* h, int dtype, void* data, int64_t rows, int64_t row_stride,
                                        int64_t col_stride, int64_t subgrid_off, void* stream) {
    if (!h) return fail(SWIFTLY_ERR_PARAM, "null argument");
    return swiftly_hip_prepare_subgrid(h, dtype, data, rows, h->xM, row_stride, col_stride, data, row_stride, col_stride,
                                       subgrid_off, stream);
}
// Swiftly.prepare_subgrid_inplace_2d(data[xM, xM], off0, off1) (core.py:851-853): both axes, axis 1 first
int swiftly_hip_prepare_subgrid_inplace_2d(swiftly_hip_t* h, int dtype, void* data, int64_t row_stride, int64_t col_stride,
                                           int64_t subgrid_off0, int64_t subgrid_off1, void* stream) {
    if (!h) return fail(SWIFTLY_ERR_PARAM, "null argument");
    int rc = swiftly_hip_prepare_subgrid_inplace(h, dtype, data, h->xM, row_stride, col_stride, subgrid_off1, stream);
    if (rc) return rc;
    return swiftly_hip_prepare_subgrid_inplace(h, dtype, data, h->xM, col_stride, row_stride, subgrid_off0, stream);
}
// Swiftly.add_to_subgrid_2d(in[m, m], out[xM, xM], facet_off0, facet_off1) (core.py:752-778; numpy form = two
// add_to_subgrid calls, core.py:274-285): ACCUMULATES.  Axis 0 first, as api_helper.py:85-99 does it (the float32
// rounding of the two orders differs: 5.6e-7 vs 9.0e-7 on the reference-generated golden contribution), into a
// stream-ordered [xM, m] intermediate, then axis 1 straight into `out`.
int swiftly_hip_add_to_subgrid_2d(swiftly_hip_t* h, int dtype, const void* in, int64_t in_row_stride,
                                  int64_t in_col_stride, void* out, int64_t out_row_stride, int64_t out_col_stride,
                                  int64_t facet_off0, int64_t facet_off1, void* stream) {
    const int64_t rows = h ? h->m : 0, in_cs = in_col_stride, out_cs = out_col_stride;
    CHECK_COMMON();
    const int64_t m = h->m, xM = h->xM;
    const size_t esz = dtype == SWIFTLY_C64 ? 8 : 16;
    void* tmp = nullptr;
    HIP_TRY(hipMallocAsync(&tmp, (size_t)m * (size_t)xM * esz, (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(tmp, 0, (size_t)m * (size_t)xM * esz, (hipStream_t)stream));  // add_to_subgrid accumulates
    // axis 0: the transform runs along the rows of `in` = its strided axis; the "rows" of the primitive are the m columns
    int rc = swiftly_hip_add_to_subgrid(h, dtype, in, m, in_col_stride, in_row_stride, tmp, 1, m, facet_off0, stream);
    if (!rc) rc = swiftly_hip_add_to_subgrid(h, dtype, tmp, xM, m, 1, out, out_row_stride, out_col_stride, facet_off1, stream);
    hipError_t e = hipFreeAsync(tmp, (hipStream_t)stream);
    if (!rc && e != hipSuccess) return fail(SWIFTLY_ERR_HIP, "hipFreeAsync: %s", hipGetErrorString(e));
    return rc;
}

int swiftly_hip_extract_from_subgrid_batch(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_rs,
                                           int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs,
                                           int64_t facet_off, int64_t nbatch, int64_t in_bs, int64_t out_bs,
                                           const int64_t* facet_offs, void* stream) {
    CHECK_COMMON();
    CHECK_BATCH();
    Batch bt{nbatch, in_bs, out_bs, facet_offs, 0};
    return DISPATCH(do_extract_from_subgrid, h, in, rows, in_rs, in_cs, out, out_rs, out_cs, facet_off, bt,
                    (hipStream_t)stream);
}
int swiftly_hip_extract_from_subgrid(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_rs,
                                     int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs, int64_t facet_off,
                                     void* stream) {
    return swiftly_hip_extract_from_subgrid_batch(h, dtype, in, rows, in_rs, in_cs, out, out_rs, out_cs, facet_off, 1,
                                                  0, 0, nullptr, stream);
}

int swiftly_hip_add_to_facet_batch(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_rs,
                                   int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs, int64_t subgrid_off,
                                   int64_t nbatch, int64_t in_bs, int64_t out_bs, const int64_t* subgrid_offs,
                                   void* stream) {
    CHECK_COMMON();
    CHECK_BATCH();
    CHECK_ACCUMULATE_BATCH();
    Batch bt{nbatch, in_bs, out_bs, subgrid_offs, 0};
    if (dtype == SWIFTLY_C64)
        return run_modcopy<float, true>(h, in, rows, in_rs, in_cs, out, out_rs, out_cs, subgrid_off, bt, (hipStream_t)stream);
    return run_modcopy<double, true>(h, in, rows, in_rs, in_cs, out, out_rs, out_cs, subgrid_off, bt, (hipStream_t)stream);
}
int swiftly_hip_add_to_facet(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_rs, int64_t in_cs,
                             void* out, int64_t out_rs, int64_t out_cs, int64_t subgrid_off, void* stream) {
    return swiftly_hip_add_to_facet_batch(h, dtype, in, rows, in_rs, in_cs, out, out_rs, out_cs, subgrid_off, 1, 0, 0,
                                          nullptr, stream);
}

int swiftly_hip_finish_facet_batch(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_rs,
                                   int64_t in_cs, void* out, int64_t out_rs, int64_t out_cs, int64_t facet_off,
                                   int64_t facet_size, const void* mask, int64_t nbatch, int64_t in_bs,
                                   int64_t out_bs, const int64_t* facet_offs, int64_t mask_bs, void* stream) {
    CHECK_COMMON();
    CHECK_BATCH();
    CHECK_FACET_SIZE();
    Batch bt{nbatch, in_bs, out_bs, facet_offs, mask ? mask_bs : 0};
    return DISPATCH(do_finish_facet, h, in, rows, in_rs, in_cs, out, out_rs, out_cs, facet_off, facet_size, mask, bt,
                    (hipStream_t)stream);
}
int swiftly_hip_finish_facet(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_rs, int64_t in_cs,
                             void* out, int64_t out_rs, int64_t out_cs, int64_t facet_off, int64_t facet_size,
                             const void* mask, void* stream) {
    return swiftly_hip_finish_facet_batch(h, dtype, in, rows, in_rs, in_cs, out, out_rs, out_cs, facet_off, facet_size,
                                          mask, 1, 0, 0, nullptr, 0, stream);
}

// The eight K1 entry points below are one implementation: prepare_facet_band for the rows [other_axis_row0,
// other_axis_row0 + rows) of a facet whose other axis has other_axis_size pixels -- the folded window of the other axis is
// that facet's, not the one of a `rows`-pixel facet (cooperative facets of the multi-GPU pass: every rank transforms a block
// of rows of the same facet); other_axis_size = 0: no window of the other axis.  The forms differ in the capability rule they
// consult, the window fields and the launcher; the real forms read float32 rows (in_row_stride counts reals, dtype = the
// output type).
enum class K1Form {
    Band,            // the band row kernel (or, for short rows and complex128, the generic contiguous-axis prepare_facet)
    RealBand,        // ... loading float32 rows: SWIFTLY_FEATURE_REAL_FACETS
    HalfLengthBand,  // one half-length transform per real row (swiftly_rowreal.h), SWIFTLY_FEATURE_REAL_FACETS_RFFT or
                     // _RFFT_64K (the compact section and the launcher's instance follow log_yN): its own
                     // kernel and its own refusals -- a call the kernel does not take is refused before anything is written,
                     // never handed to the band row kernel
    WindowRows,      // the whole-row kernel storing complete window rows (swiftly_rowwhole.h)
    RealWindowRows,  // ... loading float32 rows: SWIFTLY_FEATURE_REAL_WINDOW_ROWS
    RealBand64,      // Band in complex128 loading FLOAT64 rows: SWIFTLY_FEATURE_REAL_FACETS_F64 (a door of its own: the float32
                     // forms above keep refusing complex128)
};
static int prepare_facet_k1(K1Form form, swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                            int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off, int64_t band_start,
                            int64_t band_len, int64_t other_axis_size, int64_t other_axis_row0, void* stream,
                            const int32_t* win_d = nullptr, int64_t nwin = 0, int64_t win_stride = 0) {
    const bool half = form == K1Form::HalfLengthBand;
    const bool windows = form == K1Form::WindowRows || form == K1Form::RealWindowRows;
    const bool real_in = form != K1Form::Band && form != K1Form::WindowRows;
    const int fold_other_axis_window = other_axis_size > 0;
    if (!h || !in || !out) return fail(SWIFTLY_ERR_PARAM, "null argument");
    if (fold_other_axis_window && (other_axis_row0 < 0 || other_axis_row0 + rows > other_axis_size))
        return fail(SWIFTLY_ERR_PARAM, "rows [%lld, +%lld) are not inside a facet of %lld rows", (long long)other_axis_row0,
                    (long long)rows, (long long)other_axis_size);
    DeviceGuard device_guard_(h->device);
    CHECK_DTYPE();
    if (real_in) {  // float32 (RealBand64: float64) rows: the capability rule of the form's feature
        const std::string why = form == K1Form::RealWindowRows ? why_not_real_window_rows(*h, dtype)
                                : form == K1Form::RealBand64   ? why_not_real_facets_f64(*h, dtype)
                                : half                         ? why_not_half_length_k1(*h, dtype)
                                                               : why_not_real_facets(*h, dtype);
        if (!why.empty())
            return fail(SWIFTLY_ERR_UNSUPPORTED, "%s: %s", form == K1Form::RealWindowRows ? "prepare_facet_window_rows_real"
                        : form == K1Form::RealBand64 ? "prepare_facet_band_real64"
                        : half ? "prepare_facet_band_rfft" : "prepare_facet_band_real", why.c_str());
    }
    CHECK_FACET_SIZE();
    const int yN = (int)h->yN;
    if (dtype == SWIFTLY_C128) {
        // complex128: the plain band layout that keeps the whole padded axis, through the complex128 row transforms (one
        // workgroup per row up to 8192 points, the two-kernel long-row form for 16384 / 32768)
        if (h->log_yN < kMinLogN || h->log_yN > kBandMaxLogYNC128)
            return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_band: complex128 needs a power-of-two yN_size of 8 .. 32768, got %d", yN);
        if (band_start != 0 || band_len != yN)
            return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_band: complex128 keeps the whole padded axis (band must be (0, yN_size))");
        if (windows) return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_window_rows: complex64 only");
        if (rows < 0 || rows > 0x7fffffff) return fail(SWIFTLY_ERR_PARAM, "bad row count");
        if (fold_other_axis_window && (other_axis_row0 != 0 || other_axis_size != rows))
            return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_band_rows: complex128 has no row blocks");
        if (rows == 0) return 0;
        return do_prepare_facet<double>(h, in, rows, facet_size, in_row_stride, 1, out, out_row_stride, 1, facet_off, INT64_MIN,
                                        nullptr, nullptr, fold_other_axis_window, 0, (hipStream_t)stream,
                                        /*real_in=*/form == K1Form::RealBand64);  // (the only real form its rule lets through)
    }
    const bool mixed_yN = h->log_yN < 0 && h->mixed.count(h->yN) && h->mixed.at(h->yN).tw_f;
    if (!mixed_yN && (h->log_yN < kMinLogN || h->log_yN > kBandMaxLogYN))
        return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_band: padded facet size %d not supported (power of two 8 .. 65536, or Q * 2^k with Q = 3, 5, 7, 9)", yN);
    if (rows < 0 || rows > 0x7fffffff) return fail(SWIFTLY_ERR_PARAM, "bad row count");
    CHECK_BAND();
    if (fold_other_axis_window && (other_axis_size <= 0 || other_axis_size >= h->yN))
        return fail(SWIFTLY_ERR_PARAM, "other-axis facet size %lld must be in [1, yN_size - 1]", (long long)other_axis_size);
    const Map facet = facet_in_padded_facet(*h, facet_size, facet_off);
    if (half) {  // two adjacent reals per 8-byte load: z[n] = (x[2n], x[2n+1]) must be one aligned pair of every row
        if (facet_size & 1)
            return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_band_rfft: real facets, half-length: odd facet size %lld", (long long)facet_size);
        if (facet.a & 1)
            return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_band_rfft: real facets, half-length: the facet starts at an odd index of the "
                        "padded row (load offset %d, facet offset %lld)", facet.a, (long long)facet_off);
        if (in_row_stride & 1)
            return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_band_rfft: real facets, half-length: odd row stride %lld", (long long)in_row_stride);
        if (reinterpret_cast<uintptr_t>(in) & 7)
            return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_band_rfft: real facets, half-length: input is not 8-byte aligned");
    }
    if (rows == 0) return 0;
    if (!band_is_split(h)) {  // (never the half-length form: its capability rules need yN_size 32768 or 65536)
        // short rows: the generic contiguous-axis prepare_facet, whole padded axis, plain column order
        if (band_start != 0 || band_len != yN)
            return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_band: yN_size %d keeps the whole padded axis (band must be (0, yN_size))", yN);
        if (fold_other_axis_window && (other_axis_row0 != 0 || other_axis_size != rows))
            return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_band_rows: row blocks need the split band layout (yN_size 16384 .. 65536)");
        return do_prepare_facet<float>(h, in, rows, facet_size, in_row_stride, 1, out, out_row_stride, 1, facet_off, INT64_MIN,
                                       nullptr, nullptr, fold_other_axis_window, 0, (hipStream_t)stream, real_in);
    }
    RowPassArgs r;
    std::memset(&r, 0, sizeof r);
    r.in = (const cx<float>*)in; r.out = (cx<float>*)out;
    r.in_pitch = in_row_stride; r.out_pitch = out_row_stride;
    r.in_real = real_in ? 1 : 0;  // `in` points to float32, in_pitch counts real elements
    r.nrows = (int)rows;
    r.ld_a = facet.a; r.ld_len = facet.len; r.ld_c = facet.c; r.ld_mod = facet.mod;
    r.ld_win = h->invp_f + facet_lo(*h, facet_size);
    r.st_len = yN; r.st_mod = yN;
    r.scale = (float)(1.0 / yN);
    r.conj_ld = r.conj_st = 1;
    r.row_win = fold_other_axis_window ? h->invp_f + (facet_lo(*h, other_axis_size) + (int)other_axis_row0) : nullptr;
    r.band_start = (int)band_start; r.band_len = (int)band_len; r.band_half = (int)band_half_columns(band_len);
    if (half) r.twc = compact_twiddles(h, h->log_yN - 1, 5);  // 32 points per lane of the half-length transform
    const cx<float>* twh = twiddles<float>(h, h->log_yN - 1);
    const cx<float>* twf = twiddles<float>(h, h->log_yN);
    if (!twh || !twf || (half && !r.twc)) return fail(SWIFTLY_ERR_HIP, "internal: missing twiddle tables");
    if (half) {
        const int e = launch_row_real_band(h->log_yN, r, twh, twf, (hipStream_t)stream);
        if (e == -1) return fail(SWIFTLY_ERR_HIP, "internal: prepare_facet_band_rfft: the half-length kernel does not take this call");
        return launch_status(e);
    }
    if (windows) {  // complete window rows (whole-row kernel)
        r.win_full = 1;
        r.win_pitch = win_stride;
        r.win_d = win_d; r.nwin = (int)nwin; r.win_logm = h->log_m;
        r.win_sp = pmod(facet_shift(*h, facet_off), h->m);
        r.win_fn = h->fn_f;
        r.win_tw_m = twiddles<float>(h, h->log_m);
        r.win_twc_m = h->log_m >= 6 ? compact_twiddles(h, h->log_m, h->log_m - 6) : nullptr;
    }
    int e = launch_row_pass_band_n(h->log_yN, r, twh, twf, (hipStream_t)stream, &h->win4);
    if (e == -2)
        return fail(SWIFTLY_ERR_UNSUPPORTED, "prepare_facet_window_rows: needs yN_size 32768, contribution size 512, even facet "
                    "size / offset / row stride and a band of at most %d physical columns%s", row_pass_whole_stage_columns(),
                    real_in ? ", an even real row stride and an 8-byte-aligned input" : "");
    return launch_status(e);
}

// the entry points: every band form for a row block (`_rows`) and for a whole facet (the block that is all of its rows)
int swiftly_hip_prepare_facet_band_rows(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                        int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                        int64_t band_start, int64_t band_len, int64_t other_axis_size,
                                        int64_t other_axis_row0, void* stream) {
    return prepare_facet_k1(K1Form::Band, h, dtype, in, rows, facet_size, in_row_stride, out, out_row_stride, facet_off,
                            band_start, band_len, other_axis_size, other_axis_row0, stream);
}
int swiftly_hip_prepare_facet_band(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                   int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                   int64_t band_start, int64_t band_len, int fold_other_axis_window, void* stream) {
    return swiftly_hip_prepare_facet_band_rows(h, dtype, in, rows, facet_size, in_row_stride, out, out_row_stride, facet_off,
                                               band_start, band_len, fold_other_axis_window ? rows : 0, 0, stream);
}
int swiftly_hip_prepare_facet_band_rows_real(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                             int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                             int64_t band_start, int64_t band_len, int64_t other_axis_size,
                                             int64_t other_axis_row0, void* stream) {
    return prepare_facet_k1(K1Form::RealBand, h, dtype, in, rows, facet_size, in_row_stride, out, out_row_stride, facet_off,
                            band_start, band_len, other_axis_size, other_axis_row0, stream);
}
int swiftly_hip_prepare_facet_band_real(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                        int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                        int64_t band_start, int64_t band_len, int fold_other_axis_window, void* stream) {
    return swiftly_hip_prepare_facet_band_rows_real(h, dtype, in, rows, facet_size, in_row_stride, out, out_row_stride, facet_off,
                                                    band_start, band_len, fold_other_axis_window ? rows : 0, 0, stream);
}
int swiftly_hip_prepare_facet_band_real64(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                          int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                          int64_t band_start, int64_t band_len, int fold_other_axis_window, void* stream) {
    return prepare_facet_k1(K1Form::RealBand64, h, dtype, in, rows, facet_size, in_row_stride, out, out_row_stride, facet_off,
                            band_start, band_len, fold_other_axis_window ? rows : 0, 0, stream);
}
int swiftly_hip_prepare_facet_band_rows_rfft(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                             int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                             int64_t band_start, int64_t band_len, int64_t other_axis_size,
                                             int64_t other_axis_row0, void* stream) {
    return prepare_facet_k1(K1Form::HalfLengthBand, h, dtype, in, rows, facet_size, in_row_stride, out, out_row_stride, facet_off,
                            band_start, band_len, other_axis_size, other_axis_row0, stream);
}
int swiftly_hip_prepare_facet_band_rfft(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                        int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                        int64_t band_start, int64_t band_len, int fold_other_axis_window, void* stream) {
    return swiftly_hip_prepare_facet_band_rows_rfft(h, dtype, in, rows, facet_size, in_row_stride, out, out_row_stride, facet_off,
                                                    band_start, band_len, fold_other_axis_window ? rows : 0, 0, stream);
}

// (r6, axis-1-first pipeline) prepare_facet_band_rows that finishes the contiguous axis COMPLETELY inside K1: one persistent
// workgroup per CU owns whole rows (both output parities; swiftly_rowwhole.h), stages the band of a row in LDS and stores, for every
// window w, what swiftly_hip_finish_axis1_rows would produce for wave w from that band:
// out[row][w*m ..] = parity-split window band of  Fn[k] cfft_m(window w)[(k + s'1) mod m].
static int prepare_facet_window_rows(K1Form form, const char* name, swiftly_hip_t* h, int dtype, const void* in, int64_t rows,
                                     int64_t facet_size, int64_t in_row_stride, void* out, int64_t out_row_stride,
                                     int64_t facet_off, int64_t band_start, int64_t band_len, int64_t other_axis_size,
                                     int64_t other_axis_row0, const int32_t* window_starts, int64_t nwindows,
                                     int64_t out_window_stride, void* stream) {
    if (!window_starts || nwindows <= 0) return fail(SWIFTLY_ERR_PARAM, "%s: no windows", name);
    if (h && (out_window_stride < h->m || out_row_stride < h->m ||
              (out_window_stride < rows * out_row_stride && out_row_stride < nwindows * out_window_stride)))
        return fail(SWIFTLY_ERR_PARAM, "%s: the window rows of the output overlap (row stride %lld, window stride %lld)", name,
                    (long long)out_row_stride, (long long)out_window_stride);
    return prepare_facet_k1(form, h, dtype, in, rows, facet_size, in_row_stride, out, out_row_stride, facet_off, band_start,
                            band_len, other_axis_size, other_axis_row0, stream, window_starts, nwindows, out_window_stride);
}
int swiftly_hip_prepare_facet_window_rows(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                          int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                          int64_t band_start, int64_t band_len, int64_t other_axis_size,
                                          int64_t other_axis_row0, const int32_t* window_starts, int64_t nwindows,
                                          int64_t out_window_stride, void* stream) {
    return prepare_facet_window_rows(K1Form::WindowRows, "prepare_facet_window_rows", h, dtype, in, rows, facet_size,
                                     in_row_stride, out, out_row_stride, facet_off, band_start, band_len, other_axis_size,
                                     other_axis_row0, window_starts, nwindows, out_window_stride, stream);
}
// the same for float32 rows: the REAL window-rows instances of the whole-row kernel
int swiftly_hip_prepare_facet_window_rows_real(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t facet_size,
                                               int64_t in_row_stride, void* out, int64_t out_row_stride, int64_t facet_off,
                                               int64_t band_start, int64_t band_len, int64_t other_axis_size,
                                               int64_t other_axis_row0, const int32_t* window_starts, int64_t nwindows,
                                               int64_t out_window_stride, void* stream) {
    return prepare_facet_window_rows(K1Form::RealWindowRows, "prepare_facet_window_rows_real", h, dtype, in, rows, facet_size,
                                     in_row_stride, out, out_row_stride, facet_off, band_start, band_len, other_axis_size,
                                     other_axis_row0, window_starts, nwindows, out_window_stride, stream);
}

// finish_facet_band, its real-output twin (`out` float32, out_row_stride in reals) and the half-length form of the twin: one
// implementation.  The forms differ in the capability rule they consult and, for the half-length form, the launcher.
enum class B8Form {
    Complex,
    RealStore,       // the real-store instances of the row kernels: SWIFTLY_FEATURE_REAL_FACETS_OUT
    HalfLengthReal,  // one half-length transform per row (swiftly_rowc2r.h), SWIFTLY_FEATURE_REAL_FACETS_OUT_C2R or _C2R_64K
                     // (the compact section and the launcher's instance follow log_yN): its own kernel
                     // and its own refusals -- a call the kernel does not take is refused before anything is written, never
                     // handed to the real-store form
    RealStore64,     // complex128 band rows in, FLOAT64 rows out: SWIFTLY_FEATURE_REAL_FACETS_OUT_F64 (a door of its own: the
                     // float32 forms above keep refusing complex128)
};
static int finish_facet_band_impl(B8Form form, swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                  int64_t band_start, int64_t band_len, void* out, int64_t out_row_stride,
                                  int64_t facet_off, int64_t facet_size, const void* mask, void* stream) {
    const int64_t in_cs = 1, out_cs = 1;
    const bool real_out = form != B8Form::Complex, half = form == B8Form::HalfLengthReal;
    const char* name = half ? "finish_facet_band_c2r" : form == B8Form::RealStore64 ? "finish_facet_band_real64" : "finish_facet_band_real";
    CHECK_COMMON();
    if (real_out) {  // float32 (RealStore64: float64) rows out: the capability rule of the form's feature
        const std::string why = half                          ? why_not_half_length_finish(*h, dtype)
                                : form == B8Form::RealStore64 ? why_not_real_facets_out_f64(*h, dtype)
                                                              : why_not_real_facets_out(*h, dtype);
        if (!why.empty()) return fail(SWIFTLY_ERR_UNSUPPORTED, "%s: %s", name, why.c_str());
    }
    CHECK_FACET_SIZE();
    if (real_out && out_row_stride < facet_size)
        return fail(SWIFTLY_ERR_PARAM, "%s: out_row_stride %lld is below facet_size %lld: the rows of the output overlap", name,
                    (long long)out_row_stride, (long long)facet_size);
    // (the gate of swiftly_hip_supports(BACKWARD_BAND_EXPLICIT): identical to BACKWARD_BAND in complex64; complex128 rows run
    // through do_finish_facet<double>, 64 .. 32768 points)
    if (const std::string why = why_not_backward_band(*h, dtype, true); !why.empty())
        return fail(SWIFTLY_ERR_UNSUPPORTED, "finish_facet_band: %s", why.c_str());
    CHECK_BAND();
    if (half) {
        // one 8-byte store per output pair (y[2n], y[2n + 1]): the pair must be one aligned pair of facet columns of every row
        const Map facet = facet_in_padded_facet(*h, facet_size, facet_off);
        if (facet_size & 1)
            return fail(SWIFTLY_ERR_UNSUPPORTED, "finish_facet_band_c2r: real facets out, half-length: odd facet size %lld", (long long)facet_size);
        if (facet.a & 1)
            return fail(SWIFTLY_ERR_UNSUPPORTED, "finish_facet_band_c2r: real facets out, half-length: the facet starts at an odd index of the padded row "
                        "(store offset %d, facet offset %lld)", facet.a, (long long)facet_off);
        if (out_row_stride & 1)
            return fail(SWIFTLY_ERR_UNSUPPORTED, "finish_facet_band_c2r: real facets out, half-length: odd output row stride %lld", (long long)out_row_stride);
        if (reinterpret_cast<uintptr_t>(out) & 7)
            return fail(SWIFTLY_ERR_UNSUPPORTED, "finish_facet_band_c2r: real facets out, half-length: output is not 8-byte aligned");
        if (in_row_stride < 0) return fail(SWIFTLY_ERR_PARAM, "finish_facet_band_c2r: negative input row stride");
        if (rows == 0) return 0;
        const hipStream_t st = (hipStream_t)stream;
        const Map band = band_as_load_map(*h, band_start, band_len);
        RowPassArgs r;
        std::memset(&r, 0, sizeof r);
        r.in = (const cx<float>*)in; r.out = (cx<float>*)out;
        r.in_pitch = in_row_stride; r.out_pitch = out_row_stride;
        r.out_real = 1;  // `out` points to float32, out_pitch counts real elements
        r.nrows = (int)rows;
        r.ld_a = band.a; r.ld_len = band.len; r.ld_c = band.c; r.ld_mod = band.mod;
        r.st_a = facet.a; r.st_len = facet.len; r.st_c = facet.c; r.st_mod = facet.mod;
        // the mask and the PSWF window of finish_facet as the ONE window the mapped store of the band row kernel takes
        r.st_win = (const float*)mask; r.st_win2 = h->invp_f + facet_lo(*h, facet_size);
        r.scale = 1.f;
        r.twc = compact_twiddles(h, h->log_yN - 1, 5);  // 32 points per lane of the half-length transform
        const cx<float>* twh = twiddles<float>(h, h->log_yN - 1);
        const cx<float>* twf = twiddles<float>(h, h->log_yN);
        if (!twh || !twf || !r.twc) return fail(SWIFTLY_ERR_HIP, "internal: missing twiddle tables");
        void* tmp = nullptr;
        if (int rc = single_store_window(r, st, &tmp)) return rc;
        const int e = launch_row_c2r_band(h->log_yN, r, twh, twf, st);
        if (tmp) (void)hipFreeAsync(tmp, st);
        if (e == -1) return fail(SWIFTLY_ERR_HIP, "internal: finish_facet_band_c2r: the half-length kernel does not take this call");
        return launch_status(e);
    }
    Batch bt{1, 0, 0, nullptr, 0};
    return DISPATCH(do_finish_facet, h, in, rows, in_row_stride, in_cs, out, out_row_stride, out_cs, facet_off, facet_size,
                    mask, bt, (hipStream_t)stream, band_start, band_len, real_out);
}

int swiftly_hip_finish_facet_band(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                  int64_t band_start, int64_t band_len, void* out, int64_t out_row_stride,
                                  int64_t facet_off, int64_t facet_size, const void* mask, void* stream) {
    return finish_facet_band_impl(B8Form::Complex, h, dtype, in, rows, in_row_stride, band_start, band_len, out, out_row_stride,
                                  facet_off, facet_size, mask, stream);
}
int swiftly_hip_finish_facet_band_real(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                       int64_t band_start, int64_t band_len, void* out, int64_t out_row_stride,
                                       int64_t facet_off, int64_t facet_size, const void* mask, void* stream) {
    return finish_facet_band_impl(B8Form::RealStore, h, dtype, in, rows, in_row_stride, band_start, band_len, out,
                                  out_row_stride, facet_off, facet_size, mask, stream);
}
int swiftly_hip_finish_facet_band_real64(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                         int64_t band_start, int64_t band_len, void* out, int64_t out_row_stride,
                                         int64_t facet_off, int64_t facet_size, const void* mask, void* stream) {
    return finish_facet_band_impl(B8Form::RealStore64, h, dtype, in, rows, in_row_stride, band_start, band_len, out,
                                  out_row_stride, facet_off, facet_size, mask, stream);
}
int swiftly_hip_finish_facet_band_c2r(swiftly_hip_t* h, int dtype, const void* in, int64_t rows, int64_t in_row_stride,
                                      int64_t band_start, int64_t band_len, void* out, int64_t out_row_stride,
                                      int64_t facet_off, int64_t facet_size, const void* mask, void* stream) {
    return finish_facet_band_impl(B8Form::HalfLengthReal, h, dtype, in, rows, in_row_stride, band_start, band_len, out,
                                  out_row_stride, facet_off, facet_size, mask, stream);
}


}  // extern "C"
