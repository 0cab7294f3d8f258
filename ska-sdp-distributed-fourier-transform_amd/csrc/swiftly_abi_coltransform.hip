// The strided-axis transform of the C ABI (col_transform) over the column-tile passes of col_pass.hip / swiftly_colpass.h:
// host code only.  Plan -> single pass, or lease the scratch -> chunked (K2, two streams) or plain schedule -> release.
#include <hip/hip_runtime.h>
#include "swiftly_abi_internal.h"
#include "swiftly_colaxis1.h"

ColZ plain_colz() {
    ColZ z;
    std::memset(&z, 0, sizeof z);
    z.nb = 1;
    return z;
}

int launch_col_checked(int lg, int mode, const ColPassArgs& args, const ColZ& cz, int outer, int nb, hipStream_t st,
                       const ColPassSrc2* src2) {
    return launch_status(launch_col_pass(lg, mode, args, cz, outer, nb, st, src2));
}

// Scratch handed down by an entry point for the duration of one ABI call on this host thread (the batch entry
// points have no workspace parameter): col_transform prefers it to a stream-ordered allocation.  Measured on
// MI355X: hipMallocAsync with a size that changes from call to call costs ~2 ms of HOST time per call (the pool
// does not reuse a smaller free block), which made a 25-wave pass host-bound.
thread_local void* t_call_ws = nullptr;
thread_local size_t t_call_ws_bytes = 0;

// What one call decides before it allocates or launches anything: the split, the precision of each stage and the tables.
struct ColPlan {
    bool two, c128, f64;
    int l1, l2, n1, n2;  // single pass: l1 = logn, l2 = 0
    size_t esz; uint64_t n;
    int f64_one, f64_a, f64_b;  // float64 arithmetic in the single pass / pass A / pass B
    const cx<float> *tw1, *tw2, *twf;  // lengths 2^l1, 2^l2, 2^logn (single pass: all three are the table of 2^logn)
    const cx<double> *twd1, *twd2, *twdf;
    int a_i_rows, a_o_rows, b_i_rows, b_o_rows;  // row factors of the intermediate
};
// The split, the range and the precision of each stage are col_split's (swiftly_rowroute.h; r3 bug behind its gather-sum
// rule: a 1024-point gather-sum transform ran the plain 32-column kernel, which read the encoded table as a row map); the
// tables are the handle's.  Returns -1 when the length is outside the column-pass range or a table is missing, else 0.
static int make_plan(const swiftly_hip* h, int logn, const ColPassArgs& c, int W, ColPlan& p) {
    const ColSplit s = col_split(logn, ColAsk{c.gs != 0, c.c128 != 0, c.f64 != 0, h->col_f64_stages}, W);
    if (s.status) return -1;
    p.c128 = c.c128 != 0;
    p.esz = p.c128 ? sizeof(cx<double>) : sizeof(cx<float>);
    p.two = s.two; p.l1 = s.l1; p.l2 = s.l2;
    p.n = uint64_t(1) << logn;
    p.n1 = 1 << p.l1; p.n2 = 1 << p.l2;
    p.f64 = s.f64; p.f64_one = s.f64_one; p.f64_a = s.f64_a; p.f64_b = s.f64_b;
    p.tw1 = twiddles<float>(h, p.l1);
    p.tw2 = p.two ? twiddles<float>(h, p.l2) : p.tw1;
    p.twf = p.two ? twiddles<float>(h, logn) : p.tw1;
    if (!p.tw1 || !p.tw2 || !p.twf) return -1;
    p.twd1 = p.f64 ? twiddles<double>(h, p.l1) : nullptr;
    p.twd2 = p.f64 && p.two ? twiddles<double>(h, p.l2) : p.twd1;
    p.twdf = p.f64 && p.two ? twiddles<double>(h, logn) : p.twd1;
    if (p.f64 && (!p.twd1 || !p.twd2 || !p.twdf)) return -1;
    // Layout of the intermediate (r4): row y2 * n1 + k1 -- a pass-A workgroup (one y2) WRITES n1 consecutive rows and a
    // pass-B workgroup (one k1) reads a comb -- instead of row k1 * n2 + y2 (comb written, consecutive rows read).  HBM
    // writes are the expensive direction on this chip (tools/mall_pipe.hip: a comb costs 7 % on the write side and nothing
    // on the read side): pass A 425 -> 395 us per wave as a pure copy, 427 -> 386 us for the kernel.
    constexpr bool y2_major = true;
    // (r5: a TILE-major scratch -- [item][64-column tile][row][64], the n1 rows of a pass-A workgroup one contiguous run
    // of n1 * 512 bytes -- measured the same within the run-to-run spread: 38.87 / 39.64 / 39.33 against 39.29 / 38.75 /
    // 38.58 ms per pass, interleaved on one box; not kept)
    p.a_i_rows = y2_major ? 1 : p.n2; p.a_o_rows = y2_major ? p.n1 : 1;  // pass A: row of (e = k1, o = y2)
    p.b_i_rows = y2_major ? p.n1 : 1; p.b_o_rows = y2_major ? 1 : p.n2;  // pass B: row of (i = y2, o = k1)
    return 0;
}
// The whole transform in one launch.  Sub-transform form: plain load, store at Q*k + j of the full length.
static int run_single(const ColPlan& p, ColPassArgs one, const ColZ& cz, int nb, hipStream_t st, int qmul, int qadd, int full_n) {
    one.tw = p.tw1; one.f64 = p.f64_one; one.twd = p.twd1; one.twd_full = p.twdf;
    if (qmul > 0) {
        one.full_logn = p.l1; one.full_n = full_n; one.ld_plain = 1; one.st_qmul = qmul; one.st_qadd = qadd;
        one.ld_mul = one.st_mul = 1;
    }
    return launch_col_checked(p.l1, 2, one, cz, 1, nb, st);
}
// pass A: length n1 over y1 (input index y1*n2 + y2), outer = y2: the load side of `c`, a plain store into the
// intermediate.  The schedule sets the column range, the output (slot or scratch, and its pitch) and scratch_nt.
static ColPassArgs pass_a_args(const ColPassArgs& c, const ColPlan& p) {
    ColPassArgs A = c;
    A.out_bdiv = 0; A.out_bs_hi = 0; A.ld_mul = p.n2;
    A.out_i_rows = p.a_i_rows; A.out_o_rows = p.a_o_rows;
    A.tw = p.tw1; A.tw_full = p.twf;
    A.f64 = p.f64_a; A.twd = p.twd1; A.twd_full = p.twdf;
    A.conj_st = 0; A.accumulate = 0; A.scale = 1.f;
    A.col_win = nullptr; A.st_rowmap = nullptr; A.st_win = nullptr; A.st_win2 = nullptr;
    return A;
}
// pass B: length n2 over y2, outer = k1; output index k1 + n1*k2: a plain load from the intermediate, the store side of
// `c`.  The schedule sets the column range, the input (slot or scratch, and its pitch) and scratch_nt.
static ColPassArgs pass_b_args(const ColPassArgs& c, const ColPlan& p) {
    ColPassArgs B = c;
    B.in_bdiv = 0; B.in_bs_hi = 0;
    B.in_i_rows = p.b_i_rows; B.in_o_rows = p.b_o_rows;
    B.ld_rowmap = nullptr; B.ld_win = nullptr; B.ld_win2 = nullptr; B.gs = 0;
    B.st_mul = p.n1; B.conj_ld = 0;
    B.tw = p.tw2; B.tw_full = p.twf;
    B.f64 = p.f64_b; B.twd = p.twd2; B.twd_full = p.twdf;
    return B;
}
static ColZ pass_b_colz(ColZ zb) {
    zb.flags &= ~(kZColGather | kZLoadB | kZLoadAF);  // the scratch is read plainly
    return zb;
}
// Chunked, two-stream form (r4; K2 = the gathered forward transform of several facets): the batch items are worked
// on in chunks of `zc` items x `Wc` columns whose two passes run back to back, chunks alternating between two
// internal streams, each stream re-using ONE chunk-sized slot of the scratch: pass A of one chunk (HBM reads, scratch
// writes) runs next to pass B of the other (scratch reads that can still hit the 256 MiB Infinity Cache).  Measured on
// the 64k workload (interleaved repeats on one box, gpurun_out/s3k, s3l): 40.7 -> 39.7 ms per pass with chunks of
// 2 facets x 256 columns (134 MB); 1 x 512: 40.0; 1 x 256, 4 x 128, 2 x 128, 3 x 256, 2 x 512: no gain or worse.  The
// gain is the overlap of the two kinds of pass, not cache residency: pure-copy stand-ins of the two passes bound it at
// 8 % of K2 (tools/mall_pipe.hip) -- the cache does not absorb the scratch WRITES.
// SWIFTLY_K2_CHUNK = "cols[,items]" | 0 (off) | unset: chunks of ~128 MB when the whole intermediate exceeds 256 MB.
// Whether this call runs chunked, and in which chunks: both slots have to fit into the `ws_bytes` of the caller's workspace.
static bool chunk_shape(const ColPlan& p, const ColPassArgs& c, const ColZ& cz, int W, int nb, int qmul, size_t scratch_bytes,
                        size_t ws_bytes, int& Wc, int& zc) {
    static const char* chunk_env = getenv("SWIFTLY_K2_CHUNK");
    int chunk_cols = chunk_env ? atoi(chunk_env) : -1;
    int chunk_items = (chunk_env && strchr(chunk_env, ',')) ? std::max(1, atoi(strchr(chunk_env, ',') + 1)) : 1;
    if (chunk_cols < 0) {  // automatic
        chunk_cols = 0;
        if (scratch_bytes > (size_t(256) << 20) && W >= 256) {
            chunk_cols = 256;
            chunk_items = (int)std::max<uint64_t>(1, (uint64_t(128) << 20) / (p.n * 256 * p.esz));
        }
    }
    if (!(chunk_cols >= 64 && (cz.flags & kZColGather) && !(cz.flags & kZColScatter) && !c.gs && qmul == 0 &&
          (nb > chunk_items || W > chunk_cols)))
        return false;
    Wc = std::min<int>((chunk_cols / 64) * 64, W);
    zc = std::min(chunk_items, nb);
    return 2 * (size_t)p.n * (size_t)Wc * (size_t)zc * p.esz <= ws_bytes;
}

struct ChunkEvents {  // fork + one join per chunk stream, destroyed when the call returns
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    ~ChunkEvents() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};
// (r5: three or four chunk streams instead of two -- 41.4-42.1 ms per pass against 38.9-39.8 with the default chunks,
// 39.5-39.7 against 39.1-39.3 with chunks of 1 facet x 256 columns; one stream: 41.7 -- two streams stay)
static int run_chunked(swiftly_hip* h, const ColPlan& p, const ColPassArgs& c, const ColZ& cz, int W, int nb, hipStream_t st,
                       void* scratch, int Wc, int zc) {
    const size_t slot_elems = (size_t)p.n * (size_t)Wc * (size_t)zc;
    hipError_t he = hipSuccess;
    {
        std::lock_guard<std::mutex> lock(h->chunk_mu);
        for (hipStream_t& s2 : h->chunk_st)
            if (!s2) {
                he = hipStreamCreateWithFlags(&s2, hipStreamNonBlocking);
                if (he != hipSuccess) return fail(SWIFTLY_ERR_HIP, "hipStreamCreateWithFlags: %s", hipGetErrorString(he));
            }
    }
    // (events are per call: two host threads may drive the same handle on different streams)
    ChunkEvents events;
    hipEvent_t* const ev = events.ev;
    for (hipEvent_t& e : events.ev)
        if ((he = hipEventCreateWithFlags(&e, hipEventDisableTiming)) != hipSuccess) {
            e = nullptr;
            return fail(SWIFTLY_ERR_HIP, "hipEventCreateWithFlags: %s", hipGetErrorString(he));
        }
    // fork: the chunk streams start behind everything queued on `st` (a failed record / wait would let them
    // run ahead of the producer of the input: nothing has been launched yet, so just report it)
    // (swiftly_hip_chain_chunk_streams: the caller vouches for the inputs; the chunk streams run on from the chunks
    // of the previous call -- no pipeline drain and no idle event hops between consecutive waves, r5)
    // (a chained call still forks when the un-chunked path has used THIS workspace since the last fork)
    void* plain_ws = scratch;
    const bool plain_pending = h->ws_plain_pending.compare_exchange_strong(plain_ws, nullptr);
    if (!g_chain_chunk_streams || plain_pending) {
        he = hipEventRecord(ev[0], st);
        for (hipStream_t s2 : h->chunk_st)
            if (he == hipSuccess) he = hipStreamWaitEvent(s2, ev[0], 0);
    }
    if (he != hipSuccess) return fail(SWIFTLY_ERR_HIP, "chunked four-step, fork: %s", hipGetErrorString(he));
    const ColPassArgs A0 = pass_a_args(c, p), B0 = pass_b_args(c, p);
    const ColZ zb = pass_b_colz(cz);
    int rc = 0, i = 0;
    for (int z0 = 0; z0 < nb && !rc; z0 += zc) {
        const int nz = std::min(zc, nb - z0);
        for (int c0 = 0; c0 < W && !rc; c0 += Wc, i++) {
            const int wc = std::min(Wc, W - c0);
            hipStream_t s2 = h->chunk_st[i & 1];
            // item z of the launch sits at slot + (z - z0) * n * Wc (raw_z0: the kernels address the scratch
            // with the item index relative to the launch's first item)
            cx<float>* slot = cx_at(scratch, (long long)((size_t)(i & 1) * slot_elems), p.c128);
            ColPassArgs A = A0;  // the chunk's columns through col0 (`in` unchanged; behind the caller's first column), into the chunk's slot; `cz` as given
            A.scratch_nt = 0;
            A.ncols = wc; A.col0 = c.col0 + c0; A.z0 = z0; A.raw_z0 = z0;
            A.out = slot; A.out_pitch = (unsigned)Wc; A.out_bs = (long long)(p.n * Wc);
            rc = launch_col_checked(p.l1, 0, A, cz, p.n2, nz, s2);
            if (rc) break;
            ColPassArgs B = B0;  // the slot from its column 0; the output and its column window advanced by c0
            B.scratch_nt = 0;
            B.ncols = wc; B.col0 = 0; B.z0 = z0; B.raw_z0 = z0;
            B.in = slot; B.in_pitch = (unsigned)Wc; B.in_bs = (long long)(p.n * Wc);
            B.out = cx_at(c.out, c0, p.c128);
            if (B.col_win) B.col_win += p.c128 ? 2 * c0 : c0;  // (double table with complex128 storage)
            rc = launch_col_checked(p.l2, 1, B, zb, p.n1, nz, s2);
        }
    }
    // join: `st` continues behind both chunk streams.  If the join cannot be queued, the consumer of the output
    // on `st` must not start early: wait for the chunk streams on the host instead
    for (int k = 0; k < 2; k++) {
        he = hipEventRecord(ev[1 + k], h->chunk_st[k]);
        if (he == hipSuccess) he = hipStreamWaitEvent(st, ev[1 + k], 0);
        if (he != hipSuccess) {
            (void)hipStreamSynchronize(h->chunk_st[k]);
            if (!rc) rc = fail(SWIFTLY_ERR_HIP, "chunked four-step, join: %s", hipGetErrorString(he));
        }
    }
    return rc;
}
// Both passes over all `W` columns and `nb` items on the caller's stream, through the scratch [nb][N][W].
static int run_plain(const ColPlan& p, const ColPassArgs& c, const ColZ& cz, int W, int nb, hipStream_t st, void* scratch,
                     size_t scratch_bytes, int qmul, int qadd, int full_n) {
    // scratch accesses: a small intermediate is left cacheable so that pass B finds it in the 256 MiB Infinity
    // Cache (measured: the 160 MB of a K5b wave, K3-5 12.5 -> 11.6 ms per pass); a large one is streamed
    // non-temporally (measured: K2, 1.2 GB per wave, 18.5 ms vs 19.6 ms cacheable).
    const int scratch_nt = scratch_bytes > (size_t(192) << 20) ? 1 : 0;
    const int logn = p.l1 + p.l2;
    ColPassArgs A = pass_a_args(c, p);
    A.scratch_nt = scratch_nt; A.ncols = W;
    // scratch row width = W (column slabs that keep the intermediate cache-sized: no gain, r2-r4)
    A.out = (cx<float>*)scratch; A.out_pitch = (unsigned)W; A.out_bs = (long long)(p.n * W);
    if (qmul > 0) { A.full_logn = logn; A.full_n = 0; A.ld_plain = 1; A.st_qmul = 0; }
    ColZ za = cz;
    za.flags &= ~kZColScatter;  // the scratch is written plainly
    if (int rc = launch_col_checked(p.l1, 0, A, za, p.n2, nb, st)) return rc;
    ColPassArgs B = pass_b_args(c, p);
    B.scratch_nt = scratch_nt; B.ncols = W;
    B.in = (const cx<float>*)scratch; B.in_pitch = (unsigned)W; B.in_bs = (long long)(p.n * W);
    if (qmul > 0) { B.full_logn = logn; B.full_n = full_n; B.st_qmul = qmul; B.st_qadd = qadd; }
    return launch_col_checked(p.l2, 1, B, pass_b_colz(cz), p.n1, nb, st);
}

// Strided-axis transform of length 2^logn over `W` adjacent columns and `nb` batch items with the column-tile
// passes: one pass up to 512 points, otherwise four-step (N = n1*n2, input index y = y1*n2 + y2, output index
// k = k1 + n1*k2) through a stream-ordered scratch [nb][N][W]:
//   pass A (length n1 over y1, one per y2): scratch[k1*n2 + y2] = W_N^(y2 k1) * sum_y1 x[y1 n2 + y2] W_n1^(y1 k1)
//   pass B (length n2 over y2, one per k1): X[k1 + n1 k2]       = sum_y2 scratch[k1*n2 + y2] W_n2^(y2 k2)
// `c` carries the load / store maps, windows, conjugation flags, scale, batch strides, column gather and row
// maps of the whole transform; in/out pitches and pointers are given separately.  Returns -1 when the length
// is outside the column-pass range (col_split, swiftly_rowroute.h: the row primitives ask it before they come here), else
// a status code.
// Sub-transform form (qmul = Q > 0, swiftly_mixed.h): the input is the plain scratch of the radix-Q pass (element y of
// the length-2^logn sub-transform j = qadd at row y of `c.in`), the store map of `c` refers to the full length full_n
// with plain output index Q*k + j.
int col_transform(swiftly_hip* h, int logn, const ColPassArgs& c, const ColZ& cz, int W, int nb, hipStream_t st, void* ws,
                  size_t ws_bytes, int qmul, int qadd, int full_n) {
    if (!ws && t_call_ws) { ws = t_call_ws; ws_bytes = t_call_ws_bytes; }
    ColPlan p;
    if (make_plan(h, logn, c, W, p)) return -1;
    if (!p.two) return run_single(p, c, cz, nb, st, qmul, qadd, full_n);
    const size_t scratch_bytes = (size_t)nb * p.n * (size_t)W * p.esz;
    // caller-provided workspace (deterministic; the stream-ordered pool reuses memory across STREAMS only
    // opportunistically, which made the two-stream schedule fall back to fresh multi-GB allocations on some runs)
    ScratchLease lease;
    if (int rc = lease.acquire(ws, ws_bytes, scratch_bytes, st, "hipMallocAsync(two-pass scratch)")) return rc;
    int Wc, zc;  // (the chunked schedule needs the caller's workspace)
    if (chunk_shape(p, c, cz, W, nb, qmul, scratch_bytes, lease.own ? 0 : ws_bytes, Wc, zc))
        return lease.release(run_chunked(h, p, c, cz, W, nb, st, lease.p, Wc, zc));
    if (!lease.own) h->ws_plain_pending.store(lease.p);  // `ws` is written on `st` below: a later chained chunked call has to wait for it
    return lease.release(run_plain(p, c, cz, W, nb, st, lease.p, scratch_bytes, qmul, qadd, full_n));
}

// K2 with the contiguous-axis finish inside the first pass of its four-step (swiftly_colaxis1.h): pass A' of `x` over `nb`
// facets into the scratch [nb][yN][m], then pass B -- the store side of `c`, as col_transform runs it, with n1 = 16384 / m
// instead of col_split's halves -- both on the caller's stream and in float32.  Returns -1 without launching anything when
// (yN, m) has no instance, else a status code.
int col_transform_axis1(swiftly_hip* h, const ColPassArgs& c, const ColZ& cz, ColAxis1Args x, int nb, hipStream_t st, void* ws,
                        size_t ws_bytes) {
    if (!col_axis1_instance(h->log_yN, h->log_m)) return -1;
    const int m = (int)h->m;
    ColPlan p{};
    p.two = true;
    p.l1 = kColAxis1LogTile - h->log_m; p.l2 = h->log_yN - p.l1;
    p.n1 = 1 << p.l1; p.n2 = 1 << p.l2;
    p.esz = sizeof(cx<float>); p.n = (uint64_t)h->yN;
    p.tw2 = twiddles<float>(h, p.l2); p.twf = twiddles<float>(h, h->log_yN);
    if (!p.tw2 || !p.twf) return fail(SWIFTLY_ERR_HIP, "internal: missing twiddle table");
    p.b_i_rows = p.n1; p.b_o_rows = 1;  // the intermediate of make_plan: row y2 * n1 + k1
    const size_t scratch_bytes = (size_t)nb * p.n * (size_t)m * p.esz;
    ScratchLease lease;
    if (int rc = lease.acquire(ws, ws_bytes, scratch_bytes, st, "hipMallocAsync(two-pass scratch)")) return rc;
    if (!lease.own) h->ws_plain_pending.store(lease.p);  // (as col_transform's plain schedule: `ws` is written on `st`)
    const int scratch_nt = scratch_bytes > (size_t(192) << 20) ? 1 : 0;  // (run_plain)
    x.out = (cx<float>*)lease.p; x.out_fs = (long long)(p.n * (uint64_t)m); x.scratch_nt = scratch_nt; x.tw_full = p.twf;
    int rc = launch_status(launch_col_axis1(h->log_yN, h->log_m, x, nb, st), "axis-1 pass A'", "no instance");
    if (!rc) {
        ColPassArgs B = pass_b_args(c, p);
        B.scratch_nt = scratch_nt; B.ncols = m;
        B.in = (const cx<float>*)lease.p; B.in_pitch = (unsigned)m; B.in_bs = x.out_fs;
        rc = launch_col_checked(p.l2, 1, B, pass_b_colz(cz), p.n1, nb, st);
    }
    return lease.release(rc);
}
