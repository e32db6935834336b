// lzx_multi.hip -- batched, independent Lanczos: b <= 16 separate three-term recurrences (one per column of X) that share
// one SpMM per iteration (include/lzx.h: lzx_lanczos_multi_f64, lzx_multout_multi_f64, lzx_spmm_f64, lzx_multi_release), and
// the stochastic-trace entries built on it (lzx_probes_f64, lzx_lanczos_probes_f64, lzx_probe_diag_f64).
//
// Not block Lanczos: no QR of a block, no coupling between columns.  Each column runs serial/lib/lanczos.cc:9-56 (the
// arithmetic of lzx_lanczos_f64) plus a breakdown stop of its own.
//
// Layout.  Working vectors are vertex-major and interleaved, [n][B] fp64, B = the batch width padded to 2, 4, 8 or 16: one
// vertex's values are 16-128 bytes, so one gathered row of X fills at most one 128-byte line, and one col_idx read serves all
// B columns.  The path works on the caller-order CSR the handle keeps (d_row_ptr / d_col_idx); the sliced-ELL and
// propagation-blocked tables of the single-vector path are neither used nor touched.  Padded columns start as zero vectors
// and stop at iteration 0.
//
// One iteration is four launches:
//   k_multi_spmm    V = A Q_j.  A wavefront serves 64 / B segments of the work list, lane (segment, column); a segment is a
//                   whole row or an L-entry chunk of a longer row, summed with ONE accumulator in ascending CSR order (a row
//                   that is not split comes out bit-identical to serial/lib/SPMV.cc:19-28).  The work list is sorted by
//                   length, longest first, so the lanes of a wavefront carry about the same number of entries.
//   k_multi_alpha   the chunk totals of split rows added in chunk order into V, and per-(row segment, column) partials of
//                   alpha_c = v_c . q_{j,c}
//   k_multi_update  every workgroup closes alpha from the partials (fixed order); u = v - alpha q_j - beta_{j-1} q_{j-1} (two
//                   rounded updates, as serial/); partials of ||u||^2
//   k_multi_scale   every workgroup closes beta; breakdown stop; q_{j+1} = u / beta into the basis
// Reductions: a row segment of LZX_MULTI_SEG rows yields one partial per column.  Inside it, runs of LZX_MULTI_RUN rows are
// summed left to right by one thread, the runs' totals by a fixed wavefront tree; the segments' partials are closed
// by the fixed-order block sum of lzx_reduce.h's shape.  Nothing in that shape depends on B, on b or on the column's place in
// X, so a column's alpha, beta, basis and answer are bit-identical whatever else is in the batch.
//
// Breakdown (decided on the device, per column): after beta_{c,j} (j < k - 1) the column stops when
//   beta_{c,j} <= 2^-40 * max_{i <= j} (|alpha_{c,i}| + beta_{c,i-1}),   beta_{c,-1} = 0.
// Its beta_j is then stored as 0 and its later basis vectors are zero, so its later alpha / beta come out 0; "stopped before
// iteration j" is read from beta_{c,j-1} == 0, which every workgroup of a later launch sees complete -- no flag round trip.
//
// Probes (lzx_lanczos_probes_f64).  q_0 is written on the device by k_multi_probe from a counter hash of (seed, probe, vertex)
// -- no host upload.  Basis-free ("ring") runs keep q_{j-1}, q_j, q_{j+1} in three rotating [n][B] slots instead of the
// [k][n][B] basis: the same four launches on other pointers, so alpha / beta / k_used are those of the kept-basis run.  On a
// kept probe basis k_multi_diag forms sum_c z_c (Q_c t_c) per row, so one vector of n leaves the device per batch.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "lzx_internal.h"
#include "lzx_spmv_body.h"
#include "lzx_reduce.h"
#include "lzx_multi_shared.h"

template <typename T>
static void mfree(T *&p)
{
    if (p) (void)hipFree(p);
    p = nullptr;
}

template <typename T>
static int malloc_n(T **p, u64 count, const char *what)
{
    *p = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(p), sizeof(T) * std::max<u64>(count, 1));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        lzx_set_error("batched Lanczos: allocation of %llu bytes (%s) failed: %s", (unsigned long long)(sizeof(T) * count), what,
                      hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? LZX_ERR_NOMEM : LZX_ERR_HIP;
    }
    return LZX_OK;
}

void lzx_multi_free_work(lzx_multi_state *m)
{
    mfree(m->d_V); mfree(m->d_X); mfree(m->d_part); mfree(m->d_pa); mfree(m->d_pn);
    m->wB = 0;
}

static void free_basis(lzx_multi_state *m)
{
    mfree(m->d_Q); mfree(m->d_alpha); mfree(m->d_beta); mfree(m->d_T); mfree(m->d_mx); mfree(m->d_kused);
    m->B = m->b = m->k = 0;
    m->resident = m->ring = m->probe = false;
    m->h_kused.clear();
}

void lzx_multi_free(lzx_ctx *c, bool with_tables)
{
    lzx_multi_state *m = c->multi;
    if (!m) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    free_basis(m);
    lzx_multi_free_work(m);
    if (!with_tables) return;
    mfree(m->d_wl); mfree(m->d_split_row); mfree(m->d_split_first); mfree(m->d_run_split);
    for (hipEvent_t e : m->ev) (void)hipEventDestroy(e);
    delete m;
    c->multi = nullptr;
}

// ==================================================================================================== kernels

// out [n][B]: column c < b is probe first + c divided by div (sqrt(n) for a start vector, 1 for lzx_probes_f64); padded columns 0
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK) k_multi_probe(u64 seed, u64 first, u32 b, u64 n, double div, double *out)
{
    const u64 i = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x;
    if (i >= n * B) return;
    const u32 c = (u32)(i % B);
    out[i] = c < b ? lzx_probe_value(seed, first + c, i / B) / div : 0.0;
}

// alpha_c closed from pa by every workgroup; u = v - alpha q_j - beta_{j-1} q_{j-1} in place of v; partials of ||u||^2.
// A column that stopped before iteration j (beta_{c,j-1} == 0) has alpha = 0 and u = 0.  last: alpha only (grid of one).
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK)
k_multi_update(double *V, const double *__restrict__ Qj, const double *__restrict__ Qjm1, const double *pa, u32 n_seg,
               double *alpha, const double *beta, u32 k, u32 j, double *pn, u64 n, int last)
{
    __shared__ double sh[LZX_MULTI_RUNS * B];
    __shared__ double shw[4 * B], sa[B], sb[B];
    __shared__ int sstop[B];
    close_cols<B>(pa, n_seg, shw, sa);
    if (threadIdx.x < B) {
        const u32 c = threadIdx.x;
        const double bp = j > 0 ? beta[(u64)c * k + j - 1] : 0.0;
        const int stop = j > 0 && bp == 0.0;
        if (stop) sa[c] = 0.0;
        sb[c] = bp;
        sstop[c] = stop;
        if (blockIdx.x == 0) alpha[(u64)c * k + j] = sa[c];
    }
    __syncthreads();
    if (last) return;
    for (u32 seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
        for (u32 u = threadIdx.x; u < LZX_MULTI_RUNS * B; u += LZX_MULTI_BLOCK) {
            const u32 run = u / B, c = u % B;
            const u64 r0 = (u64)seg * LZX_MULTI_SEG + (u64)run * LZX_MULTI_RUN;
            const u64 r1 = std::min<u64>(r0 + LZX_MULTI_RUN, n);
            const double a = sa[c], bp = sb[c];
            const int stop = sstop[c];
            double s = 0.0;
            u64 r = r0;
            // eight rows' loads in flight, then the same operations row by row
            for (; r + 8 <= r1; r += 8) {
                double w[8], q[8], p[8];
#pragma unroll
                for (u32 t = 0; t < 8; ++t) {
                    w[t] = V[(r + t) * B + c];
                    q[t] = Qj[(r + t) * B + c];
                    p[t] = j > 0 ? Qjm1[(r + t) * B + c] : 0.0;
                }
#pragma unroll
                for (u32 t = 0; t < 8; ++t) {
                    w[t] -= a * q[t];
                    if (j > 0) w[t] -= bp * p[t];
                    if (stop) w[t] = 0.0;
                    V[(r + t) * B + c] = w[t];
                    s += w[t] * w[t];
                }
            }
            for (; r < r1; ++r) {
                const u64 i = r * B + c;
                double w = V[i];
                w -= a * Qj[i];
                if (j > 0) w -= bp * Qjm1[i];
                if (stop) w = 0.0;
                V[i] = w;
                s += w * w;
            }
            sh[u] = s;
        }
        seg_partials<B>(sh, pn + (u64)seg * B);
    }
}

// beta_c = sqrt(closed ||u||^2); the breakdown stop; q_{j+1} = u / beta_c (0 for a column that stopped).  Workgroup 0 stores
// beta_{c,j} and the running max of |alpha_i| + beta_{i-1} for iteration j (read at j + 1: other slots, no race).
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK)
k_multi_scale(const double *__restrict__ V, const double *pn, u32 n_seg, const double *alpha, double *beta, double *mx, u32 k, u32 j,
              double *Qn, u64 n, double lstop)
{
    __shared__ double shw[4 * B], sq[B], sd[B];
    close_cols<B>(pn, n_seg, shw, sq);
    if (threadIdx.x < B) {
        const u32 c = threadIdx.x;
        double bt = sqrt(sq[c]);
        const double bp = j > 0 ? beta[(u64)c * k + j - 1] : 0.0;
        const double m = fmax(j > 0 ? mx[(u64)(j - 1) * B + c] : 0.0, fabs(alpha[(u64)c * k + j]) + bp);
        // lstop >= 0 (operator L): the single-vector rule, beta <= 2^-40 * 2 d_max
        const bool stop = (j > 0 && bp == 0.0) || (lstop >= 0.0 ? bt <= lstop : bt <= 0x1p-40 * m);
        if (stop) bt = 0.0;
        sd[c] = bt;
        if (blockIdx.x == 0) {
            beta[(u64)c * k + j] = bt;
            mx[(u64)j * B + c] = m;
        }
    }
    __syncthreads();
    const u64 total = n * B;
    for (u64 i = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x; i < total; i += (u64)gridDim.x * LZX_MULTI_BLOCK) {
        const double d = sd[i % B];
        Qn[i] = d == 0.0 ? 0.0 : V[i] / d;
    }
}

// (Q_c t_c)[r] at i = r * B + c: sum over j < min(k, k_used[c]) of T[c][j] q_{j,c}[r], j ascending.  The one expression
// k_multi_multout and k_multi_diag share, so the diagonal's y_c is the answer's bit for bit.
template <u32 B>
__device__ __forceinline__ double multout_entry(const double *__restrict__ Q, u32 k, u64 n, const double *__restrict__ T,
                                                const u32 *__restrict__ kused, u64 i)
{
    const u32 c = (u32)(i % B);
    const u32 kc = std::min(k, kused[c]);
    double acc = 0.0;
    for (u32 j = 0; j < kc; ++j) acc += T[(u64)c * k + j] * Q[(u64)j * n * B + i];
    return acc;
}

// out[r][c] = (Q_c t_c)[r]
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK)
k_multi_multout(const double *__restrict__ Q, u32 k, u64 n, const double *__restrict__ T, const u32 *__restrict__ kused, double *out)
{
    const u64 i = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x;
    if (i >= n * B) return;
    out[i] = multout_entry<B>(Q, k, n, T, kused, i);
}

// out[r] = sum over c < b, ascending, of z_c[r] (Q_c t_c)[r] on a probe basis.  z_c[r] = the sign of q_{0,c}[r] (= z / sqrt(n),
// never 0), so the product is exact.  A workgroup holds 256 / B whole rows: the (row, column) products are staged in LDS and
// the row's column-0 thread adds them in column order.
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK)
k_multi_diag(const double *__restrict__ Q, u32 k, u64 n, u32 b, const double *__restrict__ T, const u32 *__restrict__ kused, double *out)
{
    static_assert(LZX_MULTI_BLOCK % B == 0, "rows do not straddle workgroups");
    __shared__ double sh[LZX_MULTI_BLOCK];
    const u64 i = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x;
    const u32 c = threadIdx.x % B;
    const bool in = i < n * B;
    double p = 0.0;
    if (in && c < b) {
        const double y = multout_entry<B>(Q, k, n, T, kused, i);
        p = Q[i] > 0.0 ? y : -y;
    }
    sh[threadIdx.x] = p;
    __syncthreads();
    if (in && c == 0) {
        double s = 0.0;
        for (u32 cc = 0; cc < b; ++cc) s += sh[threadIdx.x + cc];
        out[i / B] = s;
    }
}

// ==================================================================================================== host side
u32 lzx_multi_pad_width(u32 b) { return b <= 2 ? 2 : b <= 4 ? 4 : b <= 8 ? 8 : 16; }

int lzx_multi_check_handle(lzx_ctx *c, const char *fn)
{
    if (c->comm_kind != 0 || c->world > 1)
        LZX_FAIL(LZX_ERR_STATE, "%s: the batched path runs on one GPU handle; this handle is rank %d of a communicator of %d", fn, c->rank, c->world);
    if (!c->d_row_ptr || !c->d_v) LZX_FAIL(LZX_ERR_STATE, "%s: no graph has been handed over", fn);
    if (c->n >= LZX_MULTI_PART) LZX_FAIL(LZX_ERR_LIMIT, "%s: %llu vertices (the batched path takes fewer than 2^31)", fn, (unsigned long long)c->n);
    if (!c->multi) {
        c->multi = new (std::nothrow) lzx_multi_state;
        if (!c->multi) LZX_FAIL(LZX_ERR_NOMEM, "%s: host allocation failed", fn);
    }
    LZX_HIP(hipSetDevice(c->device));
    return LZX_OK;
}

// The work list, once per graph: every row of at most L entries is one segment, a longer row ceil(len / L) chunks of L
// entries (the last one shorter) whose totals go to slots of d_part; all segments stably sorted by length, longest first.
int lzx_multi_build_tables(lzx_ctx *c)
{
    lzx_multi_state *m = c->multi;
    const u32 L = c->multi_chunk_opt > 0 ? (u32)std::min<int64_t>(c->multi_chunk_opt, 1 << 30) : LZX_MULTI_CHUNK;
    if (m->d_wl && m->chunk == L) return LZX_OK;
    mfree(m->d_wl); mfree(m->d_split_row); mfree(m->d_split_first); mfree(m->d_run_split);
    const u64 n = c->n;
    std::vector<u64> rp(n + 1);
    LZX_HIP(hipMemcpy(rp.data(), c->d_row_ptr, sizeof(u64) * (n + 1), hipMemcpyDeviceToHost));
    std::vector<u32> split_row, split_first(1, 0);
    std::vector<u64> count(L + 2, 0);   // segments per length
    u64 segs = 0;
    for (u64 r = 0; r < n; ++r) {
        const u64 len = rp[r + 1] - rp[r];
        if (len <= L) {
            ++count[len];
            ++segs;
            continue;
        }
        const u64 nch = (len + L - 1) / L;
        if ((u64)split_first.back() + nch >= LZX_MULTI_PART) LZX_FAIL(LZX_ERR_LIMIT, "batched SpMM: too many row chunks");
        split_row.push_back((u32)r);
        split_first.push_back(split_first.back() + (u32)nch);
        count[L] += nch - 1;
        ++count[len - (nch - 1) * L];
        segs += nch;
    }
    // bucket offsets, longest first
    std::vector<u64> at(L + 2, 0);
    u64 acc = 0;
    for (u64 len = L + 1; len-- > 0;) { at[len] = acc; acc += count[len]; }
    const u64 n_wl = (segs + 31) / 32 * 32;
    std::vector<uint4> wl(std::max<u64>(n_wl, 1), make_uint4(0, 0, 0, LZX_MULTI_PAD));
    auto put = [&](u64 beg, u32 len, u32 dst) { wl[at[len]++] = make_uint4((u32)beg, (u32)(beg >> 32), len, dst); };
    u32 ks = 0;
    for (u64 r = 0; r < n; ++r) {
        const u64 len = rp[r + 1] - rp[r];
        if (len <= L) { put(rp[r], (u32)len, (u32)r); continue; }
        for (u32 p = split_first[ks]; p < split_first[ks + 1]; ++p) {
            const u64 off = (u64)(p - split_first[ks]) * L;
            put(rp[r] + off, (u32)std::min<u64>(L, len - off), p | LZX_MULTI_PART);
        }
        ++ks;
    }
    const u64 runs = (n + LZX_MULTI_RUN - 1) / LZX_MULTI_RUN;
    std::vector<u32> run_split(runs + 1);
    {
        u32 s = 0;
        for (u64 q = 0; q <= runs; ++q) {
            while (s < split_row.size() && split_row[s] < q * LZX_MULTI_RUN) ++s;
            run_split[q] = s;
        }
    }
    m->n_split = (u32)split_row.size();
    m->n_parts = split_first.back();
    m->n_wl = n_wl;
    m->n_seg = (u32)((n + LZX_MULTI_SEG - 1) / LZX_MULTI_SEG);
    int rc;
    if ((rc = malloc_n(&m->d_wl, wl.size(), "work list")) || (rc = malloc_n(&m->d_split_row, std::max<size_t>(split_row.size(), 1), "split rows")) ||
        (rc = malloc_n(&m->d_split_first, split_first.size(), "split rows")) || (rc = malloc_n(&m->d_run_split, run_split.size(), "split rows"))) {
        mfree(m->d_wl); mfree(m->d_split_row); mfree(m->d_split_first); mfree(m->d_run_split);
        return rc;
    }
    LZX_HIP(hipMemcpy(m->d_wl, wl.data(), sizeof(uint4) * wl.size(), hipMemcpyHostToDevice));
    if (!split_row.empty()) LZX_HIP(hipMemcpy(m->d_split_row, split_row.data(), sizeof(u32) * split_row.size(), hipMemcpyHostToDevice));
    LZX_HIP(hipMemcpy(m->d_split_first, split_first.data(), sizeof(u32) * split_first.size(), hipMemcpyHostToDevice));
    LZX_HIP(hipMemcpy(m->d_run_split, run_split.data(), sizeof(u32) * run_split.size(), hipMemcpyHostToDevice));
    m->chunk = L;
    return LZX_OK;
}

// What the builder above counted, read-only, for lzx_test_get_shape (tests/multi_model.py restates the rules): every name is 0
// until the tables exist, that is until the first batched call on the graph.
bool lzx_multi_shape(const lzx_ctx *c, const char *name, int64_t *value)
{
    const lzx_multi_state *m = c->multi;
    const bool built = m && m->d_wl;
    if (!strcmp(name, "multi_chunk")) *value = built ? m->chunk : 0;
    else if (!strcmp(name, "multi_work_items")) *value = built ? (int64_t)m->n_wl : 0;
    else if (!strcmp(name, "multi_split_rows")) *value = built ? m->n_split : 0;
    else if (!strcmp(name, "multi_chunk_slots")) *value = built ? m->n_parts : 0;
    else if (!strcmp(name, "multi_row_segments")) *value = built ? m->n_seg : 0;
    // the grid of k_multi_update and of k_multi_alpha's launch
    else if (!strcmp(name, "multi_vector_grid")) *value = built ? std::min<u32>(std::max<u32>(m->n_seg, 1), (u32)c->cu_count * 4) : 0;
    else return false;
    return true;
}

// the work vectors of width B; need_x: the second one too (packing, unpacking -- a probe run starts on the device without it)
int lzx_multi_ensure_work(lzx_ctx *c, u32 B, bool need_x)
{
    lzx_multi_state *m = c->multi;
    const u64 n = c->n;
    int rc;
    if (m->wB != B || !m->d_V) {
        lzx_multi_free_work(m);
        if ((rc = malloc_n(&m->d_V, n * B, "work vector")) || (rc = malloc_n(&m->d_part, (u64)m->n_parts * B, "chunk totals")) ||
            (rc = malloc_n(&m->d_pa, (u64)m->n_seg * B, "partials")) || (rc = malloc_n(&m->d_pn, (u64)m->n_seg * B, "partials"))) {
            lzx_multi_free_work(m);
            return rc;
        }
        m->wB = B;
    }
    if (need_x && !m->d_X && (rc = malloc_n(&m->d_X, n * B, "work vector"))) {
        lzx_multi_free_work(m);
        return rc;
    }
    return LZX_OK;
}

// The batch basis of k vectors, or (ring) three rotating slots; any other basis is given back first.
static int ensure_basis(lzx_ctx *c, u32 k, u32 B, bool ring, const char *fn)
{
    lzx_multi_state *m = c->multi;
    m->resident = m->probe = false;
    if (m->d_Q && m->k == k && m->B == B && m->ring == ring) return LZX_OK;
    free_basis(m);
    const u32 slots = ring ? 3 : k;
    const u64 bytes = (u64)slots * c->n * B * sizeof(double);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && bytes > (u64)total_b) {
        lzx_multi_free_work(m);
        LZX_FAIL(LZX_ERR_NOMEM, "%s: the batch basis needs %llu bytes (k = %u x n = %llu x B = %u x 8), the device has %llu", fn,
                 (unsigned long long)bytes, slots, (unsigned long long)c->n, B, (unsigned long long)total_b);
    }
    (void)hipGetLastError();
    int rc;
    if ((rc = malloc_n(&m->d_Q, (u64)slots * c->n * B, "batch basis")) || (rc = malloc_n(&m->d_alpha, (u64)B * k, "coefficients")) ||
        (rc = malloc_n(&m->d_beta, (u64)B * k, "coefficients")) || (rc = malloc_n(&m->d_T, (u64)B * k, "coefficients")) ||
        (rc = malloc_n(&m->d_mx, (u64)k * B, "coefficients")) || (rc = malloc_n(&m->d_kused, B, "coefficients"))) {
        free_basis(m);
        lzx_multi_free_work(m);
        if (rc == LZX_ERR_NOMEM)
            lzx_set_error("%s: the batch basis needs %llu bytes (k = %u x n = %llu x B = %u x 8) and does not fit", fn,
                          (unsigned long long)bytes, slots, (unsigned long long)c->n, B);
        return rc;
    }
    m->k = k;
    m->B = B;
    m->ring = ring;
    return LZX_OK;
}

// where the start vectors come from: the caller's X0, or probes first .. first + b - 1 of seed
struct MultiStart {
    const double *X0;
    u64 seed, first;
};

template <u32 B>
static int multi_loop(lzx_ctx *c, u32 b, MultiStart start, bool ring, u32 k, double *alpha, double *beta, uint32_t *k_used,
                      double *x_norm, double *Q, lzx_stats *stats, const char *fn)
{
    lzx_multi_state *m = c->multi;
    const u64 n = c->n, nB = n * B;
    const double *X0 = start.X0;
    // ||x_c||: left-to-right sum of squares, then sqrt (serial/lib/lanczos.cc:155-161), as lzx_lanczos_prepare_f64 forms it
    MultiDiv div{};
    for (u32 col = 0; col < 16; ++col) div.v[col] = 1.0;
    for (u32 col = 0; X0 && col < b; ++col) {
        double s = 0.0;
        const double *x = X0 + (u64)col * n;
        for (u64 i = 0; i < n; ++i) s += x[i] * x[i];
        div.v[col] = std::sqrt(s);
        x_norm[col] = div.v[col];
    }
    int rc = ensure_basis(c, k, B, ring, fn);
    if (rc == LZX_OK) rc = lzx_multi_ensure_work(c, B, X0 != nullptr);
    if (rc != LZX_OK) {   // nothing half-built is left behind
        free_basis(m);
        lzx_multi_free_work(m);
        return rc;
    }
    if (ring) mfree(m->d_X);   // the state is the three slots and V
    if (X0) {
        // x0 staged in the work vector as [b][n], packed into column 0 of the basis
        LZX_HIP(hipMemcpyAsync(m->d_V, X0, sizeof(double) * b * n, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_multi_pack<B>, dim3(grid_of(nB)), dim3(LZX_MULTI_BLOCK), 0, c->stream, m->d_V, b, n, div, m->d_Q);
    } else {
        // a +-1 probe has the norm sqrt(n) exactly: the left-to-right sum of n ones
        hipLaunchKernelGGL(k_multi_probe<B>, dim3(grid_of(nB)), dim3(LZX_MULTI_BLOCK), 0, c->stream, start.seed, start.first, b, n,
                           std::sqrt((double)n), m->d_Q);
    }
    LZX_HIP(hipGetLastError());
    // q_j: basis vector j, or slot j mod 3 of the ring (q_{j+1} overwrites q_{j-2}, which no launch of iteration j reads)
    auto slot = [&](u32 j) { return m->d_Q + (u64)(ring ? j % 3 : j) * nB; };

    // timing marks: every 4th iteration (every one when k < 8); each mark is a barrier packet
    const u32 every = k < 8 ? 1 : 4;
    const u32 marked = (k + every - 1) / every;
    while (m->ev.size() < 3 * (size_t)marked) {
        hipEvent_t e;
        LZX_HIP(hipEventCreate(&e));
        m->ev.push_back(e);
    }
    const u32 vgrid = std::min<u32>(std::max<u32>(m->n_seg, 1), (u32)c->cu_count * 4);
    const u32 sgrid = std::min<u32>(grid_of(nB), (u32)c->cu_count * 8);
    LZX_HIP(hipStreamSynchronize(c->stream));
    const auto t0 = std::chrono::steady_clock::now();
    for (u32 j = 0; j < k; ++j) {
        const bool mark = j % every == 0;
        hipEvent_t *e = m->ev.data() + 3 * (j / every);
        double *qj = slot(j);
        if (mark) LZX_HIP(hipEventRecord(e[0], c->stream));
        LZX_TRY(launch_spmm<B>(c, qj, m->d_V, qj));
        if (mark) LZX_HIP(hipEventRecord(e[1], c->stream));
        const bool last = j + 1 == k;
        hipLaunchKernelGGL(k_multi_update<B>, dim3(last ? 1 : vgrid), dim3(LZX_MULTI_BLOCK), 0, c->stream, m->d_V, qj,
                           j ? slot(j - 1) : qj, m->d_pa, m->n_seg, m->d_alpha, m->d_beta, k, j, m->d_pn, n, last ? 1 : 0);
        if (!last)
            hipLaunchKernelGGL(k_multi_scale<B>, dim3(sgrid), dim3(LZX_MULTI_BLOCK), 0, c->stream, m->d_V, m->d_pn, m->n_seg,
                               m->d_alpha, m->d_beta, m->d_mx, k, j, slot(j + 1), n, lzx_stop_threshold(c));
        LZX_HIP(hipGetLastError());
        if (mark) LZX_HIP(hipEventRecord(e[2], c->stream));
    }
    LZX_HIP(hipStreamSynchronize(c->stream));
    const double loop_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

    std::vector<double> ha((u64)B * k), hb((u64)B * k);
    LZX_HIP(hipMemcpy(ha.data(), m->d_alpha, sizeof(double) * ha.size(), hipMemcpyDeviceToHost));
    LZX_HIP(hipMemcpy(hb.data(), m->d_beta, sizeof(double) * hb.size(), hipMemcpyDeviceToHost));
    m->h_kused.assign(B, 0);
    for (u32 col = 0; col < b; ++col) {
        u32 ku = k;
        for (u32 j = 0; j + 1 < k; ++j)
            if (hb[(u64)col * k + j] == 0.0) { ku = j + 1; break; }
        m->h_kused[col] = ku;
        k_used[col] = ku;
        for (u32 j = 0; j < k; ++j) {
            alpha[(u64)col * k + j] = ha[(u64)col * k + j];
            beta[(u64)col * k + j] = j + 1 < k ? hb[(u64)col * k + j] : 0.0;
        }
    }
    LZX_HIP(hipMemcpy(m->d_kused, m->h_kused.data(), sizeof(u32) * B, hipMemcpyHostToDevice));
    if (Q) {
        // column j of every vector: [n][B] -> [b][n] in the work vector, then b rows of n with a stride of k * n on the host
        for (u32 j = 0; j < k; ++j) {
            hipLaunchKernelGGL(k_multi_unpack<B>, dim3(grid_of(nB)), dim3(LZX_MULTI_BLOCK), 0, c->stream, m->d_Q + (u64)j * nB, b, n, m->d_X);
            LZX_HIP(hipGetLastError());
            LZX_HIP(hipMemcpy2DAsync(Q + (u64)j * n, sizeof(double) * k * n, m->d_X, sizeof(double) * n, sizeof(double) * n, b,
                                     hipMemcpyDeviceToHost, c->stream));
        }
        LZX_HIP(hipStreamSynchronize(c->stream));
    }
    m->b = b;
    m->resident = !ring;
    m->probe = !ring && !X0;
    if (stats) {
        double spmm = 0, vec = 0, mn = 1e300;
        for (u32 q = 0; q < marked; ++q) {
            float a = 0.f, v = 0.f;
            hipEvent_t *e = m->ev.data() + 3 * q;
            LZX_HIP(hipEventElapsedTime(&a, e[0], e[1]));
            LZX_HIP(hipEventElapsedTime(&v, e[1], e[2]));
            spmm += a;
            vec += v;
            mn = std::min(mn, (double)a);
        }
        const double scale = (double)k / marked;
        stats->loop_ms = loop_ms;
        stats->spmv_ms = spmm * scale;
        stats->spmv_ms_min = mn;
        stats->vec_ms = vec * scale;
        stats->comm_ms = 0.0;
        stats->iters = k;
        stats->spmv_kernels = 4;   // launches per iteration: SpMM, split rows + alpha partials, update, scale
        stats->spmv_bytes = 4ull * c->nnz + 8ull * (n + 1) + 16ull * b * n;
    }
    return LZX_OK;
}

template <u32 B>
static int spmm_run(lzx_ctx *c, u32 b, const double *X, double *Y)
{
    lzx_multi_state *m = c->multi;
    const u64 n = c->n, nB = n * B;
    LZX_TRY(lzx_multi_ensure_work(c, B));
    MultiDiv one{};
    for (u32 col = 0; col < 16; ++col) one.v[col] = 1.0;
    LZX_HIP(hipMemcpyAsync(m->d_V, X, sizeof(double) * b * n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_multi_pack<B>, dim3(grid_of(nB)), dim3(LZX_MULTI_BLOCK), 0, c->stream, m->d_V, b, n, one, m->d_X);
    LZX_HIP(hipGetLastError());
    LZX_TRY(launch_spmm<B>(c, m->d_X, m->d_V, nullptr));
    hipLaunchKernelGGL(k_multi_unpack<B>, dim3(grid_of(nB)), dim3(LZX_MULTI_BLOCK), 0, c->stream, m->d_V, b, n, m->d_X);
    LZX_HIP(hipGetLastError());
    LZX_HIP(hipMemcpyAsync(Y, m->d_X, sizeof(double) * b * n, hipMemcpyDeviceToHost, c->stream));
    LZX_HIP(hipStreamSynchronize(c->stream));
    return LZX_OK;
}

// T [b][k] -> d_T [B][k], entries at or behind k_used[c] and padded columns 0
static int upload_T(lzx_ctx *c, u32 B, u32 b, const double *T, u32 k)
{
    lzx_multi_state *m = c->multi;
    std::vector<double> t((u64)B * k, 0.0);
    for (u32 col = 0; col < b; ++col)
        for (u32 j = 0; j < std::min(k, m->h_kused[col]); ++j) t[(u64)col * k + j] = T[(u64)col * k + j];
    LZX_HIP(hipMemcpyAsync(m->d_T, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice, c->stream));
    LZX_HIP(hipStreamSynchronize(c->stream));   // t is freed on return
    return LZX_OK;
}

template <u32 B>
static int multout_run(lzx_ctx *c, u32 b, const double *T, u32 k, double *ans)
{
    lzx_multi_state *m = c->multi;
    const u64 n = c->n, nB = n * B;
    LZX_TRY(lzx_multi_ensure_work(c, B));
    LZX_TRY(upload_T(c, B, b, T, k));
    hipLaunchKernelGGL(k_multi_multout<B>, dim3(grid_of(nB)), dim3(LZX_MULTI_BLOCK), 0, c->stream, m->d_Q, k, n, m->d_T, m->d_kused, m->d_V);
    hipLaunchKernelGGL(k_multi_unpack<B>, dim3(grid_of(nB)), dim3(LZX_MULTI_BLOCK), 0, c->stream, m->d_V, b, n, m->d_X);
    LZX_HIP(hipGetLastError());
    LZX_HIP(hipMemcpyAsync(ans, m->d_X, sizeof(double) * b * n, hipMemcpyDeviceToHost, c->stream));
    LZX_HIP(hipStreamSynchronize(c->stream));
    return LZX_OK;
}

template <u32 B>
static int diag_run(lzx_ctx *c, u32 b, const double *T, u32 k, double *out)
{
    lzx_multi_state *m = c->multi;
    const u64 n = c->n;
    LZX_TRY(lzx_multi_ensure_work(c, B, false));
    LZX_TRY(upload_T(c, B, b, T, k));
    hipLaunchKernelGGL(k_multi_diag<B>, dim3(grid_of(n * B)), dim3(LZX_MULTI_BLOCK), 0, c->stream, m->d_Q, k, n, b, m->d_T, m->d_kused, m->d_V);
    LZX_HIP(hipGetLastError());
    LZX_HIP(hipMemcpyAsync(out, m->d_V, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    LZX_HIP(hipStreamSynchronize(c->stream));
    return LZX_OK;
}

template <u32 B>
static int probes_run(lzx_ctx *c, u64 seed, u64 first, u32 b, double *Z)
{
    lzx_multi_state *m = c->multi;
    const u64 n = c->n, nB = n * B;
    LZX_TRY(lzx_multi_ensure_work(c, B));
    hipLaunchKernelGGL(k_multi_probe<B>, dim3(grid_of(nB)), dim3(LZX_MULTI_BLOCK), 0, c->stream, seed, first, b, n, 1.0, m->d_V);
    hipLaunchKernelGGL(k_multi_unpack<B>, dim3(grid_of(nB)), dim3(LZX_MULTI_BLOCK), 0, c->stream, m->d_V, b, n, m->d_X);
    LZX_HIP(hipGetLastError());
    LZX_HIP(hipMemcpyAsync(Z, m->d_X, sizeof(double) * b * n, hipMemcpyDeviceToHost, c->stream));
    LZX_HIP(hipStreamSynchronize(c->stream));
    return LZX_OK;
}

#define LZX_MULTI_DISPATCH(B, fn, ...)     \
    switch (B) {                           \
    case 2: return fn<2>(__VA_ARGS__);     \
    case 4: return fn<4>(__VA_ARGS__);     \
    case 8: return fn<8>(__VA_ARGS__);     \
    default: return fn<16>(__VA_ARGS__);   \
    }

// ==================================================================================================== C ABI
extern "C" int lzx_lanczos_multi_f64(lzx_handle h, uint32_t b, const double *X0, uint32_t k, double *alpha, double *beta,
                                     uint32_t *k_used, double *x_norm, double *Q, lzx_stats *stats)
{
    static const char *fn = "lzx_lanczos_multi_f64";
    if (!h) LZX_FAIL(LZX_ERR_ARG, "%s: null handle (h)", fn);
    if (b == 0) LZX_FAIL(LZX_ERR_ARG, "%s: b == 0", fn);
    if (b > 16) LZX_FAIL(LZX_ERR_LIMIT, "%s: b = %u columns (at most 16 per batch)", fn, b);
    if (!X0) LZX_FAIL(LZX_ERR_ARG, "%s: null X0", fn);
    if (!alpha || !beta) LZX_FAIL(LZX_ERR_ARG, "%s: null alpha / beta", fn);
    if (!k_used || !x_norm) LZX_FAIL(LZX_ERR_ARG, "%s: null k_used / x_norm", fn);
    if (k == 0) LZX_FAIL(LZX_ERR_ARG, "%s: k == 0", fn);
    LZX_TRY(lzx_multi_check_handle(h, fn));
    for (u32 col = 0; col < b; ++col) {
        const double *x = X0 + (u64)col * h->n;
        if (std::all_of(x, x + h->n, [](double v) { return v == 0.0; }))
            LZX_FAIL(LZX_ERR_ARG, "%s: column %u of X0 is all zero", fn, col);
    }
    int rc = lzx_multi_build_tables(h);
    if (rc) return rc;
    const u32 B = lzx_multi_pad_width(b);
    LZX_MULTI_DISPATCH(B, multi_loop, h, b, MultiStart{X0, 0, 0}, false, k, alpha, beta, k_used, x_norm, Q, stats, fn);
}

extern "C" int lzx_multout_multi_f64(lzx_handle h, uint32_t b, const double *T, uint32_t k, double *ans)
{
    static const char *fn = "lzx_multout_multi_f64";
    if (!h) LZX_FAIL(LZX_ERR_ARG, "%s: null handle (h)", fn);
    if (b == 0) LZX_FAIL(LZX_ERR_ARG, "%s: b == 0", fn);
    if (b > 16) LZX_FAIL(LZX_ERR_LIMIT, "%s: b = %u columns (at most 16 per batch)", fn, b);
    if (!T || !ans) LZX_FAIL(LZX_ERR_ARG, "%s: null T / ans", fn);
    if (k == 0) LZX_FAIL(LZX_ERR_ARG, "%s: k == 0", fn);
    LZX_TRY(lzx_multi_check_handle(h, fn));
    lzx_multi_state *m = h->multi;
    if (!m->resident) LZX_FAIL(LZX_ERR_STATE, "%s: no batched decomposition is resident", fn);
    if (b != m->b || k > m->k)
        LZX_FAIL(LZX_ERR_ARG, "%s: the resident batch has b = %u columns of k = %u vectors (asked b = %u, k = %u)", fn, m->b, m->k, b, k);
    LZX_MULTI_DISPATCH(m->B, multout_run, h, b, T, k, ans);
}

extern "C" int lzx_spmm_f64(lzx_handle h, uint32_t b, const double *X, double *Y)
{
    static const char *fn = "lzx_spmm_f64";
    if (!h) LZX_FAIL(LZX_ERR_ARG, "%s: null handle (h)", fn);
    if (b == 0) LZX_FAIL(LZX_ERR_ARG, "%s: b == 0", fn);
    if (b > 16) LZX_FAIL(LZX_ERR_LIMIT, "%s: b = %u columns (at most 16 per batch)", fn, b);
    if (!X || !Y) LZX_FAIL(LZX_ERR_ARG, "%s: null X / Y", fn);
    LZX_TRY(lzx_multi_check_handle(h, fn));
    LZX_TRY(lzx_multi_build_tables(h));
    // (the resident batch keeps its basis: only the work vectors may change width)
    LZX_MULTI_DISPATCH(lzx_multi_pad_width(b), spmm_run, h, b, X, Y);
}

extern "C" int lzx_multi_release(lzx_handle h)
{
    if (!h) LZX_FAIL(LZX_ERR_ARG, "lzx_multi_release: null handle (h)");
    lzx_multi_free(h, false);
    return LZX_OK;
}

// ---- stochastic Lanczos quadrature: probes generated on the device
static int check_probes(lzx_handle h, const char *fn, uint64_t first, uint32_t b)
{
    if (!h) LZX_FAIL(LZX_ERR_ARG, "%s: null handle (h)", fn);
    if (b == 0) LZX_FAIL(LZX_ERR_ARG, "%s: b == 0", fn);
    if (b > 16) LZX_FAIL(LZX_ERR_LIMIT, "%s: b = %u columns (at most 16 per batch)", fn, b);
    if (first > (1ull << 32) - b) LZX_FAIL(LZX_ERR_ARG, "%s: probes %llu + %u pass 2^32", fn, (unsigned long long)first, b);
    return LZX_OK;
}

extern "C" int lzx_probes_f64(lzx_handle h, uint64_t seed, uint64_t first, uint32_t b, double *Z)
{
    static const char *fn = "lzx_probes_f64";
    LZX_TRY(check_probes(h, fn, first, b));
    if (!Z) LZX_FAIL(LZX_ERR_ARG, "%s: null Z", fn);
    LZX_TRY(lzx_multi_check_handle(h, fn));
    LZX_TRY(lzx_multi_build_tables(h));
    LZX_MULTI_DISPATCH(lzx_multi_pad_width(b), probes_run, h, seed, first, b, Z);
}

extern "C" int lzx_lanczos_probes_f64(lzx_handle h, uint64_t seed, uint64_t first, uint32_t b, uint32_t k, uint32_t flags,
                                      double *alpha, double *beta, uint32_t *k_used, lzx_stats *stats)
{
    static const char *fn = "lzx_lanczos_probes_f64";
    LZX_TRY(check_probes(h, fn, first, b));
    if (k == 0) LZX_FAIL(LZX_ERR_ARG, "%s: k == 0", fn);
    if (!alpha || !beta || !k_used) LZX_FAIL(LZX_ERR_ARG, "%s: null alpha / beta / k_used", fn);
    if (flags & ~(uint32_t)LZX_PROBE_KEEP_BASIS) LZX_FAIL(LZX_ERR_ARG, "%s: unknown flags 0x%x", fn, flags);
    LZX_TRY(lzx_multi_check_handle(h, fn));
    LZX_TRY(lzx_multi_build_tables(h));
    const bool ring = !(flags & LZX_PROBE_KEEP_BASIS);
    LZX_MULTI_DISPATCH(lzx_multi_pad_width(b), multi_loop, h, b, MultiStart{nullptr, seed, first}, ring, k, alpha, beta, k_used, nullptr, nullptr,
                       stats, fn);
}

extern "C" int lzx_probe_diag_f64(lzx_handle h, const double *T, uint32_t k, double *out)
{
    static const char *fn = "lzx_probe_diag_f64";
    if (!h) LZX_FAIL(LZX_ERR_ARG, "%s: null handle (h)", fn);
    if (!T || !out) LZX_FAIL(LZX_ERR_ARG, "%s: null T / out", fn);
    if (k == 0) LZX_FAIL(LZX_ERR_ARG, "%s: k == 0", fn);
    LZX_TRY(lzx_multi_check_handle(h, fn));
    lzx_multi_state *m = h->multi;
    if (!m->resident || !m->probe)
        LZX_FAIL(LZX_ERR_STATE, "%s: no probe basis is resident (run lzx_lanczos_probes_f64 with LZX_PROBE_KEEP_BASIS)", fn);
    if (k > m->k) LZX_FAIL(LZX_ERR_ARG, "%s: the resident probe basis has k = %u vectors (asked k = %u)", fn, m->k, k);
    LZX_MULTI_DISPATCH(m->B, diag_run, h, m->b, T, k, out);
}
