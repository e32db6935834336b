// lzx_multi_shared.h -- what the batched path (lzx_multi.hip) shares with the batched solver (lzx_solve_multi.hip): the [n][B]
// layout's constants and per-graph state, the pack / unpack and SpMM kernels, the fixed-shape reductions, and the host helpers
// that build the work list and the work vectors.  Include after lzx_internal.h, lzx_spmv_body.h and lzx_reduce.h.
#pragma once

#include <algorithm>

static constexpr u32 LZX_MULTI_CHUNK = 2048;   // entries per chunk of a split row (test shape multi_row_chunk)
static constexpr u32 LZX_MULTI_RUN = 32;       // rows one thread sums left to right per column
static constexpr u32 LZX_MULTI_SEG = 2048;     // rows per partial (64 runs: one per lane of the closing wavefront)
static constexpr u32 LZX_MULTI_RUNS = LZX_MULTI_SEG / LZX_MULTI_RUN;
static constexpr u32 LZX_MULTI_BLOCK = 256;
static constexpr u32 LZX_MULTI_PAD = 0xffffffffu;   // work-list entry without output (padding)
static constexpr u32 LZX_MULTI_PART = 0x80000000u;  // work-list dst flag: a chunk total, slot = dst & ~flag

struct lzx_multi_state {
    // per graph: the work list (built on first use, freed with the graph)
    u32 chunk = 0;                     // L the list was built with
    u64 n_wl = 0;                      // entries, padded to a multiple of 32 (the most segments one wavefront takes)
    uint4 *d_wl = nullptr;             // {first entry lo, hi, length, dst}, longest first
    u32 n_split = 0, n_parts = 0;
    u32 *d_split_row = nullptr;        // [n_split] split rows, ascending
    u32 *d_split_first = nullptr;      // [n_split + 1] their first chunk slot
    u32 *d_run_split = nullptr;        // [runs + 1] first split row at or behind the run's first row
    u32 n_seg = 0;                     // partials per column
    // work vectors (width wB)
    u32 wB = 0;
    double *d_V = nullptr, *d_X = nullptr;   // [n][wB] each
    double *d_part = nullptr;          // [n_parts][wB] chunk totals
    double *d_pa = nullptr, *d_pn = nullptr; // [n_seg][wB]
    // batch basis
    u32 B = 0, b = 0, k = 0;
    bool resident = false;             // a decomposition's basis is there
    bool ring = false;                 // d_Q is three rotating slots (basis-free run), not a basis
    bool probe = false;                // the resident basis was started from probes (lzx_probe_diag_f64 works on it)
    double *d_Q = nullptr;             // [k][n][B], or [3][n][B] when ring
    double *d_alpha = nullptr, *d_beta = nullptr, *d_T = nullptr;   // [B][k]
    double *d_mx = nullptr;            // [k][B] running max of |alpha_i| + beta_{i-1}
    u32 *d_kused = nullptr;            // [B]
    std::vector<u32> h_kused;
    std::vector<hipEvent_t> ev;
};

// ---- host helpers (defined in lzx_multi.hip; prefixed: they are external symbols of the library)
u32 lzx_multi_pad_width(u32 b);
inline u32 grid_of(u64 threads) { return (u32)((threads + LZX_MULTI_BLOCK - 1) / LZX_MULTI_BLOCK); }
// one GPU handle with a graph (LZX_ERR_STATE otherwise); makes c->multi on first use and selects the device
int lzx_multi_check_handle(lzx_ctx *c, const char *fn);
// the work list, once per graph
int lzx_multi_build_tables(lzx_ctx *c);
// the work vectors of width B; need_x: the second one too
int lzx_multi_ensure_work(lzx_ctx *c, u32 B, bool need_x = true);
void lzx_multi_free_work(lzx_multi_state *m);

// in [b][n] (caller's vectors) -> out [n][B], column c divided by div[c]; padded columns 0
struct MultiDiv { double v[16]; };
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK) k_multi_pack(const double *in, u32 b, u64 n, MultiDiv div, double *out)
{
    const u64 i = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x;
    if (i >= n * B) return;
    const u32 c = (u32)(i % B);
    const u64 r = i / B;
    out[i] = c < b ? in[(u64)c * n + r] / div.v[c] : 0.0;
}

// in [n][B] -> out [b][n]
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK) k_multi_unpack(const double *in, u32 b, u64 n, double *out)
{
    const u64 i = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x;
    if (i >= n * B) return;
    const u32 c = (u32)(i % B);
    if (c < b) out[(u64)c * n + i / B] = in[i];
}

template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK)
k_multi_spmm(const uint4 *__restrict__ wl, u64 n_waves, const u32 *__restrict__ col, const double *__restrict__ X, double *Y, double *part)
{
    constexpr u32 G = 64 / B;
    const u64 w = (u64)blockIdx.x * (LZX_MULTI_BLOCK / 64) + (threadIdx.x >> 6);
    if (w >= n_waves) return;
    const u32 lane = threadIdx.x & 63, s = lane / B, c = lane % B;
    const uint4 e = wl[w * G + s];
    const u64 beg = (u64)e.x | ((u64)e.y << 32);
    const u32 len = e.z;
    double acc = 0.0;
    u32 i = 0;
    // eight gathers in flight, then added in entry order (the sum's order is the entries' whatever the loads do)
    for (; i + 8 <= len; i += 8) {
        u32 j[8];
        double t[8];
#pragma unroll
        for (u32 u = 0; u < 8; ++u) j[u] = col[beg + i + u];
#pragma unroll
        for (u32 u = 0; u < 8; ++u) t[u] = X[(u64)j[u] * B + c];
#pragma unroll
        for (u32 u = 0; u < 8; ++u) acc += t[u];
    }
    for (; i < len; ++i) acc += X[(u64)col[beg + i] * B + c];
    if (e.w == LZX_MULTI_PAD) return;
    if (e.w & LZX_MULTI_PART) part[(u64)(e.w & ~LZX_MULTI_PART) * B + c] = acc;
    else Y[(u64)e.w * B + c] = acc;
}

// Per row segment and column: LZX_MULTI_RUNS run totals in sh[run * B + c] -> one partial out[c], by a tree whose shape does
// not depend on B (lane l holds run l, then wave_sum).  Call with all threads; ends with a barrier.
template <u32 B>
__device__ __forceinline__ void seg_partials(double *sh, double *out)
{
    static_assert(LZX_MULTI_RUNS == 64, "one run per lane");
    __syncthreads();
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (u32 c = wave; c < B; c += LZX_MULTI_BLOCK / 64) {
        const double x = wave_sum(sh[lane * B + c]);
        if (lane == 0) out[c] = x;
    }
    __syncthreads();
}

// All B columns' totals of p[0 .. np) ([np][B]) closed identically in every workgroup: per column the shape of
// block_sum_fixed_256 (thread t adds entries t, t + 256, ... in index order, then wave_sum, then the four waves in order).
template <u32 B>
__device__ __forceinline__ void close_cols(const double *p, u32 np, double *shw /* [4][B] */, double *out /* [B], LDS */)
{
    double s[B];
#pragma unroll
    for (u32 c = 0; c < B; ++c) s[c] = 0.0;
    for (u32 i = threadIdx.x; i < np; i += LZX_MULTI_BLOCK) {
        double t[B];
#pragma unroll
        for (u32 c = 0; c < B; c += 2) {
            const double2 v = *reinterpret_cast<const double2 *>(p + (u64)i * B + c);
            t[c] = v.x;
            t[c + 1] = v.y;
        }
#pragma unroll
        for (u32 c = 0; c < B; ++c) s[c] += t[c];
    }
#pragma unroll
    for (u32 c = 0; c < B; ++c) {
        const double w = wave_sum(s[c]);
        if ((threadIdx.x & 63) == 0) shw[(threadIdx.x >> 6) * B + c] = w;
    }
    __syncthreads();
    if (threadIdx.x < B) {
        const u32 c = threadIdx.x;
        out[c] = ((shw[c] + shw[B + c]) + shw[2 * B + c]) + shw[3 * B + c];
    }
    __syncthreads();
}

// Split rows: V[r] = their chunk totals added in chunk order; with Q: partials of alpha = v . q per (row segment, column).
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK)
k_multi_alpha(double *V, const double *__restrict__ part, const u32 *__restrict__ split_row, const u32 *__restrict__ split_first,
                const u32 *__restrict__ run_split, u32 n_split, const double *__restrict__ Q, double *pa, u64 n, u32 n_seg,
                const u64 *__restrict__ row_ptr, const double *__restrict__ X)
{
    // row_ptr != nullptr (operator L): V[r] = fma(d_r, X[r], -V[r]) once the row's total is complete -- the epilogue of the
    // single-vector k_lap_apply, per column, so columns stay independent
    __shared__ double sh[LZX_MULTI_RUNS * B];
    for (u32 seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
        for (u32 u = threadIdx.x; u < LZX_MULTI_RUNS * B; u += LZX_MULTI_BLOCK) {
            const u32 run = u / B, c = u % B;
            const u64 r0 = (u64)seg * LZX_MULTI_SEG + (u64)run * LZX_MULTI_RUN;
            const u64 r1 = std::min<u64>(r0 + LZX_MULTI_RUN, n);
            double s = 0.0;
            u32 ks = r0 < n ? run_split[r0 / LZX_MULTI_RUN] : n_split;
            if (r0 < n && r1 == r0 + LZX_MULTI_RUN && (ks >= n_split || split_row[ks] >= r1)) {
                // no split row in this run (nearly every run): eight rows' loads in flight, products added in row order
                if (row_ptr) {
                    for (u64 r = r0; r < r1; ++r) {
                        const double v = fma((double)(row_ptr[r + 1] - row_ptr[r]), X[r * B + c], -V[r * B + c]);
                        V[r * B + c] = v;
                        if (Q) s += v * Q[r * B + c];
                    }
                } else if (Q) {
                    for (u64 r = r0; r < r1; r += 8) {
                        double v[8], q[8];
#pragma unroll
                        for (u32 t = 0; t < 8; ++t) { v[t] = V[(r + t) * B + c]; q[t] = Q[(r + t) * B + c]; }
#pragma unroll
                        for (u32 t = 0; t < 8; ++t) s += v[t] * q[t];
                    }
                }
            } else if (r0 < n) {
                for (u64 r = r0; r < r1; ++r) {
                    double v;
                    if (ks < n_split && split_row[ks] == r) {
                        v = 0.0;
                        for (u32 p = split_first[ks]; p < split_first[ks + 1]; ++p) v += part[(u64)p * B + c];
                        if (row_ptr) v = fma((double)(row_ptr[r + 1] - row_ptr[r]), X[r * B + c], -v);
                        V[r * B + c] = v;
                        ++ks;
                    } else {
                        v = V[r * B + c];
                        if (row_ptr) {
                            v = fma((double)(row_ptr[r + 1] - row_ptr[r]), X[r * B + c], -v);
                            V[r * B + c] = v;
                        }
                    }
                    if (Q) s += v * Q[r * B + c];
                }
            }
            sh[u] = s;
        }
        if (Q) seg_partials<B>(sh, pa + (u64)seg * B);
    }
}

// Y = A X on [n][B] vectors, split rows finished into Y; with Q: alpha partials into pa (the loop's first two launches)
template <u32 B>
int launch_spmm(lzx_ctx *c, const double *X, double *Y, const double *Q)
{
    lzx_multi_state *m = c->multi;
    const u64 n_waves = m->n_wl / (64 / B);
    if (n_waves)
        hipLaunchKernelGGL(k_multi_spmm<B>, dim3((u32)((n_waves + 3) / 4)), dim3(LZX_MULTI_BLOCK), 0, c->stream, m->d_wl, n_waves,
                           c->d_col_idx, X, Y, m->d_part);
    const bool lap = c->op_opt == LZX_OP_LAPLACIAN;
    if (m->n_seg && (Q || m->n_split || lap))
        hipLaunchKernelGGL(k_multi_alpha<B>, dim3(std::min<u32>(m->n_seg, (u32)c->cu_count * 4)), dim3(LZX_MULTI_BLOCK), 0, c->stream, Y,
                           m->d_part, m->d_split_row, m->d_split_first, m->d_run_split, m->n_split, Q, m->d_pa, c->n, m->n_seg,
                           lap ? c->d_row_ptr : nullptr, X);
    LZX_HIP(hipGetLastError());
    return LZX_OK;
}
