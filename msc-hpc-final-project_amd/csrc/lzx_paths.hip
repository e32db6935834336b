// lzx_paths.hip -- path-based centralities on the device: breadth-first search from many sources at once, and Brandes'
// betweenness on top of it (include/lzx.h: lzx_bfs_multi, lzx_betweenness_f64, lzx_brandes_f64; DESIGN.md sections 17 and 24).
//
// Up to 16 sources share every sweep over the edges: the per-vertex state is laid out [n][B] (B = the batch width padded to
// 2, 4, 8 or 16) like the batched path's vectors, and the sweeps walk the batched path's work list (lzx_multi_shared.h: whole
// rows and chunks of split rows, longest first), one lane per (segment, column).  The state of one batch:
//   dist   i32 [n][B]   level of the vertex seen from the column's source, -1 = not reached (yet)
//   sigma  f64 [n][B]   number of shortest paths from the source; the backward pass overwrites it with the dependency delta
//   g      f64 [n][B]   (1 + delta) / sigma (betweenness only; lzx_bfs_multi stages its outputs here)
// Both passes are the same masked SpMM in pull form, Y[v][c] = sum over the neighbours u of v with dist[u][c] == want of X[u][c],
// for the rows whose own dist meets a row condition; a lane whose row condition fails skips its gather.
//   forward, level d = 1, 2, ...   rows with dist == -1 gather sigma from the neighbours with dist == d - 1; a sum s > 0 sets
//                                  dist = d and sigma = s.  In place: a reader tests == d - 1, a writer stores d, so no read
//                                  depends on when a write lands.  Newly reached vertices are counted per column (one integer
//                                  atomic per wavefront and column after a wave reduction); the host reads those B words after
//                                  every level, stops when none grew, and forms reached / sum_dist / harmonic / ecc from them.
//   backward, level d = L ... 1    rows with dist == d gather g from the neighbours with dist == d + 1: delta = sigma * s,
//                                  g = (1 + delta) / sigma, and delta takes sigma's place (nobody reads another vertex's sigma
//                                  in this pass).  The sweep of the deepest level L finds no neighbour below and leaves
//                                  delta = 0, g = 1 / sigma there.
//   accumulate                     bc[v] += delta[v][c] for the columns c = 0, 1, ... in which v was reached and is not the
//                                  source, one column after the other: bc is the left-to-right sum over the sources in the
//                                  caller's order wherever the batch boundaries fall.
// A sum over a row is one accumulator over its entries in CSR order; a split row's chunk totals are added in chunk order by
// k_paths_split.  Those shapes depend on the graph alone, there is no floating-point atomic, and the only racing accesses are
// the forward pass's dist words, whose two possible values (-1, d) both fail the reader's test: results are the same bits in
// every run and for every composition of the batch.
//
// lzx_brandes_f64 adds edge betweenness and the endpoints to the same pass.  With ebc wanted the backward pass keeps sigma
// (delta goes to a fourth [n][B] array, and only when bc is wanted too), and after the last backward level of a batch one edge
// pass (k_paths_edges) adds, per stored entry of the caller-order CSR, sigma * g over the batch's columns in ascending order.  The
// endpoints are a 64-bit count per vertex (k_paths_endpoints), added to bc once, after the last batch.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "lzx_internal.h"
#include "lzx_graph_call.h"
#include "lzx_spmv_body.h"
#include "lzx_reduce.h"
#include "lzx_multi_shared.h"

static constexpr u32 LZX_BFS_BATCH = 16;

struct PathsSources { u32 v[LZX_BFS_BATCH]; };

// dist = -1, sigma = 0 everywhere but at the column's source (0, 1); padded columns have no source
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK) k_paths_init(int32_t *dist, double *sigma, u64 n, u32 b, PathsSources src)
{
    const u64 i = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x;
    if (i >= n * B) return;
    const u32 c = (u32)(i % B);
    const bool hit = c < b && src.v[c] == i / B;
    dist[i] = hit ? 0 : -1;
    sigma[i] = hit ? 1.0 : 0.0;
}

// part_row[p] = the row chunk slot p belongs to
__global__ void k_paths_part_rows(const u32 *split_row, const u32 *split_first, u32 n_split, u32 *part_row)
{
    const u32 ks = blockIdx.x * blockDim.x + threadIdx.x;
    if (ks >= n_split) return;
    const u32 row = split_row[ks];
    for (u32 p = split_first[ks]; p < split_first[ks + 1]; ++p) part_row[p] = row;
}

// the three forms of a level: the forward search, the backward recurrence that puts delta in sigma's place (lzx_betweenness_f64),
// and the one that keeps sigma for the edge pass (lzx_brandes_f64): delta goes to a fourth array, and only if bc is wanted
enum : int { PATHS_FORWARD = 0, PATHS_BACK = 1, PATHS_BACK_KEEP = 2 };

// what a complete row sum s does to (row, column) i; forward: 1 if the vertex was reached at this level
template <int MODE>
__device__ __forceinline__ u32 paths_epilogue(u64 i, double s, int32_t d, int32_t *dist, double *sigma, double *g, double *delta_out)
{
    if (MODE != PATHS_FORWARD) {
        const double sg = sigma[i];
        const double delta = sg * s;
        g[i] = (1.0 + delta) / sg;
        if (MODE == PATHS_BACK) sigma[i] = delta;
        else if (delta_out) delta_out[i] = delta;
        return 0;
    }
    if (!(s > 0.0)) return 0;
    dist[i] = d;
    sigma[i] = s;
    return 1;
}

// every lane holds a count for column lane % B: the wavefront's total per column, one atomic each.  Call with all 64 lanes.
template <u32 B>
__device__ __forceinline__ void paths_count(u32 v, u32 *reached)
{
#pragma unroll
    for (u32 o = 32; o >= B; o >>= 1) v += (u32)__shfl_xor((int)v, (int)o, 64);
    const u32 lane = threadIdx.x & 63;
    if (lane < B && v) atomicAdd(&reached[lane], v);
}

// One level of either pass over the work list: lane (segment, column) of a wavefront.  want_row / want: -1 / d - 1 forward,
// d / d + 1 backward.  A chunk of a split row leaves its total in part (closed by k_paths_split).
template <u32 B, int MODE>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK)
k_paths_sweep(const uint4 *__restrict__ wl, u64 n_waves, const u32 *__restrict__ col, const u32 *__restrict__ part_row, int32_t *dist,
              double *sigma, double *g, double *part, u32 b, int32_t d, u32 *reached, double *delta_out)
{
    constexpr bool BACK = MODE != PATHS_FORWARD;
    constexpr u32 G = 64 / B;
    const u64 w = (u64)blockIdx.x * (LZX_MULTI_BLOCK / 64) + (threadIdx.x >> 6);
    if (w >= n_waves) return;   // (the whole wavefront)
    const u32 lane = threadIdx.x & 63, s = lane / B, c = lane % B;
    const uint4 e = wl[w * G + s];
    const u64 beg = (u64)e.x | ((u64)e.y << 32);
    const u32 len = e.z;
    const bool pad = e.w == LZX_MULTI_PAD, chunk = !pad && (e.w & LZX_MULTI_PART);
    const u32 slot = e.w & ~LZX_MULTI_PART;
    const u32 row = pad ? 0u : chunk ? part_row[slot] : e.w;
    const u64 at = (u64)row * B + c;
    const int32_t want_row = BACK ? d : -1, want = BACK ? d + 1 : d - 1;
    const bool act = !pad && c < b && dist[at] == want_row;
    const double *X = BACK ? g : sigma;
    u32 newly = 0;
    if (act) {
        double acc = 0.0;
        u32 i = 0;
        // eight entries' levels in flight, then their values, added in entry order (a masked entry adds 0)
        for (; i + 8 <= len; i += 8) {
            u32 j[8];
            int32_t lv[8];
            double t[8];
#pragma unroll
            for (u32 u = 0; u < 8; ++u) j[u] = col[beg + i + u];
#pragma unroll
            for (u32 u = 0; u < 8; ++u) lv[u] = dist[(u64)j[u] * B + c];
#pragma unroll
            for (u32 u = 0; u < 8; ++u) t[u] = lv[u] == want ? X[(u64)j[u] * B + c] : 0.0;
#pragma unroll
            for (u32 u = 0; u < 8; ++u) acc += t[u];
        }
        for (; i < len; ++i) {
            const u64 o = (u64)col[beg + i] * B + c;
            if (dist[o] == want) acc += X[o];
        }
        if (chunk) part[(u64)slot * B + c] = acc;
        else newly = paths_epilogue<MODE>(at, acc, d, dist, sigma, g, delta_out);
    }
    if (!BACK) paths_count<B>(newly, reached);
}

// split rows: the chunk totals added in chunk order, then the same epilogue; thread (split row, column)
template <u32 B, int MODE>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK)
k_paths_split(const double *part, const u32 *__restrict__ split_row, const u32 *__restrict__ split_first, u32 n_split, int32_t *dist,
              double *sigma, double *g, u32 b, int32_t d, u32 *reached, double *delta_out)
{
    constexpr bool BACK = MODE != PATHS_FORWARD;
    const u64 i = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x;
    const u64 ks = i / B;
    const u32 c = (u32)(i % B);
    u32 newly = 0;
    if (ks < n_split && c < b) {
        const u64 at = (u64)split_row[ks] * B + c;
        if (dist[at] == (BACK ? d : -1)) {
            double acc = 0.0;
            for (u32 p = split_first[ks]; p < split_first[ks + 1]; ++p) acc += part[(u64)p * B + c];
            newly = paths_epilogue<MODE>(at, acc, d, dist, sigma, g, delta_out);
        }
    }
    if (!BACK) paths_count<B>(newly, reached);
}

// bc[v] += delta[v][c], c ascending, over the columns in which v was reached and is not the source
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK) k_paths_accumulate(const int32_t *__restrict__ dist, const double *__restrict__ delta, u64 n, u32 b, double *bc)
{
    const u64 r = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x;
    if (r >= n) return;
    int32_t lv[B];
    double t[B];
#pragma unroll
    for (u32 c = 0; c < B; ++c) {
        lv[c] = dist[r * B + c];
        t[c] = delta[r * B + c];
    }
    double x = bc[r];
#pragma unroll
    for (u32 c = 0; c < B; ++c)
        if (c < b && lv[c] > 0) x += t[c];
    bc[r] = x;
}

// the endpoints' count of one batch: cnt[v] += 1 per column whose source reaches v from elsewhere, and reached - 1 per column
// whose source v is (dist = 0 holds at the source alone)
struct PathsReached { u64 v[LZX_BFS_BATCH]; };

template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK) k_paths_endpoints(const int32_t *__restrict__ dist, u64 n, u32 b, PathsReached reached, long long *cnt)
{
    const u64 r = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x;
    if (r >= n) return;
    long long x = cnt[r];
#pragma unroll
    for (u32 c = 0; c < B; ++c) {
        const int32_t lv = dist[r * B + c];
        if (c < b && lv > 0) x += 1;
        else if (c < b && lv == 0) x += (long long)reached.v[c] - 1;
    }
    cnt[r] = x;
}

// bc[v] = bc[v] + (double)cnt[v]: the one addition of the endpoints, after the last batch
__global__ void __launch_bounds__(LZX_MULTI_BLOCK) k_paths_add_endpoints(const long long *__restrict__ cnt, u64 n, double *bc)
{
    const u64 r = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x;
    if (r < n) bc[r] = bc[r] + (double)cnt[r];
}

// The edge pass of one batch, after its last backward level: ebc[e] += c_c(u, w) for the columns c = 0, 1, ... in ascending
// order, for every stored entry e = (u, w) of the caller-order CSR.  c_c(u, w) = sigma[u][c] * g[w][c] where w lies one level
// below u, sigma[w][c] * g[u][c] where it lies one level above, +0 otherwise (x + 0 = x: such a column is skipped, and an entry
// without a column is not written).  G lanes per row, 256 / G rows per workgroup, and a whole workgroup for a row of more than
// 64 G entries; a lane keeps its row's B-wide dist / sigma / g in registers, reads the neighbour's dist line per entry, and of
// its sigma / g lines only the one word per column a term needs.  g of a source and of an unreached vertex is never formed: the
// dist tests stand in front of every use of a g.  Every entry belongs to one lane: no atomic, and a sum that depends on the
// entry's own terms alone.
// the B levels of one vertex, a line of 4 B bytes aligned to its size, in 16-byte loads
template <u32 B>
__device__ __forceinline__ void paths_load_levels(const int32_t *__restrict__ line, int32_t (&lv)[B])
{
    if constexpr (B == 2) {
        const int2 t = *reinterpret_cast<const int2 *>(line);
        lv[0] = t.x;
        lv[1] = t.y;
    } else {
#pragma unroll
        for (u32 k = 0; k < B / 4; ++k) {
            const int4 t = reinterpret_cast<const int4 *>(line)[k];
            lv[4 * k] = t.x;
            lv[4 * k + 1] = t.y;
            lv[4 * k + 2] = t.z;
            lv[4 * k + 3] = t.w;
        }
    }
}

// One lane's share of row `row`: the entries first, first + step, ... < end
template <u32 B>
__device__ __forceinline__ void paths_edges_of_row(u64 row, u64 first, u64 end, u32 step, const u32 *__restrict__ col, const int32_t *__restrict__ dist,
                                                   const double *__restrict__ sigma, const double *__restrict__ g, u32 b, double *ebc)
{
    if (first >= end) return;
    int32_t du[B];
    u32 seen = 0;
    paths_load_levels<B>(dist + row * B, du);
#pragma unroll
    for (u32 c = 0; c < B; ++c)
        if (c < b && du[c] >= 0) seen |= 1u << c;
    if (!seen) return;   // no source of the batch reaches this row: all of its terms are +0
    double su[B], gu[B];
#pragma unroll
    for (u32 c = 0; c < B; ++c) {
        su[c] = sigma[row * B + c];
        gu[c] = g[row * B + c];
    }
    for (u64 e = first; e < end; e += step) {
        const u64 w = (u64)col[e] * B;
        int32_t dw[B];
        paths_load_levels<B>(dist + w, dw);
        u32 down = 0, up = 0;
#pragma unroll
        for (u32 c = 0; c < B; ++c) {
            if (c < b && du[c] >= 0 && dw[c] == du[c] + 1) down |= 1u << c;
            if (c < b && dw[c] >= 0 && du[c] == dw[c] + 1) up |= 1u << c;
        }
        if (!(down | up)) continue;
        double x = ebc[e];
        // the neighbour's words of up to eight columns in flight, then their terms added in column order: a load inside the
        // chain of additions would wait for the one before it
        constexpr u32 CH = B < 8 ? B : 8;
#pragma unroll
        for (u32 c0 = 0; c0 < B; c0 += CH) {
            double v[CH];
#pragma unroll
            for (u32 k = 0; k < CH; ++k) {
                const u32 c = c0 + k;
                const double *from = ((down >> c) & 1u) ? g : sigma;
                v[k] = (((down | up) >> c) & 1u) ? from[w + c] : 0.0;
            }
#pragma unroll
            for (u32 k = 0; k < CH; ++k) {
                const u32 c = c0 + k;
                const double mine = ((down >> c) & 1u) ? su[c] : gu[c];   // sigma[u] * g[w] or sigma[w] * g[u]: one product either way
                if (((down | up) >> c) & 1u) x += mine * v[k];
            }
        }
        ebc[e] = x;
    }
}

// rows of at most long_row entries: G lanes per row, 256 / G rows per workgroup
template <u32 B, u32 G>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK)
k_paths_edges(const u64 *__restrict__ row_ptr, const u32 *__restrict__ col, const int32_t *__restrict__ dist, const double *__restrict__ sigma,
              const double *__restrict__ g, u64 n, u32 b, u32 long_row, double *ebc)
{
    const u64 row = (u64)blockIdx.x * (LZX_MULTI_BLOCK / G) + threadIdx.x / G;
    if (row >= n) return;
    const u64 beg = row_ptr[row], end = row_ptr[row + 1];
    if (end - beg > long_row) return;   // k_paths_edges_long's
    paths_edges_of_row<B>(row, beg + (threadIdx.x & (G - 1)), end, G, col, dist, sigma, g, b, ebc);
}

// rows of more than long_row entries among the 256 rows of blockIdx.x: gridDim.y workgroups per row, which take its entries in
// turns of 256 (the hubs of an R-MAT graph sit side by side at the low ids: one workgroup for all of them is the whole pass's tail)
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK)
k_paths_edges_long(const u64 *__restrict__ row_ptr, const u32 *__restrict__ col, const int32_t *__restrict__ dist, const double *__restrict__ sigma,
                   const double *__restrict__ g, u64 n, u32 b, u32 long_row, double *ebc)
{
    __shared__ u32 s_rows[LZX_MULTI_BLOCK];
    __shared__ u32 s_count;
    const u64 mine = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x;
    const u32 count = lzx_collect_long_rows(mine < n && row_ptr[mine + 1] - row_ptr[mine] > long_row, (u32)mine, s_rows, &s_count);
    for (u32 r = 0; r < count; ++r) {
        const u64 row = s_rows[r];
        paths_edges_of_row<B>(row, row_ptr[row] + (u64)blockIdx.y * LZX_MULTI_BLOCK + threadIdx.x, row_ptr[row + 1], LZX_MULTI_BLOCK * gridDim.y, col,
                              dist, sigma, g, b, ebc);
    }
}

// in [n][B] -> out [b][n]
template <u32 B, typename T>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK) k_paths_unpack(const T *in, u32 b, u64 n, T *out)
{
    const u64 i = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x;
    if (i >= n * B) return;
    const u32 c = (u32)(i % B);
    if (c < b) out[(u64)c * n + i / B] = in[i];
}

// ==================================================================================================== host
namespace {
struct PathsCall {
    const char *fn;
    uint32_t ns;
    const uint32_t *sources;   // null: vertex i is source i
    int32_t *dist;
    double *paths;
    uint64_t *reached, *sum_dist;
    double *harmonic;
    uint32_t *ecc;
    double *bc;                // non-null (or ebc): the backward pass runs
    lzx_bfs_info *info;
    double *ebc = nullptr;     // lzx_brandes_f64: the edge pass runs, and the backward pass keeps sigma
    bool endpoints = false;
    lzx_brandes_info *binfo = nullptr;
};

struct PathsState {
    int32_t *dist;
    double *sigma, *third, *bc, *part;
    u32 *part_row, *reached;
    double *delta, *ebc;       // the fourth [n][B] array (bc and ebc both wanted), ebc [nnz]
    long long *cnt;            // [n], the endpoints' count
    u32 lanes = 0;             // lanes per row of the edge pass
    u32 max_level = 0, sweeps = 0;
    double sweep_ms = 0.0, edge_ms = 0.0;
};

}   // namespace

template <u32 B, int MODE>
static int paths_level(lzx_ctx *c, const PathsState &s, u32 b, int32_t d)
{
    const lzx_multi_state *m = c->multi;
    const u64 n_waves = m->n_wl / (64 / B);
    if (n_waves)
        hipLaunchKernelGGL((k_paths_sweep<B, MODE>), dim3((u32)((n_waves + 3) / 4)), dim3(LZX_MULTI_BLOCK), 0, c->stream, m->d_wl, n_waves,
                           c->d_col_idx, s.part_row, s.dist, s.sigma, s.third, s.part, b, d, s.reached, s.delta);
    if (m->n_split)
        hipLaunchKernelGGL((k_paths_split<B, MODE>), dim3(grid_of((u64)m->n_split * B)), dim3(LZX_MULTI_BLOCK), 0, c->stream, s.part,
                           m->d_split_row, m->d_split_first, m->n_split, s.dist, s.sigma, s.third, b, d, s.reached, s.delta);
    LZX_HIP(hipGetLastError());
    return LZX_OK;
}

// one batch: sources first .. first + b - 1 of the call
template <u32 B>
static int paths_batch(lzx_ctx *c, const PathsCall &q, LzxGraphRun &run, PathsState &s, u32 first, u32 b)
{
    const u64 n = c->n, nB = n * B;
    hipStream_t st = c->stream;
    const dim3 blk(LZX_MULTI_BLOCK);
    PathsSources src{};
    for (u32 col = 0; col < b; ++col) src.v[col] = q.sources ? q.sources[first + col] : first + col;
    hipLaunchKernelGGL(k_paths_init<B>, dim3(grid_of(nB)), blk, 0, st, s.dist, s.sigma, n, b, src);
    LZX_HIP(hipGetLastError());
    LZX_HIP(hipMemsetAsync(s.reached, 0, sizeof(u32) * LZX_BFS_BATCH, st));

    // forward: the counters only grow; a level's share is the difference to the level before
    u32 seen[LZX_BFS_BATCH] = {}, ecc[LZX_BFS_BATCH] = {};
    u64 cnt[LZX_BFS_BATCH], sum[LZX_BFS_BATCH] = {};
    double harm[LZX_BFS_BATCH] = {};
    for (u32 col = 0; col < LZX_BFS_BATCH; ++col) cnt[col] = 1;
    u32 top = 0;
    for (u32 d = 1;; ++d) {
        if ((u64)d > n) LZX_FAIL(LZX_ERR_LIMIT, "%s: the search is still growing at level %u on %llu vertices", q.fn, d, (unsigned long long)n);
        LZX_HIP(hipEventRecord(run.ev0, st));
        LZX_TRY((paths_level<B, PATHS_FORWARD>(c, s, b, (int32_t)d)));
        LZX_HIP(hipEventRecord(run.ev1, st));
        u32 now[LZX_BFS_BATCH] = {};
        LZX_HIP(hipMemcpyAsync(now, s.reached, sizeof(u32) * B, hipMemcpyDeviceToHost, st));
        LZX_HIP(hipStreamSynchronize(st));
        float ms = 0.f;
        LZX_HIP(hipEventElapsedTime(&ms, run.ev0, run.ev1));
        s.sweep_ms += ms;
        ++s.sweeps;
        bool grew = false;
        for (u32 col = 0; col < b; ++col) {
            const u32 fresh = now[col] - seen[col];
            seen[col] = now[col];
            if (!fresh) continue;
            grew = true;
            cnt[col] += fresh;
            sum[col] += (u64)fresh * d;
            harm[col] += (double)fresh / (double)d;
            ecc[col] = d;
        }
        if (!grew) break;
        top = d;
    }
    s.max_level = std::max(s.max_level, top);
    for (u32 col = 0; col < b; ++col) {
        if (q.reached) q.reached[first + col] = cnt[col];
        if (q.sum_dist) q.sum_dist[first + col] = sum[col];
        if (q.harmonic) q.harmonic[first + col] = harm[col];
        if (q.ecc) q.ecc[first + col] = ecc[col];
    }

    // the n-vectors the caller asked for, [b][n] through the third array
    if (q.dist) {
        int32_t *stage = reinterpret_cast<int32_t *>(s.third);
        hipLaunchKernelGGL((k_paths_unpack<B, int32_t>), dim3(grid_of(nB)), blk, 0, st, s.dist, b, n, stage);
        LZX_HIP(hipGetLastError());
        LZX_HIP(hipMemcpyAsync(q.dist + (u64)first * n, stage, sizeof(int32_t) * b * n, hipMemcpyDeviceToHost, st));
    }
    if (q.paths) {
        hipLaunchKernelGGL((k_paths_unpack<B, double>), dim3(grid_of(nB)), blk, 0, st, s.sigma, b, n, s.third);
        LZX_HIP(hipGetLastError());
        LZX_HIP(hipMemcpyAsync(q.paths + (u64)first * n, s.third, sizeof(double) * b * n, hipMemcpyDeviceToHost, st));
    }
    if (q.dist || q.paths) LZX_HIP(hipStreamSynchronize(st));
    if (!q.bc && !q.ebc) return LZX_OK;

    // backward: nothing for the host to read between the levels
    const bool keep = q.ebc != nullptr;
    LZX_HIP(hipEventRecord(run.ev0, st));
    for (u32 d = top; d >= 1; --d) {
        if (keep) LZX_TRY((paths_level<B, PATHS_BACK_KEEP>(c, s, b, (int32_t)d)));
        else LZX_TRY((paths_level<B, PATHS_BACK>(c, s, b, (int32_t)d)));
        ++s.sweeps;
    }
    LZX_HIP(hipEventRecord(run.ev1, st));
    if (q.bc) {   // (a row the backward pass never wrote has dist <= 0 and is not read)
        hipLaunchKernelGGL(k_paths_accumulate<B>, dim3(grid_of(n)), blk, 0, st, s.dist, keep ? s.delta : s.sigma, n, b, s.bc);
        LZX_HIP(hipGetLastError());
    }
    if (q.endpoints) {
        PathsReached r{};
        for (u32 col = 0; col < b; ++col) r.v[col] = cnt[col];
        hipLaunchKernelGGL(k_paths_endpoints<B>, dim3(grid_of(n)), blk, 0, st, s.dist, n, b, r, s.cnt);
        LZX_HIP(hipGetLastError());
    }
    if (keep) {
        LZX_HIP(hipEventRecord(run.ev2, st));
        const u32 long_row = 64 * s.lanes;
        lzx_with_lanes<32>(s.lanes, [&](auto g) {
            hipLaunchKernelGGL((k_paths_edges<B, g>), dim3(lzx_row_grid(n, LZX_MULTI_BLOCK / g)), blk, 0, st, c->d_row_ptr, c->d_col_idx, s.dist,
                               s.sigma, s.third, n, b, long_row, s.ebc);
        });
        LZX_HIP(hipGetLastError());
        if (c->max_degree > long_row) {
            const u32 shares = (u32)std::min<u64>((c->max_degree + 2047) / 2048, 32);   // workgroups per long row
            hipLaunchKernelGGL(k_paths_edges_long<B>, dim3(grid_of(n), shares), blk, 0, st, c->d_row_ptr, c->d_col_idx, s.dist, s.sigma, s.third, n, b,
                               long_row, s.ebc);
            LZX_HIP(hipGetLastError());
        }
        LZX_HIP(hipEventRecord(run.ev3, st));
    }
    LZX_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    LZX_HIP(hipEventElapsedTime(&ms, run.ev0, run.ev1));
    s.sweep_ms += ms;
    if (keep) {
        LZX_HIP(hipEventElapsedTime(&ms, run.ev2, run.ev3));
        s.edge_ms += ms;
    }
    return LZX_OK;
}

static int paths_run(lzx_handle h, const PathsCall &q)
{
    const auto t0 = std::chrono::steady_clock::now();
    const char *fn = q.fn;
    // what needs no device
    if (q.ns == 0) LZX_FAIL(LZX_ERR_ARG, "%s: ns == 0", fn);
    lzx_ctx *c = h;
    LZX_TRY(lzx_graph_call_check(c, fn, "the search runs"));
    if (!q.sources && (u64)q.ns != c->n)
        LZX_FAIL(LZX_ERR_ARG, "%s: null sources mean every vertex: ns must be n = %llu, got %u", fn, (unsigned long long)c->n, q.ns);
    for (u32 i = 0; q.sources && i < q.ns; ++i)
        if ((u64)q.sources[i] >= c->n)
            LZX_FAIL(LZX_ERR_ARG, "%s: sources[%u] = %u is not a vertex (n = %llu)", fn, i, q.sources[i], (unsigned long long)c->n);
    LZX_TRY(lzx_multi_check_handle(c, fn));
    LZX_TRY(lzx_multi_build_tables(c));   // the one piece of the handle's state this call may add (kept, like lzx_spmm_f64's)

    const lzx_multi_state *m = c->multi;
    const u64 n = c->n;
    const u32 Bmax = lzx_multi_pad_width(std::min<u32>(q.ns, LZX_BFS_BATCH));
    const u64 nB = n * Bmax, b_ebc = q.ebc ? sizeof(double) * c->nnz : 0;
    const bool third = q.bc || q.ebc || q.dist || q.paths, fourth = q.bc && q.ebc;
    PathsState s{};
    LzxGraphRun run(c);
    char what[80];
    std::snprintf(what, sizeof what, "the state of %u interleaved columns on %llu vertices", Bmax, (ull)n);
    LZX_TRY(lzx_carve_state(fn, what, c->bfs_cap_opt, 0, &run.arena, nullptr, [&](LzxCarver &k) {
        k.take(s.dist, nB);
        k.align(16);
        k.take(s.sigma, nB);
        k.take_if(third, s.third, nB);
        k.take_if(fourth, s.delta, nB);
        k.take_if(q.bc != nullptr, s.bc, n);
        k.take_if(q.ebc != nullptr, s.ebc, c->nnz);
        k.take_if(q.endpoints, s.cnt, n);
        k.take(s.part, (u64)m->n_parts * Bmax);
        k.take(s.part_row, ((u64)m->n_parts + 3) & ~3ull);   // (16 bytes at a time)
        k.take(s.reached, LZX_BFS_BATCH);
    }));
    LZX_TRY(run.events(q.ebc ? 4 : 2));
    if (q.ebc) {
        s.lanes = lzx_lanes_per_row(c, c->nnz, 32);
        if (b_ebc) LZX_HIP(hipMemsetAsync(s.ebc, 0, b_ebc, c->stream));
    }
    if (q.endpoints) LZX_HIP(hipMemsetAsync(s.cnt, 0, sizeof(long long) * n, c->stream));
    if (m->n_split) {
        hipLaunchKernelGGL(k_paths_part_rows, dim3((m->n_split + 255) / 256), dim3(256), 0, c->stream, m->d_split_row, m->d_split_first, m->n_split, s.part_row);
        LZX_HIP(hipGetLastError());
    }
    if (q.bc) LZX_HIP(hipMemsetAsync(s.bc, 0, sizeof(double) * n, c->stream));

    u32 batches = 0;
    for (u32 first = 0; first < q.ns; first += LZX_BFS_BATCH, ++batches) {
        const u32 b = std::min<u32>(LZX_BFS_BATCH, q.ns - first);
        int rc;
        switch (lzx_multi_pad_width(b)) {
        case 2: rc = paths_batch<2>(c, q, run, s, first, b); break;
        case 4: rc = paths_batch<4>(c, q, run, s, first, b); break;
        case 8: rc = paths_batch<8>(c, q, run, s, first, b); break;
        default: rc = paths_batch<16>(c, q, run, s, first, b); break;
        }
        LZX_TRY(rc);
    }
    if (q.endpoints) {
        hipLaunchKernelGGL(k_paths_add_endpoints, dim3(grid_of(n)), dim3(LZX_MULTI_BLOCK), 0, c->stream, s.cnt, n, s.bc);
        LZX_HIP(hipGetLastError());
    }
    if (q.bc) LZX_HIP(hipMemcpyAsync(q.bc, s.bc, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    if (b_ebc) LZX_HIP(hipMemcpyAsync(q.ebc, s.ebc, b_ebc, hipMemcpyDeviceToHost, c->stream));
    if (q.bc || b_ebc) LZX_HIP(hipStreamSynchronize(c->stream));
    if (q.binfo) {
        q.binfo->ns = q.ns;
        q.binfo->batches = batches;
        q.binfo->max_level = s.max_level;
        q.binfo->sweeps = s.sweeps;
        q.binfo->sweep_ms = s.sweep_ms;
        q.binfo->edge_ms = s.edge_ms;
        q.binfo->loop_ms = lzx_ms_since(t0);
    }
    if (q.info) {
        q.info->ns = q.ns;
        q.info->batches = batches;
        q.info->max_level = s.max_level;
        q.info->sweeps = s.sweeps;
        q.info->sweep_ms = s.sweep_ms;
        q.info->loop_ms = lzx_ms_since(t0);
    }
    return LZX_OK;
}

extern "C" int lzx_bfs_multi(lzx_handle h, uint32_t ns, const uint32_t *sources, int32_t *dist, double *paths, uint64_t *reached,
                             uint64_t *sum_dist, double *harmonic, uint32_t *ecc, lzx_bfs_info *info)
{
    static const char *fn = "lzx_bfs_multi";
    if (ns > 0 && !sources) LZX_FAIL(LZX_ERR_ARG, "%s: null sources", fn);
    return paths_run(h, PathsCall{fn, ns, sources, dist, paths, reached, sum_dist, harmonic, ecc, nullptr, info});
}

extern "C" int lzx_betweenness_f64(lzx_handle h, uint32_t ns, const uint32_t *sources, double *bc, lzx_bfs_info *info)
{
    static const char *fn = "lzx_betweenness_f64";
    if (ns > 0 && !bc) LZX_FAIL(LZX_ERR_ARG, "%s: null bc", fn);
    return paths_run(h, PathsCall{fn, ns, sources, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, bc, info});
}

extern "C" int lzx_brandes_f64(lzx_handle h, uint32_t ns, const uint32_t *sources, uint32_t flags, double *bc, double *ebc, lzx_brandes_info *info)
{
    static const char *fn = "lzx_brandes_f64";
    if (ns == 0) LZX_FAIL(LZX_ERR_ARG, "%s: ns == 0", fn);
    if (!bc && !ebc) LZX_FAIL(LZX_ERR_ARG, "%s: null bc and null ebc: nothing is asked for", fn);
    if (flags & ~(uint32_t)LZX_BRANDES_ENDPOINTS) LZX_FAIL(LZX_ERR_ARG, "%s: unknown flag bits 0x%x", fn, flags & ~(uint32_t)LZX_BRANDES_ENDPOINTS);
    if ((flags & LZX_BRANDES_ENDPOINTS) && !bc) LZX_FAIL(LZX_ERR_ARG, "%s: LZX_BRANDES_ENDPOINTS with null bc: the endpoints count into bc", fn);
    PathsCall q{fn, ns, sources, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, bc, nullptr};
    q.ebc = ebc;
    q.endpoints = (flags & LZX_BRANDES_ENDPOINTS) != 0;
    q.binfo = info;
    return paths_run(h, q);
}
