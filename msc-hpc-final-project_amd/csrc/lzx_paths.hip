// lzx_paths.hip -- path-based centralities on the device: breadth-first search from many sources at once, and Brandes'
// betweenness on top of it (include/lzx.h: lzx_bfs_multi, lzx_betweenness_f64).
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

// what a complete row sum s does to (row, column) i; forward: 1 if the vertex was reached at this level
template <bool BACK>
__device__ __forceinline__ u32 paths_epilogue(u64 i, double s, int32_t d, int32_t *dist, double *sigma, double *g)
{
    if (BACK) {
        const double sg = sigma[i];
        const double delta = sg * s;
        g[i] = (1.0 + delta) / sg;
        sigma[i] = delta;
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
template <u32 B, bool BACK>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK)
k_paths_sweep(const uint4 *__restrict__ wl, u64 n_waves, const u32 *__restrict__ col, const u32 *__restrict__ part_row, int32_t *dist,
              double *sigma, double *g, double *part, u32 b, int32_t d, u32 *reached)
{
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
        else newly = paths_epilogue<BACK>(at, acc, d, dist, sigma, g);
    }
    if (!BACK) paths_count<B>(newly, reached);
}

// split rows: the chunk totals added in chunk order, then the same epilogue; thread (split row, column)
template <u32 B, bool BACK>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK)
k_paths_split(const double *part, const u32 *__restrict__ split_row, const u32 *__restrict__ split_first, u32 n_split, int32_t *dist,
              double *sigma, double *g, u32 b, int32_t d, u32 *reached)
{
    const u64 i = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x;
    const u64 ks = i / B;
    const u32 c = (u32)(i % B);
    u32 newly = 0;
    if (ks < n_split && c < b) {
        const u64 at = (u64)split_row[ks] * B + c;
        if (dist[at] == (BACK ? d : -1)) {
            double acc = 0.0;
            for (u32 p = split_first[ks]; p < split_first[ks + 1]; ++p) acc += part[(u64)p * B + c];
            newly = paths_epilogue<BACK>(at, acc, d, dist, sigma, g);
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
    double *bc;                // non-null: the backward pass runs
    lzx_bfs_info *info;
};

struct PathsState {
    int32_t *dist;
    double *sigma, *third, *bc, *part;
    u32 *part_row, *reached;
    u32 max_level = 0, sweeps = 0;
    double sweep_ms = 0.0;
};

u64 round16(u64 bytes) { return (bytes + 15) & ~15ull; }
}   // namespace

template <u32 B, bool BACK>
static int paths_level(lzx_ctx *c, const PathsState &s, u32 b, int32_t d)
{
    const lzx_multi_state *m = c->multi;
    const u64 n_waves = m->n_wl / (64 / B);
    if (n_waves)
        hipLaunchKernelGGL((k_paths_sweep<B, BACK>), dim3((u32)((n_waves + 3) / 4)), dim3(LZX_MULTI_BLOCK), 0, c->stream, m->d_wl, n_waves,
                           c->d_col_idx, s.part_row, s.dist, s.sigma, s.third, s.part, b, d, s.reached);
    if (m->n_split)
        hipLaunchKernelGGL((k_paths_split<B, BACK>), dim3(grid_of((u64)m->n_split * B)), dim3(LZX_MULTI_BLOCK), 0, c->stream, s.part,
                           m->d_split_row, m->d_split_first, m->n_split, s.dist, s.sigma, s.third, b, d, s.reached);
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
        LZX_TRY((paths_level<B, false>(c, s, b, (int32_t)d)));
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
    if (!q.bc) return LZX_OK;

    // backward: nothing for the host to read between the levels
    LZX_HIP(hipEventRecord(run.ev0, st));
    for (u32 d = top; d >= 1; --d) {
        LZX_TRY((paths_level<B, true>(c, s, b, (int32_t)d)));
        ++s.sweeps;
    }
    LZX_HIP(hipEventRecord(run.ev1, st));
    hipLaunchKernelGGL(k_paths_accumulate<B>, dim3(grid_of(n)), blk, 0, st, s.dist, s.sigma, n, b, s.bc);
    LZX_HIP(hipGetLastError());
    LZX_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    LZX_HIP(hipEventElapsedTime(&ms, run.ev0, run.ev1));
    s.sweep_ms += ms;
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
    const bool third = q.bc || q.dist || q.paths;
    const u64 b_dist = round16(sizeof(int32_t) * n * Bmax), b_vec = sizeof(double) * n * Bmax, b_bc = q.bc ? sizeof(double) * n : 0;
    const u64 b_part = sizeof(double) * (u64)m->n_parts * Bmax, b_prow = round16(sizeof(u32) * (u64)m->n_parts);
    const u64 bytes = b_dist + b_vec * (third ? 2 : 1) + b_bc + b_part + b_prow + sizeof(u32) * LZX_BFS_BATCH;
    LzxGraphRun run(c);
    char what[80];
    std::snprintf(what, sizeof what, "the state of %u interleaved columns on %llu vertices", Bmax, (ull)n);
    LZX_TRY(lzx_alloc_state(fn, what, c->bfs_cap_opt, bytes, bytes, &run.arena));
    PathsState s{};
    char *p = static_cast<char *>(run.arena);
    s.dist = reinterpret_cast<int32_t *>(p); p += b_dist;
    s.sigma = reinterpret_cast<double *>(p); p += b_vec;
    s.third = third ? reinterpret_cast<double *>(p) : nullptr; p += third ? b_vec : 0;
    s.bc = q.bc ? reinterpret_cast<double *>(p) : nullptr; p += b_bc;
    s.part = reinterpret_cast<double *>(p); p += b_part;
    s.part_row = reinterpret_cast<u32 *>(p); p += b_prow;
    s.reached = reinterpret_cast<u32 *>(p);
    LZX_HIP(hipEventCreate(&run.ev0));
    LZX_HIP(hipEventCreate(&run.ev1));
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
    if (q.bc) {
        LZX_HIP(hipMemcpyAsync(q.bc, s.bc, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        LZX_HIP(hipStreamSynchronize(c->stream));
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
