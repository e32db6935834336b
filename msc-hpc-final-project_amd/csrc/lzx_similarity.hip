// lzx_similarity.hip -- how alike two vertices are: common neighbours, the Jaccard, overlap and Sorensen coefficients, the
// Adamic-Adar and resource-allocation indices, for a list of pairs or for every stored entry, on the device over the caller-order
// CSR the handle keeps (d_row_ptr / d_col_idx): include/lzx.h, lzx_similarity; DESIGN.md section 23.
//
// Definitions.  N(x) = row x without a diagonal entry, d_x = |N(x)|, c = |N(u) n N(v)|.  The stored rows are what is walked: a
// walked entry equal to u or to v is skipped, which takes out the diagonal entries and the edge u - v itself.
//
// Preparation.
//   k_tri_degrees     d_v, one thread per row (lzx_tri_orient.h)
//   k_sim_tables      only for a sum that is asked for: 1 / log d_v (0 where d_v < 2), 1 / d_v (0 where d_v < 1), fp64 -- a hit
//                     costs one 8-byte gather, no log runs in the walk
//   k_sim_edge_pairs  edges mode: entry e of row r becomes the pair (r, col_idx[e]); only the entries with u < v are intersected
//
// The walk (sim_walk).  The shorter stored row is walked -- on a tie in length the row of the smaller id, so (u, v) and (v, u)
// take the same path -- and the longer binary-searched.  A lane's entries ascend, so each search starts where the previous one
// ended.  Three paths by s = the walked row's length:
//   k_sim_short<G>    s <= long_pair (default 64 G): G lanes per pair, lane i takes the entries i, i + G, ...
//   k_sim_long        s > long_pair: a workgroup of 256 per listed pair, thread i takes i, i + 256, ...
//   k_sim_sliced      s > long_pair and s > slice (default 16384): the walked row in min(64, ceil(s / slice)) equal contiguous
//                     slices, a workgroup each; the partial count and sums go to a table, k_sim_slices_close adds them in slice
//                     order
// k_sim_classify counts the long and the sliced pairs (and, in block partials, the short ones and the entries walked); the host
// reads the two counts, sizes the lists and the table, and the same kernel fills the lists (lzx_wave_append: in no particular
// order, which no output depends on).
//
// Sums.  A lane adds its terms in ascending position; the lanes of a group or wavefront close with a fixed shuffle tree (every
// lane ends with the same bits); the four wavefronts of a workgroup are added in LDS as (w0 + w1) + (w2 + w3); slices in ascending
// order.  Each of these orders depends only on the two row lengths, on G and on the two thresholds: a pair's bits depend neither
// on the batch nor on its place in it.  There is no floating-point atomic.
//
// k_sim_finish closes: the mirror entries of edges mode copy what the entry with u < v holds (a binary search of u in row v),
// diagonal entries get 0, the three ratios are one correctly rounded division each, the degrees are gathered, the largest c is
// taken per wavefront and then by one atomicMax.  All atomics (two list tails, the maximum) are 32-bit integer vector atomics.  No
// kernel waits on another workgroup; every walk is bounded by a row length.
#include <algorithm>
#include <chrono>
#include <vector>

#include "lzx_internal.h"
#include "lzx_graph_call.h"
#include "lzx_tri_orient.h"
#include "lzx_spmv_body.h"
#include "lzx_reduce.h"

static constexpr u32 LZX_SIM_BLOCK = 256;
static constexpr u32 LZX_SIM_SLICE = 16384;     // entries per slice of a walked row that several workgroups share (test shape sim_slice)
static constexpr u32 LZX_SIM_SLICES = 64;       // workgroups such a row is dealt to (at most)
static constexpr u32 LZX_SIM_STAT_GRID = 1024;  // workgroups of the classification = block partials of its statistics (at most)
static constexpr u32 LZX_SIM_LIST_GRID = 1u << 20;   // workgroups of a launch over a list of pairs (at most; they stride over it)
static constexpr u32 LZX_SIM_MEASURES = LZX_SIM_JACCARD | LZX_SIM_OVERLAP | LZX_SIM_SORENSEN | LZX_SIM_ADAMIC_ADAR | LZX_SIM_RESOURCE_ALLOCATION;
static_assert(LZX_SIM_BLOCK == LZX_TRI_BLOCK, "k_tri_degrees is launched with this file's grid");

enum : u32 { SIM_NONE = 0, SIM_SHORT = 1, SIM_LONG = 2, SIM_SLICED = 3 };

// what the walks work on
struct SimArgs {
    const u64 *row_ptr;
    const u32 *col_idx, *pu, *pv;
    const double *tab_aa, *tab_ra;   // 1 / log d, 1 / d; nullptr: that sum is not asked for
    u32 *common;                     // [np]
    double *out_aa, *out_ra;         // [np] each, or nullptr
    u32 np, long_pair, slice, edges_mode;
};

// pair p: S the walked row, L the searched one
struct SimRows {
    const u32 *S, *L;
    u32 ls, ll, u, v, path;
};

struct SimAcc {
    u32 c;
    double aa, ra;
};

__device__ __forceinline__ SimRows sim_rows(const SimArgs &a, u32 p)
{
    SimRows r;
    r.u = a.pu[p];
    r.v = a.pv[p];
    const u64 bu = a.row_ptr[r.u], bv = a.row_ptr[r.v];
    const u32 lu = (u32)(a.row_ptr[r.u + 1] - bu), lv = (u32)(a.row_ptr[r.v + 1] - bv);
    const bool walk_u = lu < lv || (lu == lv && r.u < r.v);
    r.S = a.col_idx + (walk_u ? bu : bv);
    r.L = a.col_idx + (walk_u ? bv : bu);
    r.ls = walk_u ? lu : lv;
    r.ll = walk_u ? lv : lu;
    if (a.edges_mode && r.u >= r.v) r.path = SIM_NONE;   // the mirror entry, a diagonal entry: k_sim_finish
    else r.path = r.ls <= a.long_pair ? SIM_SHORT : (r.ls <= a.slice ? SIM_LONG : SIM_SLICED);
    return r;
}

// the slices of a walked row of ls entries: how many, and their length
__device__ __forceinline__ u32 sim_slices(u32 ls, u32 slice) { return (u32)min((u64)LZX_SIM_SLICES, ((u64)ls + slice - 1) / slice); }
__device__ __forceinline__ u32 sim_slice_len(u32 ls, u32 ns) { return (u32)(((u64)ls + ns - 1) / ns); }

// first position in the ascending list[lo .. hi) whose entry is >= x (hi when there is none)
__device__ __forceinline__ u32 sim_lower_bound(const u32 *list, u32 lo, u32 hi, u32 x)
{
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (list[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the entries first, first + stride, ... below end of the walked row, in that order
__device__ __forceinline__ void sim_walk(const SimArgs &a, const SimRows &r, u64 first, u64 end, u32 stride, SimAcc &acc)
{
    u32 lo = 0;
    for (u64 j = first; j < end; j += stride) {
        const u32 x = r.S[j];
        if (x == r.u || x == r.v) continue;
        const u32 at = sim_lower_bound(r.L, lo, r.ll, x);
        lo = at;   // (the next x is larger)
        if (at < r.ll && r.L[at] == x) {
            ++acc.c;
            if (a.tab_aa) acc.aa += a.tab_aa[x];
            if (a.tab_ra) acc.ra += a.tab_ra[x];
        }
    }
}

template <u32 G>
__device__ __forceinline__ double sim_group_sum(double v)
{
#pragma unroll
    for (u32 o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, (int)o, 64);
    return v;   // every lane of the group holds the same bits
}

// the workgroup's total in its thread 0 (every thread must call it; s_*: one place per wavefront)
__device__ __forceinline__ SimAcc sim_block_sum(SimAcc acc, u32 *s_c, double *s_aa, double *s_ra)
{
    acc.c = lzx_wave_sum_u32(acc.c);
    acc.aa = wave_sum(acc.aa);
    acc.ra = wave_sum(acc.ra);
    if ((threadIdx.x & 63) == 0) {
        s_c[threadIdx.x >> 6] = acc.c;
        s_aa[threadIdx.x >> 6] = acc.aa;
        s_ra[threadIdx.x >> 6] = acc.ra;
    }
    __syncthreads();
    SimAcc t;
    t.c = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
    t.aa = (s_aa[0] + s_aa[1]) + (s_aa[2] + s_aa[3]);
    t.ra = (s_ra[0] + s_ra[1]) + (s_ra[2] + s_ra[3]);
    __syncthreads();
    return t;
}

__device__ __forceinline__ void sim_store(const SimArgs &a, u32 p, const SimAcc &t)
{
    a.common[p] = t.c;
    if (a.out_aa) a.out_aa[p] = t.aa;
    if (a.out_ra) a.out_ra[p] = t.ra;
}

// ---- preparation ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LZX_SIM_BLOCK) k_sim_tables(const u32 *deg, u32 n, double *tab_aa, double *tab_ra)
{
    const u64 v = (u64)blockIdx.x * LZX_SIM_BLOCK + threadIdx.x;
    if (v >= n) return;
    const u32 d = deg[v];
    if (tab_aa) tab_aa[v] = d < 2 ? 0.0 : 1.0 / log((double)d);
    if (tab_ra) tab_ra[v] = d < 1 ? 0.0 : 1.0 / (double)d;
}

template <u32 G>
__global__ void __launch_bounds__(LZX_SIM_BLOCK) k_sim_edge_pairs(const u64 *row_ptr, const u32 *col_idx, u32 n, u32 *pu, u32 *pv)
{
    const u32 sub = threadIdx.x & (G - 1);
    const u64 row = (u64)blockIdx.x * (LZX_SIM_BLOCK / G) + threadIdx.x / G;
    if (row >= n) return;
    const u64 end = row_ptr[row + 1];
    for (u64 e = row_ptr[row] + sub; e < end; e += G) {
        pu[e] = (u32)row;
        pv[e] = col_idx[e];
    }
}

// ---- classification ---------------------------------------------------------------------------------------------------------------
// tails[0] / tails[1]: the long / the sliced pairs.  list_long == nullptr: they are counted, and part[2 b], part[2 b + 1] = the
// entries walked and the short pairs of workgroup b's share; otherwise they are listed (the tails start at 0 again).
__global__ void __launch_bounds__(LZX_SIM_BLOCK) k_sim_classify(SimArgs a, u32 *tails, u32 *list_long, u32 *list_sliced, u32 cap_long, u32 cap_sliced, ull *part)
{
    __shared__ ull s_w[LZX_SIM_BLOCK / 64], s_s[LZX_SIM_BLOCK / 64];
    ull walked = 0, shorts = 0;
    // (the same trips for every thread of the workgroup: the appends are formed per wavefront)
    for (u64 p0 = (u64)blockIdx.x * LZX_SIM_BLOCK; p0 < a.np; p0 += (u64)gridDim.x * LZX_SIM_BLOCK) {
        const u64 p = p0 + threadIdx.x;
        u32 path = SIM_NONE;
        if (p < a.np) {
            const SimRows r = sim_rows(a, (u32)p);
            path = r.path;
            if (path != SIM_NONE) walked += r.ls;
            if (path == SIM_SHORT) ++shorts;
        }
        if (list_long) {
            const u32 at_l = lzx_wave_append(path == SIM_LONG, &tails[0]);
            if (path == SIM_LONG && at_l < cap_long) list_long[at_l] = (u32)p;
            const u32 at_s = lzx_wave_append(path == SIM_SLICED, &tails[1]);
            if (path == SIM_SLICED && at_s < cap_sliced) list_sliced[at_s] = (u32)p;
        } else {
            const ull ml = __ballot(path == SIM_LONG), ms = __ballot(path == SIM_SLICED);
            if ((threadIdx.x & 63) == 0) {
                if (ml) atomicAdd(&tails[0], (u32)__builtin_popcountll(ml));
                if (ms) atomicAdd(&tails[1], (u32)__builtin_popcountll(ms));
            }
        }
    }
    if (list_long) return;
    walked = wave_sum_u64(walked);
    shorts = wave_sum_u64(shorts);
    if ((threadIdx.x & 63) == 0) {
        s_w[threadIdx.x >> 6] = walked;
        s_s[threadIdx.x >> 6] = shorts;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        part[2 * blockIdx.x + 1] = s_s[0] + s_s[1] + s_s[2] + s_s[3];
    }
}

// ---- the three paths --------------------------------------------------------------------------------------------------------------
template <u32 G>
__global__ void __launch_bounds__(LZX_SIM_BLOCK) k_sim_short(SimArgs a)
{
    const u32 sub = threadIdx.x & (G - 1);
    const u64 p = (u64)blockIdx.x * (LZX_SIM_BLOCK / G) + threadIdx.x / G;
    SimRows r = {nullptr, nullptr, 0, 0, 0, 0, SIM_NONE};
    if (p < a.np) r = sim_rows(a, (u32)p);
    const bool mine = r.path == SIM_SHORT;
    SimAcc acc = {0, 0.0, 0.0};
    sim_walk(a, r, sub, mine ? r.ls : 0u, G, acc);
    acc.c = lzx_group_sum_u32<G>(acc.c);
    acc.aa = sim_group_sum<G>(acc.aa);
    acc.ra = sim_group_sum<G>(acc.ra);
    if (mine && sub == 0) sim_store(a, (u32)p, acc);
}

// the listed pairs, a workgroup per pair (the workgroups stride over the list)
__global__ void __launch_bounds__(LZX_SIM_BLOCK) k_sim_long(SimArgs a, const u32 *list, u32 count)
{
    __shared__ u32 s_c[LZX_SIM_BLOCK / 64];
    __shared__ double s_aa[LZX_SIM_BLOCK / 64], s_ra[LZX_SIM_BLOCK / 64];
    for (u32 i = blockIdx.x; i < count; i += gridDim.x) {   // (the same trips for every thread of the workgroup)
        const u32 p = list[i];
        if (p >= a.np) continue;   // (the same for every thread)
        const SimRows r = sim_rows(a, p);
        SimAcc acc = {0, 0.0, 0.0};
        sim_walk(a, r, threadIdx.x, r.ls, LZX_SIM_BLOCK, acc);
        const SimAcc t = sim_block_sum(acc, s_c, s_aa, s_ra);
        if (threadIdx.x == 0) sim_store(a, p, t);
    }
}

// the listed pairs, a workgroup per (pair, slice of its walked row): blockIdx.y is the slice; pc / paa / pra: [count][64]
__global__ void __launch_bounds__(LZX_SIM_BLOCK) k_sim_sliced(SimArgs a, const u32 *list, u32 count, u32 *pc, double *paa, double *pra)
{
    __shared__ u32 s_c[LZX_SIM_BLOCK / 64];
    __shared__ double s_aa[LZX_SIM_BLOCK / 64], s_ra[LZX_SIM_BLOCK / 64];
    for (u32 i = blockIdx.x; i < count; i += gridDim.x) {   // (the same trips for every thread of the workgroup)
        const u32 p = list[i];
        if (p >= a.np) continue;   // (the same for every thread)
        const SimRows r = sim_rows(a, p);
        const u32 ns = sim_slices(r.ls, a.slice);
        if (blockIdx.y >= ns) continue;
        const u32 len = sim_slice_len(r.ls, ns);
        const u64 beg = (u64)blockIdx.y * len, end = min((u64)r.ls, beg + len);
        SimAcc acc = {0, 0.0, 0.0};
        sim_walk(a, r, beg + threadIdx.x, end, LZX_SIM_BLOCK, acc);
        const SimAcc t = sim_block_sum(acc, s_c, s_aa, s_ra);
        if (threadIdx.x == 0) {
            const u64 at = (u64)i * LZX_SIM_SLICES + blockIdx.y;
            pc[at] = t.c;
            paa[at] = t.aa;
            pra[at] = t.ra;
        }
    }
}

// one thread per sliced pair: its slices in ascending order
__global__ void __launch_bounds__(LZX_SIM_BLOCK) k_sim_slices_close(SimArgs a, const u32 *list, u32 count, const u32 *pc, const double *paa, const double *pra)
{
    const u64 i = (u64)blockIdx.x * LZX_SIM_BLOCK + threadIdx.x;
    if (i >= count) return;
    const u32 p = list[i];
    if (p >= a.np) return;
    const u32 ns = sim_slices(sim_rows(a, p).ls, a.slice);
    SimAcc t = {0, 0.0, 0.0};
    for (u32 k = 0; k < ns; ++k) {
        const u64 at = i * LZX_SIM_SLICES + k;
        t.c += pc[at];
        t.aa += paa[at];
        t.ra += pra[at];
    }
    sim_store(a, p, t);
}

// ---- the closing launch -----------------------------------------------------------------------------------------------------------
// values: [popcount(measures)][np] in ascending order of the flags (the rows of the two sums are a.out_aa / a.out_ra)
__global__ void __launch_bounds__(LZX_SIM_BLOCK) k_sim_finish(SimArgs a, const u32 *deg, u32 measures, double *values, u32 *dgu, u32 *dgv, u32 *max_c)
{
    const u64 p = (u64)blockIdx.x * LZX_SIM_BLOCK + threadIdx.x;
    u32 c = 0;
    if (p < a.np) {
        const u32 u = a.pu[p], v = a.pv[p];
        u32 du = deg[u], dv = deg[v];
        if (a.edges_mode && u >= v) {
            SimAcc t = {0, 0.0, 0.0};
            if (u > v) {   // the mirror entry: what entry (v, u) holds
                const u64 bv = a.row_ptr[v];
                const u32 lv = (u32)(a.row_ptr[v + 1] - bv);
                const u32 at = lzx_lower_bound(a.col_idx + bv, lv, u);
                if (at < lv && a.col_idx[bv + at] == u) {
                    const u64 q = bv + at;
                    t.c = a.common[q];
                    if (a.out_aa) t.aa = a.out_aa[q];
                    if (a.out_ra) t.ra = a.out_ra[q];
                }
            } else du = dv = 0;   // a diagonal entry
            sim_store(a, (u32)p, t);
            c = t.c;
        } else c = a.common[p];
        if (dgu) dgu[p] = du;
        if (dgv) dgv[p] = dv;
        double *row = values + p;
        if (measures & LZX_SIM_JACCARD) {
            const u64 den = (u64)du + dv - c;
            *row = den ? (double)c / (double)den : 0.0;
            row += a.np;
        }
        if (measures & LZX_SIM_OVERLAP) {
            const u32 den = min(du, dv);
            *row = den ? (double)c / (double)den : 0.0;
            row += a.np;
        }
        if (measures & LZX_SIM_SORENSEN) {
            const u64 den = (u64)du + dv;
            *row = den ? (double)(2 * (u64)c) / (double)den : 0.0;
        }
    }
    u32 mx = c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (u32)__shfl_xor((int)mx, o, 64));
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(max_c, mx);
}

extern "C" int lzx_similarity(lzx_handle c, uint64_t np64, const uint32_t *u, const uint32_t *v, uint32_t measures, uint32_t *common, uint32_t *deg_u,
                              uint32_t *deg_v, double *values, lzx_similarity_info *info)
{
    const char *fn_name = "lzx_similarity";
    LZX_TRY(lzx_graph_call_check(c, fn_name, "pairs of vertices are compared"));
    const auto t0 = std::chrono::steady_clock::now();
    const u32 n = (u32)c->n;
    const u64 nnz = c->nnz;
    if (measures & ~LZX_SIM_MEASURES) LZX_FAIL(LZX_ERR_ARG, "%s: measures = 0x%x has a bit that is no measure (known: 0x%x)", fn_name, measures, LZX_SIM_MEASURES);
    if (measures && !values) LZX_FAIL(LZX_ERR_ARG, "%s: measures = 0x%x, but values is null", fn_name, measures);
    if ((u == nullptr) != (v == nullptr)) LZX_FAIL(LZX_ERR_ARG, "%s: u and v are both given (pairs) or both null (every stored entry)", fn_name);
    const bool edges_mode = u == nullptr;
    if (edges_mode && np64 != nnz)
        LZX_FAIL(LZX_ERR_ARG, "%s: without pairs there is one output per stored entry: np = %llu, but the graph has %llu entries", fn_name, (ull)np64, (ull)nnz);
    if (np64 >= 0xffffffffull) LZX_FAIL(LZX_ERR_LIMIT, "%s: %llu pairs; pair indices are 32-bit (fewer than 2^32 - 1 pairs)", fn_name, (ull)np64);
    const u32 np = (u32)np64;
    if (!edges_mode)
        for (u32 p = 0; p < np; ++p) {
            if (u[p] >= n || v[p] >= n) LZX_FAIL(LZX_ERR_ARG, "%s: pair %u is (%u, %u), but the graph has %u vertices", fn_name, p, u[p], v[p], n);
            if (u[p] == v[p]) LZX_FAIL(LZX_ERR_ARG, "%s: pair %u is (%u, %u): a vertex is not compared with itself", fn_name, p, u[p], v[p]);
        }
    if (info) {
        *info = lzx_similarity_info{};
        info->pairs = np;
    }
    if (np == 0) {
        if (info) info->loop_ms = lzx_ms_since(t0);
        return LZX_OK;
    }

    const bool want_aa = measures & LZX_SIM_ADAMIC_ADAR, want_ra = measures & LZX_SIM_RESOURCE_ALLOCATION;
    const u32 nsums = (want_aa ? 1u : 0u) + (want_ra ? 1u : 0u);
    const u32 nm = (u32)__builtin_popcount(measures);
    const u64 np_al = lzx_even(np);
    LZX_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    double *d_tab_aa, *d_tab_ra, *d_values, *d_out_aa, *d_out_ra;
    ull *d_part;
    u32 *d_deg, *d_pu, *d_pv, *d_common, *d_dgu, *d_dgv, *d_tails, *d_max;
    u64 bytes = 0;
    LzxGraphRun run(c);   // more[0]: the lists of long and sliced pairs and the slices' table
    char what[200];
    std::snprintf(what, sizeof what, "the state of %u vertices and %u pairs (degrees, %u tables, pairs, counts, %u measures)", n, np, nsums, nm);
    LZX_TRY(lzx_carve_state(fn_name, what, c->sim_cap_opt, 0, &run.arena, &bytes, [&](LzxCarver &k) {
        k.take_if(want_aa, d_tab_aa, n);   // a table per sum
        k.take_if(want_ra, d_tab_ra, n);
        // the values [nm][np] begin here.  Their rows: the ratios asked for, then Adamic-Adar, then resource allocation -- the
        // flags' ascending order
        k.take(d_values, (u64)(nm - nsums) * np);
        k.take_if(want_aa, d_out_aa, np);
        k.take_if(want_ra, d_out_ra, np);
        k.take(d_part, 2 * LZX_SIM_STAT_GRID);   // the block partials
        k.take(d_deg, lzx_even(n));
        for (u32 **p : {&d_pu, &d_pv, &d_common}) k.take(*p, np_al);
        k.take_if(deg_u != nullptr, d_dgu, np_al);
        k.take_if(deg_v != nullptr, d_dgv, np_al);
        k.take(d_tails, 2);
        k.take(d_max, 2);   // the maximum, a spare
    }));
    LZX_TRY(run.events(4));

    // ---- preparation ----
    const u32 G = lzx_lanes_per_row(c, nnz, 32);
    const u32 gb = (n + LZX_SIM_BLOCK - 1) / LZX_SIM_BLOCK;
    const u32 gp = (u32)(((u64)np + LZX_SIM_BLOCK - 1) / LZX_SIM_BLOCK);
    LZX_HIP(hipEventRecord(run.ev0, st));
    LZX_HIP(hipMemsetAsync(d_tails, 0, 4 * sizeof(u32), st));   // (the tails and the maximum)
    hipLaunchKernelGGL(k_tri_degrees, dim3(gb), dim3(LZX_TRI_BLOCK), 0, st, c->d_row_ptr, c->d_col_idx, d_deg, n);
    LZX_HIP(hipGetLastError());
    if (nsums) {
        hipLaunchKernelGGL(k_sim_tables, dim3(gb), dim3(LZX_SIM_BLOCK), 0, st, d_deg, n, d_tab_aa, d_tab_ra);
        LZX_HIP(hipGetLastError());
    }
    if (edges_mode) {
        lzx_with_lanes<32>(G, [&](auto g) {
            hipLaunchKernelGGL(k_sim_edge_pairs<g>, dim3(lzx_row_grid(n, LZX_SIM_BLOCK / g)), dim3(LZX_SIM_BLOCK), 0, st, c->d_row_ptr, c->d_col_idx, n, d_pu, d_pv);
        });
        LZX_HIP(hipGetLastError());
    } else {
        LZX_HIP(hipMemcpyAsync(d_pu, u, sizeof(u32) * np, hipMemcpyHostToDevice, st));
        LZX_HIP(hipMemcpyAsync(d_pv, v, sizeof(u32) * np, hipMemcpyHostToDevice, st));
    }
    LZX_HIP(hipEventRecord(run.ev1, st));

    // ---- classification: the counts, then the lists ----
    const u32 long_pair = lzx_shape_or(c->sim_long_opt, 64 * G);
    const u32 slice = lzx_shape_or(c->sim_slice_opt, LZX_SIM_SLICE);
    SimArgs a = {c->d_row_ptr, c->d_col_idx, d_pu, d_pv, d_tab_aa, d_tab_ra, d_common, d_out_aa, d_out_ra, np, long_pair, slice, edges_mode ? 1u : 0u};
    const u32 gs = std::min<u32>(LZX_SIM_STAT_GRID, gp);
    LZX_HIP(hipEventRecord(run.ev2, st));
    hipLaunchKernelGGL(k_sim_classify, dim3(gs), dim3(LZX_SIM_BLOCK), 0, st, a, d_tails, (u32 *)nullptr, (u32 *)nullptr, 0u, 0u, d_part);
    LZX_HIP(hipGetLastError());
    u32 tails[2] = {0, 0};
    std::vector<ull> parts(2 * (size_t)gs, 0);
    LZX_HIP(hipMemcpyAsync(tails, d_tails, sizeof(tails), hipMemcpyDeviceToHost, st));
    LZX_HIP(hipMemcpyAsync(parts.data(), d_part, sizeof(ull) * 2 * gs, hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    const u32 n_long = std::min(tails[0], np), n_sliced = std::min(tails[1], np - n_long);
    u64 walked = 0, n_short = 0;
    for (u32 i = 0; i < gs; ++i) {
        walked += parts[2 * i];
        n_short += parts[2 * i + 1];
    }
    u32 *d_list_long = nullptr, *d_list_sliced = nullptr, *d_pc = nullptr;
    double *d_paa = nullptr, *d_pra = nullptr;
    if (n_long + n_sliced) {
        const u64 cells = (u64)n_sliced * LZX_SIM_SLICES;   // of the slices' table
        std::snprintf(what, sizeof what, "the state of %u vertices and %u pairs (%u of them on a workgroup each, %u in slices)", n, np, n_long, n_sliced);
        LZX_TRY(lzx_carve_state(fn_name, what, c->sim_cap_opt, bytes, &run.more[0], nullptr, [&](LzxCarver &k) {
            k.take(d_paa, cells);
            k.take(d_pra, cells);
            k.take(d_pc, cells);
            k.take(d_list_sliced, n_sliced);
            k.take(d_list_long, n_long);
        }));
        LZX_HIP(hipMemsetAsync(d_tails, 0, 2 * sizeof(u32), st));
        hipLaunchKernelGGL(k_sim_classify, dim3(gs), dim3(LZX_SIM_BLOCK), 0, st, a, d_tails, d_list_long, d_list_sliced, n_long, n_sliced, d_part);
        LZX_HIP(hipGetLastError());
    }

    // ---- the walks ----
    if (n_short) {
        lzx_with_lanes<32>(G, [&](auto g) {
            hipLaunchKernelGGL(k_sim_short<g>, dim3(lzx_row_grid(np, LZX_SIM_BLOCK / g)), dim3(LZX_SIM_BLOCK), 0, st, a);
        });
        LZX_HIP(hipGetLastError());
    }
    if (n_long) {
        hipLaunchKernelGGL(k_sim_long, dim3(std::min(n_long, LZX_SIM_LIST_GRID)), dim3(LZX_SIM_BLOCK), 0, st, a, d_list_long, n_long);
        LZX_HIP(hipGetLastError());
    }
    if (n_sliced) {
        hipLaunchKernelGGL(k_sim_sliced, dim3(std::min(n_sliced, LZX_SIM_LIST_GRID), LZX_SIM_SLICES), dim3(LZX_SIM_BLOCK), 0, st, a, d_list_sliced, n_sliced,
                           d_pc, d_paa, d_pra);
        LZX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_sim_slices_close, dim3((n_sliced + LZX_SIM_BLOCK - 1) / LZX_SIM_BLOCK), dim3(LZX_SIM_BLOCK), 0, st, a, d_list_sliced, n_sliced,
                           d_pc, d_paa, d_pra);
        LZX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_sim_finish, dim3(gp), dim3(LZX_SIM_BLOCK), 0, st, a, d_deg, measures, d_values, d_dgu, d_dgv, d_max);
    LZX_HIP(hipGetLastError());
    LZX_HIP(hipEventRecord(run.ev3, st));

    // ---- hand back ----
    u32 max_c = 0;
    LZX_HIP(hipMemcpyAsync(&max_c, d_max, sizeof(u32), hipMemcpyDeviceToHost, st));
    if (common) LZX_HIP(hipMemcpyAsync(common, d_common, sizeof(u32) * np, hipMemcpyDeviceToHost, st));
    if (deg_u) LZX_HIP(hipMemcpyAsync(deg_u, d_dgu, sizeof(u32) * np, hipMemcpyDeviceToHost, st));
    if (deg_v) LZX_HIP(hipMemcpyAsync(deg_v, d_dgv, sizeof(u32) * np, hipMemcpyDeviceToHost, st));
    if (nm) LZX_HIP(hipMemcpyAsync(values, d_values, sizeof(double) * (u64)nm * np, hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    float prep_ms = 0.f, count_ms = 0.f;
    LZX_HIP(hipEventElapsedTime(&prep_ms, run.ev0, run.ev1));
    LZX_HIP(hipEventElapsedTime(&count_ms, run.ev2, run.ev3));
    if (info) {
        info->walked = walked;
        info->short_pairs = n_short;
        info->long_pairs = n_long;
        info->sliced_pairs = n_sliced;
        info->max_common = max_c;
        info->lanes = G;
        info->prep_ms = prep_ms;
        info->count_ms = count_ms;
        info->loop_ms = lzx_ms_since(t0);
    }
    return LZX_OK;
}
