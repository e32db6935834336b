// lzx_sweep.hip -- sweep cuts of the handle's graph: up to 16 score vectors are each turned into an order of the vertices, the
// cut and the volume of every prefix of that order, and the prefix of least conductance (or edge expansion) in a window, on the
// device over the caller-order CSR the handle keeps (d_row_ptr / d_col_idx): include/lzx.h, lzx_sweep_cut; DESIGN.md section 22.
//
// Definitions.  d_v = the entries of row v without the diagonal, M = the sum of the d_v; a diagonal entry is skipped in every walk.
//   key      s_v, or s_v / (double)d_v with LZX_SWEEP_PER_DEGREE (then a vertex with d_v = 0 comes after all others); -0.0 is +0.0
//   order    descending key (ascending with LZX_SWEEP_ASCENDING), ties by ascending id; pos = the inverse of order
//   profile  vol[k-1] = the sum of d over the first k vertices; b_v = the neighbours u != v with pos[u] < pos[v];
//            cut[k-1] = the sum of d_v - 2 b_v over the first k vertices = the edges that leave the prefix
//   best     the k of [k_min, k_max] that minimises cut_k / den_k, den_k = min(vol_k, M - vol_k) (min(k, n - k) with
//            LZX_SWEEP_EXPANSION), prefixes with den_k = 0 left out: a is better than b iff cut_a den_b < cut_b den_a in 64-bit
//            integers, or the products are equal and k_a < k_b -- a total order, so every reduction shape gives the same k
//
// Kernels.  The columns of a batch are interleaved to B = 1, 2, 4, 8 or 16 positions per vertex (ns rounded up), so that the one
// pass over the edges reads col_idx once for all of them and a neighbour's B positions as one line.
//   keys      k_sweep_keys        one thread per vertex: the score to an order-preserving u64 (complemented for descending
//                                 order, all ones for a vertex the per-degree rule puts last), and the ids 0 .. n-1 beside it
//   sort      hipcub's radix sort of (key, id) pairs, per column: it is stable, so ties keep their ascending ids
//   positions k_sweep_pos         pos[order[i]][c] = i, u32 [n][B]
//   sweep     k_sweep_back<G, B>  G lanes per row (4 .. 32 from the mean degree): for every neighbour u != v the B positions of u,
//                                 16 bytes per load where B >= 4, are compared with v's and counted in B registers; the counts and
//                                 d_v are summed over the group by shuffles, and lane c of the group stores d_v - 2 b_v (i64) and
//                                 d_v (u64) at place pos[v][c] of column c's two arrays
//             k_sweep_long_rows   only when a row of more than long_row entries (64 G) exists: those rows are listed, one
//                                 wavefront-aggregated append (lzx_wave_append) each; the order of the list is no output
//             k_sweep_back_long<B> a workgroup per listed row, every thread with 4 (B <= 4) or 2 entries' loads in flight.  The
//                                 hubs of an R-MAT graph have the smallest ids: a workgroup that walks the long rows among its own
//                                 256 rows, as k_row_count_long does, gets most of them (DESIGN.md section 22 has the times)
//   scans     hipcub's inclusive sums over the two arrays of a column: cut (i64) and vol (u64), in place
//   best      k_sweep_best        grid (blocks, columns): every block's best candidate of its share of the window
//             k_sweep_close       a workgroup per column: the best of the blocks' candidates, vol at that k, and M
// The sweep has no atomics (the list of the long rows has one per wavefront) and the device no floating point but the key's one
// division; no kernel waits on another workgroup; every loop is
// bounded by a row length, the window or the block count.  Every store of the sweep goes to place pos[v][c] < n, which k_sweep_pos
// wrote from a permutation.  A matrix that is not symmetric is not detected and its numbers mean nothing: the running cut can then
// be negative, which the signed sums and products cover (|cut| <= M < 2^32 and den < 2^31, so every product is below 2^63).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>

#include <hipcub/hipcub.hpp>

#include "lzx_internal.h"
#include "lzx_graph_call.h"

static constexpr u32 LZX_SWEEP_BLOCK = 256;
static constexpr u32 LZX_SWEEP_MAX = 16;           // columns per call
static constexpr u32 LZX_SWEEP_BEST_GRID = 1024;   // blocks that share a column's window (at most)
static constexpr u32 LZX_SWEEP_LONG_GRID = 4096;   // workgroups that stride over the list of the long rows (at most)
static constexpr u32 LZX_SWEEP_FLAGS = LZX_SWEEP_ASCENDING | LZX_SWEEP_PER_DEGREE | LZX_SWEEP_EXPANSION;
typedef long long i64;

// ---- keys and positions -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LZX_SWEEP_BLOCK)
k_sweep_keys(const u64 *row_ptr, const u32 *col_idx, const double *score, ull *keys, u32 *ids, u32 n, u32 flags)
{
    const u64 v = (u64)blockIdx.x * LZX_SWEEP_BLOCK + threadIdx.x;
    if (v >= n) return;
    double s = score[v];
    ull key = ~0ull;   // behind every key of a score: the vertices without an edge under the per-degree rule
    u32 d = 1;
    if (flags & LZX_SWEEP_PER_DEGREE) {
        d = lzx_degree_no_diagonal(row_ptr, col_idx, v);
        if (d) s = s / (double)d;
    }
    if (d) {
        ull b = (ull)__double_as_longlong(s);
        if ((b << 1) == 0) b = 0;                                  // -0.0 counts as +0.0
        b ^= (b >> 63) ? ~0ull : 0x8000000000000000ull;            // ascending in s; -inf .. +inf is 0x000f... .. 0xfff0...
        key = (flags & LZX_SWEEP_ASCENDING) ? b : ~b;
    }
    keys[v] = key;
    ids[v] = (u32)v;
}

// pos[order[i]][col] = i
__global__ void __launch_bounds__(LZX_SWEEP_BLOCK)
k_sweep_pos(const u32 *order, u32 *pos, u32 n, u32 B, u32 col)
{
    const u64 i = (u64)blockIdx.x * LZX_SWEEP_BLOCK + threadIdx.x;
    if (i < n) pos[(u64)order[i] * B + col] = (u32)i;
}

// ---- the edge sweep -----------------------------------------------------------------------------------------------------------
// the B positions of vertex u
template <u32 B>
__device__ __forceinline__ void sweep_load(const u32 *pos, u32 u, u32 (&p)[B])
{
    if constexpr (B == 1) p[0] = pos[u];
    else if constexpr (B == 2) {
        const uint2 t = reinterpret_cast<const uint2 *>(pos)[u];
        p[0] = t.x;
        p[1] = t.y;
    } else {
        const uint4 *line = reinterpret_cast<const uint4 *>(pos) + (u64)u * (B / 4);
#pragma unroll
        for (u32 q = 0; q < B / 4; ++q) {
            const uint4 t = line[q];
            p[4 * q] = t.x;
            p[4 * q + 1] = t.y;
            p[4 * q + 2] = t.z;
            p[4 * q + 3] = t.w;
        }
    }
}

// U entries of row v at once (their loads are issued together): the columns in which each u comes before v, and the degree.  A
// diagonal entry needs no branch: pos[v] < pos[v] never holds.
template <u32 B, u32 U>
__device__ __forceinline__ void sweep_entries(const u32 *pos, u32 v, const u32 (&u)[U], const u32 (&pv)[B], u32 (&cnt)[B], u32 &d)
{
    u32 pu[U][B];
#pragma unroll
    for (u32 j = 0; j < U; ++j) sweep_load<B>(pos, u[j], pu[j]);
#pragma unroll
    for (u32 j = 0; j < U; ++j) {
#pragma unroll
        for (u32 c = 0; c < B; ++c) cnt[c] += pu[j][c] < pv[c] ? 1u : 0u;
        d += u[j] != v ? 1u : 0u;
    }
}

// rows of at most long_row entries: G lanes per row, 256 / G rows per workgroup
template <u32 G, u32 B>
__global__ void __launch_bounds__(LZX_SWEEP_BLOCK)
k_sweep_back(const u64 *row_ptr, const u32 *col_idx, const u32 *pos, i64 *delta, ull *deg, u32 n, u32 ns, u32 long_row)
{
    const u32 sub = threadIdx.x & (G - 1);
    const u64 row = (u64)blockIdx.x * (LZX_SWEEP_BLOCK / G) + threadIdx.x / G;
    u64 beg = 0;
    u32 len = 0;
    bool mine = false;
    if (row < n) {
        beg = row_ptr[row];
        const u64 l = row_ptr[row + 1] - beg;
        mine = l <= long_row;   // the others are k_sweep_back_long's
        len = mine ? (u32)l : 0u;
    }
    u32 pv[B], cnt[B], d = 0;
#pragma unroll
    for (u32 c = 0; c < B; ++c) pv[c] = cnt[c] = 0;
    if (mine) sweep_load<B>(pos, (u32)row, pv);
    for (u32 e = sub; e < len; e += G) {
        const u32 u[1] = {col_idx[beg + e]};
        sweep_entries<B, 1>(pos, (u32)row, u, pv, cnt, d);
    }
    d = lzx_group_sum_u32<G>(d);
#pragma unroll
    for (u32 c = 0; c < B; ++c) {
        const u32 b = lzx_group_sum_u32<G>(cnt[c]);
        if (mine && c < ns && sub == (c & (G - 1))) {   // (pv[c] < n: k_sweep_pos wrote it)
            const u64 at = (u64)c * n + pv[c];
            delta[at] = (i64)d - 2 * (i64)b;
            deg[at] = d;
        }
    }
}

// the rows of more than long_row entries, listed in no particular order: list[0 .. *count)
__global__ void __launch_bounds__(LZX_SWEEP_BLOCK)
k_sweep_long_rows(const u64 *row_ptr, u32 *list, u32 *count, u32 n, u32 long_row)
{
    const u64 v = (u64)blockIdx.x * LZX_SWEEP_BLOCK + threadIdx.x;
    const bool take = v < n && row_ptr[v + 1] - row_ptr[v] > long_row;
    const u32 at = lzx_wave_append(take, count);
    if (take && at < n) list[at] = (u32)v;
}

// the listed rows, a workgroup per row (the workgroups stride over the list): every thread holds U entries at a time
template <u32 B>
__global__ void __launch_bounds__(LZX_SWEEP_BLOCK)
k_sweep_back_long(const u64 *row_ptr, const u32 *col_idx, const u32 *pos, i64 *delta, ull *deg, const u32 *list, const u32 *count, u32 n, u32 ns)
{
    constexpr u32 U = B <= 4 ? 4 : 2;
    __shared__ u32 s_part[LZX_SWEEP_BLOCK / 64][B + 1];
    const u32 rows = min(*count, n);
    for (u32 i = blockIdx.x; i < rows; i += gridDim.x) {   // (the same trips for every thread of the workgroup)
        const u32 v = list[i];
        const u64 beg = row_ptr[v], end = row_ptr[v + 1];
        u32 pv[B], cnt[B], d = 0;
#pragma unroll
        for (u32 c = 0; c < B; ++c) cnt[c] = 0;
        sweep_load<B>(pos, v, pv);
        u64 e = beg + threadIdx.x;
        for (; e + (U - 1) * LZX_SWEEP_BLOCK < end; e += U * LZX_SWEEP_BLOCK) {
            u32 u[U];
#pragma unroll
            for (u32 j = 0; j < U; ++j) u[j] = col_idx[e + j * LZX_SWEEP_BLOCK];
            sweep_entries<B, U>(pos, v, u, pv, cnt, d);
        }
        for (; e < end; e += LZX_SWEEP_BLOCK) {
            const u32 u[1] = {col_idx[e]};
            sweep_entries<B, 1>(pos, v, u, pv, cnt, d);
        }
        d = lzx_wave_sum_u32(d);
#pragma unroll
        for (u32 c = 0; c < B; ++c) {
            const u32 b = lzx_wave_sum_u32(cnt[c]);
            if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][c] = b;
        }
        if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][B] = d;
        __syncthreads();
#pragma unroll
        for (u32 c = 0; c < B; ++c)
            if (threadIdx.x == c && c < ns) {
                const u32 b = (s_part[0][c] + s_part[1][c]) + (s_part[2][c] + s_part[3][c]);
                const u32 dv = (s_part[0][B] + s_part[1][B]) + (s_part[2][B] + s_part[3][B]);
                const u64 at = (u64)c * n + pv[c];
                delta[at] = (i64)dv - 2 * (i64)b;
                deg[at] = dv;
            }
        __syncthreads();
    }
}

// ---- the best prefix ----------------------------------------------------------------------------------------------------------
struct SweepCand {
    ull k;     // 0: none
    i64 cut, den;
};

// a comes before b in the total order: a smaller ratio, then a smaller k; no candidate comes last
__device__ __forceinline__ bool sweep_better(const SweepCand &a, const SweepCand &b)
{
    if (a.k == 0) return false;
    if (b.k == 0) return true;
    const i64 l = a.cut * b.den, r = b.cut * a.den;
    return l != r ? l < r : a.k < b.k;
}

// the workgroup's best (in thread 0).  s: one candidate per wavefront.
__device__ __forceinline__ SweepCand sweep_block_best(SweepCand best, SweepCand *s)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        SweepCand other;
        other.k = __shfl_xor(best.k, o, 64);
        other.cut = __shfl_xor(best.cut, o, 64);
        other.den = __shfl_xor(best.den, o, 64);
        if (sweep_better(other, best)) best = other;
    }
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0)
        for (u32 w = 1; w < LZX_SWEEP_BLOCK / 64; ++w)
            if (sweep_better(s[w], best)) best = s[w];
    return best;
}

// part[column][block] = the best k of the block's share of [lo, hi] (1 <= lo <= hi <= n); cut and vol are the scanned arrays
__global__ void __launch_bounds__(LZX_SWEEP_BLOCK)
k_sweep_best(const i64 *cut, const ull *vol, SweepCand *part, u32 n, u64 lo, u64 hi, u32 expansion)
{
    __shared__ SweepCand s[LZX_SWEEP_BLOCK / 64];
    const u32 col = blockIdx.y;
    const i64 *ccut = cut + (u64)col * n;
    const ull *cvol = vol + (u64)col * n;
    const ull M = cvol[n - 1];
    SweepCand best{0, 0, 0};
    for (u64 k = lo + (u64)blockIdx.x * LZX_SWEEP_BLOCK + threadIdx.x; k <= hi; k += (u64)gridDim.x * LZX_SWEEP_BLOCK) {
        const ull vk = cvol[k - 1];
        const ull den = expansion ? min((ull)k, (ull)n - k) : min(vk, M - vk);
        const SweepCand cand{k, ccut[k - 1], (i64)den};
        if (den && sweep_better(cand, best)) best = cand;
    }
    best = sweep_block_best(best, s);
    if (threadIdx.x == 0) part[(u64)col * gridDim.x + blockIdx.x] = best;
}

// res[column] = k, cut, vol, den of the best of the column's np candidates (zeros if there is none), and M
__global__ void __launch_bounds__(LZX_SWEEP_BLOCK)
k_sweep_close(const SweepCand *part, u32 np, const ull *vol, ull *res, u32 n)
{
    __shared__ SweepCand s[LZX_SWEEP_BLOCK / 64];
    const u32 col = blockIdx.x;
    SweepCand best{0, 0, 0};
    for (u32 i = threadIdx.x; i < np; i += LZX_SWEEP_BLOCK) {
        const SweepCand cand = part[(u64)col * np + i];
        if (sweep_better(cand, best)) best = cand;
    }
    best = sweep_block_best(best, s);
    if (threadIdx.x == 0) {
        const ull *cvol = vol + (u64)col * n;
        ull *r = res + 5 * (u64)col;
        r[0] = best.k;
        r[1] = (ull)best.cut;
        r[2] = best.k ? cvol[best.k - 1] : 0ull;
        r[3] = (ull)best.den;
        r[4] = cvol[n - 1];
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
namespace {
// f(std::integral_constant<u32, B>{}) for the width B = 1, 2, 4, 8 or 16
template <typename F>
void with_width(u32 B, F f)
{
    if (B == 1) f(std::integral_constant<u32, 1>{});
    else if (B == 2) f(std::integral_constant<u32, 2>{});
    else if (B == 4) f(std::integral_constant<u32, 4>{});
    else if (B == 8) f(std::integral_constant<u32, 8>{});
    else f(std::integral_constant<u32, 16>{});
}
}   // namespace

extern "C" int lzx_sweep_cut(lzx_handle c, uint32_t ns, const double *scores, uint32_t flags, uint64_t k_min, uint64_t k_max, uint32_t *order,
                             uint64_t *cut, uint64_t *vol, lzx_sweep_result *best, lzx_sweep_info *info)
{
    const char *fn_name = "lzx_sweep_cut";
    LZX_TRY(lzx_graph_call_check(c, fn_name, "a sweep cut is taken"));
    if (!scores || !best) LZX_FAIL(LZX_ERR_ARG, "%s: null %s", fn_name, !scores ? "scores" : "best");
    if (flags & ~LZX_SWEEP_FLAGS)
        LZX_FAIL(LZX_ERR_ARG, "%s: unknown flag bits 0x%x (LZX_SWEEP_ASCENDING, LZX_SWEEP_PER_DEGREE and LZX_SWEEP_EXPANSION are the flags)", fn_name,
                 flags & ~LZX_SWEEP_FLAGS);
    if (ns == 0) LZX_FAIL(LZX_ERR_ARG, "%s: ns must be at least 1", fn_name);
    if (ns > LZX_SWEEP_MAX) LZX_FAIL(LZX_ERR_LIMIT, "%s: %u columns; at most %u per call", fn_name, ns, LZX_SWEEP_MAX);
    const u32 n = (u32)c->n;
    if (k_max > n) LZX_FAIL(LZX_ERR_ARG, "%s: k_max = %llu is above the %u vertices", fn_name, (ull)k_max, n);
    if (k_max ? k_min > k_max : k_min > n)
        LZX_FAIL(LZX_ERR_ARG, "%s: k_min = %llu is above k_max = %llu", fn_name, (ull)k_min, (ull)(k_max ? k_max : n));
    if (c->nnz >= (1ull << 32)) LZX_FAIL(LZX_ERR_LIMIT, "%s: %llu entries; the products of the comparison need fewer than 2^32", fn_name, (ull)c->nnz);
    for (u32 col = 0; col < ns; ++col)
        for (u64 i = 0; i < n; ++i)
            if (std::isnan(scores[(u64)col * n + i])) LZX_FAIL(LZX_ERR_ARG, "%s: the score of column %u at index %llu is NaN", fn_name, col, (ull)i);
    const auto t0 = std::chrono::steady_clock::now();
    const u64 lo = k_min ? k_min : 1, hi = k_max ? k_max : (n ? n - 1 : 0);   // the window; empty when lo > hi
    for (u32 col = 0; col < ns; ++col) best[col] = lzx_sweep_result{0, 0, 0, 0, std::numeric_limits<double>::infinity()};
    if (info) *info = lzx_sweep_info{0, ns, 0, 0.0, 0.0, 0.0, 0.0};
    if (n == 0) return LZX_OK;

    u32 B = 1;
    while (B < ns) B *= 2;
    const u32 nblk = lo <= hi ? (u32)std::min<u64>((hi - lo) / LZX_SWEEP_BLOCK + 1, LZX_SWEEP_BEST_GRID) : 0u;
    LZX_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    size_t tmp_sort = 0, tmp_cut = 0, tmp_vol = 0;
    LZX_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sort, (const ull *)nullptr, (ull *)nullptr, (const u32 *)nullptr, (u32 *)nullptr, (u64)n, 0, 64, st));
    LZX_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, tmp_cut, (i64 *)nullptr, (i64 *)nullptr, (size_t)n, st));
    LZX_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, tmp_vol, (ull *)nullptr, (ull *)nullptr, (size_t)n, st));
    const size_t tmp_bytes = std::max<size_t>(std::max(tmp_sort, std::max(tmp_cut, tmp_vol)), 16);
    const u64 pos_words = ((u64)n * B + 3) & ~3ull;   // pos, u32 [n][B], rounded to 16 bytes
    u32 *d_pos, *d_long_count, *d_ids, *d_order;
    ull *d_keys, *d_sorted, *d_vol, *d_res;
    i64 *d_cut;
    SweepCand *d_part;
    void *d_tmp;
    LzxGraphRun run(c);
    char what[128];
    std::snprintf(what, sizeof what, "the state of %u vertices and %u columns (positions, keys, the profiles)", n, ns);
    LZX_TRY(lzx_carve_state(fn_name, what, c->sweep_cap_opt, 0, &run.arena, nullptr, [&](LzxCarver &k) {
        k.take(d_pos, pos_words);
        k.take(d_keys, n);
        k.take(d_sorted, n);   // (the scores are uploaded here)
        k.take(d_cut, (u64)ns * n);
        k.take(d_vol, (u64)ns * n);
        k.take(d_part, (u64)ns * nblk);   // the blocks' candidates
        k.take(d_res, 5 * (u64)ns);
        k.take(d_long_count, 2);   // (a word of eight bytes)
        k.take(d_ids, lzx_even(n));
        k.take(d_order, lzx_even(n));
        k.end_of_state();   // hipcub's temporary storage follows
        k.align(256);
        k.take_bytes(d_tmp, tmp_bytes);
    }));
    u32 *d_long = d_ids;   // the list of the long rows (the ids are done with when the sorts are)
    double *d_score = reinterpret_cast<double *>(d_sorted);   // (read by k_sweep_keys before the sort writes there)
    LZX_TRY(run.events(4));
    const u32 gb = (n + LZX_SWEEP_BLOCK - 1) / LZX_SWEEP_BLOCK;

    // ---- the orders and the positions, column by column ----
    LZX_HIP(hipEventRecord(run.ev0, st));
    if (B != ns) LZX_HIP(hipMemsetAsync(d_pos, 0, sizeof(u32) * pos_words, st));   // (the padding columns are compared, never stored)
    for (u32 col = 0; col < ns; ++col) {
        LZX_HIP(hipMemcpyAsync(d_score, scores + (u64)col * n, sizeof(double) * n, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_sweep_keys, dim3(gb), dim3(LZX_SWEEP_BLOCK), 0, st, c->d_row_ptr, c->d_col_idx, (const double *)d_score, d_keys, d_ids, n, flags);
        LZX_HIP(hipGetLastError());
        size_t tb = tmp_bytes;
        LZX_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp, tb, (const ull *)d_keys, d_sorted, (const u32 *)d_ids, d_order, (u64)n, 0, 64, st));
        hipLaunchKernelGGL(k_sweep_pos, dim3(gb), dim3(LZX_SWEEP_BLOCK), 0, st, (const u32 *)d_order, d_pos, n, B, col);
        LZX_HIP(hipGetLastError());
        if (order) LZX_HIP(hipMemcpyAsync(order + (u64)col * n, d_order, sizeof(u32) * n, hipMemcpyDeviceToHost, st));
    }
    LZX_HIP(hipEventRecord(run.ev1, st));

    // ---- the edge sweep ----
    const u32 G = lzx_lanes_per_row(c, c->nnz, 32);
    const u32 long_row = lzx_shape_or(c->sweep_long_opt, 64 * G);
    const bool long_rows = c->max_degree > long_row;
    if (long_rows) {
        LZX_HIP(hipMemsetAsync(d_long_count, 0, sizeof(u32), st));
        hipLaunchKernelGGL(k_sweep_long_rows, dim3(gb), dim3(LZX_SWEEP_BLOCK), 0, st, c->d_row_ptr, d_long, d_long_count, n, long_row);
    }
    with_width(B, [&](auto b) {
        lzx_with_lanes<32>(G, [&](auto g) {
            hipLaunchKernelGGL((k_sweep_back<g, b>), dim3(lzx_row_grid(n, LZX_SWEEP_BLOCK / g)), dim3(LZX_SWEEP_BLOCK), 0, st, c->d_row_ptr, c->d_col_idx,
                               (const u32 *)d_pos, d_cut, d_vol, n, ns, long_row);
        });
        if (long_rows)
            hipLaunchKernelGGL(k_sweep_back_long<b>, dim3(std::min(n, LZX_SWEEP_LONG_GRID)), dim3(LZX_SWEEP_BLOCK), 0, st, c->d_row_ptr, c->d_col_idx,
                               (const u32 *)d_pos, d_cut, d_vol, (const u32 *)d_long, (const u32 *)d_long_count, n, ns);
    });
    LZX_HIP(hipGetLastError());
    LZX_HIP(hipEventRecord(run.ev2, st));

    // ---- the profiles and the best prefix ----
    for (u32 col = 0; col < ns; ++col) {
        size_t tb = tmp_bytes;
        LZX_HIP(hipcub::DeviceScan::InclusiveSum(d_tmp, tb, d_cut + (u64)col * n, d_cut + (u64)col * n, (size_t)n, st));
        tb = tmp_bytes;
        LZX_HIP(hipcub::DeviceScan::InclusiveSum(d_tmp, tb, d_vol + (u64)col * n, d_vol + (u64)col * n, (size_t)n, st));
    }
    if (nblk) hipLaunchKernelGGL(k_sweep_best, dim3(nblk, ns), dim3(LZX_SWEEP_BLOCK), 0, st, (const i64 *)d_cut, (const ull *)d_vol, d_part, n, lo, hi, flags & LZX_SWEEP_EXPANSION);
    hipLaunchKernelGGL(k_sweep_close, dim3(ns), dim3(LZX_SWEEP_BLOCK), 0, st, (const SweepCand *)d_part, nblk, (const ull *)d_vol, d_res, n);
    LZX_HIP(hipGetLastError());
    LZX_HIP(hipEventRecord(run.ev3, st));

    u64 res[5 * LZX_SWEEP_MAX];
    LZX_HIP(hipMemcpyAsync(res, d_res, 5 * sizeof(u64) * ns, hipMemcpyDeviceToHost, st));
    if (cut) LZX_HIP(hipMemcpyAsync(cut, d_cut, sizeof(u64) * ns * n, hipMemcpyDeviceToHost, st));
    if (vol) LZX_HIP(hipMemcpyAsync(vol, d_vol, sizeof(u64) * ns * n, hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    for (u32 col = 0; col < ns; ++col) {
        const u64 *r = res + 5 * col;
        if (r[0]) best[col] = lzx_sweep_result{r[0], r[1], r[2], r[3], (double)(int64_t)r[1] / (double)r[3]};
    }
    if (info) {
        float sort_ms = 0.f, sweep_ms = 0.f, scan_ms = 0.f;
        LZX_HIP(hipEventElapsedTime(&sort_ms, run.ev0, run.ev1));
        LZX_HIP(hipEventElapsedTime(&sweep_ms, run.ev1, run.ev2));
        LZX_HIP(hipEventElapsedTime(&scan_ms, run.ev2, run.ev3));
        info->entries = res[4];
        info->width = B;
        info->sort_ms = sort_ms;
        info->sweep_ms = sweep_ms;
        info->scan_ms = scan_ms;
        info->loop_ms = lzx_ms_since(t0);
    }
    return LZX_OK;
}
