// lzx_louvain.hip -- Louvain communities of the handle's graph (networkx.community.louvain_communities / louvain_partitions): local
// moves over the colour classes of every level graph, then aggregation, in integers only: include/lzx.h, lzx_louvain; DESIGN.md
// section 25.  The colouring, the class sort, the canonical labels and the modularity are lzx_communities.hip's, run on a view of the
// level graph (lzx_communities_shared.h); the sweep over the classes is lzx_class_sweep.h's.
//
// Definitions.  A level graph has n_l nodes, rows ascending by column and a weight w_ij >= 1 per stored entry (u32); level 0 is the
// caller-order pattern, every off-diagonal entry 1 and a diagonal entry 0.  k_i = the sum of row i, the diagonal included; M = the sum
// of the k_i, the same on every level; d_i = the off-diagonal entries of row i.
//   sweep       label[i] = i, tot[c] = k_c.  The colour classes are taken in ascending colour; every node i of the class with d_i > 0
//               decides from the labels and tot as they stand when its class begins: a = label[i], k_ic = the weight of the
//               neighbours j != i with label c, T_c = tot[c] (T_a = tot[a] - k_i), G(c) = M k_ic - T_c k_i; c* = the c != a of the
//               largest G, ties to the smallest c; i moves iff G(c*) > G(a).  tot is updated when the whole class has decided.
//   level       Qnum = M I - sum tot^2, I = the weight of the entries inside a community.  A sweep without a move ends the level; one
//               that does not raise Qnum is taken back and ends it (reverted); max_sweeps accepted sweeps end it (capped).
//   aggregation the labels that occur, ascending, are the nodes of the next level; w'_pq = the sum of the w_ij between p and q.
//
// Kernels, wave64, 256 threads, templated on W (a weight array is read) so that level 0 reads none:
//   init      k_louvain_init<W>        one thread per row: label = i, k = tot = the row sum, I += the diagonal
//   decide    (the pass over the classes, the wave insert and the far insert: lzx_class_sweep.h, shared with the propagation)
//             k_louvain_group<G, W>    rows of at most lpa_group_row entries (128): G lanes per row stage the neighbours' labels (and
//                                      weights) in the group's LDS slice; every lane sums, for its own entries, the weight of the equal
//                                      labels, gathers tot, forms G in i64, and (G, smallest c) is max-reduced over the group
//             k_louvain_table<W>       rows of at most lpa_table_row entries (2048): a workgroup per row and the open-addressing table
//                                      of the propagation in LDS, the count slot a weight sum; then every slot forms its G and the
//                                      pair is max-reduced over the workgroup
//             k_class_far_insert<W>    longer rows: the same insertion into the row's table in global memory by up to 64 workgroups,
//             k_louvain_far_pick       and the pick by the workgroup that owns the table, which clears the slots it read
//             A mover writes its label in place -- nobody in its class reads it -- and is appended (lzx_wave_append) to the move list
//             as (i, a, c*, k_ic* - k_ia); tot is not written while a class decides.
//   apply     k_louvain_apply          one thread per move of the class: tot[a] -= k_i, tot[c*] += k_i (32-bit integer atomics), and
//                                      I += 2 (k_ic* - k_ia) with one 64-bit integer atomic per wavefront: exact, because the movers of
//                                      a class are not adjacent.  The list is one per sweep; the window of a class lies between two
//                                      words kept by launch parity, as the scalars of the CG loop are.
//   Qnum      k_louvain_sum_sq         sum tot^2 over n_l words, one 64-bit atomic per wavefront.  The host reads the move count, I
//                                      and that sum once per sweep.
//   aggregate k_agg_flag, a hipcub exclusive scan (the new ids), k_agg_keys<G, W> (every entry becomes the key p << 32 | q with its
//             weight; level 0's diagonal entries get the key C << 32 and weight 0), a hipcub radix sort by key, a hipcub reduce by
//             key, k_agg_rows (row pointers by binary search in the keys, the longest row, the rows with an entry), k_agg_cols.
// No floating point before the modularity of the result; integer vector atomics only; no kernel waits on another workgroup; every
// loop is bounded by a row length, a table size or a cap; every append is clamped to n_l.
#include <algorithm>
#include <chrono>
#include <climits>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "lzx_internal.h"
#include "lzx_graph_call.h"
#include "lzx_class_sweep.h"
#include "lzx_reduce.h"

typedef long long i64;
// the accumulator words (u64) behind the counter words: I, sum tot^2, the move list's end (low word), the two window words, the
// next level's longest row and rows with an entry (u32 each), sum tot
enum { AC_INNER = 0, AC_SQ = 1, AC_TAIL = 2, AC_PREV = 3, AC_STATS = 4, AC_SUM = 5, AC_WORDS = 8 };

// what a decide launch reads and writes
struct LouvainSweep {
    const u32 *k;   // k_i
    u32 *label;
    const u32 *tot;
    u32 *moves;     // 4 words per move: i, a, c*, k_ic* - k_ia
    u32 *tail;      // the list's end
    i64 M;
    u32 n;          // n_l: the list's capacity
};

// a candidate: the better one has the larger G, then the smaller label; none = (LLONG_MIN, LZX_COM_NONE)
struct LouvainPick {
    i64 g;
    u32 c, kic;
};
__device__ __forceinline__ void pick_better(LouvainPick &p, i64 g, u32 c, u32 kic)
{
    if (g > p.g || (g == p.g && c < p.c)) {
        p.g = g;
        p.c = c;
        p.kic = kic;
    }
}
__device__ __forceinline__ void pick_exchange(LouvainPick &p, int w)
{
    const i64 g = __shfl_xor(p.g, w, 64);
    const u32 c = (u32)__shfl_xor((int)p.c, w, 64), kic = (u32)__shfl_xor((int)p.kic, w, 64);
    pick_better(p, g, c, kic);
}

// The decision of node v (this lane holds it where `decides`): the label in place and the move on the list.  Every lane of the
// wavefront must call it together.
__device__ __forceinline__ void louvain_decide(bool decides, const LouvainSweep &s, u32 v, u32 a, u32 kia, const LouvainPick &p)
{
    bool move = false;
    if (decides && p.c != LZX_COM_NONE) {
        const i64 ki = s.k[v];
        const i64 stay = s.M * (i64)kia - ((i64)s.tot[a] - ki) * ki;
        move = p.g > stay;
    }
    if (move) s.label[v] = p.c;
    const u32 at = lzx_wave_append(move, s.tail);
    if (move && at < s.n) {
        u32 *m = s.moves + 4 * (u64)at;
        m[0] = v;
        m[1] = a;
        m[2] = p.c;
        m[3] = p.kic - kia;
    }
}

// ---- init -------------------------------------------------------------------------------------------------------------------
template <bool W>
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_louvain_init(const u64 *row_ptr, const u32 *col_idx, const u32 *weights, const u32 *d, u32 *k, u32 *label, u32 *tot, ull *acc, u32 n)
{
    const u64 v = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    ull diagonal = 0;
    if (v < n) {
        u32 sum = d[v];
        if (W) {
            sum = 0;
            for (u64 e = row_ptr[v]; e < row_ptr[v + 1]; ++e) {
                sum += weights[e];
                if (col_idx[e] == (u32)v) diagonal = weights[e];
            }
        }
        k[v] = sum;
        tot[v] = sum;
        label[v] = (u32)v;
    }
    diagonal = wave_sum_u64(diagonal);
    if ((threadIdx.x & 63) == 0 && diagonal) atomicAdd(&acc[AC_INNER], diagonal);
}

// ---- decide -----------------------------------------------------------------------------------------------------------------
// the rows cls[sbeg .. sbeg + slen): G lanes per row, 256 / G rows per workgroup, 128 labels (and weights) of LDS per row
template <u32 G, bool W>
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_louvain_group(const u64 *row_ptr, const u32 *col_idx, const u32 *weights, LouvainSweep s, const u32 *cls, u32 sbeg, u32 slen)
{
    __shared__ u32 s_lab[(LZX_COM_BLOCK / G) * LZX_LPA_STAGE];
    __shared__ u32 s_wgt[W ? (LZX_COM_BLOCK / G) * LZX_LPA_STAGE : 1];
    u32 *slice = s_lab + (threadIdx.x / G) * LZX_LPA_STAGE;
    u32 *wslice = W ? s_wgt + (threadIdx.x / G) * LZX_LPA_STAGE : s_wgt;
    const u32 sub = threadIdx.x & (G - 1);
    const u64 idx = (u64)blockIdx.x * (LZX_COM_BLOCK / G) + threadIdx.x / G;
    u64 beg = 0;
    u32 len = 0, v = 0, a = 0;
    i64 ki = 0;
    if (idx < slen) {
        v = cls[sbeg + idx];
        beg = row_ptr[v];
        len = (u32)(row_ptr[v + 1] - beg);
        a = s.label[v];
        ki = s.k[v];
    }
    // the label of entry j, none for the diagonal; its weight
    auto fetch = [&](u32 j) {
        const u32 u = col_idx[beg + j];
        return u == v ? LZX_COM_NONE : s.label[u];
    };
    auto weight = [&](u32 j) { return W ? weights[beg + j] : 1u; };
    const u32 staged = min(len, LZX_LPA_STAGE);
    for (u32 j = sub; j < staged; j += G) {
        slice[j] = fetch(j);
        if (W) wslice[j] = weight(j);
    }
    __syncthreads();
    LouvainPick best{LLONG_MIN, LZX_COM_NONE, 0u};
    u32 kia = 0;
    for (u32 j = sub; j < len; j += G) {
        const u32 mine = j < staged ? slice[j] : fetch(j);
        if (mine == LZX_COM_NONE) continue;
        if (mine == a) {
            kia += j < staged ? (W ? wslice[j] : 1u) : weight(j);
            continue;
        }
        u32 kic = 0;
        for (u32 i = 0; i < staged; ++i) kic += slice[i] == mine ? (W ? wslice[i] : 1u) : 0u;
        for (u32 i = staged; i < len; ++i) kic += fetch(i) == mine ? weight(i) : 0u;
        pick_better(best, s.M * (i64)kic - (i64)s.tot[mine] * ki, mine, kic);
    }
    kia = lzx_group_sum_u32<G>(kia);
#pragma unroll
    for (u32 w = G / 2; w > 0; w >>= 1) pick_exchange(best, (int)w);
    louvain_decide(sub == 0 && idx < slen, s, v, a, kia, best);
}

// what the slots [threadIdx.x, +256, ...) of a table hold: the best candidate, and k_ia into *s_kia (one slot holds a at the most)
__device__ __forceinline__ LouvainPick louvain_scan(u32 *keys, u32 *sums, u32 slots, bool clear, const LouvainSweep &s, u32 a, i64 ki, u32 *s_kia)
{
    LouvainPick best{LLONG_MIN, LZX_COM_NONE, 0u};
    for (u32 t = threadIdx.x; t < slots; t += LZX_COM_BLOCK) {
        const u32 key = keys[t];
        if (!key) continue;
        const u32 c = key - 1, kic = sums[t];
        if (c == a) *s_kia = kic;
        else pick_better(best, s.M * (i64)kic - (i64)s.tot[c] * ki, c, kic);
        if (clear) {
            keys[t] = 0;
            sums[t] = 0;
        }
    }
    return best;
}

// the workgroup's best candidate decides for v in the first wavefront
__device__ __forceinline__ void louvain_take(LouvainPick best, const LouvainSweep &s, u32 v, u32 a, const u32 *s_kia, LouvainPick *s_pick)
{
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) pick_exchange(best, w);
    if ((threadIdx.x & 63) == 0) s_pick[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x < 64) {
        best = s_pick[0];
        for (u32 w = 1; w < LZX_COM_BLOCK / 64; ++w) pick_better(best, s_pick[w].g, s_pick[w].c, s_pick[w].kic);
        louvain_decide(threadIdx.x == 0, s, v, a, *s_kia, best);
    }
}

// the rows cls[sbeg .. sbeg + gridDim.x): a workgroup per row over a table of pow2ceil(2 len) slots in LDS
template <bool W>
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_louvain_table(const u64 *row_ptr, const u32 *col_idx, const u32 *weights, LouvainSweep s, const u32 *cls, u32 sbeg)
{
    __shared__ u32 s_table[2 * LZX_LPA_SLOTS];
    __shared__ LouvainPick s_pick[LZX_COM_BLOCK / 64];
    __shared__ u32 s_kia;
    const u32 v = cls[sbeg + blockIdx.x];
    const u64 beg = row_ptr[v], end = row_ptr[v + 1];
    const u32 a = s.label[v];
    const u32 slots = lpa_slots(end - beg, LZX_LPA_SLOTS);
    u32 *keys = s_table, *sums = s_table + slots;
    for (u32 t = threadIdx.x; t < 2 * slots; t += LZX_COM_BLOCK) s_table[t] = 0;
    if (threadIdx.x == 0) s_kia = 0;
    __syncthreads();
    for (u64 e0 = beg; e0 < end; e0 += LZX_COM_BLOCK) {   // (the same trips for every lane of the workgroup)
        const u64 e = e0 + threadIdx.x;
        const u32 u = e < end ? col_idx[e] : v;
        lzx_insert_wave<W>(u != v, u != v ? s.label[u] : 0u, (W && u != v) ? weights[e] : 1u, keys, sums, slots);
    }
    __syncthreads();
    const LouvainPick best = louvain_scan(keys, sums, slots, false, s, a, s.k[v], &s_kia);
    louvain_take(best, s, v, a, &s_kia, s_pick);
}

// The rows cls[sbeg .. sbeg + gridDim.x) of more entries, after k_class_far_insert<W> (lzx_class_sweep.h): the workgroup that owns
// the row's table picks over its slots and clears them
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_louvain_far_pick(const u64 *row_ptr, LouvainSweep s, const u32 *cls, u32 sbeg, const u32 *lpos, const u64 *loff, u32 *tables)
{
    __shared__ LouvainPick s_pick[LZX_COM_BLOCK / 64];
    __shared__ u32 s_kia;
    const u32 v = cls[sbeg + blockIdx.x];
    const u32 a = s.label[v];
    const u32 slots = lpa_slots(row_ptr[v + 1] - row_ptr[v], 1u << 31);
    u32 *keys = tables + 2 * loff[lpos[v]], *sums = keys + slots;
    if (threadIdx.x == 0) s_kia = 0;
    __syncthreads();
    const LouvainPick best = louvain_scan(keys, sums, slots, true, s, a, s.k[v], &s_kia);
    louvain_take(best, s, v, a, &s_kia, s_pick);
}

// ---- apply, Qnum ----------------------------------------------------------------------------------------------------------------
// The moves of one class, list[prev .. tail): prev = the window word of this launch's parity; thread 0 leaves tail in the other
// word for the next class's launch.  Launched over at least as many threads as the class has rows.
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_louvain_apply(const u32 *moves, const u32 *k, u32 *tot, ull *acc, u32 parity, u32 n)
{
    u32 *words = reinterpret_cast<u32 *>(acc + AC_PREV);
    const u32 tail = min(*reinterpret_cast<const u32 *>(acc + AC_TAIL), n);
    const u64 t = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    const u64 at = (u64)words[parity] + t;
    if (t == 0) words[parity ^ 1u] = tail;
    i64 twice = 0;
    if (at < tail) {
        const u32 *m = moves + 4 * at;
        const u32 ki = k[m[0]];
        atomicSub(&tot[m[1]], ki);
        atomicAdd(&tot[m[2]], ki);
        twice = 2 * (i64)(int)m[3];
    }
    const ull sum = wave_sum_u64((ull)twice);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&acc[AC_INNER], sum);
}

__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_louvain_sum_sq(const u32 *tot, ull *acc, u32 n)
{
    const u64 v = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    const ull t = v < n ? tot[v] : 0u;
    const ull sum = wave_sum_u64(t * t), plain = wave_sum_u64(t);
    if ((threadIdx.x & 63) == 0 && sum) {
        atomicAdd(&acc[AC_SQ], sum);
        atomicAdd(&acc[AC_SUM], plain);
    }
}

// ---- aggregation ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_agg_flag(const u32 *label, u32 *flag, u32 n)
{
    const u64 v = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    if (v < n && label[v] < n) flag[label[v]] = 1u;
}

// every entry of the level graph: key = new id of its row's label << 32 | of its column's, value = its weight
template <u32 G, bool W>
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_agg_keys(const u64 *row_ptr, const u32 *col_idx, const u32 *weights, const u32 *label, const u32 *newid, u64 *keys, u32 *vals, u32 n, u32 C)
{
    const u32 sub = threadIdx.x & (G - 1);
    const u64 row = (u64)blockIdx.x * (LZX_COM_BLOCK / G) + threadIdx.x / G;
    if (row >= n) return;
    const u64 beg = row_ptr[row], end = row_ptr[row + 1];
    const u64 p = newid[label[row]];
    for (u64 e = beg + sub; e < end; e += G) {
        const u32 u = col_idx[e];
        const bool dropped = !W && u == (u32)row;   // level 0's diagonal
        keys[e] = dropped ? (u64)C << 32 : (p << 32) | newid[label[u]];
        vals[e] = dropped ? 0u : (W ? weights[e] : 1u);
    }
}

// row_ptr[p] = the first key of row p (p <= C); stats[0] = the longest row, stats[1] = the rows with an entry
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_agg_rows(const u64 *keys, u64 entries, u64 *row_ptr, u32 *stats, u32 C)
{
    const u64 p = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    auto first_of = [&](u64 row) {
        u64 lo = 0, hi = entries;
        while (lo < hi) {
            const u64 mid = (lo + hi) >> 1;
            if ((keys[mid] >> 32) < row) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    };
    u32 len = 0;
    if (p <= C) {
        const u64 lo = first_of(p);
        row_ptr[p] = lo;
        if (p < C) len = (u32)(first_of(p + 1) - lo);
    }
    const ull rows = __ballot(len > 0);
    u32 longest = len;
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) longest = max(longest, (u32)__shfl_xor((int)longest, w, 64));
    if ((threadIdx.x & 63) == 0 && rows) {
        atomicMax(&stats[0], longest);
        atomicAdd(&stats[1], (u32)__builtin_popcountll(rows));
    }
}

__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_agg_cols(const u64 *keys, const u32 *vals, u32 *col_idx, u32 *weights, u64 entries)
{
    const u64 e = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    if (e < entries) {
        col_idx[e] = (u32)keys[e];
        weights[e] = vals[e];
    }
}

// comp[v] = the node of the next level that vertex v lies in
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_agg_compose(u32 *comp, const u32 *label, const u32 *newid, u32 n0)
{
    const u64 v = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    if (v < n0) comp[v] = newid[label[comp[v]]];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
namespace {
// the level graphs and the far tables of a level: what the call allocates beyond the LzxGraphRun's three blocks.  Declared after
// the run, so its end comes first: it waits for the stream as well.
struct LouvainBlocks {
    lzx_ctx *c;
    void *graph[2] = {nullptr, nullptr}, *tables = nullptr;   // the current level's graph, the next one's; the far tables
    u64 graph_bytes[2] = {0, 0}, table_bytes = 0;
    explicit LouvainBlocks(lzx_ctx *c_) : c(c_) {}
    void drop(void *&p, u64 &bytes)
    {
        if (p) {
            (void)hipStreamSynchronize(c->stream);
            (void)hipFree(p);
        }
        p = nullptr;
        bytes = 0;
    }
    ~LouvainBlocks()
    {
        (void)hipSetDevice(c->device);
        drop(graph[0], graph_bytes[0]);
        drop(graph[1], graph_bytes[1]);
        drop(tables, table_bytes);
    }
    LouvainBlocks(const LouvainBlocks &) = delete;
    LouvainBlocks &operator=(const LouvainBlocks &) = delete;
};

struct LouvainArena {
    ull *D, *I;
    LzxColorState s;
    u32 *label, *tot, *k, *label0, *tot0, *comp, *moves;
    ull *acc;
};
// the arena of n0 vertices (label0, tot0: the labels and tot a sweep may be taken back to)
void louvain_arena(LzxCarver &k, u32 n0, LouvainArena *a)
{
    const u64 n_al = lzx_even(n0);
    for (ull **p : {&a->D, &a->I}) k.take(*p, n0);
    for (u32 **p : {&a->s.d, &a->s.wait, &a->s.colour, &a->s.queue, &a->label, &a->tot, &a->k, &a->label0, &a->tot0, &a->comp}) k.take(*p, n_al);
    k.take(a->moves, 4 * n_al);   // 4 words per node
    k.take(a->s.bins, lzx_class_bins(n0));
    k.take(a->s.counters, CW_WORDS);
    k.take(a->acc, AC_WORDS);
}

// what the sweeps of a level leave
struct LouvainLevel {
    lzx_louvain_level rec{};   // sweeps, reverted, capped, the moves of the accepted sweeps, I and the sum of tot^2 after them
    u32 accepted = 0;
    float ms = 0.f;
};

// The local moves of one level: label = i, tot = k, then sweeps over the classes of cs until one moves nothing, one does not raise
// Qnum and is taken back, or max_sweeps are accepted.  *M: the sum of the k_i, which the first level sets.
int louvain_level_sweeps(lzx_ctx *c, const LzxGraphView &g, LzxGraphRun &run, const LouvainArena &a, const LzxClassSweep &cs, const char *fn_name, u32 max_sweeps, bool first_level, i64 *M_, LouvainLevel *lv)
{
    hipStream_t st = c->stream;
    const u32 n = g.n, gb = lzx_vertex_grid(n);
    LZX_HIP(hipEventRecord(run.ev2, st));
    LZX_HIP(hipMemsetAsync(a.acc, 0, AC_WORDS * sizeof(u64), st));
    lzx_with_weights(g.weights != nullptr, [&](auto w) {
        hipLaunchKernelGGL(k_louvain_init<w>, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, g.weights, (const u32 *)a.s.d, a.k, a.label, a.tot, a.acc, n);
    });
    hipLaunchKernelGGL(k_louvain_sum_sq, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, (const u32 *)a.tot, a.acc, n);
    LZX_HIP(hipGetLastError());
    u64 words[AC_WORDS] = {};   // I, sum tot^2, the moves, the window words, ..., sum tot
    LZX_HIP(hipMemcpyAsync(words, a.acc, sizeof(words), hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    lv->rec.inner_entries = words[AC_INNER];
    lv->rec.sum_degree_sq = words[AC_SQ];
    if (first_level) *M_ = (i64)words[AC_SUM];   // the sum of the k_i = the off-diagonal entries (tot is k here)
    const i64 M = *M_;
    i64 qnum = M * (i64)lv->rec.inner_entries - (i64)lv->rec.sum_degree_sq;
    const LouvainSweep sw{a.k, a.label, a.tot, a.moves, reinterpret_cast<u32 *>(a.acc + AC_TAIL), M, n};
    while (true) {
        if (lv->accepted == max_sweeps) {
            lv->rec.capped = 1;
            break;
        }
        ++lv->rec.sweeps;
        LZX_HIP(hipMemcpyAsync(a.label0, a.label, sizeof(u32) * n, hipMemcpyDeviceToDevice, st));
        LZX_HIP(hipMemcpyAsync(a.tot0, a.tot, sizeof(u32) * n, hipMemcpyDeviceToDevice, st));
        LZX_HIP(hipMemsetAsync(a.acc + AC_SQ, 0, 3 * sizeof(u64), st));   // the sum, the list's end, the window words
        u32 parity = 0;
        // tot moves when the whole class has decided
        auto apply = [&](u32 rows) {
            if (!rows) return;
            hipLaunchKernelGGL(k_louvain_apply, dim3(lzx_vertex_grid(rows)), dim3(LZX_COM_BLOCK), 0, st, (const u32 *)a.moves, (const u32 *)a.k, a.tot, a.acc, parity, n);
            parity ^= 1u;
        };
        int rc = LZX_OK;
        lzx_with_weights(g.weights != nullptr, [&](auto w) {   // the three decide launches of a class: its rows cls[first .. first + rows) of one path
            auto group = [&](u32 first, u32 rows) {
                lzx_with_lanes<32>(cs.G, [&](auto lanes) { hipLaunchKernelGGL((k_louvain_group<lanes, w>), dim3(lzx_row_grid(rows, LZX_COM_BLOCK / lanes)), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, g.weights, sw, cs.cls, first, rows); });
            };
            auto table = [&](u32 first, u32 rows) { hipLaunchKernelGGL(k_louvain_table<w>, dim3(rows), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, g.weights, sw, cs.cls, first); };
            auto far_pick = [&](u32 first, u32 rows) { hipLaunchKernelGGL(k_louvain_far_pick, dim3(rows), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, sw, cs.cls, first, cs.lpos, cs.loff, cs.tables); };
            rc = lzx_class_pass(c, g, cs, fn_name, a.label, group, table, far_pick, apply);
        });
        LZX_TRY(rc);
        hipLaunchKernelGGL(k_louvain_sum_sq, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, (const u32 *)a.tot, a.acc, n);
        LZX_HIP(hipGetLastError());
        LZX_HIP(hipMemcpyAsync(words, a.acc, sizeof(words), hipMemcpyDeviceToHost, st));
        LZX_HIP(hipStreamSynchronize(st));
        const u32 moved = std::min((u32)(words[AC_TAIL] & 0xffffffffull), n);
        if (moved == 0) break;
        const i64 after = M * (i64)words[AC_INNER] - (i64)words[AC_SQ];
        if (after <= qnum) {   // the sweep is taken back
            LZX_HIP(hipMemcpyAsync(a.label, a.label0, sizeof(u32) * n, hipMemcpyDeviceToDevice, st));
            LZX_HIP(hipMemcpyAsync(a.tot, a.tot0, sizeof(u32) * n, hipMemcpyDeviceToDevice, st));
            LZX_HIP(hipMemcpyAsync(a.acc + AC_INNER, &lv->rec.inner_entries, sizeof(u64), hipMemcpyHostToDevice, st));
            LZX_HIP(hipStreamSynchronize(st));
            lv->rec.reverted = 1;
            break;
        }
        lv->rec.inner_entries = words[AC_INNER];
        lv->rec.sum_degree_sq = words[AC_SQ];
        qnum = after;
        lv->rec.moves += moved;
        ++lv->accepted;
    }
    LZX_HIP(hipEventRecord(run.ev3, st));
    LZX_HIP(hipStreamSynchronize(st));
    LZX_HIP(hipEventElapsedTime(&lv->ms, run.ev2, run.ev3));
    return LZX_OK;
}

// The aggregation's scratch, allocated by the first level that aggregates and sized for level 0 (every later level has fewer
// nodes and no more entries): two key and two value arrays of e0 entries, hipcub's, the count of the runs.
struct LouvainScratch {
    u64 *keys = nullptr, *keys2 = nullptr;
    u32 *vals = nullptr, *vals2 = nullptr, *runs = nullptr;
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    u64 bytes = 0;
};
// what hipcub asks for: the scan over n + 1 flags, the sort and the reduction by key of `entries` pairs
int louvain_cub_bytes(u32 n, u64 entries, hipStream_t st, size_t *bytes)
{
    size_t scan_b = 0, sort_b = 0, reduce_b = 0;
    u64 *keys = nullptr;   // (the sizes do not depend on the pointers)
    u32 *vals = nullptr;
    LZX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, vals, vals, (u64)n + 1, st));
    LZX_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, keys, keys, vals, vals, entries, 0, 64, st));
    LZX_HIP(hipcub::DeviceReduce::ReduceByKey(nullptr, reduce_b, keys, keys, vals, vals, vals, hipcub::Sum(), entries, st));
    *bytes = std::max(scan_b, std::max(sort_b, reduce_b));
    return LZX_OK;
}

// From the labels of level graph g to the next level's graph: *next, in blocks.graph[1], and comp composed with the level's labels
// (level_out, or NULL: the partition of the n0 vertices after this level, canonical).  A level that merged nothing says so in
// *merged, builds no graph and leaves *next and *ms alone.  *held: the bytes the call holds, to which the scratch is added where it is allocated here.
int louvain_aggregate(lzx_ctx *c, const LzxGraphView &g, LzxGraphRun &run, LouvainBlocks &blocks, const LouvainArena &a, LouvainScratch &sc,
                      const char *fn_name, u32 n0, u64 e0, u32 G, int64_t cap, u64 *held, u32 *level_out, bool *merged, LzxGraphView *next, float *ms)
{
    hipStream_t st = c->stream;
    const u32 n = g.n, gb = lzx_vertex_grid(n);
    char what[160];
    // the labels that occur (flags and new ids in the move list's words)
    LZX_HIP(hipEventRecord(run.ev2, st));
    u32 *d_newid = a.moves;
    LZX_HIP(hipMemsetAsync(d_newid, 0, sizeof(u32) * ((u64)n + 1), st));
    hipLaunchKernelGGL(k_agg_flag, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, (const u32 *)a.label, d_newid, n);
    LZX_HIP(hipGetLastError());
    if (!run.more[0]) {
        LZX_TRY(louvain_cub_bytes(n0, e0, st, &sc.tmp_bytes));
        sc.tmp_bytes = (sc.tmp_bytes + 15) & ~(size_t)15;
        std::snprintf(what, sizeof what, "the aggregation's keys and weights of %llu entries", (ull)e0);
        LZX_TRY(lzx_carve_state(fn_name, what, cap, *held, &run.more[0], &sc.bytes, [&](LzxCarver &k) {
            k.take(sc.keys, e0);
            k.take(sc.keys2, e0);
            k.take(sc.vals, lzx_even(e0));
            k.take(sc.vals2, lzx_even(e0));
            k.take_bytes(sc.tmp, sc.tmp_bytes);
            k.take(sc.runs, 4);   // (the count, in 16 bytes)
        }));
        *held += sc.bytes;
    }
    size_t asked = 0;   // (a level that asked for more than level 0 would be refused here, not run)
    LZX_TRY(louvain_cub_bytes(n, g.entries, st, &asked));
    if (asked > sc.tmp_bytes)
        LZX_FAIL(LZX_ERR_LIMIT, "%s: the scratch of the sort of %llu entries exceeds that of level 0 (%zu bytes)", fn_name, (ull)g.entries, sc.tmp_bytes);
    size_t tb = sc.tmp_bytes;
    LZX_HIP(hipcub::DeviceScan::ExclusiveSum(sc.tmp, tb, d_newid, d_newid, (u64)n + 1, st));
    u32 C = 0;
    LZX_HIP(hipMemcpyAsync(&C, d_newid + n, sizeof(u32), hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    *merged = C < n;
    if (!*merged) return LZX_OK;

    lzx_with_lanes<32>(G, [&](auto lanes) {
        lzx_with_weights(g.weights != nullptr, [&](auto w) {
            hipLaunchKernelGGL((k_agg_keys<lanes, w>), dim3(lzx_row_grid(n, LZX_COM_BLOCK / lanes)), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, g.weights, (const u32 *)a.label, (const u32 *)d_newid, sc.keys, sc.vals, n, C);
        });
    });
    LZX_HIP(hipGetLastError());
    int key_bits = 33;
    while (key_bits < 64 && ((u64)C >> (key_bits - 32))) ++key_bits;
    tb = sc.tmp_bytes;
    LZX_HIP(hipcub::DeviceRadixSort::SortPairs(sc.tmp, tb, sc.keys, sc.keys2, sc.vals, sc.vals2, g.entries, 0, key_bits, st));
    tb = sc.tmp_bytes;
    LZX_HIP(hipcub::DeviceReduce::ReduceByKey(sc.tmp, tb, sc.keys2, sc.keys, sc.vals2, sc.vals, sc.runs, hipcub::Sum(), g.entries, st));
    u32 runs = 0;
    LZX_HIP(hipMemcpyAsync(&runs, sc.runs, sizeof(u32), hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    u64 entries = std::min<u64>(runs, g.entries);
    if (entries) {
        u64 last = 0;
        LZX_HIP(hipMemcpy(&last, sc.keys + entries - 1, sizeof(u64), hipMemcpyDeviceToHost));
        if ((last >> 32) >= C) --entries;   // the dropped diagonal entries' run
    }
    // the next level's graph
    u64 *d_rp;
    u32 *d_ci, *d_w;
    std::snprintf(what, sizeof what, "the level graph of %u nodes and %llu entries", C, (ull)entries);
    LZX_TRY(lzx_carve_state(fn_name, what, cap, *held, &blocks.graph[1], &blocks.graph_bytes[1], [&](LzxCarver &k) {
        k.take(d_rp, (u64)C + 1);
        k.take(d_ci, lzx_even(entries));
        k.take(d_w, lzx_even(entries));
    }));
    u32 *d_stats = reinterpret_cast<u32 *>(a.acc + AC_STATS);
    LZX_HIP(hipMemsetAsync(d_stats, 0, 2 * sizeof(u32), st));
    hipLaunchKernelGGL(k_agg_rows, dim3(lzx_vertex_grid(C + 1)), dim3(LZX_COM_BLOCK), 0, st, (const u64 *)sc.keys, entries, d_rp, d_stats, C);
    if (entries) hipLaunchKernelGGL(k_agg_cols, dim3(lzx_row_grid(entries, LZX_COM_BLOCK)), dim3(LZX_COM_BLOCK), 0, st, (const u64 *)sc.keys, (const u32 *)sc.vals, d_ci, d_w, entries);
    hipLaunchKernelGGL(k_agg_compose, dim3(lzx_vertex_grid(n0)), dim3(LZX_COM_BLOCK), 0, st, a.comp, (const u32 *)a.label, (const u32 *)d_newid, n0);
    LZX_HIP(hipGetLastError());
    u32 stats[2] = {0, 0};
    LZX_HIP(hipMemcpyAsync(stats, d_stats, sizeof(stats), hipMemcpyDeviceToHost, st));
    // the partition after this level, canonical (first: `queue`, out: `wait`, sizes: `colour` -- the colouring is done with them)
    if (level_out) {
        LZX_HIP(hipMemsetAsync(a.s.counters, 0, CW_WORDS * sizeof(u32), st));
        LZX_TRY(lzx_comm_canonical(c, a.comp, n0, a.s.queue, a.s.wait, a.s.colour, a.s.counters));
        LZX_HIP(hipMemcpyAsync(level_out, a.s.wait, sizeof(u32) * n0, hipMemcpyDeviceToHost, st));
    }
    LZX_HIP(hipEventRecord(run.ev3, st));
    LZX_HIP(hipStreamSynchronize(st));
    LZX_HIP(hipEventElapsedTime(ms, run.ev2, run.ev3));
    *next = LzxGraphView{d_rp, d_ci, d_w, C, entries, stats[0], stats[1]};
    return LZX_OK;
}
}   // namespace

extern "C" int lzx_louvain(lzx_handle c, uint64_t seed, uint32_t flags, uint32_t max_sweeps, uint32_t max_levels, uint32_t *labels, uint32_t *level_labels, lzx_louvain_level *levels, lzx_louvain_info *info)
{
    const char *fn_name = "lzx_louvain";
    LZX_TRY(lzx_graph_call_check(c, fn_name, "communities are aggregated"));
    if (flags & ~LZX_COLOR_TIES_BY_ID) LZX_FAIL(LZX_ERR_ARG, "%s: unknown flag bits 0x%x (LZX_COLOR_TIES_BY_ID is the only flag)", fn_name, flags & ~LZX_COLOR_TIES_BY_ID);
    if (max_sweeps == 0) LZX_FAIL(LZX_ERR_ARG, "%s: max_sweeps must be at least 1", fn_name);
    if (max_levels == 0 || max_levels > 64) LZX_FAIL(LZX_ERR_ARG, "%s: max_levels must be 1 .. 64, got %u", fn_name, max_levels);
    // M = the off-diagonal entries <= nnz: every gain, Qnum and sum of tot^2 fits a signed 64-bit integer below this
    if (c->nnz >= (1ull << 31)) LZX_FAIL(LZX_ERR_LIMIT, "%s: %llu stored entries; 2^31 or more are not supported (M k and tot^2 must fit 64 bits)", fn_name, (ull)c->nnz);
    if (c->max_degree >= LZX_LPA_MAX_ROW) LZX_FAIL(LZX_ERR_LIMIT, "%s: a row of %llu entries; rows of 2^30 entries or more are not supported", fn_name, (ull)c->max_degree);
    const auto t0 = std::chrono::steady_clock::now();
    const u32 n0 = (u32)c->n;
    const int64_t cap = c->louvain_cap_opt;
    LzxClassSweep cs(c);

    LouvainArena a;
    u64 bytes = 0;
    LZX_HIP(hipSetDevice(c->device));
    LzxGraphRun run(c);
    LouvainBlocks blocks(c);
    char what[160];
    std::snprintf(what, sizeof what, "the state of %u vertices (colours, classes, labels, totals, the move list, the modularity's sums)", n0);
    LZX_TRY(lzx_carve_state(fn_name, what, cap, 0, &run.arena, &bytes, [&](LzxCarver &k) { louvain_arena(k, n0, &a); }));
    u64 held = bytes;   // what the call holds on the device
    LZX_TRY(run.events(4));
    hipLaunchKernelGGL(k_fill_u32<true>, dim3(lzx_vertex_grid(n0)), dim3(LZX_COM_BLOCK), 0, c->stream, a.comp, n0, 0u);
    LZX_HIP(hipGetLastError());

    LouvainScratch sc;
    LzxGraphView g = lzx_view_of(c);
    i64 M = 0;
    u32 counted = 0;
    lzx_louvain_info out{};   // the totals over the counted levels and the times
    while (counted < max_levels) {
        // the colouring and the classes, the tables of the rows above table_above, the sweeps
        LZX_TRY(lzx_class_sweep_open(c, g, run, fn_name, seed, flags, a.s, a.D, a.I, cap, held, &blocks.tables, &blocks.table_bytes, &cs));
        out.color_ms += cs.col.ms;
        LouvainLevel lv;
        LZX_TRY(louvain_level_sweeps(c, g, run, a, cs, fn_name, max_sweeps, counted == 0, &M, &lv));
        out.sweep_ms += lv.ms;
        blocks.drop(blocks.tables, blocks.table_bytes);

        LzxGraphView next;
        bool merged = false;
        float ms = 0.f;
        LZX_TRY(louvain_aggregate(c, g, run, blocks, a, sc, fn_name, n0, c->nnz, cs.G, cap, &held, level_labels ? level_labels + (size_t)counted * n0 : nullptr, &merged, &next, &ms));
        if (!merged) break;   // the level changed nothing: it is not counted
        out.aggregate_ms += ms;
        if (levels) {
            lzx_louvain_level &L = lv.rec;
            L.nodes = g.n;
            L.entries = g.entries;
            L.communities = next.n;
            L.colors = cs.col.colours;
            L.color_rounds = cs.col.rounds;
            for (u32 p = 0; p < 3; ++p)   // the rows per path in one sweep
                for (u32 k = 0; k < cs.col.colours; ++k) L.path_rows[p] += cs.col.run[3 * (size_t)k + p + 1] - cs.col.run[3 * (size_t)k + p];
            levels[counted] = L;
        }
        ++counted;
        out.sweeps += lv.rec.sweeps;
        out.moves += lv.rec.moves;
        // the next level takes the place of this one
        blocks.drop(blocks.graph[0], blocks.graph_bytes[0]);
        std::swap(blocks.graph[0], blocks.graph[1]);
        std::swap(blocks.graph_bytes[0], blocks.graph_bytes[1]);
        held = bytes + sc.bytes + blocks.graph_bytes[0];
        g = next;
    }

    // ---- the result: canonical labels, the statistics, the modularity on the handle's pattern ----
    const LzxGraphView g0 = lzx_view_of(c);
    LZX_TRY(lzx_color_degrees(c, g0, a.s.d, nullptr, a.s.counters));   // (the degrees of level 0 again, the counter words 0)
    LzxCommResult res;
    LZX_TRY(lzx_comm_finish(c, g0, a.comp, a.s, a.D, a.I, labels, &res));
    res.fill(&out);
    out.levels = counted;
    out.loop_ms = lzx_ms_since(t0);
    if (info) *info = out;
    return LZX_OK;
}
