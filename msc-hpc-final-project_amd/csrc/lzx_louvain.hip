// lzx_louvain.hip -- Louvain communities of the handle's graph (networkx.community.louvain_communities / louvain_partitions): local
// moves over the colour classes of every level graph, then aggregation, in integers only: include/lzx.h, lzx_louvain; DESIGN.md
// section 25.  The colouring, the class sort, the canonical labels and the modularity are lzx_communities.hip's, run on a view of the
// level graph (lzx_communities_shared.h).
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
//   decide    k_louvain_group<G, W>    rows of at most lpa_group_row entries (128): G lanes per row stage the neighbours' labels (and
//                                      weights) in the group's LDS slice; every lane sums, for its own entries, the weight of the equal
//                                      labels, gathers tot, forms G in i64, and (G, smallest c) is max-reduced over the group
//             k_louvain_table<W>       rows of at most lpa_table_row entries (2048): a workgroup per row and the open-addressing table
//                                      of the propagation in LDS, the count slot a weight sum; then every slot forms its G and the
//                                      pair is max-reduced over the workgroup
//             k_louvain_far_insert<W>  longer rows: the same insertion into the row's table in global memory by up to 64 workgroups,
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
#include "lzx_communities_shared.h"
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

// The labels of a wavefront's lanes (have: this lane holds one of weight w) into the table: the lanes that agree with the first lane's
// label, and then with the first of the rest, are inserted as one sum; what is left inserts for itself.  Every lane of the wavefront
// must call it together.
__device__ __forceinline__ void louvain_insert_wave(bool have, u32 mine, u32 w, u32 *keys, u32 *sums, u32 slots)
{
    const u32 lane = threadIdx.x & 63;
    ull todo = __ballot(have);
    for (int it = 0; it < 2 && todo; ++it) {   // (the same trips for every lane)
        const int leader = __builtin_ctzll(todo);
        const u32 k0 = (u32)__shfl((int)mine, leader, 64);
        const bool agree = have && mine == k0;
        const ull same = __ballot(agree);
        const u32 sum = lzx_wave_sum_u32(agree ? w : 0u);
        if (lane == (u32)leader) lpa_insert(keys, sums, slots, k0, sum);
        if (agree) have = false;
        todo &= ~same;
    }
    if (have) lpa_insert(keys, sums, slots, mine, w);
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
        louvain_insert_wave(u != v, u != v ? s.label[u] : 0u, (W && u != v) ? weights[e] : 1u, keys, sums, slots);
    }
    __syncthreads();
    const LouvainPick best = louvain_scan(keys, sums, slots, false, s, a, s.k[v], &s_kia);
    louvain_take(best, s, v, a, &s_kia, s_pick);
}

// The rows cls[sbeg .. sbeg + gridDim.x) of more entries: the table of row v lies at tables + 2 loff[lpos[v]] in global memory, all
// zeros between the launches.  First launch: workgroup (row, slice) inserts every gridDim.y-th run of 256 entries of the row ...
template <bool W>
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_louvain_far_insert(const u64 *row_ptr, const u32 *col_idx, const u32 *weights, const u32 *label, const u32 *cls, u32 sbeg, const u32 *lpos,
                     const u64 *loff, u32 *tables)
{
    const u32 v = cls[sbeg + blockIdx.x];
    const u64 beg = row_ptr[v], end = row_ptr[v + 1];
    const u32 slots = lpa_slots(end - beg, 1u << 31);
    u32 *keys = tables + 2 * loff[lpos[v]], *sums = keys + slots;
    for (u64 e0 = beg + (u64)blockIdx.y * LZX_COM_BLOCK; e0 < end; e0 += (u64)gridDim.y * LZX_COM_BLOCK) {   // (the same trips for every lane)
        const u64 e = e0 + threadIdx.x;
        const u32 u = e < end ? col_idx[e] : v;
        louvain_insert_wave(u != v, u != v ? label[u] : 0u, (W && u != v) ? weights[e] : 1u, keys, sums, slots);
    }
}

// ... second launch: the workgroup that owns the table picks over its slots and clears them
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

__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_louvain_iota(u32 *x, u32 n)
{
    const u64 i = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    if (i < n) x[i] = (u32)i;
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

inline u32 entry_grid(u64 entries) { return (u32)((entries + LZX_COM_BLOCK - 1) / LZX_COM_BLOCK); }
}   // namespace

extern "C" int lzx_louvain(lzx_handle c, uint64_t seed, uint32_t flags, uint32_t max_sweeps, uint32_t max_levels, uint32_t *labels,
                           uint32_t *level_labels, lzx_louvain_level *levels, lzx_louvain_info *info)
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
    const u64 e0 = c->nnz;
    hipStream_t st = c->stream;
    const u32 group_row = c->lpa_group_opt > 0 ? (u32)std::min<int64_t>(c->lpa_group_opt, LZX_LPA_MAX_ROW) : LZX_LPA_STAGE;
    const u32 table_row = c->lpa_table_opt > 0 && c->lpa_table_opt < LZX_LPA_SLOTS / 2 ? (u32)c->lpa_table_opt : LZX_LPA_SLOTS / 2;
    const u32 table_above = std::max(group_row, table_row);   // (a test shape may send longer rows to the groups of lanes)
    const int64_t cap = c->louvain_cap_opt;

    // the arena: D, I (u64 [n]); d, wait, colour, queue, label, tot, k, the saved labels and tot, comp (u32 [n] each, rounded to 8
    // bytes), the move list (4 per node); three bins per colour; the counter words and the accumulators
    const u64 n_al = lzx_even(n0), nb = lzx_class_bins(n0);
    const u64 bytes = 2 * (u64)n0 * sizeof(u64) + (14 * n_al + nb + CW_WORDS) * sizeof(u32) + AC_WORDS * sizeof(u64);
    LZX_HIP(hipSetDevice(c->device));
    LzxGraphRun run(c);
    LouvainBlocks blocks(c);
    char what[160];
    std::snprintf(what, sizeof what, "the state of %u vertices (colours, classes, labels, totals, the move list, the modularity's sums)", n0);
    LZX_TRY(lzx_alloc_state(fn_name, what, cap, bytes, bytes, &run.arena));
    u64 held = bytes;   // what the call holds on the device
    ull *d_D = static_cast<ull *>(run.arena), *d_I = d_D + n0;
    LzxColorState s;
    s.d = reinterpret_cast<u32 *>(d_I + n0);
    s.wait = s.d + n_al;
    s.colour = s.wait + n_al;
    s.queue = s.colour + n_al;
    u32 *d_label = s.queue + n_al, *d_tot = d_label + n_al, *d_k = d_tot + n_al, *d_label0 = d_k + n_al, *d_tot0 = d_label0 + n_al;
    u32 *d_comp = d_tot0 + n_al, *d_moves = d_comp + n_al;
    s.bins = d_moves + 4 * n_al;
    s.counters = s.bins + nb;
    ull *d_acc = reinterpret_cast<ull *>(s.counters + CW_WORDS);
    u32 *d_stats = reinterpret_cast<u32 *>(d_acc + AC_STATS);
    LZX_HIP(hipEventCreate(&run.ev0));
    LZX_HIP(hipEventCreate(&run.ev1));
    LZX_HIP(hipEventCreate(&run.ev2));
    LZX_HIP(hipEventCreate(&run.ev3));
    const u32 gb0 = lzx_vertex_grid(n0);
    hipLaunchKernelGGL(k_louvain_iota, dim3(gb0), dim3(LZX_COM_BLOCK), 0, st, d_comp, n0);
    LZX_HIP(hipGetLastError());

    // the aggregation's scratch, allocated by the first level that aggregates: two key and two value arrays of e0 entries, hipcub's
    u64 *d_keys = nullptr, *d_keys2 = nullptr;
    u32 *d_vals = nullptr, *d_vals2 = nullptr, *d_runs = nullptr;
    void *d_tmp = nullptr;
    size_t tmp_bytes = 0;
    u64 scratch_bytes = 0;

    LzxGraphView g = lzx_view_of(c);
    i64 M = 0;
    u32 counted = 0;
    u64 total_sweeps = 0, total_moves = 0;
    double color_ms = 0.0, sweep_ms = 0.0, aggregate_ms = 0.0;
    while (counted < max_levels) {
        const u32 n = g.n;
        const bool weighted = g.weights != nullptr;
        const u32 gb = lzx_vertex_grid(n);
        LzxColorResult col;
        LZX_TRY(lzx_color_core(c, g, run, fn_name, seed, flags, s, true, group_row, table_row, &col));
        color_ms += col.ms;
        const u32 *d_cls = s.queue;
        const u32 G = lzx_lanes_of(c, g);

        // the rows above table_above: their places (in `wait`, which the colouring is done with), the offsets of their tables
        u32 *d_lpos = s.wait, *d_llen = reinterpret_cast<u32 *>(d_I);
        u64 *d_loff = reinterpret_cast<u64 *>(d_D);
        if (g.max_row > table_above) {
            LZX_TRY(lzx_lpa_far_tables(c, g, fn_name, table_above, cap, held, d_lpos, d_llen, d_loff, s.counters, &blocks.tables, &blocks.table_bytes));
            held += blocks.table_bytes;
        }
        u32 *d_tables = static_cast<u32 *>(blocks.tables);
        const u32 slices = (u32)std::min<u64>(std::max<u64>(g.max_row / (8 * LZX_COM_BLOCK), 1), 64);   // workgroups that share a long row's entries

        // ---- the sweeps ----
        LZX_HIP(hipEventRecord(run.ev2, st));
        LZX_HIP(hipMemsetAsync(d_acc, 0, AC_WORDS * sizeof(u64), st));
        if (weighted) hipLaunchKernelGGL(k_louvain_init<true>, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, g.weights, (const u32 *)s.d, d_k, d_label, d_tot, d_acc, n);
        else hipLaunchKernelGGL(k_louvain_init<false>, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, g.weights, (const u32 *)s.d, d_k, d_label, d_tot, d_acc, n);
        hipLaunchKernelGGL(k_louvain_sum_sq, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, (const u32 *)d_tot, d_acc, n);
        LZX_HIP(hipGetLastError());
        u64 words[AC_WORDS] = {};   // I, sum tot^2, the moves, the window words, ..., sum tot
        LZX_HIP(hipMemcpyAsync(words, d_acc, sizeof(words), hipMemcpyDeviceToHost, st));
        LZX_HIP(hipStreamSynchronize(st));
        u64 inner = words[AC_INNER], sum_sq = words[AC_SQ];
        if (counted == 0) M = (i64)words[AC_SUM];   // the sum of the k_i = the off-diagonal entries (tot is k here)
        i64 qnum = M * (i64)inner - (i64)sum_sq;
        const LouvainSweep sw{d_k, d_label, d_tot, d_moves, reinterpret_cast<u32 *>(d_acc + AC_TAIL), M, n};
        u32 sweeps = 0, accepted = 0, reverted = 0, capped = 0;
        u64 moves = 0;
        u32 path_rows[3] = {0, 0, 0};
        for (u32 k = 0; k < col.colours; ++k)
            for (u32 p = 0; p < 3; ++p) path_rows[p] += col.run[3 * (size_t)k + p + 1] - col.run[3 * (size_t)k + p];
        while (true) {
            if (accepted == max_sweeps) {
                capped = 1;
                break;
            }
            ++sweeps;
            LZX_HIP(hipMemcpyAsync(d_label0, d_label, sizeof(u32) * n, hipMemcpyDeviceToDevice, st));
            LZX_HIP(hipMemcpyAsync(d_tot0, d_tot, sizeof(u32) * n, hipMemcpyDeviceToDevice, st));
            LZX_HIP(hipMemsetAsync(d_acc + AC_SQ, 0, 3 * sizeof(u64), st));   // the sum, the list's end, the window words
            u32 parity = 0;
            for (u32 k = 0; k < col.colours; ++k) {
                const u32 *r = col.run.data() + 3 * (size_t)k;
                if (r[1] > r[0])
                    lzx_with_lanes<32>(G, [&](auto lanes) {
                        const dim3 grid(lzx_row_grid(r[1] - r[0], LZX_COM_BLOCK / lanes));
                        if (weighted) hipLaunchKernelGGL((k_louvain_group<lanes, true>), grid, dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, g.weights, sw, d_cls, r[0], r[1] - r[0]);
                        else hipLaunchKernelGGL((k_louvain_group<lanes, false>), grid, dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, g.weights, sw, d_cls, r[0], r[1] - r[0]);
                    });
                if (r[2] > r[1]) {
                    if (weighted) hipLaunchKernelGGL(k_louvain_table<true>, dim3(r[2] - r[1]), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, g.weights, sw, d_cls, r[1]);
                    else hipLaunchKernelGGL(k_louvain_table<false>, dim3(r[2] - r[1]), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, g.weights, sw, d_cls, r[1]);
                }
                if (r[3] > r[2]) {
                    if (!d_tables) LZX_FAIL(LZX_ERR_LIMIT, "%s: a row above %u entries without a table", fn_name, table_above);
                    if (weighted) hipLaunchKernelGGL(k_louvain_far_insert<true>, dim3(r[3] - r[2], slices), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, g.weights, (const u32 *)d_label, d_cls, r[2], (const u32 *)d_lpos, (const u64 *)d_loff, d_tables);
                    else hipLaunchKernelGGL(k_louvain_far_insert<false>, dim3(r[3] - r[2], slices), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, g.weights, (const u32 *)d_label, d_cls, r[2], (const u32 *)d_lpos, (const u64 *)d_loff, d_tables);
                    hipLaunchKernelGGL(k_louvain_far_pick, dim3(r[3] - r[2]), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, sw, d_cls, r[2], (const u32 *)d_lpos, (const u64 *)d_loff, d_tables);
                }
                if (r[3] > r[0]) {
                    hipLaunchKernelGGL(k_louvain_apply, dim3(lzx_vertex_grid(r[3] - r[0])), dim3(LZX_COM_BLOCK), 0, st, (const u32 *)d_moves, (const u32 *)d_k, d_tot, d_acc, parity, n);
                    parity ^= 1u;
                }
                LZX_HIP(hipGetLastError());
            }
            hipLaunchKernelGGL(k_louvain_sum_sq, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, (const u32 *)d_tot, d_acc, n);
            LZX_HIP(hipGetLastError());
            LZX_HIP(hipMemcpyAsync(words, d_acc, sizeof(words), hipMemcpyDeviceToHost, st));
            LZX_HIP(hipStreamSynchronize(st));
            const u32 moved = std::min((u32)(words[AC_TAIL] & 0xffffffffull), n);
            if (moved == 0) break;
            const i64 after = M * (i64)words[AC_INNER] - (i64)words[AC_SQ];
            if (after <= qnum) {   // the sweep is taken back
                LZX_HIP(hipMemcpyAsync(d_label, d_label0, sizeof(u32) * n, hipMemcpyDeviceToDevice, st));
                LZX_HIP(hipMemcpyAsync(d_tot, d_tot0, sizeof(u32) * n, hipMemcpyDeviceToDevice, st));
                LZX_HIP(hipMemcpyAsync(d_acc + AC_INNER, &inner, sizeof(u64), hipMemcpyHostToDevice, st));
                LZX_HIP(hipStreamSynchronize(st));
                reverted = 1;
                break;
            }
            inner = words[AC_INNER];
            sum_sq = words[AC_SQ];
            qnum = after;
            moves += moved;
            ++accepted;
        }
        LZX_HIP(hipEventRecord(run.ev3, st));
        LZX_HIP(hipStreamSynchronize(st));
        float ms = 0.f;
        LZX_HIP(hipEventElapsedTime(&ms, run.ev2, run.ev3));
        sweep_ms += ms;
        held -= blocks.table_bytes;
        blocks.drop(blocks.tables, blocks.table_bytes);

        // ---- aggregation: the labels that occur (flags and new ids in the move list's words) ----
        LZX_HIP(hipEventRecord(run.ev2, st));
        u32 *d_newid = d_moves;
        LZX_HIP(hipMemsetAsync(d_newid, 0, sizeof(u32) * ((u64)n + 1), st));
        hipLaunchKernelGGL(k_agg_flag, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, (const u32 *)d_label, d_newid, n);
        LZX_HIP(hipGetLastError());
        if (!run.more[0]) {
            // (sized for level 0: every later level has fewer nodes and no more entries)
            size_t scan_b = 0, sort_b = 0, reduce_b = 0;
            LZX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, d_newid, d_newid, (u64)n0 + 1, st));
            LZX_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, d_keys, d_keys2, d_vals, d_vals2, e0, 0, 64, st));
            LZX_HIP(hipcub::DeviceReduce::ReduceByKey(nullptr, reduce_b, d_keys2, d_keys, d_vals2, d_vals, d_runs, hipcub::Sum(), e0, st));
            tmp_bytes = (std::max(scan_b, std::max(sort_b, reduce_b)) + 15) & ~(size_t)15;
            scratch_bytes = 2 * e0 * sizeof(u64) + 2 * lzx_even(e0) * sizeof(u32) + tmp_bytes + 16;
            std::snprintf(what, sizeof what, "the aggregation's keys and weights of %llu entries", (ull)e0);
            LZX_TRY(lzx_alloc_state(fn_name, what, cap, held + scratch_bytes, scratch_bytes, &run.more[0]));
            held += scratch_bytes;
            d_keys = static_cast<u64 *>(run.more[0]);
            d_keys2 = d_keys + e0;
            d_vals = reinterpret_cast<u32 *>(d_keys2 + e0);
            d_vals2 = d_vals + lzx_even(e0);
            d_tmp = d_vals2 + lzx_even(e0);
            d_runs = reinterpret_cast<u32 *>(static_cast<char *>(d_tmp) + tmp_bytes);
        }
        {   // (hipcub's scratch was sized for level 0: a level that asked for more would be refused here, not run)
            size_t scan_b = 0, sort_b = 0, reduce_b = 0;
            LZX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, d_newid, d_newid, (u64)n + 1, st));
            LZX_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, d_keys, d_keys2, d_vals, d_vals2, g.entries, 0, 64, st));
            LZX_HIP(hipcub::DeviceReduce::ReduceByKey(nullptr, reduce_b, d_keys2, d_keys, d_vals2, d_vals, d_runs, hipcub::Sum(), g.entries, st));
            if (std::max(scan_b, std::max(sort_b, reduce_b)) > tmp_bytes)
                LZX_FAIL(LZX_ERR_LIMIT, "%s: the scratch of the sort of %llu entries exceeds that of level 0 (%zu bytes)", fn_name, (ull)g.entries, tmp_bytes);
        }
        size_t tb = tmp_bytes;
        LZX_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, d_newid, d_newid, (u64)n + 1, st));
        u32 C = 0;
        LZX_HIP(hipMemcpyAsync(&C, d_newid + n, sizeof(u32), hipMemcpyDeviceToHost, st));
        LZX_HIP(hipStreamSynchronize(st));
        if (C >= n) break;   // the level changed nothing: it is not counted

        lzx_with_lanes<32>(G, [&](auto lanes) {
            const dim3 grid(lzx_row_grid(n, LZX_COM_BLOCK / lanes));
            if (weighted) hipLaunchKernelGGL((k_agg_keys<lanes, true>), grid, dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, g.weights, (const u32 *)d_label, (const u32 *)d_newid, d_keys, d_vals, n, C);
            else hipLaunchKernelGGL((k_agg_keys<lanes, false>), grid, dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, g.weights, (const u32 *)d_label, (const u32 *)d_newid, d_keys, d_vals, n, C);
        });
        LZX_HIP(hipGetLastError());
        int key_bits = 33;
        while (key_bits < 64 && ((u64)C >> (key_bits - 32))) ++key_bits;
        tb = tmp_bytes;
        LZX_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp, tb, d_keys, d_keys2, d_vals, d_vals2, g.entries, 0, key_bits, st));
        tb = tmp_bytes;
        LZX_HIP(hipcub::DeviceReduce::ReduceByKey(d_tmp, tb, d_keys2, d_keys, d_vals2, d_vals, d_runs, hipcub::Sum(), g.entries, st));
        u32 runs = 0;
        LZX_HIP(hipMemcpyAsync(&runs, d_runs, sizeof(u32), hipMemcpyDeviceToHost, st));
        LZX_HIP(hipStreamSynchronize(st));
        u64 entries = std::min<u64>(runs, g.entries);
        if (entries) {
            u64 last = 0;
            LZX_HIP(hipMemcpy(&last, d_keys + entries - 1, sizeof(u64), hipMemcpyDeviceToHost));
            if ((last >> 32) >= C) --entries;   // the dropped diagonal entries' run
        }
        // the next level's graph: row_ptr u64 [C + 1], col_idx and weights u32 [entries]
        const u64 graph_bytes = ((u64)C + 1) * sizeof(u64) + 2 * lzx_even(entries) * sizeof(u32);
        std::snprintf(what, sizeof what, "the level graph of %u nodes and %llu entries", C, (ull)entries);
        LZX_TRY(lzx_alloc_state(fn_name, what, cap, held + graph_bytes, graph_bytes, &blocks.graph[1]));
        blocks.graph_bytes[1] = graph_bytes;
        u64 *d_rp = static_cast<u64 *>(blocks.graph[1]);
        u32 *d_ci = reinterpret_cast<u32 *>(d_rp + C + 1), *d_w = d_ci + lzx_even(entries);
        LZX_HIP(hipMemsetAsync(d_stats, 0, 2 * sizeof(u32), st));
        hipLaunchKernelGGL(k_agg_rows, dim3(lzx_vertex_grid(C + 1)), dim3(LZX_COM_BLOCK), 0, st, (const u64 *)d_keys, entries, d_rp, d_stats, C);
        if (entries) hipLaunchKernelGGL(k_agg_cols, dim3(entry_grid(entries)), dim3(LZX_COM_BLOCK), 0, st, (const u64 *)d_keys, (const u32 *)d_vals, d_ci, d_w, entries);
        hipLaunchKernelGGL(k_agg_compose, dim3(gb0), dim3(LZX_COM_BLOCK), 0, st, d_comp, (const u32 *)d_label, (const u32 *)d_newid, n0);
        LZX_HIP(hipGetLastError());
        u32 stats[2] = {0, 0};
        LZX_HIP(hipMemcpyAsync(stats, d_stats, sizeof(stats), hipMemcpyDeviceToHost, st));
        // the partition after this level, canonical (first: `queue`, out: `wait`, sizes: `colour` -- the colouring is done with them)
        if (level_labels) {
            LZX_HIP(hipMemsetAsync(s.counters, 0, CW_WORDS * sizeof(u32), st));
            LZX_TRY(lzx_comm_canonical(c, d_comp, n0, s.queue, s.wait, s.colour, s.counters));
            LZX_HIP(hipMemcpyAsync(level_labels + (size_t)counted * n0, s.wait, sizeof(u32) * n0, hipMemcpyDeviceToHost, st));
        }
        LZX_HIP(hipEventRecord(run.ev3, st));
        LZX_HIP(hipStreamSynchronize(st));
        LZX_HIP(hipEventElapsedTime(&ms, run.ev2, run.ev3));
        aggregate_ms += ms;
        if (levels) {
            lzx_louvain_level *L = levels + counted;
            L->nodes = n;
            L->entries = g.entries;
            L->communities = C;
            L->moves = moves;
            L->inner_entries = inner;
            L->sum_degree_sq = sum_sq;
            L->colors = col.colours;
            L->color_rounds = col.rounds;
            L->sweeps = sweeps;
            L->reverted = reverted;
            L->capped = capped;
            for (u32 p = 0; p < 3; ++p) L->path_rows[p] = path_rows[p];
        }
        ++counted;
        total_sweeps += sweeps;
        total_moves += moves;
        // the next level takes the place of this one
        blocks.drop(blocks.graph[0], blocks.graph_bytes[0]);
        blocks.graph[0] = blocks.graph[1];
        blocks.graph_bytes[0] = blocks.graph_bytes[1];
        blocks.graph[1] = nullptr;
        blocks.graph_bytes[1] = 0;
        held = bytes + scratch_bytes + blocks.graph_bytes[0];
        g = LzxGraphView{d_rp, d_ci, d_w, C, entries, stats[0], stats[1]};
    }

    // ---- the result: canonical labels, the statistics, the modularity on the handle's pattern ----
    const LzxGraphView g0 = lzx_view_of(c);
    LZX_TRY(lzx_color_degrees(c, g0, s.d, nullptr, s.counters));   // (the degrees of level 0 again, the counter words 0)
    u32 *d_out = s.wait;
    LZX_TRY(lzx_comm_canonical(c, d_comp, n0, s.queue, d_out, s.colour, s.counters));
    u32 cw[CW_WORDS];
    LZX_HIP(hipMemcpyAsync(cw, s.counters, sizeof(cw), hipMemcpyDeviceToHost, st));
    std::vector<u64> hD, hI;
    LzxModResult mod;
    LZX_TRY(lzx_modularity_core(c, g0, d_out, s.d, s.queue, d_D, d_I, hD, hI, &mod));
    if (labels) LZX_HIP(hipMemcpyAsync(labels, d_out, sizeof(u32) * n0, hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    if (info) {
        const u64 key = (u64)cw[CW_KEY] | ((u64)cw[CW_KEY + 1] << 32);
        info->n_communities = cw[CW_COMMUNITIES];
        info->largest_size = key >> 32;
        info->sweeps = total_sweeps;
        info->moves = total_moves;
        info->inner_entries = mod.inner;
        info->entries = mod.entries;
        info->sum_degree_sq = mod.sum_sq;
        info->largest_label = LZX_COM_NONE - (u32)(key & 0xffffffffull);
        info->levels = counted;
        info->modularity = mod.q;
        info->color_ms = color_ms;
        info->sweep_ms = sweep_ms;
        info->aggregate_ms = aggregate_ms;
        info->loop_ms = lzx_ms_since(t0);
    }
    return LZX_OK;
}
