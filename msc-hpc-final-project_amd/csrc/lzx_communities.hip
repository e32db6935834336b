// lzx_communities.hip -- greedy colouring, label-propagation communities and modularity of the handle's graph
// (networkx.coloring.greedy_color, networkx.community.label_propagation_communities, networkx.community.modularity), on the
// device over the caller-order CSR the handle keeps (d_row_ptr / d_col_idx): include/lzx.h, lzx_color, lzx_label_propagation and
// lzx_modularity; DESIGN.md section 21.  The colouring, the counting passes, the class sort, the far tables, the canonical labels and
// the modularity read a graph through an LzxGraphView (lzx_communities_shared.h): the three calls here pass the handle's, lzx_louvain
// (lzx_louvain.hip) the level graph at hand.
//
// Definitions.  d_v = the entries of row v without the diagonal; a diagonal entry is skipped in every walk.
//   order        u comes before v iff d_u > d_v, or the degrees are equal and hash(u) < hash(v) (the header's probe hash with
//                p = 0; left out with LZX_COLOR_TIES_BY_ID), or both are equal and u < v
//   colour       color[v] = the smallest colour no earlier neighbour has: sequential greedy colouring in that order
//   propagation  label[v] = v; a sweep visits the colour classes in ascending colour and gives every vertex of the class that has a
//                neighbour the label that maximises (multiplicity among its neighbours' labels, label == old, label); the call
//                ends with the first sweep that changes nothing; labels[v] = the smallest id of v's community
//   modularity   D_c = the sum of d_v over community c, I_c = the off-diagonal entries with both ends in c, M = the sum of D_c:
//                Q = the sum over the labels that occur, ascending, of I_c / M - (D_c / M)^2
//
// Colouring: Jones-Plassmann in push form, lzx_core.hip's structure.  wait[v] = the earlier neighbours of v, and `queue` is one
// queue in which every vertex is placed exactly once: a round's window [beg, end) holds the vertices whose earlier neighbours are
// all coloured, and what a launch appends behind `end` is the next window.
//   degrees    k_color_degrees       one thread per row: lzx_degree_no_diagonal, colour = none, the counters 0
//   wait       k_row_count<G>        G lanes per row count the earlier neighbours (k_row_count_long: a workgroup per row of more
//                                    than long_row entries); k_color_start appends the vertices with none: window 1
//   round      k_color_round<G>      G lanes per row of the window.  (1) the minimum excluded colour over the earlier neighbours,
//                                    all coloured by earlier launches: a 64-colour window mask is or-ed across the group, and
//                                    while it is full the window moves up by 64 and the row is walked again (at most len / 64 + 1
//                                    walks).  (2) for every later neighbour u, old = atomicSub(&wait[u], 1), and the one lane that
//                                    sees old == 1 appends u: the next launch colours it and sees v's colour
//              k_color_round_long    the window's rows of more than long_row entries, a workgroup per row: the colours of the
//                                    earlier neighbours go into an LDS bitmap.  An earlier neighbour has degree >= d_v, so a vertex
//                                    has fewer than 2^16 of them while nnz < 2^32: colours are < 2^16 and 8 KiB suffice
// The number of windows is the longest chain of the order, so it is canonical, like the colours.
//
// Classes: a counting sort of the vertices by (colour, path) -- k_class_sort<false> the histogram, the host the scan (three words
// per colour), k_class_sort<true> the fill -- so that every (class, path) is one run of `cls` and one launch with exactly its rows.
//
// Propagation, in place (the vertices of a class share no edge, so a launch reads only labels it does not write).  The pass over
// the classes, the wave insert and the far insert are lzx_class_sweep.h's, which lzx_louvain shares; the decide kernels are these:
//   short   k_lpa_group<G>        rows of at most lpa_group_row entries (128).  G lanes per row; the neighbours' labels are staged in
//                                 the group's LDS slice (the first 128; a longer row, which only the test shape sends here, reads
//                                 the rest where it lies); every lane counts, for its own entries, the equal labels in the row, and
//                                 the key  count << 33 | (label == old) << 32 | label  is max-reduced over the group
//   medium  k_lpa_table           rows of at most lpa_table_row entries (2048): a workgroup per row and an open-addressing table in
//                                 LDS, keys u32 and counts u32, pow2ceil(2 len) of its 4096 slots (32 KiB: five workgroups per
//                                 compute unit, twenty of its thirty-two wavefronts): atomicCAS on the key slot, atomicAdd on the
//                                 count, linear probing bounded by the slot count, never more than half full; then the maximum of
//                                 the same key over the slots
//   long    k_class_far_insert<W> the same insertion into a table of pow2ceil(2 len) slots in global memory, at an offset from a scan
//           k_lpa_far_pick        over the long rows made once per call: up to 64 workgroups share the entries of a row (one alone
//                                 is a chain of dependent round trips per 256 entries), and a second launch, the workgroup that owns
//                                 the table, takes the maximum and clears the slots it read.  The tables are zeroed once per call.
// The new label is an arg-max under a total order: it depends neither on the path a row takes nor on any thread order.  Changed
// labels are counted per wavefront into one word, which the host reads once per sweep.
//
// All atomics are integer vector atomics, 32-bit everywhere but in the modularity's accumulators and the largest community's
// key (64-bit); nothing in the colouring or the propagation is floating-point.  No kernel waits on another workgroup; every
// device loop is bounded by a row length, a window length or a table size; every append is clamped to n.  A matrix that is not
// symmetric is not detected and its numbers mean nothing, but a counter that wraps can append a vertex at most once more in 2^32
// decrements, the appends are clamped, the rounds and the sweeps are capped, and every label read is a vertex id.
#include <algorithm>
#include <chrono>
#include <vector>

#include "lzx_internal.h"
#include "lzx_graph_call.h"
#include "lzx_class_sweep.h"
#include "lzx_spmv_body.h"
#include "lzx_reduce.h"

// ---- the order (ColorOrder: lzx_communities_shared.h) -------------------------------------------------------------------------
// what k_row_count counts in row v: the earlier neighbours; the neighbours with v's label
struct PredEarlier {
    ColorOrder o;
    __device__ __forceinline__ bool operator()(u32 v, u32 u) const { return o.before(u, v); }
};
struct PredSameLabel {
    const u32 *label;
    __device__ __forceinline__ bool operator()(u32 v, u32 u) const { return label[u] == label[v]; }
};

// ---- rows counted under a predicate -----------------------------------------------------------------------------------------
// out[v] = the entries u != v of row v with pred(v, u): rows of at most long_row entries, G lanes per row
template <u32 G, typename P>
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_row_count(const u64 *row_ptr, const u32 *col_idx, P pred, u32 *out, u32 n, u32 long_row)
{
    const u32 sub = threadIdx.x & (G - 1);
    const u64 row = (u64)blockIdx.x * (LZX_COM_BLOCK / G) + threadIdx.x / G;
    u64 beg = 0;
    u32 len = 0;
    bool mine = false;
    if (row < n) {
        beg = row_ptr[row];
        const u64 l = row_ptr[row + 1] - beg;
        mine = l <= long_row;   // the others are k_row_count_long's
        len = mine ? (u32)l : 0u;
    }
    u32 cnt = 0;
    for (u32 e = sub; e < len; e += G) {
        const u32 u = col_idx[beg + e];
        if (u != (u32)row && pred((u32)row, u)) ++cnt;
    }
    cnt = lzx_group_sum_u32<G>(cnt);
    if (sub == 0 && mine) out[row] = cnt;
}

// rows of more than long_row entries among the workgroup's 256 rows: the whole workgroup per row
template <typename P>
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_row_count_long(const u64 *row_ptr, const u32 *col_idx, P pred, u32 *out, u32 n, u32 long_row)
{
    __shared__ u32 s_rows[LZX_COM_BLOCK];
    __shared__ u32 s_count;
    __shared__ u32 s_part[LZX_COM_BLOCK / 64];
    const u64 mine = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    const u32 count = lzx_collect_long_rows(mine < n && row_ptr[mine + 1] - row_ptr[mine] > long_row, (u32)mine, s_rows, &s_count);
    for (u32 i = 0; i < count; ++i) {
        const u32 v = s_rows[i];
        const u64 beg = row_ptr[v], end = row_ptr[v + 1];
        u32 cnt = 0;
        for (u64 e = beg + threadIdx.x; e < end; e += LZX_COM_BLOCK) {
            const u32 u = col_idx[e];
            if (u != v && pred(v, u)) ++cnt;
        }
        cnt = lzx_wave_sum_u32(cnt);
        if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) out[v] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
        __syncthreads();
    }
}

// ---- colouring --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_color_degrees(const u64 *row_ptr, const u32 *col_idx, u32 *d, u32 *colour, u32 *counters, u32 n)
{
    const u64 v = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    if (v < CW_WORDS) counters[v] = 0;
    if (v >= n) return;
    d[v] = lzx_degree_no_diagonal(row_ptr, col_idx, v);
    if (colour) colour[v] = LZX_COM_NONE;
}

// window 1: the vertices without an earlier neighbour
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_color_start(const u32 *wait, u32 *queue, u32 *counters, u32 n)
{
    const u64 v = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    const bool take = v < n && wait[v] == 0;
    const u32 at = lzx_wave_append(take, &counters[CW_END]);
    if (take && at < n) queue[at] = (u32)v;
}

// one later neighbour u of a window's vertex (later: this lane holds one): the decrement and the append
__device__ __forceinline__ void color_push(bool later, u32 u, u32 *wait, u32 *queue, u32 *counters, u32 n)
{
    bool take = false;
    if (later) take = atomicSub(&wait[u], 1u) == 1u;
    const u32 at = lzx_wave_append(take, &counters[CW_END]);
    if (take && at < n) queue[at] = u;
}

// rows of the window queue[wbeg .. wbeg + wlen) with at most long_row entries: G lanes per row, 256 / G rows per workgroup
template <u32 G>
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_color_round(const u64 *row_ptr, const u32 *col_idx, ColorOrder o, u32 *wait, u32 *colour, u32 *queue, u32 *counters, u32 n, u32 wbeg,
              u32 wlen, u32 long_row)
{
    const u32 sub = threadIdx.x & (G - 1);
    const u64 idx = (u64)blockIdx.x * (LZX_COM_BLOCK / G) + threadIdx.x / G;
    u64 beg = 0;
    u32 len = 0, v = 0;
    bool mine = false;
    if (idx < wlen) {
        v = queue[wbeg + idx];
        beg = row_ptr[v];
        const u64 l = row_ptr[v + 1] - beg;
        mine = l <= long_row;   // the others are k_color_round_long's
        len = mine ? (u32)l : 0u;
    }
    // (1) the minimum excluded colour.  `mine`, the mask after the butterfly and so every branch are the same across the group.
    u32 top = 0;   // colour + 1
    if (mine) {
        u32 c = 0;
        for (u32 base = 0, walk = 0; walk <= len / 64; ++walk, base += 64) {
            ull mask = 0;
            for (u32 e = sub; e < len; e += G) {
                const u32 u = col_idx[beg + e];
                if (u != v && o.before(u, v)) {
                    const u32 off = colour[u] - base;   // (below the window, and none: wraps to a large number)
                    if (off < 64u) mask |= 1ull << off;
                }
            }
#pragma unroll
            for (u32 w = G / 2; w > 0; w >>= 1) mask |= __shfl_xor(mask, (int)w, 64);
            c = base + 64;
            if (mask != ~0ull) {
                c = base + (u32)__builtin_ctzll(~mask);
                break;
            }
        }
        c = min(c, LZX_COLOR_CAP - 1);
        if (sub == 0) {
            colour[v] = c;
            top = c + 1;
        }
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) top = max(top, (u32)__shfl_xor((int)top, w, 64));
    if ((threadIdx.x & 63) == 0 && top) atomicMax(&counters[CW_COLORS], top);
    // (2) the later neighbours (the same trips for every lane of the wavefront: the appends are formed together)
    u32 trips = (len + G - 1) / G;
#pragma unroll
    for (int w = 32; w >= (int)G; w >>= 1) trips = max(trips, (u32)__shfl_xor((int)trips, w, 64));
    for (u32 t = 0; t < trips; ++t) {
        const u32 e = t * G + sub;
        u32 u = v;
        if (e < len) u = col_idx[beg + e];
        color_push(u != v && !o.before(u, v), u, wait, queue, counters, n);
    }
}

// rows of more than long_row entries among the workgroup's 256 window places: the whole workgroup per row
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_color_round_long(const u64 *row_ptr, const u32 *col_idx, ColorOrder o, u32 *wait, u32 *colour, u32 *queue, u32 *counters, u32 n, u32 wbeg,
                   u32 wlen, u32 long_row)
{
    __shared__ u32 s_rows[LZX_COM_BLOCK];
    __shared__ u32 s_count;
    __shared__ u32 s_bits[LZX_COLOR_CAP / 32];
    __shared__ u32 s_min[LZX_COM_BLOCK / 64];
    const u64 idx = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    const u32 mine = idx < wlen ? queue[wbeg + idx] : 0u;
    const u32 count = lzx_collect_long_rows(idx < wlen && row_ptr[mine + 1] - row_ptr[mine] > long_row, mine, s_rows, &s_count);
    for (u32 i = 0; i < count; ++i) {
        const u32 v = s_rows[i];
        const u64 beg = row_ptr[v], end = row_ptr[v + 1];
        // at most len earlier neighbours, so a colour of the first len + 1 is free
        const u64 want = (end - beg) / 32 + 1;
        const u32 words = want < LZX_COLOR_CAP / 32 ? (u32)want : LZX_COLOR_CAP / 32;
        for (u32 w = threadIdx.x; w < words; w += LZX_COM_BLOCK) s_bits[w] = 0;
        __syncthreads();
        for (u64 e = beg + threadIdx.x; e < end; e += LZX_COM_BLOCK) {
            const u32 u = col_idx[e];
            if (u != v && o.before(u, v)) {
                const u32 cu = colour[u];
                if (cu < words * 32) atomicOr(&s_bits[cu >> 5], 1u << (cu & 31));
            }
        }
        __syncthreads();
        u32 m = LZX_COM_NONE;
        for (u32 w = threadIdx.x; w < words; w += LZX_COM_BLOCK) {
            const u32 free_bits = ~s_bits[w];
            if (free_bits) {
                m = w * 32 + (u32)__builtin_ctz(free_bits);
                break;   // (a thread's words ascend)
            }
        }
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) m = min(m, (u32)__shfl_xor((int)m, w, 64));
        if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            const u32 c = min(min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3])), LZX_COLOR_CAP - 1);
            colour[v] = c;
            atomicMax(&counters[CW_COLORS], c + 1);
        }
        // (the same trips for every lane of the workgroup)
        for (u64 e0 = beg; e0 < end; e0 += LZX_COM_BLOCK) {
            const u64 e = e0 + threadIdx.x;
            u32 u = v;
            if (e < end) u = col_idx[e];
            color_push(u != v && !o.before(u, v), u, wait, queue, counters, n);
        }
        __syncthreads();
    }
}

// ---- the classes: a counting sort by (colour, path) ---------------------------------------------------------------------------
// bins[3 colour + path]: counted (!FILL), or the run's cursor, behind which the vertex is written into cls (FILL)
template <bool FILL>
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_class_sort(const u64 *row_ptr, const u32 *colour, u32 *bins, u32 *cls, u32 n, u32 colours, u32 group_row, u32 table_row)
{
    const u64 v = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    bool active = false;
    u32 key = 0;
    if (v < n) {
        const u32 c = colour[v];
        const u64 len = row_ptr[v + 1] - row_ptr[v];
        active = c < colours;
        key = 3 * c + (len <= group_row ? 0u : len <= table_row ? 1u : 2u);
    }
    const u32 at = wave_bucket_add(active, key, bins);
    if (FILL && active && at < n) cls[at] = (u32)v;
}

// ---- propagation --------------------------------------------------------------------------------------------------------------
// the rows of more than table_row entries: lpos[v] = the row's place in the list, llen[place] = its length
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_lpa_long_rows(const u64 *row_ptr, u32 *lpos, u32 *llen, u32 *counters, u32 n, u32 table_row)
{
    const u64 v = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    u64 len = 0;
    if (v < n) len = row_ptr[v + 1] - row_ptr[v];
    const bool take = len > table_row;
    const u32 at = lzx_wave_append(take, &counters[CW_LONG]);
    if (take && at < n) {
        lpos[v] = at;
        llen[at] = (u32)len;
    }
}

__device__ __forceinline__ ull lpa_key(u32 count, u32 label, u32 old) { return ((ull)count << 33) | ((ull)(label == old) << 32) | label; }

// the rows cls[sbeg .. sbeg + slen): G lanes per row, 256 / G rows per workgroup, 128 labels of LDS per row
template <u32 G>
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_lpa_group(const u64 *row_ptr, const u32 *col_idx, u32 *label, const u32 *cls, u32 sbeg, u32 slen, u32 *counters)
{
    __shared__ u32 s_lab[(LZX_COM_BLOCK / G) * LZX_LPA_STAGE];
    u32 *slice = s_lab + (threadIdx.x / G) * LZX_LPA_STAGE;
    const u32 sub = threadIdx.x & (G - 1);
    const u64 idx = (u64)blockIdx.x * (LZX_COM_BLOCK / G) + threadIdx.x / G;
    u64 beg = 0;
    u32 len = 0, v = 0, old = 0;
    if (idx < slen) {
        v = cls[sbeg + idx];
        beg = row_ptr[v];
        len = (u32)(row_ptr[v + 1] - beg);
        old = label[v];
    }
    // the label of entry j, none for the diagonal
    auto fetch = [&](u32 j) {
        const u32 u = col_idx[beg + j];
        return u == v ? LZX_COM_NONE : label[u];
    };
    const u32 staged = min(len, LZX_LPA_STAGE);
    for (u32 j = sub; j < staged; j += G) slice[j] = fetch(j);
    __syncthreads();
    ull best = 0;
    for (u32 j = sub; j < len; j += G) {
        const u32 mine = j < staged ? slice[j] : fetch(j);
        if (mine == LZX_COM_NONE) continue;
        u32 count = 0;
        for (u32 i = 0; i < staged; ++i) count += slice[i] == mine;
        for (u32 i = staged; i < len; ++i) count += fetch(i) == mine;
        const ull key = lpa_key(count, mine, old);
        best = key > best ? key : best;
    }
#pragma unroll
    for (u32 w = G / 2; w > 0; w >>= 1) {
        const ull other = __shfl_xor(best, (int)w, 64);
        best = other > best ? other : best;
    }
    const bool changed = sub == 0 && best != 0 && (u32)best != old;
    if (changed) label[v] = (u32)best;
    const ull m = __ballot(changed);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&counters[CW_CHANGED], (u32)__builtin_popcountll(m));
}

// the workgroup's largest key (in thread 0) becomes v's label
__device__ __forceinline__ void lpa_take(ull best, u32 v, u32 old, u32 *label, u32 *counters, ull *s_k)
{
    best = wave_max_u64(best);
    if ((threadIdx.x & 63) == 0) s_k[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        best = block_max_u64(s_k);
        if (best != 0 && (u32)best != old) {
            label[v] = (u32)best;
            atomicAdd(&counters[CW_CHANGED], 1u);
        }
    }
}

// the rows cls[sbeg .. sbeg + gridDim.x): a workgroup per row over a table of pow2ceil(2 len) slots in LDS
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_lpa_table(const u64 *row_ptr, const u32 *col_idx, u32 *label, const u32 *cls, u32 sbeg, u32 *counters)
{
    __shared__ u32 s_table[2 * LZX_LPA_SLOTS];
    __shared__ ull s_k[LZX_COM_BLOCK / 64];
    const u32 v = cls[sbeg + blockIdx.x];
    const u64 beg = row_ptr[v], end = row_ptr[v + 1];
    const u32 old = label[v];
    const u32 slots = lpa_slots(end - beg, LZX_LPA_SLOTS);
    u32 *keys = s_table, *counts = s_table + slots;
    for (u32 s = threadIdx.x; s < 2 * slots; s += LZX_COM_BLOCK) s_table[s] = 0;
    __syncthreads();
    for (u64 e0 = beg; e0 < end; e0 += LZX_COM_BLOCK) {   // (the same trips for every lane of the workgroup)
        const u64 e = e0 + threadIdx.x;
        const u32 u = e < end ? col_idx[e] : v;
        lzx_insert_wave<false>(u != v, u != v ? label[u] : 0u, 1u, keys, counts, slots);
    }
    __syncthreads();
    ull best = 0;
    for (u32 s = threadIdx.x; s < slots; s += LZX_COM_BLOCK) {
        const u32 k = keys[s];
        const ull key = k ? lpa_key(counts[s], k - 1, old) : 0ull;
        best = key > best ? key : best;
    }
    lpa_take(best, v, old, label, counters, s_k);
}

// The rows cls[sbeg .. sbeg + gridDim.x) of more entries, after k_class_far_insert (lzx_class_sweep.h): the workgroup that owns the
// row's table takes the maximum over its slots and clears them
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_lpa_far_pick(const u64 *row_ptr, u32 *label, const u32 *cls, u32 sbeg, const u32 *lpos, const u64 *loff, u32 *tables, u32 *counters)
{
    __shared__ ull s_k[LZX_COM_BLOCK / 64];
    const u32 v = cls[sbeg + blockIdx.x];
    const u32 old = label[v];
    const u32 slots = lpa_slots(row_ptr[v + 1] - row_ptr[v], 1u << 31);
    u32 *keys = tables + 2 * loff[lpos[v]], *counts = keys + slots;
    ull best = 0;
#pragma unroll 4
    for (u32 s = threadIdx.x; s < slots; s += LZX_COM_BLOCK) {
        const u32 k = keys[s], count = counts[s];
        const ull key = k ? lpa_key(count, k - 1, old) : 0ull;
        best = key > best ? key : best;
        if (k) {
            keys[s] = 0;
            counts[s] = 0;
        }
    }
    lpa_take(best, v, old, label, counters, s_k);
}

// ---- the communities' canonical labels and their statistics ----------------------------------------------------------------------
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_comm_first(const u32 *label, u32 *first, u32 n)
{
    const u64 v = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    // (the plain read only spares atomics on a community's address: a stale value is larger, and then the atomic decides)
    if (v < n && label[v] < n && first[label[v]] > (u32)v) atomicMin(&first[label[v]], (u32)v);
}

// out[v] = the smallest id of v's community; sizes[that id] counts its vertices
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_comm_gather(const u32 *label, const u32 *first, u32 *out, u32 *sizes, u32 n)
{
    const u64 v = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    u32 r = 0;
    if (v < n) {
        r = label[v] < n ? first[label[v]] : (u32)v;
        out[v] = r;
    }
    wave_bucket_add(v < n, r, sizes);
}

// counters[CW_COMMUNITIES] = the communities; the u64 at counters[CW_KEY] = the largest size << 32 | ~label: ties go to the smallest
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_comm_stats(const u32 *out, const u32 *sizes, u32 *counters, u32 n)
{
    const u64 v = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    const bool root = v < n && out[v] == (u32)v;
    const ull roots = __ballot(root);
    const ull key = wave_max_u64(root ? ((ull)sizes[v] << 32) | (LZX_COM_NONE - (u32)v) : 0ull);
    if ((threadIdx.x & 63) == 0 && roots) {
        atomicAdd(&counters[CW_COMMUNITIES], (u32)__builtin_popcountll(roots));
        atomicMax(reinterpret_cast<ull *>(counters + CW_KEY), key);
    }
}

// ---- modularity ---------------------------------------------------------------------------------------------------------------
// D[label[v]] += d[v], I[label[v]] += inner[v]: the lanes of a wavefront whose labels agree are combined first, for the labels of
// the wavefront's first four leaders; what is left adds for itself
__global__ void __launch_bounds__(LZX_COM_BLOCK)
k_mod_add(const u32 *label, const u32 *d, const u32 *inner, ull *D, ull *I, u32 n)
{
    const u64 v = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    const u32 lane = threadIdx.x & 63;
    bool active = v < n && label[v] < n;
    const u32 key = active ? label[v] : 0u;
    const ull dv = active ? d[v] : 0u, iv = active ? inner[v] : 0u;
    ull todo = __ballot(active);
    for (int it = 0; it < 4 && todo; ++it) {   // (the same trips for every lane)
        const int leader = __builtin_ctzll(todo);
        const u32 k0 = (u32)__shfl((int)key, leader, 64);
        const bool mine = active && key == k0;
        const ull sd = wave_sum_u64(mine ? dv : 0ull), si = wave_sum_u64(mine ? iv : 0ull);
        if (lane == (u32)leader) {
            if (sd) atomicAdd(&D[k0], sd);
            if (si) atomicAdd(&I[k0], si);
        }
        if (mine) active = false;
        todo = __ballot(active);
    }
    if (active) {
        if (dv) atomicAdd(&D[key], dv);
        if (iv) atomicAdd(&I[key], iv);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
namespace {
// out[v] = the entries of row v that satisfy pred: both launches
template <typename P>
int count_rows(lzx_ctx *c, const LzxGraphView &g_, P pred, u32 *out, u32 G, u32 long_row)
{
    const u32 n = g_.n;
    lzx_with_lanes<32>(G, [&](auto g) {
        hipLaunchKernelGGL((k_row_count<g, P>), dim3(lzx_row_grid(n, LZX_COM_BLOCK / g)), dim3(LZX_COM_BLOCK), 0, c->stream, g_.row_ptr,
                           g_.col_idx, pred, out, n, long_row);
    });
    LZX_HIP(hipGetLastError());
    if (g_.max_row > long_row) {
        hipLaunchKernelGGL(k_row_count_long<P>, dim3(lzx_vertex_grid(n)), dim3(LZX_COM_BLOCK), 0, c->stream, g_.row_ptr, g_.col_idx, pred, out, n,
                           long_row);
        LZX_HIP(hipGetLastError());
    }
    return LZX_OK;
}
}   // namespace

int lzx_color_degrees(lzx_ctx *c, const LzxGraphView &g, u32 *d, u32 *colour, u32 *counters)
{
    hipLaunchKernelGGL(k_color_degrees, dim3(std::max(lzx_vertex_grid(g.n), 1u)), dim3(LZX_COM_BLOCK), 0, c->stream, g.row_ptr, g.col_idx, d, colour,
                       counters, g.n);
    LZX_HIP(hipGetLastError());
    return LZX_OK;
}

int lzx_color_core(lzx_ctx *c, const LzxGraphView &g, LzxGraphRun &run, const char *fn_name, u64 seed, u32 flags, const LzxColorState &s, bool sorted,
                   u32 group_row, u32 table_row, LzxColorResult *res)
{
    const u32 n = g.n;
    hipStream_t st = c->stream;
    const u32 G = lzx_lanes_of(c, g);
    const u32 long_row = lzx_shape_or(c->color_long_opt, 64 * G);
    const u32 gb = lzx_vertex_grid(n);
    const ColorOrder order{s.d, seed, flags & LZX_COLOR_TIES_BY_ID};

    LZX_HIP(hipEventRecord(run.ev0, st));
    LZX_TRY(lzx_color_degrees(c, g, s.d, s.colour, s.counters));
    LZX_TRY(count_rows(c, g, PredEarlier{order}, s.wait, G, long_row));
    hipLaunchKernelGGL(k_color_start, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, s.wait, s.queue, s.counters, n);
    LZX_HIP(hipGetLastError());
    u32 words[2] = {0, 0};   // the queue's end, the colours
    LZX_HIP(hipMemcpyAsync(words, s.counters, sizeof(words), hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    u32 wbeg = 0, queued = std::min(words[0], n), rounds = 0;
    while (queued > wbeg) {   // the window [wbeg, queued)
        ++rounds;
        if ((u64)rounds > (u64)n + 1) LZX_FAIL(LZX_ERR_LIMIT, "%s: %u rounds on %u vertices", fn_name, rounds, n);
        const u32 wlen = queued - wbeg;
        lzx_with_lanes<32>(G, [&](auto lanes) {
            hipLaunchKernelGGL(k_color_round<lanes>, dim3(lzx_row_grid(wlen, LZX_COM_BLOCK / lanes)), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx,
                               order, s.wait, s.colour, s.queue, s.counters, n, wbeg, wlen, long_row);
        });
        LZX_HIP(hipGetLastError());
        if (g.max_row > long_row) {
            hipLaunchKernelGGL(k_color_round_long, dim3((wlen + LZX_COM_BLOCK - 1) / LZX_COM_BLOCK), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr,
                               g.col_idx, order, s.wait, s.colour, s.queue, s.counters, n, wbeg, wlen, long_row);
            LZX_HIP(hipGetLastError());
        }
        LZX_HIP(hipMemcpyAsync(words, s.counters, sizeof(words), hipMemcpyDeviceToHost, st));
        LZX_HIP(hipStreamSynchronize(st));
        wbeg = queued;
        queued = std::min(words[0], n);
    }
    if (queued < n)
        LZX_FAIL(LZX_ERR_LIMIT, "%s: %u of %u vertices still wait for an earlier neighbour after %u rounds -- the matrix is not symmetric", fn_name,
                 n - queued, n, rounds);
    const u32 colours = std::min(words[1], std::min(n, LZX_COLOR_CAP));
    // the classes: histogram, scan, fill
    const u32 nb = 3 * colours;
    res->run.assign((size_t)nb + 1, 0);
    LZX_HIP(hipMemsetAsync(s.bins, 0, sizeof(u32) * nb, st));
    hipLaunchKernelGGL(k_class_sort<false>, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, s.colour, s.bins, s.queue, n, colours, group_row, table_row);
    LZX_HIP(hipGetLastError());
    LZX_HIP(hipMemcpyAsync(res->run.data() + 1, s.bins, sizeof(u32) * nb, hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    u32 largest = 0;
    for (u32 k = 0; k < colours; ++k) largest = std::max(largest, res->run[3 * k + 1] + res->run[3 * k + 2] + res->run[3 * k + 3]);
    for (u32 b = 0; b < nb; ++b) res->run[b + 1] += res->run[b];
    if (sorted) {
        LZX_HIP(hipMemcpyAsync(s.bins, res->run.data(), sizeof(u32) * nb, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_class_sort<true>, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, s.colour, s.bins, s.queue, n, colours, group_row,
                           table_row);
        LZX_HIP(hipGetLastError());
    }
    LZX_HIP(hipEventRecord(run.ev1, st));
    LZX_HIP(hipStreamSynchronize(st));
    LZX_HIP(hipEventElapsedTime(&res->ms, run.ev0, run.ev1));
    res->colours = colours;
    res->rounds = rounds;
    res->largest_class = largest;
    return LZX_OK;
}

int lzx_modularity_core(lzx_ctx *c, const LzxGraphView &g, const u32 *d_label, const u32 *d_d, u32 *d_inner, ull *d_D, ull *d_I, std::vector<u64> &hD,
                        std::vector<u64> &hI, LzxModResult *res)
{
    const u32 n = g.n;
    hipStream_t st = c->stream;
    const u32 G = lzx_lanes_of(c, g);
    LZX_TRY(count_rows(c, g, PredSameLabel{d_label}, d_inner, G, 64 * G));
    LZX_HIP(hipMemsetAsync(d_D, 0, sizeof(ull) * n, st));
    LZX_HIP(hipMemsetAsync(d_I, 0, sizeof(ull) * n, st));
    hipLaunchKernelGGL(k_mod_add, dim3(lzx_vertex_grid(n)), dim3(LZX_COM_BLOCK), 0, st, d_label, d_d, d_inner, d_D, d_I, n);
    LZX_HIP(hipGetLastError());
    hD.resize(n);
    hI.resize(n);
    LZX_HIP(hipMemcpyAsync(hD.data(), d_D, sizeof(u64) * n, hipMemcpyDeviceToHost, st));
    LZX_HIP(hipMemcpyAsync(hI.data(), d_I, sizeof(u64) * n, hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    u64 M = 0, inner = 0, sq = 0;
    for (u32 k = 0; k < n; ++k) {
        M += hD[k];
        inner += hI[k];
        sq += hD[k] * hD[k];
    }
    // ascending label, one rounding per operation (the library is built without contraction).  A label that does not occur, or
    // occurs on isolated vertices only, has D = I = 0 and adds nothing.
    double q = 0.0;
    if (M)
        for (u32 k = 0; k < n; ++k)
            if (hD[k]) {
                const double x = (double)hD[k] / (double)M;
                const double sqx = x * x;
                const double term = (double)hI[k] / (double)M - sqx;
                q = q + term;
            }
    res->q = q;
    res->inner = inner;
    res->entries = M;
    res->sum_sq = sq;
    return LZX_OK;
}

int lzx_lpa_far_tables(lzx_ctx *c, const LzxGraphView &g, const char *fn_name, u32 table_above, int64_t cap, u64 held, u32 *d_lpos, u32 *d_llen,
                       u64 *d_loff, u32 *counters, void **tables, u64 *table_bytes)
{
    const u32 n = g.n;
    hipStream_t st = c->stream;
    *tables = nullptr;
    *table_bytes = 0;
    hipLaunchKernelGGL(k_lpa_long_rows, dim3(lzx_vertex_grid(n)), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, d_lpos, d_llen, counters, n, table_above);
    LZX_HIP(hipGetLastError());
    u32 nl = 0;
    LZX_HIP(hipMemcpyAsync(&nl, counters + CW_LONG, sizeof(u32), hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    nl = std::min(nl, n);
    if (!nl) return LZX_OK;
    std::vector<u32> len(nl);
    std::vector<u64> off((size_t)nl + 1, 0);
    LZX_HIP(hipMemcpy(len.data(), d_llen, sizeof(u32) * nl, hipMemcpyDeviceToHost));
    for (u32 i = 0; i < nl; ++i) {
        u64 slots = 2;
        while (slots < 2 * (u64)len[i]) slots *= 2;
        off[i + 1] = off[i] + slots;
    }
    *table_bytes = 2 * off[nl] * sizeof(u32);
    char what[128];
    std::snprintf(what, sizeof what, "the label tables of %u rows of more than %u entries", nl, table_above);
    LZX_TRY(lzx_alloc_state(fn_name, what, cap, held + *table_bytes, *table_bytes, tables));
    LZX_HIP(hipMemsetAsync(*tables, 0, *table_bytes, st));
    LZX_HIP(hipMemcpyAsync(d_loff, off.data(), sizeof(u64) * nl, hipMemcpyHostToDevice, st));
    LZX_HIP(hipStreamSynchronize(st));   // (off goes out of scope)
    return LZX_OK;
}

int lzx_comm_canonical(lzx_ctx *c, const u32 *d_label, u32 n, u32 *d_first, u32 *d_out, u32 *d_sizes, u32 *counters)
{
    hipStream_t st = c->stream;
    const u32 gb = lzx_vertex_grid(n);
    hipLaunchKernelGGL(k_fill_u32<false>, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, d_first, n, LZX_COM_NONE);
    hipLaunchKernelGGL(k_fill_u32<false>, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, d_sizes, n, 0u);
    hipLaunchKernelGGL(k_comm_first, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, d_label, d_first, n);
    hipLaunchKernelGGL(k_comm_gather, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, d_label, (const u32 *)d_first, d_out, d_sizes, n);
    hipLaunchKernelGGL(k_comm_stats, dim3(gb), dim3(LZX_COM_BLOCK), 0, st, (const u32 *)d_out, (const u32 *)d_sizes, counters, n);
    LZX_HIP(hipGetLastError());
    return LZX_OK;
}

extern "C" int lzx_color(lzx_handle c, uint64_t seed, uint32_t flags, uint32_t *color, lzx_color_info *info)
{
    const char *fn_name = "lzx_color";
    LZX_TRY(lzx_graph_call_check(c, fn_name, "a graph is coloured"));
    if (flags & ~LZX_COLOR_TIES_BY_ID) LZX_FAIL(LZX_ERR_ARG, "%s: unknown flag bits 0x%x (LZX_COLOR_TIES_BY_ID is the only flag)", fn_name, flags & ~LZX_COLOR_TIES_BY_ID);
    const auto t0 = std::chrono::steady_clock::now();
    const u32 n = (u32)c->n;
    const LzxGraphView g = lzx_view_of(c);

    LZX_HIP(hipSetDevice(c->device));
    LzxColorState s;
    LzxGraphRun run(c);
    char what[96];
    std::snprintf(what, sizeof what, "the state of %u vertices (degrees, waits, colours, the queue)", n);
    LZX_TRY(lzx_carve_state(fn_name, what, -1, 0, &run.arena, nullptr, [&](LzxCarver &k) {
        for (u32 **p : {&s.d, &s.wait, &s.colour, &s.queue}) k.take(*p, lzx_even(n));
        k.take(s.bins, lzx_class_bins(n));   // three per colour
        k.take(s.counters, CW_WORDS);
    }));
    LZX_TRY(run.events(2));
    LzxColorResult res;
    LZX_TRY(lzx_color_core(c, g, run, fn_name, seed, flags, s, false, 0xffffffffu, 0xffffffffu, &res));
    if (color) LZX_HIP(hipMemcpyAsync(color, s.colour, sizeof(u32) * n, hipMemcpyDeviceToHost, c->stream));
    LZX_HIP(hipStreamSynchronize(c->stream));
    if (info) {
        info->colors = res.colours;
        info->rounds = res.rounds;
        info->largest_class = res.largest_class;
        info->reserved_ = 0;
        info->color_ms = res.ms;
        info->loop_ms = lzx_ms_since(t0);
    }
    return LZX_OK;
}

extern "C" int lzx_label_propagation(lzx_handle c, uint64_t seed, uint32_t flags, uint32_t max_sweeps, uint32_t *labels,
                                     lzx_communities_info *info)
{
    const char *fn_name = "lzx_label_propagation";
    LZX_TRY(lzx_graph_call_check(c, fn_name, "labels are propagated"));
    if (flags & ~LZX_COLOR_TIES_BY_ID) LZX_FAIL(LZX_ERR_ARG, "%s: unknown flag bits 0x%x (LZX_COLOR_TIES_BY_ID is the only flag)", fn_name, flags & ~LZX_COLOR_TIES_BY_ID);
    if (max_sweeps == 0) LZX_FAIL(LZX_ERR_ARG, "%s: max_sweeps must be at least 1", fn_name);
    if (c->max_degree >= LZX_LPA_MAX_ROW) LZX_FAIL(LZX_ERR_LIMIT, "%s: a row of %llu entries; rows of 2^30 entries or more are not supported", fn_name, (ull)c->max_degree);
    const auto t0 = std::chrono::steady_clock::now();
    const u32 n = (u32)c->n;
    const LzxGraphView g = lzx_view_of(c);
    hipStream_t st = c->stream;
    LzxClassSweep cs(c);

    // the vertices' arena; the tables of the rows above table_row follow in one of their own once they are known
    LZX_HIP(hipSetDevice(c->device));
    ull *d_D, *d_I;
    LzxColorState s;
    u32 *d_label;
    u64 bytes = 0;
    LzxGraphRun run(c);
    char what[128];
    std::snprintf(what, sizeof what, "the state of %u vertices (degrees, colours, classes, labels, the modularity's sums)", n);
    LZX_TRY(lzx_carve_state(fn_name, what, c->lpa_cap_opt, 0, &run.arena, &bytes, [&](LzxCarver &k) {
        k.take(d_D, n);
        k.take(d_I, n);
        for (u32 **p : {&s.d, &s.wait, &s.colour, &s.queue, &d_label}) k.take(*p, lzx_even(n));
        k.take(s.bins, lzx_class_bins(n));   // three per colour
        k.take(s.counters, CW_WORDS);
    }));
    LZX_TRY(run.events(2));
    u64 table_bytes = 0;
    LZX_TRY(lzx_class_sweep_open(c, g, run, fn_name, seed, flags, s, d_D, d_I, c->lpa_cap_opt, bytes, &run.more[0], &table_bytes, &cs));

    // ---- the sweeps ----
    hipLaunchKernelGGL(k_fill_u32<true>, dim3(lzx_vertex_grid(n)), dim3(LZX_COM_BLOCK), 0, st, d_label, n, 0u);
    LZX_HIP(hipGetLastError());
    // the three decide launches of a class: its rows cls[first .. first + rows) of one path
    auto group = [&](u32 first, u32 rows) {
        lzx_with_lanes<32>(cs.G, [&](auto lanes) { hipLaunchKernelGGL(k_lpa_group<lanes>, dim3(lzx_row_grid(rows, LZX_COM_BLOCK / lanes)), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, d_label, cs.cls, first, rows, s.counters); });
    };
    auto table = [&](u32 first, u32 rows) { hipLaunchKernelGGL(k_lpa_table, dim3(rows), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, g.col_idx, d_label, cs.cls, first, s.counters); };
    auto far_pick = [&](u32 first, u32 rows) { hipLaunchKernelGGL(k_lpa_far_pick, dim3(rows), dim3(LZX_COM_BLOCK), 0, st, g.row_ptr, d_label, cs.cls, first, cs.lpos, cs.loff, cs.tables, s.counters); };
    u32 sweeps = 0;
    u64 updates = 0;
    bool converged = false;
    LZX_HIP(hipEventRecord(run.ev0, st));
    while (sweeps < max_sweeps && !converged) {
        ++sweeps;
        LZX_HIP(hipMemsetAsync(s.counters + CW_CHANGED, 0, sizeof(u32), st));
        LZX_TRY(lzx_class_pass(c, g, cs, fn_name, d_label, group, table, far_pick, [](u32) {}));
        u32 changed = 0;
        LZX_HIP(hipMemcpyAsync(&changed, s.counters + CW_CHANGED, sizeof(u32), hipMemcpyDeviceToHost, st));
        LZX_HIP(hipStreamSynchronize(st));
        updates += changed;
        converged = changed == 0;
    }
    LZX_HIP(hipEventRecord(run.ev1, st));

    LzxCommResult res;
    LZX_TRY(lzx_comm_finish(c, g, d_label, s, d_D, d_I, labels, &res));
    float sweep_ms = 0.f;
    LZX_HIP(hipEventElapsedTime(&sweep_ms, run.ev0, run.ev1));
    if (info) {
        res.fill(info);
        info->updates = updates;
        info->sweeps = sweeps;
        info->colors = cs.col.colours;
        info->color_rounds = cs.col.rounds;
        info->color_ms = cs.col.ms;
        info->sweep_ms = sweep_ms;
        info->loop_ms = lzx_ms_since(t0);
    }
    if (!converged)
        LZX_FAIL(LZX_ERR_LIMIT, "%s: sweep %u of at most %u still changed a label (labels and info hold the state after it)", fn_name, sweeps, max_sweeps);
    return LZX_OK;
}

extern "C" int lzx_modularity(lzx_handle c, const uint32_t *labels, double *q, lzx_modularity_info *info)
{
    const char *fn_name = "lzx_modularity";
    LZX_TRY(lzx_graph_call_check(c, fn_name, "a partition is scored"));
    if (!labels || !q) LZX_FAIL(LZX_ERR_ARG, "%s: null %s", fn_name, !labels ? "labels" : "q");
    const auto t0 = std::chrono::steady_clock::now();
    const u32 n = (u32)c->n;
    const LzxGraphView g = lzx_view_of(c);
    std::vector<bool> occurs(n, false);
    u64 communities = 0;
    for (u32 i = 0; i < n; ++i) {
        if (labels[i] >= n) LZX_FAIL(LZX_ERR_ARG, "%s: labels[%u] = %u is not below the %u vertices", fn_name, i, labels[i], n);
        if (!occurs[labels[i]]) {
            occurs[labels[i]] = true;
            ++communities;
        }
    }
    hipStream_t st = c->stream;

    LZX_HIP(hipSetDevice(c->device));
    ull *d_D, *d_I;
    u32 *d_label, *d_d, *d_inner, *d_counters;
    LzxGraphRun run(c);
    char what[96];
    std::snprintf(what, sizeof what, "the state of %u vertices (labels, degrees, inner entries, the sums)", n);
    LZX_TRY(lzx_carve_state(fn_name, what, -1, 0, &run.arena, nullptr, [&](LzxCarver &k) {
        k.take(d_D, n);
        k.take(d_I, n);
        for (u32 **p : {&d_label, &d_d, &d_inner}) k.take(*p, lzx_even(n));
        k.take(d_counters, CW_WORDS);
    }));
    LZX_HIP(hipMemcpyAsync(d_label, labels, sizeof(u32) * n, hipMemcpyHostToDevice, st));
    LZX_TRY(lzx_color_degrees(c, g, d_d, nullptr, d_counters));
    std::vector<u64> hD, hI;
    LzxModResult mod;
    LZX_TRY(lzx_modularity_core(c, g, d_label, d_d, d_inner, d_D, d_I, hD, hI, &mod));
    *q = mod.q;
    if (info) {
        info->communities = communities;
        info->inner_entries = mod.inner;
        info->entries = mod.entries;
        info->sum_degree_sq = mod.sum_sq;
        info->loop_ms = lzx_ms_since(t0);
    }
    return LZX_OK;
}
