// lzx_communities_shared.h -- what lzx_color / lzx_label_propagation / lzx_modularity (lzx_communities.hip) share with lzx_louvain
// (lzx_louvain.hip): a view of a graph other than the handle's, so that the colouring, the class sort and the counting passes run
// on a level graph of the aggregation as they run on the caller-order CSR; the state and the results of the colouring and the
// modularity; the open-addressing label table; and the host entry points of lzx_communities.hip that lzx_louvain.hip calls.
#pragma once

#include <vector>

#include "lzx_internal.h"
#include "lzx_graph_call.h"
#include "lzx_spmv_body.h"
#include "lzx_reduce.h"

static constexpr u32 LZX_COM_BLOCK = 256;
static constexpr u32 LZX_COM_NONE = 0xffffffffu;
static constexpr u32 LZX_COLOR_CAP = 1u << 16;    // colours are below this: the LDS bitmap's bits, the histogram's classes
static constexpr u32 LZX_LPA_STAGE = 128;         // labels a group of lanes stages in LDS
static constexpr u32 LZX_LPA_SLOTS = 4096;        // slots of the LDS table
static constexpr u32 LZX_LPA_MAX_ROW = 1u << 30;  // a longer row's table would have more than 2^31 slots
// the counter words
enum { CW_END = 0, CW_COLORS = 1, CW_CHANGED = 2, CW_LONG = 3, CW_COMMUNITIES = 4, CW_KEY = 8, CW_WORDS = 16 };


struct ColorOrder {
    const u32 *d;
    u64 seed;
    u32 by_id;
    __device__ __forceinline__ u64 hash(u32 v) const
    {
        u64 h = seed + 0x9E3779B97F4A7C15ull * ((u64)v + 1);
        h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 27; h *= 0x94D049BB133111EBull; h ^= h >> 31;
        return h;
    }
    // u comes before v
    __device__ __forceinline__ bool before(u32 u, u32 v) const
    {
        const u32 du = d[u], dv = d[v];
        if (du != dv) return du > dv;
        if (!by_id) {
            const u64 hu = hash(u), hv = hash(v);
            if (hu != hv) return hu < hv;
        }
        return u < v;
    }
};

// The calling lanes for which `active` holds add one to bins[key] each, the lanes of one key with one atomic.  Every lane of the
// wavefront must call it together.  Returns the lane's place in its bin: the count before the wavefront plus its rank among the
// wavefront's lanes of the same key (meaningless where !active).
__device__ __forceinline__ u32 wave_bucket_add(bool active, u32 key, u32 *bins)
{
    const u32 lane = threadIdx.x & 63;
    u32 place = 0;
    ull todo = __ballot(active);
    while (todo) {   // (the same trips for every lane; at most 64)
        const int leader = __builtin_ctzll(todo);
        const u32 k0 = (u32)__shfl((int)key, leader, 64);
        const bool mine = active && key == k0;
        const ull same = __ballot(mine);
        u32 base = 0;
        if (lane == (u32)leader) base = atomicAdd(&bins[k0], (u32)__builtin_popcountll(same));
        base = (u32)__shfl((int)base, leader, 64);
        if (mine) place = base + (u32)__builtin_popcountll(same & ((1ull << lane) - 1ull));
        todo &= ~same;
    }
    return place;
}


// An open-addressing table of `slots` (a power of two) keys and counts.  A key is the label + 1 and 0 an empty slot, so that a
// cleared table is all zeros.  One neighbour's label: atomicCAS on the key slot, atomicAdd on the count, linear probing bounded by
// the slot count (the table is never more than half full).
__device__ __forceinline__ void lpa_insert(u32 *keys, u32 *counts, u32 slots, u32 mine, u32 times)
{
    const u32 x = mine * 0x9E3779B1u;
    u32 h = (x ^ (x >> 16)) & (slots - 1);
    for (u32 probe = 0; probe < slots; ++probe) {
        const u32 prev = atomicCAS(&keys[h], 0u, mine + 1);
        if (prev == 0u || prev == mine + 1) {
            atomicAdd(&counts[h], times);
            break;
        }
        h = (h + 1) & (slots - 1);
    }
}


// x[i] = i (IOTA) or value, i < n.  (static, like every kernel of a header two files include: each file launches the copy in its
// own code object, so the file a call's first launch loads does not depend on the link order)
template <bool IOTA>
static __global__ void __launch_bounds__(LZX_COM_BLOCK)
k_fill_u32(u32 *x, u32 n, u32 value)
{
    const u64 i = (u64)blockIdx.x * LZX_COM_BLOCK + threadIdx.x;
    if (i < n) x[i] = IOTA ? (u32)i : value;
}

// pow2ceil(2 len), at least 2 and at most cap
__device__ __forceinline__ u32 lpa_slots(u64 len, u32 cap)
{
    u32 slots = 2;
    while (slots < 2 * len && slots < cap) slots *= 2;
    return slots;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// A graph as the colouring and the counting passes read it: the handle's caller-order CSR (weights == nullptr: every off-diagonal
// entry weighs 1), or a level graph of lzx_louvain with a u32 weight per entry.  Rows ascend by column.
struct LzxGraphView {
    const u64 *row_ptr;
    const u32 *col_idx;
    const u32 *weights;
    u32 n;
    u64 entries;       // stored entries
    u64 max_row;       // entries of the longest row
    u64 rows_active;   // rows that have an entry
};
inline LzxGraphView lzx_view_of(const lzx_ctx *c) { return LzxGraphView{c->d_row_ptr, c->d_col_idx, nullptr, (u32)c->n, c->nnz, c->max_degree, c->n_active}; }

struct LzxColorState {
    u32 *d, *wait, *colour, *queue, *bins, *counters;
};
struct LzxColorResult {
    u32 colours = 0, rounds = 0, largest_class = 0;
    float ms = 0.f;
    std::vector<u32> run;   // 3 colours + 1: where the (colour, path) runs of the sorted classes begin
};
struct LzxModResult {
    double q = 0.0;
    u64 inner = 0, entries = 0, sum_sq = 0;
};

inline u64 lzx_class_bins(u32 n) { return lzx_even(3 * (u64)std::min<u32>(n, LZX_COLOR_CAP)); }
inline u32 lzx_vertex_grid(u32 n) { return (n + LZX_COM_BLOCK - 1) / LZX_COM_BLOCK; }
inline u32 lzx_lanes_of(lzx_ctx *c, const LzxGraphView &g) { return lzx_lanes_per_row_of(c, g.entries, g.rows_active, 32); }

// (lzx_communities.hip)
// s.d = the degrees without the diagonal of g's rows (colour = none where s.colour is given), the counter words 0
int lzx_color_degrees(lzx_ctx *c, const LzxGraphView &g, u32 *d, u32 *colour, u32 *counters);
// The colouring of g into s.colour and, with `sorted`, the classes into s.queue, one run per (colour, path).  run.ev0 / ev1 exist.
int lzx_color_core(lzx_ctx *c, const LzxGraphView &g, LzxGraphRun &run, const char *fn_name, u64 seed, u32 flags, const LzxColorState &s, bool sorted,
                   u32 group_row, u32 table_row, LzxColorResult *res);
// The rows of g above table_above entries: their places in d_lpos (u32 [n]), their lengths in d_llen (u32 [n]), the offsets of their
// tables in d_loff (u64 [n], in slots) and the zeroed tables in *tables, 2 u32 per slot, pow2ceil(2 len) slots per row (nullptr: no
// such row).  `held`: the bytes the call holds already; the tables count towards cap on top of them.  counters[CW_LONG] is 0.
int lzx_lpa_far_tables(lzx_ctx *c, const LzxGraphView &g, const char *fn_name, u32 table_above, int64_t cap, u64 held, u32 *d_lpos, u32 *d_llen,
                       u64 *d_loff, u32 *counters, void **tables, u64 *table_bytes);
// d_out[v] = the smallest v' with d_label[v'] == d_label[v] (labels < n), d_sizes[that] = the members; counters[CW_COMMUNITIES] and
// the key at counters[CW_KEY] (0 before the call) = the communities and the largest.  d_first: scratch, u32 [n].
int lzx_comm_canonical(lzx_ctx *c, const u32 *d_label, u32 n, u32 *d_first, u32 *d_out, u32 *d_sizes, u32 *counters);
// The modularity of the labels in d_label (device, values < g.n) on g's pattern: d_d = the degrees, d_inner = scratch, u32 [n] each;
// D, I: u64 [n].  hD, hI: the accumulators on the host.
int lzx_modularity_core(lzx_ctx *c, const LzxGraphView &g, const u32 *d_label, const u32 *d_d, u32 *d_inner, ull *d_D, ull *d_I, std::vector<u64> &hD,
                        std::vector<u64> &hI, LzxModResult *res);
