// lzx_class_sweep.h -- the sweep over the colour classes that lzx_label_propagation (lzx_communities.hip) and lzx_louvain
// (lzx_louvain.hip) share, on top of lzx_communities_shared.h: the wave insert and the far-insert kernel of the label tables, the
// row split and the host state of a sweep, one pass over the classes, and the result both calls end with.  Each of the two keeps
// its own decide kernels (the groups of lanes, the LDS table, the pick over a far table): DESIGN.md sections 21 and 25.
#pragma once

#include "lzx_communities_shared.h"

// f(std::bool_constant<weighted>{}): the launch of a kernel template over "a weight array is read"
template <typename F>
void lzx_with_weights(bool weighted, F f)
{
    if (weighted) f(std::true_type{});
    else f(std::false_type{});
}

// ---- the tables ---------------------------------------------------------------------------------------------------------------
// The labels of a wavefront's lanes (have: this lane holds one, of weight w where W) into the table.  The lanes that agree with the
// first lane's label, and then with the first of the rest, are inserted as one -- late in a run most neighbours of a hub carry one
// label, and a hundred thousand atomics on one address are to be avoided; what is left inserts for itself.  Every lane of the
// wavefront must call it together.
template <bool W>
__device__ __forceinline__ void lzx_insert_wave(bool have, u32 mine, u32 w, u32 *keys, u32 *sums, u32 slots)
{
    const u32 lane = threadIdx.x & 63;
    ull todo = __ballot(have);
    for (int it = 0; it < 2 && todo; ++it) {   // (the same trips for every lane)
        const int leader = __builtin_ctzll(todo);
        const u32 k0 = (u32)__shfl((int)mine, leader, 64);
        const bool agree = have && mine == k0;
        const ull same = __ballot(agree);
        u32 sum = (u32)__builtin_popcountll(same);
        if constexpr (W) sum = lzx_wave_sum_u32(agree ? w : 0u);
        if (lane == (u32)leader) lpa_insert(keys, sums, slots, k0, sum);
        if (agree) have = false;
        todo &= ~same;
    }
    if (have) lpa_insert(keys, sums, slots, mine, W ? w : 1u);
}

// The rows cls[sbeg .. sbeg + gridDim.x) of more than table_above entries: the table of row v lies at tables + 2 loff[lpos[v]] in
// global memory, all zeros between the launches.  Workgroup (row, slice) inserts every gridDim.y-th run of 256 entries of the row;
// the caller's pick kernel follows, in which the workgroup that owns the table reads its slots and clears them.
template <bool W>
static __global__ void __launch_bounds__(LZX_COM_BLOCK)
k_class_far_insert(const u64 *row_ptr, const u32 *col_idx, const u32 *weights, const u32 *label, const u32 *cls, u32 sbeg, const u32 *lpos, const u64 *loff, u32 *tables)
{
    const u32 v = cls[sbeg + blockIdx.x];
    const u64 beg = row_ptr[v], end = row_ptr[v + 1];
    const u32 slots = lpa_slots(end - beg, 1u << 31);
    u32 *keys = tables + 2 * loff[lpos[v]], *sums = keys + slots;
    for (u64 e0 = beg + (u64)blockIdx.y * LZX_COM_BLOCK; e0 < end; e0 += (u64)gridDim.y * LZX_COM_BLOCK) {   // (the same trips for every lane)
        const u64 e = e0 + threadIdx.x;
        const u32 u = e < end ? col_idx[e] : v;
        lzx_insert_wave<W>(u != v, u != v ? label[u] : 0u, (W && u != v) ? weights[e] : 1u, keys, sums, slots);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// The sweep's state on the host: the split of the rows over the three paths, the classes, the far tables.
struct LzxClassSweep {
    // rows of at most group_row entries vote in a group of lanes, of at most table_row over the LDS table, and the rows above
    // table_above over a table in global memory
    u32 group_row = 0, table_row = 0, table_above = 0;
    u32 G = 4, slices = 1;        // lanes per row; workgroups that share a long row's entries
    LzxColorResult col;           // the colouring; col.run: the (colour, path) runs of cls
    const u32 *cls = nullptr, *lpos = nullptr;   // the sorted classes; a long row's place in the list of the long rows
    const u64 *loff = nullptr;                   // the offset of its table, in slots
    u32 *tables = nullptr;

    // the split: the rule, or the test shapes lpa_group_row / lpa_table_row in its place
    explicit LzxClassSweep(const lzx_ctx *c)
    {
        group_row = c->lpa_group_opt > 0 ? (u32)std::min<int64_t>(c->lpa_group_opt, LZX_LPA_MAX_ROW) : LZX_LPA_STAGE;
        table_row = LZX_LPA_SLOTS / 2;   // the LDS table is never more than half full
        if (c->lpa_table_opt > 0 && c->lpa_table_opt < table_row) table_row = (u32)c->lpa_table_opt;
        table_above = std::max(group_row, table_row);   // (a test shape may send longer rows to the groups of lanes)
    }
};

// The colouring of g and its sorted classes (cs->col, cs->cls = s.queue), the lanes per row, and for the rows above table_above
// their places (in s.wait, which the colouring is done with), the offsets of their tables (in d_D; the lengths in d_I) and the
// zeroed tables in *tables: the bytes the call holds (`held`) and the tables count towards cap.  `held` stays the caller's: the
// tables are given back before the call asks for anything else, so it is not raised by them here.
inline int lzx_class_sweep_open(lzx_ctx *c, const LzxGraphView &g, LzxGraphRun &run, const char *fn_name, u64 seed, u32 flags, const LzxColorState &s, ull *d_D, ull *d_I, int64_t cap, u64 held, void **tables, u64 *table_bytes, LzxClassSweep *cs)
{
    LZX_TRY(lzx_color_core(c, g, run, fn_name, seed, flags, s, true, cs->group_row, cs->table_row, &cs->col));
    cs->cls = s.queue;
    cs->G = lzx_lanes_of(c, g);
    cs->slices = (u32)std::min<u64>(std::max<u64>(g.max_row / (8 * LZX_COM_BLOCK), 1), 64);
    cs->lpos = s.wait;
    cs->loff = reinterpret_cast<const u64 *>(d_D);
    if (g.max_row > cs->table_above)
        LZX_TRY(lzx_lpa_far_tables(c, g, fn_name, cs->table_above, cap, held, s.wait, reinterpret_cast<u32 *>(d_I), reinterpret_cast<u64 *>(d_D), s.counters, tables, table_bytes));
    cs->tables = static_cast<u32 *>(*tables);
    return LZX_OK;
}

// One pass over the colour classes in ascending colour.  Per class: group(first, rows) launches the caller's kernel over the groups
// of lanes, table(first, rows) the one over the LDS tables, and for the rows above table_above the far insert runs on `label` and
// far_pick(first, rows) launches the caller's pick; then after(rows of the class) -- what must happen before the next class decides.
template <typename Group, typename Table, typename FarPick, typename After>
int lzx_class_pass(lzx_ctx *c, const LzxGraphView &g, const LzxClassSweep &cs, const char *fn_name, const u32 *label, Group group, Table table, FarPick far_pick, After after)
{
    for (u32 k = 0; k < cs.col.colours; ++k) {
        const u32 *r = cs.col.run.data() + 3 * (size_t)k;
        if (r[1] > r[0]) group(r[0], r[1] - r[0]);
        if (r[2] > r[1]) table(r[1], r[2] - r[1]);
        if (r[3] > r[2]) {
            if (!cs.tables) LZX_FAIL(LZX_ERR_LIMIT, "%s: a row above %u entries without a table", fn_name, cs.table_above);
            lzx_with_weights(g.weights != nullptr, [&](auto w) {
                hipLaunchKernelGGL(k_class_far_insert<w>, dim3(r[3] - r[2], cs.slices), dim3(LZX_COM_BLOCK), 0, c->stream, g.row_ptr, g.col_idx, g.weights, label, cs.cls, r[2], cs.lpos, cs.loff, cs.tables);
            });
            far_pick(r[2], r[3] - r[2]);
        }
        after(r[3] - r[0]);
        LZX_HIP(hipGetLastError());
    }
    return LZX_OK;
}

// What both calls end with: the canonical labels of d_label (into s.wait; first: s.queue, sizes: s.colour -- the colouring is done
// with them), the communities and the largest, the modularity on g's pattern (s.d = g's degrees, the counter words' statistics 0),
// and the labels on the host where `labels` is given.
struct LzxCommResult {
    u64 n_communities = 0, largest_size = 0;
    u32 largest_label = 0;
    LzxModResult mod;
    // the fields that lzx_communities_info and lzx_louvain_info share
    template <typename Info>
    void fill(Info *info) const
    {
        info->n_communities = n_communities;
        info->largest_size = largest_size;
        info->largest_label = largest_label;
        info->inner_entries = mod.inner;
        info->entries = mod.entries;
        info->sum_degree_sq = mod.sum_sq;
        info->modularity = mod.q;
    }
};
inline int lzx_comm_finish(lzx_ctx *c, const LzxGraphView &g, const u32 *d_label, const LzxColorState &s, ull *d_D, ull *d_I, u32 *labels, LzxCommResult *res)
{
    hipStream_t st = c->stream;
    u32 *d_out = s.wait;
    LZX_TRY(lzx_comm_canonical(c, d_label, g.n, s.queue, d_out, s.colour, s.counters));
    u32 words[CW_WORDS];
    LZX_HIP(hipMemcpyAsync(words, s.counters, sizeof(words), hipMemcpyDeviceToHost, st));
    std::vector<u64> hD, hI;
    LZX_TRY(lzx_modularity_core(c, g, d_out, s.d, s.queue, d_D, d_I, hD, hI, &res->mod));
    if (labels) LZX_HIP(hipMemcpyAsync(labels, d_out, sizeof(u32) * g.n, hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    const u64 key = (u64)words[CW_KEY] | ((u64)words[CW_KEY + 1] << 32);
    res->n_communities = words[CW_COMMUNITIES];
    res->largest_size = key >> 32;
    res->largest_label = LZX_COM_NONE - (u32)(key & 0xffffffffull);
    return LZX_OK;
}
