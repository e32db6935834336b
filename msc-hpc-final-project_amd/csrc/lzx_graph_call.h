// lzx_graph_call.h -- what the graph routines on the caller-order CSR (d_row_ptr / d_col_idx) share: lzx_components,
// lzx_bfs_multi / lzx_betweenness_f64 (lzx_paths.hip), lzx_triangles, lzx_core_numbers, lzx_truss and lzx_color /
// lzx_label_propagation / lzx_modularity (lzx_communities.hip), lzx_louvain (lzx_louvain.hip), lzx_sweep_cut (lzx_sweep.hip) and lzx_similarity (lzx_similarity.hip).  Host side: the preconditions of such
// a call, what it holds on the device, the capped allocation of its state (also the CG entry points' and the eigensolver's),
// the choice of lanes per row, a test shape in a rule's place.  Device side: the idioms of their kernels over ascending rows and
// wavefront-aggregated queues.  What only some of them share has a header of its own on top of this one: the oriented copy and
// the split of the walks over it (lzx_tri_orient.h: lzx_triangles, lzx_truss), the push peel (lzx_peel.h: lzx_core_numbers, lzx_truss), the
// graph view, the colouring and the modularity (lzx_communities_shared.h: lzx_communities.hip, lzx_louvain.hip) and, on top of that, the
// sweep over the colour classes (lzx_class_sweep.h: lzx_label_propagation, lzx_louvain).
#pragma once

#include <algorithm>
#include <type_traits>

#include "lzx_internal.h"
#include "lzx_carve.h"

// one GPU, a graph, all of it on this handle; `what`: "<what the call does> on one GPU handle".  A call that passes starts with
// no lanes per row on record (lzx_lanes_per_row)
inline int lzx_graph_call_check(lzx_ctx *c, const char *fn, const char *what)
{
    if (!c) LZX_FAIL(LZX_ERR_ARG, "%s: null handle", fn);
    if (c->comm_kind != 0 || c->world > 1)
        LZX_FAIL(LZX_ERR_STATE, "%s: %s on one GPU handle; this handle is rank %d of a communicator of %d", fn, what, c->rank, c->world);
    if (!c->d_row_ptr) LZX_FAIL(LZX_ERR_STATE, "%s: no graph has been handed over", fn);
    if (c->sharded) LZX_FAIL(LZX_ERR_STATE, "%s: the graph came through the sharded hand-over -- no rank holds all of it", fn);
    c->lanes_rows_ran = c->lanes_oriented_ran = 0;
    return LZX_OK;
}

// everything a graph call allocates: its end waits for the stream and gives it back, on every return path
struct LzxGraphRun {
    lzx_ctx *c;
    void *arena = nullptr, *more[2] = {nullptr, nullptr};
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    explicit LzxGraphRun(lzx_ctx *c_) : c(c_) {}
    // ev0 .. ev(k - 1), k <= 4
    int events(u32 k)
    {
        hipEvent_t *ev[4] = {&ev0, &ev1, &ev2, &ev3};
        if (k > 4) LZX_FAIL(LZX_ERR_ARG, "LzxGraphRun::events: %u events asked for, a run holds 4", k);
        for (u32 i = 0; i < k; ++i) LZX_HIP(hipEventCreate(ev[i]));
        return LZX_OK;
    }
    ~LzxGraphRun()
    {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        for (void *p : {arena, more[0], more[1]})
            if (p) (void)hipFree(p);
        for (hipEvent_t e : {ev0, ev1, ev2, ev3})
            if (e) (void)hipEventDestroy(e);
    }
    LzxGraphRun(const LzxGraphRun &) = delete;
    LzxGraphRun &operator=(const LzxGraphRun &) = delete;
};

// *out = alloc_bytes of device memory for a state of state_bytes (`what` names it), or the error: a state above cap (a test
// shape *_state_bytes; < 0: none) counts as out of device memory (lzx_solve.hip)
int lzx_alloc_state(const char *fn, const char *what, int64_t cap, u64 state_bytes, u64 alloc_bytes, void **out);

// One arena through the carver (lzx_carve.h).  layout(LzxCarver &) is the list of the arena's pieces: it is counted over a null
// base, allocated into *slot by lzx_alloc_state -- the state is `held`, the bytes the call holds already, plus the list's state
// bytes; the allocation is everything the list takes -- and carved from the allocation.  *bytes (where given): the list's state
// bytes.  A list whose two passes disagree, or that puts a piece off its type's alignment, fails here, before any kernel is
// launched on it; *slot is the caller's to free, as after any other failure.
template <typename Layout>
int lzx_carve_state(const char *fn, const char *what, int64_t cap, u64 held, void **slot, u64 *bytes, Layout layout)
{
    LzxCarver counted;
    layout(counted);
    LZX_TRY(lzx_alloc_state(fn, what, cap, held + counted.state_bytes(), counted.at, slot));
    LzxCarver carved(*slot);
    layout(carved);
    if (!carved.agrees_with(counted))
        LZX_FAIL(LZX_ERR_LIMIT, "%s: the layout of %s counts %llu bytes and carves %llu%s", fn, what, (ull)counted.at, (ull)carved.at,
                 carved.misaligned || counted.misaligned ? ", with a piece off its alignment" : "");
    if (bytes) *bytes = counted.state_bytes();
    return LZX_OK;
}

// what a launch over G lanes per row walks: the caller-order rows, or the rows of the oriented copy (lzx_tri_orient.h)
enum LzxLanesOver { LZX_OVER_ROWS, LZX_OVER_ORIENTED };

// lanes per row of a graph call's launches over `entries` entries in the rows that have an edge: about half the mean row length,
// so that a typical row is two loads per lane; 4 .. max_g, the widest instantiation of the kernels it is for.  The test shape
// graph_lanes takes the rule's place (capped at max_g as well).  What it returns goes on record for lzx_test_get_shape
// (graph_lanes_rows / graph_lanes_oriented): the widest of a call where its launches differ -- lzx_truss peels over
// min(that, 32) lanes per edge.
// (rows_of: the same rule for a graph other than the handle's, of `rows` rows that have an entry -- a level graph of lzx_louvain)
inline u32 lzx_lanes_per_row_of(lzx_ctx *c, u64 entries, u64 rows, u32 max_g, LzxLanesOver over = LZX_OVER_ROWS)
{
    const u64 mean = entries / std::max<u64>(rows, 1);
    u32 G = 4;
    while (G < max_g && 2 * G <= mean) G *= 2;
    if (c->graph_lanes_opt > 0) G = (u32)std::min<int64_t>(c->graph_lanes_opt, max_g);
    u32 &ran = over == LZX_OVER_ORIENTED ? c->lanes_oriented_ran : c->lanes_rows_ran;
    ran = std::max(ran, G);
    return G;
}
inline u32 lzx_lanes_per_row(lzx_ctx *c, u64 entries, u32 max_g, LzxLanesOver over = LZX_OVER_ROWS)
{
    return lzx_lanes_per_row_of(c, entries, c->n_active, max_g, over);
}

// f(std::integral_constant<u32, G>{}) for G = 4, 8, ... MAX_G (32 or 64; anything else counts as MAX_G): the launch of a
// kernel template over the lanes per row.  Only the widths up to MAX_G are instantiated.
template <u32 MAX_G, typename F>
void lzx_with_lanes(u32 G, F f)
{
    if (G == 4) f(std::integral_constant<u32, 4>{});
    else if (G == 8) f(std::integral_constant<u32, 8>{});
    else if (G == 16) f(std::integral_constant<u32, 16>{});
    else if (G == 32 || MAX_G == 32) f(std::integral_constant<u32, 32>{});
    else if constexpr (MAX_G == 64) f(std::integral_constant<u32, 64>{});
}
// a test shape that takes a rule's place: opt where it is set (> 0, capped at what a u32 holds), else dflt
inline u32 lzx_shape_or(int64_t opt, u32 dflt) { return opt > 0 ? (u32)std::min<int64_t>(opt, 0xffffffff) : dflt; }
// workgroups that take rows_per_block rows each
inline u32 lzx_row_grid(u64 rows, u32 rows_per_block) { return (u32)((rows + rows_per_block - 1) / rows_per_block); }

// ---- device ----
// first position in the ascending list[0 .. len) whose entry is >= x
__device__ __forceinline__ u32 lzx_lower_bound(const u32 *list, u32 len, u32 x)
{
    u32 lo = 0, hi = len;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (list[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// d_v: the entries of row v without the diagonal -- the row's length, minus one if a binary search finds v in it
__device__ __forceinline__ u32 lzx_degree_no_diagonal(const u64 *row_ptr, const u32 *col_idx, u64 v)
{
    const u64 beg = row_ptr[v];
    const u32 len = (u32)(row_ptr[v + 1] - beg);
    const u32 at = lzx_lower_bound(col_idx + beg, len, (u32)v);
    return len - ((at < len && col_idx[beg + at] == (u32)v) ? 1u : 0u);
}

// a row's count summed over the G lanes that share the row (every lane gets the sum), and over the wavefront
template <u32 G>
__device__ __forceinline__ u32 lzx_group_sum_u32(u32 v)
{
#pragma unroll
    for (u32 o = G / 2; o > 0; o >>= 1) v += (u32)__shfl_xor((int)v, (int)o, 64);
    return v;
}
__device__ __forceinline__ u32 lzx_wave_sum_u32(u32 v) { return lzx_group_sum_u32<64>(v); }

// the calling lanes for which `take` holds get consecutive places behind *tail: one atomic per wavefront.  Every lane of the
// wavefront must call it together.  Returns the lane's place (meaningless where !take).
__device__ __forceinline__ u32 lzx_wave_append(bool take, u32 *tail)
{
    const ull m = __ballot(take);
    if (m == 0) return 0;   // (the same for every lane)
    const u32 lane = threadIdx.x & 63;
    const int first = __builtin_ctzll(m);
    u32 base = 0;
    if (lane == (u32)first) base = atomicAdd(tail, (u32)__builtin_popcountll(m));
    base = (u32)__shfl((int)base, first, 64);
    return base + (u32)__builtin_popcountll(m & ((1ull << lane) - 1ull));
}

// the prologue of a long-row kernel: the ids of the threads whose row is long are collected in s_rows (LDS, one place per
// thread of the workgroup, in no particular order) and counted in *s_count (LDS).  Every thread of the workgroup must call it.
// Returns the count.
__device__ __forceinline__ u32 lzx_collect_long_rows(bool mine_is_long, u32 id, u32 *s_rows, u32 *s_count)
{
    if (threadIdx.x == 0) *s_count = 0;
    __syncthreads();
    if (mine_is_long) s_rows[atomicAdd(s_count, 1u)] = id;
    __syncthreads();
    return *s_count;
}
