// lzx_core.hip -- core numbers and onion layers of the handle's graph (networkx.core_number, networkx.onion_layers), on the
// device over the caller-order CSR the handle keeps (d_row_ptr / d_col_idx): include/lzx.h, lzx_core_numbers; DESIGN.md section 19.
//
// Definitions.  d_v = the entries of row v without the diagonal.  Rounds are numbered from 1 and k_0 = 0; round r has
// k_r = max(k_{r-1}, the smallest remaining degree of a remaining vertex) and removes, all at once, every remaining vertex whose
// remaining degree is <= k_r: core[v] = k_r, layer[v] = r.
//
// Push peeling: the loop, the level start and the push of lzx_peel.h, which lzx_truss.hip shares, over vertices.  deg[v] is the
// remaining degree, layer[v] != 0 marks a vertex that is removed or queued for removal, and `order` is one queue in which every
// vertex is placed exactly once over the whole call, so that each round's frontier is a window [beg, end) of it and what a
// launch appends behind `end` is the next window.
//   degrees      k_core_degrees       one thread per row: lzx_degree_no_diagonal (lzx_graph_call.h), and layer = 0, the queue empty
//   level start  k_peel_level         (lzx_peel.h) one thread per vertex, when the frontier is empty: an unmarked vertex with
//                                     deg <= k is marked (layer = r, core = k) and appended, the others contribute to a minimum.
//                                     The host tries k + 1 first -- after a level is peeled out every remaining degree is at least
//                                     that -- and only if nothing was appended repeats the sweep with the minimum it got back.
//   peel         k_core_peel<G>       G lanes per row of the window; for every neighbour u != v that is not marked,
//                                     lzx_peel_push: old = atomicSub(&deg[u], 1), and the one lane that sees old == k + 1 marks u
//                                     (layer = r + 1, core = k) and appends it
//                k_core_peel_long     the window's rows of more than long_row entries: a workgroup per (row, slice of its entries)
// Appends are aggregated per wavefront (lzx_wave_append: a ballot, one atomic add on the queue's end, a broadcast), and so is the
// minimum; the loops around them run the same trips on every lane of a wavefront.
//
// The "not marked" test saves traffic only; no output depends on whether a lane sees a fresh or a stale mark:
//   - decrements only lower a counter.  A vertex is marked when its counter is at most k: at a level start it is <= k, in the
//     peel it has just gone from k + 1 to k.  A later decrement of it therefore returns at most k, never k + 1, while the level
//     lasts, and the counters of marked vertices are never read again once k moves on: a removed vertex is appended once.
//   - on a symmetric matrix deg[u] counts the neighbours of u that have not been peeled yet, each of which decrements it at most
//     once (a vertex is peeled once), so no counter goes below 0.
// A matrix that is not symmetric is not detected and its numbers mean nothing; its counters may wrap.  The call still stays
// inside its memory and ends: the mark is taken by a compare-and-swap, which only the first claimant of a vertex wins (on a
// symmetric matrix the only one), so no vertex is queued twice, the queue's end never passes n -- every append is clamped to the
// n entries all the same -- every window is a fresh piece of the queue, and a level start always finds the vertex of the minimum.
//
// All atomics are 32-bit integer vector atomics; nothing is floating-point.  The order inside a window is not deterministic and
// is no output; core, layer, rounds and levels are.  No kernel waits on another workgroup; every device loop is bounded by a row
// length or a window length.  The host reads one word per peeling round (the queue's end) and two per level start (the end and
// the minimum), as lzx_components reads its flag.
#include <algorithm>
#include <chrono>

#include "lzx_internal.h"
#include "lzx_graph_call.h"
#include "lzx_peel.h"

static constexpr u32 LZX_CORE_BLOCK = 256;

__global__ void __launch_bounds__(LZX_CORE_BLOCK)
k_core_degrees(const u64 *row_ptr, const u32 *col_idx, u32 *deg, u32 *layer, u32 *counters, u32 n)
{
    const u64 v = (u64)blockIdx.x * LZX_CORE_BLOCK + threadIdx.x;
    if (v == 0) counters[0] = 0;   // the queue's end
    if (v >= n) return;
    deg[v] = lzx_degree_no_diagonal(row_ptr, col_idx, v);
    layer[v] = 0;
}

// rows of the window order[wbeg .. wbeg + wlen) with at most long_row entries: G lanes per row, 256 / G rows per workgroup
template <u32 G>
__global__ void __launch_bounds__(LZX_CORE_BLOCK)
k_core_peel(const u64 *row_ptr, const u32 *col_idx, u32 *deg, u32 *layer, u32 *core, u32 *order, u32 *counters, u32 n, u32 wbeg, u32 wlen,
            u32 k, u32 r, u32 long_row)
{
    const u32 sub = threadIdx.x & (G - 1);
    const u64 idx = (u64)blockIdx.x * (LZX_CORE_BLOCK / G) + threadIdx.x / G;
    u64 beg = 0;
    u32 len = 0, v = 0;
    if (idx < wlen) {
        v = order[wbeg + idx];
        beg = row_ptr[v];
        const u64 l = row_ptr[v + 1] - beg;
        len = l > long_row ? 0u : (u32)l;   // k_core_peel_long's
    }
    u32 trips = (len + G - 1) / G;
#pragma unroll
    for (int o = 32; o >= (int)G; o >>= 1) trips = max(trips, (u32)__shfl_xor((int)trips, o, 64));
    for (u32 t = 0; t < trips; ++t) {   // (the same trips for every lane of the wavefront: the appends are formed together)
        const u32 e = t * G + sub;
        u32 u = v;
        if (e < len) u = col_idx[beg + e];
        lzx_peel_push(u != v && layer[u] == 0, u, deg, layer, core, order, &counters[0], n, k, k, r);
    }
}

// rows of more than long_row entries among the workgroup's 256 window places: the workgroup takes every gridDim.y-th run of 256
// entries of each
__global__ void __launch_bounds__(LZX_CORE_BLOCK)
k_core_peel_long(const u64 *row_ptr, const u32 *col_idx, u32 *deg, u32 *layer, u32 *core, u32 *order, u32 *counters, u32 n, u32 wbeg,
                 u32 wlen, u32 k, u32 r, u32 long_row)
{
    __shared__ u32 s_rows[LZX_CORE_BLOCK];
    __shared__ u32 s_count;
    const u64 idx = (u64)blockIdx.x * LZX_CORE_BLOCK + threadIdx.x;
    const u32 mine = idx < wlen ? order[wbeg + idx] : 0u;
    const u32 count = lzx_collect_long_rows(idx < wlen && row_ptr[mine + 1] - row_ptr[mine] > long_row, mine, s_rows, &s_count);
    for (u32 i = 0; i < count; ++i) {
        const u32 v = s_rows[i];
        const u64 beg = row_ptr[v], end = row_ptr[v + 1];
        // (the same trips for every lane of the workgroup)
        for (u64 e0 = beg + (u64)blockIdx.y * LZX_CORE_BLOCK; e0 < end; e0 += (u64)gridDim.y * LZX_CORE_BLOCK) {
            const u64 e = e0 + threadIdx.x;
            u32 u = v;
            if (e < end) u = col_idx[e];
            lzx_peel_push(u != v && layer[u] == 0, u, deg, layer, core, order, &counters[0], n, k, k, r);
        }
    }
}

extern "C" int lzx_core_numbers(lzx_handle c, uint32_t *core, uint32_t *layer, lzx_core_info *info)
{
    const char *fn_name = "lzx_core_numbers";
    LZX_TRY(lzx_graph_call_check(c, fn_name, "core numbers are peeled"));
    const auto t0 = std::chrono::steady_clock::now();
    const u32 n = (u32)c->n;

    LZX_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    u32 *d_deg, *d_layer, *d_core, *d_order, *d_counters;
    LzxGraphRun run(c);
    char what[96];
    std::snprintf(what, sizeof what, "the state of %u vertices (remaining degrees, layers, core numbers, the queue)", n);
    LZX_TRY(lzx_carve_state(fn_name, what, c->core_cap_opt, 0, &run.arena, nullptr, [&](LzxCarver &k) {
        for (u32 **p : {&d_deg, &d_layer, &d_core, &d_order}) k.take(*p, lzx_even(n));
        k.take(d_counters, 2);   // the queue's end and the minimum
    }));
    LZX_TRY(run.events(2));

    // lanes per row of the window: about half the mean degree of the rows that have an edge.  Rows of more than 64 G entries
    // (256 ... 2048: more than 64 trips of a group) go to the long-row launch.
    const u32 G = lzx_lanes_per_row(c, c->nnz, 32);
    const u32 long_row = lzx_shape_or(c->core_long_opt, 64 * G);
    const u32 slices = lzx_peel_slices(c->max_degree, LZX_CORE_BLOCK);
    const u32 gb = (n + LZX_CORE_BLOCK - 1) / LZX_CORE_BLOCK;

    LZX_HIP(hipEventRecord(run.ev0, st));
    hipLaunchKernelGGL(k_core_degrees, dim3(gb), dim3(LZX_CORE_BLOCK), 0, st, c->d_row_ptr, c->d_col_idx, d_deg, d_layer, d_counters, n);
    LZX_HIP(hipGetLastError());
    LzxPeelResult peel;
    LZX_TRY(lzx_peel_loop(
        fn_name, {"vertex", "remaining degree", "vertices"}, st, d_counters, n,
        [&](u32 k_try, u32 r) -> int {
            hipLaunchKernelGGL(k_peel_level, dim3(lzx_row_grid(n, LZX_PEEL_BLOCK)), dim3(LZX_PEEL_BLOCK), 0, st, d_deg, d_layer, d_core, d_order, d_counters,
                               n, k_try, k_try, r);
            LZX_HIP(hipGetLastError());
            return LZX_OK;
        },
        [&](u32 wbeg, u32 wlen, u32 k, u32 r) -> int {
            lzx_with_lanes<32>(G, [&](auto g) {
                hipLaunchKernelGGL(k_core_peel<g>, dim3(lzx_row_grid(wlen, LZX_CORE_BLOCK / g)), dim3(LZX_CORE_BLOCK), 0, st, c->d_row_ptr, c->d_col_idx,
                                   d_deg, d_layer, d_core, d_order, d_counters, n, wbeg, wlen, k, r, long_row);
            });
            LZX_HIP(hipGetLastError());
            if (c->max_degree > long_row) {
                hipLaunchKernelGGL(k_core_peel_long, dim3((wlen + LZX_CORE_BLOCK - 1) / LZX_CORE_BLOCK, slices), dim3(LZX_CORE_BLOCK), 0, st,
                                   c->d_row_ptr, c->d_col_idx, d_deg, d_layer, d_core, d_order, d_counters, n, wbeg, wlen, k, r, long_row);
                LZX_HIP(hipGetLastError());
            }
            return LZX_OK;
        },
        &peel));
    LZX_HIP(hipEventRecord(run.ev1, st));
    if (core) LZX_HIP(hipMemcpyAsync(core, d_core, sizeof(u32) * n, hipMemcpyDeviceToHost, st));
    if (layer) LZX_HIP(hipMemcpyAsync(layer, d_layer, sizeof(u32) * n, hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    float peel_ms = 0.f;
    LZX_HIP(hipEventElapsedTime(&peel_ms, run.ev0, run.ev1));
    if (info) {
        info->main_core_size = (u64)n - peel.level_pos;
        info->core0 = peel.first_level == 0 ? peel.first_end : 0;
        info->degeneracy = peel.level;
        info->levels = peel.levels;
        info->rounds = peel.rounds;
        info->reserved_ = 0;
        info->peel_ms = peel_ms;
        info->loop_ms = lzx_ms_since(t0);
    }
    return LZX_OK;
}
