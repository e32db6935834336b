// lzx_tri_orient.h -- the degree-oriented copy of the caller-order CSR that lzx_triangles (lzx_triangles.hip) and lzx_truss
// (lzx_truss.hip) both build: DESIGN.md section 18.  d_v = the entries of row v without the diagonal.  Vertices are ranked by
// (d_v, v) and every edge that is not a self loop is kept once, in the row of its lower-ranked end (64-bit row pointers, u32
// columns, ascending by id).  The position of an edge in the oriented columns is lzx_truss's edge id.
//   degrees    k_tri_degrees           one thread per row: lzx_degree_no_diagonal (lzx_graph_call.h)
//   out-counts k_tri_orient (count)    a group of G lanes per row counts the neighbours of higher rank; the caller's exclusive
//                                      scan turns the counts into the row pointers, in place
//   fill       k_tri_orient (fill)     the same walk writes them: a ballot over the group orders the kept entries
// Each kernel is compiled into the file that includes this header (k_tri_degrees has internal linkage for that).
#pragma once

#include "lzx_internal.h"
#include "lzx_graph_call.h"

static constexpr u32 LZX_TRI_BLOCK = 256;
static constexpr u32 LZX_TRI_LONG = 128;         // out-entries beyond which a row goes to the wide counting kernel (test shape tri_long_list)
static constexpr u32 LZX_TRI_STAGE = 4096;       // entries of N+(a) staged in LDS by the wide counting kernel (at most)
static constexpr u32 LZX_TRI_SLICES = 64;        // workgroups a long row's out-edges are dealt to (at most)

static __global__ void __launch_bounds__(LZX_TRI_BLOCK) k_tri_degrees(const u64 *row_ptr, const u32 *col_idx, u32 *deg, u32 n)
{
    const u64 v = (u64)blockIdx.x * LZX_TRI_BLOCK + threadIdx.x;
    if (v < n) deg[v] = lzx_degree_no_diagonal(row_ptr, col_idx, v);
}

// G lanes per row.  fill == nullptr: count[row] = the neighbours of higher rank (and count[n] = 0, kmax = the largest count);
// otherwise they are written in their order behind row_ptr_out[row].
template <u32 G>
__global__ void __launch_bounds__(LZX_TRI_BLOCK)
k_tri_orient(const u64 *row_ptr, const u32 *col_idx, const u32 *deg, u32 n, u64 *count, const u64 *row_ptr_out, u32 *fill, u32 *kmax)
{
    constexpr ull group_mask = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
    const u32 sub = threadIdx.x & (G - 1);
    const u32 shift = (threadIdx.x & 63) & ~(G - 1);
    const u64 row = (u64)blockIdx.x * (LZX_TRI_BLOCK / G) + threadIdx.x / G;
    u64 beg = 0, end = 0, out0 = 0;
    u32 dv = 0;
    if (row < n) {
        beg = row_ptr[row];
        end = row_ptr[row + 1];
        dv = deg[row];
        if (fill) out0 = row_ptr_out[row];
    }
    u32 kept = 0;
    for (u64 e0 = beg; e0 < end; e0 += G) {   // (the same trips for every lane of the group)
        const u64 e = e0 + sub;
        bool k = false;
        u32 col = 0;
        if (e < end) {
            col = col_idx[e];
            if (col != (u32)row) {
                const u32 du = deg[col];
                k = du > dv || (du == dv && col > (u32)row);
            }
        }
        const ull m = (__ballot(k) >> shift) & group_mask;
        if (fill && k) fill[out0 + kept + __builtin_popcountll(m & ((1ull << sub) - 1ull))] = col;
        kept += (u32)__builtin_popcountll(m);
    }
    if (fill) return;
    if (sub == 0 && row < n) count[row] = kept;
    if (row == 0 && sub == 0) count[n] = 0;
    u32 mx = kept;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (u32)__shfl_xor((int)mx, o, 64));
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(kmax, mx);
}

static inline void orient_pass(u32 G, hipStream_t st, const lzx_ctx *c, const u32 *deg, u64 *count, const u64 *orp, u32 *fill, u32 *kmax)
{
    lzx_with_lanes<64>(G, [&](auto g) {
        hipLaunchKernelGGL(k_tri_orient<g>, dim3(lzx_row_grid(c->n, LZX_TRI_BLOCK / g)), dim3(LZX_TRI_BLOCK), 0, st, c->d_row_ptr, c->d_col_idx, deg,
                           (u32)c->n, count, orp, fill, kmax);
    });
}
