// lzx_tri_orient.h -- the degree-oriented copy of the caller-order CSR that lzx_triangles (lzx_triangles.hip) and lzx_truss
// (lzx_truss.hip) both build: DESIGN.md section 18.  d_v = the entries of row v without the diagonal.  Vertices are ranked by
// (d_v, v) and every edge that is not a self loop is kept once, in the row of its lower-ranked end (64-bit row pointers, u32
// columns, ascending by id).  The position of an edge in the oriented columns is lzx_truss's edge id.
//   degrees    k_tri_degrees           one thread per row: lzx_degree_no_diagonal (lzx_graph_call.h)
//   out-counts k_tri_orient (count)    a group of G lanes per row counts the neighbours of higher rank; hipcub's exclusive scan
//                                      turns the counts into the row pointers, in place (lzx_orient_count: the host's sequence)
//   fill       k_tri_orient (fill)     the same walk writes them: a ballot over the group orders the kept entries
// and the split of the launches that walk it (lzx_tri_shape).
// Each kernel is compiled into the file that includes this header (k_tri_degrees has internal linkage for that).
#pragma once

#include <hipcub/hipcub.hpp>

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

// The first half of the oriented copy, up to what its columns need: the scan's scratch (run.more[0]), then -- run.ev0 is
// recorded here, once the allocation is out of the way -- the degrees, the out-counts and the exclusive scan that turns them
// into the row pointers orp [n + 1], and the read-back of *m = orp[n], the oriented entries, and *kmax, the longest oriented list
// (d_kmax: one word, zeroed here).  The caller allocates the columns, on its own account, and fills them: orient_pass with `fill`.
static inline int lzx_orient_count(lzx_ctx *c, const char *fn_name, LzxGraphRun &run, u32 G, u32 *d_deg, u64 *d_orp, u32 *d_kmax, u64 *m, u32 *kmax)
{
    const u32 n = (u32)c->n;
    hipStream_t st = c->stream;
    const size_t scan_len = (size_t)n + 1;   // (hipcub takes the count's type from its argument: not limited to 2^31)
    size_t tmp_bytes = 0;
    LZX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_orp, d_orp, scan_len, st));
    tmp_bytes = std::max<size_t>(tmp_bytes, 16);
    char what[96];
    std::snprintf(what, sizeof what, "the scan's scratch for the row pointers of %u vertices", n);
    LZX_TRY(lzx_alloc_state(fn_name, what, -1, tmp_bytes, tmp_bytes, &run.more[0]));
    LZX_HIP(hipEventRecord(run.ev0, st));
    LZX_HIP(hipMemsetAsync(d_kmax, 0, sizeof(u32), st));
    hipLaunchKernelGGL(k_tri_degrees, dim3(lzx_row_grid(n, LZX_TRI_BLOCK)), dim3(LZX_TRI_BLOCK), 0, st, c->d_row_ptr, c->d_col_idx, d_deg, n);
    LZX_HIP(hipGetLastError());
    orient_pass(G, st, c, d_deg, d_orp, nullptr, nullptr, d_kmax);
    LZX_HIP(hipGetLastError());
    LZX_HIP(hipcub::DeviceScan::ExclusiveSum(run.more[0], tmp_bytes, d_orp, d_orp, scan_len, st));
    LZX_HIP(hipMemcpyAsync(m, d_orp + n, sizeof(u64), hipMemcpyDeviceToHost, st));
    LZX_HIP(hipMemcpyAsync(kmax, d_kmax, sizeof(u32), hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    return LZX_OK;
}

// The split of the two launches that walk the oriented copy (lzx_triangles' counting, lzx_truss' support): rows of more than
// long_list out-entries (the test shape tri_long_list, else LZX_TRI_LONG) go to the long-row launch, which runs only when the
// longest list, kmax, is such a row; it stages up to `stage` entries of N+(a) and deals a row's out-edges to `slices` workgroups.
struct LzxTriShape {
    u32 long_list, stage, slices;
};
inline LzxTriShape lzx_tri_shape(const lzx_ctx *c, u32 kmax)
{
    const u32 long_list = lzx_shape_or(c->tri_long_opt, LZX_TRI_LONG);
    return {long_list, (u32)std::min<u64>(32ull * long_list, LZX_TRI_STAGE), std::min<u32>(std::max<u32>(kmax / 64, 1), LZX_TRI_SLICES)};
}
