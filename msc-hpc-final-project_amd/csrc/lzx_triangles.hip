// lzx_triangles.hip -- triangles per vertex, clustering coefficients, transitivity and average clustering of the handle's graph,
// on the device over the caller-order CSR the handle keeps (d_row_ptr / d_col_idx): include/lzx.h, lzx_triangles; DESIGN.md
// section 18.
//
// Orientation.  d_v = the entries of row v without the diagonal.  Vertices are ranked by (d_v, v) and every edge that is not a
// self loop is kept once, in the row of its lower-ranked end: the oriented CSR (64-bit row pointers, u32 columns), built by
// lzx_tri_orient.h, which lzx_truss.hip shares.
//   degrees    k_tri_degrees           one thread per row: lzx_degree_no_diagonal (lzx_graph_call.h)
//   out-counts k_tri_orient (count)    a group of G lanes per row counts the neighbours of higher rank; hipcub's exclusive scan
//                                      turns the counts into the row pointers, in place (lzx_orient_count)
//   fill       k_tri_orient (fill)     the same walk writes them: a ballot over the group orders the kept entries, so the
//                                      columns stay ascending by id (a monotone filter of an ascending row)
// A vertex of out-degree k has k neighbours of degree >= k: k^2 <= nnz, every oriented list has fewer than 2^16 entries while
// nnz < 2^32.
//
// Counting.  A triangle of ranks a < b < c is found exactly once, as c in N+(a) n N+(b) while row a handles its out-edge a -> b:
// the shorter of the two lists is walked, the longer binary-searched.  A hit adds 1 to t_c; per out-edge the hits are added to
// t_b in one add (when non-zero), per row their total to t_a in one add.
//   k_tri_count        rows of at most long_list out-entries: G lanes per row, the out-edges one after the other, the lanes
//                      over the walked list
//   k_tri_count_long   rows of more: a workgroup per (row, slice of its out-edges), a wavefront per out-edge.  N+(a) is staged
//                      in LDS when it has at most `stage` entries (<= LZX_TRI_STAGE), and then the hits on c are first counted
//                      in LDS, next to the staged entry, and leave with one add per entry; a longer list is read where it lies
//                      and every hit is its own add.
// Every add is a 64-bit integer vector atomic (32-bit in LDS): the counts do not depend on the order in which they land, nor on
// how ties in the ranking could have fallen.  No kernel waits on another workgroup; every loop is bounded by a list length.
//
// Statistics.  k_tri_stats forms c_v = 2 t_v / (d_v (d_v - 1)) (one correctly rounded division; 0 where d_v < 2 or t_v = 0) and
// block partials of sum c (fp64), sum t, sum d (d - 1) / 2 (u64) and max t; k_tri_close adds them in a fixed order.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "lzx_internal.h"
#include "lzx_graph_call.h"
#include "lzx_tri_orient.h"
#include "lzx_spmv_body.h"
#include "lzx_reduce.h"

static constexpr u32 LZX_TRI_STAT_GRID = 1024;   // block partials of the statistics pass (at most)

// rows of at most long_list out-entries: G lanes per row, 256 / G rows per workgroup
template <u32 G>
__global__ void __launch_bounds__(LZX_TRI_BLOCK)
k_tri_count(const u64 *orp, const u32 *oci, ull *tri, u32 n, u32 long_list)
{
    const u32 sub = threadIdx.x & (G - 1);
    const u64 row = (u64)blockIdx.x * (LZX_TRI_BLOCK / G) + threadIdx.x / G;
    u64 beg = 0;
    u32 ka = 0;
    if (row < n) {
        beg = orp[row];
        const u64 len = orp[row + 1] - beg;
        ka = len > long_list ? 0u : (u32)len;   // k_tri_count_long's
    }
    const u32 *A = oci + beg;
    u32 total = 0;
    for (u32 i = 0; i < ka; ++i) {   // (the same trips for every lane of the group)
        const u32 b = A[i];
        const u64 bb = orp[b];
        const u32 kb = (u32)(orp[b + 1] - bb);
        const u32 *B = oci + bb;
        const bool walk_a = ka <= kb;
        const u32 *S = walk_a ? A : B, *L = walk_a ? B : A;
        const u32 ks = walk_a ? ka : kb, kl = walk_a ? kb : ka;
        u32 hits = 0;
        for (u32 j = sub; j < ks; j += G) {
            const u32 x = S[j];
            const u32 at = lzx_lower_bound(L, kl, x);
            if (at < kl && L[at] == x) {
                ++hits;
                atomicAdd(&tri[x], 1ull);
            }
        }
#pragma unroll
        for (u32 o = G / 2; o > 0; o >>= 1) hits += (u32)__shfl_xor((int)hits, (int)o, 64);
        if (sub == 0 && hits) atomicAdd(&tri[b], (ull)hits);
        total += hits;
    }
    if (sub == 0 && total) atomicAdd(&tri[row], (ull)total);
}

// rows of more than long_list out-entries among the workgroup's 256 rows: the workgroup takes every gridDim.y-th group of four
// out-edges of each, a wavefront per out-edge
__global__ void __launch_bounds__(LZX_TRI_BLOCK)
k_tri_count_long(const u64 *orp, const u32 *oci, ull *tri, u32 n, u32 long_list, u32 stage)
{
    __shared__ u32 s_rows[LZX_TRI_BLOCK];
    __shared__ u32 s_count;
    __shared__ u32 s_a[LZX_TRI_STAGE];     // N+(a)
    __shared__ u32 s_hit[LZX_TRI_STAGE];   // hits on s_a[j] as the triangle's highest rank
    __shared__ ull s_tot[LZX_TRI_BLOCK / 64];
    const u64 mine = (u64)blockIdx.x * LZX_TRI_BLOCK + threadIdx.x;
    const u32 count = lzx_collect_long_rows(mine < n && orp[mine + 1] - orp[mine] > long_list, (u32)mine, s_rows, &s_count);
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr u32 W = LZX_TRI_BLOCK / 64;
    for (u32 r = 0; r < count; ++r) {
        const u32 row = s_rows[r];
        const u64 beg = orp[row];
        const u32 ka = (u32)(orp[row + 1] - beg);
        const u32 *A = oci + beg;
        const bool staged = ka <= stage;   // (stage <= LZX_TRI_STAGE)
        if (staged)
            for (u32 j = threadIdx.x; j < ka; j += LZX_TRI_BLOCK) {
                s_a[j] = A[j];
                s_hit[j] = 0;
            }
        __syncthreads();
        ull total = 0;
        for (u32 i = blockIdx.y * W + wave; i < ka; i += gridDim.y * W) {   // (the same trips for every lane of the wavefront)
            const u32 b = staged ? s_a[i] : A[i];
            const u64 bb = orp[b];
            const u32 kb = (u32)(orp[b + 1] - bb);
            const u32 *B = oci + bb;
            u32 hits = 0;
            if (ka <= kb) {   // walk N+(a), search N+(b)
                for (u32 j = lane; j < ka; j += 64) {
                    const u32 x = staged ? s_a[j] : A[j];
                    const u32 at = lzx_lower_bound(B, kb, x);
                    if (at < kb && B[at] == x) {
                        ++hits;
                        if (staged) atomicAdd(&s_hit[j], 1u);
                        else atomicAdd(&tri[x], 1ull);
                    }
                }
            } else {          // walk N+(b), search N+(a)
                for (u32 j = lane; j < kb; j += 64) {
                    const u32 x = B[j];
                    if (staged) {
                        const u32 at = lzx_lower_bound(s_a, ka, x);
                        if (at < ka && s_a[at] == x) {
                            ++hits;
                            atomicAdd(&s_hit[at], 1u);
                        }
                    } else {
                        const u32 at = lzx_lower_bound(A, ka, x);
                        if (at < ka && A[at] == x) {
                            ++hits;
                            atomicAdd(&tri[x], 1ull);
                        }
                    }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) hits += (u32)__shfl_xor((int)hits, o, 64);
            if (lane == 0 && hits) atomicAdd(&tri[b], (ull)hits);
            total += hits;
        }
        if (lane == 0) s_tot[wave] = total;
        __syncthreads();
        if (threadIdx.x == 0) {
            ull t = 0;
            for (u32 w = 0; w < W; ++w) t += s_tot[w];
            if (t) atomicAdd(&tri[row], t);
        }
        if (staged)
            for (u32 j = threadIdx.x; j < ka; j += LZX_TRI_BLOCK)
                if (s_hit[j]) atomicAdd(&tri[s_a[j]], (ull)s_hit[j]);
        __syncthreads();
    }
}

// c_v, and block partials: sum c (fp64), sum t, sum d (d - 1) / 2, max t
__global__ void __launch_bounds__(LZX_TRI_BLOCK)
k_tri_stats(const ull *tri, const u32 *deg, u32 n, double *clus, double *part_c, ull *part_t, ull *part_w, ull *part_m)
{
    __shared__ double s_c[LZX_TRI_BLOCK / 64];
    __shared__ ull s_t[LZX_TRI_BLOCK / 64], s_w[LZX_TRI_BLOCK / 64], s_m[LZX_TRI_BLOCK / 64];
    double sc = 0.0;
    ull st = 0, sw = 0, sm = 0;
    for (u64 i = (u64)blockIdx.x * LZX_TRI_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * LZX_TRI_BLOCK) {
        const ull t = tri[i], d = deg[i];
        const ull pairs2 = d < 2 ? 0ull : d * (d - 1);
        const double c = (pairs2 == 0 || t == 0) ? 0.0 : (double)(2 * t) / (double)pairs2;
        clus[i] = c;
        sc += c;
        st += t;
        sw += pairs2 >> 1;
        sm = t > sm ? t : sm;
    }
    sc = wave_sum(sc);
    st = wave_sum_u64(st);
    sw = wave_sum_u64(sw);
    sm = wave_max_u64(sm);
    if ((threadIdx.x & 63) == 0) {
        s_c[threadIdx.x >> 6] = sc;
        s_t[threadIdx.x >> 6] = st;
        s_w[threadIdx.x >> 6] = sw;
        s_m[threadIdx.x >> 6] = sm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part_c[blockIdx.x] = ((s_c[0] + s_c[1]) + s_c[2]) + s_c[3];
        part_t[blockIdx.x] = s_t[0] + s_t[1] + s_t[2] + s_t[3];
        part_w[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        part_m[blockIdx.x] = block_max_u64(s_m);
    }
}

// out4: the mean of c (a double's bits), sum t, sum d (d - 1) / 2, max t
__global__ void __launch_bounds__(LZX_VEC_BLOCK)
k_tri_close(const double *part_c, const ull *part_t, const ull *part_w, const ull *part_m, u32 np, u32 n, ull *out4)
{
    __shared__ double sh[4];
    __shared__ ull s_t[LZX_VEC_BLOCK / 64], s_w[LZX_VEC_BLOCK / 64], s_m[LZX_VEC_BLOCK / 64];
    const double total = block_sum_fixed_256(part_c, np, sh);
    ull st = 0, sw = 0, sm = 0;
    for (u32 i = threadIdx.x; i < np; i += LZX_VEC_BLOCK) {
        st += part_t[i];
        sw += part_w[i];
        sm = part_m[i] > sm ? part_m[i] : sm;
    }
    st = wave_sum_u64(st);
    sw = wave_sum_u64(sw);
    sm = wave_max_u64(sm);
    if ((threadIdx.x & 63) == 0) {
        s_t[threadIdx.x >> 6] = st;
        s_w[threadIdx.x >> 6] = sw;
        s_m[threadIdx.x >> 6] = sm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out4[0] = (ull)__double_as_longlong(total / (double)n);
        out4[1] = s_t[0] + s_t[1] + s_t[2] + s_t[3];
        out4[2] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        out4[3] = block_max_u64(s_m);
    }
}

extern "C" int lzx_triangles(lzx_handle c, uint64_t *tri, double *clustering, lzx_triangles_info *info)
{
    const char *fn_name = "lzx_triangles";
    LZX_TRY(lzx_graph_call_check(c, fn_name, "triangles are counted"));
    const auto t0 = std::chrono::steady_clock::now();
    const u32 n = (u32)c->n;

    // the vertices' arena; the oriented columns follow in one of their own once the scan has counted them
    const u32 np = (u32)std::min<u64>(LZX_TRI_STAT_GRID, ((u64)n + LZX_TRI_BLOCK - 1) / LZX_TRI_BLOCK);   // the partials of the statistics
    LZX_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    u64 *d_orp;
    ull *d_tri, *d_pt, *d_pw, *d_pm, *d_out;
    double *d_clus, *d_pc;
    u32 *d_kmax, *d_deg, *d_oci;
    u64 bytes = 0;
    LzxGraphRun run(c);   // more[0]: the scan's scratch, more[1]: the oriented columns
    char what[160];
    std::snprintf(what, sizeof what, "the state of %u vertices (row pointers, degrees, counts, coefficients, before the oriented columns)", n);
    LZX_TRY(lzx_carve_state(fn_name, what, c->tri_cap_opt, 0, &run.arena, &bytes, [&](LzxCarver &k) {
        k.take(d_orp, (u64)n + 1);
        k.take(d_tri, n);
        k.take(d_clus, n);
        k.take(d_pc, np);
        for (ull **p : {&d_pt, &d_pw, &d_pm}) k.take(*p, np);
        k.take(d_out, 4);
        k.take(d_kmax, 2);
        k.take(d_deg, lzx_even(n));
    }));
    LZX_TRY(run.events(2));

    // ---- the oriented copy ----
    const u32 Go = lzx_lanes_per_row(c, c->nnz, 64);
    u64 m = 0;
    u32 kmax = 0;
    LZX_TRY(lzx_orient_count(c, fn_name, run, Go, d_deg, d_orp, d_kmax, &m, &kmax));
    LZX_HIP(hipMemsetAsync(d_tri, 0, sizeof(ull) * n, st));
    // the oriented columns: the scan's total, which is what the fill writes whatever was handed over ((nnz - self loops) / 2 of a
    // symmetric matrix)
    std::snprintf(what, sizeof what, "the state of %u vertices (an oriented copy of %llu entries, degrees, counts, coefficients)", n, (ull)m);
    LZX_TRY(lzx_carve_state(fn_name, what, c->tri_cap_opt, bytes, &run.more[1], nullptr, [&](LzxCarver &k) { k.take(d_oci, std::max<u64>(m, 1)); }));
    if (m) {
        orient_pass(Go, st, c, d_deg, nullptr, d_orp, d_oci, nullptr);
        LZX_HIP(hipGetLastError());
    }
    LZX_HIP(hipEventRecord(run.ev1, st));
    LZX_HIP(hipStreamSynchronize(st));
    float orient_ms = 0.f;
    LZX_HIP(hipEventElapsedTime(&orient_ms, run.ev0, run.ev1));

    // ---- counting: lanes per row about half the mean oriented degree ----
    const u32 G = lzx_lanes_per_row(c, m, 32, LZX_OVER_ORIENTED);
    LZX_HIP(hipEventRecord(run.ev0, st));
    if (m) {
        const LzxTriShape shape = lzx_tri_shape(c, kmax);
        lzx_with_lanes<32>(G, [&](auto g) {
            hipLaunchKernelGGL(k_tri_count<g>, dim3(lzx_row_grid(n, LZX_TRI_BLOCK / g)), dim3(LZX_TRI_BLOCK), 0, st, d_orp, d_oci, d_tri, n,
                               shape.long_list);
        });
        LZX_HIP(hipGetLastError());
        if (kmax > shape.long_list) {
            hipLaunchKernelGGL(k_tri_count_long, dim3(lzx_row_grid(n, LZX_TRI_BLOCK), shape.slices), dim3(LZX_TRI_BLOCK), 0, st, d_orp, d_oci, d_tri, n,
                               shape.long_list, shape.stage);
            LZX_HIP(hipGetLastError());
        }
    }
    LZX_HIP(hipEventRecord(run.ev1, st));

    // ---- coefficients and statistics ----
    hipLaunchKernelGGL(k_tri_stats, dim3(np), dim3(LZX_TRI_BLOCK), 0, st, d_tri, d_deg, n, d_clus, d_pc, d_pt, d_pw, d_pm);
    LZX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_tri_close, dim3(1), dim3(LZX_VEC_BLOCK), 0, st, d_pc, d_pt, d_pw, d_pm, np, n, d_out);
    LZX_HIP(hipGetLastError());
    ull out4[4] = {0, 0, 0, 0};
    LZX_HIP(hipMemcpyAsync(out4, d_out, sizeof(out4), hipMemcpyDeviceToHost, st));
    if (tri) LZX_HIP(hipMemcpyAsync(tri, d_tri, sizeof(ull) * n, hipMemcpyDeviceToHost, st));
    if (clustering) LZX_HIP(hipMemcpyAsync(clustering, d_clus, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    float count_ms = 0.f;
    LZX_HIP(hipEventElapsedTime(&count_ms, run.ev0, run.ev1));
    if (info) {
        double avg;
        static_assert(sizeof(avg) == sizeof(out4[0]), "a double's bits in a 64-bit word");
        memcpy(&avg, &out4[0], sizeof(avg));
        info->triangles = out4[1] / 3;
        info->wedges = out4[2];
        info->max_triangles = out4[3];
        info->oriented_entries = m;
        info->oriented_max_degree = kmax;
        info->reserved_ = 0;
        info->avg_clustering = avg;
        info->orient_ms = orient_ms;
        info->count_ms = count_ms;
        info->loop_ms = lzx_ms_since(t0);
    }
    return LZX_OK;
}
