// lzx_truss.hip -- edge supports, truss numbers and truss layers of the handle's graph (networkx.k_truss), on the device over the
// caller-order CSR the handle keeps (d_row_ptr / d_col_idx): include/lzx.h, lzx_truss; DESIGN.md section 20.
//
// Definitions.  support(e) = the triangles through the undirected edge e (self loops are no edges and close no triangle).
// Rounds are numbered from 1 and k_0 = 2; round r has k_r = max(k_{r-1}, 2 + the smallest remaining support of a remaining edge)
// and removes, all at once, every remaining edge whose remaining support is <= k_r - 2: truss[e] = k_r, layer[e] = r.  The
// remaining support counts the triangles whose three edges all remain.  Below s = k - 2 is the support level.
//
// Edge ids.  The oriented copy of lzx_tri_orient.h keeps every edge once, in the row of its lower-ranked end; an edge's id is its
// position in the oriented columns (oci), m < 2^32 of them, and src[e] is its oriented row.
//   k_truss_src        one thread per edge: the row whose piece of the oriented columns holds it (a search of the row pointers)
//   k_truss_eid        G lanes per row of the caller-order CSR: entry (u, v) searches its higher-ranked end in the oriented row of
//                      its lower-ranked end; a diagonal entry, and an entry whose search fails (only on a matrix that is not
//                      symmetric), gets LZX_TRUSS_NONE.  Every later use range-checks what it reads from eid.
//
// Support.  The counting walk of lzx_triangles (a triangle of ranks a < b < c is found once, as c in N+(a) n N+(b) while row a
// handles its out-edge a -> b; the shorter list walked, the longer searched) with u32 counters per edge: at a hit the walked
// index and the search result are the positions of the two far edges a -> c and b -> c, which get one add each; the out-edge gets
// its hits in one add.
//   k_truss_support        rows of at most long_list out-entries: G lanes per row
//   k_truss_support_long   rows of more: a workgroup per (row, slice of its out-edges), a wavefront per out-edge; N+(a) staged in
//                          LDS when it has at most `stage` entries, and then the adds on the edges of row a are first counted in
//                          LDS and leave with one add per edge
//   k_truss_stats          block partials of the sum (u64) and the maximum of the supports; the host adds them
//
// Push peeling over one queue of edge ids, as lzx_core.hip peels vertices: the loop, the level start and the push of lzx_peel.h.
// sup[e] is the remaining support, mark[e] is 0 for an edge not yet removed and else its layer, and every edge is appended to
// `queue` exactly once, so that a round's frontier is a window [beg, end) of it and what a launch appends behind `end` is the
// next window.
//   level start  k_peel_level        (lzx_peel.h) one thread per edge, when the frontier is empty: an unmarked edge with sup <= s
//                                    is marked (mark = r, truss = s + 2) and appended, the others contribute to a minimum.  The
//                                    host tries s + 1 first and only if nothing was appended sweeps again with the minimum.
//   peel         k_truss_peel<G>     G lanes per edge e1 = (a, b) of the window: the full rows of a and b in the caller-order CSR are
//                                    intersected, the shorter walked and the longer searched; w = a and w = b (self loops) are
//                                    skipped.  A common neighbour w gives e2 = eid[w's place in the walked row] and e3 = eid[its
//                                    place in the other]: the triangle rule below, then the decrements.
//                k_truss_peel_long   the window's edges whose shorter row has more than long_row entries: a workgroup per (edge,
//                                    slice of the shorter row)
// The triangle rule, for the launch of round r.  The triangle is dead if mark[e2] or mark[e3] is non-zero and < r: it died in an
// earlier round and was counted then.  Otherwise, with "in the window" meaning mark == r:
//   both in the window       nothing: all three edges leave, nobody is left to tell
//   exactly one, say e2      e1 and e2 both see this triangle; the one with the smaller edge id decrements e3
//   neither                  e1 alone sees it: both are decremented
// so every triangle that dies in round r takes exactly one from each of its edges that stays.  A decrement is lzx_peel_push:
// old = atomicSub(&sup[x], 1); the one lane that sees old == s + 1 takes the mark by atomicCAS(&mark[x], 0, r + 1), writes
// truss[x] = s + 2 and appends x.  A mark of 0 and a mark of r + 1 decide alike in the rule, and the marks equal to r or less
// were written by earlier launches: which edges a round decrements, and how often, does not depend on the order in which its
// lanes run, so every run marks the same edges in the same round.  An edge that has been marked is at or below s; a later
// decrement of it returns at most s, never s + 1, while the level lasts: it is appended once.
//
// A matrix that is not symmetric is not detected and its numbers mean nothing; counters may wrap.  The call still stays inside its
// memory and ends: the mark is taken by a compare-and-swap, so no edge is queued twice and the queue's end never passes m -- every
// append is clamped to the m entries all the same --, every id read from eid is range-checked, every window is a fresh piece of
// the queue and a level start always finds the edge of the minimum.
//
// All atomics are 32-bit integer vector atomics, in global memory and in LDS; nothing is floating-point.  No kernel waits on
// another workgroup; every device loop is bounded by a row, list or window length.  The loops around lzx_wave_append run the same
// trips on every lane of a wavefront.  The host reads one word per peeling round and two per level start.
#include <algorithm>
#include <chrono>
#include <utility>
#include <vector>

#include "lzx_internal.h"
#include "lzx_graph_call.h"
#include "lzx_tri_orient.h"
#include "lzx_peel.h"
#include "lzx_spmv_body.h"
#include "lzx_reduce.h"

static constexpr u32 LZX_TRUSS_BLOCK = 256;
static constexpr u32 LZX_TRUSS_STAT_GRID = 1024; // block partials of the support statistics (at most)
static constexpr u32 LZX_TRUSS_NONE = 0xffffffffu;
static_assert(LZX_TRUSS_BLOCK == LZX_TRI_BLOCK, "the support kernels are laid out as lzx_triangles' counting kernels");

// ---- edge ids -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LZX_TRUSS_BLOCK) k_truss_src(const u64 *orp, u32 n, u32 m, u32 *src)
{
    const u64 e = (u64)blockIdx.x * LZX_TRUSS_BLOCK + threadIdx.x;
    if (e >= m) return;
    u32 lo = 0, hi = n;   // the last row with orp[row] <= e (orp[0] = 0 <= e < m = orp[n])
    while (hi - lo > 1) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (orp[mid] <= e) lo = mid;
        else hi = mid;
    }
    src[e] = lo;
}

template <u32 G>
__global__ void __launch_bounds__(LZX_TRUSS_BLOCK)
k_truss_eid(const u64 *row_ptr, const u32 *col_idx, const u32 *deg, const u64 *orp, const u32 *oci, u32 n, u32 *eid)
{
    const u32 sub = threadIdx.x & (G - 1);
    const u64 row = (u64)blockIdx.x * (LZX_TRUSS_BLOCK / G) + threadIdx.x / G;
    if (row >= n) return;
    const u64 beg = row_ptr[row], end = row_ptr[row + 1];
    const u32 dv = deg[row];
    for (u64 e = beg + sub; e < end; e += G) {
        const u32 col = col_idx[e];
        u32 id = LZX_TRUSS_NONE;
        if (col != (u32)row) {
            const u32 du = deg[col];
            const bool col_higher = du > dv || (du == dv && col > (u32)row);
            const u32 a = col_higher ? (u32)row : col, b = col_higher ? col : (u32)row;
            const u64 ab = orp[a];
            const u32 ka = (u32)(orp[a + 1] - ab);
            const u32 at = lzx_lower_bound(oci + ab, ka, b);
            if (at < ka && oci[ab + at] == b) id = (u32)(ab + at);
        }
        eid[e] = id;
    }
}

// ---- support ------------------------------------------------------------------------------------------------------------------
// rows of at most long_list out-entries: G lanes per row, 256 / G rows per workgroup
template <u32 G>
__global__ void __launch_bounds__(LZX_TRUSS_BLOCK)
k_truss_support(const u64 *orp, const u32 *oci, u32 *sup, u32 n, u32 long_list)
{
    const u32 sub = threadIdx.x & (G - 1);
    const u64 row = (u64)blockIdx.x * (LZX_TRUSS_BLOCK / G) + threadIdx.x / G;
    u32 beg = 0, ka = 0;
    if (row < n) {
        beg = (u32)orp[row];
        const u64 len = orp[row + 1] - orp[row];
        ka = len > long_list ? 0u : (u32)len;   // k_truss_support_long's
    }
    const u32 *A = oci + beg;
    for (u32 i = 0; i < ka; ++i) {   // (the same trips for every lane of the group)
        const u32 b = A[i];
        const u32 bb = (u32)orp[b];
        const u32 kb = (u32)(orp[b + 1] - orp[b]);
        const u32 *B = oci + bb;
        const bool walk_a = ka <= kb;
        const u32 *S = walk_a ? A : B, *L = walk_a ? B : A;
        const u32 ks = walk_a ? ka : kb, kl = walk_a ? kb : ka;
        const u32 s0 = walk_a ? beg : bb, l0 = walk_a ? bb : beg;   // the edge ids of the two lists' first entries
        u32 hits = 0;
        for (u32 j = sub; j < ks; j += G) {
            const u32 x = S[j];
            const u32 at = lzx_lower_bound(L, kl, x);
            if (at < kl && L[at] == x) {
                ++hits;
                atomicAdd(&sup[s0 + j], 1u);
                atomicAdd(&sup[l0 + at], 1u);
            }
        }
#pragma unroll
        for (u32 o = G / 2; o > 0; o >>= 1) hits += (u32)__shfl_xor((int)hits, (int)o, 64);
        if (sub == 0 && hits) atomicAdd(&sup[beg + i], hits);
    }
}

// rows of more than long_list out-entries among the workgroup's 256 rows: the workgroup takes every gridDim.y-th group of four
// out-edges of each, a wavefront per out-edge
__global__ void __launch_bounds__(LZX_TRUSS_BLOCK)
k_truss_support_long(const u64 *orp, const u32 *oci, u32 *sup, u32 n, u32 long_list, u32 stage)
{
    __shared__ u32 s_rows[LZX_TRUSS_BLOCK];
    __shared__ u32 s_count;
    __shared__ u32 s_a[LZX_TRI_STAGE];     // N+(a)
    __shared__ u32 s_hit[LZX_TRI_STAGE];   // adds on the edge a -> s_a[j]
    const u64 mine = (u64)blockIdx.x * LZX_TRUSS_BLOCK + threadIdx.x;
    const u32 count = lzx_collect_long_rows(mine < n && orp[mine + 1] - orp[mine] > long_list, (u32)mine, s_rows, &s_count);
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr u32 W = LZX_TRUSS_BLOCK / 64;
    for (u32 r = 0; r < count; ++r) {
        const u32 row = s_rows[r];
        const u32 beg = (u32)orp[row];
        const u32 ka = (u32)(orp[row + 1] - orp[row]);
        const u32 *A = oci + beg;
        const bool staged = ka <= stage;   // (stage <= LZX_TRI_STAGE)
        if (staged)
            for (u32 j = threadIdx.x; j < ka; j += LZX_TRUSS_BLOCK) {
                s_a[j] = A[j];
                s_hit[j] = 0;
            }
        __syncthreads();
        for (u32 i = blockIdx.y * W + wave; i < ka; i += gridDim.y * W) {   // (the same trips for every lane of the wavefront)
            const u32 b = staged ? s_a[i] : A[i];
            const u32 bb = (u32)orp[b];
            const u32 kb = (u32)(orp[b + 1] - orp[b]);
            const u32 *B = oci + bb;
            u32 hits = 0;
            if (ka <= kb) {   // walk N+(a), search N+(b)
                for (u32 j = lane; j < ka; j += 64) {
                    const u32 x = staged ? s_a[j] : A[j];
                    const u32 at = lzx_lower_bound(B, kb, x);
                    if (at < kb && B[at] == x) {
                        ++hits;
                        if (staged) atomicAdd(&s_hit[j], 1u);
                        else atomicAdd(&sup[beg + j], 1u);
                        atomicAdd(&sup[bb + at], 1u);
                    }
                }
            } else {          // walk N+(b), search N+(a)
                for (u32 j = lane; j < kb; j += 64) {
                    const u32 x = B[j];
                    const u32 at = lzx_lower_bound(staged ? s_a : A, ka, x);
                    if (at < ka && (staged ? s_a[at] : A[at]) == x) {
                        ++hits;
                        if (staged) atomicAdd(&s_hit[at], 1u);
                        else atomicAdd(&sup[beg + at], 1u);
                        atomicAdd(&sup[bb + j], 1u);
                    }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) hits += (u32)__shfl_xor((int)hits, o, 64);
            if (lane == 0 && hits) {
                if (staged) atomicAdd(&s_hit[i], hits);
                else atomicAdd(&sup[beg + i], hits);
            }
        }
        __syncthreads();
        if (staged)
            for (u32 j = threadIdx.x; j < ka; j += LZX_TRUSS_BLOCK)
                if (s_hit[j]) atomicAdd(&sup[beg + j], s_hit[j]);
        __syncthreads();
    }
}

// block partials: the sum and the maximum of the supports
__global__ void __launch_bounds__(LZX_TRUSS_BLOCK) k_truss_stats(const u32 *sup, u32 m, ull *part_sum, ull *part_max)
{
    __shared__ ull s_t[LZX_TRUSS_BLOCK / 64], s_m[LZX_TRUSS_BLOCK / 64];
    ull st = 0, sm = 0;
    for (u64 i = (u64)blockIdx.x * LZX_TRUSS_BLOCK + threadIdx.x; i < m; i += (u64)gridDim.x * LZX_TRUSS_BLOCK) {
        const ull t = sup[i];
        st += t;
        sm = t > sm ? t : sm;
    }
    st = wave_sum_u64(st);
    sm = wave_max_u64(sm);
    if ((threadIdx.x & 63) == 0) {
        s_t[threadIdx.x >> 6] = st;
        s_m[threadIdx.x >> 6] = sm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part_sum[blockIdx.x] = s_t[0] + s_t[1] + s_t[2] + s_t[3];
        part_max[blockIdx.x] = block_max_u64(s_m);
    }
}

// ---- peel ---------------------------------------------------------------------------------------------------------------------
// what the peel works on
struct TrussPeel {
    const u64 *row_ptr;
    const u32 *col_idx, *eid, *src, *oci;
    u32 *sup, *mark, *truss, *queue, *tail;
    u32 m, wbeg, wlen, s, r, long_row;
};

// the edge e1 = (a, b) of the window: the shorter of the two full rows is S (walked), the other L (searched)
struct TrussRows {
    u64 beg_s, beg_l;
    u32 len_s, len_l, a, b;
};

__device__ __forceinline__ TrussRows truss_rows(const TrussPeel &p, u32 e1)
{
    TrussRows t;
    t.a = p.src[e1];
    t.b = p.oci[e1];
    const u64 ba = p.row_ptr[t.a], bb = p.row_ptr[t.b];
    const u32 la = (u32)(p.row_ptr[t.a + 1] - ba), lb = (u32)(p.row_ptr[t.b + 1] - bb);
    const bool walk_a = la <= lb;
    t.beg_s = walk_a ? ba : bb;
    t.beg_l = walk_a ? bb : ba;
    t.len_s = walk_a ? la : lb;
    t.len_l = walk_a ? lb : la;
    return t;
}

// entry j of the walked row of e1 (have: this lane holds one): the common neighbour, the triangle rule, the two decrements.
// Every lane of the wavefront calls it together.
__device__ __forceinline__ void truss_entry(bool have, u64 j, u32 e1, const TrussRows &t, const TrussPeel &p)
{
    bool d2 = false, d3 = false;
    u32 e2 = 0, e3 = 0;
    if (have) {
        const u32 w = p.col_idx[t.beg_s + j];
        if (w != t.a && w != t.b) {
            const u32 at = lzx_lower_bound(p.col_idx + t.beg_l, t.len_l, w);
            if (at < t.len_l && p.col_idx[t.beg_l + at] == w) {
                e2 = p.eid[t.beg_s + j];
                e3 = p.eid[t.beg_l + at];
                if (e2 < p.m && e3 < p.m) {
                    const u32 m2 = p.mark[e2], m3 = p.mark[e3];
                    const bool dead = (m2 != 0 && m2 < p.r) || (m3 != 0 && m3 < p.r);
                    const bool in2 = m2 == p.r, in3 = m3 == p.r;
                    if (!dead && !(in2 && in3)) {
                        d2 = in3 ? e1 < e3 : !in2;
                        d3 = in2 ? e1 < e2 : !in3;
                    }
                }
            }
        }
    }
    lzx_peel_push(d2, e2, p.sup, p.mark, p.truss, p.queue, p.tail, p.m, p.s, p.s + 2, p.r);
    lzx_peel_push(d3, e3, p.sup, p.mark, p.truss, p.queue, p.tail, p.m, p.s, p.s + 2, p.r);
}

// edges of the window queue[wbeg .. wbeg + wlen) whose shorter row has at most long_row entries: G lanes per edge
template <u32 G>
__global__ void __launch_bounds__(LZX_TRUSS_BLOCK) k_truss_peel(TrussPeel p)
{
    const u32 sub = threadIdx.x & (G - 1);
    const u64 idx = (u64)blockIdx.x * (LZX_TRUSS_BLOCK / G) + threadIdx.x / G;
    TrussRows t = {0, 0, 0, 0, 0, 0};
    u32 e1 = 0, len = 0;
    if (idx < p.wlen) {
        e1 = p.queue[p.wbeg + idx];
        if (e1 < p.m) {
            t = truss_rows(p, e1);
            len = t.len_s > p.long_row ? 0u : t.len_s;   // k_truss_peel_long's
        }
    }
    u32 trips = (len + G - 1) / G;
#pragma unroll
    for (int o = 32; o >= (int)G; o >>= 1) trips = max(trips, (u32)__shfl_xor((int)trips, o, 64));
    for (u32 i = 0; i < trips; ++i) {   // (the same trips for every lane of the wavefront: the appends are formed together)
        const u32 j = i * G + sub;
        truss_entry(j < len, j, e1, t, p);
    }
}

// edges whose shorter row has more than long_row entries among the workgroup's 256 window places: the workgroup takes every
// gridDim.y-th run of 256 entries of that row
__global__ void __launch_bounds__(LZX_TRUSS_BLOCK) k_truss_peel_long(TrussPeel p)
{
    __shared__ u32 s_rows[LZX_TRUSS_BLOCK];
    __shared__ u32 s_count;
    const u64 idx = (u64)blockIdx.x * LZX_TRUSS_BLOCK + threadIdx.x;
    u32 mine = 0;
    bool is_long = false;
    if (idx < p.wlen) {
        mine = p.queue[p.wbeg + idx];
        if (mine < p.m) is_long = truss_rows(p, mine).len_s > p.long_row;
    }
    const u32 count = lzx_collect_long_rows(is_long, mine, s_rows, &s_count);
    for (u32 i = 0; i < count; ++i) {
        const u32 e1 = s_rows[i];
        const TrussRows t = truss_rows(p, e1);
        // (the same trips for every lane of the workgroup)
        for (u64 j0 = (u64)blockIdx.y * LZX_TRUSS_BLOCK; j0 < t.len_s; j0 += (u64)gridDim.y * LZX_TRUSS_BLOCK) {
            const u64 j = j0 + threadIdx.x;
            truss_entry(j < t.len_s, j, e1, t, p);
        }
    }
}

// ---- hand back ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LZX_TRUSS_BLOCK) k_truss_gather(const u32 *eid, const u32 *val, u32 m, u64 nnz, u32 *out)
{
    const u64 e = (u64)blockIdx.x * LZX_TRUSS_BLOCK + threadIdx.x;
    if (e >= nnz) return;
    const u32 id = eid[e];
    out[e] = id < m ? val[id] : 0u;
}

template <u32 G>
__global__ void __launch_bounds__(LZX_TRUSS_BLOCK) k_truss_vertex(const u64 *row_ptr, const u32 *eid, const u32 *truss, u32 n, u32 m, u32 *out)
{
    const u32 sub = threadIdx.x & (G - 1);
    const u64 row = (u64)blockIdx.x * (LZX_TRUSS_BLOCK / G) + threadIdx.x / G;
    u64 beg = 0, end = 0;
    if (row < n) {
        beg = row_ptr[row];
        end = row_ptr[row + 1];
    }
    u32 top = 0;
    for (u64 e = beg + sub; e < end; e += G) {
        const u32 id = eid[e];
        if (id < m) top = max(top, truss[id]);
    }
#pragma unroll
    for (u32 o = G / 2; o > 0; o >>= 1) top = max(top, (u32)__shfl_xor((int)top, (int)o, 64));
    if (sub == 0 && row < n) out[row] = top;
}

extern "C" int lzx_truss(lzx_handle c, uint32_t *support, uint32_t *truss, uint32_t *layer, uint32_t *vertex_truss, lzx_truss_info *info)
{
    const char *fn_name = "lzx_truss";
    LZX_TRY(lzx_graph_call_check(c, fn_name, "truss numbers are peeled"));
    const auto t0 = std::chrono::steady_clock::now();
    const u32 n = (u32)c->n;
    const u64 nnz = c->nnz;

    // the vertex arena
    const u32 np = LZX_TRUSS_STAT_GRID;   // the partials of the statistics
    LZX_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    u64 *d_orp;
    ull *d_psum, *d_pmax;
    u32 *d_deg, *d_kmax, *d_counters;
    u64 bytes = 0;
    LzxGraphRun run(c);   // more[0]: the scan's scratch, more[1]: the edge state
    char what[192];
    std::snprintf(what, sizeof what, "the state of %u vertices (oriented row pointers, degrees, before the state of the edges)", n);
    LZX_TRY(lzx_carve_state(fn_name, what, c->truss_cap_opt, 0, &run.arena, &bytes, [&](LzxCarver &k) {
        k.take(d_orp, (u64)n + 1);
        k.take(d_psum, np);
        k.take(d_pmax, np);
        k.take(d_deg, n);        // (the vertices' truss numbers once the oriented copy stands)
        k.take(d_kmax, 2);       // the longest oriented list, a spare
        k.take(d_counters, 2);   // the queue's end, the minimum
    }));
    LZX_TRY(run.events(2));

    // ---- the oriented copy: lzx_triangles' ----
    const u32 Go = lzx_lanes_per_row(c, nnz, 64);
    u64 m64 = 0;
    u32 kmax = 0;
    LZX_TRY(lzx_orient_count(c, fn_name, run, Go, d_deg, d_orp, d_kmax, &m64, &kmax));
    LZX_HIP(hipMemsetAsync(d_counters, 0, 2 * sizeof(u32), st));
    if (m64 >= LZX_TRUSS_NONE) LZX_FAIL(LZX_ERR_LIMIT, "%s: %llu edges; edge ids are 32-bit (fewer than 2^32 - 1 edges)", fn_name, (ull)m64);
    const u32 m = (u32)m64;

    // the edge state; d_stage: one staging buffer for the per-entry outputs
    const u64 m_al = std::max<u64>(m, 1), z_al = std::max<u64>(nnz, 1);
    u32 *d_oci, *d_src, *d_sup, *d_mark, *d_truss, *d_queue, *d_eid, *d_stage;
    std::snprintf(what, sizeof what, "the state of %u vertices and %u edges (oriented copy, edge ids of %llu entries, supports, marks, truss numbers, the queue)",
                  n, m, (ull)nnz);
    LZX_TRY(lzx_carve_state(fn_name, what, c->truss_cap_opt, bytes, &run.more[1], nullptr, [&](LzxCarver &k) {
        for (u32 **p : {&d_oci, &d_src, &d_sup, &d_mark, &d_truss, &d_queue}) k.take(*p, m_al);
        for (u32 **p : {&d_eid, &d_stage}) k.take(*p, z_al);
    }));
    const u32 ge = (u32)(((u64)m + LZX_TRUSS_BLOCK - 1) / LZX_TRUSS_BLOCK);
    const u32 gz = (u32)((nnz + LZX_TRUSS_BLOCK - 1) / LZX_TRUSS_BLOCK);
    // (sup, mark, truss: zero; the queue is written before it is read)
    LZX_HIP(hipMemsetAsync(d_sup, 0, sizeof(u32) * 3 * m_al, st));
    if (m) {
        orient_pass(Go, st, c, d_deg, nullptr, d_orp, d_oci, nullptr);
        LZX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_truss_src, dim3(ge), dim3(LZX_TRUSS_BLOCK), 0, st, d_orp, n, m, d_src);
        LZX_HIP(hipGetLastError());
    }
    if (nnz) {
        lzx_with_lanes<64>(Go, [&](auto g) {
            hipLaunchKernelGGL(k_truss_eid<g>, dim3(lzx_row_grid(n, LZX_TRUSS_BLOCK / g)), dim3(LZX_TRUSS_BLOCK), 0, st, c->d_row_ptr, c->d_col_idx,
                               d_deg, d_orp, d_oci, n, d_eid);
        });
        LZX_HIP(hipGetLastError());
    }

    // ---- support: lanes per row about half the mean oriented degree, the split of lzx_triangles at a long list ----
    u64 sup_sum = 0, sup_max = 0;
    if (m) {
        const u32 G = lzx_lanes_per_row(c, m, 32, LZX_OVER_ORIENTED);
        const LzxTriShape shape = lzx_tri_shape(c, kmax);
        lzx_with_lanes<32>(G, [&](auto g) {
            hipLaunchKernelGGL(k_truss_support<g>, dim3(lzx_row_grid(n, LZX_TRUSS_BLOCK / g)), dim3(LZX_TRUSS_BLOCK), 0, st, d_orp, d_oci, d_sup, n,
                               shape.long_list);
        });
        LZX_HIP(hipGetLastError());
        if (kmax > shape.long_list) {
            hipLaunchKernelGGL(k_truss_support_long, dim3(lzx_row_grid(n, LZX_TRUSS_BLOCK), shape.slices), dim3(LZX_TRUSS_BLOCK), 0, st, d_orp, d_oci, d_sup,
                               n, shape.long_list, shape.stage);
            LZX_HIP(hipGetLastError());
        }
        const u32 gs = std::min<u32>(np, ge);
        hipLaunchKernelGGL(k_truss_stats, dim3(gs), dim3(LZX_TRUSS_BLOCK), 0, st, d_sup, m, d_psum, d_pmax);
        LZX_HIP(hipGetLastError());
        LZX_HIP(hipEventRecord(run.ev1, st));
        std::vector<ull> parts(2 * (size_t)np, 0);
        LZX_HIP(hipMemcpyAsync(parts.data(), d_psum, sizeof(ull) * gs, hipMemcpyDeviceToHost, st));
        LZX_HIP(hipMemcpyAsync(parts.data() + np, d_pmax, sizeof(ull) * gs, hipMemcpyDeviceToHost, st));
        LZX_HIP(hipStreamSynchronize(st));
        for (u32 i = 0; i < gs; ++i) {
            sup_sum += parts[i];
            sup_max = std::max<u64>(sup_max, parts[np + i]);
        }
    } else {
        LZX_HIP(hipEventRecord(run.ev1, st));
        LZX_HIP(hipStreamSynchronize(st));
    }
    float support_ms = 0.f;
    LZX_HIP(hipEventElapsedTime(&support_ms, run.ev0, run.ev1));
    if (support && nnz) {   // the supports leave before the peel counts them down
        hipLaunchKernelGGL(k_truss_gather, dim3(gz), dim3(LZX_TRUSS_BLOCK), 0, st, d_eid, d_sup, m, nnz, d_stage);
        LZX_HIP(hipGetLastError());
        LZX_HIP(hipMemcpyAsync(support, d_stage, sizeof(u32) * nnz, hipMemcpyDeviceToHost, st));
        LZX_HIP(hipStreamSynchronize(st));
    }

    // ---- the peel.  Lanes per edge: about half the mean row length.  Edges whose shorter row has more than 64 G entries go to the
    // long-row launch, which runs only when the graph has such a row ----
    const u32 G = lzx_lanes_per_row(c, nnz, 32);
    const u32 long_row = lzx_shape_or(c->truss_long_opt, 64 * G);
    const u32 slices = lzx_peel_slices(c->max_degree, LZX_TRUSS_BLOCK);
    TrussPeel p = {c->d_row_ptr, c->d_col_idx, d_eid, d_src, d_oci, d_sup, d_mark, d_truss, d_queue, d_counters, m, 0, 0, 0, 0, long_row};
    LZX_HIP(hipEventRecord(run.ev0, st));
    LzxPeelResult peel;
    LZX_TRY(lzx_peel_loop(
        fn_name, {"edge", "remaining support", "edges"}, st, d_counters, m,
        [&](u32 s_try, u32 r) -> int {
            hipLaunchKernelGGL(k_peel_level, dim3(lzx_row_grid(m, LZX_PEEL_BLOCK)), dim3(LZX_PEEL_BLOCK), 0, st, d_sup, d_mark, d_truss, d_queue, d_counters, m, s_try, s_try + 2, r);
            LZX_HIP(hipGetLastError());
            return LZX_OK;
        },
        [&](u32 wbeg, u32 wlen, u32 s, u32 r) -> int {
            p.wbeg = wbeg;
            p.wlen = wlen;
            p.s = s;
            p.r = r;
            lzx_with_lanes<32>(G, [&](auto g) {
                hipLaunchKernelGGL(k_truss_peel<g>, dim3(lzx_row_grid(wlen, LZX_TRUSS_BLOCK / g)), dim3(LZX_TRUSS_BLOCK), 0, st, p);
            });
            LZX_HIP(hipGetLastError());
            if (c->max_degree > long_row) {
                hipLaunchKernelGGL(k_truss_peel_long, dim3((wlen + LZX_TRUSS_BLOCK - 1) / LZX_TRUSS_BLOCK, slices), dim3(LZX_TRUSS_BLOCK), 0, st, p);
                LZX_HIP(hipGetLastError());
            }
            return LZX_OK;
        },
        &peel));
    LZX_HIP(hipEventRecord(run.ev1, st));

    // ---- hand back: one gather through eid per per-entry output (mark holds the layers), one row pass for the vertices ----
    if (nnz) {
        const std::pair<uint32_t *, const u32 *> outs[2] = {{truss, d_truss}, {layer, d_mark}};
        for (const auto &o : outs) {
            if (!o.first) continue;
            hipLaunchKernelGGL(k_truss_gather, dim3(gz), dim3(LZX_TRUSS_BLOCK), 0, st, d_eid, o.second, m, nnz, d_stage);
            LZX_HIP(hipGetLastError());
            LZX_HIP(hipMemcpyAsync(o.first, d_stage, sizeof(u32) * nnz, hipMemcpyDeviceToHost, st));
            LZX_HIP(hipStreamSynchronize(st));   // (the staging buffer is used again)
        }
    }
    if (vertex_truss && n) {
        u32 *d_vertex = d_deg;   // (the degrees are done with)
        lzx_with_lanes<64>(Go, [&](auto g) {
            hipLaunchKernelGGL(k_truss_vertex<g>, dim3(lzx_row_grid(n, LZX_TRUSS_BLOCK / g)), dim3(LZX_TRUSS_BLOCK), 0, st, c->d_row_ptr, d_eid, d_truss, n,
                               m, d_vertex);
        });
        LZX_HIP(hipGetLastError());
        LZX_HIP(hipMemcpyAsync(vertex_truss, d_vertex, sizeof(u32) * n, hipMemcpyDeviceToHost, st));
    }
    LZX_HIP(hipStreamSynchronize(st));
    float peel_ms = 0.f;
    LZX_HIP(hipEventElapsedTime(&peel_ms, run.ev0, run.ev1));
    if (info) {
        info->edges = m;
        info->triangles = sup_sum / 3;
        info->main_truss_edges = m ? (u64)m - peel.level_pos : 0;
        info->max_support = (u32)sup_max;
        info->max_truss = m ? peel.level + 2 : 0;
        info->levels = peel.levels;
        info->rounds = peel.rounds;
        info->loop_ms = lzx_ms_since(t0);
        info->support_ms = support_ms;
        info->peel_ms = peel_ms;
    }
    return LZX_OK;
}
