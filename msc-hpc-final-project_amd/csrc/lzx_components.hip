// lzx_components.hip -- connected components of the handle's graph and induced subgraphs, both on the device over the
// caller-order CSR the handle keeps (d_row_ptr / d_col_idx): include/lzx.h, lzx_components and lzx_set_graph_induced;
// DESIGN.md section 14.
//
// Components.  Three u32 arrays of n: f (the parent of every vertex, f[v] <= v, starts as v), gf = f[f] and fn, the parents
// of the NEXT round (equal to f between rounds).  One round:
//   sweep  k_cc_sweep (+ k_cc_sweep_long)   per row u: m = min(gf[u], min over the neighbours v of gf[v]) -- the pull form, a
//                                           group of G lanes per row (rows of more than 64 G entries: a whole workgroup) --
//                                           then fn[u] = min(fn[u], m) and fn[f[u]] = min(fn[f[u]], m): u and its parent hook
//                                           onto the smallest grandparent around u (FastSV's two hookings)
//   jump   k_cc_jump                        f = fn, gf = fn[fn]
// The sweep reads f and gf only and every write is a 32-bit vector atomicMin into fn, issued only where it lowers something
// (at most two per ROW, none per entry), so fn after a round does not depend on the order in which they land: labels, round
// counts and everything else are the same from run to run, and equal tests/test_components_host.py's numpy restatement.  The
// host reads one "changed" word per round.  Labels only decrease and stay inside the component; a round that lowers nothing has
// f[f] = f and f equal across every edge, which (the matrix is symmetric) makes f the component's smallest id.
// Counting: components = vertices with f[v] = v, counted in block partials closed by block_sum_fixed_256; sizes = a u32
// histogram on the roots (a wavefront adds the lanes that share its first lane's root with one atomic); the largest
// component is the maximum of size << 32 | ~root over the roots, so ties go to the smallest label.
//
// Induced subgraph: new_of_old = exclusive scan of the keep flags, one wavefront per kept row counts / writes the kept
// neighbours in their order (the map is monotone: columns stay ascending), the counts are scanned into the row pointers, and
// the result takes the place of dst's CSR in front of the same lzx_graph_prepare every hand-over ends in.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <vector>

#include "lzx_internal.h"
#include "lzx_graph_call.h"
#include "lzx_spmv_body.h"
#include "lzx_reduce.h"

static constexpr u32 LZX_CC_BLOCK = 256;
static constexpr u32 LZX_CC_STAT_GRID = 1024;   // block partials of the counting pass (at most)

// u and its parent hook onto m, the smallest grandparent seen from row u (gf[u] included)
__device__ __forceinline__ void cc_hook(u32 u, u32 m, const u32 *f, const u32 *gf, u32 *fn, u32 *changed)
{
    const u32 p = f[u];
    m = min(m, gf[u]);
    bool ch = false;
    if (m < p) { atomicMin(&fn[u], m); ch = true; }
    if (p != u && m < f[p]) { atomicMin(&fn[p], m); ch = true; }
    if (ch) changed[0] = 1u;
}

// rows of at most long_row entries: G lanes per row, 256 / G rows per workgroup
template <u32 G>
__global__ void __launch_bounds__(LZX_CC_BLOCK)
k_cc_sweep(const u64 *row_ptr, const u32 *col_idx, const u32 *f, const u32 *gf, u32 *fn, u32 *changed, u32 n, u32 long_row)
{
    const u32 sub = threadIdx.x & (G - 1);
    const u64 row = (u64)blockIdx.x * (LZX_CC_BLOCK / G) + threadIdx.x / G;
    u64 beg = 0, end = 0;
    if (row < n) {
        beg = row_ptr[row];
        end = row_ptr[row + 1];
        if (end - beg > long_row) end = beg;   // k_cc_sweep_long's
    }
    u32 m = 0xffffffffu;
#pragma unroll 4
    for (u64 e = beg + sub; e < end; e += G) m = min(m, gf[col_idx[e]]);
#pragma unroll
    for (u32 o = G / 2; o > 0; o >>= 1) m = min(m, (u32)__shfl_xor((int)m, (int)o, 64));
    if (sub == 0 && end > beg) cc_hook((u32)row, m, f, gf, fn, changed);
}

// rows of more than long_row entries among the workgroup's 256 rows: the whole workgroup per row
__global__ void __launch_bounds__(LZX_CC_BLOCK)
k_cc_sweep_long(const u64 *row_ptr, const u32 *col_idx, const u32 *f, const u32 *gf, u32 *fn, u32 *changed, u32 n, u32 long_row)
{
    __shared__ u32 s_rows[LZX_CC_BLOCK];
    __shared__ u32 s_count;
    __shared__ u32 s_min[LZX_CC_BLOCK / 64];
    const u64 mine = (u64)blockIdx.x * LZX_CC_BLOCK + threadIdx.x;
    const u32 count = lzx_collect_long_rows(mine < n && row_ptr[mine + 1] - row_ptr[mine] > long_row, (u32)mine, s_rows, &s_count);
    for (u32 r = 0; r < count; ++r) {
        const u32 row = s_rows[r];
        const u64 beg = row_ptr[row], end = row_ptr[row + 1];
        u32 m = 0xffffffffu;
#pragma unroll 4
        for (u64 e = beg + threadIdx.x; e < end; e += LZX_CC_BLOCK) m = min(m, gf[col_idx[e]]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = min(m, (u32)__shfl_xor((int)m, o, 64));
        if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) cc_hook(row, min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3])), f, gf, fn, changed);
        __syncthreads();
    }
}

__global__ void k_cc_init(u32 *f, u32 *gf, u32 *fn, u32 *sizes, u32 *changed, u32 n)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        f[i] = gf[i] = fn[i] = (u32)i;
        sizes[i] = 0;
    }
    if (i == 0) changed[0] = 0;
}

__global__ void k_cc_jump(const u32 *fn, u32 *f, u32 *gf, u32 *changed, u32 n)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const u32 a = fn[i];
        f[i] = a;
        gf[i] = fn[a];
    }
    if (i == 0) changed[0] = 0;
}

// sizes[root] = vertices below the root (the root itself is added where the sizes are read)
__global__ void __launch_bounds__(LZX_CC_BLOCK)
k_cc_sizes(const u32 *f, u32 *sizes, u32 n)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 r = i < n ? f[i] : 0u;
    const bool child = i < n && r != (u32)i;
    const unsigned long long todo = __ballot(child);
    if (todo == 0) return;
    const u32 leader = (u32)__builtin_ctzll(todo);
    const u32 r0 = (u32)__shfl((int)r, (int)leader, 64);
    const unsigned long long same = __ballot(child && r == r0);
    if ((threadIdx.x & 63) == leader) atomicAdd(&sizes[r0], (u32)__builtin_popcountll(same));
    else if (child && r != r0) atomicAdd(&sizes[r], 1u);
}

// block partials: roots (as a double, exact) and the largest size << 32 | ~root
__global__ void __launch_bounds__(LZX_CC_BLOCK)
k_cc_stats(const u32 *f, const u32 *sizes, u32 n, double *part_count, unsigned long long *part_key)
{
    __shared__ double s_c[LZX_CC_BLOCK / 64];
    __shared__ unsigned long long s_k[LZX_CC_BLOCK / 64];
    double cnt = 0.0;
    unsigned long long key = 0;
    for (u64 i = (u64)blockIdx.x * LZX_CC_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * LZX_CC_BLOCK)
        if (f[i] == (u32)i) {
            cnt += 1.0;
            const unsigned long long k = ((unsigned long long)(sizes[i] + 1u) << 32) | (0xffffffffu - (u32)i);
            key = k > key ? k : key;
        }
    cnt = wave_sum(cnt);
    key = wave_max_u64(key);
    if ((threadIdx.x & 63) == 0) { s_c[threadIdx.x >> 6] = cnt; s_k[threadIdx.x >> 6] = key; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part_count[blockIdx.x] = ((s_c[0] + s_c[1]) + s_c[2]) + s_c[3];
        part_key[blockIdx.x] = block_max_u64(s_k);
    }
}

__global__ void __launch_bounds__(LZX_VEC_BLOCK)
k_cc_close(const double *part_count, const unsigned long long *part_key, u32 np, unsigned long long *out2)
{
    __shared__ double sh[4];
    __shared__ unsigned long long s_k[LZX_VEC_BLOCK / 64];
    const double total = block_sum_fixed_256(part_count, np, sh);
    unsigned long long key = 0;
    for (u32 i = threadIdx.x; i < np; i += LZX_VEC_BLOCK) key = part_key[i] > key ? part_key[i] : key;
    key = wave_max_u64(key);
    if ((threadIdx.x & 63) == 0) s_k[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        out2[1] = block_max_u64(s_k);
        out2[0] = (unsigned long long)total;
    }
}

extern "C" int lzx_components(lzx_handle c, uint32_t *labels, lzx_components_info *info)
{
    const char *fn_name = "lzx_components";
    LZX_TRY(lzx_graph_call_check(c, fn_name, "components are labelled"));
    LZX_HIP(hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    const u32 n = (u32)c->n;
    hipStream_t st = c->stream;

    const u32 np = (u32)std::min<u64>(LZX_CC_STAT_GRID, ((u64)n + LZX_CC_BLOCK - 1) / LZX_CC_BLOCK);   // the counting pass's partials
    u32 *d_f, *d_gf, *d_fn, *d_sizes, *d_changed;
    double *d_pc;
    unsigned long long *d_pk, *d_out;
    LzxGraphRun run(c);
    char what[96];
    std::snprintf(what, sizeof what, "the state of %u vertices (parents, grandparents, next parents, sizes)", n);
    LZX_TRY(lzx_carve_state(fn_name, what, -1, 0, &run.arena, nullptr, [&](LzxCarver &k) {
        for (u32 **p : {&d_f, &d_gf, &d_fn, &d_sizes}) k.take(*p, lzx_even(n));
        k.take(d_pc, np);
        k.take(d_pk, np);
        k.take(d_out, 2);
        k.take(d_changed, 2);   // (the flag, in a word of eight bytes)
    }));
    LZX_TRY(run.events(2));

    // lanes per row: about half the mean degree of the rows that have an edge, so that a typical row is two loads per lane
    const u32 G = lzx_lanes_per_row(c, c->nnz, 32);
    const u32 long_row = 64 * G;
    const u32 gb = (n + LZX_CC_BLOCK - 1) / LZX_CC_BLOCK;

    hipLaunchKernelGGL(k_cc_init, dim3(gb), dim3(LZX_CC_BLOCK), 0, st, d_f, d_gf, d_fn, d_sizes, d_changed, n);
    LZX_HIP(hipGetLastError());
    u32 rounds = 0;
    double sweep_ms = 0.0;
    for (;;) {
        if (rounds > n) LZX_FAIL(LZX_ERR_LIMIT, "%s: no fixed point after %u rounds on %u vertices", fn_name, rounds, n);
        LZX_HIP(hipEventRecord(run.ev0, st));
        lzx_with_lanes<32>(G, [&](auto g) {
            hipLaunchKernelGGL(k_cc_sweep<g>, dim3(lzx_row_grid(n, LZX_CC_BLOCK / g)), dim3(LZX_CC_BLOCK), 0, st, c->d_row_ptr, c->d_col_idx, d_f, d_gf,
                               d_fn, d_changed, n, long_row);
        });
        LZX_HIP(hipGetLastError());
        if (c->max_degree > long_row) {
            hipLaunchKernelGGL(k_cc_sweep_long, dim3(gb), dim3(LZX_CC_BLOCK), 0, st, c->d_row_ptr, c->d_col_idx, d_f, d_gf, d_fn, d_changed, n, long_row);
            LZX_HIP(hipGetLastError());
        }
        LZX_HIP(hipEventRecord(run.ev1, st));
        u32 changed = 0;
        LZX_HIP(hipMemcpyAsync(&changed, d_changed, sizeof(u32), hipMemcpyDeviceToHost, st));
        LZX_HIP(hipStreamSynchronize(st));
        float ms = 0.f;
        LZX_HIP(hipEventElapsedTime(&ms, run.ev0, run.ev1));
        sweep_ms += ms;
        ++rounds;
        if (!changed) break;
        hipLaunchKernelGGL(k_cc_jump, dim3(gb), dim3(LZX_CC_BLOCK), 0, st, d_fn, d_f, d_gf, d_changed, n);
        LZX_HIP(hipGetLastError());
    }

    hipLaunchKernelGGL(k_cc_sizes, dim3(gb), dim3(LZX_CC_BLOCK), 0, st, d_f, d_sizes, n);
    LZX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cc_stats, dim3(np), dim3(LZX_CC_BLOCK), 0, st, d_f, d_sizes, n, d_pc, d_pk);
    LZX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cc_close, dim3(1), dim3(LZX_VEC_BLOCK), 0, st, d_pc, d_pk, np, d_out);
    LZX_HIP(hipGetLastError());
    unsigned long long out2[2] = {0, 0};
    LZX_HIP(hipMemcpyAsync(out2, d_out, sizeof(out2), hipMemcpyDeviceToHost, st));
    if (labels) LZX_HIP(hipMemcpyAsync(labels, d_f, sizeof(u32) * n, hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    if (info) {
        info->n_components = out2[0];
        info->largest_size = out2[1] >> 32;
        info->largest_label = 0xffffffffu - (u32)(out2[1] & 0xffffffffull);
        info->rounds = rounds;
        info->sweep_ms = sweep_ms;
        info->loop_ms = lzx_ms_since(t0);
    }
    return LZX_OK;
}

// ---- induced subgraph ----------------------------------------------------------------------------------------------------
__global__ void k_ind_flags(const uint8_t *keep, u32 *flag, u32 n)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) flag[i] = (i < n && keep[i]) ? 1u : 0u;
}

// One wavefront per kept row (strided over the grid): its kept neighbours, counted (cols_out == nullptr: count[new row], and
// count[n_new] = 0) or written in their order behind row_ptr_new[new row] under their new ids.
__global__ void __launch_bounds__(LZX_CC_BLOCK)
k_ind_rows(const u64 *row_ptr, const u32 *col_idx, const uint8_t *keep, const u32 *new_of_old, u32 n, u32 n_new,
           u64 *count, const u64 *row_ptr_new, u32 *cols_out)
{
    const u32 lane = threadIdx.x & 63;
    const u64 waves = (u64)gridDim.x * (LZX_CC_BLOCK / 64);
    const u64 wave0 = (u64)blockIdx.x * (LZX_CC_BLOCK / 64) + (threadIdx.x >> 6);
    if (!cols_out && wave0 == 0 && lane == 0) count[n_new] = 0;
    for (u64 row = wave0; row < n; row += waves) {
        if (!keep[row]) continue;   // wave-uniform
        const u32 nr = new_of_old[row];
        const u64 beg = row_ptr[row], end = row_ptr[row + 1];
        const u64 out0 = cols_out ? row_ptr_new[nr] : 0;
        u64 kept = 0;
        for (u64 e0 = beg; e0 < end; e0 += 64) {
            const u64 e = e0 + lane;
            const u32 col = e < end ? col_idx[e] : 0u;
            const bool k = e < end && keep[col];
            const unsigned long long m = __ballot(k);
            if (cols_out && k) cols_out[out0 + kept + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = new_of_old[col];
            kept += (u64)__builtin_popcountll(m);
        }
        if (!cols_out && lane == 0) count[nr] = kept;
    }
}

namespace {
struct IndRun {
    uint8_t *d_keep = nullptr;
    u32 *d_flag = nullptr, *d_new = nullptr, *d_ci = nullptr;
    u64 *d_count = nullptr, *d_rp = nullptr;
    void *d_tmp = nullptr;
    ~IndRun()
    {
        for (void *p : {(void *)d_keep, (void *)d_flag, (void *)d_new, (void *)d_ci, (void *)d_count, (void *)d_rp, d_tmp})
            if (p) (void)hipFree(p);
    }
};
}   // namespace

extern "C" int lzx_set_graph_induced(lzx_handle dst, lzx_handle src, const uint8_t *keep, uint32_t *old_of_new, uint64_t *n_new_out)
{
    const char *fn_name = "lzx_set_graph_induced";
    if (!dst || !src || !keep) LZX_FAIL(LZX_ERR_ARG, "%s: null %s", fn_name, !dst ? "destination handle" : !src ? "source handle" : "keep mask");
    for (const lzx_ctx *c : {(const lzx_ctx *)dst, (const lzx_ctx *)src})
        if (c->comm_kind != 0 || c->world > 1)
            LZX_FAIL(LZX_ERR_STATE, "%s: subgraphs are built on one GPU handle; the %s handle is rank %d of a communicator of %d", fn_name,
                     c == dst ? "destination" : "source", c->rank, c->world);
    if (!src->d_row_ptr) LZX_FAIL(LZX_ERR_STATE, "%s: no graph has been handed over to the source handle", fn_name);
    if (src->sharded) LZX_FAIL(LZX_ERR_STATE, "%s: the source's graph came through the sharded hand-over -- no rank holds all of it", fn_name);
    if (src->device != dst->device)
        LZX_FAIL(LZX_ERR_ARG, "%s: both handles must be on the same GPU; the source is on device %d, the destination on device %d", fn_name, src->device, dst->device);
    const u32 n = (u32)src->n;
    u64 n_new = 0;
    for (u32 i = 0; i < n; ++i) n_new += keep[i] != 0;
    if (n_new == 0) LZX_FAIL(LZX_ERR_ARG, "%s: the mask keeps none of the %u vertices", fn_name, n);
    LZX_HIP(hipSetDevice(src->device));
    hipStream_t st = src->stream;

    IndRun run;
    LZX_HIP(hipMalloc(reinterpret_cast<void **>(&run.d_keep), n));
    LZX_HIP(hipMalloc(reinterpret_cast<void **>(&run.d_flag), sizeof(u32) * ((u64)n + 1)));
    LZX_HIP(hipMalloc(reinterpret_cast<void **>(&run.d_new), sizeof(u32) * ((u64)n + 1)));
    LZX_HIP(hipMalloc(reinterpret_cast<void **>(&run.d_count), sizeof(u64) * (n_new + 1)));
    LZX_HIP(hipMalloc(reinterpret_cast<void **>(&run.d_rp), sizeof(u64) * (n_new + 1)));
    LZX_HIP(hipMemcpyAsync(run.d_keep, keep, n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_ind_flags, dim3((u32)(((u64)n + 1 + 255) / 256)), dim3(256), 0, st, run.d_keep, run.d_flag, n);
    LZX_HIP(hipGetLastError());
    size_t tb1 = 0, tb2 = 0;
    LZX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb1, run.d_flag, run.d_new, (int)(n + 1), st));
    LZX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, run.d_count, run.d_rp, (int)(n_new + 1), st));
    const size_t tb = std::max<size_t>(std::max(tb1, tb2), 16);
    LZX_HIP(hipMalloc(&run.d_tmp, tb));
    size_t t = tb;
    LZX_HIP(hipcub::DeviceScan::ExclusiveSum(run.d_tmp, t, run.d_flag, run.d_new, (int)(n + 1), st));
    const u32 grid = (u32)std::min<u64>(((u64)n + LZX_CC_BLOCK / 64 - 1) / (LZX_CC_BLOCK / 64), (u64)src->cu_count * 32);
    hipLaunchKernelGGL(k_ind_rows, dim3(grid), dim3(LZX_CC_BLOCK), 0, st, src->d_row_ptr, src->d_col_idx, run.d_keep, run.d_new, n, (u32)n_new,
                       run.d_count, (const u64 *)nullptr, (u32 *)nullptr);
    LZX_HIP(hipGetLastError());
    t = tb;
    LZX_HIP(hipcub::DeviceScan::ExclusiveSum(run.d_tmp, t, run.d_count, run.d_rp, (int)(n_new + 1), st));
    u64 nnz_new = 0;
    LZX_HIP(hipMemcpyAsync(&nnz_new, run.d_rp + n_new, sizeof(u64), hipMemcpyDeviceToHost, st));
    LZX_HIP(hipStreamSynchronize(st));
    LZX_HIP(hipMalloc(reinterpret_cast<void **>(&run.d_ci), sizeof(u32) * std::max<u64>(nnz_new, 1)));
    if (nnz_new) {
        hipLaunchKernelGGL(k_ind_rows, dim3(grid), dim3(LZX_CC_BLOCK), 0, st, src->d_row_ptr, src->d_col_idx, run.d_keep, run.d_new, n, (u32)n_new,
                           (u64 *)nullptr, (const u64 *)run.d_rp, run.d_ci);
        LZX_HIP(hipGetLastError());
    }
    LZX_HIP(hipStreamSynchronize(st));

    // from here on dst is a hand-over like any other
    if (old_of_new)
        for (u32 i = 0, j = 0; i < n; ++i)
            if (keep[i]) old_of_new[j++] = i;
    if (n_new_out) *n_new_out = n_new;
    if (dst->shard_opt > 0) {   // option sharded_ingest streams a CSR in HOST memory: give it one (the one case in which the subgraph crosses PCIe)
        std::vector<u64> rp(n_new + 1);
        std::vector<u32> ci(std::max<u64>(nnz_new, 1));
        LZX_HIP(hipMemcpy(rp.data(), run.d_rp, sizeof(u64) * (n_new + 1), hipMemcpyDeviceToHost));
        if (nnz_new) LZX_HIP(hipMemcpy(ci.data(), run.d_ci, sizeof(u32) * nnz_new, hipMemcpyDeviceToHost));
        return lzx_set_graph_csr(dst, n_new, nnz_new, rp.data(), ci.data());
    }
    lzx_graph_release(dst);   // (dst == src: the old CSR goes here, after its last reader)
    dst->n = n_new;
    dst->nnz = nnz_new;
    dst->d_row_ptr = run.d_rp;
    dst->d_col_idx = run.d_ci;
    run.d_rp = nullptr;
    run.d_ci = nullptr;
    return lzx_graph_prepare(dst);
}
