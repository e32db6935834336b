// lzx_pagerank.hip -- PageRank and personalised PageRank of the (undirected) graph for up to 16 damping factors at once by
// multi-shift conjugate gradients in the degree inner product: include/lzx.h, lzx_pagerank_f64; DESIGN.md section 15.
//
// d_i = stored entries of row i, w_i = max(d_i, 1), W = diag(w), P = D^(-1) A (zero rows where d_i = 0).  PageRank with damping
// delta, teleport vector v (>= 0, sum 1) and the dangling mass returned to v is x = y / sum(y) with (I - delta A W^(-1)) y = v.
// A W^(-1) = W P W^(-1), so y = (1 / delta) W z with (sigma I - P) z = b, sigma = 1 / delta > 1, b = W^(-1) v.  P is self-adjoint
// in <a, b>_W = sum w_i a_i b_i and sigma I - P is positive definite there: CG in that inner product on the seed (the largest
// delta = the smallest sigma), every other damping following through the recurrences of lzx_solve.hip (zeta, alpha_s, beta_s).
//
//   <p, P p>_W = p . (A p)        the SpMV's fused partials as they stand (rows with d_i = 0 have (A p)_i = 0)
//   (P p)_i    = (A p)_i / d_i    a per-row post-scale of the SpMV's output where it is read, 0 where d_i = 0
//
// Layout.  As in lzx_solve.hip: every vector in the internal vertex order with stride ldq (tail and padding rows 0, d = 0 and
// w = 1 there): b, r, p, z_0 (the seed), then z_s of dampings 1 .. nu-1, then their p_s.  The degrees are the handle's u32 array
// (lzx_ensure_degrees), read as uint2 beside the double2 of the vectors; 1 / d_i is formed in the kernel.
//
// The loop is the shifted solver's (lzx_cg_multishift, lzx_solve.hip) with its two kernels in their degree-weighted form.  One
// iteration j, no host synchronisation (the host reads the status every `poll` iterations):
//   SpMV                   t = A p, partials of p . A p
//   k_cg_update<true>      <p, S p>_W = sigma_0 sum w p^2 - p . A p closed, alpha_j; r -= alpha_j (sigma_0 p - t / d), z_0 += alpha_j p;
//                          partials of sum w r^2
//   k_cg_direction<true>   sum w r^2 closed, beta_j, zeta / alpha_s / beta_s, freeze rules; p = r + beta_j p (partials of sum w p^2);
//                          z_s += alpha_s p_s, p_s = zeta r + beta_s p_s per live damping
// This file keeps what is PageRank's own: the start b = W^(-1) v (k_pr_start), and y = sigma W z with its mass and L1 residual
// (k_pr_finish).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "lzx_internal.h"
#include "lzx_graph_call.h"
#include "lzx_spmv_body.h"
#include "lzx_reduce.h"

// b = (v / vsum) / w scattered into the internal order (v == nullptr: the uniform vector, nothing was uploaded), partials of
// ||b||_W^2 = sum w b^2.  One caller vertex per thread and grid stride; padding and tail rows keep the zeros of the memset.
__global__ void __launch_bounds__(LZX_VEC_BLOCK)
k_pr_start(const double *__restrict__ v, double vsum, double uniform, const u32 *__restrict__ gidx, const u32 *__restrict__ deg, double *b, u64 n,
           double *part)
{
    __shared__ double sh[4];
    double acc = 0.0;
    for (u64 o = (u64)blockIdx.x * LZX_VEC_BLOCK + threadIdx.x; o < n; o += (u64)gridDim.x * LZX_VEC_BLOCK) {
        const u32 g = gidx[o];
        const double w = lzx_deg_weight(deg[g]);
        const double x = (v ? v[o] / vsum : uniform) / w;
        b[g] = x;
        acc += w * (x * x);
    }
    block_partial(acc, sh, part);
}

// One damping after the loop, t = A z from one SpMV: y = sigma (w z) written over z; partials of sum y and of the true L1
// residual |v - (I - delta A W^(-1)) y| = |w b - y + t| (delta A W^(-1) y = A z).
__global__ void __launch_bounds__(LZX_VEC_BLOCK)
k_pr_finish(double *z, const double *__restrict__ t, const double *__restrict__ b, const u32 *__restrict__ deg, double sigma, u32 n, double *mass_part,
            double *res_part)
{
    __shared__ double sh[4];
    double mass = 0.0, res = 0.0;
    const u32 stride = gridDim.x * LZX_VEC_BLOCK * 2;
    for (u32 i = (blockIdx.x * LZX_VEC_BLOCK + threadIdx.x) * 2; i < n; i += stride) {
        double2 y = *reinterpret_cast<const double2 *>(z + i);
        const double2 tt = *reinterpret_cast<const double2 *>(t + i);
        const double2 bb = *reinterpret_cast<const double2 *>(b + i);
        const uint2 d = *reinterpret_cast<const uint2 *>(deg + i);
        const double wx = lzx_deg_weight(d.x), wy = lzx_deg_weight(d.y);
        y.x = sigma * (wx * y.x);
        y.y = sigma * (wy * y.y);
        *reinterpret_cast<double2 *>(z + i) = y;
        mass += y.x;
        mass += y.y;
        res += fabs(wx * bb.x - y.x + tt.x);
        res += fabs(wy * bb.y - y.y + tt.y);
    }
    block_partial(mass, sh, mass_part);
    __syncthreads();
    block_partial(res, sh, res_part);
}

// ==================================================================================================== host
extern "C" int lzx_pagerank_f64(lzx_handle h, const double *v, uint32_t nd, const double *damping, double tol, uint32_t maxiter, double *X,
                                uint32_t *iters, double *resid, lzx_pagerank_info *info)
{
    static const char *fn = "lzx_pagerank_f64";
    const auto t_start = std::chrono::steady_clock::now();
    if (nd == 0) LZX_FAIL(LZX_ERR_ARG, "%s: nd == 0", fn);
    if (nd > LZX_SOLVE_MAX_NS) LZX_FAIL(LZX_ERR_LIMIT, "%s: nd = %u damping factors (at most %u)", fn, nd, LZX_SOLVE_MAX_NS);
    if (!(tol > 0.0)) LZX_FAIL(LZX_ERR_ARG, "%s: tol must be > 0", fn);
    if (!damping) LZX_FAIL(LZX_ERR_ARG, "%s: null damping", fn);
    for (u32 s = 0; s < nd; ++s)
        if (!std::isfinite(damping[s]) || !(damping[s] > 0.0 && damping[s] < 1.0))
            LZX_FAIL(LZX_ERR_ARG, "%s: damping %u = %g is not in (0, 1)", fn, s, damping[s]);
    if (maxiter == 0) LZX_FAIL(LZX_ERR_ARG, "%s: maxiter == 0", fn);
    if (!h) LZX_FAIL(LZX_ERR_ARG, "%s: null handle (h)", fn);
    if (!X) LZX_FAIL(LZX_ERR_ARG, "%s: null X", fn);
    lzx_ctx *c = h;
    if (c->comm_kind != 0 || c->world > 1)
        LZX_FAIL(LZX_ERR_STATE, "%s: PageRank runs on one GPU handle; this handle is rank %d of a communicator of %d", fn, c->rank, c->world);
    if (!c->d_row_ptr || !c->d_v) LZX_FAIL(LZX_ERR_STATE, "%s: no graph has been handed over", fn);
    const u64 n = c->n;
    double vsum = 1.0;
    if (v) {
        vsum = 0.0;
        for (u64 i = 0; i < n; ++i) {
            if (!std::isfinite(v[i]) || v[i] < 0.0) LZX_FAIL(LZX_ERR_ARG, "%s: v[%llu] = %g is negative or not finite", fn, (unsigned long long)i, v[i]);
            vsum += v[i];
        }
        if (!(vsum > 0.0) || !std::isfinite(vsum)) LZX_FAIL(LZX_ERR_ARG, "%s: v sums to %g (a teleport vector needs a positive finite sum)", fn, vsum);
    }
    // distinct dampings descending: unique slot u of every caller damping; the seed (u = 0) is the largest, sigma_0 the smallest
    std::vector<u32> slot;
    const std::vector<double> uq = lzx_cg_distinct(damping, nd, true, slot);
    const u32 nu = (u32)uq.size();
    std::vector<double> sigma(nu);
    for (u32 u = 0; u < nu; ++u) sigma[u] = 1.0 / uq[u];
    const double sigma0 = sigma[0];

    LzxCgRun run;
    run.c = c;
    LZX_HIP(hipSetDevice(c->device));
    LZX_TRY(lzx_ensure_degrees(c));   // the handle's per-graph degree array (kept as long as the graph, as under operator L)
    // like lzx_spmv_f64: d_v / d_partials / d_io are overwritten, so a prepared decomposition is void (the resident basis, its
    // alpha / beta and the batch state are not touched)
    c->k_prep = 0;

    const u32 ncols = 2 + 2 * nu;
    const u64 state_bytes = (u64)ncols * c->ldq * sizeof(double);
    char what[64];
    std::snprintf(what, sizeof what, "the state of %u vectors (b, r, p, 2 per damping)", ncols);
    LZX_TRY(lzx_alloc_state(fn, what, c->solve_cap_opt, state_bytes, state_bytes, (void **)&run.d_V));
    auto col = [&](u32 i) { return run.d_V + (size_t)i * c->ldq; };
    double *vb = col(0), *vr = col(1), *vp = col(2), *vz0 = col(3), *vZ = col(4), *vP = col(3 + nu);

    const u32 G = lzx_cgs_grid(c);   // every kernel of this file: the grid of the shifted solver's loop
    const u32 st_words = (u32)((sizeof(CgState) + 7) / 8), mid_words = (u32)((sizeof(CgMid) + 7) / 8);
    const u64 scratch = 3ull * G + 64 + 2ull * st_words + mid_words;
    LZX_HIP(hipMalloc(reinterpret_cast<void **>(&run.d_s), sizeof(double) * scratch));
    double *bb_part = run.d_s, *rr_part = bb_part + G, *pp_part = rr_part + G, *tmp = pp_part + G;   // tmp[64]: ||b||_W^2, masses, residuals
    CgState *d_st = reinterpret_cast<CgState *>(tmp + 64);
    CgMid *d_mid = reinterpret_cast<CgMid *>(tmp + 64 + 2 * st_words);
    LZX_HIP(hipMemsetAsync(run.d_V, 0, state_bytes, c->stream));   // padding rows and tails stay 0 from here on
    LZX_HIP(hipMemsetAsync(run.d_s, 0, sizeof(double) * scratch, c->stream));

    if (v) LZX_HIP(hipMemcpyAsync(c->d_io, v, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_pr_start, dim3(G), dim3(LZX_VEC_BLOCK), 0, c->stream, v ? c->d_io : nullptr, vsum, 1.0 / (double)n, c->d_gidx_of_old, c->d_deg, vb, n,
                       bb_part);
    LZX_HIP(hipGetLastError());
    LZX_TRY(lzx_launch_reduce(c, bb_part, G, tmp, 0));
    double bb = 0.0;
    LZX_HIP(hipMemcpyAsync(&bb, tmp, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    LZX_HIP(hipStreamSynchronize(c->stream));
    if (!(bb > 0.0) || !std::isfinite(bb)) LZX_FAIL(LZX_ERR_ARG, "%s: ||W^(-1) v||_W^2 = %g (v underflows after the division by its sum)", fn, bb);
    const double bnorm = std::sqrt(bb);

    CgArgs a{};
    a.r = vr;
    a.p = vp;
    a.x0 = vz0;
    a.w = c->d_v;
    a.deg = c->d_deg;
    a.X = vZ;
    a.P = vP;
    a.ldq = c->ldq;
    a.n = c->n_loc_pad;
    a.ns = nu;
    a.sigma0 = sigma0;
    a.tolb = tol * bnorm;
    for (u32 u = 0; u < nu; ++u) a.delta[u] = sigma[u] - sigma0;
    a.pp = bb_part;
    a.npp = G;
    a.pm = c->d_partials;
    a.npm = lzx_spmv_partials(c);
    a.rr_part = rr_part;
    a.pp_part = pp_part;
    a.st = d_st;
    a.mid = d_mid;

    CgState hs;
    LzxCgLoop lp;
    LZX_TRY(lzx_cg_multishift(run, a, vb, bb, false, maxiter, hs, lp));
    const u32 launched = lp.launched;
    if (hs.done == 2)
        LZX_FAIL(LZX_ERR_ARG, "%s: <p, (sigma_0 I - P) p>_W = %.6e at iteration %u (sigma_0 = %.17g): the graph's matrix is not symmetric", fn, hs.curv,
                 hs.err_iter, sigma0);

    // every distinct damping: t = A z (one SpMV), y = sigma W z with its mass and true L1 residual, x = y / mass in the caller's order
    std::vector<u32> first(nu, nd);
    for (u32 s = 0; s < nd; ++s) first[slot[s]] = std::min(first[slot[s]], s);
    double *mass_part = rr_part, *res_part = pp_part;   // the loop's partials are dead
    for (u32 u = 0; u < nu; ++u) {
        double *z = u == 0 ? vz0 : vZ + (size_t)(u - 1) * c->ldq;
        SpmvLaunch l{z, z, c->d_v, c->d_partials};
        LZX_TRY(lzx_launch_spmv(c, l));
        hipLaunchKernelGGL(k_pr_finish, dim3(G), dim3(LZX_VEC_BLOCK), 0, c->stream, z, c->d_v, vb, c->d_deg, sigma[u], c->n_loc_pad, mass_part, res_part);
        LZX_HIP(hipGetLastError());
        LZX_TRY(lzx_launch_reduce(c, mass_part, G, tmp + 16 + u, 0));
        LZX_TRY(lzx_launch_reduce(c, res_part, G, tmp + 32 + u, 0));
        LZX_TRY(lzx_launch_permute_out(c, z, c->d_io, tmp + 16 + u));
        LZX_HIP(hipMemcpyAsync(X + (size_t)first[u] * n, c->d_io, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    }
    double ms[2 * LZX_SOLVE_MAX_NS];   // masses at [0, 16), residuals at [16, 32)
    LZX_HIP(hipMemcpyAsync(ms, tmp + 16, sizeof(ms), hipMemcpyDeviceToHost, c->stream));
    LZX_HIP(hipStreamSynchronize(c->stream));
    u32 conv = 0, last = 0;
    for (u32 s = 0; s < nd; ++s) {
        const u32 u = slot[s];
        const bool ok = !((hs.live >> u) & 1u);
        if (s != first[u]) std::memcpy(X + (size_t)s * n, X + (size_t)first[u] * n, sizeof(double) * n);
        if (iters) iters[s] = ok ? hs.iters[u] : launched;
        if (resid) resid[s] = ms[LZX_SOLVE_MAX_NS + u];   // ||v||_1 = 1: v was divided by its sum
        conv += ok;
        if (ok) last = std::max(last, hs.iters[u]);
    }
    if (info) {
        info->iterations = conv == nd ? last : launched;
        info->launched = launched;
        info->converged = conv;
        info->nd = nd;
        info->loop_ms = lzx_ms_since(t_start);
        info->spmv_ms = lp.spmv_ms;
        info->vec_ms = lp.vec_ms;
        for (u32 s = 0; s < LZX_SOLVE_MAX_NS; ++s) info->mass[s] = s < nd ? ms[slot[s]] : 0.0;
    }
    if (conv < nd)
        LZX_FAIL(LZX_ERR_LIMIT, "%s: %u of %u damping factors converged in maxiter = %u iterations (tolerance %.3e of ||W^(-1) v||_W = %.6e)", fn, conv, nd,
                 maxiter, tol, bnorm);
    return LZX_OK;
}
