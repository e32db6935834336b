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
// One iteration j, no host synchronisation (the host reads the status every `poll` iterations):
//   SpMV                 t = A p, partials of p . A p
//   k_pr_update          <p, S p>_W = sigma_0 sum w p^2 - p . A p closed, alpha_j; r -= alpha_j (sigma_0 p - t / d), z_0 += alpha_j p;
//                        partials of sum w r^2
//   k_pr_direction       sum w r^2 closed, beta_j, zeta / alpha_s / beta_s, freeze rules; p = r + beta_j p (partials of sum w p^2);
//                        z_s += alpha_s p_s, p_s = zeta r + beta_s p_s per live damping
// Every sum is closed in every workgroup with block_sum_fixed_256 (no atomics, no grid barrier): runs are bit-identical.  The
// scalars of the iteration are kept in two device copies by iteration parity, as in lzx_solve.hip.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <functional>
#include <vector>

#include "lzx_internal.h"
#include "lzx_spmv_body.h"
#include "lzx_reduce.h"

static constexpr u32 LZX_PR_MAX_ND = 16;
static constexpr u32 LZX_PR_POLL = 16;

namespace {
struct PrState {
    double rr;                  // <r_j, r_j>_W
    double alpha_prev, beta_prev;   // alpha_{j-1}, beta_{j-1} of the seed (1 and 0 at j = 0)
    double curv;                // done == 2: <p, S p>_W of the iteration that failed
    double zeta[LZX_PR_MAX_ND];       // zeta_{s,j} (slot 0, the seed: 1)
    double zeta_prev[LZX_PR_MAX_ND];  // zeta_{s,j-1}
    u32 live;                   // bit s: z_s (and p_s) are still written
    u32 done;                   // 0 running, 1 every damping frozen, 2 the curvature was not positive (A is not symmetric)
    u32 err_iter;               // done == 2: the iteration
    u32 iters[LZX_PR_MAX_ND];   // the iteration count at which damping s froze
};
struct PrMid {                  // k_pr_update (workgroup 0) -> k_pr_direction of the same iteration
    double alpha, curv;
    u32 err;
};
struct PrArgs {
    double *r, *p, *z0;         // the seed's vectors
    const double *t;            // A p (the SpMV's output)
    const u32 *deg;             // d_i, internal order (0 on padding and tail)
    double *Z, *P;              // z_s, p_s of damping s >= 1 at (s - 1) * ldq
    u32 ldq, n;                 // n: rows streamed (n_loc_pad, even)
    u32 nd;                     // distinct dampings
    double sigma0;              // 1 / the largest damping
    double tolb;                // tol ||b||_W
    double delta[LZX_PR_MAX_ND];   // sigma_s - sigma_0
    const double *pp;           // partials of sum w p^2 (k_pr_direction of the previous iteration, or of ||b||_W^2 from k_pr_start)
    u32 npp;
    const double *pm;           // partials of p . A p (the SpMV)
    u32 npm;
    double *rr_part, *pp_part;  // [gridDim.x] written by k_pr_update / k_pr_direction
    PrState *st;                // [2]
    PrMid *mid;
};
}  // namespace

// o = s word by word (a struct copy through registers would be indexed dynamically: scratch)
static __device__ __forceinline__ void pr_copy_state(PrState &o, const PrState &s)
{
    static_assert(sizeof(PrState) % 8 == 0, "PrState is copied as 8-byte words");
    const u64 *src = reinterpret_cast<const u64 *>(&s);
    u64 *dst = reinterpret_cast<u64 *>(&o);
    for (u32 i = 0; i < sizeof(PrState) / 8; ++i) dst[i] = src[i];
}

static __device__ __forceinline__ void pr_block_partial(double s, double *sh, double *out)
{
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

static __device__ __forceinline__ double pr_weight(u32 d) { return d ? (double)d : 1.0; }

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
        const double w = pr_weight(deg[g]);
        const double x = (v ? v[o] / vsum : uniform) / w;
        b[g] = x;
        acc += w * (x * x);
    }
    pr_block_partial(acc, sh, part);
}

// <p, S p>_W closed, alpha_j = <r, r>_W / <p, S p>_W; not positive (or not finite): the error is recorded, nothing written.
// r -= alpha_j (sigma_0 p - t / d) (the quotient is 0 where d = 0), z_0 += alpha_j p while the seed is live; partials of sum w r^2.
__global__ void __launch_bounds__(LZX_VEC_BLOCK) k_pr_update(PrArgs a, u32 j)
{
    __shared__ double sh[4];
    const PrState &s = a.st[j & 1];
    if (s.done) return;
    const double pp = block_sum_fixed_256(a.pp, a.npp, sh);
    const double pm = block_sum_fixed_256(a.pm, a.npm, sh);
    const double curv = a.sigma0 * pp - pm;
    const bool bad = !(curv > 0.0) || !isfinite(curv);
    const double alpha = s.rr / curv;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.mid->alpha = alpha;
        a.mid->curv = curv;
        a.mid->err = bad ? 1u : 0u;
    }
    if (bad) return;
    const bool seed = s.live & 1u;
    double acc = 0.0;
    const u32 stride = gridDim.x * LZX_VEC_BLOCK * 2;
    for (u32 i = (blockIdx.x * LZX_VEC_BLOCK + threadIdx.x) * 2; i < a.n; i += stride) {
        const double2 p = *reinterpret_cast<const double2 *>(a.p + i);
        const double2 t = *reinterpret_cast<const double2 *>(a.t + i);
        const uint2 d = *reinterpret_cast<const uint2 *>(a.deg + i);
        double2 r = *reinterpret_cast<const double2 *>(a.r + i);
        const double qx = d.x ? t.x / (double)d.x : 0.0, qy = d.y ? t.y / (double)d.y : 0.0;
        r.x -= alpha * (a.sigma0 * p.x - qx);
        r.y -= alpha * (a.sigma0 * p.y - qy);
        *reinterpret_cast<double2 *>(a.r + i) = r;
        if (seed) {
            double2 z = *reinterpret_cast<const double2 *>(a.z0 + i);
            z.x += alpha * p.x;
            z.y += alpha * p.y;
            *reinterpret_cast<double2 *>(a.z0 + i) = z;
        }
        acc += pr_weight(d.x) * (r.x * r.x);
        acc += pr_weight(d.y) * (r.y * r.y);
    }
    pr_block_partial(acc, sh, a.rr_part);
}

// sum w r^2 closed, beta_j; per damping zeta_{j+1}, alpha_s, beta_s and the freeze rule |zeta_{s,j+1}| ||r_{j+1}||_W <= tol ||b||_W
// (the seed: ||r_{j+1}||_W <= tol ||b||_W), the same in every workgroup; workgroup 0 writes the next state.  p = r + beta_j p
// (partials of sum w p^2); for each damping s >= 1 live at entry: z_s += alpha_s p_s, and p_s = zeta r + beta_s p_s unless it
// froze just now.
__global__ void __launch_bounds__(LZX_VEC_BLOCK) k_pr_direction(PrArgs a, u32 j)
{
    __shared__ double sh[4];
    __shared__ double sc[3][LZX_PR_MAX_ND];   // alpha_s, zeta_{s,j+1}, beta_s
    __shared__ u32 keep[LZX_PR_MAX_ND];       // damping s >= 1 stays live after this iteration
    const PrState &s = a.st[j & 1];
    PrState &o = a.st[(j + 1) & 1];
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    if (s.done) {
        if (writer) pr_copy_state(o, s);
        return;
    }
    const PrMid m = *a.mid;
    if (m.err) {
        if (writer) {
            pr_copy_state(o, s);
            o.live = 0;
            o.done = 2;
            o.err_iter = j;
            o.curv = m.curv;
        }
        return;
    }
    const double rr = block_sum_fixed_256(a.rr_part, gridDim.x, sh);
    const double beta = rr / s.rr, rn = sqrt(rr), alpha = m.alpha;
    const u32 live = s.live;
    const u32 t = threadIdx.x;
    if (t >= 1 && t < a.nd) {
        const double z = s.zeta[t], zp = s.zeta_prev[t];
        const double zn = z * zp * s.alpha_prev / (alpha * s.beta_prev * (zp - z) + zp * s.alpha_prev * (1.0 + a.delta[t] * alpha));
        const double q = zn / z;
        sc[0][t] = alpha * q;
        sc[1][t] = zn;
        sc[2][t] = q * q * beta;
        keep[t] = ((live >> t) & 1u) && !(fabs(zn) * rn <= a.tolb);
    }
    __syncthreads();
    if (writer) {
        u32 nl = (live & 1u) && !(rn <= a.tolb) ? 1u : 0u;
        for (u32 u = 1; u < a.nd; ++u) nl |= keep[u] << u;
        pr_copy_state(o, s);
        o.rr = rr;
        o.alpha_prev = alpha;
        o.beta_prev = beta;
        for (u32 u = 1; u < a.nd; ++u)
            if ((live >> u) & 1u) {
                o.zeta_prev[u] = s.zeta[u];
                o.zeta[u] = sc[1][u];
            }
        for (u32 u = 0; u < a.nd; ++u)
            if (((live >> u) & 1u) && !((nl >> u) & 1u)) o.iters[u] = j + 1;
        o.live = nl;
        o.done = nl == 0 ? 1u : 0u;
    }
    double acc = 0.0;
    const u32 stride = gridDim.x * LZX_VEC_BLOCK * 2;
    for (u32 i = (blockIdx.x * LZX_VEC_BLOCK + threadIdx.x) * 2; i < a.n; i += stride) {
        const double2 r = *reinterpret_cast<const double2 *>(a.r + i);
        const uint2 d = *reinterpret_cast<const uint2 *>(a.deg + i);
        double2 p = *reinterpret_cast<const double2 *>(a.p + i);
        p.x = r.x + beta * p.x;
        p.y = r.y + beta * p.y;
        *reinterpret_cast<double2 *>(a.p + i) = p;
        acc += pr_weight(d.x) * (p.x * p.x);
        acc += pr_weight(d.y) * (p.y * p.y);
        for (u32 u = 1; u < a.nd; ++u) {
            if (!((live >> u) & 1u)) continue;
            double *zs = a.Z + (size_t)(u - 1) * a.ldq + i, *ps = a.P + (size_t)(u - 1) * a.ldq + i;
            double2 z = *reinterpret_cast<const double2 *>(zs);
            double2 q = *reinterpret_cast<const double2 *>(ps);
            const double as = sc[0][u];
            z.x += as * q.x;
            z.y += as * q.y;
            *reinterpret_cast<double2 *>(zs) = z;
            if (keep[u]) {
                const double zn = sc[1][u], bs = sc[2][u];
                q.x = zn * r.x + bs * q.x;
                q.y = zn * r.y + bs * q.y;
                *reinterpret_cast<double2 *>(ps) = q;
            }
        }
    }
    pr_block_partial(acc, sh, a.pp_part);
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
        const double wx = pr_weight(d.x), wy = pr_weight(d.y);
        y.x = sigma * (wx * y.x);
        y.y = sigma * (wy * y.y);
        *reinterpret_cast<double2 *>(z + i) = y;
        mass += y.x;
        mass += y.y;
        res += fabs(wx * bb.x - y.x + tt.x);
        res += fabs(wy * bb.y - y.y + tt.y);
    }
    pr_block_partial(mass, sh, mass_part);
    __syncthreads();
    pr_block_partial(res, sh, res_part);
}

// ==================================================================================================== host
namespace {
struct PrRun {
    lzx_ctx *c = nullptr;
    double *d_V = nullptr;       // vectors, see the layout above
    double *d_s = nullptr;       // scratch
    std::vector<hipEvent_t> ev;
    ~PrRun()
    {
        if (c) {
            (void)hipSetDevice(c->device);
            (void)hipStreamSynchronize(c->stream);
        }
        if (d_V) (void)hipFree(d_V);
        if (d_s) (void)hipFree(d_s);
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
};

double pr_ms_since(std::chrono::steady_clock::time_point t)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}
}  // namespace

extern "C" int lzx_pagerank_f64(lzx_handle h, const double *v, uint32_t nd, const double *damping, double tol, uint32_t maxiter, double *X,
                                uint32_t *iters, double *resid, lzx_pagerank_info *info)
{
    static const char *fn = "lzx_pagerank_f64";
    const auto t_start = std::chrono::steady_clock::now();
    if (nd == 0) LZX_FAIL(LZX_ERR_ARG, "%s: nd == 0", fn);
    if (nd > LZX_PR_MAX_ND) LZX_FAIL(LZX_ERR_LIMIT, "%s: nd = %u damping factors (at most %u)", fn, nd, LZX_PR_MAX_ND);
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
    std::vector<double> uq(damping, damping + nd);
    std::sort(uq.begin(), uq.end(), std::greater<double>());
    uq.erase(std::unique(uq.begin(), uq.end()), uq.end());
    const u32 nu = (u32)uq.size();
    std::vector<u32> slot(nd);
    for (u32 s = 0; s < nd; ++s) slot[s] = (u32)(std::lower_bound(uq.begin(), uq.end(), damping[s], std::greater<double>()) - uq.begin());
    std::vector<double> sigma(nu);
    for (u32 u = 0; u < nu; ++u) sigma[u] = 1.0 / uq[u];
    const double sigma0 = sigma[0];

    PrRun run;
    run.c = c;
    LZX_HIP(hipSetDevice(c->device));
    LZX_TRY(lzx_ensure_degrees(c));   // the handle's per-graph degree array (kept as long as the graph, as under operator L)
    // like lzx_spmv_f64: d_v / d_partials / d_io are overwritten, so a prepared decomposition is void (the resident basis, its
    // alpha / beta and the batch state are not touched)
    c->k_prep = 0;

    const u32 ncols = 2 + 2 * nu;
    const u64 state_bytes = (u64)ncols * c->ldq * sizeof(double);
    const bool capped = c->solve_cap_opt >= 0 && state_bytes > (u64)c->solve_cap_opt;
    hipError_t e = capped ? hipErrorOutOfMemory : hipMalloc(reinterpret_cast<void **>(&run.d_V), state_bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        run.d_V = nullptr;
        LZX_FAIL(e == hipErrorOutOfMemory ? LZX_ERR_NOMEM : LZX_ERR_HIP, "%s: the state of %u vectors (b, r, p, 2 per damping) needs %llu bytes of device memory: %s", fn,
                 ncols, (unsigned long long)state_bytes, hipGetErrorString(e));
    }
    auto col = [&](u32 i) { return run.d_V + (size_t)i * c->ldq; };
    double *vb = col(0), *vr = col(1), *vp = col(2), *vz0 = col(3), *vZ = col(4), *vP = col(3 + nu);

    const u32 G = lzx_cgs_grid(c);   // every kernel of this file: the grid of the shifted solver's loop
    const u32 st_words = (u32)((sizeof(PrState) + 7) / 8), mid_words = (u32)((sizeof(PrMid) + 7) / 8);
    const u64 scratch = 3ull * G + 64 + 2ull * st_words + mid_words;
    LZX_HIP(hipMalloc(reinterpret_cast<void **>(&run.d_s), sizeof(double) * scratch));
    double *bb_part = run.d_s, *rr_part = bb_part + G, *pp_part = rr_part + G, *tmp = pp_part + G;   // tmp[64]: ||b||_W^2, masses, residuals
    PrState *d_st = reinterpret_cast<PrState *>(tmp + 64);
    PrMid *d_mid = reinterpret_cast<PrMid *>(tmp + 64 + 2 * st_words);
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

    // r = p = p_s = b, the state of iteration 0
    LZX_HIP(hipMemcpyAsync(vr, vb, sizeof(double) * c->ldq, hipMemcpyDeviceToDevice, c->stream));
    LZX_HIP(hipMemcpyAsync(vp, vb, sizeof(double) * c->ldq, hipMemcpyDeviceToDevice, c->stream));
    for (u32 u = 1; u < nu; ++u)
        LZX_HIP(hipMemcpyAsync(vP + (size_t)(u - 1) * c->ldq, vb, sizeof(double) * c->ldq, hipMemcpyDeviceToDevice, c->stream));
    PrState s0;
    std::memset(&s0, 0, sizeof(s0));
    s0.rr = bb;
    s0.alpha_prev = 1.0;
    for (u32 u = 0; u < LZX_PR_MAX_ND; ++u) s0.zeta[u] = s0.zeta_prev[u] = 1.0;
    s0.live = (1u << nu) - 1u;
    LZX_HIP(hipMemcpyAsync(d_st, &s0, sizeof(s0), hipMemcpyHostToDevice, c->stream));

    PrArgs a{};
    a.r = vr;
    a.p = vp;
    a.z0 = vz0;
    a.t = c->d_v;
    a.deg = c->d_deg;
    a.Z = vZ;
    a.P = vP;
    a.ldq = c->ldq;
    a.n = c->n_loc_pad;
    a.nd = nu;
    a.sigma0 = sigma0;
    a.tolb = tol * bnorm;
    for (u32 u = 0; u < nu; ++u) a.delta[u] = sigma[u] - sigma0;
    a.pm = c->d_partials;
    a.npm = lzx_spmv_partials(c);
    a.rr_part = rr_part;
    a.pp_part = pp_part;
    a.st = d_st;
    a.mid = d_mid;

    const u32 poll = c->solve_poll_opt > 0 ? (u32)std::min<int64_t>(c->solve_poll_opt, 1024) : LZX_PR_POLL;
    for (u32 i = 0; i < 2 * poll + 1; ++i) {
        hipEvent_t ev;
        LZX_HIP(hipEventCreate(&ev));
        run.ev.push_back(ev);
    }
    PrState hs = s0;
    double spmv_ms = 0.0, vec_ms = 0.0;
    u32 launched = 0;
    u32 k = 0;   // iterations since the last poll
    LZX_HIP(hipEventRecord(run.ev[0], c->stream));
    for (u32 j = 0; j < maxiter; ++j) {
        SpmvLaunch l{vp, vp, c->d_v, c->d_partials};
        LZX_TRY(lzx_launch_spmv(c, l));
        LZX_HIP(hipEventRecord(run.ev[2 * k + 1], c->stream));
        a.pp = j == 0 ? bb_part : pp_part;
        a.npp = G;
        hipLaunchKernelGGL(k_pr_update, dim3(G), dim3(LZX_VEC_BLOCK), 0, c->stream, a, j);
        hipLaunchKernelGGL(k_pr_direction, dim3(G), dim3(LZX_VEC_BLOCK), 0, c->stream, a, j);
        LZX_HIP(hipGetLastError());
        LZX_HIP(hipEventRecord(run.ev[2 * k + 2], c->stream));
        ++k;
        launched = j + 1;
        if (k == poll || launched == maxiter) {
            LZX_HIP(hipMemcpyAsync(&hs, d_st + (launched & 1), sizeof(hs), hipMemcpyDeviceToHost, c->stream));
            LZX_HIP(hipStreamSynchronize(c->stream));
            for (u32 i = 0; i < k; ++i) {
                float x = 0.f, y = 0.f;
                LZX_HIP(hipEventElapsedTime(&x, run.ev[2 * i], run.ev[2 * i + 1]));
                LZX_HIP(hipEventElapsedTime(&y, run.ev[2 * i + 1], run.ev[2 * i + 2]));
                spmv_ms += x;
                vec_ms += y;
            }
            k = 0;
            if (hs.done) break;
            LZX_HIP(hipEventRecord(run.ev[0], c->stream));
        }
    }
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
    double ms[2 * LZX_PR_MAX_ND];   // masses at [0, 16), residuals at [16, 32)
    LZX_HIP(hipMemcpyAsync(ms, tmp + 16, sizeof(ms), hipMemcpyDeviceToHost, c->stream));
    LZX_HIP(hipStreamSynchronize(c->stream));
    u32 conv = 0, last = 0;
    for (u32 s = 0; s < nd; ++s) {
        const u32 u = slot[s];
        const bool ok = !((hs.live >> u) & 1u);
        if (s != first[u]) std::memcpy(X + (size_t)s * n, X + (size_t)first[u] * n, sizeof(double) * n);
        if (iters) iters[s] = ok ? hs.iters[u] : launched;
        if (resid) resid[s] = ms[LZX_PR_MAX_ND + u];   // ||v||_1 = 1: v was divided by its sum
        conv += ok;
        if (ok) last = std::max(last, hs.iters[u]);
    }
    if (info) {
        info->iterations = conv == nd ? last : launched;
        info->launched = launched;
        info->converged = conv;
        info->nd = nd;
        info->loop_ms = pr_ms_since(t_start);
        info->spmv_ms = spmv_ms;
        info->vec_ms = vec_ms;
        for (u32 s = 0; s < LZX_PR_MAX_ND; ++s) info->mass[s] = s < nd ? ms[slot[s]] : 0.0;
    }
    if (conv < nd)
        LZX_FAIL(LZX_ERR_LIMIT, "%s: %u of %u damping factors converged in maxiter = %u iterations (tolerance %.3e of ||W^(-1) v||_W = %.6e)", fn, conv, nd,
                 maxiter, tol, bnorm);
    return LZX_OK;
}
