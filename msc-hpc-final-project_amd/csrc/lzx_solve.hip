// lzx_solve.hip -- (sigma_s I - A) x_s = b or (sigma_s I + L) x_s = b for up to 16 shifts at once by multi-shift conjugate
// gradients (Frommer 2003; Jegerlehner): include/lzx.h, lzx_solve_shifted_f64; DESIGN.md section 13.  The loop and its two
// kernels also run PageRank (lzx_pagerank.hip) in their degree-weighted form; the first host part
// (distinct values, lzx_cg_multishift: lzx_internal.h) serves lzx_solve_multi.hip too, lzx_alloc_state every call with a state.
//
// One Krylov sequence: plain CG on the seed system S(sigma_0) (the smallest shift), every other shift s following it through
// the scalars zeta_s, alpha_s, beta_s.  Its residual is zeta_{s,j} r_j, so no shift needs a matvec of its own.
//
// Layout.  Every vector lies in the internal vertex order with stride ldq (= n_loc_pad + LZX_TAIL, tail and padding rows 0):
// b, r, p, x_0 (the seed), then x_s of shifts 1 .. nu-1, then their p_s, then the nw deflation columns.  Shift-major columns:
// a frozen shift costs no bytes at all, and x_s is a column the SpMV can read as it lies.
//
// One iteration j, no host synchronisation (the host reads the status every `poll` iterations):
//   SpMV (+ k_lap_apply with partials under L)   w = M p, partials of p . M p
//   k_cg_update                                  p.Sp closed, alpha_j; r -= alpha_j S p, x_0 += alpha_j p; partials of r.r
//   k_cg_direction                               r.r closed, beta_j, zeta / alpha_s / beta_s, freeze rules; p = r + beta_j p
//                                                (partials of p.p); x_s += alpha_s p_s, p_s = zeta r + beta_s p_s per live shift
// Both kernels close every sum in every workgroup with block_sum_fixed_256 (no atomics, no grid barrier): runs are bit-identical.
// The scalars of the iteration are kept in two device copies by iteration parity: the kernels of iteration j read copy j & 1,
// workgroup 0 of k_cg_direction writes copy (j + 1) & 1.
//
// Both kernels are templates on the inner product.  DEG = false: the plain one, no degree is read.  DEG = true: <a, b>_W =
// sum w_i a_i b_i with w_i = max(d_i, 1), and S p = sigma0 p - (M p) / d (0 where d = 0).  The two forms share every line but
// those products; neither is the other with a weight of 1 (the library is built without contraction: equal operations, equal bits).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "lzx_internal.h"
#include "lzx_graph_call.h"
#include "lzx_spmv_body.h"
#include "lzx_reduce.h"

static constexpr u32 LZX_SOLVE_MAX_W = 8;

// o = s word by word (a struct copy through registers would be indexed dynamically: scratch)
__device__ __forceinline__ void copy_state(CgState &o, const CgState &s)
{
    static_assert(sizeof(CgState) % 8 == 0, "CgState is copied as 8-byte words");
    const u64 *src = reinterpret_cast<const u64 *>(&s);
    u64 *dst = reinterpret_cast<u64 *>(&o);
    for (u32 i = 0; i < sizeof(CgState) / 8; ++i) dst[i] = src[i];
}

// p . S p closed, alpha_j = r.r / p.Sp; not positive (or not finite): the error is recorded, nothing written.
// r -= alpha_j S p, x_0 += alpha_j p while the seed is live; partials of r . r.
template <bool DEG>
__global__ void __launch_bounds__(LZX_VEC_BLOCK) k_cg_update(CgArgs a, u32 j)
{
    __shared__ double sh[4];
    const CgState &s = a.st[j & 1];
    if (s.done) return;
    const double pp = block_sum_fixed_256(a.pp, a.npp, sh);
    const double pm = block_sum_fixed_256(a.pm, a.npm, sh);
    double curv;   // <p, P p>_W = p . (A p): the SpMV's partials as they stand
    if constexpr (DEG) curv = a.sigma0 * pp - pm;
    else curv = a.sigma0 * pp - a.sgn * pm;
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
        const double2 w = *reinterpret_cast<const double2 *>(a.w + i);
        uint2 d = make_uint2(0, 0);
        if constexpr (DEG) d = *reinterpret_cast<const uint2 *>(a.deg + i);
        double2 r = *reinterpret_cast<const double2 *>(a.r + i);
        if constexpr (DEG) {
            const double qx = d.x ? w.x / (double)d.x : 0.0, qy = d.y ? w.y / (double)d.y : 0.0;
            r.x -= alpha * (a.sigma0 * p.x - qx);
            r.y -= alpha * (a.sigma0 * p.y - qy);
        } else {
            r.x -= alpha * (a.sigma0 * p.x - a.sgn * w.x);
            r.y -= alpha * (a.sigma0 * p.y - a.sgn * w.y);
        }
        *reinterpret_cast<double2 *>(a.r + i) = r;
        if (seed) {
            double2 x = *reinterpret_cast<const double2 *>(a.x0 + i);
            x.x += alpha * p.x;
            x.y += alpha * p.y;
            *reinterpret_cast<double2 *>(a.x0 + i) = x;
        }
        if constexpr (DEG) {
            acc += lzx_deg_weight(d.x) * (r.x * r.x);
            acc += lzx_deg_weight(d.y) * (r.y * r.y);
        } else {
            acc += r.x * r.x;
            acc += r.y * r.y;
        }
    }
    block_partial(acc, sh, a.rr_part);
}

// r.r closed, beta_j; per shift zeta_{j+1}, alpha_s, beta_s and the freeze rule |zeta_{s,j+1}| ||r_{j+1}|| <= tol ||b|| (the seed:
// ||r_{j+1}|| <= tol ||b||), the same in every workgroup; workgroup 0 writes the next state.  p = r + beta_j p (partials of
// p . p); for each shift s >= 1 live at entry: x_s += alpha_s p_s, and p_s = zeta r + beta_s p_s unless it froze just now.
template <bool DEG>
__global__ void __launch_bounds__(LZX_VEC_BLOCK) k_cg_direction(CgArgs a, u32 j)
{
    __shared__ double sh[4];
    __shared__ double sc[3][LZX_SOLVE_MAX_NS];   // alpha_s, zeta_{s,j+1}, beta_s
    __shared__ u32 keep[LZX_SOLVE_MAX_NS];       // shift s >= 1 stays live after this iteration
    const CgState &s = a.st[j & 1];
    CgState &o = a.st[(j + 1) & 1];
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    if (s.done) {
        if (writer) copy_state(o, s);
        return;
    }
    const CgMid m = *a.mid;
    if (m.err) {
        if (writer) {
            copy_state(o, s);
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
    if (t >= 1 && t < a.ns) {
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
        for (u32 u = 1; u < a.ns; ++u) nl |= keep[u] << u;
        copy_state(o, s);
        o.rr = rr;
        o.alpha_prev = alpha;
        o.beta_prev = beta;
        for (u32 u = 1; u < a.ns; ++u)
            if ((live >> u) & 1u) {
                o.zeta_prev[u] = s.zeta[u];
                o.zeta[u] = sc[1][u];
            }
        for (u32 u = 0; u < a.ns; ++u)
            if (((live >> u) & 1u) && !((nl >> u) & 1u)) o.iters[u] = j + 1;
        o.live = nl;
        o.done = nl == 0 ? 1u : 0u;
    }
    double acc = 0.0;
    const u32 stride = gridDim.x * LZX_VEC_BLOCK * 2;
    for (u32 i = (blockIdx.x * LZX_VEC_BLOCK + threadIdx.x) * 2; i < a.n; i += stride) {
        const double2 r = *reinterpret_cast<const double2 *>(a.r + i);
        uint2 d = make_uint2(0, 0);
        if constexpr (DEG) d = *reinterpret_cast<const uint2 *>(a.deg + i);
        double2 p = *reinterpret_cast<const double2 *>(a.p + i);
        p.x = r.x + beta * p.x;
        p.y = r.y + beta * p.y;
        *reinterpret_cast<double2 *>(a.p + i) = p;
        if constexpr (DEG) {
            acc += lzx_deg_weight(d.x) * (p.x * p.x);
            acc += lzx_deg_weight(d.y) * (p.y * p.y);
        } else {
            acc += p.x * p.x;
            acc += p.y * p.y;
        }
        for (u32 u = 1; u < a.ns; ++u) {
            if (!((live >> u) & 1u)) continue;
            double *xs = a.X + (size_t)(u - 1) * a.ldq + i, *ps = a.P + (size_t)(u - 1) * a.ldq + i;
            double2 x = *reinterpret_cast<const double2 *>(xs);
            double2 q = *reinterpret_cast<const double2 *>(ps);
            const double as = sc[0][u];
            x.x += as * q.x;
            x.y += as * q.y;
            *reinterpret_cast<double2 *>(xs) = x;
            if (keep[u]) {
                const double zn = sc[1][u], bs = sc[2][u];
                q.x = zn * r.x + bs * q.x;
                q.y = zn * r.y + bs * q.y;
                *reinterpret_cast<double2 *>(ps) = q;
            }
        }
    }
    block_partial(acc, sh, a.pp_part);
}

// partials of ||b - sigma x + sgn v||^2 (v = M x): the true residual of S(sigma) x = b
__global__ void __launch_bounds__(LZX_VEC_BLOCK)
k_cg_resid(const double *__restrict__ b, const double *__restrict__ x, const double *__restrict__ v, double sigma, double sgn, u32 n, double *part)
{
    __shared__ double sh[4];
    double acc = 0.0;
    const u32 stride = gridDim.x * LZX_VEC_BLOCK * 2;
    for (u32 i = (blockIdx.x * LZX_VEC_BLOCK + threadIdx.x) * 2; i < n; i += stride) {
        const double2 bb = *reinterpret_cast<const double2 *>(b + i);
        const double2 xx = *reinterpret_cast<const double2 *>(x + i);
        const double2 vv = *reinterpret_cast<const double2 *>(v + i);
        const double dx = bb.x - (sigma * xx.x - sgn * vv.x), dy = bb.y - (sigma * xx.y - sgn * vv.y);
        acc += dx * dx;
        acc += dy * dy;
    }
    block_partial(acc, sh, part);
}

// ==================================================================================================== host: shared by the CG entry points
int lzx_alloc_state(const char *fn, const char *what, int64_t cap, u64 state_bytes, u64 alloc_bytes, void **out)
{
    const bool capped = cap >= 0 && state_bytes > (u64)cap;
    const hipError_t e = capped ? hipErrorOutOfMemory : hipMalloc(out, alloc_bytes);
    if (e == hipSuccess) return LZX_OK;
    (void)hipGetLastError();
    *out = nullptr;
    LZX_FAIL(e == hipErrorOutOfMemory ? LZX_ERR_NOMEM : LZX_ERR_HIP, "%s: %s needs %llu bytes of device memory: %s", fn, what,
             (unsigned long long)state_bytes, hipGetErrorString(e));
}

std::vector<double> lzx_cg_distinct(const double *v, u32 n, bool descending, std::vector<u32> &slot)
{
    const auto before = [descending](double x, double y) { return descending ? x > y : x < y; };
    std::vector<double> uq(v, v + n);
    std::sort(uq.begin(), uq.end(), before);
    uq.erase(std::unique(uq.begin(), uq.end()), uq.end());
    slot.resize(n);
    for (u32 s = 0; s < n; ++s) slot[s] = (u32)(std::lower_bound(uq.begin(), uq.end(), v[s], before) - uq.begin());
    return uq;
}

int lzx_cg_multishift(LzxCgRun &run, CgArgs a, const double *b, double bb, bool lap, u32 maxiter, CgState &hs, LzxCgLoop &t)
{
    lzx_ctx *c = run.c;
    const u32 G = lzx_cgs_grid(c);
    // r = p = p_s = b, the state of iteration 0
    LZX_HIP(hipMemcpyAsync(a.r, b, sizeof(double) * a.ldq, hipMemcpyDeviceToDevice, c->stream));
    LZX_HIP(hipMemcpyAsync(a.p, b, sizeof(double) * a.ldq, hipMemcpyDeviceToDevice, c->stream));
    for (u32 u = 1; u < a.ns; ++u)
        LZX_HIP(hipMemcpyAsync(a.P + (size_t)(u - 1) * a.ldq, b, sizeof(double) * a.ldq, hipMemcpyDeviceToDevice, c->stream));
    CgState s0;
    std::memset(&s0, 0, sizeof(s0));
    s0.rr = bb;
    s0.alpha_prev = 1.0;
    for (u32 u = 0; u < LZX_SOLVE_MAX_NS; ++u) s0.zeta[u] = s0.zeta_prev[u] = 1.0;
    s0.live = (1u << a.ns) - 1u;
    for (u32 i = 0; i < 2; ++i) LZX_HIP(hipMemcpyAsync(a.st + i, &s0, sizeof(s0), hipMemcpyHostToDevice, c->stream));
    hs = s0;
    return lzx_cg_polled_loop(
        run, a.st, hs, maxiter, t,
        [&](u32) -> int {
            SpmvLaunch l{a.p, a.p, c->d_v, c->d_partials};
            LZX_TRY(lzx_launch_spmv(c, l));
            if (lap) LZX_TRY(lzx_launch_lap_apply(c, c->d_v, a.p, c->d_partials, a.npm, c->n_loc_pad));
            return LZX_OK;
        },
        [&](u32 j) -> int {
            if (j == 1) {
                a.pp = a.pp_part;
                a.npp = G;
            }
            if (a.deg) {
                hipLaunchKernelGGL(k_cg_update<true>, dim3(G), dim3(LZX_VEC_BLOCK), 0, c->stream, a, j);
                hipLaunchKernelGGL(k_cg_direction<true>, dim3(G), dim3(LZX_VEC_BLOCK), 0, c->stream, a, j);
            } else {
                hipLaunchKernelGGL(k_cg_update<false>, dim3(G), dim3(LZX_VEC_BLOCK), 0, c->stream, a, j);
                hipLaunchKernelGGL(k_cg_direction<false>, dim3(G), dim3(LZX_VEC_BLOCK), 0, c->stream, a, j);
            }
            return LZX_OK;
        },
        [](const CgState &s) { return s.done != 0; });
}

// ==================================================================================================== host: lzx_solve_shifted_f64
extern "C" int lzx_solve_shifted_f64(lzx_handle h, const double *b, uint32_t ns, const double *shifts, double tol, uint32_t maxiter,
                                     const double *W, uint32_t nw, double *X, uint32_t *iters, double *resid, lzx_solve_info *info)
{
    static const char *fn = "lzx_solve_shifted_f64";
    const auto t_start = std::chrono::steady_clock::now();
    if (ns == 0) LZX_FAIL(LZX_ERR_ARG, "%s: ns == 0", fn);
    if (ns > LZX_SOLVE_MAX_NS) LZX_FAIL(LZX_ERR_LIMIT, "%s: ns = %u shifts (at most %u)", fn, ns, LZX_SOLVE_MAX_NS);
    if (!(tol > 0.0)) LZX_FAIL(LZX_ERR_ARG, "%s: tol must be > 0", fn);
    if (!shifts) LZX_FAIL(LZX_ERR_ARG, "%s: null shifts", fn);
    for (u32 s = 0; s < ns; ++s) {
        if (!std::isfinite(shifts[s])) LZX_FAIL(LZX_ERR_ARG, "%s: shift %u is not finite", fn, s);
        if (shifts[s] < 0.0) LZX_FAIL(LZX_ERR_ARG, "%s: shift %u = %g < 0: S(sigma) is not positive definite", fn, s, shifts[s]);
    }
    if (nw > LZX_SOLVE_MAX_W) LZX_FAIL(LZX_ERR_LIMIT, "%s: nw = %u deflation vectors (at most %u)", fn, nw, LZX_SOLVE_MAX_W);
    if (maxiter == 0) LZX_FAIL(LZX_ERR_ARG, "%s: maxiter == 0", fn);
    if (!h) LZX_FAIL(LZX_ERR_ARG, "%s: null handle (h)", fn);
    if (!b) LZX_FAIL(LZX_ERR_ARG, "%s: null b", fn);
    if (!X) LZX_FAIL(LZX_ERR_ARG, "%s: null X", fn);
    if (nw > 0 && !W) LZX_FAIL(LZX_ERR_ARG, "%s: nw = %u but W is null", fn, nw);
    lzx_ctx *c = h;
    if (c->comm_kind != 0 || c->world > 1)
        LZX_FAIL(LZX_ERR_STATE, "%s: the solver runs on one GPU handle; this handle is rank %d of a communicator of %d", fn, c->rank, c->world);
    if (!c->d_row_ptr || !c->d_v) LZX_FAIL(LZX_ERR_STATE, "%s: no graph has been handed over", fn);
    const bool lap = c->op_opt == LZX_OP_LAPLACIAN;
    // distinct shifts ascending: unique slot u of every caller shift; the seed is u = 0
    std::vector<u32> slot;
    const std::vector<double> uq = lzx_cg_distinct(shifts, ns, false, slot);
    const u32 nu = (u32)uq.size();
    const double sigma0 = uq[0];
    if (!lap && sigma0 <= 0.0) LZX_FAIL(LZX_ERR_ARG, "%s: shift %g <= 0 under A: sigma I - A is never positive definite there", fn, sigma0);
    if (lap && sigma0 == 0.0 && nw == 0)
        LZX_FAIL(LZX_ERR_ARG, "%s: shift 0 under L needs deflation vectors (nw >= 1) spanning the null space b is orthogonal to", fn);
    const u64 n = c->n;

    LzxCgRun run;
    run.c = c;
    LZX_HIP(hipSetDevice(c->device));
    if (lap) LZX_TRY(lzx_ensure_degrees(c));
    // like lzx_spmv_f64: d_v / d_partials / d_io are overwritten, so a prepared decomposition is void (the resident basis, its
    // alpha / beta and the batch state are not touched)
    c->k_prep = 0;

    const u32 ncols = 2 + 2 * nu + nw;
    const u64 state_bytes = (u64)ncols * c->ldq * sizeof(double);
    char what[80];
    std::snprintf(what, sizeof what, "the state of %u vectors (b, r, p, 2 per shift, %u deflation)", ncols, nw);
    LZX_TRY(lzx_alloc_state(fn, what, c->solve_cap_opt, state_bytes, state_bytes, (void **)&run.d_V));
    auto col = [&](u32 i) { return run.d_V + (size_t)i * c->ldq; };
    double *vb = col(0), *vr = col(1), *vp = col(2), *vx0 = col(3), *vX = col(4), *vP = col(3 + nu), *vW = col(2 + 2 * nu);

    const u32 Gc = lzx_cgs_grid(c);
    const u32 G = Gc;   // the loop's two kernels (lzx_cg_multishift): the same grid as the CGS2 launches
    const u32 st_words = (u32)((sizeof(CgState) + 7) / 8), mid_words = (u32)((sizeof(CgMid) + 7) / 8);
    const u64 scratch = (u64)std::max(nw, 1u) * Gc + 2 * LZX_SOLVE_MAX_W + Gc + 2ull * G + 64 + 2ull * st_words + mid_words;
    LZX_HIP(hipMalloc(reinterpret_cast<void **>(&run.d_s), sizeof(double) * scratch));
    LzxCgsScratch sc{Gc, run.d_s, nullptr, nullptr, nullptr};
    sc.h1 = sc.part + (size_t)std::max(nw, 1u) * Gc;
    sc.h2 = sc.h1 + LZX_SOLVE_MAX_W;
    sc.npart = sc.h2 + LZX_SOLVE_MAX_W;
    double *rr_part = sc.npart + Gc, *pp_part = rr_part + G, *tmp = pp_part + G;   // tmp[64]: ||b||^2, W norms, residuals
    CgState *d_st = reinterpret_cast<CgState *>(tmp + 64);
    CgMid *d_mid = reinterpret_cast<CgMid *>(tmp + 64 + 2 * st_words);
    LZX_HIP(hipMemsetAsync(run.d_V, 0, state_bytes, c->stream));   // padding rows and tails stay 0 from here on
    LZX_HIP(hipMemsetAsync(run.d_s, 0, sizeof(double) * scratch, c->stream));

    // deflation vectors, orthonormalised in order; b projected onto their complement (its norm before: tmp[9], after: tmp[0])
    for (u32 t = 0; t < nw; ++t) {
        LZX_HIP(hipMemcpyAsync(c->d_io, W + (size_t)t * n, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
        LZX_TRY(lzx_launch_permute_in(c, c->d_io, vW + (size_t)t * c->ldq, 1.0));
        LZX_TRY(lzx_cgs_orthonormalise(c, vW, t, sc, tmp + 1 + t));
    }
    LZX_HIP(hipMemcpyAsync(c->d_io, b, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    LZX_TRY(lzx_launch_permute_in(c, c->d_io, vb, 1.0));
    LZX_TRY(lzx_cgs2(c, vW, 0, vb, sc));
    LZX_TRY(lzx_launch_reduce(c, sc.npart, Gc, tmp + 9, 0));
    LZX_TRY(lzx_cgs2(c, vW, nw, vb, sc));   // (nw = 0: the norm partials again; the seed's first p . p closes these)
    LZX_TRY(lzx_launch_reduce(c, sc.npart, Gc, tmp, 0));
    double h_tmp[10];
    LZX_HIP(hipMemcpyAsync(h_tmp, tmp, sizeof(h_tmp), hipMemcpyDeviceToHost, c->stream));
    LZX_HIP(hipStreamSynchronize(c->stream));
    for (u32 t = 0; t < nw; ++t)
        if (!(h_tmp[1 + t] > 0.0)) LZX_FAIL(LZX_ERR_ARG, "%s: W is rank-deficient (column %u lies in the span of the columns before it)", fn, t);
    const double bb = h_tmp[0], bb_in = h_tmp[9];
    if (!std::isfinite(bb_in)) LZX_FAIL(LZX_ERR_ARG, "%s: b is not finite", fn);
    if (!(bb_in > 0.0)) LZX_FAIL(LZX_ERR_ARG, "%s: b is zero", fn);
    if (!(bb > 1e-20 * bb_in)) LZX_FAIL(LZX_ERR_ARG, "%s: b lies in the span of W", fn);
    const double bnorm = std::sqrt(bb);

    CgArgs a{};
    a.r = vr;
    a.p = vp;
    a.x0 = vx0;
    a.w = c->d_v;
    a.X = vX;
    a.P = vP;
    a.ldq = c->ldq;
    a.n = c->n_loc_pad;
    a.ns = nu;
    a.sigma0 = sigma0;
    a.sgn = lap ? -1.0 : 1.0;
    a.tolb = tol * bnorm;
    for (u32 u = 0; u < nu; ++u) a.delta[u] = uq[u] - sigma0;
    a.pp = sc.npart;
    a.npp = Gc;
    a.pm = c->d_partials;
    a.npm = lzx_spmv_partials(c);
    a.rr_part = rr_part;
    a.pp_part = pp_part;
    a.st = d_st;
    a.mid = d_mid;

    CgState hs;
    LzxCgLoop lp;
    LZX_TRY(lzx_cg_multishift(run, a, vb, bb, lap, maxiter, hs, lp));
    const u32 launched = lp.launched;
    if (hs.done == 2)
        LZX_FAIL(LZX_ERR_ARG, "%s: S(sigma_0) is not positive definite: p . S p = %.6e at iteration %u (sigma_0 = %.17g)", fn, hs.curv, hs.err_iter,
                 sigma0);

    // every x_s: projected onto the complement of W, its true residual (one SpMV), caller order
    std::vector<u32> first(nu, ns);
    for (u32 s = 0; s < ns; ++s) first[slot[s]] = std::min(first[slot[s]], s);
    for (u32 u = 0; u < nu; ++u) {
        double *x = u == 0 ? vx0 : vX + (size_t)(u - 1) * c->ldq;
        if (nw > 0) LZX_TRY(lzx_cgs2(c, vW, nw, x, sc));
        SpmvLaunch l{x, x, c->d_v, c->d_partials};
        LZX_TRY(lzx_launch_spmv(c, l));
        if (lap) LZX_TRY(lzx_launch_lap_apply(c, c->d_v, x, nullptr, 0, c->n_loc_pad));
        hipLaunchKernelGGL(k_cg_resid, dim3(G), dim3(LZX_VEC_BLOCK), 0, c->stream, vb, x, c->d_v, uq[u], a.sgn, c->n_loc_pad, rr_part);
        LZX_HIP(hipGetLastError());
        LZX_TRY(lzx_launch_reduce(c, rr_part, G, tmp + 16 + u, 0));
        LZX_TRY(lzx_launch_permute_out(c, x, c->d_io));
        LZX_HIP(hipMemcpyAsync(X + (size_t)first[u] * n, c->d_io, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    }
    double rs[LZX_SOLVE_MAX_NS];
    LZX_HIP(hipMemcpyAsync(rs, tmp + 16, sizeof(double) * nu, hipMemcpyDeviceToHost, c->stream));
    LZX_HIP(hipStreamSynchronize(c->stream));
    u32 conv = 0, last = 0;
    for (u32 s = 0; s < ns; ++s) {
        const u32 u = slot[s];
        const bool ok = !((hs.live >> u) & 1u);
        if (s != first[u]) std::memcpy(X + (size_t)s * n, X + (size_t)first[u] * n, sizeof(double) * n);
        if (iters) iters[s] = ok ? hs.iters[u] : launched;
        if (resid) resid[s] = std::sqrt(rs[u]) / bnorm;
        conv += ok;
        if (ok) last = std::max(last, hs.iters[u]);
    }
    if (info) {
        info->iterations = conv == ns ? last : launched;
        info->launched = launched;
        info->converged = conv;
        info->ns = ns;
        info->loop_ms = lzx_ms_since(t_start);
        info->spmv_ms = lp.spmv_ms;
        info->vec_ms = lp.vec_ms;
        info->bnorm = bnorm;
    }
    if (conv < ns)
        LZX_FAIL(LZX_ERR_LIMIT, "%s: %u of %u shifts converged in maxiter = %u iterations (tolerance %.3e of ||b|| = %.6e)", fn, conv, ns, maxiter, tol,
                 bnorm);
    return LZX_OK;
}
