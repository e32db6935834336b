// lzx_solve_multi.hip -- S(sigma_c) x_c = b_c for up to 16 right-hand sides at once: a batch of independent conjugate-gradient
// solves, one per column, that share one SpMM per iteration (include/lzx.h: lzx_solve_multi_f64).
//
// Not block CG: no coupling between the columns.  Column c runs plain CG (x = 0, r_0 = p_0 = b_c) on S(sigma_c) = sigma_c I - A
// (or sigma_c I + L) with scalars, a stop and a failure of its own.
//
// Layout.  b, r, p, x and the batched work vector w = M p are vertex-major and interleaved, [n][B], B = nb padded to 2, 4, 8 or
// 16 (lzx_multi_shared.h): one col_idx read and one gathered line serve every column.  Padded columns are zero and frozen from
// the start.  The deflation vectors W are plain [nw][n] columns in the caller's order.
//
// One iteration j, no host synchronisation (the host reads the status every `poll` iterations):
//   k_multi_spmm + k_multi_alpha (Q = P)   w = M p (under L with the fma(d, x, -v) epilogue), partials of p . M p
//   k_mcg_update                           p.p and p.Mp closed, alpha_c = r.r / (sigma_c p.p -+ p.Mp); live columns:
//                                          r -= alpha (sigma p -+ w), x += alpha p; partials of r . r
//   k_mcg_direction                        r.r closed, beta_c, the freeze rule ||r_c|| <= tol ||b_c||, the state of the other
//                                          parity; columns that stay live: p = r + beta p; partials of p . p
// Every sum has the batched path's shape, which depends on n alone: runs of LZX_MULTI_RUN rows added left to right by one thread,
// one partial per LZX_MULTI_SEG rows (seg_partials), closed in every workgroup by close_cols.  No atomics, no grid barrier: a
// column's bits do not depend on B, on its place in the batch or on its neighbours.  A thread works on two neighbouring columns
// of a run (16-byte loads and stores); the per-column scalars lie in LDS, never in an indexed register array.
// The scalars are kept in two device copies by iteration parity: the kernels of iteration j read copy j & 1, workgroup 0 of
// k_mcg_direction writes copy (j + 1) & 1.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "lzx_internal.h"
#include "lzx_graph_call.h"
#include "lzx_spmv_body.h"
#include "lzx_reduce.h"
#include "lzx_multi_shared.h"

static constexpr u32 LZX_MCG_MAX_NB = 16;
static constexpr u32 LZX_MCG_MAX_W = 8;
static constexpr u32 LZX_MCG_WGRID = 64;   // workgroups (and partials) of the sums over one plain W column

namespace {
struct McgState {
    double rr[LZX_MCG_MAX_NB];        // r_{c,j} . r_{c,j}
    double curv[LZX_MCG_MAX_NB];      // bad column: p . S p of the iteration that failed
    u32 iters[LZX_MCG_MAX_NB];        // the iteration count at which column c froze
    u32 err_iter[LZX_MCG_MAX_NB];     // bad column: the iteration
    u32 live;                         // bit c: x_c, r_c and p_c are still written
    u32 bad;                          // bit c: S(sigma_c) turned out not to be positive definite
    u32 pad_[2];
};
struct McgMid {                       // k_mcg_update (workgroup 0) -> k_mcg_direction of the same iteration
    double alpha[LZX_MCG_MAX_NB], curv[LZX_MCG_MAX_NB];
    u32 bad;                          // bit c: live at entry and p . S p <= 0 or not finite
    u32 pad_;
};
struct McgArgs {
    double *r, *p, *x;                // [n][B]
    const double *w;                  // [n][B] M p
    u64 n;
    u32 n_seg;
    double sgn;                       // S p = sigma p - sgn (M p): 1 under A, -1 under L
    double sigma[LZX_MCG_MAX_NB];
    double tolb[LZX_MCG_MAX_NB];      // tol ||b_c||
    const double *pp, *pm;            // [n_seg][B] partials of p . p and p . M p
    double *rr_part, *pp_part;        // [n_seg][B] written by k_mcg_update / k_mcg_direction
    McgState *st;                     // [2]
    McgMid *mid;
};
struct McgSigma { double v[LZX_MCG_MAX_NB]; };
}  // namespace

// ==================================================================================================== kernels
// The row segments of a [n][B] vector in the batched path's reduction shape: body(i, s0, s1) for i = r * B + c0 over the rows
// of a run in ascending order, one thread per (run, column pair c0, c0 + 1); the runs' totals -> one partial per segment and
// column in out[seg * B + c].  Call with all threads.
template <u32 B, typename F>
__device__ __forceinline__ void mcg_segments(u64 n, u32 n_seg, double *sh, double *out, F body)
{
    constexpr u32 H = B / 2;
    for (u32 seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
        for (u32 u = threadIdx.x; u < LZX_MULTI_RUNS * H; u += LZX_MULTI_BLOCK) {
            const u32 run = u / H, c0 = (u % H) * 2;
            const u64 r0 = (u64)seg * LZX_MULTI_SEG + (u64)run * LZX_MULTI_RUN;
            const u64 r1 = std::min<u64>(r0 + LZX_MULTI_RUN, n);
            double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
            for (u64 r = r0; r < r1; ++r) body(r * B + c0, c0, s0, s1);
            sh[run * B + c0] = s0;
            sh[run * B + c0 + 1] = s1;
        }
        seg_partials<B>(sh, out + (u64)seg * B);
    }
}

__device__ __forceinline__ double2 ld2(const double *p) { return *reinterpret_cast<const double2 *>(p); }
__device__ __forceinline__ void st2(double *p, double2 v) { *reinterpret_cast<double2 *>(p) = v; }

// partials of ||x_c||^2
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK) k_mcg_norm(const double *__restrict__ X, u64 n, u32 n_seg, double *pn)
{
    __shared__ double sh[LZX_MULTI_RUNS * B];
    mcg_segments<B>(n, n_seg, sh, pn, [&](u64 i, u32, double &s0, double &s1) {
        const double2 x = ld2(X + i);
        s0 += x.x * x.x;
        s1 += x.y * x.y;
    });
}

// partials of w . x_c for one plain vector w
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK)
k_mcg_wcoef(const double *__restrict__ w, const double *__restrict__ X, u64 n, u32 n_seg, double *pc)
{
    __shared__ double sh[LZX_MULTI_RUNS * B];
    mcg_segments<B>(n, n_seg, sh, pc, [&](u64 i, u32, double &s0, double &s1) {
        const double2 x = ld2(X + i);
        const double wr = w[i / B];
        s0 += wr * x.x;
        s1 += wr * x.y;
    });
}

// x_c -= (w . x_c) w, the coefficients closed from pc by every workgroup
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK) k_mcg_waxpy(const double *__restrict__ w, double *X, u64 n, const double *pc, u32 n_seg)
{
    __shared__ double shw[4 * B], sc[B];
    close_cols<B>(pc, n_seg, shw, sc);
    const u64 total = n * B;
    for (u64 i = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x; i < total; i += (u64)gridDim.x * LZX_MULTI_BLOCK)
        X[i] -= sc[i % B] * w[i / B];
}

// partials of ||b_c - (sigma_c x_c - sgn v_c)||^2, v = M x: the true residual of S(sigma_c) x_c = b_c
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK)
k_mcg_resid(const double *__restrict__ Bv, const double *__restrict__ X, const double *__restrict__ V, McgSigma sig, double sgn, u64 n,
            u32 n_seg, double *pn)
{
    __shared__ double sh[LZX_MULTI_RUNS * B];
    mcg_segments<B>(n, n_seg, sh, pn, [&](u64 i, u32 c0, double &s0, double &s1) {
        const double2 b = ld2(Bv + i), x = ld2(X + i), v = ld2(V + i);
        const double d0 = b.x - (sig.v[c0] * x.x - sgn * v.x), d1 = b.y - (sig.v[c0 + 1] * x.y - sgn * v.y);
        s0 += d0 * d0;
        s1 += d1 * d1;
    });
}

// out[c] = the closed total of p[.][c] (grid of one)
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK) k_mcg_close(const double *p, u32 n_seg, double *out)
{
    __shared__ double shw[4 * B], sc[B];
    close_cols<B>(p, n_seg, shw, sc);
    if (threadIdx.x < B) out[threadIdx.x] = sc[threadIdx.x];
}

// p.p and p.Mp closed; alpha_c = r.r / (sigma_c p.p - sgn p.Mp); a live column whose curvature is not positive (or not finite)
// is recorded and left alone.  Live columns: r -= alpha (sigma p - sgn w), x += alpha p; partials of r . r.
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK) k_mcg_update(McgArgs a, u32 j)
{
    __shared__ double sh[LZX_MULTI_RUNS * B];
    __shared__ double shw[4 * B], spp[B], spm[B], sal[B], ssg[B];
    __shared__ u32 sact[B], sbad[B];
    const McgState &s = a.st[j & 1];
    if (s.live == 0) return;
    close_cols<B>(a.pp, a.n_seg, shw, spp);
    close_cols<B>(a.pm, a.n_seg, shw, spm);
    if (threadIdx.x < B) {
        const u32 c = threadIdx.x;
        const bool live = (s.live >> c) & 1u;
        const double curv = a.sigma[c] * spp[c] - a.sgn * spm[c];
        const bool bad = live && (!(curv > 0.0) || !isfinite(curv));
        const double alpha = s.rr[c] / curv;
        sal[c] = alpha;
        ssg[c] = a.sigma[c];
        sact[c] = live && !bad;
        sbad[c] = bad;
        if (blockIdx.x == 0) {   // (a column that is not live: 0, not the quotient of its stale sums)
            a.mid->alpha[c] = live && !bad ? alpha : 0.0;
            a.mid->curv[c] = live ? curv : 0.0;
        }
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        u32 m = 0;
        for (u32 c = 0; c < B; ++c) m |= sbad[c] << c;
        a.mid->bad = m;
    }
    const double sgn = a.sgn;
    constexpr u32 H = B / 2;
    for (u32 seg = blockIdx.x; seg < a.n_seg; seg += gridDim.x) {
        for (u32 u = threadIdx.x; u < LZX_MULTI_RUNS * H; u += LZX_MULTI_BLOCK) {
            const u32 run = u / H, c0 = (u % H) * 2;
            const u64 r0 = (u64)seg * LZX_MULTI_SEG + (u64)run * LZX_MULTI_RUN;
            const u64 r1 = std::min<u64>(r0 + LZX_MULTI_RUN, a.n);
            const bool k0 = sact[c0], k1 = sact[c0 + 1];
            const double a0 = sal[c0], a1 = sal[c0 + 1], g0 = ssg[c0], g1 = ssg[c0 + 1];
            double s0 = 0.0, s1 = 0.0;
            if (k0 || k1) {
                u64 r = r0;
                // four rows' loads in flight, then the same operations row by row
                for (; r + 4 <= r1; r += 4) {
                    double2 p[4], w[4], rr[4], x[4];
#pragma unroll
                    for (u32 t = 0; t < 4; ++t) {
                        const u64 i = (r + t) * B + c0;
                        p[t] = ld2(a.p + i);
                        w[t] = ld2(a.w + i);
                        rr[t] = ld2(a.r + i);
                        x[t] = ld2(a.x + i);
                    }
#pragma unroll
                    for (u32 t = 0; t < 4; ++t) {
                        const u64 i = (r + t) * B + c0;
                        if (k0) {
                            rr[t].x -= a0 * (g0 * p[t].x - sgn * w[t].x);
                            x[t].x += a0 * p[t].x;
                            s0 += rr[t].x * rr[t].x;
                        }
                        if (k1) {
                            rr[t].y -= a1 * (g1 * p[t].y - sgn * w[t].y);
                            x[t].y += a1 * p[t].y;
                            s1 += rr[t].y * rr[t].y;
                        }
                        st2(a.r + i, rr[t]);
                        st2(a.x + i, x[t]);
                    }
                }
                for (; r < r1; ++r) {
                    const u64 i = r * B + c0;
                    const double2 p = ld2(a.p + i), w = ld2(a.w + i);
                    double2 rr = ld2(a.r + i), x = ld2(a.x + i);
                    if (k0) {
                        rr.x -= a0 * (g0 * p.x - sgn * w.x);
                        x.x += a0 * p.x;
                        s0 += rr.x * rr.x;
                    }
                    if (k1) {
                        rr.y -= a1 * (g1 * p.y - sgn * w.y);
                        x.y += a1 * p.y;
                        s1 += rr.y * rr.y;
                    }
                    st2(a.r + i, rr);
                    st2(a.x + i, x);
                }
            }
            sh[run * B + c0] = s0;
            sh[run * B + c0 + 1] = s1;
        }
        seg_partials<B>(sh, a.rr_part + (u64)seg * B);
    }
}

// r.r closed, beta_c = r.r / (r.r of the iteration before); a column freezes once ||r_c|| <= tol ||b_c||, the same in every
// workgroup; workgroup 0 writes the state of the next parity.  Columns that stay live: p = r + beta p; partials of p . p.
template <u32 B>
__global__ void __launch_bounds__(LZX_MULTI_BLOCK) k_mcg_direction(McgArgs a, u32 j)
{
    __shared__ double sh[LZX_MULTI_RUNS * B];
    __shared__ double shw[4 * B], srr[B], sbeta[B];
    __shared__ u32 skeep[B];
    const McgState &s = a.st[j & 1];
    McgState &o = a.st[(j + 1) & 1];
    const bool wg0 = blockIdx.x == 0;
    if (s.live == 0) {
        if (wg0 && threadIdx.x < LZX_MCG_MAX_NB) {
            const u32 c = threadIdx.x;
            o.rr[c] = s.rr[c];
            o.curv[c] = s.curv[c];
            o.iters[c] = s.iters[c];
            o.err_iter[c] = s.err_iter[c];
            if (c == 0) {
                o.live = 0;
                o.bad = s.bad;
            }
        }
        return;
    }
    close_cols<B>(a.rr_part, a.n_seg, shw, srr);
    const u32 badm = a.mid->bad;
    if (threadIdx.x < B) {
        const u32 c = threadIdx.x;
        const bool live = (s.live >> c) & 1u, isbad = (badm >> c) & 1u;
        const bool act = live && !isbad;
        const double rr = srr[c];
        const bool frz = act && sqrt(rr) <= a.tolb[c];
        sbeta[c] = rr / s.rr[c];
        skeep[c] = act && !frz;
        if (wg0) {
            o.rr[c] = act ? rr : s.rr[c];
            o.iters[c] = frz ? j + 1 : s.iters[c];
            o.curv[c] = isbad ? a.mid->curv[c] : s.curv[c];
            o.err_iter[c] = isbad ? j : s.err_iter[c];
        }
    }
    __syncthreads();
    if (wg0 && threadIdx.x == 0) {
        u32 nl = 0;
        for (u32 c = 0; c < B; ++c) nl |= skeep[c] << c;
        o.live = nl;
        o.bad = s.bad | badm;
    }
    constexpr u32 H = B / 2;
    for (u32 seg = blockIdx.x; seg < a.n_seg; seg += gridDim.x) {
        for (u32 u = threadIdx.x; u < LZX_MULTI_RUNS * H; u += LZX_MULTI_BLOCK) {
            const u32 run = u / H, c0 = (u % H) * 2;
            const u64 r0 = (u64)seg * LZX_MULTI_SEG + (u64)run * LZX_MULTI_RUN;
            const u64 r1 = std::min<u64>(r0 + LZX_MULTI_RUN, a.n);
            const bool k0 = skeep[c0], k1 = skeep[c0 + 1];
            const double b0 = sbeta[c0], b1 = sbeta[c0 + 1];
            double s0 = 0.0, s1 = 0.0;
            if (k0 || k1) {
                u64 r = r0;
                for (; r + 8 <= r1; r += 8) {
                    double2 rr[8], p[8];
#pragma unroll
                    for (u32 t = 0; t < 8; ++t) {
                        const u64 i = (r + t) * B + c0;
                        rr[t] = ld2(a.r + i);
                        p[t] = ld2(a.p + i);
                    }
#pragma unroll
                    for (u32 t = 0; t < 8; ++t) {
                        if (k0) {
                            p[t].x = rr[t].x + b0 * p[t].x;
                            s0 += p[t].x * p[t].x;
                        }
                        if (k1) {
                            p[t].y = rr[t].y + b1 * p[t].y;
                            s1 += p[t].y * p[t].y;
                        }
                        st2(a.p + (r + t) * B + c0, p[t]);
                    }
                }
                for (; r < r1; ++r) {
                    const u64 i = r * B + c0;
                    const double2 rr = ld2(a.r + i);
                    double2 p = ld2(a.p + i);
                    if (k0) {
                        p.x = rr.x + b0 * p.x;
                        s0 += p.x * p.x;
                    }
                    if (k1) {
                        p.y = rr.y + b1 * p.y;
                        s1 += p.y * p.y;
                    }
                    st2(a.p + i, p);
                }
            }
            sh[run * B + c0] = s0;
            sh[run * B + c0 + 1] = s1;
        }
        seg_partials<B>(sh, a.pp_part + (u64)seg * B);
    }
}

// ---- the deflation vectors: plain columns of n doubles, orthonormalised once per solve
// part[workgroup] = partial of a . b (LZX_MCG_WGRID workgroups)
__global__ void __launch_bounds__(LZX_MULTI_BLOCK) k_mcg_wdot(const double *__restrict__ a, const double *__restrict__ b, u64 n, double *part)
{
    __shared__ double sh[4];
    double acc = 0.0;
    for (u64 i = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * LZX_MULTI_BLOCK) acc += a[i] * b[i];
    block_partial(acc, sh, part);
}

// t = the closed sum of part.  mode 0: w -= t v (a projection step).  mode 1: w /= sqrt(t) where t > 0.  mode 2: the final norm
// sqrt(t) -> *out; at most 1e-10 (the column lay in the span of those before it): 0 is stored and w becomes 0, else w /= it.
__global__ void __launch_bounds__(LZX_MULTI_BLOCK) k_mcg_wapply(double *w, const double *v, u64 n, const double *part, int mode, double *out)
{
    __shared__ double sh[4];
    const double t = block_sum_fixed_256(part, LZX_MCG_WGRID, sh);
    double nrm = sqrt(t);
    const bool dead = mode == 2 && !(nrm > 1e-10);
    if (mode == 2 && blockIdx.x == 0 && threadIdx.x == 0) *out = dead ? 0.0 : nrm;
    if (mode == 1 && !(nrm > 0.0)) return;
    for (u64 i = (u64)blockIdx.x * LZX_MULTI_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * LZX_MULTI_BLOCK) {
        if (mode == 0) w[i] -= t * v[i];
        else w[i] = dead ? 0.0 : w[i] / nrm;
    }
}

// ==================================================================================================== host
namespace {
struct McgRun : LzxCgRun {       // d_V: b, r, p, x ([n][B] each), then W
    bool own_work = false;       // the batched path's work vectors were made (or re-made at this width) by this call
    ~McgRun()
    {
        release();
        if (c && own_work && c->multi) lzx_multi_free_work(c->multi);
    }
};

struct McgCall {
    uint32_t nb;
    const double *Bm, *shifts;
    double tol;
    uint32_t maxiter;
    const double *W;
    uint32_t nw;
    double *X;
    uint32_t *iters;
    double *resid;
    uint32_t *status;
    lzx_solve_multi_info *info;
    std::chrono::steady_clock::time_point t_start;
};
}  // namespace

template <u32 B>
static int mcg_run(lzx_ctx *c, const McgCall &q, const char *fn)
{
    lzx_multi_state *m = c->multi;
    const u64 n = c->n, nB = n * B;
    const u32 nb = q.nb, nw = q.nw, n_seg = m->n_seg;
    const bool lap = c->op_opt == LZX_OP_LAPLACIAN;
    const double sgn = lap ? -1.0 : 1.0;

    McgRun run;
    run.c = c;
    const u64 part_doubles = (u64)n_seg * B;
    const u64 state_bytes = ((5ull * B + nw) * n + 3 * part_doubles) * sizeof(double);
    // (the cap again, ahead of lzx_alloc_state's: before the work vectors are made, and this text ends without a runtime error)
    if (c->solve_cap_opt >= 0 && state_bytes > (u64)c->solve_cap_opt)
        LZX_FAIL(LZX_ERR_NOMEM, "%s: the state of 5 x %u interleaved columns and %u deflation vectors needs %llu bytes of device memory", fn, B, nw,
                 (unsigned long long)state_bytes);
    // the batched path's work vectors at this width: where the call has to make them (none yet, or another width's, which
    // lzx_multi_ensure_work frees first), it frees them at return
    run.own_work = !(m->d_V && m->wB == B);
    LZX_TRY(lzx_multi_ensure_work(c, B, false));
    char what[80];
    std::snprintf(what, sizeof what, "the state of 5 x %u interleaved columns and %u deflation vectors", B, nw);
    LZX_TRY(lzx_alloc_state(fn, what, c->solve_cap_opt, state_bytes, sizeof(double) * (4 * nB + (u64)nw * n), (void **)&run.d_V));
    double *vB = run.d_V, *vR = vB + nB, *vP = vR + nB, *vX = vP + nB, *vW = vX + nB;

    // scalars: [rr partials | pp partials | W partials | tmp | state x 2 | mid]
    const u32 st_words = (u32)((sizeof(McgState) + 7) / 8), mid_words = (u32)((sizeof(McgMid) + 7) / 8);
    const u64 n_s = 2 * part_doubles + LZX_MCG_WGRID + 64 + 2ull * st_words + mid_words;
    LZX_HIP(hipMalloc(reinterpret_cast<void **>(&run.d_s), sizeof(double) * n_s));
    double *rr_part = run.d_s, *pp_part = rr_part + part_doubles, *w_part = pp_part + part_doubles, *tmp = w_part + LZX_MCG_WGRID;
    double *t_wn = tmp, *t_bin = tmp + 8, *t_bb = tmp + 24, *t_rs = tmp + 40;   // W norms [8]; ||b||^2 before / after deflation, residuals [16] each
    McgState *d_st = reinterpret_cast<McgState *>(tmp + 64);
    McgMid *d_mid = reinterpret_cast<McgMid *>(tmp + 64 + 2 * st_words);
    LZX_HIP(hipMemsetAsync(run.d_s, 0, sizeof(double) * n_s, c->stream));
    LZX_HIP(hipMemsetAsync(vX, 0, sizeof(double) * nB, c->stream));

    const u32 vgrid = std::min<u32>(std::max<u32>(n_seg, 1), (u32)c->cu_count * 4);
    const u32 sgrid = std::min<u32>(grid_of(nB), (u32)c->cu_count * 8);
    const u32 wgrid = std::min<u32>(grid_of(n), (u32)c->cu_count * 8);
    const dim3 blk(LZX_MULTI_BLOCK);

    // deflation vectors: made unit, orthogonalised against those before (twice), made unit again
    if (nw) LZX_HIP(hipMemcpyAsync(vW, q.W, sizeof(double) * nw * n, hipMemcpyHostToDevice, c->stream));
    for (u32 t = 0; t < nw; ++t) {
        double *wt = vW + (u64)t * n;
        hipLaunchKernelGGL(k_mcg_wdot, dim3(LZX_MCG_WGRID), blk, 0, c->stream, wt, wt, n, w_part);
        hipLaunchKernelGGL(k_mcg_wapply, dim3(wgrid), blk, 0, c->stream, wt, wt, n, w_part, 1, (double *)nullptr);
        for (u32 pass = 0; pass < 2; ++pass)
            for (u32 i = 0; i < t; ++i) {
                const double *wi = vW + (u64)i * n;
                hipLaunchKernelGGL(k_mcg_wdot, dim3(LZX_MCG_WGRID), blk, 0, c->stream, wi, wt, n, w_part);
                hipLaunchKernelGGL(k_mcg_wapply, dim3(wgrid), blk, 0, c->stream, wt, wi, n, w_part, 0, (double *)nullptr);
            }
        hipLaunchKernelGGL(k_mcg_wdot, dim3(LZX_MCG_WGRID), blk, 0, c->stream, wt, wt, n, w_part);
        hipLaunchKernelGGL(k_mcg_wapply, dim3(wgrid), blk, 0, c->stream, wt, wt, n, w_part, 2, t_wn + t);
        LZX_HIP(hipGetLastError());
    }
    // x -= W W^T x over all columns of an [n][B] vector, twice (one W column after the other)
    auto project = [&](double *x) -> int {
        for (u32 pass = 0; pass < 2 && nw; ++pass)
            for (u32 t = 0; t < nw; ++t) {
                const double *wt = vW + (u64)t * n;
                hipLaunchKernelGGL(k_mcg_wcoef<B>, dim3(vgrid), blk, 0, c->stream, wt, x, n, n_seg, rr_part);
                hipLaunchKernelGGL(k_mcg_waxpy<B>, dim3(sgrid), blk, 0, c->stream, wt, x, n, rr_part, n_seg);
            }
        LZX_HIP(hipGetLastError());
        return LZX_OK;
    };

    // b: staged as [nb][n] in the work vector, packed, projected; its norms before and after
    MultiDiv one{};
    for (u32 col = 0; col < 16; ++col) one.v[col] = 1.0;
    LZX_HIP(hipMemcpyAsync(m->d_V, q.Bm, sizeof(double) * nb * n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_multi_pack<B>, dim3(grid_of(nB)), blk, 0, c->stream, m->d_V, nb, n, one, vB);
    hipLaunchKernelGGL(k_mcg_norm<B>, dim3(vgrid), blk, 0, c->stream, vB, n, n_seg, pp_part);
    hipLaunchKernelGGL(k_mcg_close<B>, dim3(1), blk, 0, c->stream, pp_part, n_seg, t_bin);
    LZX_HIP(hipGetLastError());
    LZX_TRY(project(vB));
    hipLaunchKernelGGL(k_mcg_norm<B>, dim3(vgrid), blk, 0, c->stream, vB, n, n_seg, pp_part);   // (the first p . p closes these)
    hipLaunchKernelGGL(k_mcg_close<B>, dim3(1), blk, 0, c->stream, pp_part, n_seg, t_bb);
    LZX_HIP(hipGetLastError());
    double h_tmp[40];
    LZX_HIP(hipMemcpyAsync(h_tmp, tmp, sizeof(h_tmp), hipMemcpyDeviceToHost, c->stream));
    LZX_HIP(hipStreamSynchronize(c->stream));
    for (u32 t = 0; t < nw; ++t)
        if (!(h_tmp[t] > 0.0)) LZX_FAIL(LZX_ERR_ARG, "%s: W is rank-deficient (column %u lies in the span of the columns before it)", fn, t);
    double bnorm[LZX_MCG_MAX_NB] = {};
    for (u32 col = 0; col < nb; ++col) {
        const double bb_in = h_tmp[8 + col], bb = h_tmp[24 + col];
        if (!std::isfinite(bb_in)) LZX_FAIL(LZX_ERR_ARG, "%s: column %u of b is not finite", fn, col);
        if (!(bb_in > 0.0)) LZX_FAIL(LZX_ERR_ARG, "%s: column %u of b is zero", fn, col);
        if (!(bb > 1e-20 * bb_in)) LZX_FAIL(LZX_ERR_ARG, "%s: column %u of b lies in the span of W", fn, col);
        bnorm[col] = std::sqrt(bb);
    }

    // r = p = b, the state of iteration 0 (both parities: a column that never runs keeps what it has)
    LZX_HIP(hipMemcpyAsync(vR, vB, sizeof(double) * nB, hipMemcpyDeviceToDevice, c->stream));
    LZX_HIP(hipMemcpyAsync(vP, vB, sizeof(double) * nB, hipMemcpyDeviceToDevice, c->stream));
    McgState s0;
    std::memset(&s0, 0, sizeof(s0));
    for (u32 col = 0; col < nb; ++col) s0.rr[col] = h_tmp[24 + col];
    s0.live = (1u << nb) - 1u;
    LZX_HIP(hipMemcpyAsync(d_st, &s0, sizeof(s0), hipMemcpyHostToDevice, c->stream));
    LZX_HIP(hipMemcpyAsync(d_st + 1, &s0, sizeof(s0), hipMemcpyHostToDevice, c->stream));

    McgArgs a{};
    a.r = vR;
    a.p = vP;
    a.x = vX;
    a.w = m->d_V;
    a.n = n;
    a.n_seg = n_seg;
    a.sgn = sgn;
    for (u32 col = 0; col < nb; ++col) {
        a.sigma[col] = q.shifts[col];
        a.tolb[col] = q.tol * bnorm[col];
    }
    a.pp = pp_part;
    a.pm = m->d_pa;
    a.rr_part = rr_part;
    a.pp_part = pp_part;
    a.st = d_st;
    a.mid = d_mid;

    McgState hs = s0;
    LzxCgLoop lp;
    LZX_TRY(lzx_cg_polled_loop(
        run, d_st, hs, q.maxiter, lp, [&](u32) { return launch_spmm<B>(c, vP, m->d_V, vP); },
        [&](u32 j) {
            hipLaunchKernelGGL(k_mcg_update<B>, dim3(vgrid), blk, 0, c->stream, a, j);
            hipLaunchKernelGGL(k_mcg_direction<B>, dim3(vgrid), blk, 0, c->stream, a, j);
            return LZX_OK;
        },
        [](const McgState &s) { return s.live == 0; }));
    const u32 launched = lp.launched;

    // every x_c: projected onto the complement of W, its true residual (one more SpMM), caller order
    LZX_TRY(project(vX));
    LZX_TRY(launch_spmm<B>(c, vX, m->d_V, nullptr));
    McgSigma sig{};
    for (u32 col = 0; col < nb; ++col) sig.v[col] = q.shifts[col];
    hipLaunchKernelGGL(k_mcg_resid<B>, dim3(vgrid), blk, 0, c->stream, vB, vX, m->d_V, sig, sgn, n, n_seg, rr_part);
    hipLaunchKernelGGL(k_mcg_close<B>, dim3(1), blk, 0, c->stream, rr_part, n_seg, t_rs);
    hipLaunchKernelGGL(k_multi_unpack<B>, dim3(grid_of(nB)), blk, 0, c->stream, vX, nb, n, m->d_V);
    LZX_HIP(hipGetLastError());
    LZX_HIP(hipMemcpyAsync(q.X, m->d_V, sizeof(double) * nb * n, hipMemcpyDeviceToHost, c->stream));
    double rs[LZX_MCG_MAX_NB];
    LZX_HIP(hipMemcpyAsync(rs, t_rs, sizeof(rs), hipMemcpyDeviceToHost, c->stream));
    LZX_HIP(hipStreamSynchronize(c->stream));

    u32 conv = 0, last = 0, first_bad = nb, n_limit = 0;
    for (u32 col = 0; col < nb; ++col) {
        const bool bad = (hs.bad >> col) & 1u, live = (hs.live >> col) & 1u;
        const u32 st = bad ? 2u : live ? 1u : 0u;
        const u32 it = bad ? hs.err_iter[col] : live ? launched : hs.iters[col];
        if (q.iters) q.iters[col] = it;
        if (q.resid) q.resid[col] = std::sqrt(rs[col]) / bnorm[col];
        if (q.status) q.status[col] = st;
        conv += st == 0;
        n_limit += st == 1;
        last = std::max(last, it);
        if (bad && first_bad == nb) first_bad = col;
    }
    if (q.info) {
        q.info->iterations = last;
        q.info->launched = launched;
        q.info->converged = conv;
        q.info->nb = nb;
        q.info->loop_ms = lzx_ms_since(q.t_start);
        q.info->spmv_ms = lp.spmv_ms;
        q.info->vec_ms = lp.vec_ms;
        for (u32 col = 0; col < LZX_MCG_MAX_NB; ++col) q.info->bnorm[col] = bnorm[col];
    }
    if (first_bad < nb)
        LZX_FAIL(LZX_ERR_ARG, "%s: S(sigma) of column %u is not positive definite: p . S p = %.6e at iteration %u (sigma = %.17g)", fn, first_bad,
                 hs.curv[first_bad], hs.err_iter[first_bad], q.shifts[first_bad]);
    if (n_limit)
        LZX_FAIL(LZX_ERR_LIMIT, "%s: %u of %u columns converged in maxiter = %u iterations (tolerance %.3e of ||b_c||)", fn, conv, nb, q.maxiter, q.tol);
    return LZX_OK;
}

extern "C" int lzx_solve_multi_f64(lzx_handle h, uint32_t nb, const double *Bm, const double *shifts, double tol, uint32_t maxiter,
                                   const double *W, uint32_t nw, double *X, uint32_t *iters, double *resid, uint32_t *status,
                                   lzx_solve_multi_info *info)
{
    static const char *fn = "lzx_solve_multi_f64";
    const auto t_start = std::chrono::steady_clock::now();
    if (nb == 0) LZX_FAIL(LZX_ERR_ARG, "%s: nb == 0", fn);
    if (nb > LZX_MCG_MAX_NB) LZX_FAIL(LZX_ERR_LIMIT, "%s: nb = %u right-hand sides (at most %u per call)", fn, nb, LZX_MCG_MAX_NB);
    if (!(tol > 0.0)) LZX_FAIL(LZX_ERR_ARG, "%s: tol must be > 0", fn);
    if (!shifts) LZX_FAIL(LZX_ERR_ARG, "%s: null shifts", fn);
    for (u32 col = 0; col < nb; ++col) {
        if (!std::isfinite(shifts[col])) LZX_FAIL(LZX_ERR_ARG, "%s: shift %u is not finite", fn, col);
        if (shifts[col] < 0.0) LZX_FAIL(LZX_ERR_ARG, "%s: shift %u = %g < 0: S(sigma) is not positive definite", fn, col, shifts[col]);
    }
    if (nw > LZX_MCG_MAX_W) LZX_FAIL(LZX_ERR_LIMIT, "%s: nw = %u deflation vectors (at most %u)", fn, nw, LZX_MCG_MAX_W);
    if (maxiter == 0) LZX_FAIL(LZX_ERR_ARG, "%s: maxiter == 0", fn);
    if (!Bm) LZX_FAIL(LZX_ERR_ARG, "%s: null Bm", fn);
    if (!X) LZX_FAIL(LZX_ERR_ARG, "%s: null X", fn);
    if (nw > 0 && !W) LZX_FAIL(LZX_ERR_ARG, "%s: nw = %u but W is null", fn, nw);
    if (!h) LZX_FAIL(LZX_ERR_ARG, "%s: null handle (h)", fn);
    lzx_ctx *c = h;
    if (c->comm_kind != 0 || c->world > 1)
        LZX_FAIL(LZX_ERR_STATE, "%s: the solver runs on one GPU handle; this handle is rank %d of a communicator of %d", fn, c->rank, c->world);
    const bool lap = c->op_opt == LZX_OP_LAPLACIAN;
    for (u32 col = 0; col < nb; ++col) {
        if (!lap && shifts[col] <= 0.0)
            LZX_FAIL(LZX_ERR_ARG, "%s: shift %u = %g <= 0 under A: sigma I - A is never positive definite there", fn, col, shifts[col]);
        if (lap && shifts[col] == 0.0 && nw == 0)
            LZX_FAIL(LZX_ERR_ARG, "%s: shift %u = 0 under L needs deflation vectors (nw >= 1) spanning the null space b is orthogonal to", fn, col);
    }
    LZX_TRY(lzx_multi_check_handle(c, fn));
    LZX_TRY(lzx_multi_build_tables(c));
    const McgCall q{nb, Bm, shifts, tol, maxiter, W, nw, X, iters, resid, status, info, t_start};
    switch (lzx_multi_pad_width(nb)) {
    case 2: return mcg_run<2>(c, q, fn);
    case 4: return mcg_run<4>(c, q, fn);
    case 8: return mcg_run<8>(c, q, fn);
    default: return mcg_run<16>(c, q, fn);
    }
}
