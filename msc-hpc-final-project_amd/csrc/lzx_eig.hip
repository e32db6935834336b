// lzx_eig.hip -- extreme eigenpairs of the handle's operator M (A, or L = D - A under option "operator") by thick-restart
// Lanczos (Wu-Simon; Krylov-Schur in the symmetric case) with full re-orthogonalisation: include/lzx.h, lzx_eigsh_f64;
// DESIGN.md section 12.
//
// Layout.  One basis on the device, internal vertex order, stride ldq (= n_loc_pad + LZX_TAIL, the tail and the padding rows
// exactly 0): the nw deflation columns W first, then up to m + 1 Lanczos columns.  The SpMV of the single-vector path reads a
// basis column directly (one rank: the exchange layout is the hand-over layout).
//
// One Lanczos step j (J = nw + j + 1 columns to orthogonalise against), no host synchronisation inside a restart cycle:
//   SpMV (+ k_lap_apply under L)            w = M q_j into d_v
//   k_eig_proj, k_eig_close                 h1 = Q_J^T w        (column tiles of 8: each basis column read once, w once per tile)
//   k_eig_update                            w -= Q_J h1
//   k_eig_proj, k_eig_close                 h2 = Q_J^T w; column j of H = h1 + h2 (Lanczos rows only)
//   k_eig_update (+ norm partials)          w -= Q_J h2
//   k_eig_scale                             beta_j closed in the prologue; breakdown rule; q_{j+1} = w / beta_j
// Classical Gram-Schmidt twice (CGS2): the basis is read four times per step.  Every reduction has a fixed shape (per-workgroup
// partials closed by block_sum_fixed_256), so runs are bit-identical.
//
// Restart (host, once per cycle): H and beta come back in one copy, T = (H + H^T) / 2 is diagonalised by cyclic Jacobi
// (sym_eig below), the p wanted-most Ritz vectors are formed in place by k_eig_rotate (Q[:, 0:p] <- Q[:, 0:m] Y), q_m moves
// to column p, and H restarts as diag(theta) with the coupling beta_{m-1} Y[m-1, i] in row p; the device's own projection
// coefficients of step p supply the matching column.  A breakdown (beta_j <= 2^-40 * the Gershgorin bound) ends the cycle
// early: its Ritz pairs are exact, and the next cycle starts from a fresh probe orthogonalised against what is kept (the next
// probe of the seed that does not lie in that span) -- unless W and the cycle's columns already span R^n (m + nw == n), where
// the run ends.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "lzx_internal.h"
#include "lzx_graph_call.h"
#include "lzx_spmv_body.h"
#include "lzx_reduce.h"
#include "lzx_test_hooks.h"

static constexpr u32 LZX_EIG_CT = 8;          // basis columns per tile of the projection / update kernels
static constexpr u32 LZX_EIG_ROT_ROWS = 64;   // rows one workgroup of k_eig_rotate stages in LDS
static constexpr u32 LZX_EIG_MAX_M = 128;
static constexpr u32 LZX_EIG_MAX_W = 8;
static constexpr u32 LZX_EIG_FRESH_TRIES = 64;   // probes tried for a fresh start before the span of the basis counts as all there is
typedef double nt_double2 __attribute__((ext_vector_type(2)));   // what __builtin_nontemporal_load takes for a 16-byte load

__device__ __forceinline__ double2 load_nt2(const double *p)
{
    const nt_double2 v = __builtin_nontemporal_load(reinterpret_cast<const nt_double2 *>(p));
    return make_double2(v.x, v.y);
}

// ==================================================================================================== kernels
// Partials of h = Q[:, 0:J]^T w.  Workgroup (b, t) covers rows b * 512 + k * G * 512 (two per thread) of column tile t:
// part[c * G + b] for the tile's columns c.  Columns are unit-stride streams read once, with non-temporal loads.
__global__ void __launch_bounds__(LZX_VEC_BLOCK)
k_eig_proj(const double *__restrict__ Q, u32 ldq, u32 J, const double *__restrict__ w, u32 n, double *part)
{
    __shared__ double sh[4][LZX_EIG_CT];
    const u32 G = gridDim.x, b = blockIdx.x, c0 = blockIdx.y * LZX_EIG_CT;
    const u32 nc = std::min<u32>(LZX_EIG_CT, J - c0);
    double acc[LZX_EIG_CT];
#pragma unroll
    for (u32 u = 0; u < LZX_EIG_CT; ++u) acc[u] = 0.0;
    const u32 stride = G * LZX_VEC_BLOCK * 2;
    for (u32 i = (b * LZX_VEC_BLOCK + threadIdx.x) * 2; i < n; i += stride) {
        const double2 x = *reinterpret_cast<const double2 *>(w + i);
        double2 q[LZX_EIG_CT];
#pragma unroll
        for (u32 u = 0; u < LZX_EIG_CT; ++u)
            q[u] = u < nc ? load_nt2(Q + (size_t)(c0 + u) * ldq + i) : make_double2(0.0, 0.0);
#pragma unroll
        for (u32 u = 0; u < LZX_EIG_CT; ++u) {
            acc[u] += q[u].x * x.x;
            acc[u] += q[u].y * x.y;
        }
    }
#pragma unroll
    for (u32 u = 0; u < LZX_EIG_CT; ++u) {
        const double s = wave_sum(acc[u]);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][u] = s;
    }
    __syncthreads();
    if (threadIdx.x < nc) {
        const u32 u = threadIdx.x;
        part[(size_t)(c0 + u) * G + b] = ((sh[0][u] + sh[1][u]) + sh[2][u]) + sh[3][u];
    }
}

// h[c] = sum of part[c * G .. c * G + G) in the fixed order (workgroup c).  hsum != nullptr (second pass): hsum[c - nw] =
// h_prev[c] + h[c] for the Lanczos columns c >= nw -- column j of the projected matrix.
__global__ void __launch_bounds__(LZX_VEC_BLOCK)
k_eig_close(const double *part, u32 G, double *h, const double *h_prev, double *hsum, u32 nw)
{
    __shared__ double sh[4];
    const u32 c = blockIdx.x;
    const double s = block_sum_fixed_256(part + (size_t)c * G, G, sh);
    if (threadIdx.x == 0) {
        h[c] = s;
        if (hsum && c >= nw) hsum[c - nw] = h_prev[c] + s;
    }
}

// w -= sum_c h[c] q_c over the J columns (ascending c), and, with npart != nullptr, per-workgroup partials of ||w||^2.
__global__ void __launch_bounds__(LZX_VEC_BLOCK)
k_eig_update(const double *__restrict__ Q, u32 ldq, u32 J, const double *__restrict__ h, double *w, u32 n, double *npart)
{
    __shared__ double sh[4];
    double nrm = 0.0;
    const u32 stride = gridDim.x * LZX_VEC_BLOCK * 2;
    for (u32 i = (blockIdx.x * LZX_VEC_BLOCK + threadIdx.x) * 2; i < n; i += stride) {
        double2 x = *reinterpret_cast<const double2 *>(w + i);
        u32 c = 0;
        for (; c + LZX_EIG_CT <= J; c += LZX_EIG_CT) {
            double2 q[LZX_EIG_CT];
#pragma unroll
            for (u32 u = 0; u < LZX_EIG_CT; ++u)
                q[u] = load_nt2(Q + (size_t)(c + u) * ldq + i);
#pragma unroll
            for (u32 u = 0; u < LZX_EIG_CT; ++u) {
                const double hc = h[c + u];
                x.x -= hc * q[u].x;
                x.y -= hc * q[u].y;
            }
        }
        for (; c < J; ++c) {
            const double2 q = load_nt2(Q + (size_t)c * ldq + i);
            const double hc = h[c];
            x.x -= hc * q.x;
            x.y -= hc * q.y;
        }
        *reinterpret_cast<double2 *>(w + i) = x;
        nrm += x.x * x.x;
        nrm += x.y * x.y;
    }
    if (!npart) return;
    block_partial(nrm, sh, npart);
}

// beta = sqrt(sum of npart) closed by every workgroup; beta <= stop: beta = 0 and q_next = 0 (the breakdown rule);
// otherwise q_next = w / beta (may be w itself).
__global__ void __launch_bounds__(LZX_VEC_BLOCK)
k_eig_scale(const double *w, double *q_next, const double *npart, u32 np, double *beta_out, u32 n, double stop)
{
    __shared__ double sh[4];
    double beta = sqrt(block_sum_fixed_256(npart, np, sh));
    const bool zero = beta <= stop;
    if (zero) beta = 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0 && beta_out) *beta_out = beta;
    const u32 stride = gridDim.x * LZX_VEC_BLOCK * 2;
    for (u32 i = (blockIdx.x * LZX_VEC_BLOCK + threadIdx.x) * 2; i < n; i += stride) {
        double2 x = *reinterpret_cast<const double2 *>(w + i);
        x.x /= beta;
        x.y /= beta;
        if (zero) x = make_double2(0.0, 0.0);
        *reinterpret_cast<double2 *>(q_next + i) = x;
    }
}

// Q[:, 0:p] <- Q[:, 0:m] Y, in place (out == Q) or into out.  Y: [m][ldy] row-major, ldy a multiple of 8, columns >= p zero.
// A workgroup stages its 64 rows of all m input columns in LDS (each row is owned by one workgroup, so nothing it reads is
// overwritten by another); its four wavefronts then take the output columns in groups of 8, one row per lane.
__global__ void __launch_bounds__(LZX_VEC_BLOCK)
k_eig_rotate(const double *Q, u32 ldq, u32 m, const double *__restrict__ Y, u32 ldy, u32 p, double *out, u32 ldo)
{
    extern __shared__ double qs[];   // [m][64]
    const u32 r0 = blockIdx.x * LZX_EIG_ROT_ROWS;
    for (u32 e = threadIdx.x; e < m * LZX_EIG_ROT_ROWS; e += LZX_VEC_BLOCK)
        qs[e] = Q[(size_t)(e / LZX_EIG_ROT_ROWS) * ldq + r0 + e % LZX_EIG_ROT_ROWS];
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u32 c0 = wave * LZX_EIG_CT; c0 < p; c0 += 4 * LZX_EIG_CT) {
        double acc[LZX_EIG_CT];
#pragma unroll
        for (u32 u = 0; u < LZX_EIG_CT; ++u) acc[u] = 0.0;
        for (u32 k = 0; k < m; ++k) {
            const double q = qs[k * LZX_EIG_ROT_ROWS + lane];
            const double *y = Y + (size_t)k * ldy + c0;
#pragma unroll
            for (u32 u = 0; u < LZX_EIG_CT; ++u) acc[u] += q * y[u];
        }
#pragma unroll
        for (u32 u = 0; u < LZX_EIG_CT; ++u)
            if (c0 + u < p) out[(size_t)(c0 + u) * ldo + r0 + lane] = acc[u];
    }
}

// partials of ||v - theta x||^2
__global__ void __launch_bounds__(LZX_VEC_BLOCK)
k_eig_resid(const double *__restrict__ v, const double *__restrict__ x, double theta, u32 n, double *npart)
{
    __shared__ double sh[4];
    double s = 0.0;
    const u32 stride = gridDim.x * LZX_VEC_BLOCK * 2;
    for (u32 i = (blockIdx.x * LZX_VEC_BLOCK + threadIdx.x) * 2; i < n; i += stride) {
        const double2 a = *reinterpret_cast<const double2 *>(v + i);
        const double2 b = *reinterpret_cast<const double2 *>(x + i);
        const double dx = a.x - theta * b.x, dy = a.y - theta * b.y;
        s += dx * dx;
        s += dy * dy;
    }
    block_partial(s, sh, npart);
}

// probe p of seed in the caller's order (include/lzx.h: lzx_probes_f64)
__global__ void k_eig_probe(u64 seed, u64 p, u64 n, double *io)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) io[i] = lzx_probe_value(seed, p, i);
}

// ==================================================================================================== host: dense solver
// Cyclic Jacobi on the symmetric n x n matrix A (row-major, destroyed): eigenvalues ascending into w, eigenvectors as the
// columns of V (row-major, V[i * n + j] = component i of vector j).  Rotations as in Golub / Van Loan 8.5 (the smaller angle);
// sweeps until the off-diagonal mass is below (eps^2 / 4) of the whole.
static void sym_eig(u32 n, std::vector<double> &A, double *w, double *V)
{
    std::vector<double> Z((size_t)n * n, 0.0);
    for (u32 i = 0; i < n; ++i) Z[(size_t)i * n + i] = 1.0;
    auto a = [&](u32 i, u32 j) -> double & { return A[(size_t)i * n + j]; };
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0, fro = 0.0;
        for (u32 i = 0; i < n; ++i)
            for (u32 j = 0; j < n; ++j) {
                const double x = a(i, j) * a(i, j);
                fro += x;
                if (i != j) off += x;
            }
        if (off <= 1e-34 * fro || off == 0.0) break;
        for (u32 p = 0; p + 1 < n; ++p)
            for (u32 q = p + 1; q < n; ++q) {
                const double apq = a(p, q);
                if (apq == 0.0) continue;
                const double tau = (a(q, q) - a(p, p)) / (2.0 * apq);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                for (u32 k = 0; k < n; ++k) {   // A <- A J (columns p, q)
                    const double akp = a(k, p), akq = a(k, q);
                    a(k, p) = c * akp - s * akq;
                    a(k, q) = s * akp + c * akq;
                }
                for (u32 k = 0; k < n; ++k) {   // A <- J^T A (rows p, q)
                    const double apk = a(p, k), aqk = a(q, k);
                    a(p, k) = c * apk - s * aqk;
                    a(q, k) = s * apk + c * aqk;
                }
                a(p, q) = a(q, p) = 0.0;
                for (u32 k = 0; k < n; ++k) {
                    const double zp = Z[(size_t)k * n + p], zq = Z[(size_t)k * n + q];
                    Z[(size_t)k * n + p] = c * zp - s * zq;
                    Z[(size_t)k * n + q] = s * zp + c * zq;
                }
            }
    }
    std::vector<u32> ord(n);
    for (u32 i = 0; i < n; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](u32 x, u32 y) { return a(x, x) < a(y, y); });
    for (u32 j = 0; j < n; ++j) {
        w[j] = a(ord[j], ord[j]);
        for (u32 i = 0; i < n; ++i) V[(size_t)i * n + j] = Z[(size_t)i * n + ord[j]];
    }
}

extern "C" int lzx_test_sym_eig(uint32_t n, const double *A, double *w, double *V)
{
    if (n == 0 || n > 1024 || !A || !w || !V) LZX_FAIL(LZX_ERR_ARG, "lzx_test_sym_eig: bad argument");
    std::vector<double> a(A, A + (size_t)n * n);
    sym_eig(n, a, w, V);
    return LZX_OK;
}

// ==================================================================================================== host: shared CGS2
// (include/lzx_internal.h: the solver of lzx_solve.hip deflates with the same launches)
static int launch_proj(lzx_ctx *c, const double *Q, u32 J, const double *w, u32 G, double *part)
{
    hipLaunchKernelGGL(k_eig_proj, dim3(G, (J + LZX_EIG_CT - 1) / LZX_EIG_CT), dim3(LZX_VEC_BLOCK), 0, c->stream, Q, c->ldq, J, w, c->n_loc_pad, part);
    LZX_HIP(hipGetLastError());
    return LZX_OK;
}

static int launch_update(lzx_ctx *c, const double *Q, u32 J, const double *h, double *w, u32 G, double *npart)
{
    hipLaunchKernelGGL(k_eig_update, dim3(G), dim3(LZX_VEC_BLOCK), 0, c->stream, Q, c->ldq, J, h, w, c->n_loc_pad, npart);
    LZX_HIP(hipGetLastError());
    return LZX_OK;
}

u32 lzx_cgs_grid(const lzx_ctx *c)
{
    return std::max<u32>(1u, std::min<u32>((u32)c->cu_count * 4u, (c->n_loc_pad + 2 * LZX_VEC_BLOCK - 1) / (2 * LZX_VEC_BLOCK)));
}

int lzx_cgs2(lzx_ctx *c, const double *Q, u32 J, double *w, const LzxCgsScratch &s, double *hsum, u32 nw)
{
    if (J == 0) return launch_update(c, Q, 0, s.h1, w, s.G, s.npart);
    LZX_TRY(launch_proj(c, Q, J, w, s.G, s.part));
    hipLaunchKernelGGL(k_eig_close, dim3(J), dim3(LZX_VEC_BLOCK), 0, c->stream, s.part, s.G, s.h1, nullptr, nullptr, 0u);
    LZX_TRY(launch_update(c, Q, J, s.h1, w, s.G, nullptr));
    LZX_TRY(launch_proj(c, Q, J, w, s.G, s.part));
    hipLaunchKernelGGL(k_eig_close, dim3(J), dim3(LZX_VEC_BLOCK), 0, c->stream, s.part, s.G, s.h2, s.h1, hsum, nw);
    return launch_update(c, Q, J, s.h2, w, s.G, s.npart);
}

int lzx_cgs_normalise(lzx_ctx *c, const double *w, double *q, const LzxCgsScratch &s, double *beta_out, double stop)
{
    hipLaunchKernelGGL(k_eig_scale, dim3(s.G), dim3(LZX_VEC_BLOCK), 0, c->stream, w, q, s.npart, s.G, beta_out, c->n_loc_pad, stop);
    LZX_HIP(hipGetLastError());
    return LZX_OK;
}

int lzx_cgs_orthonormalise(lzx_ctx *c, double *Q, u32 i, const LzxCgsScratch &s, double *beta_out)
{
    double *q = Q + (size_t)i * c->ldq;
    LZX_TRY(launch_update(c, Q, 0, s.h1, q, s.G, s.npart));
    LZX_TRY(lzx_cgs_normalise(c, q, q, s, nullptr, -1.0));
    LZX_TRY(lzx_cgs2(c, Q, i, q, s));
    return lzx_cgs_normalise(c, q, q, s, beta_out, 1e-10);
}

// ==================================================================================================== host: driver
namespace {
struct EigRun {
    lzx_ctx *c = nullptr;
    u32 nw = 0, m = 0, G = 0;
    double *d_B = nullptr;       // [nw + m + 1][ldq]
    double *d_s = nullptr;       // scratch, carved below
    double *part = nullptr;      // [Jmax][G]
    double *h1 = nullptr, *h2 = nullptr;   // [Jmax]
    double *H = nullptr;         // [m][m]: column j at H + j * m (rows 0 .. j)
    double *beta = nullptr;      // [m]
    double *npart = nullptr;     // [G]
    double *Y = nullptr;         // [m][ldy]
    double *tmp = nullptr;       // [16]: betas of the set-up normalisations (start vector, W columns), residuals
    std::vector<hipEvent_t> ev;  // [2 m + 1]: before the first step of a cycle, then behind every step's SpMV and its scale
    double spmv_ms = 0.0, orth_ms = 0.0;
    bool lap = false;
    double *col(u32 i) const { return d_B + (size_t)i * c->ldq; }
    ~EigRun()
    {
        if (c) {
            (void)hipSetDevice(c->device);
            (void)hipStreamSynchronize(c->stream);
        }
        if (d_B) (void)hipFree(d_B);
        if (d_s) (void)hipFree(d_s);
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }

    int spmv(const double *x)
    {
        SpmvLaunch l{x, x, c->d_v, c->d_partials};
        LZX_TRY(lzx_launch_spmv(c, l));
        if (lap) LZX_TRY(lzx_launch_lap_apply(c, c->d_v, x, nullptr, 0, c->n_loc_pad));
        return LZX_OK;
    }
    // the basis of nw + m + 1 columns and the scratch behind it, both zeroed (c, nw, m set by the caller): the padding rows
    // and tails of the basis stay 0 from here on
    int alloc(const char *fn)
    {
        const u64 basis_bytes = (u64)(nw + m + 1) * c->ldq * sizeof(double);
        char what[64];
        std::snprintf(what, sizeof what, "the basis of (nw + m + 1) = %u columns", nw + m + 1);
        LZX_TRY(lzx_alloc_state(fn, what, c->eig_basis_cap_opt, basis_bytes, basis_bytes, (void **)&d_B));
        G = lzx_cgs_grid(c);
        const u32 Jmax = nw + m + 1;
        const u64 scratch = (u64)Jmax * G + 2ull * Jmax + (u64)m * m + m + G + (u64)m * ldy() + 16;
        LZX_HIP(hipMalloc(reinterpret_cast<void **>(&d_s), sizeof(double) * scratch));
        part = d_s;
        h1 = part + (size_t)Jmax * G;
        h2 = h1 + Jmax;
        H = h2 + Jmax;
        beta = H + (size_t)m * m;
        npart = beta + m;
        Y = npart + G;
        tmp = Y + (size_t)m * ldy();
        LZX_HIP(hipMemsetAsync(d_B, 0, basis_bytes, c->stream));
        LZX_HIP(hipMemsetAsync(d_s, 0, sizeof(double) * scratch, c->stream));
        return LZX_OK;
    }
    u32 ldy() const { return (m + LZX_EIG_CT - 1) / LZX_EIG_CT * LZX_EIG_CT; }   // row stride of Y
    LzxCgsScratch scratch() const { return LzxCgsScratch{G, part, h1, h2, npart}; }
    // w orthogonalised against columns [0, J) by CGS2, the norm partials of the result in npart; hsum: column of H
    int orth(double *w, u32 J, double *hsum) { return lzx_cgs2(c, d_B, J, w, scratch(), hsum, nw); }
    int scale(const double *w, double *q, double *beta_out, double stop) { return lzx_cgs_normalise(c, w, q, scratch(), beta_out, stop); }
    int rotate(u32 first, u32 min_, const std::vector<double> &Yh, u32 ldy, u32 p)
    {
        LZX_HIP(hipMemcpyAsync(Y, Yh.data(), sizeof(double) * min_ * ldy, hipMemcpyHostToDevice, c->stream));
        const size_t lds = sizeof(double) * min_ * LZX_EIG_ROT_ROWS;
        hipLaunchKernelGGL(k_eig_rotate, dim3(c->n_loc_pad / LZX_EIG_ROT_ROWS), dim3(LZX_VEC_BLOCK), lds, c->stream, col(first), c->ldq, min_, Y, ldy,
                           p, col(first), c->ldq);
        LZX_HIP(hipGetLastError());
        return LZX_OK;
    }
    // column i (which already holds a vector) made unit, orthogonalised against columns [0, i), made unit again; the
    // final beta goes to tmp[slot] (0: the vector lay in their span)
    int orthonormalise(u32 i, u32 slot) { return lzx_cgs_orthonormalise(c, d_B, i, scratch(), tmp + slot); }
    // fresh start in column i: probe p of seed (x0 == nullptr) or x0, orthonormalised against [0, i); returns its beta
    int start(u32 i, const double *x0, u64 seed, u64 p, double *beta_host)
    {
        if (x0) LZX_HIP(hipMemcpyAsync(c->d_io, x0, sizeof(double) * c->n, hipMemcpyHostToDevice, c->stream));
        else hipLaunchKernelGGL(k_eig_probe, dim3((u32)((c->n + 255) / 256)), dim3(256), 0, c->stream, seed, p, c->n, c->d_io);
        LZX_HIP(hipGetLastError());
        LZX_HIP(hipMemsetAsync(col(i), 0, sizeof(double) * c->ldq, c->stream));
        LZX_TRY(lzx_launch_permute_in(c, c->d_io, col(i), 1.0));
        LZX_TRY(orthonormalise(i, 0));
        LZX_HIP(hipMemcpyAsync(beta_host, tmp, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        LZX_HIP(hipStreamSynchronize(c->stream));
        return LZX_OK;
    }
    // Lanczos steps [j0, m) of a cycle, queued without a host synchronisation; event marks around every SpMV
    int steps(u32 j0, double stop)
    {
        LZX_HIP(hipEventRecord(ev[2 * j0], c->stream));
        for (u32 j = j0; j < m; ++j) {
            LZX_TRY(spmv(col(nw + j)));
            LZX_HIP(hipEventRecord(ev[2 * j + 1], c->stream));
            LZX_TRY(orth(c->d_v, nw + j + 1, H + (size_t)j * m));
            LZX_TRY(scale(c->d_v, col(nw + j + 1), beta + j, stop));
            LZX_HIP(hipEventRecord(ev[2 * j + 2], c->stream));
        }
        return LZX_OK;
    }
    // after the cycle's stream synchronisation: the marks' intervals billed to SpMV / orthogonalisation
    int bill(u32 j0)
    {
        for (u32 j = j0; j < m; ++j) {
            float a = 0.f, b = 0.f;
            LZX_HIP(hipEventElapsedTime(&a, ev[2 * j], ev[2 * j + 1]));
            LZX_HIP(hipEventElapsedTime(&b, ev[2 * j + 1], ev[2 * j + 2]));
            spmv_ms += a;
            orth_ms += b;
        }
        return LZX_OK;
    }
};
}  // namespace

extern "C" int lzx_eigsh_f64(lzx_handle h, uint32_t nev, int which, uint32_t m, double tol, uint32_t max_restarts, const double *x0,
                             uint64_t seed, const double *W, uint32_t nw, double *evals, double *evecs, double *resid, lzx_eig_info *info)
{
    static const char *fn = "lzx_eigsh_f64";
    if (nev == 0) LZX_FAIL(LZX_ERR_ARG, "%s: nev == 0", fn);
    if (which != LZX_EIG_LARGEST && which != LZX_EIG_SMALLEST) LZX_FAIL(LZX_ERR_ARG, "%s: unknown which = %d", fn, which);
    if (!(tol > 0.0)) LZX_FAIL(LZX_ERR_ARG, "%s: tol must be > 0", fn);
    if (m > LZX_EIG_MAX_M) LZX_FAIL(LZX_ERR_LIMIT, "%s: m = %u (at most %u)", fn, m, LZX_EIG_MAX_M);
    if (nw > LZX_EIG_MAX_W) LZX_FAIL(LZX_ERR_LIMIT, "%s: nw = %u deflation vectors (at most %u)", fn, nw, LZX_EIG_MAX_W);
    if (!h) LZX_FAIL(LZX_ERR_ARG, "%s: null handle (h)", fn);
    if (!evals) LZX_FAIL(LZX_ERR_ARG, "%s: null evals", fn);
    if (nw > 0 && !W) LZX_FAIL(LZX_ERR_ARG, "%s: nw = %u but W is null", fn, nw);
    lzx_ctx *c = h;
    if (c->comm_kind != 0 || c->world > 1)
        LZX_FAIL(LZX_ERR_STATE, "%s: the eigensolver runs on one GPU handle; this handle is rank %d of a communicator of %d", fn, c->rank, c->world);
    if (!c->d_row_ptr || !c->d_v) LZX_FAIL(LZX_ERR_STATE, "%s: no graph has been handed over", fn);
    const u64 n = c->n;
    if (m == 0) m = (u32)std::min<u64>(std::min<u64>(LZX_EIG_MAX_M, n > nw ? n - nw : 0), std::max<u64>(2ull * nev + 1, 20));
    if ((u64)nev + 2 > m) LZX_FAIL(LZX_ERR_ARG, "%s: m = %u, but nev + 2 <= m is needed (nev = %u)", fn, m, nev);
    if ((u64)m + nw > n) LZX_FAIL(LZX_ERR_ARG, "%s: m + nw = %u exceeds n = %llu", fn, m + nw, (unsigned long long)n);
    const auto t_start = std::chrono::steady_clock::now();

    EigRun r;
    r.c = c;
    r.nw = nw;
    r.m = m;
    r.lap = c->op_opt == LZX_OP_LAPLACIAN;
    LZX_HIP(hipSetDevice(c->device));
    if (r.lap) LZX_TRY(lzx_ensure_degrees(c));
    // like lzx_spmv_f64: d_v / d_partials / d_io are overwritten, so a prepared decomposition is void (the resident basis,
    // its alpha / beta and the batch state are not touched)
    c->k_prep = 0;

    LZX_TRY(r.alloc(fn));
    const u32 ldy = r.ldy();
    for (u32 i = 0; i < 2 * m + 1; ++i) {
        hipEvent_t ev;
        LZX_HIP(hipEventCreate(&ev));
        r.ev.push_back(ev);
    }

    // deflation vectors: uploaded, orthonormalised in order on the device
    for (u32 t = 0; t < nw; ++t) {
        LZX_HIP(hipMemcpyAsync(c->d_io, W + (size_t)t * n, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
        LZX_TRY(lzx_launch_permute_in(c, c->d_io, r.col(t), 1.0));
        LZX_TRY(r.orthonormalise(t, 1 + t));
    }
    if (nw > 0) {
        double b[LZX_EIG_MAX_W];
        LZX_HIP(hipMemcpyAsync(b, r.tmp + 1, sizeof(double) * nw, hipMemcpyDeviceToHost, c->stream));
        LZX_HIP(hipStreamSynchronize(c->stream));
        for (u32 t = 0; t < nw; ++t)
            if (!(b[t] > 0.0)) LZX_FAIL(LZX_ERR_ARG, "%s: W is rank-deficient (column %u lies in the span of the columns before it)", fn, t);
    }
    double b0 = 0.0;
    if (x0 && !std::any_of(x0, x0 + n, [](double v) { return v != 0.0; })) LZX_FAIL(LZX_ERR_ARG, "%s: x0 is all zero", fn);
    LZX_TRY(r.start(nw, x0, seed, 0, &b0));
    if (!(b0 > 0.0)) LZX_FAIL(LZX_ERR_ARG, "%s: the start vector lies in the span of W", fn);

    // Gershgorin bound of ||M||: the breakdown threshold
    const double g = (r.lap ? 2.0 : 1.0) * (double)c->max_degree;
    const double stop = ldexp(g, -40);
    std::vector<double> Hh((size_t)m * m, 0.0), Hd((size_t)m * m), bh(m), T, th(m), Yfull((size_t)m * m), Yr;
    std::vector<u32> ord(m);
    u32 k = 0, restarts = 0, matvecs = 0, me = m, conv = 0;
    u64 fresh = 0;   // probes used for fresh starts so far (probe 0 was the first start vector)
    double norm_est = 0.0, host_ms = 0.0, worst = 0.0;
    std::vector<double> res(m, 0.0);
    bool exhausted = false;
    for (;;) {
        LZX_TRY(r.steps(k, stop));
        matvecs += m - k;
        LZX_HIP(hipMemcpyAsync(Hd.data(), r.H, sizeof(double) * m * m, hipMemcpyDeviceToHost, c->stream));
        LZX_HIP(hipMemcpyAsync(bh.data(), r.beta, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
        LZX_HIP(hipStreamSynchronize(c->stream));
        LZX_TRY(r.bill(k));
        const auto th0 = std::chrono::steady_clock::now();
        // the cycle's steps: column j of H (rows 0 .. j) from the device, beta_j below the diagonal; trimmed at a breakdown
        me = m;
        for (u32 j = k; j < m; ++j)
            if (bh[j] == 0.0) {
                me = j + 1;
                break;
            }
        const bool brk = bh[me - 1] == 0.0;
        for (u32 j = k; j < me; ++j) {
            for (u32 i = 0; i <= j; ++i) Hh[(size_t)i * m + j] = Hd[(size_t)j * m + i];
            if (j + 1 < m) Hh[(size_t)(j + 1) * m + j] = bh[j];
        }
        T.assign((size_t)me * me, 0.0);
        for (u32 i = 0; i < me; ++i)
            for (u32 j = 0; j < me; ++j) T[(size_t)i * me + j] = 0.5 * (Hh[(size_t)i * m + j] + Hh[(size_t)j * m + i]);
        std::vector<double> Yc((size_t)me * me), tc(me);
        sym_eig(me, T, tc.data(), Yc.data());
        ord.resize(me);
        for (u32 i = 0; i < me; ++i) ord[i] = which == LZX_EIG_LARGEST ? me - 1 - i : i;   // wanted-most first
        for (u32 i = 0; i < me; ++i) {
            th[i] = tc[ord[i]];
            for (u32 a = 0; a < me; ++a) Yfull[(size_t)a * m + i] = Yc[(size_t)a * me + ord[i]];
            norm_est = std::max(norm_est, std::fabs(th[i]));
        }
        conv = 0;
        worst = 0.0;
        for (u32 i = 0; i < std::min(nev, me); ++i) {
            res[i] = std::fabs(bh[me - 1] * Yfull[(size_t)(me - 1) * m + i]);
            worst = std::max(worst, res[i]);
            if (res[i] <= tol * norm_est) ++conv;
        }
        const bool done = !brk && conv >= nev;
        // a breakdown with W and the cycle's columns spanning all of R^n (m + nw == n at the latest): the Ritz pairs are every
        // eigenpair of the complement of W, and a fresh probe could only break down again
        if (brk && (u64)me + nw >= n) exhausted = true;
        if (done || restarts >= max_restarts || exhausted) {
            host_ms += lzx_ms_since(th0);
            break;
        }
        // thick restart: keep p wanted-most Ritz vectors
        const u32 p = std::min(nev + (m - nev) / 2, me);
        Yr.assign((size_t)me * ldy, 0.0);
        for (u32 a = 0; a < me; ++a)
            for (u32 i = 0; i < p; ++i) Yr[(size_t)a * ldy + i] = Yfull[(size_t)a * m + i];
        std::fill(Hh.begin(), Hh.end(), 0.0);
        for (u32 i = 0; i < p; ++i) Hh[(size_t)i * m + i] = th[i];
        if (!brk)
            for (u32 i = 0; i < p; ++i) Hh[(size_t)p * m + i] = bh[m - 1] * Yfull[(size_t)(m - 1) * m + i];
        host_ms += lzx_ms_since(th0);
        LZX_HIP(hipEventRecord(r.ev[0], c->stream));
        LZX_TRY(r.rotate(nw, me, Yr, ldy, p));
        if (!brk) LZX_HIP(hipMemcpyAsync(r.col(nw + p), r.col(nw + m), sizeof(double) * c->ldq, hipMemcpyDeviceToDevice, c->stream));
        LZX_HIP(hipEventRecord(r.ev[1], c->stream));
        LZX_HIP(hipEventSynchronize(r.ev[1]));
        float a = 0.f;
        LZX_HIP(hipEventElapsedTime(&a, r.ev[0], r.ev[1]));
        r.orth_ms += a;
        if (brk) {
            // W and the kept columns do not span R^n here (me + nw < n), but one +-1 probe can lie in their span by accident: with
            // three vertices and the columns (1, -1, 0), (0, 0, 1) every second one does, and taking that for "nothing new to
            // explore" returned 0 as the largest eigenvalue of an edge beside an isolated vertex.  So the following probes are tried.
            double bx = 0.0;
            for (u32 t = 0; t < LZX_EIG_FRESH_TRIES && !(bx > 0.0); ++t) LZX_TRY(r.start(nw + p, nullptr, seed, ++fresh, &bx));
            if (!(bx > 0.0)) exhausted = true;   // nothing new to explore: the next cycle is the last
        }
        LZX_HIP(hipMemsetAsync(r.beta, 0, sizeof(double) * m, c->stream));
        k = p;
        ++restarts;
    }

    // Ritz vectors V = Q Y[:, 0:nev] in place, then residuals (one SpMV each), caller order, sign fixed
    const u32 nout = std::min(nev, me);
    Yr.assign((size_t)me * ldy, 0.0);
    for (u32 a = 0; a < me; ++a)
        for (u32 i = 0; i < nout; ++i) Yr[(size_t)a * ldy + i] = Yfull[(size_t)a * m + i];
    LZX_TRY(r.rotate(nw, me, Yr, ldy, nout));
    std::vector<double> rs(nout, 0.0);
    for (u32 i = 0; i < nout; ++i) {
        LZX_TRY(r.spmv(r.col(nw + i)));
        hipLaunchKernelGGL(k_eig_resid, dim3(r.G), dim3(LZX_VEC_BLOCK), 0, c->stream, c->d_v, r.col(nw + i), th[i], c->n_loc_pad, r.npart);
        hipLaunchKernelGGL(k_eig_close, dim3(1), dim3(LZX_VEC_BLOCK), 0, c->stream, r.npart, r.G, r.tmp, nullptr, nullptr, 0u);
        LZX_HIP(hipGetLastError());
        LZX_HIP(hipMemcpyAsync(&rs[i], r.tmp, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (evecs) {
            LZX_TRY(lzx_launch_permute_out(c, r.col(nw + i), c->d_io));
            LZX_HIP(hipMemcpyAsync(evecs + (size_t)i * n, c->d_io, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        }
        LZX_HIP(hipStreamSynchronize(c->stream));
        if (evecs) {
            double *v = evecs + (size_t)i * n;
            u64 at = 0;
            for (u64 q = 1; q < n; ++q)
                if (std::fabs(v[q]) > std::fabs(v[at])) at = q;
            if (v[at] < 0.0)
                for (u64 q = 0; q < n; ++q) v[q] = -v[q];
        }
    }
    for (u32 i = 0; i < nev; ++i) {
        evals[i] = i < nout ? th[i] : NAN;
        if (resid) resid[i] = i < nout ? std::sqrt(rs[i]) : NAN;
        if (evecs && i >= nout) std::fill(evecs + (size_t)i * n, evecs + (size_t)(i + 1) * n, 0.0);
    }
    if (info) {
        info->converged = std::min(conv, nev);
        info->restarts = restarts;
        info->matvecs = matvecs;
        info->m = m;
        info->loop_ms = lzx_ms_since(t_start);
        info->spmv_ms = r.spmv_ms;
        info->orth_ms = r.orth_ms;
        info->host_ms = host_ms;
        info->norm_est = norm_est;
    }
    if (conv < nev)
        LZX_FAIL(LZX_ERR_LIMIT, "%s: %u of %u pairs converged after %u restarts (largest residual estimate %.3e, tolerance %.3e)", fn, conv, nev,
                 restarts, worst, tol * norm_est);
    return LZX_OK;
}

// ==================================================================================================== test hook
// (lzx_test_hooks.h) The dense launches above on a caller's basis: an EigRun with nw = 0 and m = J holds the J columns of Q and,
// as its column J, w -- laid out, orthogonalised, scaled and rotated by the driver's own member functions.
extern "C" int lzx_test_eig_ops(lzx_handle h, uint32_t J, uint32_t p, const double *Q, const double *w, const double *Y, double *coef,
                                double *w_out, double *beta, double *R)
{
    static const char *fn = "lzx_test_eig_ops";
    const u32 Jtop = LZX_EIG_MAX_W + LZX_EIG_MAX_M + 1;
    if (J == 0 || J > Jtop) LZX_FAIL(LZX_ERR_ARG, "%s: J = %u columns (1 to %u)", fn, J, Jtop);
    if (p == 0 || p > J) LZX_FAIL(LZX_ERR_ARG, "%s: p = %u output columns (1 to J = %u)", fn, p, J);
    if (R && J > LZX_EIG_MAX_M) LZX_FAIL(LZX_ERR_ARG, "%s: the rotation takes at most %u columns (J = %u)", fn, LZX_EIG_MAX_M, J);
    if (!Q) LZX_FAIL(LZX_ERR_ARG, "%s: null Q", fn);
    if (!w) LZX_FAIL(LZX_ERR_ARG, "%s: null w", fn);
    if (R && !Y) LZX_FAIL(LZX_ERR_ARG, "%s: R is wanted but Y is null", fn);
    if (!h) LZX_FAIL(LZX_ERR_ARG, "%s: null handle (h)", fn);
    lzx_ctx *c = h;
    if (c->comm_kind != 0 || c->world > 1) LZX_FAIL(LZX_ERR_STATE, "%s: one GPU handle only", fn);
    if (!c->d_row_ptr || !c->d_v) LZX_FAIL(LZX_ERR_STATE, "%s: no graph has been handed over", fn);
    const u64 n = c->n;

    EigRun r;
    r.c = c;
    r.nw = 0;
    r.m = J;
    LZX_HIP(hipSetDevice(c->device));
    c->k_prep = 0;   // d_io is overwritten, as in lzx_eigsh_f64
    LZX_TRY(r.alloc(fn));
    for (u32 i = 0; i <= J; ++i) {
        LZX_HIP(hipMemcpyAsync(c->d_io, i < J ? Q + (size_t)i * n : w, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
        LZX_TRY(lzx_launch_permute_in(c, c->d_io, r.col(i), 1.0));
    }
    auto fetch = [&](u32 i, double *out) -> int {   // column i in the caller's order
        LZX_TRY(lzx_launch_permute_out(c, r.col(i), c->d_io));
        LZX_HIP(hipMemcpyAsync(out, c->d_io, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        LZX_HIP(hipStreamSynchronize(c->stream));
        return LZX_OK;
    };
    LZX_TRY(r.orth(r.col(J), J, r.H));
    LZX_TRY(r.scale(r.col(J), r.col(J), r.beta, 0.0));
    if (coef) LZX_HIP(hipMemcpyAsync(coef, r.H, sizeof(double) * J, hipMemcpyDeviceToHost, c->stream));
    if (beta) LZX_HIP(hipMemcpyAsync(beta, r.beta, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    LZX_HIP(hipStreamSynchronize(c->stream));
    if (w_out) LZX_TRY(fetch(J, w_out));
    if (R) {
        const u32 ldy = r.ldy();
        std::vector<double> Yh((size_t)J * ldy, 0.0);
        for (u32 a = 0; a < J; ++a) std::copy(Y + (size_t)a * p, Y + (size_t)(a + 1) * p, Yh.begin() + (size_t)a * ldy);
        LZX_TRY(r.rotate(0, J, Yh, ldy, p));
        for (u32 i = 0; i < p; ++i) LZX_TRY(fetch(i, R + (size_t)i * n));
    }
    return LZX_OK;
}
