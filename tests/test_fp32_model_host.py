"""CPU: the instrument behind tests/test_gpu_fp32_forms.py -- a model of the several-rank lazy loop (csrc/lzx_api.hip:
lazy_step, csrc/lzx_kernels.hip: k_lazy_update) in np.longdouble, with and without the fp32 rounding of option
`exchange_fp32` (csrc/lzx_comm.hip: lzx_comm_allgather_fp32), and the checks that make it usable as a reference:

  * it reproduces the three-term recurrence it claims to model;
  * with and without the rounding it differs, on alpha_1 and on beta_1, by at least 30 times the tolerance the GPU test
    compares them at -- so that test cannot pass against the wrong one of the two;
  * no entry of the model's u_j, 1 <= j < 6, lies within 1e-11 relative of an fp32 rounding midpoint -- so the GPU test can
    recompute f32(u_j) from fetched fp64 data (which differs from the model's by rounding-level amounts, 1e-15 .. 1e-13)
    and get the same floats in EVERY entry, with none excluded.

The inputs are those of the GPU test: path graphs of 33, 65 and 257 vertices (and the path of 9 the margins were first
measured on), x0 = 0.5 + default_rng(3).random(n), k = 6."""
import numpy as np
import pytest

LD = np.longdouble
K_EXCHANGE = 6                      # Krylov dimension of the exchange_fp32 checks
PATHS_EXCHANGE = (33, 65, 257)      # the GPU test's graphs
# First-coefficient tolerances.  alpha_0 / beta_0: the project's own (tests/test_gpu_parity.py: check_leading_coefficients),
# 1e-12 relative.  alpha_1 (relative to max(|alpha_1|, |alpha_0|), as there) and beta_1 (relative): the project's 1e-10 made
# ten times TIGHTER.  At 1e-10 the rounded and the unrounded model are only 7 tolerances apart on beta_1 of the path of 65
# (7.3e-10) and 9 on alpha_1 of the path of 257 (8.6e-10): the rounding errors of 65 / 257 entries partly cancel in these two
# sums.  At 1e-11 every input keeps the 30 tolerances asked for (73 and 86 there).  What fp64 can hold: alpha_1 = D / B with
# D, B sums of n <= 257 products, each within (n + 2) 2^-53 of its sum of magnitudes, and sum |u_i w_i| / B <= ||A|| <= 2 ~
# alpha_0: 3e-14 each, the same again for what u_1 inherits from alpha_0 and the first SpMV -- below 1e-12 in all.
TOL_FIRST = 1e-12
TOL_SECOND = 1e-11
DISCRIMINATION = 30.0               # rounded and unrounded model at least this many tolerances apart
MIDPOINT_MARGIN = 1e-11


def path_csr(n):
    """The path 0 - 1 - ... - (n-1) as the pattern-only CSR the C ABI takes."""
    rows = [[j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)]
    rp = np.zeros(n + 1, dtype=np.uint64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([j for r in rows for j in r], dtype=np.uint32)
    return rp, ci


def start_vector(n):
    return 0.5 + np.random.default_rng(3).random(n)


def matvec_ld(rp, ci, x):
    """A x with every row summed in np.longdouble (pattern-only CSR: every entry is 1)."""
    rp = np.asarray(rp).astype(np.int64)
    ci = np.asarray(ci).astype(np.int64)
    x = np.asarray(x, dtype=LD)
    y = np.zeros(len(rp) - 1, dtype=LD)
    nz = np.diff(rp) > 0
    if len(ci):
        y[nz] = np.add.reduceat(x[ci], rp[:-1][nz])
    return y


def f32(x):
    """Round to fp32 the way the device does -- from the fp64 value (k_to_f32: (float)in[i]) -- and widen again."""
    return np.asarray(x).astype(np.float64).astype(np.float32).astype(LD)


def lazy_loop_model(A, x0, k, round_exchange):
    """The several-rank lazy loop in np.longdouble, line by line as lazy_step / k_lazy_update run it.  A = (row_ptr, col_idx).

      u_0 = q_0 = x0 / ||x0||                     lanczos_prepare: k_permute_in; the first SpMV multiplies the exact q_0
      m_j = f32(u_j) in EVERY entry for j >= 1    lzx_comm_allgather_fp32 converts each rank's slice (k_to_f32) and every rank
                                                  widens ALL slices, its own too, into the buffer the SpMV reads (d_xbuf)
      w = A m_j                                   lzx_launch_spmv on d_xbuf
      D = u_j . w,  B = ||u_j||^2                 the SpMV's fused partials use the rank's own UNROUNDED u_j (SpmvLaunch's
                                                  second operand is current_u); B comes from the previous k_lazy_update's
                                                  partials over the unrounded u_j; B := 1 at j = 0
      beta_{j-1} = sqrt(B), alpha_j = D / B, q_j = u_j / beta_{j-1}
      u_{j+1} = w / beta_{j-1} - alpha_j q_j - beta_{j-1} q_{j-1}

    round_exchange = False is the fp64 exchange (m_j = u_j).  Returns (alpha[k], beta[k-1], Q (k, n), U (k, n), x_norm), all
    np.longdouble; U[j] = u_j."""
    rp, ci = A
    x0 = np.asarray(x0, dtype=LD)
    n = len(x0)
    x_norm = np.sqrt((x0 * x0).sum())
    alpha, beta = np.zeros(k, dtype=LD), np.zeros(max(k - 1, 0), dtype=LD)
    Q, U = np.zeros((k, n), dtype=LD), np.zeros((k, n), dtype=LD)
    u = x0 / x_norm
    q_prev = None
    for j in range(k):
        U[j] = u
        m = f32(u) if (round_exchange and j >= 1) else u
        w = matvec_ld(rp, ci, m)
        D = (u * w).sum()
        B = LD(1) if j == 0 else (u * u).sum()
        b = np.sqrt(B)
        alpha[j] = D / B
        if j >= 1:
            beta[j - 1] = b
        q = u / b
        Q[j] = q
        nxt = w / b - alpha[j] * q
        if q_prev is not None:
            nxt = nxt - b * q_prev
        q_prev, u = q, nxt
    return alpha, beta, Q, U, x_norm


def midpoint_margin(u):
    """Smallest relative distance of a non-zero entry of u to a point where rounding to fp32 changes its result (the midpoint
    between two neighbouring floats)."""
    u = np.asarray(u, dtype=LD)
    u = u[u != 0]
    f = u.astype(np.float32)
    lo = np.nextafter(f, np.float32(-np.inf)).astype(LD)
    hi = np.nextafter(f, np.float32(np.inf)).astype(LD)
    fl = f.astype(LD)
    d = np.minimum(np.abs(u - (fl + lo) / 2), np.abs(u - (fl + hi) / 2))
    return float((d / np.abs(u)).min())


def coefficient_distances(a, b, a_ref, b_ref):
    """(alpha_0, beta_0, alpha_1, beta_1): each distance divided by the scale its tolerance is relative to."""
    a, b, a_ref, b_ref = (np.asarray(v, dtype=LD) for v in (a, b, a_ref, b_ref))
    return (float(abs(a[0] - a_ref[0]) / abs(a_ref[0])), float(abs(b[0] - b_ref[0]) / abs(b_ref[0])),
            float(abs(a[1] - a_ref[1]) / max(abs(a_ref[1]), abs(a_ref[0]))), float(abs(b[1] - b_ref[1]) / abs(b_ref[1])))


_MODELS = {}


def models(n, k=K_EXCHANGE):
    """(unrounded, rounded) model runs on the path of n, computed once per session."""
    if (n, k) not in _MODELS:
        A = path_csr(n)
        x0 = start_vector(n)
        _MODELS[(n, k)] = tuple(lazy_loop_model(A, x0, k, r) for r in (False, True))
    return _MODELS[(n, k)]


def test_longdouble_is_extended():
    """The model is only a reference if it carries more than fp64 (x87 extended: 64-bit mantissa)."""
    assert np.finfo(LD).eps <= 2.0 ** -63


@pytest.mark.parametrize("n", (9,) + PATHS_EXCHANGE)
def test_model_is_the_three_term_recurrence(n):
    """Unrounded: A q_j = beta_{j-1} q_{j-1} + alpha_j q_j + beta_j q_{j+1}, unit columns, and against an independent
    textbook Lanczos in longdouble.  Rounded: the same with A f32(u_j) / beta_{j-1} in place of A q_j, and alpha_0 untouched
    (the first SpMV multiplies the exact q_0)."""
    A = path_csr(n)
    (a, b, Q, U, xn), (ar, br, Qr, Ur, _) = models(n)
    k = len(a)
    assert abs(xn - np.linalg.norm(start_vector(n))) <= 1e-15 * xn
    for j in range(k - 1):
        r = matvec_ld(*A, Q[j]) - a[j] * Q[j] - b[j] * Q[j + 1] - (b[j - 1] * Q[j - 1] if j else 0)
        assert np.abs(r).max() <= 1e-17, (n, j)
        m = f32(Ur[j]) if j else Ur[0]
        r = matvec_ld(*A, m) / (br[j - 1] if j else LD(1)) - ar[j] * Qr[j] - br[j] * Qr[j + 1] - (br[j - 1] * Qr[j - 1] if j else 0)
        assert np.abs(r).max() <= 1e-17, (n, j)
        assert abs(np.sqrt((Q[j] * Q[j]).sum()) - 1) <= 1e-17 and abs(np.sqrt((Qr[j] * Qr[j]).sum()) - 1) <= 1e-17
    # textbook form: v = A q_j - beta_{j-1} q_{j-1}; alpha_j = v . q_j; v -= alpha_j q_j; beta_j = ||v||
    q, qp, bp = start_vector(n).astype(LD) / xn, None, LD(0)
    for j in range(k):
        v = matvec_ld(*A, q) - (bp * qp if qp is not None else 0)
        aj = (v * q).sum()
        assert abs(aj - a[j]) <= 1e-15 * max(abs(a[0]), abs(aj)), (n, j)
        v = v - aj * q
        bp = np.sqrt((v * v).sum())
        if j < k - 1:
            assert abs(bp - b[j]) <= 1e-15 * bp, (n, j)
        qp, q = q, v / bp
    assert ar[0] == a[0] and br[0] == b[0]


@pytest.mark.parametrize("n", (9,) + PATHS_EXCHANGE)
def test_rounding_is_visible_in_the_second_coefficients(n):
    """The GPU test compares alpha_1 / beta_1 of an exchange_fp32 group with the ROUNDED model at TOL_SECOND, and those of an fp64
    group with the unrounded one.  The two models must be far enough apart for that to tell them from each other.  Measured
    (alpha_1 / beta_1): 5.8e-9 / 6.5e-9 on the path of 9, 3.8e-9 / 1.6e-8 on 33, 3.4e-9 / 7.3e-10 on 65, 8.6e-10 / 3.7e-9 on 257:
    73 tolerances of 1e-11 at the least."""
    (a, b, _, _, _), (ar, br, _, _, _) = models(n)
    d = coefficient_distances(ar, br, a, b)
    print(f"path of {n}: rounded vs unrounded model: alpha_1 {d[2]:.2e}, beta_1 {d[3]:.2e} ({d[2] / TOL_SECOND:.0f} / {d[3] / TOL_SECOND:.0f} tolerances)")
    assert d[0] == 0.0 and d[1] == 0.0
    assert d[2] >= DISCRIMINATION * TOL_SECOND and d[3] >= DISCRIMINATION * TOL_SECOND, (n, d)


@pytest.mark.parametrize("n", (9,) + PATHS_EXCHANGE)
def test_no_entry_near_an_fp32_rounding_midpoint(n):
    """f32(u_j) recomputed from a u_j that differs from the model's at rounding level (the device's fp64 sums, the fetch's
    division by beta_{j-1} and the test's multiplication back) is the same float in every entry, if no entry of the model's
    u_j is closer than MIDPOINT_MARGIN to a midpoint.  (The rounded model: only the exchange_fp32 group's u_j are rounded
    again by the GPU test.  Measured: 1.4e-9, 7.6e-11, 3.0e-11 and 1.2e-11 for the paths of 9, 33, 65 and 257.)"""
    U = models(n)[1][3]
    assert (U[1:] != 0).all()
    margins = [midpoint_margin(U[j]) for j in range(1, K_EXCHANGE)]
    print(f"path of {n}: smallest relative distance of an entry of u_1 .. u_5 to an fp32 midpoint: {min(margins):.2e}")
    assert min(margins) >= MIDPOINT_MARGIN, (n, margins)


def test_midpoint_margin_sees_a_midpoint():
    """The instrument itself: an exact midpoint has margin 0, a float has margin half an ulp."""
    f = np.float32(1.0)
    mid = (LD(f) + LD(np.nextafter(f, np.float32(2)))) / 2
    assert midpoint_margin(np.array([mid, LD(0.3)])) == 0.0
    assert abs(midpoint_margin(np.array([LD(1.0)])) - 2.0 ** -25) <= 1e-12
    assert f32(np.array([1.0 + 2.0 ** -30]))[0] == 1.0
