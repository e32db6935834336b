"""CPU: stochastic Lanczos quadrature (include/lzx.h: lzx_probes_f64, lzx_lanczos_probes_f64, lzx_probe_diag_f64) without a
GPU -- argument errors of the three entry points, and the numpy quadrature helpers behind Engine.trace_expm / diag_expm
against dense matrix exponentials."""
import ctypes

import numpy as np
import pytest
from scipy.linalg import expm

_u32p = ctypes.POINTER(ctypes.c_uint32)
_f64p = ctypes.POINTER(ctypes.c_double)
LZX_ERR_ARG = -1


def probe_np(seed, p, n):
    """Probe p of seed at vertices 0 .. n-1: the definition of include/lzx.h restated in numpy (uint64 wraps mod 2^64)."""
    i = np.arange(n, dtype=np.uint64)
    h = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * ((np.uint64(p) << np.uint64(32)) + i + np.uint64(1))
    h ^= h >> np.uint64(30)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(27)
    h *= np.uint64(0x94D049BB133111EB)
    h ^= h >> np.uint64(31)
    return np.where((h >> np.uint64(63)) == 1, -1.0, 1.0)


def numpy_lanczos(matvec, z, k):
    """k steps of Lanczos with full re-orthogonalisation (the accurate side): alpha[k], beta[k] (beta[k-1] = 0)."""
    q = z / np.linalg.norm(z)
    Qs, alpha, beta = [], np.zeros(k), np.zeros(k)
    qp, bp = np.zeros_like(q), 0.0
    for j in range(k):
        Qs.append(q)
        v = matvec(q) - bp * qp
        alpha[j] = v @ q
        v -= alpha[j] * q
        for qq in Qs:
            v -= (v @ qq) * qq
        if j + 1 < k:
            bp = np.linalg.norm(v)
            beta[j] = bp
            qp, q = q, v / bp
    return alpha, beta


def small_problem(n=12, probes=5, seed=3):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    M = (M + M.T) / 2
    Z = np.stack([probe_np(seed, p, n) for p in range(probes)])
    ab = [numpy_lanczos(lambda x: M @ x, z, n) for z in Z]
    alpha = np.stack([a for a, _ in ab])
    beta = np.stack([b for _, b in ab])
    return M, Z, alpha, beta, np.full(probes, n, dtype=np.uint32)


def test_entry_points_refuse_a_null_handle(pkg):
    L = pkg.lib()
    a, bt, x = np.zeros(64), np.zeros(64), np.zeros(64)
    ku = np.zeros(16, dtype=np.uint32)
    for b in (0, 1, 16, 17):
        calls = [("lzx_probes_f64", lambda: L.lzx_probes_f64(None, 1, 0, b, x.ctypes.data_as(_f64p))),
                 ("lzx_lanczos_probes_f64", lambda: L.lzx_lanczos_probes_f64(None, 1, 0, b, 4, 0, a.ctypes.data_as(_f64p),
                                                                             bt.ctypes.data_as(_f64p), ku.ctypes.data_as(_u32p), None)),
                 ("lzx_probe_diag_f64", lambda: L.lzx_probe_diag_f64(None, a.ctypes.data_as(_f64p), 4, x.ctypes.data_as(_f64p)))]
        for name, call in calls:
            assert call() == LZX_ERR_ARG, (name, b)
            msg = L.lzx_last_error().decode()
            assert name in msg and "handle" in msg and "(h)" in msg, (name, msg)
    assert pkg.PROBE_KEEP_BASIS == 1


def test_probe_restatement_is_a_sign_pattern():
    z = probe_np(0, 0, 1 << 16)
    assert set(np.unique(z)) == {-1.0, 1.0} and abs(z.mean()) < 0.02
    assert not np.array_equal(z, probe_np(1, 0, 1 << 16)) and not np.array_equal(z, probe_np(0, 1, 1 << 16))
    assert np.array_equal(probe_np(7, 5, 100)[:10], probe_np(7, 5, 10))   # vertex i's value does not depend on n


@pytest.mark.parametrize("s", [1.0, -0.5, 2.5])
def test_quadrature_exact_on_an_exhausted_krylov_space(pkg, s):
    M, Z, alpha, beta, ku = small_problem()
    n = M.shape[0]
    ell = pkg.slq_log_quadratures(alpha, beta, ku, n, s)
    assert ell.shape == (1, Z.shape[0])
    E = expm(s * M)
    for p, z in enumerate(Z):
        assert abs(ell[0, p] - np.log(z @ E @ z)) <= 1e-12 * max(1.0, abs(ell[0, p])), p
    # the trace and its error from the per-probe values, as defined
    lt, rel = pkg.slq_trace(ell)
    q = np.array([z @ E @ z for z in Z])
    assert abs(np.exp(lt[0]) - q.mean()) <= 1e-12 * q.mean()
    assert abs(rel[0] - q.std(ddof=1) / (np.sqrt(len(q)) * q.mean())) <= 1e-12


def test_quadrature_diag_coefficients(pkg):
    """Q_p T[p] = e^{s (M - shift)} z_p, so sum_p z_p .* (Q_p T[p]) / N is the estimate of diag e^{s (M - shift)}."""
    M, Z, alpha, beta, ku = small_problem(n=10, probes=3, seed=9)
    n = M.shape[0]
    s, shift = 0.7, 2.0
    T = pkg.slq_diag_coefficients(alpha, beta, ku, n, s, shift)
    E = expm(s * (M - shift * np.eye(n)))
    for p, z in enumerate(Z):
        # the basis of the same recurrence, rebuilt: Q^T M Q = T
        q, qp, Qs = z / np.sqrt(n), np.zeros(n), []
        for j in range(n):
            Qs.append(q)
            if j + 1 < n:
                v = M @ q - alpha[p, j] * q - (beta[p, j - 1] * qp if j else 0.0)
                for qq in Qs:
                    v -= (v @ qq) * qq
                qp, q = q, v / beta[p, j]
        y = np.array(Qs).T @ T[p]
        assert np.abs(y - E @ z).max() <= 1e-11 * np.abs(E @ z).max(), p


def test_log_trace_survives_overflow(pkg):
    M, Z, alpha, beta, ku = small_problem(n=14, probes=6, seed=5)
    n = M.shape[0]
    lam = np.linalg.eigvalsh(M)
    s = 1000.0 / lam.max()                          # e^{s lambda_max} = e^1000: overflows
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.exp(s * lam).sum())
    ell = pkg.slq_log_quadratures(alpha, beta, ku, n, s)
    lt, rel = pkg.slq_trace(ell)
    assert np.isfinite(lt).all() and np.isfinite(rel).all() and np.isfinite(ell).all()
    sigma = lam.max()
    F = expm(s * (M - sigma * np.eye(n)))           # the shifted form: every entry finite
    ell_exact = np.array([np.log(z @ F @ z) + s * sigma for z in Z])
    assert np.abs(ell[0] - ell_exact).max() <= 1e-12 * np.abs(ell_exact).max()
    m = ell_exact.max()
    lt_exact = m + np.log(np.exp(ell_exact - m).sum()) - np.log(len(Z))
    assert abs(lt[0] - lt_exact) <= 1e-12 * abs(lt_exact)


def test_grid_of_t_is_bitwise_one_at_a_time(pkg):
    M, Z, alpha, beta, ku = small_problem(n=16, probes=7, seed=11)
    ku[2] = 9                                        # one probe trimmed, as a breakdown stop leaves it
    ts = np.array([0.01, 0.3, 1.0, 4.0, 250.0])
    ell = pkg.slq_log_quadratures(alpha, beta, ku, M.shape[0], ts)
    lt, rel = pkg.slq_trace(ell)
    for i, t in enumerate(ts):
        e1 = pkg.slq_log_quadratures(alpha, beta, ku, M.shape[0], t)
        l1, r1 = pkg.slq_trace(e1)
        assert np.array_equal(e1[0], ell[i]) and l1[0] == lt[i] and r1[0] == rel[i], t
