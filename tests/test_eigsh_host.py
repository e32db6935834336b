"""CPU: the eigensolver (include/lzx.h: lzx_eigsh_f64) without a GPU -- its binding, the argument errors that come back
before a device is touched, and the dense symmetric solver of its restarts (test hook lzx_test_sym_eig) against
numpy.linalg.eigh."""
import ctypes

import numpy as np
import pytest

_f64p = ctypes.POINTER(ctypes.c_double)
LZX_ERR_ARG, LZX_ERR_LIMIT = -1, -6


def test_entry_point_is_bound(pkg):
    L = pkg.lib()
    assert any(name == "lzx_eigsh_f64" for name, _, _ in pkg.SYMBOLS)
    assert hasattr(L, "lzx_eigsh_f64")
    assert (pkg.EIG_LARGEST, pkg.EIG_SMALLEST) == (0, 1)
    assert ctypes.sizeof(pkg.LzxEigInfo) == 4 * 4 + 5 * 8
    assert hasattr(pkg.Engine, "eigsh")


def _call(L, h=None, nev=4, which=0, m=0, tol=1e-10, nw=0):
    ev = np.zeros(8)
    W = np.ones(16)
    return L.lzx_eigsh_f64(h, nev, which, m, tol, 10, None, 0, W.ctypes.data_as(_f64p) if nw else None, nw,
                           ev.ctypes.data_as(_f64p), None, None, None)


def test_argument_errors_without_gpu(pkg):
    L = pkg.lib()
    cases = [(dict(), LZX_ERR_ARG, "handle"),                 # null handle
             (dict(nev=0), LZX_ERR_ARG, "nev"),
             (dict(which=2), LZX_ERR_ARG, "which"),
             (dict(which=-1), LZX_ERR_ARG, "which"),
             (dict(tol=0.0), LZX_ERR_ARG, "tol"),
             (dict(tol=-1e-8), LZX_ERR_ARG, "tol"),
             (dict(tol=float("nan")), LZX_ERR_ARG, "tol"),
             (dict(m=129), LZX_ERR_LIMIT, "m = 129"),
             (dict(nw=9), LZX_ERR_LIMIT, "nw = 9")]
    for kw, code, word in cases:
        assert _call(L, **kw) == code, kw
        msg = L.lzx_last_error().decode()
        assert "lzx_eigsh_f64" in msg and word in msg, (kw, msg)


def test_eig_ops_hook_argument_errors_without_gpu(pkg):
    """test hook lzx_test_eig_ops (csrc/lzx_test_hooks.h): every argument error comes back before a device is touched"""
    L = pkg.lib()
    buf = np.zeros(137 * 4)
    P = buf.ctypes.data_as(_f64p)

    def call(J=4, p=2, Q=P, w=P, Y=P, R=P, h=None):
        return L.lzx_test_eig_ops(h, J, p, Q, w, Y, P, P, P, R)

    cases = [(dict(J=0), "J = 0"),
             (dict(J=138, p=1, R=None), "J = 138"),
             (dict(p=0), "p = 0"),
             (dict(J=4, p=5), "p = 5"),
             (dict(J=129, p=1), "at most 128"),               # the rotation stages J columns in 64 KiB of LDS
             (dict(Q=None), "null Q"),
             (dict(w=None), "null w"),
             (dict(Y=None), "Y is null"),
             (dict(), "null handle"),
             (dict(J=137, p=1, Y=None, R=None), "null handle")]   # the largest Gram-Schmidt shape: refused for the handle alone
    for kw, word in cases:
        assert call(**kw) == LZX_ERR_ARG, kw
        msg = L.lzx_last_error().decode()
        assert "lzx_test_eig_ops" in msg and word in msg, (kw, msg)


def _sym_eig(L, A):
    n = A.shape[0]
    A = np.ascontiguousarray(A, dtype=np.float64)
    w, V = np.zeros(n), np.zeros((n, n))
    assert L.lzx_test_sym_eig(n, A.ctypes.data_as(_f64p), w.ctypes.data_as(_f64p), V.ctypes.data_as(_f64p)) == 0
    return w, V


def _matrices():
    rng = np.random.default_rng(12)
    for n in (1, 2, 5, 20, 64, 128):
        M = rng.standard_normal((n, n))
        yield f"random{n}", (M + M.T) / 2
    for n in (20, 61, 128):   # arrowhead: what a thick restart leaves (diag(theta) + one coupling row) plus a tridiagonal tail
        M = np.diag(rng.standard_normal(n) * 10)
        p = n // 2
        M[p, :p] = M[:p, p] = rng.standard_normal(p) * 1e-3
        for j in range(p, n - 1):
            M[j, j + 1] = M[j + 1, j] = rng.random()
        yield f"arrowhead{n}", M
    for n in (16, 50, 128):   # graded: entries spanning twenty orders of magnitude
        d = 10.0 ** np.linspace(0, -20, n)
        M = rng.standard_normal((n, n))
        M = (M + M.T) / 2 * np.sqrt(np.outer(d, d))
        yield f"graded{n}", M
    yield "repeated", np.diag([2.0, 2.0, 1.0, 2.0, -1.0])
    yield "zero", np.zeros((4, 4))


@pytest.mark.parametrize("name,M", list(_matrices()), ids=[nm for nm, _ in _matrices()])
def test_dense_solver_matches_numpy(pkg, name, M):
    L = pkg.lib()
    w, V = _sym_eig(L, M)
    ref = np.linalg.eigvalsh(M)
    scale = max(np.abs(ref).max(), 1e-300)
    assert np.all(np.diff(w) >= 0), "eigenvalues ascending"
    assert np.abs(w - ref).max() <= 1e-13 * scale, name
    n = M.shape[0]
    assert np.abs(V.T @ V - np.eye(n)).max() <= 1e-13, name
    assert np.abs(M @ V - V * w).max() <= 1e-13 * max(scale, 1.0) * np.sqrt(n), name


def test_dense_solver_is_deterministic(pkg):
    L = pkg.lib()
    M = np.random.default_rng(3).standard_normal((40, 40))
    M = M + M.T
    a, b = _sym_eig(L, M), _sym_eig(L, M)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
