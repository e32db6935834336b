"""CPU: the shifted solver (include/lzx.h: lzx_solve_shifted_f64) without a GPU -- its binding and struct layout, the argument
errors that come back before a device is touched, and a numpy restatement of the multi-shift CG recurrences (the seed's plain
CG, the zeta / alpha / beta of every other shift, the freeze rule) against numpy.linalg.solve.  The GPU tests use the same
restatement (multishift_cg) as their reference for counts and stop rules."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f64p = ctypes.POINTER(ctypes.c_double)
LZX_ERR_ARG, LZX_ERR_LIMIT = -1, -6


def multishift_cg(M, b, shifts, tol, maxiter, sgn=1.0):
    """S(sigma) = sigma I - sgn M.  Returns (X[ns, n], iters[ns], converged[ns]) with the library's rules: the seed is the
    smallest shift; shift s freezes once |zeta_s| ||r|| <= tol ||b|| (x_s and p_s no longer change), the seed's r and p run on
    until every shift is frozen or maxiter iterations have run."""
    shifts = np.asarray(shifts, dtype=np.float64)
    uq = np.unique(shifts)
    nu, n = len(uq), len(b)
    s0, delta = uq[0], uq - uq[0]
    tolb = tol * np.linalg.norm(b)
    r, p = b.copy(), b.copy()
    X, P = np.zeros((nu, n)), np.tile(b, (nu, 1))
    zeta, zeta_prev = np.ones(nu), np.ones(nu)
    alpha_prev, beta_prev = 1.0, 0.0
    rr = r @ r
    live = np.ones(nu, dtype=bool)
    iters = np.full(nu, maxiter)
    for j in range(maxiter):
        if not live.any():
            break
        w = M @ p
        curv = s0 * (p @ p) - sgn * (p @ w)
        if not curv > 0:
            raise ArithmeticError(f"not positive definite at iteration {j}")
        alpha = rr / curv
        if live[0]:
            X[0] += alpha * p
        r = r - alpha * (s0 * p - sgn * w)
        rr1 = r @ r
        beta = rr1 / rr
        rn = np.sqrt(rr1)
        was = live.copy()
        if live[0] and rn <= tolb:
            live[0], iters[0] = False, j + 1
        for s in range(1, nu):
            if not was[s]:
                continue
            z, zp = zeta[s], zeta_prev[s]
            zn = z * zp * alpha_prev / (alpha * beta_prev * (zp - z) + zp * alpha_prev * (1.0 + delta[s] * alpha))
            q = zn / z
            X[s] += alpha * q * P[s]
            if abs(zn) * rn <= tolb:
                live[s], iters[s] = False, j + 1
            else:
                P[s] = zn * r + q * q * beta * P[s]
            zeta_prev[s], zeta[s] = z, zn
        p = r + beta * p
        alpha_prev, beta_prev, rr = alpha, beta, rr1
    slot = np.searchsorted(uq, shifts)
    return X[slot], iters[slot], ~live[slot]


def test_entry_point_is_bound(pkg):
    L = pkg.lib()
    assert any(name == "lzx_solve_shifted_f64" for name, _, _ in pkg.SYMBOLS)
    assert hasattr(L, "lzx_solve_shifted_f64")
    assert "solve_state_bytes" in pkg.SHAPE_OPTIONS and "solve_poll" in pkg.SHAPE_OPTIONS
    assert hasattr(pkg.Engine, "solve_shifted") and hasattr(pkg.Engine, "katz")


def test_info_layout_matches_the_header(pkg, tmp_path):
    fields = [f for f, _ in pkg.LzxSolveInfo._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "lzx.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(lzx_solve_info));']
    src += [f'printf("{f} %zu\\n", offsetof(lzx_solve_info, {f}));' for f in fields]
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(pkg.LzxSolveInfo) == 4 * 4 + 4 * 8
    for f in fields:
        assert int(got[f]) == getattr(pkg.LzxSolveInfo, f).offset, f


def _call(L, ns=2, shifts=(2.0, 3.0), tol=1e-10, nw=0, maxiter=100):
    b = np.ones(8)
    sh = np.array(list(shifts) + [1.0] * 20, dtype=np.float64)
    X = np.zeros(8 * 20)
    W = np.ones(8 * 10)
    return L.lzx_solve_shifted_f64(None, b.ctypes.data_as(_f64p), ns, sh.ctypes.data_as(_f64p), tol, maxiter,
                                   W.ctypes.data_as(_f64p) if nw else None, nw, X.ctypes.data_as(_f64p), None, None, None)


def test_argument_errors_without_gpu(pkg):
    L = pkg.lib()
    nan, inf = float("nan"), float("inf")
    cases = [(dict(), LZX_ERR_ARG, "handle"),                    # null handle
             (dict(ns=0), LZX_ERR_ARG, "ns == 0"),
             (dict(ns=17), LZX_ERR_LIMIT, "ns = 17"),
             (dict(tol=0.0), LZX_ERR_ARG, "tol"),
             (dict(tol=-1e-8), LZX_ERR_ARG, "tol"),
             (dict(tol=nan), LZX_ERR_ARG, "tol"),
             (dict(shifts=(2.0, nan)), LZX_ERR_ARG, "not finite"),
             (dict(shifts=(inf, 2.0)), LZX_ERR_ARG, "not finite"),
             (dict(shifts=(2.0, -1.0)), LZX_ERR_ARG, "< 0"),
             (dict(maxiter=0), LZX_ERR_ARG, "maxiter"),
             (dict(nw=9), LZX_ERR_LIMIT, "nw = 9")]
    for kw, code, word in cases:
        assert _call(L, **kw) == code, kw
        msg = L.lzx_last_error().decode()
        assert "lzx_solve_shifted_f64" in msg and word in msg, (kw, msg)


def _spd_cases():
    rng = np.random.default_rng(5)
    for n in (5, 30, 120):
        G = rng.standard_normal((n, n))
        A = (G + G.T) / 2
        lam = np.linalg.eigvalsh(A)[-1]
        yield f"adjacency{n}", A, 1.0, lam * np.array([1.02, 1.2, 2.0, 1.2, 5.0])
    for n in (40, 100):   # a Laplacian of a random graph, sigma I + L
        E = np.triu(rng.random((n, n)) < 0.1, 1)
        E = (E | E.T).astype(np.float64)
        Lap = np.diag(E.sum(1)) - E
        yield f"laplacian{n}", Lap, -1.0, np.array([0.1, 1.0, 10.0, 1e-3])


@pytest.mark.parametrize("name,M,sgn,shifts", list(_spd_cases()), ids=[c[0] for c in _spd_cases()])
def test_recurrences_match_dense_solve(name, M, sgn, shifts):
    n = M.shape[0]
    b = np.random.default_rng(len(name)).standard_normal(n)
    tol = 1e-12
    X, iters, conv = multishift_cg(M, b, shifts, tol, 10 * n, sgn)
    assert conv.all(), (name, iters)
    for s, sig in enumerate(shifts):
        S = sig * np.eye(n) - sgn * M
        ref = np.linalg.solve(S, b)
        kappa = np.linalg.cond(S)
        assert np.linalg.norm(b - S @ X[s]) <= 10 * tol * np.linalg.norm(b) * max(1.0, kappa / 10), (name, sig)
        assert np.linalg.norm(X[s] - ref) <= kappa * 10 * tol * np.linalg.norm(ref), (name, sig)
    # a shift's vector does not depend on the others, nor on their order; a duplicate gets the same vector
    X1, it1, _ = multishift_cg(M, b, shifts[1:2], tol, 10 * n, sgn)
    Xp, _, _ = multishift_cg(M, b, shifts[::-1], tol, 10 * n, sgn)
    assert np.array_equal(Xp[::-1], X)
    if shifts[1] == shifts.min():
        assert np.array_equal(X1[0], X[1])


def test_seed_alone_has_the_same_bits():
    rng = np.random.default_rng(9)
    G = rng.standard_normal((50, 50))
    A = (G + G.T) / 2
    lam = np.linalg.eigvalsh(A)[-1]
    b = rng.standard_normal(50)
    Xa, ia, _ = multishift_cg(A, b, [1.1 * lam, 3.0 * lam, 1.5 * lam], 1e-10, 500)
    Xs, is_, _ = multishift_cg(A, b, [1.1 * lam], 1e-10, 500)
    assert np.array_equal(Xa[0], Xs[0]) and ia[0] == is_[0]
    assert ia[1] < ia[2] < ia[0]   # the better conditioned a system, the earlier it freezes


def test_not_positive_definite_is_detected():
    A = np.diag([3.0, 1.0, 0.5])
    with pytest.raises(ArithmeticError, match="iteration 0"):
        multishift_cg(A, np.array([1.0, 0.0, 0.0]), [1.5], 1e-10, 10)
