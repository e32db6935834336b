"""CPU: the batched solver (include/lzx.h: lzx_solve_multi_f64) without a GPU -- its binding and struct layout, the argument
errors that come back before a device is touched, and a numpy restatement of the batch of independent CG recurrences (per-column
freeze, per-column curvature failure, the status rules) against numpy.linalg.solve on er_n1000 under A and L.  The GPU tests use
the same restatement (batched_cg) as their reference for counts, statuses and partial iterates."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f64p = ctypes.POINTER(ctypes.c_double)
LZX_ERR_ARG, LZX_ERR_LIMIT = -1, -6


def batched_cg(M, B, shifts, tol, maxiter, W=None, sgn=1.0):
    """S(sigma_c) = sigma_c I - sgn M, one plain CG per row of B (x = 0, r = p = b_c).  Returns (X[nb, n], iters[nb], status[nb],
    bnorm[nb]) with the library's rules: W is orthonormalised in order, every b_c projected onto its complement before and every
    x_c after; column c freezes once ||r_c|| <= tol ||b_c|| (status 0, iters = the count at the freeze); a curvature <= 0 or not
    finite stops that column alone (status 2, x at the iterate before, iters = that iteration); status 1: maxiter reached."""
    B = np.array(B, dtype=np.float64, ndmin=2)
    nb, n = B.shape
    shifts = np.broadcast_to(np.asarray(shifts, dtype=np.float64), (nb,))
    Q = np.zeros((0, n))
    if W is not None:
        for w in np.atleast_2d(np.asarray(W, dtype=np.float64)):
            w = w / np.linalg.norm(w)
            for _ in range(2):
                w = w - Q.T @ (Q @ w)
            nrm = np.linalg.norm(w)
            if not nrm > 1e-10:
                raise ValueError("W is rank-deficient")
            Q = np.vstack([Q, w / nrm])

    def project(v):
        for _ in range(2):
            v = v - Q.T @ (Q @ v)
        return v

    X, iters, status, bnorm = np.zeros((nb, n)), np.full(nb, maxiter), np.ones(nb, dtype=int), np.zeros(nb)
    for c in range(nb):
        b = project(B[c])
        bnorm[c] = np.linalg.norm(b)
        if not bnorm[c] > 1e-10 * np.linalg.norm(B[c]):
            raise ValueError(f"column {c} is zero or lies in the span of W")
        x, r, p = np.zeros(n), b.copy(), b.copy()
        rr = r @ r
        for j in range(maxiter):
            w = M @ p
            curv = shifts[c] * (p @ p) - sgn * (p @ w)
            if not curv > 0 or not np.isfinite(curv):
                iters[c], status[c] = j, 2
                break
            alpha = rr / curv
            x += alpha * p
            r -= alpha * (shifts[c] * p - sgn * w)
            rr1 = r @ r
            if np.sqrt(rr1) <= tol * bnorm[c]:
                iters[c], status[c] = j + 1, 0
                break
            p = r + (rr1 / rr) * p
            rr = rr1
        X[c] = project(x)
    return X, iters, status, bnorm


def er_n1000():
    g = np.load(os.path.join(ROOT, "tests", "golden", "er_n1000.npz"))
    rp, ci = g["ref_row_offset"].astype(np.int64), g["ref_col_idx"].astype(np.int64)
    n = len(rp) - 1
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(rp)), ci] = 1.0
    return A, np.diag(np.diff(rp).astype(np.float64)) - A


def test_entry_point_is_bound(pkg):
    L = pkg.lib()
    assert any(name == "lzx_solve_multi_f64" for name, _, _ in pkg.SYMBOLS)
    assert hasattr(L, "lzx_solve_multi_f64")
    header = open(os.path.join(ROOT, "include", "lzx.h")).read()
    assert re.search(r"\bint lzx_solve_multi_f64\(", header) and "lzx_solve_multi_info" in header
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert re.search(r" T lzx_solve_multi_f64\b", out)
    assert hasattr(pkg.Engine, "solve_multi") and hasattr(pkg.Engine, "effective_resistance")


def test_info_layout_matches_the_header(pkg, tmp_path):
    fields = [f for f, _ in pkg.LzxSolveMultiInfo._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "lzx.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(lzx_solve_multi_info));']
    src += [f'printf("{f} %zu\\n", offsetof(lzx_solve_multi_info, {f}));' for f in fields]
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(pkg.LzxSolveMultiInfo) == 4 * 4 + 3 * 8 + 16 * 8
    for f in fields:
        assert int(got[f]) == getattr(pkg.LzxSolveMultiInfo, f).offset, f


def _call(L, nb=2, shifts=(2.0, 3.0), tol=1e-10, nw=0, maxiter=100, null=()):
    Bm = np.ones(8 * 20)
    sh = np.array(list(shifts) + [1.0] * 20, dtype=np.float64)
    X = np.zeros(8 * 20)
    W = np.ones(8 * 10)
    return L.lzx_solve_multi_f64(None, nb, None if "Bm" in null else Bm.ctypes.data_as(_f64p),
                                 None if "shifts" in null else sh.ctypes.data_as(_f64p), tol, maxiter,
                                 W.ctypes.data_as(_f64p) if nw and "W" not in null else None, nw, None if "X" in null else X.ctypes.data_as(_f64p),
                                 None, None, None, None)


def test_argument_errors_without_gpu(pkg):
    L = pkg.lib()
    nan, inf = float("nan"), float("inf")
    cases = [(dict(), LZX_ERR_ARG, "handle"),                    # null handle
             (dict(nb=0), LZX_ERR_ARG, "nb == 0"),
             (dict(nb=17), LZX_ERR_LIMIT, "nb = 17"),
             (dict(tol=0.0), LZX_ERR_ARG, "tol"),
             (dict(tol=-1e-8), LZX_ERR_ARG, "tol"),
             (dict(tol=nan), LZX_ERR_ARG, "tol"),
             (dict(null=("shifts",)), LZX_ERR_ARG, "null shifts"),
             (dict(shifts=(2.0, nan)), LZX_ERR_ARG, "not finite"),
             (dict(shifts=(inf, 2.0)), LZX_ERR_ARG, "not finite"),
             (dict(shifts=(2.0, -1.0)), LZX_ERR_ARG, "< 0"),
             (dict(maxiter=0), LZX_ERR_ARG, "maxiter"),
             (dict(nw=9), LZX_ERR_LIMIT, "nw = 9"),
             (dict(null=("Bm",)), LZX_ERR_ARG, "null Bm"),
             (dict(null=("X",)), LZX_ERR_ARG, "null X"),
             (dict(nw=2, null=("W",)), LZX_ERR_ARG, "W is null")]
    for kw, code, word in cases:
        assert _call(L, **kw) == code, kw
        msg = L.lzx_last_error().decode()
        assert "lzx_solve_multi_f64" in msg and word in msg, (kw, msg)


@pytest.mark.parametrize("op", ["A", "L"])
def test_restatement_matches_dense_solve(op):
    A, Lap = er_n1000()
    n = A.shape[0]
    rng = np.random.default_rng(5)
    onehot = np.zeros(n)
    onehot[np.argmax(A.sum(1))] = 1.0
    B = np.stack([np.ones(n), rng.standard_normal(n), onehot])
    tol = 1e-11
    if op == "A":
        lam = np.linalg.eigvalsh(A)
        M, sgn, shifts, W = A, 1.0, lam[-1] * np.array([1.02, 1.2, 2.0]), None
        lo, hi = shifts - lam[-1], shifts - lam[0]
    else:
        lam = np.linalg.eigvalsh(Lap)
        M, sgn, shifts, W = Lap, -1.0, np.array([0.1, 1.0, 0.0]), np.full(n, 1.0 / np.sqrt(n))
        B[0] = np.linspace(-1.0, 2.0, n)                           # (ones lies in span(W))
        lo, hi = shifts + np.where(shifts == 0.0, lam[1], 0.0), shifts + lam[-1]   # on span(W)-perp for sigma = 0
    X, iters, status, bnorm = batched_cg(M, B, shifts, tol, 2000, W=W, sgn=sgn)
    assert (status == 0).all() and (iters < 2000).all()
    for c in range(3):
        b = B[c] if W is None else B[c] - W * (W @ B[c])
        assert abs(bnorm[c] - np.linalg.norm(b)) <= 1e-12 * np.linalg.norm(b)
        S = shifts[c] * np.eye(n) - sgn * M
        ref = np.linalg.pinv(S) @ b if shifts[c] == 0.0 else np.linalg.solve(S, b)
        if W is not None:
            ref = ref - W * (W @ ref)
        assert np.linalg.norm(b - S @ X[c]) <= 10 * tol * np.linalg.norm(b), (op, c)
        assert np.linalg.norm(X[c] - ref) <= (hi[c] / lo[c]) * 10 * tol * np.linalg.norm(ref), (op, c)
    # the columns are independent: one alone, and the batch reversed, give the same bits
    X1, it1, _, _ = batched_cg(M, B[1:2], shifts[1:2], tol, 2000, W=W, sgn=sgn)
    Xr, itr, _, _ = batched_cg(M, B[::-1], shifts[::-1], tol, 2000, W=W, sgn=sgn)
    assert np.array_equal(X1[0], X[1]) and it1[0] == iters[1]
    assert np.array_equal(Xr[::-1], X) and np.array_equal(itr[::-1], iters)


def test_status_rules():
    A, _ = er_n1000()
    lam, U = np.linalg.eigh(A)
    n = A.shape[0]
    B = np.stack([np.ones(n), U[:, -1], np.ones(n)])
    shifts = np.array([1.5, 0.5, 1.02]) * lam[-1]
    X, iters, status, _ = batched_cg(A, B, shifts, 1e-10, 5)
    assert list(status) == [1, 2, 1] and list(iters) == [5, 0, 5]
    assert iters[1] == 0 and not X[1].any()            # the failing column stops at iteration 0 with x = 0
    assert status[2] == 1 and iters[2] == 5             # maxiter reached
    X0, it0, st0, _ = batched_cg(A, B[[0, 2]], shifts[[0, 2]], 1e-10, 5)
    assert np.array_equal(X0, X[[0, 2]]) and np.array_equal(it0, iters[[0, 2]])
    with pytest.raises(ValueError, match="column 1"):
        batched_cg(A, np.stack([np.ones(n), np.zeros(n)]), shifts[:2], 1e-10, 5)
    with pytest.raises(ValueError, match="rank-deficient"):
        batched_cg(A, B, shifts, 1e-10, 5, W=np.stack([np.ones(n), 2.0 * np.ones(n)]))
