"""CPU: PageRank by multi-shift CG in the degree inner product (include/lzx.h: lzx_pagerank_f64) without a GPU -- a numpy
restatement of the method (pagerank_wcg: the seed's CG in <a, b>_W, the zeta / alpha / beta of every other damping, the freeze
rule) against a dense direct solve and networkx.pagerank on the golden fixtures, the argument errors that come back before a
device is touched, and the layout of lzx_pagerank_info.  The GPU tests (test_gpu_pagerank.py) use pagerank_wcg, the dense
solves and the cases made here as their references: each is computed once per process."""
import ctypes
import os
import subprocess

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")
_f64p = ctypes.POINTER(ctypes.c_double)
LZX_ERR_ARG, LZX_ERR_LIMIT = -1, -6

FIXTURES = ("er_n1000", "rmat_n4096", "rmat_n3000_skew", "star_ring_n1500")
DAMPINGS = np.array([0.5, 0.85, 0.99])
TOL = 1e-12


def csr_matrix(rp, ci):
    rp64, ci64 = np.asarray(rp).astype(np.int64), np.asarray(ci).astype(np.int64)
    n = len(rp64) - 1
    return sp.csr_matrix((np.ones(len(ci64)), ci64, rp64), shape=(n, n))


def degrees(A):
    """d_i = stored entries of row i (a self loop counts once) and w_i = max(d_i, 1)."""
    d = np.diff(A.indptr).astype(np.float64)
    return d, np.maximum(d, 1.0)


def pagerank_wcg(A, v, dampings, tol, maxiter):
    """x_s = y_s / sum(y_s), (I - delta_s A W^(-1)) y_s = v / sum(v), for every damping from one Krylov sequence: CG in
    <a, b>_W on (sigma_0 I - P) z = W^(-1) v for the largest damping (sigma = 1 / delta, P = D^(-1) A with zero rows where d = 0),
    the other dampings by the multi-shift recurrences; damping s freezes once |zeta_s| ||r||_W <= tol ||b||_W.  v = None: uniform.
    Returns (X[nd, n], iters[nd], converged[nd], Y[nd, n]) in the caller's damping order, Y the unnormalised y_s."""
    dampings = np.asarray(dampings, dtype=np.float64)
    n = A.shape[0]
    d, w = degrees(A)
    v = np.full(n, 1.0 / n) if v is None else np.asarray(v, dtype=np.float64) / np.sum(v)
    uq = np.unique(dampings)[::-1]           # descending: the seed is the largest damping, the smallest sigma
    nu = len(uq)
    sigma = 1.0 / uq
    s0, delta = sigma[0], sigma - sigma[0]
    b = v / w
    tolb = tol * np.sqrt(np.sum(w * b * b))
    r, p = b.copy(), b.copy()
    Z, P = np.zeros((nu, n)), np.tile(b, (nu, 1))
    zeta, zeta_prev = np.ones(nu), np.ones(nu)
    alpha_prev, beta_prev = 1.0, 0.0
    rr = np.sum(w * r * r)
    live = np.ones(nu, dtype=bool)
    iters = np.full(nu, maxiter)
    for j in range(maxiter):
        if not live.any():
            break
        t = A @ p
        curv = s0 * np.sum(w * p * p) - p @ t
        if not curv > 0:
            raise ArithmeticError(f"not positive definite at iteration {j}")
        alpha = rr / curv
        if live[0]:
            Z[0] += alpha * p
        r = r - alpha * (s0 * p - np.where(d > 0, t / w, 0.0))
        rr1 = np.sum(w * r * r)
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
            Z[s] += alpha * q * P[s]
            if abs(zn) * rn <= tolb:
                live[s], iters[s] = False, j + 1
            else:
                P[s] = zn * r + q * q * beta * P[s]
            zeta_prev[s], zeta[s] = z, zn
        p = r + beta * p
        alpha_prev, beta_prev, rr = alpha, beta, rr1
    Y = sigma[:, None] * (w * Z)
    X = Y / Y.sum(axis=1)[:, None]
    slot = np.searchsorted(-uq, -dampings)
    return X[slot], iters[slot], ~live[slot], Y[slot]


def pagerank_dense(A, V, delta):
    """Columns x = y / sum(y) with (I - delta A W^(-1)) y = v / sum(v) for every column v of V, by LU."""
    n = A.shape[0]
    _, w = degrees(A)
    Y = np.linalg.solve(np.eye(n) - delta * (A.toarray() / w[None, :]), V / V.sum(axis=0)[None, :])
    return Y / Y.sum(axis=0)[None, :]


def l1_residual(A, v, delta, y):
    """||v - (I - delta A W^(-1)) y||_1 / ||v||_1 with v scaled to sum 1."""
    _, w = degrees(A)
    v = v / v.sum()
    return float(np.abs(v - y + delta * (A @ (y / w))).sum() / np.abs(v).sum())


def error_bound(A, v, delta, tol):
    """What the stop rule guarantees in exact arithmetic.  The residual of damping s in v-space is W (zeta_s r), so
    ||res||_1 = sum w |zeta r| <= sqrt(sum w) |zeta| ||r||_W <= sqrt(sum w) tol ||b||_W (Cauchy-Schwarz).  A W^(-1) has column
    sums <= 1, so ||(I - delta A W^(-1))^(-1)||_1 <= 1 / (1 - delta) and ||y - y*||_1 <= ||res||_1 / (1 - delta); sum(y*) >= 1
    (sum the equation), so the normalised vectors differ by at most twice that."""
    _, w = degrees(A)
    v = v / v.sum()
    return 2.0 * tol * np.sqrt(w.sum() * np.sum(v * v / w)) / (1.0 - delta)


def teleports(A):
    """(name, v) for the three teleport vectors of the fixture tests: uniform (None to the library), seeded random positive,
    one-hot on the highest-degree vertex (the first such)."""
    n = A.shape[0]
    d, _ = degrees(A)
    hot = np.zeros(n)
    hot[int(np.argmax(d))] = 1.0
    return [("uniform", np.full(n, 1.0 / n)), ("random", np.random.default_rng(17).random(n) + 1e-3), ("onehot", hot)]


class Case:
    """One graph with its references, each made on first use and kept for the process."""

    def __init__(self, name, rp, ci, vs=None):
        self.name, self.rp, self.ci = name, np.asarray(rp).astype(np.uint64), np.asarray(ci).astype(np.uint32)
        self.A = csr_matrix(rp, ci)
        self.n = self.A.shape[0]
        self.d, self.w = degrees(self.A)
        self._c = {} if vs is None else {"vs": list(vs)}      # vs: (name, v) teleport vectors instead of teleports(A)

    def once(self, key, make):
        if key not in self._c:
            self._c[key] = make()
        return self._c[key]

    def vs(self):
        return self.once("vs", lambda: teleports(self.A))

    def dense(self, delta):
        """{teleport name: x} by LU, the three teleport vectors in one solve."""
        def make():
            names = [nm for nm, _ in self.vs()]
            X = pagerank_dense(self.A, np.stack([v for _, v in self.vs()], axis=1), delta)
            return {nm: X[:, i].copy() for i, nm in enumerate(names)}
        return self.once(("dense", float(delta)), make)

    def model(self, vname, dampings=DAMPINGS, tol=TOL, maxiter=1000):
        v = dict(self.vs())[vname]
        return self.once(("model", vname, tuple(dampings), tol, maxiter), lambda: pagerank_wcg(self.A, v, dampings, tol, maxiter))


_CASES = {}


def fixture_case(name):
    if name not in _CASES:
        g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        _CASES[name] = Case(name, g["ref_row_offset"], g["ref_col_idx"])
    return _CASES[name]


def nx_pagerank(A, v, alpha):
    G = nx.from_scipy_sparse_array(A)
    pers = None if v is None else {i: float(v[i]) for i in range(A.shape[0])}
    pr = nx.pagerank(G, alpha=alpha, personalization=pers, tol=1e-13, max_iter=1000)
    return np.array([pr[i] for i in range(A.shape[0])])


# ---- the numpy model ----
@pytest.mark.parametrize("name", FIXTURES)
def test_model_matches_dense_solve(name):
    """Within what the stop rule guarantees (error_bound) plus 1e-13 of rounding: ||x - x*||_1 for every damping and teleport
    vector; the model's own L1 residual within the bound's residual part; iterations non-decreasing in delta."""
    c = fixture_case(name)
    for vname, v in c.vs():
        X, iters, conv, Y = c.model(vname)
        assert conv.all() and iters.max() <= 60, (name, vname, iters)
        assert np.all(np.diff(iters) >= 0), (name, vname, iters)
        for s, delta in enumerate(DAMPINGS):
            err = np.abs(X[s] - c.dense(delta)[vname]).sum()
            bound = error_bound(c.A, v, delta, TOL)
            print(name, vname, delta, f"iters {iters[s]} L1 error {err:.2e} bound {bound:.2e}")
            assert err <= bound + 1e-13, (name, vname, delta, err, bound)
            assert l1_residual(c.A, v, delta, Y[s]) <= bound * (1.0 - delta) / 2.0 + 1e-13, (name, vname, delta)
            assert abs(X[s].sum() - 1.0) <= 1e-13 and X[s].min() >= -TOL
            if vname != "uniform":
                assert np.all(X[s][(c.d == 0) & (v == 0)] == 0.0)


@pytest.mark.parametrize("name", ["er_n1000", "rmat_n4096"])
def test_model_matches_networkx(name):
    """networkx stops at an L1 change of n * 1e-13 between power iterations; 1e-8 is its stopping error, not the model's."""
    c = fixture_case(name)
    for vname in ("uniform", "random"):
        v = dict(c.vs())[vname]
        X, _, conv, _ = pagerank_wcg(c.A, v, [0.85], TOL, 1000)
        err = np.abs(X[0] - nx_pagerank(c.A, None if vname == "uniform" else v, 0.85)).sum()
        print(name, vname, f"L1 distance to networkx {err:.2e}")
        assert conv.all() and err <= 1e-8, (name, vname, err)


def test_model_orders_duplicates_and_single_dampings():
    c = fixture_case("er_n1000")
    v = dict(c.vs())["random"]
    X, iters, _, _ = pagerank_wcg(c.A, v, DAMPINGS, TOL, 1000)
    Xp, itp, _, _ = pagerank_wcg(c.A, v, DAMPINGS[[2, 0, 1, 2]], TOL, 1000)
    for i, s in enumerate([2, 0, 1, 2]):
        assert np.array_equal(Xp[i], X[s]) and itp[i] == iters[s]
    for s, delta in enumerate(DAMPINGS):
        x1, _, _, _ = pagerank_wcg(c.A, v, [delta], TOL, 1000)
        assert np.abs(x1[0] - X[s]).max() <= 10 * TOL


def test_model_edgeless_and_isolated_teleport():
    A = sp.csr_matrix((5, 5))
    v = np.array([1.0, 2.0, 0.0, 3.0, 4.0])
    X, iters, conv, _ = pagerank_wcg(A, v, [0.85, 0.5], TOL, 10)
    assert conv.all() and list(iters) == [1, 1] and np.abs(X - v / 10.0).max() <= 1e-15
    A = csr_matrix([0, 1, 2, 2], [1, 0])     # one edge and an isolated vertex that carries all of v
    X, iters, conv, _ = pagerank_wcg(A, np.array([0.0, 0.0, 1.0]), [0.85], TOL, 10)
    assert conv.all() and np.array_equal(X[0], [0.0, 0.0, 1.0])


# ---- the library without a GPU ----
def test_entry_point_is_bound(pkg):
    L = pkg.lib()
    assert any(name == "lzx_pagerank_f64" for name, _, _ in pkg.SYMBOLS)
    assert hasattr(L, "lzx_pagerank_f64") and hasattr(pkg.Engine, "pagerank")


def _call(L, nd=2, damping=(0.85, 0.5), tol=1e-10, maxiter=100, v=None, null_damping=False, null_X=False):
    dm = np.array(list(damping) + [0.5] * 20, dtype=np.float64)
    X = np.zeros(8 * 20)
    return L.lzx_pagerank_f64(None, None if v is None else np.asarray(v, dtype=np.float64).ctypes.data_as(_f64p), nd,
                              None if null_damping else dm.ctypes.data_as(_f64p), tol, maxiter, None if null_X else X.ctypes.data_as(_f64p),
                              None, None, None)


def test_argument_errors_without_gpu(pkg):
    L = pkg.lib()
    nan, inf = float("nan"), float("inf")
    cases = [(dict(), LZX_ERR_ARG, "handle"),                    # null handle
             (dict(nd=0), LZX_ERR_ARG, "nd == 0"),
             (dict(nd=17), LZX_ERR_LIMIT, "nd = 17"),
             (dict(tol=0.0), LZX_ERR_ARG, "tol"),
             (dict(tol=-1e-8), LZX_ERR_ARG, "tol"),
             (dict(tol=nan), LZX_ERR_ARG, "tol"),
             (dict(null_damping=True), LZX_ERR_ARG, "null damping"),
             (dict(damping=(0.85, 1.0)), LZX_ERR_ARG, "not in (0, 1)"),
             (dict(damping=(0.0, 0.5)), LZX_ERR_ARG, "not in (0, 1)"),
             (dict(damping=(0.85, -0.5)), LZX_ERR_ARG, "not in (0, 1)"),
             (dict(damping=(0.85, nan)), LZX_ERR_ARG, "not in (0, 1)"),
             (dict(damping=(inf, 0.5)), LZX_ERR_ARG, "not in (0, 1)"),
             (dict(maxiter=0), LZX_ERR_ARG, "maxiter")]
    for kw, code, word in cases:
        assert _call(L, **kw) == code, kw
        msg = L.lzx_last_error().decode()
        assert "lzx_pagerank_f64" in msg and word in msg, (kw, msg)


def test_info_layout_matches_the_header(pkg, tmp_path):
    fields = [f for f, _ in pkg.LzxPagerankInfo._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "lzx.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(lzx_pagerank_info));']
    src += [f'printf("{f} %zu\\n", offsetof(lzx_pagerank_info, {f}));' for f in fields]
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(pkg.LzxPagerankInfo) == 4 * 4 + 3 * 8 + 16 * 8
    assert fields == ["iterations", "launched", "converged", "nd", "loop_ms", "spmv_ms", "vec_ms", "mass"]
    for f in fields:
        assert int(got[f]) == getattr(pkg.LzxPagerankInfo, f).offset, f
