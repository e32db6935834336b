"""GPU: the entry points that sit on lzx_launch_spmv -- lzx_spmv_f64, the Lanczos loop under L, lzx_eigsh_f64 and
lzx_solve_shifted_f64 -- through EVERY blocked form of test_gpu_parity.MODES, under both operators.  They consume the launch's
side products (the fused v . q block partials counted by lzx_spmv_partials, a v that is complete after the launch, zero rows
and padding up to n_loc_pad), which the single-vector adjacency loop of test_gpu_parity does not pin for them.

A (mode, graph) pair is run only where the blocked passes really engage (info()["pb_entries"] > 0): propagation_blocking=1
needs hub_entries < n (lzx_graph_prepare: hub = min(hub_entries or 16384, n, 20000) & ~1, blocking off when hub >= n), so a
mode without hub_entries engages on er_200k, rmat_hub and the odd-n graph only.  Every test ends by asserting that every
entry of MODES[1:] engaged on at least two graphs.

Host references are made once per graph (module cache): scipy / numpy in float64 for the matrices and spectra, np.longdouble
for the first Lanczos coefficients and for the check of the three-iteration CG restatement."""
import os
import time

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csg
from scipy.sparse.linalg import eigsh, spsolve

from test_gpu_parity import MODES
from test_solve_host import multishift_cg

pytestmark = pytest.mark.gpu

LAP = 1
GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")
BIG = 10000          # above: scipy references, residual-based bounds, the C2 tests' 1e-11 on reported residuals
EIG_M = 40           # basis columns of every eigsh call (star_ring's clustered pairs need more than the default 20)
ODD = "er_odd_2001"  # odd n <= 16384: default staging leaves exactly one column unstaged and blocking stays on

_T0 = time.time()


def _fixture(name):
    g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return g["ref_row_offset"].astype(np.uint64), g["ref_col_idx"]


GRAPHS = {
    "er_200k": lambda O: O.gen_er(200000, 1000000, 21),
    "rmat_hub": lambda O: O.gen_rmat(16, 65536, 1500000, 99, a=0.7, b=0.12, c=0.12),
    "rmat_s14": lambda O: O.gen_rmat(14, 12000, 200000, 7),
    "er_tiny": lambda O: O.gen_er(130, 300, 3),
    "rmat_n4096": lambda O: _fixture("rmat_n4096"),              # 1204 components, rows without an edge
    "star_ring_n1500": lambda O: _fixture("star_ring_n1500"),    # repeated eigenvalues
    ODD: lambda O: O.gen_er(2001, 14000, 5),
}


def staged_columns(mode, n):
    """lzx_graph_prepare's rule restated: how many columns the mode stages on a graph of n vertices (0: blocking is off)."""
    if not mode.get("propagation_blocking"):
        return 0
    hub = min(mode.get("hub_entries", 16384), n, 20000) & ~1
    return hub if 0 < hub < n else 0


def will_engage(mode, n, n_active):
    """Blocked entries exist iff blocking is on and some referenced column is not staged (test_spmv_matches_oracle's rule)."""
    hub = staged_columns(mode, n)
    return hub > 0 and n_active > hub


class Graph:
    """One graph with its host references, each computed on first use."""

    def __init__(self, name, rp, ci):
        self.name, self.rp, self.ci = name, rp, ci
        self.rp64, self.ci64 = rp.astype(np.int64), ci.astype(np.int64)
        self.n = len(rp) - 1
        self.A = sp.csr_matrix((np.ones(len(self.ci64)), self.ci64, self.rp64), shape=(self.n, self.n))
        self.d = np.diff(self.rp64).astype(np.float64)
        self.L = (sp.diags(self.d) - self.A).tocsr()
        self.n_active = int((self.d > 0).sum())
        self.connected = csg.connected_components(self.A, directed=False)[0] == 1
        self.big = self.n > BIG
        self._c = {}

    def M(self, op):
        return self.L if op else self.A

    def once(self, key, make):
        if key not in self._c:
            self._c[key] = make()
        return self._c[key]

    # ---- extended precision ----
    def matvec_ld(self, op, x):
        """M x with every row summed in np.longdouble."""
        x = np.asarray(x, dtype=np.longdouble)
        y = np.zeros(self.n, dtype=np.longdouble)
        nz = self.d > 0
        if len(self.ci64):
            y[nz] = np.add.reduceat(x[self.ci64], self.rp64[:-1][nz])
        return self.d.astype(np.longdouble) * x - y if op else y

    # ---- spectra ----
    def dense(self, op):
        assert self.n <= 4096
        return self.once(("dense", op), lambda: np.linalg.eigh(self.M(op).toarray()))

    def extreme(self, op, nev, smallest=False):
        """(w ascending, V or None): the nev wanted-most DISTINCT eigenvalues (a single start vector finds one vector of a
        repeated eigenvalue: lzx.h), with vectors only where all of them are simple.  smallest: under L with the constant
        vector deflated, i.e. without the one zero eigenvalue of a connected graph."""
        def make():
            if self.n <= 4096:
                lam, U = self.dense(op)
                order = range(1, self.n) if smallest else range(self.n - 1, -1, -1)
                tol = 1e-9 * abs(lam).max()
                keep, simple = [], []
                for i in order:
                    if keep and abs(lam[keep[-1]] - lam[i]) <= tol:
                        simple[-1] = False
                        continue
                    if len(keep) == nev:
                        break
                    keep.append(i)
                    simple.append(True)
                keep = sorted(keep)
                return lam[keep], (U[:, keep] if all(simple) else None)
            assert not smallest
            w, V = eigsh(self.M(op), k=nev, which="LA", tol=1e-13)
            o = np.argsort(w)
            return w[o], V[:, o]
        return self.once(("extreme", op, nev, smallest), make)

    def lam_max(self, op):
        return float(self.extreme(op, 2 if op else 4)[0][-1])

    # ---- Laplacian Lanczos: the start of the recurrence in extended precision ----
    def lanczos_start(self, x0, xn):
        """(alpha_0, beta_0, alpha_1) of L from q_0 = x0 / xn (the engine's own division), every sum in np.longdouble."""
        ld = np.longdouble
        q0 = (x0 / xn).astype(ld)
        w = self.matvec_ld(LAP, q0)
        a0 = np.sum(w * q0)
        r = w - a0 * q0
        b0 = np.sqrt(np.sum(r * r))
        q1 = r / b0
        a1 = np.sum(self.matvec_ld(LAP, q1) * q1)
        return float(a0), float(b0), float(a1)

    # ---- shifted systems ----
    def shifts(self, op):
        return 1.0 / np.array([0.1, 1.0, 10.0]) if op else np.array([1.02, 1.2, 2.0]) * self.lam_max(0)

    def rhs(self, op):
        """(name, b) pairs: under L the constant vector is a null vector (one-step convergence), so only the random one."""
        rnd = ("random", np.random.default_rng(7).standard_normal(self.n))
        return [rnd] if op else [("ones", np.ones(self.n)), rnd]

    def cg3(self, op, bname):
        """(X, iters, converged) after at most three iterations by test_solve_host.multishift_cg, checked here against the
        same iterations in np.longdouble: where the two agree to 1e-13 the float64 restatement is a valid reference at 1e-12,
        where they do not the np.longdouble run is the reference.  (They agree on every graph here but star_ring under A from
        b = ones, 1.4e-13: the Krylov space of b closes after two steps there, the restatement freezes every shift at
        iteration 2 -- and so must the library -- and x is the solution itself to kappa * eps.)"""
        def make():
            b = dict(self.rhs(op))[bname]
            sgn = -1.0 if op else 1.0
            X, iters, conv = multishift_cg(self.M(op), b, self.shifts(op), 1e-10, 3, sgn)
            Xl = multishift_cg_ld(lambda p: self.matvec_ld(op, p), b, self.shifts(op), 1e-10, 3, sgn)
            err = float(np.abs(X - Xl).max() / np.abs(Xl).max())
            assert err <= 1e-13 or conv.all(), (self.name, op, bname, err)
            return (X if err <= 1e-13 else Xl), iters, conv
        return self.once(("cg3", op, bname), make)

    def residual(self, op, sig, x, b):
        """||b - S(sigma) x|| / ||b||: with scipy in float64 on the large graphs; in np.longdouble on the small ones, where a
        residual can sit at the rounding level of its own float64 evaluation (star_ring under A from b = ones: the Krylov space
        closes, the float64 figure is 1.2e-12 of pure rounding) and the 1e-12 on the reported residual needs a host value
        that is better than that."""
        if self.big:
            Sx = sig * x + self.L @ x if op else sig * x - self.A @ x
            return float(np.linalg.norm(b - Sx) / np.linalg.norm(b))
        ld = np.longdouble
        Mx = self.matvec_ld(op, x)
        r = b.astype(ld) - (ld(sig) * x.astype(ld) + Mx if op else ld(sig) * x.astype(ld) - Mx)
        return float(np.sqrt(np.sum(r * r)) / np.sqrt(np.sum(b.astype(ld) ** 2)))

    def direct(self, op, bname):
        """spsolve references and condition numbers, one per shift (n <= 10000 only; every right-hand side in one call)."""
        def make():
            names = [nm for nm, _ in self.rhs(op)]
            B = np.stack([b for _, b in self.rhs(op)], axis=1)
            lam = self.dense(op)[0]
            out = []
            for sig in self.shifts(op):
                S = (sig * sp.identity(self.n) + self.L if op else sig * sp.identity(self.n) - self.A).tocsc()
                kappa = (sig + lam[-1]) / sig if op else (sig - lam[0]) / (sig - lam[-1])
                out.append((np.asarray(spsolve(S, B)).reshape(self.n, len(names)), kappa))
            return out
        ref = self.once(("direct", op), make)
        col = [nm for nm, _ in self.rhs(op)].index(bname)
        return [(X[:, col], kappa) for X, kappa in ref]


def multishift_cg_ld(matvec, b, shifts, tol, maxiter, sgn):
    """test_solve_host.multishift_cg line by line (recurrences and freeze rule) with every operation in np.longdouble."""
    ld = np.longdouble
    shifts = np.asarray(shifts, dtype=np.float64)
    uq = np.unique(shifts)
    nu, n = len(uq), len(b)
    s0, delta, sgn = ld(uq[0]), (uq - uq[0]).astype(ld), ld(sgn)
    b = np.asarray(b, dtype=ld)
    tolb = ld(tol) * np.sqrt(np.sum(b * b))
    r, p = b.copy(), b.copy()
    X, P = np.zeros((nu, n), dtype=ld), np.tile(b, (nu, 1))
    zeta, zeta_prev = np.ones(nu, dtype=ld), np.ones(nu, dtype=ld)
    alpha_prev, beta_prev = ld(1.0), ld(0.0)
    rr = np.sum(r * r)
    live = np.ones(nu, dtype=bool)
    for _ in range(maxiter):
        if not live.any():
            break
        w = matvec(p)
        alpha = rr / (s0 * np.sum(p * p) - sgn * np.sum(p * w))
        if live[0]:
            X[0] += alpha * p
        r = r - alpha * (s0 * p - sgn * w)
        rr1 = np.sum(r * r)
        beta = rr1 / rr
        rn = np.sqrt(rr1)
        was = live.copy()
        if live[0] and rn <= tolb:
            live[0] = False
        for s in range(1, nu):
            if not was[s]:
                continue
            z, zp = zeta[s], zeta_prev[s]
            zn = z * zp * alpha_prev / (alpha * beta_prev * (zp - z) + zp * alpha_prev * (1 + delta[s] * alpha))
            q = zn / z
            X[s] += alpha * q * P[s]
            if abs(zn) * rn <= tolb:
                live[s] = False
            else:
                P[s] = zn * r + q * q * beta * P[s]
            zeta_prev[s], zeta[s] = z, zn
        p = r + beta * p
        alpha_prev, beta_prev, rr = alpha, beta, rr1
    return X[np.searchsorted(uq, shifts)].astype(np.float64)


_GRAPHS = {}


def graph(O, name):
    if name not in _GRAPHS:
        rp, ci = GRAPHS[name](O)
        _GRAPHS[name] = Graph(name, rp, ci)
    return _GRAPHS[name]


def run_pairs(pkg, O, what, body):
    """body(mode index, mode, graph, engine) for every pair of MODES[1:] x graphs whose blocked passes engage (what info()
    reports is asserted against the rule above).  A failed assertion of one pair does not hide the others: all of them are
    reported at the end, where every blocked mode must also have run on at least two graphs -- the modes with default staging
    on the two large graphs and on the odd-n graph -- so that this module cannot quietly become a plain-path test."""
    engaged, failed = {}, []
    for name in GRAPHS:
        g = graph(O, name)
        for i, mode in enumerate(MODES[1:], 1):
            if not will_engage(mode, g.n, g.n_active):
                continue
            eng = pkg.Engine(0, **mode)
            try:
                eng.set_graph_csr(g.rp, g.ci)
                gi = eng.info()
                assert gi["pb_entries"] > 0 and gi["hub_entries"] == staged_columns(mode, g.n), (name, mode, gi)
                engaged.setdefault(i, []).append(name)
                body(i, mode, g, eng)
            except AssertionError as e:
                failed.append(f"MODES[{i}] on {name}: {str(e)[:600]}")
            finally:
                eng.close()
    print(f"{what}: " + "; ".join(f"MODES[{i}]: {', '.join(v)}" for i, v in sorted(engaged.items())) + f" [{time.time() - _T0:.0f} s]")
    assert not failed, f"{what}: {len(failed)} (mode, graph) pairs failed:\n" + "\n".join(failed)
    for i, mode in enumerate(MODES[1:], 1):
        names = engaged.get(i, [])
        assert len(names) >= 2, (what, mode, names)
        if "hub_entries" not in mode:
            assert {"er_200k", "rmat_hub", ODD} <= set(names), (what, mode, names)
    return engaged


def test_engagement_rule_and_the_odd_n_case(pkg, oracle):
    """What info() reports for EVERY (mode, graph) pair against the rule restated in will_engage; propagation_blocking=1
    alone engages on er_200k and rmat_hub and not on the small even graphs; the odd-n graph with default staging stages
    n - 1 = 2000 columns and blocks the entries of the one column left."""
    for name in GRAPHS:
        g = graph(oracle, name)
        for mode in MODES:
            eng = pkg.Engine(0, **mode)
            try:
                eng.set_graph_csr(g.rp, g.ci)
                gi = eng.info()
            finally:
                eng.close()
            assert (gi["pb_entries"] > 0) == will_engage(mode, g.n, g.n_active), (name, mode, gi)
            assert (gi["pb_entries"] > 0) == (g.n_active > gi["hub_entries"]) or not mode["propagation_blocking"], (name, mode, gi)
            if mode == dict(propagation_blocking=1):
                assert (gi["pb_entries"] > 0) == (name in ("er_200k", "rmat_hub", ODD)), (name, gi)
            if name == ODD and "hub_entries" not in mode and mode["propagation_blocking"]:
                assert g.n % 2 == 1 and gi["hub_entries"] == g.n - 1 and g.n_active == g.n, gi
                assert 0 < gi["pb_entries"] <= int(g.d.max()), gi     # the entries of ONE column


def test_exact_spmv(pkg, oracle):
    """Integer-valued x in [-50, 50]: every row sum is an integer far below 2^53, exact in any order, so A x and L x must
    EQUAL the host's in every blocked form; and A x again after the switch back."""
    def body(i, mode, g, eng):
        x = g.once("x_int", lambda: np.random.default_rng(3).integers(-50, 51, g.n).astype(np.float64))
        y_ref = g.once("Ax_int", lambda: g.A @ x)
        y_a = eng.spmv(x)
        assert np.array_equal(y_a, y_ref), (g.name, mode, np.flatnonzero(y_a != y_ref)[:8])
        eng.set_option("operator", LAP)
        y_l = eng.spmv(x)
        assert np.array_equal(y_l, g.d * x - y_ref), (g.name, mode, np.flatnonzero(y_l != g.d * x - y_ref)[:8])
        eng.set_option("operator", 0)
        assert np.array_equal(eng.spmv(x), y_a), (g.name, mode)
    run_pairs(pkg, oracle, "exact SpMV", body)


def test_laplacian_lanczos(pkg, oracle):
    """The lazy loop under L in every blocked form, with test_gpu_laplacian's tolerances: alpha_0, beta_0 1e-12 and alpha_1
    1e-10 of extended-precision host values, the three-term recurrence with scipy's L at 1e-12 * scale on every column,
    unit columns at 1e-13, and the breakdown stop from x0 = ones.  Where the tables would let the A loop defer k_pb_finish
    (finish_deferrable: asserted for MODES[4] on er_200k) the loop under L must not."""
    deferrable = []

    def body(i, mode, g, eng):
        what = (g.name, mode)
        k = min(20, g.n - 1)
        x0 = g.once("x0", lambda: np.random.default_rng(2).standard_normal(g.n))
        if eng.shape("finish_deferrable") == 1:
            deferrable.append((i, g.name))
        if i == 4 and g.name == "er_200k":
            assert eng.shape("finish_deferrable") == 1, what
        eng.set_option("operator", LAP)
        a, b, Q, xn, st = eng.lanczos(x0, k)
        assert st["iters"] == k, what
        a0, b0, a1 = g.once(("start", xn), lambda: g.lanczos_start(x0, xn))
        print(g.name, i, f"alpha_0 {abs(a[0] - a0) / abs(a0):.1e} beta_0 {abs(b[0] - b0) / abs(b0):.1e} alpha_1 {abs(a[1] - a1) / max(abs(a1), abs(a0)):.1e}")
        assert abs(a[0] - a0) <= 1e-12 * abs(a0) and abs(b[0] - b0) <= 1e-12 * abs(b0), what
        assert abs(a[1] - a1) <= 1e-10 * max(abs(a1), abs(a0)), what
        scale = max(np.abs(a).max(), np.abs(b).max())
        for j in range(k - 1):
            r = g.L @ Q[j] - a[j] * Q[j] - b[j] * Q[j + 1] - (b[j - 1] * Q[j - 1] if j else 0.0)
            assert np.abs(r).max() <= 1e-12 * scale, (what, j, np.abs(r).max() / scale)
            assert abs(np.linalg.norm(Q[j]) - 1.0) <= 1e-13, (what, j)
        # x0 = ones: fixed by the heat kernel, the stop fires at j = 0
        assert np.abs(eng.expm_multiply(np.ones(g.n), k, 1.0) - 1.0).max() <= 1e-12, what
        a1s, b1s, Q1s, _, _ = eng.lanczos(np.ones(g.n), k)
        assert np.all(b1s == 0.0) and np.all(a1s[1:] == 0.0) and np.all(Q1s[1:] == 0.0), what
    run_pairs(pkg, oracle, "Laplacian Lanczos", body)
    print("finish_deferrable == 1:", deferrable)
    assert (4, "er_200k") in deferrable


def check_pairs(g, M, w, V, info, w_ref, V_ref, what):
    """test_gpu_eigsh.check_pairs with its numbers; the reported residuals at the C2 test's 1e-11 * norm where n > 10000."""
    nev = len(w)
    norm = max(abs(w_ref).max(), info["norm_est"])
    assert info["converged"] == nev and np.all(np.isfinite(w)) and np.all(np.isfinite(V)), (what, info)
    assert np.abs(w - w_ref).max() <= 1e-9 * norm, (what, w, w_ref)
    assert np.abs(V.T @ V - np.eye(nev)).max() <= 1e-10, what
    true_res = np.linalg.norm(M @ V - V * w, axis=0)
    assert np.abs(info["resid"] - true_res).max() <= (1e-11 if g.big else 1e-12) * norm, (what, info["resid"], true_res)
    assert true_res.max() <= 1e-8 * norm, (what, true_res)
    for i in range(nev):   # the sign convention: the entry of largest magnitude (first on a tie) is positive
        assert V[np.argmax(np.abs(V[:, i])), i] > 0, what
    if V_ref is None:
        return
    for i in range(nev):
        others = np.delete(w_ref, i) if len(w_ref) > 1 else np.array([np.inf])
        gap = np.abs(others - w_ref[i]).min()
        if gap > 1e-6 * norm:
            c = abs(V[:, i] @ V_ref[:, i])
            assert 1.0 - c <= max(1e-8, 2.0 * (true_res[i] / gap) ** 2), (what, i, c, gap)


def test_eigsh(pkg, oracle):
    """The residual SpMV (+ k_lap_apply over n_loc_pad) of the eigensolver in every blocked form: the 4 largest pairs of A,
    the 2 largest of L and, on the connected graphs, the Fiedler pair with the constant vector deflated."""
    def body(i, mode, g, eng):
        w_ref, V_ref = g.extreme(0, 4)
        w, V, info = eng.eigsh(nev=4, which="LA", m=EIG_M, tol=1e-10, max_restarts=1000)
        check_pairs(g, g.A, w, V, info, w_ref, V_ref, (g.name, mode, "A LA"))
        eng.set_option("operator", LAP)
        w_ref, V_ref = g.extreme(LAP, 2)
        w, V, info = eng.eigsh(nev=2, which="LA", m=EIG_M, tol=1e-10, max_restarts=1000)
        check_pairs(g, g.L, w, V, info, w_ref, V_ref, (g.name, mode, "L LA"))
        if g.connected:
            w_ref, V_ref = g.extreme(LAP, 1, smallest=True)
            w, V, info = eng.eigsh(nev=1, which="SA", m=EIG_M, tol=1e-10, max_restarts=1000, deflate=np.full(g.n, 1.0 / np.sqrt(g.n)))
            assert abs(np.sum(V[:, 0])) <= 1e-10 * np.sqrt(g.n), (g.name, mode)
            check_pairs(g, g.L, w, V, info, w_ref, V_ref, (g.name, mode, "L SA"))
    engaged = run_pairs(pkg, oracle, "eigsh", body)
    assert any(graph(oracle, n).connected for names in engaged.values() for n in names)


def test_multishift_cg(pkg, oracle):
    """p . S p comes from the SpMV's partials (rewritten by k_lap_apply under L): (a) three iterations against the numpy
    restatement at 1e-12 pin them in every blocked form; (b) the converged run: true residuals, the reported ones, the order
    of the freeze iterations, and the solution itself against spsolve where n <= 10000 (above, the residual bounds the error
    by ||r|| / (sigma - lambda_max) under A and ||r|| / sigma under L)."""
    tol = 1e-10

    def body(i, mode, g, eng):
        for op in (0, LAP):
            eng.set_option("operator", op)
            shifts = g.shifts(op)
            for bname, b in g.rhs(op):
                what = (g.name, mode, op, bname)
                bn = np.linalg.norm(b)
                ref3, iters3, conv3 = g.cg3(op, bname)
                try:     # LZX_ERR_LIMIT with the partial result, unless the restatement itself is through within three steps
                    X3, info3 = eng.solve_shifted(b, shifts, tol=tol, maxiter=3)
                    assert conv3.all(), what
                except pkg.LzxError as e:
                    assert "(-6)" in str(e) and not conv3.all(), (what, str(e))
                    X3, info3 = e.partial
                err3 = np.abs(X3 - ref3).max() / np.abs(ref3).max()
                assert list(info3["iters"]) == list(iters3) and info3["converged"] == conv3.sum(), (what, info3, iters3)
                assert err3 <= 1e-12, (what, err3)
                X, info = eng.solve_shifted(b, shifts, tol=tol, maxiter=50000)
                assert info["converged"] == 3 and info["launched"] >= info["iterations"] == info["iters"].max(), (what, info)
                assert abs(info["bnorm"] - bn) <= 1e-12 * bn, what
                for s, sig in enumerate(shifts):
                    res = g.residual(op, sig, X[s], b)
                    assert res <= 10 * tol, (what, sig, res)
                    assert abs(info["resid"][s] - res) <= (1e-11 if g.big else 1e-12), (what, sig, info["resid"][s], res)
                    if not g.big:
                        ref, kappa = g.direct(op, bname)[s]
                        assert np.linalg.norm(X[s] - ref) <= kappa * 10 * tol * np.linalg.norm(ref), (what, sig)
                o = np.argsort(shifts)   # the nearer the spectrum, the longer
                assert np.all(np.diff(info["iters"][o].astype(np.int64)) <= 0), (what, info["iters"])
    run_pairs(pkg, oracle, "multi-shift CG", body)


def test_no_form_state_leaks_between_entry_points(pkg, oracle):
    """A handle whose lazy A loop has just deferred k_pb_finish (finish_deferrable == 1) answers spmv, eigsh and
    solve_shifted with the bits of a fresh handle -- lzx.h promises determinism for identical graph, options and arguments --
    and again under L, whose degree array is built on its first use."""
    g = graph(oracle, "er_200k")
    mode = MODES[4]
    x = np.random.default_rng(11).standard_normal(g.n)
    b = np.random.default_rng(12).standard_normal(g.n)
    x0 = np.random.default_rng(13).standard_normal(g.n)

    def calls(eng, op):
        y = eng.spmv(x)
        w, V, ei = eng.eigsh(nev=2 if op else 4, which="LA", m=EIG_M, tol=1e-10, max_restarts=1000)
        X, si = eng.solve_shifted(b, g.shifts(op), tol=1e-10, maxiter=50000)
        return [y, w, V, ei["resid"], np.array([ei[f] for f in ("converged", "restarts", "matvecs", "m", "norm_est")]),
                X, si["resid"], si["iters"], np.array([si[f] for f in ("iterations", "launched", "converged", "bnorm")])]

    used = pkg.Engine(0, **mode)
    try:
        used.set_graph_csr(g.rp, g.ci)
        assert used.info()["pb_entries"] > 0 and used.shape("finish_deferrable") == 1
        for op in (0, LAP):
            used.set_option("operator", op)
            a, bb, _, _, st = used.lanczos(x0, 12, want_q=False)      # the lazy loop (under A: with the finish deferred)
            assert st["iters"] == 12 and np.all(np.isfinite(a)) and np.all(np.isfinite(bb))
            got = calls(used, op)
            fresh = pkg.Engine(0, **mode)
            try:
                fresh.set_graph_csr(g.rp, g.ci)
                fresh.set_option("operator", op)
                want = calls(fresh, op)
            finally:
                fresh.close()
            for what, u, v in zip(("spmv", "w", "V", "eig resid", "eig info", "X", "solve resid", "iters", "solve info"), got, want):
                assert np.array_equal(u, v), (op, what)
            assert np.allclose(got[0], g.M(op) @ x, rtol=0, atol=1e-12 * np.abs(got[0]).max()), op
    finally:
        used.close()
