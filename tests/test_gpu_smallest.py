"""GPU: every entry point on the ten smallest graphs of tests/test_smallest_host.py -- one vertex, a self loop, two and three
vertices, 65 vertices without an edge, a star of 65, one edge among 1025 vertices -- and on ranks that own no row or no entry.

The matrix.  One parametrised test per entry-point family over the ten graphs; every (graph, entry point) cell is an ANSWER
cell (the output equals the reference of the host module: equality for integers, single divisions and integer-valued SpMV /
SpMM; the tolerances of the named existing tests everywhere else) or a REFUSAL cell (a sentence of include/lzx.h excludes the
shape: the stated code comes back and the handle still answers spmv).  REFUSALS is the table of the latter, each row quoting
its sentence.  A cell records itself in CELLS once its assertions have passed; test_every_cell_ran_and_the_refusals_are_the_table,
last in the file, asserts that no cell of graphs x entry points is missing and that the refusal cells are exactly the table.
That test is a condition on the whole module: it fails when the module is run in part.

Tolerances, each from the test it names: alpha_0, beta_0 1e-12 and alpha_1 1e-10 (test_gpu_parity.check_leading_coefficients),
where the reference value itself is exactly 0 by cancellation (the constant vector under L) 1e-12 of the Gershgorin norm the
library's own breakdown rule is scaled by; e^(sM) x 1e-12 relative infinity norm against the dense exponential
(test_gpu_multi.test_breakdown_stop); eigsh: test_gpu_eigsh.check_pairs; the solvers: test_gpu_forms.test_multishift_cg's
residual, reported-residual and kappa * 10 * tol rules with kappa from the dense spectrum; PageRank:
test_gpu_pagerank.check_against_dense with the stop-rule bound; quadrature: test_gpu_trace.test_trace_exact_on_small_graphs'
1e-10 on the log quadratures and test_diag_expm_matches_expm_multiply's 1e-10.  Every toleranced family prints its largest
error."""
import os
import re
import time

import numpy as np
import pytest

from test_communities_host import chain, modularity_ref
from test_components_host import components_restatement, counts_of, scipy_labels
from test_core_host import INTS as CORE_INTS
from test_core_host import peel_rounds
from test_gpu_eigsh import check_pairs
from test_gpu_forms import staged_columns, will_engage
from test_gpu_pagerank import check_against_dense, stop_rule_bound
from test_gpu_parity import check_leading_coefficients
from test_pagerank_host import DAMPINGS, TOL, Case
from test_paths_host import assert_bc_close, bc_bound, brandes_batched
from test_similarity_host import similarity_restated, sum_error_ratio
from test_smallest_host import LAP, LD, MULTI_K, NAMES, krylov_dimension, lanczos_case, lanczos_ld, multi_case, small
from test_sweep_host import ASCENDING, EXPANSION, PER_DEGREE, result_of, sweep_ref
from test_trace_host import probe_np
from test_triangles_host import triangles_oriented
from test_truss_host import truss_rounds

pytestmark = pytest.mark.gpu

ERR_ARG = -1
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lzx.h")
ALL = tuple(NAMES)

HANDOVER = ("set_graph_csr", "set_graph_csr32", "set_graph_edges", "get_graph_csr", "info")
CORE = ("spmv", "spmm", "lanczos", "lanczos_chunks", "multout", "multout_change", "expm_multiply", "lanczos_multi", "multout_multi",
        "multout_multi_k_beyond")
QUADRATURE = ("probes", "lanczos_probes", "probe_diag", "trace_expm", "diag_expm")
LINALG = ("eigsh", "solve_shifted", "solve_multi", "pagerank", "katz")
ROUTINES = ("components", "induced_all", "induced_one", "induced_none", "bfs", "betweenness_raw", "closeness", "triangles_raw",
            "core_number_raw", "truss_raw", "similarity_pairs", "similarity_pair_0_0", "similarity_edges", "color_raw",
            "label_propagation_raw", "modularity_raw", "sweep_cut_raw", "sweep_cut_k_max_beyond")
ENTRY_POINTS = HANDOVER + CORE + QUADRATURE + LINALG + ROUTINES

# (entry point, graphs, code, the sentence of include/lzx.h that excludes the shape)
REFUSALS = [
    ("eigsh", ("v1", "loop1", "v2_empty", "edge2"), ERR_ARG,
     "limits    1 <= nev, nev + 2 <= m <= 128, m + nw <= n; m = 0 picks max(2 nev + 1, 20) clipped to those limits.  LZX_ERR_ARG: "
     "null handle, nev = 0, unknown `which`, tol <= 0, a size rule above."),
    ("multout_multi_k_beyond", ALL, ERR_ARG,
     "b must be the resident batch's, k at most its k (LZX_ERR_ARG otherwise; LZX_ERR_STATE when no batch is resident)."),
    ("induced_none", ALL, ERR_ARG,
     "errors    LZX_ERR_ARG: null dst, src or keep; nothing kept; handles on different GPUs (the message names both devices)."),
    ("similarity_pair_0_0", ALL, ERR_ARG,
     "u[p] >= n, v[p] >= n or u[p] == v[p] (the lists are the host's: both are checked before the device is touched)."),
    ("sweep_cut_k_max_beyond", ALL, ERR_ARG,
     "errors    LZX_ERR_ARG: null handle, scores or best; ns = 0; a flag bit other than the three; k_max > n; k_min > k_max"),
]
REFUSAL_CELLS = {(name, entry): code for entry, names, code, _ in REFUSALS for name in names}

CELLS = {}       # (graph, entry point) -> "answer" | "refusal", written by a cell whose assertions have passed
WORST = {}       # toleranced family -> (largest observed error / its tolerance, error, tolerance, where)
SLOW = []        # (seconds, test id)
_HALT = []       # a HIP error ends the module's use of the GPU: nothing more is started on a device that may have faulted


def note(family, err, tol, where):
    """remember the largest error of a toleranced family, relative to the tolerance it was held to"""
    ratio = float(err) / tol if tol > 0 else (0.0 if err == 0 else np.inf)
    if family not in WORST or ratio > WORST[family][0]:
        WORST[family] = (ratio, float(err), tol, where)


class Cells:
    """The cells of one (family, graph) test: `with cells(entry):` runs one, records it when its assertions pass and keeps the
    failure otherwise, so that one failed cell does not hide the others; done() reports all of them."""

    def __init__(self, name):
        assert not _HALT, f"not run: a HIP error was met earlier in this module ({_HALT[0]})"
        self.name, self.failed, self.t0 = name, [], time.time()

    def __call__(self, entry):
        self.entry = entry
        return self

    def __enter__(self):
        return self

    def __exit__(self, kind, err, tb):
        if kind is None:
            CELLS[(self.name, self.entry)] = "refusal" if (self.name, self.entry) in REFUSAL_CELLS else "answer"
            return False
        if "(-2)" in str(err) or not issubclass(kind, Exception):
            _HALT.append(f"{self.name} / {self.entry}: {str(err)[:300]}")
            return False
        self.failed.append(f"{self.entry}: {kind.__name__}: {str(err)[:500]}")
        return True

    def done(self, what):
        SLOW.append((time.time() - self.t0, f"{what}[{self.name}]"))
        assert not self.failed, f"{what} on {self.name}: {len(self.failed)} cells failed:\n" + "\n".join(self.failed)


class halting:
    """outside the matrix: a HIP error met in the body stops every later test of the module before it starts anything"""

    def __init__(self, what):
        assert not _HALT, f"not run: a HIP error was met earlier in this module ({_HALT[0]})"
        self.what, self.t0 = what, time.time()

    def __enter__(self):
        return self

    def __exit__(self, kind, err, tb):
        SLOW.append((time.time() - self.t0, self.what))
        if kind is not None and ("(-2)" in str(err) or not issubclass(kind, Exception)):
            _HALT.append(f"{self.what}: {str(err)[:300]}")
        return False


def refused(pkg, name, entry, call):
    """the call raises the code the table states for this cell"""
    code = REFUSAL_CELLS[(name, entry)]
    try:
        call()
    except pkg.LzxError as e:
        assert f"({code})" in str(e), (name, entry, str(e))
    else:
        raise AssertionError(f"{entry} on {name} was not refused")


def engine(pkg, g, **options):
    eng = pkg.Engine(0, **options)
    eng.set_graph_csr(g.rp, g.ci)
    return eng


def check_spmv(eng, g, op=0):
    """integer-valued x: M x must EQUAL the host's"""
    x = g.x_int()
    want = (g.M(op) @ x.astype(LD)).astype(np.float64)
    y = eng.spmv(x)
    assert np.array_equal(y, want), (g.name, op, np.flatnonzero(y != want)[:8])


def rel_inf(a, b):
    top = np.abs(b).max()
    return np.abs(a - b).max() / top if top > 0 else np.abs(a).max()


def check_expm(family, got, want, where):
    err = rel_inf(got, want)
    note(family, err, 1e-12, where)
    assert err <= 1e-12, (where, err)


def check_coefficients(g, op, a, b, a_ref, b_ref, k, where):
    """check_leading_coefficients on the first k coefficients (k = the Krylov dimension: b has k - 1 entries that count);
    a reference alpha_0 that is exactly 0 is a sum that cancels, held at 1e-12 of the Gershgorin norm"""
    a_ref, b_ref = np.asarray(a_ref[:k], dtype=np.float64), np.asarray(b_ref[:k - 1], dtype=np.float64)
    gersh = (2.0 if op else 1.0) * g.max_degree
    if a_ref[0] == 0.0:
        note("alpha_0 (reference exactly 0)", abs(a[0]), 1e-12 * gersh, where)
        assert abs(a[0]) <= 1e-12 * gersh, (where, a[0])
        a_ref = a_ref.copy()
        a_ref[0] = a[0]
    else:
        note("alpha_0", abs(a[0] - a_ref[0]) / abs(a_ref[0]), 1e-12, where)
    if k > 1:
        note("beta_0", abs(b[0] - b_ref[0]) / abs(b_ref[0]), 1e-12, where)
        note("alpha_1", abs(a[1] - a_ref[1]) / max(abs(a_ref[1]), abs(a_ref[0]), 1e-300), 1e-10, where)
    check_leading_coefficients(a[:k], b[:k - 1], a_ref, b_ref, where)


def expm_scale(op):
    return -1.0 if op else 1.0


def set_operator(eng_or_group, op):
    for e in getattr(eng_or_group, "engines", [eng_or_group]):
        e.set_option("operator", op)


# ---- hand-over ----------------------------------------------------------------------------------------------------------
def check_handed_over(eng, g, cells, entry):
    gi = eng.info()
    rp, ci = eng.get_graph_csr()
    assert np.array_equal(rp, g.rp) and np.array_equal(ci, g.ci), (entry, rp, ci)
    assert (gi["n"], gi["nnz"], gi["max_degree"], gi["active_vertices"]) == (g.n, g.nnz, g.max_degree, g.n_active), (entry, gi)
    assert gi["rows_local"] == g.n and gi["nnz_local"] == g.nnz and gi["world"] == 1, (entry, gi)
    check_spmv(eng, g)


@pytest.mark.parametrize("name", NAMES)
def test_handover(pkg, name):
    g, cells = small(name), Cells(name)
    eng = pkg.Engine(0)
    try:
        with cells("set_graph_csr"):
            eng.set_graph_csr(g.rp, g.ci)
            check_handed_over(eng, g, cells, "csr")
        with cells("get_graph_csr"):
            rp, ci = eng.get_graph_csr()
            assert rp.dtype == np.uint64 and ci.dtype == np.uint32 and np.array_equal(rp, g.rp) and np.array_equal(ci, g.ci)
        with cells("info"):
            gi = eng.info()
            assert (gi["n"], gi["nnz"], gi["max_degree"], gi["active_vertices"]) == (g.n, g.nnz, g.max_degree, g.n_active), gi
            assert gi["pb_entries"] == 0 and gi["rank"] == 0, gi
        with cells("set_graph_csr32"):
            eng.set_graph_csr32(g.rp, g.ci)
            check_handed_over(eng, g, cells, "csr32")
        with cells("set_graph_edges"):
            src = np.array([u for u, _ in g.edges], dtype=np.uint32)
            dst = np.array([v for _, v in g.edges], dtype=np.uint32)
            eng.set_graph_edges(g.n, src, dst)                       # m = 0 on the graphs without an edge
            check_handed_over(eng, g, cells, "edges")
            eng.set_graph_edges(g.n, np.r_[dst, src, src], np.r_[src, dst, dst])     # any order, duplicates allowed
            check_handed_over(eng, g, cells, "edges, repeated")
    finally:
        eng.close()
    cells.done("hand-over")


# ---- core path ------------------------------------------------------------------------------------------------------------
def core_path_cells(pkg, eng, g, cells, batched=True):
    """the core-path cells on one handle, under A and under L"""
    for op in (0, LAP):
        where = (g.name, "L" if op else "A")
        set_operator(eng, op)
        s = expm_scale(op)
        x0, k, a_ref, b_ref, xn_ref = lanczos_case(g.name, op)
        want = g.expm(op, s, x0)
        with cells("spmv"):
            check_spmv(eng, g, op)
        if batched:
            with cells("spmm"):
                for b in (1, 3, 16):
                    X = g.x_int(seed=10 + b, b=b)
                    Y = eng.spmm(X)
                    assert np.array_equal(Y, (X.astype(LD) @ g.M(op).T).astype(np.float64)), (where, b)
        whole = None
        with cells("lanczos"):
            a, b, Q, xn, st = eng.lanczos(x0, k)
            whole = (a, b, Q)
            assert st["iters"] == k and abs(xn - xn_ref) <= 1e-12 * xn_ref, (where, st, xn, xn_ref)
            check_coefficients(g, op, a, b, a_ref, b_ref, k, where)
        with cells("multout"):
            assert whole is not None
            t = pkg._expm_coefficients(whole[0], whole[1], xn, s)
            check_expm("e^(sM) x, single vector", eng.multout(t), want, where)
        with cells("multout_change"):
            assert whole is not None
            eng.lanczos(x0, k, want_q=False)
            y1 = eng.multout(t)
            assert eng.multout_change(t) == 1.0, where                # the first call since the prepare
            assert eng.multout_change(t) == 0.0, where                # the same answer again
            t2 = t * np.linspace(1.0, 2.0, k)
            y2 = eng.multout(t2)
            change = eng.multout_change(t2)
            ref = float(np.sqrt(np.sum((y2.astype(LD) - y1.astype(LD)) ** 2)) / np.sqrt(np.sum(y2.astype(LD) ** 2)))
            note("multout_change", abs(change - ref), 1e-12, where)
            assert abs(change - ref) <= 1e-12, (where, change, ref)
        with cells("lanczos_chunks"):
            assert whole is not None
            xn2 = eng.lanczos_prepare(x0, k)
            for j in range(k):
                assert eng.lanczos_progress() == (j, k), where
                eng.lanczos_run_steps(1)
            a2, b2, Q2 = eng.lanczos_fetch(k, want_q=True)
            assert xn2 == xn and np.array_equal(a2, whole[0]) and np.array_equal(b2, whole[1]) and np.array_equal(Q2, whole[2]), where
        with cells("expm_multiply"):
            y = eng.expm_multiply(x0, k, 1.0)
            check_expm("e^(sM) x, single vector", y, want, where)
            assert whole is None or np.array_equal(y, eng.multout(pkg._expm_coefficients(whole[0], whole[1], xn, s))), where
        if not batched:
            continue
        X0, ku_ref = multi_case(g.name, op)
        multi = None
        with cells("lanczos_multi"):
            a, b, ku, xn, Q, st = eng.lanczos_multi(X0, MULTI_K, want_q=True)
            multi = (a, b, ku, xn)
            assert np.array_equal(ku, ku_ref), (where, ku, ku_ref)
            for c in range(len(X0)):
                kc = int(ku[c])
                assert not a[c, kc:].any() and not b[c, kc - 1:].any() and not Q[c, kc:].any(), (where, c, a[c], b[c])   # zeros behind
                ar, br, xr = lanczos_ld(g.M(op), X0[c], kc)
                assert abs(xn[c] - xr) <= 1e-12 * xr, (where, c)
                check_coefficients(g, op, a[c], b[c], ar, br, kc, where + (c,))
        with cells("multout_multi"):
            assert multi is not None
            a, b, ku, xn = multi
            T = np.vstack([pkg._expm_coefficients(a[c], b[c][:MULTI_K - 1], xn[c], s) for c in range(len(X0))])
            ans = eng.multout_multi(T)
            for c in range(len(X0)):
                check_expm("e^(sM) X, batched", ans[c], g.expm(op, s, X0[c]), where + (c,))
        with cells("multout_multi_k_beyond"):
            assert multi is not None
            refused(pkg, g.name, "multout_multi_k_beyond", lambda: eng.multout_multi(np.ones((len(X0), MULTI_K + 1))))
            check_spmv(eng, g, op)
    set_operator(eng, 0)


@pytest.mark.parametrize("name", NAMES)
def test_core_path(pkg, name):
    g, cells = small(name), Cells(name)
    eng = engine(pkg, g)
    try:
        core_path_cells(pkg, eng, g, cells)
    finally:
        eng.close()
    cells.done("core path")


# ---- quadrature -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_quadrature(pkg, name):
    g, cells = small(name), Cells(name)
    n, N, seed = g.n, 16, 2026
    eng = engine(pkg, g)
    try:
        for op in (0, LAP):
            where = (name, "L" if op else "A")
            eng.set_option("operator", op)
            lam_max = float(g.lam(0)[0][-1])
            t = (5.0 / (2.0 * g.max_degree) if g.max_degree else 1.0) if op else (6.0 / lam_max if lam_max > 0 else 1.0)
            s = -t if op else t
            sigma = 0.0 if op else max(lam_max, 0.0)
            Z = np.stack([probe_np(seed, p, n) for p in range(N)])
            with cells("probes"):
                assert np.array_equal(eng.probes(seed, 0, N), Z), where
                assert np.array_equal(eng.probes(seed, 7, 3), Z[7:10]), where
            with cells("lanczos_probes"):
                a, b, ku, st = eng.lanczos_probes(seed, 0, 5, MULTI_K)
                am, bm, kum, xnm, _, _ = eng.lanczos_multi(Z[:5], MULTI_K)
                assert np.array_equal(a, am) and np.array_equal(b, bm) and np.array_equal(ku, kum), where    # lzx.h: bit-identical
                assert list(ku) == [min(krylov_dimension(g.M(op), z), MULTI_K) for z in Z[:5]], (where, ku)
                ak, bk, kuk, _ = eng.lanczos_probes(seed, 0, 5, MULTI_K, keep_basis=True)
                assert np.array_equal(a, ak) and np.array_equal(b, bk) and np.array_equal(ku, kuk), where
            with cells("probe_diag"):
                a, b, ku, _ = eng.lanczos_probes(seed, 0, 5, MULTI_K, keep_basis=True)
                T = pkg.slq_diag_coefficients(a, b, ku, n, s, sigma)
                T[1] *= -3.0                                         # any weights
                Y = eng.multout_multi(T)
                want = np.zeros(n)
                for c in range(5):
                    want = want + Z[c] * Y[c]
                assert np.array_equal(eng.probe_diag(T), want), where            # test_probe_diag_is_the_reduced_multout
            with cells("trace_expm"):
                lt, rel, ell = eng.trace_expm(t, n_probes=N, k=MULTI_K, seed=seed)
                _, _, ell_long = eng.trace_expm(t, n_probes=N, k=2 * MULTI_K, seed=seed)
                assert np.abs(ell - ell_long).max() <= 1e-12, where                # converged at k: the Krylov spaces are closed
                E = g.expm(op, s, Z.T)
                ref = np.log(np.einsum("in,ni->i", Z, E))
                note("log quadratures", np.abs(ell - ref).max(), 1e-10, where)
                assert np.abs(ell - ref).max() <= 1e-10, (where, np.abs(ell - ref).max())
                assert np.isfinite(lt) and (np.isfinite(rel) and rel >= 0), (where, lt, rel)
            with cells("diag_expm"):
                est, shift = eng.diag_expm(t, n_probes=N, k=MULTI_K, seed=seed)
                assert op == 0 or shift == 0.0, where
                Y = (g.expm(op, s, Z.T) * np.exp(-s * shift)).T
                ref = (Z * Y).sum(axis=0) / N
                err = np.abs(est - ref).max() / np.abs(ref).max()
                note("diag e^(sM) estimate", err, 1e-10, where)
                assert err <= 1e-10, (where, err)
    finally:
        eng.close()
    cells.done("quadrature")


# ---- linear algebra -------------------------------------------------------------------------------------------------------
def eigsh_cell(pkg, eng, g, op, where):
    """the largest pairs of M: one where n = 3 (nev + 2 <= m <= n), two otherwise, with m = 0 (the library's choice)"""
    nev = 1 if g.n == 3 else 2
    lam, U = g.lam(op)
    norm = float(np.abs(lam).max())
    w_ref = lam[-nev:]
    simple = all(np.sum(np.abs(lam - x) <= 1e-9 * max(norm, 1.0)) == 1 for x in w_ref)
    # (three vertices: eight seeds, so that first probes on either side of every plane x_i = +-x_j occur -- the Krylov space of
    #  one that lies in such a plane misses an eigenvector, and the fresh start after its breakdown has to find it)
    for seed in (range(8) if g.n == 3 else (0,)):
        w, V, info = eng.eigsh(nev=nev, which="LA", m=0, tol=1e-10, max_restarts=300, seed=seed)
        assert info["converged"] == nev and info["m"] == min(20, g.n), (where, seed, info)
        print(where, f"eigsh seed {seed} restarts {info['restarts']} matvecs {info['matvecs']} |w - w_ref| {np.abs(w - w_ref).max():.1e}")
        note("eigenvalues", np.abs(w - w_ref).max(), 1e-9 * norm, where + (seed,))
        check_pairs(g.M64(op), w, V, info, w_ref, U[:, -nev:] if simple else None, norm, where + (seed,))


def shifts_of(g, op):
    """test_gpu_forms.Graph.shifts, with lambda_max(A) = 0 (no edge) replaced by 1 so that sigma I is positive definite"""
    lam_max = max(float(g.lam(0)[0][-1]), 0.0)
    return 1.0 / np.array([0.1, 1.0, 10.0]) if op else np.array([1.02, 1.2, 2.0]) * (lam_max if lam_max > 0 else 1.0)


def residual_ld(g, op, sig, x, b):
    Mx = g.M(op) @ x.astype(LD)
    r = b.astype(LD) - (LD(sig) * x.astype(LD) + Mx if op else LD(sig) * x.astype(LD) - Mx)
    return float(np.sqrt(np.sum(r * r)) / np.sqrt(np.sum(b.astype(LD) ** 2)))


def check_solution(g, op, sig, x, b, resid, where, tol=1e-10):
    """test_gpu_forms.test_multishift_cg's rules for one converged system"""
    lam = g.lam(op)[0]
    S = sig * np.eye(g.n) + g.M64(op) if op else sig * np.eye(g.n) - g.M64(op)
    kappa = (sig + lam[-1]) / sig if op else (sig - lam[0]) / (sig - lam[-1])
    res = residual_ld(g, op, sig, x, b)
    ref = np.linalg.solve(S, b)
    err = np.linalg.norm(x - ref) / np.linalg.norm(ref)
    note("solver residual", res, 10 * tol, where)
    note("solver reported residual", abs(resid - res), 1e-12, where)
    note("solver error / (kappa 10 tol)", err, kappa * 10 * tol, where)
    assert res <= 10 * tol, (where, sig, res)
    assert abs(resid - res) <= 1e-12, (where, sig, resid, res)
    assert err <= kappa * 10 * tol, (where, sig, err, kappa)


def solve_shifted_cell(pkg, eng, g, op, where):
    b = np.random.default_rng(7).standard_normal(g.n)
    shifts = shifts_of(g, op)
    X, info = eng.solve_shifted(b, shifts, tol=1e-10, maxiter=1000)
    bn = np.linalg.norm(b)
    assert info["converged"] == 3 and info["launched"] >= info["iterations"] == info["iters"].max(), (where, info)
    assert abs(info["bnorm"] - bn) <= 1e-12 * bn, where
    for s, sig in enumerate(shifts):
        check_solution(g, op, sig, X[s], b, info["resid"][s], where)
    assert np.all(np.diff(info["iters"][np.argsort(shifts)].astype(np.int64)) <= 0), (where, info["iters"])


@pytest.mark.parametrize("name", NAMES)
def test_linear_algebra(pkg, name):
    g, cells = small(name), Cells(name)
    eng = engine(pkg, g)
    try:
        for op in (0, LAP):
            where = (name, "L" if op else "A")
            eng.set_option("operator", op)
            with cells("eigsh"):
                if (name, "eigsh") in REFUSAL_CELLS:
                    x0, k, _, _, _ = lanczos_case(name, op)
                    eng.lanczos_prepare(x0, k)
                    for nev, m in ((1, 0), (1, 3), (2, 0)):
                        refused(pkg, name, "eigsh", lambda: eng.eigsh(nev=nev, which="LA", m=m))
                    assert eng.lanczos_progress() == (0, k), where        # refused before the call voided anything
                    check_spmv(eng, g, op)
                else:
                    eigsh_cell(pkg, eng, g, op, where)
            with cells("solve_shifted"):
                solve_shifted_cell(pkg, eng, g, op, where)
            with cells("solve_multi"):
                B = np.random.default_rng(12).standard_normal((3, g.n))
                shifts = shifts_of(g, op)
                X, info = eng.solve_multi(B, shifts, tol=1e-10, maxiter=1000)
                assert info["converged"] == 3 and not info["status"].any(), (where, info)
                for c, sig in enumerate(shifts):
                    check_solution(g, op, sig, X[c], B[c], info["resid"][c], where + (c,))
        eng.set_option("operator", 0)
        with cells("pagerank"):
            hot = np.zeros(g.n)
            hot[0] = 1.0
            case = Case(name, g.rp, g.ci, vs=[("uniform", np.full(g.n, 1.0 / g.n)), ("onehot", hot)])
            for vname, v in case.vs():
                X, info = eng.pagerank(DAMPINGS, personalization=None if vname == "uniform" else v, tol=TOL)
                check_against_dense(case, vname, v, X, info, (name, vname), stop_rule_bound(case, v))
        with cells("katz"):
            lam = g.lam(0)[0]
            al = 0.5 / (lam[-1] if lam[-1] > 0 else 1.0)
            x = eng.katz(alpha=al, normalized=False, tol=1e-10)
            ref = np.linalg.solve(np.eye(g.n) - al * g.M64(0), np.ones(g.n))
            kappa = (1.0 / al - lam[0]) / (1.0 / al - lam[-1])
            err = np.linalg.norm(x - ref) / np.linalg.norm(ref)
            note("solver error / (kappa 10 tol)", err, kappa * 10 * 1e-10, (name, "katz"))
            assert err <= kappa * 10 * 1e-10, (name, err, kappa)
            X = x[None, :]                                         # Engine.katz's own normalisation, on the same bits
            assert np.array_equal(eng.katz(alpha=al, tol=1e-10), (X / (np.sign(X.sum(axis=1)) * np.linalg.norm(X, axis=1))[:, None])[0]), name
    finally:
        eng.close()
    cells.done("linear algebra")


# ---- graph routines -------------------------------------------------------------------------------------------------------
def similarity_direct(pkg, eng, u, v):
    """lzx_similarity on one pair through the C ABI itself (Engine.similarity_raw refuses u == v before the library sees it):
    (code, the outputs it was handed, filled with a sentinel)"""
    pu, pv = np.array([u], dtype=np.uint32), np.array([v], dtype=np.uint32)
    common, du, dv = (np.full(1, 0xdeadbeef, dtype=np.uint32) for _ in range(3))
    vals = np.full(5, -7.0)
    rc = eng.L.lzx_similarity(eng.h, 1, pkg._p(pu, pkg._u32p), pkg._p(pv, pkg._u32p), 31, pkg._p(common, pkg._u32p), pkg._p(du, pkg._u32p),
                              pkg._p(dv, pkg._u32p), pkg._p(vals, pkg._f64p), None)
    return rc, common, du, dv, vals


@pytest.mark.parametrize("name", NAMES)
def test_graph_routines(pkg, name):
    g, cells = small(name), Cells(name)
    n, A = g.n, g.A
    eng = engine(pkg, g)
    try:
        with cells("components"):
            labels, info = eng.components()
            ref, rounds = components_restatement(g.rp, g.ci)
            assert np.array_equal(labels, ref) and np.array_equal(labels, scipy_labels(g.rp, g.ci)), labels
            assert (info["n_components"], info["largest_size"], info["largest_label"]) == counts_of(ref) and info["rounds"] == rounds, info
            assert eng.components(want_labels=False)[1]["n_components"] == info["n_components"]
        with cells("induced_all"):
            sub, old = eng.induced(np.ones(n, dtype=np.uint8))
            try:
                assert np.array_equal(old, np.arange(n))
                check_handed_over(sub, g, cells, "induced, all kept")
            finally:
                sub.close()
        with cells("induced_one"):
            for v in sorted({0, n - 1}):
                keep = np.zeros(n, dtype=np.uint8)
                keep[v] = 1
                sub, old = eng.induced(keep)
                try:
                    loop = int(g.Ad[v, v] != 0)
                    rp, ci = sub.get_graph_csr()
                    assert list(old) == [v] and list(rp) == [0, loop] and list(ci) == [0] * loop, (v, old, rp, ci)
                    gi = sub.info()
                    assert (gi["n"], gi["nnz"], gi["max_degree"], gi["active_vertices"]) == (1, loop, loop, loop), gi
                    assert np.array_equal(sub.spmv(np.array([-37.0])), np.array([-37.0 * loop]))
                finally:
                    sub.close()
        with cells("induced_none"):
            refused(pkg, name, "induced_none", lambda: eng.induced(np.zeros(n, dtype=np.uint8)))
            refused(pkg, name, "induced_none", lambda: eng.restrict(np.zeros(n, dtype=np.uint8)))
            check_handed_over(eng, g, cells, "after keep none")            # dst keeps the graph it had
            eng.n = n
        sources = np.arange(n) if n <= 65 else np.array([0, 7, 8, 512, 1024, 7])
        r = brandes_batched(A, sources)
        with cells("bfs"):
            D, P, info = eng.bfs(sources, paths=True)
            assert np.array_equal(D, r["dist"]) and np.array_equal(P, r["paths"])
            for key in ("reached", "sum_dist", "harmonic", "ecc"):
                assert np.array_equal(info[key], r[key]), (key, info[key], r[key])
            assert info["max_level"] == r["max_level"] and info["ns"] == len(sources), info
        with cells("closeness"):
            r1, tot = r["reached"].astype(np.float64) - 1.0, r["sum_dist"].astype(np.float64)
            want = np.zeros(len(sources))
            ok = (tot > 0) & (n > 1)
            want[ok] = (r1[ok] / tot[ok]) * (r1[ok] / (n - 1.0))
            assert np.array_equal(eng.closeness(sources), want)
            assert np.array_equal(eng.harmonic(sources), r["harmonic"])
        with cells("betweenness_raw"):
            every = brandes_batched(A, np.arange(n))
            bc, info = eng.betweenness_raw()
            assert_bc_close(bc, every["bc"], bc_bound(A, np.arange(n), every["max_level"]))
            bc, _ = eng.betweenness_raw(sources)
            assert_bc_close(bc, r["bc"], bc_bound(A, sources, r["max_level"]))
        with cells("triangles_raw"):
            tri, clus, info = eng.triangles_raw()
            t = triangles_oriented(A)
            assert np.array_equal(tri, t["tri"]) and np.array_equal(clus, t["clustering"])
            for key in ("triangles", "wedges", "max_triangles", "oriented_entries", "oriented_max_degree"):
                assert info[key] == t[key], (key, info[key], t[key])
            assert info["avg_clustering"] == float(t["clustering"].sum()) / n      # (every coefficient here is 0 or 1: exact)
        with cells("core_number_raw"):
            core, layer, info = eng.core_number_raw()
            p = peel_rounds(A)
            assert np.array_equal(core, p["core"]) and np.array_equal(layer, p["layer"])
            assert all(info[key] == p[key] for key in CORE_INTS), (info, {key: p[key] for key in CORE_INTS})
        with cells("truss_raw"):
            support, truss, layer, vertex, info = eng.truss_raw()
            t = truss_rounds(A)
            for key, got in (("support", support), ("truss", truss), ("layer", layer), ("vertex_truss", vertex)):
                assert np.array_equal(got, t[key]), (key, got, t[key])
            for key in ("edges", "triangles", "main_truss_edges", "max_support", "max_truss", "levels", "rounds"):
                assert info[key] == t[key], (key, info[key], t[key])
        with cells("similarity_pairs"):
            pairs = g.all_pairs()
            common, du, dv, values, info = eng.similarity_raw(pairs)
            s = similarity_restated(A, pairs)
            assert info["pairs"] == len(pairs) and len(common) == len(pairs)
            assert np.array_equal(common, s["common"]) and np.array_equal(du, s["deg_u"]) and np.array_equal(dv, s["deg_v"])
            for key in ("jaccard", "overlap", "sorensen"):
                assert np.array_equal(values[key], s[key]), key
            for key, terms in (("adamic_adar", "terms_aa"), ("resource_allocation", "terms_ra")):
                assert all(sum_error_ratio(got, tm) <= 1.0 for got, tm in zip(values[key], s[terms])), key
        with cells("similarity_pair_0_0"):
            rc, common, du, dv, vals = similarity_direct(pkg, eng, 0, 0)
            assert rc == REFUSAL_CELLS[(name, "similarity_pair_0_0")], rc
            assert "not compared with itself" in eng.L.lzx_last_error().decode(), eng.L.lzx_last_error()
            # before the device is touched: nothing the call was handed has been written
            assert common[0] == du[0] == dv[0] == 0xdeadbeef and np.all(vals == -7.0)
            check_spmv(eng, g)
        with cells("similarity_edges"):
            common, du, dv, values, info = eng.similarity_raw(None)         # np == nnz == 0 on the graphs without an edge
            rows = np.repeat(np.arange(n), np.diff(g.rp.astype(np.int64)))
            cols = g.ci.astype(np.int64)
            off = rows != cols
            s = similarity_restated(A, np.stack([rows[off], cols[off]], axis=1))
            assert info["pairs"] == g.nnz and len(common) == g.nnz
            assert not common[~off].any() and not du[~off].any() and not dv[~off].any()           # a diagonal entry carries 0
            assert np.array_equal(common[off], s["common"]) and np.array_equal(du[off], s["deg_u"]) and np.array_equal(dv[off], s["deg_v"])
            for key in ("jaccard", "overlap", "sorensen"):
                assert np.array_equal(values[key][off], s[key]) and not values[key][~off].any(), key
            for key, terms in (("adamic_adar", "terms_aa"), ("resource_allocation", "terms_ra")):
                assert all(sum_error_ratio(got, tm) <= 1.0 for got, tm in zip(values[key][off], s[terms])), key
        for by_id in (True, False):
            ref = chain(A, 0, by_id)
            with cells("color_raw"):
                color, info = eng.color_raw(0, ties_by_id=by_id)
                assert np.array_equal(color, ref["color"]), (by_id, color)
                assert all(info[key] == ref[key] for key in ("colors", "rounds", "largest_class")), (by_id, info)
            with cells("label_propagation_raw"):
                labels, info = eng.label_propagation_raw(0, ties_by_id=by_id)
                assert np.array_equal(labels, ref["labels"]), (by_id, labels)
                for key in ("n_communities", "largest_size", "largest_label", "sweeps", "updates", "colors", "color_rounds", "inner_entries",
                            "entries", "sum_degree_sq"):
                    assert info[key] == ref[key], (by_id, key, info[key], ref[key])
                assert info["modularity"] == ref["q"], (by_id, info["modularity"], ref["q"])
            with cells("modularity_raw"):
                for lab in (ref["labels"], np.zeros(n, dtype=np.uint32), np.arange(n, dtype=np.uint32)[::-1].copy()):
                    q, info = eng.modularity_raw(lab)
                    m = modularity_ref(A, lab)
                    assert q == m["q"] and all(info[key] == m[key] for key in ("communities", "inner_entries", "entries", "sum_degree_sq")), (lab, q, m)
        with cells("sweep_cut_raw"):
            scores = g.scores()
            for kw, flags in ((dict(), 0), (dict(ascending=True, per_degree=True, objective="expansion"), ASCENDING | PER_DEGREE | EXPANSION)):
                order, cut, vol, results, info = eng.sweep_cut_raw(scores, want_profile=True, **kw)
                assert info["entries"] == int(g.A0.nnz) and info["ns"] == 3, info
                for c, score in enumerate(scores):
                    w = sweep_ref(A, score, flags)
                    assert np.array_equal(order[c], w["order"]) and np.array_equal(cut[c], w["cut"]) and np.array_equal(vol[c], w["vol"]), (kw, c)
                    assert results[c] == result_of(w), (kw, c, results[c], result_of(w))
        with cells("sweep_cut_k_max_beyond"):
            refused(pkg, name, "sweep_cut_k_max_beyond", lambda: eng.sweep_cut_raw(g.scores(), k_max=n + 1))
            check_spmv(eng, g)
    finally:
        eng.close()
    cells.done("graph routines")


# ---- the blocked form, forced -----------------------------------------------------------------------------------------------
BLOCKED = [dict(propagation_blocking=1, hub_entries=2), dict(propagation_blocking=1, hub_entries=2, pb_reduce=1),
           dict(propagation_blocking=1, hub_entries=2, pb_reduce=0)]
ENGAGED = {}


@pytest.mark.parametrize("mode", BLOCKED, ids=["forced", "pb_reduce_1", "pb_reduce_0"])
@pytest.mark.parametrize("name", NAMES)
def test_blocked_forced(pkg, name, mode):
    """hub = min(hub_entries, n, 20000) & ~1 = 2 from three vertices on, and blocking is on when 0 < hub < n and an active column
    is unstaged: path3 and the triangle (one unstaged column) are the smallest graphs whose blocked passes engage.  The
    core-path cells, eigsh and solve_shifted there (they are cells of the matrix already: recorded by the plain tests)."""
    g = small(name)
    cells = Cells(name)
    eng = engine(pkg, g, **mode)
    try:
        gi = eng.info()
        engage = will_engage(mode, g.n, g.n_active)
        assert (gi["pb_entries"] > 0) == engage, (name, mode, gi)
        assert engage == (name in ("path3", "triangle", "star65")), (name, engage)
        if engage:
            assert gi["hub_entries"] == staged_columns(mode, g.n) == 2, gi
            ENGAGED.setdefault(name, []).append(mode)
        core_path_cells(pkg, eng, g, cells)
        for op in (0, LAP):
            where = (name, "L" if op else "A", "blocked")
            eng.set_option("operator", op)
            with cells("solve_shifted"):
                solve_shifted_cell(pkg, eng, g, op, where)
            if (name, "eigsh") not in REFUSAL_CELLS:
                with cells("eigsh"):
                    eigsh_cell(pkg, eng, g, op, where)
    finally:
        eng.close()
    cells.done("blocked")


def test_blocking_engaged_at_three_vertices():
    assert {"path3", "triangle", "star65"} <= set(ENGAGED) and all(len(v) == len(BLOCKED) for v in ENGAGED.values()), ENGAGED


# ---- in-process groups ------------------------------------------------------------------------------------------------------
WORLDS = (2, 3, 5, 8)
_GROUPS = {}
SEEN = dict(empty_rank=set(), entryless_rank=set())


def group(pkg, world, **options):
    """one group per (world, options) for the whole module: eight handles are not made anew for every graph"""
    key = (world, tuple(sorted(options.items())))
    if key not in _GROUPS:
        _GROUPS[key] = pkg.LocalGroup([0] * world, **options)
    return _GROUPS[key]


@pytest.fixture(scope="module", autouse=True)
def close_groups():
    yield
    for grp in _GROUPS.values():
        grp.close()
    _GROUPS.clear()


def group_cells(pkg, grp, g, ops=(0, LAP)):
    """spmv, lanczos, multout and expm_multiply over a group, with the same references; what the ranks' info() must add up to"""
    world = grp.world
    grp.set_graph_csr(g.rp, g.ci)
    infos = [e.info() for e in grp.engines]
    assert [gi["rank"] for gi in infos] == list(range(world)) and all(gi["world"] == world and gi["n"] == g.n and gi["nnz"] == g.nnz for gi in infos)
    assert sum(gi["rows_local"] for gi in infos) == g.n, [gi["rows_local"] for gi in infos]
    assert sum(gi["nnz_local"] for gi in infos) == g.nnz, [gi["nnz_local"] for gi in infos]
    if world > g.n:
        assert any(gi["rows_local"] == 0 for gi in infos), infos
        SEEN["empty_rank"].add((world, g.name))
    if world > g.n_active:
        assert any(gi["nnz_local"] == 0 for gi in infos), infos
        SEEN["entryless_rank"].add((world, g.name))
    for op in ops:
        where = (g.name, "L" if op else "A", f"world {world}")
        set_operator(grp, op)
        s = expm_scale(op)
        x = g.x_int()
        want = (g.M(op) @ x.astype(LD)).astype(np.float64)
        assert np.array_equal(grp.spmv(x), want), where
        x0, k, a_ref, b_ref, xn_ref = lanczos_case(g.name, op)
        a, b, Q, xn, st = grp.lanczos(x0, k)
        assert st["iters"] == k and abs(xn - xn_ref) <= 1e-12 * xn_ref, (where, st)
        check_coefficients(g, op, a, b, a_ref, b_ref, k, where)
        ref = g.expm(op, s, x0)
        check_expm("e^(sM) x, groups", grp.multout(pkg._expm_coefficients(a, b, xn, s)), ref, where)
        check_expm("e^(sM) x, groups", grp.expm_multiply(x0, k, 1.0), ref, where)
    set_operator(grp, 0)
    return infos


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", NAMES)
def test_groups(pkg, name, world):
    with halting(f"groups[{name}-{world}]"):
        group_cells(pkg, group(pkg, world), small(name))


@pytest.mark.parametrize("name", NAMES)
def test_groups_sharded_ingest(pkg, name):
    """the same with the CSR streamed from host memory, at world 5 (above n on seven graphs, above the active vertices on all but
    star65); under A only: lzx.h refuses L there (no rank holds the row pointers the degrees come from)"""
    with halting(f"groups, sharded ingest[{name}]"):
        group_cells(pkg, group(pkg, 5, sharded_ingest=1), small(name), ops=(0,))


@pytest.mark.parametrize("world", WORLDS)
def test_groups_blocked_on_the_star(pkg, world):
    with halting(f"groups, blocked[star65-{world}]"):
        infos = group_cells(pkg, group(pkg, world, propagation_blocking=1, hub_entries=2), small("star65"))
    assert sum(gi["pb_entries"] for gi in infos) > 0 and all(gi["hub_entries"] == 2 for gi in infos), infos


def test_exchange_at_world_1_on_the_path(pkg):
    g = small("path3")
    cells = Cells("path3")
    eng = engine(pkg, g, exchange_at_world_1=1)
    try:
        core_path_cells(pkg, eng, g, cells, batched=False)
    finally:
        eng.close()
    cells.done("exchange at world 1")


def test_ranks_without_rows_and_without_entries_occurred():
    want_empty = {(w, nm) for w in WORLDS for nm in NAMES if w > small(nm).n}
    want_entryless = {(w, nm) for w in WORLDS for nm in NAMES if w > small(nm).n_active}
    assert want_empty and want_empty <= SEEN["empty_rank"], want_empty - SEEN["empty_rank"]
    assert want_entryless and want_entryless <= SEEN["entryless_rank"], want_entryless - SEEN["entryless_rank"]


# ---- the condition on the whole module --------------------------------------------------------------------------------------
def test_every_cell_ran_and_the_refusals_are_the_table():
    for family, (ratio, err, tol, where) in sorted(WORST.items()):
        print(f"largest error, {family}: {err:.3e} (held to {tol:.3e}) at {where}")
    for sec, what in sorted(SLOW, reverse=True)[:3]:
        print(f"slowest: {what} {sec:.2f} s")
    every = {(name, entry) for name in NAMES for entry in ENTRY_POINTS}
    missing = sorted(every - set(CELLS))
    assert not missing, f"{len(missing)} cells did not run or did not pass: {missing[:40]}"
    assert set(CELLS) == every, sorted(set(CELLS) - every)
    assert {cell for cell, kind in CELLS.items() if kind == "refusal"} == set(REFUSAL_CELLS)
    header = " ".join(re.sub(r"\n\s*\*", " ", open(HEADER).read()).split())       # the comment's text without its line starts
    for entry, _, _, sentence in REFUSALS:
        assert " ".join(sentence.split()) in header, f"the row of {entry} quotes a sentence include/lzx.h does not hold"
