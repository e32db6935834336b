"""GPU: the batched SpMM and its reductions -- csrc/lzx_multi_shared.h (k_multi_pack / k_multi_unpack, k_multi_spmm, k_multi_alpha,
seg_partials, close_cols), lzx_multi_build_tables, k_multi_update / k_multi_scale -- at the boundaries of their tables: the 32-row
run, the 2048-row segment, the chunk L of a split row and the eight-entry unroll, against the host model tests/multi_model.py.  The
graphs (a ring with planted hub rows) and what each is there for are in tests/test_multi_model_host.py.

Held bit for bit, because integer-valued inputs make every sum exact in any order:
  * Y = A X and Y = L X on integers of |x| <= 2^19 and on the indicators of the boundary columns, for every graph, L in {16,
    default} and b in {1, 2, 3, 4, 5, 8, 9, 16}, each checked call behind a call of a wider batch and one of the same width on
    other values (a row of length 0, a padded column or a padded list entry that keeps an old value shows up);
  * on a random real X the unsplit rows (the left-to-right sum in CSR order); split rows within u (len + chunks) sum |x_j|;
  * the six read-only shape names against the model's counts;
  * alpha_0 = x'Mx / 4^m of lanczos_multi from multi_model.exact_start vectors, for b in {1, 3, 16} and both operators, and
    beta_0 = sqrt(sum u_int^2) / 2^(3m) wherever sum u_int^2 < 2^53 (asserted from Python integers first: every graph of
    n <= 4129; under L all but `default4129`); a column alone and inside a batch of 16; the probe runs with and without a kept basis.
    n = 2 has no exact start (no a + 4 b + 9 c = 4^m with a + b + c = 2), so these checks run on every size but 2.
Held to a derived bound: beta_0 where sum u_int^2 passes 2^53 (`default4129` under L and the two graphs of many row segments): within
(D + 2) 2^-53 of the value from Python integers, D = 31 + 6 + (ceil(n_seg / 256) - 1) + 6 + 3 the longest chain of additions a
term passes through (the run, the wavefront tree, a thread's entries of close_cols, its wavefront tree, its four waves).  The
squares carry one rounding each and the square root halves the relative error of its argument, so the bound has room.
The later coefficients go through check_leading_coefficients against the oracle, BFS / betweenness and solve_multi through the
references and tolerances of their own suites.  The last test fails unless every line of the coverage table was reached.
"""
import math
from fractions import Fraction

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp
from scipy.sparse.linalg import eigsh

import multi_model as mm
from test_gpu_parity import check_leading_coefficients
from test_gpu_paths import check_against
from test_multi_model_host import (GRAPHS, L_SMALL, N_CLOSE, NAMES, TABLE, big_graph, big_model, boundary, exact_ref, graph, lap, model,
                                   n_stride, reached, starts, x_int)
from test_paths_host import brandes_batched

pytestmark = pytest.mark.gpu

LAP = 1
WIDTHS = (1, 2, 3, 4, 5, 8, 9, 16)
LS = (L_SMALL, mm.CHUNK)
SHAPE_NAMES = ("multi_chunk", "multi_work_items", "multi_split_rows", "multi_chunk_slots", "multi_row_segments", "multi_vector_grid")
U = 2.0 ** -53
SEEN = {}             # (graph, L) -> (model, shapes read from the handle): what the coverage test works from


def engine(pkg, rp, ci, L):
    eng = pkg.Engine(0, **({} if L == mm.CHUNK else dict(multi_row_chunk=L)))
    eng.set_graph_csr(rp, ci)
    return eng


def read_shapes(eng):
    return {k: eng.shape(k) for k in SHAPE_NAMES}


def tables_are_the_models(eng, m, key):
    """check (b), behind the handle's first batched call"""
    got = read_shapes(eng)
    assert got == mm.shapes(m), (key, got, mm.shapes(m))
    assert got["multi_vector_grid"] <= max(got["multi_row_segments"], 1)
    SEEN[key] = (m, got)


def spmm_behind_other_calls(eng, X, salt):
    """the checked call, behind a wider call and one of the same width on other values"""
    b, n = X.shape
    eng.spmm(x_int(n, 16, salt=salt + 1))
    eng.spmm(x_int(n, b, salt=salt + 2))
    return eng.spmm(X)


# ---- (a) and (b) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LS, ids=["L16", "Ldefault"])
@pytest.mark.parametrize("name", NAMES)
def test_spmm_bit_for_bit(pkg, oracle, name, L):
    A, rp, ci = graph(name)
    n = A.shape[0]
    m = model(name, L)
    eng = engine(pkg, rp, ci, L)
    try:
        assert not any(read_shapes(eng).values())                    # no tables before the first batched call
        eng.spmm(np.ones((1, n)))
        tables_are_the_models(eng, m, (name, L))
        E = np.zeros((len(boundary(name)), n))
        E[np.arange(len(E)), boundary(name)] = 1.0
        for op in (0, LAP):
            eng.set_option("operator", op)
            for b in WIDTHS:
                X = x_int(n, b)
                Y = spmm_behind_other_calls(eng, X, salt=b)
                assert np.array_equal(Y, exact_ref(A, X, op == LAP)), (name, L, op, b)
            for first in range(0, len(E), 16):
                Y = spmm_behind_other_calls(eng, E[first:first + 16], salt=first)
                assert np.array_equal(Y, exact_ref(A, E[first:first + 16], op == LAP)), (name, L, op, first)
        eng.set_option("operator", 0)
        # a random real X: unsplit rows are the oracle's left-to-right sums, split rows within the bound of any order
        X = np.random.default_rng(11).standard_normal((3, n))
        Y = spmm_behind_other_calls(eng, X, salt=40)
        unsplit = m.deg <= L
        nch = -(-m.deg // L)
        for c in range(3):
            ref = oracle.spmv(rp, ci, X[c])
            assert np.array_equal(Y[c][unsplit], ref[unsplit]), (name, L, c)
            bound = U * (m.deg + nch) * oracle.spmv(rp, ci, np.abs(X[c]))
            assert (np.abs(Y[c] - ref)[~unsplit] <= bound[~unsplit]).all(), (name, L, c)
    finally:
        eng.close()


# ---- (c) ----------------------------------------------------------------------------------------------------------------
def beta_bound(n_seg):
    """(D + 2) 2^-53: the module docstring"""
    return (31 + 6 + (-(-n_seg // 256) - 1) + 6 + 3 + 2) * U


def beta_within(beta, S, m, rel):
    """|beta - sqrt(S) / 2^(3m)| <= rel sqrt(S) / 2^(3m), in integers: sqrt(S) to 100 more bits than S has"""
    root = math.isqrt(S << 200)                                       # sqrt(S) 2^100, rounded down
    dev = Fraction(float(beta)) * 2 ** (3 * m) * 2 ** 100
    return abs(dev - root) <= Fraction(rel) * root + 1


def lap_callback(O, A):
    n = A.shape[0]
    d = np.diff(A.indptr).astype(np.float64)
    Af = A.astype(np.float64)

    def cb(_user, pin, pout):
        x = np.ctypeslib.as_array(pin, shape=(n,))
        np.ctypeslib.as_array(pout, shape=(n,))[:] = d * x - Af @ x
    return O.SPMV_FN(cb)


def check_first_coefficients(a, be, xn, X, m, rp, ci, lapl, n_seg, key, exact_beta=None):
    """alpha_0 and beta_0 of every column against Python integers; returns the exact beta_0 values (None where only bounded)"""
    out = []
    for c, x in enumerate(X):
        p, S, fits = mm.first_coefficients(rp, ci, x, m, lapl)
        assert abs(p) < 2 ** 53 and xn[c] == 2.0 ** m, (key, c)
        print(key, "column", c, "alpha_0", a[c, 0], "exact", p / 4 ** m, "beta_0", be[c, 0], "sum u_int^2", S, "fits", fits)
        assert a[c, 0] == p / 4 ** m, (key, c, a[c, 0], p / 4 ** m)
        if exact_beta is not None:
            assert fits == exact_beta, (key, c, S)
        if fits:
            assert be[c, 0] == mm.beta_exact(S, m), (key, c, be[c, 0], mm.beta_exact(S, m))
            out.append(mm.beta_exact(S, m))
        else:
            assert beta_within(be[c, 0], S, m, beta_bound(n_seg)), (key, c, be[c, 0], math.sqrt(S) / 2.0 ** (3 * m))
            out.append(None)
    return out


LANCZOS_CELLS = [(name, L_SMALL) for name in NAMES if GRAPHS[name][0] != 2] + [("default4129", mm.CHUNK)]


@pytest.mark.parametrize("name,L", LANCZOS_CELLS, ids=[f"{n}-L{L}" for n, L in LANCZOS_CELLS])
def test_first_coefficients_bit_for_bit(pkg, oracle, name, L):
    O = oracle
    A, rp, ci = graph(name)
    n = A.shape[0]
    X16, m = starts(name, seeds=range(16))
    eng = engine(pkg, rp, ci, L)
    k = 3
    try:
        for op in (0, LAP):
            eng.set_option("operator", op)
            runs, betas = {}, {}
            for b in (16, 3, 1):
                a, be, ku, xn, _, _ = eng.lanczos_multi(X16[:b], k)
                runs[b] = (a, be, ku)
                betas[b] = check_first_coefficients(a, be, xn, X16[:b], m, rp, ci, op == LAP, model(name, L).n_seg, (name, L, op, b),
                                                 exact_beta=not (name == "default4129" and op == LAP))
            # the module's promise: a column's coefficients do not depend on the batch around it
            for b in (3, 1):
                assert np.array_equal(runs[b][0], runs[16][0][:b]) and np.array_equal(runs[b][1], runs[16][1][:b]), (name, L, op, b)
                assert np.array_equal(runs[b][2], runs[16][2][:b])
            # the later coefficients against the oracle (a column that broke down at beta_0 has none: zeros)
            a, be, ku = runs[3]
            cb = lap_callback(O, A) if op == LAP else None
            for c in range(3):
                if be[c, 0] == 0.0:
                    assert betas[3][c] == 0.0 and ku[c] == 1 and not a[c, 1:].any() and not be[c].any(), (name, L, op, c)
                    continue
                a_ref, b_ref, _, xn_ref = O.lanczos(rp, ci, k, X16[c], ext_spmv=cb)
                assert xn_ref == 2.0 ** m
                check_leading_coefficients(a[c], be[c, :k - 1], a_ref, b_ref, (name, L, op, c))
        if (name, L) not in SEEN:
            tables_are_the_models(eng, model(name, L), (name, L))
    finally:
        eng.close()


@pytest.mark.parametrize("L", LS, ids=["L16", "Ldefault"])
def test_probe_runs_bit_for_bit(pkg, L):
    """n = 4096 = 4^6: q_0 = z / 64 is exact, so alpha_0 = z'Mz / 4096 for the z that probes() returns"""
    name, m = "n4096", 6
    A, rp, ci = graph(name)
    eng = engine(pkg, rp, ci, L)
    try:
        for op in (0, LAP):
            eng.set_option("operator", op)
            for b in (1, 3, 16):
                Z = eng.probes(5, 2, b)
                assert np.array_equal(np.abs(Z), np.ones_like(Z))
                a, be, ku, _ = eng.lanczos_probes(5, 2, b, 3)
                a2, be2, ku2, _ = eng.lanczos_probes(5, 2, b, 3, keep_basis=True)
                assert np.array_equal(a, a2) and np.array_equal(be, be2) and np.array_equal(ku, ku2), (L, op, b)
                check_first_coefficients(a, be, np.full(b, 64.0), Z, m, rp, ci, op == LAP, 2, ("probes", L, op, b), exact_beta=True)
    finally:
        eng.close()


# ---- (d) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["close_cols", "grid_stride"])
def test_many_segments(pkg, which):
    """b = 1 on one handle: n_seg > 256 (close_cols takes a second entry per thread), and n_seg > the vector kernels' grid (their
    grid-stride loops take a second row segment -- the grid is 4 x the compute units, 1024 on the MI355X, and the handle is asked)"""
    n = N_CLOSE if which == "close_cols" else n_stride(4 * mm.CU_COUNT)
    A, rp, ci = big_graph(n)
    m = big_model(n)
    eng = engine(pkg, rp, ci, mm.CHUNK)
    try:
        X = x_int(n, 1)
        for op in (0, LAP):
            eng.set_option("operator", op)
            Y = spmm_behind_other_calls(eng, X, salt=3)
            assert np.array_equal(Y, exact_ref(A, X, op == LAP)), (which, op)
        tables_are_the_models(eng, m, (which, mm.CHUNK))
        got = SEEN[(which, mm.CHUNK)][1]
        print(which, "multi_row_segments", got["multi_row_segments"], "multi_vector_grid", got["multi_vector_grid"])
        if which == "close_cols":
            assert got["multi_row_segments"] > 256
        else:
            assert got["multi_row_segments"] > got["multi_vector_grid"]
        x, mexp = mm.exact_start(n, np.random.default_rng(1000))
        for op in (0, LAP):
            eng.set_option("operator", op)
            a, be, ku, xn, _, _ = eng.lanczos_multi(x[None, :], 2)
            check_first_coefficients(a, be, xn, x[None, :], mexp, rp, ci, op == LAP, got["multi_row_segments"], (which, op), exact_beta=False)
    finally:
        eng.close()


# ---- (e) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_bfs_and_betweenness_on_the_list(pkg, name):
    A, rp, ci = graph(name)
    Af = A.astype(np.float64)
    src = boundary(name)
    ref = brandes_batched(Af, src)
    assert ref["paths"].max() < 2.0 ** 53                             # integers: the equality below is exact arithmetic
    eng = engine(pkg, rp, ci, L_SMALL)
    try:
        check_against(eng, Af, src, ref)
        if (name, L_SMALL) not in SEEN:
            tables_are_the_models(eng, model(name, L_SMALL), (name, L_SMALL))
    finally:
        eng.close()


def spectrum_ends(Af):
    n = Af.shape[0]
    if n <= 600:
        lam = np.linalg.eigvalsh(Af.toarray())
        return lam[0], lam[-1]
    lo = eigsh(Af, k=1, which="SA", tol=1e-12, return_eigenvectors=False)[0]
    hi = eigsh(Af, k=1, which="LA", tol=1e-12, return_eigenvectors=False)[0]
    return lo, hi


def dense_solve(sigma, dense, rhs):
    """(sigma I - A)^(-1) rhs by LAPACK's Cholesky solver.  Where n is a multiple of 64 the matrix is extended by one row and column
    of the identity (the same system: the extra unknown is 0): rows a power of two apart make the factorisation several times
    slower."""
    n = len(dense)
    p = n + (n % 64 == 0)
    S = np.zeros((p, p))
    S[:n, :n] = -dense
    S[np.arange(p), np.arange(p)] += sigma
    S[n:, n:] = 1.0
    R = np.zeros((p, rhs.shape[1]))
    R[:n] = rhs
    return scipy.linalg.solve(S, R, assume_a="pos")[:n]


@pytest.mark.parametrize("name", NAMES)
def test_solve_multi_on_the_list(pkg, name):
    """five shifts above lambda_max, right-hand sides the indicators of the boundary rows, against a dense solve at the tolerances
    of tests/test_gpu_solve_multi.py"""
    A, rp, ci = graph(name)
    Af = A.astype(np.float64)
    n = A.shape[0]
    lo, hi = spectrum_ends(Af)
    shifts = np.array([1.05, 1.2, 1.5, 2.0, 4.0]) * max(hi, 1.0)
    rows = boundary(name)
    B = np.zeros((len(rows), n))
    B[np.arange(len(rows)), rows] = 1.0
    sig = shifts[np.arange(len(rows)) % 5]
    tol = 1e-10
    dense = Af.toarray()
    ref = np.empty_like(B)
    for s in shifts:
        sel = np.flatnonzero(sig == s)
        if len(sel):
            ref[sel] = dense_solve(s, dense, B[sel].T).T
    eng = engine(pkg, rp, ci, L_SMALL)
    try:
        for first in range(0, len(rows), 16):
            sl = slice(first, first + 16)
            X, info = eng.solve_multi(B[sl], sig[sl], tol=tol)
            assert not info["status"].any(), (name, info["status"])
            for c in range(len(X)):
                g = first + c
                S = sig[g] * sp.identity(n) - Af
                assert np.linalg.norm(B[g] - S @ X[c]) <= 10 * tol, (name, g)
                kappa = (sig[g] - lo) / (sig[g] - hi)
                assert np.linalg.norm(X[c] - ref[g]) <= kappa * 10 * tol * np.linalg.norm(ref[g]), (name, g)
    finally:
        eng.close()


# ---- the coverage table ---------------------------------------------------------------------------------------------------
def test_every_line_of_the_coverage_table_was_reached():
    """works from the models whose counts the handles confirmed (SEEN) and, for the lines on row segments, from the numbers the
    handles reported; fails when a cell did not run"""
    want = {(name, L) for name in NAMES for L in LS} | {("close_cols", mm.CHUNK), ("grid_stride", mm.CHUNK)}
    assert want <= set(SEEN), want - set(SEEN)
    got = set()
    for (name, L), (m, shapes) in SEEN.items():
        lines = reached(m)
        if L != L_SMALL:
            lines = {g for g in lines if not g.startswith("unsplit")}
        lines = {g for g in lines if not g.startswith("n_seg")}
        seg, grid = shapes["multi_row_segments"], shapes["multi_vector_grid"]
        if seg in (1, 2, 3):
            lines.add(f"n_seg = {seg}")
        if seg > 256:
            lines.add("n_seg > 256")
        if seg > grid:
            lines.add("n_seg > grid")
        got |= lines
    assert not [line for line in TABLE if line not in got]
