"""GPU: many right-hand sides by a batch of independent CG solves that share one SpMM per iteration (include/lzx.h:
lzx_solve_multi_f64, Engine.solve_multi, Engine.effective_resistance) against scipy / numpy on the golden fixtures: sigma I - A
with one shift per column, every width and column position bit for bit, awkward sizes against dense solves, (sigma I + L), L+ B
and effective resistances with deflation, mixed outcomes in one call, the error paths, isolation, and BASELINE C2's Katz columns.
Tolerances are those of tests/test_gpu_solve.py: true residual <= 10 tol, reported resid equal to scipy's to 1e-12, x within
kappa(S) * 10 * tol of a direct solve."""
import ctypes
import glob
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csg
from scipy.sparse.linalg import eigsh, spsolve

from bench import C2_DRAWS
from test_solve_multi_host import batched_cg

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))
LAP = 1
ERR_ARG, ERR_LIMIT = -1, -6


def fixture(name):
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
    return g["ref_row_offset"].astype(np.uint64), g["ref_col_idx"]


def matrices(rp, ci):
    rp64, ci64 = np.asarray(rp).astype(np.int64), np.asarray(ci).astype(np.int64)
    n = len(rp64) - 1
    A = sp.csr_matrix((np.ones(len(ci64)), ci64, rp64), shape=(n, n))
    d = np.diff(rp64).astype(np.float64)
    return A, (sp.diags(d) - A).tocsr()


def engine(pkg, rp, ci, op=0, **shapes):
    eng = pkg.Engine(0, operator=op, **shapes)
    eng.set_graph_csr(rp, ci)
    return eng


def spectrum_ends(A):
    if A.shape[0] <= 4096:
        lam = np.linalg.eigvalsh(A.toarray())
        return lam[0], lam[-1]
    lo = eigsh(A, k=1, which="SA", tol=1e-12, return_eigenvectors=False)[0]
    hi = eigsh(A, k=1, which="LA", tol=1e-12, return_eigenvectors=False)[0]
    return lo, hi


def csr_of_edges(n, edges):
    """symmetric CSR of an edge list ((u, v) with u == v: a self loop, stored once)"""
    M = sp.lil_matrix((n, n))
    for u, v in edges:
        M[u, v] = 1.0
        M[v, u] = 1.0
    M = M.tocsr()
    M.sort_indices()
    return M.indptr.astype(np.uint64), M.indices.astype(np.uint32)


_ER = {}


def er1000():
    """er_n1000 with its dense spectrum, computed once and shared (read-only)"""
    if not _ER:
        rp, ci = fixture("er_n1000")
        A, L = matrices(rp, ci)
        lam = np.linalg.eigvalsh(A.toarray())
        _ER.update(rp=rp, ci=ci, A=A, L=L, lo=lam[0], hi=lam[-1], n=A.shape[0])
    return _ER


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_adjacency_fixtures(pkg, path):
    name = os.path.basename(path)[:-4]
    rp, ci = fixture(name)
    A, _ = matrices(rp, ci)
    n = A.shape[0]
    lo, hi = spectrum_ends(A)
    shifts = np.array([1.02, 1.2, 2.0]) * hi
    tol = 1e-10
    onehot = np.zeros(n)
    onehot[np.argmax(np.diff(rp.astype(np.int64)))] = 1.0
    B = np.stack([np.ones(n), np.random.default_rng(7).standard_normal(n), onehot])
    eng = engine(pkg, rp, ci)
    X, info = eng.solve_multi(B, shifts, tol=tol)
    assert info["converged"] == 3 and list(info["status"]) == [0, 0, 0]
    assert info["launched"] >= info["iterations"] == info["iters"].max() and info["nb"] == 3
    for c, sig in enumerate(shifts):
        b = B[c]
        assert abs(info["bnorm"][c] - np.linalg.norm(b)) <= 1e-12 * np.linalg.norm(b)
        S = (sig * sp.identity(n) - A).tocsc()
        res = np.linalg.norm(b - S @ X[c]) / np.linalg.norm(b)
        assert res <= 10 * tol, (name, c, res)
        assert abs(info["resid"][c] - res) <= 1e-12, (name, c, info["resid"][c], res)
        # (the direct solves are this test's cost: tens of seconds on er_c1_n10000, whose factors fill in; S is symmetric, and
        #  the symmetric minimum-degree ordering leaves a third of COLAMD's fill there)
        ref = spsolve(S, b, permc_spec="MMD_AT_PLUS_A")
        kappa = (sig - lo) / (sig - hi)
        assert np.linalg.norm(X[c] - ref) <= kappa * 10 * tol * np.linalg.norm(ref), (name, c)
    # equal b: the nearer sigma is to lambda_max, the longer
    Xs, infos = eng.solve_multi(np.stack([B[1]] * 3), shifts, tol=tol)
    assert infos["iters"][0] >= infos["iters"][1] >= infos["iters"][2] and list(infos["status"]) == [0, 0, 0]
    assert np.array_equal(Xs[1], X[1])
    eng.close()


def test_widths_positions_repeats_and_poll(pkg):
    g = er1000()
    n, hi = g["n"], g["hi"]
    rng = np.random.default_rng(21)
    B = rng.standard_normal((16, n))
    B[3] = 1.0
    shifts = hi * np.linspace(1.03, 2.5, 16)
    eng = engine(pkg, g["rp"], g["ci"])
    alone = [eng.solve_multi(B[c:c + 1], shifts[c:c + 1]) for c in range(16)]

    def same(X, info, i, c):
        Xa, ia = alone[c]
        return (np.array_equal(X[i], Xa[0]) and info["iters"][i] == ia["iters"][0] and info["resid"][i] == ia["resid"][0]
                and info["bnorm"][i] == ia["bnorm"][0])

    e1 = engine(pkg, g["rp"], g["ci"], solve_poll=1)
    for nb in (1, 2, 3, 5, 9, 16):
        X, info = eng.solve_multi(B[:nb], shifts[:nb])
        assert all(same(X, info, c, c) for c in range(nb)), nb
        perm = rng.permutation(16)[:nb]                           # other columns, other places
        Xp, infop = eng.solve_multi(B[perm], shifts[perm])
        assert all(same(Xp, infop, i, c) for i, c in enumerate(perm)), (nb, perm)
        X2, info2 = eng.solve_multi(B[:nb], shifts[:nb])          # a repeat
        assert np.array_equal(X2, X) and np.array_equal(info2["iters"], info["iters"]) and np.array_equal(info2["resid"], info["resid"])
        X1, info1 = e1.solve_multi(B[:nb], shifts[:nb])           # another status period
        assert np.array_equal(X1, X) and np.array_equal(info1["iters"], info["iters"]) and np.array_equal(info1["resid"], info["resid"])
        assert info1["launched"] == info1["iterations"] <= info["launched"]
    eng.close()
    e1.close()


def path_edges(n):
    return [(i, i + 1) for i in range(n - 1)]


SMALL = [("self_loop", 1, [(0, 0)]), ("edge", 2, [(0, 1)])] + [(f"path{n}", n, path_edges(n)) for n in (31, 33, 2047, 2049, 4097)]


@pytest.mark.parametrize("name,n,edges", SMALL, ids=[s[0] for s in SMALL])
def test_small_and_awkward_sizes(pkg, name, n, edges):
    rp, ci = csr_of_edges(n, edges)
    A, _ = matrices(rp, ci)
    Ad = A.toarray()
    sig = 3.0                                                      # lambda_max <= 2 on a path, 1 on the loop and the edge
    rng = np.random.default_rng(n)
    B = np.stack([np.ones(n), rng.standard_normal(n), np.eye(n)[n // 2]])
    shifts = np.array([sig, sig + 0.5, sig + 2.0])
    tol = 1e-11
    eng = engine(pkg, rp, ci)
    X, info = eng.solve_multi(B, shifts, tol=tol)
    eng.close()
    assert list(info["status"]) == [0, 0, 0]
    lam = np.linalg.eigvalsh(Ad)
    for c in range(3):
        S = shifts[c] * np.eye(n) - Ad
        ref = np.linalg.solve(S, B[c])
        kappa = (shifts[c] - lam[0]) / (shifts[c] - lam[-1])
        assert np.linalg.norm(B[c] - S @ X[c]) <= 10 * tol * np.linalg.norm(B[c]), (name, c)
        assert np.linalg.norm(X[c] - ref) <= kappa * 10 * tol * np.linalg.norm(ref), (name, c)


def test_split_rows(pkg):
    rp, ci = fixture("star_ring_n1500")
    A, L = matrices(rp, ci)
    n = A.shape[0]
    Ad = A.toarray()
    lam = np.linalg.eigvalsh(Ad)
    rng = np.random.default_rng(15)
    B = rng.standard_normal((5, n))
    tol = 1e-11
    shifts = lam[-1] * np.array([1.1, 1.3, 1.6, 2.0, 3.0])
    eng = engine(pkg, rp, ci, multi_row_chunk=8)
    X, info = eng.solve_multi(B, shifts, tol=tol)
    eng.close()
    assert list(info["status"]) == [0] * 5
    for c in range(5):
        S = shifts[c] * np.eye(n) - Ad
        ref = np.linalg.solve(S, B[c])
        kappa = (shifts[c] - lam[0]) / (shifts[c] - lam[-1])
        assert np.linalg.norm(B[c] - S @ X[c]) <= 10 * tol * np.linalg.norm(B[c]), c
        assert np.linalg.norm(X[c] - ref) <= kappa * 10 * tol * np.linalg.norm(ref), c
    Ld = L.toarray()
    eng = engine(pkg, rp, ci, op=LAP, multi_row_chunk=8)
    X, info = eng.solve_multi(B[:3], [0.5, 1.0, 4.0], tol=tol)
    eng.close()
    for c, s in enumerate([0.5, 1.0, 4.0]):
        S = s * np.eye(n) + Ld
        assert np.linalg.norm(B[c] - S @ X[c]) <= 10 * tol * np.linalg.norm(B[c]), c


def test_against_solve_shifted(pkg):
    g = er1000()
    n, lo, hi = g["n"], g["lo"], g["hi"]
    rng = np.random.default_rng(31)
    B = rng.standard_normal((4, n))
    shifts = hi * np.array([1.05, 1.3, 1.7, 2.2])
    tol = 1e-10
    eng = engine(pkg, g["rp"], g["ci"])
    X, _ = eng.solve_multi(B, shifts, tol=tol)
    for c in range(4):
        x, _ = eng.solve_shifted(B[c], shifts[c], tol=tol)
        kappa = (shifts[c] - lo) / (shifts[c] - hi)
        assert np.linalg.norm(X[c] - x) <= 10 * kappa * tol * np.linalg.norm(x), c
    eng.close()


@pytest.mark.parametrize("name", ["er_n1000", "rmat_n3000_skew"])
def test_regularised_laplacian(pkg, name):
    rp, ci = fixture(name)
    _, L = matrices(rp, ci)
    n = L.shape[0]
    b = np.random.default_rng(3).standard_normal(n)
    ts = np.array([0.1, 1.0, 10.0])
    eng = engine(pkg, rp, ci, op=LAP)
    X, info = eng.solve_multi(np.stack([b] * 3), 1.0 / ts, tol=1e-11)
    eng.close()
    Ld = L.toarray()
    lmax = np.linalg.eigvalsh(Ld)[-1]
    assert list(info["status"]) == [0, 0, 0]
    for i, t in enumerate(ts):
        S = np.eye(n) / t + Ld
        ref = np.linalg.solve(S, b)
        kappa = (1 / t + lmax) * t
        assert np.linalg.norm(X[i] - ref) <= kappa * 10 * 1e-11 * np.linalg.norm(ref), (name, t)
        assert info["resid"][i] <= 1e-10 and np.linalg.norm(b - S @ X[i]) / np.linalg.norm(b) <= 1e-10


_GIANT = {}


def giant():
    """the giant component of rmat_n4096 with its dense pseudo-inverse, computed once and shared (read-only)"""
    if not _GIANT:
        rp, ci = fixture("rmat_n4096")
        A, L = matrices(rp, ci)
        ncomp, lab = csg.connected_components(A, directed=False)
        keep = np.nonzero(lab == np.bincount(lab).argmax())[0]
        _GIANT.update(rp=rp, ci=ci, keep=keep, P=np.linalg.pinv(L[keep][:, keep].toarray()), L=L[keep][:, keep])
    return _GIANT


def test_pseudo_inverse_on_the_giant_component(pkg):
    g = giant()
    full = engine(pkg, g["rp"], g["ci"], op=LAP)
    sub, old = full.largest_component(operator=LAP)
    full.close()
    assert np.array_equal(old, g["keep"])
    n = sub.n
    B = np.random.default_rng(4).standard_normal((4, n))
    X, info = sub.solve_multi(B, 0.0, tol=1e-11, maxiter=5000, W=np.full(n, 1.0 / np.sqrt(n)))
    sub.close()
    assert list(info["status"]) == [0] * 4
    ref = (g["P"] @ B.T).T
    for c in range(4):
        assert abs(X[c].sum()) <= 1e-10 * np.linalg.norm(X[c]) * np.sqrt(n)
        assert np.linalg.norm(X[c] - ref[c]) <= 1e-8 * np.linalg.norm(ref[c]), c
        assert abs(info["bnorm"][c] - np.linalg.norm(B[c] - B[c].mean())) <= 1e-12 * np.linalg.norm(B[c])


def test_effective_resistance(pkg):
    g = giant()
    full = engine(pkg, g["rp"], g["ci"], op=LAP)
    sub, _ = full.largest_component(operator=LAP)
    full.close()
    n, P = sub.n, g["P"]
    pairs = np.random.default_rng(11).integers(0, n, size=(20, 2))
    pairs[5] = (7, 7)                                             # a degenerate pair: 0, no solve
    R = sub.effective_resistance(pairs, tol=1e-11, maxiter=5000)   # 19 right-hand sides: two batches
    sub.close()
    ref = np.array([P[u, u] + P[v, v] - 2 * P[u, v] for u, v in pairs])
    assert R.shape == (20,) and R[5] == 0.0
    assert np.abs(R - ref).max() <= 1e-8, np.abs(R - ref).max()
    adj = engine(pkg, g["rp"], g["ci"])
    with pytest.raises(ValueError, match="Laplacian"):
        adj.effective_resistance([(0, 1)])
    adj.close()


def test_mixed_outcomes_in_one_call(pkg):
    g = er1000()
    n, hi, A = g["n"], g["hi"], g["A"]
    rng = np.random.default_rng(41)
    B = rng.standard_normal((3, n))
    shifts = hi * np.array([1.3, 0.5, 2.0])
    eng = engine(pkg, g["rp"], g["ci"])
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*column 1 is not positive definite.*iteration") as ei:
        eng.solve_multi(B, shifts)
    X, info = ei.value.partial
    assert list(info["status"]) == [0, 2, 0] and info["converged"] == 2
    # (the restatement sums in another order: a residual within rounding of tol ||b|| may freeze one iteration apart)
    _, it_ref, st_ref, _ = batched_cg(A, B, shifts, 1e-10, 1000)
    assert list(st_ref) == [0, 2, 0] and all(abs(int(info["iters"][c]) - int(it_ref[c])) <= 1 for c in (0, 2))
    Xn, infon = eng.solve_multi(B[[0, 2]], shifts[[0, 2]])        # the same handle, without the bad column
    assert np.array_equal(Xn, X[[0, 2]]) and np.array_equal(infon["iters"], info["iters"][[0, 2]])
    assert np.array_equal(infon["resid"], info["resid"][[0, 2]]) and list(infon["status"]) == [0, 0]
    # maxiter = 3: every column's third iterate, as the numpy restatement forms it
    ok = hi * np.array([1.02, 1.1, 1.5])
    with pytest.raises(pkg.LzxError, match=r"\(-6\).*0 of 3 columns converged") as ei:
        eng.solve_multi(B, ok, maxiter=3)
    X3, info3 = ei.value.partial
    assert list(info3["iters"]) == [3, 3, 3] and list(info3["status"]) == [1, 1, 1] and info3["launched"] == 3
    ref, _, _, _ = batched_cg(A, B, ok, 1e-10, 3)
    for c in range(3):
        assert np.abs(X3[c] - ref[c]).max() <= 1e-12 * np.abs(ref[c]).max(), c
    eng.close()


def test_error_paths(pkg):
    g = er1000()
    n, hi = g["n"], g["hi"]
    ones = np.ones(n)
    B = np.stack([ones, np.arange(n, dtype=np.float64)])
    eng = engine(pkg, g["rp"], g["ci"])
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*column 1 of b is zero"):
        eng.solve_multi(np.stack([ones, np.zeros(n)]), 2 * hi)
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*column 0 of b lies in the span of W"):
        eng.solve_multi(B, 2 * hi, W=ones)
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*rank-deficient"):
        eng.solve_multi(B, 2 * hi, W=np.stack([ones, 2.0 * ones]))
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*<= 0 under A"):
        eng.solve_multi(B, [2 * hi, 0.0])
    with pytest.raises(pkg.LzxError, match=r"\(-6\).*nb = 17"):
        eng.solve_multi(np.ones((17, n)), 2 * hi)
    with pytest.raises(pkg.LzxError, match=r"\(-6\).*nw = 9"):
        eng.solve_multi(B, 2 * hi, W=np.eye(9, n))
    X, info = eng.solve_multi(B, 2 * hi)                            # and the handle still works
    assert info["converged"] == 2
    eng.close()
    lap = engine(pkg, g["rp"], g["ci"], op=LAP)
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*deflation"):
        lap.solve_multi(B, [1.0, 0.0])                            # sigma = 0 under L needs W
    lap.close()
    empty = pkg.Engine(0)                                        # no graph: the C entry point on the bare handle
    f64p = ctypes.POINTER(ctypes.c_double)
    sh2, Xo = np.full(2, 2 * hi), np.zeros((2, n))
    rc = pkg.lib().lzx_solve_multi_f64(empty.h, 2, B.ctypes.data_as(f64p), sh2.ctypes.data_as(f64p), 1e-10, 100, None, 0,
                                       Xo.ctypes.data_as(f64p), None, None, None, None)
    msg = pkg.lib().lzx_last_error().decode()
    assert rc == -3 and "lzx_solve_multi_f64" in msg and "no graph" in msg, (rc, msg)
    empty.close()
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(g["rp"], g["ci"])
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*one GPU"):
        grp.engines[0].solve_multi(B, 2 * hi)
    grp.close()
    # 4 columns pad to B = 4: 5 * 4 * n * 8 bytes and the partials; a single column pads to B = 2
    small = engine(pkg, g["rp"], g["ci"], solve_state_bytes=12 * n * 8)
    with pytest.raises(pkg.LzxError, match=r"\(-4\).*bytes"):
        small.solve_multi(np.ones((4, n)) + np.arange(4)[:, None], 2 * hi)
    X, info = small.solve_multi(B[:1], 2 * hi)
    assert info["converged"] == 1
    small.close()


def test_isolation(pkg):
    g = er1000()
    n, hi = g["n"], g["hi"]
    eng = engine(pkg, g["rp"], g["ci"])
    k = 20
    X0 = np.stack([np.ones(n), np.arange(n, dtype=np.float64) + 1.0, np.cos(np.arange(n))])
    eng.lanczos_multi(X0, k)                                       # width 4
    T = np.random.default_rng(1).standard_normal((3, k))
    y_multi = eng.multout_multi(T)
    eng.lanczos(np.ones(n), k, want_q=False)
    t = np.random.default_rng(2).standard_normal(k)
    y_single = eng.multout(t)
    B = np.random.default_rng(3).standard_normal((9, n))
    eng.solve_multi(B, 1.5 * hi)                                   # width 16
    assert np.array_equal(eng.multout_multi(T), y_multi) and np.array_equal(eng.multout(t), y_single)
    eng.solve_multi(B[:3], 1.5 * hi)                               # the basis' own width
    assert np.array_equal(eng.multout_multi(T), y_multi)
    # a probe basis answers probe_diag as before
    al, be, ku, _ = eng.lanczos_probes(5, 0, 6, k, keep_basis=True)
    Tp = np.random.default_rng(4).standard_normal((6, k))
    d0 = eng.probe_diag(Tp)
    eng.solve_multi(B[:2], 1.5 * hi)
    assert np.array_equal(eng.probe_diag(Tp), d0)
    # a chunked single-vector decomposition continues across the call bit for bit
    ref = engine(pkg, g["rp"], g["ci"])
    ref.lanczos_prepare(np.ones(n), k)
    ref.lanczos_run_steps(k)
    a_ref, b_ref, _ = ref.lanczos_fetch(k)
    ref.close()
    eng.lanczos_prepare(np.ones(n), k)
    eng.lanczos_run_steps(7)
    eng.solve_multi(B[:5], 1.5 * hi)
    eng.lanczos_run_steps(k - 7)
    a, b, _ = eng.lanczos_fetch(k)
    assert np.array_equal(a, a_ref) and np.array_equal(b, b_ref)
    eng.close()


def test_c2_katz_columns(pkg):
    eng = pkg.Engine(0)
    eng.gen_rmat(20, 1 << 20, C2_DRAWS, 1234)          # BASELINE C2, generated on the device
    rp, ci = eng.get_graph_csr()
    lam = float(eng.eigsh(nev=1, which="LA", want_vectors=False)[0][0])
    n = len(rp) - 1
    sig = lam / 0.85
    seeds = np.argsort(np.diff(rp.astype(np.int64)))[-8:]
    B = np.zeros((8, n))
    B[np.arange(8), seeds] = 1.0
    X, info = eng.solve_multi(B, sig, tol=1e-10)
    eng.close()
    A, _ = matrices(rp, ci)
    assert list(info["status"]) == [0] * 8
    R = B - (sig * X - (A @ X.T).T)
    for c in range(8):
        res = np.linalg.norm(R[c])                      # ||b_c|| = 1
        assert res <= 1e-9, (c, res)
        assert abs(info["resid"][c] - res) <= 1e-12
