"""GPU: shifted linear systems by multi-shift CG (include/lzx.h: lzx_solve_shifted_f64, Engine.solve_shifted, Engine.katz) against
scipy / numpy on the golden fixtures: sigma I - A near and far from lambda_max, Katz centrality against networkx, (sigma I + L)
for a grid of t, L+ b and effective resistances with deflation, BASELINE C2's Katz vectors, and the error paths, determinism
and isolation."""
import glob
import os

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csg
from scipy.sparse.linalg import eigsh, spsolve

from bench import C2_DRAWS
from test_solve_host import multishift_cg

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))
LAP = 1


def fixture(name):
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
    return g["ref_row_offset"].astype(np.uint64), g["ref_col_idx"]


def matrices(rp, ci):
    rp64, ci64 = rp.astype(np.int64), ci.astype(np.int64)
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


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_adjacency_fixtures(pkg, path):
    name = os.path.basename(path)[:-4]
    rp, ci = fixture(name)
    A, _ = matrices(rp, ci)
    n = A.shape[0]
    lo, hi = spectrum_ends(A)
    shifts = np.array([1.02, 1.2, 2.0]) * hi
    tol = 1e-10
    eng = engine(pkg, rp, ci)
    for b in (np.ones(n), np.random.default_rng(7).standard_normal(n)):
        X, info = eng.solve_shifted(b, shifts, tol=tol)
        assert info["converged"] == 3 and info["launched"] >= info["iterations"] == info["iters"].max()
        assert abs(info["bnorm"] - np.linalg.norm(b)) <= 1e-12 * np.linalg.norm(b)
        for s, sig in enumerate(shifts):
            S = (sig * sp.identity(n) - A).tocsc()
            res = np.linalg.norm(b - S @ X[s]) / np.linalg.norm(b)
            assert res <= 10 * tol, (name, sig, res)
            assert abs(info["resid"][s] - res) <= 1e-12, (name, sig, info["resid"][s], res)
            ref = spsolve(S, b)
            kappa = (sig - lo) / (sig - hi)
            assert np.linalg.norm(X[s] - ref) <= kappa * 10 * tol * np.linalg.norm(ref), (name, sig)
        assert info["iters"][0] >= info["iters"][1] >= info["iters"][2]   # the nearer lambda_max, the longer
    eng.close()


def nx_katz(A, alpha):
    G = nx.from_scipy_sparse_array(A)
    k = nx.katz_centrality_numpy(G, alpha=alpha, beta=1.0, normalized=True)
    return np.array([k[i] for i in range(A.shape[0])])


@pytest.mark.parametrize("name", ["er_n1000", "rmat_n3000_skew"])
def test_katz_against_networkx(pkg, name):
    rp, ci = fixture(name)
    A, _ = matrices(rp, ci)
    lam = np.linalg.eigvalsh(A.toarray())[-1]
    eng = engine(pkg, rp, ci)
    # (tolerances below the default 1e-10: the error bound is kappa(S) * tol, kappa = 12 at alpha = 0.85 / lambda_max)
    x = eng.katz(tol=1e-11)                          # alpha = 0.85 / lambda_max, lambda_max from eigsh on the device
    assert x.shape == (A.shape[0],)
    assert np.abs(x - nx_katz(A, 0.85 / lam)).max() <= 1e-9, name
    alphas = np.array([0.3, 0.6, 0.9]) / lam
    Xm = eng.katz(list(alphas), tol=1e-12)
    assert Xm.shape == (3, A.shape[0])
    for i, a in enumerate(alphas):
        assert np.abs(Xm[i] - eng.katz(a, tol=1e-12)).max() <= 1e-10, (name, i)
    assert np.abs(Xm[2] - nx_katz(A, alphas[2])).max() <= 1e-9
    eng.close()
    eng = engine(pkg, rp, ci, op=LAP)
    with pytest.raises(ValueError, match="adjacency"):
        eng.katz(0.1)
    eng.close()


@pytest.mark.parametrize("name", ["er_n1000", "rmat_n3000_skew"])
def test_regularised_laplacian(pkg, name):
    rp, ci = fixture(name)
    _, L = matrices(rp, ci)
    n = L.shape[0]
    b = np.random.default_rng(3).standard_normal(n)
    ts = np.array([0.1, 1.0, 10.0])
    eng = engine(pkg, rp, ci, op=LAP)
    X, info = eng.solve_shifted(b, 1.0 / ts, tol=1e-11)
    eng.close()
    Ld = L.toarray()
    lmax = np.linalg.eigvalsh(Ld)[-1]
    for i, t in enumerate(ts):
        S = np.eye(n) / t + Ld
        ref = np.linalg.solve(S, b)
        kappa = (1 / t + lmax) * t
        assert np.linalg.norm(X[i] - ref) <= kappa * 10 * 1e-11 * np.linalg.norm(ref), (name, t)
        assert info["resid"][i] <= 1e-10 and np.linalg.norm(b - S @ X[i]) / np.linalg.norm(b) <= 1e-10


def test_pseudo_inverse_connected(pkg):
    rp, ci = fixture("er_n1000")
    A, L = matrices(rp, ci)
    n = A.shape[0]
    assert csg.connected_components(A, directed=False)[0] == 1
    b = np.random.default_rng(4).standard_normal(n)
    eng = engine(pkg, rp, ci, op=LAP)
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*deflation"):
        eng.solve_shifted(b, 0.0)                   # sigma = 0 under L needs W
    x, info = eng.solve_shifted(b, 0.0, tol=1e-11, W=np.full(n, 1.0 / np.sqrt(n)))
    eng.close()
    ref = np.linalg.pinv(L.toarray()) @ b
    assert abs(x.sum()) <= 1e-10 * np.linalg.norm(x) * np.sqrt(n)
    assert np.linalg.norm(x - ref) <= 1e-8 * np.linalg.norm(ref)
    assert abs(info["bnorm"] - np.linalg.norm(b - b.mean())) <= 1e-12 * np.linalg.norm(b)


def test_effective_resistance_giant_component(pkg):
    rp, ci = fixture("rmat_n4096")
    A, L = matrices(rp, ci)
    n = A.shape[0]
    ncomp, lab = csg.connected_components(A, directed=False)
    assert ncomp == 1204
    giant = np.nonzero(lab == np.bincount(lab).argmax())[0]
    w = np.zeros(n)
    w[giant] = 1.0 / np.sqrt(len(giant))
    Lg = L[giant][:, giant].toarray()
    P = np.linalg.pinv(Lg)
    pos = {v: i for i, v in enumerate(giant)}
    rng = np.random.default_rng(11)
    pairs = [tuple(rng.choice(giant, 2, replace=False)) for _ in range(5)]
    eng = engine(pkg, rp, ci, op=LAP)
    for u, v in pairs:
        b = np.zeros(n)
        b[u], b[v] = 1.0, -1.0
        x, info = eng.solve_shifted(b, 0.0, tol=1e-12, W=w, maxiter=5000)
        R = x[u] - x[v]
        iu, iv = pos[u], pos[v]
        R_ref = P[iu, iu] + P[iv, iv] - 2 * P[iu, iv]
        assert abs(R - R_ref) <= 1e-9 * R_ref, (u, v, R, R_ref)
        assert np.abs(x[lab != lab[giant[0]]]).max() == 0.0      # nothing leaks into the other components
    eng.close()


def test_not_positive_definite_then_valid(pkg):
    rp, ci = fixture("er_n1000")
    A, _ = matrices(rp, ci)
    lam, U = np.linalg.eigh(A.toarray())
    eng = engine(pkg, rp, ci)
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*not positive definite.*iteration 0"):
        eng.solve_shifted(U[:, -1], 0.5 * lam[-1])
    x, info = eng.solve_shifted(np.ones(A.shape[0]), 1.5 * lam[-1])
    assert info["converged"] == 1 and info["resid"][0] <= 1e-9
    eng.close()


def test_maxiter_gives_partial_result(pkg):
    rp, ci = fixture("er_n1000")
    A, _ = matrices(rp, ci)
    lam = np.linalg.eigvalsh(A.toarray())[-1]
    eng = engine(pkg, rp, ci)
    shifts = [1.02 * lam, 1.1 * lam]
    with pytest.raises(pkg.LzxError, match=r"\(-6\).*0 of 2 shifts converged") as ei:
        eng.solve_shifted(np.ones(A.shape[0]), shifts, maxiter=3)
    X, info = ei.value.partial
    assert list(info["iters"]) == [3, 3] and info["launched"] == 3 and info["converged"] == 0
    ref, _, _ = multishift_cg(A, np.ones(A.shape[0]), shifts, 1e-10, 3)   # the numpy restatement after three iterations
    assert np.abs(X - ref).max() <= 1e-12 * np.abs(ref).max()
    for s, sig in enumerate(shifts):
        res = np.linalg.norm(np.ones(A.shape[0]) - (sig * X[s] - A @ X[s])) / np.sqrt(A.shape[0])
        assert res > 1e-3 and abs(info["resid"][s] - res) <= 1e-12
    eng.close()


def test_deterministic(pkg):
    rp, ci = fixture("rmat_n3000_skew")
    A, _ = matrices(rp, ci)
    n = A.shape[0]
    lam = np.linalg.eigvalsh(A.toarray())[-1]
    b = np.random.default_rng(8).standard_normal(n)
    shifts = lam * np.array([1.05, 1.5, 3.0, 1.2])
    eng = engine(pkg, rp, ci)
    X, info = eng.solve_shifted(b, shifts)
    X2, info2 = eng.solve_shifted(b, shifts)
    assert np.array_equal(X, X2) and np.array_equal(info["resid"], info2["resid"]) and np.array_equal(info["iters"], info2["iters"])
    perm = [2, 0, 3, 1, 2]                              # a permutation, with a duplicate
    Xp, infop = eng.solve_shifted(b, shifts[perm])
    for i, s in enumerate(perm):
        assert np.array_equal(Xp[i], X[s]) and infop["iters"][i] == info["iters"][s], i
    xs, infos = eng.solve_shifted(b, shifts[0])         # the seed alone
    assert np.array_equal(xs, X[0]) and infos["iters"][0] == info["iters"][0]
    eng.close()
    e1 = engine(pkg, rp, ci, solve_poll=1)
    X1, info1 = e1.solve_shifted(b, shifts)
    e1.close()
    assert np.array_equal(X1, X) and np.array_equal(info1["iters"], info["iters"])
    assert info1["launched"] == info1["iterations"] <= info["launched"]


def test_isolation_and_refusals(pkg):
    rp, ci = fixture("er_n1000")
    A, _ = matrices(rp, ci)
    n = A.shape[0]
    lam = np.linalg.eigvalsh(A.toarray())[-1]
    eng = engine(pkg, rp, ci)
    k = 20
    eng.lanczos_multi(np.stack([np.ones(n), np.arange(n, dtype=np.float64) + 1.0]), k)
    T = np.random.default_rng(1).standard_normal((2, k))
    y_multi = eng.multout_multi(T)
    eng.lanczos(np.ones(n), k, want_q=False)
    t = np.random.default_rng(2).standard_normal(k)
    y_single = eng.multout(t)
    eng.solve_shifted(np.ones(n), [1.1 * lam, 2 * lam])
    assert np.array_equal(eng.multout_multi(T), y_multi) and np.array_equal(eng.multout(t), y_single)
    eng.lanczos_prepare(np.ones(n), k)
    eng.lanczos_run_steps(5)
    eng.solve_shifted(np.ones(n), 1.1 * lam)
    with pytest.raises(pkg.LzxError, match=r"\(-3\)"):
        eng.lanczos_run_steps(5)
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*<= 0 under A"):
        eng.solve_shifted(np.ones(n), 0.0)
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*rank-deficient"):
        eng.solve_shifted(np.ones(n), 2 * lam, W=np.stack([np.ones(n), 2.0 * np.ones(n)]))
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*span of W"):
        eng.solve_shifted(np.ones(n), 2 * lam, W=np.ones(n))
    eng.close()
    eng = engine(pkg, rp, ci, solve_state_bytes=5 * 1100 * 8)   # 5 vectors of about n_loc_pad + tail doubles
    with pytest.raises(pkg.LzxError, match=r"\(-4\).*bytes"):
        eng.solve_shifted(np.ones(n), [1.1 * lam, 2 * lam])      # 2 + 2 * 2 = 6 vectors of ldq > 1100 doubles
    x, info = eng.solve_shifted(np.ones(n), 1.1 * lam)           # 4 vectors fit
    assert info["converged"] == 1
    eng.close()
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(rp, ci)
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*one GPU"):
        grp.engines[0].solve_shifted(np.ones(n), 2 * lam)
    grp.close()


def test_c2_katz(pkg):
    eng = pkg.Engine(0)
    eng.gen_rmat(20, 1 << 20, C2_DRAWS, 1234)          # BASELINE C2, generated on the device
    rp, ci = eng.get_graph_csr()
    lam = float(eng.eigsh(nev=1, which="LA", want_vectors=False)[0][0])
    alphas = np.array([0.5, 0.7, 0.85, 0.95]) / lam
    n = len(rp) - 1
    X, info = eng.solve_shifted(np.ones(n), 1.0 / alphas, tol=1e-10)
    eng.close()
    A, _ = matrices(rp, ci)
    assert info["converged"] == 4
    for i, a in enumerate(alphas):
        res = np.linalg.norm(np.ones(n) - (X[i] / a - A @ X[i])) / np.sqrt(n)
        assert res <= 1e-9, (i, res)
        assert abs(info["resid"][i] - res) <= 1e-12
