"""GPU: extreme eigenpairs by thick-restart Lanczos (include/lzx.h: lzx_eigsh_f64, Engine.eigsh) against numpy.linalg.eigh on
the golden fixtures (scipy eigsh where n > 4096): the adjacency's largest pairs, lambda_2 and the Fiedler vector under L with
deflation, the Laplacian's largest, the breakdown restart, BASELINE C2, and determinism, isolation and refusals."""
import glob
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csg
from scipy.sparse.linalg import eigsh

from bench import C2_DRAWS

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


def check_pairs(M, w, V, info, w_ref, V_ref, norm, what):
    """eigenvalues, orthonormality, reported residuals, and the vectors where the gap allows a bound (Davis-Kahan)."""
    nev = len(w)
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(V)), what
    assert np.abs(w - w_ref).max() <= 1e-9 * norm, (what, w, w_ref)
    assert np.abs(V.T @ V - np.eye(nev)).max() <= 1e-10, what
    true_res = np.linalg.norm(M @ V - V * w, axis=0)
    assert np.abs(info["resid"] - true_res).max() <= 1e-12 * norm, (what, info["resid"], true_res)
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


def dense(M):
    return np.linalg.eigh(M.toarray())


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_adjacency_largest(pkg, path):
    name = os.path.basename(path)[:-4]
    rp, ci = fixture(name)
    A, _ = matrices(rp, ci)
    eng = engine(pkg, rp, ci)
    # (m = 40: star_ring's pairs 2 cos(2 pi k / n) cluster within 1e-5 of each other, m = 20 needs more than 300 restarts)
    w, V, info = eng.eigsh(nev=6, which="LA", m=40, tol=1e-10)
    eng.close()
    assert info["converged"] == 6 and info["m"] == 40 and info["matvecs"] >= 40
    assert np.all(np.diff(w) >= 0)
    if A.shape[0] <= 4096:
        # one copy per eigenspace (lzx.h: a single start vector finds one vector of a repeated eigenvalue; star_ring's ring
        # pairs 2 cos(2 pi k / n) are double): the top 6 distinct eigenvalues, with a vector only where the value is simple
        lam, U = dense(A)
        tol = 1e-9 * abs(lam).max()
        keep, simple = [], []
        for i in range(len(lam) - 1, -1, -1):
            if keep and abs(lam[keep[-1]] - lam[i]) <= tol:
                simple[-1] = False
                continue
            if len(keep) == 6:
                break
            keep.append(i)
            simple.append(True)
        keep, simple = keep[::-1], simple[::-1]
        w_ref, V_ref = lam[keep], (U[:, keep] if all(simple) else None)
    else:
        w_ref, V_ref = eigsh(A, k=6, which="LA", tol=1e-13)
        o = np.argsort(w_ref)
        w_ref, V_ref = w_ref[o], V_ref[:, o]
    norm = max(abs(w_ref).max(), info["norm_est"])
    check_pairs(A, w, V, info, w_ref, V_ref, norm, name)


def largest_component(rp, ci):
    A, _ = matrices(rp, ci)
    _, lab = csg.connected_components(A, directed=False)
    keep = np.nonzero(lab == np.bincount(lab).argmax())[0]
    B = A[keep][:, keep].tocsr()
    B.sort_indices()
    return B.indptr.astype(np.uint64), B.indices.astype(np.uint32)


@pytest.mark.parametrize("name", ["er_n1000", "er_n4000_deg20", "star_ring_n1500", "rmat_n4096_giant"])
def test_fiedler_with_deflation(pkg, name):
    rp, ci = fixture(name.replace("_giant", ""))
    if name.endswith("_giant"):
        rp, ci = largest_component(rp, ci)
    A, L = matrices(rp, ci)
    n = A.shape[0]
    assert csg.connected_components(A, directed=False)[0] == 1
    eng = engine(pkg, rp, ci, op=LAP)
    w, V, info = eng.eigsh(nev=1, which="SA", deflate=np.full(n, 1.0 / np.sqrt(n)), tol=1e-10)
    eng.close()
    lam, U = dense(L)
    norm = lam[-1]
    assert abs(np.sum(V[:, 0])) <= 1e-10 * np.sqrt(n)        # orthogonal to the deflated constant vector
    # star_ring's lambda_2 is double (1.00001757 twice): any unit vector of that eigenspace is right
    check_pairs(L, w, V, info, lam[1:2], None if abs(lam[2] - lam[1]) < 1e-6 * norm else U[:, 1:2], norm, name)
    if name == "er_n1000":
        assert abs(w[0] - 0.784519) < 1e-6


def test_laplacian_largest(pkg):
    rp, ci = fixture("rmat_n3000_skew")
    _, L = matrices(rp, ci)
    eng = engine(pkg, rp, ci, op=LAP)
    w, V, info = eng.eigsh(nev=3, which="LA", tol=1e-10)
    eng.close()
    lam, U = dense(L)
    assert np.allclose(w, [570.4277, 581.1049, 1010.0063], atol=1e-4)
    check_pairs(L, w, V, info, lam[-3:], U[:, -3:], lam[-1], "rmat_n3000_skew L")


def small_component_vertex(A, size):
    _, lab = csg.connected_components(A, directed=False)
    comp = np.nonzero(np.bincount(lab) == size)[0][0]
    return int(np.nonzero(lab == comp)[0][0])


def test_breakdown_restart(pkg):
    """x0 = e_v in a 2-vertex component: the first cycle breaks down on its invariant subspace at step 1, the next one starts
    from a fresh probe and finds what is wanted in the rest of the graph."""
    rp, ci = fixture("rmat_n4096")
    A, L = matrices(rp, ci)
    n = A.shape[0]
    x0 = np.zeros(n)
    x0[small_component_vertex(A, 2)] = 1.0
    eng = engine(pkg, rp, ci)
    w, V, info = eng.eigsh(nev=6, which="LA", x0=x0, tol=1e-10)
    eng.close()
    lam, U = dense(A)
    check_pairs(A, w, V, info, lam[-6:], U[:, -6:], lam[-1], "rmat_n4096 A from e_v")
    # under L: the breakdown keeps the small component's null vector, the fresh probe brings a second, orthogonal one
    eng = engine(pkg, rp, ci, op=LAP)
    w, V, info = eng.eigsh(nev=2, which="SA", x0=x0, tol=1e-10)
    eng.close()
    norm = float(np.linalg.eigvalsh(L.toarray())[-1])
    assert np.all(np.isfinite(V)) and np.abs(w).max() <= 1e-9 * norm
    assert np.abs(V.T @ V - np.eye(2)).max() <= 1e-10
    assert np.abs(L @ V).max() <= 1e-8 * norm          # constant on every component
    assert info["resid"].max() <= 1e-8 * norm


def test_c2_largest(pkg):
    eng = pkg.Engine(0)
    eng.gen_rmat(20, 1 << 20, C2_DRAWS, 1234)          # BASELINE C2, generated on the device
    rp, ci = eng.get_graph_csr()
    w, V, info = eng.eigsh(nev=8, which="LA", tol=1e-10)
    eng.close()
    A, _ = matrices(rp, ci)
    ref = np.sort(eigsh(A, k=8, which="LA", tol=1e-12, return_eigenvectors=False))
    norm = ref[-1]
    assert np.abs(w - ref).max() <= 1e-9 * norm, (w, ref)
    res = np.linalg.norm(A @ V - V * w, axis=0)
    assert res.max() <= 1e-8 * norm and np.abs(info["resid"] - res).max() <= 1e-12 * norm * 10
    _, lab = csg.connected_components(A, directed=False)
    giant = lab == np.bincount(lab).argmax()
    top = V[:, -1]
    assert np.all(top[giant] > 0)                      # Perron: one-signed (positive by the sign rule) on the giant component
    assert np.abs(top[~giant]).max() <= 1e-6


def test_deterministic_and_isolated(pkg):
    rp, ci = fixture("er_n1000")
    n = len(rp) - 1
    eng = engine(pkg, rp, ci)
    k = 20
    # state that must survive: a resident batch basis and a single-vector basis
    eng.lanczos_multi(np.stack([np.ones(n), np.arange(n, dtype=np.float64) + 1.0]), k)
    T = np.random.default_rng(1).standard_normal((2, k))
    y_multi = eng.multout_multi(T)
    eng.lanczos(np.ones(n), k, want_q=False)
    t = np.random.default_rng(2).standard_normal(k)
    y_single = eng.multout(t)
    a = eng.eigsh(nev=4, which="LA")
    b = eng.eigsh(nev=4, which="LA")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2]["resid"], b[2]["resid"])
    assert all(a[2][f] == b[2][f] for f in ("converged", "restarts", "matvecs", "m", "norm_est"))
    assert np.array_equal(eng.multout_multi(T), y_multi) and np.array_equal(eng.multout(t), y_single)
    # a prepared, chunked decomposition is void afterwards, as after lzx_spmv_f64
    eng.lanczos_prepare(np.ones(n), k)
    eng.lanczos_run_steps(5)
    eng.eigsh(nev=2)
    with pytest.raises(pkg.LzxError, match=r"\(-3\)"):
        eng.lanczos_run_steps(5)
    # non-convergence: LZX_ERR_LIMIT, with the best pairs attached
    with pytest.raises(pkg.LzxError, match=r"\(-6\).*of 4 pairs converged") as ei:
        eng.eigsh(nev=4, tol=1e-15, max_restarts=1)
    w, V, info = ei.value.partial
    assert info["converged"] < 4 and info["restarts"] == 1 and np.all(np.isfinite(w)) and V.shape == (n, 4)
    assert abs(w[-1] - a[0][-1]) < 1e-3 * abs(a[0][-1])
    # refusals
    with pytest.raises(pkg.LzxError, match=r"\(-1\)"):
        eng.eigsh(nev=4, m=5)                            # nev + 2 > m
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*rank-deficient"):
        eng.eigsh(nev=1, which="SA", deflate=np.stack([np.ones(n), 2.0 * np.ones(n)]))
    eng.close()


def test_out_of_memory_leaves_nothing(pkg):
    rp, ci = fixture("er_n1000")
    eng = pkg.Engine(0, eig_basis_bytes=30 * 1100 * 8)   # 30 columns of about n_loc_pad + tail doubles
    eng.set_graph_csr(rp, ci)
    with pytest.raises(pkg.LzxError, match=r"\(-4\).*bytes"):
        eng.eigsh(nev=2, m=40)
    w, _, info = eng.eigsh(nev=2, m=20)
    assert info["converged"] == 2 and np.all(np.isfinite(w))
    eng.close()


def test_communicator_handle_refused(pkg):
    rp, ci = fixture("er_n1000")
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(rp, ci)
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*one GPU"):
        grp.engines[0].eigsh(nev=2)
    grp.close()
