"""GPU: lzx_eigsh_f64 where its kernels change shape -- m = 128 (k_eig_rotate at 64 KiB of LDS and on its
second and third column groups, p > 32; k_eig_proj / k_eig_update at J = 137), the default m at nev = 24, eight deflation
vectors (an invariant subspace that is neither orthogonal nor unit; W as the tool for repeated eigenvalues), and m + nw == n.
End to end against numpy.linalg.eigh with check_pairs' tolerances, and the dense kernels on their own through the test hook
lzx_test_eig_ops against numpy.longdouble with derived bounds."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csg

from test_gpu_eigsh import LAP, check_pairs, dense, engine, fixture, matrices

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


def csr_arrays(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.uint64), A.indices.astype(np.uint32)


def gnp(rng, n, prob):
    up = np.triu(rng.random((n, n)) < prob, 1)
    return sp.csr_matrix((up | up.T).astype(np.float64))


def connected(A):
    return csg.connected_components(A, directed=False)[0] == 1


BLOCK_SIZES = tuple(range(90, 231, 20))   # eight blocks, n = 1280


def blocks8():
    """block diagonal of eight connected G(s, 6/s) graphs (a block is drawn again until it is connected)"""
    rng = np.random.default_rng(8)
    parts = []
    for s in BLOCK_SIZES:
        B = gnp(rng, s, 6.0 / s)
        while not connected(B):
            B = gnp(rng, s, 6.0 / s)
        parts.append(B)
    return sp.block_diag(parts, format="csr")


def gnp136():
    return gnp(np.random.default_rng(136), 136, 0.3)


@functools.lru_cache(maxsize=None)
def graph(name):
    """(row_ptr, col_idx, A, L) of a golden fixture or of one of this file's generated graphs"""
    if name == "blocks8":
        rp, ci = csr_arrays(blocks8())
    elif name == "er_n1000_twice":
        B, _ = matrices(*fixture("er_n1000"))
        rp, ci = csr_arrays(sp.block_diag([B, B], format="csr"))
    elif name == "gnp136":
        rp, ci = csr_arrays(gnp136())
    elif name == "gnp135":
        rp, ci = csr_arrays(gnp136()[:135][:, :135])
    else:
        rp, ci = fixture(name)
    A, L = matrices(rp, ci)
    return rp, ci, A, L


@functools.lru_cache(maxsize=None)
def spectrum(name, op=0):
    """numpy.linalg.eigh of the dense A (op = 0) or L, computed once and shared read-only"""
    lam, U = dense(graph(name)[2 + op])
    lam.setflags(write=False)
    U.setflags(write=False)
    return lam, U


def assert_separated(values, norm, what):
    """the wanted values and the next one pairwise further apart than 1e-6 norm: check_pairs then skips no vector"""
    gaps = np.diff(np.sort(values))
    assert gaps.min() > 1e-6 * norm, (what, gaps.min() / norm)
    return gaps.min() / norm


def record(what, info, gap=None):
    print(f"[eigsh-limits] {what}: m={info['m']} restarts={info['restarts']} matvecs={info['matvecs']} converged={info['converged']}"
          + ("" if gap is None else f" min_rel_gap={gap:.2e}"))


def assert_second_column_group(info, nev, m):
    """the restart's k_eig_rotate went beyond its first group of 32 output columns"""
    assert nev + (m - nev) // 2 > 32 and info["restarts"] >= 1, (nev, m, info["restarts"])


# ---------------------------------------------------------------------------------------------- A1, A2, A6: large m, large p
def top_of_adjacency(pkg, name, nev, m):
    rp, ci, A, _ = graph(name)
    eng = engine(pkg, rp, ci)
    try:
        return eng.eigsh(nev=nev, which="LA", m=m, tol=1e-10)
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["er_n1000", "rmat_n3000_skew", "rmat_n4096"])
def test_top40_m128(pkg, name):
    """A, LA, nev = 40, m = 128: p = 84 (three trips of wavefront 0 in k_eig_rotate), 64 KiB of LDS, J up to 129"""
    A = graph(name)[2]
    lam, U = spectrum(name)
    norm = np.abs(lam).max()
    gap = assert_separated(lam[-41:], norm, name)
    w, V, info = top_of_adjacency(pkg, name, 40, 128)
    record(f"A1 {name}", info, gap)
    assert info["converged"] == 40 and info["m"] == 128
    assert_second_column_group(info, 40, 128)
    check_pairs(A, w, V, info, lam[-40:], U[:, -40:], norm, name)


@pytest.mark.parametrize("name", ["er_n1000", "rmat_n3000_skew"])
def test_default_m_nev24(pkg, name):
    """A, LA, nev = 24 with the default m = 2 nev + 1 = 49: p = 36, what a user gets from nev >= 22"""
    A = graph(name)[2]
    lam, U = spectrum(name)
    norm = np.abs(lam).max()
    gap = assert_separated(lam[-25:], norm, name)
    w, V, info = top_of_adjacency(pkg, name, 24, 0)
    record(f"A2 {name}", info, gap)
    assert info["converged"] == 24 and info["m"] == 49
    assert_second_column_group(info, 24, 49)
    check_pairs(A, w, V, info, lam[-24:], U[:, -24:], norm, name)


def test_deterministic_at_the_limit(pkg):
    a = top_of_adjacency(pkg, "er_n1000", 40, 128)
    b = top_of_adjacency(pkg, "er_n1000", 40, 128)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2]["resid"], b[2]["resid"])
    assert all(a[2][f] == b[2][f] for f in ("converged", "restarts", "matvecs", "m"))


# ---------------------------------------------------------------------------------------------- A3: eight deflation vectors
def block_indicators():
    n = sum(BLOCK_SIZES)
    ind = np.zeros((8, n))
    lo = 0
    for t, s in enumerate(BLOCK_SIZES):
        ind[t, lo:lo + s] = 1.0
        lo += s
    return ind


def check_deflated_laplacian(eng, W, nev, m, what):
    _, _, _, L = graph("blocks8")
    n = L.shape[0]
    lam, U = spectrum("blocks8", 1)
    norm = lam[-1]
    assert np.abs(lam[:8]).max() <= 1e-12 * norm           # eight connected blocks: the null space is the span of W
    gap = assert_separated(lam[7:8 + nev + 1], norm, what)
    w, V, info = eng.eigsh(nev=nev, which="SA", m=m, tol=1e-10, deflate=W)
    record(what, info, gap)
    assert info["converged"] == nev and info["m"] == m and info["restarts"] >= 1
    check_pairs(L, w, V, info, lam[8:8 + nev], U[:, 8:8 + nev], norm, what)
    assert np.abs(W @ V).max() <= 1e-10 * np.sqrt(n), what
    return info


@pytest.mark.parametrize("nev,m", [(8, 40), (40, 128)])
def test_eight_deflation_vectors(pkg, nev, m):
    """L, SA, W = a fixed random 8 x 8 matrix times the eight component indicators: neither orthogonal nor unit, so the
    orthonormalisation of W columns 1 to 7 on the device does real work; the wanted pairs are lam[8 : 8 + nev] of L"""
    mix = np.random.default_rng(88).standard_normal((8, 8))
    assert np.linalg.cond(mix) < 1e3
    W = mix @ block_indicators()
    assert np.abs(W @ W.T - np.eye(8)).max() > 1.0
    rp, ci, _, _ = graph("blocks8")
    eng = engine(pkg, rp, ci, op=LAP)
    try:
        info = check_deflated_laplacian(eng, W, nev, m, f"A3 nev={nev} m={m}")
    finally:
        eng.close()
    if nev == 40:
        assert_second_column_group(info, nev, m)


def test_component_indicators_as_deflation(pkg):
    """the README's route: Engine.components, then Engine.component_indicators as W"""
    rp, ci, _, _ = graph("blocks8")
    eng = engine(pkg, rp, ci, op=LAP)
    try:
        labels, cinfo = eng.components()
        assert cinfo["n_components"] == 8
        W = pkg.Engine.component_indicators(labels, np.unique(labels))
        check_deflated_laplacian(eng, W, 8, 40, "A3 component_indicators")
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- A4: W and repeated eigenvalues
def test_deflation_finds_the_second_copy(pkg):
    """A = block_diag(B, B): every eigenvalue is double.  With W = one vector u_i of each of the top eight eigenspaces the call
    must return the same eight values with the other vector, +-u'_i."""
    rp, ci, A, _ = graph("er_n1000_twice")
    n = A.shape[0]
    lam, U = spectrum("er_n1000_twice")
    norm = np.abs(lam).max()
    assert np.abs(lam[n - 18::2] - lam[n - 17::2]).max() <= 1e-12 * norm       # pairs
    distinct = lam[n - 17::2]                                                    # nine values ascending: the next one, then the wanted eight
    gap = assert_separated(distinct, norm, "A4")
    u, u2 = U[:, n - 15::2], U[:, n - 16::2]                                     # (n, 8) each, ascending like distinct[1:]
    W = np.ascontiguousarray(u.T)
    eng = engine(pkg, rp, ci)
    try:
        w, V, info = eng.eigsh(nev=8, which="LA", m=40, tol=1e-10, deflate=W)
    finally:
        eng.close()
    record("A4", info, gap)
    assert info["converged"] == 8
    w_ref = distinct[1:]
    check_pairs(A, w, V, info, w_ref, None, norm, "A4")
    res = np.linalg.norm(A @ V - V * w, axis=0)
    for i in range(8):
        near = min(w_ref[i] - distinct[i], (w_ref[i + 1] - w_ref[i]) if i < 7 else np.inf)
        c = abs(V[:, i] @ u2[:, i])
        assert 1.0 - c <= max(1e-8, 2.0 * (res[i] / near) ** 2), (i, c, res[i], near)
    assert np.abs(W @ V).max() <= 1e-10


# ---------------------------------------------------------------------------------------------- A5: m + nw == n
def test_m_plus_nw_equals_n(pkg):
    """n = 136, m = 128, nw = 8: the first cycle spans the whole complement of W, so its last step breaks down with nothing
    left to explore.  The Ritz pairs are then exact and the call ends there."""
    rp, ci, A, _ = graph("gnp136")
    assert A.shape[0] == 136 and connected(A)
    lam, U = spectrum("gnp136")
    norm = np.abs(lam).max()
    gap = assert_separated(lam, norm, "gnp136")
    W = np.ascontiguousarray(U[:, -8:].T)
    eng = engine(pkg, rp, ci)
    try:
        w, V, info = eng.eigsh(nev=4, which="LA", m=128, tol=1e-10, deflate=W)
    finally:
        eng.close()
    record(f"A5 gnp136 ({len(ci)} stored entries)", info, gap)
    check_pairs(A, w, V, info, lam[-12:-8], U[:, -12:-8], norm, "gnp136")
    assert np.abs(W @ V).max() <= 1e-10
    assert info["converged"] == 4 and info["m"] == 128
    assert info["restarts"] <= 1


def test_m_plus_nw_beyond_n_refused(pkg):
    rp, ci, A, _ = graph("gnp135")
    assert A.shape[0] == 135
    eng = engine(pkg, rp, ci)
    try:
        with pytest.raises(pkg.LzxError, match=r"\(-1\).*m \+ nw"):
            eng.eigsh(nev=4, which="LA", m=128, deflate=np.eye(8, 135))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- B: the dense kernels on their own
GS_COLUMNS = (1, 7, 8, 9, 64, 129, 137)
ROTATIONS = ((8, 8), (9, 9), (40, 23), (64, 33), (128, 32), (128, 33), (128, 65), (128, 126))
HOOK_GRAPHS = ("er_n1000", "gnp136")


@pytest.fixture(scope="module")
def hook_engines(pkg):
    made = {}
    for name in HOOK_GRAPHS:
        rp, ci, _, _ = graph(name)
        made[name] = engine(pkg, rp, ci)
    yield made
    for eng in made.values():
        eng.close()


@functools.lru_cache(maxsize=None)
def hook_inputs(n, J):
    """Q = the Q-factor of a fixed random n x J matrix, w random; read-only"""
    rng = np.random.default_rng(1000 * n + J)
    Q = np.linalg.qr(rng.standard_normal((n, J)))[0]
    w = rng.standard_normal(n)
    assert Q.shape == (n, J)
    Q.setflags(write=False)
    w.setflags(write=False)
    return Q, w


def gs_columns(n):
    """The issue's J, on a graph with n vertices.  Q needs J orthonormal columns of length n and something of w left outside
    their span, so J < n: where the list goes past that (137 at n = 136; the solver itself never orthogonalises against more
    than m + nw <= n columns) the largest possible J = n - 1 stands in."""
    return sorted({min(J, n - 1) for J in GS_COLUMNS})


@pytest.mark.parametrize("name,J", [(name, J) for name in HOOK_GRAPHS for J in gs_columns({"er_n1000": 1000, "gnp136": 136}[name])])
def test_gram_schmidt_kernels(hook_engines, name, J):
    """lzx_cgs2 + lzx_cgs_normalise over J columns (k_eig_proj, k_eig_close, k_eig_update, k_eig_scale): coef = h1 + h2, beta and
    the unit vector against (I - Q Q^T) w in long double.
    coef: each of the two passes is a dot product of n terms, error at most n u sum_i |q_ci w_i| to first order in any order
    of summation (u = 2^-53); the bound allows four.  beta * w_out: 2 J updates of n-vectors, each entry off by a few u |h_c|
    |q_ci|, summed in the 2-norm with |h| <= ||w||: well under 8 n u ||w|| sqrt(J)."""
    eng = hook_engines[name]
    n = eng.n
    Q, w = hook_inputs(n, J)
    coef, w_out, beta, _ = eng.eig_ops(Q, w)
    Ql, wl = Q.astype(np.longdouble), w.astype(np.longdouble)
    dots = Ql.T @ wl
    err = np.abs(coef - dots)
    bound = 4.0 * n * U53 * (np.abs(Ql).T @ np.abs(wl))
    print(f"[eig-ops] {name} J={J}: coef err/bound max {float((err / bound).max()):.3e}")
    assert np.all(err <= bound), (name, J, float((err / bound).max()))
    ref = wl - Ql @ dots
    dev = float(np.linalg.norm(w_out.astype(np.longdouble) * np.longdouble(beta) - ref))
    vbound = 8.0 * n * U53 * np.linalg.norm(w) * np.sqrt(J)
    leak = float(np.abs(Ql.T @ w_out.astype(np.longdouble)).max())
    print(f"[eig-ops] {name} J={J}: beta={beta:.6e} vector err {dev:.3e} (bound {vbound:.3e}) |Q^T w_out| {leak:.3e}")
    assert beta > 0.0 and abs(beta - float(np.linalg.norm(ref))) <= vbound
    assert dev <= vbound, (name, J, dev, vbound)
    assert leak <= 1e-14, (name, J, leak)


@pytest.mark.parametrize("name", HOOK_GRAPHS)
@pytest.mark.parametrize("J,p", ROTATIONS, ids=[f"{J}x{p}" for J, p in ROTATIONS])
def test_rotation_kernel(hook_engines, name, J, p):
    """k_eig_rotate through the driver's launch: R = (Q Y)^T element-wise against long double.  An entry is a sum of J products
    added one after another: error at most (J - 1 + 1) u sum_k |q_ik| |y_kc| to first order; the bound allows twice that."""
    eng = hook_engines[name]
    n = eng.n
    Q, w = hook_inputs(n, J)
    Y = np.random.default_rng(77 * J + p).standard_normal((J, p))
    _, _, _, R = eng.eig_ops(Q, w, Y)
    assert R.shape == (p, n)
    ref = (Q.astype(np.longdouble) @ Y.astype(np.longdouble)).T
    bound = 2.0 * J * U53 * (np.abs(Q) @ np.abs(Y)).T
    ratio = float((np.abs(R - ref) / bound).max())
    print(f"[eig-ops] {name} J={J} p={p}: rotation err/bound max {ratio:.3e}")
    assert np.all(np.isfinite(R)) and ratio <= 1.0, (name, J, p, ratio)
