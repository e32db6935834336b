"""CPU: the ten smallest graphs of tests/test_gpu_smallest.py and the references that module holds the library to -- no GPU.

Every graph fits a dense matrix, so the references are plain and of higher precision than the kernels: dense A and
L = D - A in np.longdouble for SpMV, SpMM and the Lanczos coefficients; numpy.linalg.eigh / solve and scipy.linalg.expm on the
dense matrices for the eigensolver, the solvers and e^(sM) x; the restatements of the tests/test_*_host.py modules for the graph
routines.  Here the references are checked themselves, on all ten graphs: the restatements against networkx / scipy wherever
networkx defines the quantity and does not raise (self loops removed where include/lzx.h says to compare that way), and the
Lanczos cases against the breakdown rule -- lzx_lanczos_f64 has no breakdown guard by contract, so the single-vector loop must
never be asked for a k past the Krylov dimension of its start vector, and the k_used the batched loop must report is that
dimension."""
import functools

import networkx as nx
import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

from test_communities_host import assert_equals_networkx as communities_equal_networkx
from test_communities_host import chain
from test_components_host import components_restatement, counts_of, scipy_labels
from test_core_host import assert_equals_networkx as core_equals_networkx
from test_core_host import networkx_reference as core_networkx
from test_core_host import peel_rounds, without_loops
from test_paths_host import EPS, bc_bound, brandes_batched
from test_similarity_host import assert_equals_networkx as similarity_equals_networkx
from test_similarity_host import similarity_restated
from test_sweep_host import sweep_ref
from test_triangles_host import assert_equals_networkx as triangles_equal_networkx
from test_triangles_host import networkx_reference as triangles_networkx
from test_triangles_host import triangles_oriented
from test_truss_host import edge_set, truss_rounds

LD = np.longdouble
LAP = 1
BREAKDOWN = 2.0 ** -40          # include/lzx.h: beta_j <= 2^-40 * max_{i<=j} (|alpha_i| + beta_{i-1}) stops a column
MULTI_K = 4                     # iterations asked of the batched loop: past every Krylov dimension that occurs here

# name: (n, undirected edges; (v, v) is a self loop = one diagonal entry)
GRAPHS = {
    "v1": (1, []),
    "loop1": (1, [(0, 0)]),
    "v2_empty": (2, []),
    "edge2": (2, [(0, 1)]),
    "edge_iso3": (3, [(0, 1)]),
    "path3": (3, [(0, 1), (1, 2)]),
    "triangle": (3, [(0, 1), (1, 2), (0, 2)]),
    "empty65": (65, []),                                   # one wavefront plus one
    "star65": (65, [(0, k) for k in range(1, 65)]),
    "edge_in_1025": (1025, [(7, 1024)]),                   # crosses every 256 / 512 / 1024 block size; 1023 rows without an edge
}
NAMES = list(GRAPHS)


class Small:
    """One of the ten graphs as symmetric pattern CSR (built here: no fixture file) with its dense matrices."""

    def __init__(self, name):
        self.name = name
        self.n, self.edges = GRAPHS[name]
        n = self.n
        P = np.zeros((n, n), dtype=bool)
        for u, v in self.edges:
            P[u, v] = P[v, u] = True
        self.A = sp.csr_matrix(P.astype(np.float64))
        self.A.sort_indices()
        self.rp, self.ci = self.A.indptr.astype(np.uint64), self.A.indices.astype(np.uint32)
        self.nnz = len(self.ci)
        self.d = np.diff(self.A.indptr).astype(np.float64)            # stored entries per row: a self loop counts once
        self.n_active = int((self.d > 0).sum())
        self.max_degree = int(self.d.max())
        self.Ad = P.astype(LD)
        self.Ld = np.diag(self.d.astype(LD)) - self.Ad
        self.A0 = sp.csr_matrix(without_loops(self.A))                # what networkx is asked about
        self.G = nx.from_scipy_sparse_array(self.A0)

    def M(self, op):
        """dense M in np.longdouble: A, or L = D - A under the Laplacian operator"""
        return self.Ld if op else self.Ad

    def M64(self, op):
        return self.M(op).astype(np.float64)

    def x_int(self, seed=3, b=None):
        """integer-valued entries in [-50, 50]: every row sum is an integer far below 2^53, exact in any order"""
        shape = self.n if b is None else (b, self.n)
        return np.random.default_rng(seed).integers(-50, 51, shape).astype(np.float64)

    def x0(self):
        """the start vector of the single-vector Lanczos cases"""
        return np.random.default_rng(5).standard_normal(self.n)

    def batch(self):
        """the start vectors of the batched cases: the single-vector one, the constant vector (L 1 = 0: its Krylov space closes
        at step 1 under L), the last unit vector (an isolated vertex on five of the graphs) and a second random one"""
        last = np.zeros(self.n)
        last[-1] = 1.0
        return np.stack([self.x0(), np.ones(self.n), last, np.random.default_rng(6).standard_normal(self.n)])

    def lam(self, op):
        """the spectrum of M, ascending (float64 eigh of the dense matrix)"""
        return np.linalg.eigh(self.M64(op))

    def expm(self, op, s, X):
        """e^(sM) X from the dense exponential in np.longdouble (expm_ld), rounded to float64 at the end"""
        return (expm_ld(s * self.M(op)) @ np.asarray(X, dtype=LD)).astype(np.float64)

    def all_pairs(self):
        """the pairs of the similarity cells: every u != v in both orders where n <= 3, otherwise a seeded sample that holds
        edges, the hub, isolated vertices and the last vertex"""
        n = self.n
        if n <= 3:
            return np.array([(u, v) for u in range(n) for v in range(n) if u != v], dtype=np.int64).reshape(-1, 2)
        rng = np.random.default_rng(8)
        pr = rng.integers(0, n, (60, 2))
        pr = pr[pr[:, 0] != pr[:, 1]]
        fixed = [(0, 1), (1, 0), (1, 2), (7, n - 1), (n - 1, 7), (n - 1, n - 2), (0, n - 1), (1, 64), (64, 1)]
        return np.vstack([np.array(fixed, dtype=np.int64), pr])

    def scores(self):
        """the score vectors of the sweep cells: random, constant (all ties), the degrees"""
        return np.stack([np.random.default_rng(9).standard_normal(self.n), np.ones(self.n), self.d])


@functools.lru_cache(maxsize=None)
def small(name):
    return Small(name)


# ---- the dense exponential in extended precision ---------------------------------------------------------------------------
def expm_ld(M):
    """e^M of a dense matrix by scaling and squaring around a Taylor series, every operation in np.longdouble: M / 2^j with a
    norm below 1/2, 30 terms (the remainder is below 2^-30 / 30!), then j squarings, each of which doubles a relative error that
    starts at the 2^-64 of the format -- j <= 8 here.  scipy.linalg.expm (Pade in float64) is itself only good to 1e-12 on
    star65, the bound e^(sM) x is held to, so it is the checked side here, not the reference."""
    M = np.asarray(M, dtype=LD)
    live = np.flatnonzero(np.abs(M).sum(axis=1) > 0)
    if len(live) < len(M):           # rows and columns of zeros (vertices without an edge) exponentiate to the identity
        E = np.eye(len(M), dtype=LD)
        if len(live):
            E[np.ix_(live, live)] = expm_ld(M[np.ix_(live, live)])
        return E
    norm = float(np.abs(M).sum(axis=1).max()) if M.size else 0.0
    j = max(0, int(np.ceil(np.log2(norm))) + 1) if norm > 0 else 0
    S = M / LD(2.0 ** j)
    E, term = np.eye(len(M), dtype=LD), np.eye(len(M), dtype=LD)
    for i in range(1, 31):
        term = term @ S / LD(i)
        E = E + term
    for _ in range(j):
        E = E @ E
    return E


# ---- Lanczos in extended precision ------------------------------------------------------------------------------------------
def lanczos_ld(M, x0, k, reorthogonalise=False):
    """k steps of the recurrence of lzx_lanczos_f64 on the dense M, every operation in np.longdouble: (alpha[k], beta[k], x_norm),
    beta[j] = ||v|| after step j (the library returns the first k - 1).  q_0 = fl64(x0 / ||x0||) rounded as the library's own
    division is.  Stops early (zeros behind) once the breakdown rule fires; with reorthogonalise the new vector is kept
    orthogonal to all earlier ones, so that the rule is evaluated on the exact Krylov space."""
    x0 = np.asarray(x0, dtype=np.float64)
    xn = float(np.sqrt(np.sum(x0.astype(LD) ** 2)))
    q = (x0 / xn).astype(LD)
    q_prev, b_prev = np.zeros_like(q), LD(0)
    alpha, beta = np.zeros(k, dtype=LD), np.zeros(k, dtype=LD)
    Q, scale = [q], LD(0)
    for j in range(k):
        v = M @ q
        alpha[j] = np.sum(v * q)
        v = v - alpha[j] * q - b_prev * q_prev
        if reorthogonalise:
            for u in Q:
                v = v - np.sum(v * u) * u
        beta[j] = np.sqrt(np.sum(v * v))
        scale = max(scale, abs(alpha[j]) + b_prev)
        if beta[j] <= BREAKDOWN * scale:
            beta[j] = 0
            break
        q_prev, b_prev, q = q, beta[j], v / beta[j]
        Q.append(q)
    return alpha, beta, xn


def krylov_dimension(M, x0):
    """the step at which the breakdown rule fires on the exact (re-orthogonalised, np.longdouble) Krylov space of x0: the k_used
    of the batched loop, and the largest k the single-vector loop may be asked for"""
    n = len(x0)
    _, beta, _ = lanczos_ld(M, x0, n, reorthogonalise=True)
    zero = np.flatnonzero(beta == 0)
    return int(zero[0]) + 1 if len(zero) else n


def krylov_rank(M, x0):
    """the same number by another route: the rank of the normalised Krylov matrix [x, Mx, M^2 x, ...] (numpy's SVD rank)"""
    cols, v = [], np.asarray(x0, dtype=np.float64)
    M = M.astype(np.float64)
    top = max(float(np.abs(M).sum(axis=1).max()), 1.0)
    for _ in range(min(len(x0), 6)):
        if np.linalg.norm(v) <= 1e-9 * top:          # M q = 0 up to the rounding of this float64 product: the space is closed
            break
        cols.append(v / np.linalg.norm(v))
        v = M @ cols[-1]
    return int(np.linalg.matrix_rank(np.stack(cols, axis=1), tol=1e-9))


@functools.lru_cache(maxsize=None)
def lanczos_case(name, op):
    """(x0, k, alpha, beta, x_norm) of the single-vector Lanczos cell: k = the Krylov dimension of x0 (at most 3 here), the
    coefficients in np.longdouble"""
    g = small(name)
    x0 = g.x0()
    k = krylov_dimension(g.M(op), x0)
    alpha, beta, xn = lanczos_ld(g.M(op), x0, k)
    return x0, k, alpha, beta, xn


@functools.lru_cache(maxsize=None)
def multi_case(name, op):
    """(X0, k_used expected per column) of the batched cell"""
    g = small(name)
    X0 = g.batch()
    return X0, np.array([min(krylov_dimension(g.M(op), x), MULTI_K) for x in X0], dtype=np.uint32)


# ---- the references themselves ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_graph_is_what_the_table_says(name):
    g = small(name)
    assert (g.A != g.A.T).nnz == 0 and g.A.has_sorted_indices and len(g.rp) == g.n + 1
    loops = sum(u == v for u, v in g.edges)
    assert g.nnz == 2 * (len(g.edges) - loops) + loops
    assert g.n_active == len({v for e in g.edges for v in e})
    assert np.array_equal(g.Ld.sum(axis=1), np.zeros(g.n))


@pytest.mark.parametrize("name", NAMES)
def test_graph_restatements_against_networkx_and_scipy(name):
    g = small(name)
    n, A, G = g.n, g.A, g.G
    # components
    labels, rounds = components_restatement(g.rp, g.ci)
    assert np.array_equal(labels, scipy_labels(g.rp, g.ci)) and rounds >= 1
    assert counts_of(labels)[0] == nx.number_connected_components(G)
    # paths: every vertex a source
    src = np.arange(n)
    r = brandes_batched(A, src)
    for s in range(n):
        want = np.full(n, -1)
        for v, dv in nx.single_source_shortest_path_length(G, s).items():
            want[v] = dv
        assert np.array_equal(r["dist"][s], want), s
    bc = nx.betweenness_centrality(G, normalized=False)
    ref = 2.0 * np.array([bc[v] for v in range(n)])
    bound = bc_bound(A, src, r["max_level"])
    assert not r["bc"][ref == 0].any() and (np.abs(r["bc"] - ref) <= bound * ref).all()
    if n > 1:                                                   # (networkx divides by n - 1)
        cl = nx.closeness_centrality(G)
        r1, tot = r["reached"].astype(np.float64) - 1.0, r["sum_dist"].astype(np.float64)
        mine = np.where(tot > 0, (r1 / np.maximum(tot, 1.0)) * (r1 / (n - 1.0)), 0.0)
        assert np.abs(mine - np.array([cl[v] for v in range(n)])).max() <= 4 * EPS
    # triangles, cores, trusses
    triangles_equal_networkx(triangles_oriented(A), triangles_networkx(g.A0))
    core_equals_networkx(peel_rounds(A), core_networkx(A))
    t = truss_rounds(A)
    for k in (2, 3, 4):
        want = {(min(u, v), max(u, v)) for u, v in nx.k_truss(G, k).edges()}
        assert edge_set(A, t["truss"], k) == want, k
    assert t["edges"] == G.number_of_edges() and t["triangles"] == sum(nx.triangles(G).values()) // 3
    # similarity (networkx has no pair on one vertex)
    pairs = g.all_pairs()
    s = similarity_restated(A, pairs)
    if len(pairs):
        similarity_equals_networkx(g.A0, pairs, similarity_restated(g.A0, pairs))
        for key in ("common", "deg_u", "deg_v", "jaccard", "adamic_adar"):
            assert np.array_equal(s[key], similarity_restated(g.A0, pairs)[key]), key     # a self loop changes nothing
    # colouring, label propagation, modularity
    communities_equal_networkx(A, chain(A, 0, True), chain(A, 0, False))
    # sweep profiles: cut and volume of every prefix
    for score in g.scores():
        w = sweep_ref(A, score)
        for k in range(1, n + 1) if n <= 65 else (1, 2, 7, 8, 9, n - 1, n):
            S = set(w["order"][:k].tolist())
            assert nx.volume(G, S) == w["vol"][k - 1], k
            assert (nx.cut_size(G, S) if k < n else 0) == w["cut"][k - 1], k


@pytest.mark.parametrize("name", NAMES)
def test_dense_references_agree_with_each_other(name):
    """The np.longdouble matrices against scipy's product; the np.longdouble exponential against V e^(s lambda) V^T of
    numpy.linalg.eigh at 1e-13 and against scipy.linalg.expm at the 1e-11 that Pade approximant is good for."""
    g = small(name)
    x = g.x_int()
    assert np.array_equal((g.Ad @ x.astype(LD)).astype(np.float64), g.A @ x)
    assert np.array_equal((g.Ld @ x.astype(LD)).astype(np.float64), g.d * x - g.A @ x)
    for op, s in ((0, 1.0), (LAP, -1.0)):
        lam, V = g.lam(op)
        E = expm_ld(s * g.M(op)).astype(np.float64)
        assert np.abs((V * np.exp(s * lam)) @ V.T - E).max() <= 1e-13 * np.abs(E).max()
        assert np.abs(scipy.linalg.expm(s * g.M64(op)) - E).max() <= 1e-11 * np.abs(E).max()


@pytest.mark.parametrize("op", [0, LAP], ids=["A", "L"])
@pytest.mark.parametrize("name", NAMES)
def test_lanczos_cases_stay_within_their_krylov_space(name, op):
    """beta_j > 2^-40 * max(|alpha| + beta) for every j < k - 1, in np.longdouble: the single-vector loop divides by beta_j"""
    g = small(name)
    x0, k, alpha, beta, xn = lanczos_case(name, op)
    assert 1 <= k <= min(g.n, 3) and k == krylov_rank(g.M(op), x0)
    scale = LD(0)
    for j in range(k - 1):
        scale = max(scale, abs(alpha[j]) + (beta[j - 1] if j else LD(0)))
        assert beta[j] > BREAKDOWN * scale, (j, beta[j], scale)
        assert beta[j] > 1e-3 * scale, (j, beta[j], scale)      # and far from it: no rounding of the device's can cross the rule
    # one step more would break down: k is the whole space
    _, b_more, _ = lanczos_ld(g.M(op), x0, k + 1 if k < g.n else k, reorthogonalise=True)
    assert k == g.n or b_more[k - 1] == 0


@pytest.mark.parametrize("op", [0, LAP], ids=["A", "L"])
@pytest.mark.parametrize("name", NAMES)
def test_batched_k_used_is_the_krylov_dimension(name, op):
    g = small(name)
    X0, k_used = multi_case(name, op)
    assert len(X0) == 4 and np.all(k_used >= 1) and np.all(k_used <= min(g.n, MULTI_K))
    for x, ku in zip(X0, k_used):
        assert ku == krylov_rank(g.M(op), x)
        alpha, beta, _ = lanczos_ld(g.M(op), x, MULTI_K, reorthogonalise=True)
        scale = LD(0)
        for j in range(int(ku) - 1):                           # the steps before the stop are far from the rule
            scale = max(scale, abs(alpha[j]) + (beta[j - 1] if j else LD(0)))
            assert beta[j] > 1e-3 * scale, (j, beta[j], scale)
    if op == LAP:
        assert k_used[1] == 1                                   # the constant vector: a column that closes at step 1, on every graph
    if g.nnz == 0:
        assert np.all(k_used == 1)
