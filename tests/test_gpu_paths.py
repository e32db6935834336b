"""GPU: batched breadth-first search and betweenness on the device (include/lzx.h: lzx_bfs_multi, lzx_betweenness_f64;
Engine.bfs / closeness / harmonic / betweenness): known answers on small graphs with every vertex as a source, the golden
fixtures against the numpy restatement of tests/test_paths_host.py and against networkx, every batch shape bit for bit, forced
long rows, self loops, both hand-over forms, isolation from the handle's other state, and the error paths.

Tolerances are those derived in tests/test_paths_host.py: distances, path counts and the integer scalars exact; bc within
2 (L (d_max + 4) + ns) 2^-53 of the reference, relative, entry by entry, and exactly 0 where the reference is 0; harmonic and
closeness within n 2^-53."""
import ctypes
import functools
import math
import os

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp

from test_paths_host import EPS, GOLDEN, GOLDEN_IDS, assert_bc_close, bc_bound, brandes_batched, fixture_sources, load_fixture

pytestmark = pytest.mark.gpu

_u32p = ctypes.POINTER(ctypes.c_uint32)
_f64p = ctypes.POINTER(ctypes.c_double)
SCALARS = ("reached", "sum_dist", "harmonic", "ecc")


def golden(name):
    return GOLDEN[GOLDEN_IDS.index(name)]


def engine_of(pkg, A, **options):
    eng = pkg.Engine(0, **options)
    A = sp.csr_matrix(A)
    A.sort_indices()
    eng.set_graph_csr(A.indptr.astype(np.uint64), A.indices.astype(np.uint32))
    return eng


def adjacency(n, edges):
    M = sp.lil_matrix((n, n))
    for u, v in edges:
        M[u, v] = 1.0
        M[v, u] = 1.0
    return sp.csr_matrix(M)


@functools.lru_cache(maxsize=None)
def fixture_case(path):
    """(A, the 48 sources of the host test + vertex 0 + the vertex of largest degree, their restatement): once per fixture"""
    A = load_fixture(path)
    src = np.concatenate([fixture_sources(A.shape[0]), [0, int(np.argmax(np.diff(A.indptr)))]])
    return A, src, brandes_batched(A, src)


def check_against(eng, A, src, ref):
    """one bfs and one betweenness call on `src` against the restatement `ref`"""
    n = A.shape[0]
    D, P, info = eng.bfs(src, paths=True)
    assert np.array_equal(D, ref["dist"]) and np.array_equal(P, ref["paths"])
    for key in ("reached", "sum_dist", "ecc"):
        assert np.array_equal(info[key], ref[key]), key
    assert (np.abs(info["harmonic"] - ref["harmonic"]) <= n * EPS * ref["harmonic"]).all()
    assert info["max_level"] == ref["max_level"] and info["ns"] == len(src) and info["batches"] == (len(src) + 15) // 16
    bc, binfo = eng.betweenness_raw(src)
    bound = bc_bound(A, src, ref["max_level"])
    print("bc: largest relative difference", float(np.max(np.abs(bc - ref["bc"]) / np.where(ref["bc"] > 0, ref["bc"], 1.0))), "bound", bound,
          "sweeps", binfo["sweeps"], "sweep_ms", binfo["sweep_ms"])
    assert_bc_close(bc, ref["bc"], bound)
    return D, P, info, bc


# ---- 1. known answers, every vertex a source ------------------------------------------------------------------------------
def path_graph(n):
    i = np.arange(n)
    return (adjacency(n, [(k, k + 1) for k in range(n - 1)]), np.abs(i[:, None] - i[None, :]), np.ones((n, n)), 2.0 * i * (n - 1 - i))


def star_graph(n):
    dist = np.full((n, n), 2)
    dist[0, :] = dist[:, 0] = 1
    np.fill_diagonal(dist, 0)
    bc = np.zeros(n)
    bc[0] = (n - 1.0) * (n - 2.0)                       # every ordered pair of leaves
    return adjacency(n, [(0, k) for k in range(1, n)]), dist, np.ones((n, n)), bc


def complete_graph(n):
    return adjacency(n, [(u, v) for u in range(n) for v in range(u)]), 1 - np.eye(n, dtype=np.int64), np.ones((n, n)), np.zeros(n)


def cycle_graph(n):
    i = np.arange(n)
    gap = np.abs(i[:, None] - i[None, :])
    dist = np.minimum(gap, n - gap)
    paths = np.where(dist == n // 2, 2.0, 1.0)          # n even: two ways round to the antipode
    return adjacency(n, [(k, (k + 1) % n) for k in range(n)]), dist, paths, np.full(n, (n - 2.0) ** 2 / 4.0)


def grid_graph(m):
    n = m * m
    x, y = np.divmod(np.arange(n), m)
    dx, dy = np.abs(x[:, None] - x[None, :]), np.abs(y[:, None] - y[None, :])
    paths = np.array([[float(math.comb(int(a + b), int(a))) for a, b in zip(ra, rb)] for ra, rb in zip(dx, dy)])
    A = adjacency(n, [(k, k + 1) for k in range(n) if (k + 1) % m] + [(k, k + m) for k in range(n - m)])
    ref = nx.betweenness_centrality(nx.from_scipy_sparse_array(A), normalized=False)
    return A, dx + dy, paths, 2.0 * np.array([ref[v] for v in range(n)])


def hypercube_graph(q):
    n = 1 << q
    i = np.arange(n)
    x = i[:, None] ^ i[None, :]
    dist = sum((x >> k) & 1 for k in range(q))
    fact = np.array([float(math.factorial(d)) for d in range(q + 1)])
    # every vertex carries the same load: sum over t != s of (d(s, t) - 1) = q 2^(q-1) - (2^q - 1)
    return adjacency(n, [(v, v ^ (1 << k)) for v in range(n) for k in range(q) if v < v ^ (1 << k)]), dist, fact[dist], \
        np.full(n, q * 2.0 ** (q - 1) - (n - 1.0))


KNOWN = {"single_vertex": lambda: (sp.csr_matrix((1, 1)), np.zeros((1, 1), dtype=int), np.ones((1, 1)), np.zeros(1)),
         "one_edge": lambda: path_graph(2), "path_3": lambda: path_graph(3), "path_64": lambda: path_graph(64),
         "path_65": lambda: path_graph(65), "path_513": lambda: path_graph(513), "star_300": lambda: star_graph(300),
         "complete_20": lambda: complete_graph(20), "cycle_64": lambda: cycle_graph(64), "grid_8x8": lambda: grid_graph(8),
         "hypercube_10": lambda: hypercube_graph(10)}


@pytest.mark.parametrize("name", list(KNOWN))
def test_known_answers(pkg, name):
    A, dist, paths, bc_ref = KNOWN[name]()
    n = A.shape[0]
    eng = engine_of(pkg, A)
    D, P, info = eng.bfs(np.arange(n), paths=True)
    assert np.array_equal(D, dist) and np.array_equal(P, paths)
    assert np.array_equal(info["ecc"], dist.max(axis=1)) and (info["reached"] == n).all()
    assert np.array_equal(info["sum_dist"], dist.sum(axis=1))
    harm = np.array([np.sum(1.0 / row[row > 0]) for row in dist])
    assert (np.abs(info["harmonic"] - harm) <= n * EPS * harm).all()
    bc, binfo = eng.betweenness_raw(None)
    assert binfo["ns"] == n and binfo["batches"] == (n + 15) // 16 and binfo["max_level"] == dist.max()
    assert_bc_close(bc, bc_ref, bc_bound(A, np.arange(n), int(dist.max())))
    eng.close()


# ---- 2. fixtures ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=GOLDEN_IDS)
def test_fixtures_against_the_restatement(pkg, path):
    A, src, ref = fixture_case(path)
    eng = engine_of(pkg, A)
    D, _, info, _ = check_against(eng, A, src, ref)
    if os.path.basename(path) == "rmat_n4096.npz":      # 1 204 components: sources without an edge, unreachable vertices
        assert (info["reached"] == 1).any() and (D == -1).any() and (info["reached"] > 1000).any()
        lonely = int(np.flatnonzero(info["reached"] == 1)[0])
        assert info["ecc"][lonely] == 0 and info["harmonic"][lonely] == 0.0 and np.count_nonzero(D[lonely] == 0) == 1
    eng.close()


def test_er_n1000_every_vertex_against_networkx(pkg):
    A = load_fixture(golden("er_n1000"))
    n = A.shape[0]
    G = nx.from_scipy_sparse_array(A)
    eng = engine_of(pkg, A)
    D, info = eng.bfs(np.arange(n))
    bound = bc_bound(A, np.arange(n), int(D.max())) + 4 * EPS      # + the scaling's roundings
    raw = nx.betweenness_centrality(G, normalized=False)
    raw = np.array([raw[v] for v in range(n)])
    assert_bc_close(eng.betweenness(normalized=False), raw, bound)
    assert_bc_close(eng.betweenness(), raw * 2.0 / ((n - 1) * (n - 2)), bound)
    # k = 100: the sample is numpy's, so networkx is given the same sources and networkx 3.4's scale is applied here
    picked = np.random.default_rng(0).choice(n, size=100, replace=False)
    sub = nx.betweenness_centrality_subset(G, [int(s) for s in picked], list(G), normalized=False)
    sub = 2.0 * np.array([sub[v] for v in range(n)])
    bound_k = bc_bound(A, picked, int(D.max())) + 4 * EPS
    assert_bc_close(eng.betweenness(k=100, seed=0), sub * (n / 100.0) / ((n - 1) * (n - 2)), bound_k)
    assert_bc_close(eng.betweenness(k=100, seed=0, normalized=False), sub * 0.5 * (n / 100.0), bound_k)
    assert_bc_close(eng.betweenness(sources=picked), sub * (n / 100.0) / ((n - 1) * (n - 2)), bound_k)
    # closeness and harmonic centrality of every vertex, from the counts alone
    close, harm = nx.closeness_centrality(G, wf_improved=True), nx.harmonic_centrality(G)
    close, harm = np.array([close[v] for v in range(n)]), np.array([harm[v] for v in range(n)])
    assert (np.abs(eng.closeness() - close) <= n * EPS * close).all()
    assert (np.abs(eng.harmonic() - harm) <= n * EPS * harm).all()
    assert np.array_equal(eng.closeness(picked), eng.closeness()[picked])
    eng.close()


# ---- 3. batch shapes ------------------------------------------------------------------------------------------------------
def test_batch_shapes_bit_for_bit(pkg):
    A, src, _ = fixture_case(golden("rmat_n3000_skew"))
    eng = engine_of(pkg, A)
    pool = np.concatenate([src[:32], src[5:6]])         # 33 sources, one of them twice
    single = {}
    for s in set(int(s) for s in pool):
        D, P, info = eng.bfs([s], paths=True)
        single[s] = (D[0], P[0], {k: info[k][0] for k in SCALARS}, eng.betweenness_raw([s])[0])
    for ns in (1, 2, 3, 5, 16, 17, 33):
        pick = pool[-ns:]                               # ends with the duplicate's second copy; 33 holds both
        for _ in range(2):                              # ... and the same again
            D, P, info = eng.bfs(pick, paths=True)
            acc = np.zeros(A.shape[0])
            for i, s in enumerate(int(s) for s in pick):
                assert np.array_equal(D[i], single[s][0]) and np.array_equal(P[i], single[s][1]), (ns, s)
                for k in SCALARS:
                    assert info[k][i] == single[s][2][k], (ns, s, k)
                acc = acc + single[s][3]
            assert np.array_equal(eng.betweenness_raw(pick)[0], acc), ns
    eng.close()


# ---- 4. long rows, self loops, hand-over forms ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["star_ring_n1500", "rmat_n3000_skew"])
def test_long_rows_forced(pkg, name):
    A, src, ref = fixture_case(golden(name))
    assert np.diff(A.indptr).max() > 64
    eng = engine_of(pkg, A, multi_row_chunk=8)          # every row of more than 8 entries in chunks
    check_against(eng, A, src, ref)
    eng.close()


def test_self_loops_change_nothing(pkg):
    A, src, _ = fixture_case(golden("er_n1000"))
    n = A.shape[0]
    coo = sp.triu(A).tocoo()
    loops = np.unique(np.concatenate([src[:10], np.arange(0, n, 7)]))
    out = []
    for extra in (np.zeros(0, dtype=np.int64), loops):
        eng = pkg.Engine(0)
        eng.set_graph_edges(n, np.concatenate([coo.row, extra]), np.concatenate([coo.col, extra]))
        assert eng.info()["nnz"] == A.nnz + len(extra)
        D, P, info = eng.bfs(src, paths=True)
        out.append((D, P, info, eng.betweenness_raw(src)[0]))
        eng.close()
    (D0, P0, i0, b0), (D1, P1, i1, b1) = out
    assert np.array_equal(D0, D1) and np.array_equal(P0, P1) and np.array_equal(b0, b1)
    for k in SCALARS:
        assert np.array_equal(i0[k], i1[k]), k


def test_hand_over_form_does_not_matter(pkg):
    A, src, ref = fixture_case(golden("er_n4000_deg20"))
    out = []
    for pb in (1, 0):
        eng = engine_of(pkg, A, propagation_blocking=pb)
        D, P, info = eng.bfs(src, paths=True)
        out.append((D, P, info, eng.betweenness_raw(src)[0]))
        eng.close()
    (D0, P0, i0, b0), (D1, P1, i1, b1) = out
    assert np.array_equal(D0, ref["dist"]) and np.array_equal(D0, D1) and np.array_equal(P0, P1) and np.array_equal(b0, b1)
    for k in SCALARS:
        assert np.array_equal(i0[k], i1[k]), k


# ---- 5. isolation ---------------------------------------------------------------------------------------------------------
def test_a_chunked_decomposition_is_left_alone(pkg):
    A, src, _ = fixture_case(golden("er_n1000"))
    x0 = np.random.default_rng(8).standard_normal(A.shape[0])
    eng = engine_of(pkg, A)
    a_ref, b_ref, Q_ref, _, _ = eng.lanczos(x0, 20)
    eng.lanczos_prepare(x0, 20)
    eng.lanczos_run_steps(7)
    eng.bfs(src[:5])
    eng.betweenness_raw(src[:20])
    assert eng.lanczos_progress() == (7, 20)
    eng.lanczos_run_steps(13)
    a, b, Q = eng.lanczos_fetch(20, want_q=True)
    assert np.array_equal(a, a_ref) and np.array_equal(b, b_ref) and np.array_equal(Q, Q_ref)
    eng.close()


def test_the_resident_bases_are_left_alone(pkg):
    A, src, _ = fixture_case(golden("rmat_n3000_skew"))
    n = A.shape[0]
    rng = np.random.default_rng(9)
    x0, X0 = rng.standard_normal(n), rng.standard_normal((3, n))
    t, T = rng.standard_normal(12), rng.standard_normal((3, 12))
    eng = engine_of(pkg, A)
    eng.lanczos(x0, 12, want_q=False)
    eng.lanczos_multi(X0, 12)
    ans, ans_m = eng.multout(t), eng.multout_multi(T)
    eng.bfs(src[:17], paths=True)
    eng.betweenness_raw(src[:17])
    assert np.array_equal(eng.multout(t), ans) and np.array_equal(eng.multout_multi(T), ans_m)
    # a kept probe basis
    alpha, beta, k_used, _ = eng.lanczos_probes(3, 0, 4, 12, keep_basis=True)
    Tp = pkg.slq_diag_coefficients(alpha, beta, k_used, n, 0.1, 0.0)
    diag = eng.probe_diag(Tp)
    eng.bfs(src[:3])
    eng.betweenness_raw(src[:3])
    assert np.array_equal(eng.probe_diag(Tp), diag) and np.array_equal(eng.multout(t), ans)
    eng.close()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------
def test_errors(pkg):
    L = pkg.lib()
    eng = pkg.Engine(0)
    eng.n = 4
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*no graph"):
        eng.bfs([0])
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*no graph"):
        eng.betweenness_raw([0])
    A, src, _ = fixture_case(golden("er_n1000"))
    n = A.shape[0]
    eng.close()
    eng = engine_of(pkg, A)
    bad = np.array([3, 5, n, 7], dtype=np.uint32)
    bc = np.zeros(n)
    assert L.lzx_bfs_multi(eng.h, 4, bad.ctypes.data_as(_u32p), None, None, None, None, None, None, None) == -1
    assert f"sources[2] = {n}" in L.lzx_last_error().decode()
    assert L.lzx_betweenness_f64(eng.h, 4, bad.ctypes.data_as(_u32p), bc.ctypes.data_as(_f64p), None) == -1
    assert f"sources[2] = {n}" in L.lzx_last_error().decode()
    assert L.lzx_betweenness_f64(eng.h, n - 1, None, bc.ctypes.data_as(_f64p), None) == -1
    assert f"ns must be n = {n}" in L.lzx_last_error().decode()
    assert L.lzx_bfs_multi(eng.h, 4, None, None, None, None, None, None, None, None) == -1
    assert L.lzx_betweenness_f64(eng.h, 4, bad.ctypes.data_as(_u32p), None, None) == -1
    assert L.lzx_bfs_multi(eng.h, 0, bad.ctypes.data_as(_u32p), None, None, None, None, None, None, None) == -1
    for call in (lambda: eng.bfs([n]), lambda: eng.bfs([]), lambda: eng.betweenness(k=0), lambda: eng.betweenness(k=3, sources=[1])):
        with pytest.raises(ValueError):
            call()
    eng.close()
    # the state cap: 16 columns x n x 20 bytes + n x 8 do not fit 16 n bytes; one column (padded to 2: 40 n + 8 n) does not either
    small = engine_of(pkg, A, bfs_state_bytes=16 * n)
    with pytest.raises(pkg.LzxError, match=r"\(-4\).*needs \d+ bytes"):
        small.betweenness_raw(src)
    with pytest.raises(pkg.LzxError, match=r"\(-4\).*needs \d+ bytes"):
        small.bfs(src[:1])
    x = np.random.default_rng(3).standard_normal(n)
    y = small.spmv(x)
    assert np.array_equal(small.spmv(x), y)
    small.close()
    roomy = engine_of(pkg, A, bfs_state_bytes=(20 * 16 + 8) * n + 4096)
    roomy.betweenness_raw(src)
    roomy.close()
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(A.indptr.astype(np.uint64), A.indices.astype(np.uint32))
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*communicator of 2"):
        grp.engines[0].bfs([0])
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*communicator of 2"):
        grp.engines[1].betweenness_raw([0])
    grp.close()
