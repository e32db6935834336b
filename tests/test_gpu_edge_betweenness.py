"""GPU: edge betweenness and endpoints on the device (include/lzx.h: lzx_brandes_f64; Engine.brandes_raw / edge_betweenness /
betweenness(endpoints=True)): known answers with every vertex a source, the golden fixtures against the numpy restatement of
tests/test_edge_betweenness_host.py and against networkx, every batch shape bit for bit, every number of lanes per row on the
graphs of tests/lanes_graphs.py, forced split rows, the ten smallest graphs, self loops, both hand-over forms, isolation from
the handle's other state, and the error paths.

Tolerances are those derived in tests/test_edge_betweenness_host.py: ebc within bc_bound + 2 * 2^-53 of the reference,
relative, entry by entry, and exactly 0 where the reference is 0; bc with flags = 0 is lzx_betweenness_f64's, bit for bit; the
flagged bc is that plus the endpoints' count, bit for bit."""
import ctypes
import functools
import os

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp

import lanes_graphs
from test_edge_betweenness_host import assert_close, assert_identities, brandes_edges, ebc_bound, edges_of_networkx
from test_paths_host import EPS, GOLDEN, GOLDEN_IDS, fixture_sources, load_fixture
from test_smallest_host import NAMES, small

pytestmark = pytest.mark.gpu

_u32p = ctypes.POINTER(ctypes.c_uint32)
_f64p = ctypes.POINTER(ctypes.c_double)


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
    A = sp.csr_matrix(M)
    A.sort_indices()
    return A


def entries(A):
    """(u, w) of every stored entry, in CSR order"""
    return np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), A.indices


def host_cnt(eng, src, n):
    """the endpoints' count from Engine.bfs: + 1 where a source reaches v from elsewhere, + reached - 1 at the source itself"""
    src = np.arange(n) if src is None else np.asarray(src, dtype=np.int64)
    D, info = eng.bfs(src)
    cnt = (D > 0).sum(axis=0).astype(np.int64)
    np.add.at(cnt, src, info["reached"].astype(np.int64) - 1)
    return cnt


def assert_flagged(eng, src, n, bc_plain):
    """bc with LZX_BRANDES_ENDPOINTS = bc_plain + cnt, bit for bit, and the flag leaves ebc alone"""
    bc, _, _ = eng.brandes_raw(src, want_edges=False, endpoints=True)
    assert np.array_equal(bc, bc_plain + host_cnt(eng, src, n).astype(np.float64))


@functools.lru_cache(maxsize=None)
def fixture_case(path):
    """(A, the 48 sources of the host test + vertex 0 + the vertex of largest degree, their restatement): once per fixture"""
    A = load_fixture(path)
    A.sort_indices()
    src = np.concatenate([fixture_sources(A.shape[0]), [0, int(np.argmax(np.diff(A.indptr)))]])
    return A, src, brandes_edges(A, src)


# ---- 1. known answers, every vertex a source ------------------------------------------------------------------------------
def path_case(n):
    A = adjacency(n, [(k, k + 1) for k in range(n - 1)])
    u, w = entries(A)
    i = np.minimum(u, w)
    return A, 2.0 * (i + 1) * (n - 1 - i), True


def hypercube(q):
    n = 1 << q
    return adjacency(n, [(v, v ^ (1 << k)) for v in range(n) for k in range(q) if v < v ^ (1 << k)])


def grid_case(m):
    n = m * m
    A = adjacency(n, [(k, k + 1) for k in range(n) if (k + 1) % m] + [(k, k + m) for k in range(n - m)])
    ref = nx.edge_betweenness_centrality(nx.from_scipy_sparse_array(A), normalized=False)
    return A, edges_of_networkx(A, ref), False


def constant_case(A, value, exact):
    return A, np.full(A.nnz, float(value)), exact


# name: (A, the expected ebc per stored entry, whether it is held to exactly)
KNOWN = {"single_vertex": lambda: constant_case(sp.csr_matrix((1, 1)), 0.0, True),
         "no_edge_5": lambda: constant_case(sp.csr_matrix((5, 5)), 0.0, True),
         "path_2": lambda: path_case(2), "path_3": lambda: path_case(3), "path_64": lambda: path_case(64),
         "path_65": lambda: path_case(65), "path_513": lambda: path_case(513),
         "star_300": lambda: constant_case(adjacency(300, [(0, k) for k in range(1, 300)]), 2.0 * 299, True),
         "complete_20": lambda: constant_case(adjacency(20, [(u, v) for u in range(20) for v in range(u)]), 2.0, True),
         # C_64: 2 * 64 * (64^2 / 4) units over 128 stored entries; the antipode's two paths give halves, which are exact
         "cycle_64": lambda: constant_case(adjacency(64, [(k, (k + 1) % 64) for k in range(64)]), 64.0 * 64.0 / 4.0, True),
         # Q_10: 2 * 1024 * (10 * 2^9) units over 10 * 1024 stored entries
         "hypercube_10": lambda: constant_case(hypercube(10), 1024.0, False),
         "grid_8x8": lambda: grid_case(8)}


@pytest.mark.parametrize("name", list(KNOWN))
def test_known_answers(pkg, name):
    A, ref, exact = KNOWN[name]()
    n = A.shape[0]
    eng = engine_of(pkg, A)
    bc, ebc, info = eng.brandes_raw(None)
    assert ebc.shape == (A.nnz,) and info["ns"] == n and info["batches"] == (n + 15) // 16
    if exact:
        assert np.array_equal(ebc, ref)
    else:
        assert_close(ebc, ref, ebc_bound(A, np.arange(n), info["max_level"]))
    bc_plain = eng.betweenness_raw(None)[0]
    assert np.array_equal(bc, bc_plain)
    if A.nnz == 0:
        assert not bc.any() and not ebc.any()
    assert_flagged(eng, None, n, bc_plain)
    eng.close()


# ---- 2. fixtures ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=GOLDEN_IDS)
def test_fixtures_against_the_restatement(pkg, path):
    A, src, ref = fixture_case(path)
    n = A.shape[0]
    eng = engine_of(pkg, A)
    bc, ebc, info = eng.brandes_raw(src)
    bound = ebc_bound(A, src, ref["max_level"])
    nz = ref["ebc"] > 0
    print("ebc: largest relative difference", float(np.max(np.abs(ebc - ref["ebc"])[nz] / ref["ebc"][nz])), "bound", bound,
          "sweeps", info["sweeps"], "sweep_ms", info["sweep_ms"], "edge_ms", info["edge_ms"])
    assert info["max_level"] == ref["max_level"] and info["ns"] == len(src) and info["batches"] == (len(src) + 15) // 16
    assert_close(ebc, ref["ebc"], bound)
    M = sp.csr_matrix((ebc, A.indices, A.indptr), shape=A.shape)
    assert (M != M.T).nnz == 0 and not M.diagonal().any()
    # bc with flags = 0 is lzx_betweenness_f64's, with and without ebc; ebc does not depend on bc being asked for
    bc_plain = eng.betweenness_raw(src)[0]
    assert np.array_equal(bc, bc_plain) and np.array_equal(eng.brandes_raw(src, want_edges=False)[0], bc_plain)
    none, ebc_alone, _ = eng.brandes_raw(src, want_bc=False)
    assert none is None and np.array_equal(ebc_alone, ebc)
    flagged, ebc_flagged, _ = eng.brandes_raw(src, endpoints=True)
    assert np.array_equal(flagged, bc_plain + ref["cnt"].astype(np.float64)) and np.array_equal(ebc_flagged, ebc)
    assert np.array_equal(host_cnt(eng, src, n), ref["cnt"])
    assert_identities(A, dict(ebc=ebc, bc=bc, cnt=ref["cnt"], sum_dist=ref["sum_dist"]), bound)
    if os.path.basename(path) == "rmat_n4096.npz":      # sources without an edge, unreachable vertices
        assert (ref["reached"] == 1).any() and (ref["dist"] == -1).any() and (ref["reached"] > 1000).any()
    eng.close()


# ---- 3. er_n1000, every vertex, against networkx ----------------------------------------------------------------------------
def test_er_n1000_edges_against_networkx(pkg):
    A = load_fixture(golden("er_n1000"))
    A.sort_indices()
    n = A.shape[0]
    G = nx.from_scipy_sparse_array(A)
    eng = engine_of(pkg, A)
    D, _ = eng.bfs(np.arange(n))
    bound = ebc_bound(A, np.arange(n), int(D.max())) + 4 * EPS      # + the scaling's roundings
    # one run of networkx serves both scalings: normalized=False is its raw sum times 0.5, exactly, and normalized=True is the
    # raw sum times 1 / (n (n - 1)), the one rounded product formed here
    raw = edges_of_networkx(A, nx.edge_betweenness_centrality(G, normalized=False))
    for normalized, ref in ((False, 0.5 * raw), (True, raw * (1.0 / (n * (n - 1))))):
        M = eng.edge_betweenness(normalized=normalized)
        assert sp.issparse(M) and M.dtype == np.float64 and M.shape == (n, n)
        assert np.array_equal(M.indptr, A.indptr) and np.array_equal(M.indices, A.indices)
        assert_close(M.data, ref, bound)
    # k = 100: the sample is numpy's, so networkx is given the same sources and networkx 3.4's scale is applied here
    picked = np.random.default_rng(0).choice(n, size=100, replace=False)
    sub = edges_of_networkx(A, nx.edge_betweenness_centrality_subset(G, [int(s) for s in picked], list(G), normalized=False))
    bound_k = ebc_bound(A, picked, int(D.max())) + 4 * EPS
    assert_close(eng.edge_betweenness(k=100, seed=0).data, sub * (n / 100.0) / (n * (n - 1)), bound_k)
    assert_close(eng.edge_betweenness(k=100, seed=0, normalized=False).data, sub * 0.5 * (n / 100.0), bound_k)
    assert_close(eng.edge_betweenness(sources=picked).data, sub * (n / 100.0) / (n * (n - 1)), bound_k)
    for call in (lambda: eng.edge_betweenness(k=0), lambda: eng.edge_betweenness(k=3, sources=[1])):
        with pytest.raises(ValueError):
            call()
    eng.close()


def test_er_n1000_endpoints_against_networkx(pkg):
    A = load_fixture(golden("er_n1000"))
    n = A.shape[0]
    G = nx.from_scipy_sparse_array(A)
    eng = engine_of(pkg, A)
    D, _ = eng.bfs(np.arange(n))
    bound = ebc_bound(A, np.arange(n), int(D.max())) + 4 * EPS
    # as above: networkx's two scalings of one raw sum, 0.5 and 1 / (n (n - 1))
    ref = nx.betweenness_centrality(G, normalized=False, endpoints=True)
    raw = 2.0 * np.array([ref[v] for v in range(n)])
    assert_close(eng.betweenness(normalized=False, endpoints=True), 0.5 * raw, bound)
    assert_close(eng.betweenness(endpoints=True), raw * (1.0 / (n * (n - 1))), bound)
    picked = np.random.default_rng(0).choice(n, size=100, replace=False)
    flagged = eng.brandes_raw(picked, want_edges=False, endpoints=True)[0]
    assert np.array_equal(eng.betweenness(k=100, seed=0, endpoints=True), flagged * (1.0 / (n * (n - 1)) * n / 100))
    assert np.array_equal(eng.betweenness(endpoints=False), eng.betweenness())
    eng.close()


# ---- 4. batch shapes ------------------------------------------------------------------------------------------------------
def test_batch_shapes_bit_for_bit(pkg):
    A, src, _ = fixture_case(golden("rmat_n3000_skew"))
    n = A.shape[0]
    eng = engine_of(pkg, A)
    pool = np.concatenate([src[:32], src[5:6]])         # 33 sources, one of them twice
    single = {s: eng.brandes_raw([s]) for s in set(int(s) for s in pool)}
    for ns in (1, 2, 3, 5, 16, 17, 33):
        pick = pool[-ns:]                               # ends with the duplicate's second copy; 33 holds both
        acc, bc_acc = np.zeros(A.nnz), np.zeros(n)
        for s in (int(s) for s in pick):
            acc, bc_acc = acc + single[s][1], bc_acc + single[s][0]
        cnt = host_cnt(eng, pick, n).astype(np.float64)
        for _ in range(2):                              # ... and the same again
            bc, ebc, _ = eng.brandes_raw(pick)
            assert np.array_equal(ebc, acc) and np.array_equal(bc, bc_acc), ns
            flagged, ebc_f, _ = eng.brandes_raw(pick, endpoints=True)
            assert np.array_equal(flagged, bc_acc + cnt) and np.array_equal(ebc_f, acc), ns
    eng.close()


# ---- 5. row-length and lane boundaries --------------------------------------------------------------------------------------
SETTINGS = (None, 4, 8, 16, 32, 64)          # graph_lanes: the rule, then every width (64 runs the widest kernel, 32)


def across_lanes(pkg, A, src, **options):
    """one call per setting of graph_lanes: all bit-identical, the first returned"""
    first = None
    for lanes in SETTINGS:
        eng = engine_of(pkg, A, **(options if lanes is None else dict(options, graph_lanes=lanes)))
        bc, ebc, _ = eng.brandes_raw(src)
        assert eng.shape("graph_lanes_rows") == (lanes_graphs.rule(A) if lanes is None else min(lanes, 32)), lanes
        if first is None:
            first = (bc, ebc)
        assert np.array_equal(bc, first[0]) and np.array_equal(ebc, first[1]), lanes
        eng.close()
    return first


@pytest.mark.parametrize("residue,reverse", [(0, False), (63, True)], ids=["ladder_n%64=0", "ladder_n%64=63_reversed"])
def test_every_lane_width_on_the_ladder(pkg, residue, reverse):
    A = lanes_graphs.ladder(residue, reverse)
    lengths = set(np.diff(A.indptr).tolist())
    assert {0, 1, 3, 2049} <= lengths
    src = np.random.default_rng(5).choice(A.shape[0], size=33, replace=False)
    ref = brandes_edges(A, src)
    bc, ebc = across_lanes(pkg, A, src)
    bound = ebc_bound(A, src, ref["max_level"])
    assert_close(ebc, ref["ebc"], bound)
    assert_close(bc, ref["bc"], bound)


@pytest.mark.parametrize("name", ["star_ring_n1500", "rmat_n3000_skew"])
def test_every_lane_width_with_split_rows(pkg, name):
    A, src, ref = fixture_case(golden(name))
    assert np.diff(A.indptr).max() > 64
    bc, ebc = across_lanes(pkg, A, src, multi_row_chunk=8)          # every row of more than 8 entries in chunks, both passes
    bound = ebc_bound(A, src, ref["max_level"])
    assert_close(ebc, ref["ebc"], bound)
    assert_close(bc, ref["bc"], bound)
    eng = engine_of(pkg, A)
    plain = eng.brandes_raw(src)
    eng.close()
    assert np.array_equal(plain[1] == 0.0, ebc == 0.0)


# ---- 6. the ten smallest graphs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_smallest_graphs(pkg, name):
    s = small(name)
    ref = brandes_edges(s.A, np.arange(s.n))
    eng = pkg.Engine(0)
    eng.set_graph_csr(s.rp, s.ci)
    bc, ebc, info = eng.brandes_raw(None)
    assert ebc.shape == (s.nnz,) and np.array_equal(ebc, ref["ebc"]) and np.array_equal(bc, ref["bc"])
    flagged, _, _ = eng.brandes_raw(None, endpoints=True)
    assert np.array_equal(flagged, ref["bc"] + ref["cnt"].astype(np.float64))
    assert np.array_equal(eng.brandes_raw(None, want_bc=False)[1], ref["ebc"])
    if name in ("v1", "loop1", "v2_empty", "empty65"):
        assert not ebc.any() and not bc.any() and not flagged.any() and info["max_level"] == 0
    M = eng.edge_betweenness(normalized=False)
    assert M.shape == (s.n, s.n) and np.array_equal(M.data, 0.5 * ref["ebc"])
    eng.close()


# ---- 7. self loops, hand-over forms -----------------------------------------------------------------------------------------
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
        bc, ebc, _ = eng.brandes_raw(src)
        flagged = eng.brandes_raw(src, want_edges=False, endpoints=True)[0]
        rp, ci = eng.get_graph_csr()
        u = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
        w = ci.astype(np.int64)
        assert not ebc[u == w].any()
        order = np.lexsort((w[u != w], u[u != w]))
        out.append((bc, flagged, u[u != w][order], w[u != w][order], ebc[u != w][order]))
        eng.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_hand_over_form_does_not_matter(pkg):
    A, src, ref = fixture_case(golden("er_n4000_deg20"))
    out = []
    for pb in (1, 0):
        eng = engine_of(pkg, A, propagation_blocking=pb)
        out.append(eng.brandes_raw(src, endpoints=True)[:2])
        eng.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert_close(out[0][1], ref["ebc"], ebc_bound(A, src, ref["max_level"]))


# ---- 8. isolation and errors ------------------------------------------------------------------------------------------------
def test_a_chunked_decomposition_is_left_alone(pkg):
    A, src, _ = fixture_case(golden("er_n1000"))
    x0 = np.random.default_rng(8).standard_normal(A.shape[0])
    eng = engine_of(pkg, A)
    a_ref, b_ref, Q_ref, _, _ = eng.lanczos(x0, 20)
    eng.lanczos_prepare(x0, 20)
    eng.lanczos_run_steps(7)
    eng.brandes_raw(src[:20], endpoints=True)
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
    eng.brandes_raw(src[:17], endpoints=True)
    assert np.array_equal(eng.multout(t), ans) and np.array_equal(eng.multout_multi(T), ans_m)
    # a kept probe basis
    alpha, beta, k_used, _ = eng.lanczos_probes(3, 0, 4, 12, keep_basis=True)
    Tp = pkg.slq_diag_coefficients(alpha, beta, k_used, n, 0.1, 0.0)
    diag = eng.probe_diag(Tp)
    eng.brandes_raw(src[:3])
    assert np.array_equal(eng.probe_diag(Tp), diag) and np.array_equal(eng.multout(t), ans)
    eng.close()


def test_errors(pkg):
    L = pkg.lib()
    A, src, _ = fixture_case(golden("er_n1000"))
    n, nnz = A.shape[0], A.nnz
    bad = np.array([3, 5, n, 7], dtype=np.uint32)
    bc, ebc = np.zeros(n), np.zeros(nnz)
    sp_, bp, ep = bad.ctypes.data_as(_u32p), bc.ctypes.data_as(_f64p), ebc.ctypes.data_as(_f64p)
    eng = pkg.Engine(0)
    assert L.lzx_brandes_f64(eng.h, 1, sp_, 0, bp, ep, None) == -3
    assert "lzx_brandes_f64" in L.lzx_last_error().decode() and "no graph" in L.lzx_last_error().decode()
    eng.close()
    eng = engine_of(pkg, A)
    for call, word in [(lambda: L.lzx_brandes_f64(eng.h, 4, sp_, 0, bp, ep, None), f"sources[2] = {n}"),
                       (lambda: L.lzx_brandes_f64(eng.h, n - 1, None, 0, bp, ep, None), f"ns must be n = {n}"),
                       (lambda: L.lzx_brandes_f64(eng.h, 2, sp_, 0, None, None, None), "null bc and null ebc"),
                       (lambda: L.lzx_brandes_f64(eng.h, 2, sp_, 1, None, ep, None), "LZX_BRANDES_ENDPOINTS with null bc"),
                       (lambda: L.lzx_brandes_f64(eng.h, 2, sp_, 4, bp, ep, None), "unknown flag"),
                       (lambda: L.lzx_brandes_f64(eng.h, 0, sp_, 0, bp, ep, None), "ns == 0")]:
        assert call() == -1, word
        assert "lzx_brandes_f64" in L.lzx_last_error().decode() and word in L.lzx_last_error().decode(), word
    for call in (lambda: eng.brandes_raw([n]), lambda: eng.brandes_raw([]), lambda: eng.betweenness(k=0, endpoints=True)):
        with pytest.raises(ValueError):
            call()
    eng.close()
    # the state cap: nothing of this call fits 16 n bytes
    small_cap = engine_of(pkg, A, bfs_state_bytes=16 * n)
    for kw in (dict(), dict(want_bc=False), dict(want_edges=False, endpoints=True)):
        with pytest.raises(pkg.LzxError, match=r"\(-4\).*lzx_brandes_f64.*needs \d+ bytes"):
            small_cap.brandes_raw(src[:1], **kw)
    x = np.random.default_rng(3).standard_normal(n)
    y = small_cap.spmv(x)
    assert np.array_equal(small_cap.spmv(x), y)
    small_cap.close()
    # the documented arena: lzx_betweenness_f64's 20 B n + 8 n, + 8 B n for delta, + 8 nnz for ebc, + 8 n for cnt
    arena = (20 * 16 + 8) * n + 8 * 16 * n + 8 * nnz + 8 * n
    roomy = engine_of(pkg, A, bfs_state_bytes=arena + 4096)
    roomy.brandes_raw(src, endpoints=True)
    roomy.close()
    tight = engine_of(pkg, A, bfs_state_bytes=arena - 8)
    with pytest.raises(pkg.LzxError, match=r"\(-4\).*needs \d+ bytes"):
        tight.brandes_raw(src, endpoints=True)
    tight.close()
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(A.indptr.astype(np.uint64), A.indices.astype(np.uint32))
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*communicator of 2"):
        grp.engines[1].brandes_raw([0], want_edges=False)
    grp.close()
