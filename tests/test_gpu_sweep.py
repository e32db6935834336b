"""GPU: sweep cuts on the device (include/lzx.h: lzx_sweep_cut; Engine.sweep_cut_raw / sweep_cut / cut_size / volume /
conductance / edge_expansion / spectral_bisection / local_cluster) against the numpy restatement of tests/test_sweep_host.py
(which that file pins to networkx): the golden fixtures and small graphs in both directions, with both objectives, with and
without the per-degree key, on float, many-ties, constant and signed-zero / infinite scores; self loops; both launches of the
edge sweep, forced and unforced; every width; the window; every output alone; isolation from the handle's other state; the
errors; a matrix that is not symmetric; and the wrappers.

Everything is equality, except lambda_2 against numpy, which is within the eigensolver's own residual bound."""
import ctypes
import functools
import itertools

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp

from test_core_host import GOLDEN_IDS
from test_gpu_core import complete_graph, engine_of, golden, lanes_per_row
from test_truss_host import adjacency, two_hubs
from test_communities_host import SMALL, graph_of, star_graph
from test_sweep_host import ASCENDING, EXPANSION, PER_DEGREE, RESULT_KEYS, fiedler_vector, fixture_graph, lopsided_barbell, many_ties, result_of, sweep_ref

pytestmark = pytest.mark.gpu

_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_f64p = ctypes.POINTER(ctypes.c_double)
LZX_OK, LZX_ERR_ARG, LZX_ERR_LIMIT = 0, -1, -6
INF = float("inf")
NONE = dict(k=0, cut=0, vol=0, den=0, value=INF)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name in GOLDEN_IDS:
        return fixture_graph(golden(name))
    makers = dict(SMALL, complete_200=lambda: complete_graph(200), star_4096=lambda: star_graph(4096), two_hubs=two_hubs,
                  empty_graph=lambda: sp.csr_matrix((5, 5)), single_vertex=lambda: sp.csr_matrix((1, 1)), one_edge=lambda: adjacency(2, [(0, 1)]),
                  k8_k12=lopsided_barbell)
    A = sp.csr_matrix(makers[name]())
    A.sort_indices()
    return A


def scores_of(n, seed=3):
    """(4, n): a random float score, a many-ties integer score, a constant, and one of -0.0, +0.0, +inf, -inf and +-1"""
    rng = np.random.default_rng(seed)
    special = np.array([-0.0, 0.0, np.inf, -np.inf, 1.0, -1.0])[rng.integers(0, 6, n)]
    return np.vstack([rng.standard_normal(n), many_ties(n), np.full(n, 2.5), special])


def flags_of(kw):
    return (ASCENDING if kw.get("ascending") else 0) | (PER_DEGREE if kw.get("per_degree") else 0) | \
           (EXPANSION if kw.get("objective") == "expansion" else 0)


def run(eng, S, **kw):
    """(order, cut, vol, results, info) of one call with every output"""
    order, cut, vol, results, info = eng.sweep_cut_raw(S, want_order=True, want_profile=True, **kw)
    assert order.dtype == np.uint32 and cut.dtype == np.uint64 and vol.dtype == np.uint64
    return order, cut, vol, results, info


@functools.lru_cache(maxsize=None)
def ref(name, column, seed, flags, k_min=0, k_max=0):
    """the restatement for one column of scores_of, computed once and shared (read-only)"""
    A = graph(name)
    return sweep_ref(A, scores_of(A.shape[0], seed)[column], flags, k_min, k_max)


def assert_column(got, c, r):
    order, cut, vol, results, info = got
    assert np.array_equal(order[c], r["order"]) and np.array_equal(cut[c], r["cut"]) and np.array_equal(vol[c], r["vol"])
    assert results[c] == result_of(r), (results[c], result_of(r))
    assert info["entries"] == r["M"]


COMBOS = [dict(ascending=a, per_degree=p, objective=o) for a, p, o in itertools.product((False, True), (False, True), ("conductance", "expansion"))]
SMALL_NAMES = list(SMALL) + ["empty_graph", "single_vertex", "one_edge"]


# ---- 1. fixtures and small graphs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL_NAMES)
def test_small_graphs(pkg, name):
    A = graph(name)
    n = A.shape[0]
    eng = engine_of(pkg, A)
    for kw in COMBOS:
        got = run(eng, scores_of(n), **kw)
        assert got[4]["ns"] == 4 and got[4]["width"] == 4
        for c in range(4):
            assert_column(got, c, ref(name, c, 3, flags_of(kw)))
        if name == "k5_k10_and_7_isolated" and kw["per_degree"]:
            assert (got[0][:, 15:] == np.arange(15, 22)).all()               # the isolated vertices last, whatever their score
        if name == "single_vertex" or (name == "empty_graph" and kw["objective"] == "conductance"):
            assert got[3] == [NONE] * 4 and (got[1] == 0).all()                  # no admissible k (but min(k, n - k) > 0 on 5 vertices)
        if kw == COMBOS[0]:
            assert (got[0][2] == np.arange(n)).all()                         # a constant score: the order is the ids
    eng.close()


@pytest.mark.parametrize("name", GOLDEN_IDS)
def test_fixtures_against_the_restatement(pkg, name):
    A = graph(name)
    n = A.shape[0]
    eng = engine_of(pkg, A)
    for kw in (COMBOS[0], COMBOS[7]):
        got = run(eng, scores_of(n), **kw)
        for c in range(4):
            assert_column(got, c, ref(name, c, 3, flags_of(kw)))
        assert (got[1][:, n - 1] == 0).all() and (got[2][:, n - 1] == A.nnz).all()
    members, value, result = eng.sweep_cut(many_ties(n))
    assert value == nx.conductance(graph_of(A), members.tolist()) and result == result_of(ref(name, 1, 3, 0))
    eng.close()


def test_self_loops_change_nothing(pkg):
    A = graph("er_n1000")
    n = A.shape[0]
    loops = np.zeros(n)
    loops[::20] = 1.0
    B = sp.csr_matrix(A + sp.diags(loops))
    B.sort_indices()
    assert B.nnz == A.nnz + 50
    plain, looped = engine_of(pkg, A), engine_of(pkg, B)
    assert looped.info()["nnz"] == A.nnz + 50
    for kw in (COMBOS[0], COMBOS[2], COMBOS[7]):
        a, b = run(plain, scores_of(n), **kw), run(looped, scores_of(n), **kw)
        assert all(np.array_equal(a[i], b[i]) for i in range(3)) and a[3] == b[3] and a[4]["entries"] == b[4]["entries"] == A.nnz
        assert_column(b, 0, ref("er_n1000", 0, 3, flags_of(kw)))
    plain.close()
    looped.close()


# ---- 2. both launches of the edge sweep ---------------------------------------------------------------------------------------
# (graph, sweep_long_row or None, rows for the group launch, rows for the long-row launch)
LAUNCHES = [("star_4096", None, True, True), ("two_hubs", None, True, True), ("complete_200", None, True, False), ("rmat_n3000_skew", 4, True, True)]


@pytest.mark.parametrize("name,long_row,short_rows,long_rows", LAUNCHES, ids=[f"{c[0]}-{c[1]}" for c in LAUNCHES])
def test_both_sweep_launches(pkg, name, long_row, short_rows, long_rows):
    """A row is swept by a group of lanes when it has at most sweep_long_row entries (default: 64 times the lanes per row), by a
    workgroup when it has more, in a launch that runs only when such a row exists.  Which launch gets rows is asserted from the
    row lengths:
      star_4096            4 lanes, threshold 256: the hub by the long-row launch
      two_hubs             4 lanes, threshold 256: the two rows of 311 entries by the long-row launch
      complete_200         the group launch alone
      rmat_n3000_skew, 4   both
    Each is compared with the restatement at widths 1, 4 and 16, and the forced run with the unforced one."""
    A = graph(name)
    n = A.shape[0]
    lengths = np.diff(A.indptr)
    threshold = 64 * lanes_per_row(A) if long_row is None else long_row
    print(name, "threshold", threshold, "rows above it", int((lengths > threshold).sum()), "longest row", int(lengths.max()))
    assert bool((lengths <= threshold).any()) == short_rows and bool((lengths > threshold).any()) == long_rows
    if name in ("star_4096", "two_hubs"):
        assert lanes_per_row(A) == 4
    S = np.vstack([scores_of(n, seed) for seed in (3, 4, 5, 6)])
    unforced = engine_of(pkg, A)
    first = {}
    for ns in (1, 4, 16):
        for kw in (COMBOS[0], COMBOS[6]):
            got = first[ns, flags_of(kw)] = run(unforced, S[:ns], **kw)
            for c in range(ns):
                assert_column(got, c, ref(name, c % 4, 3 + c // 4, flags_of(kw)))
    unforced.close()
    if long_row is not None:
        forced = engine_of(pkg, A, sweep_long_row=long_row)
        for (ns, flags), want in first.items():
            got = run(forced, S[:ns], **(COMBOS[0] if flags == 0 else COMBOS[6]))
            assert all(np.array_equal(got[i], want[i]) for i in range(3)) and got[3] == want[3]
        forced.close()


# ---- 3. widths ----------------------------------------------------------------------------------------------------------------
def test_every_width_and_a_column_s_place_in_the_batch(pkg):
    name = "rmat_n4096"
    A = graph(name)
    n = A.shape[0]
    S = np.vstack([scores_of(n, seed) for seed in (3, 4, 5, 6)])
    eng = engine_of(pkg, A)
    for ns, width in ((1, 1), (2, 2), (3, 4), (5, 8), (16, 16)):
        got = run(eng, S[:ns], per_degree=True)
        assert (got[4]["ns"], got[4]["width"]) == (ns, width)
        for c in range(ns):
            assert_column(got, c, ref(name, c % 4, 3 + c // 4, PER_DEGREE))
    best = (pkg.LzxSweepResult * 17)()
    wide = np.ascontiguousarray(np.vstack([S, S[:1]]))
    assert eng.L.lzx_sweep_cut(eng.h, 17, wide.ctypes.data_as(_f64p), 0, 0, 0, None, None, None, best, None) == LZX_ERR_LIMIT
    assert "17 columns" in eng.L.lzx_last_error().decode()
    # column 7 alone, first and last in a batch of 16
    alone = run(eng, S[7])
    others = np.delete(S, 7, axis=0)
    first, last = run(eng, np.vstack([S[7:8], others])), run(eng, np.vstack([others, S[7:8]]))
    for got, c in ((first, 0), (last, 15)):
        assert all(np.array_equal(got[i][c], alone[i][0]) for i in range(3)) and got[3][c] == alone[3][0]
    assert_column(alone, 0, ref(name, 3, 4, 0))
    eng.close()


# ---- 4. the window ------------------------------------------------------------------------------------------------------------
def test_the_window_and_the_set_functions(pkg):
    A = graph("er_n1000")
    n = A.shape[0]
    G = graph_of(A)
    eng = engine_of(pkg, A)
    rng = np.random.default_rng(12)
    for size in (1, 2, 37, n // 2, n - 1):
        S = np.sort(rng.choice(n, size, replace=False))
        ind = np.zeros(n)
        ind[S] = 1.0
        order, _, _, results, _ = eng.sweep_cut_raw(ind, k_min=size, k_max=size)
        assert np.array_equal(np.sort(order[0, :size]), S) and results[0] == result_of(sweep_ref(A, ind, 0, size, size))
        mask = ind != 0
        for S_in in (S, S.tolist(), mask):
            assert eng.cut_size(S_in) == nx.cut_size(G, S.tolist()) and eng.volume(S_in) == nx.volume(G, S.tolist())
            assert eng.conductance(S_in) == nx.conductance(G, S.tolist()) and eng.edge_expansion(S_in) == nx.edge_expansion(G, S.tolist())
    # no admissible k: the whole graph, and a set of isolated vertices
    s = rng.standard_normal(n)
    for kw in (dict(), dict(objective="expansion")):
        assert eng.sweep_cut_raw(s, k_min=n, k_max=n, **kw)[3] == [NONE]
    assert eng.conductance(np.arange(n)) == INF and eng.cut_size(np.arange(n)) == 0 and eng.volume(np.arange(n)) == A.nnz
    assert eng.cut_size([]) == 0 and eng.conductance([]) == INF
    win = eng.sweep_cut_raw(s, k_min=100, k_max=300)[3][0]
    assert win == result_of(sweep_ref(A, s, 0, 100, 300)) and 100 <= win["k"] <= 300
    eng.close()
    iso = engine_of(pkg, graph("k5_k10_and_7_isolated"))
    assert iso.conductance([15, 16]) == INF and iso.volume([15, 16]) == 0 and iso.edge_expansion([15, 16]) == 0.0
    assert iso.sweep_cut_raw(np.arange(22.0), k_min=2, k_max=2)[3] == [NONE]          # 21 and 20: isolated, den = 0
    iso.close()


# ---- 5. outputs ---------------------------------------------------------------------------------------------------------------
def test_every_output_alone_and_repeats(pkg):
    name = "er_n4000_deg20"
    A = graph(name)
    n = A.shape[0]
    S = np.ascontiguousarray(scores_of(n)[:2])
    r = [ref(name, c, 3, 0) for c in range(2)]
    eng = engine_of(pkg, A)

    def call(order=None, cut=None, vol=None, info=None):
        best = (pkg.LzxSweepResult * 2)()
        p = lambda a, ty: None if a is None else a.ctypes.data_as(ty)
        assert eng.L.lzx_sweep_cut(eng.h, 2, S.ctypes.data_as(_f64p), 0, 0, 0, p(order, _u32p), p(cut, _u64p), p(vol, _u64p), best,
                                   None if info is None else ctypes.byref(info)) == LZX_OK
        assert [best[c].as_dict() for c in range(2)] == [result_of(x) for x in r]

    call()
    order = np.full((2, n), 0xdeadbeef, dtype=np.uint32)
    call(order=order)
    cut = np.full((2, n), 0xdeadbeef, dtype=np.uint64)
    call(cut=cut)
    vol = np.full((2, n), 0xdeadbeef, dtype=np.uint64)
    info = pkg.LzxSweepInfo()
    call(vol=vol, info=info)
    for c in range(2):
        assert np.array_equal(order[c], r[c]["order"]) and np.array_equal(cut[c], r[c]["cut"]) and np.array_equal(vol[c], r[c]["vol"])
    assert (info.entries, info.ns, info.width) == (A.nnz, 2, 2) and info.loop_ms > 0 and min(info.sort_ms, info.sweep_ms, info.scan_ms) > 0
    raw = eng.sweep_cut_raw(S, want_order=False)
    assert raw[0] is None and raw[1] is None and raw[2] is None and raw[3] == [result_of(x) for x in r]
    a, b = run(eng, S), run(eng, S)
    assert all(np.array_equal(a[i], b[i]) for i in range(3)) and a[3] == b[3]
    two = eng.sweep_cut(S)
    assert len(two) == 2 and np.array_equal(two[0][0], np.sort(r[0]["order"][:r[0]["k"]])) and two[1][1] == r[1]["value"]
    eng.close()


# ---- 6. isolation -------------------------------------------------------------------------------------------------------------
def test_a_chunked_decomposition_is_left_alone(pkg):
    name = "er_n1000"
    A = graph(name)
    x0 = np.random.default_rng(8).standard_normal(A.shape[0])
    eng = engine_of(pkg, A)
    a_ref, b_ref, Q_ref, _, _ = eng.lanczos(x0, 20)
    eng.lanczos_prepare(x0, 20)
    eng.lanczos_run_steps(7)
    assert_column(run(eng, scores_of(A.shape[0])), 0, ref(name, 0, 3, 0))
    assert eng.lanczos_progress() == (7, 20)
    eng.lanczos_run_steps(13)
    assert eng.conductance(np.arange(10)) == nx.conductance(graph_of(A), range(10))
    a, b, Q = eng.lanczos_fetch(20, want_q=True)
    assert np.array_equal(a, a_ref) and np.array_equal(b, b_ref) and np.array_equal(Q, Q_ref)
    eng.close()


def test_the_resident_bases_are_left_alone(pkg):
    name = "rmat_n3000_skew"
    A = graph(name)
    n = A.shape[0]
    rng = np.random.default_rng(9)
    x0, X0 = rng.standard_normal(n), rng.standard_normal((3, n))
    t, T = rng.standard_normal(12), rng.standard_normal((3, 12))
    eng = engine_of(pkg, A)
    eng.lanczos(x0, 12, want_q=False)
    eng.lanczos_multi(X0, 12)
    ans, ans_m = eng.multout(t), eng.multout_multi(T)
    got = run(eng, scores_of(n))
    for c in range(4):
        assert_column(got, c, ref(name, c, 3, 0))
    assert np.array_equal(eng.multout(t), ans) and np.array_equal(eng.multout_multi(T), ans_m)
    eng.close()


# ---- 7. errors and a matrix that is not symmetric -----------------------------------------------------------------------------
def test_errors(pkg):
    eng = pkg.Engine(0)
    eng.n = 4
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*no graph"):
        eng.sweep_cut_raw(np.zeros(4))
    eng.close()
    name = "er_n1000"
    A = graph(name)
    n = A.shape[0]
    S = scores_of(n)
    eng = engine_of(pkg, A)
    bad = S.copy()
    bad[1, 17] = np.nan
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*column 1 at index 17 is NaN"):
        eng.sweep_cut_raw(bad)
    best = (pkg.LzxSweepResult * 4)()
    Sc = np.ascontiguousarray(S)
    raw = lambda ns, scores, flags, k_min, k_max, res: eng.L.lzx_sweep_cut(eng.h, ns, scores, flags, k_min, k_max, None, None, None, res, None)
    assert raw(4, Sc.ctypes.data_as(_f64p), 8, 0, 0, best) == LZX_ERR_ARG and "unknown flag" in eng.L.lzx_last_error().decode()
    assert raw(4, Sc.ctypes.data_as(_f64p), 0, 7, 6, best) == LZX_ERR_ARG and "k_min" in eng.L.lzx_last_error().decode()
    assert raw(4, Sc.ctypes.data_as(_f64p), 0, 0, n + 1, best) == LZX_ERR_ARG and "k_max" in eng.L.lzx_last_error().decode()
    assert raw(4, Sc.ctypes.data_as(_f64p), 0, n + 1, 0, best) == LZX_ERR_ARG
    assert raw(4, None, 0, 0, 0, best) == LZX_ERR_ARG and raw(4, Sc.ctypes.data_as(_f64p), 0, 0, 0, None) == LZX_ERR_ARG
    assert raw(0, Sc.ctypes.data_as(_f64p), 0, 0, 0, best) == LZX_ERR_ARG
    with pytest.raises(ValueError, match="objective"):
        eng.sweep_cut_raw(S, objective="modularity")
    with pytest.raises(ValueError, match="shape"):
        eng.sweep_cut_raw(S[:, :-1])
    assert_column(run(eng, S), 0, ref(name, 0, 3, 0))
    eng.close()
    # the header's formula: ns = 4 columns of width 4, a window of n - 1 prefixes
    blocks = min((n - 2) // 256 + 1, 1024)
    state = (4 * n * 4 + 15) // 16 * 16 + 16 * n + 16 * 4 * n + 24 * 4 * blocks + 40 * 4 + 8 + 8 * ((n + 1) & ~1)
    small = engine_of(pkg, A, sweep_state_bytes=1)
    with pytest.raises(pkg.LzxError, match=rf"\(-4\).*needs {state} bytes"):
        small.sweep_cut_raw(S)
    x = np.random.default_rng(3).standard_normal(n)
    y = small.spmv(x)
    tight = engine_of(pkg, A, sweep_state_bytes=state - 1)
    with pytest.raises(pkg.LzxError, match=rf"\(-4\).*needs {state} bytes"):
        tight.sweep_cut_raw(S)
    roomy = engine_of(pkg, A, sweep_state_bytes=state)
    assert_column(run(roomy, S), 0, ref(name, 0, 3, 0))
    assert np.array_equal(small.spmv(x), y) and np.array_equal(roomy.spmv(x), y)
    for e in (small, tight, roomy):
        e.close()
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(A.indptr.astype(np.uint64), A.indices.astype(np.uint32))
    for e in grp.engines:
        with pytest.raises(pkg.LzxError, match=r"\(-3\).*communicator of 2"):
            e.sweep_cut_raw(np.zeros(e.n))
    grp.close()


def test_a_matrix_that_is_not_symmetric_stays_within_its_memory(pkg):
    """The upper triangle of a path alone: symmetry is the caller's promise and is not checked, and the numbers of such a matrix
    mean nothing.  The call returns and the handle still answers."""
    n = 1000
    eng = pkg.Engine(0)
    eng.set_graph_csr(np.minimum(np.arange(n + 1), n - 1).astype(np.uint64), np.arange(1, n, dtype=np.uint32))
    x = np.random.default_rng(4).standard_normal(n)
    y = eng.spmv(x)
    for kw in COMBOS:
        order, cut, vol, results, info = run(eng, scores_of(n), **kw)
        assert all(sorted(o.tolist()) == list(range(n)) for o in order) and info["entries"] == n - 1
    assert np.array_equal(eng.spmv(x), y)
    eng.close()


# ---- 8. the wrappers ----------------------------------------------------------------------------------------------------------
def test_wrappers_on_the_lopsided_barbell(pkg):
    A = graph("k8_k12")
    K8, K12 = list(range(8)), list(range(8, 20))
    lam, _ = fiedler_vector(A)
    eng = engine_of(pkg, A)
    tol = 1e-10
    members, value, lambda2, info = eng.spectral_bisection(tol=tol)
    assert members.tolist() in (K8, K12) and value == 1.0 / 57.0 and info["sweep"]["cut"] == 1 and info["sweep"]["den"] == 57
    print("lambda2", lambda2, "numpy", lam, "difference", abs(lambda2 - lam))
    assert abs(lambda2 - lam) <= tol * 2 * 12 + 1e-13
    assert eng.operator == pkg.OP_ADJACENCY
    assert eng.spectral_bisection(objective="expansion")[1] == 1.0 / 8.0
    for method in ("pagerank", "heat"):
        for seed, want in ((2, K8), (15, K12)):
            members, value, result = eng.local_cluster(seed, method=method)
            assert members.tolist() == want and value == 1.0 / 57.0 and (result["cut"], result["den"]) == (1, 57), (method, seed)
        both = eng.local_cluster([2, 15], method=method)
        assert [m.tolist() for m, _, _ in both] == [K8, K12]
        assert eng.operator == pkg.OP_ADJACENCY
    with pytest.raises(ValueError, match="method"):
        eng.local_cluster(2, method="walk")
    with pytest.raises(ValueError, match="seeds"):
        eng.local_cluster(20)
    eng.close()


def test_wrappers_on_the_planted_partition(pkg):
    """local_cluster is the sweep of the engine's own diffusion: the plumbing is checked exactly.  Block recovery is not asserted
    (the sweep of exact PageRank returns 66 to 70 vertices here)."""
    A = graph("planted_8x64")
    n = A.shape[0]
    eng = engine_of(pkg, A)
    seeds = [5 + 30 * k for k in range(17)]                                   # more than one batch of 16
    X = np.zeros((17, n))
    X[np.arange(17), seeds] = 1.0
    for method in ("pagerank", "heat"):
        got = eng.local_cluster(seeds, method=method, t=2.0, k=40)
        assert len(got) == 17
        P = np.vstack([eng._diffuse(X[:16], method, 0.85, 2.0, 40, 1e-10), eng._diffuse(X[16:], method, 0.85, 2.0, 40, 1e-10)])
        for c, (members, value, result) in enumerate(got):
            r = sweep_ref(A, P[c], PER_DEGREE)
            assert result == result_of(r) and value == r["value"] and np.array_equal(members, np.sort(r["order"][:r["k"]])), (method, c)
        print(method, "sizes", [len(m) for m, _, _ in got[:8]])
    capped = eng.local_cluster(seeds[0], k_max=20)
    assert 1 <= len(capped[0]) <= 20
    members, value, lambda2, info = eng.spectral_bisection()
    assert value == nx.conductance(graph_of(A), members.tolist()) and 0 < lambda2 < 20 and info["converged"] == 1
    eng.close()


def test_a_disconnected_graph_has_no_bisection(pkg):
    eng = engine_of(pkg, graph("k5_k10_and_7_isolated"))
    with pytest.raises(ValueError, match="9 components.*largest_component"):
        eng.spectral_bisection()
    assert eng.operator == pkg.OP_ADJACENCY
    sub, old = eng.largest_component()
    members, value, _, _ = sub.spectral_bisection()
    assert value == nx.conductance(nx.complete_graph(10), members.tolist())
    sub.close()
    eng.close()
