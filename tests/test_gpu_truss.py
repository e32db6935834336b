"""GPU: edge support and truss numbers on the device (include/lzx.h: lzx_truss; Engine.truss_raw / edge_support / truss_number /
max_truss / k_truss): known answers on small graphs, the golden fixtures against the numpy/scipy restatement of
tests/test_truss_host.py (which that file pins to networkx.k_truss), both peel launches and both support launches forced, self
loops, both hand-over forms, a relabelled graph, the k-truss subgraphs, isolation from the handle's other state, a matrix that
is not symmetric, and the error paths.

Everything is an integer: every comparison is equality."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from test_core_host import GOLDEN, GOLDEN_IDS
from test_gpu_core import (adjacency, clique_with_tail, cliques_and_isolated, complete_bipartite, complete_graph, engine_of, lanes_per_row,
                           wheel_graph, windmill)
from test_truss_host import INTS, VECTORS, fixture_case, k5_ears, truss_rounds, two_hubs, value_of

pytestmark = pytest.mark.gpu

_u32p = ctypes.POINTER(ctypes.c_uint32)
LZX_OK, LZX_ERR_LIMIT = 0, -6


def golden(name):
    return GOLDEN[GOLDEN_IDS.index(name)]


def run(eng):
    support, truss, layer, vertex, info = eng.truss_raw()
    for v in (support, truss, layer, vertex):
        assert v.dtype == np.uint32
    return dict(support=support, truss=truss, layer=layer, vertex_truss=vertex), {key: info[key] for key in INTS}


def check(eng, A, r):
    """one call against the restatement's vectors and integers; the per-entry outputs lie over the handle's own CSR"""
    A = sp.csr_matrix(A)
    rp, ci = eng.get_graph_csr()
    assert np.array_equal(rp, A.indptr.astype(np.uint64)) and np.array_equal(ci, A.indices.astype(np.uint32))
    vec, info = run(eng)
    for key in VECTORS:
        assert np.array_equal(vec[key], r[key]), key
    assert info == {key: r[key] for key in INTS}
    return vec, info


def same(a, b):
    return all(np.array_equal(a[0][key], b[0][key]) for key in VECTORS) and a[1] == b[1]


# ---- 1. known answers -----------------------------------------------------------------------------------------------------
# name -> (graph, the truss number of every edge or None, the info integers that are asserted outright)
KNOWN = {
    "one_edge": lambda: (adjacency(2, [(0, 1)]), 2, dict(edges=1, triangles=0, max_truss=2, rounds=1, levels=1, main_truss_edges=1)),
    "path_65": lambda: (adjacency(65, [(k, k + 1) for k in range(64)]), 2, dict(triangles=0, max_support=0, rounds=1, levels=1)),
    "bipartite_30_40": lambda: (complete_bipartite(30, 40), 2, dict(edges=1200, triangles=0, rounds=1, levels=1, main_truss_edges=1200)),
    "triangle": lambda: (complete_graph(3), 3, dict(edges=3, triangles=1, max_support=1, max_truss=3, rounds=1, levels=1)),
    "wheel_65": lambda: (wheel_graph(64), 3, dict(edges=128, triangles=64, max_support=2, rounds=2, levels=1)),
    "windmill_50": lambda: (windmill(50), 3, dict(edges=150, triangles=50, max_support=1, max_truss=3, rounds=1, levels=1)),
    "complete_20": lambda: (complete_graph(20), 20, dict(edges=190, triangles=1140, max_support=18, max_truss=20, rounds=1, levels=1)),
    "complete_200": lambda: (complete_graph(200), 200, dict(edges=19900, max_support=198, rounds=1, levels=1, main_truss_edges=19900)),
    "k5_k10_and_7_isolated": lambda: (cliques_and_isolated(), None, dict(edges=55, triangles=130, max_truss=10, rounds=2, levels=2, main_truss_edges=45)),
    "complete_20_with_a_path_of_40": lambda: (clique_with_tail(20, 40), None, dict(edges=230, triangles=1140, max_truss=20, rounds=2, levels=2,
                                                                                main_truss_edges=190)),
    "k5_ears": lambda: (k5_ears(), None, dict(edges=14, triangles=12, max_support=5, max_truss=5, rounds=2, levels=2, main_truss_edges=10)),
    "two_hubs": lambda: (two_hubs(), None, dict(edges=710, triangles=332, max_truss=11, rounds=4, levels=3, main_truss_edges=109)),
    "empty_graph": lambda: (sp.csr_matrix((5, 5)), None, dict(edges=0, triangles=0, max_support=0, max_truss=0, rounds=0, levels=0, main_truss_edges=0)),
    "single_vertex": lambda: (sp.csr_matrix((1, 1)), None, dict(edges=0, max_truss=0, rounds=0, levels=0)),
}


@pytest.mark.parametrize("name", list(KNOWN))
def test_known_answers(pkg, name):
    A, truss_ref, ints = KNOWN[name]()
    r = truss_rounds(A)
    if truss_ref is not None:
        assert np.array_equal(r["truss"], np.full(A.nnz, truss_ref, dtype=np.uint32))
    for key, value in ints.items():
        assert r[key] == value, key
    eng = engine_of(pkg, A)
    vec, _ = check(eng, A, r)
    assert eng.max_truss() == r["max_truss"]
    if name == "k5_ears":       # one decrement per dying triangle, not one per dying edge
        assert (value_of(A, vec["support"], 0, 1), value_of(A, vec["truss"], 0, 1), value_of(A, vec["layer"], 0, 1)) == (5, 5, 2)
    if name == "two_hubs":
        assert (value_of(A, vec["support"], 0, 1), value_of(A, vec["truss"], 0, 1), value_of(A, vec["layer"], 0, 1)) == (2, 4, 2)
    eng.close()


# ---- 2. fixtures ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=GOLDEN_IDS)
def test_fixtures_against_the_restatement(pkg, path):
    A, r = fixture_case(path)
    eng = engine_of(pkg, A)
    vec, info = check(eng, A, r)
    assert info["triangles"] == eng.triangles_raw(want_triangles=False, want_clustering=False)[2]["triangles"]
    rowmax = np.zeros(A.shape[0], dtype=np.uint32)
    np.maximum.at(rowmax, r["entry_rows"], vec["truss"])
    assert np.array_equal(vec["vertex_truss"], rowmax)
    S, T = eng.edge_support(), eng.truss_number()
    for M, key in ((S, "support"), (T, "truss")):
        assert M.shape == A.shape and np.array_equal(M.indptr, A.indptr) and np.array_equal(M.indices, A.indices)
        assert M.dtype == np.uint32 and np.array_equal(M.data, r[key])
    eng.close()


# ---- 3. both peel launches --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def launch_case(name):
    if name == "two_cliques_60_80":
        A = sp.csr_matrix(sp.block_diag([complete_graph(60), complete_graph(80)]))
    elif name == "two_hubs":
        A = two_hubs()
    elif name == "complete_200":
        A = complete_graph(200)
    else:
        return fixture_case(golden(name))
    A.sort_indices()
    return A, truss_rounds(A)


# (graph, truss_long_row or None, edges for the group launch, edges for the long-row launch)
LAUNCHES = [("rmat_n3000_skew", 4, True, True), ("two_cliques_60_80", 4, False, True), ("two_cliques_60_80", None, True, False),
            ("two_hubs", None, True, True), ("rmat_n3000_skew", 1 << 20, True, False)]


@pytest.mark.parametrize("name,long_row,short_edges,long_edges", LAUNCHES, ids=[f"{c[0]}-{c[1]}" for c in LAUNCHES])
def test_both_peel_launches(pkg, name, long_row, short_edges, long_edges):
    """A window's edge is peeled by a group of lanes when the shorter of its two rows has at most truss_long_row entries, by the
    long-row launch when it has more (default: 64 times the lanes per edge).  The edges that are peeled are those of every
    window but the call's last (all m edges are queued: nobody is left to push to): the edges with layer < rounds.  Which
    launch gets edges is asserted from the host's row lengths and layers:
      rmat_n3000_skew, 4         both
      two_cliques_60_80, 4       K_60 is one window of edges whose rows have 59 entries: the long-row launch alone
      two_cliques_60_80          unforced (32 lanes, threshold 2 048): the group launch alone
      two_hubs                   unforced (4 lanes, threshold 256): the leaves' edges by the group launch, the edge (0, 1), whose
                                 rows have 311 entries each, by the long-row launch
      rmat_n3000_skew, 2^20      the group launch alone
    Each is compared with the restatement and with the unforced run."""
    A, r = launch_case(name)
    lengths = np.diff(A.indptr)
    threshold = 64 * lanes_per_row(A) if long_row is None else long_row
    rows, cols = r["entry_rows"], A.indices
    peeled = (rows != cols) & (r["layer"] < r["rounds"])
    shorter = np.minimum(lengths[rows], lengths[cols])[peeled]
    print(name, "threshold", threshold, "peeled entries", len(shorter), "long among them", int((shorter > threshold).sum()), "longest row", int(lengths.max()))
    assert bool((shorter <= threshold).any()) == short_edges and bool((shorter > threshold).any()) == long_edges
    unforced = engine_of(pkg, A)
    first = check(unforced, A, r)
    unforced.close()
    if long_row is not None:
        forced = engine_of(pkg, A, truss_long_row=long_row)
        assert same(run(forced), first)
        forced.close()


# ---- 4. the support launches --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,long_list", [("rmat_n3000_skew", 2), ("rmat_n3000_skew", 4), ("complete_200", 4)])
def test_both_support_launches(pkg, name, long_list):
    """tri_long_list forced small: oriented rows of more entries are counted by the wide support kernel (a wavefront per
    out-edge), which stages lists of at most 32 times the threshold in LDS and reads longer ones where they lie:
      rmat_n3000_skew, 4   lists of at most 72, all staged (128), both walks
      rmat_n3000_skew, 2   lists of more than 64 are not staged
      complete_200, 4      k_b < k_a on every out-edge: N+(b) walked, staged and (lists of 129 .. 199) not staged
    The same support, and all that follows from it, as the unforced run's (which the other tests compare with the restatement)."""
    A, r = launch_case(name)
    eng = engine_of(pkg, A, tri_long_list=long_list)
    kmax = eng.triangles_raw(want_triangles=False, want_clustering=False)[2]["oriented_max_degree"]
    assert kmax > 32 * long_list if (name, long_list) != ("rmat_n3000_skew", 4) else long_list < kmax <= 32 * long_list
    check(eng, A, r)
    eng.close()


# ---- 5. self loops, hand-over forms, relabelling, repeats -----------------------------------------------------------------
def test_self_loops_change_nothing(pkg):
    A, r = fixture_case(golden("er_n1000"))
    n = A.shape[0]
    coo = sp.triu(A).tocoo()
    loops = np.arange(0, n, 7)
    B = sp.csr_matrix(A + sp.csr_matrix((np.ones(len(loops)), (loops, loops)), shape=(n, n)))
    B.sort_indices()
    rb = truss_rounds(B)
    out = []
    for extra, M, ref in ((np.zeros(0, dtype=np.int64), A, r), (loops, B, rb)):
        eng = pkg.Engine(0)
        eng.set_graph_edges(n, np.concatenate([coo.row, extra]), np.concatenate([coo.col, extra]))
        assert eng.info()["nnz"] == A.nnz + len(extra)
        out.append(check(eng, M, ref))
        eng.close()
    (v0, i0), (v1, i1) = out
    off = rb["entry_rows"] != B.indices
    for key in ("support", "truss", "layer"):
        assert np.array_equal(v1[key][off], v0[key]) and not v1[key][~off].any(), key
    assert np.array_equal(v0["vertex_truss"], v1["vertex_truss"]) and i0 == i1


def test_hand_over_form_does_not_matter(pkg):
    A, r = fixture_case(golden("er_n4000_deg20"))
    for pb in (1, 0):
        eng = engine_of(pkg, A, propagation_blocking=pb)
        check(eng, A, r)
        eng.close()


def test_a_relabelled_graph_gives_the_permuted_values(pkg):
    A, r = fixture_case(golden("rmat_n4096"))
    n = A.shape[0]
    new_of_old = np.random.default_rng(6).permutation(n)
    P = sp.csr_matrix((np.ones(n), (new_of_old, np.arange(n))), shape=(n, n))
    B = sp.csr_matrix(P @ A @ P.T)
    B.sort_indices()
    eng = engine_of(pkg, B)
    vec, info = run(eng)
    for key in ("support", "truss", "layer"):
        M = sp.csr_matrix((vec[key] + 1.0, B.indices, B.indptr), shape=(n, n))        # + 1: a support of 0 stays a stored entry
        back = sp.csr_matrix(P.T @ M @ P)
        back.sort_indices()
        assert np.array_equal(back.indices, A.indices) and np.array_equal(back.data - 1.0, r[key]), key
    assert np.array_equal(vec["vertex_truss"][new_of_old], r["vertex_truss"])
    assert info == {key: r[key] for key in INTS}
    eng.close()


def test_two_calls_give_the_same_bits(pkg):
    A, r = fixture_case(golden("rmat_n3000_skew"))
    eng = engine_of(pkg, A)
    first = check(eng, A, r)
    assert same(run(eng), first)
    eng.close()


def test_counts_only_and_each_output_alone(pkg):
    A, r = fixture_case(golden("er_n1000"))
    n, nnz = A.shape[0], A.nnz
    eng = engine_of(pkg, A)
    info = pkg.LzxTrussInfo()
    assert eng.L.lzx_truss(eng.h, None, None, None, None, ctypes.byref(info)) == 0
    assert {key: getattr(info, key) for key in INTS} == {key: r[key] for key in INTS}
    assert eng.L.lzx_truss(eng.h, None, None, None, None, None) == 0
    for at, key in enumerate(VECTORS):
        out = np.full(n if key == "vertex_truss" else nnz, 0xdeadbeef, dtype=np.uint32)
        args = [None] * 5
        args[at] = out.ctypes.data_as(_u32p)
        assert eng.L.lzx_truss(eng.h, *args) == 0
        assert np.array_equal(out, r[key]), key
    s, t, l, v, _ = eng.truss_raw(want_support=False, want_layer=False)
    assert s is None and l is None and np.array_equal(t, r["truss"]) and np.array_equal(v, r["vertex_truss"])
    eng.close()


# ---- 6. the k-truss ---------------------------------------------------------------------------------------------------------
def check_truss_subgraph(sub, old, A, r, k):
    """the sub-engine holds the edges of truss number >= k and the vertices that keep one; there every edge has support >= k - 2"""
    keep = r["truss"] >= k
    F = sp.csr_matrix((np.ones(int(keep.sum())), (r["entry_rows"][keep], A.indices[keep])), shape=A.shape)
    want = np.flatnonzero(np.diff(F.indptr))
    assert np.array_equal(old, want.astype(old.dtype)) and sub.n == len(want)
    S = sp.csr_matrix(F[want][:, want])
    S.sort_indices()
    rp, ci = sub.get_graph_csr()
    assert np.array_equal(rp, S.indptr.astype(np.uint64)) and np.array_equal(ci, S.indices.astype(np.uint32))
    support, truss, _, _, info = sub.truss_raw(want_layer=False, want_vertex=False)
    assert int(support.min()) >= k - 2 and int(truss.min()) >= k
    assert info["edges"] == int(keep.sum()) // 2 and info["max_truss"] == r["max_truss"]


def test_k_truss(pkg):
    A, r = fixture_case(golden("rmat_n4096"))
    top = r["max_truss"]
    eng = engine_of(pkg, A)
    sub, old = eng.k_truss()
    check_truss_subgraph(sub, old, A, r, top)
    assert sub.info()["nnz"] == 2 * r["main_truss_edges"]
    sub.close()
    assert 4 < top and (r["truss"] == 3).any()
    sub, old = eng.k_truss(4)
    check_truss_subgraph(sub, old, A, r, 4)
    sub.close()
    with pytest.raises(ValueError, match=rf"largest truss number {top}\b"):
        eng.k_truss(top + 1)
    assert eng.max_truss() == top
    assert np.array_equal(eng.truss_raw(False, True, False, False)[1], r["truss"])      # the engine keeps its graph
    eng.close()


# ---- 7. isolation ---------------------------------------------------------------------------------------------------------
def test_a_chunked_decomposition_is_left_alone(pkg):
    A, r = fixture_case(golden("er_n1000"))
    x0 = np.random.default_rng(8).standard_normal(A.shape[0])
    eng = engine_of(pkg, A)
    a_ref, b_ref, Q_ref, _, _ = eng.lanczos(x0, 20)
    eng.lanczos_prepare(x0, 20)
    eng.lanczos_run_steps(7)
    check(eng, A, r)
    assert eng.lanczos_progress() == (7, 20)
    eng.lanczos_run_steps(13)
    a, b, Q = eng.lanczos_fetch(20, want_q=True)
    assert np.array_equal(a, a_ref) and np.array_equal(b, b_ref) and np.array_equal(Q, Q_ref)
    eng.close()


def test_the_resident_bases_are_left_alone(pkg):
    A, r = fixture_case(golden("rmat_n3000_skew"))
    n = A.shape[0]
    rng = np.random.default_rng(9)
    x0, X0 = rng.standard_normal(n), rng.standard_normal((3, n))
    t, T = rng.standard_normal(12), rng.standard_normal((3, 12))
    eng = engine_of(pkg, A)
    eng.lanczos(x0, 12, want_q=False)
    eng.lanczos_multi(X0, 12)
    ans, ans_m = eng.multout(t), eng.multout_multi(T)
    check(eng, A, r)
    assert np.array_equal(eng.multout(t), ans) and np.array_equal(eng.multout_multi(T), ans_m)
    # a kept probe basis
    alpha, beta, k_used, _ = eng.lanczos_probes(3, 0, 4, 12, keep_basis=True)
    Tp = pkg.slq_diag_coefficients(alpha, beta, k_used, n, 0.1, 0.0)
    diag = eng.probe_diag(Tp)
    assert eng.max_truss() == r["max_truss"]
    assert np.array_equal(eng.probe_diag(Tp), diag) and np.array_equal(eng.multout(t), ans)
    eng.close()


# ---- 8. not symmetric -----------------------------------------------------------------------------------------------------
def test_a_matrix_that_is_not_symmetric_stays_within_its_memory(pkg):
    """The upper triangle of a path alone: symmetry is the caller's promise and is not checked, and the numbers of such a matrix
    mean nothing.  The call returns, its rounds are bounded, and the handle still answers."""
    n = 1000
    eng = pkg.Engine(0)
    eng.set_graph_csr(np.minimum(np.arange(n + 1), n - 1).astype(np.uint64), np.arange(1, n, dtype=np.uint32))
    x = np.random.default_rng(4).standard_normal(n)
    y = eng.spmv(x)
    outs = [np.zeros(n - 1, dtype=np.uint32) for _ in range(3)] + [np.zeros(n, dtype=np.uint32)]
    info = pkg.LzxTrussInfo()
    rc = eng.L.lzx_truss(eng.h, *[o.ctypes.data_as(_u32p) for o in outs], ctypes.byref(info))
    assert rc in (LZX_OK, LZX_ERR_LIMIT)
    if rc == LZX_OK:
        assert info.edges <= n - 1 and info.rounds <= info.edges + 1
    assert np.array_equal(eng.spmv(x), y)
    eng.close()


# ---- 9. errors ------------------------------------------------------------------------------------------------------------
def test_errors(pkg):
    eng = pkg.Engine(0)
    eng.n = 4
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*no graph"):
        eng.truss_raw(False, False, False, False)
    eng.close()
    A, r = fixture_case(golden("er_n1000"))
    n, nnz = A.shape[0], A.nnz
    state = 8 * (n + 1) + 4 * n + 16 * 1024 + 16 + 24 * (nnz // 2) + 8 * nnz      # the header's formula
    for cap in (4 * n, state - 8):          # the vertices' arena; the edges' state
        small = engine_of(pkg, A, truss_state_bytes=cap)
        with pytest.raises(pkg.LzxError, match=r"\(-4\).*needs \d+ bytes"):
            small.truss_raw()
        x = np.random.default_rng(3).standard_normal(n)
        y = small.spmv(x)
        plain = engine_of(pkg, A)
        assert np.array_equal(small.spmv(x), y) and np.array_equal(plain.spmv(x), y)
        plain.close()
        small.close()
    roomy = engine_of(pkg, A, truss_state_bytes=state)
    check(roomy, A, r)
    roomy.close()
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(A.indptr.astype(np.uint64), A.indices.astype(np.uint32))
    for e in grp.engines:
        with pytest.raises(pkg.LzxError, match=r"\(-3\).*communicator of 2"):
            e.truss_raw(False, False, False, False)
    grp.close()
