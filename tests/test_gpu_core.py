"""GPU: core numbers and onion layers on the device (include/lzx.h: lzx_core_numbers; Engine.core_number / onion_layers /
degeneracy / k_core / k_shell): known answers on small graphs, the golden fixtures against networkx and the numpy restatement
of tests/test_core_host.py, both peel launches forced, self loops, both hand-over forms, a relabelled graph, the k-core and
k-shell subgraphs, isolation from the handle's other state, a matrix that is not symmetric, and the error paths.

Everything is an integer: every comparison is equality."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

from test_core_host import GOLDEN, GOLDEN_IDS, INTS, fixture_case, peel_rounds, skewed_graph

pytestmark = pytest.mark.gpu

_u32p = ctypes.POINTER(ctypes.c_uint32)


def golden(name):
    return GOLDEN[GOLDEN_IDS.index(name)]


def engine_of(pkg, A, **options):
    eng = pkg.Engine(0, **options)
    A = sp.csr_matrix(A)
    A.sort_indices()
    eng.set_graph_csr(A.indptr.astype(np.uint64), A.indices.astype(np.uint32))
    return eng


def adjacency(n, edges):
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    M = sp.coo_matrix((np.ones(2 * len(e)), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))), shape=(n, n))
    M = sp.csr_matrix(M)
    M.data[:] = 1.0
    return M


def run(eng):
    core, layer, info = eng.core_number_raw()
    assert core.dtype == np.uint32 and layer.dtype == np.uint32
    return core, layer, {key: info[key] for key in INTS}


def check(eng, r):
    """one call against the restatement's (or networkx's, where the caller checked them equal) vectors and integers"""
    core, layer, info = run(eng)
    assert np.array_equal(core, r["core"]) and np.array_equal(layer, r["layer"])
    assert info == {key: r[key] for key in INTS}
    return core, layer, info


# ---- 1. known answers -----------------------------------------------------------------------------------------------------
def clique_edges(members):
    return list(itertools.combinations(members, 2))


def complete_graph(n):
    return adjacency(n, clique_edges(range(n)))


def complete_bipartite(a, b):
    return adjacency(a + b, [(u, a + v) for u in range(a) for v in range(b)])


def grid_graph(m):
    n = m * m
    return adjacency(n, [(k, k + 1) for k in range(n) if (k + 1) % m] + [(k, k + m) for k in range(n - m)])


def hypercube_graph(q):
    return adjacency(1 << q, [(v, v ^ (1 << k)) for v in range(1 << q) for k in range(q) if v < v ^ (1 << k)])


def wheel_graph(rim):
    return adjacency(rim + 1, [(0, k) for k in range(1, rim + 1)] + [(k, k % rim + 1) for k in range(1, rim + 1)])


def windmill(blades):
    edges = []
    for k in range(blades):
        u, v = 1 + 2 * k, 2 + 2 * k
        edges += [(0, u), (0, v), (u, v)]
    return adjacency(2 * blades + 1, edges)


def binary_tree(depth):
    n = (1 << (depth + 1)) - 1
    return adjacency(n, [((v - 1) // 2, v) for v in range(1, n)])


def clique_with_tail(q, tail):
    return adjacency(q + tail, clique_edges(range(q)) + [(q - 1 + k, q + k) for k in range(tail)])


def cliques_and_isolated():
    return adjacency(22, clique_edges(range(5)) + clique_edges(range(5, 15)))


# name -> (graph, core (a number or a vector), layer (a vector) or None, the info integers that are asserted outright)
KNOWN = {
    "single_vertex": lambda: (sp.csr_matrix((1, 1)), 0, [1], dict(degeneracy=0, rounds=1, levels=1, main_core_size=1, core0=1)),
    "one_edge": lambda: (adjacency(2, [(0, 1)]), 1, [1, 1], dict(degeneracy=1, rounds=1, levels=1, main_core_size=2, core0=0)),
    "path_65": lambda: (adjacency(65, [(k, k + 1) for k in range(64)]), 1, [min(k, 64 - k) + 1 for k in range(65)], dict(rounds=33, levels=1)),
    "cycle_64": lambda: (adjacency(64, [(k, (k + 1) % 64) for k in range(64)]), 2, [1] * 64, dict(rounds=1, main_core_size=64)),
    "star_300": lambda: (adjacency(300, [(0, k) for k in range(1, 300)]), 1, [2] + [1] * 299, dict(rounds=2, levels=1, main_core_size=300)),
    "complete_20": lambda: (complete_graph(20), 19, [1] * 20, dict(rounds=1)),
    "complete_200": lambda: (complete_graph(200), 199, [1] * 200, dict(rounds=1, levels=1, main_core_size=200)),
    "bipartite_30_40": lambda: (complete_bipartite(30, 40), 30, None, dict(degeneracy=30, levels=1)),
    "grid_8x8": lambda: (grid_graph(8), 2, None, dict(degeneracy=2)),
    "hypercube_10": lambda: (hypercube_graph(10), 10, [1] * 1024, dict(rounds=1)),
    "wheel_65": lambda: (wheel_graph(64), 3, [2] + [1] * 64, dict(rounds=2)),
    "windmill_50": lambda: (windmill(50), 2, [2] + [1] * 100, dict(rounds=2)),
    "binary_tree_depth_10": lambda: (binary_tree(10), 1, None, dict(degeneracy=1, levels=1)),
    "complete_20_with_a_path_of_40": lambda: (clique_with_tail(20, 40), [19] * 20 + [1] * 40, [41] * 20 + list(range(40, 0, -1)),
                                               dict(degeneracy=19, levels=2, rounds=41, main_core_size=20, core0=0)),
    "k5_k10_and_7_isolated": lambda: (cliques_and_isolated(), [4] * 5 + [9] * 10 + [0] * 7, [2] * 5 + [3] * 10 + [1] * 7,
                                      dict(degeneracy=9, levels=3, rounds=3, core0=7, main_core_size=10)),
}


@pytest.mark.parametrize("name", list(KNOWN))
def test_known_answers(pkg, name):
    A, core_ref, layer_ref, ints = KNOWN[name]()
    n = A.shape[0]
    r = peel_rounds(A)
    assert np.array_equal(r["core"], np.broadcast_to(np.asarray(core_ref, dtype=np.uint32), (n,)))
    if layer_ref is not None:
        assert np.array_equal(r["layer"], np.asarray(layer_ref, dtype=np.uint32))
    for key, value in ints.items():
        assert r[key] == value, key
    eng = engine_of(pkg, A)
    check(eng, r)
    assert eng.degeneracy() == r["degeneracy"]
    eng.close()


# ---- 2. fixtures ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=GOLDEN_IDS)
def test_fixtures_against_networkx(pkg, path):
    A, r, (core_nx, layer_nx) = fixture_case(path)
    n = A.shape[0]
    eng = engine_of(pkg, A)
    core, layer, info = check(eng, r)
    assert np.array_equal(core, core_nx) and np.array_equal(layer, layer_nx)
    assert info["degeneracy"] == int(core_nx.max()) and info["rounds"] == int(layer_nx.max())
    assert info["levels"] == len(set(core_nx.tolist())) and info["main_core_size"] == int((core_nx == core_nx.max()).sum())
    assert info["core0"] == int((core_nx == 0).sum())
    assert eng.degeneracy() == int(core_nx.max())
    nodes = np.array([0, n - 1, 17, 17])
    assert np.array_equal(eng.core_number(nodes), core_nx[nodes]) and np.array_equal(eng.onion_layers(nodes), layer_nx[nodes])
    assert np.array_equal(eng.core_number(), core_nx) and np.array_equal(eng.onion_layers(), layer_nx)
    for bad in ([n], [-1], [0.0], [3.7], np.array([True, False]), [[0, 1]]):
        with pytest.raises(ValueError):
            eng.core_number(bad)
        with pytest.raises(ValueError):
            eng.onion_layers(bad)
    assert eng.core_number([]).shape == (0,) and np.array_equal(eng.onion_layers(np.uint32(17)), layer_nx[[17]])
    eng.close()


# ---- 3. both peel launches --------------------------------------------------------------------------------------------------
def hub_beside_a_clique():
    """star_ring_n1500 and, apart from it, K_6: the ring and its hub are peeled at k = 3, the clique is the main core, so the
    hub's row of 1 499 entries is a row of a window that is peeled (the last window of a call is not: nobody is left)"""
    A, _, _ = fixture_case(golden("star_ring_n1500"))
    return sp.csr_matrix(sp.block_diag([A, complete_graph(6)]))


def two_cliques():
    """K_200 and K_250 apart: all of K_200 is one window of 200 rows of 199 entries, every neighbour already marked"""
    return sp.csr_matrix(sp.block_diag([complete_graph(200), complete_graph(250)]))


@functools.lru_cache(maxsize=None)
def launch_case(name):
    if name == "complete_200":
        A = complete_graph(200)
    elif name == "hub_beside_a_clique":
        A = hub_beside_a_clique()
    elif name == "two_cliques_200_250":
        A = two_cliques()
    elif name == "skewed_2^14":
        return skewed_graph()
    elif name == "skewed_2^14_beside_a_clique":
        A = sp.csr_matrix(sp.block_diag([skewed_graph()[0], complete_graph(40)]))
    else:
        return fixture_case(golden(name))[:2]
    return A, peel_rounds(A)


def lanes_per_row(A):
    """the library's choice: 4 ... 32 lanes per row of a window, about half the mean length of the rows that have an entry"""
    lengths = np.diff(sp.csr_matrix(A).indptr)
    mean = int(lengths.sum()) // max(int((lengths > 0).sum()), 1)
    G = 4
    while G < 32 and 2 * G <= mean:
        G *= 2
    return G


# (graph, core_long_row or None, rows for the group launch, rows for the long-row launch)
LAUNCHES = [("rmat_n3000_skew", 4, True, True), ("star_ring_n1500", 4, True, False), ("complete_200", 4, False, False),
            ("star_ring_n1500", 1 << 20, True, False), ("hub_beside_a_clique", None, True, True), ("hub_beside_a_clique", 4, True, True),
            ("hub_beside_a_clique", 1 << 20, True, False), ("two_cliques_200_250", 4, False, True), ("two_cliques_200_250", None, True, False),
            ("skewed_2^14", None, True, False), ("skewed_2^14_beside_a_clique", None, True, True)]


@pytest.mark.parametrize("name,long_row,short_rows,long_rows", LAUNCHES, ids=[f"{c[0]}-{c[1]}" for c in LAUNCHES])
def test_both_peel_launches(pkg, name, long_row, short_rows, long_rows):
    """A window's rows of at most core_long_row entries are peeled a group of lanes per row, longer ones by the long-row launch
    (default: 64 times the lanes per row).  The rows that are peeled are those of every window but the call's last, which is
    not peeled (all n vertices are queued: nobody is left to push to): the vertices with layer < rounds.  Which launch gets rows
    is asserted from the host's degrees and layers:
      rmat_n3000_skew, 4          both
      star_ring_n1500, 4 / 2^20   the ring's rows of 3 entries; the hub is the last window, with or without the shape
      complete_200, 4             one window, the last: no peel at all
      hub_beside_a_clique         the hub's 1 499 entries: the long-row launch unforced (threshold 256) and at 4, the group kernel
                                  at 2^20
      two_cliques_200_250         K_200's rows of 199 entries: long at 4, the group kernel unforced (threshold 2 048)
      skewed_2^14                 unforced (threshold 1 024): loops, 219 rounds, 16 368 rows peeled by the group kernel; its rows of
                                  more than 1 024 entries (the longest has 7 646) all fall in the last window
      skewed_2^14_beside_a_clique  the same and K_40 apart, which is then the main core: the long rows are peeled, in 7 slices
    Each is compared with the restatement and with the unforced run."""
    A, r = launch_case(name)
    lengths = np.diff(sp.csr_matrix(A).indptr)
    threshold = 64 * lanes_per_row(A) if long_row is None else long_row
    peeled = lengths[r["layer"] < r["rounds"]]
    print(name, "threshold", threshold, "peeled rows", len(peeled), "long among them", int((peeled > threshold).sum()), "longest", int(lengths.max()))
    assert bool(((peeled <= threshold) & (peeled > 0)).any()) == short_rows and bool((peeled > threshold).any()) == long_rows
    unforced = engine_of(pkg, A)
    c0, l0, i0 = check(unforced, r)
    unforced.close()
    if long_row is not None:
        forced = engine_of(pkg, A, core_long_row=long_row)
        c1, l1, i1 = run(forced)
        assert np.array_equal(c1, c0) and np.array_equal(l1, l0) and i1 == i0
        forced.close()


# ---- 4. self loops, hand-over forms, relabelling, repeats -----------------------------------------------------------------
def test_self_loops_change_nothing(pkg):
    A, r, _ = fixture_case(golden("er_n1000"))
    n = A.shape[0]
    coo = sp.triu(A).tocoo()
    loops = np.arange(0, n, 7)
    out = []
    for extra in (np.zeros(0, dtype=np.int64), loops):
        eng = pkg.Engine(0)
        eng.set_graph_edges(n, np.concatenate([coo.row, extra]), np.concatenate([coo.col, extra]))
        assert eng.info()["nnz"] == A.nnz + len(extra)
        out.append(check(eng, r))
        eng.close()
    (c0, l0, i0), (c1, l1, i1) = out
    assert np.array_equal(c0, c1) and np.array_equal(l0, l1) and i0 == i1


def test_hand_over_form_does_not_matter(pkg):
    A, r, _ = fixture_case(golden("er_n4000_deg20"))
    for pb in (1, 0):
        eng = engine_of(pkg, A, propagation_blocking=pb)
        check(eng, r)
        eng.close()


def test_a_relabelled_graph_gives_the_permuted_vectors(pkg):
    A, r, _ = fixture_case(golden("rmat_n4096"))
    n = A.shape[0]
    new_of_old = np.random.default_rng(6).permutation(n)
    P = sp.csr_matrix((np.ones(n), (new_of_old, np.arange(n))), shape=(n, n))
    eng = engine_of(pkg, sp.csr_matrix(P @ A @ P.T))
    core, layer, info = run(eng)
    assert np.array_equal(core[new_of_old], r["core"]) and np.array_equal(layer[new_of_old], r["layer"])
    assert info == {key: r[key] for key in INTS}
    eng.close()


def test_two_calls_give_the_same_bits(pkg):
    A, r, _ = fixture_case(golden("rmat_n3000_skew"))
    eng = engine_of(pkg, A)
    c0, l0, i0 = check(eng, r)
    c1, l1, i1 = run(eng)
    assert np.array_equal(c0, c1) and np.array_equal(l0, l1) and i0 == i1
    eng.close()


def test_counts_only_and_each_vector_alone(pkg):
    A, r, _ = fixture_case(golden("er_n1000"))
    n = A.shape[0]
    eng = engine_of(pkg, A)
    info = pkg.LzxCoreInfo()
    assert eng.L.lzx_core_numbers(eng.h, None, None, ctypes.byref(info)) == 0
    assert {key: getattr(info, key) for key in INTS} == {key: r[key] for key in INTS}
    assert eng.L.lzx_core_numbers(eng.h, None, None, None) == 0
    core, layer = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    assert eng.L.lzx_core_numbers(eng.h, core.ctypes.data_as(_u32p), None, None) == 0
    assert np.array_equal(core, r["core"])
    assert eng.L.lzx_core_numbers(eng.h, None, layer.ctypes.data_as(_u32p), None) == 0
    assert np.array_equal(layer, r["layer"])
    c2, l2, _ = eng.core_number_raw(want_core=False)
    assert c2 is None and np.array_equal(l2, r["layer"])
    eng.close()


# ---- 5. subgraphs ---------------------------------------------------------------------------------------------------------
def check_subgraph(sub, old, A, members, k):
    """the sub-engine holds the subgraph of A induced by `members` (a mask); every row has at least k entries (k or None)"""
    want = np.flatnonzero(members)
    assert np.array_equal(old, want.astype(old.dtype))
    S = sp.csr_matrix(A[want][:, want])
    S.sort_indices()
    rp, ci = sub.get_graph_csr()
    assert np.array_equal(rp, S.indptr.astype(np.uint64)) and np.array_equal(ci, S.indices.astype(np.uint32))
    if k is not None:
        assert int(np.diff(rp.astype(np.int64)).min()) >= k
        assert int(sub.core_number().min()) >= k


def test_k_core_and_k_shell(pkg):
    A, r, _ = fixture_case(golden("rmat_n4096"))
    A = sp.csr_matrix(A)
    core, top = r["core"], r["degeneracy"]
    eng = engine_of(pkg, A)
    sub, old = eng.k_core()
    check_subgraph(sub, old, A, core >= top, top)
    assert sub.n == r["main_core_size"] and sub.degeneracy() == top
    sub.close()
    k = 10
    assert 0 < k < top and (core < k).any() and (core == k).any()
    sub, old = eng.k_core(k)
    check_subgraph(sub, old, A, core >= k, k)
    assert sub.degeneracy() == top
    sub.close()
    sub, old = eng.k_shell(k)
    check_subgraph(sub, old, A, core == k, None)
    sub.close()
    sub, old = eng.k_shell()
    check_subgraph(sub, old, A, core == top, top)
    sub.close()
    sub, old = eng.k_core(0)
    assert sub.n == A.shape[0]
    sub.close()
    absent = next(j for j in range(top) if not (core == j).any())
    with pytest.raises(ValueError, match=rf"degeneracy {top}\b"):
        eng.k_core(top + 1)
    with pytest.raises(ValueError, match=rf"core number {absent}\b"):
        eng.k_shell(absent)
    with pytest.raises(ValueError):
        eng.k_shell(top + 1)
    assert np.array_equal(eng.core_number(), core)      # the engine keeps its graph
    eng.close()


# ---- 6. isolation ---------------------------------------------------------------------------------------------------------
def test_a_chunked_decomposition_is_left_alone(pkg):
    A, r, _ = fixture_case(golden("er_n1000"))
    x0 = np.random.default_rng(8).standard_normal(A.shape[0])
    eng = engine_of(pkg, A)
    a_ref, b_ref, Q_ref, _, _ = eng.lanczos(x0, 20)
    eng.lanczos_prepare(x0, 20)
    eng.lanczos_run_steps(7)
    assert np.array_equal(eng.core_number(), r["core"])
    assert eng.lanczos_progress() == (7, 20)
    eng.lanczos_run_steps(13)
    a, b, Q = eng.lanczos_fetch(20, want_q=True)
    assert np.array_equal(a, a_ref) and np.array_equal(b, b_ref) and np.array_equal(Q, Q_ref)
    eng.close()


def test_the_resident_bases_are_left_alone(pkg):
    A, r, _ = fixture_case(golden("rmat_n3000_skew"))
    n = A.shape[0]
    rng = np.random.default_rng(9)
    x0, X0 = rng.standard_normal(n), rng.standard_normal((3, n))
    t, T = rng.standard_normal(12), rng.standard_normal((3, 12))
    eng = engine_of(pkg, A)
    eng.lanczos(x0, 12, want_q=False)
    eng.lanczos_multi(X0, 12)
    ans, ans_m = eng.multout(t), eng.multout_multi(T)
    assert np.array_equal(eng.core_number(), r["core"])
    assert np.array_equal(eng.multout(t), ans) and np.array_equal(eng.multout_multi(T), ans_m)
    # a kept probe basis
    alpha, beta, k_used, _ = eng.lanczos_probes(3, 0, 4, 12, keep_basis=True)
    Tp = pkg.slq_diag_coefficients(alpha, beta, k_used, n, 0.1, 0.0)
    diag = eng.probe_diag(Tp)
    assert np.array_equal(eng.onion_layers(), r["layer"])
    assert np.array_equal(eng.probe_diag(Tp), diag) and np.array_equal(eng.multout(t), ans)
    eng.close()


# ---- 7. not symmetric -----------------------------------------------------------------------------------------------------
def test_a_matrix_that_is_not_symmetric_stays_within_its_memory(pkg):
    """The upper triangle of a path alone: symmetry is the caller's promise and is not checked, and the numbers of such a matrix
    mean nothing.  The call returns, its rounds are bounded and every vertex has been given a layer; the handle still answers."""
    n = 1000
    eng = pkg.Engine(0)
    eng.set_graph_csr(np.minimum(np.arange(n + 1), n - 1).astype(np.uint64), np.arange(1, n, dtype=np.uint32))
    x = np.random.default_rng(4).standard_normal(n)
    y = eng.spmv(x)
    core, layer, info = eng.core_number_raw()      # LZX_OK, or this raises
    assert info["rounds"] <= n
    assert layer.min() >= 1 and layer.max() <= info["rounds"]
    assert np.array_equal(eng.spmv(x), y)
    eng.close()


# ---- 8. errors ------------------------------------------------------------------------------------------------------------
def test_errors(pkg):
    eng = pkg.Engine(0)
    eng.n = 4
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*no graph"):
        eng.core_number_raw()
    eng.close()
    A, r, _ = fixture_case(golden("er_n1000"))
    n = A.shape[0]
    small = engine_of(pkg, A, core_state_bytes=4 * n)
    with pytest.raises(pkg.LzxError, match=r"\(-4\).*needs \d+ bytes"):
        small.core_number_raw()
    x = np.random.default_rng(3).standard_normal(n)
    y = small.spmv(x)
    plain = engine_of(pkg, A)
    assert np.array_equal(small.spmv(x), y) and np.array_equal(plain.spmv(x), y)
    plain.close()
    small.close()
    roomy = engine_of(pkg, A, core_state_bytes=16 * n + 64)
    assert np.array_equal(roomy.core_number(), r["core"])
    roomy.close()
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(A.indptr.astype(np.uint64), A.indices.astype(np.uint32))
    for e in grp.engines:
        with pytest.raises(pkg.LzxError, match=r"\(-3\).*communicator of 2"):
            e.core_number_raw()
    grp.close()
