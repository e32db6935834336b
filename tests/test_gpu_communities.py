"""GPU: greedy colouring, label-propagation communities and modularity on the device (include/lzx.h: lzx_color,
lzx_label_propagation, lzx_modularity; Engine.color_raw / greedy_color / label_propagation_raw / label_propagation_communities /
modularity / community): known answers on small graphs and the golden fixtures against the numpy restatement of
tests/test_communities_host.py (which that file pins to networkx), with both tie rules; the shapes at which the kernels change --
the 64-colour windows, the long-row launches, the three propagation paths -- forced and unforced; self loops and isolated
vertices, both hand-over forms, repeats, every output alone, the sweep cap, the community subgraph; the modularity of arbitrary
labellings; isolation from the handle's other state, a matrix that is not symmetric, and the error paths.

Everything is equality (the modularity too: the bits of the restatement's loop), except the modularity against networkx, which is
within (C + 4) 2^-52, C the number of communities."""
import ctypes
import functools

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp

from test_core_host import GOLDEN, GOLDEN_IDS
from test_gpu_core import adjacency, complete_graph, engine_of, lanes_per_row
from test_truss_host import two_hubs
from test_communities_host import (COLOR_INTS, LPA_INTS, MOD_INTS, SMALL, chain, communities_of, fixture_case, graph_of, modularity_ref,
                                   path_graph, star_graph)

pytestmark = pytest.mark.gpu

_u32p = ctypes.POINTER(ctypes.c_uint32)
LZX_OK, LZX_ERR_ARG, LZX_ERR_LIMIT = 0, -1, -6
LPA_STAGE, LPA_TABLE_ROW = 128, 2048


def golden(name):
    return GOLDEN[GOLDEN_IDS.index(name)]


def run(eng, ties_by_id, **kw):
    """(color, colour integers, labels, propagation integers, Q) of the two calls"""
    color, cinfo = eng.color_raw(0, ties_by_id)
    labels, linfo = eng.label_propagation_raw(0, ties_by_id, **kw)
    assert color.dtype == np.uint32 and labels.dtype == np.uint32
    return color, {key: cinfo[key] for key in COLOR_INTS}, labels, {key: linfo[key] for key in LPA_INTS}, linfo["modularity"]


def check(eng, ref, ties_by_id):
    """both calls against the restatement's vectors, integers and modularity bits, and a separate lzx_modularity of the labels"""
    color, cints, labels, lints, q = run(eng, ties_by_id)
    assert np.array_equal(color, ref["color"])
    assert cints == {key: ref[key] for key in COLOR_INTS}
    assert np.array_equal(labels, ref["labels"])
    assert lints == {key: ref[key] for key in LPA_INTS}
    assert q == ref["q"]
    q2, minfo = eng.modularity_raw(labels)
    assert q2 == q and {key: minfo[key] for key in MOD_INTS} == {key: ref[key] for key in MOD_INTS}
    return color, cints, labels, lints, q


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4]


def assert_networkx(A, labels, q):
    G = graph_of(A)
    want = {frozenset(c) for c in nx.community.label_propagation_communities(G)}
    assert communities_of(labels) == want
    if A.nnz:
        assert abs(q - nx.community.modularity(G, [set(c) for c in want])) <= (len(want) + 4) * 2.0 ** -52


@functools.lru_cache(maxsize=None)
def case(name, ties_by_id):
    """(A, the restatement's chain) of a named graph, computed once and shared (read-only)"""
    if name in GOLDEN_IDS:
        A, by_id, hashed = fixture_case(golden(name))
        return A, by_id if ties_by_id else hashed
    makers = dict(SMALL, complete_200=lambda: complete_graph(200), star_4096=lambda: star_graph(4096), two_hubs=two_hubs,
                  star_129=lambda: star_graph(129), star_2048=lambda: star_graph(2048), star_2049=lambda: star_graph(2049),
                  empty_graph=lambda: sp.csr_matrix((5, 5)), single_vertex=lambda: sp.csr_matrix((1, 1)), one_edge=lambda: adjacency(2, [(0, 1)]))
    A = sp.csr_matrix(makers[name]())
    A.sort_indices()
    return A, chain(A, 0, ties_by_id)


# ---- 1. known answers and fixtures ------------------------------------------------------------------------------------------
KNOWN = {"path_65": dict(colors=2, rounds=64, sweeps=2, n_communities=32), "ring_of_cliques_12x6": dict(n_communities=11),
         "caveman_10x8": dict(n_communities=10, largest_size=8, largest_label=0), "planted_8x64": dict(),
         "k5_k10_and_7_isolated": dict(colors=10, n_communities=9, largest_size=10, largest_label=5), "one_edge": dict(colors=2, n_communities=1, entries=2),
         "empty_graph": dict(colors=1, rounds=1, largest_class=5, n_communities=5, sweeps=1, updates=0, entries=0),
         "single_vertex": dict(colors=1, rounds=1, n_communities=1, largest_size=1, largest_label=0)}


@pytest.mark.parametrize("name", list(KNOWN))
def test_known_answers(pkg, name):
    A, ref = case(name, True)
    for key, value in KNOWN[name].items():
        assert ref[key] == value, key
    eng = engine_of(pkg, A)
    _, _, labels, _, q = check(eng, ref, True)
    assert_networkx(A, labels, q)
    check(eng, case(name, False)[1], False)
    if not A.nnz:
        assert q == 0.0
    eng.close()


@pytest.mark.parametrize("ties_by_id", [True, False], ids=["by_id", "hashed"])
@pytest.mark.parametrize("name", GOLDEN_IDS)
def test_fixtures_against_the_restatement(pkg, name, ties_by_id):
    A, ref = case(name, ties_by_id)
    eng = engine_of(pkg, A)
    color, _, labels, lints, q = check(eng, ref, ties_by_id)
    assert not (color[A.nonzero()[0]] == color[A.nonzero()[1]]).any()
    if ties_by_id:
        assert_networkx(A, labels, q)
    parts = eng.label_propagation_communities(0, ties_by_id)
    assert len(parts) == lints["n_communities"] and len(parts[0]) == lints["largest_size"] and int(parts[0][0]) == lints["largest_label"]
    assert {frozenset(p.tolist()) for p in parts} == communities_of(labels)
    assert eng.modularity(parts) == q
    eng.close()


# ---- 2. the shapes where the kernels change -----------------------------------------------------------------------------------
# (graph, color_long_row or None, rows for the group launch, rows for the long-row launch)
COLOR_LAUNCHES = [("complete_65", None, True, False), ("complete_200", None, True, False), ("star_4096", None, True, True),
                  ("two_hubs", None, True, True), ("rmat_n3000_skew", 4, True, True)]


@pytest.mark.parametrize("name,long_row,short_rows,long_rows", COLOR_LAUNCHES, ids=[f"{c[0]}-{c[1]}" for c in COLOR_LAUNCHES])
def test_both_colour_launches(pkg, name, long_row, short_rows, long_rows):
    """A row is counted and coloured by a group of lanes when it has at most color_long_row entries (default: 64 times the lanes
    per row), by a workgroup with the LDS bitmap when it has more.  Which launch gets rows is asserted from the row lengths:
      complete_65, complete_200   the group launch alone; vertex number r of the order has r earlier neighbours with the colours
                                  0 .. r - 1, so the minimum-excluded-colour search walks r / 64 + 1 windows of 64 colours: up to
                                  two and up to four
      star_4096                   4 lanes, threshold 256: the hub by the long-row launch
      two_hubs                    4 lanes, threshold 256: the two rows of 311 entries by the long-row launch
      rmat_n3000_skew, 4          both
    Each is compared with the restatement, under both tie rules, and the forced run with the unforced one."""
    A, _ = case(name, True)
    lengths = np.diff(A.indptr)
    threshold = 64 * lanes_per_row(A) if long_row is None else long_row
    print(name, "threshold", threshold, "rows above it", int((lengths > threshold).sum()), "longest row", int(lengths.max()))
    assert bool((lengths <= threshold).any()) == short_rows and bool((lengths > threshold).any()) == long_rows
    if name.startswith("complete"):
        n = A.shape[0]
        assert case(name, True)[1]["colors"] == n == case(name, True)[1]["rounds"] and case(name, False)[1]["colors"] == n
    for ties_by_id in (True, False):
        ref = case(name, ties_by_id)[1]
        unforced = engine_of(pkg, A)
        first = check(unforced, ref, ties_by_id)
        unforced.close()
        if long_row is not None:
            forced = engine_of(pkg, A, color_long_row=long_row)
            assert same(run(forced, ties_by_id), first)
            forced.close()


def paths_of(A, group_row, table_row):
    """how many rows with an entry each propagation path gets: at most group_row entries, at most table_row, more"""
    lengths = np.diff(sp.csr_matrix(A).indptr)
    lengths = lengths[lengths > 0]
    short = lengths <= group_row
    medium = ~short & (lengths <= table_row)
    return int(short.sum()), int(medium.sum()), int((~short & ~medium).sum())


# (graph, lpa_group_row, lpa_table_row, which of the three paths get rows)
LPA_PATHS = [("star_128", None, None, (True, False, False)), ("star_129", None, None, (True, True, False)),
             ("star_2048", None, None, (True, True, False)), ("star_2049", None, None, (True, False, True)),
             ("rmat_n3000_skew", None, None, (True, True, False)), ("rmat_n3000_skew", 4, 8, (True, True, True)),
             ("rmat_n3000_skew", 1 << 20, 1 << 20, (True, False, False)), ("two_hubs", 4, 16, (True, True, True))]


@pytest.mark.parametrize("name,group_row,table_row,expect", LPA_PATHS, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in LPA_PATHS])
def test_the_three_propagation_paths(pkg, name, group_row, table_row, expect):
    """A row of at most lpa_group_row entries (128) is updated by a group of lanes that stages the labels in LDS, a longer one of
    at most lpa_table_row (2 048) by a workgroup over the LDS table, the rest over a table in global memory.  Which paths get
    rows is asserted from the row lengths:
      star_128, star_129     the hub's first sweep sees that many distinct labels: on both sides of the staging cap
      star_2048, star_2049   the hub in the LDS table at its fullest, and in a global table
      rmat_n3000_skew        unforced: groups and the LDS table; 4 / 8: all three paths; both 2^20: the groups alone, rows of
                             more than 128 entries read past the staged labels
      two_hubs, 4 / 16       all three: the leaves, the rows of 10 entries in the LDS table, those of 19 and 311 in global tables
    The new label is an arg-max under a total order, so every forced run equals the unforced run and the restatement."""
    A, _ = case(name, True)
    counts = paths_of(A, LPA_STAGE if group_row is None else group_row, LPA_TABLE_ROW if table_row is None else min(table_row, LPA_TABLE_ROW))
    if group_row == 1 << 20:
        assert int(np.diff(A.indptr).max()) > LPA_STAGE
    print(name, "rows per path", counts)
    assert tuple(c > 0 for c in counts) == expect
    for ties_by_id in (True, False):
        ref = case(name, ties_by_id)[1]
        unforced = engine_of(pkg, A)
        first = check(unforced, ref, ties_by_id)
        unforced.close()
        if group_row is not None:
            forced = engine_of(pkg, A, lpa_group_row=group_row, lpa_table_row=table_row)
            assert same(run(forced, ties_by_id), first)
            forced.close()


# ---- 3. other cases -----------------------------------------------------------------------------------------------------------
def test_isolated_vertices_and_self_loops(pkg):
    A, ref = case("rmat_n3000_skew", False)
    n = A.shape[0]
    assert (np.diff(A.indptr) == 0).any()
    coo = sp.triu(A).tocoo()
    loops = np.arange(0, n, 7)
    B = sp.csr_matrix(A + sp.csr_matrix((np.ones(len(loops)), (loops, loops)), shape=(n, n)))
    B.sort_indices()
    out = []
    for extra in (np.zeros(0, dtype=np.int64), loops):
        eng = pkg.Engine(0)
        eng.set_graph_edges(n, np.concatenate([coo.row, extra]), np.concatenate([coo.col, extra]))
        assert eng.info()["nnz"] == A.nnz + len(extra)
        out.append(check(eng, ref, False))
        eng.close()
    assert same(out[0], out[1])
    isolated = np.flatnonzero(np.diff(B.indptr) == 0)
    assert (out[1][0][isolated] == 0).all() and np.array_equal(out[1][2][isolated], isolated.astype(np.uint32))


def test_hand_over_form_does_not_matter(pkg):
    A, ref = case("er_n4000_deg20", False)
    for pb in (1, 0):
        eng = engine_of(pkg, A, propagation_blocking=pb)
        check(eng, ref, False)
        eng.close()


def test_two_calls_give_the_same_bits(pkg):
    A, ref = case("rmat_n4096", False)
    eng = engine_of(pkg, A)
    first = check(eng, ref, False)
    assert same(run(eng, False), first)
    other = eng.label_propagation_raw(12345)
    assert other[1]["sweeps"] >= 1 and eng.modularity(other[0]) == other[1]["modularity"]       # another seed is another order
    eng.close()


def test_counts_only_and_each_output_alone(pkg):
    A, ref = case("er_n1000", False)
    n = A.shape[0]
    eng = engine_of(pkg, A)
    cinfo, linfo = pkg.LzxColorInfo(), pkg.LzxCommunitiesInfo()
    assert eng.L.lzx_color(eng.h, 0, 0, None, ctypes.byref(cinfo)) == 0
    assert {key: getattr(cinfo, key) for key in COLOR_INTS} == {key: ref[key] for key in COLOR_INTS}
    assert eng.L.lzx_label_propagation(eng.h, 0, 0, 1000, None, ctypes.byref(linfo)) == 0
    assert {key: getattr(linfo, key) for key in LPA_INTS} == {key: ref[key] for key in LPA_INTS} and linfo.modularity == ref["q"]
    assert eng.L.lzx_color(eng.h, 0, 0, None, None) == 0 and eng.L.lzx_label_propagation(eng.h, 0, 0, 1000, None, None) == 0
    out = np.full(n, 0xdeadbeef, dtype=np.uint32)
    assert eng.L.lzx_color(eng.h, 0, 0, out.ctypes.data_as(_u32p), None) == 0 and np.array_equal(out, ref["color"])
    out = np.full(n, 0xdeadbeef, dtype=np.uint32)
    assert eng.L.lzx_label_propagation(eng.h, 0, 0, 1000, out.ctypes.data_as(_u32p), None) == 0 and np.array_equal(out, ref["labels"])
    q = ctypes.c_double(-1.0)
    assert eng.L.lzx_modularity(eng.h, out.ctypes.data_as(_u32p), ctypes.byref(q), None) == 0 and q.value == ref["q"]
    assert eng.color_raw(want_colors=False)[0] is None and eng.label_propagation_raw(want_labels=False)[0] is None
    assert np.array_equal(eng.greedy_color(), ref["color"])
    eng.close()


def test_the_sweep_cap(pkg):
    """max_sweeps = 1 on the path of 65, ties by id: LZX_ERR_LIMIT, with the labels and the info of the state after that sweep"""
    A = path_graph(65)
    ref = chain(A, 0, True, max_sweeps=1)
    assert ref["sweeps"] == 1 and not ref["converged"]
    eng = engine_of(pkg, A)
    labels = np.zeros(65, dtype=np.uint32)
    info = pkg.LzxCommunitiesInfo()
    assert eng.L.lzx_label_propagation(eng.h, 0, pkg.LZX_COLOR_TIES_BY_ID, 1, labels.ctypes.data_as(_u32p), ctypes.byref(info)) == LZX_ERR_LIMIT
    assert np.array_equal(labels, ref["labels"])
    assert {key: getattr(info, key) for key in LPA_INTS} == {key: ref[key] for key in LPA_INTS} and info.modularity == ref["q"]
    with pytest.raises(pkg.LzxError, match=r"\(-6\).*sweep 1 of at most 1"):
        eng.label_propagation_raw(0, True, max_sweeps=1)
    assert eng.L.lzx_label_propagation(eng.h, 0, 0, 0, None, None) == LZX_ERR_ARG             # max_sweeps == 0
    assert eng.L.lzx_label_propagation(eng.h, 0, 2, 10, None, None) == LZX_ERR_ARG            # an unknown flag
    assert eng.L.lzx_color(eng.h, 0, 6, None, None) == LZX_ERR_ARG
    check(eng, chain(A, 0, True), True)
    eng.close()


def test_the_community_subgraph(pkg):
    A, ref = case("planted_8x64", False)
    eng = engine_of(pkg, A)
    labels, info = eng.label_propagation_raw()
    assert np.array_equal(labels, ref["labels"])
    members = labels == info["largest_label"]
    assert int(members.sum()) == info["largest_size"]
    for which in (None, int(labels[-1])):
        keep = members if which is None else labels == which
        sub, old = eng.community(labels, which)
        assert np.array_equal(old, np.flatnonzero(keep).astype(old.dtype))
        S = sp.csr_matrix(A[keep][:, keep])
        S.sort_indices()
        rp, ci = sub.get_graph_csr()
        assert np.array_equal(rp, S.indptr.astype(np.uint64)) and np.array_equal(ci, S.indices.astype(np.uint32))
        sub.close()
    with pytest.raises(ValueError, match="no vertex has the label"):
        eng.community(labels, A.shape[0] + 5)
    eng.close()


# ---- 4. the modularity of arbitrary labellings ------------------------------------------------------------------------------------
def test_modularity_of_arbitrary_labellings(pkg):
    A, _ = case("rmat_n3000_skew", False)
    n = A.shape[0]
    G = graph_of(A)
    eng = engine_of(pkg, A)
    components = eng.components()[0]
    rng = np.random.default_rng(21)
    labellings = {"one_community": np.full(n, 7, dtype=np.uint32), "alone": np.arange(n, dtype=np.uint32), "components": components,
                  "random_40": rng.integers(0, 40, n).astype(np.uint32), "random_n": rng.integers(0, n, n).astype(np.uint32),
                  "by_degree": np.minimum(np.diff(A.indptr), n - 1).astype(np.uint32)}
    for name, labels in labellings.items():
        ref = modularity_ref(A, labels)
        q, info = eng.modularity_raw(labels)
        print(name, q, {key: info[key] for key in MOD_INTS})
        assert q == ref["q"] and {key: info[key] for key in MOD_INTS} == {key: ref[key] for key in MOD_INTS}, name
        parts = [set(c) for c in communities_of(labels)]
        assert abs(q - nx.community.modularity(G, parts)) <= (len(parts) + 4) * 2.0 ** -52, name
        assert eng.modularity([np.array(sorted(p)) for p in parts]) == modularity_ref(A, eng._labels_of(parts, "test"))["q"]
    assert eng.modularity(labellings["one_community"]) == 0.0
    bad = labellings["random_40"].copy()
    bad[17] = n
    with pytest.raises(pkg.LzxError, match=rf"\(-1\).*labels\[17\] = {n}\b"):
        eng.modularity(bad)
    with pytest.raises(ValueError, match="in no community"):
        eng.modularity([np.arange(n - 1)])
    empty = engine_of(pkg, sp.csr_matrix((6, 6)))
    assert empty.modularity(np.arange(6, dtype=np.uint32)) == 0.0
    empty.close()
    eng.close()


# ---- 5. isolation and errors ------------------------------------------------------------------------------------------------------
def test_a_chunked_decomposition_is_left_alone(pkg):
    A, ref = case("er_n1000", False)
    x0 = np.random.default_rng(8).standard_normal(A.shape[0])
    eng = engine_of(pkg, A)
    a_ref, b_ref, Q_ref, _, _ = eng.lanczos(x0, 20)
    eng.lanczos_prepare(x0, 20)
    eng.lanczos_run_steps(7)
    check(eng, ref, False)
    assert eng.lanczos_progress() == (7, 20)
    eng.lanczos_run_steps(13)
    a, b, Q = eng.lanczos_fetch(20, want_q=True)
    assert np.array_equal(a, a_ref) and np.array_equal(b, b_ref) and np.array_equal(Q, Q_ref)
    eng.close()


def test_the_resident_bases_are_left_alone(pkg):
    A, ref = case("rmat_n3000_skew", False)
    n = A.shape[0]
    rng = np.random.default_rng(9)
    x0, X0 = rng.standard_normal(n), rng.standard_normal((3, n))
    t, T = rng.standard_normal(12), rng.standard_normal((3, 12))
    eng = engine_of(pkg, A)
    eng.lanczos(x0, 12, want_q=False)
    eng.lanczos_multi(X0, 12)
    ans, ans_m = eng.multout(t), eng.multout_multi(T)
    check(eng, ref, False)
    assert np.array_equal(eng.multout(t), ans) and np.array_equal(eng.multout_multi(T), ans_m)
    alpha, beta, k_used, _ = eng.lanczos_probes(3, 0, 4, 12, keep_basis=True)
    Tp = pkg.slq_diag_coefficients(alpha, beta, k_used, n, 0.1, 0.0)
    diag = eng.probe_diag(Tp)
    assert np.array_equal(eng.greedy_color(), ref["color"])
    assert np.array_equal(eng.probe_diag(Tp), diag) and np.array_equal(eng.multout(t), ans)
    eng.close()


def test_a_matrix_that_is_not_symmetric_stays_within_its_memory(pkg):
    """The upper triangle of a path alone: symmetry is the caller's promise and is not checked, and the numbers of such a matrix
    mean nothing.  The calls return, their rounds and sweeps are bounded, and the handle still answers."""
    n = 1000
    eng = pkg.Engine(0)
    eng.set_graph_csr(np.minimum(np.arange(n + 1), n - 1).astype(np.uint64), np.arange(1, n, dtype=np.uint32))
    x = np.random.default_rng(4).standard_normal(n)
    y = eng.spmv(x)
    for flags in (0, pkg.LZX_COLOR_TIES_BY_ID):
        color, labels = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        cinfo, linfo = pkg.LzxColorInfo(), pkg.LzxCommunitiesInfo()
        rc = eng.L.lzx_color(eng.h, 0, flags, color.ctypes.data_as(_u32p), ctypes.byref(cinfo))
        assert rc in (LZX_OK, LZX_ERR_LIMIT)
        if rc == LZX_OK:
            assert cinfo.rounds <= n + 1 and cinfo.colors <= n and int(color.max()) < cinfo.colors
        rc = eng.L.lzx_label_propagation(eng.h, 0, flags, 50, labels.ctypes.data_as(_u32p), ctypes.byref(linfo))
        assert rc in (LZX_OK, LZX_ERR_LIMIT)
        if linfo.sweeps:
            assert linfo.sweeps <= 50 and int(labels.max()) < n
    q = ctypes.c_double()
    assert eng.L.lzx_modularity(eng.h, np.zeros(n, dtype=np.uint32).ctypes.data_as(_u32p), ctypes.byref(q), None) == LZX_OK
    assert np.array_equal(eng.spmv(x), y)
    eng.close()


def test_errors(pkg):
    eng = pkg.Engine(0)
    eng.n = 4
    for call in (lambda: eng.color_raw(), lambda: eng.label_propagation_raw(), lambda: eng.modularity(np.zeros(4, dtype=np.uint32))):
        with pytest.raises(pkg.LzxError, match=r"\(-3\).*no graph"):
            call()
    eng.close()
    A, ref = case("er_n1000", False)
    n = A.shape[0]
    even = lambda x: (x + 1) & ~1
    state = 16 * n + 20 * even(n) + 4 * even(3 * min(n, 65536)) + 64              # the header's formula; no row above 2 048 entries
    small = engine_of(pkg, A, lpa_state_bytes=state - 1)
    with pytest.raises(pkg.LzxError, match=rf"\(-4\).*needs {state} bytes"):
        small.label_propagation_raw()
    x = np.random.default_rng(3).standard_normal(n)
    y = small.spmv(x)
    assert np.array_equal(small.greedy_color(), ref["color"])                      # the colouring alone has no cap
    roomy = engine_of(pkg, A, lpa_state_bytes=state)
    check(roomy, ref, False)
    assert np.array_equal(roomy.spmv(x), y) and np.array_equal(small.spmv(x), y)
    roomy.close()
    small.close()
    # the global tables are part of the state: a star of 2 049 leaves needs 8 * 8 192 bytes more
    S, sref = case("star_2049", False)
    ns = S.shape[0]
    vertices = 16 * ns + 20 * even(ns) + 4 * even(3 * min(ns, 65536)) + 64
    tight = engine_of(pkg, S, lpa_state_bytes=vertices + 8 * 8192 - 1)
    with pytest.raises(pkg.LzxError, match=rf"\(-4\).*label tables of 1 rows.*needs {vertices + 8 * 8192} bytes"):
        tight.label_propagation_raw()
    tight.close()
    fits = engine_of(pkg, S, lpa_state_bytes=vertices + 8 * 8192)
    check(fits, sref, False)
    fits.close()
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(A.indptr.astype(np.uint64), A.indices.astype(np.uint32))
    for e in grp.engines:
        for call in (lambda: e.color_raw(), lambda: e.label_propagation_raw(), lambda: e.modularity(np.zeros(e.n, dtype=np.uint32))):
            with pytest.raises(pkg.LzxError, match=r"\(-3\).*communicator of 2"):
                call()
    grp.close()
