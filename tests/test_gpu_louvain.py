"""GPU: Louvain communities on the device (include/lzx.h: lzx_louvain; Engine.louvain_raw / louvain_communities /
louvain_partitions) against the numpy restatement of tests/test_louvain_host.py, which that file pins to networkx: labels, the labels
of every level, every integer of every level record and of the info, under both tie rules; the shapes at which the kernels change --
the three decide paths on level 0 and, forced, on the weighted levels, every lane width, the long-row colouring -- weights beyond 16
bits, isolated vertices, self loops, both hand-over forms, repeats, every output alone, the two caps, the community subgraph,
isolation from the handle's other state, the state cap at every allocation, a matrix that is not symmetric, and the error paths.

Everything is equality: the modularity too, with Engine.modularity of the labels and with the restatement's loop."""
import ctypes
import functools
import re

import numpy as np
import pytest
import scipy.sparse as sp

from test_core_host import GOLDEN_IDS
from test_gpu_core import adjacency, engine_of
from test_communities_host import communities_of, star_graph
from test_louvain_host import (GROUP_ROW, INFO_INTS, LEVEL_INTS, SMALL, TABLE_ROW, louvain_case, louvain_ref, path_graph, paths_of_level,
                               two_cliques_matched)

pytestmark = pytest.mark.gpu

_u32p = ctypes.POINTER(ctypes.c_uint32)
LZX_OK, LZX_ERR_ARG, LZX_ERR_LIMIT = 0, -1, -6


@functools.lru_cache(maxsize=None)
def case(name, ties_by_id):
    """(A, the restatement's result) of a named graph, computed once and shared (read-only)"""
    if name in SMALL or name in GOLDEN_IDS:
        A, by_id, hashed = louvain_case(name)
        return A, by_id if ties_by_id else hashed
    makers = dict(star_128=lambda: star_graph(128), star_129=lambda: star_graph(129), star_2048=lambda: star_graph(2048),
                  star_2049=lambda: star_graph(2049), two_cliques_matched=two_cliques_matched, empty_graph=lambda: sp.csr_matrix((5, 5)),
                  single_vertex=lambda: sp.csr_matrix((1, 1)), one_edge=lambda: adjacency(2, [(0, 1)]))
    A = sp.csr_matrix(makers[name]())
    A.sort_indices()
    return A, louvain_ref(A, 0, ties_by_id)


def run(eng, ties_by_id, **kw):
    """(labels, level_labels, the integers of the level records, their path_rows, the integers of the info, Q)"""
    labels, level_labels, levels, info = eng.louvain_raw(0, ties_by_id, **kw)
    assert labels.dtype == np.uint32 and level_labels.dtype == np.uint32 and level_labels.shape == (info["levels"], eng.n)
    return (labels, level_labels, [{key: rec[key] for key in LEVEL_INTS} for rec in levels], [rec["path_rows"] for rec in levels],
            {key: info[key] for key in INFO_INTS}, info["modularity"])


def check(eng, ref, ties_by_id, group_row=GROUP_ROW, table_row=TABLE_ROW, **kw):
    """one call against the restatement's vectors, integers and modularity bits, and a separate lzx_modularity of the labels"""
    labels, level_labels, records, path_rows, ints, q = got = run(eng, ties_by_id, **kw)
    assert np.array_equal(labels, ref["labels"]) and np.array_equal(level_labels, ref["level_labels"])
    assert records == [{key: rec[key] for key in LEVEL_INTS} for rec in ref["records"]]
    assert path_rows == [paths_of_level(g[1], group_row, table_row) for g in ref["graphs"][:ref["levels"]]]
    assert ints == {key: ref[key] for key in INFO_INTS}
    assert q == ref["q"] == eng.modularity(labels)
    return got


def same(a, b, path_rows=True):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and (a[3] == b[3] or not path_rows) and a[4] == b[4]
            and a[5] == b[5])


# ---- 1. known answers and fixtures ------------------------------------------------------------------------------------------
# (graph, counted levels by id / hashed or None, what else holds)
GRAPHS = [("karate", (2, 2)), ("path_65", (3, 3)), ("star_ring_n1500", (5, 4)), ("rmat_n3000_skew", (3, 3)), ("rmat_n4096", (3, 3)),
          ("er_n1000", (3, 3)), ("er_n4000_deg20", (3, 4)), ("lfr1000", (1, 1)), ("caveman_10x8", (1, 1)), ("planted_8x32", (1, 1)),
          ("complete_20", (1, 1)), ("one_edge", (1, 1)), ("empty_graph", (0, 0)), ("single_vertex", (0, 0))]


@pytest.mark.parametrize("ties_by_id", [True, False], ids=["by_id", "hashed"])
@pytest.mark.parametrize("name,levels", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_against_the_restatement(pkg, name, levels, ties_by_id):
    A, ref = case(name, ties_by_id)
    assert ref["levels"] == levels[0 if ties_by_id else 1]
    if name == "path_65" and not ties_by_id:
        assert [rec["reverted"] for rec in ref["records"]] == [0, 0, 1]
    if name == "star_ring_n1500":
        assert max(int(np.diff(g[1]).max()) for g in ref["graphs"][1:]) > GROUP_ROW      # a coarse row for the LDS table
    eng = engine_of(pkg, A)
    labels, level_labels, records, _, ints, q = check(eng, ref, ties_by_id)
    print(name, ints, q, [(rec["nodes"], rec["communities"], rec["sweeps"], rec["reverted"]) for rec in records])
    parts = eng.louvain_communities(0, ties_by_id)
    assert len(parts) == ints["n_communities"] and (not len(parts) or (len(parts[0]) == ints["largest_size"] and int(parts[0][0]) == ints["largest_label"]))
    assert {frozenset(p.tolist()) for p in parts} == communities_of(labels)
    if A.nnz:
        assert eng.modularity(parts) == q
    else:
        assert q == 0.0 and labels.tolist() == list(range(A.shape[0]))
    eng.close()


# ---- 2. the shapes where the kernels change -----------------------------------------------------------------------------------
LEVEL0_PATHS = [("star_128", (True, False, False)), ("star_129", (True, True, False)), ("star_2048", (True, True, False)),
                ("star_2049", (True, False, True)), ("star_4097", (True, False, True))]


@pytest.mark.parametrize("name,expect", LEVEL0_PATHS, ids=[c[0] for c in LEVEL0_PATHS])
def test_the_decide_paths_of_level_0(pkg, name, expect):
    """the hub of a star on both sides of the staging cap (128), of the LDS table's half (2 048), and far beyond it: the unweighted
    instantiation of each decide path; the star comes back as one community"""
    for ties_by_id in (True, False):
        A, ref = case(name, ties_by_id)
        assert tuple(c > 0 for c in ref["records"][0]["path_rows"]) == expect and ref["n_communities"] == 1
        eng = engine_of(pkg, A)
        check(eng, ref, ties_by_id)
        eng.close()


FORCED = [(4, 8), (4, 16), (1 << 20, 1 << 20)]
# the rows per path and level under each setting: the LDS table and the global tables get rows of weighted levels (karate level 1,
# rmat levels 1 and 2; the hub of star_ring on every level), and of level 0
FORCED_ROWS = {"karate": ([[24, 5, 5], [3, 5, 0]], [[24, 9, 1], [3, 5, 0]], [[34, 0, 0], [8, 0, 0]]),
               "planted_8x32": ([[0, 0, 256]], [[0, 37, 219]], [[256, 0, 0]]),
               "star_ring_n1500": ([[1499, 0, 1], [572, 0, 1], [225, 0, 1], [85, 0, 1]],) * 2 + ([[1500, 0, 0], [573, 0, 0], [226, 0, 0], [86, 0, 0]],),
               "rmat_n3000_skew": ([[1599, 382, 1019], [758, 17, 151], [749, 1, 19]], [[1599, 662, 739], [758, 68, 100], [749, 1, 19]],
                                   [[3000, 0, 0], [926, 0, 0], [769, 0, 0]])}


@pytest.mark.parametrize("name", ["karate", "planted_8x32", "star_ring_n1500", "rmat_n3000_skew"])
def test_the_coarse_levels_through_every_path(pkg, name):
    """lpa_group_row / lpa_table_row = 4 / 8 and 4 / 16 send the weighted level graphs' rows through the LDS table and the global
    tables, 2^20 / 2^20 sends every row to the groups of lanes (rows of more than 128 entries read past the staged labels).  The rows
    per path are asserted per level from the restatement's level graphs, and the labels are the same in all three settings."""
    A, ref = case(name, False)
    unforced = engine_of(pkg, A)
    first = check(unforced, ref, False)
    unforced.close()
    for group_row, table_row in FORCED:
        rows = [paths_of_level(g[1], group_row, table_row) for g in ref["graphs"][:ref["levels"]]]
        print(name, group_row, table_row, rows)
        assert rows == FORCED_ROWS[name][FORCED.index((group_row, table_row))]
        eng = engine_of(pkg, A, lpa_group_row=group_row, lpa_table_row=table_row)
        assert same(check(eng, ref, False, group_row, table_row), first, path_rows=False)
        eng.close()


@pytest.mark.parametrize("shape", [dict(graph_lanes=4), dict(graph_lanes=8), dict(graph_lanes=16), dict(graph_lanes=32), dict(color_long_row=4)],
                         ids=lambda s: "-".join(f"{k}-{v}" for k, v in s.items()))
def test_lane_widths_and_the_long_row_colouring(pkg, shape):
    A, ref = case("rmat_n3000_skew", False)
    eng = engine_of(pkg, A, **shape)
    check(eng, ref, False)
    eng.close()


def test_weights_beyond_16_bits(pkg):
    A, ref = case("two_cliques_matched", False)
    assert ref["graphs"][1][3].tolist() == [89700, 300, 300, 89700] and ref["n_communities"] == 2
    eng = engine_of(pkg, A)
    check(eng, ref, False)
    check(eng, case("two_cliques_matched", True)[1], True)
    eng.close()


# ---- 3. other cases -----------------------------------------------------------------------------------------------------------
def test_isolated_vertices_and_self_loops(pkg):
    A, ref = case("rmat_n3000_skew", False)
    n = A.shape[0]
    isolated = np.flatnonzero(np.diff(A.indptr) == 0)
    assert len(isolated)
    coo = sp.triu(A).tocoo()
    loops = np.arange(0, n, 7)
    B = sp.csr_matrix(A + sp.csr_matrix((np.ones(len(loops)), (loops, loops)), shape=(n, n)))
    B.sort_indices()
    looped = louvain_ref(B, 0, False)
    out = []
    for extra, r in ((np.zeros(0, dtype=np.int64), ref), (loops, looped)):
        eng = pkg.Engine(0)
        eng.set_graph_edges(n, np.concatenate([coo.row, extra]), np.concatenate([coo.col, extra]))
        assert eng.info()["nnz"] == A.nnz + len(extra)
        out.append(check(eng, r, False))
        eng.close()
    # the same result but for the stored entries and the row lengths of level 0
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][4] == out[1][4] and out[0][5] == out[1][5]
    assert out[0][2][1:] == out[1][2][1:] and out[1][2][0]["entries"] == out[0][2][0]["entries"] + len(loops)
    assert np.array_equal(out[1][0][isolated], isolated.astype(np.uint32))


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
    labels, _, levels, info = eng.louvain_raw(12345)                                       # another seed is another order
    assert info["levels"] == len(levels) >= 1 and eng.modularity(labels) == info["modularity"]
    eng.close()


def test_each_output_alone(pkg):
    A, ref = case("er_n1000", False)
    n, nl = A.shape[0], ref["levels"]
    eng = engine_of(pkg, A)
    info = pkg.LzxLouvainInfo()
    assert eng.L.lzx_louvain(eng.h, 0, 0, 100, 32, None, None, None, ctypes.byref(info)) == 0
    assert {key: getattr(info, key) for key in INFO_INTS} == {key: ref[key] for key in INFO_INTS} and info.modularity == ref["q"]
    assert eng.L.lzx_louvain(eng.h, 0, 0, 100, 32, None, None, None, None) == 0
    out = np.full(n, 0xdeadbeef, dtype=np.uint32)
    assert eng.L.lzx_louvain(eng.h, 0, 0, 100, 32, out.ctypes.data_as(_u32p), None, None, None) == 0 and np.array_equal(out, ref["labels"])
    rows = np.full((32, n), 0xdeadbeef, dtype=np.uint32)
    assert eng.L.lzx_louvain(eng.h, 0, 0, 100, 32, None, rows.ctypes.data_as(_u32p), None, None) == 0
    assert np.array_equal(rows[:nl], ref["level_labels"]) and (rows[nl:] == 0xdeadbeef).all()       # rows beyond the levels are left alone
    records = (pkg.LzxLouvainLevel * 32)()
    records[nl].nodes = 77
    assert eng.L.lzx_louvain(eng.h, 0, 0, 100, 32, None, None, records, None) == 0
    assert [{key: getattr(records[l], key) for key in LEVEL_INTS} for l in range(nl)] == [{key: rec[key] for key in LEVEL_INTS} for rec in ref["records"]]
    assert records[nl].nodes == 77
    got = eng.louvain_raw(want_labels=False, want_level_labels=False)
    assert got[0] is None and got[1] is None and len(got[2]) == nl
    eng.close()


def test_the_sweep_cap(pkg):
    """max_sweeps = 1: every level ends capped after its one accepted sweep; the result is valid and the restatement's"""
    A = path_graph(65)
    ref = louvain_ref(A, 0, True, max_sweeps=1)
    assert ref["levels"] >= 1 and all(rec["capped"] == 1 and rec["sweeps"] == 1 for rec in ref["records"])
    eng = engine_of(pkg, A)
    check(eng, ref, True, max_sweeps=1)
    check(eng, case("path_65", True)[1], True)
    eng.close()


def test_the_level_cap(pkg):
    A, ref = case("star_ring_n1500", False)
    one = louvain_ref(A, 0, False, max_levels=1)
    assert one["levels"] == 1 and np.array_equal(one["labels"], ref["level_labels"][0])
    eng = engine_of(pkg, A)
    labels = check(eng, one, False, max_levels=1)[0]
    assert np.array_equal(labels, check(eng, ref, False)[1][0])
    eng.close()


def test_partitions_and_the_community_subgraph(pkg):
    A, ref = case("karate", False)
    eng = engine_of(pkg, A)
    partitions = eng.louvain_partitions()
    assert len(partitions) == ref["levels"] == 2
    for parts, row, rec in zip(partitions, ref["level_labels"], ref["records"]):
        assert {frozenset(p.tolist()) for p in parts} == communities_of(row) and len(parts) == rec["communities"]
        assert [len(p) for p in parts] == sorted((len(p) for p in parts), reverse=True)
    assert all(any(set(fine.tolist()) <= set(coarse.tolist()) for coarse in partitions[1]) for fine in partitions[0])      # a dendrogram
    labels, _, _, info = eng.louvain_raw()
    members = labels == info["largest_label"]
    assert int(members.sum()) == info["largest_size"]
    sub, old = eng.community(labels)
    assert np.array_equal(old, np.flatnonzero(members).astype(old.dtype))
    S = sp.csr_matrix(A[members][:, members])
    S.sort_indices()
    rp, ci = sub.get_graph_csr()
    assert np.array_equal(rp, S.indptr.astype(np.uint64)) and np.array_equal(ci, S.indices.astype(np.uint32))
    assert sub.louvain_raw()[3]["entries"] == S.nnz
    sub.close()
    eng.close()


# ---- 4. isolation and errors ------------------------------------------------------------------------------------------------------
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
    eng.close()


def test_the_state_cap_at_every_allocation(pkg):
    """louvain_state_bytes one byte below what an allocation brings the state to: LZX_ERR_NOMEM with the bytes in the message.  The
    vertices' bytes are the header's formula; the later totals contain hipcub's scratch and are read from the message of the call
    that was refused there.  star_2049 has all four allocations: the arena, the hub's table, the aggregation's arrays, a level graph."""
    A, ref = case("star_2049", False)
    n = A.shape[0]
    even = lambda x: (x + 1) & ~1
    vertices = 16 * n + 56 * even(n) + 4 * even(3 * min(n, 65536)) + 128
    x = np.random.default_rng(3).standard_normal(n)
    caps, whats = [vertices], []
    for step in range(4):
        eng = engine_of(pkg, A, louvain_state_bytes=caps[-1] - 1)
        y = eng.spmv(x)
        with pytest.raises(pkg.LzxError, match=rf"\(-4\).*needs {caps[-1]} bytes") as err:
            eng.louvain_raw()
        whats.append(str(err.value))
        assert np.array_equal(eng.spmv(x), y)
        eng.close()
        eng = engine_of(pkg, A, louvain_state_bytes=caps[-1])
        if step == 3:
            check(eng, ref, False)
        else:
            with pytest.raises(pkg.LzxError, match=r"\(-4\).*needs (\d+) bytes") as err:
                eng.louvain_raw()
            caps.append(int(re.search(r"needs (\d+) bytes", str(err.value)).group(1)))
        eng.close()
    print(caps, whats)
    assert "state of" in whats[0] and "label tables of 1 rows" in whats[1] and "aggregation" in whats[2] and "level graph of 1 nodes and 1 entries" in whats[3]
    assert caps[1] == vertices + 8 * 8192                                         # the hub's table: pow2ceil(2 * 2049) slots of 8 bytes
    assert caps[2] >= caps[0] + 24 * A.nnz + 16                                  # the table is gone; keys, weights, hipcub's scratch
    assert caps[3] == caps[2] + 8 * 2 + 8 * 2                                    # row_ptr [2], one entry rounded up to two


def test_a_matrix_that_is_not_symmetric_stays_within_its_memory(pkg):
    """The upper triangle of a path alone: symmetry is the caller's promise and is not checked, and the numbers of such a matrix
    mean nothing.  The call returns and the handle still answers."""
    n = 1000
    eng = pkg.Engine(0)
    eng.set_graph_csr(np.minimum(np.arange(n + 1), n - 1).astype(np.uint64), np.arange(1, n, dtype=np.uint32))
    x = np.random.default_rng(4).standard_normal(n)
    y = eng.spmv(x)
    for flags in (0, pkg.LZX_COLOR_TIES_BY_ID):
        labels = np.zeros(n, dtype=np.uint32)
        info = pkg.LzxLouvainInfo()
        rc = eng.L.lzx_louvain(eng.h, 0, flags, 20, 8, labels.ctypes.data_as(_u32p), None, None, ctypes.byref(info))
        assert rc in (LZX_OK, LZX_ERR_LIMIT)
        if rc == LZX_OK:
            assert info.levels <= 8 and int(labels.max()) < n
    assert np.array_equal(eng.spmv(x), y)
    eng.close()


def test_errors(pkg):
    eng = pkg.Engine(0)
    eng.n = 4
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*no graph"):
        eng.louvain_raw()
    eng.close()
    A, ref = case("karate", False)
    eng = engine_of(pkg, A)
    for args in ((0, 2, 100, 32), (0, 0, 0, 32), (0, 0, 100, 0), (0, 0, 100, 65)):       # a flag, max_sweeps, max_levels
        assert eng.L.lzx_louvain(eng.h, *args, None, None, None, None) == LZX_ERR_ARG
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*max_levels must be 1 \.\. 64"):
        eng.louvain_raw(max_levels=65)
    check(eng, ref, False, max_levels=64)
    eng.close()
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(A.indptr.astype(np.uint64), A.indices.astype(np.uint32))
    for e in grp.engines:
        with pytest.raises(pkg.LzxError, match=r"\(-3\).*communicator of 2"):
            e.louvain_raw()
    grp.close()
