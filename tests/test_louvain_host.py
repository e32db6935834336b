"""CPU: Louvain communities (include/lzx.h: lzx_louvain) without a GPU -- the binding and the two struct layouts, the argument
errors that come back before a device is touched, and a numpy restatement `louvain_ref` of the header's definition: level graphs
with integer weights, the colouring of every level (greedy_color_ref of tests/test_communities_host.py), sweeps over the colour
classes with the gain G(c) = M k_ic - T_c k_i in integers, the guard that takes back a sweep which does not raise
Qnum = M I - sum tot^2, the aggregation.  The GPU tests use the same restatement as their reference.

Against networkx.community.louvain_communities (seeds 0 .. 4): where networkx returns one partition for all five seeds the
restatement returns it set for set under both tie rules; everywhere its modularity is at least networkx's smallest minus 0.02
(DESIGN.md section 25 records the deficits; the margin is twice the worst one seen, rounded up).  Everything else is an integer and
is compared by equality."""
import ctypes
import functools
import os
import re
import subprocess

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp

from test_core_host import GOLDEN, GOLDEN_IDS, load_fixture
from test_truss_host import adjacency, clique_edges
from test_communities_host import (communities_of, connected_caveman, graph_of, greedy_color_ref, modularity_ref, path_graph, ring_of_cliques,
                                   star_graph)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LZX_ERR_ARG = -1
LEVEL_INTS = ("nodes", "entries", "communities", "moves", "inner_entries", "sum_degree_sq", "colors", "color_rounds", "sweeps", "reverted", "capped")
INFO_INTS = ("n_communities", "largest_size", "largest_label", "levels", "sweeps", "moves", "inner_entries", "entries", "sum_degree_sq")
GROUP_ROW, TABLE_ROW = 128, 2048
MARGIN = 0.02


# ---- the restatement ------------------------------------------------------------------------------------------------------
def level_zero(A):
    """the level graph 0 of a scipy matrix: (n, row_ptr, col_idx, weights), rows sorted, every entry 1 and a diagonal entry 0"""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    rp, ci = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    return n, rp, ci, (rows != ci).astype(np.int64)


def paths_of_level(rp, group_row=GROUP_ROW, table_row=TABLE_ROW):
    """the rows of a level graph by the decide step's path: at most group_row stored entries, at most table_row, more"""
    lengths = np.diff(rp)
    short = lengths <= group_row
    medium = ~short & (lengths <= min(table_row, TABLE_ROW))
    return [int(short.sum()), int(medium.sum()), int((~short & ~medium).sum())]


def louvain_level(n, rp, ci, w, M, color, max_sweeps):
    """The sweeps of one level.  Returns (label, tot, record): record holds moves, inner_entries, sum_degree_sq, sweeps, reverted,
    capped and qnums, the Qnum before the first sweep and after every sweep that ran (a reverted one included)."""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    off = rows != ci
    k = np.zeros(n, dtype=np.int64)
    np.add.at(k, rows, w)
    d = np.bincount(rows[off], minlength=n)
    diagonal = int(w[~off].sum())
    label = np.arange(n, dtype=np.int64)
    tot = k.copy()
    classes = [np.flatnonzero(off & (color[rows] == c) & (d[rows] > 0)) for c in range(int(color.max()) + 1 if n else 0)]

    def integers():
        inner = diagonal + int(w[off & (label[rows] == label[ci])].sum())
        sq = sum(int(t) ** 2 for t in tot.tolist())
        return inner, sq, M * inner - sq

    inner, sq, qnum = integers()
    qnums = [qnum]
    sweeps = moves = accepted = reverted = capped = 0
    while True:
        if accepted == max_sweeps:
            capped = 1
            break
        saved = label.copy(), tot.copy()
        sweeps += 1
        moved = 0
        for entries in classes:
            if not len(entries):
                continue
            r, lab, wt = rows[entries], label[ci[entries]], w[entries]
            pair, inverse = np.unique(r * n + lab, return_inverse=True)
            kic = np.zeros(len(pair), dtype=np.int64)
            np.add.at(kic, inverse, wt)
            pr, pl = pair // n, pair % n
            a = label[pr]
            own = pl == a
            gain = M * kic - (tot[pl] - np.where(own, k[pr], 0)) * k[pr]
            stay = -(tot[label] - k) * k                       # G(a) with k_ia = 0 ...
            stay[pr[own]] = gain[own]                         # ... and where a occurs among the neighbours
            cand = np.flatnonzero(~own)
            order = cand[np.lexsort((pl[cand], -gain[cand], pr[cand]))]
            first = order[np.concatenate(([True], pr[order][1:] != pr[order][:-1]))] if len(order) else order
            go = first[gain[first] > stay[pr[first]]]
            i, to = pr[go], pl[go]
            np.subtract.at(tot, label[i], k[i])
            np.add.at(tot, to, k[i])
            label[i] = to
            moved += len(go)
        if moved == 0:
            break
        new_inner, new_sq, new_qnum = integers()
        qnums.append(new_qnum)
        if new_qnum <= qnum:
            label, tot = saved
            reverted = 1
            break
        inner, sq, qnum = new_inner, new_sq, new_qnum
        moves += moved
        accepted += 1
    return label, tot, dict(moves=moves, inner_entries=inner, sum_degree_sq=sq, sweeps=sweeps, reverted=reverted, capped=capped, qnums=qnums)


def canonical(label):
    """the smallest index of every label's members, per member"""
    n = len(label)
    first = np.full(max(int(label.max()) + 1 if n else 0, 1), n, dtype=np.int64)
    np.minimum.at(first, label, np.arange(n))
    return first[label]


def louvain_ref(A, seed=0, ties_by_id=False, max_sweeps=100, max_levels=32, group_row=GROUP_ROW, table_row=TABLE_ROW):
    """The header's definition of lzx_louvain.  Returns a dict: labels (n,) uint32, level_labels (levels, n) uint32, records (one dict per
    counted level with LEVEL_INTS, path_rows and qnums), graphs (the level graphs (n, row_ptr, col_idx, weights), the one the last level
    aggregated to included), the integers of INFO_INTS, and q."""
    A = sp.csr_matrix(A)
    n0, rp, ci, w = level_zero(A)
    n = n0
    M = int(w.sum())
    assert M < 2 ** 31
    comp = np.arange(n0, dtype=np.int64)                      # vertex -> node of the current level
    graphs, records, level_labels = [(n, rp, ci, w)], [], []
    while len(records) < max_levels:
        pattern = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))
        col = greedy_color_ref(pattern, seed, ties_by_id)
        label, tot, rec = louvain_level(n, rp, ci, w, M, col["color"].astype(np.int64), max_sweeps)
        occur = np.unique(label)
        C = len(occur)
        if C == n:
            break
        new = np.searchsorted(occur, label)
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
        keep = (rows != ci) if not records else np.ones(len(ci), dtype=bool)      # level 0's diagonal entries are dropped
        pair, inverse = np.unique(new[rows[keep]] * C + new[ci[keep]], return_inverse=True)
        w2 = np.zeros(len(pair), dtype=np.int64)
        np.add.at(w2, inverse, w[keep])
        p, q = pair // C, pair % C
        rec.update(nodes=n, entries=len(ci), communities=C, colors=col["colors"], color_rounds=col["rounds"],
                   path_rows=paths_of_level(rp, group_row, table_row))
        records.append(rec)
        comp = new[comp]
        level_labels.append(canonical(comp))
        n, rp, ci, w = C, np.concatenate(([0], np.cumsum(np.bincount(p, minlength=C)))).astype(np.int64), q, w2
        graphs.append((n, rp, ci, w))
    labels = level_labels[-1] if records else np.arange(n0, dtype=np.int64)
    sizes = np.bincount(labels, minlength=max(n0, 1))
    m = modularity_ref(A, labels) if n0 else dict(q=0.0, inner_entries=0, entries=0, sum_degree_sq=0)
    return dict(labels=labels.astype(np.uint32), level_labels=np.array(level_labels, dtype=np.uint32).reshape(len(records), n0), records=records,
                graphs=graphs, n_communities=int((sizes > 0).sum()) if n0 else 0, largest_size=int(sizes.max()) if n0 else 0,
                largest_label=int(np.argmax(sizes)) if n0 else 0, sweeps=sum(r["sweeps"] for r in records),
                moves=sum(r["moves"] for r in records), inner_entries=m["inner_entries"], entries=m["entries"], sum_degree_sq=m["sum_degree_sq"],
                q=m["q"], levels=len(records))


# ---- the graphs -------------------------------------------------------------------------------------------------------------
def pattern_of(G):
    A = sp.csr_matrix(nx.to_scipy_sparse_array(G, nodelist=range(G.number_of_nodes()), weight=None, format="csr"))
    A.data[:] = 1.0
    A.sort_indices()
    return A


def lfr1000():
    G = nx.LFR_benchmark_graph(1000, 3, 1.5, 0.1, average_degree=10, min_community=30, seed=10)
    G.remove_edges_from(list(nx.selfloop_edges(G)))
    return pattern_of(G)


def two_cliques_matched(size=300):
    """two K_size joined by a perfect matching: the coarse graph has a diagonal of size (size - 1) and an off-diagonal weight of size"""
    edges = clique_edges(range(size)) + clique_edges(range(size, 2 * size)) + [(k, size + k) for k in range(size)]
    return adjacency(2 * size, edges)


SMALL = {"karate": lambda: pattern_of(nx.karate_club_graph()), "caveman_10x8": lambda: connected_caveman(10, 8),
         "ring_of_cliques_12x6": lambda: pattern_of(nx.ring_of_cliques(12, 6)), "barbell_10": lambda: pattern_of(nx.barbell_graph(10, 0)),
         "planted_8x32": lambda: pattern_of(nx.planted_partition_graph(8, 32, 0.5, 0.02, seed=1)), "complete_20": lambda: pattern_of(nx.complete_graph(20)),
         "star_4097": lambda: star_graph(4097), "path_65": lambda: path_graph(65), "lfr1000": lfr1000}
ONE_PARTITION = ("caveman_10x8", "ring_of_cliques_12x6", "barbell_10", "planted_8x32", "complete_20", "star_4097")

# what the definition gives, ties by id / hashed with seed 0: per counted level (communities, sweeps, colours, reverted)
EXPECTED = {
    "karate": (((8, 4, 5, 0), (4, 2, 4, 0)),) * 2,
    "caveman_10x8": (((10, 3, 7, 0),),) * 2,
    "ring_of_cliques_12x6": (((12, 2, 6, 0),),) * 2,
    "barbell_10": (((2, 3, 10, 0),), ((2, 2, 10, 0),)),
    "planted_8x32": (((8, 3, 12, 0),), ((8, 4, 11, 0),)),
    "complete_20": (((1, 2, 20, 0),),) * 2,
    "star_4097": (((1, 2, 2, 0),),) * 2,
    "path_65": (((32, 2, 2, 0), (16, 2, 2, 0), (8, 2, 2, 0)), ((29, 2, 3, 0), (13, 3, 3, 0), (7, 2, 2, 1))),
    "lfr1000": (((9, 7, 8, 0),),) * 2,
    "er_c1_n10000": (((3031, 25, 10, 1), (17, 25, 21, 0), (15, 2, 17, 0)), ((3029, 26, 11, 1), (18, 39, 20, 0), (10, 2, 14, 0))),
    "er_n1000": (((303, 12, 7, 1), (30, 20, 12, 0), (13, 3, 20, 0)), ((317, 10, 7, 1), (35, 9, 11, 0), (16, 3, 23, 0))),
    "er_n4000_deg20": (((1229, 18, 10, 0), (16, 28, 19, 0), (15, 2, 16, 0)), ((902, 33, 10, 1), (28, 13, 17, 0), (12, 2, 24, 0), (11, 2, 12, 0))),
    "rmat_n3000_skew": (((956, 12, 45, 0), (766, 8, 32, 0), (761, 3, 16, 1)), ((926, 11, 45, 0), (769, 5, 29, 0), (760, 2, 17, 0))),
    "rmat_n4096": (((1623, 15, 26, 0), (1233, 6, 25, 0), (1214, 4, 21, 0)), ((1692, 18, 26, 0), (1235, 8, 26, 0), (1217, 3, 26, 0))),
    "star_ring_n1500": (((666, 45, 4, 0), (332, 2, 3, 0), (165, 3, 3, 0), (81, 4, 3, 0), (41, 2, 3, 0)),
                        ((573, 44, 4, 0), (226, 5, 4, 1), (86, 4, 4, 1), (36, 3, 4, 0)))}
REVERTS = ("er_n1000", "er_c1_n10000", "rmat_n3000_skew")


@functools.lru_cache(maxsize=None)
def louvain_case(name):
    """(A, louvain_ref by id, louvain_ref hashed with seed 0) of a named graph, computed once and shared (read-only)"""
    A = sp.csr_matrix(SMALL[name]() if name in SMALL else load_fixture(GOLDEN[GOLDEN_IDS.index(name)]))
    A.sort_indices()
    return A, louvain_ref(A, 0, True), louvain_ref(A, 0, False)


@functools.lru_cache(maxsize=None)
def networkx_runs(name):
    """networkx.community.louvain_communities for the seeds 0 .. 4: (the partitions as sets of frozensets, their modularities)"""
    G = graph_of(louvain_case(name)[0])
    parts = [nx.community.louvain_communities(G, seed=seed) for seed in range(5)]
    return [{frozenset(c) for c in p} for p in parts], [nx.community.modularity(G, p) for p in parts]


def assert_invariants(A, r):
    """what holds for every result: Qnum rises strictly over the accepted sweeps and over the levels, a sweep that was taken back did
    not raise it, every level's integers agree with its labelling, and the records add up"""
    n = A.shape[0]
    M = r["entries"]
    last = None
    for l, rec in enumerate(r["records"]):
        q = rec["qnums"]
        accepted = q[:-1] if rec["reverted"] else q
        assert all(y > x for x, y in zip(accepted, accepted[1:])), (l, q)
        if rec["reverted"]:
            assert q[-1] <= q[-2] and len(accepted) >= 2
        assert len(accepted) > 1 and rec["communities"] < rec["nodes"]
        if last is not None:
            assert accepted[0] == last                 # the aggregated graph has the Qnum its partition had
        last = accepted[-1]
        assert last == M * rec["inner_entries"] - rec["sum_degree_sq"]
        m = modularity_ref(A, r["level_labels"][l])
        assert (m["inner_entries"], m["sum_degree_sq"]) == (rec["inner_entries"], rec["sum_degree_sq"])
        assert len(np.unique(r["level_labels"][l])) == rec["communities"]
        assert rec["nodes"] == r["graphs"][l][0] and rec["entries"] == len(r["graphs"][l][2]) and sum(rec["path_rows"]) == rec["nodes"]
        assert int(r["graphs"][l + 1][3].sum()) == M and r["graphs"][l + 1][0] == rec["communities"]
    assert r["levels"] == len(r["records"]) and r["sweeps"] == sum(rec["sweeps"] for rec in r["records"])
    if r["levels"]:
        assert np.array_equal(r["labels"], r["level_labels"][-1]) and r["n_communities"] == r["records"][-1]["communities"]
        assert r["inner_entries"] == r["records"][-1]["inner_entries"] and r["sum_degree_sq"] == r["records"][-1]["sum_degree_sq"]
    assert (r["labels"] <= np.arange(n)).all() and (r["labels"][r["labels"]] == r["labels"]).all()


# ---- the binding ------------------------------------------------------------------------------------------------------------
def test_entry_point_is_bound(pkg):
    L = pkg.lib()
    names = [name for name, _, _ in pkg.SYMBOLS]
    header = open(os.path.join(ROOT, "include", "lzx.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    hooks = open(os.path.join(ROOT, "msc-hpc-final-project_amd", "csrc", "lzx_test_hooks.h")).read()
    assert "lzx_louvain" in names and hasattr(L, "lzx_louvain")
    assert re.search(r"\bint lzx_louvain\(", header) and re.search(r" T lzx_louvain\b", out)
    assert "lzx_louvain_level" in header and "lzx_louvain_info" in header
    assert "louvain_state_bytes" in pkg.SHAPE_OPTIONS and '"louvain_state_bytes"' in hooks
    assert "no Louvain" not in header
    for method in ("louvain_raw", "louvain_communities", "louvain_partitions"):
        assert hasattr(pkg.Engine, method)


LAYOUTS = [("LzxLouvainLevel", "lzx_louvain_level", 80, set(LEVEL_INTS) | {"path_rows"}),
           ("LzxLouvainInfo", "lzx_louvain_info", 104, set(INFO_INTS) | {"modularity", "loop_ms", "color_ms", "sweep_ms", "aggregate_ms"})]


@pytest.mark.parametrize("cls,struct,size,public", LAYOUTS, ids=[l[1] for l in LAYOUTS])
def test_struct_layouts_match_the_header(pkg, tmp_path, cls, struct, size, public):
    T = getattr(pkg, cls)
    fields = [f for f, _ in T._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "lzx.h"', "int main(void) {", f'printf("size %zu\\n", sizeof({struct}));']
    src += [f'printf("{f} %zu\\n", offsetof({struct}, {f}));' for f in fields]
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(T) == size
    for f in fields:
        assert int(got[f]) == getattr(T, f).offset, f
    assert set(T().as_dict()) == public == set(fields)


def test_argument_error_without_gpu(pkg):
    L = pkg.lib()
    assert L.lzx_louvain(None, 0, 0, 100, 32, None, None, None, None) == LZX_ERR_ARG
    msg = L.lzx_last_error().decode()
    assert "lzx_louvain" in msg and "null handle" in msg, msg


# ---- the restatement against networkx ---------------------------------------------------------------------------------------
ALL = list(SMALL) + GOLDEN_IDS


def test_every_graph_has_its_expected_values():
    assert sorted(EXPECTED) == sorted(ALL)


@pytest.mark.parametrize("name", ALL)
def test_restatement_against_networkx(name):
    A, by_id, hashed = louvain_case(name)
    parts, qs = networkx_runs(name)
    one = all(p == parts[0] for p in parts)
    assert one or name not in ONE_PARTITION
    for rule, r in (("by id", by_id), ("hashed", hashed)):
        print(f"{name} {rule}: Q {r['q']:.4f}, networkx {min(qs):.4f} .. {max(qs):.4f}, deficit {min(qs) - r['q']:+.4f}, levels",
              [(rec["nodes"], rec["communities"], rec["sweeps"], rec["colors"], rec["reverted"]) for rec in r["records"]])
        assert r["q"] >= min(qs) - MARGIN
        if name in ONE_PARTITION:
            assert communities_of(r["labels"]) == parts[0]
        assert abs(r["q"] - nx.community.modularity(graph_of(A), [set(c) for c in communities_of(r["labels"])])) <= (r["n_communities"] + 4) * 2.0 ** -52
        assert_invariants(A, r)
    got = tuple(tuple((rec["communities"], rec["sweeps"], rec["colors"], rec["reverted"]) for rec in r["records"]) for r in (by_id, hashed))
    assert got == EXPECTED[name]
    if name in ("complete_20", "star_4097"):
        assert by_id["n_communities"] == hashed["n_communities"] == 1
    if name == "planted_8x32":
        assert by_id["n_communities"] == 8 and sorted(len(c) for c in communities_of(by_id["labels"])) == [32] * 8


def test_the_guard_is_exercised():
    for name in REVERTS:
        _, by_id, hashed = louvain_case(name)
        assert any(rec["reverted"] for r in (by_id, hashed) for rec in r["records"]), name
    _, _, hashed = louvain_case("path_65")
    assert [rec["reverted"] for rec in hashed["records"]] == [0, 0, 1]


def test_weights_beyond_16_bits():
    """Two K_300 joined by a perfect matching.  Hashed ties find the two cliques, and the coarse graph has the diagonal 89 700.
    Ties by id do not: every colour class is one vertex of each clique, all gains of the first sweep tie, the smallest label wins on
    both sides of the matching and the cliques are mixed into 150 communities of modularity 0 -- what the definition gives, recorded
    here and in DESIGN.md section 25; networkx finds the cliques."""
    A = two_cliques_matched(300)
    r = louvain_ref(A, 0, False)
    n, rp, ci, w = r["graphs"][-1]
    assert n == 2 and rp.tolist() == [0, 2, 4] and ci.tolist() == [0, 1, 0, 1] and w.tolist() == [89700, 300, 300, 89700]
    assert r["n_communities"] == 2 and communities_of(r["labels"]) == {frozenset(range(300)), frozenset(range(300, 600))}
    assert_invariants(A, r)
    r = louvain_ref(A, 0, True)
    assert r["n_communities"] == 150 and abs(r["q"]) < 1e-15 and set(r["graphs"][-1][3].tolist()) == {8}
    assert_invariants(A, r)


def test_self_loops_and_isolated_vertices():
    A, by_id, hashed = louvain_case("rmat_n3000_skew")
    n = A.shape[0]
    isolated = np.flatnonzero(np.diff(A.indptr) == 0)
    assert len(isolated)
    loops = np.zeros(n)
    loops[::7] = 1.0
    B = sp.csr_matrix(A + sp.diags(loops))
    B.sort_indices()
    for ties_by_id, ref in ((True, by_id), (False, hashed)):
        r = louvain_ref(B, 0, ties_by_id)
        assert np.array_equal(r["labels"], ref["labels"]) and np.array_equal(r["level_labels"], ref["level_labels"]) and r["q"] == ref["q"]
        for a, b in zip(r["records"], ref["records"]):
            assert {k: a[k] for k in LEVEL_INTS if k != "entries"} == {k: b[k] for k in LEVEL_INTS if k != "entries"} and a["qnums"] == b["qnums"]
        assert r["records"][0]["entries"] == ref["records"][0]["entries"] + len(loops[::7])
        assert np.array_equal(r["labels"][isolated], isolated)


def test_the_caps():
    A = path_graph(65)
    full = louvain_ref(A, 0, True)
    one = louvain_ref(A, 0, True, max_levels=1)
    assert one["levels"] == 1 and np.array_equal(one["labels"], full["level_labels"][0]) and one["records"][0] == full["records"][0]
    capped = louvain_ref(A, 0, True, max_sweeps=1)
    assert all(rec["capped"] == 1 and rec["sweeps"] == 1 for rec in capped["records"]) and capped["levels"] >= 1
    assert_invariants(A, capped)
    empty = louvain_ref(sp.csr_matrix((5, 5)))
    assert empty["levels"] == 0 and empty["labels"].tolist() == list(range(5)) and empty["q"] == 0.0 and empty["n_communities"] == 5
