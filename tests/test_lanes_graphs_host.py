"""CPU: the graphs of tests/lanes_graphs.py reach what they were built to reach -- every hub length, the leaves' lengths, the three
residues of n, the long row first and last, the oriented lists of the complete graphs, the steps of the rule on the circulants --
and every restatement the GPU tests of tests/test_gpu_graph_lanes.py compare with is held to networkx (scipy for the
components) once on the ladder."""
import math
import time

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp

import lanes_graphs as lg
import test_communities_host as communities
import test_core_host as core
import test_similarity_host as similarity
import test_triangles_host as triangles
import test_truss_host as truss
from test_components_host import components_restatement, counts_of, scipy_labels
from test_sweep_host import EXPANSION, many_ties, sweep_ref

# stored entries per leaf of the ladder: 1 is the last leaf (the longest hub alone), 32 the leaves 1 and 2 (30 hubs and two neighbours
# on their path); 2, 25 and 28 do not occur (no leaf has one hub and one neighbour; the hub lengths leave those counts out)
LEAF_LENGTHS = sorted(set(range(1, 33)) - {2, 25, 28})


def test_the_hub_lengths_are_the_thirty_of_the_table():
    assert len(lg.HUB_LENGTHS) == 30 and lg.HUB_LENGTHS[0] == 2049 and lg.HUB_LENGTHS[-1] == 3
    for G in lg.WIDTHS:
        assert {G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 64 * G - 1, 64 * G, 64 * G + 1} <= set(lg.HUB_LENGTHS)
    assert {127, 128, 129} <= set(lg.HUB_LENGTHS)


@pytest.mark.parametrize("residue,reverse", lg.LADDERS, ids=[lg.ladder_name(*c) for c in lg.LADDERS])
def test_ladder_coverage_table(residue, reverse):
    A = lg.ladder(residue, reverse)
    n = A.shape[0]
    lengths = np.diff(A.indptr)
    hubs, leaves = lg.ladder_ids(residue, reverse)
    assert (A != A.T).nnz == 0 and A.diagonal().sum() == 0 and A.has_sorted_indices
    assert n % 64 == residue and 2189 <= n <= 2241 and A.nnz == 29834
    assert lengths[hubs].tolist() == list(lg.HUB_LENGTHS)
    assert sorted(set(lengths[leaves].tolist())) == LEAF_LENGTHS
    # the hub of T holds the leaves 0 .. T - 1 and nothing else
    for h, T in zip(hubs.tolist(), lg.HUB_LENGTHS):
        assert sorted(A.indices[A.indptr[h]:A.indptr[h + 1]].tolist()) == sorted(leaves[:T].tolist())
    lay = lg.ladder_layout(residue)
    assert int((lengths == 0).sum()) == lay["isolated"][1] - lay["isolated"][0] and (residue == 0 or (lengths == 0).any())
    cov = lg.coverage(A)
    assert cov["longest"] == 2049 and cov["first_is_longest"] == (not reverse) and cov["last_is_longest"] == reverse
    assert int((lengths == 2049).sum()) == 1
    for G in lg.WIDTHS:
        assert cov[G]["row_lengths"] and cov[G]["split"], G
        assert cov[G]["fill"] == residue % (256 // G)
    if reverse:
        assert n % 256 != 0 and all(n % (256 // G) != 0 for G in lg.WIDTHS + (64,))    # the long row's workgroup is never full
    assert lg.rule(A) == 8 and lg.rule(A, 64) == 8
    # apart from the ladder: the path of 70, K_40, nothing else
    labels = scipy_labels(A.indptr.astype(np.uint64), A.indices.astype(np.uint32))
    sizes = sorted(np.unique(labels, return_counts=True)[1].tolist(), reverse=True)
    assert sizes[:3] == [30 + lg.LEAVES, lg.SIDE_PATH, lg.CLIQUE] and set(sizes[3:]) <= {1}


def test_the_three_residues_fill_the_last_workgroup_three_ways():
    fills = {G: {lg.ladder(r).shape[0] % (256 // G) for r in lg.RESIDUES} for G in lg.WIDTHS + (64,)}
    for G, got in fills.items():
        assert got == {0, 1, 256 // G - 1}, G


@pytest.mark.parametrize("m", [200, 70])
def test_complete_graphs_have_every_oriented_length(m):
    A = lg.complete(m)
    r = triangles.triangles_oriented(A)
    assert sorted(r["out_degree"].tolist()) == list(range(m)) and r["oriented_max_degree"] == m - 1
    assert (r["tri"] == math.comb(m - 1, 2)).all() and (r["clustering"] == 1.0).all()
    # tri_long_list = 4: the stage is 128 entries; lists of 4 and 5 on both sides of the split, 127 .. 129 of the staging (K_200)
    assert {4, 5} <= set(r["out_degree"].tolist()) and ({127, 128, 129} <= set(r["out_degree"].tolist())) == (m == 200)
    # slices of the wide counting kernel: max(kmax / 64, 1)
    assert max((m - 1) // 64, 1) == {200: 3, 70: 1}[m]
    B = lg.two_cliques()
    assert B.shape[0] == 270 and set(np.diff(B.indptr).tolist()) == {69, 199}


def test_circulants_step_through_the_rule():
    assert len(lg.CIRCULANT_DEGREES) == len(lg.CIRCULANT_LANES) == 8
    for d, G in zip(lg.CIRCULANT_DEGREES, lg.CIRCULANT_LANES):
        A = lg.circulant(200, d // 2)
        assert set(np.diff(A.indptr).tolist()) == {d} and (A != A.T).nnz == 0
        assert lg.rule(A) == G and lg.rule(A, 64) == (64 if d == 64 else G)
    # the mean is taken over the rows that have an entry: 50 isolated vertices change nothing (over all rows 16 would give 12 -> 4 lanes)
    A = lg.circulant(200, 8, 50)
    assert A.shape[0] == 250 and lg.rule(A) == 16 and A.nnz // 250 == 12


@pytest.fixture(scope="module")
def ladder0():
    return lg.ladder(0, False)


def timed(what, f, *args):
    t0 = time.perf_counter()
    r = f(*args)
    print(f"{what}: {time.perf_counter() - t0:.3f} s")
    return r


def test_triangles_restatement_on_the_ladder(ladder0):
    r = timed("triangles_oriented", triangles.triangles_oriented, ladder0)
    triangles.assert_equals_networkx(r, triangles.networkx_reference(ladder0))
    # hub T closes a triangle with every pair of neighbouring leaves below T; K_40 has C(40, 3)
    pairs = sum(sum(1 for i in range(T - 1) if (i + 1) % lg.LEAF_PATH) for T in lg.HUB_LENGTHS)
    assert r["triangles"] == pairs + math.comb(40, 3) == 20611
    print("oriented_max_degree", r["oriented_max_degree"], "oriented mean", r["oriented_entries"] // int((np.diff(ladder0.indptr) > 0).sum()))


def test_core_restatement_on_the_ladder(ladder0):
    r = timed("peel_rounds", core.peel_rounds, ladder0)
    core.assert_equals_networkx(r, core.networkx_reference(ladder0))
    hubs, _ = lg.ladder_ids(0, False)
    print("rounds", r["rounds"], "levels", r["levels"], "degeneracy", r["degeneracy"])
    assert r["degeneracy"] == lg.CLIQUE - 1 and r["main_core_size"] == lg.CLIQUE
    assert (r["layer"][hubs] < r["rounds"]).all()          # every hub is a row of a window that is peeled


def test_truss_restatement_on_the_ladder(ladder0):
    r = timed("truss_rounds", truss.truss_rounds, ladder0)
    truss.assert_equals_networkx(ladder0, r)
    print("rounds", r["rounds"], "levels", r["levels"], "max_truss", r["max_truss"])
    assert r["max_truss"] == lg.CLIQUE and r["main_truss_edges"] == math.comb(lg.CLIQUE, 2)
    B = lg.two_cliques()
    rb = timed("truss_rounds, K_70 and K_200", truss.truss_rounds, B)
    truss.assert_equals_networkx(B, rb)
    assert (rb["rounds"], rb["levels"], rb["max_truss"]) == (2, 2, 200)


def test_components_restatement_on_the_ladder(ladder0):
    rp, ci = ladder0.indptr.astype(np.uint64), ladder0.indices.astype(np.uint32)
    labels, rounds = timed("components_restatement", components_restatement, rp, ci)
    want = scipy_labels(rp, ci)
    assert np.array_equal(labels, want)
    lay = lg.ladder_layout(0)
    assert counts_of(want) == (3 + lay["isolated"][1] - lay["isolated"][0], 30 + lg.LEAVES, 0)
    print("rounds", rounds)
    assert rounds >= 4                                      # the path of 70 is merged over several rounds


def test_communities_restatement_on_the_ladder(ladder0):
    by_id = timed("chain, ties by id", communities.chain, ladder0, 0, True)
    hashed = timed("chain, hashed", communities.chain, ladder0, 0, False)
    communities.assert_equals_networkx(ladder0, by_id, hashed)
    for r in (by_id, hashed):
        assert r["converged"] and r["colors"] == lg.CLIQUE
        print("colour rounds", r["rounds"], "sweeps", r["sweeps"], "communities", r["n_communities"])


def test_sweep_restatement_on_the_ladder(ladder0):
    n = ladder0.shape[0]
    G = communities.graph_of(ladder0)
    r = timed("sweep_ref", sweep_ref, ladder0, many_ties(n))
    order = r["order"].astype(np.int64)
    for k in (1, 7, n // 3, n // 2, n - 1):
        S = order[:k].tolist()
        assert int(r["cut"][k - 1]) == nx.cut_size(G, S) and int(r["vol"][k - 1]) == nx.volume(G, S), k
    assert r["value"] == nx.conductance(G, order[:r["k"]].tolist())
    x = sweep_ref(ladder0, many_ties(n), EXPANSION)
    assert x["value"] == nx.edge_expansion(G, x["order"][:x["k"]].tolist())


def test_similarity_restatement_on_the_ladder(ladder0):
    pairs = lg.ladder_pairs(0, False)
    assert len(pairs) == 435 + 200 + 200
    r = timed("similarity_restated", similarity.similarity_restated, ladder0, pairs)
    similarity.assert_equals_networkx(ladder0, pairs, r)
    # the leaf sets are nested: two hubs share the leaves of the shorter one
    hubs, _ = lg.ladder_ids(0, False)
    T = dict(zip(hubs.tolist(), lg.HUB_LENGTHS))
    assert r["common"][:435].tolist() == [min(T[u], T[v]) for u, v in pairs[:435].tolist()]
    assert r["shorter"][:435].tolist() == r["common"][:435].tolist()


def test_the_shape_and_its_read_backs_are_declared(pkg):
    root = core.ROOT
    csrc = lambda f: open(f"{root}/msc-hpc-final-project_amd/csrc/{f}").read()
    assert "graph_lanes" in pkg.SHAPE_OPTIONS and "graph_lanes" not in pkg.PRODUCT_OPTIONS
    hooks, api = csrc("lzx_test_hooks.h"), csrc("lzx_api.hip")
    for name in ("graph_lanes", "graph_lanes_rows", "graph_lanes_oriented"):
        assert f'"{name}"' in hooks and f'"{name}"' in api, name
    assert '{"graph_lanes", &lzx_ctx::graph_lanes_opt, OPT_SHAPE},' in api


def test_split_gadgets_against_networkx():
    A = lg.split_gadgets()
    lengths = np.diff(A.indptr)
    assert (A != A.T).nnz == 0 and lg.rule(A) == 4 and lg.SPLIT_LENGTHS == (256, 257, 512, 513, 1024, 1025, 2048, 2049)
    rc = timed("peel_rounds", core.peel_rounds, A)
    core.assert_equals_networkx(rc, core.networkx_reference(A))
    rt = timed("truss_rounds", truss.truss_rounds, A)
    truss.assert_equals_networkx(A, rt)
    assert (rc["rounds"], rt["rounds"]) == (5, 5)
    for T, (u, v, w) in lg.split_gadget_ids().items():
        assert lengths[u] == lengths[v] == T and lengths[w] == 20
        assert rc["layer"][[u, v, w]].tolist() == [3, 4, 4]                  # u in a round of its own, ahead of v and w
        assert [truss.value_of(A, rt["layer"], a, b) for a, b in ((u, v), (u, w), (v, w))] == [2, 3, 4]
        assert truss.value_of(A, rt["support"], u, v) == 1
