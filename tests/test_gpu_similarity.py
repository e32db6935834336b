"""GPU: the similarity of two vertices on the device (include/lzx.h: lzx_similarity; Engine.similarity_raw and the methods on top of
it): known answers on small graphs, the smallest shapes at which the walk can go wrong, every path forced, independence from the
batch, edges mode against pairs mode and against lzx_truss's supports, the golden fixtures through both hand-over forms, isolation
from the handle's other state, and the error paths.

Integers and the three ratios (one correctly rounded division of two integers) are compared by equality with the restatement of
tests/test_similarity_host.py.  A sum over c terms is compared with math.fsum of the Python terms within (2 c + 8) 2^-53, relative:
at most 2 2^-53 for the log on either side (math.log here, the device's log in the engine), one division on either side, c - 1
additions on either side.  A sum over no term is exactly 0.0.  Every check prints its worst observed error / bound."""
import ctypes
import functools
import itertools
import math

import numpy as np
import pytest
import scipy.sparse as sp

from test_similarity_host import GOLDEN, GOLDEN_IDS, RATIOS, SUMS, fixture_case, sample_pairs, similarity_restated, sum_error_ratio, without_loops
from test_truss_host import adjacency

pytestmark = pytest.mark.gpu

ALL = RATIOS + SUMS
PATHS = ("short_pairs", "long_pairs", "sliced_pairs")
SLICE_DEFAULT = 16384
u32p = ctypes.POINTER(ctypes.c_uint32)
f64p = ctypes.POINTER(ctypes.c_double)


def golden(name):
    return GOLDEN[GOLDEN_IDS.index(name)]


def engine_of(pkg, A, **options):
    eng = pkg.Engine(0, **options)
    A = sp.csr_matrix(A)
    A.sort_indices()
    eng.set_graph_csr(A.indptr.astype(np.uint64), A.indices.astype(np.uint32))
    return eng


def bits(out):
    """everything a call returns but the clocks, as bytes"""
    common, du, dv, values, info = out
    return (common.tobytes(), du.tobytes(), dv.tobytes(), tuple(values[m].tobytes() for m in ALL),
            tuple(info[k] for k in ("pairs", "walked", "max_common", "lanes") + PATHS))


def expected_paths(r, long_pair, slice_len):
    s = r["shorter"]
    return int((s <= long_pair).sum()), int(((s > long_pair) & (s <= slice_len)).sum()), int(((s > long_pair) & (s > slice_len)).sum())


def check(eng, pairs, r, label, long_pair=None, slice_len=SLICE_DEFAULT):
    """one call on `pairs` against the restatement r of the same pairs; returns what the call returned"""
    out = eng.similarity_raw(pairs)
    common, du, dv, values, info = out
    assert common.dtype == np.uint32 and np.array_equal(common, r["common"])
    assert np.array_equal(du, r["deg_u"]) and np.array_equal(dv, r["deg_v"])
    for m in RATIOS:
        assert values[m].dtype == np.float64 and np.array_equal(values[m], r[m]), m
    worst = 0.0
    for m, terms in (("adamic_adar", "terms_aa"), ("resource_allocation", "terms_ra")):
        for got, t in zip(values[m].tolist(), r[terms]):
            ratio = sum_error_ratio(got, t)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (m, got, math.fsum(t), len(t))
    long_pair = 64 * info["lanes"] if long_pair is None else long_pair
    print(f"{label}: {len(pairs)} pairs, largest c {info['max_common']}, sums' worst error / bound {worst:.4f}, lanes {info['lanes']}, "
          f"paths {[info[k] for k in PATHS]}, prep_ms {info['prep_ms']:.3f} count_ms {info['count_ms']:.3f}")
    assert info["pairs"] == len(pairs) and info["max_common"] == (int(r["common"].max()) if len(pairs) else 0)
    assert info["walked"] == int(r["shorter"].sum())
    assert tuple(info[k] for k in PATHS) == expected_paths(r, long_pair, slice_len)
    return out


def all_pairs(members):
    return np.array(list(itertools.combinations(members, 2)), dtype=np.int64)


# ---- 1. known answers -----------------------------------------------------------------------------------------------------
def test_complete_graph_70(pkg):
    """every pair is adjacent and has the other 68 vertices in common: more than a wavefront"""
    A = sp.csr_matrix(1.0 - np.eye(70))
    pairs = all_pairs(range(70))
    eng = engine_of(pkg, A)
    common, du, dv, values, _ = check(eng, pairs, similarity_restated(A, pairs), "K_70")
    assert (common == 68).all() and (du == 69).all() and (dv == 69).all()
    assert (values["jaccard"] == 68 / 70).all() and (values["overlap"] == 68 / 69).all() and (values["sorensen"] == 136 / 138).all()
    # (the 68 equal terms of a sum fall to the lanes by their place in the walked row, u and v left out: not every pair rounds alike)
    assert np.array_equal(eng.preferential_attachment(pairs), np.full(len(pairs), 69 * 69, dtype=np.int64))
    assert np.array_equal(eng.cosine_similarity(pairs), np.full(len(pairs), 68 / math.sqrt(69 * 69)))
    eng.close()


def test_complete_bipartite_5_90(pkg):
    label = np.repeat([0, 1], [5, 90])
    A = sp.csr_matrix((label[:, None] != label[None, :]).astype(np.float64))
    pairs = np.concatenate([all_pairs(range(5)), all_pairs(range(5, 95))[::7], np.array([(a, b) for a in range(5) for b in range(5, 95, 11)])])
    eng = engine_of(pkg, A)
    common, _, _, values, _ = check(eng, pairs, similarity_restated(A, pairs), "K_5,90")
    small, large = (pairs < 5).all(axis=1), (pairs >= 5).all(axis=1)
    assert (common[small] == 90).all() and (common[large] == 5).all() and not common[~small & ~large].any()
    assert (values["jaccard"][small] == 1.0).all() and (values["jaccard"][large] == 1.0).all()
    for m in ALL:
        assert not values[m][~small & ~large].any() and not np.signbit(values[m]).any(), m
    eng.close()


@pytest.mark.parametrize("leaves", [299, 300])
def test_star(pkg, leaves):
    A = adjacency(leaves + 1, [(0, k) for k in range(1, leaves + 1)])
    pairs = np.concatenate([all_pairs(range(1, leaves + 1))[::53], [(0, 1), (leaves, 0)]])
    eng = engine_of(pkg, A)
    common, _, _, values, _ = check(eng, pairs, similarity_restated(A, pairs), f"star with {leaves} leaves")
    assert (common[:-2] == 1).all() and not common[-2:].any()
    assert (values["resource_allocation"][:-2] == 1.0 / leaves).all() and (values["jaccard"][:-2] == 1.0).all()
    assert np.allclose(values["adamic_adar"][:-2], 1.0 / math.log(leaves), rtol=1e-15, atol=0)
    eng.close()


def test_path_65(pkg):
    A = adjacency(65, [(k, k + 1) for k in range(64)])
    pairs = np.array([(k, k + 1) for k in range(64)] + [(k, k + 2) for k in range(63)] + [(k + 3, k) for k in range(62)] + [(0, 64)])
    eng = engine_of(pkg, A)
    common, _, _, values, _ = check(eng, pairs, similarity_restated(A, pairs), "path of 65")
    assert np.array_equal(common, np.repeat([0, 1, 0], [64, 63, 63]))
    assert (values["resource_allocation"][64:127] == 0.5).all() and values["jaccard"][64] == 1 / 2 and values["jaccard"][65] == 1 / 3
    eng.close()


def test_two_isolated_vertices(pkg):
    eng = engine_of(pkg, sp.csr_matrix((2, 2)))
    common, du, dv, values, info = eng.similarity_raw([(0, 1), (1, 0)])
    assert not common.any() and not du.any() and not dv.any() and info["max_common"] == 0 and info["walked"] == 0
    for m in ALL:
        assert values[m].tobytes() == np.zeros(2).tobytes(), m
    common, _, _, values, info = eng.similarity_raw(None)              # edges mode on a graph without an entry
    assert len(common) == 0 and all(len(values[m]) == 0 for m in ALL) and info["pairs"] == 0
    eng.close()


def test_wheel(pkg):
    rim = 64
    A = adjacency(rim + 1, [(0, k) for k in range(1, rim + 1)] + [(k, k % rim + 1) for k in range(1, rim + 1)])
    pairs = np.array([(0, k) for k in range(1, rim + 1)] + [(k, k % rim + 1) for k in range(1, rim + 1)] + [(k, (k + 1) % rim + 1) for k in range(1, rim + 1)]
                     + [(1, 30)])
    eng = engine_of(pkg, A)
    common, _, _, _, _ = check(eng, pairs, similarity_restated(A, pairs), "wheel")
    assert np.array_equal(common, np.repeat([2, 1, 2, 1], [rim, rim, rim, 1]))
    eng.close()


# ---- 2. the smallest shapes at which the walk goes wrong ------------------------------------------------------------------
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def comb_graph():
    """vertex a_k (k = its place in LENGTHS) is joined to the first LENGTHS[k] of 65 targets: rows of length 0, 1 and G - 1, G, G + 1 for
    every G, and c(a_j, a_k) = the smaller of the two lengths.  The targets follow the a's."""
    na = len(LENGTHS)
    return adjacency(na + 65, [(k, na + t) for k, L in enumerate(LENGTHS) for t in range(L)])


def test_row_lengths_around_the_lanes(pkg):
    A = comb_graph()
    na = len(LENGTHS)
    pairs = np.concatenate([all_pairs(range(na)), all_pairs(range(na))[:, ::-1], [(k, na) for k in range(na)], [(na + 64, na)]])
    r = similarity_restated(A, pairs)
    assert np.array_equal(r["common"][:na * (na - 1) // 2], [min(LENGTHS[j], LENGTHS[k]) for j, k in itertools.combinations(range(na), 2)])
    eng = engine_of(pkg, A)
    _, _, _, _, info = check(eng, pairs, r, "comb")
    G = info["lanes"]
    assert {G - 1, G, G + 1} <= set(LENGTHS) and G in (4, 8, 16, 32)
    eng.close()


def test_first_and_last_entries_and_equal_lengths(pkg):
    """(10, 11): the only common neighbour is the first entry of both rows; (12, 13): the last entry of both; every one of these
    rows has three entries; (14, 15) are adjacent with one more common neighbour, (16, 17) adjacent with none"""
    A = adjacency(100, [(10, 0), (10, 20), (10, 21), (11, 0), (11, 30), (11, 31),
                        (12, 40), (12, 41), (12, 99), (13, 50), (13, 51), (13, 99),
                        (14, 15), (14, 60), (14, 61), (15, 60), (15, 62), (16, 17), (16, 70), (17, 71)])
    pairs = np.array([(10, 11), (11, 10), (12, 13), (13, 12), (14, 15), (15, 14), (16, 17), (17, 16), (10, 12), (0, 99), (20, 21)])
    r = similarity_restated(A, pairs)
    assert r["common"].tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1]
    eng = engine_of(pkg, A)
    check(eng, pairs, r, "first / last / equal")
    eng.close()


# ---- 3. every path --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def skew_case():
    """rmat_n3000_skew with its sampled pairs and every pair among its twelve vertices of largest degree"""
    A, pairs, _ = fixture_case(golden("rmat_n3000_skew"))
    hubs = np.argsort(-np.diff(A.indptr), kind="stable")[:12]
    pairs = np.concatenate([pairs, all_pairs(hubs.tolist())])
    return A, pairs, similarity_restated(A, pairs)


SETTINGS = {"long_1": dict(sim_long_pair=1), "default": {}, "huge": dict(sim_long_pair=1 << 30),
            "sliced_16": dict(sim_long_pair=1, sim_slice=16), "sliced_2": dict(sim_long_pair=1, sim_slice=2),
            "slice_below_long": dict(sim_long_pair=100, sim_slice=16)}


def test_every_path_forced(pkg):
    """sim_long_pair = 1 sends every pair whose shorter row has two entries or more to a workgroup of its own, 2^30 none; sim_slice = 16
    cuts the walked rows of up to 1000 entries into several slices, sim_slice = 2 into the 64 at the most.  The counts are the same on
    every path, the sums stay within the bound, and within one setting two calls give the same bits."""
    A, pairs, r = skew_case()
    assert r["shorter"].max() > 16 * 16 and r["common"].max() > 256
    seen = {}
    for name, shapes in SETTINGS.items():
        eng = engine_of(pkg, A, **shapes)
        first = check(eng, pairs, r, name, long_pair=shapes.get("sim_long_pair"), slice_len=shapes.get("sim_slice", SLICE_DEFAULT))
        assert bits(eng.similarity_raw(pairs)) == bits(first), name
        seen[name] = first
        eng.close()
    assert seen["long_1"][4]["long_pairs"] > 400 and seen["huge"][4]["long_pairs"] == 0 and seen["default"][4]["sliced_pairs"] == 0
    assert seen["sliced_16"][4]["sliced_pairs"] > 100 and seen["sliced_2"][4]["sliced_pairs"] > seen["sliced_16"][4]["sliced_pairs"]
    assert 0 < seen["slice_below_long"][4]["sliced_pairs"] < seen["sliced_16"][4]["sliced_pairs"] and seen["slice_below_long"][4]["long_pairs"] == 0


def shared_leaves_graph(k_short, k_long):
    """hubs 0, 1 share k_short leaves, hubs 2, 3 share k_long: four rows of exactly those lengths in a graph of mean degree below 8"""
    edges = [(h, 4 + t) for h in (0, 1) for t in range(k_short)] + [(h, 4 + k_short + t) for h in (2, 3) for t in range(k_long)]
    return adjacency(4 + k_short + k_long, edges)


def test_the_default_threshold(pkg):
    """mean degree below 8: four lanes per pair, so a shorter row of 256 entries is the last one a group of lanes takes"""
    A = shared_leaves_graph(256, 257)
    pairs = np.array([(0, 1), (2, 3), (3, 2), (0, 2), (4, 5), (4, 4 + 256)])
    r = similarity_restated(A, pairs)
    assert r["common"].tolist() == [256, 257, 257, 0, 2, 0] and r["shorter"].tolist() == [256, 257, 257, 256, 2, 2]
    eng = engine_of(pkg, A)
    _, _, _, _, info = check(eng, pairs, r, "threshold")
    assert info["lanes"] == 4 and (info["short_pairs"], info["long_pairs"]) == (4, 2)
    eng.close()


# ---- 4. independence from the batch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["default", "long_1", "sliced_16"])
def test_a_pair_does_not_depend_on_its_batch(pkg, setting):
    A, pairs, r = skew_case()
    best = int(np.argmax(r["common"]))
    u, v = pairs[best].tolist()
    eng = engine_of(pkg, A, **SETTINGS[setting])
    alone = eng.similarity_raw([(u, v)])
    assert alone[0][0] == r["common"][best] > 256

    def same(out, at):
        return (out[0][at] == alone[0][0] and out[1][at] == alone[1][0] and out[2][at] == alone[2][0]
                and all(out[3][m][at:at + 1].tobytes() == alone[3][m].tobytes() for m in ALL))

    repeated = eng.similarity_raw([(u, v)] * 7 + [pairs[0].tolist()] + [(u, v)] * 3)
    assert all(same(repeated, at) for at in (0, 3, 6, 8, 10))
    swapped = eng.similarity_raw([(v, u)])
    assert swapped[1][0] == alone[2][0] and swapped[2][0] == alone[1][0] and swapped[0][0] == alone[0][0]
    assert all(swapped[3][m].tobytes() == alone[3][m].tobytes() for m in ALL)
    batch = np.concatenate([pairs[:613], [(v, u)], pairs[:385], [(u, v)]])
    assert len(batch) == 1000
    big = eng.similarity_raw(batch)
    assert same(big, 999) and big[0][613] == alone[0][0] and all(big[3][m][613:614].tobytes() == alone[3][m].tobytes() for m in ALL)
    eng.close()


# ---- 5. edges mode --------------------------------------------------------------------------------------------------------
def with_loops(A, every=7):
    n = A.shape[0]
    loops = np.zeros(n)
    loops[::every] = 1.0
    B = sp.csr_matrix(A + sp.diags(loops))
    B.sort_indices()
    return B


@pytest.mark.parametrize("name,loops,shapes", [("rmat_n4096", False, {}), ("er_n1000", True, {}), ("rmat_n3000_skew", True, dict(sim_long_pair=8, sim_slice=64))])
def test_edges_mode(pkg, name, loops, shapes):
    A = without_loops(fixture_case(golden(name))[0])
    if loops:
        A = with_loops(A)
    n = A.shape[0]
    eng = engine_of(pkg, A, **shapes)
    rp, ci = eng.get_graph_csr()
    assert np.array_equal(rp, A.indptr.astype(np.uint64)) and np.array_equal(ci, A.indices.astype(np.uint32))
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    off = rows != ci
    assert (~off).sum() == (len(range(0, n, 7)) if loops else 0)
    common, du, dv, values, info = eng.similarity_raw(None)
    assert len(common) == A.nnz == info["pairs"]
    # the bits of pairs mode over the same entries
    pc, pdu, pdv, pvalues, pinfo = eng.similarity_raw(np.stack([rows[off], ci[off]], axis=1))
    assert np.array_equal(common[off], pc) and np.array_equal(du[off], pdu) and np.array_equal(dv[off], pdv)
    for m in ALL:
        assert values[m][off].tobytes() == pvalues[m].tobytes(), m
        assert not values[m][~off].any() and not np.signbit(values[m][~off]).any(), m
    assert not common[~off].any() and not du[~off].any() and not dv[~off].any()
    # each edge is intersected once
    assert 2 * info["walked"] == pinfo["walked"] and 2 * sum(info[k] for k in PATHS) == off.sum() and info["max_common"] == pinfo["max_common"]
    # the two copies of an edge
    for m in ALL:
        M = eng._edge_matrix(values[m])
        assert (M != M.T).nnz == 0, m
        assert np.array_equal(eng.edge_similarity(m).data, values[m])
    # lzx_truss's supports, entry for entry
    support = eng.edge_support()
    assert np.array_equal(common, support.data) and np.array_equal(eng.edge_similarity("common_neighbors").data, support.data)
    # a sample against the restatement
    pick = np.flatnonzero(off)[:: max(int(off.sum()) // 300, 1)]
    r = similarity_restated(A, np.stack([rows[pick], ci[pick]], axis=1))
    assert np.array_equal(common[pick], r["common"])
    worst = max(sum_error_ratio(got, t) for got, t in zip(values["adamic_adar"][pick].tolist(), r["terms_aa"]))
    print(f"edges mode on {name}: {A.nnz} entries, paths {[info[k] for k in PATHS]}, worst error / bound {worst:.4f}, count_ms {info['count_ms']:.3f}")
    assert worst <= 1.0 and np.array_equal(values["jaccard"][pick], r["jaccard"])
    if shapes:
        assert info["long_pairs"] > 0 and info["sliced_pairs"] > 0
    eng.close()


# ---- 6. fixtures, both hand-over forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=GOLDEN_IDS)
def test_fixtures_through_both_hand_over_forms(pkg, path):
    A, pairs, r = fixture_case(path)
    n = A.shape[0]
    by_csr = engine_of(pkg, A)
    first = check(by_csr, pairs, r, "csr")
    coo = sp.triu(A).tocoo()
    by_edges = pkg.Engine(0)
    by_edges.set_graph_edges(n, coo.row, coo.col)
    second = check(by_edges, pairs, r, "edge list")
    assert bits(first) == bits(second)
    # the methods on top
    some = pairs[:64]
    assert np.array_equal(by_csr.common_neighbors_count(some), r["common"][:64])
    assert np.array_equal(by_csr.jaccard_coefficient(some), r["jaccard"][:64]) and np.array_equal(by_csr.overlap_coefficient(some), r["overlap"][:64])
    assert np.array_equal(by_csr.sorensen_coefficient(some.tolist()), r["sorensen"][:64])
    assert by_csr.adamic_adar_index(some).tobytes() == first[3]["adamic_adar"][:64].tobytes()
    assert by_csr.resource_allocation_index(some).tobytes() == first[3]["resource_allocation"][:64].tobytes()
    pa = by_csr.preferential_attachment(some)
    assert pa.dtype == np.int64 and np.array_equal(pa, r["preferential_attachment"][:64])
    assert np.array_equal(by_csr.cosine_similarity(some), r["cosine"][:64])
    for bad in ([(0, n)], [(-1, 0)], [(3, 3)], [(0.5, 1.0)], [0, 1, 2]):
        with pytest.raises(ValueError):
            by_csr.jaccard_coefficient(bad)
    with pytest.raises(ValueError):
        by_csr.similarity_raw(some, measures=("cosine",))
    by_csr.close()
    by_edges.close()


def test_only_what_is_asked_for(pkg):
    A, pairs, r = fixture_case(golden("er_n4000_deg20"))
    eng = engine_of(pkg, A)
    common, du, dv, values, _ = eng.similarity_raw(pairs, measures=("resource_allocation", "overlap"), want_common=False)
    assert common is None and list(values) == ["overlap", "resource_allocation"] and np.array_equal(values["overlap"], r["overlap"])
    full = eng.similarity_raw(pairs)
    assert values["resource_allocation"].tobytes() == full[3]["resource_allocation"].tobytes() and np.array_equal(du, r["deg_u"])
    common, du, dv, values, info = eng.similarity_raw(pairs, measures=(), want_degrees=False)
    assert du is None and dv is None and values == {} and np.array_equal(common, r["common"]) and info["max_common"] == r["common"].max()
    info = pkg.LzxSimilarityInfo()
    pu, pv = np.ascontiguousarray(pairs[:, 0], dtype=np.uint32), np.ascontiguousarray(pairs[:, 1], dtype=np.uint32)
    assert eng.L.lzx_similarity(eng.h, len(pairs), pu.ctypes.data_as(u32p), pv.ctypes.data_as(u32p), 0, None, None, None, None, ctypes.byref(info)) == 0
    assert info.max_common == r["common"].max() and info.walked == r["shorter"].sum()
    assert eng.L.lzx_similarity(eng.h, len(pairs), pu.ctypes.data_as(u32p), pv.ctypes.data_as(u32p), 0, None, None, None, None, None) == 0
    eng.close()


# ---- 7. isolation ---------------------------------------------------------------------------------------------------------
def test_a_chunked_decomposition_is_left_alone(pkg):
    A, pairs, r = fixture_case(golden("er_n1000"))
    x0 = np.random.default_rng(8).standard_normal(A.shape[0])
    eng = engine_of(pkg, A)
    a_ref, b_ref, Q_ref, _, _ = eng.lanczos(x0, 20)
    eng.lanczos_prepare(x0, 20)
    eng.lanczos_run_steps(7)
    before = eng.similarity_raw(pairs)
    assert np.array_equal(before[0], r["common"])
    assert eng.lanczos_progress() == (7, 20)
    eng.lanczos_run_steps(13)
    a, b, Q = eng.lanczos_fetch(20, want_q=True)
    assert np.array_equal(a, a_ref) and np.array_equal(b, b_ref) and np.array_equal(Q, Q_ref)
    assert bits(eng.similarity_raw(pairs)) == bits(before)
    assert bits(eng.similarity_raw(None)) == bits(eng.similarity_raw(None))
    eng.close()


# ---- 8. errors ------------------------------------------------------------------------------------------------------------
def first_state_bytes(n, npairs, nsums=2, nm=5, ndeg=2):
    """the header's first allocation: tables, values, partials, degrees, pairs, counts, degree outputs, four words"""
    n_al, np_al = (n + 1) & ~1, (npairs + 1) & ~1
    return 8 * (nsums * n + nm * npairs) + 8 * 2 * 1024 + 4 * (n_al + (3 + ndeg) * np_al + 4)


def test_errors(pkg):
    eng = pkg.Engine(0)
    eng.n = 4
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*no graph"):
        eng.similarity_raw([(0, 1)])
    eng.close()
    A, pairs, r = fixture_case(golden("er_n1000"))
    n = A.shape[0]
    eng = engine_of(pkg, A)
    L, h = eng.L, eng.h
    one = np.zeros(4, dtype=np.uint32)
    vals = np.zeros(8)

    def call(count, u, v, measures, values=vals):
        p = lambda a: None if a is None else a.ctypes.data_as(u32p)   # noqa: E731
        return L.lzx_similarity(h, count, p(u), p(v), measures, p(one), None, None, None if values is None else values.ctypes.data_as(f64p), None)

    u, v = np.array([0, 1, 2, 3], dtype=np.uint32), np.array([1, 2, 3, 4], dtype=np.uint32)
    assert call(4, u, v, 1) == 0 and np.array_equal(one, similarity_restated(A, np.stack([u, v], axis=1))["common"])
    for bad_u, bad_v, word in ((np.array([0, n, 2, 3], dtype=np.uint32), v, f"has {n} vertices"), (u, np.array([1, 2, 3, 0xffffffff], dtype=np.uint32), "vertices"),
                               (u, np.array([1, 2, 2, 4], dtype=np.uint32), "itself")):
        assert call(4, bad_u, bad_v, 1) == -1
        assert word in L.lzx_last_error().decode(), L.lzx_last_error()
    assert call(4, u, v, 32) == -1 and "no measure" in L.lzx_last_error().decode()
    assert call(4, u, v, 1 << 31) == -1
    assert call(4, u, v, 1, values=None) == -1 and "values" in L.lzx_last_error().decode()
    assert call(4, u, None, 1) == -1 and call(4, None, v, 1) == -1
    assert call(4, None, None, 1) == -1 and "entries" in L.lzx_last_error().decode()      # np != nnz in edges mode
    assert call(A.nnz + 1, None, None, 0) == -1 and call(0, None, None, 0) == -1
    one[:] = 77
    assert call(0, u, v, 1) == 0 and (one == 77).all()                                     # np == 0: nothing is touched
    common, du, dv, values, info = eng.similarity_raw([])
    assert len(common) == 0 and len(du) == 0 and all(len(values[m]) == 0 for m in ALL) and info["pairs"] == 0 and info["walked"] == 0
    assert np.array_equal(eng.similarity_raw(pairs)[0], r["common"])                       # the handle still answers
    eng.close()
    # out of device memory, at either allocation
    small = engine_of(pkg, A, sim_state_bytes=4 * n)
    with pytest.raises(pkg.LzxError, match=r"\(-4\).*needs \d+ bytes"):
        small.similarity_raw(pairs)
    x = np.random.default_rng(3).standard_normal(n)
    y = small.spmv(x)
    small.close()
    first = first_state_bytes(n, len(pairs))
    second = engine_of(pkg, A, sim_state_bytes=first, sim_long_pair=1)
    with pytest.raises(pkg.LzxError, match=rf"\(-4\).*needs {first + 4 * int((r['shorter'] > 1).sum())} bytes"):
        second.similarity_raw(pairs)
    lean = second.similarity_raw(pairs, measures=(), want_degrees=False)                   # the counts alone fit under the same cap
    assert np.array_equal(lean[0], r["common"]) and lean[4]["long_pairs"] == (r["shorter"] > 1).sum() and np.array_equal(second.spmv(x), y)
    second.close()
    tight = engine_of(pkg, A, sim_state_bytes=first - 1)
    with pytest.raises(pkg.LzxError, match=rf"\(-4\).*needs {first} bytes"):
        tight.similarity_raw(pairs)
    tight.close()
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(A.indptr.astype(np.uint64), A.indices.astype(np.uint32))
    for e in grp.engines:
        with pytest.raises(pkg.LzxError, match=r"\(-3\).*communicator of 2"):
            e.similarity_raw([(0, 1)])
    grp.close()
