"""GPU: the graph routines on the caller-order CSR -- lzx_components, lzx_triangles, lzx_core_numbers, lzx_truss, lzx_color,
lzx_label_propagation (and lzx_modularity behind it), lzx_sweep_cut, lzx_similarity -- at every width of their kernel templates over G
lanes per row, on the graphs of tests/lanes_graphs.py: rows of G - 1, G, G + 1, 2 G +- 1 and 64 G, 64 G + 1 entries for every G, n on
both sides of a multiple of 256 / G rows per workgroup, the long row first and last, oriented lists of every length.

The test shape graph_lanes (csrc/lzx_test_hooks.h) forces G = 4, 8, 16, 32, 64 (capped at the widest kernel of each launch);
graph_lanes_rows / graph_lanes_oriented read back what ran.  One cell = one routine on one graph at the six settings (unforced and
the five widths): at each the read-backs are the expected widths, every output and count equals the numpy restatement of the
routine's own host file (through the comparison of the routine's own GPU file), and the outputs equal the unforced run's bit for
bit -- but the two similarity sums, held to sum_bound, and avg_clustering, held to n 2^-53 (both inside those comparisons).  The
defaults that derive from G (the long-row thresholds 64 G) are left alone, so the hubs of 64 G and 64 G + 1 entries fall on the two
sides of the split at every G.  test_coverage_table asserts what the cells reached."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import lanes_graphs as lg
import test_gpu_communities as gcomm
import test_gpu_core as gcore
import test_gpu_similarity as gsim
import test_gpu_sweep as gsweep
import test_gpu_triangles as gtri
import test_gpu_truss as gtruss
from test_communities_host import chain
from test_components_host import components_restatement, counts_of, scipy_labels
from test_core_host import peel_rounds
from test_gpu_components import COUNTS
from test_similarity_host import similarity_restated
from test_sweep_host import ASCENDING, PER_DEGREE, sweep_ref
from test_triangles_host import triangles_oriented
from test_truss_host import truss_rounds

pytestmark = pytest.mark.gpu

LZX_ERR_ARG = -1
SETTINGS = (None, 4, 8, 16, 32, 64)          # graph_lanes: unset, then every width
ROUTINES = ("components", "triangles", "core", "truss", "communities", "sweep", "similarity")
# the widest kernel of the launches behind graph_lanes_rows / graph_lanes_oriented (None: the routine has no oriented copy)
MAX_G = {"components": (32, None), "triangles": (64, 32), "core": (32, None), "truss": (64, 32), "communities": (32, None), "sweep": (32, None),
         "similarity": (32, None)}
LADDER_NAMES = tuple(lg.ladder_name(*c) for c in lg.LADDERS)
GRAPHS = LADDER_NAMES + ("complete_200", "complete_70")


@functools.lru_cache(maxsize=None)
def graph(name):
    if name in LADDER_NAMES:
        return lg.ladder(*lg.LADDERS[LADDER_NAMES.index(name)])
    if name == "two_cliques_70_200":
        return lg.two_cliques()
    if name == "twin_hubs":
        return lg.twin_hubs()
    if name == "split_gadgets":
        return lg.split_gadgets()
    if name.startswith("complete_"):
        return lg.complete(int(name[9:]))
    if name.startswith("circulant_"):
        d, iso = (int(x) for x in name[10:].split("+"))
        return lg.circulant(200, d // 2, iso)
    raise KeyError(name)


_ENGINES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()


def engine(pkg, name, lanes, **options):
    """the handle of a graph at a setting, made once and kept for the module"""
    key = (name, lanes, tuple(sorted(options.items())))
    if key not in _ENGINES:
        if lanes is not None:
            options = dict(options, graph_lanes=lanes)
        _ENGINES[key] = gcore.engine_of(pkg, graph(name), **options)
        assert _ENGINES[key].shape("graph_lanes_rows") == 0 and _ENGINES[key].shape("graph_lanes_oriented") == 0     # no graph call yet
    return _ENGINES[key]


def expected_lanes(A, lanes, max_g, oriented=False):
    """what lzx_lanes_per_row gives: the forced width or the rule on the mean row length (of the oriented copy: half the entries off
    the diagonal over the same rows), capped at the widest kernel"""
    if max_g is None:
        return 0
    if lanes is not None:
        return min(lanes, max_g)
    A = sp.csr_matrix(A)
    lengths = np.diff(A.indptr)
    entries = (A.nnz - int(A.diagonal().sum())) // 2 if oriented else A.nnz
    if oriented and entries == 0:
        return 0
    mean = entries // max(int((lengths > 0).sum()), 1)
    G = 4
    while G < max_g and 2 * G <= mean:
        G *= 2
    return G


def read_back(eng, routine, A, lanes):
    got = (eng.shape("graph_lanes_rows"), eng.shape("graph_lanes_oriented"))
    want = (expected_lanes(A, lanes, MAX_G[routine][0]), expected_lanes(A, lanes, MAX_G[routine][1], True))
    assert got == want, (routine, lanes, got, want)
    return got


# ---- the restatements, once per graph (read-only) ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_components(name):
    A = graph(name)
    rp, ci = A.indptr.astype(np.uint64), A.indices.astype(np.uint32)
    labels, rounds = components_restatement(rp, ci)
    want = scipy_labels(rp, ci)
    assert np.array_equal(labels, want)
    return want, counts_of(want) + (rounds,)


@functools.lru_cache(maxsize=None)
def ref_triangles(name):
    return triangles_oriented(graph(name))


@functools.lru_cache(maxsize=None)
def ref_core(name):
    return peel_rounds(graph(name))


@functools.lru_cache(maxsize=None)
def ref_truss(name):
    return truss_rounds(graph(name))


@functools.lru_cache(maxsize=None)
def ref_chain(name, ties_by_id):
    return chain(graph(name), 0, ties_by_id)


@functools.lru_cache(maxsize=None)
def sweep_case(name):
    """two score columns from a seeded draw and their restatements under the two flags"""
    A = graph(name)
    S = np.random.default_rng(31).standard_normal((2, A.shape[0]))
    return S, {flags: [sweep_ref(A, S[c], flags) for c in range(2)] for flags in (ASCENDING, PER_DEGREE)}


@functools.lru_cache(maxsize=None)
def similarity_case(name):
    A = graph(name)
    if name in LADDER_NAMES:
        pairs = lg.ladder_pairs(*lg.LADDERS[LADDER_NAMES.index(name)])
    elif name == "twin_hubs":     # the three pairs of hubs, hubs with leaves, leaves with leaves
        pairs = np.array([(0, 1), (0, 2), (2, 1), (1, 0), (0, 3), (1, 2051), (2, 2051), (2, 2050), (3, 4), (3, 2051), (2050, 2051)], dtype=np.int64)
    else:
        pairs = gsim.all_pairs(range(0, A.shape[0], max(A.shape[0] // 30, 1)))
    return pairs, similarity_restated(A, pairs)


# ---- one routine on one handle: the comparison of the routine's own GPU file; returns the bits that must not depend on the width ----
def run_components(eng, name, lanes):
    want, counts = ref_components(name)
    labels, info = eng.components()
    assert labels.dtype == np.uint32 and np.array_equal(labels, want)
    got = tuple(info[k] for k in COUNTS)
    print(f"  components {name} lanes {lanes}: rounds {info['rounds']} (restatement {counts[3]})")
    assert got == counts, (got, counts)
    return labels.tobytes(), got


def run_triangles(eng, name, lanes):
    r = ref_triangles(name)
    tri, clus, info = gtri.check(eng, graph(name), r["tri"], r["clustering"])
    assert {k: info[k] for k in gtri.INTS} == {k: r[k] for k in gtri.INTS}
    return tri.tobytes(), clus.tobytes(), tuple(info[k] for k in gtri.INTS)


def run_core(eng, name, lanes):
    core, layer, info = gcore.check(eng, ref_core(name))
    return core.tobytes(), layer.tobytes(), tuple(sorted(info.items()))


def run_truss(eng, name, lanes):
    vec, info = gtruss.check(eng, graph(name), ref_truss(name))
    return tuple(vec[k].tobytes() for k in gtruss.VECTORS), tuple(sorted(info.items()))


def run_communities(eng, name, lanes):
    out = []
    for ties_by_id in (True, False):
        color, cints, labels, lints, q = gcomm.check(eng, ref_chain(name, ties_by_id), ties_by_id)
        out.append((color.tobytes(), tuple(sorted(cints.items())), labels.tobytes(), tuple(sorted(lints.items())), q))
    return tuple(out)


def run_sweep(eng, name, lanes):
    S, refs = sweep_case(name)
    out = []
    for flags, kw in ((ASCENDING, dict(ascending=True)), (PER_DEGREE, dict(per_degree=True))):
        got = gsweep.run(eng, S, **kw)
        for c in range(2):
            gsweep.assert_column(got, c, refs[flags][c])
        out.append((got[0].tobytes(), got[1].tobytes(), got[2].tobytes(), repr(got[3]), got[4]["entries"]))
    return tuple(out)


def run_similarity(eng, name, lanes):
    pairs, r = similarity_case(name)
    common, du, dv, values, info = gsim.check(eng, pairs, r, f"  similarity {name} lanes {lanes}")      # (the sums: sum_bound, inside)
    assert info["lanes"] == expected_lanes(graph(name), lanes, 32)
    return common.tobytes(), du.tobytes(), dv.tobytes(), tuple(values[m].tobytes() for m in gsim.RATIOS), info["walked"], info["max_common"]


RUN = dict(components=run_components, triangles=run_triangles, core=run_core, truss=run_truss, communities=run_communities, sweep=run_sweep,
           similarity=run_similarity)
# the shapes a routine's handles carry in every cell: the propagation's group kernel takes rows of up to 129 entries, one past the 128
# labels it stages in LDS (lpa_table_row is left alone: rows of 2047 and 2048 entries in the LDS table, 2049 in a global one)
SHAPES = {"communities": dict(lpa_group_row=129)}
_CELLS = {}


def cell(pkg, routine, name, **options):
    """the routine on the graph at the six settings; returns {setting: (rows, oriented)} of the read-backs.  Run once per module."""
    key = (routine, name, tuple(sorted(options.items())))
    if key in _CELLS:
        return _CELLS[key]
    A = graph(name)
    widths, first = {}, None
    for lanes in SETTINGS:
        eng = engine(pkg, name, lanes, **dict(SHAPES.get(routine, {}), **options))
        bits = RUN[routine](eng, name, lanes)
        widths[lanes] = read_back(eng, routine, A, lanes)
        if lanes is None:
            first = bits
        assert bits == first, (routine, name, lanes, "differs from the unforced run")
    _CELLS[key] = widths
    return widths


# ---- 1. every routine on every graph at every width ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("routine", ROUTINES)
def test_every_width(pkg, routine, name):
    widths = cell(pkg, routine, name)
    print(routine, name, widths)
    cap_rows, cap_oriented = MAX_G[routine]
    assert {w[0] for lanes, w in widths.items() if lanes} == {G for G in (4, 8, 16, 32, 64) if G <= cap_rows}
    if cap_oriented:
        assert {w[1] for lanes, w in widths.items() if lanes} == {4, 8, 16, 32}


# ---- 2. the oriented lists: the split at tri_long_list and the LDS staging, 1, 2 and 3 slices of the wide kernel -----------------
@pytest.mark.parametrize("name", ["complete_200", "complete_129", "complete_70"])
@pytest.mark.parametrize("routine", ["triangles", "truss"])
def test_oriented_lists_at_the_split_and_the_stage(pkg, routine, name):
    """tri_long_list = 4: lists of 4 entries by the group kernel, of 5 and more by the wide kernel (lzx_truss's support kernel
    splits there too), which stages lists of at most 128 entries: K_200 has lists of 127, 128 and 129.  The wide kernel's slices,
    max(kmax / 64, 1), are 3, 2 and 1.  Unset (128) the wide kernel runs on K_200 alone: test_every_width."""
    r = ref_triangles(name)
    lists = set(r["out_degree"].tolist())
    m = graph(name).shape[0]
    assert {4, 5} <= lists and r["oriented_max_degree"] == m - 1 and max((m - 1) // 64, 1) == {200: 3, 129: 2, 70: 1}[m]
    cell(pkg, routine, name, tri_long_list=4)


# ---- 3. long rows that are peeled while their neighbours depend on it -----------------------------------------------------------
def peeled_lengths(routine, name):
    """the stored lengths of the rows (lzx_core_numbers) or of the shorter rows of the edges (lzx_truss) of every window but the
    last, which is not peeled: what the split between the group kernel and the long-row launch is taken on"""
    A = graph(name)
    lengths = np.diff(A.indptr)
    if routine == "core":
        r = ref_core(name)
        return lengths[r["layer"] < r["rounds"]]
    r = ref_truss(name)
    peeled = (r["entry_rows"] != A.indices) & (r["layer"] < r["rounds"])
    return np.minimum(lengths[r["entry_rows"]], lengths[A.indices])[peeled]


@pytest.mark.parametrize("routine", ["core", "truss"])
def test_peeled_long_rows_at_the_split(pkg, routine):
    """The ladder's hubs are peeled after their leaves: nothing depends on what a kernel does with their rows.  In split_gadgets
    (tests/lanes_graphs.py) a row of 64 G and one of 64 G + 1 entries, for every G, is peeled while neighbours remain whose layer
    depends on its decrements: at G forced lanes the first is the group kernel's and the second the long-row launch's."""
    name = "split_gadgets"
    A = graph(name)
    lengths = np.diff(A.indptr)
    assert lg.rule(A) == 4
    got = set(peeled_lengths(routine, name).tolist())
    assert set(lg.SPLIT_LENGTHS) <= got
    for T, (u, v, w) in lg.split_gadget_ids().items():
        assert lengths[u] == lengths[v] == T
        if routine == "core":
            r = ref_core(name)
            assert r["layer"][[u, v, w]].tolist() == [3, 4, 4] and r["rounds"] == 5
        else:
            r = ref_truss(name)
            assert [gtruss.value_of(A, r["layer"], a, b) for a, b in ((u, v), (u, w), (v, w))] == [2, 3, 4] and r["rounds"] == 5
    cell(pkg, routine, name)


# ---- 3b. both peel launches of lzx_truss ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_row", [68, 69])
def test_truss_edges_at_the_split(pkg, long_row):
    """K_70 beside K_200: K_70 is one window that is peeled, the shorter row of each of its edges has 69 entries -- exactly the
    threshold at truss_long_row = 69 (the group kernel), one more than it at 68 (the long-row launch): whole windows of edges for
    either launch.  (Nothing outside a clique's window depends on its peel; test_peeled_long_rows_at_the_split has edges on which
    something does.)"""
    name = "two_cliques_70_200"
    A, r = graph(name), ref_truss(name)
    lengths = np.diff(A.indptr)
    peeled = (r["entry_rows"] != A.indices) & (r["layer"] < r["rounds"])
    shorter = np.minimum(lengths[r["entry_rows"]], lengths[A.indices])[peeled]
    assert len(shorter) == 70 * 69 and (shorter == 69).all() and int(lengths.max()) == 199 > long_row
    cell(pkg, "truss", name, truss_long_row=long_row)


def test_similarity_pairs_at_the_split_of_32_lanes(pkg):
    """The ladder has one row of 2049 entries, so no pair of its vertices has a shorter row of 64 * 32 + 1: two hubs of the same 2049
    leaves have, and with the third hub, of 2048, a shorter row of exactly 64 * 32.  At 32 lanes (and at 64, capped to 32) the first
    pair is a workgroup's and the second a group's; the paths are counted inside the comparison."""
    pairs, r = similarity_case("twin_hubs")
    assert r["shorter"][:3].tolist() == [2049, 2048, 2048] and r["common"][:3].tolist() == [2049, 2048, 2048]
    assert lg.rule(graph("twin_hubs")) == 4
    cell(pkg, "similarity", "twin_hubs")


# ---- 4. the propagation's group kernel around its staged labels ------------------------------------------------------------------
@pytest.mark.parametrize("name", LADDER_NAMES)
def test_propagation_group_rows_of_129_and_130(pkg, name):
    """lpa_group_row = 129 (every cell of test_every_width) and 130: the hub of 129 entries is updated by a group of lanes that reads
    one label past the 128 it stages, the hub of 128 fills the stage, 127 leaves a place; the same labels either way."""
    lengths = set(np.diff(graph(name).indptr).tolist())
    assert {127, 128, 129, 2047, 2048, 2049} <= lengths
    cell(pkg, "communities", name)
    cell(pkg, "communities", name, lpa_group_row=130)


# ---- 5. the rule itself ----------------------------------------------------------------------------------------------------------
CIRCULANT_ORIENTED = (4, 4, 4, 8, 8, 16, 16, 32)          # the rule on the oriented copy: k entries per list
CIRCULANTS = [f"circulant_{d}+0" for d in lg.CIRCULANT_DEGREES] + ["circulant_16+50"]


_RULE = {}


def rule_cell(pkg, name):
    """every routine on a circulant, nothing forced; returns {routine: (rows, oriented)} read back.  Run once per module."""
    if name not in _RULE:
        A = graph(name)
        eng = engine(pkg, name, None, **SHAPES["communities"])
        got = {}
        for routine in ROUTINES:
            RUN[routine](eng, name, None)
            got[routine] = read_back(eng, routine, A, None)
        _RULE[name] = got
    return _RULE[name]


def rule_holds(name, got):
    d = int(np.diff(graph(name).indptr).max())
    at = lg.CIRCULANT_DEGREES.index(d)
    return all(rows == (64 if (d == 64 and MAX_G[routine][0] == 64) else lg.CIRCULANT_LANES[at]) and
               oriented == (CIRCULANT_ORIENTED[at] if MAX_G[routine][1] else 0) for routine, (rows, oriented) in got.items())


@pytest.mark.parametrize("name", CIRCULANTS)
def test_the_rule_at_its_steps(pkg, name):
    """C_200(1 .. k) has 2 k entries in every row: nothing is forced, and the widths read back are the rule's, 4, 8, 8, 16, 16, 32, 32,
    32 for 2 k = 6, 8, 14, 16, 30, 32, 62, 64 (and 64 for the orientation pass at 64); 50 isolated vertices do not enter the mean."""
    got = rule_cell(pkg, name)
    print(name, got)
    assert rule_holds(name, got), got


# ---- 6. the shape itself ---------------------------------------------------------------------------------------------------------
def test_graph_lanes_is_range_checked(pkg):
    eng = pkg.Engine(0)
    for value in (-1, 0, 4, 8, 16, 32, 64):
        assert eng.L.lzx_test_set_shape(eng.h, b"graph_lanes", value) == 0, value
    for value in (-2, 1, 2, 3, 5, 12, 33, 63, 65, 128, 1 << 40):
        assert eng.L.lzx_test_set_shape(eng.h, b"graph_lanes", value) == LZX_ERR_ARG, value
        assert b"graph_lanes must be" in eng.L.lzx_last_error()
    assert eng.L.lzx_set_option(eng.h, b"graph_lanes", 8) == LZX_ERR_ARG           # a test shape, not an option
    for name in ("graph_lanes_rows", "graph_lanes_oriented"):
        assert eng.shape(name) == 0
    eng.close()
    # a call without lanes (the batched search) leaves 0 behind a call with lanes
    eng = engine(pkg, "complete_70", 16)
    eng.triangles_raw()
    assert (eng.shape("graph_lanes_rows"), eng.shape("graph_lanes_oriented")) == (16, 16)
    eng.bfs([0])
    assert (eng.shape("graph_lanes_rows"), eng.shape("graph_lanes_oriented")) == (0, 0)


# ---- 7. what the cells reached ---------------------------------------------------------------------------------------------------
def split_lines(routine, G):
    """a row of exactly the threshold in force stays in the group kernel and one of threshold + 1 goes to the long-row launch, at the
    lanes G of the split's call site: from the row lengths (of the rows that are peeled, of the pairs' shorter rows)"""
    thr = 64 * G
    if routine in ("core", "truss"):
        lengths = peeled_lengths(routine, "split_gadgets")
        return bool((lengths == thr).any() and (lengths == thr + 1).any())
    for name in LADDER_NAMES:
        A = graph(name)
        lengths = np.diff(A.indptr)
        if routine == "similarity":      # (the ladder's pairs, and the two hubs of 2049 entries of twin_hubs: 64 * 32 + 1)
            lengths = np.concatenate([similarity_case(name)[1]["shorter"], similarity_case("twin_hubs")[1]["shorter"]])
        if not ((lengths == thr).any() and (lengths == thr + 1).any()):
            return False
    return True


def test_coverage_table(pkg):
    """Every line must hold, per routine; the cells are run here unless their tests already ran in this process."""
    lines = {}
    ladders = {name: lg.coverage(graph(name)) for name in LADDER_NAMES}
    for routine in ROUTINES:
        cells = {name: cell(pkg, routine, name) for name in GRAPHS}
        cap_rows, cap_oriented = MAX_G[routine]
        for G in (4, 8, 16, 32, 64):
            if G <= cap_rows:
                lines[f"{routine}: {G} lanes per row ran and were read back on every graph"] = all(w[G][0] == G for w in cells.values())
            if cap_oriented and G <= cap_oriented:
                lines[f"{routine}: {G} lanes per oriented list ran and were read back on every graph"] = all(w[G][1] == G for w in cells.values())
        lines[f"{routine}: the unforced width is the rule's"] = all(w[None][0] == lg.rule(graph(name), cap_rows) for name, w in cells.items())
        for G in lg.WIDTHS:
            lines[f"{routine}: rows of 0, 1, G - 1, G, G + 1, 2 G - 1, 2 G + 1 entries at G = {G}"] = all(c[G]["row_lengths"] for c in ladders.values())
            fills = {c[G]["fill"] for c in ladders.values()}
            lines[f"{routine}: last workgroup full, with one row, one row short at G = {G}"] = {0, 1, 256 // G - 1} <= fills
            if routine != "triangles":
                lines[f"{routine}: rows of 64 G and 64 G + 1 entries on the two sides of the split at G = {G}"] = split_lines(routine, G)
        lines[f"{routine}: the long row first in the first workgroup"] = any(c["first_is_longest"] for c in ladders.values())
        lines[f"{routine}: the long row last in a last workgroup that is not full"] = any(
            c["last_is_longest"] and all(c["n"] % (256 // G) for G in lg.WIDTHS + (64,)) and c["n"] % 256 for c in ladders.values())
    # core: two slices of the long row (max_degree / 1024), and the row is one of a window that is peeled
    r = ref_core(LADDER_NAMES[0])
    hubs, _ = lg.ladder_ids(*lg.LADDERS[0])
    lines["core: a peeled row in two slices"] = 2049 // 1024 == 2 and bool(r["layer"][hubs[0]] < r["rounds"])
    # triangles and truss: the oriented lists
    for routine in ("triangles", "truss"):
        slices = set()
        for name in ("complete_200", "complete_129", "complete_70"):
            cell(pkg, routine, name, tri_long_list=4)
            slices.add(max(ref_triangles(name)["oriented_max_degree"] // 64, 1))
        lists = set(ref_triangles("complete_200")["out_degree"].tolist())
        lines[f"{routine}: 1, 2 and 3 slices of the wide kernel"] = slices == {1, 2, 3}
        lines[f"{routine}: lists of 4 and 5 entries at tri_long_list = 4"] = {4, 5} <= lists
        lines[f"{routine}: lists of stage - 1, stage, stage + 1 entries (stage 128), staged and not"] = {127, 128, 129} <= lists
        lines[f"{routine}: the wide kernel at the default tri_long_list"] = ref_triangles("complete_200")["oriented_max_degree"] > 128
    for routine in ("core", "truss"):
        cell(pkg, routine, "split_gadgets")
    for long_row in (68, 69):
        cell(pkg, "truss", "two_cliques_70_200", truss_long_row=long_row)
    lines["truss: a window of edges of exactly truss_long_row entries for the group kernel, of truss_long_row + 1 for the long-row launch"] = bool(
        (peeled_lengths("truss", "two_cliques_70_200") == 69).all())
    for name in LADDER_NAMES:
        cell(pkg, "communities", name, lpa_group_row=130)
    cell(pkg, "similarity", "twin_hubs")
    lines["communities: rows of 127, 128, 129 entries around the staged labels, 2047, 2048, 2049 around the LDS table"] = all(
        {127, 128, 129, 2047, 2048, 2049} <= c["lengths"] for c in ladders.values())
    for name in CIRCULANTS:
        lines[f"the rule: {name}"] = rule_holds(name, rule_cell(pkg, name))
    for name, v in lines.items():
        print(f"  {'ok ' if v else 'MISSING'} {name}")
    missing = [name for name, v in lines.items() if not v]
    assert not missing, missing
    print("widths read back:", {routine: sorted({w for name in GRAPHS for w in _CELLS[routine, name, ()].values()}) for routine in ROUTINES})
