"""GPU: what a graph hand-over leaves behind, against a record -- every path into lzx_graph_prepare (csrc/lzx_graph.hip: CSR, the
sharded sweeps, induced(), the generator) in every mode that changes its decisions (csrc/lzx_prepare_plan.h).

The expected numbers are tests/golden/handover_shapes.json: recorded results of the build of the commit named there, the parent of
the change that split lzx_graph_prepare into a host planner and named device stages -- not results of the code under test.  Per
case and per rank: every field of info() but the three placement ones (they are timings), every read-only name of
lzx_test_get_shape but placement_*, and the SHA-256 of layout_pos from the hook under rank_row_sums() (where every vertex of the
caller's order lies: the degree ranking and the tie re-ranking to the bit); per case the SHA-256 of the bytes of spmv(x) for one
seeded x of integers in [1, 2^20] -- every partial sum is an integer below 2^53 (at most 3 000 entries per row), so the bits do not
depend on the order of the summation, and the fp32 exchange (integers below 2^24) rounds nothing.

Cases: rmat_n3000_skew, star_ring_n1500 and er_n1000, each plain; blocked with hub_entries 200 and tie_sort 0 and 2; blocked with
hub_entries 1500, long_row 4, item_len 4, narrow_slices 1; in-process groups of 2 and 3 ranks blocked with hub_entries 206, with the
overlap and the sparse exchange asked for and with sparse_exchange 0; exchange_fp32 on 2 ranks; a sharded hand-over
(sharded_ingest 1) on 2 ranks; and an induced() handle.  On these fixtures a rank's slice is shorter than one column band, so the
groups keep one chunk whatever is asked for: one more case hands a generated R-MAT graph of 200 000 vertices to 2 ranks, where the
two-chunk exchange and its sparse second chunk are taken (exchange_chunk0 < exchange_slice and exchange_recv in its record)."""
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from test_paths_host import GOLDEN, GOLDEN_IDS, load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "golden", "handover_shapes.json")
FIXTURES = ("rmat_n3000_skew", "star_ring_n1500", "er_n1000")
GENERATED = "rmat_generated_n200000"
GENERATED_SPEC = (18, 200000, 2000000, 11)      # gen_rmat(scale, n, draws, seed)
PLACEMENT = ("placement_tried", "placement_kept", "placement_us")
SHAPES = ("gather_items_dealt", "gather_items_drawn", "gather_workgroups", "start_vector_was_constant", "finish_deferrable",
          "finish_launched", "row_bands", "pb_runs", "pb_steps", "scatter_units", "split_rows", "split_items", "body_slices",
          "slices_wide", "slices_w8", "slices_w4", "slices_w0", "staged_workgroups", "split_entries", "body_entries",
          "staged_x_stride", "live_rows", "multi_chunk", "multi_work_items", "multi_split_rows", "multi_chunk_slots",
          "multi_row_segments", "multi_vector_grid", "graph_lanes_rows", "graph_lanes_oriented")
BLOCKED_206 = dict(propagation_blocking=1, hub_entries=206)
# name -> (ranks, how the graph arrives, options)
CASES = {
    "plain": (1, "csr", dict(propagation_blocking=0)),
    "blocked_200_tie_sort_0": (1, "csr", dict(propagation_blocking=1, hub_entries=200, tie_sort=0)),
    "blocked_200_tie_sort_2": (1, "csr", dict(propagation_blocking=1, hub_entries=200, tie_sort=2)),
    "blocked_1500_narrow": (1, "csr", dict(propagation_blocking=1, hub_entries=1500, long_row=4, item_len=4, narrow_slices=1)),
    "ranks_2_sparse": (2, "csr", dict(BLOCKED_206, overlap_exchange=1, sparse_exchange=1)),
    "ranks_3_sparse": (3, "csr", dict(BLOCKED_206, overlap_exchange=1, sparse_exchange=1)),
    "ranks_2_dense": (2, "csr", dict(BLOCKED_206, overlap_exchange=1, sparse_exchange=0)),
    "ranks_3_dense": (3, "csr", dict(BLOCKED_206, overlap_exchange=1, sparse_exchange=0)),
    "ranks_2_exchange_fp32": (2, "csr", dict(propagation_blocking=0, exchange_fp32=1)),
    "ranks_2_sharded": (2, "csr", dict(BLOCKED_206, sharded_ingest=1)),
    "induced": (1, "induced", dict(propagation_blocking=1, hub_entries=200)),
}
GENERATED_CASES = {"ranks_2_sparse": (2, "rmat", dict(BLOCKED_206, overlap_exchange=1, sparse_exchange=1))}
ALL = [(g, c) for g in FIXTURES for c in CASES] + [(GENERATED, c) for c in GENERATED_CASES]


@functools.lru_cache(maxsize=None)
def fixture(name):
    A = load_fixture(GOLDEN[GOLDEN_IDS.index(name)])
    A.sort_indices()
    return A.indptr.astype(np.uint64), A.indices.astype(np.uint32)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def layout_pos(eng):
    """layout_pos of lzx_test_rank_row_sums (csrc/lzx_test_hooks.h), which Engine.rank_row_sums() turns into ids"""
    gi = eng.info()
    v = np.empty(max(gi["rows_local"], 1))
    pos = np.empty(gi["n"], dtype=np.uint32)
    pad = ctypes.c_uint64()
    rc = eng.L.lzx_test_rank_row_sums(eng.h, v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                      pos.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(pad))
    assert rc == 0, rc
    return pos


def observe(pkg, graph, case):
    """one hand-over on fresh handles: what the record holds for it"""
    world, how, options = (GENERATED_CASES if graph == GENERATED else CASES)[case]
    parent = None
    if how == "induced":
        rp, ci = fixture(graph)
        parent = pkg.Engine(0)
        parent.set_graph_csr(rp, ci)
        keep = np.random.default_rng(5).random(len(rp) - 1) < 0.8
        g = parent.induced(keep, **options)[0]
    else:
        g = pkg.Engine(0, **options) if world == 1 else pkg.LocalGroup([0] * world, **options)
        if how == "rmat":
            g.gen_rmat(*GENERATED_SPEC)
        else:
            g.set_graph_csr(*fixture(graph))
    try:
        engines = g.engines if world > 1 else [g]
        ranks = []
        for e in engines:
            info = {k: int(v) for k, v in e.info().items() if k not in PLACEMENT}
            ranks.append(dict(info=info, shape={k: e.shape(k) for k in SHAPES}))
        x = np.random.default_rng(7).integers(1, 1 << 20, size=g.n, endpoint=True).astype(np.float64)
        out = dict(spmv_sha256=sha(g.spmv(x)), ranks=ranks)
        for e, r in zip(engines, ranks):
            r["layout_pos_sha256"] = sha(layout_pos(e))
        return out
    finally:
        g.close()
        if parent is not None:
            parent.close()


@functools.lru_cache(maxsize=None)
def recorded():
    with open(RECORD) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("graph,case", ALL)
def test_the_hand_over_is_the_recorded_one(pkg, graph, case):
    expected = recorded()["cases"][graph][case]
    got = observe(pkg, graph, case)
    assert len(got["ranks"]) == len(expected["ranks"])
    for r, (a, b) in enumerate(zip(got["ranks"], expected["ranks"])):
        for part in ("info", "shape"):
            differ = {k: (a[part].get(k), v) for k, v in b[part].items() if a[part].get(k) != v}
            print(graph, case, "rank", r, part, "differs from the record in", differ or "nothing")
            assert not differ and sorted(a[part]) == sorted(b[part])
        assert a["layout_pos_sha256"] == b["layout_pos_sha256"], (graph, case, r)
    assert got["spmv_sha256"] == expected["spmv_sha256"]


def test_the_record_holds_every_case():
    """no GPU: the record names its commit and has every case, every rank, every name -- no field was left out when it was made"""
    rec = recorded()
    assert len(rec["commit"]) >= 7 and not rec.get("left_out")
    assert sorted((g, c) for g in rec["cases"] for c in rec["cases"][g]) == sorted(ALL)
    info_keys = None
    for graph, case in ALL:
        world = (GENERATED_CASES if graph == GENERATED else CASES)[case][0]
        entry = rec["cases"][graph][case]
        assert len(entry["ranks"]) == world and len(entry["spmv_sha256"]) == 64
        for r in entry["ranks"]:
            assert sorted(r["shape"]) == sorted(SHAPES) and len(r["layout_pos_sha256"]) == 64
            assert not set(r["info"]) & set(PLACEMENT)
            info_keys = info_keys or sorted(r["info"])
            assert sorted(r["info"]) == info_keys
    # the generated case is there for the two-chunk exchange with its sparse second chunk
    for r in rec["cases"][GENERATED]["ranks_2_sparse"]["ranks"]:
        assert 0 < r["info"]["exchange_chunk0"] < r["info"]["exchange_slice"] and r["info"]["exchange_recv"] > 0
