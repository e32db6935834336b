"""GPU: the state bytes of the capped graph routines that no other test holds to the byte -- lzx_core_numbers, lzx_triangles (both
allocations), lzx_bfs_multi / lzx_betweenness_f64 with 1, 3 and 16 sources (B = 2, 4, 16 interleaved columns) and lzx_brandes_f64
in the combinations of bc, ebc and endpoints its API allows -- on er_n1000 and on star_ring_n1500.  At the default
multi_row_chunk of 2048 the batched tables split no row of either fixture (the hub of star_ring_n1500 has 1 499 entries), so the
paths' cases run a third time on star_ring_n1500 with multi_row_chunk = 8, where the tables have split rows and n_parts > 0.

The expected numbers are tests/golden/state_bytes.json: recorded results of the build of the commit named there, the parent of the
change that put the arenas on csrc/lzx_carve.h, not results of the code under test.  They were read from its errors: with the cap
at 0 the call fails with "needs N bytes"; with the cap at that N, lzx_triangles fails at its second allocation with the second N.
Per case: a cap of N - 1 fails with (-4) and that very N in the message, a cap of N succeeds with the fixture's results, and spmv
gives the same bits before and after.

Checked by hand against the formulas of that commit (even(n) = n rounded up to an even count, r16 = rounded up to 16):
  core        16 even(n) + 8:                                er_n1000 16 008, star_ring_n1500 24 008
  triangles   8 (n + 1) + 16 n + 32 np + 40 + 4 even(n) with np = min(1024, ceil(n / 256)), then + 4 max(m, 1) with m the edges
              without the self loops: the fixtures' first numbers follow from n alone, the second from m
  paths       r16(4 n B) + 8 n B (1 + third + fourth) + 8 n [bc] + 8 nnz [ebc] + 8 n [endpoints] + 8 n_parts B + r16(4 n_parts) + 64
              with third = any n-vector or bc or ebc is asked for, fourth = bc and ebc, and n_parts from the fixture's rows: a
              row of more than multi_row_chunk entries is ceil(len / chunk) parts, so 0 at the default chunk and
              ceil(1499 / 8) = 188 with the chunk of 8, where the hub's row alone is split.
(test_the_recorded_numbers_follow_the_formulas keeps that check, and needs no GPU.)"""
import functools
import json
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import test_core_host
import test_triangles_host
from test_edge_betweenness_host import assert_close, brandes_edges, ebc_bound
from test_paths_host import GOLDEN, GOLDEN_IDS, assert_bc_close, bc_bound, brandes_batched, fixture_sources, load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (the fixture, the shapes set beside the cap)
GRAPHS = {"er_n1000": ("er_n1000", {}), "star_ring_n1500": ("star_ring_n1500", {}), "star_ring_n1500_chunk8": ("star_ring_n1500", {"multi_row_chunk": 8})}
with open(os.path.join(ROOT, "tests", "golden", "state_bytes.json")) as _f:
    RECORDED = json.load(_f)


def golden(name):
    return GOLDEN[GOLDEN_IDS.index(name)]


@functools.lru_cache(maxsize=None)
def graph(name):
    A = load_fixture(golden(GRAPHS[name][0]))
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def paths_reference(name, ns):
    """the first ns of the fixture tests' sources and their restatement: lzx_brandes_f64's (ebc, the endpoints' count) with
    lzx_betweenness_f64's bc, which the device gives bit for bit with or without ebc (tests/test_gpu_edge_betweenness.py): once
    per case"""
    A = graph(name)
    src = fixture_sources(A.shape[0])[:ns]
    ref = brandes_edges(A, src)
    ref["bc"] = brandes_batched(A, src)["bc"]
    return src, ref


# ---- the cases: name -> (the cap's option, the call, the check of what it returns) ----------------------------------------------
def core_case(name):
    r = test_core_host.fixture_case(golden(GRAPHS[name][0]))[1]

    def check(out):
        assert np.array_equal(out[0], r["core"]) and np.array_equal(out[1], r["layer"])
    return "core_state_bytes", lambda eng: eng.core_number_raw(), check


def triangles_case(name):
    r = test_triangles_host.fixture_case(golden(GRAPHS[name][0]))[1]

    def check(out):
        assert np.array_equal(out[0], r["tri"])
    return "tri_state_bytes", lambda eng: eng.triangles_raw(), check


def bfs_case(name, ns):
    src, ref = paths_reference(name, ns)

    def check(out):
        assert np.array_equal(out[0], ref["dist"])
        for key in ("reached", "sum_dist", "ecc"):
            assert np.array_equal(out[1][key], ref[key]), key
    return "bfs_state_bytes", lambda eng: eng.bfs(src), check


def betweenness_case(name, ns):
    src, ref = paths_reference(name, ns)

    def check(out):
        assert_bc_close(out[0], ref["bc"], bc_bound(graph(name), src, ref["max_level"]))
    return "bfs_state_bytes", lambda eng: eng.betweenness_raw(src), check


def brandes_case(name, want_bc, want_edges, endpoints):
    src, ref = paths_reference(name, 16)

    def check(out):
        bc, ebc, _ = out
        bound = ebc_bound(graph(name), src, ref["max_level"])
        assert (bc is None) == (not want_bc) and (ebc is None) == (not want_edges)
        if want_edges:
            assert_close(ebc, ref["ebc"], bound)
        if want_bc:   # (the endpoints' count is an integer added last: one more rounding, which ebc_bound's 2 eps cover)
            assert_close(bc, ref["bc"] + (ref["cnt"].astype(np.float64) if endpoints else 0.0), bound)
    return "bfs_state_bytes", lambda eng: eng.brandes_raw(src, want_bc=want_bc, want_edges=want_edges, endpoints=endpoints), check


CASES = {"core": core_case, "triangles": triangles_case}
for _ns in (1, 3, 16):
    CASES[f"bfs_ns{_ns}"] = functools.partial(bfs_case, ns=_ns)
    CASES[f"betweenness_ns{_ns}"] = functools.partial(betweenness_case, ns=_ns)
# what lzx_brandes_f64 accepts: bc or ebc, and the endpoints only with bc
for _key, _kw in (("bc", (True, False, False)), ("ebc", (False, True, False)), ("bc_ebc", (True, True, False)),
                  ("bc_endpoints", (True, False, True)), ("bc_ebc_endpoints", (True, True, True))):
    CASES[f"brandes_{_key}"] = functools.partial(brandes_case, want_bc=_kw[0], want_edges=_kw[1], endpoints=_kw[2])


def capped(pkg, name, option, cap, call):
    """One call on a fresh handle with the option at `cap` (a shape is set before the graph is handed over).  Returns (N, None)
    where it fails -- with (-4) and "needs N bytes", anything else is an error of the test -- or (None, what the call returned);
    spmv gives the same bits before and after either way."""
    A = graph(name)
    eng = pkg.Engine(0, **{option: cap}, **GRAPHS[name][1])
    try:
        eng.set_graph_csr(A.indptr.astype(np.uint64), A.indices.astype(np.uint32))
        x = np.random.default_rng(3).standard_normal(A.shape[0])
        y = eng.spmv(x)
        try:
            out, n = call(eng), None
        except pkg.LzxError as e:
            m = re.search(r"\(-4\).*needs (\d+) bytes", str(e))
            assert m, str(e)
            out, n = None, int(m.group(1))
        assert np.array_equal(eng.spmv(x), y)
        return n, out
    finally:
        eng.close()


def cases_of(name):
    """every case, but on the graph with the chunk of 8 only those whose arena depends on it"""
    return [case for case in CASES if not GRAPHS[name][1] or case not in ("core", "triangles")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", [(name, case) for name in GRAPHS for case in cases_of(name)])
def test_the_state_bytes_are_the_recorded_ones(pkg, name, case):
    expected = RECORDED["bytes"][name][case]
    assert len(expected) == (2 if case == "triangles" else 1)
    option, call, check = CASES[case](name)
    for i, n in enumerate(expected):
        short = capped(pkg, name, option, n - 1, call)[0]
        print(name, case, "allocation", i, "recorded", n, "one byte short, this build asks for", short)
        assert short == n                                                      # that very N
        got, out = capped(pkg, name, option, n, call)
        if i + 1 < len(expected):
            assert got == expected[i + 1]                                      # the next allocation's N
        else:
            assert got is None
            check(out)


def test_the_recorded_numbers_follow_the_formulas():
    """the docstring's hand check, kept (no GPU): the recorded numbers against the formulas of the commit they were recorded from,
    with n_parts from the fixture's rows -- a row of more than multi_row_chunk entries is ceil(len / chunk) parts (lzx_multi.hip)"""
    even = lambda v: (v + 1) // 2 * 2    # noqa: E731
    r16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    for name in GRAPHS:
        A = graph(name)
        n, nnz = A.shape[0], A.nnz
        m = (nnz - int(sp.csr_matrix(A).diagonal().astype(bool).sum())) // 2
        got = RECORDED["bytes"][name]
        chunk = GRAPHS[name][1].get("multi_row_chunk", 2048)
        rows = np.diff(A.indptr)
        parts = int(sum(-(-int(length) // chunk) for length in rows[rows > chunk]))
        assert parts == RECORDED["n_parts"][name] and (parts > 0) == bool(GRAPHS[name][1]) and sorted(got) == sorted(cases_of(name))
        if name == "star_ring_n1500_chunk8":   # the hub's row alone is split
            assert (rows > chunk).sum() == 1 and rows.max() == 1499 and parts == 188
        if "core" in got:
            assert got["core"] == [16 * even(n) + 8]
            first = 8 * (n + 1) + 16 * n + 32 * min(1024, -(-n // 256)) + 40 + 4 * even(n)
            assert got["triangles"] == [first, first + 4 * max(m, 1)]

        def paths(B, third, fourth, bc, ebc, cnt):
            return r16(4 * n * B) + 8 * n * B * (1 + third + fourth) + 8 * n * bc + 8 * nnz * ebc + 8 * n * cnt + 8 * parts * B + r16(4 * parts) + 64
        for ns, B in ((1, 2), (3, 4), (16, 16)):
            assert got[f"bfs_ns{ns}"] == [paths(B, 1, 0, 0, 0, 0)]
            assert got[f"betweenness_ns{ns}"] == [paths(B, 1, 0, 1, 0, 0)]
        assert got["brandes_bc"] == [paths(16, 1, 0, 1, 0, 0)] and got["brandes_ebc"] == [paths(16, 1, 0, 0, 1, 0)]
        assert got["brandes_bc_ebc"] == [paths(16, 1, 1, 1, 1, 0)] and got["brandes_bc_endpoints"] == [paths(16, 1, 0, 1, 0, 1)]
        assert got["brandes_bc_ebc_endpoints"] == [paths(16, 1, 1, 1, 1, 1)]
