"""CPU: edge support and truss numbers (include/lzx.h: lzx_truss) without a GPU -- the binding and the struct layout, the argument
error that comes back before a device is touched, and a numpy/scipy restatement of the definition (truss_rounds: each round
the support of the remaining edges as (B @ B).multiply(B), k = max(k, the smallest support + 2), every remaining edge of
support <= k - 2 removed at once) against networkx.k_truss on the karate club and on every golden fixture, on a fixture with
self loops, on a relabelled fixture and on two small graphs with known answers.  The GPU tests use the same restatement as their
reference.

Everything here is an integer, so every comparison is equality."""
import ctypes
import functools
import itertools
import os
import re
import subprocess

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp

from test_core_host import GOLDEN, GOLDEN_IDS, load_fixture, without_loops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LZX_ERR_ARG = -1
INTS = ("edges", "triangles", "main_truss_edges", "max_support", "max_truss", "levels", "rounds")
VECTORS = ("support", "truss", "layer", "vertex_truss")

# what the definition gives on the fixtures: T, max support, max truss, rounds, levels, main truss edges
EXPECTED = {"er_n1000": (160, 3, 3, 3, 2, 466), "er_n4000_deg20": (1323, 3, 3, 3, 2, 3782), "er_c1_n10000": (1277, 3, 3, 3, 2, 3753),
            "rmat_n3000_skew": (402850, 480, 59, 222, 48, 2747), "rmat_n4096": (117588, 293, 25, 146, 24, 1880),
            "star_ring_n1500": (1499, 2, 3, 2, 1, 2998)}
EXPECTED_KEYS = ("triangles", "max_support", "max_truss", "rounds", "levels", "main_truss_edges")


def truss_rounds(A):
    """The definition on a scipy CSR adjacency matrix A (symmetric, self loops allowed).  Returns a dict: support, truss, layer
    (nnz,) uint32, one value per stored entry of A with sorted indices (0 on the diagonal), vertex_truss (n,) uint32, entry_rows
    (nnz,) the row of every entry, and the Python integers of INTS."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    rp, ci = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    nnz = len(ci)
    support, truss, layer = (np.zeros(nnz, dtype=np.uint32) for _ in range(3))
    alive = rows != ci
    m = int(alive.sum()) // 2
    k, r, first = 2, 0, True
    while alive.any():
        r += 1
        idx = np.flatnonzero(alive)
        B = sp.csr_matrix((np.ones(len(idx), dtype=np.int64), (rows[idx], ci[idx])), shape=(n, n))
        S = sp.csr_matrix((B @ B).multiply(B) + B)      # the pattern of B (the supports + 1): the entries of idx, in their order
        S.sort_indices()
        assert S.nnz == len(idx)
        sup = S.data - 1
        if first:
            support[idx] = sup
            first = False
        k = max(k, int(sup.min()) + 2)
        gone = idx[sup <= k - 2]
        truss[gone], layer[gone] = k, r
        alive[gone] = False
    vertex = np.zeros(n, dtype=np.uint32)
    np.maximum.at(vertex, rows, truss)
    off = rows != ci
    return dict(support=support, truss=truss, layer=layer, vertex_truss=vertex, entry_rows=rows, edges=m,
                triangles=int(support.astype(np.int64).sum()) // 6, main_truss_edges=int((truss[off] == k).sum()) // 2 if m else 0,
                max_support=int(support.max()) if nnz else 0, max_truss=k if m else 0, levels=len(np.unique(truss[off])), rounds=r)


def edge_set(A, values, k):
    """the edges (u < v) of A whose per-entry value is >= k"""
    A = sp.csr_matrix(A)
    A.sort_indices()
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    keep = (values >= k) & (rows < A.indices)
    return set(zip(rows[keep].tolist(), A.indices[keep].tolist()))


def assert_equals_networkx(A, r):
    """{e : truss(e) >= k} is networkx.k_truss(G, k)'s edge set for k = 3, 4, max and max + 1, vertices included"""
    G = nx.from_scipy_sparse_array(without_loops(A))
    top = r["max_truss"]
    for k in sorted({3, 4, top, top + 1}):
        H = nx.k_truss(G, k)
        want = {(min(u, v), max(u, v)) for u, v in H.edges()}
        got = edge_set(A, r["truss"], k)
        assert got == want, k
        assert set(H.nodes()) == {v for e in got for v in e}, k
    assert not edge_set(A, r["truss"], top + 1) and edge_set(A, r["truss"], top)


@functools.lru_cache(maxsize=None)
def fixture_case(path):
    """(A, restatement) of one fixture, computed once and shared (read-only)"""
    A = load_fixture(path)
    A.sort_indices()
    return A, truss_rounds(A)


def adjacency(n, edges):
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    M = sp.csr_matrix(sp.coo_matrix((np.ones(2 * len(e)), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))), shape=(n, n)))
    M.data[:] = 1.0
    M.sort_indices()
    return M


def clique_edges(members):
    return list(itertools.combinations(members, 2))


def k5_ears():
    """K_5 and two vertices each joined to both ends of the K_5 edge (0, 1): that edge has support 5 and loses two triangles in
    round 1, one per triangle and not one per dying edge"""
    return adjacency(7, clique_edges(range(5)) + [(0, 5), (1, 5), (0, 6), (1, 6)])


def two_hubs():
    """Vertices 0 and 1 are adjacent, each has 300 leaves of its own, X = {602, 603} is adjacent to both, and 0, X and eight more
    vertices form a K_11, as do 1, X and another eight (the edge inside X taken once)"""
    edges = [(0, 1)] + [(0, v) for v in range(2, 302)] + [(1, v) for v in range(302, 602)]
    a, b = [0, 602, 603] + list(range(604, 612)), [1, 602, 603] + list(range(612, 620))
    edges += clique_edges(a) + [e for e in clique_edges(b) if e != (602, 603)]
    return adjacency(620, edges)


def value_of(A, values, u, v):
    A = sp.csr_matrix(A)
    at = A.indptr[u] + np.searchsorted(A.indices[A.indptr[u]:A.indptr[u + 1]], v)
    assert A.indices[at] == v
    return int(values[at])


# ---- the binding --------------------------------------------------------------------------------------------------------
def test_entry_point_is_bound(pkg):
    L = pkg.lib()
    names = [name for name, _, _ in pkg.SYMBOLS]
    header = open(os.path.join(ROOT, "include", "lzx.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert "lzx_truss" in names and hasattr(L, "lzx_truss")
    assert re.search(r"\bint lzx_truss\(", header) and "lzx_truss_info" in header
    assert re.search(r" T lzx_truss\b", out)
    assert "truss_long_row" in pkg.SHAPE_OPTIONS and "truss_state_bytes" in pkg.SHAPE_OPTIONS
    hooks = open(os.path.join(ROOT, "msc-hpc-final-project_amd", "csrc", "lzx_test_hooks.h")).read()
    assert '"truss_long_row"' in hooks and '"truss_state_bytes"' in hooks
    assert "These thirteen" in header
    for method in ("truss_raw", "edge_support", "truss_number", "max_truss", "k_truss"):
        assert hasattr(pkg.Engine, method)


def test_info_layout_matches_the_header(pkg, tmp_path):
    fields = [f for f, _ in pkg.LzxTrussInfo._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "lzx.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(lzx_truss_info));']
    src += [f'printf("{f} %zu\\n", offsetof(lzx_truss_info, {f}));' for f in fields]
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(pkg.LzxTrussInfo) == 64
    for f in fields:
        assert int(got[f]) == getattr(pkg.LzxTrussInfo, f).offset, f
    assert set(pkg.LzxTrussInfo().as_dict()) == set(fields) == set(INTS) | {"loop_ms", "support_ms", "peel_ms"}


def test_argument_error_without_gpu(pkg):
    L = pkg.lib()
    info = pkg.LzxTrussInfo()
    for args in ((None,) * 6, (None,) * 5 + (ctypes.byref(info),)):
        assert L.lzx_truss(*args) == LZX_ERR_ARG
        msg = L.lzx_last_error().decode()
        assert "lzx_truss" in msg and "null handle" in msg, msg


# ---- the restatement against networkx -------------------------------------------------------------------------------------
def test_restatement_on_the_karate_club():
    G = nx.karate_club_graph()
    A = sp.csr_matrix(nx.to_scipy_sparse_array(G, weight=None, format="csr"))
    r = truss_rounds(A)
    assert_equals_networkx(A, r)
    assert r["edges"] == 78 and r["triangles"] == 45 and r["max_truss"] == 5
    assert r["triangles"] == sum(nx.triangles(G).values()) // 3


@pytest.mark.parametrize("path", GOLDEN, ids=GOLDEN_IDS)
def test_restatement_on_the_fixtures(path):
    A, r = fixture_case(path)
    assert not A.diagonal().any() and r["edges"] == A.nnz // 2
    assert_equals_networkx(A, r)
    print({key: r[key] for key in INTS})
    assert tuple(r[key] for key in EXPECTED_KEYS) == EXPECTED[os.path.basename(path)[:-4]]
    assert int(r["truss"].min()) >= 2 and int(r["layer"].min()) >= 1 and int(r["layer"].max()) == r["rounds"]
    T = sp.csr_matrix((r["truss"], A.indices, A.indptr), shape=A.shape)
    assert (T != T.T).nnz == 0                                     # both copies of an edge carry the same number


def test_every_fixture_has_its_expected_values():
    assert sorted(EXPECTED) == sorted(GOLDEN_IDS)


def test_self_loops_change_nothing():
    A, r = fixture_case(GOLDEN[GOLDEN_IDS.index("er_n1000")])
    n = A.shape[0]
    loops = np.zeros(n)
    loops[::7] = 1.0
    B = sp.csr_matrix(A + sp.diags(loops))
    B.sort_indices()
    assert B.nnz == A.nnz + len(loops[::7])
    rb = truss_rounds(B)
    off = rb["entry_rows"] != B.indices
    for key in ("support", "truss", "layer"):
        assert np.array_equal(rb[key][off], r[key]) and not rb[key][~off].any(), key
    assert np.array_equal(rb["vertex_truss"], r["vertex_truss"])
    for key in INTS:
        assert rb[key] == r[key], key


def test_a_relabelling_permutes_the_values():
    A, r = fixture_case(GOLDEN[GOLDEN_IDS.index("rmat_n4096")])
    n = A.shape[0]
    new_of_old = np.random.default_rng(5).permutation(n)
    P = sp.csr_matrix((np.ones(n), (new_of_old, np.arange(n))), shape=(n, n))
    B = sp.csr_matrix(P @ A @ P.T)
    B.sort_indices()
    rb = truss_rounds(B)
    for key in ("support", "truss", "layer"):
        M = sp.csr_matrix((rb[key] + 1.0, B.indices, B.indptr), shape=(n, n))     # + 1: a support of 0 stays a stored entry
        back = sp.csr_matrix(P.T @ M @ P)
        back.sort_indices()
        assert np.array_equal(back.indices, A.indices) and np.array_equal(back.data - 1.0, r[key]), key
    assert np.array_equal(rb["vertex_truss"][new_of_old], r["vertex_truss"])
    for key in INTS:
        assert rb[key] == r[key], key


# ---- two known answers ----------------------------------------------------------------------------------------------------
def test_k5_ears():
    A = k5_ears()
    r = truss_rounds(A)
    assert_equals_networkx(A, r)
    assert (A.shape[0], r["edges"], r["triangles"], r["rounds"], r["levels"]) == (7, 14, 12, 2, 2)
    per_edge = r["truss"][r["entry_rows"] < A.indices]
    assert int((per_edge == 5).sum()) == 10 and int((per_edge == 3).sum()) == 4 and r["main_truss_edges"] == 10
    assert value_of(A, r["support"], 0, 1) == 5 == r["max_support"] and value_of(A, r["truss"], 0, 1) == 5
    assert value_of(A, r["layer"], 0, 1) == 2 and value_of(A, r["layer"], 0, 5) == 1


def test_two_hubs():
    A = two_hubs()
    r = truss_rounds(A)
    assert_equals_networkx(A, r)
    assert (A.shape[0], r["edges"], r["triangles"], r["rounds"]) == (620, 710, 332, 4)
    per_edge = r["truss"][r["entry_rows"] < A.indices]
    assert sorted(zip(*np.unique(per_edge, return_counts=True))) == [(2, 600), (4, 1), (11, 109)]
    assert (value_of(A, r["support"], 0, 1), value_of(A, r["truss"], 0, 1), value_of(A, r["layer"], 0, 1)) == (2, 4, 2)
    assert int((r["layer"] == 2).sum()) == 2                       # alone in its window (both copies), which is not the last
    lengths = np.diff(A.indptr)
    assert lengths[0] == lengths[1] == 311 and A.nnz // A.shape[0] == 2
