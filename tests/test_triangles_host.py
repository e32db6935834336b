"""CPU: triangle counts and clustering (include/lzx.h: lzx_triangles) without a GPU -- the binding and the struct layout, the
argument error that comes back before a device is touched, and a numpy restatement of the method itself (triangles_oriented:
degrees without the diagonal, the ranking by (d_v, v), the oriented lists, the intersections that walk the shorter list and
binary-search the longer, and the three adds) against networkx on the karate club, on every golden fixture and on a fixture
with self loops.  The GPU tests use the same restatement and networkx as their references.

Everything here is an integer or one correctly rounded division of two integers below 2^53, so every comparison is equality:
the counts, the clustering coefficients bit for bit, and the transitivity (networkx divides sum 2 t_v by sum d_v (d_v - 1),
the operands used here)."""
import ctypes
import functools
import glob
import os
import re
import subprocess

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
GOLDEN_IDS = [os.path.basename(p)[:-4] for p in GOLDEN]
LZX_ERR_ARG = -1


def triangles_oriented(A):
    """The library's method on a scipy CSR adjacency matrix A (symmetric, entries 1, self loops allowed).  Returns a dict: tri
    (n,) uint64, deg (n,) the degrees without the diagonal, clustering (n,), triangles, wedges, max_triangles,
    oriented_entries, oriented_max_degree (Python integers), transitivity, and the oriented copy itself: out_rows, out_cols
    (its entries a -> b, row by row) and out_degree (n,)."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    rp, ci = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    off = rows != ci
    deg = np.bincount(rows[off], minlength=n).astype(np.int64)              # degrees without the diagonal
    # every edge that is not a loop, once: in the row of its lower rank (d_v, v); a filter of an ascending row stays ascending
    up = off & ((deg[ci] > deg[rows]) | ((deg[ci] == deg[rows]) & (ci > rows)))
    orow, ocol = rows[up], ci[up]
    m = len(orow)
    k = np.bincount(orow, minlength=n).astype(np.int64)                     # out-degrees
    orp = np.concatenate([[0], np.cumsum(k)])
    key = orow * n + ocol                                                   # ascending: the oriented lists one after the other
    # out-edge e = (a -> b): the shorter of N+(a), N+(b) is walked (a's on a tie), the longer binary-searched
    ka, kb = k[orow], k[ocol]
    walk_a = ka <= kb
    walked, searched = np.where(walk_a, orow, ocol), np.where(walk_a, ocol, orow)
    ks = k[walked]
    edge = np.repeat(np.arange(m, dtype=np.int64), ks)
    pos = np.arange(int(ks.sum()), dtype=np.int64) - np.repeat(np.cumsum(ks) - ks, ks)
    x = ocol[orp[walked[edge]] + pos]
    want = searched[edge] * n + x
    at = np.searchsorted(key, want)
    hit = (at < m) & (key[np.minimum(at, max(m - 1, 0))] == want) if m else np.zeros(0, dtype=bool)
    t = np.zeros(n, dtype=np.int64)
    np.add.at(t, x[hit], 1)                                                 # a hit adds 1 to t_c
    hits = np.bincount(edge[hit], minlength=m).astype(np.int64)
    np.add.at(t, ocol, hits)                                                # per out-edge: the hits to t_b
    np.add.at(t, np.arange(n), np.bincount(orow, weights=hits, minlength=n).astype(np.int64))   # per row: the total to t_a
    pairs2 = deg * (deg - 1)
    clustering = np.zeros(n)
    nz = (deg >= 2) & (t > 0)
    clustering[nz] = (2 * t[nz]) / pairs2[nz]
    total, contri = int(t.sum()), int(pairs2.sum())
    return dict(tri=t.astype(np.uint64), deg=deg, clustering=clustering, triangles=total // 3, wedges=contri // 2,
                max_triangles=int(t.max()) if n else 0, oriented_entries=m, oriented_max_degree=int(k.max()) if n else 0,
                transitivity=0.0 if total == 0 else (2 * total) / contri, out_rows=orow, out_cols=ocol, out_degree=k)


def load_fixture(path):
    g = np.load(path)
    rp, ci = g["ref_row_offset"].astype(np.int64), g["ref_col_idx"].astype(np.int64)
    n = len(rp) - 1
    return sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))


def networkx_reference(A):
    """(triangles (n,) uint64, clustering (n,), transitivity) of networkx on the graph of A"""
    G = nx.from_scipy_sparse_array(sp.csr_matrix(A))
    n = A.shape[0]
    t, c = nx.triangles(G), nx.clustering(G)
    return np.array([t[v] for v in range(n)], dtype=np.uint64), np.array([c[v] for v in range(n)]), nx.transitivity(G)


@functools.lru_cache(maxsize=None)
def fixture_case(path):
    """(A, restatement, networkx's (triangles, clustering, transitivity)) of one fixture, computed once and shared (read-only)"""
    A = load_fixture(path)
    return A, triangles_oriented(A), networkx_reference(A)


def assert_equals_networkx(r, ref):
    t, c, trans = ref
    assert np.array_equal(r["tri"], t)
    assert np.array_equal(r["clustering"], c)
    assert r["transitivity"] == trans
    assert r["triangles"] * 3 == int(t.sum()) and r["max_triangles"] == int(t.max())


# ---- the binding --------------------------------------------------------------------------------------------------------
def test_entry_point_is_bound(pkg):
    L = pkg.lib()
    names = [name for name, _, _ in pkg.SYMBOLS]
    header = open(os.path.join(ROOT, "include", "lzx.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert "lzx_triangles" in names and hasattr(L, "lzx_triangles")
    assert re.search(r"\bint lzx_triangles\(", header) and "lzx_triangles_info" in header
    assert re.search(r" T lzx_triangles\b", out)
    assert "tri_long_list" in pkg.SHAPE_OPTIONS and "tri_state_bytes" in pkg.SHAPE_OPTIONS
    for method in ("triangles", "clustering", "transitivity", "average_clustering", "triangles_raw"):
        assert hasattr(pkg.Engine, method)


def test_info_layout_matches_the_header(pkg, tmp_path):
    fields = [f for f, _ in pkg.LzxTrianglesInfo._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "lzx.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(lzx_triangles_info));']
    src += [f'printf("{f} %zu\\n", offsetof(lzx_triangles_info, {f}));' for f in fields]
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(pkg.LzxTrianglesInfo) == 4 * 8 + 2 * 4 + 4 * 8
    for f in fields:
        assert int(got[f]) == getattr(pkg.LzxTrianglesInfo, f).offset, f


def test_argument_error_without_gpu(pkg):
    L = pkg.lib()
    info = pkg.LzxTrianglesInfo()
    for args in ((None, None, None, None), (None, None, None, ctypes.byref(info))):
        assert L.lzx_triangles(*args) == LZX_ERR_ARG
        msg = L.lzx_last_error().decode()
        assert "lzx_triangles" in msg and "null handle" in msg, msg


# ---- the restatement against networkx -------------------------------------------------------------------------------------
def test_restatement_on_the_karate_club():
    G = nx.karate_club_graph()
    A = sp.csr_matrix(nx.to_scipy_sparse_array(G, weight=None, format="csr"))
    r = triangles_oriented(A)
    assert_equals_networkx(r, networkx_reference(A))
    assert r["triangles"] == 45 and r["oriented_entries"] == G.number_of_edges()
    assert r["wedges"] == sum(d * (d - 1) // 2 for _, d in G.degree())


@pytest.mark.parametrize("path", GOLDEN, ids=GOLDEN_IDS)
def test_restatement_on_the_fixtures(path):
    A, r, ref = fixture_case(path)
    assert_equals_networkx(r, ref)
    assert r["oriented_entries"] * 2 == A.nnz - int(A.diagonal().sum())
    assert nx.average_clustering(nx.from_scipy_sparse_array(A)) == sum(ref[1].tolist()) / A.shape[0]


@pytest.mark.parametrize("path", GOLDEN, ids=GOLDEN_IDS)
def test_out_degree_bound(path):
    """a vertex of out-degree k has k neighbours of degree >= k: k^2 <= nnz"""
    A, r, _ = fixture_case(path)
    assert r["oriented_max_degree"] ** 2 <= A.nnz
    assert r["oriented_max_degree"] <= int(r["deg"].max())


def test_self_loops_change_nothing():
    A, r, ref = fixture_case(GOLDEN[GOLDEN_IDS.index("er_n1000")])
    n = A.shape[0]
    loops = np.zeros(n)
    loops[::7] = 1.0
    B = sp.csr_matrix(A + sp.diags(loops))
    assert B.nnz == A.nnz + len(loops[::7]) and not A.diagonal().any()
    rb = triangles_oriented(B)
    assert_equals_networkx(rb, networkx_reference(B))          # networkx takes v out of its own neighbourhood
    for key in ("tri", "deg", "clustering"):
        assert np.array_equal(rb[key], r[key]), key
    for key in ("triangles", "wedges", "max_triangles", "oriented_entries", "oriented_max_degree", "transitivity"):
        assert rb[key] == r[key], key


def test_a_relabelling_permutes_the_counts():
    A, r, _ = fixture_case(GOLDEN[GOLDEN_IDS.index("rmat_n3000_skew")])
    n = A.shape[0]
    new_of_old = np.random.default_rng(5).permutation(n)
    P = sp.csr_matrix((np.ones(n), (new_of_old, np.arange(n))), shape=(n, n))
    rp = triangles_oriented(sp.csr_matrix(P @ A @ P.T))
    assert np.array_equal(rp["tri"][new_of_old], r["tri"]) and np.array_equal(rp["clustering"][new_of_old], r["clustering"])
    for key in ("triangles", "wedges", "max_triangles", "oriented_entries", "transitivity"):
        assert rp[key] == r[key], key
