"""CPU: the path-based centralities (include/lzx.h: lzx_bfs_multi, lzx_betweenness_f64) without a GPU -- the binding and the
struct layout, the argument errors that come back before a device is touched, and a numpy restatement of the method
(brandes_batched: the level-synchronous pull form, 16 sources per batch, two masked SpMMs per level, the columns added into bc
left to right) against networkx on the karate club and on every golden fixture.  The GPU tests use the same restatement as
their reference.

Tolerances.  Every term of every sum is non-negative, so nothing cancels: an entry of bc is a sum of at most ns dependencies,
each the product of at most L levels of (a row sum of at most d_max terms, one multiplication, one addition, one division), so
it carries a relative error of at most (L (d_max + 4) + ns) 2^-53 in the restatement, and as much in networkx's own order: the
two differ by at most twice that, relative to the reference.  An entry that is 0 in the reference is a sum of zeros here.
Closeness and harmonic centrality are sums of at most n positive terms: n 2^-53 relative.  Distances, path counts (below 2^53)
and the integer scalars are exact."""
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
_u32p = ctypes.POINTER(ctypes.c_uint32)
_f64p = ctypes.POINTER(ctypes.c_double)
LZX_ERR_ARG = -1
EPS = 2.0 ** -53
BATCH = 16


def brandes_batched(A, sources, backward=True):
    """The library's method on a scipy CSR adjacency matrix A (symmetric, entries 1, self loops allowed).  Returns a dict:
    dist (ns, n) int32, paths (ns, n), reached / sum_dist / ecc (ns,) integers, harmonic (ns,), max_level, and bc (n,) = the sum
    over the sources, in their order, of Brandes' dependencies (raw: no 1/2, no normalisation, no endpoints)."""
    A = sp.csr_matrix(A, dtype=np.float64)
    n = A.shape[0]
    sources = np.asarray(sources, dtype=np.int64)
    ns = len(sources)
    out = dict(dist=np.empty((ns, n), dtype=np.int32), paths=np.empty((ns, n)), reached=np.ones(ns, dtype=np.uint64),
               sum_dist=np.zeros(ns, dtype=np.uint64), harmonic=np.zeros(ns), ecc=np.zeros(ns, dtype=np.uint32), bc=np.zeros(n), max_level=0)
    for first in range(0, ns, BATCH):
        src = sources[first:first + BATCH]
        b = len(src)
        cols = np.arange(b)
        dist = np.full((n, b), -1, dtype=np.int32)
        sigma = np.zeros((n, b))
        dist[src, cols] = 0
        sigma[src, cols] = 1.0
        d = 1
        while True:                                         # forward: masked A @ sigma per level
            S = A @ (sigma * (dist == d - 1))
            new = (dist == -1) & (S > 0.0)
            count = new.sum(axis=0)
            if not count.any():
                break
            dist[new] = d
            sigma[new] = S[new]
            hit = count > 0
            sl = slice(first, first + b)
            out["reached"][sl] += count.astype(np.uint64)
            out["sum_dist"][sl] += (count * d).astype(np.uint64)
            out["harmonic"][sl] += count / float(d)         # (+ 0.0 where the column did not grow)
            out["ecc"][sl][hit] = d
            d += 1
        top = d - 1
        out["max_level"] = max(out["max_level"], top)
        out["dist"][first:first + b] = dist.T
        out["paths"][first:first + b] = sigma.T
        if not backward:
            continue
        delta, g = np.zeros((n, b)), np.zeros((n, b))
        for d in range(top, 0, -1):                         # backward: masked A @ g per level
            S = A @ (g * (dist == d + 1))
            on = dist == d
            delta[on] = sigma[on] * S[on]
            g[on] = (1.0 + delta[on]) / sigma[on]
        for c in range(b):                                  # one column after the other
            out["bc"] += np.where(dist[:, c] > 0, delta[:, c], 0.0)
    return out


def load_fixture(path):
    g = np.load(path)
    rp, ci = g["ref_row_offset"].astype(np.int64), g["ref_col_idx"].astype(np.int64)
    n = len(rp) - 1
    return sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))


def fixture_sources(n):
    """the 48 sources of the fixture tests"""
    return np.random.default_rng(1).choice(n, size=48, replace=False)


def bc_bound(A, sources, max_level):
    """the relative bound of the module docstring"""
    d_max = int(np.diff(A.indptr).max()) if A.shape[0] else 0
    return 2.0 * (max_level * (d_max + 4) + len(sources)) * EPS


@functools.lru_cache(maxsize=None)
def fixture_case(path):
    """(A, sources, restatement) of one fixture, computed once and shared (read-only)"""
    A = load_fixture(path)
    src = fixture_sources(A.shape[0])
    return A, src, brandes_batched(A, src)


def assert_bc_close(bc, ref, bound):
    zero = ref == 0.0
    assert not bc[zero].any()
    assert (np.abs(bc - ref) <= bound * ref).all(), float(np.max(np.abs(bc - ref)[~zero] / ref[~zero]))


# ---- the binding --------------------------------------------------------------------------------------------------------
def test_entry_points_are_bound(pkg):
    L = pkg.lib()
    names = [name for name, _, _ in pkg.SYMBOLS]
    header = open(os.path.join(ROOT, "include", "lzx.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    for name in ("lzx_bfs_multi", "lzx_betweenness_f64"):
        assert name in names and hasattr(L, name)
        assert re.search(rf"\bint {name}\(", header)
        assert re.search(rf" T {name}\b", out)
    assert "lzx_bfs_info" in header and "bfs_state_bytes" in pkg.SHAPE_OPTIONS
    for method in ("bfs", "closeness", "harmonic", "betweenness"):
        assert hasattr(pkg.Engine, method)


def test_info_layout_matches_the_header(pkg, tmp_path):
    fields = [f for f, _ in pkg.LzxBfsInfo._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "lzx.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(lzx_bfs_info));']
    src += [f'printf("{f} %zu\\n", offsetof(lzx_bfs_info, {f}));' for f in fields]
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(pkg.LzxBfsInfo) == 4 * 4 + 2 * 8
    for f in fields:
        assert int(got[f]) == getattr(pkg.LzxBfsInfo, f).offset, f


def test_argument_errors_without_gpu(pkg):
    L = pkg.lib()
    src = np.zeros(4, dtype=np.uint32)
    bc = np.zeros(4)
    sp_, bp = src.ctypes.data_as(_u32p), bc.ctypes.data_as(_f64p)
    rest = (None,) * 7
    cases = [(lambda: L.lzx_bfs_multi(None, 4, sp_, *rest), "lzx_bfs_multi", "null handle"),
             (lambda: L.lzx_bfs_multi(None, 0, sp_, *rest), "lzx_bfs_multi", "ns == 0"),
             (lambda: L.lzx_bfs_multi(None, 4, None, *rest), "lzx_bfs_multi", "null sources"),
             (lambda: L.lzx_betweenness_f64(None, 4, sp_, bp, None), "lzx_betweenness_f64", "null handle"),
             (lambda: L.lzx_betweenness_f64(None, 4, None, bp, None), "lzx_betweenness_f64", "null handle"),
             (lambda: L.lzx_betweenness_f64(None, 0, sp_, bp, None), "lzx_betweenness_f64", "ns == 0"),
             (lambda: L.lzx_betweenness_f64(None, 4, sp_, None, None), "lzx_betweenness_f64", "null bc")]
    for call, fn, word in cases:
        assert call() == LZX_ERR_ARG, (fn, word)
        msg = L.lzx_last_error().decode()
        assert fn in msg and word in msg, (fn, word, msg)


# ---- the restatement against networkx -------------------------------------------------------------------------------------
def test_restatement_on_the_karate_club():
    G = nx.karate_club_graph()
    A = nx.to_scipy_sparse_array(G, weight=None, format="csr")
    n = A.shape[0]
    r = brandes_batched(A, np.arange(n))
    ref = nx.betweenness_centrality(G, normalized=False, weight=None)
    ref = 2.0 * np.array([ref[v] for v in range(n)])
    assert_bc_close(r["bc"], ref, bc_bound(sp.csr_matrix(A), np.arange(n), r["max_level"]))
    for s in range(n):
        lengths = nx.single_source_shortest_path_length(G, s)
        assert np.array_equal(r["dist"][s], [lengths[v] for v in range(n)])
        counts = [len(list(nx.all_shortest_paths(G, s, v))) for v in range(n)]
        assert np.array_equal(r["paths"][s], counts)
    assert (r["reached"] == n).all() and np.array_equal(r["ecc"], [nx.eccentricity(G, v) for v in range(n)])
    assert np.array_equal(r["sum_dist"], r["dist"].sum(axis=1))


@pytest.mark.parametrize("path", GOLDEN, ids=GOLDEN_IDS)
def test_restatement_on_the_fixtures(path):
    A, src, r = fixture_case(path)
    n = A.shape[0]
    G = nx.from_scipy_sparse_array(A)
    ref = nx.betweenness_centrality_subset(G, [int(s) for s in src], list(G), normalized=False)
    ref = 2.0 * np.array([ref[v] for v in range(n)])
    assert_bc_close(r["bc"], ref, bc_bound(A, src, r["max_level"]))
    harm = nx.harmonic_centrality(G, nbunch=[int(s) for s in src])
    for i, s in enumerate(int(s) for s in src):
        lengths = nx.single_source_shortest_path_length(G, s)
        d = np.full(n, -1, dtype=np.int32)
        d[list(lengths)] = list(lengths.values())
        assert np.array_equal(r["dist"][i], d), s
        assert r["reached"][i] == len(lengths) and r["sum_dist"][i] == sum(lengths.values()) and r["ecc"][i] == max(lengths.values())
        assert (r["paths"][i][d < 0] == 0).all() and (r["paths"][i][d >= 0] >= 1).all() and r["paths"][i].max() < 2.0 ** 53
        close = nx.closeness_centrality(G, s, wf_improved=True)
        r1 = float(r["reached"][i]) - 1.0
        mine = (r1 / float(r["sum_dist"][i])) * (r1 / (n - 1.0)) if r["sum_dist"][i] else 0.0
        assert abs(mine - close) <= n * EPS * close, s
        assert abs(r["harmonic"][i] - harm[s]) <= n * EPS * harm[s], s


def test_batches_and_column_order():
    """a source's BFS outputs do not depend on the batch; bc is the left-to-right sum of the single-source vectors"""
    A, src, r = fixture_case(GOLDEN[GOLDEN_IDS.index("er_n1000")])
    pick = np.concatenate([src[:20], src[3:4]])          # 21 sources: two batches, one duplicate
    whole = brandes_batched(A, pick)
    acc = np.zeros(A.shape[0])
    for i, s in enumerate(pick):
        one = brandes_batched(A, [s])
        acc = acc + one["bc"]
        j = int(np.flatnonzero(src == s)[0])
        for key in ("dist", "paths", "reached", "sum_dist", "harmonic", "ecc"):
            assert np.array_equal(one[key][0], whole[key][i]) and np.array_equal(one[key][0], r[key][j]), (key, s)
    assert np.array_equal(acc, whole["bc"])
