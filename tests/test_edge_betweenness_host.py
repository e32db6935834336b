"""CPU: edge betweenness and endpoints (include/lzx.h: lzx_brandes_f64) without a GPU -- the binding and the struct layout, the
argument errors that come back before a device is touched, and a numpy restatement of the method (brandes_edges: the forward
search of tests/test_paths_host.py's brandes_batched, a backward recurrence that keeps sigma and forms g, then one pass over the
stored entries per column, ascending) against networkx on the karate club and on every golden fixture.  The GPU tests use the
same restatement as their reference.

Tolerance.  An entry of ebc is a sum of at most ns non-negative terms, each one product of an exact sigma (below 2^53) and a g
that carries the relative error bc carries (test_paths_host: bc_bound), so restatement and networkx differ by at most
bc_bound(A, sources, L) + 2 * 2^-53, relative, entry by entry; an entry that is 0 in the reference is a sum of zeros here.  The
endpoints' count is an integer, added once.  The two identities hold in exact arithmetic
    (a) the sum of ebc over all stored entries = 2 * the sum over the sources of sum_dist (a pair (s, t) spreads one unit over
        every level of its paths, and both copies of an edge are stored),
    (b) the sum of row v = 2 bc[v] + cnt[v] (what enters v from above is 1 + delta, what leaves it below is delta; at the source
        itself delta_s(s) = reached - 1),
and are asserted within the same bound, summed with math.fsum."""
import ctypes
import math
import os
import re
import subprocess

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp

from test_paths_host import BATCH, EPS, GOLDEN, GOLDEN_IDS, bc_bound, brandes_batched, fixture_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_u32p = ctypes.POINTER(ctypes.c_uint32)
_f64p = ctypes.POINTER(ctypes.c_double)
LZX_ERR_ARG = -1


def brandes_edges(A, sources):
    """lzx_brandes_f64's method on a scipy CSR adjacency matrix A (symmetric, entries 1, sorted indices, self loops allowed).
    Returns brandes_batched's dict (bc is formed here, from the recurrence that keeps sigma) plus ebc (nnz,), one value per
    stored entry in CSR order, and cnt (n,) int64, the endpoints' count."""
    A = sp.csr_matrix(A, dtype=np.float64)
    assert A.has_sorted_indices
    n = A.shape[0]
    sources = np.asarray(sources, dtype=np.int64)
    rows, ci = np.repeat(np.arange(n), np.diff(A.indptr)), A.indices
    out = brandes_batched(A, sources, backward=False)
    out.update(bc=np.zeros(n), ebc=np.zeros(A.nnz), cnt=np.zeros(n, dtype=np.int64))
    for first in range(0, len(sources), BATCH):
        src = sources[first:first + BATCH]
        b = len(src)
        dist = np.ascontiguousarray(out["dist"][first:first + b].T)
        sigma = np.ascontiguousarray(out["paths"][first:first + b].T)
        delta, g = np.zeros((n, b)), np.zeros((n, b))
        for d in range(int(dist.max()), 0, -1):             # backward: masked A @ g per level; sigma stays
            S = A @ (g * (dist == d + 1))
            on = dist == d
            delta[on] = sigma[on] * S[on]
            g[on] = (1.0 + delta[on]) / sigma[on]
        for c in range(b):                                  # one column after the other
            out["bc"] += np.where(dist[:, c] > 0, delta[:, c], 0.0)
            du, dw = dist[rows, c], dist[ci, c]
            down, up = (du >= 0) & (dw == du + 1), (dw >= 0) & (du == dw + 1)
            out["ebc"] += np.where(down, sigma[rows, c] * g[ci, c], np.where(up, sigma[ci, c] * g[rows, c], 0.0))
            out["cnt"] += dist[:, c] > 0
            out["cnt"][src[c]] += int(out["reached"][first + c]) - 1
    return out


def ebc_bound(A, sources, max_level):
    """the relative bound of the module docstring"""
    return bc_bound(A, sources, max_level) + 2.0 * EPS


def assert_close(got, ref, bound):
    """within bound of ref, relative, entry by entry; exactly 0 where ref is 0"""
    zero = ref == 0.0
    assert not got[zero].any()
    assert (np.abs(got - ref) <= bound * ref).all(), float(np.max(np.abs(got - ref)[~zero] / ref[~zero]))


def edges_of_networkx(A, ref):
    """networkx's dict over the edges (either orientation) -> one value per stored entry of A, doubled: the raw sum"""
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return 2.0 * np.array([ref[(u, w)] if (u, w) in ref else ref[(w, u)] for u, w in zip(rows.tolist(), A.indices.tolist())])


def assert_identities(A, r, bound):
    """(a) and (b) of the module docstring on a result dict with ebc, bc, cnt and sum_dist"""
    total = 2.0 * float(int(r["sum_dist"].astype(object).sum()))
    assert abs(math.fsum(r["ebc"]) - total) <= bound * total
    for v in range(A.shape[0]):
        want = math.fsum([2.0 * r["bc"][v], float(r["cnt"][v])])
        assert abs(math.fsum(r["ebc"][A.indptr[v]:A.indptr[v + 1]]) - want) <= bound * want, v


# ---- the binding --------------------------------------------------------------------------------------------------------
def test_entry_point_is_bound(pkg):
    L = pkg.lib()
    names = [name for name, _, _ in pkg.SYMBOLS]
    header = open(os.path.join(ROOT, "include", "lzx.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert "lzx_brandes_f64" in names and hasattr(L, "lzx_brandes_f64")
    assert re.search(r"\bint lzx_brandes_f64\(", header) and re.search(r" T lzx_brandes_f64\b", out)
    assert re.search(r"#define LZX_BRANDES_ENDPOINTS 1\b", header) and pkg.LZX_BRANDES_ENDPOINTS == 1
    assert "lzx_brandes_info" in header
    for method in ("brandes_raw", "edge_betweenness", "betweenness"):
        assert hasattr(pkg.Engine, method)
    import inspect
    assert list(inspect.signature(pkg.Engine.betweenness).parameters)[-1] == "endpoints"
    assert inspect.signature(pkg.Engine.betweenness).parameters["endpoints"].default is False


def test_info_layout_matches_the_header(pkg, tmp_path):
    fields = [f for f, _ in pkg.LzxBrandesInfo._fields_]
    assert fields == ["ns", "batches", "max_level", "sweeps", "loop_ms", "sweep_ms", "edge_ms"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "lzx.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(lzx_brandes_info));']
    src += [f'printf("{f} %zu\\n", offsetof(lzx_brandes_info, {f}));' for f in fields]
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(pkg.LzxBrandesInfo) == 4 * 4 + 3 * 8
    for f in fields:
        assert int(got[f]) == getattr(pkg.LzxBrandesInfo, f).offset, f


def test_argument_errors_without_gpu(pkg):
    L = pkg.lib()
    src = np.zeros(4, dtype=np.uint32)
    bc, ebc = np.zeros(4), np.zeros(4)
    sp_, bp, ep = src.ctypes.data_as(_u32p), bc.ctypes.data_as(_f64p), ebc.ctypes.data_as(_f64p)
    cases = [(lambda: L.lzx_brandes_f64(None, 4, sp_, 0, bp, ep, None), "null handle"),
             (lambda: L.lzx_brandes_f64(None, 4, None, 1, bp, None, None), "null handle"),
             (lambda: L.lzx_brandes_f64(None, 0, sp_, 0, bp, ep, None), "ns == 0"),
             (lambda: L.lzx_brandes_f64(None, 4, sp_, 0, None, None, None), "null bc and null ebc"),
             (lambda: L.lzx_brandes_f64(None, 4, sp_, 2, bp, ep, None), "unknown flag"),
             (lambda: L.lzx_brandes_f64(None, 4, sp_, 0x80000001, bp, ep, None), "unknown flag"),
             (lambda: L.lzx_brandes_f64(None, 4, sp_, 1, None, ep, None), "LZX_BRANDES_ENDPOINTS with null bc")]
    for call, word in cases:
        assert call() == LZX_ERR_ARG, word
        msg = L.lzx_last_error().decode()
        assert "lzx_brandes_f64" in msg and word in msg, (word, msg)


# ---- the restatement against networkx -------------------------------------------------------------------------------------
def test_restatement_on_the_karate_club():
    G = nx.karate_club_graph()
    A = sp.csr_matrix(nx.to_scipy_sparse_array(G, weight=None, format="csr"))
    A.sort_indices()
    n = A.shape[0]
    r = brandes_edges(A, np.arange(n))
    bound = ebc_bound(A, np.arange(n), r["max_level"])
    assert np.array_equal(r["bc"], brandes_batched(A, np.arange(n))["bc"])
    ref = edges_of_networkx(A, nx.edge_betweenness_centrality(G, normalized=False, weight=None))
    print("ebc: largest relative difference", float(np.max(np.abs(r["ebc"] - ref) / ref)), "bound", bound)
    assert_close(r["ebc"], ref, bound)
    ends = nx.betweenness_centrality(G, normalized=False, weight=None, endpoints=True)
    assert (r["cnt"] == 2 * (n - 1)).all()                  # connected: n - 1 as a target, n - 1 as a source
    assert_close(r["bc"] + r["cnt"].astype(np.float64), 2.0 * np.array([ends[v] for v in range(n)]), bound)
    assert_identities(A, r, bound)


@pytest.mark.parametrize("path", GOLDEN, ids=GOLDEN_IDS)
def test_restatement_on_the_fixtures(path):
    A, src, plain = fixture_case(path)
    r = brandes_edges(A, src)
    bound = ebc_bound(A, src, r["max_level"])
    assert np.array_equal(r["bc"], plain["bc"])
    G = nx.from_scipy_sparse_array(A)
    ref = edges_of_networkx(A, nx.edge_betweenness_centrality_subset(G, [int(s) for s in src], list(G), normalized=False))
    nz = ref > 0
    print("ebc: largest relative difference", float(np.max(np.abs(r["ebc"] - ref)[nz] / ref[nz])) if nz.any() else 0.0, "bound", bound)
    assert_close(r["ebc"], ref, bound)
    M = sp.csr_matrix((r["ebc"], A.indices, A.indptr), shape=A.shape)
    assert (M != M.T).nnz == 0 and not M.diagonal().any()
    assert_identities(A, r, bound)


def test_batches_and_column_order():
    """ebc is the left-to-right sum of the single-source vectors wherever the batch boundary falls; so are bc and cnt"""
    A, src, _ = fixture_case(GOLDEN[GOLDEN_IDS.index("er_n1000")])
    pick = np.concatenate([src[:20], src[3:4]])          # 21 sources: two batches, one duplicate
    whole = brandes_edges(A, pick)
    acc, bc, cnt = np.zeros(A.nnz), np.zeros(A.shape[0]), np.zeros(A.shape[0], dtype=np.int64)
    for s in pick:
        one = brandes_edges(A, [s])
        acc, bc, cnt = acc + one["ebc"], bc + one["bc"], cnt + one["cnt"]
    assert np.array_equal(acc, whole["ebc"]) and np.array_equal(bc, whole["bc"]) and np.array_equal(cnt, whole["cnt"])
