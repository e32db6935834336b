"""CPU: sweep cuts (include/lzx.h: lzx_sweep_cut) without a GPU -- the binding and the struct layouts, the argument error that
comes back before a device is touched, and a numpy restatement of the definitions (sweep_ref) against networkx.cut_size,
volume and conductance on every golden fixture and against known answers on small graphs.  The GPU tests use the same
restatement as their reference.

Every output is an integer or one correctly rounded division of two integers, so every comparison is equality."""
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
from test_communities_host import SMALL, graph_of, off_diagonal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LZX_ERR_ARG = -1
ASCENDING, PER_DEGREE, EXPANSION = 1, 2, 4
RESULT_KEYS = ("k", "cut", "vol", "den", "value")


# ---- the restatement ------------------------------------------------------------------------------------------------------
def sweep_ref(A, score, flags=0, k_min=0, k_max=0):
    """The definitions of lzx_sweep_cut for one score vector.  Returns a dict: order (n,) uint32, cut and vol (n,) uint64, M,
    and the best prefix's k, cut_k, vol_k, den (Python integers) and value (a Python float)."""
    n, _, ci, rows, off, d = off_diagonal(A)
    s = np.asarray(score, dtype=np.float64)
    assert s.shape == (n,) and not np.isnan(s).any()
    ids = np.arange(n, dtype=np.int64)
    key, last = s.copy(), np.zeros(n, dtype=np.int64)
    if flags & PER_DEGREE:
        has = d > 0
        key[has] = s[has] / d[has].astype(np.float64)
        key[~has] = 0.0
        last = (~has).astype(np.int64)                  # after all others whatever the score
    key = key + 0.0                                     # -0.0 counts as +0.0
    order = np.lexsort((ids, key if flags & ASCENDING else -key, last))
    pos = np.empty(n, dtype=np.int64)
    pos[order] = ids
    earlier = off & (pos[ci] < pos[rows])
    b = np.bincount(rows[earlier], minlength=n).astype(np.int64)
    cut, vol = np.cumsum((d - 2 * b)[order]), np.cumsum(d[order])
    M = int(d.sum())
    lo, hi = k_min if k_min else 1, k_max if k_max else n - 1
    best = None                                         # (cut, den, k)
    for k, ck, vk in zip(range(lo, hi + 1), cut[lo - 1:hi].tolist(), vol[lo - 1:hi].tolist()):
        den = min(k, n - k) if flags & EXPANSION else min(vk, M - vk)
        if den and (best is None or ck * best[1] < best[0] * den):
            best = (ck, den, k)
    r = dict(order=order.astype(np.uint32), cut=cut.astype(np.uint64), vol=vol.astype(np.uint64), M=M)
    if best is None:
        r.update(k=0, cut_k=0, vol_k=0, den=0, value=float("inf"))
    else:
        r.update(k=best[2], cut_k=best[0], vol_k=int(vol[best[2] - 1]), den=best[1], value=float(best[0]) / float(best[1]))
    return r


def result_of(r):
    """the restatement's best prefix under the names of lzx_sweep_result"""
    return dict(k=r["k"], cut=r["cut_k"], vol=r["vol_k"], den=r["den"], value=r["value"])


def many_ties(n):
    """an integer score with 13 values"""
    return ((np.arange(n, dtype=np.int64) * 7919 + 5) % 13).astype(np.float64)


def lopsided_barbell():
    """K8 joined to K12 by the edge (7, 8)"""
    return adjacency(20, clique_edges(range(8)) + clique_edges(range(8, 20)) + [(7, 8)])


def fiedler_vector(A):
    A = sp.csr_matrix(A).toarray()
    w, V = np.linalg.eigh(np.diag(A.sum(axis=1)) - A)
    return w[1], V[:, 1]


@functools.lru_cache(maxsize=None)
def fixture_graph(path):
    A = load_fixture(path)
    A.sort_indices()
    return A


# ---- the binding ----------------------------------------------------------------------------------------------------------
def test_entry_point_is_bound(pkg):
    L = pkg.lib()
    names = [name for name, _, _ in pkg.SYMBOLS]
    header = open(os.path.join(ROOT, "include", "lzx.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    hooks = open(os.path.join(ROOT, "msc-hpc-final-project_amd", "csrc", "lzx_test_hooks.h")).read()
    assert "lzx_sweep_cut" in names and hasattr(L, "lzx_sweep_cut")
    assert re.search(r"\bint lzx_sweep_cut\(", header) and re.search(r" T lzx_sweep_cut\b", out)
    for name, value in (("LZX_SWEEP_ASCENDING", 1), ("LZX_SWEEP_PER_DEGREE", 2), ("LZX_SWEEP_EXPANSION", 4)):
        assert re.search(rf"#define {name}\s+{value}u", header) and getattr(pkg, name) == value
    for shape in ("sweep_long_row", "sweep_state_bytes"):
        assert shape in pkg.SHAPE_OPTIONS and f'"{shape}"' in hooks
    for method in ("sweep_cut_raw", "sweep_cut", "cut_size", "volume", "conductance", "edge_expansion", "spectral_bisection", "local_cluster"):
        assert hasattr(pkg.Engine, method)


LAYOUTS = [("LzxSweepResult", "lzx_sweep_result", 40, set(RESULT_KEYS)),
           ("LzxSweepInfo", "lzx_sweep_info", 48, {"entries", "ns", "width", "loop_ms", "sort_ms", "sweep_ms", "scan_ms"})]


@pytest.mark.parametrize("cls,struct,size,public", LAYOUTS, ids=[l[1] for l in LAYOUTS])
def test_layouts_match_the_header(pkg, tmp_path, cls, struct, size, public):
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
    scores = (ctypes.c_double * 4)()
    best = (pkg.LzxSweepResult * 1)()
    assert L.lzx_sweep_cut(None, 1, scores, 0, 0, 0, None, None, None, best, None) == LZX_ERR_ARG
    msg = L.lzx_last_error().decode()
    assert "lzx_sweep_cut" in msg and "null handle" in msg, msg


# ---- the restatement against networkx -------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=GOLDEN_IDS)
def test_restatement_on_the_fixtures(path):
    A = fixture_graph(path)
    n = A.shape[0]
    G = graph_of(A)
    r = sweep_ref(A, many_ties(n))
    order = r["order"].astype(np.int64)
    assert sorted(order.tolist()) == list(range(n))
    for k in (1, 7, n // 3, n // 2, n - 1):
        S = order[:k].tolist()
        assert int(r["cut"][k - 1]) == nx.cut_size(G, S) and int(r["vol"][k - 1]) == nx.volume(G, S), k
    assert int(r["cut"][n - 1]) == 0 and int(r["vol"][n - 1]) == r["M"] == A.nnz
    assert 1 <= r["k"] <= n - 1 and r["value"] == nx.conductance(G, order[:r["k"]].tolist())
    assert r["cut_k"] == int(r["cut"][r["k"] - 1]) and r["vol_k"] == int(r["vol"][r["k"] - 1]) and r["den"] == min(r["vol_k"], r["M"] - r["vol_k"])
    x = sweep_ref(A, many_ties(n), EXPANSION)
    assert x["value"] == nx.edge_expansion(G, x["order"][:x["k"]].tolist()) and np.array_equal(x["order"], r["order"])
    print(os.path.basename(path), result_of(r), result_of(x))


def known(A, score, **kw):
    r = sweep_ref(A, score, **kw)
    return r["k"], r["cut_k"], r["den"]


def test_known_answers():
    assert known(SMALL["path_65"](), -np.arange(65.0)) == (32, 1, 63)
    assert known(SMALL["ring_of_cliques_12x6"](), -np.arange(72.0)) == (36, 2, 192)
    barbell = adjacency(12, clique_edges(range(6)) + clique_edges(range(6, 12)) + [(5, 6)])
    lam, f = fiedler_vector(barbell)
    assert known(barbell, f) == known(barbell, -f) == (6, 1, 31)
    r = sweep_ref(barbell, f)
    assert sorted(r["order"][:6].tolist()) in (list(range(6)), list(range(6, 12))) and r["value"] == 1.0 / 31.0
    lop = lopsided_barbell()
    lam, f = fiedler_vector(lop)
    got = {known(lop, f), known(lop, -f)}
    assert got == {(8, 1, 57), (12, 1, 57)}
    for sign in (1.0, -1.0):
        r = sweep_ref(lop, sign * f)
        assert sorted(r["order"][:r["k"]].tolist()) in (list(range(8)), list(range(8, 20)))
        assert r["value"] == 1.0 / 57.0 == nx.conductance(graph_of(lop), range(8))


def test_order_rules():
    A = SMALL["k5_k10_and_7_isolated"]()
    n = A.shape[0]
    s = many_ties(n)
    down, up = sweep_ref(A, s), sweep_ref(A, s, ASCENDING)
    for r, sign in ((down, -1.0), (up, 1.0)):
        o = r["order"].astype(np.int64)
        keys = list(zip((sign * s[o]).tolist(), o.tolist()))
        assert keys == sorted(keys)                                        # ties by ascending id in both directions
    for flags in (PER_DEGREE, PER_DEGREE | ASCENDING):
        r = sweep_ref(A, s + 100.0, flags)
        assert r["order"][15:].tolist() == list(range(15, 22))             # the isolated vertices last, by id
    z = np.zeros(n)
    z[::2] = -0.0
    assert sweep_ref(A, z)["order"].tolist() == list(range(n))            # -0.0 counts as +0.0
    e = np.zeros(n)
    e[3], e[4] = np.inf, -np.inf
    o = sweep_ref(A, e)["order"].tolist()
    assert o[0] == 3 and o[-1] == 4
    const = sweep_ref(A, np.full(n, 2.5))
    assert const["order"].tolist() == list(range(n))


def test_windows_and_graphs_without_an_admissible_prefix():
    for A in (sp.csr_matrix((5, 5)), sp.csr_matrix((1, 1))):
        r = sweep_ref(A, np.arange(A.shape[0], dtype=np.float64))
        assert result_of(r) == dict(k=0, cut=0, vol=0, den=0, value=float("inf")) and r["M"] == 0
    A = SMALL["caveman_10x8"]()
    n = A.shape[0]
    assert sweep_ref(A, -np.arange(n, dtype=np.float64), k_min=n, k_max=n)["k"] == 0          # the whole graph: den = 0
    G = graph_of(A)
    ind = np.zeros(n)
    S = [3, 9, 17, 18, 40, 77]
    ind[S] = 1.0
    r = sweep_ref(A, ind, k_min=len(S), k_max=len(S))
    assert sorted(r["order"][:len(S)].tolist()) == S
    assert (r["cut_k"], r["vol_k"], r["value"]) == (nx.cut_size(G, S), nx.volume(G, S), nx.conductance(G, S))
    assert sweep_ref(A, ind, EXPANSION, len(S), len(S))["value"] == nx.edge_expansion(G, S)
    # ties of the ratio go to the smallest k: a path of 4 by id has cut 1 at every k, den 1, 3, 1
    P = adjacency(4, [(0, 1), (1, 2), (2, 3)])
    assert known(P, -np.arange(4.0)) == (2, 1, 3)
    assert known(P, -np.arange(4.0), flags=EXPANSION) == (2, 1, 2)
    assert known(P, -np.arange(4.0), k_min=3) == (3, 1, 1)


def test_self_loops_change_nothing():
    A = fixture_graph(GOLDEN[GOLDEN_IDS.index("er_n1000")])
    n = A.shape[0]
    loops = np.zeros(n)
    loops[::20] = 1.0
    B = sp.csr_matrix(A + sp.diags(loops))
    B.sort_indices()
    assert B.nnz == A.nnz + 50
    s = np.random.default_rng(5).standard_normal(n)
    for flags in (0, PER_DEGREE | ASCENDING | EXPANSION):
        a, b = sweep_ref(A, s, flags), sweep_ref(B, s, flags)
        assert all(np.array_equal(a[key], b[key]) for key in a)
