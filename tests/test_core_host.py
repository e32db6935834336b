"""CPU: core numbers and onion layers (include/lzx.h: lzx_core_numbers) without a GPU -- the binding and the struct layout, the
argument error that comes back before a device is touched, and a numpy restatement of the definition (peel_rounds: degrees
without the diagonal, k_r = max(k_{r-1}, the smallest remaining degree), the frontier of remaining degree <= k_r removed at
once, one bincount of the frontier's entries subtracted from the remaining vertices) against networkx.core_number and
networkx.onion_layers on the karate club, on every golden fixture, on a fixture with self loops, on a relabelled fixture and
on a skewed graph with loops and a row of thousands of entries.  The GPU tests use the same restatement and networkx as their
references.

Everything here is an integer, so every comparison is equality."""
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
INTS = ("degeneracy", "rounds", "levels", "main_core_size", "core0")

# what the definition gives on the fixtures (checked against networkx below): degeneracy, rounds, levels, main core, core 0
EXPECTED = {"er_n1000": (7, 24, 7, 718, 0), "er_n4000_deg20": (14, 27, 7, 3497, 0), "er_c1_n10000": (14, 34, 9, 8883, 0),
            "rmat_n3000_skew": (66, 101, 45, 78, 747), "rmat_n4096": (41, 115, 38, 73, 1200), "star_ring_n1500": (3, 2, 1, 1500, 0)}


def peel_rounds(A):
    """The definition on a scipy CSR adjacency matrix A (symmetric, entries 1, self loops allowed).  Returns a dict: core, layer
    (n,) uint32, deg (n,) the degrees without the diagonal, and the Python integers degeneracy, rounds, levels, main_core_size,
    core0."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    rp, ci = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    off = rows != ci
    deg0 = np.bincount(rows[off], minlength=n).astype(np.int64)             # degrees without the diagonal
    deg = deg0.copy()
    core, layer = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    remaining = np.ones(n, dtype=bool)
    k = r = 0
    while remaining.any():
        r += 1
        k = max(k, int(deg[remaining].min()))
        frontier = np.flatnonzero(remaining & (deg <= k))
        core[frontier], layer[frontier] = k, r
        remaining[frontier] = False
        lengths = rp[frontier + 1] - rp[frontier]
        entries = ci[np.repeat(rp[frontier], lengths) + np.arange(int(lengths.sum())) - np.repeat(np.cumsum(lengths) - lengths, lengths)]
        entries = entries[entries != np.repeat(frontier, lengths)]
        deg -= np.bincount(entries, minlength=n) * remaining                 # one decrement per entry, onto the remaining vertices
    return dict(core=core, layer=layer, deg=deg0, degeneracy=k, rounds=r, levels=len(np.unique(core)),
                main_core_size=int((core == k).sum()), core0=int((core == 0).sum()))


def load_fixture(path):
    g = np.load(path)
    rp, ci = g["ref_row_offset"].astype(np.int64), g["ref_col_idx"].astype(np.int64)
    n = len(rp) - 1
    return sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))


def without_loops(A):
    B = sp.lil_matrix(sp.csr_matrix(A))
    B.setdiag(0)
    B = sp.csr_matrix(B)
    B.eliminate_zeros()
    return B


def networkx_reference(A):
    """(core (n,) uint32, layer (n,) uint32) of networkx on the graph of A, its self loops removed (networkx raises on them)"""
    G = nx.from_scipy_sparse_array(without_loops(A))
    n = A.shape[0]
    c, l = nx.core_number(G), nx.onion_layers(G)
    return np.array([c[v] for v in range(n)], dtype=np.uint32), np.array([l[v] for v in range(n)], dtype=np.uint32)


def assert_equals_networkx(r, ref):
    core, layer = ref
    assert np.array_equal(r["core"], core) and np.array_equal(r["layer"], layer)
    assert r["degeneracy"] == int(core.max()) and r["rounds"] == int(layer.max())
    assert r["levels"] == len(set(core.tolist())) and r["main_core_size"] == int((core == core.max()).sum())
    assert r["core0"] == int((core == 0).sum())


@functools.lru_cache(maxsize=None)
def fixture_case(path):
    """(A, restatement, networkx's (core, layer)) of one fixture, computed once and shared (read-only)"""
    A = load_fixture(path)
    return A, peel_rounds(A), networkx_reference(A)


@functools.lru_cache(maxsize=None)
def skewed_graph():
    """n = 2^14, 200 000 draws of both ends from n u^3: loops, a row of thousands of entries, hundreds of rounds.  (A, restatement)"""
    n, m = 1 << 14, 200000
    rng = np.random.default_rng(7)
    a = np.minimum((n * rng.random(m) ** 3).astype(np.int64), n - 1)
    b = np.minimum((n * rng.random(m) ** 3).astype(np.int64), n - 1)
    A = sp.csr_matrix(sp.coo_matrix((np.ones(2 * m), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n)))
    A.data[:] = 1.0
    A.sort_indices()
    return A, peel_rounds(A)


# ---- the binding --------------------------------------------------------------------------------------------------------
def test_entry_point_is_bound(pkg):
    L = pkg.lib()
    names = [name for name, _, _ in pkg.SYMBOLS]
    header = open(os.path.join(ROOT, "include", "lzx.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert "lzx_core_numbers" in names and hasattr(L, "lzx_core_numbers")
    assert re.search(r"\bint lzx_core_numbers\(", header) and "lzx_core_info" in header
    assert re.search(r" T lzx_core_numbers\b", out)
    assert "core_long_row" in pkg.SHAPE_OPTIONS and "core_state_bytes" in pkg.SHAPE_OPTIONS
    for method in ("core_number_raw", "core_number", "onion_layers", "degeneracy", "k_core", "k_shell"):
        assert hasattr(pkg.Engine, method)


def test_info_layout_matches_the_header(pkg, tmp_path):
    fields = [f for f, _ in pkg.LzxCoreInfo._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "lzx.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(lzx_core_info));']
    src += [f'printf("{f} %zu\\n", offsetof(lzx_core_info, {f}));' for f in fields]
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(pkg.LzxCoreInfo) == 48
    for f in fields:
        assert int(got[f]) == getattr(pkg.LzxCoreInfo, f).offset, f
    assert set(pkg.LzxCoreInfo().as_dict()) == set(fields) - {"reserved_"}


def test_argument_error_without_gpu(pkg):
    L = pkg.lib()
    info = pkg.LzxCoreInfo()
    for args in ((None, None, None, None), (None, None, None, ctypes.byref(info))):
        assert L.lzx_core_numbers(*args) == LZX_ERR_ARG
        msg = L.lzx_last_error().decode()
        assert "lzx_core_numbers" in msg and "null handle" in msg, msg


# ---- the restatement against networkx -------------------------------------------------------------------------------------
def test_restatement_on_the_karate_club():
    G = nx.karate_club_graph()
    A = sp.csr_matrix(nx.to_scipy_sparse_array(G, weight=None, format="csr"))
    r = peel_rounds(A)
    assert_equals_networkx(r, networkx_reference(A))
    assert r["degeneracy"] == 4 and r["core0"] == 0


@pytest.mark.parametrize("path", GOLDEN, ids=GOLDEN_IDS)
def test_restatement_on_the_fixtures(path):
    A, r, ref = fixture_case(path)
    assert not A.diagonal().any()
    assert_equals_networkx(r, ref)
    assert tuple(r[key] for key in INTS) == EXPECTED[os.path.basename(path)[:-4]]


def test_every_fixture_has_its_expected_values():
    assert sorted(EXPECTED) == sorted(GOLDEN_IDS)


def test_self_loops_change_nothing():
    A, r, ref = fixture_case(GOLDEN[GOLDEN_IDS.index("er_n1000")])
    n = A.shape[0]
    loops = np.zeros(n)
    loops[::7] = 1.0
    B = sp.csr_matrix(A + sp.diags(loops))
    assert B.nnz == A.nnz + len(loops[::7]) and not A.diagonal().any()
    rb = peel_rounds(B)
    assert_equals_networkx(rb, ref)                             # networkx on the loop-free graph
    for key in ("core", "layer", "deg"):
        assert np.array_equal(rb[key], r[key]), key
    for key in INTS:
        assert rb[key] == r[key], key


def test_a_relabelling_permutes_the_vectors():
    A, r, _ = fixture_case(GOLDEN[GOLDEN_IDS.index("rmat_n3000_skew")])
    n = A.shape[0]
    new_of_old = np.random.default_rng(5).permutation(n)
    P = sp.csr_matrix((np.ones(n), (new_of_old, np.arange(n))), shape=(n, n))
    rp = peel_rounds(sp.csr_matrix(P @ A @ P.T))
    assert np.array_equal(rp["core"][new_of_old], r["core"]) and np.array_equal(rp["layer"][new_of_old], r["layer"])
    for key in INTS:
        assert rp[key] == r[key], key


def test_restatement_on_the_skewed_graph():
    """the properties tests/test_gpu_core.py relies on: self loops, a row beyond every long-row threshold, hundreds of rounds"""
    A, r = skewed_graph()
    assert_equals_networkx(r, networkx_reference(A))
    loops, longest = int(A.diagonal().sum()), int(np.diff(A.indptr).max())
    print("nnz", A.nnz, "loops", loops, "largest row", longest, {key: r[key] for key in INTS})
    assert loops > 0 and longest > 4096 and r["rounds"] > 100
    assert np.array_equal(r["deg"], np.diff(A.indptr) - A.diagonal().astype(np.int64))
