"""CPU: connected components and induced subgraphs (include/lzx.h: lzx_components, lzx_set_graph_induced) -- the entry points are
bound, the ctypes struct has the header's layout, the argument errors need no GPU, and a numpy restatement of the device scheme
(csrc/lzx_components.hip: hooking by minimum + pointer jumping, every write a minimum into the next label array) gives scipy's
partition with min-id labels.  tests/test_gpu_components.py imports the restatement and the graphs from here."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))
GENERATED = ("path5000", "path5000_shuffled", "grid70", "loops_and_isolated")


def fixture(name):
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
    return g["ref_row_offset"].astype(np.uint64), g["ref_col_idx"].astype(np.uint32)


def csr_of_edges(n, u, v):
    """Symmetric pattern CSR (columns ascending, no duplicates; a self loop is one diagonal entry) of the edges (u[i], v[i])."""
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    A = sp.coo_matrix((np.ones(2 * len(u)), (np.concatenate([u, v]), np.concatenate([v, u]))), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A.indptr.astype(np.uint64), A.indices.astype(np.uint32)


def generated(name):
    if name == "path5000":
        return csr_of_edges(5000, np.arange(4999), np.arange(1, 5000))
    if name == "path5000_shuffled":
        p = np.random.default_rng(11).permutation(5000)
        return csr_of_edges(5000, p[:-1], p[1:])
    if name == "grid70":
        idx = np.arange(70 * 70).reshape(70, 70)
        return csr_of_edges(70 * 70, np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()]),
                            np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()]))
    if name == "loops_and_isolated":   # 400 vertices: a seeded sparse random part with self loops, every fifth vertex left without an edge
        rng = np.random.default_rng(5)
        live = np.array([i for i in range(400) if i % 5 != 0])
        u, v = rng.choice(live, 260), rng.choice(live, 260)
        loops = live[::7]
        return csr_of_edges(400, np.concatenate([u, loops]), np.concatenate([v, loops]))
    raise KeyError(name)


def graph(name):
    return generated(name) if name in GENERATED else fixture(name)


def scipy_labels(rp, ci):
    """The canonical labelling: labels[i] = the smallest vertex id of i's component, from scipy's connected_components."""
    n = len(rp) - 1
    A = sp.csr_matrix((np.ones(len(ci)), ci.astype(np.int64), rp.astype(np.int64)), shape=(n, n))
    _, comp = csg.connected_components(A, directed=False)
    first = np.full(comp.max() + 1, n, dtype=np.int64)
    np.minimum.at(first, comp, np.arange(n))
    return first[comp].astype(np.uint32)


def counts_of(labels):
    """(n_components, largest_size, largest_label; ties: the smallest label) of a canonical labelling."""
    roots, sizes = np.unique(labels, return_counts=True)
    return len(roots), int(sizes.max()), int(roots[np.argmax(sizes)])


def components_restatement(rp, ci):
    """The device scheme in numpy: f (parent, starts as the identity) and gf = f[f]; one round reads f and gf only and lowers the
    NEXT array fn (a copy of f) by minimum, so the order of the writes cannot matter:
        m[u]      = min(gf[u], min over the neighbours v of u of gf[v])        (the pull sweep over the CSR)
        fn[u]     = min(fn[u], m[u])                                            (u takes the smallest grandparent around it)
        fn[f[u]]  = min(fn[f[u]], m[u])                                         (and hooks its parent there as well)
    then f = fn and gf = fn[fn] (one pointer jump).  The round in which nothing was lowered is the last and is counted.
    Returns (labels, rounds)."""
    n = len(rp) - 1
    rp64, ci64 = rp.astype(np.int64), ci.astype(np.int64)
    rows = np.repeat(np.arange(n), np.diff(rp64))
    f = np.arange(n, dtype=np.int64)
    gf = f.copy()
    rounds = 0
    while True:
        rounds += 1
        assert rounds <= n + 1
        m = gf.copy()
        np.minimum.at(m, rows, gf[ci64])
        fn = f.copy()
        np.minimum.at(fn, np.arange(n), m)
        np.minimum.at(fn, f, m)
        if np.array_equal(fn, f):
            return f.astype(np.uint32), rounds
        f = fn
        gf = f[f]


def test_entry_points_are_bound(pkg):
    L = pkg.lib()
    names = [n for n, _, _ in pkg.SYMBOLS]
    for name in ("lzx_components", "lzx_set_graph_induced"):
        assert name in names and hasattr(L, name), name


def test_components_info_layout_matches_the_header(pkg, tmp_path):
    fs = [f for f, _ in pkg.LzxComponentsInfo._fields_]
    assert fs == ["n_components", "largest_size", "largest_label", "rounds", "loop_ms", "sweep_ms"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "lzx.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(lzx_components_info));']
    src += [f'printf("{f} %zu\\n", offsetof(lzx_components_info, {f}));' for f in fs]
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(pkg.LzxComponentsInfo)
    for f in fs:
        assert int(got[f]) == getattr(pkg.LzxComponentsInfo, f).offset, f


def test_null_handles_are_argument_errors(pkg):
    L = pkg.lib()
    labels = np.zeros(4, dtype=np.uint32)
    assert L.lzx_components(None, labels.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None) == -1
    assert b"lzx_components" in L.lzx_last_error() and b"null" in L.lzx_last_error()
    keep = np.ones(4, dtype=np.uint8)
    assert L.lzx_set_graph_induced(None, None, keep.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), None, None) == -1
    assert b"lzx_set_graph_induced" in L.lzx_last_error() and b"null" in L.lzx_last_error()


ROUNDS = {}


@pytest.mark.parametrize("name", [os.path.basename(p)[:-4] for p in GOLDEN] + list(GENERATED))
def test_restatement_gives_scipys_partition(name, record_property):
    rp, ci = graph(name)
    labels, rounds = components_restatement(rp, ci)
    assert np.array_equal(labels, scipy_labels(rp, ci)), name
    assert 1 <= rounds <= len(rp)
    ROUNDS[name] = rounds
    record_property("rounds", rounds)
    print(f"{name}: n={len(rp) - 1} nnz={len(ci)} rounds={rounds} components={counts_of(labels)}")


def test_expected_counts_of_the_golden_fixtures():
    assert len(GOLDEN) == 6
    for p in GOLDEN:
        name = os.path.basename(p)[:-4]
        rp, ci = fixture(name)
        n = len(rp) - 1
        nc, big, _ = counts_of(scipy_labels(rp, ci))
        want = {"rmat_n3000_skew": (750, 2249), "rmat_n4096": (1204, 2890)}.get(name, (1, n))
        assert (nc, big) == want, name


def test_component_indicators_are_unit_vectors(pkg):
    rp, ci = graph("loops_and_isolated")
    labels = scipy_labels(rp, ci)
    roots, sizes = np.unique(labels, return_counts=True)
    which = roots[sizes > 1][:3]
    W = pkg.Engine.component_indicators(labels, which)
    assert W.shape == (len(which), len(labels))
    for w, r in zip(W, which):
        assert np.array_equal(w != 0, labels == r)
        assert abs(np.linalg.norm(w) - 1.0) <= 1e-15
    not_a_root = int(np.flatnonzero(labels != np.arange(len(labels)))[0])
    with pytest.raises(ValueError):
        pkg.Engine.component_indicators(labels, [not_a_root])
