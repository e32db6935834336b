"""CPU: the similarity of two vertices (include/lzx.h: lzx_similarity) without a GPU -- the binding and the struct layout, the
argument error that comes back before a device is touched, and a numpy restatement of the definitions (similarity_restated: rows
without the diagonal, the intersection of two ascending rows, the formulas of the header) against networkx.link_prediction on the
karate club and on every golden fixture.  The GPU tests use the same restatement as their reference.

Integers and the three ratios (one correctly rounded division of two integers below 2^53) are compared by equality.  A sum over c
terms is compared with math.fsum of the Python terms within (2 c + 8) 2^-53, relative: at most 2 2^-53 for the log on either side,
one division on either side, c - 1 additions on either side.  A sum over no term is exactly 0.0."""
import ctypes
import functools
import glob
import math
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
EPS = 2.0 ** -53
RATIOS = ("jaccard", "overlap", "sorensen")
SUMS = ("adamic_adar", "resource_allocation")


def sum_bound(terms):
    """the absolute bound on a sum of these terms"""
    return (2 * len(terms) + 8) * EPS * math.fsum(terms)


def sum_error_ratio(got, terms):
    """|got - fsum(terms)| / bound (0.0 for an exact empty sum, inf for a wrong one)"""
    if not terms:
        return 0.0 if (got == 0.0 and not math.copysign(1.0, got) < 0) else math.inf
    return abs(got - math.fsum(terms)) / sum_bound(terms)


def similarity_restated(A, pairs):
    """The definitions of lzx_similarity on a scipy CSR adjacency matrix A (symmetric, self loops allowed) for an (np, 2) array of
    pairs u != v.  Returns a dict: common, deg_u, deg_v, preferential_attachment (int64), jaccard, overlap, sorensen, cosine
    (float64), adamic_adar, resource_allocation (float64: math.fsum of the terms), terms_aa, terms_ra (lists of lists of the
    Python terms 1 / math.log(d_w), 1 / d_w, ascending w) and shorter (int64: min(|row u|, |row v|), stored lengths)."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    rp, ci = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    deg = np.bincount(rows[rows != ci], minlength=n).astype(np.int64)

    def N(x):
        r = ci[rp[x]:rp[x + 1]]
        return r[r != x]

    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = {k: [] for k in ("common", "deg_u", "deg_v", "preferential_attachment", "shorter") + RATIOS + ("cosine",) + SUMS + ("terms_aa", "terms_ra")}
    for u, v in pairs.tolist():
        assert u != v
        w = np.intersect1d(N(u), N(v), assume_unique=True)        # ascending; holds neither u nor v
        c, du, dv = len(w), int(deg[u]), int(deg[v])
        out["common"].append(c)
        out["deg_u"].append(du)
        out["deg_v"].append(dv)
        out["preferential_attachment"].append(du * dv)
        out["shorter"].append(int(min(rp[u + 1] - rp[u], rp[v + 1] - rp[v])))
        out["jaccard"].append(c / (du + dv - c) if du + dv - c else 0.0)
        out["overlap"].append(c / min(du, dv) if min(du, dv) else 0.0)
        out["sorensen"].append(2 * c / (du + dv) if du + dv else 0.0)
        out["cosine"].append(c / math.sqrt(du * dv) if du * dv else 0.0)
        taa = [1.0 / math.log(int(deg[x])) for x in w.tolist()]
        tra = [1.0 / int(deg[x]) for x in w.tolist()]
        out["terms_aa"].append(taa)
        out["terms_ra"].append(tra)
        out["adamic_adar"].append(math.fsum(taa))
        out["resource_allocation"].append(math.fsum(tra))
    for k in ("common", "deg_u", "deg_v", "preferential_attachment", "shorter"):
        out[k] = np.array(out[k], dtype=np.int64)
    for k in RATIOS + ("cosine",) + SUMS:
        out[k] = np.array(out[k], dtype=np.float64)
    return out


def load_fixture(path):
    g = np.load(path)
    rp, ci = g["ref_row_offset"].astype(np.int64), g["ref_col_idx"].astype(np.int64)
    n = len(rp) - 1
    return sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))


def without_loops(A):
    A = sp.csr_matrix(A).copy()
    A.setdiag(0)
    A.eliminate_zeros()
    A.sort_indices()
    return A


def sample_pairs(A, seed, n_random=400, n_edges=200):
    """n_random seeded random pairs u != v, then n_edges stored entries off the diagonal (fewer where the graph has fewer)"""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    u = rng.integers(0, n, n_random)
    v = (u + rng.integers(1, n, n_random)) % n
    coo = A.tocoo()
    off = np.flatnonzero(coo.row != coo.col)
    pick = rng.choice(off, size=min(n_edges, len(off)), replace=False)
    return np.concatenate([np.stack([u, v], axis=1), np.stack([coo.row[pick], coo.col[pick]], axis=1)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def fixture_case(path):
    """(A without self loops, the sampled pairs, the restatement on them) of one fixture, computed once and shared (read-only)"""
    A = without_loops(load_fixture(path))
    pairs = sample_pairs(A, 23)
    return A, pairs, similarity_restated(A, pairs)


def assert_equals_networkx(A, pairs, r):
    G = nx.from_scipy_sparse_array(sp.csr_matrix(A))
    assert nx.number_of_selfloops(G) == 0
    bunch = [tuple(p) for p in pairs.tolist()]
    assert [len(list(nx.common_neighbors(G, u, v))) for u, v in bunch] == r["common"].tolist()
    assert [p for _, _, p in nx.jaccard_coefficient(G, bunch)] == r["jaccard"].tolist()
    assert [p for _, _, p in nx.preferential_attachment(G, bunch)] == r["preferential_attachment"].tolist()
    worst = 0.0
    for key, terms, fn in (("adamic_adar", "terms_aa", nx.adamic_adar_index), ("resource_allocation", "terms_ra", nx.resource_allocation_index)):
        for (_, _, got), t, mine in zip(fn(G, bunch), r[terms], r[key]):
            ratio = sum_error_ratio(got, t)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (key, got, mine)
    print("networkx sums: worst error / bound", worst, "largest c", int(r["common"].max()), "longest shorter row", int(r["shorter"].max()))


# ---- the binding --------------------------------------------------------------------------------------------------------
def test_entry_point_is_bound(pkg):
    L = pkg.lib()
    names = [name for name, _, _ in pkg.SYMBOLS]
    header = open(os.path.join(ROOT, "include", "lzx.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert "lzx_similarity" in names and hasattr(L, "lzx_similarity")
    assert re.search(r"\bint lzx_similarity\(", header) and "lzx_similarity_info" in header
    assert re.search(r" T lzx_similarity\b", out)
    for shape in ("sim_long_pair", "sim_slice", "sim_state_bytes"):
        assert shape in pkg.SHAPE_OPTIONS
        assert f'"{shape}"' in open(os.path.join(ROOT, "msc-hpc-final-project_amd", "csrc", "lzx_api.hip")).read()
        assert f'"{shape}"' in open(os.path.join(ROOT, "msc-hpc-final-project_amd", "csrc", "lzx_test_hooks.h")).read()
    for name, bit in (("JACCARD", 1), ("OVERLAP", 2), ("SORENSEN", 4), ("ADAMIC_ADAR", 8), ("RESOURCE_ALLOCATION", 16)):
        assert getattr(pkg, "LZX_SIM_" + name) == bit and re.search(rf"#define LZX_SIM_{name}\s+{bit}u", header)
    assert list(pkg.SIM_MEASURES.values()) == [1, 2, 4, 8, 16]
    for method in ("similarity_raw", "common_neighbors_count", "jaccard_coefficient", "overlap_coefficient", "sorensen_coefficient",
                   "adamic_adar_index", "resource_allocation_index", "preferential_attachment", "cosine_similarity", "edge_similarity"):
        assert hasattr(pkg.Engine, method)


def test_info_layout_matches_the_header(pkg, tmp_path):
    fields = [f for f, _ in pkg.LzxSimilarityInfo._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "lzx.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(lzx_similarity_info));']
    src += [f'printf("{f} %zu\\n", offsetof(lzx_similarity_info, {f}));' for f in fields]
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(pkg.LzxSimilarityInfo) == 5 * 8 + 2 * 4 + 3 * 8
    for f in fields:
        assert int(got[f]) == getattr(pkg.LzxSimilarityInfo, f).offset, f


def test_argument_error_without_gpu(pkg):
    L = pkg.lib()
    info = pkg.LzxSimilarityInfo()
    for args in ((None, 0, None, None, 0, None, None, None, None, None), (None, 3, None, None, 1, None, None, None, None, ctypes.byref(info))):
        assert L.lzx_similarity(*args) == LZX_ERR_ARG
        msg = L.lzx_last_error().decode()
        assert "lzx_similarity" in msg and "null handle" in msg, msg


# ---- the restatement against networkx -------------------------------------------------------------------------------------
def test_restatement_on_the_karate_club():
    G = nx.karate_club_graph()
    A = sp.csr_matrix(nx.to_scipy_sparse_array(G, weight=None, format="csr"))
    pairs = sample_pairs(A, 23)
    assert len(pairs) == 400 + 2 * G.number_of_edges()
    r = similarity_restated(A, pairs)
    assert_equals_networkx(A, pairs, r)
    one = similarity_restated(A, [(0, 33)])                        # the two hubs: not adjacent, four common neighbours
    assert one["common"].tolist() == [4] and one["deg_u"].tolist() == [16] and one["deg_v"].tolist() == [17]
    assert one["jaccard"].tolist() == [4 / 29] and one["overlap"].tolist() == [4 / 16] and one["sorensen"].tolist() == [8 / 33]


@pytest.mark.parametrize("path", GOLDEN, ids=GOLDEN_IDS)
def test_restatement_on_the_fixtures(path):
    A, pairs, r = fixture_case(path)
    assert len(pairs) == 600
    assert_equals_networkx(A, pairs, r)
    for k, t in enumerate(r["terms_aa"]):
        assert len(t) == r["common"][k] and all(math.isfinite(x) and x > 0 for x in t)      # a common neighbour has d_w >= 2
    assert (r["common"] <= np.minimum(r["deg_u"], r["deg_v"])).all() and (r["jaccard"] <= 1.0).all() and (r["overlap"] <= 1.0).all()
    assert (r["sorensen"] >= r["jaccard"]).all() and (r["cosine"] >= r["sorensen"] - 4 * EPS).all()
    swapped = similarity_restated(A, pairs[:50, ::-1])
    for key in ("common",) + RATIOS + SUMS:
        assert np.array_equal(swapped[key], r[key][:50]), key
    assert np.array_equal(swapped["deg_u"], r["deg_v"][:50])


def test_the_fixtures_reach_long_rows():
    """what the GPU tests rely on: sampled pairs of rmat_n3000_skew with more common neighbours than two wavefronts have lanes and a
    shorter row of more entries than a workgroup has threads; a row of 1499 in star_ring"""
    _, _, r = fixture_case(GOLDEN[GOLDEN_IDS.index("rmat_n3000_skew")])
    assert r["common"].max() > 128 and r["shorter"].max() > 256
    A, _, _ = fixture_case(GOLDEN[GOLDEN_IDS.index("star_ring_n1500")])
    assert int(np.diff(A.indptr).max()) == 1499


def test_self_loops_change_nothing():
    A, pairs, r = fixture_case(GOLDEN[GOLDEN_IDS.index("er_n1000")])
    n = A.shape[0]
    loops = np.zeros(n)
    loops[::7] = 1.0
    loops[pairs[:20].ravel()] = 1.0                                # on sampled ends as well
    B = sp.csr_matrix(A + sp.diags(loops))
    assert B.nnz == A.nnz + int(loops.sum()) and not A.diagonal().any()
    rb = similarity_restated(B, pairs)
    for key in ("common", "deg_u", "deg_v", "preferential_attachment") + RATIOS + ("cosine",) + SUMS:
        assert np.array_equal(rb[key], r[key]), key
    assert rb["terms_aa"] == r["terms_aa"] and rb["terms_ra"] == r["terms_ra"]


def test_a_relabelling_permutes_the_answers():
    A, pairs, r = fixture_case(GOLDEN[GOLDEN_IDS.index("rmat_n3000_skew")])
    n = A.shape[0]
    new_of_old = np.random.default_rng(5).permutation(n)
    P = sp.csr_matrix((np.ones(n), (new_of_old, np.arange(n))), shape=(n, n))
    rp = similarity_restated(sp.csr_matrix(P @ A @ P.T), new_of_old[pairs])
    for key in ("common", "deg_u", "deg_v", "preferential_attachment") + RATIOS + ("cosine",) + SUMS:      # (fsum does not depend on the order)
        assert np.array_equal(rp[key], r[key]), key
