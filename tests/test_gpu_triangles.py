"""GPU: triangle counts and clustering on the device (include/lzx.h: lzx_triangles; Engine.triangles / clustering / transitivity /
average_clustering): known answers on small graphs, the golden fixtures against networkx and the numpy restatement of
tests/test_triangles_host.py, every counting path forced, totals beyond 2^32, self loops, both hand-over forms, a relabelled
graph, isolation from the handle's other state, and the error paths.

Everything but one mean is an integer or one correctly rounded division of two integers: the comparisons are equality.
avg_clustering is a sum of n non-negative terms and one division, compared with math.fsum(c) / n within n 2^-53, relative (the
bound tests/test_paths_host.py uses for its sums)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

from test_triangles_host import GOLDEN, GOLDEN_IDS, fixture_case, triangles_oriented

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
INTS = ("triangles", "wedges", "max_triangles", "oriented_entries", "oriented_max_degree")


def golden(name):
    return GOLDEN[GOLDEN_IDS.index(name)]


def engine_of(pkg, A, **options):
    eng = pkg.Engine(0, **options)
    A = sp.csr_matrix(A)
    A.sort_indices()
    eng.set_graph_csr(A.indptr.astype(np.uint64), A.indices.astype(np.uint32))
    return eng


def adjacency(n, edges):
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    M = sp.coo_matrix((np.ones(2 * len(e)), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))), shape=(n, n))
    M = sp.csr_matrix(M)
    M.data[:] = 1.0
    return M


def complete_multipartite(*parts):
    label = np.repeat(np.arange(len(parts)), parts)
    return sp.csr_matrix((label[:, None] != label[None, :]).astype(np.float64)), label


def run(eng):
    tri, clus, info = eng.triangles_raw()
    return tri, clus, {k: info[k] for k in INTS + ("avg_clustering",)}


def check(eng, A, tri_ref, clus_ref=None):
    """one call against per-vertex counts; the coefficients and the scalars follow from them and the degrees"""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    d = np.diff(A.indptr).astype(np.int64) - A.diagonal().astype(np.int64)
    tri_ref = np.asarray(tri_ref, dtype=np.uint64)
    tri, clus, info = run(eng)
    assert tri.dtype == np.uint64 and np.array_equal(tri, tri_ref)
    t = tri_ref.astype(np.int64)
    c = np.zeros(n)
    nz = (d >= 2) & (t > 0)
    c[nz] = (2 * t[nz]) / (d[nz] * (d[nz] - 1))
    assert np.array_equal(clus, c)
    if clus_ref is not None:
        assert np.array_equal(clus, clus_ref)
    assert info["triangles"] == int(t.sum()) // 3 and info["wedges"] == int((d * (d - 1) // 2).sum())
    assert info["max_triangles"] == int(t.max())
    assert info["oriented_entries"] == (A.nnz - int(A.diagonal().sum())) // 2
    mean = math.fsum(c.tolist()) / n
    print("avg_clustering", info["avg_clustering"], "fsum / n", mean, "bound", n * EPS * mean)
    assert abs(info["avg_clustering"] - mean) <= n * EPS * mean
    return tri, clus, info


# ---- 1. known answers -----------------------------------------------------------------------------------------------------
def complete_graph(n):
    return sp.csr_matrix(1.0 - np.eye(n)), np.full(n, math.comb(n - 1, 2))


def wheel_graph(rim):
    edges = [(0, k) for k in range(1, rim + 1)] + [(k, k % rim + 1) for k in range(1, rim + 1)]
    return adjacency(rim + 1, edges), np.array([rim] + [2] * rim)


def tripartite(a, b, c):
    A, label = complete_multipartite(a, b, c)
    return A, np.array([b * c, a * c, a * b])[label]


def windmill(blades):
    edges = []
    for k in range(blades):
        u, v = 1 + 2 * k, 2 + 2 * k
        edges += [(0, u), (0, v), (u, v)]
    return adjacency(2 * blades + 1, edges), np.array([blades] + [1] * (2 * blades))


def triangle_free(A):
    A = sp.csr_matrix(A)
    return A, np.zeros(A.shape[0], dtype=np.uint64)


def grid_graph(m):
    n = m * m
    return adjacency(n, [(k, k + 1) for k in range(n) if (k + 1) % m] + [(k, k + m) for k in range(n - m)])


def hypercube_graph(q):
    return adjacency(1 << q, [(v, v ^ (1 << k)) for v in range(1 << q) for k in range(q) if v < v ^ (1 << k)])


KNOWN = {"single_vertex": lambda: triangle_free(sp.csr_matrix((1, 1))),
         "one_edge": lambda: triangle_free(adjacency(2, [(0, 1)])),
         "path_65": lambda: triangle_free(adjacency(65, [(k, k + 1) for k in range(64)])),
         "cycle_64": lambda: triangle_free(adjacency(64, [(k, (k + 1) % 64) for k in range(64)])),
         "star_300": lambda: triangle_free(adjacency(300, [(0, k) for k in range(1, 300)])),
         "grid_8x8": lambda: triangle_free(grid_graph(8)),
         "hypercube_10": lambda: triangle_free(hypercube_graph(10)),
         "bipartite_30_40": lambda: triangle_free(complete_multipartite(30, 40)[0]),
         "complete_3": lambda: complete_graph(3), "complete_4": lambda: complete_graph(4),
         "complete_20": lambda: complete_graph(20), "complete_200": lambda: complete_graph(200),
         "wheel_65": lambda: wheel_graph(64),
         "tripartite_5_7_11": lambda: tripartite(5, 7, 11),
         "windmill_50": lambda: windmill(50)}


@pytest.mark.parametrize("name", list(KNOWN))
def test_known_answers(pkg, name):
    A, tri_ref = KNOWN[name]()
    eng = engine_of(pkg, A)
    _, clus, info = check(eng, A, tri_ref)
    if name.startswith("complete_"):
        assert (clus == 1.0).all() and info["avg_clustering"] == 1.0 and eng.transitivity() == 1.0
    if not np.asarray(tri_ref).any():
        assert eng.transitivity() == 0.0 and info["avg_clustering"] == 0.0 and info["max_triangles"] == 0
    eng.close()


# ---- 2. fixtures ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=GOLDEN_IDS)
def test_fixtures_against_networkx(pkg, path):
    A, r, (t_nx, c_nx, trans_nx) = fixture_case(path)
    eng = engine_of(pkg, A)
    tri, clus, info = check(eng, A, t_nx, c_nx)
    assert eng.transitivity() == trans_nx
    for key in INTS:
        assert info[key] == r[key], key
    nodes = np.array([0, A.shape[0] - 1, 17, 17])
    assert np.array_equal(eng.triangles(nodes), tri[nodes]) and np.array_equal(eng.clustering(nodes), clus[nodes])
    assert np.array_equal(eng.triangles(), tri) and np.array_equal(eng.clustering(), clus)
    assert eng.average_clustering() == info["avg_clustering"]
    nzc = clus[clus > 0]
    assert abs(eng.average_clustering(count_zeros=False) - math.fsum(nzc.tolist()) / len(nzc)) <= len(nzc) * EPS * 1.0
    for bad in ([A.shape[0]], [-1], [0.0], [3.7], np.array([True, False]), [[0, 1]]):
        with pytest.raises(ValueError):
            eng.triangles(bad)
        with pytest.raises(ValueError):
            eng.clustering(bad)
    assert eng.triangles([]).shape == (0,) and np.array_equal(eng.triangles(np.uint32(17)), tri[[17]])
    eng.close()


# ---- 3. every path --------------------------------------------------------------------------------------------------------
def layered_graph(low=10, mid=300, top=300):
    """`low` vertices joined to all of a complete bipartite graph on `mid` (two equal halves), which is joined to all of a
    complete graph on `top`: degrees mid < low + mid / 2 + top < mid + top - 1, so the ranks rise from layer to layer, with ties
    inside each.  A low vertex a has N+(a) = the middle layer (mid entries); a middle vertex b of the first half has
    N+(b) = the second half and the top (mid / 2 + top entries): on a -> b the list of a is the shorter one, it is walked, and
    it has mid / 2 hits."""
    n = low + mid + top
    layer = np.repeat([0, 1, 2, 3], [low, mid // 2, mid - mid // 2, top])
    joined = np.zeros((4, 4), dtype=bool)
    for p, q in ((0, 1), (0, 2), (1, 2), (1, 3), (2, 3), (3, 3)):
        joined[p, q] = joined[q, p] = True
    D = joined[layer[:, None], layer[None, :]] & ~np.eye(n, dtype=bool)
    return sp.csr_matrix(D.astype(np.float64))


def walks(r, walked_is_a, longer_than):
    """(out-edges a -> b of the oriented copy with k_a > longer_than on which the list of a (or of b) is walked, hits on them)"""
    ka, kb = r["out_degree"][r["out_rows"]], r["out_degree"][r["out_cols"]]
    return (ka > longer_than) & ((ka <= kb) == walked_is_a)


@functools.lru_cache(maxsize=None)
def path_case(name):
    if name == "complete_200":
        A = complete_graph(200)[0]
        return A, triangles_oriented(A)
    if name == "layered_10_300_300":
        A = layered_graph()
        D = A.toarray()
        r = triangles_oriented(A)
        assert np.array_equal(r["tri"].astype(np.int64), np.rint(((D @ D) * D).sum(axis=1)).astype(np.int64) // 2)
        return A, r
    A, r, _ = fixture_case(golden(name))
    return A, r


@pytest.mark.parametrize("name,long_list", [("rmat_n3000_skew", 4), ("star_ring_n1500", 4), ("complete_200", 4), ("complete_200", 1 << 20),
                                            ("layered_10_300_300", 4)])
def test_every_path_forced(pkg, name, long_list):
    """tri_long_list = 4: every oriented list of more than 4 entries takes the wide kernel, staged in LDS up to 128 entries and read
    where it lies beyond.  The wide kernel has four arms -- N+(a) staged or not, N+(a) or N+(b) walked:
      rmat_n3000_skew     lists of at most 72: staged, both walks
      complete_200        k_b < k_a on every out-edge: N+(b) walked, staged and (lists of 129 .. 199) not staged
      layered_10_300_300  lists of 300 .. 450 with k_a <= k_b: N+(a) walked, not staged
      star_ring_n1500     lists of at most 3: the wide kernel is not launched, with or without the shape
    The unforced run of complete_200 (threshold 128) has both kernels at work, with every long list staged; tri_long_list = 2^20
    gives its lists of 199 to the group kernel."""
    A, r = path_case(name)
    stage = 32 * 4
    if name == "rmat_n3000_skew":
        assert 4 < r["oriented_max_degree"] <= stage and walks(r, True, 4).any() and walks(r, False, 4).any()
    elif name == "complete_200":
        assert walks(r, False, stage).any() and (walks(r, False, 4) & ~walks(r, False, stage)).any() and not walks(r, True, 4).any()
    elif name == "layered_10_300_300":
        assert walks(r, True, stage).sum() >= 10 * 150 and r["triangles"] > 0
    else:
        assert r["oriented_max_degree"] <= 4
    unforced = engine_of(pkg, A)
    forced = engine_of(pkg, A, tri_long_list=long_list)
    t0, c0, i0 = run(unforced)
    t1, c1, i1 = run(forced)
    assert np.array_equal(t0, r["tri"]) and np.array_equal(c0, r["clustering"])
    assert np.array_equal(t1, t0) and np.array_equal(c1, c0) and i1 == i0
    assert np.array([i0["avg_clustering"]]).tobytes() == np.array([i1["avg_clustering"]]).tobytes()
    unforced.close()
    forced.close()


def test_totals_beyond_32_bits(pkg):
    """K_2955, the smallest complete graph with more than 2^32 triangles"""
    n = 2955
    assert math.comb(n, 3) > 2 ** 32 > math.comb(n - 1, 3)
    mask = ~np.eye(n, dtype=bool)
    eng = pkg.Engine(0)
    eng.set_graph_csr(np.arange(n + 1, dtype=np.uint64) * (n - 1), np.nonzero(mask)[1].astype(np.uint32))
    tri, clus, info = eng.triangles_raw()
    print("K_2955: loop_ms", info["loop_ms"], "orient_ms", info["orient_ms"], "count_ms", info["count_ms"])
    assert info["triangles"] == math.comb(n, 3) and info["wedges"] == n * math.comb(n - 1, 2)
    assert (tri == math.comb(n - 1, 2)).all() and info["max_triangles"] == math.comb(n - 1, 2)
    assert (clus == 1.0).all() and info["avg_clustering"] == 1.0
    assert info["oriented_entries"] == math.comb(n, 2) and info["oriented_max_degree"] == n - 1
    eng.close()


# ---- 4. self loops, hand-over forms, relabelling, repeats -----------------------------------------------------------------
def test_self_loops_change_nothing(pkg):
    A, r, _ = fixture_case(golden("er_n1000"))
    n = A.shape[0]
    coo = sp.triu(A).tocoo()
    loops = np.arange(0, n, 7)
    out = []
    for extra in (np.zeros(0, dtype=np.int64), loops):
        eng = pkg.Engine(0)
        eng.set_graph_edges(n, np.concatenate([coo.row, extra]), np.concatenate([coo.col, extra]))
        assert eng.info()["nnz"] == A.nnz + len(extra)
        out.append(run(eng) + (eng.transitivity(),))
        eng.close()
    (t0, c0, i0, tr0), (t1, c1, i1, tr1) = out
    assert np.array_equal(t0, r["tri"]) and np.array_equal(t0, t1) and np.array_equal(c0, c1)
    assert i0 == i1 and tr0 == tr1 == r["transitivity"]      # wedges and avg_clustering among them


def test_hand_over_form_does_not_matter(pkg):
    A, r, _ = fixture_case(golden("er_n4000_deg20"))
    out = []
    for pb in (1, 0):
        eng = engine_of(pkg, A, propagation_blocking=pb)
        out.append(run(eng))
        eng.close()
    (t0, c0, i0), (t1, c1, i1) = out
    assert np.array_equal(t0, r["tri"]) and np.array_equal(t0, t1) and np.array_equal(c0, c1) and i0 == i1


def test_a_relabelled_graph_gives_the_permuted_vector(pkg):
    A, r, _ = fixture_case(golden("rmat_n4096"))
    n = A.shape[0]
    new_of_old = np.random.default_rng(6).permutation(n)
    P = sp.csr_matrix((np.ones(n), (new_of_old, np.arange(n))), shape=(n, n))
    eng = engine_of(pkg, sp.csr_matrix(P @ A @ P.T))
    tri, clus, info = run(eng)
    assert np.array_equal(tri[new_of_old], r["tri"]) and np.array_equal(clus[new_of_old], r["clustering"])
    for key in ("triangles", "wedges", "max_triangles", "oriented_entries"):
        assert info[key] == r[key], key
    eng.close()


def test_two_calls_give_the_same_bits(pkg):
    A, r, _ = fixture_case(golden("rmat_n3000_skew"))
    eng = engine_of(pkg, A)
    t0, c0, i0 = run(eng)
    t1, c1, i1 = run(eng)
    assert np.array_equal(t0, t1) and np.array_equal(c0, c1) and i0 == i1
    assert np.array([i0["avg_clustering"]]).tobytes() == np.array([i1["avg_clustering"]]).tobytes()
    eng.close()


def test_counts_only(pkg):
    A, r, _ = fixture_case(golden("er_n1000"))
    eng = engine_of(pkg, A)
    info = pkg.LzxTrianglesInfo()
    assert eng.L.lzx_triangles(eng.h, None, None, ctypes.byref(info)) == 0
    assert info.triangles == r["triangles"] and info.wedges == r["wedges"] and info.max_triangles == r["max_triangles"]
    assert eng.L.lzx_triangles(eng.h, None, None, None) == 0
    tri = np.zeros(A.shape[0], dtype=np.uint64)
    assert eng.L.lzx_triangles(eng.h, tri.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), None, None) == 0
    assert np.array_equal(tri, r["tri"])
    eng.close()


# ---- 5. isolation ---------------------------------------------------------------------------------------------------------
def test_a_chunked_decomposition_is_left_alone(pkg):
    A, r, _ = fixture_case(golden("er_n1000"))
    x0 = np.random.default_rng(8).standard_normal(A.shape[0])
    eng = engine_of(pkg, A)
    a_ref, b_ref, Q_ref, _, _ = eng.lanczos(x0, 20)
    eng.lanczos_prepare(x0, 20)
    eng.lanczos_run_steps(7)
    assert np.array_equal(eng.triangles(), r["tri"])
    assert eng.lanczos_progress() == (7, 20)
    eng.lanczos_run_steps(13)
    a, b, Q = eng.lanczos_fetch(20, want_q=True)
    assert np.array_equal(a, a_ref) and np.array_equal(b, b_ref) and np.array_equal(Q, Q_ref)
    eng.close()


def test_the_resident_bases_are_left_alone(pkg):
    A, r, _ = fixture_case(golden("rmat_n3000_skew"))
    n = A.shape[0]
    rng = np.random.default_rng(9)
    x0, X0 = rng.standard_normal(n), rng.standard_normal((3, n))
    t, T = rng.standard_normal(12), rng.standard_normal((3, 12))
    eng = engine_of(pkg, A)
    eng.lanczos(x0, 12, want_q=False)
    eng.lanczos_multi(X0, 12)
    ans, ans_m = eng.multout(t), eng.multout_multi(T)
    assert np.array_equal(eng.triangles(), r["tri"])
    assert np.array_equal(eng.multout(t), ans) and np.array_equal(eng.multout_multi(T), ans_m)
    # a kept probe basis
    alpha, beta, k_used, _ = eng.lanczos_probes(3, 0, 4, 12, keep_basis=True)
    Tp = pkg.slq_diag_coefficients(alpha, beta, k_used, n, 0.1, 0.0)
    diag = eng.probe_diag(Tp)
    assert np.array_equal(eng.clustering(), r["clustering"])
    assert np.array_equal(eng.probe_diag(Tp), diag) and np.array_equal(eng.multout(t), ans)
    eng.close()


def test_a_matrix_that_is_not_symmetric_stays_within_its_memory(pkg):
    """The upper triangle of a path alone: symmetry is the caller's promise and is not checked, the counts of such a matrix mean
    nothing, but the oriented columns hold what the fill writes -- here n - 2 entries (v -> v + 1 for every v but the last two
    rows: the last vertex has no entry and ranks below all), more than the nnz / 2 a symmetric matrix of as many entries has."""
    n = 1000
    eng = pkg.Engine(0)
    eng.set_graph_csr(np.minimum(np.arange(n + 1), n - 1).astype(np.uint64), np.arange(1, n, dtype=np.uint32))
    tri, clus, info = eng.triangles_raw()
    assert info["oriented_entries"] == n - 2 > (n - 1) // 2 and info["oriented_max_degree"] == 1
    assert not tri.any() and not clus.any() and info["triangles"] == 0
    eng.close()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------
def test_errors(pkg):
    eng = pkg.Engine(0)
    eng.n = 4
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*no graph"):
        eng.triangles_raw()
    eng.close()
    A, r, _ = fixture_case(golden("er_n1000"))
    n = A.shape[0]
    small = engine_of(pkg, A, tri_state_bytes=4 * n)
    with pytest.raises(pkg.LzxError, match=r"\(-4\).*needs \d+ bytes"):
        small.triangles_raw()
    x = np.random.default_rng(3).standard_normal(n)
    y = small.spmv(x)
    plain = engine_of(pkg, A)
    assert np.array_equal(small.spmv(x), y) and np.array_equal(plain.spmv(x), y)
    plain.close()
    small.close()
    roomy = engine_of(pkg, A, tri_state_bytes=8 * (n + 1) + 2 * A.nnz + 28 * n + 65536)
    assert np.array_equal(roomy.triangles(), r["tri"])
    roomy.close()
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(A.indptr.astype(np.uint64), A.indices.astype(np.uint32))
    for e in grp.engines:
        with pytest.raises(pkg.LzxError, match=r"\(-3\).*communicator of 2"):
            e.triangles_raw()
    grp.close()
