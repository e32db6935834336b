"""GPU: connected components and induced subgraphs on the device (include/lzx.h: lzx_components, lzx_set_graph_induced;
Engine.components / induced / restrict / largest_component / component_indicators) against scipy on the golden fixtures and
four generated graphs: canonical labels and counts, the induced CSR against scipy's A[keep][:, keep] and against the CSR
hand-over bit for bit, what the calls leave alone, lambda_2 and L+ b on the giant component of the R-MAT fixtures, the error
paths, and BASELINE C2 at full size."""
import ctypes
import glob
import os

import numpy as np
import pytest
import scipy.sparse as sp

from bench import C2_DRAWS
from test_components_host import GENERATED, components_restatement, counts_of, fixture, graph, scipy_labels

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))
NAMES = [os.path.basename(p)[:-4] for p in GOLDEN] + list(GENERATED)
LAP = 1
COUNTS = ("n_components", "largest_size", "largest_label", "rounds")
TIMING = ("placement_tried", "placement_kept", "placement_us")


def matrices(rp, ci):
    rp64, ci64 = rp.astype(np.int64), ci.astype(np.int64)
    n = len(rp64) - 1
    A = sp.csr_matrix((np.ones(len(ci64)), ci64, rp64), shape=(n, n))
    return A, (sp.diags(np.diff(rp64).astype(np.float64)) - A).tocsr()


def induced_csr(rp, ci, keep):
    A, _ = matrices(rp, ci)
    S = A[keep][:, keep].tocsr()
    S.sort_indices()
    return S.indptr.astype(np.uint64), S.indices.astype(np.uint32)


def engine(pkg, rp, ci, **options):
    eng = pkg.Engine(0, **options)
    eng.set_graph_csr(rp, ci)
    return eng


def giant_mask(rp, ci):
    labels = scipy_labels(rp, ci)
    return labels == counts_of(labels)[2]


# ---- 1. labels and counts ----
@pytest.mark.parametrize("name", NAMES)
def test_labels_and_counts(pkg, name):
    rp, ci = graph(name)
    n = len(rp) - 1
    want = scipy_labels(rp, ci)
    nc, big, big_label = counts_of(want)
    expected = {"rmat_n3000_skew": (750, 2249), "rmat_n4096": (1204, 2890)}
    if name in expected:
        assert (nc, big) == expected[name]
    elif name in [os.path.basename(p)[:-4] for p in GOLDEN]:
        assert (nc, big) == (1, n)
    _, ref_rounds = components_restatement(rp, ci)
    eng = engine(pkg, rp, ci)
    labels, info = eng.components()
    print(f"{name}: rounds {info['rounds']} (restatement {ref_rounds}), sweep_ms {info['sweep_ms']:.4f}, loop_ms {info['loop_ms']:.4f}")
    assert labels.dtype == np.uint32 and np.array_equal(labels, want), name
    assert (info["n_components"], info["largest_size"], info["largest_label"]) == (nc, big, big_label), name
    assert info["rounds"] == ref_rounds, (name, info["rounds"], ref_rounds)      # (a sweep's result is a function of its input)
    none, info2 = eng.components(want_labels=False)
    assert none is None and all(info2[f] == info[f] for f in COUNTS), name
    labels3, info3 = eng.components()
    assert np.array_equal(labels3, labels) and all(info3[f] == info[f] for f in COUNTS), name
    eng.close()


# ---- 2. and 3. the induced subgraph against scipy and against the CSR hand-over ----
def masks():
    out = []
    for name in ("rmat_n3000_skew", "rmat_n4096"):
        rp, ci = fixture(name)
        out.append((name + "_giant", rp, ci, giant_mask(rp, ci)))
    rp, ci = fixture("er_n4000_deg20")
    out.append(("er_n4000_deg20_half", rp, ci, np.random.default_rng(21).random(len(rp) - 1) < 0.5))
    return out


@pytest.mark.parametrize("case", ["rmat_n3000_skew_giant", "rmat_n4096_giant", "er_n4000_deg20_half"])
def test_induced_against_scipy_and_the_csr_handover(pkg, case):
    _, rp, ci, keep = next(m for m in masks() if m[0] == case)
    rp_s, ci_s = induced_csr(rp, ci, keep)
    src = engine(pkg, rp, ci, placement_trials=0)
    sub, old = src.induced(keep, placement_trials=0)
    assert np.array_equal(old, np.flatnonzero(keep)) and old.dtype == np.uint32
    got_rp, got_ci = sub.get_graph_csr()
    assert np.array_equal(got_rp, rp_s) and np.array_equal(got_ci, ci_s), case
    ref = engine(pkg, rp_s, ci_s, placement_trials=0)

    def same_as_ref(e):
        gi, gr = e.info(), ref.info()
        assert {k: v for k, v in gi.items() if k not in TIMING} == {k: v for k, v in gr.items() if k not in TIMING}, case
        x = np.random.default_rng(3).standard_normal(ref.n)
        assert e.n == ref.n and np.array_equal(e.spmv(x), ref.spmv(x)), case
        a, b, _, xn, _ = e.lanczos(x, 20, want_q=False)
        a_r, b_r, _, xn_r, _ = ref.lanczos(x, 20, want_q=False)
        assert np.array_equal(a, a_r) and np.array_equal(b, b_r) and xn == xn_r, case

    same_as_ref(sub)
    old2 = src.restrict(keep)                           # in place: the same again
    assert np.array_equal(old2, old)
    r_rp, r_ci = src.get_graph_csr()
    assert np.array_equal(r_rp, rp_s) and np.array_equal(r_ci, ci_s), case
    same_as_ref(src)
    for e in (src, sub, ref):
        e.close()


def test_induced_single_vertex_is_the_csr_handover_of_it(pkg):
    """A degenerate subgraph: one vertex without an edge gets whatever lzx_set_graph_csr of that CSR gets."""
    rp, ci = fixture("rmat_n4096")
    labels = scipy_labels(rp, ci)
    lonely = int(np.flatnonzero(np.bincount(labels, minlength=len(labels)) == 1)[0])
    keep = np.zeros(len(labels), dtype=bool)
    keep[lonely] = True
    ref = pkg.Engine(0)
    rc_ref = ref.L.lzx_set_graph_csr(ref.h, 1, 0, np.zeros(2, dtype=np.uint64).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                     np.zeros(1, dtype=np.uint32).ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    src = engine(pkg, rp, ci)
    dst = pkg.Engine(0)
    old = np.zeros(1, dtype=np.uint32)
    rc = src.L.lzx_set_graph_induced(dst.h, src.h, keep.astype(np.uint8).ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                     old.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None)
    assert rc == rc_ref and old[0] == lonely
    if rc == 0:
        dst.n = ref.n = 1
        assert {k: v for k, v in dst.info().items() if k not in TIMING} == {k: v for k, v in ref.info().items() if k not in TIMING}
        (d_rp, d_ci), (r_rp, r_ci) = dst.get_graph_csr(), ref.get_graph_csr()
        assert np.array_equal(d_rp, r_rp) and np.array_equal(d_ci, r_ci) and len(d_ci) == 0
    for e in (src, dst, ref):
        e.close()


# ---- 4. state ----
def test_components_leave_a_chunked_decomposition_alone(pkg):
    rp, ci = fixture("er_n1000")
    x0 = np.random.default_rng(8).standard_normal(len(rp) - 1)
    eng = engine(pkg, rp, ci)
    a_ref, b_ref, Q_ref, _, _ = eng.lanczos(x0, 20)
    eng.lanczos_prepare(x0, 20)
    eng.lanczos_run_steps(7)
    labels, info = eng.components()
    assert info["n_components"] == 1 and not labels.any()
    assert eng.lanczos_progress() == (7, 20)
    eng.lanczos_run_steps(13)
    a, b, Q = eng.lanczos_fetch(20, want_q=True)
    assert np.array_equal(a, a_ref) and np.array_equal(b, b_ref) and np.array_equal(Q, Q_ref)
    eng.close()


def test_components_leave_the_resident_bases_alone(pkg):
    rp, ci = fixture("rmat_n3000_skew")
    n = len(rp) - 1
    rng = np.random.default_rng(9)
    x0, X0 = rng.standard_normal(n), rng.standard_normal((3, n))
    t, T = rng.standard_normal(12), rng.standard_normal((3, 12))
    eng = engine(pkg, rp, ci)
    eng.lanczos(x0, 12, want_q=False)
    eng.lanczos_multi(X0, 12)
    ans, ans_m = eng.multout(t), eng.multout_multi(T)
    eng.components()
    eng.components(want_labels=False)
    assert np.array_equal(eng.multout(t), ans) and np.array_equal(eng.multout_multi(T), ans_m)
    eng.close()


def test_induced_leaves_the_source_alone(pkg):
    rp, ci = fixture("rmat_n4096")
    x = np.random.default_rng(10).standard_normal(len(rp) - 1)
    eng = engine(pkg, rp, ci)
    y = eng.spmv(x)
    sub, old = eng.largest_component()
    assert sub.n == 2890 == len(old) and eng.n == len(rp) - 1
    assert np.array_equal(eng.spmv(x), y)
    src_rp, src_ci = eng.get_graph_csr()
    assert np.array_equal(src_rp, rp) and np.array_equal(src_ci, ci)
    sub.close()
    eng.close()


# ---- 5. the payoff ----
def test_lambda_2_of_the_giant_component(pkg):
    """|theta_i - lambda_i| <= resid_i + 1e-12 ||L||: the residual bounds the eigenvalue error of a symmetric matrix, the second
    term covers the dense solver's rounding.  lambda_2 .. lambda_4 of the component are 0.3817, 0.5808, 0.6905."""
    rp, ci = fixture("rmat_n3000_skew")
    eng = engine(pkg, rp, ci)
    sub, old = eng.largest_component(operator=LAP)
    keep = giant_mask(rp, ci)
    assert np.array_equal(old, np.flatnonzero(keep))
    _, Lg = matrices(*induced_csr(rp, ci, keep))
    lam = np.linalg.eigvalsh(Lg.toarray())
    assert abs(lam[0]) <= 1e-12 * lam[-1] and lam[1] > 0.3
    n1 = sub.n
    w, V, info = sub.eigsh(nev=3, which="SA", deflate=np.full(n1, 1.0 / np.sqrt(n1)), tol=1e-10)
    print("theta", w, "lambda", lam[1:4], "resid", info["resid"], "restarts", info["restarts"])
    assert info["converged"] == 3
    for i in range(3):
        assert abs(w[i] - lam[1 + i]) <= info["resid"][i] + 1e-12 * lam[-1], (i, w[i], lam[1 + i], info["resid"][i])
    sub.close()
    eng.close()


def test_pseudo_inverse_on_the_giant_component_and_with_indicators(pkg):
    rp, ci = fixture("rmat_n4096")
    n = len(rp) - 1
    tol = 1e-10
    eng = engine(pkg, rp, ci, operator=LAP)
    sub, old = eng.largest_component(operator=LAP)
    n1 = sub.n
    _, Lg = matrices(*induced_csr(rp, ci, giant_mask(rp, ci)))
    Ld = Lg.toarray()
    lam = np.linalg.eigvalsh(Ld)
    b = np.random.default_rng(12).standard_normal(n1)
    b -= b.mean()
    X, info = sub.solve_shifted(b, [0.0], tol=tol, maxiter=5000, W=np.full(n1, 1.0 / np.sqrt(n1)))
    ref = np.linalg.pinv(Ld) @ b
    kappa = lam[-1] / lam[1]
    err = np.linalg.norm(X[0] - ref)
    print("L+ b: err", err, "bound", kappa * 10 * tol * np.linalg.norm(ref), "iters", info["iters"], "resid", info["resid"])
    assert err <= kappa * 10 * tol * np.linalg.norm(ref)
    sub.close()
    # the whole graph: the indicators of the four components of more than one vertex span the null space b can see
    labels, _ = eng.components()
    roots, sizes = np.unique(labels, return_counts=True)
    assert np.count_nonzero(sizes > 1) == 4
    W = eng.component_indicators(labels, roots[sizes > 1])
    bw = np.random.default_rng(13).standard_normal(n)
    bw[np.isin(labels, roots[sizes == 1])] = 0.0      # nothing on the vertices without an edge: the rest of the null space
    Xw, info_w = eng.solve_shifted(bw, [0.0], tol=tol, maxiter=5000, W=W)
    print("whole graph: resid", info_w["resid"], "iters", info_w["iters"])
    assert info_w["converged"] == 1 and info_w["resid"][0] <= 10 * tol
    eng.close()


# ---- 6. errors ----
def test_errors(pkg):
    eng = pkg.Engine(0)
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*no graph"):
        eng.components()
    other = pkg.Engine(0)
    eng.n = 4
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*no graph"):
        eng._induce_into(other, np.ones(4, dtype=np.uint8), "lzx_set_graph_induced")
    other.close()
    rp, ci = fixture("er_n1000")
    n = len(rp) - 1
    eng.set_graph_csr(rp, ci)
    x = np.random.default_rng(14).standard_normal(n)
    y = eng.spmv(x)
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*keeps none"):
        eng.restrict(np.zeros(n, dtype=bool))
    assert eng.n == n and np.array_equal(eng.spmv(x), y)          # a failed restrict: the old graph, the old bits
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*keeps none"):
        eng.induced(np.zeros(n))
    for bad in (np.ones(n - 1), np.ones(n + 1), np.ones((n, 1))):
        with pytest.raises(ValueError, match="keep must have shape"):
            eng.restrict(bad)
        with pytest.raises(ValueError, match="keep must have shape"):
            eng.induced(bad)
    assert np.array_equal(eng.spmv(x), y)
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(rp, ci)
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*communicator of 2"):
        grp.engines[0].components()
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*communicator of 2"):
        grp.engines[0].restrict(np.ones(n))
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*communicator of 2"):
        eng._induce_into(grp.engines[1], np.ones(n, dtype=np.uint8), "lzx_set_graph_induced")
    grp.close()
    eng.close()


# ---- 7. full size ----
def test_c2_components_and_largest_component(pkg):
    eng = pkg.Engine(0)
    eng.gen_rmat(20, 1 << 20, C2_DRAWS, 1234)          # BASELINE C2, generated on the device
    rp, ci = eng.get_graph_csr()
    want = scipy_labels(rp, ci)
    nc, big, big_label = counts_of(want)
    labels, info = eng.components()
    print(f"C2: components {info['n_components']}, largest {info['largest_size']}, rounds {info['rounds']}, "
          f"sweep_ms {info['sweep_ms']:.3f}, loop_ms {info['loop_ms']:.3f}")
    assert np.array_equal(labels, want)
    assert (info["n_components"], info["largest_size"], info["largest_label"]) == (nc, big, big_label)
    sub, old = eng.largest_component()
    assert sub.info()["n"] == info["largest_size"] == len(old)
    assert np.array_equal(old, np.flatnonzero(want == big_label))
    _, info_sub = sub.components(want_labels=False)
    assert info_sub["n_components"] == 1 and info_sub["largest_size"] == big
    sub.close()
    eng.close()
