"""GPU: PageRank for several damping factors by multi-shift CG in the degree inner product (include/lzx.h: lzx_pagerank_f64,
Engine.pagerank) against a dense direct solve, the numpy restatement of the method (test_pagerank_host.pagerank_wcg) and
networkx.pagerank: the golden fixtures, a hand-made graph with self loops, two components and isolated vertices, a graph without
edges, the smallest shapes on either side of a wavefront / a workgroup / a two-doubles-per-lane stride, the multi-shift
behaviour, what the call leaves of the handle's state, every error path, and every blocked SpMV form.

Two bounds on ||x - x*||_1 against the dense solve x*:
  fixture bound   4 x the distance pagerank_wcg reaches for the same case, plus 1e-13, and never above 1e-10 (the model stays
                  below 5e-12 on the fixtures, so the cap hides nothing);
  stop-rule bound test_pagerank_host.error_bound -- what |zeta_s| ||r||_W <= tol ||b||_W guarantees in exact arithmetic,
                  2 tol sqrt(sum w * sum v^2 / w) / (1 - delta) -- plus 1e-13 of rounding, where no fixture is involved."""
import ctypes

import numpy as np
import pytest

from test_pagerank_host import DAMPINGS, FIXTURES, TOL, Case, error_bound, fixture_case, l1_residual, nx_pagerank, pagerank_wcg

pytestmark = pytest.mark.gpu

_f64p = ctypes.POINTER(ctypes.c_double)
CAP = 1e-10


def engine(pkg, case, **options):
    eng = pkg.Engine(0, **options)
    eng.set_graph_csr(case.rp, case.ci)
    return eng


def check_against_dense(case, vname, v, X, info, what, bound_of):
    """The assertions every converged three-damping call must meet; bound_of(s, delta) bounds ||x - x*||_1."""
    assert info["converged"] == len(DAMPINGS) and info["launched"] >= info["iterations"] == info["iters"].max(), (what, info)
    assert np.all(np.diff(info["iters"].astype(np.int64)) >= 0), (what, info["iters"])     # DAMPINGS ascends
    for s, delta in enumerate(DAMPINGS):
        x = X[s]
        assert np.all(np.isfinite(x)) and abs(x.sum() - 1.0) <= 1e-13, (what, delta, x.sum() - 1.0)
        assert x.min() >= -TOL, (what, delta, x.min())
        assert np.all(x[(case.d == 0) & (v == 0)] == 0.0), (what, delta)
        err = np.abs(x - case.dense(delta)[vname]).sum()
        bound = bound_of(s, delta)
        res = l1_residual(case.A, v, delta, x * info["mass"][s])
        print(what, delta, f"iters {info['iters'][s]} L1 error {err:.2e} bound {bound:.2e} resid {info['resid'][s]:.2e} (scipy {res:.2e})")
        assert err <= bound and err <= CAP, (what, delta, err, bound)
        assert abs(info["resid"][s] - res) <= 1e-12, (what, delta, info["resid"][s], res)


def fixture_bound(case, vname):
    Xm, _, conv, _ = case.model(vname)
    assert conv.all()
    return lambda s, delta: 4.0 * np.abs(Xm[s] - case.dense(delta)[vname]).sum() + 1e-13


def stop_rule_bound(case, v):
    return lambda s, delta: error_bound(case.A, v, delta, TOL) + 1e-13


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures(pkg, name):
    case = fixture_case(name)
    eng = engine(pkg, case)
    for vname, v in case.vs():
        X, info = eng.pagerank(DAMPINGS, personalization=None if vname == "uniform" else v, tol=TOL)
        check_against_dense(case, vname, v, X, info, (name, vname), fixture_bound(case, vname))
    eng.close()


@pytest.mark.parametrize("name", ["er_n1000", "rmat_n4096"])
def test_networkx(pkg, name):
    """1e-8 in L1 is networkx's own stopping error (tol = 1e-13 per vertex on the change between two power iterations)."""
    case = fixture_case(name)
    eng = engine(pkg, case)
    for vname in ("uniform", "random"):
        v = dict(case.vs())[vname]
        x = eng.pagerank(0.85, personalization=None if vname == "uniform" else v, tol=TOL)
        assert x.shape == (case.n,)
        ref = case.once(("nx", vname), lambda: nx_pagerank(case.A, None if vname == "uniform" else v, 0.85))
        err = np.abs(x - ref).sum()
        print(name, vname, f"L1 distance to networkx {err:.2e}")
        assert err <= 1e-8, (name, vname, err)
    eng.close()


def hand_made():
    """70 vertices: a ring of 40 with chords, a path of 25 with chords, five isolated vertices (65 .. 69); self loops at 3, 17, 50."""
    rng = np.random.default_rng(23)
    edges = {(i, (i + 1) % 40) for i in range(40)} | {(40 + i, 41 + i) for i in range(24)}
    edges |= {tuple(sorted(rng.choice(40, 2, replace=False))) for _ in range(25)}
    edges |= {tuple(sorted(40 + rng.choice(25, 2, replace=False))) for _ in range(10)}
    rows = [set() for _ in range(70)]
    for a, b in edges:
        rows[a].add(int(b))
        rows[b].add(int(a))
    for i in (3, 17, 50):
        rows[i].add(i)
    rp = np.cumsum([0] + [len(r) for r in rows])
    ci = np.array([c for r in rows for c in sorted(r)])
    n = 70
    lonely, two = np.zeros(n), np.zeros(n)
    lonely[67] = 1.0                   # an isolated vertex carrying all of v
    two[[5, 50, 66]] = [1.0, 2.0, 3.0]   # mass on both components and on an isolated vertex
    return Case("hand_made", rp, ci, vs=[("uniform", np.full(n, 1.0 / n)), ("random", np.random.default_rng(5).random(n)), ("lonely", lonely),
                                         ("two", two)])


def test_hand_made_graph(pkg):
    case = hand_made()
    assert (case.d == 0).sum() == 5 and case.A.diagonal().sum() == 3 and (case.A != case.A.T).nnz == 0
    eng = engine(pkg, case)
    for vname, v in case.vs():
        X, info = eng.pagerank(DAMPINGS, personalization=None if vname == "uniform" else v, tol=TOL)
        check_against_dense(case, vname, v, X, info, ("hand_made", vname), stop_rule_bound(case, v))
        if vname == "lonely":           # x = v
            assert np.array_equal(X, np.tile(v, (3, 1))) and list(info["iters"]) == [1, 1, 1]
    eng.close()


def test_graph_without_edges(pkg):
    n = 100
    case = Case("edgeless", np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    v = np.random.default_rng(2).random(n)
    eng = engine(pkg, case)
    X, info = eng.pagerank(DAMPINGS, personalization=v, tol=TOL)
    assert list(info["iters"]) == [1, 1, 1] and info["converged"] == 3
    assert np.abs(X - v / v.sum()).max() <= 4e-16 and np.abs(info["resid"]).max() <= 1e-14
    X, info = eng.pagerank(DAMPINGS, tol=TOL)
    assert list(info["iters"]) == [1, 1, 1] and np.abs(X - 1.0 / n).max() <= 1e-17
    eng.close()


def small_case(n):
    """n = 1: one vertex without an edge; otherwise the path 0 - 1 - ... - (n - 1); uniform v and v one-hot on vertex 0."""
    hot = np.zeros(n)
    hot[0] = 1.0
    rows = [[j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)]
    return Case(f"path{n}", np.cumsum([0] + [len(r) for r in rows]), np.array([c for r in rows for c in r], dtype=np.uint32),
                vs=[("uniform", np.full(n, 1.0 / n)), ("onehot", hot)])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 513])
def test_smallest_shapes(pkg, n):
    """n = 1, one edge, and paths with n odd and on either side of a wavefront (64), a workgroup (256) and one workgroup's
    two-doubles-per-lane stride (512)."""
    case = small_case(n)
    eng = engine(pkg, case)
    for vname, v in case.vs():
        X, info = eng.pagerank(DAMPINGS, personalization=None if vname == "uniform" else v, tol=TOL)
        check_against_dense(case, vname, v, X, info, (case.name, vname), stop_rule_bound(case, v))
    eng.close()


def test_multishift_behaviour(pkg):
    case = fixture_case("rmat_n3000_skew")
    v = dict(case.vs())["random"]
    eng = engine(pkg, case)
    X, info = eng.pagerank(DAMPINGS, personalization=v, tol=TOL)
    for s, delta in enumerate(DAMPINGS):
        x1 = eng.pagerank(float(delta), personalization=v, tol=TOL)
        assert np.abs(x1 - X[s]).max() <= 10 * TOL, (delta, np.abs(x1 - X[s]).max())
    X2, info2 = eng.pagerank(DAMPINGS, personalization=v, tol=TOL)
    for f in ("iters", "resid", "mass"):
        assert np.array_equal(info[f], info2[f]), f
    assert np.array_equal(X, X2)
    perm = [2, 0, 1, 2, 0]                               # a permutation, with duplicates
    Xp, infop = eng.pagerank(DAMPINGS[perm], personalization=v, tol=TOL)
    assert infop["converged"] == 5
    for i, s in enumerate(perm):
        assert np.array_equal(Xp[i], X[s]) and infop["iters"][i] == info["iters"][s] and infop["mass"][i] == info["mass"][s], i
    eng.set_option("operator", 1)                        # the operator option is ignored
    Xl, infol = eng.pagerank(DAMPINGS, personalization=v, tol=TOL)
    assert np.array_equal(Xl, X) and np.array_equal(infol["resid"], info["resid"]) and np.array_equal(infol["iters"], info["iters"])
    eng.close()
    e1 = engine(pkg, case, solve_poll=1)                 # the results do not depend on the status period
    X1, info1 = e1.pagerank(DAMPINGS, personalization=v, tol=TOL)
    e1.close()
    assert np.array_equal(X1, X) and np.array_equal(info1["iters"], info["iters"])
    assert info1["launched"] == info1["iterations"] <= info["launched"]


def test_state_left_alone(pkg):
    case = fixture_case("er_n1000")
    n, k = case.n, 20
    eng = engine(pkg, case)
    eng.lanczos_multi(np.stack([np.ones(n), np.arange(n, dtype=np.float64) + 1.0]), k)
    T = np.random.default_rng(1).standard_normal((2, k))
    y_multi = eng.multout_multi(T)
    eng.lanczos(np.ones(n), k, want_q=False)
    t = np.random.default_rng(2).standard_normal(k)
    y_single = eng.multout(t)
    X, info = eng.pagerank(DAMPINGS)
    assert info["converged"] == 3
    assert np.array_equal(eng.multout_multi(T), y_multi) and np.array_equal(eng.multout(t), y_single)
    eng.lanczos_prepare(np.ones(n), k)
    eng.lanczos_run_steps(5)
    eng.pagerank(0.85)
    with pytest.raises(pkg.LzxError, match=r"\(-3\)"):
        eng.lanczos_run_steps(5)                         # the prepared decomposition is void
    assert np.array_equal(eng.multout_multi(T), y_multi)
    eng.close()


def raw_call(L, h, n, null_damping=False, null_X=False):
    """lzx_pagerank_f64 itself with one damping and uniform v: the pointers Engine.pagerank never leaves null."""
    dm = np.array([0.85])
    X = np.zeros(n)
    return L.lzx_pagerank_f64(h, None, 1, None if null_damping else dm.ctypes.data_as(_f64p), 1e-10, 100, None if null_X else X.ctypes.data_as(_f64p),
                              None, None, None)


def test_error_paths(pkg):
    case = fixture_case("er_n1000")
    n = case.n
    eng = engine(pkg, case)
    bad_v = [np.where(np.arange(n) == 7, -1e-300, 1.0), np.where(np.arange(n) == 7, np.nan, 1.0), np.where(np.arange(n) == 7, np.inf, 1.0)]
    for v in bad_v:
        with pytest.raises(pkg.LzxError, match=r"\(-1\).*v\[7\].*negative or not finite"):
            eng.pagerank(0.85, personalization=v)
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*sums to 0"):
        eng.pagerank(0.85, personalization=np.zeros(n))
    for alpha in (1.0, 0.0, -0.1, float("nan"), float("inf"), [0.5, 1.5]):
        with pytest.raises(pkg.LzxError, match=r"\(-1\).*not in \(0, 1\)"):
            eng.pagerank(alpha)
    for kw, word in ((dict(tol=0.0), "tol"), (dict(tol=float("nan")), "tol"), (dict(maxiter=0), "maxiter")):
        with pytest.raises(pkg.LzxError, match=r"\(-1\).*" + word):
            eng.pagerank(0.85, **kw)
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*nd == 0"):
        eng.pagerank([])
    with pytest.raises(pkg.LzxError, match=r"\(-6\).*nd = 17"):
        eng.pagerank(np.linspace(0.1, 0.9, 17))
    assert eng.pagerank(np.linspace(0.1, 0.9, 16))[1]["converged"] == 16
    assert raw_call(eng.L, eng.h, n, null_damping=True) == -1 and b"null damping" in eng.L.lzx_last_error()
    assert raw_call(eng.L, eng.h, n, null_X=True) == -1 and b"null X" in eng.L.lzx_last_error()
    assert raw_call(eng.L, None, n) == -1 and b"null handle" in eng.L.lzx_last_error()
    # maxiter runs out: LZX_ERR_LIMIT, and what one iteration gives is written and normalised
    with pytest.raises(pkg.LzxError, match=r"\(-6\).*0 of 3 damping factors converged") as ei:
        eng.pagerank(DAMPINGS, maxiter=1)
    X, info = ei.value.partial
    assert list(info["iters"]) == [1, 1, 1] and info["launched"] == 1 and info["converged"] == 0
    assert np.abs(X.sum(axis=1) - 1.0).max() <= 1e-13 and X.min() >= 0.0
    Xm, _, conv, Ym = pagerank_wcg(case.A, None, DAMPINGS, 1e-10, 1)     # the numpy restatement after one iteration
    assert not conv.any() and np.abs(X - Xm).sum(axis=1).max() <= 1e-13
    for s, delta in enumerate(DAMPINGS):
        res = l1_residual(case.A, np.full(n, 1.0 / n), delta, X[s] * info["mass"][s])
        assert abs(info["resid"][s] - res) <= 1e-12, (delta, info["resid"][s], res)
    eng.close()
    # no graph; a state that does not fit; a handle of an in-process group
    eng = pkg.Engine(0)
    assert raw_call(eng.L, eng.h, 8) == -3 and b"no graph" in eng.L.lzx_last_error()
    eng.close()
    eng = engine(pkg, case, solve_state_bytes=5 * 1100 * 8)      # 5 vectors of about n_loc_pad + tail doubles
    with pytest.raises(pkg.LzxError, match=r"\(-4\).*bytes"):
        eng.pagerank([0.5, 0.85])                                 # 2 + 2 * 2 = 6 vectors of ldq > 1100 doubles
    assert np.abs(eng.pagerank(0.85).sum() - 1.0) <= 1e-13        # 4 vectors fit
    eng.close()
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(case.rp, case.ci)
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*one GPU"):
        grp.engines[0].pagerank(0.85)
    grp.close()


def test_blocked_forms(pkg, oracle):
    """The three-damping call through every blocked SpMV form of test_gpu_parity.MODES on test_gpu_forms' graphs, only where the
    blocked passes engage: p . A p comes from the launch's fused partials and A p must be complete over n_loc_pad rows.  Against
    pagerank_wcg: where a dense solve is possible (n <= 4096) the fixture bound as it stands; above, the model's own error is
    bounded by its scipy L1 residual, ||x - x*||_1 <= 2 ||res||_1 / (1 - delta), and the distance to the model must stay within
    4 x that bound plus 1e-13 and below 1e-10; the library's reported residual agrees with scipy's to 1e-12 either way."""
    from test_gpu_forms import graph, run_pairs

    def body(i, mode, g, eng):
        case = g.once("pagerank_case", lambda: Case(g.name, g.rp, g.ci))
        for vname, v in case.vs():
            what = (g.name, i, vname)
            X, info = eng.pagerank(DAMPINGS, personalization=None if vname == "uniform" else v, tol=TOL)
            if case.n <= 4096:
                check_against_dense(case, vname, v, X, info, what, fixture_bound(case, vname))
                continue
            Xm, itm, conv, Ym = case.model(vname)
            assert conv.all() and info["converged"] == 3 and np.all(np.diff(info["iters"].astype(np.int64)) >= 0), (what, info)
            for s, delta in enumerate(DAMPINGS):
                model_err = 2.0 * l1_residual(case.A, v, delta, Ym[s]) / (1.0 - delta)
                dist = np.abs(X[s] - Xm[s]).sum()
                res = l1_residual(case.A, v, delta, X[s] * info["mass"][s])
                print(what, delta, f"iters {info['iters'][s]} (model {itm[s]}) L1 to model {dist:.2e} model bound {model_err:.2e} resid {info['resid'][s]:.2e}")
                assert dist <= 4.0 * model_err + 1e-13 and dist <= CAP, (what, delta, dist, model_err)
                assert abs(X[s].sum() - 1.0) <= 1e-13 and X[s].min() >= -TOL, (what, delta)
                assert np.all(X[s][(case.d == 0) & (v == 0)] == 0.0), (what, delta)
                assert abs(info["resid"][s] - res) <= 1e-12, (what, delta, info["resid"][s], res)
    run_pairs(pkg, oracle, "pagerank", body)
