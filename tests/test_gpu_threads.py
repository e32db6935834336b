"""GPU: "a handle is bound to one GPU and is not thread-safe; distinct handles are" (include/lzx.h, conventions).  Four roles,
each with a handle of its own that is created and closed inside its thread, run library calls at the same time (ctypes.CDLL
releases the GIL around every call); every output must be the bits of the same role run alone -- all of these calls are
documented as deterministic.  A contract check with a fixed, small number of rounds, not a stress loop."""
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROUNDS = 3
JOIN_S = 60
K = 12
GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")


def _graph(O, name):
    if name == "er_odd_2001":
        return O.gen_er(2001, 14000, 5)
    g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return g["ref_row_offset"].astype(np.uint64), g["ref_col_idx"]


def _inputs(rp):
    n = len(rp) - 1
    rng = np.random.default_rng(2718)
    dmax = float(np.diff(rp.astype(np.int64)).max())
    return dict(x0=0.5 + rng.random(n), x=rng.random(n), t=rng.random(K), X=0.5 + rng.random((5, n)), T=rng.random((3, K)),
                b=rng.random(n), shifts=dmax + np.array([1.0, 2.5, 7.0]))     # sigma I - A is positive definite: lambda_max <= d_max


def role_lanczos(e, v):
    """(a) blocked SpMV: lanczos with the basis, multout, spmv"""
    a, b, Q, xn, _ = e.lanczos(v["x0"], K)
    return [a, b, Q, np.array([xn]), e.multout(v["t"]), e.spmv(v["x"])]


def role_batch(e, v):
    """(b) spmm with b = 5, lanczos_multi with b = 3, multout_multi"""
    Y = e.spmm(v["X"])
    a, b, ku, xn, _, _ = e.lanczos_multi(v["X"][:3], K)
    return [Y, a, b, ku, xn, e.multout_multi(v["T"])]


def role_structure(e, v):
    """(c) triangles, core numbers, components"""
    tri, clus, _ = e.triangles_raw()
    core, layer, _ = e.core_number_raw()
    labels, ci = e.components()
    return [tri, clus, core, layer, labels, np.array([ci["n_components"], ci["largest_size"]])]


def role_solvers(e, v):
    """(d) solve_shifted with three shifts, eigsh(nev = 2, m = 40)"""
    X, si = e.solve_shifted(v["b"], v["shifts"])
    w, V, _ = e.eigsh(nev=2, m=40, max_restarts=1000)
    return [X, si["iters"], si["resid"], w, V]


ROLES = {"a: lanczos / multout / spmv, blocked": (role_lanczos, dict(propagation_blocking=1, hub_entries=64)),
         "b: spmm / lanczos_multi / multout_multi": (role_batch, {}),
         "c: triangles / core_numbers / components": (role_structure, {}),
         "d: solve_shifted / eigsh": (role_solvers, {})}


def _play(pkg, graph, v, role, rounds, barrier=None):
    """One role on a handle of its own: create, hand the graph over, (wait for the others,) `rounds` rounds, close."""
    fn, options = ROLES[role]
    e = pkg.Engine(0, **options)
    try:
        e.set_graph_csr(*graph)
        if barrier is not None:
            barrier.wait(timeout=JOIN_S)
        return [fn(e, v) for _ in range(rounds)]
    finally:
        e.close()


def _concurrently(pkg, graph, v, roles):
    """The roles in one thread each, released together.  Exceptions are collected per thread and re-raised here with the role's
    name; a thread that is still alive after JOIN_S seconds fails the test."""
    barrier = threading.Barrier(len(roles))
    out, errors = {}, {}

    def body(i, role):
        try:
            out[i] = _play(pkg, graph, v, role, ROUNDS, barrier)
        except BaseException as e:
            errors[i] = e
            barrier.abort()          # nobody waits for a thread that will not come

    threads = [threading.Thread(target=body, args=(i, r), daemon=True, name=r) for i, r in enumerate(roles)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=JOIN_S)
    alive = [t.name for t in threads if t.is_alive()]
    assert not alive, f"still running after {JOIN_S} s: {alive}"
    first = sorted(errors.items(), key=lambda ie: isinstance(ie[1], threading.BrokenBarrierError))
    for i, e in first:
        raise AssertionError(f"role {roles[i]} (thread {i}): {e!r}") from e
    return [out[i] for i in range(len(roles))]


def _same(got, want, where):
    assert len(got) == len(want), where
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (where, "output", i)


@pytest.mark.parametrize("name", ["er_odd_2001", "rmat_n4096"])
def test_distinct_handles_on_concurrent_threads(pkg, oracle, name):
    graph = _graph(oracle, name)
    v = _inputs(graph[0])
    solo = {role: _play(pkg, graph, v, role, 1)[0] for role in ROLES}
    for role, outs in solo.items():
        assert all(np.isfinite(o).all() for o in outs if o.dtype.kind == "f"), role
    roles = list(ROLES)
    for i, rounds in enumerate(_concurrently(pkg, graph, v, roles)):
        for r, outs in enumerate(rounds):
            _same(outs, solo[roles[i]], (name, "four roles", roles[i], "round", r))
    same_role = [roles[0]] * 4
    for i, rounds in enumerate(_concurrently(pkg, graph, v, same_role)):
        for r, outs in enumerate(rounds):
            _same(outs, solo[roles[0]], (name, "four threads of role a", "thread", i, "round", r))
