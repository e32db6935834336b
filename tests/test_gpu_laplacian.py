"""GPU: the graph Laplacian operator (option "operator" = LZX_OP_LAPLACIAN): kernel-level parity of L x (SpMV and batched
SpMM), bit-identical reference_order against the C++ class path, the production forms (plain, blocked lazy, 8 in-process
ranks, batched) against it at 1e-10, the breakdown stop, the heat kernel's closed-form properties, and the `final` CLI."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from bench import C2_DRAWS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "msc-hpc-final-project_amd", "host")
HOST_SO = os.path.join(HOST_DIR, "libmschpc_host.so")
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))
IDS = [os.path.basename(q)[:-4] for q in GOLDEN]
LAP = 1
_f64p = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def host(pkg):
    pkg.lib()
    H = ctypes.CDLL(HOST_SO)
    H.host_last_error.restype = ctypes.c_char_p
    H.host_expm_operator_file.argtypes = [ctypes.c_char_p, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                          ctypes.c_uint, ctypes.c_int, _f64p, _f64p, ctypes.c_uint, _f64p, _f64p, _f64p]
    H.host_expm_operator_file.restype = ctypes.c_long
    return H


def write_pairs(path, n, pairs):
    with open(path, "w") as f:
        f.write(f"{n} {n} {len(pairs)}\n")
        np.savetxt(f, pairs, fmt="%d")


def host_run(host, mtx, n, k, t, x0, cuda=0, reference_order=0, arnoldi_every=0, op=LAP):
    ans, alpha, beta, Q = np.zeros(n), np.zeros(k), np.zeros(max(k - 1, 1)), np.zeros((k, n))
    x = np.ascontiguousarray(x0, dtype=np.float64)
    rc = host.host_expm_operator_file(mtx.encode(), k, cuda, 0, op, t, arnoldi_every, reference_order, x.ctypes.data_as(_f64p),
                                      ans.ctypes.data_as(_f64p), n, alpha.ctypes.data_as(_f64p), beta.ctypes.data_as(_f64p),
                                      Q.ctypes.data_as(_f64p))
    assert rc == n, host.host_last_error()
    return ans, alpha, beta[:k - 1], Q


def lap_of(rp, ci):
    rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    n = len(rp) - 1
    A = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))
    d = np.diff(rp).astype(np.float64)
    return A, d


def rel_inf(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def load(tmp_path, path):
    g = np.load(path)
    n = int(g["mtx_n"])
    mtx = str(tmp_path / "graph.mtx")
    write_pairs(mtx, n, g["mtx_pairs"])
    rp, ci = g["ref_row_offset"], g["ref_col_idx"]
    return n, mtx, rp, ci


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_reference_order_bit_identical(host, tmp_path, path):
    n, mtx, rp, ci = load(tmp_path, path)
    A, d = lap_of(rp, ci)
    t = 5.0 / (2.0 * d.max())
    for x0 in (np.random.default_rng(1).standard_normal(n), np.ones(n)):
        for every in (0, 1):
            y_c, a_c, b_c, Q_c = host_run(host, mtx, n, 30, t, x0, cuda=0, arnoldi_every=every)
            y_g, a_g, b_g, Q_g = host_run(host, mtx, n, 30, t, x0, cuda=1, reference_order=1, arnoldi_every=every)
            assert np.array_equal(a_c, a_g) and np.array_equal(b_c, b_g) and np.array_equal(Q_c, Q_g), (every, x0[0])
            assert rel_inf(y_g, y_c) <= 1e-13


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
@pytest.mark.parametrize("pb", [0, 1], ids=["plain", "blocked_lazy"])
def test_production_forms_match_cpu(pkg, host, tmp_path, path, pb):
    n, mtx, rp, ci = load(tmp_path, path)
    A, d = lap_of(rp, ci)
    t = 5.0 / (2.0 * d.max())
    x0 = np.random.default_rng(2).standard_normal(n)
    y_c, a_c, b_c, _ = host_run(host, mtx, n, 30, t, x0)
    # (hub_entries=64: propagation_blocking=1 alone stages min(16384, n) columns and leaves nothing to block on graphs this small)
    eng = pkg.Engine(0, propagation_blocking=pb, operator=LAP, **(dict(hub_entries=64) if pb else {}))
    try:
        eng.set_graph_csr(rp, ci)
        assert (eng.info()["pb_entries"] > 0) == (pb == 1)
        assert rel_inf(eng.expm_multiply(x0, 30, t), y_c) <= 1e-10
        a, b, Q, xn, _ = eng.lanczos(x0, 30)
        assert abs(a[0] - a_c[0]) <= 1e-12 * abs(a_c[0]) and abs(b[0] - b_c[0]) <= 1e-12 * abs(b_c[0])
        assert abs(a[1] - a_c[1]) <= 1e-10 * max(abs(a_c[1]), abs(a_c[0]))
        # the recurrence with L on every column: L q_j = beta_{j-1} q_{j-1} + alpha_j q_j + beta_j q_{j+1}
        L = sp.diags(d) - A
        scale = max(np.abs(a).max(), np.abs(b).max())
        for j in range(len(a) - 1):
            r = L @ Q[j] - a[j] * Q[j] - b[j] * Q[j + 1] - (b[j - 1] * Q[j - 1] if j else 0.0)
            assert np.abs(r).max() <= 1e-12 * scale, j
        # x = ones: fixed by the heat kernel, the stop fires at j = 0
        assert np.abs(eng.expm_multiply(np.ones(n), 30, 1.0) - 1.0).max() <= 1e-12
        a1, b1, Q1, _, _ = eng.lanczos(np.ones(n), 30)
        assert np.all(b1 == 0.0) and np.all(a1[1:] == 0.0) and np.all(Q1[1:] == 0.0)
    finally:
        eng.close()


@pytest.mark.parametrize("pb", [0, 1], ids=["plain", "blocked"])
def test_spmv_is_exact_laplacian(pkg, oracle, pb):
    rp, ci = oracle.gen_rmat(14, 12000, 200000, 7)   # skewed, split rows
    A, d = lap_of(rp, ci)
    n = len(rp) - 1
    x = np.random.default_rng(3).integers(-50, 50, n).astype(np.float64)   # integer-valued: every sum exact
    ref = d * x - A @ x
    eng = pkg.Engine(0, propagation_blocking=pb, **(dict(hub_entries=64) if pb else {}))   # (n = 12000 < 16384: see above)
    try:
        eng.set_graph_csr(rp, ci)
        assert (eng.info()["pb_entries"] > 0) == (pb == 1)
        y_a = eng.spmv(x)
        assert np.array_equal(y_a, A @ x)
        eng.set_option("operator", LAP)
        assert np.array_equal(eng.spmv(x), ref)
        eng.set_option("operator", 0)
        assert np.array_equal(eng.spmv(x), y_a)
    finally:
        eng.close()


def test_c2_heat_kernel(pkg, oracle):
    """BASELINE C2 at k = 50: t chosen so that the k = 40 and k = 50 answers agree below 1e-12 (the approximation has
    converged); plain and blocked forms within 1e-10 of each other and of the host-side Lanczos in numpy."""
    rp, ci = oracle.gen_rmat(20, 1 << 20, C2_DRAWS, 1234)
    A, d = lap_of(rp, ci)
    n = len(rp) - 1
    t = 2.0 / (2.0 * d.max())
    x0 = np.random.default_rng(4).standard_normal(n)
    ys = {}
    for pb in (0, 1):
        eng = pkg.Engine(0, propagation_blocking=pb, operator=LAP)
        try:
            eng.set_graph_csr(rp, ci)
            y50 = eng.expm_multiply(x0, 50, t)
            y40 = eng.expm_multiply(x0, 40, t)
            assert rel_inf(y40, y50) <= 1e-12, pb
            assert abs(y50.sum() - x0.sum()) <= 1e-12 * np.abs(x0).sum(), pb
            assert np.abs(eng.expm_multiply(np.ones(n), 50, 1.0) - 1.0).max() <= 1e-12, pb
            ys[pb] = y50
            if pb:   # the batched form: ones come back, and column 0 is the single-vector answer
                a, b, ku, xn, _, _ = eng.lanczos_multi(np.vstack([x0, np.ones(n)]), 50)
                T = np.vstack([pkg._expm_coefficients(a[c], b[c][:49], xn[c], -t) for c in range(2)])
                Y = eng.multout_multi(T)
                assert rel_inf(Y[0], y50) <= 1e-10 and np.abs(Y[1] - 1.0).max() <= 1e-12
        finally:
            eng.close()
    assert rel_inf(ys[0], ys[1]) <= 1e-10
    # host-side Lanczos (numpy) on L: the same converged answer
    L = (sp.diags(d) - A).tocsr()
    k = 50
    q, qp, bp = x0 / np.linalg.norm(x0), np.zeros(n), 0.0
    al, be, Qs = [], [], []
    for j in range(k):
        Qs.append(q)
        v = L @ q - bp * qp
        a = v @ q
        v -= a * q
        for qq in Qs:   # full re-orthogonalisation: the numpy side is the accurate one
            v -= (v @ qq) * qq
        al.append(a)
        bp = np.linalg.norm(v)
        be.append(bp)
        qp, q = q, v / bp
    T = np.diag(al) + np.diag(be[:-1], 1) + np.diag(be[:-1], -1)
    lam, V = np.linalg.eigh(T)
    y_ref = np.array(Qs).T @ (V @ (np.exp(-t * lam) * (np.linalg.norm(x0) * V[0, :])))
    assert rel_inf(ys[1], y_ref) <= 1e-10


def test_default_operator_is_unchanged(pkg):
    g = np.load(GOLDEN[0])
    rp, ci = g["ref_row_offset"], g["ref_col_idx"]
    n = len(rp) - 1
    x0 = np.random.default_rng(5).standard_normal(n)
    out = []
    for opts, flip in (({}, False), ({"operator": 0}, False), ({}, True)):
        eng = pkg.Engine(0, propagation_blocking=1, hub_entries=64, **opts)
        try:
            eng.set_graph_csr(rp, ci)
            assert eng.info()["pb_entries"] > 0
            if flip:   # L, then back to A on the same graph
                eng.lanczos(x0, 20, want_q=False)
                eng.set_option("operator", LAP)
                eng.lanczos(x0, 20, want_q=False)
                eng.set_option("operator", 0)
            a, b, _, _, _ = eng.lanczos(x0, 20, want_q=False)
            out.append((a, b))
        finally:
            eng.close()
    for a, b in out[1:]:
        assert np.array_equal(a, out[0][0]) and np.array_equal(b, out[0][1])


def test_ranks_lazy_and_refusals(pkg, host, tmp_path):
    n, mtx, rp, ci = load(tmp_path, GOLDEN[0])
    A, d = lap_of(rp, ci)
    t = 5.0 / (2.0 * d.max())
    x0 = np.random.default_rng(6).standard_normal(n)
    y_c, _, _, _ = host_run(host, mtx, n, 30, t, x0)
    eng = pkg.Engine(0)
    try:
        with pytest.raises(pkg.LzxError, match="operator must be"):
            eng.set_option("operator", 2)
        eng.set_graph_csr(rp, ci)
        eng.set_option("operator", LAP)
        eng.set_option("basis_fp32", 1)   # the unnormalised basis it stores has nothing to divide by after a stop
        with pytest.raises(pkg.LzxError, match="basis_fp32"):
            eng.lanczos(x0, 10)
    finally:
        eng.close()
    # the lazy loop forced on one rank
    eng = pkg.Engine(0, lazy_normalisation=1, operator=LAP)
    try:
        eng.set_graph_csr(rp, ci)
        assert rel_inf(eng.expm_multiply(x0, 30, t), y_c) <= 1e-10
        assert np.abs(eng.expm_multiply(np.ones(n), 30, 1.0) - 1.0).max() <= 1e-12
    finally:
        eng.close()
    # 8 in-process ranks on the one GPU (lazy loop, and the non-lazy several-rank form) against one rank
    for lazy in (1, 0):
        grp = pkg.LocalGroup([0] * 8, operator=LAP, lazy_normalisation=lazy)
        try:
            grp.set_graph_csr(rp, ci)
            assert rel_inf(grp.expm_multiply(x0, 30, t), y_c) <= 1e-10, lazy
            assert np.array_equal(grp.spmv(np.round(x0 * 8)), d * np.round(x0 * 8) - A @ np.round(x0 * 8))
            assert np.abs(grp.expm_multiply(np.ones(n), 30, 1.0) - 1.0).max() <= 1e-12, lazy
        finally:
            grp.close()


def test_batched_laplacian(pkg, oracle):
    rp, ci = oracle.gen_rmat(14, 12000, 200000, 7)   # skewed, split rows
    A, d = lap_of(rp, ci)
    n = len(rp) - 1
    t = 5.0 / (2.0 * d.max())
    rng = np.random.default_rng(8)
    eng = pkg.Engine(0, operator=LAP, multi_row_chunk=64)   # many split rows: the chunk totals before the epilogue
    try:
        eng.set_graph_csr(rp, ci)
        X = rng.integers(-30, 30, (16, n)).astype(np.float64)
        assert np.array_equal(eng.spmm(X), (d[:, None] * X.T - A @ X.T).T)
        X = rng.standard_normal((16, n))
        X[3] = 0.0
        X[3, 17] = 1.0                                 # a seed column e_v
        X[5] = 1.0                                     # ones: the stop fires at j = 0
        k = 30
        alpha, beta, k_used, xn, Q, _ = eng.lanczos_multi(X, k)
        # answers of every column from the resident batch basis
        T = np.zeros((16, k))
        for c in range(16):
            T[c] = pkg._expm_coefficients(alpha[c], beta[c][:k - 1], xn[c], -t)
        Y = eng.multout_multi(T)
        assert k_used[5] == 1 and np.all(beta[5] == 0.0)
        assert np.abs(Y[5] - 1.0).max() <= 1e-12
        for c in range(16):
            y1 = eng.expm_multiply(X[c], k, t)
            assert rel_inf(Y[c], y1) <= 1e-10, c
        assert abs(Y[0].sum() - X[0].sum()) <= 1e-12 * np.abs(X[0]).sum()
        # a column's results do not depend on what else is in the batch
        a2, b2, ku2, xn2, _, _ = eng.lanczos_multi(np.vstack([X[7], X[3]]), k)
        assert np.array_equal(a2[0], alpha[7]) and np.array_equal(b2[0], beta[7]) and np.array_equal(a2[1], alpha[3])
    finally:
        eng.close()


def test_final_cli_laplacian(host, tmp_path):
    n, mtx, rp, ci = load(tmp_path, GOLDEN[0])
    env = dict(os.environ, FINAL_OPERATOR="laplacian", FINAL_TIME="0.25")
    out = subprocess.run([os.path.join(HOST_DIR, "final"), "-f", mtx, "-k", "20"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    rel = [l for l in out.stdout.splitlines() if l.startswith("Relative inf-norm")]
    assert rel and float(rel[0].split("=")[1]) <= 1e-10
    ans = np.loadtxt(mtx + ".ans20.txt")
    y_c, _, _, _ = host_run(host, mtx, n, 20, 0.25, np.ones(n))
    assert np.abs(ans - y_c).max() <= 1e-5 * np.abs(y_c).max()    # file holds 6 significant digits
    bad = subprocess.run([os.path.join(HOST_DIR, "final"), "-f", mtx, "-k", "20"], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, FINAL_OPERATOR="normalised"))
    assert bad.returncode != 0
