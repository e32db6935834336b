"""CPU: the graph Laplacian operator (lanczosOptions::op, time) of the C++ class path, driven through host_capi.cc."""
import ctypes
import glob
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import expm_multiply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SO = os.path.join(ROOT, "msc-hpc-final-project_amd", "host", "libmschpc_host.so")
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))
IDS = [os.path.basename(q)[:-4] for q in GOLDEN]

_f64p = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def host(pkg):
    pkg.lib()  # liblzx.so first (RTLD_GLOBAL), then the host library that links it
    H = ctypes.CDLL(HOST_SO)
    H.host_last_error.restype = ctypes.c_char_p
    H.host_expm_operator_file.argtypes = [ctypes.c_char_p, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                          ctypes.c_uint, ctypes.c_int, _f64p, _f64p, ctypes.c_uint, _f64p, _f64p, _f64p]
    H.host_expm_operator_file.restype = ctypes.c_long
    H.host_expm_multi_operator_file.argtypes = [ctypes.c_char_p, ctypes.c_uint, ctypes.c_uint, _f64p, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_double, _f64p, ctypes.c_uint, _f64p, _f64p, ctypes.POINTER(ctypes.c_uint)]
    H.host_expm_multi_operator_file.restype = ctypes.c_long
    return H


def write_pairs(path, n, pairs):
    with open(path, "w") as f:
        f.write(f"{n} {n} {len(pairs)}\n")
        np.savetxt(f, pairs, fmt="%d")


def run(host, mtx, n, k, op, t, x0=None, arnoldi_every=0, want_q=False):
    ans, alpha, beta = np.zeros(n), np.zeros(k), np.zeros(max(k - 1, 1))
    Q = np.zeros((k, n)) if want_q else None
    x = None if x0 is None else np.ascontiguousarray(x0, dtype=np.float64)
    rc = host.host_expm_operator_file(mtx.encode(), k, 0, 0, op, t, arnoldi_every, 0,
                                      None if x is None else x.ctypes.data_as(_f64p), ans.ctypes.data_as(_f64p), n,
                                      alpha.ctypes.data_as(_f64p), beta.ctypes.data_as(_f64p),
                                      None if Q is None else Q.ctypes.data_as(_f64p))
    assert rc == n, host.host_last_error()
    return ans, alpha, beta[:k - 1], Q


def csr_of(g):
    rp, ci = g["ref_row_offset"].astype(np.int64), g["ref_col_idx"].astype(np.int64)
    n = len(rp) - 1
    A = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))
    d = np.diff(rp).astype(np.float64)
    return A, d


def rel_inf(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def fixture(tmp_path, path):
    g = np.load(path)
    n = int(g["mtx_n"])
    mtx = str(tmp_path / "graph.mtx")
    write_pairs(mtx, n, g["mtx_pairs"])
    A, d = csr_of(g)
    return g, n, mtx, A, d


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_heat_kernel_matches_scipy(host, tmp_path, path):
    g, n, mtx, A, d = fixture(tmp_path, path)
    L = sp.diags(d) - A
    t = 5.0 / (2.0 * d.max())   # t * 2 d_max = 5: converged far below 1e-10 at k = 30
    x = np.random.default_rng(7).standard_normal(n)
    y, alpha, beta, _ = run(host, mtx, n, 30, 1, t, x)
    ref = expm_multiply(-t * L, x)
    assert rel_inf(y, ref) <= 1e-10
    assert np.all(np.isfinite(alpha)) and np.all(alpha >= -1e-9) and np.all(alpha <= 2 * d.max() + 1e-9)   # Ritz range of L
    # mass is conserved: 1^T e^{-tL} x = 1^T x
    assert abs(y.sum() - x.sum()) <= 1e-10 * np.abs(x).sum()


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_adjacency_time_matches_scipy(host, tmp_path, path):
    g, n, mtx, A, d = fixture(tmp_path, path)
    t = 3.0 / d.max()
    x = np.random.default_rng(11).standard_normal(n)
    y, _, _, _ = run(host, mtx, n, 30, 0, t, x)
    assert rel_inf(y, expm_multiply(t * A, x)) <= 1e-10


def test_time_one_keeps_adjacency_bits(host, tmp_path):
    g, n, mtx, A, d = fixture(tmp_path, GOLDEN[0])
    H = host
    ans, alpha, beta = np.zeros(n), np.zeros(20), np.zeros(19)
    H.host_expm_file.argtypes = [ctypes.c_char_p, ctypes.c_uint, ctypes.c_int, ctypes.c_int, _f64p, ctypes.c_uint, _f64p, _f64p]
    H.host_expm_file.restype = ctypes.c_long
    assert H.host_expm_file(mtx.encode(), 20, 0, 0, ans.ctypes.data_as(_f64p), n, alpha.ctypes.data_as(_f64p),
                            beta.ctypes.data_as(_f64p)) == n
    y, a2, b2, _ = run(host, mtx, n, 20, 0, 1.0)
    assert np.array_equal(alpha, a2) and np.array_equal(beta, b2) and np.array_equal(ans, y)


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_ones_is_fixed_and_stop_fires(host, tmp_path, path):
    g, n, mtx, A, d = fixture(tmp_path, path)
    for t in (0.1, 1.0):
        y, alpha, beta, Q = run(host, mtx, n, 30, 1, t, want_q=True)
        assert np.abs(y - 1.0).max() <= 1e-12
        # the stop fires at j = 0: beta_0 and everything after it exactly 0
        assert beta[0] == 0.0 and np.all(beta == 0.0) and np.all(alpha[1:] == 0.0) and np.all(Q[1:] == 0.0)
        assert abs(alpha[0]) <= 64 * np.finfo(float).eps * d.max()


def test_regular_ring_no_nan(host, tmp_path):
    n = 64   # 4-regular ring: i ~ i +- 1, i +- 2
    pairs = np.array([(i, (i + s) % n) for i in range(n) for s in (1, 2)])
    mtx = str(tmp_path / "ring.mtx")
    write_pairs(mtx, n, pairs + 1)   # Matrix Market ids are 1-based
    A = sp.coo_matrix((np.ones(2 * len(pairs)), (np.r_[pairs[:, 0], pairs[:, 1]], np.r_[pairs[:, 1], pairs[:, 0]])), shape=(n, n)).tocsr()
    L = sp.diags(np.asarray(A.sum(axis=1)).ravel()) - A
    for x0 in (None, np.eye(n)[5], np.random.default_rng(3).standard_normal(n)):
        y, alpha, beta, Q = run(host, mtx, n, 40, 1, 0.5, x0, want_q=True)
        assert np.all(np.isfinite(y)) and np.all(np.isfinite(alpha)) and np.all(np.isfinite(beta)) and np.all(np.isfinite(Q))
        x = np.ones(n) if x0 is None else x0
        assert rel_inf(y, expm_multiply(-0.5 * L, x)) <= 1e-10
        assert abs(y.sum() - x.sum()) <= 1e-12 * max(1.0, np.abs(x).sum())


def test_arnoldi_form_applies_the_operator(host, tmp_path):
    g, n, mtx, A, d = fixture(tmp_path, GOLDEN[0])
    L = sp.diags(d) - A
    t = 5.0 / (2.0 * d.max())
    x = np.random.default_rng(5).standard_normal(n)
    y, _, _, _ = run(host, mtx, n, 30, 1, t, x, arnoldi_every=1)
    assert rel_inf(y, expm_multiply(-t * L, x)) <= 1e-10


@pytest.mark.parametrize("path", GOLDEN[:3], ids=IDS[:3])
def test_batched_class_heat_kernel(host, tmp_path, path):
    g, n, mtx, A, d = fixture(tmp_path, path)
    L = sp.diags(d) - A
    t = 5.0 / (2.0 * d.max())
    X = np.random.default_rng(9).standard_normal((4, n))
    X[1] = 1.0                       # the stop fires at j = 0
    X[2] = 0.0
    X[2, 3] = 1.0                    # a seed column e_v
    k, b = 30, len(X)
    ans, alpha, beta = np.zeros(b * n), np.zeros(b * k), np.zeros(b * k)
    ku = np.zeros(b, dtype=np.uint32)
    rc = host.host_expm_multi_operator_file(mtx.encode(), k, b, X.ctypes.data_as(_f64p), 0, 1, t, ans.ctypes.data_as(_f64p), b * n,
                                            alpha.ctypes.data_as(_f64p), beta.ctypes.data_as(_f64p),
                                            ku.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)))
    assert rc == n, host.host_last_error()
    Y = ans.reshape(b, n)
    assert ku[1] == 1 and np.abs(Y[1] - 1.0).max() <= 1e-12
    for c in range(b):
        assert rel_inf(Y[c], expm_multiply(-t * L, X[c])) <= 1e-10, c
    # time alone, under A
    rc = host.host_expm_multi_operator_file(mtx.encode(), k, b, X.ctypes.data_as(_f64p), 0, 0, 2.0 / d.max(), ans.ctypes.data_as(_f64p),
                                            b * n, None, None, None)
    assert rc == n, host.host_last_error()
    for c in range(b):
        assert rel_inf(ans.reshape(b, n)[c], expm_multiply((2.0 / d.max()) * A, X[c])) <= 1e-10, c
