"""CPU: the batched, independent Lanczos path (include/lzx.h: lzx_lanczos_multi_f64 and friends) without a GPU -- argument
errors of the four entry points, and the C++ class lanczosDecompMulti with cuda = false (host/lanczos_multi.h) against the
oracle: per column the recurrence of serial/ bit for bit, plus the breakdown stop that makes seed vectors e_v usable."""
import ctypes
import glob
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SO = os.path.join(ROOT, "msc-hpc-final-project_amd", "host", "libmschpc_host.so")
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))

_u32p = ctypes.POINTER(ctypes.c_uint32)
_f64p = ctypes.POINTER(ctypes.c_double)
LZX_ERR_ARG = -1


def p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def load_host(pkg):
    pkg.lib()  # liblzx.so first (RTLD_GLOBAL), then the host library that links it
    H = ctypes.CDLL(HOST_SO)
    H.host_last_error.restype = ctypes.c_char_p
    H.host_expm_multi_file.argtypes = [ctypes.c_char_p, ctypes.c_uint, ctypes.c_uint, _f64p, ctypes.c_int, _f64p, ctypes.c_uint,
                                       _f64p, _f64p, _u32p, _f64p]
    H.host_expm_multi_file.restype = ctypes.c_long
    return H


@pytest.fixture(scope="module")
def host(pkg):
    return load_host(pkg)


def write_pairs(path, n, pairs):
    with open(path, "w") as f:
        f.write(f"{n} {n} {len(pairs)}\n")
        np.savetxt(f, pairs, fmt="%d")


def run_multi(host, mtx, n, k, X, cuda=0):
    b = X.shape[0]
    X = np.ascontiguousarray(X, dtype=np.float64)
    ans, alpha, beta = np.zeros((b, n)), np.zeros((b, k)), np.zeros((b, k))
    ku, xn = np.zeros(b, dtype=np.uint32), np.zeros(b)
    rc = host.host_expm_multi_file(mtx.encode(), k, b, p(X, _f64p), cuda, p(ans, _f64p), ans.size, p(alpha, _f64p), p(beta, _f64p),
                                   p(ku, _u32p), p(xn, _f64p))
    assert rc == n, host.host_last_error()
    return ans, alpha, beta, ku, xn


def fixture_batch(g, n):
    """X = [the fixture's x, a seeded random vector, e_hub (the vertex of largest degree)]."""
    hub = int(np.argmax(np.diff(g["ref_row_offset"].astype(np.int64))))
    e = np.zeros(n)
    e[hub] = 1.0
    return np.stack([g["x"], np.random.default_rng(11).random(n) + 0.5, e])


def with_path(g, n, m=5):
    """The fixture's edges plus a disjoint path of m vertices n .. n + m - 1 (1-based pairs as the loader reads them)."""
    path = np.array([[n + i + 1, n + i + 2] for i in range(m - 1)], dtype=np.int64)
    return n + m, np.vstack([g["mtx_pairs"], path])


def test_entry_points_refuse_a_null_handle(pkg):
    L = pkg.lib()
    x = np.ones(8)
    a, bt, xn = np.zeros(64), np.zeros(64), np.zeros(4)
    ku = np.zeros(4, dtype=np.uint32)
    for b in (0, 1, 16, 17):
        calls = [("lzx_lanczos_multi_f64", lambda: L.lzx_lanczos_multi_f64(None, b, p(x, _f64p), 4, p(a, _f64p), p(bt, _f64p), p(ku, _u32p),
                                                                           p(xn, _f64p), None, None)),
                 ("lzx_multout_multi_f64", lambda: L.lzx_multout_multi_f64(None, b, p(a, _f64p), 4, p(x, _f64p))),
                 ("lzx_spmm_f64", lambda: L.lzx_spmm_f64(None, b, p(x, _f64p), p(a, _f64p))),
                 ("lzx_multi_release", lambda: L.lzx_multi_release(None))]
        for name, call in calls:
            assert call() == LZX_ERR_ARG, (name, b)
            msg = L.lzx_last_error().decode()
            assert name in msg and "handle" in msg and "(h)" in msg, (name, msg)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(q)[:-4] for q in GOLDEN])
def test_cpu_class_matches_oracle_per_column(host, oracle, tmp_path, path):
    O = oracle
    g = np.load(path)
    n, k = int(g["mtx_n"]), int(g["k"])
    mtx = str(tmp_path / "g.mtx")
    write_pairs(mtx, n, g["mtx_pairs"])
    rp = g["ref_row_offset"].astype(np.uint64)
    ci = g["ref_col_idx"]
    X = fixture_batch(g, n)
    ans, alpha, beta, ku, xn = run_multi(host, mtx, n, k, X)
    for c in range(X.shape[0]):
        a_ref, b_ref, _, xn_ref = O.lanczos(rp, ci, k, X[c], want_q=False)
        assert xn[c] == xn_ref
        kc = int(ku[c])
        assert 1 <= kc <= k
        # the recurrence is serial/'s operation for operation wherever the stop has not fired
        assert np.array_equal(alpha[c, :kc], a_ref[:kc]), (c, kc)
        assert np.array_equal(beta[c, :kc - 1], b_ref[:kc - 1]), (c, kc)
        assert not alpha[c, kc:].any() and not beta[c, kc - 1:].any()
        if kc == k:
            ref = O.expm_action(rp, ci, k, X[c])
            assert np.abs(ans[c] - ref).max() <= 1e-12 * np.abs(ref).max(), c
    assert ku[0] == k and ku[1] == k


def test_cpu_class_stops_on_an_exhausted_krylov_space(host, tmp_path):
    """A seed e_v in a disjoint 5-vertex path spans at most 5 Krylov vectors: its column stops with k_used <= 5 and its answer
    is e^P e_v of that component (scipy.linalg.expm), while the fixture's own column runs on."""
    from scipy.linalg import expm
    g = np.load(GOLDEN[0])
    n0 = int(g["mtx_n"])
    n, pairs = with_path(g, n0)
    mtx = str(tmp_path / "gp.mtx")
    write_pairs(mtx, n, pairs)
    k = 20
    P = np.diag(np.ones(4), 1) + np.diag(np.ones(4), -1)
    E = expm(P)
    X = np.zeros((4, n))
    X[0, :n0] = g["x"]
    for i, v in enumerate((0, 2, 4)):
        X[1 + i, n0 + v] = 1.0
    ans, alpha, beta, ku, xn = run_multi(host, mtx, n, k, X)
    assert ku[0] == k
    for i, v in enumerate((0, 2, 4)):
        c = 1 + i
        assert 1 <= ku[c] <= 5, ku
        want = np.zeros(n)
        want[n0:] = E[:, v]
        assert np.abs(ans[c] - want).max() <= 1e-12 * np.abs(want).max(), (v, ku[c])
    assert np.isfinite(ans).all()
