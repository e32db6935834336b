"""GPU: batched, independent Lanczos (include/lzx.h: lzx_lanczos_multi_f64, lzx_multout_multi_f64, lzx_spmm_f64,
lzx_multi_release) against the CPU oracle, column by column, with the tolerances of tests/test_gpu_parity.py -- plus what
only the batched path has: the answer of a column does not depend on the columns beside it (bit for bit), and a column
whose Krylov space is exhausted stops on its own."""
import glob
import os

import numpy as np
import pytest

from bench import C2_DRAWS
from test_gpu_parity import REL_INF_TOL, check_leading_coefficients, check_recurrence, rel_inf, shift_weights
from test_multi_host import fixture_batch, load_host, run_multi, with_path, write_pairs

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))


def fixtures():
    for path in GOLDEN:
        g = np.load(path)
        yield os.path.basename(path)[:-4], g, g["ref_row_offset"].astype(np.uint64), g["ref_col_idx"]


def weights(O, a, b, ku, xn):
    """T[c] = shift_weights of column c's own k_used x k_used block, zero behind it."""
    T = np.zeros(a.shape)
    for c in range(a.shape[0]):
        kc = int(ku[c])
        T[c, :kc] = shift_weights(O, a[c, :kc], b[c, :kc - 1], xn[c])
    return T


def c2(pkg):
    eng = pkg.Engine(0)
    eng.gen_rmat(20, 1 << 20, C2_DRAWS, 1234)          # BASELINE C2, generated on the device
    rp, ci = eng.get_graph_csr()
    return eng, rp, ci


def test_spmm_parity(pkg, oracle):
    O = oracle
    rng = np.random.default_rng(5)
    for name, g, rp, ci in fixtures():
        n = len(rp) - 1
        eng = pkg.Engine(0)
        eng.set_graph_csr(rp, ci)
        split = pkg.Engine(0, multi_row_chunk=64)       # every row above 64 entries cut into chunks
        split.set_graph_csr(rp, ci)
        for b in (1, 3, 8, 16):
            X = rng.random((b, n)) - 0.25
            Y = eng.spmm(X)
            Ys = split.spmm(X)
            assert np.array_equal(Ys, split.spmm(X)), (name, b)
            for c in range(b):
                ref = O.spmv(rp, ci, X[c])
                assert np.array_equal(Y[c], ref), (name, b, c)
                assert (np.abs(Ys[c] - ref) <= 1e-13 * O.spmv(rp, ci, np.abs(X[c]))).all(), (name, b, c)
        eng.close()
        split.close()
    eng, rp, ci = c2(pkg)                               # rows above 2 048 entries: the default chunks
    X = rng.random((4, len(rp) - 1))
    Y = eng.spmm(X)
    for c in range(4):
        assert (np.abs(Y[c] - O.spmv(rp, ci, X[c])) <= 1e-13 * O.spmv(rp, ci, X[c])).all(), c
    eng.close()


def test_centrality_parity(pkg, oracle):
    O = oracle
    for name, g, rp, ci in fixtures():
        n, k = len(rp) - 1, int(g["k"])
        X = fixture_batch(g, n)
        eng = pkg.Engine(0)
        eng.set_graph_csr(rp, ci)
        a, b, ku, xn, _, st = eng.lanczos_multi(X, k)
        assert st["iters"] == k and st["spmv_kernels"] <= 4
        assert st["spmv_bytes"] == 4 * len(ci) + 8 * (n + 1) + 16 * 3 * n
        ans = eng.multout_multi(weights(O, a, b, ku, xn))
        for c in range(3):
            a_ref, b_ref, Q_ref, xn_ref = O.lanczos(rp, ci, k, X[c], q_colmajor=True)
            assert xn[c] == xn_ref, (name, c)
            check_leading_coefficients(a[c], b[c, :k - 1], a_ref, b_ref, (name, c))
            if ku[c] == k:
                ref = shift_weights(O, a_ref, b_ref, xn_ref) @ Q_ref
                assert rel_inf(ans[c], ref) <= REL_INF_TOL, (name, c, rel_inf(ans[c], ref))
        assert ku[0] == k and ku[1] == k
        eng.close()
    # C2 at k = 6, judged as test_eight_ranks_in_process_c2 judges it: against the extended-precision referee
    eng, rp, ci = c2(pkg)
    n, k = len(rp) - 1, 6
    X = np.stack([np.ones(n), np.random.default_rng(8).random(n)])
    a, b, ku, xn, _, st = eng.lanczos_multi(X, k)
    ans = eng.multout_multi(weights(O, a, b, ku, xn))
    for c in range(2):
        a_ref, b_ref, Q_ref, xn_ref = O.lanczos(rp, ci, k, X[c], q_colmajor=True)
        assert xn[c] == xn_ref and ku[c] == k
        check_leading_coefficients(a[c], b[c, :k - 1], a_ref, b_ref, ("c2", c), n=n)
        exact = O.referee_expm(rp, ci, k, X[c], caps=(40.0,))["ans"][0]
        e_orc = rel_inf(shift_weights(O, a_ref, b_ref, xn_ref) @ Q_ref, exact)
        e_dev = rel_inf(ans[c], exact)
        assert e_dev <= 1.5 * e_orc + 1e-13 and (e_orc > REL_INF_TOL or e_dev <= REL_INF_TOL), (c, e_dev, e_orc)
    eng.close()


def test_columns_independent_of_the_batch(pkg, oracle):
    O = oracle
    name, g, rp, ci = next(f for f in fixtures() if f[0].startswith("rmat_n3000"))
    n, k = len(rp) - 1, int(g["k"])
    rng = np.random.default_rng(21)
    X = np.vstack([fixture_batch(g, n), rng.random((13, n)) - 0.3])
    eng = pkg.Engine(0)
    eng.set_graph_csr(rp, ci)

    def run(cols):
        a, b, ku, xn, _, _ = eng.lanczos_multi(X[cols], k)
        return a, b, ku, xn, eng.multout_multi(weights(O, a, b, ku, xn))

    a16, b16, ku16, xn16, ans16 = run(list(range(16)))
    for cols in ([0], [5, 0], [3, 1, 4, 0, 2], list(rng.permutation(16))):
        a, b, ku, xn, ans = run(cols)
        for i, c in enumerate(cols):
            assert np.array_equal(a[i], a16[c]) and np.array_equal(b[i], b16[c]), (cols, c)
            assert ku[i] == ku16[c] and xn[i] == xn16[c] and np.array_equal(ans[i], ans16[c]), (cols, c)
    a, b, ku, xn, _ = run([0])
    a2, b2, ku2, xn2, _, _ = eng.lanczos_multi(2.0 * X[:1], k)
    assert np.array_equal(a2, a) and np.array_equal(b2, b) and np.array_equal(ku2, ku) and xn2[0] == 2.0 * xn[0]
    eng.close()


def joined_graph(g):
    """The fixture plus a disjoint path of 5 vertices, as CSR."""
    from scipy.sparse import coo_matrix
    n, pairs = with_path(g, int(g["mtx_n"]))
    r, c = pairs[:, 0] - 1, pairs[:, 1] - 1
    A = coo_matrix((np.ones(2 * len(r)), (np.r_[r, c], np.r_[c, r])), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return n, A.indptr.astype(np.uint64), A.indices.astype(np.uint32)


def test_breakdown_stop(pkg, oracle):
    from scipy.linalg import expm
    O = oracle
    g = np.load(GOLDEN[0])
    n0 = int(g["mtx_n"])
    n, rp, ci = joined_graph(g)
    assert np.array_equal(rp[:n0 + 1], g["ref_row_offset"].astype(np.uint64))
    k = 20
    E = expm(np.diag(np.ones(4), 1) + np.diag(np.ones(4), -1))
    X = np.zeros((5, n))
    X[0, :n0] = g["x"]
    X[1] = np.random.default_rng(4).random(n)
    seeds = (0, 2, 4)
    for i, v in enumerate(seeds):
        X[2 + i, n0 + v] = 1.0
    eng = pkg.Engine(0)
    eng.set_graph_csr(rp, ci)
    a, b, ku, xn, _, _ = eng.lanczos_multi(X, k)
    T = np.zeros((5, k))
    for c in range(5):
        kc = int(ku[c])
        lam, V = O.eigen(a[c, :kc], b[c, :kc - 1])
        T[c, :kc] = V @ (np.exp(lam) * (xn[c] * V[0, :]))   # e^A x itself: the path's component is small
    ans = eng.multout_multi(T)
    for i, v in enumerate(seeds):
        c = 2 + i
        assert 1 <= ku[c] <= 5 and not a[c, ku[c]:].any() and not b[c, ku[c] - 1:].any(), ku
        want = np.zeros(n)
        want[n0:] = E[:, v]
        assert np.abs(ans[c] - want).max() <= 1e-12 * np.abs(want).max(), (v, ku[c])
    # the other columns of the batch are untouched by the stops
    ans = eng.multout_multi(weights(O, a, b, ku, xn))
    for c in range(2):
        assert ku[c] == k
        a_ref, b_ref, Q_ref, xn_ref = O.lanczos(rp, ci, k, X[c], q_colmajor=True)
        check_leading_coefficients(a[c], b[c, :k - 1], a_ref, b_ref, c)
        assert rel_inf(ans[c], shift_weights(O, a_ref, b_ref, xn_ref) @ Q_ref) <= REL_INF_TOL, c
    eng.close()


def test_basis_recurrence(pkg, oracle):
    O = oracle
    name, g, rp, ci = next(fixtures())
    n, k = len(rp) - 1, int(g["k"])
    eng = pkg.Engine(0)
    eng.set_graph_csr(rp, ci)
    a, b, ku, xn, Q, _ = eng.lanczos_multi(fixture_batch(g, n), k, want_q=True)
    for c in range(3):
        kc = int(ku[c])
        check_recurrence(O, rp, ci, a[c, :kc], b[c, :kc - 1], Q[c, :kc], (name, c))
    eng.close()
    eng, rp, ci = c2(pkg)
    n, k = len(rp) - 1, 6
    X = np.stack([np.ones(n), np.random.default_rng(9).random(n)])
    a, b, ku, xn, Q, _ = eng.lanczos_multi(X, k, want_q=True)
    for c in range(2):
        check_recurrence(O, rp, ci, a[c], b[c, :k - 1], Q[c], ("c2", c))
    eng.close()


def test_single_vector_path_untouched(pkg, oracle):
    O = oracle
    name, g, rp, ci = next(fixtures())
    n, k = len(rp) - 1, int(g["k"])
    x = np.ones(n)
    eng = pkg.Engine(0)
    eng.set_graph_csr(rp, ci)
    eng.lanczos_prepare(x, k)
    eng.lanczos_run_steps(k)
    a0, b0, _ = eng.lanczos_fetch(k)
    t = shift_weights(O, a0, b0, np.sqrt(n))
    y0 = eng.multout(t)
    eng.lanczos_prepare(x, k)
    eng.lanczos_run_steps(5)
    eng.lanczos_multi(fixture_batch(g, n), k, want_q=True)
    eng.spmm(np.ones((3, n)))
    assert eng.lanczos_progress() == (5, k)
    eng.lanczos_run_steps(k)
    a1, b1, _ = eng.lanczos_fetch(k)
    assert np.array_equal(a1, a0) and np.array_equal(b1, b0) and np.array_equal(eng.multout(t), y0)
    eng.multi_release()
    a2, b2, _ = eng.lanczos_fetch(k)
    assert np.array_equal(a2, a0) and np.array_equal(b2, b0) and np.array_equal(eng.multout(t), y0)
    with pytest.raises(pkg.LzxError, match="no batched decomposition"):
        eng.multout_multi(np.ones((3, k)))
    eng.close()


def test_errors(pkg, oracle):
    name, g, rp, ci = next(fixtures())
    n = len(rp) - 1
    eng = pkg.Engine(0)
    eng.set_graph_csr(rp, ci)
    with pytest.raises(pkg.LzxError, match=r"\(-6\)"):
        eng.lanczos_multi(np.ones((17, n)), 4)
    X = np.ones((3, n))
    X[1] = 0.0
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*column 1"):
        eng.lanczos_multi(X, 4)
    with pytest.raises(pkg.LzxError, match=r"\(-4\).*bytes"):
        eng.lanczos_multi(np.ones((1, n)), 1 << 22)     # k * n * B * 8 = 4 Mi x 10 000 x 2 x 8 bytes
    a, b, ku, xn, _, _ = eng.lanczos_multi(np.ones((2, n)), 4)   # and nothing was left half-built
    assert (ku == 4).all() and np.isfinite(a).all()
    eng.close()
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(rp, ci)
    with pytest.raises(pkg.LzxError, match="one GPU"):
        grp.lanczos_multi(np.ones((2, n)), 4)
    grp.close()


def test_class_on_the_device_two_batches(pkg, tmp_path):
    host = load_host(pkg)
    g = np.load(GOLDEN[1])
    n, k = int(g["mtx_n"]), int(g["k"])
    mtx = str(tmp_path / "g.mtx")
    write_pairs(mtx, n, g["mtx_pairs"])
    X = np.vstack([fixture_batch(g, n), np.random.default_rng(30).random((17, n))])   # b = 20: batches of 16 and 4
    cpu = run_multi(host, mtx, n, k, X, cuda=0)
    dev = run_multi(host, mtx, n, k, X, cuda=1)
    assert np.array_equal(dev[3], cpu[3]) and np.array_equal(dev[4], cpu[4])
    for c in range(20):
        assert rel_inf(dev[0][c], cpu[0][c]) <= 1e-10, c
