"""GPU: stochastic Lanczos quadrature on the batched path (include/lzx.h: lzx_probes_f64, lzx_lanczos_probes_f64,
lzx_probe_diag_f64; Engine.trace_expm / diag_expm) -- the device probes against their numpy restatement, bit-identity with
lanczos_multi on the same probes, the quadratures against scipy's expm_multiply on the restated probes, the Hutchinson
estimate within its exact Rademacher spread, the diagonal reduction, C2 against a re-orthogonalising Lanczos in numpy, a
basis-free run whose basis could never fit, and the refusals."""
import glob
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import eigsh, expm_multiply

from bench import C2_DRAWS
from test_trace_host import numpy_lanczos, probe_np

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))
LAP = 1


def fixture(path):
    g = np.load(path)
    return os.path.basename(path)[:-4], g["ref_row_offset"].astype(np.uint64), g["ref_col_idx"]


def small_fixtures():
    return [f for f in map(fixture, GOLDEN) if len(f[1]) - 1 <= 4096]


def matrices(rp, ci):
    rp64, ci64 = rp.astype(np.int64), ci.astype(np.int64)
    n = len(rp64) - 1
    A = sp.csr_matrix((np.ones(len(ci64)), ci64, rp64), shape=(n, n))
    d = np.diff(rp64).astype(np.float64)
    return A, (sp.diags(d) - A).tocsr(), d


def engine(pkg, rp, ci, op=0):
    eng = pkg.Engine(0, operator=op)
    eng.set_graph_csr(rp, ci)
    return eng


def scale_and_shift(A, d, op):
    """(t, s, sigma): s (theta - sigma) spans about 12 under A (sigma = lambda_max), 5 under L (sigma = 0)."""
    if op == LAP:
        t = 5.0 / (2.0 * d.max())
        return t, -t, 0.0
    lam = float(eigsh(A, k=1, which="LA", return_eigenvectors=False)[0])
    t = 6.0 / lam
    return t, t, lam


def exact_ells(M, Z, s, sigma):
    """log(z^T e^{s (M - sigma)} z) + s sigma for every row z of Z."""
    n = M.shape[0]
    Y = expm_multiply(s * (M - sigma * sp.identity(n, format="csr")), Z.T)
    return np.log(np.einsum("in,ni->i", Z, Y)) + s * sigma


def c2(pkg):
    eng = pkg.Engine(0)
    eng.gen_rmat(20, 1 << 20, C2_DRAWS, 1234)          # BASELINE C2, generated on the device
    rp, ci = eng.get_graph_csr()
    return eng, rp, ci


def test_probes_match_the_definition(pkg):
    for name, rp, ci in map(fixture, GOLDEN):
        n = len(rp) - 1
        eng = engine(pkg, rp, ci)
        for seed, first, b in ((0, 0, 16), (0xDEADBEEF12345678, 7, 3), (5, (1 << 32) - 2, 2)):
            Z = eng.probes(seed, first, b)
            for c in range(b):
                assert np.array_equal(Z[c], probe_np(seed, first + c, n)), (name, seed, first, c)
        Z0, Z1 = eng.probes(0, 0, 2), eng.probes(1, 0, 2)
        assert not np.array_equal(Z0[0], Z0[1]) and not np.array_equal(Z0[0], Z1[0]), name
        eng.close()
    eng, rp, ci = c2(pkg)
    n = len(rp) - 1
    Z = eng.probes(20261016, 30, 16)
    for c in range(16):
        assert np.array_equal(Z[c], probe_np(20261016, 30 + c, n)), c
    eng.close()


def check_bit_identity(pkg, eng, k, seed, what):
    Z = eng.probes(seed, 0, 16)
    a, b, ku, _, _, st_m = eng.lanczos_multi(Z, k)
    for keep in (False, True):
        ap, bp, kup, st = eng.lanczos_probes(seed, 0, 16, k, keep_basis=keep)
        assert np.array_equal(ap, a) and np.array_equal(bp, b) and np.array_equal(kup, ku), (what, keep)
        assert st["iters"] == k and st["spmv_kernels"] == 4 and st["spmv_bytes"] == st_m["spmv_bytes"], (what, keep)
    # a probe's coefficients do not depend on the batch it runs in
    a3, b3, ku3, _ = eng.lanczos_probes(seed, 5, 3, k)
    assert np.array_equal(a3, a[5:8]) and np.array_equal(b3, b[5:8]) and np.array_equal(ku3, ku[5:8]), what


@pytest.mark.parametrize("op", [0, LAP], ids=["A", "L"])
def test_bit_identical_to_lanczos_multi(pkg, op):
    for name, rp, ci in map(fixture, GOLDEN):
        eng = engine(pkg, rp, ci, op)
        check_bit_identity(pkg, eng, 30, 77, (name, op))
        eng.close()
    eng, rp, ci = c2(pkg)
    eng.set_option("operator", op)
    check_bit_identity(pkg, eng, 20, 78, ("c2", op))
    eng.close()


@pytest.mark.parametrize("op", [0, LAP], ids=["A", "L"])
def test_trace_exact_on_small_graphs(pkg, op):
    k, N, seed = 50, 16, 2026
    for name, rp, ci in small_fixtures():
        n = len(rp) - 1
        A, L, d = matrices(rp, ci)
        M = L if op == LAP else A
        t, s, sigma = scale_and_shift(A, d, op)
        eng = engine(pkg, rp, ci, op)
        lt, rel, ell = eng.trace_expm(t, n_probes=N, k=k, seed=seed)
        _, _, ell_short = eng.trace_expm(t, n_probes=N, k=k - 10, seed=seed)
        assert np.abs(ell - ell_short).max() <= 1e-12, name           # converged at k
        Z = np.stack([probe_np(seed, p, n) for p in range(N)])
        ref = exact_ells(M, Z, s, sigma)
        assert np.abs(ell - ref).max() <= 1e-10, (name, np.abs(ell - ref).max())
        assert np.isfinite(rel) and rel > 0
        # several t in one pass: the bits of one t at a time
        ts = np.array([t / 4, t, 2 * t])
        lts, rels, ells = eng.trace_expm(ts, n_probes=N, k=k, seed=seed)
        assert lts.shape == (3,) and ells.shape == (3, N)
        for i, ti in enumerate(ts):
            l1, r1, e1 = eng.trace_expm(ti, n_probes=N, k=k, seed=seed)
            assert l1 == lts[i] and r1 == rels[i] and np.array_equal(e1, ells[i]), (name, i)
        eng.close()


@pytest.mark.parametrize("op", [0, LAP], ids=["A", "L"])
def test_trace_within_the_rademacher_spread(pkg, op):
    name, rp, ci = fixture([p for p in GOLDEN if p.endswith("er_n1000.npz")][0])
    A, L, d = matrices(rp, ci)
    M = (L if op == LAP else A).toarray()
    t = 1.0 if op == 0 else 1.0 / d.max()
    s = -t if op == LAP else t
    lam, V = np.linalg.eigh(M)
    sigma = lam.max() if op == 0 else 0.0
    F = (V * np.exp(s * (lam - sigma))) @ V.T
    N = 256
    eng = engine(pkg, rp, ci, op)
    lt, rel, ell = eng.trace_expm(t, n_probes=N, k=50, seed=99)
    eng.close()
    est = np.exp(lt - s * sigma)
    off = (F ** 2).sum() - (np.diag(F) ** 2).sum()
    assert abs(est - np.trace(F)) <= 4.0 * np.sqrt(2.0 * off) / np.sqrt(N), (est, np.trace(F))
    assert ell.shape == (N,) and rel < 0.1


def test_probe_diag_is_the_reduced_multout(pkg):
    for name, rp, ci in small_fixtures()[:3]:
        n = len(rp) - 1
        eng = engine(pkg, rp, ci)
        for first, b in ((0, 16), (40, 5)):
            a, be, ku, _ = eng.lanczos_probes(3, first, b, 30, keep_basis=True)
            T = pkg.slq_diag_coefficients(a, be, ku, n, 0.5, 0.0)
            T[1] *= -3.0                                         # any weights
            Y = eng.multout_multi(T)
            Z = eng.probes(3, first, b)
            want = np.zeros(n)
            for c in range(b):
                want = want + Z[c] * Y[c]
            assert np.array_equal(eng.probe_diag(T), want), (name, first, b)
            assert np.array_equal(eng.probe_diag(T[:, :20]), sum_rows(Z, eng.multout_multi(T[:, :20]))), name
        eng.close()


def sum_rows(Z, Y):
    acc = np.zeros(Z.shape[1])
    for c in range(Z.shape[0]):
        acc = acc + Z[c] * Y[c]
    return acc


@pytest.mark.parametrize("op", [0, LAP], ids=["A", "L"])
def test_diag_expm_matches_expm_multiply(pkg, op):
    N, seed = 32, 31
    for name, rp, ci in small_fixtures():
        n = len(rp) - 1
        A, L, d = matrices(rp, ci)
        M = L if op == LAP else A
        t, s, _ = scale_and_shift(A, d, op)
        eng = engine(pkg, rp, ci, op)
        est, sigma = eng.diag_expm(t, n_probes=N, k=50, seed=seed)
        eng.close()
        if op == LAP:
            assert sigma == 0.0
        Z = np.stack([probe_np(seed, p, n) for p in range(N)])
        Y = expm_multiply(s * (M - sigma * sp.identity(n, format="csr")), Z.T).T
        ref = (Z * Y).sum(axis=0) / N
        assert np.abs(est - ref).max() <= 1e-10 * np.abs(ref).max(), (name, np.abs(est - ref).max())


def test_c2_against_reorthogonalised_lanczos(pkg):
    """BASELINE C2 at k = 50, basis-free, N = 32: probes 0 and 17 against a numpy Lanczos with full re-orthogonalisation on the
    scipy matrix, under L at t = 1 / d_max and under A at t = 1 in shifted form (sigma = the largest Ritz value)."""
    eng, rp, ci = c2(pkg)
    A, L, d = matrices(rp, ci)
    n, k, seed = len(rp) - 1, 50, 4
    for op, M, t in ((LAP, L, 1.0 / d.max()), (0, A, 1.0)):
        eng.set_option("operator", op)
        s = -t if op == LAP else t
        lt, rel, ell = eng.trace_expm(t, n_probes=32, k=k, seed=seed)
        assert ell.shape == (32,) and np.isfinite(lt) and np.isfinite(ell).all()
        for p in (0, 17):
            a, b = numpy_lanczos(lambda x: M @ x, probe_np(seed, p, n), k)
            T = np.diag(a) + np.diag(b[:-1], 1) + np.diag(b[:-1], -1)
            theta, V = np.linalg.eigh(T)
            sigma = theta.max() if op == 0 else 0.0
            ref = np.log(n) + s * sigma + np.log(np.sum(V[0, :] ** 2 * np.exp(s * (theta - sigma))))
            assert abs(ell[p] - ref) <= 1e-10 * max(1.0, abs(ref)), (op, p, ell[p], ref)
    eng.close()


def test_basis_free_run_beyond_device_memory(pkg):
    """k * n * 16 * 8 = 2.56 TB: keeping the basis is refused; the basis-free run needs about 4 * n * 16 * 8 = 10 GB."""
    n, k = 20_000_000, 1000
    eng = pkg.Engine(0)
    eng.gen_er(n, 20_000_000, 7)
    with pytest.raises(pkg.LzxError, match=r"\(-4\).*lzx_lanczos_probes_f64.*bytes"):
        eng.lanczos_probes(1, 0, 16, k, keep_basis=True)
    with pytest.raises(pkg.LzxError, match=r"\(-3\)"):      # nothing left behind
        eng.probe_diag(np.ones((16, k)))
    a, b, ku, st = eng.lanczos_probes(1, 0, 16, k)
    assert np.isfinite(a).all() and np.isfinite(b).all() and (ku >= 1).all() and st["iters"] == k
    lt, rel = pkg.slq_trace(pkg.slq_log_quadratures(a, b, ku, n, 1.0))
    assert np.isfinite(lt).all()
    eng.close()


def test_refusals_and_isolation(pkg):
    name, rp, ci = fixture(GOLDEN[0])
    n, k = len(rp) - 1, 20
    eng = engine(pkg, rp, ci)
    with pytest.raises(pkg.LzxError, match=r"\(-6\)"):
        eng.lanczos_probes(0, 0, 17, k)
    with pytest.raises(pkg.LzxError, match=r"\(-6\)"):
        eng.probes(0, 0, 17)
    with pytest.raises(pkg.LzxError, match=r"\(-1\).*2\^32"):
        eng.lanczos_probes(0, (1 << 32) - 2, 3, k)
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*no probe basis"):   # nothing ran yet
        eng.probe_diag(np.ones((2, k)))
    eng.lanczos_probes(0, 0, 2, k)
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*no probe basis"):   # basis-free
        eng.probe_diag(np.ones((2, k)))
    with pytest.raises(pkg.LzxError, match="no batched decomposition"):
        eng.multout_multi(np.ones((2, k)))
    eng.lanczos_multi(np.ones((2, n)), k)
    with pytest.raises(pkg.LzxError, match=r"\(-3\).*no probe basis"):   # a basis of caller vectors
        eng.probe_diag(np.ones((2, k)))
    # a prepared, chunked single-vector decomposition and its basis survive probe runs
    x = np.ones(n)
    eng.lanczos_prepare(x, k)
    eng.lanczos_run_steps(k)
    a0, b0, _ = eng.lanczos_fetch(k)
    t = pkg._expm_coefficients(a0, b0, np.sqrt(n), 1.0)
    y0 = eng.multout(t)
    eng.lanczos_prepare(x, k)
    eng.lanczos_run_steps(5)
    a1, b1, ku1, _ = eng.lanczos_probes(0, 0, 16, k, keep_basis=True)
    eng.probe_diag(pkg.slq_diag_coefficients(a1, b1, ku1, n, 1.0, 0.0))
    eng.lanczos_probes(0, 0, 16, k)
    eng.trace_expm(1.0, n_probes=20, k=k)
    assert eng.lanczos_progress() == (5, k)
    eng.lanczos_run_steps(k)
    a2, b2, _ = eng.lanczos_fetch(k)
    assert np.array_equal(a2, a0) and np.array_equal(b2, b0) and np.array_equal(eng.multout(t), y0)
    eng.close()
    grp = pkg.LocalGroup([0, 0])
    grp.set_graph_csr(rp, ci)
    for call in (lambda e: e.lanczos_probes(0, 0, 2, k), lambda e: e.probes(0, 0, 2)):
        with pytest.raises(pkg.LzxError, match=r"\(-3\).*one GPU"):
            call(grp.engines[0])
    grp.close()
