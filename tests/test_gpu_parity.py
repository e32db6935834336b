"""GPU parity tests proper: the HIP path, called through the C ABI (include/lzx.h), against the CPU
oracle on the same seeded inputs.  Tolerances: integer / index work bit-exact; the centrality vector within the
north star's 1e-10 relative infinity-norm of the serial/ restatement -- always through the overflow-safe form
e^(A - theta_max) x (shifted_answer), and as e^A x itself where that is representable; x_norm exact; alpha_0, beta_0
1e-12 and alpha_1 1e-10 relative.  Later alpha_j / beta_j are NOT compared (Lanczos amplifies rounding-level
differences of the reduction order once Ritz values converge; the reference's own CPU/GPU pair behaves the same):
the three-term recurrence residual and the unit norms pin every column of the basis instead."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_INF_TOL = 1e-10  # BASELINE.json north_star: "within 1e-10 relative inf-norm of serial/"


def rel_inf(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# engine modes: plain gather path (bit-exact body rows); propagation-blocked path (long runs cross the two passes as
# partial row sums); the same with a tiny hub so that almost every entry goes through the blocked passes; every run
# plain (one x value per entry); a mix of reduced and plain runs with row bands cut into many gather items and small
# scatter units (and the 16 Ki column band that graphs of this size would not get by themselves)
MODES = [dict(propagation_blocking=0), dict(propagation_blocking=1), dict(propagation_blocking=1, hub_entries=64),
         dict(propagation_blocking=1, pb_reduce=0),
         dict(propagation_blocking=1, hub_entries=512, pb_reduce=1500, pb_target=1024, pb_unit=4096, pb_column_band=16384),
         # the 18 Ki column band (144 KiB tile, 15-bit column codes): reduced and plain runs
         dict(propagation_blocking=1, hub_entries=512, pb_column_band=18432), dict(propagation_blocking=1, hub_entries=64, pb_reduce=16, pb_column_band=18432, pb_unit=4096),
         # the forms large graphs get by themselves, forced on small ones: narrow staged-only slices class by class, small row
         # bands gathered one wavefront each (eight per item), rows ranked by staged-column count first
         dict(propagation_blocking=1, hub_entries=64, narrow_slices=1, pb_group_force=8, pb_target=2048),
         dict(propagation_blocking=1, hub_entries=256, narrow_slices=1, pb_group_force=8, pb_group=1024, tie_sort=2),
         # the gather pass's dynamic tail (large graphs: the cheapest fifth of the items is drawn from a counter by whichever
         # workgroup has finished its list): few workgroups, many small items, 40 % of them drawn; and with grouped bands
         dict(propagation_blocking=1, hub_entries=64, pb_target=1024, pb_gather_grid=8, pb_dyn_share=40),
         # ... and the kernel large graphs get: stream loads non-temporal (chosen by the stream's size; forced here)
         dict(propagation_blocking=1, hub_entries=64, pb_target=2048, pb_group_force=4, pb_gather_grid=6, pb_dyn_share=60, pb_gather_nt=1),
         dict(propagation_blocking=1, pb_gather_nt=1),
         # groups of few small bands: every band streamed by several wavefronts (four with two bands per group, eight for a
         # group's last single band), folded by its first one behind a barrier
         dict(propagation_blocking=1, hub_entries=64, pb_group_force=2, pb_target=2048),
         dict(propagation_blocking=1, hub_entries=256, pb_group_force=3, pb_group=2048, pb_gather_grid=5),
         # the reduced step's cross-lane carry through LDS slots (rounds 1 - 3) instead of the fixed-order scan in registers
         dict(propagation_blocking=1, hub_entries=64, pb_carry_scan=0), dict(propagation_blocking=1, pb_carry_scan=0, pb_target=2048),
         # the scatter pass's tables read with non-temporal loads
         dict(propagation_blocking=1, hub_entries=64, pb_scatter_nt=1)]


def graphs(O):
    yield "er_c1", O.gen_er(10000, 100000, 1234)           # BASELINE config C1
    yield "er_200k", O.gen_er(200000, 1000000, 21)           # 13 column bands x 196 row bands when blocked
    yield "rmat_s14", O.gen_rmat(14, 12000, 200000, 7)       # skewed, n not a power of two, split rows
    yield "er_tiny", O.gen_er(130, 300, 3)
    yield "rmat_hub", O.gen_rmat(16, 65536, 1500000, 99, a=0.7, b=0.12, c=0.12)  # very long rows


def pipeline_ref(O, rp, ci, k, x0):
    a, b, Q, xn = O.lanczos(rp, ci, k, x0, q_colmajor=True)
    lam, V = O.eigen(a, b)
    return a, b, Q, xn, O.mult_out(np.ascontiguousarray(Q.T), V, lam, xn)


def shift_weights(O, a, b, xn, cap=40.0):
    """t = V (e^(s (lambda - lambda_max)) .* ||x|| V[0,:]): multOut's small k x k part (parallel-final/lib/multiplyOut.cu:30-40)
    with the exponent shifted by the largest Ritz value, so that e^(s (A - theta_max)) x = Q t is finite on every graph
    (e^A x itself overflows fp64 on the hub-heavy ones, as the reference's own runs report), and with s = min(1, 40 /
    theta_max): where theta_max is in the hundreds a k-step Krylov approximation of e^A x has not converged to 1e-10
    (two correct fp64 runs then differ by more than that: the plain-mode engine and the oracle do on rmat_hub at k = 20,
    4.7e-10), while e^(sA) x with s theta_max <= 40 has, so it pins basis and coefficients at the north star's 1e-10.
    On every graph with theta_max <= 40 (all fixtures, C1) s = 1: the centrality vector itself, scaled.
    cap = None: s = 1 whatever theta_max is (e^(A - theta_max) x: at large k, where the top Ritz pair has converged)."""
    lam, V = O.eigen(a, b)
    s = 1.0 if cap is None else min(1.0, cap / max(lam.max(), 1e-300))
    return V @ (np.exp(s * (lam - lam.max())) * (xn * V[0, :]))


def check_leading_coefficients(a, b, a_ref, b_ref, name, n=0):
    """The Lanczos recurrence amplifies rounding-level differences (here: the order of the alpha / beta
    reductions) once Ritz values converge, so late alpha_j / beta_j of two correct fp64 runs differ freely
    -- the reference's own CPU and GPU paths do.  What is pinned coefficient-wise is the
    start of the recurrence; the centrality vector, which is what the method is for, is pinned at 1e-10.
    n: vertices, for the tolerance of beta_0 on large graphs -- the reference's norm is ONE left-to-right sum
    (serial/lib/lanczos.cc:157-163); with x0 = ones it adds ~n/2 identical tiny squares (the vertices without
    edges) to an accumulator that the hub vertices, first in R-MAT order, made large, and identical addends round the
    same way every time: a systematic error of up to n * eps / 2 relative (measured 1.1e-11 on the 1 M-vertex C2
    graph, where the engine's tree-shaped sums are the accurate side)."""
    assert abs(a[0] - a_ref[0]) <= 1e-12 * abs(a_ref[0]), name
    if len(b):
        assert abs(b[0] - b_ref[0]) <= max(1e-12, n * 1.2e-16) * abs(b_ref[0]), name
    if len(a) > 1:
        assert abs(a[1] - a_ref[1]) <= 1e-10 * max(abs(a_ref[1]), abs(a_ref[0])), name


def check_recurrence(O, rp, ci, a, b, Q, name):
    """Size-independent property: A Q_k = Q_k T_k + beta_k q_{k+1} e_k^T column by column, i.e. for j < k-1
    A q_j - alpha_j q_j - beta_{j-1} q_{j-1} - beta_j q_{j+1} = 0 to rounding, and every q_j has unit norm."""
    k = len(a)
    scale = max(np.abs(a).max(), np.abs(b).max() if len(b) else 0.0)
    for j in range(k - 1):
        r = O.spmv(rp, ci, Q[j]) - a[j] * Q[j] - b[j] * Q[j + 1]
        if j > 0:
            r -= b[j - 1] * Q[j - 1]
        assert np.abs(r).max() <= 1e-12 * scale, (name, j)
        assert abs(np.linalg.norm(Q[j]) - 1.0) <= 1e-13, (name, j)


def test_forced_shapes_run_the_product_library(pkg):
    """every mode of MODES -- the forced run formats, band / item / unit sizes, slice classes and
    gather groups -- is served by liblzx.so itself through its test-only entry lzx_test_set_shape (csrc/lzx_test_hooks.h),
    so the parity tests below meet the oracle with the machine code the bench runs; only experiment knobs select
    liblzx_dbg.so."""
    for mode in MODES + [dict(exchange_at_world_1=1), dict(isolated_rows=0), dict(unnormalised_basis=0), dict(fuse_staged=0), dict(fuse_staged=1),
                         dict(reference_order=1)]:
        eng = pkg.Engine(0, **mode)
        assert eng.L is pkg.lib() and not eng.debug, mode
        eng.close()
    eng = pkg.Engine(0, phase_mask=3)
    assert eng.debug and eng.L is pkg.lib(debug=True)
    eng.close()
    eng = pkg.Engine(0)
    with pytest.raises(pkg.LzxError):
        eng.set_option("phase_mask", 3)          # the product library does not know experiment knobs
    eng.close()


def test_spmv_matches_oracle(oracle, engine_factory):
    O = oracle
    rng = np.random.default_rng(1234)
    for name, (rp, ci) in graphs(O):
        n = len(rp) - 1
        x = rng.random(n)
        y_ref = O.spmv(rp, ci, x)
        for mode in MODES[1:]:
            eng = engine_factory(**mode)
            eng.set_graph_csr(rp, ci)
            gi = eng.info()
            n_active = int((np.diff(rp.astype(np.int64)) > 0).sum())   # blocked only if some referenced column is not staged
            assert (gi["pb_entries"] > 0) == (n_active > gi["hub_entries"]), (name, mode)
            assert gi["pb_reduced_entries"] <= gi["pb_entries"], (name, mode)
            if mode.get("pb_reduce", 1) == 0:      # one value per (padded) entry
                assert gi["pb_reduced_entries"] == 0 and gi["pb_values"] >= gi["pb_entries"], (name, mode)
            assert np.allclose(eng.spmv(x), y_ref, rtol=1e-13, atol=0), (name, mode)
            if "pb_dyn_share" in mode and name in ("er_200k", "rmat_hub"):   # the tail really is drawn at run time there
                assert eng.shape("gather_items_drawn") > 0 and eng.shape("gather_workgroups") == mode["pb_gather_grid"], (name, mode)
                assert np.array_equal(eng.spmv(x), eng.spmv(x)), (name, mode)
            eng.close()
        eng = engine_factory(**MODES[0])
        eng.set_graph_csr(rp, ci)
        assert eng.info()["pb_entries"] == 0
        y = eng.spmv(x)
        # Rows of the sliced-ELL body are summed left to right by one lane, the reference's own order
        # (serial/lib/SPMV.cc:24-27): bit-exact.  The split rows (degree > 128, rounded up to a whole
        # 64-row slice in degree order) are tree-summed: 1e-13 relative.
        deg = np.diff(rp.astype(np.int64))
        order = np.argsort(-deg, kind="stable")
        n_split = -(-int((deg > 128).sum()) // 64) * 64
        body = np.ones(n, dtype=bool)
        body[order[:n_split]] = False
        assert np.array_equal(y[body], y_ref[body]), name
        assert np.allclose(y[~body], y_ref[~body], rtol=1e-13, atol=0), name
        eng.close()


def test_lanczos_matches_oracle(oracle, engine_factory):
    O = oracle
    for name, (rp, ci) in graphs(O):
        n = len(rp) - 1
        k = min(20, n - 1)
        x0 = np.ones(n)
        a_ref, b_ref, Q_ref, xn_ref, ans_ref = pipeline_ref(O, rp, ci, k, x0)
        for mode in MODES:
            eng = engine_factory(**mode)
            eng.set_graph_csr(rp, ci)
            a, b, Q, xn, st = eng.lanczos(x0, k)
            assert xn == xn_ref
            check_leading_coefficients(a, b, a_ref, b_ref, (name, mode))
            check_recurrence(O, rp, ci, a, b, Q, (name, mode))
            lam, V = O.eigen(a, b)
            # the north-star criterion in its overflow-safe form, on EVERY graph: e^(A - theta_max) x
            shifted_ref = shift_weights(O, a_ref, b_ref, xn_ref) @ Q_ref
            assert np.isfinite(shifted_ref).all() and np.abs(shifted_ref).max() > 0, name
            assert rel_inf(shift_weights(O, a, b, xn) @ Q, shifted_ref) <= REL_INF_TOL, (name, mode)
            assert rel_inf(eng.multout(shift_weights(O, a, b, xn)), shifted_ref) <= REL_INF_TOL, (name, mode)
            # and as e^A x itself wherever fp64 can hold it (all graphs here but the hub-heavy one)
            assert np.isfinite(ans_ref).all() or name == "rmat_hub", name
            if np.isfinite(ans_ref).all():
                ans_host = O.mult_out(np.ascontiguousarray(Q.T), V, lam, xn)       # host multOut on the GPU basis
                ans_dev = eng.multout(V @ (np.exp(lam) * (xn * V[0, :])))            # device multOut
                assert rel_inf(ans_host, ans_ref) <= REL_INF_TOL, (name, mode)
                assert rel_inf(ans_dev, ans_ref) <= REL_INF_TOL, (name, mode)
            assert st["iters"] == k and st["loop_ms"] > 0
            eng.close()


def test_generators_bit_exact(oracle, engine_factory):
    O = oracle
    eng = engine_factory()
    eng.gen_er(5000, 40000, 42)
    rp, ci = eng.get_graph_csr()
    rp_ref, ci_ref = O.gen_er(5000, 40000, 42)
    assert np.array_equal(rp, rp_ref) and np.array_equal(ci, ci_ref)
    eng.gen_rmat(13, 7000, 90000, 5)
    rp, ci = eng.get_graph_csr()
    rp_ref, ci_ref = O.gen_rmat(13, 7000, 90000, 5)
    assert np.array_equal(rp, rp_ref) and np.array_equal(ci, ci_ref)
    eng.close()


def test_edge_ingest_matches_loader(oracle, engine_factory, tmp_path):
    O = oracle
    rp, ci = O.gen_er(3000, 20000, 11)
    path = str(tmp_path / "g.mtx")
    O.write_mtx(path, 3000, rp, ci)
    tok = np.array(open(path).read().split(), dtype=np.int64)
    pairs = tok[3:].reshape(-1, 2) - 1
    # duplicates and both orientations must collapse exactly as the std::set build does
    src = np.concatenate([pairs[:, 1], pairs[:50, 0]])
    dst = np.concatenate([pairs[:, 0], pairs[:50, 1]])
    eng = engine_factory()
    eng.set_graph_edges(3000, src, dst)
    rp2, ci2 = eng.get_graph_csr()
    assert np.array_equal(rp2, rp) and np.array_equal(ci2, ci)
    # a self loop is one diagonal entry there (both inserted keys are equal): compare with the loader on such a file
    with open(path, "a") as f:
        f.write("6 6\n8 8\n")
    lines = open(path).read().split("\n")
    hdr = lines[0].split()
    lines[0] = f"{hdr[0]} {hdr[1]} {int(hdr[2]) + 2}"
    open(path, "w").write("\n".join(lines))
    _, _, rp3, ci3 = O.load_mtx(path)
    assert len(ci3) == len(ci) + 2
    eng.set_graph_edges(3000, np.concatenate([src, [5, 7]]), np.concatenate([dst, [5, 7]]))
    rp4, ci4 = eng.get_graph_csr()
    assert np.array_equal(rp4, rp3) and np.array_equal(ci4, ci3)
    y = eng.spmv(np.arange(3000, dtype=np.float64))
    assert np.allclose(y, O.spmv(rp3, ci3, np.arange(3000, dtype=np.float64)), rtol=1e-13)
    eng.close()


def test_rows_without_an_edge_as_one_scalar_recurrence(oracle, pkg):
    """The lazy loop (blocked mode on one GPU, every mode on several) neither reads nor writes the rows of vertices
    without an edge: (A u)_i = 0 there, so q_j[i] = c_j q_0[i] with one scalar recurrence for all of them
    (k_lazy_update).  With a NON-constant start vector: the basis rows of those vertices against the oracle's
    elementwise ones (serial/lib/lanczos.cc:26-44), their share of the norms through alpha / beta, the device multOut in
    its factored form (before anybody fetched the basis) and after the basis has been materialised."""
    O = oracle
    rp, ci = O.gen_rmat(15, 30000, 120000, 11)       # about half of the vertices have no edge
    n, k = len(rp) - 1, 14
    deg = np.diff(rp.astype(np.int64))
    iso = deg == 0
    assert 0.3 * n < iso.sum() < 0.8 * n
    x0 = 0.5 + np.random.default_rng(17).random(n)
    a_ref, b_ref, Q_ref, xn_ref, ans_ref = pipeline_ref(O, rp, ci, k, x0)
    lam_ref, V_ref = O.eigen(a_ref, b_ref)
    t = V_ref @ (np.exp(lam_ref) * (xn_ref * V_ref[0, :]))
    assert np.isfinite(ans_ref).all()

    def check(eng, name):
        eng.set_graph_csr(rp, ci)
        xn = eng.lanczos_prepare(x0, k)
        eng.lanczos_run()
        assert xn == xn_ref
        ans_factored = eng.multout(t)                  # nobody has asked for the basis yet
        a, b, Q = eng.lanczos_fetch(k, want_q=True)    # materialises the rows
        ans_filled = eng.multout(t)
        check_leading_coefficients(a, b, a_ref, b_ref, name)
        check_recurrence(O, rp, ci, a, b, Q, name)
        for j in range(min(k, 6)):                     # early columns: before rounding differences have grown
            assert np.allclose(Q[j][iso], Q_ref[j][iso], rtol=1e-10, atol=1e-16), (name, j)
        assert rel_inf(ans_factored, ans_ref) <= REL_INF_TOL, name
        assert rel_inf(ans_filled, ans_ref) <= REL_INF_TOL, name
        # (relative to the largest entry: on the rows without an edge the sum over j cancels by many orders of magnitude, so
        #  the two forms -- c_j q_0[i] t_j, and the materialised column times t_j / beta_{j-1} -- agree to rounding of the TERMS)
        assert rel_inf(ans_factored, ans_filled) <= 1e-13, name
        eng.close()

    check(pkg.Engine(0, propagation_blocking=1, hub_entries=256), "blocked")
    check(pkg.Engine(0, propagation_blocking=0, lazy_normalisation=1), "plain, lazy")
    check(pkg.Engine(0, propagation_blocking=1, hub_entries=256, isolated_rows=0), "blocked, elementwise")
    # the resident basis normalised (q_j stored, u_j in two alternating buffers) instead of unnormalised
    check(pkg.Engine(0, propagation_blocking=1, hub_entries=256, unnormalised_basis=0), "blocked, q_j stored")
    check(pkg.Engine(0, propagation_blocking=1, hub_entries=256, unnormalised_basis=0, isolated_rows=0), "blocked, q_j stored, elementwise")
    # three ranks: every rank carries the rows of its own slice; their share of ||u||^2 travels in the all-reduce
    for mode in (dict(propagation_blocking=1, hub_entries=256), dict(propagation_blocking=0)):
        grp = pkg.LocalGroup([0, 0, 0], **mode)
        grp.set_graph_csr(rp, ci)
        a, b, Q, xn, st = grp.lanczos(x0, k)
        check_leading_coefficients(a, b, a_ref, b_ref, ("local3", mode))
        check_recurrence(O, rp, ci, a, b, Q, ("local3", mode))
        for j in range(min(k, 6)):
            assert np.allclose(Q[j][iso], Q_ref[j][iso], rtol=1e-10, atol=1e-16), (mode, j)
        assert rel_inf(grp.multout(t), ans_ref) <= REL_INF_TOL, mode
        grp.close()


def test_local_group_matches_single(oracle, pkg):
    """world = 3 handles on one GPU wired as an in-process communicator: same alpha/beta/answer."""
    O = oracle
    rp, ci = O.gen_rmat(14, 12000, 200000, 7)
    n, k = len(rp) - 1, 16
    x0 = np.ones(n)
    a_ref, b_ref, Q_ref, xn_ref, ans_ref = pipeline_ref(O, rp, ci, k, x0)
    # the last two: two 1-double all-reduces per iteration in the reference's operation order, instead of the default
    # single 2-double one on the unnormalised vector
    for mode in (dict(propagation_blocking=0), dict(propagation_blocking=1, hub_entries=256),
                 dict(propagation_blocking=0, lazy_normalisation=0), dict(propagation_blocking=1, hub_entries=256, lazy_normalisation=0)):
        grp = pkg.LocalGroup([0, 0, 0], **mode)
        grp.set_graph_csr(rp, ci)
        x = np.random.default_rng(5).random(n)
        assert np.allclose(grp.spmv(x), O.spmv(rp, ci, x), rtol=1e-13, atol=0)
        a, b, Q, xn, st = grp.lanczos(x0, k)
        check_leading_coefficients(a, b, a_ref, b_ref, ("local3", mode))
        check_recurrence(O, rp, ci, a, b, Q, ("local3", mode))
        lam, V = O.eigen(a, b)
        ans = grp.multout(V @ (np.exp(lam) * (xn * V[0, :])))
        assert rel_inf(ans, ans_ref) <= REL_INF_TOL
        assert rel_inf(O.mult_out(np.ascontiguousarray(Q.T), V, lam, xn), ans_ref) <= REL_INF_TOL
        grp.close()


def test_local_group_overlapped_exchange(oracle, pkg):
    """Large enough for the two-chunk exchange (chunk 0 = 32 Ki entries per rank here) to be in effect: the blocked
    SpMV starts on chunk 0 while chunk 1 is copied on the exchange streams.  Same answers as one handle, and as with
    the overlap switched off."""
    O = oracle
    rp, ci = O.gen_er(600000, 3000000, 77)
    n, k = len(rp) - 1, 10
    x0 = np.ones(n)
    a_ref, b_ref, Q_ref, xn_ref, ans_ref = pipeline_ref(O, rp, ci, k, x0)
    x = np.random.default_rng(9).random(n)
    y_ref = O.spmv(rp, ci, x)
    results = []
    # (overlap, minimum length of a reduced run): the runs of this graph are ~270 entries long, so the default (384)
    # leaves them plain and 128 makes them reduced, items of 2048 values cut every row band into several
    # the second chunk travels sparse (each peer gets what its rows reference) except in the last two variants (lazy, plain loop)
    for overlap, min_run, lazy, sparse in ((1, 384, 1, 1), (0, 384, 1, 1), (1, 128, 1, 1), (1, 384, 0, 1), (1, 384, 1, 0), (1, 384, 0, 0)):
        grp = pkg.LocalGroup([0, 0, 0], propagation_blocking=1, hub_entries=1024, overlap_exchange=overlap, pb_reduce=min_run,
                             pb_target=2048 if min_run == 128 else -1, lazy_normalisation=lazy, sparse_exchange=sparse)
        grp.set_graph_csr(rp, ci)
        gi = grp.engines[1].info()
        assert gi["pb_entries"] > 0 and 0 < gi["exchange_slice"] <= -(-gi["active_vertices"] // 3 // 64) * 64 + 64
        assert (gi["exchange_chunk0"] > 0) == (overlap == 1)
        assert (gi["exchange_recv"] < 2 * gi["exchange_slice"]) == (overlap == 1 and sparse == 1), gi
        assert (gi["pb_reduced_entries"] > gi["pb_entries"] // 2) == (min_run == 128), (overlap, min_run, gi)
        assert np.allclose(grp.spmv(x), y_ref, rtol=1e-13, atol=0)
        a, b, Q, xn, st = grp.lanczos(x0, k)
        check_leading_coefficients(a, b, a_ref, b_ref, ("overlap", overlap))
        check_recurrence(O, rp, ci, a, b, Q, ("overlap", overlap))
        lam, V = O.eigen(a, b)
        assert rel_inf(grp.multout(V @ (np.exp(lam) * (xn * V[0, :]))), ans_ref) <= REL_INF_TOL
        results.append((a, b))
        grp.close()
    # the chunked layout changes which column band an entry belongs to, hence the order of its additions: same first
    # coefficients to rounding, not bit for bit
    assert abs(results[0][0][0] - results[1][0][0]) <= 1e-13 * abs(results[1][0][0])
    assert abs(results[0][1][0] - results[1][1][0]) <= 1e-13 * abs(results[1][1][0])


def test_fp32_exchange_error_budget(oracle, pkg):
    """the exchanged vector rounded to fp32 (option exchange_fp32; sums stay fp64).  Half the bytes per
    iteration -- and, as budgeted, not within the 1e-10 criterion: every entry of the multiplied vector carries 6e-8
    relative rounding each iteration, which ends between 1e-8 and 1e-5 in the centrality vector (the reference's own
    float runs end at 1.2e-6, parallel-final/output/single_double.txt:319).  The fp64 exchange of the same group meets
    1e-10.  The recurrence stays consistent with what was multiplied: alpha_0 (the first SpMV runs on the exact x0) is
    untouched."""
    O = oracle
    rp, ci = O.gen_er(10000, 100000, 1234)                     # BASELINE C1's graph
    n, k = len(rp) - 1, 20
    x0 = np.ones(n)
    a_ref, b_ref, Q_ref, xn_ref, ans_ref = pipeline_ref(O, rp, ci, k, x0)
    seen = {}
    for fp32 in (0, 1):
        grp = pkg.LocalGroup([0, 0, 0], propagation_blocking=0, exchange_fp32=fp32)
        grp.set_graph_csr(rp, ci)
        gi = grp.engines[1].info()
        a, b, Q, xn, st = grp.lanczos(x0, k)
        lam, V = O.eigen(a, b)
        err = rel_inf(grp.multout(V @ (np.exp(lam) * (xn * V[0, :]))), ans_ref)
        seen[fp32] = (gi["exchange_recv"], err)
        assert abs(a[0] - a_ref[0]) <= 1e-12 * abs(a_ref[0])
        grp.close()
    print(f"C1 on 3 ranks, doubles received per rank and iteration / rel-inf error of e^A x: fp64 exchange {seen[0]}, fp32 exchange {seen[1]}")
    assert seen[0][1] <= REL_INF_TOL
    assert seen[1][0] * 2 == seen[0][0]
    assert 1e-9 < seen[1][1] < 1e-5, seen


def test_rccl_several_gpus():
    """The real thing where the box has it: 2 (or up to 4) ranks, one GPU each, RCCL over xGMI -- all exchange modes
    against the oracle (tests/rccl_ranks.py).  Skipped on a one-GPU box; the in-process groups above and
    test_rccl_world1 below cover the same code on one GPU."""
    import os
    import subprocess
    import sys
    import torch
    gpus = torch.cuda.device_count()
    if gpus < 2:
        pytest.skip("needs at least 2 GPUs")
    world = min(gpus, 4)
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                          "--master-addr", "127.0.0.1", "--master-port", "29641", os.path.join(here, "rccl_ranks.py")],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and f"RCCL_RANKS_OK {world}" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.parametrize("world", [2, 4])
def test_peer_windows_across_processes(world):
    """The several-process path on hardware, on the box's ONE GPU: `world` processes share it (RCCL refuses that --
    profiles/r4_rccl_one_gpu.txt -- the peer-window transport of csrc/lzx_ipc.hip does not): receive buffers mapped across
    processes, pushed slices, mailbox all-reduce, every exchange form of the loop against the oracle, the same coefficient
    bits on every rank (tests/ipc_ranks.py).  On a box with several GPUs LZX_IPC_SPREAD=1 puts one rank on each."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", LZX_IPC_TIMEOUT_MS="60000")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                          "--master-addr", "127.0.0.1", "--master-port", str(29650 + world), os.path.join(here, "ipc_ranks.py")],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and f"IPC_RANKS_OK {world}" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_peer_windows_world1(oracle, pkg):
    """The same transport at world = 1 with the test hook `exchange_at_world_1`: window creation, the board, publication of
    the receive buffers, put / wait / mailbox kernels on both streams -- in this very process."""
    O = oracle
    rp, ci = O.gen_er(300000, 1500000, 5)
    n, k = len(rp) - 1, 8
    x0 = np.ones(n)
    x = np.random.default_rng(4).random(n)
    a_ref, b_ref, Q_ref, xn_ref = O.lanczos(rp, ci, k, x0, q_colmajor=True)
    for mode in (dict(propagation_blocking=0), dict(propagation_blocking=1, hub_entries=1024),
                 dict(propagation_blocking=1, hub_entries=1024, overlap_exchange=0, lazy_normalisation=0),
                 dict(propagation_blocking=1, hub_entries=1024, sparse_exchange=0), dict(propagation_blocking=0, exchange_fp32=1)):
        eng = pkg.Engine(0, exchange_at_world_1=1, **mode)
        eng.comm_ipc_init(eng.comm_ipc_export(), 0, 1)
        eng.set_graph_csr(rp, ci)
        if not mode.get("exchange_fp32"):
            assert np.allclose(eng.spmv(x), O.spmv(rp, ci, x), rtol=1e-13, atol=0), mode
            a, b, Q, xn, st = eng.lanczos(x0, k)
            check_leading_coefficients(a, b, a_ref, b_ref, ("ipc1", mode), n=n)
            check_recurrence(O, rp, ci, a, b, Q, ("ipc1", mode))
        else:
            a, b, Q, xn, st = eng.lanczos(x0, k)
            assert np.allclose(a[:2], a_ref[:2], rtol=1e-6)
        assert st["iters"] == k
        eng.close()
    # a list that is not the handle's own export is refused; so is init without export
    eng = pkg.Engine(0)
    with pytest.raises(pkg.LzxError):
        eng.comm_ipc_init(np.zeros(128, dtype=np.uint8), 0, 1)
    blob = eng.comm_ipc_export()
    with pytest.raises(pkg.LzxError):
        eng.comm_ipc_init(np.zeros(128, dtype=np.uint8), 0, 1)
    eng.comm_ipc_init(blob, 0, 1)
    with pytest.raises(pkg.LzxError):
        eng.comm_ipc_init(blob, 0, 1)     # already wired
    eng.close()


def test_rccl_world1(oracle, pkg):
    """RCCL transport at world = 1: communicator creation, symbol resolution, stream plumbing -- and, with the test hook
    `exchange_at_world_1`, the several-rank loop itself on that communicator: ncclAllReduce of two doubles, ncclAllGather
    of the exchanged prefix, lazy normalisation and the reference's order, plain and blocked SpMV.  (Two ranks cannot
    share the one GPU of the test box under RCCL; the N > 1 arithmetic is covered by the in-process groups above.)"""
    O = oracle
    rp, ci = O.gen_er(4000, 30000, 2)
    n, k = 4000, 10
    x0 = np.ones(n)
    a_ref, b_ref, Q_ref, xn_ref, ans_ref = pipeline_ref(O, rp, ci, k, x0)
    x = np.random.default_rng(3).random(n)
    for mode in (dict(), dict(exchange_at_world_1=1), dict(exchange_at_world_1=1, lazy_normalisation=0),
                 dict(exchange_at_world_1=1, propagation_blocking=1, hub_entries=256)):
        eng = pkg.Engine(0, **mode)
        eng.comm_init_rank(pkg.Engine.unique_id(), 0, 1)
        eng.set_graph_csr(rp, ci)
        assert np.allclose(eng.spmv(x), O.spmv(rp, ci, x), rtol=1e-13, atol=0), mode
        a, b, Q, xn, st = eng.lanczos(x0, k)
        check_leading_coefficients(a, b, a_ref, b_ref, ("rccl1", mode))
        check_recurrence(O, rp, ci, a, b, Q, ("rccl1", mode))
        lam, V = O.eigen(a, b)
        assert rel_inf(eng.multout(V @ (np.exp(lam) * (xn * V[0, :]))), ans_ref) <= REL_INF_TOL, mode
        if mode.get("exchange_at_world_1"):
            assert st["comm_ms"] >= 0.0 and st["iters"] == k
        eng.close()
    # the two-chunk exchange on the second stream (blocked SpMV starting on chunk 0), same hook, a graph large enough
    rp, ci = O.gen_er(300000, 1500000, 5)
    n = len(rp) - 1
    x = np.random.default_rng(4).random(n)
    # (over RCCL the two-chunk exchange is on request only, until it has run on two or more physical GPUs)
    eng = pkg.Engine(0, exchange_at_world_1=1, propagation_blocking=1, hub_entries=1024)
    eng.comm_init_rank(pkg.Engine.unique_id(), 0, 1)
    eng.set_graph_csr(rp, ci)
    assert eng.info()["exchange_chunk0"] == 0 and eng.info()["pb_entries"] > 0
    eng.close()
    eng = pkg.Engine(0, exchange_at_world_1=1, propagation_blocking=1, hub_entries=1024, overlap_exchange=1, sparse_exchange=1)
    eng.comm_init_rank(pkg.Engine.unique_id(), 0, 1)
    eng.set_graph_csr(rp, ci)
    assert eng.info()["exchange_chunk0"] > 0 and eng.info()["pb_entries"] > 0
    assert np.allclose(eng.spmv(x), O.spmv(rp, ci, x), rtol=1e-13, atol=0)
    a, b, Q, xn, st = eng.lanczos(np.ones(n), 8)
    a_ref, b_ref, _, _ = O.lanczos(rp, ci, 8, np.ones(n))
    check_leading_coefficients(a, b, a_ref, b_ref, "rccl1 overlapped")
    check_recurrence(O, rp, ci, a, b, Q, "rccl1 overlapped")
    # Round 4: the hand-over's agreement point (lzx_comm_agree).  A rank-local failure BEFORE it -- here a column index out of
    # range, caught by the validation that precedes the reshaping -- must still cast its vote (the entry point's
    # lzx_agree_guard), come back as an error, and leave a handle and a communicator that work: the next hand-over, with its
    # own vote and the pairwise check of the sparse lists behind it, succeeds.
    bad = ci.copy()
    bad[7] = n + 5
    with pytest.raises(pkg.LzxError):
        eng.set_graph_csr(rp, bad)
    eng.set_graph_csr(rp, ci)
    assert np.allclose(eng.spmv(x), O.spmv(rp, ci, x), rtol=1e-13, atol=0)
    eng.close()


def test_known_answer_eigen_expansion_on_the_device(oracle, engine_factory):
    """The reference's own accuracy test, serial/tests/numerical_test.cc:74-116 (driver: k in 5..50), on the device:
    x = sum c_i v_i over 100 known eigenpairs, c_i ~ U(0,1) seed 1234, and the analytic e^A x = sum c_i e^(lambda_i) v_i
    as the answer -- an answer that owes nothing to the oracle.  The NotreDame_yeast fixtures (n = 2114) are not in the
    repository: the eigenpairs come from a dense eigh of a seeded graph of that size.  Checked: the reference's recorded
    error curve (serial/output/numerical_test_output.txt: 2.1 at k = 5, 3.5e-11 at k = 20, 4e-15 at k = 25, floor 3e-15)
    in shape -- monotone down to a rounding-level floor that is reached by k = 20 and kept to k = 50 -- in plain and in
    blocked mode, through the device multOut and the host one, and that the engine is never worse than the oracle."""
    O = oracle
    n = 2114
    ks = (5, 10, 15, 20, 25, 30, 40, 50)
    for gname, (rp, ci) in (("er", O.gen_er(n, 9000, 1234)), ("rmat", O.gen_rmat(12, n, 9000, 1234, a=0.45, b=0.22, c=0.22))):
        A = np.zeros((n, n))
        rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
        A[rows, ci.astype(np.int64)] = 1.0
        lam, Vec = np.linalg.eigh(A)
        c = np.random.default_rng(1234).random(100)
        top = Vec[:, -100:]
        x = top @ c
        exact = top @ (c * np.exp(lam[-100:]))                   # lambda_max = 9.5 / 26: e^A x itself is representable
        for mode in (dict(propagation_blocking=0), dict(propagation_blocking=1, hub_entries=64)):
            eng = engine_factory(**mode)
            eng.set_graph_csr(rp, ci)
            errs, errs_orc = [], []
            for k in ks:
                a, b, Q, xn, st = eng.lanczos(x, k)
                lk, V = O.eigen(a, b)
                t = V @ (np.exp(lk) * (xn * V[0, :]))
                dev = eng.multout(t)
                assert rel_inf(t @ Q, dev) <= 1e-13
                errs.append(np.linalg.norm(dev - exact) / np.linalg.norm(exact))   # the reference's measure (check_ans)
                ar, br, Qr, xr = O.lanczos(rp, ci, k, x, q_colmajor=True)
                lr, Vr = O.eigen(ar, br)
                errs_orc.append(np.linalg.norm((Vr @ (np.exp(lr) * (xr * Vr[0, :]))) @ Qr - exact) / np.linalg.norm(exact))
            print(gname, mode, " ".join(f"k={k}: {e:.1e} ({eo:.1e})" for k, e, eo in zip(ks, errs, errs_orc)))
            assert errs[0] > 1e-4 and errs[0] > errs[1] > errs[2]
            assert max(errs[3:]) < 1e-12, errs                   # the floor, reached by k = 20 and kept to k = 50
            assert all(e <= 2.0 * eo + 1e-13 for e, eo in zip(errs, errs_orc)), (errs, errs_orc)
            eng.close()


def test_general_csr_patterns(oracle, engine_factory):
    """The C ABI takes any pattern-only CSR, not only what the reference's loader produces: non-symmetric, columns in
    any order, duplicate entries (each one counts), self-loops, empty rows -- plain and blocked SpMV agree with the
    row sums of the oracle."""
    O = oracle
    rng = np.random.default_rng(11)
    n = 70000
    deg = rng.integers(0, 40, size=n)
    deg[rng.integers(0, n, size=50)] = 3000            # a few long rows
    deg[:10] = 0                                       # leading empty rows
    rp = np.zeros(n + 1, dtype=np.uint64)
    rp[1:] = np.cumsum(deg)
    ci = rng.integers(0, n, size=int(rp[-1]), dtype=np.uint32)   # unsorted, with duplicates and self-loops
    ci[: int(rp[20])] = np.arange(int(rp[20]), dtype=np.uint32) % 7   # heavy duplication in the first rows
    x = rng.random(n)
    y_ref = O.spmv(rp, ci, x)
    for mode in (dict(propagation_blocking=0), dict(propagation_blocking=1, hub_entries=1024),
                 dict(propagation_blocking=1, hub_entries=1024, pb_reduce=0)):
        eng = engine_factory(**mode)
        eng.set_graph_csr(rp, ci)
        assert np.allclose(eng.spmv(x), y_ref, rtol=1e-12, atol=1e-12), mode
        eng.close()


def test_odd_shapes_through_the_large_graph_forms(oracle, pkg):
    """Small graphs of awkward shapes -- no vertex without an edge, almost none with one, fewer vertices than a slice, a
    star, a clique beside isolated vertices, more staged slots than vertices -- through the forms large graphs take by
    themselves (narrow slice classes, grouped gather bands, shared scatter / staged-columns launch, unnormalised basis,
    rows without an edge as a scalar recurrence), on one handle and on three: SpMV of a random vector against the oracle
    at 1e-13, the recurrence of every basis column, the overflow-safe centrality functional at 1e-10."""
    O = oracle
    rng = np.random.default_rng(2024)

    def sym(n, src, dst):
        keep = src != dst
        src, dst = src[keep].astype(np.uint64), dst[keep].astype(np.uint64)
        return O.csr_from_keys(n, np.concatenate([(src << np.uint64(32)) | dst, (dst << np.uint64(32)) | src]))

    shapes = {}
    n = 5000
    ring = np.arange(n)
    shapes["ring + chords (every vertex has an edge)"] = sym(n, np.concatenate([ring, rng.integers(0, n, 20000)]),
                                                             np.concatenate([(ring + 1) % n, rng.integers(0, n, 20000)]))
    n = 40000
    shapes["three edges among 40 000 vertices"] = sym(n, np.array([5, 17, 39999]), np.array([6, 39998, 0]))
    shapes["40 vertices"] = sym(40, rng.integers(0, 40, 200), rng.integers(0, 40, 200))
    n = 30000
    shapes["star"] = sym(n, np.zeros(n - 1, dtype=np.int64), np.arange(1, n))
    k60 = np.array([(i, j) for i in range(60) for j in range(i + 1, 60)])
    shapes["clique of 60 beside 20 000 isolated vertices"] = sym(20060, k60[:, 0] + 10000, k60[:, 1] + 10000)
    n = 9000
    shapes["skewed, 9 000 vertices"] = O.gen_rmat(14, n, 150000, 3, a=0.65, b=0.15, c=0.15)
    modes = (dict(propagation_blocking=1, hub_entries=64, narrow_slices=1, pb_group_force=8, pb_target=2048),
             # the gather pass as large graphs get it (non-temporal stream loads) with a dynamic tail over three workgroups
             dict(propagation_blocking=1, hub_entries=64, narrow_slices=1, pb_target=1024, pb_gather_nt=1, pb_gather_grid=3, pb_dyn_share=50),
             dict(propagation_blocking=1, hub_entries=16384, narrow_slices=1, pb_group_force=2),
             dict(propagation_blocking=1, hub_entries=32, fuse_staged=1, tie_sort=2),
             dict(propagation_blocking=1, hub_entries=32, fuse_staged=0, unnormalised_basis=0))
    for name, (rp, ci) in shapes.items():
        n = len(rp) - 1
        k = min(12, n - 1)
        x0 = 0.5 + rng.random(n)
        x = rng.random(n)
        y_ref = O.spmv(rp, ci, x)
        a_ref, b_ref, Q_ref, xn_ref = O.lanczos(rp, ci, k, x0, q_colmajor=True)
        ref = shift_weights(O, a_ref, b_ref, xn_ref) @ Q_ref
        for mode in modes:
            for world in (1, 3):
                eng = pkg.Engine(0, **mode) if world == 1 else pkg.LocalGroup([0] * world, **mode)
                eng.set_graph_csr(rp, ci)
                assert np.allclose(eng.spmv(x), y_ref, rtol=1e-13, atol=0), (name, mode, world)
                a, b, Q, xn, st = eng.lanczos(x0, k)
                assert xn == xn_ref and np.isfinite(a).all() and np.isfinite(b).all(), (name, mode, world)
                # a Krylov space that closes early (star, clique: three or two distinct eigen-directions) ends in 0 / 0: only the
                # columns before the breakdown are defined -- in the oracle as well
                good = int(np.argmax(b_ref < 1e-9 * np.abs(a_ref).max())) if (b_ref < 1e-9 * np.abs(a_ref).max()).any() else k - 1
                check_leading_coefficients(a, b, a_ref, b_ref, (name, mode, world))
                if good >= k - 1:
                    check_recurrence(O, rp, ci, a, b, Q, (name, mode, world))
                    assert rel_inf(eng.multout(shift_weights(O, a, b, xn)), ref) <= REL_INF_TOL, (name, mode, world)
                eng.close()


def test_reference_order_shape_is_bit_identical_to_the_oracle(pkg, oracle):
    """VERDICT round 3, next 1(a).  Test shape `reference_order` of the PRODUCT library: the SpMV one lane per row of the
    caller's CSR (serial/lib/SPMV.cc:24-27 = cu_spMV1, parallel-final/lib/cu_SPMV.cu:31-41), inner product and norm one
    left-to-right accumulator over the caller's vertex order (serial/lib/lanczos.cc:155-171), the elementwise updates as in
    every other mode.  With the reductions in serial/'s order the device loop has no freedom left: alpha, beta and EVERY
    entry of the basis must equal the oracle's restatement bit for bit -- also the late coefficients, which no other test
    can compare (they amplify reduction-order noise) -- on every fixture graph, whatever layout the engine built
    underneath.  Then the production modes are reported against it: what is left is the reduction order alone."""
    O = oracle
    for name, (rp, ci) in graphs(O):
        n = len(rp) - 1
        k = min(30, n - 1)
        rng = np.random.default_rng(77)
        for x0 in (np.ones(n), rng.random(n) + 0.5):
            a_ref, b_ref, Q_ref, xn_ref = O.lanczos(rp, ci, k, x0, q_colmajor=True)
            for mode in (dict(propagation_blocking=0), dict(propagation_blocking=1, hub_entries=64)):
                eng = pkg.Engine(0, reference_order=1, **mode)
                assert eng.L is pkg.lib() and not eng.debug
                eng.set_graph_csr(rp, ci)
                a, b, Q, xn, st = eng.lanczos(x0, k)
                assert xn == xn_ref and st["iters"] == k
                assert np.array_equal(a, a_ref), (name, mode, np.flatnonzero(a != a_ref)[:4])
                assert np.array_equal(b, b_ref), (name, mode, np.flatnonzero(b != b_ref)[:4])
                assert np.array_equal(Q, Q_ref), (name, mode)
                # in chunks: the same bits (the resumable loop, N3)
                eng.lanczos_prepare(x0, k)
                eng.lanczos_run_steps(7)
                eng.lanczos_run_steps(k)
                a2, b2, Q2 = eng.lanczos_fetch(k, want_q=True)
                assert np.array_equal(a2, a_ref) and np.array_equal(b2, b_ref) and np.array_equal(Q2, Q_ref), (name, mode)
                eng.close()
    # several ranks: refused, not silently something else
    grp = pkg.LocalGroup([0, 0], reference_order=1)
    rp, ci = O.gen_er(10000, 100000, 1234)
    grp.set_graph_csr(rp, ci)
    with pytest.raises(pkg.LzxError):
        grp.lanczos(np.ones(10000), 4)
    grp.close()
    # R1 in the same shape: the Arnoldi pass of serial/lib/lanczos.cc:58-132 with its inner products left to right -- the
    # restatement orc_lanczos_arnoldi bit for bit, for the reference's own schedule (every 2nd iteration) and for every one
    for name, (rp, ci) in graphs(O):
        n = len(rp) - 1
        k = min(16, n - 1)
        x0 = np.ones(n)
        for every in (1, 2):
            a_ref, b_ref, Q_ref, xn_ref = O.lanczos_arnoldi(rp, ci, k, x0, every=every)
            eng = pkg.Engine(0, reference_order=1, reorthogonalise=every)
            eng.set_graph_csr(rp, ci)
            a, b, Q, xn, st = eng.lanczos(x0, k)
            assert xn == xn_ref and np.array_equal(a, a_ref) and np.array_equal(b, b_ref) and np.array_equal(Q, Q_ref), (name, every)
            eng.close()
