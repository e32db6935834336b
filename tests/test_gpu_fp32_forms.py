"""GPU: the two fp32 options at rounding level (include/lzx.h: "basis_fp32", "exchange_fp32").

basis_fp32 -- the kernels that touch the fp32-stored basis (k_lazy_update's f32_next store, k_to_f32, k_widen_col,
k_multout<float>, k_iso_fill<float>) against an fp64 engine of the same mode, entry by entry, at bounds that follow from where
each of them rounds; on graphs small enough for the last double2 / float2 pair to matter: paths of 2, 3, 65 and 257 vertices,
odd n = 2001, and the fixture with rows without an edge.

exchange_fp32 -- in-process groups against tests/test_fp32_model_host.py's model of the loop: the first coefficients at
TOL_FIRST / TOL_SECOND, and the three-term recurrence with the vector that WAS multiplied, f32(u_j) in every entry.

No bound below was fitted to what the device returned: each is derived where it is used, or quoted from the test it was taken
from.  Every test prints what it achieved next to its bound."""
import ctypes
import os

import numpy as np
import pytest

from test_fp32_model_host import (DISCRIMINATION, K_EXCHANGE, LD, PATHS_EXCHANGE, TOL_FIRST, TOL_SECOND, coefficient_distances,
                                  matvec_ld, models, path_csr, start_vector)

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24          # unit roundoff of fp32
U64 = 2.0 ** -53          # ... of fp64
SUB32 = 2.0 ** -149       # spacing of the fp32 subnormals (an absolute error of half of it would do)
K_BASIS = 12
CHUNKS = (1, 2, 7, 100)
GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")


def _fixture(name):
    g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return g["ref_row_offset"].astype(np.uint64), g["ref_col_idx"]


GRAPHS = {
    "path_2": lambda O: path_csr(2),
    "path_3": lambda O: path_csr(3),
    "path_65": lambda O: path_csr(65),
    "path_257": lambda O: path_csr(257),
    "er_odd_2001": lambda O: O.gen_er(2001, 14000, 5),
    "rmat_n4096": lambda O: _fixture("rmat_n4096"),          # rows without an edge: the factored form and k_iso_fill<float>
}
GROUPS_ON = ("er_odd_2001", "rmat_n4096")


class _One:
    """One handle behind the calls the checks need."""

    def __init__(self, pkg, **options):
        self.e = pkg.Engine(0, **options)

    def set_graph(self, rp, ci):
        self.e.set_graph_csr(rp, ci)
        return self.e.info()["pb_entries"]

    def prepare(self, x0, k):
        return self.e.lanczos_prepare(x0, k)

    def run_steps(self, steps):
        return self.e.lanczos_run_steps(steps)["iters"]

    def fetch(self, k):
        return self.e.lanczos_fetch(k, want_q=True)

    def multout(self, t):
        return self.e.multout(t)

    def multout_change(self, t):
        return self.e.multout_change(t)

    def close(self):
        self.e.close()


class _Three(_One):
    """Three in-process ranks on one GPU through the *_local entry points (the fetch widens each rank's slice, then all-gathers)."""

    def __init__(self, pkg, **options):
        self.pkg = pkg
        self.g = pkg.LocalGroup([0, 0, 0], **options)
        self.L, self.arr, self.world = self.g.L, self.g.arr, self.g.world

    def set_graph(self, rp, ci):
        self.g.set_graph_csr(rp, ci)
        return max(e.info()["pb_entries"] for e in self.g.engines)

    def prepare(self, x0, k):
        p = self.pkg
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        xn = ctypes.c_double()
        p._check(self.L.lzx_lanczos_prepare_f64_local(self.arr, self.world, p._p(x0, p._f64p), k, ctypes.byref(xn)),
                 "lzx_lanczos_prepare_f64_local", self.L)
        return xn.value

    def run_steps(self, steps):
        p = self.pkg
        st = p.LzxStats()
        p._check(self.L.lzx_lanczos_run_steps_local(self.arr, self.world, steps, ctypes.byref(st)), "lzx_lanczos_run_steps_local", self.L)
        return st.as_dict()["iters"]

    def fetch(self, k):
        p = self.pkg
        a, b, Q = np.zeros(k), np.zeros(max(k - 1, 1)), np.empty((k, self.g.n))
        p._check(self.L.lzx_lanczos_fetch_f64_local(self.arr, self.world, k, p._p(a, p._f64p), p._p(b, p._f64p), p._p(Q, p._f64p)),
                 "lzx_lanczos_fetch_f64_local", self.L)
        return a, b[:k - 1], Q

    def multout(self, t):
        return self.g.multout(t)

    def multout_change(self, t):
        p = self.pkg
        t = np.ascontiguousarray(t, dtype=np.float64)
        rc = ctypes.c_double()
        p._check(self.L.lzx_multout_change_f64_local(self.arr, self.world, p._p(t, p._f64p), len(t), ctypes.byref(rc)),
                 "lzx_multout_change_f64_local", self.L)
        return rc.value

    def close(self):
        self.g.close()


def _host_sums(t, Q):
    """(sum_j t_j Q[j, i], sum_j |t_j| |Q[j, i]|) in np.longdouble."""
    tl, Ql = np.asarray(t, dtype=LD), np.asarray(Q, dtype=LD)
    return tl @ Ql, np.abs(tl) @ np.abs(Ql)


def _check_basis_fp32(name, rp, ci, make, what):
    """One (graph, mode): an fp64 handle and a basis_fp32 handle of the same mode, side by side.

    WHERE THE fp32 ROUNDINGS ENTER (csrc/lzx_kernels.hip, csrc/lzx_api.hip: lanczos_prepare / lazy_step / lanczos_fetch):

    column 0          q_0 = x0 / ||x0|| in fp64 (k_permute_in), rounded once by k_to_f32; the fetch widens it (k_widen_col) and
                      divides by nothing: Q32[0] == f64(f32(Q64[0])) exactly.
    column j >= 1,    k_lazy_update stores (float)u_j beside the fp64 u_j it goes on working with; the fetch widens and divides
    rows with an      by beta_{j-1} (k_permute_out), as the fp64 engine divides its fp64 u_j.  One fp32 rounding, two fp64
    edge              ones:  |Q32 - Q64| <= 2^-24 (1 + 2^-20) |Q64| + 2^-149 / beta_{j-1}   (the second term: f32(u_j) subnormal).
    column j >= 1,    the lazy loop carries these rows as q_j[i] = c_j q_0[i], u_j[i] = d_j q_0[i] with one scalar recurrence
    rows WITHOUT      (k_lazy_update, block 0) and writes them out only for a fetch: k_iso_fill<float> stores
    an edge           (float)(d_j * z) with z = the STORED column 0, i.e. f32(q_0[i]) -- the fp64 q_0 lives in one of the
                      three ring vectors and is overwritten by u_3.  The fp64 engine stores d_j * q_0[i] (same d_j: the scalar
                      recurrence is fp64 in both).  TWO fp32 roundings (of q_0[i], then of the product), so the single-rounding
                      bound above does not hold there (it was first written down for every entry) -- a rounding that derivation
                      missed and the kernel legitimately performs.  Derived instead:
                      |Q32 - Q64| <= 2 * 2^-24 (1 + 2^-20) |Q64| + 2^-149 / beta_{j-1}.
                      (Rows without an edge below the loop's row limit, which is rounded up to a pair, take the elementwise
                      path and meet the tighter bound; the test does not rely on which rows those are.)
    every entry       Q32[j] * beta_{j-1} is an fp32 number up to the division and the multiplication back: within
                      4 * 2^-53 relative of its own fp32 rounding.

    multout(t)        k_multout<float>, rows with an edge: s = sum_j f64(stored_j) * tq_j in fp64, tq_j = t_j / beta_{j-1}
                      (k_multout_coeff).  Against sum_j t_j Q32[j, i] in longdouble, Q32[j, i] = stored_j / beta_{j-1}: per term the
                      two divisions and the product round (3), the sum adds k - 1 times: (k + 2) 2^-53, asserted as the
                      rounder (k + 4) 2^-53 sum_j |t_j| |Q32[j, i]|.
                      Rows without an edge: ALWAYS the factored form, s = sum_j (c_j * z) * t_j with z = f32(q_0[i]) and
                      c_j = d_j / beta_{j-1} -- lzx_launch_multout passes the scalars whenever the loop ran in that form,
                      "valid whether or not a fetch has materialised some columns meanwhile".  So the answer is the same
                      BITS before and after the fetch (asserted), and on these rows it stays one fp32 rounding away from the
                      host sum after the fetch too (rounding level was expected there at first; it is not what the code does,
                      and need not be).  Term by term c_j z t_j against t_j (f32(d_j z) / beta_{j-1}): one fp32 rounding of
                      d_j z, relative to the stored value 2^-24 (1 + 2^-24); fp64 roundings: d_j z, the two divisions, c_j z,
                      the product with t_j (5) and k - 1 additions:
                      (2^-24 (1 + 2^-20) + (k + 4) 2^-53) sum_j |t_j| |Q32[j, i]| + 2^-149 sum_j |t_j| / beta_{j-1}
                      -- well within (k + 4) 2^-24 times the same sum, the first estimate.
    multout_change    ||y_2 - y_1|| / ||y_2|| of two such answers: against the device's own two multout vectors at
                      1e-9 * max(change, 1e-6) (test_run_in_chunks_and_early_stop's tolerance), and against the two host sums
                      at the same tolerance plus what the fp32 rounding of the rows without an edge can move the ratio by
                      (0 on a graph that has none): with E the elementwise bounds above on those rows,
                      (||E_1|| + ||E_2|| + ratio ||E_2||) / (||y_2|| - ||E_2||)."""
    n = len(rp) - 1
    k = min(K_BASIS, n)
    x0 = start_vector(n)
    live = np.diff(rp.astype(np.int64)) > 0
    h64, h32 = make(0), make(1)
    try:
        pb64, pb32 = h64.set_graph(rp, ci), h32.set_graph(rp, ci)
        assert (pb64 > 0) == (pb32 > 0)
        xn64 = h64.prepare(x0, k)
        assert h64.run_steps(k) == k
        a64, b64, Q64 = h64.fetch(k)
        xn32 = h32.prepare(x0, k)
        assert h32.run_steps(k) == k
        t = np.random.default_rng(k).random(k)
        t2 = np.random.default_rng(k + 1).random(k)
        y_before = h32.multout(t)                      # nobody has fetched the basis yet
        a32, b32, Q32 = h32.fetch(k)
        y_after = h32.multout(t)
        y2 = h32.multout(t2)
        c1, c2 = h32.multout_change(t), h32.multout_change(t2)

        # 1. the loop never reads a rounded column
        assert xn32 == xn64 and np.array_equal(a32, a64) and np.array_equal(b32, b64), (name, what)
        assert np.isfinite(Q32).all() and np.isfinite(Q64).all() and (b64 > 0).all()
        # 2. column 0
        assert np.array_equal(Q32[0], Q64[0].astype(np.float32).astype(np.float64)), (name, what)
        # 3. columns j >= 1
        worst = {"edge": 0.0, "none": 0.0, "none/single": 0.0, "fp32": 0.0}
        for j in range(1, k):
            d = np.abs(Q32[j] - Q64[j])
            single = U32 * (1 + 2.0 ** -20) * np.abs(Q64[j]) + SUB32 / b64[j - 1]
            double = 2 * U32 * (1 + 2.0 ** -20) * np.abs(Q64[j]) + SUB32 / b64[j - 1]
            if live.any():
                worst["edge"] = max(worst["edge"], (d[live] / single[live]).max())
            if (~live).any():
                worst["none"] = max(worst["none"], (d[~live] / double[~live]).max())
                worst["none/single"] = max(worst["none/single"], (d[~live] / single[~live]).max())
            f = Q32[j] * b64[j - 1]
            r = np.abs(f - f.astype(np.float32).astype(np.float64))
            worst["fp32"] = max(worst["fp32"], (r / np.maximum(4 * U64 * np.abs(f), 1e-300)).max())
            assert (d[live] <= single[live]).all(), (name, what, j, "rows with an edge", (d[live] / single[live]).max())
            assert (d[~live] <= double[~live]).all(), (name, what, j, "rows without an edge", (d[~live] / double[~live]).max())
            assert (r <= 4 * U64 * np.abs(f)).all(), (name, what, j, "not an fp32 column")
        assert (Q32 != Q64).any(), (name, what)
        # 4. multout, before and after the fetch
        ref, S = _host_sums(t, Q32)
        ref2, S2 = _host_sums(t2, Q32)
        sub = SUB32 * float(np.abs(t[1:]) @ (1.0 / b64)) if k > 1 else 0.0
        sub2 = SUB32 * float(np.abs(t2[1:]) @ (1.0 / b64)) if k > 1 else 0.0
        E = np.where(live, (k + 4) * U64 * S, (U32 * (1 + 2.0 ** -20) + (k + 4) * U64) * S + sub)
        E2 = np.where(live, (k + 4) * U64 * S2, (U32 * (1 + 2.0 ** -20) + (k + 4) * U64) * S2 + sub2)
        ratios = {}
        for label, y, r_, e_ in (("before", y_before, ref, E), ("after", y_after, ref, E), ("second t", y2, ref2, E2)):
            dev = np.abs(y.astype(LD) - r_)
            ratios[label] = (float((dev[live] / e_[live]).max()) if live.any() else 0.0,
                             float((dev[~live] / e_[~live]).max()) if (~live).any() else 0.0)
            assert (dev <= e_).all(), (name, what, label, ratios[label])
        assert np.array_equal(y_before, y_after), (name, what)
        # multout_change
        assert c1 == 1.0
        own = float(np.linalg.norm(y2.astype(LD) - y_after.astype(LD)) / np.linalg.norm(y2.astype(LD)))
        host = float(np.linalg.norm(ref2 - ref) / np.linalg.norm(ref2))
        tol = 1e-9 * max(c2, 1e-6)
        e1n, e2n = (float(np.linalg.norm(np.where(live, 0, e_))) for e_ in (E, E2))
        slack = (e1n + e2n + host * e2n) / (float(np.linalg.norm(ref2)) - e2n)
        assert abs(c2 - own) <= tol, (name, what, c2, own)
        assert abs(c2 - host) <= tol + slack, (name, what, c2, host, slack)
        print(f"{name} {what}: |Q32 - Q64| / bound: rows with an edge {worst['edge']:.3f}, without {worst['none']:.3f} (of the two-rounding bound; "
              f"{worst['none/single']:.3f} of the single-rounding one); fp32-ness {worst['fp32']:.3f} of 4 ulp; multout / bound (with, without an "
              f"edge): before the fetch {ratios['before'][0]:.3f}, {ratios['before'][1]:.3f}; after {ratios['after'][0]:.3f}, {ratios['after'][1]:.3f}; "
              f"multout_change {c2:.6e}: own vectors {abs(c2 - own):.1e}, host sums {abs(c2 - host):.1e} (tolerance {tol:.1e} + {slack:.1e})")

        # 1 again: the same decomposition in chunks -- every prefix fetched on the way, basis included, bit for bit
        assert h32.prepare(x0, k) == xn64
        done = 0
        for steps in CHUNKS:
            if done == k:
                break
            ran = h32.run_steps(steps)
            assert ran == min(steps, k - done), (name, what, steps, ran)
            done += ran
            a, b, Q = h32.fetch(done)
            assert np.array_equal(a, a32[:done]) and np.array_equal(b, b32[:done - 1]) and np.array_equal(Q, Q32[:done]), (name, what, done)
        assert done == k
        assert np.array_equal(h32.multout(t), y_after), (name, what)
        return pb32
    finally:
        h64.close()
        h32.close()


@pytest.mark.parametrize("name", list(GRAPHS))
def test_basis_fp32_entry_by_entry(pkg, oracle, name):
    """basis_fp32 against the fp64 engine of the same mode (see _check_basis_fp32 for the bounds and their derivation).
    Modes: the plain SpMV (basis_fp32 selects the lazy loop there, so the fp64 engine beside it is given lazy_normalisation = 1:
    without it one GPU in plain mode runs the reference's operation order and its alpha / beta are other bits); the blocked
    SpMV with a hub of 64 wherever the blocked passes engage; three in-process ranks on the two larger graphs."""
    rp, ci = GRAPHS[name](oracle)
    n = len(rp) - 1
    _check_basis_fp32(name, rp, ci, lambda f: _One(pkg, propagation_blocking=0, lazy_normalisation=1, basis_fp32=f), "plain")
    probe = _One(pkg, propagation_blocking=1, hub_entries=64)
    engaged = probe.set_graph(rp, ci) > 0
    probe.close()
    # lzx_graph_prepare's rule (restated in test_gpu_forms.py: will_engage): hub = min(64, n) & ~1 columns are staged, and the
    # blocked passes engage iff hub < n and more vertices than that have an edge -- every graph here but the path of 2
    hub = min(64, n) & ~1
    assert engaged == (hub < n and int((np.diff(rp.astype(np.int64)) > 0).sum()) > hub), (name, "blocked passes")
    if engaged:
        assert _check_basis_fp32(name, rp, ci, lambda f: _One(pkg, propagation_blocking=1, hub_entries=64, basis_fp32=f), "blocked") > 0
    if name in GROUPS_ON:
        _check_basis_fp32(name, rp, ci, lambda f: _Three(pkg, basis_fp32=f), "three ranks")


def _group(pkg, rp, ci, **options):
    """Three in-process ranks; two where three are refused (printed)."""
    for world in (3, 2):
        grp = pkg.LocalGroup([0] * world, **options)
        try:
            grp.set_graph_csr(rp, ci)
            return grp, world
        except pkg.LzxError as e:
            grp.close()
            if world == 2:
                raise
            print(f"three ranks refused at n = {len(rp) - 1} ({e}): two")


@pytest.mark.parametrize("n", PATHS_EXCHANGE)
def test_exchange_fp32_against_the_loop_model(pkg, n):
    """exchange_fp32 = 1 on in-process ranks against lazy_loop_model(round_exchange=True); the fp64 exchange of the same group
    against the unrounded model.

    1. alpha_0, beta_0 at TOL_FIRST, alpha_1, beta_1 at TOL_SECOND (test_fp32_model_host.py: the project's first-coefficient
       tolerances, the second pair ten times tighter so that the two models stay 30 tolerances apart on every input).  By the
       triangle inequality the fp32 group is then at least 29 tolerances from the UNROUNDED model (asserted: a rank that
       multiplied its own slice unrounded, or rounded a wrong prefix, lands between the two).
    2. With m_0 = Q[0] and m_j = f32(beta_{j-1} Q[j]) (the model's midpoint margin makes this the vector that was multiplied,
       in every entry), A m_j / beta_{j-1} - alpha_j Q[j] - beta_{j-1} Q[j-1] - beta_j Q[j+1] <= 1e-12 * scale for j < 5:
       check_recurrence's bound (tests/test_gpu_parity.py), scale = max |alpha|, |beta|.  The same residual with the unrounded
       beta_{j-1} Q[j] must exceed 100 bounds in some column j >= 1, or the check could not see the rounding.  No entry is
       excluded.  The fp64 group meets the bound with the unrounded vector."""
    rp, ci = path_csr(n)
    x0 = start_vector(n)
    k = K_EXCHANGE
    for mode in (dict(propagation_blocking=0), dict(propagation_blocking=1, hub_entries=64)):
        for fp32 in (0, 1):
            grp, world = _group(pkg, rp, ci, exchange_fp32=fp32, **mode)
            try:
                engaged = max(e.info()["pb_entries"] for e in grp.engines) > 0
                if mode["propagation_blocking"] and not engaged:
                    print(f"path of {n}: the blocked passes do not engage on {world} ranks")
                    continue
                a, b, Q, xn, st = grp.lanczos(x0, k)
            finally:
                grp.close()
            assert st["iters"] == k and np.isfinite(Q).all()
            am, bm, _, _, xm = models(n)[fp32]
            assert abs(xn - float(xm)) <= 4 * n * U64 * xn          # one left-to-right fp64 sum of n squares, then a root
            d = coefficient_distances(a, b, am, bm)
            other = coefficient_distances(a, b, *models(n)[1 - fp32][:2])
            scale = max(np.abs(a).max(), np.abs(b).max())
            res, res_unrounded = [], []
            for j in range(k - 1):
                uj = Q[j] if j == 0 else b[j - 1] * Q[j]
                bj = 1.0 if j == 0 else b[j - 1]
                tail = a[j] * Q[j].astype(LD) + b[j] * Q[j + 1].astype(LD) + (b[j - 1] * Q[j - 1].astype(LD) if j else 0)
                res_unrounded.append(float(np.abs(matvec_ld(rp, ci, uj) / bj - tail).max()))
                mj = uj if j == 0 else uj.astype(np.float32).astype(np.float64)
                res.append(float(np.abs(matvec_ld(rp, ci, mj) / bj - tail).max()))
            print(f"path of {n}, {world} ranks, {mode}, exchange_fp32 = {fp32}: distance to the {'rounded' if fp32 else 'unrounded'} model: alpha_0 {d[0]:.1e}, "
                  f"beta_0 {d[1]:.1e} (tolerance {TOL_FIRST:.0e}), alpha_1 {d[2]:.1e}, beta_1 {d[3]:.1e} (tolerance {TOL_SECOND:.0e}); to the other model: "
                  f"alpha_1 {other[2]:.1e}, beta_1 {other[3]:.1e}; recurrence residual / scale: with the multiplied vector {max(res) / scale:.1e}, "
                  f"with the unrounded one {max(res_unrounded[1:]) / scale:.1e} (bound 1e-12)")
            assert d[0] <= TOL_FIRST and d[1] <= TOL_FIRST and d[2] <= TOL_SECOND and d[3] <= TOL_SECOND, (n, mode, fp32, d)
            assert other[2] >= (DISCRIMINATION - 1) * TOL_SECOND and other[3] >= (DISCRIMINATION - 1) * TOL_SECOND, (n, mode, fp32, other)
            if fp32:
                assert max(res) <= 1e-12 * scale, (n, mode, res)
                assert max(res_unrounded[1:]) > 100 * 1e-12 * scale, (n, mode, res_unrounded)
            else:
                assert max(res_unrounded) <= 1e-12 * scale, (n, mode, res_unrounded)
