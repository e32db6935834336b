"""GPU: the blocked SpMV of csrc/lzx_pb.hip at the counts where its table builder and its scatter kernel change behaviour,
against the host model of the table formation (tests/pb_model.py).

Per (graph, mode) cell: the library's counts -- info() pb_entries / pb_reduced_entries / pb_values and the shapes row_bands /
pb_runs / pb_steps / scatter_units -- equal the model's; the SpMV is exact (np.array_equal with scipy's A @ x on integer
vectors: ones, integers of [1, 2^30] -- never 0, row sums below 2^46 -- and the indicators of the boundary columns) under A,
under L and under A again; the start of the Lanczos loop under L is compared with its np.longdouble restatement on one mode
per (reduce on / off, defer_finish, fuse_staged) triple.  The modes are a seeded, greedily generated pairwise covering set
over thirteen hooks (asserted), behind seven hand-picked ones.  In-process groups of 2 and 3 ranks repeat the exact SpMV
with three modes.  The last test reads from the MODEL what the cells reached and fails unless every line of the coverage
table ("what the tests pin") holds: the graphs are built to sit on the boundaries, and this is where
that is asserted.

Where the model stands on the code and not on the issue text that asked for it: a blocked column's code is hub + position
(k_rank_maps) and the builder takes p = code - hub, so the column bands tile the POSITIONS (band = position // cb, the
staged positions included), not position - hub.  The boundary columns and the last-band conditions below are therefore in
positions: n_active % cb is 1 / cb - 1, and the whole layout in one band.

pb_unit: the smallest value pb_units handles without degenerate units is 1024 -- parts = ceil((512 S + 4 Q) / cap) is then
at most ceil(S / 2 + Q / 256) <= max(S, Q), so every unit gets a step or a quad; at 512 a band of one step and one quad is
cut into two units of which the first is empty.

No combination of the swept values is illegal at one rank.  (pb_carry_scan = 0 has no effect beside pb_column_band = 18432:
lzx_pb_launch's pick_scatter knows the 18 Ki band with the scan only.  The several-rank cells never use 18432:
csrc/lzx_test_hooks.h, "18432: the last on one rank only".)"""
import random
import time

import numpy as np
import pytest
import scipy.sparse as sp

import pb_model as pm
from test_gpu_forms import LAP, Graph

pytestmark = pytest.mark.gpu

CHOSEN = "L"          # pb_reduce: a run length that occurs in the graph (cell: handed over with L and with L + 1)
DEFAULT = None        # hook left unset

HOOKS = {
    "pb_reduce": [0, 2, 16, CHOSEN, 384, 1500],
    "pb_run_align": [4, 8, 16],
    "pb_taper": [0, 1],
    "pb_unit": [1024, 4096, 65536],
    "pb_target": [1024, 2048, DEFAULT],
    "pb_column_band": [8192, 16384, 18432],
    "pb_carry_scan": [0, 1],
    "fuse_staged": [0, 1],
    "defer_finish": [0, 1],
    "pb_scatter_nt": [0, 1],
    "pb_gather_nt": [0, 1],
    "item_len": [DEFAULT, 256],
    "hub_entries": [32, 512],
}
EXCLUDED = []         # (hook, value, hook, value) pairs the code's own rules forbid: none at one rank (module docstring)

# hand-picked modes ahead of the generated ones: coverage lines that need more than a pair of values
ANCHORS = [
    # a 16 Ki column band of the unstaged dominating rows (160 steps) in ONE unit of the doubled (tapered) size: 10 steps per wavefront
    dict(pb_reduce=384, pb_run_align=4, pb_taper=1, pb_unit=65536, pb_target=DEFAULT, pb_column_band=16384, pb_carry_scan=1,
         fuse_staged=0, defer_finish=1, pb_scatter_nt=0, pb_gather_nt=0, item_len=DEFAULT, hub_entries=32),
    # the same bands cut into units of 3 .. 5 steps per wavefront, carried through LDS
    dict(pb_reduce=384, pb_run_align=8, pb_taper=0, pb_unit=65536, pb_target=2048, pb_column_band=8192, pb_carry_scan=0,
         fuse_staged=1, defer_finish=0, pb_scatter_nt=1, pb_gather_nt=1, item_len=256, hub_entries=32),
    dict(pb_reduce=16, pb_run_align=16, pb_taper=1, pb_unit=4096, pb_target=1024, pb_column_band=8192, pb_carry_scan=1,
         fuse_staged=0, defer_finish=1, pb_scatter_nt=0, pb_gather_nt=1, item_len=DEFAULT, hub_entries=32),
    # every run plain, k_pb_finish always launched, staged columns in a launch of their own: with the next three: the Lanczos-start triples of pb_reduce = 0, which a pairwise set need not hold
    dict(pb_reduce=0, pb_run_align=4, pb_taper=0, pb_unit=1024, pb_target=1024, pb_column_band=18432, pb_carry_scan=1,
         fuse_staged=0, defer_finish=0, pb_scatter_nt=1, pb_gather_nt=0, item_len=256, hub_entries=512),
    dict(pb_reduce=0, pb_run_align=8, pb_taper=1, pb_unit=4096, pb_target=2048, pb_column_band=16384, pb_carry_scan=0,
         fuse_staged=0, defer_finish=1, pb_scatter_nt=0, pb_gather_nt=1, item_len=DEFAULT, hub_entries=32),
    dict(pb_reduce=0, pb_run_align=16, pb_taper=1, pb_unit=65536, pb_target=DEFAULT, pb_column_band=8192, pb_carry_scan=1,
         fuse_staged=1, defer_finish=0, pb_scatter_nt=0, pb_gather_nt=0, item_len=DEFAULT, hub_entries=512),
    dict(pb_reduce=0, pb_run_align=4, pb_taper=0, pb_unit=4096, pb_target=1024, pb_column_band=8192, pb_carry_scan=0,
         fuse_staged=1, defer_finish=1, pb_scatter_nt=1, pb_gather_nt=1, item_len=256, hub_entries=32),
]


def all_pairs():
    names = list(HOOKS)
    return {(a, va, b, vb) for i, a in enumerate(names) for b in names[i + 1:] for va in HOOKS[a] for vb in HOOKS[b]
            if (a, va, b, vb) not in EXCLUDED}


def pairs_of(mode):
    names = list(HOOKS)
    return {(a, mode[a], b, mode[b]) for i, a in enumerate(names) for b in names[i + 1:]}


def covering_set(seed=20240):
    """ANCHORS, then greedily: of 64 seeded random modes the one that covers most pairs not yet covered, until none is left."""
    rng = random.Random(seed)
    modes = [dict(m) for m in ANCHORS]
    todo = all_pairs()
    for m in modes:
        todo -= pairs_of(m)
    while todo:
        best, gain = None, -1
        for _ in range(64):
            cand = {h: rng.choice(v) for h, v in HOOKS.items()}
            if pairs_of(cand) & set(EXCLUDED):
                continue
            g = len(pairs_of(cand) & todo)
            if g > gain:
                best, gain = cand, g
        if gain > 0:
            modes.append(best)
            todo -= pairs_of(best)
    return modes


MODES = covering_set()
GROUP_MODES = [      # several ranks: never 18432; the first takes the two-chunk exchange where a rank's slice is wider than 16 Ki
    dict(pb_reduce=16, pb_column_band=8192, pb_unit=4096, pb_target=1024, hub_entries=32, pb_run_align=8),
    dict(pb_reduce=0, pb_column_band=16384, pb_taper=0, hub_entries=512, fuse_staged=0),
    dict(pb_reduce=384, pb_column_band=8192, pb_carry_scan=0, pb_unit=1024, hub_entries=32, defer_finish=0, item_len=256),
]


# ---- graphs: symmetric, built here, at most 33 000 vertices and 1.4 M entries ------------------------------------------
def sym_csr(n, src, dst):
    s, d = np.concatenate([src, dst]), np.concatenate([dst, src])
    keep = s != d
    A = sp.coo_matrix((np.ones(keep.sum()), (s[keep], d[keep])), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A.indptr.astype(np.uint64), A.indices.astype(np.uint32)


def circulant(O):
    """C_n(+-1, +-3000) with three star centres, n = 4 * 8192 + 1: every row has one or two entries per column band (steps of 512
    one-entry pieces), the last 8 Ki band holds ONE position, a last row band of one row, and a rank's slice of two is wider
    than 16 Ki (two-chunk exchange)."""
    n = 4 * 8192 + 1
    i = np.arange(n)
    src, dst = [i, i], [(i + 1) % n, (i + 3000) % n]
    for c in (5, 11000, 22000):
        leaves = i[i % 9 == c % 9]
        src.append(np.full(len(leaves), c))
        dst.append(leaves)
    return sym_csr(n, np.concatenate(src), np.concatenate(dst))


def dominating(O):
    """37 vertices joined to every vertex -- more than hub_entries = 32, so five are unstaged rows with a whole column band of
    entries each (16 steps of one piece per 8 Ki band, row bands of 16 rows, rep 64) -- over C_n(+-1, +-5000), n = 2 * 8192 - 1:
    the last referenced 8 Ki band holds cb - 1 positions."""
    n = 2 * 8192 - 1
    i = np.arange(n)
    src, dst = [i, i], [(i + 1) % n, (i + 5000) % n]
    for c in range(37):
        src.append(np.full(n, c))
        dst.append(i)
    return sym_csr(n, np.concatenate(src), np.concatenate(dst))


def ladder(O):
    """A degree ladder in a single (partial) column band, n = 8100: vertex a of block A is joined to the first a % 60 + 1
    vertices of block B, so the per-row entry counts and the run lengths take every small value; 520 vertices of degree
    140 fill the staged positions of either hub size."""
    n = 8100
    src, dst = [], []
    j = np.arange(140)
    for f in range(520):
        src.append(np.full(140, f))
        dst.append(1000 + (f * 53 + j * 17) % 7100)
    for a in range(240):
        k = a % 60 + 1
        src.append(np.full(k, 600 + a))
        dst.append(520 + np.arange(k))
    return sym_csr(n, np.concatenate(src), np.concatenate(dst))


GRAPHS = {
    "circulant": circulant,
    "dominating": dominating,
    "ladder": ladder,
    "rmat_s14": lambda O: O.gen_rmat(14, 12000, 200000, 7),     # irregular mixtures, vertices without an edge
}
_GRAPHS, _ORDER, _MODEL, _CELLS, _GROUP_CELLS = {}, {}, {}, {}, {}
_T0 = time.time()


def graph(O, name):
    if name not in _GRAPHS:
        rp, ci = GRAPHS[name](O)
        g = Graph(name, rp, ci)
        assert g.n <= 40000 and len(ci) <= 1500000
        assert (g.A != g.A.T).nnz == 0, name
        rng = np.random.default_rng(5)
        g.x_ones = np.ones(g.n)
        g.x_int = rng.integers(1, 2 ** 30 + 1, g.n).astype(np.float64)
        g.x0 = rng.standard_normal(g.n)
        assert g.d.max() * 2.0 ** 30 < 2.0 ** 46
        _GRAPHS[name] = g
    return _GRAPHS[name]


def model_args(mode, min_run):
    """the shape values of a mode as pb_model.build takes them (the builder's defaults where a hook is unset)"""
    return dict(cb=mode["pb_column_band"], min_run=min_run, run_align=mode.get("pb_run_align", pm.LZX_PB_ALIGN),
                unit_cap=mode.get("pb_unit"), taper=mode.get("pb_taper", 1) != 0, reduce=min_run is not None,
                target=mode.get("pb_target"))


def model(g, ids, hub, **args):
    """cached per (graph, order-relevant options = hub, shape values); the order itself is checked against the cache"""
    known = _ORDER.setdefault((g.name, hub), ids)
    assert np.array_equal(known, ids), (g.name, hub, "the row order changed between hand-overs")
    key = (g.name, hub) + tuple(sorted(args.items(), key=lambda kv: kv[0]))
    if key not in _MODEL:
        _MODEL[key] = pm.build(g.rp, g.ci, ids, hub, **args)
    return _MODEL[key]


def engine_options(mode, pb_reduce):
    opts = dict(propagation_blocking=1)
    for h, v in mode.items():
        if h == "pb_reduce":
            v = pb_reduce
        if v is not DEFAULT:
            opts[h] = v
    return opts


def boundary_columns(g, ids, hub, cb):
    """positions: first and last of the first band, the last staged and the first unstaged one, first and last of the last
    referenced band; as the caller's vertices"""
    last = g.n_active - 1
    pos = {0, min(cb - 1, last), hub - 1, hub, last // cb * cb, last}
    return sorted(int(ids[p]) for p in pos)


def check_spmv(g, spmv, set_operator, columns, what):
    """exact under A, under L, under A again"""
    xs = [("ones", g.x_ones), ("int", g.x_int)]
    for c in columns:
        e = np.zeros(g.n)
        e[c] = 1.0
        xs.append((f"e_{c}", e))
    refs = [g.A @ x for _, x in xs]
    assert np.array_equal(refs[0], g.d)
    for op in (0, LAP, 0):
        set_operator(op)
        for (nm, x), ax in zip(xs, refs):
            y, want = spmv(x), (g.d * x - ax if op else ax)
            bad = np.flatnonzero(y != want)
            assert len(bad) == 0, (what, "operator", op, "x", nm, "rows", bad[:8], y[bad[:4]], want[bad[:4]])


def reached(t, mode, shapes):
    """what the MODEL says this cell sits on: the raw material of the coverage table"""
    red, ln = t.run_reduced, t.run_len
    units = t.units
    r = dict(
        red_exact_min=bool(t.min_run is not None and (ln[red] == t.min_run).any()),
        plain_min_minus_1=bool(t.min_run is not None and (ln[~red] == t.min_run - 1).any()),
        red_mod_512={int(v) for v in np.unique(ln[red] % 512)},
        red_steps_max=int(t.run_steps.max()) if t.runs else 0,
        red_one_step=bool((t.run_steps[red] == 1).any()),
        planes={int(v) for v in np.unique(t.piece_plane)},
        lanes_2=bool((t.piece_lanes == 2).any()), lanes_max=int(t.piece_lanes.max()) if t.pieces else 0,
        steps_2=bool((t.row_steps == 2).any()), steps_max=int(t.row_steps.max()) if t.pieces else 0,
        step_pieces_max=int(t.step_pieces.max()) if t.steps else 0,
        lane_gaps=t.lane_gaps,
        plain_mod_4={(t.run_align, int(v)) for v in np.unique(ln[~red] % 4)},
        wave_steps=set().union(*[pm.wave_step_counts(S) for _, S, _ in units]) if units else set(),
        full_block=any(Q >= 256 for _, _, Q in units),
        tail_quads=set().union(*[pm.tail_quads(Q) for _, _, Q in units]) if units else set(),
        unit_no_steps=any(S == 0 and Q > 0 for _, S, Q in units), unit_no_quads=any(Q == 0 and S > 0 for _, S, Q in units),
        last_band=t.n_active % t.cb, single_band=t.nb == 1 and t.n_active < t.cb,
        band_rows={int(v) for v in np.unique(t.band_rows)},
        partial_last_row_band=int(t.band_rows[-1]) not in (1024, 512, 256, 128, 64, 32, 16),
        finish_launched=shapes["finish_launched"], finish_deferrable=shapes["finish_deferrable"],
        pb_entries=t.pb_entries, mode=mode,
    )
    return r


def run_cell(pkg, O, gname, mi):
    """One (graph, mode) cell: [(label, reached, error or None)] -- two hand-overs where pb_reduce is chosen from the data."""
    key = (gname, mi)
    if key in _CELLS:
        return _CELLS[key]
    g, mode = graph(O, gname), MODES[mi]
    out = []
    reduces = [mode["pb_reduce"]]
    if mode["pb_reduce"] == CHOSEN:
        # hand over once (reduced runs of the default length: the format does not enter the order), let the model list the run
        # lengths, take the most frequent length >= 2
        eng = pkg.Engine(0, **engine_options(mode, 1))
        try:
            eng.set_graph_csr(g.rp, g.ci)
            ids, hub = eng.rank_row_sums()[1], eng.info()["hub_entries"]
        finally:
            eng.close()
        t = model(g, ids, hub, **model_args(mode, pm.LZX_PBR_MIN_RUN))
        lens, cnt = np.unique(t.run_len[t.run_len >= 2], return_counts=True)
        L = int(lens[np.argmax(cnt)])
        reduces = [L, L + 1]
    for pb_reduce in reduces:
        label = f"{gname} MODES[{mi}] pb_reduce={pb_reduce}"
        rec, err = None, None
        eng = pkg.Engine(0, **engine_options(mode, pb_reduce))
        try:
            eng.set_graph_csr(g.rp, g.ci)
            gi = eng.info()
            sums, ids = eng.rank_row_sums()
            hub = gi["hub_entries"]
            assert hub == min(mode["hub_entries"], g.n_active) & ~1 and gi["world"] == 1 and gi["rows_local"] == g.n, (label, gi)
            assert np.array_equal(sums, g.d[ids]), label
            min_run = None if pb_reduce == 0 else pm.LZX_PBR_MIN_RUN if pb_reduce == 1 else pb_reduce
            t = model(g, ids, hub, **model_args(mode, min_run))
            shapes = {s: eng.shape(s) for s in ("row_bands", "pb_runs", "pb_steps", "scatter_units", "finish_launched", "finish_deferrable")}
            rec = reached(t, mode, shapes)
            got = (gi["pb_entries"], gi["pb_reduced_entries"], gi["pb_values"], shapes["row_bands"], shapes["pb_runs"],
                   shapes["pb_steps"], shapes["scatter_units"])
            want = (t.pb_entries, t.pb_reduced_entries, t.pb_values, t.row_bands, t.runs, t.steps, t.scatter_units)
            assert got == want, f"entries, reduced, values, row bands, runs, steps, units: library {got} model {want}"
            check_spmv(g, eng.spmv, lambda op: eng.set_option("operator", op), boundary_columns(g, ids, hub, t.cb), label)
        except (AssertionError, pkg.LzxError) as e:
            err = f"{label}: {str(e)[:700]}"
        finally:
            eng.close()
        out.append((label, rec, err))
    _CELLS[key] = out
    return out


# ---- the tests -----------------------------------------------------------------------------------------------------
def test_modes_cover_every_pair():
    """every pair of values of two different hooks occurs in at least one generated mode"""
    covered = set()
    for m in MODES:
        assert set(m) == set(HOOKS) and all(m[h] in HOOKS[h] for h in HOOKS), m
        covered |= pairs_of(m)
    missing = all_pairs() - covered
    assert not missing, sorted(missing, key=str)[:10]
    assert MODES == covering_set(), "the set is not deterministic"
    triples = {(m["pb_reduce"] != 0, m["defer_finish"], m["fuse_staged"]) for m in MODES}
    assert len(triples) == 8, triples     # test_lanczos_start: every (reduce on / off, defer_finish, fuse_staged)
    print(f"{len(MODES)} modes ({len(ANCHORS)} hand-picked) cover {len(all_pairs())} pairs")


@pytest.mark.parametrize("gname", list(GRAPHS))
def test_cells(pkg, oracle, gname):
    """every mode on one graph: counts against the model, exact SpMV under A, L, A.  A failed cell does not hide the others."""
    failed = []
    for mi in range(len(MODES)):
        failed += [err for _, _, err in run_cell(pkg, oracle, gname, mi) if err]
    n = sum(len(run_cell(pkg, oracle, gname, mi)) for mi in range(len(MODES)))
    print(f"{gname}: {n} cells [{time.time() - _T0:.0f} s]")
    assert not failed, f"{len(failed)} of {n} cells failed:\n" + "\n".join(failed)


@pytest.mark.parametrize("gname", list(GRAPHS))
def test_lanczos_start(pkg, oracle, gname):
    """alpha_0, beta_0 (1e-12) and alpha_1 (1e-10, test_gpu_laplacian's tolerances) of the loop under L from a random x0 against
    np.longdouble, on the first mode of every (reduce on / off, defer_finish, fuse_staged) triple: the fused v . q partials of
    multi-item bands and the k_pb_finish launch that the loop under L must not defer."""
    g = graph(oracle, gname)
    seen, failed, worst = set(), [], [0.0, 0.0, 0.0]
    for mi, mode in enumerate(MODES):
        triple = (mode["pb_reduce"] != 0, mode["defer_finish"], mode["fuse_staged"])
        if triple in seen:
            continue
        seen.add(triple)
        eng = pkg.Engine(0, **engine_options(mode, 1 if mode["pb_reduce"] == CHOSEN else mode["pb_reduce"]))
        try:
            eng.set_graph_csr(g.rp, g.ci)
            assert eng.info()["pb_entries"] > 0
            eng.set_option("operator", LAP)
            a, b, _, xn, st = eng.lanczos(g.x0, 3, want_q=False)
            a0, b0, a1 = g.once(("start", xn), lambda: g.lanczos_start(g.x0, xn))
            errs = [abs(a[0] - a0) / abs(a0), abs(b[0] - b0) / abs(b0), abs(a[1] - a1) / max(abs(a1), abs(a0))]
            worst = [max(w, e) for w, e in zip(worst, errs)]
            assert st["iters"] == 3 and errs[0] <= 1e-12 and errs[1] <= 1e-12 and errs[2] <= 1e-10, errs
        except (AssertionError, pkg.LzxError) as e:
            failed.append(f"{gname} MODES[{mi}] {triple}: {str(e)[:400]}")
        finally:
            eng.close()
    print(f"{gname}: {len(seen)} triples, largest errors alpha_0 {worst[0]:.1e} beta_0 {worst[1]:.1e} (1e-12) alpha_1 {worst[2]:.1e} (1e-10)")
    assert len(seen) == 8 and not failed, "\n".join(failed)


@pytest.mark.parametrize("gname", list(GRAPHS))
def test_several_ranks(pkg, oracle, gname):
    """in-process groups of 2 and 3 ranks on one device: the exact SpMV checks (the model's counts are for one rank)"""
    g = graph(oracle, gname)
    failed = []
    for w in (2, 3):
        for gi_, mode in enumerate(GROUP_MODES):
            label = f"{gname} world {w} GROUP_MODES[{gi_}]"
            grp = pkg.LocalGroup([0] * w, propagation_blocking=1, **mode)
            try:
                grp.set_graph_csr(g.rp, g.ci)
                infos = [e.info() for e in grp.engines]
                ids0 = np.arange(g.n)[np.argsort(-g.d, kind="stable")]     # boundary columns by degree rank: positions are per rank here
                hub = infos[0]["hub_entries"]
                cols = sorted({int(ids0[p]) for p in (0, hub - 1, hub, g.n_active - 1)})

                def set_op(op):
                    for e in grp.engines:
                        e.set_option("operator", op)
                check_spmv(g, grp.spmv, set_op, cols, label)
                _GROUP_CELLS[(gname, w, gi_)] = dict(chunk0=max(i["exchange_chunk0"] for i in infos), pb_entries=sum(i["pb_entries"] for i in infos))
            except (AssertionError, pkg.LzxError) as e:
                failed.append(f"{label}: {str(e)[:600]}")
            finally:
                grp.close()
    assert not failed, "\n".join(failed)


def test_coverage_table(pkg, oracle):
    """What the cells that ran reached, as the model sees it: conditions, not measurements.  Every line must hold."""
    cells = []
    for gname in GRAPHS:
        for mi in range(len(MODES)):
            cells += [(label, r) for label, r, _ in run_cell(pkg, oracle, gname, mi) if r is not None]
    live = [(lb, r) for lb, r in cells if r["pb_entries"] > 0]

    def some(f):
        return [lb for lb, r in live if f(r)]

    def union(field):
        return set().union(*[r[field] for _, r in live])

    lines = {
        "a reduced run of exactly min_run entries": some(lambda r: r["red_exact_min"]),
        "a plain run of min_run - 1 entries": some(lambda r: r["plain_min_minus_1"]),
        "reduced run lengths = 0, 1, 511 (mod 512)": {0, 1, 511} <= union("red_mod_512"),
        "a reduced run of one step": some(lambda r: r["red_one_step"]),
        "a reduced run of >= 16 steps": some(lambda r: r["red_steps_max"] >= 16),
        "a piece closing in each plane 0 .. 7": union("planes") == set(range(8)),
        "a row spanning exactly 2 lanes": some(lambda r: r["lanes_2"]),
        "a row spanning >= 3 lanes": some(lambda r: r["lanes_max"] >= 3),
        "a row spanning exactly 2 steps": some(lambda r: r["steps_2"]),
        "a row spanning >= 3 steps": some(lambda r: r["steps_max"] >= 3),
        "a step of 512 pieces": some(lambda r: r["step_pieces_max"] == 512),
        "a lane without a piece end between two that hold one": some(lambda r: r["lane_gaps"] > 0),
        "plain run lengths = 0 .. 3 (mod 4) under each alignment": {(a, m) for a in (4, 8, 16) for m in range(4)} <= union("plain_mod_4"),
        "wavefronts with 0, 1, 2, 3, 4, 5 steps": set(range(6)) <= union("wave_steps"),
        "a wavefront with >= 8 steps": max(union("wave_steps")) >= 8,
        "a full 256-quad block": some(lambda r: r["full_block"]),
        "a last block with 1, 2 and 3 quads for some lane": {1, 2, 3} <= union("tail_quads"),
        "a unit without reduced steps": some(lambda r: r["unit_no_steps"]),
        "a unit without quads": some(lambda r: r["unit_no_quads"]),
        "a last column band of 1 position": some(lambda r: r["last_band"] == 1),
        "a last column band of cb - 1 positions": some(lambda r: r["last_band"] == r["mode"]["pb_column_band"] - 1),
        "the whole layout in one (partial) band": some(lambda r: r["single_band"]),
        "a row band of 1024 rows": some(lambda r: 1024 in r["band_rows"]),
        "a row band of 16 rows (rep 64)": some(lambda r: 16 in r["band_rows"] and r["mode"]["pb_reduce"] != 0),
        "a partial last row band": some(lambda r: r["partial_last_row_band"]),
        "finish_launched = 1": some(lambda r: r["finish_launched"] == 1),
        "finish_launched = 0": some(lambda r: r["finish_launched"] == 0),
        "finish_deferrable = 1": some(lambda r: r["finish_deferrable"] == 1),
    }
    for h, values in HOOKS.items():
        for v in values:
            on = {lb.split()[0] for lb, r in live if r["mode"][h] == v}
            lines[f"{h} = {v} on two graphs with blocked entries"] = len(on) >= 2
    if _GROUP_CELLS:      # (filled by test_several_ranks; absent when this test is run alone)
        lines["a several-rank cell with the two-chunk exchange"] = any(c["chunk0"] > 0 and c["pb_entries"] > 0 for c in _GROUP_CELLS.values())
    print(f"{len(cells)} cells, {len(MODES)} modes")
    print("reached: reduced run <= %d steps, row across <= %d lanes / %d steps, step of <= %d pieces, wavefront <= %d steps" % (
        max(r["red_steps_max"] for _, r in live), max(r["lanes_max"] for _, r in live), max(r["steps_max"] for _, r in live),
        max(r["step_pieces_max"] for _, r in live), max(union("wave_steps"))))
    for name, v in lines.items():
        print(f"  {'ok ' if v else 'MISSING'} {name}" + (f": {len(v)} cells, e.g. {v[0]}" if isinstance(v, list) and v else ""))
    missing = [name for name, v in lines.items() if not v]
    assert not missing, "coverage lines not reached:\n" + "\n".join(missing)
