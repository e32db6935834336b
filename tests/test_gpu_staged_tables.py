"""GPU: the other half of every SpMV -- spmv_body of csrc/lzx_spmv_body.h (k_spmv<0|1|2>, and the staged-columns workgroups of
the blocked SpMV's shared launch) -- at the counts where its table builder (lzx_graph_prepare steps 3 to 5) and its software
pipelines change behaviour, against the host model of the table formation (tests/sell_model.py).

Per (graph, mode) cell: every read-only shape of the body and the split rows, info()["long_rows"] and info()["sell_padded"]
equal the model's; the SpMV is exact (np.array_equal with scipy's A @ x on ones, on integers of [1, 2^30] -- never 0, row sums
below 2^46 --, on the indicators of the columns at degree ranks hub - 1, hub, 0 and n_active - 1 and of the two staged slots
that the clamped staging loads rewrite) under A, under L and under A again; in plain mode the body rows are also bit-exact on
a random fp64 x against a left-to-right host sum in the caller's column order.  alpha from every path: the start of the Lanczos
loop (which launches with live_rows_only) from three starts against np.longdouble.  The modes are a seeded, greedily generated
pairwise covering set over nine hooks (asserted) behind hand-picked anchors.  In-process groups of 2 and 3 ranks repeat the
counts per rank and the exact SpMV.  The last test reads from the MODEL what the cells reached and fails unless every line of
the coverage table ("what the tests pin") holds.

Where the model stands on what the code does:
  * info()["sell_padded"] is sell_elems + long_elems (lzx_get_graph_info): body_entries + split_entries, restated as that sum.
  * "n_long64 capped by n_loc_pad": min(round_up(n_long, 64), n_loc_pad) never cuts (n_loc_pad is a multiple of 64 and
    n_long <= n_loc_pad); the line is read as the rounding REACHING n_loc_pad with padding rows among the split rows.
  * item_len: lzx_graph_prepare takes any positive cap (item_cap = item_opt) and nothing but the builder and spmv_body reads the
    items (32-bit lengths, 64-bit offsets), so caps of 4096 and 8192 are legal: they are in the anchors.
  * a wavefront with >= 129 slices in the general loop needs 16 * 129 slices = 132 096 rows at the smallest grid: the graph
    `ring` has that many vertices (two entries each), more than the other graphs' 70 000.
  * staged_x_stride, info()["exchange_slice"] and info()["exchange_chunk0"] follow sell_model.exchange(): one chunk (the stride is
    the rank's slice) unless the handle blocks on several ranks and an eighth of the slice, at least the staged slots' share,
    rounded up to the column band, is below the slice.  At one rank the stride is the padded rows.
  * no cell is skipped: the only combination the code forbids is a PAIR of values (EXCLUDED), kept out of the generated modes, so
    "at most 10 % of the cells excluded" is asserted on the pairs, and the last test asserts that every generated cell ran.
  * propagation_blocking = 1 with hub_entries = 0 is no mode of its own (EXCLUDED).  A blocked mode on a graph with no more
    vertices with an edge than staged slots runs plain (lzx_graph_prepare: "every referenced column is staged"); such cells run
    and are held to the plain model.
"""
import random

import numpy as np
import pytest
import scipy.sparse as sp

import sell_model as sm
from test_gpu_forms import LAP, Graph

pytestmark = pytest.mark.gpu

DEFAULT = None        # hook left unset
HOOKS = {
    "propagation_blocking": [0, 1],
    "hub_entries": [0, 200, 1500, 16384],
    "long_row": [DEFAULT, 4, 16, "D-1", "D", "D+1"],      # D: a degree that occurs in the graph (Graph.D)
    "item_len": [DEFAULT, 4, 256, 1024],
    "narrow_slices": [0, 1, DEFAULT],
    "spmv_wgs": [1, 2, DEFAULT],
    "fuse_staged": [0, 1, DEFAULT],
    "defer_finish": [0, 1],
    "tie_sort": [0, 2],
}
# (hook, value, hook, value) pairs the code's own rules forbid, with the line the rule comes from
EXCLUDED = {
    ("propagation_blocking", 1, "hub_entries", 0): "lzx_graph.hip, lzx_graph_prepare: `if (hub == 0 || hub >= n) pb = false;` -- nothing staged, nothing to block",
}


def mode_of(**kw):
    m = dict(propagation_blocking=0, hub_entries=0, long_row=DEFAULT, item_len=DEFAULT, narrow_slices=DEFAULT, spmv_wgs=DEFAULT,
             fuse_staged=DEFAULT, defer_finish=1, tie_sort=0)
    m.update(kw)
    return m


# hand-picked modes ahead of the generated ones: coverage lines that need more than a pair of values, and item caps over 2048
ANCHORS = [
    mode_of(spmv_wgs=1),                                                                  # k_spmv<0>, one workgroup: most slices per wavefront
    mode_of(hub_entries=1500, spmv_wgs=1, item_len=4096),                                 # k_spmv<1>
    mode_of(hub_entries=16384, item_len=8192, spmv_wgs=2),
    mode_of(long_row=4, item_len=4, spmv_wgs=1, hub_entries=200),                         # most items per wavefront, plain
    mode_of(propagation_blocking=1, hub_entries=16384, item_len=4096, narrow_slices=1, spmv_wgs=1),
    mode_of(propagation_blocking=1, hub_entries=16384, item_len=8192, narrow_slices=0, spmv_wgs=1, fuse_staged=0, defer_finish=0),
    mode_of(propagation_blocking=1, hub_entries=16384, narrow_slices=1, fuse_staged=1, tie_sort=2),
    mode_of(propagation_blocking=1, hub_entries=200, long_row=4, item_len=4, narrow_slices=1, spmv_wgs=1),
    mode_of(propagation_blocking=1, hub_entries=1500, long_row=16, item_len=256, narrow_slices=1, spmv_wgs=2, fuse_staged=0),
    mode_of(propagation_blocking=1, hub_entries=200, narrow_slices=1, spmv_wgs=1, fuse_staged=1, defer_finish=0),
    mode_of(propagation_blocking=1, hub_entries=200, narrow_slices=1, spmv_wgs=1, fuse_staged=0, defer_finish=1),
    mode_of(propagation_blocking=1, hub_entries=1500, narrow_slices=1, fuse_staged=0, defer_finish=0),
    mode_of(propagation_blocking=1, hub_entries=1500, narrow_slices=1, fuse_staged=1, defer_finish=1),
    mode_of(hub_entries=200, defer_finish=0),
    mode_of(propagation_blocking=1, hub_entries=200, long_row=4, item_len=4, narrow_slices=1, spmv_wgs=2),   # `hubs_small`: 64 and 65 items per wavefront
    mode_of(hub_entries=200, spmv_wgs=2),                                                 # `classes`, plain: 80 items, 2 and 3 per wavefront
    mode_of(propagation_blocking=1, hub_entries=200, narrow_slices=1, spmv_wgs=2, fuse_staged=0, defer_finish=0),   # `classes`: 1 and 2 slices of 8 codes per wavefront
    mode_of(hub_entries=1500),                                                            # the Lanczos triple (plain, default grid, defer_finish 1)
]


def all_pairs():
    names = list(HOOKS)
    return {(a, va, b, vb) for i, a in enumerate(names) for b in names[i + 1:] for va in HOOKS[a] for vb in HOOKS[b]
            if (a, va, b, vb) not in EXCLUDED}


def pairs_of(mode):
    names = list(HOOKS)
    return {(a, mode[a], b, mode[b]) for i, a in enumerate(names) for b in names[i + 1:]}


def covering_set(seed=31337):
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
CHUNK = 6             # modes per test_cells case
GROUP_MODES = [       # several ranks: staged slots that 3 ranks do not divide (they are always even: 2 ranks divide them); 16384, 1502 and 206 leave 1, 2, 2
    mode_of(propagation_blocking=1, hub_entries=16384, narrow_slices=1, long_row=16, item_len=256),   # two-chunk exchange on `big`
    mode_of(propagation_blocking=1, hub_entries=1502, narrow_slices=0, fuse_staged=0, spmv_wgs=1),
    mode_of(hub_entries=206, long_row="D", item_len=4, spmv_wgs=2),
]


# ---- graphs: symmetric, without self-loops, built here ----------------------------------------------------------------
def sym_csr(n, src, dst):
    s, d = np.concatenate([src, dst]), np.concatenate([dst, src])
    keep = s != d
    A = sp.coo_matrix((np.ones(keep.sum()), (s[keep], d[keep])), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A.indptr.astype(np.uint64), A.indices.astype(np.uint32)


def joined(n, hn, degrees, spread=None):
    """vertices 0 .. hn - 1 are the hubs H; vertex hn + i is joined to degrees[i] consecutive hubs, from H[0] (or, with spread,
    from H[i % spread]).  A row's entries all lie in high-degree columns: with enough staged slots its staged count is its
    degree, so the degree ladder below is the ladder of slice widths and item lengths in plain AND in blocked mode."""
    degrees = np.asarray(degrees, dtype=np.int64)
    assert hn + len(degrees) <= n and degrees.max() <= hn
    row = np.repeat(hn + np.arange(len(degrees)), degrees)
    j = np.arange(degrees.sum()) - np.repeat(np.cumsum(degrees) - degrees, degrees)
    start = np.repeat(np.arange(len(degrees)) % spread, degrees) if spread else 0
    return sym_csr(n, row, (start + j) % hn)


LADDER_D = 40


def ladder_degrees():
    """every slice width 4 .. 84 (64 rows each, some of them one to three entries short: uneven slices), the default thresholds
    128 and 256 with one entry more, D - 1 .. D + 2, and item lengths around 64 and 256 packets"""
    deg = []
    for k in range(1, 22):
        deg += [4 * k] * 40 + [4 * k - 1] * 8 + [4 * k - 2] * 8 + [4 * k - 3] * 8
    deg += [128] * 3 + [129] * 2 + [130] + [256] * 2 + [257] * 2 + [252, 260, 1020, 1024, 1028]
    deg += [1, 2, 3, 5, 6, 7] * 150               # many narrow slices: the classes at a few per wavefront
    return deg


def ladder(tail):
    """degree ladder over 1028 hubs; `tail` = (vertices with an edge) % 64; 300 vertices without an edge"""
    deg = ladder_degrees()
    hn = 1028          # = the largest degree: every hub has an edge
    # the count of rows over D + 1 a multiple of 64, one row of D + 1 and 62 of D: n_long = 0, 1, 63 (mod 64) at long_row D + 1, D, D - 1
    deg = [d for d in deg if d not in (LADDER_D, LADDER_D + 1)]
    over = hn_over = None
    for fill in range(64):
        d2 = np.asarray(deg + [60] * fill + [LADDER_D + 1] + [LADDER_D] * 62)
        hub_deg = (d2[None, :] > np.arange(hn)[:, None]).sum(axis=1)
        over = int((d2 > LADDER_D + 1).sum() + (hub_deg > LADDER_D + 1).sum())
        if over % 64 == 0:
            deg = d2.tolist()
            break
    assert over % 64 == 0
    active = hn + len(deg)
    pad = (tail - active) % 64
    deg += [2] * pad
    n = hn + len(deg) + 300
    return joined(n, hn, deg)


def big():
    """60 580 rows of one to eight entries spread over 3900 hubs (1032 or 1033 slices: 64 and 65 per wavefront of ONE workgroup in
    the general loop, more than 64 in a class loop), rows of every item length around 1, 64, 64 IPF packets and of two and three items, 500 vertices without
    an edge.  More than 32 Ki vertices with an edge: two and three ranks take the two-chunk exchange."""
    hn = 3900
    deg = [252, 256, 260, 1020, 1024, 1028, 1920, 2044, 2048, 2052, 2944, 3900, 300, 257, 256, 129, 128, 100, 64]
    for k in range(1, 22):
        deg += [4 * k] * 64
    deg += ([1, 2, 3, 4] * 15045 + [5, 6, 7, 8] * 100)
    n = hn + len(deg) + 300
    return joined(n, hn, deg, spread=hn)


def ring():
    """C_n(+-1), n = 16 * 129 * 64 + 64: every row two entries, 2065 slices -- a wavefront of one workgroup takes >= 129 of them"""
    n = 16 * 129 * 64 + 64
    i = np.arange(n)
    return sym_csr(n, i, (i + 1) % n)


def dense_small():
    """C_258(+-1 .. +-8): every row 16 entries -- all of them split rows at a threshold below 16, the split rows reaching the padded
    rows, and no split row at all from 16 on; blocked with 200 staged slots only.  With items of 4 entries 1032 items: 64 and 65
    per wavefront of one workgroup."""
    n = 258
    i = np.arange(n)
    return sym_csr(n, np.concatenate([i] * 8), np.concatenate([(i + k) % n for k in range(1, 9)]))


def hubs_small():
    """332 rows of 16 entries over 16 hubs.  Blocked with 200 staged slots the hubs keep 184 entries each, whichever rows the order
    stages: with items of 4 entries 16 * 46 + 332 * 4 = 2064 items -- 64 and 65 per wavefront of two workgroups."""
    return joined(16 + 332, 16, [16] * 332)


def classes():
    """16 hubs, 3584 rows of 8 entries, 3584 of 4 and 2554 vertices without an edge: blocked with 200 staged slots (the hubs and 184
    rows) one wide slice, then 56 slices of 8 codes, 56 of 4 and 40 of none -- 3 and 4, 3 and 4, 2 and 3 per wavefront of one workgroup"""
    return joined(16 + 7168 + 48 + 39 * 64 + 10, 16, [8] * 3584 + [4] * 3584, spread=16)


GRAPHS = {          # name: (builder, D)
    "ladder_1": (lambda: ladder(1), LADDER_D),
    "big": (big, 8),
    "dense_small": (dense_small, 16),
    "ladder_0": (lambda: ladder(0), LADDER_D),
    "ladder_63": (lambda: ladder(63), LADDER_D),
    "ring": (ring, 2),
    "hubs_small": (hubs_small, 16),
    "classes": (classes, 8),
}
CELL_GRAPHS = ["ladder_1", "big", "dense_small"]              # every mode
EXTRA_CELLS = [("ring", 0), ("ring", 5), ("classes", 9), ("classes", 10), ("hubs_small", 14), ("hubs_small", 3), ("classes", 15), ("classes", 16), ("ring", 9)]   # ... and anchors on graphs built for them
LANCZOS_GRAPHS = ["ladder_0", "ladder_1", "ladder_63", "big"]
GROUP_GRAPHS = ["ladder_1", "big"]
_GRAPHS, _CELLS, _GROUP_CELLS, _LANCZOS, _GROUP_RUNS, _LANCZOS_RUNS = {}, {}, {}, {}, {}, {}


def graph(name):
    if name not in _GRAPHS:
        make, D = GRAPHS[name]
        rp, ci = make()
        g = Graph(name, rp, ci)
        g.D = D
        assert g.n <= 72000 or name == "ring"
        assert len(ci) <= 1500000 and (g.A != g.A.T).nnz == 0 and g.A.diagonal().sum() == 0, name
        assert (g.d == D).any(), name
        rng = np.random.default_rng(11)
        g.x_ones = np.ones(g.n)
        g.x_int = rng.integers(1, 2 ** 30 + 1, g.n).astype(np.float64)
        g.x_rand = rng.standard_normal(g.n)
        assert g.d.max() * 2.0 ** 30 < 2.0 ** 46
        # left-to-right row sums of x_rand in the caller's column order, for rows of at most 300 entries (the body rows of every
        # plain mode here: thresholds are at most 128)
        seq = np.zeros(g.n)
        for k in range(300):
            has = np.flatnonzero(g.d > k)
            if not len(has):
                break
            seq[has] += g.x_rand[g.ci64[g.rp64[has] + k]]
        g.seq_rand, g.seq_ok = seq, g.d <= 300
        _GRAPHS[name] = g
    return _GRAPHS[name]


def resolve(g, mode):
    """the mode's hook values on graph g: D resolved, unset hooks left out"""
    opts = {}
    for h, v in mode.items():
        if isinstance(v, str):
            v = g.D + {"D-1": -1, "D": 0, "D+1": 1}[v]
        if v is not DEFAULT:
            opts[h] = v
    return opts


def rank_of_ids(n, ids_per_rank):
    """degree rank of every vertex from the local row order of every rank: rank r is local row r // P of rank r % P"""
    P = len(ids_per_rank)
    rank_of = np.full(n, -1, dtype=np.int64)
    for p, ids in enumerate(ids_per_rank):
        rank_of[ids] = np.arange(len(ids)) * P + p
    assert (rank_of >= 0).all()
    return rank_of


SHAPES = ("split_rows", "split_items", "body_slices", "slices_wide", "slices_w8", "slices_w4", "slices_w0", "staged_workgroups",
          "split_entries", "body_entries", "live_rows", "staged_x_stride")


def model_of(g, opts, ids, rank_of, hub, world=1, rank=0):
    blocked, hub_model = sm.staging(g.n, g.n_active, opts.get("propagation_blocking", 0), opts["hub_entries"])
    assert hub == hub_model, ("staged slots: library", hub, "model", hub_model)
    t = sm.build(g.rp, g.ci, ids, rank_of, hub, blocked, g.n_active, world=world, rank=rank, long_row=opts.get("long_row"),
                 item_len=opts.get("item_len"), narrow_slices=opts.get("narrow_slices"), spmv_wgs=opts.get("spmv_wgs"))
    t.xs, t.xs0 = sm.exchange(g.n, g.n_active, world, opts.get("propagation_blocking", 0), opts["hub_entries"])
    return t


def check_counts(eng, t, what):
    gi = eng.info()
    got = {s: eng.shape(s) for s in SHAPES}
    want = dict(split_rows=t.n_long64, split_items=t.n_items, body_slices=t.n_slices, slices_wide=t.ns_wide, slices_w8=t.ns_w8,
                slices_w4=t.ns_w4, slices_w0=t.ns_w0, staged_workgroups=t.grid, split_entries=t.long_elems, body_entries=t.sell_elems,
                live_rows=t.rows_live, staged_x_stride=t.xs0)
    bad = {s: (got[s], want[s]) for s in SHAPES if got[s] != want[s]}
    assert not bad, (what, "shape: (library, model)", bad)
    assert (gi["long_rows"], gi["sell_padded"]) == (t.n_long, t.sell_padded), (what, "long_rows, sell_padded", gi["long_rows"], gi["sell_padded"],
                                                                             t.n_long, t.sell_padded)
    want_x = (t.xs if t.world > 1 else 0, t.xs0 if t.xs0 < t.xs else 0)      # lzx_get_graph_info: the slice with several ranks, chunk 0 when there are two
    assert (gi["exchange_slice"], gi["exchange_chunk0"]) == want_x, (what, "exchange_slice, exchange_chunk0", gi["exchange_slice"], gi["exchange_chunk0"], want_x)


def vectors(g, vertex_of_rank, hub):
    """[(name, x)]: ones, integers, the indicators of the boundary columns by degree rank"""
    xs = [("ones", g.x_ones), ("int", g.x_int)]
    ranks = {0, g.n_active - 1, hub} | ({hub - 1, hub - 2} if hub >= 2 else set())
    for r in sorted(r for r in ranks if 0 <= r < g.n):
        e = np.zeros(g.n)
        e[vertex_of_rank[r]] = 1.0
        xs.append((f"e_rank{r}", e))
    return xs


def check_spmv(g, spmv, set_operator, xs, what):
    """exact under A, under L, under A again"""
    refs = [g.once(("Ax", nm), lambda x=x: g.A @ x) if nm in ("ones", "int") else g.A @ x for nm, x in xs]
    assert np.array_equal(refs[0], g.d)
    for op in (0, LAP, 0):
        set_operator(op)
        for (nm, x), ax in zip(xs, refs):
            y, want = spmv(x), (g.d * x - ax if op else ax)
            bad = np.flatnonzero(y != want)
            assert len(bad) == 0, (what, "operator", op, "x", nm, len(bad), "rows", bad[:8], y[bad[:4]], want[bad[:4]])


def trips(p, ipf):
    """trips of the four-packet unrolled loop of an item of p packets, lane 0 and lane 63"""
    def lane(l):
        q, k = l + 64 * ipf, 0
        while q + 192 < p:
            q, k = q + 256, k + 1
        return k, q < p
    return lane(0), lane(63)


def reached(t, g, opts, shapes):
    """what the MODEL says this cell sits on: the raw material of the coverage table"""
    b = t.blocked
    ipf, gp = (8, 8) if b else (4, 4)
    degl = t.degl
    pk = sm.item_packets(t)
    c = sm.counts(t)
    st = sm.general_packets(t)
    upk = np.unique(pk).tolist()
    tr = [trips(p, ipf) for p in upk]
    over = np.flatnonzero(degl[:t.n_long] > t.thr)
    nolen = np.flatnonzero(degl[:t.n_long] == 0)
    last_len = [int(t.item_len[np.flatnonzero(t.item_row == r)[-1]]) for r in np.flatnonzero(t.row_items >= 2)[:4000]]
    r = dict(
        blocked=b, graph=g.name, opts=opts, thr=t.thr, hub=t.hub,
        thr_in_body=bool((degl[t.n_long64:t.n_loc_real] == t.thr).any()), thr1_split=bool((degl[:t.n_long] == t.thr + 1).any()),
        n_long_mod=t.n_long % 64 if t.n_long else None, reaches_pad=t.reaches_pad, no_body=t.n_long > 0 and t.n_slices == 0,
        no_items=t.n_items == 0 and t.n_slices > 0,
        empty_split_ahead=bool(len(nolen) and len(over) and nolen[0] < over[-1]),
        one_packet_split=bool(((degl[:t.n_long64] >= 1) & (degl[:t.n_long64] <= 4)).any()),
        row_items={min(int(v), 3) for v in np.unique(t.row_items) if v > 0},
        last_item_4=4 in last_len, last_item_cap=t.item_cap in last_len,
        item_pk={{1: "1", 63: "63", 64: "64", 65: "65", 64 * ipf - 1: "I-1", 64 * ipf: "I", 64 * ipf + 1: "I+1"}[p] for p in upk
                 if p in (1, 63, 64, 65, 64 * ipf - 1, 64 * ipf, 64 * ipf + 1)},
        item_mixed=any(a[0] > 0 and b_[0] == 0 and b_[1] for a, b_ in tr), item_trips=max([a[0] for a, _ in tr], default=0),
        wave_items={int(v) for v in np.unique(c["items"])}, wave_general={int(v) for v in np.unique(c["general"])},
        st={int(v) for v in np.unique(st)}, gp=gp, st_max=int(st.max()) if len(st) else 0, thr_width=sm.round_up(t.thr, 4) // 4,
        classes=t.classes, wave_w8={int(v) for v in np.unique(c["w8"])}, wave_w4={int(v) for v in np.unique(c["w4"])},
        wave_w0={int(v) for v in np.unique(c["w0"])}, ns=(t.ns_wide, t.ns_w8, t.ns_w4, t.ns_w0), n_slices=t.n_slices,
        narrow_general=bool(not t.classes and np.isin(st, (1, 2)).any()),
        uneven=bool(t.slice_uneven.any()), grid=t.grid, waves_over_units=t.waves > t.units, wgs=opts.get("spmv_wgs"),
        split_rows=t.n_long64, finish_launched=shapes["finish_launched"], pb_entries=shapes["pb_entries"],
        w0_beyond_live=sm.launch(t, True)[3] < t.ns_w0, fuse=opts.get("fuse_staged"),
    )
    return r


def run_cell(pkg, gname, mi):
    """One (graph, mode) cell: (label, reached or None, error or None)."""
    key = (gname, mi)
    if key in _CELLS:
        return _CELLS[key]
    g, mode = graph(gname), MODES[mi]
    opts = resolve(g, mode)
    label = f"{gname} MODES[{mi}] {opts}"
    rec, err = None, None
    eng = pkg.Engine(0, **opts)
    try:
        eng.set_graph_csr(g.rp, g.ci)
        gi = eng.info()
        sums, ids = eng.rank_row_sums()
        assert gi["world"] == 1 and gi["rows_local"] == g.n and np.array_equal(sums, g.d[ids]), (label, "row sums of x = 1")
        t = model_of(g, opts, ids, rank_of_ids(g.n, [ids]), gi["hub_entries"])
        rec = reached(t, g, opts, dict(finish_launched=eng.shape("finish_launched"), pb_entries=gi["pb_entries"]))
        rec["mode"] = mode
        check_counts(eng, t, label)
        check_spmv(g, eng.spmv, lambda op: eng.set_option("operator", op), vectors(g, ids, t.hub), label)
        if not t.blocked:      # body rows, random fp64 x: the left-to-right sum in the caller's column order, bit for bit
            y = eng.spmv(g.x_rand)
            body = ids[t.n_long64:]
            body = body[g.seq_ok[body]]
            bad = body[y[body] != g.seq_rand[body]]
            assert len(bad) == 0, (label, "body rows on a random x", len(bad), bad[:8], y[bad[:4]], g.seq_rand[bad[:4]])
            rec["rand_rows"] = len(body)
    except AssertionError as e:      # (an error of the library itself ends the test: nothing more is started on the device)
        err = f"{label}: {str(e)[:900]}"
    finally:
        eng.close()
    _CELLS[key] = (label, rec, err)
    return _CELLS[key]


def cell_list():
    return [(gn, mi) for gn in CELL_GRAPHS for mi in range(len(MODES))] + EXTRA_CELLS


# ---- the tests -----------------------------------------------------------------------------------------------------
def test_modes_cover_every_pair():
    """every legal pair of values of two different hooks occurs in at least one generated mode"""
    covered = set()
    for m in MODES:
        assert set(m) == set(HOOKS) and all(m[h] in HOOKS[h] or (h == "item_len" and m[h] in (4096, 8192)) for h in HOOKS), m
        assert not pairs_of(m) & set(EXCLUDED), m
        covered |= pairs_of(m)
    missing = all_pairs() - covered
    assert not missing, sorted(missing, key=str)[:10]
    assert MODES == covering_set(), "the set is not deterministic"
    n_all = len(all_pairs()) + len(EXCLUDED)
    assert len(EXCLUDED) * 10 <= n_all, "more than 10 % of the pairs excluded"
    print(f"{len(MODES)} modes ({len(ANCHORS)} hand-picked) cover {len(all_pairs())} pairs; {len(EXCLUDED)} excluded")


@pytest.mark.parametrize("gname,chunk", [(gn, c) for gn in CELL_GRAPHS for c in range((len(MODES) + CHUNK - 1) // CHUNK)] + [("extra", 0)])
def test_cells(pkg, gname, chunk):
    """counts against the model, exact SpMV under A, L, A; body rows on a random x in plain mode.  A failed cell does not hide the others."""
    mis = EXTRA_CELLS if gname == "extra" else [(gname, mi) for mi in range(chunk * CHUNK, min(len(MODES), (chunk + 1) * CHUNK))]
    failed = [err for err in (run_cell(pkg, gn, mi)[2] for gn, mi in mis) if err]
    assert not failed, f"{len(failed)} of {len(mis)} cells failed:\n" + "\n".join(failed)


def lanczos_modes():
    """the first mode of every (plain / blocked unfused / blocked fused) x (spmv_wgs 1 / default) x defer_finish triple"""
    seen = {}
    for mi, m in enumerate(MODES):
        form = "plain" if not m["propagation_blocking"] else "unfused" if m["fuse_staged"] == 0 else "fused"
        if m["spmv_wgs"] == 2 or isinstance(m["long_row"], str):
            continue
        seen.setdefault((form, m["spmv_wgs"], m["defer_finish"]), mi)
    return seen


def start_of_recurrence(g, x0, xn):
    """(alpha_0, beta_0, alpha_1) of A from q_0 = x0 / xn (the engine's own division), every sum in np.longdouble"""
    ld = np.longdouble
    q0 = (x0 / xn).astype(ld)
    w = g.matvec_ld(0, q0)
    a0 = np.sum(w * q0)
    r = w - a0 * q0
    b0 = np.sqrt(np.sum(r * r))
    q1 = r / b0
    w1 = g.matvec_ld(0, q1) - b0 * q0
    return float(a0), float(b0), float(np.sum(w1 * q1))


def boundary_rows(t, ids):
    """local rows: the last split row, the first body row, the first and last row of each class, the last live row"""
    rows = {t.n_long - 1, t.n_long64, t.rows_live - 1, min(t.n_loc_real, t.rows_live) - 1}
    for cls in (t.perm[:t.ns_wide], t.w8, t.w4, t.w0):
        if len(cls):
            rows |= {t.n_long64 + int(cls[0]) * 64, t.n_long64 + int(cls[-1]) * 64 + 63}
    return sorted(int(ids[r]) for r in rows if 0 <= r < t.n_loc_real)


def run_lanczos(pkg, gname):
    """the Lanczos cells of one graph, once per process: [failures]; fills _LANCZOS (what the coverage table reads)"""
    if gname in _LANCZOS_RUNS:
        return _LANCZOS_RUNS[gname]
    _LANCZOS_RUNS[gname] = ["did not finish"]
    g = graph(gname)
    modes = lanczos_modes()
    assert len(modes) == 12, sorted(modes, key=str)
    failed, worst = [], [0.0, 0.0, 0.0, 0.0]
    for triple, mi in sorted(modes.items(), key=str):
        opts = resolve(g, MODES[mi])
        eng = pkg.Engine(0, **opts)
        try:
            eng.set_graph_csr(g.rp, g.ci)
            ids = eng.rank_row_sums()[1]
            t = model_of(g, opts, ids, rank_of_ids(g.n, [ids]), eng.info()["hub_entries"])
            xb = np.zeros(g.n)
            rows = boundary_rows(t, ids)
            xb[rows] = 1.0 + np.arange(len(rows))
            cut, full = sm.launch(t, True), sm.launch(t, False)
            _LANCZOS[(gname, mi)] = dict(blocked=t.blocked, tail=g.n_active % 64, triple=triple, general_cut=cut[0] < full[0],
                                         w0_cut=t.blocked and t.classes and cut[3] < full[3], split=t.n_long64 > 0, defer=opts["defer_finish"])
            for nm, x0 in (("ones", g.x_ones), ("int", g.x_int), ("boundary", xb)):
                a, b, Q, xn, st = eng.lanczos(x0, 3, want_q=True)
                a0, b0, a1 = g.once(("start", nm if nm != "boundary" else tuple(rows), xn), lambda: start_of_recurrence(g, x0, xn))
                # (relative to the reference as check_leading_coefficients takes them; a reference of exactly 0 -- no two boundary
                #  rows adjacent -- asks for exactly 0)
                def rel(got, ref, scale):
                    return 0.0 if got == ref else abs(got - ref) / scale if scale else np.inf
                errs = [rel(a[0], a0, abs(a0)), rel(b[0], b0, abs(b0)), rel(a[1], a1, max(abs(a1), abs(a0)))]
                scale = max(np.abs(a).max(), np.abs(b).max())
                rec = 0.0
                for j in range(2):
                    r = g.A @ Q[j] - a[j] * Q[j] - b[j] * Q[j + 1] - (b[j - 1] * Q[j - 1] if j else 0.0)
                    rec = max(rec, np.abs(r).max() / scale)
                worst = [max(w, e) for w, e in zip(worst, errs + [rec])]
                assert st["iters"] == 3 and errs[0] <= 1e-12 and errs[1] <= 1e-12 and errs[2] <= 1e-10 and rec <= 1e-12, (nm, errs, rec)
        except AssertionError as e:      # (an error of the library itself ends the test: nothing more is started on the device)
            failed.append(f"{gname} MODES[{mi}] {triple}: {str(e)[:400]}")
        finally:
            eng.close()
    print(f"{gname}: {len(modes)} modes x 3 starts, largest errors alpha_0 {worst[0]:.1e} beta_0 {worst[1]:.1e} (1e-12) alpha_1 {worst[2]:.1e} (1e-10) "
          f"recurrence {worst[3]:.1e} (1e-12)")
    _LANCZOS_RUNS[gname] = failed
    return failed


@pytest.mark.parametrize("gname", LANCZOS_GRAPHS)
def test_alpha_from_every_path(pkg, gname):
    """alpha_0, beta_0 (1e-12) and alpha_1 (1e-10: test_gpu_parity.check_leading_coefficients) of lzx_lanczos_f64, k = 3, against
    np.longdouble, and the three-term recurrence of the fetched columns to 1e-12 ||T||, from three starts: ones, seeded integers,
    a vector supported on the boundary rows.  The loop launches with live_rows_only: the v . q partials of every loop of
    spmv_body (the NP = 0 class loop adds nothing) with the slices cut to the live rows.  Measured over the four graphs:
    alpha_0 2.4e-15, beta_0 5.4e-15, alpha_1 7.8e-15, recurrence 3.5e-14."""
    failed = run_lanczos(pkg, gname)
    assert not failed, "\n".join(failed)


def run_group(pkg, gname, world):
    """the several-rank cells of one graph and group size, once per process: [failures]; fills _GROUP_CELLS"""
    if (gname, world) in _GROUP_RUNS:
        return _GROUP_RUNS[(gname, world)]
    _GROUP_RUNS[(gname, world)] = ["did not finish"]
    g = graph(gname)
    failed = []
    for gi_, mode in enumerate(GROUP_MODES):
        opts = resolve(g, mode)
        if opts["hub_entries"] > g.n_active:
            opts["hub_entries"] = 500          # (cut to n_active & ~1 the slots might divide by the ranks; 500 does not divide by 3)
        label = f"{gname} world {world} GROUP_MODES[{gi_}]"
        grp = pkg.LocalGroup([0] * world, **opts)
        try:
            grp.set_graph_csr(g.rp, g.ci)
            ids = [e.rank_row_sums()[1] for e in grp.engines]
            rank_of = rank_of_ids(g.n, ids)
            hub = grp.engines[0].info()["hub_entries"]
            assert world == 2 or hub % world != 0, (label, hub)      # (staged slots are even: never at 2 ranks)
            stride = set()
            for p, e in enumerate(grp.engines):
                t = model_of(g, opts, ids[p], rank_of, e.info()["hub_entries"], world=world, rank=p)
                check_counts(e, t, f"{label} rank {p}")
                stride.add((t.xs0, t.xs, t.n_loc_pad, t.blocked))       # (check_counts held the library's stride to t.xs0)
            vertex_of_rank = np.argsort(rank_of)

            def set_op(op):
                for e in grp.engines:
                    e.set_option("operator", op)
            check_spmv(g, grp.spmv, set_op, vectors(g, vertex_of_rank, hub), label)
            _GROUP_CELLS[(gname, world, gi_)] = stride
        except AssertionError as e:      # (an error of the library itself ends the test: nothing more is started on the device)
            failed.append(f"{label}: {str(e)[:700]}")
        finally:
            grp.close()
    _GROUP_RUNS[(gname, world)] = failed
    return failed


@pytest.mark.parametrize("gname", GROUP_GRAPHS)
@pytest.mark.parametrize("world", [2, 3])
def test_several_ranks(pkg, gname, world):
    """in-process groups on one device: counts per rank against the model -- staged_x_stride and the exchange slice among them --
    and the exact SpMV: the strided staging index (i % world) * staged_x_stride + i / world, and on `big` the two-chunk exchange
    (staged_x_stride below the rank's slice)"""
    failed = run_group(pkg, gname, world)
    assert not failed, "\n".join(failed)


def same_bits(pkg, g, base, variants, world, what):
    """the SpMV of every variant returns the bits of `base` on the integer and indicator vectors"""
    def run(opts):
        h = pkg.LocalGroup([0] * world, **opts) if world > 1 else pkg.Engine(0, **opts)
        try:
            h.set_graph_csr(g.rp, g.ci)
            e0 = h.engines[0] if world > 1 else h
            hub = e0.info()["hub_entries"]
            engines = h.engines if world > 1 else [h]
            order = np.argsort(rank_of_ids(g.n, [e.rank_row_sums()[1] for e in engines]))      # the library's order, ties included
            return [h.spmv(x) for _, x in vectors(g, order, hub)], e0.debug, order
        finally:
            h.close()
    want, _, order = run(base)
    for extra in variants:
        got, dbg, order_v = run(dict(base, **extra))
        assert dbg, (what, extra, "not the debug library")
        assert np.array_equal(order, order_v), (what, extra, "the row order differs")
        for i, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), (what, extra, "vector", i, np.flatnonzero(a != b)[:8])


@pytest.mark.parametrize("world", [1, 3])
def test_stage_burst_returns_the_same_bits(pkg, world):
    """debug-only form (liblzx_dbg.so): stage_burst 2, 4, 8 -- the clamped staging loads, threads past the end rewriting the last
    pair -- with 2 staged slots (= 2 mod 2048, below 2048) and with 1502, blocked and plain"""
    g = graph("ladder_1")
    for hub in (2, 1502):
        for pb in (1, 0):
            same_bits(pkg, g, dict(propagation_blocking=pb, hub_entries=hub, stage_burst=0), [dict(stage_burst=b) for b in (2, 4, 8)], world,
                      f"hub {hub} pb {pb} world {world}")


def test_deep_pipeline_and_nt_loads_return_the_same_bits(pkg):
    """debug-only forms: spmv_deep = 1 (four register sets) and nt_index_loads = 1 on the graph with >= 65 slices per wavefront"""
    g = graph("big")
    base = dict(propagation_blocking=1, hub_entries=16384, narrow_slices=0, spmv_wgs=1, stage_burst=0)
    same_bits(pkg, g, base, [dict(spmv_deep=1), dict(nt_index_loads=1), dict(spmv_deep=1, nt_index_loads=1)], 1, "big")
    same_bits(pkg, g, dict(hub_entries=1500, spmv_wgs=1, stage_burst=0), [dict(nt_index_loads=1)], 1, "big plain")


def coverage_lines(cells, lanczos, groups):
    """{line: truth or the cells that reach it} from what the model recorded"""
    lines = {}
    for b, side in ((False, "plain"), (True, "blocked")):
        cs = [(lb, r) for lb, r in cells if r["blocked"] == b]
        ipf, gp = (8, 8) if b else (4, 4)

        def some(f):
            return [lb for lb, r in cs if f(r)]

        def union(field):
            return set().union(*[r[field] for _, r in cs]) if cs else set()

        L = {}
        L["a row of exactly thr entries in the body"] = some(lambda r: r["thr_in_body"])
        L["a row of thr + 1 entries split"] = some(lambda r: r["thr1_split"])
        L["both at once"] = some(lambda r: r["thr_in_body"] and r["thr1_split"])
        L["n_long = 0, 1, 63 (mod 64)"] = {0, 1, 63} <= {r["n_long_mod"] for _, r in cs}
        L["the split rows reach the padded rows"] = some(lambda r: r["reaches_pad"])
        L["body_slices == 0"] = some(lambda r: r["no_body"])
        L["split_items == 0"] = some(lambda r: r["no_items"])
        L["a row of 1, 2 and >= 3 items"] = {1, 2, 3} <= union("row_items")
        L["a last item of 4 entries"] = some(lambda r: r["last_item_4"])
        L["a last item of exactly item_cap"] = some(lambda r: r["last_item_cap"])
        L["item packets 1, 63, 64, 65, 64 IPF - 1, 64 IPF, 64 IPF + 1"] = {"1", "63", "64", "65", "I-1", "I", "I+1"} <= union("item_pk")
        L["an item: unrolled loop for low lanes, one-packet loop for high lanes"] = some(lambda r: r["item_mixed"])
        L["an item with >= 2 trips of the unrolled loop"] = some(lambda r: r["item_trips"] >= 2)
        L["items per wavefront 0, 1, 2, 3, 64, 65, >= 129"] = {0, 1, 2, 3, 64, 65} <= union("wave_items") and max(union("wave_items")) >= 129
        want_st = {1, 2, 3, 4} | set(range(5, 4 + gp + 1)) | {4 + gp + 1, 4 + 2 * gp}
        L[f"slice packets per lane {sorted(want_st)}"] = want_st <= union("st")
        L["a width-0 slice through the general loop"] = some(lambda r: 0 in r["st"])
        L["the widest slice the threshold allows"] = some(lambda r: r["st_max"] == r["thr_width"])
        L["slices per wavefront (general loop) 0, 1, 2, 3, 64, 65"] = {0, 1, 2, 3, 64, 65} <= union("wave_general")
        L["slices per wavefront (general loop) >= 129"] = max(union("wave_general"), default=0) >= 129
        L["staged_workgroups 1, 2"] = {1, 2} <= {r["grid"] for _, r in cs}
        L["default grid with more wavefronts than units"] = some(lambda r: r["wgs"] is None and r["waves_over_units"])
        L["hub_entries cut to n_active & ~1"] = some(lambda r: r["hub"] < min(r["opts"]["hub_entries"], 20000) & ~1 and r["hub"] > 0)
        if b:
            L["a split row without a staged entry ahead of one with items"] = some(lambda r: r["empty_split_ahead"])
            L["a split row of 1 - 4 staged entries"] = some(lambda r: r["one_packet_split"])
            for cls in ("w8", "w4", "w0"):
                L[f"{cls} per wavefront = 0, 1, 2, 3 (mod 4)"] = {0, 1, 2, 3} <= {v % 4 for v in union("wave_" + cls) if v > 0}
                i = ("w8", "w4", "w0").index(cls) + 1
                L[f"{cls} empty while another class is populated"] = some(lambda r: r["classes"] and r["ns"][i] == 0 and sum(r["ns"][1:]) > 0)
                L[f"{cls}: some wavefront takes none, others some"] = some(lambda r: 0 in r["wave_" + cls] and len(r["wave_" + cls]) > 1)
            L["a class with > 64 slices per wavefront"] = some(lambda r: max(max(r["wave_w8"]), max(r["wave_w4"]), max(r["wave_w0"])) > 64)
            L["width 4 and 8 slices through the general loop and through the class loops on one graph"] = bool(
                {r["graph"] for _, r in cs if r["narrow_general"]} & {r["graph"] for _, r in cs if r["classes"] and r["ns"][1] and r["ns"][2]})
            L["narrow_slices default below the size rule: no classes"] = some(lambda r: "narrow_slices" not in r["opts"] and not r["classes"] and r["n_slices"] > 0)
            L["padding codes read the zero slots (a slice whose rows differ in staged count)"] = some(lambda r: r["uneven"])
            L["staged slots < 1024, not a multiple of 1024, 16384"] = {200, 1500, 16384} <= {r["hub"] for _, r in cs}
            L["finish_launched 1 and 0 with split rows"] = {0, 1} <= {r["finish_launched"] for _, r in cs if r["split_rows"] and r["pb_entries"]}
            L["a width-0 class slice beyond the live rows"] = some(lambda r: r["w0_beyond_live"])
            L["staged workgroups in a launch of their own, ahead of and behind the scatter units"] = {0, 1, None} <= {r["fuse"] for _, r in cs if r["pb_entries"]}
        else:
            L["k_spmv<0> and k_spmv<1>"] = bool(some(lambda r: r["hub"] == 0)) and bool(some(lambda r: r["hub"] > 0))
            L["split_rows <= 256 and > 256 (k_long_finish's second block)"] = bool(some(lambda r: 0 < r["split_rows"] <= 256)) and bool(some(lambda r: r["split_rows"] > 256))
            L["body rows bit-exact on a random x"] = some(lambda r: r.get("rand_rows", 0) > 0)
        for k, v in L.items():
            lines[f"{side}: {k}"] = v
    for h, values in HOOKS.items():
        for v in values:
            on = {r["graph"] for _, r in cells if r["mode"][h] == v}
            lines[f"{h} = {v} on two graphs"] = len(on) >= 2
    lz = list(lanczos.values())
    for tail in (0, 1, 63):
        lines[f"Lanczos, n_active % 64 = {tail}: the live-slice cut of the general loop moves (a cell without classes)"] = any(
            c["tail"] == tail and c["general_cut"] for c in lz)
        lines[f"Lanczos, n_active % 64 = {tail}: the ns_w0 prefix moves (a blocked cell with classes)"] = any(c["tail"] == tail and c["w0_cut"] for c in lz)
    lines["Lanczos: defer_finish 0 and 1 on blocked modes with split rows"] = {0, 1} <= {c["defer"] for c in lz if c["blocked"] and c["split"]}
    lines["several ranks: staged_x_stride below the rank's slice (two-chunk exchange) on a blocked rank"] = any(
        s < xs and blk for cell in groups.values() for s, xs, pad, blk in cell)
    lines["several ranks: a slice below the padded rows (vertices without an edge)"] = any(xs < pad for cell in groups.values() for s, xs, pad, blk in cell)
    return lines


def test_coverage_table(pkg):
    """What the cells that ran reached, as the model sees it: conditions, not measurements.  Every line must hold."""
    cells = []
    for gn, mi in cell_list():
        label, r, _ = run_cell(pkg, gn, mi)
        if r is not None:
            cells.append((label, r))
    # the Lanczos and several-rank cells: run here unless their tests already ran in this process
    late = [f for gn in LANCZOS_GRAPHS for f in run_lanczos(pkg, gn)] + [f for gn in GROUP_GRAPHS for w in (2, 3) for f in run_group(pkg, gn, w)]
    assert not late, "\n".join(late)
    lines = coverage_lines(cells, _LANCZOS, _GROUP_CELLS)
    print(f"{len(cells)} cells of {len(cell_list())}, {len(MODES)} modes; blocked {sum(r['blocked'] for _, r in cells)}")
    for name, v in lines.items():
        print(f"  {'ok ' if v else 'MISSING'} {name}" + (f": {len(v)} cells, e.g. {v[0]}" if isinstance(v, list) and v else ""))
    missing = [name for name, v in lines.items() if not v]
    assert len(cells) == len(cell_list()), "a generated cell did not run to its model: none may be skipped"
    assert not missing, "coverage lines not reached:\n" + "\n".join(missing)
