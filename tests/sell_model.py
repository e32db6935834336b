"""Host model of the table formation of the SpMV's other half -- the sliced-ELL body and the split rows that spmv_body
(csrc/lzx_spmv_body.h) takes: lzx_graph_prepare steps 3 to 5 of csrc/lzx_graph.hip (their arithmetic: csrc/lzx_prepare_plan.h, which
tests/test_prepare_plan_host.py runs on a CPU against this model) -- in numpy.  No GPU and no import of the
package: the tests hand it the CSR, the row order the library chose and the shape values, and compare what it counts with
what the library reports (tests/test_gpu_staged_tables.py), or with numbers counted by hand (tests/test_sell_model_host.py).

What is taken as given: the ORDER -- rank_of[v] = degree rank of the caller's vertex v, from Engine.rank_row_sums() of every
rank (with P ranks, rank r is local row r // P of rank r % P) -- and hub = info()["hub_entries"].  Neither the degree sort nor
the tie_sort re-ranking is restated.

What is restated, per rank:
  mode         staging() -- whether the handle blocks, and how many slots it stages, from the two options and the graph's size.
  degl         per local row: its degree (plain mode), or the number of its entries whose column's degree rank is below hub
               (blocked mode: the tables hold staged columns only).
  threshold    long_row if set, else 128 (plain), 256 (blocked), 1024 (blocked from 2 Mi live rows per rank).
  split rows   n_long = 1 + the index of the LAST row over the threshold (blocked: degl is not monotone, rows before it with
               fewer staged entries are split rows too); n_long64 = min(round_up(n_long, 64), n_loc_pad).
  items        per split row ceil(round_up(degl, 4) / item_cap) of item_cap entries, the last one shorter; none at degl = 0.
  slices       64 rows each behind the split rows; width round_up(max degl in the slice, 4).
  classes      blocked, narrow_slices != 0, and narrow_slices > 0 or n_slices >= 8 CUs 16: wide (> 8), 8, 4, 0 -- the processing
               order is the wide ones as they lie, then each class.
  exchange     exchange() -- a rank's slice xs of the exchange layout and the stride xs0 of its chunk 0 (staged_x_stride).
  grid         step 5: CUs x (1 blocked | 4 plain) workgroups, at most one wavefront per unit, halved below CUs 512 units in
               blocked mode, capped by spmv_wgs.
  dealing      unit i of wavefront w of the 16 grid wavefronts is w + i waves: how many items, general-loop slices and class
               slices a wavefront takes (counts()), and their packets per lane (len / 4, width / 4).
"""
import numpy as np

LZX_SLICE = 64
LZX_LONG_ROW = 128
LZX_ITEM = 2048
LZX_TAIL = 64
LZX_PB_CB = 16384       # column band of the blocked passes; 18432 for a layout of x beyond 16 MiB unless a band is forced
LZX_PB_CB_WIDE = 18432
WAVES_PER_WG = 16       # LZX_SPMV_BLOCK / 64
CU_COUNT = 256          # MI355X
PF = 4                  # packets of a slice fetched ahead of its summation


def round_up(a, m):
    return (a + m - 1) // m * m


def staging(n, n_active, propagation_blocking, hub_entries):
    """(blocked, hub_real): lzx_graph_prepare before step 1 and behind the count of vertices with an edge.  hub_entries is the
    option as set (the data-dependent default of an unset option is not restated)."""
    pb = propagation_blocking > 0
    hub = min(hub_entries, n, 20000) & ~1
    if hub == 0 or hub >= n:
        pb = False
    if hub > n_active:
        hub = n_active & ~1
        if hub == 0:
            pb = False
    if hub >= n_active:
        pb = False
    return pb, hub


def exchange(n, n_active, world, propagation_blocking, hub_entries, column_band=None, overlap=True):
    """(xs, xs0): a rank's slice of the exchange layout and the stride of its chunk 0 -- the value staged for degree rank r is read at
    (r % world) * xs0 + r // world.  One rank: both are the padded rows.  Several ranks: xs covers the vertices with an edge;
    the two-chunk exchange (blocked mode, overlap wanted: the default of an in-process group) cuts chunk 0 to the first eighth
    of the slice, at least the staged slots' share, rounded up to the column band -- taken only if that is below xs, with the
    slots as they stand BEFORE the cut to the vertices with an edge, and given up when the handle does not block after it."""
    n_loc_pad = round_up((n + world - 1) // world, LZX_SLICE)
    xs, xlen = n_loc_pad, world * n_loc_pad + LZX_TAIL
    if world > 1:
        xs = min(max(LZX_SLICE, round_up((n_active + world - 1) // world, LZX_SLICE)), n_loc_pad)
        xlen = world * xs + LZX_TAIL
    pb = propagation_blocking > 0
    hub = min(hub_entries, n, 20000) & ~1
    if hub == 0 or hub >= n:
        pb = False
    xs0 = xs
    if world > 1 and pb and overlap:
        band = LZX_PB_CB if column_band in (8192, 16384) or xlen * 8 <= (16 << 20) else LZX_PB_CB_WIDE
        x0 = round_up(max(xs // 8, (hub + world - 1) // world), band)
        if x0 < xs:
            xs0 = x0
    if not staging(n, n_active, propagation_blocking, hub_entries)[0]:
        xs0 = xs
    return xs, xs0


def dealt(units, waves):
    """how many of `units` round-robin units each of `waves` wavefronts takes"""
    w = np.arange(waves)
    return np.where(units > w, (units - w + waves - 1) // waves, 0).astype(np.int64)


class Tables:
    pass


def build(rp, ci, ids, rank_of, hub, blocked, n_active, world=1, rank=0, long_row=None, item_len=None, narrow_slices=None,
          spmv_wgs=None, cus=CU_COUNT):
    """ids[l] = the caller's vertex of local row l of this rank; rank_of[v] = degree rank of vertex v (all ranks)."""
    rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    n = len(rp) - 1
    t = Tables()
    t.blocked, t.hub, t.world = blocked, hub, world
    t.n_loc_pad = round_up((n + world - 1) // world, LZX_SLICE)
    t.n_loc_real = (n - rank + world - 1) // world if rank < n else 0
    assert len(ids) == t.n_loc_real
    live = (n_active - rank + world - 1) // world if n_active > rank else 0
    t.rows_live = min(t.n_loc_pad, round_up(live, LZX_SLICE))
    ids = np.asarray(ids, dtype=np.int64)
    deg = (rp[1:] - rp[:-1])[ids]
    degl = np.zeros(t.n_loc_pad, dtype=np.int64)
    if blocked:
        staged = np.concatenate([[0], np.cumsum(np.asarray(rank_of)[ci] < hub)])
        degl[:t.n_loc_real] = staged[rp[1:][ids]] - staged[rp[:-1][ids]]
    else:
        degl[:t.n_loc_real] = deg
    t.degl, t.deg = degl, deg
    # the split threshold
    if long_row is not None and long_row > 0:
        t.thr = long_row
    elif blocked:
        t.thr = 8 * LZX_LONG_ROW if t.rows_live >= (1 << 21) else 2 * LZX_LONG_ROW
    else:
        t.thr = LZX_LONG_ROW
    over = np.flatnonzero(degl[:t.n_loc_real] > t.thr)
    t.n_long = int(over[-1]) + 1 if len(over) else 0
    t.n_long64 = min(round_up(t.n_long, LZX_SLICE), t.n_loc_pad)
    # (n_loc_pad is a multiple of 64 and n_long <= n_loc_real <= n_loc_pad, so the min never cuts: what can happen is that the
    #  rounding reaches the padded rows -- every row a split row, padding rows among them)
    t.reaches_pad = t.n_long > 0 and t.n_long64 == t.n_loc_pad
    t.n_slices = (t.n_loc_pad - t.n_long64) // LZX_SLICE
    # items of the split rows
    t.item_cap = item_len if item_len is not None and item_len > 0 else LZX_ITEM
    dp = round_up(degl[:t.n_long64], 4)
    t.row_items = (dp + t.item_cap - 1) // t.item_cap
    t.n_items = int(t.row_items.sum())
    t.long_elems = int(dp.sum())
    lens = []
    for d, k in zip(dp.tolist(), t.row_items.tolist()):
        lens += [t.item_cap] * (k - 1) + ([d - (k - 1) * t.item_cap] if k else [])
    t.item_len = np.asarray(lens, dtype=np.int64)
    t.item_row = np.repeat(np.arange(t.n_long64), t.row_items)
    # slices
    body = degl[t.n_long64:].reshape(t.n_slices, LZX_SLICE) if t.n_slices else np.zeros((0, LZX_SLICE), dtype=np.int64)
    t.slice_w = round_up(body.max(axis=1), 4) if t.n_slices else np.zeros(0, dtype=np.int64)
    t.slice_uneven = (body.min(axis=1) < t.slice_w) if t.n_slices else np.zeros(0, dtype=bool)   # some row is padded
    t.sell_elems = int(t.slice_w.sum()) * LZX_SLICE
    t.sell_padded = t.sell_elems + t.long_elems        # lzx_get_graph_info: sell_elems + long_elems
    # classes and the processing order
    narrow = -1 if narrow_slices is None else narrow_slices
    t.classes = bool(blocked and narrow != 0 and (narrow > 0 or t.n_slices >= 8 * cus * WAVES_PER_WG))
    sid = np.arange(t.n_slices)
    wide = sid[t.slice_w > 8] if t.classes else sid
    t.w8 = sid[t.slice_w == 8] if t.classes else sid[:0]
    t.w4 = sid[t.slice_w == 4] if t.classes else sid[:0]
    t.w0 = sid[t.slice_w == 0] if t.classes else sid[:0]
    t.ns_wide, t.ns_w8, t.ns_w4, t.ns_w0 = len(wide), len(t.w8), len(t.w4), len(t.w0)
    t.perm = np.concatenate([wide, t.w8, t.w4, t.w0])
    # the grid of step 5
    per_cu = 1 if blocked else 4
    units = t.n_slices + t.n_items
    need = max(1, (units + WAVES_PER_WG - 1) // WAVES_PER_WG)
    grid = min(cus * per_cu, need)
    if blocked and units < cus * 512:
        grid = min(grid, max(1, cus // 2))
    if spmv_wgs is not None and spmv_wgs > 0:
        grid = min(cus * per_cu, need, spmv_wgs)
    t.grid, t.waves, t.units = grid, grid * WAVES_PER_WG, units
    t.fin_grid = (t.n_long64 + 255) // 256          # k_long_finish (plain mode): blocks of 256 split rows
    return t


def launch(t, live_rows_only):
    """(general-loop slices, w8, w4, w0 slices) of one launch: lzx_launch_spmv's cut to the live slices"""
    live = (t.rows_live - t.n_long64) // LZX_SLICE if t.rows_live > t.n_long64 else 0
    live = live if live_rows_only else t.n_slices
    general = t.ns_wide
    if t.ns_wide == t.n_slices:
        general = min(t.n_slices, live)
    return general, t.ns_w8, t.ns_w4, int(np.searchsorted(t.w0, live))


def counts(t, live_rows_only=False):
    """per wavefront of the staged grid: dict of arrays (one entry per wavefront) -- items, general, w8, w4, w0"""
    g, n8, n4, n0 = launch(t, live_rows_only)
    return dict(items=dealt(t.n_items, t.waves), general=dealt(g, t.waves), w8=dealt(n8, t.waves), w4=dealt(n4, t.waves),
                w0=dealt(n0, t.waves))


def wave_units(t, w, live_rows_only=False):
    """what wavefront w takes: (packets of each of its items, packets per lane of each of its general-loop slices, ids of its
    w8 / w4 / w0 slices)"""
    g, n8, n4, n0 = launch(t, live_rows_only)
    items = (t.item_len[w::t.waves] // 4).tolist()
    general = (t.slice_w[t.perm[:g][w::t.waves]] // 4).tolist()
    return items, general, t.w8[:n8][w::t.waves].tolist(), t.w4[:n4][w::t.waves].tolist(), t.w0[:n0][w::t.waves].tolist()


def item_packets(t):
    return t.item_len // 4


def general_packets(t, live_rows_only=False):
    g = launch(t, live_rows_only)[0]
    return t.slice_w[t.perm[:g]] // 4
