"""Host model of the blocked SpMV's table formation (csrc/lzx_pb.hip: pb_prepare_impl, k_pb_run_format, k_pb_run_values,
k_pbr_place, pb_units) in numpy.  No GPU and no import of the package: the tests hand it the CSR, the row order the library
chose and the shape values, and compare what it counts with what the library reports (tests/test_gpu_pb_tables.py), or
with numbers worked out by hand (tests/test_pb_model_host.py).

What is taken as given: the ORDER (ids[l] = the caller's id of local row l, Engine.rank_row_sums() at world 1; l is also
the vertex's position in the layout of x) and hub = info()["hub_entries"].  Neither the degree sort nor the tie_sort
re-ranking is restated.

What is restated, one rank:
  blocked entries  an entry is blocked when the position of its column is >= hub.  Its column code is hub + position
                   (k_rank_maps) and the builder takes p = code - hub (k_pb_emit): p IS the position.  Column band
                   p // cb, column in band p % cb; the bands tile the whole layout of x, staged positions included.
  row bands        the `rep` loop of pb_prepare_impl over the blocked count per row and the number of column bands, over
                   min(rows, rows with an edge rounded up to 64) rows; with reduce off the target / 1024-row rule.
  runs             maximal stretches of one (row band, column band) in key order (row band, column band, row, column).
  format           len >= min_run: reduced, padded to whole steps of 512 entries; a piece is one row within a step; lane
                   l of a step holds entries 8 l .. 8 l + 7 and a piece that ends at entry e of its lane lies in plane e.
  values           pieces of a reduced run, entries of a plain one, rounded up to run_align.
  scatter units    pb_units as written: steps and quads per column band (the quads of a plain run that hold an entry: the
                   padding run_align adds behind them is dealt to no band), the taper rule, parts, per-unit ranges.
"""
import numpy as np

# the builder's constants (csrc/lzx_internal.h)
LZX_PBR_STEP = 512
LZX_PBR_MIN_RUN = 384
LZX_PB_ALIGN = 4
LZX_PB_RB = 1024
LZX_PB_TARGET = 32768
LZX_SLICE = 64
LZX_TAIL = 64
CU_COUNT = 256          # MI355X: enters the default target and unit size only
LANE = 8                # entries per lane of a reduced step
WAVES = 16              # wavefronts of a scatter workgroup


def round_up(a, m):
    return (a + m - 1) // m * m


def layout_len(n):
    """xlen on one rank: the rows padded to whole slices plus the tail (lzx_graph_prepare)."""
    return round_up(n, LZX_SLICE) + LZX_TAIL


def default_unit_cap(total, xlen, cus=CU_COUNT):
    if xlen * 8 <= (16 << 20):
        return min(65536, max(8192, round_up(total // (cus * 2), 512)))
    return min(131072, max(32768, round_up(total // (cus * 4), 512)))


def default_target(total, cus=CU_COUNT):
    return min(8 * LZX_PB_TARGET, max(LZX_PB_TARGET, round_up(total // (cus * 8), 1024)))


def row_bands(nh, band_rows, nb, reduce, target, rb=LZX_PB_RB):
    """first row of every band (+ the end): pb_prepare_impl's two rules as written"""
    row0 = [0]
    if reduce:
        l = 0
        while l < band_rows:
            rep = 1
            while True:
                e = min(l + rb // rep, band_rows)
                heaviest = int(nh[l:e].max()) if e > l else 0
                need = rep
                while need < 64 and need * 2 * nb < heaviest:
                    need <<= 1
                if need == rep:
                    break
                rep = need
            l = min(l + rb // rep, band_rows)
            row0.append(l)
    else:
        rows, cnt = 0, 0
        for l in range(band_rows):
            h = int(nh[l])
            if rows > 0 and (cnt + h > target or rows == rb):
                row0.append(l)
                rows, cnt = 0, 0
            rows += 1
            cnt += h
        if rows > 0:
            row0.append(band_rows)
    if len(row0) == 1:
        row0.append(band_rows)
    return np.asarray(row0, dtype=np.int64)


def scatter_units(steps_b, quads_b, cap, taper, step=LZX_PBR_STEP):
    """pb_units: [(column band, steps, quads)] in dispatch order"""
    ent = steps_b * step + quads_b * 4
    total, done, units = int(ent.sum()), 0, []
    for b in range(len(ent)):
        entries, S, Q = int(ent[b]), int(steps_b[b]), int(quads_b[b])
        if entries == 0:
            continue
        capb = cap
        if taper:
            capb = 2 * cap if done * 10 < total * 7 else cap if done * 10 < total * 9 else max(16384, cap // 2)
        done += entries
        parts = (entries + capb - 1) // capb
        for i in range(parts):
            units.append((b, S * (i + 1) // parts - S * i // parts, Q * (i + 1) // parts - Q * i // parts))
    return units


def wave_step_counts(S):
    """how many steps the wavefronts of a unit of S steps take (wavefront w: steps w, w + 16, ...): the set of counts"""
    return {(S - w + WAVES - 1) // WAVES if S > w else 0 for w in range(WAVES)}


def tail_quads(Q):
    """the unit's partly filled last 256-quad block: the set of per-lane quad counts its tail code handles (1 .. 3)"""
    m = Q % 256
    return {c for c in ((m - lane + 63) // 64 for lane in range(min(m, 64))) if 0 < c < 4}


class Tables:
    pass


def build(rp, ci, ids, hub, cb, min_run=LZX_PBR_MIN_RUN, run_align=LZX_PB_ALIGN, unit_cap=None, taper=True, reduce=True,
          target=None, step=LZX_PBR_STEP, rb=LZX_PB_RB, nb=None, cus=CU_COUNT):
    """The tables of one rank.  step, rb and nb are parameters for the hand-worked host cases only: the GPU tests leave them at
    the builder's constants (nb: the bands of the one-rank layout)."""
    rp = np.asarray(rp).astype(np.int64)
    ci = np.asarray(ci).astype(np.int64)
    ids = np.asarray(ids).astype(np.int64)
    n = len(rp) - 1
    assert len(ids) == n and step % LANE == 0
    pos = np.empty(n, dtype=np.int64)
    pos[ids] = np.arange(n)
    deg = np.diff(rp)
    n_active = int((deg > 0).sum())
    xlen = layout_len(n)
    if nb is None:
        nb = (xlen + cb - 1) // cb
    row = np.repeat(pos, deg)
    col = pos[ci]
    keep = col >= hub
    row, p = row[keep], col[keep]
    total = len(row)
    nh = np.bincount(row, minlength=n)
    band_rows = min(n, min(round_up(n, LZX_SLICE), round_up(n_active, LZX_SLICE)))
    assert not nh[band_rows:].any(), "a row behind the rows with an edge has blocked entries: not the library's order"
    if target is None:
        target = default_target(total, cus)
    if unit_cap is None:
        unit_cap = default_unit_cap(total, xlen, cus)
    if not reduce:
        min_run = None

    t = Tables()
    t.n, t.hub, t.cb, t.nb, t.n_active, t.min_run, t.run_align = n, hub, cb, nb, n_active, min_run, run_align
    t.row0 = row_bands(nh, band_rows, nb, reduce, target, rb)
    t.row_bands = len(t.row0) - 1
    t.band_rows = np.diff(t.row0)
    t.pb_entries = total

    rband = np.searchsorted(t.row0[1:], row, side="right")
    lrow = row - t.row0[rband]
    cband, lcol = p // cb, p % cb
    o = np.lexsort((lcol, lrow, cband, rband))
    rband, cband, lrow, lcol = rband[o], cband[o], lrow[o], lcol[o]
    pair = rband * nb + cband
    head = np.ones(total, dtype=bool)
    head[1:] = pair[1:] != pair[:-1]
    runstart = np.flatnonzero(head)
    t.runs = len(runstart)
    t.run_len = np.diff(np.append(runstart, total))
    t.run_cband = cband[runstart]
    t.run_rband = rband[runstart]
    red = t.run_len >= min_run if min_run is not None else np.zeros(t.runs, dtype=bool)
    t.run_reduced = red
    t.pb_reduced_entries = int(t.run_len[red].sum())
    epad = np.where(red, round_up(t.run_len, step), 0)
    estep = np.concatenate(([0], np.cumsum(epad // step)))     # first step of every run
    t.steps = int(estep[-1])
    t.run_steps = epad // step

    # pieces of the reduced runs
    run_of = np.cumsum(head) - 1
    off = np.arange(total) - runstart[run_of]
    sel = red[run_of]
    r_run, r_off, r_row = run_of[sel], off[sel], lrow[sel]
    m = len(r_run)
    last = np.ones(m, dtype=bool)
    if m:
        last[:-1] = (r_off[:-1] % step == step - 1) | (r_run[1:] != r_run[:-1]) | (r_row[1:] != r_row[:-1])
    first = np.ones(m, dtype=bool)
    first[1:] = last[:-1]
    p_end, p_beg = r_off[last], r_off[first]
    p_run, p_row = r_run[last], r_row[last]
    t.pieces = len(p_end)
    t.piece_plane = p_end % LANE
    t.piece_step = estep[p_run] + p_end // step                 # in gather (row band major) order
    t.piece_lanes = (p_end % step) // LANE - (p_beg % step) // LANE + 1
    t.step_pieces = np.bincount(t.piece_step, minlength=t.steps)
    # steps a row spans within its run: its pieces there
    rowkey = p_run * (int(t.band_rows.max()) + 1 if t.row_bands else 1) + p_row
    t.row_steps = np.unique(rowkey, return_counts=True)[1] if t.pieces else np.zeros(0, dtype=np.int64)
    # a lane without a piece end between two lanes of its step that hold one
    lane_key = np.unique(t.piece_step * (step // LANE) + (p_end % step) // LANE)
    same = lane_key[1:] // (step // LANE) == lane_key[:-1] // (step // LANE)
    t.lane_gaps = int((same & (np.diff(lane_key) > 1)).sum())

    # values per run
    run_pieces = np.bincount(p_run, minlength=t.runs)
    vcount = round_up(np.where(red, run_pieces, t.run_len), run_align)
    t.run_values = vcount
    t.pb_values = int(vcount.sum())

    # scatter units
    steps_b = np.bincount(t.run_cband[red], weights=t.run_steps[red], minlength=nb).astype(np.int64)
    # (a quad is dealt to its column band by the entry in its first slot, k_pb_place: the quads of a plain run are those that hold
    #  an entry, ceil(len / 4); what run_align adds behind them belongs to no band and is never written)
    quads_b = np.bincount(t.run_cband[~red], weights=(t.run_len[~red] + 3) // 4, minlength=nb).astype(np.int64)
    t.band_steps, t.band_quads = steps_b, quads_b
    t.unit_cap = unit_cap
    t.units = scatter_units(steps_b, quads_b, unit_cap, taper, step)
    t.scatter_units = len(t.units)
    return t
