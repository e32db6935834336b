"""CPU: tests/pb_model.py on cases small enough to count by hand.  The order is presumed to be the identity; the expected
numbers are literals worked out from the rules in the comments of csrc/lzx_pb.hip, not taken from the model.  The small
cases shrink the step to 16 entries (two lanes of 8) and the row band to 4 rows and name the number of column bands;
the last ones use the product constants."""
import numpy as np
import pytest

import pb_model as pm


def csr(n, rows):
    """rows: {row: [columns]} -> (row_ptr, col_idx); the model needs no symmetry"""
    rp = np.zeros(n + 1, dtype=np.int64)
    ci = []
    for r in range(n):
        ci += sorted(rows.get(r, []))
        rp[r + 1] = len(ci)
    return rp, np.asarray(ci, dtype=np.int64)


# 32 positions, hub 2, bands of 8 positions: band 0 = 0..7 (0 and 1 staged), band 1 = 8..15, band 2 = 16..23.
# Row band 0 (rows 0..3): band 0 holds row 0: 2 3 4, row 1: 2 -> 4 entries; band 1 holds row 0: 8 9, row 1: 8 -> 3 entries;
# band 2 holds row 1: 16 17 18 19 -> 4 entries.  Row band 1 (rows 4..7): band 0 holds row 5: 3 4 5 6 7 -> 5 entries.
PATTERN_1 = {0: [2, 3, 4, 8, 9], 1: [2, 8, 16, 17, 18, 19], 5: [3, 4, 5, 6, 7], 6: [0, 1]}   # row 6: staged columns only


@pytest.mark.parametrize("min_run, align, expect", [
    # every run reduced, one step each.  Pieces: (row 0 ends at entry 2, row 1 at 3), (row 0 at 1, row 1 at 2), (row 1 at 3), (row 5 at 4)
    (3, 4, dict(reduced=16, steps=4, pieces=6, planes=[2, 3, 1, 2, 3, 4], values=16, units=[(0, 2, 0), (1, 1, 0), (2, 1, 0)])),
    # the run of 3 entries is plain: one quad
    (4, 4, dict(reduced=13, steps=3, pieces=4, planes=[2, 3, 3, 4], values=16, units=[(0, 2, 0), (1, 0, 1), (2, 1, 0)])),
    # eight value slots per run; the plain one still has ONE quad that holds entries (the second is padding: no band, never written)
    (4, 8, dict(reduced=13, steps=3, pieces=4, planes=[2, 3, 3, 4], values=32, units=[(0, 2, 0), (1, 0, 1), (2, 1, 0)])),
    # everything plain: 4 + 3 + 4 + 5 entries padded to 4, 4, 4, 8; band 0 holds the runs of 4 and 5: three quads
    (6, 4, dict(reduced=0, steps=0, pieces=0, planes=[], values=20, units=[(0, 0, 3), (1, 0, 1), (2, 0, 1)])),
])
def test_runs_at_the_minimum_length(min_run, align, expect):
    rp, ci = csr(32, PATTERN_1)
    t = pm.build(rp, ci, np.arange(32), hub=2, cb=8, min_run=min_run, run_align=align, unit_cap=64, taper=False, step=16, rb=4, nb=4)
    assert t.pb_entries == 16 and t.runs == 4 and list(t.run_len) == [4, 3, 4, 5]
    assert t.row_bands == 8 and list(t.row0) == [0, 4, 8, 12, 16, 20, 24, 28, 32]
    assert list(t.run_reduced) == [l >= min_run for l in (4, 3, 4, 5)]
    assert t.pb_reduced_entries == expect["reduced"] and t.steps == expect["steps"] and t.pieces == expect["pieces"]
    assert list(t.piece_plane) == expect["planes"] and t.pb_values == expect["values"]
    assert t.units == expect["units"]
    assert t.lane_gaps == 0 and all(l == 1 for l in t.piece_lanes) and all(s == 1 for s in t.row_steps)


def test_rows_across_lanes_and_steps():
    """Rows 0..3 with 5, 8, 6 and 3 entries in band 1: one run of 22 entries, padded to two steps of 16.  Row 0 takes entries
    0..4 (ends in plane 4), row 1 entries 5..12 (lanes 0 and 1, plane 4), row 2 entries 13..18: cut by the step boundary
    into 13..15 (plane 7) and 16..18 (plane 2), row 3 entries 19..21 (plane 5)."""
    rp, ci = csr(32, {0: range(8, 13), 1: range(8, 16), 2: range(8, 14), 3: range(8, 11)})
    t = pm.build(rp, ci, np.arange(32), hub=2, cb=8, min_run=3, run_align=4, unit_cap=64, taper=False, step=16, rb=4, nb=4)
    assert t.pb_entries == 22 and t.runs == 1 and list(t.run_len) == [22] and t.pb_reduced_entries == 22
    assert t.row_bands == 8          # the heaviest row has 8 entries: 2 * 4 bands is not below it, one slot per row
    assert t.steps == 2 and t.pieces == 5 and list(t.piece_plane) == [4, 4, 7, 2, 5]
    assert list(t.piece_lanes) == [1, 2, 1, 1, 1] and list(t.row_steps) == [1, 1, 2, 1] and list(t.step_pieces) == [3, 2]
    assert t.pb_values == 8 and t.units == [(1, 2, 0)] and t.lane_gaps == 0
    # three column bands instead of four: 2 * 3 < 8, the first band is closed after 4 / 2 = 2 rows, the next holds rows 2..5 -> two runs, 13 and 9 entries
    t = pm.build(rp, ci, np.arange(32), hub=2, cb=8, min_run=3, run_align=4, unit_cap=64, taper=False, step=16, rb=4, nb=3)
    assert list(t.row0[:3]) == [0, 2, 6] and list(t.run_len) == [13, 9] and t.steps == 2
    assert list(t.piece_plane) == [4, 4, 5, 0] and t.pb_values == 8


def test_one_row_of_1025_entries_product_constants():
    """Three steps and three pieces, closing in planes 7, 7 and 0; the row's band is closed after 16 rows (rep 64)."""
    rp, ci = csr(2048, {0: range(2, 1027)})
    t = pm.build(rp, ci, np.arange(2048), hub=2, cb=8192)
    assert t.nb == 1 and t.pb_entries == 1025 and t.runs == 1 and t.pb_reduced_entries == 1025
    assert t.steps == 3 and t.pieces == 3 and list(t.piece_plane) == [7, 7, 0]
    assert list(t.piece_lanes) == [64, 64, 1] and list(t.row_steps) == [3] and list(t.step_pieces) == [1, 1, 1]
    assert t.pb_values == 4 and list(t.row0) == [0, 16, 64] and t.row_bands == 2
    assert t.unit_cap == 8192 and t.units == [(0, 3, 0)]     # 1536 padded entries: one unit of the doubled (tapered) size
    # one entry fewer than the minimum is plain, the minimum itself reduced
    for length, reduced in ((383, False), (384, True)):
        rp, ci = csr(2048, {0: range(2, 2 + length)})
        t = pm.build(rp, ci, np.arange(2048), hub=2, cb=8192)
        assert list(t.run_reduced) == [reduced] and t.pb_values == (4 if reduced else 384) and t.steps == (1 if reduced else 0)
        assert t.units == [(0, 1, 0) if reduced else (0, 0, 96)]


def test_a_lane_without_a_piece_end_between_two_that_hold_one():
    """Row 0: 3 entries (lane 0), row 1: 30 entries, entries 3..32 of the step (lanes 0..4, ends in lane 4, plane 0)."""
    rp, ci = csr(64, {0: range(2, 5), 1: range(2, 32)})
    t = pm.build(rp, ci, np.arange(64), hub=2, cb=8192, min_run=3)
    assert list(t.run_len) == [33] and t.steps == 1 and list(t.piece_plane) == [2, 0] and list(t.piece_lanes) == [1, 5]
    assert t.lane_gaps == 1 and list(t.row0) == [0, 64]     # heaviest row 30: 16 replicas are enough, 64 rows


def test_the_order_is_taken_as_given():
    """A permuted order: ids[l] is the caller's id of the vertex at position l."""
    ids = np.array([3, 0, 2, 1] + list(range(4, 64)))
    # caller's vertex 3 (position 0) has the columns at positions 2 and 3, i.e. the caller's vertices 2 and 1
    rp, ci = csr(64, {3: [1, 2], 0: [3]})
    t = pm.build(rp, ci, ids, hub=2, cb=8192, min_run=2)
    assert t.pb_entries == 2 and list(t.run_len) == [2] and list(t.piece_plane) == [1]     # position 0 is staged: vertex 0's entry is not blocked


def test_scatter_units_taper_and_shares():
    # 10 bands of 2 steps + 8 quads = 1056 entries each; cap 512 tapered: the first 70 % in units of 1024, then 512, the last tenth max(16384, 256)
    units = pm.scatter_units(np.full(10, 2), np.full(10, 8), 512, True)
    parts = [sum(1 for u in units if u[0] == b) for b in range(10)]
    assert parts == [2, 2, 2, 2, 2, 2, 2, 3, 3, 1]
    assert [u[1:] for u in units if u[0] == 7] == [(0, 2), (1, 3), (1, 3)]     # steps 2 * i / 3, quads 8 * i / 3
    assert pm.wave_step_counts(0) == {0} and pm.wave_step_counts(17) == {1, 2} and pm.wave_step_counts(128) == {8}
    assert pm.tail_quads(256) == set() and pm.tail_quads(1) == {1} and pm.tail_quads(256 + 130) == {2, 3} and pm.tail_quads(200) == {3}
