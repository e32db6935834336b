"""CPU: tests/sell_model.py held to cases counted by hand.  Every expected number below is written out, not computed.
The order handed to the model is the plain one (degree descending, ties by vertex id) unless a case states its own."""
import numpy as np
import scipy.sparse as sp

import sell_model as sm


def csr(n, edges):
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    s, d = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    A = sp.coo_matrix((np.ones(len(s)), (s, d)), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int64)


def by_degree(rp):
    deg = np.diff(rp)
    ids = np.argsort(-deg, kind="stable")
    rank_of = np.empty(len(ids), dtype=np.int64)
    rank_of[ids] = np.arange(len(ids))
    return ids, rank_of, int((deg > 0).sum())


def plain(n, edges, **shapes):
    rp, ci = csr(n, edges)
    ids, rank_of, n_active = by_degree(rp)
    return sm.build(rp, ci, ids, rank_of, 0, False, n_active, **shapes)


def star_ring():
    """vertex 0 joined to the 99 vertices of a ring: degrees 99 and 3, 100 vertices, two slices of rows"""
    return [(0, i) for i in range(1, 100)] + [(i, i % 99 + 1) for i in range(1, 100)]


def test_staging_rule():
    assert sm.staging(1000, 1000, 0, 16) == (False, 16)
    assert sm.staging(1000, 1000, 1, 0) == (False, 0)             # nothing staged: nothing to block
    assert sm.staging(1000, 1000, 1, 17) == (True, 16)            # even
    assert sm.staging(1000, 1000, 1, 16384) == (False, 1000)      # everything staged
    assert sm.staging(1001, 1001, 1, 16384) == (True, 1000)       # odd n: one column left to block
    assert sm.staging(5000, 301, 1, 1500) == (True, 300)          # cut to the vertices with an edge, even
    assert sm.staging(5000, 300, 1, 1500) == (False, 300)         # ... all of which are then staged
    assert sm.staging(5000, 301, 0, 1500) == (False, 300)         # the cut holds in plain mode too
    assert sm.staging(50000, 50000, 1, 30000) == (True, 20000)    # 160 KiB of LDS


def test_path():
    t = plain(5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    assert (t.n_loc_pad, t.n_loc_real, t.rows_live) == (64, 5, 64)
    assert t.degl[:6].tolist() == [2, 2, 2, 1, 1, 0]
    assert (t.thr, t.n_long, t.n_long64, t.n_slices, t.n_items, t.long_elems) == (128, 0, 0, 1, 0, 0)      # no split row
    assert t.slice_w.tolist() == [4] and t.sell_elems == 256 and t.sell_padded == 256
    assert (t.ns_wide, t.ns_w8, t.ns_w4, t.ns_w0) == (1, 0, 0, 0) and not t.classes
    assert (t.grid, t.waves) == (1, 16)
    c = sm.counts(t)
    assert c["general"].tolist() == [1] + [0] * 15 and c["items"].tolist() == [0] * 16
    assert sm.wave_units(t, 0) == ([], [1], [], [], []) and sm.wave_units(t, 1) == ([], [], [], [], [])


def test_star_and_ring_threshold_at_the_degree():
    for thr in (99, 100):      # the centre's 99 entries are not OVER 99: it stays in the body
        t = plain(100, star_ring(), long_row=thr)
        assert (t.n_loc_pad, t.thr, t.n_long, t.n_long64, t.n_slices, t.n_items) == (128, thr, 0, 0, 2, 0)
        assert t.slice_w.tolist() == [100, 4] and t.sell_elems == 6656 and t.sell_padded == 6656
        assert sm.general_packets(t).tolist() == [25, 1]
    t = plain(100, star_ring(), long_row=98)
    # the centre is a split row, and with it the 63 ring rows that share its slice
    assert (t.n_long, t.n_long64, t.n_slices, t.n_items, t.long_elems, t.sell_elems, t.sell_padded) == (1, 64, 1, 64, 352, 256, 608)
    assert t.row_items.tolist() == [1] * 64 and t.item_len.tolist() == [100] + [4] * 63
    assert t.slice_w.tolist() == [4]
    assert (t.units, t.grid, t.waves) == (65, 5, 80) and t.fin_grid == 1
    assert sm.counts(t)["items"].tolist() == [1] * 64 + [0] * 16 and sm.counts(t)["general"].tolist() == [1] + [0] * 79
    t = plain(100, star_ring(), long_row=98, item_len=16, spmv_wgs=1)
    assert t.row_items[:2].tolist() == [7, 1] and t.item_len[:8].tolist() == [16] * 6 + [4, 4] and t.n_items == 70
    assert (t.grid, t.waves) == (1, 16)
    assert sm.counts(t)["items"].tolist() == [5] * 6 + [4] * 10       # 70 items over 16 wavefronts
    assert sm.wave_units(t, 6)[0] == [1, 1, 1, 1] and sm.wave_units(t, 0)[0] == [4, 1, 1, 1, 1]
    t = plain(100, star_ring(), long_row=98, item_len=100)
    assert t.item_len[:2].tolist() == [100, 4] and t.n_items == 64      # a last item of exactly item_cap


def test_every_row_split():
    """star + ring on 11 vertices, threshold 2: the last row over it is row 10, the split rows round up to the padded rows"""
    t = plain(11, [(0, i) for i in range(1, 11)] + [(i, i % 10 + 1) for i in range(1, 11)], long_row=2)
    assert (t.n_loc_pad, t.n_loc_real, t.n_long, t.n_long64, t.n_slices) == (64, 11, 11, 64, 0)
    assert t.row_items.tolist() == [1] * 11 + [0] * 53             # padding rows have no item
    assert t.item_len.tolist() == [12] + [4] * 10 and (t.n_items, t.long_elems, t.sell_elems, t.sell_padded) == (11, 52, 0, 52)
    assert (t.ns_wide, t.grid) == (0, 1) and sm.counts(t)["general"].tolist() == [0] * 16


def test_blocked_row_without_staged_entry_ahead_of_the_last_split_row():
    """rank = vertex id; vertices 0 and 1 are staged.  Rows 0 and 1 have no staged entry, rows 2, 3, 4 two and row 5 one."""
    rp, ci = csr(6, [(0, 2), (0, 3), (0, 4), (0, 5), (1, 2), (1, 3), (1, 4), (2, 3)])
    assert np.diff(rp).tolist() == [4, 3, 3, 3, 2, 1]
    t = sm.build(rp, ci, np.arange(6), np.arange(6), 2, True, 6, long_row=1)
    assert t.degl[:6].tolist() == [0, 0, 2, 2, 2, 1]
    assert (t.thr, t.n_long, t.n_long64, t.n_slices) == (1, 5, 64, 0)
    assert t.row_items[:7].tolist() == [0, 0, 1, 1, 1, 1, 0]          # row 5 (one staged entry) lies inside the rounding
    assert (t.n_items, t.long_elems, t.item_len.tolist(), t.item_row.tolist()) == (4, 16, [4, 4, 4, 4], [2, 3, 4, 5])
    t = sm.build(rp, ci, np.arange(6), np.arange(6), 2, True, 6)
    assert (t.thr, t.n_long, t.n_slices, t.slice_w.tolist()) == (256, 0, 1, [4])
    assert sm.build(rp, ci, np.arange(6), np.arange(6), 2, False, 6).degl[:6].tolist() == [4, 3, 3, 3, 2, 1]


def classes_graph():
    """12 staged vertices H; 64 rows joined to all 12, 64 to the first 8, 64 to the first 3, 64 joined in pairs among themselves.
    Order: H (degrees 192, 128, 64), then the four groups.  The 12 rows of H hold no staged entry and shift every group by 12 rows."""
    e = []
    for i in range(64):
        e += [(12 + i, h) for h in range(12)] + [(76 + i, h) for h in range(8)] + [(140 + i, h) for h in range(3)]
    e += [(204 + 2 * i, 205 + 2 * i) for i in range(32)]
    return csr(268, e)


def test_classes():
    rp, ci = classes_graph()
    ids, rank_of, n_active = by_degree(rp)
    assert ids.tolist() == list(range(268)) and n_active == 268
    t = sm.build(rp, ci, ids, rank_of, 12, True, n_active, narrow_slices=1)
    assert (t.n_loc_pad, t.n_long, t.n_slices) == (320, 0, 5)
    assert t.slice_w.tolist() == [12, 12, 8, 4, 0] and t.sell_elems == 2304
    assert t.slice_uneven.tolist() == [True, True, True, True, False]
    assert t.classes and (t.ns_wide, t.ns_w8, t.ns_w4, t.ns_w0) == (2, 1, 1, 1) and t.perm.tolist() == [0, 1, 2, 3, 4]
    assert (t.units, t.grid) == (5, 1)
    c = sm.counts(t)
    assert c["general"].tolist() == [1, 1] + [0] * 14 and c["w8"].tolist() == c["w4"].tolist() == c["w0"].tolist() == [1] + [0] * 15
    assert sm.wave_units(t, 0) == ([], [3], [2], [3], [4])
    # the size rule: five slices are far below 8 * 256 * 16, so the default forms no class; narrow_slices = 0 neither
    for narrow in (None, 0):
        u = sm.build(rp, ci, ids, rank_of, 12, True, n_active, narrow_slices=narrow)
        assert not u.classes and (u.ns_wide, u.ns_w8, u.ns_w4, u.ns_w0) == (5, 0, 0, 0)
        assert sm.general_packets(u).tolist() == [3, 3, 2, 1, 0]
    assert sm.build(rp, ci, ids, rank_of, 12, True, n_active, cus=0).classes      # ... and holds from 8 CUs 16 slices on
    # two staged vertices: every joined row keeps two entries -- no wide and no 8-code slice while w4 and w0 are populated
    t = sm.build(rp, ci, ids, rank_of, 2, True, n_active, narrow_slices=1)
    assert t.slice_w.tolist() == [4, 4, 4, 4, 0] and (t.ns_wide, t.ns_w8, t.ns_w4, t.ns_w0) == (0, 0, 4, 1)
    assert t.perm.tolist() == [0, 1, 2, 3, 4] and sm.counts(t)["general"].tolist() == [0] * 16
    # threshold 8 in blocked mode: the last row over it is row 75 (the last of the 12-entry group)
    t = sm.build(rp, ci, ids, rank_of, 12, True, n_active, narrow_slices=1, long_row=8, item_len=4)
    assert (t.n_long, t.n_long64, t.n_slices, t.slice_w.tolist()) == (76, 128, 3, [8, 4, 0])
    assert t.row_items[:12].tolist() == [0] * 12 and t.row_items[12:76].tolist() == [3] * 64 and t.row_items[76:128].tolist() == [2] * 52
    assert (t.n_items, t.long_elems, t.ns_wide, t.ns_w8, t.ns_w4, t.ns_w0) == (296, 1184, 0, 1, 1, 1)


def test_grid_rule():
    path = [(i, i + 1) for i in range(2047)]
    t = plain(2048, path)
    assert (t.n_slices, t.units, t.grid, t.waves) == (32, 32, 2, 32) and sm.counts(t)["general"].tolist() == [1] * 32
    t = plain(2048, path, spmv_wgs=1)
    assert (t.grid, t.waves) == (1, 16) and sm.counts(t)["general"].tolist() == [2] * 16
    t = plain(2048, path, spmv_wgs=7)
    assert t.grid == 2                                              # never more than one wavefront per unit
    t = plain(2048, path, cus=1)
    assert t.grid == 2
    t = plain(2048 * 64, [(i, i + 1) for i in range(2048 * 64 - 1)], cus=2)
    assert (t.units, t.grid) == (2048, 8)                           # 4 workgroups per CU in plain mode
    rp, ci = csr(2048 * 64, [(i, i + 1) for i in range(2048 * 64 - 1)])
    ids, rank_of, n_active = by_degree(rp)
    t = sm.build(rp, ci, ids, rank_of, 2, True, n_active, cus=8)
    assert (t.units, t.grid) == (2048, 4)                           # blocked: one per CU, halved below 8 * 512 units
    t = sm.build(rp, ci, ids, rank_of, 2, True, n_active, cus=4)
    assert t.grid == 4                                              # ... not from 4 * 512 units on
    t = sm.build(rp, ci, ids, rank_of, 2, True, n_active, cus=8, spmv_wgs=6)
    assert t.grid == 6                                              # spmv_wgs replaces the halving, not the ceiling


def test_live_rows_and_ranks():
    t = plain(200, [(i, i + 1) for i in range(69)])                 # 70 vertices with an edge, 130 without
    assert (t.n_loc_pad, t.rows_live, t.n_slices, t.slice_w.tolist()) == (256, 128, 4, [4, 4, 0, 0])
    assert sm.launch(t, False) == (4, 0, 0, 0) and sm.launch(t, True) == (2, 0, 0, 0)
    rp, ci = csr(200, [(i, i + 1) for i in range(139)])             # 140 vertices with an edge
    ids, rank_of, n_active = by_degree(rp)
    assert ids[:2].tolist() == [1, 2] and ids[136:140].tolist() == [137, 138, 0, 139]
    t = sm.build(rp, ci, ids, rank_of, 2, True, n_active, narrow_slices=1)
    # staged: ranks 0 and 1 = vertices 1 and 2; the rows of vertices 1, 2, 3 (rows 0, 1, 2) and of vertex 0 (row 138) hold a staged entry
    assert t.rows_live == 192 and t.slice_w.tolist() == [4, 0, 4, 0] and (t.ns_wide, t.ns_w8, t.ns_w4, t.ns_w0) == (0, 0, 2, 2)
    assert t.perm.tolist() == [0, 2, 1, 3]
    assert sm.launch(t, False) == (0, 0, 2, 2) and sm.launch(t, True) == (0, 0, 2, 1)      # one width-0 slice is live, one is not
    # three ranks: rank r of the order is local row r // 3 of rank r % 3
    t = sm.build(rp, ci, ids[1::3], rank_of, 2, True, n_active, world=3, rank=1)
    assert (t.n_loc_pad, t.n_loc_real, t.rows_live) == (128, 67, 64)      # 47 of this rank's rows have an edge
    assert ids[1::3][:3].tolist() == [2, 5, 8] and t.degl[:3].tolist() == [1, 0, 0]   # vertex 2: neighbours 1 (staged) and 3


def test_exchange_stride():
    assert sm.exchange(200, 140, 1, 1, 2) == (256, 256)                      # one rank: the padded rows, whatever the mode
    assert sm.exchange(200, 140, 3, 0, 2) == (64, 64)                        # 47 vertices with an edge per rank
    assert sm.exchange(200, 140, 3, 1, 2) == (64, 64)                        # blocked, but a 16 Ki band is no less than the slice
    assert sm.exchange(200, 0, 3, 0, 0) == (64, 64)                          # never below one slice
    assert sm.exchange(100000, 100000, 2, 1, 1000) == (50048, 16384)         # an eighth (6256) rounded up to the band
    assert sm.exchange(100000, 100000, 2, 0, 1000) == (50048, 50048)         # plain mode: one chunk
    assert sm.exchange(100000, 100000, 2, 1, 1000, overlap=False) == (50048, 50048)
    assert sm.exchange(100000, 100000, 3, 1, 16384) == (33344, 16384)
    assert sm.exchange(100000, 70000, 2, 1, 16384) == (35008, 16384)         # the slice covers the vertices with an edge
    assert sm.exchange(100000, 32768, 2, 1, 16384) == (16384, 16384)         # x0 = 16384 is not below the slice: one chunk
    assert sm.exchange(300000, 300000, 2, 1, 16384) == (150016, 32768)       # an eighth (18752) takes two bands
    assert sm.exchange(1200000, 1200000, 2, 1, 16384) == (600000, 81920)     # 9.6 MB of x: 16 Ki bands, 75000 -> 5 of them
    assert sm.exchange(3000000, 3000000, 2, 1, 16384) == (1500032, 202752)   # x beyond 16 MiB: 18 Ki bands, 187504 -> 11 of them
    assert sm.exchange(3000000, 3000000, 2, 1, 16384, column_band=8192) == (1500032, 196608)   # ... unless a band is forced: 12 of 16 Ki
    assert sm.exchange(100000, 20001, 2, 1, 20000) == (10048, 10048)
    assert sm.exchange(60000, 60000, 2, 1, 16384) == (30016, 16384)
    assert sm.exchange(60000, 16384, 2, 1, 16384) == (8192, 8192)            # every vertex with an edge staged: not blocked
