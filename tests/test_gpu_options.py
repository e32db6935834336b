"""GPU: the option table of csrc/lzx_api.hip -- which names lzx_set_option and lzx_test_set_shape accept in each library, their
return codes and the three names that are not plain stores.  Pins PRODUCT_OPTIONS / SHAPE_OPTIONS of the package (which Python
needs before a library is loaded) to the table."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_STATE = 0, -1, -3

# what lzx_set_option accepts in liblzx_dbg.so only
KNOBS = ("wgs_per_cu", "nt_index_loads", "long_row", "pb_target", "pb_run_align", "pb_reduce", "pb_unit", "pb_taper", "pb_dyn_share",
         "pb_gather_grid", "pb_gather_nt", "spmv_wgs", "pb_column_band", "side_stream", "pb_stamps", "pb_order", "spmv_deep", "tie_sort",
         "pb_group", "pb_group_force", "item_len", "stage_burst", "vec_blocks_per_cu", "narrow_slices", "fuse_staged", "isolated_rows",
         "unnormalised_basis", "pb_gather_waves", "exchange_at_world_1", "phase_mask", "start_vector_scan", "defer_finish")
LOOP_OPTIONS = ("reorthogonalise", "basis_fp32", "reference_order", "operator")

RP = np.array([0, 1, 2, 2], dtype=np.uint64)
CI = np.array([1, 0], dtype=np.uint32)


def _set(eng, name, value, entry="lzx_set_option"):
    rc = getattr(eng.L, entry)(eng.h, name.encode(), value)
    return rc, eng.L.lzx_last_error().decode()


def test_names_accepted_by_each_entry_point(pkg):
    assert len(KNOBS) == 32 and len(set(KNOBS)) == 32
    prod, dbg = pkg.Engine(0), pkg.Engine(0, phase_mask=3)
    assert not prod.debug and dbg.debug and prod.L is not dbg.L
    for name in pkg.PRODUCT_OPTIONS:
        assert _set(prod, name, 0)[0] == OK, name
        assert _set(dbg, name, 0)[0] == OK, name
    for name in pkg.SHAPE_OPTIONS:
        assert _set(prod, name, -1, "lzx_test_set_shape")[0] == OK, name
    for name in KNOBS:
        rc, msg = _set(prod, name, -1)
        assert rc == ERR_ARG and f"unknown option '{name}'" in msg, (name, rc, msg)
        assert _set(dbg, name, -1)[0] == OK, name
    for eng in (prod, dbg):
        rc, msg = _set(eng, "no_such_option", 1)
        assert rc == ERR_ARG and "unknown option 'no_such_option'" in msg
        rc, msg = _set(eng, "no_such_option", 1, "lzx_test_set_shape")
        assert rc == ERR_ARG and "unknown shape 'no_such_option'" in msg
        rc, msg = _set(eng, "operator", 2)
        assert rc == ERR_ARG and "operator must be" in msg
        eng.close()


def test_loop_options_after_the_hand_over(pkg):
    eng = pkg.Engine(0)
    eng.set_graph_csr(RP, CI)
    rc, msg = _set(eng, "hub_entries", 64)
    assert rc == ERR_STATE and "before the graph is handed over" in msg
    assert _set(eng, "no_such_option", 1)[0] == ERR_STATE          # the call order is judged before the name
    assert _set(eng, "pb_reduce", 1, "lzx_test_set_shape")[0] == ERR_STATE
    assert _set(eng, "operator", 2)[0] == ERR_ARG                  # ... and the operator's range before the call order
    for name in LOOP_OPTIONS:
        assert _set(eng, name, 0)[0] == OK, name
        eng.lanczos_prepare(np.ones(3), 2)
        assert eng.lanczos_progress() == (0, 2)
        assert _set(eng, name, 0)[0] == OK, name
        assert eng.lanczos_progress()[1] == 0, name
    eng.close()


def test_negative_sharded_ingest_is_off(pkg):
    """sharded_ingest = -5 is stored as 0: the hand-over takes the whole-graph path, whose CSR stays on the device as handed
    over (lzx_graph_info carries no flag of its own for this: the rank's share is the whole graph and it reads back equal)."""
    eng = pkg.Engine(0)
    assert _set(eng, "sharded_ingest", -5)[0] == OK
    eng.set_graph_csr(RP, CI)
    gi = eng.info()
    assert gi["world"] == 1 and gi["nnz"] == 2 and gi["nnz_local"] == 2 and gi["rows_local"] == 3
    rp, ci = eng.get_graph_csr()
    assert np.array_equal(rp, RP) and np.array_equal(ci, CI)
    assert np.array_equal(eng.spmv(np.array([1.0, 2.0, 3.0])), np.array([2.0, 1.0, 0.0]))
    eng.close()
