"""ctypes face of liblzx.so (include/lzx.h) for the parity tests, bench.py and the smoke check.

This is plumbing, not the product: the product is the C-ABI library built from csrc/ and the C++
drop-in classes in host/.  There is no CPU fallback here -- if liblzx.so is missing or a call fails the
error is raised; nothing in this package imports the test oracle.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblzx.so")
# the same code built with -DLZX_DEBUG_KNOBS: experiment knobs, test hooks, ablation switches (Makefile, `make debug`)
DBG_LIB_PATH = os.path.join(_HERE, "liblzx_dbg.so")
# what the product library's lzx_set_option knows (include/lzx.h); any other option name selects the debug library
PRODUCT_OPTIONS = ("hub_entries", "propagation_blocking", "overlap_exchange", "sparse_exchange", "exchange_fp32",
                   "lazy_normalisation", "timing_marks_every", "reorthogonalise", "basis_fp32", "reference_order", "placement_trials",
                   "sharded_ingest", "operator")

# test-only shapes the product library accepts through lzx_test_set_shape (csrc/lzx_test_hooks.h): they select among code
# paths the product contains (what large graphs get by themselves), so tests that force them still run liblzx.so
SHAPE_OPTIONS = ("pb_reduce", "pb_target", "pb_unit", "pb_column_band", "pb_run_align", "pb_taper", "pb_dyn_share", "pb_carry_scan", "pb_scatter_nt", "pb_gather_grid", "pb_gather_nt", "spmv_wgs", "pb_group", "pb_group_force",
                 "narrow_slices", "tie_sort", "long_row", "item_len", "exchange_at_world_1", "isolated_rows", "unnormalised_basis", "fuse_staged", "start_vector_scan", "defer_finish",
                 "multi_row_chunk", "eig_basis_bytes", "solve_state_bytes", "solve_poll", "bfs_state_bytes", "tri_long_list", "tri_state_bytes", "core_long_row", "core_state_bytes",
                 "truss_long_row", "truss_state_bytes", "color_long_row", "lpa_group_row", "lpa_table_row", "lpa_state_bytes", "louvain_state_bytes",
                 "sweep_long_row", "sweep_state_bytes", "sim_long_pair", "sim_slice", "sim_state_bytes", "graph_lanes")

LZX_BRANDES_ENDPOINTS = 1  # include/lzx.h: lzx_brandes_f64's flag, bc counts the endpoints of every path too
LZX_COLOR_TIES_BY_ID = 1   # include/lzx.h: the colouring's order without the hash, (degree descending, id ascending)
# include/lzx.h, the flags of lzx_sweep_cut: ascending keys; the key is score / degree; edge expansion instead of conductance
LZX_SWEEP_ASCENDING, LZX_SWEEP_PER_DEGREE, LZX_SWEEP_EXPANSION = 1, 2, 4
SWEEP_BATCH = 16           # score vectors per lzx_sweep_cut
# include/lzx.h, the measures of lzx_similarity, in the order of their rows in `values`
LZX_SIM_JACCARD, LZX_SIM_OVERLAP, LZX_SIM_SORENSEN, LZX_SIM_ADAMIC_ADAR, LZX_SIM_RESOURCE_ALLOCATION = 1, 2, 4, 8, 16
SIM_MEASURES = {"jaccard": LZX_SIM_JACCARD, "overlap": LZX_SIM_OVERLAP, "sorensen": LZX_SIM_SORENSEN,
                "adamic_adar": LZX_SIM_ADAMIC_ADAR, "resource_allocation": LZX_SIM_RESOURCE_ALLOCATION}

_u64p = ctypes.POINTER(ctypes.c_uint64)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_i32p = ctypes.POINTER(ctypes.c_int32)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_f64p = ctypes.POINTER(ctypes.c_double)
_h = ctypes.c_void_p
_hp = ctypes.POINTER(ctypes.c_void_p)


class LzxStats(ctypes.Structure):
    _fields_ = [("loop_ms", ctypes.c_double), ("spmv_ms", ctypes.c_double),
                ("spmv_ms_min", ctypes.c_double), ("vec_ms", ctypes.c_double),
                ("comm_ms", ctypes.c_double), ("iters", ctypes.c_uint32),
                ("spmv_kernels", ctypes.c_uint32), ("spmv_bytes", ctypes.c_uint64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class LzxGraphInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("nnz", ctypes.c_uint64), ("max_degree", ctypes.c_uint64),
                ("rows_local", ctypes.c_uint64), ("nnz_local", ctypes.c_uint64),
                ("long_rows", ctypes.c_uint64), ("sell_padded", ctypes.c_uint64),
                ("pb_entries", ctypes.c_uint64), ("active_vertices", ctypes.c_uint64),
                ("exchange_slice", ctypes.c_uint64), ("hub_entries", ctypes.c_uint32), ("world", ctypes.c_uint32), ("rank", ctypes.c_uint32),
                ("reserved_", ctypes.c_uint32), ("pb_values", ctypes.c_uint64), ("pb_reduced_entries", ctypes.c_uint64),
                ("exchange_chunk0", ctypes.c_uint64), ("exchange_recv", ctypes.c_uint64),
                ("placement_tried", ctypes.c_uint32), ("placement_kept", ctypes.c_uint32), ("placement_us", ctypes.c_uint32 * 8)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["placement_us"] = list(d["placement_us"])[:d["placement_tried"]]
        return d


class LzxEigInfo(ctypes.Structure):
    _fields_ = [("converged", ctypes.c_uint32), ("restarts", ctypes.c_uint32), ("matvecs", ctypes.c_uint32), ("m", ctypes.c_uint32),
                ("loop_ms", ctypes.c_double), ("spmv_ms", ctypes.c_double), ("orth_ms", ctypes.c_double), ("host_ms", ctypes.c_double),
                ("norm_est", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class LzxSolveInfo(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_uint32), ("launched", ctypes.c_uint32), ("converged", ctypes.c_uint32), ("ns", ctypes.c_uint32),
                ("loop_ms", ctypes.c_double), ("spmv_ms", ctypes.c_double), ("vec_ms", ctypes.c_double), ("bnorm", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class LzxSolveMultiInfo(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_uint32), ("launched", ctypes.c_uint32), ("converged", ctypes.c_uint32), ("nb", ctypes.c_uint32),
                ("loop_ms", ctypes.c_double), ("spmv_ms", ctypes.c_double), ("vec_ms", ctypes.c_double), ("bnorm", ctypes.c_double * 16)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["bnorm"] = np.array(list(d["bnorm"])[:d["nb"]])
        return d


class LzxPagerankInfo(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_uint32), ("launched", ctypes.c_uint32), ("converged", ctypes.c_uint32), ("nd", ctypes.c_uint32),
                ("loop_ms", ctypes.c_double), ("spmv_ms", ctypes.c_double), ("vec_ms", ctypes.c_double), ("mass", ctypes.c_double * 16)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["mass"] = np.array(list(d["mass"])[:d["nd"]])
        return d


class LzxComponentsInfo(ctypes.Structure):
    _fields_ = [("n_components", ctypes.c_uint64), ("largest_size", ctypes.c_uint64), ("largest_label", ctypes.c_uint32),
                ("rounds", ctypes.c_uint32), ("loop_ms", ctypes.c_double), ("sweep_ms", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class LzxBfsInfo(ctypes.Structure):
    _fields_ = [("ns", ctypes.c_uint32), ("batches", ctypes.c_uint32), ("max_level", ctypes.c_uint32), ("sweeps", ctypes.c_uint32),
                ("loop_ms", ctypes.c_double), ("sweep_ms", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class LzxBrandesInfo(ctypes.Structure):
    _fields_ = [("ns", ctypes.c_uint32), ("batches", ctypes.c_uint32), ("max_level", ctypes.c_uint32), ("sweeps", ctypes.c_uint32),
                ("loop_ms", ctypes.c_double), ("sweep_ms", ctypes.c_double), ("edge_ms", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class LzxTrianglesInfo(ctypes.Structure):
    _fields_ = [("triangles", ctypes.c_uint64), ("wedges", ctypes.c_uint64), ("max_triangles", ctypes.c_uint64),
                ("oriented_entries", ctypes.c_uint64), ("oriented_max_degree", ctypes.c_uint32), ("reserved_", ctypes.c_uint32),
                ("avg_clustering", ctypes.c_double), ("loop_ms", ctypes.c_double), ("orient_ms", ctypes.c_double), ("count_ms", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "reserved_"}


class LzxCoreInfo(ctypes.Structure):
    _fields_ = [("main_core_size", ctypes.c_uint64), ("core0", ctypes.c_uint64), ("degeneracy", ctypes.c_uint32), ("levels", ctypes.c_uint32),
                ("rounds", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("loop_ms", ctypes.c_double), ("peel_ms", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "reserved_"}


class LzxTrussInfo(ctypes.Structure):
    _fields_ = [("edges", ctypes.c_uint64), ("triangles", ctypes.c_uint64), ("main_truss_edges", ctypes.c_uint64),
                ("max_support", ctypes.c_uint32), ("max_truss", ctypes.c_uint32), ("levels", ctypes.c_uint32), ("rounds", ctypes.c_uint32),
                ("loop_ms", ctypes.c_double), ("support_ms", ctypes.c_double), ("peel_ms", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class LzxColorInfo(ctypes.Structure):
    _fields_ = [("colors", ctypes.c_uint32), ("rounds", ctypes.c_uint32), ("largest_class", ctypes.c_uint32), ("reserved_", ctypes.c_uint32),
                ("loop_ms", ctypes.c_double), ("color_ms", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "reserved_"}


class LzxCommunitiesInfo(ctypes.Structure):
    _fields_ = [("n_communities", ctypes.c_uint64), ("largest_size", ctypes.c_uint64), ("updates", ctypes.c_uint64),
                ("inner_entries", ctypes.c_uint64), ("entries", ctypes.c_uint64), ("sum_degree_sq", ctypes.c_uint64),
                ("largest_label", ctypes.c_uint32), ("sweeps", ctypes.c_uint32), ("colors", ctypes.c_uint32), ("color_rounds", ctypes.c_uint32),
                ("modularity", ctypes.c_double), ("loop_ms", ctypes.c_double), ("color_ms", ctypes.c_double), ("sweep_ms", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class LzxModularityInfo(ctypes.Structure):
    _fields_ = [("communities", ctypes.c_uint64), ("inner_entries", ctypes.c_uint64), ("entries", ctypes.c_uint64),
                ("sum_degree_sq", ctypes.c_uint64), ("loop_ms", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class LzxLouvainLevel(ctypes.Structure):
    _fields_ = [("nodes", ctypes.c_uint64), ("entries", ctypes.c_uint64), ("communities", ctypes.c_uint64), ("moves", ctypes.c_uint64),
                ("inner_entries", ctypes.c_uint64), ("sum_degree_sq", ctypes.c_uint64), ("colors", ctypes.c_uint32), ("color_rounds", ctypes.c_uint32),
                ("sweeps", ctypes.c_uint32), ("reverted", ctypes.c_uint32), ("capped", ctypes.c_uint32), ("path_rows", ctypes.c_uint32 * 3)]

    def as_dict(self):
        return {f: (list(getattr(self, f)) if f == "path_rows" else getattr(self, f)) for f, _ in self._fields_}


class LzxLouvainInfo(ctypes.Structure):
    _fields_ = [("n_communities", ctypes.c_uint64), ("largest_size", ctypes.c_uint64), ("sweeps", ctypes.c_uint64), ("moves", ctypes.c_uint64),
                ("inner_entries", ctypes.c_uint64), ("entries", ctypes.c_uint64), ("sum_degree_sq", ctypes.c_uint64),
                ("largest_label", ctypes.c_uint32), ("levels", ctypes.c_uint32), ("modularity", ctypes.c_double), ("loop_ms", ctypes.c_double),
                ("color_ms", ctypes.c_double), ("sweep_ms", ctypes.c_double), ("aggregate_ms", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class LzxSweepResult(ctypes.Structure):
    _fields_ = [("k", ctypes.c_uint64), ("cut", ctypes.c_uint64), ("vol", ctypes.c_uint64), ("den", ctypes.c_uint64), ("value", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class LzxSweepInfo(ctypes.Structure):
    _fields_ = [("entries", ctypes.c_uint64), ("ns", ctypes.c_uint32), ("width", ctypes.c_uint32), ("loop_ms", ctypes.c_double),
                ("sort_ms", ctypes.c_double), ("sweep_ms", ctypes.c_double), ("scan_ms", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class LzxSimilarityInfo(ctypes.Structure):
    _fields_ = [("pairs", ctypes.c_uint64), ("walked", ctypes.c_uint64), ("short_pairs", ctypes.c_uint64), ("long_pairs", ctypes.c_uint64),
                ("sliced_pairs", ctypes.c_uint64), ("max_common", ctypes.c_uint32), ("lanes", ctypes.c_uint32),
                ("loop_ms", ctypes.c_double), ("prep_ms", ctypes.c_double), ("count_ms", ctypes.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


# every symbol include/lzx.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("lzx_create", ctypes.c_int, [_hp, ctypes.c_int]),
    ("lzx_destroy", None, [_h]),
    ("lzx_last_error", ctypes.c_char_p, []),
    ("lzx_comm_unique_id", ctypes.c_int, [_u8p]),
    ("lzx_comm_init_rank", ctypes.c_int, [_h, _u8p, ctypes.c_int, ctypes.c_int]),
    ("lzx_comm_init_local", ctypes.c_int, [_hp, ctypes.c_int]),
    ("lzx_create_group", ctypes.c_int, [_hp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    ("lzx_comm_ipc_export", ctypes.c_int, [_h, _u8p]),
    ("lzx_comm_ipc_init", ctypes.c_int, [_h, _u8p, ctypes.c_int, ctypes.c_int]),
    ("lzx_set_graph_csr", ctypes.c_int, [_h, ctypes.c_uint64, ctypes.c_uint64, _u64p, _u32p]),
    ("lzx_set_graph_csr32", ctypes.c_int, [_h, ctypes.c_uint32, ctypes.c_uint32, _u32p, _u32p]),
    ("lzx_set_graph_edges", ctypes.c_int, [_h, ctypes.c_uint64, ctypes.c_uint64, _u32p, _u32p]),
    ("lzx_gen_graph", ctypes.c_int, [_h, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                                     ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]),
    ("lzx_get_graph_info", ctypes.c_int, [_h, ctypes.POINTER(LzxGraphInfo)]),
    ("lzx_get_graph_csr", ctypes.c_int, [_h, _u64p, _u32p]),
    ("lzx_spmv_f64", ctypes.c_int, [_h, _f64p, _f64p]),
    ("lzx_spmv_f64_local", ctypes.c_int, [_hp, ctypes.c_int, _f64p, _f64p]),
    ("lzx_lanczos_f64", ctypes.c_int, [_h, _f64p, ctypes.c_uint32, _f64p, _f64p, _f64p, _f64p,
                                       ctypes.POINTER(LzxStats)]),
    ("lzx_lanczos_f64_local", ctypes.c_int, [_hp, ctypes.c_int, _f64p, ctypes.c_uint32, _f64p, _f64p, _f64p,
                                             _f64p, ctypes.POINTER(LzxStats)]),
    ("lzx_lanczos_prepare_f64", ctypes.c_int, [_h, _f64p, ctypes.c_uint32, _f64p]),
    ("lzx_lanczos_run", ctypes.c_int, [_h, ctypes.POINTER(LzxStats)]),
    ("lzx_lanczos_fetch_f64", ctypes.c_int, [_h, ctypes.c_uint32, _f64p, _f64p, _f64p]),
    ("lzx_lanczos_fetch_f64_local", ctypes.c_int, [_hp, ctypes.c_int, ctypes.c_uint32, _f64p, _f64p, _f64p]),
    ("lzx_lanczos_run_steps", ctypes.c_int, [_h, ctypes.c_uint32, ctypes.POINTER(LzxStats)]),
    ("lzx_lanczos_run_steps_local", ctypes.c_int, [_hp, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(LzxStats)]),
    ("lzx_lanczos_prepare_f64_local", ctypes.c_int, [_hp, ctypes.c_int, _f64p, ctypes.c_uint32, _f64p]),
    ("lzx_lanczos_progress", ctypes.c_int, [_h, _u32p, _u32p]),
    ("lzx_multout_change_f64", ctypes.c_int, [_h, _f64p, ctypes.c_uint32, _f64p]),
    ("lzx_multout_change_f64_local", ctypes.c_int, [_hp, ctypes.c_int, _f64p, ctypes.c_uint32, _f64p]),
    ("lzx_device_count", ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    ("lzx_sync", ctypes.c_int, [_h]),
    ("lzx_multout_f64", ctypes.c_int, [_h, _f64p, ctypes.c_uint32, _f64p]),
    ("lzx_multout_f64_local", ctypes.c_int, [_hp, ctypes.c_int, _f64p, ctypes.c_uint32, _f64p]),
    ("lzx_bench_spmv", ctypes.c_int, [_h, ctypes.c_uint32, _f64p, _f64p]),
    ("lzx_bench_stream", ctypes.c_int, [_h, ctypes.c_uint64, ctypes.c_uint32, _f64p, _f64p]),
    ("lzx_set_option", ctypes.c_int, [_h, ctypes.c_char_p, ctypes.c_int64]),
    ("lzx_lanczos_multi_f64", ctypes.c_int, [_h, ctypes.c_uint32, _f64p, ctypes.c_uint32, _f64p, _f64p, _u32p, _f64p, _f64p,
                                             ctypes.POINTER(LzxStats)]),
    ("lzx_multout_multi_f64", ctypes.c_int, [_h, ctypes.c_uint32, _f64p, ctypes.c_uint32, _f64p]),
    ("lzx_spmm_f64", ctypes.c_int, [_h, ctypes.c_uint32, _f64p, _f64p]),
    ("lzx_multi_release", ctypes.c_int, [_h]),
    ("lzx_probes_f64", ctypes.c_int, [_h, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, _f64p]),
    ("lzx_lanczos_probes_f64", ctypes.c_int, [_h, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                              _f64p, _f64p, _u32p, ctypes.POINTER(LzxStats)]),
    ("lzx_probe_diag_f64", ctypes.c_int, [_h, _f64p, ctypes.c_uint32, _f64p]),
    ("lzx_eigsh_f64", ctypes.c_int, [_h, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_double, ctypes.c_uint32, _f64p,
                                     ctypes.c_uint64, _f64p, ctypes.c_uint32, _f64p, _f64p, _f64p, ctypes.POINTER(LzxEigInfo)]),
    ("lzx_solve_shifted_f64", ctypes.c_int, [_h, _f64p, ctypes.c_uint32, _f64p, ctypes.c_double, ctypes.c_uint32, _f64p, ctypes.c_uint32,
                                             _f64p, _u32p, _f64p, ctypes.POINTER(LzxSolveInfo)]),
    ("lzx_solve_multi_f64", ctypes.c_int, [_h, ctypes.c_uint32, _f64p, _f64p, ctypes.c_double, ctypes.c_uint32, _f64p, ctypes.c_uint32,
                                           _f64p, _u32p, _f64p, _u32p, ctypes.POINTER(LzxSolveMultiInfo)]),
    ("lzx_pagerank_f64", ctypes.c_int, [_h, _f64p, ctypes.c_uint32, _f64p, ctypes.c_double, ctypes.c_uint32, _f64p, _u32p, _f64p,
                                        ctypes.POINTER(LzxPagerankInfo)]),
    ("lzx_components", ctypes.c_int, [_h, _u32p, ctypes.POINTER(LzxComponentsInfo)]),
    ("lzx_set_graph_induced", ctypes.c_int, [_h, _h, _u8p, _u32p, _u64p]),
    ("lzx_bfs_multi", ctypes.c_int, [_h, ctypes.c_uint32, _u32p, _i32p, _f64p, _u64p, _u64p, _f64p, _u32p, ctypes.POINTER(LzxBfsInfo)]),
    ("lzx_betweenness_f64", ctypes.c_int, [_h, ctypes.c_uint32, _u32p, _f64p, ctypes.POINTER(LzxBfsInfo)]),
    ("lzx_brandes_f64", ctypes.c_int, [_h, ctypes.c_uint32, _u32p, ctypes.c_uint32, _f64p, _f64p, ctypes.POINTER(LzxBrandesInfo)]),
    ("lzx_triangles", ctypes.c_int, [_h, _u64p, _f64p, ctypes.POINTER(LzxTrianglesInfo)]),
    ("lzx_core_numbers", ctypes.c_int, [_h, _u32p, _u32p, ctypes.POINTER(LzxCoreInfo)]),
    ("lzx_truss", ctypes.c_int, [_h, _u32p, _u32p, _u32p, _u32p, ctypes.POINTER(LzxTrussInfo)]),
    ("lzx_color", ctypes.c_int, [_h, ctypes.c_uint64, ctypes.c_uint32, _u32p, ctypes.POINTER(LzxColorInfo)]),
    ("lzx_label_propagation", ctypes.c_int, [_h, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _u32p, ctypes.POINTER(LzxCommunitiesInfo)]),
    ("lzx_modularity", ctypes.c_int, [_h, _u32p, _f64p, ctypes.POINTER(LzxModularityInfo)]),
    ("lzx_louvain", ctypes.c_int, [_h, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _u32p, _u32p, ctypes.POINTER(LzxLouvainLevel),
                                   ctypes.POINTER(LzxLouvainInfo)]),
    ("lzx_sweep_cut", ctypes.c_int, [_h, ctypes.c_uint32, _f64p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, _u32p, _u64p, _u64p,
                                     ctypes.POINTER(LzxSweepResult), ctypes.POINTER(LzxSweepInfo)]),
    ("lzx_similarity", ctypes.c_int, [_h, ctypes.c_uint64, _u32p, _u32p, ctypes.c_uint32, _u32p, _u32p, _u32p, _f64p,
                                      ctypes.POINTER(LzxSimilarityInfo)]),
]

_LIB = None
_DBG_LIB = None


class LzxError(RuntimeError):
    pass


def _load(path: str, mode: int) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise LzxError(f"{path} is missing: run __graft_entry__.build() (make -C {_HERE})")
    L = ctypes.CDLL(path, mode=mode)
    for name, res, args in SYMBOLS:
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    L.lzx_test_set_shape.restype = ctypes.c_int       # test hook, not in include/lzx.h
    L.lzx_test_set_shape.argtypes = [_h, ctypes.c_char_p, ctypes.c_int64]
    L.lzx_test_get_shape.restype = ctypes.c_int
    L.lzx_test_get_shape.argtypes = [_h, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]
    L.lzx_test_allreduce_latency.restype = ctypes.c_int
    L.lzx_test_allreduce_latency.argtypes = [_h, ctypes.c_uint32, ctypes.POINTER(ctypes.c_double)]
    L.lzx_test_rank_row_sums.restype = ctypes.c_int
    L.lzx_test_rank_row_sums.argtypes = [_h, _f64p, _u32p, _u64p]
    L.lzx_test_sym_eig.restype = ctypes.c_int          # the eigensolver's dense solver (csrc/lzx_test_hooks.h)
    L.lzx_test_sym_eig.argtypes = [ctypes.c_uint32, _f64p, _f64p, _f64p]
    L.lzx_test_eig_ops.restype = ctypes.c_int          # the eigensolver's dense device kernels on a caller's basis
    L.lzx_test_eig_ops.argtypes = [_h, ctypes.c_uint32, ctypes.c_uint32, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p]
    return L


def lib(debug: bool = False) -> ctypes.CDLL:
    """liblzx.so (the product), or liblzx_dbg.so when debug-only options are wanted; raises if it has not been
    built (no fallback).  Both are linked -Bsymbolic, so they can be loaded side by side."""
    global _LIB, _DBG_LIB
    if debug:
        if _DBG_LIB is None:
            _DBG_LIB = _load(DBG_LIB_PATH, ctypes.RTLD_LOCAL)
        return _DBG_LIB
    if _LIB is None:
        _LIB = _load(LIB_PATH, ctypes.RTLD_GLOBAL)
    return _LIB


def _p(a, ty):
    return a.ctypes.data_as(ty)


def _check(rc: int, what: str, L=None):
    if rc != 0:
        raise LzxError(f"{what} failed ({rc}): {(L or lib()).lzx_last_error().decode(errors='replace')}")


# values of the option "operator" (include/lzx.h)
OP_ADJACENCY = 0
OP_LAPLACIAN = 1


def _expm_coefficients(alpha, beta, x_norm, s):
    """t = V (e^{s theta} .* ||x|| V[0, :]) of the tridiagonal T (host/multiplyOut.cc: small_part), T trimmed at the first zero
    beta (under L the breakdown stop returns every later coefficient and basis column as 0); zeros behind the trimmed block."""
    k = len(alpha)
    kb = k
    zero = np.flatnonzero(np.asarray(beta[:k - 1]) == 0.0)
    if zero.size:
        kb = int(zero[0]) + 1
    T = np.diag(np.asarray(alpha[:kb], dtype=np.float64))
    if kb > 1:
        T += np.diag(beta[:kb - 1], 1) + np.diag(beta[:kb - 1], -1)
    lam, V = np.linalg.eigh(T)
    t = np.zeros(k)
    t[:kb] = V @ (np.exp(s * lam) * (x_norm * V[0, :]))
    return t


# ---- stochastic Lanczos quadrature (include/lzx.h: lzx_lanczos_probes_f64) ----
PROBE_KEEP_BASIS = 1   # LZX_PROBE_KEEP_BASIS
EIG_LARGEST = 0        # LZX_EIG_LARGEST
EIG_SMALLEST = 1       # LZX_EIG_SMALLEST
ERR_LIMIT = -6         # LZX_ERR_LIMIT
PROBE_BATCH = 16       # probes per batched decomposition


def _probe_ritz(alpha, beta, m):
    """Eigenpairs (theta, V) of one probe's tridiagonal T trimmed to its m = k_used coefficients."""
    T = np.diag(np.asarray(alpha[:m], dtype=np.float64))
    if m > 1:
        T += np.diag(beta[:m - 1], 1) + np.diag(beta[:m - 1], -1)
    return np.linalg.eigh(T)


def _logsumexp(x):
    m = x.max()
    return m + np.log(np.sum(np.exp(x - m)))


def slq_log_quadratures(alpha, beta, k_used, n, s):
    """ell[i, p] = log(z_p^T e^{s_i M} z_p) by the Gauss quadrature of probe p's T (alpha, beta: (P, k); k_used: (P,)):
    log n + logsumexp_j(log w_j + s_i theta_j), w_j = V[0, j]^2 > 0 -- finite where e^{s theta} itself overflows.  Each
    (s_i, p) is computed on its own, so a grid of s gives the bits of one s at a time."""
    s = np.atleast_1d(np.asarray(s, dtype=np.float64))
    alpha, beta = np.atleast_2d(alpha), np.atleast_2d(beta)
    ell = np.empty((len(s), alpha.shape[0]))
    for p in range(alpha.shape[0]):
        theta, V = _probe_ritz(alpha[p], beta[p], int(k_used[p]))
        w = V[0, :] ** 2
        keep = w > 0.0
        logw, theta = np.log(w[keep]), theta[keep]
        for i, si in enumerate(s):
            ell[i, p] = np.log(float(n)) + _logsumexp(logw + si * theta)
    return ell


def slq_trace(ell):
    """From ell (S, N) of slq_log_quadratures: (log_trace[S], rel_stderr[S]) with log_trace = logsumexp_p ell_p - log N, the
    log of the Hutchinson mean, and rel_stderr = std(e^{ell - max ell}, ddof=1) / (sqrt(N) mean(e^{ell - max ell}))."""
    ell = np.atleast_2d(ell)
    N = ell.shape[1]
    log_trace, rel = np.empty(ell.shape[0]), np.empty(ell.shape[0])
    for i, e in enumerate(ell):
        log_trace[i] = _logsumexp(e) - np.log(float(N))
        r = np.exp(e - e.max())
        rel[i] = np.std(r, ddof=1) / (np.sqrt(N) * np.mean(r)) if N > 1 else np.nan
    return log_trace, rel


def slq_diag_coefficients(alpha, beta, k_used, n, s, shift):
    """T[p] = V (e^{s (theta - shift)} .* sqrt(n) V[0, :]) of probe p's trimmed T, zeros behind k_used[p]: the weights with
    which Q_p T[p] = e^{s (M - shift I)} z_p (||z_p|| = sqrt(n)), for lzx_probe_diag_f64."""
    alpha, beta = np.atleast_2d(alpha), np.atleast_2d(beta)
    T = np.zeros(alpha.shape)
    for p in range(alpha.shape[0]):
        m = int(k_used[p])
        theta, V = _probe_ritz(alpha[p], beta[p], m)
        T[p, :m] = V @ (np.exp(s * (theta - shift)) * (np.sqrt(float(n)) * V[0, :]))
    return T


def rmat_thresholds(a=0.57, b=0.19, c=0.19):
    return int(round(a * 65536)), int(round((a + b) * 65536)), int(round((a + b + c) * 65536))


class Engine:
    """One lzx handle (one GPU)."""

    def __init__(self, device: int = 0, **options):
        self.h = ctypes.c_void_p()
        self.device = device
        self.operator = OP_ADJACENCY
        self.debug = any(k not in PRODUCT_OPTIONS and k not in SHAPE_OPTIONS for k in options)   # experiment knobs: liblzx_dbg.so
        self.L = lib(debug=self.debug)
        _check(self.L.lzx_create(ctypes.byref(self.h), device), "lzx_create", self.L)
        for k, v in options.items():
            self.set_option(k, v)
        self.n = 0

    def set_option(self, name: str, value: int):
        if name in SHAPE_OPTIONS and not self.debug:
            _check(self.L.lzx_test_set_shape(self.h, name.encode(), int(value)), f"lzx_test_set_shape({name})", self.L)
            return
        _check(self.L.lzx_set_option(self.h, name.encode(), int(value)), f"lzx_set_option({name})", self.L)
        if name == "operator":
            self.operator = int(value)

    def shape(self, name: str) -> int:
        """what shape the blocked tables took (test hook lzx_test_get_shape): gather_items_dealt / _drawn, gather_workgroups,
        finish_launched / _deferrable, row_bands, pb_runs, pb_steps, scatter_units, ...; and the body and split rows of either mode:
        split_rows, split_items, body_slices, slices_wide / _w8 / _w4 / _w0, staged_workgroups, split_entries, body_entries,
        staged_x_stride, live_rows; and the batched path's work list, 0 until its first call on the graph: multi_chunk,
        multi_work_items, multi_split_rows, multi_chunk_slots, multi_row_segments, multi_vector_grid (csrc/lzx_test_hooks.h)"""
        v = ctypes.c_int64()
        _check(self.L.lzx_test_get_shape(self.h, name.encode(), ctypes.byref(v)), f"lzx_test_get_shape({name})", self.L)
        return int(v.value)

    def rank_row_sums(self):
        """test hook lzx_test_rank_row_sums: (row sums of this rank's own rows from its local SpMV of x = 1, caller's vertex id of
        every local row) -- a rank's share checked without its peers"""
        gi = self.info()
        v = np.empty(max(gi["rows_local"], 1))
        pos = np.empty(gi["n"], dtype=np.uint32)
        pad = ctypes.c_uint64()
        _check(self.L.lzx_test_rank_row_sums(self.h, _p(v, _f64p), _p(pos, _u32p), ctypes.byref(pad)), "lzx_test_rank_row_sums", self.L)
        lo = gi["rank"] * pad.value
        mine = np.flatnonzero((pos >= lo) & (pos < lo + gi["rows_local"]))
        ids = np.empty(gi["rows_local"], dtype=np.int64)
        ids[pos[mine].astype(np.int64) - lo] = mine
        return v[:gi["rows_local"]], ids

    def eig_ops(self, Q, w, Y=None):
        """test hook lzx_test_eig_ops: the eigensolver's Gram-Schmidt launches on the columns of Q (n, J) and w (n,), and with
        Y (J, p) its restart rotation.  Returns (coef (J,) = h1 + h2, w_out (n,) unit, beta, R (p, n) = (Q Y)^T or None)."""
        Qt = np.ascontiguousarray(np.asarray(Q, dtype=np.float64).T)
        w = np.ascontiguousarray(w, dtype=np.float64)
        J, n = Qt.shape
        assert n == self.n and w.shape == (n,)
        Yc = None if Y is None else np.ascontiguousarray(Y, dtype=np.float64)
        assert Yc is None or (Yc.ndim == 2 and Yc.shape[0] == J)
        p = 1 if Yc is None else Yc.shape[1]
        coef, w_out, beta = np.zeros(J), np.zeros(n), ctypes.c_double()
        R = None if Yc is None else np.zeros((p, n))
        _check(self.L.lzx_test_eig_ops(self.h, J, p, _p(Qt, _f64p), _p(w, _f64p), None if Yc is None else _p(Yc, _f64p), _p(coef, _f64p),
                                       _p(w_out, _f64p), ctypes.byref(beta), None if R is None else _p(R, _f64p)), "lzx_test_eig_ops", self.L)
        return coef, w_out, float(beta.value), R

    def close(self):
        if self.h:
            self.L.lzx_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- communicator ----
    @staticmethod
    def unique_id() -> np.ndarray:
        uid = np.zeros(128, dtype=np.uint8)
        _check(lib().lzx_comm_unique_id(_p(uid, _u8p)), "lzx_comm_unique_id")
        return uid

    def comm_init_rank(self, uid: np.ndarray, rank: int, world: int):
        uid = np.ascontiguousarray(uid, dtype=np.uint8)
        _check(self.L.lzx_comm_init_rank(self.h, _p(uid, _u8p), rank, world), "lzx_comm_init_rank", self.L)

    IPC_BLOB = 128   # LZX_IPC_BLOB

    def allreduce_latency(self, reps: int = 1000) -> float:
        """test hook lzx_test_allreduce_latency: microseconds per two-double all-reduce of the wired communicator (collective)."""
        us = ctypes.c_double()
        _check(self.L.lzx_test_allreduce_latency(self.h, reps, ctypes.byref(us)), "lzx_test_allreduce_latency", self.L)
        return us.value

    def comm_ipc_export(self) -> np.ndarray:
        """This rank's window for the peer-window transport (include/lzx.h): 128 bytes to be gathered from all ranks."""
        blob = np.zeros(self.IPC_BLOB, dtype=np.uint8)
        _check(self.L.lzx_comm_ipc_export(self.h, _p(blob, _u8p)), "lzx_comm_ipc_export", self.L)
        return blob

    def comm_ipc_init(self, blobs: np.ndarray, rank: int, world: int):
        blobs = np.ascontiguousarray(blobs, dtype=np.uint8).reshape(-1)
        if blobs.size != world * self.IPC_BLOB:
            raise ValueError(f"comm_ipc_init: {world} ranks need {world * self.IPC_BLOB} bytes of exports, got {blobs.size}")
        _check(self.L.lzx_comm_ipc_init(self.h, _p(blobs, _u8p), rank, world), "lzx_comm_ipc_init", self.L)

    # ---- graph ----
    def set_graph_csr(self, row_ptr, col_idx):
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        col_idx = np.ascontiguousarray(col_idx, dtype=np.uint32)
        n, nnz = len(row_ptr) - 1, len(col_idx)
        ci = col_idx if nnz else np.zeros(1, dtype=np.uint32)
        _check(self.L.lzx_set_graph_csr(self.h, n, nnz, _p(row_ptr, _u64p), _p(ci, _u32p)), "lzx_set_graph_csr", self.L)
        self.n = n

    def set_graph_csr32(self, row_ptr, col_idx):
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint32)
        col_idx = np.ascontiguousarray(col_idx, dtype=np.uint32)
        n, nnz = len(row_ptr) - 1, len(col_idx)
        ci = col_idx if nnz else np.zeros(1, dtype=np.uint32)
        _check(self.L.lzx_set_graph_csr32(self.h, n, nnz, _p(row_ptr, _u32p), _p(ci, _u32p)), "lzx_set_graph_csr32", self.L)
        self.n = n

    def set_graph_edges(self, n, src, dst):
        src = np.ascontiguousarray(src, dtype=np.uint32)
        dst = np.ascontiguousarray(dst, dtype=np.uint32)
        assert len(src) == len(dst)
        s = src if len(src) else np.zeros(1, dtype=np.uint32)
        d = dst if len(dst) else np.zeros(1, dtype=np.uint32)
        _check(self.L.lzx_set_graph_edges(self.h, n, len(src), _p(s, _u32p), _p(d, _u32p)), "lzx_set_graph_edges", self.L)
        self.n = n

    def gen_er(self, n, draws, seed):
        _check(self.L.lzx_gen_graph(self.h, 0, 0, n, draws, seed, 0, 0, 0), "lzx_gen_graph(er)", self.L)
        self.n = n

    def gen_rmat(self, scale, n, draws, seed, a=0.57, b=0.19, c=0.19):
        ta, tab, tabc = rmat_thresholds(a, b, c)
        _check(self.L.lzx_gen_graph(self.h, 1, scale, n, draws, seed, ta, tab, tabc), "lzx_gen_graph(rmat)", self.L)
        self.n = n

    def info(self) -> dict:
        gi = LzxGraphInfo()
        _check(self.L.lzx_get_graph_info(self.h, ctypes.byref(gi)), "lzx_get_graph_info", self.L)
        return gi.as_dict()

    def get_graph_csr(self):
        gi = self.info()
        rp = np.empty(gi["n"] + 1, dtype=np.uint64)
        ci = np.empty(max(gi["nnz"], 1), dtype=np.uint32)
        _check(self.L.lzx_get_graph_csr(self.h, _p(rp, _u64p), _p(ci, _u32p)), "lzx_get_graph_csr", self.L)
        return rp, ci[:gi["nnz"]]

    # ---- hot path ----
    def spmv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert len(x) == self.n
        y = np.empty(self.n)
        _check(self.L.lzx_spmv_f64(self.h, _p(x, _f64p), _p(y, _f64p)), "lzx_spmv_f64", self.L)
        return y

    def lanczos(self, x0, k: int, want_q: bool = True):
        """Returns (alpha[k], beta[k-1], Q (k, n) or None, x_norm, stats dict)."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        assert len(x0) == self.n
        alpha = np.zeros(k)
        beta = np.zeros(max(k - 1, 1))
        Q = np.empty((k, self.n)) if want_q else None
        xn = ctypes.c_double()
        st = LzxStats()
        _check(self.L.lzx_lanczos_f64(self.h, _p(x0, _f64p), k, _p(alpha, _f64p), _p(beta, _f64p),
                                     _p(Q, _f64p) if want_q else None, ctypes.byref(xn), ctypes.byref(st)),
               "lzx_lanczos_f64", self.L)
        return alpha, beta[:k - 1], Q, xn.value, st.as_dict()

    def lanczos_prepare(self, x0, k: int) -> float:
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        assert len(x0) == self.n
        xn = ctypes.c_double()
        _check(self.L.lzx_lanczos_prepare_f64(self.h, _p(x0, _f64p), k, ctypes.byref(xn)), "lzx_lanczos_prepare_f64", self.L)
        return xn.value

    def lanczos_run(self) -> dict:
        st = LzxStats()
        _check(self.L.lzx_lanczos_run(self.h, ctypes.byref(st)), "lzx_lanczos_run", self.L)
        return st.as_dict()

    def lanczos_run_steps(self, steps: int) -> dict:
        """Up to `steps` more iterations of the prepared decomposition (lzx_lanczos_run_steps)."""
        st = LzxStats()
        _check(self.L.lzx_lanczos_run_steps(self.h, steps, ctypes.byref(st)), "lzx_lanczos_run_steps", self.L)
        return st.as_dict()

    def lanczos_progress(self):
        done, prep = ctypes.c_uint32(), ctypes.c_uint32()
        _check(self.L.lzx_lanczos_progress(self.h, ctypes.byref(done), ctypes.byref(prep)), "lzx_lanczos_progress", self.L)
        return done.value, prep.value

    def multout_change(self, t) -> float:
        t = np.ascontiguousarray(t, dtype=np.float64)
        rc = ctypes.c_double()
        _check(self.L.lzx_multout_change_f64(self.h, _p(t, _f64p), len(t), ctypes.byref(rc)), "lzx_multout_change_f64", self.L)
        return rc.value

    def lanczos_fetch(self, k: int, want_q: bool = False):
        alpha = np.zeros(k)
        beta = np.zeros(max(k - 1, 1))
        Q = np.empty((k, self.n)) if want_q else None
        _check(self.L.lzx_lanczos_fetch_f64(self.h, k, _p(alpha, _f64p), _p(beta, _f64p),
                                           _p(Q, _f64p) if want_q else None), "lzx_lanczos_fetch_f64", self.L)
        return alpha, beta[:k - 1], Q

    def sync(self):
        _check(self.L.lzx_sync(self.h), "lzx_sync", self.L)

    def multout(self, t):
        t = np.ascontiguousarray(t, dtype=np.float64)
        ans = np.empty(self.n)
        _check(self.L.lzx_multout_f64(self.h, _p(t, _f64p), len(t), _p(ans, _f64p)), "lzx_multout_f64", self.L)
        return ans

    def expm_multiply(self, x0, k: int, t: float = 1.0):
        """e^{tA} x0 (operator adjacency) or the heat kernel e^{-tL} x0 (operator laplacian): k Lanczos iterations, the small
        eigenproblem on the host, the answer formed from the resident basis (lzx_multout_f64)."""
        alpha, beta, _, xn, _ = self.lanczos(x0, k, want_q=False)
        s = -t if self.operator == OP_LAPLACIAN else t
        return self.multout(_expm_coefficients(alpha, beta, xn, s))

    # ---- batched, independent Lanczos (include/lzx.h: up to 16 starting vectors, one SpMM per iteration) ----
    def _batch(self, X, what):
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[1] != self.n:
            raise ValueError(f"{what}: X must be a (b, n) array with n = {self.n}, got shape {X.shape}")
        return X

    def lanczos_multi(self, X0, k: int, want_q: bool = False):
        """Returns (alpha[b,k], beta[b,k] (beta[:, k-1] = 0), k_used[b], x_norm[b], Q (b, k, n) or None, stats dict)."""
        X0 = self._batch(X0, "lanczos_multi")
        b = X0.shape[0]
        alpha, beta = np.zeros((b, k)), np.zeros((b, k))
        k_used, xn = np.zeros(b, dtype=np.uint32), np.zeros(b)
        Q = np.empty((b, k, self.n)) if want_q else None
        st = LzxStats()
        _check(self.L.lzx_lanczos_multi_f64(self.h, b, _p(X0, _f64p), k, _p(alpha, _f64p), _p(beta, _f64p), _p(k_used, _u32p),
                                           _p(xn, _f64p), _p(Q, _f64p) if want_q else None, ctypes.byref(st)),
               "lzx_lanczos_multi_f64", self.L)
        return alpha, beta, k_used, xn, Q, st.as_dict()

    def multout_multi(self, T):
        """ans[b, n] = Q_c t_c per column on the resident batch basis (T: (b, k))."""
        T = np.ascontiguousarray(T, dtype=np.float64)
        if T.ndim != 2:
            raise ValueError(f"multout_multi: T must be a (b, k) array, got shape {T.shape}")
        ans = np.empty((T.shape[0], self.n))
        _check(self.L.lzx_multout_multi_f64(self.h, T.shape[0], _p(T, _f64p), T.shape[1], _p(ans, _f64p)), "lzx_multout_multi_f64", self.L)
        return ans

    def spmm(self, X):
        """Y[b, n] = A X[b, n] (the batched SpMM)."""
        X = self._batch(X, "spmm")
        Y = np.empty_like(X)
        _check(self.L.lzx_spmm_f64(self.h, X.shape[0], _p(X, _f64p), _p(Y, _f64p)), "lzx_spmm_f64", self.L)
        return Y

    def multi_release(self):
        _check(self.L.lzx_multi_release(self.h), "lzx_multi_release", self.L)

    # ---- stochastic Lanczos quadrature: tr and diag of e^{tA} / e^{-tL} from +-1 probes made on the device ----
    def probes(self, seed: int, first: int, b: int):
        """Z[b, n]: probes first .. first + b - 1 of seed (the hash of include/lzx.h, caller's vertex order)."""
        Z = np.empty((b, self.n))
        _check(self.L.lzx_probes_f64(self.h, seed, first, b, _p(Z, _f64p)), "lzx_probes_f64", self.L)
        return Z

    def lanczos_probes(self, seed: int, first: int, b: int, k: int, keep_basis: bool = False):
        """lanczos_multi(probes(seed, first, b), k) without the upload, basis-free unless keep_basis (then the basis is the
        resident batch basis, for probe_diag and multout_multi).  Returns (alpha[b,k], beta[b,k], k_used[b], stats dict);
        every x_norm is sqrt(n)."""
        alpha, beta = np.zeros((b, k)), np.zeros((b, k))
        k_used = np.zeros(b, dtype=np.uint32)
        st = LzxStats()
        _check(self.L.lzx_lanczos_probes_f64(self.h, seed, first, b, k, PROBE_KEEP_BASIS if keep_basis else 0, _p(alpha, _f64p),
                                            _p(beta, _f64p), _p(k_used, _u32p), ctypes.byref(st)), "lzx_lanczos_probes_f64", self.L)
        return alpha, beta, k_used, st.as_dict()

    def probe_diag(self, T):
        """out[n] = sum over the resident probe batch's columns c (ascending) of z_c .* (Q_c T[c]) (T: (b, k))."""
        T = np.ascontiguousarray(T, dtype=np.float64)
        if T.ndim != 2:
            raise ValueError(f"probe_diag: T must be a (b, k) array, got shape {T.shape}")
        out = np.empty(self.n)
        _check(self.L.lzx_probe_diag_f64(self.h, _p(T, _f64p), T.shape[1], _p(out, _f64p)), "lzx_probe_diag_f64", self.L)
        return out

    def _probe_scale(self, t):
        return -t if self.operator == OP_LAPLACIAN else t

    def trace_expm(self, t, n_probes: int = 64, k: int = 50, seed: int = 0):
        """Stochastic Lanczos quadrature of tr e^{tA} (or the heat trace tr e^{-tL}) for a scalar t or a 1-D array of t, from
        one basis-free pass over n_probes probes in batches of 16.  Returns (log_trace, rel_stderr, ell): the log of the
        estimate, its relative standard error, and the per-probe log quadratures ell_p (shape (N,) for a scalar t, (len(t), N)
        otherwise).  The Estrada index is exp(log_trace) at t = 1; natural connectivity is log_trace - log n."""
        ts = np.asarray(t, dtype=np.float64)
        if ts.ndim > 1:
            raise ValueError(f"trace_expm: t must be a scalar or a 1-D array, got shape {ts.shape}")
        if n_probes < 1:
            raise ValueError("trace_expm: n_probes must be at least 1")
        s = self._probe_scale(np.atleast_1d(ts))
        ell = []
        for first in range(0, n_probes, PROBE_BATCH):
            b = min(PROBE_BATCH, n_probes - first)
            alpha, beta, k_used, _ = self.lanczos_probes(seed, first, b, k)
            ell.append(slq_log_quadratures(alpha, beta, k_used, self.n, s))
        ell = np.concatenate(ell, axis=1)
        log_trace, rel = slq_trace(ell)
        if ts.ndim == 0:
            return log_trace[0], rel[0], ell[0]
        return log_trace, rel, ell

    def diag_expm(self, t: float = 1.0, n_probes: int = 64, k: int = 50, seed: int = 0, shift=None):
        """Estimate of diag e^{s (M - shift I)} (s = t under A, -t under L): (1/N) sum_p z_p .* (e^{s (M - shift I)} z_p), each
        batch of 16 probes run with its basis kept and reduced on the device (probe_diag), the batch vectors added in batch
        order.  shift defaults to the largest Ritz value of the first batch under A (subgraph centrality without overflow) and
        to 0 under L.  Returns (estimate[n], shift); diag e^{sM} = estimate * e^{s shift}.  The last batch's basis stays resident."""
        if n_probes < 1:
            raise ValueError("diag_expm: n_probes must be at least 1")
        s = self._probe_scale(float(t))
        acc = None
        for first in range(0, n_probes, PROBE_BATCH):
            b = min(PROBE_BATCH, n_probes - first)
            alpha, beta, k_used, _ = self.lanczos_probes(seed, first, b, k, keep_basis=True)
            if shift is None:
                shift = 0.0 if self.operator == OP_LAPLACIAN else \
                    max(float(_probe_ritz(alpha[p], beta[p], int(k_used[p]))[0].max()) for p in range(b))
            d = self.probe_diag(slq_diag_coefficients(alpha, beta, k_used, self.n, s, shift))
            acc = d if acc is None else acc + d
        return acc / n_probes, float(shift)

    def eigsh(self, nev: int = 6, which: str = "LA", m: int = 0, tol: float = 1e-10, max_restarts: int = 300, x0=None, seed: int = 0,
              deflate=None, want_vectors: bool = True):
        """The nev algebraically largest ("LA") or smallest ("SA") eigenpairs of the handle's operator (A, or L under option
        operator = OP_LAPLACIAN) by thick-restart Lanczos on the device (lzx_eigsh_f64), in the shape scipy.sparse.linalg.eigsh
        returns: (w ascending, V (n, nev) with column i belonging to w[i], or None, info).  info: the lzx_eig_info fields plus
        "resid" (the true residuals ||M v - w v||, ordered like w).  deflate: vectors (nw, n) or (n,) every basis vector is kept
        orthogonal to.  Non-convergence within max_restarts raises LzxError with the partial (w, V, info) as `.partial`."""
        if which not in ("LA", "SA"):
            raise ValueError(f"which must be 'LA' or 'SA', not {which!r}")
        n = self.n
        x = None if x0 is None else np.ascontiguousarray(x0, dtype=np.float64)
        if x is not None:
            assert x.shape == (n,)
        W = None if deflate is None else np.ascontiguousarray(np.atleast_2d(deflate), dtype=np.float64)
        if W is not None:
            assert W.shape[1] == n
        nw = 0 if W is None else W.shape[0]
        evals = np.zeros(nev)
        evecs = np.zeros((nev, n)) if want_vectors else None
        resid = np.zeros(nev)
        info = LzxEigInfo()
        rc = self.L.lzx_eigsh_f64(self.h, nev, EIG_LARGEST if which == "LA" else EIG_SMALLEST, m, tol, max_restarts,
                                  None if x is None else _p(x, _f64p), seed, None if W is None else _p(W, _f64p), nw,
                                  _p(evals, _f64p), None if evecs is None else _p(evecs, _f64p), _p(resid, _f64p), ctypes.byref(info))
        o = slice(None, None, -1) if which == "LA" else slice(None)   # the library sorts wanted-most first; scipy ascending
        d = info.as_dict()
        d["resid"] = resid[o].copy()
        result = (evals[o].copy(), None if evecs is None else evecs[o].T.copy(), d)
        if rc == ERR_LIMIT and info.m > 0:   # (info is written only by a run that got as far as the restarts)
            err = LzxError(f"lzx_eigsh_f64 failed ({rc}): {self.L.lzx_last_error().decode(errors='replace')}")
            err.partial = result
            raise err
        _check(rc, "lzx_eigsh_f64", self.L)
        return result

    def solve_shifted(self, b, shifts, tol: float = 1e-10, maxiter: int = 1000, W=None):
        """x_s = S(sigma_s)^(-1) b for every shift by multi-shift CG on the device (lzx_solve_shifted_f64): S(sigma) = sigma I - A,
        or sigma I + L under option operator = OP_LAPLACIAN.  Returns (X, info): X of shape (n,) for a scalar shift, (ns, n)
        otherwise; info: the lzx_solve_info fields plus "iters" and "resid" (true relative residuals), one per shift.  W: (nw, n)
        or (n,) deflation vectors (b and every x_s are projected onto their complement).  If maxiter runs out first, LzxError
        carries the partial (X, info) as `.partial`."""
        n = self.n
        b = np.ascontiguousarray(b, dtype=np.float64)
        if b.shape != (n,):
            raise ValueError(f"solve_shifted: b must have shape ({n},), got {b.shape}")
        sh = np.asarray(shifts, dtype=np.float64)
        if sh.ndim > 1:
            raise ValueError(f"solve_shifted: shifts must be a scalar or a 1-D array, got shape {sh.shape}")
        s1 = np.ascontiguousarray(np.atleast_1d(sh))
        ns = len(s1)
        Wc = None if W is None else np.ascontiguousarray(np.atleast_2d(W), dtype=np.float64)
        if Wc is not None and Wc.shape[1] != n:
            raise ValueError(f"solve_shifted: W must have n = {n} columns, got shape {Wc.shape}")
        nw = 0 if Wc is None else Wc.shape[0]
        X = np.zeros((max(ns, 1), n))
        iters = np.zeros(max(ns, 1), dtype=np.uint32)
        resid = np.zeros(max(ns, 1))
        info = LzxSolveInfo()
        rc = self.L.lzx_solve_shifted_f64(self.h, _p(b, _f64p), ns, _p(s1, _f64p) if ns else None, tol, maxiter,
                                          None if Wc is None else _p(Wc, _f64p), nw, _p(X, _f64p), _p(iters, _u32p), _p(resid, _f64p),
                                          ctypes.byref(info))
        d = info.as_dict()
        d["iters"], d["resid"] = iters[:ns].copy(), resid[:ns].copy()
        result = (X[0].copy() if sh.ndim == 0 else X[:ns].copy(), d)
        if rc == ERR_LIMIT and info.launched > 0:   # (info is written only by a run that got through its iterations)
            err = LzxError(f"lzx_solve_shifted_f64 failed ({rc}): {self.L.lzx_last_error().decode(errors='replace')}")
            err.partial = result
            raise err
        _check(rc, "lzx_solve_shifted_f64", self.L)
        return result

    def solve_multi(self, B, shifts, tol: float = 1e-10, maxiter: int = 1000, W=None):
        """x_c = S(sigma_c)^(-1) b_c for up to 16 right-hand sides by a batch of independent CG solves that share one SpMM per
        iteration (lzx_solve_multi_f64): S(sigma) = sigma I - A, or sigma I + L under option operator = OP_LAPLACIAN.  B: (nb, n);
        shifts: a scalar (the same for every column) or nb values.  Returns (X, info): X of shape (nb, n); info: the
        lzx_solve_multi_info fields plus "iters", "resid" (true relative residuals) and "status" (0 converged, 1 maxiter reached,
        2 not positive definite), one per column.  W: (nw, n) or (n,) deflation vectors shared by all columns.  If maxiter runs
        out first, LzxError carries the partial (X, info) as `.partial`."""
        n = self.n
        Bc = np.ascontiguousarray(B, dtype=np.float64)
        if Bc.ndim != 2 or Bc.shape[1] != n:
            raise ValueError(f"solve_multi: B must be a (nb, n) array with n = {n}, got shape {Bc.shape}")
        nb = Bc.shape[0]
        sh = np.asarray(shifts, dtype=np.float64)
        if sh.ndim > 1 or (sh.ndim == 1 and len(sh) != nb):
            raise ValueError(f"solve_multi: shifts must be a scalar or have one value per row of B ({nb}), got shape {sh.shape}")
        s1 = np.ascontiguousarray(np.full(nb, float(sh)) if sh.ndim == 0 else sh)
        Wc = None if W is None else np.ascontiguousarray(np.atleast_2d(W), dtype=np.float64)
        if Wc is not None and Wc.shape[1] != n:
            raise ValueError(f"solve_multi: W must have n = {n} columns, got shape {Wc.shape}")
        nw = 0 if Wc is None else Wc.shape[0]
        X = np.zeros((max(nb, 1), n))
        iters = np.zeros(max(nb, 1), dtype=np.uint32)
        status = np.zeros(max(nb, 1), dtype=np.uint32)
        resid = np.zeros(max(nb, 1))
        info = LzxSolveMultiInfo()
        rc = self.L.lzx_solve_multi_f64(self.h, nb, _p(Bc, _f64p) if nb else None, _p(s1, _f64p) if nb else None, tol, maxiter,
                                        None if Wc is None else _p(Wc, _f64p), nw, _p(X, _f64p), _p(iters, _u32p), _p(resid, _f64p),
                                        _p(status, _u32p), ctypes.byref(info))
        d = info.as_dict()
        d["iters"], d["resid"], d["status"] = iters[:nb].copy(), resid[:nb].copy(), status[:nb].copy()
        result = (X[:nb].copy(), d)
        if rc != 0 and info.launched > 0:   # (info is written only by a run that got through its iterations)
            err = LzxError(f"lzx_solve_multi_f64 failed ({rc}): {self.L.lzx_last_error().decode(errors='replace')}")
            err.partial = result
            raise err
        _check(rc, "lzx_solve_multi_f64", self.L)
        return result

    def effective_resistance(self, pairs, tol: float = 1e-10, maxiter: int = 1000):
        """R_uv = (e_u - e_v)^T L+ (e_u - e_v) for every (u, v) of `pairs` ((m, 2) vertex ids), by solve_multi in batches of 16
        right-hand sides with sigma = 0 and W = 1 / sqrt(n).  Needs operator = OP_LAPLACIAN (ValueError otherwise) and a
        CONNECTED graph: on a graph in several pieces run it on largest_component() (or another induced piece), whose null space
        the constant vector spans.  A pair with u == v has resistance 0.  Returns an array of m values."""
        if self.operator != OP_LAPLACIAN:
            raise ValueError("effective_resistance: effective resistances are defined on the Laplacian; this engine's operator is the adjacency matrix")
        pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        n = self.n
        if pr.size and (pr.min() < 0 or pr.max() >= n):
            raise ValueError(f"effective_resistance: vertex ids must lie in [0, {n})")
        out = np.zeros(len(pr))
        todo = np.flatnonzero(pr[:, 0] != pr[:, 1])
        w = np.full(n, 1.0 / np.sqrt(n))
        for first in range(0, len(todo), 16):
            idx = todo[first:first + 16]
            Bm = np.zeros((len(idx), n))
            rows = np.arange(len(idx))
            Bm[rows, pr[idx, 0]] = 1.0
            Bm[rows, pr[idx, 1]] = -1.0
            X, _ = self.solve_multi(Bm, 0.0, tol=tol, maxiter=maxiter, W=w)
            out[idx] = X[rows, pr[idx, 0]] - X[rows, pr[idx, 1]]
        return out

    def katz(self, alpha=None, beta: float = 1.0, normalized: bool = True, factor: float = 0.85, tol: float = 1e-10, maxiter: int = 1000):
        """Katz centrality x = beta (I - alpha A)^(-1) 1 as networkx.katz_centrality_numpy defines it (normalised by
        sign(sum x) ||x||_2), by one multi-shift solve with sigma = 1 / alpha: x = (beta / alpha) S(sigma)^(-1) 1.  alpha=None:
        factor / lambda_max, lambda_max from eigsh(nev=1).  A list of alpha gives one row per alpha.  Adjacency operator only."""
        if self.operator != OP_ADJACENCY:
            raise ValueError("katz: Katz centrality is defined on the adjacency matrix; this engine's operator is the Laplacian")
        if alpha is None:
            lam = float(self.eigsh(nev=1, which="LA", want_vectors=False)[0][0])
            alpha = factor / lam
        al = np.asarray(alpha, dtype=np.float64)
        if al.ndim > 1 or np.any(~(al > 0)):
            raise ValueError("katz: alpha must be a positive scalar or a 1-D array of positive values")
        a1 = np.atleast_1d(al)
        X, _ = self.solve_shifted(np.ones(self.n), 1.0 / a1, tol=tol, maxiter=maxiter)
        X = X * (beta / a1)[:, None]
        if normalized:
            X = X / (np.sign(X.sum(axis=1)) * np.linalg.norm(X, axis=1))[:, None]
        return X[0] if al.ndim == 0 else X

    def pagerank(self, alpha=0.85, personalization=None, tol: float = 1e-10, maxiter: int = 1000):
        """PageRank x = y / sum(y), (I - alpha A W^(-1)) y = v, as networkx.pagerank defines it on an undirected graph (dangling
        mass back to v), by multi-shift CG in the degree inner product on the device (lzx_pagerank_f64).  personalization: (n,)
        non-negative teleport vector (scaled to sum 1), None = uniform.  A scalar alpha returns x of shape (n,); a sequence
        returns (X, info): X of shape (nd, n), info = the lzx_pagerank_info fields plus "iters" and "resid" (true L1 residuals),
        one per damping.  The engine's operator option is ignored.  If maxiter runs out first, LzxError carries the partial
        (X, info) as `.partial`."""
        n = self.n
        al = np.asarray(alpha, dtype=np.float64)
        if al.ndim > 1:
            raise ValueError(f"pagerank: alpha must be a scalar or a 1-D array, got shape {al.shape}")
        a1 = np.ascontiguousarray(np.atleast_1d(al))
        nd = len(a1)
        v = None if personalization is None else np.ascontiguousarray(personalization, dtype=np.float64)
        if v is not None and v.shape != (n,):
            raise ValueError(f"pagerank: personalization must have shape ({n},), got {v.shape}")
        X = np.zeros((max(nd, 1), n))
        iters = np.zeros(max(nd, 1), dtype=np.uint32)
        resid = np.zeros(max(nd, 1))
        info = LzxPagerankInfo()
        rc = self.L.lzx_pagerank_f64(self.h, None if v is None else _p(v, _f64p), nd, _p(a1, _f64p) if nd else None, tol, maxiter,
                                     _p(X, _f64p), _p(iters, _u32p), _p(resid, _f64p), ctypes.byref(info))
        d = info.as_dict()
        d["iters"], d["resid"] = iters[:nd].copy(), resid[:nd].copy()
        result = (X[:nd].copy(), d)
        if rc == ERR_LIMIT and info.launched > 0:   # (info is written only by a run that got through its iterations)
            err = LzxError(f"lzx_pagerank_f64 failed ({rc}): {self.L.lzx_last_error().decode(errors='replace')}")
            err.partial = result
            raise err
        _check(rc, "lzx_pagerank_f64", self.L)
        return result[0][0] if al.ndim == 0 else result

    # ---- connected components and induced subgraphs (include/lzx.h: lzx_components, lzx_set_graph_induced) ----
    def components(self, want_labels: bool = True):
        """Connected components on the device.  Returns (labels, info): labels[i] = the smallest vertex id of i's component (uint32,
        caller's order; None with want_labels=False, and then no n-vector leaves the device), info = the lzx_components_info
        fields (n_components, largest_size, largest_label, rounds, loop_ms, sweep_ms)."""
        labels = np.empty(self.n, dtype=np.uint32) if want_labels else None
        info = LzxComponentsInfo()
        _check(self.L.lzx_components(self.h, _p(labels, _u32p) if want_labels else None, ctypes.byref(info)), "lzx_components", self.L)
        return labels, info.as_dict()

    def _keep_mask(self, keep, what):
        keep = np.asarray(keep)
        if keep.shape != (self.n,):
            raise ValueError(f"{what}: keep must have shape ({self.n},), one entry per vertex, got {keep.shape}")
        return np.ascontiguousarray(keep != 0, dtype=np.uint8)

    def _induce_into(self, dst, keep, what):
        old = np.empty(max(int(np.count_nonzero(keep)), 1), dtype=np.uint32)
        n_new = ctypes.c_uint64()
        _check(self.L.lzx_set_graph_induced(dst.h, self.h, _p(keep, _u8p), _p(old, _u32p), ctypes.byref(n_new)), what, self.L)
        dst.n = int(n_new.value)
        return old[:dst.n]

    def induced(self, keep, device=None, **options):
        """A new Engine (this one's GPU; `options` as for Engine()) holding the subgraph induced by the vertices with keep[i] != 0,
        built on the device and renumbered in ascending old id.  Returns (engine, old_of_new)."""
        keep = self._keep_mask(keep, "induced")
        sub = Engine(self.device if device is None else device, **options)
        try:
            if sub.debug != self.debug:   # two libraries, two handle layouts: both handles must come from the same one
                raise ValueError("induced: the options select the other build of the library (product / debug knobs) than this Engine's")
            old = self._induce_into(sub, keep, "lzx_set_graph_induced")
        except Exception:
            sub.close()
            raise
        return sub, old

    def restrict(self, keep):
        """Replace this Engine's graph by its subgraph on the vertices with keep[i] != 0 (lzx_set_graph_induced with dst == src).
        Returns old_of_new.  If the call fails the Engine keeps its graph."""
        return self._induce_into(self, self._keep_mask(keep, "restrict"), "lzx_set_graph_induced(in place)")

    def largest_component(self, **options):
        """components() followed by induced(labels == largest_label): (engine on the largest component, old_of_new)."""
        labels, info = self.components()
        return self.induced(labels == info["largest_label"], **options)

    @staticmethod
    def component_indicators(labels, which):
        """W[nw][n]: the unit indicator vectors of the components whose labels are listed in `which` (host numpy) -- the null
        space of L on those components, ready to be the deflation vectors of solve_shifted and eigsh."""
        labels = np.asarray(labels)
        which = np.atleast_1d(np.asarray(which))
        W = np.zeros((len(which), len(labels)))
        for i, r in enumerate(which):
            members = labels == r
            if not members.any() or labels[int(r)] != r:
                raise ValueError(f"component_indicators: {int(r)} is not the label of a component")
            W[i, members] = 1.0 / np.sqrt(np.count_nonzero(members))
        return W

    # ---- path-based centralities (include/lzx.h: lzx_bfs_multi, lzx_betweenness_f64, lzx_brandes_f64; DESIGN.md sections 17, 24) ----
    def _sources(self, sources, what):
        """(uint32 array or None for every vertex, ns)"""
        if sources is None:
            return None, self.n
        src = np.atleast_1d(np.asarray(sources))
        if src.ndim != 1 or src.size == 0:
            raise ValueError(f"{what}: sources must be a non-empty 1-D sequence of vertex ids")
        if src.min() < 0 or src.max() >= self.n:
            raise ValueError(f"{what}: vertex ids must lie in [0, {self.n})")
        return np.ascontiguousarray(src, dtype=np.uint32), len(src)

    def bfs(self, sources, paths: bool = False, dist: bool = True):
        """Breadth-first search from every source on the device, 16 sources per sweep over the edges (lzx_bfs_multi).  Returns
        (dist, info) or, with paths=True, (dist, paths, info): dist (ns, n) int32 with -1 where unreachable (None with
        dist=False: then no n-vector leaves the device), paths (ns, n) the number of shortest paths, info = the lzx_bfs_info
        fields plus "reached", "sum_dist", "harmonic" and "ecc", one per source."""
        src, ns = self._sources(np.arange(self.n, dtype=np.uint32) if sources is None else sources, "bfs")
        D = np.empty((ns, self.n), dtype=np.int32) if dist else None
        P = np.empty((ns, self.n)) if paths else None
        reached, sum_dist = np.zeros(ns, dtype=np.uint64), np.zeros(ns, dtype=np.uint64)
        harmonic, ecc = np.zeros(ns), np.zeros(ns, dtype=np.uint32)
        info = LzxBfsInfo()
        _check(self.L.lzx_bfs_multi(self.h, ns, _p(src, _u32p), _p(D, _i32p) if dist else None, _p(P, _f64p) if paths else None,
                                    _p(reached, _u64p), _p(sum_dist, _u64p), _p(harmonic, _f64p), _p(ecc, _u32p), ctypes.byref(info)),
               "lzx_bfs_multi", self.L)
        d = info.as_dict()
        d.update(reached=reached, sum_dist=sum_dist, harmonic=harmonic, ecc=ecc)
        return (D, P, d) if paths else (D, d)

    def closeness(self, sources=None):
        """networkx.closeness_centrality(G, u) with wf_improved=True for every u of `sources` (None: every vertex), from the
        per-source counts alone: ((r - 1) / sum_dist) * ((r - 1) / (n - 1)) with r the vertices u reaches; 0 for a vertex that
        reaches only itself."""
        info = self.bfs(np.arange(self.n, dtype=np.uint32) if sources is None else sources, dist=False)[1]
        r1 = info["reached"].astype(np.float64) - 1.0
        tot = info["sum_dist"].astype(np.float64)
        out = np.zeros(len(r1))
        ok = (tot > 0) & (self.n > 1)
        out[ok] = (r1[ok] / tot[ok]) * (r1[ok] / (self.n - 1.0))
        return out

    def harmonic(self, sources=None):
        """networkx.harmonic_centrality of every vertex of `sources` (None: every vertex): the sum of 1 / d(u, v) over the v != u
        that u reaches."""
        return self.bfs(np.arange(self.n, dtype=np.uint32) if sources is None else sources, dist=False)[1]["harmonic"]

    def betweenness_raw(self, sources=None):
        """(bc, info) of lzx_betweenness_f64: the sum over the sources (None: every vertex) of Brandes' dependencies, unscaled."""
        src, ns = self._sources(sources, "betweenness")
        bc = np.empty(self.n)
        info = LzxBfsInfo()
        _check(self.L.lzx_betweenness_f64(self.h, ns, None if src is None else _p(src, _u32p), _p(bc, _f64p), ctypes.byref(info)),
               "lzx_betweenness_f64", self.L)
        return bc, info.as_dict()

    def brandes_raw(self, sources=None, want_bc: bool = True, want_edges: bool = True, endpoints: bool = False):
        """(bc, ebc, info) of lzx_brandes_f64, unscaled: bc (n,) the sum over the sources (None: every vertex) of Brandes'
        dependencies -- with endpoints=True plus the endpoints' count --, ebc one value per stored entry of get_graph_csr()'s
        col_idx (both copies of an edge carry its number; a diagonal entry carries 0).  Each is None when not wanted, and then
        it does not leave the device.  info = the lzx_brandes_info fields."""
        src, ns = self._sources(sources, "brandes")
        bc = np.empty(max(self.n, 1)) if want_bc else None
        nnz = int(self.info()["nnz"]) if want_edges else 0
        ebc = np.zeros(max(nnz, 1)) if want_edges else None
        info = LzxBrandesInfo()
        _check(self.L.lzx_brandes_f64(self.h, ns, None if src is None else _p(src, _u32p), LZX_BRANDES_ENDPOINTS if endpoints else 0,
                                      None if bc is None else _p(bc, _f64p), None if ebc is None else _p(ebc, _f64p), ctypes.byref(info)),
               "lzx_brandes_f64", self.L)
        return None if bc is None else bc[:self.n], None if ebc is None else ebc[:nnz], info.as_dict()

    def _sampled_sources(self, what, k, sources, seed):
        """the sources of a sampled centrality: `sources`, or k distinct ones drawn with numpy.random.default_rng(seed)"""
        n = self.n
        if sources is not None and k is not None:
            raise ValueError(f"{what}: give k or sources, not both")
        if k is not None:
            if not 1 <= k <= n:
                raise ValueError(f"{what}: k must lie in [1, {n}]")
            sources = np.random.default_rng(seed).choice(n, size=k, replace=False)
        return sources

    def edge_betweenness(self, k=None, sources=None, normalized: bool = True, seed: int = 0):
        """Edge betweenness centrality as networkx.edge_betweenness_centrality defines it on an undirected graph: a scipy CSR
        matrix (float64) over the handle's pattern, symmetric; a diagonal entry holds 0.  k and sources as in betweenness.
        Scaling (networkx 3.4's _rescale_e): 1 / (n (n - 1)) when normalised and n > 1, 0.5 when not, both times n / k when
        sampling."""
        n = self.n
        sources = self._sampled_sources("edge_betweenness", k, sources, seed)
        ebc = self.brandes_raw(sources, want_bc=False)[1]
        ks = None if sources is None else len(np.atleast_1d(sources))
        if normalized:
            scale = 1.0 / (n * (n - 1)) if n > 1 else None
        else:
            scale = 0.5
        if scale is not None:
            if ks is not None:
                scale = scale * n / ks
            ebc = ebc * scale
        return self._edge_matrix(ebc)

    def betweenness(self, k=None, sources=None, normalized: bool = True, seed: int = 0, endpoints: bool = False):
        """Betweenness centrality as networkx.betweenness_centrality defines it on an undirected graph, without endpoints or
        (endpoints=True, through lzx_brandes_f64) with them.
        sources=None, k=None: exact; k: k distinct sources sampled with numpy.random.default_rng(seed); explicit `sources` are
        scaled as a sample of len(sources).  Scaling (networkx 3.4's _rescale): 1 / ((n - 1)(n - 2)) when normalised and n > 2
        -- with endpoints 1 / (n (n - 1)) when n >= 2 --, 0.5 when not, both times n / k when sampling."""
        n = self.n
        sources = self._sampled_sources("betweenness", k, sources, seed)
        bc = self.brandes_raw(sources, want_edges=False, endpoints=True)[0] if endpoints else self.betweenness_raw(sources)[0]
        ks = None if sources is None else len(np.atleast_1d(sources))
        if normalized:
            if endpoints:
                scale = 1.0 / (n * (n - 1)) if n >= 2 else None
            else:
                scale = 1.0 / ((n - 1) * (n - 2)) if n > 2 else None
        else:
            scale = 0.5
        if scale is not None:
            if ks is not None:
                scale = scale * n / ks
            bc = bc * scale
        return bc

    # ---- triangles and clustering (include/lzx.h: lzx_triangles) ----
    def triangles_raw(self, want_triangles: bool = True, want_clustering: bool = True):
        """(tri, clustering, info) of lzx_triangles: tri[v] = the triangles through v (uint64), clustering[v] = networkx's
        clustering coefficient (float64), both in the caller's order and None when not wanted (then that vector does not leave the
        device); info = the lzx_triangles_info fields (triangles, wedges, max_triangles, oriented_entries, oriented_max_degree,
        avg_clustering, loop_ms, orient_ms, count_ms)."""
        tri = np.empty(self.n, dtype=np.uint64) if want_triangles else None
        clus = np.empty(self.n) if want_clustering else None
        info = LzxTrianglesInfo()
        _check(self.L.lzx_triangles(self.h, _p(tri, _u64p) if want_triangles else None, _p(clus, _f64p) if want_clustering else None,
                                    ctypes.byref(info)), "lzx_triangles", self.L)
        return tri, clus, info.as_dict()

    def _nodes(self, nodes, what):
        idx = np.atleast_1d(np.asarray(nodes))
        if idx.ndim != 1 or not (np.issubdtype(idx.dtype, np.integer) or idx.size == 0) or (idx.size and (idx.min() < 0 or idx.max() >= self.n)):
            raise ValueError(f"{what}: nodes must be a 1-D sequence of integer vertex ids in [0, {self.n})")
        return idx.astype(np.int64)

    def triangles(self, nodes=None):
        """networkx.triangles: the number of triangles through every vertex (uint64 array, caller's order), or through `nodes`."""
        tri = self.triangles_raw(want_clustering=False)[0]
        return tri if nodes is None else tri[self._nodes(nodes, "triangles")]

    def clustering(self, nodes=None):
        """networkx.clustering of an unweighted, undirected graph: 2 t_v / (d_v (d_v - 1)) with d_v the neighbours other than v
        itself, 0 where d_v < 2 (float64 array, caller's order), or of `nodes`."""
        clus = self.triangles_raw(want_triangles=False)[1]
        return clus if nodes is None else clus[self._nodes(nodes, "clustering")]

    def transitivity(self):
        """networkx.transitivity: 3 T / wedges, formed from networkx's own operands (6 T and 2 wedges, Python integers); 0 for a
        graph without a triangle.  No n-vector leaves the device."""
        info = self.triangles_raw(want_triangles=False, want_clustering=False)[2]
        T, wedges = int(info["triangles"]), int(info["wedges"])
        return 0.0 if T == 0 else (6 * T) / (2 * wedges)

    def average_clustering(self, count_zeros: bool = True):
        """networkx.average_clustering.  count_zeros=True: the mean over every vertex, formed on the device (no n-vector leaves
        it); False: the mean of the non-zero coefficients, from the downloaded vector (0.0 when there is none)."""
        if count_zeros:
            return self.triangles_raw(want_triangles=False, want_clustering=False)[2]["avg_clustering"]
        clus = self.triangles_raw(want_triangles=False)[1]
        nz = clus[clus > 0.0]
        return float(nz.sum() / len(nz)) if len(nz) else 0.0

    # ---- core numbers and onion layers (include/lzx.h: lzx_core_numbers) ----
    def core_number_raw(self, want_core: bool = True, want_layers: bool = True):
        """(core, layer, info) of lzx_core_numbers: core[v] = networkx.core_number, layer[v] = networkx.onion_layers (uint32, the
        caller's order; None when not wanted, and then that vector does not leave the device); info = the lzx_core_info fields
        (main_core_size, core0, degeneracy, levels, rounds, loop_ms, peel_ms).  Self loops are ignored."""
        core = np.empty(self.n, dtype=np.uint32) if want_core else None
        layer = np.empty(self.n, dtype=np.uint32) if want_layers else None
        info = LzxCoreInfo()
        _check(self.L.lzx_core_numbers(self.h, _p(core, _u32p) if want_core else None, _p(layer, _u32p) if want_layers else None,
                                       ctypes.byref(info)), "lzx_core_numbers", self.L)
        return core, layer, info.as_dict()

    def core_number(self, nodes=None):
        """networkx.core_number: the largest k such that the vertex lies in the k-core (uint32 array, caller's order), or of `nodes`."""
        core = self.core_number_raw(want_layers=False)[0]
        return core if nodes is None else core[self._nodes(nodes, "core_number")]

    def onion_layers(self, nodes=None):
        """networkx.onion_layers: the peeling round, from 1, in which the vertex is removed (uint32 array, caller's order), or of
        `nodes`."""
        layer = self.core_number_raw(want_core=False)[1]
        return layer if nodes is None else layer[self._nodes(nodes, "onion_layers")]

    def degeneracy(self):
        """The largest core number.  No n-vector leaves the device."""
        return int(self.core_number_raw(want_core=False, want_layers=False)[2]["degeneracy"])

    def k_core(self, k=None, **options):
        """networkx.k_core: induced(core >= k) -- (engine on the k-core, old_of_new), built on the device; k=None selects the main
        core (k = the degeneracy).  `options` as for induced()."""
        core, _, info = self.core_number_raw(want_layers=False)
        top = int(info["degeneracy"])
        k = top if k is None else int(k)
        if k > top:
            raise ValueError(f"k_core: k = {k} is above the degeneracy {top} of this graph: the {k}-core is empty")
        return self.induced(core >= max(k, 0), **options)

    def k_shell(self, k=None, **options):
        """networkx.k_shell: induced(core == k) -- (engine on the vertices of core number exactly k, old_of_new); k=None selects the
        main core's shell (k = the degeneracy).  An empty shell is a ValueError."""
        core, _, info = self.core_number_raw(want_layers=False)
        top = int(info["degeneracy"])
        k = top if k is None else int(k)
        keep = core == k if k >= 0 else np.zeros(self.n, dtype=bool)
        if not keep.any():
            raise ValueError(f"k_shell: no vertex of this graph has core number {k} (the degeneracy is {top})")
        return self.induced(keep, **options)

    # ---- edge support and truss numbers (include/lzx.h: lzx_truss) ----
    def truss_raw(self, want_support: bool = True, want_truss: bool = True, want_layer: bool = True, want_vertex: bool = True):
        """(support, truss, layer, vertex_truss, info) of lzx_truss.  support, truss and layer are uint32 arrays with one value per
        stored entry of get_graph_csr()'s col_idx (both copies of an edge carry its number; a diagonal entry carries 0):
        the triangles through the edge, the largest k such that the edge lies in networkx.k_truss(G, k), and the peeling round,
        from 1, in which it is removed.  vertex_truss[v] (uint32, the caller's order) is the largest truss number among v's
        edges.  Each is None when not wanted, and then it does not leave the device.  info = the lzx_truss_info fields (edges,
        triangles, main_truss_edges, max_support, max_truss, levels, rounds, loop_ms, support_ms, peel_ms).  Self loops are
        ignored."""
        nnz = int(self.info()["nnz"]) if (want_support or want_truss or want_layer) else 0
        outs = [np.zeros(max(nnz, 1), dtype=np.uint32) if want else None for want in (want_support, want_truss, want_layer)]
        vertex = np.zeros(max(self.n, 1), dtype=np.uint32) if want_vertex else None
        info = LzxTrussInfo()
        _check(self.L.lzx_truss(self.h, *[None if o is None else _p(o, _u32p) for o in outs], None if vertex is None else _p(vertex, _u32p),
                                ctypes.byref(info)), "lzx_truss", self.L)
        support, truss, layer = [None if o is None else o[:nnz] for o in outs]
        return support, truss, layer, None if vertex is None else vertex[:self.n], info.as_dict()

    def _edge_matrix(self, values):
        import scipy.sparse as sp
        rp, ci = self.get_graph_csr()
        return sp.csr_matrix((values, ci.astype(np.int64), rp.astype(np.int64)), shape=(self.n, self.n))

    def edge_support(self):
        """The triangles through every edge: a scipy CSR matrix (uint32) over the handle's pattern, symmetric; a diagonal entry
        holds 0."""
        return self._edge_matrix(self.truss_raw(want_truss=False, want_layer=False, want_vertex=False)[0])

    def truss_number(self):
        """The truss number of every edge -- the largest k such that the edge lies in networkx.k_truss(G, k), at least 2: a scipy
        CSR matrix (uint32) over the handle's pattern, symmetric; a diagonal entry holds 0."""
        return self._edge_matrix(self.truss_raw(want_support=False, want_layer=False, want_vertex=False)[1])

    def max_truss(self):
        """The largest truss number (0 for a graph without an edge).  No vector leaves the device."""
        return int(self.truss_raw(False, False, False, False)[4]["max_truss"])

    def k_truss(self, k=None, **options):
        """networkx.k_truss: (engine on the k-truss, old_of_new) -- the edges of truss number >= k and the vertices that keep at
        least one of them, renumbered in ascending old id; k=None selects the main truss (k = max_truss()).  A truss is not a
        vertex-induced subgraph (an edge between two of its vertices may be missing from it), so unlike k_core this path is not
        built on the device: the truss numbers come back per entry, the CSR is filtered on the host and handed to a new Engine
        (this one's GPU; `options` as for Engine()) with set_graph_csr.  Self loops are dropped."""
        _, truss, _, _, info = self.truss_raw(want_support=False, want_layer=False, want_vertex=False)
        top = int(info["max_truss"])
        k = top if k is None else int(k)
        if top == 0:
            raise ValueError("k_truss: this graph has no edge")
        if k > top:
            raise ValueError(f"k_truss: k = {k} is above the largest truss number {top} of this graph: the {k}-truss is empty")
        rp, ci = self.get_graph_csr()
        keep = truss >= max(k, 2)
        rows = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(rp.astype(np.int64)))[keep]
        counts = np.bincount(rows, minlength=self.n)
        old = np.flatnonzero(counts).astype(np.uint32)
        new_of_old = np.zeros(self.n, dtype=np.uint32)
        new_of_old[old] = np.arange(len(old), dtype=np.uint32)
        sub_rp = np.concatenate([[0], np.cumsum(counts[old])]).astype(np.uint64)
        sub = Engine(self.device, **options)
        try:
            sub.set_graph_csr(sub_rp, new_of_old[ci[keep]])
        except Exception:
            sub.close()
            raise
        return sub, old

    # ---- similarity of two vertices (include/lzx.h: lzx_similarity) ----
    def _pairs(self, pairs, what):
        arr = np.asarray(pairs)
        if arr.size == 0:
            return np.zeros((0, 2), dtype=np.uint32)
        if arr.ndim != 2 or arr.shape[1] != 2 or not np.issubdtype(arr.dtype, np.integer) or arr.min() < 0 or arr.max() >= self.n:
            raise ValueError(f"{what}: pairs must be an (np, 2) array or a list of pairs of integer vertex ids in [0, {self.n})")
        if (arr[:, 0] == arr[:, 1]).any():
            raise ValueError(f"{what}: a vertex is not compared with itself")
        return arr.astype(np.uint32)

    def similarity_raw(self, pairs=None, measures=("jaccard", "overlap", "sorensen", "adamic_adar", "resource_allocation"),
                       want_common: bool = True, want_degrees: bool = True):
        """(common, deg_u, deg_v, values, info) of lzx_similarity for the pairs (u, v) of an (np, 2) array or a list of pairs, or,
        with pairs=None, for every stored entry of get_graph_csr()'s col_idx (entry e of row r is the pair (r, col_idx[e]); both
        copies of an edge carry the same bits, a diagonal entry carries 0).  common[p] = the common neighbours of the pair,
        deg_u[p] and deg_v[p] the degrees of its ends, self loops not counted (uint32; None when not wanted, and then they do not
        leave the device); values = {measure: float64 array} for the names in `measures`, out of "jaccard", "overlap",
        "sorensen", "adamic_adar", "resource_allocation"; info = the lzx_similarity_info fields (pairs, walked, short_pairs,
        long_pairs, sliced_pairs, max_common, lanes, loop_ms, prep_ms, count_ms)."""
        names = [measures] if isinstance(measures, str) else list(measures)
        unknown = [m for m in names if m not in SIM_MEASURES]
        if unknown:
            raise ValueError(f"similarity_raw: unknown measure {unknown[0]!r} (known: {', '.join(SIM_MEASURES)})")
        bits = 0
        for m in names:
            bits |= SIM_MEASURES[m]
        rows = [m for m in SIM_MEASURES if SIM_MEASURES[m] & bits]          # ascending bit order
        if pairs is None:
            count = int(self.info()["nnz"])
            pu = pv = None
        else:
            pr = self._pairs(pairs, "similarity_raw")
            count = len(pr)
            pu = np.ascontiguousarray(pr[:, 0]) if count else np.zeros(1, dtype=np.uint32)
            pv = np.ascontiguousarray(pr[:, 1]) if count else np.zeros(1, dtype=np.uint32)
        room = max(count, 1)
        common = np.zeros(room, dtype=np.uint32) if want_common else None
        deg_u = np.zeros(room, dtype=np.uint32) if want_degrees else None
        deg_v = np.zeros(room, dtype=np.uint32) if want_degrees else None
        vals = np.zeros((max(len(rows), 1), room))
        info = LzxSimilarityInfo()
        opt = lambda a: None if a is None else _p(a, _u32p)   # noqa: E731
        _check(self.L.lzx_similarity(self.h, count, opt(pu), opt(pv), bits, opt(common), opt(deg_u), opt(deg_v), _p(vals, _f64p) if rows else None,
                                     ctypes.byref(info)), "lzx_similarity", self.L)
        cut = lambda a: None if a is None else a[:count]      # noqa: E731
        flat = vals.reshape(-1)
        values = {m: flat[k * count:(k + 1) * count].copy() for k, m in enumerate(rows)}
        return cut(common), cut(deg_u), cut(deg_v), values, info.as_dict()

    def _similarity_value(self, pairs, measure):
        return self.similarity_raw(pairs, measures=(measure,), want_common=False, want_degrees=False)[3][measure]

    def common_neighbors_count(self, pairs):
        """len(networkx.common_neighbors(G, u, v)) for every pair (uint32 array), self loops ignored."""
        return self.similarity_raw(pairs, measures=(), want_degrees=False)[0]

    def jaccard_coefficient(self, pairs):
        """networkx.jaccard_coefficient: |N(u) n N(v)| / |N(u) u N(v)| for every pair, 0 where the union is empty (float64)."""
        return self._similarity_value(pairs, "jaccard")

    def overlap_coefficient(self, pairs):
        """|N(u) n N(v)| / min(d_u, d_v) for every pair, 0 where the minimum is 0 (float64)."""
        return self._similarity_value(pairs, "overlap")

    def sorensen_coefficient(self, pairs):
        """2 |N(u) n N(v)| / (d_u + d_v) for every pair, 0 where the sum is 0 (float64)."""
        return self._similarity_value(pairs, "sorensen")

    def adamic_adar_index(self, pairs):
        """networkx.adamic_adar_index: the sum over the common neighbours w of 1 / log d_w, for every pair (float64)."""
        return self._similarity_value(pairs, "adamic_adar")

    def resource_allocation_index(self, pairs):
        """networkx.resource_allocation_index: the sum over the common neighbours w of 1 / d_w, for every pair (float64)."""
        return self._similarity_value(pairs, "resource_allocation")

    def preferential_attachment(self, pairs):
        """networkx.preferential_attachment: d_u d_v for every pair, formed here as int64 from the degrees the device returns."""
        _, du, dv, _, _ = self.similarity_raw(pairs, measures=(), want_common=False)
        return du.astype(np.int64) * dv.astype(np.int64)

    def cosine_similarity(self, pairs):
        """|N(u) n N(v)| / sqrt(d_u d_v) for every pair, 0 where a degree is 0 (float64).  Formed here in numpy from the counts
        and degrees the device returns: the rounding of the device's square root is not pinned, numpy's is."""
        c, du, dv, _, _ = self.similarity_raw(pairs, measures=())
        prod = du.astype(np.float64) * dv.astype(np.float64)
        out = np.zeros(len(c))
        nz = prod > 0
        out[nz] = c[nz] / np.sqrt(prod[nz])
        return out

    def edge_similarity(self, measure="jaccard"):
        """One similarity per edge: a scipy CSR matrix over the handle's pattern, symmetric, a diagonal entry holding 0.  `measure`
        is one of similarity_raw's names (float64), or "common_neighbors" (uint32: the matrix edge_support() returns)."""
        if measure == "common_neighbors":
            return self._edge_matrix(self.similarity_raw(None, measures=(), want_degrees=False)[0])
        if measure not in SIM_MEASURES:
            raise ValueError(f"edge_similarity: unknown measure {measure!r} (known: common_neighbors, {', '.join(SIM_MEASURES)})")
        return self._edge_matrix(self._similarity_value(None, measure))

    # ---- colouring, label-propagation communities, modularity (include/lzx.h: lzx_color, lzx_label_propagation, lzx_modularity;
    # DESIGN.md section 21) ----
    def color_raw(self, seed: int = 0, ties_by_id: bool = False, want_colors: bool = True):
        """(color, info) of lzx_color: color[v] = the colour of sequential greedy colouring in the order (degree descending, hash of
        the id under `seed` ascending, id ascending) -- with ties_by_id the hash is left out and the colouring is
        networkx.coloring.greedy_color(G)'s (uint32, the caller's order; None with want_colors=False, and then no n-vector leaves
        the device); info = the lzx_color_info fields (colors, rounds, largest_class, loop_ms, color_ms).  Self loops are ignored.
        Ties by id can take n rounds; the hashed order is the default for that reason."""
        color = np.empty(self.n, dtype=np.uint32) if want_colors else None
        info = LzxColorInfo()
        _check(self.L.lzx_color(self.h, int(seed), LZX_COLOR_TIES_BY_ID if ties_by_id else 0, _p(color, _u32p) if want_colors else None,
                                ctypes.byref(info)), "lzx_color", self.L)
        return color, info.as_dict()

    def greedy_color(self, seed: int = 0, ties_by_id: bool = False):
        """networkx.coloring.greedy_color as a uint32 array in the caller's order (see color_raw)."""
        return self.color_raw(seed, ties_by_id)[0]

    def label_propagation_raw(self, seed: int = 0, ties_by_id: bool = False, max_sweeps: int = 1000, want_labels: bool = True):
        """(labels, info) of lzx_label_propagation: semi-synchronous label propagation over the colour classes of
        color_raw(seed, ties_by_id), Prec-Max ties; labels[v] = the smallest vertex id of v's community (uint32, the caller's order;
        None with want_labels=False); info = the lzx_communities_info fields (n_communities, largest_size, largest_label, sweeps,
        updates, colors, color_rounds, inner_entries, entries, sum_degree_sq, modularity, loop_ms, color_ms, sweep_ms).  With
        ties_by_id the communities are networkx.community.label_propagation_communities(G)'s.  LzxError (-6) if max_sweeps
        sweeps did not reach a fixed point."""
        labels = np.empty(self.n, dtype=np.uint32) if want_labels else None
        info = LzxCommunitiesInfo()
        _check(self.L.lzx_label_propagation(self.h, int(seed), LZX_COLOR_TIES_BY_ID if ties_by_id else 0, int(max_sweeps),
                                            _p(labels, _u32p) if want_labels else None, ctypes.byref(info)), "lzx_label_propagation", self.L)
        return labels, info.as_dict()

    def label_propagation_communities(self, seed: int = 0, ties_by_id: bool = False, max_sweeps: int = 1000):
        """networkx.community.label_propagation_communities: a list of index arrays (int64, ascending), the largest community first
        and communities of one size by their label (their smallest vertex)."""
        labels = self.label_propagation_raw(seed, ties_by_id, max_sweeps)[0]
        order = np.argsort(labels, kind="stable")
        parts = np.split(order, np.flatnonzero(np.diff(labels[order])) + 1) if self.n else []
        return sorted(parts, key=lambda part: (-len(part), int(part[0])))

    def _labels_of(self, labels_or_communities, what):
        if isinstance(labels_or_communities, np.ndarray) and labels_or_communities.ndim == 1 and len(labels_or_communities) == self.n:
            labels = labels_or_communities
        else:   # a list of vertex sets: every vertex in exactly one
            labels = np.full(self.n, -1, dtype=np.int64)
            for part in labels_or_communities:
                part = np.asarray(sorted(part) if isinstance(part, (set, frozenset)) else part, dtype=np.int64)
                if len(part) == 0:
                    continue
                if part.min() < 0 or part.max() >= self.n or (labels[part] != -1).any():
                    raise ValueError(f"{what}: the communities must be disjoint sets of vertices 0 .. {self.n - 1}")
                labels[part] = part.min()
            if (labels < 0).any():
                raise ValueError(f"{what}: vertex {int(np.flatnonzero(labels < 0)[0])} is in no community")
        labels = np.asarray(labels)
        if labels.shape != (self.n,):
            raise ValueError(f"{what}: labels must have shape ({self.n},), one per vertex, got {labels.shape}")
        if len(labels) and (labels.min() < 0 or labels.max() > 0xffffffff):
            raise ValueError(f"{what}: labels must be vertex ids 0 .. {self.n - 1}")
        return np.ascontiguousarray(labels, dtype=np.uint32)

    def modularity_raw(self, labels_or_communities):
        """(q, info) of lzx_modularity: Newman's modularity at resolution 1 of a labelling (an array of n labels < n) or of a list
        of disjoint vertex sets that cover the graph, as label_propagation_communities returns it; info = the lzx_modularity_info
        fields (communities, inner_entries, entries, sum_degree_sq, loop_ms)."""
        labels = self._labels_of(labels_or_communities, "modularity")
        q = ctypes.c_double()
        info = LzxModularityInfo()
        _check(self.L.lzx_modularity(self.h, _p(labels, _u32p), ctypes.byref(q), ctypes.byref(info)), "lzx_modularity", self.L)
        return q.value, info.as_dict()

    def modularity(self, labels_or_communities):
        """networkx.community.modularity(G, communities) as a float (see modularity_raw)."""
        return self.modularity_raw(labels_or_communities)[0]

    def community(self, labels, which=None, **options):
        """induced(labels == which): (engine on one community, old_of_new), built on the device; which=None selects the largest
        community, ties to the smallest label.  `options` as for induced()."""
        labels = np.asarray(labels)
        if labels.shape != (self.n,):
            raise ValueError(f"community: labels must have shape ({self.n},), one per vertex, got {labels.shape}")
        if which is None:
            values, counts = np.unique(labels, return_counts=True)
            which = values[np.argmax(counts)]
        keep = labels == which
        if not keep.any():
            raise ValueError(f"community: no vertex has the label {which}")
        return self.induced(keep, **options)

    # ---- Louvain communities (include/lzx.h: lzx_louvain) ----
    def louvain_raw(self, seed: int = 0, ties_by_id: bool = False, max_sweeps: int = 100, max_levels: int = 32, want_labels: bool = True,
                    want_level_labels: bool = True):
        """(labels, level_labels, levels, info) of lzx_louvain: local moves over the colour classes of every level graph, then
        aggregation, until a level changes nothing.  labels[v] = the smallest vertex id of v's final community (uint32, the caller's
        order; None with want_labels=False); level_labels = the same for the partition after every counted level, (info["levels"], n)
        (None with want_level_labels=False); levels = one dict of the lzx_louvain_level fields per counted level; info = the
        lzx_louvain_info fields.  Everything but the timings is a function of the graph, the seed and the tie rule."""
        labels = np.empty(self.n, dtype=np.uint32) if want_labels else None
        per_level = np.empty((int(max_levels), self.n), dtype=np.uint32) if want_level_labels and 1 <= int(max_levels) <= 64 else None
        records = (LzxLouvainLevel * max(min(int(max_levels), 64), 1))()
        info = LzxLouvainInfo()
        _check(self.L.lzx_louvain(self.h, int(seed), LZX_COLOR_TIES_BY_ID if ties_by_id else 0, int(max_sweeps), int(max_levels),
                                  _p(labels, _u32p) if want_labels else None, _p(per_level, _u32p) if per_level is not None else None, records,
                                  ctypes.byref(info)), "lzx_louvain", self.L)
        return (labels, None if per_level is None else per_level[:info.levels], [records[l].as_dict() for l in range(info.levels)],
                info.as_dict())

    @staticmethod
    def _parts_of(labels):
        order = np.argsort(labels, kind="stable")
        parts = np.split(order, np.flatnonzero(np.diff(labels[order])) + 1) if len(labels) else []
        return sorted(parts, key=lambda part: (-len(part), int(part[0])))

    def louvain_communities(self, seed: int = 0, ties_by_id: bool = False, max_sweeps: int = 100, max_levels: int = 32):
        """networkx.community.louvain_communities at resolution 1: a list of index arrays (int64, ascending), ordered as
        label_propagation_communities orders them."""
        return self._parts_of(self.louvain_raw(seed, ties_by_id, max_sweeps, max_levels, want_level_labels=False)[0])

    def louvain_partitions(self, seed: int = 0, ties_by_id: bool = False, max_sweeps: int = 100, max_levels: int = 32):
        """networkx.community.louvain_partitions: one such list per level, the finest first; none on a graph no level changes."""
        per_level = self.louvain_raw(seed, ties_by_id, max_sweeps, max_levels, want_labels=False)[1]
        return [self._parts_of(row) for row in per_level]

    # ---- sweep cuts, spectral bisection, local clusters (include/lzx.h: lzx_sweep_cut) ----
    def sweep_cut_raw(self, scores, ascending: bool = False, per_degree: bool = False, objective: str = "conductance", k_min: int = 0,
                      k_max: int = 0, want_order: bool = True, want_profile: bool = False):
        """(order, cut, vol, results, info) of lzx_sweep_cut for the score vectors `scores`, (n,) or (ns, n) with ns <= 16: the
        vertices by descending score (ascending=True: ascending; per_degree=True: by score / degree, vertices without an edge
        last), ties by ascending id; cut[c, k-1] and vol[c, k-1] of the first k vertices (uint64; None without want_profile, as
        order is without want_order, and then they do not leave the device); results[c] = the lzx_sweep_result fields (k, cut,
        vol, den, value) of the prefix with k_min <= k <= k_max (0: 1 and n - 1) of least conductance cut / min(vol, M - vol), or
        least edge expansion cut / min(k, n - k) with objective="expansion" (k = 0 and value = inf when no prefix has a
        denominator); info = the lzx_sweep_info fields.  The arrays always have the shape (ns, n)."""
        if objective not in ("conductance", "expansion"):
            raise ValueError(f"sweep_cut: objective must be 'conductance' or 'expansion', not {objective!r}")
        S = np.ascontiguousarray(np.atleast_2d(np.asarray(scores, dtype=np.float64)))
        if S.ndim != 2 or S.shape[1] != self.n:
            raise ValueError(f"sweep_cut: scores must have shape ({self.n},) or (ns, {self.n}), got {np.shape(scores)}")
        ns = S.shape[0]
        flags = (LZX_SWEEP_ASCENDING if ascending else 0) | (LZX_SWEEP_PER_DEGREE if per_degree else 0) | \
                (LZX_SWEEP_EXPANSION if objective == "expansion" else 0)
        order = np.empty((ns, self.n), dtype=np.uint32) if want_order else None
        cut = np.empty((ns, self.n), dtype=np.uint64) if want_profile else None
        vol = np.empty((ns, self.n), dtype=np.uint64) if want_profile else None
        best = (LzxSweepResult * max(ns, 1))()
        info = LzxSweepInfo()
        _check(self.L.lzx_sweep_cut(self.h, ns, _p(S, _f64p), flags, int(k_min), int(k_max), _p(order, _u32p) if want_order else None,
                                    _p(cut, _u64p) if want_profile else None, _p(vol, _u64p) if want_profile else None, best, ctypes.byref(info)),
               "lzx_sweep_cut", self.L)
        return order, cut, vol, [best[c].as_dict() for c in range(ns)], info.as_dict()

    def sweep_cut(self, score, **kw):
        """The best prefix of the sweep over `score` (see sweep_cut_raw, whose keywords it takes): (members = the vertices of the
        prefix as sorted ids (int64), value, result).  A 2-D score, (ns, n), gives a list of these, one per row."""
        order, _, _, results, _ = self.sweep_cut_raw(score, want_order=True, want_profile=False, **kw)
        out = [(np.sort(order[c, :r["k"]].astype(np.int64)), r["value"], r) for c, r in enumerate(results)]
        return out if np.ndim(score) == 2 else out[0]

    def _indicator(self, S, what):
        S = np.asarray(S)
        ind = np.zeros(self.n)
        if S.dtype == np.bool_:
            if S.shape != (self.n,):
                raise ValueError(f"{what}: a mask must have shape ({self.n},), got {S.shape}")
            ind[S] = 1.0
        elif S.size:
            idx = S.astype(np.int64).ravel()
            if idx.min() < 0 or idx.max() >= self.n:
                raise ValueError(f"{what}: the set must hold vertices 0 .. {self.n - 1}")
            ind[idx] = 1.0
        return ind, int(ind.sum())

    def _set_sweep(self, S, what, objective="conductance"):
        """the lzx_sweep_result of the set S against its complement: one sweep of S's indicator with k_min = k_max = |S|"""
        ind, size = self._indicator(S, what)
        if size == 0:   # (the prefix of no vertex: nothing to sweep)
            return dict(k=0, cut=0, vol=0, den=0, value=float("inf"))
        _, cut, vol, results, _ = self.sweep_cut_raw(ind, objective=objective, k_min=size, k_max=size, want_order=False, want_profile=True)
        r = results[0]
        if r["k"] == 0:   # a denominator of 0: the integers come from the profile
            r = dict(k=size, cut=int(cut[0, size - 1]), vol=int(vol[0, size - 1]), den=0, value=float("inf"))
        return r

    def cut_size(self, S):
        """networkx.cut_size(G, S): the edges between S (an index list or a boolean mask) and its complement."""
        return int(self._set_sweep(S, "cut_size")["cut"])

    def volume(self, S):
        """networkx.volume(G, S): the sum of the degrees of S, self loops not counted."""
        return int(self._set_sweep(S, "volume")["vol"])

    def conductance(self, S):
        """networkx.conductance(G, S) = cut_size / min(volume(S), volume(complement)); inf where networkx divides by zero."""
        return float(self._set_sweep(S, "conductance")["value"])

    def edge_expansion(self, S):
        """networkx.edge_expansion(G, S) = cut_size / min(|S|, |complement|); inf where networkx divides by zero."""
        return float(self._set_sweep(S, "edge_expansion", "expansion")["value"])

    def spectral_bisection(self, tol: float = 1e-10, m: int = 0, max_restarts: int = 300, seed: int = 0, objective: str = "conductance"):
        """The sweep cut of the Fiedler vector of a connected graph: (members, value, lambda2, info).  components() first (more
        than one component: ValueError -- bisect largest_component() instead); then eigsh(1, "SA") of the Laplacian with the
        constant vector deflated, and the sweep of its vector (sweep_cut).  info = eigsh's, with the sweep's result under "sweep".
        The operator option is set to the Laplacian for the solve and put back afterwards, on exceptions too.  Like eigsh, and
        like any change of the operator option, it voids a prepared chunked decomposition."""
        _, cinfo = self.components(want_labels=False)
        if cinfo["n_components"] != 1:
            raise ValueError(f"spectral_bisection: the graph has {cinfo['n_components']} components; bisect one of them, e.g. "
                             "largest_component()")
        if self.n < 2:
            raise ValueError("spectral_bisection: a graph of one vertex has no bisection")
        previous = self.operator
        self.set_option("operator", OP_LAPLACIAN)
        try:
            w, V, info = self.eigsh(1, "SA", m=m, tol=tol, max_restarts=max_restarts, seed=seed, deflate=np.full(self.n, 1.0 / np.sqrt(self.n)))
        finally:
            self.set_option("operator", previous)
        members, value, result = self.sweep_cut(V[:, 0], objective=objective)
        info["sweep"] = result
        return members, value, float(w[0]), info

    def local_cluster(self, seeds, method: str = "pagerank", alpha: float = 0.85, t: float = 1.0, k: int = 50, k_max: int = 0, tol: float = 1e-10):
        """A low-conductance set around every seed vertex: a diffusion from the seed, then the sweep of diffusion / degree
        (sweep_cut with per_degree=True and prefixes of at most k_max vertices, 0: n - 1).  method="pagerank": one
        pagerank(alpha, personalization=e_seed, tol=tol) per seed (Andersen, Chung and Lang).  method="heat": the heat kernel
        e^(-tL) e_seed by k Lanczos iterations (at most n), batched for up to 16 seeds (lanczos_multi and multout_multi under the
        Laplacian; Chung's heat-kernel PageRank); it replaces the resident batch basis and voids a prepared chunked
        decomposition, and the operator option is put back afterwards.  Up to 16 seeds share one sweep over the edges.  Returns
        one (members, value, result) per seed, as sweep_cut does; a scalar seed returns one."""
        if method not in ("pagerank", "heat"):
            raise ValueError(f"local_cluster: method must be 'pagerank' or 'heat', not {method!r}")
        ids = np.atleast_1d(np.asarray(seeds)).astype(np.int64)
        if ids.ndim != 1 or len(ids) == 0 or ids.min() < 0 or ids.max() >= self.n:
            raise ValueError(f"local_cluster: seeds must be vertices 0 .. {self.n - 1}")
        out = []
        for first in range(0, len(ids), SWEEP_BATCH):
            batch = ids[first:first + SWEEP_BATCH]
            X = np.zeros((len(batch), self.n))
            X[np.arange(len(batch)), batch] = 1.0
            out += self.sweep_cut(self._diffuse(X, method, alpha, t, k, tol), per_degree=True, k_max=k_max)
        return out[0] if np.ndim(seeds) == 0 else out

    def _diffuse(self, X, method, alpha, t, k, tol):
        """the diffusion of local_cluster from the seed indicators X (b, n), b <= 16: personalised PageRank, or e^(-tL) X"""
        if method == "pagerank":
            return np.vstack([self.pagerank(alpha, personalization=x, tol=tol) for x in X])
        k = max(1, min(int(k), self.n))
        previous = self.operator
        self.set_option("operator", OP_LAPLACIAN)
        try:
            a, b, _, xn, _, _ = self.lanczos_multi(X, k)
            T = np.vstack([_expm_coefficients(a[c], b[c][:k - 1], xn[c], -t) for c in range(len(X))])
            return self.multout_multi(T)
        finally:
            self.set_option("operator", previous)

    def bench_stream(self, nbytes: int = 1 << 30, reps: int = 5):
        rd, cp = ctypes.c_double(), ctypes.c_double()
        _check(self.L.lzx_bench_stream(self.h, nbytes, reps, ctypes.byref(rd), ctypes.byref(cp)), "lzx_bench_stream", self.L)
        return rd.value, cp.value

    def bench_spmv(self, reps: int = 20):
        avg, mn = ctypes.c_double(), ctypes.c_double()
        _check(self.L.lzx_bench_spmv(self.h, reps, ctypes.byref(avg), ctypes.byref(mn)), "lzx_bench_spmv", self.L)
        return avg.value, mn.value


class LocalGroup:
    """`world` handles wired as an in-process communicator (lzx_comm_init_local)."""

    def __init__(self, devices, **options):
        self.engines = [Engine(d, **options) for d in devices]
        self.L = self.engines[0].L
        self.world = len(devices)
        self.arr = (ctypes.c_void_p * self.world)(*[e.h for e in self.engines])
        _check(self.L.lzx_comm_init_local(self.arr, self.world), "lzx_comm_init_local", self.L)
        self.n = 0

    @classmethod
    def create(cls, devices):
        """the same group made by ONE call of the C ABI (lzx_create_group: SURVEY.md 8(b)'s `lzx_create(out, n_devices, device_ids)`)"""
        self = cls.__new__(cls)
        self.L = lib()
        self.world = len(devices)
        self.arr = (ctypes.c_void_p * self.world)()
        ids = (ctypes.c_int * self.world)(*devices)
        _check(self.L.lzx_create_group(self.arr, self.world, ids), "lzx_create_group", self.L)
        self.engines = []
        for h in self.arr:
            e = Engine.__new__(Engine)
            e.h, e.debug, e.L, e.n = ctypes.c_void_p(h), False, self.L, 0
            e.device = devices[len(self.engines)]
            self.engines.append(e)
        self.n = 0
        return self

    def set_graph_csr(self, row_ptr, col_idx):
        for e in self.engines:
            e.set_graph_csr(row_ptr, col_idx)
        self.n = self.engines[0].n

    def gen_rmat(self, scale, n, draws, seed, a=0.57, b=0.19, c=0.19):
        for e in self.engines:
            e.gen_rmat(scale, n, draws, seed, a, b, c)
        self.n = self.engines[0].n

    def gen_er(self, n, draws, seed):
        for e in self.engines:
            e.gen_er(n, draws, seed)
        self.n = self.engines[0].n

    def set_graph_edges(self, n, src, dst):
        for e in self.engines:
            e.set_graph_edges(n, src, dst)
        self.n = self.engines[0].n

    def spmv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty(self.n)
        _check(self.L.lzx_spmv_f64_local(self.arr, self.world, _p(x, _f64p), _p(y, _f64p)), "lzx_spmv_f64_local", self.L)
        return y

    def lanczos(self, x0, k: int, want_q: bool = True):
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        alpha = np.zeros(k)
        beta = np.zeros(max(k - 1, 1))
        Q = np.empty((k, self.n)) if want_q else None
        xn = ctypes.c_double()
        st = LzxStats()
        _check(self.L.lzx_lanczos_f64_local(self.arr, self.world, _p(x0, _f64p), k, _p(alpha, _f64p),
                                           _p(beta, _f64p), _p(Q, _f64p) if want_q else None,
                                           ctypes.byref(xn), ctypes.byref(st)), "lzx_lanczos_f64_local", self.L)
        return alpha, beta[:k - 1], Q, xn.value, st.as_dict()

    def multout(self, t):
        t = np.ascontiguousarray(t, dtype=np.float64)
        ans = np.empty(self.n)
        _check(self.L.lzx_multout_f64_local(self.arr, self.world, _p(t, _f64p), len(t), _p(ans, _f64p)), "lzx_multout_f64_local", self.L)
        return ans

    def expm_multiply(self, x0, k: int, t: float = 1.0):
        """Engine.expm_multiply over the group (the handles' operator)."""
        alpha, beta, _, xn, _ = self.lanczos(x0, k, want_q=False)
        s = -t if getattr(self.engines[0], "operator", OP_ADJACENCY) == OP_LAPLACIAN else t
        return self.multout(_expm_coefficients(alpha, beta, xn, s))

    def lanczos_multi(self, X0, k: int, want_q: bool = False):
        """The batched path is one-GPU: the library refuses a handle of a communicator (LzxError naming the group's size)."""
        return self.engines[0].lanczos_multi(X0, k, want_q)

    def close(self):
        for e in self.engines:
            e.close()
