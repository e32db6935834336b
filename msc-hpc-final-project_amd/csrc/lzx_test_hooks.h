// lzx_test_hooks.h -- test-only entry of liblzx.so (NOT part of the boundary in include/lzx.h; the drop-in classes never call it).
// Forces the table shapes that large graphs get by themselves onto small test graphs, so that tests/ exercise the product
// library's own kernels in every shape: "pb_reduce" (minimum run length of a reduced run; 0 = every run plain), "pb_target"
// (values per gather item), "pb_unit" (entries per scatter unit), "pb_column_band" (8192 | 16384 | 18432: the last on one rank only), "pb_run_align", "pb_taper",
// "pb_dyn_share" (per cent of the gather pass left to its dynamic tail; 0 = every item dealt by the host), "pb_gather_grid" (at most this many gather workgroups),
// "pb_gather_nt" (the gather pass's stream loads non-temporal 1 / cached 0, whatever the stream's size),
// "pb_group" / "pb_group_force" (small row bands gathered one wavefront each), "narrow_slices", "tie_sort", "long_row",
// "item_len", "spmv_wgs" (at most this many workgroups of k_spmv, and staged-columns workgroups of the blocked SpMV's shared launch; never
// more than the default rule's ceiling of workgroups per CU and of one wavefront per slice or item), "exchange_at_world_1" (a 1-rank RCCL communicator runs the several-rank loop, collectives included),
// "pb_carry_scan" (reduced steps: a row that spans lanes summed by the fixed-order cross-lane scan 1 / through LDS carry slots 0),
// "isolated_rows" (0: rows without an edge updated elementwise instead of as one scalar recurrence), "unnormalised_basis" (0: the
// resident basis holds q_j instead of u_j), "fuse_staged" (0: staged-columns kernel in a launch of its own; 1: behind the
// scatter units of the shared launch instead of ahead of them), "start_vector_scan" (0: lzx_lanczos_prepare_f64 always uploads x0 and
// sums its squares in one serial chain; default: one look at x0 first -- a constant vector is filled on the device, a sum that is
// exact in any order is formed by several threads), "defer_finish" (0: the blocked SpMV always launches k_pb_finish; default: in the lazy loop
// k_lazy_update adds the totals of multi-item gather bands where it reads v and the launch is left out), "multi_row_chunk" (entries per
// chunk of a split row in the batched SpMM of lzx_multi.hip; default 2048), "eig_basis_bytes" (lzx_eigsh_f64 takes a basis larger than this
// many bytes as out of device memory), "solve_state_bytes" (the same for the state of lzx_solve_shifted_f64 and of lzx_pagerank_f64), "solve_poll" (iterations
// between the status polls of those two; default 16), "bfs_state_bytes" (lzx_bfs_multi and lzx_betweenness_f64 take a state larger than this many
// bytes as out of device memory; their long rows are the batched SpMM's: "multi_row_chunk"), "tri_long_list" (lzx_triangles: a row of the
// oriented copy with more than this many entries is counted by the wide kernel, a workgroup per row and a wavefront per out-edge, and only
// lists of at most 32 times this many entries, 4096 at the most, are staged in LDS there; default 128), "tri_state_bytes" (lzx_triangles
// takes a state larger than this many bytes as out of device memory), "core_long_row" (lzx_core_numbers: a row of the frontier with more than
// this many entries is peeled by the long-row launch, a workgroup per row and slice of its entries; default 64 times the lanes per row,
// 256 to 2048 from the mean degree), "core_state_bytes" (lzx_core_numbers takes a state larger than this many bytes as out of device
// memory, before the device is touched), "truss_long_row" (lzx_truss: an edge of the frontier whose shorter row has more than this many
// entries is peeled by the long-row launch, a workgroup per edge and slice of that row; default 64 times the lanes per edge, 256 to 2048
// from the mean degree; its wide support kernel splits at "tri_long_list"), "truss_state_bytes" (lzx_truss takes a state larger than this
// many bytes as out of device memory, at either of its two allocations), "color_long_row" (lzx_color and the colouring of
// lzx_label_propagation: a row with more than this many entries is counted and coloured by the long-row launches, a workgroup per row with
// an LDS bitmap of colours; default 64 times the lanes per row), "lpa_group_row" (lzx_label_propagation: a row of at most this many entries
// is updated by a group of lanes, which stages the first 128 labels in LDS and reads the rest of a longer row where it lies; default 128),
// "lpa_table_row" (a longer row of at most this many entries is counted in the LDS table by a workgroup, the rest in a table in global
// memory; default and at most 2048, half the LDS table's slots), "lpa_state_bytes" (lzx_label_propagation takes a state larger than this many
// bytes as out of device memory, at the vertices' arena before the device is touched and at the global tables), "louvain_state_bytes"
// (lzx_louvain, which honours "color_long_row", "lpa_group_row" and "lpa_table_row" on every level graph, takes a state larger than this
// many bytes as out of device memory at each of its allocations: the vertices' arena, a level's global tables, the aggregation's keys
// and weights, a level graph -- the bytes held plus the bytes asked for), "sweep_long_row"
// (lzx_sweep_cut: a row with more than this many entries is swept by the long-row launch, a workgroup per row; default 64 times the
// lanes per row), "sweep_state_bytes" (lzx_sweep_cut takes a state larger than this many bytes as out of device memory, before the
// device is touched), "sim_long_pair" (lzx_similarity: a pair whose shorter row has more than this many entries is intersected by a
// workgroup of its own instead of a group of lanes; default 64 times the lanes per pair), "sim_slice" (such a pair whose shorter row
// also has more than this many entries is dealt to one workgroup per slice of that many entries, 64 at the most, whose partials a
// closing launch adds in slice order; default 16384), "sim_state_bytes" (lzx_similarity takes a state larger than this many bytes as
// out of device memory, at either of its two allocations), "graph_lanes" (lzx_components, lzx_triangles, lzx_core_numbers, lzx_truss,
// lzx_color, lzx_label_propagation, lzx_modularity, lzx_louvain, lzx_sweep_cut and lzx_similarity: 4 | 8 | 16 | 32 | 64 lanes per row in every kernel
// template they launch, in place of the rule on the mean row length and capped at the widest instantiation of each launch -- 64 for the
// orientation pass and lzx_truss's per-row passes, 32 elsewhere; 0, or -1 like every unset shape: the rule; any other value is refused
// with LZX_ERR_ARG.  The defaults of "core_long_row", "truss_long_row", "color_long_row", "sweep_long_row", "sim_long_pair" and
// lzx_components's split, 64 times the lanes, follow the forced width).
#pragma once
#include <stdint.h>
#include "lzx.h"
#ifdef __cplusplus
extern "C"
#endif
int lzx_test_set_shape(lzx_handle h, const char *name, int64_t value);
// what shape the tables of the handle's graph took: "gather_items_dealt" / "gather_items_drawn" (static lists / dynamic tail of
// the gather pass), "gather_workgroups", "placement_tried" / "placement_kept" / "placement_us_<i>" (option placement_trials: candidates of
// the value stream timed at the last hand-over, the one kept, the SpMV time of candidate i in microseconds), "start_vector_was_constant"
// (the last prepared x0 was filled on the device instead of uploaded), "finish_launched" / "finish_deferrable" (the graph's blocked SpMV has a
// k_pb_finish launch / the lazy loop may leave it out), "row_bands" / "pb_runs" / "pb_steps" / "scatter_units" (what the builder of the
// blocked tables counted: row bands, (row band, column band) runs, 512-entry steps of the reduced runs, scatter work units; read-only,
// 0 when blocking is off -- tests/pb_model.py restates the rules they follow); and what lzx_graph_prepare (steps 3 to 5) counted for
// the other half of the SpMV, the sliced-ELL body and the split rows that spmv_body takes, in plain and in blocked mode (read-only;
// tests/sell_model.py restates the rules they follow): "split_rows" (rows handled as split rows: through the last row over the
// threshold, rounded up to whole slices, at most the padded rows), "split_items" (work items of those rows), "body_slices" (64-row
// slices behind them), "slices_wide" / "slices_w8" / "slices_w4" / "slices_w0" (slices the general loop takes, and those of 8, 4 and
// 0 codes per row that the class loops take; without classes slices_wide == body_slices and the rest is 0), "staged_workgroups"
// (workgroups of k_spmv, or staged-columns workgroups of the shared launch), "split_entries" / "body_entries" (padded codes in the two
// tables; info's sell_padded is their sum), "staged_x_stride" (slice stride of chunk 0 of the exchange layout: the staged value of
// degree rank r is read at (r % world) * stride + r / world), "live_rows" (this rank's rows with an edge, rounded up to whole slices);
// and what lzx_multi_build_tables counted for the batched path's work list (read-only; each reads 0 until the tables exist, that is
// until the first batched call on the graph -- lzx_spmm_f64, lzx_lanczos_multi_f64, the probe entries, lzx_solve_multi_f64,
// lzx_bfs_multi, lzx_betweenness_f64; tests/multi_model.py restates the rules they follow): "multi_chunk" (the L the list was built
// with: multi_row_chunk, or 2048), "multi_work_items" (entries of the work list, one per unsplit row and per chunk of a split row,
// padded to a multiple of 32), "multi_split_rows" (rows of more than L entries), "multi_chunk_slots" (their chunks: one slot of
// chunk totals each), "multi_row_segments" (2048-row segments, one partial per column each: ceil(n / 2048)), "multi_vector_grid"
// (min(max(multi_row_segments, 1), 4 x compute units): the workgroups of k_multi_update and of k_multi_alpha's launch, which
// stride over the row segments); and the lanes per row the last graph call on the handle ran (read-only; 0 before the first):
// "graph_lanes_rows" (of its launches over the caller-order rows; where they differ the widest -- lzx_truss peels over min(that, 32)
// lanes per edge), "graph_lanes_oriented" (of its launches over the oriented copy: the counting kernel of lzx_triangles, the support
// kernel of lzx_truss; 0 for a call without an oriented copy or without an edge in it)
#ifdef __cplusplus
extern "C"
#endif
int lzx_test_get_shape(lzx_handle h, const char *name, int64_t *value);
// One rank's share checked without its peers (a rank of an in-process group whose other handles hold no graph; C5's rank
// share on the one-GPU test box): this handle's LOCAL SpMV of x = 1 -- the row sums of its own rows, integers, exactly the
// rows' degrees when its tables are right -- into v_local[0 .. rows_local), and the position of every vertex of the caller's
// order in the full-length layout (rank * n_loc_pad + local row) into layout_pos[0 .. n), so that the caller can tell which
// vertex a local row is.  Voids a prepared decomposition, like lzx_bench_spmv.
#ifdef __cplusplus
extern "C"
#endif
int lzx_test_rank_row_sums(lzx_handle h, double *v_local, uint32_t *layout_pos, uint64_t *n_loc_pad);
// Latency of the communicator's two-double all-reduce: `reps` of them queued back to back on the handle's main stream between
// two events, microseconds each (collective: every rank calls it with the same reps; transports RCCL and peer windows).
#ifdef __cplusplus
extern "C"
#endif
int lzx_test_allreduce_latency(lzx_handle h, uint32_t reps, double *us_each);
// The eigensolver's dense symmetric solver (lzx_eig.hip, cyclic Jacobi), no GPU needed: A is n x n row-major (n <= 1024),
// w the eigenvalues ascending, V[i * n + j] component i of the unit eigenvector of w[j].
#ifdef __cplusplus
extern "C"
#endif
int lzx_test_sym_eig(uint32_t n, const double *A, double *w, double *V);
// The eigensolver's dense device kernels on a caller's basis (lzx_eig.hip), through the launches lzx_eigsh_f64 itself uses.  The
// handle holds a graph (n vertices; its layout is the basis's: stride ldq, padding rows 0); 1 <= J <= 137, 1 <= p <= J, and
// J <= 128 when R is wanted.  Q: J columns of n doubles, w: n doubles, both in the caller's vertex order.  First the
// Gram-Schmidt of one Lanczos step: w orthogonalised twice against the J columns (k_eig_proj, k_eig_close, k_eig_update) and
// made unit (k_eig_scale): coef[c] = h1[c] + h2[c], what the solver stores as its column of H; *beta = the norm of what is
// left of w; w_out = that divided by beta.  Then, with R, the restart's rotation (k_eig_rotate, in place, Y padded to rows of
// a multiple of 8 as the driver pads it): R[i] = column i of Q Y for i < p, Y being J rows of p doubles.  coef, w_out, beta
// and R may each be null.  Argument errors come back before the device is touched; voids a prepared decomposition.
#ifdef __cplusplus
extern "C"
#endif
int lzx_test_eig_ops(lzx_handle h, uint32_t J, uint32_t p, const double *Q, const double *w, const double *Y, double *coef,
                     double *w_out, double *beta, double *R);
