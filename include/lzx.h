/*
 * lzx.h -- C ABI of the MI355X-native Lanczos e^A x engine (liblzx.so).
 *
 * This is the drop-in boundary for the hot path of hdelan/MSc-HPC-Final-Project
 * (SURVEY.md section 8): everything `lanczosDecomp<T>::cu_decompose()` does on the
 * device in parallel-final, behind plain pointers and sizes.  The reference has no
 * FFI of its own (one C++ binary); each entry point below names the reference
 * code it replaces (paths relative to the reference repository root).
 *
 * Conventions
 *   - every function returns LZX_OK (0) or a negative lzx_status; the message of
 *     the last failure on the calling thread is lzx_last_error();
 *   - all pointers are HOST pointers owned by the caller unless a name ends in
 *     `_dev`; the library owns all device memory;
 *   - a handle is bound to one GPU and is not thread-safe; distinct handles are;
 *   - the graph is an undirected, unweighted adjacency matrix handed over as
 *     pattern-only CSR (no values array): symmetric, columns ascending within a
 *     row, no duplicates -- what adjMatrix holds (parallel-final/lib/adjMatrix.h:26-30);
 *   - vertex order at this boundary is always the caller's; the library is free
 *     to (and does) relabel internally.
 */
#ifndef LZX_H_
#define LZX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lzx_ctx *lzx_handle;

typedef enum lzx_status {
    LZX_OK = 0,
    LZX_ERR_ARG = -1,    /* bad argument (null pointer, k == 0, sizes that do not match) */
    LZX_ERR_HIP = -2,    /* a HIP runtime call or kernel launch failed                   */
    LZX_ERR_STATE = -3,  /* call order: no graph yet, no decomposition yet, ...          */
    LZX_ERR_NOMEM = -4,  /* host or device allocation failed                             */
    LZX_ERR_COMM = -5,   /* RCCL not loadable / communicator failure                     */
    LZX_ERR_LIMIT = -6   /* size outside what this build supports (nnz per rank >= 2^32) */
} lzx_status;

/* Timings of the last lzx_lanczos_f64 call (all in milliseconds).  The three per-category sums come from HIP events
 * recorded on the loop's stream.  Every event is a barrier packet (about 5 us of drained pipeline between two dependent
 * kernels), so only every 4th iteration carries them (every iteration when k < 8, or with option "timing_marks_every"
 * = 1) and the sums are scaled to all k iterations. */
typedef struct lzx_stats {
    double loop_ms;       /* host wall clock around the k-iteration loop, device-synchronised on both
                             sides; excludes upload of x0 and download of alpha/beta/Q              */
    double spmv_ms;       /* sum over iterations of the SpMV(+alpha partial) launches, HIP events on
                             the stream they run on                                                */
    double spmv_ms_min;   /* fastest single iteration's SpMV time                                   */
    double vec_ms;        /* sum of the vector kernel launches (several ranks: + the scalar all-reduce) */
    double comm_ms;       /* sum of the exposed part of the all-gather(s), 0 at one rank            */
    uint32_t iters;       /* k                                                                      */
    uint32_t spmv_kernels;/* kernel launches counted in spmv_ms per iteration                       */
    uint64_t spmv_bytes;  /* algorithmic bytes of ONE SpMV on this rank:
                             4*nnz_local + 4*(rows_local+1) + 8*n (x once) + 8*rows_local (y)       */
} lzx_stats;

typedef struct lzx_graph_info {
    uint64_t n;           /* vertices (global)                                   */
    uint64_t nnz;         /* stored entries of the whole matrix = 2 * undirected edges */
    uint64_t max_degree;
    uint64_t rows_local;  /* rows this rank owns                                 */
    uint64_t nnz_local;   /* entries in those rows                               */
    uint64_t long_rows;   /* local rows handled by the split-row path            */
    uint64_t sell_padded; /* entries of the sliced-ELL body including padding    */
    uint64_t pb_entries;  /* local entries handled by the propagation-blocked passes (0 = mode off) */
    uint64_t active_vertices; /* vertices with at least one edge (global)         */
    uint64_t exchange_slice;  /* doubles each rank contributes to the per-iteration all-gather */
    uint32_t hub_entries; /* x entries staged in LDS per workgroup               */
    uint32_t world, rank;
    uint32_t reserved_;
    uint64_t pb_values;   /* values the blocked scatter passes hand to the gather pass per SpMV (padding included) */
    uint64_t pb_reduced_entries; /* of pb_entries: entries of the reduced bands, which travel as partial row sums */
    uint64_t exchange_chunk0;    /* doubles per rank in the first of the two all-gathers that overlap the blocked SpMV
                                    (0 = one all-gather per iteration) */
    uint64_t exchange_recv;      /* doubles this rank receives from the OTHER ranks per iteration: (world - 1) *
                                    exchange_slice with the plain all-gather; with the two-chunk exchange chunk 1 is
                                    sparse -- each peer sends only the entries this rank's rows reference -- and this
                                    is (world - 1) * exchange_chunk0 + what the peers pack for this rank */
    uint32_t placement_tried;    /* option "placement_trials": allocations of the value stream timed at the hand-over (the
                                    first one included; 0 = nothing to choose), */
    uint32_t placement_kept;     /* the one kept, */
    uint32_t placement_us[8];    /* and the SpMV time measured with each, in microseconds */
} lzx_graph_info;

/* ---- lifetime -------------------------------------------------------------------------------- */

/* Create an engine on GPU `device_id`.  Replaces the cudaMalloc/cudaStreamCreate block of
 * cu_decompose (parallel-final/lib/cu_lanczos.cu:37-86); unlike it, failure leaves nothing
 * half-built.                                                                                    */
int lzx_create(lzx_handle *out, int device_id);
/* GPUs visible to this process (0 when there is no usable device: never an error).  The drop-in classes use it to
 * decide between the device ingest and the host loader and to spread a decomposition over several cards, as
 * parallel-two-cards drives its two from one process (parallel-two-cards/lib/cu_lanczos.cu:73-190). */
int lzx_device_count(int *count);
void lzx_destroy(lzx_handle h);
const char *lzx_last_error(void);

/* ---- multi-GPU wiring (optional; call before handing over the graph) ----------------------------
 * Rows are dealt to ranks by degree rank (round-robin), every rank keeps a full-length copy of the
 * current Lanczos vector, and each iteration ends with an all-gather of the owned slices plus two
 * one-double all-reduces.  Replaces parallel-two-cards' split at rows0 = n/2 and its two
 * cudaMemcpyPeer per iteration (parallel-two-cards/lib/cu_lanczos.cu:62-67,125,158).
 *   lzx_comm_unique_id / lzx_comm_init_rank : one process per GPU, RCCL over xGMI.  Rank 0 makes the
 *       128-byte id, the caller ships it to the other ranks (any side channel), everyone calls init.
 *   lzx_comm_init_local : `world` handles inside ONE process (the reference's own two-cards model,
 *       any number of cards); exchanges are device-to-device copies.  Handles may share a GPU.      */
int lzx_comm_unique_id(uint8_t id[128]);
int lzx_comm_init_rank(lzx_handle h, const uint8_t id[128], int rank, int world);
/* SURVEY.md 8(b)'s sketch of the boundary in one call: `n_devices` handles, out[i] on GPU device_ids[i] (NULL: GPUs 0 .. n_devices - 1;
 * ids may repeat: handles may share a GPU), wired as ONE in-process communicator (lzx_create + lzx_comm_init_local) -- the
 * reference's parallel-two-cards model (one process, cudaSetDevice per card: parallel-two-cards/lib/cu_lanczos.cu:73-190) for
 * any number of cards.  Use the handles with the *_local entry points; destroy each with lzx_destroy.  On failure nothing is
 * left behind and every out[i] is NULL.                                                                                       */
int lzx_create_group(lzx_handle *out, int n_devices, const int *device_ids);
int lzx_comm_init_local(lzx_handle *hs, int world);
/*   lzx_comm_ipc_export / lzx_comm_ipc_init : one process per rank WITHOUT a collective library ("peer windows"): every
 *       rank's receive buffers are mapped into its peers (HIP inter-process memory handles), each rank's own kernel
 *       pushes its slice straight into them -- over xGMI point to point between GPUs, the access pattern
 *       parallel-two-cards/lib/cu_lanczos.cu:62-67 enables with cudaDeviceEnablePeerAccess -- and the iteration's two
 *       scalars travel through mailboxes in device memory (the host round trips of cu_lanczos.cu:104-105,119-120 gone).
 *       Ranks may share a GPU.  Every rank calls export (LZX_IPC_BLOB bytes out), the caller gathers the `world` blobs
 *       in rank order over any side channel, every rank calls init with the whole list.  A peer that does not arrive
 *       within LZX_IPC_TIMEOUT_MS (environment, default 20000) makes the call in progress fail with LZX_ERR_COMM.     */
#define LZX_IPC_BLOB 128
int lzx_comm_ipc_export(lzx_handle h, uint8_t blob[LZX_IPC_BLOB]);
int lzx_comm_ipc_init(lzx_handle h, const uint8_t *blobs /* [world][LZX_IPC_BLOB] */, int rank, int world);

/* ---- graph hand-over ---------------------------------------------------------------------------
 * lzx_set_graph_csr: upload of IA/JA, parallel-final/lib/cu_lanczos.cu:88-94 (`row_offset[n+1]`,
 * `col_idx[2E]`).  row_ptr is 64-bit as in serial/ (serial/lib/adjMatrix.h:23-24);
 * lzx_set_graph_csr32 takes parallel-final's `unsigned` arrays as they are.  Every rank of a
 * communicator passes the same whole graph and keeps its share (with option "sharded_ingest" the graph
 * never sits whole on any device: the CSR is streamed from the caller's memory).                  */
int lzx_set_graph_csr(lzx_handle h, uint64_t n, uint64_t nnz, const uint64_t *row_ptr,
                      const uint32_t *col_idx);
int lzx_set_graph_csr32(lzx_handle h, uint32_t n, uint32_t nnz, const uint32_t *row_ptr,
                        const uint32_t *col_idx);

/* Device-side ingest: `m` undirected edges as 0-based endpoint pairs, in any
 * order, duplicates allowed; symmetrised, sorted and de-duplicated on the GPU into the CSR that
 * adjMatrix::populate_sparse_matrix builds with a std::set (parallel-final/lib/adjMatrix.cc:21-46):
 * a self loop becomes one diagonal entry, as it does there.  Endpoints >= n are an LZX_ERR_ARG.   */
int lzx_set_graph_edges(lzx_handle h, uint64_t n, uint64_t m, const uint32_t *src, const uint32_t *dst);

/* Seeded synthetic graphs generated on the GPU (the reference's generators are seeded from
 * std::random_device, parallel-final/lib/make_graph.cc:23-24,61-62, and cannot be reproduced).
 * Integer specification shared with oracle/lanczos_oracle.c (orc_gen_er_keys, orc_gen_rmat_keys).
 * kind 0: Erdos-Renyi G(n, draws); kind 1: R-MAT with `scale` levels, 16-bit thresholds ta/tab/tabc,
 * endpoints >= n re-drawn (up to 8 attempts).                                                      */
int lzx_gen_graph(lzx_handle h, int kind, uint32_t scale, uint64_t n, uint64_t draws, uint64_t seed,
                  uint32_t ta, uint32_t tab, uint32_t tabc);

int lzx_get_graph_info(lzx_handle h, lzx_graph_info *out);
/* Copy the whole-graph CSR (caller's vertex order) back to the host: row_ptr[n+1], col_idx[nnz]. */
int lzx_get_graph_csr(lzx_handle h, uint64_t *row_ptr, uint32_t *col_idx);

/* ---- hot path ----------------------------------------------------------------------------------
 * lzx_spmv_f64: y = A x.  Kernel-level parity hook for cu_spMV1 (parallel-final/lib/cu_SPMV.cu:31-41)
 * and CPU spMV (serial/lib/SPMV.cc:19-28).  x[n], y[n] in the caller's vertex order.              */
int lzx_spmv_f64(lzx_handle h, const double *x, double *y);
int lzx_spmv_f64_local(lzx_handle *hs, int world, const double *x, double *y);

/* lzx_lanczos_f64: the whole k-step loop of cu_decompose (parallel-final/lib/cu_lanczos.cu:97-130),
 * i.e. serial/lib/lanczos.cc:9-56 on the device:
 *     q_0 = x0/||x0||;  for j<k: v = A q_j; alpha_j = v.q_j; v -= alpha_j q_j; v -= beta_{j-1} q_{j-1};
 *                                 beta_j = ||v||; q_{j+1} = v/beta_j          (last two only for j<k-1)
 * Outputs: alpha[k], beta[k-1] (beta may be NULL when k == 1), x_norm (may be NULL), and, when Q is
 * not NULL, Q[k*n] as k contiguous vectors -- the layout cu_decompose leaves on the host
 * (&Q[k*n], cu_lanczos.cu:126) and multOut consumes with Qtrans = true
 * (parallel-final/lib/multiplyOut.cu:42-44).  The basis also stays resident on the device for
 * lzx_multout_f64.  No breakdown guard for beta_j == 0, as in the reference.
 * With a communicator every rank must call it with the same arguments.                           */
int lzx_lanczos_f64(lzx_handle h, const double *x0, uint32_t k, double *alpha, double *beta,
                    double *Q, double *x_norm, lzx_stats *stats);
/* lzx_lanczos_f64 in three steps, so that a caller can bracket exactly the loop (inputs already in HBM):
 *   prepare: upload x0, q_0 = x0/||x0||, size the resident basis      (cu_lanczos.cu:30-34,88-94)
 *   run    : the k iterations, stream-synchronised on return           (cu_lanczos.cu:97-128)
 *   fetch  : alpha[k], beta[k-1], optionally Q[k*n]                     (cu_lanczos.cu:126,129-130)   */
int lzx_lanczos_prepare_f64(lzx_handle h, const double *x0, uint32_t k, double *x_norm);
int lzx_lanczos_run(lzx_handle h, lzx_stats *stats);
int lzx_lanczos_fetch_f64(lzx_handle h, uint32_t k, double *alpha, double *beta, double *Q);
int lzx_lanczos_fetch_f64_local(lzx_handle *hs, int world, uint32_t k, double *alpha, double *beta, double *Q);
/* The same loop in chunks (the reference's open problem of choosing k: parallel-final/lib/
 * multiplyOut.cu:25-49 can only evaluate a decomposition that has already run all its iterations; writeup section 11).
 * After lzx_lanczos_prepare_f64(h, x0, k_max, ..) each call runs up to `steps` more iterations of the SAME decomposition
 * -- every piece of loop state lives in HBM, so k iterations in chunks give the bits of k iterations in one go -- and
 * after every call alpha / beta / the basis of the iterations done so far can be used (lzx_lanczos_fetch_f64,
 * lzx_multout_f64, lzx_multout_change_f64 with k <= done), so that a caller who sees its answer converge stops paying for
 * SpMVs.  lzx_lanczos_run == run_steps(all that is left).  lzx_spmv_f64 / lzx_bench_spmv between two chunks void the
 * prepared state (LZX_ERR_STATE on the next chunk); lzx_multout* and lzx_lanczos_fetch* do not.
 * lzx_lanczos_progress: iterations done / prepared (prepared == 0: nothing to resume).                            */
int lzx_lanczos_run_steps(lzx_handle h, uint32_t steps, lzx_stats *stats);
int lzx_lanczos_run_steps_local(lzx_handle *hs, int world, uint32_t steps, lzx_stats *stats);
int lzx_lanczos_prepare_f64_local(lzx_handle *hs, int world, const double *x0, uint32_t k, double *x_norm);
int lzx_lanczos_progress(lzx_handle h, uint32_t *done, uint32_t *prepared);
/* Wait for everything queued on the handle's stream. */
int lzx_sync(lzx_handle h);
/* The same over `world` handles wired with lzx_comm_init_local, driven by one host thread. */
int lzx_lanczos_f64_local(lzx_handle *hs, int world, const double *x0, uint32_t k, double *alpha,
                          double *beta, double *Q, double *x_norm, lzx_stats *stats);

/* lzx_multout_f64: ans = Q t on the device-resident basis of the last decomposition (t[k] is
 * V (e^lambda * ||x|| * V[0,:]) computed by the host as in parallel-final/lib/multiplyOut.cu:30-40;
 * this call is the second dgemv, :42-46; cf. parallel-mult-on-card/lib/cu_multiplyOut.cu:66-71).
 * ans[n] in the caller's vertex order, complete on every rank.                                   */
int lzx_multout_f64(lzx_handle h, const double *t, uint32_t k, double *ans);
int lzx_multout_f64_local(lzx_handle *hs, int world, const double *t, uint32_t k, double *ans);

/* Convergence monitor without the n-vector crossing PCIe: y_k = Q_k t is formed on the device as in lzx_multout_f64 and
 * kept there; *rel_change = ||y_k - y_prev||_2 / ||y_k||_2 against the answer of the previous call since the last
 * prepare (1.0 for the first call).  The host-side stopping rule of multOutAdaptive (host/multiplyOut.cc) on two scalars. */
int lzx_multout_change_f64(lzx_handle h, const double *t, uint32_t k, double *rel_change);
int lzx_multout_change_f64_local(lzx_handle *hs, int world, const double *t, uint32_t k, double *rel_change);

/* ---- batched, independent Lanczos (one GPU) -----------------------------------------------------
 * b separate three-term recurrences, one per column of X = [x_1 .. x_b], that share ONE SpMM per iteration: with the b
 * vectors stored interleaved per vertex ([n][B], B = b padded to 2, 4, 8 or 16) one col_idx read and one gathered row of X
 * serve every column.  Not block Lanczos (no QR of a block, no coupling between columns): each column runs the recurrence of
 * lzx_lanczos_f64, plus a breakdown stop of its own, decided on the device -- after beta_{c,j} (j < k-1) column c stops when
 *     beta_{c,j} <= 2^-40 * max_{i<=j} (|alpha_{c,i}| + beta_{c,i-1}),   beta_{c,-1} = 0;
 * its beta_{c,j} and later alpha / beta are then returned as 0, its later basis vectors are zero, k_used[c] = j+1, and the
 * other columns go on.  (Without it a seed vector e_v of a small component -- communicability of a seed vertex -- would
 * divide by a rounding-level beta.)  Column c's alpha, beta, k_used, basis and answer are bit-identical whatever else is in
 * the batch (every reduction's shape depends on n alone).  The SpMM works on the caller-order CSR the handle keeps: every row
 * of at most 2048 entries is summed with one accumulator in ascending column order (bit-identical to lzx_spmv_f64's
 * reference, serial/lib/SPMV.cc:19-28); a longer row is cut into chunks of 2048 entries whose totals are added in chunk
 * order.  The work list behind it is built on first use and lives as long as the graph.
 * The batch state (basis, work vectors) is separate from the single-vector state: a batched call neither voids a prepared or
 * chunked single-vector decomposition nor touches its resident basis.  One rank only: a handle with a communicator gets
 * LZX_ERR_STATE.  A new graph and lzx_destroy free the batch state too.
 *
 * lzx_lanczos_multi_f64: b in [1, 16]; X0: b contiguous vectors of n (caller order); alpha, beta: [b][k] (beta[c][k-1]
 * unused, returned 0); k_used[b], x_norm[b] (||x_c||, left-to-right sum of squares as lzx_lanczos_prepare_f64 forms it);
 * Q (may be NULL): [b][k][n].  The basis stays resident for lzx_multout_multi_f64.  Errors: LZX_ERR_ARG for null pointers,
 * k == 0, b == 0 or an all-zero column; LZX_ERR_LIMIT for b > 16; LZX_ERR_NOMEM when the basis (k * n * B * 8 bytes) does
 * not fit -- the message states the bytes and no batch state is left behind.  stats: loop_ms (host clock around the k
 * iterations), spmv_ms (SpMM + the split-row / alpha-partial launch), vec_ms (the update and scale launches), spmv_kernels
 * = launches per iteration (4), spmv_bytes = the algorithmic bytes of ONE SpMM, 4*nnz + 8*(n+1) + 8*b*n (X once) + 8*b*n (Y). */
int lzx_lanczos_multi_f64(lzx_handle h, uint32_t b, const double *X0, uint32_t k, double *alpha, double *beta,
                          uint32_t *k_used, double *x_norm, double *Q, lzx_stats *stats);
/* ans[b][n] = per column Q_c t_c on the resident batch basis; T: [b][k] (entries >= k_used[c] ignored).  b must be the
 * resident batch's, k at most its k (LZX_ERR_ARG otherwise; LZX_ERR_STATE when no batch is resident).                  */
int lzx_multout_multi_f64(lzx_handle h, uint32_t b, const double *T, uint32_t k, double *ans);
/* Y[b][n] = A X[b][n]: kernel-level parity hook of the batched SpMM, like lzx_spmv_f64.  Leaves a resident batch basis
 * and a prepared single-vector decomposition alone.                                                                    */
int lzx_spmm_f64(lzx_handle h, uint32_t b, const double *X, double *Y);
/* Give back the batch basis and work vectors (they are also freed by a new graph and by lzx_destroy). */
int lzx_multi_release(lzx_handle h);

/* ---- stochastic Lanczos quadrature on the batched path (one GPU) ---------------------------------
 * Random +-1 probe vectors z_p for estimates of tr f(M) and diag f(M) (M = A, or L under the option "operator"): the
 * batched recurrence above started from probes generated on the device, optionally without a basis.
 * Probe p (0 <= p < 2^32) at vertex i (caller order, 0 <= i < n), all arithmetic mod 2^64:
 *     key = seed + 0x9E3779B97F4A7C15 * ((p << 32) + i + 1)
 *     h = key; h ^= h >> 30; h *= 0xBF58476D1CE4E5B9; h ^= h >> 27; h *= 0x94D049BB133111EB; h ^= h >> 31
 *     z_p[i] = (h >> 63) ? -1.0 : +1.0
 * It depends on neither the internal vertex order nor how the probes are split into batches.
 * Errors of all three, as for the batched entries: LZX_ERR_ARG for a null handle or pointer, b == 0, k == 0 or
 * first + b > 2^32; LZX_ERR_LIMIT for b > 16; LZX_ERR_STATE for a handle with a communicator or without a graph.
 *
 * lzx_probes_f64: Z[b][n] = probes first .. first + b - 1.  Leaves the resident batch basis alone.
 *
 * lzx_lanczos_probes_f64: lzx_lanczos_multi_f64 with X0 = lzx_probes_f64(seed, first, b): alpha, beta, k_used ([b][k], [b])
 * bit-identical to it, flags or not; the implied x_norm is sqrt(n) (the exact norm of a +-1 vector).  q_0 = z_p / sqrt(n)
 * is written on the device (no host upload).
 *   flags = 0: basis-free.  q_{j-1}, q_j, q_{j+1} rotate through three [n][B] slots, so the batch state is about
 *     4 * n * B * 8 bytes (slots and one work vector) plus the work list, whatever k is; any resident batch basis is given
 *     back first and none is resident afterwards (lzx_multout_multi_f64 / lzx_probe_diag_f64: LZX_ERR_STATE).
 *   flags = LZX_PROBE_KEEP_BASIS: the [k][n][B] basis is kept as the resident batch basis, for lzx_multout_multi_f64
 *     and lzx_probe_diag_f64.  LZX_ERR_NOMEM when it does not fit: the message states the bytes and no batch state is
 *     left behind.
 * stats as for lzx_lanczos_multi_f64 (spmv_bytes keeps its formula).  Any other flag bit: LZX_ERR_ARG.
 *
 * lzx_probe_diag_f64: out[n] = sum over the resident probe batch's columns c, ascending, of z_c .* (Q_c t_c), where
 * Q_c t_c is exactly lzx_multout_multi_f64's answer for T ([b][k], b the batch's, k at most its k; entries >= k_used[c]
 * ignored) and z_c is probe c (multiplied exactly: +-1).  Only the n-vector leaves the device.  LZX_ERR_STATE unless the
 * resident basis is a kept probe basis (after a basis-free run, or a basis of lzx_lanczos_multi_f64's caller vectors). */
#define LZX_PROBE_KEEP_BASIS 1
int lzx_probes_f64(lzx_handle h, uint64_t seed, uint64_t first, uint32_t b, double *Z);
int lzx_lanczos_probes_f64(lzx_handle h, uint64_t seed, uint64_t first, uint32_t b, uint32_t k, uint32_t flags,
                           double *alpha, double *beta, uint32_t *k_used, lzx_stats *stats);
int lzx_probe_diag_f64(lzx_handle h, const double *T, uint32_t k, double *out);

/* ---- extreme eigenpairs: thick-restart Lanczos --------------------------------
 * lzx_eigsh_f64: the nev algebraically largest (LZX_EIG_LARGEST) or smallest (LZX_EIG_SMALLEST) eigenpairs of the handle's
 * operator M -- A, or L = D - A under option "operator" = LZX_OP_LAPLACIAN -- by thick-restart Lanczos (Wu-Simon, the
 * symmetric Krylov-Schur) with full re-orthogonalisation (classical Gram-Schmidt twice) on the device.  One GPU handle only.
 *   start     x0 [n] in caller order; NULL: probe 0 of `seed` as lzx_probes_f64 defines it, generated on the device.  The
 *             start vector is orthogonalised against W.
 *   deflation W [nw][n] (nw <= 8, caller order): every basis vector is kept orthogonal to span(W).  The library
 *             orthonormalises W itself (on the device); a rank-deficient W is LZX_ERR_ARG.  Example: W = 1/sqrt(n) under L on
 *             a connected graph makes lambda_2 the smallest wanted eigenvalue.
 *   outputs   evals [nev]: descending for LARGEST, ascending for SMALLEST.  evecs [nev][n] (or NULL): unit vectors in caller
 *             order, each signed so that its entry of largest magnitude (the first such on a tie) is positive.  resid [nev] (or
 *             NULL): the true residual ||M v_i - theta_i v_i||_2, formed on the device with one more SpMV per pair.
 *   converged pair i converges when |beta_m y_{m,i}| <= tol * norm_est, norm_est = the largest |Ritz value| seen (under L at
 *             most 2 d_max).  If max_restarts runs out first, the best nev Ritz pairs are still written, info->converged <
 *             nev, and the call returns LZX_ERR_LIMIT with a message stating the pairs converged and the largest residual
 *             estimate.
 *   limits    1 <= nev, nev + 2 <= m <= 128, m + nw <= n; m = 0 picks max(2 nev + 1, 20) clipped to those limits.
 *             LZX_ERR_ARG: null handle, nev = 0, unknown `which`, tol <= 0, a size rule above.  LZX_ERR_LIMIT: m > 128, nw > 8.
 *             LZX_ERR_STATE: a handle with a communicator, or no graph.  LZX_ERR_NOMEM: the basis, (nw + m + 1) * n_loc_pad * 8
 *             bytes, does not fit (the message states the bytes; nothing of the eigensolver is left behind).
 *   state     like lzx_spmv_f64 the call voids a prepared (chunked) single-vector decomposition: the next
 *             lzx_lanczos_run_steps gets LZX_ERR_STATE.  The resident single-vector basis (lzx_multout_f64 on it) and the batch
 *             state are left alone; the eigensolver's basis is freed before the call returns.
 *   breakdown beta_j <= 2^-40 * g (g = d_max under A, 2 d_max under L) ends a cycle early: its Ritz pairs are exact, and the
 *             next cycle starts from a fresh probe orthogonalised against the basis: the probes of `seed` are taken in order from
 *             index 1, and one that lies in the span of W and the kept columns (three vertices: every second one can) is passed over.
 *             A breakdown at which W and the cycle's columns span all of R^n (m + nw == n) leaves nothing to explore: the
 *             call ends there with the exact pairs.
 *   repeated  a single-vector Krylov method finds one vector per eigenspace from one start vector: further copies of a
 *             repeated eigenvalue appear only through rounding or a breakdown restart.  W is the tool for getting them.
 *   determinism: the same graph, options and arguments give bit-identical evals, evecs, resid and counts.
 * info (or NULL): converged pairs, restarts, Lanczos matvecs (the residual SpMVs not counted), m used; loop_ms (host clock,
 * whole call), spmv_ms and orth_ms (device event time of the SpMVs / of Gram-Schmidt + normalise + rotation launches),
 * host_ms (dense eigenproblems and restart set-up), norm_est. */
#define LZX_EIG_LARGEST  0   /* algebraically largest */
#define LZX_EIG_SMALLEST 1   /* algebraically smallest */
typedef struct lzx_eig_info {
    uint32_t converged, restarts, matvecs, m;   /* m: the subspace size used */
    double   loop_ms, spmv_ms, orth_ms, host_ms;
    double   norm_est;                           /* the ||M|| estimate the tolerance is relative to */
} lzx_eig_info;
int lzx_eigsh_f64(lzx_handle h, uint32_t nev, int which, uint32_t m, double tol, uint32_t max_restarts,
                  const double *x0, uint64_t seed, const double *W, uint32_t nw,
                  double *evals, double *evecs, double *resid, lzx_eig_info *info);

/* ---- shifted linear systems: multi-shift conjugate gradients ------------------------------------------
 * S(sigma_s) x_s = b for s = 1 .. ns (ns <= 16) from ONE Krylov sequence, on the device, with the handle's operator:
 * S(sigma) = sigma I - A (option "operator" = LZX_OP_ADJACENCY, the default; Katz centrality x = (beta / alpha) S(1 / alpha)^(-1) 1)
 * or S(sigma) = sigma I + L (LZX_OP_LAPLACIAN; the regularised Laplacian kernel (I + t L)^(-1) = (1/t) S(1/t)^(-1), and with
 * sigma = 0 and deflation the pseudo-inverse L+ b).  S(sigma) is symmetric positive definite exactly when sigma > lambda_max(A)
 * under A, sigma > 0 under L.  No reference counterpart.
 *   method    plain CG on the seed system, the smallest shift sigma_0 (r_0 = p_0 = b, x = 0); every other shift follows it by the
 *             multi-shift recurrences (Frommer 2003; Jegerlehner): zeta_{j+1} = zeta_j zeta_{j-1} alpha_{j-1} / (alpha_j beta_{j-1}
 *             (zeta_{j-1} - zeta_j) + zeta_{j-1} alpha_{j-1} (1 + (sigma_s - sigma_0) alpha_j)), alpha^s_j = alpha_j zeta_{j+1} / zeta_j,
 *             beta^s_j = (zeta_{j+1} / zeta_j)^2 beta_j.  Shift s's residual is zeta_{s,j} r_j.  One SpMV and two streaming
 *             kernels per iteration; the state is (2 + 2 ns' + nw) vectors of n_loc_pad + 64 doubles (ns' = distinct shifts).
 *   stop      shift s is frozen (its x_s and p_s are no longer written) once |zeta_{s,j}| ||r_j|| <= tol ||b||; the seed's r and p
 *             run on until every shift is frozen or maxiter iterations have run.  The rule is evaluated on the device; the host
 *             reads a small status every 16 iterations (the results do not depend on that period).
 *   W         nw <= 8 deflation vectors (nw x n, caller order; NULL when nw = 0), orthonormalised in order on the device: b is
 *             projected onto span(W)^perp before the solve and every x_s after it.  Under L, sigma_0 = 0 is allowed only with
 *             nw >= 1 (L+ b: W = 1/sqrt(n) on a connected graph, the component indicators otherwise; b must be orthogonal to the
 *             rest of the null space).  ||b|| below is the norm after the projection.
 *   output    X[s * n + i]: x_s in the caller's shift and vertex order (a duplicate shift gets the same vector); iters[s]: the
 *             iteration at which shift s froze (maxiter if it did not); resid[s]: the true relative residual ||b - S(sigma_s) x_s||
 *             / ||b||, formed on the device with one SpMV per distinct shift.
 *   errors    LZX_ERR_ARG: null handle, b or X (or shifts); ns = 0; tol <= 0 or NaN; maxiter = 0; a shift that is not finite or
 *             < 0; sigma_0 <= 0 under A; sigma_0 = 0 under L without W; nw > 0 with W null; W rank-deficient; b zero or in
 *             span(W); and, during the solve, p . S(sigma_0) p <= 0 or not finite (S(sigma_0) is not positive definite: the
 *             message names sigma_0, the iteration and the curvature; nothing is written).  LZX_ERR_LIMIT: ns > 16, nw > 8, or
 *             maxiter reached before every shift converged (X, iters and resid are still written).  LZX_ERR_STATE: a handle
 *             with a communicator (one GPU only), no graph.  LZX_ERR_NOMEM: the state does not fit (the message states the
 *             bytes).  Nothing of the solver is left allocated after any return.
 *   state     like lzx_spmv_f64 the call voids a prepared (chunked) single-vector decomposition; the resident basis, its
 *             alpha / beta and the batch state are left alone.
 *   determinism: identical arguments give identical bits; each x_s does not depend on the order of `shifts` or on
 *             duplicates, and the seed's x has the bits of a call with sigma_0 alone.
 * info (or NULL): iterations (the last freeze; the iterations whose results were used), launched (>= iterations: the status
 * period), converged (caller's shifts that met tol), ns; loop_ms (host clock, whole call), spmv_ms / vec_ms (device event time
 * of the loop's SpMVs / of its vector kernels), bnorm (||b|| after deflation). */
typedef struct lzx_solve_info {
    uint32_t iterations;   /* seed iterations whose results were used (the last freeze) */
    uint32_t launched;     /* iterations launched, >= iterations (poll granularity)     */
    uint32_t converged;    /* shifts that met tol                                       */
    uint32_t ns;
    double   loop_ms, spmv_ms, vec_ms;   /* host clock of the call; device event time of SpMVs / vector kernels */
    double   bnorm;        /* ||b|| after deflation */
} lzx_solve_info;
int lzx_solve_shifted_f64(lzx_handle h, const double *b, uint32_t ns, const double *shifts, double tol, uint32_t maxiter,
                          const double *W, uint32_t nw, double *X, uint32_t *iters, double *resid, lzx_solve_info *info);

/* ---- many right-hand sides: a batch of independent conjugate-gradient solves ---------------------------
 * S(sigma_c) x_c = b_c for c = 1 .. nb (nb <= 16), every column with a right-hand side AND a shift of its own, on the device, with
 * the handle's operator: S(sigma) = sigma I - A or sigma I + L exactly as in lzx_solve_shifted_f64.  Effective resistances for a
 * list of pairs, columns of (I + t L)^(-1) or Katz vectors for a set of seeds, electrical flows for several demands.  One GPU
 * handle only.  No reference counterpart.
 *   method    nb plain CG recurrences (x = 0, r_0 = p_0 = b_c), NOT coupled into a block Krylov space: each column has its own
 *             alpha, beta, stop and failure.  They share one SpMM per iteration over the batched path's layout, [n][B] with the
 *             columns interleaved and B = nb padded to 2, 4, 8 or 16 (padded columns are zero and frozen from the start): col_idx
 *             is read once and one gathered line serves every column.  One SpMM and two streaming kernels per iteration; the
 *             state is b, r, p, x and the batched work vector, (5 B + nw) n doubles, plus three partial arrays of n / 2048 x B.
 *   stop      column c is frozen (its x, r and p are no longer written; no scalar of it is formed any more) once ||r_{c,j}|| <= tol ||b_c||;
 *             iters[c] is the iteration count at the freeze, or maxiter if it never froze.  The rule is evaluated on the device;
 *             the host reads a small status every 16 iterations (the results do not depend on that period).
 *   curvature p_c . S(sigma_c) p_c = sigma_c p.p -+ p.Mp <= 0 or not finite stops THAT column only: status[c] = 2, x_c stays at the
 *             iterate before the failing step (iters[c]: that iteration), the other columns go on.
 *   status[c] 0 = converged, 1 = maxiter reached, 2 = S(sigma_c) is not positive definite.
 *   returns   any column with status 2: LZX_ERR_ARG (the message names the first such column, its sigma, the iteration and the
 *             curvature); otherwise any column with status 1: LZX_ERR_LIMIT.  In both cases X, iters, resid, status and info are
 *             written for every column.
 *   W         nw <= 8 deflation vectors (nw x n, caller order; NULL when nw = 0) shared by all columns, orthonormalised in order
 *             on the device (a column within 1e-10, relative, of the span of those before it: LZX_ERR_ARG).  Every b_c is
 *             projected onto span(W)^perp before the solve and every x_c after it; bnorm and the stop rule use the projected b.
 *             Under L, sigma_c = 0 is allowed only with nw >= 1.
 *   output    Bm[c * n + i] and X[c * n + i]: column c in the caller's vertex order; resid[c]: the true relative residual
 *             ||b_c - S(sigma_c) x_c|| / ||b_c||, formed on the device with one more SpMM over X.
 *   errors    LZX_ERR_ARG: null handle, Bm, shifts or X; nb = 0; tol <= 0 or NaN; maxiter = 0; a shift that is not finite or < 0;
 *             sigma_c <= 0 under A; sigma_c = 0 under L without W; nw > 0 with W null; W rank-deficient; a column b_c that is
 *             zero or lies in span(W) (the message names the column).  LZX_ERR_LIMIT: nb > 16, nw > 8.  LZX_ERR_STATE: a handle
 *             with a communicator, or no graph.  LZX_ERR_NOMEM: the state does not fit (the message states the bytes).  The
 *             checks that need no device come first.  Nothing of the solver is left allocated after any return.
 *   state     like lzx_spmm_f64 the call does NOT void a prepared (chunked) single-vector decomposition and leaves the resident
 *             single-vector basis alone; a resident batch basis stays too (lzx_multout_multi_f64 and lzx_probe_diag_f64 answer
 *             afterwards with the bits they had before).
 *   determinism: identical arguments give identical bits, and x_c, iters[c], resid[c] and bnorm[c] are bit-identical whatever
 *             else is in the batch, whatever c's place in it and whatever nb pads to: every sum has a shape that depends on n
 *             alone (runs of 32 rows left to right, one partial per 2048 rows, a fixed-order close; no floating-point atomics).
 * info (or NULL): iterations (the largest iters[c]), launched (>= iterations: the status period), converged (columns that met
 * tol), nb; loop_ms (host clock, whole call), spmv_ms / vec_ms (device event time of the loop's SpMMs / of its vector kernels);
 * bnorm[c]: ||b_c|| after deflation, caller's column order (0 beyond nb). */
typedef struct lzx_solve_multi_info {
    uint32_t iterations;   /* the last freeze: iterations whose results were used */
    uint32_t launched;     /* >= iterations (status poll period)                   */
    uint32_t converged;    /* columns that met tol                                 */
    uint32_t nb;
    double   loop_ms, spmv_ms, vec_ms;   /* host clock of the call; device event time of SpMMs / vector kernels */
    double   bnorm[16];    /* ||b_c|| after deflation, caller's column order (0 beyond nb) */
} lzx_solve_multi_info;
int lzx_solve_multi_f64(lzx_handle h, uint32_t nb, const double *Bm /* [nb][n] caller order */,
                        const double *shifts /* [nb], one per column */, double tol, uint32_t maxiter,
                        const double *W, uint32_t nw, double *X /* [nb][n] */,
                        uint32_t *iters /* [nb] or NULL */, double *resid /* [nb] or NULL */,
                        uint32_t *status /* [nb] or NULL */, lzx_solve_multi_info *info /* or NULL */);

/* ---- PageRank: multi-shift conjugate gradients in the degree inner product -----------------------------
 * PageRank and personalised PageRank of the handle's (undirected) graph for nd <= 16 damping factors from ONE Krylov sequence,
 * on the device.  With d_i the stored entries of row i (the degree of option "operator" = LZX_OP_LAPLACIAN: a self loop counts
 * once), w_i = max(d_i, 1) and W = diag(w): PageRank with damping delta, teleport vector v (v >= 0, scaled to sum 1) and the
 * dangling mass returned to v -- networkx's default -- is x = y / sum(y) with (I - delta A W^(-1)) y = v.  It always works on A:
 * the handle's "operator" option is ignored (same bits under either value).  One GPU handle only.  No reference counterpart.
 *   method    A W^(-1) = W P W^(-1) with P = D^(-1) A (zero rows where d_i = 0), so y = (1 / delta) W z with (sigma I - P) z = b,
 *             sigma = 1 / delta > 1, b = W^(-1) v.  P is self-adjoint in <a, b>_W = sum w_i a_i b_i and sigma I - P is positive
 *             definite there: CG in that inner product on the seed system, the largest delta; every other delta follows by the
 *             multi-shift recurrences of lzx_solve_shifted_f64.  One SpMV and two streaming kernels per iteration; the state is
 *             2 + 2 nd' vectors of n_loc_pad + 64 doubles (nd' = distinct dampings), plus the handle's degree array (4 bytes per
 *             row, built on the first call that needs it and kept as long as the graph).
 *   stop      damping s is frozen once |zeta_{s,j}| ||r_j||_W <= tol ||b||_W; the rule is evaluated on the device, the host reads a
 *             small status every 16 iterations (the results do not depend on that period).
 *   v         [n] in the caller's order, or NULL: the uniform vector, made on the device (nothing is uploaded).
 *   output    X[s * n + i]: x_s in the caller's damping and vertex order, summing to 1 (the division by sum(y) happens on the
 *             device; a duplicate damping gets the same vector); iters[s] (or NULL): the iteration at which damping s froze
 *             (the iterations launched if it did not); resid[s] (or NULL): the true L1 residual ||v - (I - delta_s A W^(-1)) y_s||_1
 *             / ||v||_1, formed on the device with one SpMV per distinct damping.
 *   errors    LZX_ERR_ARG: null handle, damping or X; nd = 0; a damping that is not finite or not in (0, 1); tol <= 0 or NaN;
 *             maxiter = 0; v with a negative or non-finite entry or with sum 0; a curvature <p, (sigma_0 I - P) p>_W <= 0 during
 *             the solve (the matrix handed over is not symmetric).  LZX_ERR_LIMIT: nd > 16, or maxiter reached before every
 *             damping converged (X, iters and resid are still written).  LZX_ERR_STATE: a handle with a communicator, no graph.
 *             LZX_ERR_NOMEM: the state does not fit (the message states the bytes).  Nothing of the solver is left allocated
 *             after any return.
 *   state     like lzx_spmv_f64 the call voids a prepared (chunked) single-vector decomposition; the resident basis, its
 *             alpha / beta and the batch state are left alone.
 *   determinism: identical arguments give identical bits; each x_s does not depend on the order of `damping` or on duplicates.
 * info (or NULL): iterations (the last freeze), launched (>= iterations: the status period), converged (caller's dampings that
 * met tol), nd; loop_ms (host clock, whole call), spmv_ms / vec_ms (device event time of the loop's SpMVs / of its vector
 * kernels); mass[s]: sum of the unnormalised y_s in the caller's damping order (0 beyond nd). */
typedef struct lzx_pagerank_info {
    uint32_t iterations, launched, converged, nd;
    double   loop_ms, spmv_ms, vec_ms;
    double   mass[16];   /* sum of the unnormalised y_s, caller's damping order */
} lzx_pagerank_info;
int lzx_pagerank_f64(lzx_handle h, const double *v /* [n] caller order, or NULL = uniform */,
                     uint32_t nd, const double *damping, double tol, uint32_t maxiter,
                     double *X /* [nd][n] */, uint32_t *iters, double *resid, lzx_pagerank_info *info);

/* ---- connected components and induced subgraphs --------------------------------------------------------
 * Everything above treats the graph as one piece; R-MAT graphs are not (tests/golden/rmat_n4096: 1 204 components, 1 200 of them
 * single vertices), and under L every component adds a copy of the eigenvalue 0.  These two calls name the pieces and hand a
 * handle one of them, on the device, from the caller-order CSR the handle keeps.  One GPU handle only.  No reference counterpart.
 *
 * lzx_components: labels[i] (or NULL: counts only, no n-vector crosses PCIe) = the smallest vertex id of i's component, in the
 * caller's order -- canonical: any correct algorithm gives these bits.  A self loop changes nothing; a vertex without an edge
 * labels itself and counts as a component of size 1.
 *   method    min-label hooking with pointer jumping (FastSV's two hookings): parents f (f[v] = v at the start), grandparents
 *             gf = f[f].  A round is one pull sweep over the CSR -- row u takes m = min(gf[u], gf of its neighbours), then u and
 *             its parent f[u] are lowered to m in the next parent array (32-bit vector atomicMin, at most two per row and only
 *             where they lower something) -- followed by f = next, gf = f[f].  A sweep reads f and gf only and writes by
 *             minimum, so the labels AND the number of rounds are the same in every run.  The host reads one word per round;
 *             the round that lowers nothing is the last (and is counted).  More than n + 1 rounds: LZX_ERR_LIMIT (cannot
 *             happen on a symmetric matrix).
 *   info      (or NULL) n_components, largest_size and largest_label are formed on the device: roots (label == id) counted with
 *             the fixed-shape block reduction, sizes in a u32 histogram on the roots, the largest by size then smallest label.
 *   state     the call touches none: it neither voids a prepared or chunked decomposition nor touches the resident bases or the
 *             batch state, and what it allocates (16 n bytes and a few KiB) is freed before it returns.
 *   errors    LZX_ERR_ARG: null handle.  LZX_ERR_STATE: no graph, a handle with a communicator, a graph from a sharded hand-over
 *             over several ranks (where lzx_get_graph_csr refuses too).  LZX_ERR_NOMEM: the message states the bytes.
 *
 * lzx_set_graph_induced: dst receives the subgraph of src's graph induced by the vertices with keep[i] != 0 (keep: [n of src]),
 * renumbered in ascending old id; old_of_new[j] (or NULL; [n_new]) = the old id of new vertex j, *n_new (or NULL) their number.
 * dst == src replaces the graph in place; two different handles must be on the same GPU.  Only the mask crosses PCIe: the new
 * ids are a scan of the mask, the kept neighbours of every kept row are counted, the counts scanned into row pointers and the
 * columns written under their new ids -- the map is monotone, so they stay ascending -- and the result is handed to the same
 * reshaping every hand-over ends in, under dst's options.  Afterwards dst is in exactly the state lzx_set_graph_csr of that CSR
 * would have left it in: same status (degenerate subgraphs included), same lzx_get_graph_csr and lzx_get_graph_info, same bits
 * out of every later call.  (With dst's option "sharded_ingest" set the subgraph IS handed to lzx_set_graph_csr through host
 * memory, which that option streams from.)
 *   errors    LZX_ERR_ARG: null dst, src or keep; nothing kept; handles on different GPUs (the message names both devices).
 *             LZX_ERR_STATE: either handle with a communicator, src without a graph or without a whole caller-order CSR.
 *             After any of these, and after a failed allocation while the subgraph is built, dst keeps the graph it had; a
 *             failure of the reshaping itself leaves dst as the same failure of lzx_set_graph_csr would. */
typedef struct lzx_components_info {
    uint64_t n_components;     /* isolated vertices count as components of size 1 */
    uint64_t largest_size;     /* vertices of the largest component */
    uint32_t largest_label;    /* its label; ties: the smallest label */
    uint32_t rounds;           /* sweeps over the edges until nothing changed */
    double   loop_ms;          /* host clock, whole call */
    double   sweep_ms;         /* device event time of the edge sweeps alone */
} lzx_components_info;
int lzx_components(lzx_handle h, uint32_t *labels /* [n], caller order */, lzx_components_info *info /* or NULL */);
int lzx_set_graph_induced(lzx_handle dst, lzx_handle src, const uint8_t *keep /* [n of src], non-zero = keep */,
                          uint32_t *old_of_new /* [n_new] or NULL */, uint64_t *n_new /* or NULL */);

/* ---- path-based centralities: batched breadth-first search and betweenness ------------------------------
 * Everything above is spectral; these two calls serve the centralities defined by shortest paths of the unweighted, undirected
 * graph -- BFS distances from a set of seeds, closeness, harmonic centrality, betweenness -- on the device, from the caller-order
 * CSR the handle keeps.  One GPU handle only.  No reference counterpart.
 *
 * lzx_bfs_multi: a breadth-first search from every one of the ns sources (caller's vertex order; ns is not limited: the list
 * is cut into batches of 16 in the caller's order; a source may appear more than once).  Per source s: dist[s][v] = the number
 * of edges of a shortest path (-1: v is not reachable), paths[s][v] = the number of shortest paths (0 where unreachable, 1 at the
 * source), reached[s] = vertices reached, the source included, sum_dist[s] = the sum of the distances to them, harmonic[s] = the
 * sum over the reached v != s of 1 / dist, ecc[s] = the largest distance.  Every output may be NULL; only those asked for cross
 * PCIe.  A self loop changes nothing; a source without an edge reaches itself only.
 *
 * lzx_betweenness_f64: bc[v] = the sum over the sources s of Brandes' dependency delta_s(v), v != s -- the raw sum: no 1/2 for
 * undirectedness, no normalisation, no endpoints (sources == NULL: every vertex is a source, ns must equal n; the result is then
 * twice networkx's unnormalised betweenness).  A source listed twice counts twice.
 *
 *   method    pull form, up to 16 sources per sweep over the edges.  Per batch the state is dist (i32), sigma (f64) and g (f64),
 *             each [n][B] with B = the batch width padded to 2, 4, 8 or 16, plus one bc[n]: 20 B n + 8 n bytes.
 *             Forward, level d = 1, 2, ...: every (vertex v, column c) with dist = -1 forms s = the sum of sigma[u][c] over
 *             its neighbours u, in ascending column order, with dist[u][c] = d - 1; s > 0 sets dist = d, sigma = s -- in place:
 *             a reader tests "= d - 1", a writer stores d.  The newly reached are counted per column with integer atomics (one
 *             per wavefront and column); the host reads those B words per level, stops when none grew, and forms reached,
 *             sum_dist, harmonic (added in ascending d as count / (double)d) and ecc from them: exact functions of the level
 *             histogram.
 *             Backward (betweenness), level d = L ... 1 with g[w][c] = (1 + delta[w][c]) / sigma[w][c]: every (u, c) with
 *             dist = d forms s = the sum of g[w][c] over its neighbours with dist[w][c] = d + 1, then delta = sigma * s and
 *             g = (1 + delta) / sigma (the deepest level finds s = 0: delta = 0, g = 1 / sigma) -- networkx's
 *             coeff = (1 + delta[w]) / sigma[w]; delta[v] += sigma[v] * coeff with sigma factored out of the sum.  Then
 *             bc[v] += delta[v][c] one column after the other in ascending c, batch after batch.
 *             Both passes are one kernel shape, a masked SpMM over the batched path's work list (whole rows, and chunks of
 *             longer rows whose totals are added in chunk order); a (row, column) whose own level fails the pass's condition
 *             skips its gather.  No floating-point atomics.
 *   bits      identical arguments give identical bits.  dist, paths, reached, sum_dist, harmonic and ecc of a source are the
 *             same bits whatever else is in the call and wherever the source stands in it.  bc of a call with sources
 *             (s_1 ... s_m) equals, bit for bit, ((bc(s_1) + bc(s_2)) + ...) of m single-source calls added left to right.
 *   paths     exact while every count stays below 2^53; beyond that a rounded double, as in networkx (which keeps sigma as a
 *             float too).  Not guarded.
 *   cost      a forward level is one sweep over every entry of the rows still unreached, a backward level gathers only the
 *             rows on that level: O(L nnz) per batch forward, one more forward sweep (the one that finds nothing) than levels.
 *   state     the calls touch nothing of the handle's other state: they void no prepared or chunked decomposition and leave the
 *             resident single-vector basis and the batch basis answering with the bits they had.  The exception is the batched
 *             path's per-graph work list, which is built on first use and kept, as lzx_spmm_f64 does.  Everything else they
 *             allocate is freed before they return, on every path.
 *   info      (or NULL) sources and batches, the largest eccentricity among the sources, the edge sweeps launched (forward and
 *             backward, over all batches), the host clock of the call and the device event time of the sweeps alone.
 *   errors    LZX_ERR_ARG: null handle, ns == 0, null sources (lzx_bfs_multi), null sources with ns != n or null bc
 *             (lzx_betweenness_f64), a source >= n (the message names its index and value).  LZX_ERR_STATE: no graph, a handle
 *             with a communicator, a graph from a sharded hand-over over several ranks.  LZX_ERR_NOMEM: the message states the
 *             bytes.  The checks that need no device come first.
 *   limits    one GPU handle; unweighted, undirected graphs; no push / direction-optimising
 *             search (a small frontier still costs a sweep over the unreached rows).
 *
 * lzx_brandes_f64: the same Brandes pass with its two other outputs, networkx's edge_betweenness_centrality and
 * betweenness_centrality(endpoints=True).  bc and ebc may each be NULL, not both.
 *   ebc       one value per stored entry of the caller-order CSR, in the positions of lzx_get_graph_csr's col_idx.  For the entry
 *             e = (u, w): ebc[e] = the sum over the sources s, in the caller's order, of c_s(u, w), with
 *             c_s(u, w) = sigma_s[u] * g_s[w] if dist_s[u] >= 0 and dist_s[w] = dist_s[u] + 1, sigma_s[w] * g_s[u] if
 *             dist_s[w] >= 0 and dist_s[u] = dist_s[w] + 1, and +0 otherwise (an edge inside one level, an unreached endpoint, a
 *             diagonal entry); g = (1 + delta) / sigma as above.  Each non-zero term is one rounded product, networkx's
 *             c = sigma[v] * coeff.  Raw: no 1/2, no normalisation; with every vertex a source it is twice networkx's
 *             unnormalised edge betweenness.  Both copies of an edge carry the same bits (they form the same product), a diagonal
 *             entry carries 0, a source listed twice counts twice.
 *   bc        flags = 0: lzx_betweenness_f64's bc, bit for bit, whether ebc is asked for or not.  With LZX_BRANDES_ENDPOINTS:
 *             bc[v] = bc_plain[v] + (double)cnt[v], one addition after the last batch, where the 64-bit integer cnt[v] counts, on
 *             the device, + 1 for every source s != v that reaches v (networkx's delta[w] + 1) and + reached_s - 1 every time v is
 *             itself a source (networkx's betweenness[s] += len(S) - 1).  The flag does not change ebc.
 *   method    the forward pass of lzx_betweenness_f64.  When ebc is wanted the backward pass keeps sigma: g goes to the third
 *             [n][B] array as above, delta to a fourth one, and only when bc is wanted too (without ebc the call runs
 *             lzx_betweenness_f64's kernels).  After the last backward level of a batch one edge pass walks the caller-order rows,
 *             4 .. 32 lanes per row by the rule of the other graph routines (G lanes; a row of more than 64 G entries gets a whole
 *             workgroup); every stored entry belongs to one lane, which does
 *             x = ebc[e]; x += c_c(u, w) for the columns c = 0, 1, ... of the batch in ascending order; ebc[e] = x.  The lane
 *             keeps its row's dist / sigma / g in registers, reads the neighbour's dist line, and fetches a sigma or g word of the
 *             neighbour only for a column that meets one of the two conditions.  g of a source (level 0 has no sweep) and of an
 *             unreached vertex is never formed and never read: the dist tests stand in front of every read.  No floating-point
 *             atomic, no search for the mirror entry.
 *   bits      identical arguments give identical bits, for every number of lanes per row.  ebc of a call with sources
 *             (s_1 ... s_m) equals, bit for bit, ((ebc(s_1) + ebc(s_2)) + ...) of m single-source calls added left to right,
 *             wherever the batch boundaries fall: bc's contract.
 *   state     as lzx_betweenness_f64: nothing of the handle's other state is voided or changed; only the batched path's work list
 *             may be added.  The call's arena holds lzx_betweenness_f64's bytes (dist, sigma, g, the split rows' totals, and
 *             bc[n] when bc is wanted), + 8 B n for delta when bc and ebc are both wanted, + 8 nnz for ebc (zeroed at the start),
 *             + 8 n for cnt with the flag: one allocation under the cap of the test shape bfs_state_bytes, freed on every path.
 *   info      (or NULL) as lzx_bfs_info, and edge_ms: the device event time of the per-batch edge passes alone (sweeps does not
 *             count them).
 *   errors    LZX_ERR_ARG: null handle, ns == 0, bc and ebc both NULL, an unknown flag bit, LZX_BRANDES_ENDPOINTS with null bc,
 *             null sources with ns != n, a source >= n (the message names its index and value).  LZX_ERR_STATE and LZX_ERR_NOMEM
 *             as for lzx_betweenness_f64.  The checks that need no device come first.
 *   limits    as above; both triangles of ebc are always returned. */
typedef struct lzx_bfs_info {
    uint32_t ns, batches;      /* sources, batches of <= 16 */
    uint32_t max_level;        /* largest eccentricity among the sources */
    uint32_t sweeps;           /* edge sweeps launched, forward + backward, over all batches */
    double   loop_ms, sweep_ms;/* host clock of the call; device event time of the sweeps alone */
} lzx_bfs_info;
int lzx_bfs_multi(lzx_handle h, uint32_t ns, const uint32_t *sources,
                  int32_t *dist /* [ns][n] or NULL; -1 = not reachable */,
                  double *paths /* [ns][n] or NULL: number of shortest paths from the source (0 where unreachable) */,
                  uint64_t *reached /* [ns] or NULL: vertices reached, the source included */,
                  uint64_t *sum_dist /* [ns] or NULL */, double *harmonic /* [ns] or NULL: sum over reached v != s of 1/d(s,v) */,
                  uint32_t *ecc /* [ns] or NULL */, lzx_bfs_info *info /* or NULL */);
int lzx_betweenness_f64(lzx_handle h, uint32_t ns, const uint32_t *sources /* NULL: every vertex, ns must equal n */,
                        double *bc /* [n], caller order: sum over the sources s of Brandes' dependency delta_s(v), v != s */,
                        lzx_bfs_info *info /* or NULL */);
#define LZX_BRANDES_ENDPOINTS 1
typedef struct lzx_brandes_info {
    uint32_t ns, batches;      /* as lzx_bfs_info */
    uint32_t max_level;
    uint32_t sweeps;
    double   loop_ms, sweep_ms;
    double   edge_ms;          /* device event time of the per-batch edge passes alone */
} lzx_brandes_info;
int lzx_brandes_f64(lzx_handle h, uint32_t ns, const uint32_t *sources /* NULL: every vertex, ns must equal n */,
                    uint32_t flags /* 0 or LZX_BRANDES_ENDPOINTS */, double *bc /* [n] or NULL */,
                    double *ebc /* [nnz] or NULL: one value per stored entry of lzx_get_graph_csr's col_idx */,
                    lzx_brandes_info *info /* or NULL */);

/* ---- triangles and clustering ---------------------------------------------------------------------
 * lzx_triangles: the local structure of the handle's graph read as undirected and unweighted -- what networkx.triangles,
 * clustering, transitivity and average_clustering return -- counted on the device over the caller-order CSR.
 *   outputs   t_v = the number of triangles through v: tri[v] = t_v, caller order.  d_v = the number of stored entries of row v
 *             NOT counting a diagonal entry (networkx removes v from its own neighbourhood).
 *             clustering[v] = (double)(2 t_v) / (double)(d_v (d_v - 1)), and exactly 0.0 where d_v < 2 or t_v = 0: networkx's
 *             expression, one correctly rounded fp64 division of two integers, so these are networkx's bits while
 *             2 t_v < 2^53.  A self loop changes nothing in any output.  Every output may be NULL; only those asked for cross
 *             PCIe.
 *   info      (or NULL) triangles = T, every triangle of the graph counted once (sum t_v / 3); wedges = sum over v of
 *             d_v (d_v - 1) / 2 (<= d_max nnz / 2 < 2^63: not guarded), so that transitivity = 3 T / wedges; max_triangles =
 *             the largest t_v; avg_clustering = (1/n) sum c_v over EVERY vertex (networkx count_zeros=True), summed on the
 *             device in a fixed order; the entries and the longest list of the oriented copy (below); the host clock of the
 *             call, the device event time of building the oriented copy and of the counting launches.
 *   method    vertices are ranked by (d_v, v) and every edge that is not a self loop is kept once, pointing from its lower to
 *             its higher rank: an oriented CSR (64-bit row pointers) built by three launches and one exclusive scan -- degrees
 *             without the diagonal; out-counts, scanned into the row pointers; the fill, a monotone filter of an ascending row,
 *             so columns stay ascending by id.  A vertex of out-degree k has k neighbours of degree >= k, hence k^2 <= nnz:
 *             every oriented list has fewer than 2^16 entries while nnz < 2^32.  A triangle of ranks a < b < c is found
 *             exactly once, as c in N+(a) n N+(b) while row a handles its out-edge a -> b: the shorter of the two lists is
 *             walked and the longer binary-searched.  A hit adds 1 to t_c; per out-edge the hits are added to t_b in one add
 *             when non-zero; per row their total is added to t_a in one add.  Rows of at most 128 out-entries are counted a
 *             group of lanes per row (4 to 32, from the mean oriented degree); longer rows a workgroup per row and slice of
 *             its out-edges, a wavefront per out-edge, with N+(a) staged in LDS while it has at most 4096 entries (then the
 *             hits on c are first counted in LDS and leave with one add per entry) and read where it lies beyond that.  All adds
 *             are 64-bit INTEGER vector atomics (32-bit in LDS); there is no floating-point atomic anywhere.  No kernel waits
 *             on another workgroup and every loop is bounded by a list length.
 *   bits      identical arguments give identical bits.  tri, clustering, triangles, wedges and max_triangles are canonical:
 *             any correct algorithm gives them, and they do not depend on how ties in the ranking fall.
 *   state     the call touches none: it voids no prepared or chunked decomposition and leaves the resident bases and the batch
 *             state alone.  Everything it allocates is freed before it returns, on every path: the oriented CSR
 *             8 (n + 1) + 4 oriented_entries bytes (the columns are allocated once the scan has counted them), 4 n of
 *             degrees, 8 n of counts, 8 n of coefficients, a few KiB of partials and the scan's scratch.
 *   errors    LZX_ERR_ARG: null handle.  LZX_ERR_STATE: no graph, a handle with a communicator, a graph from a sharded
 *             hand-over.  LZX_ERR_NOMEM: the message states the bytes.  The checks that need no device come first.
 *   limits    one GPU handle; undirected, unweighted graphs; no sampling estimator (the triangles per EDGE and the k-truss
 *             are lzx_truss, below).  A matrix that is not symmetric is not detected: the call stays within its memory (the columns are
 *             sized by the count the fill repeats) and its counts mean nothing. */
typedef struct lzx_triangles_info {
    uint64_t triangles;        /* T: triangles of the graph, each counted once */
    uint64_t wedges;           /* sum over v of d_v (d_v - 1) / 2 */
    uint64_t max_triangles;    /* largest t_v */
    uint64_t oriented_entries; /* entries of the oriented copy = edges that are not self loops */
    uint32_t oriented_max_degree, reserved_;
    double   avg_clustering;   /* (1/n) sum c_v, every vertex counted (networkx count_zeros=True) */
    double   loop_ms, orient_ms, count_ms;  /* host clock of the call; device event time of building the oriented copy / of the counting launches */
} lzx_triangles_info;
int lzx_triangles(lzx_handle h, uint64_t *tri /* [n] or NULL */, double *clustering /* [n] or NULL */,
                  lzx_triangles_info *info /* or NULL */);

/* ---- core numbers and onion layers ------------------------------------------------------------------
 * lzx_core_numbers: the k-core decomposition of the handle's graph read as undirected and unweighted -- what
 * networkx.core_number and networkx.onion_layers return -- peeled on the device over the caller-order CSR.
 *   outputs   d_v = the number of stored entries of row v NOT counting a diagonal entry: a self loop changes nothing in any
 *             output (networkx raises on a graph with self loops; compare with the loops removed).  Rounds are numbered from
 *             1 and k_0 = 0.  Round r has k_r = max(k_{r-1}, the smallest remaining degree among the remaining vertices) and
 *             removes, all at once, every remaining vertex whose remaining degree is <= k_r; each of them gets core[v] = k_r
 *             (networkx.core_number) and layer[v] = r (networkx.onion_layers), caller order.  An isolated vertex has core 0 and
 *             layer 1.  Every output may be NULL; only those asked for cross PCIe.
 *   info      (or NULL) degeneracy = the largest core number = the last k; main_core_size = the vertices whose core number is
 *             the degeneracy; core0 = the vertices of core number 0 (no neighbour other than themselves); levels = the distinct
 *             core numbers that occur; rounds = the peeling rounds = the largest layer; the host clock of the call and the
 *             device event time of the peeling loop (one event pair around it, the host's reads included).  The host forms the
 *             integers from the boundaries of the queue's windows.
 *   method    push peeling, O(nnz) edge work in all.  State: the remaining degrees, the layers (0 = not yet removed: the mark),
 *             the core numbers and one queue, u32 [n] each.  Every vertex is appended to the queue exactly once over the whole
 *             call, so each round's frontier is a window of it, and what a launch appends behind the window is the next one.
 *             When the frontier is empty a level starts: one thread per vertex, an unmarked vertex of remaining degree <= k is
 *             marked and appended and the others contribute to a minimum; the host tries k + 1 first and, only if that
 *             appends nothing, repeats the sweep with the minimum.  A round is one peel of its window: a group of lanes per row
 *             (4 to 32, from the mean degree), rows of more than 64 times that many entries in a second launch, a workgroup per
 *             row and slice of its entries; for every neighbour u != v that is not marked, old = atomicSub(&deg[u], 1), and the
 *             one lane that sees old == k + 1 marks u (layer r + 1, core k) and appends it.  Appends and the minimum are
 *             aggregated per wavefront: a ballot, then one atomic per wavefront.  The mark test saves traffic only: a decrement
 *             of a removed vertex can never return k + 1, and on a symmetric matrix no counter goes below 0.  All atomics are
 *             32-bit INTEGER vector atomics; there is no floating-point anywhere.  No kernel waits on another workgroup, every
 *             device loop is bounded by a row length or a window length, every append is clamped to the queue's n entries.
 *             The host reads one word per round (the queue's end) and two per level start, and stops when n vertices are
 *             queued; the last window is not peeled (nobody is left to push to).
 *   bits      core, layer and every integer of info are canonical: any correct algorithm gives them.  The order inside a
 *             window is not deterministic and is no output.
 *   state     the call touches none: it voids no prepared or chunked decomposition and leaves the resident bases and the batch
 *             state alone.  Everything it allocates (16 n bytes and two words) is freed before it returns, on every path.
 *   errors    LZX_ERR_ARG: null handle.  LZX_ERR_STATE: no graph, a handle with a communicator, a graph from a sharded
 *             hand-over.  LZX_ERR_NOMEM: the message states the bytes.  LZX_ERR_LIMIT: more than n + 1 rounds (cannot happen).
 *             The checks that need no device come first.
 *   limits    one GPU handle; undirected, unweighted graphs; no degeneracy ordering (the order inside a round is not
 *             deterministic); cohesion by triangles instead of degrees -- per-edge support, the k-truss -- is lzx_truss, below.  A matrix that is not symmetric is not detected: its numbers mean
 *             nothing, but the call stays within its memory and ends -- the mark is taken by a compare-and-swap, so no vertex
 *             is queued twice even where a counter wraps. */
typedef struct lzx_core_info {
    uint64_t main_core_size;  /* vertices whose core number equals the degeneracy */
    uint64_t core0;           /* vertices of core number 0 (no neighbour other than themselves) */
    uint32_t degeneracy;      /* the largest core number */
    uint32_t levels;          /* distinct core numbers that occur */
    uint32_t rounds;          /* peeling rounds = the largest onion layer */
    uint32_t reserved_;
    double   loop_ms, peel_ms;/* host clock of the call; device event time of the peeling launches */
} lzx_core_info;
int lzx_core_numbers(lzx_handle h, uint32_t *core /* [n] or NULL */, uint32_t *layer /* [n] or NULL */,
                     lzx_core_info *info /* or NULL */);

/* ---- edge support and truss numbers -------------------------------------------------------------------
 * lzx_truss: the truss decomposition of the handle's graph read as undirected and unweighted -- the edge sets networkx.k_truss
 * returns, for every k at once -- peeled on the device over the caller-order CSR.
 *   outputs   support(e) = the number of triangles through the undirected edge e.  A self loop is no edge and closes no
 *             triangle: it changes nothing in any output.  Rounds are numbered from 1 and k_0 = 2.  Round r has
 *             k_r = max(k_{r-1}, 2 + the smallest remaining support among the remaining edges) and removes, all at once, every
 *             remaining edge whose remaining support is <= k_r - 2, where the remaining support counts the triangles whose
 *             three edges all remain; each removed edge gets truss = k_r and layer = r.  So every edge has truss >= 2, and
 *             {e : truss(e) >= k} is the edge set of networkx.k_truss(G, k).
 *             support, truss and layer are PER STORED ENTRY of the caller-order CSR: entry e of lzx_get_graph_csr's col_idx gets
 *             the value of its undirected edge, so both copies of an edge carry the same number and (truss, col_idx, row_ptr)
 *             is the truss matrix; a diagonal entry gets 0 in all three.  vertex_truss[v] = the largest truss number among
 *             v's edges, 0 where v has no edge other than a loop.  Every output may be NULL; only those asked for cross PCIe.
 *             On a graph without an edge every per-entry output is 0, max_truss = 0 and rounds = levels = 0.
 *   info      (or NULL) edges = m, the undirected edges that are not self loops; triangles = T = sum of the supports / 3;
 *             max_support; max_truss = the last k; main_truss_edges = the edges whose truss number is max_truss; levels = the
 *             distinct truss numbers that occur; rounds = the peeling rounds = the largest layer; the host clock of the call,
 *             the device event time from the first launch to the end of the support count (orientation, edge ids, support)
 *             and of the peeling loop (the host's reads included).  The host forms the integers from the boundaries of the
 *             queue's windows and from block partials of the supports' sum and maximum.
 *   method    (1) lzx_triangles' oriented copy: every edge once, in the row of its lower end by (d_v, v).  The EDGE ID of an edge
 *             is its position in the oriented columns, m < 2^32 - 1 ids (more is LZX_ERR_LIMIT); src[e] is its oriented row.
 *             (2) eid[entry], u32 [nnz] over the caller-order CSR: entry (u, v) binary-searches its higher-ranked end in the
 *             oriented row of its lower-ranked end; a diagonal entry, and an entry whose search fails (only on a matrix that
 *             is not symmetric), gets 0xffffffff, and every later use range-checks what it reads.  (3) Support: lzx_triangles'
 *             counting walk, the same split at a list of more than 128 out-entries and the same LDS staging, with u32 counters
 *             per edge: at a hit the walked index and the search result are the positions of the two far edges, one add each;
 *             the out-edge gets its hits in one add.  (4) Push peeling over one queue of edge ids.  State, u32 [m] each: sup,
 *             mark (0 = not yet removed, else the layer), truss, queue; every edge is appended exactly once, a round's
 *             frontier is a window of the queue.  When the window is empty a level starts: one thread per edge, an unmarked
 *             edge with sup <= s (s = k - 2) is marked and appended, the others contribute to a minimum; the host tries s + 1
 *             first and sweeps again with the minimum only if nothing was appended.  A round peels its window: for a frontier
 *             edge e1 = (u, v) the FULL rows of u and v are intersected (the shorter walked, the longer searched; w = u and
 *             w = v skipped), a common neighbour w gives e2 = eid[w in row u], e3 = eid[w in row v].  The triangle is dead if
 *             mark[e2] or mark[e3] is non-zero and < r.  Otherwise: both in the window (mark == r): nothing; exactly one in
 *             the window, say e2: e3 is decremented only if e1 < e2 (edge ids); neither: both are decremented -- every dying
 *             triangle takes exactly one from each of its edges that stays.  A decrement is old = atomicSub(&sup[x], 1); the one
 *             lane that sees old == s + 1 takes the mark by atomicCAS(&mark[x], 0, r + 1), writes truss[x] = s + 2 and appends
 *             x.  A mark of 0 and one of r + 1 decide alike and marks equal to r were written by the previous launch, so every
 *             run marks the same edges in the same round.  A group of lanes (4 to 32, from the mean degree) handles each
 *             frontier edge; edges whose SHORTER row has more than 64 times that many entries go to a second launch, a
 *             workgroup per edge and slice, which runs only when the graph has such a row.  Appends and the minimum are
 *             aggregated per wavefront.  The host reads one word per round and two per level start and stops when m edges are
 *             queued; the last window is not peeled.  (5) One gather through eid per requested per-entry output, one row pass
 *             for vertex_truss.  All atomics are 32-bit INTEGER vector atomics, in global memory and in LDS; there is no
 *             floating point anywhere.  No kernel waits on another workgroup; every device loop is bounded by a row, list or
 *             window length; every append is clamped to the queue's m entries.
 *   bits      every output and every integer of info is canonical: any correct algorithm gives these bits.  The order inside
 *             a window is not deterministic and is no output.
 *   state     the call touches none: it voids no prepared or chunked decomposition and leaves the resident bases and the batch
 *             state alone.  Everything it allocates is freed before it returns, on every path: for the vertices
 *             8 (n + 1) + 4 n bytes, 16 KiB of partials and four words (12 n, roughly); then, once the scan has counted m,
 *             24 m (oriented columns, src, sup, mark, truss, queue) + 4 nnz (eid) + 4 nnz (one staging buffer for the
 *             per-entry outputs) -- in all 8 (n + 1) + 4 n + 16400 + 24 m + 8 nnz bytes -- and the scan's scratch.
 *   errors    LZX_ERR_ARG: null handle.  LZX_ERR_STATE: no graph, a handle with a communicator, a graph from a sharded
 *             hand-over.  LZX_ERR_NOMEM: the message states the bytes.  LZX_ERR_LIMIT: 2^32 - 1 edges or more; more than m + 1
 *             rounds (cannot happen on a symmetric matrix).  The checks that need no device come first.
 *   limits    one GPU handle; undirected, unweighted graphs; no triangle listing, no truss hierarchy (connected components of
 *             each k-truss).  A matrix that is not symmetric is not detected: its numbers mean nothing, but the call returns,
 *             stays within its memory and leaves the handle answering -- the mark is taken by a compare-and-swap, so no edge is
 *             queued twice even where a counter wraps. */
typedef struct lzx_truss_info {
    uint64_t edges;            /* m: undirected edges that are not self loops */
    uint64_t triangles;        /* T = sum of the supports / 3 */
    uint64_t main_truss_edges; /* edges whose truss number is max_truss */
    uint32_t max_support, max_truss;
    uint32_t levels;           /* distinct truss numbers that occur */
    uint32_t rounds;           /* peeling rounds = the largest layer */
    double   loop_ms, support_ms, peel_ms;  /* host clock of the call; device event time up to the end of the support count / of the peeling loop */
} lzx_truss_info;
int lzx_truss(lzx_handle h, uint32_t *support /* [nnz] or NULL */, uint32_t *truss /* [nnz] or NULL */,
              uint32_t *layer /* [nnz] or NULL */, uint32_t *vertex_truss /* [n] or NULL */,
              lzx_truss_info *info /* or NULL */);

/* ---- similarity of two vertices: common neighbours, Jaccard, Adamic-Adar ---------------------------------
 * lzx_similarity: how alike two vertices of the handle's graph are, read as undirected and unweighted -- what the functions of
 * networkx.link_prediction return (common_neighbors, jaccard_coefficient, adamic_adar_index, resource_allocation_index) and the
 * overlap and Sorensen coefficients next to them -- for a list of pairs or for every stored entry, on the device over the
 * caller-order CSR.
 *   outputs   N(x) = row x without a diagonal entry, d_x = |N(x)|, c = |N(u) n N(v)|: with u != v exactly
 *             len(networkx.common_neighbors(G, u, v)) of the graph without self loops.  A self loop changes nothing in any
 *             output.  common[p] = c, deg_u[p] = d_u, deg_v[p] = d_v.  values is [popcount(measures)][np], one row of np
 *             doubles per flag of `measures`, in ascending order of the flags' bits:
 *               LZX_SIM_JACCARD              c / (d_u + d_v - c), exactly 0.0 where the denominator is 0 (networkx's rule)
 *               LZX_SIM_OVERLAP              c / min(d_u, d_v), 0.0 where the minimum is 0
 *               LZX_SIM_SORENSEN             2 c / (d_u + d_v), 0.0 where the sum is 0
 *               LZX_SIM_ADAMIC_ADAR          sum over w in N(u) n N(v) of 1 / log d_w
 *               LZX_SIM_RESOURCE_ALLOCATION  sum over w in N(u) n N(v) of 1 / d_w
 *             The first three are one correctly rounded fp64 division of two integers: networkx's bits.  A common neighbour of
 *             two distinct vertices has d_w >= 2, so no term of the two sums is infinite; a sum over no term is exactly 0.0.
 *             Every output may be NULL (values only with measures == 0); only those asked for cross PCIe.
 *             PAIRS MODE (u and v given): np pairs (u[p], v[p]).  (u, v) and (v, u) give the same bits, and a pair's outputs
 *             depend neither on what else is in the batch nor on its position in it.
 *             EDGES MODE (u == v == NULL, np must equal nnz): one output per stored entry of lzx_get_graph_csr's col_idx, laid out
 *             as lzx_truss lays out its vectors: entry e of row r gets the pair (r, col_idx[e]).  Both copies of an edge carry
 *             identical bits -- the bits pairs mode gives that pair --, a diagonal entry carries 0 everywhere (deg_u and deg_v
 *             included).  Each undirected edge is intersected once, from the entry with u < v; the mirror entry finds it by a
 *             binary search of u in row v (and carries 0 where a matrix that is not symmetric has none).
 *   info      (or NULL) pairs = np; walked = the sum of min(|row u|, |row v|), stored lengths, over the pairs intersected (in
 *             edges mode every edge once); max_common = the largest c; short_pairs, long_pairs, sliced_pairs = the pairs
 *             intersected on each of the three paths below (in edges mode they add up to the edges, not to np); lanes = the
 *             lanes per short pair; the host clock of the call, the device event time of the preparation (degrees, tables,
 *             the pair list of edges mode) and of everything from the classification to the last launch (the host's one read
 *             in between included).
 *   method    (1) Preparation: d_v by one thread per row (lzx_triangles' degree kernel) and, only for a sum that is asked for, one
 *             fp64 table per sum: 1 / log d_v (0 where d_v < 2) and 1 / d_v (0 where d_v < 1).  A hit then costs one 8-byte
 *             gather and no log runs in the walk.  (2) The walk: the shorter of the two stored rows is walked -- on a tie in
 *             length the row of the smaller id, so both orders of a pair take the same path -- and the longer binary-searched;
 *             u and v themselves are skipped; a lane's entries ascend, so each search starts at the place the previous one
 *             ended.  (3) Three paths by s = the walked row's stored length.  SHORT, s <= 64 G: a group of G lanes per pair (4 to
 *             32, from the graph's mean degree), lane i takes the entries i, i + G, ...  LONG, s above that: one workgroup of 256
 *             per pair, thread i takes i, i + 256, ...  SLICED, s also above 16384: the walked row is cut into
 *             min(64, ceil(s / 16384)) equal contiguous slices, one workgroup each, whose partial count and partial sums go to
 *             a table that a closing launch adds in slice order -- two hubs of an R-MAT graph can each have millions of
 *             entries, and one workgroup must not carry such a pair alone.  Long and sliced pairs are first counted, then
 *             listed (a ballot and one atomic per wavefront).  (4) Sums: a lane adds its terms in ascending position; the lanes
 *             of a group or wavefront close with a fixed shuffle tree; the four wavefronts of a workgroup are added in LDS as
 *             (w0 + w1) + (w2 + w3); slices are added in ascending order.  Every one of these orders depends only on the two
 *             row lengths and on G: that is what makes a pair's bits independent of the batch.  (5) One closing launch forms
 *             the three ratios, copies the mirror entries of edges mode, gathers the degrees and takes the maximum of c.
 *             There is no floating-point atomic anywhere; the integer atomics (the two list tails, the maximum) are 32-bit
 *             vector atomics.  No kernel waits on another workgroup; every walk is bounded by a row length.  The long path stages
 *             no pivots of the searched row in LDS.
 *   bits      identical arguments give identical bits.  common, deg_u, deg_v and the three ratios are canonical: any correct
 *             algorithm gives them.  The two sums depend on G -- the graph's mean degree -- and on the two row lengths only.
 *   state     the call touches none: it voids no prepared or chunked decomposition and leaves the resident bases and the batch
 *             state alone.  Everything it allocates is freed before it returns, on every path: 4 n of degrees, 8 n per sum
 *             asked for, 8 np of pairs, 4 np of counts, 8 np per measure, 4 np per degree output, 16 KiB of partials; then,
 *             once they are counted, 4 bytes per long or sliced pair and 1280 per sliced pair.
 *   errors    LZX_ERR_ARG: null handle; an unknown bit in measures; measures without values; only one of u and v; np != nnz in
 *             edges mode; u[p] >= n, v[p] >= n or u[p] == v[p] (the lists are the host's: both are checked before the device is
 *             touched).  LZX_ERR_STATE: no graph, a handle with a communicator, a graph from a sharded hand-over.
 *             LZX_ERR_LIMIT: np >= 2^32 - 1.  LZX_ERR_NOMEM: the message states the bytes.  np == 0 (after these checks) returns
 *             LZX_OK and touches nothing but *info.  The checks that need no device come first.
 *   limits    one GPU handle; undirected, unweighted graphs; no all-pairs at distance two, no top-k of a seed.  Cosine
 *             similarity c / sqrt(d_u d_v) and preferential attachment d_u d_v are left to the caller, from common, deg_u and
 *             deg_v: the rounding of the device's square root is not pinned here.  A matrix that is not symmetric is not
 *             detected: the call stays within its memory and its numbers mean nothing. */
#define LZX_SIM_JACCARD             1u
#define LZX_SIM_OVERLAP             2u
#define LZX_SIM_SORENSEN            4u
#define LZX_SIM_ADAMIC_ADAR         8u
#define LZX_SIM_RESOURCE_ALLOCATION 16u
typedef struct lzx_similarity_info {
    uint64_t pairs;            /* np */
    uint64_t walked;           /* sum of min(|row u|, |row v|) over the pairs intersected */
    uint64_t short_pairs, long_pairs, sliced_pairs;  /* pairs intersected on each path */
    uint32_t max_common;       /* the largest c */
    uint32_t lanes;            /* lanes per short pair */
    double   loop_ms, prep_ms, count_ms;  /* host clock of the call; device event time of the preparation / of the classification, the walks and the closing launch */
} lzx_similarity_info;
int lzx_similarity(lzx_handle h, uint64_t np, const uint32_t *u, const uint32_t *v /* [np] each; both NULL: every stored entry */,
                   uint32_t measures, uint32_t *common /* [np] or NULL */, uint32_t *deg_u /* [np] or NULL */,
                   uint32_t *deg_v /* [np] or NULL */, double *values /* [popcount(measures)][np], or NULL with measures == 0 */,
                   lzx_similarity_info *info /* or NULL */);

/* ---- greedy colouring, label-propagation communities, modularity ----------------------------------------
 * Three calls on the handle's graph read as undirected and unweighted, each useful alone: a proper vertex colouring
 * (networkx.coloring.greedy_color), the communities of semi-synchronous label propagation over its colour classes
 * (networkx.community.label_propagation_communities) and Newman's modularity of any labelling (networkx.community.modularity).
 * In all three d_v = the number of stored entries of row v NOT counting a diagonal entry, and a diagonal entry (self loop) is
 * ignored everywhere.
 *
 * lzx_color
 *   outputs   The vertices are put in one total order: v comes before u iff d_v > d_u, or the degrees are equal and
 *             hash(v) < hash(u), or both are equal and v < u.  hash(v) is the probe hash above with p = 0:
 *             key = seed + 0x9E3779B97F4A7C15 * (v + 1), then the three xor-shift-multiply steps, mod 2^64.  With
 *             LZX_COLOR_TIES_BY_ID in flags the hash is left out: (d descending, id ascending).  color[v] = the smallest colour
 *             that no neighbour EARLIER in the order has: exactly sequential greedy colouring in that order, and with the flag
 *             networkx's default strategy largest_first on nodes 0 .. n-1.  An isolated vertex gets colour 0.  color may be NULL,
 *             and then no n-vector crosses PCIe.
 *   info      (or NULL) colors = the colours used (the largest + 1); rounds = the windows of the method below = the longest chain
 *             v_1, v_2, ... of vertices each adjacent to and earlier than the next, which makes it canonical; largest_class = the
 *             vertices of the most frequent colour; the host clock of the call and the device event time of the colouring (the
 *             host's reads included).
 *   method    Jones-Plassmann in push form, lzx_core_numbers' structure.  State, u32 [n] each: d, wait, colour, queue.  wait[v] =
 *             the number of earlier neighbours of v, counted over the row by an init launch; the vertices with wait = 0 are
 *             appended to the queue: window 1.  A round handles its window: (1) every window vertex takes the minimum excluded
 *             colour over its earlier neighbours, all coloured by earlier launches; (2) for every later neighbour u,
 *             old = atomicSub(&wait[u], 1), and the one lane that sees old == 1 appends u (aggregated per wavefront), so u is
 *             coloured by the next launch and sees v's colour.  A group of lanes per row (4 to 32, from the mean degree) builds a
 *             64-colour window mask across the group and, while the mask is full, moves the window up by 64 and walks the row
 *             again: at most len / 64 + 1 walks.  Rows of more than 64 times that many entries go to a second launch, a
 *             workgroup per row with an LDS bitmap.  An earlier neighbour has degree >= d_v, so a vertex has fewer than 2^16
 *             earlier neighbours while nnz < 2^32: COLOURS ARE BELOW 2^16, and the bitmap's 8 KiB always suffice.  The host reads
 *             two words per round (the queue's end, the colours) and stops when n vertices are queued.  All atomics are 32-bit
 *             INTEGER vector atomics; no kernel waits on another workgroup; every device loop is bounded by a row length or a
 *             window length; every append is clamped to n.
 *             Ties by id can need n rounds -- a path numbered end to end does, and a ring around a star of 1 500 vertices takes
 *             1 500 rounds by id and 8 hashed -- so hashed ties are the default everywhere else.
 *   bits      color and every integer of info are canonical: any correct implementation of the definition gives them.
 *   state     the call touches none of the handle's.  Everything it allocates (16 n + 12 min(n, 65536) + 64 bytes, n rounded up to
 *             even) is freed before it returns, on every path.
 *   errors    LZX_ERR_ARG: null handle, a flag bit other than LZX_COLOR_TIES_BY_ID.  LZX_ERR_STATE: no graph, a handle with a
 *             communicator, a graph from a sharded hand-over.  LZX_ERR_NOMEM: the message states the bytes.  LZX_ERR_LIMIT: more
 *             than n + 1 rounds, or vertices that still wait when a window comes back empty (only on a matrix that is not
 *             symmetric).  The checks that need no device come first.
 *   limits    colours below 2^16, which holds while nnz < 2^32 (see method); n rounds at the worst, which ties by id reach; and
 *             the limits common to the three calls, below.
 *
 * lzx_label_propagation
 *   outputs   Colour as lzx_color(seed, flags) does, and start from label[v] = v.  A sweep visits the colour classes in
 *             ascending colour; every vertex v of the class that has at least one neighbour u != v is updated, the whole class at
 *             once, from the current labels: H = the labels of greatest multiplicity among v's neighbours; the new label is H's
 *             only member when |H| = 1, the old label when that is in H, max(H) otherwise (Prec-Max, Cordasco and Gargano) --
 *             equivalently the label that maximises (multiplicity, label == old, label).  The call is done after the first sweep
 *             that changes no label, and that sweep is counted.  labels[v] = the SMALLEST VERTEX ID of v's community, caller
 *             order; may be NULL.  With LZX_COLOR_TIES_BY_ID the communities are networkx's label_propagation_communities',
 *             set for set (networkx visits the classes in the order colours first appear, which is ascending).
 *   info      (or NULL) n_communities; largest_size and largest_label (ties go to the smallest label), formed on the device;
 *             sweeps; updates = the label changes over all sweeps; colors and color_rounds of the colouring; inner_entries,
 *             entries, sum_degree_sq and modularity of the result, as lzx_modularity gives them; the host clock of the call, the
 *             device event times of the colouring with the class layout and of the sweeps (the host's reads included).
 *   method    The classes are laid out once by a counting sort of (colour, path): histogram, scan (on the host: three words per
 *             colour), fill; the order inside a class is no output.  A class is one launch per path that has rows (two for the longest rows), the path
 *             chosen by the row's length.  Rows of at most 128 entries: a group of lanes per row stages the neighbours' labels in
 *             its LDS slice, every lane counts the equal labels for its own entries, and the packed key
 *             count << 33 | (label == old) << 32 | label is max-reduced over the group.  Rows of at most 2 048: a workgroup per row
 *             and an open-addressing table in LDS (4 096 slots of a u32 key and a u32 count, 32 KiB, which leaves five workgroups to a
 *             compute unit): atomicCAS on the key slot, atomicAdd on the count, linear probing bounded by the slot count, never
 *             more than half full, then the maximum of the same key over the slots.  Longer rows: the same insertion into a table of
 *             pow2ceil(2 len) slots in global memory, at an offset from a scan over the long rows made once per call, by up to 64
 *             workgroups that share the row's entries; a second launch, the workgroup that owns the table, takes the maximum and
 *             clears the slots it read (the tables are zeroed once per call).  In both tables the lanes of a wavefront whose
 *             labels agree with its first lane's, and then with the first of the rest, are inserted as one: late in a run most
 *             neighbours of a hub carry one label.  Labels are updated in place: the vertices of a class share no edge.  Changed labels are
 *             counted per wavefront into one word and the host reads one word per sweep.  The canonical labels are a 32-bit
 *             atomicMin per vertex into a map, then a gather.  32-bit INTEGER vector atomics only, in LDS and in global memory,
 *             and no floating point, up to the statistics (one 64-bit atomicMax) and the modularity pass; no kernel waits on
 *             another workgroup; every loop is bounded by a row length, a table size or the sweep cap.
 *   bits      labels and every integer of info are canonical: the new label is an arg-max under a total order, so it depends
 *             neither on the path a row takes nor on any thread order.  modularity: see lzx_modularity.
 *   state     the call touches none of the handle's.  Everything it allocates is freed before it returns, on every path:
 *             16 n + 20 n' + 12 min(n, 65536) + 64 bytes for the vertices (n' = n rounded up to even, the third term rounded up to 8) and
 *             8 pow2ceil(2 len) bytes for every row of more than 2 048 entries.
 *   errors    as lzx_color, and LZX_ERR_ARG: max_sweeps == 0.  LZX_ERR_LIMIT: max_sweeps sweeps have run and the last one changed
 *             a label -- labels and info ARE written, with the state after that sweep; a row of 2^30 entries or more.
 *   limits    rows below 2^30 entries; one launch per colour class and path in every sweep, several hundred launches per sweep on
 *             an R-MAT graph (merging the thin classes' launches is not done); and the common limits below.
 *
 * lzx_modularity
 *   outputs   *q = Newman's modularity at resolution 1 of the labelling labels[v] < n (any labelling; label values need not be
 *             members of their community).  D_c = the sum of d_v over the community, I_c = the stored off-diagonal entries with
 *             both ends in c (twice the inner edges), M = the sum of the D_c (twice the edges):
 *             q = the sum over the labels that occur, ascending, of (double)I_c / (double)M - ((double)D_c / (double)M)^2,
 *             formed in that order in fp64 without contraction; q = 0 on a graph without an edge.
 *   info      (or NULL) communities = the distinct labels; inner_entries = the sum of the I_c; entries = M; sum_degree_sq = the sum
 *             of the D_c^2 mod 2^64 (exact while M < 2^32); the host clock of the call.
 *   method    The integers are formed on the device: one launch counts, per row, the neighbours with the row's label (a group of
 *             lanes per row, long rows a workgroup each); one launch adds d_v and that count to u64 [n] accumulators with 64-bit
 *             integer atomics, one add per row at the most, the lanes of a wavefront whose labels agree combined first (one
 *             community can hold most of the graph).  The accumulators cross PCIe (16 n bytes) and the host adds the terms.
 *   bits      every integer is canonical, and q is bit-identical to the same loop in Python floats; it is within
 *             (C + 4) 2^-52 of networkx.community.modularity, C the number of communities: every term lies in [-1, 1] and carries
 *             at most four roundings.
 *   state     the call touches none of the handle's; 28 n + 64 bytes (n rounded up to even in the u32 arrays), freed on every path.
 *   errors    LZX_ERR_ARG: null handle, null labels or q, a label >= n (the message names its index and value).  LZX_ERR_STATE,
 *             LZX_ERR_NOMEM: as above.  The labels are checked before the device is touched.
 *   limits    resolution 1 only; the accumulators cross PCIe, 16 n bytes per call; and the common limits below.
 *
 *   limits    (all three) one GPU handle; undirected, unweighted graphs; Louvain is lzx_louvain below, and what is still
 *             missing is Leiden's refinement, a resolution parameter and weighted input; no asynchronous or seeded-random label
 *             propagation.  A matrix that is
 *             not symmetric is not detected: its numbers mean nothing, but the calls return and stay within their memory --
 *             appends are clamped, rounds and sweeps are capped, every label is a vertex id. */
#define LZX_COLOR_TIES_BY_ID 1u
typedef struct lzx_color_info {
    uint32_t colors;         /* colours used */
    uint32_t rounds;         /* windows = the longest chain of the order */
    uint32_t largest_class;  /* vertices of the most frequent colour */
    uint32_t reserved_;
    double   loop_ms, color_ms;  /* host clock of the call; device event time of the colouring */
} lzx_color_info;
int lzx_color(lzx_handle h, uint64_t seed, uint32_t flags, uint32_t *color /* [n] or NULL */, lzx_color_info *info /* or NULL */);

typedef struct lzx_communities_info {
    uint64_t n_communities, largest_size;
    uint64_t updates;        /* label changes over all sweeps */
    uint64_t inner_entries, entries, sum_degree_sq;  /* lzx_modularity's integers of the result */
    uint32_t largest_label;  /* of the largest community; ties go to the smallest label */
    uint32_t sweeps;         /* the last one changed nothing, unless LZX_ERR_LIMIT */
    uint32_t colors, color_rounds;
    double   modularity;
    double   loop_ms, color_ms, sweep_ms;  /* host clock of the call; device event time of the colouring / of the sweeps */
} lzx_communities_info;
int lzx_label_propagation(lzx_handle h, uint64_t seed, uint32_t flags, uint32_t max_sweeps, uint32_t *labels /* [n] or NULL */,
                          lzx_communities_info *info /* or NULL */);

typedef struct lzx_modularity_info {
    uint64_t communities;    /* distinct labels */
    uint64_t inner_entries;  /* sum of I_c */
    uint64_t entries;        /* M = sum of D_c */
    uint64_t sum_degree_sq;  /* sum of D_c^2 mod 2^64 */
    double   loop_ms;
} lzx_modularity_info;
int lzx_modularity(lzx_handle h, const uint32_t *labels /* [n], values < n */, double *q, lzx_modularity_info *info /* or NULL */);

/* ---- Louvain communities --------------------------------------------------------------------------------
 * lzx_louvain: the communities of the Louvain method (Blondel et al.; networkx.community.louvain_communities and
 * louvain_partitions) on the handle's graph read as undirected and unweighted: local moves that raise the modularity, then the
 * communities become the nodes of a weighted level graph, and again, until a level changes nothing.  The result is canonical: a
 * function of the graph, the seed and the flag, formed in integers only.
 *   outputs   A LEVEL GRAPH has n_l nodes, rows ascending by column and a weight w_ij >= 1 (u32) per stored entry; w_ii, the inner
 *             weight, counts both directions.  Level 0 is the caller-order pattern with w_ij = 1 off the diagonal and a diagonal entry
 *             ignored (w_ii = 0).  k_i = the sum of row i with the diagonal; M = the sum of the k_i, the same on every level (the
 *             off-diagonal entries); d_i = the off-diagonal ENTRIES of row i.  Every level graph is coloured as lzx_color(seed, flags)
 *             colours it: the order is (d descending, hash(seed, i) ascending, i ascending), i the node's id on that level.
 *             A SWEEP starts from label[i] = i, tot[c] = k_c on the level's first sweep and takes the colour classes in ascending
 *             colour.  Every node i of the class with d_i > 0 decides from the labels and tot as they stand when its class begins:
 *             a = label[i]; for every label c among the neighbours j != i, k_ic = the sum of w_ij over those with label[j] = c
 *             (k_ia = 0 if a does not occur); T_c = tot[c], T_a = tot[a] - k_i; G(c) = M k_ic - T_c k_i; c* = the c != a of the
 *             largest G, ties to the smallest c; i moves to c* iff G(c*) > G(a).  When the whole class has decided, label[i] = c*,
 *             tot[a] -= k_i, tot[c*] += k_i for every mover.  The nodes of a class share no edge, so every k_ic is exact and only
 *             tot is one class stale.  A LEVEL: Qnum = M I - the sum of tot[c]^2, I = the sum over i of w_ii + the w_ij of the
 *             j != i with label[j] = label[i].  A sweep without a move ends the level.  Otherwise, if Qnum after the sweep is <=
 *             Qnum before it, the labels and tot from before the sweep are put back, the level ends and reverted = 1 (the sweep is
 *             counted in sweeps, its moves are not counted).  Otherwise its moves are added and the next sweep runs; after
 *             max_sweeps accepted sweeps the level ends with capped = 1, which is no error.  AGGREGATION: the distinct labels in
 *             ascending order become the nodes 0 .. C-1 of the next level, w'_pq = the sum of the w_ij over all entries (diagonal
 *             included) between p and q.  If C = n_l the level changed nothing: it is not counted and the call is done; it is also
 *             done after max_levels counted levels, which is no error.
 *             labels[v] = the SMALLEST ORIGINAL VERTEX ID of v's final community (a vertex without an edge is its own);
 *             level_labels[l][v] = the same for the partition after counted level l; levels[l] = that level's record.  Rows of
 *             level_labels and levels at or beyond info.levels are left untouched.  Each of the three may be NULL.
 *   levels[l] nodes, entries (stored entries of the level graph: level 0's diagonal entries count), communities (C), moves (of the
 *             accepted sweeps), inner_entries (I) and sum_degree_sq (the sum of tot^2) after the level; colors and color_rounds of
 *             its colouring; sweeps (every sweep that ran: the last one without a move, or taken back, included); reverted; capped;
 *             path_rows[3] = the rows the decide step gave to each of its three paths in one sweep, by stored row length (rows
 *             without an entry are rows of the first).
 *   info      (or NULL) n_communities, largest_size, largest_label (ties to the smallest label); levels = the counted levels; sweeps
 *             and moves summed over them; inner_entries, entries, sum_degree_sq and modularity of labels exactly as lzx_modularity
 *             gives them; the host clock of the call; the device event times of the colourings, the sweeps and the aggregations.
 *   method    Per level: the colouring and the class sort of lzx_label_propagation on a view of the level graph; the far tables of
 *             its rows above 2 048 entries; an init launch (k, tot, labels, I); then per sweep and class one decide launch per path
 *             that has rows, templated on whether a weight array is read (level 0 reads none).  Rows of at most 128 entries: a
 *             group of lanes stages labels and weights in its LDS slice, every lane sums the weights of the equal labels for its
 *             own entries, gathers tot, forms G in int64, and (G, smallest c) is max-reduced over the group.  Rows of at most
 *             2 048: a workgroup and the 4 096-slot LDS table, the count slot a weight sum; every slot forms its G and the pair is
 *             max-reduced over the workgroup.  Longer rows: the table in global memory, an insert launch by up to 64 workgroups
 *             per row and a pick launch.  A mover writes its own label in place (nobody in its class reads it) and is appended,
 *             one atomic per wavefront, to a move list of (i, a, c*, k_ic* - k_ia); tot is NOT written while a class decides.  A
 *             second launch over the class's window of the list applies tot[a] -= k_i, tot[c*] += k_i with 32-bit integer atomics
 *             and adds 2 (k_ic* - k_ia) to I with one 64-bit integer atomic per wavefront: exact, since the movers of a class are
 *             not adjacent.  The sum of tot^2 is a reduction over n_l words per sweep.  The host reads the move count and the two
 *             integers of Qnum once per sweep.  Aggregation: flag the labels that occur, exclusive scan, every entry becomes the
 *             64-bit key p << 32 | q with its weight (level 0's diagonal entries are dropped here), a hipcub radix sort by key, a
 *             reduce by key, the row pointers by binary search in the keys.  The map vertex -> node of the level stays on the
 *             device; the canonical labels are lzx_label_propagation's kernels.  No floating point and no floating-point atomic
 *             before the modularity of the result; no kernel waits on another workgroup; every loop is bounded by a row length, a
 *             table size or a cap; every append is clamped.
 *   bits      labels, level_labels and every integer of levels and info are canonical: G is an integer, the arg-max is under a
 *             total order, the sums of the aggregation are integers, so nothing depends on the path a row takes or on any thread
 *             order.  modularity: bit for bit lzx_modularity's value of labels.
 *   state     the call touches none of the handle's.  Everything it allocates is freed before it returns, on every path:
 *             16 n + 56 n' + 12 min(n, 65536) + 128 bytes for the vertices (n' = n rounded up to even, the third term rounded up to
 *             8), held through the call; 8 pow2ceil(2 len) bytes for every row of more than 2 048 entries of the level at hand;
 *             from the first aggregation on 16 nnz + 8 nnz' + 16 bytes of keys and weights plus hipcub's scratch for nnz pairs; and
 *             8 (C + 1) + 8 E' bytes for the level graph at hand (C nodes, E entries rounded up to even), the next one beside it
 *             while it is built.
 *   errors    LZX_ERR_ARG: null handle, a flag bit other than LZX_COLOR_TIES_BY_ID, max_sweeps == 0, max_levels == 0 or > 64.
 *             LZX_ERR_STATE: no graph, a handle with a communicator, a graph from a sharded hand-over.  LZX_ERR_LIMIT: 2^31 stored
 *             entries or more (M is at most the stored entries; below 2^31 every G, Qnum and tot^2 fits a signed 64-bit integer and
 *             tot, k and every k_ic fit u32); a row of 2^30 entries or more; the colouring's own limits.  LZX_ERR_NOMEM: the message
 *             states the bytes held and asked for, at every allocation.  The checks that need no device come first.
 *   limits    one GPU handle; undirected, unweighted input; resolution 1; no refinement step (Leiden), so a community can be
 *             internally disconnected; one colouring per level; one launch per colour class and path in every sweep; the guard
 *             compares whole sweeps, so a sweep that is taken back ends the level even if part of it was an improvement; the
 *             aggregation sorts all entries of the level (24 nnz bytes and hipcub's scratch at level 0); and a matrix that is not
 *             symmetric is not detected: its numbers mean nothing, but the call returns and stays within its memory. */
typedef struct lzx_louvain_level {
    uint64_t nodes, entries;       /* of the level graph */
    uint64_t communities;          /* C: the nodes of the next level */
    uint64_t moves;                /* of the accepted sweeps */
    uint64_t inner_entries;        /* I after the level */
    uint64_t sum_degree_sq;        /* the sum of tot^2 after the level */
    uint32_t colors, color_rounds; /* of the level's colouring */
    uint32_t sweeps;               /* every sweep that ran */
    uint32_t reverted, capped;     /* the last sweep was taken back; max_sweeps accepted sweeps ran */
    uint32_t path_rows[3];         /* rows per decide path in one sweep */
} lzx_louvain_level;
typedef struct lzx_louvain_info {
    uint64_t n_communities, largest_size;
    uint64_t sweeps, moves;        /* over the counted levels */
    uint64_t inner_entries, entries, sum_degree_sq;  /* lzx_modularity's integers of labels */
    uint32_t largest_label;        /* of the largest community; ties go to the smallest label */
    uint32_t levels;               /* counted levels */
    double   modularity;
    double   loop_ms, color_ms, sweep_ms, aggregate_ms;  /* host clock of the call; device event times */
} lzx_louvain_info;
int lzx_louvain(lzx_handle h, uint64_t seed, uint32_t flags, uint32_t max_sweeps, uint32_t max_levels /* 1 .. 64 */,
                uint32_t *labels /* [n] or NULL */, uint32_t *level_labels /* [max_levels][n] or NULL */,
                lzx_louvain_level *levels /* [max_levels] or NULL */, lzx_louvain_info *info /* or NULL */);

/* ---- sweep cuts ----------------------------------------------------------------------------------------
 * lzx_sweep_cut: what turns a score vector -- a Fiedler vector of lzx_eigsh_f64, a personalised lzx_pagerank_f64, a heat kernel
 * e^(-tL) x -- into a set of vertices (Cheeger sweep; Andersen, Chung and Lang; Chung's heat-kernel PageRank): the vertices
 * are ordered by score, cut(S_k) / min(vol S_k, vol of the rest) is evaluated for every prefix S_k of the order, and the best
 * prefix is returned.  Up to 16 score vectors (columns) per call share one pass over the edges.  With an indicator score and
 * k_min = k_max = |S| it gives networkx.cut_size, volume, conductance and edge_expansion of S.  The graph is read as undirected
 * and unweighted; d_v = the number of stored entries of row v NOT counting a diagonal entry, M = the sum of the d_v, and a
 * diagonal entry (self loop) changes no output.
 *   inputs    scores: ns columns of n doubles, column c at scores + c * n, the caller's vertex order, host memory.
 *   key       of vertex v in a column: s_v; with LZX_SWEEP_PER_DEGREE s_v / (double)d_v, one IEEE division, and a vertex with
 *             d_v = 0 comes after all others whatever its score.  -0.0 counts as +0.0; +-inf are ordinary keys; a NaN score is
 *             LZX_ERR_ARG (the message names the column and the index; checked before the device is touched).
 *   order     descending key, ascending with LZX_SWEEP_ASCENDING; ties go by ascending vertex id in both directions.
 *             order[c * n + i] = the vertex at position i of column c; pos is its inverse.  May be NULL.
 *   profile   S_k = the first k vertices of the order.  vol[c * n + k - 1] = the sum of d over S_k.  b_v = the number of
 *             neighbours u != v with pos[u] < pos[v], and cut[c * n + k - 1] = the sum of d_v - 2 b_v over S_k = the number
 *             of edges that leave S_k; cut[n - 1] = 0 and vol[n - 1] = M.  Each may be NULL; only the outputs asked for cross
 *             PCIe.
 *   best      best[c]: the best prefix over k in [k_min, k_max]; k_min = 0 means 1 and k_max = 0 means n - 1.  den_k =
 *             min(vol_k, M - vol_k) (conductance, the default) or min(k, n - k) with LZX_SWEEP_EXPANSION (edge expansion);
 *             prefixes with den_k = 0 are left out.  The best k minimises cut_k / den_k, compared exactly: a is better than b
 *             iff cut_a * den_b < cut_b * den_a in 64-bit integers; ties go to the smallest k.  value = (double)cut /
 *             (double)den, one division.  With no admissible k (a graph without an edge, n = 1, a window of prefixes with
 *             den = 0 only, k_min = n with k_max = 0): k = cut = vol = den = 0, value = +inf, and the call returns LZX_OK.
 *   info      (or NULL) entries = M; ns and width = the columns of the call and B, the width they were padded to (1, 2, 4,
 *             8 or 16); the host clock of the call and the device event times of the sorts (uploads, keys and positions
 *             included), of the edge sweep, and of the scans with the reduction.
 *   method    Per column: one launch maps the score to an order-preserving u64 key (complemented for descending order, all
 *             ones for a vertex the per-degree rule puts last) beside the ids 0 .. n-1; hipcub's radix sort of the pairs is
 *             stable, so ties keep their ascending ids; one launch writes pos, interleaved as u32 [n][B].  Then ONE pass over
 *             the edges for all columns: a group of lanes per row (4 to 32, from the mean degree) loads, for every neighbour
 *             u != v, the B positions of u as one line (16-byte loads where B >= 4), compares them with v's and counts in B
 *             registers; the counts and d_v are summed over the group by shuffles and stored, d_v - 2 b_v (i64) and d_v (u64),
 *             at place pos[v][c] of column c's arrays.  Rows of more than 64 times that many entries are listed (one
 *             wavefront-aggregated append each; the list's order is no output) and go to a second launch, a workgroup per
 *             row; both run only when such a row exists.  hipcub's inclusive sums over the two arrays give cut and vol; a
 *             block-partial launch and a close launch apply the comparison above, and the host reads five words per column.
 *             The sweep has no atomics and, after the key, nothing is floating-point; no kernel waits on another workgroup;
 *             every loop is bounded by a row length, the list or the window.
 *   bits      every output is an integer or one correctly rounded division of two integers: all of them are canonical, and
 *             column c's outputs are bit-identical whatever else is in the batch and wherever c stands in it.
 *   state     the call touches none of the handle's.  Everything it allocates is freed before it returns, on every path:
 *             4 n B (rounded up to 16) + 16 n + 16 ns n + 24 ns g + 40 ns + 8 + 8 n' bytes (n' = n rounded up to even, g =
 *             min(w / 256 + 1, 1024) blocks for a window of w + 1 prefixes), and behind it hipcub's temporary storage.
 *   errors    LZX_ERR_ARG: null handle, scores or best; ns = 0; a flag bit other than the three; k_max > n; k_min > k_max
 *             (k_min > n when k_max = 0); a NaN score.  LZX_ERR_LIMIT: ns > 16; nnz >= 2^32 (the products of the comparison
 *             are below 2^63 because M < 2^32).  LZX_ERR_STATE: no graph, a handle with a communicator, a graph from a
 *             sharded hand-over.  LZX_ERR_NOMEM: the message states the bytes.  The checks that need no device come first.
 *   limits    one GPU handle; undirected, unweighted graphs; the columns of a call share flags and window; 16 ns n bytes of
 *             profile state whether or not the profile is asked for.  A matrix that is not symmetric is not detected and its
 *             numbers mean nothing, but the call returns and stays within its memory: every store goes to a place of the
 *             order's permutation, and signed 64-bit arithmetic covers a negative running cut. */
#define LZX_SWEEP_ASCENDING  1u
#define LZX_SWEEP_PER_DEGREE 2u
#define LZX_SWEEP_EXPANSION  4u
typedef struct lzx_sweep_result {
    uint64_t k;              /* vertices of the best prefix; 0: no admissible prefix */
    uint64_t cut, vol, den;  /* of that prefix */
    double   value;          /* (double)cut / (double)den; +inf with k = 0 */
} lzx_sweep_result;
typedef struct lzx_sweep_info {
    uint64_t entries;        /* M */
    uint32_t ns, width;      /* columns; the width B they were padded to */
    double   loop_ms, sort_ms, sweep_ms, scan_ms;  /* host clock of the call; device event times of its three stages */
} lzx_sweep_info;
int lzx_sweep_cut(lzx_handle h, uint32_t ns, const double *scores /* [ns][n] */, uint32_t flags, uint64_t k_min, uint64_t k_max,
                  uint32_t *order /* [ns][n] or NULL */, uint64_t *cut /* [ns][n] or NULL */, uint64_t *vol /* [ns][n] or NULL */,
                  lzx_sweep_result *best /* [ns] */, lzx_sweep_info *info /* or NULL */);

/* ---- measurement hook --------------------------------------------------------------------------
 * Runs `reps` back-to-back SpMVs of the current graph on a device-resident vector and returns the
 * average and minimum HIP-event time of one SpMV (all its kernels) in milliseconds.              */
int lzx_bench_spmv(lzx_handle h, uint32_t reps, double *avg_ms, double *min_ms);

/* Measurement hook (no reference counterpart): the device's own streaming rates, for the roofline's "fraction of a
 * measured STREAM kernel on the same box" (SURVEY.md 8(d)): a read-only sum and a copy over a scratch buffer of `bytes`
 * bytes (rounded to 16; >= 256 MiB recommended), best of `reps`.  Results in GB/s (copy: bytes read + bytes written). */
int lzx_bench_stream(lzx_handle h, uint64_t bytes, uint32_t reps, double *read_gbs, double *copy_gbs);

/* Values of the option "operator" (below). */
#define LZX_OP_ADJACENCY 0
#define LZX_OP_LAPLACIAN 1

/* Options, to be set before the graph is handed over ("reorthogonalise", "basis_fp32", "reference_order" and "operator":
 * any time; setting one abandons a decomposition that was being advanced in chunks):
 *   "hub_entries"           x values of the highest-degree vertices staged in LDS by the SpMV (0 = none)
 *   "propagation_blocking"  1 / 0 force the two-pass blocked treatment of non-staged columns on / off
 *                           (default: on for graphs whose x does not fit the L2s); with it off the sliced-ELL
 *                           rows are summed in the reference's order and come out bit-identical to serial/
 *   "overlap_exchange"      several ranks: 1 / 0 ask for / forbid the two-chunk all-gather that overlaps the blocked
 *                           SpMV (default: on for in-process groups; over RCCL only on request -- bench.py asks in its
 *                           guarded tuning phase -- until it has run once on two or more physical GPUs)
 *   "sparse_exchange"       1 / 0: with the two-chunk exchange, send each peer only the entries of the second chunk its rows
 *                           reference (default 1)
 *   "exchange_fp32"         1: several ranks exchange the new Lanczos vector rounded to fp32 (half the bytes; one all-gather,
 *                           sums stay fp64).  Off by default and NOT within the 1e-10 criterion: 6e-8 relative rounding per
 *                           entry and iteration ends near 1e-8 in the centrality vector (6.9e-9 measured on BASELINE C1;
 *                           the reference's own float runs end at 1.2e-6, parallel-final/output/single_double.txt:319)
 *                           -- SURVEY 8(f) N4.  Every rank multiplies the rounded vector in ALL entries, its own slice
 *                           included, while the inner product and the norm use the unrounded local vector.
 *   "lazy_normalisation"    1: multiply (and, with several ranks, exchange) the unnormalised vector, so that alpha and
 *                           beta come out of one reduction per iteration (one 2-double all-reduce) and one vector kernel;
 *                           0: the reference's operation order.  Default: 1 with several ranks and in blocked mode, 0 on
 *                           one GPU in plain mode.
 *                           NB with it on, alpha_j = D / B is formed from the sums over the UNNORMALISED vector -- not the
 *                           reference's operation order (serial/lib/lanczos.cc:26: alpha_j = <A q_j, q_j>); same recurrence,
 *                           operands rounded at other places, covered at 1e-10 on the fixtures (tests/test_gpu_parity.py)
 *   "timing_marks_every"    iterations between the HIP-event timing marks behind lzx_stats (default 4; 1 = every iteration)
 *   "reorthogonalise"       e > 0: the Arnoldi pass of serial/lib/lanczos.cc:58-132 (decompose_with_arnoldi): when j % e == 0
 *                           and j > 2, A q_j is orthogonalised against q_0 .. q_{j-2} (modified Gram-Schmidt in the
 *                           reference's order, one launch per basis vector) before alpha_j is taken.  The reference
 *                           hard-codes e = 2 (:71) -- which lets orthogonality go between two passes and then removes
 *                           components T does not record: "neither give good results", serial/tests/numerical_test_orthog.cc:3-4,
 *                           and on BASELINE C2 at k = 50 it is off by O(1) -- e = 1 keeps the basis orthogonal (C2, k = 50:
 *                           1e-11 from the extended-precision referee where the plain loop is 3e-8 away).  Runs the reference's
 *                           operation order (lazy_normalisation off).  Default 0 = off, as in the reference's production path.
 *                           May be changed between decompositions.
 *   "basis_fp32"            1: the resident basis is STORED as fp32 (half the HBM: 4.0 -> 2.0 GB at C3, k = 50), the three
 *                           vectors the recurrence works on stay fp64, so alpha / beta are those of the fp64 loop bit for
 *                           bit; lzx_multout_f64 and the host fetch read the rounded columns (6e-8 relative per entry:
 *                           the centrality vector ends near 1e-8, outside the 1e-10 criterion; the reference's float runs
 *                           end at 1.2e-6, parallel-final/output/single_double.txt:58-63).  Selects the lazy loop (an error with
 *                           lazy_normalisation = 0 or reorthogonalise).  Default 0.
 *                           SURVEY 8(f) N4.  May be changed between decompositions.
 *   "reference_order"       1: the loop with serial/'s own REDUCTION orders, for a maintainer who wants the device path to
 *                           reproduce the CPU path's numbers exactly: the SpMV one lane per row of the caller's CSR, entries
 *                           added in ascending column order (serial/lib/SPMV.cc:24-27 = cu_spMV1, parallel-final/lib/cu_SPMV.cu:31-41),
 *                           inner product and norm ONE left-to-right accumulator over the caller's vertex order
 *                           (serial/lib/lanczos.cc:155-171); the elementwise updates as in every mode.  alpha, beta and
 *                           the basis then equal serial/'s restatement BIT FOR BIT at any k (tests: every fixture, and the
 *                           1 M- and 10 M-vertex benchmark graphs at k = 50), also together with "reorthogonalise".  A parity
 *                           instrument, not a fast path (about 70 ms per iteration at 10 M vertices); one rank only.
 *                           Default 0.  May be changed between decompositions.
 *   "placement_trials"      t >= 0: at the end of a graph hand-over in blocked mode the value stream between the SpMV's two
 *                           passes is allocated t more times, the SpMV timed with each candidate and the fastest kept (a few
 *                           SpMVs of set-up time each; results are bit-identical whichever wins).  Where the driver places
 *                           that one buffer decides up to 15 % of the SpMV on uniform graphs and 1-2 % on R-MAT ones for the
 *                           life of the allocation -- the reference's cudaMalloc blocks (cu_lanczos.cu:37-86) have no
 *                           counterpart.  At most three candidates are alive at a time (the best so far, the one being timed,
 *                           the last loser).  Default 2 (round 5: a library that may live inside a host framework does not
 *                           multiply a buffer at its hand-over; bench.py asks for 7 and reports every candidate's time);
 *                           at most 7; 0 = take the first allocation.
 *   "sharded_ingest"        s > 0: every hand-over entry point builds the graph WITHOUT ever holding all of it on one
 *                           device -- the loader of parallel-final/lib/adjMatrix.cc:21-46 for graphs beyond one card (SURVEY.md 7.1
 *                           step 7).  The whole-graph hand-over sorts all 2 m directed entries at once and leaves the whole CSR
 *                           on every rank; with this option a rank sweeps the source (the seeded generator re-drawn, or the
 *                           resident endpoint pairs) in bounded batches -- degrees, then the staged-column counts that order
 *                           rows of equal degree, then ITS OWN rows -- and nothing is exchanged: all ranks compute the same
 *                           ranking from the same source.  The tables are those of the whole-graph hand-over entry for entry
 *                           (same bits in every result).  s = 1: batches of 2^28 entries; s >= 2: exactly s batches per sweep
 *                           (tests).  With several ranks lzx_get_graph_csr then fails with LZX_ERR_STATE (no rank holds the
 *                           graph), the matrix must be symmetric as documented above (the sparse exchange lists rely on it),
 *                           and "reference_order" stays a one-rank instrument.  lzx_set_graph_csr / _csr32: the CSR stays in the
 *                           caller's memory and is streamed past the device in chunks of whole rows (row_ptr once, col_idx
 *                           twice); the rank keeps its own rows -- what parallel-two-cards does for its two halves
 *                           (parallel-two-cards/lib/cu_lanczos.cu:94-95,108-109).  Default 0.  C5, rank 0 of 8: 19 GB at the peak and 8.7 GB
 *                           resident instead of 102 / 17+ GB, 12.7 s instead of 5.8 s (profiles/r4_sharded_ingest.txt).
 *   "operator"              the matrix M the Krylov space is built on.  LZX_OP_ADJACENCY (0, default): M = A, as above.
 *                           LZX_OP_LAPLACIAN (1): the combinatorial Laplacian M = L = D - A, d_i = the number of stored
 *                           entries of row i (rows without an edge: d_i = 0, (L x)_i = 0), for the heat kernel e^{-tL} x.
 *                           (L x)_i := fma(d_i, x_i, -s_i), s_i = row i of A x summed exactly as the current mode sums it,
 *                           one explicit fused multiply-add on the device and in the C++ class path alike, so that
 *                           "reference_order" stays bit-identical to that path.  The per-row degree array (4 bytes per
 *                           row) is built on the first use of L and kept as long as the graph; A allocates nothing new.
 *                           Breakdown stop: L 1 = 0, so the start vector ones (and any vector in a small invariant
 *                           subspace) exhausts the Krylov space.  Under L a beta_j <= 2^-40 * 2 d_max (2 d_max: the
 *                           Gershgorin bound of ||L||) is returned as exactly 0 and so are every later alpha, beta and
 *                           basis column; the caller trims T at the first zero beta.  Under A nothing changes.
 *                           Where L runs: every loop form -- plain, lazy (one rank or several, every exchange and
 *                           reduction), "reference_order", "reorthogonalise" -- applies v = fma(d, q, -v) after the SpMV,
 *                           and lzx_spmv_f64 / _local return L x.  The batched path applies fma(d_i, X[i][c], -sum) after
 *                           the chunk totals of split rows (lzx_spmm_f64 returns L X) and stops a column at the same
 *                           threshold.  Refused with LZX_ERR_STATE (and a message): "basis_fp32" (it stores the
 *                           unnormalised basis u_j = beta_{j-1} q_j, which a stop leaves with beta = 0 to divide by; under L
 *                           the lazy loop keeps q_j), and a sharded hand-over of a CSR in host memory (no rank holds the row
 *                           pointers the degrees come from).  Any other value: LZX_ERR_ARG.  May be changed between
 *                           decompositions.
 * These thirteen are all liblzx.so knows.  The experiment knobs and test hooks behind DESIGN.md's tuning log ("pb_*",
 * "phase_mask", "exchange_at_world_1", ...) exist only in liblzx_dbg.so, the same sources built with -DLZX_DEBUG_KNOBS
 * (`make debug`); tools/perf_probe.py and the tests that need them load that library.                               */
int lzx_set_option(lzx_handle h, const char *name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* LZX_H_ */
