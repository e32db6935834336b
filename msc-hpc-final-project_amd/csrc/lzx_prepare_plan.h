// lzx_prepare_plan.h -- the decisions of the graph hand-over (lzx_graph.hip: lzx_graph_prepare), host only: the layout
// constants they use, small value structs and pure functions over them.  Nothing of HIP and nothing else of the project is
// included, so tests/prepare_plan_check.cc runs every line below on a CPU against tests/sell_model.py and
// tests/partition_model.py.  lzx_internal.h includes this header.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

typedef uint32_t u32;
typedef uint64_t u64;

// ---- layout constants -----------------------------------------------------------------------------
// Sliced-ELL body: slices of 64 rows (one wavefront), column indices stored so that lane l of the
// wave reads 16 contiguous bytes (4 indices of ITS row) per step and the wave reads 1 KiB contiguous.
static constexpr u32 LZX_SLICE = 64;
// Rows with more entries than this leave the sliced-ELL body and are split into wave-sized items.
static constexpr u32 LZX_LONG_ROW = 128;
// Entries one wavefront sums per split-row item (multiple of 256 = 64 lanes x 4 indices).
static constexpr u32 LZX_ITEM = 2048;
// Threads per workgroup of the SpMV kernel (16 wavefronts share one LDS copy of the hub entries).
static constexpr u32 LZX_SPMV_BLOCK = 1024;
static constexpr u32 LZX_VEC_BLOCK = 256;
// Zero tail behind every full-length vector: the padding column index points here.
static constexpr u32 LZX_TAIL = 64;
// Propagation blocking (csrc/lzx_pb.hip): column band staged in LDS by the scatter phase (doubles),
// rows per wavefront-private LDS y tile in the gather phase.
static constexpr u32 LZX_PB_CB = 16384;
static constexpr u32 LZX_PB_CB_WIDE = 18432;   // test shape pb_column_band: 144 KiB of x per tile (nine 2 Ki-value staging rounds of the 1 024 threads)

inline u32 round_up(u32 a, u32 m) { return (a + m - 1) / m * m; }

// splitmix64 finaliser: the hash of the sparse exchange's index lists (lzx_plan_sx_hashes, lzx_comm_check_sparse)
inline u64 lzx_mix64(u64 z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- what the decisions read: the graph's size, the communicator, the options (-1 = unset) ---------
struct lzx_plan_in {
    u64 n = 0, nnz = 0;
    u32 world = 1, rank = 0, cu_count = 0;
    int comm_kind = 0;
    bool force_multi = false;
    int64_t pb_opt = -1, hub_opt = -1, overlap_opt = -1, xfp32_opt = -1, pb_cb_opt = -1, sparse_opt = -1, tie_sort_opt = -1;
    int64_t long_row_opt = -1, item_opt = -1, narrow_opt = -1, wgs_per_cu_opt = -1, spmv_wgs_opt = -1;
};

// ---- step 3: this rank's rows split into split rows, their items and the 64-row slices; the slices' order; the grid ----
struct lzx_row_plan {
    u32 long_thr = 0, n_long_true = 0, n_long64 = 0, n_slices = 0, n_items = 0;
    u64 long_elems = 0, sell_elems = 0;
    std::vector<u64> h_long_ptr, h_item_beg, h_slice_off;
    std::vector<u32> h_item_first, h_item_len, h_slice_w;
    bool classes = false;              // the slices are processed class by class (blocked mode, k_spmv)
    std::vector<u32> perm, h_slice_w0;
    u32 ns_wide = 0, ns_w8 = 0, ns_w4 = 0;
    u32 per_cu = 0, spmv_grid = 0, fin_grid = 0;
};

struct lzx_plan {
    lzx_plan_in in;
    // before the ranking (lzx_plan_layout)
    u32 n_loc_pad = 0, ldq = 0, n_loc_real = 0;
    u64 iolen = 0;
    bool pb = false;                   // blocked mode, as far as decided: the ranking can still take it back
    u32 hub_real = 0, hub = 0;
    size_t spmv_lds = 0;
    // behind the ranking (lzx_plan_ranked)
    u64 n_active = 0;
    u32 max_degree = 0, rows_live = 0, xs = 0, xs0 = 0;
    u64 xlen = 0;
    bool xfp32 = false, overlap = false;
    bool tie_sort = false;             // step 1a runs
    bool try_sparse = false;           // step 1b runs
    u32 sentinel = 0;                  // the padding code of the tables
    lzx_row_plan rows;
};

inline size_t lzx_plan_spmv_lds(u32 hub) { return ((size_t)hub + LZX_SPMV_BLOCK / 64) * sizeof(double); }

// The layout that follows from the sizes alone, and the first choice of blocked mode and staged slots.  Returns the message of the
// limit that was hit (a format that takes n as unsigned long long), or nullptr; behind a limit nothing further is filled in.
inline const char *lzx_plan_layout(lzx_plan &P)
{
    const lzx_plan_in &in = P.in;
    const u64 n = in.n;
    const u32 world = in.world, rank = in.rank;
    if (n >= (1ull << 31)) return "n = %llu: this build indexes vertices with 31 bits";
    const u32 per = (u32)((n + world - 1) / world);
    P.n_loc_pad = round_up(per, LZX_SLICE);
    P.ldq = P.n_loc_pad + LZX_TAIL;
    P.iolen = (u64)world * P.n_loc_pad + LZX_TAIL;
    P.xs = P.n_loc_pad;          // refined by lzx_plan_ranked once the number of vertices with an edge is known
    P.xlen = P.iolen;
    P.n_loc_real = (rank < n) ? (u32)((n - rank + world - 1) / world) : 0;
    if (P.iolen + 65536 >= (1ull << 32)) return "exchange layout does not fit 32-bit codes";

    // Propagation blocking (lzx_pb.hip) for every entry whose column is not staged in LDS.  -1 = decide here.
    // Measured (DESIGN.md section 3, 1 GPU, plain / blocked SpMV): C3 (10 M vertices, x far beyond the L2s) 2.13 / 1.05 ms;
    // C2 (1 M vertices, x = 8 MB, L2-resident) 0.136 / 0.103 ms -- since high-degree rows cross the two passes as partial
    // sums the blocked form also wins while x still fits the caches.  Below about 8 Mi entries per rank its extra
    // launches and the per-unit 128 KiB column band cost more than the gathers they replace.
    P.pb = in.pb_opt > 0 || (in.pb_opt < 0 && n >= (512u << 10) && in.nnz / (u64)world >= (8u << 20));
    // hub entries staged in LDS by k_spmv: 8192 (64 KiB, two workgroups per CU) when k_spmv also gathers from
    // memory; 16384 (128 KiB, one per CU) in propagation-blocking mode, where it only ever reads LDS.
    // (round 4, second session: 18 Ki staged values beside 18 Ki column bands on ONE rank from 4 Mi vertices -- 10 M-vertex graph
    //  SpMV - 1.9 % in two parity-controlled sweeps, profiles/r4_wide_band.txt; the 1 M-vertex graph loses 2.5 % with more staged
    //  values and keeps 16 Ki of them)
    u64 hub = (in.hub_opt >= 0) ? (u64)in.hub_opt : (P.pb ? (world == 1 && !in.force_multi && n >= (4u << 20) ? LZX_PB_CB_WIDE : 16384) : 8192);
    hub = std::min<u64>(hub, n);
    hub = std::min<u64>(hub, 20000);  // 160 KiB LDS per CU
    hub &= ~1ull;
    if (hub == 0 || hub >= n) P.pb = false;   // nothing staged, or everything staged: nothing to block
    P.hub_real = (u32)hub;
    P.hub = (u32)hub + (P.pb ? 2 : 0);       // PB mode: two zero slots behind the staged values (padding target)
    P.spmv_lds = lzx_plan_spmv_lds(P.hub);
    return nullptr;
}

// How many of the highest degrees the 1 % rule of lzx_plan_ranked wants summed (0: the rule does not apply).
inline u32 lzx_plan_hub_share_rows(const lzx_plan &P)
{
    return (P.pb && P.in.hub_opt < 0 && P.in.nnz > 0) ? (u32)std::min<u64>(P.hub_real, P.in.n) : 0;
}

// Behind the degree ranking: n_active vertices have an edge, the largest degree is max_degree, and the lzx_plan_hub_share_rows(P)
// highest degrees add up to hub_share.
inline void lzx_plan_ranked(lzx_plan &P, u64 n_active, u32 max_degree, u64 hub_share)
{
    const lzx_plan_in &in = P.in;
    const u64 n = in.n;
    const u32 world = in.world, rank = in.rank;
    P.max_degree = max_degree;
    P.n_active = n_active;
    // How many x values to stage is a per-GRAPH choice, not a per-size one (round 3): on a uniform graph the 16 Ki
    // highest-degree columns hold next to nothing (Erdos-Renyi, 10 M vertices / 200 M entries: 0.25 % of the entries), yet
    // the staged-columns kernel still sweeps every row for them, and 16 Ki fewer columns are what the blocked passes
    // would have taken anyway.  Measured (profiles/r3_er_probe.txt, SpMV ms with 16384 / 1024 staged): ER 10 M 1.31 /
    // 1.05, ER 4 M 0.474 / 0.437, ER 1 M (2.5 % of the entries staged) 0.102 / 0.109; R-MAT (31 %) needs them all.
    // Rule: below 1 % of the entries in the staged columns, stage 1 Ki.  Every rank holds the whole graph and computes
    // the same share, so all ranks agree without talking.
    if (lzx_plan_hub_share_rows(P) && hub_share * 100 < in.nnz && n > 2048) {
        P.hub_real = 1024;
        P.hub = P.hub_real + 2;
        P.spmv_lds = lzx_plan_spmv_lds(P.hub);
    }
    const u64 live = n_active > rank ? (n_active - rank + world - 1) / world : 0;
    P.rows_live = std::min<u32>(P.n_loc_pad, round_up((u32)live, LZX_SLICE));
    // Only vertices with at least one edge are ever gathered by an SpMV, and (degree-sorted, dealt round-robin)
    // they are a prefix of every rank's slice: the per-iteration exchange moves just that prefix.  (R-MAT: 41 % of
    // the 10 M-vertex benchmark graph is isolated.)  One rank exchanges nothing and gathers from the basis itself.
    if (world > 1) {
        P.xs = std::max<u32>(LZX_SLICE, round_up((u32)((n_active + world - 1) / world), LZX_SLICE));
        P.xs = std::min(P.xs, P.n_loc_pad);
        P.xlen = (u64)world * P.xs + LZX_TAIL;
    }
    // Two chunks (see lzx_internal.h: xs0) when the blocked SpMV will run on several ranks: chunk 0 is the first eighth
    // of every slice, rounded so that chunk 0 ends on a column-band boundary, and must hold the LDS-staged hub entries.
    P.xs0 = P.xs;
    P.overlap = false;
    P.xfp32 = (world > 1 || in.force_multi) && in.xfp32_opt > 0;   // N4: fp32 exchange uses the single all-gather
    // (over RCCL only on request: the two-chunk exchange with its sparse second chunk -- a grouped ncclSend / ncclRecv on
    //  the exchange stream -- has never run on two or more physical GPUs; bench.py asks for it in its guarded tuning
    //  phase.  In-process groups take it by default: every form of it is covered there, tests/test_gpu_parity.py.)
    const bool overlap_wanted = in.overlap_opt > 0 || (in.overlap_opt < 0 && in.comm_kind != 2);
    if ((world > 1 || in.force_multi) && P.pb && overlap_wanted && !P.xfp32) {
        // (rounded to the column band the blocked passes will take -- lzx_pb.hip: 18 Ki unless 16 Ki is forced or x is small)
        const u32 band = (in.pb_cb_opt == 8192 || in.pb_cb_opt == 16384 || P.xlen * sizeof(double) <= (16u << 20)) ? LZX_PB_CB : LZX_PB_CB_WIDE;
        u32 x0 = round_up(std::max<u32>(P.xs / 8, (P.hub_real + world - 1) / world), band);
        if (x0 < P.xs) {
            P.xs0 = x0;
            P.overlap = true;
        }
    }
    if (P.hub_real > n_active) {
        // staged slots beyond the vertices that have edges would never be referenced (and, with several ranks, would
        // lie outside the exchanged prefix)
        P.hub_real = (u32)(n_active & ~1ull);
        if (P.hub_real == 0) P.pb = false;
        P.hub = P.hub_real + (P.pb ? 2 : 0);
        P.spmv_lds = lzx_plan_spmv_lds(P.hub);
    }
    if (P.hub_real >= n_active) P.pb = false;   // every referenced column is staged: nothing left to block
    if (!P.pb) {
        P.xs0 = P.xs;
        P.overlap = false;
    }
    // step 1a: ties of the degree ranking broken by the staged-column count; step 1b: the sparse exchange of chunk 1
    P.tie_sort = P.pb && n_active > P.hub_real && in.tie_sort_opt != 0;
    P.try_sparse = P.overlap && (world > 1 || in.force_multi) && in.sparse_opt != 0 && P.xs > P.xs0;
    P.sentinel = P.pb ? P.hub_real : P.hub + (u32)((u64)world * P.xs);
}

// The sparse form of the exchange layout: [world][xs0] (chunk 0, dense), then this rank's packed chunk 1 of xc1 values.
inline u64 lzx_plan_sparse_xlen(u32 world, u32 xs0, u64 xc1) { return (u64)world * xs0 + round_up((u32)xc1, LZX_SLICE) + LZX_TAIL; }

// What travels is agreed on by CONTENT, not only by length (round 5, ADVICE r4: with the sharded hand-over the send lists come
// from this rank's own rows through the matrix's symmetry, so a caller's CSR that is not symmetric could give lists of the
// right lengths and the wrong members): one order-dependent 64-bit hash per peer of what this rank packs for it and of
// what it expects from it, compared pairwise beside the counts (lzx_comm_check_sparse; in-process groups: lzx_api.hip).
inline void lzx_plan_sx_hashes(u32 world, u32 n_loc_pad, const std::vector<u32> &send_off, const std::vector<u32> &recv_off,
                               const std::vector<u32> &h_idx, const std::vector<u32> &h_map, std::vector<u64> &send_hash,
                               std::vector<u64> &recv_hash)
{
    send_hash.assign(world, 0);
    recv_hash.assign(world, 0);
    for (u32 p = 0; p < world; ++p) {
        u64 hs = 0, hr = 0;
        for (u32 i = send_off[p]; i < send_off[p + 1]; ++i) hs += lzx_mix64((u64)h_idx[i] + ((u64)(i - send_off[p]) << 32));
        for (u32 i = recv_off[p]; i < recv_off[p + 1]; ++i)
            hr += lzx_mix64((u64)(h_map[i] - p * n_loc_pad) + ((u64)(i - recv_off[p]) << 32));
        send_hash[p] = hs;
        recv_hash[p] = hr;
    }
}

// ---- step 3. host: split rows / slices (local rows are sorted by degree, descending) ----
// degl[n_loc_pad]: per local row its degree (plain mode) or its count of staged columns (blocked mode); padding rows 0.
inline void lzx_plan_rows(lzx_plan &P, const std::vector<u32> &degl)
{
    const lzx_plan_in &in = P.in;
    lzx_row_plan &R = P.rows;
    // blocked mode: the tables hold staged columns only and a lane's packets come from LDS-only sums, so wider slices
    // cost less than more split-row items: 256 staged entries per row -- and 1024 where a wavefront has many slices to
    // even out the long ones (from 2 Mi rows with an edge per rank).  Round 4, parity-controlled A/B (every configuration in
    // both process states, profiles/r4_long_row.txt): 10 M vertices 0.572 -> 0.556 ms per SpMV (768: 0.551; 512 and
    // 1536: - 1 %), 4 M vertices 0.213 -> 0.206; the 1 M-vertex graph (2.5 slices per wavefront) LOSES with wider slices
    // (512: + 4 %, 1024: + 42 %: a wavefront's one long slice is the launch's tail), hence the size rule.
    R.long_thr = in.long_row_opt > 0 ? (u32)in.long_row_opt
                 : (P.pb ? (P.rows_live >= (1u << 21) ? 8 * LZX_LONG_ROW : 2 * LZX_LONG_ROW) : LZX_LONG_ROW);
    u32 n_long = 0;
    for (u32 l = 0; l < P.n_loc_real; ++l)
        if (degl[l] > R.long_thr) n_long = l + 1;
    R.n_long_true = n_long;
    R.n_long64 = std::min(round_up(n_long, LZX_SLICE), P.n_loc_pad);
    R.n_slices = (P.n_loc_pad - R.n_long64) / LZX_SLICE;

    R.h_long_ptr.assign((size_t)R.n_long64 + 1, 0);
    R.h_item_first.assign((size_t)R.n_long64 + 1, 0);
    R.h_item_beg.clear();
    R.h_item_len.clear();
    for (u32 r = 0; r < R.n_long64; ++r) {
        const u32 dp = round_up(degl[r], 4);
        R.h_long_ptr[r + 1] = R.h_long_ptr[r] + dp;
        R.h_item_first[r] = (u32)R.h_item_beg.size();
        const u32 item_cap = in.item_opt > 0 ? (u32)in.item_opt : LZX_ITEM;
        for (u32 b = 0; b < dp; b += item_cap) {
            R.h_item_beg.push_back(R.h_long_ptr[r] + b);
            R.h_item_len.push_back(std::min(item_cap, dp - b));
        }
    }
    R.h_item_first[R.n_long64] = (u32)R.h_item_beg.size();
    R.n_items = (u32)R.h_item_beg.size();
    R.long_elems = R.h_long_ptr[R.n_long64];

    R.h_slice_off.assign(R.n_slices, 0);
    R.h_slice_w.assign(R.n_slices, 0);
    u64 off = 0;
    for (u32 s = 0; s < R.n_slices; ++s) {
        u32 widest = 0;  // rows are degree-sorted, but in PB mode `degl` counts hub entries only: take the max
        for (u32 l = 0; l < LZX_SLICE; ++l) widest = std::max(widest, degl[R.n_long64 + s * LZX_SLICE + l]);
        const u32 w = round_up(widest, 4);
        R.h_slice_off[s] = off;
        R.h_slice_w[s] = w;
        off += (u64)w * LZX_SLICE;
    }
    R.sell_elems = off;
}

// processing order of the slices: by class in blocked mode (k_spmv), as they lie otherwise
inline void lzx_plan_slice_order(lzx_plan &P)
{
    const lzx_plan_in &in = P.in;
    lzx_row_plan &R = P.rows;
    R.perm.clear();
    R.perm.reserve(R.n_slices);
    R.h_slice_w0.clear();
    // classes pay from a few slices per wavefront on (each class loop starts with its own descriptor round trips:
    // on the 1 M-vertex graph, 2.4 slices per wavefront, they cost 1.6 us)
    R.classes = P.pb && in.narrow_opt != 0 && (in.narrow_opt > 0 || R.n_slices >= 8u * in.cu_count * (LZX_SPMV_BLOCK / 64));
    for (u32 s2 = 0; s2 < R.n_slices; ++s2)
        if (!R.classes || R.h_slice_w[s2] > 8) R.perm.push_back(s2);
    R.ns_wide = (u32)R.perm.size();
    for (u32 s2 = 0; R.classes && s2 < R.n_slices; ++s2)
        if (R.h_slice_w[s2] == 8) R.perm.push_back(s2);
    R.ns_w8 = (u32)R.perm.size() - R.ns_wide;
    for (u32 s2 = 0; R.classes && s2 < R.n_slices; ++s2)
        if (R.h_slice_w[s2] == 4) R.perm.push_back(s2);
    R.ns_w4 = (u32)R.perm.size() - R.ns_wide - R.ns_w8;
    for (u32 s2 = 0; R.classes && s2 < R.n_slices; ++s2)
        if (R.h_slice_w[s2] == 0) { R.perm.push_back(s2); R.h_slice_w0.push_back(s2); }
}

// step 5, the launch shape: persistent workgroups, as many as stay resident (LDS-limited), never more than
// there is work for.
inline void lzx_plan_grid(lzx_plan &P)
{
    const lzx_plan_in &in = P.in;
    lzx_row_plan &R = P.rows;
    // 4 workgroups per CU: two are resident at the default 64 KiB of staged x, the rest queue behind them, which evens
    // out the tail (measured: C3 2.16 -> 2.15 ms, C2 0.141 -> 0.133 ms against exactly-resident grids).
    // In propagation-blocking mode the kernel stages 128 KiB per workgroup and only one is resident: one per CU.
    R.per_cu = P.pb ? 1 : 4;
    if (in.wgs_per_cu_opt > 0) R.per_cu = (u32)in.wgs_per_cu_opt;
    const u32 units = R.n_slices + R.n_items;
    const u32 waves_per_wg = LZX_SPMV_BLOCK / 64;
    u32 grid = in.cu_count * R.per_cu;
    grid = std::min(grid, std::max(1u, (units + waves_per_wg - 1) / waves_per_wg));
    // Blocked mode, little staged-columns work per workgroup (below 512 slices + items each: graphs up to a few million vertices,
    // rank shares from P = 2): half as many, twice as long.  They share the scatter pass's launch; the CUs they leave free start on scatter units
    // at once, and 128 KiB of staged x are fetched half as often (1 M-vertex graph: SpMV 0.0652 -> 0.0595 ms; rank 0 of 8 / of 4:
    // 0.109 -> 0.100, 0.179 -> 0.173 ms; 4 M vertices and rank 0 of 2: - 2 %; neutral on the 10 M-vertex graph -- profiles/r3_small_units.txt)
    if (P.pb && units < in.cu_count * 512u) grid = std::min(grid, std::max(1u, in.cu_count / 2));
    if (in.spmv_wgs_opt > 0) grid = std::min<u32>(in.cu_count * R.per_cu, std::min<u32>(std::max(1u, (units + waves_per_wg - 1) / waves_per_wg), (u32)in.spmv_wgs_opt));   // test shape spmv_wgs
    R.spmv_grid = grid;
    R.fin_grid = (R.n_long64 + LZX_VEC_BLOCK - 1) / LZX_VEC_BLOCK;
}
