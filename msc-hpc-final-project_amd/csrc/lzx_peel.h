// lzx_peel.h -- the push peeling that lzx_core_numbers (lzx_core.hip, over vertices) and lzx_truss (lzx_truss.hip, over edges)
// share: DESIGN.md section 19.  An item is a vertex or an edge.  count[x] is its remaining degree or support, mark[x] is 0 while
// it remains and else the round that removes it, value[x] is the number it leaves with, and `queue` holds every item exactly
// once over the whole call, so that a round's frontier is a window [beg, end) of it and what a launch appends behind `end` is
// the next window.  counters[0] is the queue's end, counters[1] the minimum of a level start.
//   level start  k_peel_level    one thread per item, when the frontier is empty: an unmarked item with count <= level is marked
//                                (mark = r, value = value_at_level) and appended, the others contribute to a minimum
//   push         lzx_peel_push   one decrement of a caller's peel kernel: old = atomicSub(&count[x], 1), and the one lane that
//                                sees old == level + 1 takes the mark (r + 1) by a compare-and-swap, writes the value and appends x
//   the loop     lzx_peel_loop   the host's: level starts and rounds until every item is queued
// An item is marked when its count is at most `level`, so a later decrement of it returns at most `level`, never level + 1,
// while the level lasts: it is appended once.  The compare-and-swap and the clamp of every queue write keep that, and the
// queue's end, inside the `items` entries whatever the counters hold (a matrix that is not symmetric).
// The kernel is compiled into each file that includes this header (internal linkage, as k_tri_degrees).
#pragma once

#include "lzx_internal.h"
#include "lzx_graph_call.h"

static constexpr u32 LZX_PEEL_BLOCK = 256;
static constexpr u32 LZX_PEEL_SLICES = 64;   // workgroups a long row's entries are dealt to (at most)
static constexpr u32 LZX_PEEL_NONE = 0xffffffffu;

// workgroups per long row of a peel's long-row launch, which deals runs of `block` entries: a quarter of the runs of the longest row
inline u32 lzx_peel_slices(u64 max_degree, u32 block) { return (u32)std::min<u64>(std::max<u64>(max_degree / (4 * block), 1), LZX_PEEL_SLICES); }

// counters[1] = LZX_PEEL_NONE before the launch
static __global__ void __launch_bounds__(LZX_PEEL_BLOCK)
k_peel_level(const u32 *count, u32 *mark, u32 *value, u32 *queue, u32 *counters, u32 items, u32 level, u32 value_at_level, u32 r)
{
    const u64 x = (u64)blockIdx.x * LZX_PEEL_BLOCK + threadIdx.x;
    bool take = false;
    u32 least = LZX_PEEL_NONE;
    if (x < items && mark[x] == 0) {
        const u32 t = count[x];
        if (t <= level) take = true;
        else least = t;
    }
    const u32 at = lzx_wave_append(take, &counters[0]);
    if (take) {
        mark[x] = r;
        value[x] = value_at_level;
        if (at < items) queue[at] = (u32)x;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) least = min(least, (u32)__shfl_xor((int)least, o, 64));
    if ((threadIdx.x & 63) == 0 && least != LZX_PEEL_NONE) atomicMin(&counters[1], least);
}

// one decrement (have: this lane holds one), the mark, the append.  Every lane of the wavefront calls it together.
__device__ __forceinline__ void lzx_peel_push(bool have, u32 x, u32 *count, u32 *mark, u32 *value, u32 *queue, u32 *tail, u32 items, u32 level,
                                              u32 value_at_level, u32 r)
{
    bool take = false;
    if (have) {
        const u32 old = atomicSub(&count[x], 1u);
        if (old == level + 1) take = atomicCAS(&mark[x], 0u, r + 1) == 0u;
    }
    const u32 at = lzx_wave_append(take, tail);
    if (take) {
        value[x] = value_at_level;
        if (at < items) queue[at] = x;
    }
}

// the words of the two LZX_ERR_LIMIT messages: "vertex" / "remaining degree" / "vertices", "edge" / "remaining support" / "edges"
struct LzxPeelNouns {
    const char *item, *count, *items;
};

struct LzxPeelResult {
    u32 level = 0;         // the last level
    u32 levels = 0, rounds = 0;
    u32 level_pos = 0;     // the queue position at which the last level began
    u32 first_level = 0;   // the first level, and the queue's end after its start
    u32 first_end = 0;
};

// The whole peel of `items` items.  level_start(level_try, r) launches k_peel_level for round r; round(wbeg, wlen, level, r)
// launches the caller's peel kernels over the window queue[wbeg .. wbeg + wlen).  Both return LZX_OK or the error.  The host reads
// one word per round (the queue's end) and two per level start (the end and the minimum).
template <typename LevelStart, typename Round>
int lzx_peel_loop(const char *fn_name, const LzxPeelNouns &nouns, hipStream_t st, u32 *d_counters, u32 items, LevelStart level_start, Round round,
                  LzxPeelResult *res)
{
    u32 level = 0, rounds = 0, levels = 0;
    u32 queued = 0;   // the queue's end: items marked so far
    while (queued < items) {
        // ---- the frontier is empty: the next level.  level + 1 first (0 at the start); the minimum if that appends nothing ----
        u32 level_try = levels == 0 ? 0u : (level == LZX_PEEL_NONE ? level : level + 1);
        u32 end = queued;
        for (int attempt = 0; attempt < 2 && end == queued; ++attempt) {
            u32 words[2] = {0, 0};
            LZX_HIP(hipMemsetAsync(d_counters + 1, 0xff, sizeof(u32), st));
            LZX_TRY(level_start(level_try, rounds + 1));
            LZX_HIP(hipMemcpyAsync(words, d_counters, sizeof(words), hipMemcpyDeviceToHost, st));
            LZX_HIP(hipStreamSynchronize(st));
            end = std::min(words[0], items);
            if (end == queued) level_try = words[1];   // nobody at this level: the smallest remaining count is the next
        }
        if (end == queued)
            LZX_FAIL(LZX_ERR_LIMIT, "%s: no %s of %s %u among the %u left after %u rounds", fn_name, nouns.item, nouns.count, level_try, items - queued, rounds);
        level = level_try;
        if (levels == 0) {
            res->first_level = level;
            res->first_end = end;
        }
        ++levels;
        res->level_pos = queued;
        u32 wbeg = queued;
        queued = end;
        // ---- the rounds of this level: window [wbeg, queued) ----
        for (;;) {
            ++rounds;
            if ((u64)rounds > (u64)items + 1) LZX_FAIL(LZX_ERR_LIMIT, "%s: %u rounds on %u %s", fn_name, rounds, items, nouns.items);
            if (queued >= items) break;   // everything is queued: the last window has nobody left to push to
            LZX_TRY(round(wbeg, queued - wbeg, level, rounds));
            u32 word = 0;
            LZX_HIP(hipMemcpyAsync(&word, d_counters, sizeof(u32), hipMemcpyDeviceToHost, st));
            LZX_HIP(hipStreamSynchronize(st));
            end = std::min(word, items);
            if (end == queued) break;   // nothing fell to the level: the level is peeled out
            wbeg = queued;
            queued = end;
        }
    }
    res->level = level;
    res->levels = levels;
    res->rounds = rounds;
    return LZX_OK;
}
