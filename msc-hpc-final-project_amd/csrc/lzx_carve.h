// lzx_carve.h -- one layout list per arena.  A routine writes its arena once, as a list of take() lines, and the list is walked
// twice: over a null base it counts the bytes, over the allocation it hands out the pointers.  The size and the pointers come from
// the same lines, so they cannot disagree.  Host only, and nothing of HIP or of the project in it: a plain C++ program can include
// it (tests/carve_check.cc).  lzx_carve_state (lzx_graph_call.h) is what the graph routines call.
#pragma once

#include <cstddef>
#include <cstdint>

// a count of 4-byte words after which an 8-byte piece is aligned
inline uint64_t lzx_even(uint64_t count) { return (count + 1) & ~1ull; }

struct LzxCarver {
    char *base;                    // null: the counting pass
    uint64_t at = 0;               // bytes taken so far
    uint64_t state = UINT64_MAX;   // at, where end_of_state() was called; until then everything taken is state
    bool misaligned = false;       // a take() found `at` off its type's alignment
    explicit LzxCarver(void *base_ = nullptr) : base(static_cast<char *>(base_)) {}

    // p = the next count elements.  No padding is added: the list says where it rounds (lzx_even, align)
    template <typename T>
    void take(T *&p, uint64_t count)
    {
        if (at % alignof(T)) misaligned = true;
        p = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at += count * sizeof(T);
    }
    // a piece that exists only where it is wanted: otherwise null, and nothing is taken
    template <typename T>
    void take_if(bool wanted, T *&p, uint64_t count)
    {
        if (wanted) take(p, count);
        else p = nullptr;
    }
    // bytes of no type (a library's scratch)
    void take_bytes(void *&p, uint64_t bytes)
    {
        p = base ? base + at : nullptr;
        at += bytes;
    }
    // the next piece begins at a multiple of `to` bytes
    void align(uint64_t to) { at = (at + to - 1) / to * to; }
    // what is taken after this is allocated with the state but is not counted in state_bytes (scratch of a size the library
    // does not choose)
    void end_of_state() { state = at; }
    uint64_t state_bytes() const { return state == UINT64_MAX ? at : state; }
    // the carving pass took what the counting pass counted, every piece aligned
    bool agrees_with(const LzxCarver &counted) const
    {
        return !misaligned && !counted.misaligned && at == counted.at && state_bytes() == counted.state_bytes();
    }
};
