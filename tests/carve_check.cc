// carve_check.cc -- csrc/lzx_carve.h on a host buffer, for tests/test_carve_host.py: built with -fsanitize=address,undefined and run
// as a process of its own.  Every list is walked as lzx_carve_state walks it (counted over a null base, then carved from a malloc
// of exactly the counted bytes), and every piece is written to its end, so that a piece past the buffer is AddressSanitizer's
// finding and a piece off its alignment UBSan's.  Prints "carve ok" and returns 0, or says what failed and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lzx_carve.h"

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);  \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

// the pieces a list took, in its order, for the checks on their places
struct Piece {
    char *p;
    uint64_t bytes;
};
static std::vector<Piece> pieces;
template <typename T>
static void piece(LzxCarver &k, T *&p, uint64_t count)
{
    k.take(p, count);
    if (k.base) {
        for (uint64_t i = 0; i < count; ++i) p[i] = T(1);   // written to its end
        pieces.push_back({reinterpret_cast<char *>(p), count * sizeof(T)});
    }
}
template <typename T>
static void piece_if(bool wanted, LzxCarver &k, T *&p, uint64_t count)
{
    if (wanted) piece(k, p, count);
    else {
        const uint64_t before = k.at;
        p = reinterpret_cast<T *>(&failures);   // (anything but null)
        k.take_if(false, p, count);
        CHECK(p == nullptr && k.at == before);
    }
}

// Counts, allocates exactly that, carves, and checks what every list must satisfy: the passes agree, the pieces follow one
// another with no gap but the ones `gaps` allows (an align), the first begins the buffer and the last ends it.
template <typename Layout>
static uint64_t walk(Layout layout, uint64_t gaps_allowed = 0)
{
    LzxCarver counted;
    layout(counted);
    CHECK(!counted.misaligned);
    char *buf = static_cast<char *>(std::malloc(counted.at ? counted.at : 1));
    pieces.clear();
    LzxCarver carved(buf);
    layout(carved);
    CHECK(carved.at == counted.at && carved.agrees_with(counted));
    char *next = buf;
    uint64_t gaps = 0;
    for (const Piece &pc : pieces) {
        CHECK(pc.p >= next);
        gaps += (uint64_t)(pc.p - next);
        next = pc.p + pc.bytes;
    }
    CHECK(gaps <= gaps_allowed);
    CHECK(next == buf + counted.at);   // the last byte of the last piece is the buffer's last
    std::free(buf);
    return counted.at;
}

int main()
{
    // ---- u32 pieces of lzx_even(n) words, then u64: the shape of components, core, colour, propagation, Louvain ----
    CHECK(lzx_even(0) == 0 && lzx_even(1) == 2 && lzx_even(2) == 2 && lzx_even(1001) == 1002);
    for (uint64_t n : {1ull, 2ull, 1001ull}) {
        uint32_t *a, *b, *c;
        uint64_t *d;
        double *e;
        const uint64_t bytes = walk([&](LzxCarver &k) {
            piece(k, a, lzx_even(n));
            piece(k, b, lzx_even(n));
            piece(k, c, lzx_even(n));
            piece(k, d, n);
            piece(k, e, 3);
        });
        CHECK(bytes == 12 * lzx_even(n) + 8 * n + 24);
        // the same list with the counts not rounded: the u64 piece is off its alignment where n is odd, and the list says so
        LzxCarver odd;
        odd.take(a, n);
        odd.take(d, n);
        CHECK(odd.misaligned == (n % 2 == 1));
    }

    // ---- an 8-byte take at an offset of 4 is reported; so is a second pass with one piece more ----
    {
        uint32_t *w;
        double *x;
        LzxCarver k;
        k.take(w, 1);
        CHECK(k.at == 4 && !k.misaligned);
        k.take(x, 1);
        CHECK(k.misaligned && k.at == 12);
        CHECK(!k.agrees_with(k));   // a list with such a piece fails even where its two passes agree
        LzxCarver one, two;
        one.take(w, 2);
        two.take(w, 2);
        CHECK(two.agrees_with(one));
        two.take(w, 1);
        CHECK(!two.agrees_with(one));
    }

    // ---- the five conditional pieces of lzx_paths.hip in their 2^5 combinations ----
    for (unsigned mask = 0; mask < 32; ++mask) {
        const bool third = mask & 1, fourth = mask & 2, bc = mask & 4, ebc = mask & 8, cnt = mask & 16;
        const uint64_t n = 37, B = 2, nnz = 91, parts = 3;
        int32_t *dist;
        double *sigma, *p_third, *p_delta, *p_bc, *p_ebc, *part;
        long long *p_cnt;
        uint32_t *part_row, *reached;
        const uint64_t bytes = walk(
            [&](LzxCarver &k) {
                piece(k, dist, n * B);
                k.align(16);
                piece(k, sigma, n * B);
                piece_if(third, k, p_third, n * B);
                piece_if(fourth, k, p_delta, n * B);
                piece_if(bc, k, p_bc, n);
                piece_if(ebc, k, p_ebc, nnz);
                piece_if(cnt, k, p_cnt, n);
                piece(k, part, parts * B);
                piece(k, part_row, (parts + 3) & ~3ull);   // 16 bytes at a time, wherever it begins
                piece(k, reached, 16);
            },
            /* 4 n B = 296 is followed by 8 bytes */ 8);
        const uint64_t r16 = (4 * n * B + 15) / 16 * 16;
        CHECK(bytes == r16 + 8 * n * B * (1 + third + fourth) + 8 * n * bc + 8 * nnz * ebc + 8 * n * cnt + 8 * parts * B + 16 + 64);
    }

    // ---- align: multiples of 16 and of 256, and nothing where the offset is one already ----
    for (uint64_t bytes = 0; bytes <= 600; ++bytes) {
        LzxCarver k;
        void *p;
        k.take_bytes(p, bytes);
        CHECK(p == nullptr && k.at == bytes);
        k.align(16);
        CHECK(k.at % 16 == 0 && k.at >= bytes && k.at < bytes + 16);
        const uint64_t at16 = k.at;
        k.align(16);
        CHECK(k.at == at16);
        k.align(256);
        CHECK(k.at % 256 == 0 && k.at >= at16 && k.at < at16 + 256);
    }

    // ---- raw bytes behind a 256-byte boundary, outside the state: the shape of lzx_sweep.hip ----
    for (uint64_t n : {1ull, 63ull, 1001ull}) {
        uint32_t *ids;
        uint64_t *keys;
        void *tmp = nullptr;
        uint64_t state = 0;
        const uint64_t tmp_bytes = 777;
        const uint64_t bytes = walk(
            [&](LzxCarver &k) {
                piece(k, keys, n);
                piece(k, ids, lzx_even(n));
                k.end_of_state();
                state = k.state_bytes();
                k.align(256);
                k.take_bytes(tmp, tmp_bytes);
                if (k.base) {
                    std::memset(tmp, 0xff, tmp_bytes);
                    pieces.push_back({static_cast<char *>(tmp), tmp_bytes});
                    CHECK((uint64_t)(static_cast<char *>(tmp) - k.base) % 256 == 0);
                }
            },
            255);
        CHECK(state == 8 * n + 4 * lzx_even(n));
        CHECK(bytes == (state + 255) / 256 * 256 + tmp_bytes);
    }

    if (failures) return 1;
    std::printf("carve ok\n");
    return 0;
}
