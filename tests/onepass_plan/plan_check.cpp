// The host-only planning of the one-pass connected-word decoder (csrc/sr_onepass_plan.h) on the CPU, without a device: the
// block length L, the word-cost bound, the block list and the launch groups, over random stores, frame bounds and hook values
// against a brute-force restatement -- the blocks tile [0, cap) in order, none is longer than L, each resumes where the last one
// began; a word that starts inside a block cannot end inside it (checked frame by frame from the reach rule); every column is
// swept by the block that holds it and, unless it is a block's first, by the next one; the groups' scratch stays within 256 MiB.
// A stand-alone program for the sanitizers:
//   hipcc --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I<csrc> plan_check.cpp -o plan_check && ./plan_check
// (tests/test_onepass_ref.py builds and runs it).  Prints "plan_check ok" and returns 0, or says what failed and returns 1.
#include <cstdio>

#include "sr_onepass_plan.h"

using namespace sr;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("plan_check: line %d: %s\n", __LINE__, #cond);     \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static uint32_t rnd(uint64_t &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
}

// brute force, from the definitions: the fewest input frames of a word over a template of M frames -- every horizontal or
// vertical step directly after a diagonal one, so of the M - 1 row advances at most every second one is vertical
static uint32_t fewest_frames(uint32_t M)
{
    uint32_t frames = 1, row = 0;
    bool diag_last = false;
    while (row + 1 < M) {
        if (diag_last) row++, diag_last = false;       // vertical: no new frame
        else row++, frames++, diag_last = true;        // diagonal: one new frame
    }
    return frames;
}

static int check_case(const std::vector<uint32_t> &len, uint32_t tpl_len, uint32_t max_frames, uint32_t frames_cap, uint32_t block, uint32_t rows,
                      uint32_t word_cost)
{
    const uint32_t K = (uint32_t)len.size();
    uint32_t L = 0;
    for (uint32_t m : len)
        if (m && (!L || fewest_frames(m) < L)) L = fewest_frames(m);
    CHECK(onepass_reach(len.data(), K) == L);
    const OnePassPlan p = onepass_plan(tpl_len, K, max_frames, frames_cap, L, block, rows);
    const uint32_t cap = frames_cap && frames_cap < max_frames ? frames_cap : max_frames;
    CHECK(p.cap == cap && p.L == L && p.n >= 1);
    if (L) {
        CHECK(p.n <= L && p.n == (block ? (block < L ? block : L) : L));
    } else {
        CHECK(p.blocks.size() == 1);
    }
    // the word-cost bound in u64, word by word
    uint64_t sum = 0;
    for (uint32_t at = 0; L && at + L <= cap; at += L) sum += word_cost;
    CHECK(onepass_cost_ok(cap, L, word_cost) == (sum <= (1ull << 30)));
    // the blocks tile [0, cap) in order
    std::vector<uint32_t> swept(cap, 0u);
    uint32_t at = 0;
    for (size_t b = 0; b < p.blocks.size(); b++) {
        const OnePassBlock &o = p.blocks[b];
        CHECK(o.c0 == at && o.cN > o.c0 && o.cN <= cap && o.cN - o.c0 <= p.n);
        CHECK(b + 1 == p.blocks.size() ? o.cN == cap : o.cN - o.c0 == p.n);
        CHECK(b ? o.c0_prev == p.blocks[b - 1].c0 : o.c0_prev == 0);
        for (uint32_t x = b ? o.c0_prev + 1 : 0; x < o.cN; x++) swept[x]++;
        // a word that starts behind c0 inside the block ends at or after cN: its key is not wanted before the next block
        for (uint32_t s = o.c0 + 1; L && s < o.cN; s++) CHECK(s + L - 1 >= o.cN);
        at = o.cN;
    }
    CHECK(at == cap && p.launches == 2 * p.blocks.size() + 2);
    for (size_t b = 0; b < p.blocks.size(); b++)
        for (uint32_t x = p.blocks[b].c0; x < p.blocks[b].cN; x++)
            CHECK(swept[x] == (x == p.blocks[b].c0 || b + 1 == p.blocks.size() ? 1u : 2u));
    // scratch
    const size_t row_bytes = ((size_t)max_frames + 1) * 12 + (size_t)K * tpl_len * 16;
    CHECK(p.row_bytes == row_bytes && p.a_row == (size_t)max_frames + 1 && p.e_row == p.a_row && p.col_row == (size_t)K * tpl_len);
    CHECK(p.rows >= 1 && p.rows <= kOnePassMaxRows);
    if (rows) {
        CHECK(p.rows == (rows < kOnePassMaxRows ? rows : kOnePassMaxRows));
    } else {
        CHECK(p.rows == 1 || (size_t)p.rows * row_bytes <= kOnePassScratch);
        CHECK(p.rows == kOnePassMaxRows || (size_t)(p.rows + 1) * row_bytes > kOnePassScratch);
    }
    return 0;
}

int main()
{
    for (uint32_t M = 1; M < 300; M++)
        if (fewest_frames(M) != M / 2 + 1) {
            std::printf("plan_check: the reach rule fails at M = %u\n", M);
            return 1;
        }
    uint64_t s = 20261019;
    for (int it = 0; it < 4000; it++) {
        const uint32_t K = 1 + rnd(s) % 12, tpl_len = 1 + rnd(s) % 200;
        std::vector<uint32_t> len(K);
        for (uint32_t &m : len) m = rnd(s) % 4 == 0 ? 0u : 1 + rnd(s) % tpl_len;
        const uint32_t max_frames = 2 + rnd(s) % (it % 16 ? 700 : 16382);
        const uint32_t frames_cap = rnd(s) % 3 == 0 ? 0u : 1 + rnd(s) % (max_frames + 50);
        const uint32_t block = rnd(s) % 2 ? 0u : 1 + rnd(s) % 120, rows = rnd(s) % 3 ? 0u : 1 + rnd(s) % 70000;
        const uint32_t word_cost = rnd(s) % 4 ? rnd(s) % ((1u << 24) + 1) : 1u << 24;
        if (check_case(len, tpl_len, max_frames, frames_cap, block, rows, word_cost)) {
            std::printf("plan_check: case %d failed\n", it);
            return 1;
        }
    }
    // a store as large as they come: one row does not fit 256 MiB, the plan still gives one row per group
    if (check_case(std::vector<uint32_t>(65536, 1300u), 1300, 16383, 0, 0, 0, 7)) return 1;
    std::printf("plan_check ok\n");
    return 0;
}
