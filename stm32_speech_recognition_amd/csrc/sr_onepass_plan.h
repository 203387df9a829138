// sr_onepass_plan.h -- host-side planning of the one-pass connected-word decoder (include/sr_engine.h, "one-pass connected-word
// decoding"; sr_onepass.cpp): the block length L from the store's valid template lengths, the word-cost bound, the list of
// blocks and the launch groups.  HOST ONLY and free of HIP, so that tests/onepass_plan/plan_check.cpp can run it under the
// sanitizers on a machine without a device.
//
// The block argument.  A word over a template of M frames spans at least M / 2 + 1 input frames (the span section's reach rule,
// sr_forced_plan.h's minlen), so a word that STARTS at frame s ends at frame s + L - 1 at the earliest, L = min over the valid
// slots of M / 2 + 1.  A(p) -- the best word that ends at frame p - 1 -- therefore depends on E(s) for s <= p - L only, and for
// a block of n <= L positions (c0, c0 + n] every A(p) and E(p) of the block follows from E at or before c0: the blocks are
// ordered by the stream alone, and inside a block all rows and slots run in parallel.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sr {

constexpr size_t kOnePassScratch = (size_t)256 << 20;  // bytes of scratch per launch group at most
constexpr uint32_t kOnePassMaxRows = 65535u;           // rows of a launch group (four per workgroup of the sweep: the grid's y)
constexpr uint64_t kOnePassWordCostSum = 1ull << 30;   // (frames_cap / L) * word_cost at most: with it every cost stays below 2^32 - 1

// L: min over the valid slots of M / 2 + 1; tpl_len[k] = the frames of a valid slot, 0 for an invalid one.  0: no valid slot
inline uint32_t onepass_reach(const uint32_t *tpl_len, uint32_t K)
{
    uint32_t L = 0;
    for (uint32_t k = 0; k < K; k++) {
        if (!tpl_len[k]) continue;
        const uint32_t reach = tpl_len[k] / 2u + 1u;
        L = L && L < reach ? L : reach;
    }
    return L;
}

// a row of cap frames holds at most cap / L words: their word costs together stay within 2^30 (L = 0: no word at all)
inline bool onepass_cost_ok(uint32_t cap, uint32_t L, uint32_t word_cost)
{
    return !L || (uint64_t)(cap / L) * word_cost <= kOnePassWordCostSum;
}

// one block of frames [c0, cN): k_onepass_words resumes from the column saved at c0_prev (block 0 starts fresh: c0_prev is not
// read) and sweeps the columns (c0_prev, cN), k_onepass_close gives E over (c0, cN]
struct OnePassBlock {
    uint32_t c0_prev, c0, cN;
};

struct OnePassPlan {
    uint32_t cap = 0;       // frames of a row at most: min(max_frames, frames_cap), frames_cap 0 = max_frames
    uint32_t L = 0;         // as given (0: no valid slot)
    uint32_t n = 0;         // the block length, 1..max(L, 1) -- or cap when there is no valid slot: nothing depends on anything
    size_t a_row = 0, e_row = 0, col_row = 0;  // elements per row: u64 keys, u32 prefix costs, 16-byte column entries
    size_t row_bytes = 0;
    uint32_t rows = 0;      // per launch group
    uint32_t launches = 0;  // per launch group: init, two per block, trace
    std::vector<OnePassBlock> blocks;
};

// tpl_len = the longest template of the store (rows of a saved column), max_frames >= 1; block / forced_rows: the testing hooks, 0 = default
inline OnePassPlan onepass_plan(uint32_t tpl_len, uint32_t K, uint32_t max_frames, uint32_t frames_cap, uint32_t L, uint32_t block,
                                uint32_t forced_rows)
{
    OnePassPlan p;
    p.cap = frames_cap && frames_cap < max_frames ? frames_cap : max_frames;
    p.L = L;
    p.n = L ? L : p.cap;
    if (L && block) p.n = block < L ? block : L;  // a block longer than L would be wrong
    if (!p.n) p.n = 1;
    p.a_row = p.e_row = (size_t)max_frames + 1u;
    p.col_row = (size_t)K * tpl_len;
    p.row_bytes = p.a_row * 8u + p.e_row * 4u + p.col_row * 16u;
    const size_t fit = kOnePassScratch / p.row_bytes;
    p.rows = (uint32_t)(fit < 1 ? 1 : fit > kOnePassMaxRows ? kOnePassMaxRows : fit);
    if (forced_rows) p.rows = forced_rows < kOnePassMaxRows ? forced_rows : kOnePassMaxRows;
    for (uint32_t c0 = 0; c0 < p.cap; c0 += p.n) {
        const uint32_t cN = p.cap - c0 < p.n ? p.cap : c0 + p.n;
        p.blocks.push_back(OnePassBlock{c0 ? c0 - p.n : 0u, c0, cN});
    }
    p.launches = 2u * (uint32_t)p.blocks.size() + 2u;
    return p;
}

}  // namespace sr
