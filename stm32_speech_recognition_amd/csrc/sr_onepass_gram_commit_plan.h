// What a commit call of a live one-pass grammar decoding session (sr_onepass_gram_live.cpp, sr_onepass_gram_live_commit[_dev])
// decides on the host before anything reaches the device: the window of the commit rule from the grammar's kept items, the
// kernel's block and ring, and the rows of a channel list.  The list is the live one-pass decoder's
// (sr_onepass_live_plan.h: one row per distinct channel at its first mention, with the frames the mirror holds) under the
// grammar sessions' binding: the mirror stands on one constant serial, and a stale grammar refuses the call before the list
// is looked at.
// HOST ONLY, and free of HIP calls: tests/onepass_gram_commit_plan/plan_check.cpp runs it on the CPU under the sanitizers.
#pragma once
#include "sr_gram_live_plan.h"
#include "sr_onepass_live_plan.h"

namespace sr {

// W = 2 * max M_k - 1 over the slots of the kept items -- a word over M template frames covers at most 2M - 1 input frames --
// with item_slot[i] the slot of kept item i and tpl_len[k] the frames of a valid slot, 0 for an invalid one (a grammar keeps
// items of valid slots only; a slot past the store counts as invalid).  0: nothing is kept
inline uint32_t onepass_gram_commit_window(const uint32_t *item_slot, uint32_t n_items, const uint32_t *tpl_len, uint32_t K)
{
    uint32_t longest = 0;
    for (uint32_t i = 0; i < n_items; i++)
        if (item_slot[i] < K) longest = std::max(longest, tpl_len[item_slot[i]]);
    return longest ? 2u * longest - 1u : 0u;
}

// The kernel sweeps the positions downwards in blocks and keeps the marks of the positions not yet swept in an LDS ring of u64
// (k_onepass_gram_live.hip).  A block holds at most 64 positions (a lane each) and at most L = reach of the store: a word covers
// at least L frames, so what a node of a block leads to lies below the block.  The ring holds a block and the W positions
// below it, rounded up to a power of two for the index mask: at most 8 x 2 x (W + 64) bytes.
inline uint32_t onepass_gram_commit_block(uint32_t L) { return std::min(std::max(L, 1u), 64u); }
inline uint32_t onepass_gram_commit_ring(uint32_t W)
{
    uint32_t ring = 64;
    while (ring < W + 64u) ring <<= 1;  // W <= 2 x 16 383 - 1: no overflow
    return ring;
}

// the rows of a commit list.  stale: the session's grammar is stale (why_stale says how): refused first, as a push is.  The
// mirror is not changed.
inline bool onepass_gram_commit_list(const OnePassLiveMirror &m, bool stale, const std::string &why_stale, const uint32_t *channels, uint32_t n_ch,
                                     std::vector<sr_chain_live_row> *order, std::string *why)
{
    order->clear();
    if (stale) {
        *why = why_stale;
        return false;
    }
    return onepass_live_commit_list(m, kGramLiveBound, channels, n_ch, order, why);
}

}  // namespace sr
