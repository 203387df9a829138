// sr_onepass_gram_plan.h -- host-side planning of one-pass grammar decoding (include/sr_engine.h, "one-pass grammar decoding";
// sr_onepass_gram.cpp): which items and states of a compiled grammar the decoder keeps, the cost bound, the scratch of a row
// and, through sr_onepass_plan.h, the blocks and the launch groups.  HOST ONLY and free of HIP, so that
// tests/onepass_gram_plan/plan_check.cpp can run it under the sanitizers on a machine without a device.
//
// The block argument, per state.  A word over a template of M frames spans at least M / 2 + 1 input frames whatever state it
// leads into, so A(p, t) depends on E(x, s) for x <= p - L only, L = min over the valid slots of M / 2 + 1: for a block of
// n <= L positions (c0, c0 + n] every A(p, t) and E(p, t) of the block follows from E at or before c0, of every state.
//
// The pruning is static: one list for the whole call, not one per level.  An item (slot, target) is KEPT when its charge list
// names a state that can be reached from state 0 in any number of arcs and its target reaches a final state.  A state is KEPT
// -- its E row is initialised and closed -- when a kept item's charge list names it or when it is final and can be reached.
// That includes states without an incoming arc: state 0 of a sequence grammar is charged from by the first position's items
// at every block, and with skipping on E(p, 0) = p x skip_cost must exist for them.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "sr_onepass_plan.h"

namespace sr {

constexpr uint64_t kOnePassGramCostSum = 1ull << 30;  // (frames_cap / L) x (word_cost + largest arc cost) + largest final cost at most

// the one-pass bound with one arc per word and one final cost added (L = 0: no word at all)
inline bool onepass_gram_cost_ok(uint32_t cap, uint32_t L, uint32_t word_cost, uint32_t max_arc_cost, uint32_t max_final_cost)
{
    return !L || (uint64_t)(cap / L) * ((uint64_t)word_cost + max_arc_cost) + max_final_cost <= kOnePassGramCostSum;
}

struct OnePassGramKeep {
    uint64_t reach = 0, alive = 0;       // the states reachable from state 0; the states that reach a final state
    std::vector<uint32_t> items, states; // ascending: indices into the grammar's items; state numbers
};

// arcs[i].from / .to, items[i].target / .set (sr_gram_arc and GramItem; templates keep this header free of both), masks[set] =
// the states of charge list `set`, finals = the final states; n_states <= 64.  prune false: everything is kept
template <class Arc, class Item>
inline OnePassGramKeep onepass_gram_keep(uint32_t n_states, const Arc *arcs, uint32_t n_arcs, uint64_t finals, const Item *items, uint32_t n_items,
                                         const unsigned long long *masks, bool prune)
{
    OnePassGramKeep k;
    k.reach = 1ull;
    k.alive = finals;
    for (bool more = true; more;) {  // at most n_states rounds each way
        more = false;
        for (uint32_t a = 0; a < n_arcs; a++) {
            const uint64_t f = 1ull << arcs[a].from, t = 1ull << arcs[a].to;
            if ((k.reach & f) && !(k.reach & t)) k.reach |= t, more = true;
            if ((k.alive & t) && !(k.alive & f)) k.alive |= f, more = true;
        }
    }
    uint64_t states = prune ? (finals & k.reach) : (n_states >= 64 ? ~0ull : (1ull << n_states) - 1);
    for (uint32_t i = 0; i < n_items; i++) {
        const uint64_t m = masks[items[i].set];
        if (prune && (!(m & k.reach) || !(k.alive >> items[i].target & 1))) continue;
        k.items.push_back(i);
        states |= m;
    }
    for (uint32_t s = 0; s < n_states; s++)
        if (states >> s & 1) k.states.push_back(s);
    return k;
}

struct OnePassGramPlan {
    OnePassPlan o;            // cap, L, n, the blocks; its row figures are the one-pass decoder's and are not used
    size_t a_row = 0, e_row = 0, col_row = 0;  // elements per row: u64 keys and u32 prefix costs [n_states][max_frames + 1], 16-byte column entries
    size_t row_bytes = 0;
    bool fits = false;        // one row stays within kOnePassScratch: a call is refused otherwise
    uint32_t rows = 0;        // per launch group
    uint32_t launches = 0;    // per launch group: init, two per block (one where nothing is kept to sweep), trace
};

// tpl_len = the longest template of the store (rows of a saved column); block / forced_rows: the testing hooks, 0 = default
inline OnePassGramPlan onepass_gram_plan(uint32_t tpl_len, uint32_t n_states, uint32_t kept_items, uint32_t kept_states, uint32_t max_frames,
                                         uint32_t frames_cap, uint32_t L, uint32_t block, uint32_t forced_rows)
{
    OnePassGramPlan p;
    p.o = onepass_plan(tpl_len, 1u, max_frames, frames_cap, L, block, forced_rows);
    p.a_row = p.e_row = (size_t)n_states * ((size_t)max_frames + 1u);
    p.col_row = (size_t)kept_items * tpl_len;
    p.row_bytes = p.a_row * 8u + p.e_row * 4u + p.col_row * 16u;
    p.fits = p.row_bytes <= kOnePassScratch;
    const size_t fit = kOnePassScratch / p.row_bytes;
    p.rows = (uint32_t)(fit < 1 ? 1 : fit > kOnePassMaxRows ? kOnePassMaxRows : fit);
    if (forced_rows) p.rows = forced_rows < kOnePassMaxRows ? forced_rows : kOnePassMaxRows;
    const uint32_t per_block = (kept_items ? 1u : 0u) + (kept_states ? 1u : 0u);
    p.launches = per_block * (uint32_t)p.o.blocks.size() + (kept_states ? 2u : 1u);
    return p;
}

}  // namespace sr
