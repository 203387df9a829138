// What a live one-pass grammar decoding session (sr_onepass_gram_live.cpp) knows on the host: the live one-pass decoder's
// mirror and cut (sr_onepass_live_plan.h, used as they are) under the grammar sessions' binding (sr_gram_live_plan.h: the
// grammar carries the store and the word map, so the mirror is opened, planned and reset with one constant serial, and an end
// list of a stale grammar is planned with another), and on top of them the state bytes and the launch counts of a session
// whose history is dense by state and whose columns are the grammar's kept items.  The cost bound is NOT part of a push's plan:
// it is checked when a grammar is adopted, and a stale grammar refuses pushes, so the store cannot change under a live bound.
// HOST ONLY, and free of HIP calls: tests/onepass_gram_live_plan/plan_check.cpp runs it on the CPU under the sanitizers.
#pragma once
#include "sr_gram_live_plan.h"
#include "sr_onepass_gram_plan.h"
#include "sr_onepass_live_plan.h"

namespace sr {

// What a push with these counts does, from the counts alone: decode_live_plan's refusals, channel by channel, then the cut into
// blocks of onepass_live_block(L, hook, the most new frames).  Returns false with the reason in *why; the mirror is not changed.
inline bool onepass_gram_live_plan(const OnePassLiveMirror &m, uint32_t L, uint32_t hook, const uint32_t *n, uint32_t n_all, OnePassLivePlan *pl,
                                   std::string *why)
{
    *pl = OnePassLivePlan{};
    if (!decode_live_plan(m.d, kGramLiveBound, n, n_all, &pl->d, why)) return false;
    pl->block = onepass_live_block(L, hook, pl->d.max_frames);
    pl->n_blocks = (pl->d.max_frames + pl->block - 1) / pl->block;
    for (uint32_t c = 0; c < m.d.C; c++) pl->d.chan[c].aux = m.c0_prev[c];
    return true;
}

// launches per block: a sweep where an item is kept, a close where a state is kept
inline uint32_t onepass_gram_live_per_block(uint32_t kept_items, uint32_t kept_states) { return (kept_items ? 1u : 0u) + (kept_states ? 1u : 0u); }

// the launches of a push of n_blocks blocks: per block, and the trace
inline uint32_t onepass_gram_live_push_launches(uint32_t n_blocks, uint32_t kept_items, uint32_t kept_states)
{
    return onepass_gram_live_per_block(kept_items, kept_states) * n_blocks + 1u;
}

// sr_onepass_gram_live_geometry's out[3]: a feature push of chunk_max frames
inline uint32_t onepass_gram_live_launches(uint32_t chunk_max, uint32_t block, uint32_t kept_items, uint32_t kept_states)
{
    return onepass_gram_live_push_launches((chunk_max + block - 1) / block, kept_items, kept_states);
}

// sr_onepass_gram_live_geometry's out[0]: per channel the dense history (u64 keys and u32 prefix costs over utt_frames + 1
// positions of every state), one saved column per kept item and the whole feature row, saturating
inline uint32_t onepass_gram_live_state_bytes(uint32_t n_states, uint32_t kept_items, uint32_t tpl_len, uint32_t utt_frames)
{
    const uint64_t hist = (uint64_t)n_states * ((uint64_t)utt_frames + 1u) * 12u;  // <= 2^6 * 2^14 * 12
    const uint64_t cols = (uint64_t)kept_items * tpl_len * 16u;                    // <= 2^32 * 2^14 * 2^4
    const uint64_t feat = (uint64_t)utt_frames * 24u;
    return (uint32_t)std::min<uint64_t>(hist + cols + feat, 0xFFFFFFFFull);
}

}  // namespace sr
