// What a live grammar-constrained decoding session (sr_gram_live.cpp) knows on the host next to the decoder's mirror
// (sr_decode_live_plan.h, used as it is): where each level's boundary columns start, given the items the grammar keeps per
// level; whether the session's grammar is older than the engine's store or word map; whether every channel is empty, which
// is when the grammar may be switched.  The mirror's store binding is not used by a grammar session -- the grammar carries the
// store AND the word map it was compiled against -- so the mirror is opened, planned and reset with one constant serial, and
// an end list of a stale grammar is planned with another: every listed recording is then dropped.
// HOST ONLY, and free of HIP calls: tests/gram_live_plan/plan_check.cpp runs it on the CPU under the sanitizers.
#pragma once
#include "sr_decode_live_plan.h"
#include "sr_dtw_plan.h"

namespace sr {

constexpr uint64_t kGramLiveBound = 0, kGramLiveStale = 1;  // the mirror's serial of a session; what a stale end list is planned with

struct GramLiveLayout {
    uint32_t col_off[kChainMaxWords] = {};  // level l's first column at col_off[l - 1]
    uint32_t columns = 0;                   // boundary columns per channel: the items kept, summed over the levels
    uint32_t levels = 0;                    // levels that keep items
    uint32_t launches() const { return 2 + 2 * levels; }  // init, per level with items (words, close), trace
};

// items_per_level[l - 1]: the items sr_grammar_plan reports for level l of max_words (<= 16 levels of <= 2^20 items: no overflow)
inline GramLiveLayout gram_live_layout(const uint32_t *items_per_level, uint32_t max_words)
{
    GramLiveLayout lay;
    for (uint32_t l = 0; l < max_words && l < kChainMaxWords; l++) {
        lay.col_off[l] = lay.columns;
        lay.columns += items_per_level[l];
        lay.levels += items_per_level[l] ? 1u : 0u;
    }
    return lay;
}

// sr_gram_live_geometry's out[0]: the columns and the dense [S] history of one channel, saturating
inline uint32_t gram_live_state_bytes(uint32_t columns, uint32_t tpl_len, uint32_t n_states, uint32_t max_words, uint32_t utt_frames)
{
    const uint64_t cols = (uint64_t)columns * tpl_len * 16u;  // <= 2^24 * 2^14 * 2^4
    const uint64_t hist = ((uint64_t)utt_frames + 1u) * n_states * ((uint64_t)max_words * 8u + ((uint64_t)max_words + 1u) * 4u);
    return (uint32_t)std::min<uint64_t>(cols + hist, 0xFFFFFFFFull);
}

// a grammar compiled against (g_store, g_word) under an engine that stands at (h_store, h_word); *why names what changed
inline bool gram_live_stale(uint64_t g_store, uint64_t g_word, uint64_t h_store, uint64_t h_word, std::string *why)
{
    if (g_store != h_store) {
        *why = "the template store changed since the session's grammar was compiled: end the channels, then sr_gram_live_set_grammar";
        return true;
    }
    if (g_word != h_word) {
        *why = "the word map changed since the session's grammar was compiled: end the channels, then sr_gram_live_set_grammar";
        return true;
    }
    return false;
}

// sr_gram_live_set_grammar: only while no channel holds frames or (PCM) kept samples
inline bool gram_live_all_empty(const DecodeLiveMirror &m, std::string *why)
{
    for (uint32_t c = 0; c < m.C; c++)
        if (m.frames[c] || m.kept[c]) {
            *why = "channel " + std::to_string(c) + " holds a recording: end every channel before the grammar is switched";
            return false;
        }
    return true;
}

}  // namespace sr
