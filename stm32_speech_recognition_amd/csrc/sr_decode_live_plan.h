// The host mirror of a live connected-word decoding session (sr_decode_live.cpp) and what it says about a call before
// anything reaches the device: which channels a push touches, where each stands, which compact output row it gets, and why a
// push is refused; the distinct channels of an end list.  The host knows every count, so nothing is read back.
// HOST ONLY, and free of HIP calls: tests/decode_live_plan/plan_check.cpp runs it on the CPU under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "sr_live_plan.h"

namespace sr {

struct DecodeLiveMirror {
    uint32_t C = 0, chunk_max = 0, utt_frames = 0;
    bool pcm = false;
    uint32_t frame_len = 0, hop = 1;      // PCM sessions: the engine's framing
    std::vector<uint64_t> bound;          // per channel: the store serial it is bound to,
    std::vector<uint32_t> frames, kept;   // its frames so far and (PCM) its kept samples
    void open(uint32_t n_channels, uint64_t serial)
    {
        C = n_channels;
        bound.assign(C, serial);
        frames.assign(C, 0);
        kept.assign(C, 0);
    }
};

using DecodeLivePlan = LivePlan;  // chan = ChainLiveArgs::chan; rows = the channels that emit one

// What a push with these counts does, from the counts alone.  Refusals, channel by channel in ascending order and per
// channel in this order: a count above chunk_max; a channel bound to a replaced store; a channel taken past utt_frames.
// Returns false with the reason in *why; the mirror is not changed.
inline bool decode_live_plan(const DecodeLiveMirror &m, uint64_t store_serial, const uint32_t *n, uint32_t n_all, DecodeLivePlan *pl,
                             std::string *why)
{
    *pl = DecodeLivePlan{};
    pl->chan.assign(m.C, SpotLiveChan{});
    for (uint32_t c = 0; c < m.C; c++) {
        const uint32_t cnt = n ? n[c] : n_all;
        SpotLiveChan &ch = pl->chan[c];
        if (cnt > m.chunk_max) {
            *why = "count of channel " + std::to_string(c) + " exceeds chunk_max";
            return false;
        }
        if (cnt && m.bound[c] != store_serial) {
            *why = "the template store changed: end channel " + std::to_string(c) + " before pushing to it";
            return false;
        }
        const uint32_t nf = m.pcm ? live_pcm_frames(m.kept[c], cnt, m.frame_len, m.hop, &ch, &pl->max_row) : cnt;
        if ((uint64_t)m.frames[c] + nf > m.utt_frames) {
            *why = "channel " + std::to_string(c) + " would pass utt_frames: end it first";
            return false;
        }
        ch.x0 = m.frames[c];
        ch.n = nf;
        ch.row_base = pl->rows;
        ch.first_win = cnt ? 1u : 0u;  // the channel emits a row
        pl->rows += cnt ? 1u : 0u;
        pl->max_n = std::max(pl->max_n, cnt);
        pl->max_frames = std::max(pl->max_frames, nf);
    }
    return true;
}

// the push is enqueued: the mirror follows, and the caller learns which channel each row holds
inline void decode_live_advance(DecodeLiveMirror &m, const DecodeLivePlan &pl, sr_chain_live_row *rows, uint32_t *n_rows)
{
    for (uint32_t c = 0; c < m.C; c++) {
        const SpotLiveChan &ch = pl.chan[c];
        m.frames[c] = ch.x0 + ch.n;
        if (m.pcm) m.kept[c] = ch.kept + ch.n_samp - ch.drop;
        if (ch.first_win) rows[ch.row_base] = sr_chain_live_row{c, m.frames[c]};
    }
    if (n_rows) *n_rows = pl.rows;
}

// sr_decode_live_end: one row per DISTINCT listed channel, in the order of first mention.  chan[c] of a listed channel says
// "trace x0 frames into row row_base"; a channel bound to a replaced store has lost its recording (x0 = 0: no parse).
// Returns false for a channel past the session's last.
inline bool decode_live_end_list(const DecodeLiveMirror &m, uint64_t store_serial, const uint32_t *channels, uint32_t n_ch,
                                 std::vector<SpotLiveChan> *chan, std::vector<sr_chain_live_row> *order, std::string *why)
{
    chan->assign(m.C, SpotLiveChan{});
    order->clear();
    for (uint32_t i = 0; i < n_ch; i++)
        if (channels[i] >= m.C) {
            *why = "channel " + std::to_string(channels[i]) + " is past the session's last";
            return false;
        }
    for (uint32_t i = 0; i < n_ch; i++) {
        const uint32_t c = channels[i];
        SpotLiveChan &ch = (*chan)[c];
        if (ch.first_win) continue;  // listed before: it counts once
        ch.x0 = m.bound[c] == store_serial ? m.frames[c] : 0u;
        ch.row_base = (uint32_t)order->size();
        ch.first_win = 1u;
        order->push_back(sr_chain_live_row{c, ch.x0});
    }
    return true;
}

// ... after which each of them is as freshly opened, and bound to the current store
inline void decode_live_reset(DecodeLiveMirror &m, uint64_t store_serial, const std::vector<sr_chain_live_row> &order)
{
    for (const sr_chain_live_row &r : order) {
        m.frames[r.channel] = 0;
        m.kept[r.channel] = 0;
        m.bound[r.channel] = store_serial;
    }
}

// sr_decode_live_geometry's out[0]: the columns and the A / E history of one channel, saturating
inline uint32_t decode_live_state_bytes(uint32_t tpl_len, uint32_t K, uint32_t max_words, uint32_t utt_frames)
{
    const uint64_t cols = (uint64_t)max_words * K * tpl_len * 16u;
    const uint64_t hist = ((uint64_t)utt_frames + 1u) * ((uint64_t)max_words * 8u + ((uint64_t)max_words + 1u) * 4u);
    return (uint32_t)std::min<uint64_t>(cols + hist, 0xFFFFFFFFull);
}

}  // namespace sr
