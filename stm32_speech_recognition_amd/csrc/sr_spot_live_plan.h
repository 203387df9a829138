// The host mirror of a live word-spotting session (sr_spot_live.cpp) and what it says about a call before anything reaches
// the device: where each channel stands, which windows a push completes and which output row each of them gets, why a push is
// refused; the distinct channels of an end list.  The host knows every count, so nothing is read back.  The plan of a push and
// the samples-to-frames rule are every live session's (sr_live_plan.h).
// HOST ONLY, and free of HIP calls: tests/spot_live_plan/plan_check.cpp runs it on the CPU under the sanitizers.
#pragma once
#include "sr_live_plan.h"

namespace sr {

constexpr uint32_t kSpotLiveMaxFrames = 0xFFFF0000u;  // absolute starts live in the low word of a packed state

struct SpotLiveMirror {
    uint32_t C = 0, chunk_max = 0, win = 0;
    bool pcm = false;
    uint32_t frame_len = 0, hop = 1;      // PCM sessions: the engine's framing
    std::vector<uint64_t> bound;          // per channel: the store serial it is bound to,
    std::vector<uint32_t> frames, kept;   // its frames so far and (PCM) its kept samples
    void open(uint32_t n_channels, uint64_t serial, uint32_t origin)  // origin: the frame count a fresh channel stands at
    {
        C = n_channels;
        bound.assign(C, serial);
        frames.assign(C, origin);
        kept.assign(C, 0);
    }
};

inline uint64_t spot_live_state_bytes(uint32_t K, uint32_t tpl_len) { return (uint64_t)K * ((uint64_t)tpl_len * 16u + kSpotLiveCarryBytes); }
inline uint32_t spot_live_windows_done(uint32_t x0, uint32_t n, uint32_t win) { return (x0 + n) / win - x0 / win; }  // (x0 + n <= 0xFFFF0000)

// What a push with these counts does, from the counts alone.  Refusals, channel by channel in ascending order and per
// channel in this order: a count above chunk_max; a channel bound to a replaced store; a channel taken past 0xFFFF0000
// frames.  Returns false with the reason in *why; the mirror is not changed.
inline bool spot_live_plan(const SpotLiveMirror &m, uint64_t store_serial, const uint32_t *n, uint32_t n_all, LivePlan *pl, std::string *why)
{
    *pl = LivePlan{};
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
        if ((uint64_t)m.frames[c] + nf > kSpotLiveMaxFrames) {
            *why = "channel " + std::to_string(c) + " would pass 0xFFFF0000 frames: end it first";
            return false;
        }
        ch.x0 = m.frames[c];
        ch.n = nf;
        ch.row_base = pl->rows;
        ch.first_win = ch.x0 / m.win;
        pl->rows += spot_live_windows_done(ch.x0, nf, m.win);
        pl->max_n = std::max(pl->max_n, cnt);
        pl->max_frames = std::max(pl->max_frames, nf);
    }
    return true;
}

// the push is enqueued: the mirror follows, and the caller learns which window each row holds
inline void spot_live_advance(SpotLiveMirror &m, const LivePlan &pl, sr_spot_win *wins, uint32_t *n_rows)
{
    for (uint32_t c = 0; c < m.C; c++) {
        const SpotLiveChan &ch = pl.chan[c];
        const uint32_t done = spot_live_windows_done(ch.x0, ch.n, m.win);
        for (uint32_t i = 0; i < done; i++) wins[ch.row_base + i] = sr_spot_win{c, ch.first_win + i};
        m.frames[c] = ch.x0 + ch.n;
        if (m.pcm) m.kept[c] = ch.kept + ch.n_samp - ch.drop;
    }
    if (n_rows) *n_rows = pl.rows;
}

// sr_spot_live_end: one entry per DISTINCT listed channel, in the order of first mention -- a channel listed again is fresh by
// then, has no open window and needs no second reset (and k_spot_live_flush gives every entry threads of its own, which
// nothing orders).  An entry has a row where the channel stands inside a window AND its state is that of the current store:
// the device state is laid out for layout_serial, the engine stands at store_serial.  *rows = the entries with a row.
// Returns false for a channel past the session's last.
inline bool spot_live_end_list(const SpotLiveMirror &m, uint64_t layout_serial, uint64_t store_serial, const uint32_t *channels, uint32_t n_ch,
                               std::vector<SpotLiveFlush> *list, uint32_t *rows, std::string *why)
{
    list->clear();
    *rows = 0;
    for (uint32_t i = 0; i < n_ch; i++)
        if (channels[i] >= m.C) {
            *why = "channel " + std::to_string(channels[i]) + " is past the session's last";
            return false;
        }
    std::vector<uint8_t> seen(m.C, 0);
    for (uint32_t i = 0; i < n_ch; i++) {
        const uint32_t c = channels[i], N = m.frames[c];
        if (seen[c]) continue;
        seen[c] = 1;
        const bool open = layout_serial == store_serial && m.bound[c] == layout_serial && N % m.win != 0;
        list->push_back(SpotLiveFlush{c, open ? (*rows)++ : 0xFFFFFFFFu, N / m.win, 0u});
    }
    return true;
}

// ... after which each of them is as freshly opened, and bound to the current store; the caller learns each row's window
inline void spot_live_reset(SpotLiveMirror &m, uint64_t store_serial, uint32_t origin, const std::vector<SpotLiveFlush> &list, sr_spot_win *wins)
{
    for (const SpotLiveFlush &f : list) {
        if (f.row != 0xFFFFFFFFu) wins[f.row] = sr_spot_win{f.channel, f.wid};
        m.frames[f.channel] = origin;
        m.kept[f.channel] = 0;
        m.bound[f.channel] = store_serial;
    }
}

}  // namespace sr
