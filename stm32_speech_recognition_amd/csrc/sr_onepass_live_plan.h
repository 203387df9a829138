// The host mirror of a live one-pass decoding session (sr_onepass_live.cpp) and what it says about a call before anything
// reaches the device: which channels a push touches, where each stands, which compact output row it gets, how its new frames
// are cut into blocks, and why a push is refused; the distinct channels of an end list and of a commit list.  The host knows
// every count -- and the first frame of the block each channel's saved columns are of -- so nothing is read back.
// HOST ONLY, and free of HIP calls: tests/onepass_live_plan/plan_check.cpp and tests/onepass_commit_plan/plan_check.cpp run it
// on the CPU under the sanitizers.
//
// The cut.  The decode session's mirror and rules (sr_decode_live_plan.h) serve unchanged; on top of them a push's new frames
// [x0, x0 + n) of a channel are cut into blocks of `block` frames, block = min(L, the testing hook) with L the block length of
// the one-pass decoder for the current store (sr_onepass_plan.h): block b is [x0 + b * block, min(x0 + (b + 1) * block, x0 + n)).
// Launch b sweeps block b of every channel that has one, so a push enqueues ceil(max_c n[c] / block) sweeps.  The first block
// resumes from the column saved at c0_prev[c], the first frame of the channel's last block so far; blocks of different pushes
// may differ in length (a push boundary, or a hook set in between): none is longer than L, which is all the argument needs.
#pragma once
#include "sr_decode_live_plan.h"
#include "sr_onepass_plan.h"

namespace sr {

struct OnePassLiveMirror {
    DecodeLiveMirror d;             // channels, counts, store binding, PCM framing: the decode session's
    std::vector<uint32_t> c0_prev;  // per channel: the first frame of its last block (0 while it is empty)
    void open(uint32_t n_channels, uint64_t serial)
    {
        d.open(n_channels, serial);
        c0_prev.assign(n_channels, 0);
    }
};

struct OnePassLivePlan {
    DecodeLivePlan d;        // chan[c].aux = c0_prev[c]
    uint32_t block = 1;      // frames per block of this push
    uint32_t n_blocks = 0;   // sweeps: ceil(d.max_frames / block)
};

// frames per block for a store whose one-pass block length is L (0: no valid slot -- no word at all, one block serves), the
// testing hook (0: none) and pushes of at most max_new frames
inline uint32_t onepass_live_block(uint32_t L, uint32_t hook, uint32_t max_new)
{
    if (!L) return max_new ? max_new : 1u;
    return hook && hook < L ? hook : L;
}

// What a push with these counts does, from the counts alone.  Refusals: first the word-cost bound against the current store,
// (utt_frames / L) * word_cost <= 2^30; then decode_live_plan's, channel by channel.  Returns false with the reason in *why;
// the mirror is not changed.
inline bool onepass_live_plan(const OnePassLiveMirror &m, uint64_t store_serial, uint32_t L, uint32_t hook, uint32_t word_cost, const uint32_t *n,
                              uint32_t n_all, OnePassLivePlan *pl, std::string *why)
{
    *pl = OnePassLivePlan{};
    if (!onepass_cost_ok(m.d.utt_frames, L, word_cost)) {
        *why = "(utt_frames / L) * word_cost must be at most 2^30, L = the shortest valid template's frames / 2 + 1";
        return false;
    }
    if (!decode_live_plan(m.d, store_serial, n, n_all, &pl->d, why)) return false;
    pl->block = onepass_live_block(L, hook, pl->d.max_frames);
    pl->n_blocks = (pl->d.max_frames + pl->block - 1) / pl->block;
    for (uint32_t c = 0; c < m.d.C; c++) pl->d.chan[c].aux = m.c0_prev[c];
    return true;
}

// the push is enqueued: the mirror follows, and the caller learns which channel each row holds
inline void onepass_live_advance(OnePassLiveMirror &m, const OnePassLivePlan &pl, sr_chain_live_row *rows, uint32_t *n_rows)
{
    for (uint32_t c = 0; c < m.d.C; c++) {
        const SpotLiveChan &ch = pl.d.chan[c];
        if (ch.n) m.c0_prev[c] = ch.x0 + (ch.n - 1) / pl.block * pl.block;  // the first frame of its last block
    }
    decode_live_advance(m.d, pl.d, rows, n_rows);
}

// sr_onepass_live_end: decode_live_end_list's rows -- one per DISTINCT listed channel, in the order of first mention; x0 = the
// frames to parse, 0 for a channel bound to a replaced store -- with aux = the frames the channel holds: the positions of its
// keys that are wiped behind the trace
inline bool onepass_live_end_list(const OnePassLiveMirror &m, uint64_t store_serial, const uint32_t *channels, uint32_t n_ch,
                                  std::vector<SpotLiveChan> *chan, std::vector<sr_chain_live_row> *order, std::string *why)
{
    if (!decode_live_end_list(m.d, store_serial, channels, n_ch, chan, order, why)) return false;
    for (const sr_chain_live_row &r : *order) (*chan)[r.channel].aux = m.d.frames[r.channel];
    return true;
}

// ... after which each of them is as freshly opened, and bound to the current store
inline void onepass_live_reset(OnePassLiveMirror &m, uint64_t store_serial, const std::vector<sr_chain_live_row> &order)
{
    decode_live_reset(m.d, store_serial, order);
    for (const sr_chain_live_row &r : order) m.c0_prev[r.channel] = 0;
}

// sr_onepass_live_commit: the window of the commit rule for a store, W = 2 * (the longest valid template's frames) - 1 -- a
// word over M template frames covers at most 2M - 1 input frames -- with tpl_len[k] = the frames of a valid slot, 0 for an
// invalid one.  0: no valid slot
inline uint32_t onepass_commit_window(const uint32_t *tpl_len, uint32_t K)
{
    uint32_t longest = 0;
    for (uint32_t k = 0; k < K; k++) longest = std::max(longest, tpl_len[k]);
    return longest ? 2u * longest - 1u : 0u;
}

// ... and its rows: one per DISTINCT listed channel, in the order of first mention, with the frames the channel holds.  The
// mirror is not changed.  Returns false for a channel past the session's last and for one bound to a replaced store (its
// history speaks of slots that are gone: end it first).
inline bool onepass_live_commit_list(const OnePassLiveMirror &m, uint64_t store_serial, const uint32_t *channels, uint32_t n_ch,
                                     std::vector<sr_chain_live_row> *order, std::string *why)
{
    order->clear();
    for (uint32_t i = 0; i < n_ch; i++) {
        if (channels[i] >= m.d.C) {
            *why = "channel " + std::to_string(channels[i]) + " is past the session's last";
            return false;
        }
        if (m.d.bound[channels[i]] != store_serial) {
            *why = "the template store changed: end channel " + std::to_string(channels[i]) + " before committing on it";
            return false;
        }
    }
    std::vector<uint8_t> listed(m.d.C, 0);
    for (uint32_t i = 0; i < n_ch; i++) {
        const uint32_t c = channels[i];
        if (listed[c]) continue;  // listed before: it counts once
        listed[c] = 1;
        order->push_back(sr_chain_live_row{c, m.d.frames[c]});
    }
    return true;
}

// sr_onepass_live_geometry's out[0]: per channel the history (u64 keys and u32 prefix costs over utt_frames + 1 positions), one
// saved column per slot and the whole feature row, saturating
inline uint32_t onepass_live_state_bytes(uint32_t tpl_len, uint32_t K, uint32_t utt_frames)
{
    const uint64_t hist = ((uint64_t)utt_frames + 1u) * 12u, cols = (uint64_t)K * tpl_len * 16u, feat = (uint64_t)utt_frames * 24u;
    return (uint32_t)std::min<uint64_t>(hist + cols + feat, 0xFFFFFFFFull);
}

// ... and its out[3]: a sweep and a close per block, and the trace
inline uint32_t onepass_live_launches(uint32_t chunk_max, uint32_t block) { return 2u * ((chunk_max + block - 1) / block) + 1u; }

}  // namespace sr
