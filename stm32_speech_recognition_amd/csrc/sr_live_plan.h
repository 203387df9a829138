// What the plans of every live session have in common (sr_spot_live_plan.h, sr_decode_live_plan.h and what builds on them):
// the plan of a push and the samples-to-frames rule of the PCM sessions.  HOST ONLY, and free of HIP calls.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "sr_device.h"

namespace sr {

// what a push does, from its counts alone
struct LivePlan {
    std::vector<SpotLiveChan> chan;                              // what d_chan holds during the push, sr_device.h
    uint32_t rows = 0, max_n = 0, max_frames = 0, max_row = 0;   // output rows; the largest count, frame count and [kept | chunk] row
};

// PCM sessions: a channel that keeps `kept` samples gets `cnt` more.  Frame j exists once 1 + j * hop + frame_len samples have
// arrived, and the row [kept | chunk] starts at the first new frame's predecessor: the new frames are returned, kept, n_samp
// and drop = the samples no later frame needs go into *ch, and *max_row follows the longest row that got samples.
inline uint32_t live_pcm_frames(uint32_t kept, uint32_t cnt, uint32_t frame_len, uint32_t hop, SpotLiveChan *ch, uint32_t *max_row)
{
    const uint64_t total = (uint64_t)kept + cnt;
    const uint32_t nf = total >= 1 + (uint64_t)frame_len ? (uint32_t)((total - 1 - frame_len) / hop + 1) : 0;
    ch->kept = kept;
    ch->n_samp = cnt;
    ch->drop = nf * hop;
    if (cnt) *max_row = std::max(*max_row, (uint32_t)total);
    return nf;
}

}  // namespace sr
