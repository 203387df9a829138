// The front end of the PCM sessions (every live session through LiveCore, sr_live_host.h): a channel keeps the samples from its next frame's
// pre-emphasis predecessor on; a push stages [kept | chunk] rows (k_spot_live_stage), runs the frame kernel over them as
// sr_mfcc_batch_dev launches it, and puts back what the next push's first frame needs (k_spot_live_keep).  HOST ONLY.
#pragma once
#include "sr_engine_internal.h"

namespace sr {

// the layout the stage and keep kernels share: one definition for every session
static inline uint32_t live_pcm_keep_stride(const sr_engine *h) { return (h->frame_len + 7u) & ~7u; }  // a channel keeps at most frame_len samples
static inline uint64_t live_pcm_stage_stride(const sr_engine *h, uint32_t chunk_max)  // [kept | chunk] and a frame of slack
{
    return ((uint64_t)2 * h->frame_len + chunk_max + 16 + 7) & ~7ull;
}

// chan[c] (host copy of what d_chan holds): kept, n_samp, drop and n = the new frames of channel c; max_row = the longest
// [kept | chunk] row, max_frames = the largest n.  The features of channel c land at feat + c * max_frames(engine) * 12.
static inline int live_pcm_front_end(sr_engine *h, const SpotLiveChan *d_chan, const std::vector<SpotLiveChan> &chan, const std::vector<uint32_t> &mid,
                                     uint32_t max_row, uint32_t max_frames, const uint16_t *d_pcm, uint64_t pcm_stride, uint16_t *keep,
                                     uint32_t keep_stride, uint16_t *stage, uint64_t stage_stride, sr_vad_rec *d_recs, int16_t *feat, hipStream_t s)
{
    const uint32_t C = (uint32_t)chan.size();
    const SpotLivePcmArgs pa{d_chan, C, d_pcm, pcm_stride, keep, keep_stride, stage, stage_stride, max_row};
    launch_spot_live_stage(pa, s);
    if (max_frames) {
        std::vector<sr_vad_rec> recs(C);
        for (uint32_t c = 0; c < C; c++) {
            sr_vad_rec &r = recs[c];
            std::memset(&r, 0, sizeof r);
            r.atap.mid_val = mid[c];
            for (int i = 0; i < 2 * SR_MAX_SEG; i++) r.seg[i] = -1;
            r.seg[0] = 1;  // sample 0 of a row is the first new frame's pre-emphasis predecessor
            r.seg[1] = (int32_t)(chan[c].kept + chan[c].n_samp);
            r.frm_num = chan[c].n;
        }
        HIP_TRY(hipMemcpyAsync(d_recs, recs.data(), (size_t)C * sizeof(sr_vad_rec), hipMemcpyHostToDevice, s));
        launch_mfcc(mfcc_args(h, stage, stage_stride, C, d_recs, feat), mfcc_mag_tab(h), s);
    }
    launch_spot_live_keep(pa, s);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

}  // namespace sr
