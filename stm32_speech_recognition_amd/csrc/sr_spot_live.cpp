// Live word spotting (include/sr_engine.h, "live word spotting"): feature frames or samples that arrive in pushes, the
// spotter's boundary column and window carry of every (channel, slot) pair kept on the device between calls (k_spot_live.hip).
// OPT-IN EXTENSION, NO REFERENCE COUNTERPART.
//
// The host knows every count: each channel's frames so far, hence which windows a push completes and which output row each
// of them gets (the mirror, sr_spot_live_plan.h).  Nothing is read back to size or to label an output.  The session core, the
// input checks and the push sequence are every live session's (sr_live_host.h).
#include "sr_live_host.h"
#include "sr_spot_live_plan.h"

using namespace sr;

struct sr_spot_live : LiveCore {
    SpotLiveMirror m;                     // per channel the store it is bound to, its frames and (PCM) its kept samples
    // layout of the device state: that of the store the session was opened or last reset against
    uint32_t K = 0, tpl_len = 0;
    uint64_t chan_stride = 0, layout_serial = 0;
    DevBuf<uint8_t> state;
};

namespace {

// the conditions of sr_spot_dp_batch_dev on the engine and its current store
int check_store(const sr_engine *h)
{
    if (h->nc != (uint32_t)kCoef) return fail(SR_ERR_BAD_CONFIG, "the word spotter is built for 12-coefficient records");
    if (!h->K) return fail(SR_ERR_NO_TEMPLATES, "no templates set");
    if (store_tpl_len(h) > spot_max_tpl(h->lds)) return fail(SR_ERR_BAD_ARG, "templates too long for the word spotter's LDS image");
    return SR_OK;
}

// the device state laid out for the engine's current store (nothing of value is in it: see sr_spot_live_end)
int relayout(sr_spot_live *l)
{
    const sr_engine *h = l->h;
    const uint64_t per = spot_live_state_bytes(h->K, store_tpl_len(h));
    if (int rc = l->state.reserve((size_t)(per * l->C))) return rc;
    l->K = h->K;
    l->tpl_len = store_tpl_len(h);
    l->chan_stride = per;
    l->layout_serial = h->store_serial;
    return SR_OK;
}

// development hook "spot_live_origin" (testing build; 0 otherwise): the frame count a fresh channel stands at
int spot_live_origin(uint32_t *origin)
{
    const int64_t v = dev_hook(kHookSpotLiveOrigin);
    if (v < 0 || v > (int64_t)kSpotLiveMaxFrames) return fail(SR_ERR_BAD_ARG, "development hook spot_live_origin: 0..0xFFFF0000 frames");
    *origin = (uint32_t)v;
    return SR_OK;
}

// channel c fresh at a nonzero origin: nothing before it is reachable -- every saved column entry kSpotInf, no carry, the
// carry's window 0xFFFFFFFF, which is what all-ones bytes say (the kernel reads the saved column whenever x0 != 0)
int unreachable_before_origin(sr_spot_live *l, uint32_t c, hipStream_t s)
{
    HIP_TRY(hipMemsetAsync(l->state.p + (uint64_t)c * l->chan_stride, 0xFF, l->chan_stride, s));
    return SR_OK;
}

// what a push with these counts does; everything a push can refuse for its counts is refused here (sr_spot_live_plan.h)
int plan_push(const sr_spot_live *l, const uint32_t *n, uint32_t n_all, LivePlan *pl)
{
    std::string why;
    if (!spot_live_plan(l->m, l->h->store_serial, n, n_all, pl, &why)) return fail(SR_ERR_BAD_ARG, why);
    return SR_OK;
}

int check_outputs(const LivePlan &pl, uint32_t max_rows, const void *hits, const sr_spot_win *wins)
{
    if (max_rows < pl.rows)
        return fail(SR_ERR_BAD_ARG, "max_rows " + std::to_string(max_rows) + " is below the " + std::to_string(pl.rows) +
                                        " window rows of this push (sr_spot_live_rows)");
    if (pl.rows && (!hits || !wins)) return fail(SR_ERR_BAD_ARG, "null argument");
    return SR_OK;
}

// the spotter over the new frames of every channel, enqueued on s (PCM: samples that complete no frame are staged and kept only)
int launch_push(sr_spot_live *l, const LivePlan &pl, const int16_t *d_mfcc, uint64_t row_stride, sr_spot_hit *d_hits, uint32_t *d_scores,
                hipStream_t s)
{
    const sr_engine *h = l->h;
    if (!pl.max_frames) return SR_OK;
    launch_spot_live(SpotLiveArgs{d_mfcc, row_stride, l->d_chan.p, l->C, h->tpl.p, h->tpl_frames.p, h->tpl_valid.p, l->K, h->tpl_stride,
                                  l->tpl_len, l->m.win, l->state.p, l->chan_stride, d_hits, d_scores},
                     s);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

// host forms: the engine's device copies of the outputs, and their way back
struct SpotHostOutputs {
    sr_engine *h;
    uint32_t rows;
    sr_spot_hit *hits;
    uint32_t *scores;
    int reserve()
    {
        const size_t n_rec = (size_t)std::max(rows, 1u) * h->K;
        if (int rc = h->s_spot_hits.reserve(n_rec)) return rc;
        return scores ? h->s_spot_scores.reserve(n_rec) : SR_OK;
    }
    int down()
    {
        if (!rows) return SR_OK;
        COPY_DOWN(hits, h->s_spot_hits.p, (size_t)rows * h->K * sizeof(sr_spot_hit));
        if (scores) COPY_DOWN(scores, h->s_spot_scores.p, (size_t)rows * h->K * 4);
        return SR_OK;
    }
};

// the four push forms: a frame push enqueues work when it brings a frame, a PCM push when it brings a sample
int push(sr_spot_live *l, const LiveIn &in, bool device, void *stream, const uint32_t *n, uint32_t n_all, uint32_t max_rows, sr_spot_hit *hits,
         uint32_t *scores, sr_spot_win *wins, uint32_t *n_rows)
{
    if (!l) return fail(SR_ERR_BAD_ARG, "null session");
    LivePlan pl;
    int rc = plan_push(l, n, n_all, &pl);
    if (!rc) rc = check_live_in(l->m.pcm, in, pl.max_n, device);
    if (!rc) rc = check_outputs(pl, max_rows, hits, wins);
    if (rc) return rc;
    const bool work = in.pcm ? pl.max_n : pl.max_frames;
    const auto advance = [&] { spot_live_advance(l->m, pl, wins, n_rows); };
    if (device)
        return live_push_dev(*l, pl, work, in, stream,
                             [&](const int16_t *f, uint64_t rs, hipStream_t s) { return launch_push(l, pl, f, rs, hits, scores, s); }, advance);
    sr_engine *h = l->h;
    return live_push_host(*l, pl, work, in, [&] { return SpotHostOutputs{h, pl.rows, hits, scores}; },
                          [&](SpotHostOutputs &, const int16_t *f, uint64_t rs, hipStream_t s) {
                              return launch_push(l, pl, f, rs, h->s_spot_hits.p, scores ? h->s_spot_scores.p : nullptr, s);
                          }, advance);
}

}  // namespace

extern "C" {

int sr_spot_live_geometry(uint32_t tpl_rows, uint32_t K, uint32_t chunk_max, uint32_t win_frames, uint32_t out[3])
{
    if (!out || !tpl_rows || tpl_rows > 16383 || !K || !chunk_max || !win_frames) return fail(SR_ERR_BAD_ARG, "null / zero argument");
    const LdsBudget mi355x;  // no device: MI355X's figures
    out[0] = (uint32_t)(((uint64_t)chunk_max + win_frames - 1) / win_frames);  // entering on a window's last frame
    out[1] = (uint32_t)std::min<uint64_t>(spot_live_state_bytes(K, tpl_rows), 0xFFFFFFFFull);
    out[2] = spot_max_tpl(mi355x);
    return SR_OK;
}

int sr_spot_live_open(sr_engine *h, uint32_t n_channels, uint32_t chunk_max, uint32_t win_frames, const uint32_t *mid, sr_spot_live **out)
{
    if (!h || !out) return fail(SR_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (!n_channels || n_channels > kLiveMaxChannels || !chunk_max || !win_frames)
        return fail(SR_ERR_BAD_ARG, "n_channels not in 1..65535 / chunk_max 0 / win_frames 0");
    if (int rc = check_store(h)) return rc;
    if (int rc = LiveCore::check_open(h, n_channels, chunk_max, h->cfg.max_frames, mid)) return rc;
    uint32_t origin = 0;
    if (int rc = spot_live_origin(&origin)) return rc;
    ENTER_DEVICE(h);
    sr_spot_live *l = new sr_spot_live();
    l->m.open(n_channels, h->store_serial, origin);
    l->m.chunk_max = chunk_max;
    l->m.win = win_frames;
    l->m.pcm = mid != nullptr;
    l->m.frame_len = h->frame_len;
    l->m.hop = h->hop;
    int rc = l->open_common(h, n_channels, chunk_max, mid);
    if (!rc) rc = relayout(l);
    for (uint32_t c = 0; c < n_channels && origin && !rc; c++) rc = unreachable_before_origin(l, c, nullptr);
    if (!rc && origin && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(SR_ERR_HIP, "hipStreamSynchronize failed");
    if (rc) {
        (void)hipGetLastError();
        sr_spot_live_close(l);
        return rc;
    }
    *out = l;
    return SR_OK;
}

void sr_spot_live_close(sr_spot_live *l)
{
    if (!l) return;
    DeviceGuard guard;
    (void)guard.enter(l->h->device);
    l->release();
    l->state.release();
    delete l;
}

uint32_t sr_spot_live_windows(uint32_t win_frames, const uint32_t *frames_before, const uint32_t *n_new, uint32_t n_channels)
{
    if (!win_frames || !frames_before || !n_new) return 0;
    uint64_t rows = 0;
    for (uint32_t c = 0; c < n_channels; c++) {
        if ((uint64_t)frames_before[c] + n_new[c] > kSpotLiveMaxFrames) return 0;
        rows += spot_live_windows_done(frames_before[c], n_new[c], win_frames);
    }
    return (uint32_t)std::min<uint64_t>(rows, 0xFFFFFFFFull);
}

uint32_t sr_spot_live_rows(const sr_spot_live *l, const uint32_t *n, uint32_t n_all)
{
    if (!l) return 0;
    LivePlan pl;
    return plan_push(l, n, n_all, &pl) ? 0 : pl.rows;
}

int sr_spot_live_push_dev(sr_spot_live *l, const int16_t *d_mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                          sr_spot_hit *d_hits, uint32_t *d_scores, sr_spot_win *wins, uint32_t *n_rows, void *stream)
{
    return push(l, LiveIn{d_mfcc, row_stride, false}, true, stream, n, n_all, max_rows, d_hits, d_scores, wins, n_rows);
}

int sr_spot_live_push(sr_spot_live *l, const int16_t *mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                      sr_spot_hit *hits, uint32_t *scores, sr_spot_win *wins, uint32_t *n_rows)
{
    return push(l, LiveIn{mfcc, row_stride, false}, false, nullptr, n, n_all, max_rows, hits, scores, wins, n_rows);
}

int sr_spot_live_push_pcm_dev(sr_spot_live *l, const uint16_t *d_pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                              uint32_t max_rows, sr_spot_hit *d_hits, uint32_t *d_scores, sr_spot_win *wins, uint32_t *n_rows, void *stream)
{
    return push(l, LiveIn{d_pcm, pcm_stride, true}, true, stream, n, n_all, max_rows, d_hits, d_scores, wins, n_rows);
}

int sr_spot_live_push_pcm(sr_spot_live *l, const uint16_t *pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                          sr_spot_hit *hits, uint32_t *scores, sr_spot_win *wins, uint32_t *n_rows)
{
    return push(l, LiveIn{pcm, pcm_stride, true}, false, nullptr, n, n_all, max_rows, hits, scores, wins, n_rows);
}

int sr_spot_live_end(sr_spot_live *l, const uint32_t *channels, uint32_t n_ch, sr_spot_hit *hits, sr_spot_win *wins, uint32_t *n_rows)
{
    if (!l || (n_ch && !channels)) return fail(SR_ERR_BAD_ARG, "null argument");
    sr_engine *h = l->h;
    std::vector<SpotLiveFlush> list;
    uint32_t rows = 0, origin = 0;
    std::string why;
    if (!spot_live_end_list(l->m, l->layout_serial, h->store_serial, channels, n_ch, &list, &rows, &why)) return fail(SR_ERR_BAD_ARG, why);
    if (int rc = spot_live_origin(&origin)) return rc;
    const bool changed = l->layout_serial != h->store_serial;  // then every channel that holds state is bound to a store that is gone
    if (changed)
        if (int rc = check_store(h)) return rc;
    if (rows && (!hits || !wins)) return fail(SR_ERR_BAD_ARG, "null argument");
    if (!n_ch) {
        if (n_rows) *n_rows = 0;
        return SR_OK;
    }
    ENTER_HOST_CALL(h);
    if (int rc = l->wait_last()) return rc;
    TmpDevBuf<SpotLiveFlush> d_list;
    if (int rc = d_list.reserve(list.size())) return rc;
    if (rows)
        if (int rc = h->s_spot_hits.reserve((size_t)rows * l->K)) return rc;
    COPY_UP(d_list.p, list.data(), list.size() * sizeof(SpotLiveFlush));
    launch_spot_live_flush(d_list.p, (uint32_t)list.size(), l->state.p, l->chan_stride, l->K, l->tpl_len, h->s_spot_hits.p, nullptr);
    HIP_TRY(hipGetLastError());
    if (rows) COPY_DOWN(hits, h->s_spot_hits.p, (size_t)rows * l->K * sizeof(sr_spot_hit));
    else HIP_TRY(hipStreamSynchronize(nullptr));
    if (changed)
        if (int rc = relayout(l)) return rc;
    if (origin) {  // behind the flush on the null stream; complete before a push on any stream can follow
        for (const SpotLiveFlush &f : list)
            if (int rc = unreachable_before_origin(l, f.channel, nullptr)) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    spot_live_reset(l->m, h->store_serial, origin, list, wins);
    if (n_rows) *n_rows = rows;
    return SR_OK;
}

}  // extern "C"
