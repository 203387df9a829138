// Live word spotting (include/sr_engine.h, "live word spotting"): feature frames or samples that arrive in pushes, the
// spotter's boundary column and window carry of every (channel, slot) pair kept on the device between calls (k_spot_live.hip).
// OPT-IN EXTENSION, NO REFERENCE COUNTERPART.
//
// The host knows every count: each channel's frames so far, hence which windows a push completes and which output row each
// of them gets (the mirror below).  Nothing is read back to size or to label an output.
#include "sr_host_call.h"
#include "sr_live_pcm.h"

using namespace sr;

struct sr_spot_live {
    sr_engine *h = nullptr;
    uint32_t C = 0, chunk_max = 0, win = 0;
    bool pcm = false;
    std::vector<uint32_t> mid;            // PCM sessions: the channels' mid values
    // layout of the device state: that of the store the session was opened or last reset against
    uint32_t K = 0, tpl_len = 0;
    uint64_t chan_stride = 0, layout_serial = 0;
    // the mirror: per channel the store it is bound to, its frames and (PCM) its kept samples
    std::vector<uint64_t> bound;
    std::vector<uint32_t> frames, kept;
    DevBuf<uint8_t> state;
    DevBuf<SpotLiveChan> d_chan;
    // PCM sessions: kept samples, the rows [kept | chunk], their records and the features of one push
    DevBuf<uint16_t> keep, stage;
    DevBuf<sr_vad_rec> recs;
    DevBuf<int16_t> feat;
    uint32_t keep_stride = 0;
    uint64_t stage_stride = 0;
    hipEvent_t ev_last = nullptr;         // end of the last push (sr_spot_live_end / _close wait for it)
    hipStream_t last_stream = nullptr;    // ... and the stream it ran on: a push on another stream runs behind it
    bool pending = false;
};

namespace {

constexpr uint32_t kSpotLiveMaxFrames = 0xFFFF0000u;  // absolute starts live in the low word of a packed state
constexpr uint32_t kSpotLiveMaxChannels = 65535u;     // a grid dimension

uint64_t state_bytes(uint32_t K, uint32_t tpl_len) { return (uint64_t)K * ((uint64_t)tpl_len * 16u + kSpotLiveCarryBytes); }
uint32_t windows_done(uint32_t x0, uint32_t n, uint32_t win) { return (x0 + n) / win - x0 / win; }  // (x0 + n <= 0xFFFF0000)

// the conditions of sr_spot_dp_batch_dev on the engine and its current store
int check_store(const sr_engine *h)
{
    if (h->nc != (uint32_t)kCoef) return fail(SR_ERR_BAD_CONFIG, "the word spotter is built for 12-coefficient records");
    if (!h->K) return fail(SR_ERR_NO_TEMPLATES, "no templates set");
    if (h->tpl_rows - 1 > spot_max_tpl(h->lds)) return fail(SR_ERR_BAD_ARG, "templates too long for the word spotter's LDS image");
    return SR_OK;
}

// the device state laid out for the engine's current store (nothing of value is in it: see sr_spot_live_end)
int relayout(sr_spot_live *l)
{
    const sr_engine *h = l->h;
    const uint64_t per = state_bytes(h->K, h->tpl_rows - 1);
    if (int rc = l->state.reserve((size_t)(per * l->C))) return rc;
    l->K = h->K;
    l->tpl_len = h->tpl_rows - 1;
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

struct PushPlan {
    std::vector<SpotLiveChan> chan;
    uint32_t rows = 0, max_n = 0, max_frames = 0, max_row = 0;  // windows completed; the largest count, frame count and [kept | chunk] row
};

// what a push with these counts does, from the counts alone; everything a push can refuse for its counts is refused here
int plan_push(const sr_spot_live *l, const uint32_t *n, uint32_t n_all, PushPlan *pl)
{
    const sr_engine *h = l->h;
    pl->chan.assign(l->C, SpotLiveChan{});
    for (uint32_t c = 0; c < l->C; c++) {
        const uint32_t cnt = n ? n[c] : n_all;
        SpotLiveChan &ch = pl->chan[c];
        if (cnt > l->chunk_max) return fail(SR_ERR_BAD_ARG, "count of channel " + std::to_string(c) + " exceeds chunk_max");
        if (cnt && l->bound[c] != h->store_serial)
            return fail(SR_ERR_BAD_ARG, "the template store changed: end channel " + std::to_string(c) + " before pushing to it");
        uint32_t nf = cnt;
        if (l->pcm) {  // frame j exists once 1 + j * hop + frame_len samples have arrived; the row starts at frame x0's predecessor
            const uint32_t total = l->kept[c] + cnt;
            nf = total >= 1 + h->frame_len ? (total - 1 - h->frame_len) / h->hop + 1 : 0;
            ch.kept = l->kept[c];
            ch.n_samp = cnt;
            ch.drop = nf * h->hop;
            if (cnt) pl->max_row = std::max(pl->max_row, total);
        }
        if ((uint64_t)l->frames[c] + nf > kSpotLiveMaxFrames)
            return fail(SR_ERR_BAD_ARG, "channel " + std::to_string(c) + " would pass 0xFFFF0000 frames: end it first");
        ch.x0 = l->frames[c];
        ch.n = nf;
        ch.row_base = pl->rows;
        ch.first_win = ch.x0 / l->win;
        pl->rows += windows_done(ch.x0, nf, l->win);
        pl->max_n = std::max(pl->max_n, cnt);
        pl->max_frames = std::max(pl->max_frames, nf);
    }
    return SR_OK;
}

int check_outputs(const PushPlan &pl, uint32_t max_rows, const void *hits, const sr_spot_win *wins)
{
    if (max_rows < pl.rows)
        return fail(SR_ERR_BAD_ARG, "max_rows " + std::to_string(max_rows) + " is below the " + std::to_string(pl.rows) +
                                        " window rows of this push (sr_spot_live_rows)");
    if (pl.rows && (!hits || !wins)) return fail(SR_ERR_BAD_ARG, "null argument");
    return SR_OK;
}

// the spotter over the new frames of every channel, enqueued on s; the plan goes up first
int launch_push(sr_spot_live *l, const PushPlan &pl, const int16_t *d_mfcc, uint64_t row_stride, sr_spot_hit *d_hits, uint32_t *d_scores,
                hipStream_t s)
{
    const sr_engine *h = l->h;
    if (!pl.max_frames) return SR_OK;
    launch_spot_live(SpotLiveArgs{d_mfcc, row_stride, l->d_chan.p, l->C, h->tpl.p, h->tpl_frames.p, h->tpl_valid.p, l->K, h->tpl_stride,
                                  l->tpl_len, l->win, l->state.p, l->chan_stride, d_hits, d_scores},
                     s);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

// (a pageable source is staged before the call returns: the plan may go out of scope)
int upload_plan(sr_spot_live *l, const PushPlan &pl, hipStream_t s)
{
    HIP_TRY(hipMemcpyAsync(l->d_chan.p, pl.chan.data(), (size_t)l->C * sizeof(SpotLiveChan), hipMemcpyHostToDevice, s));
    return SR_OK;
}

// PCM sessions: [kept | chunk] rows, the frame kernel over them as sr_mfcc_batch_dev launches it, the samples to keep
int launch_front_end(sr_spot_live *l, const PushPlan &pl, const uint16_t *d_pcm, uint64_t pcm_stride, hipStream_t s)
{
    return live_pcm_front_end(l->h, l->d_chan.p, pl.chan, l->mid, pl.max_row, pl.max_frames, d_pcm, pcm_stride, l->keep.p, l->keep_stride,
                              l->stage.p, l->stage_stride, l->recs.p, l->feat.p, s);
}

// the push is enqueued: the mirror follows, and the caller learns which window each row holds
void advance(sr_spot_live *l, const PushPlan &pl, sr_spot_win *wins, uint32_t *n_rows)
{
    for (uint32_t c = 0; c < l->C; c++) {
        const SpotLiveChan &ch = pl.chan[c];
        const uint32_t done = windows_done(ch.x0, ch.n, l->win);
        for (uint32_t i = 0; i < done; i++) wins[ch.row_base + i] = sr_spot_win{c, ch.first_win + i};
        l->frames[c] = ch.x0 + ch.n;
        if (l->pcm) l->kept[c] = ch.kept + ch.n_samp - ch.drop;
    }
    if (n_rows) *n_rows = pl.rows;
}

int mark_push(sr_spot_live *l, hipStream_t s)
{
    HIP_TRY(hipEventRecord(l->ev_last, s));
    l->pending = true;
    l->last_stream = s;
    return SR_OK;
}

// the channels' state belongs to one push at a time: a push on another stream than the last one's runs behind it
int order_after_last_push(sr_spot_live *l, hipStream_t s)
{
    if (!l->pending || s == l->last_stream) return SR_OK;
    HIP_TRY(hipStreamWaitEvent(s, l->ev_last, 0));
    return SR_OK;
}

int check_frames_in(const sr_spot_live *l, const PushPlan &pl, const int16_t *mfcc, uint64_t row_stride, bool device)
{
    if (l->pcm) return fail(SR_ERR_BAD_ARG, "a PCM session takes samples (sr_spot_live_push_pcm)");
    if (!pl.max_n) return SR_OK;
    if (!mfcc) return fail(SR_ERR_BAD_ARG, "null argument");
    if ((uint64_t)pl.max_n * kCoef > row_stride) return fail(SR_ERR_BAD_ARG, "a count exceeds row_stride");
    if (device && (((uintptr_t)mfcc & 7) || (row_stride & 3))) return fail(SR_ERR_BAD_ARG, "mfcc must be 8-byte aligned, row_stride % 4 == 0");
    if (!device && ((uintptr_t)mfcc & 1)) return fail(SR_ERR_BAD_ARG, "mfcc must be 2-byte aligned");
    return SR_OK;
}

int check_pcm_in(const sr_spot_live *l, const PushPlan &pl, const uint16_t *pcm, uint64_t pcm_stride, bool device)
{
    if (!l->pcm) return fail(SR_ERR_BAD_ARG, "a feature session takes frames (sr_spot_live_push)");
    if (!pl.max_n) return SR_OK;
    if (!pcm) return fail(SR_ERR_BAD_ARG, "null pcm");
    if (pl.max_n > pcm_stride) return fail(SR_ERR_BAD_ARG, "a count exceeds pcm_stride");
    if (device && (((uintptr_t)pcm & 15) || (pcm_stride & 7))) return fail(SR_ERR_BAD_ARG, "pcm must be 16-byte aligned, stride % 8 == 0");
    if (!device && ((uintptr_t)pcm & 1)) return fail(SR_ERR_BAD_ARG, "pcm must be 2-byte aligned");
    return SR_OK;
}

// host forms: the engine's device copies of the outputs
int reserve_host_outputs(sr_engine *h, const PushPlan &pl, bool scores)
{
    const size_t n_rec = (size_t)std::max(pl.rows, 1u) * h->K;
    if (int rc = h->s_spot_hits.reserve(n_rec)) return rc;
    if (scores)
        if (int rc = h->s_spot_scores.reserve(n_rec)) return rc;
    return SR_OK;
}

}  // namespace

extern "C" {

int sr_spot_live_geometry(uint32_t tpl_rows, uint32_t K, uint32_t chunk_max, uint32_t win_frames, uint32_t out[3])
{
    if (!out || !tpl_rows || tpl_rows > 16383 || !K || !chunk_max || !win_frames) return fail(SR_ERR_BAD_ARG, "null / zero argument");
    const LdsBudget mi355x;  // no device: MI355X's figures
    out[0] = (uint32_t)(((uint64_t)chunk_max + win_frames - 1) / win_frames);  // entering on a window's last frame
    out[1] = (uint32_t)std::min<uint64_t>(state_bytes(K, tpl_rows), 0xFFFFFFFFull);
    out[2] = spot_max_tpl(mi355x);
    return SR_OK;
}

int sr_spot_live_open(sr_engine *h, uint32_t n_channels, uint32_t chunk_max, uint32_t win_frames, const uint32_t *mid, sr_spot_live **out)
{
    if (!h || !out) return fail(SR_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (!n_channels || n_channels > kSpotLiveMaxChannels || !chunk_max || !win_frames)
        return fail(SR_ERR_BAD_ARG, "n_channels not in 1..65535 / chunk_max 0 / win_frames 0");
    if (int rc = check_store(h)) return rc;
    const uint32_t R = h->cfg.max_frames;
    if (mid) {
        if (((uint64_t)chunk_max + h->hop - 1) / h->hop > R)
            return fail(SR_ERR_BAD_ARG, "a push of chunk_max samples could complete more than max_frames frames");
        for (uint32_t c = 0; c < n_channels; c++)
            if (mid[c] > 0xFFFFu) return fail(SR_ERR_BAD_ARG, "mid exceeds the u16 sample range");
        if (int rc = check_batch(h, n_channels)) return rc;
    } else if (chunk_max > R) {
        return fail(SR_ERR_BAD_ARG, "chunk_max not in 1..max_frames");
    }
    uint32_t origin = 0;
    if (int rc = spot_live_origin(&origin)) return rc;
    ENTER_DEVICE(h);
    sr_spot_live *l = new sr_spot_live();
    l->h = h;
    l->C = n_channels;
    l->chunk_max = chunk_max;
    l->win = win_frames;
    l->pcm = mid != nullptr;
    l->bound.assign(n_channels, h->store_serial);
    l->frames.assign(n_channels, origin);
    l->kept.assign(n_channels, 0);
    int rc = relayout(l);
    for (uint32_t c = 0; c < n_channels && origin && !rc; c++) rc = unreachable_before_origin(l, c, nullptr);
    if (!rc && origin && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(SR_ERR_HIP, "hipStreamSynchronize failed");
    if (!rc) rc = l->d_chan.reserve(n_channels);
    if (!rc && mid) {
        l->mid.assign(mid, mid + n_channels);
        l->keep_stride = live_pcm_keep_stride(h);
        l->stage_stride = live_pcm_stage_stride(h, chunk_max);
        rc = l->keep.reserve((size_t)n_channels * l->keep_stride);
        if (!rc) rc = l->stage.reserve((size_t)n_channels * l->stage_stride);
        if (!rc) rc = l->recs.reserve(n_channels);
        if (!rc) rc = l->feat.reserve(h->mfcc_elems(n_channels));
    }
    if (!rc && hipEventCreateWithFlags(&l->ev_last, hipEventDisableTiming) != hipSuccess) rc = fail(SR_ERR_HIP, "hipEventCreate failed");
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
    if (l->pending) (void)hipEventSynchronize(l->ev_last);
    l->state.release();
    l->d_chan.release();
    l->keep.release();
    l->stage.release();
    l->recs.release();
    l->feat.release();
    if (l->ev_last) (void)hipEventDestroy(l->ev_last);
    delete l;
}

uint32_t sr_spot_live_windows(uint32_t win_frames, const uint32_t *frames_before, const uint32_t *n_new, uint32_t n_channels)
{
    if (!win_frames || !frames_before || !n_new) return 0;
    uint64_t rows = 0;
    for (uint32_t c = 0; c < n_channels; c++) {
        if ((uint64_t)frames_before[c] + n_new[c] > kSpotLiveMaxFrames) return 0;
        rows += windows_done(frames_before[c], n_new[c], win_frames);
    }
    return (uint32_t)std::min<uint64_t>(rows, 0xFFFFFFFFull);
}

uint32_t sr_spot_live_rows(const sr_spot_live *l, const uint32_t *n, uint32_t n_all)
{
    if (!l) return 0;
    PushPlan pl;
    return plan_push(l, n, n_all, &pl) ? 0 : pl.rows;
}

int sr_spot_live_push_dev(sr_spot_live *l, const int16_t *d_mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                          sr_spot_hit *d_hits, uint32_t *d_scores, sr_spot_win *wins, uint32_t *n_rows, void *stream)
{
    if (!l) return fail(SR_ERR_BAD_ARG, "null session");
    PushPlan pl;
    int rc = plan_push(l, n, n_all, &pl);
    if (!rc) rc = check_frames_in(l, pl, d_mfcc, row_stride, true);
    if (!rc) rc = check_outputs(pl, max_rows, d_hits, wins);
    if (rc) return rc;
    ENTER_DEVICE(l->h);
    const hipStream_t s = (hipStream_t)stream;
    if (pl.max_frames) {
        if ((rc = order_after_last_push(l, s))) return rc;
        if ((rc = upload_plan(l, pl, s))) return rc;
        if ((rc = launch_push(l, pl, d_mfcc, row_stride, d_hits, d_scores, s))) return rc;
    }
    advance(l, pl, wins, n_rows);
    return pl.max_frames ? mark_push(l, s) : SR_OK;
}

int sr_spot_live_push(sr_spot_live *l, const int16_t *mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                      sr_spot_hit *hits, uint32_t *scores, sr_spot_win *wins, uint32_t *n_rows)
{
    if (!l) return fail(SR_ERR_BAD_ARG, "null session");
    PushPlan pl;
    int rc = plan_push(l, n, n_all, &pl);
    if (!rc) rc = check_frames_in(l, pl, mfcc, row_stride, false);
    if (!rc) rc = check_outputs(pl, max_rows, hits, wins);
    if (rc) return rc;
    sr_engine *h = l->h;
    ENTER_HOST_CALL(h);
    if (pl.max_frames) {
        const size_t ds = (size_t)pl.max_frames * kCoef;  // device rows hold the largest count
        if ((rc = h->s_mfcc.reserve((size_t)l->C * ds))) return rc;
        if ((rc = reserve_host_outputs(h, pl, scores != nullptr))) return rc;
        for (uint32_t c = 0; c < l->C; c++)  // count by count: nothing past n[c] of a caller's row is read
            if (pl.chan[c].n) COPY_UP(h->s_mfcc.p + c * ds, mfcc + (size_t)c * row_stride, (size_t)pl.chan[c].n * kCoef * 2);
        if ((rc = order_after_last_push(l, nullptr))) return rc;
        if ((rc = upload_plan(l, pl, nullptr))) return rc;
        if ((rc = launch_push(l, pl, h->s_mfcc.p, ds, h->s_spot_hits.p, scores ? h->s_spot_scores.p : nullptr, nullptr))) return rc;
    }
    advance(l, pl, wins, n_rows);
    if (pl.max_frames && (rc = mark_push(l, nullptr))) return rc;
    if (pl.rows) {
        COPY_DOWN(hits, h->s_spot_hits.p, (size_t)pl.rows * h->K * sizeof(sr_spot_hit));
        if (scores) COPY_DOWN(scores, h->s_spot_scores.p, (size_t)pl.rows * h->K * 4);
    }
    return SR_OK;
}

int sr_spot_live_push_pcm_dev(sr_spot_live *l, const uint16_t *d_pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                              uint32_t max_rows, sr_spot_hit *d_hits, uint32_t *d_scores, sr_spot_win *wins, uint32_t *n_rows, void *stream)
{
    if (!l) return fail(SR_ERR_BAD_ARG, "null session");
    PushPlan pl;
    int rc = plan_push(l, n, n_all, &pl);
    if (!rc) rc = check_pcm_in(l, pl, d_pcm, pcm_stride, true);
    if (!rc) rc = check_outputs(pl, max_rows, d_hits, wins);
    if (rc) return rc;
    sr_engine *h = l->h;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    if (pl.max_n) {
        if ((rc = order_after_last_push(l, s))) return rc;
        if ((rc = upload_plan(l, pl, s))) return rc;
        if ((rc = launch_front_end(l, pl, d_pcm, pcm_stride, s))) return rc;
        if ((rc = launch_push(l, pl, l->feat.p, (uint64_t)h->cfg.max_frames * kCoef, d_hits, d_scores, s))) return rc;
    }
    advance(l, pl, wins, n_rows);
    return pl.max_n ? mark_push(l, s) : SR_OK;
}

int sr_spot_live_push_pcm(sr_spot_live *l, const uint16_t *pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                          sr_spot_hit *hits, uint32_t *scores, sr_spot_win *wins, uint32_t *n_rows)
{
    if (!l) return fail(SR_ERR_BAD_ARG, "null session");
    PushPlan pl;
    int rc = plan_push(l, n, n_all, &pl);
    if (!rc) rc = check_pcm_in(l, pl, pcm, pcm_stride, false);
    if (!rc) rc = check_outputs(pl, max_rows, hits, wins);
    if (rc) return rc;
    sr_engine *h = l->h;
    ENTER_HOST_CALL(h);
    if (pl.max_n) {
        const uint64_t ds = dev_pitch(pl.max_n);
        if ((rc = h->s_pcm.reserve((size_t)l->C * ds))) return rc;
        if ((rc = reserve_host_outputs(h, pl, scores != nullptr))) return rc;
        for (uint32_t c = 0; c < l->C; c++)  // count by count: nothing past n[c] of a caller's row is read
            if (pl.chan[c].n_samp) COPY_UP(h->s_pcm.p + c * ds, pcm + (size_t)c * pcm_stride, (size_t)pl.chan[c].n_samp * 2);
        if ((rc = order_after_last_push(l, nullptr))) return rc;
        if ((rc = upload_plan(l, pl, nullptr))) return rc;
        if ((rc = launch_front_end(l, pl, h->s_pcm.p, ds, nullptr))) return rc;
        if ((rc = launch_push(l, pl, l->feat.p, (uint64_t)h->cfg.max_frames * kCoef, h->s_spot_hits.p, scores ? h->s_spot_scores.p : nullptr,
                              nullptr)))
            return rc;
    }
    advance(l, pl, wins, n_rows);
    if (pl.max_n && (rc = mark_push(l, nullptr))) return rc;
    if (pl.rows) {
        COPY_DOWN(hits, h->s_spot_hits.p, (size_t)pl.rows * h->K * sizeof(sr_spot_hit));
        if (scores) COPY_DOWN(scores, h->s_spot_scores.p, (size_t)pl.rows * h->K * 4);
    }
    return SR_OK;
}

int sr_spot_live_end(sr_spot_live *l, const uint32_t *channels, uint32_t n_ch, sr_spot_hit *hits, sr_spot_win *wins, uint32_t *n_rows)
{
    if (!l || (n_ch && !channels)) return fail(SR_ERR_BAD_ARG, "null argument");
    for (uint32_t i = 0; i < n_ch; i++)
        if (channels[i] >= l->C) return fail(SR_ERR_BAD_ARG, "channel " + std::to_string(channels[i]) + " is past the session's last");
    sr_engine *h = l->h;
    uint32_t origin = 0;
    if (int rc = spot_live_origin(&origin)) return rc;
    const bool changed = l->layout_serial != h->store_serial;  // then every channel that holds state is bound to a store that is gone
    if (changed)
        if (int rc = check_store(h)) return rc;
    // One entry per DISTINCT listed channel, in the order of first mention: a channel listed again is fresh by then, has no
    // open window and needs no second reset (and k_spot_live_flush gives every entry threads of its own, which nothing orders).
    std::vector<SpotLiveFlush> list;
    std::vector<uint8_t> seen(l->C, 0);
    uint32_t rows = 0;
    for (uint32_t i = 0; i < n_ch; i++) {
        const uint32_t c = channels[i], N = l->frames[c];
        if (seen[c]) continue;
        seen[c] = 1;
        const bool open = !changed && l->bound[c] == l->layout_serial && N % l->win != 0;
        list.push_back(SpotLiveFlush{c, open ? rows++ : 0xFFFFFFFFu, N / l->win, 0u});
    }
    if (rows && (!hits || !wins)) return fail(SR_ERR_BAD_ARG, "null argument");
    if (!n_ch) {
        if (n_rows) *n_rows = 0;
        return SR_OK;
    }
    ENTER_HOST_CALL(h);
    if (l->pending) {
        HIP_TRY(hipEventSynchronize(l->ev_last));
        l->pending = false;
    }
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
    for (const SpotLiveFlush &f : list) {
        if (f.row != 0xFFFFFFFFu) wins[f.row] = sr_spot_win{f.channel, f.wid};
        l->frames[f.channel] = origin;
        l->kept[f.channel] = 0;
        l->bound[f.channel] = h->store_serial;
    }
    if (n_rows) *n_rows = rows;
    return SR_OK;
}

}  // extern "C"
