// Live sessions (include/sr_engine.h, "live sessions"): audio that arrives in chunks, the stream VAD's state and each
// channel's recent samples kept on the device between pushes (k_live.hip), every ended segment recognised by the frame kernel,
// DTW, the slot scan and N-best exactly as sr_recognize_stream does.  EXTENSION, NO REFERENCE COUNTERPART.
//
// The host knows every count, hence every channel's received total, its consumed frames and whether its noise head is
// complete (the mirror below); only the VAD state and the number of ended segments live on the device alone.
#include "sr_host_call.h"

using namespace sr;

struct sr_live {
    sr_engine *h = nullptr;
    uint32_t C = 0, chunk_max = 0, ring_blocks = 0, ev_slots = 0;
    uint64_t ring_stride = 0;
    bool given = false;             // thresholds handed in at open (the scan then takes the form for any mid value)
    std::vector<sr_atap> atap0;     // ... those thresholds
    std::vector<uint64_t> received, frames;  // host mirror of LiveChan::received / next_frame
    std::vector<uint8_t> head_done;          // ... of atap_set
    DevBuf<LiveChan> chan;
    DevBuf<uint16_t> ring;
    DevBuf<LiveEvent> events;
    DevBuf<uint32_t> ev_count, d_n;
    DevBuf<sr_live_seg> o_segs;     // host form: device copies of its segment output and count
    DevBuf<uint32_t> o_count;
    hipEvent_t ev_last = nullptr;   // end of the last push (sr_live_end / sr_live_close wait for it)
    bool pending = false;
};

namespace {

constexpr uint32_t kLiveChunkMax = 1u << 24;

uint64_t frames_of(uint64_t recv, uint32_t frame_len, uint32_t hop)  // VAD.C:121, as stream_frames()
{
    return recv > frame_len ? (recv - frame_len + hop - 1) / hop : 0;
}

// ring samples per channel.  At an END event in frame i the oldest sample still needed is start - kStreamLead with
// end - start <= (max_frames + 1) * hop for a segment that is read at all, and the newest sample written lies below
// i * hop + frame_len + chunk_max + 1 (frame i was not consumable before the push): a span of at most
// (max_frames + s_durmax + 1) * hop + kStreamLead + chunk_max samples, plus a block at either end for whole blocks.  The
// second term keeps the noise head, and the frames taken from 0 on when it completes, inside the first turn.
uint64_t ring_samples(const ConfigFraming &g, uint32_t chunk_max)
{
    const uint64_t a = (uint64_t)(g.max_frames + g.s_durmax + 4) * g.hop + kStreamLead + chunk_max;
    const uint64_t b = (uint64_t)g.noise_len + g.frame_len + chunk_max;
    return (std::max(a, b) + g.hop - 1) / g.hop * g.hop;
}

// most frames one push of chunk_max samples can make consumable: ceil(chunk_max / hop) in the steady state, every frame of
// noise_len - 1 + chunk_max samples when the push completes the noise head
uint64_t frames_per_push(const ConfigFraming &g, uint32_t chunk_max)
{
    const uint64_t steady = ((uint64_t)chunk_max + g.hop - 1) / g.hop;
    return std::max(steady, frames_of((uint64_t)g.noise_len - 1 + chunk_max, g.frame_len, g.hop));
}

ConfigFraming framing_of(const sr_engine *h)
{
    return ConfigFraming{h->frame_len, h->hop, h->v_durmin, h->s_durmax, h->noise_len, h->cfg.max_frames};
}

// development hook "live_origin" (testing build; 0 otherwise): the position a fresh channel starts at.  Refused unless it is a
// whole number of hops in a session with given thresholds (a noise head is defined from position 0).
int live_origin(const sr_live *l, uint64_t *origin)
{
    const int64_t v = dev_hook(kHookLiveOrigin);
    if (v && (v < 0 || v % l->h->hop != 0 || !l->given))
        return fail(SR_ERR_BAD_ARG, "development hook live_origin: a positive multiple of hop, in a session opened with atap_in");
    *origin = (uint64_t)v;
    return SR_OK;
}

LiveChan fresh_chan(const sr_live *l, uint32_t c, uint64_t origin)
{
    LiveChan s{};
    if (l->given) {
        s.atap = l->atap0[c];
        s.atap_set = 1;
    }
    s.received = origin;  // as if `origin` samples had been consumed in silence
    s.next_frame = origin / l->h->hop;
    return s;
}

void fresh_mirror(sr_live *l, uint32_t c, uint64_t origin)
{
    l->received[c] = origin;
    l->frames[c] = origin / l->h->hop;
    l->head_done[c] = l->given ? 1 : 0;
}

// new whole frames of channel c after cnt more samples (0 while its noise head is incomplete)
uint64_t new_frames(const sr_live *l, uint32_t c, uint32_t cnt)
{
    const uint64_t recv = l->received[c] + cnt;
    if (!l->head_done[c] && recv < l->h->noise_len) return 0;
    const uint64_t F = frames_of(recv, l->h->frame_len, l->h->hop);
    return F > l->frames[c] ? F - l->frames[c] : 0;
}

// records [0, n) of a push recognised: stream_recognize (sr_stream.cpp) with the ring-aware record builder
int live_recognize(sr_live *l, const sr_live_seg *d_segs, const uint32_t *d_count, uint32_t n, sr_result *d_results,
                   uint32_t *d_scores, int16_t *d_mfcc, hipStream_t s, const NbestOut *nb, uint32_t chunk, uint64_t row)
{
    sr_engine *h = l->h;
    const uint32_t R = h->cfg.max_frames, nc = h->nc, K = h->K;
    bool counted = false;
    for (uint32_t r0 = 0; r0 < n; r0 += chunk) {
        const uint32_t m = std::min(chunk, n - r0);
        LiveRecArgs ra{l->chan.p, l->ring.p, l->ring_stride, d_segs, d_count, r0, h->frame_len, h->hop, R, h->s_st_rows.p, row, h->s_st_recs.p};
        launch_live_records(ra, m, s);
        int16_t *mc = d_mfcc ? d_mfcc + (size_t)r0 * R * nc : h->s_mfcc.p;
        launch_mfcc(mfcc_args(h, h->s_st_rows.p, row, m, h->s_st_recs.p, mc), mfcc_mag_tab(h), s);
        DtwArgs da = dtw_args(h, mc, h->s_st_recs.p, nullptr, m, d_scores ? d_scores + (size_t)r0 * K : h->s_scores.p,
                              d_results ? d_results + r0 : h->s_results.p);
        if (launch_dtw_auto(h, da, 0, s, s)) counted = true;
        else launch_argmin(da, s);
        if (nb) launch_nbest(nbest_args(h, da.scores, m, *nb, r0), s);
    }
    if (counted) HIP_TRY(hipEventRecord(h->ev_cells, s));
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

struct PushPlan {
    uint32_t max_n = 0;              // the largest count
    uint32_t head_c0 = 0, head_n = 0;  // channels whose noise head this push completes lie in [head_c0, head_c0 + head_n)
    uint32_t chunk = 0;              // records per recognition chunk
    uint64_t row = 0;                // samples per record row
};

// argument checks shared by both forms; everything a push can refuse is refused here, before any state changes
int check_push(const sr_live *l, const void *pcm, uint64_t pcm_stride, bool device, const uint32_t *n, uint32_t n_all,
               uint32_t max_segs, const void *segs, uint32_t n_best, const void *nbest, const void *results, const void *scores,
               const void *mfcc, PushPlan *pl)
{
    if (!l) return fail(SR_ERR_BAD_ARG, "null session");
    const sr_engine *h = l->h;
    uint32_t c_lo = l->C, c_hi = 0;
    for (uint32_t c = 0; c < l->C; c++) {
        const uint32_t cnt = n ? n[c] : n_all;
        if (cnt > l->chunk_max) return fail(SR_ERR_BAD_ARG, "count of channel " + std::to_string(c) + " exceeds chunk_max");
        pl->max_n = std::max(pl->max_n, cnt);
        if (!l->head_done[c] && l->received[c] + cnt >= h->noise_len) {
            c_lo = std::min(c_lo, c);
            c_hi = c;
        }
    }
    if (c_lo < l->C) {
        pl->head_c0 = c_lo;
        pl->head_n = c_hi - c_lo + 1;
    }
    if (pl->max_n) {
        if (!pcm) return fail(SR_ERR_BAD_ARG, "null pcm");
        if (pl->max_n > pcm_stride) return fail(SR_ERR_BAD_ARG, "a count exceeds pcm_stride");
        if (device && (((uintptr_t)pcm & 15) || (pcm_stride & 7))) return fail(SR_ERR_BAD_ARG, "pcm must be 16-byte aligned, stride % 8 == 0");
        if (!device && ((uintptr_t)pcm & 1)) return fail(SR_ERR_BAD_ARG, "pcm must be 2-byte aligned");
    }
    if (max_segs && !segs) return fail(SR_ERR_BAD_ARG, "null argument");
    const bool recog = results || n_best;
    if ((scores || mfcc) && !recog) return fail(SR_ERR_BAD_ARG, "scores / mfcc need results");
    if (n_best) {
        if (int rc = check_nbest(h, n_best, nbest)) return rc;
    } else if (nbest) {
        return fail(SR_ERR_BAD_ARG, "n_best must be 1.." + std::to_string(SR_NBEST_MAX) + " with an N-best output");
    }
    if (recog && !h->K) return fail(SR_ERR_NO_TEMPLATES, "no templates set");
    const uint32_t bound = sr_live_event_bound(l, n, n_all);
    if (max_segs < bound)
        return fail(SR_ERR_BAD_ARG, "max_segs " + std::to_string(max_segs) + " is below this push's event bound " + std::to_string(bound) +
                                        " (sr_live_event_bound): records are never dropped");
    pl->row = ((uint64_t)kStreamLead + (uint64_t)(h->cfg.max_frames + 1) * h->hop + 16 + 7) & ~7ull;
    return SR_OK;
}

// scratch of the recognition launches over n records, reserved before anything is enqueued
int reserve_recognition(sr_live *l, uint32_t n, bool own_results, bool own_scores, bool own_mfcc, PushPlan *pl)
{
    sr_engine *h = l->h;
    int rc;
    pl->chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, (64ull << 20) / pl->row));  // rows: 128 MB at most
    if ((rc = check_batch(h, pl->chunk))) return rc;
    if ((rc = h->s_st_rows.reserve((size_t)pl->chunk * pl->row))) return rc;
    if ((rc = h->s_st_recs.reserve(pl->chunk))) return rc;
    if (own_mfcc && (rc = h->s_mfcc.reserve((size_t)pl->chunk * h->cfg.max_frames * h->nc))) return rc;
    if (own_scores && (rc = h->s_scores.reserve((size_t)pl->chunk * h->K))) return rc;
    if (own_results && (rc = h->s_results.reserve(pl->chunk))) return rc;
    return SR_OK;
}

// append, the thresholds of completed noise heads, scan and compaction on `s`
int live_segment(sr_live *l, const uint16_t *d_pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all, const PushPlan &pl,
                 uint32_t max_segs, sr_live_seg *d_segs, uint32_t *d_count, hipStream_t s)
{
    sr_engine *h = l->h;
    LiveArgs a{};
    a.chan = l->chan.p;
    a.ring = l->ring.p;
    a.ring_stride = l->ring_stride;
    a.ring_blocks = l->ring_blocks;
    a.C = l->C;
    a.pcm = d_pcm;
    a.pcm_stride = pcm_stride;
    a.n_all = n_all;
    if (n) {  // (a pageable source is staged before the call returns: the caller's array is free again)
        HIP_TRY(hipMemcpyAsync(l->d_n.p, n, (size_t)l->C * 4, hipMemcpyHostToDevice, s));
        a.n = l->d_n.p;
    }
    a.head_vad = h->s_st_vad.p;
    a.head_c0 = pl.head_c0;
    a.noise_len = h->noise_len;
    a.frame_len = h->frame_len;
    a.hop = h->hop;
    a.v_durmin = h->v_durmin;
    a.s_durmax = h->s_durmax;
    a.max_frames = h->cfg.max_frames;
    a.events = l->events.p;
    a.ev_count = l->ev_count.p;
    a.ev_slots = l->ev_slots;
    a.segs = d_segs;
    a.max_segs = max_segs;
    a.count = d_count;
    if (pl.max_n) launch_live_append(a, s);
    // noise_atap over the heads this push completed: the VAD kernel itself over the noise_len samples, as stream_segment does
    // (a head lies in the first turn of its ring, unwrapped; records of channels in between are not read)
    if (pl.head_n)
        launch_vad(vad_args(h, l->ring.p + (uint64_t)pl.head_c0 * l->ring_stride, l->ring_stride, h->noise_len, h->noise_len, pl.head_n,
                            h->s_st_vad.p),
                   s);
    launch_live_scan(a, !l->given, s);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

// the push is enqueued: the mirror follows the device's records
void advance_mirror(sr_live *l, const uint32_t *n, uint32_t n_all)
{
    const sr_engine *h = l->h;
    for (uint32_t c = 0; c < l->C; c++) {
        l->received[c] += n ? n[c] : n_all;
        if (!l->head_done[c] && l->received[c] >= h->noise_len) l->head_done[c] = 1;
        if (l->head_done[c]) l->frames[c] = std::max(l->frames[c], frames_of(l->received[c], h->frame_len, h->hop));
    }
}

int mark_push(sr_live *l, hipStream_t s)
{
    HIP_TRY(hipEventRecord(l->ev_last, s));
    l->pending = true;
    return SR_OK;
}

}  // namespace

uint32_t sr_live_events_in_frames(uint32_t v_durmin, uint32_t s_durmax, uint64_t frames)
{
    // From the last tail state one quiet frame ends a segment; the next END needs max(v_durmin, 2) loud frames up to the START
    // (the count is checked on a loud frame met in the onset, VAD.C:173-181) and max(s_durmax, 2) quiet ones up to the END
    // (VAD.C:196-207).  tests/test_live_session.py holds this to an exhaustive search over the state machine.
    if (!frames) return 0;
    const uint64_t cycle = (uint64_t)std::max(v_durmin, 2u) + std::max(s_durmax, 2u);
    return (uint32_t)std::min<uint64_t>(1 + (frames - 1) / cycle, 0xFFFFFFFFull);
}

int sr_live_geometry(const sr_config *cfg, uint32_t chunk_max, uint32_t out[3])
{
    if (!cfg || !out || chunk_max < 1 || chunk_max > kLiveChunkMax) return fail(SR_ERR_BAD_ARG, "null argument / chunk_max not in 1..2^24");
    ConfigFraming g;
    if (int rc = config_framing(cfg, &g)) return rc;
    const uint64_t ring = ring_samples(g, chunk_max);
    const uint32_t slots = sr_live_events_in_frames(g.v_durmin, g.s_durmax, frames_per_push(g, chunk_max));
    out[0] = (uint32_t)ring;
    out[1] = slots;
    out[2] = (uint32_t)(ring * 2 + sizeof(LiveChan) + (uint64_t)slots * sizeof(LiveEvent) + 2 * sizeof(uint32_t));
    return SR_OK;
}

int sr_live_open(sr_engine *h, uint32_t n_channels, uint32_t chunk_max, const sr_atap *atap_in, sr_live **out)
{
    if (!h || !out) return fail(SR_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (!n_channels || chunk_max < 1 || chunk_max > kLiveChunkMax) return fail(SR_ERR_BAD_ARG, "n_channels 0 / chunk_max not in 1..2^24");
    ENTER_DEVICE(h);
    const ConfigFraming g = framing_of(h);
    sr_live *l = new sr_live();
    l->h = h;
    l->C = n_channels;
    l->chunk_max = chunk_max;
    l->ring_stride = ring_samples(g, chunk_max);
    l->ring_blocks = (uint32_t)(l->ring_stride / g.hop);
    l->ev_slots = sr_live_events_in_frames(g.v_durmin, g.s_durmax, frames_per_push(g, chunk_max));
    l->given = atap_in != nullptr;
    if (atap_in) l->atap0.assign(atap_in, atap_in + n_channels);
    l->received.assign(n_channels, 0);
    l->frames.assign(n_channels, 0);
    l->head_done.assign(n_channels, 0);
    uint64_t origin = 0;
    int rc = live_origin(l, &origin);
    std::vector<LiveChan> init(n_channels);
    for (uint32_t c = 0; c < n_channels && !rc; c++) {
        init[c] = fresh_chan(l, c, origin);
        fresh_mirror(l, c, origin);
    }
    if (!rc) rc = l->chan.reserve(n_channels);
    if (!rc) rc = l->ring.reserve((size_t)n_channels * l->ring_stride);
    if (!rc) rc = l->events.reserve((size_t)n_channels * l->ev_slots);
    if (!rc) rc = l->ev_count.reserve(n_channels);
    if (!rc) rc = l->d_n.reserve(n_channels);
    if (!rc) rc = l->o_count.reserve(1);
    if (!rc && hipEventCreateWithFlags(&l->ev_last, hipEventDisableTiming) != hipSuccess) rc = fail(SR_ERR_HIP, "hipEventCreate failed");
    if (!rc && hipMemcpy(l->chan.p, init.data(), (size_t)n_channels * sizeof(LiveChan), hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(SR_ERR_HIP, "hipMemcpy failed");
    if (rc) {
        (void)hipGetLastError();
        sr_live_close(l);
        return rc;
    }
    *out = l;
    return SR_OK;
}

void sr_live_close(sr_live *l)
{
    if (!l) return;
    DeviceGuard guard;
    (void)guard.enter(l->h->device);
    if (l->pending) (void)hipEventSynchronize(l->ev_last);
    l->chan.release();
    l->ring.release();
    l->events.release();
    l->ev_count.release();
    l->d_n.release();
    l->o_segs.release();
    l->o_count.release();
    if (l->ev_last) (void)hipEventDestroy(l->ev_last);
    delete l;
}

uint32_t sr_live_event_bound(const sr_live *l, const uint32_t *n, uint32_t n_all)
{
    if (!l) return 0;
    uint64_t bound = 0;
    for (uint32_t c = 0; c < l->C; c++)
        bound += sr_live_events_in_frames(l->h->v_durmin, l->h->s_durmax, new_frames(l, c, n ? n[c] : n_all));
    return (uint32_t)std::min<uint64_t>(bound, 0xFFFFFFFFull);
}

int sr_live_push_dev(sr_live *l, const uint16_t *d_pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all, uint32_t max_segs,
                     sr_live_seg *d_segs, uint32_t *d_count, uint32_t n_best, sr_nbest_entry *d_nbest, uint32_t *d_n_matched,
                     sr_result *d_results, uint32_t *d_scores, int16_t *d_mfcc, void *stream)
{
    PushPlan pl;
    int rc = check_push(l, d_pcm, pcm_stride, true, n, n_all, max_segs, d_segs, n_best, d_nbest, d_results, d_scores, d_mfcc, &pl);
    if (rc) return rc;
    if (!d_count) return fail(SR_ERR_BAD_ARG, "null argument");
    sr_engine *h = l->h;
    const bool recog = (d_results || n_best) && max_segs;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    if ((rc = order_after_scratch_users(h, s))) return rc;
    if (pl.head_n && (rc = h->s_st_vad.reserve(pl.head_n))) return rc;
    if (recog && (rc = reserve_recognition(l, max_segs, !d_results, !d_scores, !d_mfcc, &pl))) return rc;
    if ((rc = live_segment(l, d_pcm, pcm_stride, n, n_all, pl, max_segs, d_segs, d_count, s))) return rc;
    advance_mirror(l, n, n_all);
    // the count stays on the device: every one of the max_segs slots is launched, those past the total as failed records
    const NbestOut nb{n_best, d_nbest, d_n_matched};
    if (recog) rc = live_recognize(l, d_segs, d_count, max_segs, d_results, d_scores, d_mfcc, s, n_best ? &nb : nullptr, pl.chunk, pl.row);
    const int rc_mark = mark_push(l, s), rc_scr = mark_scratch_user(h, s);
    return rc ? rc : (rc_mark ? rc_mark : rc_scr);
}

int sr_live_push(sr_live *l, const uint16_t *pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all, uint32_t max_segs,
                 sr_live_seg *segs, uint32_t n_best, sr_nbest_entry *nbest, uint32_t *n_matched, sr_result *results, uint32_t *scores,
                 int16_t *mfcc, uint32_t *n_segs)
{
    PushPlan pl;
    int rc = check_push(l, pcm, pcm_stride, false, n, n_all, max_segs, segs, n_best, nbest, results, scores, mfcc, &pl);
    if (rc) return rc;
    sr_engine *h = l->h;
    const bool recog = (results || n_best) && max_segs;
    const uint32_t R = h->cfg.max_frames, nc = h->nc, K = h->K;
    ENTER_HOST_CALL(h);
    // everything that can fail for want of memory comes before the first launch
    if (pl.head_n && (rc = h->s_st_vad.reserve(pl.head_n))) return rc;
    if ((rc = l->o_segs.reserve(std::max(1u, max_segs)))) return rc;
    if (recog) {
        if ((rc = h->s_results.reserve(max_segs))) return rc;
        if (scores && (rc = h->s_scores.reserve((size_t)max_segs * K))) return rc;
        if (mfcc && (rc = h->s_mfcc.reserve((size_t)max_segs * R * nc))) return rc;
        if (n_best && ((rc = h->s_nbest.reserve((size_t)max_segs * n_best)) || (rc = h->s_nmatched.reserve(max_segs)))) return rc;
        if ((rc = reserve_recognition(l, max_segs, false, !scores, !mfcc, &pl))) return rc;
    }
    uint64_t ds = 8;
    if (pl.max_n && (rc = stage_pcm(h, pcm, pcm_stride, pl.max_n, l->C, &ds))) return rc;
    if ((rc = live_segment(l, h->s_pcm.p, ds, n, n_all, pl, max_segs, l->o_segs.p, l->o_count.p, nullptr))) return rc;
    advance_mirror(l, n, n_all);
    if ((rc = mark_push(l, nullptr))) return rc;
    uint32_t total = 0;
    COPY_DOWN(&total, l->o_count.p, 4);  // syncs on the count
    total = std::min(total, max_segs);   // (never more: max_segs covers the bound)
    if (n_segs) *n_segs = total;
    if (total) COPY_DOWN(segs, l->o_segs.p, (size_t)total * sizeof(sr_live_seg));
    if (!recog || !total) return SR_OK;
    const NbestOut d_nb{n_best, h->s_nbest.p, h->s_nmatched.p};
    pl.chunk = std::min(pl.chunk, total);
    if ((rc = live_recognize(l, l->o_segs.p, l->o_count.p, total, h->s_results.p, scores ? h->s_scores.p : nullptr,
                             mfcc ? h->s_mfcc.p : nullptr, nullptr, n_best ? &d_nb : nullptr, pl.chunk, pl.row)))
        return rc;
    if (n_best) {
        COPY_DOWN(nbest, h->s_nbest.p, (size_t)total * n_best * sizeof(sr_nbest_entry));
        if (n_matched) COPY_DOWN(n_matched, h->s_nmatched.p, (size_t)total * 4);
    }
    if (results) COPY_DOWN(results, h->s_results.p, (size_t)total * sizeof(sr_result));
    if (scores) COPY_DOWN(scores, h->s_scores.p, (size_t)total * K * 4);
    if (mfcc) COPY_DOWN(mfcc, h->s_mfcc.p, (size_t)total * R * nc * 2);
    return SR_OK;
}

int sr_live_end(sr_live *l, const uint32_t *channels, uint32_t n_ch, sr_live_seg *segs, uint32_t *n_segs)
{
    if (!l || (n_ch && (!channels || !segs))) return fail(SR_ERR_BAD_ARG, "null argument");
    for (uint32_t i = 0; i < n_ch; i++)
        if (channels[i] >= l->C) return fail(SR_ERR_BAD_ARG, "channel " + std::to_string(channels[i]) + " is past the session's last");
    uint64_t origin = 0;
    if (int rc = live_origin(l, &origin)) return rc;
    if (n_segs) *n_segs = 0;
    if (!n_ch) return SR_OK;
    sr_engine *h = l->h;
    ENTER_DEVICE(h);
    if (l->pending) {
        HIP_TRY(hipEventSynchronize(l->ev_last));
        l->pending = false;
    }
    std::vector<LiveChan> st(l->C);
    COPY_DOWN(st.data(), l->chan.p, (size_t)l->C * sizeof(LiveChan));
    const uint32_t sp = std::max(h->v_durmin, 2u);  // StreamSm: speech = onset states + 1
    std::vector<sr_live_seg> open;
    for (uint32_t i = 0; i < n_ch; i++) {
        const uint32_t c = channels[i];
        if (st[c].state >= sp) open.push_back(sr_live_seg{c, 0u, st[c].open_start, -1});
        st[c] = fresh_chan(l, c, origin);
    }
    COPY_UP(l->chan.p, st.data(), (size_t)l->C * sizeof(LiveChan));
    for (uint32_t i = 0; i < n_ch; i++) fresh_mirror(l, channels[i], origin);
    if (!open.empty()) std::memcpy(segs, open.data(), open.size() * sizeof(sr_live_seg));
    if (n_segs) *n_segs = (uint32_t)open.size();
    return SR_OK;
}
