// Live connected-word decoding (include/sr_engine.h, "live connected-word decoding"): feature frames or samples that arrive
// in pushes; per (channel, level, slot) the decoder's boundary column and per channel the A / E history kept on the device
// between calls (k_chain_live.hip).  OPT-IN EXTENSION, NO REFERENCE COUNTERPART.
//
// The host knows every count: each channel's frames so far, hence which channels a push touches and which compact output row
// each of them gets (the mirror, sr_decode_live_plan.h).  Nothing is read back to size or to label an output.
#include "sr_decode_live_host.h"

using namespace sr;

struct sr_decode_live {
    sr_engine *h = nullptr;
    DecodeLiveMirror m;
    uint32_t max_words = 0, n_words_exact = 0, skip_cost = 0, word_cost = 0;
    std::vector<uint32_t> mid;            // PCM sessions: the channels' mid values
    // layout of the boundary columns: that of the store the session was opened or last reset against
    uint32_t K = 0, tpl_len = 0;
    uint64_t layout_serial = 0;
    DevBuf<ulonglong2> cols;              // [C][max_words][K][tpl_len]
    DevBuf<unsigned long long> A;         // [C][max_words][utt_frames + 1]
    DevBuf<uint32_t> E;                   // [C][max_words + 1][utt_frames + 1]
    DevBuf<SpotLiveChan> d_chan;
    // PCM sessions: kept samples, the rows [kept | chunk], their records and the features of one push
    DevBuf<uint16_t> keep, stage;
    DevBuf<sr_vad_rec> recs;
    DevBuf<int16_t> feat;
    uint32_t keep_stride = 0;
    uint64_t stage_stride = 0;
    hipEvent_t ev_last = nullptr;         // end of the last push (sr_decode_live_end / _close wait for it)
    hipStream_t last_stream = nullptr;    // ... and the stream it ran on: a push on another stream runs behind it
    bool pending = false;
};

namespace {

constexpr uint32_t kDecodeLiveMaxChannels = 65535u;  // a grid dimension
constexpr uint32_t kDecodeLiveMaxFrames = 16383u;    // the u32 cost bound and the 14-bit start of a key

// the boundary columns laid out for the engine's current store (nothing of value is in them: see sr_decode_live_end)
int relayout(sr_decode_live *l)
{
    const sr_engine *h = l->h;
    const uint32_t tpl_len = h->tpl_rows - 1;
    if (int rc = l->cols.reserve((size_t)l->m.C * l->max_words * h->K * tpl_len)) return rc;
    l->K = h->K;
    l->tpl_len = tpl_len;
    l->layout_serial = h->store_serial;
    return SR_OK;
}

int plan_push(const sr_decode_live *l, const uint32_t *n, uint32_t n_all, DecodeLivePlan *pl)
{
    std::string why;
    if (!decode_live_plan(l->m, l->h->store_serial, n, n_all, pl, &why)) return fail(SR_ERR_BAD_ARG, why);
    return SR_OK;
}

ChainLiveArgs live_args(const sr_decode_live *l, const int16_t *d_mfcc, uint64_t row_stride, sr_chain_rec *d_rec, sr_chain_word *d_words,
                        uint32_t *d_level_cost)
{
    const sr_engine *h = l->h;
    const uint32_t *t = h->wg_tab.p;  // order[K] | group_start[n_words + 1] | word_id[n_words] | group_of_slot[K]
    return ChainLiveArgs{d_mfcc, row_stride, l->d_chan.p, l->m.C, h->tpl.p, h->tpl_frames.p, h->tpl_valid.p, l->K, h->tpl_stride, l->tpl_len,
                         l->m.utt_frames + 1u, l->max_words, l->n_words_exact, l->skip_cost, l->word_cost, l->cols.p, l->A.p, l->E.p,
                         t + h->K + 2 * (size_t)h->wg_words + 1, t + h->K + h->wg_words + 1, d_rec, d_words, d_level_cost};
}

// the levels over the new frames of every channel and the trace of every emitting one, enqueued on s
int launch_push(sr_decode_live *l, const DecodeLivePlan &pl, const int16_t *d_mfcc, uint64_t row_stride, sr_chain_rec *d_rec,
                sr_chain_word *d_words, uint32_t *d_level_cost, hipStream_t s)
{
    if (!pl.rows) return SR_OK;
    const ChainLiveArgs a = live_args(l, d_mfcc, row_stride, d_rec, d_words, d_level_cost);
    if (pl.max_frames) launch_chain_live(a, s);
    else launch_chain_live_trace(a, s);  // (PCM) samples, but no new frame: the parse so far again
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

}  // namespace

extern "C" {

int sr_decode_live_geometry(uint32_t tpl_rows, uint32_t K, uint32_t max_words, uint32_t utt_frames, uint32_t chunk_max, uint32_t out[3])
{
    if (!out || !tpl_rows || tpl_rows > 16383 || !K || K > kChainMaxSlots || max_words < 1 || max_words > kChainMaxWords || !utt_frames ||
        utt_frames > kDecodeLiveMaxFrames || !chunk_max || chunk_max > utt_frames)
        return fail(SR_ERR_BAD_ARG, "null / zero argument, or one outside its range");
    const LdsBudget mi355x;  // no device: MI355X's figures
    out[0] = decode_live_state_bytes(tpl_rows, K, max_words, utt_frames);
    out[1] = spot_max_tpl(mi355x);
    out[2] = 2 * max_words + 2;
    return SR_OK;
}

int sr_decode_live_open(sr_engine *h, uint32_t n_channels, uint32_t chunk_max, uint32_t utt_frames, uint32_t max_words, uint32_t n_words_exact,
                        uint32_t skip_cost, uint32_t word_cost, const uint32_t *mid, sr_decode_live **out)
{
    if (!h || !out) return fail(SR_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (int rc = check_chain(h, max_words, n_words_exact, skip_cost, word_cost)) return rc;
    if (!n_channels || n_channels > kDecodeLiveMaxChannels || !utt_frames || utt_frames > kDecodeLiveMaxFrames)
        return fail(SR_ERR_BAD_ARG, "n_channels not in 1..65535 / utt_frames not in 1..16383");
    if (!chunk_max) return fail(SR_ERR_BAD_ARG, "chunk_max 0");
    if (mid) {
        if (((uint64_t)chunk_max + h->hop - 1) / h->hop > std::min(h->cfg.max_frames, utt_frames))
            return fail(SR_ERR_BAD_ARG, "a push of chunk_max samples could complete more than min(max_frames, utt_frames) frames");
        for (uint32_t c = 0; c < n_channels; c++)
            if (mid[c] > 0xFFFFu) return fail(SR_ERR_BAD_ARG, "mid exceeds the u16 sample range");
        if (int rc = check_batch(h, n_channels)) return rc;
    } else if (chunk_max > utt_frames) {
        return fail(SR_ERR_BAD_ARG, "chunk_max not in 1..utt_frames");
    }
    ENTER_DEVICE(h);
    sr_decode_live *l = new sr_decode_live();
    l->h = h;
    l->m.open(n_channels, h->store_serial);
    l->m.chunk_max = chunk_max;
    l->m.utt_frames = utt_frames;
    l->m.pcm = mid != nullptr;
    l->m.frame_len = h->frame_len;
    l->m.hop = h->hop;
    l->max_words = max_words;
    l->n_words_exact = n_words_exact;
    l->skip_cost = skip_cost;
    l->word_cost = word_cost;
    const size_t P = (size_t)utt_frames + 1;
    int rc = relayout(l);
    if (!rc) rc = l->A.reserve((size_t)n_channels * max_words * P);
    if (!rc) rc = l->E.reserve((size_t)n_channels * (max_words + 1u) * P);
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
        sr_decode_live_close(l);
        return rc;
    }
    *out = l;
    return SR_OK;
}

void sr_decode_live_close(sr_decode_live *l)
{
    if (!l) return;
    DeviceGuard guard;
    (void)guard.enter(l->h->device);
    if (l->pending) (void)hipEventSynchronize(l->ev_last);
    l->cols.release();
    l->A.release();
    l->E.release();
    l->d_chan.release();
    l->keep.release();
    l->stage.release();
    l->recs.release();
    l->feat.release();
    if (l->ev_last) (void)hipEventDestroy(l->ev_last);
    delete l;
}

int sr_decode_live_push_dev(sr_decode_live *l, const int16_t *d_mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                            sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_level_cost, sr_chain_live_row *rows, uint32_t *n_rows,
                            void *stream)
{
    if (!l) return fail(SR_ERR_BAD_ARG, "null session");
    DecodeLivePlan pl;
    int rc = plan_push(l, n, n_all, &pl);
    if (!rc) rc = check_frames_in(l, pl, d_mfcc, row_stride, true);
    if (!rc) rc = check_outputs(l, pl.rows, max_rows, d_rec, d_words, d_level_cost, rows);
    if (rc) return rc;
    ENTER_DEVICE(l->h);
    const hipStream_t s = (hipStream_t)stream;
    if (pl.rows) {
        if ((rc = order_after_last_push(l, s))) return rc;
        if ((rc = upload_chan(l, pl.chan, s))) return rc;
        if ((rc = launch_push(l, pl, d_mfcc, row_stride, d_rec, d_words, d_level_cost, s))) return rc;
    }
    decode_live_advance(l->m, pl, rows, n_rows);
    return pl.rows ? mark_push(l, s) : SR_OK;
}

int sr_decode_live_push(sr_decode_live *l, const int16_t *mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                        sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost, sr_chain_live_row *rows, uint32_t *n_rows)
{
    if (!l) return fail(SR_ERR_BAD_ARG, "null session");
    DecodeLivePlan pl;
    int rc = plan_push(l, n, n_all, &pl);
    if (!rc) rc = check_frames_in(l, pl, mfcc, row_stride, false);
    if (!rc) rc = check_outputs(l, pl.rows, max_rows, rec, words, level_cost, rows);
    if (rc) return rc;
    sr_engine *h = l->h;
    ENTER_HOST_CALL(h);
    HostOutputs o;
    if (pl.rows) {
        const size_t ds = (size_t)pl.max_frames * kCoef;  // device rows hold the largest count
        if ((rc = h->s_mfcc.reserve((size_t)l->m.C * ds))) return rc;
        if ((rc = o.reserve(pl.rows, l->max_words, level_cost != nullptr))) return rc;
        for (uint32_t c = 0; c < l->m.C; c++)  // count by count: nothing past n[c] of a caller's row is read
            if (pl.chan[c].n) COPY_UP(h->s_mfcc.p + c * ds, mfcc + (size_t)c * row_stride, (size_t)pl.chan[c].n * kCoef * 2);
        if ((rc = order_after_last_push(l, nullptr))) return rc;
        if ((rc = upload_chan(l, pl.chan, nullptr))) return rc;
        if ((rc = launch_push(l, pl, h->s_mfcc.p, ds, o.rec.p, o.words.p, level_cost ? o.lc.p : nullptr, nullptr))) return rc;
    }
    decode_live_advance(l->m, pl, rows, n_rows);
    if (pl.rows && (rc = mark_push(l, nullptr))) return rc;
    return pl.rows ? o.down(pl.rows, l->max_words, rec, words, level_cost) : SR_OK;
}

int sr_decode_live_push_pcm_dev(sr_decode_live *l, const uint16_t *d_pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                                uint32_t max_rows, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_level_cost,
                                sr_chain_live_row *rows, uint32_t *n_rows, void *stream)
{
    if (!l) return fail(SR_ERR_BAD_ARG, "null session");
    DecodeLivePlan pl;
    int rc = plan_push(l, n, n_all, &pl);
    if (!rc) rc = check_pcm_in(l, pl, d_pcm, pcm_stride, true);
    if (!rc) rc = check_outputs(l, pl.rows, max_rows, d_rec, d_words, d_level_cost, rows);
    if (rc) return rc;
    sr_engine *h = l->h;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    if (pl.rows) {
        if ((rc = order_after_last_push(l, s))) return rc;
        if ((rc = upload_chan(l, pl.chan, s))) return rc;
        if ((rc = launch_front_end(l, pl, d_pcm, pcm_stride, s))) return rc;
        if ((rc = launch_push(l, pl, l->feat.p, (uint64_t)h->cfg.max_frames * kCoef, d_rec, d_words, d_level_cost, s))) return rc;
    }
    decode_live_advance(l->m, pl, rows, n_rows);
    return pl.rows ? mark_push(l, s) : SR_OK;
}

int sr_decode_live_push_pcm(sr_decode_live *l, const uint16_t *pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                            sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost, sr_chain_live_row *rows, uint32_t *n_rows)
{
    if (!l) return fail(SR_ERR_BAD_ARG, "null session");
    DecodeLivePlan pl;
    int rc = plan_push(l, n, n_all, &pl);
    if (!rc) rc = check_pcm_in(l, pl, pcm, pcm_stride, false);
    if (!rc) rc = check_outputs(l, pl.rows, max_rows, rec, words, level_cost, rows);
    if (rc) return rc;
    sr_engine *h = l->h;
    ENTER_HOST_CALL(h);
    HostOutputs o;
    if (pl.rows) {
        const uint64_t ds = dev_pitch(pl.max_n);
        if ((rc = h->s_pcm.reserve((size_t)l->m.C * ds))) return rc;
        if ((rc = o.reserve(pl.rows, l->max_words, level_cost != nullptr))) return rc;
        for (uint32_t c = 0; c < l->m.C; c++)  // count by count: nothing past n[c] of a caller's row is read
            if (pl.chan[c].n_samp) COPY_UP(h->s_pcm.p + c * ds, pcm + (size_t)c * pcm_stride, (size_t)pl.chan[c].n_samp * 2);
        if ((rc = order_after_last_push(l, nullptr))) return rc;
        if ((rc = upload_chan(l, pl.chan, nullptr))) return rc;
        if ((rc = launch_front_end(l, pl, h->s_pcm.p, ds, nullptr))) return rc;
        if ((rc = launch_push(l, pl, l->feat.p, (uint64_t)h->cfg.max_frames * kCoef, o.rec.p, o.words.p, level_cost ? o.lc.p : nullptr, nullptr)))
            return rc;
    }
    decode_live_advance(l->m, pl, rows, n_rows);
    if (pl.rows && (rc = mark_push(l, nullptr))) return rc;
    return pl.rows ? o.down(pl.rows, l->max_words, rec, words, level_cost) : SR_OK;
}

int sr_decode_live_end(sr_decode_live *l, const uint32_t *channels, uint32_t n_ch, sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost,
                       sr_chain_live_row *rows, uint32_t *n_rows)
{
    if (!l || (n_ch && !channels)) return fail(SR_ERR_BAD_ARG, "null argument");
    sr_engine *h = l->h;
    std::vector<SpotLiveChan> chan;
    std::vector<sr_chain_live_row> order;
    std::string why;
    if (!decode_live_end_list(l->m, h->store_serial, channels, n_ch, &chan, &order, &why)) return fail(SR_ERR_BAD_ARG, why);
    const uint32_t n_out = (uint32_t)order.size();
    if (int rc = check_outputs(l, n_out, n_out, rec, words, level_cost, rows)) return rc;
    if (int rc = check_end_rows(l, n_out, rec, words, level_cost, rows)) return rc;
    if (!n_out) {
        if (n_rows) *n_rows = 0;
        return SR_OK;
    }
    ENTER_HOST_CALL(h);
    if (l->pending) {
        HIP_TRY(hipEventSynchronize(l->ev_last));
        l->pending = false;
    }
    HostOutputs o;
    if (int rc = o.reserve(n_out, l->max_words, level_cost != nullptr)) return rc;
    // Every channel that still holds state is bound to a store that is gone, and the trace reads no column: the columns are
    // laid out again BEFORE anything is written, so that a failed allocation leaves outputs, mirror and layout as they were.
    if (l->layout_serial != h->store_serial)
        if (int rc = relayout(l)) return rc;
    if (int rc = upload_chan(l, chan, nullptr)) return rc;
    launch_chain_live_trace(live_args(l, nullptr, 0, o.rec.p, o.words.p, level_cost ? o.lc.p : nullptr), nullptr);
    HIP_TRY(hipGetLastError());
    if (int rc = o.down(n_out, l->max_words, rec, words, level_cost)) return rc;
    decode_live_reset(l->m, h->store_serial, order);
    for (uint32_t r = 0; r < n_out; r++) rows[r] = order[r];
    if (n_rows) *n_rows = n_out;
    return SR_OK;
}

}  // extern "C"
