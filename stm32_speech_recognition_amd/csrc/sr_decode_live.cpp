// Live connected-word decoding (include/sr_engine.h, "live connected-word decoding"): feature frames or samples that arrive
// in pushes; per (channel, level, slot) the decoder's boundary column and per channel the A / E history kept on the device
// between calls (k_chain_live.hip).  OPT-IN EXTENSION, NO REFERENCE COUNTERPART.
//
// The host knows every count: each channel's frames so far, hence which channels a push touches and which compact output row
// each of them gets (the mirror, sr_decode_live_plan.h).  Nothing is read back to size or to label an output.  The session
// core, the checks, the push sequence and the sequence of an end call are every live session's (sr_live_host.h).
#include "sr_live_host.h"

using namespace sr;

struct sr_decode_live : LiveCore {
    DecodeLiveMirror m;
    uint32_t max_words = 0, n_words_exact = 0, skip_cost = 0, word_cost = 0;
    // layout of the boundary columns: that of the store the session was opened or last reset against
    uint32_t K = 0, tpl_len = 0;
    uint64_t layout_serial = 0;
    DevBuf<ulonglong2> cols;              // [C][max_words][K][tpl_len]
    DevBuf<unsigned long long> A;         // [C][max_words][utt_frames + 1]
    DevBuf<uint32_t> E;                   // [C][max_words + 1][utt_frames + 1]
};

namespace {

// the boundary columns laid out for the engine's current store (nothing of value is in them: see sr_decode_live_end)
int relayout(sr_decode_live *l)
{
    const sr_engine *h = l->h;
    const uint32_t tpl_len = store_tpl_len(h);
    if (int rc = l->cols.reserve((size_t)l->C * l->max_words * h->K * tpl_len)) return rc;
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

// the trace will read the store's frame counts and the word map: the conditions of sr_decode_words_dp_dev on the engine, its
// current store and word map
int check_out(const sr_decode_live *l, uint32_t n_out, uint32_t max_rows, const sr_chain_rec *rec, const sr_chain_word *words,
              const uint32_t *level_cost, const sr_chain_live_row *rows)
{
    return check_outputs(l->max_words, n_out, max_rows, rec, words, level_cost, rows,
                         [&] { return check_chain(l->h, l->max_words, l->n_words_exact, l->skip_cost, l->word_cost); });
}

ChainLiveArgs live_args(const sr_decode_live *l, const int16_t *d_mfcc, uint64_t row_stride, sr_chain_rec *d_rec, sr_chain_word *d_words,
                        uint32_t *d_level_cost)
{
    const sr_engine *h = l->h;
    const WordTab wt = word_tab(h);
    return ChainLiveArgs{d_mfcc, row_stride, l->d_chan.p, l->C, h->tpl.p, h->tpl_frames.p, h->tpl_valid.p, l->K, h->tpl_stride, l->tpl_len,
                         l->m.utt_frames + 1u, l->max_words, l->n_words_exact, l->skip_cost, l->word_cost, l->cols.p, l->A.p, l->E.p,
                         wt.group_of_slot, wt.word_id, d_rec, d_words, d_level_cost};
}

// the levels over the new frames of every channel and the trace of every emitting one, enqueued on s
int launch_push(sr_decode_live *l, const DecodeLivePlan &pl, const int16_t *d_mfcc, uint64_t row_stride, sr_chain_rec *d_rec,
                sr_chain_word *d_words, uint32_t *d_level_cost, hipStream_t s)
{
    const ChainLiveArgs a = live_args(l, d_mfcc, row_stride, d_rec, d_words, d_level_cost);
    if (pl.max_frames) launch_chain_live(a, s);
    else launch_chain_live_trace(a, s);  // (PCM) samples, but no new frame: the parse so far again
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

// the four push forms: a push enqueues work when a channel emits a row
int push(sr_decode_live *l, const LiveIn &in, bool device, void *stream, const uint32_t *n, uint32_t n_all, uint32_t max_rows, sr_chain_rec *rec,
         sr_chain_word *words, uint32_t *level_cost, sr_chain_live_row *rows, uint32_t *n_rows)
{
    if (!l) return fail(SR_ERR_BAD_ARG, "null session");
    DecodeLivePlan pl;
    int rc = plan_push(l, n, n_all, &pl);
    if (!rc) rc = check_live_in(l->m.pcm, in, pl.max_n, device);
    if (!rc) rc = check_out(l, pl.rows, max_rows, rec, words, level_cost, rows);
    if (rc) return rc;
    return live_push_chain(
        *l, pl, in, device, stream, l->max_words, rec, words, level_cost,
        [&](const int16_t *f, uint64_t rs, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_lc, hipStream_t s) {
            return launch_push(l, pl, f, rs, d_rec, d_words, d_lc, s);
        },
        [&] { decode_live_advance(l->m, pl, rows, n_rows); });
}

}  // namespace

extern "C" {

int sr_decode_live_geometry(uint32_t tpl_rows, uint32_t K, uint32_t max_words, uint32_t utt_frames, uint32_t chunk_max, uint32_t out[3])
{
    if (!out || !tpl_rows || tpl_rows > 16383 || !K || K > kChainMaxSlots || max_words < 1 || max_words > kChainMaxWords || !utt_frames ||
        utt_frames > kLiveMaxFrames || !chunk_max || chunk_max > utt_frames)
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
    if (!n_channels || n_channels > kLiveMaxChannels || !utt_frames || utt_frames > kLiveMaxFrames)
        return fail(SR_ERR_BAD_ARG, "n_channels not in 1..65535 / utt_frames not in 1..16383");
    if (int rc = LiveCore::check_open(h, n_channels, chunk_max, mid ? std::min(h->cfg.max_frames, utt_frames) : utt_frames, mid)) return rc;
    ENTER_DEVICE(h);
    sr_decode_live *l = new sr_decode_live();
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
    int rc = l->open_common(h, n_channels, chunk_max, mid);
    if (!rc) rc = relayout(l);
    if (!rc) rc = l->A.reserve((size_t)n_channels * max_words * P);
    if (!rc) rc = l->E.reserve((size_t)n_channels * (max_words + 1u) * P);
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
    l->release();
    l->cols.release();
    l->A.release();
    l->E.release();
    delete l;
}

int sr_decode_live_push_dev(sr_decode_live *l, const int16_t *d_mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                            sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_level_cost, sr_chain_live_row *rows, uint32_t *n_rows,
                            void *stream)
{
    return push(l, LiveIn{d_mfcc, row_stride, false}, true, stream, n, n_all, max_rows, d_rec, d_words, d_level_cost, rows, n_rows);
}

int sr_decode_live_push(sr_decode_live *l, const int16_t *mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                        sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost, sr_chain_live_row *rows, uint32_t *n_rows)
{
    return push(l, LiveIn{mfcc, row_stride, false}, false, nullptr, n, n_all, max_rows, rec, words, level_cost, rows, n_rows);
}

int sr_decode_live_push_pcm_dev(sr_decode_live *l, const uint16_t *d_pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                                uint32_t max_rows, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_level_cost,
                                sr_chain_live_row *rows, uint32_t *n_rows, void *stream)
{
    return push(l, LiveIn{d_pcm, pcm_stride, true}, true, stream, n, n_all, max_rows, d_rec, d_words, d_level_cost, rows, n_rows);
}

int sr_decode_live_push_pcm(sr_decode_live *l, const uint16_t *pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                            sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost, sr_chain_live_row *rows, uint32_t *n_rows)
{
    return push(l, LiveIn{pcm, pcm_stride, true}, false, nullptr, n, n_all, max_rows, rec, words, level_cost, rows, n_rows);
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
    if (int rc = check_out(l, n_out, n_out, rec, words, level_cost, rows)) return rc;
    if (int rc = check_end_rows(l->max_words, n_out, rec, words, level_cost, rows)) return rc;
    // Every channel that still holds state is bound to a store that is gone, and the trace reads no column: the columns are
    // laid out again BEFORE anything is written, so that a failed allocation leaves outputs, mirror and layout as they were.
    return live_end(
        *l, chan, order, l->max_words, rec, words, level_cost, rows, n_rows,
        [&] { return l->layout_serial != h->store_serial ? relayout(l) : SR_OK; },
        [&](sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_lc) {
            launch_chain_live_trace(live_args(l, nullptr, 0, d_rec, d_words, d_lc), nullptr);
        },
        [&] { decode_live_reset(l->m, h->store_serial, order); });
}

}  // extern "C"
