// Live one-pass connected-word decoding (include/sr_engine.h, "live one-pass connected-word decoding"): feature frames or
// samples that arrive in pushes; per channel the one-pass decoder's A / E history, one saved column per slot and the feature
// row kept on the device between calls (k_onepass_live.hip).  OPT-IN EXTENSION, NO REFERENCE COUNTERPART.
//
// The host knows every count: each channel's frames so far and the first frame of its last block, hence which channels a push
// touches, how their new frames are cut into blocks and which compact output row each of them gets (the mirror,
// sr_onepass_live_plan.h).  Nothing is read back to size or to label an output.  The session core, the checks, the push
// sequence and the sequence of an end call are every live session's (sr_live_host.h).
#include "sr_onepass_live_plan.h"
#include "sr_live_host.h"

using namespace sr;

struct sr_onepass_live : LiveCore {
    OnePassLiveMirror om;
    uint32_t words_cap = 0;               // the word rows of an output row; no count is given
    uint32_t tail = 0, skip_cost = 0, word_cost = 0;
    // layout of the saved columns: that of the store the session was opened or last reset against
    uint32_t K = 0, tpl_len = 0;
    uint64_t layout_serial = 0;
    DevBuf<ulonglong2> cols;              // [C][K][tpl_len]
    DevBuf<unsigned long long> A;         // [C][utt_frames + 1]
    DevBuf<uint32_t> E;                   // [C][utt_frames + 1]
    DevBuf<int16_t> hist;                 // [C][utt_frames][12]: the channels' feature rows
    // sr_onepass_live_commit: per channel {words delivered, the last delivered word's node}, and the rows of the call in flight
    DevBuf<uint2> cursor;                 // [C]
    DevBuf<sr_chain_live_row> commit_rows;  // [C]
};

namespace {

uint32_t block_hook()
{
    const int64_t v = dev_hook(kHookOnePassBlock);  // testing build: short blocks put seams into small test shapes
    return v > 0 ? (uint32_t)std::min<int64_t>(v, 16383) : 0u;
}

// the decoder's conditions on the engine, the store, the word map and the costs (the word-cost bound is the plan's)
int check_store(const sr_onepass_live *l) { return check_chain(l->h, 1, 0, l->skip_cost, l->word_cost); }

// the saved columns laid out for the engine's current store (nothing of value is in them: see sr_onepass_live_end)
int relayout(sr_onepass_live *l)
{
    const sr_engine *h = l->h;
    const uint32_t tpl_len = store_tpl_len(h);
    if (int rc = l->cols.reserve((size_t)l->C * h->K * tpl_len)) return rc;
    l->K = h->K;
    l->tpl_len = tpl_len;
    l->layout_serial = h->store_serial;
    return SR_OK;
}

int plan_push(const sr_onepass_live *l, const uint32_t *n, uint32_t n_all, OnePassLivePlan *pl)
{
    const sr_engine *h = l->h;
    std::string why;
    if (!onepass_live_plan(l->om, h->store_serial, onepass_reach(h->tpl_len_host.data(), h->K), block_hook(), l->word_cost, n, n_all, pl, &why))
        return fail(SR_ERR_BAD_ARG, why);
    return SR_OK;
}

// (the store is checked behind the buffers here)
int check_out(const sr_onepass_live *l, uint32_t n_out, uint32_t max_rows, const sr_chain_rec *rec, const sr_chain_word *words,
              const sr_chain_live_row *rows)
{
    if (int rc = check_outputs(l->words_cap, n_out, max_rows, rec, words, nullptr, rows, [] { return SR_OK; })) return rc;
    return n_out ? check_store(l) : SR_OK;
}

OnePassLiveArgs live_args(const sr_onepass_live *l, const int16_t *d_mfcc, uint64_t row_stride, uint32_t block, sr_chain_rec *d_rec,
                          sr_chain_word *d_words)
{
    const sr_engine *h = l->h;
    const WordTab wt = word_tab(h);
    return OnePassLiveArgs{d_mfcc, row_stride, l->d_chan.p, l->C, h->tpl.p, h->tpl_frames.p, h->tpl_valid.p, l->K, h->tpl_stride, l->tpl_len,
                           l->om.d.utt_frames + 1u, block, l->words_cap, l->tail, l->skip_cost, l->word_cost, l->cols.p, l->A.p, l->E.p, l->hist.p,
                           wt.group_of_slot, wt.word_id, d_rec, d_words};
}

// the blocks over the new frames of every channel and the trace of every emitting one, enqueued on s (PCM: samples, but no
// new frame, is no block: the parse so far again)
int launch_push(sr_onepass_live *l, const OnePassLivePlan &pl, const int16_t *d_mfcc, uint64_t row_stride, sr_chain_rec *d_rec,
                sr_chain_word *d_words, hipStream_t s)
{
    launch_onepass_live(live_args(l, d_mfcc, row_stride, pl.block, d_rec, d_words), pl.n_blocks, s);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

// the four push forms: a push enqueues work when a channel emits a row
int push(sr_onepass_live *l, const LiveIn &in, bool device, void *stream, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
         sr_chain_rec *rec, sr_chain_word *words, sr_chain_live_row *rows, uint32_t *n_rows)
{
    if (!l) return fail(SR_ERR_BAD_ARG, "null session");
    OnePassLivePlan pl;
    int rc = plan_push(l, n, n_all, &pl);
    if (!rc) rc = check_live_in(l->om.d.pcm, in, pl.d.max_n, device);
    if (!rc) rc = check_out(l, pl.d.rows, max_rows, rec, words, rows);
    if (rc) return rc;
    return live_push_chain(
        *l, pl.d, in, device, stream, l->words_cap, rec, words, nullptr,
        [&](const int16_t *f, uint64_t rs, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *, hipStream_t s) {
            return launch_push(l, pl, f, rs, d_rec, d_words, s);
        },
        [&] { onepass_live_advance(l->om, pl, rows, n_rows); });
}

// a commit call up to its launch: the rows of the distinct listed channels from the mirror, then the checks -- nothing is
// enqueued, written or changed before all of them pass.  host: rows is a host buffer like crec and cwords (the host form)
int plan_commit(const sr_onepass_live *l, const uint32_t *channels, uint32_t n_ch, const sr_commit_rec *crec, const sr_chain_word *cwords,
                const sr_chain_live_row *rows, bool host, std::vector<sr_chain_live_row> *order)
{
    if (!l || (n_ch && !channels)) return fail(SR_ERR_BAD_ARG, "null argument");
    std::string why;
    if (!onepass_live_commit_list(l->om, l->h->store_serial, channels, n_ch, order, &why)) return fail(SR_ERR_BAD_ARG, why);
    const size_t n_out = order->size();
    if (!n_out) return SR_OK;
    if (!crec || !cwords || !rows) return fail(SR_ERR_BAD_ARG, "null argument");
    if (int rc = check_store(l)) return rc;
    const size_t n_c = n_out * sizeof *crec, n_w = n_out * l->words_cap * sizeof *cwords, n_r = n_out * sizeof *rows;
    if (overlap(crec, n_c, cwords, n_w)) return fail(SR_ERR_BAD_ARG, "crec and cwords overlap");
    if (host && (overlap(rows, n_r, crec, n_c) || overlap(rows, n_r, cwords, n_w)))
        return fail(SR_ERR_BAD_ARG, "rows overlaps crec or cwords");
    return SR_OK;
}

// ... and the launch on s: behind the session's last push or commit, and the next one runs behind it
int enqueue_commit(sr_onepass_live *l, const std::vector<sr_chain_live_row> &order, sr_commit_rec *d_crec, sr_chain_word *d_cwords, hipStream_t s)
{
    const sr_engine *h = l->h;
    if (int rc = l->order_after_last_push(s)) return rc;
    // (a pageable source is staged before the call returns: the list may go out of scope)
    HIP_TRY(hipMemcpyAsync(l->commit_rows.p, order.data(), order.size() * sizeof(sr_chain_live_row), hipMemcpyHostToDevice, s));
    const WordTab wt = word_tab(h);
    launch_onepass_live_commit(
        OnePassCommitArgs{l->commit_rows.p, (uint32_t)order.size(), l->om.d.utt_frames + 1u, onepass_commit_window(h->tpl_len_host.data(), h->K),
                          l->words_cap, l->word_cost, l->A.p, l->E.p, l->cursor.p, h->tpl_frames.p, wt.group_of_slot,
                          wt.word_id, d_crec, d_cwords},
        s);
    HIP_TRY(hipGetLastError());
    return l->mark_push(s);
}

void label_commit(const std::vector<sr_chain_live_row> &order, sr_chain_live_row *rows, uint32_t *n_rows)
{
    for (size_t r = 0; r < order.size(); r++) rows[r] = order[r];
    if (n_rows) *n_rows = (uint32_t)order.size();
}

}  // namespace

extern "C" {

int sr_onepass_live_geometry(uint32_t tpl_rows, uint32_t K, uint32_t min_tpl_frames, uint32_t utt_frames, uint32_t chunk_max, uint32_t out[4])
{
    if (!out || !tpl_rows || tpl_rows > 16383 || !K || K > kChainMaxSlots || !min_tpl_frames || min_tpl_frames > tpl_rows || !utt_frames ||
        utt_frames > kLiveMaxFrames || !chunk_max || chunk_max > utt_frames)
        return fail(SR_ERR_BAD_ARG, "null / zero argument, or one outside its range");
    const LdsBudget mi355x;  // no device: MI355X's figures
    const uint32_t L = min_tpl_frames / 2u + 1u;
    out[0] = onepass_live_state_bytes(tpl_rows, K, utt_frames);
    out[1] = spot_max_tpl(mi355x);
    out[2] = L;
    out[3] = onepass_live_launches(chunk_max, onepass_live_block(L, block_hook(), chunk_max));
    return SR_OK;
}

int sr_onepass_live_open(sr_engine *h, uint32_t n_channels, uint32_t chunk_max, uint32_t utt_frames, uint32_t words_cap, uint32_t flags,
                         uint32_t skip_cost, uint32_t word_cost, const uint32_t *mid, sr_onepass_live **out)
{
    if (!h || !out) return fail(SR_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (int rc = check_chain(h, 1, 0, skip_cost, word_cost)) return rc;
    if (!words_cap) return fail(SR_ERR_BAD_ARG, "words_cap must be at least 1");
    if (flags & ~SR_OP_LIVE_TAIL) return fail(SR_ERR_BAD_ARG, "unknown flag");
    if (!n_channels || n_channels > kLiveMaxChannels || !utt_frames || utt_frames > kLiveMaxFrames)
        return fail(SR_ERR_BAD_ARG, "n_channels not in 1..65535 / utt_frames not in 1..16383");
    if (!onepass_cost_ok(utt_frames, onepass_reach(h->tpl_len_host.data(), h->K), word_cost))
        return fail(SR_ERR_BAD_ARG, "(utt_frames / L) * word_cost must be at most 2^30, L = the shortest valid template's frames / 2 + 1");
    if (int rc = LiveCore::check_open(h, n_channels, chunk_max, mid ? std::min(h->cfg.max_frames, utt_frames) : utt_frames, mid)) return rc;
    ENTER_DEVICE(h);
    sr_onepass_live *l = new sr_onepass_live();
    l->om.open(n_channels, h->store_serial);
    l->om.d.chunk_max = chunk_max;
    l->om.d.utt_frames = utt_frames;
    l->om.d.pcm = mid != nullptr;
    l->om.d.frame_len = h->frame_len;
    l->om.d.hop = h->hop;
    l->words_cap = words_cap;
    l->tail = flags & SR_OP_LIVE_TAIL;
    l->skip_cost = skip_cost;
    l->word_cost = word_cost;
    const size_t P = (size_t)utt_frames + 1;
    int rc = l->open_common(h, n_channels, chunk_max, mid);
    if (!rc) rc = relayout(l);
    if (!rc) rc = l->A.reserve((size_t)n_channels * P);
    if (!rc) rc = l->E.reserve((size_t)n_channels * P);
    if (!rc) rc = l->hist.reserve((size_t)n_channels * utt_frames * kCoef);
    if (!rc) rc = l->cursor.reserve(n_channels);
    if (!rc) rc = l->commit_rows.reserve(n_channels);
    // no word yet anywhere, E(0) = 0: the state of an empty channel, which a push finds without a launch of its own (every other
    // position of E is written before it is read)
    if (!rc && (hipMemsetAsync(l->A.p, 0xFF, (size_t)n_channels * P * 8, nullptr) != hipSuccess ||
                hipMemsetAsync(l->E.p, 0, (size_t)n_channels * P * 4, nullptr) != hipSuccess ||
                hipMemsetAsync(l->cursor.p, 0, (size_t)n_channels * sizeof(uint2), nullptr) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess))
        rc = fail(SR_ERR_HIP, "clearing the session's history failed");
    if (rc) {
        (void)hipGetLastError();
        sr_onepass_live_close(l);
        return rc;
    }
    *out = l;
    return SR_OK;
}

void sr_onepass_live_close(sr_onepass_live *l)
{
    if (!l) return;
    DeviceGuard guard;
    (void)guard.enter(l->h->device);
    l->release();
    l->cols.release();
    l->A.release();
    l->E.release();
    l->hist.release();
    l->cursor.release();
    l->commit_rows.release();
    delete l;
}

int sr_onepass_live_push_dev(sr_onepass_live *l, const int16_t *d_mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                             sr_chain_rec *d_rec, sr_chain_word *d_words, sr_chain_live_row *rows, uint32_t *n_rows, void *stream)
{
    return push(l, LiveIn{d_mfcc, row_stride, false}, true, stream, n, n_all, max_rows, d_rec, d_words, rows, n_rows);
}

int sr_onepass_live_push(sr_onepass_live *l, const int16_t *mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                         sr_chain_rec *rec, sr_chain_word *words, sr_chain_live_row *rows, uint32_t *n_rows)
{
    return push(l, LiveIn{mfcc, row_stride, false}, false, nullptr, n, n_all, max_rows, rec, words, rows, n_rows);
}

int sr_onepass_live_push_pcm_dev(sr_onepass_live *l, const uint16_t *d_pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                                 uint32_t max_rows, sr_chain_rec *d_rec, sr_chain_word *d_words, sr_chain_live_row *rows, uint32_t *n_rows,
                                 void *stream)
{
    return push(l, LiveIn{d_pcm, pcm_stride, true}, true, stream, n, n_all, max_rows, d_rec, d_words, rows, n_rows);
}

int sr_onepass_live_push_pcm(sr_onepass_live *l, const uint16_t *pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                             sr_chain_rec *rec, sr_chain_word *words, sr_chain_live_row *rows, uint32_t *n_rows)
{
    return push(l, LiveIn{pcm, pcm_stride, true}, false, nullptr, n, n_all, max_rows, rec, words, rows, n_rows);
}

int sr_onepass_live_end(sr_onepass_live *l, const uint32_t *channels, uint32_t n_ch, sr_chain_rec *rec, sr_chain_word *words,
                        sr_chain_live_row *rows, uint32_t *n_rows)
{
    if (!l || (n_ch && !channels)) return fail(SR_ERR_BAD_ARG, "null argument");
    sr_engine *h = l->h;
    std::vector<SpotLiveChan> chan;
    std::vector<sr_chain_live_row> order;
    std::string why;
    if (!onepass_live_end_list(l->om, h->store_serial, channels, n_ch, &chan, &order, &why)) return fail(SR_ERR_BAD_ARG, why);
    const uint32_t n_out = (uint32_t)order.size();
    if (int rc = check_out(l, n_out, n_out, rec, words, rows)) return rc;
    if (int rc = check_end_rows(l->words_cap, n_out, rec, words, nullptr, rows)) return rc;
    // Every channel that still holds state is bound to a store that is gone, and the trace reads no column: the columns are
    // laid out again BEFORE anything is written, so that a failed allocation leaves outputs, mirror and layout as they were.
    return live_end(
        *l, chan, order, l->words_cap, rec, words, nullptr, rows, n_rows,
        [&] { return l->layout_serial != h->store_serial ? relayout(l) : SR_OK; },
        [&](sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *) {
            launch_onepass_live_end(live_args(l, nullptr, 0, 1u, d_rec, d_words), l->cursor.p, nullptr);
        },
        [&] { onepass_live_reset(l->om, h->store_serial, order); });
}

int sr_onepass_live_commit_dev(sr_onepass_live *l, const uint32_t *channels, uint32_t n_ch, sr_commit_rec *d_crec, sr_chain_word *d_cwords,
                               sr_chain_live_row *rows, uint32_t *n_rows, void *stream)
{
    std::vector<sr_chain_live_row> order;
    if (int rc = plan_commit(l, channels, n_ch, d_crec, d_cwords, rows, false, &order)) return rc;
    if (!order.empty()) {
        ENTER_DEVICE(l->h);
        if (int rc = enqueue_commit(l, order, d_crec, d_cwords, (hipStream_t)stream)) return rc;
    }
    label_commit(order, rows, n_rows);
    return SR_OK;
}

int sr_onepass_live_commit(sr_onepass_live *l, const uint32_t *channels, uint32_t n_ch, sr_commit_rec *crec, sr_chain_word *cwords,
                           sr_chain_live_row *rows, uint32_t *n_rows)
{
    std::vector<sr_chain_live_row> order;
    if (int rc = plan_commit(l, channels, n_ch, crec, cwords, rows, true, &order)) return rc;
    if (!order.empty()) {
        ENTER_HOST_CALL(l->h);
        const size_t n_out = order.size(), n_w = n_out * l->words_cap;
        TmpDevBuf<sr_commit_rec> d_crec;  // per-call device copies of the outputs, reserved before anything is enqueued
        TmpDevBuf<sr_chain_word> d_cwords;
        if (int rc = d_crec.reserve(n_out)) return rc;
        if (int rc = d_cwords.reserve(n_w)) return rc;
        if (int rc = enqueue_commit(l, order, d_crec.p, d_cwords.p, nullptr)) return rc;
        COPY_DOWN(crec, d_crec.p, n_out * sizeof *crec);
        COPY_DOWN(cwords, d_cwords.p, n_w * sizeof *cwords);
    }
    label_commit(order, rows, n_rows);
    return SR_OK;
}

}  // extern "C"
