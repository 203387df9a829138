// What the two live decoding sessions (sr_decode_live.cpp, sr_gram_live.cpp) do alike on the host: the checks of a push's
// inputs and outputs, the plan upload, the PCM front end, the event that orders pushes on different streams, and the host
// forms' device copies of their outputs.  A session S has the members h, m (DecodeLiveMirror), max_words, n_words_exact,
// skip_cost, word_cost, mid, d_chan, keep, stage, recs, feat, keep_stride, stage_stride, ev_last, last_stream, pending: one
// definition of each rule serves both.  HOST ONLY.
#pragma once
#include "sr_decode_live_plan.h"
#include "sr_host_call.h"
#include "sr_live_pcm.h"

namespace sr {

inline bool live_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && na && nb && x < y + nb && y < x + na;
}

// store: the trace will read the store's frame counts and the word map -- the conditions of sr_decode_words_dp_dev on the
// engine, its current store and word map
template <typename S>
int check_outputs(const S *l, uint32_t n_out, uint32_t max_rows, const sr_chain_rec *rec, const sr_chain_word *words, const uint32_t *level_cost,
                  const sr_chain_live_row *rows, bool store = true)
{
    if (max_rows < n_out)
        return fail(SR_ERR_BAD_ARG, "max_rows " + std::to_string(max_rows) + " is below the " + std::to_string(n_out) + " rows of this call");
    if (!n_out) return SR_OK;
    if (store)
        if (int rc = check_chain(l->h, l->max_words, l->n_words_exact, l->skip_cost, l->word_cost)) return rc;
    if (!rec || !words || !rows) return fail(SR_ERR_BAD_ARG, "null argument");
    const size_t n_rec = (size_t)n_out * sizeof *rec, n_w = (size_t)n_out * l->max_words * sizeof *words, n_lc = (size_t)n_out * l->max_words * 4;
    if (live_overlap(rec, n_rec, words, n_w) || live_overlap(rec, n_rec, level_cost, n_lc) || live_overlap(words, n_w, level_cost, n_lc))
        return fail(SR_ERR_BAD_ARG, "rec, words and level_cost overlap");
    return SR_OK;
}

// sr_*_live_end: every output is a host buffer there, so the labels must not lie inside the records either
template <typename S>
int check_end_rows(const S *l, uint32_t n_out, const sr_chain_rec *rec, const sr_chain_word *words, const uint32_t *level_cost,
                   const sr_chain_live_row *rows)
{
    const size_t n_r = (size_t)n_out * sizeof *rows, n_w = (size_t)n_out * l->max_words;
    if (live_overlap(rows, n_r, rec, (size_t)n_out * sizeof *rec) || live_overlap(rows, n_r, words, n_w * sizeof *words) ||
        live_overlap(rows, n_r, level_cost, n_w * 4))
        return fail(SR_ERR_BAD_ARG, "rows overlaps rec, words or level_cost");
    return SR_OK;
}

template <typename S>
int check_frames_in(const S *l, const DecodeLivePlan &pl, const int16_t *mfcc, uint64_t row_stride, bool device)
{
    if (l->m.pcm) return fail(SR_ERR_BAD_ARG, "a PCM session takes samples (the session's push_pcm calls)");
    if (!pl.max_n) return SR_OK;
    if (!mfcc) return fail(SR_ERR_BAD_ARG, "null argument");
    if ((uint64_t)pl.max_n * kCoef > row_stride) return fail(SR_ERR_BAD_ARG, "a count exceeds row_stride");
    if (device && (((uintptr_t)mfcc & 7) || (row_stride & 3))) return fail(SR_ERR_BAD_ARG, "mfcc must be 8-byte aligned, row_stride % 4 == 0");
    if (!device && ((uintptr_t)mfcc & 1)) return fail(SR_ERR_BAD_ARG, "mfcc must be 2-byte aligned");
    return SR_OK;
}

template <typename S>
int check_pcm_in(const S *l, const DecodeLivePlan &pl, const uint16_t *pcm, uint64_t pcm_stride, bool device)
{
    if (!l->m.pcm) return fail(SR_ERR_BAD_ARG, "a feature session takes frames (the session's push calls)");
    if (!pl.max_n) return SR_OK;
    if (!pcm) return fail(SR_ERR_BAD_ARG, "null pcm");
    if (pl.max_n > pcm_stride) return fail(SR_ERR_BAD_ARG, "a count exceeds pcm_stride");
    if (device && (((uintptr_t)pcm & 15) || (pcm_stride & 7))) return fail(SR_ERR_BAD_ARG, "pcm must be 16-byte aligned, stride % 8 == 0");
    if (!device && ((uintptr_t)pcm & 1)) return fail(SR_ERR_BAD_ARG, "pcm must be 2-byte aligned");
    return SR_OK;
}

// (a pageable source is staged before the call returns: the plan may go out of scope)
template <typename S>
int upload_chan(S *l, const std::vector<SpotLiveChan> &chan, hipStream_t s)
{
    HIP_TRY(hipMemcpyAsync(l->d_chan.p, chan.data(), (size_t)l->m.C * sizeof(SpotLiveChan), hipMemcpyHostToDevice, s));
    return SR_OK;
}

template <typename S>
int launch_front_end(S *l, const DecodeLivePlan &pl, const uint16_t *d_pcm, uint64_t pcm_stride, hipStream_t s)
{
    return live_pcm_front_end(l->h, l->d_chan.p, pl.chan, l->mid, pl.max_row, pl.max_frames, d_pcm, pcm_stride, l->keep.p, l->keep_stride,
                              l->stage.p, l->stage_stride, l->recs.p, l->feat.p, s);
}

template <typename S>
int mark_push(S *l, hipStream_t s)
{
    HIP_TRY(hipEventRecord(l->ev_last, s));
    l->pending = true;
    l->last_stream = s;
    return SR_OK;
}

// the channels' state belongs to one push at a time: a push on another stream than the last one's runs behind it
template <typename S>
int order_after_last_push(S *l, hipStream_t s)
{
    if (!l->pending || s == l->last_stream) return SR_OK;
    HIP_TRY(hipStreamWaitEvent(s, l->ev_last, 0));
    return SR_OK;
}

// host forms: device copies of the outputs of n_out rows, and their way back
struct HostOutputs {
    TmpDevBuf<sr_chain_rec> rec;
    TmpDevBuf<sr_chain_word> words;
    TmpDevBuf<uint32_t> lc;
    int reserve(uint32_t n_out, uint32_t max_words, bool level_cost)
    {
        const size_t n_w = (size_t)std::max(n_out, 1u) * max_words;
        if (int rc = rec.reserve(std::max(n_out, 1u))) return rc;
        if (int rc = words.reserve(n_w)) return rc;
        return level_cost ? lc.reserve(n_w) : SR_OK;
    }
    int down(uint32_t n_out, uint32_t max_words, sr_chain_rec *h_rec, sr_chain_word *h_words, uint32_t *h_lc)
    {
        const size_t n_w = (size_t)n_out * max_words;
        COPY_DOWN(h_rec, rec.p, (size_t)n_out * sizeof *h_rec);
        COPY_DOWN(h_words, words.p, n_w * sizeof *h_words);
        if (h_lc) COPY_DOWN(h_lc, lc.p, n_w * 4);
        return SR_OK;
    }
};

}  // namespace sr
