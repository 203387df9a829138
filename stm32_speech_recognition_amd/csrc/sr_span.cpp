// Word alternatives (include/sr_engine.h, "word alternatives"): the checks and the launches of the span scorer (k_span.hip),
// and the unconstrained decoder with alternatives -- sr_decode_words_dp_dev as it stands, k_span_words over its word rows,
// sr_nbest_batch_dev's reduction over the span score rows -- everything on the caller's stream.  The host knows every count:
// nothing is read back.  The host forms stage their rows (and the decoder's outputs) through sr_stage_host.h.
#include "sr_stage_host.h"

using namespace sr;

static constexpr uint32_t kSpanMaxSpans = 0x7FFFFFFFu;

// the conditions of sr_score_word_spans_dev on the engine, the store and the parameters (not on the buffers)
static int check_span(const sr_engine *h, uint32_t frames_stride, uint32_t n_rows, uint32_t words_per_row, uint32_t mode)
{
    if (h->nc != (uint32_t)kCoef) return fail(SR_ERR_BAD_CONFIG, "the span scorer is built for 12-coefficient records");
    if (!h->K) return fail(SR_ERR_NO_TEMPLATES, "no templates set");
    if (!frames_stride) return fail(SR_ERR_BAD_ARG, "frames_stride must be at least 1");
    if (words_per_row < 1 || words_per_row > kChainMaxWords) return fail(SR_ERR_BAD_ARG, "words_per_row must be 1..16");
    if (mode != SR_SPAN_ACC && mode != SR_SPAN_DIS) return fail(SR_ERR_BAD_ARG, "mode must be SR_SPAN_ACC or SR_SPAN_DIS");
    if ((uint64_t)n_rows * words_per_row > kSpanMaxSpans) return fail(SR_ERR_BAD_ARG, "too many spans");
    if (h->K > kChainMaxSlots) return fail(SR_ERR_BAD_ARG, "the span scorer takes a store of at most 65536 slots");
    if (store_tpl_len(h) > spot_max_tpl(h->lds)) return fail(SR_ERR_BAD_ARG, "templates too long for the span scorer's LDS image");
    return SR_OK;
}

static int check_span_stage(const sr_engine *h, const void *mfcc, const void *frames, uint32_t frames_stride, uint32_t n_rows,
                            uint32_t words_per_row, const sr_chain_word *words, uint32_t mode, const uint32_t *scores)
{
    if (!h || !mfcc || !frames || !words || !scores) return fail(SR_ERR_BAD_ARG, "null argument");
    if (int rc = check_span(h, frames_stride, n_rows, words_per_row, mode)) return rc;
    const size_t n = (size_t)n_rows * words_per_row;
    if (overlap(words, n * sizeof *words, scores, n * h->K * 4)) return fail(SR_ERR_BAD_ARG, "d_words and d_scores overlap");
    return SR_OK;
}

static void launch_span_stage(const sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_frames, uint32_t frames_stride, uint32_t n_rows,
                              uint32_t words_per_row, const sr_chain_word *d_words, uint32_t mode, uint32_t *d_scores, hipStream_t s)
{
    // testing build: few groups per launch put slice seams into small test shapes
    const int64_t groups = dev_hook(kHookSpanGroups);
    launch_span(SpanArgs{d_mfcc, d_frames, frames_stride, h->cfg.max_frames, h->tpl.p, h->tpl_frames.p, h->tpl_valid.p, h->K, h->tpl_stride,
                         store_tpl_len(h), d_words, words_per_row, n_rows * words_per_row, mode,
                         groups > 0 ? (uint32_t)std::min<int64_t>(groups, 65535) : 65535u, d_scores},
                s);
}

extern "C" {

int sr_score_word_spans_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                            uint32_t words_per_row, const sr_chain_word *d_words, uint32_t mode, uint32_t *d_scores, void *stream)
{
    int rc = check_span_stage(h, d_mfcc, d_in_frames, frames_stride, n_rows, words_per_row, d_words, mode, d_scores);
    if (rc || !n_rows) return rc;
    ENTER_DEVICE(h);
    launch_span_stage(h, d_mfcc, d_in_frames, frames_stride, n_rows, words_per_row, d_words, mode, d_scores, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

int sr_score_word_spans(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                        uint32_t words_per_row, const sr_chain_word *words, uint32_t mode, uint32_t *scores)
{
    int rc = check_span_stage(h, mfcc, in_frames, frames_stride, n_rows, words_per_row, words, mode, scores);
    if (rc || !n_rows) return rc;
    ENTER_HOST_CALL(h);
    const size_t n = (size_t)n_rows * words_per_row;
    if ((rc = stage_rows(h, mfcc, in_frames, frames_stride, n_rows)) || (rc = h->s_span_words.reserve(n)) ||
        (rc = h->s_span_scores.reserve(n * h->K)))
        return rc;
    COPY_UP(h->s_span_words.p, words, n * sizeof *words);
    launch_span_stage(h, h->s_mfcc.p, h->s_u32a.p, 1, n_rows, words_per_row, h->s_span_words.p, mode, h->s_span_scores.p, nullptr);
    HIP_TRY(hipGetLastError());
    COPY_DOWN(scores, h->s_span_scores.p, n * h->K * 4);
    return SR_OK;
}

// what the alternatives add to the decoder's checks: the N-best rules, the mode, and outputs that keep clear of each other
static int check_alts(const sr_engine *h, uint32_t n_rows, uint32_t max_words, const sr_chain_rec *rec, const sr_chain_word *words,
                      const uint32_t *level_cost, uint32_t n_best, uint32_t mode, const sr_nbest_entry *alts, const uint32_t *n_matched,
                      const uint32_t *span_scores)
{
    if (int rc = check_nbest(h, n_best, alts)) return rc;
    if (int rc = check_span(h, 1, n_rows, max_words, mode)) return rc;
    const size_t n_w = (size_t)n_rows * max_words;
    const void *buf[6] = {rec, words, level_cost, alts, n_matched, span_scores};
    const size_t len[6] = {(size_t)n_rows * sizeof *rec, n_w * sizeof *words, n_w * 4, n_w * n_best * sizeof *alts, n_w * 4, n_w * h->K * 4};
    for (int i = 0; i < 6; i++)
        for (int j = i < 3 ? 3 : i + 1; j < 6; j++)  // (the decoder's own three have been checked against each other)
            if (overlap(buf[i], len[i], buf[j], len[j])) return fail(SR_ERR_BAD_ARG, "d_alts, d_n_matched, d_span_scores and the decoder's outputs overlap");
    return SR_OK;
}

int sr_decode_words_alts_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                             uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *d_rec,
                             sr_chain_word *d_words, uint32_t *d_level_cost, uint32_t n_best, uint32_t mode, sr_nbest_entry *d_alts,
                             uint32_t *d_n_matched, uint32_t *d_span_scores, void *stream)
{
    int rc = check_chain_stage(h, d_mfcc, d_in_frames, frames_stride, n_rows, max_words, n_words_exact, skip_cost, word_cost, d_rec, d_words,
                               d_level_cost);
    if (rc || (rc = check_alts(h, n_rows, max_words, d_rec, d_words, d_level_cost, n_best, mode, d_alts, d_n_matched, d_span_scores)) || !n_rows)
        return rc;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t n_w = n_rows * max_words;
    if (!d_span_scores) {  // the scores are the engine's: behind every earlier user of its scratch, as the decoder's keys
        if ((rc = order_after_scratch_users(h, s)) || (rc = h->s_span_scores.reserve((size_t)n_w * h->K))) return rc;
        d_span_scores = h->s_span_scores.p;
    }
    if ((rc = sr_decode_words_dp_dev(h, d_mfcc, d_in_frames, frames_stride, n_rows, max_words, n_words_exact, skip_cost, word_cost, d_rec,
                                     d_words, d_level_cost, stream)))
        return rc;
    launch_span_stage(h, d_mfcc, d_in_frames, frames_stride, n_rows, max_words, d_words, mode, d_span_scores, s);
    launch_nbest(nbest_args(h, d_span_scores, n_w, NbestOut{n_best, d_alts, d_n_matched}, 0), s);
    HIP_TRY(hipGetLastError());
    return mark_scratch_user(h, s);
}

int sr_decode_words_alts(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                         uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *rec,
                         sr_chain_word *words, uint32_t *level_cost, uint32_t n_best, uint32_t mode, sr_nbest_entry *alts,
                         uint32_t *n_matched, uint32_t *span_scores)
{
    int rc = check_chain_stage(h, mfcc, in_frames, frames_stride, n_rows, max_words, n_words_exact, skip_cost, word_cost, rec, words, level_cost);
    if (rc || (rc = check_alts(h, n_rows, max_words, rec, words, level_cost, n_best, mode, alts, n_matched, span_scores)) || !n_rows) return rc;
    ENTER_HOST_CALL(h);
    const size_t n_w = (size_t)n_rows * max_words;
    HostOutputs o(n_rows, max_words, rec, words, level_cost);  // the decoder's three; the alternatives' own copies beside them
    TmpDevBuf<uint32_t> d_nm;
    TmpDevBuf<sr_nbest_entry> d_alts;
    if ((rc = stage_rows(h, mfcc, in_frames, frames_stride, n_rows)) || (rc = o.reserve()) || (rc = d_alts.reserve(n_w * n_best)) ||
        (n_matched && (rc = d_nm.reserve(n_w))))
        return rc;
    if ((rc = sr_decode_words_alts_dev(h, h->s_mfcc.p, h->s_u32a.p, 1, n_rows, max_words, n_words_exact, skip_cost, word_cost, o.rec.p, o.words.p,
                                       o.lc.p, n_best, mode, d_alts.p, n_matched ? d_nm.p : nullptr, nullptr, nullptr)) ||
        (rc = o.down()))
        return rc;
    COPY_DOWN(alts, d_alts.p, n_w * n_best * sizeof *alts);
    if (n_matched) COPY_DOWN(n_matched, d_nm.p, n_w * 4);
    if (span_scores) COPY_DOWN(span_scores, h->s_span_scores.p, n_w * h->K * 4);  // the scratch the device form left them in
    return SR_OK;
}

}  // extern "C"
