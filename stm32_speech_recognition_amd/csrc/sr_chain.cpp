// Connected-word decoding (include/sr_engine.h, "connected-word decoding"): the checks, the launch plan (chain_plan,
// sr_dtw_plan.h) and the slicing of a call into launch groups whose keys and prefix costs fit the engine's scratch.  Per group:
// k_chain_init, max_words x (k_chain_words, k_chain_close), k_chain_trace, everything on the caller's stream.  The host form
// stages its rows and outputs through sr_stage_host.h; the whole-path host form is in sr_host.cpp, next to sr_spot_batch.
#include "sr_stage_host.h"

using namespace sr;

static ChainPlan plan_for(uint32_t tpl_len, uint32_t max_frames, uint32_t max_words)
{
    // testing build: small chunks and small groups put seams into small test shapes
    const int64_t cols = dev_hook(kHookChainChunk), rows = dev_hook(kHookChainRows);
    return chain_plan(tpl_len, max_frames, max_words, cols > 0 ? (uint32_t)std::min<int64_t>(cols, 16383) : 0u,
                      rows > 0 ? (uint32_t)std::min<int64_t>(rows, kChainMaxRows) : 0u);
}

static int check_limits(uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost)
{
    if (max_words < 1 || max_words > kChainMaxWords) return fail(SR_ERR_BAD_ARG, "max_words must be 1..16");
    if (n_words_exact > max_words) return fail(SR_ERR_BAD_ARG, "n_words_exact exceeds max_words");
    if (skip_cost > 65535u && skip_cost != SR_DIS_ERR) return fail(SR_ERR_BAD_ARG, "skip_cost must be at most 65535, or SR_DIS_ERR for no skipping");
    if (word_cost > (1u << 24)) return fail(SR_ERR_BAD_ARG, "word_cost must be at most 2^24");
    return SR_OK;
}

int check_chain(const sr_engine *h, uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost)
{
    if (h->nc != (uint32_t)kCoef) return fail(SR_ERR_BAD_CONFIG, "the connected-word decoder is built for 12-coefficient records");
    if (!h->K) return fail(SR_ERR_NO_TEMPLATES, "no templates set");
    if (int rc = check_limits(max_words, n_words_exact, skip_cost, word_cost)) return rc;
    if (h->K > kChainMaxSlots) return fail(SR_ERR_BAD_ARG, "the connected-word decoder takes a store of at most 65536 slots");
    if (store_tpl_len(h) > spot_max_tpl(h->lds)) return fail(SR_ERR_BAD_ARG, "templates too long for the connected-word decoder's LDS image");
    if (h->wg_K != h->K) return fail(SR_ERR_BAD_ARG, "the word map does not fit the template store");
    return SR_OK;
}

int check_chain_stage(const sr_engine *h, const void *mfcc, const void *frames, uint32_t frames_stride, uint32_t n_rows, uint32_t max_words,
                      uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost, const sr_chain_rec *rec, const sr_chain_word *words,
                      const uint32_t *level_cost)
{
    if (!h || !mfcc || !frames || !rec || !words) return fail(SR_ERR_BAD_ARG, "null argument");
    if (int rc = check_chain(h, max_words, n_words_exact, skip_cost, word_cost)) return rc;
    if (!frames_stride) return fail(SR_ERR_BAD_ARG, "frames_stride must be at least 1");
    const size_t n_rec = (size_t)n_rows * sizeof *rec, n_w = (size_t)n_rows * max_words * sizeof *words, n_lc = (size_t)n_rows * max_words * 4;
    if (overlap(rec, n_rec, words, n_w) || overlap(rec, n_rec, level_cost, n_lc) || overlap(words, n_w, level_cost, n_lc))
        return fail(SR_ERR_BAD_ARG, "d_rec, d_words and d_level_cost overlap");
    return SR_OK;
}

extern "C" {

int sr_decode_geometry(uint32_t tpl_rows, uint32_t max_frames, uint32_t max_words, uint32_t out[4])
{
    if (!out || !tpl_rows || tpl_rows > 16383 || max_frames < 2 || max_frames > 16383 || max_words < 1 || max_words > kChainMaxWords)
        return fail(SR_ERR_BAD_ARG, "null / zero argument");
    const LdsBudget mi355x;  // no device: MI355X's figures
    const ChainPlan p = plan_for(tpl_rows, max_frames, max_words);
    out[0] = (uint32_t)p.row_bytes;
    out[1] = p.rows;
    out[2] = spot_max_tpl(mi355x);
    out[3] = p.g.chunk_cols;
    return SR_OK;
}

int sr_decode_words_dp_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                           uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *d_rec,
                           sr_chain_word *d_words, uint32_t *d_level_cost, void *stream)
{
    int rc = check_chain_stage(h, d_mfcc, d_in_frames, frames_stride, n_rows, max_words, n_words_exact, skip_cost, word_cost, d_rec, d_words,
                               d_level_cost);
    if (rc || !n_rows) return rc;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    const ChainPlan p = plan_for(store_tpl_len(h), h->cfg.max_frames, max_words);
    const uint32_t per = std::min(p.rows, n_rows);
    if ((rc = order_after_scratch_users(h, s))) return rc;  // the keys and prefix costs are the engine's
    if ((rc = h->s_ch_a.reserve(per * p.a_row)) || (rc = h->s_ch_e.reserve(per * p.e_row))) return rc;
    const WordTab wt = word_tab(h);
    for (uint32_t r0 = 0; r0 < n_rows; r0 += per) {  // the groups follow each other on s: one scratch serves them all
        launch_chain(ChainArgs{d_mfcc + (size_t)r0 * h->cfg.max_frames * kCoef, d_in_frames + (size_t)r0 * frames_stride, frames_stride,
                               std::min(per, n_rows - r0), h->cfg.max_frames, h->tpl.p, h->tpl_frames.p, h->tpl_valid.p, h->K, h->tpl_stride,
                               store_tpl_len(h), p.g.chunk_cols, p.g.n_chunks, max_words, n_words_exact, skip_cost, word_cost, h->s_ch_a.p,
                               h->s_ch_e.p, wt.group_of_slot, wt.word_id, d_rec + r0, d_words + (size_t)r0 * max_words,
                               d_level_cost ? d_level_cost + (size_t)r0 * max_words : nullptr},
                     s);
    }
    HIP_TRY(hipGetLastError());
    return mark_scratch_user(h, s);
}

int sr_decode_words_dp(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                       uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *rec,
                       sr_chain_word *words, uint32_t *level_cost)
{
    int rc = check_chain_stage(h, mfcc, in_frames, frames_stride, n_rows, max_words, n_words_exact, skip_cost, word_cost, rec, words, level_cost);
    if (rc || !n_rows) return rc;
    return decode_rows_host(h, mfcc, in_frames, frames_stride, n_rows, max_words, rec, words, level_cost,
                            [&](const int16_t *d_mfcc, const uint32_t *d_frames, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_lc) {
                                return sr_decode_words_dp_dev(h, d_mfcc, d_frames, 1, n_rows, max_words, n_words_exact, skip_cost, word_cost, d_rec,
                                                              d_words, d_lc, nullptr);
                            });
}

}  // extern "C"
