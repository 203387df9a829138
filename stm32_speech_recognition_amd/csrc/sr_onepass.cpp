// One-pass connected-word decoding (include/sr_engine.h, "one-pass connected-word decoding"): the checks, the plan
// (sr_onepass_plan.h: the block length from the host mirror of the store's template lengths, the blocks, the launch groups --
// host-only code) and the sequencing.  Per launch group: k_onepass_init, per block (k_onepass_words, k_onepass_close),
// k_onepass_trace, everything on the caller's stream; frames_cap fixes the blocks, nothing is read back.  The host form stages
// its rows and outputs through sr_stage_host.h; the whole-path host form is in sr_host.cpp, next to sr_decode_words_batch.
#include "sr_stage_host.h"

using namespace sr;

static OnePassPlan plan_for(uint32_t tpl_len, uint32_t K, uint32_t max_frames, uint32_t frames_cap, uint32_t L)
{
    // testing build: short blocks and small groups put seams into small test shapes
    const int64_t block = dev_hook(kHookOnePassBlock), rows = dev_hook(kHookOnePassRows);
    return onepass_plan(tpl_len, K, max_frames, frames_cap, L, block > 0 ? (uint32_t)std::min<int64_t>(block, 16383) : 0u,
                        rows > 0 ? (uint32_t)std::min<int64_t>(rows, kOnePassMaxRows) : 0u);
}

int check_onepass(const sr_engine *h, uint32_t frames_cap, uint32_t words_cap, uint32_t skip_cost, uint32_t word_cost)
{
    if (int rc = check_chain(h, 1, 0, skip_cost, word_cost)) return rc;  // the decoder's conditions on the engine, the store and the costs
    if (!words_cap) return fail(SR_ERR_BAD_ARG, "words_cap must be at least 1");
    const uint32_t cap = frames_cap && frames_cap < h->cfg.max_frames ? frames_cap : h->cfg.max_frames;
    if (!onepass_cost_ok(cap, onepass_reach(h->tpl_len_host.data(), h->K), word_cost))
        return fail(SR_ERR_BAD_ARG, "(frames_cap / L) * word_cost must be at most 2^30, L = the shortest valid template's frames / 2 + 1");
    return SR_OK;
}

static int check_stage(const sr_engine *h, const void *mfcc, const void *frames, uint32_t frames_stride, uint32_t n_rows, uint32_t frames_cap,
                       uint32_t words_cap, uint32_t skip_cost, uint32_t word_cost, const sr_chain_rec *rec, const sr_chain_word *words)
{
    if (!h || !mfcc || !frames || !rec || !words) return fail(SR_ERR_BAD_ARG, "null argument");
    if (int rc = check_onepass(h, frames_cap, words_cap, skip_cost, word_cost)) return rc;
    if (!frames_stride) return fail(SR_ERR_BAD_ARG, "frames_stride must be at least 1");
    if (overlap(rec, (size_t)n_rows * sizeof *rec, words, (size_t)n_rows * words_cap * sizeof *words))
        return fail(SR_ERR_BAD_ARG, "d_rec and d_words overlap");
    return SR_OK;
}

extern "C" {

int sr_decode_onepass_geometry(uint32_t tpl_rows, uint32_t K, uint32_t max_frames, uint32_t min_tpl_frames, uint32_t out[4])
{
    if (!out || !tpl_rows || tpl_rows > 16383 || !K || K > kChainMaxSlots || max_frames < 2 || max_frames > 16383 || !min_tpl_frames ||
        min_tpl_frames > tpl_rows)
        return fail(SR_ERR_BAD_ARG, "null / zero argument");
    const OnePassPlan p = plan_for(tpl_rows, K, max_frames, 0u, min_tpl_frames / 2u + 1u);
    out[0] = (uint32_t)std::min<size_t>(p.row_bytes, 0xFFFFFFFFu);
    out[1] = p.rows;
    out[2] = p.n;
    out[3] = p.launches;
    return SR_OK;
}

int sr_decode_onepass_dp_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                             uint32_t frames_cap, uint32_t words_cap, uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *d_rec,
                             sr_chain_word *d_words, void *stream)
{
    int rc = check_stage(h, d_mfcc, d_in_frames, frames_stride, n_rows, frames_cap, words_cap, skip_cost, word_cost, d_rec, d_words);
    if (rc || !n_rows) return rc;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t tpl_len = store_tpl_len(h);
    const OnePassPlan p = plan_for(tpl_len, h->K, h->cfg.max_frames, frames_cap, onepass_reach(h->tpl_len_host.data(), h->K));
    const uint32_t per = std::min(p.rows, n_rows);
    if ((rc = order_after_scratch_users(h, s))) return rc;  // the keys, the prefix costs and the saved columns are the engine's
    if ((rc = h->s_ch_a.reserve(per * p.a_row)) || (rc = h->s_ch_e.reserve(per * p.e_row)) || (rc = h->s_op_cols.reserve(per * p.col_row))) return rc;
    const WordTab wt = word_tab(h);
    for (uint32_t r0 = 0; r0 < n_rows; r0 += per) {  // the groups follow each other on s: one scratch serves them all
        launch_onepass(OnePassArgs{d_mfcc + (size_t)r0 * h->cfg.max_frames * kCoef, d_in_frames + (size_t)r0 * frames_stride, frames_stride,
                                   std::min(per, n_rows - r0), h->cfg.max_frames, p.cap, h->tpl.p, h->tpl_frames.p, h->tpl_valid.p, h->K,
                                   h->tpl_stride, tpl_len, words_cap, skip_cost, word_cost, h->s_ch_a.p, h->s_ch_e.p, h->s_op_cols.p,
                                   wt.group_of_slot, wt.word_id, d_rec + r0,
                                   d_words + (size_t)r0 * words_cap},
                       p.blocks.data(), (uint32_t)p.blocks.size(), s);
    }
    HIP_TRY(hipGetLastError());
    return mark_scratch_user(h, s);
}

int sr_decode_onepass_dp(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                         uint32_t frames_cap, uint32_t words_cap, uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *rec, sr_chain_word *words)
{
    int rc = check_stage(h, mfcc, in_frames, frames_stride, n_rows, frames_cap, words_cap, skip_cost, word_cost, rec, words);
    if (rc || !n_rows) return rc;
    return decode_rows_host(h, mfcc, in_frames, frames_stride, n_rows, words_cap, rec, words, nullptr,
                            [&](const int16_t *d_mfcc, const uint32_t *d_frames, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *) {
                                return sr_decode_onepass_dp_dev(h, d_mfcc, d_frames, 1, n_rows, frames_cap, words_cap, skip_cost, word_cost, d_rec, d_words,
                                                                nullptr);
                            });
}

}  // extern "C"
