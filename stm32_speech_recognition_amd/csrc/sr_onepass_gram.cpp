// One-pass grammar decoding (include/sr_engine.h, "one-pass grammar decoding"): the checks, the plan (sr_onepass_gram_plan.h:
// the kept items and states were listed when the grammar was compiled, sr_gram.cpp; the block length, the blocks and the
// launch groups are the one-pass decoder's -- host-only code) and the sequencing.  Per launch group: k_onepass_gram_init, per
// block (k_onepass_gram_words, k_onepass_gram_close), k_onepass_gram_trace, everything on the caller's stream; a grammar with
// a nonzero cost takes k_onepass_gram_words_w and k_onepass_gram_trace_w in their places.  frames_cap fixes the blocks,
// nothing is read back.  The host form stages its rows and outputs through sr_stage_host.h; the whole-path host form is in
// sr_host.cpp, next to sr_decode_onepass_batch.
#include "sr_stage_host.h"
#include "sr_onepass_gram_plan.h"

using namespace sr;

namespace {

struct Kept {
    uint32_t items, states;
    bool pruned;
};

// testing build: the hook keeps every item and every state
Kept kept_of(const sr_grammar *g)
{
    if (dev_hook(kHookOnePassGramPruneOff)) return Kept{g->n_items, g->n_states, false};
    return Kept{g->op_n_items, g->op_n_states, true};
}

OnePassGramPlan plan_for(const sr_grammar *g, const Kept &k, uint32_t frames_cap)
{
    // testing build: the one-pass decoder's hooks put seams and small groups into small test shapes
    const int64_t block = dev_hook(kHookOnePassBlock), rows = dev_hook(kHookOnePassRows);
    const sr_engine *h = g->h;
    return onepass_gram_plan(g->tpl_len, g->n_states, k.items, k.states, g->max_frames, frames_cap, onepass_reach(h->tpl_len_host.data(), h->K),
                             block > 0 ? (uint32_t)std::min<int64_t>(block, 16383) : 0u,
                             rows > 0 ? (uint32_t)std::min<int64_t>(rows, kOnePassMaxRows) : 0u);
}

int check_stage(const sr_engine *h, const sr_grammar *g, const void *mfcc, const void *frames, uint32_t frames_stride, uint32_t n_rows,
                uint32_t frames_cap, uint32_t words_cap, uint32_t skip_cost, uint32_t word_cost, const sr_chain_rec *rec, const sr_chain_word *words)
{
    if (!h || !mfcc || !frames || !rec || !words) return fail(SR_ERR_BAD_ARG, "null argument");
    if (int rc = check_onepass_grammar(h, g, frames_cap, words_cap, skip_cost, word_cost)) return rc;
    if (!frames_stride) return fail(SR_ERR_BAD_ARG, "frames_stride must be at least 1");
    if (overlap(rec, (size_t)n_rows * sizeof *rec, words, (size_t)n_rows * words_cap * sizeof *words))
        return fail(SR_ERR_BAD_ARG, "d_rec and d_words overlap");
    return SR_OK;
}

}  // namespace

int check_onepass_grammar(const sr_engine *h, const sr_grammar *g, uint32_t frames_cap, uint32_t words_cap, uint32_t skip_cost, uint32_t word_cost)
{
    if (int rc = check_chain(h, 1, 0, skip_cost, word_cost)) return rc;  // the decoder's conditions on the engine, the store and the costs
    if (int rc = check_grammar(h, g)) return rc;
    if (!words_cap) return fail(SR_ERR_BAD_ARG, "words_cap must be at least 1");
    const uint32_t cap = frames_cap && frames_cap < h->cfg.max_frames ? frames_cap : h->cfg.max_frames;
    if (!onepass_gram_cost_ok(cap, onepass_reach(h->tpl_len_host.data(), h->K), word_cost, g->max_arc_cost, g->max_final_cost))
        return fail(SR_ERR_BAD_ARG, "(frames_cap / L) * (word_cost + the grammar's largest arc cost) + its largest final cost must be at most 2^30, "
                                    "L = the shortest valid template's frames / 2 + 1");
    const OnePassGramPlan p = plan_for(g, kept_of(g), frames_cap);
    if (!p.fits)
        return fail(SR_ERR_BAD_ARG, "one row of this grammar needs row_bytes = " + std::to_string(p.row_bytes) + " of scratch, a launch group holds " +
                                        std::to_string(kOnePassScratch));
    return SR_OK;
}

extern "C" {

int sr_onepass_grammar_plan(const sr_grammar *g, uint32_t frames_cap, uint32_t out[6])
{
    if (!g || !out) return fail(SR_ERR_BAD_ARG, "null argument");
    const Kept k = kept_of(g);
    const OnePassGramPlan p = plan_for(g, k, frames_cap);
    out[0] = (uint32_t)std::min<size_t>(p.row_bytes, 0xFFFFFFFFu);
    out[1] = p.fits ? p.rows : 0u;
    out[2] = p.o.n;
    out[3] = p.launches;
    out[4] = k.items;
    out[5] = k.states;
    return SR_OK;
}

int sr_decode_onepass_grammar_dp_dev(sr_engine *h, const sr_grammar *g, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride,
                                     uint32_t n_rows, uint32_t frames_cap, uint32_t words_cap, uint32_t skip_cost, uint32_t word_cost,
                                     sr_chain_rec *d_rec, sr_chain_word *d_words, void *stream)
{
    int rc = check_stage(h, g, d_mfcc, d_in_frames, frames_stride, n_rows, frames_cap, words_cap, skip_cost, word_cost, d_rec, d_words);
    if (rc || !n_rows) return rc;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    const Kept k = kept_of(g);
    const OnePassGramPlan p = plan_for(g, k, frames_cap);
    const uint32_t per = std::min(p.rows, n_rows);
    if ((rc = order_after_scratch_users(h, s))) return rc;  // the keys, the prefix costs and the saved columns are the engine's
    if ((rc = h->s_ch_a.reserve(per * p.a_row)) || (rc = h->s_ch_e.reserve(per * p.e_row)) ||
        (rc = h->s_op_cols.reserve(std::max<size_t>(per * p.col_row, 1))))
        return rc;
    const WordTab wt = word_tab(h);
    OnePassGramArgs a{};
    a.n_states = g->n_states;
    a.n_items = g->n_items;
    a.n_keep_items = k.items;
    a.n_keep_states = k.states;
    a.masks = g->blob.p;
    a.items = (const GramItem *)(g->blob.p + g->items_at);
    a.final_state = (const uint8_t *)(g->blob.p + g->final_at);
    a.keep_items = k.pruned ? (const uint32_t *)(g->blob.p + g->op_items_at) : nullptr;
    a.keep_states = k.pruned ? (const uint32_t *)(g->blob.p + g->op_states_at) : nullptr;
    const GramCosts w = g->costs();
    for (uint32_t r0 = 0; r0 < n_rows; r0 += per) {  // the groups follow each other on s: one scratch serves them all
        a.o = OnePassArgs{d_mfcc + (size_t)r0 * h->cfg.max_frames * kCoef, d_in_frames + (size_t)r0 * frames_stride, frames_stride,
                          std::min(per, n_rows - r0), h->cfg.max_frames, p.o.cap, h->tpl.p, h->tpl_frames.p, h->tpl_valid.p, h->K,
                          h->tpl_stride, g->tpl_len, words_cap, skip_cost, word_cost, h->s_ch_a.p, h->s_ch_e.p, h->s_op_cols.p,
                          wt.group_of_slot, wt.word_id, d_rec + r0, d_words + (size_t)r0 * words_cap};
        launch_onepass_gram(a, g->weighted ? &w : nullptr, p.o.blocks.data(), (uint32_t)p.o.blocks.size(), s);
    }
    HIP_TRY(hipGetLastError());
    return mark_scratch_user(h, s);
}

int sr_decode_onepass_grammar_dp(sr_engine *h, const sr_grammar *g, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride,
                                 uint32_t n_rows, uint32_t frames_cap, uint32_t words_cap, uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *rec,
                                 sr_chain_word *words)
{
    int rc = check_stage(h, g, mfcc, in_frames, frames_stride, n_rows, frames_cap, words_cap, skip_cost, word_cost, rec, words);
    if (rc || !n_rows) return rc;
    return decode_rows_host(h, mfcc, in_frames, frames_stride, n_rows, words_cap, rec, words, nullptr,
                            [&](const int16_t *d_mfcc, const uint32_t *d_frames, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *) {
                                return sr_decode_onepass_grammar_dp_dev(h, g, d_mfcc, d_frames, 1, n_rows, frames_cap, words_cap, skip_cost, word_cost,
                                                                        d_rec, d_words, nullptr);
                            });
}

}  // extern "C"
