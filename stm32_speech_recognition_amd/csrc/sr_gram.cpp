// Grammar-constrained decoding (include/sr_engine.h, "grammar-constrained decoding" and "weighted grammars"): a grammar
// compiled against the engine's store and word map (the construction itself is host-only code, sr_gram_compile.h), the
// checks, the plan (which items each level keeps, the scratch of a row) and the slicing of a call into launch groups.  Per
// group: k_gram_init, per level that keeps items (k_gram_charge, k_gram_words, k_gram_close), k_gram_trace, everything on the
// caller's stream; a grammar with a nonzero cost takes k_gram_charge_w and k_gram_trace_w in their places.  The host form
// stages its rows and outputs through sr_stage_host.h; the whole-path host form is in sr_host.cpp, next to sr_decode_words_batch.
#include "sr_gram_compile.h"
#include "sr_stage_host.h"
#include "sr_onepass_gram_plan.h"

using namespace sr;

// (the compiled form, struct sr_grammar, is in sr_engine_internal.h: the live session of sr_gram_live.cpp reads it too)
namespace {

struct Scratch {
    size_t a_row, e_row, c_row, row_bytes;
    uint32_t rows;
    SpotGeom g;
};

Scratch gram_plan(const sr_grammar *g, uint32_t max_words)
{
    // testing build: the decoder's hooks put seams and small groups into small test shapes
    const int64_t cols = dev_hook(kHookChainChunk), rows = dev_hook(kHookChainRows);
    const ChainPlan cp = chain_plan(g->tpl_len, g->max_frames, max_words, cols > 0 ? (uint32_t)std::min<int64_t>(cols, 16383) : 0u, 0u);
    Scratch p;
    p.g = cp.g;
    const size_t P = g->max_frames + 1u;
    p.a_row = (size_t)max_words * g->n_states * P;
    p.e_row = (size_t)(max_words + 1u) * g->n_states * P;
    p.c_row = (size_t)g->n_sets * P;
    p.row_bytes = p.a_row * 8u + (p.e_row + p.c_row) * 4u;
    const size_t fit = kChainScratch / p.row_bytes;
    p.rows = (uint32_t)(fit < 1 ? 1 : fit > kChainMaxRows ? kChainMaxRows : fit);
    if (rows > 0) p.rows = (uint32_t)std::min<int64_t>(rows, kChainMaxRows);
    return p;
}

}  // namespace

// what level l (1-based) of a call with max_words keeps
GramLevel gram_level_of(const sr_grammar *g, uint32_t l, uint32_t max_words)
{
    const sr_grammar::Level &v = g->lv[l - 1];
    const uint32_t j = max_words - l + 1;  // distances 0..max_words - l
    return GramLevel{v.item0, v.items[j], v.set0, v.sets[j], v.state0, v.states[j]};
}

int check_grammar(const sr_engine *h, const sr_grammar *g)
{
    if (!g) return fail(SR_ERR_BAD_ARG, "null grammar");
    if (g->h != h) return fail(SR_ERR_BAD_ARG, "the grammar belongs to another engine");
    if (g->store_serial != h->store_serial) return fail(SR_ERR_BAD_ARG, "the template store changed since the grammar was compiled");
    if (g->word_serial != h->word_serial) return fail(SR_ERR_BAD_ARG, "the word map changed since the grammar was compiled");
    return SR_OK;
}

extern "C" {

int sr_grammar_create_weighted(sr_engine *h, uint32_t n_states, const sr_gram_arc *arcs, const uint32_t *arc_cost, uint32_t n_arcs,
                               const uint8_t *final_state, const uint32_t *final_cost, sr_grammar **out)
{
    if (!h || !arcs || !final_state || !out) return fail(SR_ERR_BAD_ARG, "null argument");
    if (int rc = check_chain(h, 1, 0, SR_DIS_ERR, 0)) return rc;  // the engine and the store, as every decode call
    const uint32_t S = n_states, K = h->K;
    std::vector<uint32_t> label(K);
    for (uint32_t k = 0; k < K; k++) label[k] = h->word_explicit ? h->word_labels[k] : k / h->word_spw;
    GramNet net;
    std::string why;
    if (!gram_check(n_states, arcs, arc_cost, n_arcs, final_state, final_cost, label, &net, &why)) return fail(SR_ERR_BAD_ARG, why);

    ENTER_DEVICE(h);
    // slots(w): the VALID slots of the store, which lives on the device
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint8_t> valid(K);
    std::vector<uint32_t> frames(K);
    HIP_TRY(hipMemcpy(valid.data(), h->tpl_valid.p, K, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(frames.data(), h->tpl_frames.p, (size_t)K * 4, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < K; k++) valid[k] = valid[k] && frames[k];
    GramCompiled c;
    if (!gram_build(net, arcs, n_arcs, label, valid, &c, &why)) return fail(SR_ERR_BAD_ARG, why);

    sr_grammar *g = new sr_grammar();
    g->h = h;
    g->store_serial = h->store_serial;
    g->word_serial = h->word_serial;
    g->n_states = S;
    g->n_sets = (uint32_t)c.masks.size();
    g->n_items = (uint32_t)c.items.size();
    g->max_frames = h->cfg.max_frames;
    g->tpl_len = store_tpl_len(h);
    g->weighted = net.weighted;
    std::copy(c.lv, c.lv + kChainMaxWords, g->lv);

    g->items_at = c.masks.size();
    g->lists_at = g->items_at + c.items.size() * 2;
    g->final_at = g->lists_at + (c.lists.size() + 1) / 2;
    size_t end = g->final_at + (S + 7) / 8;
    if (g->weighted) {  // a grammar without a nonzero cost uploads what it always has
        g->cost_off_at = end;
        g->costs_at = g->cost_off_at + (c.cost_off.size() + 1) / 2;
        g->final_cost_at = g->costs_at + (c.costs.size() + 1) / 2;
        end = g->final_cost_at + (S + 1) / 2;
    }
    // one-pass grammar decoding (sr_onepass_gram.cpp): its static lists, built once, behind everything the level decoders read
    const OnePassGramKeep keep = onepass_gram_keep(S, arcs, n_arcs, net.finals, c.items.data(), g->n_items, c.masks.data(), true);
    g->op_n_items = (uint32_t)keep.items.size();
    g->op_n_states = (uint32_t)keep.states.size();
    for (uint32_t i : keep.items) g->op_item_slots.push_back(c.items[i].slot);
    g->op_items_at = end;
    g->op_states_at = g->op_items_at + (keep.items.size() + 1) / 2;
    end = g->op_states_at + (keep.states.size() + 1) / 2;
    for (uint32_t i = 0; i < n_arcs; i++) g->max_arc_cost = std::max(g->max_arc_cost, arc_cost ? arc_cost[i] : 0u);
    for (uint32_t s = 0; s < S; s++) g->max_final_cost = std::max(g->max_final_cost, net.final_cost[s]);
    std::vector<unsigned long long> blob(end, 0ull);
    if (!keep.items.empty()) std::memcpy(blob.data() + g->op_items_at, keep.items.data(), keep.items.size() * 4);
    if (!keep.states.empty()) std::memcpy(blob.data() + g->op_states_at, keep.states.data(), keep.states.size() * 4);
    std::memcpy(blob.data(), c.masks.data(), c.masks.size() * 8);
    if (!c.items.empty()) std::memcpy(blob.data() + g->items_at, c.items.data(), c.items.size() * sizeof(GramItem));
    if (!c.lists.empty()) std::memcpy(blob.data() + g->lists_at, c.lists.data(), c.lists.size() * 4);
    for (uint32_t s = 0; s < S; s++) ((uint8_t *)(blob.data() + g->final_at))[s] = final_state[s] ? 1 : 0;
    if (g->weighted) {
        std::memcpy(blob.data() + g->cost_off_at, c.cost_off.data(), c.cost_off.size() * 4);
        if (!c.costs.empty()) std::memcpy(blob.data() + g->costs_at, c.costs.data(), c.costs.size() * 4);
        std::memcpy(blob.data() + g->final_cost_at, net.final_cost.data(), (size_t)S * 4);
    }
    int rc = g->blob.reserve(blob.size());
    if (!rc) {
        const hipError_t e = hipMemcpy(g->blob.p, blob.data(), blob.size() * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail(SR_ERR_HIP, std::string("grammar upload: ") + hipGetErrorString(e));
    }
    if (rc) {
        g->blob.release();
        delete g;
        return rc;
    }
    *out = g;
    return SR_OK;
}

int sr_grammar_create(sr_engine *h, uint32_t n_states, const sr_gram_arc *arcs, uint32_t n_arcs, const uint8_t *final_state,
                      sr_grammar **out)
{
    return sr_grammar_create_weighted(h, n_states, arcs, nullptr, n_arcs, final_state, nullptr, out);
}

void sr_grammar_destroy(sr_grammar *g)
{
    if (!g) return;
    DeviceGuard guard;
    if (guard.enter(g->h->device) == SR_OK) (void)hipDeviceSynchronize();  // a decode call in flight may still read the lists
    g->blob.release();
    delete g;
}

int sr_grammar_plan(const sr_grammar *g, uint32_t max_words, uint32_t *items_per_level, uint32_t out[4])
{
    if (!g || !out) return fail(SR_ERR_BAD_ARG, "null argument");
    if (max_words < 1 || max_words > kChainMaxWords) return fail(SR_ERR_BAD_ARG, "max_words must be 1..16");
    const Scratch p = gram_plan(g, max_words);
    uint32_t launches = 2;
    for (uint32_t l = 1; l <= max_words; l++) {
        const GramLevel lv = gram_level_of(g, l, max_words);
        if (items_per_level) items_per_level[l - 1] = lv.n_items;
        if (lv.n_items) launches += 3;
    }
    out[0] = (uint32_t)std::min<size_t>(p.row_bytes, 0xFFFFFFFFu);
    out[1] = p.rows;
    out[2] = launches;
    out[3] = g->n_sets;
    return SR_OK;
}

int sr_decode_grammar_dp_dev(sr_engine *h, const sr_grammar *g, const int16_t *d_mfcc, const uint32_t *d_in_frames,
                             uint32_t frames_stride, uint32_t n_rows, uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost,
                             uint32_t word_cost, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_level_cost, void *stream)
{
    int rc = check_chain_stage(h, d_mfcc, d_in_frames, frames_stride, n_rows, max_words, n_words_exact, skip_cost, word_cost, d_rec, d_words,
                               d_level_cost);
    if (rc || (rc = check_grammar(h, g)) || !n_rows) return rc;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    const Scratch p = gram_plan(g, max_words);
    const uint32_t per = std::min(p.rows, n_rows);
    if ((rc = order_after_scratch_users(h, s))) return rc;  // the keys, prefix costs and charges are the engine's
    if ((rc = h->s_ch_a.reserve(per * p.a_row)) || (rc = h->s_ch_e.reserve(per * (p.e_row + p.c_row)))) return rc;
    const WordTab wt = word_tab(h);
    GramArgs a{};
    a.n_states = g->n_states;
    a.n_sets = g->n_sets;
    a.n_items = g->n_items;
    a.masks = g->blob.p;
    a.items = (const GramItem *)(g->blob.p + g->items_at);
    a.lists = (const uint32_t *)(g->blob.p + g->lists_at);
    a.final_state = (const uint8_t *)(g->blob.p + g->final_at);
    a.C = h->s_ch_e.p + per * p.e_row;  // behind the prefix costs of the largest group
    for (uint32_t l = 1; l <= max_words; l++) a.lv[l - 1] = gram_level_of(g, l, max_words);
    const GramCosts w = g->costs();
    for (uint32_t r0 = 0; r0 < n_rows; r0 += per) {  // the groups follow each other on s: one scratch serves them all
        a.c = ChainArgs{d_mfcc + (size_t)r0 * h->cfg.max_frames * kCoef, d_in_frames + (size_t)r0 * frames_stride, frames_stride,
                        std::min(per, n_rows - r0), h->cfg.max_frames, h->tpl.p, h->tpl_frames.p, h->tpl_valid.p, h->K, h->tpl_stride,
                        g->tpl_len, p.g.chunk_cols, p.g.n_chunks, max_words, n_words_exact, skip_cost, word_cost, h->s_ch_a.p,
                        h->s_ch_e.p, wt.group_of_slot, wt.word_id, d_rec + r0,
                        d_words + (size_t)r0 * max_words, d_level_cost ? d_level_cost + (size_t)r0 * max_words : nullptr};
        launch_gram(a, g->weighted ? &w : nullptr, s);
    }
    HIP_TRY(hipGetLastError());
    return mark_scratch_user(h, s);
}

int sr_decode_grammar_dp(sr_engine *h, const sr_grammar *g, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride,
                         uint32_t n_rows, uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost,
                         sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost)
{
    int rc = check_chain_stage(h, mfcc, in_frames, frames_stride, n_rows, max_words, n_words_exact, skip_cost, word_cost, rec, words, level_cost);
    if (rc || (rc = check_grammar(h, g)) || !n_rows) return rc;
    return decode_rows_host(h, mfcc, in_frames, frames_stride, n_rows, max_words, rec, words, level_cost,
                            [&](const int16_t *d_mfcc, const uint32_t *d_frames, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_lc) {
                                return sr_decode_grammar_dp_dev(h, g, d_mfcc, d_frames, 1, n_rows, max_words, n_words_exact, skip_cost, word_cost, d_rec,
                                                                d_words, d_lc, nullptr);
                            });
}

}  // extern "C"
