// Live grammar-constrained decoding (include/sr_engine.h, "live grammar-constrained decoding"): sr_decode_live.cpp under a
// grammar.  Feature frames or samples arrive in pushes; per (channel, level, kept item) the boundary column and per channel
// the A / E history of every grammar state stay on the device between calls (k_gram_live.hip).  OPT-IN EXTENSION, NO
// REFERENCE COUNTERPART.
//
// The host knows every count (the decoder's mirror, sr_decode_live_plan.h) and every column offset (sr_gram_live_plan.h):
// nothing is read back to size or to label an output.  Refusals come in the order plan, inputs, outputs, device; the session
// core, the checks, the push sequence and the sequence of an end call are every live session's (sr_live_host.h).
#include "sr_live_host.h"
#include "sr_gram_live_plan.h"

using namespace sr;

struct sr_gram_live : LiveCore {
    const sr_grammar *g = nullptr;        // the grammar of the current dialogue state (sr_gram_live_set_grammar switches it)
    DecodeLiveMirror m;                   // bound to kGramLiveBound throughout: the grammar carries the store and the word map
    uint32_t max_words = 0, n_words_exact = 0, skip_cost = 0, word_cost = 0;
    // what g keeps per level of max_words, and where each level's columns start
    GramLevel lv[kChainMaxWords] = {};
    GramLiveLayout lay;
    uint32_t tpl_len = 0;
    DevBuf<ulonglong2> cols;              // [C][columns][tpl_len]
    DevBuf<unsigned long long> A;         // [C][max_words][S][utt_frames + 1]
    DevBuf<uint32_t> E;                   // [C][max_words + 1][S][utt_frames + 1]
};

namespace {

int check_store(const sr_gram_live *l) { return check_chain(l->h, l->max_words, l->n_words_exact, l->skip_cost, l->word_cost); }  // sr_gram_live_set_grammar

bool stale(const sr_gram_live *l, std::string *why)
{
    return gram_live_stale(l->g->store_serial, l->g->word_serial, l->h->store_serial, l->h->word_serial, why);
}

// room for `count` elements behind `cur`: a NEW buffer in `fresh` when cur is too small, cur itself untouched (DevBuf::reserve
// would free it first)
template <typename T>
int grow_aside(const DevBuf<T> &cur, DevBuf<T> &fresh, size_t count)
{
    return count > cur.n ? fresh.reserve(count) : SR_OK;
}
template <typename T>
void take(DevBuf<T> &cur, DevBuf<T> &fresh)
{
    if (!fresh.p) return;
    std::swap(cur, fresh);
    fresh.release();  // the old buffer: nothing of the session is in flight (a fresh session, or sr_gram_live_set_grammar has waited)
}

// The columns and the history laid out for g, then g adopted.  Whatever has to grow is allocated ASIDE, and the session's
// buffers, layout and grammar change only after the last allocation has succeeded: a failed allocation frees what was
// allocated aside and leaves the session exactly as it was, on its old grammar.
int adopt(sr_gram_live *l, const sr_grammar *g)
{
    GramLevel lv[kChainMaxWords] = {};
    uint32_t items[kChainMaxWords] = {};
    for (uint32_t i = 1; i <= l->max_words; i++) {
        lv[i - 1] = gram_level_of(g, i, l->max_words);
        items[i - 1] = lv[i - 1].n_items;
    }
    const GramLiveLayout lay = gram_live_layout(items, l->max_words);
    const size_t C = l->m.C, P = (size_t)l->m.utt_frames + 1, S = g->n_states;
    TmpDevBuf<ulonglong2> cols;
    TmpDevBuf<unsigned long long> A;
    TmpDevBuf<uint32_t> E;
    if (int rc = grow_aside(l->cols, cols, C * lay.columns * g->tpl_len)) return rc;
    if (int rc = grow_aside(l->A, A, C * l->max_words * S * P)) return rc;
    if (int rc = grow_aside(l->E, E, C * (l->max_words + 1u) * S * P)) return rc;
    take<ulonglong2>(l->cols, cols);
    take<unsigned long long>(l->A, A);
    take<uint32_t>(l->E, E);
    std::copy(lv, lv + kChainMaxWords, l->lv);
    l->lay = lay;
    l->tpl_len = g->tpl_len;
    l->g = g;
    return SR_OK;
}

// a push is refused for a stale grammar first, then for its counts
int plan_push(const sr_gram_live *l, const uint32_t *n, uint32_t n_all, DecodeLivePlan *pl)
{
    std::string why;
    if (stale(l, &why)) return fail(SR_ERR_BAD_ARG, why);
    if (!decode_live_plan(l->m, kGramLiveBound, n, n_all, pl, &why)) return fail(SR_ERR_BAD_ARG, why);
    return SR_OK;
}

// store: the trace will read the store's frame counts and the word map (not so for a dropped recording)
int check_out(const sr_gram_live *l, uint32_t n_out, uint32_t max_rows, const sr_chain_rec *rec, const sr_chain_word *words,
              const uint32_t *level_cost, const sr_chain_live_row *rows, bool store = true)
{
    return check_outputs(l->max_words, n_out, max_rows, rec, words, level_cost, rows, [&] { return store ? check_store(l) : SR_OK; });
}

GramLiveArgs live_args(const sr_gram_live *l, const int16_t *d_mfcc, uint64_t row_stride, sr_chain_rec *d_rec, sr_chain_word *d_words,
                       uint32_t *d_level_cost)
{
    const sr_engine *h = l->h;
    const sr_grammar *g = l->g;
    const WordTab wt = word_tab(h);
    GramLiveArgs a{};
    a.c = ChainLiveArgs{d_mfcc, row_stride, l->d_chan.p, l->C, h->tpl.p, h->tpl_frames.p, h->tpl_valid.p, h->K, h->tpl_stride, l->tpl_len,
                        l->m.utt_frames + 1u, l->max_words, l->n_words_exact, l->skip_cost, l->word_cost, l->cols.p, l->A.p, l->E.p,
                        wt.group_of_slot, wt.word_id, d_rec, d_words,
                        d_level_cost};  // (no grouping: only a dropped recording is traced then, which reads neither)
    a.n_states = g->n_states;
    a.n_items = g->n_items;
    a.columns = l->lay.columns;
    a.masks = g->blob.p;
    a.items = (const GramItem *)(g->blob.p + g->items_at);
    a.lists = (const uint32_t *)(g->blob.p + g->lists_at);
    a.final_state = (const uint8_t *)(g->blob.p + g->final_at);
    std::copy(l->lv, l->lv + kChainMaxWords, a.lv);
    std::copy(l->lay.col_off, l->lay.col_off + kChainMaxWords, a.col_off);
    return a;
}

// the levels over the new frames of every channel and the trace of every emitting one, enqueued on s
int launch_push(sr_gram_live *l, const DecodeLivePlan &pl, const int16_t *d_mfcc, uint64_t row_stride, sr_chain_rec *d_rec,
                sr_chain_word *d_words, uint32_t *d_level_cost, hipStream_t s)
{
    const GramLiveArgs a = live_args(l, d_mfcc, row_stride, d_rec, d_words, d_level_cost);
    const GramCosts w = l->g->costs();
    if (pl.max_frames) launch_gram_live(a, l->g->weighted ? &w : nullptr, s);
    else launch_gram_live_trace(a, l->g->weighted ? &w : nullptr, s);  // (PCM) samples, but no new frame: the parse so far again
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

// the four push forms: a push enqueues work when a channel emits a row
int push(sr_gram_live *l, const LiveIn &in, bool device, void *stream, const uint32_t *n, uint32_t n_all, uint32_t max_rows, sr_chain_rec *rec,
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

int sr_gram_live_geometry(const sr_grammar *g, uint32_t max_words, uint32_t utt_frames, uint32_t chunk_max, uint32_t out[4])
{
    if (!g || !out || max_words < 1 || max_words > kChainMaxWords || !utt_frames || utt_frames > kLiveMaxFrames || !chunk_max ||
        chunk_max > utt_frames)
        return fail(SR_ERR_BAD_ARG, "null / zero argument, or one outside its range");
    uint32_t items[kChainMaxWords] = {};
    for (uint32_t l = 1; l <= max_words; l++) items[l - 1] = gram_level_of(g, l, max_words).n_items;
    const GramLiveLayout lay = gram_live_layout(items, max_words);
    const LdsBudget mi355x;  // no device: MI355X's figures
    out[0] = gram_live_state_bytes(lay.columns, g->tpl_len, g->n_states, max_words, utt_frames);
    out[1] = spot_max_tpl(mi355x);
    out[2] = lay.launches();
    out[3] = lay.columns;
    return SR_OK;
}

int sr_gram_live_open(sr_engine *h, const sr_grammar *g, uint32_t n_channels, uint32_t chunk_max, uint32_t utt_frames, uint32_t max_words,
                      uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost, const uint32_t *mid, sr_gram_live **out)
{
    if (!h || !out) return fail(SR_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (int rc = check_chain(h, max_words, n_words_exact, skip_cost, word_cost)) return rc;
    if (int rc = check_grammar(h, g)) return rc;
    if (!n_channels || n_channels > kLiveMaxChannels || !utt_frames || utt_frames > kLiveMaxFrames)
        return fail(SR_ERR_BAD_ARG, "n_channels not in 1..65535 / utt_frames not in 1..16383");
    if (int rc = LiveCore::check_open(h, n_channels, chunk_max, mid ? std::min(h->cfg.max_frames, utt_frames) : utt_frames, mid)) return rc;
    ENTER_DEVICE(h);
    sr_gram_live *l = new sr_gram_live();
    l->m.open(n_channels, kGramLiveBound);
    l->m.chunk_max = chunk_max;
    l->m.utt_frames = utt_frames;
    l->m.pcm = mid != nullptr;
    l->m.frame_len = h->frame_len;
    l->m.hop = h->hop;
    l->max_words = max_words;
    l->n_words_exact = n_words_exact;
    l->skip_cost = skip_cost;
    l->word_cost = word_cost;
    int rc = l->open_common(h, n_channels, chunk_max, mid);
    if (!rc) rc = adopt(l, g);
    if (rc) {
        (void)hipGetLastError();
        sr_gram_live_close(l);
        return rc;
    }
    *out = l;
    return SR_OK;
}

void sr_gram_live_close(sr_gram_live *l)
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

int sr_gram_live_set_grammar(sr_gram_live *l, const sr_grammar *g)
{
    if (!l) return fail(SR_ERR_BAD_ARG, "null session");
    if (int rc = check_grammar(l->h, g)) return rc;
    if (int rc = check_store(l)) return rc;  // the store g was compiled against must fit the sweep's LDS image as well
    std::string why;
    if (!gram_live_all_empty(l->m, &why)) return fail(SR_ERR_BAD_ARG, why);
    ENTER_DEVICE(l->h);
    if (int rc = l->wait_last()) return rc;  // nothing of an empty session is in flight but a trace, which reads the old grammar's lists
    return adopt(l, g);
}

int sr_gram_live_push_dev(sr_gram_live *l, const int16_t *d_mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                          sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_level_cost, sr_chain_live_row *rows, uint32_t *n_rows,
                          void *stream)
{
    return push(l, LiveIn{d_mfcc, row_stride, false}, true, stream, n, n_all, max_rows, d_rec, d_words, d_level_cost, rows, n_rows);
}

int sr_gram_live_push(sr_gram_live *l, const int16_t *mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                      sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost, sr_chain_live_row *rows, uint32_t *n_rows)
{
    return push(l, LiveIn{mfcc, row_stride, false}, false, nullptr, n, n_all, max_rows, rec, words, level_cost, rows, n_rows);
}

int sr_gram_live_push_pcm_dev(sr_gram_live *l, const uint16_t *d_pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                              sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_level_cost, sr_chain_live_row *rows, uint32_t *n_rows,
                              void *stream)
{
    return push(l, LiveIn{d_pcm, pcm_stride, true}, true, stream, n, n_all, max_rows, d_rec, d_words, d_level_cost, rows, n_rows);
}

int sr_gram_live_push_pcm(sr_gram_live *l, const uint16_t *pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                          sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost, sr_chain_live_row *rows, uint32_t *n_rows)
{
    return push(l, LiveIn{pcm, pcm_stride, true}, false, nullptr, n, n_all, max_rows, rec, words, level_cost, rows, n_rows);
}

int sr_gram_live_end(sr_gram_live *l, const uint32_t *channels, uint32_t n_ch, sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost,
                     sr_chain_live_row *rows, uint32_t *n_rows)
{
    if (!l || (n_ch && !channels)) return fail(SR_ERR_BAD_ARG, "null argument");
    std::vector<SpotLiveChan> chan;
    std::vector<sr_chain_live_row> order;
    std::string why;
    // Under a stale grammar the history belongs to a store or a word map that is gone: every listed recording is dropped.  Its
    // trace has N = 0 and reads neither the store nor the word map, so whatever state those are in, the channels can be ended.
    const bool dropped = stale(l, &why);
    if (!decode_live_end_list(l->m, dropped ? kGramLiveStale : kGramLiveBound, channels, n_ch, &chan, &order, &why)) return fail(SR_ERR_BAD_ARG, why);
    const uint32_t n_out = (uint32_t)order.size();
    if (int rc = check_out(l, n_out, n_out, rec, words, level_cost, rows, !dropped)) return rc;
    if (int rc = check_end_rows(l->max_words, n_out, rec, words, level_cost, rows)) return rc;
    const GramCosts w = l->g->costs();
    return live_end(
        *l, chan, order, l->max_words, rec, words, level_cost, rows, n_rows, [] { return SR_OK; },
        [&](sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_lc) {
            launch_gram_live_trace(live_args(l, nullptr, 0, d_rec, d_words, d_lc), l->g->weighted ? &w : nullptr, nullptr);
        },
        [&] { decode_live_reset(l->m, kGramLiveBound, order); });
}

}  // extern "C"
