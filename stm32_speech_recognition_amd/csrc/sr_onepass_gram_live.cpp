// Live one-pass grammar decoding (include/sr_engine.h, "live one-pass grammar decoding"): sr_onepass_live.cpp under a grammar.
// Feature frames or samples arrive in pushes; per channel the one-pass grammar decoder's A / E history of every state, one
// saved column per kept item and the feature row stay on the device between calls (k_onepass_gram_live.hip).  OPT-IN
// EXTENSION, NO REFERENCE COUNTERPART.
//
// The host knows every count: each channel's frames so far and the first frame of its last block (the live one-pass decoder's
// mirror, sr_onepass_live_plan.h), bound to a constant as the grammar sessions bind theirs (sr_gram_live_plan.h) -- the grammar
// carries the store and the word map.  Nothing is read back to size or to label an output.  Refusals come in the order stale
// grammar, counts, inputs, outputs, device; the session core, the checks, the push sequence and the sequence of an end call
// are every live session's (sr_live_host.h).  A push never synchronises; open, sr_onepass_gram_live_set_grammar and the end
// call may: they establish and restore what lets a push run without an init launch (k_onepass_gram_live_wipe).
#include "sr_live_host.h"
#include "sr_onepass_gram_commit_plan.h"
#include "sr_onepass_gram_live_plan.h"

using namespace sr;

struct sr_onepass_gram_live : LiveCore {
    const sr_grammar *g = nullptr;        // the grammar of the current dialogue state (sr_onepass_gram_live_set_grammar switches it)
    OnePassLiveMirror om;                 // bound to kGramLiveBound throughout
    uint32_t words_cap = 0;               // the word rows of an output row; no count is given
    uint32_t tail = 0, skip_cost = 0, word_cost = 0;
    // the layout of the state, fixed when g was adopted: the states of the dense history, what the decoder keeps of g (the
    // grammar's static lists, or everything under the hook "onepass_gram_prune_off" as read then) and the rows of a column
    uint32_t S = 0, kept_items = 0, kept_states = 0, tpl_len = 0;
    bool pruned = true;
    DevBuf<ulonglong2> cols;              // [C][kept items][tpl_len]
    DevBuf<unsigned long long> A;         // [C][S][utt_frames + 1]
    DevBuf<uint32_t> E;                   // [C][S][utt_frames + 1]
    DevBuf<int16_t> hist;                 // [C][utt_frames][12]: the channels' feature rows
    // sr_onepass_gram_live_commit: per channel {words delivered, the last delivered word's node}, the rows of the call in
    // flight, and the window of the rule under g (from its kept items, whatever the pruning hook says)
    DevBuf<uint2> cursor;                 // [C]
    DevBuf<sr_chain_live_row> commit_rows;  // [C]
    uint32_t commit_W = 0, commit_ring = 64, commit_block = 1;
};

namespace {

uint32_t block_hook()
{
    const int64_t v = dev_hook(kHookOnePassBlock);  // testing build: short blocks put seams into small test shapes
    return v > 0 ? (uint32_t)std::min<int64_t>(v, 16383) : 0u;
}

struct Kept {
    uint32_t items, states;
    bool pruned;
};
Kept kept_of(const sr_grammar *g)  // testing build: the hook keeps every item and every state
{
    if (dev_hook(kHookOnePassGramPruneOff)) return Kept{g->n_items, g->n_states, false};
    return Kept{g->op_n_items, g->op_n_states, true};
}

uint32_t reach_of(const sr_engine *h) { return onepass_reach(h->tpl_len_host.data(), h->K); }

// the decoder's conditions on the engine, the store and the costs
int check_store(const sr_onepass_gram_live *l) { return check_chain(l->h, 1, 0, l->skip_cost, l->word_cost); }

// the cost bound of a session of utt_frames under g (g is fresh: the engine's store is the one it was compiled against)
int check_bound(const sr_engine *h, const sr_grammar *g, uint32_t utt_frames, uint32_t word_cost)
{
    if (!onepass_gram_cost_ok(utt_frames, reach_of(h), word_cost, g->max_arc_cost, g->max_final_cost))
        return fail(SR_ERR_BAD_ARG, "(utt_frames / L) * (word_cost + the grammar's largest arc cost) + its largest final cost must be at most 2^30, "
                                    "L = the shortest valid template's frames / 2 + 1");
    return SR_OK;
}

bool stale(const sr_onepass_gram_live *l, std::string *why)
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
    fresh.release();  // the old buffer: nothing of the session is in flight (a fresh session, or set_grammar has waited)
}

OnePassGramLiveArgs live_args(const sr_onepass_gram_live *l, const int16_t *d_mfcc, uint64_t row_stride, uint32_t block, sr_chain_rec *d_rec,
                              sr_chain_word *d_words)
{
    const sr_engine *h = l->h;
    const sr_grammar *g = l->g;
    const WordTab wt = word_tab(h);
    OnePassGramLiveArgs a{};
    a.o = OnePassLiveArgs{d_mfcc, row_stride, l->d_chan.p, l->C, h->tpl.p, h->tpl_frames.p, h->tpl_valid.p, h->K, h->tpl_stride, l->tpl_len,
                          l->om.d.utt_frames + 1u, block, l->words_cap, l->tail, l->skip_cost, l->word_cost, l->cols.p, l->A.p, l->E.p, l->hist.p,
                          wt.group_of_slot, wt.word_id, d_rec,
                          d_words};  // (no grouping: only a dropped recording is traced then, which reads neither)
    a.n_states = l->S;
    a.n_items = g->n_items;
    a.n_keep_items = l->kept_items;
    a.n_keep_states = l->kept_states;
    a.masks = g->blob.p;
    a.items = (const GramItem *)(g->blob.p + g->items_at);
    a.final_state = (const uint8_t *)(g->blob.p + g->final_at);
    a.keep_items = l->pruned ? (const uint32_t *)(g->blob.p + g->op_items_at) : nullptr;
    a.keep_states = l->pruned ? (const uint32_t *)(g->blob.p + g->op_states_at) : nullptr;
    return a;
}

// The state laid out for g, then g adopted, then the invariants of an empty session put in place under the new layout.
// Whatever has to grow is allocated ASIDE, and the session's buffers, layout and grammar change only after the last
// allocation has succeeded: a failed allocation frees what was allocated aside and leaves the session exactly as it was, on
// its old grammar.  Every channel is empty, so nothing of value is in the buffers: the wipe covers every position of every
// state of the new layout, on old data and on fresh memory alike.  On the null stream, and waited for.
int adopt(sr_onepass_gram_live *l, const sr_grammar *g)
{
    const Kept k = kept_of(g);
    const size_t C = l->om.d.C, P = (size_t)l->om.d.utt_frames + 1, S = g->n_states;
    TmpDevBuf<ulonglong2> cols;
    TmpDevBuf<unsigned long long> A;
    TmpDevBuf<uint32_t> E;
    if (int rc = grow_aside(l->cols, cols, C * k.items * g->tpl_len)) return rc;
    if (int rc = grow_aside(l->A, A, C * S * P)) return rc;
    if (int rc = grow_aside(l->E, E, C * S * P)) return rc;
    take<ulonglong2>(l->cols, cols);
    take<unsigned long long>(l->A, A);
    take<uint32_t>(l->E, E);
    l->S = g->n_states;
    l->kept_items = k.items;
    l->kept_states = k.states;
    l->pruned = k.pruned;
    l->tpl_len = g->tpl_len;
    l->g = g;
    l->commit_W = onepass_gram_commit_window(g->op_item_slots.data(), (uint32_t)g->op_item_slots.size(), l->h->tpl_len_host.data(), l->h->K);
    l->commit_ring = onepass_gram_commit_ring(l->commit_W);
    l->commit_block = onepass_gram_commit_block(reach_of(l->h));
    std::vector<SpotLiveChan> all(l->C, SpotLiveChan{});
    for (SpotLiveChan &ch : all) {
        ch.first_win = 1u;
        ch.aux = l->om.d.utt_frames;
    }
    if (int rc = l->upload_chan(all, nullptr)) return rc;
    launch_onepass_gram_live_wipe(live_args(l, nullptr, 0, 1u, nullptr, nullptr), nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(l->cursor.p, 0, C * sizeof(uint2), nullptr));  // no channel has delivered a word
    HIP_TRY(hipStreamSynchronize(nullptr));
    return SR_OK;
}

// a push is refused for a stale grammar first, then for its counts
int plan_push(const sr_onepass_gram_live *l, const uint32_t *n, uint32_t n_all, OnePassLivePlan *pl)
{
    std::string why;
    if (stale(l, &why)) return fail(SR_ERR_BAD_ARG, why);
    if (!onepass_gram_live_plan(l->om, reach_of(l->h), block_hook(), n, n_all, pl, &why)) return fail(SR_ERR_BAD_ARG, why);
    return SR_OK;
}

// store: the trace will read the store's frame counts and the word map (not so for a dropped recording)
int check_out(const sr_onepass_gram_live *l, uint32_t n_out, uint32_t max_rows, const sr_chain_rec *rec, const sr_chain_word *words,
              const sr_chain_live_row *rows, bool store = true)
{
    return check_outputs(l->words_cap, n_out, max_rows, rec, words, nullptr, rows, [&] { return store ? check_store(l) : SR_OK; });
}

// the blocks over the new frames of every channel and the trace of every emitting one, enqueued on s (PCM: samples, but no
// new frame, is no block: the parse so far again)
int launch_push(sr_onepass_gram_live *l, const OnePassLivePlan &pl, const int16_t *d_mfcc, uint64_t row_stride, sr_chain_rec *d_rec,
                sr_chain_word *d_words, hipStream_t s)
{
    const GramCosts w = l->g->costs();
    launch_onepass_gram_live(live_args(l, d_mfcc, row_stride, pl.block, d_rec, d_words), l->g->weighted ? &w : nullptr, pl.n_blocks, s);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

// the four push forms: a push enqueues work when a channel emits a row
int push(sr_onepass_gram_live *l, const LiveIn &in, bool device, void *stream, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
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

// a commit call up to its launch: the stale grammar first, then the rows of the distinct listed channels from the mirror, then
// the checks -- nothing is enqueued, written or changed before all of them pass.  host: rows is a host buffer like crec and
// cwords (the host form)
int plan_commit(const sr_onepass_gram_live *l, const uint32_t *channels, uint32_t n_ch, const sr_commit_rec *crec, const sr_chain_word *cwords,
                const sr_chain_live_row *rows, bool host, std::vector<sr_chain_live_row> *order)
{
    if (!l) return fail(SR_ERR_BAD_ARG, "null session");
    std::string why_stale, why;
    const bool is_stale = stale(l, &why_stale);
    if (!is_stale && n_ch && !channels) return fail(SR_ERR_BAD_ARG, "null argument");
    if (!onepass_gram_commit_list(l->om, is_stale, why_stale, channels, n_ch, order, &why)) return fail(SR_ERR_BAD_ARG, why);
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
int enqueue_commit(sr_onepass_gram_live *l, const std::vector<sr_chain_live_row> &order, sr_commit_rec *d_crec, sr_chain_word *d_cwords,
                   hipStream_t s)
{
    const sr_grammar *g = l->g;
    if (int rc = l->order_after_last_push(s)) return rc;
    // (a pageable source is staged before the call returns: the list may go out of scope)
    HIP_TRY(hipMemcpyAsync(l->commit_rows.p, order.data(), order.size() * sizeof(sr_chain_live_row), hipMemcpyHostToDevice, s));
    const GramCosts w = g->costs();
    launch_onepass_gram_live_commit(
        OnePassGramCommitArgs{live_args(l, nullptr, 0, 1u, nullptr, nullptr), l->commit_rows.p, (uint32_t)order.size(), l->commit_W, l->commit_ring, l->commit_block,
                              (const uint32_t *)(g->blob.p + g->op_states_at), g->op_n_states, l->cursor.p, d_crec, d_cwords},
        g->weighted ? &w : nullptr, s);
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

int sr_onepass_gram_live_geometry(const sr_grammar *g, uint32_t utt_frames, uint32_t chunk_max, uint32_t out[6])
{
    if (!g || !out || !utt_frames || utt_frames > kLiveMaxFrames || !chunk_max || chunk_max > utt_frames)
        return fail(SR_ERR_BAD_ARG, "null / zero argument, or one outside its range");
    const Kept k = kept_of(g);
    const LdsBudget mi355x;  // no device: MI355X's figures
    const uint32_t L = reach_of(g->h);
    out[0] = onepass_gram_live_state_bytes(g->n_states, k.items, g->tpl_len, utt_frames);
    out[1] = spot_max_tpl(mi355x);
    out[2] = L;
    out[3] = onepass_gram_live_launches(chunk_max, onepass_live_block(L, block_hook(), chunk_max), k.items, k.states);
    out[4] = k.items;
    out[5] = k.states;
    return SR_OK;
}

int sr_onepass_gram_live_open(sr_engine *h, const sr_grammar *g, uint32_t n_channels, uint32_t chunk_max, uint32_t utt_frames, uint32_t words_cap,
                              uint32_t flags, uint32_t skip_cost, uint32_t word_cost, const uint32_t *mid, sr_onepass_gram_live **out)
{
    if (!h || !out) return fail(SR_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (int rc = check_chain(h, 1, 0, skip_cost, word_cost)) return rc;
    if (int rc = check_grammar(h, g)) return rc;
    if (!words_cap) return fail(SR_ERR_BAD_ARG, "words_cap must be at least 1");
    if (flags & ~SR_OP_LIVE_TAIL) return fail(SR_ERR_BAD_ARG, "unknown flag");
    if (!n_channels || n_channels > kLiveMaxChannels || !utt_frames || utt_frames > kLiveMaxFrames)
        return fail(SR_ERR_BAD_ARG, "n_channels not in 1..65535 / utt_frames not in 1..16383");
    if (int rc = check_bound(h, g, utt_frames, word_cost)) return rc;
    if (int rc = LiveCore::check_open(h, n_channels, chunk_max, mid ? std::min(h->cfg.max_frames, utt_frames) : utt_frames, mid)) return rc;
    ENTER_DEVICE(h);
    sr_onepass_gram_live *l = new sr_onepass_gram_live();
    l->g = g;
    l->om.open(n_channels, kGramLiveBound);
    l->om.d.chunk_max = chunk_max;
    l->om.d.utt_frames = utt_frames;
    l->om.d.pcm = mid != nullptr;
    l->om.d.frame_len = h->frame_len;
    l->om.d.hop = h->hop;
    l->words_cap = words_cap;
    l->tail = flags & SR_OP_LIVE_TAIL;
    l->skip_cost = skip_cost;
    l->word_cost = word_cost;
    int rc = l->open_common(h, n_channels, chunk_max, mid);
    if (!rc) rc = l->hist.reserve((size_t)n_channels * utt_frames * kCoef);
    if (!rc) rc = l->cursor.reserve(n_channels);
    if (!rc) rc = l->commit_rows.reserve(n_channels);
    if (!rc) rc = adopt(l, g);
    if (rc) {
        (void)hipGetLastError();
        sr_onepass_gram_live_close(l);
        return rc;
    }
    *out = l;
    return SR_OK;
}

void sr_onepass_gram_live_close(sr_onepass_gram_live *l)
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

int sr_onepass_gram_live_set_grammar(sr_onepass_gram_live *l, const sr_grammar *g)
{
    if (!l) return fail(SR_ERR_BAD_ARG, "null session");
    if (int rc = check_grammar(l->h, g)) return rc;
    if (int rc = check_store(l)) return rc;  // the store g was compiled against must fit the sweep's LDS image as well
    if (int rc = check_bound(l->h, g, l->om.d.utt_frames, l->word_cost)) return rc;
    std::string why;
    if (!gram_live_all_empty(l->om.d, &why)) return fail(SR_ERR_BAD_ARG, why);
    ENTER_DEVICE(l->h);
    if (int rc = l->wait_last()) return rc;  // nothing of an empty session is in flight but a trace, which reads the old grammar's lists
    return adopt(l, g);
}

int sr_onepass_gram_live_push_dev(sr_onepass_gram_live *l, const int16_t *d_mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all,
                                  uint32_t max_rows, sr_chain_rec *d_rec, sr_chain_word *d_words, sr_chain_live_row *rows, uint32_t *n_rows,
                                  void *stream)
{
    return push(l, LiveIn{d_mfcc, row_stride, false}, true, stream, n, n_all, max_rows, d_rec, d_words, rows, n_rows);
}

int sr_onepass_gram_live_push(sr_onepass_gram_live *l, const int16_t *mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all, uint32_t max_rows,
                              sr_chain_rec *rec, sr_chain_word *words, sr_chain_live_row *rows, uint32_t *n_rows)
{
    return push(l, LiveIn{mfcc, row_stride, false}, false, nullptr, n, n_all, max_rows, rec, words, rows, n_rows);
}

int sr_onepass_gram_live_push_pcm_dev(sr_onepass_gram_live *l, const uint16_t *d_pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                                      uint32_t max_rows, sr_chain_rec *d_rec, sr_chain_word *d_words, sr_chain_live_row *rows, uint32_t *n_rows,
                                      void *stream)
{
    return push(l, LiveIn{d_pcm, pcm_stride, true}, true, stream, n, n_all, max_rows, d_rec, d_words, rows, n_rows);
}

int sr_onepass_gram_live_push_pcm(sr_onepass_gram_live *l, const uint16_t *pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                                  uint32_t max_rows, sr_chain_rec *rec, sr_chain_word *words, sr_chain_live_row *rows, uint32_t *n_rows)
{
    return push(l, LiveIn{pcm, pcm_stride, true}, false, nullptr, n, n_all, max_rows, rec, words, rows, n_rows);
}

int sr_onepass_gram_live_end(sr_onepass_gram_live *l, const uint32_t *channels, uint32_t n_ch, sr_chain_rec *rec, sr_chain_word *words,
                             sr_chain_live_row *rows, uint32_t *n_rows)
{
    if (!l || (n_ch && !channels)) return fail(SR_ERR_BAD_ARG, "null argument");
    std::vector<SpotLiveChan> chan;
    std::vector<sr_chain_live_row> order;
    std::string why;
    // Under a stale grammar the history belongs to a store or a word map that is gone: every listed recording is dropped.  Its
    // trace has N = 0 and reads neither the store nor the word map, so whatever state those are in, the channels can be ended;
    // the wipe runs all the same, over the frames the channel held (aux), in the layout the session still stands in.
    const bool dropped = stale(l, &why);
    if (!onepass_live_end_list(l->om, dropped ? kGramLiveStale : kGramLiveBound, channels, n_ch, &chan, &order, &why))
        return fail(SR_ERR_BAD_ARG, why);
    const uint32_t n_out = (uint32_t)order.size();
    if (int rc = check_out(l, n_out, n_out, rec, words, rows, !dropped)) return rc;
    if (int rc = check_end_rows(l->words_cap, n_out, rec, words, nullptr, rows)) return rc;
    const GramCosts w = l->g->costs();
    return live_end(
        *l, chan, order, l->words_cap, rec, words, nullptr, rows, n_rows, [] { return SR_OK; },
        [&](sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *) {
            launch_onepass_gram_live_end(live_args(l, nullptr, 0, 1u, d_rec, d_words), l->g->weighted ? &w : nullptr, l->cursor.p, nullptr);
        },
        [&] { onepass_live_reset(l->om, kGramLiveBound, order); });
}

int sr_onepass_gram_live_commit_dev(sr_onepass_gram_live *l, const uint32_t *channels, uint32_t n_ch, sr_commit_rec *d_crec,
                                    sr_chain_word *d_cwords, sr_chain_live_row *rows, uint32_t *n_rows, void *stream)
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

int sr_onepass_gram_live_commit(sr_onepass_gram_live *l, const uint32_t *channels, uint32_t n_ch, sr_commit_rec *crec, sr_chain_word *cwords,
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
