// Transcript-forced alignment and the span gather (include/sr_engine.h, "forced alignment against a transcript"): the
// checks and the plan (sr_forced_plan.h: item lists, tail, launch groups -- host-only code), the upload of the plan's tables
// and the sequencing.  Per launch group: k_chain_init, per level (k_forced_words over the level's items, k_chain_close),
// k_forced_trace, everything on the caller's stream; the host knows every item and count, nothing is read back.  The host
// forms stage their rows (and the aligner's outputs) through sr_stage_host.h.
#include "sr_forced_plan.h"
#include "sr_stage_host.h"

using namespace sr;

namespace {

// what both alignment forms check; the store under the word map comes back
int check_forced(const sr_engine *h, const void *mfcc, const void *frames, uint32_t frames_stride, uint32_t n_rows, const uint32_t *transcript,
                 const uint32_t *n_words, uint32_t words_per_row, uint32_t skip_cost, uint32_t word_cost, const sr_chain_rec *rec,
                 const sr_chain_word *words, ForcedStore *store)
{
    if (!h || !mfcc || !frames || !rec || !words || !transcript || !n_words) return fail(SR_ERR_BAD_ARG, "null argument");
    if (words_per_row < 1 || words_per_row > kForcedMaxWords) return fail(SR_ERR_BAD_ARG, "words_per_row must be 1..16");
    if (int rc = check_chain(h, words_per_row, 0, skip_cost, word_cost)) return rc;  // the decoder's own conditions
    if (!frames_stride) return fail(SR_ERR_BAD_ARG, "frames_stride must be at least 1");
    if (overlap(rec, (size_t)n_rows * sizeof *rec, words, (size_t)n_rows * words_per_row * sizeof *words))
        return fail(SR_ERR_BAD_ARG, "d_rec and d_words overlap");
    std::vector<uint32_t> label(h->K);
    for (uint32_t k = 0; k < h->K; k++) label[k] = h->word_explicit ? h->word_labels[k] : k / h->word_spw;
    *store = forced_store(label.data(), h->tpl_len_host.data(), h->K);
    std::string why;
    if (!forced_check(*store, transcript, n_words, n_rows, words_per_row, &why)) return fail(SR_ERR_BAD_ARG, why);
    return SR_OK;
}

// the stage on s; every pointer a device pointer except the two host arrays, which passed check_forced
int run_forced(sr_engine *h, const ForcedStore &store, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
               const uint32_t *transcript, const uint32_t *n_words, uint32_t W, uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *d_rec,
               sr_chain_word *d_words, hipStream_t s)
{
    // the decoder's scratch and its rows-per-group rule at max_words = W; testing build: its hooks (and the spotter's chunk hook,
    // whose sweep this is) put seams and small groups into small test shapes
    const int64_t cc = dev_hook(kHookChainChunk), sc = dev_hook(kHookSpotChunk), rows = dev_hook(kHookChainRows);
    const int64_t cols = cc > 0 ? cc : sc;
    const uint32_t tpl_len = store_tpl_len(h);
    const ChainPlan p = chain_plan(tpl_len, h->cfg.max_frames, W, cols > 0 ? (uint32_t)std::min<int64_t>(cols, 16383) : 0u,
                                   rows > 0 ? (uint32_t)std::min<int64_t>(rows, kChainMaxRows) : 0u);
    const uint32_t per = std::min(p.rows, n_rows);
    const ForcedPlan fp = forced_plan(store, transcript, n_words, n_rows, W, per, dev_hook(kHookForcedPruneOff) == 0);
    int rc;
    if ((rc = order_after_scratch_users(h, s))) return rc;  // the keys, the prefix costs and the tables are the engine's
    if ((rc = h->s_ch_a.reserve(per * p.a_row)) || (rc = h->s_ch_e.reserve(per * p.e_row)) || (rc = h->s_fc_tab.reserve(fp.tab.size() + 2)))
        return rc;
    // the items are pairs of words read as uint2: they start at an even word.  (a pageable source is staged before the call returns)
    const size_t items_at = (fp.items_at() + 1) & ~(size_t)1;
    HIP_TRY(hipMemcpyAsync(h->s_fc_tab.p, fp.tab.data(), fp.items_at() * 4, hipMemcpyHostToDevice, s));
    if (fp.n_items)
        HIP_TRY(hipMemcpyAsync(h->s_fc_tab.p + items_at, fp.tab.data() + fp.items_at(), (size_t)fp.n_items * 8, hipMemcpyHostToDevice, s));
    const WordTab wt = word_tab(h);
    for (const ForcedGroup &g : fp.groups) {  // the groups follow each other on s: one scratch serves them all
        ForcedArgs a{};
        a.c = ChainArgs{d_mfcc + (size_t)g.row0 * h->cfg.max_frames * kCoef, d_in_frames + (size_t)g.row0 * frames_stride, frames_stride, g.n_rows,
                        h->cfg.max_frames, h->tpl.p, h->tpl_frames.p, h->tpl_valid.p, h->K, h->tpl_stride, tpl_len, p.g.chunk_cols, p.g.n_chunks, W,
                        0u, skip_cost, word_cost, h->s_ch_a.p, h->s_ch_e.p, wt.group_of_slot, wt.word_id,
                        d_rec + g.row0, d_words + (size_t)g.row0 * W, nullptr};
        a.items = (const uint2 *)(h->s_fc_tab.p + items_at);
        a.tail = h->s_fc_tab.p + (size_t)g.row0 * W;
        a.count = h->s_fc_tab.p + fp.count_at() + g.row0;
        a.row0 = g.row0;
        launch_forced(a, g.item0, g.levels, s);
    }
    HIP_TRY(hipGetLastError());
    return mark_scratch_user(h, s);
}

int check_gather(const sr_engine *h, const void *mfcc, const void *frames, uint32_t frames_stride, uint32_t n_rows, const sr_chain_word *words,
                 uint32_t words_per_row, const uint32_t *dst_of_span, uint32_t n_ex, uint32_t ex_rows, const int16_t *ex, const uint32_t *ex_frames,
                 std::vector<uint32_t> *src_of_ex)
{
    if (!h || !mfcc || !frames || !words || !dst_of_span || !ex || !ex_frames) return fail(SR_ERR_BAD_ARG, "null argument");
    if (h->nc != (uint32_t)kCoef) return fail(SR_ERR_BAD_CONFIG, "the span gather is built for 12-coefficient records");
    if (!frames_stride) return fail(SR_ERR_BAD_ARG, "frames_stride must be at least 1");
    if (words_per_row < 1 || words_per_row > kForcedMaxWords) return fail(SR_ERR_BAD_ARG, "words_per_row must be 1..16");
    if (ex_rows < 1 || ex_rows > SR_ALIGN_MAX_FRAMES) return fail(SR_ERR_BAD_ARG, "ex_rows must be 1..SR_ALIGN_MAX_FRAMES");
    if ((uint64_t)n_rows * words_per_row >= 0xFFFFFFFFull) return fail(SR_ERR_BAD_ARG, "too many spans");
    if (((uintptr_t)mfcc | (uintptr_t)ex) & 3) return fail(SR_ERR_BAD_ARG, "the feature rows and d_ex must be 4-byte aligned");
    if (overlap(ex, (size_t)n_ex * ex_rows * kCoef * 2, ex_frames, (size_t)n_ex * 4)) return fail(SR_ERR_BAD_ARG, "d_ex and d_ex_frames overlap");
    std::string why;
    if (!forced_gather_table(dst_of_span, (size_t)n_rows * words_per_row, n_ex, src_of_ex, &why)) return fail(SR_ERR_BAD_ARG, why);
    return SR_OK;
}

int run_gather(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, const sr_chain_word *d_words,
               uint32_t words_per_row, const std::vector<uint32_t> &src_of_ex, uint32_t ex_rows, int16_t *d_ex, uint32_t *d_ex_frames, hipStream_t s)
{
    const uint32_t n_ex = (uint32_t)src_of_ex.size();
    int rc;
    if ((rc = order_after_scratch_users(h, s)) || (rc = h->s_fc_src.reserve(n_ex))) return rc;  // the table is the engine's
    HIP_TRY(hipMemcpyAsync(h->s_fc_src.p, src_of_ex.data(), (size_t)n_ex * 4, hipMemcpyHostToDevice, s));  // (staged before the call returns)
    launch_gather_spans(GatherArgs{d_mfcc, d_in_frames, frames_stride, h->cfg.max_frames, d_words, words_per_row, h->s_fc_src.p, n_ex, ex_rows, d_ex,
                                   d_ex_frames},
                        s);
    HIP_TRY(hipGetLastError());
    return mark_scratch_user(h, s);
}

}  // namespace

extern "C" {

int sr_align_transcripts_dp_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                                const uint32_t *transcript, const uint32_t *n_words, uint32_t words_per_row, uint32_t skip_cost,
                                uint32_t word_cost, sr_chain_rec *d_rec, sr_chain_word *d_words, void *stream)
{
    ForcedStore store;
    int rc = check_forced(h, d_mfcc, d_in_frames, frames_stride, n_rows, transcript, n_words, words_per_row, skip_cost, word_cost, d_rec, d_words,
                          &store);
    if (rc || !n_rows) return rc;
    ENTER_DEVICE(h);
    return run_forced(h, store, d_mfcc, d_in_frames, frames_stride, n_rows, transcript, n_words, words_per_row, skip_cost, word_cost, d_rec, d_words,
                      (hipStream_t)stream);
}

int sr_align_transcripts_dp(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                            const uint32_t *transcript, const uint32_t *n_words, uint32_t words_per_row, uint32_t skip_cost, uint32_t word_cost,
                            sr_chain_rec *rec, sr_chain_word *words)
{
    ForcedStore store;
    int rc = check_forced(h, mfcc, in_frames, frames_stride, n_rows, transcript, n_words, words_per_row, skip_cost, word_cost, rec, words, &store);
    if (rc || !n_rows) return rc;
    return decode_rows_host(h, mfcc, in_frames, frames_stride, n_rows, words_per_row, rec, words, nullptr,
                            [&](const int16_t *d_mfcc, const uint32_t *d_frames, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *) {
                                return run_forced(h, store, d_mfcc, d_frames, 1, n_rows, transcript, n_words, words_per_row, skip_cost, word_cost, d_rec,
                                                  d_words, nullptr);
                            });
}

int sr_gather_word_spans_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                             const sr_chain_word *d_words, uint32_t words_per_row, const uint32_t *dst_of_span, uint32_t n_ex, uint32_t ex_rows,
                             int16_t *d_ex, uint32_t *d_ex_frames, void *stream)
{
    std::vector<uint32_t> src_of_ex;
    int rc = check_gather(h, d_mfcc, d_in_frames, frames_stride, n_rows, d_words, words_per_row, dst_of_span, n_ex, ex_rows, d_ex, d_ex_frames,
                          &src_of_ex);
    if (rc || !n_ex) return rc;
    ENTER_DEVICE(h);
    return run_gather(h, d_mfcc, d_in_frames, frames_stride, d_words, words_per_row, src_of_ex, ex_rows, d_ex, d_ex_frames, (hipStream_t)stream);
}

int sr_gather_word_spans(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                         const sr_chain_word *words, uint32_t words_per_row, const uint32_t *dst_of_span, uint32_t n_ex, uint32_t ex_rows,
                         int16_t *ex, uint32_t *ex_frames)
{
    std::vector<uint32_t> src_of_ex;
    int rc = check_gather(h, mfcc, in_frames, frames_stride, n_rows, words, words_per_row, dst_of_span, n_ex, ex_rows, ex, ex_frames, &src_of_ex);
    if (rc || !n_ex) return rc;
    ENTER_HOST_CALL(h);
    const size_t n_w = (size_t)n_rows * words_per_row, n_out = (size_t)n_ex * ex_rows * kCoef;
    TmpDevBuf<sr_chain_word> d_words;
    TmpDevBuf<int16_t> d_ex;
    TmpDevBuf<uint32_t> d_ef;
    if ((rc = stage_rows(h, mfcc, in_frames, frames_stride, n_rows)) || (rc = d_words.reserve(std::max<size_t>(n_w, 1))) || (rc = d_ex.reserve(n_out)) ||
        (rc = d_ef.reserve(n_ex)))
        return rc;
    if (n_w) COPY_UP(d_words.p, words, n_w * sizeof *words);
    if ((rc = run_gather(h, h->s_mfcc.p, h->s_u32a.p, 1, d_words.p, words_per_row, src_of_ex, ex_rows, d_ex.p, d_ef.p, nullptr))) return rc;
    COPY_DOWN(ex, d_ex.p, n_out * 2);
    COPY_DOWN(ex_frames, d_ef.p, (size_t)n_ex * 4);
    return SR_OK;
}

}  // extern "C"
