// What the host forms of the batch stages (the decoders sr_chain.cpp, sr_gram.cpp, sr_onepass.cpp, sr_onepass_gram.cpp, the
// spotter sr_spot.cpp, sr_span.cpp, sr_align.cpp, sr_cluster.cpp, sr_forced.cpp, sr_rescore.cpp and the whole-path PCM forms of
// sr_host.cpp) do alike: feature rows and their frame counts to the engine's scratch, the per-call device copies of a decoder's
// outputs and their way back, and the front of a whole-path call -- explicit segments of capture rows to feature rows where
// the stage reads them.  Next to them the small things every stage asks of the engine: the longest template, the word table.
// A stage file keeps its checks, its plan and its launch loop; nothing here knows a stage.  The live sessions (sr_live_host.h)
// take the outputs and the helpers from here.  HOST ONLY.
#pragma once
#include "sr_host_call.h"
#include "sr_overlap.h"

namespace sr {

// the longest template of the store: upload_templates keeps one row of slack behind it
static inline uint32_t store_tpl_len(const sr_engine *h) { return h->tpl_rows - 1; }

// the engine's word table (sr_nbest.cpp builds and uploads it), device pointers:
//   order[K] | group_start[n_words + 1] | word_id[n_words] | group_of_slot[K]
// An engine without a table (no store yet) has null pointers.
struct WordTab {
    const uint32_t *order, *group_start, *word_id, *group_of_slot;
};
static inline WordTab word_tab(const sr_engine *h)
{
    const uint32_t *t = h->wg_tab.p;
    if (!t) return WordTab{nullptr, nullptr, nullptr, nullptr};
    return WordTab{t, t + h->K, t + h->K + h->wg_words + 1, t + h->K + 2 * (size_t)h->wg_words + 1};
}

// the feature rows of a host-buffer call into s_mfcc and their frame counts into s_u32a: the counts go up dense, whatever
// records they came in.  A call without rows (a training over no examples) still gets both buffers.
static inline int stage_rows(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows)
{
    if (int rc = h->s_mfcc.reserve(h->mfcc_elems(std::max(n_rows, 1u)))) return rc;
    if (int rc = h->s_u32a.reserve(std::max(n_rows, 1u))) return rc;
    if (!n_rows) return SR_OK;
    std::vector<uint32_t> frames(n_rows);
    for (uint32_t r = 0; r < n_rows; r++) frames[r] = in_frames[(size_t)r * frames_stride];
    COPY_UP(h->s_mfcc.p, mfcc, h->mfcc_elems(n_rows) * 2);
    COPY_UP(h->s_u32a.p, frames.data(), (size_t)n_rows * 4);
    return SR_OK;
}

// ---- the decoders' outputs: a record, max_words word rows and (level decoders) max_words level costs per row ---------------
// host forms: per-call device copies of the outputs of n_out rows (lc only where the caller wants level costs: lc.p is null
// otherwise), and their way back to the caller's buffers
struct HostOutputs {
    const uint32_t n_out, max_words;
    sr_chain_rec *const h_rec;
    sr_chain_word *const h_words;
    uint32_t *const h_lc;
    TmpDevBuf<sr_chain_rec> rec;
    TmpDevBuf<sr_chain_word> words;
    TmpDevBuf<uint32_t> lc;
    HostOutputs(uint32_t n, uint32_t mw, sr_chain_rec *r, sr_chain_word *w, uint32_t *l) : n_out(n), max_words(mw), h_rec(r), h_words(w), h_lc(l) {}
    int reserve()
    {
        const size_t n_w = (size_t)std::max(n_out, 1u) * max_words;
        if (int rc = rec.reserve(std::max(n_out, 1u))) return rc;
        if (int rc = words.reserve(n_w)) return rc;
        return h_lc ? lc.reserve(n_w) : SR_OK;
    }
    int down()
    {
        if (!n_out) return SR_OK;
        const size_t n_w = (size_t)n_out * max_words;
        COPY_DOWN(h_rec, rec.p, (size_t)n_out * sizeof *h_rec);
        COPY_DOWN(h_words, words.p, n_w * sizeof *h_words);
        if (h_lc) COPY_DOWN(h_lc, lc.p, n_w * 4);
        return SR_OK;
    }
};

// A decoder's *_dp host form after its checks (n_rows >= 1), on the null stream: the rows up, stage(d_mfcc, d_frames, d_rec,
// d_words, d_level_cost) -- the public *_dev stage over the staged rows (dense counts) into the copies -- and the copies down.
template <typename Stage>
int decode_rows_host(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows, uint32_t max_words,
                     sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost, Stage &&stage)
{
    ENTER_HOST_CALL(h);
    HostOutputs o(n_rows, max_words, rec, words, level_cost);
    if (int rc = stage_rows(h, mfcc, in_frames, frames_stride, n_rows)) return rc;
    if (int rc = o.reserve()) return rc;
    if (int rc = stage(h->s_mfcc.p, h->s_u32a.p, o.rec.p, o.words.p, o.lc.p)) return rc;
    return o.down();
}

// ---- whole-path PCM forms: explicit segments of capture rows ----------------------------------------------------------------
// Per-item failure, as get_mfcc has it (MFCC.C:102-107: a segment shorter than a frame underflows the u32 frame count,
// which then exceeds vv_frm_max -> frm_num = 0): one bad record yields frm_num[b] = 0, an all-zero MFCC record and
// status[b] != 0; the other records of the batch are processed.
// The per-utterance records the frame kernel consumes (what k_vad would have produced) for explicit segments.
static inline int mfcc_records(const sr_engine *h, uint32_t buf_len, uint32_t B, const int32_t *start, const int32_t *end,
                               const uint32_t *mid, uint32_t *frm_num, uint32_t *status, std::vector<sr_vad_rec> &recs)
{
    recs.resize(B);
    for (uint32_t b = 0; b < B; b++) {
        sr_vad_rec &r = recs[b];
        std::memset(&r, 0, sizeof r);
        // samples and mid are 16-bit quantities in the reference (u16 VcBuf, mid_val = a mean of u16 samples,
        // VAD.C:41-47); the frame kernel's 24-bit multiplies rely on |sample - mid| < 2^23
        if (mid[b] > 0xFFFFu) return fail(SR_ERR_BAD_ARG, "mid exceeds the u16 sample range");
        r.atap.mid_val = mid[b];
        for (int i = 0; i < 2 * SR_MAX_SEG; i++) r.seg[i] = -1;
        r.seg[0] = start[b];
        r.seg[1] = end[b];
        if (start[b] < 1 || end[b] > (int32_t)buf_len || end[b] < start[b]) {
            r.status = SR_ST_SEG_OOB;  // outside the buffer (start >= 1: MFCC.C:119 reads start[-1])
        } else {
            // MFCC.C:102: u32 arithmetic, u16 truncation -- a segment shorter than a frame wraps to a count above the cap
            const uint32_t n = ((((uint32_t)(end[b] - start[b]) - h->frame_len) / h->hop) + 1) & 0xFFFF;
            const bool shorter = (uint32_t)(end[b] - start[b]) < h->frame_len;  // the wrapped count may alias a small one
            r.status = (shorter || n > h->cfg.max_frames) ? SR_ST_MFCC_FAIL : SR_ST_OK;  // MFCC.C:103-107
            r.frm_num = r.status == SR_ST_OK ? n : 0;
        }
        if (r.status != SR_ST_OK) r.seg[0] = 1, r.seg[1] = 1;  // never dereferenced (no frames); keep the record harmless
        if (frm_num) frm_num[b] = r.frm_num;
        if (status) status[b] = r.status;
    }
    return SR_OK;
}

// what the caller of a whole-path PCM form hands in (mfcc, frm_num, status: optional outputs)
struct PcmSegments {
    const uint16_t *pcm;
    uint64_t pcm_stride;
    uint32_t buf_len, B;
    const int32_t *start, *end;
    const uint32_t *mid;
    int16_t *mfcc;
    uint32_t *frm_num, *status;
};

// A whole-path PCM form after its null check and the feature's own check, on the null stream: the records and the frame
// kernel of sr_mfcc_batch_status, then stage(d_mfcc, d_frames, frames_stride) over the feature rows where they are -- frame
// counts straight from the records (a failed one has frm_num 0) -- which also brings the stage's outputs down; the feature
// rows come down last.
template <typename Stage>
int pcm_segments_host(sr_engine *h, const PcmSegments &in, Stage &&stage)
{
    if (in.B == 0) return SR_OK;
    if (in.buf_len > in.pcm_stride) return fail(SR_ERR_BAD_ARG, "buf_len exceeds pcm_stride");
    ENTER_HOST_CALL(h);
    std::vector<sr_vad_rec> recs;
    int rc = mfcc_records(h, in.buf_len, in.B, in.start, in.end, in.mid, in.frm_num, in.status, recs);
    if (rc) return rc;
    const size_t n_mfcc = h->mfcc_elems(in.B);
    if ((rc = h->s_vad.reserve(in.B)) || (rc = h->s_mfcc.reserve(n_mfcc))) return rc;
    uint64_t ds = 0;
    if ((rc = stage_pcm(h, in.pcm, in.pcm_stride, in.buf_len, in.B, &ds))) return rc;
    COPY_UP(h->s_vad.p, recs.data(), (size_t)in.B * sizeof(sr_vad_rec));
    if ((rc = sr_mfcc_batch_dev(h, h->s_pcm.p, ds, in.B, h->s_vad.p, h->s_mfcc.p, nullptr))) return rc;
    if ((rc = stage(h->s_mfcc.p, &h->s_vad.p[0].frm_num, (uint32_t)(sizeof(sr_vad_rec) / 4)))) return rc;
    if (in.mfcc) COPY_DOWN(in.mfcc, h->s_mfcc.p, n_mfcc * 2);
    return SR_OK;
}

// a decoder's whole-path form: the front, stage(d_mfcc, d_frames, frames_stride, d_rec, d_words, d_level_cost) into per-call
// copies of its outputs, the copies down
template <typename Stage>
int pcm_decode_host(sr_engine *h, const PcmSegments &in, uint32_t max_words, sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost,
                    Stage &&stage)
{
    return pcm_segments_host(h, in, [&](const int16_t *d_mfcc, const uint32_t *d_frames, uint32_t frames_stride) -> int {
        HostOutputs o(in.B, max_words, rec, words, level_cost);
        if (int rc = o.reserve()) return rc;
        if (int rc = stage(d_mfcc, d_frames, frames_stride, o.rec.p, o.words.p, o.lc.p)) return rc;
        return o.down();
    });
}

}  // namespace sr
