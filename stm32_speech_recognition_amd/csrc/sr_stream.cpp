// Stream recognition (include/sr_engine.h, "Stream recognition"): every segment of recordings of any length -- the stream VAD
// of k_vad_stream.hip (three launches), then each segment recognised by the frame kernel, DTW and the slot scan exactly as
// segment 0 of sr_recognize_batch_dev.  EXTENSION, NO REFERENCE COUNTERPART (the firmware stops at 3 segments, VAD.C:203).
#include "sr_host_call.h"

using namespace sr;

namespace {

uint32_t stream_tile_frames()
{
    const int64_t v = dev_hook(kHookStreamTile);  // testing build: small tiles put every boundary case on a tile edge
    if (v >= 16 && v <= (int64_t)kStreamTileMax && v % 16 == 0) return (uint32_t)v;
    return kStreamTileDefault;
}

int check_stream(const sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                 uint32_t max_segs, const sr_stream_seg *segs, const uint32_t *seg_offsets)
{
    if (!h || !seg_offsets || (max_segs && !segs)) return fail(SR_ERR_BAD_ARG, "null argument");
    if (int rc = check_pcm(h, pcm, pcm_stride, buf_len)) return rc;
    if (B && (uint64_t)(B - 1) * pcm_stride + buf_len > (1ull << 62)) return fail(SR_ERR_BAD_ARG, "recordings too large");
    return SR_OK;
}

// the three segmentation launches on `s`; d_pcm etc. as sr_stream_segments_dev
int stream_segment(sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t buf_len, const uint32_t *d_len, uint32_t B,
                   const sr_atap *d_atap_in, uint32_t max_segs, sr_stream_seg *d_segs, uint32_t *d_off, sr_atap *d_atap,
                   hipStream_t s)
{
    int rc;
    VadStreamArgs a{};
    if (d_atap_in) {
        a.atap_src = (const uint8_t *)d_atap_in;
        a.atap_src_stride = sizeof(sr_atap);
    } else {
        // noise_atap over each recording's head: the VAD kernel itself over the noise_len samples (its records carry the atap)
        if ((rc = h->s_st_vad.reserve(B))) return rc;
        launch_vad(vad_args(h, d_pcm, pcm_stride, h->noise_len, h->noise_len, B, h->s_st_vad.p), s);
        a.atap_src = (const uint8_t *)h->s_st_vad.p;
        a.atap_src_stride = sizeof(sr_vad_rec);
    }
    const uint32_t T = stream_tile_frames();
    const uint32_t F = buf_len > h->frame_len ? (buf_len - h->frame_len + h->hop - 1) / h->hop : 0;
    a.pcm = d_pcm;
    a.pcm_stride = pcm_stride;
    a.buf_len = buf_len;
    a.len = d_len;
    a.B = B;
    a.frame_len = h->frame_len;
    a.hop = h->hop;
    a.v_durmin = h->v_durmin;
    a.s_durmax = h->s_durmax;
    a.n_front = std::max(h->v_durmin, 2u) - 1;
    a.n_states = 2 + a.n_front + (std::max(h->s_durmax, 2u) - 1);
    a.tile_frames = T;
    a.nt = std::max(1u, (F + T - 1) / T);
    a.mask_words = (T + 31) / 32;
    a.max_frames = h->cfg.max_frames;
    const uint64_t slots = (uint64_t)B * a.nt;
    if (slots >= (1ull << 31)) return fail(SR_ERR_BAD_ARG, "recordings too large");
    if ((rc = h->s_st_tab.reserve(slots * 3 * a.n_states))) return rc;
    if ((rc = h->s_st_mask.reserve(slots * 3 * a.mask_words))) return rc;
    if ((rc = h->s_st_tin.reserve(slots))) return rc;
    if ((rc = h->s_st_atap.reserve(B))) return rc;
    a.tab = h->s_st_tab.p;
    a.masks = h->s_st_mask.p;
    a.tile_in = h->s_st_tin.p;
    a.atap_res = h->s_st_atap.p;
    a.atap_out = d_atap;
    a.seg_offsets = d_off;
    a.segs = d_segs;
    a.max_segs = max_segs;
    launch_vad_stream(a, d_atap_in == nullptr, s);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

// records [0, n) of a segmentation (whose thresholds are in s_st_atap) recognised: per chunk of records, rows + records
// (k_stream_records), the frame kernel, DTW, the slot scan, and with nb the word-level N-best of the chunk's score rows
int stream_recognize(sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t B, const sr_stream_seg *d_segs,
                     const uint32_t *d_off, uint32_t n, sr_result *d_results, uint32_t *d_scores, int16_t *d_mfcc, hipStream_t s,
                     const NbestOut *nb = nullptr)
{
    if (!n) return SR_OK;
    int rc;
    const uint32_t R = h->cfg.max_frames, nc = h->nc, K = h->K;
    const uint64_t row = ((uint64_t)kStreamLead + (uint64_t)(R + 1) * h->hop + 16 + 7) & ~7ull;  // samples per record row
    const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, (64ull << 20) / row));  // rows: 128 MB at most
    if ((rc = check_batch(h, chunk))) return rc;
    if ((rc = h->s_st_rows.reserve((size_t)chunk * row))) return rc;
    if ((rc = h->s_st_recs.reserve(chunk))) return rc;
    if (!d_mfcc && (rc = h->s_mfcc.reserve((size_t)chunk * R * nc))) return rc;
    if (!d_scores && (rc = h->s_scores.reserve((size_t)chunk * K))) return rc;
    bool counted = false;
    for (uint32_t r0 = 0; r0 < n; r0 += chunk) {
        const uint32_t m = std::min(chunk, n - r0);
        StreamRecArgs ra{d_pcm, pcm_stride, d_segs, d_off, B, h->s_st_atap.p, r0, h->frame_len, h->hop, R,
                         h->s_st_rows.p, row, h->s_st_recs.p};
        launch_stream_records(ra, m, s);
        int16_t *mc = d_mfcc ? d_mfcc + (size_t)r0 * R * nc : h->s_mfcc.p;
        launch_mfcc(mfcc_args(h, h->s_st_rows.p, row, m, h->s_st_recs.p, mc), mfcc_mag_tab(h), s);
        DtwArgs da = dtw_args(h, mc, h->s_st_recs.p, nullptr, m, d_scores ? d_scores + (size_t)r0 * K : h->s_scores.p, d_results + r0);
        if (launch_dtw_auto(h, da, 0, s, s)) counted = true;
        else launch_argmin(da, s);
        if (nb) launch_nbest(nbest_args(h, da.scores, m, *nb, r0), s);
    }
    if (counted) HIP_TRY(hipEventRecord(h->ev_cells, s));
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

}  // namespace

int sr_stream_segments_dev(sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t buf_len, const uint32_t *d_len,
                           uint32_t B, const sr_atap *d_atap_in, uint32_t max_segs, sr_stream_seg *d_segs,
                           uint32_t *d_seg_offsets, sr_atap *d_atap, void *stream)
{
    int rc = check_stream(h, d_pcm, pcm_stride, buf_len, B, max_segs, d_segs, d_seg_offsets);
    if (rc) return rc;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        HIP_TRY(hipMemsetAsync(d_seg_offsets, 0, sizeof(uint32_t), s));
        return SR_OK;
    }
    if ((rc = order_after_scratch_users(h, s))) return rc;
    if ((rc = stream_segment(h, d_pcm, pcm_stride, buf_len, d_len, B, d_atap_in, max_segs, d_segs, d_seg_offsets, d_atap, s)))
        return rc;
    return mark_scratch_user(h, s);
}

static int recognize_stream_dev(sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t buf_len, const uint32_t *d_len,
                                uint32_t B, const sr_atap *d_atap_in, uint32_t max_segs, sr_stream_seg *d_segs,
                                uint32_t *d_seg_offsets, sr_result *d_results, uint32_t *d_scores, int16_t *d_mfcc, void *stream,
                                const NbestOut *nb)
{
    int rc = check_stream(h, d_pcm, pcm_stride, buf_len, B, max_segs, d_segs, d_seg_offsets);
    if (rc) return rc;
    if (max_segs && !d_results) return fail(SR_ERR_BAD_ARG, "null argument");
    if (!h->K) return fail(SR_ERR_NO_TEMPLATES, "no templates set");
    if (nb && (rc = check_nbest(h, nb->n_best, nb->out))) return rc;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    if (B == 0) {  // no recording: every result slot is padding
        HIP_TRY(hipMemsetAsync(d_seg_offsets, 0, sizeof(uint32_t), s));
    }
    if ((rc = order_after_scratch_users(h, s))) return rc;
    if (B && (rc = stream_segment(h, d_pcm, pcm_stride, buf_len, d_len, B, d_atap_in, max_segs, d_segs, d_seg_offsets, nullptr, s)))
        return rc;
    // the count stays on the device: every one of the max_segs slots is launched, those past the total as failed records
    // (their score rows are all dis_err: the N-best form leaves them empty entries and n_matched 0)
    if ((rc = stream_recognize(h, d_pcm, pcm_stride, B, d_segs, d_seg_offsets, max_segs, d_results, d_scores, d_mfcc, s, nb))) return rc;
    return mark_scratch_user(h, s);
}

int sr_recognize_stream_dev(sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t buf_len, const uint32_t *d_len,
                            uint32_t B, const sr_atap *d_atap_in, uint32_t max_segs, sr_stream_seg *d_segs,
                            uint32_t *d_seg_offsets, sr_result *d_results, uint32_t *d_scores, int16_t *d_mfcc, void *stream)
{
    return recognize_stream_dev(h, d_pcm, pcm_stride, buf_len, d_len, B, d_atap_in, max_segs, d_segs, d_seg_offsets, d_results,
                                d_scores, d_mfcc, stream, nullptr);
}

int sr_recognize_stream_nbest_dev(sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t buf_len,
                                  const uint32_t *d_len, uint32_t B, const sr_atap *d_atap_in, uint32_t max_segs,
                                  sr_stream_seg *d_segs, uint32_t *d_seg_offsets, uint32_t n_best, sr_nbest_entry *d_nbest,
                                  uint32_t *d_n_matched, sr_result *d_results, uint32_t *d_scores, int16_t *d_mfcc,
                                  void *stream)
{
    const NbestOut nb{n_best, d_nbest, d_n_matched};
    return recognize_stream_dev(h, d_pcm, pcm_stride, buf_len, d_len, B, d_atap_in, max_segs, d_segs, d_seg_offsets, d_results,
                                d_scores, d_mfcc, stream, &nb);
}

// nb (N-best form): HOST pointers; its rows are written for the min(total, max_segs) recognised records like the other outputs
static int recognize_stream_host(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, const uint32_t *len,
                                 uint32_t B, const sr_atap *atap_in, uint32_t max_segs, sr_stream_seg *segs, uint32_t *seg_offsets,
                                 sr_result *results, uint32_t *scores, int16_t *mfcc, uint32_t *n_segs, const NbestOut *nb)
{
    if (!h || !pcm || !seg_offsets || (max_segs && !segs)) return fail(SR_ERR_BAD_ARG, "null argument");
    if ((uintptr_t)pcm & 1) return fail(SR_ERR_BAD_ARG, "pcm must be 2-byte aligned");
    if (buf_len > pcm_stride) return fail(SR_ERR_BAD_ARG, "buf_len exceeds pcm_stride");
    if (buf_len < h->noise_len || buf_len <= h->frame_len || buf_len > 0x7FFFFFF0u)
        return fail(SR_ERR_BAD_ARG, "buf_len shorter than the noise head");
    if ((results || scores || mfcc || nb) && !h->K) return fail(SR_ERR_NO_TEMPLATES, "no templates set");
    if ((scores || mfcc) && !results && !nb) return fail(SR_ERR_BAD_ARG, "scores / mfcc need results");
    if (nb) {
        if (int rcn = check_nbest(h, nb->n_best, nb->out)) return rcn;
    }
    for (uint32_t b = 0; len && b < B; b++) {
        if (len[b] > buf_len) return fail(SR_ERR_BAD_ARG, "len[" + std::to_string(b) + "] exceeds buf_len");
        if (!atap_in && (len[b] < h->noise_len || len[b] <= h->frame_len))
            return fail(SR_ERR_BAD_ARG, "len[" + std::to_string(b) + "] shorter than the noise head and a frame");
    }
    ENTER_HOST_CALL(h);
    int rc;
    if (B == 0) {
        seg_offsets[0] = 0;
        if (n_segs) *n_segs = 0;
        return SR_OK;
    }
    uint64_t ds = 0;
    if ((rc = stage_pcm(h, pcm, pcm_stride, buf_len, B, &ds))) return rc;
    uint32_t *d_len = nullptr;
    sr_atap *d_atap_in = nullptr;
    if (len) {
        if ((rc = h->s_u32a.reserve(B))) return rc;
        d_len = h->s_u32a.p;
        COPY_UP(d_len, len, (size_t)B * 4);
    }
    if (atap_in) {
        if ((rc = h->s_atap.reserve(B))) return rc;
        d_atap_in = h->s_atap.p;
        COPY_UP(d_atap_in, atap_in, (size_t)B * sizeof(sr_atap));
    }
    if ((rc = h->s_st_segs.reserve(std::max(1u, max_segs)))) return rc;
    if ((rc = h->s_st_off.reserve((size_t)B + 1))) return rc;
    if ((rc = stream_segment(h, h->s_pcm.p, ds, buf_len, d_len, B, d_atap_in, max_segs, h->s_st_segs.p, h->s_st_off.p, nullptr,
                             nullptr)))
        return rc;
    COPY_DOWN(seg_offsets, h->s_st_off.p, ((size_t)B + 1) * 4);  // syncs on the count
    const uint32_t total = seg_offsets[B], n = std::min(total, max_segs);
    if (n_segs) *n_segs = total;
    if (n) COPY_DOWN(segs, h->s_st_segs.p, (size_t)n * sizeof(sr_stream_seg));
    if ((!results && !nb) || !n) return SR_OK;
    const uint32_t R = h->cfg.max_frames, nc = h->nc, K = h->K;
    NbestOut d_nb{};
    if (nb) {
        if ((rc = h->s_nbest.reserve((size_t)n * nb->n_best))) return rc;
        if ((rc = h->s_nmatched.reserve(n))) return rc;
        d_nb = NbestOut{nb->n_best, h->s_nbest.p, h->s_nmatched.p};
    }
    if ((rc = h->s_results.reserve(n))) return rc;
    if (scores && (rc = h->s_scores.reserve((size_t)n * K))) return rc;
    if (mfcc && (rc = h->s_mfcc.reserve((size_t)n * R * nc))) return rc;
    if ((rc = stream_recognize(h, h->s_pcm.p, ds, B, h->s_st_segs.p, h->s_st_off.p, n, h->s_results.p,
                               scores ? h->s_scores.p : nullptr, mfcc ? h->s_mfcc.p : nullptr, nullptr, nb ? &d_nb : nullptr)))
        return rc;
    if (nb) {
        COPY_DOWN(nb->out, h->s_nbest.p, (size_t)n * nb->n_best * sizeof(sr_nbest_entry));
        if (nb->n_matched) COPY_DOWN(nb->n_matched, h->s_nmatched.p, (size_t)n * 4);
    }
    if (results) COPY_DOWN(results, h->s_results.p, (size_t)n * sizeof(sr_result));
    if (scores) COPY_DOWN(scores, h->s_scores.p, (size_t)n * K * 4);
    if (mfcc) COPY_DOWN(mfcc, h->s_mfcc.p, (size_t)n * R * nc * 2);
    return SR_OK;
}

int sr_recognize_stream(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, const uint32_t *len,
                        uint32_t B, const sr_atap *atap_in, uint32_t max_segs, sr_stream_seg *segs, uint32_t *seg_offsets,
                        sr_result *results, uint32_t *scores, int16_t *mfcc, uint32_t *n_segs)
{
    return recognize_stream_host(h, pcm, pcm_stride, buf_len, len, B, atap_in, max_segs, segs, seg_offsets, results, scores, mfcc,
                                 n_segs, nullptr);
}

int sr_recognize_stream_nbest(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, const uint32_t *len,
                              uint32_t B, const sr_atap *atap_in, uint32_t max_segs, sr_stream_seg *segs,
                              uint32_t *seg_offsets, uint32_t n_best, sr_nbest_entry *nbest, uint32_t *n_matched,
                              sr_result *results, uint32_t *scores, int16_t *mfcc, uint32_t *n_segs)
{
    const NbestOut nb{n_best, nbest, n_matched};
    return recognize_stream_host(h, pcm, pcm_stride, buf_len, len, B, atap_in, max_segs, segs, seg_offsets, results, scores, mfcc,
                                 n_segs, &nb);
}
