// Host-buffer entry points of the C ABI (include/sr_engine.h): captures / records staged through HBM, the diagnostics, and
// the scalar helpers behind the reference-compatible symbols of sr_compat.cpp.  How buffers travel is sr_host_call.h's
// business (HostCall: the pinned staging area and one synchronisation for small calls, blocking copies otherwise); an entry
// point here decides the mode once and writes its launch sequence once, on hc.stream().  Only sr_recognize_batch knows a
// third way up, the chunked upload of large batches overlapped with the kernels.  The whole-path forms of the spotter and the
// decoders share one front and one way down for their outputs (pcm_segments_host / pcm_decode_host, sr_stage_host.h).
#include "sr_stage_host.h"

using namespace sr;

// the kernel sequences that more than one entry point launches itself (no *_dev form): launch + launch-error check
static int run_vad(const VadArgs &a, hipStream_t s)
{
    launch_vad(a, s);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
// DTW of feature records + the slot scan (by k_dtw_cells itself where it owns the pair counters, else k_argmin)
static int run_dtw(sr_engine *h, DtwArgs a, hipStream_t s)
{
    if (launch_dtw_auto(h, a, 0, s, s)) HIP_TRY(hipEventRecord(h->ev_cells, s));
    else launch_argmin(a, s);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

// Host buffers -> results.  `packed` = false: u16 rows of pcm_stride SAMPLES; true: rows of 12-bit codes, two samples in
// three bytes, row stride in BYTES (sr_recognize_batch_packed12).
static int recognize_host(sr_engine *h, const void *pcm, uint64_t row_stride, bool packed, uint32_t buf_len, uint32_t B,
                          sr_result *results, uint32_t *scores, int16_t *mfcc, sr_vad_rec *vad)
{
    if (!h || !pcm || !results) return fail(SR_ERR_BAD_ARG, "null argument");
    if (!h->K) return fail(SR_ERR_NO_TEMPLATES, "no templates set");
    if (B == 0) return SR_OK;
    const uint64_t src_row_bytes = packed ? ((uint64_t)(buf_len + 1) / 2) * 3 : (uint64_t)buf_len * 2;  // bytes that carry samples
    const uint64_t src_pitch = packed ? row_stride : row_stride * 2;
    if (src_row_bytes > src_pitch) return fail(SR_ERR_BAD_ARG, packed ? "row stride smaller than ceil(buf_len / 2) * 3 bytes" : "buf_len exceeds pcm_stride");
    ENTER_HOST_CALL(h);
    const uint64_t ds = dev_pitch(buf_len);
    const uint64_t dpk = ds / 8 * 12;  // device pitch of a packed row: whole groups of 8 samples = 12 bytes
    int rc;
    if ((rc = h->s_pcm.reserve((size_t)B * ds))) return rc;
    if (packed && (rc = h->s_pack.reserve((size_t)B * dpk + 16))) return rc;
    if ((rc = h->s_results.reserve(B))) return rc;
    if ((rc = h->s_vad.reserve(B))) return rc;
    if ((rc = h->s_mfcc.reserve(h->mfcc_elems(B)))) return rc;
    if ((rc = h->s_scores.reserve((size_t)B * h->K))) return rc;
    // The upload dominates (2*buf_len bytes per utterance over PCIe vs ~0.5 us of kernels): split the batch into
    // chunks and let the upload of chunk c+1 run on the copy stream while chunk c is processed on the compute
    // stream.  hipMemcpy2DAsync from pageable memory returns when the host buffer has been consumed, so the host
    // thread paces the copies; kernels are only enqueued.  Results come back once, after the last chunk.
    const uint32_t n_chunks = (B >= 2048) ? std::min<uint32_t>(16, B / 1024) : 1;
    const uint8_t *src = (const uint8_t *)pcm;
    // A few captures (spch_recg's one): two blocking copies cost more than the kernels.  The rows go through the pinned staging
    // area, the result records are written by the kernel into pinned host memory, and the host waits once.
    const bool pinned = !packed && !h->profiling && B <= kPinMaxB && pin_fits(h, (size_t)B * ds * 2, (size_t)B * sizeof(sr_result));
    if (n_chunks <= 1 || h->profiling) {  // one chunk, pinned or blocking (kPinMaxB captures are one chunk)
        HostCall hc(h, pinned);
        void *d_res = h->s_results.p;
        uint64_t ds_up = 0;
        if (packed) {  // (never pinned: nothing is outstanding if this returns)
            HIP_TRY(hipMemcpy2D(h->s_pack.p, dpk, src, src_pitch, src_row_bytes, B, hipMemcpyHostToDevice));
            launch_unpack12(h->s_pack.p, dpk, h->s_pcm.p, ds, buf_len, B, nullptr);
        } else {
            rc = hc.put_rows((const uint16_t *)pcm, row_stride, buf_len, B, &ds_up);
        }
        if (!rc && pinned) rc = hc.land(results, (size_t)B * sizeof(sr_result), &d_res);
        if (!rc)
            rc = sr_recognize_batch_dev(h, h->s_pcm.p, ds, buf_len, B, (sr_result *)d_res, h->s_scores.p, h->s_mfcc.p, h->s_vad.p,
                                        hc.stream());
        if ((rc = hc.finish(rc))) return rc;
    } else {
        if (!h->st_copy) HIP_TRY(hipStreamCreateWithFlags(&h->st_copy, hipStreamNonBlocking));
        if (!h->st_comp) HIP_TRY(hipStreamCreateWithFlags(&h->st_comp, hipStreamNonBlocking));
        while (h->ev_chunk.size() < n_chunks) {
            hipEvent_t e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            h->ev_chunk.push_back(e);
        }
        HIP_TRY(hipDeviceSynchronize());  // earlier null-stream work on the scratch buffers is finished
        const uint32_t per = (B + n_chunks - 1) / n_chunks;
        for (uint32_t c = 0, b0 = 0; b0 < B; c++, b0 += per) {
            const uint32_t n = std::min(per, B - b0);
            if (packed)
                HIP_TRY(hipMemcpy2DAsync(h->s_pack.p + (size_t)b0 * dpk, dpk, src + (size_t)b0 * src_pitch, src_pitch, src_row_bytes, n,
                                         hipMemcpyHostToDevice, h->st_copy));
            else
                HIP_TRY(hipMemcpy2DAsync(h->s_pcm.p + (size_t)b0 * ds, ds * 2, src + (size_t)b0 * src_pitch, src_pitch, src_row_bytes, n,
                                         hipMemcpyHostToDevice, h->st_copy));
            HIP_TRY(hipEventRecord(h->ev_chunk[c], h->st_copy));
            HIP_TRY(hipStreamWaitEvent(h->st_comp, h->ev_chunk[c], 0));
            if (packed) launch_unpack12(h->s_pack.p + (size_t)b0 * dpk, dpk, h->s_pcm.p + (size_t)b0 * ds, ds, buf_len, n, h->st_comp);
            rc = sr_recognize_batch_dev(h, h->s_pcm.p + (size_t)b0 * ds, ds, buf_len, n, h->s_results.p + b0,
                                        h->s_scores.p + (size_t)b0 * h->K, h->s_mfcc.p + h->mfcc_elems(b0), h->s_vad.p + b0, h->st_comp);
            if (rc) {
                (void)hipDeviceSynchronize();
                return rc;
            }
        }
        HIP_TRY(hipStreamSynchronize(h->st_comp));
    }
    if (!pinned) COPY_DOWN(results, h->s_results.p, (size_t)B * sizeof(sr_result));  // pinned: finish() has delivered them
    if (scores) COPY_DOWN(scores, h->s_scores.p, (size_t)B * h->K * 4);
    if (mfcc) COPY_DOWN(mfcc, h->s_mfcc.p, h->mfcc_elems(B) * 2);
    if (vad) COPY_DOWN(vad, h->s_vad.p, (size_t)B * sizeof(sr_vad_rec));
    return SR_OK;
}

int sr_recognize_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                       sr_result *results, uint32_t *scores, int16_t *mfcc, sr_vad_rec *vad)
{
    return recognize_host(h, pcm, pcm_stride, false, buf_len, B, results, scores, mfcc, vad);
}

// sr_recognize_batch, then the N-best of the score rows it left in the engine's scratch (all of them, whichever way the
// captures went up), on the null stream the plain call's copies ran on
// (nbest == NULL: the rescored form that does not want the first-pass list back; the checks are the caller's then)
static int recognize_nbest_host(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B, uint32_t n_best,
                                sr_nbest_entry *nbest, uint32_t *n_matched, sr_result *results, uint32_t *scores, int16_t *mfcc,
                                sr_vad_rec *vad)
{
    int rc;
    if ((rc = recognize_host(h, pcm, pcm_stride, false, buf_len, B, results, scores, mfcc, vad)) || B == 0) return rc;
    ENTER_DEVICE(h);
    if ((rc = h->s_nbest.reserve((size_t)B * n_best))) return rc;
    if ((rc = h->s_nmatched.reserve(B))) return rc;
    launch_nbest(nbest_args(h, h->s_scores.p, B, NbestOut{n_best, h->s_nbest.p, h->s_nmatched.p}, 0), nullptr);
    HIP_TRY(hipGetLastError());
    if (nbest) COPY_DOWN(nbest, h->s_nbest.p, (size_t)B * n_best * sizeof(sr_nbest_entry));
    if (n_matched) COPY_DOWN(n_matched, h->s_nmatched.p, (size_t)B * 4);
    return SR_OK;
}

int sr_recognize_nbest_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B, uint32_t n_best,
                             sr_nbest_entry *nbest, uint32_t *n_matched, sr_result *results, uint32_t *scores, int16_t *mfcc,
                             sr_vad_rec *vad)
{
    if (!h || !pcm || !results) return fail(SR_ERR_BAD_ARG, "null argument");
    if (!h->K) return fail(SR_ERR_NO_TEMPLATES, "no templates set");
    if (int rc = check_nbest(h, n_best, nbest)) return rc;
    return recognize_nbest_host(h, pcm, pcm_stride, buf_len, B, n_best, nbest, n_matched, results, scores, mfcc, vad);
}

// sr_recognize_nbest_batch, then ONE second pass over all B rows where that call left them in the engine's scratch: feature
// records, the frame counts inside the VAD records, the first-pass lists
int sr_recognize_rescored_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B, uint32_t n_best,
                                sr_nbest_entry *nbest, uint32_t *n_matched, sr_nbest_entry *rescored, uint32_t *n_rescored,
                                sr_result *results, uint32_t *scores, int16_t *mfcc, sr_vad_rec *vad)
{
    if (!h || !pcm || !results) return fail(SR_ERR_BAD_ARG, "null argument");
    if (!h->K) return fail(SR_ERR_NO_TEMPLATES, "no templates set");
    int rc = check_rescore(h, n_best, rescored);
    if (rc) return rc;
    if (rescored == nbest) return fail(SR_ERR_BAD_ARG, "the rescored list must not be the first-pass list");
    if (B > kRescoreMaxRows) return fail(SR_ERR_BAD_ARG, "batch too large");
    if ((rc = recognize_nbest_host(h, pcm, pcm_stride, buf_len, B, n_best, nbest, n_matched, results, scores, mfcc, vad)) || B == 0) return rc;
    ENTER_DEVICE(h);
    if ((rc = h->s_rs_out.reserve((size_t)B * n_best))) return rc;
    if ((rc = h->s_rs_n.reserve(B))) return rc;
    if ((rc = reserve_rescore(h, 1, B, B))) return rc;
    if ((rc = launch_rescore(h, h->s_mfcc.p, &h->s_vad.p->frm_num, sizeof(sr_vad_rec) / 4, n_best, h->s_nbest.p,
                             RescoreOut{h->s_rs_out.p, h->s_rs_n.p}, 0, B, 0, B, nullptr)))
        return rc;
    COPY_DOWN(rescored, h->s_rs_out.p, (size_t)B * n_best * sizeof(sr_nbest_entry));
    if (n_rescored) COPY_DOWN(n_rescored, h->s_rs_n.p, (size_t)B * 4);
    return SR_OK;
}

int sr_recognize_batch_packed12(sr_engine *h, const uint8_t *packed, uint64_t row_stride_bytes, uint32_t buf_len, uint32_t B,
                                sr_result *results, uint32_t *scores, int16_t *mfcc, sr_vad_rec *vad)
{
    return recognize_host(h, packed, row_stride_bytes, true, buf_len, B, results, scores, mfcc, vad);
}

int sr_recognize_segments_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                                sr_result *results, uint32_t *scores, sr_vad_rec *vad)
{
    if (!h || !pcm || !results) return fail(SR_ERR_BAD_ARG, "null argument");
    if (!h->K) return fail(SR_ERR_NO_TEMPLATES, "no templates set");
    if (B == 0) return SR_OK;
    if (buf_len > pcm_stride) return fail(SR_ERR_BAD_ARG, "buf_len exceeds pcm_stride");
    ENTER_HOST_CALL(h);
    const uint32_t ms = h->cfg.max_seg;
    uint64_t ds = 0;
    int rc = stage_pcm(h, pcm, pcm_stride, buf_len, B, &ds);
    if (rc) return rc;
    if ((rc = h->s_results.reserve((size_t)B * ms))) return rc;
    if ((rc = h->s_vad.reserve(B))) return rc;
    if ((rc = h->s_scores.reserve((size_t)B * h->K * ms))) return rc;
    rc = sr_recognize_segments_batch_dev(h, h->s_pcm.p, ds, buf_len, B, h->s_results.p, h->s_scores.p, h->s_vad.p, nullptr);
    if (rc) return rc;
    COPY_DOWN(results, h->s_results.p, (size_t)B * ms * sizeof(sr_result));
    if (scores) COPY_DOWN(scores, h->s_scores.p, (size_t)B * h->K * ms * 4);
    if (vad) COPY_DOWN(vad, h->s_vad.p, (size_t)B * sizeof(sr_vad_rec));
    return SR_OK;
}

int sr_vad_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B, sr_vad_rec *vad)
{
    if (!h || !pcm || !vad) return fail(SR_ERR_BAD_ARG, "null argument");
    if (B == 0) return SR_OK;
    if (buf_len > pcm_stride) return fail(SR_ERR_BAD_ARG, "buf_len exceeds pcm_stride");
    ENTER_HOST_CALL(h);
    int rc;
    if ((rc = h->s_vad.reserve(B))) return rc;
    const size_t vbytes = (size_t)B * sizeof(sr_vad_rec);
    HostCall hc(h, B <= kPinMaxB && pin_fits(h, (size_t)B * dev_pitch(buf_len) * 2, vbytes));
    uint64_t ds = 0;
    rc = hc.put_rows(pcm, pcm_stride, buf_len, B, &ds);
    if (!rc) rc = sr_vad_batch_dev(h, h->s_pcm.p, ds, buf_len, B, h->s_vad.p, hc.stream());
    if (!rc) rc = hc.get(vad, h->s_vad.p, vbytes);
    return hc.finish(rc);
}

// diagnostics: per-utterance ballots of the "loud" decision (VAD.C:164), 63 frames per 64-bit word
int sr_vad_debug_masks(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                       sr_vad_rec *vad, uint64_t *masks /* [B][16] */)
{
    if (!h || !pcm || !vad || !masks) return fail(SR_ERR_BAD_ARG, "null argument");
    if (B == 0) return SR_OK;
    if (buf_len > pcm_stride) return fail(SR_ERR_BAD_ARG, "buf_len exceeds pcm_stride");
    ENTER_HOST_CALL(h);
    uint64_t ds = 0;
    int rc = stage_pcm(h, pcm, pcm_stride, buf_len, B, &ds);
    if (rc) return rc;
    if ((rc = check_pcm(h, h->s_pcm.p, ds, buf_len))) return rc;
    if ((rc = h->s_vad.reserve(B))) return rc;
    TmpDevBuf<uint64_t> dm;
    if ((rc = dm.reserve((size_t)B * 16))) return rc;
    HIP_TRY(hipMemset(dm.p, 0, (size_t)B * 16 * 8));
    if ((rc = run_vad(vad_args(h, h->s_pcm.p, ds, buf_len, h->noise_len, B, h->s_vad.p, nullptr, dm.p), nullptr))) return rc;
    COPY_DOWN(vad, h->s_vad.p, (size_t)B * sizeof(sr_vad_rec));
    COPY_DOWN(masks, dm.p, (size_t)B * 16 * 8);
    return SR_OK;
}

// (mfcc_records, the records of explicit segments, is sr_stage_host.h's: the whole-path forms below make them there)
int sr_mfcc_batch_status(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                         const int32_t *start, const int32_t *end, const uint32_t *mid, int16_t *mfcc, uint32_t *frm_num,
                         uint32_t *status)
{
    if (!h || !pcm || !start || !end || !mid || !mfcc) return fail(SR_ERR_BAD_ARG, "null argument");
    if (B == 0) return SR_OK;
    if (buf_len > pcm_stride) return fail(SR_ERR_BAD_ARG, "buf_len exceeds pcm_stride");
    ENTER_HOST_CALL(h);
    std::vector<sr_vad_rec> recs;
    if (int rc_rec = mfcc_records(h, buf_len, B, start, end, mid, frm_num, status, recs)) return rc_rec;
    const size_t mbytes = h->mfcc_elems(B) * 2, rbytes = (size_t)B * sizeof(sr_vad_rec);
    int rc;
    if ((rc = h->s_vad.reserve(B))) return rc;
    if ((rc = h->s_mfcc.reserve(mbytes / 2))) return rc;
    // a few segments (get_mfcc: one) go through the pinned area
    HostCall hc(h, B <= kPinMaxB && mbytes <= kPinMfccBytes && pin_fits(h, (size_t)B * dev_pitch(buf_len) * 2 + rbytes, mbytes, 2, 1));
    uint64_t ds = 0;
    rc = hc.put_rows(pcm, pcm_stride, buf_len, B, &ds);
    if (!rc) rc = hc.put(h->s_vad.p, recs.data(), rbytes);
    if (!rc) rc = sr_mfcc_batch_dev(h, h->s_pcm.p, ds, B, h->s_vad.p, h->s_mfcc.p, hc.stream());
    if (!rc) rc = hc.get(mfcc, h->s_mfcc.p, mbytes);
    return hc.finish(rc);
}

// Word spotting, whole path (sr_spot.cpp has the stage): the front of sr_stage_host.h -- the records and the frame kernel of
// sr_mfcc_batch_status -- then the stage over the feature rows where they are (a failed record has frm_num 0: no hits)
int sr_spot_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B, const int32_t *start,
                  const int32_t *end, const uint32_t *mid, uint32_t win_frames, sr_spot_hit *hits, uint32_t *scores, int16_t *mfcc,
                  uint32_t *frm_num, uint32_t *status)
{
    if (!h || !pcm || !start || !end || !mid || !hits) return fail(SR_ERR_BAD_ARG, "null argument");
    SpotGeom g;
    if (int rc_chk = check_spot(h, B, win_frames, &g)) return rc_chk;
    return pcm_segments_host(h, PcmSegments{pcm, pcm_stride, buf_len, B, start, end, mid, mfcc, frm_num, status},
                             [&](const int16_t *d_mfcc, const uint32_t *d_frames, uint32_t frames_stride) -> int {
                                 const size_t n_rec = (size_t)B * g.n_win * h->K;
                                 int rc;
                                 if ((rc = h->s_spot_hits.reserve(n_rec)) || (scores && (rc = h->s_spot_scores.reserve(n_rec)))) return rc;
                                 if ((rc = launch_spot_stage(h, d_mfcc, d_frames, frames_stride, B, g, h->s_spot_hits.p,
                                                             scores ? h->s_spot_scores.p : nullptr, nullptr)))
                                     return rc;
                                 COPY_DOWN(hits, h->s_spot_hits.p, n_rec * sizeof(sr_spot_hit));
                                 if (scores) COPY_DOWN(scores, h->s_spot_scores.p, n_rec * 4);
                                 return SR_OK;
                             });
}

// Connected-word decoding, whole path (sr_chain.cpp has the stage): the same front, then the public stage into per-call copies
// of the outputs (a failed record has frm_num 0: no parse)
int sr_decode_words_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B, const int32_t *start,
                          const int32_t *end, const uint32_t *mid, uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost,
                          uint32_t word_cost, sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost, int16_t *mfcc,
                          uint32_t *frm_num, uint32_t *status)
{
    if (!h || !pcm || !start || !end || !mid || !rec || !words) return fail(SR_ERR_BAD_ARG, "null argument");
    if (int rc_chk = check_chain(h, max_words, n_words_exact, skip_cost, word_cost)) return rc_chk;
    return pcm_decode_host(h, PcmSegments{pcm, pcm_stride, buf_len, B, start, end, mid, mfcc, frm_num, status}, max_words, rec, words, level_cost,
                           [&](const int16_t *d_mfcc, const uint32_t *d_frames, uint32_t fs, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_lc) {
                               return sr_decode_words_dp_dev(h, d_mfcc, d_frames, fs, B, max_words, n_words_exact, skip_cost, word_cost, d_rec, d_words,
                                                             d_lc, nullptr);
                           });
}

// One-pass connected-word decoding, whole path (sr_onepass.cpp has the stage): the same, the stage with frames_cap = max_frames
int sr_decode_onepass_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B, const int32_t *start,
                            const int32_t *end, const uint32_t *mid, uint32_t words_cap, uint32_t skip_cost, uint32_t word_cost,
                            sr_chain_rec *rec, sr_chain_word *words, int16_t *mfcc, uint32_t *frm_num, uint32_t *status)
{
    if (!h || !pcm || !start || !end || !mid || !rec || !words) return fail(SR_ERR_BAD_ARG, "null argument");
    if (int rc_chk = check_onepass(h, 0u, words_cap, skip_cost, word_cost)) return rc_chk;
    return pcm_decode_host(h, PcmSegments{pcm, pcm_stride, buf_len, B, start, end, mid, mfcc, frm_num, status}, words_cap, rec, words, nullptr,
                           [&](const int16_t *d_mfcc, const uint32_t *d_frames, uint32_t fs, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *) {
                               return sr_decode_onepass_dp_dev(h, d_mfcc, d_frames, fs, B, 0u, words_cap, skip_cost, word_cost, d_rec, d_words, nullptr);
                           });
}

// One-pass grammar decoding, whole path (sr_onepass_gram.cpp has the stage): sr_decode_onepass_batch under a grammar
int sr_decode_onepass_grammar_batch(sr_engine *h, const sr_grammar *g, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                                    const int32_t *start, const int32_t *end, const uint32_t *mid, uint32_t words_cap, uint32_t skip_cost,
                                    uint32_t word_cost, sr_chain_rec *rec, sr_chain_word *words, int16_t *mfcc, uint32_t *frm_num, uint32_t *status)
{
    if (!h || !pcm || !start || !end || !mid || !rec || !words) return fail(SR_ERR_BAD_ARG, "null argument");
    if (int rc_chk = check_onepass_grammar(h, g, 0u, words_cap, skip_cost, word_cost)) return rc_chk;
    return pcm_decode_host(h, PcmSegments{pcm, pcm_stride, buf_len, B, start, end, mid, mfcc, frm_num, status}, words_cap, rec, words, nullptr,
                           [&](const int16_t *d_mfcc, const uint32_t *d_frames, uint32_t fs, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *) {
                               return sr_decode_onepass_grammar_dp_dev(h, g, d_mfcc, d_frames, fs, B, 0u, words_cap, skip_cost, word_cost, d_rec, d_words,
                                                                       nullptr);
                           });
}

// sr_decode_words_batch under a grammar (sr_gram.cpp has the stage)
int sr_decode_grammar_batch(sr_engine *h, const sr_grammar *g, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len,
                            uint32_t B, const int32_t *start, const int32_t *end, const uint32_t *mid, uint32_t max_words,
                            uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *rec, sr_chain_word *words,
                            uint32_t *level_cost, int16_t *mfcc, uint32_t *frm_num, uint32_t *status)
{
    if (!h || !pcm || !start || !end || !mid || !rec || !words) return fail(SR_ERR_BAD_ARG, "null argument");
    if (int rc_chk = check_chain(h, max_words, n_words_exact, skip_cost, word_cost)) return rc_chk;
    if (int rc_chk = check_grammar(h, g)) return rc_chk;
    return pcm_decode_host(h, PcmSegments{pcm, pcm_stride, buf_len, B, start, end, mid, mfcc, frm_num, status}, max_words, rec, words, level_cost,
                           [&](const int16_t *d_mfcc, const uint32_t *d_frames, uint32_t fs, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_lc) {
                               return sr_decode_grammar_dp_dev(h, g, d_mfcc, d_frames, fs, B, max_words, n_words_exact, skip_cost, word_cost, d_rec,
                                                               d_words, d_lc, nullptr);
                           });
}

// the frame kernels' per-frame intermediate values for explicit segments: the records of sr_mfcc_batch_status, staged like
// its large-batch path
// (not pcm_segments_host: the stage here IS the frame kernel -- it reads the capture rows and the records, no feature rows)
int sr_frame_features_batch(sr_engine *h, int kind, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                            const int32_t *start, const int32_t *end, const uint32_t *mid, uint32_t *feat, int16_t *mfcc,
                            uint32_t *frm_num, uint32_t *status)
{
    if (!h || !pcm || !start || !end || !mid || !feat) return fail(SR_ERR_BAD_ARG, "null argument");
    const uint32_t width = sr_frame_feature_width(h, kind);
    if (!width) return fail(SR_ERR_BAD_ARG, "unknown feature kind " + std::to_string(kind));
    if (B == 0) return SR_OK;
    if (buf_len > pcm_stride) return fail(SR_ERR_BAD_ARG, "buf_len exceeds pcm_stride");
    ENTER_HOST_CALL(h);
    std::vector<sr_vad_rec> recs;
    int rc = mfcc_records(h, buf_len, B, start, end, mid, frm_num, status, recs);
    if (rc) return rc;
    uint64_t ds = 0;
    if ((rc = stage_pcm(h, pcm, pcm_stride, buf_len, B, &ds))) return rc;
    if ((rc = h->s_vad.reserve(B))) return rc;
    const size_t n_mfcc = h->mfcc_elems(B), n_feat = (size_t)B * h->cfg.max_frames * width;
    if ((rc = h->s_mfcc.reserve(n_mfcc))) return rc;
    TmpDevBuf<uint32_t> df;
    if ((rc = df.reserve(n_feat))) return rc;
    COPY_UP(h->s_vad.p, recs.data(), (size_t)B * sizeof(sr_vad_rec));
    if ((rc = sr_frame_features_batch_dev(h, kind, h->s_pcm.p, ds, B, h->s_vad.p, df.p, h->s_mfcc.p, nullptr))) return rc;
    COPY_DOWN(feat, df.p, n_feat * sizeof(uint32_t));
    if (mfcc) COPY_DOWN(mfcc, h->s_mfcc.p, n_mfcc * sizeof(int16_t));
    return SR_OK;
}

int sr_mfcc_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                  const int32_t *start, const int32_t *end, const uint32_t *mid, int16_t *mfcc, uint32_t *frm_num)
{
    return sr_mfcc_batch_status(h, pcm, pcm_stride, buf_len, B, start, end, mid, mfcc, frm_num, nullptr);
}

// Template training: save_mdl (main.c:121-138) for n captures + the slot image save_ftr_mdl programs
// (Flash.C:17-67): on success the slot is erased (0xFF) and u16 save_mask | u16 frm_num | frm_num*12 s16 are
// written; on VAD / MFCC failure the slot is left untouched (main.c:126-135).
int sr_train_store(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t n,
                   const uint32_t *slot, void *store, uint32_t n_slots, uint32_t stride_bytes, uint32_t *status)
{
    if (!h || !pcm || !slot || !store) return fail(SR_ERR_BAD_ARG, "null argument");
    if (n == 0) return SR_OK;
    if (buf_len > pcm_stride) return fail(SR_ERR_BAD_ARG, "buf_len exceeds pcm_stride");
    if (stride_bytes < 4 + 2 * h->nc) return fail(SR_ERR_BAD_ARG, "slot stride too small for a v_ftr_tag");
    const uint32_t slot_rows = (stride_bytes - 4) / (2 * h->nc);
    for (uint32_t i = 0; i < n; i++)
        if (slot[i] >= n_slots) return fail(SR_ERR_BAD_ARG, "slot index outside the store");  // Flash.C:22-26
    ENTER_HOST_CALL(h);
    uint64_t ds = 0;
    int rc = stage_pcm(h, pcm, pcm_stride, buf_len, n, &ds);
    if (rc) return rc;
    if ((rc = h->s_vad.reserve(n))) return rc;
    const size_t msz = h->mfcc_elems(n);
    if ((rc = h->s_mfcc.reserve(msz))) return rc;
    if ((rc = sr_vad_batch_dev(h, h->s_pcm.p, ds, buf_len, n, h->s_vad.p, nullptr))) return rc;
    if ((rc = sr_mfcc_batch_dev(h, h->s_pcm.p, ds, n, h->s_vad.p, h->s_mfcc.p, nullptr))) return rc;
    std::vector<sr_vad_rec> recs(n);
    std::vector<int16_t> mf(msz);
    COPY_DOWN(recs.data(), h->s_vad.p, (size_t)n * sizeof(sr_vad_rec));
    COPY_DOWN(mf.data(), h->s_mfcc.p, msz * 2);
    uint8_t *st = (uint8_t *)store;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t code = recs[i].status;  // 0 save_ok, 1 VAD_fail, 2 MFCC_fail (main.c:38-40)
        if (code == SR_ST_OK && recs[i].frm_num > slot_rows) code = SR_ST_MFCC_FAIL;
        if (status) status[i] = code;
        if (code != SR_ST_OK) continue;
        uint8_t *dst = st + (size_t)slot[i] * stride_bytes;
        std::memset(dst, 0xFF, stride_bytes);  // FLASH_ErasePage, Flash.C:32-39
        const uint16_t sign = SR_SAVE_MASK, fr = (uint16_t)recs[i].frm_num;
        std::memcpy(dst, &sign, 2);
        std::memcpy(dst + 2, &fr, 2);
        std::memcpy(dst + 4, &mf[h->mfcc_elems(i)], (size_t)fr * h->nc * 2);
    }
    return SR_OK;
}

int sr_dtw_batch(sr_engine *h, const int16_t *in_mfcc, const uint32_t *in_frames, uint32_t B, uint32_t *scores,
                 sr_result *results)
{
    if (!h || !in_mfcc || !in_frames || !scores) return fail(SR_ERR_BAD_ARG, "null argument");
    if (!h->K) return fail(SR_ERR_NO_TEMPLATES, "no templates set");
    if (B == 0) return SR_OK;
    for (uint32_t b = 0; b < B; b++)
        if (in_frames[b] > h->cfg.max_frames) return fail(SR_ERR_BAD_ARG, "in_frames exceeds max_frames");
    ENTER_HOST_CALL(h);
    int rc;
    const size_t msz = h->mfcc_elems(B);
    if ((rc = h->s_mfcc.reserve(msz))) return rc;
    if ((rc = h->s_u32a.reserve(B))) return rc;
    if ((rc = h->s_scores.reserve((size_t)B * h->K))) return rc;
    if ((rc = h->s_results.reserve(B))) return rc;
    const size_t sc_bytes = (size_t)B * h->K * 4, res_bytes = results ? (size_t)B * sizeof(sr_result) : 0;
    HostCall hc(h, pin_fits(h, msz * 2 + (size_t)B * 4, sc_bytes + res_bytes, 2, 2));  // a few records (dtw(): one)
    rc = hc.put(h->s_mfcc.p, in_mfcc, msz * 2);
    if (!rc) rc = hc.put(h->s_u32a.p, in_frames, (size_t)B * 4);
    if (!rc) rc = run_dtw(h, dtw_args(h, h->s_mfcc.p, nullptr, h->s_u32a.p, B, h->s_scores.p, h->s_results.p), hc.stream());
    if (!rc) rc = hc.get(scores, h->s_scores.p, sc_bytes);
    if (!rc && results) rc = hc.get(results, h->s_results.p, res_bytes);
    return hc.finish(rc);
}

// get_mdl (DTW.C:217-296): merge pairs of feature records along their greedy DTW path
int sr_get_mdl_batch(sr_engine *h, const int16_t *in1, const uint32_t *n1, uint32_t rows1, const int16_t *in2,
                     const uint32_t *n2, uint32_t rows2, uint32_t P, int16_t *mdl, uint32_t mdl_rows,
                     uint32_t *mdl_frames, uint32_t *dis)
{
    if (!h || !in1 || !n1 || !in2 || !n2 || !mdl_frames || !dis || (mdl_rows && !mdl))
        return fail(SR_ERR_BAD_ARG, "null argument");
    if (P == 0) return SR_OK;
    if (h->nc != (uint32_t)kCoef) return fail(SR_ERR_BAD_CONFIG, "get_mdl is built for 12-coefficient records");
    if (rows1 == 0 || rows2 == 0) return fail(SR_ERR_BAD_ARG, "rows1 / rows2 must be at least 1");
    for (uint32_t p = 0; p < P; p++)
        if (n1[p] > rows1 || n2[p] > rows2 || n1[p] > 0xFFFF || n2[p] > 0xFFFF)
            return fail(SR_ERR_BAD_ARG, "frame count exceeds the rows of its record (or the u16 range)");
    ENTER_HOST_CALL(h);
    int rc;
    const size_t e1 = (size_t)P * rows1 * kCoef, e2 = (size_t)P * rows2 * kCoef, eo = (size_t)P * mdl_rows * kCoef;
    if ((rc = h->s_mfcc.reserve(e1 + e2 + eo + 16))) return rc;
    if ((rc = h->s_u32a.reserve((size_t)2 * P))) return rc;
    if ((rc = h->s_u32b.reserve((size_t)2 * P))) return rc;
    int16_t *d1 = h->s_mfcc.p, *d2 = d1 + ((e1 + 3) & ~(size_t)3), *dm = d2 + ((e2 + 3) & ~(size_t)3);  // 8-byte aligned rows
    COPY_UP(d1, in1, e1 * 2);
    COPY_UP(d2, in2, e2 * 2);
    COPY_UP(h->s_u32a.p, n1, (size_t)P * 4);
    COPY_UP(h->s_u32a.p + P, n2, (size_t)P * 4);
    if (eo) HIP_TRY(hipMemset(dm, 0, eo * 2));
    GetMdlArgs a{d1, h->s_u32a.p, rows1, d2, h->s_u32a.p + P, rows2, P, dm, mdl_rows, h->s_u32b.p, h->s_u32b.p + P};
    launch_get_mdl(a, nullptr);
    HIP_TRY(hipGetLastError());
    if (eo) COPY_DOWN(mdl, dm, eo * 2);
    COPY_DOWN(mdl_frames, h->s_u32b.p, (size_t)P * 4);
    COPY_DOWN(dis, h->s_u32b.p + P, (size_t)P * 4);
    return SR_OK;
}

int sr_dtw_dp_batch(sr_engine *h, const int16_t *in_mfcc, const uint32_t *in_frames, uint32_t B, uint32_t *scores)
{
    if (!h || !in_mfcc || !in_frames || !scores) return fail(SR_ERR_BAD_ARG, "null argument");
    if (!h->K) return fail(SR_ERR_NO_TEMPLATES, "no templates set");
    if (B == 0) return SR_OK;
    for (uint32_t b = 0; b < B; b++)
        if (in_frames[b] > h->cfg.max_frames) return fail(SR_ERR_BAD_ARG, "in_frames exceeds max_frames");
    ENTER_HOST_CALL(h);
    int rc;
    const size_t msz = h->mfcc_elems(B);
    if ((rc = h->s_mfcc.reserve(msz))) return rc;
    if ((rc = h->s_u32a.reserve(B))) return rc;
    if ((rc = h->s_scores.reserve((size_t)B * h->K))) return rc;
    COPY_UP(h->s_mfcc.p, in_mfcc, msz * 2);
    COPY_UP(h->s_u32a.p, in_frames, (size_t)B * 4);
    if ((rc = sr_dtw_dp_batch_dev(h, h->s_mfcc.p, h->s_u32a.p, nullptr, B, h->s_scores.p, nullptr))) return rc;
    COPY_DOWN(scores, h->s_scores.p, (size_t)B * h->K * 4);
    return SR_OK;
}

int sr_delta_mfcc_batch(sr_engine *h, const int16_t *mfcc, const uint32_t *frames, uint32_t B, int16_t *delta)
{
    if (!h || !mfcc || !frames || !delta) return fail(SR_ERR_BAD_ARG, "null argument");
    if (B == 0) return SR_OK;
    ENTER_HOST_CALL(h);
    int rc;
    const size_t msz = h->mfcc_elems(B);
    if ((rc = h->s_mfcc.reserve(2 * msz))) return rc;
    if ((rc = h->s_u32a.reserve(B))) return rc;
    COPY_UP(h->s_mfcc.p, mfcc, msz * 2);
    COPY_UP(h->s_u32a.p, frames, (size_t)B * 4);
    if ((rc = sr_delta_mfcc_batch_dev(h, h->s_mfcc.p, nullptr, h->s_u32a.p, B, h->s_mfcc.p + msz, nullptr))) return rc;
    COPY_DOWN(delta, h->s_mfcc.p + msz, msz * 2);
    return SR_OK;
}

// diagnostics: out[3*i + {0,1,2}] = (u32)(log(x)*100), (u32)sqrtf(x), (u32)(sqrtf((s32)x)*10) as the kernels compute them
int sr_math_diag(sr_engine *h, const uint32_t *in, uint32_t *out, uint32_t n)
{
    if (!h || !in || !out) return fail(SR_ERR_BAD_ARG, "null argument");
    if (n == 0) return SR_OK;
    ENTER_DEVICE(h);
    int rc;
    if ((rc = h->s_u32a.reserve(n))) return rc;
    if ((rc = h->s_u32b.reserve((size_t)3 * n))) return rc;
    COPY_UP(h->s_u32a.p, in, (size_t)n * 4);
    launch_math_diag(h->s_u32a.p, h->s_u32b.p, n, h->dev, nullptr);
    HIP_TRY(hipGetLastError());
    COPY_DOWN(out, h->s_u32b.p, (size_t)3 * n * 4);
    return SR_OK;
}

// diagnostics: the cheap magnitude form against the exact one, n in [0, n_max]: out[0] = mismatches, out[1] = first mismatching n
int sr_mag_fast_sweep(sr_engine *h, uint32_t n_max, uint64_t out[2])
{
    if (!h || !out) return fail(SR_ERR_BAD_ARG, "null argument");
    ENTER_DEVICE(h);
    int rc;
    if ((rc = h->s_u32a.reserve(4))) return rc;
    uint32_t init[4] = {0, 0, 0xFFFFFFFFu, 0};
    COPY_UP(h->s_u32a.p, init, sizeof init);
    launch_mag_fast_sweep(n_max, (unsigned long long *)h->s_u32a.p, h->s_u32a.p + 2, nullptr);
    HIP_TRY(hipGetLastError());
    uint32_t back[4];
    COPY_DOWN(back, h->s_u32a.p, sizeof back);
    out[0] = (uint64_t)back[0] | ((uint64_t)back[1] << 32);
    out[1] = back[2];
    return SR_OK;
}

// diagnostics: overwrite the local data share of every compute unit with a seeded pattern (on `stream`, asynchronous); the
// suite launches it between calls so that no kernel can pass by reading what its own previous workgroups left in LDS
int sr_lds_poison(sr_engine *h, uint32_t seed, void *stream, uint32_t *bytes_per_cu)
{
    if (!h) return fail(SR_ERR_BAD_ARG, "null argument");
    ENTER_DEVICE(h);
    const int n = launch_lds_poison(seed, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    if (n < 0) return fail(SR_ERR_HIP, "sr_lds_poison: device attribute query failed");
    if (bytes_per_cu) *bytes_per_cu = (uint32_t)n;
    return SR_OK;
}

// testing build only (launch points, sr_device.h): the poison launches issued through launch points since the hook
// "lds_poison_launches" was last set, and the distinct kernel names they stood in front of, comma-separated
int sr_lds_launch_points(uint64_t *count, char *names, uint32_t names_cap)
{
#ifdef SR_TESTING
    if (!count) return fail(SR_ERR_BAD_ARG, "null argument");
    *count = launch_points_seen(names, names_cap);
    return SR_OK;
#else
    (void)count, (void)names, (void)names_cap;
    return fail(SR_ERR_BAD_ARG, "sr_lds_launch_points: launch points are not compiled into the product library");
#endif
}

// testing build only: what the first `words` words of every CU's LDS hold (k_lds_probe, launched through a launch point)
int sr_lds_probe(sr_engine *h, uint32_t words, uint32_t *d_out, void *stream)
{
#ifdef SR_TESTING
    if (!h || !d_out || !words || words > 4096u) return fail(SR_ERR_BAD_ARG, "sr_lds_probe: null argument, or words outside 1..4096");
    ENTER_DEVICE(h);
    const int n = launch_lds_probe(words, d_out, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    if (n < 0) return fail(SR_ERR_HIP, "sr_lds_probe: device attribute query failed");
    return SR_OK;
#else
    (void)h, (void)words, (void)d_out, (void)stream;
    return fail(SR_ERR_BAD_ARG, "sr_lds_probe: launch points are not compiled into the product library");
#endif
}

// diagnostics: k_mfcc's fused filterbank term against the reference's expression, see k_mel_term_sweep
int sr_mel_term_sweep(sr_engine *h, uint32_t tri_lo, uint32_t tri_hi, uint32_t e_max, uint64_t *mismatches)
{
    if (!h || !mismatches) return fail(SR_ERR_BAD_ARG, "null argument");
    if (tri_hi <= tri_lo || tri_hi - tri_lo > 65535u || tri_hi - 1 > kMelTriMax || e_max >= (1u << 28))
        return fail(SR_ERR_BAD_ARG, "sr_mel_term_sweep: weights must lie in [0, 1599], at most 65535 of them, and E below 2^28");
    ENTER_DEVICE(h);
    const uint32_t n = tri_hi - tri_lo;
    int rc;
    if ((rc = h->s_u32a.reserve((size_t)2 * n))) return rc;
    HIP_TRY(hipMemset(h->s_u32a.p, 0, (size_t)n * 8));
    launch_mel_term_sweep(tri_lo, n, e_max, (unsigned long long *)h->s_u32a.p, nullptr);
    HIP_TRY(hipGetLastError());
    COPY_DOWN(mismatches, h->s_u32a.p, (size_t)n * 8);
    return SR_OK;
}

int sr_fft_q15_batch(sr_engine *h, const uint32_t *in, uint32_t *out, uint32_t n)
{
    if (!h || !in || !out) return fail(SR_ERR_BAD_ARG, "null argument");
    if (n == 0) return SR_OK;
    ENTER_HOST_CALL(h);
    int rc;
    if ((rc = h->s_u32a.reserve((size_t)n * kNfft))) return rc;
    if ((rc = h->s_u32b.reserve((size_t)n * kNfft))) return rc;
    COPY_UP(h->s_u32a.p, in, (size_t)n * kNfft * 4);
    launch_fft_q15(h->s_u32a.p, h->s_u32b.p, n, h->dev, nullptr);
    HIP_TRY(hipGetLastError());
    COPY_DOWN(out, h->s_u32b.p, (size_t)n * kNfft * 4);
    return SR_OK;
}

namespace sr {
int engine_fft_mag(sr_engine *h, const int16_t *frame, uint32_t len, uint32_t *mag, uint32_t *raw_hi)
{
    ENTER_HOST_CALL(h);
    int rc;
    if ((rc = h->s_mfcc.reserve(len > 0 ? len : 1))) return rc;
    if ((rc = h->s_u32a.reserve(kBins))) return rc;
    if ((rc = h->s_u32b.reserve(kBins))) return rc;
    if (len) COPY_UP(h->s_mfcc.p, frame, (size_t)len * 2);
    launch_fft_mag(h->s_mfcc.p, len, h->s_u32a.p, h->s_u32b.p, 1, h->dev, nullptr);
    HIP_TRY(hipGetLastError());
    COPY_DOWN(mag, h->s_u32a.p, kBins * 4);
    COPY_DOWN(raw_hi, h->s_u32b.p, kBins * 4);
    return SR_OK;
}

// get_dis() / dtw_limit(): one item of the batched forms below
int engine_get_dis(sr_engine *h, const int16_t *a, const int16_t *b, uint32_t *out) { return sr_get_dis_batch(h, a, b, 1, out); }

// dtw_limit (DTW.C:76-109) on n points (x, y) with the statics X1, X2, in_n, mdl_n of the dtw() call before; out[i] = 1: outside
static int dtw_limit_points(sr_engine *h, const uint16_t *xy, uint32_t n, int X1, int X2, int in_n, int mdl_n, uint8_t *out)
{
    ENTER_HOST_CALL(h);
    if (int rc = h->s_u32a.reserve(((size_t)n * 4 + 3) / 4 + ((size_t)n + 3) / 4)) return rc;  // the points, then a byte each
    uint8_t *d_out = (uint8_t *)(h->s_u32a.p + n);
    COPY_UP(h->s_u32a.p, xy, (size_t)n * 4);
    launch_dtw_limit((const uint16_t *)h->s_u32a.p, d_out, n, X1, X2, in_n, mdl_n, nullptr);
    HIP_TRY(hipGetLastError());
    COPY_DOWN(out, d_out, n);
    return SR_OK;
}

int engine_dtw_limit(sr_engine *h, uint16_t x, uint16_t y, int X1, int X2, int in_n, int mdl_n, uint8_t *out)
{
    const uint16_t xy[2] = {x, y};
    return dtw_limit_points(h, xy, 1, X1, X2, in_n, mdl_n, out);
}

}  // namespace sr

// Batched forms of the two small scalar symbols (the kernels get_dis() / dtw_limit() launch with n = 1), so that tests can
// compare them with the reference object over whole grids in one launch.
// get_dis (DTW.C:45-62) on n pairs of 12-coefficient rows
int sr_get_dis_batch(sr_engine *h, const int16_t *a, const int16_t *b, uint32_t n, uint32_t *out)
{
    if (!h || !a || !b || !out) return fail(SR_ERR_BAD_ARG, "null argument");
    if (n == 0) return SR_OK;
    if (h->nc != (uint32_t)kCoef) return fail(SR_ERR_BAD_CONFIG, "sr_get_dis_batch: 12-coefficient front ends only");
    ENTER_HOST_CALL(h);
    int rc;
    if ((rc = h->s_mfcc.reserve((size_t)2 * n * kCoef))) return rc;
    if ((rc = h->s_u32a.reserve(n))) return rc;
    COPY_UP(h->s_mfcc.p, a, (size_t)n * kCoef * 2);
    COPY_UP(h->s_mfcc.p + (size_t)n * kCoef, b, (size_t)n * kCoef * 2);
    launch_get_dis(h->s_mfcc.p, h->s_mfcc.p + (size_t)n * kCoef, h->s_u32a.p, n, nullptr);
    HIP_TRY(hipGetLastError());
    COPY_DOWN(out, h->s_u32a.p, (size_t)n * 4);
    return SR_OK;
}

// dtw_limit (DTW.C:76-109) on n points (x, y) for the statics a dtw() call of in_frames against mdl_frames leaves behind
// (DTW.C:129-130, 141-142: X1 = (2 mdl - in) / 3, X2 = (4 in - 2 mdl) / 3 as u16); out[i] = 1: outside
int sr_dtw_limit_batch(sr_engine *h, const uint16_t *xy, uint32_t n, uint32_t in_frames, uint32_t mdl_frames, uint8_t *out)
{
    if (!h || !xy || !out) return fail(SR_ERR_BAD_ARG, "null argument");
    if (n == 0) return SR_OK;
    if (in_frames > 65535u || mdl_frames > 65535u) return fail(SR_ERR_BAD_ARG, "sr_dtw_limit_batch: frame counts are u16 (DTW.C:65-68)");
    // the statics a dtw() call of in_frames against mdl_frames leaves behind (DTW.C:129-130, 141-142), as u16
    const int X1 = (int)(uint16_t)((2 * (int)mdl_frames - (int)in_frames) / 3), X2 = (int)(uint16_t)((4 * (int)in_frames - 2 * (int)mdl_frames) / 3);
    return dtw_limit_points(h, xy, n, X1, X2, (int)in_frames, (int)mdl_frames, out);
}

namespace sr {

int engine_vad_with_atap(sr_engine *h, const uint16_t *pcm, uint32_t buf_len, const sr_atap *atap, sr_vad_rec *rec)
{
    ENTER_HOST_CALL(h);
    int rc;
    if ((rc = h->s_vad.reserve(1))) return rc;
    if ((rc = h->s_atap.reserve(1))) return rc;
    HostCall hc(h, pin_fits(h, (size_t)dev_pitch(buf_len) * 2 + sizeof(sr_atap), sizeof(sr_vad_rec), 2, 1));  // VAD(): one capture
    uint64_t ds = 0;
    rc = hc.put_rows(pcm, buf_len, buf_len, 1, &ds);
    if (!rc) rc = hc.put(h->s_atap.p, atap, sizeof(sr_atap));
    if (!rc) rc = run_vad(vad_args(h, h->s_pcm.p, ds, buf_len, h->noise_len, 1, h->s_vad.p, h->s_atap.p), hc.stream());
    if (!rc) rc = hc.get(rec, h->s_vad.p, sizeof(sr_vad_rec));
    return hc.finish(rc);
}

// noise_atap alone: run the VAD kernel on the noise head only (buf_len = n_len gives F frames of no
// interest; only the atap part of the record is used)
int engine_noise_atap(sr_engine *h, const uint16_t *noise, uint32_t n_len, sr_atap *out)
{
    ENTER_HOST_CALL(h);
    int rc;
    if ((rc = h->s_vad.reserve(1))) return rc;
    HostCall hc(h, pin_fits(h, (size_t)dev_pitch(n_len) * 2, sizeof(sr_vad_rec)));  // noise_atap(): one noise head
    uint64_t ds = 0;
    sr_vad_rec rec;
    rc = hc.put_rows(noise, n_len, n_len, 1, &ds);
    if (!rc) rc = run_vad(vad_args(h, h->s_pcm.p, ds, n_len, n_len, 1, h->s_vad.p), hc.stream());
    if (!rc) rc = hc.get(&rec, h->s_vad.p, sizeof(sr_vad_rec));
    if (!(rc = hc.finish(rc))) *out = rec.atap;
    return rc;
}
}  // namespace sr
