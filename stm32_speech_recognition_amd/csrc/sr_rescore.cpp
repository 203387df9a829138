// Two-pass recognition (include/sr_engine.h, "second pass"): the N-best words of a first pass rescored with the full-DP
// scorer and ranked again, on the device.  Three launches per rescoring behind two fills: k_rescore_mark (the pair set),
// the sparse form of the full-DP kernels (k_dtw_dp.hip: those pairs only), k_nbest over the second-pass score rows.  The
// whole-path device form runs the same sequence per chunk from sr_launch.cpp, the whole-path host form is in sr_host.cpp; the
// host form here stages its rows through sr_stage_host.h.
#include "sr_stage_host.h"

using namespace sr;

int check_rescore(const sr_engine *h, uint32_t n_best, const void *out)
{
    if (h->nc != (uint32_t)kCoef) return fail(SR_ERR_BAD_CONFIG, "the full-DP scorer is built for 12-coefficient records");
    if (int rc = check_nbest(h, n_best, out)) return rc;
    if ((size_t)h->tpl_rows * 48 > h->lds.stage_cap) return fail(SR_ERR_BAD_ARG, "templates too long for the LDS-staged DP kernel");
    return SR_OK;
}

int reserve_rescore(sr_engine *h, uint32_t n_chunks, uint32_t per, size_t n_rows)
{
    if (int rc = h->s_rs_marks.reserve((size_t)n_chunks * h->K * rescore_mark_stride(per))) return rc;
    return h->s_rs_scores.reserve(n_rows * h->K);
}

int launch_rescore(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_frames, uint32_t frames_stride, uint32_t n_best,
                   const sr_nbest_entry *in, const RescoreOut &out, uint32_t chunk, uint32_t per, size_t row0, uint32_t n, hipStream_t s)
{
    if (!n) return SR_OK;
    const uint32_t K = h->K, stride = rescore_mark_stride(n);
    uint8_t *marks = h->s_rs_marks.p + (size_t)chunk * K * rescore_mark_stride(per);
    uint32_t *scores = h->s_rs_scores.p + row0 * K;
    // no pair marked, every second-pass score dis_err (0xFF bytes): what the sparse scorer does not reach stays that way
    HIP_TRY(hipMemsetAsync(marks, 0, (size_t)K * stride, s));
    HIP_TRY(hipMemsetAsync(scores, 0xFF, (size_t)n * K * 4, s));
    const WordTab wt = word_tab(h);
    launch_rescore_mark(RescoreMarkArgs{in + row0 * n_best, n, n_best, K, wt.order, wt.group_start, wt.group_of_slot, h->tpl_rank.p, marks, stride}, s);
    DtwArgs a = dtw_args(h, d_mfcc + h->mfcc_elems(row0), nullptr, d_frames + row0 * frames_stride, n, scores, nullptr);
    if (!h->tpl_staged_ok) a.tplR = nullptr;  // as sr_dtw_dp_batch_dev: such a store takes the generic kernel
    launch_dtw_dp_sparse(a, marks, stride, frames_stride, h->tpl_rank.p, h->dp_lanes, h->lds, s);
    launch_nbest(nbest_args(h, scores, n, NbestOut{n_best, out.out, out.n_rescored}, row0), s);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

static int check_stage(const sr_engine *h, const void *mfcc, const void *frames, uint32_t frames_stride, uint32_t n_rows, uint32_t n_best,
                       const void *in, const void *out)
{
    if (!h || !mfcc || !frames || !in) return fail(SR_ERR_BAD_ARG, "null argument");
    if (int rc = check_rescore(h, n_best, out)) return rc;
    if (!frames_stride) return fail(SR_ERR_BAD_ARG, "frames_stride must be at least 1");
    if (in == out) return fail(SR_ERR_BAD_ARG, "the rescored list must not be the input list");
    if (n_rows > kRescoreMaxRows) return fail(SR_ERR_BAD_ARG, "too many rows");
    return SR_OK;
}

extern "C" {

int sr_rescore_nbest_dp_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                            uint32_t n_best, const sr_nbest_entry *d_nbest_in, sr_nbest_entry *d_nbest_out, uint32_t *d_n_rescored,
                            void *stream)
{
    int rc = check_stage(h, d_mfcc, d_in_frames, frames_stride, n_rows, n_best, d_nbest_in, d_nbest_out);
    if (rc || !n_rows) return rc;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    if ((rc = order_after_scratch_users(h, s))) return rc;  // the marks and the second-pass scores are the engine's
    if ((rc = reserve_rescore(h, 1, n_rows, n_rows))) return rc;
    if ((rc = launch_rescore(h, d_mfcc, d_in_frames, frames_stride, n_best, d_nbest_in, RescoreOut{d_nbest_out, d_n_rescored}, 0, n_rows, 0,
                             n_rows, s)))
        return rc;
    return mark_scratch_user(h, s);
}

int sr_rescore_nbest_dp(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                        uint32_t n_best, const sr_nbest_entry *nbest_in, sr_nbest_entry *nbest_out, uint32_t *n_rescored)
{
    int rc = check_stage(h, mfcc, in_frames, frames_stride, n_rows, n_best, nbest_in, nbest_out);
    if (rc || !n_rows) return rc;
    ENTER_HOST_CALL(h);
    if ((rc = stage_rows(h, mfcc, in_frames, frames_stride, n_rows))) return rc;
    if ((rc = h->s_nbest.reserve((size_t)n_rows * n_best))) return rc;
    if ((rc = h->s_rs_out.reserve((size_t)n_rows * n_best))) return rc;
    if ((rc = h->s_rs_n.reserve(n_rows))) return rc;
    if ((rc = reserve_rescore(h, 1, n_rows, n_rows))) return rc;
    COPY_UP(h->s_nbest.p, nbest_in, (size_t)n_rows * n_best * sizeof(sr_nbest_entry));
    if ((rc = launch_rescore(h, h->s_mfcc.p, h->s_u32a.p, 1, n_best, h->s_nbest.p, RescoreOut{h->s_rs_out.p, h->s_rs_n.p}, 0, n_rows, 0, n_rows,
                             nullptr)))
        return rc;
    COPY_DOWN(nbest_out, h->s_rs_out.p, (size_t)n_rows * n_best * sizeof(sr_nbest_entry));
    if (n_rescored) COPY_DOWN(n_rescored, h->s_rs_n.p, (size_t)n_rows * 4);
    return SR_OK;
}

}  // extern "C"
