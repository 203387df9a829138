// Full-DP alignment and DBA training (include/sr_engine.h, "full-DP alignment and word models from many examples"): the checks,
// the launch plan (align_plan, sr_dtw_plan.h) and the sequencing of k_dp_align / k_align_accum / k_align_finalise.  A call is cut
// into launches of as many pairs as the scratch budget holds; everything stays on the caller's stream.  The host forms stage
// their rows through sr_stage_host.h.
#include "sr_stage_host.h"

using namespace sr;

int check_align_common(const sr_engine *h, const AlignIn &in, const void *ref, const void *ref_frames, uint32_t ref_rows, const char *what)
{
    if (!h || !in.mfcc || !in.frames || !ref || !ref_frames) return fail(SR_ERR_BAD_ARG, "null argument");
    if (h->nc != (uint32_t)kCoef) return fail(SR_ERR_BAD_CONFIG, "the full-DP aligner is built for 12-coefficient records");
    if (!in.frames_stride) return fail(SR_ERR_BAD_ARG, "frames_stride must be at least 1");
    if (!ref_rows || ref_rows > SR_ALIGN_MAX_FRAMES) return fail(SR_ERR_BAD_ARG, std::string(what) + " must be 1..SR_ALIGN_MAX_FRAMES");
    return SR_OK;
}

namespace {

AlignPlan plan_for(uint32_t max_frames, uint32_t ref_rows, const LdsBudget &lds, size_t extra)
{
    const int64_t pairs = dev_hook(kHookAlignPairs);  // testing build: a few pairs per launch put seams into small test shapes
    return align_plan(max_frames, ref_rows, lds, extra, dev_hook(kHookAlignGlobal) != 0,
                      pairs > 0 ? (uint32_t)std::min<int64_t>(pairs, kAlignMaxPairs) : 0u);
}

int check_align(const sr_engine *h, const AlignIn &in, const void *ref, const void *ref_frames, uint32_t ref_rows, uint32_t n_ref,
                const void *ref_of_row, const sr_align_rec *rec, const uint32_t *span)
{
    if (int rc = check_align_common(h, in, ref, ref_frames, ref_rows, "ref_rows")) return rc;
    if (!rec) return fail(SR_ERR_BAD_ARG, "null argument");
    if (!n_ref || (!ref_of_row && n_ref < in.n_rows)) return fail(SR_ERR_BAD_ARG, "fewer references than rows and no d_ref_of_row");
    if (overlap(rec, (size_t)in.n_rows * sizeof *rec, span, (size_t)in.n_rows * h->cfg.max_frames * 4))
        return fail(SR_ERR_BAD_ARG, "d_rec and d_span overlap");
    return SR_OK;
}

// rows [0, n_rows) against their references, in launches of p.pairs pairs on s.  rec / span: the caller's (whole call), or
// nullptr = the engine's per-launch scratch, which `after` (optional) consumes launch by launch.
template <typename After>
int run_align(sr_engine *h, const AlignIn &in, const int16_t *ref, const uint32_t *ref_frames, uint32_t ref_rows, uint32_t n_ref,
              const uint32_t *ref_of_row, sr_align_rec *rec, uint32_t *span, bool scratch_out, const AlignPlan &p, hipStream_t s, After after)
{
    for (uint32_t r0 = 0; r0 < in.n_rows; r0 += p.pairs) {
        const uint32_t n = std::min(p.pairs, in.n_rows - r0);
        launch_align(AlignArgs{in.mfcc, in.frames, in.frames_stride, h->cfg.max_frames, ref, ref_frames, ref_rows, n_ref, ref_of_row,
                               scratch_out ? h->s_al_rec.p : rec, scratch_out ? h->s_al_span.p : span, scratch_out ? r0 : 0u,
                               p.lds_marks ? nullptr : h->s_al_marks.p, p.mark_w, p.mark_words, r0, n},
                     p.lds_bytes, s);
        after(r0, n);
    }
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

int reserve_marks(sr_engine *h, const AlignPlan &p, uint32_t n_rows)
{
    if (p.lds_marks) return SR_OK;
    return h->s_al_marks.reserve((size_t)std::min(p.pairs, n_rows) * p.mark_words);
}

int check_train(const sr_engine *h, const AlignIn &in, const uint32_t *ex_start, uint32_t M, const int16_t *cen_in, const uint32_t *cen_frames,
                uint32_t cen_rows, uint32_t n_iter, const int16_t *cen_out, const sr_train_stat *stats, uint32_t *n_ex)
{
    if (int rc = check_align_common(h, in, cen_in, cen_frames, cen_rows, "cen_rows")) return rc;
    if (!ex_start || !cen_out) return fail(SR_ERR_BAD_ARG, "null argument");
    if (!M) return fail(SR_ERR_BAD_ARG, "no models");
    if (n_iter < 1 || n_iter > 16) return fail(SR_ERR_BAD_ARG, "n_iter must be 1..16");
    if (ex_start[0] != 0) return fail(SR_ERR_BAD_ARG, "ex_start must begin at 0");
    const uint32_t n_cap = std::min<uint32_t>(h->cfg.max_frames, SR_ALIGN_MAX_FRAMES);
    for (uint32_t m = 0; m < M; m++) {
        if (ex_start[m + 1] < ex_start[m]) return fail(SR_ERR_BAD_ARG, "ex_start must be ascending");
        if ((uint64_t)(ex_start[m + 1] - ex_start[m]) * n_cap > 65535u)
            return fail(SR_ERR_BAD_ARG, "too many examples of model " + std::to_string(m) + " for exact s32 sums: examples x min(max_frames, "
                                        "SR_ALIGN_MAX_FRAMES) must not exceed 65535");
    }
    const size_t cen_bytes = (size_t)M * cen_rows * kCoef * 2, st_bytes = (size_t)n_iter * M * sizeof(sr_train_stat);
    if (overlap(cen_out, cen_bytes, cen_in, cen_bytes)) return fail(SR_ERR_BAD_ARG, "d_cen_out overlaps d_cen_in");
    if (overlap(cen_out, cen_bytes, stats, st_bytes) || overlap(cen_in, cen_bytes, stats, st_bytes))
        return fail(SR_ERR_BAD_ARG, "d_stats overlaps the centroids");
    *n_ex = ex_start[M];
    return SR_OK;
}

// the whole training on s; every pointer a device pointer except ex_start
int run_train(sr_engine *h, const AlignIn &in, const uint32_t *ex_start, uint32_t M, const int16_t *d_cen_in, const uint32_t *d_cen_frames,
              uint32_t cen_rows, uint32_t n_iter, int16_t *d_cen_out, sr_train_stat *d_stats, hipStream_t s)
{
    const uint32_t E = in.n_rows;
    AlignPlan p;
    int rc;
    if ((rc = dba_begin(h, E, M, cen_rows, n_iter, &p, s)) || (rc = h->s_al_map.reserve(std::max(E, 1u)))) return rc;
    if (E) {  // (a pageable source is staged before the call returns)
        std::vector<uint32_t> model_of(E);
        for (uint32_t m = 0; m < M; m++) std::fill(model_of.begin() + ex_start[m], model_of.begin() + ex_start[m + 1], m);
        HIP_TRY(hipMemcpyAsync(h->s_al_map.p, model_of.data(), (size_t)E * 4, hipMemcpyHostToDevice, s));
    }
    if (d_stats) HIP_TRY(hipMemsetAsync(d_stats, 0, (size_t)n_iter * M * sizeof(sr_train_stat), s));
    const int16_t *cur = d_cen_in;
    for (uint32_t it = 0; it < n_iter; it++) {
        // the outputs alternate between the scratch set and d_cen_out so that the last one lands in d_cen_out
        int16_t *next = (n_iter - 1 - it) % 2 == 0 ? d_cen_out : h->s_al_cen.p;
        if ((rc = dba_iteration(h, in, h->s_al_map.p, M, cur, d_cen_frames, cen_rows, next, d_stats ? d_stats + (size_t)it * M : nullptr, p, s)))
            return rc;
        cur = next;
    }
    return SR_OK;
}

}  // namespace

int dba_begin(sr_engine *h, uint32_t E, uint32_t M, uint32_t cen_rows, uint32_t n_iter, AlignPlan *p, hipStream_t s)
{
    const uint32_t maxf = h->cfg.max_frames;
    *p = plan_for(maxf, cen_rows, h->lds, (size_t)maxf * 4 + sizeof(sr_align_rec));
    const size_t n_cen = (size_t)M * cen_rows, per = std::min(p->pairs, std::max(E, 1u));
    int rc;
    if ((rc = reserve_marks(h, *p, E)) || (rc = h->s_al_span.reserve(per * maxf)) || (rc = h->s_al_rec.reserve(per)) ||
        (rc = h->s_al_sum.reserve(n_cen * kCoef)) || (rc = h->s_al_cnt.reserve(n_cen)) || (n_iter > 1 && (rc = h->s_al_cen.reserve(n_cen * kCoef))))
        return rc;
    HIP_TRY(hipMemsetAsync(h->s_al_sum.p, 0, n_cen * kCoef * 4, s));
    HIP_TRY(hipMemsetAsync(h->s_al_cnt.p, 0, n_cen * 4, s));
    return SR_OK;
}

int dba_iteration(sr_engine *h, const AlignIn &in, const uint32_t *d_model_of, uint32_t M, const int16_t *cur, const uint32_t *d_cen_frames,
                  uint32_t cen_rows, int16_t *next, sr_train_stat *st, const AlignPlan &p, hipStream_t s)
{
    const uint32_t maxf = h->cfg.max_frames;
    int rc = run_align(h, in, cur, d_cen_frames, cen_rows, M, d_model_of, nullptr, nullptr, true, p, s, [&](uint32_t r0, uint32_t n) {
        launch_align_accum(AlignAccumArgs{in.mfcc, in.frames, in.frames_stride, maxf, h->s_al_rec.p, h->s_al_span.p, d_model_of, d_cen_frames,
                                          cen_rows, h->s_al_sum.p, h->s_al_cnt.p, st, r0, n},
                           s);
    });
    if (rc) return rc;
    launch_align_finalise(AlignFinalArgs{cur, next, d_cen_frames, cen_rows, M, h->s_al_sum.p, h->s_al_cnt.p}, s);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

extern "C" {

int sr_align_geometry(uint32_t max_frames, uint32_t ref_rows, uint32_t out[3])
{
    if (!out || !max_frames || max_frames > 16383 || !ref_rows || ref_rows > SR_ALIGN_MAX_FRAMES) return fail(SR_ERR_BAD_ARG, "null / zero argument");
    const LdsBudget mi355x;  // no device: MI355X's figures
    const AlignPlan p = plan_for(max_frames, ref_rows, mi355x, 0);
    out[0] = p.pair_bytes;
    out[1] = p.pairs;
    out[2] = SR_ALIGN_MAX_FRAMES;
    return SR_OK;
}

int sr_dtw_dp_align_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                        const int16_t *d_ref, const uint32_t *d_ref_frames, uint32_t ref_rows, uint32_t n_ref,
                        const uint32_t *d_ref_of_row, sr_align_rec *d_rec, uint32_t *d_span, void *stream)
{
    const AlignIn in{d_mfcc, d_in_frames, frames_stride, n_rows};
    int rc = check_align(h, in, d_ref, d_ref_frames, ref_rows, n_ref, d_ref_of_row, d_rec, d_span);
    if (rc || !n_rows) return rc;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    const AlignPlan p = plan_for(h->cfg.max_frames, ref_rows, h->lds, 0);
    const bool own_scratch = !p.lds_marks;  // the marks are the engine's
    if (own_scratch && ((rc = order_after_scratch_users(h, s)) || (rc = reserve_marks(h, p, n_rows)))) return rc;
    if ((rc = run_align(h, in, d_ref, d_ref_frames, ref_rows, n_ref, d_ref_of_row, d_rec, d_span, false, p, s, [](uint32_t, uint32_t) {})))
        return rc;
    return own_scratch ? mark_scratch_user(h, s) : SR_OK;
}

int sr_dtw_dp_align(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                    const int16_t *ref, const uint32_t *ref_frames, uint32_t ref_rows, uint32_t n_ref, const uint32_t *ref_of_row,
                    sr_align_rec *rec, uint32_t *span)
{
    int rc = check_align(h, AlignIn{mfcc, in_frames, frames_stride, n_rows}, ref, ref_frames, ref_rows, n_ref, ref_of_row, rec, span);
    if (rc || !n_rows) return rc;
    ENTER_HOST_CALL(h);
    const size_t n_span = (size_t)n_rows * h->cfg.max_frames, n_refel = (size_t)n_ref * ref_rows * kCoef;
    TmpDevBuf<int16_t> d_ref;
    TmpDevBuf<uint32_t> d_rf, d_map, d_span;
    TmpDevBuf<sr_align_rec> d_rec;
    if ((rc = stage_rows(h, mfcc, in_frames, frames_stride, n_rows)) || (rc = d_ref.reserve(n_refel)) ||
        (rc = d_rf.reserve(n_ref)) || (rc = d_rec.reserve(n_rows)) || (ref_of_row && (rc = d_map.reserve(n_rows))) ||
        (span && (rc = d_span.reserve(n_span))))
        return rc;
    COPY_UP(d_ref.p, ref, n_refel * 2);
    COPY_UP(d_rf.p, ref_frames, (size_t)n_ref * 4);
    if (ref_of_row) COPY_UP(d_map.p, ref_of_row, (size_t)n_rows * 4);
    if ((rc = sr_dtw_dp_align_dev(h, h->s_mfcc.p, h->s_u32a.p, 1, n_rows, d_ref.p, d_rf.p, ref_rows, n_ref, ref_of_row ? d_map.p : nullptr,
                                  d_rec.p, span ? d_span.p : nullptr, nullptr)))
        return rc;
    COPY_DOWN(rec, d_rec.p, (size_t)n_rows * sizeof *rec);
    if (span) COPY_DOWN(span, d_span.p, n_span * 4);
    return SR_OK;
}

int sr_train_models_dp_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride,
                           const uint32_t *ex_start, uint32_t M, const int16_t *d_cen_in, const uint32_t *d_cen_frames,
                           uint32_t cen_rows, uint32_t n_iter, int16_t *d_cen_out, sr_train_stat *d_stats, void *stream)
{
    AlignIn in{d_mfcc, d_in_frames, frames_stride, 0};
    int rc = check_train(h, in, ex_start, M, d_cen_in, d_cen_frames, cen_rows, n_iter, d_cen_out, d_stats, &in.n_rows);
    if (rc) return rc;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    if ((rc = order_after_scratch_users(h, s))) return rc;  // accumulators, spans and the intermediate set are the engine's
    if ((rc = run_train(h, in, ex_start, M, d_cen_in, d_cen_frames, cen_rows, n_iter, d_cen_out, d_stats, s))) return rc;
    return mark_scratch_user(h, s);
}

int sr_train_models_dp(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, const uint32_t *ex_start,
                       uint32_t M, const int16_t *cen_in, const uint32_t *cen_frames, uint32_t cen_rows, uint32_t n_iter,
                       int16_t *cen_out, sr_train_stat *stats)
{
    AlignIn in{mfcc, in_frames, frames_stride, 0};
    int rc = check_train(h, in, ex_start, M, cen_in, cen_frames, cen_rows, n_iter, cen_out, stats, &in.n_rows);
    if (rc) return rc;
    ENTER_HOST_CALL(h);
    const uint32_t E = in.n_rows;
    const size_t n_cen = (size_t)M * cen_rows * kCoef, n_st = (size_t)n_iter * M;
    TmpDevBuf<int16_t> d_in, d_out;
    TmpDevBuf<uint32_t> d_cf;
    TmpDevBuf<sr_train_stat> d_st;
    if ((rc = stage_rows(h, mfcc, in_frames, frames_stride, E)) || (rc = d_in.reserve(n_cen)) || (rc = d_out.reserve(n_cen)) ||
        (rc = d_cf.reserve(M)) || (stats && (rc = d_st.reserve(n_st))))
        return rc;
    COPY_UP(d_in.p, cen_in, n_cen * 2);
    COPY_UP(d_cf.p, cen_frames, (size_t)M * 4);
    if ((rc = run_train(h, AlignIn{h->s_mfcc.p, h->s_u32a.p, 1, E}, ex_start, M, d_in.p, d_cf.p, cen_rows, n_iter, d_out.p,
                        stats ? d_st.p : nullptr, nullptr)))
        return rc;
    COPY_DOWN(cen_out, d_out.p, n_cen * 2);
    if (stats) COPY_DOWN(stats, d_st.p, n_st * sizeof *stats);
    return SR_OK;
}

}  // extern "C"
