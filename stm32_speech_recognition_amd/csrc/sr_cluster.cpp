// Word-model clustering (include/sr_engine.h, "word models: clustering a word's examples"): the checks, the plan
// (sr_cluster_plan.h) and the sequencing -- per iteration k_cluster_score over every (example, model of its word) pair,
// k_cluster_assign, k_cluster_tally, then the DBA iteration of sr_align.cpp (k_dp_align on the chosen pairs, k_align_accum,
// k_align_finalise) with the assignment as its example -> model map.  Everything stays on the caller's stream; the host
// knows every count, nothing is read back.  The host forms stage their rows through sr_stage_host.h.
#include "sr_stage_host.h"

using namespace sr;

namespace {

struct Buf {
    const void *p;
    size_t bytes;
};
template <size_t N>
bool any_overlap(const Buf (&b)[N])
{
    for (size_t i = 0; i < N; i++)
        for (size_t j = i + 1; j < N; j++)
            if (overlap(b[i].p, b[i].bytes, b[j].p, b[j].bytes)) return true;
    return false;
}

// what both calls check before their own buffers; E and M come back
int check_cluster(const sr_engine *h, AlignIn *in, const uint32_t *word_start, const uint32_t *mdl_start, uint32_t W, const void *cen,
                  const void *cen_frames, uint32_t cen_rows, uint32_t *M)
{
    if (int rc = check_align_common(h, *in, cen, cen_frames, cen_rows, "cen_rows")) return rc;
    if (!word_start || !mdl_start) return fail(SR_ERR_BAD_ARG, "null argument");
    if (const char *why = cluster_check(word_start, mdl_start, W, std::min<uint32_t>(h->cfg.max_frames, SR_ALIGN_MAX_FRAMES)))
        return fail(SR_ERR_BAD_ARG, why);
    if (!cluster_fits(cen_rows, h->lds)) return fail(SR_ERR_BAD_ARG, "centroids too long for the score pass's LDS image");
    in->n_rows = word_start[W];
    *M = mdl_start[W];
    return SR_OK;
}

int check_assign(const sr_engine *h, AlignIn *in, const uint32_t *word_start, const uint32_t *mdl_start, uint32_t W, const void *cen,
                 const void *cen_frames, uint32_t cen_rows, const uint32_t *assign, const uint32_t *best, const uint32_t *scores)
{
    uint32_t M;
    if (int rc = check_cluster(h, in, word_start, mdl_start, W, cen, cen_frames, cen_rows, &M)) return rc;
    if (!assign) return fail(SR_ERR_BAD_ARG, "null argument");
    const size_t E = in->n_rows;
    if (any_overlap<3>({{assign, E * 4}, {best, E * 4}, {scores, E * kClusterMax * 4}})) return fail(SR_ERR_BAD_ARG, "d_assign, d_best and d_scores overlap");
    return SR_OK;
}

int check_models(const sr_engine *h, AlignIn *in, const uint32_t *word_start, const uint32_t *mdl_start, uint32_t W, const int16_t *cen_in,
                 const void *cen_frames, uint32_t cen_rows, uint32_t n_iter, const int16_t *cen_out, const uint32_t *assign,
                 const sr_train_stat *stats, const sr_cluster_iter *iter, uint32_t *M)
{
    if (int rc = check_cluster(h, in, word_start, mdl_start, W, cen_in, cen_frames, cen_rows, M)) return rc;
    if (!cen_out) return fail(SR_ERR_BAD_ARG, "null argument");
    if (n_iter < 1 || n_iter > 16) return fail(SR_ERR_BAD_ARG, "n_iter must be 1..16");
    const size_t cen_bytes = (size_t)*M * cen_rows * kCoef * 2;
    if (overlap(cen_out, cen_bytes, cen_in, cen_bytes)) return fail(SR_ERR_BAD_ARG, "d_cen_out overlaps d_cen_in");
    if (any_overlap<5>({{cen_in, cen_bytes}, {cen_out, cen_bytes}, {assign, (size_t)in->n_rows * 4},
                        {stats, (size_t)n_iter * *M * sizeof(sr_train_stat)}, {iter, (size_t)n_iter * sizeof(sr_cluster_iter)}}))
        return fail(SR_ERR_BAD_ARG, "d_cen_out, d_assign, d_stats, d_iter and the centroids overlap");
    return SR_OK;
}

// the plan of a call and its tables in the engine's scratch, uploaded on s
struct Tables {
    ClusterPlan p;
    const uint32_t *mdl0, *nm, *wg;
};
int stage_tables(sr_engine *h, const uint32_t *word_start, const uint32_t *mdl_start, uint32_t W, Tables *t, hipStream_t s)
{
    const int64_t pairs = dev_hook(kHookClusterPairs);  // testing build: a few pairs per launch put seams into small test shapes
    t->p = cluster_plan(word_start, mdl_start, W, pairs > 0 ? (uint32_t)std::min<int64_t>(pairs, kClusterMaxPairs) : kClusterMaxPairs);
    if (int rc = h->s_cl_tab.reserve(std::max<size_t>(t->p.tab.size(), 1))) return rc;
    // (a pageable source is staged before the call returns)
    if (!t->p.tab.empty()) HIP_TRY(hipMemcpyAsync(h->s_cl_tab.p, t->p.tab.data(), t->p.tab.size() * 4, hipMemcpyHostToDevice, s));
    t->mdl0 = h->s_cl_tab.p;
    t->nm = h->s_cl_tab.p + t->p.E;
    t->wg = h->s_cl_tab.p + t->p.wg_at();
    return SR_OK;
}

// every pair's score against `cen`, launch by launch on s
void score_pass(const sr_engine *h, const AlignIn &in, const Tables &t, const int16_t *cen, const uint32_t *cen_frames, uint32_t cen_rows,
                uint32_t *dis, uint32_t *acc, hipStream_t s)
{
    for (size_t l = 0; l + 1 < t.p.cut.size(); l++)
        launch_cluster_score(ClusterScoreArgs{in.mfcc, in.frames, in.frames_stride, h->cfg.max_frames, cen, cen_frames, cen_rows, t.wg, t.mdl0, t.nm,
                                              dis, acc, t.p.cut[l], t.p.cut[l + 1] - t.p.cut[l]},
                             cluster_lds_bytes(cen_rows), s);
}

// the stage on s; every pointer a device pointer except the two host arrays
int run_assign(sr_engine *h, const AlignIn &in, const uint32_t *word_start, const uint32_t *mdl_start, uint32_t W, const int16_t *d_cen,
               const uint32_t *d_cen_frames, uint32_t cen_rows, uint32_t *d_assign, uint32_t *d_best, uint32_t *d_scores, hipStream_t s)
{
    Tables t;
    int rc;
    if ((rc = stage_tables(h, word_start, mdl_start, W, &t, s))) return rc;
    if (!d_scores) {
        if ((rc = h->s_cl_dis.reserve(std::max<size_t>((size_t)t.p.E * kClusterMax, 1)))) return rc;
        d_scores = h->s_cl_dis.p;
    }
    score_pass(h, in, t, d_cen, d_cen_frames, cen_rows, d_scores, nullptr, s);
    launch_cluster_assign(ClusterAssignArgs{d_scores, nullptr, t.mdl0, t.nm, t.p.E, nullptr, nullptr, d_assign, d_best, nullptr, nullptr}, s);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

// the full operation on s
int run_models(sr_engine *h, const AlignIn &in, const uint32_t *word_start, const uint32_t *mdl_start, uint32_t W, const int16_t *d_cen_in,
               const uint32_t *d_cen_frames, uint32_t cen_rows, uint32_t n_iter, int16_t *d_cen_out, uint32_t *d_assign, sr_train_stat *d_stats,
               sr_cluster_iter *d_iter, hipStream_t s)
{
    Tables t;
    AlignPlan ap;
    int rc;
    if ((rc = stage_tables(h, word_start, mdl_start, W, &t, s))) return rc;
    const uint32_t E = t.p.E, M = t.p.M;
    const bool want_stats = d_stats || d_iter;  // the iteration record is tallied from a statistics row: the caller's, or scratch
    const size_t n_sc = std::max<size_t>((size_t)E * kClusterMax, 1);
    if ((rc = h->s_cl_dis.reserve(n_sc)) || (want_stats && (rc = h->s_cl_acc.reserve(n_sc))) ||
        (rc = h->s_cl_map.reserve(std::max<size_t>((size_t)2 * E, 1))) || (d_iter && !d_stats && (rc = h->s_cl_stat.reserve(M))) ||
        (rc = dba_begin(h, E, M, cen_rows, n_iter, &ap, s)))
        return rc;
    if (d_stats) HIP_TRY(hipMemsetAsync(d_stats, 0, (size_t)n_iter * M * sizeof(sr_train_stat), s));
    if (d_iter) HIP_TRY(hipMemsetAsync(d_iter, 0, (size_t)n_iter * sizeof(sr_cluster_iter), s));
    const int16_t *cur = d_cen_in;
    for (uint32_t it = 0; it < n_iter; it++) {
        // the outputs alternate between the scratch set and d_cen_out so that the last one lands in d_cen_out
        int16_t *next = (n_iter - 1 - it) % 2 == 0 ? d_cen_out : h->s_al_cen.p;
        uint32_t *map = h->s_cl_map.p + (size_t)(it & 1) * E, *prev = h->s_cl_map.p + (size_t)(~it & 1) * E;
        sr_train_stat *st = d_stats ? d_stats + (size_t)it * M : want_stats ? h->s_cl_stat.p : nullptr;
        sr_cluster_iter *ir = d_iter ? d_iter + it : nullptr;
        if (st && !d_stats) HIP_TRY(hipMemsetAsync(st, 0, (size_t)M * sizeof(sr_train_stat), s));
        score_pass(h, in, t, cur, d_cen_frames, cen_rows, h->s_cl_dis.p, want_stats ? h->s_cl_acc.p : nullptr, s);
        launch_cluster_assign(ClusterAssignArgs{h->s_cl_dis.p, h->s_cl_acc.p, t.mdl0, t.nm, E, it ? prev : nullptr, map,
                                                it + 1 == n_iter ? d_assign : nullptr, nullptr, st, ir},
                              s);
        if (ir) launch_cluster_tally(st, M, ir, s);
        // the update: this call's statistics are the assign kernel's, so k_align_accum gets none -- it would count the
        // unassigned examples, whose map entry names no model, as failures of model 0xFFFFFFFF
        if ((rc = dba_iteration(h, in, map, M, cur, d_cen_frames, cen_rows, next, nullptr, ap, s))) return rc;
        cur = next;
    }
    return SR_OK;
}

}  // namespace

extern "C" {

int sr_cluster_assign_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride,
                          const uint32_t *word_start, const uint32_t *mdl_start, uint32_t W, const int16_t *d_cen,
                          const uint32_t *d_cen_frames, uint32_t cen_rows, uint32_t *d_assign, uint32_t *d_best, uint32_t *d_scores,
                          void *stream)
{
    AlignIn in{d_mfcc, d_in_frames, frames_stride, 0};
    int rc = check_assign(h, &in, word_start, mdl_start, W, d_cen, d_cen_frames, cen_rows, d_assign, d_best, d_scores);
    if (rc || !in.n_rows) return rc;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    if ((rc = order_after_scratch_users(h, s))) return rc;  // the tables (and the scores) are the engine's
    if ((rc = run_assign(h, in, word_start, mdl_start, W, d_cen, d_cen_frames, cen_rows, d_assign, d_best, d_scores, s))) return rc;
    return mark_scratch_user(h, s);
}

int sr_cluster_assign(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, const uint32_t *word_start,
                      const uint32_t *mdl_start, uint32_t W, const int16_t *cen, const uint32_t *cen_frames, uint32_t cen_rows,
                      uint32_t *assign, uint32_t *best, uint32_t *scores)
{
    AlignIn in{mfcc, in_frames, frames_stride, 0};
    int rc = check_assign(h, &in, word_start, mdl_start, W, cen, cen_frames, cen_rows, assign, best, scores);
    if (rc || !in.n_rows) return rc;
    ENTER_HOST_CALL(h);
    const uint32_t E = in.n_rows, M = mdl_start[W];
    const size_t n_cen = (size_t)M * cen_rows * kCoef;
    TmpDevBuf<int16_t> d_cen;
    TmpDevBuf<uint32_t> d_cf, d_as, d_best, d_sc;
    if ((rc = stage_rows(h, mfcc, in_frames, frames_stride, E)) || (rc = d_cen.reserve(n_cen)) || (rc = d_cf.reserve(M)) ||
        (rc = d_as.reserve(E)) || (best && (rc = d_best.reserve(E))) || (scores && (rc = d_sc.reserve((size_t)E * kClusterMax))))
        return rc;
    COPY_UP(d_cen.p, cen, n_cen * 2);
    COPY_UP(d_cf.p, cen_frames, (size_t)M * 4);
    if ((rc = run_assign(h, AlignIn{h->s_mfcc.p, h->s_u32a.p, 1, E}, word_start, mdl_start, W, d_cen.p, d_cf.p, cen_rows, d_as.p,
                         best ? d_best.p : nullptr, scores ? d_sc.p : nullptr, nullptr)))
        return rc;
    COPY_DOWN(assign, d_as.p, (size_t)E * 4);
    if (best) COPY_DOWN(best, d_best.p, (size_t)E * 4);
    if (scores) COPY_DOWN(scores, d_sc.p, (size_t)E * kClusterMax * 4);
    return SR_OK;
}

int sr_cluster_models_dp_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride,
                             const uint32_t *word_start, const uint32_t *mdl_start, uint32_t W, const int16_t *d_cen_in,
                             const uint32_t *d_cen_frames, uint32_t cen_rows, uint32_t n_iter, int16_t *d_cen_out, uint32_t *d_assign,
                             sr_train_stat *d_stats, sr_cluster_iter *d_iter, void *stream)
{
    AlignIn in{d_mfcc, d_in_frames, frames_stride, 0};
    uint32_t M;
    int rc = check_models(h, &in, word_start, mdl_start, W, d_cen_in, d_cen_frames, cen_rows, n_iter, d_cen_out, d_assign, d_stats, d_iter, &M);
    if (rc) return rc;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    if ((rc = order_after_scratch_users(h, s))) return rc;  // scores, maps, accumulators and the intermediate set are the engine's
    if ((rc = run_models(h, in, word_start, mdl_start, W, d_cen_in, d_cen_frames, cen_rows, n_iter, d_cen_out, d_assign, d_stats, d_iter, s)))
        return rc;
    return mark_scratch_user(h, s);
}

int sr_cluster_models_dp(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, const uint32_t *word_start,
                         const uint32_t *mdl_start, uint32_t W, const int16_t *cen_in, const uint32_t *cen_frames, uint32_t cen_rows,
                         uint32_t n_iter, int16_t *cen_out, uint32_t *assign, sr_train_stat *stats, sr_cluster_iter *iter)
{
    AlignIn in{mfcc, in_frames, frames_stride, 0};
    uint32_t M;
    int rc = check_models(h, &in, word_start, mdl_start, W, cen_in, cen_frames, cen_rows, n_iter, cen_out, assign, stats, iter, &M);
    if (rc) return rc;
    ENTER_HOST_CALL(h);
    const uint32_t E = in.n_rows;
    const size_t n_cen = (size_t)M * cen_rows * kCoef, n_st = (size_t)n_iter * M;
    TmpDevBuf<int16_t> d_in, d_out;
    TmpDevBuf<uint32_t> d_cf, d_as;
    TmpDevBuf<sr_train_stat> d_st;
    TmpDevBuf<sr_cluster_iter> d_it;
    if ((rc = stage_rows(h, mfcc, in_frames, frames_stride, E)) || (rc = d_in.reserve(n_cen)) || (rc = d_out.reserve(n_cen)) ||
        (rc = d_cf.reserve(M)) || (assign && E && (rc = d_as.reserve(E))) || (stats && (rc = d_st.reserve(n_st))) ||
        (iter && (rc = d_it.reserve(n_iter))))
        return rc;
    COPY_UP(d_in.p, cen_in, n_cen * 2);
    COPY_UP(d_cf.p, cen_frames, (size_t)M * 4);
    if ((rc = run_models(h, AlignIn{h->s_mfcc.p, h->s_u32a.p, 1, E}, word_start, mdl_start, W, d_in.p, d_cf.p, cen_rows, n_iter, d_out.p,
                         assign && E ? d_as.p : nullptr, stats ? d_st.p : nullptr, iter ? d_it.p : nullptr, nullptr)))
        return rc;
    COPY_DOWN(cen_out, d_out.p, n_cen * 2);
    if (assign && E) COPY_DOWN(assign, d_as.p, (size_t)E * 4);
    if (stats) COPY_DOWN(stats, d_st.p, n_st * sizeof *stats);
    if (iter) COPY_DOWN(iter, d_it.p, (size_t)n_iter * sizeof *iter);
    return SR_OK;
}

}  // extern "C"
