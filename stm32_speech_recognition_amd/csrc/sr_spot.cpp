// Word spotting (include/sr_engine.h, "word spotting"): subsequence DTW of the templates inside long feature rows.  One
// launch of k_spot per call, plus k_spot_finish when a window is longer than a kernel chunk; the partial records of such a
// call live in the engine's scratch.  The host form stages its rows through sr_stage_host.h; the whole-path host form is in
// sr_host.cpp, next to sr_mfcc_batch_status.
#include "sr_stage_host.h"

using namespace sr;

static constexpr uint32_t kSpotMaxWindows = 65535u * 256u;  // n_rows * n_win of one call, as the rows of a rescoring

static uint32_t spot_forced_cols()
{
    const int64_t v = dev_hook(kHookSpotChunk);  // testing build: small chunks put seams into small test shapes
    return v > 0 ? (uint32_t)std::min<int64_t>(v, 16383) : 0u;
}

int check_spot(const sr_engine *h, uint32_t n_rows, uint32_t win_frames, SpotGeom *g)
{
    if (h->nc != (uint32_t)kCoef) return fail(SR_ERR_BAD_CONFIG, "the word spotter is built for 12-coefficient records");
    if (!h->K) return fail(SR_ERR_NO_TEMPLATES, "no templates set");
    if (store_tpl_len(h) > spot_max_tpl(h->lds)) return fail(SR_ERR_BAD_ARG, "templates too long for the word spotter's LDS image");
    *g = spot_geom(store_tpl_len(h), h->cfg.max_frames, win_frames, spot_forced_cols());
    if ((uint64_t)n_rows * g->n_win > kSpotMaxWindows) return fail(SR_ERR_BAD_ARG, "too many windows (n_rows * n_win)");
    return SR_OK;
}

int launch_spot_stage(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_frames, uint32_t frames_stride, uint32_t n_rows,
                      const SpotGeom &g, sr_spot_hit *d_hits, uint32_t *d_scores, hipStream_t s)
{
    if (!n_rows) return SR_OK;
    if (g.split)
        if (int rc = h->s_spot_part.reserve((size_t)n_rows * g.n_chunks * h->K)) return rc;
    launch_spot(SpotArgs{d_mfcc, d_frames, frames_stride, n_rows, h->cfg.max_frames, h->tpl.p, h->tpl_frames.p, h->tpl_valid.p, h->K,
                         h->tpl_stride, store_tpl_len(h), g.n_win, g.win, g.chunk_cols, g.n_chunks, g.split, g.per, d_hits, d_scores,
                         g.split ? h->s_spot_part.p : nullptr},
                s);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

static int check_stage(const sr_engine *h, const void *mfcc, const void *frames, uint32_t frames_stride, uint32_t n_rows,
                       uint32_t win_frames, const void *hits, SpotGeom *g)
{
    if (!h || !mfcc || !frames || !hits) return fail(SR_ERR_BAD_ARG, "null argument");
    if (int rc = check_spot(h, n_rows, win_frames, g)) return rc;
    if (!frames_stride) return fail(SR_ERR_BAD_ARG, "frames_stride must be at least 1");
    return SR_OK;
}

extern "C" {

int sr_spot_geometry(uint32_t tpl_rows, uint32_t max_frames, uint32_t win_frames, uint32_t out[4])
{
    if (!out || !tpl_rows || tpl_rows > 16383 || max_frames < 2 || max_frames > 16383) return fail(SR_ERR_BAD_ARG, "null / zero argument");
    const LdsBudget mi355x;  // no device: MI355X's figures
    const SpotGeom g = spot_geom(tpl_rows, max_frames, win_frames, spot_forced_cols());
    out[0] = g.n_win;
    out[1] = spot_lds_bytes(tpl_rows);
    out[2] = spot_max_tpl(mi355x);
    out[3] = g.chunk_cols;
    return SR_OK;
}

int sr_spot_dp_batch_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                         uint32_t win_frames, sr_spot_hit *d_hits, uint32_t *d_scores, void *stream)
{
    SpotGeom g;
    int rc = check_stage(h, d_mfcc, d_in_frames, frames_stride, n_rows, win_frames, d_hits, &g);
    if (rc || !n_rows) return rc;
    ENTER_DEVICE(h);
    const hipStream_t s = (hipStream_t)stream;
    if (g.split && (rc = order_after_scratch_users(h, s))) return rc;  // the partial records are the engine's
    if ((rc = launch_spot_stage(h, d_mfcc, d_in_frames, frames_stride, n_rows, g, d_hits, d_scores, s))) return rc;
    return g.split ? mark_scratch_user(h, s) : SR_OK;
}

int sr_spot_dp_batch(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                     uint32_t win_frames, sr_spot_hit *hits, uint32_t *scores)
{
    SpotGeom g;
    int rc = check_stage(h, mfcc, in_frames, frames_stride, n_rows, win_frames, hits, &g);
    if (rc || !n_rows) return rc;
    ENTER_HOST_CALL(h);
    const size_t n_rec = (size_t)n_rows * g.n_win * h->K;
    if ((rc = stage_rows(h, mfcc, in_frames, frames_stride, n_rows))) return rc;
    if ((rc = h->s_spot_hits.reserve(n_rec))) return rc;
    if (scores && (rc = h->s_spot_scores.reserve(n_rec))) return rc;
    if ((rc = launch_spot_stage(h, h->s_mfcc.p, h->s_u32a.p, 1, n_rows, g, h->s_spot_hits.p, scores ? h->s_spot_scores.p : nullptr, nullptr)))
        return rc;
    COPY_DOWN(hits, h->s_spot_hits.p, n_rec * sizeof(sr_spot_hit));
    if (scores) COPY_DOWN(scores, h->s_spot_scores.p, n_rec * 4);
    return SR_OK;
}

}  // extern "C"
