// What the live sessions (sr_spot_live.cpp, sr_decode_live.cpp, sr_gram_live.cpp, sr_onepass_live.cpp, sr_onepass_gram_live.cpp)
// do alike on the host: the session core -- engine, channel plan, the PCM front end's buffers, the event that orders pushes on different streams --
// with its open and release; the checks of a push's input; ONE push sequence for frames or samples, on the device or from
// host buffers; and for the four decoders the output checks, the choice between the device and the host form of a push and
// the sequence of an end call (the host forms' device copies of their outputs, HostOutputs, are the batch decoders' too:
// sr_stage_host.h).  A session supplies its plan, its launch and its advance; nothing here knows a session type.
// HOST ONLY.
#pragma once
#include "sr_decode_live_plan.h"
#include "sr_live_pcm.h"
#include "sr_stage_host.h"

namespace sr {

constexpr uint32_t kLiveMaxChannels = 65535u;  // a grid dimension
constexpr uint32_t kLiveMaxFrames = 16383u;    // the decoders' utt_frames: the u32 cost bound and the start field of a key

// the input of a push: frames (s16 [n][12] rows) or samples (u16 rows), on the device or on the host; stride in elements
struct LiveIn {
    const void *p;
    uint64_t stride;
    bool pcm;
};

struct LiveCore {
    sr_engine *h = nullptr;
    uint32_t C = 0;
    std::vector<uint32_t> mid;            // PCM sessions: the channels' mid values (empty: a feature session)
    DevBuf<SpotLiveChan> d_chan;          // the channel plan of the push in flight
    // PCM sessions: kept samples, the rows [kept | chunk], their records and the features of one push
    DevBuf<uint16_t> keep, stage;
    DevBuf<sr_vad_rec> recs;
    DevBuf<int16_t> feat;
    uint32_t keep_stride = 0;
    uint64_t stage_stride = 0;
    hipEvent_t ev_last = nullptr;         // end of the last push (an end call, a grammar switch and release wait for it)
    hipStream_t last_stream = nullptr;    // ... and the stream it ran on: a push on another stream runs behind it
    bool pending = false;

    // open, before the device is entered: the arguments every session refuses alike.  frame_cap bounds the frames of one push:
    // a push of chunk_max samples must not complete more, a push of frames is at most that long.
    static int check_open(const sr_engine *h, uint32_t n_channels, uint32_t chunk_max, uint32_t frame_cap, const uint32_t *mid)
    {
        if (!n_channels || n_channels > kLiveMaxChannels) return fail(SR_ERR_BAD_ARG, "n_channels not in 1..65535");
        if (!chunk_max) return fail(SR_ERR_BAD_ARG, "chunk_max 0");
        if (!mid) return chunk_max > frame_cap ? fail(SR_ERR_BAD_ARG, "chunk_max not in 1.." + std::to_string(frame_cap) + " frames") : SR_OK;
        if (((uint64_t)chunk_max + h->hop - 1) / h->hop > frame_cap)
            return fail(SR_ERR_BAD_ARG, "a push of chunk_max samples could complete more than " + std::to_string(frame_cap) + " frames");
        for (uint32_t c = 0; c < n_channels; c++)
            if (mid[c] > 0xFFFFu) return fail(SR_ERR_BAD_ARG, "mid exceeds the u16 sample range");
        return check_batch(h, n_channels);
    }
    // open, on the device: the channel plan, the PCM buffers and the event (a failure leaves what release() frees)
    int open_common(sr_engine *engine, uint32_t n_channels, uint32_t chunk_max, const uint32_t *mid_in)
    {
        h = engine;
        C = n_channels;
        int rc = d_chan.reserve(C);
        if (!rc && mid_in) {
            mid.assign(mid_in, mid_in + C);
            keep_stride = live_pcm_keep_stride(h);
            stage_stride = live_pcm_stage_stride(h, chunk_max);
            rc = keep.reserve((size_t)C * keep_stride);
            if (!rc) rc = stage.reserve((size_t)C * stage_stride);
            if (!rc) rc = recs.reserve(C);
            if (!rc) rc = feat.reserve(h->mfcc_elems(C));
        }
        if (!rc && hipEventCreateWithFlags(&ev_last, hipEventDisableTiming) != hipSuccess) rc = fail(SR_ERR_HIP, "hipEventCreate failed");
        return rc;
    }
    void release()
    {
        if (pending) (void)hipEventSynchronize(ev_last);
        d_chan.release();
        keep.release();
        stage.release();
        recs.release();
        feat.release();
        if (ev_last) (void)hipEventDestroy(ev_last);
    }
    int wait_last()
    {
        if (!pending) return SR_OK;
        HIP_TRY(hipEventSynchronize(ev_last));
        pending = false;
        return SR_OK;
    }
    int mark_push(hipStream_t s)
    {
        HIP_TRY(hipEventRecord(ev_last, s));
        pending = true;
        last_stream = s;
        return SR_OK;
    }
    // the channels' state belongs to one push at a time: a push on another stream than the last one's runs behind it
    int order_after_last_push(hipStream_t s)
    {
        if (!pending || s == last_stream) return SR_OK;
        HIP_TRY(hipStreamWaitEvent(s, ev_last, 0));
        return SR_OK;
    }
    // (a pageable source is staged before the call returns: the plan may go out of scope)
    int upload_chan(const std::vector<SpotLiveChan> &chan, hipStream_t s)
    {
        HIP_TRY(hipMemcpyAsync(d_chan.p, chan.data(), (size_t)C * sizeof(SpotLiveChan), hipMemcpyHostToDevice, s));
        return SR_OK;
    }
    // PCM sessions: [kept | chunk] rows, the frame kernel over them as sr_mfcc_batch_dev launches it, the samples to keep
    int launch_front_end(const LivePlan &pl, const uint16_t *d_pcm, uint64_t pcm_stride, hipStream_t s)
    {
        return live_pcm_front_end(h, d_chan.p, pl.chan, mid, pl.max_row, pl.max_frames, d_pcm, pcm_stride, keep.p, keep_stride, stage.p,
                                  stage_stride, recs.p, feat.p, s);
    }
    // what a push enqueues on s, the same for every form: behind the last push, the plan, (PCM) the front end, the session's
    // launch(features, their row stride, s) -- over the caller's frames, or over the features the front end has just written
    template <typename Launch>
    int enqueue(const LivePlan &pl, const LiveIn &d_in, hipStream_t s, Launch &&launch)
    {
        if (int rc = order_after_last_push(s)) return rc;
        if (int rc = upload_chan(pl.chan, s)) return rc;
        if (!d_in.pcm) return launch((const int16_t *)d_in.p, d_in.stride, s);
        if (int rc = launch_front_end(pl, (const uint16_t *)d_in.p, d_in.stride, s)) return rc;
        return launch((const int16_t *)feat.p, (uint64_t)h->cfg.max_frames * kCoef, s);
    }
};

// the input of a push against the kind of the session and the largest count of the plan
inline int check_live_in(bool session_pcm, const LiveIn &in, uint32_t max_n, bool device)
{
    const uintptr_t at = (uintptr_t)in.p;
    if (in.pcm) {
        if (!session_pcm) return fail(SR_ERR_BAD_ARG, "a feature session takes frames (the session's push calls)");
        if (!max_n) return SR_OK;
        if (!in.p) return fail(SR_ERR_BAD_ARG, "null pcm");
        if (max_n > in.stride) return fail(SR_ERR_BAD_ARG, "a count exceeds pcm_stride");
        if (device && ((at & 15) || (in.stride & 7))) return fail(SR_ERR_BAD_ARG, "pcm must be 16-byte aligned, stride % 8 == 0");
        if (!device && (at & 1)) return fail(SR_ERR_BAD_ARG, "pcm must be 2-byte aligned");
        return SR_OK;
    }
    if (session_pcm) return fail(SR_ERR_BAD_ARG, "a PCM session takes samples (the session's push_pcm calls)");
    if (!max_n) return SR_OK;
    if (!in.p) return fail(SR_ERR_BAD_ARG, "null argument");
    if ((uint64_t)max_n * kCoef > in.stride) return fail(SR_ERR_BAD_ARG, "a count exceeds row_stride");
    if (device && ((at & 7) || (in.stride & 3))) return fail(SR_ERR_BAD_ARG, "mfcc must be 8-byte aligned, row_stride % 4 == 0");
    if (!device && (at & 1)) return fail(SR_ERR_BAD_ARG, "mfcc must be 2-byte aligned");
    return SR_OK;
}

// ---- one push, after the session has planned it and checked its inputs and outputs ------------------------------------------
// work: the push enqueues something (the session's own predicate); advance(): the mirror follows, the caller learns its rows.
// Device form: everything on the caller's stream, no synchronisation, nothing read back.
template <typename Launch, typename Advance>
int live_push_dev(LiveCore &k, const LivePlan &pl, bool work, const LiveIn &d_in, void *stream, Launch &&launch, Advance &&advance)
{
    ENTER_DEVICE(k.h);
    const hipStream_t s = (hipStream_t)stream;
    if (work)
        if (int rc = k.enqueue(pl, d_in, s, launch)) return rc;
    advance();
    return work ? k.mark_push(s) : SR_OK;
}

// Host form, on the null stream: the input goes to the engine's s_mfcc / s_pcm, the outputs to device copies that make_out()'s
// object reserves (before anything is enqueued) and copies down (after the mirror has advanced and the push is marked).  The
// object lives inside the call, on the engine's device; launch(out, features, row stride, s) launches into its copies.
template <typename MakeOut, typename Launch, typename Advance>
int live_push_host(LiveCore &k, const LivePlan &pl, bool work, const LiveIn &in, MakeOut &&make_out, Launch &&launch, Advance &&advance)
{
    sr_engine *h = k.h;
    ENTER_HOST_CALL(h);
    auto out = make_out();
    if (work) {
        const size_t per = in.pcm ? 1 : kCoef;  // elements of a count; device rows hold the largest count
        const uint64_t ds = in.pcm ? dev_pitch(pl.max_n) : (uint64_t)pl.max_frames * kCoef;
        if (int rc = in.pcm ? h->s_pcm.reserve((size_t)k.C * ds) : h->s_mfcc.reserve((size_t)k.C * ds)) return rc;
        if (int rc = out.reserve()) return rc;
        uint8_t *d_in = in.pcm ? (uint8_t *)h->s_pcm.p : (uint8_t *)h->s_mfcc.p;
        for (uint32_t c = 0; c < k.C; c++) {  // count by count: nothing past n[c] of a caller's row is read
            const size_t cnt = in.pcm ? pl.chan[c].n_samp : pl.chan[c].n;
            if (cnt) COPY_UP(d_in + c * ds * 2, (const uint8_t *)in.p + (size_t)c * in.stride * 2, cnt * per * 2);
        }
        const auto into_out = [&](const int16_t *f, uint64_t rs, hipStream_t s) { return launch(out, f, rs, s); };
        if (int rc = k.enqueue(pl, LiveIn{d_in, ds, in.pcm}, nullptr, into_out)) return rc;
    }
    advance();
    if (work)
        if (int rc = k.mark_push(nullptr)) return rc;
    return out.down();
}

// ---- the decoders' outputs: a record, max_words word rows and (level sessions) max_words level costs per row ----------------
// store(): what the trace will read of the engine -- its store, its word map -- is fit for it (check_chain, where the session
// has not lost its recordings anyway)
template <typename Store>
int check_outputs(uint32_t max_words, uint32_t n_out, uint32_t max_rows, const sr_chain_rec *rec, const sr_chain_word *words,
                  const uint32_t *level_cost, const sr_chain_live_row *rows, Store &&store)
{
    if (max_rows < n_out)
        return fail(SR_ERR_BAD_ARG, "max_rows " + std::to_string(max_rows) + " is below the " + std::to_string(n_out) + " rows of this call");
    if (!n_out) return SR_OK;
    if (int rc = store()) return rc;
    if (!rec || !words || !rows) return fail(SR_ERR_BAD_ARG, "null argument");
    const size_t n_rec = (size_t)n_out * sizeof *rec, n_w = (size_t)n_out * max_words * sizeof *words, n_lc = (size_t)n_out * max_words * 4;
    if (overlap(rec, n_rec, words, n_w) || overlap(rec, n_rec, level_cost, n_lc) || overlap(words, n_w, level_cost, n_lc))
        return fail(SR_ERR_BAD_ARG, "rec, words and level_cost overlap");
    return SR_OK;
}

// an end call: every output is a host buffer there, so the labels must not lie inside the records either
inline int check_end_rows(uint32_t max_words, uint32_t n_out, const sr_chain_rec *rec, const sr_chain_word *words, const uint32_t *level_cost,
                          const sr_chain_live_row *rows)
{
    const size_t n_r = (size_t)n_out * sizeof *rows, n_w = (size_t)n_out * max_words;
    if (overlap(rows, n_r, rec, (size_t)n_out * sizeof *rec) || overlap(rows, n_r, words, n_w * sizeof *words) ||
        overlap(rows, n_r, level_cost, n_w * 4))
        return fail(SR_ERR_BAD_ARG, "rows overlaps rec, words or level_cost");
    return SR_OK;
}

// A push of a decoder in any of its four forms, after the session has planned it and checked its inputs and outputs: a push
// enqueues work when a channel emits a row.  launch(features, row stride, rec, words, level_cost, s) is the session's launch
// into device pointers: the caller's own (device forms) or the per-call copies (host forms).
template <typename Launch, typename Advance>
int live_push_chain(LiveCore &k, const LivePlan &pl, const LiveIn &in, bool device, void *stream, uint32_t max_words, sr_chain_rec *rec,
                    sr_chain_word *words, uint32_t *level_cost, Launch &&launch, Advance &&advance)
{
    if (device)
        return live_push_dev(k, pl, pl.rows != 0, in, stream,
                             [&](const int16_t *f, uint64_t rs, hipStream_t s) { return launch(f, rs, rec, words, level_cost, s); }, advance);
    return live_push_host(k, pl, pl.rows != 0, in, [&] { return HostOutputs(pl.rows, max_words, rec, words, level_cost); },
                          [&](HostOutputs &o, const int16_t *f, uint64_t rs, hipStream_t s) { return launch(f, rs, o.rec.p, o.words.p, o.lc.p, s); },
                          advance);
}

// An end call of a decoder, after its list (chan, order) and its checks: wait for the last push, trace the listed channels
// into per-call device copies of the outputs, copy down, reset, label.  prepare(): what must be in place before anything is
// written (a relayout that may fail); trace(rec, words, level_cost): the session's trace launch into the copies; reset(): the
// listed channels are as freshly opened.
template <typename Prepare, typename Trace, typename Reset>
int live_end(LiveCore &k, const std::vector<SpotLiveChan> &chan, const std::vector<sr_chain_live_row> &order, uint32_t max_words,
             sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost, sr_chain_live_row *rows, uint32_t *n_rows, Prepare &&prepare,
             Trace &&trace, Reset &&reset)
{
    const uint32_t n_out = (uint32_t)order.size();
    if (!n_out) {
        if (n_rows) *n_rows = 0;
        return SR_OK;
    }
    ENTER_HOST_CALL(k.h);
    if (int rc = k.wait_last()) return rc;
    HostOutputs o(n_out, max_words, rec, words, level_cost);
    if (int rc = o.reserve()) return rc;
    if (int rc = prepare()) return rc;
    if (int rc = k.upload_chan(chan, nullptr)) return rc;
    trace(o.rec.p, o.words.p, o.lc.p);
    HIP_TRY(hipGetLastError());
    if (int rc = o.down()) return rc;
    reset();
    for (uint32_t r = 0; r < n_out; r++) rows[r] = order[r];
    if (n_rows) *n_rows = n_out;
    return SR_OK;
}

}  // namespace sr
