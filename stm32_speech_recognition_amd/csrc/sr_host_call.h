// Transport of the host-buffer entry points (sr_host.cpp, sr_stream.cpp, sr_nbest.cpp): how a caller's host buffers reach
// the engine's scratch in HBM and how results come back.  HOST ONLY: no k_*.hip unit includes this header.
//
// A host-buffer call is "what goes up, the launches, what comes back".  HostCall carries the first and the last part in one
// of two modes, so that the entry point writes its launch sequence ONCE, on hc.stream():
//
//   blocking  hipMemcpy / hipMemcpy2D on the null stream, each waiting for itself; finish() has nothing left to do.
//   pinned    small calls (spch_recg / get_mfcc / VAD / dtw: one capture, one record).  What goes up is staged in the first
//             part of the engine's pinned area, what comes back lands in its second part (result records can be written
//             there by the kernel itself, land()); every copy is asynchronous on the internal stream st_comp and the host
//             waits ONCE, in finish(), which then hands the landed blocks to the caller's buffers.
//
// Invariants (every entry point ends in `return hc.finish(rc)`, which is what keeps them):
//   * once anything has been enqueued on st_comp the call does not return before that stream has been synchronised, on
//     failure too -- the caller's buffers and the engine's scratch are free again when the call returns;
//   * a failed launch, copy or synchronisation yields SR_ERR_HIP, a failing *_dev sub-call its own code;
//   * where both a sub-call and the synchronisation fail, the sub-call's code wins (finish(rc) returns rc first);
//   * after the first failure nothing more is enqueued: every step of an entry point is guarded by `if (!rc)`.
#pragma once
#include "sr_engine_internal.h"

namespace sr {

// ENTER_DEVICE for an entry point that works on the engine's scratch buffers from the null stream or st_comp: those run
// behind the last asynchronous *_dev call that used the scratch on a caller's stream
#define ENTER_HOST_CALL(h) \
    ENTER_DEVICE(h);       \
    if (int rc_ord_ = order_after_scratch_users((h), nullptr)) return rc_ord_

// blocking copies of the null stream: host buffer -> device, device -> host buffer
#define COPY_UP(dev, src, bytes) HIP_TRY(hipMemcpy((dev), (src), (bytes), hipMemcpyHostToDevice))
#define COPY_DOWN(dst, dev, bytes) HIP_TRY(hipMemcpy((dst), (dev), (bytes), hipMemcpyDeviceToHost))

// samples between capture rows in s_pcm: rows start 16-byte aligned
static inline uint64_t dev_pitch(uint32_t buf_len) { return ((uint64_t)buf_len + 7) & ~7ull; }

// B rows of buf_len samples at pcm_stride -> s_pcm at the device pitch, one blocking 2-D copy
static inline int stage_pcm(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B, uint64_t *dev_stride)
{
    const uint64_t ds = dev_pitch(buf_len);
    if (int rc = h->s_pcm.reserve((size_t)B * ds)) return rc;
    HIP_TRY(hipMemcpy2D(h->s_pcm.p, ds * 2, pcm, pcm_stride * 2, (size_t)buf_len * 2, B, hipMemcpyHostToDevice));
    *dev_stride = ds;
    return SR_OK;
}

// ---- the pinned area -----------------------------------------------------------------------------------------------------
static constexpr size_t kPinUpload = 256 * 1024, kPinMaxB = 256;           // captures of one small call; utterances
static constexpr size_t kPinUpBytes = kPinUpload + 64 * 1024;             // + records / frame counts / thresholds
static constexpr size_t kPinDownBytes = 704 * 1024, kPinTotal = kPinUpBytes + kPinDownBytes;
static constexpr size_t kPinMfccBytes = 512 * 1024;

// false = no pinned area on this host (allocation refused: the callers keep their blocking copies)
static inline bool ensure_pin(sr_engine *h)
{
    if (h->pin_cap < kPinTotal) {
        if (h->pin_failed) return false;
        if (hipHostMalloc(&h->pin_buf, kPinTotal, hipHostMallocMapped) != hipSuccess) {
            (void)hipGetLastError();
            h->pin_buf = nullptr;
            h->pin_failed = true;
            return false;
        }
        h->pin_cap = kPinTotal;
    }
    if (!h->st_comp && hipStreamCreateWithFlags(&h->st_comp, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        h->st_comp = nullptr;
        return false;
    }
    return true;
}

// Which calls take the pinned mode.  Common to all six: small-launch mode != 1, every block rounded up to 64 bytes (the
// allowance of 64 per block) inside its part of the area, and the area exists.  ds = dev_pitch(buf_len); the entry point
// tests its own column first, pin_fits last (it is the one that allocates):
//
//   entry point            its own condition                         goes up (blocks)                      comes back (blocks)
//   recognize_host         !packed, !profiling, B <= kPinMaxB        B*ds*2 (1)                            B*sizeof(sr_result) (1)
//   sr_vad_batch           B <= kPinMaxB                             B*ds*2 (1)                            B*sizeof(sr_vad_rec) (1)
//   sr_mfcc_batch_status   B <= kPinMaxB, mbytes <= kPinMfccBytes    B*(ds*2 + sizeof(sr_vad_rec)) (2)     mbytes (1)
//   sr_dtw_batch           -                                         records + B*4 (2)                     scores + results (2)
//   engine_vad_with_atap   -                                         ds*2 + sizeof(sr_atap) (2)            sizeof(sr_vad_rec) (1)
//   engine_noise_atap      -                                         ds*2 (1)                              sizeof(sr_vad_rec) (1)
static inline bool pin_fits(sr_engine *h, size_t up_bytes, size_t down_bytes, uint32_t n_up = 1, uint32_t n_down = 1)
{
    return h->small_launch != 1 && up_bytes + 64 * (size_t)n_up <= kPinUpBytes && down_bytes + 64 * (size_t)n_down <= kPinDownBytes &&
           ensure_pin(h);
}

class HostCall {
public:
    // pinned = the entry point's row of the table above held.  The internal stream is non-blocking: it is ordered explicitly
    // behind the last asynchronous call that used the scratch buffers on a caller's stream.
    HostCall(sr_engine *e, bool pinned) : h(e), base(pinned ? (uint8_t *)e->pin_buf : nullptr)
    {
        if (base) err = order_after_scratch_users(e, e->st_comp);
    }
    HostCall(const HostCall &) = delete;

    hipStream_t stream() const { return base ? h->st_comp : nullptr; }  // where the entry point launches

    int put(void *dev, const void *src, size_t bytes)  // host buffer -> device
    {
        if (!base) {
            COPY_UP(dev, src, bytes);
            return SR_OK;
        }
        uint8_t *p = take(up, kPinUpBytes, bytes);
        if (!p) return err;
        std::memcpy(p, src, bytes);
        return async(hipMemcpyAsync(dev, p, bytes, hipMemcpyHostToDevice, h->st_comp));
    }
    // B capture rows of buf_len samples -> s_pcm at the device pitch (samples, *dev_stride), the pad of a staged row zeroed
    int put_rows(const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B, uint64_t *dev_stride)
    {
        if (!base) return stage_pcm(h, pcm, pcm_stride, buf_len, B, dev_stride);
        const uint64_t ds = dev_pitch(buf_len);
        const size_t row = (size_t)buf_len * 2, pitch = (size_t)ds * 2;
        if (err || (err = h->s_pcm.reserve((size_t)B * ds))) return err;
        uint8_t *st = take(up, kPinUpBytes, (size_t)B * pitch);
        if (!st) return err;
        for (uint32_t b = 0; b < B; b++) {
            std::memcpy(st + b * pitch, (const uint8_t *)pcm + (size_t)b * pcm_stride * 2, row);
            if (pitch > row) std::memset(st + b * pitch + row, 0, pitch - row);
        }
        *dev_stride = ds;
        return async(hipMemcpyAsync(h->s_pcm.p, st, (size_t)B * pitch, hipMemcpyHostToDevice, h->st_comp));
    }
    int get(void *dst, const void *dev, size_t bytes)  // device -> host buffer (pinned: dst is written in finish())
    {
        if (!base) {
            COPY_DOWN(dst, dev, bytes);
            return SR_OK;
        }
        uint8_t *p = landed(dst, bytes);
        if (!p) return err;
        return async(hipMemcpyAsync(p, dev, bytes, hipMemcpyDeviceToHost, h->st_comp));
    }
    // pinned mode only: a landing block the kernels write themselves, through the device pointer *dev; dst as get()
    int land(void *dst, size_t bytes, void **dev)
    {
        uint8_t *p = landed(dst, bytes);
        if (!p) return err;
        return async(hipHostGetDevicePointer(dev, p, 0));
    }
    // rc = how the entry point's steps went.  Pinned: the one synchronisation of the call, then the landed blocks go to the
    // caller's buffers.  Blocking: nothing is outstanding.
    int finish(int rc)
    {
        if (!base) return rc;
        const hipError_t e = hipStreamSynchronize(h->st_comp);
        if (e != hipSuccess) (void)hipGetLastError();
        if (rc) return rc;
        if (err) return err;
        if (e != hipSuccess) return fail(SR_ERR_HIP, std::string("small host call: synchronisation failed: ") + hipGetErrorString(e));
        for (uint32_t i = 0; i < n_out; i++) std::memcpy(out[i].dst, out[i].src, out[i].bytes);
        return SR_OK;
    }

private:
    struct Out { void *dst; const uint8_t *src; size_t bytes; };  // a landed block and the caller's buffer it goes to
    static constexpr uint32_t kMaxOut = 4;
    sr_engine *h;
    uint8_t *base;  // the pinned area; nullptr = blocking mode
    size_t up = 0, down = kPinUpBytes;
    int err = SR_OK;  // first failure of the transport itself (sticky: nothing more is enqueued after it)
    Out out[kMaxOut];
    uint32_t n_out = 0;

    // bump allocation in [at, end) of the area, blocks rounded up to 64 bytes.  The entry points check their sizes beforehand
    // (pin_fits), so running out means that a condition and the blocks its call takes have drifted apart: an error, never an overrun.
    uint8_t *take(size_t &at, size_t end, size_t bytes)
    {
        const size_t rounded = (bytes + 63) & ~(size_t)63;
        if (!err && (!base || rounded > end - at)) err = fail(SR_ERR_HIP, "small host call: no room in the pinned area");
        if (err) return nullptr;
        at += rounded;
        return base + at - rounded;
    }
    uint8_t *landed(void *dst, size_t bytes)
    {
        if (!err && n_out == kMaxOut) err = fail(SR_ERR_HIP, "small host call: too many landing blocks");
        uint8_t *p = take(down, kPinTotal, bytes);
        if (p) out[n_out++] = Out{dst, p, bytes};
        return p;
    }
    int async(hipError_t e)
    {
        if (e == hipSuccess) return SR_OK;
        (void)hipGetLastError();
        return err = fail(SR_ERR_HIP, std::string("small host call: ") + hipGetErrorString(e));
    }
};

}  // namespace sr
