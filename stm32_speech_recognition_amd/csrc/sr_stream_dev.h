// sr_stream_dev.h -- the endpoint state machine of the stream VAD (VAD.C:164-216) and the frame count of a segment
// (MFCC.C:102-107), shared by the one-shot scan (k_vad_stream.hip) and the live session (k_live.hip).
#pragma once
#include "sr_vad_dev.h"

namespace sr {

// the endpoint state machine (VAD.C:164-216) with the counters folded into one state number:
//   0 silence | 1..nF onset, front = s | sp = nF + 1 speech | sp + 1 .. sp + nB tail, back = s - sp
struct StreamSm {
    uint32_t nF, sp, v_durmin, s_durmax;
    // one frame; ev: 1 = a segment starts at this frame (VAD.C:175-180), 2 = one ends (VAD.C:198-207)
    __device__ __forceinline__ uint32_t step(uint32_t s, bool loud, uint32_t &ev) const
    {
        ev = 0;
        if (s == 0) return loud ? 1u : 0u;
        if (s <= nF) {  // front++ is checked on loud frames only, after the increment (VAD.C:173-181)
            if (!loud) return 0u;
            if (s + 1 >= v_durmin) {
                ev = 1;
                return sp;
            }
            return s + 1;
        }
        if (s == sp) return loud ? sp : sp + 1;
        if (loud) return sp;  // a loud frame returns to speech (VAD.C:186-190)
        const uint32_t back = s - sp + 1;
        if (back >= s_durmax) {
            ev = 2;
            return 0u;
        }
        return sp + back;
    }
};

// frm_num per k_select_segment (k_vad.hip) / MFCC.C:102-107: 0 for an open end or a start < 1
__device__ __forceinline__ uint32_t stream_frm_num(int st, int en, uint32_t frame_len, uint32_t hop, uint32_t max_frames)
{
    if (en < 0 || st < 1) return 0;
    const uint32_t n = ((((uint32_t)(en - st) - frame_len) / hop) + 1) & 0xFFFF;
    return n > max_frames ? 0u : n;
}

}  // namespace sr
