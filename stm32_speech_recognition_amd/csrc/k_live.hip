// k_live.hip -- live sessions: audio that arrives in chunks, the stream VAD's state carried from one push to the next.
// EXTENSION, NO REFERENCE COUNTERPART, like stream recognition (k_vad_stream.hip), whose per-block and per-frame arithmetic
// (sr_vad_dev.h) and endpoint state machine (sr_stream_dev.h) these kernels share.  The entering state of every channel is
// KNOWN, so none of the one-shot scan's tables over every possible entering state are needed.
// gfx950 (MI355X, CDNA4) only; wave = 64 lanes; integer VALU.
//
//   k_live_append   one workgroup per channel: the chunk copied in behind the channel's last sample.  The history is a ring of
//                   whole hop-sized blocks indexed by absolute block number modulo its capacity; a 16-byte vector at an
//                   absolute position that is a multiple of 8 never straddles the wrap (the capacity is a multiple of 8).
//   k_live_scan     one wave per channel: the new whole frames in rounds of 64 blocks -- block summaries, the last-class
//                   prefix seeded with the carried class, the loud bit of VAD.C:164 as k_stream_tiles forms it, a ballot,
//                   StreamSm::step over the mask -- END events into the channel's bounded slots, the state written back.
//   k_live_compact  one workgroup: exclusive offsets of the per-channel counts in channel order, the events written out as
//                   sr_live_seg records, the total.  Deterministic: no atomics, no inter-workgroup flags.
//   k_live_records  the ring-aware k_stream_records: every ended segment copied, with its lead, into a row of its own.
#include "sr_stream_dev.h"

namespace sr {

constexpr int kLiveAppendThreads = 128, kLiveWaves = 4, kLiveCompactThreads = 1024;

__device__ __forceinline__ uint32_t live_count(const LiveArgs &a, uint32_t c) { return a.n ? a.n[c] : a.n_all; }

// ---- append ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kLiveAppendThreads) k_live_append(const LiveArgs a)
{
    const uint32_t c = blockIdx.x;
    const uint32_t n = live_count(a, c);
    if (!n) return;
    const uint64_t p0 = a.chan[c].received, p1 = p0 + n;  // absolute positions [p0, p1) are written
    const uint16_t *src = a.pcm + (uint64_t)c * a.pcm_stride;
    uint16_t *ring = a.ring + (uint64_t)c * a.ring_stride;
    uint64_t a0 = (p0 + 7) & ~7ull, a1 = p1 & ~7ull;  // the 16-byte aligned part of the destination
    if (a0 > a1) a0 = a1 = p1;                         // the chunk lies inside one vector: edges only
    // edges: plain 2-byte stores
    for (uint64_t p = p0 + threadIdx.x; p < a0; p += blockDim.x) ring[p % a.ring_stride] = src[p - p0];
    for (uint64_t p = a1 + threadIdx.x; p < p1; p += blockDim.x) ring[p % a.ring_stride] = src[p - p0];
    const bool src_aligned = ((a0 - p0) & 7) == 0;  // rows are 16-byte aligned: source vectors are too when p0 is a multiple of 8
    for (uint64_t p = a0 + 8ull * threadIdx.x; p < a1; p += 8ull * blockDim.x) {
        const uint16_t *q = src + (p - p0);
        uint4 v;
        if (src_aligned) {
            v = *(const uint4 *)q;
        } else {
            v.x = q[0] | (uint32_t)q[1] << 16;
            v.y = q[2] | (uint32_t)q[3] << 16;
            v.z = q[4] | (uint32_t)q[5] << 16;
            v.w = q[6] | (uint32_t)q[7] << 16;
        }
        *(uint4 *)(ring + p % a.ring_stride) = v;
    }
}

// ---- scan --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uniform64(uint64_t v) { return (uint64_t)uniform((uint32_t)v) | (uint64_t)uniform((uint32_t)(v >> 32)) << 32; }

template <int kFrameLen, int kHop, bool kSad>
__global__ void __launch_bounds__(64 * kLiveWaves) k_live_scan(const LiveArgs a)
{
    const int lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.x * kLiveWaves + (threadIdx.x >> 6);
    if (c >= a.C) return;
    LiveChan *st = a.chan + c;
    const uint64_t recv = uniform64(st->received) + live_count(a, c);
    sr_atap at = st->atap;
    uint32_t set = uniform(st->atap_set);
    if (!set && recv >= a.noise_len) {  // the noise head became complete in this push: k_vad has just run over it
        at = a.head_vad[c - a.head_c0].atap;
        set = 1;
    }
    uint64_t j0 = uniform64(st->next_frame);
    // frame j is consumed once MORE than j * hop + frame_len samples are there: the loop bound of VAD.C:121
    const uint64_t F = (set && recv > (uint64_t)kFrameLen) ? (recv - kFrameLen + kHop - 1) / kHop : 0;
    uint32_t s = uniform(st->state), carry = uniform(st->carry), nev = 0;
    int64_t open_start = (int64_t)uniform64((uint64_t)st->open_start);

    const uint32_t mid = at.mid_val, n_thl = at.n_thl, z_thl = at.z_thl, s_thl = at.s_thl;
    const uint32_t a_thl = mid + n_thl, b_thl = mid - n_thl;  // VAD.C:112-113 (u32, may wrap)
    const uint32_t mid2 = (mid & 0xFFFFu) * 0x10001u;
    const uint32_t nF = (a.v_durmin > 2 ? a.v_durmin : 2u) - 1;
    const StreamSm sm{nF, nF + 1, a.v_durmin, a.s_durmax};
    const uint16_t *ring = a.ring + (uint64_t)c * a.ring_stride;
    LiveEvent *ev_out = a.events + (uint64_t)c * a.ev_slots;

    for (uint64_t jb = j0; jb < F; jb += 63) {
        const uint64_t j = jb + lane;  // block index; frame j uses blocks j and j + 1, each wrapping on its own
        uint32_t A = 0, internal = 0, last = 0, cf = 0, c78 = 0;
        int pfo = -1;
        if (j <= F)
            vad_block_summary<kHop, kSad>((const uint4 *)(ring + (uint64_t)(uint32_t)(j % a.ring_blocks) * kHop), mid, mid2, a_thl, b_thl, A,
                                          internal, last, cf, c78, pfo);
        // R = class of the last out-of-band sample in blocks <= j, the carried class included
        uint32_t R = last;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(R, d, 64);
            if (lane >= d) R = R ? R : o;
        }
        R = R ? R : carry;
        uint32_t Rprev = __shfl_up(R, 1, 64);
        if (lane == 0) Rprev = carry;
        const uint32_t nfr = (F - jb < 63u) ? (uint32_t)(F - jb) : 63u;  // frames of this round
        carry = __shfl(R, (int)nfr - 1, 64);                            // through block jb + nfr - 1
        // the loud bit exactly as k_stream_tiles forms it (its P0 = this lane's block, P1 = the next lane's)
        const uint32_t in1 = __shfl_down(internal, 1, 64), cf1 = __shfl_down(cf, 1, 64), A1 = __shfl_down(A, 1, 64);
        const uint32_t ff0 = (cf != 0 && Rprev != 0 && Rprev != cf) ? 1u : 0u;
        const uint32_t ff1 = (cf1 != 0 && R != 0 && R != cf1) ? 1u : 0u;
        uint32_t Z = internal + in1 + ff1;
        if (pfo < 0 || pfo == kHop - 1) Z += ff0;
        else if (pfo > 0 && j > 0) Z += (c78 != cf) ? 1u : 0u;  // the ABSOLUTE frame index: frame 0 starts with last_sig = 0
        const bool loud = (lane < 63) && (j < F) && (A + A1 > s_thl || Z > z_thl);  // VAD.C:164
        const uint64_t mask = __ballot(loud);
        if (s == 0 && mask == 0) continue;  // silence stays silence
        for (uint32_t k = 0; k < nfr; k++) {
            uint32_t ev;
            s = sm.step(s, (mask >> k) & 1u, ev);
            const int64_t i = (int64_t)(jb + k) * kHop;
            if (ev == 1) {
                open_start = i - (int64_t)(a.v_durmin - 1) * kHop;  // VAD.C:178
            } else if (ev == 2) {
                if (lane == 0 && nev < a.ev_slots) ev_out[nev] = LiveEvent{open_start, i - (int64_t)a.s_durmax * kHop + kFrameLen};  // VAD.C:201
                nev++;
            }
        }
    }
    if (lane == 0) {
        st->atap = at;
        st->atap_set = set;
        st->carry = carry;
        st->state = s;
        st->next_frame = F > j0 ? F : j0;
        st->open_start = open_start;
        st->received = recv;
        a.ev_count[c] = nev < a.ev_slots ? nev : a.ev_slots;
    }
}

// ---- count, offsets, compaction ----------------------------------------------------------------------------------------
// frm_num of a live segment: stream_frm_num on 64-bit offsets, WITHOUT the u16 wrap of MFCC.C:102 -- a segment of 65 536
// frames or more fails like every other one above max_frames (its head has left the ring; include/sr_engine.h)
__device__ __forceinline__ uint32_t live_frm_num(int64_t st, int64_t en, uint32_t frame_len, uint32_t hop, uint32_t max_frames)
{
    if (en < 0 || st < 1) return 0;
    const uint64_t n = ((uint64_t)(en - st) - frame_len) / hop + 1;
    return n > max_frames ? 0u : (uint32_t)n;
}

__global__ void __launch_bounds__(kLiveCompactThreads) k_live_compact(const LiveArgs a)
{
    __shared__ uint32_t s_w[kLiveCompactThreads / 64];
    __shared__ uint32_t s_base;
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < a.C; c0 += kLiveCompactThreads) {
        const uint32_t c = c0 + tid;
        const uint32_t count = c < a.C ? a.ev_count[c] : 0u;
        uint32_t incl = count;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, 64);
            if ((int)lane >= d) incl += o;
        }
        if (lane == 63) s_w[w] = incl;
        __syncthreads();
        uint32_t wbase = s_base;
        for (uint32_t i = 0; i < w; i++) wbase += s_w[i];
        const uint32_t off = wbase + incl - count;
        for (uint32_t e = 0; e < count; e++) {
            const LiveEvent g = a.events[(uint64_t)c * a.ev_slots + e];
            if (off + e < a.max_segs)
                a.segs[off + e] = sr_live_seg{c, live_frm_num(g.start, g.end, a.frame_len, a.hop, a.max_frames), g.start, g.end};
        }
        __syncthreads();
        if (tid == kLiveCompactThreads - 1) s_base = wbase + incl;
        __syncthreads();
    }
    if (tid == 0) a.count[0] = s_base;
}

// ---- recognition records -----------------------------------------------------------------------------------------------
// k_stream_records over the ring: record r0 + i -> an sr_vad_rec for the frame / DTW kernels and the segment's samples in a
// row of its own, seg[0] = kStreamLead.  Records at or past the total are padding: SR_ST_VAD_FAIL.
__global__ void __launch_bounds__(256) k_live_records(const LiveRecArgs a)
{
    const uint32_t i = blockIdx.x, r = a.r0 + i;
    const uint32_t total = a.count[0];
    int64_t st = -1, en = -1;
    uint32_t ch = 0;
    if (r < total) {
        const sr_live_seg g = a.segs[r];
        st = g.start;
        en = g.end;
        ch = g.channel;
    }
    uint32_t status, frm = 0;
    if (en < 0) {
        status = SR_ST_VAD_FAIL;
    } else if (st < 1) {
        status = SR_ST_SEG_OOB;
    } else {
        frm = live_frm_num(st, en, a.frame_len, a.hop, a.max_frames);
        status = frm ? SR_ST_OK : SR_ST_MFCC_FAIL;
    }
    if (threadIdx.x == 0) {
        sr_vad_rec *o = a.recs + i;
        o->atap = (r < total) ? a.chan[ch].atap : sr_atap{0, 0, 0, 0};
        o->seg[0] = (int)kStreamLead;
        o->seg[1] = status == SR_ST_OK ? (int)kStreamLead + (int)(en - st) : (en < 0 ? -1 : (int)kStreamLead);
#pragma unroll
        for (int q = 2; q < 2 * SR_MAX_SEG; q++) o->seg[q] = -1;
        o->frm_num = frm;
        o->status = status;
        o->_pad = 0;
    }
    if (status != SR_ST_OK) return;
    // samples [st - kStreamLead, st + (frm + 1) * hop): st is a multiple of hop (>= hop >= 80), so every 16-byte vector of
    // the copy starts at an absolute position that is a multiple of 8 and lies inside one turn of the ring
    const uint16_t *ring = a.ring + (uint64_t)ch * a.ring_stride;
    uint4 *dst = (uint4 *)(a.rows + (uint64_t)i * a.row_stride);
    const uint64_t p0 = (uint64_t)st - kStreamLead;
    const uint32_t nv = (kStreamLead + (frm + 1) * a.hop) / 8;
    for (uint32_t v = threadIdx.x; v < nv; v += blockDim.x) dst[v] = *(const uint4 *)(ring + (p0 + 8ull * v) % a.ring_stride);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
void launch_live_append(const LiveArgs &a, hipStream_t s)
{
    if (!a.C) return;
    SR_LAUNCH_POINT(s, "k_live_append");
    hipLaunchKernelGGL(k_live_append, dim3(a.C), dim3(kLiveAppendThreads), 0, s, a);
}

template <int FL>
static void launch_scan_fl(const LiveArgs &a, bool sad, hipStream_t s)
{
    const dim3 grid((a.C + kLiveWaves - 1) / kLiveWaves), block(64 * kLiveWaves);
    if (sad) {
        SR_LAUNCH_POINT(s, "k_live_scan");
        hipLaunchKernelGGL((k_live_scan<FL, FL / 2, true>), grid, block, 0, s, a);
    } else {
        SR_LAUNCH_POINT(s, "k_live_scan");
        hipLaunchKernelGGL((k_live_scan<FL, FL / 2, false>), grid, block, 0, s, a);
    }
}

void launch_live_scan(const LiveArgs &a, bool sad, hipStream_t s)
{
    if (!a.C) return;
    switch (a.frame_len) {
    case 160: launch_scan_fl<160>(a, sad, s); break;
    case 240: launch_scan_fl<240>(a, sad, s); break;
    case 256: launch_scan_fl<256>(a, sad, s); break;
    case 320: launch_scan_fl<320>(a, sad, s); break;
    case 400: launch_scan_fl<400>(a, sad, s); break;
    case 512: launch_scan_fl<512>(a, sad, s); break;
    default: return;  // sr_create accepts only the framings of vad_framing_supported
    }
    SR_LAUNCH_POINT(s, "k_live_compact");
    hipLaunchKernelGGL(k_live_compact, dim3(1), dim3(kLiveCompactThreads), 0, s, a);
}

void launch_live_records(const LiveRecArgs &a, uint32_t n, hipStream_t s)
{
    if (!n) return;
    SR_LAUNCH_POINT(s, "k_live_records");
    hipLaunchKernelGGL(k_live_records, dim3(n), dim3(256), 0, s, a);
}

}  // namespace sr
