// k_vad_stream.hip -- VAD (VAD.C:97-218) with max_vc_con unbounded over recordings of any length, as a scan over tiles of
// T frames in three launches, and the per-segment record builder of stream recognition.
// EXTENSION, NO REFERENCE COUNTERPART: the firmware stops after max_vc_con = 3 segments (VAD.H:4, VAD.C:203) of a u16-long
// buffer.  The arithmetic per block and per frame is k_vad's (sr_vad_dev.h), whose comments explain the block algebra.
// gfx950 (MI355X, CDNA4) only; wave = 64 lanes; integer VALU.
//
//   pass 1  k_stream_tiles   one wave per tile: the samples are read once.  Per frame the "loud" bit of VAD.C:164 for each of
//                            the three values the carried last_sig can have on entry (0, 1, 2: only the frames up to the
//                            tile's first out-of-band sample depend on it), then for every (carry in, state in) pair the
//                            endpoint state machine over the tile: state out, carry out, segment starts, last start.
//   pass 2  k_stream_scan    one workgroup: per recording the tile tables composed in order (each tile's true entering
//                            carry, state, segment index and the start of the segment open on entry), then the exclusive
//                            sum of the per-recording counts over B.  Deterministic: no atomics, no inter-workgroup flags.
//   pass 3  k_stream_emit    one lane per tile: the tile's frames replayed from its entering state; every END event writes
//                            the whole record (start from the replay or from the scan), as does the end of a recording that
//                            ends inside a segment (end = -1).  Each record is written by exactly one lane.
#include "sr_stream_dev.h"  // StreamSm, stream_frm_num (shared with k_live.hip)

namespace sr {

__device__ __forceinline__ StreamSm stream_sm(const VadStreamArgs &a)
{
    return StreamSm{a.n_front, a.n_front + 1, a.v_durmin, a.s_durmax};
}
__device__ __forceinline__ uint32_t stream_frames(const VadStreamArgs &a, uint32_t b)
{
    uint32_t S = a.len ? a.len[b] : a.buf_len;
    S = S < a.buf_len ? S : a.buf_len;
    return S > a.frame_len ? (S - a.frame_len + a.hop - 1) / a.hop : 0u;  // VAD.C:121
}
__device__ __forceinline__ sr_atap stream_atap(const VadStreamArgs &a, uint32_t b)
{
    return *(const sr_atap *)(a.atap_src + (uint64_t)b * a.atap_src_stride);
}

// ---- pass 1 ------------------------------------------------------------------------------------------------------------
// LDS per tile: the summaries of its T + 1 blocks (block T is the next tile's first: frame T-1 reads it) and its loud masks.
template <int kFrameLen, int kHop, bool kSad>
__global__ void __launch_bounds__(64) k_stream_tiles(const VadStreamArgs a)
{
    __shared__ uint32_t s_A[kStreamTileMax + 1], s_P[kStreamTileMax + 1];
    __shared__ uint32_t s_mask[3][kStreamTileMax / 32];
    const int lane = threadIdx.x;
    const uint32_t tile = blockIdx.x, b = tile / a.nt, t = tile - b * a.nt;
    const uint32_t F = stream_frames(a, b), T = a.tile_frames, j0 = t * T;
    if (j0 >= F) return;
    const uint4 *row = (const uint4 *)(a.pcm + (uint64_t)b * a.pcm_stride);
    const sr_atap at = stream_atap(a, b);
    const uint32_t mid = at.mid_val, n_thl = at.n_thl, z_thl = at.z_thl, s_thl = at.s_thl;
    const uint32_t a_thl = mid + n_thl, b_thl = mid - n_thl;  // VAD.C:112-113 (u32, may wrap)
    const uint32_t mid2 = (mid & 0xFFFFu) * 0x10001u;

    // block summaries; Rloc(k) = class of the last out-of-band sample in the tile's blocks 0..k (0: none yet)
    //   s_P: internal (9 bits) | last << 9 | cf << 11 | c78 << 13 | Rloc << 15 | (pfo + 1) << 17
    uint32_t rcarry = 0;
    for (uint32_t k0 = 0; k0 <= T; k0 += 64) {
        const uint32_t k = k0 + lane, j = j0 + k;
        uint32_t A = 0, internal = 0, last = 0, cf = 0, c78 = 0;
        int pfo = -1;
        if (k <= T && j <= F) vad_block_summary<kHop, kSad>(row + (uint64_t)j * (kHop / 8), mid, mid2, a_thl, b_thl, A, internal, last, cf, c78, pfo);
        uint32_t R = last;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(R, d, 64);
            if (lane >= d) R = R ? R : o;
        }
        R = R ? R : rcarry;
        rcarry = __shfl(R, 63, 64);
        if (k <= T) {
            s_A[k] = A;
            s_P[k] = internal | last << 9 | cf << 11 | c78 << 13 | R << 15 | (uint32_t)(pfo + 1) << 17;
        }
    }
    __syncthreads();

    // loud bits per frame for carry-in c = 0, 1, 2 (k_vad's frame rule, sr_vad_dev.h)
    const uint32_t nw = (T + 31) / 32;
    for (uint32_t k0 = 0; k0 < T; k0 += 64) {
        const uint32_t k = k0 + lane, j = j0 + k;
        uint32_t loud3 = 0;
        if (k < T && j < F) {
            const uint32_t P0 = s_P[k], P1 = s_P[k + 1], Pm = k ? s_P[k - 1] : 0u;
            const uint32_t in0 = P0 & 511, cf0 = (P0 >> 11) & 3, c780 = (P0 >> 13) & 3, R0 = (P0 >> 15) & 3;
            const int pfo0 = (int)(P0 >> 17) - 1;
            const uint32_t in1 = P1 & 511, cf1 = (P1 >> 11) & 3, Rm = (Pm >> 15) & 3;
            const uint32_t frm_sum = s_A[k] + s_A[k + 1];
#pragma unroll
            for (uint32_t c = 0; c < 3; c++) {
                const uint32_t Rp = Rm ? Rm : c, Rk = R0 ? R0 : c;  // class before block k / before block k + 1
                const uint32_t ff0 = (cf0 != 0 && Rp != 0 && Rp != cf0) ? 1u : 0u;
                const uint32_t ff1 = (cf1 != 0 && Rk != 0 && Rk != cf1) ? 1u : 0u;
                uint32_t Z = in0 + in1 + ff1;
                if (pfo0 < 0 || pfo0 == kHop - 1) Z += ff0;
                else if (pfo0 > 0 && j > 0) Z += (c780 != cf0) ? 1u : 0u;
                if (frm_sum > s_thl || Z > z_thl) loud3 |= 1u << c;  // VAD.C:164
            }
        }
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) {
            const uint64_t m = __ballot((loud3 >> c) & 1u);
            if (lane == 0) {
                const uint32_t w = k0 / 32;
                if (w < nw) s_mask[c][w] = (uint32_t)m;
                if (w + 1 < nw) s_mask[c][w + 1] = (uint32_t)(m >> 32);
            }
        }
    }
    __syncthreads();
    uint32_t *mout = a.masks + (uint64_t)tile * 3 * a.mask_words;
    for (uint32_t i = lane; i < 3 * nw; i += 64) mout[(i / nw) * a.mask_words + i % nw] = s_mask[i / nw][i % nw];

    // the tile as a function of (carry in, state in): one pair per lane and round
    const StreamSm sm = stream_sm(a);
    const uint32_t rlast = (s_P[T - 1] >> 15) & 3, nf = (F - j0 < T) ? F - j0 : T;
    uint64_t *tout = a.tab + (uint64_t)tile * 3 * a.n_states;
    for (uint32_t p = lane; p < 3 * a.n_states; p += 64) {
        const uint32_t c = p / a.n_states;
        uint32_t s = p - c * a.n_states, starts = 0, last_start = 0xFFFFFFFFu;
        for (uint32_t k = 0; k < nf; k++) {
            uint32_t ev;
            s = sm.step(s, (s_mask[c][k >> 5] >> (k & 31)) & 1u, ev);
            if (ev == 1) {
                starts++;
                last_start = k;
            }
        }
        const uint32_t cout = rlast ? rlast : c;
        tout[p] = (uint64_t)(s | cout << 8 | starts << 10) | (uint64_t)last_start << 32;
    }
}

// ---- pass 2 ------------------------------------------------------------------------------------------------------------
constexpr int kScanThreads = 1024;
__global__ void __launch_bounds__(kScanThreads) k_stream_scan(const VadStreamArgs a)
{
    __shared__ uint32_t s_w[kScanThreads / 64];
    __shared__ uint32_t s_base;
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) s_base = 0;
    for (uint32_t b0 = 0; b0 < a.B; b0 += kScanThreads) {
        const uint32_t b = b0 + tid;
        uint32_t count = 0;
        if (b < a.B) {
            const sr_atap at = stream_atap(a, b);
            a.atap_res[b] = at;
            if (a.atap_out) a.atap_out[b] = at;
            const uint32_t F = stream_frames(a, b), nt = (F + a.tile_frames - 1) / a.tile_frames;
            uint32_t c = 0, s = 0;
            int open_start = -1;
            for (uint32_t t = 0; t < nt; t++) {
                const uint64_t tile = (uint64_t)b * a.nt + t;
                a.tile_in[tile] = uint4{c | s << 8, count, (uint32_t)open_start, 0u};
                const uint64_t e = a.tab[tile * 3 * a.n_states + c * a.n_states + s];
                const uint32_t lo = (uint32_t)e, st = lo >> 10;
                if (st) open_start = (int)((t * a.tile_frames + (uint32_t)(e >> 32) - (a.v_durmin - 1)) * a.hop);  // VAD.C:178
                count += st;
                s = lo & 0xFF;
                c = (lo >> 8) & 3;
            }
        }
        // exclusive sum of the counts over the chunk, in recording order
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
        if (b < a.B) a.seg_offsets[b] = wbase + incl - count;
        __syncthreads();
        if (tid == kScanThreads - 1) s_base = wbase + incl;
        __syncthreads();
    }
    if (tid == 0) a.seg_offsets[a.B] = s_base;
}

// ---- pass 3 ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_stream_emit(const VadStreamArgs a)
{
    const uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tile >= (uint64_t)a.B * a.nt) return;
    const uint32_t b = (uint32_t)(tile / a.nt), t = (uint32_t)(tile - (uint64_t)b * a.nt);
    const uint32_t F = stream_frames(a, b), T = a.tile_frames, j0 = t * T;
    if (j0 >= F) return;
    const uint4 tin = a.tile_in[tile];
    const uint32_t c = tin.x & 0xFF;
    uint32_t s = tin.x >> 8;
    uint32_t next = a.seg_offsets[b] + tin.y;  // index of the next segment to start
    int cur_start = (int)tin.z;                // the open segment (index next - 1), if any
    const uint32_t *mask = a.masks + (uint64_t)tile * 3 * a.mask_words + c * a.mask_words;
    const StreamSm sm = stream_sm(a);
    const uint32_t nf = (F - j0 < T) ? F - j0 : T;
    auto put = [&](uint32_t idx, int st, int en) {
        if (idx < a.max_segs)
            a.segs[idx] = sr_stream_seg{b, st, en, stream_frm_num(st, en, a.frame_len, a.hop, a.max_frames)};
    };
    uint32_t word = 0;
    for (uint32_t k = 0; k < nf; k++) {
        if ((k & 31) == 0) word = mask[k >> 5];
        uint32_t ev;
        s = sm.step(s, (word >> (k & 31)) & 1u, ev);
        const int i = (int)((j0 + k) * a.hop);
        if (ev == 1) {
            cur_start = i - (int)((a.v_durmin - 1) * a.hop);  // VAD.C:178
            next++;
        } else if (ev == 2) {
            put(next - 1, cur_start, i - (int)(a.s_durmax * a.hop) + (int)a.frame_len);  // VAD.C:201
        }
    }
    if (j0 + nf == F && s >= sm.sp) put(next - 1, cur_start, -1);  // the recording ended inside this segment
}

// ---- recognition records --------------------------------------------------------------------------------------------------
// Records r0 .. r0 + n - 1 of a segmentation -> sr_vad_rec records for the frame / DTW kernels, each segment's samples copied
// to its own row: seg[0] = kStreamLead in the row, so the pre-emphasis predecessor (MFCC.C:119) is there.  Rows because the
// extension frame kernel bounds a row by 2 * pcm_stride bytes (a buffer resource), so one shared base cannot serve it.
// Records at or past the true total are padding: SR_ST_VAD_FAIL.
__global__ void __launch_bounds__(256) k_stream_records(const StreamRecArgs a)
{
    const uint32_t i = blockIdx.x, r = a.r0 + i;
    const uint32_t total = a.seg_offsets[a.B];
    int st = -1, en = -1;
    uint32_t stream = 0;
    if (r < total) {
        const sr_stream_seg g = a.segs[r];
        st = g.start;
        en = g.end;
        stream = g.stream;
    }
    uint32_t status, frm = 0;
    if (en < 0) {
        status = SR_ST_VAD_FAIL;
    } else if (st < 1) {
        status = SR_ST_SEG_OOB;
    } else {
        frm = stream_frm_num(st, en, a.frame_len, a.hop, a.max_frames);
        status = frm ? SR_ST_OK : SR_ST_MFCC_FAIL;
    }
    if (threadIdx.x == 0) {
        sr_vad_rec *o = a.recs + i;
        o->atap = (r < total) ? a.atap[stream] : sr_atap{0, 0, 0, 0};
        o->seg[0] = (int)kStreamLead;
        o->seg[1] = en < 0 ? -1 : (int)kStreamLead + (en - st);
#pragma unroll
        for (int q = 2; q < 2 * SR_MAX_SEG; q++) o->seg[q] = -1;
        o->frm_num = frm;
        o->status = status;
        o->_pad = 0;
    }
    if (status != SR_ST_OK) return;
    // samples [st - kStreamLead, st + (frm + 1) * hop): the frames of the record (frame_len = 2 * hop) and the lead; st is a
    // multiple of hop (>= hop >= 80), so the copy is 16-byte aligned at both ends
    const uint4 *src = (const uint4 *)(a.pcm + (uint64_t)stream * a.pcm_stride + (uint32_t)st - kStreamLead);
    uint4 *dst = (uint4 *)(a.rows + (uint64_t)i * a.row_stride);
    const uint32_t nv = (kStreamLead + (frm + 1) * a.hop) / 8;
    for (uint32_t v = threadIdx.x; v < nv; v += blockDim.x) dst[v] = src[v];
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
template <int FL>
static void launch_tiles_fl(const VadStreamArgs &a, bool sad, hipStream_t s)
{
    const dim3 grid((uint32_t)((uint64_t)a.B * a.nt)), block(64);
    if (sad) {
        SR_LAUNCH_POINT(s, "k_stream_tiles");
        hipLaunchKernelGGL((k_stream_tiles<FL, FL / 2, true>), grid, block, 0, s, a);
    } else {
        SR_LAUNCH_POINT(s, "k_stream_tiles");
        hipLaunchKernelGGL((k_stream_tiles<FL, FL / 2, false>), grid, block, 0, s, a);
    }
}

void launch_vad_stream(const VadStreamArgs &a, bool sad, hipStream_t s)
{
    if (!a.B) return;
    switch (a.frame_len) {
    case 160: launch_tiles_fl<160>(a, sad, s); break;
    case 240: launch_tiles_fl<240>(a, sad, s); break;
    case 256: launch_tiles_fl<256>(a, sad, s); break;
    case 320: launch_tiles_fl<320>(a, sad, s); break;
    case 400: launch_tiles_fl<400>(a, sad, s); break;
    case 512: launch_tiles_fl<512>(a, sad, s); break;
    default: return;  // sr_create accepts only the framings of vad_framing_supported
    }
    SR_LAUNCH_POINT(s, "k_stream_scan");
    hipLaunchKernelGGL(k_stream_scan, dim3(1), dim3(kScanThreads), 0, s, a);
    const uint64_t slots = (uint64_t)a.B * a.nt;
    SR_LAUNCH_POINT(s, "k_stream_emit");
    hipLaunchKernelGGL(k_stream_emit, dim3((uint32_t)((slots + 255) / 256)), dim3(256), 0, s, a);
}

void launch_stream_records(const StreamRecArgs &a, uint32_t n, hipStream_t s)
{
    if (!n) return;
    SR_LAUNCH_POINT(s, "k_stream_records");
    hipLaunchKernelGGL(k_stream_records, dim3(n), dim3(256), 0, s, a);
}

}  // namespace sr
