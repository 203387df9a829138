// k_spot_live.hip -- live word spotting (include/sr_engine.h, "live word spotting"): k_spot's sweep, resumed from push to push.
// OPT-IN EXTENSION, no reference counterpart.  gfx950 (MI355X, CDNA4) only; wave = 64 lanes; integer VALU + LDS.
//
// The two-state recurrence of k_spot.hip looks back exactly one column: Dd(x,y) needs min(Dd, Dn)(x-1,y-1), Dn(x,y) needs
// Dd(x-1,y) and Dd(x,y-1).  Between two 64-column sweeps k_spot therefore hands over one boundary column, per template row
// the pair (Dd, min(Dd, Dn)), and the carry of the window reduction.  Here the same two things are kept in device memory
// between calls: they are the complete state of a (channel, slot) pair.  A wave enters at x0 = the channel's frame count so
// far (any value, not a multiple of 64), takes lane 0's left neighbour from the saved column (unreachable for a fresh
// channel), sweeps the new columns 64 at a time and saves the column of the LAST LIVE lane with the carry.  Starts are
// absolute frame indices of the channel's recording, so the packed (cost, start) minimum is the tie rule of the one-shot
// spotter over the whole recording, whatever the chunking.
// Grid (slot, groups of kSpotWaves channels): the template is staged once per workgroup and shared by its channels, one wave
// each.  A push is not split along time.  A window's record is written by the lane of its last end frame, exactly once, to
// the row the host assigned (it knows every count).  No atomics, no flags between workgroups, plain stores.
#include "sr_dtw_plan.h"
#include "sr_spot_dev.h"
#include "sr_sweep_dev.h"

namespace sr {

__device__ __forceinline__ sr_spot_hit spot_live_record(uint64_t key, uint32_t start, uint32_t acc)
{
    if (key == kSpotInf) return sr_spot_hit{SR_DIS_ERR, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    return sr_spot_hit{(uint32_t)(key >> 32), start, (uint32_t)key, acc};
}

// the carry of (channel c, slot k): kSpotLiveCarryBytes, laid out as sr_device.h says; `list` entries of one flush launch name
// distinct channels (the host sees to it), so no two threads of it touch the same carry
__device__ __forceinline__ ulonglong2 *spot_live_carry(uint8_t *state, uint64_t chan_stride, uint32_t c, uint32_t K, uint32_t tpl_len, uint32_t k)
{
    return (ulonglong2 *)(state + (uint64_t)c * chan_stride + (uint64_t)K * tpl_len * 16u) + (kSpotLiveCarryBytes / 16u) * k;
}

__global__ void __launch_bounds__(64 * kSpotWaves) k_spot_live(const SpotLiveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 sl_smem[];  // template rows [tpl_len][2], then the waves' boundary columns
    const uint32_t k = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.y * kSpotWaves + w;
    uint32_t M = a.tpl_valid[k] ? a.tpl_frames[k] : 0u;
    M = M < a.tpl_len ? M : a.tpl_len;
    ulonglong2 *s_col = (ulonglong2 *)(sl_smem + (size_t)a.tpl_len * 2) + (size_t)w * a.tpl_len;  // (Dd, min(Dd, Dn)) per row
    sweep_stage_tpl(sl_smem, a.tpl + (size_t)k * a.tpl_stride, M);
    __syncthreads();
    if (c >= a.C) return;
    const SpotLiveChan ch = a.chan[c];
    if (!ch.n) return;  // (wave-uniform) a silent channel is not touched

    const uint32_t xs = ch.x0, cN = ch.x0 + ch.n, W = a.win;  // the new columns [xs, cN), absolute
    ulonglong2 *g_col = (ulonglong2 *)(a.state + (uint64_t)c * a.chan_stride) + (size_t)k * a.tpl_len;
    ulonglong2 *g_carry = spot_live_carry(a.state, a.chan_stride, c, a.K, a.tpl_len, k);
    auto put = [&](uint32_t wid, const sr_spot_hit &rec) {
        const size_t at = ((size_t)ch.row_base + (wid - ch.first_win)) * a.K + k;
        a.hits[at] = rec;
        if (a.scores) a.scores[at] = rec.dis;
    };
    if (!M) {  // an invalid slot: no hit in every window this push completes, and a carry that says so
        const sr_spot_hit none = spot_live_record(kSpotInf, 0u, 0u);
        const uint32_t w1 = cN / W;
        for (uint32_t wv = ch.first_win + lane; wv < w1; wv += 64) put(wv, none);
        if (lane == 0) {
            g_carry[0] = ulonglong2{kSpotInf, ~0ull};
            g_carry[1] = ulonglong2{(cN - 1) / W, 0ull};
        }
        return;
    }

    uint64_t carry_key = kSpotInf;
    uint32_t carry_s = 0xFFFFFFFFu, carry_d = 0xFFFFFFFFu, carry_wid = 0xFFFFFFFFu;
    if (xs) {  // resume: the saved column (16-byte loads, coalesced over template rows) and the carry
        for (uint32_t r = lane; r < M; r += 64) s_col[r] = g_col[r];
        const ulonglong2 c0 = g_carry[0], c1 = g_carry[1];
        carry_key = c0.x;
        carry_s = (uint32_t)c0.y;
        carry_d = (uint32_t)(c0.y >> 32);
        carry_wid = (uint32_t)c1.x;
        wave_sync();
    }
    const int16_t *in = a.mfcc + (uint64_t)c * a.row_stride;
    for (uint32_t x0 = xs; x0 < cN; x0 += 64) {  // (wave-uniform)
        const uint32_t col = x0 + lane;
        const bool live = col < cN;
        const uint32_t last = (cN - x0 < 64u ? cN - x0 : 64u) - 1;  // the sweep's last live lane: its column is handed on
        Row32 fi = row_from2(u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, 0u);
        if (live) fi = sweep_frame(in + (size_t)(col - xs) * kCoef);
        uint64_t up_d = kSpotInf, up_m = kSpotInf;  // Dd and min(Dd, Dn) of (col, row - 1): the lane's last results
        uint64_t diag = kSpotInf;                   // min(Dd, Dn) of (col - 1, row - 1): last step's value from the left
        uint64_t end_v = kSpotInf;                  // min(Dd, Dn) of (col, M - 1)
        const uint32_t steps = M + last;
        for (uint32_t t = 0; t < steps; t++) {
            const int r = (int)t - (int)lane;
            // the left lane's results of the previous step are the states of (col - 1, r)
            uint64_t fl_d = spot_shfl_up(up_d, 1), fl_m = spot_shfl_up(up_m, 1);
            if (lane == 0) {
                fl_d = fl_m = kSpotInf;
                if (x0 != 0 && t < M) {  // column x0 - 1: this call's last sweep, or the last push (none for a fresh channel)
                    const ulonglong2 v = s_col[t];
                    fl_d = v.x;
                    fl_m = v.y;
                }
            }
            if (live && r >= 0 && r < (int)M) {
                const Row32 fm = row_from(sl_smem[2 * r], sl_smem[2 * r + 1]);
                const uint32_t d = dis_from(fi.w[6], fm.w[6], dot_rows(fi, fm));
                uint64_t cd = kSpotInf, cn = ((uint64_t)d << 32) | col;  // row 0: a start, of the non-diagonal kind
                if (r > 0) {
                    cd = spot_add(diag, d);
                    cn = spot_add(spot_min(fl_d, up_d), d);
                }
                up_d = cd;
                up_m = spot_min(cd, cn);
                if (lane == last) s_col[r] = ulonglong2{up_d, up_m};  // (lane 0 has read row r before it writes it)
                if (r == (int)M - 1) end_v = up_m;
            }
            diag = fl_m;
        }
        wave_sync();  // the boundary column is complete before the next sweep's lane 0, or the save below, reads it

        // q(e) of the sweep's end frames, then the first minimum per window: k_spot's segmented min-scan on (q, e)
        const uint32_t e_s = (uint32_t)end_v, e_d = (uint32_t)(end_v >> 32);
        uint64_t key = kSpotInf;
        if (end_v != kSpotInf) key = ((uint64_t)(e_d / (col - e_s + 1 + M)) << 32) | col;
        const uint32_t wid = col / W;
#pragma unroll
        for (uint32_t by = 1; by < 64; by <<= 1) {
            const uint32_t o_wid = __shfl_up(wid, by, 64);
            const uint64_t o_key = spot_shfl_up(key, by);
            if (lane >= by && o_wid == wid) key = spot_min(key, o_key);
        }
        if (wid == carry_wid) key = spot_min(key, carry_key);
        // start and cost of the winner: its lane of this sweep, or the carry when it ended in an earlier sweep or push
        const uint32_t we = (uint32_t)key;
        uint32_t p_s = __shfl(e_s, (int)((we - x0) & 63u), 64), p_d = __shfl(e_d, (int)((we - x0) & 63u), 64);
        if (key != kSpotInf && we < x0) {
            p_s = carry_s;
            p_d = carry_d;
        }
        if (live && col % W == W - 1) put(wid, spot_live_record(key, p_s, p_d));  // the window's last end frame has arrived
        carry_key = spot_shfl(key, last);
        carry_s = __shfl(p_s, (int)last, 64);
        carry_d = __shfl(p_d, (int)last, 64);
        carry_wid = __shfl(wid, (int)last, 64);
    }
    // the state for the next push: column cN - 1 (16-byte stores, coalesced over template rows) and the carry
    for (uint32_t r = lane; r < M; r += 64) g_col[r] = s_col[r];
    if (lane == 0) {
        g_carry[0] = ulonglong2{carry_key, (uint64_t)carry_s | ((uint64_t)carry_d << 32)};
        g_carry[1] = ulonglong2{carry_wid, 0ull};
    }
}

// sr_spot_live_end: the open window of each listed channel as a record (the carry is its first minimum so far)
__global__ void __launch_bounds__(256) k_spot_live_flush(const SpotLiveFlush *list, uint32_t n_list, uint8_t *state, uint64_t chan_stride,
                                                         uint32_t K, uint32_t tpl_len, sr_spot_hit *hits)
{
    const uint64_t n = (uint64_t)n_list * K;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const SpotLiveFlush f = list[i / K];
        const uint32_t k = (uint32_t)(i % K);
        ulonglong2 *g = spot_live_carry(state, chan_stride, f.channel, K, tpl_len, k);
        if (f.row != 0xFFFFFFFFu) {
            const ulonglong2 c0 = g[0], c1 = g[1];
            const bool mine = (uint32_t)c1.x == f.wid;
            hits[(size_t)f.row * K + k] = spot_live_record(mine ? c0.x : kSpotInf, (uint32_t)c0.y, (uint32_t)(c0.y >> 32));
        }
        g[0] = ulonglong2{kSpotInf, ~0ull};  // as a fresh channel's
        g[1] = ulonglong2{0xFFFFFFFFull, 0ull};
    }
}

// PCM sessions: row c = [the channel's kept samples | its chunk], what the frame kernel reads with seg[0] = 1
__global__ void __launch_bounds__(256) k_spot_live_stage(const SpotLivePcmArgs a)
{
    const uint32_t c = blockIdx.y;
    const SpotLiveChan ch = a.chan[c];
    if (!ch.n_samp) return;
    const uint16_t *keep = a.keep + (size_t)c * a.keep_stride, *pcm = a.pcm + (uint64_t)c * a.pcm_stride;
    uint16_t *row = a.stage + (uint64_t)c * a.stage_stride;
    const uint32_t len = ch.kept + ch.n_samp;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < len; i += gridDim.x * 256) row[i] = i < ch.kept ? keep[i] : pcm[i - ch.kept];
}

// ... and after it the samples from the next frame's predecessor on (at most frame_len of them) back into the channel's store
__global__ void __launch_bounds__(256) k_spot_live_keep(const SpotLivePcmArgs a)
{
    const uint32_t c = blockIdx.x;
    const SpotLiveChan ch = a.chan[c];
    if (!ch.n_samp) return;
    const uint16_t *row = a.stage + (uint64_t)c * a.stage_stride + ch.drop;
    uint16_t *keep = a.keep + (size_t)c * a.keep_stride;
    const uint32_t len = ch.kept + ch.n_samp - ch.drop;
    for (uint32_t i = threadIdx.x; i < len && i < a.keep_stride; i += 256) keep[i] = row[i];
}

void launch_spot_live(const SpotLiveArgs &a, hipStream_t s)
{
    if (!a.C || !a.K) return;
    const dim3 grid(a.K, (a.C + kSpotWaves - 1) / kSpotWaves);
    SR_LAUNCH_POINT(s, "k_spot_live");
    hipLaunchKernelGGL(k_spot_live, grid, dim3(64 * kSpotWaves), spot_lds_bytes(a.tpl_len), s, a);
}
void launch_spot_live_flush(const SpotLiveFlush *list, uint32_t n_list, uint8_t *state, uint64_t chan_stride, uint32_t K, uint32_t tpl_len,
                            sr_spot_hit *hits, hipStream_t s)
{
    if (!n_list || !K) return;
    const uint64_t blocks = ((uint64_t)n_list * K + 255) / 256;
    SR_LAUNCH_POINT(s, "k_spot_live_flush");
    hipLaunchKernelGGL(k_spot_live_flush, dim3((uint32_t)(blocks < 65536u ? blocks : 65536u)), dim3(256), 0, s, list, n_list, state, chan_stride, K,
                       tpl_len, hits);
}
void launch_spot_live_stage(const SpotLivePcmArgs &a, hipStream_t s)
{
    if (!a.C || !a.max_row) return;
    const uint32_t bx = (a.max_row + 255) / 256;
    SR_LAUNCH_POINT(s, "k_spot_live_stage");
    hipLaunchKernelGGL(k_spot_live_stage, dim3(bx < 64u ? bx : 64u, a.C), dim3(256), 0, s, a);
}
void launch_spot_live_keep(const SpotLivePcmArgs &a, hipStream_t s)
{
    if (!a.C || !a.max_row) return;
    SR_LAUNCH_POINT(s, "k_spot_live_keep");
    hipLaunchKernelGGL(k_spot_live_keep, dim3(a.C), dim3(256), 0, s, a);
}
const char *spot_live_allow_lds(uint32_t bytes) { return allow_dynamic_lds({{(const void *)k_spot_live, "k_spot_live"}}, bytes); }

}  // namespace sr
