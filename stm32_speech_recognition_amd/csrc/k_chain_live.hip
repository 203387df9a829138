// k_chain_live.hip -- live connected-word decoding (include/sr_engine.h, "live connected-word decoding"): the levels of
// k_chain.hip, resumed from push to push.  OPT-IN EXTENSION, no reference counterpart.  gfx950 (MI355X, CDNA4) only; wave = 64
// lanes; integer VALU + LDS.
//
// Three facts of the batch decoder make it resumable without changing a cost.  A level is k_spot's two-state recurrence with a
// charged start row: column x needs column x - 1 and E_{l-1}(x), nothing else.  A_l(p) and E_l(p) depend on frames < p only
// (the (N - j) * skip form of k_chain_close is a way to compute, N does not enter the value), so the history of a recording is
// a prefix of the history of any longer one.  Count and trace read A, E and N.  A push that appends frames [x0, x0 + n) is:
//   k_chain_live_init    E_0 and all-ones A_l over the new positions (x0, x0 + n]; position 0 too for a fresh channel;
//   per level l = 1..max_words, in stream order:
//   k_chain_live_words   k_spot_live's resumed sweep -- grid (slot, groups of kSpotWaves channels), the saved boundary column
//                        of (channel, level, slot) in, the last live lane's column out -- with k_chain_words' charged row 0
//                        and its 64-bit atomic minimum of every new end frame's key into A_l(col + 1);
//   k_chain_live_close   E_l over (x0, x0 + n] from the carried E_l(x0): k_chain_close's wave scan with a carry;
//   k_chain_live_trace   chain_trace_row (sr_spot_dev.h) with N = x0 + n into the compact row the host assigned.
// No workgroup waits on another: the levels are ordered by the stream alone.  Plain vector stores; the atomic minimum on A is
// the only atomic, and it does not depend on the order of the waves, so two runs give the same bytes.
#include "sr_dtw_plan.h"
#include "sr_spot_dev.h"
#include "sr_sweep_dev.h"

namespace sr {

__device__ __forceinline__ unsigned long long *chain_live_A(const ChainLiveArgs &a, uint32_t c, uint32_t level)  // level 1..max_words
{
    return a.A + ((size_t)c * a.max_words + (level - 1)) * a.P;
}
__device__ __forceinline__ uint32_t *chain_live_E(const ChainLiveArgs &a, uint32_t c, uint32_t level)  // level 0..max_words
{
    return a.E + ((size_t)c * (a.max_words + 1u) + level) * a.P;
}

// the new positions of every level: E_0, "no word yet" in every A; a fresh channel also gets position 0
__global__ void __launch_bounds__(256) k_chain_live_init(const ChainLiveArgs a)
{
    const uint32_t c = blockIdx.x;
    const SpotLiveChan ch = a.chan[c];
    if (!ch.n) return;
    const bool skip = a.skip_cost != kChainNone;
    const uint32_t p0 = ch.x0 ? ch.x0 + 1 : 0u, p1 = ch.x0 + ch.n;  // positions [p0, p1], p1 <= utt_frames = P - 1
    uint32_t *e0 = chain_live_E(a, c, 0);
    for (uint32_t p = p0 + threadIdx.x; p <= p1; p += 256) e0[p] = skip ? p * a.skip_cost : (p ? kChainNone : 0u);
    for (uint32_t l = 1; l <= a.max_words; l++) {
        unsigned long long *A = chain_live_A(a, c, l);
        for (uint32_t p = p0 + threadIdx.x; p <= p1; p += 256) A[p] = kSpotInf;
        if (!ch.x0 && threadIdx.x == 0) chain_live_E(a, c, l)[0] = kChainNone;
    }
}

__global__ void __launch_bounds__(64 * kSpotWaves) k_chain_live_words(const ChainLiveArgs a, const uint32_t level)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 cl_smem[];  // template rows [tpl_len][2], then the waves' boundary columns
    const uint32_t k = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.y * kSpotWaves + w;
    uint32_t M = a.tpl_valid[k] ? a.tpl_frames[k] : 0u;
    M = M < a.tpl_len ? M : a.tpl_len;
    ulonglong2 *s_col = (ulonglong2 *)(cl_smem + (size_t)a.tpl_len * 2) + (size_t)w * a.tpl_len;  // (Dd, min(Dd, Dn)) per row
    sweep_stage_tpl(cl_smem, a.tpl + (size_t)k * a.tpl_stride, M);
    __syncthreads();
    if (c >= a.C || !M) return;  // (an invalid slot ends no word and keeps no column)
    const SpotLiveChan ch = a.chan[c];
    if (!ch.n) return;  // (wave-uniform) a silent channel is not touched

    const uint32_t xs = ch.x0, cN = ch.x0 + ch.n;  // the new columns [xs, cN), absolute; cN <= utt_frames
    ulonglong2 *g_col = a.cols + (((size_t)c * a.max_words + (level - 1)) * a.K + k) * a.tpl_len;
    const uint32_t *e_prev = chain_live_E(a, c, level - 1);
    unsigned long long *A = chain_live_A(a, c, level);
    if (xs) {  // resume: the saved column (16-byte loads, coalesced over template rows)
        for (uint32_t r = lane; r < M; r += 64) s_col[r] = g_col[r];
        wave_sync();
    }
    const int16_t *in = a.mfcc + (uint64_t)c * a.row_stride;
    for (uint32_t x0 = xs; x0 < cN; x0 += 64) {  // (wave-uniform)
        const uint32_t col = x0 + lane;
        const bool live = col < cN;
        const uint32_t last = (cN - x0 < 64u ? cN - x0 : 64u) - 1;  // the sweep's last live lane: its column is handed on
        Row32 fi = row_from2(u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, 0u);
        uint32_t charge = kChainNone;  // E_{l-1}(col): what a word that starts in this column builds on
        if (live) {
            fi = sweep_frame(in + (size_t)(col - xs) * kCoef);
            charge = e_prev[col];
        }
        // the step loop stands here and not in sweep_step: shared, this kernel measured 0.2 to 0.4 % slower than unshared
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
                const Row32 fm = row_from(cl_smem[2 * r], cl_smem[2 * r + 1]);
                const uint32_t d = dis_from(fi.w[6], fm.w[6], dot_rows(fi, fm));
                uint64_t cd = kSpotInf, cn;
                if (r > 0) {
                    cd = spot_add(diag, d);
                    cn = spot_add(spot_min(fl_d, up_d), d);
                } else {  // row 0: a charged start, of the non-diagonal kind
                    cn = charge == kChainNone ? kSpotInf : ((uint64_t)(charge + d) << 32) | col;
                }
                up_d = cd;
                up_m = spot_min(cd, cn);
                if (lane == last) s_col[r] = ulonglong2{up_d, up_m};  // (lane 0 has read row r before it writes it)
                if (r == (int)M - 1) end_v = up_m;
            }
            diag = fl_m;
        }
        wave_sync();  // the boundary column is complete before the next sweep's lane 0, or the save below, reads it

        // the key of each new end frame: (cost + word_cost, start, slot) -> A_l(col + 1); col + 1 <= cN <= utt_frames
        if (live && end_v != kSpotInf) atomicMin(&A[col + 1], sweep_end_key(end_v, a.word_cost, k));
    }
    // the state for the next push: column cN - 1 (16-byte stores, coalesced over template rows)
    for (uint32_t r = lane; r < M; r += 64) g_col[r] = s_col[r];
}

// E_l(p), p in (x0, x0 + n]: min(min over x0 < j <= p of A_l(j).cost + (p - j) * skip, E_l(x0) + (p - x0) * skip), as a prefix
// minimum of A_l(j).cost + (cN - j) * skip in u64 that starts from the carried E_l(x0) + (cN - x0) * skip, less (cN - p) * skip.
// One workgroup per channel: wave scans plus an LDS carry, as k_chain_close.
__global__ void __launch_bounds__(256) k_chain_live_close(const ChainLiveArgs a, const uint32_t level)
{
    __shared__ uint64_t s_tot[4];
    const uint32_t c = blockIdx.x;
    const SpotLiveChan ch = a.chan[c];
    if (!ch.n) return;  // (uniform)
    const uint32_t xs = ch.x0, cN = ch.x0 + ch.n;
    const unsigned long long *A = chain_live_A(a, c, level);
    uint32_t *E = chain_live_E(a, c, level);
    close_window(A, E, xs, cN, a.skip_cost, s_tot);
}

// one wave per emitting channel: the parse of its N = x0 + n frames into its compact row
__global__ void __launch_bounds__(64) k_chain_live_trace(const ChainLiveArgs a)
{
    const uint32_t c = blockIdx.x, W = a.max_words;
    const SpotLiveChan ch = a.chan[c];
    if (!ch.first_win) return;
    const size_t row = ch.row_base;
    chain_trace_row(chain_live_A(a, c, 1), chain_live_E(a, c, 0), a.P, ch.x0 + ch.n, W, a.n_words_exact, a.word_cost, a.tpl_frames,
                    a.group_of_slot, a.word_id, a.rec + row, a.words + row * W, a.level_cost ? a.level_cost + row * W : nullptr, threadIdx.x);
}

void launch_chain_live(const ChainLiveArgs &a, hipStream_t s)
{
    if (!a.C || !a.K) return;
    const size_t lds = spot_lds_bytes(a.tpl_len);
    SR_LAUNCH_POINT(s, "k_chain_live_init");
    hipLaunchKernelGGL(k_chain_live_init, dim3(a.C), dim3(256), 0, s, a);
    const dim3 grid(a.K, (a.C + kSpotWaves - 1) / kSpotWaves);
    for (uint32_t l = 1; l <= a.max_words; l++) {
        SR_LAUNCH_POINT(s, "k_chain_live_words");
        hipLaunchKernelGGL(k_chain_live_words, grid, dim3(64 * kSpotWaves), lds, s, a, l);
        SR_LAUNCH_POINT(s, "k_chain_live_close");
        hipLaunchKernelGGL(k_chain_live_close, dim3(a.C), dim3(256), 0, s, a, l);
    }
    SR_LAUNCH_POINT(s, "k_chain_live_trace");
    hipLaunchKernelGGL(k_chain_live_trace, dim3(a.C), dim3(64), 0, s, a);
}
void launch_chain_live_trace(const ChainLiveArgs &a, hipStream_t s)
{
    if (!a.C) return;
    SR_LAUNCH_POINT(s, "k_chain_live_trace");
    hipLaunchKernelGGL(k_chain_live_trace, dim3(a.C), dim3(64), 0, s, a);
}
const char *chain_live_allow_lds(uint32_t bytes) { return allow_dynamic_lds({{(const void *)k_chain_live_words, "k_chain_live_words"}}, bytes); }

}  // namespace sr
