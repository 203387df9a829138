// k_span.hip -- word alternatives: the cost of the best path of EVERY template over one fixed span of frames, start and end
// pinned (include/sr_engine.h, "word alternatives").  OPT-IN EXTENSION, no reference counterpart; the local distance is the
// reference's get_dis (DTW.C:45-62).
// gfx950 (MI355X, CDNA4) only; wave = 64 lanes; no MFMA (the path has no dense contraction), integer VALU + LDS.
//
//   F_k(S, e) = the minimum over the connected-word decoder's word paths from (S, 0) to (e, M - 1) of the sum of d
// is k_spot's recurrence in its two-state form -- Dd = d + min(Dd, Dn)(x-1,y-1), Dn = d + min(Dd(x-1,y), Dd(x,y-1)), row 0 of
// the Dn kind -- with ONE start column: row 0 is reachable in column S only.  The start is known, so a state is a bare u32
// cost, all ones = unreachable (a cost stays below 2^31: d <= 65 536 and a path has at most 2M - 1 cells): half the shuffles
// and half the boundary column of the packed (cost, start) states of k_spot / k_chain_words.
//
// Layout: one wave per (span, slot), grid (slot, groups of kSpotWaves spans); the template is staged once per workgroup as
// k_spot stages it.  A wave runs k_chain_words' skewed anti-diagonal wavefront over the columns S..e -- lane = one column, at
// step t it meets template row t - lane, 64 columns per sweep, the sweeps start at S and the last column of a sweep goes
// through LDS to the next.  An invalid span, an invalid slot and a length no path of the slot can have (L outside
// [M/2 + 1, 2M - 1]) write SR_DIS_ERR from one lane.  Every score is written exactly once by a plain vector store: no atomics,
// two runs give the same bytes.
#include <algorithm>

#include "sr_dtw_plan.h"
#include "sr_spot_dev.h"
#include "sr_sweep_dev.h"

namespace sr {

constexpr uint32_t kSpanInf = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t span_min(uint32_t a, uint32_t b) { return b < a ? b : a; }
__device__ __forceinline__ uint32_t span_add(uint32_t a, uint32_t d) { return a == kSpanInf ? kSpanInf : a + d; }

// LDS of a workgroup: the template image (32-byte rows), then per wave a boundary column of (Dd, min(Dd, Dn)) u32 pairs
static inline uint32_t span_lds_bytes(uint32_t tpl_len) { return tpl_len * (32u + kSpotWaves * 8u); }  // <= spot_lds_bytes

__global__ void __launch_bounds__(64 * kSpotWaves) k_span_words(const SpanArgs a)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 sn_smem[];  // template rows [tpl_len][2], then the waves' boundary columns
    const uint32_t k = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t span = blockIdx.y * kSpotWaves + w;
    uint32_t M = a.tpl_valid[k] ? a.tpl_frames[k] : 0u;
    M = M < a.tpl_len ? M : a.tpl_len;
    uint2 *s_col = (uint2 *)(sn_smem + (size_t)a.tpl_len * 2) + (size_t)w * a.tpl_len;  // (Dd, min(Dd, Dn)) per row
    sweep_stage_tpl(sn_smem, a.tpl + (size_t)k * a.tpl_stride, M);
    __syncthreads();
    if (span >= a.n_spans) return;

    const uint32_t row = span / a.words_per_row;
    uint32_t N = a.in_frames[(size_t)row * a.frames_stride];
    N = N < a.max_frames ? N : a.max_frames;
    const uint32_t S = a.words[span].start, e = a.words[span].end;
    uint32_t *out = a.scores + (size_t)span * a.K + k;
    // (wave-uniform) nothing to walk: an invalid span or slot, or a length no path of this slot has
    const bool valid = M && S != 0xFFFFFFFFu && e != 0xFFFFFFFFu && S <= e && e < N;
    const uint32_t L = valid ? e - S + 1 : 0u;
    if (!valid || L < M / 2 + 1 || L > 2 * M - 1) {
        if (lane == 0) *out = SR_DIS_ERR;
        return;
    }
    const int16_t *in = a.mfcc + (size_t)row * a.max_frames * kCoef;
    uint32_t end_v = kSpanInf;  // min(Dd, Dn) of (e, M - 1), in the lane of column e
    for (uint32_t x0 = S; x0 <= e; x0 += 64) {  // (wave-uniform; e < 16 383: no wrap)
        const uint32_t col = x0 + lane;
        const bool live = col <= e;
        Row32 fi = row_from2(u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, 0u);
        if (live) fi = sweep_frame(in + (size_t)col * kCoef);  // S <= col <= e < N: inside the row's frames
        uint32_t up_d = kSpanInf, up_m = kSpanInf;  // Dd and min(Dd, Dn) of (col, row - 1): the lane's last results
        uint32_t diag = kSpanInf;                   // min(Dd, Dn) of (col - 1, row - 1): last step's value from the left
        const uint32_t steps = M + (e + 1 - x0 < 64u ? e + 1 - x0 : 64u) - 1;
        for (uint32_t t = 0; t < steps; t++) {
            const int r = (int)t - (int)lane;
            // the left lane's results of the previous step are the states of (col - 1, r)
            uint32_t fl_d = __shfl_up(up_d, 1, 64), fl_m = __shfl_up(up_m, 1, 64);
            if (lane == 0) {
                fl_d = fl_m = kSpanInf;
                if (x0 != S && t < M) {
                    const uint2 v = s_col[t];
                    fl_d = v.x;
                    fl_m = v.y;
                }
            }
            if (live && r >= 0 && r < (int)M) {
                const Row32 fm = row_from(sn_smem[2 * r], sn_smem[2 * r + 1]);
                const uint32_t d = dis_from(fi.w[6], fm.w[6], dot_rows(fi, fm));
                uint32_t cd = kSpanInf, cn;
                if (r > 0) {
                    cd = span_add(diag, d);
                    cn = span_add(span_min(fl_d, up_d), d);
                } else {  // row 0: the one start, of the non-diagonal kind
                    cn = col == S ? d : kSpanInf;
                }
                up_d = cd;
                up_m = span_min(cd, cn);
                if (lane == 63) s_col[r] = uint2{up_d, up_m};
                if (r == (int)M - 1) end_v = up_m;
            }
            diag = fl_m;
        }
        wave_sync();  // the boundary column is complete before the next sweep's lane 0 reads it
        if (col == e) *out = end_v == kSpanInf ? SR_DIS_ERR : a.mode == SR_SPAN_DIS ? end_v / (L + M) : end_v;
    }
}

void launch_span(const SpanArgs &a, hipStream_t s)
{
    if (!a.n_spans || !a.K) return;
    const size_t lds = span_lds_bytes(a.tpl_len);
    // the groups of spans are the grid's second dimension (<= 65 535): more go out in slices of whole rows, as launch_spot's
    // (max_groups is that limit; a testing build may lower it, and a slice then holds one row at least)
    const uint32_t per = std::max(a.max_groups * kSpotWaves / a.words_per_row, 1u) * a.words_per_row;
    for (uint64_t s0 = 0; s0 < a.n_spans; s0 += per) {
        SpanArgs sa = a;
        sa.n_spans = (uint32_t)std::min<uint64_t>(a.n_spans - s0, per);
        const uint64_t r0 = s0 / a.words_per_row;
        sa.mfcc = a.mfcc + (size_t)r0 * a.max_frames * kCoef;
        sa.in_frames = a.in_frames + (size_t)r0 * a.frames_stride;
        sa.words = a.words + s0;
        sa.scores = a.scores + (size_t)s0 * a.K;
        SR_LAUNCH_POINT(s, "k_span_words");
        hipLaunchKernelGGL(k_span_words, dim3(a.K, (sa.n_spans + kSpotWaves - 1) / kSpotWaves), dim3(64 * kSpotWaves), lds, s, sa);
    }
}
const char *span_allow_lds(uint32_t bytes) { return allow_dynamic_lds({{(const void *)k_span_words, "k_span_words"}}, bytes); }

}  // namespace sr
