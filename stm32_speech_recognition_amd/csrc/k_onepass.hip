// k_onepass.hip -- one-pass connected-word decoding (include/sr_engine.h, "one-pass connected-word decoding"): ONE prefix-cost
// array E(p) over all word counts instead of one per level, so a row holds any number of words and a call pays 2 x K x M x N
// cells whatever that number is.  OPT-IN EXTENSION, no reference counterpart.  gfx950 (MI355X, CDNA4) only; wave = 64 lanes;
// integer VALU + LDS.
//
// E(p) needs every slot's end at frame p - 1; taken literally that is a chip-wide synchronisation per frame.  A word over M
// template frames spans at least M / 2 + 1 input frames, so with L = min_k(M_k / 2 + 1) a word that starts inside a block of
// n <= L frames [c0, c0 + n) ends at or after c0 + n: A and E over (c0, c0 + n] follow from E at or before c0 alone
// (sr_onepass_plan.h).  Per launch group:
//   k_onepass_init    E(0) = 0 and all-ones A;
//   per block [c0, cN) of the host's list, in stream order:
//   k_onepass_words   k_chain_live_words' resumed wavefront -- grid (slot, groups of kSpotWaves rows), lane = column, the template
//                     in LDS -- from the saved column of (row, slot), the EXACT column at the previous block's c0, over the
//                     columns (c0_prev, cN).  A start is charged E(col) for col <= c0 (final by then) and is unreachable for
//                     col > c0.  Column c0 is exact again and is saved; the end keys of the columns >= c0 go to A(col + 1) with the
//                     64-bit atomic minimum.  The columns (c0, cN) lack the starts inside the block -- which cannot reach the end
//                     row before cN -- and are swept again, exactly, by the next block: every column is swept twice;
//   k_onepass_close   k_chain_live_close's carried prefix minimum: E over (c0, cN] from E(c0);
//   k_onepass_trace   one wave per row, 64 positions per step as chain_trace_row, walked twice: count, then write.
// No workgroup waits on another: the blocks are ordered by the stream alone.  Plain vector stores; the atomic minimum on A is
// the only atomic, and it does not depend on the order of the waves, so two runs give the same bytes.
#include "sr_dtw_plan.h"
#include "sr_spot_dev.h"
#include "sr_sweep_dev.h"

namespace sr {

__device__ __forceinline__ uint32_t onepass_frames(const OnePassArgs &a, uint32_t row)
{
    const uint32_t n = a.in_frames[(size_t)row * a.frames_stride];
    return n < a.frames_cap ? n : a.frames_cap;  // frames_cap <= max_frames
}

__global__ void __launch_bounds__(256) k_onepass_init(const OnePassArgs a)
{
    const uint32_t row = blockIdx.x, P = a.max_frames + 1u;
    unsigned long long *A = a.A + (size_t)row * P;
    for (uint32_t p = threadIdx.x; p < P; p += 256) A[p] = kSpotInf;
    if (threadIdx.x == 0) a.E[(size_t)row * P] = 0u;
}

// block [c0, cN) of every (slot, row): the columns [xs, cN) with xs = c0_prev + 1, or 0 for the first block
__global__ void __launch_bounds__(64 * kSpotWaves) k_onepass_words(const OnePassArgs a, const uint32_t xs, const uint32_t c0, const uint32_t cN_blk)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 op_smem[];  // template rows [tpl_len][2], then the waves' boundary columns
    const uint32_t k = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t row = blockIdx.y * kSpotWaves + w;
    uint32_t M = a.tpl_valid[k] ? a.tpl_frames[k] : 0u;
    M = M < a.tpl_len ? M : a.tpl_len;
    ulonglong2 *s_col = (ulonglong2 *)(op_smem + (size_t)a.tpl_len * 2) + (size_t)w * a.tpl_len;  // (Dd, min(Dd, Dn)) per row
    sweep_stage_tpl(op_smem, a.tpl + (size_t)k * a.tpl_stride, M);
    __syncthreads();
    if (row >= a.n_rows || !M) return;  // (an invalid slot ends no word and keeps no column)
    const uint32_t N = onepass_frames(a, row);
    if (N <= c0) return;  // (wave-uniform) the row ended before this block
    const uint32_t cN = cN_blk < N ? cN_blk : N, P = a.max_frames + 1u;  // the row may end inside the block

    ulonglong2 *g_col = a.cols + ((size_t)row * a.K + k) * a.tpl_len;
    const uint32_t *E = a.E + (size_t)row * P;
    unsigned long long *A = a.A + (size_t)row * P;
    if (xs) {  // resume: the saved column, that of xs - 1 (16-byte loads, coalesced over template rows)
        for (uint32_t r = lane; r < M; r += 64) s_col[r] = g_col[r];
        wave_sync();
    }
    const int16_t *in = a.mfcc + (size_t)row * a.max_frames * kCoef;
    for (uint32_t x0 = xs; x0 < cN; x0 += 64) {  // (wave-uniform)
        const uint32_t col = x0 + lane;
        const bool live = col < cN;
        const uint32_t last = (cN - x0 < 64u ? cN - x0 : 64u) - 1;  // the sweep's last live lane: its column is handed on
        const bool keep = col == c0;                                // the exact column the next block resumes from
        Row32 fi = row_from2(u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, 0u);
        uint32_t charge = kChainNone;  // E(col): what a word that starts in this column builds on; none yet inside the block
        if (live) {
            fi = sweep_frame(in + (size_t)col * kCoef);
            if (col <= c0) charge = E[col];
        }
        SweepLane sw;
        for (uint32_t t = 0; t < M + last; t++)
            sweep_step(op_smem, s_col, g_col, keep, fi, charge, col, live, x0 != 0, last, M, lane, t, sw);
        wave_sync();  // the boundary column is complete before the next sweep's lane 0 reads it

        // the key of each end frame of the block: (cost + word_cost, start, slot) -> A(col + 1); col + 1 <= cN <= max_frames
        if (live && col >= c0 && sw.end_v != kSpotInf) atomicMin(&A[col + 1], sweep_end_key(sw.end_v, a.word_cost, k));
    }
}

// E(p), p in (c0, cN]: min(min over c0 < j <= p of A(j).cost + (p - j) * skip, E(c0) + (p - c0) * skip), as a prefix minimum of
// A(j).cost + (cN - j) * skip in u64 that starts from the carried E(c0) + (cN - c0) * skip, less (cN - p) * skip.  One workgroup
// per row: wave scans plus an LDS carry, as k_chain_live_close.
__global__ void __launch_bounds__(256) k_onepass_close(const OnePassArgs a, const uint32_t c0, const uint32_t cN_blk)
{
    __shared__ uint64_t s_tot[4];
    const uint32_t row = blockIdx.x, P = a.max_frames + 1u;
    const uint32_t N = onepass_frames(a, row);
    if (N <= c0) return;  // (uniform)
    const uint32_t cN = cN_blk < N ? cN_blk : N;
    const unsigned long long *A = a.A + (size_t)row * P;
    uint32_t *E = a.E + (size_t)row * P;
    close_window(A, E, c0, cN, a.skip_cost, s_tot);
}

// one wave per row: the history is walked twice (onepass_word_at, sr_spot_dev.h), first for the count, then for the words in
// spoken order
__global__ void __launch_bounds__(64) k_onepass_trace(const OnePassArgs a)
{
    const uint32_t row = blockIdx.x, lane = threadIdx.x, P = a.max_frames + 1u, W = a.words_cap;
    const uint32_t N = onepass_frames(a, row);
    const unsigned long long *A = a.A + (size_t)row * P;
    const uint32_t *E = a.E + (size_t)row * P;
    sr_chain_word *words = a.words + (size_t)row * W;
    const sr_chain_word none = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    const uint32_t total = N ? E[N] : kChainNone;
    if (total == kChainNone) {  // (uniform) an empty row or no parse
        for (uint32_t i = lane; i < W; i += 64) words[i] = none;
        if (lane == 0) a.rec[row] = sr_chain_rec{kChainNone, 0u, 0u, SR_CH_NONE};
        return;
    }
    uint32_t n = 0, in_words = 0;
    for (uint32_t p = N; p;) {  // (uniform) the count; every start lies below its end position: the walk ends
        uint64_t key = kSpotInf;
        const uint32_t q = onepass_word_at(A, E, p, lane, &key);
        if (!q) break;
        const uint32_t start = (uint32_t)(key >> 16) & 0xFFFFu;
        n++;
        in_words += q - start;  // frames start .. q - 1
        p = start;
    }
    for (uint32_t i = (n < W ? n : W) + lane; i < W; i += 64) words[i] = none;
    uint32_t i = n;
    for (uint32_t p = N; p;) {
        uint64_t key = kSpotInf;
        const uint32_t q = onepass_word_at(A, E, p, lane, &key);
        if (!q) break;
        const uint32_t slot = (uint32_t)key & 0xFFFFu, start = (uint32_t)(key >> 16) & 0xFFFFu, end = q - 1;
        i--;
        if (lane == 0 && i < W) {
            const uint32_t acc = (uint32_t)(key >> 32) - a.word_cost - E[start];
            words[i] = sr_chain_word{a.word_id[a.group_of_slot[slot]], slot, start, end, acc, acc / (end - start + 1 + a.tpl_frames[slot]), E[q], 0u};
        }
        p = start;
    }
    if (lane == 0) a.rec[row] = sr_chain_rec{total, n, N - in_words, n > W ? SR_CH_TRUNCATED : SR_CH_OK};
}

void launch_onepass(const OnePassArgs &a, const OnePassBlock *blocks, uint32_t n_blocks, hipStream_t s)
{
    if (!a.n_rows || !a.K) return;
    const size_t lds = spot_lds_bytes(a.tpl_len);
    SR_LAUNCH_POINT(s, "k_onepass_init");
    hipLaunchKernelGGL(k_onepass_init, dim3(a.n_rows), dim3(256), 0, s, a);
    const dim3 grid(a.K, (a.n_rows + kSpotWaves - 1) / kSpotWaves);
    for (uint32_t b = 0; b < n_blocks; b++) {
        const OnePassBlock &o = blocks[b];
        SR_LAUNCH_POINT(s, "k_onepass_words");
        hipLaunchKernelGGL(k_onepass_words, grid, dim3(64 * kSpotWaves), lds, s, a, b ? o.c0_prev + 1u : 0u, o.c0, o.cN);
        SR_LAUNCH_POINT(s, "k_onepass_close");
        hipLaunchKernelGGL(k_onepass_close, dim3(a.n_rows), dim3(256), 0, s, a, o.c0, o.cN);
    }
    SR_LAUNCH_POINT(s, "k_onepass_trace");
    hipLaunchKernelGGL(k_onepass_trace, dim3(a.n_rows), dim3(64), 0, s, a);
}
const char *onepass_allow_lds(uint32_t bytes) { return allow_dynamic_lds({{(const void *)k_onepass_words, "k_onepass_words"}}, bytes); }

}  // namespace sr
