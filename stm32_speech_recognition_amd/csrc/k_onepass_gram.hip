// k_onepass_gram.hip -- one-pass grammar decoding (include/sr_engine.h, "one-pass grammar decoding"): k_onepass.hip's ONE
// prefix-cost array, kept per state of a grammar, so a row holds any number of words of a word network and a call pays
// 2 x (kept items) x M x N cells whatever that number is.  OPT-IN EXTENSION, no reference counterpart.  gfx950 (MI355X, CDNA4)
// only; wave = 64 lanes; integer VALU + LDS.
//
// The block argument of k_onepass.hip holds state by state (sr_onepass_gram_plan.h): a word that starts inside a block of
// n <= L frames [c0, c0 + n) ends at or after c0 + n whatever state it leads into, so A(., t) and E(., t) over (c0, c0 + n]
// follow from E(., s) at or before c0 alone.  Per launch group:
//   k_onepass_gram_init     all-ones A of the kept states, E(0, 0) = 0 and E(0, s) unreachable;
//   per block [c0, cN) of the host's list, in stream order:
//   k_onepass_gram_words    k_onepass_words' resumed wavefront -- grid (kept item, groups of kSpotWaves rows), lane = column,
//                           the item's template in LDS -- from the saved column of (row, item).  The start charge of a column
//                           col <= c0 is taken in the kernel, as k_gram_live_words takes it: the minimum of E(col, s) over the
//                           item's charge list; a column behind c0 is unreachable.  Column c0 is saved; the end keys of the
//                           columns >= c0 go to A(col + 1, target) with the 64-bit atomic minimum;
//   k_onepass_gram_close    k_onepass_close per (row, kept state): E(., t) over (c0, cN] from the carried E(c0, t), closed even
//                           where no key arrived -- a state without an incoming arc still carries its filler;
//   k_onepass_gram_trace    one wave per row, walked twice (count, then write) with onepass_word_at on the A / E of the state
//                           the walk stands in, switching to the word's source state behind every word.
// A WEIGHTED grammar takes k_onepass_gram_words_w and k_onepass_gram_trace_w, with the costs in a second argument block; init
// and close serve it unchanged, and a grammar without a nonzero cost launches the unweighted kernels only.  No workgroup waits
// on another: the blocks are ordered by the stream alone.  Plain vector stores; the atomic minimum on A is the only atomic, and
// it does not depend on the order of the waves, so two runs give the same bytes.  The sweep, the close and the charge of a
// column are sr_sweep_dev.h's; the two sweeps are one body (opg_words), compiled with and without costs.
#include "sr_dtw_plan.h"
#include "sr_spot_dev.h"
#include "sr_sweep_dev.h"

namespace sr {

__device__ __forceinline__ uint32_t opg_frames(const OnePassArgs &o, uint32_t row)
{
    const uint32_t n = o.in_frames[(size_t)row * o.frames_stride];
    return n < o.frames_cap ? n : o.frames_cap;  // frames_cap <= max_frames
}
__device__ __forceinline__ unsigned long long *opg_A(const OnePassGramArgs &a, uint32_t row, uint32_t state)
{
    return a.o.A + ((size_t)row * a.n_states + state) * (a.o.max_frames + 1u);
}
__device__ __forceinline__ uint32_t *opg_E(const OnePassGramArgs &a, uint32_t row, uint32_t state)
{
    return a.o.E + ((size_t)row * a.n_states + state) * (a.o.max_frames + 1u);
}
__device__ __forceinline__ uint32_t opg_state(const OnePassGramArgs &a, uint32_t i) { return a.keep_states ? a.keep_states[i] : i; }

// grid (rows, kept states)
__global__ void __launch_bounds__(256) k_onepass_gram_init(const OnePassGramArgs a)
{
    const uint32_t row = blockIdx.x, state = opg_state(a, blockIdx.y), P = a.o.max_frames + 1u;
    unsigned long long *A = opg_A(a, row, state);
    for (uint32_t p = threadIdx.x; p < P; p += 256) A[p] = kSpotInf;
    if (threadIdx.x == 0) opg_E(a, row, state)[0] = state ? kChainNone : 0u;
}

// block [c0, cN) of every (kept item, row): the columns [xs, cN) with xs = c0_prev + 1, or 0 for the first block.  wt: null, or
// the costs of a weighted grammar (include/sr_engine.h, "weighted grammars"): the charge of a column is then taken over the
// item's charge list with the arc costs added
__device__ __forceinline__ void opg_words(const OnePassGramArgs &a, const GramCosts *wt, const uint32_t xs, const uint32_t c0, const uint32_t cN_blk)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 og_smem[];  // template rows [tpl_len][2], then the waves' boundary columns
    const GramItem it = a.items[a.keep_items ? a.keep_items[blockIdx.x] : blockIdx.x];
    const uint32_t k = it.slot, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t row = blockIdx.y * kSpotWaves + w;
    uint32_t M = a.o.tpl_valid[k] ? a.o.tpl_frames[k] : 0u;
    M = M < a.o.tpl_len ? M : a.o.tpl_len;
    ulonglong2 *s_col = (ulonglong2 *)(og_smem + (size_t)a.o.tpl_len * 2) + (size_t)w * a.o.tpl_len;  // (Dd, min(Dd, Dn)) per row
    sweep_stage_tpl(og_smem, a.o.tpl + (size_t)k * a.o.tpl_stride, M);
    __syncthreads();
    if (row >= a.o.n_rows || !M) return;  // (a grammar keeps items of valid slots only)
    const uint32_t N = opg_frames(a.o, row);
    if (N <= c0) return;  // (wave-uniform) the row ended before this block
    const uint32_t cN = cN_blk < N ? cN_blk : N, P = a.o.max_frames + 1u;  // the row may end inside the block

    ulonglong2 *g_col = a.o.cols + ((size_t)row * a.n_keep_items + blockIdx.x) * a.o.tpl_len;
    const uint32_t *E = opg_E(a, row, 0);  // state s at E + s * P
    const unsigned long long mask = a.masks[it.set];
    const uint32_t *cost = gram_costs_of(wt, it.set);  // by ascending state, as the mask is walked
    unsigned long long *A = opg_A(a, row, it.target);
    if (xs) {  // resume: the saved column, that of xs - 1 (16-byte loads, coalesced over template rows)
        for (uint32_t r = lane; r < M; r += 64) s_col[r] = g_col[r];
        wave_sync();
    }
    const int16_t *in = a.o.mfcc + (size_t)row * a.o.max_frames * kCoef;
    for (uint32_t x0 = xs; x0 < cN; x0 += 64) {  // (wave-uniform)
        const uint32_t col = x0 + lane;
        const bool live = col < cN;
        const uint32_t last = (cN - x0 < 64u ? cN - x0 : 64u) - 1;  // the sweep's last live lane: its column is handed on
        const bool keep = col == c0;                                // the exact column the next block resumes from
        Row32 fi = row_from2(u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, 0u);
        if (live) fi = sweep_frame(in + (size_t)col * kCoef);
        // C(col): what a word that starts in this column builds on, the cheapest state of the charge list; final for col <= c0,
        // none yet inside the block (col <= c0 < N <= max_frames: inside the state's row)
        const uint32_t charge = gram_charge(E, P, col, live && col <= c0, mask, cost);
        SweepLane sw;
        for (uint32_t t = 0; t < M + last; t++)
            sweep_step(og_smem, s_col, g_col, keep, fi, charge, col, live, x0 != 0, last, M, lane, t, sw);
        wave_sync();  // the boundary column is complete before the next sweep's lane 0 reads it

        // the key of each end frame of the block: (cost + word_cost, start, slot) -> A(col + 1, target); col + 1 <= cN <= max_frames
        if (live && col >= c0 && sw.end_v != kSpotInf) atomicMin(&A[col + 1], sweep_end_key(sw.end_v, a.o.word_cost, k));
    }
}

__global__ void __launch_bounds__(64 * kSpotWaves) k_onepass_gram_words(const OnePassGramArgs a, const uint32_t xs, const uint32_t c0,
                                                                        const uint32_t cN_blk)
{
    opg_words(a, nullptr, xs, c0, cN_blk);
}
__global__ void __launch_bounds__(64 * kSpotWaves) k_onepass_gram_words_w(const OnePassGramArgs a, const GramCosts wt, const uint32_t xs,
                                                                          const uint32_t c0, const uint32_t cN_blk)
{
    opg_words(a, &wt, xs, c0, cN_blk);
}

// k_onepass_close per (row, kept state); grid (rows, kept states).  E(p, t), p in (c0, cN], as a prefix minimum of A(j, t).cost +
// (cN - j) * skip in u64 that starts from the carried E(c0, t) + (cN - c0) * skip, less (cN - p) * skip.  A state no key arrived
// in is closed all the same: its filler, or unreachable.
__global__ void __launch_bounds__(256) k_onepass_gram_close(const OnePassGramArgs a, const uint32_t c0, const uint32_t cN_blk)
{
    __shared__ uint64_t s_tot[4];
    const uint32_t row = blockIdx.x;
    const uint32_t state = opg_state(a, blockIdx.y);
    const uint32_t N = opg_frames(a.o, row);
    if (N <= c0) return;  // (uniform)
    const uint32_t cN = cN_blk < N ? cN_blk : N;
    const unsigned long long *A = opg_A(a, row, state);
    uint32_t *E = opg_E(a, row, state);
    close_window(A, E, c0, cN, a.o.skip_cost, s_tot);
}

// the item (slot, t) by bisection of the items, which ascend by (slot, target): its index, or n_items
__device__ __forceinline__ uint32_t opg_item_of(const OnePassGramArgs &a, uint32_t slot, uint32_t t)
{
    uint32_t lo = 0, hi = a.n_items;
    const uint64_t want = ((uint64_t)slot << 32) | t;
    while (lo < hi) {  // (uniform)
        const uint32_t mid = lo + (hi - lo) / 2;
        const GramItem it = a.items[mid];
        if ((((uint64_t)it.slot << 32) | it.target) < want) lo = mid + 1;
        else hi = mid;
    }
    if (lo < a.n_items) {
        const GramItem it = a.items[lo];
        if (it.slot == slot && it.target == t) return lo;
    }
    return a.n_items;
}

// One step of the walk, all lanes alike: the word that closes E(., t) at or below p.  Returns its end position q (0: the rest
// is filler) with its key, the charge it started from and the smallest state of its charge list that carries that charge; wt
// null: no costs.  *bad is set where A, E and the items disagree, which cannot happen.
__device__ __forceinline__ uint32_t opg_step(const OnePassGramArgs &a, const GramCosts *wt, uint32_t row, uint32_t p, uint32_t t, uint32_t lane,
                                             uint64_t *key, uint32_t *charge, uint32_t *src, bool *bad)
{
    *key = kSpotInf;
    const uint32_t q = onepass_word_at(opg_A(a, row, t), opg_E(a, row, t), p, lane, key);
    if (!q) return 0u;
    const uint32_t slot = (uint32_t)*key & 0xFFFFu, start = (uint32_t)(*key >> 16) & 0xFFFFu;
    const uint32_t at = opg_item_of(a, slot, t);
    if (at == a.n_items) {
        *bad = true;
        return 0u;
    }
    const uint32_t set = a.items[at].set;
    const uint32_t *ac = wt ? wt->cost + wt->cost_off[set] : nullptr;
    uint32_t c = kChainNone, s0 = 0;
    for (unsigned long long m = a.masks[set]; m; m &= m - 1) {  // (uniform; ascending states)
        const uint32_t s = (uint32_t)__ffsll((long long)m) - 1u;
        const uint32_t e = opg_E(a, row, s)[start], v = ac ? e + *ac++ : e;
        if (e != kChainNone && v < c) c = v, s0 = s;
    }
    *charge = c;
    *src = s0;
    return q;
}

// one wave per row: the end state, then the history walked twice, first for the count, then for the words in spoken order
__device__ __forceinline__ void opg_trace_row(const OnePassGramArgs &a, const GramCosts *wt, uint32_t row, uint32_t lane)
{
    const uint32_t W = a.o.words_cap;
    const uint32_t N = opg_frames(a.o, row);
    sr_chain_word *words = a.o.words + (size_t)row * W;
    const sr_chain_word none = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    // the cheapest final state, its final cost included, the smallest state among equals (the kept states ascend)
    uint32_t total = kChainNone, fin = 0;
    for (uint32_t i = 0; N && i < a.n_keep_states; i++) {  // (uniform)
        const uint32_t f = opg_state(a, i);
        if (!a.final_state[f]) continue;
        const uint32_t e = opg_E(a, row, f)[N];
        if (e == kChainNone) continue;  // an unreachable state takes no cost
        const uint32_t v = wt ? e + wt->final_cost[f] : e;
        if (v < total) total = v, fin = f;
    }
    if (total == kChainNone) {  // (uniform) an empty row or no parse
        for (uint32_t i = lane; i < W; i += 64) words[i] = none;
        if (lane == 0) a.o.rec[row] = sr_chain_rec{kChainNone, 0u, 0u, SR_CH_NONE};
        return;
    }
    uint32_t n = 0, in_words = 0;
    bool bad = false;
    for (uint32_t p = N, t = fin; p;) {  // (uniform) the count; every start lies below its end position: the walk ends
        uint64_t key;
        uint32_t charge = 0, src = 0;
        const uint32_t q = opg_step(a, wt, row, p, t, lane, &key, &charge, &src, &bad);
        if (!q) break;
        const uint32_t start = (uint32_t)(key >> 16) & 0xFFFFu;
        n++;
        in_words += q - start;  // frames start .. q - 1
        p = start;
        t = src;
    }
    if (bad) {  // leave a whole record that says so
        for (uint32_t i = lane; i < W; i += 64) words[i] = none;
        if (lane == 0) a.o.rec[row] = sr_chain_rec{kChainNone, 0u, 0u, SR_CH_NONE};
        return;
    }
    for (uint32_t i = (n < W ? n : W) + lane; i < W; i += 64) words[i] = none;
    uint32_t i = n;
    for (uint32_t p = N, t = fin; p;) {
        uint64_t key;
        uint32_t charge = 0, src = 0;
        const uint32_t q = opg_step(a, wt, row, p, t, lane, &key, &charge, &src, &bad);
        if (!q) break;
        const uint32_t slot = (uint32_t)key & 0xFFFFu, start = (uint32_t)(key >> 16) & 0xFFFFu, end = q - 1;
        i--;
        if (lane == 0 && i < W) {
            const uint32_t cum = (uint32_t)(key >> 32), acc = cum - a.o.word_cost - charge;
            words[i] = sr_chain_word{a.o.word_id[a.o.group_of_slot[slot]], slot, start, end, acc, acc / (end - start + 1 + a.o.tpl_frames[slot]), cum, t};
        }
        p = start;
        t = src;
    }
    if (lane == 0) a.o.rec[row] = sr_chain_rec{total, n, N - in_words, n > W ? SR_CH_TRUNCATED : SR_CH_OK};
}

__global__ void __launch_bounds__(64) k_onepass_gram_trace(const OnePassGramArgs a) { opg_trace_row(a, nullptr, blockIdx.x, threadIdx.x); }
// under costs: the final cost at the end, the charge and the source state of a word judged on E + the arc cost
__global__ void __launch_bounds__(64) k_onepass_gram_trace_w(const OnePassGramArgs a, const GramCosts wt) { opg_trace_row(a, &wt, blockIdx.x, threadIdx.x); }

void launch_onepass_gram(const OnePassGramArgs &a, const GramCosts *w, const OnePassBlock *blocks, uint32_t n_blocks, hipStream_t s)
{
    if (!a.o.n_rows) return;
    const size_t lds = spot_lds_bytes(a.o.tpl_len);
    if (a.n_keep_states) {
        SR_LAUNCH_POINT(s, "k_onepass_gram_init");
        hipLaunchKernelGGL(k_onepass_gram_init, dim3(a.o.n_rows, a.n_keep_states), dim3(256), 0, s, a);
    }
    const dim3 grid(a.n_keep_items, (a.o.n_rows + kSpotWaves - 1) / kSpotWaves);
    for (uint32_t b = 0; b < n_blocks; b++) {
        const OnePassBlock &o = blocks[b];
        const uint32_t xs = b ? o.c0_prev + 1u : 0u;
        if (a.n_keep_items) {
            if (w) {
                SR_LAUNCH_POINT(s, "k_onepass_gram_words_w");
                hipLaunchKernelGGL(k_onepass_gram_words_w, grid, dim3(64 * kSpotWaves), lds, s, a, *w, xs, o.c0, o.cN);
            } else {
                SR_LAUNCH_POINT(s, "k_onepass_gram_words");
                hipLaunchKernelGGL(k_onepass_gram_words, grid, dim3(64 * kSpotWaves), lds, s, a, xs, o.c0, o.cN);
            }
        }
        if (a.n_keep_states) {
            SR_LAUNCH_POINT(s, "k_onepass_gram_close");
            hipLaunchKernelGGL(k_onepass_gram_close, dim3(a.o.n_rows, a.n_keep_states), dim3(256), 0, s, a, o.c0, o.cN);
        }
    }
    if (w) {
        SR_LAUNCH_POINT(s, "k_onepass_gram_trace_w");
        hipLaunchKernelGGL(k_onepass_gram_trace_w, dim3(a.o.n_rows), dim3(64), 0, s, a, *w);
    } else {
        SR_LAUNCH_POINT(s, "k_onepass_gram_trace");
        hipLaunchKernelGGL(k_onepass_gram_trace, dim3(a.o.n_rows), dim3(64), 0, s, a);
    }
}
const char *onepass_gram_allow_lds(uint32_t bytes)
{
    return allow_dynamic_lds({{(const void *)k_onepass_gram_words, "k_onepass_gram_words"}, {(const void *)k_onepass_gram_words_w, "k_onepass_gram_words_w"}},
                             bytes);
}

}  // namespace sr
