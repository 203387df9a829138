// k_gram_live.hip -- live grammar-constrained decoding (include/sr_engine.h, "live grammar-constrained decoding"): the levels
// of k_gram.hip, resumed from push to push as k_chain_live.hip resumes those of k_chain.hip.  OPT-IN EXTENSION, no reference
// counterpart.  gfx950 (MI355X, CDNA4) only; wave = 64 lanes; integer VALU + LDS.
//
// The exactness argument of k_chain_live.hip carries over state by state: column x of an item needs column x - 1 and the
// charge at x, which is a minimum over E_{l-1}(x, s); A_l(p, t) and E_l(p, t) depend on frames < p only, so the history of a
// recording is a prefix of the history of any longer one; count, end state and trace read A, E and N.  A push that appends
// frames [x0, x0 + n) is, on one stream:
//   k_gram_live_init     the new positions (x0, x0 + n] of every level and state (position 0 too for a fresh channel): E_0 of
//                        state 0 by the skip rule, every other E unreachable, every A all ones.  States that are no target at
//                        a level, and levels without items, are never written again: they stay unreachable;
//   per level l that keeps items:
//   k_gram_live_words    k_chain_live_words' resumed sweep -- grid (the level's items, groups of kSpotWaves channels) -- with
//                        the slot and the target from the item, the boundary column of (channel, level, item) in and out, the
//                        charge of a column taken in the kernel as the minimum of E_{l-1}(col, s) over the item's from-set,
//                        and the 64-bit atomic minimum of every new end frame's key into A_l(col + 1, target);
//   k_gram_live_close    E_l(., t) over (x0, x0 + n] from the carried E_l(x0, t), per target state of the level;
//   k_gram_live_trace    k_gram_trace's walk with N = x0 + n into the compact row the host assigned.
// There is no charge kernel and no row of charges: a push has few columns, a launch more per level would cost more than the
// loads it saves.  No workgroup waits on another: the levels are ordered by the stream alone.  Plain vector stores; the atomic
// minimum on A is the only atomic, and it does not depend on the order of the waves, so two runs give the same bytes.  The
// staging, the frame load, the key and the close are sr_sweep_dev.h's; k_gram_live_words keeps its charge and its step loop.
//
// A WEIGHTED grammar (include/sr_engine.h, "weighted grammars") takes k_gram_live_words_w and k_gram_live_trace_w, with the
// costs in a second argument block, in the places of the sweep and the trace; init and close serve it unchanged.  A grammar
// without a nonzero cost launches exactly what it always has.
#include "sr_dtw_plan.h"
#include "sr_spot_dev.h"
#include "sr_sweep_dev.h"

namespace sr {

__device__ __forceinline__ unsigned long long *gram_live_A(const GramLiveArgs &a, uint32_t c, uint32_t level, uint32_t state)  // level 1..max_words
{
    return a.c.A + (((size_t)c * a.c.max_words + (level - 1)) * a.n_states + state) * a.c.P;
}
__device__ __forceinline__ uint32_t *gram_live_E(const GramLiveArgs &a, uint32_t c, uint32_t level, uint32_t state)  // level 0..max_words
{
    return a.c.E + (((size_t)c * (a.c.max_words + 1u) + level) * a.n_states + state) * a.c.P;
}

// the new positions of level blockIdx.y in every state; grid (channels, max_words + 1)
__global__ void __launch_bounds__(256) k_gram_live_init(const GramLiveArgs a)
{
    const uint32_t c = blockIdx.x, l = blockIdx.y;
    const SpotLiveChan ch = a.c.chan[c];
    if (!ch.n) return;
    const bool skip = a.c.skip_cost != kChainNone;
    const uint32_t p0 = ch.x0 ? ch.x0 + 1 : 0u, cnt = ch.x0 + ch.n - p0 + 1;  // positions [p0, p0 + cnt), the last <= utt_frames = P - 1
    uint32_t *E = gram_live_E(a, c, l, 0);
    unsigned long long *A = l ? gram_live_A(a, c, l, 0) : nullptr;
    for (uint32_t i = threadIdx.x; i < a.n_states * cnt; i += 256) {
        const uint32_t s = i / cnt, p = p0 + (i - s * cnt);
        const size_t at = (size_t)s * a.c.P + p;
        E[at] = (l || s) ? kChainNone : (skip ? p * a.c.skip_cost : (p ? kChainNone : 0u));
        if (l) A[at] = kSpotInf;
    }
}

// The sweep of one level.  This kernel holds its whole body, the charge of a column and the step loop included, and shares
// only the staging, the frame load and the key (sr_sweep_dev.h): as one inline body with its weighted twin, behind a one-line
// kernel, its step loop had one v_add more than unshared and it measured 0.2 to 0.5 % slower (profiles/experiments/RESULTS.md).
__global__ void __launch_bounds__(64 * kSpotWaves) k_gram_live_words(const GramLiveArgs a, const uint32_t level)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 gl_smem[];  // template rows [tpl_len][2], then the waves' boundary columns
    const GramItem it = a.items[a.lists[a.lv[level - 1].item0 + blockIdx.x]];
    const uint32_t k = it.slot, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.y * kSpotWaves + w;
    uint32_t M = a.c.tpl_valid[k] ? a.c.tpl_frames[k] : 0u;
    M = M < a.c.tpl_len ? M : a.c.tpl_len;
    ulonglong2 *s_col = (ulonglong2 *)(gl_smem + (size_t)a.c.tpl_len * 2) + (size_t)w * a.c.tpl_len;  // (Dd, min(Dd, Dn)) per row
    sweep_stage_tpl(gl_smem, a.c.tpl + (size_t)k * a.c.tpl_stride, M);
    __syncthreads();
    if (c >= a.c.C || !M) return;  // (a grammar keeps items of valid slots only)
    const SpotLiveChan ch = a.c.chan[c];
    if (!ch.n) return;  // (wave-uniform) a silent channel is not touched

    const uint32_t xs = ch.x0, cN = ch.x0 + ch.n;  // the new columns [xs, cN), absolute; cN <= utt_frames
    ulonglong2 *g_col = a.c.cols + (((size_t)c * a.columns + a.col_off[level - 1] + blockIdx.x)) * a.c.tpl_len;
    const uint32_t *e_prev = gram_live_E(a, c, level - 1, 0);  // state s at e_prev + s * P
    const unsigned long long mask = a.masks[it.set];
    unsigned long long *A = gram_live_A(a, c, level, it.target);
    if (xs) {  // resume: the saved column (16-byte loads, coalesced over template rows)
        for (uint32_t r = lane; r < M; r += 64) s_col[r] = g_col[r];
        wave_sync();
    }
    const int16_t *in = a.c.mfcc + (uint64_t)c * a.c.row_stride;
    for (uint32_t x0 = xs; x0 < cN; x0 += 64) {  // (wave-uniform)
        const uint32_t col = x0 + lane;
        const bool live = col < cN;
        const uint32_t last = (cN - x0 < 64u ? cN - x0 : 64u) - 1;  // the sweep's last live lane: its column is handed on
        Row32 fi = row_from2(u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, 0u);
        if (live) fi = sweep_frame(in + (size_t)(col - xs) * kCoef);
        // C_l(col): what a word that starts in this column builds on, the cheapest state of the from-set
        uint32_t charge = kChainNone;
        for (unsigned long long m = mask; m; m &= m - 1) {  // (wave-uniform; col <= utt_frames - 1 where live)
            const uint32_t s = (uint32_t)__ffsll((long long)m) - 1u;
            const uint32_t e = live ? e_prev[(size_t)s * a.c.P + col] : kChainNone;
            charge = e < charge ? e : charge;
        }
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
                const Row32 fm = row_from(gl_smem[2 * r], gl_smem[2 * r + 1]);
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

        // the key of each new end frame: (cost + word_cost, start, slot) -> A_l(col + 1, target); col + 1 <= cN <= utt_frames
        if (live && end_v != kSpotInf) atomicMin(&A[col + 1], sweep_end_key(end_v, a.c.word_cost, k));
    }
    // the state for the next push: column cN - 1 (16-byte stores, coalesced over template rows)
    for (uint32_t r = lane; r < M; r += 64) g_col[r] = s_col[r];
}


// k_gram_live_words under costs (include/sr_engine.h, "weighted grammars"): the same resumed sweep, the charge of a column
// taken over the item's charge list with the arc costs added (gram_charge), the step sweep_step.
__global__ void __launch_bounds__(64 * kSpotWaves) k_gram_live_words_w(const GramLiveArgs a, const GramCosts wt, const uint32_t level)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 glw_smem[];  // template rows [tpl_len][2], then the waves' boundary columns
    const GramItem it = a.items[a.lists[a.lv[level - 1].item0 + blockIdx.x]];
    const uint32_t k = it.slot, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.y * kSpotWaves + w;
    uint32_t M = a.c.tpl_valid[k] ? a.c.tpl_frames[k] : 0u;
    M = M < a.c.tpl_len ? M : a.c.tpl_len;
    ulonglong2 *s_col = (ulonglong2 *)(glw_smem + (size_t)a.c.tpl_len * 2) + (size_t)w * a.c.tpl_len;  // (Dd, min(Dd, Dn)) per row
    sweep_stage_tpl(glw_smem, a.c.tpl + (size_t)k * a.c.tpl_stride, M);
    __syncthreads();
    if (c >= a.c.C || !M) return;  // (a grammar keeps items of valid slots only)
    const SpotLiveChan ch = a.c.chan[c];
    if (!ch.n) return;  // (wave-uniform) a silent channel is not touched

    const uint32_t xs = ch.x0, cN = ch.x0 + ch.n;  // the new columns [xs, cN), absolute; cN <= utt_frames
    ulonglong2 *g_col = a.c.cols + (((size_t)c * a.columns + a.col_off[level - 1] + blockIdx.x)) * a.c.tpl_len;
    const uint32_t *e_prev = gram_live_E(a, c, level - 1, 0);  // state s at e_prev + s * P
    const unsigned long long mask = a.masks[it.set];
    const uint32_t *cost = gram_costs_of(&wt, it.set);  // by ascending state, as the mask is walked
    unsigned long long *A = gram_live_A(a, c, level, it.target);
    if (xs) {  // resume: the saved column (16-byte loads, coalesced over template rows)
        for (uint32_t r = lane; r < M; r += 64) s_col[r] = g_col[r];
        wave_sync();
    }
    const int16_t *in = a.c.mfcc + (uint64_t)c * a.c.row_stride;
    for (uint32_t x0 = xs; x0 < cN; x0 += 64) {  // (wave-uniform)
        const uint32_t col = x0 + lane;
        const bool live = col < cN;
        const uint32_t last = (cN - x0 < 64u ? cN - x0 : 64u) - 1;  // the sweep's last live lane: its column is handed on
        Row32 fi = row_from2(u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, 0u);
        if (live) fi = sweep_frame(in + (size_t)(col - xs) * kCoef);
        // C_l(col): the cheapest E + arc cost of the item's charge list (col <= utt_frames - 1 where live)
        const uint32_t charge = gram_charge(e_prev, a.c.P, col, live, mask, cost);
        SweepLane sw;
        for (uint32_t t = 0; t < M + last; t++)
            sweep_step(glw_smem, s_col, nullptr, false, fi, charge, col, live, x0 != 0, last, M, lane, t, sw);
        wave_sync();  // the boundary column is complete before the next sweep's lane 0, or the save below, reads it

        // the key of each new end frame: (cost + word_cost, start, slot) -> A_l(col + 1, target); col + 1 <= cN <= utt_frames
        if (live && sw.end_v != kSpotInf) atomicMin(&A[col + 1], sweep_end_key(sw.end_v, a.c.word_cost, k));
    }
    // the state for the next push: column cN - 1 (16-byte stores, coalesced over template rows)
    for (uint32_t r = lane; r < M; r += 64) g_col[r] = s_col[r];
}


// k_chain_live_close per (channel, target state of the level): E_l(p, t), p in (x0, x0 + n], as a prefix minimum of
// A_l(j, t).cost + (cN - j) * skip in u64 that starts from the carried E_l(x0, t) + (cN - x0) * skip, less (cN - p) * skip.
__global__ void __launch_bounds__(256) k_gram_live_close(const GramLiveArgs a, const uint32_t level)
{
    __shared__ uint64_t s_tot[4];
    const uint32_t c = blockIdx.x;
    const uint32_t state = a.lists[a.lv[level - 1].state0 + blockIdx.y];
    const SpotLiveChan ch = a.c.chan[c];
    if (!ch.n) return;  // (uniform)
    const uint32_t xs = ch.x0, cN = ch.x0 + ch.n;
    const unsigned long long *A = gram_live_A(a, c, level, state);
    uint32_t *E = gram_live_E(a, c, level, state);
    close_window(A, E, xs, cN, a.c.skip_cost, s_tot);
}

// One wave per emitting channel: k_gram_trace's level costs, count, end state and walk back through levels and states, with
// N = x0 + n, the session's history in the place of the scratch, into the channel's compact row.
__global__ void __launch_bounds__(64) k_gram_live_trace(const GramLiveArgs a)
{
    const uint32_t c = blockIdx.x, W = a.c.max_words, S = a.n_states, lane = threadIdx.x;
    const SpotLiveChan ch = a.c.chan[c];
    if (!ch.first_win) return;
    const uint32_t N = ch.x0 + ch.n;
    const size_t row = ch.row_base;
    sr_chain_rec *rec = a.c.rec + row;
    sr_chain_word *words = a.c.words + row * W;
    // L_l = the cheapest final state of level l = lane, the smallest state among equals; then the count as chain_trace_row
    uint32_t cost = kChainNone, fin = 0;
    if (N && lane >= 1 && lane <= W) {
        for (uint32_t f = 0; f < S; f++) {
            if (!a.final_state[f]) continue;
            const uint32_t e = gram_live_E(a, c, lane, f)[N];
            if (e < cost) cost = e, fin = f;
        }
    }
    if (a.c.level_cost && lane >= 1 && lane <= W) a.c.level_cost[row * W + lane - 1] = cost;
    uint32_t n = a.c.n_words_exact;
    if (!n) {
        uint64_t key = ((uint64_t)cost << 32) | lane;  // lanes without a level carry all-ones costs and lose to none of them
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) key = spot_min(key, spot_shfl(key, lane ^ (uint32_t)d));
        n = (uint32_t)(key >> 32) == kChainNone ? 1u : (uint32_t)key;
    }
    const uint32_t total = __shfl(cost, (int)n, 64);
    uint32_t t = __shfl(fin, (int)n, 64);
    const bool ok = total != kChainNone;
    const sr_chain_word none = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    for (uint32_t i = (ok ? n : 0u) + lane; i < W; i += 64) words[i] = none;
    if (!ok) {
        if (lane == 0) *rec = sr_chain_rec{kChainNone, 0u, 0u, SR_CH_NONE};
        return;
    }
    uint32_t p = N, in_words = 0;
    for (uint32_t l = n; l >= 1; l--) {  // (uniform)
        const unsigned long long *A = gram_live_A(a, c, l, t);
        const uint32_t *E = gram_live_E(a, c, l, t);
        // the first position at or below p whose own word closes E_l(., t) there; E_l(p, t) is finite, so there is one above 0
        uint64_t key = kSpotInf;
        uint32_t cum = 0;
        while (p >= 1) {
            const bool mine = lane < p;  // position p - lane >= 1
            const uint64_t ky = mine ? A[p - lane] : kSpotInf;
            const uint32_t e = mine ? E[p - lane] : kChainNone;
            const unsigned long long hit = __ballot(mine && ky != kSpotInf && (uint32_t)(ky >> 32) == e);
            if (hit) {
                const uint32_t first = (uint32_t)__ffsll((long long)hit) - 1u;
                key = spot_shfl(ky, first);
                cum = __shfl(e, (int)first, 64);
                p -= first;
                break;
            }
            p = p > 64u ? p - 64u : 0u;
        }
        const uint32_t slot = (uint32_t)key & 0xFFFFu, start = (uint32_t)(key >> 16) & 0xFFFFu, end = p - 1;
        // the item (slot, t) by bisection of the items, which ascend by (slot, target): its from-set
        uint32_t lo = 0, hi = a.n_items;
        const uint64_t want = ((uint64_t)slot << 32) | t;
        while (key != kSpotInf && lo < hi) {  // (uniform)
            const uint32_t mid = lo + (hi - lo) / 2;
            const GramItem it = a.items[mid];
            if ((((uint64_t)it.slot << 32) | it.target) < want) lo = mid + 1;
            else hi = mid;
        }
        bool found = false;
        if (key != kSpotInf && lo < a.n_items) {
            const GramItem it = a.items[lo];
            found = it.slot == slot && it.target == t;
        }
        if (!found) {  // cannot happen while A, E and the items agree; leave a whole record that says so
            for (uint32_t i = lane; i < W; i += 64) words[i] = none;
            if (lane == 0) *rec = sr_chain_rec{kChainNone, 0u, 0u, SR_CH_NONE};
            return;
        }
        // the charge the word started from and the smallest state of the from-set that carries it
        uint32_t charge = kChainNone, src = 0;
        for (unsigned long long m = a.masks[a.items[lo].set]; m; m &= m - 1) {  // (uniform; ascending states)
            const uint32_t s = (uint32_t)__ffsll((long long)m) - 1u;
            const uint32_t e = gram_live_E(a, c, l - 1, s)[start];
            if (e < charge) charge = e, src = s;
        }
        if (lane == 0) {
            const uint32_t acc = (uint32_t)(key >> 32) - a.c.word_cost - charge;
            words[l - 1] = sr_chain_word{a.c.word_id[a.c.group_of_slot[slot]], slot, start, end, acc,
                                         acc / (end - start + 1 + a.c.tpl_frames[slot]), cum, t};
        }
        in_words += end - start + 1;
        p = start;
        t = src;
    }
    if (lane == 0) *rec = sr_chain_rec{total, n, N - in_words, SR_CH_OK};
}

// k_gram_live_trace under costs, as k_gram_trace_w: L_l adds the final cost, the charge and the source state of a word are
// judged on E_{l-1} + the arc cost, both over reachable E only.  A kernel of its own beside k_gram_live_trace.
__global__ void __launch_bounds__(64) k_gram_live_trace_w(const GramLiveArgs a, const GramCosts wt)
{
    const uint32_t c = blockIdx.x, W = a.c.max_words, S = a.n_states, lane = threadIdx.x;
    const SpotLiveChan ch = a.c.chan[c];
    if (!ch.first_win) return;
    const uint32_t N = ch.x0 + ch.n;
    const size_t row = ch.row_base;
    sr_chain_rec *rec = a.c.rec + row;
    sr_chain_word *words = a.c.words + row * W;
    // L_l = the cheapest final state of level l = lane with its final cost, the smallest state among equals; then the count
    uint32_t cost = kChainNone, fin = 0;
    if (N && lane >= 1 && lane <= W) {
        for (uint32_t f = 0; f < S; f++) {
            if (!a.final_state[f]) continue;
            const uint32_t e = gram_live_E(a, c, lane, f)[N];
            if (e == kChainNone) continue;  // an unreachable state takes no cost
            const uint32_t v = e + wt.final_cost[f];
            if (v < cost) cost = v, fin = f;
        }
    }
    if (a.c.level_cost && lane >= 1 && lane <= W) a.c.level_cost[row * W + lane - 1] = cost;
    uint32_t n = a.c.n_words_exact;
    if (!n) {
        uint64_t key = ((uint64_t)cost << 32) | lane;  // lanes without a level carry all-ones costs and lose to none of them
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) key = spot_min(key, spot_shfl(key, lane ^ (uint32_t)d));
        n = (uint32_t)(key >> 32) == kChainNone ? 1u : (uint32_t)key;
    }
    const uint32_t total = __shfl(cost, (int)n, 64);
    uint32_t t = __shfl(fin, (int)n, 64);
    const bool ok = total != kChainNone;
    const sr_chain_word none = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    for (uint32_t i = (ok ? n : 0u) + lane; i < W; i += 64) words[i] = none;
    if (!ok) {
        if (lane == 0) *rec = sr_chain_rec{kChainNone, 0u, 0u, SR_CH_NONE};
        return;
    }
    uint32_t p = N, in_words = 0;
    for (uint32_t l = n; l >= 1; l--) {  // (uniform)
        const unsigned long long *A = gram_live_A(a, c, l, t);
        const uint32_t *E = gram_live_E(a, c, l, t);
        // the first position at or below p whose own word closes E_l(., t) there; E_l(p, t) is finite, so there is one above 0
        uint64_t key = kSpotInf;
        uint32_t cum = 0;
        while (p >= 1) {
            const bool mine = lane < p;  // position p - lane >= 1
            const uint64_t ky = mine ? A[p - lane] : kSpotInf;
            const uint32_t e = mine ? E[p - lane] : kChainNone;
            const unsigned long long hit = __ballot(mine && ky != kSpotInf && (uint32_t)(ky >> 32) == e);
            if (hit) {
                const uint32_t first = (uint32_t)__ffsll((long long)hit) - 1u;
                key = spot_shfl(ky, first);
                cum = __shfl(e, (int)first, 64);
                p -= first;
                break;
            }
            p = p > 64u ? p - 64u : 0u;
        }
        const uint32_t slot = (uint32_t)key & 0xFFFFu, start = (uint32_t)(key >> 16) & 0xFFFFu, end = p - 1;
        // the item (slot, t) by bisection of the items, which ascend by (slot, target): its from-set
        uint32_t lo = 0, hi = a.n_items;
        const uint64_t want = ((uint64_t)slot << 32) | t;
        while (key != kSpotInf && lo < hi) {  // (uniform)
            const uint32_t mid = lo + (hi - lo) / 2;
            const GramItem it = a.items[mid];
            if ((((uint64_t)it.slot << 32) | it.target) < want) lo = mid + 1;
            else hi = mid;
        }
        bool found = false;
        if (key != kSpotInf && lo < a.n_items) {
            const GramItem it = a.items[lo];
            found = it.slot == slot && it.target == t;
        }
        if (!found) {  // cannot happen while A, E and the items agree; leave a whole record that says so
            for (uint32_t i = lane; i < W; i += 64) words[i] = none;
            if (lane == 0) *rec = sr_chain_rec{kChainNone, 0u, 0u, SR_CH_NONE};
            return;
        }
        // the charge the word started from, arc cost included, and the smallest state of the list that carries it
        uint32_t charge = kChainNone, src = 0;
        const uint32_t set = a.items[lo].set;
        const uint32_t *ac = wt.cost + wt.cost_off[set];
        for (unsigned long long m = a.masks[set]; m; m &= m - 1) {  // (uniform; ascending states)
            const uint32_t s = (uint32_t)__ffsll((long long)m) - 1u;
            const uint32_t e = gram_live_E(a, c, l - 1, s)[start], v = e + *ac++;
            if (e != kChainNone && v < charge) charge = v, src = s;
        }
        if (lane == 0) {
            const uint32_t acc = (uint32_t)(key >> 32) - a.c.word_cost - charge;
            words[l - 1] = sr_chain_word{a.c.word_id[a.c.group_of_slot[slot]], slot, start, end, acc,
                                         acc / (end - start + 1 + a.c.tpl_frames[slot]), cum, t};
        }
        in_words += end - start + 1;
        p = start;
        t = src;
    }
    if (lane == 0) *rec = sr_chain_rec{total, n, N - in_words, SR_CH_OK};
}

void launch_gram_live(const GramLiveArgs &a, const GramCosts *w, hipStream_t s)
{
    if (!a.c.C) return;
    const size_t lds = spot_lds_bytes(a.c.tpl_len);
    SR_LAUNCH_POINT(s, "k_gram_live_init");
    hipLaunchKernelGGL(k_gram_live_init, dim3(a.c.C, a.c.max_words + 1u), dim3(256), 0, s, a);
    const uint32_t groups = (a.c.C + kSpotWaves - 1) / kSpotWaves;
    for (uint32_t l = 1; l <= a.c.max_words; l++) {
        const GramLevel &lv = a.lv[l - 1];
        if (!lv.n_items) continue;  // nothing can end here: the level stays unreachable
        if (w) {
            SR_LAUNCH_POINT(s, "k_gram_live_words_w");
            hipLaunchKernelGGL(k_gram_live_words_w, dim3(lv.n_items, groups), dim3(64 * kSpotWaves), lds, s, a, *w, l);
        } else {
            SR_LAUNCH_POINT(s, "k_gram_live_words");
            hipLaunchKernelGGL(k_gram_live_words, dim3(lv.n_items, groups), dim3(64 * kSpotWaves), lds, s, a, l);
        }
        SR_LAUNCH_POINT(s, "k_gram_live_close");
        hipLaunchKernelGGL(k_gram_live_close, dim3(a.c.C, lv.n_states), dim3(256), 0, s, a, l);
    }
    launch_gram_live_trace(a, w, s);
}
void launch_gram_live_trace(const GramLiveArgs &a, const GramCosts *w, hipStream_t s)
{
    if (!a.c.C) return;
    if (w) {
        SR_LAUNCH_POINT(s, "k_gram_live_trace_w");
        hipLaunchKernelGGL(k_gram_live_trace_w, dim3(a.c.C), dim3(64), 0, s, a, *w);
    } else {
        SR_LAUNCH_POINT(s, "k_gram_live_trace");
        hipLaunchKernelGGL(k_gram_live_trace, dim3(a.c.C), dim3(64), 0, s, a);
    }
}
const char *gram_live_allow_lds(uint32_t bytes)
{
    return allow_dynamic_lds({{(const void *)k_gram_live_words, "k_gram_live_words"}, {(const void *)k_gram_live_words_w, "k_gram_live_words_w"}}, bytes);
}

}  // namespace sr
