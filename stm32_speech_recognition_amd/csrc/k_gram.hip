// k_gram.hip -- grammar-constrained decoding: k_chain.hip's level building over a finite-state word network (include/
// sr_engine.h, "grammar-constrained decoding").  OPT-IN EXTENSION, no reference counterpart; the local distance is the
// reference's get_dis (DTW.C:45-62).  gfx950 (MI355X, CDNA4) only; wave = 64 lanes; no MFMA, integer VALU + LDS.
//
// Per row and per grammar state t the scratch keeps k_chain's arrays,
//   A_l(p, t)   the best last word INTO state t of a parse of in[0..p) into l words that ends at frame p - 1, as the key
//               cost << 32 | start << 16 | slot; all ones = none
//   E_l(p, t)   the cost of the best such parse with trailing frames skipped; SR_DIS_ERR = none
// and one row of charges per from-set, C(x) = min over the set's states s of E_{l-1}(x, s), rewritten for every level.  A call
// is k_gram_init, then per level that keeps items (k_gram_charge, k_gram_words, k_gram_close), then k_gram_trace, all on one
// stream.  An ITEM is one word pass: slot k into target state t, charged by the from-set of (t, word of k).  Because
// min_s (E(x, s) + path) = (min_s E(x, s)) + path, that one pass serves every arc of the word into t; the trace recovers the
// source state from E_{l-1} at the word's start column.
//
// k_gram_words is k_chain_words' sweep with three differences: grid.x runs over the level's items, the start row is charged
// from the item's C row, and the key goes to A_l of the item's target state.  A slot has one label, so a (slot, target) pair
// is one item at most and the u64 minimum over the items of a target is the (cost, start, slot) rule.  The sweep itself is
// sr_sweep_dev.h's, as in k_chain.hip.
//
// A WEIGHTED grammar (include/sr_engine.h, "weighted grammars": a cost on every arc and every final state) takes two kernels
// of its own, k_gram_charge_w and k_gram_trace_w, with the costs in a second argument block; init, sweep and close serve it
// unchanged, because the arc cost sits inside the charge: min_s (E(x, s) + c_s + path) = (min_s (E(x, s) + c_s)) + path.  A
// grammar without a nonzero cost launches exactly what it always has.
#include <algorithm>

#include "sr_dtw_plan.h"
#include "sr_spot_dev.h"
#include "sr_sweep_dev.h"

namespace sr {

__device__ __forceinline__ unsigned long long *gram_A(const GramArgs &a, uint32_t row, uint32_t level, uint32_t state)  // level 1..max_words
{
    return a.c.A + (((size_t)row * a.c.max_words + (level - 1)) * a.n_states + state) * (a.c.max_frames + 1u);
}
__device__ __forceinline__ uint32_t *gram_E(const GramArgs &a, uint32_t row, uint32_t level, uint32_t state)  // level 0..max_words
{
    return a.c.E + (((size_t)row * (a.c.max_words + 1u) + level) * a.n_states + state) * (a.c.max_frames + 1u);
}
__device__ __forceinline__ uint32_t *gram_C(const GramArgs &a, uint32_t row, uint32_t set)
{
    return a.C + ((size_t)row * a.n_sets + set) * (a.c.max_frames + 1u);
}
__device__ __forceinline__ uint32_t gram_frames(const GramArgs &a, uint32_t row)
{
    const uint32_t N = a.c.in_frames[(size_t)row * a.c.frames_stride];
    return N < a.c.max_frames ? N : a.c.max_frames;
}

// E_0 of state 0, unreachable in every other state and level, "no word yet" in every A; grid (rows, blocks that share a row)
__global__ void __launch_bounds__(256) k_gram_init(const GramArgs a)
{
    const uint32_t row = blockIdx.x, P = a.c.max_frames + 1u;
    const bool skip = a.c.skip_cost != kChainNone;
    uint32_t *E = gram_E(a, row, 0, 0);
    const size_t n_e = (size_t)(a.c.max_words + 1u) * a.n_states * P, n_a = (size_t)a.c.max_words * a.n_states * P;
    const size_t first = (size_t)blockIdx.y * 256u + threadIdx.x, step = (size_t)gridDim.y * 256u;
    for (size_t i = first; i < n_e; i += step) {
        const uint32_t p = (uint32_t)i;  // only used where i < P
        E[i] = i < P ? (skip ? p * a.c.skip_cost : (p ? kChainNone : 0u)) : kChainNone;
    }
    unsigned long long *A = gram_A(a, row, 1, 0);
    for (size_t i = first; i < n_a; i += step) A[i] = kSpotInf;
}

// the charges of the from-sets this level uses: grid (blocks of 256 positions, the level's from-sets, rows)
__global__ void __launch_bounds__(256) k_gram_charge(const GramArgs a, const uint32_t level)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, row = blockIdx.z, P = a.c.max_frames + 1u;
    if (x >= P) return;
    const uint32_t set = a.lists[a.lv[level - 1].set0 + blockIdx.y];
    const uint32_t *E = gram_E(a, row, level - 1, 0);
    uint32_t c = kChainNone;
    for (unsigned long long m = a.masks[set]; m; m &= m - 1) {  // (uniform)
        const uint32_t s = (uint32_t)__ffsll((long long)m) - 1u;
        const uint32_t e = E[(size_t)s * P + x];
        c = e < c ? e : c;
    }
    gram_C(a, row, set)[x] = c;
}

__global__ void __launch_bounds__(64 * kSpotWaves) k_gram_words(const GramArgs a, const uint32_t level)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 gr_smem[];  // template rows [tpl_len][2], then the waves' boundary columns
    const GramItem it = a.items[a.lists[a.lv[level - 1].item0 + blockIdx.x]];
    const uint32_t k = it.slot, row = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t chunk = blockIdx.z * kSpotWaves + w;
    uint32_t M = a.c.tpl_valid[k] ? a.c.tpl_frames[k] : 0u;
    M = M < a.c.tpl_len ? M : a.c.tpl_len;
    ulonglong2 *s_col = (ulonglong2 *)(gr_smem + (size_t)a.c.tpl_len * 2) + (size_t)w * a.c.tpl_len;  // (Dd, min(Dd, Dn)) per row
    sweep_stage_tpl(gr_smem, a.c.tpl + (size_t)k * a.c.tpl_stride, M);
    __syncthreads();
    if (chunk >= a.c.n_chunks || !M) return;

    const uint32_t N = gram_frames(a, row);
    const uint32_t c0 = chunk * a.c.chunk_cols;              // the chunk's end frames [c0, cN)
    const uint32_t c1 = c0 + a.c.chunk_cols, cN = c1 < N ? c1 : N;
    if (c0 >= cN) return;
    const int16_t *in = a.c.mfcc + (size_t)row * a.c.max_frames * kCoef;
    const uint32_t *e_prev = gram_C(a, row, it.set);
    unsigned long long *A = gram_A(a, row, level, it.target);
    const uint32_t cs = c0 > 2 * M - 2 ? c0 - (2 * M - 2) : 0u;  // the exact lead-in
    for (uint32_t x0 = cs; x0 < cN; x0 += 64) {  // (wave-uniform)
        const uint32_t col = x0 + lane;
        const bool live = col < cN;
        Row32 fi = row_from2(u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, 0u);
        uint32_t charge = kChainNone;  // C(col): what a word that starts in this column builds on
        if (live) {
            fi = sweep_frame(in + (size_t)col * kCoef);
            charge = e_prev[col];
        }
        const uint32_t end_lane = (cN - x0 < 64u ? cN - x0 : 64u) - 1;  // the sweep's last live lane
        SweepLane sw;
        for (uint32_t t = 0; t < M + end_lane; t++)
            sweep_step(gr_smem, s_col, nullptr, false, fi, charge, col, live, x0 != cs, 63, M, lane, t, sw);
        wave_sync();  // the boundary column is complete before the next sweep's lane 0 reads it

        // the key of each end frame of the chunk: (cost + word_cost, start, slot) -> A_l(col + 1, target); col + 1 <= N <= max_frames
        if (live && col >= c0 && sw.end_v != kSpotInf) atomicMin(&A[col + 1], sweep_end_key(sw.end_v, a.c.word_cost, k));
    }
}

// k_chain_close per (row, state): E_l(p, t) = min(A_l(p, t).cost, E_l(p-1, t) + skip), a prefix minimum of A_l(j).cost +
// (N - j) * skip in u64, less (N - p) * skip.  grid (rows, the level's target states); the other states stay unreachable.
__global__ void __launch_bounds__(256) k_gram_close(const GramArgs a, const uint32_t level)
{
    __shared__ uint64_t s_tot[4];
    const uint32_t row = blockIdx.x, P = a.c.max_frames + 1u, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t state = a.lists[a.lv[level - 1].state0 + blockIdx.y];
    const uint32_t N = gram_frames(a, row);
    const unsigned long long *A = gram_A(a, row, level, state);
    uint32_t *E = gram_E(a, row, level, state);
    if (a.c.skip_cost == kChainNone) {  // no skipping: the costs themselves (all ones stays SR_DIS_ERR)
        for (uint32_t p = threadIdx.x; p < P; p += 256) E[p] = p <= N ? (uint32_t)(A[p] >> 32) : kChainNone;
        return;
    }
    const uint64_t skip = a.c.skip_cost;
    uint64_t carry = kSpotInf;  // the minimum over every position before this block of 256
    for (uint32_t p0 = 0; p0 < P; p0 += 256) {  // (uniform)
        const uint32_t p = p0 + threadIdx.x;
        uint64_t v = kSpotInf;
        if (p >= 1 && p <= N) {
            const uint64_t key = A[p];
            if (key != kSpotInf) v = (key >> 32) + (uint64_t)(N - p) * skip;
        }
#pragma unroll
        for (uint32_t by = 1; by < 64; by <<= 1) {
            const uint64_t o = spot_shfl_up(v, by);
            if (lane >= by) v = spot_min(v, o);
        }
        if (lane == 63) s_tot[w] = v;
        __syncthreads();
        uint64_t m = spot_min(v, carry);
        for (uint32_t i = 0; i < w; i++) m = spot_min(m, s_tot[i]);
        if (p < P) E[p] = (p <= N && m != kSpotInf) ? (uint32_t)(m - (uint64_t)(N - p) * skip) : kChainNone;
        for (uint32_t i = 0; i < 4; i++) carry = spot_min(carry, s_tot[i]);
        __syncthreads();  // s_tot is read before the next block overwrites it
    }
}

// The level costs, the word count, the end state, the walk back through levels and states, the records.  One wave per row;
// chain_trace_row's walk (sr_spot_dev.h) with a state that changes from word to word.
__global__ void __launch_bounds__(64) k_gram_trace(const GramArgs a)
{
    const uint32_t row = blockIdx.x, W = a.c.max_words, S = a.n_states, lane = threadIdx.x;
    const uint32_t N = gram_frames(a, row);
    sr_chain_rec *rec = a.c.rec + row;
    sr_chain_word *words = a.c.words + (size_t)row * W;
    // L_l = the cheapest final state of level l = lane, the smallest state among equals; then the count as chain_trace_row
    uint32_t c = kChainNone, fin = 0;
    if (N && lane >= 1 && lane <= W) {
        for (uint32_t f = 0; f < S; f++) {
            if (!a.final_state[f]) continue;
            const uint32_t e = gram_E(a, row, lane, f)[N];
            if (e < c) c = e, fin = f;
        }
    }
    if (a.c.level_cost && lane >= 1 && lane <= W) a.c.level_cost[(size_t)row * W + lane - 1] = c;
    uint32_t n = a.c.n_words_exact;
    if (!n) {
        uint64_t key = ((uint64_t)c << 32) | lane;  // lanes without a level carry all-ones costs and lose to none of them
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) key = spot_min(key, spot_shfl(key, lane ^ (uint32_t)d));
        n = (uint32_t)(key >> 32) == kChainNone ? 1u : (uint32_t)key;
    }
    const uint32_t total = __shfl(c, (int)n, 64);
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
        const unsigned long long *A = gram_A(a, row, l, t);
        const uint32_t *E = gram_E(a, row, l, t);
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
            const uint32_t e = gram_E(a, row, l - 1, s)[start];
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

// k_gram_charge under costs: one row of charges per distinct charge list, C(x) = min over the list's (s, c) with E_{l-1}(x, s)
// reachable of E_{l-1}(x, s) + c.  An unreachable E takes no cost: all ones + c would wrap to c - 1 and win every minimum.
// Same grid; a kernel of its own beside k_gram_charge.
__global__ void __launch_bounds__(256) k_gram_charge_w(const GramArgs a, const GramCosts wt, const uint32_t level)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, row = blockIdx.z, P = a.c.max_frames + 1u;
    if (x >= P) return;
    const uint32_t set = a.lists[a.lv[level - 1].set0 + blockIdx.y];
    const uint32_t *E = gram_E(a, row, level - 1, 0);
    const uint32_t *cost = wt.cost + wt.cost_off[set];
    uint32_t c = kChainNone;
    for (unsigned long long m = a.masks[set]; m; m &= m - 1) {  // (uniform; ascending states, as the costs are stored)
        const uint32_t s = (uint32_t)__ffsll((long long)m) - 1u;
        const uint32_t e = E[(size_t)s * P + x], v = e + *cost++;
        c = (e != kChainNone && v < c) ? v : c;
    }
    gram_C(a, row, set)[x] = c;
}

// k_gram_trace under costs: L_l adds the final cost of the state it ends in, the charge of a word and its source state are
// judged on E_{l-1} + the arc cost, both over finite E only.  A kernel of its own beside k_gram_trace.
__global__ void __launch_bounds__(64) k_gram_trace_w(const GramArgs a, const GramCosts wt)
{
    const uint32_t row = blockIdx.x, W = a.c.max_words, S = a.n_states, lane = threadIdx.x;
    const uint32_t N = gram_frames(a, row);
    sr_chain_rec *rec = a.c.rec + row;
    sr_chain_word *words = a.c.words + (size_t)row * W;
    // L_l = the cheapest final state of level l = lane with its final cost, the smallest state among equals; then the count
    uint32_t c = kChainNone, fin = 0;
    if (N && lane >= 1 && lane <= W) {
        for (uint32_t f = 0; f < S; f++) {
            if (!a.final_state[f]) continue;
            const uint32_t e = gram_E(a, row, lane, f)[N];
            if (e == kChainNone) continue;  // an unreachable state takes no cost: all ones + cost would wrap
            const uint32_t v = e + wt.final_cost[f];
            if (v < c) c = v, fin = f;
        }
    }
    if (a.c.level_cost && lane >= 1 && lane <= W) a.c.level_cost[(size_t)row * W + lane - 1] = c;
    uint32_t n = a.c.n_words_exact;
    if (!n) {
        uint64_t key = ((uint64_t)c << 32) | lane;  // lanes without a level carry all-ones costs and lose to none of them
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) key = spot_min(key, spot_shfl(key, lane ^ (uint32_t)d));
        n = (uint32_t)(key >> 32) == kChainNone ? 1u : (uint32_t)key;
    }
    const uint32_t total = __shfl(c, (int)n, 64);
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
        const unsigned long long *A = gram_A(a, row, l, t);
        const uint32_t *E = gram_E(a, row, l, t);
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
        const uint32_t *cost = wt.cost + wt.cost_off[set];
        for (unsigned long long m = a.masks[set]; m; m &= m - 1) {  // (uniform; ascending states)
            const uint32_t s = (uint32_t)__ffsll((long long)m) - 1u;
            const uint32_t e = gram_E(a, row, l - 1, s)[start], ac = *cost++;
            if (e != kChainNone && e + ac < charge) charge = e + ac, src = s;
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

void launch_gram(const GramArgs &a, const GramCosts *w, hipStream_t s)
{
    if (!a.c.n_rows) return;
    const size_t lds = spot_lds_bytes(a.c.tpl_len);
    const uint32_t P = a.c.max_frames + 1u;
    const size_t n_e = (size_t)(a.c.max_words + 1u) * a.n_states * P;
    SR_LAUNCH_POINT(s, "k_gram_init");
    hipLaunchKernelGGL(k_gram_init, dim3(a.c.n_rows, (uint32_t)std::min<size_t>((n_e + 4095u) / 4096u, 64u)), dim3(256), 0, s, a);
    for (uint32_t l = 1; l <= a.c.max_words; l++) {
        const GramLevel &lv = a.lv[l - 1];
        if (!lv.n_items) continue;  // nothing can end here: the level stays unreachable
        const dim3 charge_grid((P + 255u) / 256u, lv.n_sets, a.c.n_rows);
        if (w) {
            SR_LAUNCH_POINT(s, "k_gram_charge_w");
            hipLaunchKernelGGL(k_gram_charge_w, charge_grid, dim3(256), 0, s, a, *w, l);
        } else {
            SR_LAUNCH_POINT(s, "k_gram_charge");
            hipLaunchKernelGGL(k_gram_charge, charge_grid, dim3(256), 0, s, a, l);
        }
        SR_LAUNCH_POINT(s, "k_gram_words");
        hipLaunchKernelGGL(k_gram_words, dim3(lv.n_items, a.c.n_rows, (a.c.n_chunks + kSpotWaves - 1) / kSpotWaves), dim3(64 * kSpotWaves), lds, s,
                           a, l);
        SR_LAUNCH_POINT(s, "k_gram_close");
        hipLaunchKernelGGL(k_gram_close, dim3(a.c.n_rows, lv.n_states), dim3(256), 0, s, a, l);
    }
    if (w) {
        SR_LAUNCH_POINT(s, "k_gram_trace_w");
        hipLaunchKernelGGL(k_gram_trace_w, dim3(a.c.n_rows), dim3(64), 0, s, a, *w);
    } else {
        SR_LAUNCH_POINT(s, "k_gram_trace");
        hipLaunchKernelGGL(k_gram_trace, dim3(a.c.n_rows), dim3(64), 0, s, a);
    }
}
const char *gram_allow_lds(uint32_t bytes) { return allow_dynamic_lds({{(const void *)k_gram_words, "k_gram_words"}}, bytes); }

}  // namespace sr
