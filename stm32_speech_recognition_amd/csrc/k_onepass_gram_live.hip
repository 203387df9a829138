// k_onepass_gram_live.hip -- live one-pass grammar decoding (include/sr_engine.h, "live one-pass grammar decoding"):
// k_onepass_gram.hip's blocks with the boundaries set by the caller's pushes, per channel and of unequal length, as
// k_onepass_live.hip sets them for the decoder without a grammar.  OPT-IN EXTENSION, no reference counterpart.  gfx950 (MI355X,
// CDNA4) only; wave = 64 lanes; integer VALU + LDS.
//
// The block argument holds state by state (sr_onepass_gram_plan.h) and whatever the lengths of the blocks before (k_onepass_live
// .hip): a word that starts inside a block of at most L frames cannot end inside it whatever state it leads into, so A(., t) and
// E(., t) over a block follow from E(., s) at or before its first frame.  A channel keeps A and E of every state over its whole
// recording, dense by state index, per kept item the EXACT column at the first frame c0 of the block swept last, and its feature
// row.  A push that appends the frames [x0, x0 + n) is, per block b = 0.. of `block` <= L frames, in stream order:
//   k_onepass_gram_live_words   k_onepass_gram_words with (xs, c0, cN) per channel from the plan table: c0 = x0 + b * block, the
//                               sweep starts behind the saved column (that of the last push's last block for b = 0).  Columns
//                               before x0 come from the channel's kept feature row, the rest from the push.  A channel with
//                               fewer than b + 1 blocks leaves (wave-uniform);
//   k_onepass_gram_live_close   k_onepass_gram_close per (channel, kept state); the workgroups of the FIRST kept state also append
//                               the block's frames to the kept feature row, which no sweep of this push reads at those columns;
//   k_onepass_gram_live_trace   opg_trace_row's walk with N = x0 + n into the compact row the host assigned, the first words_cap
//                               words or (tail) the last.
//   k_onepass_gram_live_commit  (sr_onepass_gram_live_commit, a call of its own behind a push) the words of the listed channels
//                               that no later frame can change, from A, E, N and the grammar's static lists: see the kernel.
// A WEIGHTED grammar takes k_onepass_gram_live_words_w, k_onepass_gram_live_trace_w and k_onepass_gram_live_commit_w; a grammar
// without a nonzero cost launches the unweighted kernels only.  No init launch: a position of A that no push has reached holds
// all ones, E(0, 0) = 0 and E(0, s) is unreachable for s != 0 from the open call (or the adoption of a grammar) on, and the end call puts that back
// (k_onepass_gram_live_wipe).  Where no state is kept no item is kept either (a kept item's charge list is kept): nothing sweeps,
// nothing closes, nothing parses, and the feature row is neither written nor read.  No workgroup waits on another: the blocks are
// ordered by the stream alone.  Plain vector stores; the atomic minimum on A is the only atomic, and it does not depend on the
// order of the waves, so two runs give the same bytes.  The sweep, the close and the charge of a column are sr_sweep_dev.h's;
// the two sweeps are one body (opgl_words), compiled with and without costs.
#include "sr_dtw_plan.h"
#include "sr_spot_dev.h"
#include "sr_sweep_dev.h"

namespace sr {

// block b of a channel: frames [c0, cN); false: the channel has no such block (a silent channel has none at all)
__device__ __forceinline__ bool opgl_block(const OnePassGramLiveArgs &a, const SpotLiveChan &ch, uint32_t b, uint32_t *c0, uint32_t *cN)
{
    const uint32_t end = ch.x0 + ch.n;  // <= utt_frames <= 16 383, and b * block < 16 384: no wrap
    *c0 = ch.x0 + b * a.o.block;
    *cN = end - *c0 < a.o.block ? end : *c0 + a.o.block;
    return *c0 < end;
}
__device__ __forceinline__ unsigned long long *opgl_A(const OnePassGramLiveArgs &a, uint32_t c, uint32_t state)
{
    return a.o.A + ((size_t)c * a.n_states + state) * a.o.P;
}
__device__ __forceinline__ uint32_t *opgl_E(const OnePassGramLiveArgs &a, uint32_t c, uint32_t state)
{
    return a.o.E + ((size_t)c * a.n_states + state) * a.o.P;
}
__device__ __forceinline__ uint32_t opgl_state(const OnePassGramLiveArgs &a, uint32_t i) { return a.keep_states ? a.keep_states[i] : i; }

// block b of every (kept item, channel).  wt: null, or the costs of a weighted grammar (include/sr_engine.h, "weighted
// grammars"): the charge of a column is then taken over the item's charge list with the arc costs added
__device__ __forceinline__ void opgl_words(const OnePassGramLiveArgs &a, const GramCosts *wt, const uint32_t b)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 ogl_smem[];  // template rows [tpl_len][2], then the waves' boundary columns
    const GramItem it = a.items[a.keep_items ? a.keep_items[blockIdx.x] : blockIdx.x];
    const uint32_t k = it.slot, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.y * kSpotWaves + w;
    uint32_t M = a.o.tpl_valid[k] ? a.o.tpl_frames[k] : 0u;
    M = M < a.o.tpl_len ? M : a.o.tpl_len;
    ulonglong2 *s_col = (ulonglong2 *)(ogl_smem + (size_t)a.o.tpl_len * 2) + (size_t)w * a.o.tpl_len;  // (Dd, min(Dd, Dn)) per row
    sweep_stage_tpl(ogl_smem, a.o.tpl + (size_t)k * a.o.tpl_stride, M);
    __syncthreads();
    if (c >= a.o.C || !M) return;  // (a grammar keeps items of valid slots only)
    const SpotLiveChan ch = a.o.chan[c];
    uint32_t c0, cN;
    if (!opgl_block(a, ch, b, &c0, &cN)) return;  // (wave-uniform)
    // the sweep starts behind the saved column: that of this push's last block, or of the last push's (none at frame 0)
    const uint32_t xs = c0 ? (b ? c0 - a.o.block : ch.aux) + 1u : 0u;
    const uint32_t P = a.o.P;

    ulonglong2 *g_col = a.o.cols + ((size_t)c * a.n_keep_items + blockIdx.x) * a.o.tpl_len;
    const uint32_t *E = opgl_E(a, c, 0);  // state s at E + s * P
    const unsigned long long mask = a.masks[it.set];
    const uint32_t *cost = gram_costs_of(wt, it.set);  // by ascending state, as the mask is walked
    unsigned long long *A = opgl_A(a, c, it.target);
    if (xs) {  // resume: the saved column, that of xs - 1 (16-byte loads, coalesced over template rows)
        for (uint32_t r = lane; r < M; r += 64) s_col[r] = g_col[r];
        wave_sync();
    }
    const int16_t *kept = a.o.feat + (size_t)c * (P - 1u) * kCoef;  // the columns before the push
    const int16_t *in = a.o.mfcc + (uint64_t)c * a.o.row_stride;     // the columns [x0, x0 + n)
    for (uint32_t s0 = xs; s0 < cN; s0 += 64) {  // (wave-uniform)
        const uint32_t col = s0 + lane;
        const bool live = col < cN;
        const uint32_t last = (cN - s0 < 64u ? cN - s0 : 64u) - 1;  // the sweep's last live lane: its column is handed on
        const bool keep = col == c0;                                // the exact column the next block resumes from
        Row32 fi = row_from2(u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, 0u);
        if (live) fi = sweep_frame(col < ch.x0 ? kept + (size_t)col * kCoef : in + (size_t)(col - ch.x0) * kCoef);
        // C(col): what a word that starts in this column builds on, the cheapest state of the charge list; final for col <= c0,
        // none yet inside the block (col <= c0 < utt_frames: inside the state's row)
        const uint32_t charge = gram_charge(E, P, col, live && col <= c0, mask, cost);
        SweepLane sw;
        for (uint32_t t = 0; t < M + last; t++)
            sweep_step(ogl_smem, s_col, g_col, keep, fi, charge, col, live, s0 != 0, last, M, lane, t, sw);
        wave_sync();  // the boundary column is complete before the next sweep's lane 0 reads it

        // the key of each end frame of the block: (cost + word_cost, start, slot) -> A(col + 1, target); col + 1 <= cN <= utt_frames
        if (live && col >= c0 && sw.end_v != kSpotInf) atomicMin(&A[col + 1], sweep_end_key(sw.end_v, a.o.word_cost, k));
    }
}

__global__ void __launch_bounds__(64 * kSpotWaves) k_onepass_gram_live_words(const OnePassGramLiveArgs a, const uint32_t b) { opgl_words(a, nullptr, b); }
__global__ void __launch_bounds__(64 * kSpotWaves) k_onepass_gram_live_words_w(const OnePassGramLiveArgs a, const GramCosts wt, const uint32_t b)
{
    opgl_words(a, &wt, b);
}

// k_onepass_gram_close per (channel, kept state) and channel block; grid (channels, kept states).  A state that no key arrived
// in is closed all the same: its filler, or unreachable.  Before it, the workgroups of the first kept state append the block's
// frames to the kept feature row.
__global__ void __launch_bounds__(256) k_onepass_gram_live_close(const OnePassGramLiveArgs a, const uint32_t b)
{
    __shared__ uint64_t s_tot[4];
    const uint32_t c = blockIdx.x;
    const uint32_t state = opgl_state(a, blockIdx.y);
    const SpotLiveChan ch = a.o.chan[c];
    uint32_t c0, cN;
    if (!opgl_block(a, ch, b, &c0, &cN)) return;  // (uniform)
    if (blockIdx.y == 0) {  // 24-byte rows as three 8-byte words each; both sides are 8-byte aligned
        const uint2 *src = (const uint2 *)(a.o.mfcc + (uint64_t)c * a.o.row_stride + (size_t)(c0 - ch.x0) * kCoef);
        uint2 *dst = (uint2 *)(a.o.feat + ((size_t)c * (a.o.P - 1u) + c0) * kCoef);
        for (uint32_t i = threadIdx.x; i < (cN - c0) * 3u; i += 256) dst[i] = src[i];
    }
    const unsigned long long *A = opgl_A(a, c, state);
    uint32_t *E = opgl_E(a, c, state);
    close_window(A, E, c0, cN, a.o.skip_cost, s_tot);
}

// the item (slot, t) by bisection of the items, which ascend by (slot, target): its index, or n_items
__device__ __forceinline__ uint32_t opgl_item_of(const OnePassGramLiveArgs &a, uint32_t slot, uint32_t t)
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

// One step of the walk, all lanes alike, as opg_step takes it: the word that closes E(., t) at or below p.  Returns its end
// position q (0: the rest is filler) with its key, the charge it started from and the smallest state of its charge list that
// carries that charge; wt null: no costs.  *bad is set where A, E and the items disagree, which cannot happen.
__device__ __forceinline__ uint32_t opgl_step(const OnePassGramLiveArgs &a, const GramCosts *wt, uint32_t c, uint32_t p, uint32_t t, uint32_t lane,
                                              uint64_t *key, uint32_t *charge, uint32_t *src, bool *bad)
{
    *key = kSpotInf;
    const uint32_t q = onepass_word_at(opgl_A(a, c, t), opgl_E(a, c, t), p, lane, key);
    if (!q) return 0u;
    const uint32_t slot = (uint32_t)*key & 0xFFFFu, start = (uint32_t)(*key >> 16) & 0xFFFFu;
    const uint32_t at = opgl_item_of(a, slot, t);
    if (at == a.n_items) {
        *bad = true;
        return 0u;
    }
    const uint32_t set = a.items[at].set;
    const uint32_t *ac = wt ? wt->cost + wt->cost_off[set] : nullptr;
    uint32_t cst = kChainNone, s0 = 0;
    for (unsigned long long m = a.masks[set]; m; m &= m - 1) {  // (uniform; ascending states)
        const uint32_t s = (uint32_t)__ffsll((long long)m) - 1u;
        const uint32_t e = opgl_E(a, c, s)[start], v = ac ? e + *ac++ : e;
        if (e != kChainNone && v < cst) cst = v, s0 = s;
    }
    *charge = cst;
    *src = s0;
    return q;
}

// one wave per emitting channel: the end state, then the history of its N = x0 + n frames walked twice, first for the count,
// then for the words in spoken order -- the first words_cap of them, or (tail) the last, where the second walk ends as soon as
// they are written
__device__ __forceinline__ void opgl_trace_chan(const OnePassGramLiveArgs &a, const GramCosts *wt, uint32_t c, uint32_t lane)
{
    const SpotLiveChan ch = a.o.chan[c];
    if (!ch.first_win) return;
    const uint32_t W = a.o.words_cap, N = ch.x0 + ch.n;
    sr_chain_rec *rec = a.o.rec + ch.row_base;
    sr_chain_word *words = a.o.words + (size_t)ch.row_base * W;
    const sr_chain_word none = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    // the cheapest final state, its final cost included, the smallest state among equals (the kept states ascend)
    uint32_t total = kChainNone, fin = 0;
    for (uint32_t i = 0; N && i < a.n_keep_states; i++) {  // (uniform)
        const uint32_t f = opgl_state(a, i);
        if (!a.final_state[f]) continue;
        const uint32_t e = opgl_E(a, c, f)[N];
        if (e == kChainNone) continue;  // an unreachable state takes no cost
        const uint32_t v = wt ? e + wt->final_cost[f] : e;
        if (v < total) total = v, fin = f;
    }
    if (total == kChainNone) {  // (uniform) an empty channel or no parse
        for (uint32_t i = lane; i < W; i += 64) words[i] = none;
        if (lane == 0) *rec = sr_chain_rec{kChainNone, 0u, 0u, SR_CH_NONE};
        return;
    }
    uint32_t n = 0, in_words = 0;
    bool bad = false;
    for (uint32_t p = N, t = fin; p;) {  // (uniform) the count; every start lies below its end position: the walk ends
        uint64_t key;
        uint32_t charge = 0, src = 0;
        const uint32_t q = opgl_step(a, wt, c, p, t, lane, &key, &charge, &src, &bad);
        if (!q) break;
        const uint32_t start = (uint32_t)(key >> 16) & 0xFFFFu;
        n++;
        in_words += q - start;  // frames start .. q - 1
        p = start;
        t = src;
    }
    if (bad) {  // leave a whole record that says so
        for (uint32_t i = lane; i < W; i += 64) words[i] = none;
        if (lane == 0) *rec = sr_chain_rec{kChainNone, 0u, 0u, SR_CH_NONE};
        return;
    }
    const uint32_t shown = n < W ? n : W, first = a.o.tail ? n - shown : 0u;  // the words first .. first + shown - 1 are written
    for (uint32_t i = shown + lane; i < W; i += 64) words[i] = none;
    uint32_t i = n;
    for (uint32_t p = N, t = fin; p && i > first;) {  // (uniform)
        uint64_t key;
        uint32_t charge = 0, src = 0;
        const uint32_t q = opgl_step(a, wt, c, p, t, lane, &key, &charge, &src, &bad);
        if (!q) break;
        const uint32_t slot = (uint32_t)key & 0xFFFFu, start = (uint32_t)(key >> 16) & 0xFFFFu, end = q - 1;
        i--;
        if (lane == 0 && i - first < shown) {
            const uint32_t cum = (uint32_t)(key >> 32), acc = cum - a.o.word_cost - charge;
            words[i - first] =
                sr_chain_word{a.o.word_id[a.o.group_of_slot[slot]], slot, start, end, acc, acc / (end - start + 1 + a.o.tpl_frames[slot]), cum, t};
        }
        p = start;
        t = src;
    }
    if (lane == 0) *rec = sr_chain_rec{total, n, N - in_words, n > W ? SR_CH_TRUNCATED : SR_CH_OK};
}

__global__ void __launch_bounds__(64) k_onepass_gram_live_trace(const OnePassGramLiveArgs a) { opgl_trace_chan(a, nullptr, blockIdx.x, threadIdx.x); }
// under costs: the final cost at the end, the charge and the source state of a word judged on E + the arc cost
__global__ void __launch_bounds__(64) k_onepass_gram_live_trace_w(const OnePassGramLiveArgs a, const GramCosts wt)
{
    opgl_trace_chan(a, &wt, blockIdx.x, threadIdx.x);
}

// grid (channels, states of the dense layout): the keys of every listed channel are all ones again over the positions it had
// reached (0..aux, aux <= utt_frames = P - 1), in EVERY state -- which covers every state a key can have been written in,
// whatever was kept -- and the prefix cost of position 0 is the empty channel's
__global__ void __launch_bounds__(256) k_onepass_gram_live_wipe(const OnePassGramLiveArgs a)
{
    const uint32_t c = blockIdx.x, state = blockIdx.y;
    const SpotLiveChan ch = a.o.chan[c];
    if (!ch.first_win) return;
    unsigned long long *A = opgl_A(a, c, state);
    for (uint32_t p = threadIdx.x; p <= ch.aux; p += 256) A[p] = kSpotInf;
    if (threadIdx.x == 0) opgl_E(a, c, state)[0] = state ? kChainNone : 0u;
}

// sr_onepass_gram_live_end, behind the wipe: the commit cursors of the listed channels say "nothing delivered" again
__global__ void __launch_bounds__(256) k_onepass_gram_live_uncommit(const OnePassGramLiveArgs a, uint2 *cursor)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c < a.o.C && a.o.chan[c].first_win) cursor[c] = uint2{0u, 0u};
}

// ---- sr_onepass_gram_live_commit: the words that can no longer change -------------------------------------------------------
// k_onepass_live_commit's rule (include/sr_engine.h, COMMITTED WORDS of the live one-pass grammar section) with a NODE a pair
// (q, t): t a kept state, q >= 1 and the word A(q, t) closes E(q, t); or the root (0, 0).  end(p, t) = the first node of state t
// at or below p, the root if there is none; the parent of a node whose word starts at x with source state s is end(x, s).
// Parents lie strictly below their children, and A(p, .), E(p, .) depend on frames < p only: the tree never changes where it
// stands.  The entries are the (x, s), s kept, x in the window [lo, N], lo = max(0, N - W), with E(x, s) reachable (none: every
// reachable (x, s) at the last position that has one); the commit node c is the deepest node shared by the walks from end(x, s)
// of all entries.
//
// What the kernel makes of it, one wave per listed channel, every loop with a wave operation in it wave-uniform.  A walk is a
// chain of PAIRS (x, s) with E(x, s) reachable at falling positions: from a pair that is no node to (x - 1, s) -- E came from
// the frame skipped -- and from a node to (the start of its word, its source state).  A grammar has at most 64 states, so the
// pairs of one position that some walk passes are ONE 64-bit mask, and the masks of the positions not yet swept live in an LDS
// ring (a pair's successor lies at most W below it).  The entries are marked, then the positions are swept from the top down
// in blocks of at most min(64, L) positions, lane = position:
//   * a word covers at least L frames, so the successor of a node lies below its block: inside a block only the skipped
//     frames chain, p(x) = marks(x) | (p(x + 1) & ~hits(x + 1)), a prefix scan over the lanes;
//   * the nodes of the block, p & hits, are expanded lane by lane -- the item, its charge list, the source state, as opgl_step
//     finds them -- and mark their successors; what is pending at the block's last position and is no node goes one down;
//   * T counts the marked pairs.  Walks that meet share a mark, so T falls; with one pair left that is a node, that node is c:
//     every walk runs through it, and none did through any node above (T was larger there).  Position 0 is the root.
// The work is the number of distinct pairs above c, not the sum of the walks' lengths.  Before the sweep one case is settled
// at once: a state that is reachable in the window below its first hit there and has no node below the window either -- with
// skipping on, a start state no word leads back into -- contributes the root, and the root is shared with everything.
// Then two walks from c down to the cursor's node, as the trace walks: the count, then the earliest words_cap pending words.
// The cursor's node is c of an earlier call, and c never leaves the chain it once stood on: the walk from c meets it at its
// position.
struct OpglNode {
    uint32_t q, t;       // (0, 0): the root
    uint32_t charge, src;  // of the node's word: what it started from, and in which state
    uint64_t key;
};

// end(p, t)
__device__ __forceinline__ OpglNode opgl_end(const OnePassGramLiveArgs &a, const GramCosts *wt, uint32_t c, uint32_t p, uint32_t t, uint32_t lane)
{
    OpglNode n{0u, 0u, 0u, 0u, kSpotInf};
    bool bad = false;  // (set where A, E and the items disagree, which cannot happen: the walk ends in the root then)
    n.q = opgl_step(a, wt, c, p, t, lane, &n.key, &n.charge, &n.src, &bad);
    n.t = n.q ? t : 0u;
    return n;
}
__device__ __forceinline__ OpglNode opgl_parent(const OnePassGramLiveArgs &a, const GramCosts *wt, uint32_t c, const OpglNode &n, uint32_t lane)
{
    return opgl_end(a, wt, c, (uint32_t)(n.key >> 16) & 0xFFFFu, n.src, lane);  // the start lies below n.q: the walk ends
}

// the source state of the word `key` into state t, as opgl_step finds it, for ONE lane (no wave operation: the lanes of a
// block expand different nodes); 64: A, E and the items disagree, which cannot happen
__device__ __forceinline__ uint32_t opgl_source(const OnePassGramLiveArgs &a, const GramCosts *wt, uint32_t c, uint32_t t, uint64_t key)
{
    const uint32_t slot = (uint32_t)key & 0xFFFFu, start = (uint32_t)(key >> 16) & 0xFFFFu;
    const uint32_t at = opgl_item_of(a, slot, t);
    if (at == a.n_items) return 64u;
    const uint32_t set = a.items[at].set;
    const uint32_t *ac = wt ? wt->cost + wt->cost_off[set] : nullptr;
    uint32_t cst = kChainNone, s0 = 64u;
    for (unsigned long long m = a.masks[set]; m; m &= m - 1) {  // (ascending states)
        const uint32_t s = (uint32_t)__ffsll((long long)m) - 1u;
        const uint32_t e = opgl_E(a, c, s)[start], v = ac ? e + *ac++ : e;
        if (e != kChainNone && v < cst) cst = v, s0 = s;
    }
    return s0;
}

__device__ __forceinline__ uint64_t opgl_wave_or(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v |= ((uint64_t)__shfl_xor((uint32_t)(v >> 32), d, 64) << 32) | __shfl_xor((uint32_t)v, d, 64);
    return v;
}

__device__ __forceinline__ void opgl_commit_chan(const OnePassGramCommitArgs &a, const GramCosts *wt, uint32_t r, uint32_t lane)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long opgl_ring[];  // [a.ring] the marks of the positions not yet swept
    const OnePassGramLiveArgs &g = a.g;
    const uint32_t cap = g.o.words_cap, rmask = a.ring - 1u;  // (a power of two, at least W + 64)
    const sr_chain_live_row row = a.rows[r];
    const uint32_t c = row.channel, N = row.frames;  // N <= utt_frames = P - 1: no position past the history is read
    sr_chain_word *words = a.cwords + (size_t)r * cap;
    const sr_chain_word none = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    const uint32_t lo = N > a.W ? N - a.W : 0u;
    for (uint32_t i = lane; i < a.ring; i += 64) opgl_ring[i] = 0ull;
    wave_sync();

    // the entries: per kept state the reachable positions of the window, marked (a lane owns its positions: no conflict)
    uint32_t T = 0, top = N;
    bool at_root = false;
    for (uint32_t i = 0; i < a.n_kept && !at_root; i++) {  // (uniform)
        const uint32_t s = a.states[i];
        const unsigned long long *A = opgl_A(g, c, s);
        const uint32_t *E = opgl_E(g, c, s);
        uint32_t first_hit = kChainNone, low_reach = kChainNone;  // of state s in the window
        for (uint32_t x0 = lo; x0 <= N; x0 += 64) {  // (uniform) 64 positions per round, coalesced
            const uint32_t x = x0 + lane;
            const bool in = x <= N;
            const uint32_t e = in ? E[x] : kChainNone;
            const uint64_t ky = in && x ? A[x] : kSpotInf;  // position 0 ends no word
            const bool hit = ky != kSpotInf && (uint32_t)(ky >> 32) == e;
            const unsigned long long hits = __ballot(hit), reach = __ballot(e != kChainNone);
            if (low_reach == kChainNone && reach) low_reach = x0 + (uint32_t)__ffsll((long long)reach) - 1u;
            if (first_hit == kChainNone && hits) first_hit = x0 + (uint32_t)__ffsll((long long)hits) - 1u;
            if (e != kChainNone) opgl_ring[x & rmask] |= 1ull << s;
            T += (uint32_t)__popcll(reach);
        }
        // reachable below its first hit of the window: such a walk ends in end(lo - 1, s).  No node there: the root
        if (low_reach != kChainNone && low_reach != first_hit) {
            uint64_t key = kSpotInf;
            at_root = !lo || !onepass_word_at(A, E, lo - 1u, lane, &key);
        }
    }
    if (!T && !at_root) {  // (uniform) an empty window: the last position below it where a kept state is reachable, and its states
        uint32_t xs = kChainNone;
        for (uint32_t hi = lo; hi && xs == kChainNone; hi = hi > 64u ? hi - 64u : 0u) {  // (uniform) positions hi - 1 - lane
            for (uint32_t i = 0; i < a.n_kept; i++) {
                const uint32_t e = lane < hi ? opgl_E(g, c, a.states[i])[hi - 1u - lane] : kChainNone;
                const unsigned long long reach = __ballot(e != kChainNone);
                if (!reach) continue;
                const uint32_t x = hi - (uint32_t)__ffsll((long long)reach);
                xs = xs == kChainNone || x > xs ? x : xs;
            }
        }
        unsigned long long at = 0ull;
        for (uint32_t i = 0; xs != kChainNone && i < a.n_kept; i++)  // (uniform)
            if (opgl_E(g, c, a.states[i])[xs] != kChainNone) at |= 1ull << a.states[i];
        if (at) {
            if (lane == 0) opgl_ring[xs & rmask] = at;
            T = (uint32_t)__popcll(at);
            top = xs;
        }
    }
    wave_sync();

    // the sweep.  cq, ct: the commit node; the root where the sweep reaches position 0 or nothing is marked
    uint32_t cq = 0, ct = 0;
    for (uint32_t y = at_root || !T ? 0u : top; y;) {  // (uniform) the block y - B + 1 .. y, lane i at x = y - i
        const uint32_t B = y < a.block ? y : a.block, x = y - lane;
        const bool in = lane < B;
        unsigned long long m = 0ull;
        if (in) {
            m = opgl_ring[x & rmask];
            opgl_ring[x & rmask] = 0ull;
        }
        const unsigned long long live = opgl_wave_or(m);  // only these states can be pending in the block
        unsigned long long h = 0ull;
        for (unsigned long long sb = live; sb; sb &= sb - 1) {  // (uniform)
            const uint32_t s = (uint32_t)__ffsll((long long)sb) - 1u;
            const uint64_t ky = in ? opgl_A(g, c, s)[x] : kSpotInf;
            const uint32_t e = in ? opgl_E(g, c, s)[x] : kChainNone;
            if (ky != kSpotInf && (uint32_t)(ky >> 32) == e) h |= 1ull << s;
        }
        // p(lane) = m | (p(lane - 1) & ~h(lane - 1)): what is pending above and is no node there comes one position down
        const unsigned long long h_above = spot_shfl_up(h, 1);  // (by every lane: lane 1 reads lane 0)
        unsigned long long G = m, K = lane ? ~h_above : 0ull;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const unsigned long long Gd = spot_shfl_up(G, d), Kd = spot_shfl_up(K, d);
            if (lane >= d) {
                G |= K & Gd;
                K &= Kd;
            }
        }
        const unsigned long long nodes = in ? G & h : 0ull;
        const unsigned long long down = spot_shfl(G & ~h, B - 1u);  // pending at the block's last position and no node
        const uint32_t n_nodes = wave_sum((uint32_t)__popcll(nodes)), x_below = y - B;
        // (position 0 holds the root alone: whatever comes down to it is the pair (0, 0))
        const unsigned long long down_bits = x_below ? down : (down ? 1ull : 0ull), below = opgl_ring[x_below & rmask];
        T = T - wave_sum((uint32_t)__popcll(m)) + n_nodes + (uint32_t)__popcll(down_bits & ~below);
        if (T == 1u && n_nodes == 1u) {  // (uniform) every walk runs through this node
            const unsigned long long has = __ballot(nodes != 0ull);
            const uint32_t l = (uint32_t)__ffsll((long long)has) - 1u;
            cq = y - l;
            ct = (uint32_t)__ffsll((long long)spot_shfl(nodes, l)) - 1u;
            break;
        }
        wave_sync();
        if (lane == 0 && down_bits) opgl_ring[x_below & rmask] = below | down_bits;
        wave_sync();
        uint32_t added = 0;
        for (unsigned long long nb = nodes; nb; nb &= nb - 1) {  // (per lane) the successors of the block's nodes
            const uint32_t t = (uint32_t)__ffsll((long long)nb) - 1u;
            const uint64_t key = opgl_A(g, c, t)[x];
            const uint32_t start = (uint32_t)(key >> 16) & 0xFFFFu, s0 = opgl_source(g, wt, c, t, key);
            if (s0 == 64u) continue;
            const unsigned long long bit = start ? 1ull << s0 : 1ull;
            added += !(atomicOr(&opgl_ring[start & rmask], bit) & bit);
        }
        T = T - n_nodes + wave_sum(added);
        wave_sync();
        if (!T) break;  // (uniform; cannot happen)
        y = x_below;
    }
    const OpglNode cur = cq ? opgl_end(g, wt, c, cq, ct, lane) : OpglNode{0u, 0u, 0u, 0u, kSpotInf};

    const uint2 cu = a.cursor[c];  // {delivered, the last delivered word's node}: an ancestor of c, or c
    const uint32_t cu_q = cu.y & ((1u << kOpgCommitStateShift) - 1u);
    uint32_t pending = 0;
    for (OpglNode n = cur; n.q > cu_q; n = opgl_parent(g, wt, c, n, lane)) pending++;  // (uniform)
    const uint32_t n_new = pending < cap ? pending : cap;
    for (uint32_t i = n_new + lane; i < cap; i += 64) words[i] = none;
    uint32_t last_node = cu.y, j = pending;  // the words on the walk are pending words j - 1 .. 0, the earliest n_new are written
    for (OpglNode n = cur; n.q > cu_q; n = opgl_parent(g, wt, c, n, lane)) {  // (uniform)
        j--;
        if (j >= n_new) continue;
        if (j == n_new - 1u) last_node = n.q | n.t << kOpgCommitStateShift;
        if (lane == 0) {
            const uint32_t slot = (uint32_t)n.key & 0xFFFFu, start = (uint32_t)(n.key >> 16) & 0xFFFFu, end = n.q - 1;
            const uint32_t cum = (uint32_t)(n.key >> 32), acc = cum - g.o.word_cost - n.charge;
            words[j] =
                sr_chain_word{g.o.word_id[g.o.group_of_slot[slot]], slot, start, end, acc, acc / (end - start + 1 + g.o.tpl_frames[slot]), cum, n.t};
        }
    }
    if (lane == 0) {
        a.crec[r] = sr_commit_rec{cu.x + pending, cu.x, n_new, cur.q};
        a.cursor[c] = uint2{cu.x + n_new, last_node};
    }
}

__global__ void __launch_bounds__(64) k_onepass_gram_live_commit(const OnePassGramCommitArgs a) { opgl_commit_chan(a, nullptr, blockIdx.x, threadIdx.x); }
// under costs: the charge and the source state of a word judged on E + the arc cost
__global__ void __launch_bounds__(64) k_onepass_gram_live_commit_w(const OnePassGramCommitArgs a, const GramCosts wt)
{
    opgl_commit_chan(a, &wt, blockIdx.x, threadIdx.x);
}

static void opgl_launch_trace(const OnePassGramLiveArgs &a, const GramCosts *w, hipStream_t s)
{
    if (w) {
        SR_LAUNCH_POINT(s, "k_onepass_gram_live_trace_w");
        hipLaunchKernelGGL(k_onepass_gram_live_trace_w, dim3(a.o.C), dim3(64), 0, s, a, *w);
    } else {
        SR_LAUNCH_POINT(s, "k_onepass_gram_live_trace");
        hipLaunchKernelGGL(k_onepass_gram_live_trace, dim3(a.o.C), dim3(64), 0, s, a);
    }
}

void launch_onepass_gram_live(const OnePassGramLiveArgs &a, const GramCosts *w, uint32_t n_blocks, hipStream_t s)
{
    if (!a.o.C) return;
    const size_t lds = spot_lds_bytes(a.o.tpl_len);
    const dim3 grid(a.n_keep_items, (a.o.C + kSpotWaves - 1) / kSpotWaves);
    for (uint32_t b = 0; b < n_blocks; b++) {
        if (a.n_keep_items) {
            if (w) {
                SR_LAUNCH_POINT(s, "k_onepass_gram_live_words_w");
                hipLaunchKernelGGL(k_onepass_gram_live_words_w, grid, dim3(64 * kSpotWaves), lds, s, a, *w, b);
            } else {
                SR_LAUNCH_POINT(s, "k_onepass_gram_live_words");
                hipLaunchKernelGGL(k_onepass_gram_live_words, grid, dim3(64 * kSpotWaves), lds, s, a, b);
            }
        }
        if (a.n_keep_states) {
            SR_LAUNCH_POINT(s, "k_onepass_gram_live_close");
            hipLaunchKernelGGL(k_onepass_gram_live_close, dim3(a.o.C, a.n_keep_states), dim3(256), 0, s, a, b);
        }
    }
    opgl_launch_trace(a, w, s);
}
void launch_onepass_gram_live_wipe(const OnePassGramLiveArgs &a, hipStream_t s)
{
    if (!a.o.C || !a.n_states) return;
    SR_LAUNCH_POINT(s, "k_onepass_gram_live_wipe");
    hipLaunchKernelGGL(k_onepass_gram_live_wipe, dim3(a.o.C, a.n_states), dim3(256), 0, s, a);
}
void launch_onepass_gram_live_end(const OnePassGramLiveArgs &a, const GramCosts *w, uint2 *cursor, hipStream_t s)
{
    if (!a.o.C) return;
    opgl_launch_trace(a, w, s);
    launch_onepass_gram_live_wipe(a, s);
    SR_LAUNCH_POINT(s, "k_onepass_gram_live_uncommit");
    hipLaunchKernelGGL(k_onepass_gram_live_uncommit, dim3((a.o.C + 255u) / 256u), dim3(256), 0, s, a, cursor);
}
void launch_onepass_gram_live_commit(const OnePassGramCommitArgs &a, const GramCosts *w, hipStream_t s)
{
    if (!a.n_rows) return;
    const size_t lds = (size_t)a.ring * 8;  // the ring of marks: 32 KiB under the longest template that fits the sweep's LDS image
    if (w) {
        SR_LAUNCH_POINT(s, "k_onepass_gram_live_commit_w");
        hipLaunchKernelGGL(k_onepass_gram_live_commit_w, dim3(a.n_rows), dim3(64), lds, s, a, *w);
    } else {
        SR_LAUNCH_POINT(s, "k_onepass_gram_live_commit");
        hipLaunchKernelGGL(k_onepass_gram_live_commit, dim3(a.n_rows), dim3(64), lds, s, a);
    }
}
const char *onepass_gram_live_allow_lds(uint32_t bytes)
{
    return allow_dynamic_lds({{(const void *)k_onepass_gram_live_words, "k_onepass_gram_live_words"},
                              {(const void *)k_onepass_gram_live_words_w, "k_onepass_gram_live_words_w"},
                              // (the commit's ring stays below 64 KiB under any store the sweeps accept)
                              {(const void *)k_onepass_gram_live_commit, "k_onepass_gram_live_commit"},
                              {(const void *)k_onepass_gram_live_commit_w, "k_onepass_gram_live_commit_w"}},
                             bytes);
}

}  // namespace sr
