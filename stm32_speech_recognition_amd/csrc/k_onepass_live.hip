// k_onepass_live.hip -- live one-pass connected-word decoding (include/sr_engine.h, "live one-pass connected-word decoding"):
// k_onepass.hip's blocks with the boundaries set by the caller's pushes, per channel and of unequal length.  OPT-IN EXTENSION,
// no reference counterpart.  gfx950 (MI355X, CDNA4) only; wave = 64 lanes; integer VALU + LDS.
//
// The batch kernel's argument carries over: a word that starts inside a block of at most L = min_k(M_k / 2 + 1) frames cannot
// end inside it, so A and E over a block follow from E at or before its first frame -- whatever the lengths of the blocks
// before it.  A channel keeps A and E over its whole recording, per slot the EXACT column at the first frame c0 of the block
// swept last, and its feature row.  A push that appends the frames [x0, x0 + n) is, per block b = 0.. of `block` <= L frames,
// in stream order:
//   k_onepass_live_words   k_onepass_words with (xs, c0, cN) per channel from the plan table: c0 = x0 + b * block, the sweep
//                          starts behind the saved column (that of the last push's last block for b = 0).  Columns before x0
//                          come from the channel's kept feature row, the rest from the push.  A channel with fewer than b + 1
//                          blocks leaves (wave-uniform);
//   k_onepass_live_close   k_onepass_close per channel; it also appends the block's frames to the kept feature row, which no
//                          sweep of this push reads at those columns;
//   k_onepass_live_trace   k_onepass_trace with N = x0 + n into the compact row the host assigned, the first words_cap words
//                          or (tail) the last.
//   k_onepass_live_commit  (sr_onepass_live_commit, a call of its own behind a push) the words of the listed channels that no
//                          later frame can change, from A, E and N alone: see the kernel.
// No init launch: a position of A that no push has reached holds all ones from the open call on, and the end call puts that
// back (k_onepass_live_wipe); E(0) = 0 never changes.  No workgroup waits on another: the blocks are ordered by the stream
// alone.  Plain vector stores; the atomic minimum on A is the only atomic, and it does not depend on the order of the waves, so
// two runs give the same bytes.
#include "sr_dtw_plan.h"
#include "sr_spot_dev.h"
#include "sr_sweep_dev.h"

namespace sr {

// block b of a channel: frames [c0, cN); false: the channel has no such block (a silent channel has none at all)
__device__ __forceinline__ bool onepass_live_block(const OnePassLiveArgs &a, const SpotLiveChan &ch, uint32_t b, uint32_t *c0, uint32_t *cN)
{
    const uint32_t end = ch.x0 + ch.n;  // <= utt_frames <= 16 383, and b * block < 16 384: no wrap
    *c0 = ch.x0 + b * a.block;
    *cN = end - *c0 < a.block ? end : *c0 + a.block;
    return *c0 < end;
}

__global__ void __launch_bounds__(64 * kSpotWaves) k_onepass_live_words(const OnePassLiveArgs a, const uint32_t b)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 ol_smem[];  // template rows [tpl_len][2], then the waves' boundary columns
    const uint32_t k = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.y * kSpotWaves + w;
    uint32_t M = a.tpl_valid[k] ? a.tpl_frames[k] : 0u;
    M = M < a.tpl_len ? M : a.tpl_len;
    ulonglong2 *s_col = (ulonglong2 *)(ol_smem + (size_t)a.tpl_len * 2) + (size_t)w * a.tpl_len;  // (Dd, min(Dd, Dn)) per row
    sweep_stage_tpl(ol_smem, a.tpl + (size_t)k * a.tpl_stride, M);
    __syncthreads();
    if (c >= a.C || !M) return;  // (an invalid slot ends no word and keeps no column)
    const SpotLiveChan ch = a.chan[c];
    uint32_t c0, cN;
    if (!onepass_live_block(a, ch, b, &c0, &cN)) return;  // (wave-uniform)
    // the sweep starts behind the saved column: that of this push's last block, or of the last push's (none at frame 0)
    const uint32_t xs = c0 ? (b ? c0 - a.block : ch.aux) + 1u : 0u;

    ulonglong2 *g_col = a.cols + ((size_t)c * a.K + k) * a.tpl_len;
    const uint32_t *E = a.E + (size_t)c * a.P;
    unsigned long long *A = a.A + (size_t)c * a.P;
    if (xs) {  // resume: the saved column, that of xs - 1 (16-byte loads, coalesced over template rows)
        for (uint32_t r = lane; r < M; r += 64) s_col[r] = g_col[r];
        wave_sync();
    }
    const int16_t *kept = a.feat + (size_t)c * (a.P - 1u) * kCoef;  // the columns before the push
    const int16_t *in = a.mfcc + (uint64_t)c * a.row_stride;         // the columns [x0, x0 + n)
    for (uint32_t s0 = xs; s0 < cN; s0 += 64) {  // (wave-uniform)
        const uint32_t col = s0 + lane;
        const bool live = col < cN;
        const uint32_t last = (cN - s0 < 64u ? cN - s0 : 64u) - 1;  // the sweep's last live lane: its column is handed on
        const bool keep = col == c0;                                // the exact column the next block resumes from
        Row32 fi = row_from2(u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, 0u);
        uint32_t charge = kChainNone;  // E(col): what a word that starts in this column builds on; none yet inside the block
        if (live) {
            fi = sweep_frame(col < ch.x0 ? kept + (size_t)col * kCoef : in + (size_t)(col - ch.x0) * kCoef);
            if (col <= c0) charge = E[col];
        }
        SweepLane sw;
        for (uint32_t t = 0; t < M + last; t++)
            sweep_step(ol_smem, s_col, g_col, keep, fi, charge, col, live, s0 != 0, last, M, lane, t, sw);
        wave_sync();  // the boundary column is complete before the next sweep's lane 0 reads it

        // the key of each end frame of the block: (cost + word_cost, start, slot) -> A(col + 1); col + 1 <= cN <= utt_frames
        if (live && col >= c0 && sw.end_v != kSpotInf) atomicMin(&A[col + 1], sweep_end_key(sw.end_v, a.word_cost, k));
    }
}

// E(p), p in (c0, cN], as k_onepass_close gives it, per channel; before it, the block's frames go to the kept feature row.
// One workgroup per channel: wave scans plus an LDS carry.
__global__ void __launch_bounds__(256) k_onepass_live_close(const OnePassLiveArgs a, const uint32_t b)
{
    __shared__ uint64_t s_tot[4];
    const uint32_t c = blockIdx.x;
    const SpotLiveChan ch = a.chan[c];
    uint32_t c0, cN;
    if (!onepass_live_block(a, ch, b, &c0, &cN)) return;  // (uniform)
    {  // 24-byte rows as three 8-byte words each; both sides are 8-byte aligned
        const uint2 *src = (const uint2 *)(a.mfcc + (uint64_t)c * a.row_stride + (size_t)(c0 - ch.x0) * kCoef);
        uint2 *dst = (uint2 *)(a.feat + ((size_t)c * (a.P - 1u) + c0) * kCoef);
        for (uint32_t i = threadIdx.x; i < (cN - c0) * 3u; i += 256) dst[i] = src[i];
    }
    const unsigned long long *A = a.A + (size_t)c * a.P;
    uint32_t *E = a.E + (size_t)c * a.P;
    close_window(A, E, c0, cN, a.skip_cost, s_tot);
}

// one wave per emitting channel: the history of its N = x0 + n frames is walked twice (onepass_word_at, sr_spot_dev.h), first
// for the count, then for the words in spoken order -- the first words_cap of them, or (tail) the last, where the second walk
// ends as soon as they are written
__global__ void __launch_bounds__(64) k_onepass_live_trace(const OnePassLiveArgs a)
{
    const uint32_t c = blockIdx.x, lane = threadIdx.x, W = a.words_cap;
    const SpotLiveChan ch = a.chan[c];
    if (!ch.first_win) return;
    const uint32_t N = ch.x0 + ch.n;
    const unsigned long long *A = a.A + (size_t)c * a.P;
    const uint32_t *E = a.E + (size_t)c * a.P;
    sr_chain_rec *rec = a.rec + ch.row_base;
    sr_chain_word *words = a.words + (size_t)ch.row_base * W;
    const sr_chain_word none = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    const uint32_t total = N ? E[N] : kChainNone;
    if (total == kChainNone) {  // (uniform) an empty channel or no parse
        for (uint32_t i = lane; i < W; i += 64) words[i] = none;
        if (lane == 0) *rec = sr_chain_rec{kChainNone, 0u, 0u, SR_CH_NONE};
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
    const uint32_t shown = n < W ? n : W, first = a.tail ? n - shown : 0u;  // the words first .. first + shown - 1 are written
    for (uint32_t i = shown + lane; i < W; i += 64) words[i] = none;
    uint32_t i = n;
    for (uint32_t p = N; p && i > first;) {  // (uniform)
        uint64_t key = kSpotInf;
        const uint32_t q = onepass_word_at(A, E, p, lane, &key);
        if (!q) break;
        const uint32_t slot = (uint32_t)key & 0xFFFFu, start = (uint32_t)(key >> 16) & 0xFFFFu, end = q - 1;
        i--;
        if (lane == 0 && i - first < shown) {
            const uint32_t acc = (uint32_t)(key >> 32) - a.word_cost - E[start];
            words[i - first] =
                sr_chain_word{a.word_id[a.group_of_slot[slot]], slot, start, end, acc, acc / (end - start + 1 + a.tpl_frames[slot]), E[q], 0u};
        }
        p = start;
    }
    if (lane == 0) *rec = sr_chain_rec{total, n, N - in_words, n > W ? SR_CH_TRUNCATED : SR_CH_OK};
}

// sr_onepass_live_end, behind the trace: the keys of every listed channel are all ones again over the positions it had reached,
// and its commit cursor says "nothing delivered"
__global__ void __launch_bounds__(256) k_onepass_live_wipe(const OnePassLiveArgs a, uint2 *cursor)
{
    const uint32_t c = blockIdx.x;
    const SpotLiveChan ch = a.chan[c];
    if (!ch.first_win) return;
    unsigned long long *A = a.A + (size_t)c * a.P;
    for (uint32_t p = 1 + threadIdx.x; p <= ch.aux; p += 256) A[p] = kSpotInf;  // aux <= utt_frames = P - 1
    if (threadIdx.x == 0) cursor[c] = uint2{0u, 0u};
}

// ---- sr_onepass_live_commit: the words that can no longer change ------------------------------------------------------------
// A NODE is a position q >= 1 whose own word closes E there (onepass_word_at's hit), or 0; end(p) = the first node at or below
// p; the parent of a node is end(the start of its word).  Parents lie strictly below their children, and A(p), E(p) depend on
// frames < p only, so the tree never changes where it stands.  The rule (include/sr_engine.h): every hypothesis alive in the last
// column started inside the window [lo, N], lo = max(0, N - W); the entries are the positions of the window where E is
// reachable (none: the last reachable position below it); the commit node c is the deepest node shared by the walks from
// end(x) of all entries x.
//
// What the kernel makes of it, one wave per listed channel, every loop wave-uniform (N, W, ballots and shuffled keys only):
//   * a hit is reachable, so the entry nodes are the hits of the window and -- unless the lowest reachable position of the
//     window is itself a hit -- end(lo - 1), the node below the window.  With nothing reachable in the window that node is c.
//   * a hit whose word starts at or above the window's first hit has its parent inside the window: the parent is an entry node
//     too, and the child adds nothing to what all walks share.  The others are the ROOTS, where a walk leaves the window.
//   * c = the common node of the roots and the node below, folded pair by pair: while two nodes differ, the one at the higher
//     position goes to its parent.  That cannot step over the common node: the common node is a proper ancestor of any node
//     above it on either walk, and a parent lies below its child.
// Then two walks from c down to the cursor's node, as the trace walks: the count, then the earliest words_cap pending words.

// the parent of the node whose key is *key; *key becomes the parent's (unchanged garbage for node 0, which has no word)
__device__ __forceinline__ uint32_t commit_parent(const unsigned long long *A, const uint32_t *E, uint32_t lane, uint64_t *key)
{
    const uint32_t start = (uint32_t)(*key >> 16) & 0xFFFFu;  // < the node's position: the walk ends
    return onepass_word_at(A, E, start, lane, key);
}

// (*cur, *cur_key) becomes the common node of itself and (q, key); kChainNone: no node yet
__device__ __forceinline__ void commit_join(const unsigned long long *A, const uint32_t *E, uint32_t lane, uint32_t *cur, uint64_t *cur_key,
                                            uint32_t q, uint64_t key)
{
    if (*cur == kChainNone) {
        *cur = q;
        *cur_key = key;
        return;
    }
    while (*cur != q) {  // (uniform)
        if (*cur > q)
            *cur = commit_parent(A, E, lane, cur_key);
        else
            q = commit_parent(A, E, lane, &key);
    }
}

__global__ void __launch_bounds__(64) k_onepass_live_commit(const OnePassCommitArgs a)
{
    const uint32_t lane = threadIdx.x, cap = a.words_cap;
    const sr_chain_live_row row = a.rows[blockIdx.x];
    const uint32_t c = row.channel, N = row.frames;  // N <= utt_frames = P - 1: no position past the history is read
    const unsigned long long *A = a.A + (size_t)c * a.P;
    const uint32_t *E = a.E + (size_t)c * a.P;
    sr_chain_word *words = a.cwords + (size_t)blockIdx.x * cap;
    const sr_chain_word none = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    const uint32_t lo = N > a.W ? N - a.W : 0u;

    uint32_t first_hit = kChainNone, low_reach = kChainNone;  // of the window
    uint32_t cur = kChainNone;                                // the common node so far
    uint64_t cur_key = kSpotInf;
    for (uint32_t x0 = lo; x0 <= N; x0 += 64) {  // (uniform) the window, 64 positions per round, coalesced
        const uint32_t x = x0 + lane;
        const bool in = x <= N;
        const uint32_t e = in ? E[x] : kChainNone;
        const uint64_t ky = in && x ? A[x] : kSpotInf;  // position 0 ends no word
        const bool hit = ky != kSpotInf && (uint32_t)(ky >> 32) == e;
        const unsigned long long hits = __ballot(hit), reach = __ballot(e != kChainNone);
        if (low_reach == kChainNone && reach) low_reach = x0 + (uint32_t)__ffsll((long long)reach) - 1u;
        if (first_hit == kChainNone && hits) first_hit = x0 + (uint32_t)__ffsll((long long)hits) - 1u;
        unsigned long long roots = __ballot(hit && ((uint32_t)(ky >> 16) & 0xFFFFu) < first_hit);
        while (roots) {  // (uniform)
            const uint32_t b = (uint32_t)__ffsll((long long)roots) - 1u;
            roots &= roots - 1;
            commit_join(A, E, lane, &cur, &cur_key, x0 + b, spot_shfl(ky, b));
        }
    }
    if (first_hit == kChainNone || low_reach != first_hit) {  // (uniform) the node below the window is an entry node, or c itself
        uint64_t key = kSpotInf;
        const uint32_t below = lo ? onepass_word_at(A, E, lo - 1u, lane, &key) : 0u;
        commit_join(A, E, lane, &cur, &cur_key, below, key);
    }

    const uint2 cu = a.cursor[c];  // {delivered, the last delivered word's node}: an ancestor of c, or c
    uint32_t pending = 0;
    {
        uint64_t key = cur_key;
        for (uint32_t q = cur; q > cu.y; q = commit_parent(A, E, lane, &key)) pending++;  // (uniform)
    }
    const uint32_t n_new = pending < cap ? pending : cap;
    for (uint32_t i = n_new + lane; i < cap; i += 64) words[i] = none;
    uint32_t last_node = cu.y, j = pending;  // the words on the walk are pending words j - 1 .. 0, the earliest n_new are written
    uint64_t key = cur_key;
    for (uint32_t q = cur; q > cu.y; q = commit_parent(A, E, lane, &key)) {  // (uniform)
        j--;
        if (j >= n_new) continue;
        if (j == n_new - 1u) last_node = q;
        if (lane == 0) {
            const uint32_t slot = (uint32_t)key & 0xFFFFu, start = (uint32_t)(key >> 16) & 0xFFFFu, end = q - 1;
            const uint32_t acc = (uint32_t)(key >> 32) - a.word_cost - E[start];
            words[j] = sr_chain_word{a.word_id[a.group_of_slot[slot]], slot, start, end, acc, acc / (end - start + 1 + a.tpl_frames[slot]), E[q], 0u};
        }
    }
    if (lane == 0) {
        a.crec[blockIdx.x] = sr_commit_rec{cu.x + pending, cu.x, n_new, cur};
        a.cursor[c] = uint2{cu.x + n_new, last_node};
    }
}

void launch_onepass_live(const OnePassLiveArgs &a, uint32_t n_blocks, hipStream_t s)
{
    if (!a.C || !a.K) return;
    const size_t lds = spot_lds_bytes(a.tpl_len);
    const dim3 grid(a.K, (a.C + kSpotWaves - 1) / kSpotWaves);
    for (uint32_t b = 0; b < n_blocks; b++) {
        SR_LAUNCH_POINT(s, "k_onepass_live_words");
        hipLaunchKernelGGL(k_onepass_live_words, grid, dim3(64 * kSpotWaves), lds, s, a, b);
        SR_LAUNCH_POINT(s, "k_onepass_live_close");
        hipLaunchKernelGGL(k_onepass_live_close, dim3(a.C), dim3(256), 0, s, a, b);
    }
    SR_LAUNCH_POINT(s, "k_onepass_live_trace");
    hipLaunchKernelGGL(k_onepass_live_trace, dim3(a.C), dim3(64), 0, s, a);
}
void launch_onepass_live_end(const OnePassLiveArgs &a, uint2 *cursor, hipStream_t s)
{
    if (!a.C) return;
    SR_LAUNCH_POINT(s, "k_onepass_live_trace");
    hipLaunchKernelGGL(k_onepass_live_trace, dim3(a.C), dim3(64), 0, s, a);
    SR_LAUNCH_POINT(s, "k_onepass_live_wipe");
    hipLaunchKernelGGL(k_onepass_live_wipe, dim3(a.C), dim3(256), 0, s, a, cursor);
}
void launch_onepass_live_commit(const OnePassCommitArgs &a, hipStream_t s)
{
    if (!a.n_rows) return;
    SR_LAUNCH_POINT(s, "k_onepass_live_commit");
    hipLaunchKernelGGL(k_onepass_live_commit, dim3(a.n_rows), dim3(64), 0, s, a);
}
const char *onepass_live_allow_lds(uint32_t bytes)
{
    return allow_dynamic_lds({{(const void *)k_onepass_live_words, "k_onepass_live_words"}}, bytes);
}

}  // namespace sr
