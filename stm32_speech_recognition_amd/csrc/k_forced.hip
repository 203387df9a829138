// k_forced.hip -- transcript-forced alignment and the span gather (include/sr_engine.h, "forced alignment against a
// transcript").  OPT-IN EXTENSION, no reference counterpart; the local distance is the reference's get_dis (DTW.C:45-62).
// gfx950 (MI355X, CDNA4) only; wave = 64 lanes; no MFMA (the path has no dense contraction), integer VALU + LDS.
//
// The scratch is k_chain.hip's, A[row][level][max_frames + 1] and E[row][level 0..][max_frames + 1] with max_words =
// words_per_row, and so are k_chain_init and k_chain_close (launch_chain_init / launch_chain_close).  Two kernels are new.
//
// k_forced_words is k_chain_words' sweep -- the skewed anti-diagonal wavefront, the template staged in LDS, packed (cost,
// start) states, a 64-bit atomic minimum per end frame -- with a grid over the host's ITEM list of the level (sr_forced_plan.h:
// (row, slot) for every row whose transcript has the level and every valid slot of its word there) and with the exact column
// bound of a linear transcript: level l of a row needs the end frames e with e + 1 <= N - tail only, tail = the fewest frames
// the words after position l can take.  N is a device value, so the wave forms the bound itself; a wave whose chunk lies
// beyond it exits, and so does a 64-column sweep that no reachable charge has entered yet (E_{l-1} is unreachable in the early
// columns of a late level).  The sweep of 64 columns itself is sr_sweep_dev.h's, as in k_chain.hip and k_gram.hip.
//
// k_forced_trace is chain_trace_row's walk (sr_spot_dev.h) with the word count taken per row and the word's 1-based position in
// `reserved`: what k_gram_trace writes under the sequence grammar of the row's transcript.
//
// k_gather_spans copies the frames of a word span into an example row of the trainers' layout, one workgroup per example.
#include "sr_dtw_plan.h"
#include "sr_spot_dev.h"
#include "sr_sweep_dev.h"

namespace sr {

__device__ __forceinline__ unsigned long long *forced_A(const ChainArgs &a, uint32_t row, uint32_t level)  // level 1..max_words
{
    return a.A + ((size_t)row * a.max_words + (level - 1)) * (a.max_frames + 1u);
}
__device__ __forceinline__ uint32_t *forced_E(const ChainArgs &a, uint32_t row, uint32_t level)  // level 0..max_words
{
    return a.E + ((size_t)row * (a.max_words + 1u) + level) * (a.max_frames + 1u);
}
__device__ __forceinline__ uint32_t forced_frames(const ChainArgs &a, uint32_t row)
{
    const uint32_t N = a.in_frames[(size_t)row * a.frames_stride];
    return N < a.max_frames ? N : a.max_frames;
}

__global__ void __launch_bounds__(64 * kSpotWaves) k_forced_words(const ForcedArgs a, const uint32_t level, const uint32_t item0)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 fc_smem[];  // template rows [tpl_len][2], then the waves' boundary columns
    const uint2 it = a.items[item0 + blockIdx.x];
    const uint32_t row = it.x - a.row0, k = it.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t chunk = blockIdx.y * kSpotWaves + w;
    uint32_t M = a.c.tpl_valid[k] ? a.c.tpl_frames[k] : 0u;
    M = M < a.c.tpl_len ? M : a.c.tpl_len;
    ulonglong2 *s_col = (ulonglong2 *)(fc_smem + (size_t)a.c.tpl_len * 2) + (size_t)w * a.c.tpl_len;  // (Dd, min(Dd, Dn)) per row
    sweep_stage_tpl(fc_smem, a.c.tpl + (size_t)k * a.c.tpl_stride, M);
    __syncthreads();
    if (chunk >= a.c.n_chunks || !M) return;

    // the end frames this level needs: [0, N - tail), the words still to come take the rest
    const uint32_t N = forced_frames(a.c, row), tail = a.tail[(size_t)row * a.c.max_words + (level - 1)];
    const uint32_t Nb = N > tail ? N - tail : 0u;
    const uint32_t c0 = chunk * a.c.chunk_cols;              // the chunk's end frames [c0, cN)
    const uint32_t c1 = c0 + a.c.chunk_cols, cN = c1 < Nb ? c1 : Nb;
    if (c0 >= cN) return;
    const int16_t *in = a.c.mfcc + (size_t)row * a.c.max_frames * kCoef;
    const uint32_t *e_prev = forced_E(a.c, row, level - 1);
    unsigned long long *A = forced_A(a.c, row, level);
    const uint32_t cs = c0 > 2 * M - 2 ? c0 - (2 * M - 2) : 0u;  // the exact lead-in
    bool fresh = true;  // no sweep so far had a reachable charge: every state left of x0 is unreachable, as left of cs
    for (uint32_t x0 = cs; x0 < cN; x0 += 64) {  // (wave-uniform)
        const uint32_t col = x0 + lane;
        const bool live = col < cN;
        const uint32_t charge = live ? e_prev[col] : kChainNone;  // E_{l-1}(col): what a word that starts in this column builds on
        if (fresh && !__ballot(charge != kChainNone)) continue;   // (uniform) nothing starts here and nothing arrives: all unreachable
        Row32 fi = row_from2(u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, 0u);
        if (live) fi = sweep_frame(in + (size_t)col * kCoef);
        const uint32_t end_lane = (cN - x0 < 64u ? cN - x0 : 64u) - 1;  // the sweep's last live lane
        SweepLane sw;
        for (uint32_t t = 0; t < M + end_lane; t++)
            sweep_step(fc_smem, s_col, nullptr, false, fi, charge, col, live, !fresh, 63, M, lane, t, sw);
        wave_sync();  // the boundary column is complete before the next sweep's lane 0 reads it
        fresh = false;

        // the key of each end frame of the chunk: (cost + word_cost, start, slot) -> A_l(col + 1); col + 1 <= N - tail <= max_frames
        if (live && col >= c0 && sw.end_v != kSpotInf) atomicMin(&A[col + 1], sweep_end_key(sw.end_v, a.c.word_cost, k));
    }
}

// The records of a row: its count is the transcript's, level n's cost at N decides, then chain_trace_row's walk.  One wave per row.
__global__ void __launch_bounds__(64) k_forced_trace(const ForcedArgs a)
{
    const uint32_t row = blockIdx.x, W = a.c.max_words, P = a.c.max_frames + 1u, lane = threadIdx.x;
    const uint32_t N = forced_frames(a.c, row);
    const uint32_t n = a.count[row] < W ? a.count[row] : W;
    const unsigned long long *A1 = forced_A(a.c, row, 1);
    const uint32_t *E0 = forced_E(a.c, row, 0);
    sr_chain_rec *rec = a.c.rec + row;
    sr_chain_word *words = a.c.words + (size_t)row * W;
    const uint32_t total = (n && N) ? E0[(size_t)n * P + N] : kChainNone;
    const bool ok = total != kChainNone;
    const sr_chain_word none = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    for (uint32_t i = (ok ? n : 0u) + lane; i < W; i += 64) words[i] = none;
    if (!ok) {
        if (lane == 0) *rec = sr_chain_rec{kChainNone, 0u, 0u, SR_CH_NONE};
        return;
    }
    uint32_t p = N, in_words = 0;
    for (uint32_t l = n; l >= 1; l--) {  // (uniform)
        const unsigned long long *A = A1 + (size_t)(l - 1) * P;
        const uint32_t *E = E0 + (size_t)l * P;
        // the first position at or below p whose own word closes E_l there; E_l(p) is finite, so there is one above 0.  p is N or
        // the start of word l + 1, at most N - tail_l: only positions the bounded sweep filled are read
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
        if (key == kSpotInf) {  // cannot happen while A and E agree; leave a whole record that says so
            for (uint32_t i = lane; i < W; i += 64) words[i] = none;
            if (lane == 0) *rec = sr_chain_rec{kChainNone, 0u, 0u, SR_CH_NONE};
            return;
        }
        const uint32_t slot = (uint32_t)key & 0xFFFFu, start = (uint32_t)(key >> 16) & 0xFFFFu, end = p - 1;
        if (lane == 0) {
            const uint32_t acc = (uint32_t)(key >> 32) - a.c.word_cost - (E - P)[start];  // E_{l-1}(start)
            words[l - 1] = sr_chain_word{a.c.word_id[a.c.group_of_slot[slot]], slot, start, end, acc,
                                         acc / (end - start + 1 + a.c.tpl_frames[slot]), cum, l};
        }
        in_words += end - start + 1;
        p = start;
    }
    if (lane == 0) *rec = sr_chain_rec{total, n, N - in_words, SR_CH_OK};
}

// Example e: the frames start..end of its span into rows 0..L-1, zero behind them; an example without a span, an invalid
// span (start > end or end >= N) or one longer than ex_rows gives a zero row of 0 frames.  Rows are 24 bytes = 6 words.
__global__ void __launch_bounds__(256) k_gather_spans(const GatherArgs a)
{
    const uint32_t e = blockIdx.x, src = a.src_of_ex[e];
    uint32_t L = 0;
    const uint32_t *in = nullptr;
    if (src != 0xFFFFFFFFu) {
        const uint32_t row = src / a.words_per_row;
        const uint32_t start = a.words[src].start, end = a.words[src].end;
        const uint32_t Nr = a.in_frames[(size_t)row * a.frames_stride], N = Nr < a.max_frames ? Nr : a.max_frames;
        if (start <= end && end < N && end - start < a.ex_rows) {
            L = end - start + 1;
            in = (const uint32_t *)(a.mfcc + ((size_t)row * a.max_frames + start) * kCoef);
        }
    }
    uint32_t *out = (uint32_t *)(a.ex + (size_t)e * a.ex_rows * kCoef);
    for (uint32_t i = threadIdx.x; i < a.ex_rows * 6u; i += 256) out[i] = i < L * 6u ? in[i] : 0u;
    if (threadIdx.x == 0) a.ex_frames[e] = L;
}

void launch_forced(const ForcedArgs &a, const uint32_t *item0, uint32_t levels, hipStream_t s)
{
    if (!a.c.n_rows) return;
    const size_t lds = spot_lds_bytes(a.c.tpl_len);
    launch_chain_init(a.c, s);
    for (uint32_t l = 1; l <= levels; l++) {
        const uint32_t n_items = item0[l] - item0[l - 1];
        if (n_items) {  // (a level without items stays unreachable: the close below says so in E_l)
            SR_LAUNCH_POINT(s, "k_forced_words");
            hipLaunchKernelGGL(k_forced_words, dim3(n_items, (a.c.n_chunks + kSpotWaves - 1) / kSpotWaves), dim3(64 * kSpotWaves), lds, s, a, l,
                               item0[l - 1]);
        }
        launch_chain_close(a.c, l, s);
    }
    SR_LAUNCH_POINT(s, "k_forced_trace");
    hipLaunchKernelGGL(k_forced_trace, dim3(a.c.n_rows), dim3(64), 0, s, a);
}
void launch_gather_spans(const GatherArgs &a, hipStream_t s)
{
    if (a.n_ex) {
        SR_LAUNCH_POINT(s, "k_gather_spans");
        hipLaunchKernelGGL(k_gather_spans, dim3(a.n_ex), dim3(256), 0, s, a);
    }
}
const char *forced_allow_lds(uint32_t bytes) { return allow_dynamic_lds({{(const void *)k_forced_words, "k_forced_words"}}, bytes); }

}  // namespace sr
