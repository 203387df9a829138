// sr_spot_dev.h -- the packed (cost, start) state of the subsequence DTW kernels (k_spot.hip, k_chain.hip): cost in the high
// word of one u64, so that the tie rule (smallest start among equal costs) is the u64 minimum; unreachable = all ones.
// gfx950 (MI355X, CDNA4) only; wave = 64 lanes.
#pragma once
#include "sr_dtw_dev.h"

namespace sr {

constexpr uint64_t kSpotInf = ~0ull;

__device__ __forceinline__ uint64_t spot_min(uint64_t a, uint64_t b) { return b < a ? b : a; }
__device__ __forceinline__ uint64_t spot_add(uint64_t a, uint32_t d) { return a == kSpotInf ? kSpotInf : a + ((uint64_t)d << 32); }
__device__ __forceinline__ uint64_t spot_shfl_up(uint64_t v, uint32_t by)
{
    const uint32_t lo = __shfl_up((uint32_t)v, by, 64), hi = __shfl_up((uint32_t)(v >> 32), by, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t spot_shfl(uint64_t v, uint32_t from)
{
    const uint32_t lo = __shfl((uint32_t)v, (int)from, 64), hi = __shfl((uint32_t)(v >> 32), (int)from, 64);
    return ((uint64_t)hi << 32) | lo;
}

constexpr uint32_t kChainNone = 0xFFFFFFFFu;  // an unreachable prefix cost of the connected-word decoders (= SR_DIS_ERR)

// The connected-word decoders' word count, walk back through the levels and records (k_chain.hip, k_chain_live.hip): one wave
// per row, 64 prefix positions at a time.  A1 = the row's keys of level 1, E0 = its prefix costs of level 0, P entries per
// level (level l: A1 + (l - 1) * P, E0 + l * P); N = the row's frames (N = 0 reads nothing: no parse); words = the row's W
// word records, level_cost (optional) its W level costs.
__device__ __forceinline__ void chain_trace_row(const unsigned long long *A1, const uint32_t *E0, uint32_t P, uint32_t N, uint32_t W,
                                                uint32_t n_words_exact, uint32_t word_cost, const uint32_t *tpl_frames,
                                                const uint32_t *group_of_slot, const uint32_t *word_id, sr_chain_rec *rec, sr_chain_word *words,
                                                uint32_t *level_cost, uint32_t lane)
{
    // E_l(N) of every level; the count: the given one, or the first minimum in ascending l
    uint32_t c = kChainNone;
    if (N && lane >= 1 && lane <= W) c = E0[(size_t)lane * P + N];
    if (level_cost && lane >= 1 && lane <= W) level_cost[lane - 1] = c;
    uint32_t n = n_words_exact;
    if (!n) {
        uint64_t key = ((uint64_t)c << 32) | lane;  // lanes without a level carry all-ones costs and lose to none of them
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) key = spot_min(key, spot_shfl(key, lane ^ (uint32_t)d));
        n = (uint32_t)(key >> 32) == kChainNone ? 1u : (uint32_t)key;
    }
    const uint32_t total = __shfl(c, (int)n, 64);
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
        // the first position at or below p whose own word closes E_l there; E_l(p) is finite, so there is one above 0
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
            const uint32_t acc = (uint32_t)(key >> 32) - word_cost - (E - P)[start];  // E_{l-1}(start)
            words[l - 1] = sr_chain_word{word_id[group_of_slot[slot]], slot, start, end, acc, acc / (end - start + 1 + tpl_frames[slot]), cum, 0u};
        }
        in_words += end - start + 1;
        p = start;
    }
    if (lane == 0) *rec = sr_chain_rec{total, n, N - in_words, SR_CH_OK};
}

// The one-pass decoders' step of the trace (k_onepass.hip, k_onepass_live.hip), one wave per row: the first position q in
// [1, p] from above whose own word closes E there (A(q) reachable and A(q).cost == E(q)), 64 positions per step; returns q and
// its key, or 0: the rest of the row is filler
__device__ __forceinline__ uint32_t onepass_word_at(const unsigned long long *A, const uint32_t *E, uint32_t p, uint32_t lane, uint64_t *key)
{
    while (p >= 1) {  // (uniform)
        const bool mine = lane < p;  // position p - lane >= 1
        const uint64_t ky = mine ? A[p - lane] : kSpotInf;
        const uint32_t e = mine ? E[p - lane] : kChainNone;
        const unsigned long long hit = __ballot(mine && ky != kSpotInf && (uint32_t)(ky >> 32) == e);
        if (hit) {
            const uint32_t first = (uint32_t)__ffsll((long long)hit) - 1u;
            *key = spot_shfl(ky, first);
            return p - first;
        }
        p = p > 64u ? p - 64u : 0u;
    }
    return 0u;
}

}  // namespace sr
