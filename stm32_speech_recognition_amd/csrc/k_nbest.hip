// k_nbest.hip -- word-level N-best: a row of K slot distances reduced to its n_best best WORDS (include/sr_engine.h, "words
// instead of slots").  EXTENSION of the result format; the definition is the firmware's slot scan (main.c:283-289) with its
// min_comm /= ftr_per_comm (main.c:292) generalised to any slot -> word map, repeated n_best times.
// gfx950 (MI355X, CDNA4) only; wave = 64 lanes; integer VALU, no LDS, no atomics.
#include "sr_device.h"

namespace sr {

// One wave per score row, four rows per workgroup (k_argmin's shape; the row is read once from HBM, every later touch hits L1).
// The host has grouped the slots by word (NbestArgs::order / group_start), so a lane owns WHOLE words -- lane, lane + 64, ... --
// and reduces each of them on its own to the 64-bit key dis << 32 | slot: the minimum of the keys of a word's matching slots is
// its first minimum in slot order (strict <, main.c:285), and keys of different words differ because slots do.  Selection is
// n_best rounds of a wave-wide minimum over the keys not yet emitted (>= the last one + 1); the lane that owns the winning key
// writes the entry -- one lane per entry, one 16-byte record each, every entry of the row written exactly once.
// kRegs: up to 4 words per lane (256 words) keep key and count in registers between the rounds; stores with more words
// recompute a word's key from the L1-resident row in every round.
// Build knobs of profiles/experiments/nbest_ab.py --shapes (same-box A/B of the two variants): words per lane kept in registers,
// and the largest word count the register variant takes (0: every store recomputes).
#ifndef SR_NBEST_REG_WORDS
#define SR_NBEST_REG_WORDS 4
#endif
#ifndef SR_NBEST_REG_LIMIT
#define SR_NBEST_REG_LIMIT (64 * SR_NBEST_REG_WORDS)
#endif
constexpr uint32_t kNbestRegWords = SR_NBEST_REG_WORDS;
constexpr uint64_t kNoKey = ~0ull;  // above every key: a matching slot has dis <= 0xFFFFFFFE

__device__ __forceinline__ uint64_t nbest_word_key(const NbestArgs &a, const uint32_t *sc, uint32_t w, uint32_t *count)
{
    uint64_t key = kNoKey;
    uint32_t c = 0;
    const uint32_t p1 = a.group_start[w + 1];
    for (uint32_t p = a.group_start[w]; p < p1; p++) {
        const uint32_t k = a.order[p], d = sc[k];
        if (d != SR_DIS_ERR) {
            const uint64_t kd = (uint64_t)d << 32 | k;
            key = kd < key ? kd : key;
            c++;
        }
    }
    *count = c;
    return key;
}

template <bool kRegs>
__global__ void __launch_bounds__(256) k_nbest(const NbestArgs a)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.n_rows) return;  // (wave-uniform: the last workgroup may be partly empty)
    const uint32_t *sc = a.scores + (size_t)row * a.K;
    sr_nbest_entry *out = a.out + (size_t)row * a.n_best;
    uint64_t keys[kNbestRegWords];
    uint32_t cnts[kNbestRegWords];
    if (kRegs || a.n_matched) {  // every word once: its key and count, and the number of candidates of the row
        uint32_t matched = 0;
        if (kRegs) {
#pragma unroll
            for (uint32_t i = 0; i < kNbestRegWords; i++) {
                const uint32_t w = lane + 64 * i;
                keys[i] = kNoKey;
                cnts[i] = 0;
                if (w < a.n_words) keys[i] = nbest_word_key(a, sc, w, &cnts[i]);
                matched += keys[i] != kNoKey;
            }
        } else {
            for (uint32_t w = lane; w < a.n_words; w += 64) {
                uint32_t c;
                matched += nbest_word_key(a, sc, w, &c) != kNoKey;
            }
        }
        if (a.n_matched) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) matched += __shfl_xor(matched, d, 64);
            if (lane == 0) a.n_matched[row] = matched;
        }
    }
    uint64_t lo = 0;  // keys below it have been emitted
    uint32_t r = 0;
    for (; r < a.n_best; r++) {
        uint64_t best = kNoKey;
        uint32_t bw = 0, bc = 0;
        if (kRegs) {
#pragma unroll
            for (uint32_t i = 0; i < kNbestRegWords; i++) {
                if (keys[i] >= lo && keys[i] < best) {  // (kNoKey never passes the second test)
                    best = keys[i];
                    bw = lane + 64 * i;
                    bc = cnts[i];
                }
            }
        } else {
            for (uint32_t w = lane; w < a.n_words; w += 64) {
                uint32_t c;
                const uint64_t key = nbest_word_key(a, sc, w, &c);
                if (key >= lo && key < best) {
                    best = key;
                    bw = w;
                    bc = c;
                }
            }
        }
        uint64_t m = best;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t oh = __shfl_xor((uint32_t)(m >> 32), d, 64), ol = __shfl_xor((uint32_t)m, d, 64);
            const uint64_t o = (uint64_t)oh << 32 | ol;
            m = o < m ? o : m;
        }
        if (m == kNoKey) break;  // (wave-uniform) no candidate left
        if (best == m) {         // the one lane that owns the winning word
            sr_nbest_entry e;
            e.word = a.word_id[bw];
            e.slot = (uint32_t)m;
            e.dis = (uint32_t)(m >> 32);
            e.count = bc;
            out[r] = e;
        }
        lo = m + 1;
    }
    for (uint32_t i = r + lane; i < a.n_best; i += 64) {  // entries past the last candidate
        sr_nbest_entry e;
        e.word = SR_NO_WORD;
        e.slot = 0xFFFFFFFFu;
        e.dis = SR_DIS_ERR;
        e.count = 0;
        out[i] = e;
    }
}

void launch_nbest(const NbestArgs &a, hipStream_t s)
{
    if (!a.n_rows) return;
    const dim3 grid((a.n_rows + 3) / 4), block(256);
    if (a.n_words <= (uint32_t)(SR_NBEST_REG_LIMIT)) {
        SR_LAUNCH_POINT(s, "k_nbest");
        hipLaunchKernelGGL(k_nbest<true>, grid, block, 0, s, a);
    } else {
        SR_LAUNCH_POINT(s, "k_nbest");
        hipLaunchKernelGGL(k_nbest<false>, grid, block, 0, s, a);
    }
}

}  // namespace sr
