// k_chain.hip -- connected-word decoding: level-building DTW over the template store (include/sr_engine.h, "connected-word
// decoding").  OPT-IN EXTENSION, no reference counterpart; the local distance is the reference's get_dis (DTW.C:45-62).
// gfx950 (MI355X, CDNA4) only; wave = 64 lanes; no MFMA (the path has no dense contraction), integer VALU + LDS.
//
// Level l holds the best parse of every prefix of a row into exactly l words.  Per row the scratch keeps
//   A_l(p), p = 0..max_frames   the best last word of a parse of in[0..p) into l words that ENDS at frame p - 1, as the key
//                               cost << 32 | start << 16 | slot (u64 minimum = the tie rule: cost, start, slot); all ones = none
//   E_l(p)                      the cost of the best parse of in[0..p) into l words, trailing frames skipped; SR_DIS_ERR = none
// and a call is init, then max_words x (k_chain_words, k_chain_close), then k_chain_trace, all on one stream.
//
// k_chain_words is k_spot's sweep -- the skewed anti-diagonal wavefront, one wave per (slot, row, chunk), the template staged
// in LDS, packed (cost, start) states (sr_spot_dev.h) -- with two changes.  Row 0 is a CHARGED start, E_{l-1}(col) + d, and
// unreachable where E_{l-1}(col) is; the end row is not reduced to windows: the key of every end frame col >= c0 goes to
// A_l(col + 1) with a 64-bit atomic minimum.  The minimum does not depend on the order of the waves, so two runs give the same
// bytes.  The lead-in of 2M - 2 columns stays exact, for the spotter's reason: a word that ends in column e >= c0 covers at
// most 2M - 1 columns, and the start charges E_{l-1} are a global array that does not depend on the chunk.
// Costs are u32 and exact: d <= 65 536, at most 3L cells per word over L frames, N <= 16 383, 16 words of word_cost <= 2^24.
#include "sr_dtw_plan.h"
#include "sr_spot_dev.h"
#include "sr_sweep_dev.h"

namespace sr {

__device__ __forceinline__ unsigned long long *chain_A(const ChainArgs &a, uint32_t row, uint32_t level)  // level 1..max_words
{
    return a.A + ((size_t)row * a.max_words + (level - 1)) * (a.max_frames + 1u);
}
__device__ __forceinline__ uint32_t *chain_E(const ChainArgs &a, uint32_t row, uint32_t level)  // level 0..max_words
{
    return a.E + ((size_t)row * (a.max_words + 1u) + level) * (a.max_frames + 1u);
}
__device__ __forceinline__ uint32_t chain_frames(const ChainArgs &a, uint32_t row)
{
    const uint32_t N = a.in_frames[(size_t)row * a.frames_stride];
    return N < a.max_frames ? N : a.max_frames;
}

// E_0 of every row and "no word yet" in every A
__global__ void __launch_bounds__(256) k_chain_init(const ChainArgs a)
{
    const uint32_t row = blockIdx.x, P = a.max_frames + 1u;
    uint32_t *e0 = chain_E(a, row, 0);
    const bool skip = a.skip_cost != kChainNone;
    for (uint32_t p = threadIdx.x; p < P; p += 256) e0[p] = skip ? p * a.skip_cost : (p ? kChainNone : 0u);
    unsigned long long *A = chain_A(a, row, 1);
    for (size_t i = threadIdx.x; i < (size_t)a.max_words * P; i += 256) A[i] = kSpotInf;
}

__global__ void __launch_bounds__(64 * kSpotWaves) k_chain_words(const ChainArgs a, const uint32_t level)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 ch_smem[];  // template rows [tpl_len][2], then the waves' boundary columns
    const uint32_t k = blockIdx.x, row = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t chunk = blockIdx.z * kSpotWaves + w;
    uint32_t M = a.tpl_valid[k] ? a.tpl_frames[k] : 0u;
    M = M < a.tpl_len ? M : a.tpl_len;
    ulonglong2 *s_col = (ulonglong2 *)(ch_smem + (size_t)a.tpl_len * 2) + (size_t)w * a.tpl_len;  // (Dd, min(Dd, Dn)) per row
    sweep_stage_tpl(ch_smem, a.tpl + (size_t)k * a.tpl_stride, M);
    __syncthreads();
    if (chunk >= a.n_chunks || !M) return;

    const uint32_t N = chain_frames(a, row);
    const uint32_t c0 = chunk * a.chunk_cols;              // the chunk's end frames [c0, cN)
    const uint32_t c1 = c0 + a.chunk_cols, cN = c1 < N ? c1 : N;
    if (c0 >= cN) return;
    const int16_t *in = a.mfcc + (size_t)row * a.max_frames * kCoef;
    const uint32_t *e_prev = chain_E(a, row, level - 1);
    unsigned long long *A = chain_A(a, row, level);
    const uint32_t cs = c0 > 2 * M - 2 ? c0 - (2 * M - 2) : 0u;  // the exact lead-in
    for (uint32_t x0 = cs; x0 < cN; x0 += 64) {  // (wave-uniform)
        const uint32_t col = x0 + lane;
        const bool live = col < cN;
        Row32 fi = row_from2(u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, 0u);
        uint32_t charge = kChainNone;  // E_{l-1}(col): what a word that starts in this column builds on
        if (live) {
            fi = sweep_frame(in + (size_t)col * kCoef);
            charge = e_prev[col];
        }
        const uint32_t end_lane = (cN - x0 < 64u ? cN - x0 : 64u) - 1;  // the sweep's last live lane
        SweepLane sw;
        for (uint32_t t = 0; t < M + end_lane; t++)
            sweep_step(ch_smem, s_col, nullptr, false, fi, charge, col, live, x0 != cs, 63, M, lane, t, sw);
        wave_sync();  // the boundary column is complete before the next sweep's lane 0 reads it

        // the key of each end frame of the chunk: (cost + word_cost, start, slot) -> A_l(col + 1); col + 1 <= N <= max_frames
        if (live && col >= c0 && sw.end_v != kSpotInf) atomicMin(&A[col + 1], sweep_end_key(sw.end_v, a.word_cost, k));
    }
}

// E_l(p) = min(A_l(p).cost, E_l(p-1) + skip) = min over j <= p of A_l(j).cost + (p - j) * skip: a prefix minimum of
// A_l(j).cost + (N - j) * skip in u64, less (N - p) * skip.  One workgroup per row: wave scans plus an LDS carry.
__global__ void __launch_bounds__(256) k_chain_close(const ChainArgs a, const uint32_t level)
{
    __shared__ uint64_t s_tot[4];
    const uint32_t row = blockIdx.x, P = a.max_frames + 1u, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t N = chain_frames(a, row);
    const unsigned long long *A = chain_A(a, row, level);
    uint32_t *E = chain_E(a, row, level);
    if (a.skip_cost == kChainNone) {  // no skipping: the costs themselves (all ones stays SR_DIS_ERR)
        for (uint32_t p = threadIdx.x; p < P; p += 256) E[p] = p <= N ? (uint32_t)(A[p] >> 32) : kChainNone;
        return;
    }
    const uint64_t skip = a.skip_cost;
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

// the word count, the walk back through the levels, the records (chain_trace_row, sr_spot_dev.h).  One wave per row.
__global__ void __launch_bounds__(64) k_chain_trace(const ChainArgs a)
{
    const uint32_t row = blockIdx.x, W = a.max_words;
    chain_trace_row(chain_A(a, row, 1), chain_E(a, row, 0), a.max_frames + 1u, chain_frames(a, row), W, a.n_words_exact, a.word_cost, a.tpl_frames,
                    a.group_of_slot, a.word_id, a.rec + row, a.words + (size_t)row * W, a.level_cost ? a.level_cost + (size_t)row * W : nullptr,
                    threadIdx.x);
}

void launch_chain(const ChainArgs &a, hipStream_t s)
{
    if (!a.n_rows || !a.K) return;
    const size_t lds = spot_lds_bytes(a.tpl_len);
    SR_LAUNCH_POINT(s, "k_chain_init");
    hipLaunchKernelGGL(k_chain_init, dim3(a.n_rows), dim3(256), 0, s, a);
    const dim3 grid(a.K, a.n_rows, (a.n_chunks + kSpotWaves - 1) / kSpotWaves);
    for (uint32_t l = 1; l <= a.max_words; l++) {
        SR_LAUNCH_POINT(s, "k_chain_words");
        hipLaunchKernelGGL(k_chain_words, grid, dim3(64 * kSpotWaves), lds, s, a, l);
        SR_LAUNCH_POINT(s, "k_chain_close");
        hipLaunchKernelGGL(k_chain_close, dim3(a.n_rows), dim3(256), 0, s, a, l);
    }
    SR_LAUNCH_POINT(s, "k_chain_trace");
    hipLaunchKernelGGL(k_chain_trace, dim3(a.n_rows), dim3(64), 0, s, a);
}
void launch_chain_init(const ChainArgs &a, hipStream_t s)
{
    SR_LAUNCH_POINT(s, "k_chain_init");
    hipLaunchKernelGGL(k_chain_init, dim3(a.n_rows), dim3(256), 0, s, a);
}
void launch_chain_close(const ChainArgs &a, uint32_t level, hipStream_t s)
{
    SR_LAUNCH_POINT(s, "k_chain_close");
    hipLaunchKernelGGL(k_chain_close, dim3(a.n_rows), dim3(256), 0, s, a, level);
}
const char *chain_allow_lds(uint32_t bytes) { return allow_dynamic_lds({{(const void *)k_chain_words, "k_chain_words"}}, bytes); }

}  // namespace sr
