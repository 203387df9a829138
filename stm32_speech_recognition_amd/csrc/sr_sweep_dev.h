// sr_sweep_dev.h -- the pieces every decoder kernel shares (k_chain*.hip, k_gram*.hip, k_forced.hip, k_onepass*.hip; the first
// two also k_spot.hip, k_spot_live.hip and k_span.hip): the staging of a template into LDS, the load of an input frame, one
// step of the skewed anti-diagonal sweep of 64 columns with a charged start, the key of an end frame, the windowed close and
// the minimum over a grammar's charge list.  Plain inline functions: a kernel keeps its own prologue (which slot, row or
// channel, which columns), the step loop, its barriers and its epilogue.  gfx950 (MI355X, CDNA4) only; wave = 64 lanes.
#pragma once
#include "sr_spot_dev.h"

namespace sr {

// The M rows of a template (tpl: its first row) into smem[2 * r], smem[2 * r + 1]: the 24-byte row, then its squared norm.  By
// the whole workgroup; the caller's __syncthreads() follows.
__device__ __forceinline__ void sweep_stage_tpl(u32x4 *smem, const int16_t *tpl, uint32_t M)
{
    for (uint32_t r = threadIdx.x; r < M; r += blockDim.x) {  // 24-byte rows + squared norm, as dp_wave64_stage
        const uint2 *src = (const uint2 *)(tpl + (size_t)r * kCoef);
        const uint2 q0 = src[0], q1 = src[1], q2 = src[2];
        Row32 f = row_from2(u32x2{q0.x, q0.y}, u32x2{q1.x, q1.y}, u32x2{q2.x, q2.y}, 0u);
        smem[2 * r] = u32x4{q0.x, q0.y, q1.x, q1.y};
        smem[2 * r + 1] = u32x4{q2.x, q2.y, (uint32_t)dot_rows(f, f), 0u};
    }
}

// the input frame at `frame` (24 bytes, 8-byte aligned) with its squared norm in w[6]
__device__ __forceinline__ Row32 sweep_frame(const int16_t *frame)
{
    const uint2 *src = (const uint2 *)frame;
    const uint2 q0 = src[0], q1 = src[1], q2 = src[2];
    Row32 fi = row_from2(u32x2{q0.x, q0.y}, u32x2{q1.x, q1.y}, u32x2{q2.x, q2.y}, 0u);
    fi.w[6] = (uint32_t)dot_rows(fi, fi);
    return fi;
}

// A lane's state in one sweep of 64 columns, lane = column: Dd and min(Dd, Dn) of (col, row - 1), the lane's last results;
// min(Dd, Dn) of (col - 1, row - 1), last step's value from the left; min(Dd, Dn) of (col, M - 1), all ones = no word ends here
struct SweepLane {
    uint64_t up_d = kSpotInf, up_m = kSpotInf, diag = kSpotInf, end_v = kSpotInf;
};

// Step t of a sweep over the M template rows staged in smem, lane = column `col` with frame fi: the lane stands in row
// t - lane.  Row 0 is a CHARGED start, charge + d, unreachable where charge is kChainNone.  `left`: lane 0 has a column to its
// left, in s_col; lane `last` hands its column on through s_col (the caller's wave_sync() follows the loop): 63 where only a
// full sweep has a successor, the last live lane where the column is also the state kept for a later launch.  `keep`: the
// lane's column goes to g_col as well.  The loop `for (t = 0; t < M + the last live lane; t++)` stays in the kernel: with the
// loop inside the helper seven of the twelve sweeps took two more VGPRs (profiles/experiments/RESULTS.md).
__device__ __forceinline__ void sweep_step(const u32x4 *smem, ulonglong2 *s_col, ulonglong2 *g_col, bool keep, const Row32 &fi, uint32_t charge,
                                           uint32_t col, bool live, bool left, uint32_t last, uint32_t M, uint32_t lane, uint32_t t, SweepLane &s)
{
    const int r = (int)t - (int)lane;
    // the left lane's results of the previous step are the states of (col - 1, r)
    uint64_t fl_d = spot_shfl_up(s.up_d, 1), fl_m = spot_shfl_up(s.up_m, 1);
    if (lane == 0) {
        fl_d = fl_m = kSpotInf;
        if (t < M && left) {  // (t < M first: tested the other way round, every step waits for its shuffles at the top)
            const ulonglong2 v = s_col[t];
            fl_d = v.x;
            fl_m = v.y;
        }
    }
    if (live && r >= 0 && r < (int)M) {
        const Row32 fm = row_from(smem[2 * r], smem[2 * r + 1]);
        const uint32_t d = dis_from(fi.w[6], fm.w[6], dot_rows(fi, fm));
        uint64_t cd = kSpotInf, cn;
        if (r > 0) {
            cd = spot_add(s.diag, d);
            cn = spot_add(spot_min(fl_d, s.up_d), d);
        } else {  // row 0: a charged start, of the non-diagonal kind
            cn = charge == kChainNone ? kSpotInf : ((uint64_t)(charge + d) << 32) | col;
        }
        s.up_d = cd;
        s.up_m = spot_min(cd, cn);
        if (lane == last) s_col[r] = ulonglong2{s.up_d, s.up_m};  // (lane 0 has read row r before it writes it)
        if (keep) g_col[r] = ulonglong2{s.up_d, s.up_m};
        if (r == (int)M - 1) s.end_v = s.up_m;
    }
    s.diag = fl_m;
}

// the key of an end frame, (cost + word_cost, start, slot): the u64 minimum over keys is the tie rule cost, start, slot
__device__ __forceinline__ unsigned long long sweep_end_key(uint64_t end_v, uint32_t word_cost, uint32_t slot)
{
    return ((uint64_t)((uint32_t)(end_v >> 32) + word_cost) << 32) | ((uint64_t)(uint32_t)end_v << 16) | slot;
}

// E(p), p in (lo, hi]: min(min over lo < j <= p of A(j).cost + (p - j) * skip, E(lo) + (p - lo) * skip), as a prefix minimum of
// A(j).cost + (hi - j) * skip in u64 that starts from the carried E(lo) + (hi - lo) * skip, less (hi - p) * skip.  By a whole
// workgroup of 256: wave scans plus an LDS carry in s_tot[4].  skip_cost == kChainNone: no skipping, the costs themselves.
__device__ __forceinline__ void close_window(const unsigned long long *A, uint32_t *E, uint32_t lo, uint32_t hi, uint32_t skip_cost, uint64_t *s_tot)
{
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (skip_cost == kChainNone) {  // (all ones stays SR_DIS_ERR)
        for (uint32_t p = lo + 1 + threadIdx.x; p <= hi; p += 256) E[p] = (uint32_t)(A[p] >> 32);
        return;
    }
    const uint64_t skip = skip_cost;
    const uint32_t e_lo = E[lo];  // (written by the close of the window before, or by an init)
    uint64_t carry = e_lo == kChainNone ? kSpotInf : (uint64_t)e_lo + (uint64_t)(hi - lo) * skip;
    for (uint32_t p0 = lo + 1; p0 <= hi; p0 += 256) {  // (uniform)
        const uint32_t p = p0 + threadIdx.x;
        uint64_t v = kSpotInf;
        if (p <= hi) {
            const uint64_t key = A[p];
            if (key != kSpotInf) v = (key >> 32) + (uint64_t)(hi - p) * skip;
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
        if (p <= hi) E[p] = m != kSpotInf ? (uint32_t)(m - (uint64_t)(hi - p) * skip) : kChainNone;
        for (uint32_t i = 0; i < 4; i++) carry = spot_min(carry, s_tot[i]);
        __syncthreads();  // s_tot is read before the next round overwrites it
    }
}

// C(col): what a word that starts in column col builds on, the minimum of E(col, s) over the states s of `mask` (state s at
// E + s * P), all ones where the column is not `charged`.  cost: null, or the arc costs of the list by ascending state, added
// to E; an unreachable E takes no cost (all ones + c would wrap to c - 1 and win).  The caller's `cost` is null or not at
// compile time (gram_costs_of below): one of the two forms is compiled, never a test inside the loop.
__device__ __forceinline__ uint32_t gram_charge(const uint32_t *E, uint32_t P, uint32_t col, bool charged, unsigned long long mask, const uint32_t *cost)
{
    uint32_t charge = kChainNone;
    uint32_t j = 0;
    for (unsigned long long m = mask; m; m &= m - 1, j++) {  // (wave-uniform)
        const uint32_t s = (uint32_t)__ffsll((long long)m) - 1u;
        const uint32_t e = charged ? E[(size_t)s * P + col] : kChainNone;
        if (cost) {
            const uint32_t v = e + cost[j];
            charge = (e != kChainNone && v < charge) ? v : charge;
        } else {
            charge = e < charge ? e : charge;
        }
    }
    return charge;
}

// the arc costs of charge list `set`, or null without costs.  The assumption tells the compiler what the host guarantees (a
// weighted grammar's cost block is allocated): without it gram_charge's test of `cost` survives in the weighted kernels, which
// then carry both loops and measured 1.5 to 2 % slower on a 31-state grammar.
__device__ __forceinline__ const uint32_t *gram_costs_of(const GramCosts *wt, uint32_t set)
{
    if (!wt) return nullptr;
    const uint32_t *cost = wt->cost + wt->cost_off[set];
    __builtin_assume(cost != nullptr);
    return cost;
}

}  // namespace sr
