// k_spot.hip -- word spotting: subsequence DTW of every template inside every feature row (include/sr_engine.h, "word
// spotting").  OPT-IN EXTENSION, no reference counterpart; the local distance is the reference's get_dis (DTW.C:45-62).
// gfx950 (MI355X, CDNA4) only; wave = 64 lanes; no MFMA (the path has no dense contraction), integer VALU + LDS.
//
//   D(x,0) = d(x,0), S(x,0) = x;  D(x,y) = d(x,y) + min(D(x-1,y-1), D(x-2,y-1) + d(x-1,y), D(x-1,y-2) + d(x,y-1))
// is evaluated in its two-state form: Dd = "arrived by a diagonal step" = d + min(Dd, Dn)(x-1,y-1), Dn = "arrived by a
// horizontal or vertical step" = d + min(Dd(x-1,y), Dd(x,y-1)), row 0 is of the Dn kind.  A state is the pair (cost, start)
// in one u64, cost in the high word, so that the tie rule (smallest start among equal costs) is the u64 minimum;
// unreachable = all ones (a cost stays below 2^31: d <= 65 536 and a path has at most 2M - 1 <= 32 765 cells).
//
// Layout: the skewed anti-diagonal wavefront of k_dtw_dp_wave64.  Lane = one utterance frame (column), at step t it meets
// template row t - lane; the left neighbour's states of the previous step arrive by __shfl_up, 64 columns are swept at a
// time and the last column of a sweep goes through LDS to the next.  The template is staged once per workgroup.
// Grid (slot, row, four chunks): a wave owns the end frames [c0, c1) of its chunk and starts its sweeps 2M - 2 columns
// earlier.  That is exact: a path that ends in column e >= c0 covers at most 2M - 1 columns, so it lies inside the columns
// the wave has seen, and D and S of the end row do not depend on anything before them.  Long rows therefore supply
// parallelism even when there are few of them.
// Windows: q(e) = D / (L + M) of the end row is reduced on the key (q, e) -- first minimum in ascending e = u64 minimum -- by
// a segmented scan over the lanes of a sweep plus a carry from sweep to sweep.  Chunks never straddle a window edge
// (spot_geom): either a chunk holds whole windows and writes their records, or it is one of the pieces of a long window and
// leaves a partial record that k_spot_finish reduces in chunk order.  No atomics; every record is written exactly once.
#include "sr_dtw_plan.h"
#include "sr_spot_dev.h"
#include "sr_sweep_dev.h"

namespace sr {

// the record of a window (or of a piece of one) from its key (q, e) and the winner's start and cost
__device__ __forceinline__ sr_spot_hit spot_record(uint64_t key, uint32_t start, uint32_t acc)
{
    if (key == kSpotInf) return sr_spot_hit{SR_DIS_ERR, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    return sr_spot_hit{(uint32_t)(key >> 32), start, (uint32_t)key, acc};
}
__device__ __forceinline__ uint64_t spot_key(const sr_spot_hit &r) { return ((uint64_t)r.dis << 32) | r.end; }

__global__ void __launch_bounds__(64 * kSpotWaves) k_spot(const SpotArgs a)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 sp_smem[];  // template rows [tpl_len][2], then the waves' boundary columns
    const uint32_t k = blockIdx.x, row = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t chunk = blockIdx.z * kSpotWaves + w;
    uint32_t M = a.tpl_valid[k] ? a.tpl_frames[k] : 0u;
    M = M < a.tpl_len ? M : a.tpl_len;
    ulonglong2 *s_col = (ulonglong2 *)(sp_smem + (size_t)a.tpl_len * 2) + (size_t)w * a.tpl_len;  // (Dd, min(Dd, Dn)) per row
    sweep_stage_tpl(sp_smem, a.tpl + (size_t)k * a.tpl_stride, M);
    __syncthreads();
    if (chunk >= a.n_chunks) return;

    // the chunk's end frames [c0, c1), its windows [w0, w1) and the length of a reduction segment
    uint32_t c0, c1, w0, w1, seg;
    if (a.split) {
        const uint32_t wv = chunk / a.per, i = chunk % a.per;
        c0 = wv * a.win + i * a.chunk_cols;
        c1 = c0 + a.chunk_cols < (wv + 1) * a.win ? c0 + a.chunk_cols : (wv + 1) * a.win;
        w0 = w1 = 0;
        seg = 0x40000000u;  // one segment: the chunk
    } else {
        w0 = chunk * a.per;
        w1 = w0 + a.per < a.n_win ? w0 + a.per : a.n_win;
        c0 = w0 * a.win;
        c1 = c0 + a.chunk_cols;
        seg = a.win;
    }
    uint32_t N = a.in_frames[(size_t)row * a.frames_stride];
    N = N < a.max_frames ? N : a.max_frames;
    const uint32_t cN = c1 < N ? c1 : N;  // end of the columns this chunk walks
    const bool has = M > 0 && c0 < cN;
    const size_t part_at = ((size_t)row * a.n_chunks + chunk) * a.K + k;
    auto put = [&](uint32_t wid, const sr_spot_hit &rec) {
        if (a.split) {
            a.part[part_at] = rec;
        } else {
            const size_t at = ((size_t)row * a.n_win + wid) * a.K + k;
            a.hits[at] = rec;
            if (a.scores) a.scores[at] = rec.dis;
        }
    };

    if (has) {
        const int16_t *in = a.mfcc + (size_t)row * a.max_frames * kCoef;
        const uint32_t cs = c0 > 2 * M - 2 ? c0 - (2 * M - 2) : 0u;  // the exact lead-in
        uint64_t carry_key = kSpotInf;
        uint32_t carry_s = 0xFFFFFFFFu, carry_d = 0xFFFFFFFFu, carry_wid = 0xFFFFFFFFu;
        for (uint32_t x0 = cs; x0 < cN; x0 += 64) {  // (wave-uniform)
            const uint32_t col = x0 + lane;
            const bool live = col < cN;
            Row32 fi = row_from2(u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, 0u);
            if (live) fi = sweep_frame(in + (size_t)col * kCoef);
            uint64_t up_d = kSpotInf, up_m = kSpotInf;  // Dd and min(Dd, Dn) of (col, row - 1): the lane's last results
            uint64_t diag = kSpotInf;                   // min(Dd, Dn) of (col - 1, row - 1): last step's value from the left
            uint64_t end_v = kSpotInf;                  // min(Dd, Dn) of (col, M - 1)
            const uint32_t steps = M + (cN - x0 < 64u ? cN - x0 : 64u) - 1;
            for (uint32_t t = 0; t < steps; t++) {
                const int r = (int)t - (int)lane;
                // the left lane's results of the previous step are the states of (col - 1, r)
                uint64_t fl_d = spot_shfl_up(up_d, 1), fl_m = spot_shfl_up(up_m, 1);
                if (lane == 0) {
                    fl_d = fl_m = kSpotInf;
                    if (x0 != cs && t < M) {
                        const ulonglong2 v = s_col[t];
                        fl_d = v.x;
                        fl_m = v.y;
                    }
                }
                if (live && r >= 0 && r < (int)M) {
                    const Row32 fm = row_from(sp_smem[2 * r], sp_smem[2 * r + 1]);
                    const uint32_t d = dis_from(fi.w[6], fm.w[6], dot_rows(fi, fm));
                    uint64_t cd = kSpotInf, cn = ((uint64_t)d << 32) | col;  // row 0: a start, of the non-diagonal kind
                    if (r > 0) {
                        cd = spot_add(diag, d);
                        cn = spot_add(spot_min(fl_d, up_d), d);
                    }
                    up_d = cd;
                    up_m = spot_min(cd, cn);
                    if (lane == 63) s_col[r] = ulonglong2{up_d, up_m};
                    if (r == (int)M - 1) end_v = up_m;
                }
                diag = fl_m;
            }
            wave_sync();  // the boundary column is complete before the next sweep's lane 0 reads it

            // q(e) of the sweep's end frames, then the first minimum per window: a segmented min-scan on (q, e)
            const uint32_t e_s = (uint32_t)end_v, e_d = (uint32_t)(end_v >> 32);
            uint64_t key = kSpotInf;
            if (end_v != kSpotInf && col >= c0) key = ((uint64_t)(e_d / (col - e_s + 1 + M)) << 32) | col;
            const uint32_t wid = col / seg;
#pragma unroll
            for (uint32_t by = 1; by < 64; by <<= 1) {
                const uint32_t o_wid = __shfl_up(wid, by, 64);
                const uint64_t o_key = spot_shfl_up(key, by);
                if (lane >= by && o_wid == wid) key = spot_min(key, o_key);
            }
            if (wid == carry_wid) key = spot_min(key, carry_key);
            // start and cost of the winner: its lane of this sweep, or the carry when it ended in an earlier one
            const uint32_t we = (uint32_t)key;
            uint32_t p_s = __shfl(e_s, (int)((we - x0) & 63u), 64), p_d = __shfl(e_d, (int)((we - x0) & 63u), 64);
            if (key != kSpotInf && we < x0) {
                p_s = carry_s;
                p_d = carry_d;
            }
            const uint32_t w_end = (wid + 1) * seg;  // (seg <= 2^30, wid = 0 there: no overflow)
            if (live && col >= c0 && col == (w_end < cN ? w_end : cN) - 1) put(wid, spot_record(key, p_s, p_d));
            carry_key = spot_shfl(key, 63);
            carry_s = __shfl(p_s, 63, 64);
            carry_d = __shfl(p_d, 63, 64);
            carry_wid = __shfl(wid, 63, 64);
        }
    }
    // what has no column below cN has no hit
    const sr_spot_hit none = spot_record(kSpotInf, 0u, 0u);
    if (a.split) {
        if (!has && lane == 0) put(0u, none);
    } else {
        for (uint32_t wv = (has ? (cN + a.win - 1) / a.win : w0) + lane; wv < w1; wv += 64) put(wv, none);
    }
}

// split launches: window by window, slot by slot, the first minimum of the pieces' records in chunk order
__global__ void __launch_bounds__(256) k_spot_finish(const SpotArgs a)
{
    const uint64_t n = (uint64_t)a.n_rows * a.n_win * a.K;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint64_t rw = i / a.K, k = i % a.K;
        sr_spot_hit best = spot_record(kSpotInf, 0u, 0u);
        for (uint32_t c = 0; c < a.per; c++) {
            const sr_spot_hit p = a.part[(rw * a.per + c) * a.K + k];
            if (spot_key(p) < spot_key(best)) best = p;
        }
        a.hits[i] = best;
        if (a.scores) a.scores[i] = best.dis;
    }
}

void launch_spot(const SpotArgs &a, hipStream_t s)
{
    if (!a.n_rows || !a.K) return;
    const size_t lds = spot_lds_bytes(a.tpl_len);
    // the rows are the grid's second dimension (<= 65 535): more go out in slices
    for (uint32_t r0 = 0; r0 < a.n_rows; r0 += 65535u) {
        SpotArgs sa = a;
        sa.n_rows = a.n_rows - r0 < 65535u ? a.n_rows - r0 : 65535u;
        sa.mfcc = a.mfcc + (size_t)r0 * a.max_frames * kCoef;
        sa.in_frames = a.in_frames + (size_t)r0 * a.frames_stride;
        sa.hits = a.hits + (size_t)r0 * a.n_win * a.K;
        sa.scores = a.scores ? a.scores + (size_t)r0 * a.n_win * a.K : nullptr;
        sa.part = a.part ? a.part + (size_t)r0 * a.n_chunks * a.K : nullptr;
        const dim3 grid(a.K, sa.n_rows, (a.n_chunks + kSpotWaves - 1) / kSpotWaves);
        SR_LAUNCH_POINT(s, "k_spot");
        hipLaunchKernelGGL(k_spot, grid, dim3(64 * kSpotWaves), lds, s, sa);
    }
    if (a.split) {
        const uint64_t n = (uint64_t)a.n_rows * a.n_win * a.K, blocks = (n + 255) / 256;
        SR_LAUNCH_POINT(s, "k_spot_finish");
        hipLaunchKernelGGL(k_spot_finish, dim3((uint32_t)(blocks < 65536u ? blocks : 65536u)), dim3(256), 0, s, a);
    }
}
const char *spot_allow_lds(uint32_t bytes) { return allow_dynamic_lds({{(const void *)k_spot, "k_spot"}}, bytes); }

}  // namespace sr
