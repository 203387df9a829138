// k_align.hip -- the optimal warping path of the full-DP scorer, and DTW barycentre averaging on top of it (include/sr_engine.h,
// "full-DP alignment and word models from many examples").  OPT-IN EXTENSION, no reference counterpart; the local distance is
// the reference's get_dis (DTW.C:45-62), the cells are those of dtw_limit (DTW.C:76-109), the mean is get_mean's s32 division.
// gfx950 (MI355X, CDNA4) only; wave = 64 lanes; no MFMA (the path has no dense contraction), integer VALU + LDS.
//
// k_dp_align: the skewed anti-diagonal wavefront of k_dtw_dp_wave64, one wave = one workgroup per pair.  Lane = one input frame
// (column), at step t it meets reference row t - lane; D(x-1,y) is the left lane's value of the previous step (__shfl_up),
// D(x-1,y-1) that of the step before, D(x,y-1) the lane's own last value; 64 columns are swept at a time and the last column of
// a sweep goes through LDS to the next.  The values and their order of evaluation are k_dtw_dp_wave64's, so acc / (N + R) is
// that kernel's score.  What is new: every cell also records WHICH predecessor it took, 2 bits (0 = (x-1,y-1), 1 = (x-1,y),
// 2 = (x,y-1)), chosen by strict comparisons in the tie order of the definition -- not by whichever operand a min() returns.
// A lane packs the marks of 16 consecutive reference rows of its column into one word and stores it when the word is full or
// the column ends: word (x, y / 16) at marks[x * mark_w + y / 16].  The marks live in LDS behind the reference image and the
// boundary column when the launch plan says so (align_plan, sr_dtw_plan.h), else in global scratch.
// Then lane 0 walks back from (N-1, R-1) to (0, 0) along the marks, one dependent read per path point, and writes the span of
// every input frame as it leaves the frame; the other lanes fill the span entries past N.  A cell that was reached has a reached
// predecessor, so the walk only ever reads marks of cells inside the band; it is bounded by N + R steps all the same.
#include "sr_dtw_dev.h"
#include "sr_dtw_plan.h"

namespace sr {

constexpr uint32_t kAlInf = 0xFFFFFFFFu;

__global__ void __launch_bounds__(64) k_dp_align(const AlignArgs a)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 al_smem[];  // reference rows [ref_rows][2], boundary column, marks
    const uint32_t lane = threadIdx.x, row = a.row0 + blockIdx.x;
    uint32_t *s_col = (uint32_t *)(al_smem + (size_t)a.ref_rows * 2);
    uint32_t *marks = a.marks ? a.marks + (size_t)blockIdx.x * a.mark_words : s_col + a.ref_rows;

    uint32_t N = a.in_frames[(size_t)row * a.frames_stride];
    N = N < a.max_frames ? N : a.max_frames;
    const uint32_t ri = a.ref_of_row ? a.ref_of_row[row] : row;
    uint32_t R = ri < a.n_ref ? a.ref_frames[ri] : 0u;
    if (R > a.ref_rows) R = 0;  // an invalid reference
    uint32_t status = SR_AL_OK;
    if (N > SR_ALIGN_MAX_FRAMES) status = SR_AL_TOO_LONG;
    else if (!N || !R || N > 2 * R || 2 * N < R) status = SR_AL_GATED;

    uint32_t acc = kAlInf;
    if (status == SR_AL_OK) {  // (workgroup-uniform)
        const int16_t *ref = a.ref + (size_t)ri * a.ref_rows * kCoef;
        for (uint32_t r = lane; r < R; r += 64) {  // 24-byte rows + squared norm, as dp_wave64_stage
            const uint2 *src = (const uint2 *)(ref + (size_t)r * kCoef);
            const uint2 q0 = src[0], q1 = src[1], q2 = src[2];
            const Row32 f = row_from2(u32x2{q0.x, q0.y}, u32x2{q1.x, q1.y}, u32x2{q2.x, q2.y}, 0u);
            al_smem[2 * r] = u32x4{q0.x, q0.y, q1.x, q1.y};
            al_smem[2 * r + 1] = u32x4{q2.x, q2.y, (uint32_t)dot_rows(f, f), 0u};
        }
        wave_sync();
        const int in_n = (int)N, mdl_n = (int)R;
        const int X1 = ((2 * mdl_n - in_n) / 3) & 0xFFFF, X2 = ((4 * in_n - 2 * mdl_n) / 3) & 0xFFFF;  // DTW.C:141-142
        const int16_t *in = a.mfcc + (size_t)row * a.max_frames * kCoef;
        for (uint32_t x0 = 0; x0 < N; x0 += 64) {  // (wave-uniform)
            const uint32_t col = x0 + lane;
            const bool live = col < N;
            Row32 fi;
            {
                const uint2 *src = (const uint2 *)(in + (size_t)(live ? col : 0) * kCoef);
                const uint2 q0 = src[0], q1 = src[1], q2 = src[2];
                fi = row_from2(u32x2{q0.x, q0.y}, u32x2{q1.x, q1.y}, u32x2{q2.x, q2.y}, 0u);
                fi.w[6] = (uint32_t)dot_rows(fi, fi);
            }
            uint32_t up = kAlInf;    // D(col, r - 1), own previous step
            uint32_t left = kAlInf;  // D(col - 1, r) as delivered last step = this step's diagonal
            uint32_t mw = 0;         // the marks of the current 16 rows of this column
            uint32_t *mcol = marks + (size_t)col * a.mark_w;
            const uint32_t steps = R + (N - x0 < 64u ? N - x0 : 64u) - 1;
            for (uint32_t t = 0; t < steps; t++) {
                const int r = (int)t - (int)lane;
                uint32_t from_left = __shfl_up(up, 1, 64);
                if (lane == 0) from_left = (x0 == 0 || r >= mdl_n) ? kAlInf : s_col[r];  // (lane 0: r = t >= 0)
                const uint32_t diag = left;
                const bool in_range = live && r >= 0 && r < mdl_n;
                if (in_range) {
                    uint32_t cur = kAlInf, dir = 0;
                    if (!dtw_out((int)col + 1, r + 1, X1, X2, in_n, mdl_n)) {
                        const Row32 fm = row_from(al_smem[2 * r], al_smem[2 * r + 1]);
                        const uint32_t d = dis_from(fi.w[6], fm.w[6], dot_rows(fi, fm));
                        // the tie order: (x-1,y-1), then (x-1,y), then (x,y-1) -- a later candidate must be strictly smaller
                        uint32_t best = diag;
                        if (from_left < best) best = from_left, dir = 1;
                        if (up < best) best = up, dir = 2;
                        if (col == 0 && r == 0) best = 0;  // D(1,1) = d(1,1)
                        // (no saturation: d < 2^16 and a path has at most N + R <= 2048 points)
                        if (best != kAlInf) cur = best + d;
                    }
                    up = cur;
                    mw |= dir << (2 * (r & 15));
                    if ((r & 15) == 15 || r == mdl_n - 1) {
                        mcol[r >> 4] = mw;
                        mw = 0;
                    }
                    if (lane == 63) s_col[r] = cur;  // the last column of the sweep, for the next one
                    if (col == N - 1 && r == mdl_n - 1) acc = cur;
                }
                left = from_left;
            }
            wave_sync();
        }
        acc = wave_min_u32(acc);  // the end cell lives in exactly one lane
        if (acc == kAlInf) status = SR_AL_GATED;
    }

    uint32_t path_len = 0;
    uint32_t *span = a.span ? a.span + (size_t)(row - a.out0) * a.max_frames : nullptr;
    if (status == SR_AL_OK) {
        if (a.marks) __threadfence();  // the other lanes' mark words are in memory before lane 0 reads them
        if (lane == 0) {
            int x = (int)N - 1, y = (int)R - 1, y_last = y;
            for (uint32_t it = 0; it < N + R; it++) {
                path_len++;
                if (x == 0 && y == 0) {
                    if (span) span[0] = (uint32_t)y_last << 16;
                    break;
                }
                uint32_t dir = (marks[(size_t)x * a.mark_w + (y >> 4)] >> (2 * (y & 15))) & 3u;
                if (x == 0) dir = 2;  // (what the marks say there anyway: the only predecessor inside the grid)
                if (y == 0) dir = 1;
                if (dir == 2) {
                    y--;
                } else {
                    if (span) span[x] = (uint32_t)y | ((uint32_t)y_last << 16);
                    x--;
                    y -= dir == 0;
                    y_last = y;
                }
            }
        }
    }
    if (span)
        for (uint32_t x = (status == SR_AL_OK ? N : 0u) + lane; x < a.max_frames; x += 64) span[x] = 0xFFFFFFFFu;
    if (lane == 0) {
        const bool ok = status == SR_AL_OK;
        a.rec[row - a.out0] = sr_align_rec{ok ? acc / (N + R) : SR_DIS_ERR, ok ? acc : 0xFFFFFFFFu, path_len, status};
    }
}

// The path points of the OK pairs of a launch, summed into their models' accumulators.  One workgroup per example; a thread
// takes a centroid row y: the input frames matched to it are one contiguous run [lo, hi] (the path is monotone: y_first and
// y_last do not decrease with x), found by two binary searches in the example's span row, summed privately, and added with one
// integer atomic per (row, coefficient) and one for the count.  Integer sums: the order of arrival does not matter.
__global__ void __launch_bounds__(64) k_align_accum(const AlignAccumArgs a)
{
    const uint32_t e = a.row0 + blockIdx.x, m = a.model_of[e];
    const sr_align_rec rec = a.rec[blockIdx.x];
    const bool ok = rec.status == SR_AL_OK;
    if (threadIdx.x == 0 && a.stats) {
        if (ok) {
            atomicAdd(&a.stats[m].n_ok, 1u);
            atomicAdd((unsigned long long *)&a.stats[m].acc, (unsigned long long)rec.acc);
        } else {
            atomicAdd(&a.stats[m].n_fail, 1u);
        }
    }
    if (!ok) return;
    uint32_t N = a.in_frames[(size_t)e * a.frames_stride];
    N = N < a.max_frames ? N : a.max_frames;
    const uint32_t F = a.cen_frames[m];  // (an OK record: 1 <= F <= cen_rows)
    const uint32_t *span = a.span + (size_t)blockIdx.x * a.max_frames;
    const int16_t *in = a.mfcc + (size_t)e * a.max_frames * kCoef;
    for (uint32_t y = threadIdx.x; y < F; y += 64) {
        uint32_t lo = 0, n = N;  // first x with y_last(x) >= y
        while (n) {
            const uint32_t half = n >> 1;
            if ((span[lo + half] >> 16) < y) lo += half + 1, n -= half + 1;
            else n = half;
        }
        uint32_t hi = lo;  // first x with y_first(x) > y, at or after lo
        n = N - lo;
        while (n) {
            const uint32_t half = n >> 1;
            if ((span[hi + half] & 0xFFFFu) <= y) hi += half + 1, n -= half + 1;
            else n = half;
        }
        int s[kCoef];
#pragma unroll
        for (int c = 0; c < kCoef; c++) s[c] = 0;
        for (uint32_t x = lo; x < hi; x++) {
            const Frame12 f = load_frame(in + (size_t)x * kCoef);
#pragma unroll
            for (int i = 0; i < 6; i++) {
                s[2 * i] += sext_lo(f.w[i]);
                s[2 * i + 1] += sext_hi(f.w[i]);
            }
        }
        int32_t *sum = a.sum + ((size_t)m * a.cen_rows + y) * kCoef;
#pragma unroll
        for (int c = 0; c < kCoef; c++) atomicAdd(sum + c, s[c]);
        atomicAdd(a.cnt + (size_t)m * a.cen_rows + y, hi - lo);
    }
}

// One thread per centroid row: the division (get_mean's: s32, truncating toward zero), "keep the row nobody was matched to",
// zero rows past the model's length, an invalid centroid copied through; and the accumulators cleared for the next iteration.
__global__ void __launch_bounds__(256) k_align_finalise(const AlignFinalArgs a)
{
    const uint64_t n = (uint64_t)a.M * a.cen_rows;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t m = (uint32_t)(i / a.cen_rows), y = (uint32_t)(i % a.cen_rows);
        const uint32_t F = a.cen_frames[m];
        const bool valid = F >= 1 && F <= a.cen_rows;
        Frame12 o;
#pragma unroll
        for (int k = 0; k < 6; k++) o.w[k] = 0;
        if (!valid || y < F) {
            o = load_frame(a.cen_cur + i * kCoef);
            const uint32_t cnt = a.cnt[i];
            if (valid && cnt) {
                int32_t *sum = a.sum + i * kCoef;
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    o.w[k] = pack16(sum[2 * k] / (int)cnt, sum[2 * k + 1] / (int)cnt);
                    sum[2 * k] = sum[2 * k + 1] = 0;
                }
                a.cnt[i] = 0;
            }
        }
        uint2 *dst = (uint2 *)(a.cen_next + i * kCoef);
        dst[0] = make_uint2(o.w[0], o.w[1]);
        dst[1] = make_uint2(o.w[2], o.w[3]);
        dst[2] = make_uint2(o.w[4], o.w[5]);
    }
}

void launch_align(const AlignArgs &a, size_t lds_bytes, hipStream_t s)
{
    if (!a.n_pairs) return;
    SR_LAUNCH_POINT(s, "k_dp_align");
    hipLaunchKernelGGL(k_dp_align, dim3(a.n_pairs), dim3(64), lds_bytes, s, a);
}
void launch_align_accum(const AlignAccumArgs &a, hipStream_t s)
{
    if (!a.n_pairs) return;
    SR_LAUNCH_POINT(s, "k_align_accum");
    hipLaunchKernelGGL(k_align_accum, dim3(a.n_pairs), dim3(64), 0, s, a);
}
void launch_align_finalise(const AlignFinalArgs &a, hipStream_t s)
{
    const uint64_t n = (uint64_t)a.M * a.cen_rows, blocks = (n + 255) / 256;
    if (!n) return;
    SR_LAUNCH_POINT(s, "k_align_finalise");
    hipLaunchKernelGGL(k_align_finalise, dim3((uint32_t)(blocks < 65536u ? blocks : 65536u)), dim3(256), 0, s, a);
}
const char *align_allow_lds(uint32_t bytes) { return allow_dynamic_lds({{(const void *)k_dp_align, "k_dp_align"}}, bytes); }

}  // namespace sr
