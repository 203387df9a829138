// k_cluster.hip -- k-means under DTW for word models (include/sr_engine.h, "word models: clustering a word's examples").
// OPT-IN EXTENSION, no reference counterpart; the local distance is the reference's get_dis (DTW.C:45-62), the cells are those
// of dtw_limit (DTW.C:76-109).  gfx950 (MI355X, CDNA4) only; wave = 64 lanes; no MFMA (the path has no dense contraction),
// integer VALU + LDS.
//
// k_cluster_score: the accumulated cost of every (example, model of its word) pair -- k_dp_align's recurrence in k_dp_align's
// order of evaluation (k_align.hip: lane = input frame, skewed anti-diagonals, 64 columns per sweep, the last column of a sweep
// handed to the next through LDS), so acc and acc / (N + R) are that kernel's values bit for bit; no predecessor marks, no
// trace-back.  What the aligner cannot do is share: there one wave = one workgroup stages the reference for itself.  Here a
// workgroup serves ONE model and up to kClusterWaves examples of its word (the host's list, sr_cluster_plan.h): the centroid
// image (24-byte rows + squared norm, as k_dp_align and dp_wave64_stage build it) is staged once by all the waves, then
// every wave walks its own example against it with a boundary column of its own -- k_dtw_dp_wave64's sharing, applied to a
// reference array that is not the engine's store and to a per-model row range.
// LDS: [cen_rows][2] u32x4 image | kClusterWaves x [cen_rows] u32 boundary columns = cluster_lds_bytes (sr_dtw_plan.h).
// Every scores[e][c] is written exactly once, by a plain vector store: column c by the workgroup of model mdl0 + c, the
// columns past the word's model count by the workgroup of the word's first model.
//
// k_cluster_assign: one thread per example, the first minimum of at most 16 scores; k_cluster_tally: one thread per model.
#include "sr_dtw_dev.h"
#include "sr_dtw_plan.h"

namespace sr {

constexpr uint32_t kClInf = 0xFFFFFFFFu;

__global__ void __launch_bounds__(64 * kClusterWaves) k_cluster_score(const ClusterScoreArgs a)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 cl_smem[];  // centroid rows [cen_rows][2], one boundary column per wave
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t *g = a.wg + (size_t)(a.wg0 + blockIdx.x) * 3;
    const uint32_t m = g[0], e = g[1] + w, n_ex = g[2];
    uint32_t *s_col = (uint32_t *)(cl_smem + (size_t)a.cen_rows * 2) + (size_t)w * a.cen_rows;
    uint32_t R = a.cen_frames[m];
    if (R > a.cen_rows) R = 0;  // an invalid centroid
    {
        const int16_t *ref = a.cen + (size_t)m * a.cen_rows * kCoef;
        for (uint32_t r = threadIdx.x; r < R; r += 64 * kClusterWaves) {  // 24-byte rows + squared norm, as k_dp_align
            const uint2 *src = (const uint2 *)(ref + (size_t)r * kCoef);
            const uint2 q0 = src[0], q1 = src[1], q2 = src[2];
            const Row32 f = row_from2(u32x2{q0.x, q0.y}, u32x2{q1.x, q1.y}, u32x2{q2.x, q2.y}, 0u);
            cl_smem[2 * r] = u32x4{q0.x, q0.y, q1.x, q1.y};
            cl_smem[2 * r + 1] = u32x4{q2.x, q2.y, (uint32_t)dot_rows(f, f), 0u};
        }
    }
    __syncthreads();
    if (w >= n_ex) return;  // (wave-uniform; no barrier follows)

    uint32_t N = a.in_frames[(size_t)e * a.frames_stride];
    N = N < a.max_frames ? N : a.max_frames;
    const bool ok_pair = N <= SR_ALIGN_MAX_FRAMES && N && R && !(N > 2 * R || 2 * N < R);
    uint32_t acc = kClInf;
    if (ok_pair) {  // (wave-uniform)
        const int in_n = (int)N, mdl_n = (int)R;
        const int X1 = ((2 * mdl_n - in_n) / 3) & 0xFFFF, X2 = ((4 * in_n - 2 * mdl_n) / 3) & 0xFFFF;  // DTW.C:141-142
        const int16_t *in = a.mfcc + (size_t)e * a.max_frames * kCoef;
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
            uint32_t up = kClInf;    // D(col, r - 1), own previous step
            uint32_t left = kClInf;  // D(col - 1, r) as delivered last step = this step's diagonal
            const uint32_t steps = R + (N - x0 < 64u ? N - x0 : 64u) - 1;
            for (uint32_t t = 0; t < steps; t++) {
                const int r = (int)t - (int)lane;
                uint32_t from_left = __shfl_up(up, 1, 64);
                if (lane == 0) from_left = (x0 == 0 || r >= mdl_n) ? kClInf : s_col[r];  // (lane 0: r = t >= 0)
                const uint32_t diag = left;
                if (live && r >= 0 && r < mdl_n) {
                    uint32_t cur = kClInf;
                    if (!dtw_out((int)col + 1, r + 1, X1, X2, in_n, mdl_n)) {
                        const Row32 fm = row_from(cl_smem[2 * r], cl_smem[2 * r + 1]);
                        const uint32_t d = dis_from(fi.w[6], fm.w[6], dot_rows(fi, fm));
                        uint32_t best = diag;
                        if (from_left < best) best = from_left;
                        if (up < best) best = up;
                        if (col == 0 && r == 0) best = 0;  // D(1,1) = d(1,1)
                        // (no saturation: d < 2^16 and a path has at most N + R <= 2048 points)
                        if (best != kClInf) cur = best + d;
                    }
                    up = cur;
                    if (lane == 63) s_col[r] = cur;  // the last column of the sweep, for the next one
                    if (col == N - 1 && r == mdl_n - 1) acc = cur;
                }
                left = from_left;
            }
            wave_sync();
        }
        acc = wave_min_u32(acc);  // the end cell lives in exactly one lane
    }
    const uint32_t c = m - a.ex_mdl0[e], nm = a.ex_nm[e];
    const size_t at = (size_t)e * kClusterMax;
    if (lane == 0) {
        a.dis[at + c] = acc != kClInf ? acc / (N + R) : SR_DIS_ERR;
        if (a.acc) a.acc[at + c] = acc;
    } else if (c == 0 && lane >= nm && lane < kClusterMax) {  // the columns no model of this word owns
        a.dis[at + lane] = SR_DIS_ERR;
        if (a.acc) a.acc[at + lane] = kClInf;
    }
}

__global__ void __launch_bounds__(256) k_cluster_assign(const ClusterAssignArgs a)
{
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    const bool in = e < a.E;
    uint32_t best = SR_DIS_ERR, pick = SR_CLUSTER_NONE, acc = 0;
    bool moved = false;
    if (in) {
        const uint32_t nm = a.ex_nm[e];
        const uint32_t *row = a.dis + (size_t)e * kClusterMax;
        uint32_t c_best = 0;
        for (uint32_t c = 0; c < nm; c++) {  // the first minimum in model order
            const uint32_t s = row[c];
            if (s < best) best = s, c_best = c;
        }
        if (best != SR_DIS_ERR) {
            pick = a.ex_mdl0[e] + c_best;
            if (a.stats) acc = a.acc[(size_t)e * kClusterMax + c_best];
        }
        moved = pick != (a.prev ? a.prev[e] : SR_CLUSTER_NONE);
        if (a.cur) a.cur[e] = pick;
        if (a.assign) a.assign[e] = pick;
        if (a.best) a.best[e] = best;
        if (a.stats && pick != SR_CLUSTER_NONE) {
            atomicAdd(&a.stats[pick].n_ok, 1u);
            atomicAdd((unsigned long long *)&a.stats[pick].acc, (unsigned long long)acc);
        }
    }
    if (a.iter) {  // one integer atomic per wave and counter
        const uint32_t n_as = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(in && pick != SR_CLUSTER_NONE));
        const uint32_t n_un = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(in && pick == SR_CLUSTER_NONE));
        const uint32_t n_mv = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(in && moved));
        if ((threadIdx.x & 63) == 0) {
            if (n_as) atomicAdd(&a.iter->n_assigned, n_as);
            if (n_un) atomicAdd(&a.iter->n_unassigned, n_un);
            if (n_mv) atomicAdd(&a.iter->n_moved, n_mv);
        }
    }
}

__global__ void __launch_bounds__(256) k_cluster_tally(const sr_train_stat *stats, uint32_t M, sr_cluster_iter *iter)
{
    const uint32_t m = blockIdx.x * 256 + threadIdx.x;
    const bool in = m < M;
    const uint32_t n_ok = in ? stats[m].n_ok : 1u;
    const uint32_t n_empty = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(in && n_ok == 0));
    if ((threadIdx.x & 63) == 0 && n_empty) atomicAdd(&iter->n_empty, n_empty);
    if (in && n_ok) atomicAdd((unsigned long long *)&iter->acc, (unsigned long long)stats[m].acc);
}

void launch_cluster_score(const ClusterScoreArgs &a, size_t lds_bytes, hipStream_t s)
{
    if (!a.n_wg) return;
    SR_LAUNCH_POINT(s, "k_cluster_score");
    hipLaunchKernelGGL(k_cluster_score, dim3(a.n_wg), dim3(64 * kClusterWaves), lds_bytes, s, a);
}
void launch_cluster_assign(const ClusterAssignArgs &a, hipStream_t s)
{
    if (!a.E) return;
    SR_LAUNCH_POINT(s, "k_cluster_assign");
    hipLaunchKernelGGL(k_cluster_assign, dim3((a.E + 255) / 256), dim3(256), 0, s, a);
}
void launch_cluster_tally(const sr_train_stat *stats, uint32_t M, sr_cluster_iter *iter, hipStream_t s)
{
    SR_LAUNCH_POINT(s, "k_cluster_tally");
    hipLaunchKernelGGL(k_cluster_tally, dim3((M + 255) / 256), dim3(256), 0, s, stats, M, iter);
}
const char *cluster_allow_lds(uint32_t bytes) { return allow_dynamic_lds({{(const void *)k_cluster_score, "k_cluster_score"}}, bytes); }

}  // namespace sr
