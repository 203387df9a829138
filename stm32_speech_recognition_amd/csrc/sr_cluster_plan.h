// sr_cluster_plan.h -- host-side planning of the word-model clustering calls (include/sr_engine.h, "word models: clustering a
// word's examples"; sr_cluster.cpp): the checks on the two host arrays, the per-example model ranges, the workgroups of the
// score pass and how they are cut into launches.  HOST ONLY and free of HIP, so that tests/cluster_plan/plan_check.cpp can run
// it under the sanitizers on a machine without a device.
//
// A workgroup of k_cluster_score serves ONE model and up to kClusterWaves consecutive examples of that model's word, one per
// wave; the workgroups are listed model by model, and a launch takes a run of that list whose pairs stay within the budget.
#pragma once
#include <cstdint>
#include <vector>

namespace sr {

constexpr uint32_t kClusterMax = 16;             // SR_CLUSTER_MAX: models of one word, columns of a score row
constexpr uint32_t kClusterWaves = 4;            // examples (waves) of one k_cluster_score workgroup
constexpr uint32_t kClusterMaxPairs = 1u << 20;  // (example, model) pairs of one launch at most

// nullptr, or what is wrong with the arrays.  n_cap = min(max_frames, SR_ALIGN_MAX_FRAMES): the exactness bound of the s32
// accumulators, (examples of a word) x n_cap <= 65 535 -- any one model of the word may receive all of them.
inline const char *cluster_check(const uint32_t *word_start, const uint32_t *mdl_start, uint32_t W, uint32_t n_cap)
{
    if (!W) return "no words";
    if (word_start[0] != 0 || mdl_start[0] != 0) return "word_start and mdl_start must begin at 0";
    for (uint32_t w = 0; w < W; w++) {
        if (word_start[w + 1] < word_start[w] || mdl_start[w + 1] < mdl_start[w]) return "word_start and mdl_start must be ascending";
        const uint32_t nm = mdl_start[w + 1] - mdl_start[w];
        if (nm < 1 || nm > kClusterMax) return "every word needs 1..SR_CLUSTER_MAX models";
        if ((uint64_t)(word_start[w + 1] - word_start[w]) * n_cap > 65535u)
            return "too many examples of one word for exact s32 sums: examples x min(max_frames, SR_ALIGN_MAX_FRAMES) must not exceed 65535";
    }
    return nullptr;
}

struct ClusterPlan {
    uint32_t E = 0, M = 0, n_wg = 0;
    std::vector<uint32_t> tab;     // what goes to the device: mdl0[E] | n_mdl[E] | wg[n_wg][3] = (model, first example, examples)
    std::vector<uint32_t> cut;     // launch l takes the workgroups [cut[l], cut[l + 1])
    size_t wg_at() const { return (size_t)2 * E; }
};

// arrays that passed cluster_check.  max_pairs: pairs of one launch (1..kClusterMaxPairs)
inline ClusterPlan cluster_plan(const uint32_t *word_start, const uint32_t *mdl_start, uint32_t W, uint32_t max_pairs)
{
    ClusterPlan p;
    p.E = word_start[W];
    p.M = mdl_start[W];
    max_pairs = max_pairs < 1 ? 1 : max_pairs > kClusterMaxPairs ? kClusterMaxPairs : max_pairs;
    const uint32_t per = max_pairs < kClusterWaves ? max_pairs : kClusterWaves;  // examples of a workgroup
    p.tab.assign((size_t)2 * p.E, 0u);
    for (uint32_t w = 0; w < W; w++)
        for (uint32_t e = word_start[w]; e < word_start[w + 1]; e++) {
            p.tab[e] = mdl_start[w];
            p.tab[(size_t)p.E + e] = mdl_start[w + 1] - mdl_start[w];
        }
    p.cut.push_back(0);
    uint32_t in_launch = 0;  // pairs of the launch being filled
    for (uint32_t w = 0; w < W; w++)
        for (uint32_t m = mdl_start[w]; m < mdl_start[w + 1]; m++)
            for (uint32_t e = word_start[w]; e < word_start[w + 1]; e += per) {
                const uint32_t n = word_start[w + 1] - e < per ? word_start[w + 1] - e : per;
                if (in_launch + n > max_pairs) {
                    p.cut.push_back(p.n_wg);
                    in_launch = 0;
                }
                p.tab.push_back(m);
                p.tab.push_back(e);
                p.tab.push_back(n);
                p.n_wg++;
                in_launch += n;
            }
    if (p.cut.back() != p.n_wg) p.cut.push_back(p.n_wg);
    return p;
}

}  // namespace sr
