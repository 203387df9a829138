// The host-only planning of the word-model clustering calls (csrc/sr_cluster_plan.h) on the CPU, without a device: the checks
// on word_start / mdl_start, each example's model range, the score pass's workgroups and their cut into launches, over random
// corpora against properties stated from scratch -- every (example, model of its word) pair is covered exactly once, a
// workgroup holds 1..kClusterWaves examples of one word and one of its models, a launch stays within its budget.  A
// stand-alone program for the sanitizers:
//   hipcc --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I<csrc> plan_check.cpp -o plan_check && ./plan_check
// (tests/test_cluster_ref.py builds and runs it).  Prints "plan_check ok" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>

#include "sr_cluster_plan.h"

using namespace sr;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("plan_check: line %d: %s\n", __LINE__, #cond);     \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static uint32_t rnd(uint64_t &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
}

static int check_plan(const std::vector<uint32_t> &ws, const std::vector<uint32_t> &ms, uint32_t max_pairs)
{
    const uint32_t W = (uint32_t)ws.size() - 1;
    const ClusterPlan p = cluster_plan(ws.data(), ms.data(), W, max_pairs);
    const uint32_t budget = max_pairs < 1 ? 1 : max_pairs > kClusterMaxPairs ? kClusterMaxPairs : max_pairs;
    CHECK(p.E == ws[W] && p.M == ms[W]);
    CHECK(p.tab.size() == (size_t)2 * p.E + (size_t)3 * p.n_wg && p.wg_at() == (size_t)2 * p.E);
    std::vector<uint32_t> word_of(p.E);
    for (uint32_t w = 0; w < W; w++)
        for (uint32_t e = ws[w]; e < ws[w + 1]; e++) {
            word_of[e] = w;
            CHECK(p.tab[e] == ms[w] && p.tab[(size_t)p.E + e] == ms[w + 1] - ms[w]);
        }
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> seen;  // (example, model) -> times covered
    uint64_t pairs = 0;
    for (uint32_t i = 0; i < p.n_wg; i++) {
        const uint32_t *g = p.tab.data() + p.wg_at() + (size_t)3 * i;
        const uint32_t m = g[0], e0 = g[1], n = g[2];
        CHECK(n >= 1 && n <= kClusterWaves && n <= budget && m < p.M && e0 < p.E && e0 + n <= p.E);
        const uint32_t w = word_of[e0];
        CHECK(word_of[e0 + n - 1] == w && m >= ms[w] && m < ms[w + 1]);
        for (uint32_t e = e0; e < e0 + n; e++) seen[{e, m}]++;
        pairs += n;
    }
    uint64_t want = 0;
    for (uint32_t w = 0; w < W; w++) want += (uint64_t)(ws[w + 1] - ws[w]) * (ms[w + 1] - ms[w]);
    CHECK(pairs == want && seen.size() == want);
    for (const auto &kv : seen) CHECK(kv.second == 1);
    // the launches: a partition of the list into runs within the budget, none empty
    CHECK(!p.cut.empty() && p.cut.front() == 0 && p.cut.back() == p.n_wg);
    CHECK((p.n_wg == 0) == (p.cut.size() == 1));
    for (size_t l = 0; l + 1 < p.cut.size(); l++) {
        CHECK(p.cut[l] < p.cut[l + 1]);
        uint64_t in_launch = 0;
        for (uint32_t i = p.cut[l]; i < p.cut[l + 1]; i++) in_launch += p.tab[p.wg_at() + (size_t)3 * i + 2];
        CHECK(in_launch <= budget);
        // greedy: the next workgroup would not have fitted
        if (l + 2 < p.cut.size()) CHECK(in_launch + p.tab[p.wg_at() + (size_t)3 * p.cut[l + 1] + 2] > budget);
    }
    return 0;
}

int main()
{
    // the checks
    {
        const uint32_t ws[] = {0, 4, 4, 9}, ms[] = {0, 2, 3, 19};
        CHECK(cluster_check(ws, ms, 3, 80) == nullptr);
        CHECK(cluster_check(ws, ms, 0, 80) != nullptr);
        const uint32_t ws1[] = {1, 4, 4, 9}, ms1[] = {1, 2, 3, 19}, ws2[] = {0, 4, 3, 9}, ms2[] = {0, 2, 1, 19};
        CHECK(cluster_check(ws1, ms, 3, 80) && cluster_check(ws, ms1, 3, 80) && cluster_check(ws2, ms, 3, 80) && cluster_check(ws, ms2, 3, 80));
        const uint32_t ms3[] = {0, 2, 2, 18}, ms4[] = {0, 2, 3, 20};
        CHECK(cluster_check(ws, ms3, 3, 80) && std::strstr(cluster_check(ws, ms3, 3, 80), "1..SR_CLUSTER_MAX"));
        CHECK(cluster_check(ws, ms4, 3, 80) && std::strstr(cluster_check(ws, ms4, 3, 80), "1..SR_CLUSTER_MAX"));
        const uint32_t big[] = {0, 819, 1639}, one[] = {0, 1, 2};  // 819 x 80 = 65 520 passes, 820 x 80 does not
        CHECK(cluster_check(big, one, 1, 80) == nullptr);
        CHECK(cluster_check(big, one, 2, 80) && std::strstr(cluster_check(big, one, 2, 80), "exact"));
        const uint32_t top[] = {0, 0xFFFFFFFFu};  // no overflow in the bound
        CHECK(cluster_check(top, one, 1, 1024) && std::strstr(cluster_check(top, one, 1, 1024), "exact"));
    }
    // plans over random corpora and budgets, 0 and more than the cap included
    uint64_t seed = 2024;
    for (int round = 0; round < 400; round++) {
        const uint32_t W = 1 + rnd(seed) % 6;
        std::vector<uint32_t> ws(1, 0), ms(1, 0);
        for (uint32_t w = 0; w < W; w++) {
            const uint32_t kind = rnd(seed) % 4;
            ws.push_back(ws.back() + (kind == 0 ? 0 : kind == 1 ? 1 + rnd(seed) % 5 : rnd(seed) % 40));
            ms.push_back(ms.back() + (rnd(seed) % 3 == 0 ? kClusterMax : 1 + rnd(seed) % kClusterMax));
        }
        CHECK(cluster_check(ws.data(), ms.data(), W, 80) == nullptr);
        const uint32_t budgets[] = {0, 1, 2, 3, 4, 5, 7, 1 + rnd(seed) % 64, 1000, kClusterMaxPairs, 0xFFFFFFFFu};
        for (uint32_t b : budgets)
            if (check_plan(ws, ms, b)) {
                std::printf("plan_check: round %d, budget %u\n", round, b);
                return 1;
            }
    }
    std::printf("plan_check ok\n");
    return 0;
}
