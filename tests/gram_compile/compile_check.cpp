// The host-only compile step of a grammar (csrc/sr_gram_compile.h) on the CPU, without a device: the checks of
// sr_grammar_create_weighted on the network, the distinct charge lists, the items and the per-level lists, over random grammars
// of up to 64 states and 4096 arcs, against a brute-force restatement that shares no code with it.  A stand-alone program for
// the sanitizers:
//   hipcc --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I<csrc> compile_check.cpp -o compile_check && ./compile_check
// (tests/test_wgram_ref.py builds and runs it).  Prints "compile_check ok" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstdlib>

#include "sr_gram_compile.h"

using namespace sr;

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("compile_check: line %d: %s\n", __LINE__, #cond);     \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static uint32_t rnd(uint64_t &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
}

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

struct Case {
    uint32_t S = 0;
    std::vector<sr_gram_arc> arcs;
    std::vector<uint32_t> arc_cost, final_cost, label;
    std::vector<uint8_t> final_state, usable;
};

// a random network; costs 0: none, 1: a few small values (lists get shared), 2: anything up to the bound
static Case make(uint64_t &seed, uint32_t S, uint32_t n_arcs, uint32_t n_words, uint32_t K, int costs)
{
    Case c;
    c.S = S;
    c.label.resize(K);
    c.usable.resize(K);
    for (uint32_t k = 0; k < K; k++) {
        c.label[k] = (rnd(seed) % n_words) * 3 + 1;  // labels need not be dense
        c.usable[k] = rnd(seed) % 5 != 0;
    }
    std::set<std::tuple<uint32_t, uint32_t, uint32_t>> seen;
    for (uint32_t tries = 0; c.arcs.size() < n_arcs && tries < 8 * n_arcs + 64; tries++) {
        const uint32_t s = rnd(seed) % S, t = rnd(seed) % S, w = c.label[rnd(seed) % K];
        if (!seen.emplace(s, t, w).second) continue;
        c.arcs.push_back(sr_gram_arc{s, t, w, 0u});
        c.arc_cost.push_back(costs == 0 ? 0u : costs == 1 ? rnd(seed) % 3 : rnd(seed) % (kGramMaxCost + 1));
    }
    c.final_state.assign(S, 0);
    c.final_cost.assign(S, 0);
    c.final_state[rnd(seed) % S] = 1;
    for (uint32_t s = 0; s < S; s++) {
        if (rnd(seed) % 4 == 0) c.final_state[s] = 1 + rnd(seed) % 200;  // any nonzero byte flags a final state
        if (c.final_state[s] && costs) c.final_cost[s] = rnd(seed) % 2 ? kGramMaxCost : rnd(seed) % 1000;
    }
    return c;
}

// everything the compile step promises, restated with plain loops over the arcs
static int compare(const Case &c, bool null_costs)
{
    GramNet net;
    GramCompiled out;
    std::string why;
    CHECK(gram_check(c.S, c.arcs.data(), null_costs ? nullptr : c.arc_cost.data(), (uint32_t)c.arcs.size(), c.final_state.data(),
                     null_costs ? nullptr : c.final_cost.data(), c.label, &net, &why));
    CHECK(gram_build(net, c.arcs.data(), (uint32_t)c.arcs.size(), c.label, c.usable, &out, &why));
    const uint32_t n_arcs = (uint32_t)c.arcs.size(), S = c.S, K = (uint32_t)c.label.size();
    auto cost_of = [&](uint32_t i) { return null_costs ? 0u : c.arc_cost[i]; };

    bool any = false;
    for (uint32_t i = 0; i < n_arcs; i++) any = any || cost_of(i);
    for (uint32_t s = 0; s < S; s++) {
        any = any || (!null_costs && c.final_cost[s]);
        CHECK(net.final_cost[s] == (null_costs ? 0u : c.final_cost[s]) && (net.finals >> s & 1) == (c.final_state[s] != 0));
    }
    CHECK(net.weighted == any);

    // the charge list of every pair (t, w), brute force: the arcs by ascending source state
    std::map<std::pair<uint32_t, uint32_t>, std::vector<std::pair<uint32_t, uint32_t>>> all_lists;
    for (uint32_t s = 0; s < S; s++)
        for (uint32_t i = 0; i < n_arcs; i++)
            if (c.arcs[i].from == s) all_lists[{c.arcs[i].to, c.arcs[i].word}].push_back({s, cost_of(i)});
    auto list_of = [&](uint32_t t, uint32_t w) {
        const auto it = all_lists.find({t, w});
        return it == all_lists.end() ? std::vector<std::pair<uint32_t, uint32_t>>{} : it->second;
    };
    auto compiled_list = [&](uint32_t set) {
        std::vector<std::pair<uint32_t, uint32_t>> l;
        uint32_t j = out.cost_off[set];
        for (uint32_t s = 0; s < 64; s++)
            if (out.masks[set] >> s & 1) l.push_back({s, out.costs[j++]});
        return j == out.cost_off[set + 1] ? l : std::vector<std::pair<uint32_t, uint32_t>>{{~0u, ~0u}};
    };
    const uint32_t n_sets = (uint32_t)out.masks.size();
    CHECK(out.cost_off.size() == n_sets + 1 && out.cost_off[0] == 0 && out.cost_off[n_sets] == out.costs.size());
    std::set<std::vector<std::pair<uint32_t, uint32_t>>> distinct, pairs_lists;
    for (uint32_t i = 0; i < n_sets; i++) CHECK(distinct.insert(compiled_list(i)).second);  // no list twice
    for (uint32_t i = 0; i < n_arcs; i++) pairs_lists.insert(list_of(c.arcs[i].to, c.arcs[i].word));
    CHECK(distinct == pairs_lists);  // exactly the lists of the pairs that have an arc
    if (!any) {  // without costs a list is its set of states: as many lists as distinct from-sets
        std::set<unsigned long long> masks(out.masks.begin(), out.masks.end());
        CHECK(masks.size() == n_sets);
    }

    // the items: one per usable slot k and target t with an arc (., t, label[k]), ascending (slot, target), charged by that pair's list
    std::vector<GramItem> want;
    for (uint32_t k = 0; k < K; k++)
        for (uint32_t t = 0; t < S && c.usable[k]; t++)
            if (!list_of(t, c.label[k]).empty()) want.push_back(GramItem{k, t, 0u, 0u});
    CHECK(want.size() == out.items.size());
    for (size_t i = 0; i < want.size(); i++) {
        const GramItem &it = out.items[i];
        CHECK(it.slot == want[i].slot && it.target == want[i].target && it.reserved == 0 && it.set < n_sets);
        CHECK(compiled_list(it.set) == list_of(it.target, c.label[it.slot]));
    }

    // reach and distance by plain relaxation over booleans
    std::vector<std::vector<uint8_t>> reach(kChainMaxWords, std::vector<uint8_t>(S, 0));
    reach[0][0] = 1;
    for (uint32_t i = 1; i < kChainMaxWords; i++)
        for (uint32_t a = 0; a < n_arcs; a++)
            if (reach[i - 1][c.arcs[a].from]) reach[i][c.arcs[a].to] = 1;
    std::vector<uint32_t> dist(S, 1000);
    for (uint32_t s = 0; s < S; s++)
        if (c.final_state[s]) dist[s] = 0;
    for (bool moved = true; moved;) {
        moved = false;
        for (uint32_t a = 0; a < n_arcs; a++)
            if (dist[c.arcs[a].to] + 1 < dist[c.arcs[a].from]) dist[c.arcs[a].from] = dist[c.arcs[a].to] + 1, moved = true;
    }
    // what level l of a call with max_words keeps: the prefix of each list
    for (uint32_t W = 1; W <= kChainMaxWords; W++)
        for (uint32_t l = 1; l <= W; l++) {
            const GramLevelLists &v = out.lv[l - 1];
            const uint32_t j = W - l + 1;
            std::set<uint32_t> items, sets, states, got_items, got_sets, got_states;
            for (uint32_t i = 0; i < out.items.size(); i++) {
                const GramItem &it = out.items[i];
                bool meets = false;
                for (uint32_t st = 0; st < S; st++) meets = meets || (reach[l - 1][st] && (out.masks[it.set] >> st & 1));  // (the list was compared above)
                if (!meets || dist[it.target] > W - l) continue;
                items.insert(i);
                sets.insert(it.set);
                states.insert(it.target);
            }
            CHECK(v.items[j] <= out.lists.size() - v.item0 && v.sets[j] <= out.lists.size() - v.set0 && v.states[j] <= out.lists.size() - v.state0);
            for (uint32_t i = 0; i < v.items[j]; i++) CHECK(got_items.insert(out.lists[v.item0 + i]).second);
            for (uint32_t i = 0; i < v.sets[j]; i++) CHECK(got_sets.insert(out.lists[v.set0 + i]).second);
            for (uint32_t i = 0; i < v.states[j]; i++) CHECK(got_states.insert(out.lists[v.state0 + i]).second);
            CHECK(got_items == items && got_sets == sets && got_states == states);
        }
    return 0;
}

static int random_grammars()
{
    uint64_t seed = 5;
    for (int it = 0; it < 30; it++) {
        const uint32_t S = 1 + rnd(seed) % kGramMaxStates, n_words = 1 + rnd(seed) % 6, K = n_words + rnd(seed) % 12;
        const uint32_t n_arcs = 1 + rnd(seed) % (it % 3 ? 40 : 400);
        for (int costs = 0; costs < 3; costs++) {
            const Case c = make(seed, S, n_arcs, n_words, K, costs);
            if (compare(c, false)) return 1;
            if (costs == 0 && compare(c, true)) return 1;  // NULL arrays are all-zero arrays
        }
    }
    // the limits themselves: 64 states, 4096 arcs (every arc of one word), unweighted and at the cost bound
    for (int costs = 0; costs < 3; costs += 2) {
        Case c;
        c.S = kGramMaxStates;
        c.label = {7, 7, 9};
        c.usable = {1, 1, 1};
        for (uint32_t s = 0; s < 64; s++)
            for (uint32_t t = 0; t < 64; t++) {
                c.arcs.push_back(sr_gram_arc{s, t, 7u, 0u});
                c.arc_cost.push_back(costs ? (s * 64 + t) % 5 ? kGramMaxCost : 0u : 0u);
            }
        c.final_state.assign(64, 1);
        c.final_cost.assign(64, costs ? kGramMaxCost : 0u);
        CHECK(c.arcs.size() == kGramMaxArcs);
        if (compare(c, false)) return 1;
    }
    return 0;
}

// all-zero costs compile to exactly what NULL arrays compile to, and a cost makes equal from-sets distinct lists
static int zero_costs_and_sharing()
{
    uint64_t seed = 23;
    const Case c = make(seed, 9, 60, 4, 7, 0);
    GramNet n0, n1;
    GramCompiled a, b;
    std::string why;
    const uint32_t n_arcs = (uint32_t)c.arcs.size();
    CHECK(gram_check(c.S, c.arcs.data(), nullptr, n_arcs, c.final_state.data(), nullptr, c.label, &n0, &why));
    CHECK(gram_check(c.S, c.arcs.data(), c.arc_cost.data(), n_arcs, c.final_state.data(), c.final_cost.data(), c.label, &n1, &why));
    CHECK(!n0.weighted && !n1.weighted);
    CHECK(gram_build(n0, c.arcs.data(), n_arcs, c.label, c.usable, &a, &why) && gram_build(n1, c.arcs.data(), n_arcs, c.label, c.usable, &b, &why));
    CHECK(a.masks == b.masks && a.cost_off == b.cost_off && a.costs == b.costs && a.lists == b.lists && a.items.size() == b.items.size());
    for (size_t i = 0; i < a.items.size(); i++) CHECK(a.items[i].slot == b.items[i].slot && a.items[i].target == b.items[i].target && a.items[i].set == b.items[i].set);
    for (uint32_t l = 0; l < kChainMaxWords; l++)
        for (uint32_t j = 0; j <= kChainMaxWords; j++)
            CHECK(a.lv[l].items[j] == b.lv[l].items[j] && a.lv[l].sets[j] == b.lv[l].sets[j] && a.lv[l].states[j] == b.lv[l].states[j]);
    // two pairs with the from-set {0, 1}: one list without costs, two once one arc of the four costs something
    const sr_gram_arc arcs[4] = {{0, 2, 1, 0}, {1, 2, 1, 0}, {0, 3, 4, 0}, {1, 3, 4, 0}};
    const uint8_t fin[4] = {0, 0, 1, 1};
    const std::vector<uint32_t> label = {1, 4};
    const std::vector<uint8_t> usable = {1, 1};
    for (uint32_t extra = 0; extra < 2; extra++) {
        const uint32_t cost[4] = {5, 0, 5, extra};
        GramNet n;
        GramCompiled g;
        CHECK(gram_check(4, arcs, cost, 4, fin, nullptr, label, &n, &why) && n.weighted);
        CHECK(gram_build(n, arcs, 4, label, usable, &g, &why));
        CHECK(g.masks.size() == 1 + extra && g.masks[0] == 3 && g.costs[0] == 5 && g.costs[1] == 0 && g.items.size() == 2);
    }
    return 0;
}

static int refusals()
{
    const sr_gram_arc ok[2] = {{0, 1, 3, 0}, {1, 1, 5, 0}};
    const uint8_t fin[2] = {0, 1};
    const std::vector<uint32_t> label = {3, 5};
    auto refused = [&](uint32_t S, const sr_gram_arc *arcs, const uint32_t *ac, uint32_t n, const uint8_t *f, const uint32_t *fc, const char *what) {
        GramNet net;
        std::string why;
        return !gram_check(S, arcs, ac, n, f, fc, label, &net, &why) && has(why, what);
    };
    GramNet net;
    std::string why;
    const uint32_t at_bound[2] = {kGramMaxCost, kGramMaxCost}, fc_ok[2] = {0, kGramMaxCost};
    CHECK(gram_check(2, ok, at_bound, 2, fin, fc_ok, label, &net, &why) && net.weighted);  // the bound itself is accepted
    const uint32_t above[2] = {0, kGramMaxCost + 1}, fc_above[2] = {0, kGramMaxCost + 1}, fc_not_final[2] = {1, 0};
    CHECK(refused(2, ok, above, 2, fin, nullptr, "arc 1: cost above 2^24"));
    CHECK(refused(2, ok, nullptr, 2, fin, fc_above, "final cost above 2^24"));
    CHECK(refused(2, ok, nullptr, 2, fin, fc_not_final, "not final"));
    CHECK(refused(0, ok, nullptr, 2, fin, nullptr, "n_states") && refused(65, ok, nullptr, 2, fin, nullptr, "n_states"));
    CHECK(refused(2, ok, nullptr, 0, fin, nullptr, "n_arcs") && refused(2, ok, nullptr, 4097, fin, nullptr, "n_arcs"));
    const sr_gram_arc high[1] = {{0, 2, 3, 0}}, res[1] = {{0, 1, 3, 1}}, word[1] = {{0, 1, 4, 0}}, dup[2] = {{0, 1, 3, 0}, {0, 1, 3, 0}};
    CHECK(refused(2, high, nullptr, 1, fin, nullptr, "state index") && refused(2, res, nullptr, 1, fin, nullptr, "reserved"));
    CHECK(refused(2, word, nullptr, 1, fin, nullptr, "no label") && refused(2, dup, nullptr, 2, fin, nullptr, "duplicate"));
    const uint8_t none[2] = {0, 0};
    CHECK(refused(2, ok, nullptr, 2, none, nullptr, "no final state"));
    return 0;
}

int main()
{
    if (refusals() || zero_costs_and_sharing() || random_grammars()) return 1;
    std::printf("compile_check ok\n");
    return 0;
}
