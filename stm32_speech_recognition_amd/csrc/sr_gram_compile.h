// The compile step of a grammar (include/sr_engine.h, "grammar-constrained decoding" and "weighted grammars"): the checks of
// sr_grammar_create[_weighted] on the network itself, the distinct charge lists, the items and, per level 1..16, the lists a
// call keeps.  A CHARGE LIST is what a word pass is charged from: the ascending-by-state list of (source state s, arc cost c)
// of one pair (target t, word w).  With every cost zero a list is its set of states, the from-set, and the lists, their order
// and every count are what the unweighted grammar has always had; the masks are kept for both.
// HOST ONLY, and free of HIP calls: tests/gram_compile/compile_check.cpp runs it on the CPU under the sanitizers.
#pragma once
#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <unordered_set>
#include <vector>

#include "sr_dtw_plan.h"

namespace sr {

constexpr uint32_t kGramMaxStates = 64, kGramMaxArcs = 4096, kGramMaxItems = 1u << 20;
constexpr uint32_t kGramMaxCost = 1u << 24;  // of an arc and of a final state: keeps every cost below 2^32 (the header has the sum)
constexpr uint32_t kGramFar = 0xFFFFFFFFu;   // a state from which no final state is reachable

// Level l keeps the items whose charge list meets the states reachable from state 0 in exactly l - 1 arcs; its lists are
// sorted by the distance (in arcs) from the target to a final state, so that what a call with max_words keeps -- distance <=
// max_words - l -- is a PREFIX of each list, and a call only counts.
struct GramLevelLists {
    uint32_t item0 = 0, set0 = 0, state0 = 0;                                  // where the level's lists start in `lists`
    uint32_t items[kChainMaxWords + 1] = {}, sets[kChainMaxWords + 1] = {}, states[kChainMaxWords + 1] = {};  // [j]: entries of distance < j
};

// the checked network: per pair (t, w), in the order (t, w), its charge list
struct GramNet {
    uint32_t n_states = 0;
    uint64_t finals = 0;
    bool weighted = false;  // some arc or final cost is nonzero
    std::map<std::pair<uint32_t, uint32_t>, std::vector<std::pair<uint32_t, uint32_t>>> from;  // (t, w) -> (s, c), ascending s
    std::vector<uint32_t> final_cost;  // [n_states]
};

struct GramCompiled {
    std::vector<unsigned long long> masks;  // [n_sets]: the states of each charge list
    std::vector<uint32_t> cost_off;         // [n_sets + 1]: list i's costs are costs[cost_off[i] .. cost_off[i + 1]), by ascending state
    std::vector<uint32_t> costs;
    std::vector<GramItem> items;            // ascending (slot, target); .set = the charge list
    std::vector<uint32_t> lists;            // level by level: item indices, charge lists, target states
    GramLevelLists lv[kChainMaxWords];
};

// The checks that need no device, in sr_grammar_create's order.  arc_cost / final_cost may be null: all 0.
inline bool gram_check(uint32_t n_states, const sr_gram_arc *arcs, const uint32_t *arc_cost, uint32_t n_arcs, const uint8_t *final_state,
                       const uint32_t *final_cost, const std::vector<uint32_t> &label, GramNet *net, std::string *why)
{
    if (n_states < 1 || n_states > kGramMaxStates) return *why = "n_states must be 1..64", false;
    if (n_arcs < 1 || n_arcs > kGramMaxArcs) return *why = "n_arcs must be 1..4096", false;
    const std::unordered_set<uint32_t> known(label.begin(), label.end());
    std::set<std::tuple<uint32_t, uint32_t, uint32_t>> seen;
    net->n_states = n_states;
    for (uint32_t i = 0; i < n_arcs; i++) {
        const sr_gram_arc &a = arcs[i];
        const std::string at = "arc " + std::to_string(i);
        if (a.from >= n_states || a.to >= n_states) return *why = at + ": state index at or above n_states", false;
        if (a.reserved) return *why = at + ": reserved must be 0", false;
        if (!known.count(a.word)) return *why = at + ": word " + std::to_string(a.word) + " is no label of the word map", false;
        if (!seen.emplace(a.from, a.to, a.word).second) return *why = at + ": duplicate arc", false;
        const uint32_t c = arc_cost ? arc_cost[i] : 0u;
        if (c > kGramMaxCost) return *why = at + ": cost above 2^24", false;
        net->weighted = net->weighted || c;
        net->from[{a.to, a.word}].push_back({a.from, c});
    }
    for (auto &f : net->from) std::sort(f.second.begin(), f.second.end());  // the arcs are distinct: one entry per state
    net->final_cost.assign(n_states, 0u);
    for (uint32_t s = 0; s < n_states; s++) {
        const uint32_t c = final_cost ? final_cost[s] : 0u;
        if (final_state[s]) net->finals |= 1ull << s;
        else if (c) return *why = "state " + std::to_string(s) + ": a final cost on a state that is not final", false;
        if (c > kGramMaxCost) return *why = "state " + std::to_string(s) + ": final cost above 2^24", false;
        net->weighted = net->weighted || c;
        net->final_cost[s] = c;
    }
    if (!net->finals) return *why = "no final state", false;
    return true;
}

// The lists, the items and the levels.  label[k]: the word of slot k; usable[k]: the slot is valid and holds frames.
inline bool gram_build(const GramNet &net, const sr_gram_arc *arcs, uint32_t n_arcs, const std::vector<uint32_t> &label,
                       const std::vector<uint8_t> &usable, GramCompiled *out, std::string *why)
{
    const uint32_t S = net.n_states;
    std::map<uint32_t, std::vector<uint32_t>> slots;
    for (uint32_t k = 0; k < label.size(); k++)
        if (usable[k]) slots[label[k]].push_back(k);

    // the distinct charge lists in the order of their first pair (t, w), and the items by ascending (slot, target)
    std::map<std::vector<std::pair<uint32_t, uint32_t>>, uint32_t> set_of;
    out->cost_off.assign(1, 0u);
    for (const auto &f : net.from) {
        const auto it = set_of.emplace(f.second, (uint32_t)out->masks.size());
        if (it.second) {
            unsigned long long m = 0;
            for (const auto &sc : f.second) {
                m |= 1ull << sc.first;
                out->costs.push_back(sc.second);
            }
            out->masks.push_back(m);
            out->cost_off.push_back((uint32_t)out->costs.size());
        }
        const auto sl = slots.find(f.first.second);
        if (sl == slots.end()) continue;  // every slot of the word is invalid: it contributes nothing
        for (uint32_t k : sl->second) out->items.push_back(GramItem{k, f.first.first, it.first->second, 0u});
    }
    if (out->items.size() > kGramMaxItems) return *why = "the grammar compiles to more than 2^20 (slot, state) items", false;
    std::sort(out->items.begin(), out->items.end(),
              [](const GramItem &a, const GramItem &b) { return a.slot != b.slot ? a.slot < b.slot : a.target < b.target; });

    // reach[i]: the states reachable from state 0 in exactly i arcs; dist[s]: the fewest arcs from s to a final state
    uint64_t reach[kChainMaxWords] = {1ull};
    for (uint32_t i = 1; i < kChainMaxWords; i++)
        for (uint32_t a = 0; a < n_arcs; a++)
            if (reach[i - 1] >> arcs[a].from & 1) reach[i] |= 1ull << arcs[a].to;
    std::vector<uint32_t> dist(S, kGramFar);
    for (uint32_t s = 0; s < S; s++)
        if (net.finals >> s & 1) dist[s] = 0;
    for (uint32_t round = 1; round < S; round++)
        for (uint32_t a = 0; a < n_arcs; a++)
            if (dist[arcs[a].to] != kGramFar && dist[arcs[a].to] + 1 < dist[arcs[a].from]) dist[arcs[a].from] = dist[arcs[a].to] + 1;

    std::vector<uint32_t> &lists = out->lists;
    for (uint32_t l = 1; l <= kChainMaxWords; l++) {
        GramLevelLists &v = out->lv[l - 1];
        // (distance, index) of the level's items, of the charge lists they use (by their nearest item) and of their targets
        std::vector<std::pair<uint32_t, uint32_t>> li;
        std::map<uint32_t, uint32_t> ls, lt;
        for (uint32_t i = 0; i < out->items.size(); i++) {
            const GramItem &it = out->items[i];
            const uint32_t d = dist[it.target];
            if (!(out->masks[it.set] & reach[l - 1]) || d > kChainMaxWords - l) continue;
            li.push_back({d, i});
            auto s = ls.emplace(it.set, d);
            if (!s.second && d < s.first->second) s.first->second = d;
            lt.emplace(it.target, d);
        }
        auto emit = [&lists](std::vector<std::pair<uint32_t, uint32_t>> e, uint32_t *start, uint32_t *below) {
            std::sort(e.begin(), e.end());
            *start = (uint32_t)lists.size();
            for (const auto &x : e) lists.push_back(x.second);
            for (uint32_t j = 0; j <= kChainMaxWords; j++)
                below[j] = (uint32_t)(std::lower_bound(e.begin(), e.end(), std::make_pair(j, 0u)) - e.begin());
        };
        std::vector<std::pair<uint32_t, uint32_t>> es, et;
        for (const auto &s : ls) es.push_back({s.second, s.first});
        for (const auto &t : lt) et.push_back({t.second, t.first});
        emit(li, &v.item0, v.items);
        emit(es, &v.set0, v.sets);
        emit(et, &v.state0, v.states);
    }
    return true;
}

}  // namespace sr
