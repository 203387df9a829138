// The host-only planning of one-pass grammar decoding (csrc/sr_onepass_gram_plan.h) on the CPU, without a device: which states
// can be reached from state 0 and which reach a final state, the kept items and states, the cost bound, the bytes of a row and
// the refusal of a row that exceeds a launch group, over random grammars, stores and hook values against a brute-force
// restatement -- reachability by walking every arc sequence breadth first (the plan closes a bit mask), a sum in u64 word by
// word for the bound.  A stand-alone program for the sanitizers:
//   hipcc --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I<csrc> plan_check.cpp -o plan_check && ./plan_check
// (tests/test_onepass_gram_ref.py builds and runs it).  Prints "plan_check ok" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <set>

#include "sr_onepass_gram_plan.h"

using namespace sr;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("plan_check: line %d: %s\n", __LINE__, #cond);     \
            return 1;                                                      \
        }                                                                  \
    } while (0)

struct Arc {
    uint32_t from, to, word, reserved;
};
struct Item {
    uint32_t slot, target, set, reserved;
};

static uint32_t rnd(uint64_t &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
}

// brute force: the states a walk of any length from `from` visits, one queue entry per newly seen state
static std::set<uint32_t> walk(const std::vector<Arc> &arcs, uint32_t from, bool backwards)
{
    std::set<uint32_t> seen{from};
    std::vector<uint32_t> todo{from};
    while (!todo.empty()) {
        const uint32_t at = todo.back();
        todo.pop_back();
        for (const Arc &a : arcs) {
            const uint32_t src = backwards ? a.to : a.from, dst = backwards ? a.from : a.to;
            if (src == at && seen.insert(dst).second) todo.push_back(dst);
        }
    }
    return seen;
}

static int check_grammar(uint32_t S, const std::vector<Arc> &arcs, uint64_t finals, const std::vector<Item> &items,
                         const std::vector<unsigned long long> &masks)
{
    const std::set<uint32_t> fwd = walk(arcs, 0, false);
    std::set<uint32_t> back;
    for (uint32_t f = 0; f < S; f++)
        if (finals >> f & 1)
            for (uint32_t s : walk(arcs, f, true)) back.insert(s);
    for (int prune = 1; prune >= 0; prune--) {
        const OnePassGramKeep k = onepass_gram_keep(S, arcs.data(), (uint32_t)arcs.size(), finals, items.data(), (uint32_t)items.size(), masks.data(),
                                                    prune != 0);
        for (uint32_t s = 0; s < S; s++) {
            CHECK((k.reach >> s & 1) == (uint64_t)fwd.count(s));
            CHECK((k.alive >> s & 1) == (uint64_t)back.count(s));
        }
        std::vector<uint32_t> want_items;
        std::set<uint32_t> want_states;
        for (uint32_t s = 0; s < S; s++)
            if (!prune || ((finals >> s & 1) && fwd.count(s))) want_states.insert(s);
        for (uint32_t i = 0; i < items.size(); i++) {
            bool named = false;
            for (uint32_t s = 0; s < S; s++) named = named || ((masks[items[i].set] >> s & 1) && fwd.count(s));
            if (prune && (!named || !back.count(items[i].target))) continue;
            want_items.push_back(i);
            for (uint32_t s = 0; s < S; s++)
                if (masks[items[i].set] >> s & 1) want_states.insert(s);
        }
        CHECK(k.items == want_items);
        CHECK(k.states == std::vector<uint32_t>(want_states.begin(), want_states.end()));
        if (!prune) CHECK(k.items.size() == items.size() && k.states.size() == S);
        // a kept item's target is charged from somewhere, and whoever is charged from is closed: every state of a kept list is
        // kept; a reachable final state is kept whether a word leaves it or not
        for (uint32_t i : k.items)
            for (uint32_t s = 0; s < S; s++)
                if (masks[items[i].set] >> s & 1) CHECK(want_states.count(s));
    }
    return 0;
}

static int check_plan(uint32_t tpl_len, uint32_t S, uint32_t kept_items, uint32_t kept_states, uint32_t max_frames, uint32_t frames_cap, uint32_t L,
                      uint32_t block, uint32_t rows)
{
    const OnePassGramPlan p = onepass_gram_plan(tpl_len, S, kept_items, kept_states, max_frames, frames_cap, L, block, rows);
    const OnePassPlan o = onepass_plan(tpl_len, 1u, max_frames, frames_cap, L, block, rows);
    CHECK(p.o.cap == o.cap && p.o.n == o.n && p.o.blocks.size() == o.blocks.size());  // the blocks are the one-pass decoder's
    for (size_t b = 0; b < o.blocks.size(); b++)
        CHECK(p.o.blocks[b].c0_prev == o.blocks[b].c0_prev && p.o.blocks[b].c0 == o.blocks[b].c0 && p.o.blocks[b].cN == o.blocks[b].cN);
    const size_t P = (size_t)max_frames + 1, row_bytes = (size_t)S * P * 12 + (size_t)kept_items * tpl_len * 16;
    CHECK(p.a_row == (size_t)S * P && p.e_row == p.a_row && p.col_row == (size_t)kept_items * tpl_len && p.row_bytes == row_bytes);
    CHECK(p.fits == (row_bytes <= kOnePassScratch));
    CHECK(p.rows >= 1 && p.rows <= kOnePassMaxRows);
    if (rows) {
        CHECK(p.rows == (rows < kOnePassMaxRows ? rows : kOnePassMaxRows));
    } else if (p.fits) {
        CHECK((size_t)p.rows * row_bytes <= kOnePassScratch);
        CHECK(p.rows == kOnePassMaxRows || (size_t)(p.rows + 1) * row_bytes > kOnePassScratch);
    }
    const uint32_t n_blocks = (uint32_t)o.blocks.size();
    CHECK(p.launches == (kept_items ? n_blocks : 0u) + (kept_states ? n_blocks + 1u : 0u) + 1u);
    if (kept_items && kept_states) CHECK(p.launches == 2 * n_blocks + 2);
    return 0;
}

int main()
{
    uint64_t s = 20261019;
    for (int it = 0; it < 3000; it++) {
        const uint32_t S = it % 50 == 0 ? 64u : 1 + rnd(s) % 12, n_words = 1 + rnd(s) % 6;
        const uint32_t n_arcs = 1 + rnd(s) % (3 * S);
        std::vector<Arc> arcs;
        std::set<std::pair<uint32_t, std::pair<uint32_t, uint32_t>>> seen;
        for (uint32_t a = 0; a < n_arcs; a++) {
            const Arc arc{rnd(s) % S, rnd(s) % S, rnd(s) % n_words, 0u};
            if (seen.insert({arc.from, {arc.to, arc.word}}).second) arcs.push_back(arc);
        }
        uint64_t finals = 0;
        for (uint32_t f = 0; f < S; f++)
            if (rnd(s) % 3 == 0) finals |= 1ull << f;
        if (!finals) finals = 1ull << (rnd(s) % S);
        // the charge lists per (target, word) and one or two slots per word, as the compile step lays them out
        std::vector<unsigned long long> masks;
        std::vector<Item> items;
        for (uint32_t t = 0; t < S; t++)
            for (uint32_t w = 0; w < n_words; w++) {
                unsigned long long m = 0;
                for (const Arc &a : arcs)
                    if (a.to == t && a.word == w) m |= 1ull << a.from;
                if (!m) continue;
                masks.push_back(m);
                for (uint32_t k = 0; k < 1 + w % 2; k++) items.push_back(Item{2 * w + k, t, (uint32_t)masks.size() - 1, 0u});
            }
        if (check_grammar(S, arcs, finals, items, masks)) {
            std::printf("plan_check: grammar %d failed\n", it);
            return 1;
        }
        const uint32_t tpl_len = 1 + rnd(s) % 200, max_frames = 2 + rnd(s) % (it % 16 ? 700 : 16382);
        const uint32_t frames_cap = rnd(s) % 3 == 0 ? 0u : 1 + rnd(s) % (max_frames + 50), L = rnd(s) % 8 == 0 ? 0u : 1 + rnd(s) % (tpl_len / 2 + 1);
        const uint32_t block = rnd(s) % 2 ? 0u : 1 + rnd(s) % 120, rows = rnd(s) % 3 ? 0u : 1 + rnd(s) % 70000;
        const uint32_t kept_items = rnd(s) % 10 == 0 ? 0u : (rnd(s) % 20 == 0 ? 1u << 20 : 1 + rnd(s) % 500);
        const uint32_t kept_states = rnd(s) % 10 == 0 ? 0u : 1 + rnd(s) % S;
        if (check_plan(tpl_len, S, kept_items, kept_states, max_frames, frames_cap, L, block, rows)) {
            std::printf("plan_check: plan %d failed\n", it);
            return 1;
        }
        // the cost bound in u64, word by word
        const uint32_t cap = frames_cap && frames_cap < max_frames ? frames_cap : max_frames;
        const uint32_t wc = rnd(s) % 4 ? rnd(s) % ((1u << 24) + 1) : 1u << 24, ac = rnd(s) % 4 ? rnd(s) % ((1u << 24) + 1) : 1u << 24;
        const uint32_t fc = rnd(s) % ((1u << 24) + 1);
        uint64_t sum = fc;
        for (uint32_t at = 0; L && at + L <= cap; at += L) sum += (uint64_t)wc + ac;
        if (onepass_gram_cost_ok(cap, L, wc, ac, fc) != (!L || sum <= (1ull << 30))) {
            std::printf("plan_check: cost bound %d failed\n", it);
            return 1;
        }
        if (onepass_gram_cost_ok(cap, L, wc, 0u, 0u) != onepass_cost_ok(cap, L, wc)) return 1;  // without costs: the one-pass bound
    }
    // refusals: 64 states over the longest rows fit, 2^20 items of long templates do not; a forced group size does not make them fit
    if (check_plan(1300, 64, 100, 64, 16383, 0, 40, 0, 0)) return 1;
    const OnePassGramPlan big = onepass_gram_plan(1300, 64, 1u << 20, 64, 16383, 0, 40, 0, 0);
    const OnePassGramPlan forced = onepass_gram_plan(1300, 64, 1u << 20, 64, 16383, 0, 40, 0, 7);
    if (big.fits || forced.fits || big.rows != 1 || forced.rows != 7 || big.row_bytes != (size_t)64 * 16384 * 12 + ((size_t)1300 << 20) * 16) {
        std::printf("plan_check: the refusal of a row over the group budget\n");
        return 1;
    }
    std::printf("plan_check ok\n");
    return 0;
}
