// The host-only planning of the transcript-forced alignment and of the span gather (csrc/sr_forced_plan.h) on the CPU, without
// a device: the store under the word map, the checks on transcript / n_words / dst_of_span, minlen and tail, the per-level item
// lists and the launch groups, over random stores and corpora against a brute-force restatement -- the items of (group, level)
// are exactly the (row, valid slot of the row's word at that position) pairs, in ascending order and contiguous in the list;
// tail is the sum of the minimum reaches of the words still to come; the groups partition the rows.  A stand-alone program for
// the sanitizers:
//   hipcc --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I<csrc> plan_check.cpp -o plan_check && ./plan_check
// (tests/test_forced_ref.py builds and runs it).  Prints "plan_check ok" and returns 0, or says what failed and returns 1.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <utility>

#include "sr_forced_plan.h"

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

struct Corpus {
    std::vector<uint32_t> label, len;  // the store
    uint32_t W = 1;
    std::vector<uint32_t> t, n;        // transcript[n_rows][W], n_words[n_rows]
};

// brute force, from the definitions
static std::vector<uint32_t> slots_of(const Corpus &c, uint32_t lab)
{
    std::vector<uint32_t> out;
    for (uint32_t k = 0; k < c.label.size(); k++)
        if (c.label[k] == lab && c.len[k]) out.push_back(k);
    return out;
}
static uint32_t minlen_of(const Corpus &c, uint32_t lab)
{
    uint32_t m = 0;
    for (uint32_t k : slots_of(c, lab)) m = !m || c.len[k] / 2 + 1 < m ? c.len[k] / 2 + 1 : m;
    return m;
}

static int check_store(const Corpus &c, const ForcedStore &s)
{
    std::vector<uint32_t> first;  // labels in the order of their first slot
    for (uint32_t lab : c.label)
        if (std::find(first.begin(), first.end(), lab) == first.end()) first.push_back(lab);
    CHECK(s.index.size() == first.size() && s.start.size() == first.size() + 1 && s.minlen.size() == first.size() && s.start[0] == 0);
    for (uint32_t w = 0; w < first.size(); w++) {
        CHECK(s.index.count(first[w]) && s.index.at(first[w]) == w);
        const std::vector<uint32_t> want = slots_of(c, first[w]);
        CHECK(s.start[w + 1] - s.start[w] == want.size() && s.start[w + 1] <= s.slots.size());
        CHECK(std::equal(want.begin(), want.end(), s.slots.begin() + s.start[w]));
        CHECK(s.minlen[w] == minlen_of(c, first[w]) && (s.minlen[w] == 0) == want.empty());
    }
    CHECK(s.start.back() == s.slots.size());
    return 0;
}

static int check_plan(const Corpus &c, const ForcedStore &s, uint32_t per, bool prune)
{
    const uint32_t R = (uint32_t)c.n.size(), W = c.W;
    const ForcedPlan p = forced_plan(s, c.t.data(), c.n.data(), R, W, per, prune);
    if (!per) per = 1;
    CHECK(p.n_rows == R && p.W == W && p.count_at() == (size_t)R * W && p.items_at() == (size_t)R * W + R);
    CHECK(p.tab.size() == p.items_at() + (size_t)2 * p.n_items);
    for (uint32_t r = 0; r < R; r++) {
        CHECK(p.tab[p.count_at() + r] == c.n[r]);
        for (uint32_t l = 1; l <= W; l++) {
            uint32_t tail = 0;
            for (uint32_t i = l; i < c.n[r]; i++) tail += minlen_of(c, c.t[(size_t)r * W + i]);
            CHECK(p.tab[(size_t)r * W + l - 1] == (prune && l <= c.n[r] ? tail : 0u));
        }
    }
    // the groups: a partition of the rows into runs of `per`, the last one shorter
    CHECK(p.groups.size() == (R + per - 1) / per);
    uint32_t next_row = 0, next_item = 0;
    for (const ForcedGroup &g : p.groups) {
        CHECK(g.row0 == next_row && g.n_rows >= 1 && g.n_rows <= per && g.row0 + g.n_rows <= R);
        CHECK(g.n_rows == per || g.row0 + g.n_rows == R);
        next_row += g.n_rows;
        uint32_t levels = 0;
        for (uint32_t r = g.row0; r < g.row0 + g.n_rows; r++) levels = std::max(levels, c.n[r]);
        CHECK(g.levels == levels && levels <= W);
        for (uint32_t l = 1; l <= kForcedMaxWords; l++) {
            CHECK(g.item0[l - 1] == next_item && g.item0[l] >= g.item0[l - 1] && g.item0[l] <= p.n_items);
            std::vector<std::pair<uint32_t, uint32_t>> want;
            if (l <= levels)
                for (uint32_t r = g.row0; r < g.row0 + g.n_rows; r++)
                    if (c.n[r] >= l)
                        for (uint32_t k : slots_of(c, c.t[(size_t)r * W + l - 1])) want.push_back({r, k});
            CHECK(g.item0[l] - g.item0[l - 1] == want.size());
            for (size_t i = 0; i < want.size(); i++) {
                const uint32_t *it = p.tab.data() + p.items_at() + 2 * ((size_t)g.item0[l - 1] + i);
                CHECK(it[0] == want[i].first && it[1] == want[i].second);
                CHECK(it[0] >= g.row0 && it[0] - g.row0 < g.n_rows && it[1] < c.label.size() && c.len[it[1]] > 0);
            }
            next_item = g.item0[l];
        }
    }
    CHECK(next_row == R && next_item == p.n_items);
    return 0;
}

int main()
{
    std::string why;
    // the checks
    {
        const uint32_t label[] = {7, 7, 3, 9, 3}, len[] = {5, 0, 1, 0, 8};
        const ForcedStore s = forced_store(label, len, 5);
        CHECK(s.minlen[s.index.at(7)] == 3 && s.minlen[s.index.at(3)] == 1 && s.minlen[s.index.at(9)] == 0);
        const uint32_t t[] = {7, 3, 9, 3, 3, 3}, n[] = {3, 0};
        CHECK(forced_check(s, t, n, 2, 3, &why));
        CHECK(!forced_check(s, t, n, 2, 0, &why) && why.find("1..16") != std::string::npos);
        CHECK(!forced_check(s, t, n, 2, 17, &why) && why.find("1..16") != std::string::npos);
        CHECK(!forced_check(s, nullptr, n, 2, 3, &why) && !forced_check(s, t, nullptr, 2, 3, &why));
        CHECK(forced_check(s, nullptr, nullptr, 0, 3, &why));
        const uint32_t n_long[] = {3, 4};
        CHECK(!forced_check(s, t, n_long, 2, 3, &why) && why.find("row 1 has 4 words") != std::string::npos);
        const uint32_t t_bad[] = {7, 3, 9, 3, 4, 3}, n_two[] = {3, 2};
        CHECK(!forced_check(s, t_bad, n_two, 2, 3, &why) && why.find("row 1, position 1") != std::string::npos && why.find("label 4") != std::string::npos);
        const uint32_t n_one[] = {3, 1};  // ... a label behind the row's count is not read
        CHECK(forced_check(s, t_bad, n_one, 2, 3, &why));
        // a word without a valid slot has no items and adds nothing to a tail
        const ForcedPlan p = forced_plan(s, t, n, 2, 3, 5, true);
        CHECK(p.n_items == 3 && p.tab[0] == 1 && p.tab[1] == 0 && p.tab[2] == 0 && p.groups.size() == 1 && p.groups[0].levels == 3);
        CHECK(p.groups[0].item0[0] == 0 && p.groups[0].item0[1] == 1 && p.groups[0].item0[2] == 3 && p.groups[0].item0[3] == 3);
        char buf[64];
        CHECK(forced_overlap(buf, 16, buf + 15, 4) && !forced_overlap(buf, 16, buf + 16, 4) && !forced_overlap(buf, 0, buf, 4) &&
              !forced_overlap(nullptr, 16, buf, 4));
    }
    // the one overlap test of every stage's buffer checks (csrc/sr_overlap.h)
    {
        char buf[64];
        CHECK(!overlap(nullptr, 8, nullptr, 8) && !overlap(buf, 8, nullptr, 8) && !overlap(nullptr, 8, buf, 8));  // null: never
        CHECK(!overlap(buf, 0, buf, 8) && !overlap(buf, 8, buf, 0) && !overlap(buf + 4, 0, buf, 8) && !overlap(buf, 0, buf, 0));  // empty: never
        CHECK(!overlap(buf, 8, buf + 8, 8) && !overlap(buf + 8, 8, buf, 8));  // touching ranges share no byte ...
        CHECK(overlap(buf, 9, buf + 8, 8) && overlap(buf + 8, 8, buf, 9));    // ... one byte more and they do, either way round
        CHECK(overlap(buf, 8, buf, 8) && overlap(buf, 1, buf, 1));            // the same range
        CHECK(overlap(buf, 32, buf + 8, 4) && overlap(buf + 8, 4, buf, 32));  // nested, either way round
        CHECK(overlap(buf, 32, buf + 31, 1) && overlap(buf, 32, buf, 1) && !overlap(buf, 32, buf + 32, 1));  // the first and last byte; one past
        CHECK(!overlap(buf, 4, buf + 40, 4) && !overlap(buf + 40, 4, buf, 4));  // far apart
    }
    // the gather's table
    {
        std::vector<uint32_t> src;
        const uint32_t dst[] = {2, kForcedNone, 0, 3}, dup[] = {2, 0, 2, 1}, big[] = {0, 4, 1, 2};
        CHECK(forced_gather_table(dst, 4, 5, &src, &why) && src.size() == 5);
        CHECK(src[0] == 2 && src[1] == kForcedNone && src[2] == 0 && src[3] == 3 && src[4] == kForcedNone);
        CHECK(!forced_gather_table(dup, 4, 5, &src, &why) && why.find("same example 2") != std::string::npos);
        CHECK(!forced_gather_table(big, 4, 4, &src, &why) && why.find("not below n_ex") != std::string::npos);
        CHECK(forced_gather_table(dst, 0, 0, &src, &why) && src.empty());
    }
    // stores, corpora and plans at random
    uint64_t seed = 2025;
    for (int round = 0; round < 300; round++) {
        Corpus c;
        const uint32_t K = 1 + rnd(seed) % 24, n_lab = 1 + rnd(seed) % 6;
        for (uint32_t k = 0; k < K; k++) {
            c.label.push_back(100 + 7 * (rnd(seed) % n_lab));
            c.len.push_back(rnd(seed) % 4 == 0 ? 0 : 1 + rnd(seed) % 40);
        }
        const ForcedStore s = forced_store(c.label.data(), c.len.data(), K);
        if (check_store(c, s)) return 1;
        c.W = 1 + rnd(seed) % kForcedMaxWords;
        const uint32_t R = rnd(seed) % 20;
        for (uint32_t r = 0; r < R; r++) {
            c.n.push_back(rnd(seed) % 3 == 0 ? rnd(seed) % 2 * c.W : rnd(seed) % (c.W + 1));
            for (uint32_t i = 0; i < c.W; i++) c.t.push_back(i < c.n.back() ? c.label[rnd(seed) % K] : 0xDEAD0000u + i);
        }
        c.t.push_back(0);  // (data() of an empty vector may be null; the checks want an array)
        c.n.push_back(0);
        c.n.pop_back();
        CHECK(forced_check(s, c.t.data(), c.n.data(), R, c.W, &why));
        if (R) {  // one bad entry is found and named
            Corpus bad = c;
            const uint32_t r = rnd(seed) % R;
            if (bad.n[r]) {
                const uint32_t i = rnd(seed) % bad.n[r];
                bad.t[(size_t)r * c.W + i] = 99;
                CHECK(!forced_check(s, bad.t.data(), bad.n.data(), R, c.W, &why));
                CHECK(why.find("row " + std::to_string(r) + ", position " + std::to_string(i) + ":") == 0);
            }
            bad = c;
            bad.n[r] = c.W + 1 + rnd(seed) % 3;
            CHECK(!forced_check(s, bad.t.data(), bad.n.data(), R, c.W, &why) && why.find("row " + std::to_string(r) + " has") == 0);
        }
        const uint32_t pers[] = {0, 1, 2, 3, 1 + rnd(seed) % 8, R ? R : 1, R + 5, 65535};
        for (uint32_t per : pers)
            for (int prune = 0; prune < 2; prune++)
                if (check_plan(c, s, per, prune != 0)) {
                    std::printf("plan_check: round %d, rows per group %u, prune %d\n", round, per, prune);
                    return 1;
                }
        // the gather's table against its definition
        const uint32_t n_spans = R * c.W, n_ex = rnd(seed) % (n_spans + 3);
        std::vector<uint32_t> dst(n_spans + 1, kForcedNone), src;
        std::vector<uint32_t> perm(n_ex);
        for (uint32_t e = 0; e < n_ex; e++) perm[e] = e;
        for (uint32_t e = n_ex; e > 1; e--) std::swap(perm[e - 1], perm[rnd(seed) % e]);
        uint32_t used = 0;
        for (uint32_t i = 0; i < n_spans && used < n_ex; i++)
            if (rnd(seed) % 3) dst[i] = perm[used++];
        CHECK(forced_gather_table(dst.data(), n_spans, n_ex, &src, &why) && src.size() == n_ex);
        for (uint32_t e = 0; e < n_ex; e++) {
            uint32_t named = 0, by = kForcedNone;
            for (uint32_t i = 0; i < n_spans; i++)
                if (dst[i] == e) named++, by = i;
            CHECK(named <= 1 && src[e] == by);
        }
        if (used >= 2) {  // a destination named twice, one out of range
            std::vector<uint32_t> d2 = dst;
            uint32_t a = kForcedNone, b = kForcedNone;
            for (uint32_t i = 0; i < n_spans; i++)
                if (d2[i] != kForcedNone) (a == kForcedNone ? a : b) = i;
            d2[b] = d2[a];
            CHECK(!forced_gather_table(d2.data(), n_spans, n_ex, &src, &why));
            d2 = dst;
            d2[a] = n_ex + rnd(seed) % 3;
            CHECK(!forced_gather_table(d2.data(), n_spans, n_ex, &src, &why));
        }
    }
    std::printf("plan_check ok\n");
    return 0;
}
