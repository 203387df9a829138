// The host side of a commit call of a live one-pass grammar session (csrc/sr_onepass_gram_commit_plan.h) on the CPU, without a
// device, against a brute-force restatement: the window from the kept items' slots, the rows of a list under the grammar
// sessions' binding -- a stale grammar refuses before the list is looked at, a refused or accepted list changes nothing -- and
// the kernel's block and ring.  A stand-alone program for the sanitizers:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I<csrc> plan_check.cpp -o plan_check && ./plan_check
// (tests/test_onepass_gram_commit_ref.py builds and runs it).  Prints "plan_check ok" and returns 0, or says what failed and
// returns 1.
#include <cstdio>
#include <cstdlib>

#include "sr_onepass_gram_commit_plan.h"

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

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

static int windows()
{
    uint64_t seed = 3;
    for (int it = 0; it < 2000; it++) {
        const uint32_t K = 1 + rnd(seed) % 12, n = rnd(seed) % 20;
        std::vector<uint32_t> len(K), slot(n);
        for (uint32_t &m : len) m = rnd(seed) % 4 ? 1 + rnd(seed) % 300 : 0u;  // 0: an invalid slot
        for (uint32_t &k : slot) k = rnd(seed) % K;
        uint32_t want = 0;  // the longest span any kept item's template can cover
        for (uint32_t k : slot)
            if (len[k] && 2 * len[k] - 1 > want) want = 2 * len[k] - 1;
        CHECK(onepass_gram_commit_window(slot.data(), n, len.data(), K) == want);
    }
    const uint32_t len[4] = {8, 0, 200, 14}, all[4] = {0, 1, 2, 3}, some[2] = {3, 0}, out[2] = {9, 3}, cap[1] = {16383}, zero[1] = {0};
    CHECK(onepass_gram_commit_window(all, 4, len, 4) == 399 && onepass_gram_commit_window(some, 2, len, 4) == 27);
    CHECK(onepass_gram_commit_window(all + 1, 1, len, 4) == 0 && onepass_gram_commit_window(nullptr, 0, len, 4) == 0);
    CHECK(onepass_gram_commit_window(out, 2, len, 4) == 27);  // a slot past the store counts as invalid
    CHECK(onepass_gram_commit_window(zero, 1, cap, 1) == 32765);
    // the same store, the grammar of every slot: the window of the session without a grammar
    CHECK(onepass_gram_commit_window(all, 4, len, 4) == onepass_commit_window(len, 4));
    return 0;
}

// random sessions under the constant binding: pushes, ends, and lists with repeats and strangers, fresh and stale
static int lists()
{
    uint64_t seed = 17;
    for (uint32_t C : {1u, 3u, 8u, 33u}) {
        OnePassLiveMirror m;
        m.open(C, kGramLiveBound);
        m.d.chunk_max = 40;
        m.d.utt_frames = 500;
        std::vector<uint32_t> frames(C, 0);
        for (int it = 0; it < 600; it++) {
            const uint32_t what = rnd(seed) % 6;
            if (what == 0) {  // some channels end
                std::vector<uint32_t> list;
                for (uint32_t c = 0; c < C; c++)
                    if (rnd(seed) % 3 == 0) list.push_back(c);
                std::vector<SpotLiveChan> chan;
                std::vector<sr_chain_live_row> order;
                std::string why;
                CHECK(onepass_live_end_list(m, kGramLiveBound, list.data(), (uint32_t)list.size(), &chan, &order, &why));
                onepass_live_reset(m, kGramLiveBound, order);
                for (uint32_t c : list) frames[c] = 0;
            } else if (what < 4) {  // a push
                std::vector<uint32_t> n(C);
                for (uint32_t c = 0; c < C; c++) n[c] = frames[c] + 40 <= 500 && rnd(seed) % 2 ? rnd(seed) % 41 : 0u;
                OnePassLivePlan pl;
                std::string why;
                CHECK(onepass_live_plan(m, kGramLiveBound, 5, 0, 0, n.data(), 0, &pl, &why));
                std::vector<sr_chain_live_row> out(C);
                onepass_live_advance(m, pl, out.data(), nullptr);
                for (uint32_t c = 0; c < C; c++) frames[c] += n[c];
            }
            const uint32_t n_ch = rnd(seed) % (2 * C + 1);
            std::vector<uint32_t> list(n_ch);
            for (uint32_t &c : list) c = rnd(seed) % 16 ? rnd(seed) % C : C + rnd(seed) % 3;
            const bool stale = rnd(seed) % 5 == 0;
            const OnePassLiveMirror before = m;
            std::vector<sr_chain_live_row> order(3, sr_chain_live_row{7, 7});
            std::string why;
            const bool ok = onepass_gram_commit_list(m, stale, "the grammar is stale", list.data(), n_ch, &order, &why);
            CHECK(m.d.frames == before.d.frames && m.d.bound == before.d.bound && m.c0_prev == before.c0_prev && m.d.kept == before.d.kept);
            if (stale) {  // first, whatever the list holds
                CHECK(!ok && why == "the grammar is stale" && order.empty());
                continue;
            }
            bool want_ok = true;
            for (uint32_t i = 0; i < n_ch && want_ok; i++)
                if (list[i] >= C) {
                    want_ok = false;
                    CHECK(!ok && has(why, "past the session's last") && has(why, ("channel " + std::to_string(list[i]) + " ").c_str()));
                }
            CHECK(ok == want_ok);
            if (!ok) continue;
            std::vector<sr_chain_live_row> want;
            for (uint32_t i = 0; i < n_ch; i++) {
                bool seen = false;
                for (uint32_t j = 0; j < i; j++) seen = seen || list[j] == list[i];
                if (!seen) want.push_back(sr_chain_live_row{list[i], frames[list[i]]});
            }
            CHECK(order.size() == want.size() && order.size() <= C);
            for (size_t r = 0; r < want.size(); r++) CHECK(order[r].channel == want[r].channel && order[r].frames == want[r].frames);
        }
    }
    // no list at all: no row, no pointer read; a stale grammar refuses even that
    OnePassLiveMirror m;
    m.open(2, kGramLiveBound);
    std::vector<sr_chain_live_row> order(1);
    std::string why;
    CHECK(onepass_gram_commit_list(m, false, "", nullptr, 0, &order, &why) && order.empty());
    CHECK(!onepass_gram_commit_list(m, true, "stale", nullptr, 0, &order, &why) && why == "stale");
    return 0;
}

// the kernel's block and ring: a block never passes a wave or the shortest word, and the ring is a power of two that holds a
// block and the W positions below it, within the 64 KiB a kernel gets without asking
static int rings()
{
    for (uint32_t L = 0; L <= 9000; L++) {
        const uint32_t b = onepass_gram_commit_block(L);
        CHECK(b >= 1 && b <= 64 && (L == 0 || b <= L) && (L < 1 || L > 64 || b == L));
    }
    for (uint32_t W = 0; W <= 32765; W += (W < 600 ? 1 : 97)) {
        const uint32_t r = onepass_gram_commit_ring(W);
        CHECK((r & (r - 1)) == 0 && r >= W + 64 && r >= 64 && (r == 64 || r / 2 < W + 64));
        CHECK(W > 4000 || (size_t)r * 8 <= 64 * 1024);  // templates that fit the sweep's LDS image have at most 1 706 rows
    }
    CHECK(onepass_gram_commit_ring(0) == 64 && onepass_gram_commit_ring(17) == 128 && onepass_gram_commit_ring(239) == 512);
    return 0;
}

int main()
{
    if (windows() || lists() || rings()) return 1;
    std::printf("plan_check ok\n");
    return 0;
}
