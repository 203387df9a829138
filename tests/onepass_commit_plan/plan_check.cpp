// The host side of a commit call of a live one-pass session (csrc/sr_onepass_live_plan.h: onepass_live_commit_list,
// onepass_commit_window) on the CPU, without a device, against a brute-force restatement: the rows of a list -- one per distinct
// channel at its first mention, with the frames the mirror holds -- the refusals and that a refused or accepted list changes
// nothing; the window as the longest span any valid template can cover, found by walking its step pattern.  A stand-alone
// program for the sanitizers:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I<csrc> plan_check.cpp -o plan_check && ./plan_check
// (tests/test_onepass_commit_ref.py builds and runs it).  Prints "plan_check ok" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstdlib>

#include "sr_onepass_live_plan.h"

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

// random sessions: pushes, ends, a store that changes, and lists with repeats, strangers and stale channels
static int lists()
{
    uint64_t seed = 11;
    for (uint32_t C : {1u, 3u, 8u, 33u}) {
        OnePassLiveMirror m;
        uint64_t serial = 5;
        m.open(C, serial);
        m.d.chunk_max = 40;
        m.d.utt_frames = 500;
        std::vector<uint32_t> frames(C, 0);
        std::vector<uint64_t> bound(C, serial);
        for (int it = 0; it < 800; it++) {
            const uint32_t what = rnd(seed) % 8;
            if (what == 0) {  // the store is replaced
                serial++;
            } else if (what == 1) {  // some channels end
                std::vector<uint32_t> list;
                for (uint32_t c = 0; c < C; c++)
                    if (rnd(seed) % 3 == 0) list.push_back(c);
                std::vector<SpotLiveChan> chan;
                std::vector<sr_chain_live_row> order;
                std::string why;
                CHECK(onepass_live_end_list(m, serial, list.data(), (uint32_t)list.size(), &chan, &order, &why));
                onepass_live_reset(m, serial, order);
                for (uint32_t c : list) {
                    frames[c] = 0;
                    bound[c] = serial;
                }
            } else if (what < 5) {  // a push
                std::vector<uint32_t> n(C);
                for (uint32_t c = 0; c < C; c++) n[c] = bound[c] == serial && frames[c] + 40 <= 500 && rnd(seed) % 2 ? rnd(seed) % 41 : 0u;
                OnePassLivePlan pl;
                std::string why;
                CHECK(onepass_live_plan(m, serial, 5, 0, 0, n.data(), 0, &pl, &why));
                std::vector<sr_chain_live_row> out(C);
                onepass_live_advance(m, pl, out.data(), nullptr);
                for (uint32_t c = 0; c < C; c++) frames[c] += n[c];
            }
            // a commit list
            const uint32_t n_ch = rnd(seed) % (2 * C + 1);
            std::vector<uint32_t> list(n_ch);
            for (uint32_t &c : list) c = rnd(seed) % 16 ? rnd(seed) % C : C + rnd(seed) % 3;
            const OnePassLiveMirror before = m;
            std::vector<sr_chain_live_row> order(3, sr_chain_live_row{7, 7});
            std::string why;
            const bool ok = onepass_live_commit_list(m, serial, list.data(), n_ch, &order, &why);
            CHECK(m.d.frames == before.d.frames && m.d.bound == before.d.bound && m.c0_prev == before.c0_prev && m.d.kept == before.d.kept);
            // the model: the first offender in list order decides; otherwise every channel at its first mention
            bool want_ok = true;
            for (uint32_t i = 0; i < n_ch && want_ok; i++) {
                if (list[i] >= C) {
                    want_ok = false;
                    CHECK(!ok && has(why, "past the session's last") && has(why, ("channel " + std::to_string(list[i]) + " ").c_str()));
                } else if (bound[list[i]] != serial) {
                    want_ok = false;
                    CHECK(!ok && has(why, "store changed") && has(why, ("channel " + std::to_string(list[i]) + " ").c_str()));
                }
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
    // no list at all: no row, no pointer read
    OnePassLiveMirror m;
    m.open(2, 1);
    std::vector<sr_chain_live_row> order(1);
    std::string why;
    CHECK(onepass_live_commit_list(m, 1, nullptr, 0, &order, &why) && order.empty());
    CHECK(!onepass_live_commit_list(m, 2, nullptr, 0, &order, &why) || order.empty());  // a replaced store refuses listed channels only
    return 0;
}

// the longest run of input frames a template of M frames can cover: cells (x, y) reached by the decoder's steps -- diagonal;
// one frame to the right or one row up, each only directly after a diagonal step -- from (0, 0) to row M - 1
static uint32_t longest_span(uint32_t M)
{
    const uint32_t X = 2 * M + 2;
    std::vector<uint8_t> diag((size_t)X * M, 0), any((size_t)X * M, 0);  // reached by a diagonal step / at all
    any[0] = 1;  // the start is of the non-diagonal kind: a diagonal step must follow it
    uint32_t best = 0;
    for (uint32_t x = 0; x < X; x++)
        for (uint32_t y = 0; y < M; y++) {
            uint8_t &d = diag[(size_t)x * M + y], &a = any[(size_t)x * M + y];
            if (x && y && any[(size_t)(x - 1) * M + y - 1]) d = a = 1;
            if (x && diag[(size_t)(x - 1) * M + y]) a = 1;
            if (y && diag[(size_t)x * M + y - 1]) a = 1;
            if (a && y == M - 1) best = x + 1;
        }
    return best;
}

static int windows()
{
    for (uint32_t M = 1; M <= 40; M++) {
        const uint32_t one[1] = {M};
        CHECK(onepass_commit_window(one, 1) == 2 * M - 1 && longest_span(M) == onepass_commit_window(one, 1));
    }
    CHECK(longest_span(12) == 23 && longest_span(1) == 1);
    const uint32_t mixed[5] = {8, 0, 200, 14, 0}, none[3] = {0, 0, 0};  // 0: an invalid slot
    CHECK(onepass_commit_window(mixed, 5) == 399 && onepass_commit_window(mixed, 2) == 15 && onepass_commit_window(mixed + 3, 2) == 27);
    CHECK(onepass_commit_window(none, 3) == 0 && onepass_commit_window(none, 0) == 0);
    const uint32_t cap[1] = {16383};
    CHECK(onepass_commit_window(cap, 1) == 32765);
    return 0;
}

int main()
{
    if (lists() || windows()) return 1;
    std::printf("plan_check ok\n");
    return 0;
}
