// The host mirror of a live connected-word decoding session (csrc/sr_decode_live_plan.h) on the CPU, without a device: row
// counting, the cap and the order of the refusals, distinct-channel lists.  A stand-alone program for the sanitizers:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I<csrc> plan_check.cpp -o plan_check && ./plan_check
// (tests/test_chain_live.py builds and runs it).  Prints "plan_check ok" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstdlib>

#include "sr_decode_live_plan.h"

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

// feature sessions: random pushes against a model kept next to the mirror
static int feature_walk()
{
    uint64_t seed = 1;
    for (uint32_t C : {1u, 3u, 6u, 17u}) {
        DecodeLiveMirror m;
        m.open(C, 7);
        m.chunk_max = 40;
        m.utt_frames = 200;
        std::vector<uint32_t> model(C, 0), n(C);
        for (int it = 0; it < 400; it++) {
            for (uint32_t c = 0; c < C; c++) n[c] = rnd(seed) % 3 == 0 ? 0u : rnd(seed) % 46;  // some above chunk_max
            DecodeLivePlan pl;
            std::string why;
            const std::vector<uint32_t> before = m.frames;
            const bool ok = decode_live_plan(m, 7, n.data(), 0, &pl, &why);
            // the first channel that breaks a rule names the refusal; a count above chunk_max comes before the cap
            bool want_ok = true;
            for (uint32_t c = 0; c < C && want_ok; c++) {
                if (n[c] > m.chunk_max) {
                    want_ok = false;
                    CHECK(!ok && has(why, "chunk_max") && has(why, ("channel " + std::to_string(c) + " ").c_str()));
                } else if (model[c] + n[c] > m.utt_frames) {
                    want_ok = false;
                    CHECK(!ok && has(why, "utt_frames") && has(why, ("channel " + std::to_string(c) + " ").c_str()));
                }
            }
            CHECK(ok == want_ok && m.frames == before);  // planning changes nothing
            if (!ok) {
                if (rnd(seed) % 4 == 0) {  // end the fullest channel, twice in the list, with another one
                    uint32_t full = 0;
                    for (uint32_t c = 0; c < C; c++)
                        if (model[c] > model[full]) full = c;
                    const uint32_t list[4] = {full, C - 1, full, C - 1};
                    std::vector<SpotLiveChan> chan;
                    std::vector<sr_chain_live_row> order;
                    CHECK(decode_live_end_list(m, 7, list, 4, &chan, &order, &why));
                    CHECK(chan.size() == C && order.size() == (full == C - 1 ? 1u : 2u));
                    CHECK(order[0].channel == full && order[0].frames == model[full] && chan[full].row_base == 0 && chan[full].first_win == 1);
                    if (full != C - 1) CHECK(order[1].channel == C - 1 && order[1].frames == model[C - 1] && chan[C - 1].row_base == 1);
                    for (uint32_t c = 0; c < C; c++) CHECK(chan[c].n == 0 && (chan[c].first_win != 0) == (c == full || c == C - 1));
                    decode_live_reset(m, 7, order);
                    model[full] = model[C - 1] = 0;
                    CHECK(m.frames == model);
                }
                continue;
            }
            uint32_t rows = 0, max_n = 0;
            for (uint32_t c = 0; c < C; c++) {
                const SpotLiveChan &ch = pl.chan[c];
                CHECK(ch.x0 == model[c] && ch.n == n[c] && (ch.first_win != 0) == (n[c] > 0));
                if (n[c]) CHECK(ch.row_base == rows);
                rows += n[c] > 0;
                max_n = std::max(max_n, n[c]);
                model[c] += n[c];
            }
            CHECK(pl.rows == rows && pl.max_n == max_n && pl.max_frames == max_n && pl.chan.size() == C);
            std::vector<sr_chain_live_row> out(rows + 1, sr_chain_live_row{0xAAAAAAAAu, 0xAAAAAAAAu});
            uint32_t n_rows = 0xDEADu;
            decode_live_advance(m, pl, out.data(), &n_rows);
            CHECK(n_rows == rows && m.frames == model && out[rows].channel == 0xAAAAAAAAu);  // rows past n_rows are not written
            for (uint32_t r = 0, c = 0; r < rows; r++, c++) {
                while (!n[c]) c++;
                CHECK(out[r].channel == c && out[r].frames == model[c]);  // ascending channels
            }
        }
    }
    return 0;
}

// n NULL = n_all on every channel; exactly utt_frames is reached, one more frame is not
static int uniform_counts_and_the_cap()
{
    DecodeLiveMirror m;
    m.open(4, 1);
    m.chunk_max = 64;
    m.utt_frames = 130;
    DecodeLivePlan pl;
    std::string why;
    sr_chain_live_row out[4];
    for (uint32_t cnt : {64u, 64u}) {
        CHECK(decode_live_plan(m, 1, nullptr, cnt, &pl, &why) && pl.rows == 4 && pl.max_frames == cnt);
        decode_live_advance(m, pl, out, nullptr);
    }
    CHECK(!decode_live_plan(m, 1, nullptr, 3, &pl, &why) && has(why, "channel 0 would pass utt_frames"));
    CHECK(!decode_live_plan(m, 1, nullptr, 65, &pl, &why) && has(why, "chunk_max"));
    CHECK(decode_live_plan(m, 1, nullptr, 2, &pl, &why));
    decode_live_advance(m, pl, out, nullptr);
    CHECK(out[3].channel == 3 && out[3].frames == 130);
    CHECK(decode_live_plan(m, 1, nullptr, 0, &pl, &why) && pl.rows == 0 && pl.max_n == 0);  // nothing pushed, nothing refused
    const uint32_t one[4] = {0, 1, 0, 0};
    CHECK(!decode_live_plan(m, 1, one, 0, &pl, &why) && has(why, "channel 1 would pass"));
    return 0;
}

// a replaced store: pushes to bound channels are refused until they are ended, which drops their recording
static int store_binding()
{
    DecodeLiveMirror m;
    m.open(3, 10);
    m.chunk_max = 50;
    m.utt_frames = 100;
    DecodeLivePlan pl;
    std::string why;
    sr_chain_live_row out[3];
    const uint32_t first[3] = {20, 0, 30};
    CHECK(decode_live_plan(m, 10, first, 0, &pl, &why) && pl.rows == 2);
    decode_live_advance(m, pl, out, nullptr);
    CHECK(out[0].channel == 0 && out[0].frames == 20 && out[1].channel == 2 && out[1].frames == 30);
    const uint32_t big[3] = {51, 1, 1}, quiet[3] = {0, 0, 0}, mid_only[3] = {0, 5, 0};
    CHECK(!decode_live_plan(m, 11, big, 0, &pl, &why) && has(why, "chunk_max"));         // the count comes first
    CHECK(!decode_live_plan(m, 11, mid_only, 0, &pl, &why) && has(why, "store changed") && has(why, "channel 1"));
    CHECK(decode_live_plan(m, 11, quiet, 0, &pl, &why) && pl.rows == 0);
    const uint32_t list[3] = {2, 1, 2}, bad[2] = {0, 3};
    std::vector<SpotLiveChan> chan;
    std::vector<sr_chain_live_row> order;
    CHECK(!decode_live_end_list(m, 11, bad, 2, &chan, &order, &why) && has(why, "channel 3"));
    CHECK(decode_live_end_list(m, 11, list, 3, &chan, &order, &why) && order.size() == 2);
    CHECK(order[0].channel == 2 && order[0].frames == 0 && order[1].channel == 1 && order[1].frames == 0);  // dropped
    CHECK(m.frames[2] == 30);  // listing changes nothing
    decode_live_reset(m, 11, order);
    CHECK(m.frames[2] == 0 && m.bound[2] == 11 && m.bound[1] == 11 && m.bound[0] == 10 && m.frames[0] == 20);
    CHECK(decode_live_plan(m, 11, mid_only, 0, &pl, &why) && pl.rows == 1 && pl.chan[1].x0 == 0);
    const uint32_t zero_first[3] = {1, 0, 0};
    CHECK(!decode_live_plan(m, 11, zero_first, 0, &pl, &why) && has(why, "channel 0"));
    CHECK(decode_live_end_list(m, 11, nullptr, 0, &chan, &order, &why) && order.empty() && chan.size() == 3);
    return 0;
}

// PCM sessions: frames from samples, the kept tail, a row for every channel that got samples
static int pcm_counts()
{
    DecodeLiveMirror m;
    m.open(2, 1);
    m.pcm = true;
    m.frame_len = 160;
    m.hop = 80;
    m.chunk_max = 400;
    m.utt_frames = 5;
    DecodeLivePlan pl;
    std::string why;
    sr_chain_live_row out[2];
    uint64_t seed = 5;
    uint32_t got[2] = {0, 0};
    for (int it = 0; it < 200; it++) {
        uint32_t n[2] = {rnd(seed) % 90, rnd(seed) % 5 == 0 ? 0u : rnd(seed) % 200};
        auto frames_of = [](uint32_t s) { return s >= 161 ? (s - 161) / 80 + 1 : 0u; };
        const bool fits = frames_of(got[0] + n[0]) <= 5 && frames_of(got[1] + n[1]) <= 5;
        const bool ok = decode_live_plan(m, 1, n, 0, &pl, &why);
        CHECK(ok == fits);
        if (!ok) break;
        for (int c = 0; c < 2; c++) {
            const SpotLiveChan &ch = pl.chan[c];
            CHECK(ch.x0 == frames_of(got[c]) && ch.n == frames_of(got[c] + n[c]) - frames_of(got[c]) && ch.n_samp == n[c]);
            CHECK(ch.kept == got[c] - ch.x0 * 80 && ch.drop == ch.n * 80 && (ch.first_win != 0) == (n[c] > 0));
            got[c] += n[c];
        }
        CHECK(pl.rows == (uint32_t)(n[0] > 0) + (n[1] > 0));
        decode_live_advance(m, pl, out, nullptr);
        CHECK(m.frames[0] == frames_of(got[0]) && m.kept[1] == got[1] - m.frames[1] * 80);
    }
    CHECK(decode_live_state_bytes(15, 9, 5, 200) == 5u * 9 * 15 * 16 + 201u * (5 * 8 + 6 * 4));
    CHECK(decode_live_state_bytes(16383, 65536, 16, 16383) == 0xFFFFFFFFu);
    return 0;
}

int main()
{
    if (feature_walk() || uniform_counts_and_the_cap() || store_binding() || pcm_counts()) return 1;
    std::printf("plan_check ok\n");
    return 0;
}
