// The host-only logic of a live grammar-constrained decoding session (csrc/sr_gram_live_plan.h, on top of the decoder's
// mirror in csrc/sr_decode_live_plan.h) on the CPU, without a device: the per-level column offsets, the state bytes, the
// stale-grammar check, the "every channel empty" rule of sr_gram_live_set_grammar, and row counting through a session's life
// as sr_gram_live.cpp drives the mirror.  A stand-alone program for the sanitizers:
//   hipcc --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I<csrc> plan_check.cpp -o plan_check && ./plan_check
// (tests/test_gram_live.py builds and runs it).  Prints "plan_check ok" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstdlib>

#include "sr_gram_live_plan.h"

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

// offsets are the running sum of the kept items, levels without items take no column and no launch
static int column_offsets()
{
    const uint32_t seq[5] = {3, 3, 2, 0, 0};
    GramLiveLayout lay = gram_live_layout(seq, 5);
    CHECK(lay.columns == 8 && lay.levels == 3 && lay.launches() == 8);
    CHECK(lay.col_off[0] == 0 && lay.col_off[1] == 3 && lay.col_off[2] == 6 && lay.col_off[3] == 8 && lay.col_off[4] == 8);
    lay = gram_live_layout(seq, 2);  // max_words below the list: only its levels
    CHECK(lay.columns == 6 && lay.levels == 2 && lay.col_off[1] == 3 && lay.col_off[2] == 0);
    const uint32_t none[3] = {0, 0, 0};
    lay = gram_live_layout(none, 3);
    CHECK(lay.columns == 0 && lay.levels == 0 && lay.launches() == 2);
    const uint32_t holes[4] = {0, 5, 0, 1};  // a level without items between two with
    lay = gram_live_layout(holes, 4);
    CHECK(lay.columns == 6 && lay.levels == 2 && lay.col_off[0] == 0 && lay.col_off[1] == 0 && lay.col_off[2] == 5 && lay.col_off[3] == 5);
    uint32_t full[kChainMaxWords];
    for (uint32_t l = 0; l < kChainMaxWords; l++) full[l] = 1u << 20;  // the most a grammar compiles to, at every level
    lay = gram_live_layout(full, kChainMaxWords);
    CHECK(lay.columns == 16u << 20 && lay.levels == 16 && lay.launches() == 34 && lay.col_off[15] == 15u << 20);
    uint64_t seed = 3;
    for (int it = 0; it < 200; it++) {  // every level's columns lie behind the previous level's, none overlap
        uint32_t items[kChainMaxWords], W = 1 + rnd(seed) % kChainMaxWords, sum = 0, lv = 0;
        for (uint32_t l = 0; l < W; l++) items[l] = rnd(seed) % 3 ? rnd(seed) % 50 : 0u;
        lay = gram_live_layout(items, W);
        for (uint32_t l = 0; l < W; l++) {
            CHECK(lay.col_off[l] == sum);
            sum += items[l];
            lv += items[l] != 0;
        }
        CHECK(lay.columns == sum && lay.levels == lv);
    }
    CHECK(gram_live_state_bytes(8, 14, 4, 5, 160) == 8u * 14 * 16 + 161u * 4 * (5 * 8 + 6 * 4));
    CHECK(gram_live_state_bytes(5, 14, 1, 5, 160) == decode_live_state_bytes(14, 1, 5, 160));  // the anchor: the decoder's state
    CHECK(gram_live_state_bytes(0, 14, 3, 5, 160) == 161u * 3 * 64);
    CHECK(gram_live_state_bytes(16u << 20, 16383, 64, 16, 16383) == 0xFFFFFFFFu);  // saturates
    return 0;
}

static int staleness()
{
    std::string why;
    CHECK(!gram_live_stale(4, 9, 4, 9, &why) && why.empty());
    CHECK(gram_live_stale(4, 9, 5, 9, &why) && has(why, "template store"));
    CHECK(gram_live_stale(4, 9, 4, 10, &why) && has(why, "word map"));
    CHECK(gram_live_stale(4, 9, 5, 10, &why) && has(why, "template store"));  // the store is named first
    return 0;
}

// a session's life as sr_gram_live.cpp drives the mirror: pushes, set_grammar refusals, a stale end, ends
static int session_walk()
{
    uint64_t seed = 11;
    for (uint32_t C : {1u, 4u, 6u}) {
        DecodeLiveMirror m;
        m.open(C, kGramLiveBound);
        m.chunk_max = 40;
        m.utt_frames = 120;
        std::string why;
        CHECK(gram_live_all_empty(m, &why));  // freshly opened
        std::vector<uint32_t> model(C, 0), n(C);
        for (int it = 0; it < 300; it++) {
            for (uint32_t c = 0; c < C; c++) n[c] = rnd(seed) % 3 == 0 ? 0u : rnd(seed) % 41;
            DecodeLivePlan pl;
            const bool ok = decode_live_plan(m, kGramLiveBound, n.data(), 0, &pl, &why);
            bool fits = true;
            for (uint32_t c = 0; c < C; c++) fits = fits && model[c] + n[c] <= m.utt_frames;
            CHECK(ok == fits);
            if (ok) {
                uint32_t rows = 0;
                for (uint32_t c = 0; c < C; c++) {
                    CHECK(pl.chan[c].x0 == model[c] && pl.chan[c].n == n[c]);
                    if (n[c]) CHECK(pl.chan[c].row_base == rows && pl.chan[c].first_win == 1);
                    rows += n[c] > 0;
                    model[c] += n[c];
                }
                std::vector<sr_chain_live_row> out(rows + 1, sr_chain_live_row{0xAAAAAAAAu, 0xAAAAAAAAu});
                uint32_t n_rows = 0xDEADu;
                decode_live_advance(m, pl, out.data(), &n_rows);
                CHECK(n_rows == rows && pl.rows == rows && m.frames == model && out[rows].channel == 0xAAAAAAAAu);
            }
            // the grammar may be switched exactly while no channel holds a frame; the refusal names the first that does
            bool empty = true;
            uint32_t first = 0;
            for (uint32_t c = C; c-- > 0;)
                if (model[c]) empty = false, first = c;
            CHECK(gram_live_all_empty(m, &why) == empty);
            if (!empty) CHECK(has(why, ("channel " + std::to_string(first) + " ").c_str()));
            if (!ok || rnd(seed) % 5 == 0) {  // end some channels; one time in three under a stale grammar: the recordings are dropped
                const bool is_stale = rnd(seed) % 3 == 0;
                std::vector<uint32_t> list;
                for (uint32_t c = 0; c < C; c++)
                    if (!ok || rnd(seed) % 2) list.push_back(c), list.push_back(c);  // listed twice: counted once
                std::vector<SpotLiveChan> chan;
                std::vector<sr_chain_live_row> order;
                CHECK(decode_live_end_list(m, is_stale ? kGramLiveStale : kGramLiveBound, list.data(), (uint32_t)list.size(), &chan, &order, &why));
                CHECK(order.size() == list.size() / 2);
                for (uint32_t r = 0; r < order.size(); r++) {
                    const uint32_t c = order[r].channel;
                    CHECK(c == list[2 * r] && order[r].frames == (is_stale ? 0u : model[c]) && chan[c].row_base == r && chan[c].n == 0);
                    CHECK(chan[c].x0 == order[r].frames);  // what the trace reads as N: 0 = no parse
                }
                CHECK(m.frames == model);  // listing changes nothing
                decode_live_reset(m, kGramLiveBound, order);
                for (uint32_t r = 0; r < order.size(); r++) model[order[r].channel] = 0;
                CHECK(m.frames == model);
                for (uint32_t c = 0; c < C; c++) CHECK(m.bound[c] == kGramLiveBound);  // a later push plans against the same serial
                if (!ok) CHECK(gram_live_all_empty(m, &why));  // every channel was ended
            }
        }
    }
    return 0;
}

// PCM sessions: kept samples without a frame make a channel non-empty
static int pcm_channels()
{
    DecodeLiveMirror m;
    m.open(2, kGramLiveBound);
    m.pcm = true;
    m.frame_len = 160;
    m.hop = 80;
    m.chunk_max = 400;
    m.utt_frames = 50;
    DecodeLivePlan pl;
    std::string why;
    sr_chain_live_row out[2];
    const uint32_t few[2] = {0, 100};
    CHECK(decode_live_plan(m, kGramLiveBound, few, 0, &pl, &why) && pl.rows == 1 && pl.max_frames == 0);  // samples, no frame: a row all the same
    decode_live_advance(m, pl, out, nullptr);
    CHECK(out[0].channel == 1 && out[0].frames == 0 && m.frames[1] == 0 && m.kept[1] == 100);
    CHECK(!gram_live_all_empty(m, &why) && has(why, "channel 1 "));
    const uint32_t list[1] = {1};
    std::vector<SpotLiveChan> chan;
    std::vector<sr_chain_live_row> order;
    CHECK(decode_live_end_list(m, kGramLiveBound, list, 1, &chan, &order, &why) && order.size() == 1 && order[0].frames == 0);
    decode_live_reset(m, kGramLiveBound, order);
    CHECK(m.kept[1] == 0 && gram_live_all_empty(m, &why));
    return 0;
}

int main()
{
    if (column_offsets() || staleness() || session_walk() || pcm_channels()) return 1;
    std::printf("plan_check ok\n");
    return 0;
}
