// The host mirror of a live word-spotting session (csrc/sr_spot_live_plan.h) on the CPU, without a device: the windows a push
// completes and their rows, the framing of PCM pushes and that the decoders' plan frames alike, the refusals and their order,
// the distinct-channel flush list.  Every expected value is a literal worked out by hand from the definitions.  A stand-alone
// program for the sanitizers:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I<csrc> plan_check.cpp -o plan_check && ./plan_check
// (tests/test_spot_live.py builds and runs it).  Prints "plan_check ok" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstdlib>

#include "sr_decode_live_plan.h"
#include "sr_spot_live_plan.h"

using namespace sr;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("plan_check: line %d: %s\n", __LINE__, #cond);     \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

static SpotLiveMirror feature_session(uint32_t C, uint32_t win, uint32_t origin)
{
    SpotLiveMirror m;
    m.open(C, 7, origin);
    m.chunk_max = 20;
    m.win = win;
    return m;
}

// win = 5, a channel at x0 = 3: window 0 ends with frame 4, window 1 with frame 9, window 2 with frame 14
static int windows_across_a_push()
{
    CHECK(spot_live_windows_done(3, 1, 5) == 0 && spot_live_windows_done(3, 2, 5) == 1 && spot_live_windows_done(3, 12, 5) == 3);
    CHECK(spot_live_windows_done(3, 0, 5) == 0 && spot_live_windows_done(5, 5, 5) == 1 && spot_live_windows_done(0, 4, 5) == 0);
    const SpotLiveMirror m = feature_session(1, 5, 3);
    LivePlan pl;
    std::string why;
    CHECK(spot_live_plan(m, 7, nullptr, 1, &pl, &why) && pl.rows == 0 && pl.chan[0].x0 == 3 && pl.chan[0].n == 1);
    CHECK(spot_live_plan(m, 7, nullptr, 2, &pl, &why) && pl.rows == 1 && pl.chan[0].first_win == 0 && pl.chan[0].row_base == 0);
    CHECK(spot_live_plan(m, 7, nullptr, 12, &pl, &why) && pl.rows == 3 && pl.max_n == 12 && pl.max_frames == 12 && pl.max_row == 0);
    SpotLiveMirror after = m;
    sr_spot_win wins[4] = {{9, 9}, {9, 9}, {9, 9}, {9, 9}};
    uint32_t n_rows = 0xDEADu;
    spot_live_advance(after, pl, wins, &n_rows);
    CHECK(n_rows == 3 && after.frames[0] == 15 && m.frames[0] == 3);  // planning changed nothing
    CHECK(wins[0].channel == 0 && wins[0].window == 0 && wins[1].window == 1 && wins[2].window == 2);
    CHECK(wins[3].channel == 9 && wins[3].window == 9);  // rows past n_rows are not written
    CHECK(spot_live_plan(after, 7, nullptr, 0, &pl, &why) && pl.rows == 0 && pl.max_n == 0 && pl.chan[0].first_win == 3);
    return 0;
}

// channels 0, 1, 2 at 3, 4 and 0 frames get 2, 0 and 10: one window, none, two
static int row_bases()
{
    SpotLiveMirror m = feature_session(3, 5, 0);
    m.frames = {3, 4, 0};
    const uint32_t n[3] = {2, 0, 10};
    LivePlan pl;
    std::string why;
    CHECK(spot_live_plan(m, 7, n, 99, &pl, &why));  // n given: n_all is not looked at
    CHECK(pl.chan[0].row_base == 0 && pl.chan[1].row_base == 1 && pl.chan[2].row_base == 1 && pl.rows == 3);
    CHECK(pl.chan[0].first_win == 0 && pl.chan[1].first_win == 0 && pl.chan[2].first_win == 0 && pl.max_n == 10 && pl.max_frames == 10);
    sr_spot_win wins[3];
    spot_live_advance(m, pl, wins, nullptr);
    CHECK(wins[0].channel == 0 && wins[0].window == 0 && wins[1].channel == 2 && wins[1].window == 0 && wins[2].channel == 2 && wins[2].window == 1);
    CHECK(m.frames[0] == 5 && m.frames[1] == 4 && m.frames[2] == 10);
    return 0;
}

static SpotLiveMirror pcm_session(uint32_t C)
{
    SpotLiveMirror m = feature_session(C, 1, 0);
    m.pcm = true;
    m.frame_len = 8;
    m.hop = 4;
    return m;
}

// frame_len = 8, hop = 4: frame 0 needs 9 samples (its pre-emphasis predecessor and 8), frame 1 needs 13
static int pcm_framing()
{
    const SpotLiveMirror fresh = pcm_session(1);
    LivePlan pl;
    std::string why;
    CHECK(spot_live_plan(fresh, 7, nullptr, 8, &pl, &why) && pl.chan[0].n == 0 && pl.chan[0].drop == 0 && pl.rows == 0 && pl.max_row == 8);
    CHECK(spot_live_plan(fresh, 7, nullptr, 13, &pl, &why) && pl.chan[0].n == 2 && pl.chan[0].drop == 8 && pl.rows == 2);
    CHECK(spot_live_plan(fresh, 7, nullptr, 9, &pl, &why) && pl.chan[0].n == 1 && pl.chan[0].drop == 4 && pl.chan[0].kept == 0);
    CHECK(pl.chan[0].n_samp == 9 && pl.max_n == 9 && pl.max_frames == 1 && pl.max_row == 9 && pl.rows == 1);
    SpotLiveMirror m = fresh;
    sr_spot_win wins[2];
    spot_live_advance(m, pl, wins, nullptr);
    CHECK(m.kept[0] == 5 && m.frames[0] == 1);  // kept + n_samp - drop = 0 + 9 - 4
    // four more samples make 13 in all: the second frame, from a row of 5 kept and 4 new samples
    CHECK(spot_live_plan(m, 7, nullptr, 4, &pl, &why) && pl.chan[0].kept == 5 && pl.chan[0].n == 1 && pl.chan[0].drop == 4 && pl.chan[0].x0 == 1);
    CHECK(pl.max_row == 9 && pl.max_n == 4);
    spot_live_advance(m, pl, wins, nullptr);
    CHECK(m.kept[0] == 5 && m.frames[0] == 2);
    CHECK(spot_live_plan(m, 7, nullptr, 0, &pl, &why) && pl.chan[0].n == 0 && pl.max_row == 0);  // no samples: no row to stage
    // the rule itself, where a 32-bit sum would wrap
    SpotLiveChan ch{};
    uint32_t max_row = 0;
    CHECK(live_pcm_frames(0xFFFFFFFFu, 10, 8, 4, &ch, &max_row) == 0x40000001u);  // (2^32 + 9 - 9) / 4 + 1
    return 0;
}

// win = 1: the decoders' plan, on a mirror opened with the same framing, frames the same pushes alike
static int the_two_plans_agree()
{
    SpotLiveMirror sm = pcm_session(2);
    DecodeLiveMirror dm;
    dm.open(2, 7);
    dm.pcm = true;
    dm.frame_len = 8;
    dm.hop = 4;
    dm.chunk_max = 20;
    dm.utt_frames = 1000;
    const uint32_t pushes[6][2] = {{9, 0}, {4, 13}, {0, 3}, {7, 8}, {20, 1}, {0, 0}};
    const uint32_t frames_after[6][2] = {{1, 0}, {2, 2}, {2, 2}, {3, 4}, {8, 5}, {8, 5}};  // (total - 9) / 4 + 1 of 9, 13, 13, 20, 40, 40 | 0, 13, 16, 24, 25, 25
    for (int i = 0; i < 6; i++) {
        LivePlan sp;
        DecodeLivePlan dp;
        std::string why;
        CHECK(spot_live_plan(sm, 7, pushes[i], 0, &sp, &why) && decode_live_plan(dm, 7, pushes[i], 0, &dp, &why));
        for (int c = 0; c < 2; c++) {
            const SpotLiveChan &a = sp.chan[c], &b = dp.chan[c];
            CHECK(a.x0 == b.x0 && a.n == b.n && a.kept == b.kept && a.n_samp == b.n_samp && a.drop == b.drop);
            CHECK(a.x0 + a.n == frames_after[i][c]);
        }
        CHECK(sp.max_row == dp.max_row && sp.max_n == dp.max_n && sp.max_frames == dp.max_frames);
        sr_spot_win wins[8];
        sr_chain_live_row rows[2];
        spot_live_advance(sm, sp, wins, nullptr);
        decode_live_advance(dm, dp, rows, nullptr);
        CHECK(sm.frames == dm.frames && sm.kept == dm.kept);
    }
    return 0;
}

static int refusals_in_order()
{
    SpotLiveMirror m = feature_session(3, 5, 0);
    m.frames = {3, 4, 0};
    m.bound[1] = 6;  // channel 1 is bound to a store that is gone
    const SpotLiveMirror before = m;
    LivePlan pl;
    std::string why;
    const uint32_t big[3] = {2, 21, 0}, stale[3] = {2, 1, 0}, quiet[3] = {20, 0, 20}, big_first[3] = {21, 1, 0};
    CHECK(!spot_live_plan(m, 7, big, 0, &pl, &why) && has(why, "channel 1 exceeds chunk_max"));  // the count comes before the binding
    CHECK(!spot_live_plan(m, 7, stale, 0, &pl, &why) && has(why, "store changed") && has(why, "channel 1 "));
    CHECK(!spot_live_plan(m, 7, big_first, 0, &pl, &why) && has(why, "channel 0 exceeds chunk_max"));  // channels in ascending order
    CHECK(spot_live_plan(m, 7, quiet, 0, &pl, &why) && pl.rows == 8);  // nothing for the stale channel: 4 windows each for the others
    CHECK(!spot_live_plan(m, 7, nullptr, 21, &pl, &why) && has(why, "chunk_max"));
    CHECK(m.frames == before.frames && m.kept == before.kept && m.bound == before.bound);  // a refused plan leaves the mirror as it was
    // the frame cap: 0xFFFF0000 is reached, not passed
    SpotLiveMirror far = feature_session(2, 5, 0xFFFF0000u - 1);
    far.frames[0] = 0;
    const uint32_t two[2] = {0, 2}, one[2] = {20, 1};
    CHECK(!spot_live_plan(far, 7, two, 0, &pl, &why) && has(why, "channel 1 would pass 0xFFFF0000"));
    CHECK(far.frames[0] == 0 && far.frames[1] == 0xFFFEFFFFu);
    CHECK(spot_live_plan(far, 7, one, 0, &pl, &why) && pl.rows == 5 && pl.chan[1].row_base == 4);  // 0xFFFF0000 / 5 is whole: one window
    CHECK(pl.chan[1].first_win == 0x33330000u - 1);                                              // 0xFFFF0000 / 5 = 0x33330000
    return 0;
}

static int end_list()
{
    SpotLiveMirror m = feature_session(3, 5, 0);
    m.frames = {10, 4, 7};
    m.kept = {1, 2, 3};
    const uint32_t listed[3] = {2, 0, 2}, past[2] = {0, 3};
    std::vector<SpotLiveFlush> list;
    uint32_t rows = 99;
    std::string why;
    CHECK(!spot_live_end_list(m, 7, 7, past, 2, &list, &rows, &why) && has(why, "channel 3 "));
    CHECK(spot_live_end_list(m, 7, 7, listed, 3, &list, &rows, &why) && list.size() == 2 && rows == 1);
    CHECK(list[0].channel == 2 && list[0].row == 0 && list[0].wid == 1);            // 7 frames: two into window 1
    CHECK(list[1].channel == 0 && list[1].row == 0xFFFFFFFFu && list[1].wid == 2);  // 10 frames: no window is open
    CHECK(m.frames[2] == 7);  // listing changes nothing
    // the state is laid out for a store that is gone, or the channel is bound to one: reset only
    CHECK(spot_live_end_list(m, 7, 8, listed, 3, &list, &rows, &why) && list.size() == 2 && rows == 0 && list[0].row == 0xFFFFFFFFu);
    m.bound[2] = 6;
    CHECK(spot_live_end_list(m, 7, 7, listed, 3, &list, &rows, &why) && rows == 0 && list[0].channel == 2 && list[0].row == 0xFFFFFFFFu);
    m.bound[2] = 7;
    CHECK(spot_live_end_list(m, 7, 7, nullptr, 0, &list, &rows, &why) && list.empty() && rows == 0);
    CHECK(spot_live_end_list(m, 7, 7, listed, 3, &list, &rows, &why) && rows == 1);
    sr_spot_win wins[2] = {{9, 9}, {9, 9}};
    spot_live_reset(m, 8, 0, list, wins);
    CHECK(wins[0].channel == 2 && wins[0].window == 1 && wins[1].channel == 9);
    CHECK(m.frames[0] == 0 && m.frames[1] == 4 && m.frames[2] == 0 && m.kept[0] == 0 && m.kept[1] == 2 && m.kept[2] == 0);
    CHECK(m.bound[0] == 8 && m.bound[1] == 7 && m.bound[2] == 8);
    CHECK(spot_live_state_bytes(6, 70) == 6912 && spot_live_state_bytes(65536, 16383) == 17180917760ull);  // K * (tpl_len * 16 + 32)
    return 0;
}

int main()
{
    if (windows_across_a_push() || row_bases() || pcm_framing() || the_two_plans_agree() || refusals_in_order() || end_list()) return 1;
    std::printf("plan_check ok\n");
    return 0;
}
