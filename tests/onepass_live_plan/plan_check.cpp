// The host mirror of a live one-pass decoding session (csrc/sr_onepass_live_plan.h) on the CPU, without a device, against a
// brute-force restatement: the cut of every channel's push into blocks, frame by frame; the first frame of each channel's last
// block; the refusals and their order; the end list and what it wipes; the geometry formulas.  A stand-alone program for the
// sanitizers:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I<csrc> plan_check.cpp -o plan_check && ./plan_check
// (tests/test_onepass_live_ref.py builds and runs it).  Prints "plan_check ok" and returns 0, or says what failed and returns 1.
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

// what the kernels make of a plan entry (k_onepass_live.hip's onepass_live_block): block b of a channel, or none
static bool kernel_block(const SpotLiveChan &ch, uint32_t block, uint32_t b, uint32_t *xs, uint32_t *c0, uint32_t *cN)
{
    const uint32_t end = ch.x0 + ch.n;
    *c0 = ch.x0 + b * block;
    *cN = end - *c0 < block ? end : *c0 + block;
    *xs = *c0 ? (b ? *c0 - block : ch.aux) + 1u : 0u;
    return *c0 < end;
}

// random pushes, hooks and ends against a model that walks every channel frame by frame
static int block_walk()
{
    uint64_t seed = 3;
    for (uint32_t L : {1u, 2u, 5u, 36u}) {
        for (uint32_t C : {1u, 4u, 9u}) {
            OnePassLiveMirror m;
            m.open(C, 7);
            m.d.chunk_max = 3 * L + 7;
            m.d.utt_frames = 40 * L + 3;
            std::vector<uint32_t> frames(C, 0), last_c0(C, 0), n(C);
            for (int it = 0; it < 600; it++) {
                const uint32_t hook = rnd(seed) % 3 ? 0u : 1u + rnd(seed) % (L + 2);  // sometimes above L: clamped
                const uint32_t block = hook && hook < L ? hook : L;
                for (uint32_t c = 0; c < C; c++) n[c] = rnd(seed) % 4 == 0 ? 0u : rnd(seed) % (m.d.chunk_max + 2);
                OnePassLivePlan pl;
                std::string why;
                const OnePassLiveMirror before = m;
                const bool ok = onepass_live_plan(m, 7, L, hook, 0, n.data(), 0, &pl, &why);
                bool want_ok = true;
                for (uint32_t c = 0; c < C && want_ok; c++) {
                    if (n[c] > m.d.chunk_max) {
                        want_ok = false;
                        CHECK(!ok && has(why, "chunk_max") && has(why, ("channel " + std::to_string(c) + " ").c_str()));
                    } else if (frames[c] + n[c] > m.d.utt_frames) {
                        want_ok = false;
                        CHECK(!ok && has(why, "utt_frames") && has(why, ("channel " + std::to_string(c) + " ").c_str()));
                    }
                }
                CHECK(ok == want_ok && m.d.frames == before.d.frames && m.c0_prev == before.c0_prev);  // planning changes nothing
                if (!ok) {
                    if (rnd(seed) % 3 == 0) {  // end the fullest channel and the last one
                        uint32_t full = 0;
                        for (uint32_t c = 0; c < C; c++)
                            if (frames[c] > frames[full]) full = c;
                        const uint32_t list[3] = {full, C - 1, full};
                        std::vector<SpotLiveChan> chan;
                        std::vector<sr_chain_live_row> order;
                        CHECK(onepass_live_end_list(m, 7, list, 3, &chan, &order, &why) && order.size() == (full == C - 1 ? 1u : 2u));
                        for (uint32_t c = 0; c < C; c++) {
                            const bool listed = c == full || c == C - 1;
                            CHECK(chan[c].n == 0 && (chan[c].first_win != 0) == listed);
                            if (listed) CHECK(chan[c].x0 == frames[c] && chan[c].aux == frames[c]);  // parse and wipe what it holds
                        }
                        onepass_live_reset(m, 7, order);
                        frames[full] = frames[C - 1] = last_c0[full] = last_c0[C - 1] = 0;
                        CHECK(m.d.frames == frames && m.c0_prev == last_c0);
                    }
                    continue;
                }
                CHECK(pl.block == block && pl.block >= 1 && pl.block <= L);
                uint32_t most = 0;
                for (uint32_t c = 0; c < C; c++) {
                    const SpotLiveChan &ch = pl.d.chan[c];
                    CHECK(ch.x0 == frames[c] && ch.n == n[c] && ch.aux == last_c0[c]);
                    // the model: the push frame by frame, a block begins every `block` frames of the push
                    std::vector<uint32_t> starts;
                    for (uint32_t i = 0; i < n[c]; i++)
                        if (i % block == 0) starts.push_back(frames[c] + i);
                    most = std::max<uint32_t>(most, (uint32_t)starts.size());
                    uint32_t prev = last_c0[c];
                    for (uint32_t b = 0; b <= pl.n_blocks; b++) {
                        uint32_t xs, c0, cN;
                        const bool there = kernel_block(ch, pl.block, b, &xs, &c0, &cN);
                        CHECK(there == (b < starts.size()));
                        if (!there) continue;
                        const uint32_t want_end = b + 1 < starts.size() ? starts[b + 1] : frames[c] + n[c];
                        CHECK(c0 == starts[b] && cN == want_end && cN - c0 >= 1 && cN - c0 <= L);  // the blocks tile the push, none above L
                        CHECK(xs == (c0 ? prev + 1 : 0u) && xs <= c0 && c0 - (xs ? xs - 1 : 0) <= L);  // ... behind the block before it
                        prev = c0;
                    }
                    if (n[c]) last_c0[c] = prev;
                    frames[c] += n[c];
                }
                CHECK(pl.n_blocks == most && pl.n_blocks == (pl.d.max_frames + block - 1) / block);
                CHECK(2 * pl.n_blocks + 1 <= onepass_live_launches(m.d.chunk_max, block));
                std::vector<sr_chain_live_row> out(pl.d.rows + 1, sr_chain_live_row{0xAAAAAAAAu, 0xAAAAAAAAu});
                uint32_t n_rows = 0xDEADu;
                onepass_live_advance(m, pl, out.data(), &n_rows);
                CHECK(n_rows == pl.d.rows && m.d.frames == frames && m.c0_prev == last_c0 && out[pl.d.rows].channel == 0xAAAAAAAAu);
                for (uint32_t r = 0, c = 0; r < n_rows; r++, c++) {
                    while (!n[c]) c++;
                    CHECK(out[r].channel == c && out[r].frames == frames[c]);  // ascending channels
                }
            }
        }
    }
    return 0;
}

// the word-cost bound comes first and follows the store; a store without a valid slot runs one block per push
static int cost_bound_and_empty_store()
{
    OnePassLiveMirror m;
    m.open(2, 1);
    m.d.chunk_max = 100;
    m.d.utt_frames = 1000;
    OnePassLivePlan pl;
    std::string why;
    const uint32_t at = (1u << 30) / 66;  // L = 15: 66 words in 1000 frames at most
    CHECK(onepass_live_plan(m, 1, 15, 0, at, nullptr, 10, &pl, &why) && pl.block == 15 && pl.n_blocks == 1);
    CHECK(!onepass_live_plan(m, 1, 15, 0, at + 1, nullptr, 10, &pl, &why) && has(why, "2^30"));
    CHECK(!onepass_live_plan(m, 1, 15, 0, at + 1, nullptr, 101, &pl, &why) && has(why, "2^30"));  // before the counts
    CHECK(!onepass_live_plan(m, 1, 8, 0, at, nullptr, 10, &pl, &why) && has(why, "2^30"));        // a store with a smaller L
    CHECK(onepass_live_plan(m, 1, 0, 0, 1u << 24, nullptr, 100, &pl, &why) && pl.block == 100 && pl.n_blocks == 1);  // no valid slot
    CHECK(onepass_live_plan(m, 1, 0, 3, 0, nullptr, 0, &pl, &why) && pl.block == 1 && pl.n_blocks == 0 && pl.d.rows == 0);
    CHECK(onepass_live_plan(m, 1, 15, 4, 0, nullptr, 100, &pl, &why) && pl.block == 4 && pl.n_blocks == 25);
    CHECK(onepass_live_plan(m, 1, 15, 99, 0, nullptr, 100, &pl, &why) && pl.block == 15 && pl.n_blocks == 7);
    return 0;
}

// a replaced store: pushes to bound channels are refused until they are ended; the end parses nothing but wipes what was held
static int store_binding()
{
    OnePassLiveMirror m;
    m.open(3, 10);
    m.d.chunk_max = 50;
    m.d.utt_frames = 100;
    OnePassLivePlan pl;
    std::string why;
    sr_chain_live_row out[3];
    const uint32_t first[3] = {20, 0, 33};
    CHECK(onepass_live_plan(m, 10, 5, 0, 0, first, 0, &pl, &why) && pl.d.rows == 2 && pl.n_blocks == 7);
    onepass_live_advance(m, pl, out, nullptr);
    CHECK(m.c0_prev[0] == 15 && m.c0_prev[1] == 0 && m.c0_prev[2] == 30);
    const uint32_t mid_only[3] = {0, 5, 0}, quiet[3] = {0, 0, 0};
    CHECK(!onepass_live_plan(m, 11, 5, 0, 0, mid_only, 0, &pl, &why) && has(why, "store changed") && has(why, "channel 1"));
    CHECK(onepass_live_plan(m, 11, 5, 0, 0, quiet, 0, &pl, &why) && pl.d.rows == 0 && pl.n_blocks == 0);
    const uint32_t list[3] = {2, 1, 2}, bad[2] = {0, 3};
    std::vector<SpotLiveChan> chan;
    std::vector<sr_chain_live_row> order;
    CHECK(!onepass_live_end_list(m, 11, bad, 2, &chan, &order, &why) && has(why, "channel 3"));
    CHECK(onepass_live_end_list(m, 11, list, 3, &chan, &order, &why) && order.size() == 2);
    CHECK(order[0].channel == 2 && order[0].frames == 0 && chan[2].x0 == 0 && chan[2].aux == 33);  // dropped, and wiped
    CHECK(order[1].channel == 1 && chan[1].aux == 0 && chan[0].first_win == 0 && chan[0].aux == 0);
    CHECK(m.d.frames[2] == 33 && m.c0_prev[2] == 30);  // listing changes nothing
    onepass_live_reset(m, 11, order);
    CHECK(m.d.frames[2] == 0 && m.c0_prev[2] == 0 && m.d.bound[2] == 11 && m.d.bound[0] == 10 && m.c0_prev[0] == 15);
    CHECK(onepass_live_plan(m, 11, 5, 0, 0, mid_only, 0, &pl, &why) && pl.d.chan[1].x0 == 0 && pl.d.chan[1].aux == 0);
    return 0;
}

// PCM sessions: the blocks are cut from the frames a push completes, not from its samples
static int pcm_blocks()
{
    OnePassLiveMirror m;
    m.open(2, 1);
    m.d.pcm = true;
    m.d.frame_len = 160;
    m.d.hop = 80;
    m.d.chunk_max = 800;
    m.d.utt_frames = 50;
    OnePassLivePlan pl;
    std::string why;
    sr_chain_live_row out[2];
    const uint32_t a[2] = {161 + 80 * 6, 100};  // 7 frames, none
    CHECK(onepass_live_plan(m, 1, 3, 0, 0, a, 0, &pl, &why) && pl.d.rows == 2 && pl.d.max_frames == 7 && pl.n_blocks == 3);
    CHECK(pl.d.chan[0].n == 7 && pl.d.chan[1].n == 0 && pl.d.chan[1].first_win == 1);
    onepass_live_advance(m, pl, out, nullptr);
    CHECK(m.c0_prev[0] == 6 && m.c0_prev[1] == 0 && m.d.frames[0] == 7);
    const uint32_t b[2] = {10, 10};  // samples, but no new frame: rows, no block
    CHECK(onepass_live_plan(m, 1, 3, 0, 0, b, 0, &pl, &why) && pl.d.rows == 2 && pl.n_blocks == 0);
    onepass_live_advance(m, pl, out, nullptr);
    CHECK(m.c0_prev[0] == 6 && out[0].frames == 7 && out[1].frames == 0);
    return 0;
}

static int geometry()
{
    CHECK(onepass_live_state_bytes(14, 5, 200) == 201u * 12 + 5u * 14 * 16 + 200u * 24);
    CHECK(onepass_live_state_bytes(1, 1, 1) == 2u * 12 + 16 + 24);
    CHECK(onepass_live_state_bytes(16383, 65536, 16383) == 0xFFFFFFFFu);
    for (uint32_t L : {1u, 5u, 36u})
        for (uint32_t chunk : {1u, 4u, 5u, 6u, 100u, 16383u}) {
            const uint32_t blocks = (chunk + L - 1) / L;
            CHECK(onepass_live_launches(chunk, L) == 2 * blocks + 1 && onepass_live_launches(chunk, L) <= 2 * blocks + 2);
        }
    CHECK(onepass_live_block(5, 0, 9) == 5 && onepass_live_block(5, 5, 9) == 5 && onepass_live_block(5, 2, 9) == 2);
    CHECK(onepass_live_block(0, 2, 9) == 9 && onepass_live_block(0, 0, 0) == 1);
    return 0;
}

int main()
{
    if (block_walk() || cost_bound_and_empty_store() || store_binding() || pcm_blocks() || geometry()) return 1;
    std::printf("plan_check ok\n");
    return 0;
}
