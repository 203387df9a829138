// The host plan of a live one-pass grammar decoding session (csrc/sr_onepass_gram_live_plan.h) on the CPU, without a device,
// against a brute-force restatement: the state bytes added up element by element, the launches counted launch by launch, the
// cut of every channel's push into blocks frame by frame, the mirror's advance, the end list of a fresh and of a stale grammar
// and the reset.  A stand-alone program for the sanitizers:
//   hipcc --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I<csrc> plan_check.cpp -o plan_check && ./plan_check
// (tests/test_onepass_gram_live_ref.py builds and runs it).  Prints "plan_check ok" and returns 0, or says what failed and
// returns 1.
#include <cstdio>
#include <cstdlib>

#include "sr_onepass_gram_live_plan.h"

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

// what the kernels make of a plan entry (k_onepass_gram_live.hip's opgl_block and the sweep's xs): block b of a channel, or none
static bool kernel_block(const SpotLiveChan &ch, uint32_t block, uint32_t b, uint32_t *xs, uint32_t *c0, uint32_t *cN)
{
    const uint32_t end = ch.x0 + ch.n;
    *c0 = ch.x0 + b * block;
    *cN = end - *c0 < block ? end : *c0 + block;
    *xs = *c0 ? (b ? *c0 - block : ch.aux) + 1u : 0u;
    return *c0 < end;
}

// the state of one channel, added up element by element
static int state_bytes()
{
    for (uint32_t S : {1u, 2u, 7u, 64u})
        for (uint32_t items : {0u, 1u, 5u, 300u})
            for (uint32_t tpl : {1u, 14u, 151u})
                for (uint32_t utt : {1u, 80u, 4000u, 16383u}) {
                    uint64_t sum = 0;
                    for (uint32_t s = 0; s < S; s++)
                        for (uint32_t p = 0; p <= utt; p++) sum += 8 + 4;  // a key and a prefix cost per state and position
                    for (uint32_t i = 0; i < items; i++) sum += (uint64_t)tpl * 16;  // one saved column per kept item
                    sum += (uint64_t)utt * 12 * 2;                                    // the feature row
                    CHECK(onepass_gram_live_state_bytes(S, items, tpl, utt) == (sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sum));
                }
    CHECK(onepass_gram_live_state_bytes(64, 0xFFFFFFFFu, 16383, 16383) == 0xFFFFFFFFu);  // saturates
    CHECK(onepass_gram_live_state_bytes(1, 5, 14, 200) == onepass_live_state_bytes(14, 5, 200));  // the anchor: the one-pass session's
    return 0;
}

// the launches of a push, counted launch by launch as launch_onepass_gram_live enqueues them
static int launches()
{
    for (uint32_t items : {0u, 1u, 9u})
        for (uint32_t states : {0u, 1u, 4u})
            for (uint32_t block : {1u, 2u, 5u, 36u})
                for (uint32_t chunk : {1u, 4u, 5u, 6u, 100u, 16383u}) {
                    uint32_t n = 0;
                    for (uint32_t c0 = 0; c0 < chunk; c0 += block) {
                        if (items) n++;   // the sweep
                        if (states) n++;  // the close
                    }
                    n++;  // the trace
                    CHECK(onepass_gram_live_launches(chunk, block, items, states) == n);
                    CHECK(onepass_gram_live_push_launches((chunk + block - 1) / block, items, states) == n);
                }
    CHECK(onepass_gram_live_push_launches(0, 3, 2) == 1);  // samples, but no new frame: the trace only
    CHECK(onepass_gram_live_per_block(0, 0) == 0 && onepass_gram_live_per_block(0, 3) == 1 && onepass_gram_live_per_block(2, 3) == 2);
    CHECK(onepass_gram_live_launches(13, 5, 4, 2) == onepass_live_launches(13, 5));  // something kept: the one-pass session's count
    return 0;
}

// random pushes, hooks and ends against a model that walks every channel frame by frame; the session is bound to the constant
static int block_walk()
{
    uint64_t seed = 5;
    for (uint32_t L : {1u, 2u, 5u, 36u}) {
        for (uint32_t C : {1u, 4u, 9u}) {
            OnePassLiveMirror m;
            m.open(C, kGramLiveBound);
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
                const bool ok = onepass_gram_live_plan(m, L, hook, n.data(), 0, &pl, &why);
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
                    if (rnd(seed) % 3 == 0) {  // end the fullest channel and the last one, under a fresh or a stale grammar
                        uint32_t full = 0;
                        for (uint32_t c = 0; c < C; c++)
                            if (frames[c] > frames[full]) full = c;
                        const bool stale = rnd(seed) % 2;
                        const uint32_t list[3] = {full, C - 1, full};
                        std::vector<SpotLiveChan> chan;
                        std::vector<sr_chain_live_row> order;
                        CHECK(onepass_live_end_list(m, stale ? kGramLiveStale : kGramLiveBound, list, 3, &chan, &order, &why));
                        CHECK(order.size() == (full == C - 1 ? 1u : 2u));
                        for (uint32_t c = 0; c < C; c++) {
                            const bool listed = c == full || c == C - 1;
                            CHECK(chan[c].n == 0 && (chan[c].first_win != 0) == listed);
                            // a fresh grammar parses what the channel holds, a stale one drops it; both wipe what it held
                            if (listed) CHECK(chan[c].x0 == (stale ? 0u : frames[c]) && chan[c].aux == frames[c]);
                        }
                        for (const sr_chain_live_row &r : order) CHECK(r.frames == (stale ? 0u : frames[r.channel]));
                        onepass_live_reset(m, kGramLiveBound, order);
                        frames[full] = frames[C - 1] = last_c0[full] = last_c0[C - 1] = 0;
                        CHECK(m.d.frames == frames && m.c0_prev == last_c0);
                        for (uint32_t c = 0; c < C; c++) CHECK(m.d.bound[c] == kGramLiveBound);  // ... and the binding stays the constant
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
                        CHECK(cN <= m.d.utt_frames);                                                  // A(col + 1) stays inside the state's row
                        prev = c0;
                    }
                    if (n[c]) last_c0[c] = prev;
                    frames[c] += n[c];
                }
                CHECK(pl.n_blocks == most && pl.n_blocks == (pl.d.max_frames + block - 1) / block);
                CHECK(onepass_gram_live_push_launches(pl.n_blocks, 3, 2) <= onepass_gram_live_launches(m.d.chunk_max, block, 3, 2));
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

// no cost bound in a push's plan; a store without a valid slot runs one block per push; staleness and emptiness
static int bound_free_plan_and_grammar_rules()
{
    OnePassLiveMirror m;
    m.open(2, kGramLiveBound);
    m.d.chunk_max = 100;
    m.d.utt_frames = 1000;
    OnePassLivePlan pl;
    std::string why;
    CHECK(onepass_gram_live_plan(m, 15, 0, nullptr, 10, &pl, &why) && pl.block == 15 && pl.n_blocks == 1 && pl.d.rows == 2);
    CHECK(onepass_gram_live_plan(m, 0, 0, nullptr, 100, &pl, &why) && pl.block == 100 && pl.n_blocks == 1);  // no valid slot
    CHECK(onepass_gram_live_plan(m, 0, 3, nullptr, 0, &pl, &why) && pl.block == 1 && pl.n_blocks == 0 && pl.d.rows == 0);
    CHECK(onepass_gram_live_plan(m, 15, 4, nullptr, 100, &pl, &why) && pl.block == 4 && pl.n_blocks == 25);
    CHECK(onepass_gram_live_plan(m, 15, 99, nullptr, 100, &pl, &why) && pl.block == 15 && pl.n_blocks == 7);
    CHECK(!onepass_gram_live_plan(m, 15, 0, nullptr, 101, &pl, &why) && has(why, "chunk_max"));
    // the bound is the batch decoder's, on utt_frames: 1000 / 15 = 66 words
    const uint32_t at = (1u << 30) / 66;
    CHECK(onepass_gram_cost_ok(1000, 15, at, 0, 0) && !onepass_gram_cost_ok(1000, 15, at + 1, 0, 0));
    CHECK(onepass_gram_cost_ok(1000, 15, at - 5, 5, (1u << 30) - 66 * at) && !onepass_gram_cost_ok(1000, 15, at - 5, 5, (1u << 30) - 66 * at + 1));
    CHECK(gram_live_all_empty(m.d, &why));
    sr_chain_live_row out[2];
    const uint32_t one[2] = {0, 7};
    CHECK(onepass_gram_live_plan(m, 5, 0, one, 0, &pl, &why) && pl.d.rows == 1 && pl.n_blocks == 2);
    onepass_live_advance(m, pl, out, nullptr);
    CHECK(m.c0_prev[1] == 5 && m.d.frames[1] == 7 && out[0].channel == 1 && out[0].frames == 7);
    CHECK(!gram_live_all_empty(m.d, &why) && has(why, "channel 1"));
    CHECK(gram_live_stale(3, 4, 5, 4, &why) && has(why, "store") && gram_live_stale(3, 4, 3, 5, &why) && has(why, "word map"));
    CHECK(!gram_live_stale(3, 4, 3, 4, &why));
    return 0;
}

// PCM sessions: the blocks are cut from the frames a push completes, not from its samples
static int pcm_blocks()
{
    OnePassLiveMirror m;
    m.open(2, kGramLiveBound);
    m.d.pcm = true;
    m.d.frame_len = 160;
    m.d.hop = 80;
    m.d.chunk_max = 800;
    m.d.utt_frames = 50;
    OnePassLivePlan pl;
    std::string why;
    sr_chain_live_row out[2];
    const uint32_t a[2] = {161 + 80 * 6, 100};  // 7 frames, none
    CHECK(onepass_gram_live_plan(m, 3, 0, a, 0, &pl, &why) && pl.d.rows == 2 && pl.d.max_frames == 7 && pl.n_blocks == 3);
    CHECK(pl.d.chan[0].n == 7 && pl.d.chan[1].n == 0 && pl.d.chan[1].first_win == 1);
    onepass_live_advance(m, pl, out, nullptr);
    CHECK(m.c0_prev[0] == 6 && m.c0_prev[1] == 0 && m.d.frames[0] == 7);
    const uint32_t b[2] = {10, 10};  // samples, but no new frame: rows, no block
    CHECK(onepass_gram_live_plan(m, 3, 0, b, 0, &pl, &why) && pl.d.rows == 2 && pl.n_blocks == 0);
    CHECK(onepass_gram_live_push_launches(pl.n_blocks, 4, 2) == 1);
    onepass_live_advance(m, pl, out, nullptr);
    CHECK(m.c0_prev[0] == 6 && out[0].frames == 7 && out[1].frames == 0);
    CHECK(!gram_live_all_empty(m.d, &why));  // kept samples count as a recording
    return 0;
}

int main()
{
    if (state_bytes() || launches() || block_walk() || bound_free_plan_and_grammar_rules() || pcm_blocks()) return 1;
    std::printf("plan_check ok\n");
    return 0;
}
