// sr_forced_plan.h -- host-side planning of the transcript-forced alignment and of the span gather (include/sr_engine.h,
// "forced alignment against a transcript"; sr_forced.cpp): the store under the word map, every check on the host arrays, the
// per-level item lists, minlen and tail of the exact column pruning, and the launch groups.  HOST ONLY and free of HIP, so that
// tests/forced_plan/plan_check.cpp can run it under the sanitizers on a machine without a device.
//
// An ITEM of level l is one word pass of k_forced_words: (row, slot) for a row whose transcript has at least l words and a
// VALID slot of the word at position l - 1.  The items are listed group by group (a launch group is a run of rows whose scratch
// fits), inside a group level by level, inside a level by ascending (row, slot): a launch takes one contiguous run.
#pragma once
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "sr_overlap.h"  // overlap(): the buffer checks of sr_forced.cpp, exercised by plan_check.cpp with the rest

namespace sr {

constexpr uint32_t kForcedMaxWords = 16;          // words of one transcript at most (= the decoder's levels)
constexpr uint32_t kForcedNone = 0xFFFFFFFFu;     // "not wanted" in dst_of_span, "no span" in the gather's table

// The store under the word map.  Words are numbered by their first slot, as sr_word_groups numbers them.
struct ForcedStore {
    std::unordered_map<uint32_t, uint32_t> index;  // label -> word
    std::vector<uint32_t> start;                   // [words + 1]: the VALID slots of word w are slots[start[w] .. start[w + 1]), ascending
    std::vector<uint32_t> slots;
    std::vector<uint32_t> minlen;                  // [words]: min over the valid slots of M / 2 + 1 frames; 0 = no valid slot
};

// label[K] = the word map; tpl_len[K] = the frames of a valid slot, 0 for an invalid one (an empty template is invalid)
inline ForcedStore forced_store(const uint32_t *label, const uint32_t *tpl_len, uint32_t K)
{
    ForcedStore s;
    std::vector<uint32_t> word_of(K);
    for (uint32_t k = 0; k < K; k++) word_of[k] = s.index.emplace(label[k], (uint32_t)s.index.size()).first->second;
    const uint32_t n_words = (uint32_t)s.index.size();
    s.start.assign((size_t)n_words + 1, 0u);
    s.minlen.assign(n_words, 0u);
    for (uint32_t k = 0; k < K; k++)
        if (tpl_len[k]) s.start[word_of[k] + 1]++;
    for (uint32_t w = 0; w < n_words; w++) s.start[w + 1] += s.start[w];
    std::vector<uint32_t> fill(s.start.begin(), s.start.end() - 1);
    s.slots.resize(s.start[n_words]);
    for (uint32_t k = 0; k < K; k++) {
        if (!tpl_len[k]) continue;
        const uint32_t w = word_of[k], reach = tpl_len[k] / 2u + 1u;  // the span section's reach rule: M rows need M / 2 + 1 frames
        s.slots[fill[w]++] = k;
        s.minlen[w] = s.minlen[w] && s.minlen[w] < reach ? s.minlen[w] : reach;
    }
    return s;
}

// what sr_align_transcripts_dp checks on its two host arrays; false: *why says what is wrong
inline bool forced_check(const ForcedStore &s, const uint32_t *transcript, const uint32_t *n_words, uint32_t n_rows, uint32_t words_per_row,
                         std::string *why)
{
    if (words_per_row < 1 || words_per_row > kForcedMaxWords) {
        *why = "words_per_row must be 1..16";
        return false;
    }
    if (n_rows && (!transcript || !n_words)) {
        *why = "null argument";
        return false;
    }
    for (uint32_t r = 0; r < n_rows; r++) {
        if (n_words[r] > words_per_row) {
            *why = "row " + std::to_string(r) + " has " + std::to_string(n_words[r]) + " words, words_per_row is " + std::to_string(words_per_row);
            return false;
        }
        for (uint32_t i = 0; i < n_words[r]; i++) {
            const uint32_t lab = transcript[(size_t)r * words_per_row + i];
            if (!s.index.count(lab)) {
                *why = "row " + std::to_string(r) + ", position " + std::to_string(i) + ": no slot of the word map carries the label " + std::to_string(lab);
                return false;
            }
        }
    }
    return true;
}

// the buffer checks' overlap test under the name this header has always had for it: the one function of sr_overlap.h
inline constexpr auto &forced_overlap = overlap;

struct ForcedGroup {
    uint32_t row0, n_rows;
    uint32_t levels;                       // the longest transcript of the group: levels above it are never read
    uint32_t item0[kForcedMaxWords + 1];   // level l = 1..levels takes the items [item0[l - 1], item0[l]) of the call's list
};
struct ForcedPlan {
    uint32_t n_rows = 0, W = 0, n_items = 0;
    std::vector<uint32_t> tab;             // what goes to the device: tail[n_rows][W] | count[n_rows] | items[n_items][2] = (row, slot)
    std::vector<ForcedGroup> groups;
    size_t count_at() const { return (size_t)n_rows * W; }
    size_t items_at() const { return (size_t)n_rows * W + n_rows; }
};

// arrays that passed forced_check.  rows_per_group >= 1.  tail[r][l - 1] = the sum of minlen over the positions after l (0 with
// prune off, and at and above the row's count): level l of row r needs the end frames e with e + 1 <= N - tail only.
inline ForcedPlan forced_plan(const ForcedStore &s, const uint32_t *transcript, const uint32_t *n_words, uint32_t n_rows, uint32_t words_per_row,
                              uint32_t rows_per_group, bool prune)
{
    ForcedPlan p;
    p.n_rows = n_rows;
    p.W = words_per_row;
    p.tab.assign(p.items_at(), 0u);
    for (uint32_t r = 0; r < n_rows; r++) {
        const uint32_t *t = transcript + (size_t)r * words_per_row;
        p.tab[p.count_at() + r] = n_words[r];
        uint32_t tail = 0;
        for (uint32_t l = n_words[r]; l >= 1; l--) {  // level l: the words at positions l .. n - 1 are still to come
            p.tab[(size_t)r * words_per_row + l - 1] = prune ? tail : 0u;
            tail += s.minlen[s.index.at(t[l - 1])];
        }
    }
    if (!rows_per_group) rows_per_group = 1;
    for (uint32_t r0 = 0; r0 < n_rows; r0 += rows_per_group) {
        ForcedGroup g{};
        g.row0 = r0;
        g.n_rows = n_rows - r0 < rows_per_group ? n_rows - r0 : rows_per_group;
        for (uint32_t r = r0; r < r0 + g.n_rows; r++) g.levels = n_words[r] > g.levels ? n_words[r] : g.levels;
        for (uint32_t l = 1; l <= kForcedMaxWords; l++) {
            g.item0[l - 1] = p.n_items;
            if (l > g.levels) continue;
            for (uint32_t r = r0; r < r0 + g.n_rows; r++) {
                if (n_words[r] < l) continue;
                const uint32_t w = s.index.at(transcript[(size_t)r * words_per_row + l - 1]);
                for (uint32_t i = s.start[w]; i < s.start[w + 1]; i++) {
                    p.tab.push_back(r);
                    p.tab.push_back(s.slots[i]);
                    p.n_items++;
                }
            }
        }
        g.item0[kForcedMaxWords] = p.n_items;
        p.groups.push_back(g);
    }
    return p;
}

// sr_gather_word_spans: dst_of_span[n_spans] -> src_of_ex[n_ex] (the span that fills example e, kForcedNone: none).  false:
// an index at or above n_ex, or one that two spans name; *why says which
inline bool forced_gather_table(const uint32_t *dst_of_span, size_t n_spans, uint32_t n_ex, std::vector<uint32_t> *src_of_ex, std::string *why)
{
    src_of_ex->assign(n_ex, kForcedNone);
    for (size_t i = 0; i < n_spans; i++) {
        const uint32_t e = dst_of_span[i];
        if (e == kForcedNone) continue;
        if (e >= n_ex) {
            *why = "dst_of_span[" + std::to_string(i) + "] = " + std::to_string(e) + " is not below n_ex = " + std::to_string(n_ex);
            return false;
        }
        if ((*src_of_ex)[e] != kForcedNone) {
            *why = "dst_of_span[" + std::to_string(i) + "] and dst_of_span[" + std::to_string((*src_of_ex)[e]) + "] name the same example " + std::to_string(e);
            return false;
        }
        (*src_of_ex)[e] = (uint32_t)i;
    }
    return true;
}

}  // namespace sr
