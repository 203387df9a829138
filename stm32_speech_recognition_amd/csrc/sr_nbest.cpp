// Word-level N-best (include/sr_engine.h, "words instead of slots"): the slot -> word map of an engine, the grouping of the
// store's slots under it that k_nbest.hip reads, and the stage-level entry points.  The whole-path and stream forms launch the
// same kernel from sr_launch.cpp / sr_host.cpp / sr_stream.cpp.
#include "sr_host_call.h"

#include <unordered_map>

using namespace sr;

// slots grouped by word: ascending slot inside a word, words by their first slot (a counting sort over dense word indices)
static int word_groups(const uint32_t *word_of_slot, uint32_t n_slots, uint32_t spw, std::vector<uint32_t> &order,
                       std::vector<uint32_t> &start, std::vector<uint32_t> &ids)
{
    if (!n_slots) return fail(SR_ERR_BAD_ARG, "word map: no slots");
    if (!word_of_slot && !spw) return fail(SR_ERR_BAD_ARG, "word map: slots_per_word must be at least 1");
    std::vector<uint32_t> dense(n_slots);
    ids.clear();
    if (word_of_slot) {
        std::unordered_map<uint32_t, uint32_t> index;
        for (uint32_t k = 0; k < n_slots; k++) {
            if (word_of_slot[k] == SR_NO_WORD) return fail(SR_ERR_BAD_ARG, "word map: slot " + std::to_string(k) + " carries SR_NO_WORD");
            const auto it = index.emplace(word_of_slot[k], (uint32_t)ids.size());
            if (it.second) ids.push_back(word_of_slot[k]);
            dense[k] = it.first->second;
        }
    } else {
        for (uint32_t k = 0; k < n_slots; k++) dense[k] = k / spw;  // main.c:292
        ids.resize((n_slots - 1) / spw + 1);
        for (uint32_t w = 0; w < ids.size(); w++) ids[w] = w;
    }
    start.assign(ids.size() + 1, 0);
    for (uint32_t k = 0; k < n_slots; k++) start[dense[k] + 1]++;
    for (size_t w = 0; w < ids.size(); w++) start[w + 1] += start[w];
    std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    order.resize(n_slots);
    for (uint32_t k = 0; k < n_slots; k++) order[fill[dense[k]]++] = k;
    return SR_OK;
}

// The grouping of the CURRENT store under the current map, uploaded.  Called when either changes (sr_set_word_map, the
// template-store setters), so that no N-best call has to build or copy anything; built in a fresh buffer after the device has
// drained, because a kernel of an earlier asynchronous call may still be reading the previous one.  A map with labels for
// another number of slots leaves the engine without a grouping: N-best calls then fail until map and store agree.
int regroup_words(sr_engine *h, bool drained)
{
    h->wg_K = 0;
    h->wg_words = 0;
    h->word_serial++;
    if (!h->K || (h->word_explicit && h->word_labels.size() != h->K)) return SR_OK;
    std::vector<uint32_t> order, start, ids;
    if (int rc = word_groups(h->word_explicit ? h->word_labels.data() : nullptr, h->K, h->word_spw, order, start, ids)) return rc;
    std::vector<uint32_t> tab(order);
    tab.insert(tab.end(), start.begin(), start.end());
    tab.insert(tab.end(), ids.begin(), ids.end());
    std::vector<uint32_t> group_of(h->K);  // the rescoring mark pass goes from a slot to its word group
    for (uint32_t w = 0; w + 1 < start.size(); w++)
        for (uint32_t p = start[w]; p < start[w + 1]; p++) group_of[order[p]] = w;
    tab.insert(tab.end(), group_of.begin(), group_of.end());
    ENTER_DEVICE(h);
    if (!drained) HIP_TRY(hipDeviceSynchronize());
    DevBuf<uint32_t> fresh;
    if (int rc = fresh.reserve(tab.size())) return rc;
    const hipError_t e = hipMemcpy(fresh.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        fresh.release();
        return fail(SR_ERR_HIP, std::string("word grouping upload: ") + hipGetErrorString(e));
    }
    std::swap(h->wg_tab, fresh);
    fresh.release();
    h->wg_K = h->K;
    h->wg_words = (uint32_t)ids.size();
    return SR_OK;
}

int check_nbest(const sr_engine *h, uint32_t n_best, const void *nbest)
{
    if (!nbest) return fail(SR_ERR_BAD_ARG, "null N-best output");
    if (n_best < 1 || n_best > SR_NBEST_MAX) return fail(SR_ERR_BAD_ARG, "n_best must be 1.." + std::to_string(SR_NBEST_MAX));
    if (!h->K) return fail(SR_ERR_NO_TEMPLATES, "no templates set");
    if (h->wg_K != h->K)
        return fail(SR_ERR_BAD_ARG, h->word_explicit && h->word_labels.size() != h->K
                                        ? "the word map has " + std::to_string(h->word_labels.size()) + " slots, the template store " +
                                              std::to_string(h->K)
                                        : std::string("no word grouping for this store (its upload failed): set the word map again"));
    return SR_OK;
}

// rows [row0, row0 + n_rows) of an N-best output, for the score rows at d_scores
NbestArgs nbest_args(const sr_engine *h, const uint32_t *d_scores, uint32_t n_rows, const NbestOut &nb, size_t row0)
{
    const uint32_t *t = h->wg_tab.p;
    return NbestArgs{d_scores, n_rows, h->K, h->wg_words, nb.n_best, t, t + h->K, t + h->K + h->wg_words + 1,
                     nb.out + row0 * nb.n_best, nb.n_matched ? nb.n_matched + row0 : nullptr};
}

extern "C" {

int sr_word_groups(const uint32_t *word_of_slot, uint32_t n_slots, uint32_t slots_per_word, uint32_t *order, uint32_t *group_start,
                   uint32_t *word_id, uint32_t *n_words)
{
    std::vector<uint32_t> o, s, w;
    if (int rc = word_groups(word_of_slot, n_slots, slots_per_word, o, s, w)) return rc;
    if (order) std::memcpy(order, o.data(), o.size() * 4);
    if (group_start) std::memcpy(group_start, s.data(), s.size() * 4);
    if (word_id) std::memcpy(word_id, w.data(), w.size() * 4);
    if (n_words) *n_words = (uint32_t)w.size();
    return SR_OK;
}

int sr_set_word_map(sr_engine *h, const uint32_t *word_of_slot, uint32_t n_slots, uint32_t slots_per_word)
{
    if (!h) return fail(SR_ERR_BAD_ARG, "null engine");
    if (word_of_slot) {
        if (!n_slots) return fail(SR_ERR_BAD_ARG, "word map: no slots");
        for (uint32_t k = 0; k < n_slots; k++)
            if (word_of_slot[k] == SR_NO_WORD) return fail(SR_ERR_BAD_ARG, "word map: slot " + std::to_string(k) + " carries SR_NO_WORD");
        h->word_labels.assign(word_of_slot, word_of_slot + n_slots);
    } else {
        if (!slots_per_word) return fail(SR_ERR_BAD_ARG, "word map: slots_per_word must be at least 1");
        h->word_labels.clear();
        h->word_spw = slots_per_word;
    }
    h->word_explicit = word_of_slot != nullptr;
    return regroup_words(h, false);
}

int sr_nbest_batch_dev(sr_engine *h, const uint32_t *d_scores, uint32_t n_rows, uint32_t n_best, sr_nbest_entry *d_nbest,
                       uint32_t *d_n_matched, void *stream)
{
    if (!h || !d_scores) return fail(SR_ERR_BAD_ARG, "null argument");
    if (int rc = check_nbest(h, n_best, d_nbest)) return rc;
    if (n_rows > 0xFFFFFFF0u) return fail(SR_ERR_BAD_ARG, "too many rows");
    ENTER_DEVICE(h);
    launch_nbest(nbest_args(h, d_scores, n_rows, NbestOut{n_best, d_nbest, d_n_matched}, 0), (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

int sr_nbest_batch(sr_engine *h, const uint32_t *scores, uint32_t n_rows, uint32_t n_best, sr_nbest_entry *nbest, uint32_t *n_matched)
{
    if (!h || !scores) return fail(SR_ERR_BAD_ARG, "null argument");
    if (int rc = check_nbest(h, n_best, nbest)) return rc;
    if (n_rows > 0xFFFFFFF0u) return fail(SR_ERR_BAD_ARG, "too many rows");
    if (!n_rows) return SR_OK;
    ENTER_HOST_CALL(h);
    int rc;
    if ((rc = h->s_scores.reserve((size_t)n_rows * h->K))) return rc;
    if ((rc = h->s_nbest.reserve((size_t)n_rows * n_best))) return rc;
    if ((rc = h->s_nmatched.reserve(n_rows))) return rc;
    COPY_UP(h->s_scores.p, scores, (size_t)n_rows * h->K * 4);
    launch_nbest(nbest_args(h, h->s_scores.p, n_rows, NbestOut{n_best, h->s_nbest.p, h->s_nmatched.p}, 0), nullptr);
    HIP_TRY(hipGetLastError());
    COPY_DOWN(nbest, h->s_nbest.p, (size_t)n_rows * n_best * sizeof(sr_nbest_entry));
    if (n_matched) COPY_DOWN(n_matched, h->s_nmatched.p, (size_t)n_rows * 4);
    return SR_OK;
}

}  // extern "C"
