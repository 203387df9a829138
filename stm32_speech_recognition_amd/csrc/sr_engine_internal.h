// Shared by the host translation units of the library (sr_engine.cpp: lifecycle, template store, settings;
// sr_launch.cpp: the device-resident entry points and kernel sequencing; sr_host.cpp: host-buffer entry points and
// diagnostics, whose transport is sr_host_call.h): the engine handle, device-memory / device-selection helpers and the
// launch-argument builders.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "sr_device.h"
#include "sr_dtw_plan.h"
#include "sr_gram_compile.h"
#include "sr_tables.h"

namespace sr {

int set_error(int code, const std::string &msg);  // records the message sr_last_error() returns (thread-local), returns code
static inline int fail(int code, const std::string &msg) { return set_error(code, msg); }

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(SR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                \
    } while (0)


// Every entry point runs on the engine's device and puts the caller's current device back afterwards (a
// single-process multi-GPU caller -- or PyTorch on another ordinal -- keeps its own current device).
struct DeviceGuard {
    int prev = -1;
    bool restore = false;
    int enter(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        hipError_t e = hipSetDevice(dev);
        if (e != hipSuccess) return fail(SR_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
        restore = prev >= 0 && prev != dev;
        return SR_OK;
    }
    ~DeviceGuard()
    {
        if (restore) (void)hipSetDevice(prev);
    }
};
#define ENTER_DEVICE(h)                      \
    DeviceGuard dev_guard_;                  \
    do {                                     \
        int rc_dev_ = dev_guard_.enter((h)->device); \
        if (rc_dev_) return rc_dev_;         \
    } while (0)

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    int reserve(size_t count)
    {
        if (count <= n) return SR_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e != hipSuccess) return fail(SR_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        n = count;
        return SR_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

// a DevBuf that lives for one call: freed on every return path
template <typename T>
struct TmpDevBuf : DevBuf<T> {
    TmpDevBuf() = default;
    TmpDevBuf(const TmpDevBuf &) = delete;
    ~TmpDevBuf() { this->release(); }
};

}  // namespace sr

using namespace sr;  // internal header of three host units of one library: the handle below is a global C type built from sr:: parts

// launch sizes below which VAD / the frame kernel take their small-launch forms (captures; work items of 64 frames)
static constexpr uint32_t kVadWideBelow = 1024, kMfccFill = 1024;  // measured crossover ~2 000 captures; work items that fill 256 CUs x 4 (RESULTS.md)
// utterances of one call whose slot scan k_dtw_cells can do itself (one counter each); beyond that k_argmin runs as usual
static constexpr uint32_t kPairCounters = 65536;

struct sr_engine {
    sr_config cfg;
    int device = 0;
    uint32_t noise_len = 0, atap_frm = 0;
    uint32_t n_cu = 256;  // compute units of the engine's device (sr_create)
    LdsBudget lds;        // its LDS (sr_create): every DTW launch shape is planned from these figures, not MI355X's
    const uint16_t *dev_mag_q = nullptr;  // QUIET-tier magnitude table inside table_blob (kMagTabEntries x u16, its own 256-byte-aligned part)
    uint32_t mag_cheap_max = 0;  // kMagCheapMax once the device sweep at sr_create has confirmed the cheap magnitude form on this chip, else 0
    uint32_t mfcc_tile = 64, mfcc_tile_mid = 64, mfcc_tile_small = 64, mfcc_grid_cap = 0;  // frames per k_mfcc work item (batch form / the two forms for underfilled launches), resident workgroups
    uint32_t frame_len = 160, hop = 80;          // 160/80 reference, 320/160 extension, or the generic front end's framing
    uint32_t nc = 12, n_mel = 24;                // s16 per feature row (n_coef), Mel filters
    size_t mfcc_elems(size_t B) const { return B * cfg.max_frames * nc; }  // s16 in the feature records of B utterances
    bool generic = false;                        // GENERIC front end (k_mfcc_gen; k_dtw_lds's 16-wide form when nc > 12)
    uint32_t v_durmin = 8, s_durmax = 11;        // VAD.C:72-75 in frames
    HostTables host;
    DevTables dev{};
    void *table_blob = nullptr;
    // template store, dense layout in HBM
    DevBuf<int16_t> tpl;
    DevBuf<uint32_t> tpl_frames;
    DevBuf<uint8_t> tpl_valid;
    bool tpl_staged_ok = true;     // every coefficient of the store fits the -2*coef rows of tplR
    DevBuf<uint32_t> tplR;         // [rows][K] 32-byte rows (12 x s16 | norm | pad), templates ordered by length
    DevBuf<uint32_t> tpl_frames_s, tpl_orig;
    DevBuf<uint32_t> tpl_rank;     // [K] rank of each slot in that order (the inverse of tpl_orig): the sparse full-DP scorer's marks
    uint32_t K = 0, tpl_rows = 0, tpl_stride = 0;
    uint64_t store_serial = 0;     // bumped by every template upload: what a live spotting session's state was shaped by (sr_spot_live.cpp)
    DtwPlan plan;                  // which DTW kernel serves this store, in what shape (plan_dtw, when the store is set)
    uint32_t dp_lanes = 0;         // sr_set_dp_lanes: lanes per pair of the opt-in full-DP scorer (0 = default)
    std::vector<uint32_t> cells_by_len;  // most band points per template length, computed once (dtw_cells_max_points)
    int small_launch = 0;          // sr_set_small_launch: 0 = automatic (k_dtw_cells for a few hundred pairs, k_dtw_quad up to two rounds of the chip), 1 = never, 2 / 3 = k_dtw_cells / k_dtw_quad whenever it fits
    // scratch used when the caller does not ask for an intermediate (or passes host buffers)
    DevBuf<uint16_t> s_pcm;
    DevBuf<uint8_t> s_pack;   // sr_recognize_batch_packed12: the packed rows as uploaded, before k_unpack12
    DevBuf<sr_vad_rec> s_vad;
    DevBuf<int16_t> s_mfcc;
    DevBuf<uint32_t> s_scores;
    DevBuf<sr_result> s_results;
    DevBuf<uint32_t> s_u32a, s_u32b;
    DevBuf<sr_atap> s_atap;
    DevBuf<sr_vad_rec> s_vad2;
    // stream recognition (sr_stream.cpp): thresholds, tile tables, loud masks, tile entry states, per-chunk rows / records,
    // and the host form's device copies of its outputs
    DevBuf<sr_vad_rec> s_st_vad;
    DevBuf<uint64_t> s_st_tab;
    DevBuf<uint32_t> s_st_mask;
    DevBuf<uint4> s_st_tin;
    DevBuf<sr_atap> s_st_atap;
    DevBuf<uint16_t> s_st_rows;
    DevBuf<sr_vad_rec> s_st_recs;
    DevBuf<sr_stream_seg> s_st_segs;
    DevBuf<uint32_t> s_st_off;
    DevBuf<uint32_t> s_pcnt;  // k_dtw_cells: finished-pair counters per utterance of a call, zero between launches (kPairCounters)
    // The counters are hidden per-engine state shared by every launch: two small calls in flight on DIFFERENT caller streams
    // would both count in them.  They therefore belong to one caller stream at a time (internal chunk streams are forked from /
    // joined to it, so its order covers them); a call on any other stream leaves the slot scan to k_argmin -- unless the last
    // call that used the counters has COMPLETED: ev_cells is recorded on that call's caller-level stream after its join, so it
    // covers every chunk, and once it has completed nothing counts in them and the calling stream becomes the owner.
    hipStream_t cells_owner = nullptr;
    bool cells_owner_set = false;
    hipEvent_t ev_cells = nullptr;  // created with s_pcnt (sr_create)
    // An asynchronous *_dev call that was handed no buffer for an intermediate uses the engine's scratch (s_vad, s_mfcc,
    // s_scores, s_vad2) on the CALLER's stream.  The event marks the end of the last such call; the host-buffer entry points,
    // which reuse the same scratch on internal or the null stream, order their stream behind it first (order_after_scratch_users).
    hipEvent_t ev_scratch = nullptr;
    bool scratch_pending = false;
    // host-buffer pipeline (sr_recognize_batch): upload of chunk c+1 overlaps the kernels of chunk c
    hipStream_t st_copy = nullptr, st_comp = nullptr;
    // small host-buffer calls (spch_recg: one capture), HostCall's pinned mode in sr_host_call.h: one mapped pinned area of
    // kPinTotal bytes -- staging for what goes up, then the part results land in (written by the kernel itself or by
    // asynchronous copies), all on st_comp: one stream synchronisation per call instead of a blocking copy each way.
    // Allocated on the first small call (ensure_pin); pin_failed = the host refused it, every call stays blocking
    void *pin_buf = nullptr;
    size_t pin_cap = 0;
    bool pin_failed = false;
    std::vector<hipEvent_t> ev_chunk;
    // device-resident pipeline (sr_recognize_batch_dev): the batch is cut into chunks that run on a few internal
    // streams, forked from and joined back to the caller's stream, so that the kernels of different chunks overlap
    // (k_vad / k_dtw_lds waves fill the issue slots k_mfcc leaves idle: 32.0 -> 28.2 ms per 65 536 utterances)
    static constexpr uint32_t kPipeStreams = 4;
    hipStream_t st_pipe[kPipeStreams] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[kPipeStreams] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t pipe_streams = 3;             // sr_set_pipeline streams (1 = one chunk on the caller's stream); measured: 2 -> 28.8,
                                           // 3 -> 28.2, 4 -> 30.0 ms per 65 536 utterances (1 -> 32.0)
    uint32_t pipe_min_chunk = 4096;        // sr_set_pipeline min_chunk: utterances per chunk at least (smaller chunks lose more than they gain:
                                           // 4 096 x 10 as two chunks of 2 048: 1.93 ms per step, as one chunk 1.63)
    uint32_t pipe_max_chunks = 12;         // chunks per call at most (sr_set_pipeline); one per stream for large stores, see upload_templates
    bool pipe_user_set = false;            // sr_set_pipeline was called: the engine no longer adapts the chunk count to the store
    // profiling (sr_set_profiling / sr_get_stage_ms): events recorded since profiling was switched on
    bool profiling = false;
    std::vector<hipEvent_t> ev;  // 5 per kernel group (chunk): before VAD, MFCC, DTW, argmin, after argmin
    size_t ev_used = 0;          // groups recorded
    std::vector<hipEvent_t> ev_call;  // 2 per call on the caller's stream: before the fork, after the join
    size_t calls_used = 0;
    // word-level N-best (sr_nbest.cpp): the map as the caller set it, and the grouping of the current store's slots under it
    std::vector<uint32_t> word_labels;  // sr_set_word_map with labels (word_explicit); else word = slot / word_spw
    bool word_explicit = false;
    uint32_t word_spw = 1;
    DevBuf<uint32_t> wg_tab;            // order[K] | group_start[n_words + 1] | word_id[n_words] (sr_word_groups) | group_of_slot[K]
    uint32_t wg_K = 0, wg_words = 0;    // the store size the grouping was built for (0: none, or a map of another length)
    uint64_t word_serial = 0;           // bumped whenever the grouping is rebuilt (a new map or a new store): what a grammar was compiled against (sr_gram.cpp)
    DevBuf<sr_nbest_entry> s_nbest;     // host-buffer forms: device copies of their N-best outputs
    DevBuf<uint32_t> s_nmatched;
    // two-pass rescoring (sr_rescore.cpp): the pair marks [chunk][K ranks][mark stride] and the second-pass score rows [rows][K]
    // of a call (its own matrix: s_scores may hold the first pass), the first-pass lists of a whole-path call that was handed no
    // buffer for them, and the host-buffer forms' device copies of their outputs
    DevBuf<uint8_t> s_rs_marks;
    DevBuf<uint32_t> s_rs_scores;
    DevBuf<sr_nbest_entry> s_rs_first, s_rs_out;
    DevBuf<uint32_t> s_rs_n;
    // word spotting (sr_spot.cpp): the partial records of a call whose windows are longer than a kernel chunk, and the
    // host-buffer forms' device copies of their outputs
    DevBuf<sr_spot_hit> s_spot_part, s_spot_hits;
    DevBuf<uint32_t> s_spot_scores;
    // full-DP alignment and DBA training (sr_align.cpp): the predecessor marks of one launch when they do not fit the LDS; a
    // training call's per-launch spans and records, its example -> model map, accumulators and intermediate centroid set
    DevBuf<uint32_t> s_al_marks, s_al_span, s_al_map, s_al_cnt;
    DevBuf<sr_align_rec> s_al_rec;
    DevBuf<int32_t> s_al_sum;
    DevBuf<int16_t> s_al_cen;
    // connected-word decoding (sr_chain.cpp): the keys and prefix costs of one launch group
    DevBuf<unsigned long long> s_ch_a;
    DevBuf<uint32_t> s_ch_e;
    // word alternatives (sr_span.cpp): the span score rows of a call that was handed no buffer for them, and the host-buffer
    // forms' device copies of their word rows
    DevBuf<uint32_t> s_span_scores;
    DevBuf<sr_chain_word> s_span_words;
    // word-model clustering (sr_cluster.cpp): the plan's tables (each example's model range, the score pass's workgroups), the
    // score and accumulated-cost rows [E][16], the assignment maps of the previous and the current iteration [2][E], and one
    // iteration's statistics when the caller asked for the iteration records only
    DevBuf<uint32_t> s_cl_tab, s_cl_dis, s_cl_acc, s_cl_map;
    DevBuf<sr_train_stat> s_cl_stat;
    // transcript-forced alignment and the span gather (sr_forced.cpp): the rows a valid slot holds (0: an invalid slot), kept on
    // the host with every store, so that a call can plan without reading the store back; the plan's tables of a call in flight
    std::vector<uint32_t> tpl_len_host;
    DevBuf<uint32_t> s_fc_tab, s_fc_src;
    // one-pass connected-word decoding (sr_onepass.cpp): the saved columns of one launch group (its keys and prefix costs are
    // s_ch_a / s_ch_e)
    DevBuf<ulonglong2> s_op_cols;
};

// what an N-best form adds to the call it extends (device pointers); nullptr where the plain call is meant
struct NbestOut {
    uint32_t n_best;
    sr_nbest_entry *out;
    uint32_t *n_matched;  // optional
};

// ---- helpers shared by the launch and the host-buffer units (sr_launch.cpp) --------------------------------------
int check_batch(const sr_engine *h, uint32_t B);
int check_pcm(const sr_engine *h, const uint16_t *pcm, uint64_t stride, uint32_t buf_len);
int mark_scratch_user(sr_engine *h, hipStream_t s);
int order_after_scratch_users(sr_engine *h, hipStream_t s);
VadArgs vad_args(const sr_engine *h, const uint16_t *pcm, uint64_t stride, uint32_t buf_len, uint32_t noise_len, uint32_t B,
                     sr_vad_rec *vad, const sr_atap *atap_in = nullptr, uint64_t *dbg = nullptr);
MfccArgs mfcc_args(const sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t B, const sr_vad_rec *d_vad, int16_t *d_mfcc);
MfccMagTab mfcc_mag_tab(const sr_engine *h);  // what launch_mfcc / launch_mfcc_features take next to it
DtwArgs dtw_args(const sr_engine *h, const int16_t *d_mfcc, const sr_vad_rec *d_vad, const uint32_t *d_in_frames, uint32_t B,
                     uint32_t *d_scores, sr_result *d_results);
void plan_dtw(sr_engine *h, const uint32_t *frames, const uint8_t *valid);
bool launch_dtw_auto(sr_engine *h, DtwArgs &a, uint32_t b0, hipStream_t s, hipStream_t owner);
// ---- live sessions (sr_live.cpp) -------------------------------------------------------------------------------------------
namespace sr {
struct ConfigFraming {
    uint32_t frame_len, hop, v_durmin, s_durmax, noise_len, max_frames;
};
int config_framing(const sr_config *cfg, ConfigFraming *out);  // sr_engine.cpp: host-only, sr_create's checks and figures
}  // namespace sr
// ---- word-level N-best (sr_nbest.cpp) -----------------------------------------------------------------------------------
// (re)build and upload the grouping for the current store and map; waits for the device unless the caller has (`drained`)
int regroup_words(sr_engine *h, bool drained);
int check_nbest(const sr_engine *h, uint32_t n_best, const void *nbest);  // n_best range, non-null output, a grouping for this store
NbestArgs nbest_args(const sr_engine *h, const uint32_t *d_scores, uint32_t n_rows, const NbestOut &nb, size_t row0);
// ---- two-pass rescoring (sr_rescore.cpp) ----------------------------------------------------------------------------------
// what a rescoring form adds to the N-best call it extends (device pointers)
struct RescoreOut {
    sr_nbest_entry *out;   // [rows][n_best]
    uint32_t *n_rescored;  // optional
};
static constexpr uint32_t kRescoreMaxRows = 65535u * 256u;  // rows of one rescoring: the sparse scorer's grid (256 rows per workgroup at least)
static inline uint32_t rescore_mark_stride(uint32_t n_rows) { return (n_rows + 15u) & ~15u; }  // bytes of marks per template
// check_nbest's rules for `out` + the conditions of sr_dtw_dp_batch_dev
int check_rescore(const sr_engine *h, uint32_t n_best, const void *out);
// room for `n_chunks` concurrent rescorings of at most `per` rows each, n_rows rows in all
int reserve_rescore(sr_engine *h, uint32_t n_chunks, uint32_t per, size_t n_rows);
// the second pass of rows [row0, row0 + n) of a call as chunk `chunk` of reserve_rescore's layout, enqueued on s: d_mfcc /
// d_frames / in / out / n_rescored point at the CALL's first row
int launch_rescore(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_frames, uint32_t frames_stride, uint32_t n_best,
                   const sr_nbest_entry *in, const RescoreOut &out, uint32_t chunk, uint32_t per, size_t row0, uint32_t n, hipStream_t s);
// ---- word spotting (sr_spot.cpp) --------------------------------------------------------------------------------------------
// the conditions of sr_spot_dp_batch_dev on the engine and the store, and how a call of n_rows rows is cut into chunks
int check_spot(const sr_engine *h, uint32_t n_rows, uint32_t win_frames, SpotGeom *g);
// the stage over n_rows rows, enqueued on s (d_scores may be nullptr); reserves the partial records it needs
int launch_spot_stage(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_frames, uint32_t frames_stride, uint32_t n_rows,
                      const SpotGeom &g, sr_spot_hit *d_hits, uint32_t *d_scores, hipStream_t s);
// ---- full-DP alignment and DBA training (sr_align.cpp), shared with the clustering calls (sr_cluster.cpp) ---------------------
struct AlignIn {  // the feature rows every aligner call takes
    const int16_t *mfcc;
    const uint32_t *frames;
    uint32_t frames_stride, n_rows;
};
// what every aligner call checks: the engine's configuration, the required pointers, frames_stride, ref_rows (named `what`)
int check_align_common(const sr_engine *h, const AlignIn &in, const void *ref, const void *ref_frames, uint32_t ref_rows, const char *what);
// room for the DBA iterations of a call over E examples and M models (marks, spans, records, accumulators, and the
// intermediate centroid set when n_iter > 1), the accumulators cleared on s; *p = the launch plan dba_iteration takes
int dba_begin(sr_engine *h, uint32_t E, uint32_t M, uint32_t cen_rows, uint32_t n_iter, AlignPlan *p, hipStream_t s);
// one DBA iteration on s: every row aligned against the centroid d_model_of names (an entry that names none is gated), the
// OK rows' path points summed, `cur` divided into `next`; st (optional): this iteration's statistics row, or nullptr
int dba_iteration(sr_engine *h, const AlignIn &in, const uint32_t *d_model_of, uint32_t M, const int16_t *cur, const uint32_t *d_cen_frames,
                  uint32_t cen_rows, int16_t *next, sr_train_stat *st, const AlignPlan &p, hipStream_t s);
// ---- connected-word decoding (sr_chain.cpp) -----------------------------------------------------------------------------------
// the conditions of sr_decode_words_dp_dev on the engine, the store and the parameters (not on the buffers)
int check_chain(const sr_engine *h, uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost);
// the conditions of sr_decode_words_dp_dev on its buffers as well (check_chain first)
int check_chain_stage(const sr_engine *h, const void *mfcc, const void *frames, uint32_t frames_stride, uint32_t n_rows, uint32_t max_words,
                      uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost, const sr_chain_rec *rec, const sr_chain_word *words,
                      const uint32_t *level_cost);
// ---- one-pass connected-word decoding (sr_onepass.cpp) ------------------------------------------------------------------------
// the conditions of sr_decode_onepass_dp_dev on the engine, the store and the parameters (not on the buffers)
int check_onepass(const sr_engine *h, uint32_t frames_cap, uint32_t words_cap, uint32_t skip_cost, uint32_t word_cost);
// ---- grammar-constrained decoding (sr_gram.cpp) -------------------------------------------------------------------------------
// The compiled form (sr_gram_compile.h builds it on the host).  Items ascend by (slot, target); level l's lists are sorted by
// the distance from the target to a final state, so that what a call with max_words keeps is a PREFIX of each list.
struct sr_grammar {
    sr_engine *h = nullptr;
    uint64_t store_serial = 0, word_serial = 0;
    uint32_t n_states = 0, n_sets = 0, n_items = 0, max_frames = 0, tpl_len = 0;
    using Level = GramLevelLists;
    Level lv[kChainMaxWords];
    // device: masks u64 [n_sets] | items [n_items] | lists u32 | final u8 [n_states], and behind them for a weighted grammar
    // (some cost nonzero; every other grammar ends at `final`): cost_off u32 [n_sets + 1] | costs u32 | final_cost u32 [n_states]
    DevBuf<unsigned long long> blob;
    size_t items_at = 0, lists_at = 0, final_at = 0;  // offsets in u64 units
    bool weighted = false;
    size_t cost_off_at = 0, costs_at = 0, final_cost_at = 0;  // offsets in u64 units (weighted only)
    // behind all of that, for one-pass grammar decoding (sr_onepass_gram.cpp; sr_onepass_gram_plan.h builds them at create):
    // kept items u32 [op_n_items] (indices into items) | kept states u32 [op_n_states], both ascending
    size_t op_items_at = 0, op_states_at = 0;  // offsets in u64 units
    uint32_t op_n_items = 0, op_n_states = 0;
    std::vector<uint32_t> op_item_slots;  // host: the slot of each kept item (the commit window of a live session)
    uint32_t max_arc_cost = 0, max_final_cost = 0;  // the largest of each: the decoder's cost bound
    GramCosts costs() const  // the weighted kernels' second argument
    {
        return GramCosts{(const uint32_t *)(blob.p + cost_off_at), (const uint32_t *)(blob.p + costs_at), (const uint32_t *)(blob.p + final_cost_at)};
    }
};
// a grammar of this engine, compiled against its current store and word map
int check_grammar(const sr_engine *h, const sr_grammar *g);
// what level l (1-based) of a call with max_words keeps
GramLevel gram_level_of(const sr_grammar *g, uint32_t l, uint32_t max_words);
// ---- one-pass grammar decoding (sr_onepass_gram.cpp) --------------------------------------------------------------------------
// the conditions of sr_decode_onepass_grammar_dp_dev on the engine, the store, the grammar and the parameters (not on the buffers)
int check_onepass_grammar(const sr_engine *h, const sr_grammar *g, uint32_t frames_cap, uint32_t words_cap, uint32_t skip_cost, uint32_t word_cost);
