// Kernel argument blocks and launch entry points shared by the host engine and the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sr_engine.h"
#include "sr_onepass_plan.h"

namespace sr {

// Development / test hooks (C ABI: sr_dev_hook): process-global integer knobs, 0 = default behaviour.  They exist ONLY in
// the -DSR_TESTING build (libsr_engine_testing.so, used by the test suite and the tuning sweeps): in the product library
// dev_hook() is the constant 0, every branch on it folds away at compile time, and sr_dev_hook refuses every name.
// Nothing in the product depends on the environment, except SR_RCCL_LIBRARY (the path of the collective library, a
// deployment setting).
enum DevHook {
    kHookDtwU,            // "dtw_u":       force U utterances per k_dtw_lds workgroup (read when a template store is set)
    kHookDtwTieG,         // "dtw_tie_g":   force the staged tie-table size
    kHookDtwKc,           // "dtw_kc":      cap the templates per k_dtw_lds workgroup
    kHookMfccGrid,        // "mfcc_grid":   workgroups of the frame kernel (read by sr_create)
    kHookPerturbLogThr,   // "perturb_log_thr": move host-built log step m by one (exercises the shipped-table check)
    kHookLogThrFromHost,  // "log_thr_from_host": keep the host's log step table even where it differs from the shipped one
    kHookMultiAllowDup,   // "multi_allow_dup": sr_multi_create accepts one device several times (1-GPU tests over the RCCL double)
    kHookDtwDebug,        // "dtw_debug":   print the DTW plan when a store is set, and the full-DP scorer's form per launch
    kHookCellsLiteral,    // "cells_literal": k_dtw_cells walks every pair literally (the fallback of walks that leave the band)
    kHookMagCheapOff,     // "mag_cheap_off": sr_create behaves as if the device sweep of the cheap magnitude form had failed (bound 0)
    kHookMagTableOff,     // "mag_table_off": k_mfcc sends QUIET frames down the MID tier (cheap root, literal filterbank term) instead of the table
    kHookStreamTile,      // "stream_tile_frames": frames per tile of the stream VAD scan (16..1024, a multiple of 16)
    kHookSpotChunk,       // "spot_chunk_cols": columns per chunk of the word spotter (1..16383; read per launch)
    kHookAlignPairs,      // "align_pairs": pairs per launch of the full-DP aligner (read per call and by sr_align_geometry)
    kHookAlignGlobal,     // "align_marks_global": the aligner keeps its predecessor marks in global scratch whatever fits the LDS
    kHookChainChunk,      // "chain_chunk_cols": columns per chunk of the connected-word decoder (1..16383; read per call)
    kHookChainRows,       // "chain_rows": rows per launch group of the connected-word decoder (read per call and by sr_decode_geometry)
    kHookSpanGroups,      // "span_groups": groups of spans per launch of the span scorer (default 65 535, the grid's limit; read per call)
    kHookClusterPairs,    // "cluster_pairs": (example, model) pairs per launch of the clustering score pass (default 2^20; read per call)
    kHookForcedPruneOff,  // "forced_prune_off": the forced aligner sweeps every end frame of every level (no column bound; read per call)
    kHookOnePassBlock,    // "onepass_block": frames per block of the one-pass decoder, clamped to 1..L (read per call and push, and by the two one-pass geometry calls)
    kHookOnePassRows,     // "onepass_rows": rows per launch group of the one-pass decoder (read per call and by sr_decode_onepass_geometry)
    kHookOnePassGramPruneOff,  // "onepass_gram_prune_off": one-pass grammar decoding keeps every item and every state (no static pruning; read per call and by sr_onepass_grammar_plan; the live session reads it when it adopts a grammar)
    kHookLiveOrigin,      // "live_origin": samples a fresh sr_live channel behaves as having consumed before (a multiple of hop; read at open / end)
    kHookSpotLiveOrigin,  // "spot_live_origin": frames a fresh sr_spot_live channel stands at (up to 0xFFFF0000; read at open / end)
    kHookLdsPoisonLaunches,  // "lds_poison_launches": k_lds_poison in front of every kernel launch (SR_LAUNCH_POINT): bits 0..31 seed, 32..33 pattern
    kHookCount
};
#ifdef SR_TESTING
int64_t dev_hook(DevHook h);
#else
constexpr int64_t dev_hook(DevHook) { return 0; }
#endif

// Launch points: SR_LAUNCH_POINT(stream, "k_name") stands immediately in front of EVERY kernel launch of the library
// (tests/test_stale_state.py scans the sources for one that has none).  The product library compiles it to nothing.  In the
// -DSR_TESTING build it calls launch_point (k_misc.hip): while the hook "lds_poison_launches" is non-zero, the LDS of every CU is
// overwritten on that stream before the kernel runs -- between the launches of ONE call too, where no caller can reach -- and
// the kernel's name is recorded.  Patterns (bits 32..33 of the hook): kPoisonHigh is sr_lds_poison's, every word >= 2^31 (loses
// every minimum: "unreachable"); kPoisonLow is (seed ^ i * 2654435761) & 7, a small, valid-looking cost, index or s16 pair that
// WINS every minimum it enters.
constexpr uint32_t kPoisonHigh = 0, kPoisonLow = 1;
#ifdef SR_TESTING
void launch_point(hipStream_t s, const char *kernel);
void launch_points_reset();                                   // counter and names back to nothing (sr_dev_hook, when the hook is set)
uint64_t launch_points_seen(char *names, size_t names_cap);   // poison launches since then; the distinct names, comma-separated
int launch_lds_probe(uint32_t words, uint32_t *d_out, hipStream_t s);  // returns the workgroups launched (one per CU), < 0 on failure
#define SR_LAUNCH_POINT(stream, name) ::sr::launch_point((stream), (name))
#else
#define SR_LAUNCH_POINT(stream, name) ((void)0)
#endif

// device-resident constant tables (see sr_tables.h)
struct DevTables {
    const uint16_t *hamm;      // [160]
    const uint16_t *tri_even;  // [512]
    const uint16_t *tri_odd;   // [512]
    const uint16_t *tri_cen;   // [24]
    const int8_t *dct;         // [288]
    const uint32_t *tw_a;      // [1020]
    const uint32_t *tw_b;      // [1020]
    const uint32_t *log_thr;   // [2220]
    const uint32_t *tri_even32;  // [bins] the same weights widened to 32 bits (16-byte vector loads in k_mfcc)
    const uint32_t *tri_odd32;
    const uint32_t *tri_even_m;  // [bins] mel_fused_multiplier(tri_even[i]) (sr_tables.h): k_mfcc's filterbank terms are one v_mul_hi_u32
    const uint32_t *tri_odd_m;
    const uint32_t *w512_a;    // [256]  EXTENSION front end only
    const uint32_t *w512_b;    // [256]
    const int8_t *tie_delta;   // [kTieMax] DTW tie thresholds: T(g) = g*(g+2) + tie_delta[g] (sr_tables.h)
    const uint32_t *hamm_pk;   // [frame_len / 2] hamm[2p] | hamm[2p+1] << 16 (k_mfcc_ext reads its window weights as pairs)
};

struct VadArgs {
    const uint16_t *pcm;  // [B][pcm_stride], 16-byte aligned rows
    uint64_t pcm_stride;  // samples
    uint32_t buf_len;     // samples scanned by VAD (VcBuf_Len)
    uint32_t noise_len;   // atap_len
    uint32_t atap_frm;    // atap_frm_len (240)
    uint32_t max_frames;  // vv_frm_max
    uint32_t max_seg;     // max_vc_con
    uint32_t B;
    sr_vad_rec *vad;      // [B]
    const sr_atap *atap_in;  // optional [B]: use these thresholds instead of running noise_atap
    uint64_t *dbg_masks;     // optional [B][16]: per-round ballot of "loud" frames (diagnostics)
    uint32_t frame_len;      // 160 (reference), 320 (extension) or one of the generic front end's framings (k_vad_gen.hip)
    uint32_t v_durmin;       // VAD.C:72-73: 80 ms / (frame_time - frame_mov_t) frames (8 at 20 / 10 ms)
    uint32_t s_durmax;       // VAD.C:74-75: 110 ms / (frame_time - frame_mov_t) frames (11)
    uint32_t wide;           // 1: a workgroup of four waves per capture (k_vad_wide.hip; small launches), 0: one wave per capture
};

// stream VAD (k_vad_stream.hip): B recordings scanned in tiles of tile_frames frames, nt tile slots per recording
struct VadStreamArgs {
    const uint16_t *pcm;      // [B][pcm_stride], 16-byte aligned rows
    uint64_t pcm_stride;      // samples
    uint32_t buf_len;         // samples per recording at most
    const uint32_t *len;      // optional [B]: samples of each recording (clamped to buf_len)
    uint32_t B;
    const uint8_t *atap_src;  // thresholds of recording b at atap_src + b * atap_src_stride (sr_atap, or sr_vad_rec.atap)
    uint32_t atap_src_stride;
    uint32_t frame_len, hop, v_durmin, s_durmax;
    uint32_t n_front;         // onset states: max(v_durmin - 1, 1); tail states likewise from s_durmax
    uint32_t n_states;        // 2 + onset states + tail states
    uint32_t tile_frames;     // T, a multiple of 16, <= kStreamTileMax
    uint32_t nt;              // tile slots per recording: ceil(frames of buf_len / T)
    uint32_t mask_words;      // ceil(T / 32)
    uint32_t max_frames;
    uint64_t *tab;            // [B * nt][3][n_states]: state out | carry out << 8 | starts << 10, last start frame << 32
    uint32_t *masks;          // [B * nt][3][mask_words]: loud bits per carry in
    uint4 *tile_in;           // [B * nt]: carry | state << 8, segments before the tile, start of the open segment
    sr_atap *atap_res;        // [B] the thresholds used
    sr_atap *atap_out;        // optional [B]
    uint32_t *seg_offsets;    // [B + 1]
    sr_stream_seg *segs;      // [max_segs]
    uint32_t max_segs;
};
constexpr uint32_t kStreamTileMax = 1024, kStreamTileDefault = 512;  // frames per tile of the stream VAD scan
constexpr uint32_t kStreamLead = 8;  // samples before a segment in its recognition row (the pre-emphasis predecessor)
struct StreamRecArgs {
    const uint16_t *pcm;
    uint64_t pcm_stride;
    const sr_stream_seg *segs;
    const uint32_t *seg_offsets;  // [B + 1]
    uint32_t B;
    const sr_atap *atap;          // [B]
    uint32_t r0;                  // first record of this launch
    uint32_t frame_len, hop, max_frames;
    uint16_t *rows;               // [n][row_stride]
    uint64_t row_stride;
    sr_vad_rec *recs;             // [n]
};

// live sessions (k_live.hip): chunked audio, VAD state carried from push to push.  One record per channel; the host mirrors
// received / next_frame / atap_set (it knows every count), carry, state and open_start live on the device alone.
struct LiveChan {  // 48 bytes
    sr_atap atap;         // the thresholds, once atap_set
    uint32_t atap_set;    // 1: given at open, or computed when the noise head was complete
    uint32_t carry;       // class of the last out-of-band sample in blocks < next_frame (last_sig, VAD.C:99: never reset)
    uint32_t state;       // StreamSm state number
    uint64_t next_frame;  // frames consumed so far = absolute index of the next one
    int64_t open_start;   // start of the segment open in state speech / tail (VAD.C:178)
    uint64_t received;    // samples since the channel's recording began
};
struct LiveEvent {  // an END event (VAD.C:198-207) of one push, in the channel's bounded slots
    int64_t start, end;
};
struct LiveArgs {
    LiveChan *chan;             // [C]
    uint16_t *ring;             // [C][ring_stride]: whole blocks of hop samples, by absolute block number modulo ring_blocks
    uint64_t ring_stride;       // samples = ring_blocks * hop
    uint32_t ring_blocks;
    uint32_t C;
    const uint16_t *pcm;        // the chunks of this push: [C][pcm_stride], 16-byte aligned rows
    uint64_t pcm_stride;
    const uint32_t *n;          // [C] samples of each chunk; NULL: n_all each
    uint32_t n_all;
    const sr_vad_rec *head_vad; // k_vad records of channels head_c0 ..: thresholds of the noise heads completed by this push
    uint32_t head_c0;
    uint32_t noise_len;
    uint32_t frame_len, hop, v_durmin, s_durmax, max_frames;
    LiveEvent *events;          // [C][ev_slots]
    uint32_t *ev_count;         // [C]
    uint32_t ev_slots;
    sr_live_seg *segs;          // [max_segs] compacted: ascending channel, then ascending start
    uint32_t max_segs;
    uint32_t *count;            // [1] the total
};
struct LiveRecArgs {
    const LiveChan *chan;
    const uint16_t *ring;
    uint64_t ring_stride;
    const sr_live_seg *segs;
    const uint32_t *count;        // [1]
    uint32_t r0;                  // first record of this launch
    uint32_t frame_len, hop, max_frames;
    uint16_t *rows;               // [n][row_stride]
    uint64_t row_stride;
    sr_vad_rec *recs;             // [n]
};
void launch_live_append(const LiveArgs &a, hipStream_t s);
void launch_live_scan(const LiveArgs &a, bool sad, hipStream_t s);  // scan + count / offsets / compaction
void launch_live_records(const LiveRecArgs &a, uint32_t n, hipStream_t s);

struct MfccArgs {
    const uint16_t *pcm;
    uint64_t pcm_stride;
    uint32_t B;
    uint32_t max_frames;
    const sr_vad_rec *vad;  // segment 0 + mid_val + frm_num per utterance
    int16_t *mfcc;          // [B][max_frames][12]
    uint32_t tiles;         // frame tiles per utterance
    uint32_t small_tiles;   // 0: 64-frame work items; 1 / 2: the 16- / 4-frame forms of k_mfcc for underfilled launches (tiles counts those)
    uint32_t n_items;       // B * tiles
    uint32_t grid_cap;      // resident workgroups of k_mfcc on this device (0 = default)
    uint32_t mag_cheap_max; // k_mfcc: largest re^2 + im^2 whose magnitude may take the uncorrected v_sqrt_f32 (kMagCheapMax where sr_create's sweep of this device confirmed it, else 0)
    uint32_t frame_len;     // 160 -> k_mfcc (reference front end), 320 -> k_mfcc_ext (extension)
    uint32_t generic;       // 1 -> k_mfcc_gen (GENERIC front end): the four fields below are only read there
    uint32_t hop, n_mel, n_coef;
    DevTables t;
};
// k_mfcc alone also takes the QUIET-tier magnitude table.  A block of its own, appended to the kernel's arguments by the
// launcher (k_mfcc.hip MfccTabArgs): MfccArgs and DevTables are shared with k_mfcc_ext / k_mfcc_gen, whose argument layout --
// and with it their code -- stays as it is.
struct MfccMagTab {
    const uint16_t *mag_q;   // [kMagTabEntries] magnitudes << 2 (sr_tables.h), read through a buffer resource of exactly that size
    uint32_t mag_table_off;  // -DSR_TESTING build only: development hook "mag_table_off"
};

// launch arguments of the feature kernels (sr_frame_features_batch_dev): the frame kernel's block + the feature output
// feat[B][max_frames][width], kind = SR_FEAT_*.  A separate type, so that the frame kernels' own argument block stays as it is;
// the kernels are templates on the argument type (mfcc_feat_kind<MfccArgs> = 0: no feature stores).
template <int kKind>
struct MfccFeatArgs : MfccArgs {
    uint32_t *feat;
};
template <typename Args>
constexpr int mfcc_feat_kind = 0;
template <int kKind>
constexpr int mfcc_feat_kind<MfccFeatArgs<kKind>> = kKind;
template <int kKind>
inline MfccFeatArgs<kKind> mfcc_feat_args(const MfccArgs &a, uint32_t *feat)
{
    MfccFeatArgs<kKind> f;
    static_cast<MfccArgs &>(f) = a;
    f.feat = feat;
    return f;
}

struct DtwArgs {
    const int16_t *mfcc;      // [B][max_frames][12]
    const sr_vad_rec *vad;    // frm_num / status per utterance (or NULL with in_frames)
    const uint32_t *in_frames;  // optional [B] explicit frame counts (stage-level API)
    uint32_t B;
    uint32_t max_frames;
    const int16_t *tpl;       // [K][tpl_stride]
    const uint32_t *tpl_frames;
    const uint8_t *tpl_valid;
    uint32_t K;
    uint32_t tpl_stride;      // int16 elements per template
    uint32_t tpl_rows;        // rows allocated per template
    uint32_t *scores;         // [B][K]
    sr_result *results;       // [B] (argmin kernel)
    // length-sorted, row-interleaved copy of the store for k_dtw_lds / k_dtw_dp_band
    const void *tplR;             // [tpl_rows][K] 32-byte rows: 12 x s16 | u32 squared norm | pad  (48-byte rows of 16 x s16 when n_coef > 12)
    const uint32_t *tpl_frames_s; // [K]
    const uint32_t *tpl_orig;     // [K]
    const int8_t *tie_delta;      // DevTables::tie_delta
    uint32_t n_coef;              // s16 per feature row: 12 everywhere except the GENERIC front end (1..16)
    uint32_t *pair_count;         // k_dtw_cells only: [B] zeroed counters of finished pairs (the last one does the slot scan); may be NULL
    uint32_t cells_points;        // k_dtw_cells only: most band points of any pair of this store (DtwPlan::cells_points)
    uint32_t cells_literal;       // k_dtw_cells only: development hook "cells_literal" -- every pair takes the literal fallback walk
};

// word-level N-best (k_nbest.hip): rows of K scores reduced to the n_best best words under the engine's word grouping
struct NbestArgs {
    const uint32_t *scores;       // [n_rows][K]
    uint32_t n_rows;
    uint32_t K;
    uint32_t n_words;             // 1..K
    uint32_t n_best;              // 1..SR_NBEST_MAX
    const uint32_t *order;        // [K] the slots grouped by word, ascending inside a word (sr_word_groups)
    const uint32_t *group_start;  // [n_words + 1] where each word's slots start in order
    const uint32_t *word_id;      // [n_words] the caller's labels
    sr_nbest_entry *out;          // [n_rows][n_best]
    uint32_t *n_matched;          // optional [n_rows]
};
void launch_nbest(const NbestArgs &a, hipStream_t s);

// two-pass rescoring, the mark pass (k_rescore.hip): the slots of the candidate words of every row's input list
struct RescoreMarkArgs {
    const sr_nbest_entry *in;       // [n_rows][n_best] first-pass lists (read only)
    uint32_t n_rows;
    uint32_t n_best;
    uint32_t K;
    const uint32_t *order;          // the engine's word grouping, as NbestArgs
    const uint32_t *group_start;
    const uint32_t *group_of_slot;  // [K] index of the word group a slot belongs to
    const uint32_t *tpl_rank;       // [K] rank of a slot in the store's length order
    uint8_t *marks;                 // [K ranks][mark_stride] zeroed; 1 = score this (row, slot)
    uint32_t mark_stride;
};
void launch_rescore_mark(const RescoreMarkArgs &a, hipStream_t s);

// word spotting (k_spot.hip): subsequence DTW of every template inside every feature row.  The end frames of a row are cut
// into chunks of chunk_cols columns, one wave each.  split = 0: a chunk holds `per` whole windows and writes their records
// itself; split = 1: a window is cut into `per` chunks, each leaves one partial record and k_spot_finish reduces them.
struct SpotArgs {
    const int16_t *mfcc;        // [n_rows][max_frames][12]
    const uint32_t *in_frames;  // frame count of row r at in_frames[r * frames_stride] (clamped to max_frames)
    uint32_t frames_stride;
    uint32_t n_rows;
    uint32_t max_frames;
    const int16_t *tpl;         // [K][tpl_stride]
    const uint32_t *tpl_frames;
    const uint8_t *tpl_valid;
    uint32_t K;
    uint32_t tpl_stride;
    uint32_t tpl_len;           // the longest template: rows of the LDS image and of a boundary column
    uint32_t n_win;             // windows per row
    uint32_t win;               // end frames per window (max_frames when there is one window)
    uint32_t chunk_cols;
    uint32_t n_chunks;          // chunks per row
    uint32_t split, per;
    sr_spot_hit *hits;          // [n_rows * n_win][K]
    uint32_t *scores;           // optional [n_rows * n_win][K]
    sr_spot_hit *part;          // split only: [n_rows * n_chunks][K]
};
void launch_spot(const SpotArgs &a, hipStream_t s);

// live word spotting (k_spot_live.hip): k_spot's sweep resumed from push to push.  The state of a (channel, slot) pair is the
// boundary column -- (Dd, min(Dd, Dn)) per template row, starts absolute -- and the window reduction's carry; a channel's
// state is cols[K][tpl_len] followed by K carries, chan_stride bytes per channel.  The host knows every count: it says where
// each channel stands and where its records go.
struct SpotLiveChan {  // 32 bytes, one per channel and push
    uint32_t x0;         // frames of the channel before this push = absolute index of its first new frame
    uint32_t n;          // new frames (0: the channel is not touched)
    uint32_t row_base;   // output row of the first window this push completes
    uint32_t first_win;  // ... and that window's number, x0 / win
    uint32_t kept;       // PCM sessions: samples kept from earlier pushes, new samples, and the samples at the front of
    uint32_t n_samp;     // [kept | chunk] that no later frame needs (new frames * hop)
    uint32_t drop;
    uint32_t aux;        // one-pass live sessions (OnePassLiveArgs) -- a push: the first frame of the block the channel's saved
                         // columns are of; the end call: the frames the channel holds.  Every other session: 0
};
// the carry: the first minimum so far of the window the channel's last frame lies in, two 16-byte words
// {key = q << 32 | end (all ones = none; an invalid slot keeps it that way), start | cost << 32}, {window id, 0}
// (read and written by spot_live_carry()'s users in k_spot_live.hip alone)
constexpr uint32_t kSpotLiveCarryBytes = 32;
struct SpotLiveArgs {
    const int16_t *mfcc;        // channel c's new frames at mfcc + c * row_stride, 8-byte aligned rows
    uint64_t row_stride;        // s16 elements
    const SpotLiveChan *chan;   // [C]
    uint32_t C;
    const int16_t *tpl;         // [K][tpl_stride]
    const uint32_t *tpl_frames;
    const uint8_t *tpl_valid;
    uint32_t K;
    uint32_t tpl_stride;
    uint32_t tpl_len;           // the longest template: rows of the LDS image and of a boundary column
    uint32_t win;               // end frames per window, >= 1
    uint8_t *state;             // [C][chan_stride]
    uint64_t chan_stride;       // bytes, a multiple of 16
    sr_spot_hit *hits;          // [rows][K], compact over the windows the push completes
    uint32_t *scores;           // optional [rows][K]
};
void launch_spot_live(const SpotLiveArgs &a, hipStream_t s);
struct SpotLiveFlush {  // one listed channel of sr_spot_live_end
    uint32_t channel, row;  // row = 0xFFFFFFFF: no open window, the state is reset only
    uint32_t wid, _pad;
};
void launch_spot_live_flush(const SpotLiveFlush *list, uint32_t n_list, uint8_t *state, uint64_t chan_stride, uint32_t K,
                            uint32_t tpl_len, sr_spot_hit *hits, hipStream_t s);
// PCM sessions: rows [kept | chunk] for the frame kernel, then what the next push's first frame needs back into `keep`
struct SpotLivePcmArgs {
    const SpotLiveChan *chan;
    uint32_t C;
    const uint16_t *pcm;        // [C][pcm_stride] the chunks
    uint64_t pcm_stride;
    uint16_t *keep;             // [C][keep_stride]
    uint32_t keep_stride;
    uint16_t *stage;            // [C][stage_stride], 16-byte aligned rows
    uint64_t stage_stride;
    uint32_t max_row;           // the longest [kept | chunk] row of this push
};
void launch_spot_live_stage(const SpotLivePcmArgs &a, hipStream_t s);
void launch_spot_live_keep(const SpotLivePcmArgs &a, hipStream_t s);

// connected-word decoding (k_chain.hip): level building over the template store.  One launch group covers n_rows rows whose
// scratch is A[row][level 1..max_words][max_frames + 1] (packed cost << 32 | start << 16 | slot, all ones = unreachable) and
// E[row][level 0..max_words][max_frames + 1] (prefix costs, SR_DIS_ERR = unreachable); every pointer is the group's first row.
struct ChainArgs {
    const int16_t *mfcc;        // [n_rows][max_frames][12]
    const uint32_t *in_frames;  // frame count of row r at in_frames[r * frames_stride] (clamped to max_frames)
    uint32_t frames_stride;
    uint32_t n_rows;            // <= 65 535
    uint32_t max_frames;
    const int16_t *tpl;         // [K][tpl_stride]
    const uint32_t *tpl_frames;
    const uint8_t *tpl_valid;
    uint32_t K;                 // <= 65 536: the slot is 16 bits of a key
    uint32_t tpl_stride;
    uint32_t tpl_len;           // the longest template: rows of the LDS image and of a boundary column
    uint32_t chunk_cols;        // end frames per wave
    uint32_t n_chunks;          // chunks per row
    uint32_t max_words;         // levels
    uint32_t n_words_exact;     // 0: the cheapest count
    uint32_t skip_cost;         // SR_DIS_ERR: no skipping
    uint32_t word_cost;
    unsigned long long *A;
    uint32_t *E;
    const uint32_t *group_of_slot;  // the engine's word grouping (sr_nbest.cpp): slot -> group, group -> label
    const uint32_t *word_id;
    sr_chain_rec *rec;          // [n_rows]
    sr_chain_word *words;       // [n_rows][max_words]
    uint32_t *level_cost;       // optional [n_rows][max_words]
};
void launch_chain(const ChainArgs &a, hipStream_t s);  // init, max_words x (k_chain_words, k_chain_close), k_chain_trace
// k_chain_init and one level's k_chain_close alone, for the forced aligner, whose scratch is the decoder's (k_forced.hip)
void launch_chain_init(const ChainArgs &a, hipStream_t s);
void launch_chain_close(const ChainArgs &a, uint32_t level, hipStream_t s);

// transcript-forced alignment (k_forced.hip): the decoder's levels with a grid over a host-built item list.  c is the decoder's
// argument block for one launch group with max_words = words_per_row (n_words_exact and level_cost are not read); an item is
// (row of the CALL, slot); tail and count are the group's rows of the host's tables (sr_forced_plan.h).
struct ForcedArgs {
    ChainArgs c;
    const uint2 *items;     // the call's list
    const uint32_t *tail;   // [n_rows][max_words]: level l of a row sweeps the end frames e with e + 1 <= N - tail[l - 1]
    const uint32_t *count;  // [n_rows]: words of each transcript, 0..max_words
    uint32_t row0;          // the group's first row in the call
};
// init, per level 1..levels (k_forced_words over the items [item0[l - 1], item0[l]) when there are any, k_chain_close), k_forced_trace
void launch_forced(const ForcedArgs &a, const uint32_t *item0, uint32_t levels, hipStream_t s);
// span gather (k_forced.hip): example e = the frames of span src_of_ex[e] of the word rows, or an empty row
struct GatherArgs {
    const int16_t *mfcc;         // [n_rows][max_frames][12]
    const uint32_t *in_frames;   // frame count of row r at in_frames[r * frames_stride] (clamped to max_frames)
    uint32_t frames_stride;
    uint32_t max_frames;
    const sr_chain_word *words;  // [n_rows][words_per_row]; only start and end are read
    uint32_t words_per_row;
    const uint32_t *src_of_ex;   // [n_ex]: a span index, or all ones
    uint32_t n_ex, ex_rows;
    int16_t *ex;                 // [n_ex][ex_rows][12]
    uint32_t *ex_frames;         // [n_ex]
};
void launch_gather_spans(const GatherArgs &a, hipStream_t s);

// word alternatives (k_span.hip): the best path of every template over fixed spans of frames, start and end pinned.  Span i
// = words[i] (only start and end are read) lies in feature row i / words_per_row; one wave per (span, slot).
struct SpanArgs {
    const int16_t *mfcc;        // [n_rows][max_frames][12]
    const uint32_t *in_frames;  // frame count of row r at in_frames[r * frames_stride] (clamped to max_frames)
    uint32_t frames_stride;
    uint32_t max_frames;
    const int16_t *tpl;         // [K][tpl_stride]
    const uint32_t *tpl_frames;
    const uint8_t *tpl_valid;
    uint32_t K;
    uint32_t tpl_stride;
    uint32_t tpl_len;           // the longest template: rows of the LDS image and of a boundary column
    const sr_chain_word *words; // [n_spans]
    uint32_t words_per_row;     // >= 1
    uint32_t n_spans;           // n_rows * words_per_row
    uint32_t mode;              // SR_SPAN_ACC / SR_SPAN_DIS
    uint32_t max_groups;        // groups of kSpotWaves spans per launch, 1..65 535
    uint32_t *scores;           // [n_spans][K]
};
void launch_span(const SpanArgs &a, hipStream_t s);

// one-pass connected-word decoding (k_onepass.hip): ONE prefix-cost array over all word counts, built in blocks of at most
// L = min_k(M_k / 2 + 1) frames.  One launch group covers n_rows rows whose scratch is A[row][max_frames + 1] (ChainArgs' keys),
// E[row][max_frames + 1] and cols[row][K][tpl_len]: per (row, slot) ONE saved column in k_chain_live_words' (Dd, min(Dd, Dn))
// layout -- the exact column at the first frame of the block swept last.  Every pointer is the group's first row.
struct OnePassArgs {
    const int16_t *mfcc;        // [n_rows][max_frames][12]
    const uint32_t *in_frames;  // frame count of row r at in_frames[r * frames_stride] (clamped to frames_cap)
    uint32_t frames_stride;
    uint32_t n_rows;
    uint32_t max_frames;
    uint32_t frames_cap;        // 1..max_frames: the host's bound on every row's frames; it fixes the blocks
    const int16_t *tpl;         // [K][tpl_stride]
    const uint32_t *tpl_frames;
    const uint8_t *tpl_valid;
    uint32_t K;                 // <= 65 536: the slot is 16 bits of a key
    uint32_t tpl_stride;
    uint32_t tpl_len;           // the longest template: rows of the LDS image and of a saved column
    uint32_t words_cap;         // word rows per row of d_words, >= 1
    uint32_t skip_cost;         // SR_DIS_ERR: no skipping
    uint32_t word_cost;
    unsigned long long *A;
    uint32_t *E;
    ulonglong2 *cols;
    const uint32_t *group_of_slot;
    const uint32_t *word_id;
    sr_chain_rec *rec;          // [n_rows]
    sr_chain_word *words;       // [n_rows][words_cap]
};
// init, per block of the host's list (sr_onepass_plan.h) (k_onepass_words, k_onepass_close), k_onepass_trace
void launch_onepass(const OnePassArgs &a, const OnePassBlock *blocks, uint32_t n_blocks, hipStream_t s);

// live one-pass connected-word decoding (k_onepass_live.hip): k_onepass.hip's blocks with the boundaries set by the caller's
// pushes.  Per channel the session keeps the history A[C][P] / E[C][P], P = utt_frames + 1, in OnePassArgs' layout, one saved
// column per slot, cols[C][K][tpl_len] -- the EXACT column at the first frame of the block swept last, chan[c].aux -- and the
// channel's whole feature row feat[C][utt_frames][12], of which a sweep reads the columns before the push.  A position of A no
// push has reached holds all ones (set at open, put back by the end call); E(0) = 0.  The per-channel entry is the spot
// session's: x0, n; row_base = the channel's compact output row; first_win != 0 = the channel emits a row.  A push's frames
// [x0, x0 + n) are cut into blocks of `block` frames; launch b sweeps block b of every channel that has one.
struct OnePassLiveArgs {
    const int16_t *mfcc;        // channel c's new frames at mfcc + c * row_stride, 8-byte aligned rows
    uint64_t row_stride;        // s16 elements
    const SpotLiveChan *chan;   // [C]
    uint32_t C;
    const int16_t *tpl;         // [K][tpl_stride]
    const uint32_t *tpl_frames;
    const uint8_t *tpl_valid;
    uint32_t K;
    uint32_t tpl_stride;
    uint32_t tpl_len;           // the longest template: rows of the LDS image and of a saved column
    uint32_t P;                 // utt_frames + 1: positions of the history
    uint32_t block;             // frames per block, 1..max(L, 1)
    uint32_t words_cap;
    uint32_t tail;              // SR_OP_LIVE_TAIL: the last words_cap words instead of the first
    uint32_t skip_cost;         // SR_DIS_ERR: no skipping
    uint32_t word_cost;
    ulonglong2 *cols;
    unsigned long long *A;
    uint32_t *E;
    int16_t *feat;
    const uint32_t *group_of_slot;
    const uint32_t *word_id;
    sr_chain_rec *rec;          // [rows], compact over the emitting channels
    sr_chain_word *words;       // [rows][words_cap]
};
void launch_onepass_live(const OnePassLiveArgs &a, uint32_t n_blocks, hipStream_t s);  // n_blocks x (words, close), trace
// sr_onepass_live_end: the trace of the listed channels (n = 0, x0 = the frames to parse), then all ones over their keys again
// (positions 1..aux: the frames the channel held)
// cursor[C]: the commit cursors (below), which the wipe zeroes for the listed channels
void launch_onepass_live_end(const OnePassLiveArgs &a, uint2 *cursor, hipStream_t s);

// sr_onepass_live_commit[_dev] (k_onepass_live_commit): the words of the listed channels that can no longer change.  It reads the
// history A / E of OnePassLiveArgs and the host's rows -- the channel and its frames N -- and keeps per channel a cursor
// {words delivered so far, the position of the last delivered word's node}, all zero for a channel without a recording.
struct OnePassCommitArgs {
    const sr_chain_live_row *rows;  // [n_rows] on the device: the distinct listed channels and their N
    uint32_t n_rows;
    uint32_t P;                     // utt_frames + 1: positions of the history
    uint32_t W;                     // the window: 2 * (the longest valid template's frames) - 1, 0 without a valid slot
    uint32_t words_cap;
    uint32_t word_cost;
    const unsigned long long *A;
    const uint32_t *E;
    uint2 *cursor;                  // [C]
    const uint32_t *tpl_frames;
    const uint32_t *group_of_slot;
    const uint32_t *word_id;
    sr_commit_rec *crec;            // [n_rows]
    sr_chain_word *cwords;          // [n_rows][words_cap]
};
void launch_onepass_live_commit(const OnePassCommitArgs &a, hipStream_t s);

// grammar-constrained decoding (k_gram.hip): k_chain's levels over a word network of n_states states.  c is the decoder's
// argument block with the scratch in the grammar's layout: c.A[row][level 1..max_words][state][max_frames + 1], c.E[row][level
// 0..max_words][state][max_frames + 1]; C[row][from-set][max_frames + 1] holds the charges of the level in flight.  An item is
// one word pass: a slot into a target state, charged by a from-set.  lists holds, level by level, the indices of the level's
// items, the from-sets they use and their target states; lv[l - 1] says where and how many of each this call keeps.
struct GramItem {
    uint32_t slot, target, set, reserved;
};
struct GramLevel {
    uint32_t item0, n_items, set0, n_sets, state0, n_states;
};
struct GramArgs {
    ChainArgs c;
    uint32_t n_states, n_sets, n_items;
    const unsigned long long *masks;  // [n_sets]: the states of each from-set
    const GramItem *items;            // [n_items], ascending (slot, target)
    const uint32_t *lists;
    const uint8_t *final_state;       // [n_states]
    uint32_t *C;
    GramLevel lv[16];
};
// A weighted grammar's costs (include/sr_engine.h, "weighted grammars"), the second argument of the weighted kernels: charge
// list i's arc costs are cost[cost_off[i] .. cost_off[i + 1]), in the ascending order of the states of masks[i];
// final_cost[n_states] is 0 for a state that is not final.  The unweighted kernels and their argument blocks stay as they are.
struct GramCosts {
    const uint32_t *cost_off, *cost, *final_cost;
};
// init, per level with items (charge, words, close), trace; w null: the unweighted kernels, otherwise the weighted charge and trace
void launch_gram(const GramArgs &a, const GramCosts *w, hipStream_t s);

// live connected-word decoding (k_chain_live.hip): the levels of k_chain.hip resumed from push to push.  Per channel the session
// keeps one boundary column per (level, slot), cols[C][max_words][K][tpl_len], and the history A[C][max_words][P] /
// E[C][max_words + 1][P], P = utt_frames + 1, in ChainArgs' layout with max_frames = utt_frames: after every push positions
// 0..N of a channel hold what the batch decoder's scratch holds for its recording as one row.  The per-channel entry is the
// spot session's (the PCM kernels read it): x0, n as there; row_base = the channel's compact output row; first_win != 0 = the
// channel emits a row (a push: n > 0; sr_decode_live_end: a listed channel, n = 0, x0 = its frames).
struct ChainLiveArgs {
    const int16_t *mfcc;        // channel c's new frames at mfcc + c * row_stride, 8-byte aligned rows
    uint64_t row_stride;        // s16 elements
    const SpotLiveChan *chan;   // [C]
    uint32_t C;
    const int16_t *tpl;         // [K][tpl_stride]
    const uint32_t *tpl_frames;
    const uint8_t *tpl_valid;
    uint32_t K;
    uint32_t tpl_stride;
    uint32_t tpl_len;           // the longest template: rows of the LDS image and of a boundary column
    uint32_t P;                 // utt_frames + 1: positions of a level's history
    uint32_t max_words;
    uint32_t n_words_exact;
    uint32_t skip_cost;         // SR_DIS_ERR: no skipping
    uint32_t word_cost;
    ulonglong2 *cols;
    unsigned long long *A;
    uint32_t *E;
    const uint32_t *group_of_slot;
    const uint32_t *word_id;
    sr_chain_rec *rec;          // [rows], compact over the emitting channels
    sr_chain_word *words;       // [rows][max_words]
    uint32_t *level_cost;       // optional [rows][max_words]
};
void launch_chain_live(const ChainLiveArgs &a, hipStream_t s);        // init, max_words x (words, close), trace
void launch_chain_live_trace(const ChainLiveArgs &a, hipStream_t s);  // the trace alone (sr_decode_live_end)

// live grammar-constrained decoding (k_gram_live.hip): k_gram's levels resumed from push to push.  c is the live decoder's
// argument block with the history in the grammar's layout, c.A[C][max_words][state][P] and c.E[C][max_words + 1][state][P],
// and c.cols[C][columns][tpl_len]: one boundary column per item a level keeps, level l's first at col_off[l - 1], in the order
// of the level's item list.  c.K is not read.  There is no row of charges: a sweep takes the minimum over the from-set itself.
struct GramLiveArgs {
    ChainLiveArgs c;
    uint32_t n_states, n_items, columns;
    const unsigned long long *masks;  // [n_sets]: the states of each from-set
    const GramItem *items;            // [n_items], ascending (slot, target)
    const uint32_t *lists;
    const uint8_t *final_state;       // [n_states]
    GramLevel lv[16];
    uint32_t col_off[16];
};
// w null: the unweighted kernels, otherwise the weighted sweep and trace
void launch_gram_live(const GramLiveArgs &a, const GramCosts *w, hipStream_t s);        // init, per level with items (words, close), trace
void launch_gram_live_trace(const GramLiveArgs &a, const GramCosts *w, hipStream_t s);  // the trace alone (no new frame, sr_gram_live_end)

// one-pass grammar decoding (k_onepass_gram.hip): k_onepass.hip's blocks over the states of a grammar.  o is the one-pass
// decoder's argument block with the scratch in the grammar's layout: o.A[row][state][max_frames + 1], o.E[row][state][max_frames
// + 1] and o.cols[row][kept item][tpl_len]; o.K is not read.  keep_items / keep_states are the host's static lists, ascending
// (sr_onepass_gram_plan.h); a null list is the identity: everything is kept.
struct OnePassGramArgs {
    OnePassArgs o;
    uint32_t n_states, n_items;
    uint32_t n_keep_items, n_keep_states;
    const unsigned long long *masks;  // [n_sets]: the states of each charge list
    const GramItem *items;            // [n_items], ascending (slot, target)
    const uint8_t *final_state;       // [n_states]
    const uint32_t *keep_items;       // [n_keep_items] indices into items, or null
    const uint32_t *keep_states;      // [n_keep_states] states, or null
};
// init, per block of the host's list (sweep, close), trace; w null: the unweighted kernels, otherwise the weighted sweep and trace
void launch_onepass_gram(const OnePassGramArgs &a, const GramCosts *w, const OnePassBlock *blocks, uint32_t n_blocks, hipStream_t s);

// live one-pass grammar decoding (k_onepass_gram_live.hip): k_onepass_gram.hip's blocks with the boundaries set by the caller's
// pushes.  o is the live one-pass decoder's argument block with the history in the grammar's layout, dense by state index:
// o.A[C][n_states][P] and o.E[C][n_states][P], P = utt_frames + 1, and o.cols[C][kept item][tpl_len]; o.feat is the channels'
// feature rows as there; o.K is not read.  A position of A no push has reached holds all ones, E(0, 0) = 0 and E(0, s) is
// unreachable for s != 0 (set at open and when a grammar is adopted, put back by the end call).  keep_items / keep_states as in
// OnePassGramArgs.
struct OnePassGramLiveArgs {
    OnePassLiveArgs o;
    uint32_t n_states, n_items;
    uint32_t n_keep_items, n_keep_states;
    const unsigned long long *masks;  // [n_sets]: the states of each charge list
    const GramItem *items;            // [n_items], ascending (slot, target)
    const uint8_t *final_state;       // [n_states]
    const uint32_t *keep_items;       // [n_keep_items] indices into items, or null
    const uint32_t *keep_states;      // [n_keep_states] states, or null
};
// n_blocks x (sweep where an item is kept, close where a state is kept), trace; w null: the unweighted kernels
void launch_onepass_gram_live(const OnePassGramLiveArgs &a, const GramCosts *w, uint32_t n_blocks, hipStream_t s);
// sr_onepass_gram_live_end: the trace of the listed channels (n = 0, x0 = the frames to parse), then the wipe, then the commit
// cursors (below) of the listed channels back to "nothing delivered"
void launch_onepass_gram_live_end(const OnePassGramLiveArgs &a, const GramCosts *w, uint2 *cursor, hipStream_t s);
// the wipe alone, over every state of the dense layout: the keys of every listed channel (first_win != 0) all ones over the
// positions 0..aux, E(0, 0) = 0 and E(0, s) unreachable (the end call; open and a grammar switch list every channel)
void launch_onepass_gram_live_wipe(const OnePassGramLiveArgs &a, hipStream_t s);

// sr_onepass_gram_live_commit[_dev] (k_onepass_gram_live_commit[_w]): the words of the listed channels that can no longer
// change.  g is the session's argument block as a push fills it (the history, the items and the charge lists; mfcc, chan, rec
// and words are not read); states is the grammar's STATIC kept list whatever g.keep_states is -- the testing hook changes what
// is swept, never what the rule ranges over.  Per channel the cursor is {words delivered so far, the last delivered word's
// node as position | state << kOpgCommitStateShift}, all zero for a channel without a recording.
constexpr uint32_t kOpgCommitStateShift = 16;  // positions take 14 bits, states 6
struct OnePassGramCommitArgs {
    OnePassGramLiveArgs g;
    const sr_chain_live_row *rows;  // [n_rows] on the device: the distinct listed channels and their N
    uint32_t n_rows;
    uint32_t W;                     // the window: 2 * (the longest kept item's template frames) - 1, 0 where nothing is kept
    uint32_t ring;                  // entries of the kernel's LDS ring of marks: a power of two, at least W + 64
    uint32_t block;                 // positions swept at once: 1..64 and at most L, the frames the shortest word covers
    const uint32_t *states;         // [n_kept] the kept states, ascending
    uint32_t n_kept;
    uint2 *cursor;                  // [C]
    sr_commit_rec *crec;            // [n_rows]
    sr_chain_word *cwords;          // [n_rows][words_cap]
};
// w null: the unweighted kernel
void launch_onepass_gram_live_commit(const OnePassGramCommitArgs &a, const GramCosts *w, hipStream_t s);

// full-DP alignment (k_align.hip): one wave per (feature row, reference) pair.  The launch covers rows [row0, row0 + n_pairs)
// of the call; the record and the span of row r go to index r - out0 (0: the caller's buffers; row0: per-launch scratch), the
// marks are indexed by the pair of the launch.
struct AlignArgs {
    const int16_t *mfcc;         // [n_rows][max_frames][12]
    const uint32_t *in_frames;   // frame count of row r at in_frames[r * frames_stride] (clamped to max_frames)
    uint32_t frames_stride;
    uint32_t max_frames;
    const int16_t *ref;          // [n_ref][ref_rows][12]
    const uint32_t *ref_frames;  // [n_ref]; 0 or above ref_rows: an invalid reference
    uint32_t ref_rows, n_ref;
    const uint32_t *ref_of_row;  // optional [n_rows]; NULL: row r pairs with reference r
    sr_align_rec *rec;
    uint32_t *span;              // optional, [..][max_frames]
    uint32_t out0;
    uint32_t *marks;             // [n_pairs][mark_words] in global scratch; NULL: the marks live in LDS
    uint32_t mark_w;             // mark words per input column: 16 reference rows per word, odd
    uint32_t mark_words;         // mark words per pair: columns of the longest admissible row x mark_w
    uint32_t row0, n_pairs;
};
void launch_align(const AlignArgs &a, size_t lds_bytes, hipStream_t s);
// DBA training on top of it: the path points of the OK pairs of a launch summed into the models' accumulators, then one
// pass that divides, keeps, zeroes and clears
struct AlignAccumArgs {
    const int16_t *mfcc;
    const uint32_t *in_frames;
    uint32_t frames_stride;
    uint32_t max_frames;
    const sr_align_rec *rec;     // [n_pairs] of the launch
    const uint32_t *span;        // [n_pairs][max_frames]
    const uint32_t *model_of;    // [n_rows] model of each example
    const uint32_t *cen_frames;  // [M]
    uint32_t cen_rows;
    int32_t *sum;                // [M][cen_rows][12]
    uint32_t *cnt;               // [M][cen_rows]
    sr_train_stat *stats;        // optional [M]: this iteration's row
    uint32_t row0, n_pairs;
};
void launch_align_accum(const AlignAccumArgs &a, hipStream_t s);
struct AlignFinalArgs {
    const int16_t *cen_cur;      // [M][cen_rows][12] the centroids that entered the iteration
    int16_t *cen_next;           // [M][cen_rows][12]
    const uint32_t *cen_frames;
    uint32_t cen_rows, M;
    int32_t *sum;
    uint32_t *cnt;
};
void launch_align_finalise(const AlignFinalArgs &a, hipStream_t s);

// word-model clustering (k_cluster.hip).  The score pass: the cost-only full DP of every (example, model of its word) pair;
// workgroup i of a launch is entry wg0 + i of the host's list (sr_cluster_plan.h): one model, up to kClusterWaves examples.
struct ClusterScoreArgs {
    const int16_t *mfcc;         // [E][max_frames][12]
    const uint32_t *in_frames;   // frame count of example e at in_frames[e * frames_stride] (clamped to max_frames)
    uint32_t frames_stride;
    uint32_t max_frames;
    const int16_t *cen;          // [M][cen_rows][12]
    const uint32_t *cen_frames;  // [M]; 0 or above cen_rows: an invalid centroid
    uint32_t cen_rows;
    const uint32_t *wg;          // [..][3]: model, first example, examples
    const uint32_t *ex_mdl0;     // [E] first model of the example's word
    const uint32_t *ex_nm;       // [E] models of the example's word (1..16)
    uint32_t *dis;               // [E][16]: column c = the model ex_mdl0[e] + c; SR_DIS_ERR from ex_nm[e] on
    uint32_t *acc;               // optional [E][16]: the pairs' accumulated costs, 0xFFFFFFFF where dis is SR_DIS_ERR
    uint32_t wg0, n_wg;
};
void launch_cluster_score(const ClusterScoreArgs &a, size_t lds_bytes, hipStream_t s);
// one thread per example: the first minimum of its score row, the counters of the iteration, the map the update reads
struct ClusterAssignArgs {
    const uint32_t *dis;         // [E][16]
    const uint32_t *acc;         // [E][16], read when stats or iter is given
    const uint32_t *ex_mdl0, *ex_nm;
    uint32_t E;
    const uint32_t *prev;        // optional [E]: the previous iteration's assignment (n_moved)
    uint32_t *cur;               // optional [E]: this iteration's, for the update and the next iteration
    uint32_t *assign;            // optional [E]: the caller's
    uint32_t *best;              // optional [E]
    sr_train_stat *stats;        // optional [M]: this iteration's row, zero on entry
    sr_cluster_iter *iter;       // optional: this iteration's record, zero on entry
};
void launch_cluster_assign(const ClusterAssignArgs &a, hipStream_t s);
void launch_cluster_tally(const sr_train_stat *stats, uint32_t M, sr_cluster_iter *iter, hipStream_t s);  // n_empty and acc

// get_mdl (DTW.C:217-296): P independent pairs
struct GetMdlArgs {
    const int16_t *in1;     // [P][rows1][12]
    const uint32_t *n1;     // [P] frames of in1 ("in" role)
    uint32_t rows1;
    const int16_t *in2;     // [P][rows2][12]
    const uint32_t *n2;     // [P] frames of in2 ("mdl" role)
    uint32_t rows2;
    uint32_t P;
    int16_t *mdl;           // [P][mdl_rows][12] merged templates
    uint32_t mdl_rows;
    uint32_t *mdl_frames;   // [P] step count = frames of the merged template (may exceed mdl_rows), 0 on dis_err
    uint32_t *dis;          // [P] dis/step or dis_err
};
void launch_get_mdl(const GetMdlArgs &a, hipStream_t s);

void launch_vad(const VadArgs &a, hipStream_t s);
void launch_vad_wide(const VadArgs &a, hipStream_t s);  // k_vad_wide.hip
bool vad_framing_supported(uint32_t frame_len, uint32_t hop);  // the VAD kernel is instantiated per framing
void launch_select_segment(const sr_vad_rec *in, sr_vad_rec *out, uint32_t B, uint32_t seg_idx, uint32_t max_frames,
                           uint32_t frame_len, uint32_t hop, hipStream_t s);
void launch_vad_stream(const VadStreamArgs &a, bool sad, hipStream_t s);  // the three passes (sad: 16-bit mid, see k_vad)
void launch_stream_records(const StreamRecArgs &a, uint32_t n, hipStream_t s);
void launch_mfcc(const MfccArgs &a, const MfccMagTab &tab, hipStream_t s);
void launch_mfcc_gen(const MfccArgs &a, hipStream_t s);  // GENERIC front end (k_mfcc_gen.hip)
// the same kernels' per-frame intermediate values (kind = SR_FEAT_*) into feat[B][max_frames][width], MFCC rows into a.mfcc
void launch_mfcc_features(const MfccArgs &a, const MfccMagTab &tab, int kind, uint32_t *feat, hipStream_t s);
void launch_mfcc_gen_features(const MfccArgs &a, int kind, uint32_t *feat, hipStream_t s);
uint32_t mfcc_frames_per_tile(uint32_t frame_len);        // frames one work item of the frame kernel covers
uint32_t mfcc_frames_per_tile_small(uint32_t frame_len, uint32_t which);  // ... of its forms for underfilled launches (MfccArgs::small_tiles - 1)
uint32_t mfcc_resident_workgroups(uint32_t frame_len);  // occupancy x CUs on the current device
void launch_argmin(const DtwArgs &a, hipStream_t s);  // (the DTW launchers: sr_dtw_plan.h)
// generic complex 1024-point Q15 FFT, n arrays (cr4_fft_1024_stm32 semantics)
void launch_fft_q15(const uint32_t *in, uint32_t *out, uint32_t n, const DevTables &t, hipStream_t s);
// magnitude*10 of bins 0..511 of zero-padded real frames: fft() of MFCC.C:27-62.
// frames: [n][160] int16; mag: [n][512]; also writes raw FFT words of bins 512..1023 to raw_hi if non-null
void launch_fft_mag(const int16_t *frames, uint32_t len, uint32_t *mag, uint32_t *raw_hi, uint32_t n,
                    const DevTables &t, hipStream_t s);
// EXTENSION: delta cepstra of B records (frame counts from vad[] or, when non-null, frames[])
void launch_delta_mfcc(const int16_t *mfcc, const sr_vad_rec *vad, const uint32_t *frames, uint32_t B, uint32_t max_frames,
                       uint32_t n_coef, int16_t *delta, hipStream_t s);
// host transport: rows of 12-bit codes packed 2 samples / 3 bytes (row_bytes a multiple of 12) -> u16 rows (out_stride samples)
void launch_unpack12(const void *packed, uint64_t row_bytes, uint16_t *out, uint64_t out_stride, uint32_t buf_len, uint32_t B,
                     hipStream_t s);
// diagnostics: log / sqrt device functions swept directly (see k_math_diag)
void launch_math_diag(const uint32_t *in, uint32_t *out, uint32_t n, const DevTables &t, hipStream_t s);
// diagnostics: fused Mel filterbank term vs the reference's u32 expression, weights [tri_lo, tri_lo + n_tri), E <= e_max
void launch_mel_term_sweep(uint32_t tri_lo, uint32_t n_tri, uint32_t e_max, unsigned long long *bad, hipStream_t s);
int launch_lds_poison(uint32_t seed, hipStream_t s);  // k_misc.hip; returns the bytes of LDS each workgroup filled, < 0 on failure
void launch_mag_fast_sweep(uint32_t n_max, unsigned long long *bad, uint32_t *first_bad, hipStream_t s);
// get_dis (DTW.C:45-62) for n frame pairs
void launch_get_dis(const int16_t *a, const int16_t *b, uint32_t *out, uint32_t n, hipStream_t s);
// dtw_limit (DTW.C:76-109) for n points with explicit statics
void launch_dtw_limit(const uint16_t *xy, uint8_t *out, uint32_t n, int X1, int X2, int in_n, int mdl_n, hipStream_t s);

}  // namespace sr
