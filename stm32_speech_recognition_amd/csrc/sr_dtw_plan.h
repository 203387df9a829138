// sr_dtw_plan.h -- which DTW kernel runs, in what shape, with how much LDS.  Everything that depends only on the template
// store and the device is decided once, when the store is set (plan_dtw, sr_launch.cpp), from the device's LDS figures;
// launch_dtw_auto then only compares the launch's pairs with the plan's thresholds and calls one of the launchers below.
#pragma once
#include <cstdint>
#include <initializer_list>
#include <utility>
#include <vector>

#include "sr_cluster_plan.h"
#include "sr_device.h"

namespace sr {

// LDS of the engine's device (sr_create reads it from the device; the defaults are MI355X's)
struct LdsBudget {
    uint32_t per_cu = 160 * 1024;     // bytes per CU
    uint32_t per_wg = 160 * 1024;     // bytes one workgroup may take
    uint32_t granule = 1280;          // allocation unit (gfx950: 128 per CU)
    uint32_t stage_cap = 150 * 1024;  // what the LDS-staged kernels plan one workgroup with: min(150 KiB, per_wg)
    // Workgroups of `bytes` that fit a CU.  LDS goes out in whole granules: three workgroups fit an MI355X CU only if each
    // stays within 42 granules = 53 760 bytes -- 20 bytes more and the third one silently does not (measured: mean waves per
    // SIMD 5.0 -> 3.3), although hipOccupancyMaxActiveBlocksPerMultiprocessor still reports 3.
    uint32_t wgs_per_cu(size_t bytes) const { return (uint32_t)(per_cu / ((bytes + granule - 1) / granule * granule)); }
};

// the DTW launch plan of one template store (sr_engine::plan)
struct DtwPlan {
    uint32_t lds_u = 0, lds_kc = 0, lds_tie_g = 0, lds_bytes = 0;  // k_dtw_lds: U utterances x Kc templates (U = 0: not staged)
    uint32_t cells_points = 0, cells_bytes = 0;  // k_dtw_cells: most band points of any pair (0 = does not fit) and its LDS
    uint32_t quad_pu = 0, quad_pk = 0, quad_bytes = 0;  // k_dtw_quad: PU utterances x PK templates (PU = 0: does not fit)
    bool quad_neg2 = false;                      // k_dtw_quad's instance with -2 * coefficient template rows (tpl_staged_ok)
    uint64_t cells_pairs = 0, quad_pairs = 0;    // automatic mode: k_dtw_cells up to cells_pairs pairs, then k_dtw_quad up to quad_pairs
};

// Shapes (called by plan_dtw).  U utterances per k_dtw_lds workgroup for K templates / max_frames rows (0 = not staged); the
// development hooks dtw_u / dtw_kc / dtw_tie_g override it.  row_words: packed coefficient pairs per feature row of the
// staged kernel's form: 6 = up to 12 coefficients, 8 = 13..16.
uint32_t dtw_lds_pick_u(uint32_t K, uint32_t max_frames, const LdsBudget &lds, uint32_t *lds_bytes, uint32_t *tie_g, uint32_t *kc,
                        uint32_t row_words = 6);
// the most points of dtw_limit's band any (utterance, template) pair of a store can have (0: not worth setting up).
// by_len: the engine's cache per template length (the frame cap of an engine never changes), so that a store that grows
// slot by slot -- dtw()'s model cache -- pays per new length
uint32_t dtw_cells_max_points(uint32_t max_frames, const uint32_t *frames, const uint8_t *valid, uint32_t K, std::vector<uint32_t> &by_len);
size_t dtw_cells_lds(uint32_t max_frames, uint32_t tpl_rows, uint32_t max_points);
// k_dtw_quad's workgroup: pu utterances x pk templates (pu * pk <= 64 pairs) and its LDS bytes; false = not even 1 x 4 fits
bool dtw_quad_pick(uint32_t K, uint32_t max_frames, uint32_t tpl_rows, uint32_t n_coef, const LdsBudget &lds, uint32_t *pu,
                   uint32_t *pk, uint32_t *lds_bytes);

// Launchers, identical scores in every form: k_dtw_lds / k_dtw_gen / k_dtw (the batch kernels); k_dtw_cells, one workgroup
// per pair (a few hundred pairs); k_dtw_quad, four lanes per pair (a few thousand to ~100 000)
void launch_dtw(const DtwArgs &a, const DtwPlan &p, hipStream_t s);
void launch_dtw_cells(const DtwArgs &a, const DtwPlan &p, hipStream_t s);
void launch_dtw_quad(const DtwArgs &a, const DtwPlan &p, hipStream_t s);
void launch_dtw_dp(const DtwArgs &a, uint32_t lanes, const LdsBudget &lds, hipStream_t s);  // opt-in full-DP scorer (sr_set_dp_lanes)
// two-pass rescoring: the full-DP score of the pairs marked in marks[template rank][row] (one byte per pair, mark_stride bytes
// per template, a multiple of 16, rows past a.B zero), frame counts at a.in_frames[row * frames_stride]; unmarked pairs untouched
void launch_dtw_dp_sparse(const DtwArgs &a, const uint8_t *marks, uint32_t mark_stride, uint32_t frames_stride, const uint32_t *tpl_rank,
                          uint32_t lanes, const LdsBudget &lds, hipStream_t s);

// Word spotter (k_spot.hip).  LDS of a workgroup: the template image (32-byte rows) and one boundary column per wave (two
// (cost, start) pairs = 16 bytes per row), both as long as the store's longest template.
constexpr uint32_t kSpotWaves = 4;  // waves = chunks per workgroup
inline uint32_t spot_lds_bytes(uint32_t tpl_len) { return tpl_len * (32u + kSpotWaves * 16u); }
inline uint32_t spot_max_tpl(const LdsBudget &lds) { return lds.stage_cap / spot_lds_bytes(1); }
// How the end frames of a row are cut into chunks (SpotArgs).  cols = 0: the default, eight times the longest template (the
// lead-in of 2M - 2 columns a chunk recomputes is then a quarter of its own columns), 256 at least.  A chunk never straddles
// a window edge: windows no longer than that are packed whole into a chunk, longer ones are cut into chunks of their own.
struct SpotGeom {
    uint32_t n_win, win, chunk_cols, n_chunks, split, per;
};
inline SpotGeom spot_geom(uint32_t tpl_len, uint32_t max_frames, uint32_t win_frames, uint32_t cols)
{
    SpotGeom g;
    g.win = win_frames && win_frames < max_frames ? win_frames : max_frames;
    g.n_win = (max_frames + g.win - 1) / g.win;
    if (!cols) cols = tpl_len * 8u < 256u ? 256u : (tpl_len * 8u + 63u) & ~63u;
    cols = cols > 16383u ? 16383u : cols;
    g.split = g.win > cols;
    if (g.split) {
        g.chunk_cols = cols;
        g.per = (g.win + cols - 1) / cols;  // chunks per window
        g.n_chunks = g.n_win * g.per;
    } else {
        g.per = cols / g.win;               // windows per chunk
        g.chunk_cols = g.per * g.win;
        g.n_chunks = (g.n_win + g.per - 1) / g.per;
    }
    return g;
}

// Connected-word decoder (k_chain.hip): k_spot's workgroup (spot_lds_bytes) and its chunks with one window per row
// (spot_geom with win_frames 0).  Scratch of a row: max_words levels of u64 keys and max_words + 1 levels of u32 prefix costs,
// max_frames + 1 entries each; rows go out in launch groups whose scratch stays within kChainScratch.
constexpr size_t kChainScratch = (size_t)256 << 20;
constexpr uint32_t kChainMaxWords = 16, kChainMaxSlots = 65536u, kChainMaxRows = 65535u;  // levels; 16-bit slot of a key; grid rows
struct ChainPlan {
    SpotGeom g;
    size_t a_row, e_row;  // elements of A (u64) and E (u32) per row
    size_t row_bytes;
    uint32_t rows;        // per launch group
};
inline ChainPlan chain_plan(uint32_t tpl_len, uint32_t max_frames, uint32_t max_words, uint32_t cols, uint32_t forced_rows)
{
    ChainPlan p;
    p.g = spot_geom(tpl_len, max_frames, 0u, cols);
    if (!p.g.split) p.g.chunk_cols = max_frames, p.g.n_chunks = 1;  // the one window of a row fits one chunk
    p.a_row = (size_t)max_words * (max_frames + 1u);
    p.e_row = (size_t)(max_words + 1u) * (max_frames + 1u);
    p.row_bytes = p.a_row * 8u + p.e_row * 4u;
    const size_t fit = kChainScratch / p.row_bytes;
    p.rows = (uint32_t)(fit < 1 ? 1 : fit > kChainMaxRows ? kChainMaxRows : fit);
    if (forced_rows) p.rows = forced_rows < kChainMaxRows ? forced_rows : kChainMaxRows;
    return p;
}

// Full-DP aligner (k_align.hip): one wave = one workgroup per pair.  LDS: the reference image (32-byte rows), the boundary
// column (one word per row) and, when they fit, the predecessor marks: 2 bits per cell, 16 reference rows per word, mark_w
// words per input column (odd, so that the lanes' words spread over the banks).  The marks stay in LDS while
// kAlignMinWgs workgroups -- two waves per SIMD -- still fit a CU; otherwise they go to global scratch, and a call is cut
// into launches of as many pairs as kAlignScratch holds.
constexpr uint32_t kAlignMinWgs = 8;
constexpr size_t kAlignScratch = (size_t)256 << 20;
constexpr uint32_t kAlignMaxPairs = 1u << 20;  // pairs of one launch at most
struct AlignPlan {
    uint32_t mark_w, mark_words;  // words per column, per pair
    uint32_t lds_bytes;           // of one workgroup
    bool lds_marks;
    uint32_t pair_bytes;          // global scratch per pair: the marks (0 in LDS) + `extra`
    uint32_t pairs;               // per launch
};
inline AlignPlan align_plan(uint32_t max_frames, uint32_t ref_rows, const LdsBudget &lds, size_t extra, bool force_global, uint32_t forced_pairs)
{
    AlignPlan p;
    const uint32_t n_cap = max_frames < SR_ALIGN_MAX_FRAMES ? max_frames : SR_ALIGN_MAX_FRAMES;
    p.mark_w = ((ref_rows + 15u) / 16u) | 1u;
    p.mark_words = n_cap * p.mark_w;
    const uint32_t base = ref_rows * 36u, with = base + p.mark_words * 4u;
    p.lds_marks = !force_global && with <= lds.stage_cap && lds.wgs_per_cu(with) >= kAlignMinWgs;
    p.lds_bytes = p.lds_marks ? with : base;
    p.pair_bytes = (uint32_t)((p.lds_marks ? 0u : p.mark_words * 4u) + extra);
    const size_t fit = p.pair_bytes ? kAlignScratch / p.pair_bytes : kAlignMaxPairs;
    p.pairs = (uint32_t)(fit < 1 ? 1 : fit > kAlignMaxPairs ? kAlignMaxPairs : fit);
    if (forced_pairs) p.pairs = forced_pairs < kAlignMaxPairs ? forced_pairs : kAlignMaxPairs;
    return p;
}

// Word-model clustering (k_cluster.hip): a workgroup of kClusterWaves waves (sr_cluster_plan.h) shares one centroid image
// (32-byte rows) and gives every wave a boundary column (one word per row).  At SR_ALIGN_MAX_FRAMES rows that is 48 KiB,
// within every device's per-workgroup LDS the engine accepts; at word-sized centroids (100 rows: 4 granules) the LDS never
// limits the waves of a CU.
inline uint32_t cluster_lds_bytes(uint32_t cen_rows) { return cen_rows * (32u + kClusterWaves * 4u); }
inline bool cluster_fits(uint32_t cen_rows, const LdsBudget &lds) { return cluster_lds_bytes(cen_rows) <= lds.stage_cap; }

// sr_create: let every instance of the file's kernels take up to `bytes` of dynamic LDS (the default limit is 64 KiB);
// returns the name of an instance that was refused, or nullptr
const char *dtw_lds_allow_lds(uint32_t bytes);
const char *dtw_cells_allow_lds(uint32_t bytes);
const char *dtw_quad_allow_lds(uint32_t bytes);
const char *dtw_dp_allow_lds(uint32_t bytes);
const char *spot_allow_lds(uint32_t bytes);
const char *spot_live_allow_lds(uint32_t bytes);
const char *align_allow_lds(uint32_t bytes);
const char *chain_allow_lds(uint32_t bytes);
const char *chain_live_allow_lds(uint32_t bytes);
const char *gram_allow_lds(uint32_t bytes);
const char *gram_live_allow_lds(uint32_t bytes);
const char *span_allow_lds(uint32_t bytes);
const char *cluster_allow_lds(uint32_t bytes);
const char *forced_allow_lds(uint32_t bytes);
const char *onepass_allow_lds(uint32_t bytes);
const char *onepass_live_allow_lds(uint32_t bytes);
const char *onepass_gram_allow_lds(uint32_t bytes);
const char *onepass_gram_live_allow_lds(uint32_t bytes);
inline const char *allow_dynamic_lds(std::initializer_list<std::pair<const void *, const char *>> kernels, uint32_t bytes)
{
    for (const auto &k : kernels)
        if (hipFuncSetAttribute(k.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return k.second;
    return nullptr;
}

}  // namespace sr
