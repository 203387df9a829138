/*
 * sr_engine.h -- C ABI of the MI355X-native isolated-word recognition engine.
 *
 * Drop-in boundary for the hot path of gk969/stm32-speech-recognition
 * (noise_atap -> VAD -> get_mfcc/fft/cr4_fft_1024_stm32 -> dtw -> spch_recg).
 * The reference has no plugin API; its boundary is the set of C functions that
 * Src/APP/main.c calls (main.c:121-138, 249-296).  This header declares
 *
 *   1. the batched engine API the benchmark drives (no reference counterpart:
 *      the firmware recognises one utterance at a time), and
 *   2. the reference's own scalar entry points, same names / argument meaning /
 *      sentinel error behaviour, each executed as a 1-item dispatch of the same
 *      HIP kernels (there is NO CPU fallback anywhere in this library: every
 *      entry point fails with SR_ERR_NO_DEVICE if no gfx950 device is usable).
 *
 * Plain C types only; every pointer is caller-owned.  Thread-safety: distinct
 * sr_engine handles are independent; one handle must not be used concurrently.
 * The scalar reference-compatible symbols share one implicit handle and are,
 * like the reference (file-scope statics in MFCC.C:14-15, DTW.C:65-68,
 * main.c:22-25), not re-entrant.
 */
#ifndef SR_ENGINE_H
#define SR_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status / errors */
#define SR_OK 0
#define SR_ERR_NO_DEVICE 1   /* no HIP device / not gfx950 / HIP runtime error */
#define SR_ERR_BAD_CONFIG 2  /* configuration not supported by the kernels */
#define SR_ERR_BAD_ARG 3     /* null pointer, bad alignment, size out of range */
#define SR_ERR_NO_TEMPLATES 4
#define SR_ERR_HIP 5

/* per-utterance status in sr_result.status (the reference's sentinel returns) */
#define SR_ST_OK 0
#define SR_ST_VAD_FAIL 1  /* valid_voice[0].end == NULL            main.c:261-266 */
#define SR_ST_MFCC_FAIL 2 /* frm_num == 0 (segment > max_frames)   main.c:269-274, MFCC.C:103-107 */
#define SR_ST_SEG_OOB 3   /* segment starts at sample < 1: the reference would read before VcBuf (MFCC.C:119) */

#define SR_DIS_ERR 0xFFFFFFFFu /* dis_err / dis_max, DTW.H:4-5 */
#define SR_SAVE_MASK 12345u    /* save_mask, Flash.H:11 */

/* ------------------------------------------------------------------ configuration
 * The reference's compile-time constants (ADC.H:7-11, VAD.H:4-8, MFCC.H:7-16) as a run-time configuration.  Two front ends
 * have specialised kernels:
 *   reference   fs 8000, 20/10 ms framing (160/80 samples), nfft 1024, 24 Mel, 12 MFCC   (the firmware's constants)
 *   extension   fs 16000, 20/10 ms framing (320/160 samples), nfft 512, 40 Mel, 12 MFCC   (no reference counterpart)
 * Every other accepted configuration runs the GENERIC front end (same arithmetic rules, tables from the same formulas, about
 * 2.3x slower per frame; no reference counterpart for the constants):
 *   nfft 1024; fs a multiple of 4000 Hz; frame_time_ms = 2 * frame_mov_ms with a frame of 160, 240, 256, 320, 400 or 512
 *   samples; n_mel even, 4..64; n_coef 1..16 (feature records are n_coef wide everywhere: mfcc[B][max_frames][n_coef],
 *   template rows, slot images; sr_get_mdl_batch and the full-DP scorer require 12).
 * Anything else: SR_ERR_BAD_CONFIG.  Free in every configuration: max_frames (2..16383), noise_len_ms (a multiple of 30 ms
 * that holds whole frames), max_seg (1..3), device. */
typedef struct sr_config {
    uint32_t fs;            /* ADC.H:7       8000 */
    uint32_t frame_time_ms; /* VAD.H:5       20  -> frame_len 160 */
    uint32_t frame_mov_ms;  /* VAD.H:6       10  -> hop 80 */
    uint32_t nfft;          /* MFCC.H:8      1024 */
    uint32_t n_mel;         /* MFCC.H:12     24 */
    uint32_t n_coef;        /* MFCC.H:13     12 */
    uint32_t max_frames;    /* MFCC.H:15-16  119 in the firmware; runtime cap here (<= 16383) */
    uint32_t noise_len_ms;  /* ADC.H:10      300 -> atap_len 2400 */
    uint32_t max_seg;       /* VAD.H:4       3 */
    int32_t device;         /* HIP device ordinal; -1 = current device */
} sr_config;

/* adaptive thresholds, VAD.H:10-16 (same field order and widths) */
typedef struct sr_atap {
    uint32_t mid_val;
    uint16_t n_thl;
    uint16_t z_thl;
    uint32_t s_thl;
} sr_atap;

#define SR_MAX_SEG 3
/* what the VAD stage leaves per utterance (device- or host-resident), 48 bytes */
typedef struct sr_vad_rec {
    sr_atap atap;                /* noise_atap output */
    int32_t seg[2 * SR_MAX_SEG]; /* start/end sample offsets of up to 3 segments, -1 = NULL (VAD.H:18-22) */
    uint32_t frm_num;            /* frames of segment 0 per MFCC.C:102-107 (0 on any failure) */
    uint32_t status;             /* SR_ST_* */
    uint32_t _pad;               /* written as 0 by every call that writes the record */
} sr_vad_rec;

/* recognition record, 16 bytes: the argmin of main.c:276-295 */
typedef struct sr_result {
    uint32_t best_tpl; /* template slot of the first minimum (strict <, main.c:285) */
    uint32_t min_dis;  /* *mtch_dis; SR_DIS_ERR if nothing matched */
    uint32_t frm_num;  /* frames of segment 0 */
    uint32_t status;   /* SR_ST_* */
} sr_result;

typedef struct sr_engine sr_engine;

/* ------------------------------------------------------------------ lifecycle */
void sr_default_config(sr_config *cfg); /* the reference's compile-time constants */
int sr_create(const sr_config *cfg, sr_engine **out);
void sr_destroy(sr_engine *h);
const char *sr_last_error(void); /* thread-local text of the last failure */

/* Host-only (touches no device): the constant tables sr_create generates for cfg, for inspection and for
 * diffing against the reference's pasted tables (MFCC_Arg.h:6-44: hamm, tri_cen, tri_odd, tri_even, dct_arg;
 * cr4_fft_1024_stm32.s:285-629: the (Kr', Ki) coefficient columns).  Every pointer may be NULL. */
typedef struct sr_tables {
    uint16_t *hamm;     /* [frame_len]       hamm[],    MFCC_Arg.h:6-9 */
    uint16_t *tri_cen;  /* [n_mel]           tri_cen[], MFCC_Arg.h:11-15 */
    uint16_t *tri_even; /* [nfft / 2]        tri_even[] */
    uint16_t *tri_odd;  /* [nfft / 2]        tri_odd[] */
    int8_t *dct;        /* [n_coef * n_mel]  dct_arg[] */
    int16_t *tw_kr;     /* [1020]            first  DCW column of the ST coefficient table, in table order */
    int16_t *tw_ki;     /* [1020]            second DCW column */
    uint32_t *log_thr;  /* [2220]            log_thr[m] = min{n : (u32)(log((double)n)*100) >= m} (host libm), [2219] = sentinel */
} sr_tables; /* layout frozen (eight pointers): further tables get their own entry point, like sr_build_tie_table below, so a
              * caller compiled against an older header never hands over a shorter struct than the library reads */
int sr_build_tables(const sr_config *cfg, const sr_tables *out);
/* Host-only: the tie-threshold table of the staged DTW kernel, out[32768]:
 * DTW.C:59,156-184: T(g) = g*(g+2) + out[g] = min{d : (u32)sqrtf((float)d) >= g + 1}  (independent of the front end) */
int sr_build_tie_table(int8_t *out);
/* The log step table is built with the run-time host's libm `log` -- the expression MFCC.C:168 evaluates -- and compared with
 * the positions the library ships (csrc/sr_log_thr_ref.inc: the libm the golden fixtures were generated with).  If they
 * differ (a libm whose log is off in the last bit at an integer crossing of log(n)*100) the SHIPPED table is used, sr_create
 * still succeeds, sr_last_error() holds a warning, and this returns the number of differing entries of the last
 * sr_create / sr_build_tables of the process (0 = this host agrees). */
int sr_log_table_mismatches(void);
/* The magnitude stage of the reference front end's frame kernel, (u32)(sqrtf(re^2+im^2)*10) (MFCC.C:56-58), takes the
 * uncorrected v_sqrt_f32 on frames whose largest re^2+im^2 is at most 70 171: equal to the exact form there on gfx950, a
 * property of the chip that sr_create re-checks on the device it runs on by sweeping the whole range.  Returns the bound
 * in use for this engine: 70171 after a clean sweep, 0 (every frame takes the exactly corrected root; sr_last_error()
 * holds a warning from sr_create) otherwise, and for front ends whose kernels do not use the form. */
uint32_t sr_mag_cheap_bound(const sr_engine *h);
/* Host-only (touches no device): frames whose largest re^2+im^2 is at most 26 843 (the QUIET tier) take their magnitudes from
 * a table, t[n] = (u32)(sqrtf((float)n) * 10) << 2 -- MFCC.C:58 evaluated on the host, shifted so that t*t is the operand of
 * the fused filterbank term.  Copies the first min(n, length) entries to out (may be NULL) and returns the length, 26 844. */
uint32_t sr_mag_table(uint16_t *out, uint32_t n);

/* ------------------------------------------------------------------ template store
 * The firmware keeps templates as v_ftr_tag images in MCU flash at a 4 KiB stride
 * (Flash.H:11-20, MFCC.H:18-25: u16 save_sign | u16 frm_num | s16 mfcc[]), and
 * spch_recg scans every slot in address order (main.c:279-291). */
int sr_set_templates(sr_engine *h, const void *store, uint32_t n_slots, uint32_t stride_bytes);
/* dense batched layout: mfcc[k*tpl_stride + frame*n_coef + c]; valid[k]!=0 <=> save_sign==12345 */
int sr_set_templates_dense(sr_engine *h, const int16_t *mfcc, const uint32_t *frames, const uint8_t *valid,
                           uint32_t n_templates, uint32_t tpl_stride);
uint32_t sr_num_templates(const sr_engine *h);
/* Template training = save_mdl (main.c:121-138): capture i -> noise_atap/VAD/get_mfcc -> slot[i] of the
 * host store image exactly as save_ftr_mdl programs it (Flash.C:17-67: slot erased to 0xFF, then
 * save_mask | frm_num | frm_num*12 coefficients).  status[i] (optional): 0 save_ok, 1 VAD_fail,
 * 2 MFCC_fail (main.c:38-40), 3 SR_ST_SEG_OOB; failed captures leave their slot untouched. */
int sr_train_store(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t n,
                   const uint32_t *slot, void *store, uint32_t n_slots, uint32_t stride_bytes, uint32_t *status);

/* ------------------------------------------------------------------ batched recognition
 * B capture buffers of buf_len samples, buffer b at pcm + b*pcm_stride (in samples).
 * Outputs (each may be NULL except results):
 *   results[B], scores[B*K] (cur_dis of every slot, main.c:283), mfcc[B*max_frames*n_coef]
 *   (frame-major, rows >= frm_num zeroed), vad[B].
 *
 * sr_recognize_batch:      HOST buffers; stages them through HBM (PCIe-inclusive).  HOST capture buffers of every
 *                          entry point need only the 2-byte alignment of their samples and take any
 *                          pcm_stride >= buf_len, odd ones included; nothing outside [0, buf_len) of a row is read.
 * sr_recognize_batch_dev:  DEVICE buffers already resident in HBM, enqueued on `stream`
 *                          (a hipStream_t; NULL = default stream), asynchronous.
 *                          pcm must be 16-byte aligned and pcm_stride a multiple of 8.
 */
int sr_recognize_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                       sr_result *results, uint32_t *scores, int16_t *mfcc, sr_vad_rec *vad);
int sr_recognize_batch_dev(sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                           sr_result *d_results, uint32_t *d_scores, int16_t *d_mfcc, sr_vad_rec *d_vad,
                           void *stream);
/* sr_recognize_batch for HOST callers whose captures are 12-bit ADC codes (ADC.H:7-11: the firmware's converter), packed
 * two samples in three bytes: sample 2i = b[3i] | (b[3i+1] & 0x0F) << 8, sample 2i+1 = b[3i+1] >> 4 | b[3i+2] << 4; row b
 * starts at packed + b*row_stride_bytes and holds ceil(buf_len / 2) * 3 bytes.  The host-buffer path is PCIe-bound
 * (INTEGRATION.md 2); this moves 25 % fewer bytes and unpacks on the device.  Same results as the u16 call on the same codes. */
int sr_recognize_batch_packed12(sr_engine *h, const uint8_t *packed, uint64_t row_stride_bytes, uint32_t buf_len, uint32_t B,
                                sr_result *results, uint32_t *scores, int16_t *mfcc, sr_vad_rec *vad);

/* Multi-segment recognition: every segment the VAD returns (up to max_seg, VAD.H:4) is matched like segment 0.
 * The firmware stops at segment 0 (main.c:268); this is an extension with segment-major outputs:
 * results[s*B + b], scores[(s*B + b)*K + k]; a segment that does not exist has status SR_ST_VAD_FAIL. */
int sr_recognize_segments_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                                sr_result *results, uint32_t *scores, sr_vad_rec *vad);
int sr_recognize_segments_batch_dev(sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t buf_len,
                                    uint32_t B, sr_result *d_results, uint32_t *d_scores, sr_vad_rec *d_vad,
                                    void *stream);

/* Stream recognition: every word of recordings of any length.  EXTENSION, NO REFERENCE COUNTERPART: the firmware's VAD
 * stops after max_vc_con = 3 segments (VAD.H:4, VAD.C:203) of a buffer of at most 65 535 samples.  Per recording b the
 * segmentation is exactly VAD() with max_vc_con unbounded over its len[b] samples (VAD.C:121-217; state carried from frame to
 * frame as there, never reset between segments), thresholds from noise_atap over its first noise_len samples (VAD.C:22-71)
 * unless given.  One record per segment start, stream-major, then by start; a segment the recording ended inside (state 2
 * or 3) has end = -1 (what VAD.C leaves in valid_voice[n].end) and is never recognised; a recording that ends in the onset
 * (state 1) reports nothing for that run.  frm_num and the recognition status follow segment selection to the letter:
 * end < 0 -> SR_ST_VAD_FAIL, start < 1 -> SR_ST_SEG_OOB, else the u16-wrapping frame count of MFCC.C:102-107, more than
 * max_frames -> SR_ST_MFCC_FAIL.  cfg.max_seg does not limit these calls.  Argument rules: those of sr_vad_batch, plus
 * len[b] <= buf_len and, without atap_in, len[b] >= the noise head and > frame_len (the host form checks them; the device
 * form clamps d_len[b] to buf_len and reads nothing beyond it). */
typedef struct sr_stream_seg { /* 16 bytes */
    uint32_t stream;           /* recording index b */
    int32_t start;             /* sample offset in recording b (VAD.C:178) */
    int32_t end;               /* sample offset (VAD.C:201); -1: the recording ended inside this segment */
    uint32_t frm_num;          /* frames of the segment per MFCC.C:102-107, 0 on failure */
} sr_stream_seg;
/* DEVICE buffers, asynchronous on `stream`.  Recording b is d_pcm + b*pcm_stride, d_len[b] <= buf_len samples long
 * (d_len NULL: every recording is buf_len long).  d_atap_in NULL: noise_atap on each recording's head.
 * d_seg_offsets[B+1] (required): exclusive offsets of each recording's segments in the output, d_seg_offsets[B] = the
 * TRUE total, which may exceed max_segs.  Only records with index < max_segs are written.  d_atap[B] optional. */
int sr_stream_segments_dev(sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t buf_len,
                           const uint32_t *d_len, uint32_t B, const sr_atap *d_atap_in, uint32_t max_segs,
                           sr_stream_seg *d_segs, uint32_t *d_seg_offsets, sr_atap *d_atap, void *stream);
/* The same, then every written segment recognised like segment 0 of sr_recognize_batch_dev:
 * d_results[max_segs], d_scores[max_segs*K], d_mfcc[max_segs*max_frames*n_coef] (scores, mfcc optional).
 * Result slots in [total, max_segs) are written as failed records (SR_ST_VAD_FAIL, SR_DIS_ERR, frm_num 0). */
int sr_recognize_stream_dev(sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t buf_len,
                            const uint32_t *d_len, uint32_t B, const sr_atap *d_atap_in, uint32_t max_segs,
                            sr_stream_seg *d_segs, uint32_t *d_seg_offsets, sr_result *d_results, uint32_t *d_scores,
                            int16_t *d_mfcc, void *stream);
/* HOST buffers: copy in, run, copy out.  *n_segs = the true total; it syncs on the count, so the recognition launches cover
 * exactly min(total, max_segs) records (outputs past them are not written).  len, atap_in, results, scores, mfcc may be
 * NULL (results NULL: segmentation only). */
int sr_recognize_stream(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, const uint32_t *len,
                        uint32_t B, const sr_atap *atap_in, uint32_t max_segs, sr_stream_seg *segs, uint32_t *seg_offsets,
                        sr_result *results, uint32_t *scores, int16_t *mfcc, uint32_t *n_segs);

/* ------------------------------------------------------------------ words instead of slots: N-best
 * The firmware enrols every command ftr_per_comm = 4 times (Flash.H:15) and ends spch_recg with min_comm /= ftr_per_comm
 * (main.c:292): its answer is a WORD, the slot scan's a template slot.  EXTENSION of the result format (no score, no
 * existing record and no existing call changes): per score row the n_best best words, each with its best slot, that slot's
 * distance and the number of its slots that matched at all -- the runner-up for a rejection margin, a short candidate list
 * for a later stage -- reduced on the device from the u32 scores[.][K] rows the slot scan reads.
 *
 * Word map (host state of an engine; the grouping of the slots by word is built once per map and store and uploaded):
 *   word_of_slot != NULL  one label per slot, any u32 except SR_NO_WORD; sparse, unordered, slots of a word need not be
 *                         adjacent.  n_slots must equal sr_num_templates(h) when an N-best call runs; otherwise that call
 *                         fails with SR_ERR_BAD_ARG and writes nothing.  slots_per_word is ignored.
 *   word_of_slot == NULL  the firmware's rule word = slot / slots_per_word (main.c:292) for whatever store is set;
 *                         slots_per_word >= 1, n_slots is ignored.
 * An engine that never had a map set behaves as (NULL, 0, 1): word = slot, a plain template N-best.  Setting a template
 * store leaves the map alone.  The call waits for the device (a kernel in flight may be reading the previous grouping). */
#define SR_NO_WORD 0xFFFFFFFFu
#define SR_NBEST_MAX 16
int sr_set_word_map(sr_engine *h, const uint32_t *word_of_slot, uint32_t n_slots, uint32_t slots_per_word);
/* host-only (touches no device): the grouping sr_set_word_map uploads.  order[n_slots] = the slots grouped by word
 * (ascending slot inside a word, words by their first slot), group_start[*n_words + 1] = where each word's slots start in
 * order, word_id[*n_words] = the caller's label of each word (slot / slots_per_word without a map); any output pointer may
 * be NULL; returns SR_OK / SR_ERR_BAD_ARG (n_slots 0, a label SR_NO_WORD, slots_per_word 0 without a map) */
int sr_word_groups(const uint32_t *word_of_slot, uint32_t n_slots, uint32_t slots_per_word, uint32_t *order,
                   uint32_t *group_start, uint32_t *word_id, uint32_t *n_words);
/* One candidate.  The definition is the firmware's scan (main.c:283-289), repeated: a word's distance is the minimum of its
 * slots' cur_dis under strict < in slot order; a word with no slot below dis_err is no candidate; candidates are ranked by
 * (dis, slot) ascending -- what re-running the scan gives after removing the winning word each time.  Entries past the last
 * candidate are {SR_NO_WORD, 0xFFFFFFFF, SR_DIS_ERR, 0}.  So entry 0 has slot == best_tpl and dis == min_dis of the row's
 * sr_result whenever min_dis != SR_DIS_ERR; a failed record (VAD / MFCC / SEG_OOB) and one that matched nothing have no
 * candidate at all (sr_result keeps its firmware form, best_tpl 0; the list does not invent a slot 0). */
typedef struct sr_nbest_entry { /* 16 bytes */
    uint32_t word;              /* caller's label; SR_NO_WORD: no such candidate */
    uint32_t slot;              /* the word's best slot: first minimum in slot order; 0xFFFFFFFF if none */
    uint32_t dis;               /* that slot's cur_dis; SR_DIS_ERR if none */
    uint32_t count;             /* slots of this word whose distance != SR_DIS_ERR; 0 if none */
} sr_nbest_entry;
/* Stage level: any u32 score matrix rows[n_rows][K] in sr_dtw_batch_dev's layout (also the segment-major matrix of
 * sr_recognize_segments_batch_dev with n_rows = max_seg*B, and sr_dtw_dp_batch_dev's).  n_best 1..SR_NBEST_MAX;
 * d_nbest[n_rows*n_best] (required; each row's n_best entries are written whole), d_n_matched[n_rows] (optional) = the
 * true number of candidates of the row, which may exceed n_best.  DEVICE form: asynchronous on `stream`. */
int sr_nbest_batch_dev(sr_engine *h, const uint32_t *d_scores, uint32_t n_rows, uint32_t n_best, sr_nbest_entry *d_nbest,
                       uint32_t *d_n_matched, void *stream);
int sr_nbest_batch(sr_engine *h, const uint32_t *scores, uint32_t n_rows, uint32_t n_best, sr_nbest_entry *nbest,
                   uint32_t *n_matched);
/* Whole path: sr_recognize_batch[_dev] (same arguments, same rules, the same bytes in every output) plus
 * d_nbest[B*n_best] and d_n_matched[B] (optional).  The device form stays ONE asynchronous operation on the caller's stream:
 * the reduction runs per chunk behind that chunk's slot scan.  The HOST form is sr_recognize_batch as it stands (outputs
 * copied back included) followed by ONE reduction over all B score rows in the engine's scratch and one more copy back. */
int sr_recognize_nbest_batch_dev(sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                                 uint32_t n_best, sr_nbest_entry *d_nbest, uint32_t *d_n_matched, sr_result *d_results,
                                 uint32_t *d_scores, int16_t *d_mfcc, sr_vad_rec *d_vad, void *stream);
int sr_recognize_nbest_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                             uint32_t n_best, sr_nbest_entry *nbest, uint32_t *n_matched, sr_result *results,
                             uint32_t *scores, int16_t *mfcc, sr_vad_rec *vad);
/* Stream: sr_recognize_stream[_dev] plus n_best, nbest[max_segs*n_best] (required) and n_matched[max_segs] (optional).
 * Device form: result slots in [total, max_segs) get empty entries and n_matched 0 (as d_results is padded there).
 * Host form: exactly min(total, max_segs) rows are written; results may be NULL. */
int sr_recognize_stream_nbest_dev(sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t buf_len,
                                  const uint32_t *d_len, uint32_t B, const sr_atap *d_atap_in, uint32_t max_segs,
                                  sr_stream_seg *d_segs, uint32_t *d_seg_offsets, uint32_t n_best, sr_nbest_entry *d_nbest,
                                  uint32_t *d_n_matched, sr_result *d_results, uint32_t *d_scores, int16_t *d_mfcc,
                                  void *stream);
int sr_recognize_stream_nbest(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, const uint32_t *len,
                              uint32_t B, const sr_atap *atap_in, uint32_t max_segs, sr_stream_seg *segs,
                              uint32_t *seg_offsets, uint32_t n_best, sr_nbest_entry *nbest, uint32_t *n_matched,
                              sr_result *results, uint32_t *scores, int16_t *mfcc, uint32_t *n_segs);

/* ------------------------------------------------------------------ second pass: full-DP rescoring of the N-best words
 * EXTENSION, NO REFERENCE COUNTERPART: the classic two-pass recogniser built from the two extensions above and below.  The
 * first pass (the firmware's greedy dtw() walk) names n_best candidate words per row; the second pass gives EVERY slot of
 * every candidate word its full-DP score -- exactly the value sr_dtw_dp_batch_dev writes for that (row, slot), SR_DIS_ERR
 * included -- and ranks the words again, all on the device.  No existing call, record or score changes.
 *
 * Per row, from its feature record, its frame count and an input list of n_best sr_nbest_entry:
 *   candidates  for every input entry with word != SR_NO_WORD and slot < K: the word group that SLOT belongs to under the
 *               engine's current word map (the entry's word field is not trusted any further).  A word named twice counts
 *               once; entries with slot >= K are ignored and nothing is read out of range.
 *   output      what sr_nbest_batch returns, with the same n_best, for a score row that holds the full-DP scores at the
 *               candidate words' slots and SR_DIS_ERR everywhere else: first minimum in slot order inside a word, ranking by
 *               (dis, slot), count = the word's slots with a full-DP score, the tail filled with
 *               {SR_NO_WORD, 0xFFFFFFFF, SR_DIS_ERR, 0}; a word none of whose slots gets a score drops out.
 *               n_rescored[row] = the candidates that survived.
 * Stage level: d_mfcc[n_rows][max_frames][12] (frames[row] <= max_frames, as for sr_dtw_dp_batch_dev); d_in_frames points at
 * the FIRST row's u32 frame count and frames_stride (u32 words, >= 1) leads to the next row's, so one argument serves every
 * record the library emits: 1 for a plain array, 4 for &d_results[0].frm_num and &d_segs[0].frm_num (sr_stream_seg), 6 for
 * sr_live_seg, 12 for &d_vad[0].frm_num (sr_vad_rec).  Stream and live callers rescore with this call on the d_mfcc and
 * d_nbest they already hold.  d_nbest_out[n_rows*n_best] (required) must not be d_nbest_in, which is never written;
 * d_n_rescored[n_rows] is optional; n_rows <= 16 776 960.  DEVICE form: asynchronous on `stream`, no host synchronisation,
 * no read-back; the pair marks and the second-pass score rows live in the engine's scratch.  sr_set_dp_lanes applies, with
 * the same fallbacks and the same values in every form.
 * Errors, before anything is launched or written: SR_ERR_BAD_CONFIG unless n_coef == 12; SR_ERR_BAD_ARG for a null required
 * pointer, n_best outside 1..SR_NBEST_MAX, a word map that does not fit the store, frames_stride 0, d_nbest_out ==
 * d_nbest_in, templates too long for the LDS-staged DP kernel; SR_ERR_NO_TEMPLATES. */
int sr_rescore_nbest_dp_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride,
                            uint32_t n_rows, uint32_t n_best, const sr_nbest_entry *d_nbest_in, sr_nbest_entry *d_nbest_out,
                            uint32_t *d_n_rescored, void *stream);
int sr_rescore_nbest_dp(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                        uint32_t n_best, const sr_nbest_entry *nbest_in, sr_nbest_entry *nbest_out, uint32_t *n_rescored);
/* Whole path: sr_recognize_nbest_batch[_dev] (same arguments, the same bytes in every output) plus rescored[B*n_best]
 * (required) and n_rescored[B] (optional) = the stage-level call on that call's mfcc, vad[].frm_num and nbest.  The
 * first-pass list stays an output but may be NULL here (it then lives in the engine's scratch).  The device form stays ONE
 * asynchronous operation: the second pass runs per chunk, on that chunk's stream, behind its first-pass reduction.  The
 * host form is sr_recognize_nbest_batch followed by ONE second pass over all B rows in the engine's scratch. */
int sr_recognize_rescored_batch_dev(sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                                    uint32_t n_best, sr_nbest_entry *d_nbest, uint32_t *d_n_matched, sr_nbest_entry *d_rescored,
                                    uint32_t *d_n_rescored, sr_result *d_results, uint32_t *d_scores, int16_t *d_mfcc,
                                    sr_vad_rec *d_vad, void *stream);
int sr_recognize_rescored_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                                uint32_t n_best, sr_nbest_entry *nbest, uint32_t *n_matched, sr_nbest_entry *rescored,
                                uint32_t *n_rescored, sr_result *results, uint32_t *scores, int16_t *mfcc, sr_vad_rec *vad);

/* ------------------------------------------------------------------ live sessions: chunked audio, VAD state carried
 * EXTENSION, NO REFERENCE COUNTERPART, like stream recognition.  A session owns n_channels channels; audio arrives in pushes
 * of at most chunk_max samples per channel, and the session keeps each channel's VAD state and a ring of its recent samples
 * on the device between calls.  THE RULE: let X_c be everything pushed to channel c since it was opened or last ended.  After
 * pushing it in ANY chunking and ending the channel, the records the session emitted for c equal what sr_recognize_stream
 * returns for X_c as one recording with len = |X_c| -- thresholds by the same rule (noise_atap over the first noise_len
 * samples, or those given at open), same order, start, end, frm_num, sr_result, score row, MFCC rows and N-best entries,
 * byte for byte -- except for the record type (64-bit offsets) and ONE DEVIATION: a segment of 65 536 frames or more always
 * fails with SR_ST_MFCC_FAIL (frm_num 0).  The u16-wrapped count of MFCC.C:102 would pass the max_frames cap there and read
 * samples the ring no longer holds (sr_mfcc_batch_status documents a deviation of the same kind).
 *
 * Frame j of a channel is consumed as soon as MORE than j*hop + frame_len samples have arrived (the loop bound of VAD.C:121).
 * Without given thresholds a channel consumes nothing until noise_len samples have arrived; they are then computed once over
 * that head and frames are taken from 0 on.  A push emits the segments whose END event (VAD.C:198-207) falls into the frames
 * it consumed, by ascending channel, then ascending start (deterministic).  Records are never dropped: a push whose max_segs
 * is below sr_live_event_bound() returns SR_ERR_BAD_ARG, writes nothing and changes no state; so does every other failed
 * call.  Templates and the word map may change between pushes.  The session uses its engine's scratch buffers: the engine's
 * one-caller-at-a-time rule covers its sessions. */
typedef struct sr_live sr_live;
typedef struct sr_live_seg {   /* 24 bytes */
    uint32_t channel;
    uint32_t frm_num;          /* as sr_stream_seg.frm_num (0 on failure; see the deviation above) */
    int64_t start;             /* sample offset since the channel's recording began (VAD.C:178) */
    int64_t end;               /* VAD.C:201; -1: the recording was ended inside this segment */
} sr_live_seg;
/* host-only, no device (like sr_dtw_geometry): out[0] = ring samples per channel -- whole hop-sized blocks covering
 * max((max_frames + s_durmax + 4)*hop + 8 + chunk_max, noise_len + frame_len + chunk_max); out[1] = most records one channel
 * can emit in one push of chunk_max samples; out[2] = device bytes per channel.  chunk_max 1..2^24. */
int sr_live_geometry(const sr_config *cfg, uint32_t chunk_max, uint32_t out[3]);
/* host-only: most END events of the VAD's endpoint state machine in `frames` consecutive frames, from any entering state:
 * 0 for no frame, else 1 + (frames - 1) / (max(v_durmin, 2) + max(s_durmax, 2)) -- what the two bounds are made of */
uint32_t sr_live_events_in_frames(uint32_t v_durmin, uint32_t s_durmax, uint64_t frames);
/* atap_in: HOST [n_channels] thresholds, or NULL (noise_atap over each channel's head, again after every sr_live_end) */
int sr_live_open(sr_engine *h, uint32_t n_channels, uint32_t chunk_max, const sr_atap *atap_in, sr_live **out);
void sr_live_close(sr_live *l); /* before sr_destroy of its engine; waits for the session's last push */
/* host-only: upper bound on the records THIS push can emit, from the counts alone (n NULL: n_all each) */
uint32_t sr_live_event_bound(const sr_live *l, const uint32_t *n, uint32_t n_all);
/* One push.  n: HOST array [n_channels] in both forms, 0 <= n[c] <= chunk_max (any number, 0 = silent in this push); NULL:
 * n_all each.  Channel c's samples are d_pcm + c*pcm_stride.  DEVICE form: d_pcm 16-byte aligned, pcm_stride a multiple of 8;
 * one asynchronous operation on `stream`.  d_segs[max_segs], d_count[1] (the true total, <= max_segs) are required;
 * d_results NULL and n_best 0: segmentation only.  Recognition is launched over all max_segs slots, those in
 * [*d_count, max_segs) padded as failed records as sr_recognize_stream[_nbest]_dev pads them.  n_best 0 or 1..SR_NBEST_MAX
 * with d_nbest[max_segs*n_best] (required then) and d_n_matched[max_segs] (optional); d_scores, d_mfcc optional.
 * HOST form: the same with host buffers; syncs on the count and writes exactly *n_segs rows of every output. */
int sr_live_push_dev(sr_live *l, const uint16_t *d_pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                     uint32_t max_segs, sr_live_seg *d_segs, uint32_t *d_count, uint32_t n_best, sr_nbest_entry *d_nbest,
                     uint32_t *d_n_matched, sr_result *d_results, uint32_t *d_scores, int16_t *d_mfcc, void *stream);
int sr_live_push(sr_live *l, const uint16_t *pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all, uint32_t max_segs,
                 sr_live_seg *segs, uint32_t n_best, sr_nbest_entry *nbest, uint32_t *n_matched, sr_result *results,
                 uint32_t *scores, int16_t *mfcc, uint32_t *n_segs);
/* The listed channels' recordings end here: a channel inside a segment (state speech or tail) reports {start, -1}, in the
 * order listed; then the channel is as freshly opened.  segs[n_ch], *n_segs = records written.  Waits for the device. */
int sr_live_end(sr_live *l, const uint32_t *channels, uint32_t n_ch, sr_live_seg *segs, uint32_t *n_segs);

/* stage-level entry points on DEVICE buffers (same kernels the full path launches).  d_vad records a caller writes itself
 * follow the rules of those sr_vad_batch_dev writes: a failed record (status != 0) has frm_num 0.  The frame kernels
 * (sr_mfcc_batch_dev, sr_frame_features_batch_dev) take seg[0] and frm_num as given and read frm_num frames from seg[0] - 1
 * on; the DTW, full-DP and delta forms treat a record with status != 0 as failed whatever frm_num it carries. */
int sr_vad_batch_dev(sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                     sr_vad_rec *d_vad, void *stream);
int sr_mfcc_batch_dev(sr_engine *h, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t B, const sr_vad_rec *d_vad,
                      int16_t *d_mfcc, void *stream);
int sr_dtw_batch_dev(sr_engine *h, const int16_t *d_mfcc, const sr_vad_rec *d_vad, uint32_t B, uint32_t *d_scores,
                     sr_result *d_results, void *stream);

/* stage-level entry points on HOST buffers (copy in, launch, copy out) */
int sr_vad_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                 sr_vad_rec *vad);
/* MFCC of segment [start[b], end[b]) of buffer b with mid value mid[b]; frm_num[b] receives the frame count */
int sr_mfcc_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                  const int32_t *start, const int32_t *end, const uint32_t *mid, int16_t *mfcc, uint32_t *frm_num);
/* The same with PER-RECORD failure, as get_mfcc has it (MFCC.C:102-107: a segment shorter than a frame underflows the u32
 * frame count, which then exceeds vv_frm_max -> frm_num = 0): a bad record yields frm_num[b] = 0, an all-zero MFCC record
 * and status[b] = SR_ST_SEG_OOB (start < 1, end beyond the buffer, end < start) or SR_ST_MFCC_FAIL (shorter than a frame,
 * more than max_frames frames); the other records of the batch are processed.  sr_mfcc_batch is this call with
 * status == NULL.  (One deviation from the literal u16 arithmetic of MFCC.C:102: a segment shorter than a frame always
 * fails; the wrapped count 13107 would pass a cap of 13107 frames or more and read far beyond the segment.) */
int sr_mfcc_batch_status(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                         const int32_t *start, const int32_t *end, const uint32_t *mid, int16_t *mfcc, uint32_t *frm_num,
                         uint32_t *status);
/* Per-frame intermediate values of get_mfcc for segment 0, emitted by the same frame kernels at the point where each value
 * exists (no second transform): feat[b][max_frames][width], frame-major, rows >= frm_num (and every row of a failed record)
 * zeroed.  Widths (sr_frame_feature_width): reference front end 512 / 512 / 24 / 24, extension 256 / 256 / 40 / 40,
 * GENERIC nfft/2 for the two spectrum kinds and n_mel for the two Mel kinds; 0 for an unknown kind.
 * The extension front end's FFT words are its 512-point transform's bins (oracle/q15_fft.c), not cr4_fft_1024_stm32's.
 * LOGMEL of a Mel energy of 0 is 0 (log(0) = -inf; the cast gives 0 on the firmware's and common hosts' compilers). */
#define SR_FEAT_FFT 1    /* u32 x nfft/2: packed (re low16, im high16) words of cr4_fft_1024_stm32's output, bins 0..nfft/2-1 */
#define SR_FEAT_MAG 2    /* u32 x nfft/2: |X|*10 exactly as fft() returns it (MFCC.C:49-60) */
#define SR_FEAT_MEL 3    /* u32 x n_mel:  pow_spct before the log, u32-wrapping terms (MFCC.C:128-162) */
#define SR_FEAT_LOGMEL 4 /* u32 x n_mel:  (u32)(log(pow_spct)*100) as the DCT consumes it (MFCC.C:165-170) */
uint32_t sr_frame_feature_width(const sr_engine *h, int kind);
/* DEVICE buffers, same inputs and alignment rules as sr_mfcc_batch_dev; d_mfcc (may be NULL) receives the MFCC rows of the
 * same launch, identical to sr_mfcc_batch_dev's.  Asynchronous on `stream`. */
int sr_frame_features_batch_dev(sr_engine *h, int kind, const uint16_t *d_pcm, uint64_t pcm_stride, uint32_t B,
                                const sr_vad_rec *d_vad, uint32_t *d_feat, int16_t *d_mfcc, void *stream);
/* HOST buffers, same inputs and per-record failure semantics as sr_mfcc_batch_status (frm_num, status; a failed record
 * has all-zero feature rows); mfcc and status may be NULL. */
int sr_frame_features_batch(sr_engine *h, int kind, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                            const int32_t *start, const int32_t *end, const uint32_t *mid, uint32_t *feat, int16_t *mfcc,
                            uint32_t *frm_num, uint32_t *status);
/* all-pairs greedy DTW of B feature sequences (in_mfcc[b*max_frames*n_coef], in_frames[b]) against the store */
int sr_dtw_batch(sr_engine *h, const int16_t *in_mfcc, const uint32_t *in_frames, uint32_t B, uint32_t *scores,
                 sr_result *results);
/* get_mdl (DTW.C:217-296; present in the reference but not called by main.c): template averaging.  For each of
 * the P pairs the greedy dtw() path of (in1 as input, in2 as model) is walked and the start point plus every point
 * the walk moves to contributes one merged frame, the per-coefficient get_mean (DTW.C:195-205) (a + b) / 2 in int
 * arithmetic.  in1 [P][rows1][12], in2 [P][rows2][12] (host); rows past n are read as by dtw() (one slack row).
 * mdl [P][mdl_rows][12] receives the merged templates (rows past the merged length are zero);
 * mdl_frames[p] = number of merged frames = step (DTW.C:293) -- when it exceeds mdl_rows only the first mdl_rows
 * frames were stored (the reference would overrun its 119-frame record); dis[p] = dis/step.  Pairs whose length ratio
 * is outside 1/2..2 give dis = 0xFFFFFFFF, mdl_frames = 0 and an all-zero mdl (DTW.C:236-239). */
int sr_get_mdl_batch(sr_engine *h, const int16_t *in1, const uint32_t *n1, uint32_t rows1, const int16_t *in2,
                     const uint32_t *n2, uint32_t rows2, uint32_t P, int16_t *mdl, uint32_t mdl_rows,
                     uint32_t *mdl_frames, uint32_t *dis);

/* OPT-IN, NON-REFERENCE scorer: full dynamic-programming DTW (anti-diagonal wavefront across the 64-lane wave,
 * template staged in LDS) with the reference's parallelogram (dtw_limit) and local distance (get_dis):
 *   D(1,1)=d(1,1); D(x,y)=d(x,y)+min(D(x-1,y-1),D(x-1,y),D(x,y-1)); score = D(in,mdl)/(in+mdl), dis_err if gated/unreachable.
 * The reference's dtw() is a greedy walk (DTW.C:150-188), so these scores differ from dtw()'s by design and are
 * never used by sr_recognize_* or the dtw symbol. */
/* Kernel: a band-limited anti-diagonal wavefront, `lanes` lanes of a wave per (utterance, template) pair (strips of that
 * many utterance frames; the value from the left moves by DPP, strip boundaries through LDS, the template staged in
 * LDS); sr_set_dp_lanes chooses 4, 8 or 16 (0 = automatic: 8 while three of its workgroups fit a CU's LDS, else 16),
 * or 1 = the first version (one wave per pair, 64-column sweeps of the whole rectangle), which also serves stores the
 * band kernel cannot stage.  All variants give identical scores. */
int sr_set_dp_lanes(sr_engine *h, uint32_t lanes);
int sr_dtw_dp_batch(sr_engine *h, const int16_t *in_mfcc, const uint32_t *in_frames, uint32_t B, uint32_t *scores);
int sr_dtw_dp_batch_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, const sr_vad_rec *d_vad,
                        uint32_t B, uint32_t *d_scores, void *stream);

/* ------------------------------------------------------------------ word spotting: subsequence DTW inside long features
 * OPT-IN EXTENSION, NO REFERENCE COUNTERPART.  Every other scorer takes an utterance the VAD has cut out, first frame to last
 * frame.  This one has a free start and a free end: for a feature row in[0..N) and a valid template mdl[0..M) it says where
 * inside the row the template matches best, and how well.  No existing call, record or score changes.
 *   d(x,y)   get_dis (DTW.C:45-62) of in[x] and mdl[y], as everywhere.
 *   paths    start at some (s, 0), end at some (e, M-1); steps (+1,+1), (+1,0), (0,+1), every horizontal or vertical step
 *            directly after a diagonal one (symmetric P = 1: slope 1/2..2, so no band and no length gate); cost = sum of d.
 *            D(x,0) = d(x,0), S(x,0) = x;
 *            D(x,y) = d(x,y) + min(D(x-1,y-1), D(x-2,y-1) + d(x-1,y), D(x-1,y-2) + d(x,y-1)),  D = INF outside the grid.
 *   ties     candidates are compared as (cost, start) pairs: S(x,y) is the smallest start among the paths of minimal cost.
 *   score    q(e) = D(e,M-1) / (L + M), L = e - S(e,M-1) + 1, u32 division.  The first reachable end frame is M / 2.
 *   windows  win_frames = 0: one window per row; else window w holds the end frames [w*win_frames, min((w+1)*win_frames, N))
 *            and n_win = ceil(max_frames / win_frames) for every row.  A window's hit is the FIRST minimum of q(e) over its
 *            reachable end frames (ascending e, strict <).  A window without a reachable end (past N, N <= M/2, N = 0, an
 *            invalid slot) gets {SR_DIS_ERR, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF}. */
typedef struct sr_spot_hit { /* 16 bytes */
    uint32_t dis;   /* q(e); SR_DIS_ERR: no hit */
    uint32_t start; /* S, 0-based frame of the row */
    uint32_t end;   /* e, 0-based, inclusive */
    uint32_t acc;   /* D(e, M-1) */
} sr_spot_hit;
/* Stage level, DEVICE buffers: d_mfcc[n_rows][max_frames][12]; d_in_frames / frames_stride as for sr_rescore_nbest_dp_dev (so
 * &d_vad[0].frm_num with stride 12 serves sr_mfcc_batch_dev's records; a failed record has frm_num 0).  A count above
 * max_frames is clamped; nothing outside rows [0, frames) of a feature record is read.  d_hits[(row*n_win + w)*K + slot]
 * (required): every record is written whole on every call.  d_scores (optional): the dis fields alone, u32 [n_rows*n_win][K]
 * -- the layout sr_nbest_batch_dev takes with n_rows*n_win rows, so word map, N-best and rejection margin apply per window.
 * Asynchronous on `stream`, no host synchronisation, no read-back.
 * Errors, before anything is launched or written: SR_ERR_BAD_CONFIG unless n_coef == 12; SR_ERR_NO_TEMPLATES; SR_ERR_BAD_ARG
 * for a null required pointer, frames_stride 0, n_rows*n_win above 16 776 960, a store whose longest template exceeds
 * sr_spot_geometry's out[2]. */
int sr_spot_dp_batch_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                         uint32_t win_frames, sr_spot_hit *d_hits, uint32_t *d_scores, void *stream);
/* the same on HOST buffers (copy in, launch, copy out) */
int sr_spot_dp_batch(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                     uint32_t win_frames, sr_spot_hit *hits, uint32_t *scores);
/* Whole path on HOST buffers: sr_mfcc_batch_status (its arguments, its per-record failure rules; mfcc, frm_num and status
 * may be NULL here) followed by the stage over those rows; a failed record has no hits.  The device whole path is
 * sr_mfcc_batch_dev followed by sr_spot_dp_batch_dev. */
int sr_spot_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B, const int32_t *start,
                  const int32_t *end, const uint32_t *mid, uint32_t win_frames, sr_spot_hit *hits, uint32_t *scores,
                  int16_t *mfcc, uint32_t *frm_num, uint32_t *status);
/* Host-only, MI355X's LDS figures: out[0] = n_win, out[1] = LDS bytes of one workgroup for a store whose longest template has
 * tpl_rows rows, out[2] = the longest template that fits, out[3] = columns (end frames) per kernel chunk. */
int sr_spot_geometry(uint32_t tpl_rows, uint32_t max_frames, uint32_t win_frames, uint32_t out[4]);

/* ------------------------------------------------------------------ live word spotting: spotter state carried between pushes
 * OPT-IN EXTENSION, NO REFERENCE COUNTERPART.  The spotter above takes a complete feature row of at most max_frames frames.
 * A session takes the frames of n_channels channels as they arrive, in pushes of any size up to chunk_max, keeps per
 * (channel, slot) ONE column of the recurrence and the open window's first minimum on the device between calls, and emits
 * every window's record when its last end frame has arrived: n * M cells per push of n frames, and no cap on a channel's
 * length below 0xFFFF0000 frames.  No existing call, record or score changes.
 * THE RULE: let Y_c be every feature frame pushed to channel c since it was opened or last ended, N = |Y_c|, W = win_frames
 * (>= 1, fixed at open).  Window w of channel c holds the end frames [w*W, (w+1)*W).  A push emits the windows whose last end
 * frame it consumed, by ascending channel, then ascending window; sr_spot_live_end emits the open window if it holds at
 * least one frame (N mod W != 0).  For every slot the record of window w is the record the word spotting section defines for
 * Y_c as ONE row of N frames with that win_frames -- byte for byte, whatever the chunking; start and end are 0-based frame
 * indices of the channel's recording.  While N <= max_frames it is therefore what sr_spot_dp_batch[_dev] writes for that row.
 * An invalid slot, and a window without a reachable end frame, get the no-hit record.  Every emitted record is written whole,
 * exactly once.  A push that would take a channel past 0xFFFF0000 frames returns SR_ERR_BAD_ARG (absolute starts live in 32
 * bits of the packed state).
 * PCM sessions (mid given at open): the channel's samples X_c, R = |X_c|, are framed as sr_spot_batch frames a segment with
 * start = 1, end = R and mid[c]: sample 0 serves only as pre-emphasis predecessor, frame j exists once
 * R >= 1 + j*hop + frame_len; the records are those of the rule above on these frames, so while there are at most max_frames
 * of them they equal sr_spot_batch(X_c, 1, R, mid[c], W).  The device keeps the samples from the next frame's predecessor on.
 * Every call refused for its arguments, its counts or the store (SR_ERR_BAD_ARG, SR_ERR_BAD_CONFIG, SR_ERR_NO_TEMPLATES) is
 * refused before anything is enqueued: it writes nothing and changes no state.  A HIP failure (SR_ERR_HIP: allocation, copy,
 * launch) may come after part of a push has been enqueued; the session is then undefined and must be closed.  Pushes of one
 * session may go to different streams: a push on another stream than the last push's is ordered behind it by an event, and
 * the host forms and sr_spot_live_end run behind the last push likewise.  A session's state is shaped by the template store: a channel is
 * bound to the store that was set when the session was opened or the channel last ended, and a push of frames to a channel
 * whose store has since been replaced returns SR_ERR_BAD_ARG until that channel is ended (its open window is then dropped:
 * the templates it was scored against are gone).  The session uses its engine's scratch buffers: the engine's
 * one-caller-at-a-time rule covers its sessions. */
typedef struct sr_spot_live sr_spot_live;
typedef struct sr_spot_win { /* 8 bytes: which window an emitted row holds */
    uint32_t channel;
    uint32_t window;
} sr_spot_win;
/* host-only, no device: out[0] = most windows one channel can complete in one push of chunk_max frames, out[1] = device state
 * bytes per channel for K slots whose longest template has tpl_rows rows (saturating), out[2] = the longest template that
 * fits (sr_spot_geometry's out[2]) */
int sr_spot_live_geometry(uint32_t tpl_rows, uint32_t K, uint32_t chunk_max, uint32_t win_frames, uint32_t out[3]);
/* mid NULL: a feature session, chunk_max in frames, 1..max_frames.  mid a HOST array [n_channels]: a PCM session, chunk_max in
 * samples; SR_ERR_BAD_ARG if a push of chunk_max samples could complete more than max_frames frames.  n_channels 1..65535,
 * win_frames >= 1.  Configuration errors as sr_spot_dp_batch_dev (n_coef != 12, no templates, templates too long). */
int sr_spot_live_open(sr_engine *h, uint32_t n_channels, uint32_t chunk_max, uint32_t win_frames, const uint32_t *mid,
                      sr_spot_live **out);
void sr_spot_live_close(sr_spot_live *l); /* before sr_destroy of its engine; waits for the session's last push */
/* host-only: the EXACT number of window rows a push with these counts emits (n NULL: n_all each); 0 for counts a push refuses */
uint32_t sr_spot_live_rows(const sr_spot_live *l, const uint32_t *n, uint32_t n_all);
/* host-only, no session: the count sr_spot_live_rows is made of -- channel c stands at frames_before[c] frames and gets
 * n_new[c] more: sum over c of (frames_before[c] + n_new[c]) / win_frames - frames_before[c] / win_frames; 0 for win_frames 0,
 * a null array or a channel that would pass 0xFFFF0000 frames */
uint32_t sr_spot_live_windows(uint32_t win_frames, const uint32_t *frames_before, const uint32_t *n_new, uint32_t n_channels);
/* One push.  n: HOST array [n_channels] in both forms, 0 <= n[c] <= chunk_max, 0 leaves the channel untouched; NULL: n_all
 * each.  Channel c's new frames are d_mfcc + c*row_stride (s16, 12 per frame; row_stride in s16 elements, at least 12 times
 * the largest count); nothing past n[c] frames of a row is read.  DEVICE form: d_mfcc 8-byte aligned, row_stride a multiple
 * of 4; ONE asynchronous operation on `stream`, no host synchronisation, no read-back.  d_hits[r*K + slot] and the optional
 * d_scores[r*K + slot] (the dis fields: sr_nbest_batch_dev's input with *n_rows rows) are COMPACT over the emitted rows r;
 * rows at and past *n_rows are not written.  wins[max_rows] and *n_rows are HOST outputs, filled from the counts alone before
 * the call returns.  max_rows below sr_spot_live_rows() returns SR_ERR_BAD_ARG. */
int sr_spot_live_push_dev(sr_spot_live *l, const int16_t *d_mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all,
                          uint32_t max_rows, sr_spot_hit *d_hits, uint32_t *d_scores, sr_spot_win *wins, uint32_t *n_rows,
                          void *stream);
/* the same on HOST buffers (2-byte aligned rows, any row_stride that holds the largest count) */
int sr_spot_live_push(sr_spot_live *l, const int16_t *mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all,
                      uint32_t max_rows, sr_spot_hit *hits, uint32_t *scores, sr_spot_win *wins, uint32_t *n_rows);
/* PCM sessions: channel c's new samples are d_pcm + c*pcm_stride, n in samples; alignment rules as sr_live_push_dev (device
 * form: 16-byte aligned, pcm_stride a multiple of 8).  A copy kernel builds [kept | chunk] rows, the frame kernel launch of
 * sr_mfcc_batch_dev turns them into the push's new frames, the spotter runs over those. */
int sr_spot_live_push_pcm_dev(sr_spot_live *l, const uint16_t *d_pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                              uint32_t max_rows, sr_spot_hit *d_hits, uint32_t *d_scores, sr_spot_win *wins, uint32_t *n_rows,
                              void *stream);
int sr_spot_live_push_pcm(sr_spot_live *l, const uint16_t *pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                          uint32_t max_rows, sr_spot_hit *hits, uint32_t *scores, sr_spot_win *wins, uint32_t *n_rows);
/* The listed channels' recordings end here: HOST outputs hits[n_ch][K] and wins[n_ch], of which *n_rows rows are written --
 * the open window of each listed channel that has one, in the order listed.  A channel listed more than once counts once, at
 * its first mention (it is fresh, with nothing open, by the second).  Waits for the device.  Each listed channel is then as
 * freshly opened, and bound to the current store. */
int sr_spot_live_end(sr_spot_live *l, const uint32_t *channels, uint32_t n_ch, sr_spot_hit *hits, sr_spot_win *wins,
                     uint32_t *n_rows);

/* ------------------------------------------------------------------ connected-word decoding: level-building DTW
 * OPT-IN EXTENSION, NO REFERENCE COUNTERPART.  The spotter says where each template matches best, slot by slot; this section
 * says which SEQUENCE of words a feature row in[0..N) contains (N clamped to max_frames): digits or a command and its
 * argument spoken without pauses.  Level l holds the best parse of every prefix of the row into exactly l words; one level is
 * one spotter-shaped pass whose start row carries the previous level's costs.  No existing call, record or score changes.
 *   d(x,y)   get_dis (DTW.C:45-62), as everywhere.
 *   words    a word is a path of the spotter's kind through one valid slot k of M_k frames: from (s, 0) to (e, M_k-1), steps
 *            (+1,+1), (+1,0), (0,+1), every horizontal or vertical step directly after a diagonal one, cost = sum of d.
 *   E_0(p)   cost of the prefix of length p (p = 0..N) without a word: p * skip_cost when skipping is on (skip_cost !=
 *            SR_DIS_ERR), else E_0(0) = 0 and E_0(p > 0) = INF.
 *   level l  >= 1, per slot: the spotter's recurrence with a CHARGED start, D(x,0) = E_{l-1}(x) + d(x,0), S(x,0) = x, the
 *            start unreachable where E_{l-1}(x) is INF; everything else as in the word spotting section.
 *   A_l(p)   p >= 1: the minimum over the valid slots k of (D_k(p-1, M_k-1) + word_cost, S, k), candidates compared as
 *            (cost, start, slot): a tie goes to the smallest start, then to the smallest slot.
 *   E_l(p)   min(A_l(p).cost, E_l(p-1) + skip_cost), the second term only when skipping is on; E_l(0) = INF.
 *   count    n = n_words_exact when that is nonzero, else the n of 1..max_words with the smallest E_n(N), the fewest words
 *            among equal costs.  No finite E_n(N) (an empty row, no valid slot, no parse): status SR_CH_NONE.
 *   trace    p = N; for l = n down to 1: while A_l(p) is unreachable or A_l(p).cost != E_l(p), frame p-1 is skipped and
 *            p -= 1; word l is A_l(p): its slot, start = S, end = p-1; then p = S.  The p frames left after level 1 are
 *            leading skipped frames (none when skipping is off).  Filler between and after words is as short as the cost allows.
 *   limits   max_words 1..16; skip_cost <= 65 535 or SR_DIS_ERR; word_cost <= 2^24; a store of at most 65 536 slots.  With
 *            d <= 65 536, at most 3L cells in a word over L frames and N <= 16 383 every cost stays below
 *            3 * 16 383 * 65 536 + 16 * 2^24 < 2^32: u32 costs are exact.  Arguments outside these limits are refused. */
#define SR_CH_OK 0u
#define SR_CH_NONE 1u
typedef struct sr_chain_rec { /* 16 bytes */
    uint32_t cost;    /* E_n(N); SR_DIS_ERR unless status is SR_CH_OK */
    uint32_t n_words; /* n; 0 unless OK */
    uint32_t skipped; /* frames of the row that belong to no word; 0 unless OK */
    uint32_t status;  /* SR_CH_OK / SR_CH_NONE */
} sr_chain_rec;
typedef struct sr_chain_word { /* 32 bytes */
    uint32_t word;     /* the engine's word map (sr_set_word_map) applied to slot */
    uint32_t slot;
    uint32_t start;    /* 0-based frame of the row */
    uint32_t end;      /* 0-based, inclusive */
    uint32_t acc;      /* the word's own path cost, without word_cost */
    uint32_t dis;      /* acc / (L + M), L = end - start + 1, as the spotter's q */
    uint32_t cum;      /* E_l at the word's end */
    uint32_t reserved; /* 0 */
} sr_chain_word;
/* Stage level, DEVICE buffers: d_mfcc / d_in_frames / frames_stride as for sr_spot_dp_batch_dev; nothing outside rows
 * [0, frames) of a feature record is read.  d_rec[n_rows] and d_words[n_rows][max_words] (required; word l of a row at index
 * l-1, entries at or beyond n_words all ones), d_level_cost (optional) u32 [n_rows][max_words] = E_l(N) or SR_DIS_ERR: every
 * record and every word row is written whole on every call.  One asynchronous operation on `stream` (a row's keys and prefix
 * costs live in the engine's scratch, sr_decode_geometry), no host synchronisation, no read-back; two runs give the same bytes.
 * Errors, before anything is launched or written: SR_ERR_BAD_CONFIG unless n_coef == 12; SR_ERR_NO_TEMPLATES; SR_ERR_BAD_ARG
 * for a null required pointer, frames_stride 0, an argument outside the limits above, n_words_exact > max_words, a word map
 * that does not fit the store, a store whose longest template exceeds sr_decode_geometry's out[2], outputs that overlap. */
int sr_decode_words_dp_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                           uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *d_rec,
                           sr_chain_word *d_words, uint32_t *d_level_cost, void *stream);
/* the same on HOST buffers (copy in, launch, copy out) */
int sr_decode_words_dp(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                       uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *rec,
                       sr_chain_word *words, uint32_t *level_cost);
/* Whole path on HOST buffers: sr_mfcc_batch_status (its arguments, its per-record failure rules; mfcc, frm_num and status
 * may be NULL here) followed by the stage over those rows; a failed record has no parse.  The device whole path is
 * sr_mfcc_batch_dev followed by sr_decode_words_dp_dev. */
int sr_decode_words_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B, const int32_t *start,
                          const int32_t *end, const uint32_t *mid, uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost,
                          uint32_t word_cost, sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost, int16_t *mfcc,
                          uint32_t *frm_num, uint32_t *status);
/* Host-only, MI355X's LDS figures: out[0] = scratch bytes per row, out[1] = rows per launch group (what 256 MiB of scratch
 * hold, 65 535 at most), out[2] = the longest template that fits, out[3] = columns (end frames) per kernel chunk. */
int sr_decode_geometry(uint32_t tpl_rows, uint32_t max_frames, uint32_t max_words, uint32_t out[4]);

/* ------------------------------------------------------------------ live connected-word decoding: decoder state carried between pushes
 * OPT-IN EXTENSION, NO REFERENCE COUNTERPART.  The decoder above takes a complete feature row and pays N x max_words x K x M
 * cells for it.  A session takes the frames of n_channels channels as they arrive, in pushes of any size up to chunk_max,
 * keeps per (channel, level, slot) ONE column of the recurrence and per channel the A / E history on the device between
 * calls, and after every push says how everything heard so far parses: n x max_words x K x M cells per push of n frames,
 * plus a trace.  No existing call, record or score changes.
 * THE RULE: let Y_c be every feature frame pushed to channel c since it was opened or last ended, N = |Y_c|; N is at most
 * utt_frames, fixed at open in 1..16 383 (the u32 cost bound and the start field of a key end there).  Every push emits one
 * row for every channel with n[c] > 0, by ascending channel: an sr_chain_rec, max_words x sr_chain_word and optionally
 * level_cost[max_words].  The row is, byte for byte, what the connected-word decoding section defines for Y_c as ONE row of N
 * frames with the session's max_words, n_words_exact, skip_cost, word_cost and the engine's current word map -- whatever the
 * chunking.  Whenever an engine's max_frames >= N it therefore equals what sr_decode_words_dp[_dev] writes for that row.
 * start and end are 0-based frame indices of the channel's recording.  Ties: smallest start, then slot, then fewest words,
 * unchanged.  Why it is exact: column x of a level depends on column x-1 and E_{l-1}(x) only; A_l(p) and E_l(p) depend on
 * frames < p only, so the history of a recording is a prefix of that of any longer one; count and trace read A, E and N.
 * PCM sessions (mid given at open): the channel's samples X_c, R = |X_c|, are framed exactly as the live word spotting section
 * frames them (a segment with start = 1, end = R and mid[c]); n[c] counts samples, a row is emitted for n[c] > 0 whether or
 * not a frame was completed, and while there are at most max_frames frames the row equals sr_decode_words_batch(X_c, 1, R,
 * mid[c]).
 * Every call refused for its arguments, its counts or the store (SR_ERR_BAD_ARG, SR_ERR_BAD_CONFIG, SR_ERR_NO_TEMPLATES) is
 * refused before anything is enqueued: it writes nothing and changes no state.  A HIP failure (SR_ERR_HIP) may come after
 * part of a push has been enqueued; the session is then undefined and must be closed.  Stream ordering as in the spot
 * session: a push on another stream than the last push's is ordered behind it by an event, the host forms and
 * sr_decode_live_end run behind the last push likewise.  A channel is bound to the template store that was set when the
 * session was opened or the channel last ended; a push to a channel whose store has since been replaced returns
 * SR_ERR_BAD_ARG until that channel is ended (its recording is then dropped: it ends with the SR_CH_NONE record).  The
 * session uses its engine's scratch buffers: the engine's one-caller-at-a-time rule covers its sessions. */
typedef struct sr_decode_live sr_decode_live;
typedef struct sr_chain_live_row { /* 8 bytes: which channel an emitted row holds */
    uint32_t channel;
    uint32_t frames; /* N after the push */
} sr_chain_live_row;
/* host-only, no device: out[0] = device state bytes per channel -- the columns, max_words * K * tpl_rows * 16, plus the A / E
 * history, (utt_frames + 1) * (max_words * 8 + (max_words + 1) * 4) -- saturating; out[1] = the longest template that fits
 * (sr_spot_geometry's out[2]); out[2] = the kernel launches one feature push enqueues, 2 * max_words + 2.  tpl_rows and
 * utt_frames 1..16 383, K 1..65 536, max_words 1..16, chunk_max 1..utt_frames. */
int sr_decode_live_geometry(uint32_t tpl_rows, uint32_t K, uint32_t max_words, uint32_t utt_frames, uint32_t chunk_max, uint32_t out[3]);
/* mid NULL: a feature session, chunk_max in frames, 1..utt_frames.  mid a HOST array [n_channels]: a PCM session, chunk_max in
 * samples; SR_ERR_BAD_ARG if a push of chunk_max samples could complete more than min(max_frames, utt_frames) frames.
 * n_channels 1..65535.  Argument limits and configuration errors exactly as sr_decode_words_dp_dev. */
int sr_decode_live_open(sr_engine *h, uint32_t n_channels, uint32_t chunk_max, uint32_t utt_frames, uint32_t max_words,
                        uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost, const uint32_t *mid, sr_decode_live **out);
void sr_decode_live_close(sr_decode_live *l); /* before sr_destroy of its engine; waits for the session's last push */
/* One push.  n: HOST array [n_channels] in both forms, 0 <= n[c] <= chunk_max, 0 leaves the channel untouched; NULL: n_all
 * each.  Channel c's new frames are d_mfcc + c*row_stride (s16, 12 per frame; row_stride in s16 elements, at least 12 times
 * the largest count); nothing past n[c] frames of a row is read.  DEVICE form: d_mfcc 8-byte aligned, row_stride a multiple
 * of 4; ONE asynchronous operation on `stream`, no host synchronisation, no read-back.  d_rec[r], d_words[r*max_words + i]
 * and the optional d_level_cost[r*max_words + i] are COMPACT over the emitted rows r; rows at and past *n_rows are not
 * written.  rows[max_rows] and *n_rows are HOST outputs, filled from the counts alone before the call returns.  Refused
 * (SR_ERR_BAD_ARG): a count above chunk_max, a push that would take a channel past utt_frames, max_rows below the number of
 * channels with n[c] > 0, a channel bound to a replaced store, a word map that does not fit, a null required pointer,
 * outputs that overlap. */
int sr_decode_live_push_dev(sr_decode_live *l, const int16_t *d_mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all,
                            uint32_t max_rows, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_level_cost,
                            sr_chain_live_row *rows, uint32_t *n_rows, void *stream);
/* the same on HOST buffers (2-byte aligned rows, any row_stride that holds the largest count) */
int sr_decode_live_push(sr_decode_live *l, const int16_t *mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all,
                        uint32_t max_rows, sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost, sr_chain_live_row *rows,
                        uint32_t *n_rows);
/* PCM sessions: channel c's new samples are d_pcm + c*pcm_stride, n in samples; alignment rules as sr_spot_live_push_pcm_dev
 * (device form: 16-byte aligned, pcm_stride a multiple of 8).  The spot session's copy kernels and the frame kernel launch of
 * sr_mfcc_batch_dev turn them into the push's new frames, the decoder runs over those. */
int sr_decode_live_push_pcm_dev(sr_decode_live *l, const uint16_t *d_pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                                uint32_t max_rows, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_level_cost,
                                sr_chain_live_row *rows, uint32_t *n_rows, void *stream);
int sr_decode_live_push_pcm(sr_decode_live *l, const uint16_t *pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                            uint32_t max_rows, sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost,
                            sr_chain_live_row *rows, uint32_t *n_rows);
/* The listed channels' recordings end here: HOST outputs rec[n_ch], words[n_ch][max_words], the optional level_cost[n_ch]
 * [max_words] and rows[n_ch], of which *n_rows rows are written -- one per DISTINCT listed channel, at its first mention: the
 * decode of everything pushed to it (an empty channel gives the SR_CH_NONE record, as an empty row does in the batch call).
 * Waits for the device.  Each listed channel is then as freshly opened, and bound to the current store.  rows overlapping
 * rec, words or level_cost is refused like outputs that overlap in a push.  A HIP failure (SR_ERR_HIP) before the trace --
 * an allocation -- writes nothing and leaves the session as it was; one after it leaves the session undefined, as in a push. */
int sr_decode_live_end(sr_decode_live *l, const uint32_t *channels, uint32_t n_ch, sr_chain_rec *rec, sr_chain_word *words,
                       uint32_t *level_cost, sr_chain_live_row *rows, uint32_t *n_rows);

/* ------------------------------------------------------------------ grammar-constrained decoding: level building over a word network
 * OPT-IN EXTENSION, NO REFERENCE COUNTERPART.  The connected-word decoder accepts ANY sequence of words; an application has a
 * syntax (digit strings of a known shape, a command and its argument).  A grammar is a finite-state network whose arcs carry
 * words; the decoder below returns the cheapest parse among the word sequences the network accepts, and spends no cell on the
 * others.  No existing call, record, score or byte changes.
 *   grammar  states 0..S-1, state 0 the start; final_state[s] != 0 flags the final states; n_arcs distinct arcs (from, to,
 *            word), word a label of the engine's word map (sr_set_word_map; default word = slot).  slots(w) = the valid slots
 *            with label w.  For a pair (t, w) with at least one arc, From(t, w) = { s : (s, t, w) is an arc }.
 *   limits   S 1..64 (a from-set is one 64-bit mask), n_arcs 1..4096, every word a label of the current map.  No duplicate
 *            arcs, no empty (epsilon) arcs.  Dead and unreachable states are allowed; a word whose slots are all invalid is
 *            allowed and contributes nothing.  Costs on arcs and final states: sr_grammar_create_weighted below.
 * Everything not restated here is the connected-word decoding section: d, the word path, skip_cost, word_cost, the argument
 * limits, the u32 cost bound, the record formats.
 *   E_0(p,s) that section's E_0(p) for s = 0; INF for every other state.
 *   charge   C_l(x; t, w) = min over s in From(t, w) of E_{l-1}(x, s).
 *   level l  >= 1, per pair (t, w) and slot k of slots(w): the spotter's recurrence with D(x,0) = C_l(x; t, w) + d(x,0),
 *            S(x,0) = x, the start unreachable where the charge is.
 *   A_l(p,t) p >= 1: the minimum over all pairs (t, w) and all k of slots(w) of (D_k(p-1, M_k-1) + word_cost, S, k), candidates
 *            compared as (cost, start, slot).  A slot has one label, so for a fixed t it occurs at most once.
 *   E_l(p,t) min(A_l(p,t).cost, E_l(p-1,t) + skip_cost), the second term only when skipping is on; E_l(0,t) = INF.  Filler
 *            after a word stays in that word's target state.
 *   L_l      min over the final states f of E_l(N, f): the level cost.
 *   count    n = n_words_exact when that is nonzero, else the n of 1..max_words with the smallest L_n, the fewest words among
 *            equal costs.  No finite L_n: status SR_CH_NONE, with the decoder's record.
 *   end      the smallest final state f with E_n(N, f) = L_n.
 *   trace    p = N, t = f; for l = n down to 1: while A_l(p,t) is unreachable or its cost differs from E_l(p,t), p -= 1; word
 *            l is A_l(p,t): its slot k, start = S, end = p-1, cum = E_l(p,t); acc = cost - word_cost - C_l(S; t, w(k)); the
 *            source state is the smallest s of From(t, w(k)) with E_{l-1}(S, s) = C_l(S; t, w(k)); then p = S, t = s.
 *   records  sr_chain_rec and sr_chain_word as they are; in rows written by the calls below sr_chain_word.reserved holds the
 *            grammar state AFTER the word (t).  d_level_cost[l-1] = L_l.
 * Why one pass per (slot, target state) serves every arc of that word into that state: min_s (E(x,s) + path) = (min_s E(x,s))
 * + path, and the source state is recoverable from E_{l-1} at the start column.  A word-pair grammar (one state per word)
 * therefore costs the K passes per level of the unconstrained decoder.
 * Anchor: S = 1, final_state[0] = 1 and one arc (0, 0, w) per label give, byte for byte, what sr_decode_words_dp writes
 * (reserved = 0 included).
 * Out of scope: epsilon arcs; more than 64 states.  (The push-by-push session is the next section.) */
typedef struct sr_gram_arc { /* 16 bytes */
    uint32_t from;
    uint32_t to;
    uint32_t word;
    uint32_t reserved; /* 0 */
} sr_gram_arc;
typedef struct sr_grammar sr_grammar;
/* Compiles the grammar against the engine's CURRENT store and word map: the distinct from-sets as 64-bit masks, the items
 * (slot, target state, from-set) and, per level 1..16, the items that can matter.  The only call of this section that may wait
 * for the device and upload.  arcs and final_state[n_states] are HOST arrays.  Many grammars may exist per engine (one per
 * dialogue state).  A grammar is bound to the store and the word map it was compiled against: after either is set again a
 * decode call with it returns SR_ERR_BAD_ARG and writes nothing.  Errors, nothing created: SR_ERR_BAD_CONFIG unless n_coef ==
 * 12; SR_ERR_NO_TEMPLATES; SR_ERR_BAD_ARG for a null pointer, n_states 0 or above 64, n_arcs 0 or above 4096, a state index at
 * or above n_states, a duplicate arc, nonzero reserved, a word the map does not have, no final state, a word map that does not
 * fit the store, a store of more than 65 536 slots. */
int sr_grammar_create(sr_engine *h, uint32_t n_states, const sr_gram_arc *arcs, uint32_t n_arcs, const uint8_t *final_state,
                      sr_grammar **out);
/* Weighted grammars: arc weights and final costs.  A grammar above can only allow or forbid a word in a context; the grammars
 * applications use are bigram tables, priors over commands and a price for stopping early: "this word is likely here, that
 * one unlikely", as a cost added to the acoustic cost.  arc_cost[i] (u32) belongs to arc i, final_cost[s] (u32) to the final
 * state s; write c(s,t,w) for the cost of arc (s,t,w).  Everything not restated is the section above.
 *   limits   every arc cost <= 2^24 and every final cost <= 2^24; a state that is not final has final cost 0.  The cost bound of
 *            the connected-word section still holds: 3 * 16 383 * 65 536 + 16 * 2^24 (paths and word costs) + 16 * 2^24 (arcs)
 *            + 2^24 (final) = 3 774 676 992 < 2^32, so u32 costs stay exact.
 *   charge   C_l(x; t, w) = min over the s in From(t, w) with E_{l-1}(x, s) finite of E_{l-1}(x, s) + c(s,t,w); INF when there
 *            is no such s.  An unreachable E (SR_DIS_ERR) never has a cost added to it.
 *   level, A_l, E_l  unchanged: the arc cost is part of a word's key cost and of cum.  Filler after a word stays in the word's
 *            target state at skip_cost per frame.
 *   L_l      min over the final f with E_l(N, f) finite of E_l(N, f) + final_cost[f].  d_level_cost[l-1] = L_l and
 *            sr_chain_rec.cost = L_n.
 *   count    as above, over these L_l.
 *   end      the smallest final f with E_n(N, f) + final_cost[f] = L_n.
 *   trace    as above, with acc = key cost - word_cost - C_l(S; t, w(k)): still the word's own path cost, without its arc
 *            cost; cum = E_l(p,t), so the LAST word's cum excludes the final cost while sr_chain_rec.cost includes it; the
 *            source state is the smallest s of From(t, w(k)) with E_{l-1}(S, s) finite and E_{l-1}(S, s) + c(s,t,w(k)) =
 *            C_l(S; t, w(k)).
 *   ties     smallest start, then slot, then fewest words, then smallest final state, then smallest source state, all judged
 *            on the costs including arc and final costs.
 *   pruning  unchanged: it is structural and costs are finite, so it still never changes an output byte.
 * Why one pass per (slot, target state) still serves every arc of the word into that state: min_s (E(x,s) + c_s + path) =
 * (min_s (E(x,s) + c_s)) + path.  A bigram grammar over W words costs K word passes per level, not W x K.
 * The compile step keeps, per pair (t, w), its CHARGE LIST: the ascending-by-state list of (s, c(s,t,w)); distinct lists are
 * shared as from-sets are, and sr_grammar_plan's out[3] and the "from-sets * 4" term of out[0] count distinct charge lists.
 * Anchor: all costs zero (or both arrays NULL) gives the grammar sr_grammar_create makes -- the same plan figures, the same
 * kernels and launches, byte for byte the same outputs in every batch and live call.
 * arc_cost is a HOST array [n_arcs] or NULL (all 0), final_cost a HOST array [n_states] or NULL (all 0).  The grammar carries
 * its costs: every call that takes an sr_grammar takes it unchanged (sr_decode_grammar_dp[_dev], sr_decode_grammar_batch,
 * sr_grammar_plan, and the live session's open, set_grammar, pushes, end and geometry).  Errors as sr_grammar_create
 * (sr_gram_arc.reserved must still be 0); SR_ERR_BAD_ARG as well, nothing created, for a cost above 2^24 or a nonzero
 * final_cost on a state that is not final. */
int sr_grammar_create_weighted(sr_engine *h, uint32_t n_states, const sr_gram_arc *arcs, const uint32_t *arc_cost, uint32_t n_arcs,
                               const uint8_t *final_state, const uint32_t *final_cost, sr_grammar **out);
void sr_grammar_destroy(sr_grammar *g); /* before sr_destroy of its engine; waits for the device */
/* Host-only.  Per-level pruning, exact (it never changes an output byte): level l of a call with max_words keeps item (slot,
 * t, from-set) only if the from-set meets the states reachable from state 0 in exactly l-1 arcs and a final state is
 * reachable from t in at most max_words - l further arcs; a level without items launches no word pass.  items_per_level
 * (optional) [max_words]: the items kept at level l at index l-1.  out[0] = scratch bytes per row: (max_frames + 1) *
 * (max_words * S * 8 + (max_words + 1) * S * 4 + from-sets * 4); out[1] = rows per launch group (what 256 MiB of scratch hold,
 * 1..65 535); out[2] = kernel launches of one launch group: 2 (init, trace) + per level with items 3 (charge, words, close);
 * out[3] = the number of distinct from-sets. */
int sr_grammar_plan(const sr_grammar *g, uint32_t max_words, uint32_t *items_per_level, uint32_t out[4]);
/* sr_decode_words_dp_dev under the grammar: its arguments, buffers, limits, errors and guarantees (one asynchronous operation
 * on `stream`, no host synchronisation, no read-back, every record and word row written whole, two runs give the same bytes).
 * Refused as well, before anything is launched or written (SR_ERR_BAD_ARG): a null grammar, a grammar of another engine, a
 * grammar older than the engine's store or word map. */
int sr_decode_grammar_dp_dev(sr_engine *h, const sr_grammar *g, const int16_t *d_mfcc, const uint32_t *d_in_frames,
                             uint32_t frames_stride, uint32_t n_rows, uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost,
                             uint32_t word_cost, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_level_cost, void *stream);
/* the same on HOST buffers (copy in, launch, copy out) */
int sr_decode_grammar_dp(sr_engine *h, const sr_grammar *g, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride,
                         uint32_t n_rows, uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost,
                         sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost);
/* whole path on HOST buffers: sr_decode_words_batch under the grammar */
int sr_decode_grammar_batch(sr_engine *h, const sr_grammar *g, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                            const int32_t *start, const int32_t *end, const uint32_t *mid, uint32_t max_words, uint32_t n_words_exact,
                            uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost,
                            int16_t *mfcc, uint32_t *frm_num, uint32_t *status);

/* ------------------------------------------------------------------ live grammar-constrained decoding: grammar state carried between pushes
 * OPT-IN EXTENSION, NO REFERENCE COUNTERPART.  The live connected-word session under a grammar: a session takes the frames of
 * n_channels channels as they arrive, keeps per (channel, level, kept item) ONE column of the recurrence and per channel the
 * A / E history of every grammar state on the device between calls, and after every push says how everything heard so far
 * parses UNDER THE GRAMMAR.  No existing call, record, score or byte changes.
 * THE RULE: let Y_c be every feature frame pushed to channel c since it was opened or last ended, N = |Y_c| <= utt_frames
 * (1..16 383).  Every push emits one row for every channel with n[c] > 0, by ascending channel: an sr_chain_rec, max_words x
 * sr_chain_word and optionally level_cost[max_words], labelled by an sr_chain_live_row.  The row is, byte for byte, what the
 * grammar-constrained decoding section defines for Y_c as ONE row of N frames under the session's grammar, max_words,
 * n_words_exact, skip_cost and word_cost -- whatever the chunking; sr_chain_word.reserved (the state after the word) and
 * level_cost[l-1] = L_l included.  Whenever an engine's max_frames >= N it therefore equals what sr_decode_grammar_dp[_dev]
 * writes for that row.  Ties keep their rule: smallest start, then slot, then fewest words, then smallest final state, then
 * smallest source state.  Why it is exact: A_l(p,t) and E_l(p,t) depend on frames < p only; column x of an item needs column
 * x-1 and the charge at x, a minimum over E_{l-1}(x, .); count, end state and trace read A, E and N.
 * PCM sessions (mid given at open) frame the samples exactly as the live connected-word decoding section does; a row is
 * emitted for n[c] > 0 whether or not a frame was completed, and while there are at most max_frames frames the row equals
 * sr_decode_grammar_batch(X_c, 1, R, mid[c]).
 * A session is bound to ONE grammar at a time (one per dialogue state: sr_gram_live_set_grammar switches it between
 * recordings).  A grammar is stale once the store or the word map has been set after sr_grammar_create: a push is then
 * refused (SR_ERR_BAD_ARG), sr_gram_live_end drops the listed recordings (each ends with the SR_CH_NONE record), and
 * sr_gram_live_set_grammar with a fresh grammar puts the session back to work.  Refusals, HIP failures, stream ordering and
 * the engine's one-caller-at-a-time rule as in the live connected-word decoding section.  Teardown: the session before its
 * grammar, the grammar before the engine.
 * A weighted grammar (sr_grammar_create_weighted) is taken as it is by every call below, sr_gram_live_set_grammar included: the
 * row is then what the weighted definitions give for Y_c as one row, and sr_gram_live_geometry's figures are those of the
 * same network without costs.
 * Out of scope: a grammar per channel; epsilon arcs; more than 64 states; a history compacted to each level's
 * target states (the dense [S] history is what sr_gram_live_geometry reports); splitting a push along time. */
typedef struct sr_gram_live sr_gram_live;
/* host-only, no device: out[0] = device state bytes per channel, saturating: columns * tpl_rows * 16 + (utt_frames + 1) * S *
 * (max_words * 8 + (max_words + 1) * 4), tpl_rows the longest template of the store the grammar was compiled against; out[1] =
 * the longest template that fits (sr_spot_geometry's out[2]); out[2] = the kernel launches of one feature push, 2 (init,
 * trace) + 2 (words, close) per level that keeps items; out[3] = columns, the sum over the levels 1..max_words of the items
 * sr_grammar_plan keeps there: a level stores boundary columns only for the items it sweeps.  max_words 1..16, utt_frames
 * 1..16 383, chunk_max 1..utt_frames. */
int sr_gram_live_geometry(const sr_grammar *g, uint32_t max_words, uint32_t utt_frames, uint32_t chunk_max, uint32_t out[4]);
/* sr_decode_live_open under g: its arguments, limits and errors; SR_ERR_BAD_ARG as well for a null grammar, a grammar of
 * another engine, a grammar older than the engine's store or word map. */
int sr_gram_live_open(sr_engine *h, const sr_grammar *g, uint32_t n_channels, uint32_t chunk_max, uint32_t utt_frames,
                      uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost, const uint32_t *mid,
                      sr_gram_live **out);
void sr_gram_live_close(sr_gram_live *l); /* before sr_grammar_destroy of its grammar; waits for the session's last push */
/* The grammar of the next dialogue state, or a fresh one in the place of a stale one: accepted only while every channel is
 * empty (freshly opened or ended), otherwise SR_ERR_BAD_ARG and the session stays as it was; refused like sr_gram_live_open
 * for the grammar itself.  Lays the columns and the history out for g: what has to grow is allocated aside and swapped in
 * after the last allocation, so an allocation failure (SR_ERR_HIP) leaves the session on its old grammar, buffers included. */
int sr_gram_live_set_grammar(sr_gram_live *l, const sr_grammar *g);
/* The four pushes: argument lists, alignment rules, compact outputs, host-filled rows / *n_rows, stream ordering by event and
 * the refusal list of sr_decode_live_push_dev, _push, _push_pcm_dev and _push_pcm.  The device forms are ONE asynchronous
 * operation on `stream`, no host synchronisation, no read-back.  A call refused for its arguments writes nothing and changes
 * no state.  Refused as well (SR_ERR_BAD_ARG): any push while the session's grammar is stale. */
int sr_gram_live_push_dev(sr_gram_live *l, const int16_t *d_mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all,
                          uint32_t max_rows, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_level_cost,
                          sr_chain_live_row *rows, uint32_t *n_rows, void *stream);
int sr_gram_live_push(sr_gram_live *l, const int16_t *mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all,
                      uint32_t max_rows, sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost, sr_chain_live_row *rows,
                      uint32_t *n_rows);
int sr_gram_live_push_pcm_dev(sr_gram_live *l, const uint16_t *d_pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                              uint32_t max_rows, sr_chain_rec *d_rec, sr_chain_word *d_words, uint32_t *d_level_cost,
                              sr_chain_live_row *rows, uint32_t *n_rows, void *stream);
int sr_gram_live_push_pcm(sr_gram_live *l, const uint16_t *pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                          uint32_t max_rows, sr_chain_rec *rec, sr_chain_word *words, uint32_t *level_cost,
                          sr_chain_live_row *rows, uint32_t *n_rows);
/* sr_decode_live_end under the grammar: HOST outputs, one row per DISTINCT listed channel at its first mention, the parse of
 * everything pushed to it; waits for the device; each listed channel is then as freshly opened.  With a stale grammar the
 * listed recordings are dropped: each gets the SR_CH_NONE record and frames = 0, and the channels are empty afterwards --
 * whatever the engine's current store and word map are (a map that does not fit the store does not refuse this call: nothing
 * of either is read), so a session can always be emptied for sr_gram_live_set_grammar. */
int sr_gram_live_end(sr_gram_live *l, const uint32_t *channels, uint32_t n_ch, sr_chain_rec *rec, sr_chain_word *words,
                     uint32_t *level_cost, sr_chain_live_row *rows, uint32_t *n_rows);

/* ------------------------------------------------------------------ word alternatives: every template over a decoded span
 * OPT-IN EXTENSION, NO REFERENCE COUNTERPART.  The decoders above say which word they chose for a stretch of frames, not how
 * close the second-best word was on it: A_l(p) keeps one candidate per end frame.  This section scores EVERY template over a
 * fixed span of frames, start and end pinned; the score rows are sr_nbest_batch_dev's input, so word map, N-best and count
 * apply per decoded word: a runner-up and a rejection margin, a correction list.  No existing call, record or score changes.
 * For a feature row in[0..N) (N clamped to max_frames), a span (S, e) and a valid slot k of M frames:
 *   F_k(S,e)  the minimum over the word paths of the connected-word section from (S, 0) to (e, M-1) -- steps (+1,+1), (+1,0),
 *             (0,+1), every horizontal or vertical step directly after a diagonal one, the start cell of the non-diagonal
 *             kind -- of the sum of d = get_dis (DTW.C:45-62): the spotter's recurrence with the one start column S.
 *   reach     with L = e - S + 1, F is finite exactly when M/2 + 1 <= L <= 2M - 1 (integer division; M = 1: L = 1 only).
 *   q_k(S,e)  F / (L + M): the spotter's q, the decoder's sr_chain_word.dis.
 *   score row scores[k] = F_k in mode SR_SPAN_ACC, q_k in mode SR_SPAN_DIS; SR_DIS_ERR for an invalid slot, an unreachable
 *             (L, M) and an invalid span: start or end all ones, start > end, or end >= N.  Nothing outside rows [0, N) of the
 *             feature record is read.  Costs stay below 2^31: d <= 65 536 and a path has at most 2M - 1 cells.
 * Three facts (tests/test_span_ref.py, tests/test_span.py):
 *   1. For every word row ANY decoder of this library emits -- unconstrained, grammar, weighted grammar, live -- F_slot(start,
 *      end) == acc and q_slot == dis: acc is the word's own path cost, and the tuple minimum keeps the cheapest path from its
 *      start.
 *   2. For the unconstrained decoder the decoded slot is the first minimum in slot order of F_k(start, end) over the valid
 *      slots: another slot with a smaller F, or an equal F and a smaller index, would have won A_l(end + 1) under the (cost,
 *      start, slot) rule.  So entry 0 of sr_nbest_batch over the span's SR_SPAN_ACC row has slot == words[i].slot and dis ==
 *      words[i].acc, under any word map.
 *   3. Under a grammar fact 2 need not hold: the grammar may forbid the acoustically best word.  Entry 0 is then the best word
 *      REGARDLESS of syntax.
 * Out of scope: alternatives restricted to a grammar's arcs; sessions that score spans themselves (they do not keep the
 * feature history: a live or grammar caller who keeps its feature rows runs the stage call on the emitted word rows); free
 * span ends; N-best sequences. */
#define SR_SPAN_ACC 0u
#define SR_SPAN_DIS 1u
/* Stage level, DEVICE buffers: d_mfcc / d_in_frames / frames_stride as for sr_decode_words_dp_dev.  d_words[n_rows]
 * [words_per_row]: entry [r][i] is a span of feature row r and only its start and end are read -- any decoder's word rows
 * unchanged (entries at or beyond n_words are all ones: invalid spans), or spans of the caller's own making.  d_scores
 * [n_rows * words_per_row][K] u32 (required): every row is written whole, every score exactly once; two runs give the same
 * bytes.  words_per_row 1..16.  One asynchronous operation on `stream`; the host knows every count, nothing is read back.
 * Errors, before anything is launched or written: SR_ERR_BAD_CONFIG unless n_coef == 12; SR_ERR_NO_TEMPLATES; SR_ERR_BAD_ARG
 * for a null pointer, frames_stride 0, words_per_row outside 1..16, a mode other than the two above, more than 2^31 - 1
 * spans, a store of more than 65 536 slots or one whose longest template exceeds sr_decode_geometry's out[2], d_words and
 * d_scores that overlap. */
int sr_score_word_spans_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                            uint32_t words_per_row, const sr_chain_word *d_words, uint32_t mode, uint32_t *d_scores, void *stream);
/* the same on HOST buffers (copy in, launch, copy out) */
int sr_score_word_spans(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                        uint32_t words_per_row, const sr_chain_word *words, uint32_t mode, uint32_t *scores);
/* The unconstrained decoder with alternatives, DEVICE buffers: sr_decode_words_dp_dev as it stands (its arguments, its rules,
 * the same bytes in d_rec / d_words / d_level_cost), then the span scores of its d_words in `mode`, then sr_nbest_batch_dev's
 * reduction over those n_rows * max_words score rows.  d_alts[n_rows][max_words][n_best] (required), d_n_matched[n_rows]
 * [max_words] (optional), d_span_scores[n_rows * max_words][K] (optional; NULL: the scores live in the engine's scratch).
 * Word positions at or beyond n_words get sr_nbest_batch's "no candidate" entries and n_matched 0.  n_best 1..SR_NBEST_MAX.
 * ONE asynchronous operation on `stream`.  Errors, before anything is launched or written: those of sr_decode_words_dp_dev,
 * of sr_score_word_spans_dev and of sr_nbest_batch_dev, and SR_ERR_BAD_ARG for outputs that overlap. */
int sr_decode_words_alts_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                             uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *d_rec,
                             sr_chain_word *d_words, uint32_t *d_level_cost, uint32_t n_best, uint32_t mode, sr_nbest_entry *d_alts,
                             uint32_t *d_n_matched, uint32_t *d_span_scores, void *stream);
/* the same on HOST buffers (copy in, launch, copy out) */
int sr_decode_words_alts(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                         uint32_t max_words, uint32_t n_words_exact, uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *rec,
                         sr_chain_word *words, uint32_t *level_cost, uint32_t n_best, uint32_t mode, sr_nbest_entry *alts,
                         uint32_t *n_matched, uint32_t *span_scores);

/* ------------------------------------------------------------------ full-DP alignment and word models from many examples
 * OPT-IN EXTENSION, NO REFERENCE COUNTERPART.  sr_dtw_dp_batch_dev says how far a feature row is from a template; this
 * section says HOW the two were aligned, and builds word models from many examples on top of that (DTW barycentre
 * averaging).  Neither call reads or writes the engine's template store; no existing call, record or score changes.
 *   pair     an input row in[0..N) and a reference ref[0..R), both 12 x s16 per frame.
 *   d(x,y)   get_dis (DTW.C:45-62), as in every other scorer.
 *   gate     sr_dtw_dp_batch's: N >= 1, R >= 1 and not (N > 2R or 2N < R).
 *   cells    those inside dtw_limit's parallelogram (DTW.C:76-109).
 *   D        D(1,1) = d(1,1); D(x,y) = d(x,y) + min(D(x-1,y-1), D(x-1,y), D(x,y-1)).
 *   acc, dis acc = D(N,R), dis = acc / (N + R): exactly the value sr_dtw_dp_batch_dev writes for the same pair.
 *   path     traced back from (N,R) to (1,1): at each cell the reachable predecessor of minimal D; on ties (x-1,y-1), then
 *            (x-1,y), then (x,y-1).  The steps are monotone, so the path is one span per input frame:
 *            span[x] = y_first | y_last << 16, the 0-based inclusive reference rows matched to input frame x, and
 *            path_len = sum over x of (y_last - y_first + 1).
 *   status   SR_AL_TOO_LONG: N (after the clamp to max_frames) above SR_ALIGN_MAX_FRAMES -- it takes precedence;
 *            SR_AL_GATED: an empty row, a pair that fails the gate, an unreachable end cell, or an invalid reference (its
 *            index >= n_ref, its frame count 0 or above ref_rows); SR_AL_OK otherwise.
 * A record that is not OK has dis = SR_DIS_ERR, acc = 0xFFFFFFFF, path_len = 0 and a span row of 0xFFFFFFFF.  On every call
 * the span entries at x >= N are 0xFFFFFFFF; every record and every span row is written whole.
 * SR_ALIGN_MAX_FRAMES: the predecessor marks cost 2 bits per cell -- 256 KiB per pair at 1024 x 1024, 67 MB at the 16 383-frame
 * cap -- and enrolment material is words, not recordings. */
#define SR_ALIGN_MAX_FRAMES 1024u
#define SR_AL_OK 0u
#define SR_AL_GATED 1u
#define SR_AL_TOO_LONG 2u
typedef struct sr_align_rec { /* 16 bytes */
    uint32_t dis;
    uint32_t acc;
    uint32_t path_len;
    uint32_t status;
} sr_align_rec;
/* DEVICE buffers: d_mfcc[n_rows][max_frames][12]; d_in_frames / frames_stride as for sr_rescore_nbest_dp_dev (a count above
 * max_frames is clamped; nothing outside rows [0, frames) of a record or of a reference is read).  d_ref[n_ref][ref_rows][12],
 * d_ref_frames[n_ref].  d_ref_of_row[n_rows]: the reference of each row; NULL: row r pairs with reference r, then n_ref must be
 * >= n_rows.  d_rec[n_rows] (required), d_span[n_rows][max_frames] (optional).  Asynchronous on `stream`, no host
 * synchronisation, no read-back; a call whose marks do not fit the LDS keeps them in the engine's scratch and runs as
 * several launches on the same stream once they exceed 256 MiB.
 * Errors, before anything is launched or written: SR_ERR_BAD_CONFIG unless n_coef == 12; SR_ERR_BAD_ARG for a null required
 * pointer, frames_stride 0, ref_rows 0 or above SR_ALIGN_MAX_FRAMES, n_ref 0, n_ref < n_rows without d_ref_of_row, d_rec and
 * d_span overlapping. */
int sr_dtw_dp_align_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                        const int16_t *d_ref, const uint32_t *d_ref_frames, uint32_t ref_rows, uint32_t n_ref,
                        const uint32_t *d_ref_of_row, sr_align_rec *d_rec, uint32_t *d_span, void *stream);
/* the same on HOST buffers (copy in, launch, copy out) */
int sr_dtw_dp_align(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                    const int16_t *ref, const uint32_t *ref_frames, uint32_t ref_rows, uint32_t n_ref, const uint32_t *ref_of_row,
                    sr_align_rec *rec, uint32_t *span);
/* DBA training: M word models refined from E = ex_start[M] example rows in n_iter iterations (1..16).  Model m has the
 * centroid C_m of F_m = cen_frames[m] frames and the examples e in [ex_start[m], ex_start[m+1]).  One iteration:
 *   - every example is aligned as input against C_m as reference;
 *   - for every OK example and every path point (x,y): sum[y][c] += in_e[x][c], cnt[y] += 1;
 *   - C'_m[y][c] = cnt[y] ? sum[y][c] / cnt[y] : C_m[y][c], s32 division truncating toward zero (get_mean, DTW.C:195-205);
 *   - F_m never changes; a model without an OK example stays as it is; output rows at or beyond F_m are zero;
 *   - a centroid whose frame count is 0 or above cen_rows is invalid: all its cen_rows rows are copied through unchanged
 *     and its examples are GATED.
 * Iterations chain: the output of iteration i is the centroid set of iteration i + 1.  The sums are integers, so the result
 * does not depend on the order in which examples are accumulated: two runs give identical bytes.
 * stats (optional) [n_iter][M]: the OK and the failed examples of model m in that iteration and the sum of the OK examples'
 * acc against the centroid that ENTERED it.
 * ex_start[M+1] is a HOST array in both forms (ascending, ex_start[0] = 0), so that the call can check before anything is
 * launched that (examples of m) x min(max_frames, SR_ALIGN_MAX_FRAMES) <= 65 535 for every model: then cnt stays within u16
 * range and |sum| < 2^31 -- the s32 accumulators are exact.
 * d_cen_in / d_cen_out[M][cen_rows][12] (the layout sr_set_templates_dense takes with tpl_stride = cen_rows*12); d_cen_out must
 * not overlap d_cen_in.  The device form is ONE asynchronous operation on `stream`; marks, accumulators and the intermediate
 * centroid set live in the engine's scratch.
 * Errors as sr_dtw_dp_align_dev's, and SR_ERR_BAD_ARG for M 0, cen_rows 0 or above SR_ALIGN_MAX_FRAMES, n_iter outside 1..16,
 * an ex_start that is not ascending from 0, the accumulator bound above, overlapping outputs. */
typedef struct sr_train_stat { /* 16 bytes */
    uint32_t n_ok;
    uint32_t n_fail;
    uint64_t acc;
} sr_train_stat;
int sr_train_models_dp_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride,
                           const uint32_t *ex_start, uint32_t M, const int16_t *d_cen_in, const uint32_t *d_cen_frames,
                           uint32_t cen_rows, uint32_t n_iter, int16_t *d_cen_out, sr_train_stat *d_stats, void *stream);
int sr_train_models_dp(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, const uint32_t *ex_start,
                       uint32_t M, const int16_t *cen_in, const uint32_t *cen_frames, uint32_t cen_rows, uint32_t n_iter,
                       int16_t *cen_out, sr_train_stat *stats);
/* Host-only, MI355X's LDS figures: out[0] = bytes of global scratch per pair for the predecessor marks (0: they live in LDS),
 * out[1] = pairs per launch, out[2] = SR_ALIGN_MAX_FRAMES. */
int sr_align_geometry(uint32_t max_frames, uint32_t ref_rows, uint32_t out[3]);

/* ------------------------------------------------------------------ word models: clustering a word's examples into templates
 * OPT-IN EXTENSION, NO REFERENCE COUNTERPART.  The store holds several templates per word (sr_set_word_map); this section
 * produces them from a corpus: k-means under DTW -- assign every example to the nearest centroid OF ITS WORD, re-average
 * each centroid from the examples it received (one DBA iteration of sr_train_models_dp), repeat.  Neither call reads or
 * writes the engine's template store; no existing call, record or score changes.  pair, d, gate, cells, D, acc, dis, path
 * and status are those of the section above, verbatim.
 *   inputs   W words.  Word w owns the example rows [word_start[w], word_start[w+1]) of mfcc[E][max_frames][12] and the
 *            models [mdl_start[w], mdl_start[w+1]) of cen[M][cen_rows][12] with cen_frames[M].  word_start[W+1] and
 *            mdl_start[W+1] are HOST arrays, as ex_start is, and ascend from 0; E = word_start[W], M = mdl_start[W].  Every
 *            word has 1..SR_CLUSTER_MAX models; a word may have no examples.
 *   score    for example e of word w and model m of w: s(e,m) = the aligner's dis of the pair (row e as input, centroid m as
 *            reference) -- exactly what sr_dtw_dp_align_dev and sr_dtw_dp_batch_dev give for it -- and SR_DIS_ERR when the
 *            pair is not SR_AL_OK: an empty row, a failed gate, an unreachable end cell, an invalid centroid (frame count 0
 *            or above cen_rows), or N above SR_ALIGN_MAX_FRAMES.
 *   assign   assign[e] = the first minimum in model order of s(e,m) over the models of e's word (the key is (dis, m)), as
 *            the model's index in [0, M).  If every score is SR_DIS_ERR: assign[e] = SR_CLUSTER_NONE (unassigned) and
 *            best[e] = SR_DIS_ERR; otherwise best[e] = s(e, assign[e]).
 *   iteration  assign against the centroid set that ENTERS it, then ONE DBA iteration of sr_train_models_dp's definition
 *            with model_of = assign: same sums, same s32 division truncating toward zero; rows nobody matched stay, F_m
 *            never changes, rows past F_m are zero, an invalid centroid is copied through.  A model that received no
 *            example stays as it is; unassigned examples contribute nothing.  Iterations chain.
 *   per iteration  stats[n_iter][M] (sr_train_stat): n_ok = the examples assigned to m, acc = the sum of their acc against
 *            the entering centroid, n_fail = 0.  iter[n_iter] (sr_cluster_iter): n_assigned + n_unassigned = E; n_moved =
 *            the examples whose assignment differs from the previous iteration's (before the first, every example is
 *            unassigned); n_empty = the models with n_ok == 0; acc = the sum of stats[.].acc.
 *   final    assign_out[E] = the assignment of the LAST iteration (made against the set that entered it, not against
 *            cen_out); cen_out[M][cen_rows][12] in sr_set_templates_dense's layout.
 *   exact    checked on the host before anything is launched: (examples of WORD w) x min(max_frames, SR_ALIGN_MAX_FRAMES)
 *            <= 65 535 for every word -- any one model of the word may receive all of them.  All sums are integers and
 *            all counters integer atomics: two runs give identical bytes.
 * Out of scope: choosing the number of clusters, splitting or merging clusters, changing a centroid's length, clustering
 * across words. */
#define SR_CLUSTER_MAX 16u
#define SR_CLUSTER_NONE 0xFFFFFFFFu
typedef struct sr_cluster_iter { /* 24 bytes */
    uint32_t n_assigned;
    uint32_t n_unassigned;
    uint32_t n_moved;
    uint32_t n_empty;
    uint64_t acc;
} sr_cluster_iter;
/* The stage: which model of its word every example is closest to.  DEVICE buffers as sr_train_models_dp_dev's (d_mfcc,
 * d_in_frames / frames_stride, d_cen, d_cen_frames); d_assign[E] (required), d_best[E] (optional), d_scores[E]
 * [SR_CLUSTER_MAX] (optional): s(e, mdl_start[w] + c) in column c, SR_DIS_ERR at and beyond the word's model count.  Every
 * output row is written whole.  ONE asynchronous operation on `stream`: nothing is read back, no host synchronisation; the
 * per-example tables (and the scores when d_scores is NULL) live in the engine's scratch.
 * Errors, before anything is launched or written: those of sr_train_models_dp_dev that apply (SR_ERR_BAD_CONFIG unless
 * n_coef == 12; SR_ERR_BAD_ARG for a null required pointer, frames_stride 0, cen_rows 0 or above SR_ALIGN_MAX_FRAMES), and
 * SR_ERR_BAD_ARG for W 0, a word_start or mdl_start that does not ascend from 0, a word with 0 or more than SR_CLUSTER_MAX
 * models, the bound above, overlapping outputs. */
int sr_cluster_assign_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride,
                          const uint32_t *word_start, const uint32_t *mdl_start, uint32_t W, const int16_t *d_cen,
                          const uint32_t *d_cen_frames, uint32_t cen_rows, uint32_t *d_assign, uint32_t *d_best, uint32_t *d_scores,
                          void *stream);
/* the same on HOST buffers (copy in, launch, copy out) */
int sr_cluster_assign(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, const uint32_t *word_start,
                      const uint32_t *mdl_start, uint32_t W, const int16_t *cen, const uint32_t *cen_frames, uint32_t cen_rows,
                      uint32_t *assign, uint32_t *best, uint32_t *scores);
/* The full operation: n_iter (1..16) iterations as ONE asynchronous operation on `stream`.  d_cen_out (required) must not
 * overlap d_cen_in; d_assign[E], d_stats[n_iter][M] and d_iter[n_iter] are optional, and leaving one out changes nothing
 * else.  Scores, assignment maps, accumulators and the intermediate centroid set live in the engine's scratch.  Errors as
 * above, and SR_ERR_BAD_ARG for n_iter outside 1..16. */
int sr_cluster_models_dp_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride,
                             const uint32_t *word_start, const uint32_t *mdl_start, uint32_t W, const int16_t *d_cen_in,
                             const uint32_t *d_cen_frames, uint32_t cen_rows, uint32_t n_iter, int16_t *d_cen_out, uint32_t *d_assign,
                             sr_train_stat *d_stats, sr_cluster_iter *d_iter, void *stream);
int sr_cluster_models_dp(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, const uint32_t *word_start,
                         const uint32_t *mdl_start, uint32_t W, const int16_t *cen_in, const uint32_t *cen_frames, uint32_t cen_rows,
                         uint32_t n_iter, int16_t *cen_out, uint32_t *assign, sr_train_stat *stats, sr_cluster_iter *iter);

/* ------------------------------------------------------------------ forced alignment against a transcript:
 * word models trained on connected speech
 * OPT-IN EXTENSION, NO REFERENCE COUNTERPART.  The trainers above learn from one word per feature row; the decoders hold the
 * result against words spoken without pauses.  This section aligns a corpus of connected recordings to their KNOWN
 * transcripts, one transcript per row, and cuts the rows at the word boundaries into the trainers' example layout.  Neither
 * call reads a grammar or writes the template store; no existing call, record or score changes.
 *
 * THE RULE.  Row r has the transcript t[r][0..n_r), labels of the engine's word map (sr_set_word_map), n_r = n_words[r] in
 * 0..words_per_row, words_per_row in 1..16.  Everything is the connected-word decoding section's: d, the word path, E_0, the
 * charged start, the key (cost, start, slot), E_l, the trace, skip_cost, word_cost, every limit.  Two things change:
 *   level    at level l the minimum of A_l runs only over the VALID slots whose label is t[r][l-1];
 *   count    it is exactly n_r.
 *   status   SR_CH_NONE (cost SR_DIS_ERR, n_words 0, skipped 0, every word row all ones) when n_r = 0, when a transcript word
 *            has no valid slot, or when E_{n_r}(N) is not finite; SR_CH_OK otherwise.
 *   outputs  d_rec[n_rows]; d_words[n_rows][words_per_row], entries at and beyond n_r all ones; sr_chain_word.reserved is the
 *            word's 1-based position.  There is no level_cost output, and the levels below n_r are not part of the contract.
 * Anchor: for a row with n_r >= 1, the record and the n_r word rows are byte for byte what sr_decode_grammar_dp writes for it
 * under the sequence grammar (state i --t[r][i]--> state i+1, the last state final) with max_words = n_words_exact = n_r.  A
 * grammar belongs to a call, so that route costs one grammar and one one-row call per recording; this call takes R rows with R
 * transcripts at once.
 *
 * EXACT COLUMN PRUNING, which only a linear transcript allows.  minlen(w) = the minimum of M/2 + 1 over the valid slots of w
 * (M frames of template need M/2 + 1 frames of input at least -- the span section's reach rule; 1 for M = 1).  tail_l = the sum
 * of minlen over the positions after l.  Level l of row r is swept only over the end frames e with e + 1 <= N - tail_l.  Record
 * and word rows do not change: a word of level l+1 that starts after N - tail_l ends after N - tail_{l+1}, which is itself
 * pruned; E_l(p) for p <= N - tail_l depends only on A_l(j <= p); the trace enters level l at a start <= N - tail_l; and level
 * n_r has tail 0.  The host uploads tail per (row, level); N is a device value, so the kernel forms the bound itself.  A sweep
 * that no reachable start has entered yet exits as well (E_{l-1} is unreachable in the early columns of a late level).
 *
 * Arguments: d_mfcc, d_in_frames / frames_stride, n_rows as for sr_decode_words_dp_dev.  transcript[n_rows][words_per_row] and
 * n_words[n_rows] are HOST arrays in both forms, as ex_start is: the host knows every item and count, builds the per-level
 * lists of (row, slot) word passes the kernel's grid runs over and uploads them once per call (a pageable source is staged
 * before the call returns).  ONE asynchronous operation on `stream`: nothing is read back; two runs give identical bytes;
 * every record and every word row is written whole.  Scratch is the decoder's at max_words = words_per_row, and a call is cut
 * into launch groups by the same rule (sr_decode_geometry).
 * Errors, before anything is launched or written: those of sr_decode_words_dp_dev; SR_ERR_BAD_ARG for words_per_row outside
 * 1..16, an n_words[r] above words_per_row, a transcript label that no slot of the word map carries (sr_last_error names row
 * and position), d_rec overlapping d_words.
 *
 * Out of scope: alternatives per position in a transcript; optional words; live sessions; a device-side store update (the
 * store is set from host memory: a training loop reads its centroids back once per iteration); changing template lengths. */
int sr_align_transcripts_dp_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride,
                                uint32_t n_rows, const uint32_t *transcript, const uint32_t *n_words, uint32_t words_per_row,
                                uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *d_rec, sr_chain_word *d_words, void *stream);
/* the same on HOST buffers (copy in, launch, copy out) */
int sr_align_transcripts_dp(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                            const uint32_t *transcript, const uint32_t *n_words, uint32_t words_per_row, uint32_t skip_cost,
                            uint32_t word_cost, sr_chain_rec *rec, sr_chain_word *words);
/* Word spans to example rows.  d_words[n_rows][words_per_row] (1..16) are ANY decoder's word rows over the feature rows
 * d_mfcc / d_in_frames; only start and end are read.  dst_of_span[n_rows * words_per_row] is a HOST array: the example index
 * (below n_ex) span i is copied to, or all ones for "not wanted"; the indices are distinct.  d_ex[n_ex][ex_rows][12] and
 * d_ex_frames[n_ex] are written whole: a valid span (start <= end < N, N clamped to max_frames) of L = end - start + 1 <=
 * ex_rows frames puts the frames start..end into rows 0..L-1, zero behind them, and ex_frames = L; an invalid span, L above
 * ex_rows and an example no span names give a zero row with ex_frames = 0, which the trainers gate as an empty row.  Nothing
 * outside the rows [0, N) is read.  ONE asynchronous operation on `stream`; the table derived from dst_of_span lives in the
 * engine's scratch.  Errors, before anything is launched or written: SR_ERR_BAD_CONFIG unless n_coef == 12; SR_ERR_BAD_ARG for
 * a null pointer, frames_stride 0, words_per_row outside 1..16, ex_rows 0 or above SR_ALIGN_MAX_FRAMES, a destination at or
 * above n_ex or named twice, feature rows or d_ex not 4-byte aligned, d_ex overlapping d_ex_frames. */
int sr_gather_word_spans_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                             const sr_chain_word *d_words, uint32_t words_per_row, const uint32_t *dst_of_span, uint32_t n_ex,
                             uint32_t ex_rows, int16_t *d_ex, uint32_t *d_ex_frames, void *stream);
int sr_gather_word_spans(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                         const sr_chain_word *words, uint32_t words_per_row, const uint32_t *dst_of_span, uint32_t n_ex, uint32_t ex_rows,
                         int16_t *ex, uint32_t *ex_frames);

/* ------------------------------------------------------------------ one-pass connected-word decoding: no word cap
 * OPT-IN EXTENSION, NO REFERENCE COUNTERPART.  Level building (the connected-word decoding section) keeps one prefix-cost
 * array per word count: a row holds at most 16 words and a call pays max_words x K x M x N cells.  This section keeps ONE
 * prefix-cost array E(p) over all word counts: a row holds as many words as its frames allow, and a call pays 2 x K x M x N
 * cells whatever that number is.  No existing call, record or byte changes.
 * Everything not restated here is the connected-word decoding section: d, the word path, skip_cost, word_cost, the key
 * cost << 32 | start << 16 | slot, sr_chain_rec, sr_chain_word.
 *   E(0)     0.
 *   D_k      per valid slot k the spotter's recurrence with a charged start, D_k(x,0) = E(x) + d(x,0), S = x, the start
 *            unreachable where E(x) is.
 *   A(p)     p >= 1: the minimum over the valid slots of (D_k(p-1, M_k-1) + word_cost, S, k), compared as (cost, start, slot).
 *   E(p)     min(A(p).cost, E(p-1) + skip_cost), the second term only when skipping is on.
 *   result   E(N) unreachable, or N = 0: status SR_CH_NONE, with the decoder's NONE record (cost SR_DIS_ERR, n_words 0,
 *            skipped 0, every word row all ones).  Otherwise SR_CH_OK, cost = E(N), n_words = the words on the trace.  That may
 *            be 0: with skipping on a row that is cheaper as filler than as any word is a legitimate "nothing was said", with
 *            cost = N * skip_cost and skipped = N.
 *   trace    p = N; while p > 0: if A(p) is unreachable or A(p).cost != E(p), frame p-1 is skipped and p -= 1; else the word
 *            is A(p): end = p-1, cum = E(p), acc = A(p).cost - word_cost - E(start), and p = start.  A word is preferred to
 *            filler at equal cost, as in the level decoder's trace.
 *   output   d_words[n_rows][words_cap], words_cap >= 1 of any size, words in spoken order, entries at or beyond n_words all
 *            ones, reserved = 0.  When n_words > words_cap the FIRST words_cap words are written, sr_chain_rec.n_words is the
 *            true count and status is SR_CH_TRUNCATED (cost and skipped as for SR_CH_OK).
 *   levels   E(N) = min(N * skip_cost when skipping is on, min over n >= 1 of E_n(N)) with n unbounded.  Where that minimum
 *            is unique and has at most 16 words, the word rows equal sr_decode_words_dp's at max_words 16, cum included.
 *            Under ties the two decoders may choose differently: level building prefers the fewest words globally, this
 *            decoder traces locally (a word before filler at every position).  Byte equality with the level decoder is NOT
 *            promised.
 *   blocks   a word over a template of M frames spans at least M / 2 + 1 input frames, so with L = the minimum of M_k / 2 + 1
 *            over the valid slots, A and E over a block of L positions depend only on E at or before the block's first
 *            frame.  The call runs as ceil(frames_cap / L) blocks ordered by the stream alone; inside a block all rows and
 *            slots run in parallel and every column is swept twice.
 *   limits   skip_cost <= 65 535 or SR_DIS_ERR; word_cost <= 2^24 and (frames_cap / L) * word_cost <= 2^30: a row holds at
 *            most N / L words, and 3 * 16 383 * 65 536 + 2^30 < 2^32 - 1, so u32 costs stay exact; a store of at most 65 536
 *            slots.  Arguments outside these limits are refused.
 * Out of scope: grammars, n_words_exact, N-best sequences.  (The push-by-push session is the next section.) */
#define SR_CH_TRUNCATED 2u
/* Stage level, DEVICE buffers: d_mfcc / d_in_frames / frames_stride as for sr_decode_words_dp_dev.  frames_cap is a HOST-side
 * bound on the frames of every row, 0 = max_frames: N is clamped to min(max_frames, frames_cap), and frames_cap fixes the
 * number of blocks -- the host never reads the device counts.  d_rec[n_rows] and d_words[n_rows][words_cap] are written whole
 * on every call.  ONE asynchronous operation on `stream` (keys, prefix costs and one saved column per (row, slot) live in the
 * engine's scratch, sr_decode_onepass_geometry), no host synchronisation, no read-back; two runs give the same bytes.
 * Errors, before anything is launched or written: SR_ERR_BAD_CONFIG unless n_coef == 12; SR_ERR_NO_TEMPLATES; SR_ERR_BAD_ARG
 * for a null pointer, frames_stride 0, words_cap 0, an argument outside the limits above, a word map that does not fit the
 * store, a store whose longest template exceeds sr_decode_geometry's out[2], outputs that overlap. */
int sr_decode_onepass_dp_dev(sr_engine *h, const int16_t *d_mfcc, const uint32_t *d_in_frames, uint32_t frames_stride, uint32_t n_rows,
                             uint32_t frames_cap, uint32_t words_cap, uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *d_rec,
                             sr_chain_word *d_words, void *stream);
/* the same on HOST buffers (copy in, launch, copy out) */
int sr_decode_onepass_dp(sr_engine *h, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride, uint32_t n_rows,
                         uint32_t frames_cap, uint32_t words_cap, uint32_t skip_cost, uint32_t word_cost, sr_chain_rec *rec,
                         sr_chain_word *words);
/* Whole path on HOST buffers: sr_mfcc_batch_status (its arguments, its per-record failure rules; mfcc, frm_num and status
 * may be NULL here) followed by the stage over those rows with frames_cap = max_frames; a failed record has no parse. */
int sr_decode_onepass_batch(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B, const int32_t *start,
                            const int32_t *end, const uint32_t *mid, uint32_t words_cap, uint32_t skip_cost, uint32_t word_cost,
                            sr_chain_rec *rec, sr_chain_word *words, int16_t *mfcc, uint32_t *frm_num, uint32_t *status);
/* Host-only: a store of K slots whose longest template has tpl_rows rows and whose shortest valid one has min_tpl_frames
 * frames.  out[0] = state bytes per row (keys, prefix costs, saved columns), out[1] = rows per launch group (what 256 MiB of
 * scratch hold, 65 535 at most), out[2] = the block length L = min_tpl_frames / 2 + 1, out[3] = launches per group,
 * 2 * ceil(max_frames / L) + 2. */
int sr_decode_onepass_geometry(uint32_t tpl_rows, uint32_t K, uint32_t max_frames, uint32_t min_tpl_frames, uint32_t out[4]);

/* ------------------------------------------------------------------ live one-pass connected-word decoding: no word cap, state carried between pushes
 * OPT-IN EXTENSION, NO REFERENCE COUNTERPART.  The live connected-word decoding section holds at most 16 words per recording
 * and pays max_words levels per push.  A session of this section takes the frames of n_channels channels as they arrive, in
 * pushes of any size up to chunk_max, keeps per channel ONE A / E history, per (channel, slot) ONE saved column and the
 * channel's feature row on the device between calls, and after every push says how everything heard so far parses under the
 * one-pass section's definition: as many words as the frames allow, 2 x n x K x M cells per push of n frames, plus a trace.
 * No existing call, record or byte changes.
 * THE RULE: let Y_c be every feature frame pushed to channel c since it was opened or last ended, N = |Y_c|; N is at most
 * utt_frames, fixed at open in 1..16 383 (the u32 cost bound and the 16-bit start field of a key end there).  Every push
 * emits one row for every channel with n[c] > 0, by ascending channel: an sr_chain_rec and words_cap x sr_chain_word, compact
 * and labelled with sr_chain_live_row.  The row is, byte for byte, what the one-pass section defines for Y_c as ONE row of N
 * frames with the session's words_cap, skip_cost, word_cost and the engine's current word map -- whatever the chunking.
 * Whenever an engine's max_frames >= N it therefore equals what sr_decode_onepass_dp[_dev] writes for that row, under ties
 * too: the definition is the same and so is the tie rule.  start and end are 0-based frame indices of the channel's
 * recording.
 *   flags    0: the batch call's truncation -- when n_words > words_cap the FIRST words_cap words are written, n_words is the
 *            true count and status is SR_CH_TRUNCATED.  SR_OP_LIVE_TAIL: the LAST words_cap words of the trace instead, in
 *            spoken order in entries 0..words_cap-1 (a feed that runs past words_cap words wants the recent ones); the record
 *            is the same.  Any other flag is refused.
 *   blocks   why it is exact: the one-pass section's block argument asks of a block only that it is at most L frames long.  A
 *            push of n[c] frames is cut into ceil(n[c] / L) blocks; the first resumes from the column saved at the first frame
 *            of the channel's last block, whichever push that was in.  A word that starts inside a block cannot end inside
 *            it, so A and E over a block follow from E at or before its first frame.  A(p) and E(p) depend on frames < p
 *            only: the history of a recording is a prefix of that of any longer one, and the trace reads A, E and N.
 *   state    per channel on the device: A (u64) and E (u32) over utt_frames + 1 positions; one saved exact column per slot,
 *            K x tpl_rows x 16 bytes; and the channel's WHOLE feature row, utt_frames x 24 bytes, of which a block sweeps the
 *            at most L - 1 frames before the push again (a ring of L - 1 frames would do; the whole row needs no wrap and
 *            survives a store whose L differs).  Nothing is read back: the host mirror knows every channel's N and the first
 *            frame of its last block.
 *   limits   the one-pass section's; (utt_frames / L) * word_cost <= 2^30 is checked at open against the current store and
 *            again at every push.
 * PCM sessions (mid given at open): the channel's samples X_c, R = |X_c|, are framed exactly as the live word spotting section
 * frames them (a segment with start = 1, end = R and mid[c]); n[c] counts samples, a row is emitted for n[c] > 0 whether or
 * not a frame was completed, and while there are at most max_frames frames the row equals sr_decode_onepass_batch(X_c, 1, R,
 * mid[c]).
 * Refusals, stream ordering and the binding of a channel to its template store are the live connected-word decoding
 * section's: a call refused for its arguments, its counts or the store is refused before anything is enqueued, writes nothing
 * and changes no state; a push on another stream than the last push's is ordered behind it by an event; a push to a channel
 * whose store has been replaced returns SR_ERR_BAD_ARG until that channel is ended, and it ends with the SR_CH_NONE record.
 * The session uses its engine's scratch buffers: the engine's one-caller-at-a-time rule covers its sessions.
 * COMMITTED WORDS (sr_onepass_live_commit[_dev], below): the parse at N frames may change at N + 10, whole words included; a
 * commit call says which of its words are final.  With A, E as the one-pass section defines them:
 *   node     a position q >= 1 with A(q) reachable and A(q).cost == E(q), or 0.  end(p) = the largest node <= p: where the
 *            trace, started at p, finds its first word.  The walk from p is end(p) -> end(start(A(end(p)))) -> ... -> 0, its
 *            words are the words the trace writes from p.  A(p) and E(p) depend on frames < p only: a walk never changes.
 *   window   a word over M template frames covers at most 2M - 1 input frames (one start column, then at most one
 *            horizontal step per diagonal step), so with W = 2 * max_k M_k - 1 over the valid slots of the store the channel
 *            is bound to, every hypothesis alive in column N - 1 started at or after N - W.
 *   entries  the positions x in [max(0, N - W), N] where E(x) is reachable; if there are none, the single largest reachable
 *            x <= N (position 0 always qualifies; such a recording can no longer parse).
 *   c(N)     the deepest node shared by the walks from all entries.  The committed words are the words on the walk from
 *            c(N), and frames = c(N): every frame below it is decided.
 * Why they are final: the trace at any N' >= N goes down through positions where E is reachable, by one frame (a skipped
 * frame) or from a node to the start of its word.  Let x be the first of them that is <= N.  It was reached by a one-frame
 * step, then x = N; or as the start of a word that ends at or after frame N, then x = N or the word is alive in column N - 1
 * and x >= N - W.  Either way x is an entry, and from x on the trace is the walk from x, which runs through c(N).  So every
 * later parse of the recording, the end call's included, BEGINS with exactly the committed word rows, byte for byte, acc,
 * score and cum included; c(N) never moves backwards; and c(N) is a function of the recording and N alone, so it does not
 * depend on the chunking.  The rule is conservative by up to W frames: while N <= W nothing is committed.
 * Out of scope: recordings past 16 383 frames (forgetting a committed prefix), n_words_exact, N-best sequences; a tighter,
 * frontier-based marker (it needs the exact column at N - 1, which the device never has -- blocks charge nothing behind their
 * first frame -- and would depend on the chunking).  Grammar sessions commit by the same rule over (position, state) nodes:
 * sr_onepass_gram_live_commit[_dev], the live one-pass grammar decoding section. */
#define SR_OP_LIVE_TAIL 1u
typedef struct sr_onepass_live sr_onepass_live;
/* host-only, no device: a store of K slots whose longest template has tpl_rows rows and whose shortest valid one has
 * min_tpl_frames frames.  out[0] = device state bytes per channel, (utt_frames + 1) * 12 + K * tpl_rows * 16 + utt_frames * 24,
 * saturating; out[1] = the longest template that fits (sr_spot_geometry's out[2]); out[2] = L = min_tpl_frames / 2 + 1;
 * out[3] = the kernel launches a feature push of chunk_max frames enqueues at most, 2 * ceil(chunk_max / L) + 1: a sweep and a
 * close per block, and the trace (no launch initialises anything: see k_onepass_live.hip).  tpl_rows and utt_frames 1..16 383,
 * K 1..65 536, min_tpl_frames 1..tpl_rows, chunk_max 1..utt_frames. */
int sr_onepass_live_geometry(uint32_t tpl_rows, uint32_t K, uint32_t min_tpl_frames, uint32_t utt_frames, uint32_t chunk_max, uint32_t out[4]);
/* mid NULL: a feature session, chunk_max in frames, 1..utt_frames.  mid a HOST array [n_channels]: a PCM session, chunk_max in
 * samples; SR_ERR_BAD_ARG if a push of chunk_max samples could complete more than min(max_frames, utt_frames) frames.
 * n_channels 1..65535, words_cap >= 1.  Argument limits and configuration errors exactly as sr_decode_onepass_dp_dev. */
int sr_onepass_live_open(sr_engine *h, uint32_t n_channels, uint32_t chunk_max, uint32_t utt_frames, uint32_t words_cap, uint32_t flags,
                         uint32_t skip_cost, uint32_t word_cost, const uint32_t *mid, sr_onepass_live **out);
void sr_onepass_live_close(sr_onepass_live *l); /* before sr_destroy of its engine; waits for the session's last push */
/* One push: sr_decode_live_push_dev's arguments and rules without level costs.  n: HOST array [n_channels] in both forms,
 * 0 <= n[c] <= chunk_max, 0 leaves the channel untouched; NULL: n_all each.  Channel c's new frames are d_mfcc + c*row_stride;
 * nothing past n[c] frames of a row is read.  DEVICE form: d_mfcc 8-byte aligned, row_stride a multiple of 4; ONE asynchronous
 * operation on `stream`, no host synchronisation, no read-back.  d_rec[r] and d_words[r*words_cap + i] are COMPACT over the
 * emitted rows r; rows at and past *n_rows are not written.  rows[max_rows] and *n_rows are HOST outputs, filled from the
 * counts alone before the call returns.  Refused (SR_ERR_BAD_ARG): the word-cost bound against the current store, a count
 * above chunk_max, a channel bound to a replaced store, a push that would take a channel past utt_frames, max_rows below the
 * number of channels with n[c] > 0, a word map that does not fit, a null required pointer, outputs that overlap. */
int sr_onepass_live_push_dev(sr_onepass_live *l, const int16_t *d_mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all,
                             uint32_t max_rows, sr_chain_rec *d_rec, sr_chain_word *d_words, sr_chain_live_row *rows, uint32_t *n_rows,
                             void *stream);
/* the same on HOST buffers (2-byte aligned rows, any row_stride that holds the largest count) */
int sr_onepass_live_push(sr_onepass_live *l, const int16_t *mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all,
                         uint32_t max_rows, sr_chain_rec *rec, sr_chain_word *words, sr_chain_live_row *rows, uint32_t *n_rows);
/* PCM sessions: channel c's new samples are d_pcm + c*pcm_stride, n in samples; alignment rules as sr_spot_live_push_pcm_dev
 * (device form: 16-byte aligned, pcm_stride a multiple of 8).  The spot session's copy kernels and the frame kernel launch of
 * sr_mfcc_batch_dev turn them into the push's new frames, the decoder runs over those. */
int sr_onepass_live_push_pcm_dev(sr_onepass_live *l, const uint16_t *d_pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                                 uint32_t max_rows, sr_chain_rec *d_rec, sr_chain_word *d_words, sr_chain_live_row *rows,
                                 uint32_t *n_rows, void *stream);
int sr_onepass_live_push_pcm(sr_onepass_live *l, const uint16_t *pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                             uint32_t max_rows, sr_chain_rec *rec, sr_chain_word *words, sr_chain_live_row *rows, uint32_t *n_rows);
/* The listed channels' recordings end here: HOST outputs rec[n_ch], words[n_ch][words_cap] and rows[n_ch], of which *n_rows
 * rows are written -- one per DISTINCT listed channel, at its first mention: the parse of everything pushed to it (an empty
 * channel gives the SR_CH_NONE record).  Waits for the device.  Each listed channel is then as freshly opened, and bound to
 * the current store.  rows overlapping rec or words is refused like outputs that overlap in a push.  HIP failures as in
 * sr_decode_live_end. */
int sr_onepass_live_end(sr_onepass_live *l, const uint32_t *channels, uint32_t n_ch, sr_chain_rec *rec, sr_chain_word *words,
                        sr_chain_live_row *rows, uint32_t *n_rows);
/* The committed words of the listed channels (COMMITTED WORDS above), for feature and PCM sessions alike.  channels: a HOST
 * list as in the end call; one row per DISTINCT listed channel at its first mention, compact.  rows[n_ch] and *n_rows are
 * HOST outputs filled from the host mirror before the call returns -- the channel and its frames N; nothing is read back.
 *   n_committed  the true count of committed words at N
 *   first        the words earlier commit calls delivered for this recording
 *   n_new        min(n_committed - first, words_cap) (the session's words_cap)
 *   frames       c(N)
 * d_cwords[r*words_cap + i], i < n_new, are the words first .. first + n_new - 1 in spoken order, as the trace writes them;
 * the entries from n_new on are the all-ones row.  Per channel the session keeps a cursor on the device (8 bytes, outside
 * sr_onepass_live_geometry's state bytes): it advances by n_new, so the words delivered over the calls, concatenated, are
 * every committed word exactly once and in order, whatever words_cap is; a backlog drains over later calls.  A call with no
 * push in between returns n_new 0 (once drained) and the same n_committed; an empty channel gives {0, 0, 0, 0}.
 * sr_onepass_live_end returns what it always did and puts the cursors of the channels it ends back to zero; a caller that
 * wants the undelivered rest at the end opens the session with SR_OP_LIVE_TAIL and words_cap >= the words it can fall behind
 * by: the end call's record says n_words, so the rest are the last n_words - (first + n_new) entries of its row.
 * DEVICE form: ONE asynchronous operation on `stream`, no host synchronisation; it runs behind the session's last push by
 * the event rule of the pushes, and later pushes run behind it.  The HOST form writes host buffers and waits.
 * Refused (SR_ERR_BAD_ARG) before anything is enqueued, nothing written, no state changed: a null required pointer, a
 * channel past the session's last, a channel bound to a replaced store (end it first), a word map that does not fit, outputs
 * that overlap (the host form: rows inside crec or cwords too). */
typedef struct sr_commit_rec {
    uint32_t n_committed, first, n_new, frames;
} sr_commit_rec; /* 16 bytes */
int sr_onepass_live_commit_dev(sr_onepass_live *l, const uint32_t *channels, uint32_t n_ch, sr_commit_rec *d_crec, sr_chain_word *d_cwords,
                               sr_chain_live_row *rows, uint32_t *n_rows, void *stream);
int sr_onepass_live_commit(sr_onepass_live *l, const uint32_t *channels, uint32_t n_ch, sr_commit_rec *crec, sr_chain_word *cwords,
                           sr_chain_live_row *rows, uint32_t *n_rows);

/* ------------------------------------------------------------------ one-pass grammar decoding: word networks without a word cap
 * OPT-IN EXTENSION, NO REFERENCE COUNTERPART.  Grammar decoding (the grammar-constrained decoding and weighted grammars
 * sections) is level building: at most 16 words a row, max_words sweeps of every row.  A grammar with a loop -- "a command,
 * then any number of digits", a bigram model, a phone-number network -- describes sequences whose length the caller does not
 * know.  This section runs the one-pass recurrence over the states of a grammar: a row holds as many words as its frames
 * allow, and a call pays 2 x (kept items) x M x N cells whatever that number is.  No existing call, record or byte changes.
 * Everything not restated here is the one-pass section's: d, the word path, skip_cost, word_cost, the key (cost, start,
 * slot), sr_chain_rec, sr_chain_word, SR_CH_TRUNCATED.  Grammar notation is the weighted grammar's: states 0..S-1, state 0
 * the start, the charge list of a pair (t, w), final_cost.  The calls take an sr_grammar as sr_grammar_create[_weighted]
 * made it.
 *   E(0, 0)   0; E(0, s) unreachable for s != 0.
 *   charge    C(x; t, w) = the minimum over the (s, c) of the list of (t, w) with E(x, s) reachable of E(x, s) + c; else
 *             unreachable.  An unreachable E never has a cost added to it.
 *   D_k,t     per item (slot k, target t), k a valid slot of a word w with a pair (t, w): the spotter's recurrence with a
 *             charged start, D(x, 0) = C(x; t, w) + d(x, 0), S = x.
 *   A(p, t)   p >= 1: the minimum over the items into t of (D_k,t(p-1, M_k-1) + word_cost, S, k), compared as (cost, start,
 *             slot).
 *   E(p, t)   min(A(p, t).cost, E(p-1, t) + skip_cost), the second term only when skipping is on.
 *   result    over the final f with E(N, f) reachable: cost = min E(N, f) + final_cost[f], the end state the smallest such f.
 *             None, or N = 0: status SR_CH_NONE with the decoder's NONE record.
 *   trace     p = N, t = the end state; while p > 0: if A(p, t) is unreachable or A(p, t).cost != E(p, t), frame p-1 is
 *             skipped and p -= 1; else the word is A(p, t): end = p-1, cum = E(p, t), acc = A(p, t).cost - word_cost -
 *             C(start; t, w(k)), reserved = t; the source state is the smallest s of the list with E(start, s) reachable and
 *             E(start, s) + c = C(start; t, w(k)); p = start, t = s.
 *   output    as the one-pass section's, with the grammar state after each word in `reserved`.
 * Consequences:
 *   - n_words 0 with SR_CH_OK is possible only when state 0 is final and filler is cheaper than every accepted sequence.
 *   - The walk always ends in state 0: only E(0, 0) is reachable at position 0.
 *   - Under the anchor grammar (one final state, one loop per label) record and word rows are sr_decode_onepass_dp's bytes;
 *     reserved is 0 there, the anchor's only state.
 *   - Where the minimum over sr_decode_grammar_dp's level costs is unique and has at most 16 words, the word rows equal that
 *     decoder's at max_words 16.  When state 0 is final and skipping is on that minimum also includes N x skip_cost +
 *     final_cost[0].  Under ties the two decoders may choose differently.
 *   blocks    the one-pass section's argument, state by state: a word over M template frames spans at least M / 2 + 1 input
 *             frames whatever state it leads into, so A(p, t) depends on E(x, s) for x <= p - L only.  The call runs as
 *             ceil(frames_cap / L) blocks ordered by the stream alone.
 *   pruning   static, not per level.  An item (slot, target) is kept when its charge list contains a state reachable from
 *             state 0 in any number of arcs and its target reaches a final state.  The states whose E is kept are every state
 *             that a kept charge list names and every final state that can be reached -- states without an incoming arc too:
 *             with skipping on E(p, 0) = p x skip_cost of a sequence grammar's start state is what its first words build on.
 *             Pruning changes no byte.
 *   limits    the one-pass section's, with one arc per word and one final cost added: (frames_cap / L) x (word_cost + the
 *             grammar's largest arc cost) + its largest final cost <= 2^30, refused with SR_ERR_BAD_ARG otherwise; and one
 *             row's scratch -- S x (max_frames + 1) keys and prefix costs and one saved column per kept item -- within the
 *             256 MiB of a launch group.
 * Out of scope: n_words_exact, N-best sequences, word alternatives under this decoder (sr_score_word_spans takes its word
 * rows), grammars of more than 64 states, recordings past 16 383 frames.  (The push-by-push session is the section "live
 * one-pass grammar decoding" below.) */
/* Stage level, DEVICE buffers: sr_decode_onepass_dp_dev's arguments and rules with the grammar in front.  ONE asynchronous
 * operation on `stream`, no host synchronisation, no read-back; two runs give the same bytes.  Errors, before anything is
 * launched or written: sr_decode_onepass_dp_dev's, and SR_ERR_BAD_ARG for a null grammar, a grammar of another engine, a
 * grammar compiled before the last sr_set_templates* or sr_set_word_map, the cost bound above, a row whose scratch exceeds a
 * launch group (the message names row_bytes). */
int sr_decode_onepass_grammar_dp_dev(sr_engine *h, const sr_grammar *g, const int16_t *d_mfcc, const uint32_t *d_in_frames,
                                     uint32_t frames_stride, uint32_t n_rows, uint32_t frames_cap, uint32_t words_cap, uint32_t skip_cost,
                                     uint32_t word_cost, sr_chain_rec *d_rec, sr_chain_word *d_words, void *stream);
/* the same on HOST buffers (copy in, launch, copy out) */
int sr_decode_onepass_grammar_dp(sr_engine *h, const sr_grammar *g, const int16_t *mfcc, const uint32_t *in_frames, uint32_t frames_stride,
                                 uint32_t n_rows, uint32_t frames_cap, uint32_t words_cap, uint32_t skip_cost, uint32_t word_cost,
                                 sr_chain_rec *rec, sr_chain_word *words);
/* Whole path on HOST buffers: sr_decode_onepass_batch under the grammar. */
int sr_decode_onepass_grammar_batch(sr_engine *h, const sr_grammar *g, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                                    const int32_t *start, const int32_t *end, const uint32_t *mid, uint32_t words_cap, uint32_t skip_cost,
                                    uint32_t word_cost, sr_chain_rec *rec, sr_chain_word *words, int16_t *mfcc, uint32_t *frm_num,
                                    uint32_t *status);
/* Host-only: what a call with this grammar and frames_cap (0 = max_frames) takes.  out[0] = scratch bytes per row, saturating;
 * out[1] = rows per launch group (0: one row does not fit, the call is refused); out[2] = the block length L; out[3] =
 * launches per group, 2 x ceil(frames_cap / L) + 2; out[4] = kept items; out[5] = kept states. */
int sr_onepass_grammar_plan(const sr_grammar *g, uint32_t frames_cap, uint32_t out[6]);

/* ------------------------------------------------------------------ live one-pass grammar decoding: state carried between pushes
 * OPT-IN EXTENSION, NO REFERENCE COUNTERPART.  A grammar is for feeds -- a dialogue's command and its argument arrive as audio,
 * not as a finished row -- and the looping grammars are the ones the live grammar-constrained decoding section serves worst: 16
 * words at most, max_words sweeps per push.  A session of this section takes the frames of n_channels channels as they arrive,
 * in pushes of any size up to chunk_max, keeps the one-pass grammar decoder's state on the device between calls, and after
 * every push says how everything heard so far parses under the one-pass grammar decoding section's definition, at
 * 2 x n x (kept items) x M cells per push of n frames, plus a trace.  No existing call, record or byte changes.
 * THE RULE: let Y_c be every feature frame pushed to channel c since it was opened or last ended, N = |Y_c| <= utt_frames,
 * utt_frames fixed at open in 1..16 383.  Every push emits one compact row for every channel with n[c] > 0, by ascending
 * channel: an sr_chain_rec and words_cap x sr_chain_word (no level costs), labelled by an sr_chain_live_row that the host fills
 * before the call returns.  The row is, byte for byte and whatever the chunking, what the one-pass grammar decoding section
 * defines for Y_c as ONE row of N frames under the session's grammar, skip_cost and word_cost; `reserved` holds the state
 * after each word.  Ties are that decoder's -- so they are not sr_gram_live's.  Whenever an engine's max_frames >= N the row
 * therefore equals sr_decode_onepass_grammar_dp[_dev]'s.  A weighted grammar is taken as it is.  Under the anchor grammar the
 * bytes are sr_onepass_live_push_dev's.
 *   flags    SR_OP_LIVE_TAIL: the LAST words_cap words of the trace instead of the first, as in the live one-pass section; the
 *            record is the same.  Any other flag is refused.
 *   exact    why: A(p, t) and E(p, t) depend on frames below p only, so the history of a recording is a prefix of that of any
 *            longer one; a word that starts inside a block of at most L frames cannot end inside it, whatever state it leads
 *            into, so a push's frames may be cut into blocks at the push boundaries, each resumed from the column saved at
 *            the first frame of the channel's last block; and the trace reads A, E and N only.
 *   state    per channel on the device: A[S][utt_frames + 1] (u64 keys) and E[S][utt_frames + 1] (u32), dense by state index;
 *            one saved exact column per kept item, tpl_len x 16 bytes; the channel's whole feature row, utt_frames x 24 bytes.
 *            The kept items and states are the static pruning the grammar carries (the one-pass grammar decoding section).  A
 *            position of A that no push has reached holds all ones, E(0, 0) = 0 and E(0, s) is unreachable for s != 0: open,
 *            sr_onepass_gram_live_set_grammar and the end call establish and restore that and may synchronise; a push runs
 *            without an init launch and never synchronises.  A grammar that keeps no state parses nothing: its pushes launch
 *            the trace alone, and the feature row is neither written nor read.
 *   limits   (utt_frames / L) x (word_cost + the grammar's largest arc cost) + its largest final cost <= 2^30, checked at open
 *            and at sr_onepass_gram_live_set_grammar.  A stale grammar refuses pushes, so the store cannot change under a live
 *            bound.
 * The session's grammar, its switching and a grammar gone stale follow the live grammar-constrained decoding section: a grammar
 * compiled before the last sr_set_templates* or sr_set_word_map refuses every push until the channels are ended (each listed
 * recording is then DROPPED: the SR_CH_NONE record, frames = 0 -- whatever the engine's current store and word map are) and a
 * fresh grammar is set.  Teardown order: the session before its grammar, the grammar before the engine.
 * PCM sessions (mid given at open) share the spot session's front end exactly as the live one-pass section's do: a row is
 * emitted for n[c] > 0 whether or not a frame was completed; samples without a new frame give the parse so far again (that
 * push launches the trace only); while the recording has at most max_frames frames the row equals
 * sr_decode_onepass_grammar_batch(X_c, 1, R, mid[c]).
 * Refusals come in the order stale grammar, counts, inputs, outputs, device; a refused call writes nothing and changes no
 * state.  Stream ordering is the live connected-word decoding section's.
 * COMMITTED WORDS (sr_onepass_gram_live_commit[_dev], below): under a sequence or a looping grammar the row of a push is
 * SR_CH_NONE for most of an utterance -- no final state is reachable yet -- so a session tells its caller nothing until the
 * utterance completes.  A commit call says which words every parse this recording can still get begins with, from the state
 * the session keeps and without a sweep.  With A(p, t), E(p, t), the charge C(x; t, w) and the source state of a word as the
 * one-pass grammar section defines them:
 *   kept     the kept states and kept items are the grammar's static pruning lists, as sr_onepass_grammar_plan counts them.
 *            They do not depend on the testing hook "onepass_gram_prune_off": the hook changes what is swept, never what the
 *            rule ranges over.
 *   node     a pair (q, t), t a kept state, q >= 1, A(q, t) reachable and A(q, t).cost == E(q, t); or the root (0, 0).
 *            end(p, t) = the node (q, t) with the largest q <= p, the root if state t has none.  The parent of (q, t), whose
 *            word starts at x with source state s, is end(x, s); parents lie strictly below their children.  The walk from
 *            (p, t) is end(p, t), its parent, and so on down to the root; its words are what the trace writes from (p, t).
 *            A and E at p depend on frames < p only: a walk never changes.
 *   window   W = 2 * max M_k - 1 over the slots of the kept items (0 if none are kept): a word over M template frames covers at
 *            most 2M - 1 input frames.  The grammar changes only while every channel is empty, so W is constant over a
 *            recording.
 *   entries  the pairs (x, s), s a kept state, x in [max(0, N - W), N], with E(x, s) reachable; if there are none, every
 *            reachable (x, s) at the largest x <= N that has one ((0, 0) always qualifies where state 0 is kept; such a
 *            recording can no longer parse).
 *   c(N)     the deepest node shared by the walks from all entries.  Shared nodes lie on one chain and a walk holds one node
 *            per position, so it is the shared node at the largest position.  The committed words are the words on the walk
 *            from c(N), and frames = the position of c(N).
 * Why they are final: a later trace starts in a reachable final state and goes down through pairs whose E is reachable.  Take
 * its first pair (x, s) with x <= N.  If it was reached by a skipped frame, x = N.  Otherwise it is the start of a word that
 * ends at or after frame N: that word is alive in column N - 1, so x >= N - W.  Every state on a trace is kept: it is reachable
 * from state 0, and it is final or named by the charge list of an item whose target reaches a final state.  So (x, s) is an
 * entry, and from there the trace is the walk from (x, s), which passes through c(N).  Hence every later row of the recording
 * whose status is not SR_CH_NONE, the end call's included, BEGINS with exactly the committed word rows, byte for byte, acc,
 * score, cum and reserved included; c(N) never moves back; c(N) depends on the recording, the grammar and N only, not on the
 * chunking; and the rule is conservative by up to W frames.
 * How much it commits is the grammar's: a node is shared only where every hypothesis still alive runs through it.  With
 * skipping on, a start state that no word leads back into stays reachable at every frame -- everything so far skipped --
 * and the walk from there is the root alone: a later parse may still begin that way, and such a grammar commits nothing
 * while it skips.  States that count words (a sequence grammar's) keep the hypotheses of different word counts apart: they
 * share nothing before no state is reachable in the window any more, and then the fallback commits the whole sequence at
 * once.  States that words lead back into (loops, the anchor grammar's one state) are where walks merge and words commit
 * about W frames behind the speaker.
 * Words are committed WHILE THE ROW ITSELF IS STILL SR_CH_NONE.  They mean "if this recording ever parses, it begins thus"; if
 * the grammar's end is never reached, the caller has still been told the truth.  Under the anchor grammar every byte of the
 * commit outputs is sr_onepass_live_commit_dev's on the same pushes.
 * Out of scope: a grammar per channel; a history compacted to the kept states; a row for the best non-final state while an
 * utterance is incomplete; n_words_exact; N-best sequences; recordings past 16 383 frames (forgetting a committed prefix); a
 * frontier-based marker; commits in the level-building sessions (sr_gram_live, sr_decode_live). */
typedef struct sr_onepass_gram_live sr_onepass_gram_live;
/* host-only, no device.  out[0] = device state bytes per channel, S x (utt_frames + 1) x 12 + kept items x tpl_len x 16 +
 * utt_frames x 24, saturating (the commit cursor, 8 bytes per channel, lies outside these state bytes);
 * out[1] = the longest template that fits (sr_spot_geometry's out[2]); out[2] = L; out[3] = the
 * kernel launches a feature push of chunk_max frames enqueues, per_block x ceil(chunk_max / L) + 1 with per_block = (kept items ?
 * 1 : 0) + (kept states ? 1 : 0); out[4] = kept items; out[5] = kept states.  utt_frames 1..16 383, chunk_max 1..utt_frames. */
int sr_onepass_gram_live_geometry(const sr_grammar *g, uint32_t utt_frames, uint32_t chunk_max, uint32_t out[6]);
/* sr_onepass_live_open's arguments and rules with the grammar in front; SR_ERR_BAD_ARG also for a null grammar, a grammar of
 * another engine, a stale grammar and the cost bound above. */
int sr_onepass_gram_live_open(sr_engine *h, const sr_grammar *g, uint32_t n_channels, uint32_t chunk_max, uint32_t utt_frames,
                              uint32_t words_cap, uint32_t flags, uint32_t skip_cost, uint32_t word_cost, const uint32_t *mid,
                              sr_onepass_gram_live **out);
void sr_onepass_gram_live_close(sr_onepass_gram_live *l); /* before sr_grammar_destroy of its grammar; waits for the last push */
/* sr_gram_live_set_grammar's rules: g a fresh grammar of the session's engine, accepted only while every channel is empty
 * (SR_ERR_BAD_ARG otherwise, nothing changes).  The state is laid out for g -- what has to grow is allocated aside and swapped in
 * after the last allocation, so a failed allocation leaves the session as it was -- and the invariants above are put in place
 * under the new layout.  Waits for the device. */
int sr_onepass_gram_live_set_grammar(sr_onepass_gram_live *l, const sr_grammar *g);
/* The four push forms: sr_onepass_live_push[_pcm][_dev]'s arguments and rules. */
int sr_onepass_gram_live_push_dev(sr_onepass_gram_live *l, const int16_t *d_mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all,
                                  uint32_t max_rows, sr_chain_rec *d_rec, sr_chain_word *d_words, sr_chain_live_row *rows,
                                  uint32_t *n_rows, void *stream);
int sr_onepass_gram_live_push(sr_onepass_gram_live *l, const int16_t *mfcc, uint64_t row_stride, const uint32_t *n, uint32_t n_all,
                              uint32_t max_rows, sr_chain_rec *rec, sr_chain_word *words, sr_chain_live_row *rows, uint32_t *n_rows);
int sr_onepass_gram_live_push_pcm_dev(sr_onepass_gram_live *l, const uint16_t *d_pcm, uint64_t pcm_stride, const uint32_t *n,
                                      uint32_t n_all, uint32_t max_rows, sr_chain_rec *d_rec, sr_chain_word *d_words,
                                      sr_chain_live_row *rows, uint32_t *n_rows, void *stream);
int sr_onepass_gram_live_push_pcm(sr_onepass_gram_live *l, const uint16_t *pcm, uint64_t pcm_stride, const uint32_t *n, uint32_t n_all,
                                  uint32_t max_rows, sr_chain_rec *rec, sr_chain_word *words, sr_chain_live_row *rows,
                                  uint32_t *n_rows);
/* sr_onepass_live_end's arguments and rules.  With a stale grammar the listed recordings are dropped (above); the channels
 * are then empty, and their keys are wiped all the same. */
int sr_onepass_gram_live_end(sr_onepass_gram_live *l, const uint32_t *channels, uint32_t n_ch, sr_chain_rec *rec, sr_chain_word *words,
                             sr_chain_live_row *rows, uint32_t *n_rows);
/* The committed words of the listed channels (COMMITTED WORDS above): sr_onepass_live_commit[_dev]'s arguments, outputs and
 * delivery on a grammar session.  One row per DISTINCT listed channel at its first mention; rows and *n_rows are HOST outputs
 * filled from the host mirror before the call returns; the sr_commit_rec says n_committed, first, n_new = min(n_committed -
 * first, words_cap) and frames = the position of c(N); d_cwords[r*words_cap + i], i < n_new, are the words first .. first +
 * n_new - 1 as the trace writes them, `reserved` = the state after the word, the entries from n_new on the all-ones row.  Per
 * channel the session keeps a cursor on the device -- the words delivered and the last delivered word's node WITH its state, 8
 * bytes, outside sr_onepass_gram_live_geometry's state bytes -- so every committed word is delivered exactly once and in order,
 * and a backlog drains over later calls.  An empty channel gives {0, 0, 0, 0}; a grammar that keeps no state gives {0, 0, 0, 0}
 * for every channel.  sr_onepass_gram_live_end (dropped recordings of a stale grammar included) and
 * sr_onepass_gram_live_set_grammar put the cursors back to zero.
 * DEVICE form: ONE asynchronous operation on `stream`, no host synchronisation, nothing read back; it runs behind the
 * session's last push by the event rule of the pushes, and later pushes run behind it.  The HOST form writes host buffers and
 * waits.  A weighted grammar takes the kernel that judges charges with the arc costs; any other grammar the plain one.
 * Refused (SR_ERR_BAD_ARG) before anything is enqueued, nothing written, no state changed: a stale grammar (first, as in the
 * pushes), a null required pointer, a channel past the session's last, a word map that does not fit, outputs that overlap
 * (the host form: rows inside crec or cwords too). */
int sr_onepass_gram_live_commit_dev(sr_onepass_gram_live *l, const uint32_t *channels, uint32_t n_ch, sr_commit_rec *d_crec,
                                    sr_chain_word *d_cwords, sr_chain_live_row *rows, uint32_t *n_rows, void *stream);
int sr_onepass_gram_live_commit(sr_onepass_gram_live *l, const uint32_t *channels, uint32_t n_ch, sr_commit_rec *crec, sr_chain_word *cwords,
                                sr_chain_live_row *rows, uint32_t *n_rows);

/* EXTENSION, NO REFERENCE COUNTERPART (the thesis that accompanies the reference, p.32, lists difference cepstra as
 * future work; the firmware computes none): delta MFCC by the standard two-frame regression over the s16 rows,
 *   delta[t][c] = ((m[t+1][c] - m[t-1][c]) + 2*(m[t+2][c] - m[t-2][c])) / 10,
 * row indices clamped to [0, frames-1], s32 arithmetic, division truncating toward zero; rows >= frames are zero.
 * mfcc / delta: [B][max_frames][n_coef].  Never used by the recognition path or the reference-compatible symbols. */
int sr_delta_mfcc_batch(sr_engine *h, const int16_t *mfcc, const uint32_t *frames, uint32_t B, int16_t *delta);
int sr_delta_mfcc_batch_dev(sr_engine *h, const int16_t *d_mfcc, const sr_vad_rec *d_vad /* or */, const uint32_t *d_frames,
                            uint32_t B, int16_t *d_delta, void *stream);
/* generic 1024-point Q15 FFT of n independent packed-complex arrays (re = low half, im = high half) */
int sr_fft_q15_batch(sr_engine *h, const uint32_t *in, uint32_t *out, uint32_t n);
/* batched forms of the two small scalar symbols below (the same kernels get_dis() / dtw_limit() launch with n = 1):
 * get_dis (DTW.C:45-62) on n pairs of 12-coefficient rows a[i*12..], b[i*12..];
 * dtw_limit (DTW.C:76-109) on n points xy[2i] = x, xy[2i+1] = y for the file statics a dtw() call of in_frames against
 * mdl_frames leaves behind (DTW.C:129-130, 141-142); out[i] = 1: the point lies outside the parallelogram. */
int sr_get_dis_batch(sr_engine *h, const int16_t *a, const int16_t *b, uint32_t n, uint32_t *out);
int sr_dtw_limit_batch(sr_engine *h, const uint16_t *xy, uint32_t n, uint32_t in_frames, uint32_t mdl_frames, uint8_t *out);

/* ------------------------------------------------------------------ multi-GPU (one process, several MI355X)
 * Utterances are sharded over the devices (B_per_dev each), templates are replicated, the argmin is local, and the
 * path's single exchange step is ONE RCCL all-gather of the per-template score matrix over xGMI: after the call every
 * device holds u32 scores[n_dev*B_per_dev][K] in global utterance order -- what the firmware's slot scan
 * (main.c:279-291: cur_dis of every slot) produces, for every utterance of the job.  RCCL (librccl.so.1) is bound at
 * run time; without it sr_multi_create fails with SR_ERR_NO_DEVICE.  Processes that run one rank per GPU (MPI,
 * torchrun) keep one sr_engine each and use sr_allgather_scores on their own communicator. */
typedef struct sr_multi sr_multi;
int sr_multi_create(const sr_config *cfg, const int *devices, uint32_t n_dev, sr_multi **out); /* cfg->device ignored */
void sr_multi_destroy(sr_multi *m);
uint32_t sr_multi_num_devices(const sr_multi *m);
sr_engine *sr_multi_engine(sr_multi *m, uint32_t i); /* the engine of devices[i] */
int sr_multi_set_templates(sr_multi *m, const void *store, uint32_t n_slots, uint32_t stride_bytes);
int sr_multi_set_templates_dense(sr_multi *m, const int16_t *mfcc, const uint32_t *frames, const uint8_t *valid,
                                 uint32_t n_templates, uint32_t tpl_stride);
/* device-resident shards: d_pcm[i], d_results[i] (B_per_dev records) and d_scores_all[i] (n_dev*B_per_dev*K words) live
 * on devices[i]; asynchronous on streams[i] (hipStream_t; streams == NULL: internal streams, returns when drained) */
int sr_multi_recognize_dev(sr_multi *m, const uint16_t *const *d_pcm, uint64_t pcm_stride, uint32_t buf_len,
                           uint32_t B_per_dev, sr_result *const *d_results, uint32_t *const *d_scores_all,
                           void *const *streams);
/* host buffers: shards, uploads, recognises, gathers; results[B], scores[B*K] (optional, read back from devices[0]) */
int sr_multi_recognize(sr_multi *m, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                       sr_result *results, uint32_t *scores);
/* the exchange step alone on a caller-owned ncclComm_t: d_all[n_ranks*count] <- all ranks' d_scores[count] */
int sr_allgather_scores(void *nccl_comm, const uint32_t *d_scores, uint32_t *d_all, uint64_t count, void *stream);

/* ------------------------------------------------------------------ measurement hooks (bench.py)
 * sr_recognize_batch_dev cuts a large batch into chunks (at least min_chunk = 4096 utterances each, at most
 * max_chunks = 12; one chunk per stream once the store holds 256 templates or more) and runs them on streams = 3 (max 4)
 * internal streams forked from / joined to the
 * caller's stream, so each kernel is launched once per chunk and kernels of different chunks overlap
 * (sr_set_pipeline changes the three numbers; streams = 1 keeps everything on the caller's stream).  The library reads
 * no tuning knob from the environment (the only environment variable it honours is SR_RCCL_LIBRARY, the path of the
 * collective library).
 * With profiling on, every kernel launch is bracketed with hipEvents on the stream it is launched on;
 * sr_get_stage_ms synchronises and returns, averaged over everything recorded since sr_set_profiling(h, 1):
 * ms[0] VAD, ms[1] MFCC (frame kernel), ms[2] DTW, ms[3] argmin = duration of ONE launch of that kernel (under
 * overlap with the other chunks' kernels), ms[4] = one whole call on the caller's stream (fork -> join).
 * sr_get_stage_launches: launches of each kernel per call (= chunks). */
int sr_set_pipeline(sr_engine *h, uint32_t streams, uint32_t min_chunk, uint32_t max_chunks); /* same knobs at run time */
/* Small launches -- one capture against the store (spch_recg, main.c:276-295), one dtw() / get_mfcc() call, a handful of
 * captures -- are latency-bound: every stage of the path is a serial chain per capture (VAD's state across frames, a wave's
 * frames, dtw's walk), and a few of them leave the GPU idle.  The engine then spends the idle width instead:
 *   VAD   fewer than 1024 captures: a workgroup of four waves per capture (k_vad_wide) instead of one wave;
 *   MFCC  fewer than 1024 work items of 64 frames: 16 or 4 frames per workgroup instead (reference front end);
 *   DTW   up to 320 000 / max_frames pairs per launch (2 689 at the firmware's 119 frames, 1 000 at 320): every pair gets
 *         its own workgroup (k_dtw_cells: all points of dtw_limit's band evaluated at once, then one lane follows the
 *         precomputed moves, and the last pair of an utterance does the slot scan), provided the band fits a workgroup's
 *         LDS beside the rows (frame cap and templates up to 400 frames; a pair whose band is larger than the LDS is walked
 *         literally by its workgroup);
 *         beyond that, up to two "rounds" of what the chip holds at once (65 536 pairs at the firmware's shapes): FOUR LANES
 *         PER PAIR (k_dtw_quad: the three candidates of a step evaluated by three lanes of a quad at the same time, minimum
 *         and move in one cross-lane reduction, both sequences staged in LDS), because the batch kernel's one-lane-per-pair
 *         walk takes the same ~126 us for 5 000 pairs as for 160 000;
 *   host  sr_recognize_batch with at most 256 KB of captures: pinned staging, results written to pinned host memory.
 * Same results bit for bit (tests run the DTW / VAD / recognition cases in every mode).  One 16 000-sample capture against
 * 80 slots: 242 us -> 64 us per spch_recg call on an otherwise idle MI355X (profiles/, latency block of bench.py).
 * The in-kernel slot scan of the one-workgroup-per-pair form counts finished pairs in per-engine counters, so it is available to
 * ONE caller stream per engine -- the first that launches it (the internal stream of the host-buffer calls counts as one);
 * small launches on any other stream of the same engine run the separate slot-scan kernel instead (same results, one more
 * launch).  Calls on one engine from several host threads at once remain forbidden as everywhere in this API.
 * mode 0 = automatic (default), 1 = never (always the batch kernels), 2 = always (the one-workgroup-per-pair DTW form whenever
 * the rectangle fits), 3 = the four-lanes-per-pair DTW form whenever the sequences fit (VAD / MFCC / host side as in mode 0),
 * whatever the launch size: for tests and measurements. */
int sr_set_small_launch(sr_engine *h, int mode);
int sr_set_profiling(sr_engine *h, int on);
int sr_get_stage_ms(sr_engine *h, float ms[5]);
int sr_get_stage_launches(sr_engine *h, uint32_t *launches_per_call);

/* Development and test hooks -- NOT part of the production surface and NOT in the product library: libsr_engine.so is
 * built without them (every name is refused with SR_ERR_BAD_ARG, sr_testing_build() == 0); the test suite and the tuning
 * sweeps load libsr_engine_testing.so, the same sources compiled with -DSR_TESTING (csrc/Makefile).
 * Process-global integer knobs, 0 = default:
 *   "dtw_u", "dtw_tie_g", "dtw_kc"   force the staged DTW kernel's workgroup geometry (read when a template store is set;
 *                                    a forced combination that does not fit the LDS / the grid is ignored)
 *   "mfcc_grid"                      workgroups of the frame kernel (read by sr_create)
 *   "dtw_debug"                      print the DTW plan (staged, per-pair and four-lane forms) when a store is set, and
 *                                    the full-DP scorer's lanes per pair at each launch
 *   "perturb_log_thr", "log_thr_from_host"   exercise / bypass the shipped log-step-table check (sr_log_table_mismatches)
 *   "mag_cheap_off"                  sr_create behaves as if its device sweep of the cheap magnitude form had failed
 *   "mag_table_off"                  the frame kernel sends QUIET frames down the MID tier (v_sqrt_f32 root, literal filterbank
 *                                    term -- exact over the QUIET range too) instead of the magnitude table; read per launch
 *   "stream_tile_frames"             frames per tile of the stream VAD scan (16..1024, a multiple of 16; default 512)
 *   "spot_chunk_cols"                end frames per kernel chunk of the word spotter (1..16383; default eight times the
 *                                    longest template, 256 at least); read per launch and by sr_spot_geometry
 *   "align_pairs"                    pairs per launch of the full-DP aligner (default: what 256 MiB of scratch hold); read
 *                                    per call and by sr_align_geometry
 *   "align_marks_global"             the aligner keeps its predecessor marks in global scratch even where they fit the LDS
 *   "chain_chunk_cols"               end frames per kernel chunk of the connected-word decoder (as "spot_chunk_cols"); read per
 *                                    call and by sr_decode_geometry; the grammar decoder reads it likewise
 *   "chain_rows"                     rows per launch group of the connected-word decoder (default: what 256 MiB of scratch
 *                                    hold); read per call and by sr_decode_geometry; the grammar decoder and sr_grammar_plan
 *                                    read it likewise
 *   "span_groups"                    groups of four spans per launch of the span scorer (default 65 535, the grid's limit;
 *                                    a launch holds one feature row's spans at least); read per call
 *   "cluster_pairs"                  (example, model) pairs per launch of the clustering score pass (default 2^20); read per call
 *   "forced_prune_off"               sr_align_transcripts_dp sweeps every end frame of every level (tail = 0: no column bound;
 *                                    the same bytes come out); read per call.  The call also reads "chain_chunk_cols" (or,
 *                                    when that is 0, "spot_chunk_cols") and "chain_rows" as the decoder does
 *   "onepass_block"                  frames per block of the one-pass decoder, clamped to 1..L (a longer block would be wrong;
 *                                    the same bytes come out of every admissible length); read per call and by
 *                                    sr_decode_onepass_geometry; the live one-pass session reads it per push, and
 *                                    sr_onepass_live_geometry reads it likewise
 *   "onepass_rows"                   rows per launch group of the one-pass decoder (default: what 256 MiB of scratch hold);
 *                                    read per call and by sr_decode_onepass_geometry
 *   "onepass_gram_prune_off"         one-pass grammar decoding keeps every item and every state (no static pruning; the same
 *                                    bytes come out); read per call and by sr_onepass_grammar_plan.  The calls also read
 *                                    "onepass_block" and "onepass_rows" as the one-pass decoder does.  The live one-pass
 *                                    grammar session reads it when a grammar is adopted (open, set_grammar: it fixes the
 *                                    column layout until the next adoption), sr_onepass_gram_live_geometry when called;
 *                                    the session reads "onepass_block" per push
 *   "live_origin"                   samples (an int64 multiple of the hop) a fresh sr_live channel behaves as having consumed
 *                                    before: received = the value, next frame = value / hop, in the device state and the host
 *                                    mirror; nothing in the push path knows of it.  Read where a channel is made fresh
 *                                    (sr_live_open, sr_live_end), which return SR_ERR_BAD_ARG and change nothing when the value
 *                                    is negative, no multiple of the hop, or the session was opened without atap_in (a noise
 *                                    head is defined from position 0).  Puts positions past 2^31 / 2^32 within a test's reach
 *   "spot_live_origin"               frames (up to 0xFFFF0000) a fresh sr_spot_live channel stands at, with nothing reachable
 *                                    before them: every saved column entry unreachable, no carry.  Read where a channel is made
 *                                    fresh (sr_spot_live_open, sr_spot_live_end; SR_ERR_BAD_ARG above 0xFFFF0000), feature and
 *                                    PCM sessions alike.  Puts columns up to the frame cap within a test's reach
 *   "multi_allow_dup"                sr_multi_create accepts one device several times; honoured only when SR_RCCL_LIBRARY
 *                                    names the collective library explicitly (1-GPU tests over the in-process RCCL double)
 *   "lds_poison_launches"            while non-zero, the LDS of every CU is overwritten (k_lds_poison, as sr_lds_poison does) on
 *                                    the launch's own stream in front of EVERY kernel launch of the library, between the
 *                                    launches of one call too.  Bits 0..31 are the seed, bits 32..33 the pattern: 0 = HIGH,
 *                                    sr_lds_poison's (seed ^ i * 2654435761) | 0x80000000 for word i, which loses every minimum
 *                                    it enters; 1 = LOW, (seed ^ i * 2654435761) & 7, a small, valid-looking cost or index that
 *                                    wins every minimum.  Other patterns and negative values return SR_ERR_BAD_ARG.  Setting
 *                                    it (to any value) empties what sr_lds_launch_points reports.  It multiplies the launches
 *                                    of a call: keep it 0 around timings, sr_get_stage_launches and sr_get_stage_ms
 * Unknown names return SR_ERR_BAD_ARG. */
int sr_dev_hook(const char *name, int64_t value);
int sr_testing_build(void);
/* Testing build only (the product library returns SR_ERR_BAD_ARG from both).
 * sr_lds_launch_points: *count = poison launches issued in front of kernel launches since "lds_poison_launches" was last set;
 * names (optional, names_cap bytes) = the distinct kernel names they stood in front of, comma-separated, in order of first use.
 * sr_lds_probe: one workgroup per CU copies the first `words` (1..4096) words of its LDS -- which it does not write -- to
 * d_out[workgroup * words + i] (device memory, CUs * words words), asynchronous on `stream`.  Each workgroup takes a CU's whole
 * LDS, so word i is the CU's word i.  The launch goes through a launch point like every other. */
int sr_lds_launch_points(uint64_t *count, char *names, uint32_t names_cap);
int sr_lds_probe(sr_engine *h, uint32_t words, uint32_t *d_out, void *stream);

/* diagnostics, host-only (touches no device): the launch geometry the staged DTW kernel would use for a store of n_templates
 * and a frame cap of max_frames: out[0] = utterances per workgroup (0 = generic kernel), out[1] = templates per workgroup (the
 * store is walked in ceil(n_templates / out[1]) chunks), out[2] = tie-threshold table entries staged in LDS, out[3] = LDS bytes
 * per workgroup, out[4] = workgroups that fit one CU's 160 KiB at gfx950's allocation granule of 1280 bytes. */
int sr_dtw_geometry(uint32_t n_templates, uint32_t max_frames, uint32_t out[5]);

/* diagnostics: the path's non-integer device functions swept directly:
 * out[3i] = (u32)(log((double)x)*100) (MFCC.C:168), out[3i+1] = (u32)sqrtf((float)x) (DTW.C:59),
 * out[3i+2] = (u32)(sqrtf((float)(s32)(x & 0x7fffffff))*10) (MFCC.C:56-58) */
int sr_math_diag(sr_engine *h, const uint32_t *in, uint32_t *out, uint32_t n);
/* diagnostics: the fused Mel filterbank term of the frame kernel -- one v_mul_hi_u32 of E << 4 with ceil(tri * 2^28 / 100) --
 * against the reference's u32 expression frq_spct[i]*tri[i]/(tri_top/10) (MFCC.C:139-161) for every weight tri in
 * [tri_lo, tri_hi) and every energy E in [0, e_max]: mismatches[tri - tri_lo] = number of E where they differ (plus 2^40 if
 * the weight recovered from the multiplier for the literal form is wrong).  The kernel takes the fused form while every E
 * of a frame is <= 2 684 354 = floor(2^28 / 100). */
int sr_mel_term_sweep(sr_engine *h, uint32_t tri_lo, uint32_t tri_hi, uint32_t e_max, uint64_t *mismatches);
/* diagnostics: the cheap magnitude form the frame kernel may use on quiet frames -- (u32)(v_sqrt_f32((float)n) * 10) -- against the
 * exact one for every n in [0, n_max]: out[0] = number of n where they differ, out[1] = the smallest such n (0xFFFFFFFF: none).
 * With bit 31 of n_max set the sweep compares what the DTW kernel's small-root form uses, floor(v_sqrt_f32((float)d)), with the
 * exact (u32)sqrtf((float)d) of DTW.C:59 for every d in [0, n_max & 0x7fffffff]. */
int sr_mag_fast_sweep(sr_engine *h, uint32_t n_max, uint64_t out[2]);
/* diagnostics: fill the whole local data share of every compute unit with a seeded pattern (asynchronous on `stream`; one
 * workgroup per CU at a time, each taking the device's full per-CU LDS).  *bytes_per_cu (optional) receives the bytes
 * each workgroup filled (163840 on MI355X).  The test suite launches it between calls: a kernel that reads LDS it has not
 * written itself gets the same values only as long as the CU's previous tenant was a workgroup of the same kernel. */
int sr_lds_poison(sr_engine *h, uint32_t seed, void *stream, uint32_t *bytes_per_cu);
/* diagnostics: per-utterance ballots of the VAD "loud" decision (VAD.C:164), 63 frames per 64-bit word, 16 words */
int sr_vad_debug_masks(sr_engine *h, const uint16_t *pcm, uint64_t pcm_stride, uint32_t buf_len, uint32_t B,
                       sr_vad_rec *vad, uint64_t *masks);

/* ------------------------------------------------------------------ reference-compatible scalar symbols
 * Exact reference signatures (u8/u16/u32/s16 = stdint fixed widths, stm32f10x.h:421-439).
 * Each one replaces the reference function cited; all run on the GPU through an implicit
 * default engine (reference constants, max_frames 119). */
typedef struct {
    uint32_t mid_val;
    uint16_t n_thl;
    uint16_t z_thl;
    uint32_t s_thl;
} atap_tag; /* VAD.H:10-16 */
typedef struct {
    uint16_t *start;
    uint16_t *end;
} valid_tag; /* VAD.H:18-22 */
#define SR_VV_FRM_MAX 119 /* MFCC.H:15-16 */
#pragma pack(push, 1)
typedef struct {
    uint16_t save_sign;
    uint16_t frm_num;
    int16_t mfcc_dat[SR_VV_FRM_MAX * 12];
} v_ftr_tag; /* MFCC.H:18-25, 2860 bytes */
#pragma pack(pop)

void noise_atap(const uint16_t *noise, uint16_t n_len, atap_tag *atap);                          /* VAD.H:24, VAD.C:22 */
void VAD(const uint16_t *vc, uint16_t buf_len, valid_tag *valid_voice, atap_tag *atap_arg);      /* VAD.H:25, VAD.C:97 */
void get_mfcc(valid_tag *valid, v_ftr_tag *v_ftr, atap_tag *atap_arg);                           /* MFCC.H:27, MFCC.C:86 */
uint32_t *fft(int16_t *dat_buf, uint16_t buf_len);                                               /* MFCC.C:27 */
void cr4_fft_1024_stm32(void *pssOUT, void *pssIN, uint16_t Nbin);                               /* MFCC.C:12, .s:219 */
uint32_t get_dis(int16_t *frm_ftr1, int16_t *frm_ftr2);                                          /* DTW.C:45 */
uint8_t dtw_limit(uint16_t x, uint16_t y);                                                       /* DTW.C:76 */
/* dtw(): models are cached by content on the device (up to 128 records, least recently used replaced); a model that is
 * new to the cache costs one store upload, an input record that is new one launch against every cached model.  Callers
 * whose model changes on every call (random pair sweeps) should use sr_dtw_batch.  Like every symbol of this section:
 * one implicit engine, file-scope state, NOT thread-safe (as the reference: DTW.C:65-68). */
uint32_t dtw(v_ftr_tag *ftr_in, v_ftr_tag *frt_mdl);                                             /* DTW.H:7, DTW.C:120 */
uint8_t *spch_recg(uint16_t *v_dat, uint32_t *mtch_dis);                                         /* main.c:249 */
void get_mean(int16_t *frm_ftr1, int16_t *frm_ftr2, int16_t *mean);                              /* DTW.C:195 */
uint32_t get_mdl(v_ftr_tag *ftr_in1, v_ftr_tag *ftr_in2, v_ftr_tag *ftr_mdl);                    /* DTW.C:217 */
/* BASELINE.json's north-star spellings; they do not exist in the reference -> aliases of get_mfcc */
void GetMfcc(valid_tag *valid, v_ftr_tag *v_ftr, atap_tag *atap_arg);
void MFCC_Comp(valid_tag *valid, v_ftr_tag *v_ftr, atap_tag *atap_arg);

/* The firmware reads its template store at a fixed flash address (Flash.H:19-20) and returns a
 * pointer into commstr[] (main.c:31,295).  The scalar spch_recg needs both handed over: */
int sr_compat_set_templates(const void *store, uint32_t n_slots, uint32_t stride_bytes);
int sr_compat_set_labels(const uint8_t *labels, uint32_t n_labels, uint32_t label_stride, uint32_t ftr_per_comm);
sr_engine *sr_compat_engine(void);
/* diagnostics: out[0] = uploads of dtw()'s model store so far, out[1] = DTW launches, out[2] = models cached */
void sr_compat_dtw_stats(uint32_t out[3]);

#ifdef __cplusplus
}
#endif
#endif /* SR_ENGINE_H */
