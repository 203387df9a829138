// k_mfcc.hip -- get_mfcc (MFCC.C:86-191) incl. fft (MFCC.C:27-62) and cr4_fft_1024_stm32 (.s:95-281): the reference front end, one wave per frame.
// gfx950 (MI355X, CDNA4) only; wave = 64 lanes; no MFMA (the path has no dense contraction), integer VALU + LDS.
// Every kernel reproduces the reference's integer arithmetic bit for bit; cited lines are relative to the reference tree.
#include "sr_fft_dev.h"

#include <type_traits>

namespace sr {

// ------------------------------------------------------------------------------------------------
// k_mfcc
// ------------------------------------------------------------------------------------------------
constexpr int kMfccWaves = 4;       // waves per workgroup
// consecutive frames one wave turns into MFCCs per work item: 16 in the batch form (the lane constants and tables a workgroup
// sets up are amortised over 64 frames); 4 and 1 for launches that would leave the chip underfilled (a wave's frames are a
// serial chain of ~1.5 us each: one capture = 110 frames is 28 workgroups of 4 frames instead of 2 of 64 -- 7 us instead of
// 28-33 -- and 256 captures are 2 048 workgroups of 16 frames instead of 512 of 64)
constexpr int kFramesPerWave = 16, kFramesPerWaveMid = 4, kFramesPerWaveSmall = 1;
// bins per lane whose QUIET-tier magnitude comes from the table mag_q (sr_tables.h) instead of v_sqrt_f32: 8 = all of them,
// 4 = the `+ 256` half only, 0 = none.  A knob per form: the batch form hides the gathers behind the other waves' arithmetic;
// a one-frame launch would wait for a cold table, so the underfilled-launch forms keep the root (RESULTS.md, round 7).
#ifndef SR_MAG_TAB_BINS
#define SR_MAG_TAB_BINS 8
#endif
constexpr int mfcc_tab_bins(int fpw) { return fpw == kFramesPerWave ? SR_MAG_TAB_BINS : 0; }
static_assert(SR_MAG_TAB_BINS == 0 || SR_MAG_TAB_BINS == 4 || SR_MAG_TAB_BINS == 8, "table bins per lane");
// switches of the batch form's two-frame loop (RESULTS.md, round 8; the defaults are the variant that was kept): SR_MFCC_PIPE 0 =
// the serial loop of round 7; SR_MFCC_PIPE_PEEL 0 = one loop with its first / last-frame tests as scalar branches;
// SR_MFCC_PIPE_VMCNT 0 = every wait drains the counter, 3 = the steady-state wait leaves the three younger sample loads in
// flight (peeled form only: elsewhere they are not behind the gathers on every path)
#ifndef SR_MFCC_PIPE
#define SR_MFCC_PIPE 1
#endif
#ifndef SR_MFCC_PIPE_PEEL
#define SR_MFCC_PIPE_PEEL 1
#endif
#ifndef SR_MFCC_PIPE_VMCNT
#define SR_MFCC_PIPE_VMCNT (SR_MFCC_PIPE_PEEL ? 3 : 0)
#endif
static_assert(SR_MFCC_PIPE_VMCNT == 0 || (SR_MFCC_PIPE_VMCNT == 3 && SR_MFCC_PIPE_PEEL), "younger loads counted by the wait");
constexpr bool mfcc_pipelined(int fpw) { return SR_MFCC_PIPE && mfcc_tab_bins(fpw) == 8; }
// switches of round 11, which cut the cycles a frame keeps the CU's LDS pipe busy (RESULTS.md, round 11):
// SR_MFCC_TM_REGS 1 = the batch form keeps the QUIET tier's sixteen filterbank multipliers in VGPRs, not in s_tm;
// the other half of that round is mel_prefix_store below.  Kept together: alone they are worth +0.7 % and -0.5 % of the step,
// the two -2.0 %.
#ifndef SR_MFCC_TM_REGS
#define SR_MFCC_TM_REGS 1
#endif
#ifdef SR_INJECT_LDS_RACE  // (the injected race is the late fill of s_tm: that build keeps the multipliers there)
#undef SR_MFCC_TM_REGS
#define SR_MFCC_TM_REGS 0
#endif
constexpr bool mfcc_tm_regs(int fpw) { return SR_MFCC_TM_REGS && mfcc_pipelined(fpw); }
// per-wave LDS: exchange/scratch words + windowed frame + filterbank outputs of the wave's frames
// rows of the filterbank outputs and of the DCT tables are kMelPad = 25 words apart: in the DCT the lanes of a wave read
// 6 different frames x 12 different coefficients rows at the same column, and a stride of 24 folds those onto 4 banks
constexpr int kMelPad = kMel + 1;
// the windowed frame aliases the exchange area; the last 64 words hold the odd filters' lane offsets
// Scratch order of the filterbank stage.  Both of its stores are lane-contiguous (ds_write_addtid_b32, 2 cycles of the CU's
// store path each; a 4-byte store with an address register takes 4, a 16-byte one 13):
//   energies  (round 12) bin b at word energy_word(b) of sr_fft_layout.h -- mel_energy_store below
//   prefixes  (round 11) the in-lane prefix P[j] of bin j = 8 l + k at word 64 k + l of its poly-line's half.  The look-up's
//             addresses are lane constants in any order; in this one its 24 lanes meet on a bank two at a time at most.
__device__ __forceinline__ constexpr int mel_prefix_word(int j) { return 64 * (j & 7) + (j >> 3); }
// The stores: lane l writes pe[k] to word 64 k + l and po[k] to word kBins + 64 k + l of the area at LDS byte address `base`
// (wave-uniform).  ds_write_addtid_b32's address is M0 + offset + 4 * lane: no address VGPR goes to the LDS.  M0 is set in
// the same statement (one wait state before an add-TID instruction reads it) and named as clobbered.  The compiler treats M0
// as reserved and says so about the clobber; it has no use of M0 of its own in this kernel -- no LDS bounds on gfx9+, no
// movrel, no message, no LDS-DMA: `m0` occurs in the kernel's assembly in the three add-TID statements only (this one,
// mel_energy_store, fft_exchange_tid of sr_fft_dev.h).  Look again after adding any
// of those.  The wave's LDS operations complete in issue order, so a wait the compiler counts for its own reads, which does
// not know of these stores, can only come out stricter.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void mel_prefix_store(uint32_t base, const uint32_t (&pe)[8], const uint32_t (&po)[8])
{
    static_assert(kBins == 512, "the offsets below are written out for two halves of 512 words");
    asm volatile("s_mov_b32 m0, %16\n\ts_nop 0\n\t"
                 "ds_write_addtid_b32 %0\n\tds_write_addtid_b32 %1 offset:256\n\tds_write_addtid_b32 %2 offset:512\n\t"
                 "ds_write_addtid_b32 %3 offset:768\n\tds_write_addtid_b32 %4 offset:1024\n\tds_write_addtid_b32 %5 offset:1280\n\t"
                 "ds_write_addtid_b32 %6 offset:1536\n\tds_write_addtid_b32 %7 offset:1792\n\t"
                 "ds_write_addtid_b32 %8 offset:2048\n\tds_write_addtid_b32 %9 offset:2304\n\tds_write_addtid_b32 %10 offset:2560\n\t"
                 "ds_write_addtid_b32 %11 offset:2816\n\tds_write_addtid_b32 %12 offset:3072\n\tds_write_addtid_b32 %13 offset:3328\n\t"
                 "ds_write_addtid_b32 %14 offset:3584\n\tds_write_addtid_b32 %15 offset:3840"
                 :
                 : "v"(pe[0]), "v"(pe[1]), "v"(pe[2]), "v"(pe[3]), "v"(pe[4]), "v"(pe[5]), "v"(pe[6]), "v"(pe[7]), "v"(po[0]),
                   "v"(po[1]), "v"(po[2]), "v"(po[3]), "v"(po[4]), "v"(po[5]), "v"(po[6]), "v"(po[7]), "s"(base)
                 : "m0", "memory");
}
// The energies, stored the same way (sr_fft_layout.h): magnitude lane l' holds en[2 e3 + half] of bin l' + 64 e3 + 256 half,
// plane q = e3 + 4 half lies at word energy_plane(q) + l'.  Filter lane l then reads its bins 8 l .. 8 l + 7 as two 16-byte
// words from energy_read_base(l) on; the plane bases keep those reads conflict-free.
__device__ __forceinline__ void mel_energy_store(uint32_t base, const uint32_t (&en)[8])
{
    static_assert(4 * energy_plane(1) == 256 && 4 * energy_plane(2) == 528 && 4 * energy_plane(3) == 784 && 4 * energy_plane(4) == 1040 &&
                      4 * energy_plane(5) == 1296 && 4 * energy_plane(6) == 1568 && 4 * energy_plane(7) == 1824 && kBins == kEnergyBins,
                  "the offsets below are written out for these plane bases");
    asm volatile("s_mov_b32 m0, %8\n\ts_nop 0\n\t"
                 "ds_write_addtid_b32 %0\n\tds_write_addtid_b32 %1 offset:256\n\tds_write_addtid_b32 %2 offset:528\n\t"
                 "ds_write_addtid_b32 %3 offset:784\n\tds_write_addtid_b32 %4 offset:1040\n\tds_write_addtid_b32 %5 offset:1296\n\t"
                 "ds_write_addtid_b32 %6 offset:1568\n\tds_write_addtid_b32 %7 offset:1824"
                 :
                 : "v"(en[0]), "v"(en[2]), "v"(en[4]), "v"(en[6]), "v"(en[1]), "v"(en[3]), "v"(en[5]), "v"(en[7]), "s"(base)
                 : "m0", "memory");
}
#pragma clang diagnostic pop
constexpr int mfcc_wave_lds_words(int fpw) { return kXchgWords + fpw * kMelPad + 64; }

// the kernel's argument block: the block every frame kernel takes (MfccArgs, or MfccFeatArgs<kind>) + the magnitude table
template <typename Base>
struct MfccTabArgs : Base {
    const uint16_t *mag_q;
    uint32_t mag_table_off;
};
template <typename Base>
constexpr int mfcc_feat_kind<MfccTabArgs<Base>> = mfcc_feat_kind<Base>;
template <typename Base>
static MfccTabArgs<Base> mfcc_tab_args(const Base &b, const MfccMagTab &tab)
{
    MfccTabArgs<Base> r;
    static_cast<Base &>(r) = b;
    r.mag_q = tab.mag_q;
    r.mag_table_off = tab.mag_table_off;
    return r;
}

// Args = MfccTabArgs<MfccArgs>: the frame kernel.  Args = MfccTabArgs<MfccFeatArgs<kind>>: the same kernel, which also stores
// one intermediate value per frame into a.feat[b][max_frames][width] at the point where it exists
// (sr_frame_features_batch_dev).  Every feature store sits under `if constexpr`: the frame kernel carries none of them.
template <int kFPW, typename Args = MfccTabArgs<MfccArgs>>
__global__ void __launch_bounds__(64 * kMfccWaves, 4) k_mfcc(const Args a)
{
    constexpr int kFeat = mfcc_feat_kind<Args>;
    constexpr uint32_t kFeatW = (kFeat == SR_FEAT_FFT || kFeat == SR_FEAT_MAG) ? kBins : kMel;  // feature words per frame
    constexpr int kWaveLdsWords = mfcc_wave_lds_words(kFPW);
    constexpr int kTabBins = mfcc_tab_bins(kFPW);
    constexpr bool kPipe = mfcc_pipelined(kFPW);
    constexpr bool kTmRegs = mfcc_tm_regs(kFPW);
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ uint32_t s_dctM[kCoef * kMelPad];
    __shared__ int s_dctS[kCoef * kMelPad];  // 32-bit: read with the wide LDS loads, no byte extraction
    __shared__ u32x4 s_tw3[kTw3Row * 4], s_tw5[8 * 64];  // pass-3 (per d0) / pass-5 (per lane) coefficients, shared by the waves
    __shared__ u32x4 s_tm[4 * 64];                 // filterbank multipliers of the lane's eight bins (both poly-lines)
    // (the wave index as a SCALAR: frame counts, loop bounds and the frame's sample pointer then live on the scalar unit --
    // left in a VGPR they cost three vector instructions per frame for the next frame's load address and loop test)
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *buf = smem + w * kWaveLdsWords;
    uint32_t *xw = buf;  // windowed frame, one word per sample: consumed by the pass-1 gather before the exchange overwrites it
    uint32_t *powb = buf + kXchgWords, *moff = powb + kFPW * kMelPad;
    // LDS byte address of buf, wave-uniform: the base of the prefix stores
    const uint32_t buf_lds = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint32_t *)buf;
    (void)buf_lds;

    // DCT term (MFCC.C:179): (s32)pow * dct / 100, truncated toward zero, with 0 <= pow <= 2218 (= (u32)(ln(2^32)*100))
    // and |dct| <= 128.  floor(pow*|c|/100) == (pow * M_c) >> 18 with M_c = ceil(|c| * 2^18 / 100) for every such pair
    // (the rounding excess pow*eps/2^18 stays below 1/100 because 100*pow < 2^18); the log stage stores pow << 14 so
    // the quotient is one v_mul_hi_u32, and the sign of c is applied by the accumulating 24-bit multiply.
    for (int i = threadIdx.x; i < kCoef * kMel; i += blockDim.x) {
        const int c = a.t.dct[i], o = (i / kMel) * kMelPad + i % kMel;
        s_dctM[o] = (uint32_t)(((c < 0 ? -c : c) * 262144 + 99) / 100);
        s_dctS[o] = (c > 0) - (c < 0);
    }
    __syncthreads();

    // ---- lane-invariant constants --------------------------------------------------------------
    LaneTw tw;
    load_lane_tw(a.t, lane, lane >> 4, tw);  // front lane = d3 + 4 d4 + 16 d0 (sr_fft_layout.h)
    real_leg_tw(tw);  // pass 2 multiplies duplicated real legs (sr_fft_dev.h window_store)
    if (w == 0 && (lane & 15) == 0) {  // the four pass-3 rows, from lanes with d0 = 0..3
        const uint32_t *f = &tw.s3[0][0][0];
        const int d0 = lane >> 4;
#pragma unroll
        for (int c = 0; c < 8; c++) s_tw3[d0 * kTw3Row + c] = u32x4{f[4 * c], f[4 * c + 1], f[4 * c + 2], f[4 * c + 3]};
    }
    if (w == 1 % kMfccWaves) store_tw32(s_tw5, lane, tw.s5);
    // triangle weights of bins 8*lane .. 8*lane+7 of both poly-lines as fused multipliers ceil(tri * 2^28 / 100)
    // (sr_tables.h mel_fused_multiplier), parked in LDS as lane-contiguous 16-byte chunks like the pass-5 coefficients
    // (chunk c of lane l at s_tm[64 c + l]: even 0-3, even 4-7, odd 0-3, odd 4-7; conflict-free ds_read_b128, and LDS
    // instructions do not take VALU issue slots): held in 16 VGPRs for the whole kernel they pushed it past 128
    // (-DSR_INJECT_LDS_RACE=1 / =2, fault injection for the suite's race-class tests -- profiles/experiments/ab_build.sh race2 . -DSR_INJECT_LDS_RACE=2:
    // the fill is moved BEHIND the barrier, which is the defect round 5's soak found; level 2 also delays the late writer, which
    // opens the window on every workgroup instead of once in thousands of calls; what the tests make of both: RESULTS.md, round 6)
    // (round 11: the batch form has the registers for them again since round 9 took it from 128 to 112 -- kTmRegs; four
    // ds_read_b128 per frame and this table leave its LDS budget.  The forms for underfilled launches keep the table.)
    u32x4 tm_r[4];
    if constexpr (kTmRegs) {
#pragma unroll
        for (int c = 0; c < 2; c++) {
            tm_r[c] = *(const u32x4 *)(a.t.tri_even_m + 8 * lane + 4 * c);
            tm_r[c + 2] = *(const u32x4 *)(a.t.tri_odd_m + 8 * lane + 4 * c);
        }
    }
#ifndef SR_INJECT_LDS_RACE
    if (!kTmRegs && w == 2 % kMfccWaves) {
#pragma unroll
        for (int c = 0; c < 2; c++) {
            s_tm[64 * c + lane] = *(const u32x4 *)(a.t.tri_even_m + 8 * lane + 4 * c);
            s_tm[64 * (c + 2) + lane] = *(const u32x4 *)(a.t.tri_odd_m + 8 * lane + 4 * c);
        }
    }
#endif
    __syncthreads();  // every table above is written by ONE wave and read by all of them: nothing shared is written below this line
#ifdef SR_INJECT_LDS_RACE
    if (w == 2 % kMfccWaves) {
#if SR_INJECT_LDS_RACE >= 2  // level 2: the late writer is also held back ~3.4 us (what a slow table load does to it once in thousands of calls)
        __builtin_amdgcn_s_sleep(127);
#endif
#pragma unroll
        for (int c = 0; c < 2; c++) {
            s_tm[64 * c + lane] = *(const u32x4 *)(a.t.tri_even_m + 8 * lane + 4 * c);
            s_tm[64 * (c + 2) + lane] = *(const u32x4 *)(a.t.tri_odd_m + 8 * lane + 4 * c);
        }
    }
#endif
    int hamm_m[3];  // window weights of the lane's three samples as fused multipliers (sr_tables.h hamm_fused_multiplier)
#pragma unroll
    for (int k = 0; k < 3; k++) hamm_m[k] = (lane + 64 * k < kFrameLen) ? hamm_fused_multiplier(a.t.hamm[lane + 64 * k]) : 0;
    // filter h < 24 owned by lane h: bins [lo, hi) of poly-line (h & 1)  (MFCC.C:136-162)
    // prefix P[j] of bin j sits at word mel_prefix_word(j) of its poly-line's half, the lane offsets X[l] behind them: the
    // addresses of P[hi - 1] / P[lo - 1] are lane constants
    int f_lo = 0, p_hi = 0, p_lo = 0, x_hi = 0, x_lo = 0;
    if (lane < kMel) {
        const int h = lane;
        f_lo = (h == 0) ? 0 : (int)a.t.tri_cen[h - 1];
        const int f_hi = (h == kMel - 1) ? kBins : (int)a.t.tri_cen[h + 1];
        const int ih = f_hi - 1, il = f_lo ? f_lo - 1 : 0, half = (h & 1) ? kBins : 0;
        // X holds INCLUSIVE lane sums: the bins below lane l's first bin sum to X[l - 1]; every edge looked up lies in lane >= 1
        // (tri_cen[0] - 1 = 10), clamped so that an unused entry stays inside the array
        p_hi = half + mel_prefix_word(ih), x_hi = (ih >> 3) > 0 ? (ih >> 3) - 1 : 0;
        p_lo = half + mel_prefix_word(il), x_lo = (il >> 3) > 0 ? (il >> 3) - 1 : 0;
    }
    // The magnitude table as a structured buffer of exactly its size (stride 2, num_records in elements): the gathers index
    // it with n itself (idxen) -- no address arithmetic on the VALU -- and an n past the end could only load 0, never fault
    // (none occurs: only QUIET frames, every n <= kMagSmallMax, gather).  No builtin emits the indexed form, so the loads are
    // inline assembly.
    const uint64_t mag_p = (uint64_t)a.mag_q;
    const u32x4 mag_rs = {(uint32_t)mag_p, (uint32_t)(mag_p >> 32) | (2u << 16), kMagTabEntries, 0x00027000u};
    const uint32_t tw_off = 32u * (uint32_t)lane;  // byte offset of the lane's eight raw filterbank weights (LOUD / MID tiers)
    // the energies of the filter lane's bins 8 lane .. 8 lane + 7: two 16-byte words of the energies image (sr_fft_layout.h)
    const int c0 = energy_read_base(lane), c1 = c0 + 4;

    // the per-utterance record of the NEXT work item is fetched while the current one is processed
    uint32_t item = blockIdx.x;
    uint32_t nx_nfrm = 0;
    int nx_mid = 0, nx_seg0 = 0;
    if (item < a.n_items) {
        const sr_vad_rec *rec = a.vad + item / a.tiles;
        nx_nfrm = rec->frm_num;
        nx_mid = (int)rec->atap.mid_val;
        nx_seg0 = rec->seg[0];
    }
    for (; item < a.n_items; item += gridDim.x) {
        const uint32_t b = item / a.tiles, tile = item - b * a.tiles;
        const uint32_t nfrm = nx_nfrm;
        const int mid = nx_mid, seg0 = nx_seg0;
        if (item + gridDim.x < a.n_items) {
            const sr_vad_rec *rec = a.vad + (item + gridDim.x) / a.tiles;
            nx_nfrm = rec->frm_num;
            nx_mid = (int)rec->atap.mid_val;
            nx_seg0 = rec->seg[0];
        }
        const uint16_t *row = a.pcm + (uint64_t)b * a.pcm_stride;
        int16_t *out = a.mfcc + (uint64_t)b * a.max_frames * kCoef;
        const uint32_t f0 = tile * (kMfccWaves * kFPW) + w * kFPW;
        uint32_t *frow = nullptr;  // feature rows of utterance b
        if constexpr (kFeat != 0) frow = a.feat + (uint64_t)b * a.max_frames * kFeatW;
        uint32_t nf = 0;  // frames this wave really has
        if (f0 < nfrm) nf = (nfrm - f0 < (uint32_t)kFPW) ? nfrm - f0 : (uint32_t)kFPW;

        // samples of frame fi+1 are requested while frame fi is transformed
        // one 2-byte-aligned dword per sample: x[i-1] in the low half, x[i] in the high half
        uint32_t s_pp[3] = {0, 0, 0};
        if (nf) {
            const uint16_t *x = row + seg0 + (int)kHop * (int)f0;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int i = lane + 64 * k;
                if (i < kFrameLen) s_pp[k] = *(const u32_align2 *)(x + i - 1);
            }
        }
        // the in-lane prefixes of the lane's eight bins, both poly-lines (mel_prefix_word; every lane has read its energies: the
        // wave's LDS operations complete in order)
        auto store_prefixes = [&](const uint32_t (&pe)[8], const uint32_t (&po)[8]) { mel_prefix_store(buf_lds, pe, po); };
        // the squares of the lane's eight magnitudes, en[2 e3 + half] of bin lane + 64 e3 + 256 half, into the energies image
        auto store_energies = [&](const uint32_t (&en)[8]) { mel_energy_store(buf_lds, en); };
        auto exchange = [&](const uint32_t (&v)[4][4], uint32_t (&u)[4][4]) { fft_exchange_tid(buf, buf_lds, lane, v, u); };
        if constexpr (!kPipe)  // the forms without the table (and the feature variants of those): one frame at a time
        for (uint32_t fi = 0; fi < nf; fi++) {
            // ---- pre-emphasis + Hamming (MFCC.C:115-124); x[-1] is the sample before the frame
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int i = lane + 64 * k;
                // stored as pass 2 consumes them (sr_fft_dev.h window_store): samples 0..63 (k = 0) are only ever its A legs, the others
                // its real B and C legs
                if (i < kFrameLen) k == 0 ? window_store<0>(xw, i, s_pp[k], mid, hamm_m[k]) : window_store<1>(xw, i, s_pp[k], mid, hamm_m[k]);
            }
            if (fi + 1 < nf) {
                const uint16_t *x = row + seg0 + (int)kHop * (int)(f0 + fi + 1);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const int i = lane + 64 * k;
                    if (i < kFrameLen) s_pp[k] = *(const u32_align2 *)(x + i - 1);
                }
            }
            wave_sync();
            // ---- FFT passes 1-3 in registers, exchange, passes 4-5 in registers
            uint32_t v[4][4], u[4][4];
            fft_front_real160(xw, lane, tw, s_tw3, v);
            exchange(v, u);
#pragma unroll
            for (int e4 = 0; e4 < 4; e4++) fft_pass4_dbl(u, e4, tw);
            // pass 5: only x[j] and x[j+q] (bins < 512) are consumed (MFCC.C:49)
            wave_sync();
            uint32_t k5[4][4][2];
            load_tw32(s_tw5, lane, k5);
            uint32_t nn[8];  // re^2 + im^2 of the lane's eight bins (one v_dot2_i32_i16 each, from the stored 16-bit halves)
#pragma unroll
            for (int e3 = 0; e3 < 4; e3++) {
                bfly_pk_dbl<true, false, 0>(u[e3][0], u[e3][1], u[e3][2], u[e3][3], k5[e3][0][0], k5[e3][0][1], k5[e3][1][0],
                                            k5[e3][1][1], k5[e3][2][0], k5[e3][2][1], k5[e3][3][0], k5[e3][3][1]);
                if constexpr (kFeat == SR_FEAT_FFT) {  // x[j], x[j + 256] as the asm stores them: bins lane + 64 e3 (+ 256)
                    uint32_t *fr = frow + (f0 + fi) * kFeatW + lane + 64 * e3;
                    fr[0] = u[e3][0];
                    fr[256] = u[e3][1];
                }
                nn[2 * e3] = (uint32_t)sdot2z(u[e3][0], u[e3][0]);
                nn[2 * e3 + 1] = (uint32_t)sdot2z(u[e3][1], u[e3][1]);
            }
            // ---- |X|*10 and energy (MFCC.C:49-60, 128-133), three tiers by the largest re^2 + im^2 of the frame, decided for the whole
            // wave so that every branch is uniform:
            //   QUIET  (<= kMagSmallMax = 26 843, i.e. |X|*10 <= 1638 and E <= kMelFusedMaxE): magnitude from the table mag_q (batch form;
            //                                     cheap magnitude in the forms without it, mfcc_tab_bins) + fused filterbank term
            //   MID    (<= a.mag_cheap_max = 70 171 on gfx950, |X|*10 <= 2648):              cheap magnitude + literal filterbank term
            //   LOUD   (anything else):                                                     exact magnitude + literal filterbank term
            // cheap magnitude = (u32)(v_sqrt_f32 * 10): equal to the exact form for every n <= 70 171 on gfx950 -- a property of this
            // chip's v_sqrt_f32, so sr_create sweeps the whole range on the device it runs on and passes 0 if it does not hold
            // (sr_engine.cpp, sr_mag_fast_sweep); 4.5 issue slots per bin against 6.5 for the exactly corrected root (all 2^32 inputs
            // certified, sr_dev.h sqrt_rn_int).  At the benchmark's amplitudes 97-99 % of the frames are QUIET; at SURVEY 8(d)'s
            // (gain 2.4) 29 % QUIET / 47 % MID / 24 % LOUD; near-clipping captures are LOUD (profiles/experiments/RESULTS.md).
            const uint32_t nmax = max(max(max(max(nn[0], nn[1]), nn[2]), max(max(nn[3], nn[4]), nn[5])), max(nn[6], nn[7]));
#ifdef SR_TESTING  // development hook "mag_table_off": QUIET frames take the MID tier, independent arithmetic that is exact there too
            const bool quiet = __builtin_expect(__builtin_amdgcn_ballot_w64(nmax > kMagSmallMax) == 0 && !a.mag_table_off, 1);
#else
            const bool quiet = __builtin_expect(__builtin_amdgcn_ballot_w64(nmax > kMagSmallMax) == 0, 1);
#endif
            // the literal filterbank form multiplies by the weights themselves: requested from the (cache-resident) table now, they
            // arrive behind the magnitude stage.  Kept out of LDS (the workgroup's share is full at four workgroups per CU) and out
            // of the quiet path's registers.
            u32x4 tw_e[2], tw_o[2];
            bool cheap = true;
            if (!quiet) {
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    tw_e[c] = *(const u32x4 *)((const char *)a.t.tri_even32 + tw_off + 16 * c);
                    tw_o[c] = *(const u32x4 *)((const char *)a.t.tri_odd32 + tw_off + 16 * c);
                }
                cheap = __builtin_amdgcn_ballot_w64(nmax > a.mag_cheap_max) == 0;
            } else {
                // never read on this path: "defined" by an empty asm so that the quiet frame does not pay 16 register clears
                asm volatile("" : "=v"(tw_e[0]), "=v"(tw_e[1]), "=v"(tw_o[0]), "=v"(tw_o[1]));
            }
            // energies go to the wave's scratch in the order the filterbank reads them in (store_energies)
            uint32_t en[8];
            if (kTabBins > 0 && quiet) {
                // QUIET-tier magnitudes << 2 from the table: eight gathers on the vector-memory path, which take no VALU issue
                // slot -- the SIMD's other waves issue under them.  Requested only once the frame is known to be QUIET: gathered
                // inside pass 5, before the decision, they cost the frames of the other tiers (scattered indices, nothing saved)
                // more than the earlier start bought here (RESULTS.md, round 7).  (nn come from v_dot2; the nmax reduction and
                // the branch between them and this point are more than the wait states a vector-memory read of them needs.)
                uint32_t tq[8];
#pragma unroll
                for (int e3 = 0; e3 < 4; e3++) {
                    if constexpr (kTabBins == 8)
                        asm volatile("buffer_load_ushort %0, %1, %2, 0 idxen" : "=v"(tq[2 * e3]) : "v"(nn[2 * e3]), "s"(mag_rs));
                    asm volatile("buffer_load_ushort %0, %1, %2, 0 idxen" : "=v"(tq[2 * e3 + 1]) : "v"(nn[2 * e3 + 1]), "s"(mag_rs));
                }
                uint32_t q0s[4];  // kTabBins = 4: the bins the table does not serve keep the root, shifted to match, under the gathers
                if constexpr (kTabBins == 4) {
#pragma unroll
                    for (int e3 = 0; e3 < 4; e3++) q0s[e3] = cvt_u32(__builtin_amdgcn_sqrtf((float)(int)nn[2 * e3]) * 10.0f) << 2;
                }
                // the compiler does not count loads issued from inline assembly: the wait is written out, with the values tied in
                if constexpr (kTabBins == 8)
                    asm volatile("s_waitcnt vmcnt(0)" : "+v"(tq[0]), "+v"(tq[1]), "+v"(tq[2]), "+v"(tq[3]), "+v"(tq[4]), "+v"(tq[5]), "+v"(tq[6]), "+v"(tq[7]));
                else
                    asm volatile("s_waitcnt vmcnt(0)" : "+v"(tq[1]), "+v"(tq[3]), "+v"(tq[5]), "+v"(tq[7]));
                // the entries are |X|*10 << 2: their squares are E << 4, the operand of the fused filterbank term
#pragma unroll
                for (int e3 = 0; e3 < 4; e3++) {
                    uint32_t q0, q1 = tq[2 * e3 + 1];
                    if constexpr (kTabBins == 8) q0 = tq[2 * e3];
                    else q0 = q0s[e3];
                    if constexpr (kFeat == SR_FEAT_MAG) {  // the QUIET tier's magnitudes
                        uint32_t *fr = frow + (f0 + fi) * kFeatW + lane + 64 * e3;
                        fr[0] = q0 >> 2;
                        fr[256] = q1 >> 2;
                    }
                    en[2 * e3] = umul24(q0, q0);
                    en[2 * e3 + 1] = umul24(q1, q1);
                }
            } else if (cheap) {
#pragma unroll
                for (int e3 = 0; e3 < 4; e3++) {
                    const f32x2 m = f32x2{__builtin_amdgcn_sqrtf((float)(int)nn[2 * e3]), __builtin_amdgcn_sqrtf((float)(int)nn[2 * e3 + 1])} *
                                    f32x2{10.0f, 10.0f};
                    const uint32_t m0 = cvt_u32(m.x), m1 = cvt_u32(m.y);
                    if constexpr (kFeat == SR_FEAT_MAG) {  // the MID tier's magnitudes (and the QUIET tier's in a form without the table)
                        uint32_t *fr = frow + (f0 + fi) * kFeatW + lane + 64 * e3;
                        fr[0] = m0;
                        fr[256] = m1;
                    }
                    en[2 * e3] = umul24(m0, m0);
                    en[2 * e3 + 1] = umul24(m1, m1);
                }
            } else {
#pragma unroll
                for (int e3 = 0; e3 < 4; e3++) {
                    // both bins' roots and the x10 in packed f32 operations (plain IEEE multiplies and fused multiply-adds, see sqrt_rn_int)
                    const f32x2 m = sqrt_rn_int2(f32x2{(float)(int)nn[2 * e3], (float)(int)nn[2 * e3 + 1]}) * f32x2{10.0f, 10.0f};
                    const uint32_t m0 = cvt_u32(m.x), m1 = cvt_u32(m.y);  // < 2^19
                    if constexpr (kFeat == SR_FEAT_MAG) {  // the LOUD tier's
                        uint32_t *fr = frow + (f0 + fi) * kFeatW + lane + 64 * e3;
                        fr[0] = m0;
                        fr[256] = m1;
                    }
                    en[2 * e3] = umul24(m0, m0);
                    en[2 * e3 + 1] = umul24(m1, m1);
                }
            }
            store_energies(en);
            wave_sync();
            // ---- Mel filterbank as prefix sums over bins (each term /100 before summing, u32 wrap)
            uint32_t pe[8], po[8], xe, xo;
            {
                const uint4 q0 = *(const uint4 *)(buf + c0), q1 = *(const uint4 *)(buf + c1);
                const uint32_t e[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                uint32_t se = 0, so = 0;
                // E*tri/100 (MFCC.C:139-161): in a quiet frame (every E <= kMelFusedMaxE, see above) a term is ONE v_mul_hi_u32 of
                // E << 4 with the per-bin multiplier (the shift shared by both poly-lines): 5 instructions per bin instead of 8
                // (mul_lo, mul_hi, shift, add per term).  A louder frame takes the literal u32-wrapping form.
                if (quiet) {
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        const u32x4 me = s_tm[64 * c + lane], mo = s_tm[64 * (c + 2) + lane];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const uint32_t es = kTabBins > 0 ? e[4 * c + k] : e[4 * c + k] << 4;  // (the table's squares are shifted already)
                            se += mel_term_fused(es, me[k]);
                            so += mel_term_fused(es, mo[k]);
                            pe[4 * c + k] = se;
                            po[4 * c + k] = so;
                        }
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 2; c++) {
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            se += e[4 * c + k] * tw_e[c][k] / 100u;
                            so += e[4 * c + k] * tw_o[c][k] / 100u;
                            pe[4 * c + k] = se;
                            po[4 * c + k] = so;
                        }
                    }
                }
                xe = wave_scan_incl(se);  // sum over the bins of the lanes up to and including this one: a filter lane reads the
                xo = wave_scan_incl(so);  // entry of the lane BELOW its bin's (never lane 0: the first filter edge is bin 10)
            }
            // (no ordering point is needed here: every lane's energy reads above were issued before the stores below, the wave's LDS
            // operations complete in order, and nobody reads the stored words before the next wave_sync)
            // in-lane prefixes and the per-lane offsets are stored separately: the 24 filter lanes add them on lookup
            // (2 adds) instead of every lane adding its offset to 16 prefixes
            store_prefixes(pe, po);
            buf[2 * kBins + lane] = xe;
            moff[lane] = xo;
            wave_sync();
            if (lane < kMel) {
                const uint32_t *X = (lane & 1) ? moff : buf + 2 * kBins;
                const uint32_t hi = buf[p_hi] + X[x_hi], lo = f_lo ? buf[p_lo] + X[x_lo] : 0u;
                powb[fi * kMelPad + lane] = hi - lo;
                if constexpr (kFeat == SR_FEAT_MEL) frow[(f0 + fi) * kFeatW + lane] = hi - lo;
            }
            wave_sync();
        } else {
            // ---- the batch form: two frames in flight per wave (round 8).  Frame fi's BACK END (energies, filterbank, look-up)
            // runs after frame fi+1's FFT front, so that a QUIET frame's eight gathers have a whole FFT front -- window, ten LDS
            // reads, passes 2-3 -- to come back under, instead of stopping the wave once per frame.  Order of one iteration:
            //   front(fi): xw -> v[][] in registers (buf is free from here) ; back end of fi-1 through buf -> powb[fi-1] ;
            //   exchange, passes 4-5, nn[] of fi ; window(fi+1) -> xw (u[][] is in registers: buf is free again) ;
            //   tier of fi: QUIET issues the gathers, MID / LOUD compute ; request the samples of fi+2.
            // Carried over the iteration boundary: mq[8] (|X|*10 of the lane's bins; << 2 from the table in a QUIET frame, plain
            // otherwise -- umul24(q, q) serves both, as in the serial loop) and the wave-uniform flag pq (that frame was QUIET).
            // vmcnt is ONE in-order counter and the compiler does not count the gathers: any wait it writes for an OLDER load
            // between the gathers and the back end's explicit wait would drain them there.  Hence window(fi+1), the consumer of the
            // prefetched samples, sits BEFORE the gathers and the next request AFTER them; a feature store never sits in between.
            // Found in the disassembly of k_mfcc<16> (gfx950, -O3): on the QUIET path from the last gather to the explicit wait
            // there are the three sample loads, the loop branch and the whole FFT front -- no s_waitcnt that names vmcnt, and no
            // instruction that reads one of the eight gather registers (the compiler keeps mq[] in the same VGPRs on all paths;
            // a copy there would read a register still in flight: look again after any change to this loop).
            uint32_t mq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            bool pq = true;
            auto window = [&]() {  // pre-emphasis + Hamming (MFCC.C:115-124) of the requested samples, as in the serial loop below
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const int i = lane + 64 * k;
                    if (i < kFrameLen) k == 0 ? window_store<0>(xw, i, s_pp[k], mid, hamm_m[k]) : window_store<1>(xw, i, s_pp[k], mid, hamm_m[k]);
                }
            };
            auto request = [&](uint32_t f) {
                const uint16_t *x = row + seg0 + (int)kHop * (int)(f0 + f);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const int i = lane + 64 * k;
                    if (i < kFrameLen) s_pp[k] = *(const u32_align2 *)(x + i - 1);
                }
            };
            // exchange .. tier decision of frame fi (`more`: frame fi+1 exists); comments of the stages: the serial loop below
            auto middle = [&](uint32_t fi, uint32_t (&v)[4][4], bool more) {
                uint32_t u[4][4];
                exchange(v, u);
#pragma unroll
                for (int e4 = 0; e4 < 4; e4++) fft_pass4_dbl(u, e4, tw);
                wave_sync();
                uint32_t k5[4][4][2];
                load_tw32(s_tw5, lane, k5);
                uint32_t nn[8];
#pragma unroll
                for (int e3 = 0; e3 < 4; e3++) {
                    bfly_pk_dbl<true, false, 0>(u[e3][0], u[e3][1], u[e3][2], u[e3][3], k5[e3][0][0], k5[e3][0][1], k5[e3][1][0],
                                                k5[e3][1][1], k5[e3][2][0], k5[e3][2][1], k5[e3][3][0], k5[e3][3][1]);
                    if constexpr (kFeat == SR_FEAT_FFT) {
                        uint32_t *fr = frow + (f0 + fi) * kFeatW + lane + 64 * e3;
                        fr[0] = u[e3][0];
                        fr[256] = u[e3][1];
                    }
                    nn[2 * e3] = (uint32_t)sdot2z(u[e3][0], u[e3][0]);
                    nn[2 * e3 + 1] = (uint32_t)sdot2z(u[e3][1], u[e3][1]);
                }
                const uint32_t nmax = max(max(max(max(nn[0], nn[1]), nn[2]), max(max(nn[3], nn[4]), nn[5])), max(nn[6], nn[7]));
                if (more) {  // every exchange word has been read: the next frame's window goes over them
                    wave_sync();
                    window();
                }
#ifdef SR_TESTING
                const bool quiet = __builtin_expect(__builtin_amdgcn_ballot_w64(nmax > kMagSmallMax) == 0 && !a.mag_table_off, 1);
#else
                const bool quiet = __builtin_expect(__builtin_amdgcn_ballot_w64(nmax > kMagSmallMax) == 0, 1);
#endif
                if (quiet) {
#pragma unroll
                    for (int k = 0; k < 8; k++) asm volatile("buffer_load_ushort %0, %1, %2, 0 idxen" : "=v"(mq[k]) : "v"(nn[k]), "s"(mag_rs));
                } else if (__builtin_amdgcn_ballot_w64(nmax > a.mag_cheap_max) == 0) {
#pragma unroll
                    for (int e3 = 0; e3 < 4; e3++) {
                        const f32x2 m = f32x2{__builtin_amdgcn_sqrtf((float)(int)nn[2 * e3]), __builtin_amdgcn_sqrtf((float)(int)nn[2 * e3 + 1])} *
                                        f32x2{10.0f, 10.0f};
                        mq[2 * e3] = cvt_u32(m.x);
                        mq[2 * e3 + 1] = cvt_u32(m.y);
                    }
                } else {
#pragma unroll
                    for (int e3 = 0; e3 < 4; e3++) {
                        const f32x2 m = sqrt_rn_int2(f32x2{(float)(int)nn[2 * e3], (float)(int)nn[2 * e3 + 1]}) * f32x2{10.0f, 10.0f};
                        mq[2 * e3] = cvt_u32(m.x);
                        mq[2 * e3 + 1] = cvt_u32(m.y);
                    }
                }
                pq = quiet;
                if (fi + 2 < nf) request(fi + 2);
            };
            // energies .. powb[r] of the carried frame, row r of the wave.  `young`: the three sample loads of request() were issued
            // behind the gathers on every path that leads here, so the wait may leave them in flight.
            auto back_end = [&](uint32_t r, auto young) {
                wave_sync();  // (the front's reads of xw are done: buf takes the energies)
                auto energies = [&]() {  // squares of the carried magnitudes, in the order the filterbank reads them in
                    uint32_t en[8];
#pragma unroll
                    for (int e3 = 0; e3 < 4; e3++) {
                        const uint32_t q0 = mq[2 * e3], q1 = mq[2 * e3 + 1];
                        if constexpr (kFeat == SR_FEAT_MAG) {  // the carried frame's row
                            uint32_t *fr = frow + (f0 + r) * kFeatW + lane + 64 * e3;
                            const uint32_t sh = pq ? 2u : 0u;
                            fr[0] = q0 >> sh;
                            fr[256] = q1 >> sh;
                        }
                        en[2 * e3] = umul24(q0, q0);
                        en[2 * e3 + 1] = umul24(q1, q1);
                    }
                    store_energies(en);
                    wave_sync();
                };
                // the two tiers' back ends are two whole branches: the literal form's sixteen raw weights are live in its own only
                uint32_t pe[8], po[8], se = 0, so = 0;
                if (pq) {
                    if constexpr (decltype(young)::value)
                        asm volatile("s_waitcnt vmcnt(3)" : "+v"(mq[0]), "+v"(mq[1]), "+v"(mq[2]), "+v"(mq[3]), "+v"(mq[4]), "+v"(mq[5]), "+v"(mq[6]), "+v"(mq[7]));
                    else
                        asm volatile("s_waitcnt vmcnt(0)" : "+v"(mq[0]), "+v"(mq[1]), "+v"(mq[2]), "+v"(mq[3]), "+v"(mq[4]), "+v"(mq[5]), "+v"(mq[6]), "+v"(mq[7]));
                    energies();
                    const uint4 q0 = *(const uint4 *)(buf + c0), q1 = *(const uint4 *)(buf + c1);
                    const uint32_t e[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        u32x4 me, mo;
                        if constexpr (kTmRegs) me = tm_r[c], mo = tm_r[c + 2];
                        else me = s_tm[64 * c + lane], mo = s_tm[64 * (c + 2) + lane];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            se += mel_term_fused(e[4 * c + k], me[k]);  // (the table's squares are E << 4 already)
                            so += mel_term_fused(e[4 * c + k], mo[k]);
                            pe[4 * c + k] = se;
                            po[4 * c + k] = so;
                        }
                    }
                } else {
                    u32x4 tw_e[2], tw_o[2];  // requested from the (cache-resident) table first: they arrive behind the energies
                    uint32_t off = tw_off;   // (opaque: hoisted out of the loop, the two 64-bit lane addresses cost the QUIET path four VGPRs)
                    asm("" : "+v"(off));
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        tw_e[c] = *(const u32x4 *)((const char *)a.t.tri_even32 + off + 16 * c);
                        tw_o[c] = *(const u32x4 *)((const char *)a.t.tri_odd32 + off + 16 * c);
                    }
                    energies();
                    const uint4 q0 = *(const uint4 *)(buf + c0), q1 = *(const uint4 *)(buf + c1);
                    const uint32_t e[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
                    for (int c = 0; c < 2; c++) {
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            se += e[4 * c + k] * tw_e[c][k] / 100u;
                            so += e[4 * c + k] * tw_o[c][k] / 100u;
                            pe[4 * c + k] = se;
                            po[4 * c + k] = so;
                        }
                    }
                }
                const uint32_t xe = wave_scan_incl(se), xo = wave_scan_incl(so);
                store_prefixes(pe, po);
                buf[2 * kBins + lane] = xe;
                moff[lane] = xo;
                wave_sync();
                if (lane < kMel) {
                    const uint32_t *X = (lane & 1) ? moff : buf + 2 * kBins;
                    const uint32_t hi = buf[p_hi] + X[x_hi], lo = f_lo ? buf[p_lo] + X[x_lo] : 0u;
                    powb[r * kMelPad + lane] = hi - lo;
                    if constexpr (kFeat == SR_FEAT_MEL) frow[(f0 + r) * kFeatW + lane] = hi - lo;
                }
                wave_sync();  // (the exchange of the frame in flight overwrites the prefixes)
            };
            constexpr std::false_type kDrain{};
            if (nf) {
                window();
                if (nf > 1) request(1);
#if SR_MFCC_PIPE_PEEL
                // first and last frame peeled: the steady-state body is one straight-line block, and on every path into its back end
                // the next request follows the gathers
                constexpr std::integral_constant<bool, SR_MFCC_PIPE_VMCNT != 0> kSteady{};
                {
                    wave_sync();
                    uint32_t v[4][4];
                    fft_front_real160(xw, lane, tw, s_tw3, v);
                    middle(0, v, nf > 1);
                }
                for (uint32_t fi = 1; fi + 1 < nf; fi++) {
                    wave_sync();
                    uint32_t v[4][4];
                    fft_front_real160(xw, lane, tw, s_tw3, v);
                    back_end(fi - 1, kSteady);
                    middle(fi, v, true);
                }
                if (nf > 1) {
                    wave_sync();
                    uint32_t v[4][4];
                    fft_front_real160(xw, lane, tw, s_tw3, v);
                    back_end(nf - 2, kDrain);
                    middle(nf - 1, v, false);
                }
#else
                for (uint32_t fi = 0; fi < nf; fi++) {
                    wave_sync();
                    uint32_t v[4][4];
                    fft_front_real160(xw, lane, tw, s_tw3, v);
                    if (fi > 0) back_end(fi - 1, kDrain);
                    middle(fi, v, fi + 1 < nf);
                }
#endif
                back_end(nf - 1, kDrain);
            }
        }

        // ---- log (MFCC.C:165-170) and DCT (MFCC.C:173-183) for the wave's nf frames, all lanes busy
        // (the pad word of each row goes through the log as well: harmless, never read)
        // (round 6: all rounds' estimates first, then all threshold pairs in flight at once, then the corrections -- as a loop
        // each round waited for its own pair of thresholds from the table in L2: seven serial round trips per 16 frames)
        {
            constexpr int kLogRounds = (kFPW * kMelPad + 63) / 64;
            const uint32_t n_log = nf * kMelPad;
            uint32_t nv[kLogRounds], mv[kLogRounds];
            u32x2 tv[kLogRounds];
#pragma unroll
            for (int r = 0; r < kLogRounds; r++) {
                const uint32_t t = lane + 64u * r;
                nv[r] = powb[t];  // (rounds past n_log read the wave's own scratch behind the filterbank outputs: in bounds, unused)
                mv[r] = log100_est(nv[r]);
                tv[r] = *(const u32_pair_align4 *)((const char *)a.t.log_thr + 4u * mv[r]);
            }
#pragma unroll
            for (int r = 0; r < kLogRounds; r++) {
                const uint32_t t = lane + 64u * r;
                if (t < n_log) powb[t] = log100_fix(nv[r], mv[r], tv[r].x, tv[r].y) << 14;
            }
        }
        wave_sync();
        if constexpr (kFeat == SR_FEAT_LOGMEL) {  // the log stage's outputs as the DCT reads them, un-shifted: word t = fi*24 + h
            uint32_t *fw = frow + f0 * kFeatW;
            for (uint32_t t = lane; t < nf * kFeatW; t += 64) {
                const uint32_t fi = t / kFeatW, h = t - fi * kFeatW;
                fw[t] = powb[fi * kMelPad + h] >> 14;
            }
        }
        // output t = fi*12 + h of the wave's tile goes to out[(f0 + fi)*12 + h] = out_w[t]: consecutive lanes store
        // consecutive s16; fi = t / 12 by a 24-bit multiply (exact for t < 2^13), all index arithmetic in 32 bits
        // (left to the compiler the 64-bit subscript became eight v_mad_u64_u32 per round)
        {
            int16_t *out_w = out + (size_t)f0 * kCoef;
#pragma unroll
            for (uint32_t tl = lane; tl < (uint32_t)(kFPW * kCoef); tl += 64) {
                uint32_t t = tl;
                // (two-frame loop: a round's row and table addresses are functions of the lane alone; hoisted out of the work-item
                // loop they sat in VGPRs through the frame loop, which has none to spare -- opaque, they are recomputed per 16 frames)
                if constexpr (kPipe) asm volatile("" : "+v"(t));
                if (t < nf * kCoef) {
                    const uint32_t fi = umul24(t, 10923u) >> 17, h = t - umul24(fi, (uint32_t)kCoef);
                    const uint32_t *pw = powb + umul24(fi, (uint32_t)kMelPad), *dm = s_dctM + umul24(h, (uint32_t)kMelPad);
                    const int *ds = s_dctS + umul24(h, (uint32_t)kMelPad);
                    int acc = 0;
#pragma unroll
                    for (int i = 0; i < kMel; i++) acc = mad24((int)__umulhi(pw[i], dm[i]), ds[i], acc);
                    out_w[t] = (int16_t)acc;
                }
            }
        }
        wave_sync();
        // rows >= frm_num of this tile are zeroed so that every row of the output is defined
        {
            const uint32_t r0 = f0 + nf, r1 = (f0 + kFPW < a.max_frames) ? f0 + kFPW : a.max_frames;
            for (uint32_t t = r0 * kCoef + lane; t < r1 * kCoef && r0 < r1; t += 64) out[t] = 0;
        }
        if constexpr (kFeat != 0) {  // feature rows >= frm_num of this tile, likewise
            const uint32_t r0 = f0 + nf, r1 = (f0 + kFPW < a.max_frames) ? f0 + kFPW : a.max_frames;
            for (uint32_t t = r0 * kFeatW + lane; t < r1 * kFeatW && r0 < r1; t += 64) frow[t] = 0;
        }
    }
}

// the 16 kHz / 512-point EXTENSION front end lives in k_mfcc_ext.hip
uint32_t mfcc_ext_frames_per_tile();
int mfcc_ext_occupancy(int *per_cu);
void launch_mfcc_ext(const MfccArgs &a, uint32_t grid, hipStream_t s);
void launch_mfcc_ext_features(const MfccArgs &a, int kind, uint32_t *feat, uint32_t grid, hipStream_t s);

uint32_t mfcc_frames_per_tile(uint32_t frame_len) { return frame_len == 320 ? mfcc_ext_frames_per_tile() : (uint32_t)(kMfccWaves * kFramesPerWave); }
// frames per work item of the underfilled-launch forms, 0 = mid, 1 = small (the extension kernel has one form)
uint32_t mfcc_frames_per_tile_small(uint32_t frame_len, uint32_t which)
{
    return frame_len == 320 ? mfcc_ext_frames_per_tile() : (uint32_t)(kMfccWaves * (which ? kFramesPerWaveSmall : kFramesPerWaveMid));
}

// workgroups of the frame kernel that fit on the current device at once (occupancy query x CU count)
uint32_t mfcc_resident_workgroups(uint32_t frame_len)
{
    int dev = 0, n_cu = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu < 1) return 0;
    int e;
    if (frame_len == 320)
        e = mfcc_ext_occupancy(&per_cu);
    else
        e = (int)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_mfcc<kFramesPerWave>, 64 * kMfccWaves,
                                                              (size_t)kMfccWaves * mfcc_wave_lds_words(kFramesPerWave) * sizeof(uint32_t));
    if (e != (int)hipSuccess || per_cu < 1) return 0;
    return (uint32_t)(per_cu * n_cu);
}

void launch_mfcc(const MfccArgs &a, const MfccMagTab &tab, hipStream_t s)
{
    if (a.generic) {
        launch_mfcc_gen(a, s);
        return;
    }
    if (a.n_items == 0) return;
    // persistent-style grid: a few times the workgroups that are resident at once (see sr_create), work items strided
    const uint32_t cap = a.grid_cap ? a.grid_cap : 4096u;
    const uint32_t grid = a.n_items < cap ? a.n_items : cap;
    if (a.frame_len == 320) {
        launch_mfcc_ext(a, grid, s);
        return;
    }
    if (a.small_tiles == 2) {  // a.tiles counts tiles of mfcc_frames_per_tile_small(frame_len, 1) frames
        const size_t lds = (size_t)kMfccWaves * mfcc_wave_lds_words(kFramesPerWaveSmall) * sizeof(uint32_t);
        SR_LAUNCH_POINT(s, "k_mfcc");
        hipLaunchKernelGGL(k_mfcc<kFramesPerWaveSmall>, dim3(grid), dim3(64 * kMfccWaves), lds, s, mfcc_tab_args(a, tab));
        return;
    }
    if (a.small_tiles == 1) {  // ... of mfcc_frames_per_tile_small(frame_len, 0) frames
        const size_t lds = (size_t)kMfccWaves * mfcc_wave_lds_words(kFramesPerWaveMid) * sizeof(uint32_t);
        SR_LAUNCH_POINT(s, "k_mfcc");
        hipLaunchKernelGGL(k_mfcc<kFramesPerWaveMid>, dim3(grid), dim3(64 * kMfccWaves), lds, s, mfcc_tab_args(a, tab));
        return;
    }
    const size_t lds = (size_t)kMfccWaves * mfcc_wave_lds_words(kFramesPerWave) * sizeof(uint32_t);
    SR_LAUNCH_POINT(s, "k_mfcc");
    hipLaunchKernelGGL(k_mfcc<kFramesPerWave>, dim3(grid), dim3(64 * kMfccWaves), lds, s, mfcc_tab_args(a, tab));
}

template <int kFPW, int kKind>
static void launch_mfcc_feat_kind(const MfccArgs &a, const MfccMagTab &tab, uint32_t *feat, uint32_t grid, hipStream_t s)
{
    const size_t lds = (size_t)kMfccWaves * mfcc_wave_lds_words(kFPW) * sizeof(uint32_t);
    SR_LAUNCH_POINT(s, "k_mfcc");
    hipLaunchKernelGGL((k_mfcc<kFPW, MfccTabArgs<MfccFeatArgs<kKind>>>), dim3(grid), dim3(64 * kMfccWaves), lds, s,
                       mfcc_tab_args(mfcc_feat_args<kKind>(a, feat), tab));
}
template <int kFPW>
static void launch_mfcc_feat_form(const MfccArgs &a, const MfccMagTab &tab, int kind, uint32_t *feat, uint32_t grid, hipStream_t s)
{
    switch (kind) {
    case SR_FEAT_FFT: launch_mfcc_feat_kind<kFPW, SR_FEAT_FFT>(a, tab, feat, grid, s); break;
    case SR_FEAT_MAG: launch_mfcc_feat_kind<kFPW, SR_FEAT_MAG>(a, tab, feat, grid, s); break;
    case SR_FEAT_MEL: launch_mfcc_feat_kind<kFPW, SR_FEAT_MEL>(a, tab, feat, grid, s); break;
    case SR_FEAT_LOGMEL: launch_mfcc_feat_kind<kFPW, SR_FEAT_LOGMEL>(a, tab, feat, grid, s); break;
    default: break;  // (kinds are checked by the entry point)
    }
}

// the feature kernels in the form and grid launch_mfcc would pick for the same arguments
void launch_mfcc_features(const MfccArgs &a, const MfccMagTab &tab, int kind, uint32_t *feat, hipStream_t s)
{
    if (a.generic) {
        launch_mfcc_gen_features(a, kind, feat, s);
        return;
    }
    if (a.n_items == 0) return;
    const uint32_t cap = a.grid_cap ? a.grid_cap : 4096u;
    const uint32_t grid = a.n_items < cap ? a.n_items : cap;
    if (a.frame_len == 320)
        launch_mfcc_ext_features(a, kind, feat, grid, s);
    else if (a.small_tiles == 2)
        launch_mfcc_feat_form<kFramesPerWaveSmall>(a, tab, kind, feat, grid, s);
    else if (a.small_tiles == 1)
        launch_mfcc_feat_form<kFramesPerWaveMid>(a, tab, kind, feat, grid, s);
    else
        launch_mfcc_feat_form<kFramesPerWave>(a, tab, kind, feat, grid, s);
}

}  // namespace sr
