// sr_fft_dev.h -- the Q15 radix-4 butterfly of cr4_fft_1024_stm32.s in packed 16-bit arithmetic, coefficient loading, and the register/LDS layouts shared by k_mfcc, k_mfcc_ext and the generic FFT kernels.
// gfx950 (MI355X, CDNA4) only; wave = 64 lanes; no MFMA (the path has no dense contraction), integer VALU + LDS.
// Every kernel reproduces the reference's integer arithmetic bit for bit; cited lines are relative to the reference tree.
#pragma once
#include <type_traits>

#include "sr_dev.h"
#include "sr_fft_layout.h"

namespace sr {

// ------------------------------------------------------------------------------------------------
// Q15 radix-4 butterfly of the ST FFT (cr4_fft_1024_stm32.s)
// ------------------------------------------------------------------------------------------------
// CXMUL_V7 (.s:95-102): Y*conj(K), Q14.  The asm's 3-multiply form equals, in the ring of 32-bit
// integers, re = Yr*Kc + Yi*Ks, im = Yi*Kc - Yr*Ks with Kc = Kr'+Ki, Ks = Ki (no term overflows).
__device__ __forceinline__ void cxmul(uint32_t y, uint32_t ka, uint32_t kb, int &re, int &im)
{
    re = sdot2z(y, ka);
    im = sdot2z(y, kb);
}

// CXADDA4 (.s:105-129, S = 14) and the combine of BUTFLY4ZERO_OPT (.s:147-168, S = 0).
// In: A (sign-extended sample), B, C, D (products or samples).  Out as stored by the asm:
//   x[j] = (ar, ai)   x[j+q] = (br, bi)   x[j+2q] = (cr, ci)   x[j+3q] = (di, dr)   <- "inversion"
template <int S>
__device__ __forceinline__ void r4_combine(int &ar, int &ai, int &br, int &bi, int &cr, int &ci, int &dr, int &di)
{
    int tr = cr + dr, ti = ci + di;  // (C,D) = (C+D, C-D)
    dr = cr - dr;
    di = ci - di;
    cr = tr;
    ci = ti;
    ar >>= 2;
    ai >>= 2;
    ar += br >> (2 + S);
    ai += bi >> (2 + S);
    br = ar - (br >> (1 + S));
    bi = ai - (bi >> (1 + S));
    ar += cr >> (2 + S);
    ai += ci >> (2 + S);
    cr = ar - (cr >> (1 + S));
    ci = ai - (ci >> (1 + S));
    br += di >> (2 + S);
    bi -= dr >> (2 + S);
    di = br - (di >> (1 + S));
    dr = bi + (dr >> (1 + S));
}

// One twiddled butterfly on packed words; k* = packed coefficient pairs for the legs j+q, j+2q, j+3q.
// CXADDA4 (.s:105-129) in packed 16-bit arithmetic.  Every value the asm stores is the low 16 bits of a
// 32-bit sum of terms (A>>2), (X>>16), (X>>15); sums mod 2^16 may be taken in any order.  With h(X) = X>>16 and
// p(X) = X>>15 (both halves at once, mod 2^16) and (X>>15) = 2*(X>>16) + bit15(X):
//   A1 = a + h(B)                B1 = A1 - (B>>15)                    = A1 - p(B)
//   A2 = A1 + h(C')   = x[j]     C2 = A2 - (C'>>15)                   = x[j] - p(C')      = x[j+2q]
//   B2 = B1 + S*h(D'~) = x[j+q]  D2 = B2 - S*(D'>>15)~                = x[j+q] - S*p(D'~) = x[j+3q]
// S = (+1,-1), ~ = halves swapped (.s:125-128: Br += Di>>16, Bi -= Dr>>16, Di = Br - Di>>15, Dr = Bi + Dr>>15, stored
// as (Di, Dr)).  Each ">>15" output is therefore ONE packed op on the matching ">>16" output; h() is one v_perm_b32,
// p() a plain shift + one SDWA shift: 16 VALU for the combine of a full butterfly (19 with the bit-15 form of round 1).
constexpr uint32_t kPkPlusMinus = 0xFFFF0001u;  // (+1, -1)
constexpr uint32_t kPkMinusPlus = 0x0001FFFFu;  // (-1, +1)

// combine step on 32-bit products B, C' = C+D, D' = C-D and the packed sample A
// CD_SAME: the D leg is zero, so C' = D' = C and the swapped D' halves are the C' halves rotated by 16 bits
// A_SHIFTED: x0_in already holds A >> 2 (k_mfcc stores the samples that are pass-2 A legs that way)
template <bool HALF, bool HAS_B, bool CD_SAME = false, bool A_SHIFTED = false>
__device__ __forceinline__ void r4_packed(uint32_t x0_in, int br, int bi, int sr, int si, int tr, int ti, uint32_t &x0,
                                          uint32_t &x1, uint32_t &x2, uint32_t &x3)
{
    const uint32_t a = A_SHIFTED ? x0_in : pk_ashr(x0_in, 2);
    uint32_t A1 = a, B1 = a;
    if (HAS_B) {
        A1 = pk_add(a, pk_hi16(br, bi));
        B1 = pk_sub(A1, pk_s15(br, bi));
    }
    const uint32_t hC = pk_hi16(sr, si);
    x0 = pk_add(A1, hC);
    // D' with its halves swapped: (D'i>>16, D'r>>16).  CD_SAME: they are C''s own halves, exchanged by the multiply-add's operand
    // selects (round 6; a v_alignbit_b32 each before: 8 instructions per frame in pass 2)
    x1 = CD_SAME ? pk_mad_swap(hC, kPkPlusMinus, B1) : pk_mad(pk_hi16(ti, tr), kPkPlusMinus, B1);
    if (!HALF) {
        const uint32_t pC = pk_s15(sr, si);
        x2 = pk_sub(x0, pC);
        x3 = CD_SAME ? pk_mad_swap(pC, kPkMinusPlus, x1) : pk_mad(pk_s15(ti, tr), kPkMinusPlus, x1);
    }
}

template <bool HALF>  // HALF: only x0, x1 are produced (last pass: bins >= 512 are never read, MFCC.C:49)
__device__ __forceinline__ void bfly_pk(uint32_t &x0, uint32_t &x1, uint32_t &x2, uint32_t &x3, uint32_t k1a,
                                        uint32_t k1b, uint32_t k2a, uint32_t k2b, uint32_t k3a, uint32_t k3b,
                                        uint32_t k3na, uint32_t k3nb)
{
    int br, bi, cr, ci;
    cxmul(x2, k2a, k2b, cr, ci);
    cxmul(x1, k1a, k1b, br, bi);
    // C' = C + D and D' = C - D without ever forming D: D = x3*conj(K3) is accumulated onto C with K3 and -K3
    const int sr = sdot2a(x3, k3a, cr), si = sdot2a(x3, k3b, ci);
    const int tr = sdot2a(x3, k3na, cr), ti = sdot2a(x3, k3nb, ci);
    r4_packed<HALF, true>(x0, br, bi, sr, si, tr, ti, x0, x1, x2, x3);
}

// ---- DOUBLED LEGS (round 9): the combine for legs that enter their multiply as 2 Y --------------------------------------
// v_dot2_i32_i16(2 Y, K) is 2 X mod 2^32 whenever 2 Y is an i16, so for a product pair computed from a doubled leg
//   p(X) = bits 15..30 of X = bits 16..31 of 2 X          : ONE v_perm_b32, the selector h() uses on plain products
//   h(X) = bits 16..31 of X = p(X) >> 1 (arithmetic, per half) : one v_pk_ashrrev_i16, IF bit 31 of X equals bit 30, i.e. |X| < 2^30
// -- two VALU per pair instead of three, no SDWA and none of its wait states.  A butterfly whose outputs are non-A legs of
// the next pass emits them doubled (or times a lane's m in {1, 2}) so that doubling costs nothing there: the add chain above
// becomes v_pk_mad_u16 with the multipliers (m, m), (-m, -m), (m, -m), (-m, m) -- operand selects of ONE word (+m, -m),
// pk_mad_sel -- started from m * (A >> 2), the only extra instruction (it is not A >> 1: the low bit of A >> 2 is kept).
// Sums are mod 2^16 in any order, as before; the doubled output is 2 x for the value x the asm stores iff |x| < 2^14.
//
// WHERE IT MAY BE USED.  Both conditions -- every doubled leg |Y| < 2^14, every product pair |B|, |C + D|, |C - D| < 2^30 --
// are properties of the input range, so only the zero-padded real frame of k_mfcc takes this form (fft_front_real160 and
// the passes 4-5 behind it); transforms of arbitrary 16-bit complex input (k_mfcc_ext, k_mfcc_gen, fft_full_wave) keep the
// plain one.  The bound, with the constants of the table gen_twiddles writes (sr_tables.cpp; recomputed from the table
// itself by tests/test_fft_leg_bounds.py): every entry has |Kc|, |Ks| <= 16384 (+16384 occurs: Kc at b = 0, Ks at m = 2,
// b = q/2 -- which is why the LEG is doubled and never the coefficient: 32768 is no i16) and |Kc| + |Ks| <= 23171
// (16384 sqrt 2, rounded entries).  With M the largest |component| entering a pass:
//   a component of Y conj(K) is |Yr Kc + Yi Ks| <= 23171 M, of C +- D <= 46342 M;
//   an output is (A >> 2) +- h(B) +- h or (p - h) of C' or D'~, each term rounded by at most 1:
//   |x| <= M/4 + (23171 + 46342) M / 65536 + 3 < 1.3107 M + 3.
//   pass 1 (folded into the window): x >> 2 of an s16                     -> M2 <= 8192, legs REAL (they enter pass 2 DUPLICATED,
//                                                                            not doubled -- window_store below -- with the same 2 X)
//   pass 2: real legs, D = 0: |h(B)|, |h(C)| <= 8192 * 16384 / 65536 = 2048, A leg stored >> 4: 2048 + 2 * 2048 + 3
//                                                                         -> M3 <= 6147
//   pass 3: 1.3107 * 6147 + 3                                             -> M4 <= 8060
//   pass 4: 1.3107 * 8060 + 3                                             -> M5 <= 10568
// All below 2^14 = 16384; the largest product pair is |C +- D| of pass 5, 46342 * 10568 < 4.9e8 < 2^30 = 1.07e9 (pass 5
// doubles its B leg only: 23171 * 10568 < 2.5e8).  This holds for EVERY 16-bit capture: the window's s16 wrap bounds M2.
constexpr uint32_t kPkTwo = 0xFFFE0002u;  // (+2, -2)

// OUT = 0: outputs as the asm stores them; 1: doubled; 2: times the lane's m, `mul` = (+m, -m) in a VGPR.
// a = OUT-scaled A >> 2.  B (when HAS_B) comes from a doubled leg; C', D' too iff DBL_CD.
template <bool HALF, bool HAS_B, bool CD_SAME, bool DBL_CD, int OUT>
__device__ __forceinline__ void r4_packed_dbl(uint32_t a, uint32_t mul, int br, int bi, int sr, int si, int tr, int ti,
                                              uint32_t &x0, uint32_t &x1, uint32_t &x2, uint32_t &x3)
{
    // acc + x * (s_lo m, s_hi m), the halves of x exchanged if SWAP: L / H = 1 picks -m for that half
    auto madd = [&](uint32_t x, auto L, auto H, auto SWAP, uint32_t acc) -> uint32_t {
        constexpr int l = decltype(L)::value, h = decltype(H)::value;
        constexpr bool swap = decltype(SWAP)::value;
        if constexpr (OUT == 2) return pk_mad_sel<true, l, h, swap>(x, mul, acc);
        else if constexpr (OUT == 1) return pk_mad_sel<false, l, h, swap>(x, kPkTwo, acc);
        else if constexpr (swap) return pk_mad_swap(x, l ? kPkMinusPlus : kPkPlusMinus, acc);
        else if constexpr (l != h) return pk_mad(x, l ? kPkMinusPlus : kPkPlusMinus, acc);
        else if constexpr (l) return pk_sub(acc, x);
        else return pk_add(acc, x);
    };
    constexpr std::integral_constant<int, 0> P{};
    constexpr std::integral_constant<int, 1> N{};
    constexpr std::false_type kStraight{};
    constexpr std::integral_constant<bool, CD_SAME> kSwapC{};
    uint32_t A1 = a, B1 = a;
    if (HAS_B) {
        const uint32_t pB = pk_hi16(br, bi), hB = pk_ashr(pB, 1);
        A1 = madd(hB, P, P, kStraight, a);
        B1 = madd(pB, N, N, kStraight, A1);
    }
    uint32_t pC = 0, hC;
    if (DBL_CD) {
        pC = pk_hi16(sr, si);
        hC = pk_ashr(pC, 1);
    } else {
        hC = pk_hi16(sr, si);
        if (!HALF) pC = pk_s15(sr, si);
    }
    x0 = madd(hC, P, P, kStraight, A1);
    // D' with its halves swapped; CD_SAME: C''s own halves, exchanged by the operand selects (see r4_packed)
    uint32_t pD = 0, hD;
    if (CD_SAME) {
        pD = pC;
        hD = hC;
    } else if (DBL_CD) {
        pD = pk_hi16(ti, tr);
        hD = pk_ashr(pD, 1);
    } else {
        hD = pk_hi16(ti, tr);
        if (!HALF) pD = pk_s15(ti, tr);
    }
    x1 = madd(hD, P, N, kSwapC, B1);
    if (!HALF) {
        x2 = madd(pC, N, N, kStraight, x0);
        x3 = madd(pD, N, P, kSwapC, x1);
    }
}

// bfly_pk for a butterfly whose B leg x1 is doubled, and whose C and D legs x2, x3 are iff DBL_CD; outputs by OUT as above
template <bool HALF, bool DBL_CD, int OUT>
__device__ __forceinline__ void bfly_pk_dbl(uint32_t &x0, uint32_t &x1, uint32_t &x2, uint32_t &x3, uint32_t k1a,
                                            uint32_t k1b, uint32_t k2a, uint32_t k2b, uint32_t k3a, uint32_t k3b,
                                            uint32_t k3na, uint32_t k3nb, uint32_t mul = 0)
{
    int br, bi, cr, ci;
    cxmul(x2, k2a, k2b, cr, ci);
    cxmul(x1, k1a, k1b, br, bi);
    const int sr = sdot2a(x3, k3a, cr), si = sdot2a(x3, k3b, ci);
    const int tr = sdot2a(x3, k3na, cr), ti = sdot2a(x3, k3nb, ci);
    uint32_t a = pk_ashr(x0, 2);
    if (OUT == 1) a = pk_add(a, a);
    if (OUT == 2) a = pk_mul_lo_lo(a, mul);
    r4_packed_dbl<HALF, true, false, DBL_CD, OUT>(a, mul, br, bi, sr, si, tr, ti, x0, x1, x2, x3);
}

__device__ __forceinline__ uint32_t pk_neg(uint32_t w) { return pk_sub(0u, w); }

__device__ __forceinline__ void bfly(uint32_t &x0, uint32_t &x1, uint32_t &x2, uint32_t &x3, uint32_t k1a, uint32_t k1b,
                                     uint32_t k2a, uint32_t k2b, uint32_t k3a, uint32_t k3b)
{
    bfly_pk<false>(x0, x1, x2, x3, k1a, k1b, k2a, k2b, k3a, k3b, pk_neg(k3a), pk_neg(k3b));  // generic paths: negate on the fly
}

__device__ __forceinline__ int rev2(int d) { return ((d & 1) << 1) | (d >> 1); }

// LDS image of the 1024-point work array between passes 3 and 4: word j lives at j + 4*(j>>6).
// With lane = d0 + 4*d3 + 16*d4 writing j = d0 + 4*d1 + 16*d2 + 64*d3 + 256*d4 the 32 lanes of a
// ds_write_b32 group hit 32 distinct banks; reads by lane = j & 63 are consecutive words.
__device__ __forceinline__ int xaddr(int j) { return j + ((j >> 6) << 2); }
// (kXchgWords = 1088, the size of the area: sr_fft_layout.h)

// Coefficients a lane needs, all lane-invariant across frames -> loaded once per wave into VGPRs.
struct LaneTw {
    uint32_t s2[2][2];     // pass 2 (q=4):   legs j+q, j+2q (j+3q is always zero-padding); k_mfcc: low halves duplicated, real_leg_tw
    uint32_t s3[4][4][2];  // pass 3 (q=16):  per d1, legs j+q, j+2q, j+3q, and the j+3q pair negated
    uint32_t s4[4][2];     // pass 4 (q=64)
    uint32_t s5[4][4][2];  // pass 5 (q=256): per d3
};

// Table entry order per butterfly is (leg j+3q, leg j+2q, leg j+q)  (.s:182-191).
__device__ __forceinline__ void load_tw3(const DevTables &t, int base, int b, uint32_t (&k)[3][2])
{
    const int e = base + 3 * b;
    k[0][0] = t.tw_a[e + 2];
    k[0][1] = t.tw_b[e + 2];  // leg j+q
    k[1][0] = t.tw_a[e + 1];
    k[1][1] = t.tw_b[e + 1];  // leg j+2q
    k[2][0] = t.tw_a[e + 0];
    k[2][1] = t.tw_b[e + 0];  // leg j+3q
}

// legs j+q, j+2q, j+3q as above + entry [3] = the j+3q pair negated (for C+D / C-D by accumulation)
__device__ __forceinline__ void load_tw4(const DevTables &t, int base, int b, uint32_t (&k)[4][2])
{
    uint32_t k3[3][2];
    load_tw3(t, base, b, k3);
#pragma unroll
    for (int e = 0; e < 3; e++) {
        k[e][0] = k3[e][0];
        k[e][1] = k3[e][1];
    }
    k[3][0] = pk_sub(0u, k3[2][0]);
    k[3][1] = pk_sub(0u, k3[2][1]);
}

// d0: the digit of the FRONT lane order (passes 2 and 3); s4 and s5 belong to the reading lane = j & 63 of every order
__device__ __forceinline__ void load_lane_tw(const DevTables &t, int lane, int d0, LaneTw &tw)
{
    {
        uint32_t k[3][2];
        load_tw3(t, 0, d0, k);
        tw.s2[0][0] = k[0][0];
        tw.s2[0][1] = k[0][1];
        tw.s2[1][0] = k[1][0];
        tw.s2[1][1] = k[1][1];
    }
#pragma unroll
    for (int d1 = 0; d1 < 4; d1++) load_tw4(t, 12, d0 + 4 * d1, tw.s3[d1]);
    load_tw4(t, 60, lane, tw.s4);
#pragma unroll
    for (int d3 = 0; d3 < 4; d3++) load_tw4(t, 252, lane + 64 * d3, tw.s5[d3]);
}

// 32 lane-invariant coefficient words (4 entries x 2 words per butterfly, 4 butterflies) parked in LDS as
// 8 x 16-byte chunks, chunk c of lane l at [c*64 + l] (consecutive lanes -> consecutive 16-byte slots:
// conflict-free ds_read_b128 / ds_write_b128)
__device__ __forceinline__ void store_tw32(u32x4 *lds, int lane, const uint32_t (&k)[4][4][2])
{
    const uint32_t *f = &k[0][0][0];
#pragma unroll
    for (int c = 0; c < 8; c++) lds[c * 64 + lane] = u32x4{f[4 * c], f[4 * c + 1], f[4 * c + 2], f[4 * c + 3]};
}
__device__ __forceinline__ void load_tw32(const u32x4 *lds, int lane, uint32_t (&k)[4][4][2])
{
    uint32_t *f = &k[0][0][0];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const u32x4 q = lds[c * 64 + lane];
        f[4 * c] = q.x;
        f[4 * c + 1] = q.y;
        f[4 * c + 2] = q.z;
        f[4 * c + 3] = q.w;
    }
}
// pass-3 coefficients depend on (d0, d1) only: 4 x 32 words, read with lane-broadcast by d0 (k_mfcc: lane >> 4, two values per
// service group of the read; the reasoning below was made for d0 = lane & 3 and holds for fewer rows per group).  The four rows are
// kTw3Row = 9 chunks apart, not 8: the lanes of a ds_read_b128 service group hold all four d0, and with rows of 32 words
// d0 = 0 / 2 (and 1 / 3) fall on the same banks with different addresses -- every one of the loads was a 2-way conflict
// (round 6: 32 of k_mfcc's 53 conflict cycles per frame, profiles/experiments/RESULTS.md)
constexpr int kTw3Row = 9;
__device__ __forceinline__ void load_tw32_d0(const u32x4 *lds, int d0, uint32_t (&k)[4][4][2])
{
    uint32_t *f = &k[0][0][0];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const u32x4 q = lds[d0 * kTw3Row + c];
        f[4 * c] = q.x;
        f[4 * c + 1] = q.y;
        f[4 * c + 2] = q.z;
        f[4 * c + 3] = q.w;
    }
}

// Passes 1-3 for the zero-padded real frame that get_mfcc feeds (MFCC.C:37-47): only x[0..159] are
// non-zero and every imaginary part is 0.  Pass 1 (.s:226-232) then degenerates exactly to
// out[4*idx+k] = x[bitrev8(idx)] >> 2 (k = 0..3), so it is folded into the gather.
// lane = d3 + 4*d4 + 16*d0 ; v[d1][d2] <-> j = d0 + 4*d1 + 16*d2 + 64*d3 + 256*d4.  (The lane order is the one the exchange image
// behind it wants, fft_exchange_tid below: the lanes that hold one reading lane's sixteen words are consecutive.  The generic
// transforms keep d0 + 4*d3 + 16*d4 and fft_exchange.  tw.s2, tw.s3 and the rows of tw3_lds are per d0: load_lane_tw(.., d0 = lane >> 4, ..).)
// xw: the windowed frame as one 32-bit word per sample, written by window_store below: 4-byte stores of consecutive samples and
// the reads below at word base + 16 m are both conflict-free; with two samples per word the stores of lanes 2 m / 2 m + 1 went
// to one word.  Samples 0..63, the A legs of pass 2, are stored >> 2 once more (round 6), as the word (a, 2 a): butterfly
// d2 = 0 reads the low half, the doubled butterflies d2 > 0 their 2 a from the high half.  Samples 64..159, its B and C legs,
// are stored as (Y, Y): the real leg enters its multiply DUPLICATED instead of doubled -- with the coefficient word's low half
// in both halves too (real_leg_tw), v_dot2_i32_i16((Y, Y), (K, K)) = 2 Y K, the doubled product at no instruction at all.
constexpr uint32_t kPkOneTwo = 0x00020001u;  // (1, 2)
template <int K>  // K = 0: sample i < 64
__device__ __forceinline__ void window_store(uint32_t *xw, int i, uint32_t prev_cur, int mid, int hm)
{
    if (K == 0) {
        xw[i] = pk_mul_lo_dup(window_sample<4>(prev_cur, mid, hm), kPkOneTwo);
    } else {
        // the pass-1 output A >> 2 as a 16-bit pattern into both halves: a second 2-byte LDS store, which takes no VALU slot
        const uint32_t y = window_sample<2>(prev_cur, mid, hm);
        xw[i] = y;
        ((uint16_t *)(xw + i))[1] = (uint16_t)y;
    }
}
// pass-2 coefficient words for duplicated real legs: (Kc, Ks) -> (Kc, Kc) and (-Ks, Kc) -> (-Ks, -Ks)
__device__ __forceinline__ void real_leg_tw(LaneTw &tw)
{
#pragma unroll
    for (int l = 0; l < 2; l++)
#pragma unroll
        for (int w = 0; w < 2; w++) tw.s2[l][w] = __builtin_amdgcn_perm(0u, tw.s2[l][w], 0x01000100u);
}
__device__ __forceinline__ void fft_front_real160(const uint32_t *xw, int lane, const LaneTw &tw, const u32x4 *tw3_lds,
                                                  uint32_t (&v)[4][4])
{
    const int d0 = lane >> 4, d3 = lane & 3, d4 = (lane >> 2) & 3;
    const int base = rev2(d4) + 4 * rev2(d3);
    // bitrev8(j>>2) = base + 16*rev2(d2) + 64*rev2(d1); >= 160 <=> zero padding
    uint32_t y[10];
    y[0] = *(const uint16_t *)(xw + base);
#pragma unroll
    for (int m = 1; m < 4; m++) y[m] = ((const uint16_t *)(xw + base + 16 * m))[1];
#pragma unroll
    for (int m = 4; m < 10; m++) y[m] = xw[base + 16 * m];
    // (the A legs go into packed adds as they are: opaque, or the compiler re-zeroes halves that ds_read_u16 has just zero-extended)
#pragma unroll
    for (int m = 0; m < 4; m++) asm("" : "+v"(y[m]));
    // pass 2: the outputs of butterfly d2 are all leg d2 of pass 3 -- d2 = 0 the A legs (plain), d2 > 0 doubled
#pragma unroll
    for (int d2 = 0; d2 < 4; d2++) {
        const int r2 = ((d2 & 1) << 1) | (d2 >> 1);
        uint32_t x0 = y[r2];                                      // d1 = 0 -> rows   0..63
        uint32_t x2 = y[4 + r2];                                  // d1 = 2 -> rows  64..127
        uint32_t x1 = (d2 == 0) ? y[8] : (d2 == 2) ? y[9] : 0u;   // d1 = 1 -> rows 128..159, else padding
        uint32_t x3 = 0u;                                         // d1 = 3 -> rows >= 192: padding
        // real samples, duplicated, against the duplicated coefficient halves (real_leg_tw): the dot products give
        // (2 Yr*Kc, -2 Yr*Ks) directly; D = 0 => C' = D' = C
        int cr, ci;
        cxmul(x2, tw.s2[1][0], tw.s2[1][1], cr, ci);
        (void)x3;
        if (d2 == 0) {
            int br, bi;
            cxmul(x1, tw.s2[0][0], tw.s2[0][1], br, bi);
            r4_packed_dbl<false, true, true, true, 0>(x0, 0u, br, bi, cr, ci, cr, ci, v[0][d2], v[1][d2], v[2][d2], v[3][d2]);
        } else if (d2 == 2) {
            int br, bi;
            cxmul(x1, tw.s2[0][0], tw.s2[0][1], br, bi);
            r4_packed_dbl<false, true, true, true, 1>(x0, 0u, br, bi, cr, ci, cr, ci, v[0][d2], v[1][d2], v[2][d2], v[3][d2]);
        } else {
            r4_packed_dbl<false, false, true, true, 1>(x0, 0u, 0, 0, cr, ci, cr, ci, v[0][d2], v[1][d2], v[2][d2], v[3][d2]);
        }
    }
    // pass-3 coefficients (24 words per lane) are parked in LDS, shared by the workgroup's waves
    uint32_t k3[4][4][2];
    load_tw32_d0(tw3_lds, d0, k3);
    // pass 3: across the exchange an output's leg in pass 4 is d3 of THIS lane -- d3 = 0 writes A legs (m = 1), the others
    // doubled legs (m = 2)
    const uint32_t mul = d3 ? kPkTwo : kPkPlusMinus;
#pragma unroll
    for (int d1 = 0; d1 < 4; d1++)
        bfly_pk_dbl<false, true, 2>(v[d1][0], v[d1][1], v[d1][2], v[d1][3], k3[d1][0][0], k3[d1][0][1], k3[d1][1][0], k3[d1][1][1],
                                    k3[d1][2][0], k3[d1][2][1], k3[d1][3][0], k3[d1][3][1], mul);
}

// lane (d0,d3,d4) -> LDS -> lane' = j & 63 holding u[d3][d4]: the generic transforms' exchange (lane = d0 + 4*d3 + 16*d4)
__device__ __forceinline__ void fft_exchange(uint32_t *buf, int lane, const uint32_t (&v)[4][4], uint32_t (&u)[4][4])
{
    const int d0 = lane & 3, d3 = (lane >> 2) & 3, d4 = lane >> 4;
    const int jw = d0 + 64 * d3 + 256 * d4;
#pragma unroll
    for (int d1 = 0; d1 < 4; d1++)
#pragma unroll
        for (int d2 = 0; d2 < 4; d2++) buf[xaddr(jw + 4 * d1 + 16 * d2)] = v[d1][d2];
    wave_sync();
#pragma unroll
    for (int e3 = 0; e3 < 4; e3++)
#pragma unroll
        for (int e4 = 0; e4 < 4; e4++) u[e3][e4] = buf[xaddr(lane + 64 * e3 + 256 * e4)];
}

// The same exchange behind fft_front_real160's lane order d3 + 4 d4 + 16 d0 (sr_fft_layout.h): register v[d1][d2] is plane
// d1 + 4 d2 of the image, stored lane-contiguously at word 68 p + lane by ds_write_addtid_b32 (address = M0 + offset + 4 lane;
// `base` = LDS byte address of buf, wave-uniform), and the reading lane's sixteen words u[e3][e4] are consecutive: four
// ds_read_b128.  M0, the in-order completion of the wave's LDS operations and what the compiler knows of both: see
// mel_prefix_store in k_mfcc.hip, the statement this one is modelled on.  EXEC is all ones wherever a frame is transformed.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void fft_exchange_tid(const uint32_t *buf, uint32_t base, int lane, const uint32_t (&v)[4][4], uint32_t (&u)[4][4])
{
    static_assert(4 * kXchgPlane == 272 && xchg_plane(1, 0) == 1 && xchg_plane(0, 1) == 4, "the offsets below are written out for planes d1 + 4 d2 of 68 words");
    asm volatile("s_mov_b32 m0, %16\n\ts_nop 0\n\t"
                 "ds_write_addtid_b32 %0\n\tds_write_addtid_b32 %1 offset:272\n\tds_write_addtid_b32 %2 offset:544\n\t"
                 "ds_write_addtid_b32 %3 offset:816\n\tds_write_addtid_b32 %4 offset:1088\n\tds_write_addtid_b32 %5 offset:1360\n\t"
                 "ds_write_addtid_b32 %6 offset:1632\n\tds_write_addtid_b32 %7 offset:1904\n\t"
                 "ds_write_addtid_b32 %8 offset:2176\n\tds_write_addtid_b32 %9 offset:2448\n\tds_write_addtid_b32 %10 offset:2720\n\t"
                 "ds_write_addtid_b32 %11 offset:2992\n\tds_write_addtid_b32 %12 offset:3264\n\tds_write_addtid_b32 %13 offset:3536\n\t"
                 "ds_write_addtid_b32 %14 offset:3808\n\tds_write_addtid_b32 %15 offset:4080"
                 :
                 : "v"(v[0][0]), "v"(v[1][0]), "v"(v[2][0]), "v"(v[3][0]), "v"(v[0][1]), "v"(v[1][1]), "v"(v[2][1]), "v"(v[3][1]),
                   "v"(v[0][2]), "v"(v[1][2]), "v"(v[2][2]), "v"(v[3][2]), "v"(v[0][3]), "v"(v[1][3]), "v"(v[2][3]), "v"(v[3][3]), "s"(base)
                 : "m0", "memory");
    wave_sync();
    const u32x4 *rd = (const u32x4 *)(buf + xchg_read_base(lane));
#pragma unroll
    for (int e4 = 0; e4 < 4; e4++) {
        const u32x4 q = rd[e4];
        u[0][e4] = q.x;
        u[1][e4] = q.y;
        u[2][e4] = q.z;
        u[3][e4] = q.w;
    }
}
#pragma clang diagnostic pop

// Pass-4 butterfly e4 behind fft_front_real160 + fft_exchange: its B, C and D legs u[1..3][e4] arrive doubled (written by the lanes
// with d3 > 0).  Its outputs u[.][e4] are all leg e4 of pass 5, which takes only its B leg doubled (its HALF form needs p() of B
// alone: doubling C and D there would turn their single v_perm_b32 into two instructions) -- so butterfly e4 = 1 emits doubled.
__device__ __forceinline__ void fft_pass4_dbl(uint32_t (&u)[4][4], int e4, const LaneTw &tw)
{
    if (e4 == 1)
        bfly_pk_dbl<false, true, 1>(u[0][e4], u[1][e4], u[2][e4], u[3][e4], tw.s4[0][0], tw.s4[0][1], tw.s4[1][0], tw.s4[1][1],
                                    tw.s4[2][0], tw.s4[2][1], tw.s4[3][0], tw.s4[3][1]);
    else
        bfly_pk_dbl<false, true, 0>(u[0][e4], u[1][e4], u[2][e4], u[3][e4], tw.s4[0][0], tw.s4[0][1], tw.s4[1][0], tw.s4[1][1],
                                    tw.s4[2][0], tw.s4[2][1], tw.s4[3][0], tw.s4[3][1]);
}

// ---- the full complex transform, one wave per array (used by the generic kernels: k_fft.hip, k_mfcc_gen.hip) ----
__device__ __forceinline__ int bitrev8(int v) { return (int)(__brev((uint32_t)v) >> 24); }

// Full-complex passes 1-5, result in natural order in `out` (global).  in/out may not alias in LDS terms.
__device__ inline void fft_full_wave(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t *buf, int lane,
                              const DevTables &t)
{
    // pass 1 (.s:226-232): 256 butterflies, 4 per lane, bit-reversed gather, legs 256 words apart
    // loaded in the order A, C, B, D (.s:134-145); outputs to buf[4*idx + k]
    for (int m = 0; m < 4; m++) {
        const int idx = lane + 64 * m, r = bitrev8(idx);
        const uint32_t wa = in[r], wc = in[r + 256], wb = in[r + 512], wd = in[r + 768];
        int ar = sext_lo(wa), ai = sext_hi(wa), br = sext_lo(wb), bi = sext_hi(wb);
        int cr = sext_lo(wc), ci = sext_hi(wc), dr = sext_lo(wd), di = sext_hi(wd);
        r4_combine<0>(ar, ai, br, bi, cr, ci, dr, di);
        buf[xaddr(4 * idx + 0)] = pack16(ar, ai);
        buf[xaddr(4 * idx + 1)] = pack16(br, bi);
        buf[xaddr(4 * idx + 2)] = pack16(cr, ci);
        buf[xaddr(4 * idx + 3)] = pack16(di, dr);
    }
    wave_sync();
    LaneTw tw;
    load_lane_tw(t, lane, lane & 3, tw);
    uint32_t k2[3][2];
    load_tw3(t, 0, lane & 3, k2);
    const int d0 = lane & 3, d3 = (lane >> 2) & 3, d4 = lane >> 4;
    uint32_t v[4][4], u[4][4];
#pragma unroll
    for (int d1 = 0; d1 < 4; d1++)
#pragma unroll
        for (int d2 = 0; d2 < 4; d2++) v[d1][d2] = buf[xaddr(d0 + 4 * d1 + 16 * d2 + 64 * d3 + 256 * d4)];
    wave_sync();
#pragma unroll
    for (int d2 = 0; d2 < 4; d2++)
        bfly(v[0][d2], v[1][d2], v[2][d2], v[3][d2], k2[0][0], k2[0][1], k2[1][0], k2[1][1], k2[2][0], k2[2][1]);
#pragma unroll
    for (int d1 = 0; d1 < 4; d1++)
        bfly(v[d1][0], v[d1][1], v[d1][2], v[d1][3], tw.s3[d1][0][0], tw.s3[d1][0][1], tw.s3[d1][1][0],
             tw.s3[d1][1][1], tw.s3[d1][2][0], tw.s3[d1][2][1]);
    fft_exchange(buf, lane, v, u);
#pragma unroll
    for (int e4 = 0; e4 < 4; e4++)
        bfly(u[0][e4], u[1][e4], u[2][e4], u[3][e4], tw.s4[0][0], tw.s4[0][1], tw.s4[1][0], tw.s4[1][1], tw.s4[2][0],
             tw.s4[2][1]);
#pragma unroll
    for (int e3 = 0; e3 < 4; e3++) {
        bfly(u[e3][0], u[e3][1], u[e3][2], u[e3][3], tw.s5[e3][0][0], tw.s5[e3][0][1], tw.s5[e3][1][0],
             tw.s5[e3][1][1], tw.s5[e3][2][0], tw.s5[e3][2][1]);
#pragma unroll
        for (int e4 = 0; e4 < 4; e4++) out[lane + 64 * e3 + 256 * e4] = u[e3][e4];
    }
}

}  // namespace sr
