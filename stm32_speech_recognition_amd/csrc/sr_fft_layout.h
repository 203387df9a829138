// sr_fft_layout.h -- where the words of k_mfcc's two transposing LDS images lie, and the bank model that says what reading them
// costs.  Plain constexpr C++ with no HIP in it: the kernel (sr_fft_dev.h, k_mfcc.hip) and the host check
// (tests/fft_layout/layout_check.cpp) take their addresses from the same functions, and the static_asserts at the end hold
// for every build of either.
//
// Both images are written by lane-contiguous stores (ds_write_addtid_b32: word = plane base + lane, no address register) and
// read as 16-byte words (ds_read_b128), so the transposition is done by WHICH lane holds WHAT, not by the addresses:
//   exchange between passes 3 and 4   front lane = d3 + 4 d4 + 16 d0 holds v[d1][d2] = x[d0 + 4 d1 + 16 d2 + 64 d3 + 256 d4];
//                                     plane p = d1 + 4 d2 lies at word 68 p + lane.  The reading lane l' = j & 63
//                                     = d0 + 4 d1 + 16 d2 wants u[e3][e4] = x[l' + 64 e3 + 256 e4]: plane l' >> 2, front lanes
//                                     16 (l' & 3) + e3 + 4 e4 -- sixteen consecutive words, four 16-byte reads.
//   energies -> filterbank            magnitude lane l' holds bins l' + 64 e3 + 256 half; plane q = e3 + 4 half lies at word
//                                     energy_plane(q) + l', so bin b is at energy_plane(b >> 6) + (b & 63) and filter lane l
//                                     reads its bins 8 l .. 8 l + 7 as two 16-byte words.
// The plane bases (stride 68; 64 q + 4 ((q + 2) >> 2)) are what keeps the 16-lane service groups of ds_read_b128 off each
// other's banks: b128_extra_cycles below is that model, and it reports the conflicts of the plain strides.
#pragma once

namespace sr {

constexpr int kXchgWords = 1024 + 4 * 16;  // 1088: the wave's exchange area (either image of the work array fits)

// ---- exchange image ---------------------------------------------------------------------------------------------------------
constexpr int kXchgPlane = 68;  // words between planes
constexpr int xchg_front_lane(int d0, int d3, int d4) { return d3 + 4 * d4 + 16 * d0; }
// element of the 1024-point work array that front lane `lane` holds in v[d1][d2]
constexpr int xchg_front_elem(int lane, int d1, int d2) { return (lane >> 4) + 4 * d1 + 16 * d2 + 64 * (lane & 3) + 256 * ((lane >> 2) & 3); }
constexpr int xchg_plane(int d1, int d2) { return d1 + 4 * d2; }
constexpr int xchg_store_word(int lane, int d1, int d2) { return kXchgPlane * xchg_plane(d1, d2) + lane; }
// first of the sixteen words of reading lane rl; word e3 + 4 e4 of them is u[e3][e4] = x[rl + 64 e3 + 256 e4]
constexpr int xchg_read_base(int rl, int plane_stride = kXchgPlane) { return plane_stride * (rl >> 2) + 16 * (rl & 3); }
constexpr int xchg_read_word(int rl, int e3, int e4) { return xchg_read_base(rl) + e3 + 4 * e4; }
constexpr int kXchgImageWords = xchg_store_word(63, 3, 3) + 1;  // 1084

// ---- energies image ---------------------------------------------------------------------------------------------------------
constexpr int kEnergyBins = 512;
constexpr int energy_plane(int q) { return 64 * q + 4 * ((q + 2) >> 2); }  // 0, 64, 132, 196, 260, 324, 392, 456
constexpr int energy_store_word(int lane, int e3, int half) { return energy_plane(e3 + 4 * half) + lane; }
constexpr int energy_word(int bin) { return energy_plane(bin >> 6) + (bin & 63); }
// first word of filter lane l's bins 8 l .. 8 l + 7: two 16-byte reads, at this word and 4 further on
constexpr int energy_read_base(int l, int plane_stride = 0) { return (plane_stride ? plane_stride * (l >> 3) : energy_plane(l >> 3)) + 8 * (l & 7); }
constexpr int kEnergyImageWords = energy_word(kEnergyBins - 1) + 1;  // 520

// ---- bank model of ds_read_b128 ---------------------------------------------------------------------------------------------
// A wave's 16-byte read is served in four groups of sixteen lanes, one LDS cycle each: {0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} and the same of the upper half.  The bank of a word is its address mod 64.  Lanes of one group that
// touch a bank at different addresses take one more cycle per further address (equal addresses broadcast).
constexpr int b128_group(int lane)
{
    const int l = lane & 31;
    return ((l < 4 || (l >= 12 && l < 16) || (l >= 20 && l < 28)) ? 0 : 1) + 2 * (lane >> 5);
}
// extra cycles of one ds_read_b128 whose lane l reads the four words from word_of_lane(l) on
template <class F>
constexpr int b128_extra_cycles(F word_of_lane)
{
    int extra = 0;
    for (int g = 0; g < 4; g++) {
        int first[16] = {}, lanes = 0, worst = 1;
        for (int lane = 0; lane < 64; lane++)
            if (b128_group(lane) == g) first[lanes++] = word_of_lane(lane);
        for (int bank = 0; bank < 64; bank++) {
            int seen[16] = {}, n = 0;  // distinct first words among the group's lanes that touch this bank
            for (int k = 0; k < lanes; k++) {
                const int a = first[k];
                if (((bank - a) & 63) >= 4) continue;
                bool known = false;
                for (int i = 0; i < n; i++) known = known || seen[i] == a;
                if (!known) seen[n++] = a;
            }
            if (n > worst) worst = n;
        }
        extra += worst - 1;
    }
    return extra;
}
constexpr int xchg_read_extra_cycles(int e4, int plane_stride = kXchgPlane)
{
    return b128_extra_cycles([=](int lane) { return xchg_read_base(lane, plane_stride) + 4 * e4; });
}
constexpr int energy_read_extra_cycles(int second, int plane_stride = 0)
{
    return b128_extra_cycles([=](int lane) { return energy_read_base(lane, plane_stride) + 4 * second; });
}

// ---- the images are consistent: every word written once, found by its reader, inside its area ------------------------------
constexpr bool xchg_image_consistent()
{
    bool elem[1024] = {}, word[kXchgWords] = {};
    for (int lane = 0; lane < 64; lane++)
        for (int d1 = 0; d1 < 4; d1++)
            for (int d2 = 0; d2 < 4; d2++) {
                const int j = xchg_front_elem(lane, d1, d2), at = xchg_store_word(lane, d1, d2);
                if (j < 0 || j >= 1024 || at < 0 || at >= kXchgWords || elem[j] || word[at]) return false;
                elem[j] = word[at] = true;
                if (xchg_read_word(j & 63, (j >> 6) & 3, j >> 8) != at) return false;
                if (xchg_front_lane(j & 3, (j >> 6) & 3, j >> 8) != lane) return false;
            }
    return true;  // (64 x 16 distinct elements of 1024: all of them)
}
constexpr bool energy_image_consistent()
{
    bool word[kEnergyImageWords] = {};
    for (int b = 0; b < kEnergyBins; b++) {
        const int at = energy_store_word(b & 63, (b >> 6) & 3, b >> 8);
        if (at < 0 || at >= kEnergyImageWords || word[at]) return false;
        word[at] = true;
        if (energy_word(b) != at || energy_read_base(b >> 3) + (b & 7) != at) return false;
    }
    return true;
}
static_assert(xchg_image_consistent() && kXchgImageWords <= kXchgWords, "exchange image");
static_assert(energy_image_consistent() && kEnergyImageWords <= kXchgWords, "energies image");
static_assert(xchg_read_base(63) % 4 == 0 && kXchgPlane % 4 == 0 && energy_read_base(63) % 4 == 0 && energy_plane(7) % 4 == 0, "16-byte reads are aligned");
static_assert(xchg_read_extra_cycles(0) == 0 && xchg_read_extra_cycles(1) == 0 && xchg_read_extra_cycles(2) == 0 && xchg_read_extra_cycles(3) == 0,
              "exchange reads are conflict-free");
static_assert(energy_read_extra_cycles(0) == 0 && energy_read_extra_cycles(1) == 0, "energy reads are conflict-free");
static_assert(xchg_read_extra_cycles(0, 64) == 12 && xchg_read_extra_cycles(0, 72) == 4 && energy_read_extra_cycles(0, 64) > 0,
              "the model sees the conflicts of the plain strides");

}  // namespace sr
