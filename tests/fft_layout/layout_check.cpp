// The two transposing LDS images of k_mfcc (csrc/sr_fft_layout.h) on the CPU, at run time: the images are SIMULATED -- every
// front lane stores its sixteen registers, every magnitude lane its eight energies, into an array the size of the wave's
// area, and the readers fetch their words from it by the reader formulas -- instead of only comparing formulas, and the bank
// model is restated here lane by lane and compared with the header's.  A stand-alone program for the sanitizers:
//   hipcc --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I<csrc> layout_check.cpp -o layout_check && ./layout_check
// (tests/test_mfcc_exchange_image.py builds and runs it).  Prints "layout_check ok" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <set>
#include <vector>

#include "sr_fft_layout.h"

using namespace sr;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("layout_check: line %d: %s\n", __LINE__, #cond);     \
            return 1;                                                        \
        }                                                                    \
    } while (0)

// the guide's service groups of ds_read_b128, written out
static const int kGroups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                   {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                   {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                   {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

// extra cycles of a 16-byte read, lane l at word first[l]: per group, the most distinct addresses that meet on one bank, less one
static int extra_cycles(const int (&first)[64])
{
    int extra = 0;
    for (const auto &g : kGroups) {
        size_t worst = 1;
        for (int bank = 0; bank < 64; bank++) {
            std::set<int> at;
            for (int l : g)
                for (int i = 0; i < 4; i++)
                    if (((first[l] + i) & 63) == bank) at.insert(first[l]);
            if (at.size() > worst) worst = at.size();
        }
        extra += (int)worst - 1;
    }
    return extra;
}

static int exchange()
{
    std::vector<int> area(kXchgWords, -1);  // element number held by each word
    std::vector<int> writers(1024, 0);
    for (int lane = 0; lane < 64; lane++)
        for (int d1 = 0; d1 < 4; d1++)
            for (int d2 = 0; d2 < 4; d2++) {
                const int d0 = lane >> 4, d3 = lane & 3, d4 = (lane >> 2) & 3;
                CHECK(xchg_front_lane(d0, d3, d4) == lane);
                const int j = d0 + 4 * d1 + 16 * d2 + 64 * d3 + 256 * d4;
                CHECK(xchg_front_elem(lane, d1, d2) == j);
                const int at = xchg_store_word(lane, d1, d2);
                CHECK(at >= 0 && at < kXchgWords && at < kXchgImageWords);
                CHECK(at == 68 * (d1 + 4 * d2) + lane);
                CHECK(area.at(at) == -1);  // no two elements share a word
                area.at(at) = j;
                writers.at(j)++;
            }
    for (int j = 0; j < 1024; j++) CHECK(writers[j] == 1);  // every element is written by exactly one (lane, register)
    // the reader: lane rl = j & 63 finds u[e3][e4] = x[rl + 64 e3 + 256 e4] in its sixteen consecutive, 16-byte aligned words
    for (int rl = 0; rl < 64; rl++) {
        CHECK(xchg_read_base(rl) % 4 == 0);
        for (int e3 = 0; e3 < 4; e3++)
            for (int e4 = 0; e4 < 4; e4++) {
                CHECK(xchg_read_word(rl, e3, e4) == xchg_read_base(rl) + e3 + 4 * e4);
                CHECK(area.at(xchg_read_word(rl, e3, e4)) == rl + 64 * e3 + 256 * e4);
            }
    }
    for (int e4 = 0; e4 < 4; e4++) {
        int first[64], plain[64], wide[64];
        for (int l = 0; l < 64; l++) {
            first[l] = xchg_read_base(l) + 4 * e4;
            plain[l] = xchg_read_base(l, 64) + 4 * e4;
            wide[l] = xchg_read_base(l, 72) + 4 * e4;
        }
        CHECK(extra_cycles(first) == 0 && xchg_read_extra_cycles(e4) == 0);
        // the model itself: the plain stride is a four-way conflict in every group, and the header's model agrees with this one
        CHECK(extra_cycles(plain) == 12 && xchg_read_extra_cycles(e4, 64) == 12);
        CHECK(extra_cycles(wide) == 4 && xchg_read_extra_cycles(e4, 72) == 4);
    }
    return 0;
}

static int energies()
{
    std::vector<int> area(kXchgWords, -1);  // bin number held by each word
    for (int lane = 0; lane < 64; lane++)
        for (int e3 = 0; e3 < 4; e3++)
            for (int half = 0; half < 2; half++) {
                const int at = energy_store_word(lane, e3, half);
                CHECK(at >= 0 && at < kEnergyImageWords && kEnergyImageWords <= kXchgWords);
                CHECK(area.at(at) == -1);
                area.at(at) = lane + 64 * e3 + 256 * half;
            }
    // every bin 0..511 is found by its filter lane l = bin >> 3, in the two 16-byte words from energy_read_base(l) on
    for (int b = 0; b < kEnergyBins; b++) {
        CHECK(energy_read_base(b >> 3) % 4 == 0);
        CHECK(area.at(energy_read_base(b >> 3) + (b & 7)) == b);
        CHECK(energy_word(b) == energy_read_base(b >> 3) + (b & 7));
    }
    for (int second = 0; second < 2; second++) {
        int first[64], plain[64];
        for (int l = 0; l < 64; l++) {
            first[l] = energy_read_base(l) + 4 * second;
            plain[l] = energy_read_base(l, 64) + 4 * second;
        }
        CHECK(extra_cycles(first) == 0 && energy_read_extra_cycles(second) == 0);
        CHECK(extra_cycles(plain) > 0 && energy_read_extra_cycles(second, 64) == extra_cycles(plain));
    }
    return 0;
}

int main()
{
    for (int g = 0; g < 4; g++)
        for (int l : kGroups[g]) CHECK(b128_group(l) == g);
    if (exchange() || energies()) return 1;
    std::printf("layout_check ok\n");
    return 0;
}
