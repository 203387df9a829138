// gather_rate.hip -- what a 64-lane 2-byte table gather costs a CU's vector-memory path when the frame kernel's occupancy
// and issue pressure are around it: the measurement behind k_mfcc's QUIET-tier magnitude table (RESULTS.md, round 7).
//   hipcc --offload-arch=gfx950 -O2 -o gather_rate gather_rate.hip
//   python profiles/experiments/gather_idx_dump.py /tmp/gather_idx.bin     (real indices: re^2 + im^2 of headline frames)
//   ./gather_rate /tmp/gather_idx.bin
// 16 waves per CU on every CU (4 workgroups of 4 waves, like k_mfcc).  A wave works through "frames": per frame it fetches its
// eight indices n = re^2 + im^2 in the frame kernel's lane order (bins lane + 64 e3, + 256; four coalesced dwords of two u16
// each, n > 65 535 stored as 65 535 = past the table like the real thing), issues eight buffer_load_ushort into the 26 844-entry
// table, runs `fill` blocks of eight dependent-free v_mad_u32_u24 (470 VALU per frame = the frame kernel's issue load, so that
// a frame takes about 8 300 cycles with four waves per SIMD), then squares and sums the eight values.
// Forms: 0 = no gathers (the filler and the index loads alone), 1 = raw buffer, byte offset 2 n in a VGPR (one v_lshlrev per
// gather), 2 = indexed (idxen, stride 2 in the descriptor, num_records in elements: no address arithmetic on the VALU).
// Reported per form and fill: kernel time, shader cycles per frame and wave (s_memtime), and the difference to form 0 per gather.
// The sums of all forms must agree with the host's (form 2 doubles as the check that the indexed form's range check counts
// elements).  Counters (texture-addresser busy, L1 hits) come from a rocprofv3 --pmc run of this program, on its own.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

constexpr uint32_t kEntries = 26844;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int kForm>
__global__ void __launch_bounds__(256) gather(const uint16_t *tab, const uint32_t *idx, uint32_t n_frames, uint32_t frames_per_wave,
                                              int fill, unsigned long long *sums, unsigned long long *cycles)
{
    const uint32_t lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t p = (uint64_t)tab;
    // V# of the table: raw (stride 0, range in bytes) or structured (stride 2, range in elements)
    const u32x4 rs = {(uint32_t)p, (uint32_t)(p >> 32) | (kForm == 2 ? 2u << 16 : 0u), kForm == 2 ? kEntries : 2 * kEntries, 0x00027000u};
    uint32_t f = (uint32_t)(((uint64_t)wave * frames_per_wave) % n_frames);
    uint32_t a0 = lane, a1 = lane + 1, a2 = lane + 2, a3 = lane + 3, a4 = lane + 4, a5 = lane + 5, a6 = lane + 6, a7 = lane + 7;
    unsigned long long sum = 0;
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (uint32_t r = 0; r < frames_per_wave; r++) {
        const u32x4 q = *(const u32x4 *)(idx + ((uint64_t)f * 64 + lane) * 4);  // pair e3: bin lane + 64 e3 low half, + 256 high half
        if (++f == n_frames) f = 0;
        uint32_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (kForm != 0) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint32_t n = (j & 1) ? q[j >> 1] >> 16 : q[j >> 1] & 0xFFFFu;
                if (kForm == 1) {
                    const uint32_t off = n << 1;
                    asm volatile("buffer_load_ushort %0, %1, %2, 0 offen" : "=v"(t[j]) : "v"(off), "s"(rs));
                } else {
                    asm volatile("buffer_load_ushort %0, %1, %2, 0 idxen" : "=v"(t[j]) : "v"(n), "s"(rs));
                }
            }
        } else {
            sum += q[0] + q[1] + q[2] + q[3];
        }
        for (int i = 0; i < fill; i++)
            asm volatile("v_mad_u32_u24 %0, %0, %8, %9\n\tv_mad_u32_u24 %1, %1, %8, %9\n\tv_mad_u32_u24 %2, %2, %8, %9\n\t"
                         "v_mad_u32_u24 %3, %3, %8, %9\n\tv_mad_u32_u24 %4, %4, %8, %9\n\tv_mad_u32_u24 %5, %5, %8, %9\n\t"
                         "v_mad_u32_u24 %6, %6, %8, %9\n\tv_mad_u32_u24 %7, %7, %8, %9"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                         : "v"(lane | 3u), "v"(r));
        if (kForm != 0) {
            // (loads issued from inline assembly are not counted by the compiler: wait for them here, with the values tied in)
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]));
#pragma unroll
            for (int j = 0; j < 8; j++) sum += (unsigned long long)(t[j] * t[j]);
        }
    }
    const unsigned long long t1 = __builtin_readcyclecounter();
    sum += (a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7) == 0x12345678u;  // keeps the filler alive
    sums[(uint64_t)wave * 64 + lane] = sum;
    if (lane == 0) cycles[wave] = t1 - t0;
}

#define CK(x)                                                                          \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                    \
            return 2;                                                                  \
        }                                                                              \
    } while (0)

int main(int argc, char **argv)
{
    // indices: u32 header n_frames, then n_frames x 64 lanes x 4 dwords (two u16 each)
    std::vector<uint32_t> idx;
    uint32_t n_frames = 0;
    if (argc > 1) {
        FILE *fp = fopen(argv[1], "rb");
        if (!fp || fread(&n_frames, 4, 1, fp) != 1 || n_frames == 0 || n_frames > (1u << 20)) {
            fprintf(stderr, "cannot read %s\n", argv[1]);
            return 2;
        }
        idx.resize((size_t)n_frames * 256);
        if (fread(idx.data(), 4, idx.size(), fp) != idx.size()) {
            fprintf(stderr, "short index file\n");
            return 2;
        }
        fclose(fp);
    } else {  // no file: a stand-in with the same shape (most bins small, a few per cent of the frames past the table)
        n_frames = 4096;
        idx.resize((size_t)n_frames * 256);
        uint32_t s = 12345;
        for (auto &w : idx) {
            uint32_t h[2];
            for (int k = 0; k < 2; k++) {
                s = s * 1664525u + 1013904223u;
                const uint32_t u = s >> 8;
                h[k] = (u & 0xFF) < 200 ? (u >> 8) % 300 : (u & 0xFF) < 250 ? (u >> 8) % 8000 : (u >> 8) % 65536;
            }
            w = h[0] | h[1] << 16;
        }
        printf("no index file given: synthetic indices\n");
    }
    std::vector<uint16_t> tab(kEntries);
    for (uint32_t n = 0; n < kEntries; n++) tab[n] = (uint16_t)(((uint32_t)(sqrtf((float)n) * 10.0f)) << 2);
    {  // what the indices look like: share past the table, distinct 128-byte lines (64 entries) per gather
        uint64_t past = 0, lines = 0, total = 0;
        for (uint32_t f = 0; f < n_frames; f++)
            for (int j = 0; j < 8; j++) {
                bool seen[1024] = {false};
                for (int l = 0; l < 64; l++) {
                    const uint32_t w = idx[((size_t)f * 64 + l) * 4 + (j >> 1)], n = (j & 1) ? w >> 16 : w & 0xFFFF;
                    total++;
                    if (n >= kEntries) {
                        past++;
                        continue;
                    }
                    if (!seen[n >> 6]) seen[n >> 6] = true, lines++;
                }
            }
        printf("%u frames, %.2f %% of the indices past the table, %.1f distinct 128-byte lines per 64-lane gather\n", n_frames,
               100.0 * past / total, (double)lines / (n_frames * 8.0));
    }
    int dev = 0, n_cu = 0, khz = 0;
    CK(hipGetDevice(&dev));
    CK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    CK(hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, dev));
    const uint32_t wgs = 4 * n_cu, waves = 4 * wgs, fpw = 2048;
    uint16_t *d_tab;
    uint32_t *d_idx;
    unsigned long long *d_sum, *d_cyc;
    CK(hipMalloc(&d_tab, 128 * 1024));  // (room behind the table: a range check in the wrong unit would still read inside the allocation)
    CK(hipMemset(d_tab, 0, 128 * 1024));
    CK(hipMemcpy(d_tab, tab.data(), kEntries * 2, hipMemcpyHostToDevice));
    CK(hipMalloc(&d_idx, idx.size() * 4));
    CK(hipMemcpy(d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&d_sum, (size_t)waves * 64 * 8));
    CK(hipMalloc(&d_cyc, (size_t)waves * 8));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::vector<unsigned long long> h_sum((size_t)waves * 64), h_cyc(waves);
    // the host's sums of t^2 per wave and lane
    std::vector<unsigned long long> want((size_t)waves * 64, 0);
    for (uint32_t w = 0; w < waves; w++) {
        uint32_t f = (uint32_t)(((uint64_t)w * fpw) % n_frames);
        for (uint32_t r = 0; r < fpw; r++) {
            for (int l = 0; l < 64; l++)
                for (int j = 0; j < 8; j++) {
                    const uint32_t q = idx[((size_t)f * 64 + l) * 4 + (j >> 1)], n = (j & 1) ? q >> 16 : q & 0xFFFF;
                    const uint32_t t = n < kEntries ? tab[n] : 0;
                    want[(size_t)w * 64 + l] += (unsigned long long)(t * t);
                }
            if (++f == n_frames) f = 0;
        }
    }
    printf("%d CUs, %u workgroups x 4 waves, %u frames per wave, 8 gathers per frame\n", n_cu, wgs, fpw);
    double base_ms[2] = {0, 0}, base_cyc[2] = {0, 0};
    const int fills[2] = {0, 59};  // 59 x 8 = 472 VALU per frame
    for (int fi = 0; fi < 2; fi++)
        for (int form = 0; form < 3; form++) {
            float ms = 0;
            for (int rep = 0; rep < 2; rep++) {  // (the first launch warms the caches and the clocks)
                CK(hipEventRecord(e0));
                if (form == 0) gather<0><<<wgs, 256>>>(d_tab, d_idx, n_frames, fpw, fills[fi], d_sum, d_cyc);
                if (form == 1) gather<1><<<wgs, 256>>>(d_tab, d_idx, n_frames, fpw, fills[fi], d_sum, d_cyc);
                if (form == 2) gather<2><<<wgs, 256>>>(d_tab, d_idx, n_frames, fpw, fills[fi], d_sum, d_cyc);
                CK(hipEventRecord(e1));
                CK(hipEventSynchronize(e1));
                CK(hipGetLastError());
                CK(hipEventElapsedTime(&ms, e0, e1));
            }
            CK(hipMemcpy(h_sum.data(), d_sum, h_sum.size() * 8, hipMemcpyDeviceToHost));
            CK(hipMemcpy(h_cyc.data(), d_cyc, h_cyc.size() * 8, hipMemcpyDeviceToHost));
            double cyc = 0;
            for (auto c : h_cyc) cyc += (double)c;
            cyc /= (double)waves * fpw;  // counter ticks per frame and wave
            size_t bad = 0;
            if (form != 0)
                for (size_t i = 0; i < want.size(); i++) bad += h_sum[i] != want[i];
            // per-CU time per frame slot: 16 waves x 8 gathers share one texture path
            const double us_frame = ms * 1e3 / fpw;
            printf("fill %2d form %d (%s): %8.3f ms, %7.3f us per frame and wave, %9.1f counter ticks per frame", fills[fi], form,
                   form == 0 ? "no gather" : form == 1 ? "raw offen" : "idxen    ", ms, us_frame, cyc);
            if (form == 0) {
                base_ms[fi] = ms;
                base_cyc[fi] = cyc;
                printf("\n");
            } else {
                // extra time of the whole CU per gather instruction: (ms - base) / (frames x 16 waves x 8) in ns, and in shader cycles
                // at the reported clock
                const double ns = (ms - base_ms[fi]) * 1e6 / ((double)fpw * 16 * 8);
                printf(", +%.2f ns = +%.1f cycles (at %d MHz) of CU time per gather, sums %s (%zu differ)\n", ns, ns * khz / 1e6, khz / 1000,
                       bad ? "WRONG" : "ok", bad);
            }
            (void)base_cyc;
        }
    return 0;
}
