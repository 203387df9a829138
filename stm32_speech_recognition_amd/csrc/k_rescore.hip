// k_rescore.hip -- two-pass recognition, the mark pass (include/sr_engine.h, "second pass: full-DP rescoring of the N-best
// words").  EXTENSION, no reference counterpart.  The first pass left n_best candidate entries per row; the second pass scores
// every slot of every candidate WORD with the full-DP scorer (k_dtw_dp.hip, sparse forms) and reduces those scores with
// k_nbest.  This kernel turns the lists into the pair set the sparse scorer reads.
// gfx950 (MI355X, CDNA4) only; wave = 64 lanes; integer VALU, no LDS, no atomics.
#include "sr_device.h"

namespace sr {

// One thread per input entry.  An entry counts when word != SR_NO_WORD and slot < K; its candidate is the word group the SLOT
// belongs to (the word field is not trusted any further).  Every slot of that group gets its mark, one byte at
// marks[rank of the slot][row]: a template's marks are contiguous in the row, which is how the sparse scorer's workgroups (one
// template, a range of rows) read them.  A word named twice stores the same bytes twice: no duplicate search, no atomics.
__global__ void __launch_bounds__(256) k_rescore_mark(const RescoreMarkArgs a)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;  // (n_rows * n_best < 2^32: sr_rescore_nbest_dp_dev's row limit)
    if (i >= a.n_rows * a.n_best) return;
    const sr_nbest_entry e = a.in[i];
    if (e.word == SR_NO_WORD || e.slot >= a.K) return;
    const uint32_t row = i / a.n_best, g = a.group_of_slot[e.slot];
    const uint32_t p1 = a.group_start[g + 1];
    for (uint32_t p = a.group_start[g]; p < p1; p++) a.marks[(size_t)a.tpl_rank[a.order[p]] * a.mark_stride + row] = 1;
}

void launch_rescore_mark(const RescoreMarkArgs &a, hipStream_t s)
{
    const uint64_t n = (uint64_t)a.n_rows * a.n_best;
    if (!n) return;
    SR_LAUNCH_POINT(s, "k_rescore_mark");
    hipLaunchKernelGGL(k_rescore_mark, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace sr
