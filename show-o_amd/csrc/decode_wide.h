// Wide decode batches (decode_wide.hip): the two MFMA skinny GEMMs of a decode step with 1..32 rows, and their workspace.
#pragma once
#include "decode_common.h"

namespace showo {

// Per-stream workspace of the wide step: the normalised bf16 rows, the split-K partials of the out GEMM and its ticket words
// (zero between launches).  Launches that share one must be ordered on one stream.
struct WideWs {
    bf16_t* hn = nullptr;     // [32, H]
    float4* part = nullptr;   // [splits <= 8][column groups][256] fragments
    unsigned* tick = nullptr; // [column groups]
    int64_t hn_elems = 0;
    int groups = 0;
};
int wide_ws_reserve(WideWs* w, int H, int N);  // grows for hidden size H and N output columns of the out GEMM (synchronises when it grows)
void wide_ws_free(WideWs* w);

// LnGemvBArgs / OutGemvBArgs as ln_gemvB / out_gemvB take them (bf16 weights, no scales); nb = 1..32 rows
int ln_gemmW(int nb, const LnGemvBArgs& g, const WideWs& w, hipStream_t s);
int out_gemmW(int nb, const OutGemvBArgs& g, const WideWs& w, hipStream_t s);

}  // namespace showo
