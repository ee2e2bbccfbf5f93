// Shared-prefix decode attention (attn_shared.hip): the per-layer launches of a wide batch whose slots keep only a suffix cache.
#pragma once
#include "common.h"

namespace showo {
struct SharedAttnArgs {
    const bf16_t* qkv;  // [nb, 3 nH 64] projection rows of the new tokens
    const float *qw, *qb, *kw, *kb, *cosT, *sinT;
    const bf16_t *Kp, *Vp;  // one layer of the prefix cache: [nH, cap_pre, 64] / [nH, 64, cap_pre]
    int cap_pre;
    bf16_t *Ks, *Vs;  // one layer of the suffix caches: [nb][nH][cap_suf][64] / [nb][nH][64][cap_suf]
    int cap_suf;
    int lo1, hi1, lo2, hi2;  // what every new row sees of the prefix (clipped to [0, P) by the launcher)
    int P, base;             // prefix length; base = P & ~63: key k >= P lives at row / column k - base of a suffix cache
    const int* pos_dev;      // [nb] absolute positions of the new tokens.  Host invariant: P <= pos < base + cap_suf (and < lk_max when
                             // given) for every slot; a slot outside it gets a NaN output row and neither appends nor reads anything
    int lk_max;              // upper bound of pos + 1 over the replays of a captured step (0: base + cap_suf)
    bf16_t* O;               // [nb, nH 64]
    float* ws;               // shared_attn_ws_elems(nH, P) floats: (m, l, o[64]) per (split, head, slot)
    int nb, nH, rot;
    float eps;
};
int64_t shared_attn_ws_elems(int nH, int P);
int attn_decode_shared(SharedAttnArgs a, hipStream_t s);  // the prefix launch and the suffix + merge launch
}  // namespace showo
