// Batched AR decode: NB independent sequences (BASELINE cfg4: "batch=4 images"), NB KV caches, ONE weight stream per token step.
//
// Reference: inference_mmu.py:87-177 walks the images one by one and Showo.mmu_generate (models/modeling_showo.py:183-240) is batch-1;
// a decode step is weight-streaming bound (2.66 GB of bf16 weights per token), so serving the NB sequences of a
// batch together reads every weight byte once per STEP instead of once per token.  The GEMVs become M = NB skinny GEMMs:
//
//   ln_gemvB_kernel<NB>   x [NB, H] -> LayerNorm (all NB rows in every block's LDS) -> qkv [NB, 3H] (bf16) and gelu(fc1) [NB, F] (bf16)
//   attn_decode_kernel<FUSED> (attention.hip), grid (heads, NB): prep + cache append + single-query attention, per-sequence position
//   out_gemvB_kernel<C, NB>  x[b] = (x[b] + (dense(attn[b]) + bd)) + (fc2(ffn[b]) + b2)
//   ln_gemvB_kernel<NB>   final LayerNorm + lm_head -> logits [NB, V] (fp32)
//   greedy_seam_rows_kernel: per sequence arg-max -> token, store, position + 1, next mask row, next embedding row
//
// A wave owns whole output columns and splits K over its lanes EXACTLY like the batch-1 kernels of decode.hip (same lane split, same
// accumulation order per sequence, same epilogue expressions), so every sequence gets the bits its batch-1 run gets: tokens AND
// logits of showo_engine_batch_decode_greedy equal NB separate showo_engine_decode_greedy runs (tests/test_decode_batch_gpu.py).
// A wide batch (decode_wide.hip) runs MFMA skinny GEMMs instead; a shared-prefix batch (attn_shared.hip) is a wide batch whose slots
// hold only the rows behind the engine's own decode cache and attend to that cache in place.
// The whole step replays as a hipGraph with the NB positions in device memory (engine.h replay_steps, shared with the batch-1 loop of
// decode_engine.hip).  The weight images of a layer come from decode_layer_ops (decode.hip), the prefill / append of a slot from
// engine_prefill_into / engine_append_into (decode_engine.hip); every NB-templated launch goes through dispatch_int below.
#include "engine.h"
#include "decode_common.h"
#include "sample_row.h"
#include "decode_wide.h"
#include "attn_shared.h"
#include "logit_adjust.h"
#include "seq_rules.h"
#include "beam.h"
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <type_traits>

using namespace showo;

namespace {

constexpr int MAXB = 32;   // per-slot storage: a wide batch (showo_engine_batch_begin_wide, decode_wide.hip) holds up to 32 sequences
constexpr int NARROW_B = 8;  // the dot2 kernels of this file serve 1..8

// REG (NB <= 4): after the LayerNorm every lane keeps ITS 32 activation values of each sequence in registers as 16 packed bf16 pairs
// (the k positions lane * 8 + u * 512 + j are the same for every weight row), so a weight row costs 16 NB v_dot2c_f32_bf16 per lane, no
// conversion and no LDS read -- with the activations re-read from LDS per row (the batch-1 form, !REG) four sequences made the step
// VALU / LDS-bound.  Fewer, longer-lived waves (2 blocks per CU) amortise the register fill (grid caps 256 / 1024 and 4 rows in flight
// measured slower: profiles/r5_decode_batch_sweep.txt).  Same products and the same accumulation order per sequence either way.
// F16: weights and 16-bit activations are IEEE half (precision 2; common.h Op16).  HEAD3 (precision 2's lm_head, fp32 logits only): the
// normalised row is kept as a (hi, lo) bf16 pair and the weights come as (hi, lo) bf16 rows (W0, W0lo): acc = hi.hi + lo.hi + hi.lo in
// ONE chain per sequence -- the split-bf16 product of engine.hip head_rows_precise_fast without its 3 H image (2 x 240 MB instead of
// 719 MB per token step) and without a separate LayerNorm launch.  The bits of that 3 H GEMV where H is a multiple of 2048 (Phi-1.5's
// width: its three segments then start on chunk boundaries and a lane's chain visits them in this order); at any other H the same
// 3 H products reach the lanes' chains in another grouping (tests/test_decode_batch_gpu.py, the H 576 geometry).
// Q8 (precision 3): int8 weight rows, converted exactly to bf16 ONCE per weight for all NB sequences, and tot * scale[n] in front of the
// epilogue (decode_common.h): per sequence the arithmetic of ln_gemv2_kernel's int8 instance.
template <int NB, bool REG, bool F16 = false, bool HEAD3 = false, bool Q8 = false>
__global__ __launch_bounds__(256, 2) void ln_gemvB_kernel(LnGemvBArgs g) {  // H <= 2048; 2 weight rows in flight per wave (4: measured slower)
    static_assert(!(HEAD3 && (REG || F16)), "the split head keeps its activations in LDS and multiplies bf16 halves");
    static_assert(!(Q8 && (F16 || HEAD3)), "int8 weights multiply bf16 activations");
    constexpr int R = 2;
    extern __shared__ bf16_t sh[];  // [NB][H] normalised rows (16-bit, like showo_layernorm_f32_op16's output); HEAD3: [NB][2 H] = hi | lo
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: row bases live in SGPRs
    const int H = g.H, Ntot = g.N0 + g.N1;
    const int stride = gridDim.x * 4;
    int n = blockIdx.x * 4 + wave;
    auto rowp = [&](int c) { return c < g.N0 ? wrow<Q8>(g.W0, c, H) : wrow<Q8>(g.W1, c - g.N0, H); };
    typename WVec<Q8>::type br[R][4];
    uint4 bl[HEAD3 ? R : 1][4];
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (n + r * stride < Ntot) {
            load4(rowp(n + r * stride), lane * 8, H, br[r]);
            if constexpr (HEAD3) load4(g.W0lo + (int64_t)(n + r * stride) * H, lane * 8, H, bl[r]);
        }
    constexpr int LDH = HEAD3 ? 2 : 1;  // activation row stride in LDS, in units of H
    // LayerNorm: wave w normalises rows w, w + 4, ... with ln_gemv2_kernel's lane split and expressions (same bits per row)
    for (int b = wave; b < NB; b += 4) {
        const float* xr = g.x + (int64_t)b * H;
        float4 xv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = lane * 4 + j * 256;
            xv[j] = i < H ? *reinterpret_cast<const float4*>(xr + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (lane * 4 + j * 256 < H) s += (xv[j].x + xv[j].y) + (xv[j].z + xv[j].w);
        const float mean = wave_sum(s) / (float)H;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (lane * 4 + j * 256 < H) {
                const float a = xv[j].x - mean, c = xv[j].y - mean, d = xv[j].z - mean, e = xv[j].w - mean;
                q += (a * a + c * c) + (d * d + e * e);
            }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)H + g.eps);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = lane * 4 + j * 256;
            if (i < H) {
                const float4 v = xv[j];
                const float4 w = *reinterpret_cast<const float4*>(g.lnw + i);
                const float4 bb = *reinterpret_cast<const float4*>(g.lnb + i);
                const float y0 = (v.x - mean) * rstd * w.x + bb.x, y1 = (v.y - mean) * rstd * w.y + bb.y;
                const float y2 = (v.z - mean) * rstd * w.z + bb.z, y3 = (v.w - mean) * rstd * w.w + bb.w;
                uint2 o;
                o.x = Op16<F16>::pack2(y0, y1);
                o.y = Op16<F16>::pack2(y2, y3);
                *reinterpret_cast<uint2*>(sh + b * LDH * H + i) = o;
                if constexpr (HEAD3) {  // low halves: y - bf16(y), rounded to bf16 (precise.hip ln_split3_kernel's expressions)
                    uint2 lo;
                    lo.x = pack_bf2(y0 - bf2f((bf16_t)(o.x & 0xffffu)), y1 - bf2f((bf16_t)(o.x >> 16)));
                    lo.y = pack_bf2(y2 - bf2f((bf16_t)(o.y & 0xffffu)), y3 - bf2f((bf16_t)(o.y >> 16)));
                    *reinterpret_cast<uint2*>(sh + b * LDH * H + H + i) = lo;
                }
            }
        }
    }
    __syncthreads();
    uint32_t act[REG ? NB : 1][16];
    if constexpr (REG) {
#pragma unroll
        for (int b = 0; b < NB; ++b) load_act_pairs(sh + b * H, lane * 8, H, act[b]);
    }
    while (n < Ntot) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int c = n + r * stride;
            if (c < Ntot) {
                float acc[NB];
                if constexpr (REG) {
#pragma unroll
                    for (int b = 0; b < NB; ++b) acc[b] = 0.f;
                    fma4_regs<NB, F16>(br[r], act, lane * 8, H, acc);
                } else if constexpr (HEAD3) {
#pragma unroll
                    for (int b = 0; b < NB; ++b) {  // K' = [hi.hi | lo.hi | hi.lo], one chain (the order of the 3 H GEMV it replaces)
                        float t = fma4(br[r], sh + b * 2 * H, lane * 8, H, 0.f);
                        t = fma4(br[r], sh + b * 2 * H + H, lane * 8, H, t);
                        acc[b] = fma4(bl[r], sh + b * 2 * H, lane * 8, H, t);
                    }
                } else {
#pragma unroll
                    for (int b = 0; b < NB; ++b) acc[b] = fma4<F16>(br[r], sh + b * H, lane * 8, H, 0.f);
                }
                if (c + R * stride < Ntot) {
                    load4(rowp(c + R * stride), lane * 8, H, br[r]);
                    if constexpr (HEAD3) load4(g.W0lo + (int64_t)(c + R * stride) * H, lane * 8, H, bl[r]);
                }
                if constexpr (NB <= 4) {  // lane 16 b finishes sequence b (wave_sum's order of additions per sequence: decode_common.h)
                    const float tot = wave_sum_groups<NB>(acc);
                    const int b = lane >> 4;
                    if ((lane & 15) == 0 && b < NB) {
                        if (c < g.N0) {
                            const float a = q8_scale<Q8>(tot, g.s0, c);
                            const float v = a + g.b0[c];
                            if (g.outf) g.outf[(int64_t)b * g.ld0 + c] = v;
                            else g.out0[(int64_t)b * g.ld0 + c] = Op16<F16>::cvt(v);
                        } else {
                            const float a = q8_scale<Q8>(tot, g.s1, c - g.N0);
                            g.out1[(int64_t)b * g.ld1 + (c - g.N0)] = Op16<F16>::cvt(gelu_new_fast(a + g.b1[c - g.N0]));
                        }
                    }
                } else {
#pragma unroll
                    for (int b = 0; b < NB; ++b) acc[b] = wave_sum(acc[b]);
                    if (lane == 0) {
                        if (c < g.N0) {
                            const float bias = g.b0[c];
#pragma unroll
                            for (int b = 0; b < NB; ++b) {
                                const float a = q8_scale<Q8>(acc[b], g.s0, c);
                                const float v = a + bias;
                                if (g.outf) g.outf[(int64_t)b * g.ld0 + c] = v;
                                else g.out0[(int64_t)b * g.ld0 + c] = Op16<F16>::cvt(v);
                            }
                        } else {
                            const float bias = g.b1[c - g.N0];
#pragma unroll
                            for (int b = 0; b < NB; ++b) {
                                const float a = q8_scale<Q8>(acc[b], g.s1, c - g.N0);
                                g.out1[(int64_t)b * g.ld1 + (c - g.N0)] = Op16<F16>::cvt(gelu_new_fast(a + bias));
                            }
                        }
                    }
                }
            }
        }
        n += R * stride;
    }
}

// C = 2048-element chunks per output column (dense chunks first, then fc2 chunks), all in flight per wave (out_gemv2_kernel<C, 0>)
template <int C, int NB, bool F16 = false, bool Q8 = false>
__global__ __launch_bounds__(512) void out_gemvB_kernel(OutGemvBArgs g) {
    extern __shared__ bf16_t sa[];  // [NB][K0 + K1]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: row bases live in SGPRs
    const int stride = gridDim.x * 8;
    const int c0 = (g.K0 + 2047) / 2048;
    const int KK = g.K0 + g.K1;
    int n = blockIdx.x * 8 + wave;
    typedef typename WVec<Q8>::type wvec_t;
    auto issue = [&](int col, int t, wvec_t (&wv)[4]) {
        if (t < c0) load4(wrow<Q8>(g.W0, col, g.K0), t * 2048 + lane * 8, g.K0, wv);
        else load4(wrow<Q8>(g.W1, col, g.K1), (t - c0) * 2048 + lane * 8, g.K1, wv);
    };
    wvec_t buf[C][4];
    if (n < g.N) {
#pragma unroll
        for (int t = 0; t < C; ++t) issue(n, t, buf[t]);
    }
    for (int b = 0; b < NB; ++b)
        for (int i = threadIdx.x * 8; i < KK; i += 512 * 8)
            *reinterpret_cast<uint4*>(sa + b * KK + i) = i < g.K0 ? *reinterpret_cast<const uint4*>(g.a0 + (int64_t)b * g.lda0 + i)
                                                                  : *reinterpret_cast<const uint4*>(g.a1 + (int64_t)b * g.lda1 + (i - g.K0));
    __syncthreads();
    while (n < g.N) {
        const int nn = n + stride;
        float acc0[NB], acc1[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) { acc0[b] = 0.f; acc1[b] = 0.f; }
#pragma unroll
        for (int t = 0; t < C; ++t) {
            if constexpr (Q8) {  // fma4 per sequence, u ascending into the same chain; an int8 group is converted once for all NB
                if (t < c0) fma4_lds<NB>(buf[t], sa, KK, t * 2048 + lane * 8, g.K0, acc0);
                else fma4_lds<NB>(buf[t], sa + g.K0, KK, (t - c0) * 2048 + lane * 8, g.K1, acc1);
            } else {
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if (t < c0) acc0[b] = fma4<F16>(buf[t], sa + b * KK, t * 2048 + lane * 8, g.K0, acc0[b]);
                    else acc1[b] = fma4<F16>(buf[t], sa + b * KK + g.K0, (t - c0) * 2048 + lane * 8, g.K1, acc1[b]);
                }
            }
            if (nn < g.N) issue(nn, t, buf[t]);
        }
        if constexpr (NB <= 4) {
            const float t0 = wave_sum_groups<NB>(acc0), t1 = wave_sum_groups<NB>(acc1);
            if ((lane & 15) == 0 && (lane >> 4) < NB) {
                const int64_t i = (int64_t)(lane >> 4) * g.N + n;
                const float d0 = q8_scale<Q8>(t0, g.s0, n), d1 = q8_scale<Q8>(t1, g.s1, n);
                float v = d0 + g.b0[n];  // x1 = x + (dense + bd)       (out_gemv2_kernel's order and parenthesisation)
                v += g.x[i];
                float v2 = d1 + g.b1[n];  // x2 = x1 + (fc2 + b2)
                v2 += v;
                g.x[i] = v2;
            }
        } else {
#pragma unroll
            for (int b = 0; b < NB; ++b) { acc0[b] = wave_sum(acc0[b]); acc1[b] = wave_sum(acc1[b]); }
            if (lane == 0) {
                const float bd = g.b0[n], b2 = g.b1[n];
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const float d0 = q8_scale<Q8>(acc0[b], g.s0, n), d1 = q8_scale<Q8>(acc1[b], g.s1, n);
                    float v = d0 + bd;
                    v += g.x[(int64_t)b * g.N + n];
                    float v2 = d1 + b2;
                    v2 += v;
                    g.x[(int64_t)b * g.N + n] = v2;
                }
            }
        }
        n = nn;
    }
}

// Third launch of the co-scheduled batched layer: x[b][n] = (x[b][n] + (dense(attn[b]) + bd)) + y2[b][n]  (out_gemv2_kernel<1, 2>'s
// expression; y2 = fc2 + b2 from the fc2 role of the attention launch).  K0 <= 2048: the lane's 32 attention values per sequence stay
// in registers.
template <int NB, bool F16 = false, bool Q8 = false>
__global__ __launch_bounds__(512) void out_dense_y2B_kernel(OutGemvBArgs g) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: row bases live in SGPRs
    const int stride = gridDim.x * 8;
    int n = blockIdx.x * 8 + wave;
    typename WVec<Q8>::type buf[4];
    if (n < g.N) load4(wrow<Q8>(g.W0, n, g.K0), lane * 8, g.K0, buf);
    uint32_t act[NB][16];
#pragma unroll
    for (int b = 0; b < NB; ++b) load_act_pairs(g.a0 + (int64_t)b * g.lda0, lane * 8, g.K0, act[b]);
    while (n < g.N) {
        const int nn = n + stride;
        // epilogue operands of this column requested up front (they do not depend on the products): no dependent round trip at the tail
        const bool writer = (lane & 15) == 0 && (lane >> 4) < NB;
        const int64_t i = (int64_t)(lane >> 4) * g.N + n;
        float xv = 0.f, yv = 0.f, bd = 0.f;
        if (writer) { xv = g.x[i]; yv = g.y2[i]; bd = g.b0[n]; }
        float acc0[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) acc0[b] = 0.f;
        fma4_regs<NB, F16>(buf, act, lane * 8, g.K0, acc0);
        if (nn < g.N) load4(wrow<Q8>(g.W0, nn, g.K0), lane * 8, g.K0, buf);
        const float tot = wave_sum_groups<NB>(acc0);
        if (writer) {
            const float d0 = q8_scale<Q8>(tot, g.s0, n);
            float v = d0 + bd;
            v += xv;
            float v2 = yv;
            v2 += v;
            g.x[i] = v2;
        }
        n = nn;
    }
}

__global__ void batch_iv_kernel(const int32_t* __restrict__ last_iv, const int* __restrict__ L0, const int* __restrict__ pos, int32_t* __restrict__ iv,
                                int nb) {
    const int b = threadIdx.x;
    if (b < nb) next_iv(last_iv + 4 * b, L0[b], pos[b], iv + 4 * b);
}

// Token boundary of the batched greedy loop, one block per sequence: arg-max of its logits row (first maximal index, like
// showo_argmax_f32) -> token, append to its output row, position + 1, next mask row, next embedding row.
__global__ __launch_bounds__(1024) void greedy_seam_rows_kernel(const float* __restrict__ logits, int V, int64_t* __restrict__ tok,
                                                                int64_t* __restrict__ out_tokens, int n_steps, int* __restrict__ pos,
                                                                const int* __restrict__ base, const float* __restrict__ table,
                                                                float* __restrict__ x, int H, const int32_t* __restrict__ last_iv,
                                                                const int* __restrict__ L0, int32_t* __restrict__ iv) {
    __shared__ RowPickSmem sm;
    __shared__ int s_tok;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int bi = argmax_row_1024(logits + (int64_t)b * V, V, sm);
    if (tid == 0) {
        s_tok = bi;
        tok[b] = bi;
        const int P = pos[b];
        out_tokens[(int64_t)b * n_steps + (P - base[b])] = bi;
        pos[b] = P + 1;
        next_iv(last_iv + 4 * b, L0[b], P + 1, iv + 4 * b);
    }
    __syncthreads();
    const int id = s_tok;
    float* xr = x + (int64_t)b * H;
    if (id < 0 || id >= V) {
        for (int i = tid; i < H; i += 1024) xr[i] = __builtin_nanf("");
        return;
    }
    const float* src = table + (int64_t)id * H;
    for (int i = tid; i < H; i += 1024) xr[i] = src[i];
}

// shared memory of the sampled seam: the nucleus instance adds the mass histogram
template <bool NUCLEUS> struct SeamPickSmem { RowPickSmem pick; };
template <> struct SeamPickSmem<true> : RowNucleusSmem {};

// Per-slot state of showo_engine_batch_decode_sample: set by the host before the steps are captured, advanced by the sampled seam.
struct SlotDraw {
    const float* noise;  // NULL or [*, V] Exp(1) rows: row d replaces the Philox draw d
    uint64_t seed;
    float temperature;
    int top_k;
    int draw0;     // draw index of the slot's first token in this call
    int budget;    // tokens the slot may emit in this call
    int produced;  // tokens emitted so far in this call
    int step;      // seam launches so far in this call (the column of out_tokens)
    int active;    // 0: stopped (budget spent or <eot> emitted) or idle from the start
    float top_p;   // >= 1: no nucleus filter (sample_topk_row); 0 < top_p < 1: sample_topk_topp_row
};
static_assert(sizeof(SlotDraw) % sizeof(int) == 0 && offsetof(SlotDraw, active) % sizeof(int) == 0,
              "the adjust launch reads SlotDraw.active as a strided int array");

// (slot_embed_row, the row of slot b for its next step: decode_common.h)
__global__ __launch_bounds__(256) void slot_embed_kernel(const int64_t* __restrict__ tok, const SlotDraw* __restrict__ sd,
                                                         const float* __restrict__ table, float* __restrict__ x, int H, int V) {
    const int b = blockIdx.x;
    slot_embed_row(tok[b], sd[b].active != 0, table, x + (int64_t)b * H, H, V, threadIdx.x, 256);
}

// Token boundary of the batched sampled loop, one block per slot.  A decoding slot picks its token -- the arg-max for top_k == 1 (the
// greedy seam's pick), else sample_topk_row with its own top_k / temperature / seed / draw index (the batch-1 sampler's draw) -- and
// stores it, then either advances (position + 1, next mask row, next embedding row) or, after its last budgeted token or <eot>, goes
// idle.  An idle slot writes -1 into its output row, keeps its position (at most lim - 1, so its K/V append never leaves the cache and
// the rotary tables) and feeds the zero row.  NUCLEUS: some slot of the call has top_p < 1; such a slot draws with sample_topk_topp_row,
// every other slot exactly as in the instance without it.
template <bool NUCLEUS>
__global__ __launch_bounds__(1024) void sample_seam_rows_kernel(const float* __restrict__ logits, int V, int64_t eot, int64_t* __restrict__ tok,
                                                                int64_t* __restrict__ out_tokens, int n_steps, int* __restrict__ pos, int lim,
                                                                SlotDraw* __restrict__ sd, const float* __restrict__ table, float* __restrict__ x,
                                                                int H, const int32_t* __restrict__ last_iv, const int* __restrict__ L0,
                                                                int32_t* __restrict__ iv) {
    __shared__ SeamPickSmem<NUCLEUS> smem;
    RowPickSmem& sm = smem.pick;
    __shared__ int s_tok, s_go;
    const int b = blockIdx.x, tid = threadIdx.x;
    SlotDraw* s = sd + b;
    const int active = s->active, top_k = s->top_k, d = s->draw0 + s->produced;  // block-uniform
    int pick = -1;
    if (active) {
        const float* row = logits + (int64_t)b * V;
        const float* en = s->noise ? s->noise + (int64_t)d * V : nullptr;
        if (top_k == 1) pick = argmax_row_1024(row, V, sm);
        else if (NUCLEUS && s->top_p < 1.f) {
            if constexpr (NUCLEUS) pick = sample_topk_topp_row(row, V, top_k, s->top_p, s->temperature, en, s->seed, d, smem);
        } else pick = sample_topk_row(row, V, top_k, s->temperature, en, s->seed, d, sm);
    }
    __syncthreads();  // every thread has read *s
    if (tid == 0) {
        const int j = s->step;
        int64_t* out = out_tokens + (int64_t)b * n_steps;
        const int P = pos[b];
        int go = 0;
        if (active) {
            tok[b] = pick;
            if (j < n_steps) out[j] = pick;
            const int np = s->produced + 1;
            s->produced = np;
            go = !(np >= s->budget || pick == eot);
            if (!go) s->active = 0;
            const int Pn = go ? P + 1 : min(P + 1, lim - 1);
            pos[b] = Pn;
            next_iv(last_iv + 4 * b, L0[b], Pn, iv + 4 * b);
        } else if (j < n_steps) {
            out[j] = -1;
        }
        s->step = j + 1;
        s_tok = pick;
        s_go = go;
    }
    __syncthreads();
    slot_embed_row(s_tok, s_go != 0, table, x + (int64_t)b * H, H, V, tid, 1024);
}

// Log-probability of what the sampled seam just stored, one block per slot: column sd[b].step - 1 of the slot's output row against its
// logits row (the seam leaves the rows alone).  A slot that idled in the step stored -1: logprob_row's t < 0 case, 0.0f / -1.
__global__ __launch_bounds__(1024) void logprob_slots_kernel(const float* __restrict__ logits, int V, const int64_t* __restrict__ out_tokens,
                                                             int n_steps, const SlotDraw* __restrict__ sd, float* __restrict__ lp,
                                                             int32_t* __restrict__ rank) {
    __shared__ RowLogprobSmem sm;
    const int b = blockIdx.x;
    const int j = sd[b].step - 1;
    if (j < 0 || j >= n_steps) return;  // block-uniform
    const int64_t at = (int64_t)b * n_steps + j;
    const RowLogprob o = logprob_row(logits + (int64_t)b * V, V, out_tokens[at], sm);
    if (threadIdx.x == 0) {
        lp[at] = o.lp;
        if (rank) rank[at] = o.rank;
    }
}

// f(std::integral_constant<int, n>) for the run-time n in LO..HI: the compile-time instance of a sequence count or chunk count
template <int LO, int HI, class F>
int dispatch_int(int n, const char* range_msg, F&& f) {
    if constexpr (LO > HI) return set_error_msg(1, range_msg);
    else return n == LO ? f(std::integral_constant<int, LO>{}) : dispatch_int<LO + 1, HI>(n, range_msg, f);
}

template <int NB>
int launch_ln_gemvB(const LnGemvBArgs& g, hipStream_t s, int op, bool head3) {
    const int Ntot = g.N0 + g.N1;
    const bool q8 = g.s0 != nullptr;  // int8 weight images (precision 3): the grids of the bf16 instances
    if (q8 && (op || head3 || (g.N1 && !g.s1) || (g.H % 16)))
        return set_error_msg(1, "ln_gemvB: int8 weights take bf16 activations, a scale per matrix and H % 16 == 0");
    // precision 2's lm_head: (hi, lo) activations in LDS, (hi, lo) bf16 weight rows
    if (head3 && (!g.W0lo || !g.outf || g.N1)) return set_error_msg(1, "ln_gemvB: the split head writes fp32 logits from (hi, lo) weight rows");
    // register-resident activations (NB <= 4, 16 NB packed registers per lane): up to 4 blocks per CU resident; else 12 rows per block
    const bool reg = NB <= 4 && !head3;
    const int want = reg ? (Ntot + 7) / 8 : (Ntot + 11) / 12, cap = reg ? showo::decode_tuning().batch_ln_blocks : 1280;
    const dim3 grid(want < cap ? want : cap);
    const size_t smem = (size_t)NB * g.H * sizeof(bf16_t) * (head3 ? 2 : 1);
    // (both forms are named for every NB, as they always were: the LDS-form instances of NB <= 4 are built and never launched)
    auto go = [&](auto kreg, auto klds) {
        if (reg) kreg<<<grid, dim3(256), smem, s>>>(g);
        else klds<<<grid, dim3(256), smem, s>>>(g);
    };
    if (q8) go(ln_gemvB_kernel<NB, (NB <= 4), false, false, true>, ln_gemvB_kernel<NB, false, false, false, true>);
    else if (head3) ln_gemvB_kernel<NB, false, false, true><<<grid, dim3(256), smem, s>>>(g);
    else if (op) go(ln_gemvB_kernel<NB, (NB <= 4), true>, ln_gemvB_kernel<NB, false, true>);
    else go(ln_gemvB_kernel<NB, (NB <= 4)>, ln_gemvB_kernel<NB, false>);
    return hipGetLastError() == hipSuccess ? 0 : set_error_msg(7, "ln_gemvB launch failed");
}
int ln_gemvB(int nb, const LnGemvBArgs& g, hipStream_t s, int op = 0, bool head3 = false) {
    return dispatch_int<1, NARROW_B>(nb, "batched decode: 1..8 sequences",
                                     [&](auto NB) { return launch_ln_gemvB<decltype(NB)::value>(g, s, op, head3); });
}

template <int C, int NB, bool F16, bool Q8 = false>
int launch_out_gemvB(const OutGemvBArgs& g, hipStream_t s) {
    static bool attr_set = false;
    const size_t smem = (size_t)NB * (g.K0 + g.K1) * sizeof(bf16_t);
    auto kfn = out_gemvB_kernel<C, NB, F16, Q8>;
    if (!attr_set && smem > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return set_error_hip(e, "hipFuncSetAttribute(out_gemvB)", __FILE__, __LINE__);
        attr_set = true;
    }
    if (smem > 160 * 1024) return set_error_msg(5, "batched decode: activations exceed the LDS");
    int blocks = (g.N + 7) / 8;
    if (blocks > showo::decode_tuning().out_blocks) blocks = showo::decode_tuning().out_blocks;
    kfn<<<dim3(blocks), dim3(512), smem, s>>>(g);
    return hipGetLastError() == hipSuccess ? 0 : set_error_msg(7, "out_gemvB launch failed");
}
int out_gemvB(int nb, const OutGemvBArgs& g, hipStream_t s, int op) {
    const bool q8 = g.s0 || g.s1;  // int8 weight images (precision 3)
    return dispatch_int<1, NARROW_B>(nb, "batched decode: 1..8 sequences", [&](auto NB) {
        if (q8 && (op || !g.s0 || !g.s1 || (g.K0 % 16) || (g.K1 % 16)))
            return set_error_msg(1, "out_gemvB: int8 weights take bf16 activations, both scales and K % 16 == 0");
        return dispatch_int<2, 5>((g.K0 + 2047) / 2048 + (g.K1 + 2047) / 2048, "batched decode: unsupported K0 / K1 (decode_fused_shapes_ok)", [&](auto C) {
            constexpr int c = decltype(C)::value, n = decltype(NB)::value;
            return q8 ? launch_out_gemvB<c, n, false, true>(g, s) : op ? launch_out_gemvB<c, n, true>(g, s) : launch_out_gemvB<c, n, false>(g, s);
        });
    });
}
int out_dense_y2B(int nb, const OutGemvBArgs& g, hipStream_t s, int op) {
    int blocks = (g.N + 7) / 8;
    if (blocks > showo::decode_tuning().out_blocks) blocks = showo::decode_tuning().out_blocks;
    const bool q8 = g.s0 != nullptr;  // int8 image of the dense matrix (precision 3)
    if (q8 && (op || (g.K0 % 16))) return set_error_msg(1, "out_dense_y2B: int8 weights take bf16 activations and K % 16 == 0");
    const int rc = dispatch_int<2, 4>(nb, "batched decode: the co-scheduled layer serves 2..4 sequences", [&](auto NB) {
        constexpr int n = decltype(NB)::value;
        if (q8) out_dense_y2B_kernel<n, false, true><<<dim3(blocks), dim3(512), 0, s>>>(g);
        else if (op) out_dense_y2B_kernel<n, true><<<dim3(blocks), dim3(512), 0, s>>>(g);
        else out_dense_y2B_kernel<n><<<dim3(blocks), dim3(512), 0, s>>>(g);
        return 0;
    });
    if (rc) return rc;
    return hipGetLastError() == hipSuccess ? 0 : set_error_msg(7, "out_dense_y2B launch failed");
}

}  // namespace

namespace showo {
// LayerNorm + lm_head of `nb` residual rows as the split-bf16 product (precision 2's head on a decode step): logits[b][n] = fp32,
// row stride ld.  One launch, 2 x [N, H] bf16 of weights (ln_gemvB_kernel<.., HEAD3>); the batched loop and the batch-1 step share it.
int decode_split_head(const float* x, const float* lnw, const float* lnb, float eps, int H, const bf16_t* Whi, const bf16_t* Wlo,
                      const float* bias, float* logits, int N, int ld, int nb, hipStream_t s) {
    LnGemvBArgs h{x, lnw, lnb, eps, H, Whi, bias, nullptr, logits, N, ld, nullptr, nullptr, nullptr, 0, 0};
    h.W0lo = Wlo;
    return ln_gemvB(nb, h, s, 0, true);
}
}  // namespace showo

// ---- engine entry points ------------------------------------------------------------------------------------------------------
// State of a decode batch: per-layer caches [nb][heads][cap][64] (K) / [nb][heads][64][cap] (V^T), per-sequence prompt length,
// live length and last prompt mask row; device copies for the graph-replayed loop.
struct showo_engine::BatchDecode {
    int nb = 0, cap = 0;
    bf16_t *k = nullptr, *vt = nullptr;
    int64_t elems = 0;  // allocated elements per cache
    int prompt_len[MAXB] = {0}, cache_len[MAXB] = {0};
    int last_iv[MAXB][4] = {{0}};
    int *pos_dev = nullptr, *L0_dev = nullptr, *base_dev = nullptr;
    int32_t *last_iv_dev = nullptr, *iv_dev = nullptr;
    float* y2 = nullptr;  // [nb, H] fc2 + b2 of the current layer (co-scheduled form)
    SlotDraw* slots_dev = nullptr;  // [MAXB] per-slot draw / stop state of showo_engine_batch_decode_sample
    int precision = 0;    // the precision the caches were prefilled under (element type of K / V^T)
    bool wide = false;    // begun by showo_engine_batch_begin_wide: the step runs the MFMA kernels of decode_wide.hip
    showo::WideWs wws;    // their workspace (one per engine: its decode steps are ordered on one stream)
    // shared-prefix slots (showo_engine_batch_begin_shared; attn_shared.hip): k / vt are SUFFIX caches of `cap` rows, key k >= P of a
    // slot at row k - base; every length and position of this struct stays absolute
    bool shared = false;
    int P = 0, base = 0;     // the engine cache's length when the batch began; P & ~63
    int64_t epoch = 0;       // its epoch then
    int pre_iv[4] = {0, 0, 0, 0};  // what every appended or decode row sees of [0, P): the last prefill row's rule at position P - 1
    float* sws = nullptr;    // the prefix partials (showo::shared_attn_ws_elems)
    int64_t sws_elems = 0;
    int abs_cap() const { return shared ? base + cap : cap; }  // first position beyond a slot's cache
    // beam search (showo_engine_batch_beam_begin / _batch_decode_beam; beam.hip): the selection's buffers, the slots' pointer tables and
    // the staging buffer of the parent copies, sized for rows [beam_P0, beam_P0 + beam_span)
    float *beam_norm = nullptr, *beam_ws = nullptr;
    showo::BeamCand* beam_cand = nullptr;
    uint16_t **beam_ktab = nullptr, **beam_vtab = nullptr;
    bf16_t *beam_stage_k = nullptr, *beam_stage_vt = nullptr;
    int64_t beam_stage_elems = 0;
    int beam_P0 = 0, beam_span = 0;
    const int32_t* beam_state = nullptr;  // the state block of the running search (nullptr: none)
};

namespace showo {
void engine_batch_free(showo_engine* e) {
    if (e && e->bd) { showo::wide_ws_free(&e->bd->wws); delete e->bd; e->bd = nullptr; }  // the other device buffers live in e->allocs
}
}  // namespace showo

static int batch_begin(showo_engine* e, int nb, int cap_tokens, bool wide, bool shared = false) {
    if (!e) return set_error_msg(1, "engine: null handle");
    int pre_iv[4] = {0, 0, 0, 0};  // shared: what every row behind P sees of [0, P)
    if (!wide && (nb < 1 || nb > NARROW_B)) return set_error_msg(1, "batch_begin: 1..8 sequences");
    if (wide && (nb < 1 || nb > MAXB)) return set_error_msg(1, "batch_begin_wide: 1..32 sequences");
    if (wide && e->precision != 0) return set_error_msg(1, "batch_begin_wide: the wide decode batch runs at precision 0 (bf16 operands) only");
    if (wide && ((e->H % 32) || (e->F % 32))) return set_error_msg(1, "batch_begin_wide: hidden and ffn must be multiples of 32");
    if (!decode_fused_shapes_ok(e->H, e->F)) return set_error_msg(1, "batch_begin: hidden <= 2048 and ffn <= 8192 (multiples of 8) required");
    if (shared) {
        if (e->cache_len <= 0) return set_error_msg(1, "batch_begin_shared: prefill first");
        if (e->cache_precision != e->precision)
            return set_error_msg(1, "batch_begin_shared: the KV cache was prefilled under another precision: prefill again");
        if (cap_tokens < (e->cache_len & 63) + 2) return set_error_msg(5, "batch_begin_shared: no room behind the prefix");
        // the decode rule at position P - 1 (decode_common.h next_iv): the run that ends at prompt_len, or an empty one, reaches P
        int* v = pre_iv;
        for (int i = 0; i < 4; ++i) v[i] = e->last_iv[i];
        const int L0 = e->prompt_len, P = e->cache_len;
        if (v[1] == L0 && v[0] < v[1]) v[1] = P;
        else if (v[3] == L0 && v[2] < v[3]) v[3] = P;
        else if (!(v[2] < v[3])) { v[2] = L0; v[3] = P; }
        else if (!(v[0] < v[1])) { v[0] = L0; v[1] = P; }
        else return set_error_msg(6, "batch_begin_shared: mask row needs more than two intervals");
    }
    if (nb > e->maxT) return set_error_msg(5, "batch_begin: more sequences than workspace rows");
    int cap = ((cap_tokens + 63) / 64) * 64;
    if (cap_tokens < 2 || cap > ((e->cfg.max_pos + 63) / 64) * 64) return set_error_msg(5, "batch_begin: capacity exceeds max_position_embeddings");
    if ((size_t)cap * 4 + 2048 > 60000) return set_error_msg(5, "batch_begin: capacity exceeds the single-block decode attention");
    if (!e->bd) e->bd = new showo_engine::BatchDecode();
    auto* d = e->bd;
    const int64_t need = (int64_t)e->nL * nb * e->nH * cap * 64;
    if (need > d->elems) {  // grow: the previous caches are freed first (nothing of an earlier batch survives a batch_begin)
        SHOWO_CHECK_HIP(hipDeviceSynchronize());
        e->release(&d->k);
        e->release(&d->vt);
        d->elems = 0;
        TRY(e->alloc(&d->k, need));
        TRY(e->alloc(&d->vt, need));
        d->elems = need;
        // zeroed ONCE, when the caches are (re)allocated (the two memsets -- 600 MB at cfg4 -- ran on every call): columns of
        // V^T beyond a sequence's live length only ever meet probabilities that are exactly 0, so they must be FINITE, not zero; what an
        // earlier batch left there need not be (a NaN activation), so each prefill re-zeroes the columns its last key tile reads
        // (engine_prefill_into), and the decode steps never multiply columns beyond the live length
        SHOWO_CHECK_HIP(hipMemset(d->k, 0, (size_t)need * sizeof(bf16_t)));
        SHOWO_CHECK_HIP(hipMemset(d->vt, 0, (size_t)need * sizeof(bf16_t)));
    }
    if (!d->pos_dev) {
        TRY(e->alloc(&d->pos_dev, MAXB)); TRY(e->alloc(&d->L0_dev, MAXB)); TRY(e->alloc(&d->base_dev, MAXB));
        TRY(e->alloc(&d->last_iv_dev, 4 * MAXB)); TRY(e->alloc(&d->iv_dev, 4 * MAXB));
    }
    if (wide) TRY(showo::wide_ws_reserve(&d->wws, e->H, e->H));
    if (shared) {
        const int64_t need_ws = showo::shared_attn_ws_elems(e->nH, e->cache_len);
        if (need_ws > d->sws_elems) {
            SHOWO_CHECK_HIP(hipDeviceSynchronize());
            e->release(&d->sws);
            d->sws_elems = 0;
            TRY(e->alloc(&d->sws, need_ws));
            d->sws_elems = need_ws;
        }
    }
    // nothing above can fail from here on: the batch's fields change together
    d->shared = shared;
    if (shared) {
        d->P = e->cache_len; d->base = e->cache_len & ~63; d->epoch = e->cache_epoch;
        for (int i = 0; i < 4; ++i) d->pre_iv[i] = pre_iv[i];
        d->precision = e->precision;
    }
    d->nb = nb; d->cap = cap; d->wide = wide;
    d->beam_state = nullptr;  // (a search does not outlive its batch)
    for (int b = 0; b < MAXB; ++b) { d->prompt_len[b] = 0; d->cache_len[b] = 0; }
    return 0;
}

extern "C" int showo_engine_batch_begin(showo_engine* e, int nb, int cap_tokens) { return batch_begin(e, nb, cap_tokens, false); }
extern "C" int showo_engine_batch_begin_wide(showo_engine* e, int nb, int cap_tokens) { return batch_begin(e, nb, cap_tokens, true); }
extern "C" int showo_engine_batch_begin_shared(showo_engine* e, int nb, int cap_suffix_tokens) {
    return batch_begin(e, nb, cap_suffix_tokens, true, true);
}
extern "C" int showo_engine_batch_shared_state(const showo_engine* e, int* P, int* base, int* cap_s) {
    if (!e || !e->bd || e->bd->nb == 0 || !e->bd->shared) return set_error_msg(1, "batch_shared_state: showo_engine_batch_begin_shared first");
    if (P) *P = e->bd->P;
    if (base) *base = e->bd->base;
    if (cap_s) *cap_s = e->bd->cap;
    return 0;
}

extern "C" int showo_engine_batch_prefill(showo_engine* e, int b, const int64_t* ids, const float* embeds, const float* mask, int L,
                                          float* logits_last, void* stream) {
    if (!e || !e->bd || e->bd->nb == 0) return set_error_msg(1, "batch_prefill: showo_engine_batch_begin first");
    auto* d = e->bd;
    if (b < 0 || b >= d->nb) return set_error_msg(1, "batch_prefill: bad sequence index");
    if (d->shared) return set_error_msg(1, "batch_prefill: a shared-prefix batch fills its slots with showo_engine_batch_attach_append");
    if (L + 1 > d->cap) return set_error_msg(5, "batch_prefill: prompt exceeds the batch's cache capacity");
    if (showo_engine_missing(e) != 0) return set_error_msg(4, "engine: weights missing (showo_engine_missing() != 0)");
    if (L < 1 || L > e->maxT || L > e->cfg.max_seq || L > e->cfg.max_pos) return set_error_msg(5, "engine: sequence exceeds the configured workspace");
    if (e->precision == 1) return set_error_msg(1, "batch_prefill: the batched decode runs at precision 0 (bf16 operands) or 2 (fp16 operands)");
    const int64_t per_seq = (int64_t)e->nH * d->cap * 64, lstride = (int64_t)d->nb * per_seq;
    TRY(showo::engine_prefill_into(e, ids, embeds, mask, L, d->k + b * per_seq, d->vt + b * per_seq, lstride, lstride, d->cap, d->last_iv[b],
                                   logits_last, (hipStream_t)stream, nullptr, nullptr));
    d->prompt_len[b] = L;
    d->cache_len[b] = L;
    d->precision = e->precision;
    return 0;
}

// ---- mmu sessions: a slot that starts as a copy of the engine's decode cache, and more prompt rows onto a slot ---------------------
extern "C" int showo_engine_batch_slot_ptrs(showo_engine* e, int b, uint16_t** k, uint16_t** vt, int64_t* k_lstride, int64_t* v_lstride,
                                            int* cap) {
    if (!e || !e->bd || e->bd->nb == 0) return set_error_msg(1, "batch_slot_ptrs: showo_engine_batch_begin first");
    auto* d = e->bd;
    if (b < 0 || b >= d->nb) return set_error_msg(1, "batch_slot_ptrs: bad sequence index");
    const int64_t per_seq = (int64_t)e->nH * d->cap * 64, lstride = (int64_t)d->nb * per_seq;
    if (k) *k = d->k + b * per_seq;
    if (vt) *vt = d->vt + b * per_seq;
    if (k_lstride) *k_lstride = lstride;
    if (v_lstride) *v_lstride = lstride;
    if (cap) *cap = d->cap;
    return 0;
}

extern "C" int showo_engine_batch_fork(showo_engine* e, int b, void* stream) {
    if (!e || !e->bd || e->bd->nb == 0) return set_error_msg(1, "batch_fork: showo_engine_batch_begin first");
    auto* d = e->bd;
    if (b < 0 || b >= d->nb) return set_error_msg(1, "batch_fork: bad sequence index");
    if (d->shared) return set_error_msg(1, "batch_fork: a shared-prefix batch fills its slots with showo_engine_batch_attach_append");
    if (e->cache_len <= 0) return set_error_msg(1, "batch_fork: prefill first");
    if (e->precision == 1) return set_error_msg(1, "batch_fork: the batched decode runs at precision 0, 2 or 3");
    if (e->cache_precision != e->precision) return set_error_msg(1, "batch_fork: the KV cache was prefilled under another precision: prefill again");
    if (e->cache_len + 1 > d->cap) return set_error_msg(5, "batch_fork: the cache exceeds the batch's cache capacity");
    const int64_t per_seq = (int64_t)e->nH * d->cap * 64, lstride = (int64_t)d->nb * per_seq;
    const int64_t src_lstride = (int64_t)e->nH * e->cache_cap * 64;
    TRY(showo_kv_fork(e->kcache, e->vtcache, e->cache_cap, src_lstride, src_lstride, d->k + b * per_seq, d->vt + b * per_seq, d->cap, lstride,
                      lstride, e->nL, e->nH, e->cache_len, stream));
    d->prompt_len[b] = e->prompt_len;
    d->cache_len[b] = e->cache_len;
    for (int i = 0; i < 4; ++i) d->last_iv[b][i] = e->last_iv[i];
    d->precision = e->precision;
    return 0;
}

extern "C" int showo_engine_batch_prefill_append(showo_engine* e, int b, const int64_t* ids, const float* embeds, int Ln, float* logits_last,
                                                 void* stream) {
    if (!e || !e->bd || e->bd->nb == 0) return set_error_msg(1, "batch_prefill_append: showo_engine_batch_begin first");
    auto* d = e->bd;
    if (b < 0 || b >= d->nb) return set_error_msg(1, "batch_prefill_append: bad sequence index");
    if (d->shared) return set_error_msg(1, "batch_prefill_append: a shared-prefix batch fills its slots with showo_engine_batch_attach_append");
    if (d->cache_len[b] <= 0) return set_error_msg(1, "batch_prefill_append: the slot has no prefill (showo_engine_batch_prefill / _batch_fork first)");
    if (e->precision == 1) return set_error_msg(1, "batch_prefill_append: the batched decode runs at precision 0, 2 or 3");
    if (d->precision != e->precision) return set_error_msg(1, "batch_prefill_append: the caches were prefilled under another precision: prefill again");
    const int64_t per_seq = (int64_t)e->nH * d->cap * 64, lstride = (int64_t)d->nb * per_seq;
    const int P = d->cache_len[b];
    TRY(showo::engine_append_into(e, ids, embeds, Ln, P, d->last_iv[b], d->prompt_len[b], d->k + b * per_seq, d->vt + b * per_seq, lstride,
                                  lstride, d->cap, logits_last, (hipStream_t)stream, nullptr, nullptr));
    d->cache_len[b] = P + Ln;
    return 0;
}

// ---- shared-prefix slots: the slot keeps the rows behind the engine cache's [0, P) only ----------------------------------------------
namespace {
// the engine's decode cache is still the one the shared batch began on
int shared_cache_check(const showo_engine* e, const char* what) {
    const auto* d = e->bd;
    if (e->cache_epoch != d->epoch || e->cache_len != d->P || e->cache_precision != e->precision || d->precision != e->precision)
        return set_error_msg(1, (std::string(what) + ": the engine's decode cache is no longer the one the shared batch began on "
                                                     "(another prefill, another length or another precision)").c_str());
    return 0;
}
}  // namespace

extern "C" int showo_engine_batch_attach_append(showo_engine* e, int b, const int64_t* ids, const float* embeds, int Ln, float* logits_last,
                                                void* stream) {
    if (!e || !e->bd || e->bd->nb == 0 || !e->bd->shared) return set_error_msg(1, "batch_attach_append: showo_engine_batch_begin_shared first");
    auto* d = e->bd;
    if (b < 0 || b >= d->nb) return set_error_msg(1, "batch_attach_append: bad sequence index");
    if (e->precision != 0) return set_error_msg(1, "batch_attach_append: a shared-prefix batch runs at precision 0 (bf16 operands) only");
    TRY(shared_cache_check(e, "batch_attach_append"));
    const int P = d->P;
    if (Ln < 1 || P - d->base + Ln + 1 > d->cap) return set_error_msg(5, "batch_attach_append: the rows exceed the batch's suffix capacity");
    const showo::KVDest kv = showo::kv_decode_cache(e);
    // showo_engine_prefill_append's call on the engine's own cache, whose length stays P on the books
    int rc = showo::engine_append_into(e, ids, embeds, Ln, P, e->last_iv, e->prompt_len, kv.k, kv.vt, kv.k_lstride, kv.v_lstride, kv.Lcap,
                                       logits_last, (hipStream_t)stream, kv.k_lo, kv.vt_lo);
    if (!rc) {
        const int64_t per_seq = (int64_t)e->nH * d->cap * 64, lstride = (int64_t)d->nb * per_seq;
        rc = showo_kv_copy_rows(kv.k, kv.vt, kv.Lcap, kv.k_lstride, kv.v_lstride, d->k + b * per_seq, d->vt + b * per_seq, d->cap, lstride,
                                lstride, e->nL, e->nH, P, P + Ln, d->base, stream);
    }
    // rewind to P whatever happened: the V^T columns the rows (or a part of them) wrote are zero again up to the end of their last tile
    e->cache_len = P + Ln < kv.Lcap ? P + Ln : kv.Lcap;
    const int rc2 = showo_engine_cache_rewind(e, P, stream);
    e->cache_len = P;
    if (rc) return rc;
    if (rc2) return rc2;
    d->prompt_len[b] = e->prompt_len;
    d->cache_len[b] = P + Ln;
    for (int i = 0; i < 4; ++i) d->last_iv[b][i] = e->last_iv[i];
    return 0;
}

namespace {
// Preconditions shared by the batched decode entries (precision, weight images, per-slot prefill, two-interval mask rows).
int batch_decode_checks(showo_engine* e, const char* what) {
    auto* d = e->bd;
    auto fail = [&](int code, const char* msg) { return set_error_msg(code, (std::string(what) + ": " + msg).c_str()); };
    if (e->precision == 1) return fail(1, "precision 0 (bf16 operands) or 2 (fp16 operands)");
    if (d->wide && e->precision != 0) return fail(1, "a wide batch (showo_engine_batch_begin_wide) runs at precision 0 (bf16 operands) only");
    if (e->precision == 3 && (int)e->q8_loaded.size() != e->nL * 6 + 1)
        return fail(4, "(precision 3) the int8 weight images are missing or stale: upload the weights again");
    const int op = e->precision == 2 ? SHOWO_OP_F16 : SHOWO_OP_BF16;
    if ((op == SHOWO_OP_F16) != e->img_f16) return fail(4, "the weight images hold the other 16-bit type: upload the weights again");
    if (d->precision != e->precision) return fail(1, "the caches were prefilled under another precision: prefill again");
    if (d->shared) TRY(shared_cache_check(e, what));
    if (op && (!e->wlm_lo || !e->lo_loaded.count("showo.lm_head.weight")))
        return fail(4, "(precision 2) the lm_head's low half is missing: upload the weights again");
    for (int b = 0; b < d->nb; ++b) {
        if (d->cache_len[b] <= 0) return fail(1, "a sequence has no prefill");
        const int *v = d->last_iv[b], L0 = d->prompt_len[b];
        if (!((v[1] == L0 && v[0] < v[1]) || (v[3] == L0 && v[2] < v[3]) || !(v[2] < v[3]) || !(v[0] < v[1])))
            return fail(6, "mask row needs more than two intervals");
    }
    return 0;
}

// One token step of the batch up to its logits: nb rows through the layers against their caches, final LayerNorm + lm_head.
// co: the co-scheduled layer (2..4 sequences at Phi-1.5's shape), else three plain launches per layer.
int batch_step_layers(showo_engine* e, int op, bool co, int lk_max, float* logits_ws, hipStream_t s) {
    auto* d = e->bd;
    const int nb = d->nb, H = e->H, F = e->F, nH = e->nH, V = e->V;
    const int64_t per_seq = (int64_t)nH * d->cap * 64, lstride = (int64_t)nb * per_seq;
    const bool q8 = e->precision == 3;
    const int co_blocks = showo::decode_tuning().batch_co_blocks;  // 128 role blocks + 32 nb attention blocks = one block per CU at nb = 4
    for (int li = 0; li < e->nL; ++li) {
        showo::Layer& l = e->layers[li];
        const showo::DecodeLayerOps w = showo::decode_layer_ops(e, li);  // (a wide batch runs at precision 0: the bf16 images)
        LnGemvBArgs a{e->x, l.ln_w, l.ln_b, e->cfg.ln_eps, H, w.Wqkv, w.bqkv, e->qkv, nullptr, 3 * H, 3 * H, w.W1, w.b1, e->ffn, F, F};
        a.s0 = w.sqkv; a.s1 = w.s1;
        const OutGemvBArgs o{e->x, w.Wd, e->attn, w.bd, H, H, w.W2, e->ffn, w.b2, F, F, H, d->y2, w.sd, w.s2};
        if (d->wide) {  // ln_gemmW -> attention (heads x nb blocks) -> out_gemmW: the MFMA step of decode_wide.hip
            TRY(showo::ln_gemmW(nb, a, d->wws, s));
            if (d->shared) {  // the prefix launch over the engine's cache + the suffix / merge launch over the slots (attn_shared.hip)
                const showo::KVDest kv = showo::kv_decode_cache(e);
                showo::SharedAttnArgs sa{e->qkv, l.qln_w, l.qln_b, l.kln_w, l.kln_b, e->cosT, e->sinT, kv.k + li * kv.k_lstride,
                                         kv.vt + li * kv.v_lstride, kv.Lcap, d->k + li * lstride, d->vt + li * lstride, d->cap,
                                         d->pre_iv[0], d->pre_iv[1], d->pre_iv[2], d->pre_iv[3], d->P, d->base, d->pos_dev, lk_max,
                                         e->attn, d->sws, nb, nH, e->cfg.rotary_dim, e->cfg.ln_eps};
                TRY(showo::attn_decode_shared(sa, s));
                TRY(showo::out_gemmW(nb, o, d->wws, s));
                continue;
            }
            TRY(showo::attn_decode_fused_batch(e->qkv, l.qln_w, l.qln_b, l.kln_w, l.kln_b, e->cosT, e->sinT, d->k + li * lstride,
                                               d->vt + li * lstride, d->iv_dev, e->attn, nb, nH, e->cfg.rotary_dim, e->cfg.ln_eps,
                                               d->pos_dev, lk_max, d->cap, d->cap, s, 0));
            TRY(showo::out_gemmW(nb, o, d->wws, s));
            continue;
        }
        TRY(ln_gemvB(nb, a, s, op));
        if (co) {
            // [ attention of the nb x heads (sequence, head) pairs || fc2 of all nb sequences -> y2 ] -> dense + both residual adds
            // (Phi's block is parallel-residual, models/phi.py:806-835: fc2 does not depend on the attention; decode.hip's batch-1 layer
            // co-schedules the same way)
            showo::DecodePrefetch pf;
            showo::decode_prefetch_plan(e, li, &pf);
            if (q8) pf = showo::DecodePrefetch{};  // (the plan describes the bf16 images, which these launches never stream)
            TRY(showo::attn_decode_co_batch(e->qkv, l.qln_w, l.qln_b, l.kln_w, l.kln_b, e->cosT, e->sinT, d->k + li * lstride,
                                            d->vt + li * lstride, d->iv_dev, e->attn, nb, nH, e->cfg.rotary_dim, e->cfg.ln_eps,
                                            d->pos_dev, lk_max, d->cap, d->cap, o, co_blocks, s, &pf, op));
            TRY(out_dense_y2B(nb, o, s, op));
        } else {
            TRY(showo::attn_decode_fused_batch(e->qkv, l.qln_w, l.qln_b, l.kln_w, l.kln_b, e->cosT, e->sinT, d->k + li * lstride,
                                               d->vt + li * lstride, d->iv_dev, e->attn, nb, nH, e->cfg.rotary_dim, e->cfg.ln_eps,
                                               d->pos_dev, lk_max, d->cap, d->cap, s, op));
            TRY(out_gemvB(nb, o, s, op));
        }
    }
    if (d->wide) {
        LnGemvBArgs h{e->x, e->fln_w, e->fln_b, e->cfg.ln_eps, H, e->wlm, e->blm, nullptr, logits_ws, V, V, nullptr, nullptr, nullptr, 0, 0};
        return showo::ln_gemmW(nb, h, d->wws, s);
    }
    if (op) {  // precision 2: the lm_head is the split-bf16 product (its images stay bf16 (hi, lo) at that precision)
        TRY(showo::decode_split_head(e->x, e->fln_w, e->fln_b, e->cfg.ln_eps, H, e->wlm, e->wlm_lo, e->blm, logits_ws, V, V, nb, s));
    } else {
        const showo::DecodeHeadOps w = showo::decode_head_ops(e);
        LnGemvBArgs h{e->x, e->fln_w, e->fln_b, e->cfg.ln_eps, H, w.W, w.b, nullptr, logits_ws, V, V, nullptr, nullptr, nullptr, 0, 0};
        h.s0 = w.s;
        TRY(ln_gemvB(nb, h, s));
    }
    return 0;
}

// co-scheduled layer (fc2 streams next to the latency-bound attention blocks): Phi-1.5's shape, 2..4 sequences (the fc2 role keeps
// nb x 8192 bf16 activations in LDS); SHOWO_DECODE_BATCH_CO=0 / other shapes: three plain launches per layer
int batch_use_co(showo_engine* e, bool* co) {
    static const int co_on = showo::env_flag("SHOWO_DECODE_BATCH_CO", 1);
    const int nb = e->bd->nb;
    *co = !e->bd->wide && co_on && e->F == 8192 && e->H <= 2048 && nb >= 2 && nb <= 4 && (size_t)nb * e->F * 2 <= 128 * 1024;
    if (*co && !e->bd->y2) TRY(e->alloc(&e->bd->y2, (int64_t)MAXB * e->H));
    return 0;
}

}  // namespace

// tok int64 [nb] (device): in = the token each sequence feeds first (e.g. the arg-max of its prefill logits), out = the last tokens
// produced; out_tokens int64 [nb, n_steps] (device); logits_ws fp32 [nb, vocab] (device).  Every sequence advances n_steps tokens
// (the caller cuts each row at its <eot>, like the chunked batch-1 loop of Showo.mmu_generate).
extern "C" int showo_engine_batch_decode_greedy(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws,
                                                int use_graph, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!e || !e->bd || e->bd->nb == 0) return set_error_msg(1, "batch_decode_greedy: showo_engine_batch_begin + _batch_prefill first");
    auto* d = e->bd;
    const int nb = d->nb, H = e->H, V = e->V;
    if (!tok || !out_tokens || !logits_ws || n_steps < 1) return set_error_msg(1, "batch_decode_greedy: bad arguments");
    TRY(batch_decode_checks(e, "batch_decode_greedy"));
    const int op = e->precision == 2 ? SHOWO_OP_F16 : SHOWO_OP_BF16;
    int lk_max = 0;
    int P0[MAXB];
    for (int b = 0; b < nb; ++b) {
        P0[b] = d->cache_len[b];
        if (P0[b] + n_steps > d->abs_cap() || P0[b] + n_steps > e->cfg.max_pos) return set_error_msg(5, "batch_decode_greedy: cache full");
        lk_max = lk_max > P0[b] + n_steps ? lk_max : P0[b] + n_steps;
    }
    SHOWO_CHECK_HIP(hipMemcpyAsync(d->pos_dev, P0, sizeof(int) * nb, hipMemcpyHostToDevice, s));
    SHOWO_CHECK_HIP(hipMemcpyAsync(d->base_dev, P0, sizeof(int) * nb, hipMemcpyHostToDevice, s));
    SHOWO_CHECK_HIP(hipMemcpyAsync(d->L0_dev, d->prompt_len, sizeof(int) * nb, hipMemcpyHostToDevice, s));
    SHOWO_CHECK_HIP(hipMemcpyAsync(d->last_iv_dev, d->last_iv, sizeof(int32_t) * 4 * nb, hipMemcpyHostToDevice, s));
    SHOWO_CHECK_HIP(hipStreamSynchronize(s));  // P0 is a host temporary of this call
    TRY(showo_embed_f32(tok, e->embed, e->x, nb, H, V, s));
    batch_iv_kernel<<<1, 64, 0, s>>>(d->last_iv_dev, d->L0_dev, d->pos_dev, d->iv_dev, nb);
    SHOWO_CHECK_HIP(hipGetLastError());
    bool co = false;
    TRY(batch_use_co(e, &co));
    auto one = [&]() -> int {
        TRY(batch_step_layers(e, op, co, lk_max, logits_ws, s));
        greedy_seam_rows_kernel<<<dim3(nb), dim3(1024), 0, s>>>(logits_ws, V, tok, out_tokens, n_steps, d->pos_dev, d->base_dev, e->embed, e->x,
                                                               H, d->last_iv_dev, d->L0_dev, d->iv_dev);
        SHOWO_CHECK_HIP(hipGetLastError());
        return 0;
    };
    TRY(showo::replay_steps(one, n_steps, use_graph != 0, s));
    for (int b = 0; b < nb; ++b) d->cache_len[b] = P0[b] + n_steps;
    return 0;
}

// The sampled form with a per-slot stop (include/showo_hip.h): slot b draws with its own top_k / temperature / seed / draw index and
// emits at most budget[b] tokens, stopping early after `eot`; a stopped or idle slot keeps decoding a fixed row in place so that the
// captured step stays the same for every slot.  Its cache length advances by what it produced.
// top_p == NULL: no slot filters (showo_engine_batch_decode_sample); else host float [nb], per slot >= 1 (off) or in (0, 1).
// adj != NULL (showo_engine_batch_decode_sample_adj): one adjust launch for all nb slots between the layers and the seam reads
// logits_ws, marks tok[b] of the slots whose SlotDraw.active is set (an idle slot is skipped) and writes adj->ws, which the seam reads
// instead; logprob_slots_kernel keeps reading logits_ws.  The <= 8 slots, the wide slots and the shared-prefix slots share this seam.
// seq != NULL (showo_engine_batch_decode_sample_seq; needs adj): one ban launch for all nb slots directly behind the adjust launch
// works on adj->ws in place and appends tok[b] of the active slots to their device histories (seq_rules.hip).
static int batch_decode_sample(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, const int* top_k,
                               const float* top_p, const float* temperature, const uint64_t* seed, const int* draw0,
                               const float* const* exp_noise, const int* budget, int64_t eot, int* produced, int use_graph, void* stream,
                               float* lps = nullptr, int32_t* ranks = nullptr, const showo::LogitAdjust* adj = nullptr,
                               const showo_seq_rules* seq = nullptr) {
    hipStream_t s = (hipStream_t)stream;
    if (!e || !e->bd || e->bd->nb == 0) return set_error_msg(1, "batch_decode_sample: showo_engine_batch_begin + _batch_prefill first");
    auto* d = e->bd;
    const int nb = d->nb, H = e->H, V = e->V;
    if (!tok || !out_tokens || !logits_ws || n_steps < 1 || !top_k || !temperature || !seed || !draw0 || !budget || !produced)
        return set_error_msg(1, "batch_decode_sample: bad arguments");
    TRY(batch_decode_checks(e, "batch_decode_sample"));
    if (adj) {
        if (!adj->ws || adj->ws == logits_ws) return set_error_msg(1, "batch_decode_sample_adj: needs an adj_ws [nb, V] of its own");
        TRY(showo::logits_adjust_check(nb, V, adj->seen, adj->seen_ld, adj->penalty, "batch_decode_sample_adj"));
        if (seq) TRY(showo::seq_rules_check(nb, seq, "batch_decode_sample_seq"));
    } else if (seq) {
        return set_error_msg(1, "batch_decode_sample_seq: the rules work on the adjusted rows");
    }
    const int op = e->precision == 2 ? SHOWO_OP_F16 : SHOWO_OP_BF16;
    // positions stay below lim: the cache capacity and the rotary tables (max_position_embeddings)
    const int lim = d->abs_cap() < e->cfg.max_pos ? d->abs_cap() : e->cfg.max_pos;
    int lk_max = 0;
    int P0[MAXB], pos0[MAXB];
    SlotDraw sd[MAXB];
    bool nucleus = false;  // some decoding, sampling slot filters by top_p
    for (int b = 0; b < nb; ++b) {
        if (budget[b] < 0 || draw0[b] < 0) return set_error_msg(1, "batch_decode_sample: budget and draw0 must be >= 0");
        if (top_p && !(top_p[b] > 0.f)) return set_error_msg(1, "batch_decode_sample: top_p must be > 0 (>= 1: no nucleus filter)");
        sd[b].top_p = top_p && top_p[b] < 1.f ? top_p[b] : 1.f;
        nucleus = nucleus || (budget[b] > 0 && top_k[b] != 1 && sd[b].top_p < 1.f);
        if (budget[b] > 0 && top_k[b] != 1 && !(temperature[b] > 0.f)) return set_error_msg(1, "batch_decode_sample: temperature must be > 0");
        P0[b] = d->cache_len[b];
        const int emit = budget[b] < n_steps ? budget[b] : n_steps;  // what the slot can still emit in this call
        if (P0[b] + emit > lim) return set_error_msg(5, "batch_decode_sample: cache full");
        pos0[b] = P0[b] < lim - 1 ? P0[b] : lim - 1;
        // highest position + 1 the slot reaches: P0 + emit while it decodes, one more once it idles after its stop (below lim)
        const int reach = P0[b] + emit + 1 < lim ? P0[b] + emit + 1 : lim;
        lk_max = lk_max > reach ? lk_max : reach;
        sd[b].noise = exp_noise ? exp_noise[b] : nullptr;
        sd[b].seed = seed[b];
        sd[b].temperature = temperature[b];
        sd[b].top_k = top_k[b];
        sd[b].draw0 = draw0[b];
        sd[b].budget = budget[b];
        sd[b].produced = 0;
        sd[b].step = 0;
        sd[b].active = budget[b] > 0;
    }
    if (!d->slots_dev) TRY(e->alloc(&d->slots_dev, MAXB));
    SHOWO_CHECK_HIP(hipMemcpyAsync(d->pos_dev, pos0, sizeof(int) * nb, hipMemcpyHostToDevice, s));
    SHOWO_CHECK_HIP(hipMemcpyAsync(d->L0_dev, d->prompt_len, sizeof(int) * nb, hipMemcpyHostToDevice, s));
    SHOWO_CHECK_HIP(hipMemcpyAsync(d->last_iv_dev, d->last_iv, sizeof(int32_t) * 4 * nb, hipMemcpyHostToDevice, s));
    SHOWO_CHECK_HIP(hipMemcpyAsync(d->slots_dev, sd, sizeof(SlotDraw) * nb, hipMemcpyHostToDevice, s));
    SHOWO_CHECK_HIP(hipStreamSynchronize(s));  // pos0 / sd are host temporaries of this call
    slot_embed_kernel<<<dim3(nb), dim3(256), 0, s>>>(tok, d->slots_dev, e->embed, e->x, H, V);
    batch_iv_kernel<<<1, 64, 0, s>>>(d->last_iv_dev, d->L0_dev, d->pos_dev, d->iv_dev, nb);
    SHOWO_CHECK_HIP(hipGetLastError());
    bool co = false;
    TRY(batch_use_co(e, &co));
    auto one = [&]() -> int {
        TRY(batch_step_layers(e, op, co, lk_max, logits_ws, s));
        const float* pick = logits_ws;
        if (adj) {
            const int* active = reinterpret_cast<const int*>(reinterpret_cast<const char*>(d->slots_dev) + offsetof(SlotDraw, active));
            TRY(showo::logits_adjust_launch(logits_ws, V, nb, V, adj->seen, adj->seen_ld, tok, adj->penalty, adj->bias, active,
                                            (int)(sizeof(SlotDraw) / sizeof(int)), adj->ws, V, s));
            if (seq) TRY(showo::seq_ban_launch(adj->ws, V, nb, V, seq, tok, active, (int)(sizeof(SlotDraw) / sizeof(int)), s));
            pick = adj->ws;
        }
        if (nucleus)
            sample_seam_rows_kernel<true><<<dim3(nb), dim3(1024), 0, s>>>(pick, V, eot, tok, out_tokens, n_steps, d->pos_dev, lim,
                                                                         d->slots_dev, e->embed, e->x, H, d->last_iv_dev, d->L0_dev, d->iv_dev);
        else
            sample_seam_rows_kernel<false><<<dim3(nb), dim3(1024), 0, s>>>(pick, V, eot, tok, out_tokens, n_steps, d->pos_dev, lim,
                                                                          d->slots_dev, e->embed, e->x, H, d->last_iv_dev, d->L0_dev, d->iv_dev);
        if (lps) logprob_slots_kernel<<<dim3(nb), dim3(1024), 0, s>>>(logits_ws, V, out_tokens, n_steps, d->slots_dev, lps, ranks);
        SHOWO_CHECK_HIP(hipGetLastError());
        return 0;
    };
    TRY(showo::replay_steps(one, n_steps, use_graph != 0, s));
    SHOWO_CHECK_HIP(hipMemcpyAsync(sd, d->slots_dev, sizeof(SlotDraw) * nb, hipMemcpyDeviceToHost, s));
    SHOWO_CHECK_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < nb; ++b) {
        produced[b] = sd[b].produced;
        d->cache_len[b] = P0[b] + sd[b].produced;
    }
    return 0;
}

extern "C" int showo_engine_batch_decode_sample(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws,
                                                const int* top_k, const float* temperature, const uint64_t* seed, const int* draw0,
                                                const float* const* exp_noise, const int* budget, int64_t eot, int* produced,
                                                int use_graph, void* stream) {
    return batch_decode_sample(e, tok, n_steps, out_tokens, logits_ws, top_k, nullptr, temperature, seed, draw0, exp_noise, budget, eot,
                               produced, use_graph, stream);
}

extern "C" int showo_engine_batch_decode_sample_p(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws,
                                                  const int* top_k, const float* top_p, const float* temperature, const uint64_t* seed,
                                                  const int* draw0, const float* const* exp_noise, const int* budget, int64_t eot,
                                                  int* produced, int use_graph, void* stream) {
    if (!top_p) return set_error_msg(1, "batch_decode_sample_p: bad arguments");
    return batch_decode_sample(e, tok, n_steps, out_tokens, logits_ws, top_k, top_p, temperature, seed, draw0, exp_noise, budget, eot,
                               produced, use_graph, stream);
}


// showo_engine_batch_decode_sample_p (top_p may be NULL: no slot filters) that also reports how probable every token was
extern "C" int showo_engine_batch_decode_sample_lp(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws,
                                                   const int* top_k, const float* top_p, const float* temperature, const uint64_t* seed,
                                                   const int* draw0, const float* const* exp_noise, const int* budget, int64_t eot,
                                                   int* produced, float* logprobs, int32_t* ranks, int use_graph, void* stream) {
    return batch_decode_sample(e, tok, n_steps, out_tokens, logits_ws, top_k, top_p, temperature, seed, draw0, exp_noise, budget, eot,
                               produced, use_graph, stream, logprobs, logprobs ? ranks : nullptr);
}

// showo_engine_batch_decode_sample_lp with the logit adjustment in front of the seam (include/showo_hip.h, "Logit adjustment")
extern "C" int showo_engine_batch_decode_sample_adj(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws,
                                                    const int* top_k, const float* top_p, const float* temperature, const uint64_t* seed,
                                                    const int* draw0, const float* const* exp_noise, const int* budget, int64_t eot,
                                                    int* produced, float* logprobs, int32_t* ranks, uint32_t* seen, int64_t seen_ld,
                                                    const float* penalty, const float* const* bias, float* adj_ws, int use_graph,
                                                    void* stream) {
    const showo::LogitAdjust adj{seen, seen_ld, penalty, bias, adj_ws};
    return batch_decode_sample(e, tok, n_steps, out_tokens, logits_ws, top_k, top_p, temperature, seed, draw0, exp_noise, budget, eot,
                               produced, use_graph, stream, logprobs, logprobs ? ranks : nullptr, &adj);
}

// showo_engine_batch_decode_sample_adj with the sequence rules behind the adjustment (include/showo_hip.h, "Sequence rules")
extern "C" int showo_engine_batch_decode_sample_seq(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws,
                                                    const int* top_k, const float* top_p, const float* temperature, const uint64_t* seed,
                                                    const int* draw0, const float* const* exp_noise, const int* budget, int64_t eot,
                                                    int* produced, float* logprobs, int32_t* ranks, uint32_t* seen, int64_t seen_ld,
                                                    const float* penalty, const float* const* bias, float* adj_ws,
                                                    const showo_seq_rules* rules, int use_graph, void* stream) {
    if (!rules) return set_error_msg(1, "batch_decode_sample_seq: bad arguments");
    const showo::LogitAdjust adj{seen, seen_ld, penalty, bias, adj_ws};
    return batch_decode_sample(e, tok, n_steps, out_tokens, logits_ws, top_k, top_p, temperature, seed, draw0, exp_noise, budget, eot,
                               produced, use_graph, stream, logprobs, logprobs ? ranks : nullptr, &adj, rules);
}

// ---- beam search (include/showo_hip.h, "Beam search") -----------------------------------------------------------------------
namespace {
// a regular batch whose slots all hold caches of one length (forks of the engine's cache): *P = that length
int beam_checks(showo_engine* e, const char* what, int* P) {
    auto* d = e->bd;
    auto fail = [&](int code, const char* msg) { return set_error_msg(code, (std::string(what) + ": " + msg).c_str()); };
    if (d->wide || d->shared) return fail(1, "beams run on a regular batch (showo_engine_batch_begin), not on a wide or shared-prefix one");
    if (e->V < 2 * d->nb) return fail(1, "the vocabulary must hold 2 x beams tokens");
    TRY(batch_decode_checks(e, what));
    for (int b = 1; b < d->nb; ++b)
        if (d->cache_len[b] != d->cache_len[0] || d->prompt_len[b] != d->prompt_len[0])
            return fail(1, "the slots hold caches of unequal length (fork every slot from one cache)");
    *P = d->cache_len[0];
    return 0;
}

int beam_upload_positions(showo_engine* e, int P, hipStream_t s) {
    auto* d = e->bd;
    int P0[NARROW_B];
    for (int b = 0; b < d->nb; ++b) P0[b] = P;
    SHOWO_CHECK_HIP(hipMemcpyAsync(d->pos_dev, P0, sizeof(int) * d->nb, hipMemcpyHostToDevice, s));
    SHOWO_CHECK_HIP(hipMemcpyAsync(d->L0_dev, d->prompt_len, sizeof(int) * d->nb, hipMemcpyHostToDevice, s));
    SHOWO_CHECK_HIP(hipMemcpyAsync(d->last_iv_dev, d->last_iv, sizeof(int32_t) * 4 * d->nb, hipMemcpyHostToDevice, s));
    SHOWO_CHECK_HIP(hipStreamSynchronize(s));  // P0 is a host temporary of this call
    return 0;
}

showo::BeamSeamArgs beam_seam_args(showo_engine* e, const float* logits, int32_t* state, int64_t eot, int early, int first, int lim,
                                   int32_t* tr_parent, int32_t* tr_token, float* tr_cum, float* tr_lp, void* hyp) {
    auto* d = e->bd;
    return showo::BeamSeamArgs{logits, e->V, e->V, d->beam_norm, d->beam_cand, d->nb, eot, early, first, state, tr_parent, tr_token, tr_cum,
                               tr_lp, reinterpret_cast<showo::BeamHyp*>(hyp), d->pos_dev, lim, e->embed, e->x, e->H, d->last_iv_dev,
                               d->L0_dev, d->iv_dev};
}
}  // namespace

extern "C" int showo_engine_batch_beam_begin(showo_engine* e, int32_t* state, int max_new, const float* logits_row, int64_t eot,
                                             float length_penalty, int early_stopping, int32_t* tr_parent, int32_t* tr_token, float* tr_cum,
                                             float* tr_lp, void* hyp, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!e || !e->bd || e->bd->nb == 0) return set_error_msg(1, "batch_beam_begin: showo_engine_batch_begin + _batch_fork first");
    auto* d = e->bd;
    if (!state || !logits_row || !tr_parent || !tr_token || !tr_cum || !tr_lp || !hyp || max_new < 1 || !std::isfinite(length_penalty) ||
        ((uintptr_t)state & 7))
        return set_error_msg(1, "batch_beam_begin: bad arguments");
    int P = 0;
    TRY(beam_checks(e, "batch_beam_begin", &P));
    const int nb = d->nb, V = e->V;
    const int lim = d->abs_cap() < e->cfg.max_pos ? d->abs_cap() : e->cfg.max_pos;
    if (P + max_new - 1 > lim) return set_error_msg(5, "batch_beam_begin: cache full");
    if (!d->beam_norm) {
        TRY(e->alloc(&d->beam_norm, 2 * showo::BEAM_MAX));
        TRY(e->alloc(&d->beam_ws, 4 * showo::BEAM_MAX * showo::BEAM_MAX));
        TRY(e->alloc(&d->beam_cand, 2 * showo::BEAM_MAX));
        TRY(e->alloc(&d->beam_ktab, showo::BEAM_MAX));
        TRY(e->alloc(&d->beam_vtab, showo::BEAM_MAX));
    }
    const int64_t need = (int64_t)nb * e->nL * e->nH * 64 * showo::kv_permute_pitch(max_new);
    if (need > d->beam_stage_elems) {
        SHOWO_CHECK_HIP(hipDeviceSynchronize());
        e->release(&d->beam_stage_k);
        e->release(&d->beam_stage_vt);
        d->beam_stage_elems = 0;
        TRY(e->alloc(&d->beam_stage_k, need));
        TRY(e->alloc(&d->beam_stage_vt, need));
        d->beam_stage_elems = need;
    }
    d->beam_state = nullptr;
    std::vector<int32_t> hd(showo::BEAM_STATE_HEAD + max_new + 1, 0);
    auto bits = [](float f) { int32_t i; memcpy(&i, &f, 4); return i; };
    hd[showo::BS_WORST] = bits(-INFINITY);
    hd[showo::BS_MAXNEW] = max_new;
    hd[showo::BS_B] = nb;
    for (int b = 0; b < showo::BEAM_MAX; ++b) hd[showo::BS_PARENT + b] = b;
    for (int len = 1; len <= max_new; ++len) hd[showo::BEAM_STATE_HEAD + len] = bits((float)std::pow((double)len, (double)length_penalty));
    const int64_t per_seq = (int64_t)e->nH * d->cap * 64;
    uint16_t *kt[showo::BEAM_MAX], *vt[showo::BEAM_MAX];
    for (int b = 0; b < showo::BEAM_MAX; ++b) {
        kt[b] = reinterpret_cast<uint16_t*>(d->k + (b < nb ? b : 0) * per_seq);
        vt[b] = reinterpret_cast<uint16_t*>(d->vt + (b < nb ? b : 0) * per_seq);
    }
    SHOWO_CHECK_HIP(hipMemcpyAsync(state, hd.data(), hd.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    SHOWO_CHECK_HIP(hipMemcpyAsync(d->beam_ktab, kt, sizeof(kt), hipMemcpyHostToDevice, s));
    SHOWO_CHECK_HIP(hipMemcpyAsync(d->beam_vtab, vt, sizeof(vt), hipMemcpyHostToDevice, s));
    TRY(beam_upload_positions(e, P, s));  // (synchronises: hd, kt and vt are host temporaries)
    // the first step: the 2B best tokens of the prefill's one row, cumulative score 0
    TRY(showo::beam_select_launch(logits_row, V, 1, V, reinterpret_cast<const float*>(state + showo::BS_CUM), nb, d->beam_norm, d->beam_cand,
                                  d->beam_ws, s));
    TRY(showo::beam_seam_launch(beam_seam_args(e, logits_row, state, eot, early_stopping != 0, 1, lim, tr_parent, tr_token, tr_cum, tr_lp, hyp),
                                s));
    d->beam_state = state;
    d->beam_P0 = P;
    d->beam_span = max_new;
    return 0;
}

extern "C" int showo_engine_batch_decode_beam(showo_engine* e, int32_t* state, int n_steps, int64_t eot, float length_penalty,
                                              int early_stopping, float* logits_ws, int32_t* tr_parent, int32_t* tr_token, float* tr_cum,
                                              float* tr_lp, void* hyp, int use_graph, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!e || !e->bd || e->bd->nb == 0) return set_error_msg(1, "batch_decode_beam: showo_engine_batch_begin + _batch_fork first");
    auto* d = e->bd;
    if (!state || !logits_ws || !tr_parent || !tr_token || !tr_cum || !tr_lp || !hyp || n_steps < 1 || !std::isfinite(length_penalty))
        return set_error_msg(1, "batch_decode_beam: bad arguments");
    if (d->beam_state != state) return set_error_msg(1, "batch_decode_beam: showo_engine_batch_beam_begin on this state block first");
    int P = 0;
    TRY(beam_checks(e, "batch_decode_beam", &P));
    const int nb = d->nb, H = e->H, V = e->V;
    int32_t hd[showo::BEAM_STATE_HEAD];
    SHOWO_CHECK_HIP(hipMemcpyAsync(hd, state, sizeof(hd), hipMemcpyDeviceToHost, s));
    SHOWO_CHECK_HIP(hipStreamSynchronize(s));
    const int t0 = hd[showo::BS_T], max_new = hd[showo::BS_MAXNEW];
    if (hd[showo::BS_B] != nb || max_new != d->beam_span || t0 < 1 || t0 > max_new || P != d->beam_P0 + t0 - 1)
        return set_error_msg(1, "batch_decode_beam: the state block does not belong to the batch as it stands");
    if (hd[showo::BS_DONE] || t0 >= max_new) return 0;  // the search is over: nothing to run
    const int n = n_steps < max_new - t0 ? n_steps : max_new - t0;
    const int lim = d->abs_cap() < e->cfg.max_pos ? d->abs_cap() : e->cfg.max_pos;
    if (P + n > lim) return set_error_msg(5, "batch_decode_beam: cache full");
    const int lk_max = P + n + 1 < lim ? P + n + 1 : lim;
    const int op = e->precision == 2 ? SHOWO_OP_F16 : SHOWO_OP_BF16;
    TRY(beam_upload_positions(e, P, s));
    TRY(showo_embed_f32(reinterpret_cast<const int64_t*>(state + showo::BS_TOK), e->embed, e->x, nb, H, V, s));
    batch_iv_kernel<<<1, 64, 0, s>>>(d->last_iv_dev, d->L0_dev, d->pos_dev, d->iv_dev, nb);
    SHOWO_CHECK_HIP(hipGetLastError());
    bool co = false;
    TRY(batch_use_co(e, &co));
    const int64_t lstride = (int64_t)nb * e->nH * d->cap * 64;
    const showo::BeamSeamArgs sa = beam_seam_args(e, logits_ws, state, eot, early_stopping != 0, 0, lim, tr_parent, tr_token, tr_cum, tr_lp, hyp);
    auto one = [&]() -> int {
        TRY(batch_step_layers(e, op, co, lk_max, logits_ws, s));
        TRY(showo::beam_select_launch(logits_ws, V, nb, V, reinterpret_cast<const float*>(state + showo::BS_CUM), nb, d->beam_norm,
                                      d->beam_cand, d->beam_ws, s));
        TRY(showo::beam_seam_launch(sa, s));
        // every new beam inherits rows [P0, position) of its parent (the seam has advanced the positions; idle: the identity map)
        return showo_kv_permute_rows(d->beam_ktab, d->beam_vtab, d->cap, lstride, lstride, e->nL, e->nH, nb, state + showo::BS_PARENT,
                                     d->beam_P0, d->pos_dev, reinterpret_cast<uint16_t*>(d->beam_stage_k),
                                     reinterpret_cast<uint16_t*>(d->beam_stage_vt), d->beam_span, s);
    };
    TRY(showo::replay_steps(one, n, use_graph != 0, s));
    SHOWO_CHECK_HIP(hipMemcpyAsync(hd, state, sizeof(hd), hipMemcpyDeviceToHost, s));
    SHOWO_CHECK_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < nb; ++b) d->cache_len[b] = P + (hd[showo::BS_T] - t0);
    return 0;
}

// ---- test hooks: the dot2 GEMV kernels alone (tests/test_decode_narrow_kernels_gpu.py) ---------------------------------------------
// Each hook checks everything the engine guarantees its own launches (shapes of decode_fused_shapes_ok, the int8 forms' % 16 rule, the
// slot range, 16-byte operand alignment) and refuses before any launch; then it calls the launcher the engine calls.
static bool hook_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int showo_decode_narrow_ln_gemv(int kernel, int nb, int op, const float* x, const float* lnw, const float* lnb, float eps, int H,
                                           const void* W0, const uint16_t* W0lo, const float* s0, const float* b0, uint16_t* out0,
                                           float* outf, int N0, int ld0, const void* W1, const float* s1, const float* b1, uint16_t* out1,
                                           int N1, int ld1, void* stream) {
    const char* who = "showo_decode_narrow_ln_gemv";
    auto bad = [&](const char* what) { return set_error_msg(1, (std::string(who) + ": " + what).c_str()); };
    if (kernel != 0 && kernel != 1) return bad("kernel is 0 (ln_gemv2, one row) or 1 (ln_gemvB)");
    if (op != SHOWO_OP_BF16 && op != SHOWO_OP_F16) return bad("op must be SHOWO_OP_BF16 or SHOWO_OP_F16");
    if (kernel == 0 ? nb != 1 : (nb < 1 || nb > NARROW_B)) return bad("nb is 1 for ln_gemv2 and 1..8 for ln_gemvB");
    if (!x || !lnw || !lnb || !W0 || !b0 || (!out0) == (!outf)) return bad("x, lnw, lnb, W0, b0 and exactly one of out0 / outf required");
    if (N0 < 1 || N1 < 0 || ld0 < N0 || (N1 > 0 && (!W1 || !b1 || !out1 || ld1 < N1))) return bad("N0 >= 1, ld >= N, and W1 / b1 / out1 with N1 > 0");
    if (H < 8 || H > 2048 || (H % 8)) return bad("H must be a multiple of 8 in 8..2048");
    if ((s1 && !s0) || (s0 && (op || W0lo || (N1 > 0 && !s1) || (H % 16))))
        return bad("int8 weights take bf16 activations, a scale per matrix, no split head and H % 16 == 0");
    if (W0lo && (kernel != 1 || !outf || N1 > 0 || op)) return bad("the split head is ln_gemvB with bf16 halves, fp32 logits and no second matrix");
    if (!hook_al16(x) || !hook_al16(lnw) || !hook_al16(lnb) || !hook_al16(W0) || !hook_al16(W0lo) || (N1 > 0 && !hook_al16(W1)))
        return bad("x, lnw, lnb and the weight matrices must be 16-byte aligned");
    LnGemvBArgs g{x, lnw, lnb, eps, H, reinterpret_cast<const bf16_t*>(W0), b0, outf ? nullptr : out0, outf, N0, ld0,
                  N1 > 0 ? reinterpret_cast<const bf16_t*>(W1) : nullptr, N1 > 0 ? b1 : nullptr, N1 > 0 ? out1 : nullptr, N1, ld1};
    g.W0lo = W0lo;
    g.s0 = s0;
    g.s1 = N1 > 0 ? s1 : nullptr;
    if (kernel == 0) return showo::decode_ln_gemv2(g, (hipStream_t)stream, op);
    return ln_gemvB(nb, g, (hipStream_t)stream, op, W0lo != nullptr);
}

extern "C" int showo_decode_narrow_out_gemv(int kernel, int nb, int mode, int op, float* x, const void* W0, const uint16_t* a0, const float* s0,
                                            const float* b0, int K0, int lda0, const void* W1, const uint16_t* a1, const float* s1,
                                            const float* b1, int K1, int lda1, int N, float* y2, void* stream) {
    const char* who = "showo_decode_narrow_out_gemv";
    auto bad = [&](const char* what) { return set_error_msg(1, (std::string(who) + ": " + what).c_str()); };
    if (kernel < 0 || kernel > 2) return bad("kernel is 0 (out_gemv2, one row), 1 (out_gemvB) or 2 (out_dense_y2B)");
    if (op != SHOWO_OP_BF16 && op != SHOWO_OP_F16) return bad("op must be SHOWO_OP_BF16 or SHOWO_OP_F16");
    if (mode < 0 || mode > 2 || (kernel == 1 && mode != 0) || (kernel == 2 && mode != 2))
        return bad("mode 0..2 for out_gemv2, 0 for out_gemvB, 2 for out_dense_y2B");
    if (kernel == 0 ? nb != 1 : kernel == 1 ? (nb < 1 || nb > NARROW_B) : (nb < 2 || nb > 4))
        return bad("nb is 1 for out_gemv2, 1..8 for out_gemvB and 2..4 for out_dense_y2B");
    const bool use0 = mode != 1, use1 = mode != 2;  // the dense half / the fc2 half
    if (N < 1 || (use0 && (!x || !W0 || !a0 || !b0)) || (use1 && (!W1 || !a1 || !b1)) || (mode && !y2))
        return bad("N >= 1, x / W0 / a0 / b0 (modes 0, 2), W1 / a1 / b1 (modes 0, 1) and y2 (modes 1, 2) required");
    if (use0 && (K0 < 8 || K0 > 2048 || (K0 % 8) || lda0 < K0 || (lda0 % 8))) return bad("K0 must be a multiple of 8 in 8..2048, lda0 % 8 == 0 >= K0");
    if (use1 && (K1 < 8 || K1 > 8192 || (K1 % 8) || lda1 < K1 || (lda1 % 8))) return bad("K1 must be a multiple of 8 in 8..8192, lda1 % 8 == 0 >= K1");
    const bool q8 = (use0 && s0) || (use1 && s1);
    if (q8 && (op || (use0 && (!s0 || (K0 % 16))) || (use1 && (!s1 || (K1 % 16)))))
        return bad("int8 weights take bf16 activations, a scale per matrix and K % 16 == 0");
    if ((use0 && (!hook_al16(W0) || !hook_al16(a0))) || (use1 && (!hook_al16(W1) || !hook_al16(a1))))
        return bad("weights and activations must be 16-byte aligned");
    const bf16_t* w0 = use0 ? reinterpret_cast<const bf16_t*>(W0) : nullptr;
    const bf16_t* w1 = use1 ? reinterpret_cast<const bf16_t*>(W1) : nullptr;
    const int k0 = use0 ? K0 : 0, k1 = use1 ? K1 : 0;
    if (kernel == 0) {
        const OutGemvArgs g{x, w0, use0 ? a0 : nullptr, b0, k0, w1, use1 ? a1 : nullptr, b1, k1, N, y2, use0 ? s0 : nullptr, use1 ? s1 : nullptr};
        return showo::decode_out_gemv2(g, (hipStream_t)stream, mode, op);
    }
    const OutGemvBArgs g{x, w0, use0 ? a0 : nullptr, b0, k0, lda0, w1, use1 ? a1 : nullptr, b1, k1, lda1, N, y2, use0 ? s0 : nullptr,
                         use1 ? s1 : nullptr};
    if (kernel == 1) return out_gemvB(nb, g, (hipStream_t)stream, op);
    return out_dense_y2B(nb, g, (hipStream_t)stream, op);
}
