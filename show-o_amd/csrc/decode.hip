// Fused AR-decode layer for one new token (B = 1, L = 1): three launches per transformer layer instead of seven.
//
//   reference path per layer (models/phi.py:806-835 parallel block, 1 token against the KV cache, modeling_showo.py:190-240):
//     LN -> qkv projection -> q/k LayerNorm + RoPE + cache append -> attention -> dense(+x) ; LN -> fc1+gelu -> fc2(+x)
//   here:
//     ln_gemv2_kernel   x -> LayerNorm (in LDS, every block) -> qkv row (bf16) and gelu(fc1) row (bf16)       56 MB of weights
//     attn_decode_kernel<FUSED> (attention.hip): prep of the new token + cache append + single-query attention
//     out_gemv2_kernel  x += dense(attn) + bd ; x += fc2(ffn) + b2                                             40 MB of weights
//
// All three are HBM-streaming kernels: every weight byte is read exactly once per token (2.4 GB over 24 layers + 240 MB
// lm_head), a wave owns whole output columns and splits K over its lanes exactly like gemv_kernel (gemm.hip) -- same
// lane split, same accumulation order, same epilogue expressions -- so the fused step is bit-identical to the unfused one.
// The next 4 x 16-B weight loads of a wave are always in flight while the current ones are multiplied.
//
// Host side of this file: decode_layer_ops / decode_head_ops (which weight images a layer's launches stream), the launchers
// decode_ln_gemv2 / decode_out_gemv2 (argument structs of decode_common.h), and decode_layers_b1, the ONE batch-1 layer step that
// run_layers (engine.hip) calls for a one-token step.  The KV cache and the token loop around it are in decode_engine.hip.
#include "common.h"
#include "engine.h"
#include "decode_common.h"
#include "../../include/showo_hip.h"

using namespace showo;

namespace {

struct LnGemvArgs {
    const float* x;     // [H] fp32 residual stream row
    const float *lnw, *lnb;
    float eps;
    int H;
    const bf16_t* W0;   // [N0, H]  -> out0 = bf16(W0 h + b0)   or, when outf != nullptr, outf = fp32(W0 h + b0)
    const float* b0;
    bf16_t* out0;
    float* outf;
    int N0;
    const bf16_t* W1;   // [N1, H]  -> out1 = bf16(gelu_new(W1 h + b1))
    const float* b1;
    bf16_t* out1;
    int N1;
    const float* s0 = nullptr;  // Q8 instances (precision 3): W0 / W1 are int8 row-major, s0 [N0] / s1 [N1] their row scales
    const float* s1 = nullptr;
};

// R = weight rows in flight per wave (2; see decode_ln_gemv2 for the measurement of 4); larger matrices (lm_head) loop and refill.
// Q8: int8 weight rows (8-byte loads, exact conversion to bf16, the same dot2 chain) and acc * scale[n] in front of the epilogue.
template <int R, bool F16 = false, bool Q8 = false>
__global__ __launch_bounds__(256) void ln_gemv2_kernel(LnGemvArgs g) {  // H <= 2048: one 4-load group covers a weight row
    extern __shared__ bf16_t sh[];  // normalised row, bf16 like showo_layernorm_f32_bf16's output
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: weight-row bases in SGPRs
    const int H = g.H, Ntot = g.N0 + g.N1;
    const int stride = gridDim.x * 4;
    int n = blockIdx.x * 4 + wave;
    auto rowp = [&](int c) { return c < g.N0 ? wrow<Q8>(g.W0, c, H) : wrow<Q8>(g.W1, c - g.N0, H); };
    // the first R weight rows of the wave are in flight before anything else: they do not depend on the LayerNorm
    typename WVec<Q8>::type br[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (n + r * stride < Ntot) load4(rowp(n + r * stride), lane * 8, H, br[r]);
    {   // every wave repeats layernorm_kernel's statistics (same lane split, same expressions => same bits) on a register
        // copy of the row (one global round trip instead of three), then writes a quarter of the normalised row to LDS.
        // (Measured: a 1024-thread block sharing one wave's statistics is slower, 23 us vs 19 us -- two barriers and a second
        // pass over x cost more than the redundant reductions.)
        float4 xv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = lane * 4 + j * 256;
            xv[j] = i < H ? *reinterpret_cast<const float4*>(g.x + i) : make_float4(0.f, 0.f, 0.f, 0.f);
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
            if ((j & 3) == wave && i < H) {
                const float4 v = xv[j];
                const float4 w = *reinterpret_cast<const float4*>(g.lnw + i);
                const float4 bb = *reinterpret_cast<const float4*>(g.lnb + i);
                uint2 o;
                o.x = Op16<F16>::pack2((v.x - mean) * rstd * w.x + bb.x, (v.y - mean) * rstd * w.y + bb.y);
                o.y = Op16<F16>::pack2((v.z - mean) * rstd * w.z + bb.z, (v.w - mean) * rstd * w.w + bb.w);
                *reinterpret_cast<uint2*>(sh + i) = o;
            }
        }
    }
    __syncthreads();
    auto finish = [&](int c, float acc) {
        acc = wave_sum_swap(acc);
        if (lane == 0) {
            if (c < g.N0) {
                const float a = q8_scale<Q8>(acc, g.s0, c);
                const float v = a + g.b0[c];
                if (g.outf) g.outf[c] = v;
                else g.out0[c] = Op16<F16>::cvt(v);
            } else {
                const float a = q8_scale<Q8>(acc, g.s1, c - g.N0);
                g.out1[c - g.N0] = Op16<F16>::cvt(gelu_new_fast(a + g.b1[c - g.N0]));
            }
        }
    };
    while (n < Ntot) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int c = n + r * stride;
            if (c < Ntot) {
                const float acc = fma4<F16>(br[r], sh, lane * 8, H, 0.f);
                if (c + R * stride < Ntot) load4(rowp(c + R * stride), lane * 8, H, br[r]);
                finish(c, acc);
            }
        }
        n += R * stride;
    }
}

// C = 2048-element chunks per output column (dense chunks first, then fc2 chunks), ALL of them in flight per wave: a wave
// streams 20 KB per column at the real shape and only 8 waves per CU exist, so depth is what hides the HBM latency.
// MODE 0: x[n] = (x[n] + (dense + bd)) + (fc2 + b2) in one launch.  The co-scheduled decode layer (decode_layers_b1) splits it so that fc2 --
// which does not depend on the attention -- streams its 33.5 MB of weights WHILE the attention kernel runs:
//   MODE 1 (K0 = 0): y2[n] = fc2 + b2            (side stream, next to the attention kernel)
//   MODE 2 (K1 = 0): x[n] = (x[n] + (dense + bd)) + y2[n]   (after the join)
// Same lane split, accumulation order and parenthesisation in every mode: the three forms agree bit for bit.
template <int C, int MODE, bool F16 = false, bool Q8 = false>
__global__ __launch_bounds__(512) void out_gemv2_kernel(OutGemvArgs g) {
    extern __shared__ bf16_t sa[];  // [K0] attention row, [K1] gelu(fc1) row: read once per block instead of once per wave
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: weight-row bases in SGPRs
    const int stride = gridDim.x * 8;
    const int c0 = (g.K0 + 2047) / 2048;
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
    for (int i = threadIdx.x * 8; i < g.K0 + g.K1; i += 512 * 8)
        *reinterpret_cast<uint4*>(sa + i) = i < g.K0 ? *reinterpret_cast<const uint4*>(g.a0 + i) : *reinterpret_cast<const uint4*>(g.a1 + (i - g.K0));
    __syncthreads();
    const bf16_t* a0 = sa;
    const bf16_t* a1 = sa + g.K0;
    while (n < g.N) {
        const int nn = n + stride;
        float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
        for (int t = 0; t < C; ++t) {
            if (t < c0) acc0 = fma4<F16>(buf[t], a0, t * 2048 + lane * 8, g.K0, acc0);
            else acc1 = fma4<F16>(buf[t], a1, (t - c0) * 2048 + lane * 8, g.K1, acc1);
            if (nn < g.N) issue(nn, t, buf[t]);
        }
        acc0 = wave_sum_swap(acc0);
        acc1 = wave_sum_swap(acc1);
        if (lane == 0) {
            if (MODE != 1) acc0 = q8_scale<Q8>(acc0, g.s0, n);
            if (MODE != 2) acc1 = q8_scale<Q8>(acc1, g.s1, n);
            if (MODE == 1) {
                g.y2[n] = acc1 + g.b1[n];
            } else {
                float v = acc0 + g.b0[n];   // x1 = x + (dense + bd)         (RESID epilogue order of gemv_kernel)
                v += g.x[n];
                float v2 = MODE == 2 ? g.y2[n] : acc1 + g.b1[n];  // x2 = x1 + (fc2 + b2)
                v2 += v;
                g.x[n] = v2;
            }
        }
        n = nn;
    }
}

int pick_blocks(int cols, int waves_per_block, int max_blocks) {  // strided column assignment: any grid covers the matrix
    const int b = (cols + waves_per_block - 1) / waves_per_block;
    return b < max_blocks ? b : max_blocks;
}

}  // namespace

namespace showo {

bool decode_fused_shapes_ok(int H, int F) { return (H % 8) == 0 && (F % 8) == 0 && H <= 2048 && F <= 8192; }

DecodeLayerOps decode_layer_ops(const showo_engine* e, int li) {
    const Layer& l = e->layers[li];
    auto q = [](const int8_t* w) { return reinterpret_cast<const bf16_t*>(w); };
    if (e->precision == 3) return DecodeLayerOps{q(l.qqkv), q(l.q1), q(l.qd), q(l.q2), l.sqkv, l.s1, l.sd, l.s2, l.bqkv, l.b1, l.bd, l.b2};
    return DecodeLayerOps{l.wqkv, l.w1, l.wd, l.w2, nullptr, nullptr, nullptr, nullptr, l.bqkv, l.b1, l.bd, l.b2};
}
DecodeHeadOps decode_head_ops(const showo_engine* e, int col0) {
    if (e->precision == 3) return DecodeHeadOps{reinterpret_cast<const bf16_t*>(e->qlm + (int64_t)col0 * e->H), e->slm + col0, e->blm + col0};
    return DecodeHeadOps{e->wlm + (int64_t)col0 * e->H, nullptr, e->blm + col0};
}

// x -> LN(lnw, lnb) -> { out0 = bf16(W0 h + b0) | outf = fp32(W0 h + b0) } and out1 = bf16(gelu(W1 h + b1))  (N1 may be 0)
int decode_ln_gemv2(const LnGemvBArgs& a, hipStream_t s, int op) {
    LnGemvArgs g{a.x, a.lnw, a.lnb, a.eps, a.H, a.W0, a.b0, a.out0, a.outf, a.N0, a.W1, a.b1, a.out1, a.N1, a.s0, a.s1};
    if (g.s0 && (op || (g.N1 && !g.s1) || (g.H % 16)))
        return set_error_msg(1, "decode_ln_gemv2: int8 weights take bf16 activations, a scale per matrix and H % 16 == 0");
    // two weight rows in flight per wave (12 rows per block; a wave's third row is requested behind its first FMA).  Four rows -- the whole
    // layer matrix requested at kernel start -- measured SLOWER on cfg4 (0.983-0.992 vs 0.958-0.969 ms per token, round 2: 123 VGPRs halve
    // the resident waves and the single burst queues behind itself); that instance left the library in round 6.
    const dim3 grid(pick_blocks(g.N0 + g.N1, 12, showo::decode_tuning().ln_blocks));
    const size_t smem = (size_t)g.H * sizeof(bf16_t);
    // (int8 instance: four rows in flight per wave -- the bytes in flight of the bf16 instance's two -- measured no faster on cfg4 in a
    // one-process A/B; that instance is not built)
    if (g.s0) ln_gemv2_kernel<2, false, true><<<grid, dim3(256), smem, s>>>(g);
    else if (op) ln_gemv2_kernel<2, true><<<grid, dim3(256), smem, s>>>(g);
    else ln_gemv2_kernel<2><<<grid, dim3(256), smem, s>>>(g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error_hip(e, "ln_gemv2 launch", __FILE__, __LINE__);
    return 0;
}

// the (mode, C) instances of one operand type: the forked layer's two halves at Phi-1.5's shape, the one-launch form for C = 2..5
template <bool F16, bool Q8>
static int launch_out_gemv2(const OutGemvArgs& g, int mode, int C, dim3 grid, size_t smem, hipStream_t s) {
    if (mode == 1 && C == 4) out_gemv2_kernel<4, 1, F16, Q8><<<grid, dim3(512), smem, s>>>(g);
    else if (mode == 1 && C >= 1 && C <= 3) out_gemv2_kernel<3, 1, F16, Q8><<<grid, dim3(512), smem, s>>>(g);
    else if (mode == 2 && C == 1) out_gemv2_kernel<1, 2, F16, Q8><<<grid, dim3(512), smem, s>>>(g);
    else if (mode != 0) return set_error_msg(1, "decode_out_gemv2: unsupported K0/K1 for the forked layer");
    else switch (C) {
        case 2: out_gemv2_kernel<2, 0, F16, Q8><<<grid, dim3(512), smem, s>>>(g); break;
        case 3: out_gemv2_kernel<3, 0, F16, Q8><<<grid, dim3(512), smem, s>>>(g); break;
        case 4: out_gemv2_kernel<4, 0, F16, Q8><<<grid, dim3(512), smem, s>>>(g); break;
        case 5: out_gemv2_kernel<5, 0, F16, Q8><<<grid, dim3(512), smem, s>>>(g); break;
        default: return set_error_msg(1, "decode_out_gemv2: unsupported K0/K1 (decode_fused_shapes_ok)");
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error_hip(e, "out_gemv2 launch", __FILE__, __LINE__);
    return 0;
}

// x[n] += (W0[n,:] a0 + b0[n]);  x[n] += (W1[n,:] a1 + b1[n])
int decode_out_gemv2(const OutGemvArgs& args, hipStream_t s, int mode, int op) {
    OutGemvArgs g = args;
    const bool q8 = g.s0 || g.s1;  // int8 weight images (precision 3)
    if (q8 && (op || (mode != 1 && !g.s0) || (mode != 2 && !g.s1) || (g.K0 % 16) || (g.K1 % 16)))
        return set_error_msg(1, "decode_out_gemv2: int8 weights take bf16 activations, a scale per matrix and K % 16 == 0");
    if (mode == 1) g.K0 = 0;
    if (mode == 2) g.K1 = 0;
    if (mode && !g.y2) return set_error_msg(1, "decode_out_gemv2: y2 required");
    const int C = (g.K0 + 2047) / 2048 + (g.K1 + 2047) / 2048;
    const dim3 grid(pick_blocks(g.N, 8, showo::decode_tuning().out_blocks));
    const size_t smem = (size_t)(g.K0 + g.K1) * sizeof(bf16_t);
    if (q8) return launch_out_gemv2<false, true>(g, mode, C, grid, smem, s);
    if (op) return launch_out_gemv2<true, false>(g, mode, C, grid, smem, s);  // IEEE-half operands (precision 2)
    return launch_out_gemv2<false, false>(g, mode, C, grid, smem, s);
}

// AR decode step: three launches per layer.  Co-scheduled layer (co, the default at Phi-1.5's shape): the attention launch carries extra
// blocks that stream the fc2 weights into y2 (attention.hip, attn_decode_co_kernel) -- fc2 does not depend on the attention (Phi's block
// is parallel-residual) -- and the third launch adds dense(attn) and y2:
//   LN + qkv GEMV + fc1 GEMV  ->  [ attention (32 blocks) || fc2 GEMV -> y2 (co_blocks) ]  ->  dense GEMV + both residual adds
// Same arithmetic and parenthesisation as the plain chain (x = (x + (dense + bd)) + (fc2 + b2)): bit-identical results.
// Measured (one box, cfg4): chain 857-861 tokens/s; co-scheduled 922-928 with 224 fc2 blocks, 965 with 128, 969 with 96.  (A stream
// fork / join of the same overlap was SLOWER than the chain, 705-711 vs 843-846 tokens/s -- every fork / join edge of the per-token
// graph costs more than the overlap buys -- and left the library in round 6; so did folding the third launch into the second behind an
// in-launch hand-off, profiles/r6_decode_merge_ab.txt.)  !co (SHOWO_DECODE_FORK=0 / showo_decode_set_impl(2), other shapes): the chain.
int decode_layers_b1(showo_engine* e, int op, const KVDest& kv, const int32_t* iv, int pos0, bool co, hipStream_t s) {
    const int H = e->H, F = e->F;
    const int co_blocks = showo::decode_tuning().co_blocks;
    if (co && !e->y2) TRY(e->alloc(&e->y2, H));
    for (int li = 0; li < e->nL; ++li) {
        const Layer& l = e->layers[li];
        const DecodeLayerOps w = decode_layer_ops(e, li);
        LnGemvBArgs a{e->x, l.ln_w, l.ln_b, e->cfg.ln_eps, H, w.Wqkv, w.bqkv, e->qkv, nullptr, 3 * H, 3 * H, w.W1, w.b1, e->ffn, F, F};
        a.s0 = w.sqkv; a.s1 = w.s1;
        const OutGemvArgs o{e->x, w.Wd, e->attn, w.bd, H, w.W2, e->ffn, w.b2, F, H, co ? e->y2 : nullptr, w.sd, w.s2};
        TRY(decode_ln_gemv2(a, s, op));
        // the prefetch role reads ahead in the bf16 / fp16 images: none where the launches stream the int8 images instead
        DecodePrefetch pf{};
        if (co && !w.sqkv) decode_prefetch_plan(e, li, &pf);
        TRY(attn_decode_fused(e->qkv, l.qln_w, l.qln_b, l.kln_w, l.kln_b, e->cosT, e->sinT, kv.k + li * kv.k_lstride, kv.vt + li * kv.v_lstride,
                              iv, e->attn, e->nH, e->cfg.rotary_dim, e->cfg.ln_eps, pos0, kv.Lcap, kv.Lp, s, co ? &o : nullptr, co ? co_blocks : 0,
                              co && !w.sqkv ? &pf : nullptr, op));
        TRY(decode_out_gemv2(o, s, co ? 2 : 0, op));
    }
    return 0;
}

}  // namespace showo
