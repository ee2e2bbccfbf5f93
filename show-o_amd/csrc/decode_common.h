// Pieces of the AR-decode GEMV kernels shared by decode.hip and the co-scheduled attention launch (attention.hip).
#pragma once
#include "common.h"

namespace showo {

// mask row of the token at position P (the batched decode seams, showo_mask_append_rows): the last prompt row extended by the columns [L0, P] (modeling_showo.py:203-217)
// q / k LayerNorm(64) + partial RoPE of one head row of a NEW token, lane = dimension: the statistics on the VALU-only reductions
// (the bits of wave_sum), the RoPE operands (cs, sn: the lane's entries of the position's table row) in registers.  The ONE copy of
// these expressions: the fused single-query attention (attention.hip attn_decode_body) and both launches of the shared-prefix
// attention (attn_shared.hip) call it, so a query row has the same bits wherever it is prepared.
static __device__ __forceinline__ float decode_prep_lane(float x0, float lnw, float lnb, float eps, float cs, float sn, int rot, int lane) {
    const float mean = wave_sum_swap(x0) * (1.0f / 64.0f);
    const float c = x0 - mean;
    const float var = wave_sum_swap(c * c) * (1.0f / 64.0f);
    float y = c * (1.0f / sqrtf(var + eps)) * lnw + lnb;
    const int half = rot >> 1;
    const float partner = __shfl_xor(y, half, 64);
    if (lane < rot) y = y * cs + (lane < half ? -partner : partner) * sn;
    return y;
}

static __device__ __forceinline__ void next_iv(const int32_t* last_iv, int L0, int P, int32_t* iv) {
    int a = last_iv[0], b = last_iv[1], c = last_iv[2], d = last_iv[3];
    if (b == L0 && a < b) b = P + 1;
    else if (d == L0 && c < d) d = P + 1;
    else if (!(c < d)) { c = L0; d = P + 1; }
    else if (!(a < b)) { a = L0; b = P + 1; }
    iv[0] = a; iv[1] = b; iv[2] = c; iv[3] = d;
}

// Row of slot b for its next step (the batched sampled seam and the beam seam): the embedding of its token while it decodes; zeros
// once it is idle (a fixed, finite row, so the idle slot's residual row stays bounded while the other slots keep decoding).
static __device__ __forceinline__ void slot_embed_row(int64_t id, bool active, const float* __restrict__ table, float* __restrict__ xr, int H,
                                                      int V, int tid, int nthr) {
    if (!active) {
        for (int i = tid; i < H; i += nthr) xr[i] = 0.f;
    } else if (id < 0 || id >= V) {
        for (int i = tid; i < H; i += nthr) xr[i] = __builtin_nanf("");
    } else {
        const float* src = table + id * H;
        for (int i = tid; i < H; i += nthr) xr[i] = src[i];
    }
}

static __device__ __forceinline__ void load4(const bf16_t* row, int k0, int K, uint4 (&wv)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int k = k0 + u * 512;
        wv[u] = k < K ? ldg_nt16(row + k) : make_uint4(0, 0, 0, 0);
    }
}
// ---- int8 weight stream (precision 3) -----------------------------------------------------------------------------------------------
// The int8 image is row-major: a lane keeps its k assignment (k in [8 l, 8 l + 8) + 512 u) and loads 8 bytes per sub-span instead of
// 16.  WVec<Q8>::type is what one such load returns; wrow<Q8> is the typed base of weight row `col` of a [*, K] matrix whose pointer
// travels as bf16_t* in the argument structs.
template <bool Q8> struct WVec { typedef uint4 type; };
template <> struct WVec<true> { typedef uint2 type; };
template <bool Q8>
static __device__ __forceinline__ auto wrow(const bf16_t* W, int64_t col, int K) {
    if constexpr (Q8) return reinterpret_cast<const int8_t*>(W) + col * K;
    else return W + col * K;
}
static __device__ __forceinline__ void load4(const int8_t* row, int k0, int K, uint2 (&wv)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int k = k0 + u * 512;
        wv[u] = k < K ? ldg_nt8(row + k) : make_uint2(0, 0);
    }
}
// 8 int8 weights -> 4 packed bf16 pairs, EXACTLY (|q| <= 127 fits bf16's 8-bit significand: the fp32 image truncates without loss)
static __device__ __forceinline__ uint32_t q8_pair(uint32_t w, int i) {
    const float lo = (float)(int)(int8_t)(w >> (8 * i)), hi = (float)(int)(int8_t)(w >> (8 * i + 8));
    return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);
}
static __device__ __forceinline__ uint4 q8_to_bf16x8(const uint2& w) {
    return make_uint4(q8_pair(w.x, 0), q8_pair(w.x, 2), q8_pair(w.y, 0), q8_pair(w.y, 2));
}
// the weight scale of output column n in front of the epilogue: ONE fp32 multiply, a statement of its own (never contracted into the
// bias add), so every kernel form gives the same bits; for a power-of-two scale the result is what the bf16 kernel computes on q * s
template <bool Q8>
static __device__ __forceinline__ float q8_scale(float acc, const float* s, int n) {
    if constexpr (Q8) {
        const float v = acc * s[n];
        return v;
    } else {
        return acc;
    }
}

// acc += sum over the 4 loaded 8-element groups, in gemv_kernel's order (u ascending, pairs ascending: dot8_bf16)
// F16: the operand type of weights and activations (common.h Op16; precision 2 = IEEE half on v_dot2_f32_f16)
template <bool F16 = false, class AP>
static __device__ __forceinline__ float fma4(const uint4 (&wv)[4], AP act, int k0, int K, float acc) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int k = k0 + u * 512;
        if (k >= K) break;
        acc = dot8_op<F16>(wv[u], *reinterpret_cast<const uint4*>(act + k), acc);
    }
    return acc;
}
// the same chain on int8 weights (bf16 activations): the conversion is exact, the dot2 chain is the bf16 one
template <bool F16 = false, class AP>
static __device__ __forceinline__ float fma4(const uint2 (&wv)[4], AP act, int k0, int K, float acc) {
    static_assert(!F16, "int8 weights multiply bf16 activations");
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int k = k0 + u * 512;
        if (k >= K) break;
        acc = dot8_op<false>(q8_to_bf16x8(wv[u]), *reinterpret_cast<const uint4*>(act + k), acc);
    }
    return acc;
}

struct OutGemvArgs {
    float* x;           // [N] fp32 residual stream row, updated in place
    const bf16_t* W0;   // [N, K0] dense weight,  a0 [K0] attention output
    const bf16_t* a0;
    const float* b0;
    int K0;
    const bf16_t* W1;   // [N, K1] fc2 weight,    a1 [K1] gelu(fc1) row
    const bf16_t* a1;
    const float* b1;
    int K1;
    int N;
    float* y2;          // [N] fp32: fc2 + b2 of the forked layer (MODE 1 writes it, MODE 2 adds it)
    const float* s0 = nullptr;  // Q8 instances: W0 / W1 are int8 [N, K0] / [N, K1], s0 / s1 [N] their row scales
    const float* s1 = nullptr;
};


// fc2 role of the co-scheduled decode launch (attention.hip, attn_decode_co_kernel): y2[n] = W1[n, :] a1 + b1[n] for the columns of
// role-block `rb` of `nrb`, `nw` waves per block.  Same lane split, accumulation order and epilogue expression as
// out_gemv2_kernel<C, 1> (decode.hip), so the result does not depend on which launch computed it.  sa: >= K1 bf16 of LDS.
template <int C, bool F16 = false, bool Q8 = false>
static __device__ __forceinline__ void fc2_columns_role(const OutGemvArgs& g, int rb, int nrb, int nw, bf16_t* sa) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int stride = nrb * nw;
    int n = wave * nrb + rb;
    typename WVec<Q8>::type buf[C][4];
    if (n < g.N) {
#pragma unroll
        for (int t = 0; t < C; ++t) load4(wrow<Q8>(g.W1, n, g.K1), t * 2048 + lane * 8, g.K1, buf[t]);
    }
    for (int i = threadIdx.x * 8; i < g.K1; i += nw * 64 * 8) *reinterpret_cast<uint4*>(sa + i) = *reinterpret_cast<const uint4*>(g.a1 + i);
    __syncthreads();
    while (n < g.N) {
        const int nn = n + stride;
        float acc1 = 0.f;
#pragma unroll
        for (int t = 0; t < C; ++t) {
            acc1 = fma4<F16>(buf[t], sa, t * 2048 + lane * 8, g.K1, acc1);
            if (nn < g.N) load4(wrow<Q8>(g.W1, nn, g.K1), t * 2048 + lane * 8, g.K1, buf[t]);
        }
        acc1 = wave_sum_swap(acc1);
        if (lane == 0) {
            const float v1 = q8_scale<Q8>(acc1, g.s1, n);
            g.y2[n] = v1 + g.b1[n];
        }
        n = nn;
    }
}

// ---- Infinity-Cache prefetch role of the co-scheduled decode launches ---------------------------------------------------------------
// The attention launch of a decode layer is latency-bound (32 x NB single-query blocks) and its fc2 role needs 33.5 MB: HBM idles for
// part of it, and the CUs neither role occupies idle throughout.  Extra blocks of the SAME launch read weights the NEXT launches will
// stream (this layer's dense matrix, the next layer's [Wqkv ; W1]) so that those launches find them in the 256 MiB memory-side cache.
// The reads are LDS-DMA (global_load_lds, 16 B per lane, default cache policy, no VGPR round trip; the LDS image is scratch that every
// wave overwrites): nothing is computed from them, the product's results cannot depend on this role.
struct DecodePrefetch {
    const void* p[3];   // up to three segments, read in order
    int64_t bytes[3];   // multiples of 16
    int blocks;         // prefetch blocks appended to the grid (0: role absent)
};
// block rb of nrb: a contiguous slice of every segment; lds: >= nw KiB of LDS (1 KiB per wave)
static __device__ __forceinline__ void prefetch_role(const DecodePrefetch& pf, int rb, int nrb, void* lds) {
    const int wave = threadIdx.x >> 6, nthr = blockDim.x;
    bf16_t* dst = reinterpret_cast<bf16_t*>(lds) + wave * 512;
#pragma unroll 1
    for (int sgm = 0; sgm < 3; ++sgm) {
        const int64_t n16 = pf.bytes[sgm] >> 4;
        if (n16 <= 0) continue;
        const int64_t per = (((n16 + nrb - 1) / nrb) + nthr - 1) / nthr * nthr;
        const int64_t i0 = (int64_t)rb * per, i1 = i0 + per < n16 ? i0 + per : n16;
        const bf16_t* src = reinterpret_cast<const bf16_t*>(pf.p[sgm]);
        for (int64_t i = i0 + threadIdx.x; i < i1; i += nthr) glds16(src + i * 8, dst);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- batched decode (decode_batch.hip): NB sequences share one weight stream --------------------------------------------------
struct OutGemvBArgs {
    float* x;          // [NB, N] fp32 residual rows (ld = N), updated in place
    const bf16_t* W0;  // [N, K0] dense;  a0 [NB, K0] (lda0)
    const bf16_t* a0;
    const float* b0;
    int K0, lda0;
    const bf16_t* W1;  // [N, K1] fc2;    a1 [NB, K1] (lda1)
    const bf16_t* a1;
    const float* b1;
    int K1, lda1;
    int N;
    float* y2;         // [NB, N] fp32: fc2 + b2 per sequence (written by the co-scheduled role, added by out_gemvB_kernel<.., 2>)
    const float* s0 = nullptr;  // Q8 instances: W0 / W1 are int8 [N, K0] / [N, K1], s0 / s1 [N] their row scales
    const float* s1 = nullptr;
};

// LayerNorm + two GEMV / GEMM outputs of the batched decode step (decode_batch.hip ln_gemvB_kernel, decode_wide.hip ln_gemmW_kernel)
struct LnGemvBArgs {
    const float* x;  // [NB, H] fp32 residual rows
    const float *lnw, *lnb;
    float eps;
    int H;
    const bf16_t* W0;  // [N0, H] -> out0[b][n] = bf16(W0 h_b + b0) (ld0) or outf[b][n] = fp32(...) (ld0)
    const float* b0;
    bf16_t* out0;
    float* outf;
    int N0, ld0;
    const bf16_t* W1;  // [N1, H] -> out1[b][n] = bf16(gelu_new(W1 h_b + b1)) (ld1)
    const float* b1;
    bf16_t* out1;
    int N1, ld1;
    const bf16_t* W0lo = nullptr;  // HEAD3 instances (precision 2's lm_head): low halves of W0's rows, same layout
    const float* s0 = nullptr;     // Q8 instances (precision 3): W0 / W1 are int8 row-major, s0 [N0] / s1 [N1] their row scales
    const float* s1 = nullptr;
};

// wave_sum of up to four accumulators at once, each with wave_sum's own order of additions (partners 32, 16, 8, 4, 2, 1 away: the same
// bits).  The 32 / 16 steps run on every accumulator with gfx950's row-swap instructions (VALU only); after them a lane holds, for
// each b, the sum over its 4-lane group {l, l^16, l^32, l^48}, so lane group g = lane >> 4 continues with accumulator g alone: ONE
// register takes the remaining four steps (DPP: row_sum_dpp).  No LDS-crossbar permute at all (6 per sequence in wave_sum).  Returns, in the lanes
// 16 b .. 16 b + 15, the wave-wide sum of acc[b] (b < NB <= 4).
template <int NB>
static __device__ __forceinline__ float wave_sum_groups(const float (&acc)[NB]) {
    static_assert(NB >= 1 && NB <= 4, "one 16-lane group per accumulator");
    const int g = (threadIdx.x >> 4) & 3;
    float r = 0.f;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[b]), __float_as_uint(acc[b]), false, false);
        const float v = __uint_as_float(s32[0]) + __uint_as_float(s32[1]);
        const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        const float w = __uint_as_float(s16[0]) + __uint_as_float(s16[1]);
        r = g == b ? w : r;
    }
    return row_sum_dpp(r);
}

// acc[b] += sum over the 4 loaded 8-element groups of w * act[b], in fma4's order (u ascending, pairs ascending) per sequence.
// act: this lane's 32 activation values per sequence as 16 packed bf16 pairs (registers).
template <int NB, bool F16 = false>
static __device__ __forceinline__ void fma4_regs(const uint4 (&wv)[4], const uint32_t (&act)[NB][16], int k0, int K, float (&acc)[NB]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (k0 + u * 512 >= K) break;
        const uint32_t w[4] = {wv[u].x, wv[u].y, wv[u].z, wv[u].w};
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = Op16<F16>::dot2(w[p], act[b][u * 4 + p], acc[b]);
    }
}
// int8 weights: converted once per weight (not per sequence), then the bf16 chain
template <int NB, bool F16 = false>
static __device__ __forceinline__ void fma4_regs(const uint2 (&wv)[4], const uint32_t (&act)[NB][16], int k0, int K, float (&acc)[NB]) {
    static_assert(!F16, "int8 weights multiply bf16 activations");
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (k0 + u * 512 >= K) break;
        const uint4 wb = q8_to_bf16x8(wv[u]);
        const uint32_t w[4] = {wb.x, wb.y, wb.z, wb.w};
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = Op16<false>::dot2(w[p], act[b][u * 4 + p], acc[b]);
    }
}
// this lane's 16 pairs of one bf16 activation row (global or LDS), zero beyond K
template <class AP>
static __device__ __forceinline__ void load_act_pairs(AP row, int k0, int K, uint32_t (&act)[16]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int k = k0 + u * 512;
        uint4 av = make_uint4(0, 0, 0, 0);
        if (k < K) av = *reinterpret_cast<const uint4*>(row + k);
        act[u * 4 + 0] = av.x; act[u * 4 + 1] = av.y; act[u * 4 + 2] = av.z; act[u * 4 + 3] = av.w;
    }
}
// the same with the activations in LDS (sa: row b at sa + b * ld, bf16): one 16-byte read per 8 products per sequence
template <int NB, bool F16 = false>
static __device__ __forceinline__ void fma4_lds(const uint4 (&wv)[4], const bf16_t* sa, int ld, int k0, int K, float (&acc)[NB]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int k = k0 + u * 512;
        if (k >= K) break;
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = dot8_op<F16>(wv[u], *reinterpret_cast<const uint4*>(sa + (size_t)b * ld + k), acc[b]);
    }
}

template <int NB, bool F16 = false>
static __device__ __forceinline__ void fma4_lds(const uint2 (&wv)[4], const bf16_t* sa, int ld, int k0, int K, float (&acc)[NB]) {
    static_assert(!F16, "int8 weights multiply bf16 activations");
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int k = k0 + u * 512;
        if (k >= K) break;
        const uint4 wb = q8_to_bf16x8(wv[u]);
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = dot8_op<false>(wb, *reinterpret_cast<const uint4*>(sa + (size_t)b * ld + k), acc[b]);
    }
}

// fc2 role of the co-scheduled BATCHED decode launch (attention.hip, attn_decode_coB_kernel): y2[b][n] = W1[n, :] a1[b] + b1[n] for
// the columns of role-block rb of nrb, nw waves per block.  fc2_columns_role's lane split and accumulation order per sequence (chunks
// t ascending into ONE accumulator chain, then the wave reduction): the bits of the batch-1 launch.  The NB activation rows live in
// LDS as bf16 (NB * K1 * 2 bytes: 64 KiB at NB = 4).
template <int C, int NB, bool F16 = false, bool Q8 = false>
static __device__ __forceinline__ void fc2_columns_roleB(const OutGemvBArgs& g, int rb, int nrb, int nw, bf16_t* sa) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int stride = nrb * nw;
    int n = wave * nrb + rb;
    typename WVec<Q8>::type buf[C][4];
    if (n < g.N) {
#pragma unroll
        for (int t = 0; t < C; ++t) load4(wrow<Q8>(g.W1, n, g.K1), t * 2048 + lane * 8, g.K1, buf[t]);
    }
    for (int b = 0; b < NB; ++b)
        for (int i = threadIdx.x * 8; i < g.K1; i += nw * 64 * 8)
            *reinterpret_cast<uint4*>(sa + (size_t)b * g.K1 + i) = *reinterpret_cast<const uint4*>(g.a1 + (int64_t)b * g.lda1 + i);
    __syncthreads();
    while (n < g.N) {
        const int nn = n + stride;
        float acc1[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) acc1[b] = 0.f;
#pragma unroll
        for (int t = 0; t < C; ++t) {
            fma4_lds<NB, F16>(buf[t], sa, g.K1, t * 2048 + lane * 8, g.K1, acc1);
            if (nn < g.N) load4(wrow<Q8>(g.W1, nn, g.K1), t * 2048 + lane * 8, g.K1, buf[t]);
        }
        const float tot = wave_sum_groups<NB>(acc1);
        if ((lane & 15) == 0 && (lane >> 4) < NB) {
            const float v1 = q8_scale<Q8>(tot, g.s1, n);
            g.y2[(int64_t)(lane >> 4) * g.N + n] = v1 + g.b1[n];
        }
        n = nn;
    }
}
}  // namespace showo
