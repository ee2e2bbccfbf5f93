// Wide decode batches: 1..32 sequences per weight stream on v_mfma_f32_16x16x32_bf16 (precision 0, bf16 operands).
//
// The batched GEMVs of decode_batch.hip keep one v_dot2c chain per sequence, so their VALU work grows with the slot count and the step
// stops being a weight stream from four slots up.  A decode step with M <= 32 rows is what one MFMA covers: the WEIGHT tile is the A
// operand (16 output columns), the sequences are the B operand (16 per instruction), so 16 sequences cost the MFMA issue of one and 32
// cost two.  Operand mapping (lane l, g = l >> 4):
//   A: weight row n0 + (l & 15), k = 8 g + j          -> one 16-byte non-temporal load straight from HBM to VGPRs (no LDS round trip:
//                                                         no other wave shares a weight fragment)
//   B: sequence (l & 15) (+ 16 for the second M tile), the same k -> 16 bytes of that sequence's bf16 activation row (L2-resident)
//   D: column = sequence l & 15, rows 4 g + r = 4 consecutive output columns of ONE sequence -> one 8-byte bf16 / 16-byte fp32 store
// A wave owns TWO column tiles (32 output columns), so every activation fragment it fetches from L2 meets two weight fragments and
// every weight fragment meets both M tiles before it is dropped.  Rows >= nb are fed zeros and never stored.
//
//   ln_rows_wide_kernel   x fp32 [nb, H] -> LayerNorm -> bf16 row image hn [nb, H] (the bits of showo_layernorm_f32_op16): ONE launch
//                         per use instead of every GEMM block re-normalising 32 rows
//   ln_gemmW_kernel       hn -> out0 = bf16(W0 h + b0) | outf = fp32(...), out1 = bf16(gelu_new_fast(W1 h + b1))
//   out_gemmW_kernel      x[b] += (Wd attn[b] + bd) + (W2 ffn[b] + b2) as ONE K-concatenated accumulator (K0 + K1), K split over the 8
//                         waves of a block (summed in LDS in wave order) and over `ksplit` blocks (fp32 partials in a workspace, a
//                         ticket per column group, the last arriver sums in split order and re-arms the ticket: no atomics on
//                         floats, no waiting on other blocks, the order of additions is fixed)
//
// Contract: an output column of the MFMA reads only its own sequence's column and the K order is fixed, so a sequence's results do not
// depend on nb, on its row index or on the other rows.  They are NOT the bits of the dot2 chains of decode_batch.hip (the MFMA's
// internal summation order is the hardware's): same rounding points, another fp32 summation order.
#include "engine.h"
#include "decode_common.h"
#include "decode_wide.h"

using namespace showo;

namespace {

constexpr int WT = 2;        // column tiles of 16 per wave
constexpr int OUT_NW = 8;    // waves per block of the out kernel
constexpr int KS_MAX = 8;    // blocks that may share one column group's K range
constexpr int ITEMS = 256;   // float4 fragments of one column group: WT x 2 M tiles x 64 lanes

// LayerNorm of row b = blockIdx.x by ONE wave: the lane split and the expressions of ln_gemvB_kernel / ln_gemv2_kernel, statement for
// statement (the same bits per row as showo_layernorm_f32_op16).  H <= 2048, H % 4 == 0.
__global__ __launch_bounds__(64) void ln_rows_wide_kernel(const float* __restrict__ x, const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                          float eps, int H, bf16_t* __restrict__ hn) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const float* xr = x + (int64_t)b * H;
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
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)H + eps);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i = lane * 4 + j * 256;
        if (i < H) {
            const float4 v = xv[j];
            const float4 w = *reinterpret_cast<const float4*>(lnw + i);
            const float4 bb = *reinterpret_cast<const float4*>(lnb + i);
            const float y0 = (v.x - mean) * rstd * w.x + bb.x, y1 = (v.y - mean) * rstd * w.y + bb.y;
            const float y2 = (v.z - mean) * rstd * w.z + bb.z, y3 = (v.w - mean) * rstd * w.w + bb.w;
            uint2 o;
            o.x = Op16<false>::pack2(y0, y1);
            o.y = Op16<false>::pack2(y2, y3);
            *reinterpret_cast<uint2*>(hn + (int64_t)b * H + i) = o;
        }
    }
}

// One operand pair of the K-concatenated product: k-step j (32 elements) lies in segment 0 for j < c0, else in segment 1.
// w0 / w1: this lane's weight-row pointers (row and 8 g already applied); a0 / a1: its activation-row pointers per M tile.
template <int MT>
struct WideOperands {
    const bf16_t* w0[WT];
    const bf16_t* w1[WT];
    const bf16_t* a0[MT];
    const bf16_t* a1[MT];
    bool live[MT];  // the lane's sequence of M tile m exists (< nb); else its B fragment is zero
    int c0;
};

// acc[t][m] += W tile t x sequences of M tile m over the k-steps [j0, j1), U steps in flight (all loads issued before the first MFMA)
template <int MT, int U>
__device__ __forceinline__ void wide_steps(const WideOperands<MT>& o, int j0, int j1, f32x4 (&acc)[WT][MT]) {
    int j = j0;
    for (; j + U <= j1; j += U) {
        uint4 w[U][WT], a[U][MT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int jj = j + u;
            const bool first = jj < o.c0;
            const int k = (first ? jj : jj - o.c0) * 32;
#pragma unroll
            for (int t = 0; t < WT; ++t) w[u][t] = ldg_nt16((first ? o.w0[t] : o.w1[t]) + k);
#pragma unroll
            for (int m = 0; m < MT; ++m)
                a[u][m] = o.live[m] ? *reinterpret_cast<const uint4*>((first ? o.a0[m] : o.a1[m]) + k) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < WT; ++t)
#pragma unroll
                for (int m = 0; m < MT; ++m)
                    acc[t][m] = Op16<false>::mfma16(__builtin_bit_cast(bf16x8, w[u][t]), __builtin_bit_cast(bf16x8, a[u][m]), acc[t][m]);
    }
    if constexpr (U > 1) wide_steps<MT, 1>(o, j, j1, acc);
}

template <int MT>
__global__ __launch_bounds__(256) void ln_gemmW_kernel(LnGemvBArgs g, const bf16_t* __restrict__ hn, int nb, int vec) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int H = g.H, Ntot = g.N0 + g.N1, ngroups = (Ntot + 16 * WT - 1) / (16 * WT);
    const int lr = lane & 15, lg = lane >> 4;
    WideOperands<MT> o;
    o.c0 = H / 32;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int seq = 16 * m + lr;
        o.live[m] = seq < nb;
        o.a0[m] = o.a1[m] = hn + (int64_t)(o.live[m] ? seq : 0) * H + 8 * lg;
    }
    for (int grp = blockIdx.x * 4 + wave; grp < ngroups; grp += gridDim.x * 4) {
        const int n0 = grp * 16 * WT;
#pragma unroll
        for (int t = 0; t < WT; ++t) {  // rows beyond the last column are clamped (loaded, never stored)
            int r = n0 + 16 * t + lr;
            r = r < Ntot ? r : Ntot - 1;
            o.w0[t] = o.w1[t] = (r < g.N0 ? g.W0 + (int64_t)r * H : g.W1 + (int64_t)(r - g.N0) * H) + 8 * lg;
        }
        f32x4 acc[WT][MT];
#pragma unroll
        for (int t = 0; t < WT; ++t)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[t][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
        wide_steps<MT, 8>(o, 0, o.c0, acc);
#pragma unroll
        for (int t = 0; t < WT; ++t) {
            const int ct = n0 + 16 * t;  // wave-uniform: a tile lies in W0 or in W1 (N0 % 16 == 0 when N1 > 0)
            if (ct >= Ntot) continue;
            const int c = ct + 4 * lg;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int seq = 16 * m + lr;
                if (seq >= nb) continue;
                float v[4];
                if (ct < g.N0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = acc[t][m][r] + (c + r < g.N0 ? g.b0[c + r] : 0.f);
                    if (g.outf) {
                        float* dst = g.outf + (int64_t)seq * g.ld0 + c;
                        if (vec && c + 3 < g.N0) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                        else {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (c + r < g.N0) dst[r] = v[r];
                        }
                    } else {
                        bf16_t* dst = g.out0 + (int64_t)seq * g.ld0 + c;
                        if (vec && c + 3 < g.N0) *reinterpret_cast<uint2*>(dst) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
                        else {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (c + r < g.N0) dst[r] = f2bf(v[r]);
                        }
                    }
                } else {
                    const int c1 = c - g.N0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = gelu_new_fast(acc[t][m][r] + (c1 + r < g.N1 ? g.b1[c1 + r] : 0.f));
                    bf16_t* dst = g.out1 + (int64_t)seq * g.ld1 + c1;
                    if (vec && c1 + 3 < g.N1) *reinterpret_cast<uint2*>(dst) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
                    else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (c1 + r < g.N1) dst[r] = f2bf(v[r]);
                    }
                }
            }
        }
    }
}

// grid (column groups of 32, ksplit).  Block (grp, ks) covers the k-steps of split ks; its 8 waves split them again.
template <int MT>
__global__ __launch_bounds__(512) void out_gemmW_kernel(OutGemvBArgs g, int nb, float4* __restrict__ part, unsigned* __restrict__ tick) {
    __shared__ float4 sh[OUT_NW][WT * MT][64];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = blockIdx.x, ngroups = gridDim.x, ks = blockIdx.y, KS = gridDim.y;
    const int lr = lane & 15, lg = lane >> 4, n0 = grp * 16 * WT;
    WideOperands<MT> o;
    o.c0 = g.K0 / 32;
    const int steps = o.c0 + g.K1 / 32, S = KS * OUT_NW, sp = ks * OUT_NW + wave;
    const int j0 = (int)((int64_t)steps * sp / S), j1 = (int)((int64_t)steps * (sp + 1) / S);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int seq = 16 * m + lr;
        o.live[m] = seq < nb;
        o.a0[m] = g.a0 + (int64_t)(o.live[m] ? seq : 0) * g.lda0 + 8 * lg;
        o.a1[m] = g.a1 + (int64_t)(o.live[m] ? seq : 0) * g.lda1 + 8 * lg;
    }
#pragma unroll
    for (int t = 0; t < WT; ++t) {
        int r = n0 + 16 * t + lr;
        r = r < g.N ? r : g.N - 1;
        o.w0[t] = g.W0 + (int64_t)r * g.K0 + 8 * lg;
        o.w1[t] = g.W1 + (int64_t)r * g.K1 + 8 * lg;
    }
    f32x4 acc[WT][MT];
#pragma unroll
    for (int t = 0; t < WT; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[t][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    wide_steps<MT, 5>(o, j0, j1, acc);
#pragma unroll
    for (int t = 0; t < WT; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m) sh[wave][t * MT + m][lane] = make_float4(acc[t][m][0], acc[t][m][1], acc[t][m][2], acc[t][m][3]);
    __syncthreads();
    const bool owner = tid < WT * MT * 64;  // thread (item i = tid >> 6, lane) finishes one fragment
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (owner) {
        for (int w = 0; w < OUT_NW; ++w) {  // wave order
            const float4 p = sh[w][tid >> 6][lane];
            v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        }
    }
    if (KS > 1) {  // (grid-uniform)
        float4* base = part + (size_t)grp * ITEMS + tid;
        const size_t sstride = (size_t)ngroups * ITEMS;
        if (owner) base[ks * sstride] = v;
        // release by one lane after the block barrier, then the ticket; the last arriver re-arms it for the next launch on the stream
        __syncthreads();
        if (tid == 0) {
            __threadfence();
            const unsigned old = atomicAdd(tick + grp, 1u);
            const int last = old == (unsigned)(KS - 1);
            if (last) atomicExch(tick + grp, 0u);
            s_last = last;
            if (last) __threadfence();  // acquire
        }
        __syncthreads();
        if (!s_last) return;
        if (owner) {
            v = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k = 0; k < KS; ++k) {  // split order
                const float4 p = base[k * sstride];
                v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
            }
        }
    }
    if (!owner) return;
    const int i = tid >> 6, t = i / MT, m = i % MT;
    const int seq = 16 * m + lr, c = n0 + 16 * t + 4 * lg;
    if (seq >= nb || c >= g.N) return;
    float* xr = g.x + (int64_t)seq * g.N + c;
    const float vv[4] = {v.x, v.y, v.z, v.w};
    if (c + 3 < g.N && (g.N & 3) == 0) {
        const float4 xo = *reinterpret_cast<const float4*>(xr), bd = *reinterpret_cast<const float4*>(g.b0 + c),
                     b2 = *reinterpret_cast<const float4*>(g.b1 + c);
        *reinterpret_cast<float4*>(xr) = make_float4(xo.x + (vv[0] + (bd.x + b2.x)), xo.y + (vv[1] + (bd.y + b2.y)),
                                                     xo.z + (vv[2] + (bd.z + b2.z)), xo.w + (vv[3] + (bd.w + b2.w)));
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (c + r < g.N) xr[r] += vv[r] + (g.b0[c + r] + g.b1[c + r]);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

namespace showo {

void wide_ws_free(WideWs* w) {
    if (w->hn) hipFree(w->hn);
    if (w->part) hipFree(w->part);
    if (w->tick) hipFree(w->tick);
    *w = WideWs{};
}

int wide_ws_reserve(WideWs* w, int H, int N) {
    const int64_t hn = (int64_t)32 * H;
    const int groups = (N + 16 * WT - 1) / (16 * WT);
    if (hn <= w->hn_elems && groups <= w->groups) return 0;
    SHOWO_CHECK_HIP(hipDeviceSynchronize());  // nothing in flight still reads what is freed
    const int64_t hn_new = hn > w->hn_elems ? hn : w->hn_elems;
    const int groups_new = groups > w->groups ? groups : w->groups;
    wide_ws_free(w);
    SHOWO_CHECK_HIP(hipMalloc((void**)&w->hn, (size_t)hn_new * sizeof(bf16_t)));
    SHOWO_CHECK_HIP(hipMalloc((void**)&w->part, (size_t)KS_MAX * groups_new * ITEMS * sizeof(float4)));
    SHOWO_CHECK_HIP(hipMalloc((void**)&w->tick, (size_t)groups_new * sizeof(unsigned)));
    SHOWO_CHECK_HIP(hipMemset(w->tick, 0, (size_t)groups_new * sizeof(unsigned)));  // armed once; every launch leaves the words at zero
    w->hn_elems = hn_new;
    w->groups = groups_new;
    return 0;
}

int ln_gemmW(int nb, const LnGemvBArgs& g, const WideWs& w, hipStream_t s) {
    const int Ntot = g.N0 + g.N1;
    if (nb < 1 || nb > 32) return set_error_msg(1, "ln_gemmW: 1..32 rows");
    if (g.H < 32 || g.H > 2048 || (g.H % 32) || g.N0 < 1 || g.N1 < 0 || (g.N1 > 0 && (g.N0 % 16)))
        return set_error_msg(1, "ln_gemmW: hidden <= 2048 and a multiple of 32; N0 % 16 == 0 when N1 > 0");
    if (g.s0 || g.s1 || g.W0lo) return set_error_msg(1, "ln_gemmW: bf16 weights only (precision 0)");
    if (!w.hn || (int64_t)32 * g.H > w.hn_elems) return set_error_msg(5, "ln_gemmW: workspace too small");
    if (!aligned16(g.W0) || (g.N1 && !aligned16(g.W1)) || !aligned16(g.x) || !aligned16(g.lnw) || !aligned16(g.lnb))
        return set_error_msg(1, "ln_gemmW: operands must be 16-byte aligned");
    ln_rows_wide_kernel<<<dim3(nb), dim3(64), 0, s>>>(g.x, g.lnw, g.lnb, g.eps, g.H, w.hn);
    // vector stores: every output row starts on a 16-byte boundary (else element stores, e.g. fp32 logits rows of an odd vocabulary)
    int vec = g.outf ? (aligned16(g.outf) && g.ld0 % 4 == 0) : (aligned16(g.out0) && g.ld0 % 8 == 0);
    if (g.N1) vec = vec && aligned16(g.out1) && g.ld1 % 8 == 0;
    const int ngroups = (Ntot + 16 * WT - 1) / (16 * WT);
    int blocks = (ngroups + 3) / 4;
    const int cap = showo::decode_tuning().wide_ln_blocks;
    if (blocks > cap) blocks = cap;
    if (nb <= 16) ln_gemmW_kernel<1><<<dim3(blocks), dim3(256), 0, s>>>(g, w.hn, nb, vec);
    else ln_gemmW_kernel<2><<<dim3(blocks), dim3(256), 0, s>>>(g, w.hn, nb, vec);
    return hipGetLastError() == hipSuccess ? 0 : set_error_msg(7, "ln_gemmW launch failed");
}

int out_gemmW(int nb, const OutGemvBArgs& g, const WideWs& w, hipStream_t s) {
    if (nb < 1 || nb > 32) return set_error_msg(1, "out_gemmW: 1..32 rows");
    if (g.N < 1 || g.K0 < 32 || g.K1 < 32 || (g.K0 % 32) || (g.K1 % 32) || (g.lda0 % 8) || (g.lda1 % 8))
        return set_error_msg(1, "out_gemmW: K0 and K1 multiples of 32, activation rows 16-byte aligned");
    if (g.s0 || g.s1) return set_error_msg(1, "out_gemmW: bf16 weights only (precision 0)");
    if (!aligned16(g.W0) || !aligned16(g.W1) || !aligned16(g.a0) || !aligned16(g.a1) || !aligned16(g.x) || !aligned16(g.b0) || !aligned16(g.b1))
        return set_error_msg(1, "out_gemmW: operands must be 16-byte aligned");
    const int ngroups = (g.N + 16 * WT - 1) / (16 * WT);
    if (!w.part || !w.tick || ngroups > w.groups) return set_error_msg(5, "out_gemmW: workspace too small");
    int ks = showo::decode_tuning().wide_out_ksplit;
    if (ks > KS_MAX) ks = KS_MAX;
    if (ks < 1) ks = 1;
    if (nb <= 16) out_gemmW_kernel<1><<<dim3(ngroups, ks), dim3(512), 0, s>>>(g, nb, w.part, w.tick);
    else out_gemmW_kernel<2><<<dim3(ngroups, ks), dim3(512), 0, s>>>(g, nb, w.part, w.tick);
    return hipGetLastError() == hipSuccess ? 0 : set_error_msg(7, "out_gemmW launch failed");
}

}  // namespace showo

// ---- test hooks: the two kernels alone (tests/test_decode_wide_kernels_gpu.py) ----------------------------------------------------
// One workspace per process, grown on demand: the hooks are for one stream at a time.
static showo::WideWs g_hook_ws;

extern "C" int showo_decode_wide_ln_gemm(const float* x, const float* lnw, const float* lnb, float eps, int H, const uint16_t* W0,
                                         const float* b0, uint16_t* out0, float* outf, int N0, int ld0, const uint16_t* W1, const float* b1,
                                         uint16_t* out1, int N1, int ld1, int nb, void* stream) {
    if (!x || !lnw || !lnb || !W0 || !b0 || (!out0 && !outf) || (N1 > 0 && (!W1 || !b1 || !out1)) || H < 1 || N0 < 1 || N1 < 0 || ld0 < N0 ||
        (N1 > 0 && ld1 < N1))
        return set_error_msg(1, "showo_decode_wide_ln_gemm: bad arguments");
    if (int rc = showo::wide_ws_reserve(&g_hook_ws, H, 32)) return rc;
    LnGemvBArgs g{x, lnw, lnb, eps, H, W0, b0, outf ? nullptr : out0, outf, N0, ld0, W1, b1, out1, N1, ld1};
    return showo::ln_gemmW(nb, g, g_hook_ws, (hipStream_t)stream);
}

extern "C" int showo_decode_wide_out_gemm(float* x, const uint16_t* Wd, const uint16_t* attn, const float* bd, int K0, const uint16_t* W2,
                                          const uint16_t* ffn, const float* b2, int K1, int N, int nb, void* stream) {
    if (!x || !Wd || !attn || !bd || !W2 || !ffn || !b2 || N < 1) return set_error_msg(1, "showo_decode_wide_out_gemm: bad arguments");
    if (int rc = showo::wide_ws_reserve(&g_hook_ws, 32, N)) return rc;
    OutGemvBArgs g{x, Wd, attn, bd, K0, K0, W2, ffn, b2, K1, K1, N, nullptr};
    return showo::out_gemmW(nb, g, g_hook_ws, (hipStream_t)stream);
}
