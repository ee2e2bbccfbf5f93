// Shared-prefix decode attention ("Shared-prefix slots"): the nb <= 32 slots of a wide decode batch continue ONE prefix
// [0, P) that lives in the engine's decode cache; a slot owns only its suffix (appended rows + generated tokens), stored at row /
// column k - base of a suffix cache, base = P & ~63 (so the 64-key tiles of source and destination line up).  Per layer, in place of the
// heads x nb single-query blocks that each stream their own copy of the prefix:
//
//   attn_shared_prefix_kernel   grid (heads, ceil(P / 64)), one wave.  The block prepares the nb query rows of its head (q LayerNorm,
//                               partial RoPE at each slot's position, x 0.125, bf16: decode_prep_lane of decode_common.h, the function
//                               attn_decode_body's FUSED prep calls), then S^T = K Q^T for its 64 keys against all queries on v_mfma_f32_32x32x16_bf16 (keys on
//                               rows, queries on columns: a lane owns one query), the per-query max / sum of its key range, and
//                               O^T = V^T P^T with P rounded to bf16 -- the accumulator tile of S^T is the B operand of the second
//                               product as it stands (attn_fwd_kernel's layout).  Writes fp32 (m, l, o[64]) per (split, head, slot).
//   attn_shared_suffix_kernel   grid (heads, nb), 4 waves.  The single-query attention over the slot's suffix: appends the new K row /
//                               V^T column at pos - base (taken from LDS inside the launch), scores the keys [P - base, pos - base],
//                               then merges its (m, l, o) with the prefix partials in split order by log-sum-exp rescaling and writes
//                               the bf16 row.  The kernel boundary is the hand-off: no atomics, no tickets.
//
// A slot's row depends only on its own query, the prefix and its own suffix: the key split (KSPLIT) is a constant of the build, the MFMA
// shape and every summation order are the same for every nb (query columns >= nb are zero operands whose results are dropped), and
// rows >= nb of the inputs, the output and the workspace are neither read nor written.  Keys >= P of the prefix cache and rows /
// columns outside [P - base, pos - base] of a suffix cache may hold anything: their scores are replaced before the max and their V
// elements are selected to zero, never multiplied.
#include "attn_shared.h"
#include "decode_common.h"
#include "../../include/showo_hip.h"
#include <cmath>

using namespace showo;

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int KSPLIT = 64;     // keys per prefix block
constexpr int WS_STRIDE = 68;  // floats per (split, head, slot): m, l, two pads, o[64] (16-byte aligned)
constexpr int QPITCH = 72;     // bf16 per query row in LDS (144 B: the 16-byte fragment reads of 32 rows spread over the banks)

__device__ __forceinline__ bf16x8 pack8(const float* p) {
    uint4 u;
    u.x = pack_bf2(p[0], p[1]);
    u.y = pack_bf2(p[2], p[3]);
    u.z = pack_bf2(p[4], p[5]);
    u.w = pack_bf2(p[6], p[7]);
    return __builtin_bit_cast(bf16x8, u);
}

// the first n of four 16-bit elements, zeros behind them (n <= 0: none, n >= 4: all)
__device__ __forceinline__ uint2 keep_first(uint2 v, int n) {
    v.x = n >= 2 ? v.x : (n == 1 ? (v.x & 0xffffu) : 0u);
    v.y = n >= 4 ? v.y : (n == 3 ? (v.y & 0xffffu) : 0u);
    return v;
}

__global__ __launch_bounds__(64) void attn_shared_prefix_kernel(SharedAttnArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t sq[32 * QPITCH];
    const int lane = threadIdx.x, head = blockIdx.x, split = blockIdx.y;
    const int qi = lane & 31, hh = lane >> 5;
    const int k0 = split * KSPLIT;  // k0 + 64 <= cap_pre: k0 < P <= cap_pre, both multiples of 64 or below one
    const int Hq = a.nH * 64;
    // the cache loads first: K rows k0 + 32 t + qi (16 bytes per k-step) and the V^T fragments of both 32-key tiles
    const bf16_t* Kb = a.Kp + ((int64_t)head * a.cap_pre + k0 + qi) * 64 + 8 * hh;
    const bf16_t* Vb = a.Vp + ((int64_t)head * 64 + qi) * a.cap_pre + k0 + 4 * hh;
    uint4 kf[2][4];
    uint2 vf[2][2][2][2];  // [tile][k-step][dim half][first / second group of four keys]
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int m = 0; m < 4; ++m) kf[t][m] = *reinterpret_cast<const uint4*>(Kb + (int64_t)t * 32 * 64 + 16 * m);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int dh = 0; dh < 2; ++dh) {
                const bf16_t* v = Vb + (int64_t)dh * 32 * a.cap_pre + 32 * t + 16 * kk;
                vf[t][kk][dh][0] = *reinterpret_cast<const uint2*>(v);
                vf[t][kk][dh][1] = *reinterpret_cast<const uint2*>(v + 8);
            }
    // the nb query rows of this head -> LDS as bf16; rows >= nb are zero operands (their index is clamped: no row >= nb is read)
    const float lnw = a.qw[lane], lnb = a.qb[lane];
    const int posv = a.pos_dev[lane < a.nb ? lane : a.nb - 1];
    const int dl = lane < a.rot ? lane : 0;
    bf16_t xin[32];
    float cs[32], sn[32];
#pragma unroll
    for (int b = 0; b < 32; ++b) {
        const int bb = b < a.nb ? b : a.nb - 1;
        const int pos = __shfl(posv, bb, 64);
        xin[b] = a.qkv[(int64_t)bb * 3 * Hq + head * 64 + lane];
        cs[b] = a.cosT[(int64_t)pos * a.rot + dl];
        sn[b] = a.sinT[(int64_t)pos * a.rot + dl];
    }
#pragma unroll
    for (int b = 0; b < 32; ++b) {
        const float y = decode_prep_lane(bf2f(xin[b]), lnw, lnb, a.eps, cs[b], sn[b], a.rot, lane);
        sq[b * QPITCH + lane] = b < a.nb ? f2bf(y * 0.125f) : (bf16_t)0;
    }
    __syncthreads();
    bf16x8 qf[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) qf[m] = *reinterpret_cast<const bf16x8*>(sq + qi * QPITCH + 16 * m + 8 * hh);
    // S^T = K Q^T: lane (qi, hh) holds the scores of query qi against keys k0 + 32 t + (r & 3) + 8 (r >> 2) + 4 hh
    float sv[32];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) s = Op16<false>::mfma32(__builtin_bit_cast(bf16x8, kf[t][m]), qf[m], s);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hh;
            const bool vis = ((key >= a.lo1) & (key < a.hi1)) | ((key >= a.lo2) & (key < a.hi2));  // hi <= P: a key >= P is never visible
            sv[16 * t + r] = vis ? s[r] : -INFINITY;
            mx = fmaxf(mx, sv[16 * t + r]);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mu = (mx == -INFINITY) ? 0.f : mx;
    float p[32];
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 32; ++r) {
        p[r] = __builtin_amdgcn_exp2f((sv[r] - mu) * LOG2E);
        ps += p[r];
    }
    const float l = ps + __shfl_xor(ps, 32, 64);
    // O^T[d][q] = sum_keys V^T[d][key] P^T[key][q]: k-step kk of tile t multiplies the keys 32 t + 16 kk + 4 hh + {0..3} and + 8 + {0..3}
    // of this lane (the keys of p[16 t + 8 kk .. + 7]); V elements of keys >= P are selected to zero
    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const bf16x8 pb = pack8(p + 16 * t + 8 * kk);
            const int n0 = a.P - (k0 + 32 * t + 16 * kk + 4 * hh);  // live keys from the first group's first key on
            const uint2 a0 = keep_first(vf[t][kk][0][0], n0), a1 = keep_first(vf[t][kk][0][1], n0 - 8);
            const uint2 b0 = keep_first(vf[t][kk][1][0], n0), b1 = keep_first(vf[t][kk][1][1], n0 - 8);
            o0 = Op16<false>::mfma32(__builtin_bit_cast(bf16x8, make_uint4(a0.x, a0.y, a1.x, a1.y)), pb, o0);
            o1 = Op16<false>::mfma32(__builtin_bit_cast(bf16x8, make_uint4(b0.x, b0.y, b1.x, b1.y)), pb, o1);
        }
    if (qi < a.nb) {
        float* w = a.ws + (((int64_t)split * a.nH + head) * 32 + qi) * WS_STRIDE;
        if (hh == 0) { w[0] = mx; w[1] = l; }
#pragma unroll
        for (int g = 0; g < 4; ++g) {  // dims 8 g + 4 hh + {0..3} of each half
            *reinterpret_cast<float4*>(w + 4 + 8 * g + 4 * hh) = make_float4(o0[4 * g], o0[4 * g + 1], o0[4 * g + 2], o0[4 * g + 3]);
            *reinterpret_cast<float4*>(w + 36 + 8 * g + 4 * hh) = make_float4(o1[4 * g], o1[4 * g + 1], o1[4 * g + 2], o1[4 * g + 3]);
        }
    }
}

// lmax: suffix rows the launch may touch (the size of sp, a multiple of 512 at or above it)
__global__ __launch_bounds__(256) void attn_shared_suffix_kernel(SharedAttnArgs a, int nsplit, int lmax) {
    extern __shared__ float sp[];  // scores, then probabilities, zero padded to a multiple of 512 keys
    __shared__ float red[8];
    __shared__ float sq[64], sk[64], sv[64], so[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int head = blockIdx.x, b = blockIdx.y;
    const int cap = a.cap_suf;
    const int64_t bh = (int64_t)b * a.nH + head;
    bf16_t* Kb = a.Ks + bh * cap * 64;
    bf16_t* Vb = a.Vs + bh * 64 * cap;
    const int pos = a.pos_dev[b];
    const int ps = pos - a.base;   // the new token's row / column in the suffix cache
    const int lo = a.P - a.base;   // first live row
    if (ps < lo || ps >= lmax) {  // block-uniform.  The host keeps every position inside [P, base + lmax) (attn_shared.h); should one
        // ever lie outside, nothing is appended or read and the slot's row is NaN, which its logits then show
        if (tid < 64) a.O[(int64_t)b * a.nH * 64 + head * 64 + tid] = (bf16_t)0x7FC0;
        return;
    }
    const int Lk = ps + 1;
    {   // the new token of this head: wave 0 q, wave 1 k (appended), wave 2 v (appended), wave 3 idles through the same expressions
        const int Hq = a.nH * 64;
        const int sel = wave < 2 ? wave : 2;
        const bf16_t xin = a.qkv[(int64_t)b * 3 * Hq + sel * Hq + head * 64 + lane];
        const float lnw = (sel == 0 ? a.qw : a.kw)[lane], lnb = (sel == 0 ? a.qb : a.kb)[lane];
        const int dl = lane < a.rot ? lane : 0;
        const float cs = a.cosT[(int64_t)pos * a.rot + dl], sn = a.sinT[(int64_t)pos * a.rot + dl];
        const float y = decode_prep_lane(bf2f(xin), lnw, lnb, a.eps, cs, sn, a.rot, lane);
        if (wave == 0) {
            sq[lane] = bf2f(f2bf(y * 0.125f));
        } else if (wave == 1) {
            const bf16_t kb = f2bf(y);
            sk[lane] = bf2f(kb);
            Kb[(int64_t)ps * 64 + lane] = kb;
        } else if (wave == 2) {
            sv[lane] = bf2f(xin);
            Vb[(int64_t)lane * cap + ps] = xin;
        }
    }
    __syncthreads();
    // scores: 8 lanes per key row (16-byte chunk ch), 32 rows per pass; dead rows (< lo) and the row in LDS are not loaded
    const int r8 = tid >> 3, ch = tid & 7;
    float qv[8], skv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { qv[j] = sq[ch * 8 + j]; skv[j] = sk[ch * 8 + j]; }
    float mx = -INFINITY;
    for (int kt = lo & ~31; kt < Lk; kt += 32) {
        const int k = kt + r8;
        const bool vis = k >= lo && k < Lk;
        const uint4 kr = (vis && k != ps) ? *reinterpret_cast<const uint4*>(Kb + (int64_t)k * 64 + ch * 8) : make_uint4(0, 0, 0, 0);
        const bf16_t* e = reinterpret_cast<const bf16_t*>(&kr);
        float sc = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) sc = fmaf(qv[j], k == ps ? skv[j] : bf2f(e[j]), sc);
        sc += dpp_move<DPP_XOR1>(sc);
        sc += dpp_move<DPP_XOR2>(sc);
        sc += dpp_move<DPP_HALF_MIRROR>(sc);
        sc = vis ? sc : -INFINITY;
        if (k < Lk && ch == 0) sp[k] = sc;
        mx = fmaxf(mx, sc);
    }
    mx = wave_max_swap(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));  // finite: the new token sees itself
    const int Lkp = (Lk + 511) & ~511;
    float sum = 0.f;
    for (int k = tid; k < Lkp; k += 256) {
        float p = 0.f;
        if (k >= lo && k < Lk) {
            p = __builtin_amdgcn_exp2f((sp[k] - mx) * LOG2E);
            sum += p;
            p = bf2f(f2bf(p));  // P is rounded to bf16 before it multiplies V, as in every attention path
        }
        sp[k] = p;
    }
    sum = wave_sum_swap(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    const float ls = (red[4] + red[5]) + (red[6] + red[7]);
    // o[d] = sum_k p[k] V^T[d][k]: wave w owns dims 16 w .. 16 w + 15, a lane 8 consecutive keys of a 512-key pass
    float o[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.f;
    const bf16_t* vr = Vb + (int64_t)(wave * 16) * cap;
    for (int c = 0; c < Lkp; c += 512) {
        const int kk = c + 8 * lane;
        uint4 u[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) u[i] = kk < Lk ? *reinterpret_cast<const uint4*>(vr + (int64_t)i * cap + kk) : make_uint4(0, 0, 0, 0);
        const float4 p0 = *reinterpret_cast<const float4*>(sp + kk);
        const float4 p1 = *reinterpret_cast<const float4*>(sp + kk + 4);
        const float pr[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const bf16_t* e = reinterpret_cast<const bf16_t*>(&u[i]);
            const float svi = sv[wave * 16 + i];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = kk + j;
                const float v = key == ps ? svi : ((key >= lo && key < Lk) ? bf2f(e[j]) : 0.f);  // dead or stale elements never multiply
                o[i] = fmaf(pr[j], v, o[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = wave_sum_swap(o[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) so[wave * 16 + i] = o[i];
    }
    __syncthreads();
    // merge with the prefix partials in split order; a partial with no visible key (m = -inf) contributes nothing
    if (tid < 64) {
        const float* w0 = a.ws + ((int64_t)head * 32 + b) * WS_STRIDE;
        const int64_t wstep = (int64_t)a.nH * 32 * WS_STRIDE;
        float M = mx;
        for (int i = 0; i < nsplit; ++i) M = fmaxf(M, w0[i * wstep]);
        float L = 0.f, acc = 0.f;
        for (int i = 0; i < nsplit; ++i) {
            const float* w = w0 + i * wstep;
            const float mi = w[0];
            const float sc = (mi == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((mi - M) * LOG2E);
            L += w[1] * sc;
            acc += w[4 + tid] * sc;
        }
        const float sc = __builtin_amdgcn_exp2f((mx - M) * LOG2E);
        L += ls * sc;
        acc += so[tid] * sc;
        a.O[(int64_t)b * a.nH * 64 + head * 64 + tid] = f2bf(acc * (1.0f / L));
    }
}

}  // namespace

namespace showo {

int64_t shared_attn_ws_elems(int nH, int P) {
    return (int64_t)((P + KSPLIT - 1) / KSPLIT) * nH * 32 * WS_STRIDE;
}

int attn_decode_shared(SharedAttnArgs a, hipStream_t s) {
    if (!a.qkv || !a.qw || !a.qb || !a.kw || !a.kb || !a.cosT || !a.sinT || !a.Kp || !a.Vp || !a.Ks || !a.Vs || !a.pos_dev || !a.O || !a.ws)
        return set_error_msg(1, "attn_decode_shared: null argument");
    if (a.nb < 1 || a.nb > 32 || a.nH < 1 || a.nH > 65535) return set_error_msg(1, "attn_decode_shared: 1..32 slots, 1..65535 heads");
    if (a.rot < 2 || a.rot > 64 || (a.rot & (a.rot - 1))) return set_error_msg(1, "attn_decode_shared: rotary_dim must be a power of two in 2..64");
    if (a.cap_pre < 64 || a.cap_suf < 64 || (a.cap_pre % 64) || (a.cap_suf % 64)) return set_error_msg(1, "attn_decode_shared: capacities must be multiples of 64");
    if (a.P < 1 || a.P > a.cap_pre) return set_error_msg(5, "attn_decode_shared: the prefix exceeds its cache's capacity");
    if (((uintptr_t)a.Kp | (uintptr_t)a.Vp | (uintptr_t)a.Ks | (uintptr_t)a.Vs | (uintptr_t)a.ws) & 15)
        return set_error_msg(1, "attn_decode_shared: 16-byte alignment required");
    a.base = a.P & ~63;
    a.hi1 = a.hi1 < a.P ? a.hi1 : a.P;
    a.hi2 = a.hi2 < a.P ? a.hi2 : a.P;
    a.lo1 = a.lo1 > 0 ? a.lo1 : 0;
    a.lo2 = a.lo2 > 0 ? a.lo2 : 0;
    const int nsplit = (a.P + KSPLIT - 1) / KSPLIT;
    if (nsplit > 65535) return set_error_msg(5, "attn_decode_shared: prefix too long");
    int rows = a.cap_suf;  // suffix rows a launch may touch
    if (a.lk_max > 0 && a.lk_max - a.base < rows) rows = a.lk_max - a.base;
    if (rows <= a.P - a.base) return set_error_msg(5, "attn_decode_shared: no room behind the prefix");
    const int lmax = rows;
    const size_t smem = (size_t)((rows + 511) & ~511) * sizeof(float);
    if (smem > 60000) return set_error_msg(5, "attn_decode_shared: suffix longer than the single-block kernel supports");
    attn_shared_prefix_kernel<<<dim3(a.nH, nsplit), dim3(64), 0, s>>>(a);
    SHOWO_CHECK_HIP(hipGetLastError());
    attn_shared_suffix_kernel<<<dim3(a.nH, a.nb), dim3(256), smem, s>>>(a, nsplit, lmax);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace showo

extern "C" int showo_attn_shared_ws_elems(int nH, int P) {
    if (nH < 1 || P < 1) return 0;
    const int64_t n = showo::shared_attn_ws_elems(nH, P);
    return n > 0x7fffffff ? 0 : (int)n;  // 0: no size an int can name
}

extern "C" int showo_attn_decode_shared(const uint16_t* qkv, const float* qln_w, const float* qln_b, const float* kln_w, const float* kln_b,
                                        const float* cosT, const float* sinT, const uint16_t* k_pre, const uint16_t* vt_pre, int cap_pre,
                                        uint16_t* k_suf, uint16_t* vt_suf, int cap_suf, const int32_t* pre_iv, int P, const int* pos_dev,
                                        int lk_max, uint16_t* O, float* ws, int nb, int nH, int rot, float eps, void* stream) {
    if (!pre_iv) return set_error_msg(1, "attn_decode_shared: null argument");
    SharedAttnArgs a{qkv, qln_w, qln_b, kln_w, kln_b, cosT, sinT, k_pre, vt_pre, cap_pre, k_suf, vt_suf, cap_suf,
                     pre_iv[0], pre_iv[1], pre_iv[2], pre_iv[3], P, 0, pos_dev, lk_max, O, ws, nb, nH, rot, eps};
    return showo::attn_decode_shared(a, (hipStream_t)stream);
}
