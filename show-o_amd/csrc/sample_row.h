// Per-row token picks of the AR decode, shared by the batch-1 sampler (sampler.hip sample_topk_kernel), the batched greedy seam and the
// batched sampled seam (decode_batch.hip): one 1024-thread block per logits row, the result in thread 0.  Both decode paths call the
// same function, so a batched slot draws the bits of its batch-1 run by construction.
#pragma once
#include "common.h"

namespace showo {

__device__ __forceinline__ uint32_t order_key(float x) {  // ascending float order -> ascending unsigned order
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct RowPickSmem {
    unsigned hist[256];
    unsigned sel[2];
    float red_f[16];
    int red_i[16];
};

// arg-max of row[0, V): the first maximal index (showo_argmax_f32's rule).  Valid in thread 0.
__device__ __forceinline__ int argmax_row_1024(const float* __restrict__ row, int V, RowPickSmem& sm) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid; i < V; i += 1024) {
        const float v = row[i];
        if (v > best || (v == best && i < bi)) { best = v; bi = i; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { sm.red_f[wave] = best; sm.red_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (sm.red_f[w] > best || (sm.red_f[w] == best && sm.red_i[w] < bi)) { best = sm.red_f[w]; bi = sm.red_i[w]; }
    }
    return bi;
}

// Next-token draw of the AR decode (modeling_showo.py:220-228): x = logits / T; keep x >= (top_k-th largest x) (ties with the k-th
// value stay; top_k <= 0 or >= V: no filter); p = softmax(x); token = argmax_i p_i / E_i, E = en[i] when en != NULL, else
// Philox(seed; step, i).  Four 8-bit radix-select passes over an order-preserving key find the exact k-th largest value, then max, sum
// and the arg-max (lowest index among ties).  The row stays in L2 and is re-read per pass.  Valid in thread 0.
__device__ __forceinline__ int sample_topk_row(const float* __restrict__ logits, int V, int top_k, float T, const float* __restrict__ en,
                                               uint64_t seed, int step, RowPickSmem& sm) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t thr = 0;  // keep keys >= thr
    if (top_k > 0 && top_k < V) {
        uint32_t prefix = 0, mask = 0;
        unsigned k = (unsigned)top_k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) sm.hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < V; i += 1024) {
                const uint32_t key = order_key(__fdiv_rn(logits[i], T));
                if ((key & mask) == prefix) atomicAdd(&sm.hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned cum = 0;
                int b = 255;
                for (; b > 0; --b) {
                    if (cum + sm.hist[b] >= k) break;
                    cum += sm.hist[b];
                }
                sm.sel[0] = (unsigned)b;
                sm.sel[1] = k - cum;  // rank of the wanted element inside bin b
            }
            __syncthreads();
            prefix |= sm.sel[0] << shift;
            mask |= 255u << shift;
            k = sm.sel[1];
            __syncthreads();
        }
        thr = prefix;
    }
    // max of the kept values
    float mx = -INFINITY;
    for (int i = tid; i < V; i += 1024) {
        const float x = __fdiv_rn(logits[i], T);
        if (order_key(x) >= thr) mx = fmaxf(mx, x);
    }
    mx = wave_max(mx);
    if (lane == 0) sm.red_f[wave] = mx;
    __syncthreads();
    mx = sm.red_f[0];
    for (int w = 1; w < 16; ++w) mx = fmaxf(mx, sm.red_f[w]);
    __syncthreads();
    float sum = 0.f;
    for (int i = tid; i < V; i += 1024) {
        const float x = __fdiv_rn(logits[i], T);
        if (order_key(x) >= thr) sum += expf(x - mx);
    }
    sum = wave_sum(sum);
    if (lane == 0) sm.red_f[wave] = sum;
    __syncthreads();
    sum = 0.f;
    for (int w = 0; w < 16; ++w) sum += sm.red_f[w];
    __syncthreads();
    Philox ph(seed);
    float best = -1.f;
    int bi = 0x7fffffff;
    for (int i0 = tid * 4; i0 < V; i0 += 4096) {
        float e4[4];
        if (en) {
#pragma unroll
            for (int j = 0; j < 4; ++j) e4[j] = (i0 + j < V) ? en[i0 + j] : 1.f;
        } else {
            uint32_t r4[4];
            ph.gen((uint32_t)(i0 >> 2), 0u, (uint32_t)step, 0x77u, r4);
#pragma unroll
            for (int j = 0; j < 4; ++j) e4[j] = -logf(u32_to_unit(r4[j]));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = i0 + j;
            if (i < V) {
                const float x = __fdiv_rn(logits[i], T);
                if (order_key(x) >= thr) {
                    const float sc = __fdiv_rn(__fdiv_rn(expf(x - mx), sum), e4[j]);
                    if (sc > best || (sc == best && i < bi)) { best = sc; bi = i; }
                }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { sm.red_f[wave] = best; sm.red_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (sm.red_f[w] > best || (sm.red_f[w] == best && sm.red_i[w] < bi)) { best = sm.red_f[w]; bi = sm.red_i[w]; }
    }
    return bi;
}

}  // namespace showo
