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

// ---- nucleus (top-p) draw -----------------------------------------------------------------------------------------------------------
// sample_topk_row with the reference's top_k_top_p_filtering (models/sampling.py:80-118) between the top-k filter and the draw.
// x_i = logits[i] / T (fp32 division).
//   1. top-k exactly as sample_topk_row: keep x >= (top_k-th largest x), ties with the k-th value stay, top_k <= 0 or >= V: no filter.
//      The survivors are the candidates.
//   2. p = softmax over the candidates.
//   3. token i is kept iff the probability mass of the candidates with STRICTLY LARGER x is <= top_p.
//   token = argmax_i p'_i / E_i, p' = p renormalised over the kept set, E as in sample_topk_row (injected row, or Philox(seed; step, i)
//   with the same counter layout, 0x77), lowest index among ties.
// Rule 3 is the reference's rule wherever no tie sits at the cut (it sorts, shifts the cumulative mass right by one and drops what
// lies beyond top_p); the largest token has no mass above it, so it always stays (min_tokens_to_keep = 1); the rule does not depend on a
// sort order; and it is tie-inclusive: every candidate equal to the cut value stays, like the top-k rule.  Callers take this function
// only for 0 < top_p < 1; top_p >= 1 is sample_topk_row itself.
//
// The cut is a radix select BY MASS over order_key: four 8-bit passes, each a 256-bin histogram of the weights of the keys that match
// the prefix found so far, then one thread walks the bins from the top, carrying the mass above the prefix region, to the lowest
// non-empty bin whose mass above is still within top_p.  Everything downstream compares bits, so the masses are integers (float LDS
// atomics add in no fixed order): w_i = (uint64)(expf(x_i - mx) * 2^40), mx the candidates' max -- the scaling is exact, the
// conversion truncates, w <= 2^40 and the sums stay below 2^64 for V < 2^24 -- added with 64-bit integer LDS atomics, and
//   kept(i)  <=>  (double)A_i <= (double)top_p * (double)S,   A_i = sum of w over candidates with x > x_i,  S = sum of w over candidates.
// A candidate with w == 0 (x < mx - 27.7) has A = S and is never kept.  The normaliser and the p / E arg-max then run over the kept set
// in sample_topk_row's float reduction order.  Valid in thread 0.
struct RowNucleusSmem {
    RowPickSmem pick;
    unsigned long long mass[256];
    unsigned long long above;  // integer mass above the prefix region
    unsigned long long total;  // S
};

__device__ __forceinline__ int sample_topk_topp_row(const float* __restrict__ logits, int V, int top_k, float top_p, float T,
                                                    const float* __restrict__ en, uint64_t seed, int step, RowNucleusSmem& ns) {
    RowPickSmem& sm = ns.pick;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t thr = 0;  // candidates: keys >= thr
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
                sm.sel[1] = k - cum;
            }
            __syncthreads();
            prefix |= sm.sel[0] << shift;
            mask |= 255u << shift;
            k = sm.sel[1];
            __syncthreads();
        }
        thr = prefix;
    }
    // max of the candidates (the largest candidate is always kept: also the max of the kept set)
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
    // the cut by mass: afterwards the kept set is { keys >= thr } again
    {
        uint32_t prefix = 0, mask = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) ns.mass[tid] = 0ull;
            __syncthreads();
            for (int i = tid; i < V; i += 1024) {
                const float x = __fdiv_rn(logits[i], T);
                const uint32_t key = order_key(x);
                if (key >= thr && (key & mask) == prefix) {
                    const unsigned long long w = (unsigned long long)(expf(x - mx) * 1099511627776.0f);
                    if (w) atomicAdd(&ns.mass[(key >> shift) & 255u], w);
                }
            }
            __syncthreads();
            if (tid == 0) {
                if (shift == 24) {
                    unsigned long long S = 0ull;
                    for (int b = 0; b < 256; ++b) S += ns.mass[b];
                    ns.total = S;
                    ns.above = 0ull;
                }
                const double lim = (double)top_p * (double)ns.total;
                unsigned long long A = ns.above, selA = A;
                int sel = 255;
                for (int b = 255; b >= 0; --b) {
                    if (!((double)A <= lim)) break;  // the bins below have at least this much above them
                    if (ns.mass[b]) { sel = b; selA = A; }
                    A += ns.mass[b];
                }
                sm.sel[0] = (unsigned)sel;
                ns.above = selA;
            }
            __syncthreads();
            prefix |= sm.sel[0] << shift;
            mask |= 255u << shift;
            __syncthreads();
        }
        thr = prefix;  // >= the top-k threshold: a candidate's key
    }
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

// ---- log-probability of a given token -------------------------------------------------------------------------------------------------
// For one fp32 logits row x[0, V) and a target t:
//   lp   = x[t] - max(x) - log sum_i exp(x[i] - max(x))     log-softmax of the RAW logits (temperature 1, no top-k / top-p filter)
//   rank = #{ i : x[i] > x[t] }                             strict: 0 for the arg-max and everything tied with it
// t < 0 (the -100 of the label convention): lp = 0, rank = -1.  t >= V: lp = NaN, rank = -1 (the embedding kernel's poisoning of
// out-of-range ids).  -inf entries add 0 to the sum; a -inf target gives lp = -inf; a row of -inf alone gives NaN.
//
// Two passes over the row (it was just written by the lm_head and sits in L2): max and rank, then the sum.  The row is read with
// 16-byte loads behind a peel to its alignment (rows of a [n, 58498] block alternate between 8- and 16-byte alignment), so WHICH lane
// meets which element depends on where the row lies.  The result must not: the same row bits give the same lp bits from every caller
// (stand-alone, batch-1 loop, batched slot, scoring).  The max and the rank are order-free by nature; the sum is made order-free the
// way the nucleus cut is: w_i = (uint64)(expf(x_i - max) * 2^40) -- the scaling is exact, the conversion truncates, w <= 2^40 and
// the total stays below 2^64 for V < 2^24 -- added as integers.  The arg-max term is exactly 2^40, so the total S >= 2^40 and the
// truncation costs at most V 2^-40 (5e-8 at V = 58498) relative: below the fp32 rounding of the final logf.  Valid in thread 0.
struct RowLogprobSmem {
    float red_f[16];
    int red_i[16];
    unsigned long long red_w[16];
};
struct RowLogprob {
    float lp;
    int rank;
};

// f(v) for every element of row[0, V): the elements in front of the first 16-byte boundary and behind the last whole quad one by
// one, the quads in between as float4
template <class F>
__device__ __forceinline__ void row_for_each_1024(const float* __restrict__ row, int V, F&& f) {
    const int tid = threadIdx.x;
    int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);
    if (head > V) head = V;
    const int n4 = (V - head) >> 2, tail0 = head + 4 * n4;
    if (tid < head) f(row[tid]);
    const float4* __restrict__ q = reinterpret_cast<const float4*>(row + head);
    for (int i = tid; i < n4; i += 1024) {
        const float4 v = q[i];
        f(v.x); f(v.y); f(v.z); f(v.w);
    }
    if (tid < V - tail0) f(row[tail0 + tid]);
}

// The same walk with the element's index: f(v, i) for every i in [0, V)
template <class F>
__device__ __forceinline__ void row_for_each_idx_1024(const float* __restrict__ row, int V, F&& f) {
    const int tid = threadIdx.x;
    int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);
    if (head > V) head = V;
    const int n4 = (V - head) >> 2, tail0 = head + 4 * n4;
    if (tid < head) f(row[tid], tid);
    const float4* __restrict__ q = reinterpret_cast<const float4*>(row + head);
    for (int i = tid; i < n4; i += 1024) {
        const float4 v = q[i];
        const int at = head + 4 * i;
        f(v.x, at); f(v.y, at + 1); f(v.z, at + 2); f(v.w, at + 3);
    }
    if (tid < V - tail0) f(row[tail0 + tid], tail0 + tid);
}

// The normaliser of a row's log-softmax, shared by logprob_row and the beam selection (beam.hip): mx = max(x) and the integer sum
// S = sum_i (uint64)(expf(x_i - mx) * 2^40) (0 for a row whose max is not finite); count = sum_i count_of(x_i), an int the first pass
// adds up on the way (logprob_row: the rank).  mx and count are valid in every thread, S in thread 0.
struct RowNorm {
    float mx;
    int count;
    unsigned long long S;
};
template <class C>
__device__ __forceinline__ RowNorm row_norm_1024(const float* __restrict__ row, int V, RowLogprobSmem& sm, C&& count_of) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float mx = -INFINITY;
    int above = 0;
    row_for_each_1024(row, V, [&](float v) { mx = fmaxf(mx, v); above += count_of(v); });
    mx = wave_max(mx);
    for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
    if (lane == 0) { sm.red_f[wave] = mx; sm.red_i[wave] = above; }
    __syncthreads();
    mx = sm.red_f[0];
    above = sm.red_i[0];
    for (int w = 1; w < 16; ++w) { mx = fmaxf(mx, sm.red_f[w]); above += sm.red_i[w]; }
    unsigned long long acc = 0ull;
    if (mx > -INFINITY && mx < INFINITY)  // (a row of -inf alone, or one with +inf: x - mx is NaN; the sum stays 0 and the result is NaN)
        row_for_each_1024(row, V, [&](float v) { acc += (unsigned long long)(expf(v - mx) * 1099511627776.0f); });
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) sm.red_w[wave] = acc;
    __syncthreads();
    RowNorm n{mx, above, 0ull};
    if (tid == 0)
        for (int w = 0; w < 16; ++w) n.S += sm.red_w[w];
    __syncthreads();  // the caller may reuse sm
    return n;
}
// log S of a RowNorm with S != 0, as logprob_row subtracts it
__device__ __forceinline__ float row_norm_logS(unsigned long long S) { return logf((float)((double)S * (1.0 / 1099511627776.0))); }

__device__ __forceinline__ RowLogprob logprob_row(const float* __restrict__ row, int V, int64_t target, RowLogprobSmem& sm) {
    RowLogprob r{0.f, -1};
    if (target < 0 || target >= V) {  // block-uniform
        r.lp = target < 0 ? 0.f : __builtin_nanf("");
        r.rank = -1;
        return r;
    }
    const float xt = row[target];
    const RowNorm n = row_norm_1024(row, V, sm, [&](float v) { return (int)(v > xt); });
    if (threadIdx.x == 0) {
        r.lp = n.S ? (xt - n.mx) - row_norm_logS(n.S) : __builtin_nanf("");
        r.rank = n.count;
    }
    return r;
}

}  // namespace showo
