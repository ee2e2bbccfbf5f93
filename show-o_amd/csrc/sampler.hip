// Mask-predict (MaskGIT) sampler kernels for gfx950.
// Replaces (reference): models/modeling_showo.py:140-179 (CFG combine, slice, softmax, multinomial,
// confidence gather, mask_len clamp, write-back) and models/sampling.py:10-16,31-36 (log, gumbel_noise,
// mask_by_random_topk).  Arithmetic order follows the reference expression by expression (explicit
// __fmul_rn/__fadd_rn so hipcc cannot contract them into FMAs); only the libm-level functions
// (exp/log) can differ in the last ulp from the CPU.
#include "common.h"
#include "sample_row.h"
#include "../../include/showo_hip.h"
#include <cfloat>

using namespace showo;

namespace {

struct SampleArgs {
    const float *lc, *lu;
    int ld;
    float a1, a2;  // (1+w), w as fp32 scalars (python float -> fp32 tensor op)
    const int64_t* cur;
    int64_t mask_id;
    const float* exp_noise;
    uint64_t seed;
    uint32_t step;
    int64_t* sampled;
    float* sel;
    int N, V;
    // graph replay: the step index (and the seed: int32 pair at step_dev + 2) live in device memory -- the captured launch is
    // identical for every step and every call
    const int* step_dev;
    int64_t noise_stride;  // elements of injected noise per step
};

// one block per image token row; z staged in LDS (V*4 bytes, 32 KB at V=8192)
__global__ __launch_bounds__(256) void cfg_softmax_sample_kernel(SampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sz[];
    __shared__ float red_f[4];
    __shared__ int red_i[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (a.step_dev) {
        a.step = (uint32_t)*a.step_dev;
        a.seed = (uint64_t)(uint32_t)a.step_dev[2] | ((uint64_t)(uint32_t)a.step_dev[3] << 32);
        if (a.exp_noise) a.exp_noise += (int64_t)a.step * a.noise_stride;
    }
    const int64_t c = a.cur[row];
    if (c != a.mask_id) {  // known token: keeps its id, confidence = finfo.max (modeling_showo.py:154,164)
        if (tid == 0) { a.sampled[row] = c; a.sel[row] = FLT_MAX; }
        return;
    }
    const float* lc = a.lc + (int64_t)row * a.ld;
    const float* lu = a.lu ? a.lu + (int64_t)row * a.ld : nullptr;
    float mx = -INFINITY;
    for (int i = tid; i < a.V; i += 256) {
        float z = lu ? __fsub_rn(__fmul_rn(a.a1, lc[i]), __fmul_rn(a.a2, lu[i])) : lc[i];
        sz[i] = z;
        mx = fmaxf(mx, z);
    }
    mx = wave_max(mx);
    if (lane == 0) red_f[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red_f[0], red_f[1]), fmaxf(red_f[2], red_f[3]));
    __syncthreads();
    float s = 0.f;
    for (int i = tid; i < a.V; i += 256) {
        float e = expf(sz[i] - mx);
        sz[i] = e;
        s += e;
    }
    s = wave_sum(s);
    if (lane == 0) red_f[wave] = s;
    __syncthreads();
    s = (red_f[0] + red_f[1]) + (red_f[2] + red_f[3]);
    __syncthreads();
    // argmax_i p_i / E_i  (what torch.multinomial(p, 1) computes: q.exponential_(1); argmax(p / q))
    Philox ph(a.seed);
    float best = -1.f;
    int bi = 0x7fffffff;
    for (int i0 = tid * 4; i0 < a.V; i0 += 1024) {
        float e4[4];
        if (a.exp_noise) {
#pragma unroll
            for (int j = 0; j < 4; ++j) e4[j] = (i0 + j < a.V) ? a.exp_noise[(int64_t)row * a.V + i0 + j] : 1.f;
        } else {
            uint32_t r4[4];
            ph.gen((uint32_t)(i0 >> 2), (uint32_t)row, a.step, 0x51u, r4);
#pragma unroll
            for (int j = 0; j < 4; ++j) e4[j] = -logf(u32_to_unit(r4[j]));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int i = i0 + j;
            if (i < a.V) {
                float p = __fdiv_rn(sz[i], s);
                float sc = __fdiv_rn(p, e4[j]);
                if (sc > best || (sc == best && i < bi)) { best = sc; bi = i; }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        float ob = __shfl_xor(best, o, 64);
        int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { red_f[wave] = best; red_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (red_f[w] > best || (red_f[w] == best && red_i[w] < bi)) { best = red_f[w]; bi = red_i[w]; }
        a.sampled[row] = bi;
        a.sel[row] = __fdiv_rn(sz[bi], s);
    }
}

struct TopkArgs {
    const float* sel;
    const int64_t* sampled;
    int64_t *cur, *ids_c, *ids_u;
    int ld_ids, img_start;
    int64_t mask_id, id_offset;
    float mask_len_f, temp;
    const float* uniform;
    uint64_t seed;
    uint32_t step;
    uint8_t* masking_out;
    int N;
    const int* step_dev;   // graph replay: step index, schedule constants sched[0..steps) = mask_len, [steps..2 steps) = temperature
    const float* sched;
    int steps;
    int64_t noise_stride;
};

// one block per sample; confidences in LDS; k-th smallest by rank counting (N <= 4096)
__global__ __launch_bounds__(256) void mask_by_topk_kernel(TopkArgs a) {
    extern __shared__ __attribute__((aligned(16))) float conf[];
    __shared__ int cnt_unknown;
    __shared__ float cut_s;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (a.step_dev) {
        a.step = (uint32_t)*a.step_dev;
        a.seed = (uint64_t)(uint32_t)a.step_dev[2] | ((uint64_t)(uint32_t)a.step_dev[3] << 32);
        a.mask_len_f = a.sched[a.step];
        a.temp = a.sched[a.steps + a.step];
        if (a.uniform) a.uniform += (int64_t)a.step * a.noise_stride;
    }
    if (tid == 0) { cnt_unknown = 0; cut_s = INFINITY; }
    __syncthreads();
    Philox ph(a.seed);
    int local_unknown = 0;
    for (int i = tid; i < a.N; i += 256) {
        int64_t idx = (int64_t)b * a.N + i;
        if (a.cur[idx] == a.mask_id) local_unknown++;
        float u;
        if (a.uniform) {
            u = a.uniform[idx];
        } else {
            uint32_t r4[4];
            ph.gen((uint32_t)i, (uint32_t)b, a.step, 0x6bu, r4);
            u = u32_to_unit(r4[0]);
        }
        // gumbel_noise: -log(-log(u)) with log(t) = log(clamp(t, 1e-20)) (sampling.py:10-16)
        float g = -logf(fmaxf(-logf(fmaxf(u, 1e-20f)), 1e-20f));
        conf[i] = __fadd_rn(logf(fmaxf(a.sel[idx], 1e-20f)), __fmul_rn(a.temp, g));
    }
    if (local_unknown) atomicAdd(&cnt_unknown, local_unknown);
    __syncthreads();
    // mask_len = max(1, min(unknown - 1, floor(N * ratio)))  (modeling_showo.py:166-171), as floats then .long()
    float ml = fmaxf(1.0f, fminf((float)(cnt_unknown - 1), a.mask_len_f));
    int k = (int)ml;
    if (k > a.N - 1) k = a.N - 1;
    for (int i = tid; i < a.N; i += 256) {
        float x = conf[i];
        int less = 0, leq = 0;
        for (int j = 0; j < a.N; ++j) {
            float y = conf[j];
            less += (y < x);
            leq += (y <= x);
        }
        if (less <= k && k < leq) cut_s = x;  // same value from every writer
    }
    __syncthreads();
    const float cut = cut_s;
    for (int i = tid; i < a.N; i += 256) {
        int64_t idx = (int64_t)b * a.N + i;
        bool m = conf[i] < cut;
        int64_t sid = a.sampled[idx];
        int64_t tok = m ? a.mask_id : sid + a.id_offset;
        a.ids_c[(int64_t)b * a.ld_ids + a.img_start + i] = tok;
        if (a.ids_u) a.ids_u[(int64_t)b * a.ld_ids + a.img_start + i] = tok;
        a.cur[idx] = m ? a.mask_id : sid;
        if (a.masking_out) a.masking_out[idx] = m ? 1 : 0;
    }
}

__global__ void step_inc_kernel(int* step) {
    if (threadIdx.x == 0) *step += 1;
}

}  // namespace

// Device-side step mode (engine-internal, used while a denoise step is captured into a hipGraph): when set, both sampler
// kernels take the step index from *step_dev, the schedule constants from sched and offset injected noise themselves.
static const int* g_sampler_step_dev = nullptr;
static const float* g_sampler_sched = nullptr;
static int g_sampler_steps = 0;
namespace showo {
void sampler_set_device_step(const int* step_dev, const float* sched, int steps) {
    g_sampler_step_dev = step_dev; g_sampler_sched = sched; g_sampler_steps = steps;
}
int sampler_step_inc(int* step_dev, hipStream_t s) {
    step_inc_kernel<<<1, 64, 0, s>>>(step_dev);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
}  // namespace showo

extern "C" int showo_cfg_softmax_sample(const float* logits_c, const float* logits_u, int ld, float guidance,
                                        const int64_t* cur, int64_t mask_id, const float* exp_noise, uint64_t seed,
                                        uint32_t step, int64_t* sampled, float* sel_prob, int B, int N, int V,
                                        void* stream) {
    int rows = B * N;
    if (rows <= 0) return 0;
    if (V <= 0 || V > 40000) return set_error_msg(1, "sampler: V out of range (LDS staging supports V <= 40000)");
    SampleArgs a;
    a.lc = logits_c; a.lu = logits_u; a.ld = ld;
    a.a1 = (float)(1.0 + (double)guidance); a.a2 = guidance;
    a.cur = cur; a.mask_id = mask_id; a.exp_noise = exp_noise; a.seed = seed; a.step = step;
    a.step_dev = g_sampler_step_dev; a.noise_stride = (int64_t)rows * V;
    a.sampled = sampled; a.sel = sel_prob; a.N = N; a.V = V;
    size_t smem = (size_t)V * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        SHOWO_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(cfg_softmax_sample_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, 160000));
        attr_set = true;
    }
    cfg_softmax_sample_kernel<<<dim3(rows), dim3(256), smem, (hipStream_t)stream>>>(a);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int showo_mask_by_topk(const float* sel_prob, const int64_t* sampled, int64_t* cur, int64_t* ids_cond,
                                  int64_t* ids_uncond, int ld_ids, int img_start, int64_t mask_id, int64_t id_offset,
                                  float mask_len_f, float temperature, const float* uniform, uint64_t seed,
                                  uint32_t step, uint8_t* masking_out, int B, int N, void* stream) {
    if (B <= 0 || N <= 0) return 0;
    if (N > 4096) return set_error_msg(1, "mask_by_topk: N <= 4096 supported");
    TopkArgs a;
    a.sel = sel_prob; a.sampled = sampled; a.cur = cur; a.ids_c = ids_cond; a.ids_u = ids_uncond;
    a.ld_ids = ld_ids; a.img_start = img_start; a.mask_id = mask_id; a.id_offset = id_offset;
    a.mask_len_f = mask_len_f; a.temp = temperature; a.uniform = uniform; a.seed = seed; a.step = step;
    a.step_dev = g_sampler_step_dev; a.sched = g_sampler_sched; a.steps = g_sampler_steps; a.noise_stride = (int64_t)B * N;
    a.masking_out = masking_out; a.N = N;
    mask_by_topk_kernel<<<dim3(B), dim3(256), (size_t)N * sizeof(float), (hipStream_t)stream>>>(a);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// Next-token sampling of the AR decode (modeling_showo.py:220-228): x = logits / temperature; keep x >= (top_k-th
// largest x) (`logits[logits < v[:, [-1]]] = -inf`: ties with the k-th value stay); p = softmax(x); token =
// multinomial(p, 1) = argmax_i p_i / E_i with E ~ Exp(1) (asserted against torch in oracle/make_golden.py).
// One 1024-thread block; the vocabulary row (58 498 fp32 = 234 KB) stays in L2 and is re-read per pass: four 8-bit
// radix-select passes over an order-preserving key find the exact k-th largest value, then max, sum and the arg-max
// (sample_row.h sample_topk_row, which the batched sampled seam of decode_batch.hip calls as well).
// ------------------------------------------------------------------------------------------------------------------
namespace {
struct DecSampleArgs {
    const float* logits;
    int V, top_k;
    float temperature;
    const float* exp_noise;   // optional [*, V]: row `step` is used (parity tests); else Philox(seed; step)
    int64_t noise_stride;
    uint64_t seed;
    int step;                 // index of this draw within the generation ...
    const int* pos_dev;       // ... or step + (*pos_dev - pos_base) when the position lives on the device (graph replay)
    int pos_base;
    int64_t* tok;
};
__global__ __launch_bounds__(1024) void sample_topk_kernel(DecSampleArgs a) {
    __shared__ RowPickSmem sm;
    const int step = a.step + (a.pos_dev ? *a.pos_dev - a.pos_base : 0);
    const float* en = a.exp_noise ? a.exp_noise + (int64_t)step * a.noise_stride : nullptr;
    const int bi = sample_topk_row(a.logits, a.V, a.top_k, a.temperature, en, a.seed, step, sm);
    if (threadIdx.x == 0) a.tok[0] = bi;
}
// the same draw behind the nucleus filter (sample_row.h sample_topk_topp_row), 0 < top_p < 1
__global__ __launch_bounds__(1024) void sample_topk_topp_kernel(DecSampleArgs a, float top_p) {
    __shared__ RowNucleusSmem sm;
    const int step = a.step + (a.pos_dev ? *a.pos_dev - a.pos_base : 0);
    const float* en = a.exp_noise ? a.exp_noise + (int64_t)step * a.noise_stride : nullptr;
    const int bi = sample_topk_topp_row(a.logits, a.V, a.top_k, top_p, a.temperature, en, a.seed, step, sm);
    if (threadIdx.x == 0) a.tok[0] = bi;
}
}  // namespace

namespace showo {
int sample_topk_launch(const float* logits, int V, int top_k, float temperature, const float* exp_noise, int64_t noise_stride,
                       uint64_t seed, int step, const int* pos_dev, int pos_base, int64_t* tok, hipStream_t s) {
    if (!logits || !tok || V <= 0) return set_error_msg(1, "sample_topk: bad arguments");
    if (!(temperature > 0.f)) return set_error_msg(1, "sample_topk: temperature must be > 0");
    DecSampleArgs a{logits, V, top_k, temperature, exp_noise, noise_stride, seed, step, pos_dev, pos_base, tok};
    sample_topk_kernel<<<dim3(1), dim3(1024), 0, s>>>(a);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

// top_p >= 1: sample_topk_launch itself (the bits of a call without top_p); 0 < top_p < 1: the nucleus kernel; else error 1, no launch
int sample_topk_topp_launch(const float* logits, int V, int top_k, float top_p, float temperature, const float* exp_noise,
                            int64_t noise_stride, uint64_t seed, int step, const int* pos_dev, int pos_base, int64_t* tok, hipStream_t s) {
    if (!(top_p > 0.f)) return set_error_msg(1, "sample_topk_topp: top_p must be > 0 (>= 1: no nucleus filter)");
    if (top_p >= 1.f) return sample_topk_launch(logits, V, top_k, temperature, exp_noise, noise_stride, seed, step, pos_dev, pos_base, tok, s);
    if (!logits || !tok || V <= 0) return set_error_msg(1, "sample_topk_topp: bad arguments");
    if (V >= (1 << 24)) return set_error_msg(1, "sample_topk_topp: V < 2^24 supported (64-bit mass sums)");
    if (!(temperature > 0.f)) return set_error_msg(1, "sample_topk_topp: temperature must be > 0");
    DecSampleArgs a{logits, V, top_k, temperature, exp_noise, noise_stride, seed, step, pos_dev, pos_base, tok};
    sample_topk_topp_kernel<<<dim3(1), dim3(1024), 0, s>>>(a, top_p);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}
}  // namespace showo

// ------------------------------------------------------------------------------------------------------------------
// Log-probability and rank of a given token per logits row (sample_row.h logprob_row): one 1024-thread block per row.
// ------------------------------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(1024) void logprob_rows_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                            const int64_t* __restrict__ targets, float* __restrict__ lp,
                                                            int32_t* __restrict__ rank) {
    __shared__ RowLogprobSmem sm;
    const int r = blockIdx.x;
    const RowLogprob o = logprob_row(logits + (int64_t)r * ld, V, targets[r], sm);
    if (threadIdx.x == 0) {
        lp[r] = o.lp;
        if (rank) rank[r] = o.rank;
    }
}
// the decode loop's form: the row of the step that just stored its token (*tok) and advanced *pos; entry *pos - 1 - base
__global__ __launch_bounds__(1024) void logprob_step_kernel(const float* __restrict__ logits, int V, const int64_t* __restrict__ tok,
                                                            const int* __restrict__ pos, int base, float* __restrict__ lp,
                                                            int32_t* __restrict__ rank) {
    __shared__ RowLogprobSmem sm;
    const RowLogprob o = logprob_row(logits, V, *tok, sm);
    if (threadIdx.x == 0) {
        const int j = *pos - 1 - base;
        lp[j] = o.lp;
        if (rank) rank[j] = o.rank;
    }
}
}  // namespace

namespace showo {
int logprob_step_launch(const float* logits, int V, const int64_t* tok, const int* pos_dev, int pos_base, float* lp, int32_t* rank,
                        hipStream_t s) {
    if (!logits || !tok || !pos_dev || !lp || V <= 0) return set_error_msg(1, "logprob_step: bad arguments");
    logprob_step_kernel<<<dim3(1), dim3(1024), 0, s>>>(logits, V, tok, pos_dev, pos_base, lp, rank);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}
}  // namespace showo

extern "C" int showo_logprob_rows(const float* logits, int64_t ld, int nrows, int V, const int64_t* targets, float* logprob,
                                  int32_t* rank, void* stream) {
    if (nrows == 0) return 0;
    if (!logits || !targets || !logprob || nrows < 0) return set_error_msg(1, "logprob_rows: bad arguments");
    if (V < 1 || V >= (1 << 24) || ld < V) return set_error_msg(1, "logprob_rows: needs 1 <= V < 2^24 (64-bit mass sums) and ld >= V");
    if ((uintptr_t)logits & 3) return set_error_msg(1, "logprob_rows: logits must be 4-byte aligned");
    logprob_rows_kernel<<<dim3(nrows), dim3(1024), 0, (hipStream_t)stream>>>(logits, ld, V, targets, logprob, rank);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int showo_sample_topk_topp(const float* logits, int V, int top_k, float top_p, float temperature, const float* exp_noise,
                                      uint64_t seed, int step, int64_t* tok, void* stream) {
    return showo::sample_topk_topp_launch(logits, V, top_k, top_p, temperature, exp_noise, (int64_t)V, seed, step, nullptr, 0, tok,
                                          (hipStream_t)stream);
}

extern "C" int showo_sample_topk(const float* logits, int V, int top_k, float temperature, const float* exp_noise, uint64_t seed,
                                 int step, int64_t* tok, void* stream) {
    return showo::sample_topk_launch(logits, V, top_k, temperature, exp_noise, (int64_t)V, seed, step, nullptr, 0, tok,
                                     (hipStream_t)stream);
}
