// Per-row symmetric int8 weight format: the weight images the KV-cached decode streams under showo_engine_set_precision(e, 3).
//
//   amax = max_k |w[n,k]|     scale[n] = amax / 127.0f                       (IEEE fp32 division)
//   q[n,k] = clamp(rint(w[n,k] / scale[n]), -127, 127)                       (IEEE division, round half to even; never -128)
//   amax < 2^-100 (all-zero rows included): scale[n] = 1, q[n,:] = 0         (every step stays clear of fp32 denormals)
//
// The quantiser is a load-time kernel (one pass per weight upload), not a hot path: one block per row, two passes over the row.
// The maximum is order-independent, so the result does not depend on the reduction tree.
#include "common.h"
#include "engine.h"
#include "../../include/showo_hip.h"

using namespace showo;

namespace {

constexpr float Q8_TINY = 7.888609052210118e-31f;  // 2^-100

// bad: set to 1 when a row holds NaN / inf (plain vector store of the same value from every thread that sees one)
__global__ __launch_bounds__(256) void quantize_rows_kernel(const float* __restrict__ w, int64_t K, int8_t* __restrict__ q,
                                                            float* __restrict__ scale, int* __restrict__ bad) {
    __shared__ float red[4];
    const int64_t n = blockIdx.x;
    const float* row = w + n * K;
    float m = 0.f;
    bool nonfinite = false;
    for (int64_t k = threadIdx.x; k < K; k += 256) {
        const float a = fabsf(row[k]);
        if (!(a <= 3.402823466e+38f)) nonfinite = true;  // NaN or inf
        else m = fmaxf(m, a);
    }
    if (nonfinite) *bad = 1;
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    const float amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const bool live = amax >= Q8_TINY;
    const float s = live ? amax / 127.0f : 1.0f;
    if (threadIdx.x == 0) scale[n] = s;
    int8_t* qrow = q + n * K;
    for (int64_t k = threadIdx.x; k < K; k += 256) {
        const float r = rintf(row[k] / s);
        const float c = fminf(fmaxf(r, -127.0f), 127.0f);
        qrow[k] = live ? (int8_t)(int)c : (int8_t)0;
    }
}

__global__ void dequantize_rows_kernel(const int8_t* __restrict__ q, const float* __restrict__ scale, int64_t K, int64_t total,
                                       float* __restrict__ w) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        w[i] = (float)q[i] * scale[i / K];
}
// the bf16 image of the dequantised weights: what the MFMA GEMMs of precision 3 multiply (exact for power-of-two scales)
__global__ void dequantize_rows_bf16_kernel(const int8_t* __restrict__ q, const float* __restrict__ scale, int64_t K, int64_t total,
                                            bf16_t* __restrict__ w) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        w[i] = f2bf((float)q[i] * scale[i / K]);
}
// bad |= 1: a q of -128;  bad |= 2: a scale that is not positive and finite  (same-value stores; the two bits come from two launches)
__global__ void validate_q_kernel(const int8_t* __restrict__ q, int64_t total, int* __restrict__ bad) {
    bool b = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) b |= q[i] == -128;
    if (b) bad[0] = 1;
}
__global__ void validate_scale_kernel(const float* __restrict__ s, int64_t N, int* __restrict__ bad) {
    bool b = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x)
        b |= !(s[i] > 0.f && s[i] <= 3.402823466e+38f);
    if (b) bad[1] = 1;
}

int grid_for(int64_t total) {
    const int64_t b = (total + 255) / 256;
    return (int)(b < 4096 ? (b > 0 ? b : 1) : 4096);
}

// bad: two device ints owned by the caller, zeroed on the stream by flags_zero and read back (synchronising) by flags_read
int flags_zero(int* bad, hipStream_t s) {
    SHOWO_CHECK_HIP(hipMemsetAsync(bad, 0, 2 * sizeof(int), s));
    return 0;
}
int flags_read(const int* bad, int (&host)[2], hipStream_t s) {
    hipError_t e = hipMemcpyAsync(host, bad, 2 * sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return set_error_hip(e, "quantiser flag read-back", __FILE__, __LINE__);
    return 0;
}

}  // namespace

// the public entry point owns a flag word per call; the engine's loader passes its own (q8_quantize_rows: no allocation per tensor)
extern "C" int showo_quantize_rows_i8(const float* w, int64_t N, int64_t K, int8_t* q, float* scale, void* stream) {
    int* bad = nullptr;
    SHOWO_CHECK_HIP(hipMalloc((void**)&bad, 2 * sizeof(int)));
    const int rc = showo::q8_quantize_rows(w, N, K, q, scale, bad, (hipStream_t)stream);
    hipFree(bad);
    return rc;
}

extern "C" int showo_dequantize_rows_i8(const int8_t* q, const float* scale, int64_t N, int64_t K, float* w, void* stream) {
    if (!w || !q || !scale) return set_error_msg(1, "dequantize_rows_i8: null argument");
    if (N < 1 || K < 1) return set_error_msg(1, "dequantize_rows_i8: bad shape");
    dequantize_rows_kernel<<<dim3(grid_for(N * K)), dim3(256), 0, (hipStream_t)stream>>>(q, scale, K, N * K, w);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

namespace showo {
// showo_quantize_rows_i8 with a caller-owned flag word (bad: 2 device ints); synchronises the stream
int q8_quantize_rows(const float* w, int64_t N, int64_t K, int8_t* q, float* scale, int* bad, hipStream_t s) {
    if (!w || !q || !scale || !bad) return set_error_msg(1, "quantize_rows_i8: null argument");
    if (N < 1 || K < 1 || N > 0x7fffffff) return set_error_msg(1, "quantize_rows_i8: bad shape");
    int rc = flags_zero(bad, s);
    if (rc) return rc;
    quantize_rows_kernel<<<dim3((unsigned)N), dim3(256), 0, s>>>(w, K, q, scale, bad);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error_hip(e, "quantize_rows launch", __FILE__, __LINE__);
    int host[2] = {0, 0};
    rc = flags_read(bad, host, s);
    if (rc) return rc;
    if (host[0]) return set_error_msg(8, "quantize_rows_i8: a row holds NaN or inf; no int8 image is built from it");
    return 0;
}
int q8_dequant_bf16(const int8_t* q, const float* scale, int64_t N, int64_t K, bf16_t* w, hipStream_t s) {
    dequantize_rows_bf16_kernel<<<dim3(grid_for(N * K)), dim3(256), 0, s>>>(q, scale, K, N * K, w);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}
// |q| <= 127 everywhere and every scale positive and finite, else an error (synchronises the stream)
int q8_validate(const int8_t* q, const float* scale, int64_t N, int64_t K, int* bad, hipStream_t s) {
    int rc = flags_zero(bad, s);
    if (rc) return rc;
    validate_q_kernel<<<dim3(grid_for(N * K)), dim3(256), 0, s>>>(q, N * K, bad);
    validate_scale_kernel<<<dim3(grid_for(N)), dim3(256), 0, s>>>(scale, N, bad);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error_hip(e, "q8 validate launch", __FILE__, __LINE__);
    int host[2] = {0, 0};
    rc = flags_read(bad, host, s);
    if (rc) return rc;
    if (host[0]) return set_error_msg(8, "engine_load_q8: q holds -128 (the format is symmetric: |q| <= 127)");
    if (host[1]) return set_error_msg(8, "engine_load_q8: every scale must be positive and finite");
    return 0;
}
}  // namespace showo
