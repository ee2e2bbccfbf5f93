// Exponential moving average of the weights (reference models/training_utils.py:61-296, `EMA.step`), DESIGN.md "EMA of the weights".
//
// One step of a shadow tensor s against its parameter p is the reference's  s.sub_(one_minus_decay * (s - p)):  three fp32 operations,
// each rounded on its own (showo::ema_next in common.h keeps them apart: no fma).  A parameter that does not train copies: s = p.
//
// Both kernels run over a segment table (EmaSeg: shadow, parameter, optional engine destination, n) cut into chunks of ADAM_CHUNK
// elements, one block per chunk, like the multi-tensor AdamW.  A chunk whose pointers are 16-byte aligned (every chunk start is a
// multiple of ADAM_CHUNK, so the segment's base pointers decide) moves float4s and finishes its last n % 4 elements one by one; any
// other chunk moves single floats.  The arithmetic per element is the same on both paths.
//   ema_multi_kernel   s' = ema_next(s, p, omd)  (mode 0)   |   s' = p  (mode 1)
//   ema_swap_kernel    p <-> s in place; the value going into p is also written to the engine's image (bf16 cast or fp32 copy), from
//                      the register that holds it -- no third copy of the weights exists, and two swaps restore every bit
#include "common.h"
#include "../../include/showo_hip.h"
#include <cstring>
#include <vector>

using namespace showo;

namespace {

__device__ __forceinline__ bool aligned16(const void* a, const void* b) { return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }

__global__ __launch_bounds__(256) void ema_multi_kernel(const EmaSeg* __restrict__ segs, const int* __restrict__ modes,
                                                        const int* __restrict__ seg_of, const int64_t* __restrict__ start_of, float omd) {
    const int si = seg_of[blockIdx.x];
    const EmaSeg sg = segs[si];
    const int copy = modes[si];
    const int64_t i0 = start_of[blockIdx.x];
    const int64_t i1 = i0 + ADAM_CHUNK < sg.n ? i0 + ADAM_CHUNK : sg.n;
    int64_t body = i0;  // [i0, body) goes in float4s
    if (aligned16(sg.s, sg.p)) {
        body = i0 + ((i1 - i0) & ~(int64_t)3);
        for (int64_t i = i0 + threadIdx.x * 4; i < body; i += 1024) {
            const float4 p = *reinterpret_cast<const float4*>(sg.p + i);
            float4 s = p;
            if (!copy) {
                s = *reinterpret_cast<const float4*>(sg.s + i);
                s.x = ema_next(s.x, p.x, omd);
                s.y = ema_next(s.y, p.y, omd);
                s.z = ema_next(s.z, p.z, omd);
                s.w = ema_next(s.w, p.w, omd);
            }
            *reinterpret_cast<float4*>(sg.s + i) = s;
        }
    }
    for (int64_t i = body + threadIdx.x; i < i1; i += 256) {
        const float p = sg.p[i];
        sg.s[i] = copy ? p : ema_next(sg.s[i], p, omd);
    }
}

__global__ __launch_bounds__(256) void ema_swap_kernel(const EmaSeg* __restrict__ segs, const int* __restrict__ seg_of,
                                                       const int64_t* __restrict__ start_of) {
    const EmaSeg sg = segs[seg_of[blockIdx.x]];
    const int64_t i0 = start_of[blockIdx.x];
    const int64_t i1 = i0 + ADAM_CHUNK < sg.n ? i0 + ADAM_CHUNK : sg.n;
    int64_t body = i0;
    if (aligned16(sg.s, sg.p) && (((uintptr_t)sg.dst32) & 15) == 0 && (((uintptr_t)sg.dst16) & 7) == 0) {
        body = i0 + ((i1 - i0) & ~(int64_t)3);
        for (int64_t i = i0 + threadIdx.x * 4; i < body; i += 1024) {
            const float4 p = *reinterpret_cast<const float4*>(sg.p + i);
            const float4 s = *reinterpret_cast<const float4*>(sg.s + i);
            *reinterpret_cast<float4*>(sg.p + i) = s;
            *reinterpret_cast<float4*>(sg.s + i) = p;
            if (sg.dst16) {
                ushort4 h;
                h.x = f2bf(s.x); h.y = f2bf(s.y); h.z = f2bf(s.z); h.w = f2bf(s.w);
                *reinterpret_cast<ushort4*>(sg.dst16 + i) = h;
            } else if (sg.dst32) {
                *reinterpret_cast<float4*>(sg.dst32 + i) = s;
            }
        }
    }
    for (int64_t i = body + threadIdx.x; i < i1; i += 256) {
        const float p = sg.p[i];
        const float s = sg.s[i];
        sg.p[i] = s;
        sg.s[i] = p;
        if (sg.dst16) sg.dst16[i] = f2bf(s);
        else if (sg.dst32) sg.dst32[i] = s;
    }
}

bool capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    hipStreamIsCapturing(s, &cs);
    return cs != hipStreamCaptureStatusNone;
}

}  // namespace

namespace showo {

void EmaTable::release() {
    if (segs) hipFree(segs);
    if (modes) hipFree(modes);
    if (seg_of) hipFree(seg_of);
    if (start_of) hipFree(start_of);
    segs = nullptr; modes = nullptr; seg_of = nullptr; start_of = nullptr;
    chunks = 0; count = 0;
    host_modes.clear();
}

// upload the table of `host` (segments of n == 0 are kept: they own no chunk); modes start as 0
int EmaTable::build(const std::vector<EmaSeg>& host) {
    release();
    if (host.empty()) return 0;
    std::vector<int> so;
    std::vector<int64_t> st;
    for (size_t k = 0; k < host.size(); ++k)
        for (int64_t at = 0; at < host[k].n; at += ADAM_CHUNK) { so.push_back((int)k); st.push_back(at); }
    SHOWO_CHECK_HIP(hipMalloc(&segs, host.size() * sizeof(EmaSeg)));
    SHOWO_CHECK_HIP(hipMalloc(&modes, host.size() * sizeof(int)));
    SHOWO_CHECK_HIP(hipMalloc(&seg_of, (so.size() + 1) * sizeof(int)));
    SHOWO_CHECK_HIP(hipMalloc(&start_of, (st.size() + 1) * sizeof(int64_t)));
    SHOWO_CHECK_HIP(hipMemcpy(segs, host.data(), host.size() * sizeof(EmaSeg), hipMemcpyHostToDevice));
    SHOWO_CHECK_HIP(hipMemset(modes, 0, host.size() * sizeof(int)));
    if (!so.empty()) {
        SHOWO_CHECK_HIP(hipMemcpy(seg_of, so.data(), so.size() * sizeof(int), hipMemcpyHostToDevice));
        SHOWO_CHECK_HIP(hipMemcpy(start_of, st.data(), st.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    host_modes.assign(host.size(), 0);
    chunks = (int)so.size();
    count = (int)host.size();
    return 0;
}

// the modes live on the device next to the table; a call with other modes than the last one re-uploads them (never inside a capture)
int EmaTable::set_modes(const int* m, hipStream_t s) {
    std::vector<int> want(count, 0);
    if (m)
        for (int k = 0; k < count; ++k) want[k] = m[k] ? 1 : 0;
    if (want == host_modes) return 0;
    if (capturing(s)) return set_error_msg(7, "ema: the modes of a table change outside a stream capture only");
    SHOWO_CHECK_HIP(hipStreamSynchronize(s));  // an earlier update on this stream may still read the old modes
    SHOWO_CHECK_HIP(hipMemcpy(modes, want.data(), want.size() * sizeof(int), hipMemcpyHostToDevice));
    host_modes.swap(want);
    return 0;
}

int EmaTable::update(float omd, hipStream_t s) const {
    if (chunks <= 0) return 0;
    ema_multi_kernel<<<dim3(chunks), dim3(256), 0, s>>>(segs, modes, seg_of, start_of, omd);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error_hip(e, "ema_multi launch", __FILE__, __LINE__);
    return 0;
}

int EmaTable::swap(hipStream_t s) const {
    if (chunks <= 0) return 0;
    ema_swap_kernel<<<dim3(chunks), dim3(256), 0, s>>>(segs, seg_of, start_of);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error_hip(e, "ema_swap launch", __FILE__, __LINE__);
    return 0;
}

}  // namespace showo

struct showo_ema_table { showo::EmaTable t; };

extern "C" int showo_ema_table_create(float* const* shadow, float* const* param, const int64_t* n, int count, uint16_t* const* dst_bf16,
                                      float* const* dst_f32, showo_ema_table** out) {
    if (!shadow || !param || !n || !out) return set_error_msg(1, "ema_table_create: null argument");
    if (count < 1) return set_error_msg(1, "ema_table_create: count must be at least 1");
    std::vector<EmaSeg> host;
    for (int k = 0; k < count; ++k) {
        if (n[k] < 0) return set_error_msg(1, "ema_table_create: negative element count");
        if (n[k] > 0 && (!shadow[k] || !param[k])) return set_error_msg(1, "ema_table_create: null tensor pointer");
        if ((((uintptr_t)shadow[k]) | ((uintptr_t)param[k])) & 3) return set_error_msg(1, "ema_table_create: fp32 tensors are 4-byte aligned");
        EmaSeg sg{shadow[k], param[k], dst_bf16 ? dst_bf16[k] : nullptr, dst_f32 ? dst_f32[k] : nullptr, n[k]};
        if (sg.dst16 && sg.dst32) return set_error_msg(1, "ema_table_create: a segment has one destination, 16-bit or fp32");
        if ((((uintptr_t)sg.dst16) & 1) || (((uintptr_t)sg.dst32) & 3)) return set_error_msg(1, "ema_table_create: misaligned destination");
        host.push_back(sg);
    }
    showo_ema_table* h = new showo_ema_table();
    int rc = h->t.build(host);
    if (rc) { h->t.release(); delete h; return rc; }
    *out = h;
    return 0;
}

extern "C" void showo_ema_table_destroy(showo_ema_table* h) {
    if (!h) return;
    h->t.release();
    delete h;
}

extern "C" int showo_ema_table_update(showo_ema_table* h, const int* modes, float omd, void* stream) {
    if (!h) return set_error_msg(1, "ema_table_update: null handle");
    if (!(omd >= 0.f && omd <= 1.f)) return set_error_msg(1, "ema_table_update: 1 - decay must lie in [0, 1]");
    int rc = h->t.set_modes(modes, (hipStream_t)stream);
    if (rc) return rc;
    return h->t.update(omd, (hipStream_t)stream);
}

extern "C" int showo_ema_table_swap(showo_ema_table* h, void* stream) {
    if (!h) return set_error_msg(1, "ema_table_swap: null handle");
    return h->t.swap((hipStream_t)stream);
}
