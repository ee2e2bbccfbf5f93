// mmu sessions ("mmu sessions"): the device pieces that continuing and sharing a KV cache need beyond the layer stack.
//
//   showo_mask_append_rows  visibility intervals of Ln rows appended at position P: each is a decode row (last prefill row + causal)
//   showo_kv_fork           the prefix [0, P) of a per-layer K / V^T cache -> another cache with its own capacity (a batch slot)
//   showo_kv_copy_rows      the fork for a row range [r0, r1) -> rows [r0 - base, r1 - base) of a suffix cache (shared-prefix slots)
//
// The fork is a pure HBM stream (4 P 64 nL nH bytes each way: 119 MB at the cfg4 prefix of 607 rows), written like showo_copy_b128
// (basic.hip): 16-byte loads and stores, four independent loads in flight per thread before the first store.
#include "common.h"
#include "decode_common.h"
#include "../../include/showo_hip.h"

using namespace showo;

namespace {

__global__ __launch_bounds__(256) void mask_append_rows_kernel(int4 last, int L0, int P, int Ln, int32_t* __restrict__ iv) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Ln) return;
    const int32_t lv[4] = {last.x, last.y, last.z, last.w};
    int32_t o[4];
    next_iv(lv, L0, P + j, o);
    *reinterpret_cast<int4*>(iv + 4 * (int64_t)j) = make_int4(o[0], o[1], o[2], o[3]);
}

// K: per (layer, head) the rows [0, P) are one contiguous run of n16 = 8 P 16-byte chunks.  grid (chunk blocks, nL * nH).
__global__ __launch_bounds__(256) void kv_fork_k_kernel(const bf16_t* __restrict__ src, int64_t lstride_s, int cap_s, bf16_t* __restrict__ dst,
                                                        int64_t lstride_d, int cap_d, int nH, int n16) {
    const int l = blockIdx.y / nH, h = blockIdx.y - l * nH;
    const uint4* s = reinterpret_cast<const uint4*>(src + l * lstride_s + (int64_t)h * cap_s * 64);
    uint4* d = reinterpret_cast<uint4*>(dst + l * lstride_d + (int64_t)h * cap_d * 64);
    const int stride = gridDim.x * 1024;
    for (int i = blockIdx.x * 1024 + threadIdx.x; i < n16; i += stride) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (i + u * 256 < n16) ? s[i + u * 256] : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * 256 < n16) d[i + u * 256] = v[u];
    }
}

// V^T: rows = nL * nH * 64 rows of cap elements; a wave owns one row and walks the chunks of its first 64 ceil(P / 64) columns:
// whole chunks below P are copied, the chunk that holds column P keeps its elements below P and gets zeros above (the source chunk is
// read whole: it ends inside the source row, whose pitch is a multiple of 64), chunks beyond are zero.  grid (ceil(rows / 4)).
__global__ __launch_bounds__(256) void kv_fork_vt_kernel(const bf16_t* __restrict__ src, int64_t lstride_s, int cap_s, bf16_t* __restrict__ dst,
                                                         int64_t lstride_d, int cap_d, int rows_per_layer, int rows, int P) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int l = r / rows_per_layer, rr = r - l * rows_per_layer;
    const uint4* s = reinterpret_cast<const uint4*>(src + l * lstride_s + (int64_t)rr * cap_s);
    uint4* d = reinterpret_cast<uint4*>(dst + l * lstride_d + (int64_t)rr * cap_d);
    const int nfull = P >> 3, rem = P & 7, nread = (P + 7) >> 3, nall = ((P + 63) >> 6) << 3;
    for (int c = lane; c < nall; c += 256) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (c + u * 64 < nread) ? s[c + u * 64] : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int cc = c + u * 64;
            if (cc >= nall) continue;
            if (cc == nfull && rem) {  // elements [rem, 8) of this chunk are columns >= P
                uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (2 * q >= rem) w[q] = 0;
                    else if (2 * q + 1 >= rem) w[q] &= 0xffffu;
                }
                v[u] = make_uint4(w[0], w[1], w[2], w[3]);
            }
            d[cc] = v[u];
        }
    }
}

// V^T columns [r0, r1) of every row -> columns [r0 - base, r1 - base) of the destination row (base a multiple of 64: source and
// destination chunks line up), zeros up to the end of the destination's last 64-column tile.  A wave owns one row and walks the chunks
// from the one that holds r0: a chunk that begins below r0 keeps its elements below r0 (2-byte stores of the others), every other chunk
// is one 16-byte store with the elements at or beyond r1 zeroed.  grid (ceil(rows / 4)).
__global__ __launch_bounds__(256) void kv_copy_vt_rows_kernel(const bf16_t* __restrict__ src, int64_t lstride_s, int cap_s, bf16_t* __restrict__ dst,
                                                              int64_t lstride_d, int cap_d, int rows_per_layer, int rows, int r0, int r1, int base) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int l = r / rows_per_layer, rr = r - l * rows_per_layer;
    const bf16_t* s = src + l * lstride_s + (int64_t)rr * cap_s;
    bf16_t* d = dst + l * lstride_d + (int64_t)rr * cap_d;
    const int cend = base + (((r1 - base) + 63) & ~63);  // end of the zeroed tail, as a source column
    for (int col = ((r0 >> 3) + lane) * 8; col < cend; col += 512) {
        const uint4 v = col < r1 ? *reinterpret_cast<const uint4*>(s + col) : make_uint4(0, 0, 0, 0);  // read whole: it ends inside the source row
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (col + 2 * q >= r1) w[q] = 0;
            else if (col + 2 * q + 1 >= r1) w[q] &= 0xffffu;
        }
        if (col >= r0) {
            *reinterpret_cast<uint4*>(d + (col - base)) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (col + j >= r0) d[col + j - base] = (bf16_t)(j & 1 ? w[j >> 1] >> 16 : w[j >> 1] & 0xffffu);
        }
    }
}

}  // namespace

extern "C" int showo_kv_copy_rows(const uint16_t* k_src, const uint16_t* vt_src, int cap_src, int64_t k_lstride_src, int64_t v_lstride_src,
                                  uint16_t* k_dst, uint16_t* vt_dst, int cap_dst, int64_t k_lstride_dst, int64_t v_lstride_dst, int nL, int nH,
                                  int r0, int r1, int base, void* stream) {
    if (!k_src || !vt_src || !k_dst || !vt_dst) return set_error_msg(1, "kv_copy_rows: null argument");
    if (nL < 1 || nH < 1 || (int64_t)nL * nH > 65535) return set_error_msg(1, "kv_copy_rows: 1 <= layers * heads <= 65535");
    if (cap_src < 64 || cap_dst < 64 || (cap_src % 64) || (cap_dst % 64)) return set_error_msg(1, "kv_copy_rows: capacities must be multiples of 64");
    if (base < 0 || (base % 64) || r0 < base || r1 <= r0) return set_error_msg(1, "kv_copy_rows: needs base % 64 == 0 and base <= r0 < r1");
    if (r1 > cap_src || r1 - base > cap_dst) return set_error_msg(5, "kv_copy_rows: the rows exceed a cache's capacity");
    if ((((uintptr_t)k_src | (uintptr_t)vt_src | (uintptr_t)k_dst | (uintptr_t)vt_dst) & 15) ||
        ((k_lstride_src | v_lstride_src | k_lstride_dst | v_lstride_dst) & 7))
        return set_error_msg(1, "kv_copy_rows: 16-byte alignment required");
    const int64_t per_layer = (int64_t)nH * 64;
    if (k_lstride_src < per_layer * cap_src || v_lstride_src < per_layer * cap_src || k_lstride_dst < per_layer * cap_dst ||
        v_lstride_dst < per_layer * cap_dst)
        return set_error_msg(1, "kv_copy_rows: a layer stride is shorter than a layer");
    hipStream_t s = (hipStream_t)stream;
    // K: rows [r0, r1) of a head are one contiguous run, as the fork's rows [0, P) are
    const int n16 = (r1 - r0) * 8;
    kv_fork_k_kernel<<<dim3((n16 + 1023) / 1024, nL * nH), dim3(256), 0, s>>>(k_src + (int64_t)r0 * 64, k_lstride_src, cap_src,
                                                                            k_dst + (int64_t)(r0 - base) * 64, k_lstride_dst, cap_dst, nH, n16);
    SHOWO_CHECK_HIP(hipGetLastError());
    const int64_t rows = (int64_t)nL * per_layer;
    kv_copy_vt_rows_kernel<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s>>>(vt_src, v_lstride_src, cap_src, vt_dst, v_lstride_dst, cap_dst,
                                                                               (int)per_layer, (int)rows, r0, r1, base);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int showo_mask_append_rows(const int32_t* last_iv, int L0, int P, int Ln, int32_t* iv, void* stream) {
    if (!last_iv || !iv) return set_error_msg(1, "mask_append_rows: null argument");
    if (Ln < 1 || L0 < 1 || P < L0) return set_error_msg(1, "mask_append_rows: needs Ln >= 1 and P >= L0 >= 1");
    if ((uintptr_t)iv & 15) return set_error_msg(1, "mask_append_rows: iv must be 16-byte aligned (one 16-byte store per row)");
    const int a = last_iv[0], b = last_iv[1], c = last_iv[2], d = last_iv[3];
    if (!((b == L0 && a < b) || (d == L0 && c < d) || !(c < d) || !(a < b)))
        return set_error_msg(6, "mask_append_rows: mask row needs more than two intervals");
    mask_append_rows_kernel<<<dim3((Ln + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(make_int4(a, b, c, d), L0, P, Ln, iv);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int showo_kv_fork(const uint16_t* k_src, const uint16_t* vt_src, int cap_src, int64_t k_lstride_src, int64_t v_lstride_src,
                             uint16_t* k_dst, uint16_t* vt_dst, int cap_dst, int64_t k_lstride_dst, int64_t v_lstride_dst, int nL, int nH,
                             int P, void* stream) {
    if (!k_src || !vt_src || !k_dst || !vt_dst) return set_error_msg(1, "kv_fork: null argument");
    if (nL < 1 || nH < 1 || (int64_t)nL * nH > 65535) return set_error_msg(1, "kv_fork: 1 <= layers * heads <= 65535");
    if (cap_src < 64 || cap_dst < 64 || (cap_src % 64) || (cap_dst % 64)) return set_error_msg(1, "kv_fork: capacities must be multiples of 64");
    if (P < 1 || P > cap_src || P > cap_dst) return set_error_msg(5, "kv_fork: the prefix exceeds a cache's capacity");
    if ((((uintptr_t)k_src | (uintptr_t)vt_src | (uintptr_t)k_dst | (uintptr_t)vt_dst) & 15) ||
        ((k_lstride_src | v_lstride_src | k_lstride_dst | v_lstride_dst) & 7))
        return set_error_msg(1, "kv_fork: 16-byte alignment required");
    const int64_t per_layer = (int64_t)nH * 64;
    if (k_lstride_src < per_layer * cap_src || v_lstride_src < per_layer * cap_src || k_lstride_dst < per_layer * cap_dst ||
        v_lstride_dst < per_layer * cap_dst)
        return set_error_msg(1, "kv_fork: a layer stride is shorter than a layer");
    hipStream_t s = (hipStream_t)stream;
    const int n16 = P * 8;
    kv_fork_k_kernel<<<dim3((n16 + 1023) / 1024, nL * nH), dim3(256), 0, s>>>(k_src, k_lstride_src, cap_src, k_dst, k_lstride_dst, cap_dst, nH, n16);
    SHOWO_CHECK_HIP(hipGetLastError());
    const int64_t rows = (int64_t)nL * per_layer;  // <= 65535 * 64
    kv_fork_vt_kernel<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s>>>(vt_src, v_lstride_src, cap_src, vt_dst, v_lstride_dst, cap_dst,
                                                                          (int)per_layer, (int)rows, P);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}
