// HBM-bound VQGAN kernels for gfx950 (channel-last activations):
//   GroupNorm(32, eps=1e-6) statistics + normalise(+swish) -> bf16   (reference models/common_modules.py:16-24)
//   thin 1x1/3x3 fp32 convolution for the 13-channel latent convs     (reference models/modeling_magvitv2.py:131-139, 360-362)
//   channel pad + cast fp32 -> bf16 (feeds the MFMA implicit-GEMM conv in gemm.hip)
#include "common.h"
#include "../../include/showo_hip.h"
#include <type_traits>

using namespace showo;

namespace {

constexpr int GN_GROUPS = 32;
constexpr int GN_PIX_PER_BLOCK = 512;

// Deterministic GroupNorm statistics (no atomics: the same input gives the same bits on every run, which the
// sign-test quantizer downstream needs).  Pass 1: block (blk, b) reduces GN_PIX_PER_BLOCK pixels to 32 (sum, sumsq)
// pairs in double and writes them to part[b][blk][g][2].  Thread t owns channel quad f = t % (C/4) for all of its
// pixels, so its partial sums belong to exactly one group (C % 128 == 0  =>  channels-per-group % 4 == 0); every
// group is owned by exactly 8 threads of the block.  Pass 2 adds the per-block partials in block order.
__global__ __launch_bounds__(256) void gn_partial_kernel(const float* __restrict__ x, double* __restrict__ part, int HW, int C) {
    __shared__ double ssum[256], ssq[256];
    const int tid = threadIdx.x, b = blockIdx.y, nblk = gridDim.x;
    const int quads = C >> 2, ppp = 256 / quads;  // pixels per pass
    const int f = tid % quads, pl = tid / quads;
    const int p0 = blockIdx.x * GN_PIX_PER_BLOCK;
    const int pend = min(p0 + GN_PIX_PER_BLOCK, HW);
    const float* xb = x + (int64_t)b * HW * C;
    double s = 0.0, q = 0.0;
    for (int p = p0 + pl; p < pend; p += ppp) {
        float4 v = *reinterpret_cast<const float4*>(xb + (int64_t)p * C + f * 4);
        s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        q += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
    }
    // slot layout: group-major, 8 owners per group in (pixel-lane, quad-in-group) order
    const int qpg = quads / GN_GROUPS;  // quads per group
    const int g = f / qpg;
    const int slot = g * 8 + pl * qpg + (f - g * qpg);
    ssum[slot] = s;
    ssq[slot] = q;
    __syncthreads();
    if (tid < GN_GROUPS) {
        double a = 0.0, c = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) { a += ssum[tid * 8 + i]; c += ssq[tid * 8 + i]; }
        double* o = part + (((int64_t)b * nblk + blockIdx.x) * GN_GROUPS + tid) * 2;
        o[0] = a;
        o[1] = c;
    }
}
// stats[b][t] = sum_k part[b][k][t], t = g * 2 + which.  256 threads: four quarters of the k range (k = q, q + 4, ..) are summed in
// parallel and combined in a fixed order ((q0 + q1) + (q2 + q3)): same bits on every run.
__global__ __launch_bounds__(256) void gn_finalize_kernel(const double* __restrict__ part, double* __restrict__ stats, int nblk) {
    __shared__ double sq[4][GN_GROUPS * 2];
    const int b = blockIdx.x, t = threadIdx.x & 63, q = threadIdx.x >> 6;
    double a = 0.0;
    for (int k = q; k < nblk; k += 4) a += part[((int64_t)b * nblk + k) * (GN_GROUPS * 2) + t];
    sq[q][t] = a;
    __syncthreads();
    if (q == 0) stats[(int64_t)b * GN_GROUPS * 2 + t] = (sq[0][t] + sq[1][t]) + (sq[2][t] + sq[3][t]);
}

// part != nullptr: the statistics are still `nblk` per-block partials (part[b][k][g][2], nblk <= SHOWO_GN_FOLD_MAX) and every block sums
// them in its prologue, in gn_finalize_kernel's order -- four strided quarters, (q0 + q1) + (q2 + q3), in double -- so the mean / rstd
// have the bits of the gn_finalize_kernel + gn_apply_kernel pair without the separate launch.  ppb = pixels per block (a multiple of
// the block's pixels per pass): the host sizes the grid to the tensor with it; the kernel is elementwise given the statistics.
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, const double* __restrict__ stats,
                                                       const double* __restrict__ part, int nblk,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       bf16_t* __restrict__ y, bf16_t* __restrict__ ylo, int HW, int C, float eps,
                                                       int do_swish, int ppb) {
    __shared__ float smean[GN_GROUPS], srstd[GN_GROUPS];
    __shared__ double sq[4][GN_GROUPS * 2];
    const int tid = threadIdx.x, b = blockIdx.y;
    if (part) {
        const int t = tid & 63, q = tid >> 6;
        double a = 0.0;
        for (int k = q; k < nblk; k += 4) a += part[((int64_t)b * nblk + k) * (GN_GROUPS * 2) + t];
        sq[q][t] = a;
        __syncthreads();
    }
    if (tid < GN_GROUPS) {
        double s0, s1;
        if (part) {
            s0 = (sq[0][tid * 2] + sq[1][tid * 2]) + (sq[2][tid * 2] + sq[3][tid * 2]);
            s1 = (sq[0][tid * 2 + 1] + sq[1][tid * 2 + 1]) + (sq[2][tid * 2 + 1] + sq[3][tid * 2 + 1]);
        } else {
            s0 = stats[((int64_t)b * GN_GROUPS + tid) * 2];
            s1 = stats[((int64_t)b * GN_GROUPS + tid) * 2 + 1];
        }
        double n = (double)HW * (C / GN_GROUPS);
        double mean = s0 / n;
        double var = s1 / n - mean * mean;
        if (var < 0) var = 0;
        smean[tid] = (float)mean;
        srstd[tid] = (float)(1.0 / sqrt(var + (double)eps));
    }
    __syncthreads();
    const int quads = C >> 2, ppp = 256 / quads;
    const int f = tid % quads, pl = tid / quads;
    const int g = (f * 4) / (C / GN_GROUPS);
    const float mean = smean[g], rstd = srstd[g];
    const float4 ga = *reinterpret_cast<const float4*>(gamma + f * 4);
    const float4 be = *reinterpret_cast<const float4*>(beta + f * 4);
    const int p0 = blockIdx.x * ppb;
    const int pend = min(p0 + ppb, HW);
    const float* xb = x + (int64_t)b * HW * C;
    bf16_t* yb = y + (int64_t)b * HW * C;
    bf16_t* ylb = ylo ? ylo + (int64_t)b * HW * C : nullptr;
    for (int p = p0 + pl; p < pend; p += ppp) {
        float4 v = *reinterpret_cast<const float4*>(xb + (int64_t)p * C + f * 4);
        float o[4] = {(v.x - mean) * rstd * ga.x + be.x, (v.y - mean) * rstd * ga.y + be.y,
                      (v.z - mean) * rstd * ga.z + be.z, (v.w - mean) * rstd * ga.w + be.w};
        if (do_swish) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = o[j] * __builtin_amdgcn_rcpf(1.0f + __expf(-o[j]));
        }
        uint2 pk;
        pk.x = pack_bf2(o[0], o[1]);
        pk.y = pack_bf2(o[2], o[3]);
        *reinterpret_cast<uint2*>(yb + (int64_t)p * C + f * 4) = pk;
        if (ylb) {  // split precision: lo = bf16(x - float(hi))
            uint2 pl2;
            pl2.x = pack_bf2(o[0] - bf2f((bf16_t)(pk.x & 0xffff)), o[1] - bf2f((bf16_t)(pk.x >> 16)));
            pl2.y = pack_bf2(o[2] - bf2f((bf16_t)(pk.y & 0xffff)), o[3] - bf2f((bf16_t)(pk.y >> 16)));
            *reinterpret_cast<uint2*>(ylb + (int64_t)p * C + f * 4) = pl2;
        }
    }
}

// thin direct conv (fp32): one thread per output element; used only for the 13->13 1x1 latent convs
__global__ void conv_small_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                  float* __restrict__ out, int H, int W, int Cin, int Cout, int ks, int64_t total) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int co = (int)(i % Cout);
    int64_t p = i / Cout;
    int ox = (int)(p % W);
    int64_t t = p / W;
    int oy = (int)(t % H);
    int64_t b = t / H;
    int pad = (ks - 1) / 2;
    float acc = bias ? bias[co] : 0.f;
    for (int ky = 0; ky < ks; ++ky) {
        int iy = oy + ky - pad;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < ks; ++kx) {
            int ix = ox + kx - pad;
            if (ix < 0 || ix >= W) continue;
            const float* xp = x + ((b * H + iy) * W + ix) * (int64_t)Cin;
            const float* wp = w + ((int64_t)(co * ks + ky) * ks + kx) * Cin;
            for (int ci = 0; ci < Cin; ++ci) acc += xp[ci] * wp[ci];
        }
    }
    out[i] = acc;
}

// ---- thin-Cout 3x3 convolution on split operands (decoder.conv_out: 128 -> 3 channels at the full image resolution).  The MFMA conv
// computes a 128-wide n-tile for it -- the FLOPs of a 128 -> 128 conv for 3 useful columns; this kernel is bound by one pass over
// the (hi, lo) activation image instead.  A lane owns two channels (c = 128 j + 2 lane, j < NCH) and keeps ITS weights of all nine
// taps and CO outputs in registers; a wave walks one output row segment of up to THIN_SEG pixels along x with a 3 x 3 sliding window
// of input pixels, so every input pixel is loaded once per output row (4 bytes hi + 4 bytes lo per lane: 256 B per wave
// instruction).  Per output pixel: the lane's partial dot products (the three products of the split kernels as
// x_hi * (w_hi + w_lo) + x_lo * w_hi, fp32 FMAs), a 64-lane butterfly sum (every lane ends with the same sum, in the same order on
// every run), and lane (pixel - segment start) keeps the result for one coalesced fp32 NHWC store at the end of the segment.
constexpr int THIN_SEG = 64;
typedef float f32x2 __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ f32x2 bf2_widen(uint32_t u) {
    f32x2 r;
    r.x = __uint_as_float(u << 16);
    r.y = __uint_as_float(u & 0xffff0000u);
    return r;
}

static __device__ __forceinline__ void thin_fmac(float& acc, float a, float b) {  // acc = fma(a, b, acc)
    asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(a), "v"(b));
}

template <int CO, int NCH>
__global__ __launch_bounds__(256) void conv3_thin_split_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ xlo,
                                                               const bf16_t* __restrict__ w, const bf16_t* __restrict__ wlo,
                                                               const float* __restrict__ bias, float* __restrict__ out, int H, int W,
                                                               int Cin, int nseg, int64_t nwork) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wid >= nwork) return;  // (wave-uniform)
    const int seg = (int)(wid % nseg);
    const int64_t row = wid / nseg;  // b * H + y
    const int y = (int)(row % H);
    const int64_t img = row - y;     // b * H
    const int xs = seg * THIN_SEG, xe = min(xs + THIN_SEG, W);
    bool cok[NCH];
    f32x2 wf[NCH][3][3][CO], wh[NCH][3][3][CO];  // wf = w_hi + w_lo, wh = w_hi of this lane's channel pair
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c = j * 128 + 2 * lane;
        cok[j] = c < Cin;
#pragma unroll
        for (int co = 0; co < CO; ++co)
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int64_t o = (int64_t)(co * 9 + t) * Cin + c;
                const uint32_t uh = cok[j] ? *reinterpret_cast<const uint32_t*>(w + o) : 0u;
                const uint32_t ul = cok[j] ? *reinterpret_cast<const uint32_t*>(wlo + o) : 0u;
                wh[j][t / 3][t % 3][co] = bf2_widen(uh);
                wf[j][t / 3][t % 3][co] = bf2_widen(uh) + bf2_widen(ul);
            }
    }
    // raw (hi, lo) pairs of input column xi, rows y - 1 .. y + 1 (zero outside the image: the conv's padding)
    // Three columns are in flight (ring slot = the column's window slot), so a step does not wait for loads issued one step earlier.
    uint32_t rh[3][NCH][3], rl[3][NCH][3];
    auto load_col = [&](auto rc, int xi) {
        constexpr int R = decltype(rc)::value;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int yi = y + ky - 1;
            const bool ok = xi >= 0 && xi < W && yi >= 0 && yi < H;  // (wave-uniform)
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                rh[R][j][ky] = 0u;
                rl[R][j][ky] = 0u;
                if (ok && cok[j]) {
                    const int64_t o = ((img + yi) * W + xi) * Cin + j * 128 + 2 * lane;
                    rh[R][j][ky] = *reinterpret_cast<const uint32_t*>(x + o);
                    rl[R][j][ky] = *reinterpret_cast<const uint32_t*>(xlo + o);
                }
            }
        }
    };
    f32x2 xh[NCH][3][3], xl[NCH][3][3];  // [ky][window slot]: column xi lives in slot (xi - (xs - 1)) % 3
    float res[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) res[co] = 0.f;
    int xi = xs - 1;
    load_col(std::integral_constant<int, 0>(), xi);  // columns xs - 1 .. xe are needed; xe >= xs + 1
    load_col(std::integral_constant<int, 1>(), xi + 1);
    load_col(std::integral_constant<int, 2>(), xi + 2);
    // one column per step; R = its window slot (compile time, so the window and the ring are plain registers).  The loads of the
    // column three steps ahead are issued in front of this column's arithmetic.
    auto step = [&](auto rc) -> bool {
        constexpr int R = decltype(rc)::value;
        if (xi > xe) return false;
#pragma unroll
        for (int j = 0; j < NCH; ++j)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                xh[j][ky][R] = bf2_widen(rh[R][j][ky]);
                xl[j][ky][R] = bf2_widen(rl[R][j][ky]);
            }
        if (xi + 3 <= xe) load_col(rc, xi + 3);
        if (xi >= xs + 1) {  // columns xo - 1, xo, xo + 1 of output pixel xo = xi - 1 are in the window: kx -> slot (R + 1 + kx) % 3
            // scalar v_fmac_f32 chains, one per output channel.  Written as asm because the compiler's SLP pass packs any adjacent pair of
            // these into v_pk_fma_f32 (plus the v_mov_b32 to line the operands up), which issues at a fraction of the scalar rate on
            // this chip.  Register operands only, no memory access.  (profiles/vq_tail.txt: what was measured of this kernel.)
            float a[CO];
#pragma unroll
            for (int co = 0; co < CO; ++co) a[co] = 0.f;
#pragma unroll
            for (int j = 0; j < NCH; ++j)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const f32x2 h = xh[j][ky][(R + 1 + kx) % 3], l = xl[j][ky][(R + 1 + kx) % 3];
#pragma unroll
                        for (int co = 0; co < CO; ++co) {
                            thin_fmac(a[co], h.x, wf[j][ky][kx][co].x);
                            thin_fmac(a[co], h.y, wf[j][ky][kx][co].y);
                            thin_fmac(a[co], l.x, wh[j][ky][kx][co].x);
                            thin_fmac(a[co], l.y, wh[j][ky][kx][co].y);
                        }
                    }
#pragma unroll
            for (int co = 0; co < CO; ++co) {
                const float t = wave_sum_swap(a[co]);  // on the VALU: no ds_bpermute round trips (249 -> 228 us at 8 x 256 x 256 x 128)
                if (lane == xi - 1 - xs) res[co] = t;
            }
        }
        ++xi;
        return true;
    };
    for (;;) {
        if (!step(std::integral_constant<int, 0>())) break;
        if (!step(std::integral_constant<int, 1>())) break;
        if (!step(std::integral_constant<int, 2>())) break;
    }
    if (lane < xe - xs) {
        float* o = out + ((img + y) * W + xs + lane) * CO;
#pragma unroll
        for (int co = 0; co < CO; ++co) o[co] = res[co] + (bias ? bias[co] : 0.f);
    }
}

template <int CO>
int launch_conv3_thin(const bf16_t* x, const bf16_t* xlo, const bf16_t* w, const bf16_t* wlo, const float* bias, float* out, int B, int H,
                      int W, int Cin, hipStream_t s) {
    const int nseg = (W + THIN_SEG - 1) / THIN_SEG;
    const int64_t nwork = (int64_t)B * H * nseg;
    const dim3 grid((unsigned)((nwork + 3) / 4));
    if (Cin <= 128) conv3_thin_split_kernel<CO, 1><<<grid, dim3(256), 0, s>>>(x, xlo, w, wlo, bias, out, H, W, Cin, nseg, nwork);
    else conv3_thin_split_kernel<CO, 2><<<grid, dim3(256), 0, s>>>(x, xlo, w, wlo, bias, out, H, W, Cin, nseg, nwork);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

// fp32 [P, C] -> bf16 [P, Cpad] (zero padded channels)
__global__ void pad_cast_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, bf16_t* __restrict__ ylo, int C, int Cpad,
                                int64_t total) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int c = (int)(i % Cpad);
    int64_t p = i / Cpad;
    float v = (c < C) ? x[p * C + c] : 0.f;
    bf16_t h = f2bf(v);
    y[i] = h;
    if (ylo) ylo[i] = f2bf(v - bf2f(h));
}

__global__ void lfq_unpack_nhwc_kernel(const int64_t* __restrict__ ids, float* __restrict__ zq, int C, int64_t total) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    int64_t id = ids[t];
    float* zp = zq + t * C;
    for (int c = 0; c < C; ++c) zp[c] = ((id >> (C - 1 - c)) & 1) ? 1.0f : -1.0f;
}

}  // namespace

// [B, 32, 2] result + per-block partials: one per GN_PIX_PER_BLOCK pixels for showo_gn_stats, one per 256-pixel conv tile when the
// statistics come from the convolution epilogue (showo_conv3x3_bf16x3_gn) -- sized for the latter
extern "C" int showo_gn_stats_doubles(int B, int HW) {
    int nblk = (HW + 255) / 256;
    return B * GN_GROUPS * 2 * (1 + nblk);
}

// stats[b][g][2] = sum over k < nblk of part[b][k][g][2], in k order
extern "C" int showo_gn_finalize(const double* part, double* stats, int B, int nblk, void* stream) {
    if (B <= 0 || nblk <= 0) return 0;
    gn_finalize_kernel<<<dim3(B), dim3(256), 0, (hipStream_t)stream>>>(part, stats, nblk);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int showo_gn_stats(const float* x, double* stats, int B, int HW, int C, void* stream) {
    if (B <= 0 || HW <= 0) return 0;
    if ((C % 128) || C > 1024) return set_error_msg(1, "gn_stats: C must be a multiple of 128 and <= 1024");
    const int nblk = (HW + GN_PIX_PER_BLOCK - 1) / GN_PIX_PER_BLOCK;
    double* part = stats + (int64_t)B * GN_GROUPS * 2;  // per-block partials live behind the [B,32,2] result
    gn_partial_kernel<<<dim3(nblk, B), dim3(256), 0, (hipStream_t)stream>>>(x, part, HW, C);
    gn_finalize_kernel<<<dim3(B), dim3(256), 0, (hipStream_t)stream>>>(part, stats, nblk);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

// The partial pass alone when the image has at most SHOWO_GN_FOLD_MAX partials and the caller can take them (pending != nullptr):
// *pending = their count and showo_gn_apply_part sums them in its prologue; otherwise *pending = 0 and stats holds the result.
extern "C" int showo_gn_stats_lazy(const float* x, double* stats, int B, int HW, int C, int* pending, void* stream) {
    if (pending) *pending = 0;
    if (B <= 0 || HW <= 0) return 0;
    const int nblk = (HW + GN_PIX_PER_BLOCK - 1) / GN_PIX_PER_BLOCK;
    if (!pending || nblk > SHOWO_GN_FOLD_MAX) return showo_gn_stats(x, stats, B, HW, C, stream);
    if ((C % 128) || C > 1024) return set_error_msg(1, "gn_stats: C must be a multiple of 128 and <= 1024");
    gn_partial_kernel<<<dim3(nblk, B), dim3(256), 0, (hipStream_t)stream>>>(x, stats + (int64_t)B * GN_GROUPS * 2, HW, C);
    SHOWO_CHECK_HIP(hipGetLastError());
    *pending = nblk;
    return 0;
}

namespace {
int g_gn_fixed_grid = 0;

// Pixels per block of the apply pass: 512 on the large levels; on the small ones halved until B x blocks reaches about 1024, down to
// one pass of the block (256 / (C / 4) pixels).  A 16 x 16 x 512 tensor of 8 images ran on 8 blocks of 256 CUs with the fixed 512.
int gn_apply_ppb(int B, int HW, int C) {
    int ppb = GN_PIX_PER_BLOCK;
    if (g_gn_fixed_grid) return ppb;
    int ppp = 256 / (C >> 2);
    if (ppp < 1) ppp = 1;
    while (ppb / 2 >= ppp && (ppb / 2) % ppp == 0 && (int64_t)B * ((HW + ppb - 1) / ppb) < 1024) ppb /= 2;
    return ppb;
}

int gn_apply_launch(const float* x, const double* stats, const double* part, int nblk, const float* gamma, const float* beta,
                    uint16_t* y, uint16_t* ylo, int B, int HW, int C, float eps, int do_swish, void* stream) {
    if (B <= 0 || HW <= 0) return 0;
    if ((C % 128) || C > 1024) return set_error_msg(1, "gn_apply: C must be a multiple of 128 and <= 1024");
    const int ppb = gn_apply_ppb(B, HW, C);
    gn_apply_kernel<<<dim3((HW + ppb - 1) / ppb, B), dim3(256), 0, (hipStream_t)stream>>>(x, stats, part, nblk, gamma, beta, y, ylo, HW,
                                                                                         C, eps, do_swish, ppb);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}
}  // namespace

// 1: the apply pass keeps 512 pixels per block whatever the tensor (the grid before the sizing above; A/B and tests).  Same output bits.
extern "C" int showo_gn_set_fixed_grid(int on) {
    g_gn_fixed_grid = on ? 1 : 0;
    return 0;
}

extern "C" int showo_gn_apply(const float* x, const double* stats, const float* gamma, const float* beta, uint16_t* y,
                              uint16_t* ylo, int B, int HW, int C, float eps, int do_swish, void* stream) {
    return gn_apply_launch(x, stats, nullptr, 0, gamma, beta, y, ylo, B, HW, C, eps, do_swish, stream);
}

// showo_gn_apply from unsummed partials: part[b][k][32][2], k < nblk (what showo_gn_stats_lazy / showo_conv3x3_bf16x3_gn_lazy leave
// behind the [B, 32, 2] result).  The output has the bits of showo_gn_finalize(part, stats, B, nblk) + showo_gn_apply(stats).
extern "C" int showo_gn_apply_part(const float* x, const double* part, int nblk, const float* gamma, const float* beta, uint16_t* y,
                                   uint16_t* ylo, int B, int HW, int C, float eps, int do_swish, void* stream) {
    if (!part || nblk < 1 || nblk > SHOWO_GN_FOLD_MAX) return set_error_msg(1, "gn_apply_part: 1 <= nblk <= SHOWO_GN_FOLD_MAX partials required");
    return gn_apply_launch(x, nullptr, part, nblk, gamma, beta, y, ylo, B, HW, C, eps, do_swish, stream);
}

extern "C" int showo_conv_small_f32(const float* x, const float* w, const float* bias, float* out, int B, int H, int W,
                                    int Cin, int Cout, int ksize, void* stream) {
    int64_t total = (int64_t)B * H * W * Cout;
    if (total <= 0) return 0;
    if (ksize != 1 && ksize != 3) return set_error_msg(1, "conv_small: ksize must be 1 or 3");
    conv_small_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(x, w, bias, out, H, W, Cin,
                                                                                                  Cout, ksize, total);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

// Thin-Cout 3x3 convolution (stride 1, pad 1) on split operands: x / xlo bf16 NHWC [B, H, W, Cin], w / wlo bf16 [Cout][3][3][Cin],
// out fp32 NHWC [B, H, W, Cout] = conv + bias.  Cout <= 4, Cin % 32 == 0, Cin <= 256.
extern "C" int showo_conv3x3_thin_bf16x3(const uint16_t* x, const uint16_t* xlo, const uint16_t* w, const uint16_t* wlo, const float* bias,
                                         float* out, int B, int H, int W, int Cin, int Cout, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    if (Cout < 1 || Cout > 4) return set_error_msg(1, "conv3x3 thin: 1 <= Cout <= 4 required");
    if ((Cin % 32) || Cin <= 0 || Cin > 256) return set_error_msg(1, "conv3x3 thin: Cin must be a multiple of 32 and <= 256");
    if (!x || !xlo || !w || !wlo || !out) return set_error_msg(1, "conv3x3 thin: null operand (hi and lo images required)");
    if ((((uintptr_t)x) | ((uintptr_t)xlo) | ((uintptr_t)w) | ((uintptr_t)wlo) | ((uintptr_t)out)) & 3)
        return set_error_msg(1, "conv3x3 thin: operands must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    switch (Cout) {
        case 1: return launch_conv3_thin<1>(x, xlo, w, wlo, bias, out, B, H, W, Cin, s);
        case 2: return launch_conv3_thin<2>(x, xlo, w, wlo, bias, out, B, H, W, Cin, s);
        case 3: return launch_conv3_thin<3>(x, xlo, w, wlo, bias, out, B, H, W, Cin, s);
        default: return launch_conv3_thin<4>(x, xlo, w, wlo, bias, out, B, H, W, Cin, s);
    }
}

extern "C" int showo_pad_cast_bf16(const float* x, uint16_t* y, uint16_t* ylo, int64_t P, int C, int Cpad, void* stream) {
    int64_t total = P * Cpad;
    if (total <= 0) return 0;
    pad_cast_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(x, y, ylo, C, Cpad, total);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int showo_lfq_unpack_nhwc(const int64_t* ids, float* zq, int B, int C, int hw, void* stream) {
    int64_t total = (int64_t)B * hw;
    if (total <= 0) return 0;
    if (C < 1 || C > 62) return set_error_msg(1, "lfq: C must be in [1,62]");
    lfq_unpack_nhwc_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(ids, zq, C, total);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}
