// Logit adjustment in front of the token pick of the mmu decode (include/showo_hip.h, "Logit adjustment"; DESIGN.md has the section).
//
// For one fp32 logits row x[0, V), a token set S (a bitmap: token i is bit i & 31 of word i >> 5), a penalty theta > 0 and an optional
// fp32 bias row beta[0, V):
//   r_i = x_i                                   i not in S
//   r_i = x_i * theta  if x_i < 0,  else  x_i / theta      i in S   (fp32 multiply; IEEE division, __fdiv_rn)
//   y_i = r_i + beta_i                          (no bias row: y_i = r_i)
// Hugging Face's RepetitionPenaltyLogitsProcessor followed by a sequence bias.  -0.0 and 0.0 are "not < 0", -inf stays -inf, a bias
// of -inf bans its token.  y goes to a SECOND row: the raw row stays what the head wrote, for the log-probabilities.
//
// One launch serves all rows: grid (chunks of 4096 logits, rows), 256 threads.  A block first puts the 128 bitmap words of its chunk
// (and the one behind them) into LDS, one word per thread -- a word serves 32 consecutive logits and is read from memory once, not
// once per element -- then walks the chunk with 16-byte loads and stores behind a peel to the row's alignment (rows of a [n, 58498]
// block alternate between 8- and 16-byte alignment), consecutive lanes on consecutive quads.  A bias row or an output row that is
// aligned differently from the logits row is read / written element by element.
// `mark` names one more member per row (the token the decode step just fed): the thread that owns its bitmap word ORs the bit into
// memory atomically, and EVERY thread that loads that word ORs the bit into its own copy as well, so the output does not depend on
// when the atomic lands.
// The work is elementwise -- y_i depends on x_i, beta_i, theta and the membership of i alone, never on which lane or block meets the
// element -- so the same row gives the same bits wherever it lies, at every alignment, row count and from every caller (stand-alone,
// batch-1 loop, batched slot).  The multiply, the division and the add are three separately rounded fp32 operations (never an fma).
#include "logit_adjust.h"
#include "../../include/showo_hip.h"
#include <cmath>
#include <string>

using namespace showo;

namespace {

constexpr int ADJ_THREADS = 256;
constexpr int ADJ_QUADS = 4;                             // 16-byte quads per thread
constexpr int ADJ_CHUNK = ADJ_THREADS * 4 * ADJ_QUADS;   // logits per block
constexpr int ADJ_WORDS = ADJ_CHUNK / 32;                // bitmap words per block
constexpr int ADJ_MAXROWS = 32;                          // rows per launch (the per-row operands travel as kernel arguments)
static_assert(ADJ_WORDS < ADJ_THREADS, "one bitmap word per thread, and one more");

struct AdjRows {
    const float* bias[ADJ_MAXROWS];
    float penalty[ADJ_MAXROWS];
};

__device__ __forceinline__ float adjust_one(float v, bool in_set, float theta, bool has_bias, float b) {
    float r = v;
    if (in_set) {
        if (v < 0.f) r = __fmul_rn(v, theta);
        else r = __fdiv_rn(v, theta);
    }
    if (has_bias) r = __fadd_rn(r, b);
    return r;
}

__global__ __launch_bounds__(ADJ_THREADS) void logits_adjust_kernel(const float* __restrict__ logits, int64_t ld, int V, uint32_t* seen,
                                                                    int64_t seen_ld, const int64_t* __restrict__ mark,
                                                                    const int* __restrict__ active, int active_stride, float* __restrict__ out,
                                                                    int64_t ld_out, AdjRows rows) {
    __shared__ uint32_t sw[ADJ_WORDS + 1];
    const int r = blockIdx.y, tid = threadIdx.x;
    if (active && active[(int64_t)r * active_stride] == 0) return;  // block-uniform: an inactive row is neither marked nor written
    const float* __restrict__ x = logits + (int64_t)r * ld;
    float* __restrict__ y = out + (int64_t)r * ld_out;
    const float* __restrict__ beta = rows.bias[r];
    const float theta = rows.penalty[r];
    uint32_t* sr = seen + (int64_t)r * seen_ld;
    const int nwords = (V + 31) >> 5;
    const int64_t m64 = mark ? mark[r] : -1;
    const int mk = (m64 >= 0 && m64 < V) ? (int)m64 : -1;  // outside [0, V): none
    const int W0 = blockIdx.x * ADJ_WORDS;
    if (tid <= ADJ_WORDS) {  // words W0 .. W0 + ADJ_WORDS: the last one belongs to the next block, a quad may reach into it
        const int w = W0 + tid;
        uint32_t v = w < nwords ? sr[w] : 0u;
        if (mk >= 0 && (mk >> 5) == w) {
            const uint32_t bit = 1u << (mk & 31);
            if (tid < ADJ_WORDS) atomicOr(&sr[w], bit);  // the word's one owner in the whole grid row
            v |= bit;
        }
        sw[tid] = v;
    }
    __syncthreads();
    int head = (int)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) >> 2);
    if (head > V) head = V;
    const int n4 = (V - head) >> 2, tail0 = head + 4 * n4;
    const bool has_b = beta != nullptr;
    const bool y16 = ((((uintptr_t)y) ^ ((uintptr_t)x)) & 15u) == 0;
    const bool b16 = has_b && ((((uintptr_t)beta) ^ ((uintptr_t)x)) & 15u) == 0;
    auto in_set = [&](int i) { return ((sw[(i >> 5) - W0] >> (i & 31)) & 1u) != 0; };
    const int B0 = blockIdx.x * ADJ_CHUNK;
    // the elements in front of the row's first 16-byte boundary (block 0) and behind its last whole quad (the block that quad ends in)
    if (blockIdx.x == 0 && tid < head) y[tid] = adjust_one(x[tid], in_set(tid), theta, has_b, has_b ? beta[tid] : 0.f);
    if (tail0 / ADJ_CHUNK == (int)blockIdx.x && tid < V - tail0) {
        const int i = tail0 + tid;
        y[i] = adjust_one(x[i], in_set(i), theta, has_b, has_b ? beta[i] : 0.f);
    }
    // quads that START in [B0, B0 + ADJ_CHUNK): i0 = head (mod 4), so the last one may end up to 3 elements into the next chunk
    float4 xv[ADJ_QUADS], bq[ADJ_QUADS];
#pragma unroll
    for (int j = 0; j < ADJ_QUADS; ++j) {
        const int i0 = B0 + head + 4 * (tid + ADJ_THREADS * j);
        bq[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i0 < tail0) {
            xv[j] = *reinterpret_cast<const float4*>(x + i0);
            if (b16) bq[j] = *reinterpret_cast<const float4*>(beta + i0);
            else if (has_b) bq[j] = make_float4(beta[i0], beta[i0 + 1], beta[i0 + 2], beta[i0 + 3]);
        }
    }
#pragma unroll
    for (int j = 0; j < ADJ_QUADS; ++j) {
        const int i0 = B0 + head + 4 * (tid + ADJ_THREADS * j);
        if (i0 < tail0) {
            float4 o;
            o.x = adjust_one(xv[j].x, in_set(i0), theta, has_b, bq[j].x);
            o.y = adjust_one(xv[j].y, in_set(i0 + 1), theta, has_b, bq[j].y);
            o.z = adjust_one(xv[j].z, in_set(i0 + 2), theta, has_b, bq[j].z);
            o.w = adjust_one(xv[j].w, in_set(i0 + 3), theta, has_b, bq[j].w);
            if (y16) *reinterpret_cast<float4*>(y + i0) = o;
            else { y[i0] = o.x; y[i0 + 1] = o.y; y[i0 + 2] = o.z; y[i0 + 3] = o.w; }
        }
    }
}

__global__ void seen_mark_kernel(uint32_t* row, int V, const int64_t* __restrict__ ids, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int64_t id = ids[t];
    if (id < 0 || id >= V) return;  // (the -1 of an idle slot's output row)
    atomicOr(&row[id >> 5], 1u << (id & 31));
}

}  // namespace

namespace showo {

int logits_adjust_check(int nrows, int V, const uint32_t* seen, int64_t seen_ld, const float* penalty, const char* who) {
    auto fail = [&](const char* msg) { return set_error_msg(1, (std::string(who) + ": " + msg).c_str()); };
    if (nrows < 1 || V < 1 || !seen || !penalty) return fail("the adjustment needs rows, a bitmap and a penalty per row");
    if (seen_ld < (int64_t)((V + 31) / 32)) return fail("seen_ld must cover the vocabulary (>= ceil(V / 32) words)");
    if ((uintptr_t)seen & 3) return fail("the bitmap must be 4-byte aligned");
    for (int r = 0; r < nrows; ++r)
        if (!std::isfinite(penalty[r]) || !(penalty[r] > 0.f)) return fail("a penalty must be finite and > 0");
    return 0;
}

int logits_adjust_launch(const float* logits, int64_t ld, int nrows, int V, uint32_t* seen, int64_t seen_ld, const int64_t* mark,
                         const float* penalty, const float* const* bias, const int* active, int active_stride, float* out, int64_t ld_out,
                         hipStream_t s) {
    if (nrows == 0) return 0;
    if (!logits || !out || nrows < 0) return set_error_msg(1, "logits_adjust: bad arguments");
    if (V < 1 || ld < V || ld_out < V) return set_error_msg(1, "logits_adjust: needs V >= 1, ld >= V and ld_out >= V");
    if (((uintptr_t)logits | (uintptr_t)out) & 3) return set_error_msg(1, "logits_adjust: rows must be 4-byte aligned");
    if (const int rc = logits_adjust_check(nrows, V, seen, seen_ld, penalty, "logits_adjust")) return rc;
    {   // the adjusted rows are written while other blocks still read raw ones, and the raw rows must survive for the log-probabilities
        const float *l0 = logits, *l1 = logits + (int64_t)(nrows - 1) * ld + V, *o0 = out, *o1 = out + (int64_t)(nrows - 1) * ld_out + V;
        if (o0 < l1 && l0 < o1) return set_error_msg(1, "logits_adjust: out must not alias logits");
    }
    if (bias)
        for (int r = 0; r < nrows; ++r)
            if ((uintptr_t)bias[r] & 3) return set_error_msg(1, "logits_adjust: bias rows must be 4-byte aligned");
    for (int r0 = 0; r0 < nrows; r0 += ADJ_MAXROWS) {
        const int n = nrows - r0 < ADJ_MAXROWS ? nrows - r0 : ADJ_MAXROWS;
        AdjRows rows;
        for (int r = 0; r < ADJ_MAXROWS; ++r) {
            rows.bias[r] = (bias && r < n) ? bias[r0 + r] : nullptr;
            rows.penalty[r] = r < n ? penalty[r0 + r] : 1.f;
        }
        logits_adjust_kernel<<<dim3((V + ADJ_CHUNK - 1) / ADJ_CHUNK, n), dim3(ADJ_THREADS), 0, s>>>(
            logits + (int64_t)r0 * ld, ld, V, seen + (int64_t)r0 * seen_ld, seen_ld, mark ? mark + r0 : nullptr,
            active ? active + (int64_t)r0 * active_stride : nullptr, active_stride, out + (int64_t)r0 * ld_out, ld_out, rows);
        SHOWO_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace showo

extern "C" int showo_logits_adjust(const float* logits, int64_t ld, int nrows, int V, uint32_t* seen, int64_t seen_ld, const int64_t* mark,
                                   const float* penalty, const float* const* bias, const int32_t* active, float* out, int64_t ld_out,
                                   void* stream) {
    return showo::logits_adjust_launch(logits, ld, nrows, V, seen, seen_ld, mark, penalty, bias, active, 1, out, ld_out, (hipStream_t)stream);
}

extern "C" int showo_seen_mark(uint32_t* seen_row, int V, const int64_t* ids, int n, void* stream) {
    if (n == 0) return 0;
    if (!seen_row || !ids || n < 0 || V < 1) return set_error_msg(1, "seen_mark: bad arguments");
    if ((uintptr_t)seen_row & 3) return set_error_msg(1, "seen_mark: the bitmap must be 4-byte aligned");
    seen_mark_kernel<<<dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(seen_row, V, ids, n);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}
