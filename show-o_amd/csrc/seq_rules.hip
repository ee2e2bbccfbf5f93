// Sequence rules in front of the token pick of the mmu decode (include/showo_hip.h, "Sequence rules"; DESIGN.md has the section).
//
// Per row: a history h[0, len) of token ids in device memory (the request's context ids, then every token the call fed), and three
// rules that ban a token w for this pick -- its entry of the fp32 row becomes -inf, every other entry keeps its bits:
//   n-gram       n >= 1: some j in [0, len - n] has h[j .. j+n-2] == h[len-n+1 .. len-1] and w == h[j+n-1]
//   bad word     a sequence s of the row's table, m = |s| >= 2 <= len + 1: h[len-m+1 .. len-1] == s[0 .. m-2] and w == s[m-1]
//   min length   w == eot and len - ctx_len < min_new
// One block per row, 256 threads, no state across blocks.  Every thread reads the row's length, the tail's n - 1 tokens go to LDS,
// the threads stride over the start positions j and over the table's sequences, thread 0 does the minimum-length rule.  `mark` is
// the newest member of the history: position len0 reads it from the register, never from memory, so the append -- thread 0, behind
// the barrier that follows every read of hist_len -- can land whenever it likes.  Several threads may store -inf to one entry (the
// same bits).  Ids are compared as plain integers; a ban of an id outside [0, V) stores nothing.
// Everything that changes from step to step (length, history, mark, activity) is read from device memory: one captured launch
// serves every replay of a decode step.
#include "seq_rules.h"
#include <string>

using namespace showo;

namespace {

constexpr int SEQ_THREADS = 256;
constexpr int SEQ_MAXROWS = 32;  // rows per launch (the per-row operands travel as kernel arguments)

struct SeqRows {
    const int32_t* bad[SEQ_MAXROWS];
    int32_t ngram[SEQ_MAXROWS];
    int32_t ctx_len[SEQ_MAXROWS];
    int32_t min_new[SEQ_MAXROWS];
};

__global__ __launch_bounds__(SEQ_THREADS) void seq_ban_kernel(float* __restrict__ rows, int64_t ld, int V, int32_t* hist, int64_t hist_ld,
                                                              int32_t* hist_len, const int64_t* __restrict__ mark,
                                                              const int* __restrict__ active, int active_stride, int64_t eot, SeqRows p) {
    __shared__ int tail[SEQ_NGRAM_MAX];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (active && active[(int64_t)r * active_stride] == 0) return;  // block-uniform: an inactive row is neither appended to nor written
    float* y = rows + (int64_t)r * ld;
    int32_t* h = hist + (int64_t)r * hist_ld;
    int len0 = hist_len[r];
    if (len0 < 0) len0 = 0;
    if (len0 > hist_ld) len0 = (int)hist_ld;
    const int64_t m64 = mark ? mark[r] : -1;
    const int mk = (m64 >= 0 && m64 < V) ? (int)m64 : -1;  // outside [0, V): none
    const int len = len0 + (mk >= 0 ? 1 : 0);              // (a full row still SEES its mark: len0 + 1 may exceed hist_ld)
    auto at = [&](int i) { return i < len0 ? h[i] : mk; };  // i < len
    const float ninf = __int_as_float((int)0xFF800000u);
    const int n = p.ngram[r];
    if (n >= 1 && len >= n && tid < n - 1) tail[tid] = at(len - n + 1 + tid);
    __syncthreads();  // every read of hist_len lies in front of this barrier, the append behind it
    if (tid == 0) {
        if (mk >= 0 && len0 < hist_ld) {
            h[len0] = mk;
            hist_len[r] = len0 + 1;
        }
        if (eot >= 0 && eot < V && len - p.ctx_len[r] < p.min_new[r]) y[eot] = ninf;
    }
    if (n >= 1 && len >= n) {
        for (int j = tid; j <= len - n; j += SEQ_THREADS) {
            bool eq = true;
            for (int k = 0; k < n - 1 && eq; ++k) eq = at(j + k) == tail[k];
            if (!eq) continue;
            const int w = at(j + n - 1);
            if (w >= 0 && w < V) y[w] = ninf;
        }
    }
    const int32_t* t = p.bad[r];
    if (t) {
        const int S = t[0];
        const int32_t* off = t + 1;
        const int32_t* tk = t + 2 + S;
        for (int i = tid; i < S; i += SEQ_THREADS) {
            const int a = off[i], m = off[i + 1] - a;
            if (m < 2 || len < m - 1) continue;
            bool eq = true;
            for (int k = 0; k < m - 1 && eq; ++k) eq = at(len - m + 1 + k) == tk[a + k];
            if (!eq) continue;
            const int w = tk[a + m - 1];
            if (w >= 0 && w < V) y[w] = ninf;
        }
    }
}

}  // namespace

namespace showo {

int seq_rules_check(int nrows, const showo_seq_rules* q, const char* who) {
    auto fail = [&](const char* msg) { return set_error_msg(1, (std::string(who) + ": " + msg).c_str()); };
    if (nrows < 1 || !q || !q->hist || !q->hist_len || !q->ngram || !q->ctx_len || !q->min_new)
        return fail("the rules need rows, a history, its lengths and ngram / ctx_len / min_new per row");
    if (q->hist_ld < 1 || q->hist_ld > 0x7fffffff) return fail("hist_ld must be in [1, 2^31)");
    if (((uintptr_t)q->hist | (uintptr_t)q->hist_len) & 3) return fail("the history must be 4-byte aligned");
    for (int r = 0; r < nrows; ++r) {
        if (q->ngram[r] < 0 || q->ngram[r] > SEQ_NGRAM_MAX) return fail("no_repeat_ngram_size must be in [0, 16] (0: off)");
        if (q->ctx_len[r] < 0 || q->min_new[r] < 0) return fail("ctx_len and min_new must be >= 0");
        if (q->bad && ((uintptr_t)q->bad[r] & 3)) return fail("bad-word tables must be 4-byte aligned");
    }
    return 0;
}

int seq_ban_launch(float* rows, int64_t ld, int nrows, int V, const showo_seq_rules* q, const int64_t* mark, const int* active,
                   int active_stride, hipStream_t s) {
    if (nrows == 0) return 0;
    if (!rows || nrows < 0) return set_error_msg(1, "seq_ban: bad arguments");
    if (V < 1 || ld < V) return set_error_msg(1, "seq_ban: needs V >= 1 and ld >= V");
    if ((uintptr_t)rows & 3) return set_error_msg(1, "seq_ban: rows must be 4-byte aligned");
    if (const int rc = seq_rules_check(nrows, q, "seq_ban")) return rc;
    for (int r0 = 0; r0 < nrows; r0 += SEQ_MAXROWS) {
        const int n = nrows - r0 < SEQ_MAXROWS ? nrows - r0 : SEQ_MAXROWS;
        SeqRows p;
        for (int r = 0; r < SEQ_MAXROWS; ++r) {
            p.bad[r] = (q->bad && r < n) ? q->bad[r0 + r] : nullptr;
            p.ngram[r] = r < n ? q->ngram[r0 + r] : 0;
            p.ctx_len[r] = r < n ? q->ctx_len[r0 + r] : 0;
            p.min_new[r] = r < n ? q->min_new[r0 + r] : 0;
        }
        seq_ban_kernel<<<dim3(n), dim3(SEQ_THREADS), 0, s>>>(rows + (int64_t)r0 * ld, ld, V, q->hist + (int64_t)r0 * q->hist_ld, q->hist_ld,
                                                             q->hist_len + r0, mark ? mark + r0 : nullptr,
                                                             active ? active + (int64_t)r0 * active_stride : nullptr, active_stride, q->eot, p);
        SHOWO_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace showo

extern "C" int showo_seq_ban(float* rows, int64_t ld, int nrows, int V, const showo_seq_rules* rules, const int64_t* mark,
                             const int32_t* active, void* stream) {
    return showo::seq_ban_launch(rows, ld, nrows, V, rules, mark, active, 1, (hipStream_t)stream);
}
