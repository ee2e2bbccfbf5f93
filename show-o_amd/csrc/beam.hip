// Beam search on the device ("Beam search"): the token boundary of a beam step.
//
//   showo_beam_select       the 2B best continuations over nb logits rows: per row the log-softmax normaliser (logprob_row's code)
//                           and its 2B best (score, token), then a merge of the nb x 2B survivors by (score, beam, token)
//   beam seam               the bookkeeping of one step on the 2B candidates: live beams, finished hypotheses, the done flag, and
//                           the tokens / positions / mask rows / embedding rows of the next step
//   showo_kv_permute_rows   beam c takes the K rows / V^T columns [r0, r1) of beam parent[c], through a staging buffer
//
// Every launch reads what varies from step to step (cumulative scores, the parent map, r1, the step counter) from device memory, so one
// captured step serves a whole search.
#include "beam.h"
#include "sample_row.h"
#include "decode_common.h"
#include "../../include/showo_hip.h"

using namespace showo;

namespace {

// ---- selection ------------------------------------------------------------------------------------------------------------------------
// One block per row.  score_i = cum + ((x_i - mx) - logS) in exactly this fp32 order, logS = row_norm_logS(S) of logprob_row's integer
// sum: given (mx, logS) the scores are a pure function of the row's bits, and the 2B picks -- the maxima of the order (score
// descending, token ascending), found one by one as "the best element behind the previous pick" -- a pure function of the scores.
// Neither depends on which lane met which element, so neither depends on the row's alignment.  Different logits may round to one
// score, hence the order on the score, not on the logit.
// REG (V <= 65536, so at most 16 quads per thread behind row_for_each_1024's alignment peel): a thread computes the scores of ITS
// elements once and keeps them in registers -- 64 + the peel's two -- so a walk costs compares only, no loads.  Absent elements hold NaN, which no comparison takes.  !REG: larger rows are
// re-read per pass (they sit in L2: the lm_head just wrote them).
// A row with NaN or +inf, or of -inf alone, has no normaliser: logS = NaN, every candidate (NaN, -1).
constexpr int SELECT_REG_QUADS = 16;
template <bool REG>
__global__ __launch_bounds__(1024) void beam_row_topk_kernel(const float* __restrict__ logits, int64_t ld, int V, const float* __restrict__ cum,
                                                             int K, float* __restrict__ norm, float* __restrict__ ws) {
    __shared__ RowLogprobSmem sm;
    __shared__ float s_logS;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = logits + (int64_t)b * ld;
    const RowNorm n = row_norm_1024(row, V, sm, [](float v) { return (int)!(v < INFINITY); });  // counts NaN and +inf
    if (tid == 0) s_logS = (n.S && !n.count) ? row_norm_logS(n.S) : __builtin_nanf("");
    __syncthreads();
    const float mx = n.mx, logS = s_logS;
    float* out = ws + (int64_t)b * K * 2;
    if (tid == 0) { norm[2 * b] = mx; norm[2 * b + 1] = logS; }
    if (logS != logS) {  // block-uniform
        if (tid < K) { out[2 * tid] = __builtin_nanf(""); out[2 * tid + 1] = __int_as_float(-1); }
        return;
    }
    const float c = cum[b];
    auto score_of = [&](float v) { return c + ((v - mx) - logS); };
    // row_for_each_1024's split of the row: `head` elements in front of the first 16-byte boundary, n4 quads, the rest from tail0
    int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);
    if (head > V) head = V;
    const int n4 = (V - head) >> 2, tail0 = head + 4 * n4;
    float sc[REG ? SELECT_REG_QUADS : 1][4];
    float s_head = __builtin_nanf(""), s_tail = __builtin_nanf("");
    if constexpr (REG) {
        const float4* __restrict__ q = reinterpret_cast<const float4*>(row + head);
#pragma unroll
        for (int u = 0; u < SELECT_REG_QUADS; ++u) {
            const int i4 = tid + u * 1024;
            if (i4 < n4) {
                const float4 v = q[i4];
                sc[u][0] = score_of(v.x); sc[u][1] = score_of(v.y); sc[u][2] = score_of(v.z); sc[u][3] = score_of(v.w);
            } else {
                sc[u][0] = sc[u][1] = sc[u][2] = sc[u][3] = __builtin_nanf("");
            }
        }
        if (tid < head) s_head = score_of(row[tid]);
        if (tid < V - tail0) s_tail = score_of(row[tail0 + tid]);
    }
    // A pick costs one block reduction, not one walk: every thread keeps the best of ITS elements that lies behind the previous pick.
    // The picks are the head of a total order, so after j picks the elements not yet taken are exactly those behind pick j, and a
    // thread's best changes only when the pick was its own: only that thread walks its elements again (the compares of a whole-row
    // walk fill one CU for 11 us; measured).
    float ps = INFINITY;  // the previous pick: everything lies behind (+inf, -1)
    int pt = -1;
    float mine = -INFINITY;
    int mine_t = 0x7fffffff;
    auto take = [&](float s, int i) {
        const bool behind = s < ps || (s == ps && i > pt);
        if (behind && (s > mine || (s == mine && i < mine_t))) { mine = s; mine_t = i; }
    };
    auto walk = [&]() {  // the thread's own elements, in row_for_each_1024's assignment
        mine = -INFINITY;
        mine_t = 0x7fffffff;
        if constexpr (REG) {
            take(s_head, tid);
#pragma unroll
            for (int u = 0; u < SELECT_REG_QUADS; ++u) {
                const int at = head + 4 * (tid + u * 1024);
#pragma unroll
                for (int e = 0; e < 4; ++e) take(sc[u][e], at + e);
            }
            take(s_tail, tail0 + tid);
        } else {
            row_for_each_idx_1024(row, V, [&](float v, int i) { take(score_of(v), i); });
        }
    };
    walk();
    for (int j = 0; j < K; ++j) {
        float best = mine;
        int bt = mine_t;
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bt, o, 64);
            if (ob > best || (ob == best && oi < bt)) { best = ob; bt = oi; }
        }
        if (lane == 0) { sm.red_f[wave] = best; sm.red_i[wave] = bt; }
        __syncthreads();
        best = sm.red_f[0];
        bt = sm.red_i[0];
        for (int w = 1; w < 16; ++w)
            if (sm.red_f[w] > best || (sm.red_f[w] == best && sm.red_i[w] < bt)) { best = sm.red_f[w]; bt = sm.red_i[w]; }
        __syncthreads();  // the next pick writes red_f / red_i again
        if (bt == 0x7fffffff) { best = __builtin_nanf(""); bt = -1; }  // (nothing left to take: scores that compare with nothing, a NaN cum)
        if (tid == 0) { out[2 * j] = best; out[2 * j + 1] = __int_as_float(bt); }
        ps = best;
        pt = bt;
        if (mine_t == pt && j + 1 < K) walk();  // the owner of the pick (token ids are unique; -1 owns nothing)
    }
}

// The 2B best of the nb x K row survivors (K = 2B) by (score descending, beam ascending, token ascending); the (NaN, -1) candidates of a
// row without a normaliser come behind every other one, so such a row costs the others nothing.  n <= 128 entries: every thread counts
// the entries in front of its own.
__global__ __launch_bounds__(128) void beam_merge_kernel(const float* __restrict__ ws, int nb, int K, BeamCand* __restrict__ cand) {
    __shared__ float s_s[128];
    __shared__ int s_t[128];
    const int tid = threadIdx.x, n = nb * K;
    if (tid < n) { s_s[tid] = ws[2 * tid]; s_t[tid] = __float_as_int(ws[2 * tid + 1]); }
    __syncthreads();
    if (tid >= n) return;
    const float s = s_s[tid];
    const int t = s_t[tid], b = tid / K;
    const bool nan = s != s;
    int rank = 0;
    for (int f = 0; f < n; ++f) {
        const float fs = s_s[f];
        const int ft = s_t[f], fb = f / K;
        bool front;
        if (fs != fs) front = nan && f < tid;
        else if (nan) front = true;
        else front = fs > s || (fs == s && (fb < b || (fb == b && ft < t)));
        rank += front;
    }
    if (rank < K) cand[rank] = BeamCand{s, b, t};
}

// ---- the seam -------------------------------------------------------------------------------------------------------------------------
// One block.  Thread 0 walks the 2B candidates (the rule of DESIGN.md, "Beam search"), all threads then write the B embedding rows.
// Once the state's done flag is set (or max_new tokens are out) a step is idle: zero rows, positions and every table as they are.
__global__ __launch_bounds__(1024) void beam_seam_kernel(BeamSeamArgs a) {
    __shared__ int s_tok[BEAM_MAX];
    __shared__ int s_go;
    const int tid = threadIdx.x, B = a.B;
    int32_t* st = a.state;
    if (tid == 0) {
        const int t = st[BS_T], max_new = st[BS_MAXNEW];
        int go = 0;
        if (!st[BS_DONE] && t < max_new) {
            const int len = t + 1;
            const float div = __int_as_float(st[BEAM_STATE_HEAD + len]);
            int n_hyp = st[BS_NHYP], order = st[BS_ORDER];
            BeamHyp* hyp = a.hyp;
            auto insert = [&](int step, int beam, int kind, float sumlp, float lp) {  // keep the B best; a new one beats the worst only strictly
                const float fin = __fdiv_rn(sumlp, div);
                const int ord = order++;
                if (n_hyp == B) {
                    if (!(fin > hyp[B - 1].final)) return;
                    n_hyp = B - 1;
                }
                int i = n_hyp;
                for (; i > 0 && hyp[i - 1].final < fin; --i) hyp[i] = hyp[i - 1];
                hyp[i] = BeamHyp{step, beam, kind, fin, len, sumlp, ord, lp};
                ++n_hyp;
            };
            auto lp_of = [&](int p, int id) {  // logprob_row's expression on the candidate's row
                return id >= 0 && id < a.V ? (a.logits[(int64_t)p * a.ld + id] - a.norm[2 * p]) - a.norm[2 * p + 1] : __builtin_nanf("");
            };
            float ncum[BEAM_MAX], nlp[BEAM_MAX];
            int npar[BEAM_MAX], ntok[BEAM_MAX];
            int nlive = 0;
            for (int r = 0; r < 2 * B; ++r) {
                const BeamCand c = a.cand[r];
                if (a.eot >= 0 && (int64_t)c.token == a.eot) {
                    if (r < B) insert(t, c.beam, 0, c.score, lp_of(c.beam, c.token));
                } else if (nlive < B) {
                    npar[nlive] = c.beam; ntok[nlive] = c.token; ncum[nlive] = c.score;
                    ++nlive;
                }
            }
            for (int b = nlive; b < B; ++b) { npar[b] = b; ntok[b] = -1; ncum[b] = __builtin_nanf(""); }  // (cannot happen: 2B candidates, B <eot> at most)
            for (int b = 0; b < B; ++b) {
                const int p = npar[b], id = ntok[b];
                const float lp = nlp[b] = lp_of(p, id);
                const int64_t at = (int64_t)t * B + b;
                a.tr_parent[at] = p; a.tr_token[at] = id; a.tr_cum[at] = ncum[b]; a.tr_lp[at] = lp;
                st[BS_CUM + b] = __float_as_int(ncum[b]);
                reinterpret_cast<int64_t*>(st + BS_TOK)[b] = id;
                s_tok[b] = id;
            }
            float worst = n_hyp == B ? hyp[B - 1].final : -INFINITY;
            bool fin = n_hyp == B && (a.early || worst >= __fdiv_rn(ncum[0], div));
            if (!fin && len == max_new) {  // the live beams join the finished set
                for (int b = 0; b < B; ++b) insert(t, b, 1, ncum[b], nlp[b]);
                worst = n_hyp == B ? hyp[B - 1].final : -INFINITY;
                fin = true;
            }
            st[BS_T] = len; st[BS_NHYP] = n_hyp; st[BS_ORDER] = order; st[BS_WORST] = __float_as_int(worst); st[BS_DONE] = fin;
            go = !fin;
            for (int b = 0; b < B; ++b) {
                st[BS_PARENT + b] = go ? npar[b] : b;
                const int P = a.pos[b];
                const int Pn = a.first ? P : (go ? P + 1 : min(P + 1, a.lim - 1));
                a.pos[b] = Pn;
                next_iv(a.last_iv + 4 * b, a.L0[b], Pn, a.iv + 4 * b);
            }
        } else {
            for (int b = 0; b < B; ++b) { st[BS_PARENT + b] = b; s_tok[b] = -1; }
        }
        s_go = go;
    }
    __syncthreads();
    const bool go = s_go != 0;
    for (int b = 0; b < B; ++b) slot_embed_row(s_tok[b], go, a.table, a.x + (int64_t)b * a.H, a.H, a.V, tid, 1024);
}

// ---- cache rows of the parents ---------------------------------------------------------------------------------------------------------
// Beam c takes K rows / V^T columns [r0, r1) of beam parent[c], for every (layer, head), through a staging buffer: the gather launch
// copies slot parent[c] -> stage[c], the scatter launch stage[c] -> slot c, for every c with parent[c] != c (an index outside [0, B)
// counts as c).  No slot is written before every slot has been read, so any map is served: swaps, cycles, one parent for all.
// Whole 16-byte chunks are copied: K rows are whole chunks; of V^T the chunks [r0 / 8, ceil(r1 / 8)) of every row, i.e. also the
// columns [8 floor(r0 / 8), r0) -- below r0, the common prompt, all beams hold identical bits (they are forks of one cache), so these
// keep their bits -- and [r1, 8 ceil(r1 / 8)) -- beyond the live length, which no decode step reads.  Nothing else is written.
// parent and r1 are read from device memory; r1 is clipped to r0 + span and to the capacity.  grid (PERMUTE_GX, layers x heads, B):
// sized for the capacity, blocks behind r1 leave at once.  A wave per V^T row, as in the fork (kv_session.hip).
constexpr int PERMUTE_GX = 4;
template <bool GATHER>
__global__ __launch_bounds__(256) void kv_permute_kernel(uint16_t* const* __restrict__ k_tab, uint16_t* const* __restrict__ vt_tab, int cap,
                                                         int64_t k_lstride, int64_t v_lstride, int nL, int nH, int B,
                                                         const int32_t* __restrict__ parent, int r0, const int32_t* __restrict__ r1p, int span,
                                                         uint16_t* __restrict__ stage_k, uint16_t* __restrict__ stage_vt, int64_t sp) {
    const int c = blockIdx.z, p = parent[c];
    if (p == c || p < 0 || p >= B) return;
    int r1 = *r1p;
    r1 = min(r1, min(r0 + span, cap));
    if (r1 <= r0) return;
    const int l = blockIdx.y / nH, h = blockIdx.y - l * nH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t lh = ((int64_t)c * nL + l) * nH + h;
    {
        uint4* slot = reinterpret_cast<uint4*>(k_tab[GATHER ? p : c] + l * k_lstride + ((int64_t)h * cap + r0) * 64);
        uint4* stg = reinterpret_cast<uint4*>(stage_k + lh * sp * 64);
        const int n16 = (r1 - r0) * 8;
        for (int i = blockIdx.x * 256 + tid; i < n16; i += PERMUTE_GX * 256) {
            if (GATHER) stg[i] = slot[i];
            else slot[i] = stg[i];
        }
    }
    const int c0 = r0 >> 3, c1 = (r1 + 7) >> 3;
    for (int rr = blockIdx.x * 4 + wave; rr < 64; rr += PERMUTE_GX * 4) {
        uint4* slot = reinterpret_cast<uint4*>(vt_tab[GATHER ? p : c] + l * v_lstride + ((int64_t)h * 64 + rr) * cap);
        uint4* stg = reinterpret_cast<uint4*>(stage_vt + (lh * 64 + rr) * sp);
        for (int cc = c0 + lane; cc < c1; cc += 64) {
            if (GATHER) stg[cc - c0] = slot[cc];
            else slot[cc] = stg[cc - c0];
        }
    }
}

}  // namespace

namespace showo {

int beam_select_launch(const float* logits, int64_t ld, int nb, int V, const float* cum, int B, float* norm, BeamCand* cand, float* ws,
                       hipStream_t s) {
    if (V <= SELECT_REG_QUADS * 4096)
        beam_row_topk_kernel<true><<<dim3(nb), dim3(1024), 0, s>>>(logits, ld, V, cum, 2 * B, norm, ws);
    else
        beam_row_topk_kernel<false><<<dim3(nb), dim3(1024), 0, s>>>(logits, ld, V, cum, 2 * B, norm, ws);
    beam_merge_kernel<<<dim3(1), dim3(128), 0, s>>>(ws, nb, 2 * B, cand);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

int beam_seam_launch(const BeamSeamArgs& a, hipStream_t s) {
    beam_seam_kernel<<<dim3(1), dim3(1024), 0, s>>>(a);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace showo

extern "C" int showo_beam_select(const float* logits, int64_t ld, int nb, int V, const float* cum, int B, float* norm, void* cand, float* ws,
                                 void* stream) {
    if (!logits || !cum || !norm || !cand || !ws) return set_error_msg(1, "beam_select: null argument");
    if (nb < 1 || nb > BEAM_MAX || B < 1 || B > BEAM_MAX) return set_error_msg(1, "beam_select: 1 <= nb <= 8 and 1 <= B <= 8");
    if (V < 2 * B || V >= (1 << 24) || ld < V) return set_error_msg(1, "beam_select: needs 2 B <= V < 2^24 and ld >= V");
    if (((uintptr_t)logits | (uintptr_t)cum | (uintptr_t)norm | (uintptr_t)cand | (uintptr_t)ws) & 3)
        return set_error_msg(1, "beam_select: 4-byte alignment required");
    return beam_select_launch(logits, ld, nb, V, cum, B, norm, reinterpret_cast<BeamCand*>(cand), ws, (hipStream_t)stream);
}

extern "C" int64_t showo_kv_permute_stage_elems(int nL, int nH, int B, int span) {
    if (nL < 1 || nH < 1 || B < 1 || span < 1) return 0;
    return (int64_t)B * nL * nH * 64 * kv_permute_pitch(span);
}

extern "C" int showo_kv_permute_rows(uint16_t* const* k_slots, uint16_t* const* vt_slots, int cap, int64_t k_lstride, int64_t v_lstride, int nL,
                                     int nH, int B, const int32_t* parent, int r0, const int32_t* r1, uint16_t* stage_k, uint16_t* stage_vt,
                                     int span, void* stream) {
    if (!k_slots || !vt_slots || !parent || !r1 || !stage_k || !stage_vt) return set_error_msg(1, "kv_permute_rows: null argument");
    if (nL < 1 || nH < 1 || (int64_t)nL * nH > 65535) return set_error_msg(1, "kv_permute_rows: 1 <= layers * heads <= 65535");
    if (B < 1 || B > BEAM_MAX) return set_error_msg(1, "kv_permute_rows: 1 <= B <= 8");
    if (cap < 64 || (cap % 64)) return set_error_msg(1, "kv_permute_rows: the capacity must be a multiple of 64");
    if (r0 < 0 || span < 1) return set_error_msg(1, "kv_permute_rows: needs r0 >= 0 and span >= 1");
    if (r0 >= cap) return set_error_msg(5, "kv_permute_rows: r0 exceeds the capacity");
    if ((((uintptr_t)stage_k | (uintptr_t)stage_vt) & 15) || ((k_lstride | v_lstride) & 7))
        return set_error_msg(1, "kv_permute_rows: 16-byte alignment required");
    if (k_lstride < (int64_t)nH * 64 * cap || v_lstride < (int64_t)nH * 64 * cap)
        return set_error_msg(1, "kv_permute_rows: a layer stride is shorter than a layer");
    hipStream_t s = (hipStream_t)stream;
    const int64_t sp = kv_permute_pitch(span);
    const dim3 grid(PERMUTE_GX, nL * nH, B);
    kv_permute_kernel<true><<<grid, dim3(256), 0, s>>>(k_slots, vt_slots, cap, k_lstride, v_lstride, nL, nH, B, parent, r0, r1, span, stage_k,
                                                      stage_vt, sp);
    kv_permute_kernel<false><<<grid, dim3(256), 0, s>>>(k_slots, vt_slots, cap, k_lstride, v_lstride, nL, nH, B, parent, r0, r1, span, stage_k,
                                                       stage_vt, sp);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}
