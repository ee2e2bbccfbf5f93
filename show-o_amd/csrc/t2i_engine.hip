// Show-o text-to-image generation on the engine: Showo.t2i_generate (reference models/modeling_showo.py:104-181) as one entry point,
// showo_engine_t2i_generate, and its read-outs.  The layer stack and the head are engine.hip's (run_layers / head_rows), the sampler
// kernels sampler.hip's; this file owns the host side of a call -- the stages below, in the order a call runs them -- and the small
// kernels only t2i uses.  State that lives across calls is showo_engine::T2I (engine.h).
//   showo_engine_t2i_generate   checks, workspace, mask -> intervals, weight images; then up to two attempts
//     attempt(reuse)            queue_inputs -> wait_step0_plan -> prepare_prefix_cache -> the steps (eager, or run_graphed) -> deferred check
//       denoise_step            run_rows (one of three RowPass descriptions) [-> bcast_shared_uncond] -> sample_and_remask
//       run_graphed             upload_schedule -> graph_key -> graph_find | capture + graph_insert -> replays
#include "engine.h"
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

using namespace showo;

namespace {

__global__ void init_cur_kernel(const int64_t* ids, int ld, int img_start, int64_t mask_id, int64_t offset, int64_t* cur, int N,
                                int total) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int b = i / N, n = i - b * N;
    int64_t v = ids[(int64_t)b * ld + img_start + n];
    cur[i] = (v == mask_id) ? mask_id : v - offset;
}
// uncond rows = uncond prefix (first `prefix` tokens) + cond tokens from `prefix` on (modeling_showo.py:137-138)
__global__ void build_ids_kernel(const int64_t* cond, const int64_t* uncond, int64_t* all, int B, int L, int prefix) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * L) return;
    int b = i / L, l = i - b * L;
    int64_t c = cond[i];
    all[i] = c;
    if (uncond) all[(int64_t)(B + b) * L + l] = (l < prefix) ? uncond[i] : c;
}
__global__ void rows_index_kernel(int32_t* rows, int nseq, int L, int img_start, int N) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nseq * N) return;
    int b = i / N, n = i - b * N;
    rows[i] = b * L + img_start + n;
}
// ---- t2i prefix reuse: rows [0, prefix) of every sequence (pads + text; causal, never see an image column) are step-invariant
__global__ void gather_ids_kernel(const int64_t* __restrict__ all, int64_t* __restrict__ act, int nseq, int L, int prefix) {
    const int La = L - prefix;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nseq * La) return;
    int b = i / La, j = i - b * La;
    act[i] = all[(int64_t)b * L + prefix + j];
}
__global__ void gather_iv_kernel(const int32_t* __restrict__ iv, int32_t* __restrict__ act, int nseq, int L, int prefix) {
    const int La = L - prefix;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nseq * La) return;
    int b = i / La, j = i - b * La;
    reinterpret_cast<int4*>(act)[i] = reinterpret_cast<const int4*>(iv)[(int64_t)b * L + prefix + j];
}
// out |= 1 if a prefix row can see a column >= prefix (then the prefix is not step-invariant), out |= 2 if *mask_flag is set
__global__ void prefix_check_kernel(const int32_t* __restrict__ iv, const int32_t* __restrict__ mask_flag, int32_t* __restrict__ out,
                                    int nseq, int L, int prefix) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && mask_flag && *mask_flag) atomicOr(out, 2);
    if (i >= nseq * prefix) return;
    int b = i / prefix, r = i - b * prefix;
    const int4 v = reinterpret_cast<const int4*>(iv)[(int64_t)b * L + r];
    int hi = 0;
    if (v.x < v.y) hi = max(hi, v.y);
    if (v.z < v.w) hi = max(hi, v.w);
    if (hi > prefix) atomicOr(out, 1);
}
// ---- t2i reduced step 0: which rows of the full step does the result need?  One block per sequence b.
//   p_b = the largest p <= prefix such that no row r >= p of the sequence sees a column < p (rows [p_b, L) are closed under "sees"; both
//         intervals of a row count).  With left padding that is the pad count: text and image rows never see a pad column.
//   out[2] / out[3] = max over the sequences [0, first] / (first, nseq) of prefix - p_b  (the uniform trim is the smallest p_b)
//   out[1] |= 1  when an unconditional sequence first+1 .. nseq-1 differs from sequence `first` in an id or an interval row (first > 0:
//                CFG call), or when the mask is not an interval mask (then also p = 0)
// (out[0] belongs to prefix_check_kernel; all four ints are zeroed before the two launches.)
__global__ void step0_plan_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ iv, const int32_t* __restrict__ mask_flag,
                                  int32_t* __restrict__ out, int first, int nseq, int L, int prefix) {
    __shared__ int s_min[256];
    __shared__ int s_best;
    const int b = blockIdx.x, t = threadIdx.x;
    const int4* row = reinterpret_cast<const int4*>(iv) + (int64_t)b * L;
    auto lo_of = [&](int r) {  // first column row r sees (INT_MAX: none)
        const int4 v = row[r];
        int lo = 0x7fffffff;
        if (v.x < v.y) lo = min(lo, v.x);
        if (v.z < v.w) lo = min(lo, v.z);
        return lo;
    };
    const int chunk = (L + 255) / 256, r0 = min(L, t * chunk), r1 = min(L, r0 + chunk);
    int m = 0x7fffffff;
    for (int r = r0; r < r1; ++r) m = min(m, lo_of(r));
    s_min[t] = m;
    if (t == 0) s_best = 0;
    __syncthreads();
    m = 0x7fffffff;  // min over the rows behind this thread's chunk
    for (int j = t + 1; j < 256; ++j) m = min(m, s_min[j]);
    for (int r = r1 - 1; r >= r0; --r) {
        m = min(m, lo_of(r));
        if (r <= prefix && m >= r) { atomicMax(&s_best, r); break; }
    }
    __syncthreads();
    if (t == 0) {
        atomicMax(out + (b <= first ? 2 : 3), prefix - s_best);
        if (b == 0 && mask_flag && *mask_flag) { atomicOr(out + 1, 1); atomicMax(out + 2, prefix); }
    }
    if (first > 0 && b > first) {
        const int64_t *ia = ids + (int64_t)first * L, *ib = ids + (int64_t)b * L;
        const int4* ra = reinterpret_cast<const int4*>(iv) + (int64_t)first * L;
        bool diff = false;
        for (int r = t; r < L; r += 256) {
            const int4 u = ra[r], v = row[r];
            diff |= ia[r] != ib[r] || u.x != v.x || u.y != v.y || u.z != v.z || u.w != v.w;
        }
        if (diff) atomicOr(out + 1, 1);
    }
}
// interval rows [p, L) of the first nseq sequences with every interval cut to columns >= p.  A no-op for the rows that are closed under
// "sees" at p; a pad row of a sequence with more than p pads would otherwise read cache rows < p, which the reduced step 0 never writes.
// Such a row then computes something else than in the full step, but nothing that is used can see it (it lies before its sequence's p_b).
__global__ void gather_iv_cut_kernel(const int32_t* __restrict__ iv, int32_t* __restrict__ act, int nseq, int L, int p) {
    const int La = L - p;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nseq * La) return;
    int b = i / La, j = i - b * La;
    int4 v = reinterpret_cast<const int4*>(iv)[(int64_t)b * L + p + j];
    v.x = max(v.x, p); v.z = max(v.z, p);
    reinterpret_cast<int4*>(act)[i] = v;
}
// Copies `len` units at `off` of every (layer, inner) chunk of one sequence to the same place of the next `ndst` sequences:
// chunk (li, h) starts at base + li * lstride + h * istride, sequences are seq_stride apart.  T = uint4 wherever the layout allows.
template <class T>
__global__ void bcast_seq_kernel(T* __restrict__ base, int64_t lstride, int inner, int64_t istride, int64_t off, int len, int64_t seq_stride,
                                 int ndst, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t o = i / len, li = o / inner;
    T* src = base + li * lstride + (o - li * inner) * istride + off + (i - o * len);
    const T v = *src;
    for (int d = 1; d <= ndst; ++d) src[d * seq_stride] = v;
}
// per-call constants of the graph-replayed denoise loop, passed BY VALUE as kernel arguments (no host staging buffer to keep alive,
// no stream synchronisation): sched[0..n) = mask_len_f | temperature per step, hdr = step index | pad | seed lo | seed hi
struct SchedArgs { float v[512]; int hdr[4]; int n; };
__global__ void sched_upload_kernel(SchedArgs a, float* __restrict__ sched, int* __restrict__ hdr) {
    for (int i = threadIdx.x; i < a.n; i += blockDim.x) sched[i] = a.v[i];
    if (threadIdx.x < 4) hdr[threadIdx.x] = a.hdr[threadIdx.x];
}
__global__ void copy_i64_kernel(const int64_t* s, int64_t* d, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = s[i];
}

// bcast_seq_kernel in the widest unit that every stride, offset and length (given in elements of E) is a multiple of
template <class E>
int bcast_seq(E* base, int64_t lstride, int n_layers, int inner, int64_t istride, int64_t off, int64_t len, int64_t seq_stride, int ndst,
              hipStream_t s) {
    if (ndst <= 0 || len <= 0) return 0;
    constexpr int W = 16 / (int)sizeof(E);
    const bool wide = !(lstride % W) && !(istride % W) && !(off % W) && !(len % W) && !(seq_stride % W) && !((uintptr_t)base & 15);
    const int64_t u = wide ? W : 1, total = (int64_t)n_layers * inner * (len / u);
    if (len / u >= ((int64_t)1 << 31) || (total + 255) / 256 >= ((int64_t)1 << 31)) return set_error_msg(5, "t2i: broadcast too large");
    const dim3 grid((unsigned)((total + 255) / 256));
    if (wide)
        bcast_seq_kernel<uint4><<<grid, dim3(256), 0, s>>>(reinterpret_cast<uint4*>(base), lstride / W, inner, istride / W, off / W, (int)(len / W),
                                                           seq_stride / W, ndst, total);
    else
        bcast_seq_kernel<E><<<grid, dim3(256), 0, s>>>(base, lstride, inner, istride, off, (int)len, seq_stride, ndst, total);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

using T2I = showo_engine::T2I;
constexpr int thr = 256;
dim3 blocks(int n) { return dim3((n + thr - 1) / thr); }

// what is fixed for one showo_engine_t2i_generate call: filled once by the entry point, read by every stage
struct T2ICall {
    int B, nseq, L, N, prefix, La, LpC, img_start, nrows;  // nseq = B or 2 B (CFG); La = L - prefix active rows; LpC = L rounded up to 64
    bool cfg, pfast;
    int id_offset, codebook, steps, use_graph;
    int64_t mask_id;
    float guidance;
    uint64_t seed;
    int64_t *ids_cond, *ids_uncond;
    const float *mask, *mask_len_host, *temps_host, *exp_noise, *uniform;
    const int32_t *iv, *flag;  // visibility intervals of the call (compressed from `mask`, or the caller's), null: causal
    hipStream_t s;
};
// the reduced step 0 as decided on the device: sequences run, leading rows trimmed, one unconditional sequence standing for all B
struct Step0Plan {
    int nseq0, p0;
    bool shared;
    bool reduced() const { return shared || p0 > 0; }
};
// one attempt's running state: where K / V^T go, and whether a step has run yet
struct Attempt {
    bool reuse;
    Step0Plan plan;
    KVDest kvc;
    bool first_step = true;
};
// "rows through the model": gather ids -> embed -> pin split-K -> layers -> head, for some rows of some sequences
struct RowPass {
    int nseq, rows, pos0;       // sequences, rows per sequence, position of the first row
    const int32_t* iv;          // interval table of those rows
    bool dense;                 // the call's dense mask and its flag go along (the full step only)
    bool gather;                // ids of the columns [pos0, L) are gathered first; otherwise embed straight from ids_all
    const int32_t* head_index;  // rows of x that feed the head
    int n_head;
    int pin_layers, pin_head;   // gemm_pin_split_m of the layers / of the head (0: none)
};

// the precisions whose layers run on the production kernels: they can reuse the prefix and replay a cached graph
bool on_production_kernels(const showo_engine* e, bool pfast) { return e->precision == 0 || e->precision == 2 || e->precision == 3 || pfast; }

// ---- the graph cache: instantiated graphs of one denoise step, least recently used out first (see showo_engine::T2I) ---------------
T2I::GraphEntry* graph_find(T2I& t, const T2I::GraphKey& key) {
    for (auto& ge : t.graphs)
        if (memcmp(&key, &ge.key, sizeof(key)) == 0) return &ge;
    return nullptr;
}
void graph_touch(T2I& t, T2I::GraphEntry* ent) { ent->last_use = ++t.tick; }
T2I::GraphEntry* graph_insert(T2I& t, const T2I::GraphKey& key, hipGraphExec_t exec) {
    if ((int)t.graphs.size() >= T2I::T2I_GRAPH_SLOTS) {  // evict the least recently used graph
        size_t lru = 0;
        for (size_t i = 1; i < t.graphs.size(); ++i)
            if (t.graphs[i].last_use < t.graphs[lru].last_use) lru = i;
        // the evicted graph may still be executing a previous call's replays on another stream
        hipDeviceSynchronize();
        hipGraphExecDestroy(t.graphs[lru].exec);
        t.graphs.erase(t.graphs.begin() + lru);
    }
    t.graphs.push_back(T2I::GraphEntry{key, exec, 0});
    t.captures++;
    return &t.graphs.back();
}
// everything BAKED into the launches of a captured step (see showo_engine::T2I)
T2I::GraphKey graph_key(const showo_engine* e, const T2ICall& c, bool reuse) {
    const T2I& t = e->t2i;
    T2I::GraphKey key;
    memset(&key, 0, sizeof(key));  // padding bytes take part in the memcmp of graph_find
    key.B = c.B; key.nseq = c.nseq; key.L = c.L; key.N = c.N; key.prefix = c.prefix; key.steps = c.steps; key.id_offset = c.id_offset;
    key.codebook = c.codebook; key.reuse = reuse ? 1 : 0; key.cfg = c.cfg ? 1 : 0; key.has_iv = c.iv ? 1 : 0;
    key.mask_id = c.mask_id; key.guidance = c.guidance; key.prec = e->precision;
    key.p[11] = (reuse && c.pfast) ? t.tk_lo : nullptr; key.p[12] = (reuse && c.pfast) ? t.tvt_lo : nullptr;
    if (!reuse) { key.p[0] = c.iv; key.p[1] = c.flag; key.p[2] = c.mask; }  // with reuse the captured step reads t.iv_act only
    key.p[3] = c.exp_noise; key.p[4] = c.uniform; key.p[5] = t.row_logits;
    key.p[6] = reuse ? t.tk : nullptr; key.p[7] = reuse ? t.tvt : nullptr; key.p[8] = t.sched_dev; key.p[9] = t.step_dev; key.p[10] = c.s;
    return key;
}

// ---- the stages of an attempt ------------------------------------------------------------------------------------------------------
// ids of every sequence, the image tokens as codes, the head's row list; with reuse the prefix check (and, red, the step-0 plan) whose
// four flag words travel to pinned host memory behind ev_pfx
int queue_inputs(showo_engine* e, const T2ICall& c, bool reuse, bool red, bool* check_pending) {
    T2I& t = e->t2i;
    build_ids_kernel<<<blocks(c.B * c.L), dim3(thr), 0, c.s>>>(c.ids_cond, c.cfg ? c.ids_uncond : nullptr, t.ids_all, c.B, c.L, c.prefix);
    init_cur_kernel<<<blocks(c.B * c.N), dim3(thr), 0, c.s>>>(c.ids_cond, c.L, c.img_start, c.mask_id, c.id_offset, t.cur, c.N, c.B * c.N);
    rows_index_kernel<<<blocks(c.nrows), dim3(thr), 0, c.s>>>(e->rows, c.nseq, c.L, c.img_start, c.N);
    SHOWO_CHECK_HIP(hipGetLastError());
    if (reuse && c.iv) {
        SHOWO_CHECK_HIP(hipMemsetAsync(t.pfx_flag, 0, 4 * sizeof(int32_t), c.s));
        prefix_check_kernel<<<blocks(c.nseq * c.prefix), dim3(thr), 0, c.s>>>(c.iv, c.flag, t.pfx_flag, c.nseq, c.L, c.prefix);
        if (red) step0_plan_kernel<<<dim3(c.nseq), dim3(256), 0, c.s>>>(t.ids_all, c.iv, c.flag, t.pfx_flag, c.cfg ? c.B : 0, c.nseq, c.L, c.prefix);
        SHOWO_CHECK_HIP(hipMemcpyAsync(t.pfx_host, t.pfx_flag, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        SHOWO_CHECK_HIP(hipEventRecord(t.ev_pfx, c.s));
        *check_pending = true;
    }
    return 0;
}

// The one host wait in front of step 0: grid sizes depend on the plan.  *prefix_bad: the prefix check, read in the same wait, fired.
int wait_step0_plan(showo_engine* e, const T2ICall& c, Step0Plan* plan, bool* prefix_bad) {
    T2I& t = e->t2i;
    const auto t0 = std::chrono::steady_clock::now();
    SHOWO_CHECK_HIP(hipEventSynchronize(t.ev_pfx));
    t.step0[3] += (int)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    const volatile int32_t* h = t.pfx_host;
    *prefix_bad = h[0] != 0;
    if (*prefix_bad) return 0;
    plan->shared = c.cfg && c.B > 1 && !h[1];
    const int trim_short = plan->shared ? h[2] : std::max(h[2], h[3]);
    plan->p0 = std::min(std::max(c.prefix - trim_short, 0), c.prefix);
    plan->nseq0 = plan->shared ? c.B + 1 : c.nseq;
    return 0;
}

// the batch-wide K / V^T cache of this call (grown on demand, V^T zeroed) and the interval / row-index lists of the active rows
int prepare_prefix_cache(showo_engine* e, const T2ICall& c, const Step0Plan& plan, KVDest* kvc) {
    T2I& t = e->t2i;
    hipStream_t s = c.s;
    const int64_t kn = (int64_t)e->nL * c.nseq * e->nH * c.L * 64, vn = (int64_t)e->nL * c.nseq * e->nH * 64 * c.LpC;
    if (kn > t.tk_cap) { TRY(e->alloc(&t.tk, kn)); t.tk_cap = kn; }
    if (vn > t.tvt_cap) { TRY(e->alloc(&t.tvt, vn)); t.tvt_cap = vn; }
    SHOWO_CHECK_HIP(hipMemsetAsync(t.tvt, 0, (size_t)vn * sizeof(bf16_t), s));  // pad key columns must stay finite
    // (iv_act / rows_act: the active rows of the later steps, and behind them those of the reduced step 0)
    if (!t.ids_act) { TRY(e->alloc(&t.ids_act, e->maxT)); TRY(e->alloc(&t.iv_act, e->maxT * 8)); TRY(e->alloc(&t.rows_act, e->maxT * 2)); }
    if (t.poison) SHOWO_CHECK_HIP(hipMemsetAsync(t.tk, 0xff, (size_t)kn * sizeof(bf16_t), s));
    if (c.pfast) {
        if (kn > t.tk_lo_cap) { TRY(e->alloc(&t.tk_lo, kn)); t.tk_lo_cap = kn; }
        if (vn > t.tvt_lo_cap) { TRY(e->alloc(&t.tvt_lo, vn)); t.tvt_lo_cap = vn; }
        SHOWO_CHECK_HIP(hipMemsetAsync(t.tvt_lo, 0, (size_t)vn * sizeof(bf16_t), s));
        if (t.poison) SHOWO_CHECK_HIP(hipMemsetAsync(t.tk_lo, 0xff, (size_t)kn * sizeof(bf16_t), s));
    }
    *kvc = KVDest{t.tk, t.tvt, (int64_t)c.nseq * e->nH * c.L * 64, (int64_t)c.nseq * e->nH * 64 * c.LpC, c.L, c.LpC, c.pfast ? t.tk_lo : nullptr,
                  c.pfast ? t.tvt_lo : nullptr};
    if (c.iv) gather_iv_kernel<<<blocks(c.nseq * c.La), dim3(thr), 0, s>>>(c.iv, t.iv_act, c.nseq, c.L, c.prefix);
    rows_index_kernel<<<blocks(c.nrows), dim3(thr), 0, s>>>(t.rows_act, c.nseq, c.La, c.img_start - c.prefix, c.N);
    if (plan.reduced()) {
        const int nseq0 = plan.nseq0, p0 = plan.p0;
        gather_iv_cut_kernel<<<blocks(nseq0 * (c.L - p0)), dim3(thr), 0, s>>>(c.iv, t.iv_act + e->maxT * 4, nseq0, c.L, p0);
        rows_index_kernel<<<blocks(nseq0 * c.N), dim3(thr), 0, s>>>(t.rows_act + e->maxT, nseq0, c.L - p0, c.img_start - p0, c.N);
    }
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

// p.nseq x p.rows rows through the model into row_logits.  The pin is reset on every exit path.
int run_rows(showo_engine* e, const T2ICall& c, const KVDest& kvc, const RowPass& p) {
    T2I& t = e->t2i;
    const int64_t* ids = t.ids_all;
    if (p.gather) {
        gather_ids_kernel<<<blocks(p.nseq * p.rows), dim3(thr), 0, c.s>>>(t.ids_all, t.ids_act, p.nseq, c.L, p.pos0);
        ids = t.ids_act;
    }
    TRY(showo_embed_f32(ids, e->embed, e->x, p.nseq * p.rows, e->H, e->V, c.s));
    showo::gemm_pin_split_m(p.pin_layers);
    int rc = run_layers(e, p.nseq, p.rows, p.pos0, kvc, p.iv, p.dense ? c.flag : nullptr, p.dense ? c.mask : nullptr, c.s);
    showo::gemm_pin_split_m(p.pin_head);
    if (!rc) rc = head_rows(e, p.head_index, p.n_head, c.id_offset, c.codebook, t.row_logits, c.s);
    showo::gemm_pin_split_m(0);
    return rc;
}

// the one unconditional sequence (index B) stands for all B: its prefix K rows [p0, prefix) and V^T columns (widened to
// 16-byte units: columns < p0 are zero on both sides, columns >= prefix are rewritten by every later step) of every
// layer, and its logit rows
int bcast_shared_uncond(showo_engine* e, const T2ICall& c, int p0, const KVDest& kvc) {
    const int B = c.B, L = c.L, LpC = c.LpC;
    const int64_t ks = (int64_t)e->nH * L * 64, vs = (int64_t)e->nH * 64 * LpC;
    const int c0 = p0 & ~7, c1 = std::min(LpC, (c.prefix + 7) & ~7);
    for (int half = 0; half < (c.pfast ? 2 : 1); ++half) {
        TRY(bcast_seq(half ? kvc.k_lo : kvc.k, kvc.k_lstride, e->nL, e->nH, (int64_t)L * 64, B * ks + (int64_t)p0 * 64,
                      (int64_t)(c.prefix - p0) * 64, ks, B - 1, c.s));
        TRY(bcast_seq(half ? kvc.vt_lo : kvc.vt, kvc.v_lstride, e->nL, e->nH * 64, (int64_t)LpC, B * vs + c0, (int64_t)(c1 - c0), vs, B - 1, c.s));
    }
    return bcast_seq(e->t2i.row_logits, 0, 1, 1, 0, (int64_t)B * c.N * c.codebook, (int64_t)c.N * c.codebook, (int64_t)c.N * c.codebook, B - 1, c.s);
}

// CFG softmax + draw, then re-mask by confidence.  step < 0: the step index / schedule constants are read on the device and the noise
// offsets are applied inside the kernels.
int sample_and_remask(showo_engine* e, const T2ICall& c, int step) {
    T2I& t = e->t2i;
    const int B = c.B, N = c.N;
    const float* lu = c.cfg ? t.row_logits + (int64_t)B * N * c.codebook : nullptr;
    const bool dev = step < 0;
    TRY(showo_cfg_softmax_sample(t.row_logits, lu, c.codebook, c.guidance, t.cur, c.mask_id,
                                 c.exp_noise ? c.exp_noise + (dev ? 0 : (int64_t)step * B * N * c.codebook) : nullptr, c.seed,
                                 (uint32_t)(dev ? 0 : step), t.sampled, t.sel, B, N, c.codebook, c.s));
    return showo_mask_by_topk(t.sel, t.sampled, t.cur, t.ids_all, c.cfg ? t.ids_all + (int64_t)B * c.L : nullptr, c.L, c.img_start,
                              c.mask_id, c.id_offset, dev ? 0.f : c.mask_len_host[step], dev ? 0.f : c.temps_host[step],
                              c.uniform ? c.uniform + (dev ? 0 : (int64_t)step * B * N) : nullptr, c.seed, (uint32_t)(dev ? 0 : step), nullptr,
                              B, N, c.s);
}

// one denoise step (modeling_showo.py:135-179).  step < 0: device-step mode (sample_and_remask).
// full: run every row (always in step 0); otherwise only the rows [prefix, L) against the cached prefix keys.
int denoise_step(showo_engine* e, const T2ICall& c, Attempt& a, int step, bool full) {
    T2I& t = e->t2i;
    const int nseq = c.nseq, L = c.L;
    if (full && a.plan.reduced()) {
        // rows [p0, L) of the sequences 0 .. nseq0 - 1 through the machinery of the later steps; K / V^T go to their true positions in
        // the batch-wide cache (cache rows < p0 are never written and never visible: the attention kernel selects masked scores away,
        // V^T there is zero).  Every GEMM keeps the k-partition of the full-shape launch it replaces (gemm_pin_split_m).
        const int nseq0 = a.plan.nseq0, p0 = a.plan.p0;
        TRY(run_rows(e, c, a.kvc, RowPass{nseq0, L - p0, p0, t.iv_act + e->maxT * 4, false, true, t.rows_act + e->maxT, nseq0 * c.N,
                                          nseq * L, nseq * c.N}));
        if (a.plan.shared) TRY(bcast_shared_uncond(e, c, p0, a.kvc));
    } else if (full) {
        TRY(run_rows(e, c, a.kvc, RowPass{nseq, L, 0, c.iv, true, false, e->rows, c.nrows, 0, 0}));
    } else {
        // like the reduced step 0, the active-rows launches sum K in the order of the full-shape launches they stand for: with fewer
        // than 16 sequences the residual GEMM splits K and the count follows M, and the text rows in the cache (step 0) and the path
        // without reuse were summed in the full shape's order.  (Baked into the captured launches; a no-op where neither shape splits.)
        TRY(run_rows(e, c, a.kvc, RowPass{nseq, c.La, c.prefix, c.iv ? t.iv_act : nullptr, false, true, t.rows_act, c.nrows, nseq * L, 0}));
    }
    if (a.first_step && t.logits0)
        SHOWO_CHECK_HIP(hipMemcpyAsync(t.logits0, t.row_logits, (size_t)c.nrows * c.codebook * sizeof(float), hipMemcpyDeviceToDevice, c.s));
    a.first_step = false;
    return sample_and_remask(e, c, step);
}

// step index | pad | seed and the per-step schedule into device memory, where the captured step reads them
int upload_schedule(showo_engine* e, const T2ICall& c) {
    T2I& t = e->t2i;
    const int steps = c.steps;
    if (!t.step_dev) { TRY(e->alloc(&t.step_dev, 4)); }
    if (t.sched_cap < 2 * steps) {
        // (re)allocation changes a pointer baked into cached graphs: they are keyed on it (p[8]) and simply miss afterwards
        TRY(e->alloc(&t.sched_dev, 2 * (steps > 256 ? steps : 256))); t.sched_cap = 2 * (steps > 256 ? steps : 256);
    }
    if (2 * steps <= 512) {
        SchedArgs a;
        for (int i = 0; i < steps; ++i) { a.v[i] = c.mask_len_host[i]; a.v[steps + i] = c.temps_host[i]; }
        a.hdr[0] = 0; a.hdr[1] = 0; a.hdr[2] = (int)(uint32_t)(c.seed & 0xffffffffu); a.hdr[3] = (int)(uint32_t)(c.seed >> 32);
        a.n = 2 * steps;
        sched_upload_kernel<<<1, 256, 0, c.s>>>(a, t.sched_dev, t.step_dev);
        SHOWO_CHECK_HIP(hipGetLastError());
    } else {
        std::vector<float> sched(2 * steps);
        for (int i = 0; i < steps; ++i) { sched[i] = c.mask_len_host[i]; sched[steps + i] = c.temps_host[i]; }
        const int hdr[4] = {0, 0, (int)(uint32_t)(c.seed & 0xffffffffu), (int)(uint32_t)(c.seed >> 32)};  // step index | pad | seed
        SHOWO_CHECK_HIP(hipMemcpyAsync(t.sched_dev, sched.data(), sizeof(float) * 2 * steps, hipMemcpyHostToDevice, c.s));
        SHOWO_CHECK_HIP(hipMemcpyAsync(t.step_dev, hdr, sizeof(hdr), hipMemcpyHostToDevice, c.s));
        SHOWO_CHECK_HIP(hipStreamSynchronize(c.s));  // `sched` / `hdr` are host temporaries
    }
    return 0;
}

// hipGraph path (the default of Showo.t2i_generate): ONE denoise step -- every row from <soi> on, ~80 kernels -- is captured with
// everything that changes from step to step or call to call in device memory (step index, schedule constants, seed, the gathered
// visibility intervals) and the instantiated graph is CACHED on the engine (LRU of T2I_GRAPH_SLOTS), keyed by every launch
// argument baked into it; later calls with the same key replay it without capturing again and without a host synchronisation.
// The eager steps before a capture (2 with prefix reuse: the full step 0 and one active-rows step) launch every kernel variant
// once (first-use attributes, GEMM tile tuning) outside the capture; step 0 always runs eagerly.  Not combined with per-launch
// event timing.
int run_graphed(showo_engine* e, const T2ICall& c, Attempt& a, int n_eager) {
    T2I& t = e->t2i;
    TRY(upload_schedule(e, c));
    showo::sampler_set_device_step(t.step_dev, t.sched_dev, c.steps);
    auto step = [&](bool full) -> int {
        const int rs = denoise_step(e, c, a, -1, full);
        return rs ? rs : showo::sampler_step_inc(t.step_dev, c.s);
    };
    const T2I::GraphKey key = graph_key(e, c, a.reuse);
    T2I::GraphEntry* ent = graph_find(t, key);
    const int first_replay = ent ? 1 : n_eager;
    int rc = 0;
    for (int i = 0; i < first_replay && !rc; ++i) rc = step(i == 0 || !a.reuse);
    if (!rc && !ent) {
        hipGraphExec_t exec = nullptr;
        rc = showo::capture_step(c.s, [&]() -> int { return step(!a.reuse); }, &exec);
        if (!rc) ent = graph_insert(t, key, exec);
    }
    if (!rc) graph_touch(t, ent);
    for (int i = first_replay; !rc && i < c.steps; ++i) {
        hipError_t he = hipGraphLaunch(ent->exec, c.s);
        if (he != hipSuccess) rc = set_error_hip(he, "hipGraphLaunch", __FILE__, __LINE__);
    }
    showo::sampler_set_device_step(nullptr, nullptr, 0);
    return rc;
}

// One pass over all steps, with or without prefix reuse.  *retry: the prefix check fired -- a text row sees an image column, or the mask
// is not an interval mask -- and the call must be repeated without reuse.
int attempt(showo_engine* e, const T2ICall& c, bool reuse, bool* retry) {
    T2I& t = e->t2i;
    *retry = false;
    // ---- reduced step 0 (use_graph bit 2 disables it).  Step 0 only has to leave the prefix K / V^T in the cache and produce the image
    // rows' logits.  (a) Leading rows that no later row can see (left pads) feed nothing: rows [p0, L) are run, p0 the smallest of the
    // sequences' own trims (the pad rows that a sequence has beyond p0 run with their intervals cut at p0: nothing that is used sees
    // them).  (b) In a pure t2i CFG call the unconditional sequences are ONE sequence (empty prompt, all-mask image part): it is run once
    // and its prefix K / V^T and logit rows are copied to the other B - 1.  Both are decided on the device from the ids and intervals of
    // THIS call; grid sizes depend on the answer, so the host waits for it here, once, before the first launch of step 0.
    const bool red = reuse && c.iv && !(c.use_graph & 4);
    bool check_pending = false;
    TRY(queue_inputs(e, c, reuse, red, &check_pending));
    Attempt a{reuse, Step0Plan{c.nseq, 0, false}, kv_workspace(e, c.L)};
    if (red) {
        TRY(wait_step0_plan(e, c, &a.plan, retry));
        if (*retry) return 0;  // repeat without reuse (and without the optimistic attempt)
        check_pending = false;
    }
    if (reuse) {
        t.step0[0] = a.plan.nseq0; t.step0[1] = a.plan.p0; t.step0[2] = a.plan.nseq0 * (c.L - a.plan.p0);
        TRY(prepare_prefix_cache(e, c, a.plan, &a.kvc));
    }
    const int n_eager = reuse ? 2 : 1;
    // A registered range-check counter forces the eager path: its launches (and the caller's counter pointer) must not be baked into a
    // cached graph that later plain calls replay, and a replayed cached graph would skip them.
    const bool graph = (c.use_graph & 1) && c.steps > n_eager && !showo::g_prof_on_query() && on_production_kernels(e, c.pfast) &&
                       !(e->range_count && e->precision == 2);
    if (!graph) {
        for (int step = 0; step < c.steps; ++step) TRY(denoise_step(e, c, a, step, step == 0 || !reuse));
    } else {
        TRY(run_graphed(e, c, a, n_eager));
    }
    if (check_pending) {
        SHOWO_CHECK_HIP(hipEventSynchronize(t.ev_pfx));  // recorded before the first step: long since complete
        *retry = *(volatile int32_t*)t.pfx_host != 0;
    }
    return 0;
}

}  // namespace

extern "C" int showo_engine_t2i_captures(const showo_engine* e) { return e ? e->t2i.captures : -1; }
// what step 0 of the last showo_engine_t2i_generate call ran: sequences, leading rows trimmed, rows (= out[0] * (L - out[1])), and the
// host time in microseconds spent waiting for that decision
extern "C" int showo_engine_t2i_step0(const showo_engine* e, int* out) {
    if (!e || !out) return set_error_msg(1, "engine: null argument");
    for (int i = 0; i < 4; ++i) out[i] = e->t2i.step0[i];
    return 0;
}
// test hooks of t2i_generate.  logits0 (device, fp32 [nseq * N, codebook], or null): receives the logit rows of step 0.  poison_kv: the
// batch-wide K cache is filled with NaN bit patterns at the start of every call (rows that no step writes must never reach a result).
extern "C" int showo_engine_t2i_debug(showo_engine* e, float* logits0, int poison_kv) {
    if (!e) return set_error_msg(1, "engine: null handle");
    e->t2i.logits0 = logits0;
    e->t2i.poison = poison_kv != 0;
    return 0;
}

extern "C" int showo_engine_t2i_generate(showo_engine* e, int64_t* ids_cond, int64_t* ids_uncond, const float* mask, int B,
                                         int L, int N, int text_len, int64_t mask_id, int id_offset, int codebook,
                                         float guidance, int steps, const float* mask_len_host, const float* temps_host,
                                         uint64_t seed, const float* exp_noise, const float* uniform, int use_graph,
                                         int64_t* sampled_out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const bool cfg = (ids_uncond != nullptr) && guidance > 0.f;  // modeling_showo.py:136
    const int nseq = cfg ? 2 * B : B;
    TRY(check_ready(e, nseq, L));
    if (N + 2 > L || steps < 1 || !mask_len_host || !temps_host) return set_error_msg(1, "t2i: bad arguments");
    if (id_offset + codebook > e->V) return set_error_msg(1, "t2i: codebook slice exceeds the vocabulary");
    T2I& t = e->t2i;
    T2ICall c;
    c.B = B; c.nseq = nseq; c.L = L; c.N = N; c.cfg = cfg;
    c.img_start = L - (N + 1);  // input_ids[:, -(N+1):-1]
    c.nrows = nseq * N;
    if ((int64_t)c.nrows * codebook > t.row_logits_cap) {
        t.row_logits_cap = (int64_t)c.nrows * codebook;
        TRY(e->alloc(&t.row_logits, t.row_logits_cap));
    }
    c.iv = nullptr; c.flag = nullptr;
    if (mask) {
        TRY(showo_mask_compress(mask, e->iv, e->flag, nseq, L, L, s));  // the mask is step-invariant: compress once
        c.iv = e->iv; c.flag = e->flag;
    } else if (e->ext_iv) {
        c.iv = e->ext_iv; c.flag = e->ext_flag;
    }
    // ---- prefix reuse.  Rows [0, prefix) of every sequence (pads + text, prefix = position of <soi>) are causal: they never see
    // an image column, and their ids never change, so their hidden states -- hence their K / V in every layer -- are the same
    // in all steps.  Step 0 runs the whole sequence and leaves K / V^T of every layer in a batch-wide cache; the later steps run
    // only the rows [prefix, L) (soi, image tokens, eoi: 258 of 387 at 256x256) against the cached text keys.  Exact up to the
    // grouping of rows into tiles (same arithmetic per row); checked on the device: interval masks only, no prefix row may see
    // a column >= prefix.  use_graph bit 1 disables it.
    // The check is DEFERRED: its flag travels to pinned host memory behind an event and is read after every step of the call has
    // been queued (the GPU never waits for the host); in the case that it fires the call is repeated without reuse -- ids_cond /
    // sampled_out are only written at the very end, so nothing of the optimistic attempt is visible to the caller.
    c.prefix = text_len + 1;
    c.La = L - c.prefix;
    c.LpC = ((L + 63) / 64) * 64;
    c.pfast = e->precision == 1 && precise_fast_ok(e);
    c.id_offset = id_offset; c.codebook = codebook; c.steps = steps; c.use_graph = use_graph;
    c.mask_id = mask_id; c.guidance = guidance; c.seed = seed;
    c.ids_cond = ids_cond; c.ids_uncond = ids_uncond;
    c.mask = mask; c.mask_len_host = mask_len_host; c.temps_host = temps_host; c.exp_noise = exp_noise; c.uniform = uniform;
    c.s = s;
    const bool reuse_ok = on_production_kernels(e, c.pfast) && !(use_graph & 2) && steps > 1 && c.prefix >= 1 && c.La >= N + 1 && nseq * c.La >= 1;
    hipStreamCaptureStatus cs0 = hipStreamCaptureStatusNone;
    hipStreamIsCapturing(s, &cs0);
    if (cs0 != hipStreamCaptureStatusNone) return set_error_msg(7, "t2i_generate: the call captures its own graph; do not call it inside a stream capture");
    TRY(fused_sync(e, s));  // weight images of the fused launches: rebuilt here (never inside a capture), so cached graphs stay valid
    if (c.pfast) TRY(precise_sync(e, s));
    if (e->precision == 2) TRY(head3_sync(e, s));
    if (reuse_ok && !t.pfx_flag) {
        TRY(e->alloc(&t.pfx_flag, 4));
        SHOWO_CHECK_HIP(hipHostMalloc((void**)&t.pfx_host, 64, hipHostMallocDefault));
        SHOWO_CHECK_HIP(hipEventCreateWithFlags(&t.ev_pfx, hipEventDisableTiming));
    }
    t.step0[0] = nseq; t.step0[1] = 0; t.step0[2] = nseq * L; t.step0[3] = 0;
    for (int n = 0; n < 2; ++n) {
        bool retry = false;
        TRY(attempt(e, c, reuse_ok && n == 0, &retry));
        if (!retry) break;
    }
    copy_i64_kernel<<<blocks(B * L), dim3(thr), 0, s>>>(t.ids_all, ids_cond, B * L);  // in-place update like the reference
    copy_i64_kernel<<<blocks(B * N), dim3(thr), 0, s>>>(t.sampled, sampled_out, B * N);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}
