// KV-cached AR decode of ONE sequence on the engine's own cache: prefill, decode step, append (mmu sessions), rewind, and the
// continuation loop { embed -> layers -> lm_head -> next token } whose step replays as a hipGraph (engine.h replay_steps).
//
// The incremental form of Showo.mmu_generate (models/modeling_showo.py:183-240; the reference re-runs the whole sequence per token,
// here K / V of earlier rows are cached, which is exact because the mask it grows never lets an old row see a new column,
// modeling_showo.py:203-217).  The layers and the head are the engine's (engine.hip run_layers / head_rows; a one-token step takes the
// fused launches of decode.hip); engine_prefill_into / engine_append_into also fill the slots of a decode batch (decode_batch.hip).
#include "engine.h"
#include "logit_adjust.h"
#include "seq_rules.h"

using namespace showo;

namespace {

__global__ void set_iv_kernel(int32_t* iv, int a, int b, int c, int d) {
    if (threadIdx.x == 0) { iv[0] = a; iv[1] = b; iv[2] = c; iv[3] = d; }
}
// V^T columns [c0, c1) of every (layer, head, d) row of one sequence's cache: grid (nH * 64 rows, layers), row pitch = Lp
__global__ void zero_vt_cols_kernel(bf16_t* vt, int64_t lstride, int Lp, int c0, int c1) {
    bf16_t* r = vt + blockIdx.y * lstride + (int64_t)blockIdx.x * Lp;
    for (int c = c0 + threadIdx.x; c < c1; c += blockDim.x) r[c] = 0;
}
// mask row of the token at position *pos: the last prompt row extended by the columns [L0, pos] (modeling_showo.py:203-217)
__global__ void decode_iv_kernel(const int32_t* __restrict__ last_iv, int L0, const int* __restrict__ pos, int32_t* __restrict__ iv) {
    if (threadIdx.x != 0) return;
    int a = last_iv[0], b = last_iv[1], c = last_iv[2], d = last_iv[3];
    const int P = *pos;
    if (b == L0 && a < b) b = P + 1;
    else if (d == L0 && c < d) d = P + 1;
    else if (!(c < d)) { c = L0; d = P + 1; }
    else if (!(a < b)) { a = L0; b = P + 1; }
    iv[0] = a; iv[1] = b; iv[2] = c; iv[3] = d;
}
__global__ void store_token_kernel(const int64_t* __restrict__ tok, int64_t* __restrict__ out, const int* __restrict__ pos, int base) {
    if (threadIdx.x == 0) out[*pos - base] = *tok;
}

}  // namespace

KVDest showo::kv_decode_cache(showo_engine* e) {
    return KVDest{e->kcache, e->vtcache, (int64_t)e->nH * e->cache_cap * 64, (int64_t)e->nH * 64 * e->cache_cap, e->cache_cap, e->cache_cap,
                  e->kcache_lo, e->vtcache_lo};
}

// ---- KV-cached decode ---------------------------------------------------------------------------------
static int ensure_cache(showo_engine* e, int need) {
    if (need <= e->cache_cap) return 0;
    int cap = ((need + 63) / 64) * 64;
    if (cap > e->cfg.max_pos) cap = ((e->cfg.max_pos + 63) / 64) * 64;
    if (need > cap) return set_error_msg(5, "decode: sequence exceeds max_position_embeddings");
    if (e->cache_cap != 0) return set_error_msg(5, "decode: cache capacity exceeded");
    // allocate once at the maximum the position table allows (2048 tokens: 2 x 201 MB at full size)
    cap = ((e->cfg.max_pos + 63) / 64) * 64;
    int64_t n = (int64_t)e->nL * e->nH * cap * 64;
    TRY(e->alloc(&e->kcache, n));
    TRY(e->alloc(&e->vtcache, n));
    hipMemset(e->kcache, 0, (size_t)n * sizeof(bf16_t));
    hipMemset(e->vtcache, 0, (size_t)n * sizeof(bf16_t));
    e->cache_cap = cap;
    return 0;
}
// accuracy mode: low halves of the decode cache (same capacity), allocated when the first precision-1 prefill arrives
static int ensure_cache_lo(showo_engine* e) {
    if (e->kcache_lo || e->cache_cap == 0) return 0;
    const int64_t n = (int64_t)e->nL * e->nH * e->cache_cap * 64;
    TRY(e->alloc(&e->kcache_lo, n));
    TRY(e->alloc(&e->vtcache_lo, n));
    hipMemset(e->kcache_lo, 0, (size_t)n * sizeof(bf16_t));
    hipMemset(e->vtcache_lo, 0, (size_t)n * sizeof(bf16_t));
    return 0;
}

// prefill of ONE sequence into a given per-layer K / V^T destination (the engine's own decode cache, or a slot of a decode batch):
// runs the prompt, leaves K / V^T of every layer there, returns the last prompt row's visibility intervals and its logits
namespace showo {
int engine_prefill_into(showo_engine* e, const int64_t* ids, const float* embeds, const float* mask, int L, bf16_t* k, bf16_t* vt,
                        int64_t k_lstride, int64_t v_lstride, int cap, int* last_iv_out, float* logits_last, hipStream_t s,
                        bf16_t* k_lo, bf16_t* vt_lo) {
    TRY(embed_in(e, ids, embeds, L, s));
    const int32_t *iv = nullptr, *flag = nullptr;
    if (mask) {
        TRY(showo_mask_compress(mask, e->iv, e->flag, 1, L, L, s));
        iv = e->iv; flag = e->flag;
    } else if (e->ext_iv) {  // caller-built intervals (showo_engine_use_intervals, e.g. from showo_mask_mmu_vit)
        iv = e->ext_iv; flag = e->ext_flag;
    }
    // The prefill attention multiplies the V^T columns of its last 64-key tile beyond L by P = 0, which is 0 only if they are finite.
    // The projection epilogue of >= 256-row prefills writes columns [0, L) alone, and a cache is zeroed once, when it is allocated: an
    // earlier, longer prompt with a NaN activation may have left NaN in [L, 64 * ceil(L / 64)).
    const int c1 = ((L + 63) / 64) * 64 < cap ? ((L + 63) / 64) * 64 : cap;
    if (c1 > L) {
        zero_vt_cols_kernel<<<dim3(e->nH * 64, e->nL), 64, 0, s>>>(vt, v_lstride, cap, L, c1);
        SHOWO_CHECK_HIP(hipGetLastError());
        if (vt_lo) {
            zero_vt_cols_kernel<<<dim3(e->nH * 64, e->nL), 64, 0, s>>>(vt_lo, v_lstride, cap, L, c1);
            SHOWO_CHECK_HIP(hipGetLastError());
        }
    }
    TRY(run_layers(e, 1, L, 0, KVDest{k, vt, k_lstride, v_lstride, cap, cap, k_lo, vt_lo}, iv, flag, mask, s));
    if (iv) {
        int32_t f = 0;
        SHOWO_CHECK_HIP(hipMemcpyAsync(last_iv_out, iv + (int64_t)(L - 1) * 4, 16, hipMemcpyDeviceToHost, s));
        if (flag) SHOWO_CHECK_HIP(hipMemcpyAsync(&f, flag, 4, hipMemcpyDeviceToHost, s));
        SHOWO_CHECK_HIP(hipStreamSynchronize(s));
        if (f) return set_error_msg(6, "decode: prompt mask is not interval-representable; KV-cached decode unsupported");
    } else {
        last_iv_out[0] = 0; last_iv_out[1] = L; last_iv_out[2] = 0; last_iv_out[3] = 0;
    }
    set_iv_kernel<<<1, 64, 0, s>>>(e->rows, L - 1, 0, 0, 0);  // rows[0] = L-1
    return head_rows(e, e->rows, 1, 0, e->V, logits_last, s);
}
}  // namespace showo

extern "C" int showo_engine_prefill(showo_engine* e, const int64_t* ids, const float* embeds, const float* mask, int L,
                                    float* logits_last, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    TRY(check_ready(e, 1, L));
    if (e->precision == 1 && !precise_fast_ok(e))
        return set_error_msg(1, "prefill: in accuracy mode the KV-cached decode needs the production-kernel form (showo_engine_precise_fast)");
    TRY(ensure_cache(e, L + 1));
    if (e->precision == 1) TRY(ensure_cache_lo(e));
    const KVDest kv = kv_decode_cache(e);
    ++e->cache_epoch;  // from here on the cache belongs to this prompt (also when the call fails half way)
    TRY(showo::engine_prefill_into(e, ids, embeds, mask, L, kv.k, kv.vt, kv.k_lstride, kv.v_lstride, kv.Lcap, e->last_iv, logits_last, s,
                                   kv.k_lo, kv.vt_lo));
    e->prompt_len = L;
    e->cache_len = L;
    e->cache_precision = e->precision;
    return 0;
}

// a cache prefilled under one precision must not be decoded under another -- precision 1 would attend with zero low halves
// (bf16-grade results while get_precision() says 1), precision 2 would read bf16 keys as fp16
static int check_cache_precision(const showo_engine* e) {
    if (e->cache_precision != e->precision)
        return set_error_msg(1, "decode: the KV cache was prefilled under another precision (showo_engine_set_precision changed since "
                                "showo_engine_prefill): prefill again");
    return 0;
}

extern "C" int showo_engine_decode_step(showo_engine* e, const int64_t* id, const float* embed, float* logits_last, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!e || e->cache_len <= 0) return set_error_msg(1, "decode_step: prefill first");
    TRY(check_cache_precision(e));
    const int P = e->cache_len;  // position of the new token
    if (P + 1 > e->cache_cap || P + 1 > e->cfg.max_pos) return set_error_msg(5, "decode_step: cache full");
    TRY(embed_in(e, id, embed, 1, s));
    // mask row of the new token = last prompt row + [prompt_len, P] (modeling_showo.py:203-217)
    int a = e->last_iv[0], b = e->last_iv[1], c = e->last_iv[2], d = e->last_iv[3];
    const int L0 = e->prompt_len;
    if (b == L0 && a < b) b = P + 1;
    else if (d == L0 && c < d) d = P + 1;
    else if (!(c < d)) { c = L0; d = P + 1; }
    else if (!(a < b)) { a = L0; b = P + 1; }
    else return set_error_msg(6, "decode_step: mask row needs more than two intervals");
    set_iv_kernel<<<1, 64, 0, s>>>(e->iv1, a, b, c, d);
    hipMemsetAsync(e->flag, 0, 4, s);
    if (e->precision == 1) TRY(ensure_cache_lo(e));
    TRY(run_layers(e, 1, 1, P, kv_decode_cache(e), e->iv1, e->flag, nullptr, s));
    e->cache_len = P + 1;
    return head_rows(e, nullptr, 1, 0, e->V, logits_last, s);
}

// ---- mmu sessions: more prompt rows onto a cache (include/showo_hip.h; DESIGN.md, "mmu sessions") -------------------------------------
static int zero_vt_tail(showo_engine* e, bf16_t* vt, bf16_t* vt_lo, int64_t v_lstride, int cap, int c0, int c1, hipStream_t s) {
    if (c1 > cap) c1 = cap;
    if (c1 <= c0) return 0;
    zero_vt_cols_kernel<<<dim3(e->nH * 64, e->nL), 64, 0, s>>>(vt, v_lstride, cap, c0, c1);
    if (vt_lo) zero_vt_cols_kernel<<<dim3(e->nH * 64, e->nL), 64, 0, s>>>(vt_lo, v_lstride, cap, c0, c1);
    SHOWO_CHECK_HIP(hipGetLastError());
    return 0;
}

// Ln rows of ONE sequence at positions P .. P + Ln - 1 of a per-layer K / V^T destination that holds the rows below P (the engine's
// decode cache, or a slot of a decode batch): every row attends as a decode row (last prefill row + causal), K / V^T of the new rows
// land behind the old ones, logits_last = the logits of the last new row.  Ln == 1 is the decode step's layer and head launches behind the tail zeroing.
namespace showo {
int engine_append_into(showo_engine* e, const int64_t* ids, const float* embeds, int Ln, int P, const int* last_iv, int L0, bf16_t* k,
                       bf16_t* vt, int64_t k_lstride, int64_t v_lstride, int cap, float* logits_last, hipStream_t s, bf16_t* k_lo,
                       bf16_t* vt_lo) {
    if (showo_engine_missing(e) != 0) return set_error_msg(4, "engine: weights missing (showo_engine_missing() != 0)");
    if (Ln < 1 || !logits_last) return set_error_msg(1, "prefill_append: needs Ln >= 1 and a logits buffer");
    if (Ln > e->maxT) return set_error_msg(5, "engine: batch/sequence exceeds the configured workspace");
    if (P + Ln + 1 > cap || P + Ln + 1 > e->cfg.max_pos) return set_error_msg(5, "prefill_append: cache full");
    int32_t lv[4] = {last_iv[0], last_iv[1], last_iv[2], last_iv[3]};
    if (!((lv[1] == L0 && lv[0] < lv[1]) || (lv[3] == L0 && lv[2] < lv[3]) || !(lv[2] < lv[3]) || !(lv[0] < lv[1])))
        return set_error_msg(6, "prefill_append: mask row needs more than two intervals");
    TRY(embed_in(e, ids, embeds, Ln, s));
    // the attention of the new rows reads whole 64-key tiles: the V^T columns behind the last new row meet P = 0 and must be finite
    // (decode steps leave them as they found them, engine_prefill_into's comment says what may be there)
    TRY(zero_vt_tail(e, vt, vt_lo, v_lstride, cap, P + Ln, ((P + Ln + 63) / 64) * 64, s));
    const KVDest kv{k, vt, k_lstride, v_lstride, cap, cap, k_lo, vt_lo};
    SHOWO_CHECK_HIP(hipMemsetAsync(e->flag, 0, 4, s));
    if (Ln == 1) {  // showo_engine_decode_step
        int a = lv[0], b = lv[1], c = lv[2], d = lv[3];
        if (b == L0 && a < b) b = P + 1;
        else if (d == L0 && c < d) d = P + 1;
        else if (!(c < d)) { c = L0; d = P + 1; }
        else { a = L0; b = P + 1; }
        set_iv_kernel<<<1, 64, 0, s>>>(e->iv1, a, b, c, d);
        TRY(run_layers(e, 1, 1, P, kv, e->iv1, e->flag, nullptr, s));
        return head_rows(e, nullptr, 1, 0, e->V, logits_last, s);
    }
    TRY(showo_mask_append_rows(lv, L0, P, Ln, e->iv, s));
    TRY(run_layers(e, 1, Ln, P, kv, e->iv, e->flag, nullptr, s));
    set_iv_kernel<<<1, 64, 0, s>>>(e->rows, Ln - 1, 0, 0, 0);  // rows[0] = Ln - 1
    return head_rows(e, e->rows, 1, 0, e->V, logits_last, s);
}
}  // namespace showo

extern "C" int showo_engine_prefill_append(showo_engine* e, const int64_t* ids, const float* embeds, int Ln, float* logits_last,
                                           void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!e || e->cache_len <= 0) return set_error_msg(1, "prefill_append: prefill first");
    TRY(check_cache_precision(e));
    if (e->precision == 1) TRY(ensure_cache_lo(e));
    const KVDest kv = kv_decode_cache(e);
    const int P = e->cache_len;
    TRY(showo::engine_append_into(e, ids, embeds, Ln, P, e->last_iv, e->prompt_len, kv.k, kv.vt, kv.k_lstride, kv.v_lstride, kv.Lcap,
                                  logits_last, s, kv.k_lo, kv.vt_lo));
    e->cache_len = P + Ln;
    return 0;
}

extern "C" int showo_engine_cache_rewind(showo_engine* e, int len, void* stream) {
    if (!e || e->cache_len <= 0) return set_error_msg(1, "cache_rewind: prefill first");
    if (len < e->prompt_len || len > e->cache_len) return set_error_msg(1, "cache_rewind: prompt_len <= len <= cache length required");
    const KVDest kv = kv_decode_cache(e);
    TRY(zero_vt_tail(e, kv.vt, kv.vt_lo, kv.v_lstride, kv.Lcap, len, ((e->cache_len + 63) / 64) * 64, (hipStream_t)stream));
    e->cache_len = len;
    return 0;
}

extern "C" int showo_engine_cache_state(const showo_engine* e, int* cache_len, int* prompt_len, int* cap, int64_t* epoch) {
    if (!e) return set_error_msg(1, "engine: null handle");
    if (cache_len) *cache_len = e->cache_len;
    if (prompt_len) *prompt_len = e->prompt_len;
    if (cap) *cap = e->cache_cap;
    if (epoch) *epoch = e->cache_epoch;
    return 0;
}

extern "C" int showo_engine_cache_ptrs(showo_engine* e, uint16_t** k, uint16_t** vt, int64_t* k_lstride, int64_t* v_lstride) {
    if (!e || !e->kcache) return set_error_msg(1, "cache_ptrs: no decode cache yet (prefill first)");
    const KVDest kv = kv_decode_cache(e);
    if (k) *k = kv.k;
    if (vt) *vt = kv.vt;
    if (k_lstride) *k_lstride = kv.k_lstride;
    if (v_lstride) *v_lstride = kv.v_lstride;
    return 0;
}

// Continuation loop: n_steps times { embed(tok) -> 24 layers against the KV cache -> lm_head -> next token -> tok }, the
// position and the mask row living in device memory so that ONE step can be captured into a hipGraph and replayed.
// tok int64[1] (device): in = the token to feed first, out = the last token produced; out_tokens int64 [n_steps] (device).
// top_k == 1: arg-max (the reference caller's setting); otherwise temperature / top-k / multinomial on the device
// (showo_sample_topk semantics; draw j of this call uses noise row / Philox stream step0 + j); 0 < top_p < 1 puts the nucleus filter
// in front of the draw (showo_sample_topk_topp), top_p >= 1 is the launch of a call without it.
// lps != NULL (showo_engine_decode_sample_lp): one more launch per step, behind the token boundary, scores the token the step stored
// against the step's row in logits_ws (sample_row.h logprob_row) -> lps / ranks [n_steps]; NULL: no launch, the loop of a call without.
// adj != NULL (showo_engine_decode_sample_adj): one adjust launch behind the head reads logits_ws, marks *tok -- the token this step fed,
// the newest member of the set -- and writes adj->ws, which the pick reads; the log-prob launch keeps reading logits_ws.  The greedy
// form then leaves the fused token seam for the arg-max on adj->ws and the separate store / increment launches.  NULL: nothing changes.
// seq != NULL (showo_engine_decode_sample_seq; needs adj): one ban launch directly behind the adjust launch works on adj->ws in place
// and appends *tok to the device history (seq_rules.hip).
static int decode_loop(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, int top_k, float top_p,
                       float temperature, const float* exp_noise, uint64_t seed, int step0, int use_graph, void* stream,
                       float* lps = nullptr, int32_t* ranks = nullptr, const showo::LogitAdjust* adj = nullptr,
                       const showo_seq_rules* seq = nullptr) {
    hipStream_t s = (hipStream_t)stream;
    if (!e || e->cache_len <= 0) return set_error_msg(1, "decode_greedy: prefill first");
    if (!tok || !out_tokens || !logits_ws || n_steps < 1) return set_error_msg(1, "decode_greedy: bad arguments");
    TRY(check_cache_precision(e));
    const int P0 = e->cache_len;
    if (P0 + n_steps > e->cache_cap || P0 + n_steps > e->cfg.max_pos) return set_error_msg(5, "decode_greedy: cache full");
    {   // the decode_step precondition: the mask row must stay a two-interval row
        int a = e->last_iv[0], b = e->last_iv[1], c = e->last_iv[2], d = e->last_iv[3];
        const int L0 = e->prompt_len;
        if (!((b == L0 && a < b) || (d == L0 && c < d) || !(c < d) || !(a < b)))
            return set_error_msg(6, "decode_greedy: mask row needs more than two intervals");
    }
    if (!e->pos_dev) { TRY(e->alloc(&e->pos_dev, 4)); TRY(e->alloc(&e->last_iv_dev, 4)); }
    SHOWO_CHECK_HIP(hipMemcpyAsync(e->pos_dev, &P0, sizeof(int), hipMemcpyHostToDevice, s));
    SHOWO_CHECK_HIP(hipMemcpyAsync(e->last_iv_dev, e->last_iv, 4 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    SHOWO_CHECK_HIP(hipMemsetAsync(e->flag, 0, 4, s));
    SHOWO_CHECK_HIP(hipStreamSynchronize(s));  // P0 / last_iv are host temporaries of this call
    // accuracy mode: the production-kernel layers take the position from the host (no device-side position in those launches), so the
    // steps run eagerly with pos = P0 + i; the token boundary (seam / sampler) keeps pos_dev in step with it
    const bool prec = e->precision == 1;
    if (prec) TRY(ensure_cache_lo(e));
    int step_i = 0;
    if (!prec) showo::attn_set_decode_pos(e->pos_dev, P0 + n_steps);
    // Greedy loop (top_k == 1, the reference caller's setting): the token boundary -- arg-max merge, token store, position increment, next
    // embedding row, next mask row -- is one launch (basic.hip, greedy_token_seam_kernel) at the END of a step, so a step is
    // [layers, lm_head, arg-max partials, boundary] and only the first step embeds its token up front.  SHOWO_DECODE_TOKSEAM=0: the
    // five separate launches.
    static const int tokseam = env_flag("SHOWO_DECODE_TOKSEAM", 1);
    const bool seam_tok = tokseam && top_k == 1 && e->V >= 16384 && !adj;
    auto pre = [&]() -> int {
        TRY(showo_embed_f32(tok, e->embed, e->x, 1, e->H, e->V, s));
        decode_iv_kernel<<<1, 64, 0, s>>>(e->last_iv_dev, e->prompt_len, e->pos_dev, e->iv1);
        return 0;
    };
    auto one = [&]() -> int {
        if (!seam_tok) TRY(pre());
        // host-side P only sizes nothing here (grids depend on L = 1); the kernels read the position from pos_dev
        TRY(run_layers(e, 1, 1, prec ? P0 + step_i : P0, kv_decode_cache(e), e->iv1, e->flag, nullptr, s));
        ++step_i;
        TRY(head_rows(e, nullptr, 1, 0, e->V, logits_ws, s));
        // the token boundary leaves the token in *tok and the position ALREADY advanced: the log-prob launch writes entry pos - 1 - P0
        auto score = [&]() -> int { return lps ? showo::logprob_step_launch(logits_ws, e->V, tok, e->pos_dev, P0, lps, ranks, s) : 0; };
        if (seam_tok) {
            TRY(showo::greedy_token_seam(logits_ws, e->V, tok, out_tokens, e->pos_dev, P0, e->embed, e->x, e->H, e->V, e->last_iv_dev,
                                         e->prompt_len, e->iv1, s));
            return score();
        }
        const float* pick = logits_ws;
        if (adj) {
            TRY(showo::logits_adjust_launch(logits_ws, e->V, 1, e->V, adj->seen, adj->seen_ld, tok, adj->penalty, adj->bias, nullptr, 0, adj->ws,
                                            e->V, s));
            if (seq) TRY(showo::seq_ban_launch(adj->ws, e->V, 1, e->V, seq, tok, nullptr, 0, s));
            pick = adj->ws;
        }
        if (top_k == 1) TRY(showo_argmax_f32(pick, e->V, tok, s));
        else if (top_p >= 1.f) TRY(showo::sample_topk_launch(pick, e->V, top_k, temperature, exp_noise, (int64_t)e->V, seed, step0, e->pos_dev, P0,
                                                             tok, s));
        else TRY(showo::sample_topk_topp_launch(pick, e->V, top_k, top_p, temperature, exp_noise, (int64_t)e->V, seed, step0,
                                                e->pos_dev, P0, tok, s));
        store_token_kernel<<<1, 64, 0, s>>>(tok, out_tokens, e->pos_dev, P0);
        TRY(showo::sampler_step_inc(e->pos_dev, s));
        return score();
    };
    int rc = seam_tok ? pre() : 0;
    if (!rc) rc = showo::replay_steps(one, n_steps, use_graph && !prec, s);
    showo::attn_set_decode_pos(nullptr);
    if (rc) return rc;
    e->cache_len = P0 + n_steps;
    return 0;
}

extern "C" int showo_engine_decode_greedy(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws,
                                          int use_graph, void* stream) {
    return decode_loop(e, tok, n_steps, out_tokens, logits_ws, 1, 1.0f, 1.0f, nullptr, 0, 0, use_graph, stream);
}

extern "C" int showo_engine_decode_sample(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws,
                                          int top_k, float temperature, const float* exp_noise, uint64_t seed, int step0,
                                          int use_graph, void* stream) {
    if (!(temperature > 0.f)) return set_error_msg(1, "decode_sample: temperature must be > 0");
    return decode_loop(e, tok, n_steps, out_tokens, logits_ws, top_k, 1.0f, temperature, exp_noise, seed, step0, use_graph, stream);
}

extern "C" int showo_engine_decode_sample_p(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws,
                                            int top_k, float top_p, float temperature, const float* exp_noise, uint64_t seed,
                                            int step0, int use_graph, void* stream) {
    if (!(temperature > 0.f)) return set_error_msg(1, "decode_sample_p: temperature must be > 0");
    if (!(top_p > 0.f)) return set_error_msg(1, "decode_sample_p: top_p must be > 0 (>= 1: no nucleus filter)");
    return decode_loop(e, tok, n_steps, out_tokens, logits_ws, top_k, top_p, temperature, exp_noise, seed, step0, use_graph, stream);
}

// showo_engine_decode_sample_p that also reports how probable every token was (include/showo_hip.h)
extern "C" int showo_engine_decode_sample_lp(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws,
                                             int top_k, float top_p, float temperature, const float* exp_noise, uint64_t seed,
                                             int step0, float* logprobs, int32_t* ranks, int use_graph, void* stream) {
    if (!(temperature > 0.f)) return set_error_msg(1, "decode_sample_lp: temperature must be > 0");
    if (!(top_p > 0.f)) return set_error_msg(1, "decode_sample_lp: top_p must be > 0 (>= 1: no nucleus filter)");
    return decode_loop(e, tok, n_steps, out_tokens, logits_ws, top_k, top_p, temperature, exp_noise, seed, step0, use_graph, stream,
                       logprobs, logprobs ? ranks : nullptr);
}

// showo_engine_decode_sample_lp with the logit adjustment in front of the pick (include/showo_hip.h, "Logit adjustment")
extern "C" int showo_engine_decode_sample_adj(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, int top_k,
                                              float top_p, float temperature, const float* exp_noise, uint64_t seed, int step0,
                                              float* logprobs, int32_t* ranks, uint32_t* seen, int64_t seen_ld, const float* penalty,
                                              const float* const* bias, float* adj_ws, int use_graph, void* stream) {
    if (!(temperature > 0.f)) return set_error_msg(1, "decode_sample_adj: temperature must be > 0");
    if (!(top_p > 0.f)) return set_error_msg(1, "decode_sample_adj: top_p must be > 0 (>= 1: no nucleus filter)");
    if (!e || !adj_ws || adj_ws == logits_ws) return set_error_msg(1, "decode_sample_adj: needs an adj_ws [V] of its own");
    TRY(showo::logits_adjust_check(1, e->V, seen, seen_ld, penalty, "decode_sample_adj"));
    const showo::LogitAdjust adj{seen, seen_ld, penalty, bias, adj_ws};
    return decode_loop(e, tok, n_steps, out_tokens, logits_ws, top_k, top_p, temperature, exp_noise, seed, step0, use_graph, stream,
                       logprobs, logprobs ? ranks : nullptr, &adj);
}

// showo_engine_decode_sample_adj with the sequence rules behind the adjustment (include/showo_hip.h, "Sequence rules")
extern "C" int showo_engine_decode_sample_seq(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, int top_k,
                                              float top_p, float temperature, const float* exp_noise, uint64_t seed, int step0,
                                              float* logprobs, int32_t* ranks, uint32_t* seen, int64_t seen_ld, const float* penalty,
                                              const float* const* bias, float* adj_ws, const showo_seq_rules* rules, int use_graph,
                                              void* stream) {
    if (!(temperature > 0.f)) return set_error_msg(1, "decode_sample_seq: temperature must be > 0");
    if (!(top_p > 0.f)) return set_error_msg(1, "decode_sample_seq: top_p must be > 0 (>= 1: no nucleus filter)");
    if (!e || !adj_ws || adj_ws == logits_ws) return set_error_msg(1, "decode_sample_seq: needs an adj_ws [V] of its own");
    TRY(showo::logits_adjust_check(1, e->V, seen, seen_ld, penalty, "decode_sample_seq"));
    TRY(showo::seq_rules_check(1, rules, "decode_sample_seq"));
    const showo::LogitAdjust adj{seen, seen_ld, penalty, bias, adj_ws};
    return decode_loop(e, tok, n_steps, out_tokens, logits_ws, top_k, top_p, temperature, exp_noise, seed, step0, use_graph, stream,
                       logprobs, logprobs ? ranks : nullptr, &adj, rules);
}
