// Training step of the Show-o transformer on gfx950: forward with saved activations, the three cross-entropies of
// Showo.forward and the full backward into fp32 gradient buffers that carry the reference's state-dict names.
// Replaces (reference): Showo.forward with labels (models/modeling_showo.py:59-102) + loss.backward()
// (training/train.py:590-612) for the Phi stack (models/phi.py:774-790, 953-1183).
//
// GEMM forms (all on the one NT kernel C = A W^T, K-contiguous operands):
//   forward   Y[T,N]   = X[T,K]     W[N,K]^T
//   dgrad     dX[T,K]  = dY[T,N]    (W^T)[K,N]^T        -> needs the transposed weight copy W^T (made at load time)
//   wgrad     dW[N,K]  = (dY^T)[N,Tp] (X^T)[K,Tp]^T     -> needs token-contiguous images of dY and X
//             (showo_transpose_bf16; the bias gradient = column sums of dY comes out of the same pass)
// Saved per layer: x (fp32 block input), h = LN(x), raw qkv, Q, K, V^T, lse, attention output, fc1 pre-activation.
#include "engine.h"
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <map>
#include <set>

using namespace showo;

#define TRY(expr)            \
    do {                     \
        int _rc = (expr);    \
        if (_rc) return _rc; \
    } while (0)

namespace {
struct LayerT {
    bf16_t *wqkvT = nullptr, *wdT = nullptr, *w1T = nullptr, *w2T = nullptr;  // [K_in, N_out] images for dgrad
    // saved activations
    float* x = nullptr;
    bf16_t *h = nullptr, *qkv = nullptr, *Q = nullptr, *K = nullptr, *Vt = nullptr, *attn = nullptr, *f = nullptr;
    bf16_t* a = nullptr;  // gelu_new(f) [T, F]: the token-major operand of the fc2 weight gradient (showo_gemm_tn_bf16)
    float* lse = nullptr;
    // gradients (fp32, reference parameter layout)
    float *gwqkv = nullptr, *gbqkv = nullptr, *gwd = nullptr, *gbd = nullptr, *gw1 = nullptr, *gb1 = nullptr, *gw2 = nullptr, *gb2 = nullptr;
    float *gln = nullptr;   // [2,H] (weight, bias)
    float* gqk = nullptr;   // [4,64] (q_ln w, b, k_ln w, b)
    uint64_t tv[4] = {0, 0, 0, 0};  // engine versions (Layer::ver) the transposed images wqkvT, wdT, w1T, w2T were made from
};
struct Grad { float* p; int64_t n; };
// which of a block's gradients the backward writes (showo_train_set_trainable): a group flag is on when any of its tensors trains
struct LayerPlan {
    bool wqkv = true, bqkv = true, wd = true, bd = true, w1 = true, b1 = true, w2 = true, b2 = true, ln = true, qk = true;
    bool any = true;
    std::vector<Grad> clear;  // frozen members of a group that one launch writes whole (q/k/v, LayerNorm pairs): cleared after it
};
struct Bound { std::string key; float *p, *m, *v; int64_t n; bool decay; float* s = nullptr; };  // s: EMA shadow (showo_train_bind_ema)

// SHOWO_TRAIN_TN (default 1): weight gradients by showo_gemm_tn_bf16 on the token-major tensors the backward already holds (dY, and the
// activations saved by the forward) + showo_colsum_bf16 for the bias gradients; 0 = transpose both operands and run the k-contiguous
// GEMM (the round-2 path: 243 transposes per step).  Read once per process: the per-layer gelu(fc1) buffers exist only in TN mode.
bool train_tn() {
    static const bool v = env_flag("SHOWO_TRAIN_TN", true);
    return v;
}
// the batch split a forward was called with: its cross-entropy tables (and an announced d(logits)) serve a backward with the same one only
struct Split {
    int b_t2i = 0, b_lm = 0, b_mmu = 0, max_seq_len = 0;
    bool operator==(const Split& o) const { return b_t2i == o.b_t2i && b_lm == o.b_lm && b_mmu == o.b_mmu && max_seq_len == o.max_seq_len; }
};
}  // namespace

struct showo_trainer {
    showo_engine* e;
    int maxB, maxL, Tmax, Tp, Lp, Vp;
    std::vector<void*> allocs;
    std::vector<LayerT> L;
    bf16_t* wlmT = nullptr;
    std::map<std::string, Grad> grads;
    std::vector<Bound> bound;  // master weights + AdamW moments registered by the host (showo_train_bind_param)
    showo::AdamSeg* adam_segs = nullptr;  // device tables of the multi-tensor optimizer launch (train_kernels.hip, adamw_multi_kernel)
    int* adam_seg_of = nullptr;
    int64_t* adam_start_of = nullptr;
    int adam_chunks = 0;
    bool adam_dirty = true;
    std::vector<std::pair<std::string, uint64_t*>> adam_keys;  // tensors the table updates + their engine version stamps
    // EMA of the weights (ema.hip): shadows bound per key, 1 - decay announced for the next optimizer step (negative: none), and two
    // tables rebuilt under the rule of adam_dirty -- every shadowed tensor with its engine destination (the swap), and the trainable
    // ones alone (the table update behind the per-tensor AdamW of SHOWO_TRAIN_ADAMW_MULTI=0)
    bool adam_shadowed = false;  // every segment of the AdamW table carries a shadow
    float ema_omd = -1.f;
    bool ema_dirty = true;
    showo::EmaTable ema_all, ema_trainable;
    std::vector<std::pair<std::string, uint64_t*>> ema_keys;  // tensors of ema_all + their engine version stamps
    // head
    float *logits = nullptr, *gembed = nullptr, *gfln = nullptr, *gwlm = nullptr, *gblm = nullptr;
    bf16_t *dlogits = nullptr, *bigT = nullptr;  // bigT: [max(Vp, F, 3H), Tp] transposed image of the dY side (SHOWO_TRAIN_TN=0 only)
    // backward scratch
    float *dy = nullptr, *dh = nullptr, *colpart = nullptr, *lnpart = nullptr, *qkpart = nullptr, *D = nullptr, *rowloss = nullptr;
    bf16_t *dy16 = nullptr, *d_o = nullptr, *dff = nullptr, *dqk = nullptr, *dqkv = nullptr, *xT = nullptr, *QT = nullptr, *KT = nullptr, *dOT = nullptr;
    void* ce_rows = nullptr;
    int* counts = nullptr;
    int* order_ws = nullptr;
    float* losses = nullptr;
    int64_t* ids = nullptr;
    // state of the last forward
    int B = 0, Lq = 0;
    bool have_fwd = false;
    Split split;  // of the last forward
    uint64_t generation = 0;  // training forwards started (showo_train_generation)
    bool has_mask = false;
    bool from_embeds = false;  // last forward started from caller-provided embeddings: d(loss)/d(embeddings) = dy
    // last forward spliced the projector's rows into layer 0's input (showo_train_forward_spliced): the last sp_n sequences hold sp_P
    // placeholder columns from start[j]; the table scatter leaves them out and showo_train_image_grad compacts their rows of dy
    bool spliced = false;
    int sp_n = 0, sp_P = 0;
    int32_t* start = nullptr;
    uint64_t tv_wlm = 0;  // engine version of lm_head.weight that wlmT was made from
    // trainable set (showo_train_set_trainable): state-dict keys whose gradients are not wanted; their slots read as zeros
    std::set<std::string> frozen, pending_zero;
    bool want_input = true;  // d(loss)/d(input embeddings) is wanted (showo_train_set_input_grad)
    bool plan_dirty = true;
    std::vector<LayerPlan> plan;
    std::vector<char> any_below;  // any_below[i]: some block j < i trains
    bool p_emb = true, p_fln = true, p_wlm = true, p_blm = true;
    std::vector<Grad> fln_clear;
    bool gembed_dirty = false;  // gembed holds a scatter of an earlier backward (the next one that does not scatter clears it)
    float *sc_ln = nullptr, *sc_b = nullptr, *sc_b1 = nullptr, *sc_qk = nullptr;  // side outputs of fused launches for frozen tensors
    int64_t cnt[5] = {0, 0, 0, 0, 0};  // showo_train_counters
    // loss weights announced before the forward (showo_train_set_loss_weights): the forward's cross-entropy pass then writes the
    // logit gradients as well, and a backward with the same labels / split / weights skips its own pass over the 2.6 GB of logits
    bool lw_set = false;
    float lw[3] = {0.f, 0.f, 0.f};
    bool dl_valid = false;
    float dl_g[3] = {0.f, 0.f, 0.f};
    const int64_t* dl_labels = nullptr;
    // gradient accumulation (showo_train_set_accumulate): every parameter-gradient write of the backward adds into the flat buffer
    bool accumulate = false;
    // loss head on the labelled rows only (showo_train_set_loss_rows): the census of a forward with labels is an ordered compaction,
    // its row count comes back through a pinned int (the one host wait of the mode) and the head runs on the compact rows
    int loss_rows = 0;       // the mode the NEXT forward takes (0 = all rows)
    bool compact = false;    // the LAST forward ran the compact head: logits / dlogits / hf / dh hold Tc rows in row_index order
    int Tc = 0;              // its labelled rows (the backward must be asked for the forward's batch split)
    int *row_index = nullptr, *row_slot = nullptr, *scan_ws = nullptr;
    void* ce_rows_c = nullptr;
    int32_t* tc_host = nullptr;
    hipEvent_t ev_tc = nullptr;

    template <class T>
    int alloc(T** p, int64_t n) {
        void* q = nullptr;
        hipError_t err = hipMalloc(&q, (size_t)(n > 0 ? n : 1) * sizeof(T));
        if (err != hipSuccess) return set_error_hip(err, "hipMalloc(trainer)", __FILE__, __LINE__);
        allocs.push_back(q);
        *p = (T*)q;
        return 0;
    }
    // gradients live in ONE flat fp32 buffer (bucket = contiguous range: embed | layer 0 .. nL-1 | head), so a data-parallel
    // job all-reduces a bucket with one collective while the backward of the next block runs
    float* gflat = nullptr;
    int64_t gflat_n = 0, gcursor = 0;
    std::vector<std::pair<int64_t, int64_t>> buckets;  // (offset, count)
    float* carve(int64_t n) {
        n = (n + 63) & ~(int64_t)63;  // keep every tensor 256-B aligned
        float* p = gflat + gcursor;
        gcursor += n;
        return p;
    }
    int galloc(const std::string& key, float** p, int64_t n) {
        *p = carve(n);
        grads[key] = Grad{*p, n};
        return 0;
    }
};

extern "C" int showo_train_create(showo_engine* e, int max_batch, int max_seq, showo_trainer** out) {
    if (!e || !out) return set_error_msg(1, "train_create: null argument");
    if (max_batch > e->cfg.max_batch || max_seq > e->cfg.max_seq || (int64_t)max_batch * max_seq > e->maxT)
        return set_error_msg(5, "train_create: the engine workspace is smaller than the training batch");
    if (e->cfg.rotary_dim != 32) return set_error_msg(1, "train: rotary_dim 32 only");
    if (e->H % 64 || e->H > 2048) return set_error_msg(1, "train: hidden must be a multiple of 64 and <= 2048");
    showo_trainer* t = new showo_trainer();
    t->e = e;
    t->maxB = max_batch; t->maxL = max_seq;
    t->Tmax = max_batch * max_seq;
    t->Tp = ((t->Tmax + 63) / 64) * 64;
    t->Lp = ((max_seq + 63) / 64) * 64;
    t->Vp = ((e->V + 255) / 256) * 256;  // whole 256-column tiles: the lm_head weight gradient (gemm_tn.hip) fetches its dY columns unchecked
    const int64_t H = e->H, F = e->F, V = e->V, T = t->Tmax, Tp = t->Tp, Vp = t->Vp, nH = e->nH;
    int rc = 0;
    t->L.resize(e->nL);
    char key[160];
    {
        auto al = [](int64_t n) { return (n + 63) & ~(int64_t)63; };
        const int64_t per_layer = al(3 * H * H) + al(3 * H) + al(H * H) + al(H) + al(F * H) + al(F) + al(H * F) + al(H) + al(2 * H) + al(256);
        t->gflat_n = al(V * H) + e->nL * per_layer + al(2 * H) + al(V * H) + al(Vp);
        rc |= t->alloc(&t->gflat, t->gflat_n);
        if (rc) { showo_train_destroy(t); return rc; }
        hipMemset(t->gflat, 0, (size_t)t->gflat_n * sizeof(float));
    }
    { int64_t c0 = t->gcursor; t->galloc("showo.model.embed_tokens.weight", &t->gembed, V * H); t->buckets.push_back({c0, t->gcursor - c0}); }
    for (int i = 0; i < e->nL; ++i) {
        LayerT& l = t->L[i];
        rc |= t->alloc(&l.wqkvT, H * 3 * H); rc |= t->alloc(&l.wdT, H * H); rc |= t->alloc(&l.w1T, H * F); rc |= t->alloc(&l.w2T, F * H);
        // token-major operands of showo_gemm_tn_bf16 (h, attn, a; dy16 / dff / dqkv / dlogits below) are allocated with Tp rows: the
        // kernel reads -- and zeroes in registers -- the rows between T and the next multiple of 64
        rc |= t->alloc(&l.x, T * H); rc |= t->alloc(&l.h, Tp * H); rc |= t->alloc(&l.qkv, T * 3 * H);
        rc |= t->alloc(&l.Q, T * H); rc |= t->alloc(&l.K, T * H); rc |= t->alloc(&l.Vt, (int64_t)max_batch * H * t->Lp);
        rc |= t->alloc(&l.attn, Tp * H); rc |= t->alloc(&l.f, T * F); rc |= t->alloc(&l.lse, (int64_t)max_batch * nH * max_seq);
        if (train_tn()) rc |= t->alloc(&l.a, Tp * F);
        if (rc) break;
        hipMemset(l.Vt, 0, (size_t)max_batch * H * t->Lp * sizeof(bf16_t));
        const char* names[3] = {"q_proj", "k_proj", "v_proj"};
        const int64_t lc0 = t->gcursor;
        l.gwqkv = t->carve(3 * H * H); l.gbqkv = t->carve(3 * H);
        for (int j = 0; j < 3 && !rc; ++j) {
            snprintf(key, sizeof key, "showo.model.layers.%d.self_attn.%s.weight", i, names[j]);
            t->grads[key] = Grad{l.gwqkv + j * H * H, H * H};
            snprintf(key, sizeof key, "showo.model.layers.%d.self_attn.%s.bias", i, names[j]);
            t->grads[key] = Grad{l.gbqkv + j * H, H};
        }
        snprintf(key, sizeof key, "showo.model.layers.%d.self_attn.dense.weight", i); rc |= t->galloc(key, &l.gwd, H * H);
        snprintf(key, sizeof key, "showo.model.layers.%d.self_attn.dense.bias", i); rc |= t->galloc(key, &l.gbd, H);
        snprintf(key, sizeof key, "showo.model.layers.%d.mlp.fc1.weight", i); rc |= t->galloc(key, &l.gw1, F * H);
        snprintf(key, sizeof key, "showo.model.layers.%d.mlp.fc1.bias", i); rc |= t->galloc(key, &l.gb1, F);
        snprintf(key, sizeof key, "showo.model.layers.%d.mlp.fc2.weight", i); rc |= t->galloc(key, &l.gw2, H * F);
        snprintf(key, sizeof key, "showo.model.layers.%d.mlp.fc2.bias", i); rc |= t->galloc(key, &l.gb2, H);
        l.gln = t->carve(2 * H);
        l.gqk = t->carve(256);
        t->buckets.push_back({lc0, t->gcursor - lc0});
        snprintf(key, sizeof key, "showo.model.layers.%d.input_layernorm.weight", i); t->grads[key] = Grad{l.gln, H};
        snprintf(key, sizeof key, "showo.model.layers.%d.input_layernorm.bias", i); t->grads[key] = Grad{l.gln + H, H};
        const char* qk[4] = {"q_layernorm.weight", "q_layernorm.bias", "k_layernorm.weight", "k_layernorm.bias"};
        for (int j = 0; j < 4; ++j) {
            snprintf(key, sizeof key, "showo.model.layers.%d.self_attn.%s", i, qk[j]);
            t->grads[key] = Grad{l.gqk + 64 * j, 64};
        }
    }
    rc |= t->alloc(&t->wlmT, H * Vp);
    const int64_t hc0 = t->gcursor;
    t->gfln = t->carve(2 * H);
    t->galloc("showo.lm_head.weight", &t->gwlm, V * H);
    t->galloc("showo.lm_head.bias", &t->gblm, Vp);
    t->buckets.push_back({hc0, t->gcursor - hc0});
    if (!rc) {
        t->grads["showo.lm_head.bias"].n = V;
        t->grads["showo.model.final_layernorm.weight"] = Grad{t->gfln, H};
        t->grads["showo.model.final_layernorm.bias"] = Grad{t->gfln + H, H};
    }
    rc |= t->alloc(&t->logits, T * V);
    rc |= t->alloc(&t->dlogits, Tp * Vp);
    // bigT holds the transposed dY side of every wgrad GEMM: dlogits^T [Vp, Tp], df^T [F, Tp], dqkv^T [3H, Tp] -- the tallest wins
    // (round 3: sizing it by max(Vp, F) alone overflowed for geometries with 3H > max(Vp, F), found by the SMALL training fixture)
    const int64_t bigrows = std::max<int64_t>(std::max<int64_t>(Vp, F), 3 * H);
    if (!train_tn()) {  // the transposed operand images exist only on the transpose + NT path (1.5 GB at the stage-1 geometry)
        rc |= t->alloc(&t->bigT, bigrows * Tp);
        rc |= t->alloc(&t->xT, std::max<int64_t>(F, H) * Tp);
    }
    rc |= t->alloc(&t->dy, T * H); rc |= t->alloc(&t->dh, T * H); rc |= t->alloc(&t->dy16, Tp * H); rc |= t->alloc(&t->d_o, T * H);
    rc |= t->alloc(&t->dff, Tp * F); rc |= t->alloc(&t->dqk, T * 2 * H); rc |= t->alloc(&t->dqkv, Tp * 3 * H);
    rc |= t->alloc(&t->QT, (int64_t)max_batch * H * t->Lp); rc |= t->alloc(&t->KT, (int64_t)max_batch * H * t->Lp);
    rc |= t->alloc(&t->dOT, (int64_t)max_batch * H * t->Lp);
    rc |= t->alloc(&t->D, (int64_t)max_batch * nH * max_seq);
    rc |= t->alloc(&t->colpart, (Tp / 32 + 8) * bigrows);  // showo_colsum_bf16 writes one partial row per 32 tokens
    rc |= t->alloc(&t->lnpart, (int64_t)showo_ln_bwd_blocks((int)T) * 3 * H);
    rc |= t->alloc(&t->qkpart, (int64_t)showo_qkln_rope_bwd_blocks((int)T, (int)nH) * 256);
    rc |= t->alloc(&t->rowloss, 2 * T);
    rc |= t->alloc(&t->sc_ln, 2 * H); rc |= t->alloc(&t->sc_b, H); rc |= t->alloc(&t->sc_b1, F); rc |= t->alloc(&t->sc_qk, 256);
    rc |= t->alloc((char**)&t->ce_rows, 12 * T);
    rc |= t->alloc(&t->counts, 4);  // the three valid-label counts + the labelled rows of the compact census
    rc |= t->alloc((char**)&t->ce_rows_c, 12 * T);
    rc |= t->alloc(&t->row_index, T); rc |= t->alloc(&t->row_slot, T); rc |= t->alloc(&t->scan_ws, showo_ce_rows_compact_ws((int)T));
    rc |= t->alloc(&t->order_ws, 2 * T);
    rc |= t->alloc(&t->losses, 4);
    rc |= t->alloc(&t->ids, T);
    rc |= t->alloc(&t->start, max_batch);
    // the ranking of the leave-out scatter fills order_ws for the live tokens only: whatever else a launch could read is a row index
    if (!rc && hipMemset(t->order_ws, 0, (size_t)2 * T * sizeof(int)) != hipSuccess) rc = set_error_msg(7, "train_create: hipMemset failed");
    if (rc) { showo_train_destroy(t); return rc; }
    *out = t;
    return 0;
}

extern "C" void showo_train_destroy(showo_trainer* t) {
    if (!t) return;
    for (void* p : t->allocs) hipFree(p);
    if (t->adam_segs) { hipFree(t->adam_segs); hipFree(t->adam_seg_of); hipFree(t->adam_start_of); }
    t->ema_all.release();
    t->ema_trainable.release();
    if (t->ev_tc) hipEventDestroy(t->ev_tc);
    if (t->tc_host) hipHostFree(t->tc_host);
    delete t;
}

extern "C" int showo_train_invalidate_weights(showo_trainer* t) {
    if (!t) return set_error_msg(1, "train: null handle");
    for (auto& l : t->L) std::fill(l.tv, l.tv + 4, 0);
    t->tv_wlm = 0;
    return 0;
}

// transposed bf16 weight images for the dgrad GEMMs: rebuilt for the tensors whose engine image changed since they were made
// (engine versions, Layer::ver: showo_engine_load and the fused AdamW stamp every write)
static int sync_weights(showo_trainer* t, hipStream_t s) {
    showo_engine* e = t->e;
    const int H = e->H, F = e->F, V = e->V;
    for (int i = 0; i < e->nL; ++i) {
        Layer& w = e->layers[i];
        LayerT& l = t->L[i];
        const bool st[4] = {l.tv[0] < w.ver[0], l.tv[1] < w.ver[1], l.tv[2] < w.ver[2], l.tv[3] < w.ver[3]};
        if (st[0]) TRY(showo_transpose_bf16(w.wqkv, H, l.wqkvT, 3 * H, H, 3 * H, 0, nullptr, nullptr, 0, s));  // [3H,H] -> [H,3H]
        if (st[1]) TRY(showo_transpose_bf16(w.wd, H, l.wdT, H, H, H, 0, nullptr, nullptr, 0, s));
        if (st[2]) TRY(showo_transpose_bf16(w.w1, H, l.w1T, F, H, F, 0, nullptr, nullptr, 0, s));                // [F,H] -> [H,F]
        if (st[3]) TRY(showo_transpose_bf16(w.w2, F, l.w2T, H, F, H, 0, nullptr, nullptr, 0, s));                // [H,F] -> [F,H]
        for (int k = 0; k < 4; ++k)
            if (st[k]) { l.tv[k] = w.ver[k]; ++t->cnt[4]; }
    }
    if (t->tv_wlm < e->ver_wlm) {
        TRY(showo_transpose_bf16(e->wlm, H, t->wlmT, V, H, t->Vp, 0, nullptr, nullptr, 0, s));        // [V,H] -> [H,Vp]
        t->tv_wlm = e->ver_wlm;
        ++t->cnt[4];
    }
    return 0;
}

// ---- trainable set
// (Re)derive the per-block plan from the frozen keys, and clear the gradient slots of tensors frozen since the last call: a frozen
// tensor's slot is zeroed ONCE and never written again, so the flat buffer's norm is the norm over the trainable tensors.
static int plan_sync(showo_trainer* t, hipStream_t s) {
    for (const std::string& k : t->pending_zero) {
        const Grad& g = t->grads[k];
        SHOWO_CHECK_HIP(hipMemsetAsync(g.p, 0, (size_t)g.n * sizeof(float), s));
        if (k == "showo.model.embed_tokens.weight") t->gembed_dirty = false;
    }
    t->pending_zero.clear();
    if (!t->plan_dirty) return 0;
    const int nL = t->e->nL;
    auto on = [&](const std::string& k) { return t->frozen.count(k) == 0; };
    // group flag = any member trains; members that do not are cleared after the group's launch (LayerPlan::clear)
    auto group = [&](const std::vector<std::string>& keys, std::vector<Grad>& clear) {
        bool any = false;
        for (auto& k : keys) any = any || on(k);
        if (any)
            for (auto& k : keys)
                if (!on(k)) clear.push_back(t->grads[k]);
        return any;
    };
    t->plan.assign(nL, LayerPlan());
    t->any_below.assign(nL + 1, 0);
    for (int i = 0; i < nL; ++i) {
        LayerPlan& p = t->plan[i];
        const std::string pre = "showo.model.layers." + std::to_string(i) + ".";
        const std::string a = pre + "self_attn.";
        p.wqkv = group({a + "q_proj.weight", a + "k_proj.weight", a + "v_proj.weight"}, p.clear);
        p.bqkv = group({a + "q_proj.bias", a + "k_proj.bias", a + "v_proj.bias"}, p.clear);
        p.ln = group({pre + "input_layernorm.weight", pre + "input_layernorm.bias"}, p.clear);
        p.qk = group({a + "q_layernorm.weight", a + "q_layernorm.bias", a + "k_layernorm.weight", a + "k_layernorm.bias"}, p.clear);
        p.wd = on(a + "dense.weight"); p.bd = on(a + "dense.bias");
        p.w1 = on(pre + "mlp.fc1.weight"); p.b1 = on(pre + "mlp.fc1.bias");
        p.w2 = on(pre + "mlp.fc2.weight"); p.b2 = on(pre + "mlp.fc2.bias");
        p.any = p.wqkv || p.bqkv || p.ln || p.qk || p.wd || p.bd || p.w1 || p.b1 || p.w2 || p.b2;
        t->any_below[i + 1] = t->any_below[i] || p.any;
    }
    t->fln_clear.clear();
    t->p_fln = group({"showo.model.final_layernorm.weight", "showo.model.final_layernorm.bias"}, t->fln_clear);
    t->p_wlm = on("showo.lm_head.weight");
    t->p_blm = on("showo.lm_head.bias");
    t->p_emb = on("showo.model.embed_tokens.weight");
    t->plan_dirty = false;
    return 0;
}

// d(loss)/d(input of block i) is consumed below it: by a lower block, the embedding table (ids flow) or the caller (embeddings flow)
static bool below_needs(const showo_trainer* t, int i) {
    if (t->spliced && t->want_input && t->sp_n * t->sp_P > 0) return true;  // the projector consumes the placeholder rows of dy
    return (t->from_embeds ? t->want_input : t->p_emb) || t->any_below[i];
}

// where the column sums of block i's residual-stream gradient (= the dense and fc2 bias gradients) go: fc2's slot, else dense's, else nowhere
static float* b2_dst(showo_trainer* t, int i) {
    const LayerPlan& p = t->plan[i];
    return p.b2 ? t->L[i].gb2 : p.bd ? t->L[i].gbd : nullptr;
}

extern "C" int showo_train_set_trainable(showo_trainer* t, const char* key, int on) {
    if (!t || !key) return set_error_msg(1, "train_set_trainable: null argument");
    std::string k(key);
    if (!t->grads.count(k)) return set_error_msg(3, "train_set_trainable: unknown state-dict key");
    const bool was = t->frozen.count(k) == 0;
    if (was == (on != 0)) return 0;
    if (on) { t->frozen.erase(k); t->pending_zero.erase(k); }
    else { t->frozen.insert(k); t->pending_zero.insert(k); }
    t->plan_dirty = true;
    t->adam_dirty = true;
    t->ema_dirty = true;
    return 0;
}

extern "C" int showo_train_set_input_grad(showo_trainer* t, int on) {
    if (!t) return set_error_msg(1, "train_set_input_grad: null handle");
    t->want_input = on != 0;
    return 0;
}

extern "C" int showo_train_set_accumulate(showo_trainer* t, int on) {
    if (!t) return set_error_msg(1, "train_set_accumulate: null handle");
    t->accumulate = on != 0;
    return 0;
}

// Loss head on the labelled rows only.  mode 1: a forward with labels runs the final LayerNorm, the lm_head GEMM and the cross-entropy
// on the rows that carry a label (ordered compaction, showo_ce_rows_compact), and the head backward contracts over those rows; the
// full logits are not materialised.  Per call, like the accumulate switch: the module's autograd path shares this trainer.
extern "C" int showo_train_set_loss_rows(showo_trainer* t, int mode) {
    if (!t) return set_error_msg(1, "train_set_loss_rows: null handle");
    if (mode != 0 && mode != 1) return set_error_msg(1, "train_set_loss_rows: mode must be 0 (all rows) or 1 (labelled rows)");
    t->loss_rows = mode;
    return 0;
}
// (rows the head of the last forward ran on, rows of its batch): the host ints of the forward's one wait, no synchronisation here
extern "C" int showo_train_loss_rows(showo_trainer* t, int* rows, int* total) {
    if (!t || !rows || !total) return set_error_msg(1, "train_loss_rows: null argument");
    if (!t->have_fwd) return set_error_msg(1, "train_loss_rows: run showo_train_forward first");
    *total = t->B * t->Lq;
    *rows = t->compact ? t->Tc : *total;
    return 0;
}

extern "C" int showo_train_counters(showo_trainer* t, int64_t* out6, int reset) {
    if (!t) return set_error_msg(1, "train_counters: null handle");
    if (out6) {
        for (int k = 0; k < 5; ++k) out6[k] = t->cnt[k];
        out6[5] = t->e->fused_rebuilt;
    }
    if (reset) { std::fill(t->cnt, t->cnt + 5, 0); t->e->fused_rebuilt = 0; }
    return 0;
}

// Visibility intervals built on the device (showo_mask_predict_next / _mmu) instead of a dense mask: the next
// showo_train_forward call that passes mask == NULL attends (forward and backward) with iv int32 [B,L,4]; NULL restores causal.
// flag (optional, int32[1] written by the interval builders): non-zero = some row needs more than two visibility runs, the
// intervals do not describe the mask; checked on the device, without a host sync: the three losses come back as NaN.
extern "C" int showo_trainer_use_intervals(showo_trainer* t, const int32_t* iv, const int32_t* flag) {
    if (!t) return set_error_msg(1, "trainer: null handle");
    t->e->ext_iv = iv;
    t->e->ext_flag = iv ? flag : nullptr;
    return 0;
}

namespace {
__global__ void poison_losses_kernel(float* __restrict__ losses, const int32_t* __restrict__ flag) {
    if (threadIdx.x < 3 && *flag != 0) losses[threadIdx.x] = __builtin_nanf("");
}
// Row count of the compact head's GEMM launches (lm_head forward, dgrad): Tc rounded up to 256, at most T.  The labelled-row count
// changes with every batch (the t2i masking rate is drawn per step) and the GEMM dispatch times its tile candidates once per distinct
// (M, N, K): rounding bounds the shapes a run meets by T / 256.  The rows between Tc and the rounded count hold stale operands; a GEMM
// row depends on its own operand row only, and nothing reads those output rows.
int compact_gemm_rows(int Tc, int T) { return std::min(T, ((Tc + 255) / 256) * 256); }
}  // namespace

// the spliced rows of a forward (showo_train_forward_spliced); rows == nullptr: a plain ids / embeds forward
struct Splice { const float* rows = nullptr; const int32_t* start = nullptr; int n = 0, P = 0; };

static int train_forward_impl(showo_trainer* t, const int64_t* ids, const float* embeds, const float* mask, const int64_t* labels,
                              int B, int L, int b_t2i, int b_lm, int b_mmu, int max_seq_len, float* logits_out, float* losses_out,
                              void* stream, const Splice* sp = nullptr) {
    hipStream_t s = (hipStream_t)stream;
    if (!t || ((ids == nullptr) == (embeds == nullptr))) return set_error_msg(1, "train_forward: exactly one of ids / embeds");
    // a refused spliced call leaves the trainer as the last forward left it: checked before anything is counted or queued
    if (sp && (!ids || sp->n < 0 || sp->n > B || sp->P < 0 || sp->P > L || (sp->n * sp->P > 0 && (!sp->rows || !sp->start))))
        return set_error_msg(1, "train_forward_spliced: need ids, 0 <= n <= B, 0 <= P <= L, and rows + start when n * P > 0");
    ++t->generation;
    showo_engine* e = t->e;
    if (showo_engine_missing(e) != 0) return set_error_msg(4, "train: weights missing");
    const bool compact = t->loss_rows == 1 && labels != nullptr;
    if (compact && logits_out)
        return set_error_msg(1, "train_forward: loss rows = labelled (showo_train_set_loss_rows 1) does not materialise the [B*L, V] logits; "
                                "pass logits_out = NULL, or set mode 0 for a forward that returns them");
    if (compact) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        hipStreamIsCapturing(s, &cs);
        if (cs != hipStreamCaptureStatusNone)
            return set_error_msg(7, "train_forward: loss rows = labelled waits on the host for the row count; not inside a stream capture");
    }
    if (B > t->maxB || L > t->maxL || (int64_t)B * L > t->Tmax) return set_error_msg(5, "train: batch exceeds the trainer workspace");
    if ((e->H % 64) || (e->F % 64)) return set_error_msg(1, "train: hidden/ffn must be multiples of 64");
    if (e->img_f16 || e->precision == 2)
        return set_error_msg(4, "train: the engine's weight images hold fp16 (precision 2); training runs on bf16 images -- "
                                "showo_engine_set_precision(e, 0) and upload the weights again");
    if (e->precision == 3)
        return set_error_msg(4, "train: the engine's weight images hold the int8-dequantised weights (precision 3); training runs on the "
                                "bf16 images of the masters -- showo_engine_set_precision(e, 0) and upload the weights again");
    TRY(sync_weights(t, s));
    TRY(plan_sync(t, s));
    const int H = e->H, F = e->F, V = e->V, nH = e->nH, T = B * L;
    const int Lp = ((L + 63) / 64) * 64;
    if (compact) {
        // the row census first: its count is on its way to the host while the blocks are queued, and the wait below (before the head)
        // is on this event only -- the stream keeps its queue
        if (!t->tc_host) {
            SHOWO_CHECK_HIP(hipHostMalloc((void**)&t->tc_host, 64, hipHostMallocDefault));
            SHOWO_CHECK_HIP(hipEventCreateWithFlags(&t->ev_tc, hipEventDisableTiming));
        }
        TRY(showo_ce_rows_compact(labels, B, L, b_t2i, b_lm, b_mmu, max_seq_len, t->ce_rows, t->ce_rows_c, t->counts, t->row_index, t->row_slot,
                                  t->counts + 3, t->scan_ws, s));
        SHOWO_CHECK_HIP(hipMemcpyAsync(t->tc_host, t->counts + 3, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        SHOWO_CHECK_HIP(hipEventRecord(t->ev_tc, s));
    }
    if (sp) {  // table rows and the projector's rows in one launch; ids and start stay for the backward
        TRY(showo_embed_splice_f32(ids, e->embed, sp->rows, sp->start, t->L[0].x, B, L, sp->n, sp->P, H, V, s));
        SHOWO_CHECK_HIP(hipMemcpyAsync(t->ids, ids, (size_t)T * 8, hipMemcpyDeviceToDevice, s));
        if (sp->n * sp->P > 0)
            SHOWO_CHECK_HIP(hipMemcpyAsync(t->start, sp->start, (size_t)sp->n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    } else if (ids) {
        SHOWO_CHECK_HIP(hipMemcpyAsync(t->ids, ids, (size_t)T * 8, hipMemcpyDeviceToDevice, s));
        TRY(showo_embed_f32(ids, e->embed, t->L[0].x, T, H, V, s));  // layer 0's saved input IS the embedding output (no copy)
    } else {  // inputs_embeds path (modeling_showo.py:77-78, phi.py:1005-1006): the residual stream starts from the caller's rows
        SHOWO_CHECK_HIP(hipMemcpyAsync(t->L[0].x, embeds, (size_t)T * H * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    t->from_embeds = ids == nullptr;
    t->spliced = sp != nullptr;
    t->sp_n = sp ? sp->n : 0;
    t->sp_P = sp ? sp->P : 0;
    const int32_t *iv = nullptr, *flag = nullptr;
    if (mask) {
        TRY(showo_mask_compress(mask, e->iv, e->flag, B, L, L, s));
        iv = e->iv; flag = e->flag;
    } else if (e->ext_iv) {
        // caller-built visibility intervals (showo_trainer_use_intervals): kept in the engine's own buffer for the backward
        SHOWO_CHECK_HIP(hipMemcpyAsync(e->iv, e->ext_iv, (size_t)T * 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        if (e->ext_flag) SHOWO_CHECK_HIP(hipMemcpyAsync(e->flag, e->ext_flag, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        else SHOWO_CHECK_HIP(hipMemsetAsync(e->flag, 0, sizeof(int32_t), s));
        iv = e->iv; flag = e->flag;
    }
    // SHOWO_TRAIN_FUSED_PROJ (default 1): the fused projection launch of the inference layer, in its save-for-backward form
    static const bool fused_env = env_flag("SHOWO_TRAIN_FUSED_PROJ", true);
    // SHOWO_TRAIN_QKPREP (default 0): 1 = raw-only projection launch + showo_qk_prep (A/B of the epilogue's LayerNorm / RoPE cost)
    static const bool qkprep_env = env_flag("SHOWO_TRAIN_QKPREP", false);
    const bool fused_proj = fused_env && T >= 256 && e->cfg.rotary_dim == 32 && (3 * H) % 256 == 0 && (F % 8) == 0 &&
                            (int64_t)T * F * 2 < ((int64_t)1 << 32);
    for (int i = 0; i < e->nL; ++i) {
        Layer& w = e->layers[i];
        LayerT& l = t->L[i];
        // The layer's input (saved for ln_bwd) lives in l.x already: the previous layer's fc2 epilogue wrote it there.  The residual
        // stream ping-pongs l.x -> e->x (after dense) -> L[i + 1].x (after fc2; e->x for the last layer): no 92 MB copy per layer.
        float* xnext = (i + 1 < e->nL) ? t->L[i + 1].x : e->x;
        bf16_t* ffn = train_tn() ? l.a : e->ffn;  // TN form keeps gelu(fc1) per layer for the fc2 weight gradient
        TRY(showo_layernorm_f32_bf16(l.x, w.ln_w, w.ln_b, l.h, nullptr, T, H, e->cfg.ln_eps, s));
        // projection stage.  Fused: q/k/v_proj + q/k LayerNorm + RoPE + relayout AND fc1 + gelu_new in one launch that also saves qkv
        // and the fc1 pre-activation for backward ([Wqkv ; W1] is one allocation, engine.hip); its raw-only form (SHOWO_TRAIN_QKPREP)
        // stores qkv / the fc1 pre-activation / gelu and leaves q/k LayerNorm + RoPE + relayout to showo_qk_prep on the saved qkv, as
        // the unfused GEMM does.  Same bits in all three: each starts from the rounded values.
        const bool prep = !fused_proj || qkprep_env;
        if (fused_proj)
            TRY(showo_gemm_qkv_fc1_save_bf16(l.h, H, w.wqkv, H, w.bqkv, w.qln_w, w.qln_b, w.kln_w, w.kln_b, e->cosT, e->sinT, prep ? nullptr : l.Q,
                                             prep ? nullptr : l.K, prep ? nullptr : l.Vt, l.qkv, 3 * H, l.f, ffn, F, F, B, L, nH, e->cfg.rotary_dim,
                                             e->cfg.ln_eps, 0, L, Lp, 0, s));
        else
            TRY(showo_gemm_bf16(l.h, H, w.wqkv, H, w.bqkv, 0, l.qkv, 3 * H, nullptr, 0, T, 3 * H, H, SHOWO_EPI_BF16, s));
        if (prep)
            TRY(showo_qk_prep(l.qkv, w.qln_w, w.qln_b, w.kln_w, w.kln_b, e->cosT, e->sinT, l.Q, l.K, l.Vt, B, L, nH, e->cfg.rotary_dim,
                              e->cfg.ln_eps, 0, L, Lp, s));
        TRY(showo_attn_fwd_lse(l.Q, l.K, l.Vt, iv, flag, mask, l.attn, l.lse, B, nH, L, L, L, Lp, H, s));
        TRY(showo_gemm_bf16(l.attn, H, w.wd, H, w.bd, 0, e->x, H, l.x, H, T, H, H, SHOWO_EPI_RESID_F32, s));
        if (!fused_proj) {
            TRY(showo_gemm_bf16(l.h, H, w.w1, H, w.b1, 0, l.f, F, nullptr, 0, T, F, H, SHOWO_EPI_BF16, s));
            TRY(showo_gelu_bf16(l.f, ffn, (int64_t)T * F, s));
        }
        TRY(showo_gemm_bf16(ffn, F, w.w2, F, w.b2, 0, xnext, H, e->x, H, T, H, F, SHOWO_EPI_RESID_F32, s));
    }
    int Tc = 0;
    if (compact) {
        SHOWO_CHECK_HIP(hipEventSynchronize(t->ev_tc));
        Tc = *(volatile int32_t*)t->tc_host;
        if (Tc < 0 || Tc > T) return set_error_msg(1, "train_forward: the row census returned a count outside [0, B*L]");
        if (Tc > 0) {
            // compact row j stands for row row_index[j]: gathered final LayerNorm, lm_head on the k-partition of the T-row launch
            TRY(showo_layernorm_f32_bf16(e->x, e->fln_w, e->fln_b, e->hf, t->row_index, Tc, H, e->cfg.ln_eps, s));
            showo::gemm_pin_split_m(T);
            const int rc = showo_gemm_bf16(e->hf, H, e->wlm, H, e->blm, 0, t->logits, V, nullptr, 0, compact_gemm_rows(Tc, T), V, H, SHOWO_EPI_F32, s);
            showo::gemm_pin_split_m(0);
            TRY(rc);
        }
    } else {
    TRY(showo_layernorm_f32_bf16(e->x, e->fln_w, e->fln_b, e->hf, nullptr, T, H, e->cfg.ln_eps, s));
    TRY(showo_gemm_bf16(e->hf, H, e->wlm, H, e->blm, 0, t->logits, V, nullptr, 0, T, V, H, SHOWO_EPI_F32, s));
    }
    t->compact = compact;
    t->Tc = Tc;
    t->split = Split{b_t2i, b_lm, b_mmu, max_seq_len};
    if (logits_out) SHOWO_CHECK_HIP(hipMemcpyAsync(logits_out, t->logits, (size_t)T * V * sizeof(float), hipMemcpyDeviceToDevice, s));
    t->B = B; t->Lq = L;
    t->have_fwd = true;
    t->has_mask = iv != nullptr;
    t->dl_valid = false;
    if (labels) {
        // announced loss weights (lw_set): the one pass writes losses and d(sum_g w_g loss_g)/d(logits), remembered for the backward
        bf16_t* dl = t->lw_set ? t->dlogits : nullptr;
        const float* lw = t->lw;  // read by the kernels only where they write d(logits)
        if (compact)  // the census ran ahead of the blocks: the cross-entropy of the Tc compact rows (none: only the 0 / 0 finalisation)
            TRY(showo::ce_loss_compact(t->logits, V, Tc, V, lw[0], lw[1], lw[2], nullptr, t->ce_rows_c, t->counts, t->rowloss, dl, t->Vp,
                                       t->losses, s));
        else
            TRY(showo_ce_loss(t->logits, V, labels, B, L, V, b_t2i, b_lm, b_mmu, max_seq_len, dl ? lw[0] : 0.f, dl ? lw[1] : 0.f,
                              dl ? lw[2] : 0.f, t->ce_rows, t->counts, t->rowloss, dl, dl ? t->Vp : 0, t->losses, s));
        if (dl) {
            t->dl_valid = true;
            t->dl_labels = labels;
            std::copy(t->lw, t->lw + 3, t->dl_g);
        }
        // the backward works on the interval form only: a mask with more than two visibility runs in a row (never produced by
        // the reference's builders with contiguous padding) must not train silently wrong -> NaN losses, no host sync
        if (iv) poison_losses_kernel<<<1, 64, 0, s>>>(t->losses, e->flag);
        if (losses_out) SHOWO_CHECK_HIP(hipMemcpyAsync(losses_out, t->losses, 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

extern "C" int showo_train_forward(showo_trainer* t, const int64_t* ids, const float* mask, const int64_t* labels, int B, int L,
                                   int b_t2i, int b_lm, int b_mmu, int max_seq_len, float* logits_out, float* losses_out,
                                   void* stream) {
    return train_forward_impl(t, ids, nullptr, mask, labels, B, L, b_t2i, b_lm, b_mmu, max_seq_len, logits_out, losses_out, stream);
}
extern "C" int showo_train_forward_embeds(showo_trainer* t, const float* embeds, const float* mask, const int64_t* labels, int B,
                                          int L, int b_t2i, int b_lm, int b_mmu, int max_seq_len, float* logits_out,
                                          float* losses_out, void* stream) {
    return train_forward_impl(t, nullptr, embeds, mask, labels, B, L, b_t2i, b_lm, b_mmu, max_seq_len, logits_out, losses_out, stream);
}
// showo_train_forward with the projector's rows [n*P, H] spliced into layer 0's input (header: layout); the argument list of
// showo_train_forward itself is unchanged
extern "C" int showo_train_forward_spliced(showo_trainer* t, const int64_t* ids, const float* rows, const int32_t* start, int n, int P,
                                           const float* mask, const int64_t* labels, int B, int L, int b_t2i, int b_lm, int b_mmu,
                                           int max_seq_len, float* logits_out, float* losses_out, void* stream) {
    Splice sp;
    sp.rows = rows; sp.start = start; sp.n = n; sp.P = P;
    return train_forward_impl(t, ids, nullptr, mask, labels, B, L, b_t2i, b_lm, b_mmu, max_seq_len, logits_out, losses_out, stream, &sp);
}
// the placeholder rows of d(weighted loss)/d(layer 0's input), compacted in row order: fp32 [n*P, H] = d/d(projector output)
extern "C" int showo_train_image_grad(showo_trainer* t, float* out, int64_t n_elems, void* stream) {
    if (!t || !t->have_fwd || !t->spliced) return set_error_msg(1, "train_image_grad: run showo_train_forward_spliced + the backward first");
    if (!t->want_input) return set_error_msg(1, "train_image_grad: not requested (showo_train_set_input_grad)");
    if (n_elems != (int64_t)t->sp_n * t->sp_P * t->e->H) return set_error_msg(1, "train_image_grad: size mismatch");
    if (n_elems == 0) return 0;
    if (!out) return set_error_msg(1, "train_image_grad: null output");
    return showo_gather_splice_rows_f32(t->dy, t->start, out, t->B, t->Lq, t->sp_n, t->sp_P, t->e->H, stream);
}
// d(weighted loss) / d(input embeddings) fp32 [B*L, H] of the last backward (the residual-stream gradient at block 0's input)
extern "C" int showo_train_input_grad(showo_trainer* t, float* out, int64_t n, void* stream) {
    if (!t || !out || !t->have_fwd) return set_error_msg(1, "train_input_grad: run forward + backward first");
    if (n != (int64_t)t->B * t->Lq * t->e->H) return set_error_msg(1, "train_input_grad: size mismatch");
    if (!t->want_input) return set_error_msg(1, "train_input_grad: not requested (showo_train_set_input_grad)");
    SHOWO_CHECK_HIP(hipMemcpyAsync(out, t->dy, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// ---- backward, in three phases so that a data-parallel driver can start the gradient exchange of a finished bucket
// while the next block is still running: head (bucket nL+1) -> blocks nL-1 .. 0 (buckets i+1) -> embedding (bucket 0)
#define BW_PROLOGUE                                                                                                   \
    hipStream_t s = (hipStream_t)stream;                                                                              \
    if (!t || !t->have_fwd) return set_error_msg(1, "train_backward: run showo_train_forward first");                  \
    showo_engine* e = t->e;                                                                                           \
    const int H = e->H, F = e->F, V = e->V, nH = e->nH, B = t->B, L = t->Lq, T = B * L, Vp = t->Vp;                    \
    const int Tp = ((T + 63) / 64) * 64, Lp = ((L + 63) / 64) * 64;                                                   \
    const int32_t* iv = t->has_mask ? e->iv : nullptr;                                                                \
    const int acc = t->accumulate ? 1 : 0; /* parameter-gradient writers add into their slot; scratch side outputs never do */ \
    (void)F; (void)V; (void)nH; (void)Vp; (void)Tp; (void)Lp; (void)iv; (void)s; (void)acc;

// weight gradient of the NT form: out fp32 [M, N] (+)= (dY^T)[M, Tp] (X^T)[N, Tp]^T on the k-contiguous GEMM; accumulating =
// the residual epilogue with resid = out (the finished accumulator is added to the old value once)
static int wgrad_nt(const bf16_t* dyT, const bf16_t* xT, float* out, int ldo, int M, int N, int Tp, int acc, hipStream_t s) {
    return showo_gemm_bf16(dyT, Tp, xT, Tp, nullptr, 0, out, ldo, acc ? out : nullptr, acc ? ldo : 0, M, N, Tp,
                           acc ? SHOWO_EPI_RESID_F32 : SHOWO_EPI_F32, s);
}

namespace {
// The two forms (SHOWO_TRAIN_TN) of a weight gradient dW[M, N] (+)= dY^T X over R token rows and of its bias gradient db = column
// sums of dY.  The backward asks image(dY) once per dY tensor, then weight(dY, X) for every weight that contracts with it.
//   TN form: showo_gemm_tn_bf16 on the token-major tensors; image() is showo_colsum_bf16 into db, unless the launch that produced
//            dY wrote db already (fused: showo_ln_bwd_colsum_acc for dy16, showo_dgelu_colsum_bf16_acc for d f).
//   NT form: image() transposes dY into bigT and writes db from the same pass; weight() transposes X into xT and runs wgrad_nt.
//            bigT holds ONE dY image and xT ONE X image at a time, so the order of the calls is part of the result: every weight()
//            of a dY comes before the next image().  xT remembers the X it holds: h^T serves dW1 and dWqkv when both run (hold_x,
//            asked for ahead of dW1 so that it is made at the same point whichever of the two trains).
//   fc2's X is gelu_new(f): the NT transpose applies it (mode 1) to the saved pre-activation l.f, the TN form reads the rows the
//   forward saved (l.a, allocated in that form only).
struct XOp { const bf16_t* p; int mode; };
struct WGrad {
    showo_trainer* t;
    int R, Tp, acc;  // token rows, their padded count (the row length of both images), 1 = add into the gradient slots
    hipStream_t s;
    const bf16_t* held = nullptr;  // NT: the X whose image xT holds

    enum Weights { NO_WEIGHT, WEIGHT_FOLLOWS };       // some weight() of this dY follows (NT form: the image is needed for it)
    enum TnSums { TN_SUMS_HERE, TN_SUMS_BY_PRODUCER };  // TN form: who writes db -- image(), or the launch that produced dY
    XOp fc2_x(const LayerT& l) const { return train_tn() ? XOp{l.a, 0} : XOp{l.f, 1}; }
    // dY [R, M]; db: bias gradient slot or NULL
    int image(const bf16_t* dY, int M, Weights w, float* db, TnSums sums) {
        if (train_tn()) return (db && sums == TN_SUMS_HERE) ? showo_colsum_bf16(dY, M, R, M, t->colpart, db, acc, s) : 0;
        return (w == WEIGHT_FOLLOWS || db) ? showo_transpose_bf16(dY, M, t->bigT, R, M, Tp, 0, t->colpart, db, acc, s) : 0;
    }
    static Weights follows(bool any) { return any ? WEIGHT_FOLLOWS : NO_WEIGHT; }
    int hold_x(XOp x, int N) {
        if (train_tn() || held == x.p) return 0;
        held = x.p;
        return showo_transpose_bf16(x.p, N, t->xT, R, N, Tp, x.mode, nullptr, nullptr, 0, s);
    }
    // out [M, N] (+)= dY[R, :M]^T X[R, N]
    int weight(const bf16_t* dY, int ldy, XOp x, int N, float* out, int M) {
        if (train_tn()) TRY(showo_gemm_tn_bf16(dY, ldy, x.p, N, out, N, M, N, R, acc, 1, s));
        else {
            TRY(hold_x(x, N));
            TRY(wgrad_nt(t->bigT, t->xT, out, N, M, N, Tp, acc, s));
        }
        ++t->cnt[0];
        return 0;
    }
};
}  // namespace

// The LayerNorm backward that leaves dy / dy16 as block j's incoming gradient (j < 0: nothing above the embedding consumes them as a
// block).  TN form: the launch also writes the column sums of dy16 = block j's dense / fc2 bias gradients (b2_dst, scratch when both
// are frozen).  slot != NULL: the row-slot form over a compact dh (dy is written whole, not added to).
static int ln_bwd_into_block(showo_trainer* t, int j, const float* x, const float* gamma, float* gln, int acc_g, const int* slot, int T,
                             hipStream_t s) {
    const int H = t->e->H;
    const float eps = t->e->cfg.ln_eps;
    const bool sums = train_tn() && j >= 0;
    float* cb = sums ? b2_dst(t, j) : nullptr;
    const int acc_cb = t->accumulate && cb;
    float* dxsum = sums ? (cb ? cb : t->sc_b) : nullptr;
    if (slot)
        return showo::ln_bwd_slot(x, gamma, t->dh, slot, t->dy, t->dy16, t->lnpart, gln, dxsum, acc_g, acc_cb, T, H, eps, s);
    if (sums)
        return showo_ln_bwd_colsum_acc(x, gamma, t->dh, t->dy, t->dy, t->dy16, t->lnpart, gln, dxsum, acc_g, acc_cb, T, H, eps, s);
    return showo_ln_bwd_acc(x, gamma, t->dh, t->dy, t->dy, t->dy16, t->lnpart, gln, acc_g, T, H, eps, s);
}

// the head phase after d(logits) is in t->dlogits: lm_head weight / bias gradients, d(final LayerNorm), dy of the top block.
// Frozen lm_head tensors get no launch; the dgrad GEMM and the final-LayerNorm backward run only when something below consumes them.
static int backward_head_from_dlogits(showo_trainer* t, void* stream) {
    BW_PROLOGUE
    TRY(plan_sync(t, s));
    // R: the token rows the lm_head gradients contract over -- all of them, or the Tc compact rows of a labelled-rows forward
    // (dlogits, hf and dh are then compact; the row-slot LayerNorm backward scatters dh back to the T rows)
    const int R = t->compact ? t->Tc : T;
    if (R == 0) {  // no labelled row: the head's gradients are zero (accumulating: nothing is added), no zero-sized launch
        if (!acc && t->p_blm) SHOWO_CHECK_HIP(hipMemsetAsync(t->gblm, 0, (size_t)Vp * sizeof(float), s));
        if (!acc && t->p_wlm) SHOWO_CHECK_HIP(hipMemsetAsync(t->gwlm, 0, (size_t)V * H * sizeof(float), s));
    } else {
        WGrad wg{t, R, Tp, acc, s};
        TRY(wg.image(t->dlogits, Vp, WGrad::follows(t->p_wlm), t->p_blm ? t->gblm : nullptr, WGrad::TN_SUMS_HERE));  // lm_head bias grad
        if (t->p_wlm) TRY(wg.weight(t->dlogits, Vp, XOp{e->hf, 0}, H, t->gwlm, V));    // dWlm [V,H]
    }
    if (!t->p_fln && !below_needs(t, e->nL)) return 0;  // nothing below the head trains (linear probe): no dgrad, no LayerNorm backward
    if (!t->compact || R > 0) {  // d hf; compact: on the k-partition of the T-row launch
        if (t->compact) showo::gemm_pin_split_m(T);
        const int rows = t->compact ? compact_gemm_rows(R, T) : T;
        const int rc = showo_gemm_bf16(t->dlogits, Vp, t->wlmT, Vp, nullptr, 0, t->dh, H, nullptr, 0, rows, H, Vp, SHOWO_EPI_F32, s);
        if (t->compact) showo::gemm_pin_split_m(0);
        TRY(rc);
        ++t->cnt[1];
    }
    // compact: every row of dy / dy16 is written (zeros for the rows without a label): no clear of dy, and with R == 0 dh is never read
    if (!t->compact) SHOWO_CHECK_HIP(hipMemsetAsync(t->dy, 0, (size_t)T * H * sizeof(float), s));
    TRY(ln_bwd_into_block(t, e->nL - 1, e->x, e->fln_w, t->p_fln ? t->gfln : t->sc_ln, acc && t->p_fln,
                          t->compact ? t->row_slot : nullptr, T, s));
    for (const Grad& g : t->fln_clear) SHOWO_CHECK_HIP(hipMemsetAsync(g.p, 0, (size_t)g.n * sizeof(float), s));
    return 0;
}

// Both head entry points: the three loss weights on the host (g) or in device memory (g3).  A compact forward's logits are in the order
// of its census, so its backward works from that table and those counts and must be asked for the same split; the cross-entropy pass
// that fills d(logits) is skipped when the forward's announced one (showo_train_set_loss_weights) answers the same question.
static int backward_head(showo_trainer* t, const int64_t* labels, const Split& sp, const float* g, const float* g3, void* stream) {
    BW_PROLOGUE
    const bool dev = !g;  // showo_train_backward_head_dev: the weights are g3's
    if (!labels || (dev && !g3))
        return set_error_msg(1, dev ? "train_backward_head_dev: labels and g3 required" : "train_backward: labels required");
    const bool have_dl = g && t->dl_valid && t->dl_labels == labels && std::equal(g, g + 3, t->dl_g) && t->split == sp;
    t->dl_valid = false;  // a second backward must not trust a consumed flag blindly
    if (t->compact && !(t->split == sp))
        return set_error_msg(1, dev ? "train_backward_head_dev: the labelled-rows forward was made with another batch split"
                                    : "train_backward: the labelled-rows forward was made with another batch split");
    const float g0 = g ? g[0] : 0.f, g1 = g ? g[1] : 0.f, g2 = g ? g[2] : 0.f;
    if (!have_dl) {
        if (t->compact)
            TRY(showo::ce_loss_compact(t->logits, V, t->Tc, V, g0, g1, g2, g3, t->ce_rows_c, t->counts, t->rowloss, t->dlogits, Vp, nullptr, s));
        else if (g3)
            TRY(showo::ce_loss_dev_weights(t->logits, V, labels, B, L, V, sp.b_t2i, sp.b_lm, sp.b_mmu, sp.max_seq_len, g3, t->ce_rows, t->counts,
                                           t->rowloss, t->dlogits, Vp, s));
        else
            TRY(showo_ce_loss(t->logits, V, labels, B, L, V, sp.b_t2i, sp.b_lm, sp.b_mmu, sp.max_seq_len, g0, g1, g2, t->ce_rows, t->counts,
                              t->rowloss, t->dlogits, Vp, nullptr, s));
    }
    return backward_head_from_dlogits(t, stream);
}

extern "C" int showo_train_backward_head(showo_trainer* t, const int64_t* labels, int b_t2i, int b_lm, int b_mmu, int max_seq_len,
                                         float g_t2i, float g_lm, float g_mmu, void* stream) {
    const float g[3] = {g_t2i, g_lm, g_mmu};
    return backward_head(t, labels, Split{b_t2i, b_lm, b_mmu, max_seq_len}, g, nullptr, stream);
}

// the same with the three loss weights in device memory g3[3] (the autograd path: they are the incoming gradients of the three loss
// outputs, training/train.py:600,612, and are never read on the host).  Always runs its own cross-entropy pass over the logits.
extern "C" int showo_train_backward_head_dev(showo_trainer* t, const int64_t* labels, int b_t2i, int b_lm, int b_mmu, int max_seq_len,
                                             const float* g3, void* stream) {
    return backward_head(t, labels, Split{b_t2i, b_lm, b_mmu, max_seq_len}, nullptr, g3, stream);
}

// number of training forwards this trainer has started (showo_train_forward / _embeds, whether or not they succeeded): a backward
// driven from the host checks that the saved activations still belong to its own forward
extern "C" int64_t showo_train_generation(showo_trainer* t) { return t ? (int64_t)t->generation : -1; }

// Block i's phase.  Frozen tensors get no weight-gradient launch; the fused launches that also carry a parameter gradient as a side
// output (dgelu_colsum, qkln_rope_bwd, ln_bwd_colsum) keep running for their data gradients with that output pointed at scratch, so
// the data-gradient chain is the same bits whatever trains.  A chain runs only if something consumes it: d a -> d f for W1 / b1 or
// dh, d o -> attention -> d qkv for Wqkv / bqkv / q,k-LN or dh, and dh + the LayerNorm backward only when this block's LayerNorm or
// anything below trains (the lowest phase anything needs stops there).  Nothing at or below the block trains: no launch at all.
extern "C" int showo_train_backward_layer(showo_trainer* t, int i, void* stream) {
    BW_PROLOGUE
    if (i < 0 || i >= e->nL) return set_error_msg(1, "train_backward_layer: bad layer index");
    TRY(plan_sync(t, s));
    const LayerPlan& p = t->plan[i];
    const bool below = below_needs(t, i);
    if (!p.any && !below) return 0;
    ++t->cnt[2];
    const bool need_dh = below || p.ln;
    const bool mlp = p.w1 || p.b1 || need_dh;
    const bool attn = p.wqkv || p.bqkv || p.qk || need_dh;
    Layer& w = e->layers[i];
    LayerT& l = t->L[i];
    WGrad wg{t, T, Tp, acc, s};
    // dy16: the dense / fc2 bias gradients are its column sums (TN form: written by the LayerNorm backward that produced dy16)
    TRY(wg.image(t->dy16, H, WGrad::follows(p.w2 || p.wd), b2_dst(t, i), WGrad::TN_SUMS_BY_PRODUCER));
    if (p.bd && p.b2) SHOWO_CHECK_HIP(hipMemcpyAsync(l.gbd, l.gb2, (size_t)H * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (p.w2) TRY(wg.weight(t->dy16, H, wg.fc2_x(l), F, l.gw2, H));                                                         // dW2 [H,F]
    if (p.wd) TRY(wg.weight(t->dy16, H, XOp{l.attn, 0}, H, l.gwd, H));                                                      // dWd [H,H]
    if (mlp) {
        TRY(showo_gemm_bf16(t->dy16, H, l.w2T, H, nullptr, 0, t->dff, F, nullptr, 0, T, F, H, SHOWO_EPI_BF16, s));          // d a
        ++t->cnt[1];
        if (train_tn())                                                                                                     // d f (, db1)
            TRY(showo_dgelu_colsum_bf16_acc(t->dff, l.f, t->dff, F, T, F, t->colpart, p.b1 ? l.gb1 : t->sc_b1, acc && p.b1, s));
        else
            TRY(showo_dgelu_bf16(t->dff, l.f, t->dff, (int64_t)T * F, s));
        TRY(wg.image(t->dff, F, WGrad::follows(p.w1), p.b1 ? l.gb1 : nullptr, WGrad::TN_SUMS_BY_PRODUCER));  // (dgelu_colsum above)
        if (p.w1 || p.wqkv) TRY(wg.hold_x(XOp{l.h, 0}, H));  // NT: h^T is made HERE for dW1 and dWqkv, whichever of them trains
        if (p.w1) TRY(wg.weight(t->dff, F, XOp{l.h, 0}, H, l.gw1, F));                                                      // dW1 [F,H]
        if (need_dh) {
            TRY(showo_gemm_bf16(t->dff, F, l.w1T, F, nullptr, 0, t->dh, H, nullptr, 0, T, H, F, SHOWO_EPI_F32, s));         // dh (mlp)
            ++t->cnt[1];
        }
    }
    if (attn) {
        TRY(showo_gemm_bf16(t->dy16, H, l.wdT, H, nullptr, 0, t->d_o, H, nullptr, 0, T, H, H, SHOWO_EPI_BF16, s));          // d o
        ++t->cnt[1];
        TRY(showo_head_transpose(l.Q, t->QT, B, nH, L, Lp, (int64_t)nH * L * 64, (int64_t)L * 64, 64, s));
        TRY(showo_head_transpose(l.K, t->KT, B, nH, L, Lp, (int64_t)nH * L * 64, (int64_t)L * 64, 64, s));
        TRY(showo_attn_bwd(l.Q, l.K, t->QT, t->KT, l.qkv + 2 * H, 3 * H, l.attn, t->d_o, H, t->dOT, l.lse, t->D, iv, nullptr, t->dqk, 2 * H,
                           t->dqk + H, 2 * H, t->dqkv + 2 * H, 3 * H, B, nH, L, Lp, s));
        TRY(showo_qkln_rope_bwd_acc(t->dqk, t->dqk + H, 2 * H, l.qkv, w.qln_w, w.kln_w, e->cosT, e->sinT, t->dqkv, t->qkpart,
                                    p.qk ? l.gqk : t->sc_qk, acc && p.qk, T, L, nH, e->cfg.rotary_dim, e->cfg.ln_eps, s));
        TRY(wg.image(t->dqkv, 3 * H, WGrad::follows(p.wqkv), p.bqkv ? l.gbqkv : nullptr, WGrad::TN_SUMS_HERE));             // dbqkv
        if (p.wqkv) TRY(wg.weight(t->dqkv, 3 * H, XOp{l.h, 0}, H, l.gwqkv, 3 * H));                                         // dWqkv [3H,H]
        if (need_dh) {
            // dh += attn part
            TRY(showo_gemm_bf16(t->dqkv, 3 * H, l.wqkvT, 3 * H, nullptr, 0, t->dh, H, t->dh, H, T, H, 3 * H, SHOWO_EPI_RESID_F32, s));
            ++t->cnt[1];
        }
    }
    // LayerNorm + residual (+ the column sums of dy16 = the dense / fc2 bias gradients of block i - 1, wherever that block trains)
    if (need_dh) TRY(ln_bwd_into_block(t, i - 1, l.x, w.ln_w, p.ln ? l.gln : t->sc_ln, acc && p.ln, nullptr, T, s));
    for (const Grad& g : p.clear) SHOWO_CHECK_HIP(hipMemsetAsync(g.p, 0, (size_t)g.n * sizeof(float), s));
    return 0;
}

// Announce the weights of the three losses (training/train.py:600: loss = w_t2i loss_t2i + w_lm loss_lm + w_mmu loss_mmu) BEFORE the
// forward: its cross-entropy pass then also writes d(loss)/d(logits), and showo_train_backward[_head] called with the same labels
// pointer, batch split and weights does not read the logits a second time.  enable = 0 restores the two-pass behaviour.
extern "C" int showo_train_set_loss_weights(showo_trainer* t, float w_t2i, float w_lm, float w_mmu, int enable) {
    if (!t) return set_error_msg(1, "train_set_loss_weights: null handle");
    t->lw_set = enable != 0;
    t->lw[0] = w_t2i; t->lw[1] = w_lm; t->lw[2] = w_mmu;
    t->dl_valid = false;
    return 0;
}

extern "C" int showo_train_backward_embed(showo_trainer* t, void* stream) {
    BW_PROLOGUE
    // ---- embedding: a frozen table gets no launch (its slot was zeroed when it froze); a forward from caller-provided embeddings did
    // not read the table, its caller owns d/d(embeddings) (showo_train_input_grad) and the table's gradient is zero -- cleared once
    // after a scatter of an earlier backward, not on every step
    TRY(plan_sync(t, s));
    if (!t->p_emb) return 0;
    // overwriting: the table is cleared first (once, when nothing was scattered into it since).  Accumulating: it keeps the window's
    // partial sum -- no clear, and the scatter adds its position-ordered row sums into the rows this micro-batch touches; a
    // micro-batch that started from embeddings contributes nothing to the table
    if (!acc) {
        if (t->from_embeds && !t->gembed_dirty) return 0;
        SHOWO_CHECK_HIP(hipMemsetAsync(t->gembed, 0, (size_t)V * H * sizeof(float), s));
        ++t->cnt[3];
        t->gembed_dirty = false;
    }
    if (t->from_embeds) return 0;
    if (t->spliced) TRY(showo_embed_bwd_splice(t->ids, t->dy, t->gembed, t->order_ws, t->start, acc, B, L, t->sp_n, t->sp_P, H, V, s));
    else TRY(showo_embed_bwd_acc(t->ids, t->dy, t->gembed, t->order_ws, acc, T, H, V, s));
    ++t->cnt[3];
    t->gembed_dirty = true;
    return 0;
}

// d(g_t2i loss_t2i + g_lm loss_lm + g_mmu loss_mmu) / d(parameters) of the last showo_train_forward
extern "C" int showo_train_backward(showo_trainer* t, const int64_t* labels, int b_t2i, int b_lm, int b_mmu, int max_seq_len,
                                    float g_t2i, float g_lm, float g_mmu, void* stream) {
    TRY(showo_train_backward_head(t, labels, b_t2i, b_lm, b_mmu, max_seq_len, g_t2i, g_lm, g_mmu, stream));
    for (int i = t->e->nL - 1; i >= 0; --i) TRY(showo_train_backward_layer(t, i, stream));
    return showo_train_backward_embed(t, stream);
}

// bucket b of the flat gradient buffer: 0 = embedding, 1 + i = block i, nL + 1 = head (final LayerNorm, lm_head)
extern "C" int showo_train_bucket(showo_trainer* t, int b, float** ptr, int64_t* n) {
    if (!t || !ptr || !n || b < 0 || b >= (int)t->buckets.size()) return set_error_msg(1, "train_bucket: bad argument");
    *ptr = t->gflat + t->buckets[b].first;
    *n = t->buckets[b].second;
    return 0;
}
extern "C" int showo_train_num_buckets(showo_trainer* t) { return t ? (int)t->buckets.size() : -1; }

extern "C" int showo_train_grad(showo_trainer* t, const char* key, float** ptr, int64_t* n) {
    if (!t || !key || !ptr || !n) return set_error_msg(1, "train_grad: null argument");
    auto it = t->grads.find(key);
    if (it == t->grads.end()) return set_error_msg(3, "train_grad: unknown state-dict key");
    *ptr = it->second.p;
    *n = it->second.n;
    return 0;
}

extern "C" int showo_train_losses(showo_trainer* t, float* out3, void* stream) {
    if (!t || !out3) return set_error_msg(1, "train_losses: null argument");
    SHOWO_CHECK_HIP(hipMemcpyAsync(out3, t->losses, 3 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int showo_train_grad_copy(showo_trainer* t, const char* key, float* dst, int64_t n, void* stream) {
    float* p = nullptr;
    int64_t m = 0;
    TRY(showo_train_grad(t, key, &p, &m));
    if (m != n) return set_error_msg(2, "train_grad_copy: element count mismatch");
    SHOWO_CHECK_HIP(hipMemcpyAsync(dst, p, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// ---- optimizer: the host registers its fp32 master tensors and moment buffers once; one call then updates everything
extern "C" int showo_train_bind_param(showo_trainer* t, const char* key, float* param, float* exp_avg, float* exp_avg_sq, int64_t n) {
    if (!t || !key || !param || !exp_avg || !exp_avg_sq) return set_error_msg(1, "train_bind_param: null argument");
    auto it = t->grads.find(key);
    if (it == t->grads.end()) return set_error_msg(3, "train_bind_param: unknown state-dict key");
    if (it->second.n != n) return set_error_msg(2, "train_bind_param: element count mismatch");
    std::string k(key);
    // reference rule (training/train.py:211): no weight decay for names containing one of these substrings
    const char* nd[4] = {"bias", "layer_norm.weight", "mlm_ln.weight", "embeddings.weight"};
    bool decay = true;
    for (const char* x : nd) decay = decay && k.find(x) == std::string::npos;
    t->adam_dirty = true;  // the optimizer's segment table is rebuilt by the next step
    t->ema_dirty = true;
    for (auto& b : t->bound)
        if (b.key == k) { b.p = param; b.m = exp_avg; b.v = exp_avg_sq; b.n = n; b.decay = decay; return 0; }  // (a bound shadow stays)
    t->bound.push_back(Bound{k, param, exp_avg, exp_avg_sq, n, decay});
    return 0;
}

// ---- EMA of the weights: a shadow tensor per bound key (NULL takes it away again); the tables are rebuilt by their next user
extern "C" int showo_train_bind_ema(showo_trainer* t, const char* key, float* shadow, int64_t n) {
    if (!t || !key) return set_error_msg(1, "train_bind_ema: null argument");
    std::string k(key);
    for (auto& b : t->bound)
        if (b.key == k) {
            if (b.n != n) return set_error_msg(2, "train_bind_ema: element count mismatch");
            if (shadow && shadow == b.p) return set_error_msg(1, "train_bind_ema: the shadow is the parameter itself");
            b.s = shadow;
            t->adam_dirty = true;
            t->ema_dirty = true;
            return 0;
        }
    return set_error_msg(3, "train_bind_ema: the key has no bound parameter (showo_train_bind_param first)");
}

extern "C" int showo_train_set_ema(showo_trainer* t, float one_minus_decay) {
    if (!t) return set_error_msg(1, "train_set_ema: null handle");
    if (one_minus_decay > 1.f || one_minus_decay != one_minus_decay) return set_error_msg(1, "train_set_ema: 1 - decay must lie in [0, 1] (negative: no EMA)");
    t->ema_omd = one_minus_decay < 0.f ? -1.f : one_minus_decay;
    return 0;
}

static int ema_tables_sync(showo_trainer* t, hipStream_t s) {
    if (!t->ema_dirty) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    hipStreamIsCapturing(s, &cs);
    if (cs != hipStreamCaptureStatusNone) return set_error_msg(7, "train ema: the segment tables must be built outside a stream capture");
    std::vector<showo::EmaSeg> all, trainable;
    t->ema_keys.clear();
    for (auto& b : t->bound) {
        if (!b.s) continue;
        showo::EmaSeg sg{b.s, b.p, nullptr, nullptr, b.n};
        if (!t->frozen.count(b.key)) trainable.push_back(sg);
        uint16_t* d16 = nullptr;
        TRY(showo_engine_slot(t->e, b.key.c_str(), b.n, &d16, &sg.dst32));
        sg.dst16 = d16;
        all.push_back(sg);
        t->ema_keys.push_back({b.key, showo::engine_version(t->e, b.key.c_str())});
    }
    TRY(t->ema_all.build(all));
    TRY(t->ema_trainable.build(trainable));
    t->ema_dirty = false;
    return 0;
}

// Exchange every shadowed parameter (frozen ones included) with its shadow in place and write the engine's images from the values that
// go into the parameters; same bookkeeping as the optimizer step for the rewritten tensors.  Twice = every bit as before.
extern "C" int showo_train_ema_swap(showo_trainer* t, void* stream) {
    if (!t) return set_error_msg(1, "train_ema_swap: null handle");
    hipStream_t s = (hipStream_t)stream;
    TRY(ema_tables_sync(t, s));
    if (t->ema_all.count == 0) return set_error_msg(1, "train_ema_swap: no shadow bound (showo_train_bind_ema)");
    TRY(t->ema_all.swap(s));
    showo_engine* e = t->e;
    for (auto& kv : t->ema_keys) {
        if (kv.second) *kv.second = ++e->clock;
        e->lo_loaded.erase(kv.first);
    }
    e->px3_valid = false;
    e->head3_valid = false;
    e->img_f16 = false;
    return 0;
}

// torch.optim.AdamW.step() over every bound parameter that trains (showo_train_set_trainable) with the gradients of the last backward,
// followed by the refresh of the engine's bf16 weight images of those parameters: their version stamps make the next user rebuild
// exactly the derived images (transposed dgrad images, fused block images) that depend on them
extern "C" int showo_train_adamw_step(showo_trainer* t, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                      void* stream) {
    if (!t) return set_error_msg(1, "train_adamw_step: null handle");
    if (t->bound.empty()) return set_error_msg(1, "train_adamw_step: no parameters bound");
    // SHOWO_TRAIN_ADAMW_MULTI (default 1): one launch over a segment table instead of one adamw + one image refresh per tensor
    static const bool multi = env_flag("SHOWO_TRAIN_ADAMW_MULTI", true);
    const float omd = t->ema_omd;  // announced for this step alone (showo_train_set_ema)
    t->ema_omd = -1.f;
    if (multi) {
        hipStream_t s = (hipStream_t)stream;
        if (t->adam_dirty) {  // (re)build the table: segments = bound tensors with their engine destinations, chunks of ADAM_CHUNK elements
            std::vector<showo::AdamSeg> segs;
            std::vector<int> seg_of;
            std::vector<int64_t> start_of;
            t->adam_keys.clear();
            t->adam_shadowed = true;
            for (auto& b : t->bound) {
                if (t->frozen.count(b.key)) continue;
                t->adam_keys.push_back({b.key, showo::engine_version(t->e, b.key.c_str())});
                showo::AdamSeg sg{b.p, b.m, b.v, t->grads[b.key].p, nullptr, nullptr, b.n, b.decay ? 1 : 0, b.s};
                t->adam_shadowed = t->adam_shadowed && b.s != nullptr;
                uint16_t* d16 = nullptr;
                TRY(showo_engine_slot(t->e, b.key.c_str(), b.n, &d16, &sg.dst32));
                sg.dst16 = d16;
                for (int64_t st = 0; st < b.n; st += showo::ADAM_CHUNK) { seg_of.push_back((int)segs.size()); start_of.push_back(st); }
                segs.push_back(sg);
            }
            if (segs.empty()) return set_error_msg(1, "train_adamw_step: every bound parameter is frozen");
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            hipStreamIsCapturing(s, &cs);
            if (cs != hipStreamCaptureStatusNone) return set_error_msg(7, "train_adamw_step: the segment table must be built outside a stream capture");
            if (t->adam_segs) { hipFree(t->adam_segs); hipFree(t->adam_seg_of); hipFree(t->adam_start_of); }
            SHOWO_CHECK_HIP(hipMalloc(&t->adam_segs, segs.size() * sizeof(showo::AdamSeg)));
            SHOWO_CHECK_HIP(hipMalloc(&t->adam_seg_of, seg_of.size() * sizeof(int)));
            SHOWO_CHECK_HIP(hipMalloc(&t->adam_start_of, start_of.size() * sizeof(int64_t)));
            SHOWO_CHECK_HIP(hipMemcpy(t->adam_segs, segs.data(), segs.size() * sizeof(showo::AdamSeg), hipMemcpyHostToDevice));
            SHOWO_CHECK_HIP(hipMemcpy(t->adam_seg_of, seg_of.data(), seg_of.size() * sizeof(int), hipMemcpyHostToDevice));
            SHOWO_CHECK_HIP(hipMemcpy(t->adam_start_of, start_of.data(), start_of.size() * sizeof(int64_t), hipMemcpyHostToDevice));
            t->adam_chunks = (int)seg_of.size();
            t->adam_dirty = false;
        }
        if (omd >= 0.f && !t->adam_shadowed) return set_error_msg(1, "train_adamw_step: EMA announced, but a trainable parameter has no shadow bound");
        TRY(showo::adamw_multi_launch(t->adam_segs, t->adam_seg_of, t->adam_start_of, t->adam_chunks, lr, beta1, beta2, eps, weight_decay, step, omd, s));
        // the bookkeeping of showo_engine_weights_touched, for the rewritten tensors only
        showo_engine* e = t->e;
        for (auto& kv : t->adam_keys) {
            if (kv.second) *kv.second = ++e->clock;
            e->lo_loaded.erase(kv.first);  // the hi images were rewritten without their low halves: accuracy mode needs a re-upload
        }
        e->px3_valid = false;
        e->head3_valid = false;
        e->img_f16 = false;  // the trainer writes bf16 images: a precision-2 engine needs a re-upload too (run_layers checks)
        return 0;
    }
    for (auto& b : t->bound) {
        if (t->frozen.count(b.key)) continue;
        const Grad& g = t->grads[b.key];
        TRY(showo_adamw(b.p, g.p, b.m, b.v, b.n, lr, beta1, beta2, eps, b.decay ? weight_decay : 0.f, step, stream));
        TRY(showo_engine_load(t->e, b.key.c_str(), b.p, b.n, stream));
    }
    if (omd >= 0.f) {  // the table update over the trainable tensors, from the masters the loop above just wrote: the fused form's bits
        TRY(ema_tables_sync(t, (hipStream_t)stream));
        for (auto& b : t->bound)
            if (!b.s && !t->frozen.count(b.key)) return set_error_msg(1, "train_adamw_step: EMA announced, but a trainable parameter has no shadow bound");
        TRY(t->ema_trainable.update(omd, (hipStream_t)stream));
    }
    return 0;
}
