// Show-o transformer engine: packed bf16 weights + workspaces resident in HBM, whole-module entry points.
// Replaces (reference): PhiForCausalLM/PhiModel forward (models/phi.py:953-1183), Showo.forward without
// labels (models/modeling_showo.py:76-79), the layer stack and head under Showo.t2i_generate (its host side is t2i_engine.hip) and the
// layer stack and head under the incremental form of Showo.mmu_generate (models/modeling_showo.py:183-240; its KV cache
// and token loop are in decode_engine.hip, the launches of a one-token step in decode.hip).
//
// Data layout in HBM (T = B*L tokens, H hidden, F ffn):
//   x      fp32 [T,H]    residual stream (kept fp32; both GEMM epilogues accumulate into it in place)
//   h      bf16 [T,H]    LayerNorm output (shared by the attention and MLP branches, phi.py:776-790)
//   qkv    bf16 [T,3H]   fused q|k|v projection
//   Q,K    bf16 [B,nH,L,64]; Vt bf16 [B,nH,64,Lp]    head-major operands of the attention kernel
//   attn   bf16 [T,H]; ffn bf16 [T,F]
//   weights: Wqkv [3H,H], Wd [H,H], W1 [F,H], W2 [H,F], Wlm [V,H] bf16 row-major (= nn.Linear layout,
//   K-contiguous, exactly what the MFMA GEMM's operand loader wants); biases / LayerNorm params fp32.
#include "engine.h"
#include "decode_common.h"
#include <algorithm>
#include <cstdio>
#include <vector>
#include <cstring>
#include <set>
#include <string>
#include <vector>

using namespace showo;

extern "C" int showo_engine_create(const showo_engine_config* c, showo_engine** out) {
    if (!c || !out) return set_error_msg(1, "engine_create: null argument");
    if (c->hidden % 64 || c->hidden != c->heads * 64) return set_error_msg(1, "engine: head_dim must be 64");
    if (c->ffn % 64) return set_error_msg(1, "engine: ffn must be a multiple of 64");
    showo_engine* e = new showo_engine();
    e->cfg = *c;
    e->H = c->hidden; e->nL = c->layers; e->nH = c->heads; e->F = c->ffn; e->V = c->vocab;
    e->maxT = (int64_t)c->max_batch * c->max_seq;
    const int H = e->H, F = e->F, V = e->V;
    int rc = 0;
    rc |= e->alloc(&e->embed, (int64_t)V * H);
    e->layers.resize(e->nL);
    for (auto& l : e->layers) {
        rc |= e->alloc(&l.wqkv, (int64_t)(3 * H + F) * H); rc |= e->alloc(&l.bqkv, 3 * H + F);
        if (!rc) { l.w1 = l.wqkv + (int64_t)3 * H * H; l.b1 = l.bqkv + 3 * H; }
        rc |= e->alloc(&l.wd, (int64_t)H * H); rc |= e->alloc(&l.bd, H);
        rc |= e->alloc(&l.w2, (int64_t)H * F); rc |= e->alloc(&l.b2, H);
        rc |= e->alloc(&l.wd2, showo_gemm_tiled_elems(H, H + F)); rc |= e->alloc(&l.bd2, H);
        rc |= e->alloc(&l.ln_w, H); rc |= e->alloc(&l.ln_b, H);
        rc |= e->alloc(&l.qln_w, 64); rc |= e->alloc(&l.qln_b, 64);
        rc |= e->alloc(&l.kln_w, 64); rc |= e->alloc(&l.kln_b, 64);
    }
    rc |= e->alloc(&e->fln_w, H); rc |= e->alloc(&e->fln_b, H);
    rc |= e->alloc(&e->wlm, (int64_t)V * H); rc |= e->alloc(&e->blm, V);
    rc |= e->alloc(&e->cosT, (int64_t)c->max_pos * c->rotary_dim);
    rc |= e->alloc(&e->sinT, (int64_t)c->max_pos * c->rotary_dim);
    const int64_t T = e->maxT;
    const int Lp = ((c->max_seq + 63) / 64) * 64;
    rc |= e->alloc(&e->x, T * H); rc |= e->alloc(&e->h, T * H); rc |= e->alloc(&e->qkv, T * 3 * H);
    rc |= e->alloc(&e->Q, T * H); rc |= e->alloc(&e->K, T * H);
    rc |= e->alloc(&e->Vt, (int64_t)c->max_batch * H * Lp);
    rc |= e->alloc(&e->attn, T * H); rc |= e->alloc(&e->ffn, T * F); rc |= e->alloc(&e->hf, (T + 64) * H);  // + 64 rows: the trainer's lm_head weight gradient reads hf up to the next multiple of 64 rows
    rc |= e->alloc(&e->iv, T * 4); rc |= e->alloc(&e->flag, 4); rc |= e->alloc(&e->rows, T);
    rc |= e->alloc(&e->t2i.ids_all, T); rc |= e->alloc(&e->t2i.cur, T); rc |= e->alloc(&e->t2i.sampled, T); rc |= e->alloc(&e->t2i.sel, T);
    rc |= e->alloc(&e->iv1, 4); rc |= e->alloc(&e->tok1, 1);
    if (rc) { showo_engine_destroy(e); return rc; }
    hipMemset(e->Vt, 0, (size_t)c->max_batch * H * Lp * sizeof(bf16_t));
    hipMemset(e->flag, 0, 16);
    e->expected = 1 + e->nL * 18 + 2 + 2 + 2;
    *out = e;
    return 0;
}

extern "C" void showo_engine_destroy(showo_engine* e) {
    if (!e) return;
    for (auto& ge : e->t2i.graphs)
        if (ge.exec) hipGraphExecDestroy(ge.exec);
    if (e->t2i.ev_pfx) hipEventDestroy(e->t2i.ev_pfx);
    if (e->t2i.pfx_host) hipHostFree(e->t2i.pfx_host);
    showo::engine_batch_free(e);
    for (void* p : e->allocs) hipFree(p);
    delete e;
}

// parity hook: the next forward calls copy the fp32 residual stream into buf [layers + 1, B*L, hidden] (slot 0 = embeddings,
// slot i = output of block i - 1); NULL switches it off.  Lets a test hold EVERY block to the oracle on the GPU's own block input.
extern "C" int showo_engine_set_collect(showo_engine* e, float* buf) {
    if (!e) return set_error_msg(1, "engine: null handle");
    e->collect = buf;
    return 0;
}

extern "C" int showo_engine_missing(const showo_engine* e) { return e ? e->expected - (int)e->loaded.size() : -1; }

static int copy_f32(float* dst, const float* src, int64_t n, int64_t expect, hipStream_t s) {
    if (n != expect) return set_error_msg(2, "engine_load: element count mismatch");
    hipError_t e = hipMemcpyAsync(dst, src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return set_error_hip(e, "hipMemcpyAsync", __FILE__, __LINE__);
    return 0;
}
// GEMM weight: bf16 image; in accuracy mode also the low half (hi + lo = w to 2^-17; hi is the same RNE rounding either way)
// Precision 2: the layer weights become IEEE-half images (saturating RNE); the lm_head keeps its (hi, lo) bf16 pair (head_rows_split).
// Precision 3: the fp32 source is quantised per output row (quant.hip) into the int8 image + scales the decode step streams, and the
// bf16 image becomes bf16(q * scale): every entry point then runs the same quantised model.
struct Q8Slot { int8_t* q = nullptr; float* scale = nullptr; int64_t N = 0, K = 0; };
static int cast_w(showo_engine* e, const std::string& key, bf16_t* dst, bf16_t* dst_lo, const float* src, int64_t n, int64_t expect, hipStream_t s,
                  bool is_head = false, Q8Slot q8 = Q8Slot()) {
    if (n != expect) return set_error_msg(2, "engine_load: element count mismatch");
    if (e->precision == 3) {
        if (!q8.q || q8.N * q8.K != n) return set_error_msg(4, "engine_load (precision 3): the int8 images are missing (showo_engine_set_precision(e, 3) makes them)");
        if (!is_head) e->img_f16 = false;
        e->q8_loaded.erase(key);
        TRY(showo::q8_quantize_rows(src, q8.N, q8.K, q8.q, q8.scale, e->q8_flags, s));
        TRY(showo::q8_dequant_bf16(q8.q, q8.scale, q8.N, q8.K, dst, s));
        e->q8_loaded.insert(key);
        return 0;
    }
    if ((e->precision == 1 || (e->precision == 2 && is_head)) && dst_lo) {
        if (!is_head) e->img_f16 = false;  // the hi half is a bf16 image (a precision-2 engine switched to 1 must not keep the fp16 flag)
        int rc = showo_split_f32_bf16(src, dst, dst_lo, n, s);
        if (!rc) e->lo_loaded.insert(key);
        return rc;
    }
    if (!is_head) e->img_f16 = e->precision == 2;
    return showo_cast_f32_op16(src, dst, n, (e->precision == 2 && !is_head) ? SHOWO_OP_F16 : SHOWO_OP_BF16, s);
}

// The seven GEMM weight kinds (q/k/v_proj, dense, fc1, fc2 of a block; lm_head): where their images live.  q8.N / q8.K are always set;
// q8.q / q8.scale once precision 3 has allocated the int8 images.
static bool gemm_weight_slot(showo_engine* e, const char* key, bf16_t** dst, bf16_t** dst_lo, Q8Slot* q8, bool* is_head) {
    const int64_t H = e->H, F = e->F, V = e->V;
    *is_head = false;
    if (!strcmp(key, "showo.lm_head.weight")) {
        *dst = e->wlm; *dst_lo = e->wlm_lo; *is_head = true;
        *q8 = Q8Slot{e->qlm, e->slm, V, H};
        return true;
    }
    int li = -1;
    char sub[128];
    if (sscanf(key, "showo.model.layers.%d.%127s", &li, sub) != 2 || li < 0 || li >= e->nL) return false;
    showo::Layer& l = e->layers[li];
    const std::string t(sub);
    int j = t == "self_attn.q_proj.weight" ? 0 : t == "self_attn.k_proj.weight" ? 1 : t == "self_attn.v_proj.weight" ? 2 : -1;
    if (j >= 0) {  // three tensors stacked in wqkv; their int8 rows and scales stack the same way
        *dst = l.wqkv + j * H * H; *dst_lo = l.wqkv_lo ? l.wqkv_lo + j * H * H : nullptr;
        *q8 = Q8Slot{l.qqkv ? l.qqkv + j * H * H : nullptr, l.sqkv ? l.sqkv + j * H : nullptr, H, H};
    } else if (t == "self_attn.dense.weight") {
        *dst = l.wd; *dst_lo = l.wd_lo; *q8 = Q8Slot{l.qd, l.sd, H, H};
    } else if (t == "mlp.fc1.weight") {
        *dst = l.w1; *dst_lo = l.w1_lo; *q8 = Q8Slot{l.q1, l.s1, F, H};
    } else if (t == "mlp.fc2.weight") {
        *dst = l.w2; *dst_lo = l.w2_lo; *q8 = Q8Slot{l.q2, l.s2, H, F};
    } else {
        return false;
    }
    return true;
}

extern "C" int showo_engine_load(showo_engine* e, const char* key, const float* src, int64_t n, void* stream) {
    if (!e || !key || !src) return set_error_msg(1, "engine_load: null argument");
    hipStream_t s = (hipStream_t)stream;
    const int64_t H = e->H, F = e->F, V = e->V;
    std::string k(key);
    int rc = -1;
    int li = -1;
    char sub[128];
    bf16_t *gdst = nullptr, *gdst_lo = nullptr;
    Q8Slot q8;
    bool is_head = false;
    if (gemm_weight_slot(e, key, &gdst, &gdst_lo, &q8, &is_head)) rc = cast_w(e, k, gdst, gdst_lo, src, n, q8.N * q8.K, s, is_head, q8);
    else if (k == "showo.model.embed_tokens.weight") rc = copy_f32(e->embed, src, n, V * H, s);
    else if (k == "showo.model.final_layernorm.weight") rc = copy_f32(e->fln_w, src, n, H, s);
    else if (k == "showo.model.final_layernorm.bias") rc = copy_f32(e->fln_b, src, n, H, s);
    else if (k == "showo.lm_head.bias") rc = copy_f32(e->blm, src, n, V, s);
    else if (k == "rope.cos") rc = copy_f32(e->cosT, src, n, (int64_t)e->cfg.max_pos * e->cfg.rotary_dim, s);
    else if (k == "rope.sin") rc = copy_f32(e->sinT, src, n, (int64_t)e->cfg.max_pos * e->cfg.rotary_dim, s);
    else if (sscanf(key, "showo.model.layers.%d.%127s", &li, sub) == 2 && li >= 0 && li < e->nL) {
        showo::Layer& l = e->layers[li];
        std::string t(sub);
        if (t == "self_attn.q_proj.bias") rc = copy_f32(l.bqkv, src, n, H, s);
        else if (t == "self_attn.k_proj.bias") rc = copy_f32(l.bqkv + H, src, n, H, s);
        else if (t == "self_attn.v_proj.bias") rc = copy_f32(l.bqkv + 2 * H, src, n, H, s);
        else if (t == "self_attn.dense.bias") rc = copy_f32(l.bd, src, n, H, s);
        else if (t == "self_attn.q_layernorm.weight") rc = copy_f32(l.qln_w, src, n, 64, s);
        else if (t == "self_attn.q_layernorm.bias") rc = copy_f32(l.qln_b, src, n, 64, s);
        else if (t == "self_attn.k_layernorm.weight") rc = copy_f32(l.kln_w, src, n, 64, s);
        else if (t == "self_attn.k_layernorm.bias") rc = copy_f32(l.kln_b, src, n, 64, s);
        else if (t == "mlp.fc1.bias") rc = copy_f32(l.b1, src, n, F, s);
        else if (t == "mlp.fc2.bias") rc = copy_f32(l.b2, src, n, H, s);
        else if (t == "input_layernorm.weight") rc = copy_f32(l.ln_w, src, n, H, s);
        else if (t == "input_layernorm.bias") rc = copy_f32(l.ln_b, src, n, H, s);
    }
    if (rc == -1) return set_error_msg(3, "engine_load: unknown state-dict key");
    if (rc == 0) e->loaded.insert(k);
    // the images made from this tensor (the fused block images -- and with them a cached t2i graph's preconditions -- and the
    // trainer's transposed images) are rebuilt by their next user
    if (uint64_t* v = showo::engine_version(e, key)) *v = ++e->clock;
    e->px3_valid = false;
    e->head3_valid = false;
    return rc;
}

extern "C" int showo_engine_load_q8(showo_engine* e, const char* key, const int8_t* q, const float* scale, int64_t N, int64_t K, void* stream) {
    if (!e || !key || !q || !scale) return set_error_msg(1, "engine_load_q8: null argument");
    if (e->precision != 3) return set_error_msg(1, "engine_load_q8: int8 images exist under precision 3 only (showo_engine_set_precision(e, 3) first)");
    hipStream_t s = (hipStream_t)stream;
    bf16_t *dst = nullptr, *dst_lo = nullptr;
    Q8Slot q8;
    bool is_head = false;
    if (!gemm_weight_slot(e, key, &dst, &dst_lo, &q8, &is_head)) return set_error_msg(3, "engine_load_q8: not a GEMM weight key");
    if (N != q8.N || K != q8.K) return set_error_msg(2, "engine_load_q8: shape mismatch");
    if (!q8.q) return set_error_msg(4, "engine_load_q8: the int8 images are missing");
    TRY(showo::q8_validate(q, scale, N, K, e->q8_flags, s));
    e->q8_loaded.erase(key);
    SHOWO_CHECK_HIP(hipMemcpyAsync(q8.q, q, (size_t)(N * K), hipMemcpyDeviceToDevice, s));
    SHOWO_CHECK_HIP(hipMemcpyAsync(q8.scale, scale, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, s));
    TRY(showo::q8_dequant_bf16(q8.q, q8.scale, N, K, dst, s));
    if (!is_head) e->img_f16 = false;
    e->q8_loaded.insert(key);
    e->loaded.insert(key);
    if (uint64_t* v = showo::engine_version(e, key)) *v = ++e->clock;  // same bookkeeping as showo_engine_load
    e->px3_valid = false;
    e->head3_valid = false;
    return 0;
}

// Destination of a state-dict tensor inside the engine, without copying: bf16 weight image OR fp32 vector (exactly one is set).
// Used by the trainer's fused optimizer step, which writes the refreshed images itself (train_engine.hip).
extern "C" int showo_engine_slot(showo_engine* e, const char* key, int64_t n, uint16_t** dst_bf16, float** dst_f32) {
    if (!e || !key || !dst_bf16 || !dst_f32) return set_error_msg(1, "engine_slot: null argument");
    const int64_t H = e->H, F = e->F, V = e->V;
    *dst_bf16 = nullptr; *dst_f32 = nullptr;
    std::string k(key);
    int64_t expect = -1;
    int li = -1;
    char sub[128];
    if (k == "showo.model.embed_tokens.weight") { *dst_f32 = e->embed; expect = V * H; }
    else if (k == "showo.model.final_layernorm.weight") { *dst_f32 = e->fln_w; expect = H; }
    else if (k == "showo.model.final_layernorm.bias") { *dst_f32 = e->fln_b; expect = H; }
    else if (k == "showo.lm_head.weight") { *dst_bf16 = e->wlm; expect = V * H; }
    else if (k == "showo.lm_head.bias") { *dst_f32 = e->blm; expect = V; }
    else if (sscanf(key, "showo.model.layers.%d.%127s", &li, sub) == 2 && li >= 0 && li < e->nL) {
        showo::Layer& l = e->layers[li];
        std::string t(sub);
        if (t == "self_attn.q_proj.weight") { *dst_bf16 = l.wqkv; expect = H * H; }
        else if (t == "self_attn.k_proj.weight") { *dst_bf16 = l.wqkv + H * H; expect = H * H; }
        else if (t == "self_attn.v_proj.weight") { *dst_bf16 = l.wqkv + 2 * H * H; expect = H * H; }
        else if (t == "self_attn.q_proj.bias") { *dst_f32 = l.bqkv; expect = H; }
        else if (t == "self_attn.k_proj.bias") { *dst_f32 = l.bqkv + H; expect = H; }
        else if (t == "self_attn.v_proj.bias") { *dst_f32 = l.bqkv + 2 * H; expect = H; }
        else if (t == "self_attn.dense.weight") { *dst_bf16 = l.wd; expect = H * H; }
        else if (t == "self_attn.dense.bias") { *dst_f32 = l.bd; expect = H; }
        else if (t == "self_attn.q_layernorm.weight") { *dst_f32 = l.qln_w; expect = 64; }
        else if (t == "self_attn.q_layernorm.bias") { *dst_f32 = l.qln_b; expect = 64; }
        else if (t == "self_attn.k_layernorm.weight") { *dst_f32 = l.kln_w; expect = 64; }
        else if (t == "self_attn.k_layernorm.bias") { *dst_f32 = l.kln_b; expect = 64; }
        else if (t == "mlp.fc1.weight") { *dst_bf16 = l.w1; expect = F * H; }
        else if (t == "mlp.fc1.bias") { *dst_f32 = l.b1; expect = F; }
        else if (t == "mlp.fc2.weight") { *dst_bf16 = l.w2; expect = H * F; }
        else if (t == "mlp.fc2.bias") { *dst_f32 = l.b2; expect = H; }
        else if (t == "input_layernorm.weight") { *dst_f32 = l.ln_w; expect = H; }
        else if (t == "input_layernorm.bias") { *dst_f32 = l.ln_b; expect = H; }
    }
    if (expect < 0) return set_error_msg(3, "engine_slot: unknown state-dict key");
    if (expect != n) return set_error_msg(2, "engine_slot: element count mismatch");
    return 0;
}
// the caller rewrote weight images through showo_engine_slot pointers: same bookkeeping as showo_engine_load
extern "C" int showo_engine_weights_touched(showo_engine* e) {
    if (!e) return set_error_msg(1, "engine: null handle");
    showo::engine_bump_all(e);
    e->px3_valid = false;
    e->head3_valid = false;
    e->lo_loaded.clear();  // the hi images were rewritten without their low halves: accuracy mode needs a re-upload
    e->img_f16 = false;    // the trainer writes bf16 images: a precision-2 engine needs a re-upload too (run_layers checks)
    e->q8_loaded.clear();  // ... and the int8 images of precision 3 no longer match them
    return 0;
}

uint64_t* showo::engine_version(showo_engine* e, const char* key) {
    if (!strcmp(key, "showo.lm_head.weight")) return &e->ver_wlm;
    int li = -1;
    char sub[128];
    if (sscanf(key, "showo.model.layers.%d.%127s", &li, sub) != 2 || li < 0 || li >= e->nL) return nullptr;
    showo::Layer& l = e->layers[li];
    const char* names[6] = {nullptr, "self_attn.dense.weight", "mlp.fc1.weight", "mlp.fc2.weight", "self_attn.dense.bias", "mlp.fc2.bias"};
    if (!strcmp(sub, "self_attn.q_proj.weight") || !strcmp(sub, "self_attn.k_proj.weight") || !strcmp(sub, "self_attn.v_proj.weight")) return &l.ver[0];
    for (int j = 1; j < 6; ++j)
        if (!strcmp(sub, names[j])) return &l.ver[j];
    return nullptr;
}

void showo::engine_bump_all(showo_engine* e) {
    const uint64_t v = ++e->clock;
    for (auto& l : e->layers)
        for (uint64_t& x : l.ver) x = v;
    e->ver_wlm = v;
}

static bool block_stale(const showo::Layer& l) { return l.fused_at == 0 || *std::max_element(l.ver, l.ver + 6) > l.fused_at; }

bool showo::engine_fused_stale(const showo_engine* e) {
    for (auto& l : e->layers)
        if (block_stale(l)) return true;
    return false;
}

namespace {
__global__ void add2_f32_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ o, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = a[i] + b[i];
}
}  // namespace

// SHOWO_W_TILED=0 keeps the fused projections on row-major weights (A/B runs)
static bool w_tiled_enabled() {
    static int v = -1;
    if (v < 0) {
        const char* env = getenv("SHOWO_W_TILED");
        v = env ? (atoi(env) != 0) : 1;
    }
    return v != 0;
}

// Weight images of the two fused projections, rebuilt for every block whose wqkv / wd / w1 / w2 / bd / b2 changed since they were built:
//   wd2  = [Wd | W2] ([H, H + F], K-concatenated) for showo_gemm_kcat_bf16, bd2 = bd + b2;
//   wq1t = tiled copy of [Wqkv ; W1] (showo_gemm_tile_weight) -- with SHOWO_W_TILED (default) wd2 is stored tiled as well
int showo::fused_sync(showo_engine* e, hipStream_t s) {
    if (!showo::engine_fused_stale(e)) return 0;
    const int H = e->H, F = e->F;
    const bool tiled = w_tiled_enabled();
    if (tiled && !e->wtmp) TRY(e->alloc(&e->wtmp, (int64_t)H * (H + F)));
    for (auto& l : e->layers) {
        if (!block_stale(l)) continue;
        bf16_t* cat = tiled ? e->wtmp : l.wd2;
        SHOWO_CHECK_HIP(hipMemcpy2DAsync(cat, (size_t)(H + F) * 2, l.wd, (size_t)H * 2, (size_t)H * 2, H, hipMemcpyDeviceToDevice, s));
        SHOWO_CHECK_HIP(hipMemcpy2DAsync(cat + H, (size_t)(H + F) * 2, l.w2, (size_t)F * 2, (size_t)F * 2, H, hipMemcpyDeviceToDevice, s));
        if (tiled) {
            TRY(showo_gemm_tile_weight(cat, H + F, H, H + F, l.wd2, s));
            if (!l.wq1t) TRY(e->alloc(&l.wq1t, showo_gemm_tiled_elems(3 * H + F, H)));
            TRY(showo_gemm_tile_weight(l.wqkv, H, 3 * H + F, H, l.wq1t, s));
        }
        add2_f32_kernel<<<dim3((H + 255) / 256), dim3(256), 0, s>>>(l.bd, l.b2, l.bd2, H);
        l.fused_at = std::max<uint64_t>(e->clock, 1);
        ++e->fused_rebuilt;
    }
    SHOWO_CHECK_HIP(hipGetLastError());
    e->fused_tiled = tiled;
    return 0;
}

// SHOWO_FUSED_LAYER=0 restores the four-GEMM layer (A/B runs)
static bool fused_layer_enabled() {
    static int v = -1;
    if (v < 0) {
        const char* env = getenv("SHOWO_FUSED_LAYER");
        v = env ? (atoi(env) != 0) : 1;
    }
    return v != 0;
}

// ---- the 24-layer stack.  K / V^T go to a KVDest (engine.h): the per-call workspace here, or a per-layer cache.
KVDest showo::kv_workspace(showo_engine* e, int L) { return KVDest{e->K, e->Vt, 0, 0, L, ((L + 63) / 64) * 64, e->p_Klo, e->p_Vtlo}; }
namespace showo { int g_decode_impl = 0; }
static int g_decode_chain = 0;  // 1: the fused layer as a plain three-launch chain (no co-scheduled fc2 role)
extern "C" int showo_decode_set_impl(int impl) {
    if (impl < 0 || impl > 2) return set_error_msg(1, "decode_set_impl: 0 = fused layer (default), 1 = unfused, 2 = fused chain without the co-scheduled fc2 role");
    showo::g_decode_impl = impl == 1;
    g_decode_chain = impl == 2;
    return 0;
}

// parity hook (showo_engine_set_collect): copy the fp32 residual stream after layer `slot - 1` (slot 0 = the embeddings)
static int collect_x(showo_engine* e, int slot, int T, hipStream_t s) {
    if (!e->collect) return 0;
    SHOWO_CHECK_HIP(hipMemcpyAsync(e->collect + (int64_t)slot * T * e->H, e->x, (size_t)T * e->H * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

// ---- Infinity-Cache prefetch plan of the decode layers (decode_common.h, prefetch_role) -------------------------------------------
static int g_pf_mb = -1, g_pf_dense = 0, g_pf_blocks = 64;  // off by default (measured negative: profiles/r5_decode_dot2_sweep.txt)
static void decode_prefetch_env() {
    if (g_pf_mb >= 0) return;
    g_pf_mb = env_flag("SHOWO_DECODE_PF_MB", 0);
    if (g_pf_mb < 0) g_pf_mb = 0;
    g_pf_dense = env_flag("SHOWO_DECODE_PF_DENSE", g_pf_dense) != 0;
    const int b = env_flag("SHOWO_DECODE_PF_BLOCKS", 0);
    if (b > 0) g_pf_blocks = b;
}
extern "C" int showo_decode_set_prefetch(int next_mb, int dense, int blocks) {
    if (next_mb < 0 || blocks < 0 || blocks > 1024) return set_error_msg(1, "showo_decode_set_prefetch: next_mb >= 0, 0 <= blocks <= 1024");
    decode_prefetch_env();
    g_pf_mb = next_mb;
    g_pf_dense = dense != 0;
    g_pf_blocks = blocks;
    return 0;
}
namespace showo {
DecodeTuning& decode_tuning() {
    static DecodeTuning t;
    static bool init = false;
    if (!init) {
        init = true;
        auto env = [](const char* name, int* v) { const char* e = getenv(name); if (e && atoi(e) > 0) *v = atoi(e); };
        env("SHOWO_DECODE_CO_BLOCKS", &t.co_blocks);
        env("SHOWO_DECODE_BATCH_CO_BLOCKS", &t.batch_co_blocks);
        env("SHOWO_DECODE_BATCH_LN_BLOCKS", &t.batch_ln_blocks);
        env("SHOWO_DECODE_LN_BLOCKS", &t.ln_blocks);
        env("SHOWO_DECODE_OUT_BLOCKS", &t.out_blocks);
        env("SHOWO_DECODE_WIDE_LN_BLOCKS", &t.wide_ln_blocks);
        env("SHOWO_DECODE_WIDE_OUT_KSPLIT", &t.wide_out_ksplit);
    }
    return t;
}
}  // namespace showo
extern "C" int showo_decode_set_tuning(const char* name, int value) {
    if (!name || value < 1 || value > 65535) return set_error_msg(1, "showo_decode_set_tuning: name and 1 <= value <= 65535");
    showo::DecodeTuning& t = showo::decode_tuning();
    const std::string n(name);
    if (n == "co_blocks") t.co_blocks = value;
    else if (n == "batch_co_blocks") t.batch_co_blocks = value;
    else if (n == "batch_ln_blocks") t.batch_ln_blocks = value;
    else if (n == "ln_blocks") t.ln_blocks = value;
    else if (n == "out_blocks") t.out_blocks = value;
    else if (n == "wide_ln_blocks") t.wide_ln_blocks = value;
    else if (n == "wide_out_ksplit") t.wide_out_ksplit = value;
    else return set_error_msg(1, "showo_decode_set_tuning: unknown knob");
    return 0;
}
namespace showo {
void decode_prefetch_plan(const ::showo_engine* e, int li, DecodePrefetch* pf) {
    decode_prefetch_env();
    *pf = DecodePrefetch{};
    if ((g_pf_mb == 0 && !g_pf_dense) || g_pf_blocks == 0) return;
    const int64_t H = e->H, F = e->F;
    int n = 0;
    if (g_pf_dense) { pf->p[n] = e->layers[li].wd; pf->bytes[n] = H * H * 2; ++n; }
    int64_t left = (int64_t)g_pf_mb << 20;
    auto add = [&](const void* p, int64_t bytes) {
        if (left <= 0 || !p) return;
        const int64_t b = (bytes < left ? bytes : left) & ~(int64_t)15;
        pf->p[n] = p; pf->bytes[n] = b; ++n;
        left -= b;
    };
    if (li + 1 < e->nL) {
        add(e->layers[li + 1].wqkv, 3 * H * H * 2);
        if (n < 3) add(e->layers[li + 1].w1, F * H * 2);
    } else {
        add(e->wlm, (int64_t)e->V * H * 2);
    }
    pf->blocks = n ? g_pf_blocks : 0;
}
}  // namespace showo


// ---- accuracy mode ----------------------------------------------------------------------------------------------------------------
// Two implementations.  (1) precise.hip (run_layers_precise): split-bf16 GEMMs on the 128^2 kernel, everything between them in fp32 on
// the vector ALU: any shape, slow.  (2) run_layers_precise_fast (round 5): the PRODUCTION kernels on K-concatenated split images.  A
// split-precision product a w = a_hi w_hi + a_lo w_hi + a_hi w_lo is ONE bf16 GEMM over K' = 3K between A' = [a_hi | a_lo | a_hi] and
// W' = [w_hi | w_hi | w_lo] with the fp32 accumulation the MFMA does anyway, so gemm2p / gemm3w run unchanged (tile tuner, tiled
// weights, split-K, the K-concatenated residual form); only the fused projection epilogue (epilogue_qkv_split: outputs as (hi, lo)
// pairs, IEEE gelu) and the attention (attn_lds_body<SPLIT>: three MFMAs per fragment pair) have accuracy-mode forms.  A layer is
// the same two GEMM launches + attention as in precision 0, so prefix reuse, hipGraph replay and the KV cache all apply.
static int g_precise_fast = -1;  // -1: read SHOWO_PRECISE_FAST once (default on); 0 / 1: showo_precise_set_fast
extern "C" int showo_precise_set_fast(int on) { g_precise_fast = on ? 1 : 0; return 0; }
static bool precise_fast_shape_ok(const showo_engine* e) {
    if (g_precise_fast < 0) { const char* env = getenv("SHOWO_PRECISE_FAST"); g_precise_fast = env ? (atoi(env) != 0) : 1; }
    return g_precise_fast && e->cfg.rotary_dim == 32 && (3 * e->H) % 256 == 0 && e->H % 64 == 0 && e->F % 64 == 0 && e->H % 4 == 0;
}
// ... and its images / workspaces exist (showo_engine_set_precision(e, 1) made them)
bool showo::precise_fast_ok(const showo_engine* e) { return precise_fast_shape_ok(e) && e->p_h3 != nullptr; }
extern "C" int showo_engine_set_precision(showo_engine* e, int precision) {
    if (!e) return set_error_msg(1, "engine: null handle");
    if (precision < 0 || precision > 3)
        return set_error_msg(1, "engine_set_precision: 0 = bf16 operands, 1 = split bf16 (fp32-class), 2 = fp16 operands, 3 = int8 decode weights");
    if (precision == 3) {
        // the int8 rows are read by the fused decode step alone: without it the mode would silently be precision 0 on rounded weights
        if (!showo::decode_fused_shapes_ok(e->H, e->F) || e->H % 16 || e->F % 16)
            return set_error_msg(1, "engine_set_precision(3): the int8 decode needs hidden <= 2048 and ffn <= 8192, both multiples of 16");
        if (!e->qlm) {  // int8 images + row scales, allocated on first use: 1 byte per GEMM weight next to the bf16 images
            const int64_t H = e->H, F = e->F, V = e->V;
            int rc = 0;
            for (auto& l : e->layers) {
                rc |= e->alloc(&l.qqkv, (3 * H + F) * H); rc |= e->alloc(&l.sqkv, 3 * H + F);
                if (!rc) { l.q1 = l.qqkv + 3 * H * H; l.s1 = l.sqkv + 3 * H; }
                rc |= e->alloc(&l.qd, H * H); rc |= e->alloc(&l.sd, H);
                rc |= e->alloc(&l.q2, H * F); rc |= e->alloc(&l.s2, H);
            }
            rc |= e->alloc(&e->slm, V);
            if (!e->q8_flags) rc |= e->alloc(&e->q8_flags, 2);
            if (!rc) rc |= e->alloc(&e->qlm, V * H);
            if (rc) {
                for (auto& l : e->layers) { e->release(&l.qqkv); e->release(&l.sqkv); e->release(&l.qd); e->release(&l.sd); e->release(&l.q2); e->release(&l.s2); l.q1 = nullptr; l.s1 = nullptr; }
                e->release(&e->slm); e->release(&e->qlm);
                return rc;
            }
        }
    }
    if (precision == 2 && !e->wlm3) {  // the lm_head of precision 2 is a split-bf16 product: its low half, [hi | hi | lo] image and LayerNorm workspace
        const int64_t H = e->H, V = e->V, T = e->maxT;
        int rc = 0;
        if (!e->wlm_lo) rc |= e->alloc(&e->wlm_lo, V * H);
        if (!e->p_hf3) rc |= e->alloc(&e->p_hf3, (T + 256) * 3 * H);
        if (!rc) rc |= e->alloc(&e->wlm3, V * 3 * H);
        if (rc) { e->release(&e->wlm3); return rc; }
        e->head3_valid = false;
    }
    // what the GEMM weight images hold: bf16(w) (precision 0 / 1), fp16(w) (2), bf16 of the int8-dequantised w (3)
    auto img_class = [](int p) { return p == 2 ? 2 : p == 3 ? 3 : 0; };
    if (img_class(precision) != img_class(e->precision)) {
        // the layer weight images change their element type or their values: un-load every GEMM weight so that the host uploads them
        // again (showo_engine_missing() > 0 until it has); cached t2i graphs are keyed on the precision and simply miss
        for (auto it = e->loaded.begin(); it != e->loaded.end();) {
            const std::string& k = *it;
            const bool gemm_w = k.size() > 7 && k.compare(k.size() - 7, 7, ".weight") == 0 &&
                                (k.find("_proj.") != std::string::npos || k.find(".dense.") != std::string::npos || k.find(".fc1.") != std::string::npos ||
                                 k.find(".fc2.") != std::string::npos || k == "showo.lm_head.weight");
            if (gemm_w) it = e->loaded.erase(it); else ++it;
        }
        e->lo_loaded.clear();
        e->q8_loaded.clear();
        showo::engine_bump_all(e); e->px3_valid = false; e->head3_valid = false;
    }
    if (precision == 1 && !e->p_hlo) {  // low halves of every GEMM weight + fp32 workspaces, allocated on first use
        const int64_t H = e->H, F = e->F, V = e->V, T = e->maxT;
        int rc = 0;
        for (auto& l : e->layers) {
            rc |= e->alloc(&l.wqkv_lo, (3 * H + F) * H);
            if (!rc) l.w1_lo = l.wqkv_lo + 3 * H * H;
            rc |= e->alloc(&l.wd_lo, H * H);
            rc |= e->alloc(&l.w2_lo, H * F);
        }
        rc |= e->alloc(&e->p_hlo, T * H); rc |= e->alloc(&e->p_actlo, T * F);
        rc |= e->alloc(&e->p_qkv, T * 3 * H); rc |= e->alloc(&e->p_f, T * F);
        rc |= e->alloc(&e->p_Q, T * H); rc |= e->alloc(&e->p_K, T * H); rc |= e->alloc(&e->p_V, T * H); rc |= e->alloc(&e->p_a, T * H);
        if (!e->wlm_lo) rc |= e->alloc(&e->wlm_lo, V * H);
        if (rc) return rc;
    }
    if (precision == 1 && precise_fast_shape_ok(e) && !e->p_h3) {  // K-concatenated split images + workspaces of the production-kernel path
        const int64_t H = e->H, F = e->F, V = e->V, T = e->maxT, HF = H + F;
        const int64_t Lp = ((e->cfg.max_seq + 63) / 64) * 64;
        int rc = 0;
        for (auto& l : e->layers) {
            rc |= e->alloc(&l.wq1x3, showo_gemm_tiled_elems((int)(3 * H + F), (int)(3 * H)));
            rc |= e->alloc(&l.wd2x3, showo_gemm_tiled_elems((int)H, (int)(3 * HF)));
        }
        const int64_t t1 = (3 * H + F) * 3 * H, t2 = H * 3 * HF;
        rc |= e->alloc(&e->wtmp3, t1 > t2 ? t1 : t2);
        rc |= e->alloc(&e->p_h3, (T + 256) * 3 * H);
        if (!e->p_hf3) rc |= e->alloc(&e->p_hf3, (T + 256) * 3 * H);
        rc |= e->alloc(&e->p_act, (T + 256) * 2 * HF);
        rc |= e->alloc(&e->p_Qlo, T * H); rc |= e->alloc(&e->p_Klo, T * H);
        rc |= e->alloc(&e->p_Vtlo, (int64_t)e->cfg.max_batch * H * Lp);
        if (!e->wlm3) rc |= e->alloc(&e->wlm3, V * 3 * H);
        if (rc) {  // a partial set must not survive (wlm3 == NULL would re-allocate everything at the next call)
            for (auto& l : e->layers) { e->release(&l.wq1x3); e->release(&l.wd2x3); }
            e->release(&e->wtmp3); e->release(&e->p_h3); e->release(&e->p_act); e->release(&e->p_Qlo); e->release(&e->p_Klo);
            e->release(&e->p_Vtlo);
            return rc;
        }
        hipMemset(e->p_Vtlo, 0, (size_t)e->cfg.max_batch * H * Lp * sizeof(bf16_t));
        e->px3_valid = false;
    }
    e->precision = precision;
    return 0;
}
// 1 when accuracy mode runs on the production kernels (K-concatenated split images): prefix reuse, hipGraph replay and the KV-cached
// decode are then available in precision 1 as well; 0: the fp32 reference kernels of precise.hip (small / odd shapes, SHOWO_PRECISE_FAST=0)
extern "C" int showo_engine_precise_fast(const showo_engine* e) { return e && precise_fast_ok(e) ? 1 : 0; }
// 1 when every GEMM weight has a current low half (q, k, v, dense, fc1, fc2 per layer + lm_head), i.e. precision 1 can run
extern "C" int showo_engine_precise_ready(const showo_engine* e) {
    return e && e->wlm_lo && e->p_hlo && (int)e->lo_loaded.size() == e->nL * 6 + 1;
}
extern "C" int showo_engine_get_precision(const showo_engine* e) { return e ? e->precision : -1; }

static int precise_check(showo_engine* e) {
    if (!showo_engine_precise_ready(e))
        return set_error_msg(4, "engine (precision 1): the low halves of the weights are missing or stale (weights were loaded before "
                                "showo_engine_set_precision(e, 1), or rewritten by the trainer): upload the weights again");
    return 0;
}

// One pass over the layer stack in accuracy mode.  Same operation order as models/phi.py:774-790; the two residual adds land as
// (x + dense(attn)) + fc2(gelu(fc1(h))) (fp32 either way).  K / V of the call live in the fp32 workspace: no KV cache in this mode.
static int run_layers_precise(showo_engine* e, int B, int L, const int32_t* iv, const int32_t* flag, const float* dense, hipStream_t s) {
    const int H = e->H, F = e->F, nH = e->nH, T = B * L;
    TRY(precise_check(e));
    if (e->cfg.rotary_dim != 32) return set_error_msg(1, "engine (precision 1): rotary_dim 32 only");
    TRY(collect_x(e, 0, T, s));
    for (int li = 0; li < e->nL; ++li) {
        showo::Layer& l = e->layers[li];
        TRY(showo::precise_ln_split(e->x, l.ln_w, l.ln_b, nullptr, e->h, e->p_hlo, T, H, e->cfg.ln_eps, s));
        TRY(showo_gemm_bf16x3(e->h, e->p_hlo, H, l.wqkv, l.wqkv_lo, H, l.bqkv, 0, e->p_qkv, 3 * H, nullptr, 0, T, 3 * H, H, s));
        TRY(showo::precise_qk_prep(e->p_qkv, l.qln_w, l.qln_b, l.kln_w, l.kln_b, e->cosT, e->sinT, e->p_Q, e->p_K, e->p_V, B, L, nH,
                                   e->cfg.ln_eps, 0, L, s));
        TRY(showo::precise_attention(e->p_Q, e->p_K, e->p_V, iv, flag, dense, e->p_a, B, nH, L, L, L, H, s));
        TRY(showo_split_f32_bf16(e->p_a, e->attn, e->p_actlo, (int64_t)T * H, s));
        TRY(showo_gemm_bf16x3(e->attn, e->p_actlo, H, l.wd, l.wd_lo, H, l.bd, 0, e->x, H, e->x, H, T, H, H, s));
        TRY(showo_gemm_bf16x3(e->h, e->p_hlo, H, l.w1, l.w1_lo, H, l.b1, 0, e->p_f, F, nullptr, 0, T, F, H, s));
        TRY(showo::precise_gelu_split(e->p_f, e->ffn, e->p_actlo, (int64_t)T * F, s));
        TRY(showo_gemm_bf16x3(e->ffn, e->p_actlo, F, l.w2, l.w2_lo, F, l.b2, 0, e->x, H, e->x, H, T, H, F, s));
        TRY(collect_x(e, li + 1, T, s));
    }
    return 0;
}
static int head_rows_precise(showo_engine* e, const int32_t* rows, int nrows, int col0, int ncols, float* logits, hipStream_t s) {
    TRY(precise_check(e));
    TRY(showo::precise_ln_split(e->x, e->fln_w, e->fln_b, rows, e->hf, e->p_hlo, nrows, e->H, e->cfg.ln_eps, s));
    return showo_gemm_bf16x3(e->hf, e->p_hlo, e->H, e->wlm + (int64_t)col0 * e->H, e->wlm_lo + (int64_t)col0 * e->H, e->H, e->blm + col0, 0,
                             logits, ncols, nullptr, 0, nrows, ncols, e->H, s);
}

// [hi | hi | lo] rows of the lm_head (precision 1 and 2: the head is a split-bf16 product in both); never inside a capture
int showo::head3_sync(showo_engine* e, hipStream_t s) {
    if (e->head3_valid) return 0;
    if (!e->wlm3 || !e->wlm_lo || !e->lo_loaded.count("showo.lm_head.weight"))
        return set_error_msg(4, "engine: the low half of the lm_head is missing or stale (the weights were loaded before "
                                "showo_engine_set_precision(e, 1 | 2), or rewritten by the trainer): upload the weights again");
    const int64_t H = e->H, V = e->V;
    SHOWO_CHECK_HIP(hipMemcpy2DAsync(e->wlm3, (size_t)3 * H * 2, e->wlm, (size_t)H * 2, (size_t)H * 2, (size_t)V, hipMemcpyDeviceToDevice, s));
    SHOWO_CHECK_HIP(hipMemcpy2DAsync(e->wlm3 + H, (size_t)3 * H * 2, e->wlm, (size_t)H * 2, (size_t)H * 2, (size_t)V, hipMemcpyDeviceToDevice, s));
    SHOWO_CHECK_HIP(hipMemcpy2DAsync(e->wlm3 + 2 * H, (size_t)3 * H * 2, e->wlm_lo, (size_t)H * 2, (size_t)H * 2, (size_t)V, hipMemcpyDeviceToDevice, s));
    e->head3_valid = true;
    return 0;
}
// K-concatenated split images of every GEMM weight (see "accuracy mode" above), rebuilt after any weight load; never inside a capture
int showo::precise_sync(showo_engine* e, hipStream_t s) {
    if (e->px3_valid) return 0;
    TRY(precise_check(e));
    TRY(fused_sync(e, s));  // bd2 = bd + b2
    const int64_t H = e->H, F = e->F, V = e->V, HF = H + F;
    auto cp = [&](bf16_t* dst, int64_t ldd, const bf16_t* src, int64_t lds, int64_t cols, int64_t rows) -> int {
        SHOWO_CHECK_HIP(hipMemcpy2DAsync(dst, (size_t)ldd * 2, src, (size_t)lds * 2, (size_t)cols * 2, (size_t)rows, hipMemcpyDeviceToDevice, s));
        return 0;
    };
    for (auto& l : e->layers) {
        bf16_t* cat = e->wtmp3;
        // [Wqkv ; W1] rows -> [w_hi | w_hi | w_lo]  (wqkv / w1 and their low halves are one allocation each)
        TRY(cp(cat, 3 * H, l.wqkv, H, H, 3 * H + F));
        TRY(cp(cat + H, 3 * H, l.wqkv, H, H, 3 * H + F));
        TRY(cp(cat + 2 * H, 3 * H, l.wqkv_lo, H, H, 3 * H + F));
        TRY(showo_gemm_tile_weight(cat, (int)(3 * H), (int)(3 * H + F), (int)(3 * H), l.wq1x3, s));
        // [Wd | W2] rows -> [Wd_hi | W2_hi | Wd_hi | W2_hi | Wd_lo | W2_lo] against act = [attn_hi | ffn_hi | attn_lo | ffn_lo | attn_hi | ffn_hi]
        for (int rep = 0; rep < 3; ++rep) {
            TRY(cp(cat + rep * HF, 3 * HF, rep == 2 ? l.wd_lo : l.wd, H, H, H));
            TRY(cp(cat + rep * HF + H, 3 * HF, rep == 2 ? l.w2_lo : l.w2, F, F, H));
        }
        TRY(showo_gemm_tile_weight(cat, (int)(3 * HF), (int)H, (int)(3 * HF), l.wd2x3, s));
    }
    TRY(head3_sync(e, s));
    e->px3_valid = true;
    return 0;
}

// One pass over the layer stack in accuracy mode on the production kernels: LayerNorm -> [hi | lo | hi]; ONE [Wqkv ; W1] projection
// (K' = 3H) whose epilogue writes Q / K / V^T and gelu(fc1) as (hi, lo) pairs; split attention; ONE K-concatenated residual GEMM
// (K' = 3 (H + F)) over act = [attn_hi | ffn_hi | attn_lo | ffn_lo] read as [act | act[:, :H + F]].  Any T >= 1, any KV destination.
static int run_layers_precise_fast(showo_engine* e, int B, int L, int pos0, const KVDest& kv, const int32_t* iv, const int32_t* flag,
                                   const float* dense, hipStream_t s) {
    const int H = e->H, F = e->F, nH = e->nH, T = B * L, HF = H + F, lda = 2 * HF;
    if (!kv.k_lo || !kv.vt_lo) return set_error_msg(7, "engine (precision 1): the low-half K / V^T destination is missing");
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    hipStreamIsCapturing(s, &cs);
    if (!e->px3_valid && cs != hipStreamCaptureStatusNone) return set_error_msg(7, "engine (precision 1): split weight images must be built before a stream capture");
    TRY(precise_sync(e, s));
    TRY(collect_x(e, 0, T, s));
    const int Lk = pos0 + L;
    for (int li = 0; li < e->nL; ++li) {
        showo::Layer& l = e->layers[li];
        bf16_t* Kd = kv.k + li * kv.k_lstride;
        bf16_t* Vd = kv.vt + li * kv.v_lstride;
        bf16_t* Kl = kv.k_lo + li * kv.k_lstride;
        bf16_t* Vl = kv.vt_lo + li * kv.v_lstride;
        TRY(showo::precise_ln_split3(e->x, l.ln_w, l.ln_b, nullptr, e->p_h3, T, H, e->cfg.ln_eps, s));
        TRY(showo_gemm_qkv_fc1_split(e->p_h3, 3 * H, l.wq1x3, 3 * H, 3 * H, l.bqkv, l.qln_w, l.qln_b, l.kln_w, l.kln_b, e->cosT, e->sinT,
                                     e->Q, e->p_Qlo, Kd, Kl, Vd, Vl, e->p_act + H, e->p_act + HF + H, lda, F, B, L, nH, e->cfg.rotary_dim,
                                     e->cfg.ln_eps, pos0, kv.Lcap, kv.Lp, 1, s));
        TRY(showo_attn_fwd_split(e->Q, e->p_Qlo, Kd, Kl, Vd, Vl, iv, flag, dense, e->p_act, e->p_act + HF, B, nH, L, Lk, kv.Lcap, kv.Lp, lda, s));
        TRY(showo_gemm_kcat_bf16(e->p_act, lda, 2 * HF, e->p_act, lda, HF, l.wd2x3, 3 * HF, l.bd2, e->x, H, e->x, H, T, H,
                                 SHOWO_EPI_RESID_F32, 1, s));
        TRY(collect_x(e, li + 1, T, s));
    }
    return 0;
}
// final LayerNorm -> [hi | lo | hi], lm_head rows [hi | hi | lo]: ONE bf16 GEMM over 3H (precision 1 on the production kernels, and the
// head of precision 2: final hidden state and lm_head weight are then not rounding points at all, oracle/predict_rounding.py)
static int head_rows_precise_fast(showo_engine* e, const int32_t* rows, int nrows, int col0, int ncols, float* logits, hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    hipStreamIsCapturing(s, &cs);
    if (e->precision == 2) {
        if (!e->head3_valid && cs != hipStreamCaptureStatusNone) return set_error_msg(7, "engine (precision 2): the lm_head image must be built before a stream capture");
        TRY(head3_sync(e, s));
    } else {
        if (!e->px3_valid && cs != hipStreamCaptureStatusNone) return set_error_msg(7, "engine (precision 1): split weight images must be built before a stream capture");
        TRY(precise_sync(e, s));
    }
    const int H = e->H;
    TRY(showo::precise_ln_split3(e->x, e->fln_w, e->fln_b, rows, e->p_hf3, nrows, H, e->cfg.ln_eps, s));
    return showo_gemm_bf16(e->p_hf3, 3 * H, e->wlm3 + (int64_t)col0 * 3 * H, 3 * H, e->blm + col0, 0, logits, ncols, nullptr, 0, nrows, ncols,
                           3 * H, SHOWO_EPI_F32, s);
}

// precision 2 range check (showo_engine_set_range_check): count the elements of a freshly written 16-bit activation that sit at the
// fp16 saturation value (or are inf / NaN).  Off (one pointer test) unless a counter is registered; never inside the timed path.
static int range_check(showo_engine* e, const bf16_t* x, int64_t n, hipStream_t s) {
    if (!e->range_count || e->precision != 2) return 0;
    return showo_count_f16_saturated(x, n, e->range_count, s);
}
extern "C" int showo_engine_set_range_check(showo_engine* e, int64_t* count) {
    if (!e) return set_error_msg(1, "engine: null handle");
    e->range_count = count;
    return 0;
}

int showo::run_layers(showo_engine* e, int B, int L, int pos0, const KVDest& kv, const int32_t* iv, const int32_t* flag,
                      const float* dense, hipStream_t s) {
    const int H = e->H, F = e->F, nH = e->nH;
    const int T = B * L;
    if (e->precision == 1) {
        if (precise_fast_ok(e)) return run_layers_precise_fast(e, B, L, pos0, kv, iv, flag, dense, s);
        if (pos0 != 0 || kv.k != e->K) return set_error_msg(1, "engine (precision 1): KV-cached calls need the production-kernel form of accuracy mode (showo_engine_precise_fast)");
        return run_layers_precise(e, B, L, iv, flag, dense, s);
    }
    // precision 2: the same launches with IEEE-half operands (op = SHOWO_OP_F16 on every 16-bit operand, weight image and activation)
    const int op = e->precision == 2 ? SHOWO_OP_F16 : SHOWO_OP_BF16;
    if ((op == SHOWO_OP_F16) != e->img_f16)
        return set_error_msg(4, "engine: the weight images hold the other 16-bit type (loaded under another precision, or rewritten by the "
                                "trainer): upload the weights again");
    // precision 3: bf16 operands on the images of the dequantised weights; the fused decode step below streams the int8 images instead
    const bool q8 = e->precision == 3;
    if (q8 && (int)e->q8_loaded.size() != e->nL * 6 + 1)
        return set_error_msg(4, "engine (precision 3): the int8 weight images are missing or stale (the weights were loaded before "
                                "showo_engine_set_precision(e, 3), or rewritten by the trainer): upload the weights again");
    TRY(collect_x(e, 0, T, s));
    const int Lk = pos0 + L;
    const int Lcap = kv.Lcap, Lp = kv.Lp;
    // a decode step that the fused layer cannot take would be served from the bf16 images at 2 bytes per weight: refused, not silent
    // (showo_decode_set_impl(1) asks for that layer explicitly; a one-token forward with a dense mask is not a decode step)
    if (q8 && T == 1 && showo::g_decode_impl == 0 && !dense && (size_t)Lcap * 4 + 2048 > 60000)
        return set_error_msg(5, "engine (precision 3): the int8 decode step serves KV caches of up to 14 488 tokens");
    // (the fused three-launch decode layer of decode.hip has instances for both operand types since round 6)
    if (T == 1 && showo::g_decode_impl == 0 && !dense && showo::decode_fused_shapes_ok(H, F) && (size_t)Lcap * 4 + 2048 <= 60000) {
        // AR decode step: three launches per layer (decode.hip, decode_layers_b1), the co-scheduled form unless SHOWO_DECODE_FORK=0 /
        // showo_decode_set_impl(2) ask for the plain chain
        static const int co_on = env_flag("SHOWO_DECODE_FORK", 1);
        return showo::decode_layers_b1(e, op, kv, iv, pos0, co_on && F == 8192 && !g_decode_chain, s);
    }
    // Prefill / t2i layers: TWO GEMM launches.  Phi's block is parallel-residual (phi.py:774-790): q/k/v_proj and fc1 read the
    // same LayerNorm output -> one [Wqkv ; W1] projection with a column-split epilogue; dense and fc2 add into the same residual
    // row -> one K-concatenated GEMM over [attn | ffn] with a single read-modify-write of x.
    const bool fused = T >= 256 && e->cfg.rotary_dim == 32 && fused_layer_enabled() && (3 * H) % 256 == 0 &&
                       (int64_t)T * F * 2 < ((int64_t)1 << 32);
    if (fused) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        hipStreamIsCapturing(s, &cs);
        if (showo::engine_fused_stale(e) && cs != hipStreamCaptureStatusNone) return set_error_msg(7, "engine: fused weight images must be built before a stream capture");
        TRY(fused_sync(e, s));
        for (int li = 0; li < e->nL; ++li) {
            showo::Layer& l = e->layers[li];
            bf16_t* Kd = kv.k + li * kv.k_lstride;
            bf16_t* Vd = kv.vt + li * kv.v_lstride;
            TRY(showo_layernorm_f32_op16(e->x, l.ln_w, l.ln_b, e->h, nullptr, T, H, e->cfg.ln_eps, op, s));
            TRY(range_check(e, e->h, (int64_t)T * H, s));
            TRY(showo_gemm_qkv_fc1_op16(e->h, H, e->fused_tiled ? l.wq1t : l.wqkv, H, l.bqkv, l.qln_w, l.qln_b, l.kln_w, l.kln_b, e->cosT,
                                        e->sinT, e->Q, Kd, Vd, e->ffn, F, F, B, L, nH, e->cfg.rotary_dim, e->cfg.ln_eps, pos0, Lcap, Lp,
                                        e->fused_tiled ? 1 : 0, op, s));
            TRY(range_check(e, e->Q, (int64_t)T * H, s));
            TRY(range_check(e, e->ffn, (int64_t)T * F, s));
            TRY(showo_attn_fwd_op16(e->Q, Kd, Vd, iv, flag, dense, e->attn, B, nH, L, Lk, Lcap, Lp, H, op, s));
            TRY(range_check(e, e->attn, (int64_t)T * H, s));
            TRY(showo_gemm_kcat_op16(e->attn, H, H, e->ffn, F, F, l.wd2, H + F, l.bd2, e->x, H, e->x, H, T, H, SHOWO_EPI_RESID_F32,
                                     e->fused_tiled ? 1 : 0, op, s));
            TRY(collect_x(e, li + 1, T, s));
        }
        return 0;
    }
    for (int li = 0; li < e->nL; ++li) {
        showo::Layer& l = e->layers[li];
        bf16_t* Kd = kv.k + li * kv.k_lstride;
        bf16_t* Vd = kv.vt + li * kv.v_lstride;
        TRY(showo_layernorm_f32_op16(e->x, l.ln_w, l.ln_b, e->h, nullptr, T, H, e->cfg.ln_eps, op, s));
        TRY(range_check(e, e->h, (int64_t)T * H, s));
        if (T >= 256 && e->cfg.rotary_dim == 32) {
            // prefill / t2i: one kernel (the projection's epilogue normalises, rotates and relayouts the fp32 accumulators)
            TRY(showo_gemm_qkv_fc1_op16(e->h, H, l.wqkv, H, l.bqkv, l.qln_w, l.qln_b, l.kln_w, l.kln_b, e->cosT, e->sinT, e->Q, Kd, Vd,
                                        nullptr, 0, 0, B, L, nH, e->cfg.rotary_dim, e->cfg.ln_eps, pos0, Lcap, Lp, 0, op, s));
        } else {
            TRY(showo_gemm_op16(e->h, H, l.wqkv, H, l.bqkv, 0, e->qkv, 3 * H, nullptr, 0, T, 3 * H, H, SHOWO_EPI_BF16, op, s));
            TRY(range_check(e, e->qkv, (int64_t)T * 3 * H, s));
            TRY(showo_qk_prep_op16(e->qkv, l.qln_w, l.qln_b, l.kln_w, l.kln_b, e->cosT, e->sinT, e->Q, Kd, Vd, B, L, nH,
                                   e->cfg.rotary_dim, e->cfg.ln_eps, pos0, Lcap, Lp, op, s));
        }
        TRY(showo_attn_fwd_op16(e->Q, Kd, Vd, iv, flag, dense, e->attn, B, nH, L, Lk, Lcap, Lp, H, op, s));
        TRY(range_check(e, e->attn, (int64_t)T * H, s));
        TRY(showo_gemm_op16(e->attn, H, l.wd, H, l.bd, 0, e->x, H, e->x, H, T, H, H, SHOWO_EPI_RESID_F32, op, s));
        TRY(showo_gemm_op16(e->h, H, l.w1, H, l.b1, 0, e->ffn, F, nullptr, 0, T, F, H, SHOWO_EPI_GELU_BF16, op, s));
        TRY(range_check(e, e->ffn, (int64_t)T * F, s));
        TRY(showo_gemm_op16(e->ffn, F, l.w2, F, l.b2, 0, e->x, H, e->x, H, T, H, F, SHOWO_EPI_RESID_F32, op, s));
        TRY(collect_x(e, li + 1, T, s));
    }
    return 0;
}

int showo::check_ready(showo_engine* e, int B, int L) {
    if (!e) return set_error_msg(1, "engine: null handle");
    if (showo_engine_missing(e) != 0) return set_error_msg(4, "engine: weights missing (showo_engine_missing() != 0)");
    if ((int64_t)B * L > e->maxT || B > e->cfg.max_batch || L > e->cfg.max_seq || L > e->cfg.max_pos)
        return set_error_msg(5, "engine: batch/sequence exceeds the configured workspace");
    return 0;
}

int showo::embed_in(showo_engine* e, const int64_t* ids, const float* embeds, int T, hipStream_t s) {
    if ((ids == nullptr) == (embeds == nullptr)) return set_error_msg(1, "engine: exactly one of ids / embeds must be given");
    if (ids) return showo_embed_f32(ids, e->embed, e->x, T, e->H, e->V, s);
    SHOWO_CHECK_HIP(hipMemcpyAsync(e->x, embeds, (size_t)T * e->H * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

static int hidden(showo_engine* e, const int64_t* ids, const float* embeds, const float* mask, int B, int L, hipStream_t s) {
    TRY(check_ready(e, B, L));
    TRY(embed_in(e, ids, embeds, B * L, s));
    const int32_t *iv = nullptr, *flag = nullptr;
    if (mask) {
        TRY(showo_mask_compress(mask, e->iv, e->flag, B, L, L, s));
        iv = e->iv; flag = e->flag;
    } else if (e->ext_iv) {
        iv = e->ext_iv; flag = e->ext_flag;
    }
    return run_layers(e, B, L, 0, kv_workspace(e, L), iv, flag, mask, s);
}

int showo::head_rows(showo_engine* e, const int32_t* rows, int nrows, int col0, int ncols, float* logits, hipStream_t s) {
    if (col0 < 0 || ncols <= 0 || col0 + ncols > e->V) return set_error_msg(1, "engine: bad vocabulary slice");
    if (e->precision == 1) return precise_fast_ok(e) ? head_rows_precise_fast(e, rows, nrows, col0, ncols, logits, s)
                                                       : head_rows_precise(e, rows, nrows, col0, ncols, logits, s);
    if (e->precision == 2) {
        // the split-bf16 head; a decode step (one row) takes the fused LayerNorm + (hi, lo) GEMV: 2 x 240 MB of weights in one launch
        // instead of the LayerNorm launch + a GEMV over the 719 MB [hi | hi | lo] image
        if (nrows == 1 && !rows && showo::g_decode_impl == 0 && showo::decode_fused_shapes_ok(e->H, e->F) && e->wlm_lo &&
            e->lo_loaded.count("showo.lm_head.weight"))
            return showo::decode_split_head(e->x, e->fln_w, e->fln_b, e->cfg.ln_eps, e->H, e->wlm + (int64_t)col0 * e->H,
                                            e->wlm_lo + (int64_t)col0 * e->H, e->blm + col0, logits, ncols, ncols, 1, s);
        return head_rows_precise_fast(e, rows, nrows, col0, ncols, logits, s);  // (any shape)
    }
    if (nrows == 1 && !rows && showo::g_decode_impl == 0 && showo::decode_fused_shapes_ok(e->H, e->F)) {
        // decode step: LN + lm_head in one launch, under precision 3 on the int8 image of the lm_head
        if (e->precision == 3 && !e->q8_loaded.count("showo.lm_head.weight"))
            return set_error_msg(4, "engine (precision 3): the int8 image of the lm_head is missing or stale: upload the weights again");
        const showo::DecodeHeadOps w = showo::decode_head_ops(e, col0);
        showo::LnGemvBArgs h{e->x, e->fln_w, e->fln_b, e->cfg.ln_eps, e->H, w.W, w.b, nullptr, logits, ncols, ncols, nullptr, nullptr, nullptr, 0, 0};
        h.s0 = w.s;
        return showo::decode_ln_gemv2(h, s);
    }
    TRY(showo_layernorm_f32_bf16(e->x, e->fln_w, e->fln_b, e->hf, rows, nrows, e->H, e->cfg.ln_eps, s));
    return showo_gemm_bf16(e->hf, e->H, e->wlm + (int64_t)col0 * e->H, e->H, e->blm + col0, 0, logits, ncols, nullptr, 0,
                           nrows, ncols, e->H, SHOWO_EPI_F32, s);
}

extern "C" int showo_engine_forward(showo_engine* e, const int64_t* ids, const float* embeds, const float* mask, int B, int L,
                                    float* logits, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (B == 0 || L == 0) return 0;  // empty batch: nothing to compute (the reference returns an empty logits tensor)
    TRY(hidden(e, ids, embeds, mask, B, L, s));
    return head_rows(e, nullptr, B * L, 0, e->V, logits, s);
}

extern "C" int showo_engine_forward_rows(showo_engine* e, const int64_t* ids, const float* embeds, const float* mask, int B,
                                         int L, const int32_t* rows, int nrows, int col0, int ncols, float* logits,
                                         void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (nrows > e->maxT) return set_error_msg(5, "engine: too many rows");
    TRY(hidden(e, ids, embeds, mask, B, L, s));
    return head_rows(e, rows, nrows, col0, ncols, logits, s);
}

// Visibility intervals built on the device (showo_mask_predict_next / _mmu / _mmu_vit) instead of a dense mask: the next
// forward / forward_rows / t2i_generate calls that pass mask == NULL attend with iv int32 [B,L,4] (NULL restores causal).
extern "C" int showo_engine_use_intervals(showo_engine* e, const int32_t* iv, const int32_t* flag) {
    if (!e) return set_error_msg(1, "engine: null handle");
    e->ext_iv = iv;
    e->ext_flag = iv ? flag : nullptr;
    return 0;
}

// ---- scoring given tokens (include/showo_hip.h; DESIGN.md, "Log-probabilities") ---------------------------------------------------------
// [rows, V] logits workspace of one chunk: chunk_rows <= 0 picks the largest chunk within 256 MB; never more than n or the LayerNorm
// workspace (maxT rows)
static int score_workspace(showo_engine* e, int n, int chunk_rows, int* chunk) {
    int64_t c = chunk_rows > 0 ? chunk_rows : ((int64_t)256 << 20) / ((int64_t)e->V * (int64_t)sizeof(float));
    if (c < 1) c = 1;
    if (c > n) c = n;
    if (c > e->maxT) c = e->maxT;
    if (c > e->score_rows) {
        SHOWO_CHECK_HIP(hipDeviceSynchronize());  // (an earlier call's launches may still read the buffer that goes)
        e->release(&e->score_ws);
        e->score_rows = 0;
        TRY(e->alloc(&e->score_ws, c * e->V));
        e->score_rows = c;
    }
    *chunk = (int)c;
    return 0;
}
// head + log-prob of the residual rows rows[0, n) against targets[0, n), chunk by chunk
static int score_rows(showo_engine* e, const int32_t* rows, const int64_t* targets, int n, int chunk, float* logprob, int32_t* rank,
                      hipStream_t s) {
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int m = n - c0 < chunk ? n - c0 : chunk;
        TRY(head_rows(e, rows + c0, m, 0, e->V, e->score_ws, s));
        TRY(showo_logprob_rows(e->score_ws, e->V, m, e->V, targets + c0, logprob + c0, rank ? rank + c0 : nullptr, s));
    }
    return 0;
}

extern "C" int showo_engine_score(showo_engine* e, const int64_t* ids, const float* embeds, const float* mask, int B, int L,
                                  const int32_t* rows, const int64_t* targets, int n, int chunk_rows, float* logprob, int32_t* rank,
                                  void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!e) return set_error_msg(1, "engine: null handle");
    if (n == 0 || B == 0 || L == 0) return 0;
    if (n < 0 || !rows || !targets || !logprob) return set_error_msg(1, "score: bad arguments");
    int chunk = 0;
    TRY(check_ready(e, B, L));
    TRY(score_workspace(e, n, chunk_rows, &chunk));
    TRY(hidden(e, ids, embeds, mask, B, L, s));
    return score_rows(e, rows, targets, n, chunk, logprob, rank, s);
}

namespace {
__global__ void iota_i32_kernel(int32_t* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i;
}
__global__ void fill_f32_i32_kernel(float* f, float fv, int32_t* i, int32_t iv) {
    if (threadIdx.x == 0) { *f = fv; if (i) *i = iv; }
}
}  // namespace

extern "C" int showo_engine_prefill_append_score(showo_engine* e, const int64_t* ids, int Ln, const float* logits_prev, float* logprob,
                                                 int32_t* rank, float* logits_last, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!e) return set_error_msg(1, "engine: null handle");
    if (!ids || !logprob) return set_error_msg(1, "prefill_append_score: bad arguments");
    if (logits_prev && logits_prev == logits_last) return set_error_msg(1, "prefill_append_score: logits_prev must not be logits_last");
    int chunk = 0;
    if (Ln > 1) {
        if (Ln > e->maxT) return set_error_msg(5, "engine: batch/sequence exceeds the configured workspace");
        TRY(score_workspace(e, Ln - 1, 0, &chunk));
        if (!e->score_iota) {
            TRY(e->alloc(&e->score_iota, e->maxT));
            iota_i32_kernel<<<dim3((unsigned)((e->maxT + 255) / 256)), dim3(256), 0, s>>>(e->score_iota, (int)e->maxT);
            SHOWO_CHECK_HIP(hipGetLastError());
        }
    }
    TRY(showo_engine_prefill_append(e, ids, nullptr, Ln, logits_last, stream));
    // ids[0] against the logits of the row in front of the append; ids[j] against the appended row j - 1 (the residual rows are still in x)
    if (logits_prev) {
        TRY(showo_logprob_rows(logits_prev, e->V, 1, e->V, ids, logprob, rank, s));
    } else {
        fill_f32_i32_kernel<<<1, 64, 0, s>>>(logprob, __builtin_nanf(""), rank, -1);
        SHOWO_CHECK_HIP(hipGetLastError());
    }
    if (Ln > 1) TRY(score_rows(e, e->score_iota, ids + 1, Ln - 1, chunk, logprob + 1, rank ? rank + 1 : nullptr, s));
    return 0;
}
