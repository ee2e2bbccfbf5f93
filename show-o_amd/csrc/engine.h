// Internal layout of the transformer engine and the functions its files share (engine.hip, t2i_engine.hip, decode.hip,
// decode_engine.hip, decode_batch.hip, train_engine.hip), each declared once; hipGraph capture / replay helpers at the end.
#pragma once
#include "common.h"
#include "../../include/showo_hip.h"
#include <set>
#include <string>
#include <vector>

namespace showo {
struct Layer {
    // wqkv and w1 are ONE allocation ([3H + F, H] rows q|k|v|fc1, biases likewise): the fused [Wqkv ; W1] projection reads it as is
    bf16_t *wqkv = nullptr, *wd = nullptr, *w1 = nullptr, *w2 = nullptr;
    float *bqkv = nullptr, *bd = nullptr, *b1 = nullptr, *b2 = nullptr;
    // K-concatenated image of the two residual projections: wd2 [H, H + F] rows [Wd[n,:] | W2[n,:]], bd2 = bd + b2
    // (rebuilt lazily after a weight load, see fused_sync in engine.hip)
    bf16_t* wd2 = nullptr;
    float* bd2 = nullptr;
    bf16_t* wq1t = nullptr;  // tiled copy of [Wqkv ; W1] (showo_gemm_tile_weight), allocated on first use
    float *ln_w = nullptr, *ln_b = nullptr, *qln_w = nullptr, *qln_b = nullptr, *kln_w = nullptr, *kln_b = nullptr;
    // accuracy mode (showo_engine_set_precision 1): low halves of the weights, w = hi + lo to 2^-17 (same layouts as the hi images;
    // wqkv_lo and w1_lo are one allocation like wqkv / w1)
    bf16_t *wqkv_lo = nullptr, *wd_lo = nullptr, *w1_lo = nullptr, *w2_lo = nullptr;
    // accuracy mode on the production kernels: K-concatenated, tiled split images (precise_sync in engine.hip)
    //   wq1x3 rows [w_hi | w_hi | w_lo] of [Wqkv ; W1]  ([3H + F, 3H]);  wd2x3 rows [Wd_hi | W2_hi | Wd_hi | W2_hi | Wd_lo | W2_lo] ([H, 3 (H + F)])
    bf16_t *wq1x3 = nullptr, *wd2x3 = nullptr;
    // int8 decode (showo_engine_set_precision 3): row-major int8 images and fp32 row scales of the four matrices, streamed by the fused
    // decode step; qqkv / q1 and sqkv / s1 are one allocation each like wqkv / w1.  The bf16 images above then hold bf16(q * scale).
    int8_t *qqkv = nullptr, *qd = nullptr, *q1 = nullptr, *q2 = nullptr;
    float *sqkv = nullptr, *sd = nullptr, *s1 = nullptr, *s2 = nullptr;
    // image versions (showo::engine_version): wqkv (any of q / k / v), wd, w1, w2, bd, b2 -- stamped from showo_engine::clock whenever the
    // tensor is written; fused_at = the clock when this block's wd2 / bd2 / wq1t images were last built (0: never)
    uint64_t ver[6] = {0, 0, 0, 0, 0, 0};
    uint64_t fused_at = 0;
};
}  // namespace showo

struct showo_engine;
namespace showo {
void sampler_set_device_step(const int* step_dev, const float* sched, int steps);
void gemm_pin_split_m(int M);  // gemm2p.hip (documented in gemm_common.h): split-K count of this thread's GEMM launches taken from M rows; 0 = off
int sampler_step_inc(int* step_dev, hipStream_t s);
void attn_set_decode_pos(const int* p, int lk_max = 0);
int sample_topk_launch(const float* logits, int V, int top_k, float temperature, const float* exp_noise, int64_t noise_stride,
                       uint64_t seed, int step, const int* pos_dev, int pos_base, int64_t* tok, hipStream_t s);
int sample_topk_topp_launch(const float* logits, int V, int top_k, float top_p, float temperature, const float* exp_noise,
                            int64_t noise_stride, uint64_t seed, int step, const int* pos_dev, int pos_base, int64_t* tok, hipStream_t s);
// sampler.hip: log-probability / rank of *tok on the logits row of the decode step that just stored it and advanced *pos_dev
int logprob_step_launch(const float* logits, int V, const int64_t* tok, const int* pos_dev, int pos_base, float* lp, int32_t* rank,
                        hipStream_t s);
// ---- the decode step's launches, each declared here once (decode.hip, decode_batch.hip, attention.hip; argument structs in
// decode_common.h).  op: SHOWO_OP_BF16 | SHOWO_OP_F16 -- the element type of weights and 16-bit activations; non-null row scales in an
// argument struct say that its weight pointers are int8 images (precision 3, op 0).
struct DecodePrefetch;
struct LnGemvBArgs;
struct OutGemvArgs;
struct OutGemvBArgs;
// K / V^T destination of a pass over the layers: the per-call workspace (layer stride 0) or a per-layer cache -- the AR decode cache
// (one sequence), a slot of a decode batch, or the t2i prefix-reuse cache (whole batch)
struct KVDest {
    bf16_t *k, *vt;
    int64_t k_lstride, v_lstride;  // elements between consecutive layers
    int Lcap, Lp;                  // key rows per head in k, columns per row in vt
    bf16_t *k_lo = nullptr, *vt_lo = nullptr;  // accuracy mode: low halves (same layout and strides)
};
// What a layer's decode launches stream: the bf16 / fp16 images, or under precision 3 the int8 images (they travel as bf16_t*) and
// their row scales (null otherwise); the lm_head likewise.  The ONE place that picks between them.
struct DecodeLayerOps {
    const bf16_t *Wqkv, *W1, *Wd, *W2;
    const float *sqkv, *s1, *sd, *s2;
    const float *bqkv, *b1, *bd, *b2;
};
struct DecodeHeadOps {
    const bf16_t* W;
    const float *s, *b;
};
DecodeLayerOps decode_layer_ops(const ::showo_engine* e, int li);
DecodeHeadOps decode_head_ops(const ::showo_engine* e, int col0 = 0);  // the rows from vocabulary entry col0 on
bool decode_fused_shapes_ok(int H, int F);
// batch-1 launches: a.ld0 / a.ld1 / a.W0lo are not read
int decode_ln_gemv2(const LnGemvBArgs& a, hipStream_t s, int op = 0);
int decode_out_gemv2(const OutGemvArgs& g, hipStream_t s, int mode = 0, int op = 0);  // mode: out_gemv2_kernel's MODE
int decode_split_head(const float* x, const float* lnw, const float* lnb, float eps, int H, const bf16_t* Whi, const bf16_t* Wlo,
                      const float* bias, float* logits, int N, int ld, int nb, hipStream_t s);  // decode_batch.hip: precision 2's head on a decode step
// fc2 != nullptr: the co-scheduled fc2 role (its W1 / a1 / b1 / K1 / N / y2 / s1 members) on co_blocks extra blocks, pf its prefetch role
int attn_decode_fused(const bf16_t* qkv, const float* qw, const float* qb, const float* kw, const float* kb, const float* cosT,
                      const float* sinT, bf16_t* K, bf16_t* Vt, const int32_t* iv, bf16_t* O, int nH, int rot, float eps, int pos,
                      int Lcap, int Lp, hipStream_t s, const OutGemvArgs* fc2 = nullptr, int co_blocks = 0,
                      const DecodePrefetch* pf = nullptr, int op = 0);
int attn_decode_co_batch(const bf16_t* qkv, const float* qw, const float* qb, const float* kw, const float* kb, const float* cosT,
                         const float* sinT, bf16_t* K, bf16_t* Vt, const int32_t* iv, bf16_t* O, int B, int nH, int rot, float eps,
                         const int* pos_dev, int lk_max, int Lcap, int Lp, const OutGemvBArgs& fc2, int co_blocks, hipStream_t s,
                         const DecodePrefetch* pf, int op = 0);
int attn_decode_fused_batch(const bf16_t* qkv, const float* qw, const float* qb, const float* kw, const float* kb, const float* cosT,
                            const float* sinT, bf16_t* K, bf16_t* Vt, const int32_t* iv, bf16_t* O, int B, int nH, int rot, float eps,
                            const int* pos_dev, int lk_max, int Lcap, int Lp, hipStream_t s, int op = 0);
// the layers of one batch-1 decode step (decode.hip): per layer LN + qkv / fc1 GEMV -> attention (co: with the fc2 role) -> dense / fc2
// GEMV + both residual adds.  The caller (run_layers, engine.hip) has decided that the fused step applies.
int decode_layers_b1(::showo_engine* e, int op, const KVDest& kv, const int32_t* iv, int pos0, bool co, hipStream_t s);
// engine.hip, for the KV-cached decode (decode_engine.hip, decode_batch.hip) and t2i generation (t2i_engine.hip)
int run_layers(::showo_engine* e, int B, int L, int pos0, const KVDest& kv, const int32_t* iv, const int32_t* flag, const float* dense,
               hipStream_t s);
int head_rows(::showo_engine* e, const int32_t* rows, int nrows, int col0, int ncols, float* logits, hipStream_t s);
KVDest kv_workspace(::showo_engine* e, int L);         // the per-call K / V^T workspace as a destination
int fused_sync(::showo_engine* e, hipStream_t s);      // derived weight images, rebuilt where stale; never inside a capture
int precise_sync(::showo_engine* e, hipStream_t s);
int head3_sync(::showo_engine* e, hipStream_t s);
int embed_in(::showo_engine* e, const int64_t* ids, const float* embeds, int T, hipStream_t s);
int check_ready(::showo_engine* e, int B, int L);
bool precise_fast_ok(const ::showo_engine* e);
// decode_engine.hip
KVDest kv_decode_cache(::showo_engine* e);
int engine_prefill_into(::showo_engine* e, const int64_t* ids, const float* embeds, const float* mask, int L, bf16_t* k, bf16_t* vt,
                        int64_t k_lstride, int64_t v_lstride, int cap, int* last_iv_out, float* logits_last, hipStream_t s,
                        bf16_t* k_lo, bf16_t* vt_lo);
int engine_append_into(::showo_engine* e, const int64_t* ids, const float* embeds, int Ln, int P, const int* last_iv, int L0, bf16_t* k,
                       bf16_t* vt, int64_t k_lstride, int64_t v_lstride, int cap, float* logits_last, hipStream_t s, bf16_t* k_lo,
                       bf16_t* vt_lo);
// int8 weight format helpers (quant.hip)
int q8_dequant_bf16(const int8_t* q, const float* scale, int64_t N, int64_t K, bf16_t* w, hipStream_t s);
int q8_validate(const int8_t* q, const float* scale, int64_t N, int64_t K, int* bad, hipStream_t s);  // bad: 2 device ints of the caller
int q8_quantize_rows(const float* w, int64_t N, int64_t K, int8_t* q, float* scale, int* bad, hipStream_t s);
// Infinity-Cache prefetch role of the co-scheduled decode launches (decode_common.h): what layer li's attention launch reads ahead.
// next_mb: MB of the next launches' weights ([Wqkv ; W1] of layer li + 1, the lm_head after the last layer), dense: this layer's Wd
// first, blocks: prefetch blocks per launch (0: off).  Defaults from SHOWO_DECODE_PF_MB / _DENSE / _BLOCKS; showo_decode_set_prefetch.
void decode_prefetch_plan(const ::showo_engine* e, int li, DecodePrefetch* pf);
// grid knobs of the decode launches: defaults <- environment (read once) <- showo_decode_set_tuning (sweeps in one process)
struct DecodeTuning {
    // defaults = the best of the one-process sweeps of profiles/r5_decode_dot2_sweep.txt (cfg4 shape, after the v_dot2c rewrite)
    int co_blocks = 128;        // fc2 role blocks of the batch-1 attention launch (one column per wave) SHOWO_DECODE_CO_BLOCKS
    int batch_co_blocks = 128;  // fc2 role blocks of the batched attention launch                       SHOWO_DECODE_BATCH_CO_BLOCKS
    int batch_ln_blocks = 1024; // grid cap of ln_gemvB_kernel<NB <= 4> (register activations)           SHOWO_DECODE_BATCH_LN_BLOCKS
    int ln_blocks = 1024;       // grid cap of ln_gemv2_kernel<2>                                        SHOWO_DECODE_LN_BLOCKS
    int out_blocks = 256;       // grid cap of out_gemv2_kernel / out_gemvB / out_dense_y2B              SHOWO_DECODE_OUT_BLOCKS
    int wide_ln_blocks = 256;   // grid cap of ln_gemmW_kernel (4 waves x 32 columns per block trip)     SHOWO_DECODE_WIDE_LN_BLOCKS
    int wide_out_ksplit = 4;    // blocks per column group of out_gemmW_kernel (1..8)                    SHOWO_DECODE_WIDE_OUT_KSPLIT
};
DecodeTuning& decode_tuning();
int greedy_token_seam(const float* logits, int n, int64_t* tok, int64_t* out_tokens, int* pos, int base, const float* table, float* x, int H,
                      int V, const int32_t* last_iv, int L0, int32_t* iv, hipStream_t s);
// accuracy-mode kernels (precise.hip)
int precise_ln_split(const float* x, const float* w, const float* b, const int32_t* row_index, bf16_t* hi, bf16_t* lo, int rows, int H,
                     float eps, hipStream_t s);
int precise_ln_split3(const float* x, const float* w, const float* b, const int32_t* row_index, bf16_t* out, int rows, int H, float eps,
                      hipStream_t s);
int precise_qk_prep(const float* qkv, const float* qw, const float* qb, const float* kw, const float* kb, const float* cosT,
                    const float* sinT, float* Q, float* K, float* V, int B, int L, int nH, float eps, int pos0, int Lcap, hipStream_t s);
int precise_attention(const float* Q, const float* K, const float* V, const int32_t* iv, const int32_t* flag, const float* dense, float* O,
                      int B, int nH, int Lq, int Lk, int Lcap, int ldo, hipStream_t s);
int precise_gelu_split(const float* f, bf16_t* hi, bf16_t* lo, int64_t n, hipStream_t s);
void engine_batch_free(showo_engine* e);  // decode_batch.hip
extern int g_decode_impl;  // 0 = fused decode layer (default), 1 = the seven-launch path (showo_decode_set_impl)
extern bool g_prof_on_query();
// version stamp of a state-dict tensor that derived weight images are built from (nullptr: none is) -- engine.hip
uint64_t* engine_version(showo_engine* e, const char* key);
void engine_bump_all(showo_engine* e);  // every image stale (a blanket write: showo_engine_weights_touched, precision switch)
bool engine_fused_stale(const showo_engine* e);
}  // namespace showo

using showo::bf16_t;
using showo::set_error_hip;
using showo::set_error_msg;

struct showo_engine {
    showo_engine_config cfg;
    int H, nL, nH, F, V;
    int64_t maxT;
    std::vector<void*> allocs;
    std::set<std::string> loaded;
    int expected = 0;
    // per-tensor image validity: every write of a weight that some derived image is made from stamps the tensor's version with ++clock
    // (showo_engine_load, the trainer's fused AdamW); fused_sync rebuilds the blocks whose stamps are newer than their images
    uint64_t clock = 0;
    uint64_t ver_wlm = 0;        // lm_head.weight (the trainer's transposed image)
    int64_t fused_rebuilt = 0;   // blocks whose fused images were rebuilt (showo_train_counters)
    bool fused_tiled = false;  // layout of wd2 (and use of wq1t): tiled (default) or row-major (SHOWO_W_TILED=0)
    bf16_t* wtmp = nullptr;    // staging of one layer's [Wd | W2] rows while its tiled image is built
    // weights
    float* embed = nullptr;
    std::vector<showo::Layer> layers;
    float *fln_w = nullptr, *fln_b = nullptr, *blm = nullptr, *cosT = nullptr, *sinT = nullptr;
    bf16_t* wlm = nullptr;
    // workspace
    float* x = nullptr;
    bf16_t *h = nullptr, *qkv = nullptr, *Q = nullptr, *K = nullptr, *Vt = nullptr, *attn = nullptr, *ffn = nullptr, *hf = nullptr;
    int32_t *iv = nullptr, *flag = nullptr, *rows = nullptr;
    // decode (KV cache) state: per-layer caches, capacity cap tokens
    bf16_t *kcache = nullptr, *vtcache = nullptr;
    int cache_cap = 0, cache_len = 0, prompt_len = 0;
    int cache_precision = 0;  // the precision the decode cache was prefilled under (its element type and which halves exist): decode steps must match
    int64_t cache_epoch = 0;  // showo_engine_prefill calls so far: a session that continues the cache sees that another prompt replaced it
    int last_iv[4] = {0, 0, 0, 0};
    int32_t* iv1 = nullptr;
    int64_t* tok1 = nullptr;
    // caller-provided visibility intervals (showo_engine_use_intervals): used when a call passes no dense mask
    const int32_t* ext_iv = nullptr;
    const int32_t* ext_flag = nullptr;
    // hipGraph replay of the decode step: position and last-prompt-row intervals in device memory
    int* pos_dev = nullptr;
    int32_t* last_iv_dev = nullptr;
    // second stream for the two independent branches of a Phi block (attention branch | fc1): see run_layers
    float* y2 = nullptr;  // forked decode layer: fc2 + b2 of the current layer
    // accuracy mode (showo_engine_set_precision): 0 = bf16 operands (default, the timed path), 1 = split-bf16 GEMMs + fp32 attention.
    // lo_loaded: GEMM weights whose low halves are current (cleared when somebody rewrites the hi images behind the loader's back).
    // precision 2 (round 6): IEEE-half ("fp16") operands on the same kernels -- the layer weight images (wqkv / w1 / wd / w2 and the fused
    // wq1t / wd2) and every 16-bit activation (h, Q, K, V^T, attn, ffn, the KV caches) then hold fp16 bits; img_f16 says which type the
    // layer images hold RIGHT NOW (set by the loader; a switch between precision 2 and 0 / 1 un-loads the GEMM weights so that the host
    // uploads them again).  The lm_head stays a split-bf16 product in precision 2 (wlm / wlm_lo / wlm3 + p_hf3, as in precision 1).
    int precision = 0;
    bool img_f16 = false;
    bool head3_valid = false;  // wlm3 = [hi | hi | lo] rows of the lm_head matches wlm / wlm_lo
    int64_t* range_count = nullptr;  // precision 2 range check (showo_engine_set_range_check): device counter of saturated fp16 elements
    std::set<std::string> lo_loaded;
    // precision 3: int8 image + row scales of the lm_head, and the GEMM weights whose int8 images are current (the loader makes them
    // next to the bf16 image of the dequantised values; cleared when somebody rewrites the bf16 images behind the loader's back)
    int8_t* qlm = nullptr;
    float* slm = nullptr;
    int* q8_flags = nullptr;  // flag word of the quantiser / validator (one read-back per loaded tensor, no allocation)
    std::set<std::string> q8_loaded;
    bf16_t* wlm_lo = nullptr;
    bf16_t *p_hlo = nullptr, *p_actlo = nullptr;                            // low halves of h / hf and of attn | gelu(fc1)
    float *p_qkv = nullptr, *p_f = nullptr, *p_Q = nullptr, *p_K = nullptr, *p_V = nullptr, *p_a = nullptr;  // fp32 intermediates
    // accuracy mode on the production kernels (run_layers_precise_fast): split images of the lm_head ([V, 3H] rows [hi | hi | lo]),
    // LayerNorm outputs [T, 3H] = [hi | lo | hi], the attention / gelu(fc1) operand of the residual GEMM act [T, 2 (H + F)] =
    // [attn_hi | ffn_hi | attn_lo | ffn_lo], low halves of Q / K / V^T and of the KV caches
    bool px3_valid = false;
    bf16_t *wlm3 = nullptr, *p_h3 = nullptr, *p_hf3 = nullptr, *p_act = nullptr, *p_Qlo = nullptr, *p_Klo = nullptr, *p_Vtlo = nullptr;
    bf16_t *kcache_lo = nullptr, *vtcache_lo = nullptr;
    bf16_t* wtmp3 = nullptr;
    // batched AR decode (decode_batch.hip: showo_engine_batch_begin / _batch_prefill / _batch_decode_greedy)
    struct BatchDecode;
    BatchDecode* bd = nullptr;
    // scoring (showo_engine_score / showo_engine_prefill_append_score): [score_rows, V] logits of one chunk of rows, grown on demand;
    // the rows 0 .. maxT - 1 as an index list; one target slot for the row in front of an append
    float* score_ws = nullptr;
    int64_t score_rows = 0;
    int32_t* score_iota = nullptr;
    float* collect = nullptr;  // parity hook (showo_engine_set_collect)
    // ---- t2i generation (t2i_engine.hip): everything that lives across showo_engine_t2i_generate calls
    struct T2I {
        int64_t *ids_all = nullptr, *cur = nullptr, *sampled = nullptr;
        float *sel = nullptr, *row_logits = nullptr;
        int64_t row_logits_cap = 0;
        // prefix reuse: per-layer K / V^T of the whole batch (text rows are written once, image rows every step); the low halves in
        // accuracy mode on the production kernels; ids / intervals / head rows of the active rows
        bf16_t *tk = nullptr, *tvt = nullptr, *tk_lo = nullptr, *tvt_lo = nullptr;
        int64_t tk_cap = 0, tvt_cap = 0, tk_lo_cap = 0, tvt_lo_cap = 0;
        int64_t* ids_act = nullptr;
        int32_t *iv_act = nullptr, *rows_act = nullptr, *pfx_flag = nullptr;
        // deferred prefix check: the device flag lands in pinned host memory behind an event; the host looks at it only after every
        // step of the call is queued (no pipeline bubble), and repeats the call without prefix reuse in the (never yet seen) case
        // that a text row can see an image column
        int32_t* pfx_host = nullptr;
        hipEvent_t ev_pfx = nullptr;
        // step index | pad | seed and the per-step schedule, read on the device by a replayed step
        int* step_dev = nullptr;
        float* sched_dev = nullptr;
        int sched_cap = 0;
        // hipGraph replay of the denoise step: instantiated graphs of one active-rows step are cached (small LRU), keyed by everything
        // BAKED into their launches: shapes, scalars, and every pointer that is neither engine-owned-and-fixed nor refreshed per call.
        // With prefix reuse the captured step reads its visibility intervals from the engine's own gathered copy (iv_act, rewritten by
        // every call), so the caller's mask / interval pointers are NOT part of the key: a caller that builds a fresh, equal mask tensor
        // per batch (reference inference_t2i.py:290-318) replays the same graph.  Without reuse the step reads the caller's intervals /
        // dense mask directly and their pointers stay in the key.
        struct GraphKey {
            int B, nseq, L, N, prefix, steps, id_offset, codebook, reuse, cfg, has_iv;
            int64_t mask_id;
            float guidance;
            int prec;
            const void* p[13];
        };
        struct GraphEntry {
            GraphKey key;
            hipGraphExec_t exec;
            uint64_t last_use;
        };
        static constexpr int T2I_GRAPH_SLOTS = 6;  // full / ragged last batch x CFG on / off x reuse on / off never thrash
        std::vector<GraphEntry> graphs;
        uint64_t tick = 0;
        int captures = 0;  // how often a denoise step was captured (tests: a second identical call must not capture again)
        int step0[4] = {0, 0, 0, 0};  // last t2i_generate call: sequences / rows trimmed / rows run in step 0, host wait in us (showo_engine_t2i_step0)
        float* logits0 = nullptr;     // test hooks (showo_engine_t2i_debug): step-0 logits go here; NaN-fill the K cache per call
        bool poison = false;
    };
    T2I t2i;

    // hipFree a buffer obtained from alloc() and forget it (buffers that are re-sized during the engine's life)
    template <class T>
    void release(T** p) {
        if (!*p) return;
        for (size_t i = 0; i < allocs.size(); ++i)
            if (allocs[i] == (void*)*p) { allocs.erase(allocs.begin() + i); break; }
        hipFree((void*)*p);
        *p = nullptr;
    }
    template <class T>
    int alloc(T** p, int64_t n) {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, (size_t)(n > 0 ? n : 1) * sizeof(T));
        if (e != hipSuccess) return set_error_hip(e, "hipMalloc", __FILE__, __LINE__);
        allocs.push_back(q);
        *p = (T*)q;
        return 0;
    }
};

#ifndef TRY
#define TRY(expr)            \
    do {                     \
        int _rc = (expr);    \
        if (_rc) return _rc; \
    } while (0)
#endif

namespace showo {
// ---- hipGraph capture and replay of one step (the decode loops, the t2i denoise step) ----------------------------------------------
// fn() queues one step on s; it runs inside a thread-local stream capture and *exec becomes the instantiated graph (nullptr on failure)
template <class Step>
int capture_step(hipStream_t s, Step&& fn, hipGraphExec_t* exec) {
    *exec = nullptr;
    hipGraph_t g = nullptr;
    SHOWO_CHECK_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int rc = fn();
    hipError_t he2 = hipStreamEndCapture(s, &g);
    if (!rc && he2 != hipSuccess) rc = set_error_hip(he2, "hipStreamEndCapture", __FILE__, __LINE__);
    if (!rc) {
        hipError_t he3 = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
        if (he3 != hipSuccess) { *exec = nullptr; rc = set_error_hip(he3, "hipGraphInstantiate", __FILE__, __LINE__); }
    }
    if (g) hipGraphDestroy(g);
    return rc;
}
// n_steps runs of fn(): the first eagerly (kernel attributes, launch variants), the rest as replays of one captured step (use_graph; never
// under per-launch profiling) or eagerly.  A captured step is synchronised and destroyed before the call returns.
template <class Step>
int replay_steps(Step&& fn, int n_steps, bool use_graph, hipStream_t s) {
    int rc = fn();
    hipGraphExec_t ge = nullptr;
    if (!rc && use_graph && n_steps > 1 && !g_prof_on_query()) {
        rc = capture_step(s, fn, &ge);
        for (int i = 1; !rc && i < n_steps; ++i) {
            hipError_t he = hipGraphLaunch(ge, s);
            if (he != hipSuccess) rc = set_error_hip(he, "hipGraphLaunch", __FILE__, __LINE__);
        }
    } else {
        for (int i = 1; !rc && i < n_steps; ++i) rc = fn();
    }
    if (ge) { hipStreamSynchronize(s); hipGraphExecDestroy(ge); }
    return rc;
}
}  // namespace showo
