/*
 * showo_hip.h — C ABI of libshowo_hip.so: the MI355X (gfx950) native Show-o hot path.
 *
 * The reference (showlab/Show-o) is pure Python/PyTorch and has no FFI of its own; its boundary for this
 * path is the Python class API `models.Showo` / `models.MAGVITv2` (reference models/__init__.py:1-4).
 * This header is the plain-C surface those classes' replacements (show-o_amd/modeling_*.py) bind through
 * ctypes.  Every entry point names the reference code it replaces (paths relative to the reference
 * root).  Conventions:
 *   - all pointers are DEVICE pointers unless the name ends in `_host`;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous on it;
 *   - return value: 0 on success, non-zero on error; showo_last_error() returns a static description;
 *   - no allocation ownership crosses the boundary except handles created/destroyed here;
 *   - bf16 tensors are raw uint16 bit patterns; "ids" are int64 as in the reference.
 */
#ifndef SHOWO_HIP_H
#define SHOWO_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SHOWO_ABI_VERSION 1

const char* showo_last_error(void);
int showo_abi_version(void);
/* number of compute units / wave size of the current device; used by bench/tests for sanity. */
int showo_device_info(int* cu_count, int* wave_size, char* arch_name, int arch_name_len);

/* A HIP stream whose kernels never run on `reserve` of the device's CUs (a multiple of 8: reserve / 8 CUs of EVERY XCD, since blocks
 * are dealt to the XCDs round-robin); 0 = a plain non-blocking stream.  The data-parallel trainer runs its compute on such a stream while gradient buckets are being
 * all-reduced, so that RCCL's channel kernels (training/train.py:449,612 through accelerate / DeepSpeed in the reference) find idle
 * CUs instead of queueing behind full-chip GEMM grids.  Destroy with showo_stream_destroy. */
int showo_stream_create_cu_mask(int reserve, void** stream_out);
int showo_stream_destroy(void* stream);
int showo_cu_reserved_max(void);  /* largest `reserve` among the LIVE masked streams (0 = none) */
/* CUs a launch on `stream` may use (device CUs minus the stream's reserve): the one number every grid-sizing rule reads (split-K
 * targets, tile-height model, cooperative-residency test), so launches on a masked stream are sized for what they can occupy */
int showo_cu_usable(void* stream);
/* which CUs does a launch on `stream` run on?  Launches `blocks` one-wave blocks and records per block (xcc_id << 16) | hw_id bits
 * (se, sh, cu) into ids int32 [blocks] (device): tests count the distinct CUs per XCD under a mask. */
int showo_cu_census(int32_t* ids, int blocks, int spin, void* stream);
/* test probe of the wave reductions (common.h): wave w reduces in[64 w .. 64 w + 63]; out[4 w + {0,1,2,3}] = the ds_bpermute butterfly
 * sum, the VALU-only sum (v_permlane32/16_swap + DPP) the decode kernels use, the butterfly max, the VALU-only max.  Same bits. */
int showo_wave_reduce_probe(const float* in, float* out, int n_waves, void* stream);

/* per-launch HIP-event timing of the hot kernels (bench.py roofline leg).  kind: 0 = GEMM, 1 = attention,
 * 2 = conv.  read() synchronises the device and returns summed elapsed ms, launch count, summed algorithmic flops. */
int showo_prof_enable(int on);
int showo_prof_reset(void);
int showo_prof_read(int kind, double* total_ms, int64_t* launches, double* work);
/* time only every stride-th launch of a kind (systematic sample: keeps the instrumentation overhead of a timed region small) */
int showo_prof_set_stride(int stride);
/* launches seen and work submitted per kind since the last reset, timed or not */
int showo_prof_totals(int kind, int64_t* launches, double* work);

/* ---------------------------------------------------------------------------------------------
 * MAGVIT-v2 lookup-free quantizer (reference models/modeling_magvitv2.py:201-206, 208-221, 239-241)
 * ------------------------------------------------------------------------------------------- */
/* z: fp32 [B, C, hw] (NCHW flattened) -> ids int64 [B, hw]; bit for channel c (MSB = channel 0) is (z_c > 0). */
int showo_lfq_pack_nchw(const float* z, int64_t* ids, int B, int C, int hw, void* stream);
/* same, channel-last input z: fp32 [B, hw, ldz] (first C channels used). */
int showo_lfq_pack_nhwc(const float* z, int64_t* ids, int B, int C, int hw, int ldz, void* stream);
/* ids int64 [B, hw] -> z_q fp32 [B, C, hw] of +-1 (get_codebook_entry, NCHW as the reference returns it). */
int showo_lfq_unpack_nchw(const int64_t* ids, float* zq, int B, int C, int hw, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Transformer building blocks (reference models/phi.py)
 * ------------------------------------------------------------------------------------------- */
/* nn.LayerNorm over the last dim (phi.py:744,776,937,1065): x fp32 [rows_in, H] -> y bf16 [rows, H].
 * row_index (optional, int32 [rows]) gathers input rows (used to run the final LN on image rows only). */
int showo_layernorm_f32_bf16(const float* x, const float* w, const float* b, uint16_t* y, const int32_t* row_index,
                             int rows, int H, float eps, void* stream);

/* 16-bit OPERAND TYPE of the `_op16` entry points (round 6): every `uint16_t*` operand, weight image and 16-bit output of such a call
 * holds raw bits of this type.  SHOWO_OP_BF16 = bfloat16 (what the `_bf16` entry points use; they are the op = SHOWO_OP_BF16 case of
 * their `_op16` twin).  SHOWO_OP_F16 = IEEE binary16: the same MFMA / dot2 rate with 11 significand bits instead of 8 -- the operands
 * of showo_engine_set_precision(e, 2), which brings the logits within 1e-3 of the reference's fp32 inference (inference_t2i.py:67,
 * models/phi.py:1182-1183) at the speed of the bf16 path.  Conversions to fp16 saturate at +-65504; subnormals are kept. */
enum { SHOWO_OP_BF16 = 0, SHOWO_OP_F16 = 1 };
/* nn.LayerNorm with the 16-bit output of either type (showo_layernorm_f32_bf16 = op SHOWO_OP_BF16). */
int showo_layernorm_f32_op16(const float* x, const float* w, const float* b, uint16_t* y, const int32_t* row_index,
                             int rows, int H, float eps, int op, void* stream);

/* epilogues of showo_gemm_bf16 */
enum {
    SHOWO_EPI_BF16 = 0,       /* out bf16 = acc + bias                       (q/k/v proj, phi.py:657-659)        */
    SHOWO_EPI_GELU_BF16 = 1,  /* out bf16 = gelu_new(acc + bias)              (fc1 + act, phi.py:208-210)         */
    SHOWO_EPI_F32 = 2,        /* out fp32 = acc + bias                        (lm_head + .float(), phi.py:1182-3) */
    SHOWO_EPI_RESID_F32 = 3   /* out fp32 = resid + acc + bias (resid may alias out) (dense/fc2 + residual, phi.py:727,790) */
};
/* C[M,N] = A[M,K] * W[N,K]^T (+bias[N]); A, W bf16 row-major with leading dims lda, ldw (elements);
 * K % 64 == 0.  `bias` fp32 or NULL.  `bias_per_row` != 0 adds bias[m] instead of bias[n]. */
int showo_gemm_bf16(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias, int bias_per_row,
                    void* out, int ldo, const float* resid, int ldr, int M, int N, int K, int epilogue, void* stream);
/* The same GEMM on either operand type: A, W and the 16-bit output of SHOWO_EPI_BF16 / SHOWO_EPI_GELU_BF16 are `op` values
 * (q/k/v/dense/fc1/fc2/lm_head of models/phi.py:657-659,727,208-212,1182-1183 in precision 2). */
int showo_gemm_op16(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias, int bias_per_row,
                    void* out, int ldo, const float* resid, int ldr, int M, int N, int K, int epilogue, int op, void* stream);

/* kernel selection for tests/benchmarks: 0 = by shape (default), 1 = 128x128 register-staged, 2 = 256x256 global_load_lds,
 * 3 = 256x256 phase-split (4 phases per k-tile), 4 = 256x256 phase-split (2 phases per k-tile),
 * 5 = production 2-phase kernel with a per-launch tile height (256 / 208 rows; default for M >= 1024) */
int showo_gemm_set_impl(int impl);
/* development knobs of the 256^2 phase-split kernel (impl 3), used by tools/gemm_bench.cpp: gn = weight panels per
 * tile group of the block->tile map, flags bit0 = run the two wave groups without the one-barrier stagger,
 * dbg = device buffer of 512 uint64 for per-barrier timestamps (NULL = off).  flags >> 8 forces a tile variant of the production
 * kernel (0 = tuned per shape); bits 1/2 weight-panel prefetch on/off, 3/4 direct / LDS-staged bf16 epilogue stores, 6/7 split-K of
 * launches with few tiles off / on (default on: tiles x splits ~ 256 blocks, partials summed in split order by the last block). */
int showo_gemm_tune(int gn, int flags, unsigned long long* dbg);

/* Weight-gradient GEMM on token-major operands (training/train.py:612 loss.backward(): autograd of F.linear): out fp32 [M, N] (ldo)
 * (+)= A^T B, A = dY bf16 [T, M] (lda), B = X bf16 [T, N] (ldb), contraction over the T token rows -- dW = dY^T X without transposing
 * either operand (gfx950's transposing LDS read feeds the MFMA; gemm_tn.hip).  lda, ldb multiples of 8 that cover M, N rounded up
 * to 8; operands 16-byte aligned; any T >= 1.  accumulate != 0 adds into out.  rows_padded != 0: both buffers are readable up to
 * row roundup(T, 64) - 1 (contents arbitrary; zeroed in registers) -- with lda, ldb covering whole 256-column tiles this selects the
 * fast form (unchecked DMAs, 3-deep operand ring); otherwise every fetch is checked.  Split-K by the rule of the production GEMM
 * (a function of (M, N, T) alone: run-to-run identical bits).  Bias gradients: showo_colsum_bf16 on the same dY. */
int showo_gemm_tn_bf16(const uint16_t* A, int lda, const uint16_t* B, int ldb, float* out, int ldo, int M, int N, int T,
                       int accumulate, int rows_padded, void* stream);
/* colsum[c] (+)= sum_t x[t][c], x bf16 [T, C] (row stride ld, 16-byte aligned, ld % 8 == 0); colpart: fp32 scratch of
 * (ceil(T / 32) + 8) * C floats.  Deterministic (per-64-row partials in row order, then a fixed two-level sum). */
int showo_colsum_bf16(const uint16_t* x, int ld, int T, int C, float* colpart, float* colsum, int accumulate, void* stream);

/* Launch counters of the production GEMM family (gemm2p / gemm3w): out3[0] = launches, out3[1] = of those the fused [Wqkv ; W1]
 * save-for-backward form (showo_gemm_qkv_fc1_save_bf16), out3[2] = launches that split K; reset != 0 zeroes them after reading.
 * Parity tests use it to assert that a training batch ran the T >= 256 kernels that the benchmark times. */
int showo_gemm_counters(int64_t* out3, int reset);
/* Cooperative split-K reduction (small-M launches whose tiles x splits blocks are all resident): a block waits for its tile's siblings at
 * most `polls` polls (default 32 768, ~2 ms; negative restores it), then the tile falls back to the last-arriver sum -- the same bits,
 * no abort.  0 makes every early block give up at once (test hook). */
int showo_gemm_set_coop_polls(int polls);
/* Store form of the fused projection's Q / K / V^T epilogue: 1 (default; negative restores it) = 16-byte stores, 0 = the narrow form
 * (8-byte Q / K pieces, 2-byte V^T).  Same bytes at the same addresses either way: the A/B lever of tools/gemm_bench and the
 * reference of tests/test_epilogue_stores_gpu.py.  SHOWO_GEMM_STAGE=4 selects 0 from the environment. */
int showo_gemm_set_wide_stores(int on);
/* Residual epilogue (SHOWO_EPI_RESID_F32) of the production GEMM family: 1 (default; negative restores it) = a wave tile that lies inside
 * M and N issues the residual loads of a group of fragments back to back, waits, adds and stores the group; 0 = one load, add and
 * store per fragment.  Needs 16-byte aligned out / resid rows and no per-row bias (otherwise the per-fragment form runs).  The same
 * additions on the same values either way: the A/B lever of tools/gemm_bench and the reference of tests/test_resid_epilogue_gpu.py.
 * SHOWO_GEMM_RESID_BATCH=0 selects 0 from the environment. */
int showo_gemm_set_resid_batch(int on);

/* Split-precision forms (VQGAN path): every operand is a (hi, lo) bf16 pair, x = hi + lo to ~2^-17; the MFMA
 * accumulates hi*hi + hi*lo + lo*hi in fp32.  fp32 output, optional residual.  Same layouts as the plain calls. */
int showo_gemm_bf16x3(const uint16_t* A, const uint16_t* Alo, int lda, const uint16_t* W, const uint16_t* Wlo, int ldw,
                      const float* bias, int bias_per_row, float* out, int ldo, const float* resid, int ldr, int M, int N,
                      int K, void* stream);
int showo_conv3x3_bf16x3(const uint16_t* x, const uint16_t* xlo, const uint16_t* w, const uint16_t* wlo, const float* bias,
                         const float* resid, float* out, int B, int Hin, int Win, int Cin, int Cout, int mode, void* stream);
/* The same convolution plus the GroupNorm(32) statistics of its OUTPUT -- what showo_gn_stats(out, stats, B, Hout*Wout, Cout)
 * returns, equal to the last bits of the double sums.  In a VQGAN block every 3x3 conv is followed by GroupNorm of its
 * result (common_modules.py:337-357); the conv epilogue produces the per-tile (sum, sumsq) partials (deterministic, no
 * atomics) whenever a 256-pixel tile cannot straddle two images (Hout*Wout % 256 == 0, B*Hout*Wout >= 2048), which saves
 * the read-back of the tensor; otherwise the separate reduction runs.  Cout % 128 == 0; stats: showo_gn_stats_doubles(). */
int showo_conv3x3_bf16x3_gn(const uint16_t* x, const uint16_t* xlo, const uint16_t* w, const uint16_t* wlo, const float* bias,
                            const float* resid, float* out, double* stats, int B, int Hin, int Win, int Cin, int Cout, int mode,
                            void* stream);
/* The same, leaving the statistics as partials when there are at most SHOWO_GN_FOLD_MAX per image: *pending = their count (at
 * stats + B * 64, for showo_gn_apply_part) or 0 when stats holds the final sums. */
int showo_conv3x3_bf16x3_gn_lazy(const uint16_t* x, const uint16_t* xlo, const uint16_t* w, const uint16_t* wlo, const float* bias,
                                 const float* resid, float* out, double* stats, int B, int Hin, int Win, int Cin, int Cout, int mode,
                                 int* pending, void* stream);
/* Thin-Cout 3x3 convolution (stride 1, pad 1) on split operands, for decoder.conv_out (128 -> 3 channels at the image resolution): one
 * pass over the (hi, lo) activation image with the weights in registers and fp32 FMAs (x_hi * (w_hi + w_lo) + x_lo * w_hi: the three
 * products of the split kernels), instead of a 128-wide MFMA n-tile for 3 columns.  x / xlo NHWC [B, H, W, Cin], w / wlo
 * [Cout][3][3][Cin], out fp32 NHWC [B, H, W, Cout] = conv + bias.  Cout <= 4, Cin % 32 == 0, Cin <= 256.  The summation order differs
 * from the MFMA kernel: same accuracy class (3e-5 of the output scale against fp64), not the same bits. */
int showo_conv3x3_thin_bf16x3(const uint16_t* x, const uint16_t* xlo, const uint16_t* w, const uint16_t* wlo, const float* bias,
                              float* out, int B, int H, int W, int Cin, int Cout, void* stream);
/* Strided batch of showo_gemm_bf16x3: image z < batch uses A + z * sA (hi and lo), W + z * sW (hi and lo), out + z * sOut,
 * resid + z * sResid and bias + z * sBias (strides in elements; 0 = shared by every image).  One launch with the image index as the
 * grid's second dimension; every image runs the tiles of its own (M, N, K) launch, so the result has the bits of `batch` calls of
 * showo_gemm_bf16x3.  Operand strides must be multiples of 8 elements. */
int showo_gemm_bf16x3_batched(const uint16_t* A, const uint16_t* Alo, int lda, int64_t sA, const uint16_t* W, const uint16_t* Wlo,
                              int ldw, int64_t sW, const float* bias, int bias_per_row, int64_t sBias, float* out, int ldo,
                              int64_t sOut, const float* resid, int ldr, int64_t sResid, int M, int N, int K, int batch,
                              void* stream);
/* Launches so far of the split conv kernel that stages the activation operand once per (ky, channel chunk) for all three kx taps
 * (gemm.hip conv3t_split_kernel: modes 0 / 1, Wout a multiple of 16 that divides or is a multiple of 256, Hout * Wout % 256 == 0;
 * SHOWO_CONV_3TAP=0 turns it off).  Tests assert their coverage with it. */
int64_t showo_conv3t_launches(void);
/* Of those, the launches that split K: the 3-tap kernel takes the split launches of the 16 x 16 / 32 x 32 levels too (contiguous
 * ranges of (ky, channel chunk) stages per split, last-arriver reduction in split order: the same bits on every run).
 * SHOWO_CONV_3TAP_SPLITK=0 sends them to the older kernel. */
int64_t showo_conv3t_split_launches(void);
/* fp32 -> (hi, lo) bf16 pair */
int showo_split_f32_bf16(const float* src, uint16_t* hi, uint16_t* lo, int64_t n, void* stream);

/* float4 grid-stride device copy (nbytes, src, dst 16-byte aligned): the measured HBM ceiling printed next to the 8 TB/s
 * spec by tools/ceiling.py and bench.py ("re-measure with a copy kernel"). */
int showo_copy_b128(const void* src, void* dst, int64_t nbytes, void* stream);

/* fp32 -> bf16 cast (weight packing) */
int showo_cast_f32_bf16(const float* src, uint16_t* dst, int64_t n, void* stream);
/* fp32 -> 16-bit cast of either operand type (round to nearest even; SHOWO_OP_F16 saturates at +-65504) */
int showo_cast_f32_op16(const float* src, uint16_t* dst, int64_t n, int op, void* stream);
/* Per-row symmetric int8 weight format (the weight images of showo_engine_set_precision(e, 3)).  w fp32 [N, K] row-major, per row n:
 *   amax = max_k |w[n,k]|;  scale[n] = amax / 127.0f (IEEE);  q[n,k] = clamp(rint(w[n,k] / scale[n]), -127, 127) (IEEE division,
 *   round half to even; -128 is never produced);  amax < 2^-100 (an all-zero row included): scale[n] = 1, q[n,:] = 0.
 * q int8 [N, K] row-major, scale fp32 [N].  A row that holds NaN or inf is refused (error return; q / scale are then undefined).
 * Synchronises the stream (the refusal is decided on the device). */
int showo_quantize_rows_i8(const float* w, int64_t N, int64_t K, int8_t* q, float* scale, void* stream);
/* w[n,k] = (float)q[n,k] * scale[n] (one rounding) */
int showo_dequantize_rows_i8(const int8_t* q, const float* scale, int64_t N, int64_t K, float* w, void* stream);
/* number of elements of a 16-bit image whose magnitude is >= 65504 or NaN when read as IEEE half: the range check of precision 2
 * (a saturated convert leaves exactly 65504).  count: device int64, ACCUMULATED into (zero it first). */
int showo_count_f16_saturated(const uint16_t* x, int64_t n, int64_t* count, void* stream);

/* embedding gather (phi.py:1006): ids int64 [T] -> x fp32 [T, H] from table fp32 [V, H]. */
int showo_embed_f32(const int64_t* ids, const float* table, float* x, int T, int H, int V, void* stream);

/* q/k per-head LayerNorm + partial RoPE + head-major relayout (phi.py:661-694):
 * qkv bf16 [B*L, 3*nH*64] (q|k|v) -> Q bf16 [B,nH,L,64] (pre-scaled by 1/sqrt(64)), K bf16 [B,nH,L,64],
 * Vt bf16 [B,nH,64,Lp] (transposed V, Lp % 64 == 0, pad columns zero).  The L new tokens sit at positions
 * pos0 .. pos0+L-1 (pos0 > 0 = KV-cache append): K rows / Vt columns pos0.. are written, K has Lcap rows per head.
 * cos/sin: fp32 [max_pos, rot] tables built exactly as PhiRotaryEmbedding does (phi.py:86-102). */
int showo_qk_prep(const uint16_t* qkv, const float* qln_w, const float* qln_b, const float* kln_w, const float* kln_b,
                  const float* cos_tab, const float* sin_tab, uint16_t* Q, uint16_t* K, uint16_t* Vt,
                  int B, int L, int nH, int rot, float eps, int pos0, int Lcap, int Lp, void* stream);
/* the same on either operand type (qkv in, Q / K / Vt out) */
int showo_qk_prep_op16(const uint16_t* qkv, const float* qln_w, const float* qln_b, const float* kln_w, const float* kln_b,
                       const float* cos_tab, const float* sin_tab, uint16_t* Q, uint16_t* K, uint16_t* Vt,
                       int B, int L, int nH, int rot, float eps, int pos0, int Lcap, int Lp, int op, void* stream);

/* The same result as showo_gemm_bf16(h, Wqkv) + showo_qk_prep in ONE kernel: the QKV projection whose epilogue applies
 * bias, the per-head LayerNorm(64) of q and k, the partial rotary embedding (rot must be 32) and writes Q (pre-scaled),
 * K and V^T head-major -- the fp32 accumulators are normalised directly (no bf16 round trip of qkv).
 * A bf16 [B*L, lda] (LayerNorm output h), Wqkv bf16 [3*nH*64, ldw] rows q|k|v, bias fp32 [3*nH*64]. */
int showo_gemm_qkv_bf16(const uint16_t* A, int lda, const uint16_t* Wqkv, int ldw, const float* bias, const float* qln_w,
                        const float* qln_b, const float* kln_w, const float* kln_b, const float* cos_tab,
                        const float* sin_tab, uint16_t* Q, uint16_t* K, uint16_t* Vt, int B, int L, int nH, int rot,
                        float eps, int pos0, int Lcap, int Lp, void* stream);

/* showo_gemm_qkv_bf16 and fc1 + gelu_new in ONE launch: PhiDecoderLayer feeds the same LayerNorm output to q/k/v_proj and to
 * mlp.fc1 (models/phi.py:776-790, 208-212), so the weight is the row concatenation [Wqkv ; W1] bf16 [3*nH*64 + F, ldw] (bias
 * fp32 [3*nH*64 + F]); output columns below 3*nH*64 take the QKV epilogue above, the others
 * ffn_out bf16 [B*L, ldf] = gelu_new(A W1^T + b1).  Results are bit-identical to the two separate launches whenever both sides
 * use the same k-partition: always with SHOWO_GEMM_SPLITK=0, and otherwise unless the narrower separate launch is a split-K shape
 * (few tiles, K >= 2048: the split count is a function of (M, N, K) only, never of the tile variant the tuner picks).
 * w_tiled = 1: Wqkv_fc1 is the tiled copy made by showo_gemm_tile_weight (ldw must equal K = nH*64). */
int showo_gemm_qkv_fc1_bf16(const uint16_t* A, int lda, const uint16_t* Wqkv_fc1, int ldw, const float* bias,
                            const float* qln_w, const float* qln_b, const float* kln_w, const float* kln_b,
                            const float* cos_tab, const float* sin_tab, uint16_t* Q, uint16_t* K, uint16_t* Vt,
                            uint16_t* ffn_out, int ldf, int F, int B, int L, int nH, int rot, float eps, int pos0, int Lcap,
                            int Lp, int w_tiled, void* stream);
/* showo_gemm_qkv_fc1_bf16 (ffn_out != NULL) / showo_gemm_qkv_bf16 (ffn_out == NULL: F, ldf, w_tiled ignored) on either operand
 * type: A, the weight image and Q / K / V^T / ffn_out are `op` values; LayerNorm(64), RoPE and gelu_new see the fp32 accumulators. */
int showo_gemm_qkv_fc1_op16(const uint16_t* A, int lda, const uint16_t* Wqkv_fc1, int ldw, const float* bias,
                            const float* qln_w, const float* qln_b, const float* kln_w, const float* kln_b,
                            const float* cos_tab, const float* sin_tab, uint16_t* Q, uint16_t* K, uint16_t* Vt,
                            uint16_t* ffn_out, int ldf, int F, int B, int L, int nH, int rot, float eps, int pos0, int Lcap,
                            int Lp, int w_tiled, int op, void* stream);

/* Training forward of showo_gemm_qkv_fc1_bf16 (training/train.py:510-628 through models/phi.py:657-694, 208-212): the same launch
 * also saves what backward reads -- raw_qkv bf16 [B*L, ldraw] = A Wqkv^T + b (pre-LayerNorm q, k and v: the input of
 * showo_qkln_rope_bwd / showo_attn_bwd) and ffn_pre bf16 [B*L, ldf] = A W1^T + b1 (the input of showo_dgelu_bf16) -- and derives
 * Q / K / V^T and ffn_out = gelu_new(ffn_pre) from those ROUNDED values: one launch instead of showo_gemm_bf16 + showo_qk_prep +
 * showo_gemm_bf16 + showo_gelu_bf16, with the forward and the recomputation in backward seeing the same numbers.
 * Q = K = Vt = NULL selects the raw-only form: raw_qkv / ffn_pre / ffn_out are written and the caller runs showo_qk_prep on
 * raw_qkv (same Q / K / V^T bits; A/B switch of the trainer: SHOWO_TRAIN_QKPREP=1). */
int showo_gemm_qkv_fc1_save_bf16(const uint16_t* A, int lda, const uint16_t* Wqkv_fc1, int ldw, const float* bias,
                                 const float* qln_w, const float* qln_b, const float* kln_w, const float* kln_b,
                                 const float* cos_tab, const float* sin_tab, uint16_t* Q, uint16_t* K, uint16_t* Vt,
                                 uint16_t* raw_qkv, int ldraw, uint16_t* ffn_pre, uint16_t* ffn_out, int ldf, int F, int B, int L,
                                 int nH, int rot, float eps, int pos0, int Lcap, int Lp, int w_tiled, void* stream);

/* Accuracy-mode form of showo_gemm_qkv_fc1_bf16 on the same kernels.  Operands are K-concatenated split images: A3 bf16 [M, Kcat]
 * = [a_hi | a_lo | a_hi] (Kcat = 3 K), W3 rows [w_hi | w_hi | w_lo] ([3 nH 64 + F, Kcat], tiled when w_tiled) -- one bf16 GEMM whose
 * fp32 accumulators receive hi*hi + lo*hi + hi*lo.  Every output is a (hi, lo) bf16 pair with hi = RNE(v), lo = RNE(v - hi):
 * Q / Qlo, K / Klo, Vt / Vtlo (layouts of showo_qk_prep), ffn_out / ffn_lo = gelu_new(A W1^T + b1) with IEEE exp and division
 * (both halves with leading dimension ldf).  Reference: models/phi.py:657-694, 208-212 in fp32 (inference_t2i.py:67). */
int showo_gemm_qkv_fc1_split(const uint16_t* A3, int lda, const uint16_t* W3, int ldw, int Kcat, const float* bias,
                             const float* qln_w, const float* qln_b, const float* kln_w, const float* kln_b,
                             const float* cos_tab, const float* sin_tab, uint16_t* Q, uint16_t* Qlo, uint16_t* K, uint16_t* Klo,
                             uint16_t* Vt, uint16_t* Vtlo, uint16_t* ffn_out, uint16_t* ffn_lo, int ldf, int F, int B, int L,
                             int nH, int rot, float eps, int pos0, int Lcap, int Lp, int w_tiled, void* stream);

/* K-concatenated GEMM: out[M,N] = epilogue([A0 | A1] [W0 | W1]^T + bias) with A0 bf16 [M,K0] (lda0), A1 bf16 [M,K1] (lda1) and
 * weight rows [W0[n,:] | W1[n,:]] bf16 [N, ldw] (ldw >= K0 + K1; K0, K1 multiples of 64).  epilogue must be SHOWO_EPI_RESID_F32
 * (out fp32 = acc + bias + resid, in place allowed).
 * Phi's block is parallel-residual (models/phi.py:774-790): x + dense(attn) + fc2(ffn) = x + [attn | ffn] [Wd | W2]^T + (bd + b2)
 * is one launch with ONE read-modify-write of the fp32 residual stream instead of two. */
int showo_gemm_kcat_bf16(const uint16_t* A0, int lda0, int K0, const uint16_t* A1, int lda1, int K1, const uint16_t* W, int ldw,
                         const float* bias, void* out, int ldo, const float* resid, int ldr, int M, int N, int epilogue,
                         int w_tiled, void* stream);
/* the same on either operand type (A0, A1, W) */
int showo_gemm_kcat_op16(const uint16_t* A0, int lda0, int K0, const uint16_t* A1, int lda1, int K1, const uint16_t* W, int ldw,
                         const float* bias, void* out, int ldo, const float* resid, int ldr, int M, int N, int epilogue,
                         int w_tiled, int op, void* stream);

/* Tiled weight layout accepted by the two entry points above (w_tiled = 1): [ceil(N/256)][K/64][256][64] bf16, rows beyond N zero,
 * the eight 16-byte chunks of a row stored at position chunk ^ (row & 7).  One (panel, k-tile) block = 32 KiB = the LDS image the
 * kernel's DMA fills, so a k-loop streams ONE contiguous region per weight panel (DRAM-page friendly; 1 KiB contiguous per
 * wave-instruction).  showo_gemm_tiled_elems = number of bf16 elements of the tiled copy.  W bf16 [N, ldw] row-major (for the
 * K-concatenated GEMM: the [W0 | W1] rows, K = K0 + K1). */
int64_t showo_gemm_tiled_elems(int N, int K);
int showo_gemm_tile_weight(const uint16_t* W, int ldw, int N, int K, uint16_t* out, void* stream);

/* Compress an additive attention mask [B,1,Lq,Lk] fp32 (values 0 / very negative, as built by
 * training/prompting_utils.py:466-511, 591-624) into per-row visibility intervals
 * iv int32 [B, Lq, 4] = (lo1, hi1, lo2, hi2): key c is visible iff lo1<=c<hi1 or lo2<=c<hi2.
 * flag int32[1] is set to 1 if some row is not representable (more than two runs, or a value that is
 * neither 0 nor <= -1e9); the attention kernel then adds the dense mask instead. */
int showo_mask_compress(const float* mask, int32_t* iv, int32_t* flag, int B, int Lq, int Lk, void* stream);

/* On-device mask construction from token ids (reference training/prompting_utils.py:466-511, 591-624).
 * Each call writes the per-row visibility intervals iv int32 [B,L,4] the attention kernels consume and/or the dense
 * additive mask fp32 [B,1,L,L] with the reference's values (0 / float(iinfo(int64).min)); either pointer may be NULL
 * (mmu forms always need iv).  predict_next: flag int32[1] is set if a row needs more than two runs (non-contiguous pads). */
int showo_mask_predict_next(const int64_t* ids, int B, int L, int64_t pad_id, int64_t soi_id, int64_t eoi_id, int rm_pad_in_image,
                            int32_t* iv, int32_t* flag, float* dense, void* stream);
int showo_mask_mmu(const int64_t* ids, int B, int L, int64_t eoi_id, int32_t* iv, float* dense, void* stream);
int showo_mask_mmu_vit(int B, int L, int system_prompt_len, int num_image_tokens, int32_t* iv, float* dense, void* stream);

/* MLM corruption of a training batch's image tokens on the device (reference training/utils.py:77-154
 * mask_or_random_replace_tokens).  Random form: position j of row b is masked iff argsort(noise[b])[j] < num_masked[b]
 * (the reference's `batch_randperm < num_token_masked`, :101-102).  Contiguous form (rect != NULL, :104-129): rows
 * [y0,y1) x columns [x0,x1) of the res x res token grid, rect int32 [B,4] = y0,y1,x0,x1.
 * input_ids = mask_id where masked else the token (:133); labels = the token where masked else ignore_id, or the token
 * everywhere when predict_all != 0 (:143-151); mask uint8 [B,N] is optional. */
int showo_mask_tokens(const int64_t* tokens, const float* noise, const int32_t* num_masked, const int32_t* rect, int res, int B, int N,
                      int64_t mask_id, int64_t ignore_id, int predict_all, int64_t* input_ids, int64_t* labels, uint8_t* mask,
                      void* stream);

/* Fused omni-attention forward (replaces SDPA + dense additive mask, phi.py:715-722):
 * O[b, l, h*64 + d] bf16 = softmax(Q K^T + M) V.  Q,K,Vt as produced by showo_qk_prep (Q already scaled).
 * iv/flag from showo_mask_compress; dense_mask may be NULL iff *flag is known to be 0.
 * Lq query rows (row r attends with mask row r); Lk keys; K holds Lcap rows per head, Vt rows are Lp long.
 * iv == NULL and flag == NULL: causal (query r sees keys <= r + Lk - Lq). */
/* kernel selection for tests/benchmarks: 0 = by shape (default: LDS-tiled for Lq >= 64), 1 = gather form (one wave
 * per 32 query rows, operands straight from L2), 2 = LDS-tiled form (4 waves share 64-key K / V^T tiles staged by
 * global_load_lds; 4 waves/SIMD, no register spill) */
int showo_attn_set_impl(int impl);
/* Output stores of the prefill / t2i attention forward: 1 (default; negative restores it) = 16-byte stores where ldo is a multiple of 8
 * and O is 16-byte aligned, 0 = 8-byte stores always.  Same bytes either way (A/B lever, test reference; SHOWO_ATTN_WIDE=0). */
int showo_attn_set_wide_stores(int on);
/* AR decode step (one new token against the KV cache): 0 = fused layer, three launches (LN + qkv/fc1 GEMV; prep +
 * single-query attention with the fc2 GEMV co-scheduled on the CUs the 32 attention blocks leave idle (F = 8192 only);
 * dense GEMV + both residual adds; default), 1 = the general seven-launch layer, 2 = the fused layer as a plain chain
 * (fc2 in the third launch).  All three give the same bits; 1 and 2 exist so that tests and profiles can compare them.
 * Under precision 3 (int8 decode) 0 and 2 stream the int8 images and agree bit for bit; 1 has no int8 form and runs on the bf16
 * image of the dequantised weights, so it gives the bits of 0 / 2 for power-of-two row scales only. */
int showo_decode_set_impl(int impl);
/* Infinity-Cache prefetch role of the co-scheduled decode launches (batch 1 and batched): `blocks` extra blocks of every layer's
 * attention launch read, by LDS-DMA, weights the NEXT launches will stream -- this layer's dense matrix when dense != 0, then
 * next_mb MB of the next layer's [Wqkv ; W1] (the lm_head after the last layer) -- so that those launches find them in the 256 MiB
 * memory-side cache.  Nothing is computed from the prefetched bytes: results are bit-identical for every setting
 * (tests/test_modules_gpu.py).  blocks = 0 or (next_mb = 0 and dense = 0): role absent.  Defaults: SHOWO_DECODE_PF_MB /
 * SHOWO_DECODE_PF_DENSE / SHOWO_DECODE_PF_BLOCKS.  Takes effect at the next decode call (its graph is captured per call). */
int showo_decode_set_prefetch(int next_mb, int dense, int blocks);
/* Grid knobs of the decode launches for sweeps in one process (defaults <- environment): name in
 * { "co_blocks", "batch_co_blocks", "batch_ln_blocks", "ln_blocks", "out_blocks", "wide_ln_blocks", "wide_out_ksplit" }.  Results
 * never depend on the grid caps (every grid walks the output columns with a stride; each column is reduced by one wave in one fixed
 * order).  "wide_out_ksplit" (1..8, wide batches only) is the number of blocks that share a column group's K range: it fixes the
 * order of the fp32 additions, so results are deterministic for a given value and may differ in the last bits between values. */
int showo_decode_set_tuning(const char* name, int value);
int showo_attn_fwd(const uint16_t* Q, const uint16_t* K, const uint16_t* Vt, const int32_t* iv, const int32_t* flag,
                   const float* dense_mask, uint16_t* O, int B, int nH, int Lq, int Lk, int Lcap, int Lp, int ldo,
                   void* stream);
/* the same attention on either operand type: Q, K, V^T, the soft-max numerator P inside the kernel and O are `op` values */
int showo_attn_fwd_op16(const uint16_t* Q, const uint16_t* K, const uint16_t* Vt, const int32_t* iv, const int32_t* flag,
                        const float* dense_mask, uint16_t* O, int B, int nH, int Lq, int Lk, int Lcap, int Lp, int ldo,
                        int op, void* stream);

/* Accuracy-mode attention: Q, K, V^T and the output as (hi, lo) bf16 pairs (same layouts as showo_attn_fwd; O / Olo share ldo);
 * S = Khi Qhi + Khi Qlo + Klo Qhi, fp32 soft-max, O = Vhi Phi + Vhi Plo + Vlo Phi with P split in registers: the fp32 SDPA of
 * models/phi.py:715-722 to ~1e-5 on the MFMA.  Any Lq >= 1. */
int showo_attn_fwd_split(const uint16_t* Q, const uint16_t* Qlo, const uint16_t* K, const uint16_t* Klo, const uint16_t* Vt,
                         const uint16_t* Vtlo, const int32_t* iv, const int32_t* flag, const float* dense_mask, uint16_t* O,
                         uint16_t* Olo, int B, int nH, int Lq, int Lk, int Lcap, int Lp, int ldo, void* stream);

/* Training forward: showo_attn_fwd that also writes lse fp32 [B, nH, Lq] = log sum_k exp(score) of every (masked) row. */
int showo_attn_fwd_lse(const uint16_t* Q, const uint16_t* K, const uint16_t* Vt, const int32_t* iv, const int32_t* flag,
                       const float* dense_mask, uint16_t* O, float* lse, int B, int nH, int Lq, int Lk, int Lcap, int Lp,
                       int ldo, void* stream);

/* X rows [.., L, 64] (row r of (b, h) at x + b*batch_stride + h*head_stride + r*row_stride) -> XT bf16 [B, nH, 64, Lp]
 * (columns >= L zero).  Makes the k-contiguous operand images (Q^T, K^T) of showo_attn_bwd. */
int showo_head_transpose(const uint16_t* x, uint16_t* xt, int B, int nH, int L, int Lp, int64_t batch_stride,
                         int64_t head_stride, int row_stride, void* stream);

/* Backward of the fused attention (autograd of SDPA + mask, phi.py:715-722).  Self-attention, Lq = Lk = L, interval
 * masks (iv from showo_mask_compress, NULL = causal; *flag must be 0).
 * in : Q (pre-scaled), K bf16 [B,nH,L,64]; QT, KT bf16 [B,nH,64,Lp] (showo_head_transpose); V rows token-major (row
 *      stride ldv, head h at column 64h: the v section of the raw qkv projection); O, dO bf16 token-major [B*L, lddo];
 *      lse fp32 [B,nH,L] from showo_attn_fwd_lse.
 * scratch: dOT bf16 [B,nH,64,Lp], D fp32 [B,nH,L].
 * out: dQ (w.r.t. the pre-scaled Q), dK, dV bf16 token-major (row strides ldq/ldk/ldvo, head h at column 64h). */
int showo_attn_bwd(const uint16_t* Q, const uint16_t* K, const uint16_t* QT, const uint16_t* KT, const uint16_t* V, int ldv,
                   const uint16_t* O, const uint16_t* dO, int lddo, uint16_t* dOT, const float* lse, float* D,
                   const int32_t* iv, const int32_t* flag, uint16_t* dQ, int ldq, uint16_t* dK, int ldk, uint16_t* dV,
                   int ldvo, int B, int nH, int L, int Lp, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training kernels (autograd of the block + loss + optimizer; reference training/train.py:590-628).
 * Every reduction is fixed-order (block partials + finalize): bit-reproducible gradients.
 * ------------------------------------------------------------------------------------------- */
/* X bf16 [T, C] (row stride ld) -> XT bf16 [C, Tp] (Tp % 64 == 0, columns >= T zero): the k-contiguous operand of the
 * weight-gradient GEMMs dW = dY^T X.  mode 1 writes gelu_new(X)^T (the MLP activation from the saved pre-activation).
 * colsum (optional, fp32 [C]): column sums of X = bias gradient (accumulate != 0 adds); colpart: scratch fp32 [Tp/64 + 8, C]. */
int showo_transpose_bf16(const uint16_t* x, int ld, uint16_t* xt, int T, int C, int Tp, int mode, float* colpart, float* colsum,
                         int accumulate, void* stream);
/* LayerNorm backward fused with the residual add of the parallel block (phi.py:774-790): dx = dy + dLN(x)^T dh.
 * x, dh, dy fp32 [T,H]; dx32 fp32 (may alias dy), dx16 bf16 copy (may be NULL); dgb fp32 [2,H] = (dgamma, dbeta);
 * part: scratch fp32 [showo_ln_bwd_blocks(T), 2, H]. */
int showo_ln_bwd(const float* x, const float* gamma, const float* dh, const float* dy, float* dx32, uint16_t* dx16, float* part,
                 float* dgb, int T, int H, float eps, void* stream);
int showo_ln_bwd_blocks(int T);
/* the same plus dxsum[H] = column sums of dx16: dx is the output gradient of the block below, whose dense / fc2 bias gradients are
 * exactly these sums (no second pass over dx16).  part: scratch fp32 [showo_ln_bwd_blocks(T), 3, H]. */
int showo_ln_bwd_colsum(const float* x, const float* gamma, const float* dh, const float* dy, float* dx32, uint16_t* dx16, float* part,
                        float* dgb, float* dxsum, int T, int H, float eps, void* stream);
/* Accumulating forms of the parameter-gradient side outputs (gradient accumulation over micro-batches).  Contract of every
 * showo_*_acc entry point: accumulate == 0 is the plain call; accumulate != 0 gives out = out_old + v where v is, bit for bit, what
 * the plain call writes for the same inputs -- the old value is added once, to the finished fp32 sum, by the last stage of the
 * kernel's fixed-order reduction (the way SHOWO_EPI_RESID_F32 / showo_gemm_tn_bf16(accumulate) add theirs).  Data-gradient outputs
 * (dx32, dx16, dqkv, df) are per micro-batch and always overwritten.  showo_ln_bwd_colsum_acc has one switch per destination. */
int showo_ln_bwd_acc(const float* x, const float* gamma, const float* dh, const float* dy, float* dx32, uint16_t* dx16, float* part,
                     float* dgb, int accumulate, int T, int H, float eps, void* stream);
int showo_ln_bwd_colsum_acc(const float* x, const float* gamma, const float* dh, const float* dy, float* dx32, uint16_t* dx16,
                            float* part, float* dgb, float* dxsum, int accumulate_dgb, int accumulate_dxsum, int T, int H, float eps,
                            void* stream);
/* Backward of q/k LayerNorm(64) + partial rotary + the 1/8 fold (phi.py:661-694): dq, dk bf16 [T, ldg] (w.r.t. the stored Q,
 * K), raw qkv bf16 [T, 3*nH*64] -> dqkv bf16 [T, 3*nH*64] (q and k sections), dparams fp32 [4,64] = (dq_ln_w, dq_ln_b,
 * dk_ln_w, dk_ln_b); part: scratch fp32 [showo_qkln_rope_bwd_blocks(T, nH), 4, 64]. */
int showo_qkln_rope_bwd(const uint16_t* dq, const uint16_t* dk, int ldg, const uint16_t* qkv, const float* qw, const float* kw,
                        const float* cos_tab, const float* sin_tab, uint16_t* dqkv, float* part, float* dparams, int T, int L,
                        int nH, int rot, float eps, void* stream);
int showo_qkln_rope_bwd_blocks(int T, int nH);
int showo_qkln_rope_bwd_acc(const uint16_t* dq, const uint16_t* dk, int ldg, const uint16_t* qkv, const float* qw, const float* kw,
                            const float* cos_tab, const float* sin_tab, uint16_t* dqkv, float* part, float* dparams, int accumulate,
                            int T, int L, int nH, int rot, float eps, void* stream);
/* The three mean cross-entropies of Showo.forward (modeling_showo.py:80-98) and their gradient.
 * logits fp32 [B*L, ldl]; labels int64 [B,L] (-100 = ignore).  losses fp32 [3] = (t2i, lm, mmu);
 * dlogits (optional) bf16 [B*L, ldd] = d(g_t2i*loss_t2i + g_lm*loss_lm + g_mmu*loss_mmu)/dlogits, pad columns zero.
 * scratch: rows_ws 12*B*L bytes, counts int[3], rowloss fp32 [2*B*L]. */
int showo_ce_loss(const float* logits, int ldl, const int64_t* labels, int B, int L, int V, int b_t2i, int b_lm, int b_mmu,
                  int max_seq_len, float g_t2i, float g_lm, float g_mmu, void* rows_ws, int* counts, float* rowloss,
                  uint16_t* dlogits, int ldd, float* losses, void* stream);
/* The row census of showo_ce_loss as an ORDERED compaction (the loss head on the labelled rows only, showo_train_set_loss_rows).
 * A logits row (b, l) is labelled when it carries a t2i target (b < b_t2i, l > max_seq_len, labels[b, l] != -100) or a next-token
 * target of the lm / mmu slice (l < L - 1, labels[b, l + 1] != -100; b_mmu == 0 selects the whole batch, the reference's
 * logits[-0:]); a row can carry both.  Writes rows_ws (the 12-byte table of showo_ce_loss, all B*L rows) and counts int[3] as
 * showo_ce_loss does, and: row_index int32 [Tc] = the labelled rows in ASCENDING row order, row_slot int32 [B*L] = the compact
 * index of a row or -1, rows_compact = the table entries of the labelled rows in compact order (12 * B*L bytes), *n_rows = Tc.
 * Ballot / popcount scan over blocks of rows in two passes, no atomic cursor: two runs give the same bits.
 * scan_ws: int32 [showo_ce_rows_compact_ws(B * L)] (one int per scan block). */
int showo_ce_rows_compact(const int64_t* labels, int B, int L, int b_t2i, int b_lm, int b_mmu, int max_seq_len, void* rows_ws,
                          void* rows_compact, int* counts, int* row_index, int* row_slot, int* n_rows, int* scan_ws, void* stream);
int showo_ce_rows_compact_ws(int rows);
/* Embedding backward (deterministic): dE[ids[t]] = sum of dx[t] over equal ids, in position order.  dE must be
 * zero-filled by the caller; order_ws: scratch int[2*T]. */
int showo_embed_bwd(const int64_t* ids, const float* dx, float* dE, int* order_ws, int T, int H, int V, void* stream);
/* accumulate != 0: dE[ids[t]] += the same position-ordered sums, only in the rows this batch touches (no zero-fill, every other row
 * is left alone); accumulate == 0 is showo_embed_bwd. */
int showo_embed_bwd_acc(const int64_t* ids, const float* dx, float* dE, int* order_ws, int accumulate, int T, int H, int V,
                        void* stream);
/* Spliced image rows (the w_clip_vit training flow, training/train_w_clip_vit.py:530-589: the projector's rows are concatenated
 * between the embedded text ids).  Layout: ids int64 [B,L] at full length; the LAST n sequences (0 <= n <= B) each hold P placeholder
 * columns [start[j], start[j] + P) whose ids are never read; start int32 [n] on the device with 0 <= start[j], start[j] + P <= L
 * (the caller's contract: the kernels clamp, so a bad start reads and writes nothing outside its tensors, but the results are then
 * undefined); rows fp32 [n*P, H] = the projector's output.  H % 4 == 0, 16-byte aligned tensors.  No atomics, no host wait.
 * showo_embed_splice_f32: x fp32 [B*L, H] = rows[j*P + k] at placeholder position (B-n+j, start[j]+k), table[ids] elsewhere -- the
 * bits of showo_embed_f32, NaN rows for out-of-range ids included; n == 0 is showo_embed_f32.
 * showo_gather_splice_rows_f32: out fp32 [n*P, H] = the placeholder rows of dx fp32 [B*L, H] in row order.
 * showo_embed_bwd_splice: showo_embed_bwd_acc that leaves the placeholder positions out of the ranking and of the sums: bit-equal to
 * showo_embed_bwd[_acc] on the batch with the placeholder tokens removed (ids and dx rows compacted in position order); table rows
 * no live id names are not written; order_ws: scratch int[2*B*L]; live ids must be in [0, V). */
int showo_embed_splice_f32(const int64_t* ids, const float* table, const float* rows, const int32_t* start, float* x, int B, int L,
                           int n, int P, int H, int V, void* stream);
int showo_gather_splice_rows_f32(const float* dx, const int32_t* start, float* out, int B, int L, int n, int P, int H, void* stream);
int showo_embed_bwd_splice(const int64_t* ids, const float* dx, float* dE, int* order_ws, const int32_t* start, int accumulate, int B,
                           int L, int n, int P, int H, int V, void* stream);
/* torch.optim.AdamW step on fp32 tensors (step counts from 1). */
int showo_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                float weight_decay, int step, void* stream);
int showo_scale_f32(float* x, int64_t n, float s, void* stream);

/* bf16 gradient wire of the data-parallel exchange (reference: mixed_precision bf16 + DeepSpeed ZeRO-2 reduce,
 * configs/showo_pretraining_stage1.yaml:87, accelerate_configs/8_gpus_deepspeed_zero2.yaml:2-16; SURVEY.md 8e: 2.90 GB per rank
 * per step).  pack: wire[i] = bf16(grad[i] * scale), scale = 1 / world_size applied before rounding, so that the all-reduce SUM
 * of the wire is the mean; unpack: grad[i] = float(wire[i]).  grad 16-byte, wire 8-byte aligned. */
int showo_grad_wire_pack(const float* grad, uint16_t* wire, int64_t n, float scale, void* stream);
int showo_grad_wire_unpack(const uint16_t* wire, float* grad, int64_t n, void* stream);
/* df = da * gelu_new'(f) (bf16, elementwise) */
int showo_dgelu_bf16(const uint16_t* da, const uint16_t* f, uint16_t* df, int64_t n, void* stream);
/* showo_dgelu_bf16 on a [T, C] matrix (row stride ld) fused with the column sums of its result (the fc1 bias gradient, like
 * showo_colsum_bf16 on df); colpart: fp32 scratch of (ceil(T / 64) + 8) * C floats; df may alias da. */
int showo_dgelu_colsum_bf16(const uint16_t* da, const uint16_t* f, uint16_t* df, int ld, int T, int C, float* colpart, float* colsum,
                            void* stream);
int showo_dgelu_colsum_bf16_acc(const uint16_t* da, const uint16_t* f, uint16_t* df, int ld, int T, int C, float* colpart,
                                float* colsum, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * t2i sampler (reference models/modeling_showo.py:140-179, models/sampling.py:14-36)
 * ------------------------------------------------------------------------------------------- */
/* One categorical draw per image token from softmax((1+w)*cond - w*uncond) using the algorithm
 * torch.multinomial uses for one draw (argmax_i p_i / E_i, E~Exp(1)).
 * logits_c/logits_u: fp32 [B*N, ld] (uncond NULL -> no CFG).  cur: int64 [B,N] current code ids or mask_id.
 * exp_noise: optional fp32 [B*N, V] injected noise (tests); else Philox(seed, step).
 * out: sampled int64 [B,N] (known tokens keep their id), sel_prob fp32 [B,N] (FLT_MAX for known tokens). */
int showo_cfg_softmax_sample(const float* logits_c, const float* logits_u, int ld, float guidance, const int64_t* cur,
                             int64_t mask_id, const float* exp_noise, uint64_t seed, uint32_t step,
                             int64_t* sampled, float* sel_prob, int B, int N, int V, void* stream);
/* mask_by_random_topk + write-back (modeling_showo.py:166-179): per sample b,
 * mask_len = max(1, min(#unknown-1, mask_len_f)); conf = log(p)+temp*gumbel(u); cut = sort(conf)[mask_len];
 * masking = conf < cut; ids_cond/ids_uncond[b, img_start + i] = masking ? mask_id : sampled+offset;
 * cur[b,i] = masking ? mask_id : sampled.  uniform: optional injected fp32 [B,N] draws. */
int showo_mask_by_topk(const float* sel_prob, const int64_t* sampled, int64_t* cur, int64_t* ids_cond,
                       int64_t* ids_uncond, int ld_ids, int img_start, int64_t mask_id, int64_t id_offset,
                       float mask_len_f, float temperature, const float* uniform, uint64_t seed, uint32_t step,
                       uint8_t* masking_out, int B, int N, void* stream);

/* ---------------------------------------------------------------------------------------------
 * VQGAN building blocks (reference models/common_modules.py, channel-last activations)
 * ------------------------------------------------------------------------------------------- */
/* GroupNorm(32, eps) statistics over x fp32 NHWC [B, HW, C]: stats double [B, 32, 2] = (sum, sumsq).
 * Deterministic two-pass reduction (no atomics): `stats` must provide showo_gn_stats_doubles(B, HW) doubles
 * ([B,32,2] result followed by per-block partials). */
int showo_gn_stats_doubles(int B, int HW);
int showo_gn_stats(const float* x, double* stats, int B, int HW, int C, void* stream);
/* second pass alone: stats[b][g][2] = sum_k part[b][k][g][2] over nblk per-block partials, in k order */
int showo_gn_finalize(const double* part, double* stats, int B, int nblk, void* stream);
/* y bf16 NHWC = act((x - mean) * rstd * gamma + beta); act = swish if do_swish (common_modules.py:16-24).
 * ylo (optional): low half for split precision, ylo = bf16(value - float(y)). */
int showo_gn_apply(const float* x, const double* stats, const float* gamma, const float* beta, uint16_t* y, uint16_t* ylo,
                   int B, int HW, int C, float eps, int do_swish, void* stream);
/* The apply pass sizes its grid to the tensor: 512 pixels per block on the large levels, fewer on the small ones so that B x blocks
 * reaches about 1024 (down to one pass of the block).  showo_gn_set_fixed_grid(1) keeps 512 everywhere (the former grid: A/B lever and
 * reference of tests/test_vq_tail_gpu.py).  The kernel is elementwise given the statistics: same output bits either way. */
int showo_gn_set_fixed_grid(int on);
/* Folded finalize.  An image with at most SHOWO_GN_FOLD_MAX partials (the 16^2 ... 64^2 levels) does not need the separate
 * showo_gn_finalize launch: showo_gn_apply_part takes part[b][k][32][2], k < nblk, and every block sums them in its prologue in
 * showo_gn_finalize's order (four strided quarters, (q0 + q1) + (q2 + q3), in double), so y / ylo have the bits of the
 * showo_gn_finalize + showo_gn_apply pair.  showo_gn_stats_lazy is showo_gn_stats that stops after the partial pass when it may:
 * *pending = the partial count (they lie at stats + B * 64) or 0 when stats holds the final sums (pending == NULL: always final). */
#define SHOWO_GN_FOLD_MAX 16
int showo_gn_stats_lazy(const float* x, double* stats, int B, int HW, int C, int* pending, void* stream);
int showo_gn_apply_part(const float* x, const double* part, int nblk, const float* gamma, const float* beta, uint16_t* y,
                        uint16_t* ylo, int B, int HW, int C, float eps, int do_swish, void* stream);
/* 3x3 convolution as implicit GEMM on MFMA. x bf16 NHWC [B,Hin,Win,Cin]; w bf16 [Cout][3][3][Cin];
 * out fp32 NHWC [B,Hout,Wout,Cout] = conv + bias (+ resid).  mode: 0 = stride 1 pad 1;
 * 1 = nearest-2x upsample then stride 1 pad 1 (common_modules.py:36-40); 2 = pad (0,1,0,1) then stride 2
 * (common_modules.py:83-88).  Cin % 64 == 0 (thin inputs are zero-padded to 64 channels); any Cout. */
int showo_conv3x3_bf16(const uint16_t* x, const uint16_t* w, const float* bias, const float* resid, float* out,
                       int B, int Hin, int Win, int Cin, int Cout, int mode, void* stream);
/* direct convolution for the thin layers (Cin or Cout in {3,13}): x fp32 NHWC, w fp32 [Cout][k][k][Cin],
 * out fp32 NHWC; ksize 1 or 3, stride 1, pad (k-1)/2. */
int showo_conv_small_f32(const float* x, const float* w, const float* bias, float* out, int B, int H, int W,
                         int Cin, int Cout, int ksize, void* stream);
/* row softmax with scale: x fp32 [rows, n] -> y bf16 [rows, ldy] = softmax(x * scale) (AttnBlock, common_modules.py:199-201) */
int showo_softmax_rows_bf16(const float* x, uint16_t* y, uint16_t* ylo, int rows, int n, int ldy, float scale, void* stream);
/* fp32 [P, C] -> bf16 [P, Cpad] with zero-padded channels (feeds the MFMA conv for the 3-/13-channel inputs) */
int showo_pad_cast_bf16(const float* x, uint16_t* y, uint16_t* ylo, int64_t P, int C, int Cpad, void* stream);
/* ids int64 [B, hw] -> z_q fp32 [B, hw, C] (channel-last form of get_codebook_entry) */
int showo_lfq_unpack_nhwc(const int64_t* ids, float* zq, int B, int C, int hw, void* stream);
/* layout changes at the image / latent boundary */
int showo_nchw_to_nhwc_f32(const float* x, float* y, int B, int C, int HW, void* stream);
int showo_nhwc_to_nchw_f32(const float* x, float* y, int B, int C, int HW, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Engines: whole-module entry points.  Handles own packed bf16 weights + workspaces in HBM.
 * ------------------------------------------------------------------------------------------- */
typedef struct showo_engine showo_engine;
typedef struct {
    int hidden, layers, heads, ffn, vocab;
    int rotary_dim, max_pos;
    float ln_eps, rope_theta;
    int max_batch, max_seq; /* workspace sizing: tokens = max_batch*max_seq */
} showo_engine_config;

int showo_engine_create(const showo_engine_config* cfg, showo_engine** out);
void showo_engine_destroy(showo_engine* e);
/* Load one tensor by its REFERENCE state-dict key, e.g.
 * "showo.model.layers.3.self_attn.q_proj.weight"; src = device fp32, n = element count.  GEMM weights are
 * converted to bf16 and q/k/v are packed into one [3H,H] matrix.  cos/sin tables: keys "rope.cos"/"rope.sin". */
int showo_engine_load(showo_engine* e, const char* key, const float* src, int64_t n, void* stream);
/* Where showo_engine_load would put a tensor, without copying: exactly one of *dst_bf16 (weight image) / *dst_f32 (vector, embedding
 * table) is set.  The trainer's fused optimizer launch writes the refreshed images through these pointers and then calls
 * showo_engine_weights_touched (the bookkeeping showo_engine_load does: fused weight images / cached graphs are rebuilt). */
int showo_engine_slot(showo_engine* e, const char* key, int64_t n, uint16_t** dst_bf16, float** dst_f32);
int showo_engine_weights_touched(showo_engine* e);
/* number of tensors still missing (0 = ready) */
int showo_engine_missing(const showo_engine* e);
/* number of times showo_engine_t2i_generate captured a denoise step into a hipGraph on this engine (the instantiated graph is
 * cached: identical calls replay it without capturing again) */
int showo_engine_t2i_captures(const showo_engine* e);
/* what step 0 of the last showo_engine_t2i_generate call ran: out[0] sequences (B + 1 of 2 B when the unconditional sequences of a CFG
 * call were found identical), out[1] leading rows trimmed from every sequence, out[2] rows run (= out[0] * (L - out[1])), out[3] host
 * time in microseconds spent waiting for that decision.  Without prefix reuse: all sequences, 0, all rows, 0. */
int showo_engine_t2i_step0(const showo_engine* e, int* out);
/* test hooks of showo_engine_t2i_generate.  logits0 (device fp32 [(2)B * num_vq_tokens, codebook], or NULL): receives the logit rows of
 * step 0.  poison_kv != 0: the batch-wide K cache is filled with NaN bit patterns at the start of every call. */
int showo_engine_t2i_debug(showo_engine* e, float* logits0, int poison_kv);
/* parity hook: while buf != NULL every forward copies the fp32 residual stream into buf fp32 [layers + 1, B*L, hidden] (slot 0 = the
 * embedded input, slot i = output of transformer block i - 1), so that a test can check each block against the oracle evaluated on
 * the block's own input as the GPU computed it (no error amplification across blocks). */
int showo_engine_set_collect(showo_engine* e, float* buf);
/* Operand precision.  precision 0 (default): bf16 GEMM / attention operands, fp32 accumulation.  precision 1: the reference's fp32
 * inference (inference_t2i.py:67 keeps the model in fp32; models/phi.py:1182-1183 returns fp32 logits) to ~1e-5 end to end with
 * split-bf16 operands (x = hi + lo to 2^-17, products hi*hi + lo*hi + hi*lo accumulated in fp32).
 * Production form (showo_engine_precise_fast() == 1: rotary_dim 32, 3 * hidden a multiple of 256 -- Phi-1.5's shape): the SAME
 * kernels and launch structure as precision 0 on K-concatenated split images -- activations [hi | lo | hi], weight rows
 * [hi | hi | lo], one bf16 GEMM over 3K per product (showo_gemm_qkv_fc1_split, showo_gemm_kcat_bf16), split attention
 * (showo_attn_fwd_split) -- so every entry point works in this mode, including prefix reuse and hipGraph replay in _t2i_generate and
 * the KV-cached prefill / decode (decode steps run eagerly).  Otherwise (tiny test shapes, SHOWO_PRECISE_FAST=0) the fp32 reference
 * kernels of csrc/precise.hip serve forward / forward_rows / t2i_generate and the KV-cached entry points refuse.
 * The weights must be uploaded (showo_engine_load) AFTER switching to precision 1 -- the loader then also keeps their low halves;
 * showo_engine_precise_ready tells whether they are current. */
/* precision 2 (round 6): IEEE-half ("fp16") operands.  The SAME launches, tiles, prefix reuse and hipGraph replay as precision 0 --
 * v_mfma_f32_*_f16 runs at the bf16 rate -- with operand rounding 2^-12 instead of 2^-9: weights of the 24 blocks, LayerNorm output,
 * Q / K / V^T, the soft-max numerator, the attention output and gelu(fc1) are fp16 (saturating converts, subnormals kept); the residual
 * stream, LayerNorm / RoPE / soft-max arithmetic and every accumulator stay fp32, and the final LayerNorm + lm_head run as the split-bf16
 * product of precision 1 (so the final hidden state and the lm_head weight are not rounding points).  End to end against the fp32
 * reference: rel_rms ~8e-4 / rel_max <= 1e-3 at model scale where bf16 operands give 7e-3 (oracle/predict_rounding.py,
 * tests/test_modules_gpu.py).  KV-cached decode steps run on the general (seven-launch) layer; the batched decode refuses.
 * Switching between precision 2 and 0 / 1 un-loads the GEMM weights (their images change element type): showo_engine_missing() is
 * then > 0 until the host has uploaded them again.  Training keeps bf16 images (showo_train_* refuse a precision-2 engine). */
/* precision 3: int8 decode.  bf16 operands everywhere, as in precision 0, on a QUANTISED model: showo_engine_load of a GEMM weight
 * (q/k/v_proj, dense, fc1, fc2 of every block, lm_head) quantises the fp32 source per output row (showo_quantize_rows_i8) and keeps two
 * images: int8 + scale, which the fused decode step (showo_decode_set_impl 0 / 2) streams at one byte per weight, and the bf16 image of
 * the dequantised values bf16(q * scale) for everything on the MFMA GEMMs (prefill, forward, forward_rows, t2i_generate, the
 * seven-launch decode layer).  Decode arithmetic per output column: the int8 weights converted exactly to bf16, the dot2 chain, lane
 * split and wave reduction of the bf16 kernels, then ONE fp32 multiply by scale[n] in front of the unchanged epilogue -- bit-identical
 * to the bf16 kernels on q * scale whenever the scales are powers of two.  Biases, LayerNorm parameters, embeddings: fp32, unchanged.
 * This mode trades accuracy for speed (the only one that does).  Costs 1 byte per GEMM weight on top of the bf16 images.  Switching to
 * or from 3 un-loads the GEMM weights like precision 2 does.  Refused unless hidden <= 2048, ffn <= 8192, both multiples of 16; a
 * decode step against a KV cache too long for the fused layer (capacity > 14 488 tokens) is refused as well, never served from the
 * bf16 image.  The batched decode (showo_engine_batch_*) streams the int8 images too: every sequence keeps its batch-1 bits. */
int showo_engine_set_precision(showo_engine* e, int precision);
/* precision 3 only: load a caller-quantised GEMM weight (same keys as showo_engine_load; q int8 [N, K] row-major with |q| <= 127,
 * scale fp32 [N] positive and finite, both on the device) into both images.  Synchronises the stream (the inputs are validated). */
int showo_engine_load_q8(showo_engine* e, const char* key, const int8_t* q, const float* scale, int64_t N, int64_t K, void* stream);
int showo_engine_get_precision(const showo_engine* e);
/* precision 2 range check: while count != NULL (device int64, zero it first) every forward adds the number of fp16 activation
 * elements (LayerNorm output, q|k|v or Q, attention output, gelu(fc1)) that left a convert saturated (|x| = 65504) or non-finite.
 * Extra launches: a diagnostic, not for timed runs.  Random-init weights never saturate; REAL Phi-1.5 checkpoints decide the range
 * question for a deployment -- run one batch with the counter on. */
int showo_engine_set_range_check(showo_engine* e, int64_t* count);
int showo_engine_precise_ready(const showo_engine* e);
int showo_engine_precise_fast(const showo_engine* e);
/* process-wide A/B switch of the two accuracy-mode implementations (default: SHOWO_PRECISE_FAST, on): 0 = always the fp32 reference
 * kernels of csrc/precise.hip.  Call showo_engine_set_precision(e, 1) again after switching it on (workspaces are made there). */
int showo_precise_set_fast(int on);
/* Showo.forward without labels (modeling_showo.py:76-79 -> phi.py:953-1183):
 * ids int64 [B,L] or embeds fp32 [B,L,H] (exactly one non-NULL); mask fp32 [B,1,L,L] or NULL (causal);
 * logits fp32 [B,L,vocab]. */
/* attend with caller-built visibility intervals (showo_mask_predict_next etc.) in the following calls that pass
 * mask == NULL; iv == NULL restores the default (no mask = causal).  flag may be NULL (= known representable). */
int showo_engine_use_intervals(showo_engine* e, const int32_t* iv, const int32_t* flag);
int showo_engine_forward(showo_engine* e, const int64_t* ids, const float* embeds, const float* mask, int B, int L,
                         float* logits, void* stream);
/* Final-LN'ed hidden rows + restricted lm_head: logits fp32 [nrows, ncols] for token rows `rows`
 * (int32 [nrows], index into B*L) and vocabulary columns [col0, col0+ncols).  Same math as the reference
 * restricted to the entries t2i_generate consumes (modeling_showo.py:144). */
int showo_engine_forward_rows(showo_engine* e, const int64_t* ids, const float* embeds, const float* mask, int B, int L,
                              const int32_t* rows, int nrows, int col0, int ncols, float* logits, void* stream);
/* Showo.t2i_generate (modeling_showo.py:104-181).  ids_cond int64 [B,L] is updated in place like the
 * reference; ids_uncond may be NULL (no CFG).  mask fp32 [(2)B,1,L,L].  mask_len_host/temps_host: per-step
 * host constants (floor(N*schedule((k+1)/T)) and the compounding temperature).  use_graph: bit 0 = capture one
 * denoise step into a hipGraph and replay it; bit 1 = do NOT reuse the step-invariant text rows (by default step 0 runs
 * the whole sequence and leaves every layer's K / V^T in a cache, later steps run only the rows from <soi> on); bit 2 = do NOT reduce
 * step 0 (by default, with reuse, it skips the leading rows that no later row can see and runs identical unconditional sequences once;
 * the host waits once, before step 0, for that decision).  Optional injected noise (tests): exp_noise [steps,B*N,V],
 * uniform [steps,B,N].  out sampled int64 [B,N]. */
int showo_engine_t2i_generate(showo_engine* e, int64_t* ids_cond, int64_t* ids_uncond, const float* mask, int B, int L,
                              int num_vq_tokens, int text_len, int64_t mask_id, int id_offset, int codebook,
                              float guidance, int steps, const float* mask_len_host, const float* temps_host,
                              uint64_t seed, const float* exp_noise, const float* uniform, int use_graph,
                              int64_t* sampled_out, void* stream);
/* Incremental (KV-cached) decode used by mmu_generate (modeling_showo.py:183-240).  prefill: run the prompt
 * (ids or embeds, mask [1,1,L,L]) and keep K/V; step: append one token (id or embedding row) whose mask row
 * is `last prompt mask row + causal` exactly as the reference grows it (modeling_showo.py:203-217).
 * logits_last fp32 [vocab] = logits of the last position. */
int showo_engine_prefill(showo_engine* e, const int64_t* ids, const float* embeds, const float* mask, int L,
                         float* logits_last, void* stream);
int showo_engine_decode_step(showo_engine* e, const int64_t* id, const float* embed, float* logits_last, void* stream);
/* n_steps greedy (top_k = 1: the reference caller's setting, inference_mmu.py:81) continuation steps without host round trips:
 * { embed(tok) -> layers against the KV cache -> lm_head -> arg-max -> tok }.  tok int64[1] (device) holds the token to feed
 * first and the last produced one afterwards; out_tokens int64 [n_steps] (device); logits_ws fp32 [vocab] scratch.
 * use_graph: capture one step (position and mask row live in device memory) into a hipGraph and replay it. */
int showo_engine_decode_greedy(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, int use_graph,
                               void* stream);

/* Batched KV-cached greedy decode: nb <= 8 independent sequences (BASELINE cfg4's "batch=4 images"), nb caches, ONE weight stream per
 * token step -- the reference's batch-1 mmu_generate (models/modeling_showo.py:183-240) serves them one after the other
 * (inference_mmu.py:87-177) and streams the 2.66 GB of weights once per token per sequence.  Every sequence gets the bits of its own
 * batch-1 run (same lane split / accumulation order per sequence): tokens and logits equal nb showo_engine_decode_greedy runs.
 *   showo_engine_batch_begin(e, nb, cap_tokens): (re)sizes nb caches for cap_tokens >= max(prompt) + new tokens + 1 and clears them;
 *   showo_engine_batch_prefill(e, b, ...): showo_engine_prefill of sequence b into its slot (own length, own mask);
 *   showo_engine_batch_decode_greedy: tok int64 [nb] (device; in = first token to feed per sequence, out = last produced),
 *     out_tokens int64 [nb, n_steps], logits_ws fp32 [nb, vocab]; every sequence advances n_steps tokens (the caller cuts at <eot>);
 *     one hipGraph replay per step with the nb positions in device memory.  Precision 0 (bf16) or 2 (fp16 operands). */
int showo_engine_batch_begin(showo_engine* e, int nb, int cap_tokens);
/* Wide decode batch (opt-in; csrc/decode_wide.hip): showo_engine_batch_begin for 1 <= nb <= 32 sequences at precision 0, and the batch's
 * decode steps run two MFMA skinny GEMMs per layer (16 sequences per v_mfma_f32_16x16x32_bf16 column block) instead of one dot2
 * chain per sequence.  Every other showo_engine_batch_* entry serves a wide batch unchanged.  Contract of a wide batch: results are
 * deterministic, and a sequence's tokens, logits and log-probabilities do not depend on nb, on its slot or on the other slots
 * (an MFMA output column reads only its own sequence; the K order is fixed) -- but they are NOT the bits of the batch-1 run: same
 * rounding points (16-bit LayerNorm output, qkv, gelu(fc1), attention output; fp32 accumulators, residual, logits), another fp32
 * summation order.  Precision != 0 is refused here and by the decode entries. */
int showo_engine_batch_begin_wide(showo_engine* e, int nb, int cap_tokens);
/* The two kernels of the wide step alone (test hooks; arguments as ln_gemvB / out_gemvB take them, nb = 1..32 rows):
 *   ln_gemm:  h = LayerNorm(x [nb, H] fp32) as bf16 (the bits of showo_layernorm_f32_op16); out0 [nb, ld0] = bf16(W0 h + b0) or, when
 *             outf is given, outf [nb, ld0] = fp32(W0 h + b0); out1 [nb, ld1] = bf16(gelu_new(W1 h + b1)) (N1 = 0: absent).
 *             H <= 2048, H % 32 == 0, N0 % 16 == 0 when N1 > 0.
 *   out_gemm: x [nb, N] fp32 += (Wd attn + bd) + (W2 ffn + b2), attn [nb, K0] / ffn [nb, K1] bf16, K0 % 32 == K1 % 32 == 0. */
int showo_decode_wide_ln_gemm(const float* x, const float* lnw, const float* lnb, float eps, int H, const uint16_t* W0, const float* b0,
                              uint16_t* out0, float* outf, int N0, int ld0, const uint16_t* W1, const float* b1, uint16_t* out1, int N1,
                              int ld1, int nb, void* stream);
int showo_decode_wide_out_gemm(float* x, const uint16_t* Wd, const uint16_t* attn, const float* bd, int K0, const uint16_t* W2,
                               const uint16_t* ffn, const float* b2, int K1, int N, int nb, void* stream);
/* The dot2 GEMV kernels of the default decode step alone (test hooks; tests/test_decode_narrow_kernels_gpu.py).  Each call validates
 * (nonzero return and a message, nothing launched) and then runs the launcher the engine runs.  op: SHOWO_OP_BF16 / SHOWO_OP_F16, the
 * type of every 16-bit operand and output.  s0 / s1 != NULL: W0 / W1 are int8 row-major with one fp32 scale per row (bf16 activations,
 * every K a multiple of 16).  Weights, activations, x, lnw and lnb of ln_gemv must be 16-byte aligned.
 *   ln_gemv:  kernel 0 = ln_gemv2_kernel (nb = 1; ld0 / ld1 not read), 1 = ln_gemvB_kernel (nb = 1..8).  h = LayerNorm(x [nb, H]) as op
 *             values; out0 [nb, ld0] = op(W0 h + b0) or (outf given instead) outf [nb, ld0] = fp32(W0 h + b0); out1 [nb, ld1] =
 *             op(gelu_new(W1 h + b1)) (N1 = 0: absent).  H % 8 == 0, H <= 2048.  W0lo != NULL (kernel 1, bf16, outf, N1 = 0): the
 *             split head, W0 / W0lo the (hi, lo) bf16 halves of the weight rows.
 *   out_gemv: kernel 0 = out_gemv2_kernel (nb = 1; lda0 / lda1 not read), mode 0: x [N] = (x + (W0 a0 + b0)) + (W1 a1 + b1); mode 1:
 *             y2 [N] = W1 a1 + b1; mode 2: x = (x + (W0 a0 + b0)) + y2.  kernel 1 = out_gemvB_kernel (mode 0, nb = 1..8; x [nb, N],
 *             a0 [nb, lda0], a1 [nb, lda1]).  kernel 2 = out_dense_y2B_kernel (mode 2, nb = 2..4; y2 [nb, N]).  K0 % 8 == 0 <= 2048,
 *             K1 % 8 == 0 <= 8192; the half a mode does not use is not read. */
int showo_decode_narrow_ln_gemv(int kernel, int nb, int op, const float* x, const float* lnw, const float* lnb, float eps, int H,
                                const void* W0, const uint16_t* W0lo, const float* s0, const float* b0, uint16_t* out0, float* outf, int N0,
                                int ld0, const void* W1, const float* s1, const float* b1, uint16_t* out1, int N1, int ld1, void* stream);
int showo_decode_narrow_out_gemv(int kernel, int nb, int mode, int op, float* x, const void* W0, const uint16_t* a0, const float* s0,
                                 const float* b0, int K0, int lda0, const void* W1, const uint16_t* a1, const float* s1, const float* b1,
                                 int K1, int lda1, int N, float* y2, void* stream);
int showo_engine_batch_prefill(showo_engine* e, int b, const int64_t* ids, const float* embeds, const float* mask, int L,
                               float* logits_last, void* stream);
int showo_engine_batch_decode_greedy(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, int use_graph,
                                     void* stream);
/* showo_engine_batch_decode_greedy with a per-slot draw and a per-slot stop.  Host arrays of nb entries:
 *   top_k[b]        1 = arg-max (the greedy pick); <= 0 or >= vocab: no filter; else top-k (ties with the k-th value stay)
 *   temperature[b]  > 0 where top_k[b] != 1
 *   seed[b], draw0[b]  draw j of slot b in this call = showo_sample_topk(..., seed[b], step = draw0[b] + j)
 *   exp_noise       NULL, or nb entries each NULL or a device fp32 [*, vocab] table whose row draw0[b] + j replaces the Philox draw
 *   budget[b]       tokens slot b may still emit in this call (0 = idle from the start); eot: stop id, -1 = none
 * A slot stops after its budget[b]-th token or after emitting eot; for the rest of the call it is idle: its position stays, its
 * out_tokens entries are -1, it feeds a zero row (its K/V append rewrites one column beyond its live length, never beyond the cache).
 * tok int64 [nb] (device): in = the token each decoding slot feeds first, out = its last token.  out_tokens int64 [nb, n_steps]
 * (device).  produced[b] (host) = tokens slot b emitted; its cache length grows by that much.  Capacity: P0[b] + min(budget[b],
 * n_steps) <= cap for every slot.
 * Refill: showo_engine_batch_prefill(e, b, ...) on a running batch replaces the occupant of slot b (new length, new mask, re-zeroed
 * tail columns); the other slots' caches and positions are untouched, so a scheduler can refill a stopped slot between calls. */
int showo_engine_batch_decode_sample(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, const int* top_k,
                                     const float* temperature, const uint64_t* seed, const int* draw0, const float* const* exp_noise,
                                     const int* budget, int64_t eot, int* produced, int use_graph, void* stream);
/* mmu sessions: continue a KV cache with more prompt rows, and fork it to the slots of a decode batch ("mmu sessions").
 * For the mmu mask families every row at or beyond the end of the image sees what the last prefix row sees plus the columns up to
 * itself, so K / V^T of the prefix do not depend on what follows it and an appended row is, mask-wise, a decode row.
 *
 * showo_mask_append_rows: iv int32 [Ln, 4] (device), row j = the decode rule applied to position P + j: the run of last_iv (HOST, the
 * last prefill row's intervals) that ends at L0 is extended to P + j + 1, or an empty run becomes [L0, P + j + 1).  Error 6 when both
 * runs are non-empty and neither ends at L0 (showo_engine_decode_step's refusal), 1 when iv is not 16-byte aligned (a row is one
 * 16-byte store).  One launch.
 * showo_kv_fork: bit copy of K rows [0, P) of every (layer, head) ([heads, cap, 64] per layer, layer stride k_lstride elements) and of
 * V^T columns [0, P) of every (layer, head, dim) row ([heads, 64, cap] per layer) from a cache of capacity cap_src into one of capacity
 * cap_dst (multiples of 64, >= P; pointers 16-byte aligned, layer strides multiples of 8), and zeroes V^T columns [P, 64 ceil(P / 64))
 * of the destination.  Nothing else is written: K rows >= P and V^T columns beyond that tile keep their contents.  Two launches of
 * 16-byte loads and stores (HBM-bound: 4 P 64 nL nH bytes read and as many written). */
int showo_mask_append_rows(const int32_t* last_iv, int L0, int P, int Ln, int32_t* iv, void* stream);
int showo_kv_fork(const uint16_t* k_src, const uint16_t* vt_src, int cap_src, int64_t k_lstride_src, int64_t v_lstride_src,
                  uint16_t* k_dst, uint16_t* vt_dst, int cap_dst, int64_t k_lstride_dst, int64_t v_lstride_dst, int nL, int nH, int P,
                  void* stream);
/* showo_engine_prefill_append: Ln more prompt rows (ids or embeds, exactly one non-NULL) at positions P .. P + Ln - 1, P = the cache
 * length, with the intervals of showo_mask_append_rows; their K / V^T join the decode cache, logits_last fp32 [vocab] = the logits of
 * row P + Ln - 1, the cache length becomes P + Ln.  prompt_len and the last prefill row's intervals stay those of showo_engine_prefill
 * (decode steps and further appends keep extending the same run).  Every precision showo_engine_prefill serves; the cache must have
 * been prefilled under the current one.  Ln == 1 runs showo_engine_decode_step's layer and head launches (same bits) behind the
 * tail-zeroing launch every append makes when P + Ln is no multiple of 64.  Errors: 1 without a
 * prefill, 5 when P + Ln + 1 exceeds the cache capacity or max_position_embeddings, or Ln the workspace rows (max_batch * max_seq).
 * showo_engine_cache_rewind: forget the rows >= len (prompt_len <= len <= cache length) and re-zero the V^T columns
 * [len, 64 ceil(old length / 64)).  Invariant kept by prefill, append, rewind and fork: V^T columns [cache length, 64 ceil(cache
 * length / 64)) of the cache they wrote are zero, so the attention's last key tile never multiplies P = 0 with a stale NaN.
 * showo_engine_cache_state: any out pointer may be NULL; epoch = showo_engine_prefill calls on this engine so far (a host object
 * that continues the cache can tell that another prompt replaced it).
 * showo_engine_cache_ptrs / showo_engine_batch_slot_ptrs (test hooks): device pointers and layer strides (elements) of the decode
 * cache / of slot b of the running batch, and the slot's capacity. */
int showo_engine_prefill_append(showo_engine* e, const int64_t* ids, const float* embeds, int Ln, float* logits_last, void* stream);
int showo_engine_cache_rewind(showo_engine* e, int len, void* stream);
int showo_engine_cache_state(const showo_engine* e, int* cache_len, int* prompt_len, int* cap, int64_t* epoch);
int showo_engine_cache_ptrs(showo_engine* e, uint16_t** k, uint16_t** vt, int64_t* k_lstride, int64_t* v_lstride);
int showo_engine_batch_slot_ptrs(showo_engine* e, int b, uint16_t** k, uint16_t** vt, int64_t* k_lstride, int64_t* v_lstride, int* cap);
/* showo_engine_batch_fork: showo_kv_fork of the decode cache [0, cache length) into slot b of the running batch; the slot takes the
 * engine's cache length, prompt_len and last prefill row.  Like showo_engine_batch_prefill on a running batch it replaces the
 * occupant and leaves the other slots alone.  Refused: cache length + 1 > the batch's capacity (5), precision 1 (1), a cache prefilled
 * under another precision than the current one (1).
 * showo_engine_batch_prefill_append: showo_engine_prefill_append on slot b (the same code with the slot as destination: the same
 * prefix and rows give the same bits in the engine's cache and in a forked slot). */
int showo_engine_batch_fork(showo_engine* e, int b, void* stream);
int showo_engine_batch_prefill_append(showo_engine* e, int b, const int64_t* ids, const float* embeds, int Ln, float* logits_last,
                                      void* stream);
/* Shared-prefix slots (opt-in; csrc/attn_shared.hip, DESIGN.md "Shared-prefix slots"): a wide batch whose slots hold only a SUFFIX
 * cache and read the engine's decode cache [0, P) in place, P = the cache length when the batch begins.  With base = P & ~63, key
 * k >= P of a slot lives at row / column k - base of its suffix cache (K [heads, cap_s, 64], V^T [heads, 64, cap_s] per layer, cap_s a
 * multiple of 64); rows below P - base of a suffix cache are dead.  Per layer the step runs two launches in place of the wide step's
 * attention: the prefix launch (grid heads x 64-key splits of [0, P), one wave each: q prep of all nb slots, S^T = K Q^T and
 * O^T = V^T P^T on v_mfma_f32_32x32x16_bf16, fp32 partials (m, l, o[64]) per (split, head, slot)) and the suffix + merge launch (grid
 * heads x nb: the single-query attention over the slot's suffix with the new token's K row / V^T column appended, then the partials
 * merged in split order by log-sum-exp rescaling).  A slot's row depends only on its own query, the prefix and its own suffix.
 *
 * showo_engine_batch_begin_shared: showo_engine_batch_begin_wide whose capacity counts suffix tokens: cap_suffix_tokens >= (P - base) +
 *   appended rows + new tokens + 1.  Refused (1) without a prefill or when the cache was prefilled under another precision.
 * showo_engine_batch_attach_append: fills slot b: the Ln rows are appended to the ENGINE'S cache at P by the code of
 *   showo_engine_prefill_append (logits_last has its bits), K rows / V^T columns [P, P + Ln) are copied into the slot, and the engine's
 *   cache is rewound to P (also when a step failed).  Replaces the occupant of b, leaves the other slots alone.
 * Every showo_engine_batch_decode_* entry serves a shared batch; it refuses (1) once the engine's cache is not the one the batch began
 * on (another prefill, a length other than P, another precision).  showo_engine_batch_slot_ptrs reports the suffix cache and cap_s;
 * showo_engine_batch_fork / _batch_prefill / _batch_prefill_append refuse a shared batch (1).
 * showo_engine_batch_shared_state (test hook): P, base and cap_s of the running shared batch (any out pointer may be NULL).
 *
 * The kernels alone (test hooks):
 * showo_attn_decode_shared: one layer's two launches on caller buffers.  qkv [nb, 3 heads 64] bf16 projection rows; k_pre / vt_pre one
 *   layer of a prefix cache of capacity cap_pre; k_suf / vt_suf [nb][heads][cap_suf][64] / [nb][heads][64][cap_suf]; pre_iv (HOST) the
 *   two prefix intervals, clipped to [0, P) here; pos_dev int [nb] (device) absolute positions, P <= pos < base + cap_suf; lk_max = an
 *   upper bound of pos + 1 (0: none); O [nb, heads 64] bf16; ws fp32 of showo_attn_shared_ws_elems(heads, P) elements.  Rows >= nb of
 *   O and ws are neither read nor written.  Keys >= P of the prefix buffers may hold anything.
 * showo_attn_shared_ws_elems: returns the element count (not an error code); 0 for bad arguments or a count beyond INT_MAX.
 * showo_kv_copy_rows: showo_kv_fork for a row range: K rows / V^T columns [r0, r1) of the source go to [r0 - base, r1 - base) of the
 *   destination (base a multiple of 64, base <= r0 < r1), V^T columns [r1 - base, 64 ceil((r1 - base) / 64)) of the destination are
 *   zeroed, nothing else is written. */
int showo_engine_batch_begin_shared(showo_engine* e, int nb, int cap_suffix_tokens);
int showo_engine_batch_attach_append(showo_engine* e, int b, const int64_t* ids, const float* embeds, int Ln, float* logits_last,
                                     void* stream);
int showo_engine_batch_shared_state(const showo_engine* e, int* P, int* base, int* cap_s);
int showo_attn_decode_shared(const uint16_t* qkv, const float* qln_w, const float* qln_b, const float* kln_w, const float* kln_b,
                             const float* cosT, const float* sinT, const uint16_t* k_pre, const uint16_t* vt_pre, int cap_pre,
                             uint16_t* k_suf, uint16_t* vt_suf, int cap_suf, const int32_t* pre_iv, int P, const int* pos_dev, int lk_max,
                             uint16_t* O, float* ws, int nb, int nH, int rot, float eps, void* stream);
int showo_attn_shared_ws_elems(int nH, int P);
int showo_kv_copy_rows(const uint16_t* k_src, const uint16_t* vt_src, int cap_src, int64_t k_lstride_src, int64_t v_lstride_src,
                       uint16_t* k_dst, uint16_t* vt_dst, int cap_dst, int64_t k_lstride_dst, int64_t v_lstride_dst, int nL, int nH,
                       int r0, int r1, int base, void* stream);
/* Next-token draw of the AR decode (modeling_showo.py:220-228): x = logits / temperature; values below the top_k-th largest
 * are dropped (top_k <= 0 or >= V: none); token = multinomial(softmax(x), 1) computed as argmax_i p_i / E_i, E ~ Exp(1):
 * E = exp_noise[step * V + i] when exp_noise != NULL (parity tests inject the reference's draws), else Philox(seed; step, i). */
int showo_sample_topk(const float* logits, int V, int top_k, float temperature, const float* exp_noise, uint64_t seed, int step,
                      int64_t* tok, void* stream);
/* showo_engine_decode_greedy with that draw instead of the arg-max; draw j of the call uses noise row / stream step0 + j. */
int showo_engine_decode_sample(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, int top_k,
                               float temperature, const float* exp_noise, uint64_t seed, int step0, int use_graph, void* stream);
/* Nucleus (top-p) sampling, the reference's top_k_top_p_filtering (models/sampling.py:80-118) in front of the same draw.
 * x_i = logits[i] / temperature (fp32 division):
 *   1. top-k exactly as showo_sample_topk (ties with the k-th value stay; top_k <= 0 or >= V: no filter): the candidates;
 *   2. p = softmax over the candidates;
 *   3. token i is kept iff the probability mass of the candidates with strictly larger x is <= top_p;
 *   token = argmax_i p'_i / E_i, p' = p renormalised over the kept set, E as in showo_sample_topk (same Philox counters).
 * This is the reference's rule wherever no tie sits at the cut; the largest token always stays (min_tokens_to_keep = 1); the rule
 * does not depend on a sort order; all candidates equal to the cut value stay (tie-inclusive, like top-k).  On the device the masses
 * are integers, w_i = (uint64)(expf(x_i - max) * 2^40) added with integer atomics (bit-deterministic run to run), and
 * kept(i) <=> (double)A_i <= (double)top_p * (double)S with A_i the sum of w above x_i and S the candidates' sum.
 * 0 < top_p < 1 filters; top_p >= 1 is off: the launch and the bits of the call without top_p; top_p <= 0 or NaN: error 1, nothing
 * is launched.  top_k == 1 stays the arg-max.  V < 2^24.
 * showo_engine_decode_sample_p / showo_engine_batch_decode_sample_p: showo_engine_decode_sample / _batch_decode_sample with that
 * filter; top_p of the batched form is a host array of nb entries (per slot; ignored where top_k[b] == 1). */
int showo_sample_topk_topp(const float* logits, int V, int top_k, float top_p, float temperature, const float* exp_noise, uint64_t seed,
                           int step, int64_t* tok, void* stream);
int showo_engine_decode_sample_p(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, int top_k, float top_p,
                                 float temperature, const float* exp_noise, uint64_t seed, int step0, int use_graph, void* stream);
int showo_engine_batch_decode_sample_p(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, const int* top_k,
                                       const float* top_p, const float* temperature, const uint64_t* seed, const int* draw0,
                                       const float* const* exp_noise, const int* budget, int64_t eot, int* produced, int use_graph,
                                       void* stream);
/* Log-probabilities.  For one fp32 logits row x[0, V) and a target token t:
 *   lp   = x[t] - max(x) - log sum_i exp(x[i] - max(x))   the log-softmax of the RAW logits (temperature 1, in front of any top-k /
 *                                                         top-p filter): what torch.log_softmax(x, -1)[t] returns;
 *   rank = #{ i : x[i] > x[t] }                           strict: 0 for the arg-max and for everything tied with it.
 * t < 0 (the -100 of the label convention): lp = 0.0f, rank = -1.  t >= V: lp = NaN, rank = -1 (the embedding kernel's poisoning of
 * out-of-range ids).  -inf entries add nothing to the sum, a -inf target gives lp = -inf.  The maximum is subtracted before exp.
 * One 1024-thread block per row, two passes of 16-byte loads over the row behind a peel to its alignment (max and rank, then the
 * sum).  The sum runs over integers, w_i = (uint64)(expf(x_i - max) * 2^40) (exact scaling, truncating conversion, V < 2^24), so it
 * does not depend on which lane met which element: the same row bits and target give the same lp bits on every run, at every row
 * alignment and from every caller below.  |lp - exact| <= ~3e-7 (1 + |lp|): the truncation costs V 2^-40 relative to a sum >= 1.
 * showo_logprob_rows: rows logits + r * ld (ld >= V, any 4-byte alignment), r < nrows, against targets[r]; logprob fp32 [nrows],
 * rank int32 [nrows] or NULL.  nrows == 0 launches nothing.
 * showo_engine_decode_sample_lp / showo_engine_batch_decode_sample_lp: showo_engine_decode_sample_p / _batch_decode_sample_p with one
 * more launch per step, behind the token boundary and inside the captured step, that scores the token the step stored against the
 * step's row of logits_ws: logprobs fp32 [n_steps] / [nb, n_steps] (device) is indexed like out_tokens, ranks likewise or NULL.  An
 * idle slot's entries are 0.0f / -1 where its out_tokens entry is -1.  The token launches are those of the calls without (top_k == 1:
 * the greedy step, token-seam form included; top_p >= 1: the plain top-k draw), so tokens keep their bits; logprobs == NULL is that
 * call exactly.  The batched form also takes top_p == NULL (no slot filters).  Every precision the underlying loop serves.
 * showo_engine_score: ONE forward exactly as showo_engine_forward_rows runs it (mask / showo_engine_use_intervals, every precision),
 * then, for chunks of at most chunk_rows rows, the head over the full vocabulary into an engine-owned [chunk_rows, V] workspace and
 * showo_logprob_rows on it: rows int32 [n] (device) index the B * L residual rows, targets int64 [n] (device), logprob [n], rank [n]
 * or NULL.  chunk_rows <= 0: the largest chunk within 256 MB.  [n, V] is never allocated whole; n == 0 launches nothing.
 * showo_engine_prefill_append_score: showo_engine_prefill_append on ids with the head run on all Ln appended rows: logprob[j] scores
 * ids[j], from the logits of appended row j - 1 for j >= 1 and from logits_prev fp32 [V] (the logits of the last cached row; must
 * not be logits_last) for j == 0 -- NaN / -1 when logits_prev is NULL.  logits_last and the cache are left as the plain append leaves
 * them.  The engine's own cache only. */
int showo_logprob_rows(const float* logits, int64_t ld, int nrows, int V, const int64_t* targets, float* logprob, int32_t* rank,
                       void* stream);
int showo_engine_decode_sample_lp(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, int top_k, float top_p,
                                  float temperature, const float* exp_noise, uint64_t seed, int step0, float* logprobs, int32_t* ranks,
                                  int use_graph, void* stream);
int showo_engine_batch_decode_sample_lp(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, const int* top_k,
                                        const float* top_p, const float* temperature, const uint64_t* seed, const int* draw0,
                                        const float* const* exp_noise, const int* budget, int64_t eot, int* produced, float* logprobs,
                                        int32_t* ranks, int use_graph, void* stream);
int showo_engine_score(showo_engine* e, const int64_t* ids, const float* embeds, const float* mask, int B, int L, const int32_t* rows,
                       const int64_t* targets, int n, int chunk_rows, float* logprob, int32_t* rank, void* stream);
int showo_engine_prefill_append_score(showo_engine* e, const int64_t* ids, int Ln, const float* logits_prev, float* logprob, int32_t* rank,
                                      float* logits_last, void* stream);
/* Logit adjustment: repetition penalty and logit bias in front of the pick, on the device (csrc/logit_adjust.hip).
 * For one fp32 logits row x[0, V), a token set S, a penalty theta (finite, > 0) and an optional fp32 bias row beta[0, V):
 *   r_i = x_i                                  i not in S
 *   r_i = x_i * theta  if x_i < 0,  else  x_i / theta     i in S   (fp32 multiply; fp32 IEEE division)
 *   y_i = r_i + beta_i                         (no bias row: y_i = r_i)
 * Hugging Face's RepetitionPenaltyLogitsProcessor followed by a sequence bias, both ahead of temperature / top-k / top-p, which the
 * picks apply to y exactly as they apply them to x.  -0.0 and 0.0 count as "not < 0"; -inf stays -inf; beta_i = -inf bans token i
 * (the callers refuse +inf and NaN in beta).  theta == 1 without a bias row is a bit copy.  y goes to a second row: x is never
 * overwritten, and log-probabilities stay the log-softmax of x.  The work is elementwise, so equal rows give equal bits at every
 * row alignment, row count and from every caller below.
 * The set is a bitmap (part of this ABI): uint32 words [rows, seen_ld], seen_ld >= ceil(V / 32); token i is bit i & 31 of word
 * i >> 5 of its row; bits at positions >= V of the last word are never set.  The caller owns it (and clears it).
 * showo_seen_mark: sets the bits of ids int64 [n] (device) in ONE bitmap row; ids < 0 or >= V are ignored (the -1 of an idle slot's
 * output row may be passed in); n == 0 launches nothing.
 * showo_logits_adjust: rows logits + r * ld -> out + r * ld_out (ld, ld_out >= V; 4-byte aligned), r < nrows, one launch per 32
 * rows.  mark: NULL, or int64 [nrows] (device): row r treats mark[r] as a member of its set and ORs its bit into the bitmap
 * (atomically; the output does not depend on when that lands); a mark outside [0, V) means none.  penalty: HOST float [nrows].
 * bias: NULL, or a HOST array of nrows device pointers (fp32 [V] rows), NULL entries allowed.  active: NULL, or int32 [nrows]
 * (device): a row whose entry is 0 is neither marked nor written.  Error 1, before any launch: out overlapping logits, a penalty
 * that is not finite or not > 0, seen_ld too small.  nrows == 0 launches nothing.
 * showo_engine_decode_sample_adj / showo_engine_batch_decode_sample_adj: showo_engine_decode_sample_lp / _batch_decode_sample_lp
 * (logprobs may be NULL, the batched top_p may be NULL) with one adjust launch per step, inside the captured step, between the
 * lm_head and the pick: it reads logits_ws, marks the token the step FED (*tok; tok[b] of the slots that are still decoding -- an
 * idle or stopped slot is skipped) and writes adj_ws fp32 [nb, V] (device), which the pick reads.  The log-probability launch keeps
 * reading logits_ws: log-probabilities are those of the RAW logits.  seen: bitmap [nb, seen_ld] (nb = 1 for the batch-1 form);
 * penalty HOST float [nb]; bias NULL or HOST [nb] of device rows, NULL entries allowed; all fixed for the call.  The caller marks
 * what the set starts with (showo_seen_mark) and adjusts the prefill logits for the first token (showo_logits_adjust).  With an
 * adjustment the batch-1 greedy step (top_k == 1) takes showo_argmax_f32 on adj_ws and the separate store / increment launches
 * instead of the fused token seam.  A row with theta == 1 and no bias draws the bits of the call without. */
int showo_seen_mark(uint32_t* seen_row, int V, const int64_t* ids, int n, void* stream);
int showo_logits_adjust(const float* logits, int64_t ld, int nrows, int V, uint32_t* seen, int64_t seen_ld, const int64_t* mark,
                        const float* penalty, const float* const* bias, const int32_t* active, float* out, int64_t ld_out, void* stream);
int showo_engine_decode_sample_adj(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, int top_k,
                                   float top_p, float temperature, const float* exp_noise, uint64_t seed, int step0, float* logprobs,
                                   int32_t* ranks, uint32_t* seen, int64_t seen_ld, const float* penalty, const float* const* bias,
                                   float* adj_ws, int use_graph, void* stream);
int showo_engine_batch_decode_sample_adj(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws,
                                         const int* top_k, const float* top_p, const float* temperature, const uint64_t* seed,
                                         const int* draw0, const float* const* exp_noise, const int* budget, int64_t eot, int* produced,
                                         float* logprobs, int32_t* ranks, uint32_t* seen, int64_t seen_ld, const float* penalty,
                                         const float* const* bias, float* adj_ws, int use_graph, void* stream);
/* Sequence rules: no-repeat n-grams, multi-token bad words and a minimum length in front of the pick, on the device
 * (csrc/seq_rules.hip; DESIGN.md, "Sequence rules").  Per row, the history h[0, len) is a list of token ids in device memory: the
 * request's context ids (ctx_len of them), then every token the call has fed.  A token w is banned for the pick of a row if
 *   n-gram      n = ngram >= 1: some j, 0 <= j <= len - n, has h[j .. j+n-2] == h[len-n+1 .. len-1] (n - 1 tokens) and w == h[j+n-1]
 *               (Hugging Face's NoRepeatNGramLogitsProcessor on h; n == 1 bans every token of h), or
 *   bad word    a sequence s of the row's table with m = |s| >= 2 and len >= m - 1 has h[len-m+1 .. len-1] == s[0 .. m-2] and
 *               w == s[m-1] (NoBadWordsLogitsProcessor, without its skip of a prefix that is the whole input), or
 *   min length  w == eot and len - ctx_len < min_new (MinNewTokensLengthLogitsProcessor).
 * A banned token's fp32 entry becomes -inf (0xFF800000); every other entry keeps its bits.  Ids are compared as plain integers; an
 * id outside [0, V), in the history or in a table, is never stored to: no store lands outside [row, row + V).
 * struct showo_seq_rules, part of this ABI and fixed for a call: hist int32 [nrows, hist_ld] and hist_len int32 [nrows] on the device, owned
 * by the caller (which seeds them with the context); ngram (0: off, at most 16), ctx_len, min_new: HOST int32 [nrows]; eot (< 0: no
 * minimum-length rule); bad: NULL, or a HOST array of nrows device pointers to bad-word tables, NULL entries allowed.
 * Bad-word table (flat int32, device): t[0] = S, the number of sequences; t[1 .. S+1] = S + 1 offsets, off[0] = 0, non-decreasing;
 * t[S+2 ..] = the tokens: sequence i is tokens[off[i], off[i+1]).  Sequences shorter than 2 are skipped (a single id is a bias of
 * -inf).  The kernel walks any S and any length; the table is trusted as the bitmap of the adjustment is.
 * Limits: ngram <= 16, hist_ld in [1, 2^31); nothing else (rows go 32 to a launch).  Beyond them: error 1 before any launch.
 * showo_seq_ban: works in place on the fp32 rows rows + r * ld (ld >= V, 4-byte aligned), r < nrows.  mark: NULL, or int64 [nrows]
 * (device): a mark in [0, V) is the newest member of row r's history -- the rules see hist[r][0, len0) ++ [mark[r]] -- and is stored
 * (hist[r][len0] = mark[r], hist_len[r] = len0 + 1) if len0 < hist_ld; a full row stores nothing and nothing is read or written
 * beyond hist_ld; a mark outside [0, V) (the -1 of an idle slot) means none.  active: NULL, or int32 [nrows] (device): a row whose
 * entry is 0 is neither appended to nor written.  A row left without a finite entry is picked from as the picks do today: the
 * arg-max returns token 0 and the sampled draw sees NaN probabilities (the callers do not guard it).
 * showo_engine_decode_sample_seq / showo_engine_batch_decode_sample_seq: the _adj entries with `rules` in front of use_graph: one
 * ban launch per step directly behind the adjust launch, on adj_ws, marking the token the step FED with the activity the adjust
 * launch uses; a request without penalty or bias passes penalty 1 and no bias row (the adjust launch is then a bit copy).  The
 * batched entry bans the <eot> of rules->eot, which the caller sets to its `eot`. */
typedef struct showo_seq_rules {
    int32_t* hist;
    int64_t hist_ld;
    int32_t* hist_len;
    const int32_t* ngram;
    const int32_t* ctx_len;
    const int32_t* min_new;
    int64_t eot;
    const int32_t* const* bad;
} showo_seq_rules;
int showo_seq_ban(float* rows, int64_t ld, int nrows, int V, const showo_seq_rules* rules, const int64_t* mark, const int32_t* active,
                  void* stream);
int showo_engine_decode_sample_seq(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, int top_k,
                                   float top_p, float temperature, const float* exp_noise, uint64_t seed, int step0, float* logprobs,
                                   int32_t* ranks, uint32_t* seen, int64_t seen_ld, const float* penalty, const float* const* bias,
                                   float* adj_ws, const showo_seq_rules* rules, int use_graph, void* stream);
int showo_engine_batch_decode_sample_seq(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws,
                                         const int* top_k, const float* top_p, const float* temperature, const uint64_t* seed,
                                         const int* draw0, const float* const* exp_noise, const int* budget, int64_t eot, int* produced,
                                         float* logprobs, int32_t* ranks, uint32_t* seen, int64_t seen_ld, const float* penalty,
                                         const float* const* bias, float* adj_ws, const showo_seq_rules* rules, int use_graph,
                                         void* stream);
/* Beam search (csrc/beam.hip; DESIGN.md, "Beam search"): Hugging Face beam search for one prompt, do_sample=False, no processors,
 * B = number of beams = the slots of a regular batch, every slot a showo_engine_batch_fork of the engine's cache.
 * A candidate (beam b, token i) of a step scores cum[b] + lp(b, i), lp the log-softmax of the RAW logits (showo_logprob_rows' value
 * and bits).  The 2B best over all B x V are taken in the order (score descending, beam ascending, token ascending) and walked in that
 * order: an <eot> candidate of rank < B becomes a finished hypothesis with final = score / len ** length_penalty (len = generated
 * tokens, the <eot> included), one of rank >= B is dropped; every other candidate becomes the next live beam until B are filled.  The B
 * best hypotheses are kept (a new one beats the worst only strictly).  Done: B are finished and (early_stopping, or worst final >=
 * best live score / len ** length_penalty).  At max_new tokens without done the B live beams join the table (len = max_new).
 *
 * showo_beam_select (the selection alone; test hook): logits fp32 rows logits + b * ld (any 4-byte alignment), b < nb, cum fp32 [nb]
 *   -> norm fp32 [nb, 2] = (row max mx, logS = logf(S 2^-40), S the integer sum of showo_logprob_rows) and cand [2B] records
 *   { float score; int32 beam; int32 token; } in the order above, score = cum[b] + ((x - mx) - logS) in exactly this fp32 order: given
 *   norm, the scores and the selection are a pure function of the input bits at every row alignment.  1 <= nb, B <= 8, 2B <= V < 2^24.
 *   A -inf logit scores -inf.  A row with NaN or +inf (or of -inf alone) gets logS = NaN and the candidates (NaN, token -1), which
 *   rank behind every other row's.  ws: fp32 [nb, 2B, 2] (the per-row survivors).  Two launches: one 1024-thread block per row (the
 *   normaliser, then the picks from per-thread bests: a block reduction per pick), one 128-thread merge block.
 * showo_kv_permute_rows (the parent copy alone; test hook): k_slots / vt_slots are DEVICE tables of B slot pointers ([layers] of
 *   [heads][cap][64] K and [heads][64][cap] V^T with the given layer strides, elements).  Beam c takes K rows / V^T columns [r0, r1) of
 *   beam parent[c], for every c with parent[c] != c (an index outside [0, B) counts as c).  parent int32 [B] and r1 int32 [1] are read
 *   from DEVICE memory by the launches (r1 is clipped to r0 + span and cap).  A gather launch copies slot parent[c] -> stage[c], a
 *   scatter launch stage[c] -> slot c, so every map is served.  Whole 16-byte chunks move: of V^T also the columns [8 floor(r0 / 8), r0)
 *   -- precondition: below r0 all beams hold identical bits -- and [r1, 8 ceil(r1 / 8)), beyond the live length; nothing else is
 *   written.  stage_k / stage_vt: showo_kv_permute_stage_elems(layers, heads, B, span) 16-bit elements each (returns the count, not
 *   an error code; 0 for bad arguments), B layers heads 64 (8 ceil(span / 8) + 8).
 * showo_engine_batch_beam_begin: starts a search of at most max_new tokens on the running batch and takes its first step, on
 *   logits_row fp32 [V] (the prefill's / append's last row): the 2B best tokens of that row with cumulative score 0; no cache row moves.
 *   state: int32 [64 + max_new + 1] (device, 8-byte aligned), written here: word 0 generated length t, 1 done, 2 finished hypotheses,
 *   3 worst final (fp32), 4 max_new, 5 B, 8.. cum fp32 [8], 16.. the last parent map [8], 32.. int64 [8] the tokens the beams feed next,
 *   64 + len the fp32 divisor (float)pow(len, length_penalty).  Trace (device, [max_new, B], row t - 1 = the live beams after t tokens):
 *   tr_parent / tr_token int32, tr_cum / tr_lp fp32 (lp of that token).  hyp (device): [B] records { int32 step, beam, kind; float final;
 *   int32 len; float sumlp; int32 order; float lp (of its last token) } sorted best first; kind 0 ended on <eot>: its tokens are those of live beam `beam` of
 *   trace row step - 1 (none for step 0) plus <eot>; kind 1 is live beam `beam` of row `step`.  Token sequences are rebuilt from the
 *   back-pointers.  eot < 0: nothing finishes early.
 *   Refused before anything changes: a wide or shared batch (1), slots of unequal length (1), what showo_engine_batch_decode_greedy
 *   refuses, V < 2B (1), a non-finite length_penalty (1), cache length + max_new - 1 beyond the capacity (5).
 * showo_engine_batch_decode_beam: the next min(n_steps, max_new - t) steps, each batch_step_layers -> select -> seam -> permute pair
 *   over [cache length at begin, position + 1), one captured step replayed on `stream`.  Once done is set the remaining steps of the
 *   call idle (zero rows, frozen positions, no table changes), and a call on a finished search runs nothing.  The caller reads done and
 *   the tables once per call.  logits_ws fp32 [B, V].  The same state / trace / hyp pointers as at begin; precisions 0, 2 and 3. */
int showo_beam_select(const float* logits, int64_t ld, int nb, int V, const float* cum, int B, float* norm, void* cand, float* ws,
                      void* stream);
int64_t showo_kv_permute_stage_elems(int nL, int nH, int B, int span);
int showo_kv_permute_rows(uint16_t* const* k_slots, uint16_t* const* vt_slots, int cap, int64_t k_lstride, int64_t v_lstride, int nL, int nH,
                          int B, const int32_t* parent, int r0, const int32_t* r1, uint16_t* stage_k, uint16_t* stage_vt, int span,
                          void* stream);
int showo_engine_batch_beam_begin(showo_engine* e, int32_t* state, int max_new, const float* logits_row, int64_t eot, float length_penalty,
                                  int early_stopping, int32_t* tr_parent, int32_t* tr_token, float* tr_cum, float* tr_lp, void* hyp,
                                  void* stream);
int showo_engine_batch_decode_beam(showo_engine* e, int32_t* state, int n_steps, int64_t eot, float length_penalty, int early_stopping,
                                   float* logits_ws, int32_t* tr_parent, int32_t* tr_token, float* tr_cum, float* tr_lp, void* hyp,
                                   int use_graph, void* stream);
/* greedy/top-k=1 pick on device: out int64[1] = argmax(logits) (first maximal index, like torch.topk/multinomial on a one-hot). */
int showo_argmax_f32(const float* x, int n, int64_t* out, void* stream);

typedef struct showo_vq showo_vq;
typedef struct {
    int ch, z_channels;
    int enc_ch_mult[8], enc_blocks[8], enc_levels;
    int dec_ch_mult[8], dec_blocks[8], dec_levels;
    int max_batch, max_res; /* workspace sizing */
    int precision;          /* 0 = bf16 operands; 1 = split (hi+lo) bf16 operands, fp32-class accuracy (default of MAGVITv2) */
} showo_vq_config;
int showo_vq_create(const showo_vq_config* cfg, showo_vq** out);
void showo_vq_destroy(showo_vq* v);
/* key = reference state-dict key ("decoder.up.3.block.0.conv1.weight", ...); src fp32 in the reference's
 * layout (conv: [Cout,Cin,kh,kw]); repacked to channel-last bf16 inside. */
int showo_vq_load(showo_vq* v, const char* key, const float* src, int64_t n, void* stream);
int showo_vq_missing(const showo_vq* v);
/* A/B switches of the low-resolution tail (1 = on, the default; 0 = off; negative = leave unchanged).  attn_batched: the attention block
 * runs V^T, Q K^T, softmax and P V once for all images (showo_gemm_bf16x3_batched; split precision, B > 1) instead of looping over
 * them.  gn_fold: GroupNorm applies from <= SHOWO_GN_FOLD_MAX partials (showo_gn_apply_part) without the finalize launch.  The outputs
 * have the same bits with either setting of those two.  thin_conv: decoder.conv_out (Cout = 3) runs showo_conv3x3_thin_bf16x3 instead of
 * the MFMA conv (split precision); this one changes the image's low bits.  SHOWO_VQ_ATTN_BATCH=0 / SHOWO_GN_FOLD=0 /
 * SHOWO_CONV_THIN=0 select 0 at creation. */
int showo_vq_set_tail(showo_vq* v, int attn_batched, int gn_fold, int thin_conv);
/* One attention block alone (prefix = "decoder.mid.attn_1" or "encoder.mid.attn_1"), in place on x fp32 channel-last [B, H * W, C]:
 * x += AttnBlock(x) (common_modules.py:187-211).  Per image the result does not depend on B; tests of the batched form use it. */
int showo_vq_attn_block(showo_vq* v, const char* prefix, float* x, int B, int H, int W, void* stream);
/* MAGVITv2.decode_code (modeling_magvitv2.py:429-433): ids int64 [B,h*w] -> image fp32 NCHW [B,3,16h,16w]. */
int showo_vq_decode_code(showo_vq* v, const int64_t* ids, int B, int h, int w, float* image, void* stream);
/* MAGVITv2.get_code (modeling_magvitv2.py:423-427): pixels fp32 NCHW [B,3,H,W] -> ids int64 [B,(H/16)*(W/16)];
 * z_out (optional) fp32 [B,13,H/16,W/16] = pre-quantisation latents (for the |z|<eps agreement test). */
int showo_vq_get_code(showo_vq* v, const float* pixels, int B, int H, int W, int64_t* ids, float* z_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training step (reference Showo.forward with labels + loss.backward(), models/modeling_showo.py:59-102,
 * training/train.py:590-612).  A trainer borrows an engine's weights and workspaces and owns the saved activations,
 * the transposed weight images of the dgrad GEMMs and one fp32 gradient buffer per reference parameter.
 * ------------------------------------------------------------------------------------------- */
typedef struct showo_trainer showo_trainer;
int showo_train_create(showo_engine* e, int max_batch, int max_seq, showo_trainer** out);
void showo_train_destroy(showo_trainer* t);
/* The transposed images of the dgrad GEMMs follow the engine's per-tensor version stamps (showo_engine_load and the fused AdamW
 * stamp every write): the next forward rebuilds the images of the tensors that changed, and only those.  This call marks every
 * image stale regardless. */
int showo_train_invalidate_weights(showo_trainer* t);
/* Trainable set (reference: torch AdamW built over the `requires_grad` parameters only, training/train.py:210-223).  key = a
 * reference state-dict key; every tensor starts trainable.  A frozen tensor gets no weight-gradient launch, no optimizer update
 * (showo_train_adamw_step) and no image rebuild; a launch whose only consumer is frozen does not run (a backward phase with nothing
 * trainable at or below it launches nothing).  Zero contract: after a backward every frozen tensor's gradient slot reads as zeros
 * (cleared once, when it froze), so showo_grad_clip_norm over the flat buffer is the norm over the trainable tensors.  With every
 * tensor trainable the launch sequence and every bit are those of the full backward.
 * Bias coupling: the dense / fc2 bias gradients of block i are column sums written by the LayerNorm backward of block i + 1 (of
 * the final LayerNorm for the top block); that write happens whenever block i's biases train. */
int showo_train_set_trainable(showo_trainer* t, const char* key, int on);
/* whether d(loss)/d(input embeddings) of a showo_train_forward_embeds is wanted (default 1; 0: showo_train_input_grad refuses and
 * the backward stops at the lowest block that trains) */
int showo_train_set_input_grad(showo_trainer* t, int on);
/* Gradient accumulation over micro-batches (reference: accelerator.accumulate, training/train.py:589-631).  While on, every
 * parameter-gradient write of showo_train_backward[_head[_dev] / _layer / _embed] ADDS into the flat buffer (showo_gemm_tn_bf16 /
 * showo_colsum_bf16 with accumulate, the showo_*_acc side outputs, SHOWO_EPI_RESID_F32 on the SHOWO_TRAIN_TN=0 path) and the
 * embedding phase adds its row sums into the rows the micro-batch touches without clearing the table.  A window is: off for its
 * first micro-batch, on for the rest; the sum differs from the fp64 sum of the per-micro-batch gradients by one fp32 rounding per
 * added micro-batch.  Frozen slots stay zero and side outputs pointed at scratch stay overwriting.  Default off. */
int showo_train_set_accumulate(showo_trainer* t, int on);
/* Loss head on the labelled rows only.  mode 0 (default): every launch as before.  mode 1: a showo_train_forward[_embeds] WITH labels
 * runs the census above first, waits on the host once (after the blocks are queued, on an event recorded behind the census) for
 * Tc, and runs the final LayerNorm (gathered), the lm_head GEMM and the cross-entropy on the Tc labelled rows; the head backward
 * contracts over those rows and a row-slot LayerNorm backward scatters d(hidden) to the B*L rows (zeros elsewhere).  The [B*L, V]
 * logits are not materialised: logits_out != NULL is refused (error 1).  Any other mode: error 1.  The backward of such a forward
 * works from the forward's census: it must be asked for the same batch split, and does not read `labels` again.  Every gradient
 * below lm_head equals the dense mode's; lm_head.weight / .bias differ in the grouping of their fp32 sums over rows; the losses in
 * the last bit at most.  No labelled row at all: NaN losses (0 / 0), zero head gradients, no zero-sized launch.  The mode is per
 * call, like showo_train_set_accumulate: reset it after the step, the module's autograd path shares the trainer. */
int showo_train_set_loss_rows(showo_trainer* t, int mode);
/* (rows the head of the last forward ran on, B*L of that forward); rows == total after a mode-0 forward.  No synchronisation. */
int showo_train_loss_rows(showo_trainer* t, int* rows, int* total);
/* launch counters since the last reset (tests): out6 = {weight-gradient GEMMs, data-gradient GEMMs, block phases that ran,
 * embedding-phase launches, transposed weight images rebuilt, fused block images rebuilt by the engine}; reset != 0 zeroes them */
int showo_train_counters(showo_trainer* t, int64_t* out6, int reset);
/* Training with visibility intervals built on the device (showo_mask_predict_next / showo_mask_mmu; reference
 * training/train.py:522-577 builds and concatenates dense [B,1,L,L] masks instead): the next showo_train_forward call with
 * mask == NULL uses iv int32 [B,L,4] for the forward and the backward; iv == NULL restores the causal default.
 * flag (optional int32[1], as written by showo_mask_predict_next): when non-zero the intervals cannot represent the mask
 * and the three losses of that forward are returned as NaN (device-side check, no host synchronisation). */
int showo_trainer_use_intervals(showo_trainer* t, const int32_t* iv, const int32_t* flag);

/* forward with saved activations.  ids int64 [B,L]; mask [B,1,L,L] fp32 or NULL (causal); labels int64 [B,L] or NULL.
 * logits_out (optional) fp32 [B,L,V]; losses_out (optional, needs labels) fp32 [3] = (loss_t2i, loss_lm, loss_mmu).
 * Masks must be interval-representable (at most two visibility runs per row: every mask the reference builds with
 * contiguous padding is); otherwise the three losses come back as NaN. */
int showo_train_forward(showo_trainer* t, const int64_t* ids, const float* mask, const int64_t* labels, int B, int L, int b_t2i,
                        int b_lm, int b_mmu, int max_seq_len, float* logits_out, float* losses_out, void* stream);
/* the same from caller-provided input embeddings fp32 [B,L,H] (reference modeling_showo.py:77-78 `inputs_embeds`; the w_clip_vit
 * training flow, training/train_w_clip_vit.py:530-613); after the backward, showo_train_input_grad returns
 * d(weighted loss)/d(embeds) fp32 [B*L*H] so that the caller's autograd graph (embed_tokens, mm_projector) can continue. */
int showo_train_forward_embeds(showo_trainer* t, const float* embeds, const float* mask, const int64_t* labels, int B, int L,
                               int b_t2i, int b_lm, int b_mmu, int max_seq_len, float* logits_out, float* losses_out, void* stream);
int showo_train_input_grad(showo_trainer* t, float* out, int64_t n, void* stream);
/* showo_train_forward with the projector's rows spliced into layer 0's input (showo_embed_splice_f32 is its first launch; layout
 * above): the native form of the w_clip_vit step.  ids and start are saved for the backward.  Works with the interval masks, the
 * announced loss weights, the loss-rows mode and the accumulate switch exactly as showo_train_forward does.  Backward: block 0
 * produces its data gradient when the embedding table trains or showo_train_set_input_grad is on (the projector trains -- also
 * with the table and every block frozen); showo_train_image_grad then returns the n*P placeholder rows of it, compacted in row
 * order (fp32 [n*P, H], n_elems = n*P*H), after showo_train_backward_layer(t, 0, ...); showo_train_backward_embed runs the
 * leave-out scatter (showo_embed_bwd_splice). */
int showo_train_forward_spliced(showo_trainer* t, const int64_t* ids, const float* rows, const int32_t* start, int n, int P,
                                const float* mask, const int64_t* labels, int B, int L, int b_t2i, int b_lm, int b_mmu,
                                int max_seq_len, float* logits_out, float* losses_out, void* stream);
int showo_train_image_grad(showo_trainer* t, float* out, int64_t n_elems, void* stream);
/* gradients of g_t2i*loss_t2i + g_lm*loss_lm + g_mmu*loss_mmu of the last forward w.r.t. every parameter */
int showo_train_backward(showo_trainer* t, const int64_t* labels, int b_t2i, int b_lm, int b_mmu, int max_seq_len, float g_t2i,
                         float g_lm, float g_mmu, void* stream);
/* the same backward in three phases (head -> blocks nL-1 .. 0 -> embedding): a data-parallel driver starts the gradient
 * exchange of a finished bucket while the next phase runs */
int showo_train_backward_head(showo_trainer* t, const int64_t* labels, int b_t2i, int b_lm, int b_mmu, int max_seq_len,
                              float g_t2i, float g_lm, float g_mmu, void* stream);
/* showo_train_backward_head with the three loss weights read from device memory g3 fp32 [3] = (g_t2i, g_lm, g_mmu) instead of host
 * scalars: the autograd path, where they are the incoming gradients of the three losses (training/train.py:600 builds the weighted
 * loss, :612 calls accelerator.backward on it) and the host never reads them.  Same as showo_train_backward_head without an announced
 * d(logits) (showo_train_set_loss_weights): its own cross-entropy pass, bit-identical d(logits) for equal weight values. */
int showo_train_backward_head_dev(showo_trainer* t, const int64_t* labels, int b_t2i, int b_lm, int b_mmu, int max_seq_len,
                                  const float* g3, void* stream);
int showo_train_backward_layer(showo_trainer* t, int layer, void* stream);
int showo_train_backward_embed(showo_trainer* t, void* stream);
/* Announce the loss weights (training/train.py:600: loss = w_t2i*loss_t2i + w_lm*loss_lm + w_mmu*loss_mmu) BEFORE the forward:
 * its cross-entropy pass then also writes d(loss)/d(logits), and a showo_train_backward[_head] call with the same labels
 * pointer (contents unchanged), batch split and weights skips its own pass over the [B*L, V] fp32 logits.  Any mismatch falls
 * back to the two-pass behaviour; enable = 0 turns the announcement off. */
int showo_train_set_loss_weights(showo_trainer* t, float w_t2i, float w_lm, float w_mmu, int enable);
/* all gradients live in one flat fp32 buffer; bucket 0 = embedding, 1 + i = block i, nL + 1 = head */
int showo_train_num_buckets(showo_trainer* t);
int showo_train_bucket(showo_trainer* t, int bucket, float** ptr, int64_t* n);
/* gradient buffer of a reference state-dict key (device pointer, element count) / copy of it */
int showo_train_grad(showo_trainer* t, const char* key, float** ptr, int64_t* n);
int showo_train_grad_copy(showo_trainer* t, const char* key, float* dst, int64_t n, void* stream);
int showo_train_losses(showo_trainer* t, float* out3, void* stream);
/* number of training forwards started on this trainer (showo_train_forward / _embeds): a host-driven backward checks that the
 * saved activations are still those of its own forward; -1 for a NULL handle */
int64_t showo_train_generation(showo_trainer* t);
/* optimizer (torch.optim.AdamW with the reference's two parameter groups, training/train.py:205-231): register the fp32
 * master tensor and the two moment buffers of a state-dict key once, then one call per step updates every trainable bound
 * parameter from the gradients of the last backward and refreshes its engine weight image; frozen ones are left untouched. */
int showo_train_bind_param(showo_trainer* t, const char* key, float* param, float* exp_avg, float* exp_avg_sq, int64_t n);
int showo_train_adamw_step(showo_trainer* t, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                           void* stream);
/* ---- EMA of the weights (reference models/training_utils.py:61-296 `EMA`; csrc/ema.hip) --------------------------------------
 * One step of a shadow value s against its parameter p is the reference's s.sub_(one_minus_decay * (s - p)): d = s - p,
 * t = one_minus_decay * d, s' = s - t, three fp32 operations each rounded on its own (never an fma).  one_minus_decay is the
 * Python float 1 - decay rounded to fp32, in [0, 1].
 *
 * Stand-alone table over `count` pairs of contiguous fp32 device tensors (shadow[k], param[k], n[k] elements; host arrays, read
 * and uploaded by create; pointers 4-byte aligned, 16-byte aligned ones move four elements per access).  dst_bf16 / dst_f32
 * (host arrays or NULL, entries NULL or at most one of the two set per pair): where swap also writes the bf16 cast / the fp32
 * copy of the value that goes into param[k].
 *   update  modes (host, count ints, NULL = all 0): 0 = the step above, 1 = shadow[k] = param[k] (the reference's branch for a
 *           parameter that does not require grad).  One launch.  The modes are kept on the device; a call with other modes than
 *           the one before waits for the stream and uploads them, and is refused inside a stream capture.
 *   swap    exchanges param[k] and shadow[k] in place, one launch, no third copy; twice restores every bit. */
typedef struct showo_ema_table showo_ema_table;
int showo_ema_table_create(float* const* shadow, float* const* param, const int64_t* n, int count, uint16_t* const* dst_bf16,
                           float* const* dst_f32, showo_ema_table** out);
void showo_ema_table_destroy(showo_ema_table* h);
int showo_ema_table_update(showo_ema_table* h, const int* modes, float one_minus_decay, void* stream);
int showo_ema_table_swap(showo_ema_table* h, void* stream);
/* On the trainer: showo_train_bind_ema registers the shadow of a key bound with showo_train_bind_param (NULL takes it away).
 * showo_train_set_ema announces one_minus_decay for the NEXT showo_train_adamw_step alone: that step updates the shadow of every
 * trainable parameter from the new master value inside the AdamW launch (every trainable parameter needs a shadow); negative = no
 * EMA, the step is the plain one.  With SHOWO_TRAIN_ADAMW_MULTI=0 the per-tensor AdamW is followed by one table update: same bits.
 * Frozen parameters are not touched by either.  showo_train_ema_swap exchanges every shadowed parameter, frozen ones included, with
 * its shadow and rewrites the engine's weight images from the values that go into the parameters (version stamps as after an
 * optimizer step).  The segment tables are rebuilt after a bind / trainable-set change, outside a stream capture only. */
int showo_train_bind_ema(showo_trainer* t, const char* key, float* shadow, int64_t n);
int showo_train_set_ema(showo_trainer* t, float one_minus_decay);
int showo_train_ema_swap(showo_trainer* t, void* stream);
/* torch.nn.utils.clip_grad_norm_ on a flat fp32 gradient buffer (reference training/train.py:614-615): g *= min(max_norm /
 * (||g||_2 + 1e-6), 1).  Fixed-order reduction (block partials in double, one block sums them in index order), the coefficient stays in
 * device memory: out2 (device, 2 floats) = {total norm, coefficient}; ws = showo_grad_clip_ws_doubles() doubles of scratch. */
int showo_grad_clip_norm(float* g, int64_t n, float max_norm, double* ws, float* out2, void* stream);
int showo_grad_clip_ws_doubles(void);
/* the same over TWO ranges with ONE global norm (the Show-o flat buffer and the projector's gradients: the reference clips
 * model.parameters(), training/train_w_clip_vit.py): partials of range 0 then range 1, summed in index order; both ranges are scaled
 * by the one coefficient.  ws = 2 * showo_grad_clip_ws_doubles() doubles.  n1 == 0 (g1 may be NULL) is showo_grad_clip_norm's norm. */
int showo_grad_clip_norm2(float* g0, int64_t n0, float* g1, int64_t n1, float max_norm, double* ws, float* out2, void* stream);
int showo_gelu_bf16(const uint16_t* f, uint16_t* a, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * CLIP ViT vision tower + mm_projector of the w_clip_vit understanding path.
 * Replaces transformers.CLIPVisionModel(images, output_hidden_states=True).hidden_states[-2][:, 1:] as called by
 * models/clip_encoder.py:29-49, and model.mm_projector (models/modeling_showo.py:48-53, inference_mmu.py:133-134).
 * run_layers = layers + 1 + select_layer (23 of 24 for select_layer = -2).
 * --------------------------------------------------------------------------------------------- */
typedef struct showo_clip showo_clip;
typedef struct {
    int image_size, patch_size, hidden, heads, ffn, layers, run_layers, max_batch;
    float ln_eps;
} showo_clip_config;
int showo_clip_create(const showo_clip_config* cfg, showo_clip** out);
void showo_clip_destroy(showo_clip* c);
/* one tensor by its transformers state-dict key ("vision_model.embeddings.patch_embedding.weight", ..., optionally prefixed
 * "vision_tower." as in the reference wrapper's state dict, with or without the "vision_model." level); src = device fp32 */
int showo_clip_load(showo_clip* c, const char* key, const float* src, int64_t n, void* stream);
int showo_clip_missing(const showo_clip* c);
/* images fp32 [B,3,S,S] (normalised) -> features fp32 [B, (S/patch)^2, hidden] */
int showo_clip_features(showo_clip* c, const float* images, int B, float* features, void* stream);
/* 0 (default): bf16 GEMM / attention operands.  1: accuracy mode -- every GEMM on the split-bf16 MFMA kernel (hi + lo operand pairs),
 * LayerNorm / attention / quick_gelu in fp32: the fp32 tower of transformers' CLIPVisionModel (models/clip_encoder.py:29-49 runs it in
 * the model's dtype) to ~1e-4.  The low halves of the weights are kept from every showo_clip_load; the fp32 workspace is allocated
 * by the first call with precision 1. */
int showo_clip_set_precision(showo_clip* c, int precision);
int showo_clip_get_precision(const showo_clip* c);
/* 1 when every GEMM weight of the tower has a current low half: they are allocated by the FIRST showo_clip_set_precision(c, 1) (a
 * precision-0 user never pays the 0.6 GB), so weights loaded before that call must be uploaded again. */
int showo_clip_precise_ready(const showo_clip* c);
/* mm_projector: Linear(in,out) -> exact GELU -> Linear(out,out).  Keys "0.weight", "0.bias", "2.weight", "2.bias" (optionally
 * prefixed "mm_projector."); x fp32 [T,in] -> out fp32 [T,out], T <= max_rows. */
typedef struct showo_projector showo_projector;
int showo_projector_create(int in_dim, int out_dim, int max_rows, showo_projector** out);
void showo_projector_destroy(showo_projector* p);
int showo_projector_load(showo_projector* p, const char* key, const float* src, int64_t n, void* stream);
int showo_projector_forward(showo_projector* p, const float* x, int T, float* out, void* stream);
/* 0: bf16 operands (default, also what showo_projector_backward differentiates); 1: split-bf16 GEMMs + fp32 exact GELU (inference) */
int showo_projector_set_precision(showo_projector* p, int precision);
int showo_projector_precise_ready(const showo_projector* p);  /* as showo_clip_precise_ready */
/* backward of the LAST showo_projector_forward (same T rows): dout fp32 [T,out] -> gw0 fp32 [out,in], gb0 [out], gw1 [out,out],
 * gb1 [out], dx fp32 [T,in] (optional).  Autograd of nn.Sequential(Linear, GELU(), Linear) (training/train_w_clip_vit.py trains it). */
int showo_projector_backward(showo_projector* p, const float* dout, int T, float* dx, float* gw0, float* gb0, float* gw1, float* gb1,
                             void* stream);
/* accumulating form (gradient accumulation over micro-batches, the contract of showo_train_set_accumulate): accumulate != 0 adds the
 * finished sums into gw0 / gb0 / gw1 / gb1 (one fp32 rounding per added micro-batch); accumulate == 0 is showo_projector_backward.
 * Any of the four may be NULL (a frozen tensor): its gradient is neither computed nor written. */
int showo_projector_backward_acc(showo_projector* p, const float* dout, int T, float* dx, float* gw0, float* gb0, float* gw1,
                                 float* gb1, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Image pre / post-processing on the device.
 * showo_image_resize_crop_normalize = training/utils.py:178-185 image_transform (torchvision Resize(bicubic) on a PIL image ->
 * CenterCrop -> ToTensor -> Normalize(0.5, 0.5)): PIL's antialiased bicubic with its 22-bit fixed-point coefficient tables
 * (computed by the host exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do), uint8 between the two passes;
 * byte-exact with PIL.  img u8 [H,W,C] (C = 1 or 3) -> out fp32 [C,crop_h,crop_w]; bounds int32 [n,2] = (first tap, tap count),
 * kk int32 [n,ksize]; tmp: >= H*Wout*C bytes; out_u8 (optional) u8 [crop_h,crop_w,C] = the resized + cropped bytes.
 * showo_images_to_uint8 = inference_t2i.py:157-159 (clamp((x+1)/2,0,1)*255, truncated, NCHW -> NHWC).
 * showo_mask_downsample_threshold = inference_t2i.py:100-108 (F.interpolate(mode='bicubic') to s_out x s_out, >= 0.5).
 * --------------------------------------------------------------------------------------------- */
int showo_image_resize_crop_normalize(const uint8_t* img, int H, int W, int C, int Hout, int Wout, const int32_t* bounds_h,
                                      const int32_t* kk_h, int ksize_h, const int32_t* bounds_v, const int32_t* kk_v, int ksize_v,
                                      int ct, int cl, int crop_h, int crop_w, int normalize, uint8_t* tmp, float* out, uint8_t* out_u8,
                                      void* stream);
int showo_images_to_uint8(const float* x, uint8_t* out, int B, int C, int H, int W, void* stream);
int showo_mask_downsample_threshold(const float* mask, int S, int s_out, uint8_t* out, float* values, void* stream);

#ifdef __cplusplus
}
#endif
#endif
