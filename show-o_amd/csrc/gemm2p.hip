#include "gemm2p_kernel.h"
#include "prof.h"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>

namespace showo {

// =====================================================================================================
// Production GEMM: 2-phase, phase-split kernel with a selectable tile HEIGHT.  Tile = 16 (MF0 + MF1) rows x 256 columns x 64 (k);
// 8 waves = 4 along n x 2 groups along m; group g owns MFg 16-row m-fragments; wave tile 64 (n) x 16 MFg (m) as 4 x MFg
// v_mfma_f32_16x16x32_bf16 fragments (weight tile = MFMA A operand: a lane owns 4 consecutive output columns).
// Operands go HBM -> LDS by global_load_lds (16 B / lane, source-side XOR swizzle, conflict-free ds_read_b128), double-buffered
// with counted vmcnt (the DMA queue is never drained in the loop) and raw s_barrier; the two wave groups run the phase program
// ONE BARRIER APART so that each SIMD alternates one wave's MFMA segment with the other wave's LDS-read / DMA-issue segment.
//
// A launch is rounds x tile-time long, rounds = ceil(tiles / 256 CUs), so the height is chosen per shape (see the tuner).
// Two phase programs (a k-tile is 2 phases; a phase = [ds_read + DMA issue + vmcnt] barrier [MFMAs] barrier):
//   NS = false, "m-split" (13..16 fragments):  ph0 = all 4 W fragments x the group's first 4 A fragments (32 MFMAs per wave),
//       ph1 = W x the remaining MFg - 4 fragments.  DMA: ph0 W (4 pieces / wave) + A-lo (2), ph1 A-hi (2).
//   NS = true,  "n-split" (8..12 fragments):   ph0 = W fragments 0,1 x ALL MFg A fragments, ph1 = W fragments 2,3 x all A fragments
//       (2 MFg MFMAs per k-step in both phases: balanced for short tiles, where the m-split leaves ph1 nearly empty and its length
//       is set by the other group's load segment).  DMA: ph0 W rows of fragments 0,1 (2 pieces / wave) + all of A (NPW), ph1 W rows
//       of fragments 2,3 (2).
// Hazards (both programs; group 1 runs one barrier behind group 0):
//   RAW: a DMA is waited for (counted vmcnt, by the issuing wave) in the load segment of the phase AFTER the one that issued it and
//        its data is read one phase after that wait, i.e. two barriers after every wave's wait.
//   WAR: a region is re-staged two phases after the phase whose load segment read it last (its reads retire at the head of that
//        phase's MFMA segment, at least two barriers before the DMA issue of any wave).
// K-concatenated A operand (GemmArgs::A2) and the fused [Wqkv ; W1] epilogue (GemmArgs::Nq): see gemm_common.h.
// =====================================================================================================
// (the kernel template and its launchers: gemm2p_kernel.h; this file = host state, split-K policy, the tile tuner, the bf16 instances)

// ---- split-K workspace: one per stream that asks for it (at most 4), allocated on first use outside a stream capture.
// 96 MiB covers tiles x splits <= 256 blocks of the tallest tile (256 x 256 fp32 = 256 KiB per block).
namespace {
struct SplitWs { hipStream_t s; float4* ws; unsigned* tick; };
SplitWs g_sws[8];
int g_nsws = 0;
constexpr size_t SPLITK_WS_BYTES = (size_t)96 << 20;
}  // namespace

bool splitk_ws(hipStream_t s, size_t need, float4** ws, unsigned** tick) {
    if (need > SPLITK_WS_BYTES) return false;
    for (int i = 0; i < g_nsws; ++i)
        if (g_sws[i].s == s) { *ws = g_sws[i].ws; *tick = g_sws[i].tick; return true; }
    if (g_nsws == 8) return false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return false;  // never allocate inside a capture
    SplitWs w{s, nullptr, nullptr};
    if (hipMalloc(&w.ws, SPLITK_WS_BYTES) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (hipMalloc(&w.tick, SPLITK_TICKS * sizeof(unsigned)) != hipSuccess || hipMemset(w.tick, 0, SPLITK_TICKS * sizeof(unsigned)) != hipSuccess) {
        (void)hipGetLastError();
        hipFree(w.ws);
        return false;
    }
    g_sws[g_nsws++] = w;
    *ws = w.ws; *tick = w.tick;
    return true;
}

// ---- split-K policy.  Few tiles, long K: split until ~one block per CU, >= 16 k-tiles per split.  The exchange costs a tile-sized fp32
// write per split, one L2 write-back + ticket per block and `splits` tile reads in the last block.  Measured
// (profiles/r2_gemm_harness.txt, r3c / r3d): M = 631, K = 10 240 residual GEMM 168 -> 70 us; CLIP fc2 (K = 4 096) 65 -> 37-40 us; cfg4
// prefill 6.3 -> 4.5 ms, CLIP tower 5.8 -> 4.9 ms, time to first token 12.1 -> 9.5 ms.  Splits of 8 k-tiles measured within noise of
// none -> floor 16 (SHOWO_GEMM_SPLITK_MIN).
// The count is derived from the PROBLEM (tile count of the tallest, 256-row, tile), never from the tile variant that runs it: the
// k-partition -- and with it the fp32 summation order of every output element -- is then the same for every variant, so the
// wall-clock race of the tuner cannot change results between processes, ranks or runs (with the count taken from the
// variant's own tile count, M = 631 gave S = 10 at 256 rows and S = 6 at 144).  The ring variants (gemm3w) do not split; they are
// kept out of the candidate list of split shapes (launch2p_bm) for the same reason.
int64_t g_cnt_gemm2p = 0, g_cnt_qkv_save = 0, g_cnt_splitk = 0;
// cooperative split-K reduction (gemm_common.h splitk_coop_finish): every block of the launch must be resident at once -- one 512-thread
// block with 128+ KiB of LDS per CU -- on the CUs that no masked stream of this process keeps free (showo_stream_create_cu_mask).
// SHOWO_GEMM_COOP=0 restores the last-arriver reduction (A/B runs).
int splitk_coop_mode() {  // SHOWO_GEMM_COOP: 2 (default) = write-through (sc1) partial stores, no fence; 1 = plain stores + release fence
    static int m = -1;        // (r4g, one box: dense|fc2 at M = 631 72 -> 61 us, batch-1 t2i 66.0 -> 63.2 ms per image; same bits)
    if (m < 0) { const char* e = getenv("SHOWO_GEMM_COOP"); m = e ? atoi(e) : 2; }
    return m == 1 ? 1 : 2;
}
// Residency: blocks are dealt to the 8 XCDs round-robin, so the test is per XCD -- ceil(blocks / 8) blocks on the usable(stream) / 8 CUs
// of one XCD (a global count admits launches whose XCD share does not fit under an uneven mask).
// Ownership: the spin-wait of splitk_coop_finish is only safe when NOTHING else can take CUs away from a half-resident launch.  Two
// cooperative launches on different streams could each be partly resident and wait for each other until the trap, so ONE
// stream at a time owns the cooperative form: the first stream that asks; another stream takes over only when the owner's last
// cooperative launch has completed (event), and a stream that CAPTURED cooperative launches into a hipGraph keeps the ownership (the
// graph may replay at any time).  Everybody else gets the last-arriver reduction: the same bits, no waiting.  Work of ANOTHER PROCESS
// on the same GPU is outside this gate, but no longer a hazard: a block whose siblings do not show up falls back to the last-arriver
// form after coop_polls polls (gemm_common.h splitk_coop_finish).
namespace {
struct CoopOwner { hipStream_t s = nullptr; hipEvent_t ev = nullptr; bool sticky = false, used = false; };
CoopOwner g_coop_owner;
}  // namespace
bool splitk_coop_ok(int blocks, hipStream_t s) {  // caller holds g_gemm_mu
    static int on = -1;
    if (on < 0) {
        const char* e = getenv("SHOWO_GEMM_COOP");
        on = e ? atoi(e) : 1;
    }
    if (!on || (blocks + 7) / 8 > showo_cu_usable((void*)s) / 8) return false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
    CoopOwner& o = g_coop_owner;
    if (o.used && o.s != s) {
        if (o.sticky) return false;
        if (o.ev && hipEventQuery(o.ev) != hipSuccess) { (void)hipGetLastError(); return false; }  // the owner's cooperative work is still in flight
    }
    if (!o.ev && !capturing && hipEventCreateWithFlags(&o.ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; }
    o.s = s; o.used = true;
    if (capturing) o.sticky = true;
    return true;
}
void splitk_coop_launched(hipStream_t s) {  // after a cooperative launch outside a capture: marks the end of the owner's cooperative work
    CoopOwner& o = g_coop_owner;
    if (o.sticky || !o.ev) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) (void)hipEventRecord(o.ev, s);
}
// split count for a launch that may use `cus` CUs (showo_cu_usable(stream): 256 on a plain stream).  A function of the problem and of
// that number alone -- never of the tile variant -- so every variant produces the same bits under a given CU budget.
int splitk_count(int M, int N, int K, int cus) {
    if (g_gemm_splitk < 0) { const char* e = getenv("SHOWO_GEMM_SPLITK"); g_gemm_splitk = e ? atoi(e) : 1; }
    static int min_kt = 0;  // k-tiles per split at least (SHOWO_GEMM_SPLITK_MIN, default 16)
    if (!min_kt) { const char* e = getenv("SHOWO_GEMM_SPLITK_MIN"); min_kt = (e && atoi(e) >= 2) ? atoi(e) : 16; }
    const int tiles = ((M + 255) / 256) * ((N + B2 - 1) / B2), nk = K / GEMM_BK;
    if (!g_gemm_splitk || tiles * 2 > cus || nk < 2 * min_kt) return 1;
    int S = cus / tiles;
    if (S > nk / min_kt) S = nk / min_kt;
    if (S > 16) S = 16;
    if (S < 2) return 1;
    const int per = (nk + S - 1) / S;
    S = (nk + per - 1) / per;  // no empty split
    return S >= 2 ? S : 1;
}

// Tile variants: code = rows (+ 1000 for the n-split phase program).
//   m-split: 256 (8+8), 240 (8+7), 224 (7+7), 208 (7+6), 176 (6+5), 160 (5+5), 144 (5+4)
//   n-split: 1192 (6+6), 1176 (6+5), 1160 (5+5), 1144 (5+4), 1128 (4+4)
//   m-split with a 3-deep weight ring (gemm3w.hip): 2256 (8+8), 2240 (8+7), 2224 (7+7), 2208 (7+6)
//   n-split on the ring: 3192 (6+6), 3176 (6+5), 3160 (5+5), 3144 (5+4)
//   the same with buffer-descriptor DMAs: 4192, 4176, 4160, 4144
//   (5256, the four-wave 128 x 128-wave-tile kernel of round 4, lives in tools/experiments/gemm4h.hip: a measured negative, not shipped)
namespace {
constexpr int N_VARIANTS = 24;
const int k_variants[N_VARIANTS] = {256, 240, 224, 208, 176, 160, 144, 1192, 1176, 1160, 1144, 1128, 2256, 2240, 2224, 2208, 3192, 3176, 3160, 3144,
                                    4192, 4176, 4160, 4144};
bool is_variant(int v) {
    for (int i = 0; i < N_VARIANTS; ++i)
        if (k_variants[i] == v) return true;
    return false;
}
}  // namespace

// the bfloat16 instances of every (epilogue, tile variant); the IEEE-half ones are in gemm2p_f16.hip
int gemm2p_variant_bf16(const GemmArgs& g, int epilogue, int h, hipStream_t s) {
    switch (epilogue) {
        case SHOWO_EPI_BF16: return g2p::launch2p_h<SHOWO_EPI_BF16, false>(g, h, s);
        case SHOWO_EPI_GELU_BF16: return g2p::launch2p_h<SHOWO_EPI_GELU_BF16, false>(g, h, s);
        case SHOWO_EPI_F32: return g2p::launch2p_h<SHOWO_EPI_F32, false>(g, h, s);
        case SHOWO_EPI_RESID_F32: return g2p::launch2p_h<SHOWO_EPI_RESID_F32, false>(g, h, s);
        case EPI_QKV: return g2p::launch2p_h<EPI_QKV, false>(g, h, s);
        case EPI_QKV_SPLIT: return g2p::launch2p_h<EPI_QKV_SPLIT, false>(g, h, s);
    }
    return set_error_msg(1, "gemm: unknown epilogue");
}

int g_gemm_coop_polls = 1 << 15;  // showo_gemm_set_coop_polls
int g_gemm_gn = 4;  // n-panels per XCD tile group (same-process sweep on the bench workload: 8 -> 24.6-24.7, 4 -> 25.1, 2 -> 25.1, 1 -> 24.7, 16 -> 24.5 images/s)
int g_gemm_bm = 0;  // 0 = read SHOWO_GEMM_BM once; -1 = choose per shape; a variant code = force it
int g_gemm_splitk = -1;  // SHOWO_GEMM_SPLITK: 0 = off, 1 (default) = launches with <= 128 tiles split K until ~256 blocks exist
int g_gemm_stage = -1;  // bf16 epilogue stores staged through LDS: -1 = read SHOWO_GEMM_STAGE once (default on), 0 / 1 = forced
int g_gemm_wide = -1;   // Q / K / V^T stores of the projection epilogue: 0 = the narrow form (8-byte Q / K, 2-byte V^T: A/B runs, tests), else 16-byte (showo_gemm_set_wide_stores)
int g_gemm_resid_batch = -1;  // residual epilogue of full wave tiles: -1 = read SHOWO_GEMM_RESID_BATCH once (default on), 0 = one load / add / store per fragment (A/B runs, tests), else the residual loads of a fragment group back to back (showo_gemm_set_resid_batch)
int g_gemm_pf = -1; // L2 prefetch of the weight panel: -1 = read SHOWO_GEMM_PF once (default OFF: measured -3...-8 % in the harness
                    // with cold weights and within noise in the pipeline, profiles/r2_gemm_harness.txt), 0 / 1 = forced (showo_gemm_tune)

namespace {

// model used when a shape cannot be timed (stream capture, SHOWO_GEMM_TUNE=0, small problems): rounds x (rows + fixed cost),
// rounds = ceil(tiles / CUs); short tiles use the n-split program
int pick_bm(int M, int N, int cus) {
    if (g_gemm_bm == 0) {  // SHOWO_GEMM_BM=<variant code> forces a tile (A/B runs of bench.py)
        const char* e = getenv("SHOWO_GEMM_BM");
        g_gemm_bm = e ? atoi(e) : -1;
    }
    if (is_variant(g_gemm_bm)) return g_gemm_bm;
    const int tilesN = (N + B2 - 1) / B2;
    const int cand[8] = {256, 240, 224, 208, 1192, 1176, 1160, 1144};  // (the ring variants are only chosen by measurement)
    long best_cost = -1;
    int best = 256;
    for (int c : cand) {
        const int rows = c % 1000;
        const long tiles = (long)((M + rows - 1) / rows) * tilesN;
        const long cost = ((tiles + cus - 1) / cus) * (rows + 24);  // + ~1.5 fragments of prologue / epilogue per tile
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = c; }
    }
    return best;
}

// Tile variant per (M, N, K, epilogue).  The rounds model mispredicts by up to ~10 % (per-tile weight streaming, epilogue traffic,
// DVFS), so the first launch of a shape times every candidate (interleaved passes, HIP events) and the winner is cached.  Every
// CANDIDATE of a shape computes bit-identical results: an output element is one fp32 chain over k in order, or -- for shapes that
// split K -- `splitk_count(M, N, K)` chains over a k-partition that depends on the problem only, summed in split order; the ring
// variants, which never split, are not candidates of a split shape.  So the timing race never changes numerics.  Skipped while the
// stream is being captured (the model is used), and with SHOWO_GEMM_TUNE=0.  In-place residual launches are timed on a scratch output.
// g_bm_cache / the split-K workspaces are process-wide: guarded by g_gemm_mu (autograd's backward thread launches GEMMs too).
std::mutex g_gemm_mu;

std::map<std::tuple<int, int, int, int, int>, int> g_bm_cache;  // (M, N, K, EPI, split-policy M) -> variant | tile-group width << 16
thread_local int t_split_m_pin = 0;  // gemm_pin_split_m
int g_gemm_tune = -1;

// one tile variant of (epilogue, operand type) by run-time codes
int launch_variant(const GemmArgs& g, int EPI, int h, hipStream_t s) {
    return g.op ? gemm2p_variant_f16(g, EPI, h, s) : gemm2p_variant_bf16(g, EPI, h, s);
}

int launch2p_bm(const GemmArgs& g, int EPI, hipStream_t s) {
    const bool F16 = g.op != 0;
    const int cus = showo_cu_usable((void*)s);
    if (g_gemm_bm == 0) pick_bm(g.M, g.N, cus);  // reads SHOWO_GEMM_BM
    if (g_gemm_bm > 0) return launch_variant(g, EPI, g_gemm_bm, s);
    if (g_gemm_tune < 0) { const char* e = getenv("SHOWO_GEMM_TUNE"); g_gemm_tune = e ? atoi(e) : 1; }
    const auto key = std::make_tuple(g.M, g.N, g.K, EPI | (F16 ? 0x80 : 0) | (cus << 8), g.split_m);  // the CU budget of the stream is part of the shape: other split counts, other rounds
    const bool split_shape = splitk_count(g.split_m ? g.split_m : g.M, g.N, g.K, cus) >= 2;  // ring variants never split: not candidates (bit-identity, see above)
    auto it = g_bm_cache.find(key);
    if (it != g_bm_cache.end()) {
        GemmArgs c = g;
        if (it->second >> 16) c.gn = it->second >> 16;
        return launch_variant(c, EPI, it->second & 0xffff, s);
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
    if (!g_gemm_tune || capturing || (int64_t)g.M * g.N < ((int64_t)1 << 20)) return launch_variant(g, EPI, pick_bm(g.M, g.N, cus), s);
    GemmArgs t = g;
    void* scratch = nullptr;
    if (EPI == SHOWO_EPI_RESID_F32) {  // accumulates in place: time it on a scratch output
        if (hipMalloc(&scratch, (size_t)g.M * g.ldo * sizeof(float)) != hipSuccess) return launch_variant(g, EPI, pick_bm(g.M, g.N, cus), s);
        t.out = scratch; t.resid = (const float*)scratch; t.ldr = g.ldo;
    }
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    int best = pick_bm(g.M, g.N, cus);
    float best_ms = 1e30f;
    // interleaved passes over the candidates, 3 timed launches each, minimum per candidate: the first measurements of a process
    // run on a GPU that is still ramping its clocks, and a single sample mis-ranks tiles that differ by ~10 %
    float cand_ms[N_VARIANTS];
    for (int ci = 0; ci < N_VARIANTS; ++ci) cand_ms[ci] = 1e30f;
    static int ring_ok = -1;  // SHOWO_GEMM_RING=0 keeps the 3-deep-ring variants (gemm3w.hip) out of the tuner (A/B runs)
    if (ring_ok < 0) { const char* e = getenv("SHOWO_GEMM_RING"); ring_ok = e ? (atoi(e) != 0) : 1; }
    for (int pass = 0; pass < 2; ++pass) {
        for (int ci = 0; ci < N_VARIANTS; ++ci) {
            const int h = k_variants[ci];
            if (h >= 2000 && (!ring_ok || split_shape)) continue;
            int rc = launch_variant(t, EPI, h, s);  // warm-up (instruction cache, attribute set)
            (void)hipEventRecord(e0, s);
            for (int rep = 0; rep < 3 && !rc; ++rep) rc = launch_variant(t, EPI, h, s);
            (void)hipEventRecord(e1, s);
            if (rc || hipEventSynchronize(e1) != hipSuccess) continue;
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms < cand_ms[ci]) cand_ms[ci] = ms;
        }
    }
    for (int ci = 0; ci < N_VARIANTS; ++ci)
        if (cand_ms[ci] < best_ms) { best_ms = cand_ms[ci]; best = k_variants[ci]; }
    // second dimension, at the chosen height: n-panels per XCD tile group (L2 / Infinity-Cache locality of the co-resident tiles).
    // Measured on the bench workload the better of {4, 8} differs from box to box (+1.7 % / -0.6 %), hence per shape, per process.
    int best_gn = g.gn;
    {
        const int gns[2] = {4, 8};
        float gn_ms[2] = {1e30f, 1e30f};
        for (int pass = 0; pass < 2; ++pass) {
            for (int gi = 0; gi < 2; ++gi) {
                t.gn = gns[gi];
                int rc = launch_variant(t, EPI, best, s);
                (void)hipEventRecord(e0, s);
                for (int rep = 0; rep < 3 && !rc; ++rep) rc = launch_variant(t, EPI, best, s);
                (void)hipEventRecord(e1, s);
                if (rc || hipEventSynchronize(e1) != hipSuccess) continue;
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms < gn_ms[gi]) gn_ms[gi] = ms;
            }
        }
        if (gn_ms[0] < 1e29f || gn_ms[1] < 1e29f) best_gn = gn_ms[0] <= gn_ms[1] ? gns[0] : gns[1];
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (scratch) (void)hipFree(scratch);
    g_bm_cache[key] = best | (best_gn << 16);
    if (const char* tl = getenv("SHOWO_GEMM_TUNE_LOG")) {
        fprintf(stderr, "[gemm2p tune] M=%d N=%d K=%d epi=%d%s -> variant %d gn %d (%.1f us)\n", g.M, g.N, g.K, EPI, F16 ? " f16" : "", best, best_gn, best_ms * 1000.f / 3.f);
        if (atoi(tl) >= 2) {  // every candidate
            fprintf(stderr, "[gemm2p tune]   ");
            for (int ci = 0; ci < N_VARIANTS; ++ci)
                if (cand_ms[ci] < 1e29f) fprintf(stderr, " %d:%.1f", k_variants[ci], cand_ms[ci] * 1000.f / 3.f);
            fprintf(stderr, "\n");
        }
    }
    GemmArgs c = g;
    c.gn = best_gn;
    return launch_variant(c, EPI, best, s);
}

}  // namespace

// split-K policy / workspace / launch counters shared with gemm_tn.hip (the caller holds no lock; the workspace table is guarded here)
int gemm_splitk_count(int M, int N, int K, int cus) { return splitk_count(M, N, K, cus); }
bool gemm_splitk_ws(hipStream_t s, size_t need, float4** ws, unsigned** tick) {
    std::lock_guard<std::mutex> lock(g_gemm_mu);
    return splitk_ws(s, need, ws, tick);
}
int gemm_splitk_ticks() { return SPLITK_TICKS; }
void gemm_count_launch(bool split) {
    std::lock_guard<std::mutex> lock(g_gemm_mu);
    g_cnt_gemm2p++;
    if (split) g_cnt_splitk++;
}

void gemm_pin_split_m(int M) { t_split_m_pin = M > 0 ? M : 0; }

int gemm2p_dispatch(GemmArgs g, int epilogue, hipStream_t s) {
    std::lock_guard<std::mutex> lock(g_gemm_mu);
    g.split_m = (t_split_m_pin && t_split_m_pin != g.M) ? t_split_m_pin : 0;
    g_cnt_gemm2p++;
    if (epilogue == EPI_QKV && g.raw && g.pre) g_cnt_qkv_save++;
    g.gn = g_gemm_gn > 0 ? g_gemm_gn : 1;
    if (g_gemm_pf < 0) { const char* e = getenv("SHOWO_GEMM_PF"); g_gemm_pf = e ? (atoi(e) != 0) : 0; }
    if (g_gemm_stage < 0) {  // SHOWO_GEMM_STAGE: 0 direct stores, 1 (default) staged except Q / K, 2 all, 3 = 1 with V^T direct, 4 = 1 with the narrow Q / K / V^T stores
        const char* e = getenv("SHOWO_GEMM_STAGE");
        g_gemm_stage = e ? atoi(e) : 1;
        if (g_gemm_stage == 4) { g_gemm_stage = 1; if (g_gemm_wide < 0) g_gemm_wide = 0; }
    }
    g.flags = (g_gemm_pf ? 2 : 0) | (g_gemm_stage ? 0 : 8) | (g_gemm_stage == 2 ? 32 : 0) | (g_gemm_stage == 3 ? 64 : 0);
    if (epilogue == EPI_QKV && g_gemm_wide != 0) {
        // 16-byte Q / K / V^T stores of the projection epilogue (qkv_head_rows): every row of Q and K is 128 bytes and Lp is a multiple
        // of 64, so the base addresses decide.  Bit 8: the same for the raw rows of the save form.
        auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
        if (g.Q && al16(g.Q) && al16(g.Kd) && al16(g.Vt) && (g.Lp % 8) == 0) g.flags |= 128;
        if (g.Q && g.raw && al16(g.raw) && (g.ldraw % 8) == 0) g.flags |= 256;
    }
    if (g_gemm_resid_batch < 0) { const char* e = getenv("SHOWO_GEMM_RESID_BATCH"); g_gemm_resid_batch = e ? (atoi(e) != 0) : 1; }
    // batched residual loads (gemm_common.h resid_tile_batched): vec_out already says that out, resid and both leading dimensions allow
    // 16-byte access; the kernel adds the per-tile condition (the wave tile inside M and N)
    if (epilogue == SHOWO_EPI_RESID_F32 && g_gemm_resid_batch && g.vec_out && !g.bias_per_row && g.resid) g.flags |= 512;
    g.dbg = nullptr;
    g.coop_polls = g_gemm_coop_polls;
    if (g.op && epilogue == EPI_QKV && (g.raw || g.pre)) return set_error_msg(1, "gemm: the save-for-backward projection has bf16 operands only");
    if (g.op && epilogue == EPI_QKV_SPLIT) return set_error_msg(1, "gemm: the (hi, lo) projection epilogue has bf16 operands only");
    if (epilogue >= 0 && epilogue <= EPI_QKV_SPLIT) return launch2p_bm(g, epilogue, s);
    return set_error_msg(1, "gemm: unknown epilogue");
}

}  // namespace showo

// Launch counters of the production GEMM family (tests assert that a batch took the T >= 256 branch the bench times):
// out[0] = launches through gemm2p_dispatch (gemm2p / gemm3w kernels), out[1] = of those, the fused [Wqkv ; W1] save-for-backward form
// (showo_gemm_qkv_fc1_save_bf16), out[2] = launches that split K.  reset != 0 zeroes them after reading.
// test hook of the cooperative split-K reduction: polls before a waiting block switches its tile to the last-arriver sum
// (default 32 768, ~2 ms; 0 = every block that is not the last to arrive gives up at once).  Results never depend on it.
extern "C" int showo_gemm_set_coop_polls(int polls) {
    std::lock_guard<std::mutex> lock(showo::g_gemm_mu);
    showo::g_gemm_coop_polls = polls < 0 ? (1 << 15) : polls;
    return 0;
}

// A/B lever and test reference of the projection epilogue's store forms: 0 = the narrow stores (8-byte Q / K pieces, 2-byte V^T), 1 = the
// 16-byte stores, < 0 = the default (16-byte).  Both forms write the same bytes to the same addresses.
extern "C" int showo_gemm_set_wide_stores(int on) {
    std::lock_guard<std::mutex> lock(showo::g_gemm_mu);
    showo::g_gemm_wide = on < 0 ? 1 : (on != 0);
    return 0;
}

// A/B lever and test reference of the residual epilogue: 0 = one residual load, add and store per fragment, 1 = the loads of a fragment
// group issued back to back (full wave tiles of 16-byte aligned launches only), < 0 = the default (1).  Same additions on the same
// values either way.
extern "C" int showo_gemm_set_resid_batch(int on) {
    std::lock_guard<std::mutex> lock(showo::g_gemm_mu);
    showo::g_gemm_resid_batch = on < 0 ? 1 : (on != 0);
    return 0;
}

extern "C" int showo_gemm_counters(int64_t* out3, int reset) {
    std::lock_guard<std::mutex> lock(showo::g_gemm_mu);
    if (out3) { out3[0] = showo::g_cnt_gemm2p; out3[1] = showo::g_cnt_qkv_save; out3[2] = showo::g_cnt_splitk; }
    if (reset) showo::g_cnt_gemm2p = showo::g_cnt_qkv_save = showo::g_cnt_splitk = 0;
    return 0;
}
