"""Precision 2 (IEEE-half operands, `Showo.set_precision(2)`) at its range limits and across precision switches, on the GPU.

test_fp16_gpu.py holds the fp16 instances to the oracle on benign inputs (N(0, 0.02) weights, unit-scale activations).  This file
covers what those inputs never reach:
  A. kernel edges of the `_op16` entry points: GEMM epilogue outputs at and beyond 65504 (clamp, then round to nearest even, bit for
     bit), a NaN that must stay a NaN through every fp16 store, the attention output when V sits at +-65504 and P rounds up,
     subnormal operands, and the saturation counter;
  B. a heavy-tailed tiny model (oracle/weights.py profile "heavy": outlier channels, LayerNorm gains >> 1, a peaked lm_head) whose
     LayerNorm outputs saturate in fp16: parity of every precision with its own oracle, the range check, NaN propagation;
  C. the engine's state contract: every ordered precision switch, the range check around a graph-replayed t2i_generate, and the
     batched decode after a batch that left NaN in its caches.
Every expected value is computed on the CPU from the same 16-bit-rounded operands (float64 for the kernel tests, the rounding-point
oracle of oracle/showo_oracle.py for the model tests)."""
import numpy as np
import pytest
import torch

import util
from util import O, Wt, dev
from test_fp16_gpu import F16, FP16_TOL, _attn_oracle16, _prep16, f16r, from_h16, h16

pytestmark = pytest.mark.gpu

F16_MAX = 65504.0


def L():
    return util.lib()


def S():
    return util.lib().stream()


def sat_rne(v):
    """fp32 -> fp16 the way the kernels convert: clamp to +-65504 (NaN stays NaN), then round to nearest even"""
    return v.float().clamp(-F16_MAX, F16_MAX).to(torch.float16)


def assert_f16_equal(got, want, what):
    """bit-equal fp16 tensors, except that any NaN matches any NaN"""
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), (what, "NaN positions", int(gn.sum()), int(wn.sum()))
    g, w = got[~gn].view(torch.int16), want[~wn].view(torch.int16)
    bad = (g != w).nonzero()
    assert bad.numel() == 0, (what, bad[:5].flatten().tolist(), got[~gn][bad[:5, 0]].tolist(), want[~wn][bad[:5, 0]].tolist())


# ------------------------------------------------------------------------------------------------------ A. kernel edges
_A_VALS = [F16_MAX, -F16_MAX, 32752.0, 1.0]                    # column 0 of A (fp16-exact)
_W_VALS = [1.0, -1.0, 2.0, 0.5]                                # column 0 of W (fp16-exact)
_BIAS = [0.0, 6.0, 15.99, 16.0, 17.0, 1e6, float("inf"), float("-inf"), -6.0, -16.0, 3e38, 1.5]


def _edge_operands(M, N, K, seed):
    """out[m, n] = A[m, 0] * W[n, 0] + bias[n] exactly in fp32: the product of two fp16 values is exact in fp32, and every other column
    of W is zero (A's other columns are random, so the kernel still walks all of K).  The targets land exactly on 65504, in
    (65504, 65520), at >= 65520 (where RNE alone would give inf) and at +-inf in fp32."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g)
    A[:, 0] = torch.tensor(_A_VALS)[torch.arange(M) % len(_A_VALS)]
    W = torch.zeros(N, K)
    W[:, 0] = torch.tensor(_W_VALS)[torch.arange(N) % len(_W_VALS)]
    bias = torch.tensor(_BIAS)[(torch.arange(N) // len(_W_VALS)) % len(_BIAS)]
    acc = f16r(A[:, :1]) * f16r(W[:, :1]).T  # exact
    return A, W, bias, acc + bias          # one fp32 add, as the epilogue does


def _gemm16_bits(A, W, bias, epi):
    """showo_gemm_op16 with a 16-bit output, returned as an fp16 tensor (bits as written)"""
    M, K = A.shape
    N = W.shape[0]
    out = torch.zeros((M, N), dtype=torch.int16, device="cuda")
    L().call("showo_gemm_op16", L().ptr(dev(h16(A))), K, L().ptr(dev(h16(W))), K, L().ptr(dev(bias)), 0, L().ptr(out), N, None, 0,
             M, N, K, epi, F16, S())
    torch.cuda.synchronize()
    return out.cpu().view(torch.float16)


def _check_edges(A, W, bias, pre, what):
    assert torch.isinf(pre).any() and ((pre.abs() > F16_MAX) & (pre.abs() < 65520)).any() and (pre.abs() == F16_MAX).any()
    got = _gemm16_bits(A, W, bias, 0)
    assert_f16_equal(got, sat_rne(pre), what + " plain epilogue")
    # gelu_new(x) == x in fp32 for x >= 10 (the tanh / exp term is exactly 1); for large negative x it is -0 or a tiny value, and
    # gelu_new(-inf) = -inf * 0 is NaN (float64 oracle)
    gg = _gemm16_bits(A, W, bias, 1).float()
    pos = pre >= 10
    assert_f16_equal(gg[pos].half(), sat_rne(pre[pos]), what + " GELU epilogue, positive")
    neg = pre <= -10
    want = O.gelu_new(pre[neg].double())
    assert torch.equal(torch.isnan(gg[neg]), torch.isnan(want)), (what, "GELU of -inf must be NaN")
    fin = ~torch.isnan(want)
    assert ((gg[neg][fin].double() - want[fin]).abs() <= 1e-3).all(), what
    # one NaN in A: its row is NaN in every output column of both epilogues, not -65504; the other rows are untouched
    A2 = A.clone()
    r = A.shape[0] // 2
    A2[r, 3] = float("nan")
    W2 = W.clone()
    W2[:, 3] = 0.25
    rest = torch.arange(A.shape[0]) != r
    for epi in (0, 1):
        out = _gemm16_bits(A2, W2, bias, epi).float()
        assert torch.isnan(out[r]).all(), (what, "epi", epi, out[r, :8].tolist())
        # the other rows: finite + +-inf never makes a NaN; only gelu_new(-inf) does
        want_nan = torch.isneginf(pre[rest]) if epi == 1 else torch.zeros_like(pre[rest], dtype=torch.bool)
        assert torch.equal(torch.isnan(out[rest]), want_nan), (what, "epi", epi)


# M = 1 / 5: GEMV; 200: the 128^2 kernel; 774: production kernel; (631, 2048, 2048) and (577, 1024, 4096): split-K
@pytest.mark.parametrize("M,N,K", [(1, 512, 256), (5, 384, 512), (200, 256, 128), (774, 2048, 2048), (631, 2048, 2048), (577, 1024, 4096)])
def test_gemm_fp16_epilogue_saturation_and_nan(M, N, K):
    A, W, bias, pre = _edge_operands(M, N, K, M + N + K)
    _check_edges(A, W, bias, pre, f"M={M} N={N} K={K}")


@pytest.mark.parametrize("variant", [1192, 3144])
def test_gemm_fp16_epilogue_saturation_tile_families(variant):
    """two production tile families (forced variants) on the same edge operands"""
    M, N, K = 1290, 1024, 1024
    A, W, bias, pre = _edge_operands(M, N, K, variant)
    try:
        L().call("showo_gemm_set_impl", 5)
        L().call("showo_gemm_tune", 8, variant << 8, None)
        _check_edges(A, W, bias, pre, f"variant {variant}")
    finally:
        L().call("showo_gemm_tune", 8, 0, None)
        L().call("showo_gemm_set_impl", 0)


def test_qk_prep_fp16_keeps_nan():
    """a NaN in the q (k) part of one qkv row makes that row's Q (K) NaN in all 64 dims after q/k LayerNorm; a NaN in the v part is
    that one V^T element; every other element is finite"""
    B, Lq, nH = 1, 40, 2
    torch.manual_seed(1)
    qkv = torch.randn(B * Lq, 3 * nH * 64)
    qkv[5, 64 + 3] = float("nan")              # q of token 5, head 1
    qkv[9, nH * 64 + 7] = float("nan")         # k of token 9, head 0
    qkv[12, 2 * nH * 64 + 64 + 11] = float("nan")  # v of token 12, head 1, d = 11
    one, zero = torch.ones(64), torch.zeros(64)
    Q, K, Vt = _prep16(qkv, one, zero, one, zero, B, Lq, nH)
    q, k, vt = from_h16(Q.cpu()), from_h16(K.cpu()), from_h16(Vt.cpu())[..., :Lq]
    assert torch.isnan(q[0, 1, 5]).all() and torch.isnan(k[0, 0, 9]).all() and torch.isnan(vt[0, 1, 11, 12])
    assert int(torch.isnan(q).sum()) == 64 and int(torch.isnan(k).sum()) == 64 and int(torch.isnan(vt).sum()) == 1


def _attn16(Q, K, Vt, mask, rows, Lk, nH):
    B = Q.shape[0]
    md = dev(mask)
    iv = torch.zeros((B, rows, 4), dtype=torch.int32, device="cuda")
    flag = torch.zeros(4, dtype=torch.int32, device="cuda")
    Od = torch.zeros((B, rows, nH * 64), dtype=torch.int16, device="cuda")
    L().call("showo_mask_compress", L().ptr(md), L().ptr(iv), L().ptr(flag), B, rows, Lk, S())
    L().call("showo_attn_fwd_op16", L().ptr(Q), L().ptr(K), L().ptr(Vt), L().ptr(iv), L().ptr(flag), L().ptr(md), L().ptr(Od), B, nH, rows,
             Lk, K.shape[2], Vt.shape[-1], nH * 64, F16, S())
    torch.cuda.synchronize()
    return from_h16(Od.cpu())


def _roundup_score():
    """an fp16 score s < 0 whose fp32 exp(s) lies in [0.5, 1) and rounds UP to fp16 by ~0.4 ulp: P = fp16(p) exceeds p by ~4e-4 relative,
    more than the 2^-12 between 65504 and the overflow threshold 65520"""
    best = None
    for bits in range(0x3800, 0x3a00):  # fp16 values 0.5 .. 0.75
        s = -float(torch.tensor(bits, dtype=torch.int16).view(torch.float16))
        p = torch.tensor(np.exp(np.float32(s)), dtype=torch.float32)
        ulp = 2.0 ** -11
        frac = float(p) / ulp - np.floor(float(p) / ulp)
        if 0.55 <= frac <= 0.7 and float(p) >= 0.5 and (best is None or float(p) < best[1]):
            best = (s, float(p))
    assert best is not None
    return best[0]


def _bound_operands(Lk, rows):
    """Q = e0, K_j = s_j e0: scores 0 on every 16th key (each tile's maximum is the row's maximum) and the round-up score elsewhere;
    V^T = +65504 on even dims, -65504 on odd dims, for every key"""
    B, nH = 1, 1
    s = _roundup_score()
    Lp = ((Lk + 63) // 64) * 64
    q = torch.zeros(B, nH, rows, 64)
    q[..., 0] = 1.0
    k = torch.zeros(B, nH, Lk, 64)
    k[..., 0] = s
    k[:, :, ::16, 0] = 0.0
    vt = torch.zeros(B, nH, 64, Lp)
    vt[:, :, 0::2, :Lk] = F16_MAX
    vt[:, :, 1::2, :Lk] = -F16_MAX
    return dev(h16(q)), dev(h16(k)), dev(h16(vt))


@pytest.mark.parametrize("impl", [1, 2], ids=["gather", "lds-tiled"])
def test_attention_fp16_output_stays_finite_at_v_max(impl):
    """O = sum_j P_j V_j / l with P rounded to fp16 and l summing the unrounded p: at |V| = 65504 every key, O exceeds 65504 by the
    rounding of P and must be stored saturated, not as +-inf.  Prefill rows and the single-query (decode) form."""
    L().call("showo_attn_set_impl", impl)
    try:
        for rows, Lk in ((64, 256), (130, 300), (1, 256)):
            Q, K, Vt = _bound_operands(Lk, rows)
            mask = torch.zeros(1, 1, rows, Lk)
            got = _attn16(Q, K, Vt, mask, rows, Lk, 1)
            want = _attn_oracle16(Q, K, Vt, mask, rows, Lk)
            assert torch.isfinite(got).all(), (rows, Lk, got[0, 0, :4].tolist())
            err = float((got - want).abs().max())
            print(f"[parity] fp16 attention at |V| = 65504 (impl {impl}, {rows} rows x {Lk} keys): max err {err:.1f}")
            assert err <= 2.5 * 2 ** -11 * F16_MAX, (rows, Lk, err)
    finally:
        L().call("showo_attn_set_impl", 0)


@pytest.mark.parametrize("impl", [1, 2], ids=["gather", "lds-tiled"])
def test_attention_fp16_nan_in_v_and_subnormal_operands(impl):
    """a NaN in one V element reaches every output row that sees its key (NaN, not a finite value); subnormal Q, K or V are used as
    they are (a flushed operand moves the output by far more than the bound)"""
    torch.manual_seed(impl)
    B, nH, Lk = 1, 2, 200
    L().call("showo_attn_set_impl", impl)
    try:
        for rows in (Lk, 1):
            mask = torch.zeros(B, 1, rows, Lk)
            # NaN in V^T[head 1, d 5, key 17]
            q, k = torch.randn(B, nH, rows, 64) * 0.3, torch.randn(B, nH, Lk, 64) * 0.3
            vt = torch.randn(B, nH, 64, 256)
            vt[..., Lk:] = 0
            vt[0, 1, 5, 17] = float("nan")
            got = _attn16(dev(h16(q)), dev(h16(k)), dev(h16(vt)), mask, rows, Lk, nH)
            assert torch.isnan(got[:, :, 64 + 5]).all(), rows
            assert int(torch.isnan(got).sum()) == B * rows, rows
            # subnormal operands: fp16 normals start at 2^-14 = 6.1e-5
            sub = 2.0 ** -17  # randn * 2^-17 stays below 2^-14
            for case in ("q", "k", "v"):
                qs = torch.randn(B, nH, rows, 64) * (sub if case == "q" else 1e4)
                ks = torch.randn(B, nH, Lk, 64) * (sub if case == "k" else (1e4 if case == "q" else 0.3))
                if case == "v":
                    qs = torch.randn(B, nH, rows, 64) * 0.3
                vs = torch.randn(B, nH, 64, 256) * (sub if case == "v" else 1.0)
                vs[..., Lk:] = 0
                Q, K, Vt = dev(h16(qs)), dev(h16(ks)), dev(h16(vs))
                assert (from_h16(Q.cpu() if case == "q" else (K.cpu() if case == "k" else Vt.cpu())).abs().max() < 2.0 ** -14)
                got = _attn16(Q, K, Vt, mask, rows, Lk, nH)
                want = _attn_oracle16(Q, K, Vt, mask, rows, Lk)
                err = float((got - want).abs().max())
                tol = 2.5 * 2 ** -11 * float(want.abs().max()) + 2.0 ** -24 + (2e-4 * float(want.abs().max()) if case != "v" else 0.0)
                print(f"[parity] fp16 attention, subnormal {case} (impl {impl}, {rows} rows): max err {err:.3e} (scale {float(want.abs().max()):.3e})")
                assert err <= tol, (case, rows, err, tol)
    finally:
        L().call("showo_attn_set_impl", 0)


def test_count_f16_saturated_counts_max_inf_and_nan():
    """+-65504, +-inf and every NaN encoding count; 65472 (the largest value below 65504) and everything else does not"""
    torch.manual_seed(2)
    x = (torch.randn(50000) * 1000).half().view(torch.int16)
    special = [0x7bff, 0xfbff, 0x7c00, 0xfc00, 0x7e00, 0xfe00, 0x7c01, 0xffff, 0x7fff]
    perm = torch.randperm(x.numel())
    idx = perm[:len(special) * 7]
    for i, j in enumerate(idx.tolist()):
        x[j] = torch.tensor(special[i % len(special)], dtype=torch.int32).to(torch.int16)
    x[perm[-5:]] = 0x7bfe  # 65472: not counted
    xv = x.view(torch.float16).float()
    want = int(((xv.abs() == F16_MAX) | torch.isinf(xv) | torch.isnan(xv)).sum())
    assert want == len(idx)
    for n in (x.numel(), 1 + int(idx.max())):
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        L().call("showo_count_f16_saturated", L().ptr(dev(x)), n, L().ptr(cnt), S())
        w = int(((xv[:n].abs() == F16_MAX) | ~torch.isfinite(xv[:n])).sum())
        assert int(cnt) == w, (n, int(cnt), w)


# ------------------------------------------------------------------------------------------------------ B. heavy-tailed tiny model
def heavy_state(seed=11):
    d = util.tiny_dims()
    return d, Wt.make_showo_state(d, seed=seed, profile="heavy")


class _ClampCounter(O.Bf16Points):
    """the fp16 rounding-point oracle that also counts the activation elements its converts saturate"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.clamped = 0

    def r(self, site, t):
        if site in self.sites and site not in ("w", "w_lm"):
            self.clamped += int((t.abs() >= F16_MAX - 16).sum())  # values that round to +-65504 after the clamp
        return super().r(site, t)


_SITES16 = [s for s in O.Bf16Points.SITES if s not in ("w_lm", "hf")]  # precision 2: the final LayerNorm + lm_head are split-bf16


def _t2i_case():
    g = util.golden("showo_tiny_forward.npz")
    return torch.from_numpy(g["t2i_ids"]), torch.from_numpy(g["t2i_mask"])


def test_heavy_model_parity_at_every_precision():
    """the heavy profile saturates LayerNorm outputs in fp16 (the oracle says where); each precision stays within its own gate"""
    d, sd = heavy_state()
    sdt = O.to_torch(sd)
    m = util.build_showo(d, sd)
    g = util.golden("showo_tiny_forward.npz")
    for key in ("t2i", "mmu"):
        ids, mask = torch.from_numpy(g[f"{key}_ids"]), torch.from_numpy(g[f"{key}_mask"])
        ref = O.showo_logits(sdt, d, ids, attention_mask=mask)
        p16 = _ClampCounter(qkv_round=True, dtype=torch.float16, sites=_SITES16)
        want16 = O.showo_logits(sdt, d, ids, attention_mask=mask, pts=p16)
        want0 = O.showo_logits(sdt, d, ids, attention_mask=mask, pts=O.Bf16Points(qkv_round=True))
        assert p16.clamped > 0, "the heavy profile must saturate some fp16 activation"
        r1 = util.relerr(m.set_precision(1)(dev(ids), attention_mask=dev(mask)), ref)
        r0 = util.relerr(m.set_precision(0)(dev(ids), attention_mask=dev(mask)), want0)
        r2 = util.relerr(m.set_precision(2)(dev(ids), attention_mask=dev(mask)), want16)
        print(f"[parity] heavy tiny {key}: precision 1 vs fp32 oracle rel_max={r1[0]:.3e} rel_rms={r1[1]:.3e}; precision 0 vs bf16 points "
              f"{r0[0]:.3e} / {r0[1]:.3e}; precision 2 vs fp16 points {r2[0]:.3e} / {r2[1]:.3e} (oracle: {p16.clamped} clamped elements; "
              f"fp16 points vs fp32 {util.relerr(want16, ref)[0]:.3e})")
        assert r1[0] <= 1e-4, (key, r1)
        assert r0[1] <= 1e-2 and r0[0] <= 3e-2, (key, r0)  # test_modules_gpu REL_RMS / REL_MAX
        assert r2[0] <= FP16_TOL and r2[1] <= 5e-4, (key, r2)  # test_fp16_gpu's rounding-point gate


def test_range_check_matches_the_oracle_prediction():
    """range_check > 0 exactly when the fp16 oracle clamps something: on the heavy weights, and 0 on the default ones"""
    ids, mask = _t2i_case()
    for prof in ("default", "heavy"):
        d = util.tiny_dims()
        sd = Wt.make_showo_state(d, seed=11, profile=prof)
        p16 = _ClampCounter(qkv_round=True, dtype=torch.float16, sites=_SITES16)
        O.showo_logits(O.to_torch(sd), d, ids, attention_mask=mask, pts=p16)
        m = util.build_showo(d, sd).set_precision(2)
        n = m.range_check(lambda: m(dev(ids), attention_mask=dev(mask)))
        print(f"[parity] range check, {prof} weights: GPU {n} saturated fp16 activations, oracle {p16.clamped} clamped")
        assert (n > 0) == (p16.clamped > 0), (prof, n, p16.clamped)
        assert (n > 0) == (prof == "heavy")


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_nan_embedding_row_reaches_the_logits(precision):
    """a NaN planted in one embedding row: every row of that sequence that sees the token (through K / V in the 16-bit attention
    operands, not only its own residual row) gives NaN logits; the other sequences stay finite"""
    d, sd = heavy_state()
    ids, _ = _t2i_case()
    ids = ids.clone()
    used = set(ids.flatten().tolist())
    tok = next(t for t in range(10, d.llm_vocab) if t not in used)
    b = 1
    j = int((ids[b] == d.t2i_id).nonzero()[0, 0]) + 1  # the first text token after <t2i>
    ids[b, j] = tok
    mask = O.mask_t2i(ids, d.pad_id, d.soi_id, d.eoi_id)
    sd = {k: v.copy() for k, v in sd.items()}
    sd["showo.model.embed_tokens.weight"][tok] = np.nan
    m = util.build_showo(d, sd).set_precision(precision)
    lg = m(dev(ids), attention_mask=dev(mask)).cpu()
    sees = mask[b, 0, :, j] == 0
    assert sees.sum() > 1
    assert torch.isnan(lg[b][sees]).all(), (precision, int(torch.isnan(lg[b][sees]).all(-1).sum()), int(sees.sum()))
    others = torch.arange(ids.shape[0]) != b
    assert torch.isfinite(lg[others]).all(), precision


# ------------------------------------------------------------------------------------------------------ C. engine state contract
def _outputs(m, d):
    """forward logits, a t2i trajectory under fixed noise, greedy mmu tokens and a greedy two-sequence mmu batch"""
    g = util.golden("showo_tiny_forward.npz")
    out = {"forward": m(dev(g["t2i_ids"]), attention_mask=dev(g["t2i_mask"])).cpu()}
    g2 = util.golden("showo_tiny_t2i.npz")
    steps, B = int(g2["steps"]), g2["ids_cond"].shape[0]
    N, V = d.num_vq_tokens, d.codebook
    ids_c = dev(g2["ids_cond"]).clone()
    out["t2i"] = m.t2i_generate(input_ids=ids_c, uncond_input_ids=dev(g2["ids_uncond"]), attention_mask=dev(g2["mask"]), timesteps=steps,
                                guidance_scale=float(g2["guidance"]), config=util.gen_config(d),
                                _exp_noise=dev(g2["exp_noise"].reshape(steps, B * N, V)), _uniform=dev(g2["uniform"].reshape(steps, B, N))).cpu()
    g3 = util.golden("showo_tiny_mmu.npz")
    out["mmu"] = [int(t) for t in m.mmu_generate(dev(g3["ids"]), attention_mask=dev(g3["mask"]), max_new_tokens=6, top_k=1)]
    ids3 = dev(g3["ids"])
    seqs = [ids3, ids3[:, :-3].contiguous()]
    out["batch"] = [[int(t) for t in r] for r in m.mmu_generate_batch(seqs, attention_mask=[None, None], max_new_tokens=6, top_k=1)]
    return out


def _same(a, b, what):
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), (what, k, util.relerr(a[k].float(), b[k].float()))
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


_FRESH = {}


def _fresh(p):
    if p not in _FRESH:
        d, sd = util.tiny_state()
        _FRESH[p] = _outputs(util.build_showo(d, sd).set_precision(p), d)
    return _FRESH[p]


@pytest.mark.parametrize("chain", [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (2, 1, 0)], ids=lambda c: "->".join(map(str, c)))
def test_precision_switch_gives_the_fresh_engine_bits(chain):
    """one engine run at each precision of `chain` in turn gives, at the last one, the bits of an engine built at that precision"""
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd)
    for p in chain[:-1]:
        m.set_precision(p)
        _outputs(m, d)
    _same(_outputs(m.set_precision(chain[-1]), d), _fresh(chain[-1]), chain)


def test_precision_2_to_1_then_training_step_then_2():
    """2 -> 1 (the split images are bf16), a training step (bf16 images), back to 2: the bits of a fresh precision-2 engine on the
    updated weights"""
    g = util.golden("showo_tiny_forward.npz")
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd).set_precision(2)
    _outputs(m, d)
    m.set_precision(1)
    _outputs(m, d)
    m.train()
    tr = util.pkg().Trainer(m, lr=1e-3)
    tr.step(dev(g["train_ids"]), dev(g["train_mask"]), dev(g["train_labels"]), 2, 1, 2, d.max_text_len)
    m.eval()
    sd_now = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    got = _outputs(m.set_precision(2), d)
    want = _outputs(util.build_showo(d, sd_now).set_precision(2), d)
    _same(got, want, "2 -> 1 -> step -> 2")


def test_range_check_around_graph_replayed_t2i():
    """range_check around t2i_generate counts what use_graph=0 counts and leaves the ids alone, whether or not a graph for the same
    key is already cached; a graph captured while a counter was registered must not write that counter on later plain calls"""
    d, sd = heavy_state()
    m = util.build_showo(d, sd).set_precision(2)
    g2 = util.golden("showo_tiny_t2i.npz")
    steps, B = int(g2["steps"]), g2["ids_cond"].shape[0]
    N, V = d.num_vq_tokens, d.codebook
    unc, mask = dev(g2["ids_uncond"]), dev(g2["mask"])
    noise, unif = dev(g2["exp_noise"].reshape(steps, B * N, V)), dev(g2["uniform"].reshape(steps, B, N))
    cfg = util.gen_config(d)
    eng = m.engine()
    lib = util.lib()

    def run(use_graph):
        ids = dev(g2["ids_cond"]).clone()
        return m.t2i_generate(input_ids=ids, uncond_input_ids=unc, attention_mask=mask, timesteps=steps, guidance_scale=float(g2["guidance"]),
                              config=cfg, _exp_noise=noise, _uniform=unif, use_graph=use_graph).cpu()

    out_e = [None]
    n_eager = m.range_check(lambda: out_e.__setitem__(0, run(0)))
    assert n_eager > 0, "the heavy weights must saturate something"
    caps0 = lib.load().showo_engine_t2i_captures(eng)
    # no graph cached for this key yet: the counter is registered by hand and kept alive by the test
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    lib.call("showo_engine_set_range_check", eng, lib.ptr(cnt))
    try:
        out1 = run(1)
    finally:
        lib.call("showo_engine_set_range_check", eng, None)
    torch.cuda.synchronize()
    n1 = int(cnt.item())
    cnt.zero_()
    out2 = run(1)  # plain graphed call (captures or replays)
    out3 = run(1)  # plain graphed call (replays)
    torch.cuda.synchronize()
    assert int(cnt.item()) == 0, f"a plain graphed t2i_generate wrote {int(cnt.item())} into a counter no longer registered"
    assert lib.load().showo_engine_t2i_captures(eng) > caps0, "the plain graphed calls must have used a graph"
    # a graph for this key is cached now: range_check must still count every step
    out_r = [None]
    n_cached = m.range_check(lambda: out_r.__setitem__(0, run(1)))
    print(f"[parity] range check around t2i_generate (heavy weights): eager {n_eager}, graphed before capture {n1}, "
          f"graphed with a cached graph {n_cached}")
    assert n1 == n_eager and n_cached == n_eager
    for o in (out1, out2, out3, out_r[0]):
        assert torch.equal(o, out_e[0])


def _mmu_prompt(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(10, 290, (1, n), generator=g)


@pytest.mark.parametrize("poison", ["nan-row", "other-precision"])
def test_batched_decode_after_a_poisoned_batch(poison):
    """a first batch leaves NaN (a planted NaN embedding row) or the other 16-bit type in the batched KV caches; a following, shorter
    clean batch on the same engine gives the tokens of the same batch on a fresh engine.  Prompts of >= 256 tokens take the
    projection-epilogue path that writes V^T columns [0, L) only."""
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd, max_seq=512).set_precision(2)
    tok = 299
    first = [_mmu_prompt(300, 1), _mmu_prompt(280, 2)]
    clean = [_mmu_prompt(270, 3), _mmu_prompt(262, 4)]
    for p in first + clean:
        p[p == tok] = 298
    first[0][0, 10] = tok
    w = m.showo.model.embed_tokens.weight
    if poison == "nan-row":
        keep = w[tok].detach().clone()
        with torch.no_grad():
            w[tok] = float("nan")
    else:
        m.set_precision(0)
    m.mmu_generate_batch([dev(p) for p in first], attention_mask=[None, None], max_new_tokens=4, top_k=1)
    if poison == "nan-row":
        with torch.no_grad():
            w[tok] = keep
    m.set_precision(2)
    got = [[int(t) for t in r] for r in m.mmu_generate_batch([dev(p) for p in clean], attention_mask=[None, None], max_new_tokens=4, top_k=1)]
    fresh = util.build_showo(d, sd, max_seq=512).set_precision(2)
    want = [[int(t) for t in r] for r in fresh.mmu_generate_batch([dev(p) for p in clean], attention_mask=[None, None], max_new_tokens=4, top_k=1)]
    assert got == want, (poison, got, want)
