"""The training (backward) kernels at the shapes and on the branches the production step takes, each against an fp64 torch reference
of the same operation on the same bf16-rounded operands.

The per-kernel tests in test_train_gpu.py / test_kernels_gpu.py run small shapes: every attention grid there has B * nH <= 6 (only the
tail branch of the XCD-aware block order), the cross-entropy vocabularies are odd (only the scalar logits path), and the column sums
reduce at most a few partial blocks.  Here:
  * attention forward-with-lse / backward on grouped-only (B * nH a multiple of 8, the production 2 x 32 grid), mixed grouped + tail and
    tail-only grids, L a multiple of 64 (Lp == L), L = 1155 (19 key tiles) and L = 64 (one tile), on the mask families the reference
    builds (t2i with rm_pad_in_image, mmu, mmu_vit, causal lm), plus a peaked case with |S| in the tens;
  * the forward kernel (both attn_impl forms) on the mixed and production grids;
  * cross-entropy at V = 58 498 (float2 pair path), odd V with even ldl (pairs + odd tail) and odd ldl (scalar path);
  * column sums over T = 11 223 rows (351 partial blocks: ~44 per subset, the per-wave k += 32 loop runs ~11 times);
  * LayerNorm backward, qk-LayerNorm + RoPE backward and the embedding backward at stage-1 sizes.
Bounds are derived from each kernel's rounding points (u = 2^-24 is the fp32 unit roundoff, 2^-9 the bf16 one) and are never looser
than the existing test of the same kernel, which is asserted as well.  Every test prints its measured error beside its bound."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import util
from util import O, Wt, dev, from_bf16_bits, to_bf16_bits, bf16_round

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # fp32 unit roundoff


def _gamma(n):
    """gamma_n = n u / (1 - n u): the error factor of n fp32 roundings in a chain (recursive summation of n + 1 terms errs by at most
    gamma_n sum|x|)"""
    n = torch.as_tensor(n, dtype=torch.float64)
    return n * U / (1 - n * U)


def L():
    return util.lib()


def S():
    return util.lib().stream()


def _bits(t):
    return dev(to_bf16_bits(t))


def _col(t, c):
    """device pointer of column c of a row-major [rows, ld] tensor (a column section of a wider row, as the kernels address it)"""
    assert t.is_cuda and t.is_contiguous()
    return t.data_ptr() + c * t.element_size()


def _cuda_gen(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


# ================================================================================================ attention
# (B, nH, L, mask family, peaked).  Grid classes of the XCD-aware block order (attn_block_coords / bwd_block_coords): the first
# B*nH & ~7 (batch, head) pairs are "grouped", the rest "tail".
ATTN_CASES = [
    pytest.param(2, 4, 387, "t2i", False, id="grouped8-L387-t2i"),
    pytest.param(2, 32, 387, "t2i", False, id="grouped64-production-L387-t2i"),
    pytest.param(2, 6, 387, "mmu", False, id="mixed12-L387-mmu"),
    pytest.param(1, 10, 448, "mmu_vit", False, id="mixed10-L448-LpEqL-mmu_vit"),
    pytest.param(2, 3, 384, "lm", False, id="tail6-L384-LpEqL-lm"),
    pytest.param(1, 3, 130, "mmu", False, id="tail3-L130-mmu"),
    pytest.param(3, 4, 1155, "t2i", False, id="mixed12-L1155-t2i"),
    pytest.param(2, 5, 1155, "mmu_vit", False, id="mixed10-L1155-mmu_vit"),
    pytest.param(2, 5, 64, "t2i", False, id="mixed10-L64-single-tile-t2i"),
    pytest.param(2, 6, 387, "t2i", True, id="mixed12-L387-t2i-peaked"),
]
FWD_CASES = [
    pytest.param(2, 32, 387, "t2i", id="grouped64-production-L387-t2i"),
    pytest.param(2, 6, 387, "mmu", id="mixed12-L387-mmu"),
    pytest.param(1, 10, 448, "mmu_vit", id="mixed10-L448-mmu_vit"),
    pytest.param(3, 4, 1155, "t2i", id="mixed12-L1155-t2i"),
]


@functools.lru_cache(maxsize=None)
def _mask(kind, B, Lq):
    """additive mask [B, 1, L, L] of a mask family, built by the oracle's transcription of the reference's prompting_utils"""
    d = Wt.ShowoDims(**Wt.FULL)
    if kind == "t2i":  # left-padded text, [soi] image [eoi]; rm_pad_in_image = True (the training default)
        T = min(129, Lq // 3)
        N = Lq - T - 2
        g = torch.Generator().manual_seed(B * 7 + Lq)
        rows = []
        for b in range(B):
            k = (3, T, T // 2 + 1)[b % 3]
            words = torch.randint(0, 100, (k,), generator=g).tolist()
            rows.append([d.pad_id] * (T - k) + words + [d.soi_id] + [d.mask_token_id] * N + [d.eoi_id])
        return O.mask_t2i(torch.tensor(rows), d.pad_id, d.soi_id, d.eoi_id)
    if kind == "mmu":  # [mmu][soi] image [eoi] text: causal + the image prefix visible to every row
        N = min(256, Lq // 2)
        ids = torch.tensor([[d.mmu_id, d.soi_id] + [7] * N + [d.eoi_id] + [5] * (Lq - N - 3)] * B)
        return O.mask_mmu(ids, d.eoi_id)
    if kind == "mmu_vit":  # causal + the 576 CLIP-ViT columns after the system prompt
        return O.mask_mmu_vit(B, Lq, system_prompt_len=28)
    if kind == "lm":  # pure text: causal
        return O.mask_t2i(torch.full((B, Lq), 5), d.pad_id, d.soi_id, d.eoi_id, rm_pad_in_image=False)
    raise ValueError(kind)


def _attn_operands(B, nH, Lq, peaked, seed):
    g = torch.Generator().manual_seed(seed)
    qs = 1.5 if peaked else 0.4  # pre-scaled Q as the forward path stores it; peaked: |S| reaches tens
    q = bf16_round(torch.randn(B, nH, Lq, 64, generator=g) * qs)
    k = bf16_round(torch.randn(B, nH, Lq, 64, generator=g))
    v = bf16_round(torch.randn(B, nH, Lq, 64, generator=g))
    do = bf16_round(torch.randn(B, Lq, nH * 64, generator=g))
    return q, k, v, do


def _compress(mask, B, Lq):
    md = dev(mask)
    iv = torch.zeros((B, Lq, 4), dtype=torch.int32, device="cuda")
    flag = torch.zeros(4, dtype=torch.int32, device="cuda")
    L().call("showo_mask_compress", L().ptr(md), L().ptr(iv), L().ptr(flag), B, Lq, Lq, S())
    torch.cuda.synchronize()
    assert int(flag[0]) == 0, "reference-built masks are interval-representable"
    vis = mask[:, 0] == 0
    c = torch.arange(Lq)[None, None, :]
    ivc = iv.cpu()
    rec = ((c >= ivc[..., 0:1]) & (c < ivc[..., 1:2])) | ((c >= ivc[..., 2:3]) & (c < ivc[..., 3:4]))
    assert torch.equal(rec, vis)
    return md, iv, flag


def _vt(v, Lp):
    B, nH, Lq, _ = v.shape
    Vt = torch.zeros((B, nH, 64, Lp), dtype=torch.int16, device="cuda")
    Vt[..., :Lq] = _bits(v.transpose(2, 3).contiguous())
    return Vt


def _lse_bound(q, k, s, vis, lse):
    """|lse - logsumexp(S)| per row, from the forward's rounding points (u = 2^-24):
      S      : 64 bf16 x bf16 products (exact) summed in fp32 by the MFMA   <= 64 u sum_d |q_d k_d| =: 64 u A      (shifts lse by <= that)
      exp2   : the argument fma(S, log2 e, -m log2 e) and v_exp_f32         <= 2 u |S|max + 2 u          (relative, per term)
      l      : sum of n_vis positive fp32 terms (any order), the rescales   <= (n_vis + 16) u             (relative)
      lse    : m + __logf(l) (fast log: a few ulp of 2^-24)                 <= 2 u |lse| + 32 u
    The bound is the sum; it is ~1e-4 at these shapes (the existing test gates lse at 2e-2 absolute)."""
    A = (q.abs().double() @ k.abs().double().transpose(-1, -2)).masked_fill(~vis, 0).amax(-1)
    smax = s.masked_fill(~vis, 0).abs().amax(-1)
    nvis = vis.sum(-1).double()
    return U * (64 * A + 2 * smax + nvis + 2 * lse.abs() + 50)


@pytest.mark.parametrize("B,nH,Lq,kind,peaked", ATTN_CASES)
def test_attention_lse_and_backward_at_scale(B, nH, Lq, kind, peaked):
    """showo_attn_fwd_lse + showo_head_transpose + showo_attn_bwd vs fp64 autograd of softmax(Q K^T + mask) V on the same bf16
    operands, V and the gradients in the production token-major layout (rows of the [B*L, 3H] qkv / dqkv buffers).
    Bounds: lse per row by _lse_bound; O at the existing 2.5 * 2^-8 of max|O| (P and O are rounded to bf16 once each);
    dQ / dK / dV at the existing 2^-6 of the gradient scale: the bf16 roundings of P (2^-9), of dS = P (dP - D) with D from the bf16 O
    (2^-9 + 2^-8), and of the output (2^-9) add up to 2^-7 relative per term, 2^-6 with the accumulation over L;
    rel rms at 2^-7 (tighter than the existing 1e-2).  Every row of these families sees at least its own key (asserted), so no row
    relies on the reference's all-masked convention.  The backward runs twice: identical bits."""
    H = nH * 64
    Lp = (Lq + 63) // 64 * 64
    mask = _mask(kind, B, Lq)
    vis = (mask[:, 0] == 0)[:, None]  # [B, 1, L, L]
    assert bool(vis.any(-1).all()), "a row without a visible key"
    q, k, v, do = _attn_operands(B, nH, Lq, peaked, seed=B * 1000 + nH * 10 + Lq + peaked)
    # fp64 reference (autograd)
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    s = qr @ kr.transpose(-1, -2) + mask.double()
    o = (torch.softmax(s, -1) @ vr).transpose(1, 2).reshape(B, Lq, H)
    o.backward(do.double())
    s = s.detach()
    want_lse = torch.logsumexp(s, -1)
    if peaked:
        assert float(s.masked_fill(~vis, 0).abs().max()) > 20.0
    # device operands; V inside a [B*L, 3H] qkv buffer (v section), outputs into the q / k / v sections of a [B*L, 3H] buffer
    Qd, Kd = _bits(q), _bits(k)
    Vt = _vt(v, Lp)
    qkv = torch.zeros((B * Lq, 3 * H), dtype=torch.int16, device="cuda")
    qkv[:, 2 * H:] = _bits(v.transpose(1, 2).reshape(B * Lq, H).contiguous())
    md, iv, flag = _compress(mask, B, Lq)
    Od = torch.zeros((B * Lq, H), dtype=torch.int16, device="cuda")
    lse = torch.full((B, nH, Lq), float("nan"), dtype=torch.float32, device="cuda")
    L().call("showo_attn_fwd_lse", L().ptr(Qd), L().ptr(Kd), L().ptr(Vt), L().ptr(iv), L().ptr(flag), None, L().ptr(Od), L().ptr(lse),
             B, nH, Lq, Lq, Lq, Lp, H, S())
    torch.cuda.synchronize()
    lerr = (lse.cpu().double() - want_lse).abs()
    lbound = _lse_bound(q, k, s, vis, want_lse)
    worst = int((lerr / lbound).argmax())
    print(f"[parity] attn lse {kind} B={B} nH={nH} L={Lq}: max err {float(lerr.max()):.3e}, worst err/bound {float((lerr / lbound).max()):.3f} "
          f"(bound there {float(lbound.flatten()[worst]):.3e})")
    assert bool((lerr <= lbound).all()) and float(lerr.max()) < 2e-2
    oerr = float((from_bf16_bits(Od).cpu().double() - o.detach().reshape(B * Lq, H)).abs().max())
    obound = 2.5 * 2 ** -8 * float(o.abs().max()) + 1e-3
    print(f"[parity] attn fwd O {kind} B={B} nH={nH} L={Lq}: max err {oerr:.3e} <= {obound:.3e}")
    assert oerr < obound
    QT = torch.zeros((B, nH, 64, Lp), dtype=torch.int16, device="cuda")
    KT = torch.zeros_like(QT)
    L().call("showo_head_transpose", L().ptr(Qd), L().ptr(QT), B, nH, Lq, Lp, nH * Lq * 64, Lq * 64, 64, S())
    L().call("showo_head_transpose", L().ptr(Kd), L().ptr(KT), B, nH, Lq, Lp, nH * Lq * 64, Lq * 64, 64, S())
    qt = from_bf16_bits(QT).cpu()
    assert torch.equal(qt[..., :Lq], q.transpose(2, 3)) and (qt[..., Lq:] == 0).all()
    assert torch.equal(from_bf16_bits(KT).cpu()[..., :Lq], k.transpose(2, 3))
    dOd = _bits(do.reshape(B * Lq, H))

    def backward():
        dOT = torch.full((B, nH, 64, Lp), 0x7fc0, dtype=torch.int16, device="cuda")  # scratch starts as NaN: fully overwritten
        D = torch.full((B, nH, Lq), float("nan"), dtype=torch.float32, device="cuda")
        out = torch.full((B * Lq, 3 * H), 0x7fc0, dtype=torch.int16, device="cuda")
        L().call("showo_attn_bwd", L().ptr(Qd), L().ptr(Kd), L().ptr(QT), L().ptr(KT), _col(qkv, 2 * H), 3 * H, L().ptr(Od),
                 L().ptr(dOd), H, L().ptr(dOT), L().ptr(lse), L().ptr(D), L().ptr(iv), L().ptr(flag), _col(out, 0), 3 * H,
                 _col(out, H), 3 * H, _col(out, 2 * H), 3 * H, B, nH, Lq, Lp, S())
        torch.cuda.synchronize()
        return out

    out = backward()
    got = from_bf16_bits(out).cpu().double()
    assert torch.isfinite(got).all(), "some (batch, head, row) of dQ / dK / dV was never written"

    def tok(gr):  # [B,nH,L,64] -> token-major [B*L, H]
        return gr.transpose(1, 2).reshape(B * Lq, H)

    for i, (name, want) in enumerate((("dQ", tok(qr.grad)), ("dK", tok(kr.grad)), ("dV", tok(vr.grad)))):
        g = got[:, i * H:(i + 1) * H]
        err = float((g - want).abs().max())
        scale = float(want.abs().max())
        rms = float((g - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt())
        # worst (batch, head) pair: a wrong block-to-(batch, head) mapping shows up as one pair far off
        per_bh = (g - want).abs().view(B, Lq, nH, 64).amax(dim=(1, 3)) / want.abs().view(B, Lq, nH, 64).amax(dim=(1, 3)).clamp(min=1e-30)
        print(f"[parity] attn bwd {kind} B={B} nH={nH} L={Lq}{' peaked' if peaked else ''} {name}: max err {err:.3e} <= "
              f"{2 ** -6 * scale + 1e-3:.3e}, rel rms {rms:.3e} <= {2 ** -7:.3e}, worst (b, h) rel max {float(per_bh.max()):.3e}")
        assert err < 2 ** -6 * scale + 1e-3 and rms < 2 ** -7, name
        assert float(per_bh.max()) < 2 ** -5, name
    assert torch.equal(backward(), out), "attention backward is not run-to-run deterministic"


@pytest.fixture(params=[1, 2], ids=["gather", "lds-tiled"])
def attn_impl(request):
    L().call("showo_attn_set_impl", request.param)
    yield request.param
    L().call("showo_attn_set_impl", 0)


@pytest.mark.parametrize("B,nH,Lq,kind", FWD_CASES)
def test_attention_forward_at_scale(B, nH, Lq, kind, attn_impl):
    """showo_attn_fwd (both kernels) on the production and mixed grids vs fp64 softmax(Q K^T + mask) V on the same bf16 operands,
    written into a strided [B*L, 3H] output (ldo = 3H) whose other columns must stay untouched.  Bound: the existing
    2.5 * 2^-8 of max|O| (P and O are each rounded to bf16 once: 2 * 2^-9 relative), asserted per (batch, head) pair as well."""
    H = nH * 64
    Lp = (Lq + 63) // 64 * 64
    mask = _mask(kind, B, Lq)
    q, k, v, _ = _attn_operands(B, nH, Lq, False, seed=B * 1000 + nH * 10 + Lq + 7)
    with torch.no_grad():
        s = q.double() @ k.double().transpose(-1, -2) + mask.double()
        want = (torch.softmax(s, -1) @ v.double()).transpose(1, 2).reshape(B * Lq, H)
    md, iv, flag = _compress(mask, B, Lq)
    Od = torch.full((B * Lq, 3 * H), 0x7fc0, dtype=torch.int16, device="cuda")
    L().call("showo_attn_fwd", L().ptr(_bits(q)), L().ptr(_bits(k)), L().ptr(_vt(v, Lp)), L().ptr(iv), L().ptr(flag), L().ptr(md),
             _col(Od, H), B, nH, Lq, Lq, Lq, Lp, 3 * H, S())
    torch.cuda.synchronize()
    full = from_bf16_bits(Od).cpu()
    assert torch.isnan(full[:, :H]).all() and torch.isnan(full[:, 2 * H:]).all(), "wrote outside its columns"
    got = full[:, H:2 * H].double()
    err = (got - want).abs()
    bound = 2.5 * 2 ** -8 * float(want.abs().max()) + 1e-3
    per_bh = err.view(B, Lq, nH, 64).amax(dim=(1, 3)) / want.abs().view(B, Lq, nH, 64).amax(dim=(1, 3))
    print(f"[parity] attn fwd impl={attn_impl} {kind} B={B} nH={nH} L={Lq}: max err {float(err.max()):.3e} <= {bound:.3e}, "
          f"worst (b, h) rel max {float(per_bh.max()):.3e}")
    assert bool(torch.isfinite(got).all()) and float(err.max()) < bound


# ================================================================================================ cross-entropy
CE_CASES = [
    pytest.param(58498, 58498, id="pairs-V58498-ldl58498"),
    pytest.param(58497, 58498, id="pairs+odd-tail-V58497-ldl58498"),
    pytest.param(58497, 58497, id="scalar-V58497-ldl58497"),
]


@pytest.mark.parametrize("V,ldl", CE_CASES)
def test_cross_entropy_production_vocab(V, ldl):
    """showo_ce_loss at the production vocabulary on a stage-1-like batch (2 t2i, 2 lm, 2 mmu rows of 134 tokens: 804 logits rows,
    -100 labels), labels 0 and V - 1 present, and every third row peaked (one logit 30 above the row's max, at columns 0, 1, V-3, V-2,
    V-1 -- the last float2 pair and the odd tail -- at the row's label or at random).  The pad column of ldl > V holds 1e4: read, it
    would wreck the row.  vs fp64 autograd of the three F.cross_entropy slices of Showo.forward.
    Bounds (u = 2^-24, zmax = max|logit|): a row's lse is the fp32 max, a fp32 sum of V exponentials in chains of <= 2 ceil(V / 256)
    per thread + 8 reduction levels, and logf: |d lse| <= u (2 ceil(V/256) + 32 + 4 zmax) =: u K; the mean over rows keeps it (the
    finalize sums in fp64), plus 2 u |loss| for the final rounding.  dlogits = w (softmax - onehot) rounded to bf16:
    |d g| <= 2^-8 |g| + u K w_row elementwise.  The existing gates (1e-4 |loss| + 1e-5; 2^-8 max|g| + 1e-6) are asserted too.
    Columns [V, Vp) of dlogits must be zero."""
    b_t2i, b_lm, b_mmu, Lq, msl = 2, 2, 2, 134, 40
    B = b_t2i + b_lm + b_mmu
    R = B * Lq
    Vp = (V + 63) // 64 * 64
    g = torch.Generator().manual_seed(V + ldl)
    z = torch.randn(R, V, generator=g) * 2
    labels = torch.randint(0, V, (B, Lq), generator=g)
    labels[:b_t2i, :msl + 1] = -100  # t2i: text part never labelled
    labels[:b_t2i][torch.rand(b_t2i, Lq, generator=g) < 0.5] = -100  # unmasked image tokens
    labels[b_t2i:b_t2i + b_lm, -20:] = -100  # lm padding
    labels[-b_mmu:, :60] = -100  # mmu: the image part carries no label
    labels[0, msl + 1], labels[1, msl + 2], labels[b_t2i, 5], labels[-1, 70], labels[-2, Lq - 1] = 0, V - 1, 0, V - 1, 0
    # the row's target column (A: labels[b, l] of t2i rows; B: labels[b, l + 1] of lm / mmu rows) -- used to place some peaks
    tgt = torch.full((B, Lq), -1, dtype=torch.int64)
    tgt[:b_t2i] = labels[:b_t2i]
    tgt[b_t2i:, :-1] = labels[b_t2i:, 1:]
    tgt = tgt.reshape(R)
    spots = [0, 1, V - 3, V - 2, V - 1, None, "rand"]
    for n, r in enumerate(range(0, R, 3)):
        p = spots[n % len(spots)]
        if p is None:
            p = int(tgt[r]) if int(tgt[r]) >= 0 else V - 1
        elif p == "rand":
            p = int(torch.randint(0, V, (1,), generator=g))
        z[r, p] = z[r].max() + 30.0
    gw = (1.0, 0.2, 0.8)
    zr = z.double().requires_grad_(True)
    zv = zr.view(B, Lq, V)
    l1 = F.cross_entropy(zv[:b_t2i, msl + 1:].reshape(-1, V), labels[:b_t2i, msl + 1:].reshape(-1), ignore_index=-100)
    l2 = F.cross_entropy(zv[b_t2i:b_t2i + b_lm, :-1].reshape(-1, V), labels[b_t2i:b_t2i + b_lm, 1:].reshape(-1), ignore_index=-100)
    l3 = F.cross_entropy(zv[-b_mmu:, :-1].reshape(-1, V), labels[-b_mmu:, 1:].reshape(-1), ignore_index=-100)
    (gw[0] * l1 + gw[1] * l2 + gw[2] * l3).backward()
    want_g = zr.grad
    # per-row weight w = wa + wb of the kernel (mean over each group's valid labels)
    c1 = int((labels[:b_t2i, msl + 1:] != -100).sum())
    c2 = int((labels[b_t2i:b_t2i + b_lm, 1:] != -100).sum())
    c3 = int((labels[-b_mmu:, 1:] != -100).sum())
    w = torch.zeros(B, Lq, dtype=torch.float64)
    w[:b_t2i, msl + 1:] += (labels[:b_t2i, msl + 1:] != -100) * (gw[0] / c1)
    w[b_t2i:b_t2i + b_lm, :-1] += (labels[b_t2i:b_t2i + b_lm, 1:] != -100) * (gw[1] / c2)
    w[-b_mmu:, :-1] += (labels[-b_mmu:, 1:] != -100) * (gw[2] / c3)
    w = w.reshape(R, 1)
    K = 2 * math.ceil(V / 256) + 32 + 4 * float(z.abs().max())
    # device: logits rows of stride ldl, pad columns poisoned
    zd = torch.full((R, ldl), 1e4, dtype=torch.float32)
    zd[:, :V] = z
    zd = dev(zd)
    rows = torch.zeros(3 * R, dtype=torch.int32, device="cuda")
    counts = torch.zeros(4, dtype=torch.int32, device="cuda")
    rowloss = torch.zeros(2 * R, dtype=torch.float32, device="cuda")
    dl = torch.full((R, Vp), 0x7fc0, dtype=torch.int16, device="cuda")
    losses = torch.zeros(4, dtype=torch.float32, device="cuda")
    L().call("showo_ce_loss", L().ptr(zd), ldl, L().ptr(dev(labels)), B, Lq, V, b_t2i, b_lm, b_mmu, msl, gw[0], gw[1], gw[2],
             L().ptr(rows), L().ptr(counts), L().ptr(rowloss), L().ptr(dl), Vp, L().ptr(losses), S())
    torch.cuda.synchronize()
    got = losses.cpu().double()
    for i, l in enumerate((l1, l2, l3)):
        lv = float(l)
        err, bound = abs(float(got[i]) - lv), U * K + 2 * U * abs(lv)
        print(f"[parity] ce V={V} ldl={ldl} loss[{i}] = {lv:.6f}: err {err:.3e} <= {bound:.3e}")
        assert err <= bound and err < 1e-4 * abs(lv) + 1e-5, (i, float(got[i]), lv)
    gd = from_bf16_bits(dl).cpu()
    assert (gd[:, V:] == 0).all(), "pad columns of dlogits"
    e = (gd[:, :V].double() - want_g).abs()
    eb = 2 ** -8 * want_g.abs() + U * K * w
    print(f"[parity] ce V={V} ldl={ldl} dlogits: max err {float(e.max()):.3e} (scale {float(want_g.abs().max()):.3e}), "
          f"worst err/elementwise bound {float((e / eb.clamp(min=1e-300)).max()):.3f}")
    assert bool((e <= eb).all()) and float(e.max()) < 2 ** -8 * float(want_g.abs().max()) + 1e-6


# ================================================================================================ column sums
T_STAGE1 = 11223  # tokens of the stage-1 training batch


def _cancelling_bf16(T, ld, seed):
    """bf16 [T, ld] on the device: column c holds (-1)^t M_c + N(0, 1) with M_c in [-20, 20] (sums cancel to ~sqrt(T) against
    sum|x| ~ 10 T), every 7th column a same-signed large mean 10 + N(0, 1)"""
    g = _cuda_gen(seed)
    M = (torch.rand(ld, generator=g, device="cuda") * 2 - 1) * 20
    sgn = 1.0 - 2.0 * (torch.arange(T, device="cuda") % 2).float()
    x = sgn[:, None] * M[None, :] + torch.randn(T, ld, generator=g, device="cuda")
    x[:, ::7] = 10.0 + torch.randn(T, (ld + 6) // 7, generator=g, device="cuda")
    return x.to(torch.bfloat16)


def _colsum_ref(xb, C):
    """fp64 column sums and sums of |x| of a bf16 [T, >= C] device matrix, in row chunks (no T x C fp64 copy)"""
    s = torch.zeros(C, dtype=torch.float64, device="cuda")
    a = torch.zeros_like(s)
    for r in range(0, xb.shape[0], 1024):
        blk = xb[r:r + 1024, :C].double()
        s += blk.sum(0)
        a += blk.abs().sum(0)
    return s, a


def _colsum_chain(nblk_rows, rows_per_block):
    """longest chain of fp32 additions in colsum_reduce over nblk partial rows of rows_per_block-row sums: the block's own sum, the
    subset wave's sequential sum (ceil(nblk / 32) terms), the (0+1)+(2+3) wave combine and the 3-level combine of the 8 subsets"""
    return rows_per_block + math.ceil(nblk_rows / 32) + 2 + 3


@pytest.mark.parametrize("C,ld", [(2048, 2048), (8192, 8192), (6144, 6208), (58560, 58560), (2045, 2056)],
                         ids=["C2048", "C8192", "C6144-ld6208", "C58560-lm_head", "C2045-ld2056-ragged"])
def test_colsum_stage1_rows(C, ld):
    """showo_colsum_bf16 over T = 11 223 rows (351 partial blocks of 32 rows: 44 per subset, 11 per subset wave) vs fp64 sums on
    columns with cancellation and large means; accumulate = 1 into a non-zero base; two runs identical bits.
    Bound (recursive summation): |err_c| <= gamma_{n-1} sum_t |x_tc| (~ (n - 1) u) per column, n = 32 + ceil(351 / 32) + 2 + 3 the
    longest addition chain (+1 for the accumulate), and the existing gate 1e-5 max|sum| + 1e-4 over all columns."""
    T = T_STAGE1
    xb = _cancelling_bf16(T, ld, seed=C + ld)
    nblk = (T + 31) // 32
    part = torch.full(((nblk + 8) * C,), float("nan"), dtype=torch.float32, device="cuda")
    cs = torch.full((C,), float("nan"), dtype=torch.float32, device="cuda")
    L().call("showo_colsum_bf16", L().ptr(xb), ld, T, C, L().ptr(part), L().ptr(cs), 0, S())
    torch.cuda.synchronize()
    want, absum = _colsum_ref(xb, C)
    n = _colsum_chain(nblk, 32)
    err = (cs.double() - want).abs()
    bound = _gamma(n - 1) * absum
    print(f"[parity] colsum T={T} C={C} ld={ld}: max err {float(err.max()):.3e}, worst err/bound {float((err / bound).max()):.3f}, "
          f"max |sum| {float(want.abs().max()):.3e}, median |sum| / sum|x| {float((want.abs() / absum).median()):.2e}")
    assert bool((err <= bound).all()) and float(err.max()) < 1e-5 * float(want.abs().max()) + 1e-4
    cs2 = torch.full_like(cs, float("nan"))
    L().call("showo_colsum_bf16", L().ptr(xb), ld, T, C, L().ptr(part), L().ptr(cs2), 0, S())
    torch.cuda.synchronize()
    assert torch.equal(cs, cs2), "colsum is not run-to-run deterministic"
    base = torch.randn(C, generator=_cuda_gen(C), device="cuda") * 100
    acc = base.clone()
    L().call("showo_colsum_bf16", L().ptr(xb), ld, T, C, L().ptr(part), L().ptr(acc), 1, S())
    torch.cuda.synchronize()
    wa = base.double() + want
    erra = (acc.double() - wa).abs()
    bounda = _gamma(n) * (absum + base.double().abs())
    print(f"[parity] colsum accumulate T={T} C={C}: max err {float(erra.max()):.3e}, worst err/bound {float((erra / bounda).max()):.3f}")
    assert bool((erra <= bounda).all())


def test_dgelu_colsum_stage1_rows():
    """showo_dgelu_colsum_bf16 at the fc1 shape [11 223, 8192] (176 partial blocks of 64 rows), in place: df bit-equal to
    showo_dgelu_bf16, column sums vs the fp64 sums of that df within gamma_{n-1} sum|df| (n = 64 + ceil(176 / 32) + 5) and the
    existing gate 1e-5 max|sum| + 1e-5"""
    T, C = T_STAGE1, 8192
    g = _cuda_gen(5)
    f = (torch.randn(T, C, generator=g, device="cuda") * 2).to(torch.bfloat16)
    da = (torch.randn(T, C, generator=g, device="cuda") + 3.0 * (torch.arange(C, device="cuda") % 5 == 0)).to(torch.bfloat16)
    ref = torch.empty_like(da)
    L().call("showo_dgelu_bf16", L().ptr(da), L().ptr(f), L().ptr(ref), T * C, S())
    buf = da.clone()
    nblk = (T + 63) // 64
    part = torch.full(((nblk + 8) * C,), float("nan"), dtype=torch.float32, device="cuda")
    cs = torch.full((C,), float("nan"), dtype=torch.float32, device="cuda")
    L().call("showo_dgelu_colsum_bf16", L().ptr(buf), L().ptr(f), L().ptr(buf), C, T, C, L().ptr(part), L().ptr(cs), S())
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int16), ref.view(torch.int16))
    want, absum = _colsum_ref(ref, C)
    err = (cs.double() - want).abs()
    bound = _gamma(_colsum_chain(nblk, 64) - 1) * absum
    print(f"[parity] dgelu colsum T={T} C={C}: max err {float(err.max()):.3e}, worst err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()) and float(err.max()) < 1e-5 * float(want.abs().max()) + 1e-5


# ================================================================================================ LayerNorm backward
@pytest.mark.parametrize("T,H", [(T_STAGE1, 2048), (3001, 2048)], ids=["T11223-H2048", "T3001-H2048"])
def test_layernorm_backward_stage1(T, H):
    """showo_ln_bwd and showo_ln_bwd_colsum at the stage-1 size (702 blocks of LNB_ROWS = 16 rows; T % 16 != 0 in both cases) vs fp64
    autograd of LayerNorm, with near-constant rows (variance 1e-8 << eps) and rows of mean +-50.
    Bounds: dx32 per row at the existing 1e-4 of the row's max|dx| (fp32 mean / variance / two reductions: ~100 u relative,
    the mean's rounding on a mean-50 row ~40 u * 50 against a unit deviation); dx16 == bf16(dx32) exactly; dgamma / dbeta at the
    existing 1e-4 max + 1e-5; dxsum (column sums of dx16) vs fp64 within gamma_{n-1} sum|dx16|, n = 4 + 2 + ceil(blocks / 32) + 5, and the
    existing 1e-5 max + 1e-5.  Two runs: identical bits."""
    g = torch.Generator().manual_seed(T + H)
    x = torch.randn(T, H, generator=g) * 1.5 + 0.2
    nc = torch.arange(5, T, 97)  # near-constant rows
    x[nc] = (torch.rand(len(nc), 1, generator=g) * 2 - 1) + 1e-4 * torch.randn(len(nc), H, generator=g)
    lm = torch.arange(11, T, 53)  # large-mean rows
    x[lm] = 50.0 * torch.sign(torch.randn(len(lm), 1, generator=g)) + torch.randn(len(lm), H, generator=g)
    gamma = torch.randn(H, generator=g) * 0.1 + 1
    dh, dy = torch.randn(T, H, generator=g), torch.randn(T, H, generator=g)
    xr, gr, br = x.double().requires_grad_(True), gamma.double().requires_grad_(True), torch.zeros(H, dtype=torch.float64, requires_grad=True)
    (O.layer_norm(xr, gr, br, 1e-5) * dh.double()).sum().backward()
    want_dx = xr.grad + dy.double()
    nblk = L().load().showo_ln_bwd_blocks(T)
    xd, gd, dhd = dev(x), dev(gamma), dev(dh)

    def run(colsum):
        part = torch.full((nblk, 3 if colsum else 2, H), float("nan"), dtype=torch.float32, device="cuda")
        dgb = torch.full((2, H), float("nan"), dtype=torch.float32, device="cuda")
        dx32 = dev(dy.clone())
        dx16 = torch.zeros((T, H), dtype=torch.int16, device="cuda")
        if colsum:
            dxs = torch.full((H,), float("nan"), dtype=torch.float32, device="cuda")
            L().call("showo_ln_bwd_colsum", L().ptr(xd), L().ptr(gd), L().ptr(dhd), L().ptr(dx32), L().ptr(dx32), L().ptr(dx16),
                     L().ptr(part), L().ptr(dgb), L().ptr(dxs), T, H, 1e-5, S())
        else:
            dxs = None
            L().call("showo_ln_bwd", L().ptr(xd), L().ptr(gd), L().ptr(dhd), L().ptr(dx32), L().ptr(dx32), L().ptr(dx16),
                     L().ptr(part), L().ptr(dgb), T, H, 1e-5, S())
        torch.cuda.synchronize()
        return dx32, dx16, dgb, dxs

    dx32, dx16, dgb, _ = run(False)
    e = (dx32.cpu().double() - want_dx).abs()
    row_rel = e.amax(1) / want_dx.abs().amax(1)
    print(f"[parity] ln_bwd T={T} H={H}: dx32 worst row rel max {float(row_rel.max()):.3e} <= 1e-4 "
          f"(near-constant rows {float(row_rel[nc].max()):.3e}, mean-50 rows {float(row_rel[lm].max()):.3e})")
    assert float(row_rel.max()) < 1e-4
    assert torch.equal(from_bf16_bits(dx16).cpu(), bf16_round(dx32.cpu()))
    for i, (name, want) in enumerate((("dgamma", gr.grad), ("dbeta", br.grad))):
        err = float((dgb[i].cpu().double() - want).abs().max())
        print(f"[parity] ln_bwd T={T} {name}: max err {err:.3e} <= {1e-4 * float(want.abs().max()) + 1e-5:.3e}")
        assert err < 1e-4 * float(want.abs().max()) + 1e-5, name
    dx32b, dx16b, dgb2, dxs = run(True)
    assert torch.equal(dx32b, dx32) and torch.equal(dx16b, dx16) and torch.equal(dgb2, dgb)
    want, absum = _colsum_ref(dx16.view(torch.bfloat16), H)
    n = 4 + 2 + math.ceil((nblk - 8) / 32) + 5
    err = (dxs.double() - want).abs()
    bound = _gamma(n - 1) * absum
    print(f"[parity] ln_bwd_colsum T={T} dxsum: max err {float(err.max()):.3e}, worst err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()) and float(err.max()) < 1e-5 * float(want.abs().max()) + 1e-5
    again = run(True)
    assert all(torch.equal(a, b) for a, b in zip(again, (dx32b, dx16b, dgb2, dxs))), "ln_bwd is not run-to-run deterministic"


# ================================================================================================ qk-LayerNorm + RoPE backward
@pytest.mark.parametrize("B,Lq,nH", [(6, 387, 32), (3, 387, 5)], ids=["B6-L387-nH32", "B3-L387-nH5-ragged-rows"])
def test_qk_layernorm_rope_backward_at_scale(B, Lq, nH):
    """showo_qkln_rope_bwd with 32 heads at L = 387 (RoPE positions up to 386 from the full 2048-position tables, rotary_dim 32;
    291 blocks of 256 (token, head) rows) and a 5-head case whose T * nH is not a multiple of the block's rows, vs fp64 autograd.
    Bounds: dqkv within 2^-8 of max|grad| (half the existing 2^-7: one bf16 output rounding, 2^-9, plus fp32 LayerNorm arithmetic
    ~100 u); d(ln weights / biases) within (n + 64) u sum_rows |term| (n = 8 + 3 + 2 + ceil(blocks / 32) + 5 additions, the 64 u
    for the fp32 terms themselves) and the existing 1e-3 max + 1e-4.  The v section stays untouched; two runs identical bits."""
    T, H = B * Lq, nH * 64
    g = torch.Generator().manual_seed(B * nH + Lq)
    qkv = bf16_round(torch.randn(T, 3 * H, generator=g) * 1.5 + 0.3)
    qw, qb = torch.randn(64, generator=g) * .1 + 1, torch.randn(64, generator=g) * .05
    kw, kb = torch.randn(64, generator=g) * .1 + 1, torch.randn(64, generator=g) * .05
    dq, dk = bf16_round(torch.randn(T, H, generator=g)), bf16_round(torch.randn(T, H, generator=g))
    cos, sin = O.rope_tables(32, 2048, 10000.0)
    x = qkv.double().requires_grad_(True)
    pw = [t.double().requires_grad_(True) for t in (qw, qb, kw, kb)]
    xv = x.view(B, Lq, 3, nH, 64)
    cs, sn = cos[:Lq].double(), sin[:Lq].double()
    qn = O.layer_norm(xv[:, :, 0].transpose(1, 2), pw[0], pw[1], 1e-5)
    kn = O.layer_norm(xv[:, :, 1].transpose(1, 2), pw[2], pw[3], 1e-5)
    q = O.apply_partial_rope(qn, cs, sn, 32) * 0.125
    k = O.apply_partial_rope(kn, cs, sn, 32)
    dqd, dkd = dq.double().view(B, Lq, nH, 64).transpose(1, 2), dk.double().view(B, Lq, nH, 64).transpose(1, 2)
    ((q * dqd).sum() + (k * dkd).sum()).backward()
    # |terms| of the parameter gradients: d(ln out) (= the rope / scale backward of dq, dk) times xhat, and d(ln out) itself
    qn_, kn_ = qn.detach(), kn.detach()
    with torch.no_grad():
        gq = torch.autograd.functional.vjp(lambda t: O.apply_partial_rope(t, cs, sn, 32) * 0.125, qn_, dqd)[1]
        gk = torch.autograd.functional.vjp(lambda t: O.apply_partial_rope(t, cs, sn, 32), kn_, dkd)[1]
    xq = (qn_ - pw[1].detach()) / pw[0].detach()
    xk = (kn_ - pw[3].detach()) / pw[2].detach()
    absterm = [(gq * xq).abs().sum((0, 1, 2)), gq.abs().sum((0, 1, 2)), (gk * xk).abs().sum((0, 1, 2)), gk.abs().sum((0, 1, 2))]
    nblk = L().load().showo_qkln_rope_bwd_blocks(T, nH)
    cosd, sind, qkvd = dev(cos), dev(sin), _bits(qkv)

    def run():
        part = torch.full((nblk, 4, 64), float("nan"), dtype=torch.float32, device="cuda")
        dpar = torch.full((4, 64), float("nan"), dtype=torch.float32, device="cuda")
        dqkv = torch.full((T, 3 * H), 0x7fc0, dtype=torch.int16, device="cuda")
        L().call("showo_qkln_rope_bwd", L().ptr(_bits(dq)), L().ptr(_bits(dk)), H, L().ptr(qkvd), L().ptr(dev(qw)), L().ptr(dev(kw)),
                 L().ptr(cosd), L().ptr(sind), L().ptr(dqkv), L().ptr(part), L().ptr(dpar), T, Lq, nH, 32, 1e-5, S())
        torch.cuda.synchronize()
        return dqkv, dpar

    dqkv, dpar = run()
    got = from_bf16_bits(dqkv).cpu()
    assert torch.isnan(got[:, 2 * H:]).all(), "the v section belongs to the attention backward"
    want = x.grad[:, :2 * H]
    err = float((got[:, :2 * H].double() - want).abs().max())
    print(f"[parity] qkln_rope_bwd B={B} L={Lq} nH={nH}: dqkv max err {err:.3e} <= {2 ** -8 * float(want.abs().max()):.3e}")
    assert err < 2 ** -8 * float(want.abs().max())
    n = 8 + 3 + 2 + math.ceil((nblk - 8) / 32) + 5
    for i, (p, name) in enumerate(zip(pw, ("dq_ln_w", "dq_ln_b", "dk_ln_w", "dk_ln_b"))):
        e = (dpar[i].cpu().double() - p.grad).abs()
        bound = (n + 64) * U * absterm[i]
        print(f"[parity] qkln_rope_bwd {name}: max err {float(e.max()):.3e}, worst err/bound {float((e / bound).max()):.3f}")
        assert bool((e <= bound).all()) and float(e.max()) < 1e-3 * float(p.grad.abs().max()) + 1e-4, name
    dqkv2, dpar2 = run()
    assert torch.equal(dqkv2, dqkv) and torch.equal(dpar2, dpar), "qkln_rope_bwd is not run-to-run deterministic"


# ================================================================================================ embedding backward
def test_embedding_backward_stage1():
    """showo_embed_bwd at T = 11 223, H = 2048, V = 58 498 with the mask token (V - 1) on half the rows and ids 0 and V - 1 present,
    vs fp64 index_add.  Each id's row is an fp32 sum of its n_id rows in position order: |err| <= gamma_{n_id - 1} sum|dx|; the existing
    absolute 1e-4 holds too (dx ~ 0.01, a gradient's scale).  Rows of absent ids stay zero; two runs identical bits."""
    T, H, V = T_STAGE1, 2048, 58498
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, V, (T,), generator=g)
    ids[torch.rand(T, generator=g) < 0.5] = V - 1  # the mask token of the t2i rows
    ids[torch.randint(0, T, (40,), generator=g)] = 7  # a common text token
    ids[[3, 4000, T - 1]] = 0
    dx = torch.randn(T, H, generator=g) * 0.01
    uniq, inv = torch.unique(ids, return_inverse=True)
    want = torch.zeros(len(uniq), H, dtype=torch.float64).index_add_(0, inv, dx.double())
    absum = torch.zeros(len(uniq), H, dtype=torch.float64).index_add_(0, inv, dx.double().abs())
    cnt = torch.bincount(inv, minlength=len(uniq)).double()[:, None]
    idd, dxd = dev(ids), dev(dx)
    ws = torch.zeros(2 * T, dtype=torch.int32, device="cuda")

    def run():
        dE = torch.zeros((V, H), dtype=torch.float32, device="cuda")
        L().call("showo_embed_bwd", L().ptr(idd), L().ptr(dxd), L().ptr(dE), L().ptr(ws), T, H, V, S())
        torch.cuda.synchronize()
        return dE

    dE = run()
    got = dE[uniq.cuda()].cpu().double()
    err = (got - want).abs()
    bound = _gamma((cnt - 1).clamp(min=0)) * absum
    print(f"[parity] embed_bwd T={T} H={H} V={V}: {int(cnt.max())} rows of id {int(uniq[int(cnt.argmax())])}, max err "
          f"{float(err.max()):.3e} <= 1e-4, worst err/bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all()) and float(err.max()) < 1e-4
    assert int((dE != 0).any(1).sum()) == len(uniq), "rows of absent ids were written"
    assert torch.equal(run(), dE), "embedding backward is not run-to-run deterministic"
