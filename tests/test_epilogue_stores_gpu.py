"""The 16-byte store forms of the projection epilogue (Q / K / V^T) and of the attention forward output against the narrow forms they
replace.  Both forms must write the SAME bytes to the SAME addresses and nothing else: every case runs one call twice in one process
-- showo_gemm_set_wide_stores / showo_attn_set_wide_stores 0, then 1 -- into destination buffers pre-filled with a non-zero sentinel
pattern, and asserts torch.equal on the WHOLE buffers (cached text columns left of pos0, the columns of other sequences, the pad
between rows of a strided output and the rows past Lq of a last tile must all survive).  No tolerance: bit equality.

Projection cases (B, Lq, nH, pos0) with Lp = roundup64(pos0 + Lq) and Lcap = pos0 + Lq + 3.  showo_gemm_qkv_fc1_bf16 needs
3 nH 64 to be a multiple of the 256-column tile (the fc1 columns start on a tile boundary), which nH = 1 and nH = 2 are not: each
case therefore runs with the stated nH through showo_gemm_qkv_bf16 (the same launch and epilogue without the fc1 columns) AND with
nH = 4 through showo_gemm_qkv_fc1_bf16."""
import pytest
import torch

import util
from util import dev, to_bf16_bits

pytestmark = pytest.mark.gpu

F16 = 1  # SHOWO_OP_F16


def L():
    return util.lib()


def S():
    return util.lib().stream()


def _sentinel(shape, seed, lead=0):
    """int16 buffer of a non-zero pattern; `lead` extra elements in front (for a base that is offset from the allocation)"""
    numel = 1
    for s in shape:
        numel *= s
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(1, 0x7f00, (numel + lead,), generator=g, dtype=torch.int32).to(torch.int16)
    return t.cuda()


CASES = [(3, 130, 2, 129),   # odd offset, a sequence boundary inside wave tiles
         (4, 70, 1, 7),      # three segments in one wave tile
         (2, 97, 1, 5),      # M not a multiple of 16, ragged last tile
         (1, 200, 2, 0),     # aligned
         (2, 258, 2, 129),   # the t2i geometry
         (5, 40, 1, 7)]      # (added) three segments in every 96-row wave tile: the fallback inside the 16-byte form
VARIANTS = [3192, 3160, 1192, 256]  # the new V^T path on three tile families; MF 8: the 2-byte form


class _Proj:
    """operands of one projection case, made once"""

    def __init__(self, B, Lq, nH, pos0, F, half=False):
        torch.manual_seed(B * 1000 + Lq * 7 + nH + pos0)
        self.B, self.Lq, self.nH, self.pos0, self.F = B, Lq, nH, pos0, F
        H = self.H = nH * 64
        self.M = B * Lq
        self.Lp = (pos0 + Lq + 63) // 64 * 64
        self.Lcap = pos0 + Lq + 3
        conv = (lambda t: t.to(torch.float16).view(torch.int16)) if half else to_bf16_bits
        self.h = dev(conv(torch.randn(self.M, H)))
        self.W = dev(conv(torch.randn(3 * H + F, H) * 0.05))
        self.bias = dev(torch.randn(3 * H + F) * 0.1)
        self.ln = [dev(torch.randn(64) * 0.2 + (1.0 if i % 2 == 0 else 0.0)) for i in range(4)]
        ang = torch.arange(self.Lcap + 8, dtype=torch.float32)[:, None] * (10000.0 ** (-torch.arange(32, dtype=torch.float32) % 16 / 16.0))[None]
        self.cos, self.sin = dev(torch.cos(ang).contiguous()), dev(torch.sin(ang).contiguous())

    def run(self, wide, entry="fc1", q_lead=0):
        """one launch into fresh sentinel buffers; returns every destination buffer (whole allocations)"""
        B, Lq, nH, H, F, M = self.B, self.Lq, self.nH, self.H, self.F, self.M
        Q = _sentinel((B, nH, Lq, 64), 1, q_lead)
        K = _sentinel((B, nH, self.Lcap, 64), 2)
        Vt = _sentinel((B, nH, 64, self.Lp), 3)
        f = _sentinel((M, max(F, 4)), 4)
        raw = _sentinel((M, 3 * H), 5)
        pre = _sentinel((M, max(F, 4)), 6)
        p = L().ptr
        qp = Q.data_ptr() + 2 * q_lead
        common = [p(self.h), H, p(self.W), H, p(self.bias), *[p(t) for t in self.ln], p(self.cos), p(self.sin), qp, p(K), p(Vt)]
        tail = [B, Lq, nH, 32, 1e-5, self.pos0, self.Lcap, self.Lp]
        L().call("showo_gemm_set_wide_stores", wide)
        try:
            if entry == "fc1":
                L().call("showo_gemm_qkv_fc1_bf16", *common, p(f), F, F, *tail, 0, S())
            elif entry == "qkv":
                L().call("showo_gemm_qkv_bf16", *common, *tail, S())
            elif entry == "f16":
                L().call("showo_gemm_qkv_fc1_op16", *common, p(f), F, F, *tail, 0, F16, S())
            elif entry == "save":
                L().call("showo_gemm_qkv_fc1_save_bf16", *common, p(raw), 3 * H, p(pre), p(f), F, F, *tail, 0, S())
            else:
                raise AssertionError(entry)
            torch.cuda.synchronize()
        finally:
            L().call("showo_gemm_set_wide_stores", -1)
        return {"Q": Q, "K": K, "Vt": Vt, "ffn": f, "raw": raw, "pre": pre}


def _same(old, new, sentinel_left=()):
    for k in old:
        assert torch.equal(old[k], new[k]), f"{k}: the 16-byte stores differ from the narrow stores"
    for k in sentinel_left:
        assert torch.equal(old[k], _sentinel(tuple(old[k].shape), {"raw": 5, "pre": 6, "ffn": 4}[k])), f"{k} was written"


def _written(p, out):
    """the launch wrote what it should have: the new rows differ from the sentinel in (nearly) every element"""
    ref = _sentinel((p.B, p.nH, 64, p.Lp), 3).view(p.B, p.nH, 64, p.Lp)
    v = out["Vt"].view(p.B, p.nH, 64, p.Lp)
    new = v[..., p.pos0:p.pos0 + p.Lq] != ref[..., p.pos0:p.pos0 + p.Lq]
    assert float(new.float().mean()) > 0.99
    assert torch.equal(v[..., :p.pos0], ref[..., :p.pos0]) and torch.equal(v[..., p.pos0 + p.Lq:], ref[..., p.pos0 + p.Lq:])


@pytest.fixture
def variant(request):
    L().call("showo_gemm_tune", 8, request.param << 8, None)
    yield request.param
    L().call("showo_gemm_tune", 8, 0, None)


@pytest.mark.parametrize("variant", VARIANTS, indirect=True)
@pytest.mark.parametrize("B,Lq,nH,pos0", CASES)
def test_projection_wide_stores_equal_narrow_stores(variant, B, Lq, nH, pos0):
    p = _Proj(B, Lq, nH, pos0, 0)
    old, new = p.run(0, "qkv"), p.run(1, "qkv")
    _same(old, new, ("raw", "pre", "ffn"))
    _written(p, new)
    p4 = _Proj(B, Lq, 4, pos0, 256)
    old, new = p4.run(0, "fc1"), p4.run(1, "fc1")
    _same(old, new, ("raw", "pre"))
    _written(p4, new)


@pytest.mark.parametrize("variant", [3192], indirect=True)
def test_projection_wide_stores_fp16_instance(variant):
    p = _Proj(3, 130, 4, 129, 256, half=True)
    old, new = p.run(0, "f16"), p.run(1, "f16")
    _same(old, new, ("raw", "pre"))
    _written(p, new)


@pytest.mark.parametrize("variant", [3192], indirect=True)
def test_projection_wide_stores_save_form(variant):
    p = _Proj(2, 258, 4, 129, 256)
    old, new = p.run(0, "save"), p.run(1, "save")
    _same(old, new)
    _written(p, new)
    assert not torch.equal(new["raw"], _sentinel(tuple(new["raw"].shape), 5))


@pytest.mark.parametrize("variant", [3192], indirect=True)
def test_projection_unaligned_q_base_takes_the_narrow_stores(variant):
    """a Q base 8 bytes off a 16-byte boundary: the 16-byte form must not be used, and the launch still writes the right bytes"""
    p = _Proj(3, 130, 4, 129, 256)
    aligned = p.run(1, "fc1")
    old, new = p.run(0, "fc1", q_lead=4), p.run(1, "fc1", q_lead=4)
    _same(old, new, ("raw", "pre"))
    assert torch.equal(new["Q"][4:], aligned["Q"]) and torch.equal(new["Q"][:4], _sentinel((p.B, p.nH, p.Lq, 64), 1, 4)[:4])
    assert torch.equal(new["K"], aligned["K"]) and torch.equal(new["Vt"], aligned["Vt"])


# ----------------------------------------------------------------------------------------------------------------- attention
def _attn_operands(B, nH, Lq, Lk, split=False):
    torch.manual_seed(B * 100 + nH * 10 + Lq)
    Lp = (Lk + 63) // 64 * 64

    def bits(t):
        hi = to_bf16_bits(t)
        lo = to_bf16_bits(t - util.from_bf16_bits(hi))
        return dev(hi), dev(lo)

    q, k = torch.randn(B, nH, Lq, 64) * 0.25, torch.randn(B, nH, Lk, 64)
    vt = torch.zeros(B, nH, 64, Lp)
    vt[..., :Lk] = torch.randn(B, nH, 64, Lk)
    return bits(q), bits(k), bits(vt), Lp


def _attn_run(wide, ops, B, nH, Lq, Lk, ldo, mask, split=False, impl=0):
    (Q, Ql), (K, Kl), (Vt, Vl), Lp = ops
    Od = _sentinel((B * Lq + 40, ldo), 11)   # 40 rows behind the last one: a last tile's rows >= Lq would land there
    Ol = _sentinel((B * Lq + 40, ldo), 12)
    iv = None
    if mask == "interval":  # row (b, q) sees keys [lo, Lk): text rows right of a pad run, then the image block
        ivh = torch.zeros(B, Lq, 4, dtype=torch.int32)
        for b in range(B):
            ivh[b, :, 0] = (7 * b + 3) % max(1, Lk - Lq + 1)
            ivh[b, :, 1] = Lk
        iv = ivh.cuda()
    p = L().ptr
    L().call("showo_attn_set_wide_stores", wide)
    L().call("showo_attn_set_impl", impl)
    try:
        if split:
            L().call("showo_attn_fwd_split", p(Q), p(Ql), p(K), p(Kl), p(Vt), p(Vl), p(iv) if iv is not None else None, None, None, p(Od), p(Ol),
                     B, nH, Lq, Lk, Lk, Lp, ldo, S())
        else:
            L().call("showo_attn_fwd", p(Q), p(K), p(Vt), p(iv) if iv is not None else None, None, None, p(Od), B, nH, Lq, Lk, Lk, Lp, ldo, S())
        torch.cuda.synchronize()
    finally:
        L().call("showo_attn_set_impl", 0)
        L().call("showo_attn_set_wide_stores", -1)
    return Od, Ol


def _attn_check(old, new, B, nH, Lq, ldo, split):
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])
    for t, seed in ((new[0], 11), (new[1], 12)):
        ref = _sentinel((B * Lq + 40, ldo), seed).view(-1, ldo)
        t = t.view(-1, ldo)
        if seed == 12 and not split:
            assert torch.equal(t, ref)
            continue
        assert torch.equal(t[B * Lq:], ref[B * Lq:]), "rows past Lq were written"
        assert torch.equal(t[:, nH * 64:], ref[:, nH * 64:]), "the pad between rows was written"
        assert float((t[:B * Lq, :nH * 64] != ref[:B * Lq, :nH * 64]).float().mean()) > 0.99


@pytest.mark.parametrize("mask", ["causal", "interval"])
@pytest.mark.parametrize("pad", [0, 8, 4])  # ldo = nH 64 (+ 8: wide, sentinel between rows; + 4: the 8-byte form is taken)
@pytest.mark.parametrize("B,nH,Lq,Lk,impl", [(2, 2, 258, 387, 0), (1, 1, 33, 33, 0), (1, 1, 33, 33, 2)])
def test_attention_wide_stores_equal_narrow_stores(B, nH, Lq, Lk, impl, pad, mask):
    """impl 0 = by shape (Lq 258: the LDS-tiled kernel; Lq 33: the gather form), impl 2 = the LDS-tiled kernel at Lq 33, whose last
    tile has 31 rows past Lq"""
    ldo = nH * 64 + pad
    ops = _attn_operands(B, nH, Lq, Lk)
    old = _attn_run(0, ops, B, nH, Lq, Lk, ldo, mask, impl=impl)
    new = _attn_run(1, ops, B, nH, Lq, Lk, ldo, mask, impl=impl)
    _attn_check(old, new, B, nH, Lq, ldo, False)


@pytest.mark.parametrize("pad", [8, 4])
def test_attention_split_instance_wide_stores_equal_narrow_stores(pad):
    B, nH, Lq, Lk = 2, 2, 258, 387
    ldo = nH * 64 + pad
    ops = _attn_operands(B, nH, Lq, Lk)
    old = _attn_run(0, ops, B, nH, Lq, Lk, ldo, "interval", split=True)
    new = _attn_run(1, ops, B, nH, Lq, Lk, ldo, "interval", split=True)
    _attn_check(old, new, B, nH, Lq, ldo, True)
