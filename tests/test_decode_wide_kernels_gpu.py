"""GPU tests of the two MFMA skinny GEMMs of the wide decode step (csrc/decode_wide.hip), through their hooks
showo_decode_wide_ln_gemm / showo_decode_wide_out_gemm.

An MFMA's accumulation order belongs to the hardware, so nothing here compares against the dot2 kernels' bits.  What IS exact is
checked exactly (integer operands: every partial sum is an integer below 2^24, exact in fp32 in ANY order; one-hot weight rows: the
output is one LayerNorm value), and the random-operand cases are held to the worst-case bound of an fp32 sum of K exact products in
any order, which is derived and not measured."""
import functools

import pytest
import torch

import util
from util import O, dev

pytestmark = pytest.mark.gpu

NBS = [1, 9, 16, 17, 32]
EPS = 1e-5
# |gelu_new_fast(x) - gelu_new(x)| <= GELU_FAST_REL * |gelu_new(x)| + GELU_FAST_ABS: common.h's x * rcp(1 + exp2(x * p)) on v_exp_f32 /
# v_rcp_f32 against fp64 gelu_new (in its cancellation-free form x / (1 + exp(-2u)); the tanh form loses the far negative tail in
# fp64 itself), MEASURED on an MI355X over the grid x = -24 .. 24 in steps of 2^-10 (49 153 points): worst relative error 1.042e-5
# (at x = -9.02; 7.18e-6 for |x| <= 8: the rounding of the exponent's argument grows with |x|), worst absolute error 5.07e-7 (at
# x = 4.67, one fp32 ulp), and 8.8e-36 where |gelu_new| < 1e-30.  The constants are that measurement rounded up; no existing decode
# test states a figure for this function.  DESIGN.md ("Wide decode batches") records it.
GELU_FAST_REL = 1.1e-5
GELU_FAST_ABS = 1e-35


def L():
    return util.lib()


def S():
    return L().stream()


def _bits(t):
    return util.to_bf16_bits(t)


def _layernorm_bits(x, w, b):
    """showo_layernorm_f32_op16's bf16 output (int16 bits) of the fp32 rows x"""
    rows, H = x.shape
    y = torch.empty((rows, H), dtype=torch.int16, device="cuda")
    L().call("showo_layernorm_f32_op16", L().ptr(x), L().ptr(w), L().ptr(b), L().ptr(y), None, rows, H, EPS, 0, S())
    torch.cuda.synchronize()
    return y


def _ints(shape, seed, lo=-3, hi=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, device="cuda").float()


# ---- 1. out-GEMM, exact ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _out_case(K0, K1, N):
    """integer operands for 32 rows and the exact result (fp64 holds these integers exactly: |sum| <= 9 (K0 + K1) + 9 < 2^24)"""
    Wd, W2 = _ints((N, K0), 1), _ints((N, K1), 2)
    attn, ffn = _ints((32, K0), 3), _ints((32, K1), 4)
    bd, b2, x = _ints((N,), 5), _ints((N,), 6), _ints((32, N), 7)
    want = x.double() + (attn.double() @ Wd.double().T + bd.double()) + (ffn.double() @ W2.double().T + b2.double())
    assert float(want.abs().max()) < 2 ** 24
    return dict(Wd=_bits(Wd), W2=_bits(W2), attn=_bits(attn), ffn=_bits(ffn), bd=bd, b2=b2, x=x, want=want.float())


def _out_gemm(c, x, attn, ffn, K0, K1, N, nb):
    L().call("showo_decode_wide_out_gemm", L().ptr(x), L().ptr(c["Wd"]), L().ptr(attn), L().ptr(c["bd"]), K0, L().ptr(c["W2"]), L().ptr(ffn),
             L().ptr(c["b2"]), K1, N, nb, S())
    torch.cuda.synchronize()


# (2048, 8192, 48): two column groups only, the second half empty -- the K split over waves and blocks is still exercised
# (576, 2080) and (1536, 4640): K ends inside a 512-element span / a 2048-element chunk, within the kernel's K % 32 rule
@pytest.mark.parametrize("shape", [(128, 256, 128), (576, 2080, 128), (1536, 4640, 128), (2048, 8192, 2048), (2048, 8192, 48)])
@pytest.mark.parametrize("nb", NBS)
def test_out_gemm_is_exact_on_integer_operands(nb, shape):
    K0, K1, N = shape
    c = _out_case(K0, K1, N)
    x = c["x"].clone()
    _out_gemm(c, x, c["attn"], c["ffn"], K0, K1, N, nb)
    assert torch.equal(x[:nb], c["want"][:nb]), float((x[:nb] - c["want"][:nb]).abs().max())
    assert torch.equal(x[nb:], c["x"][nb:])  # rows >= nb are not touched
    y = c["x"].clone()  # a second launch finds the ticket words re-armed
    _out_gemm(c, y, c["attn"], c["ffn"], K0, K1, N, nb)
    assert torch.equal(y, x)


# ---- 2. ln-GEMM, indexing -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ln_rows(H):
    g = torch.Generator(device="cuda").manual_seed(100 + H)
    x = torch.randn((32, H), generator=g, device="cuda") * 2 + 0.3
    w = torch.randn((H,), generator=g, device="cuda") * 0.1 + 1
    b = torch.randn((H,), generator=g, device="cuda") * 0.05
    return x, w, b, _layernorm_bits(x, w, b)


@functools.lru_cache(maxsize=None)
def _one_hot(N, H):
    W = torch.zeros((N, H), dtype=torch.float32, device="cuda")
    k = (7 * torch.arange(N, device="cuda") + 3) % H
    W[torch.arange(N, device="cuda"), k] = 1.0
    return _bits(W), k, torch.zeros((N,), dtype=torch.float32, device="cuda")


def _check_one_hot(H, N, nb):
    x, w, b, hbits = _ln_rows(H)
    W, k, zero = _one_hot(N, H)
    out = torch.full((32, N), -777.0, dtype=torch.float32, device="cuda")
    L().call("showo_decode_wide_ln_gemm", L().ptr(x), L().ptr(w), L().ptr(b), EPS, H, L().ptr(W), L().ptr(zero), None, L().ptr(out), N, N,
             None, None, None, 0, 0, nb, S())
    torch.cuda.synchronize()
    want = util.from_bf16_bits(hbits)[:, k]  # [32, N]: output (b, n) is LayerNorm value (b, (7 n + 3) mod H)
    assert torch.equal(out[:nb], want[:nb]), (H, N, nb)
    assert (out[nb:] == -777.0).all()


@pytest.mark.parametrize("N", [439, 642])
@pytest.mark.parametrize("H", [128, 576, 2048])
@pytest.mark.parametrize("nb", NBS)
def test_ln_gemm_one_hot_rows_return_the_layernorm_bits(nb, H, N):
    _check_one_hot(H, N, nb)


# A block of ln_gemmW_kernel is 4 waves of 32 columns and the default grid cap ("wide_ln_blocks") is 256 blocks: one trip of the
# whole grid covers 256 * 4 * 32 = 32 768 columns.  N = 2 * 32 768 + 23 gives every wave at least two trips of its column loop, a
# third to some, and a last tile of 7 columns.
@pytest.mark.parametrize("nb", [9, 32])
def test_ln_gemm_one_hot_rows_over_several_trips_of_the_column_loop(nb):
    _check_one_hot(128, 2 * 32768 + 23, nb)


# ---- 3. ln-GEMM, values ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _value_case(H, N0, N1):
    x, w, b, hbits = _ln_rows(H)
    g = torch.Generator(device="cuda").manual_seed(7 * H + N0)
    W0 = util.bf16_round(torch.randn((N0, H), generator=g, device="cuda") / H ** 0.5)
    W1 = util.bf16_round(torch.randn((N1, H), generator=g, device="cuda") / H ** 0.5)
    b0 = torch.randn((N0,), generator=g, device="cuda") * 0.1
    b1 = torch.randn((N1,), generator=g, device="cuda") * 0.1
    h = util.from_bf16_bits(hbits).double()
    # fp64 product of the SAME bf16 operands; mag = sum_k |a_k w_k| per output
    e0, e1 = h @ W0.double().T + b0.double(), h @ W1.double().T + b1.double()
    m0, m1 = h.abs() @ W0.double().abs().T, h.abs() @ W1.double().abs().T
    return dict(x=x, w=w, b=b, W0=_bits(W0), W1=_bits(W1), b0=b0, b1=b1, e0=e0, e1=e1, m0=m0, m1=m1)


def _bf16_ulp(v):
    """one bf16 ulp of the (fp64) value v: 2^(floor(log2 |v|) - 7)"""
    _, e = torch.frexp(v.abs().clamp(min=2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 8)


@pytest.mark.parametrize("dims", [(128, 384, 256), (2048, 6144, 8192)])
@pytest.mark.parametrize("nb", NBS)
def test_ln_gemm_values_within_the_any_order_bound(nb, dims):
    H, N0, N1 = dims
    c = _value_case(H, N0, N1)
    out0 = torch.full((32, N0), 0x7fc1, dtype=torch.int16, device="cuda")
    out1 = torch.full((32, N1), 0x7fc1, dtype=torch.int16, device="cuda")
    outf = torch.full((32, N0), -777.0, dtype=torch.float32, device="cuda")
    out1f = torch.full((32, N1), 0x7fc1, dtype=torch.int16, device="cuda")
    common = (L().ptr(c["x"]), L().ptr(c["w"]), L().ptr(c["b"]), EPS, H, L().ptr(c["W0"]), L().ptr(c["b0"]))
    tail = (N0, N0, L().ptr(c["W1"]), L().ptr(c["b1"]))
    L().call("showo_decode_wide_ln_gemm", *common, L().ptr(out0), None, *tail, L().ptr(out1), N1, N1, nb, S())
    L().call("showo_decode_wide_ln_gemm", *common, None, L().ptr(outf), *tail, L().ptr(out1f), N1, N1, nb, S())
    torch.cuda.synchronize()
    # worst case of an fp32 sum of K exact products in any order, per-operation error <= 2 ulp-halves: 2 K 2^-24 sum_k |a_k w_k|
    bound0, bound1 = 2 * H * 2.0 ** -24 * c["m0"][:nb], 2 * H * 2.0 ** -24 * c["m1"][:nb]
    e0, e1 = c["e0"][:nb], c["e1"][:nb]
    err_f = (outf[:nb].double() - e0).abs()
    err_b = (util.from_bf16_bits(out0[:nb]).double() - e0).abs()
    g = O.gelu_new(e1)
    gel = util.from_bf16_bits(out1[:nb]).double()
    err_g = (gel - g).abs()
    bound_g = 1.13 * bound1 + _bf16_ulp(g) + GELU_FAST_REL * g.abs() + GELU_FAST_ABS
    print(f"[parity] wide ln_gemm nb={nb} H={H} N0={N0} N1={N1}: worst err / bound fp32 {float((err_f / bound0).max()):.3f}, "
          f"bf16 {float((err_b / (bound0 + _bf16_ulp(e0))).max()):.3f}, gelu {float((err_g / bound_g).max()):.3f} "
          f"(gelu_new_fast vs gelu_new: {GELU_FAST_REL:g} relative + {GELU_FAST_ABS:g}, measured on a grid)")
    assert (err_f <= bound0).all()
    assert (err_b <= bound0 + _bf16_ulp(e0)).all()
    assert (err_g <= bound_g).all()
    assert torch.equal(out1f, out1)  # the gelu half does not depend on the form of the other output
    assert (out0[nb:] == 0x7fc1).all() and (out1[nb:] == 0x7fc1).all() and (outf[nb:] == -777.0).all()


# ---- 4. row hygiene -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", NBS)
def test_rows_beyond_nb_are_neither_read_nor_written(nb):
    # out-GEMM: NaN activation rows and residual rows >= nb
    K0, K1, N = 128, 256, 128
    c = _out_case(K0, K1, N)
    nan16 = torch.full((1,), float("nan")).to(torch.bfloat16).view(torch.int16).item()
    attn, ffn, x = c["attn"].clone(), c["ffn"].clone(), c["x"].clone()
    attn[nb:], ffn[nb:], x[nb:] = nan16, nan16, float("nan")
    _out_gemm(c, x, attn, ffn, K0, K1, N, nb)
    assert torch.equal(x[:nb], c["want"][:nb])
    assert torch.isnan(x[nb:]).all()
    # ln-GEMM: NaN residual rows >= nb; sentinels in every output
    H, N0, N1 = 128, 384, 256
    v = _value_case(H, N0, N1)
    outs = []
    for poison in (False, True):
        xx = v["x"].clone()
        if poison:
            xx[nb:] = float("nan")
        out0 = torch.full((32, N0), 0x7fc1, dtype=torch.int16, device="cuda")
        out1 = torch.full((32, N1), 0x7fc1, dtype=torch.int16, device="cuda")
        L().call("showo_decode_wide_ln_gemm", L().ptr(xx), L().ptr(v["w"]), L().ptr(v["b"]), EPS, H, L().ptr(v["W0"]), L().ptr(v["b0"]),
                 L().ptr(out0), None, N0, N0, L().ptr(v["W1"]), L().ptr(v["b1"]), L().ptr(out1), N1, N1, nb, S())
        torch.cuda.synchronize()
        assert (out0[nb:] == 0x7fc1).all() and (out1[nb:] == 0x7fc1).all()
        outs.append((out0, out1))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
