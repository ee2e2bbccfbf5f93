"""GPU tests of the dot2 GEMV kernels every default mmu decode step runs (csrc/decode.hip ln_gemv2_kernel / out_gemv2_kernel,
csrc/decode_batch.hip ln_gemvB_kernel / out_gemvB_kernel / out_dense_y2B_kernel, the pieces of csrc/decode_common.h), through their
hooks showo_decode_narrow_ln_gemv / showo_decode_narrow_out_gemv.

Position k of a weight row belongs to lane (k % 512) / 8, sub-span u = (k % 2048) / 512 and chunk t = k / 2048; the shapes below are
the smallest that end a row inside a sub-span (576), 8 elements into one (1544: lane 0 of u = 3 only), 8 elements into a chunk
(2056, 6152) and at every chunk count C = 2..5 (C = 1..4 of the fc2-only mode).  Tiers: exact on integers (out kernels), one-hot
indexing (ln kernels), the bits of the general layer (showo_layernorm_f32_op16 + showo_gemm_op16), values against fp64 within the
derived any-order bound of tests/test_decode_wide_kernels_gpu.py, refusals.  Hygiene rides on every launch: activation / residual
rows >= nb hold NaN, every operand row is followed by NaN-filled slack (a read past a row's end turns the output into NaN instead of
faulting), every output has sentinel rows and sentinel padding behind ld that must stay put."""
import functools

import pytest
import torch

import util
from util import O
from test_decode_wide_kernels_gpu import EPS, GELU_FAST_ABS, GELU_FAST_REL, L, S

pytestmark = pytest.mark.gpu

FORMS = ["bf16", "fp16", "int8"]
HS = {"bf16": [128, 576, 1544, 2048], "fp16": [128, 576, 1544, 2048], "int8": [128, 576, 1552, 2048]}
SHAPES = [(128, 256), (576, 576), (576, 2056), (1544, 4616), (2048, 6152), (2048, 8192)]       # C = 2, 2, 3, 4, 5, 5
SHAPES_Q8 = [(128, 256), (576, 576), (576, 2064), (1552, 4624), (2048, 6160), (2048, 8192)]    # the int8 forms' K % 16
NS = [1, 130, 439]
MAXB = 8
SENT16 = 0x7fc1   # a NaN of both 16-bit types: poison of operands, sentinel of 16-bit outputs
SENTF = -777.0
SLACK = 64        # elements of poison behind every operand


def _op(form):
    return 1 if form == "fp16" else 0


def _t16(op):
    return torch.float16 if op else torch.bfloat16


def _bits(t, op=0):
    return t.to(_t16(op)).view(torch.int16)


def _vals(bits, op=0):
    return bits.view(_t16(op)).float()


def _ints(shape, seed, lo=-3, hi=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, device="cuda").float()


def _randn(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda")


def _padded(t, rows, ld, fill):
    """flat buffer of rows * ld + SLACK elements of `fill` holding the 2-D tensor t in its top left corner"""
    r, k = t.shape
    buf = torch.full((rows * ld + SLACK,), fill, dtype=t.dtype, device="cuda")
    buf[:rows * ld].view(rows, ld)[:r, :k] = t
    return buf


def _wbuf(W, q8=False):
    """contiguous weight rows [N, K] with poison behind the last row (int8: 127, no NaN exists)"""
    return _padded(W, W.shape[0], W.shape[1], 127 if q8 else SENT16)


def _fbuf(v):
    """fp32 vector with NaN slack"""
    return _padded(v[None], 1, v.shape[0], float("nan"))


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


class Knobs:
    """showo_decode_set_tuning for the duration of a with-block (defaults: csrc/engine.h DecodeTuning)"""
    DEFAULT = {"ln_blocks": 1024, "batch_ln_blocks": 1024, "out_blocks": 256}

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            L().call("showo_decode_set_tuning", k.encode(), v)

    def __exit__(self, *exc):
        for k in self.kw:
            L().call("showo_decode_set_tuning", k.encode(), self.DEFAULT[k])


# ---- launch helpers -------------------------------------------------------------------------------------------------------------
def _out_call(kernel, nb, mode, op, c, N, x=None, y2=None, rows=None, check=True):
    """one launch of the out hook on case c (operands of MAXB rows, N columns).  rows: which case rows feed slots 0..nb-1.  x / y2:
    [MAXB, N] tensors (kernel 0: row 0 is the launch's row); returns (x, y2) buffers as [MAXB, N] views after the launch."""
    rows = list(range(nb)) if rows is None else rows
    K0, K1 = c["K0"], c["K1"]
    lda0, lda1 = (K0, K1) if kernel == 0 else (K0 + 8, K1 + 24)
    a0 = _padded(c["a0"][rows], MAXB, lda0, SENT16)
    a1 = _padded(c["a1"][rows], MAXB, lda1, SENT16)
    xb = None if x is None else _padded(x, MAXB, N, float("nan"))
    yb = None if y2 is None else _padded(y2, MAXB, N, float("nan"))
    p = L().ptr
    rc = getattr(L().load(), "showo_decode_narrow_out_gemv")(
        kernel, nb, mode, op, p(xb), p(c["W0"]), p(a0), p(c["s0"]), p(c["b0"]), K0, lda0, p(c["W1"]), p(a1), p(c["s1"]), p(c["b1"]), K1, lda1, N,
        p(yb), S())
    if check:
        L().check(rc, "showo_decode_narrow_out_gemv")
    torch.cuda.synchronize()
    view = lambda b: None if b is None else b[:MAXB * N].view(MAXB, N)
    if check:
        for b in (xb, yb):
            assert b is None or torch.isnan(b[MAXB * N:]).all()
    return (view(xb), view(yb)) if check else rc


@functools.lru_cache(maxsize=2)
def _int_master(K0, K1, form):
    """integer operands for MAXB rows and 439 columns.  bf16 / fp16: everything in [-3, 3].  int8: weights in [-127, 127] with scales in
    {1/2, 1, 2}.  `mag` bounds every partial sum of every evaluation order (sum of |terms|); the exactness argument needs the
    accumulators (integers) below 2^24 and the scaled sums (multiples of 1/2) below 2^23."""
    q8 = form == "int8"
    N = NS[-1]
    wl = 127 if q8 else 3
    W0, W1 = _ints((N, K0), 1, -wl, wl), _ints((N, K1), 2, -wl, wl)
    a0, a1 = _ints((MAXB, K0), 3), _ints((MAXB, K1), 4)
    b0, b1, x = _ints((N,), 5), _ints((N,), 6), _ints((MAXB, N), 7)
    s0 = 2.0 ** _ints((N,), 8, -1, 1) if q8 else torch.ones((N,), device="cuda")
    s1 = 2.0 ** _ints((N,), 9, -1, 1) if q8 else torch.ones((N,), device="cuda")
    D = lambda t: t.double()
    d = (D(a0) @ D(W0).T) * D(s0) + D(b0)
    f = (D(a1) @ D(W1).T) * D(s1) + D(b1)
    m0, m1 = D(a0).abs() @ D(W0).abs().T, D(a1).abs() @ D(W1).abs().T
    assert float(torch.maximum(m0, m1).max()) < 2 ** 24
    mag = D(x).abs() + m0 * D(s0) + D(b0).abs() + m1 * D(s1) + D(b1).abs()
    assert float(mag.max()) < (2 ** 23 if q8 else 2 ** 24)
    return dict(W0=W0, W1=W1, a0=a0, a1=a1, b0=b0, b1=b1, x=x, s0=s0, s1=s1, d=d, f=f, q8=q8)


def _int_case(K0, K1, form, N):
    m, op, q8 = _int_master(K0, K1, form), _op(form), form == "int8"
    wb = (lambda W: _wbuf(W.to(torch.int8), True)) if q8 else (lambda W: _wbuf(_bits(W, op)))
    return dict(K0=K0, K1=K1, W0=wb(m["W0"][:N]), W1=wb(m["W1"][:N]), a0=_bits(m["a0"], op), a1=_bits(m["a1"], op), b0=_fbuf(m["b0"][:N]),
                b1=_fbuf(m["b1"][:N]), s0=_fbuf(m["s0"][:N]) if q8 else None, s1=_fbuf(m["s1"][:N]) if q8 else None,
                x=m["x"][:, :N].contiguous(), y2=m["f"][:, :N].float().contiguous(),
                want=(m["x"][:, :N].double() + m["d"][:, :N] + m["f"][:, :N]).float().contiguous())


def _nan_rows(t, nb):
    t = t.clone()
    t[nb:] = float("nan")
    return t


# ---- 1. out kernels, exact on integers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_out_kernels_are_exact_on_integer_operands(shape, form):
    """every (K0, K1) of the table, N = 1 / 130 / 439: out_gemvB at nb = 1..8, out_gemv2 in modes 0, 1, 2 (mode 1 at K1 = 256, 576,
    2056, 4616, 6152, 8192: C = 1, 1, 2, 3 on the <3, 1> instance, 4, 4 on <4, 1>), out_dense_y2B at nb = 2..4.  fp32 holds every
    partial sum exactly, so the result is the fp64 result bit for bit in any order; rows >= nb keep their (NaN) bits."""
    K0, K1 = (SHAPES_Q8 if form == "int8" else SHAPES)[shape]
    op = _op(form)
    for N in NS:
        c = _int_case(K0, K1, form, N)
        for nb in range(1, MAXB + 1):
            x0 = _nan_rows(c["x"], nb)
            x, _ = _out_call(1, nb, 0, op, c, N, x=x0)
            assert torch.equal(x[:nb], c["want"][:nb]), (K0, K1, N, nb, float((x[:nb] - c["want"][:nb]).abs().max()))
            assert _same_bits(x[nb:], x0[nb:])
            y, _ = _out_call(1, nb, 0, op, c, N, x=x0)  # a second launch on fresh x
            assert _same_bits(y, x)
        for nb in (2, 3, 4):
            x0, y0 = _nan_rows(c["x"], nb), _nan_rows(c["y2"], nb)
            x, y2 = _out_call(2, nb, 2, op, c, N, x=x0, y2=y0)
            assert torch.equal(x[:nb], c["want"][:nb]), (K0, K1, N, nb)
            assert _same_bits(x[nb:], x0[nb:]) and _same_bits(y2, y0)
        for r in (0, MAXB - 1):  # the batch-1 kernel on the first and the last row of the case
            x0, y0 = _nan_rows(c["x"][r:r + 1], 1), _nan_rows(c["y2"][r:r + 1], 1)
            x, _ = _out_call(0, 1, 0, op, c, N, x=x0, rows=[r])
            assert torch.equal(x[0], c["want"][r]), (K0, K1, N, r)
            assert torch.isnan(x[1:]).all()
            x, _ = _out_call(0, 1, 0, op, c, N, x=x0, rows=[r])
            assert torch.equal(x[0], c["want"][r])
            _, y2 = _out_call(0, 1, 1, op, c, N, y2=torch.full_like(y0, float("nan")), rows=[r])
            assert torch.equal(y2[0], c["y2"][r]) and torch.isnan(y2[1:]).all(), (K0, K1, N, r)
            x, yk = _out_call(0, 1, 2, op, c, N, x=x0, y2=y2, rows=[r])
            assert torch.equal(x[0], c["want"][r]) and torch.isnan(x[1:]).all() and _same_bits(yk, y2)


# ---- LayerNorm operands and the ln launch ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ln_rows(H, op):
    x = _randn((MAXB, H), 100 + H) * 2 + 0.3
    w = _randn((H,), 200 + H) * 0.1 + 1
    b = _randn((H,), 300 + H) * 0.05
    y = torch.empty((MAXB, H), dtype=torch.int16, device="cuda")
    L().call("showo_layernorm_f32_op16", L().ptr(x), L().ptr(w), L().ptr(b), L().ptr(y), None, MAXB, H, EPS, op, S())
    torch.cuda.synchronize()
    return x, _fbuf(w), _fbuf(b), y


def _ln_call(kernel, nb, op, H, W0, b0, N0, f32, W1=None, b1=None, N1=0, W0lo=None, s0=None, s1=None, rows=None, check=True, x=None):
    """one launch of the ln hook on rows `rows` of _ln_rows(H, op).  Returns (out0 or outf [nb, N0], out1 [nb, N1] or None)."""
    rows = list(range(nb)) if rows is None else rows
    xr, w, b, _ = _ln_rows(H, op if op in (0, 1) else 0)  # (the refusal cases pass operand types that do not exist)
    xb = _padded(xr[rows] if x is None else x, MAXB, H, float("nan"))
    ld0, ld1 = N0 + 5, N1 + 3
    o0 = torch.full((MAXB * ld0,), SENTF if f32 else SENT16, dtype=torch.float32 if f32 else torch.int16, device="cuda")
    o1 = torch.full((MAXB * ld1,), SENT16, dtype=torch.int16, device="cuda") if N1 else None
    p = L().ptr
    rc = getattr(L().load(), "showo_decode_narrow_ln_gemv")(
        kernel, nb, op, p(xb), p(w), p(b), EPS, H, p(W0), p(W0lo), p(s0), p(b0), None if f32 else p(o0), p(o0) if f32 else None, N0, ld0,
        p(W1), p(s1), p(b1), p(o1), N1, ld1, S())
    if not check:
        torch.cuda.synchronize()
        return rc, o0, o1
    L().check(rc, "showo_decode_narrow_ln_gemv")
    torch.cuda.synchronize()

    def take(o, N, ld, sent):
        if o is None:
            return None
        if kernel == 0:  # one row, no leading dimension
            assert (o[N:] == sent).all()
            return o[:N][None].clone()
        v = o.view(MAXB, ld)
        assert (v[:nb, N:] == sent).all() and (v[nb:] == sent).all()
        return v[:nb, :N].clone()

    return take(o0, N0, ld0, SENTF if f32 else SENT16), take(o1, N1, ld1, SENT16)


# ---- 2. ln kernels, indexing ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_hot(N, H, op):
    W = torch.zeros((N, H), dtype=torch.float32, device="cuda")
    n = torch.arange(N, device="cuda")
    k = (7 * n + 3) % H
    W[n, k] = 1.0
    return _wbuf(_bits(W, op)), k, _fbuf(torch.zeros((N,), device="cuda")), _wbuf(torch.zeros((N, H), dtype=torch.int16, device="cuda"))


def _check_one_hot(H, N, form, nbs=range(1, MAXB + 1), split=False):
    op = _op(form)
    W, k, zero, Wzero = _one_hot(N, H, op)
    want = _vals(_ln_rows(H, op)[3], op)[:, k]  # output (b, n) is LayerNorm value (b, (7 n + 3) mod H)
    for nb in nbs:
        if split:  # hi . 0 + lo . 0 + hi . e_k: the bf16 LayerNorm value
            got, _ = _ln_call(1, nb, 0, H, Wzero, zero, N, True, W0lo=W)
        else:
            got, _ = _ln_call(1, nb, op, H, W, zero, N, True)
        assert torch.equal(got, want[:nb]), (H, N, form, nb, split)
    if not split:
        for r in (0, MAXB - 1):
            got, _ = _ln_call(0, 1, op, H, W, zero, N, True, rows=[r])
            assert torch.equal(got[0], want[r]), (H, N, form, r)


@pytest.mark.parametrize("form", ["bf16", "fp16"])
@pytest.mark.parametrize("H", HS["bf16"])
def test_ln_one_hot_rows_return_the_layernorm_bits(H, form):
    for N in NS:
        _check_one_hot(H, N, form)


@pytest.mark.parametrize("H", HS["bf16"])
def test_split_head_one_hot_low_rows_return_the_bf16_layernorm_bits(H):
    for N in NS:
        _check_one_hot(H, N, "bf16", split=True)


def test_ln_one_hot_rows_over_several_trips_of_the_column_loop():
    """3 blocks: 12 waves x 2 rows in flight = 24 columns per trip of ln_gemv2_kernel / ln_gemvB_kernel<NB <= 4>, 19 trips for N = 439 (the
    last one partial).  The LDS forms (NB >= 5, split head) have a fixed cap of 1280 blocks: 37 blocks at N = 439, two trips."""
    with Knobs(ln_blocks=3, batch_ln_blocks=3):
        for H in (128, 1544):
            _check_one_hot(H, 439, "bf16")
            _check_one_hot(H, 439, "bf16", split=True)
        _check_one_hot(576, 439, "fp16")


@pytest.mark.parametrize("form", ["bf16", "fp16"])
def test_ln_one_hot_rows_at_a_vocabulary_sized_n_under_the_default_caps(form):
    """N = 58 498 at H = 128: 1024 blocks x 4 waves x 2 rows = 8192 columns per trip (1280 blocks: 10 240), 6-8 trips, a partial last"""
    _check_one_hot(128, 58498, form, nbs=(1, 4, 5, 8))
    if form == "bf16":
        _check_one_hot(128, 58498, form, nbs=(1, 8), split=True)


# ---- 3. the bits of the general layer -------------------------------------------------------------------------------------------
def _pad64(bits):
    """[r, K] -> [r, K64] with zeros behind K: showo_gemm_op16 takes K % 64 == 0 only.  The padding adds products that are exactly +0
    to the same accumulator chains (the GEMV form's lane split is the decode kernels': k -> lane (k % 512) / 8, u and chunk ascending),
    so the padded call has the bits of the K-element sum."""
    r, K = bits.shape
    out = torch.zeros((r, (K + 63) // 64 * 64), dtype=torch.int16, device="cuda")
    out[:, :K] = bits
    return out


def _gemm(A, W, bias, out, resid, M, N, epi, op):
    p = L().ptr
    L().call("showo_gemm_op16", p(A), A.shape[1], p(W), W.shape[1], p(bias), 0, p(out), N, p(resid), N, M, N, A.shape[1], epi, op, S())


@functools.lru_cache(maxsize=None)
def _rand_mats(K, N, op, seed):
    return _bits(_randn((N, K), seed) / K ** 0.5, op)


@pytest.mark.parametrize("form", ["bf16", "fp16"])
@pytest.mark.parametrize("H", [576, 1544, 2048])
def test_ln_kernels_give_the_bits_of_layernorm_plus_gemm(H, form):
    op = _op(form)
    N0, N1 = 439, 130
    W0, W1 = _rand_mats(H, N0, op, 11), _rand_mats(H, N1, op, 12)
    b0, b1 = _randn((N0,), 13) * 0.1, _randn((N1,), 14) * 0.1
    h = _pad64(_ln_rows(H, op)[3])
    ref16 = torch.empty((MAXB, N0), dtype=torch.int16, device="cuda")
    reff = torch.empty((MAXB, N0), dtype=torch.float32, device="cuda")
    refg = torch.empty((MAXB, N1), dtype=torch.int16, device="cuda")
    _gemm(h, _pad64(W0), b0, ref16, None, MAXB, N0, 0, op)
    _gemm(h, _pad64(W0), b0, reff, None, MAXB, N0, 2, op)
    _gemm(h, _pad64(W1), b1, refg, None, MAXB, N1, 1, op)
    torch.cuda.synchronize()
    W0b, W1b, b0b, b1b = _wbuf(W0), _wbuf(W1), _fbuf(b0), _fbuf(b1)

    def run(kernel, nb, rows=None):
        o16, g1 = _ln_call(kernel, nb, op, H, W0b, b0b, N0, False, W1=W1b, b1=b1b, N1=N1, rows=rows)
        of, g2 = _ln_call(kernel, nb, op, H, W0b, b0b, N0, True, W1=W1b, b1=b1b, N1=N1, rows=rows)
        assert torch.equal(g1, g2)
        return o16, of, g1

    def check(kernel, nb, rows=None):
        idx = list(range(nb)) if rows is None else rows
        o16, of, g = run(kernel, nb, rows)
        assert torch.equal(o16, ref16[idx]) and torch.equal(of, reff[idx]) and torch.equal(g, refg[idx]), (H, form, kernel, nb, rows)

    for nb in (1, 3, 4, 5, 8):
        check(1, nb)
    check(1, 1, rows=[6])  # row b of an nb-slot launch equals the nb = 1 launch of that row: both equal the reference's row
    check(0, 1)
    check(0, 1, rows=[6])
    with Knobs(ln_blocks=6, batch_ln_blocks=6):  # 24 waves, 48 columns per trip: 12 trips
        for nb in (1, 4, 8):
            check(1, nb)
        check(0, 1)


@pytest.mark.parametrize("form", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(576, 576), (576, 2056), (1544, 4616), (2048, 6152)])
def test_out_kernels_give_the_bits_of_two_residual_gemms(shape, form):
    K0, K1 = shape
    op = _op(form)
    for N in (130, 439):
        W0, W1 = _rand_mats(K0, N, op, 21), _rand_mats(K1, N, op, 22)
        a0, a1 = _bits(_randn((MAXB, K0), 23), op), _bits(_randn((MAXB, K1), 24), op)
        b0, b1, x = _randn((N,), 25) * 0.1, _randn((N,), 26) * 0.1, _randn((MAXB, N), 27)
        ref = x.clone()
        _gemm(_pad64(a0), _pad64(W0), b0, ref, ref, MAXB, N, 3, op)
        _gemm(_pad64(a1), _pad64(W1), b1, ref, ref, MAXB, N, 3, op)
        torch.cuda.synchronize()
        c = dict(K0=K0, K1=K1, W0=_wbuf(W0), W1=_wbuf(W1), a0=a0, a1=a1, b0=_fbuf(b0), b1=_fbuf(b1), s0=None, s1=None)

        def sweep():
            for nb in (1, 3, 4, 5, 8):
                got, _ = _out_call(1, nb, 0, op, c, N, x=_nan_rows(x, nb))
                assert torch.equal(got[:nb], ref[:nb]), (shape, form, N, nb)
            for r in (0, 6):
                x0 = _nan_rows(x[r:r + 1].repeat(MAXB, 1), 1)
                got, _ = _out_call(1, 1, 0, op, c, N, x=x0, rows=[r])  # the nb = 1 launch of a row of the nb-slot launch
                assert torch.equal(got[0], ref[r])
                got, _ = _out_call(0, 1, 0, op, c, N, x=x0, rows=[r])
                assert torch.equal(got[0], ref[r]), (shape, form, N, r)
                _, y2 = _out_call(0, 1, 1, op, c, N, y2=torch.full_like(x0, float("nan")), rows=[r])
                got, _ = _out_call(0, 1, 2, op, c, N, x=x0, y2=y2, rows=[r])
                assert torch.equal(got[0], ref[r]), (shape, form, N, r)
            # the co-scheduled batched form: y2 rows from the fc2-only mode, then out_dense_y2B
            y2 = torch.full_like(x, float("nan"))
            for r in range(4):
                y2[r] = _out_call(0, 1, 1, op, c, N, y2=torch.full_like(x, float("nan")), rows=[r])[1][0]
            for nb in (2, 3, 4):
                got, _ = _out_call(2, nb, 2, op, c, N, x=_nan_rows(x, nb), y2=_nan_rows(y2, nb))
                assert torch.equal(got[:nb], ref[:nb]), (shape, form, N, nb)

        sweep()
        with Knobs(out_blocks=2):  # 16 waves: 9 / 28 columns per wave
            sweep()


# ---- 4. values against fp64 -----------------------------------------------------------------------------------------------------
def _ulp16(v, op):
    """one ulp of the 16-bit type at the (fp64) value v: 2^(floor(log2 |v|) - 7) for bf16, - 10 for fp16 (normal range)"""
    _, e = torch.frexp(v.abs().clamp(min=2.0 ** (-14 if op else -126)))
    return torch.ldexp(torch.ones_like(v), e - (11 if op else 8))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hi", range(4))
def test_ln_values_within_the_any_order_bound(hi, form):
    """ln kernels with both halves, every nb, against the fp64 product of the SAME rounded operands.  Bound: the worst case of an fp32 sum
    of K exact products in any order, 2 K 2^-24 sum_k |a_k w_k| (tests/test_decode_wide_kernels_gpu.py), times the row scale for the int8
    form (the scale multiplies the finished sum: one more rounding, inside the factor 2), plus one output ulp where the output is 16-bit;
    the gelu half adds |gelu_new'| <= 1.13 on the argument's bound and the stated error of gelu_new_fast."""
    H = HS[form][hi]
    op, q8 = _op(form), form == "int8"
    N0, N1 = 439, 130
    h = _vals(_ln_rows(H, op)[3], op).double()
    if q8:  # free scales: what the quantiser would give a weight row of this size, not a power of two
        W0, W1 = _ints((N0, H), 31, -127, 127), _ints((N1, H), 32, -127, 127)
        s0 = (torch.rand((N0,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(33)) + 0.5) / (127 * H ** 0.5)
        s1 = (torch.rand((N1,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(34)) + 0.5) / (127 * H ** 0.5)
        W0b, W1b = _wbuf(W0.to(torch.int8), True), _wbuf(W1.to(torch.int8), True)
    else:
        W0, W1 = _vals(_rand_mats(H, N0, op, 11), op), _vals(_rand_mats(H, N1, op, 12), op)
        s0, s1 = torch.ones((N0,), device="cuda"), torch.ones((N1,), device="cuda")
        W0b, W1b = _wbuf(_bits(W0, op)), _wbuf(_bits(W1, op))
    b0, b1 = _randn((N0,), 13) * 0.1, _randn((N1,), 14) * 0.1
    e0 = (h @ W0.double().T) * s0.double() + b0.double()
    e1 = (h @ W1.double().T) * s1.double() + b1.double()
    bound0 = 2 * H * 2.0 ** -24 * (h.abs() @ W0.double().abs().T) * s0.double()
    bound1 = 2 * H * 2.0 ** -24 * (h.abs() @ W1.double().abs().T) * s1.double()
    g = O.gelu_new(e1)
    bound_g = 1.13 * bound1 + _ulp16(g, op) + GELU_FAST_REL * g.abs() + GELU_FAST_ABS
    sb, s0b, s1b = (_fbuf(b0), _fbuf(b1)), _fbuf(s0) if q8 else None, _fbuf(s1) if q8 else None
    worst = [0.0, 0.0, 0.0]
    for kernel, nb in [(0, 1)] + [(1, n) for n in range(1, MAXB + 1)]:
        kw = dict(W1=W1b, b1=sb[1], N1=N1, s0=s0b, s1=s1b)
        o16, g1 = _ln_call(kernel, nb, op, H, W0b, sb[0], N0, False, **kw)
        of, g2 = _ln_call(kernel, nb, op, H, W0b, sb[0], N0, True, **kw)
        assert torch.equal(g1, g2)  # the gelu half does not depend on the form of the other output
        ef = (of.double() - e0[:nb]).abs() / bound0[:nb]
        e16 = (_vals(o16, op).double() - e0[:nb]).abs() / (bound0[:nb] + _ulp16(e0[:nb], op))
        eg = (_vals(g1, op).double() - g[:nb]).abs() / bound_g[:nb]
        worst = [max(worst[0], float(ef.max())), max(worst[1], float(e16.max())), max(worst[2], float(eg.max()))]
        assert (ef <= 1).all() and (e16 <= 1).all() and (eg <= 1).all(), (H, form, kernel, nb, float(ef.max()), float(e16.max()), float(eg.max()))
    print(f"[parity] narrow ln_gemv {form} H={H} N0={N0} N1={N1}: worst err / bound fp32 {worst[0]:.3f}, 16-bit {worst[1]:.3f}, "
          f"gelu {worst[2]:.3f}")


@pytest.mark.parametrize("H", HS["bf16"])
def test_split_head_values_within_the_bound_of_three_products(H):
    """HEAD3: acc = hi.Whi + lo.Whi + hi.Wlo in one fp32 chain of 3 H products, for the row y ~ hi + lo and the weight W = Whi + Wlo.
    Operands: hi = the bf16 LayerNorm bits (showo_layernorm_f32_op16; the one-hot tier shows the kernel holds exactly these), Whi / Wlo
    = the bf16 halves of an fp32 matrix.  lo is not observable through any entry point of its own, so it is read back through one-hot
    hi rows: that launch returns fl32(hi + lo), i.e. lo up to one fp32 rounding, |dlo| <= 2^-24 |hi + lo|.  Reference: the fp64 product
    (hi + lo')(Whi + Wlo) + b with lo' = that read-back minus hi.  Bound, term by term:
      2 (3 H) 2^-24 sum(|hi Whi| + |lo' Whi| + |hi Wlo|)   any-order fp32 sum of the 3 H products the kernel forms
      + sum |lo' Wlo|                                      the product the kernel drops by design
      + 2^-24 sum |hi + lo'| |Whi|                         the read-back's rounding, through the lo.Whi products.
    |lo'| <= 2^-8 |hi| is asserted too (a low half of a bf16 split is at most half an ulp of hi)."""
    N = 439
    W = _randn((N, H), 41) / H ** 0.5
    Whi = util.bf16_round(W)
    Wlo = util.bf16_round(W - Whi)
    b = _randn((N,), 42) * 0.1
    hi = _vals(_ln_rows(H, 0)[3], 0).double()
    eye = torch.eye(H, device="cuda")
    zeroH = _fbuf(torch.zeros((H,), device="cuda"))
    s, _ = _ln_call(1, MAXB, 0, H, _wbuf(_bits(eye)), zeroH, H, True, W0lo=_wbuf(torch.zeros((H, H), dtype=torch.int16, device="cuda")))
    lo = s.double() - hi
    assert (lo.abs() <= 2.0 ** -8 * hi.abs()).all() and float(lo.abs().max()) > 0
    D = lambda t: t.double()
    want = (hi + lo) @ (D(Whi) + D(Wlo)).T + D(b)
    m3 = hi.abs() @ D(Whi).abs().T + lo.abs() @ D(Whi).abs().T + hi.abs() @ D(Wlo).abs().T
    bound = 2 * 3 * H * 2.0 ** -24 * m3 + lo.abs() @ D(Wlo).abs().T + 2.0 ** -24 * ((hi + lo).abs() @ D(Whi).abs().T)
    Wh, Wl, bb = _wbuf(_bits(Whi)), _wbuf(_bits(Wlo)), _fbuf(b)
    worst = 0.0
    for nb in range(1, MAXB + 1):
        got, _ = _ln_call(1, nb, 0, H, Wh, bb, N, True, W0lo=Wl)
        r = (got.double() - want[:nb]).abs() / bound[:nb]
        worst = max(worst, float(r.max()))
        assert (r <= 1).all(), (H, nb, float(r.max()))
    print(f"[parity] narrow split head H={H} N={N}: worst err / bound {worst:.3f}")


# ---- 5. hygiene: NaN in the rows a launch must not read -------------------------------------------------------------------------
@pytest.mark.parametrize("nb", range(1, MAXB + 1))
def test_ln_rows_beyond_nb_are_not_read(nb):
    """(every other launch of this file already poisons rows >= nb of x and of the out kernels' operands and checks the sentinels; here
    the SAME launch with finite rows >= nb gives the same bits)"""
    H, N0, N1 = 576, 130, 130
    W0, W1 = _wbuf(_rand_mats(H, N0, 0, 11)), _wbuf(_rand_mats(H, N1, 0, 12))
    b0, b1 = _fbuf(_randn((N0,), 13) * 0.1), _fbuf(_randn((N1,), 14) * 0.1)
    a = _ln_call(1, nb, 0, H, W0, b0, N0, False, W1=W1, b1=b1, N1=N1)
    b = _ln_call(1, nb, 0, H, W0, b0, N0, False, W1=W1, b1=b1, N1=N1, x=_ln_rows(H, 0)[0])  # all 8 rows finite
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.isnan(_vals(a[0])).any() and not torch.isnan(_vals(a[1])).any()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def _refused(rc):
    assert rc != 0 and len(L().load().showo_last_error()) > 0


def test_ln_hook_refuses_what_the_kernels_do_not_serve():
    H, N = 128, 130
    W, _, zero, Wz = _one_hot(N, H, 0)
    W8, sc = _wbuf(torch.ones((N, 136), dtype=torch.int8, device="cuda"), True), _fbuf(torch.ones((N,), device="cuda"))

    def bad(kernel, nb, op, H, f32=True, **kw):
        rc, o0, o1 = _ln_call(kernel, nb, op, H, kw.pop("W0", W), zero, N, f32, check=False, x=_ln_rows(128, 0)[0][:, :min(H, 128)], **kw)
        _refused(rc)
        assert (o0 == (SENTF if f32 else SENT16)).all() and (o1 is None or (o1 == SENT16).all())  # nothing was launched

    bad(1, 1, 0, 132)                      # H % 8
    bad(1, 1, 0, 2056)                     # H > 2048
    bad(1, 0, 0, H)                        # nb range
    bad(1, 9, 0, H)
    bad(0, 2, 0, H)                        # the batch-1 kernel serves one row
    bad(2, 1, 0, H)                        # no such kernel
    bad(1, 1, 2, H)                        # no such operand type
    bad(1, 1, 0, 136, W0=W8, s0=sc)        # int8: H % 16
    bad(1, 1, 1, H, W0=W8, s0=sc)          # int8 weights multiply bf16 activations
    bad(1, 1, 0, H, W0=W8, s0=sc, W1=W8, b1=zero, N1=N)  # int8: a scale per matrix
    bad(1, 1, 0, H, W0=W8, s0=sc, W0lo=W)  # int8 and the split head
    bad(0, 1, 0, H, W0lo=W)                # the split head is the batched kernel's
    bad(1, 1, 0, H, f32=False, W0lo=W)     # ... writes fp32 logits
    bad(1, 1, 1, H, W0lo=W)                # ... multiplies bf16 halves
    bad(1, 1, 0, H, W0lo=W, W1=W, b1=zero, N1=N)  # ... has no second matrix
    bad(1, 1, 0, H, W0=W[4:])              # 16-byte alignment of the weights
    bad(1, 1, 0, H, W1=W[4:], b1=zero, N1=N)
    p = L().ptr
    o = torch.full((N,), SENTF, device="cuda")
    x, w, b, _ = _ln_rows(H, 0)
    fn = L().load().showo_decode_narrow_ln_gemv
    _refused(fn(1, 1, 0, p(x) + 4, p(w), p(b), EPS, H, p(W), None, None, p(zero), None, p(o), N, N, None, None, None, None, 0, 0, S()))
    _refused(fn(1, 1, 0, p(x), p(w), p(b), EPS, H, p(W), None, None, p(zero), None, None, N, N, None, None, None, None, 0, 0, S()))  # no output
    _refused(fn(1, 1, 0, p(x), p(w), p(b), EPS, H, p(W), None, None, p(zero), None, p(o), N, N - 1, None, None, None, None, 0, 0, S()))  # ld0 < N0
    torch.cuda.synchronize()
    assert (o == SENTF).all()


def test_out_hook_refuses_what_the_kernels_do_not_serve():
    N = 130
    c = _int_case(128, 256, "bf16", N)
    q = _int_case(128, 256, "int8", N)

    def bad(kernel, nb, mode, op, case=c, y2=True, **kw):
        cc = dict(case, **kw)
        x0 = case["x"].clone()
        y0 = case["y2"].clone() if y2 else None
        xb, yb = _padded(x0, MAXB, N, float("nan")), None if y0 is None else _padded(y0, MAXB, N, float("nan"))
        p = L().ptr
        K0, K1 = cc["K0"], cc["K1"]
        a0, a1 = _padded(case["a0"], MAXB, 136, SENT16), _padded(case["a1"], MAXB, 264, SENT16)
        rc = L().load().showo_decode_narrow_out_gemv(kernel, nb, mode, op, p(xb), p(cc["W0"]), p(cc.get("A0", a0)), p(cc["s0"]), p(cc["b0"]), K0,
                                                     cc.get("lda0", 136), p(cc["W1"]), p(a1), p(cc["s1"]), p(cc["b1"]), K1, cc.get("lda1", 264), N,
                                                     p(yb), S())
        _refused(rc)
        torch.cuda.synchronize()
        assert torch.equal(xb[:MAXB * N].view(MAXB, N), x0) and (yb is None or torch.equal(yb[:MAXB * N].view(MAXB, N), y0))

    bad(1, 1, 0, 0, K0=132)                 # K0 % 8
    bad(1, 1, 0, 0, K0=2056)                # K0 > 2048
    bad(1, 1, 0, 0, K1=8200)                # K1 > 8192
    bad(1, 1, 0, 0, K1=260)                 # K1 % 8
    bad(0, 1, 1, 0, K1=8200)
    bad(0, 1, 2, 0, K0=2056)
    bad(1, 0, 0, 0)                         # nb ranges
    bad(1, 9, 0, 0)
    bad(0, 2, 0, 0)
    bad(2, 1, 2, 0)
    bad(2, 5, 2, 0)
    bad(3, 1, 0, 0)                         # no such kernel
    bad(0, 1, 3, 0)                         # no such mode
    bad(1, 2, 1, 0)                         # the batched kernels: mode 0 (out_gemvB) and mode 2 (out_dense_y2B) only
    bad(2, 2, 0, 0)
    bad(1, 1, 0, 2)                         # no such operand type
    bad(0, 1, 1, 0, y2=False)               # modes 1 and 2 need y2
    bad(0, 1, 2, 0, y2=False)
    bad(2, 2, 2, 0, y2=False)
    bad(1, 1, 0, 0, lda0=120)               # lda < K
    bad(1, 1, 0, 0, lda1=260)               # lda % 8
    bad(1, 1, 0, 0, W0=c["W0"][4:])         # 16-byte alignment
    bad(1, 1, 0, 0, W1=c["W1"][4:])
    bad(1, 2, 0, 0, A0=_padded(c["a0"], MAXB, 136, SENT16)[4:])
    bad(1, 1, 0, 1, case=q)                 # int8 weights multiply bf16 activations
    bad(1, 1, 0, 0, case=q, K0=120)         # int8: K % 16
    bad(1, 1, 0, 0, case=q, K1=248)
    bad(2, 2, 2, 0, case=q, K0=120)
    bad(1, 1, 0, 0, case=q, s1=None)        # int8: a scale per matrix
    bad(0, 1, 0, 0, case=q, s0=None)
