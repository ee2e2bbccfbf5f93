"""Exact, row-by-row tests of which keys the multi-row (prefill / t2i / training) attention kernels see: csrc/attention.hip
attn_fwd_kernel (gather form) and attn_lds_body (LDS-tiled form: bf16, IEEE half, split and lse variants), csrc/attention_bwd.hip.

Every other test of these kernels compares random Gaussian operands with an fp64 soft-max at a bf16 tolerance: at L = 387 a row sees
some 300 keys, so one key too many or too few moves the output by 1/300 of |V| -- inside the bound.  Here nothing is approximate
(operands and expectations come from tests/attn_exact_ref.py, which tests/test_attn_exact_ref_cpu.py checks on the CPU):

  1. counting         Q = 0, integer V, power-of-two visibility: O is the rounded mean of the visible rows, bit for bit; the same
                      visibility as a dense additive mask (flag = 1), and through showo_mask_compress (flag == 0, same visibility)
  2. dominating key   a score gap of 256: O[r] is row k*_r of V, bit for bit (K row order against V^T column order, stale mass)
  3. the same on showo_attn_fwd_split (hi / lo pairs) and showo_attn_fwd_lse (lse = ln n or 512 within _lse_bound of
     test_train_kernels_scale_gpu.py)
  4. backward         one-hot probes: dV / dK columns are exactly 0 on every hidden key, nonzero on every visible one
  5. an empty row     a row without a visible key does not disturb the other rows of its wave
  plus appended rows (Lq < Lk, no table: the causal offset) by an indicator V.

Layout of every launch: Lcap = Lk + 64 with NaN in the K rows behind Lk, Lp = ceil64(Lk) with zero V^T pad columns (the engine's
invariant for the MFMA kernels), O with ldo = nH * 64 + 8 (one case + 4: no 16-byte stores) and two rows behind the last one, a
sentinel in everything the kernel must not write.  (B, nH) = (1, 3) is tail-only in the XCD-aware block order, (2, 5) grouped + tail;
batch b walks the interval table with another phase, and values depend on batch and head.

No tolerance here is new: bit equality and exact zero patterns, except lse (_lse_bound, imported), the visible entries of dV (2^-7
relative: the per-term bound in the docstring of test_train_kernels_scale_gpu.py::test_attention_lse_and_backward_at_scale) and dQ
(2^-6 * scale + 1e-3 of the same test)."""
import functools

import pytest
import torch

import util
import attn_exact_ref as R
from attn_exact_ref import BF16, F16
from test_train_kernels_scale_gpu import _lse_bound

pytestmark = pytest.mark.gpu

SQUARE = [2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 258, 387]  # 64: gather -> tiled by shape; 128 / 129: one and two blocks; 258 / 387: t2i
COUNT_ONLY = 1155                                              # 19 key tiles
APPENDED = [(5, 45), (70, 200), (130, 517)]
BACKWARD = [64, 129, 387]
GRIDS = [(1, 3), (2, 5)]
NAN_BITS = {BF16: 0x7FC0, F16: 0x7E00}
SENT = 0x5A5A  # sentinel bit pattern of the output buffer (a finite value in either type)


def L():
    return util.lib()


def S():
    return util.lib().stream()


@pytest.fixture(params=[1, 2], ids=["gather", "lds-tiled"])
def attn_impl(request):
    """both forward kernels (as in test_kernels_gpu.py): 1 = gather form, 2 = LDS-tiled form; restored to by-shape afterwards"""
    L().call("showo_attn_set_impl", request.param)
    yield request.param
    L().call("showo_attn_set_impl", 0)


# ------------------------------------------------------------------------------------------------ launches
def _kv(k, v, Lk, op):
    """K [B, nH, Lk + 64, 64] (NaN behind Lk) and V^T [B, nH, 64, ceil64(Lk)] (zero pad columns) on the device"""
    B, nH = k.shape[:2]
    K = torch.full((B, nH, Lk + 64, 64), NAN_BITS[op], dtype=torch.int16)
    K[:, :, :Lk] = R.bits(k, op)
    Vt = torch.zeros((B, nH, 64, R.ceil64(Lk)), dtype=torch.int16)
    Vt[..., :Lk] = R.bits(v, op).transpose(2, 3)
    return K.cuda(), Vt.cuda()


def _mask_args(B, Lq, Lk, iv, dense):
    """(iv, flag, dense) device tensors: an interval table (flag 0), a dense additive mask (flag 1), or neither (causal)"""
    if dense is not None:
        return (torch.zeros((B, Lq, 4), dtype=torch.int32, device="cuda"), torch.ones(4, dtype=torch.int32, device="cuda"),
                dense.reshape(B, 1, Lq, Lk).to(torch.float32).contiguous().cuda())
    if iv is not None:
        return iv.to(torch.int32).contiguous().cuda(), torch.zeros(4, dtype=torch.int32, device="cuda"), None
    return None, None, None


def _out(B, Lq, ldo):
    return torch.full((B * Lq + 2, ldo), SENT, dtype=torch.int16, device="cuda")


def _take(Od, B, nH, Lq, op, what):
    """the [B, Lq, nH * 64] values of an output buffer, after checking that the extra columns and rows still hold the sentinel"""
    o = Od.cpu()
    assert bool((o[:B * Lq, nH * 64:] == SENT).all()) and bool((o[B * Lq:] == SENT).all()), ("wrote outside its rows / columns", what)
    return R.vals(o[:B * Lq, :nH * 64].contiguous(), op).reshape(B, Lq, nH * 64)


def _fwd(q, k, v, Lk, op, iv=None, dense=None, pad=8, lse=False, what=None):
    """showo_attn_fwd / _op16 / _lse on fp32 q [B, nH, Lq, 64], k / v [B, nH, Lk, 64] (rounded to the operand type here)"""
    B, nH, Lq, _ = q.shape
    ldo = nH * 64 + pad
    Qd = R.bits(q, op).contiguous().cuda()
    Kd, Vd = _kv(k, v, Lk, op)
    ivd, flag, md = _mask_args(B, Lq, Lk, iv, dense)
    Od = _out(B, Lq, ldo)
    head = (L().ptr(Qd), L().ptr(Kd), L().ptr(Vd), L().ptr(ivd), L().ptr(flag), L().ptr(md), L().ptr(Od))
    tail = (B, nH, Lq, Lk, Lk + 64, R.ceil64(Lk), ldo)
    lsed = None
    if lse:
        assert op == BF16
        lsed = torch.full((B, nH, Lq), float("nan"), dtype=torch.float32, device="cuda")
        L().call("showo_attn_fwd_lse", *head, L().ptr(lsed), *tail, S())
    elif op == BF16:
        L().call("showo_attn_fwd", *head, *tail, S())
    else:
        L().call("showo_attn_fwd_op16", *head, *tail, op, S())
    torch.cuda.synchronize()
    o = _take(Od, B, nH, Lq, op, what)
    return (o, lsed.cpu()) if lse else o


def _fwd_split(q, k, klo, vhi, vlo, Lk, iv=None, dense=None, what=None):
    """showo_attn_fwd_split: Q low halves 0, K as (k, klo), V as (vhi, vlo); returns (Ohi, Olo)"""
    B, nH, Lq, _ = q.shape
    ldo = nH * 64 + 8
    Qd = R.bits(q, BF16).contiguous().cuda()
    Ql = torch.zeros_like(Qd)
    Kd, Vd = _kv(k, vhi, Lk, BF16)
    Kl, Vl = _kv(klo, vlo, Lk, BF16)
    ivd, flag, md = _mask_args(B, Lq, Lk, iv, dense)
    Oh, Ol = _out(B, Lq, ldo), _out(B, Lq, ldo)
    L().call("showo_attn_fwd_split", L().ptr(Qd), L().ptr(Ql), L().ptr(Kd), L().ptr(Kl), L().ptr(Vd), L().ptr(Vl), L().ptr(ivd), L().ptr(flag),
             L().ptr(md), L().ptr(Oh), L().ptr(Ol), B, nH, Lq, Lk, Lk + 64, R.ceil64(Lk), ldo, S())
    torch.cuda.synchronize()
    return _take(Oh, B, nH, Lq, BF16, what), _take(Ol, B, nH, Lq, BF16, what)


def _assert_rows(got, want, iv, what, rows=None):
    """equality of every value (a NaN never passes; +0 and -0 are the same value) of [B, Lq, nH * 64] on every row, or on the bool
    [B, Lq] selection, naming the interval rows that differ"""
    bad = (got != want) | torch.isnan(got)
    bad = bad.any(-1)
    if rows is not None:
        bad = bad & rows
    if bool(bad.any()):
        idx = bad.nonzero().tolist()
        show = [(b, r, iv[b, r].tolist() if iv is not None else None) for b, r in idx[:12]]
        diff = float((got - want)[bad].abs().nan_to_num(nan=float("inf")).max())
        raise AssertionError(f"{what}: {len(idx)} rows differ, max |diff| {diff:.4g}; (batch, row, (lo1, hi1, lo2, hi2)): {show}")


def _live(iv, Lk):
    return R.vis_of(iv, Lk).any(-1)


# ------------------------------------------------------------------------------------------------ shared CPU cases (computed once)
@functools.lru_cache(maxsize=None)
def _counting(B, nH, Lq, Lk, layout, empty=False):
    torch.manual_seed(Lq * 7 + Lk)
    iv = R.batch_table(B, Lq, Lk, layout, empty=empty)
    v = R.int_v(B, nH, Lk)
    live = _live(iv, Lk)
    ivl = iv.clone()
    ivl[~live] = torch.tensor([0, 1, 0, 0], dtype=torch.int32)  # an empty row's expectation is not defined (and not compared)
    mean = R.counting_mean(v, ivl)
    return dict(iv=iv, v=v, k=torch.randn(B, nH, Lk, 64), q=torch.zeros(B, nH, Lq, 64), live=live, mean=mean,
                want={op: R.rnd(mean, op) for op in (BF16, F16)}, dense=R.dense_of(R.vis_of(iv, Lk)))


@functools.lru_cache(maxsize=None)
def _dominating(B, nH, L_, layout, empty=False):
    iv = R.batch_table(B, L_, L_, layout, empty=empty)
    q, k, ks = R.dominating_qk(iv, L_, nH)
    g = torch.Generator().manual_seed(31 * L_ + B)
    v = torch.randn(B, nH, L_, 64, generator=g)
    return dict(iv=iv, q=q, k=k, ks=ks, v=v, live=_live(iv, L_), dense=R.dense_of(R.vis_of(iv, L_)))


def _shapes():
    return [(n, n) for n in SQUARE]


# ================================================================================================ 1. counting
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_counting_bit_exact(layout, attn_impl):
    """1. Q = 0 (every visible p is 1), integer V, intervals given directly (flag = 0) and as a dense additive mask (flag = 1), bf16
    and fp16: O == the rounded mean of the visible rows on every row.  ldo = nH * 64 + 8; at L = 129 also + 4 (8-byte stores)."""
    for B, nH in GRIDS:
        for Lq, Lk in _shapes() + ([(COUNT_ONLY, COUNT_ONLY)] if (B, nH) == (1, 3) else []):
            c = _counting(B, nH, Lq, Lk, layout)
            for op in (BF16, F16):
                for pad in (8, 4) if Lq == 129 else (8, ):
                    what = (layout, attn_impl, B, nH, Lq, op, pad)
                    _assert_rows(_fwd(c["q"], c["k"], c["v"], Lk, op, iv=c["iv"], pad=pad, what=what), c["want"][op], c["iv"], ("intervals", ) + what)
                    if Lq < COUNT_ONLY or op == BF16:
                        got = _fwd(c["q"], c["k"], c["v"], Lk, op, dense=c["dense"], pad=pad, what=what)
                        _assert_rows(got, c["want"][op], c["iv"], ("dense", ) + what)


def _compress(mask, B, Lq, Lk):
    md = mask.reshape(B, 1, Lq, Lk).to(torch.float32).contiguous().cuda()
    iv = torch.full((B, Lq, 4), -7, dtype=torch.int32, device="cuda")
    flag = torch.full((4, ), 9, dtype=torch.int32, device="cuda")
    L().call("showo_mask_compress", L().ptr(md), L().ptr(iv), L().ptr(flag), B, Lq, Lk, S())
    torch.cuda.synchronize()
    return iv.cpu(), int(flag[0])


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_mask_compress_recovers_the_table(layout):
    """1c. the dense mask of every table through showo_mask_compress: flag == 0 and intervals of the same visibility (equal to the
    table itself: the table's two runs are never adjacent)"""
    for Lq, Lk in _shapes() + [(COUNT_ONLY, COUNT_ONLY)]:
        c = _counting(2, 5, Lq, Lk, layout) if Lq < COUNT_ONLY else _counting(1, 3, Lq, Lk, layout)
        B = c["iv"].shape[0]
        iv, flag = _compress(c["dense"], B, Lq, Lk)
        assert flag == 0, (layout, Lq)
        assert torch.equal(R.vis_of(iv, Lk), R.vis_of(c["iv"], Lk)), (layout, Lq)
        assert torch.equal(iv, c["iv"]), (layout, Lq)


@pytest.mark.parametrize("Lq,Lk", [(7, 63), (9, 64), (8, 65), (70, 200), (16, 129)])  # Lq >= the number of edges: every edge starts a run
def test_mask_compress_rule_at_ballot_boundaries(Lq, Lk):
    """1d. the compress kernel's rule around its 64-column ballots: masks of 1, 2 and 3 runs whose run edges sit at 63 / 64 / 65 (and at
    Lk) round-trip (3 runs: flag set); a NaN or a -5.0 anywhere sets the flag; -0.0 counts as visible; Lq != Lk"""
    E = R.edges(Lk)
    assert Lq >= len(E)
    base = []
    for i in range(Lq):  # row i: runs that start / end at successive edges
        lo, hi = sorted((E[i % len(E)], E[(i + 2) % len(E)]))
        lo = min(lo, Lk - 1)
        base.append((lo, max(hi, lo + 1), 0, 0))
    one = torch.tensor(base, dtype=torch.int32)[None]
    iv, flag = _compress(R.dense_of(R.vis_of(one, Lk)), 1, Lq, Lk)
    assert flag == 0 and torch.equal(iv, one), (iv.tolist(), one.tolist())
    # two runs: hide one key inside every run that has at least three
    vis2 = R.vis_of(one, Lk).clone()
    want2 = one.clone()
    for i, (lo, hi, _, _) in enumerate(base):
        if hi - lo >= 3:
            cut = 63 if lo < 63 < hi - 1 else (64 if lo < 64 < hi - 1 else lo + 1)
            vis2[0, i, cut] = False
            want2[0, i] = torch.tensor([lo, cut, cut + 1, hi])
    iv, flag = _compress(R.dense_of(vis2), 1, Lq, Lk)
    assert flag == 0 and torch.equal(iv, want2), (iv.tolist(), want2.tolist())
    assert torch.equal(R.vis_of(iv, Lk), vis2)
    # -0.0 is visible
    m = R.dense_of(vis2)
    m[m == 0] = -0.0
    iv, flag = _compress(m, 1, Lq, Lk)
    assert flag == 0 and torch.equal(iv, want2)
    # three runs in one row: the flag
    vis3 = torch.zeros(1, Lq, Lk, dtype=torch.bool)
    vis3[0, :, 0] = vis3[0, :, Lk // 2] = vis3[0, :, Lk - 1] = True
    assert _compress(R.dense_of(vis3), 1, Lq, Lk)[1] == 1
    vis3[0, :-1] = vis2[0, :-1]  # only the last row has three runs
    assert _compress(R.dense_of(vis3), 1, Lq, Lk)[1] == 1
    # a NaN or a soft bias anywhere (first / last column, the ballot boundaries), on a visible or a hidden key
    for col in sorted({0, 62, 63, 64, 65, Lk - 1} & set(range(Lk))):
        for val in (float("nan"), -5.0):
            for row in (0, Lq - 1):
                m = R.dense_of(vis2)
                m[0, row, col] = val
                assert _compress(m, 1, Lq, Lk)[1] == 1, (col, val, row)


# ================================================================================================ 2. dominating key
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_dominating_key_bit_exact(layout, attn_impl):
    """2. the target key scores 512, every other key at most 256: every other exp2 term is exactly 0 and O[r] is row k*_r of V bit for
    bit, with the intervals and with the dense mask, in bf16 and fp16.  The targets walk lo1, hi1 - 1, lo2, hi2 - 1 and the interior."""
    for B, nH in GRIDS:
        for n, _ in _shapes():
            c = _dominating(B, nH, n, layout)
            for op in (BF16, F16):
                v = R.rnd(c["v"], op)
                want = R.gather_rows(v, c["ks"])
                for pad in (8, 4) if n == 129 else (8, ):
                    what = (layout, attn_impl, B, nH, n, op, pad)
                    _assert_rows(_fwd(c["q"], c["k"], v, n, op, iv=c["iv"], pad=pad, what=what), want, c["iv"], ("intervals", ) + what)
                    _assert_rows(_fwd(c["q"], c["k"], v, n, op, dense=c["dense"], pad=pad, what=what), want, c["iv"], ("dense", ) + what)


# ================================================================================================ 3. the other entry points
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_split_entry_counting_and_dominating_key(layout, attn_impl):
    """3a. showo_attn_fwd_split.  Counting: V low halves 0, K a (hi, lo) pair of random values: Ohi == the bf16 expectation, Olo ==
    bf16(mean - Ohi).  Dominating key: V a (hi, lo) pair with |lo| <= ulp(hi) / 2: Ohi == hi and Olo == lo of row k*_r.
    (This entry has the LDS-tiled form only: it must give the same bits under either setting of showo_attn_set_impl.)"""
    for B, nH in GRIDS:
        for n, _ in _shapes():
            c = _counting(B, nH, n, n, layout)
            khi, klo = R.split_of(c["k"])
            zero = torch.zeros_like(c["v"])
            for name, kw in (("intervals", dict(iv=c["iv"])), ("dense", dict(dense=c["dense"]))):
                what = (name, "counting", layout, B, nH, n)
                oh, ol = _fwd_split(c["q"], khi, klo, c["v"], zero, n, what=what, **kw)
                _assert_rows(oh, c["want"][BF16], c["iv"], ("Ohi", ) + what)
                _assert_rows(ol, R.rnd(c["mean"] - c["want"][BF16], BF16), c["iv"], ("Olo", ) + what)
            d = _dominating(B, nH, n, layout)
            vhi, vlo = R.split_v(B, nH, n, 17 * n + B)
            for name, kw in (("intervals", dict(iv=d["iv"])), ("dense", dict(dense=d["dense"]))):
                what = (name, "dominating", layout, B, nH, n)
                oh, ol = _fwd_split(d["q"], d["k"], torch.zeros_like(d["k"]), vhi, vlo, n, what=what, **kw)
                _assert_rows(oh, R.gather_rows(vhi, d["ks"]), d["iv"], ("Ohi", ) + what)
                _assert_rows(ol, R.gather_rows(vlo, d["ks"]), d["iv"], ("Olo", ) + what)


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_lse_entry_counting_and_dominating_key(layout, attn_impl):
    """3b. showo_attn_fwd_lse: O as in 1 and 2; lse == ln n (counting) or 512 (dominating key) within the per-row _lse_bound of
    test_train_kernels_scale_gpu.py (imported: no new tolerance).  Only the tiled form writes lse, whatever showo_attn_set_impl says."""
    for B, nH in GRIDS:
        for n, _ in _shapes():
            c = _counting(B, nH, n, n, layout)
            d = _dominating(B, nH, n, layout)
            vd = R.rnd(d["v"], BF16)
            for name, x, v, want_o in (("counting", c, c["v"], c["want"][BF16]), ("dominating", d, vd, R.gather_rows(vd, d["ks"]))):
                vis = R.vis_of(x["iv"], n)[:, None]  # [B, 1, Lq, Lk]
                s = x["q"].double() @ R.rnd(x["k"], BF16).double().transpose(-1, -2)
                want_lse = torch.logsumexp(s.masked_fill(~vis, float("-inf")), -1)
                for mode, kw in (("intervals", dict(iv=x["iv"])), ("dense", dict(dense=x["dense"]))):
                    what = (mode, name, layout, B, nH, n)
                    o, lse = _fwd(x["q"], x["k"], v, n, BF16, lse=True, what=what, **kw)
                    _assert_rows(o, want_o, x["iv"], what)
                    err = (lse.double() - want_lse).abs()
                    bound = _lse_bound(x["q"], R.rnd(x["k"], BF16), s, vis, want_lse)
                    assert bool((err <= bound).all()), (what, float(err.max()), float((err / bound).max()))


# ================================================================================================ appended rows (causal offset)
@pytest.mark.parametrize("Lq,Lk", APPENDED)
def test_appended_rows_causal_indicator_bit_exact(Lq, Lk, attn_impl):
    """Lq < Lk without a table: row r sees the first r + 1 + Lk - Lq keys (no power of two).  The indicator-V trick of
    test_decode_attn_lengths_gpu.py::test_counting_causal_indicator_bit_exact: V is 1 at one key per (head, dimension); O is 0 where
    that key is hidden (every row) and round(1 / n) where it is seen, on the rows whose 1 / n passes that file's
    _one_over_is_unambiguous."""
    torch.manual_seed(Lk)
    for B, nH in GRIDS:
        q, k = torch.zeros(B, nH, Lq, 64), torch.randn(B, nH, Lk, 64)
        for op in (BF16, F16):
            v, want, check = R.indicator_case(B, nH, Lq, Lk, op)
            got = _fwd(q, k, v, Lk, op, what=(Lq, Lk, B, nH, op))
            assert torch.isfinite(got).all()
            civ = R.causal_table(B, Lq, Lk)
            _assert_rows(torch.where(want == 0, got, want), want, civ, ("hidden keys", Lq, Lk, B, nH, op))
            assert bool(((got != 0) == (want != 0)).all()), "a visible indicator key gave 0"
            _assert_rows(got, want, civ, ("1 / n", Lq, Lk, B, nH, op), rows=check[None].expand(B, Lq))


# ================================================================================================ 4. backward
def _col(t, c):
    return t.data_ptr() + c * t.element_size()


def _run_backward(c):
    """showo_attn_fwd_lse + showo_head_transpose + showo_attn_bwd on a backward_case (production layout: V and the gradients in
    [B * L, 3H] token-major buffers).  Returns (O, lse, out) with out [B * L, 3H] = dQ | dK | dV, and a second backward's out."""
    B, nH, n, _ = c["q"].shape
    H, Lp = nH * 64, R.ceil64(n)
    Qd, Kd = (R.bits(c[t], BF16).contiguous().cuda() for t in ("q", "k"))
    Vt = torch.zeros((B, nH, 64, Lp), dtype=torch.int16, device="cuda")
    Vt[..., :n] = R.bits(c["v"], BF16).transpose(2, 3).cuda()
    qkv = torch.zeros((B * n, 3 * H), dtype=torch.int16, device="cuda")
    qkv[:, 2 * H:] = R.bits(c["v"], BF16).transpose(1, 2).reshape(B * n, H).cuda()
    iv = c["iv"].contiguous().cuda()
    flag = torch.zeros(4, dtype=torch.int32, device="cuda")
    Od = torch.zeros((B * n, H), dtype=torch.int16, device="cuda")
    lse = torch.full((B, nH, n), float("nan"), dtype=torch.float32, device="cuda")
    L().call("showo_attn_fwd_lse", L().ptr(Qd), L().ptr(Kd), L().ptr(Vt), L().ptr(iv), L().ptr(flag), None, L().ptr(Od), L().ptr(lse),
             B, nH, n, n, n, Lp, H, S())
    QT = torch.zeros((B, nH, 64, Lp), dtype=torch.int16, device="cuda")
    KT = torch.zeros_like(QT)
    L().call("showo_head_transpose", L().ptr(Qd), L().ptr(QT), B, nH, n, Lp, nH * n * 64, n * 64, 64, S())
    L().call("showo_head_transpose", L().ptr(Kd), L().ptr(KT), B, nH, n, Lp, nH * n * 64, n * 64, 64, S())
    dOd = R.bits(c["do"].reshape(B * n, H), BF16).contiguous().cuda()

    def backward():
        dOT = torch.full((B, nH, 64, Lp), 0x7fc0, dtype=torch.int16, device="cuda")
        D = torch.full((B, nH, n), float("nan"), dtype=torch.float32, device="cuda")
        out = torch.full((B * n, 3 * H), 0x7fc0, dtype=torch.int16, device="cuda")
        L().call("showo_attn_bwd", L().ptr(Qd), L().ptr(Kd), L().ptr(QT), L().ptr(KT), _col(qkv, 2 * H), 3 * H, L().ptr(Od),
                 L().ptr(dOd), H, L().ptr(dOT), L().ptr(lse), L().ptr(D), L().ptr(iv), L().ptr(flag), _col(out, 0), 3 * H,
                 _col(out, H), 3 * H, _col(out, 2 * H), 3 * H, B, nH, n, Lp, S())
        torch.cuda.synchronize()
        return out.cpu()

    out = backward()
    return R.vals(Od.cpu(), BF16), lse.cpu(), out, backward()


def _head_major(out, i, B, nH, n):
    """section i (0 dQ, 1 dK, 2 dV) of out [B * L, 3H] as fp32 [B, nH, L, 64]"""
    H = nH * 64
    return R.vals(out[:, i * H:(i + 1) * H].contiguous(), BF16).reshape(B, n, nH, 64).transpose(1, 2)


@pytest.mark.parametrize("layout", ["mixed", "block_gap"])
@pytest.mark.parametrize("n", BACKWARD)
def test_backward_visibility_pattern(n, layout, attn_impl):
    """4. One-hot probes (rows at wave and block edges, one head dimension each).
    dV: Q = 0, dO[r*_j] = e_{d_j}: dV[k, d_j] = P[r*_j, k] -- exactly 0 on every key hidden from r*_j, nonzero and within 2^-7 relative
        of 1 / n on every visible one (the per-term bound of test_attention_lse_and_backward_at_scale's docstring).
    dK: K = 0, Q[r*_j] = dO[r*_j] = e_{d_j}, V = +-1 with both signs visible: dK[k, d_j] = P (dP - D) is exactly 0 iff k is hidden.
    dQ (and dK / dV as a whole) against the fp64 autograd at that test's 2^-6 * scale + 1e-3.  Two backward runs: identical bits."""
    for B, nH in GRIDS:
        for which in ("dv", "dk"):
            c = R.backward_case(B, nH, n, layout, which)
            o, lse, out, again = _run_backward(c)
            what = (which, layout, B, nH, n)
            assert torch.equal(out, again), ("attention backward is not run-to-run deterministic", what)
            ro, rlse, rdq, rdk, rdv = R.backward_reference(c)
            got = [_head_major(out, i, B, nH, n) for i in range(3)]
            assert all(bool(torch.isfinite(g).all()) for g in got), ("a gradient row was never written", what)
            nvis = c["vis"].sum(-1)
            for b in range(B):
                for h in range(nH):
                    for j, (r, d) in enumerate(zip(c["rows"], c["dims"][b][h])):
                        vis = c["vis"][b, r]
                        col = got[2 if which == "dv" else 1][b, h, :, d]
                        hidden_nz = ((col != 0) & ~vis).nonzero().flatten().tolist()
                        assert not hidden_nz, (what, "nonzero on hidden keys", b, h, r, c["iv"][b, r].tolist(), hidden_nz[:8])
                        if which == "dv" or bool(c["usable"][b, h, j]):
                            vis_z = ((col == 0) & vis).nonzero().flatten().tolist()
                            assert not vis_z, (what, "zero on visible keys", b, h, r, c["iv"][b, r].tolist(), vis_z[:8])
                        if which == "dv":
                            p = 1.0 / float(nvis[b, r])
                            rel = float((col[vis] - p).abs().max()) / p
                            assert rel <= 2 ** -7, (what, b, h, r, rel)
            if which == "dv":
                assert bool((got[1] == 0).all()), ("dK = dS^T Q with Q = 0", what)
            for name, g, want in (("dQ", got[0], rdq), ("dK", got[1], rdk), ("dV", got[2], rdv)):
                err, scale = float((g.double() - want).abs().max()), float(want.abs().max())
                print(f"[parity] attn bwd probes {what} {name}: max err {err:.3e} <= {2 ** -6 * scale + 1e-3:.3e}")
                assert err < 2 ** -6 * scale + 1e-3, (what, name, err, scale)


# ================================================================================================ 5. a row without a visible key
@pytest.mark.parametrize("n", [33, 64, 129, 387])
def test_empty_row_does_not_disturb_its_wave(n, attn_impl):
    """5. In the "mixed" table one row per wave, at wave position 0 or 31, sees nothing (0, 0, 0, 0).  Every other row is still bit
    exact under counting and under the dominating key.  The empty row's own output is not asserted: the kernels divide by l = 0 there
    (the reference's convention, a uniform average over all keys, is a separate decision).  Measured on the MI355X: both forms, both
    operand types return NaN in every element of such a row (0 * inf), and the lse entry returns -inf."""
    for B, nH in GRIDS:
        c = _counting(B, nH, n, n, "mixed", True)
        d = _dominating(B, nH, n, "mixed", True)
        assert int((~c["live"]).sum()) == B * len(R.empty_rows(n)) > 0
        for op in (BF16, F16):
            what = ("empty rows", attn_impl, B, nH, n, op)
            got = _fwd(c["q"], c["k"], c["v"], n, op, iv=c["iv"], what=what)
            _assert_rows(got, c["want"][op], c["iv"], ("counting", ) + what, rows=c["live"])
            e = got[~c["live"]]
            print(f"[parity] attn empty row {what}: all NaN {bool(torch.isnan(e).all())}, values {sorted(set(e.flatten().tolist()[:64]), key=str)[:4]}")
            v = R.rnd(d["v"], op)
            got = _fwd(d["q"], d["k"], v, n, op, iv=d["iv"], what=what)
            _assert_rows(got, R.gather_rows(v, d["ks"]), d["iv"], ("dominating", ) + what, rows=d["live"])
        o, lse = _fwd(c["q"], c["k"], c["v"], n, BF16, iv=c["iv"], lse=True, what="empty rows lse")
        _assert_rows(o, c["want"][BF16], c["iv"], ("lse entry", B, nH, n), rows=c["live"])
        el = lse[(~c["live"])[:, None].expand_as(lse)]
        print(f"[parity] attn empty row lse B={B} nH={nH} L={n}: {sorted(set(el.tolist()), key=str)[:4]}")
