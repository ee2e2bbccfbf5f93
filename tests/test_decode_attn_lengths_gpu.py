"""GPU tests of the single-query decode attention (csrc/attention.hip attn_decode_body) across KV-cache lengths.

The kernel's arithmetic is organised around the cache length: the first 1024 key rows are requested up front, keys from 1024 on go
through a tail loop with its own predicate, V^T comes as two prefetched 512-key chunks plus a loop from key 1024, the device-side decode
loops pass an upper bound instead of the length and clamp their loads onto it, the fused form takes the newest key / value from LDS, and
above 60 000 bytes of LDS `showo_attn_fwd` falls back to the gather kernel.  The tests here walk the lengths at which each of these
changes behaviour, with techniques that are EXACT, so that one key dropped or counted twice among a thousand cannot hide in a bf16
tolerance:

  Part 1 (kernel, through showo_attn_fwd / showo_attn_fwd_op16 with Lq = 1; K rows and V^T columns behind the live length hold NaN)
    1. counting: Q = 0, every p = 1, integer V: every fp32 sum is an exact integer, the output is known bit for bit
    2. a dominating key (score gap 256: every other exp2 term is exactly 0): the output is one row of V, bit for bit
    3. random operands against an fp64 soft-max, within the bound tests/test_kernels_gpu.py applies to this kernel
    4. the LDS switch: 14 848 keys (last length on the decode kernel) and 14 849 (first on the gather fallback)
  Part 2 (the fused forms, through the engine; tiny model with a 2048-row cache, start lengths that cross 512 / 1024 / 1536)
    5. hint bound (decode_greedy, graph and eager) against exact bound (decode_step): tokens, logits bits, cache bits
    6. fused three-launch layer against the seven-launch layer: logits bits at every step
    7. NaN in every stale cache row: same tokens and logits bits, the rows behind the run untouched
    8. the full cache: position 2047 succeeds, the next step is refused with the state unchanged
    9. teacher-forced logits at positions 511, 512, 1023, 1024, 1025, 2047 against the fp32 oracle
   10. batched slots (4 narrow: batch-1 bits; 9 wide: slot-independent bits)
   11. full width (H 2048, F 8192): co-scheduled launch == chain == seven-launch layer, batched co-scheduled launch == batch-1 runs

No tolerance here is new: everything is bit equality except test 3 (the kernel bound of test_kernels_gpu.py / test_fp16_gpu.py) and
test 9 (REL_RMS / REL_MAX of test_modules_gpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import util
from util import O, Wt

pytestmark = pytest.mark.gpu

BF16, F16 = 0, 1  # SHOWO_OP_BF16 / SHOWO_OP_F16
NAN_BITS = {BF16: 0x7FC0, F16: 0x7E00}
LENGTHS = [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1031, 1032, 1033, 1535, 1536, 1537, 2047, 2048]
LDS_SWITCH = [14848, 14849]  # 4 * 512 * ceil(Lk / 512) <= 60000 holds up to 14848
ROOMY = 2112
CACHE_FORMS = ["roomy", "full"]


def L():
    return util.lib()


def S():
    return util.lib().stream()


def _ceil64(n):
    return (n + 63) // 64 * 64


def _rnd(t, op):
    """fp32 -> the operand type and back"""
    return t.to(torch.float16 if op == F16 else torch.bfloat16).to(torch.float32)


def _bits(t, op):
    return t.to(torch.float16 if op == F16 else torch.bfloat16).view(torch.int16)


def _vals(b, op):
    return b.view(torch.float16 if op == F16 else torch.bfloat16).to(torch.float32)


def _pow2_le(n):
    return 1 << (int(n).bit_length() - 1)


def _kstars(Lk):
    return sorted({k for k in (0, 7, 8, 511, 512, 513, 1023, 1024, 1025, 1031, 1032, 1535, 1536, Lk - 1) if 0 <= k < Lk})


def _launch(q, k, v, Lk, form, op, iv=None, dense=None, zero_tail=False):
    """q [B, nH, 64], k / v [B, nH, Lk, 64] fp32 (rounded to the operand type here).  iv: [B, 4] visibility intervals (None: causal);
    dense: [B, Lk] additive fp32 mask, run with the dense flag set.  Slots behind Lk hold NaN (zero_tail: V^T columns hold 0, the
    engine's invariant for the MFMA / gather kernels).  Returns O [B, nH * 64] as fp32 values."""
    B, nH = q.shape[:2]
    if form == "full":
        Lcap, Lp = Lk, _ceil64(Lk)
    else:
        Lcap = Lp = max(ROOMY, _ceil64(Lk) + 64)
    nan = NAN_BITS[op]
    K = torch.full((B, nH, Lcap, 64), nan, dtype=torch.int16)
    K[:, :, :Lk] = _bits(k, op)
    Vt = torch.full((B, nH, 64, Lp), 0 if zero_tail else nan, dtype=torch.int16)
    Vt[..., :Lk] = _bits(v, op).transpose(2, 3)
    Kd, Vd, Qd = K.cuda(), Vt.cuda(), _bits(q, op).reshape(B, nH, 1, 64).contiguous().cuda()
    Od = torch.full((B, 1, nH * 64), nan, dtype=torch.int16, device="cuda")
    ivd = flag = md = None
    if dense is not None:
        ivd = torch.zeros((B, 1, 4), dtype=torch.int32, device="cuda")
        flag = torch.ones(4, dtype=torch.int32, device="cuda")  # what showo_mask_compress leaves for a mask no two intervals represent
        md = dense.reshape(B, 1, 1, Lk).to(torch.float32).contiguous().cuda()
    elif iv is not None:
        ivd = torch.tensor(iv, dtype=torch.int32).reshape(B, 1, 4).contiguous().cuda()
        flag = torch.zeros(4, dtype=torch.int32, device="cuda")
    args = (L().ptr(Qd), L().ptr(Kd), L().ptr(Vd), L().ptr(ivd), L().ptr(flag), L().ptr(md), L().ptr(Od), B, nH, 1, Lk, Lcap, Lp, nH * 64)
    if op == BF16:
        L().call("showo_attn_fwd", *args, S())
    else:
        L().call("showo_attn_fwd_op16", *args, op, S())
    torch.cuda.synchronize()
    return _vals(Od.cpu(), op).reshape(B, nH * 64)


def _vis_of(iv, Lk):
    """[B, Lk] bool visibility of interval rows (lo1, hi1, lo2, hi2)"""
    c = torch.arange(Lk)[None]
    t = torch.tensor(iv, dtype=torch.int64).reshape(-1, 4)
    return ((c >= t[:, 0:1]) & (c < t[:, 1:2])) | ((c >= t[:, 2:3]) & (c < t[:, 3:4]))


def _dense_of(vis):
    return torch.where(vis, torch.zeros(()), torch.full((), O.NEG_MASK))


def _int_v(B, nH, Lk):
    """deterministic integers in {-2 .. 2} that depend on key, dimension, head and sequence"""
    k = torch.arange(Lk)[None, None, :, None]
    d = torch.arange(64)[None, None, None, :]
    h = torch.arange(nH)[None, :, None, None]
    b = torch.arange(B)[:, None, None, None]
    return (((k * 31 + d * 17 + (k >> 3) * 7 + (k >> 9) * 3 + h * 11 + b * 13 + k * d) % 5) - 2).to(torch.float32)


def _mean_rows(v, vis, op):
    """rounded mean of the visible rows of integer v [B, nH, Lk, 64] under vis [B, Lk] with a power-of-two count: exact in fp32"""
    n = vis.sum(dim=1)
    assert all(int(x) > 0 and int(x) & (int(x) - 1) == 0 for x in n), n
    s = (v.to(torch.int64) * vis[:, None, :, None]).sum(dim=2)  # [B, nH, 64]
    assert int(s.abs().max()) < 2 ** 24
    want = s.to(torch.float32) / n[:, None, None].to(torch.float32)
    return _rnd(want, op).reshape(v.shape[0], -1)


def _interval_sets(Lk):
    """interval rows with a power-of-two visible count: one run and two runs, straddling 511/512, 1023/1024, 1535/1536 and ending at Lk"""
    out = [(Lk - _pow2_le(Lk), Lk, 0, 0)]
    for b in (512, 1024, 1536):
        if b >= Lk:
            continue
        h = _pow2_le(min(b, Lk - b))
        out.append((b - h, b + h, 0, 0))                       # h keys on either side of the boundary
        n = min(_pow2_le(b + 1), 256)
        out.append((b + 1 - n, b + 1, 0, 0))                   # the last visible key is the first one behind the boundary
        n = min(_pow2_le(Lk - b + 1), 256)
        out.append((b - 1, b - 1 + n, 0, 0))                   # the first visible key is the last one before the boundary
        w, c = 0, 2
        while b + c // 2 <= Lk - c and c // 2 <= b:            # largest w: [b - w/2, b + w/2) and [Lk - w, Lk) disjoint
            w, c = c, 2 * c
        if w:
            out.append((b - w // 2, b + w // 2, Lk - w, Lk))   # two runs of w keys: across the boundary, and up to Lk
    if Lk >= 2:
        h = _pow2_le(Lk // 2)
        out.append((0, h, Lk - h, Lk))
    for lo1, hi1, lo2, hi2 in out:
        assert 0 <= lo1 < hi1 <= Lk and (lo2 == hi2 == 0 or hi1 <= lo2 < hi2 <= Lk), (Lk, out)
    return out


def _one_over_is_unambiguous(Lk, op):
    """1 / Lk and its two fp32 neighbours round to the same 16-bit value: a reciprocal that is one ulp off cannot change the expectation"""
    f = np.float32(1) / np.float32(Lk)
    c = [f, np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(1))]
    r = {float(_rnd(torch.tensor(float(x), dtype=torch.float32), op)) for x in c}
    return len(r) == 1


# ================================================================================================ Part 1: the kernel
@pytest.mark.parametrize("Lk", LENGTHS)
def test_counting_intervals_with_power_of_two_visibility_bit_exact(Lk):
    """1a. Q = 0: every visible p is 1, V integers: O = round(sum of the visible rows / n), bit for bit.  One sequence per interval row."""
    torch.manual_seed(Lk)
    ivs = _interval_sets(Lk)
    B, nH = len(ivs), 2
    v = _int_v(B, nH, Lk)
    k = torch.randn(B, nH, Lk, 64)  # arbitrary: Q = 0
    q = torch.zeros(B, nH, 64)
    vis = _vis_of(ivs, Lk)
    for op in (BF16, F16):
        want = _mean_rows(v, vis, op)
        for form in CACHE_FORMS:
            got = _launch(q, k, v, Lk, form, op, iv=ivs)
            assert torch.isfinite(got).all(), (Lk, form, op)
            bad = (got != want).any(dim=1).nonzero().flatten().tolist()
            assert not bad, (Lk, form, op, [ivs[b] for b in bad], float((got - want).abs().max()))


@pytest.mark.parametrize("Lk", LENGTHS + LDS_SWITCH)
def test_counting_causal_indicator_bit_exact(Lk):
    """1b (and 4). Q = 0 under the causal form (all Lk keys), V = 1 at one key k* in one dimension: O = round(1 / Lk) there, 0 elsewhere.
    One head per k*; at the LDS switch one head, the indicator at Lk - 1 and at 1024 (one sequence each)."""
    torch.manual_seed(Lk)
    switch = Lk in LDS_SWITCH
    ks = [Lk - 1, 1024] if switch else _kstars(Lk)
    B, nH = (len(ks), 1) if switch else (1, len(ks))
    v = torch.zeros(B, nH, Lk, 64)
    want = torch.zeros(B, nH, 64)
    for i, kk in enumerate(ks):
        b, h = (i, 0) if switch else (0, i)
        v[b, h, kk, (5 * i + 3) % 64] = 1.0
        want[b, h, (5 * i + 3) % 64] = 1.0
    k = torch.randn(B, nH, Lk, 64)
    q = torch.zeros(B, nH, 64)
    for op in (BF16, F16):
        assert _one_over_is_unambiguous(Lk, op), (Lk, op)
        w = (want * _rnd(torch.tensor(1.0) / torch.tensor(float(Lk)), op)).reshape(B, -1)
        for form in CACHE_FORMS:
            got = _launch(q, k, v, Lk, form, op, zero_tail=(Lk == 14849))
            assert torch.isfinite(got).all(), (Lk, form, op)
            bad = (got != w).reshape(B * nH, 64).any(dim=1).nonzero().flatten().tolist()
            assert not bad, (Lk, form, op, [ks[i] for i in bad], float((got - w).abs().max()))


def _hidden_runs(k, Lk):
    """two runs around a hidden key k with a power-of-two count of visible keys"""
    n = _pow2_le(Lk - 1)
    a = min(k, n // 2)
    c = n - a
    if c > Lk - k - 1:
        c = Lk - k - 1
        a = n - c
    assert 0 <= a <= k and 0 <= c <= Lk - k - 1 and a + c == n
    return (k - a, k, k + 1, k + 1 + c) if a > 0 else (k + 1, k + 1 + c, 0, 0)


@pytest.mark.parametrize("Lk", LENGTHS)
def test_dominating_key_returns_its_value_row_bit_exact(Lk):
    """2. Q = 16 in one dimension, key k* = 16 there, every other live key 0: the score gap is 256, exp2 of every other term is exactly 0,
    tot = 1 and O is row k* of V bit for bit -- under the causal, one-interval, two-interval and dense masks, one sequence per k*.
    With k* hidden by the mask the output is the mean of the visible rows: counting (integer V, power-of-two visibility), exact."""
    torch.manual_seed(1000 + Lk)
    ks = _kstars(Lk)
    B, nH = len(ks), 2
    q = torch.zeros(B, nH, 64)
    k = torch.zeros(B, nH, Lk, 64)
    for b, kk in enumerate(ks):
        for h in range(nH):
            dq = (7 * b + 13 * h + 5) % 64
            q[b, h, dq] = 16.0
            k[b, h, kk, dq] = 16.0
    one = [(max(0, kk - 37), min(Lk, kk + 6), 0, 0) for kk in ks]
    two = [(max(0, kk - 300), kk + 1, min(Lk, kk + 3), Lk) if b % 2 == 0 else (0, min(kk, 5), kk, min(Lk, kk + 100)) for b, kk in enumerate(ks)]
    two = [(a, b_, (c if c < d else 0), (d if c < d else 0)) for a, b_, c, d in two]
    two = [(c, d, 0, 0) if a >= b_ else (a, b_, c, d) for a, b_, c, d in two]
    dvis = torch.rand(B, Lk) < 0.5
    for b, kk in enumerate(ks):
        dvis[b, kk] = True
    v_rand = torch.randn(B, nH, Lk, 64)
    for op in (BF16, F16):
        vr = _rnd(v_rand, op)
        want = torch.stack([vr[b, :, kk] for b, kk in enumerate(ks)]).reshape(B, -1)
        for form in CACHE_FORMS:
            for name, kw in (("causal", {}), ("one", dict(iv=one)), ("two", dict(iv=two)), ("dense", dict(dense=_dense_of(dvis)))):
                got = _launch(q, k, vr, Lk, form, op, **kw)
                assert torch.isfinite(got).all(), (Lk, form, op, name)
                bad = (got != want).any(dim=1).nonzero().flatten().tolist()
                assert not bad, (Lk, form, op, name, [ks[b] for b in bad], float((got - want).abs().max()))
    if Lk < 2:
        return  # one key: hiding it leaves a fully masked row (out of scope: the newest token always sees itself)
    hid = [_hidden_runs(kk, Lk) for kk in ks]
    hvis = _vis_of(hid, Lk)
    n = _pow2_le(Lk - 1)
    dh = torch.zeros(B, Lk, dtype=torch.bool)
    for b, kk in enumerate(ks):
        others = torch.cat([torch.arange(0, kk), torch.arange(kk + 1, Lk)])
        dh[b, others[torch.randperm(Lk - 1)[:n]]] = True
    vi = _int_v(B, nH, Lk)
    for op in (BF16, F16):
        for form in CACHE_FORMS:
            for name, vis, kw in (("hidden-two", hvis, dict(iv=hid)), ("hidden-dense", dh, dict(dense=_dense_of(dh)))):
                assert not any(bool(vis[b, kk]) for b, kk in enumerate(ks))
                got = _launch(q, k, vi, Lk, form, op, **kw)
                want = _mean_rows(vi, vis, op)
                assert torch.isfinite(got).all(), (Lk, form, op, name)
                bad = (got != want).any(dim=1).nonzero().flatten().tolist()
                assert not bad, (Lk, form, op, name, [ks[b] for b in bad], float((got - want).abs().max()))


def _random_case(Lk, nH, switch):
    """3. B = 2 with different intervals per sequence, the four mask families and both operand types against an fp64 soft-max"""
    torch.manual_seed(2000 + Lk)
    B = 2
    q0, k0, v0 = torch.randn(B, nH, 64) * 0.25, torch.randn(B, nH, Lk, 64), torch.randn(B, nH, Lk, 64)
    m = lambda x: max(1, x)  # noqa: E731
    one = [(Lk // 5, Lk - Lk // 7, 0, 0), (0, m(2 * Lk // 3), 0, 0)]
    two = [(0, m(Lk // 10), Lk // 2, Lk), (Lk // 3, min(Lk, Lk // 3 + m(Lk // 4)), Lk - m(Lk // 8), Lk)]
    dvis = torch.rand(B, Lk) < 0.5
    dvis[:, 0] = True
    dense = _dense_of(dvis)
    if Lk > 5:
        dense[:, 5] = -0.75  # a soft bias
    causal = torch.zeros(B, Lk)
    cases = (("causal", causal, {}), ("one", _dense_of(_vis_of(one, Lk)), dict(iv=one)), ("two", _dense_of(_vis_of(two, Lk)), dict(iv=two)),
             ("dense", dense, dict(dense=dense)))
    for op in (BF16, F16):
        q, k, v = _rnd(q0, op), _rnd(k0, op), _rnd(v0, op)
        s = torch.einsum("bhd,bhkd->bhk", q.double(), k.double())
        for name, add, kw in cases:
            want = torch.einsum("bhk,bhkd->bhd", torch.softmax(s + add[:, None, :].double(), dim=-1), v.double()).reshape(B, -1)
            for form in CACHE_FORMS:
                got = _launch(q, k, v, Lk, form, op, zero_tail=switch and Lk == 14849, **kw)
                assert torch.isfinite(got).all(), (Lk, form, op, name)
                err = float((got.double() - want).abs().max())
                # bf16: the bound of test_single_query_decode_attention_two_intervals_and_dense; fp16: the bound of test_fp16_gpu.py's
                # single-query case (the same with 2^-8 -> 2^-11)
                bound = (2.5 * 2 ** -11 * float(want.abs().max()) + 2e-4) if op == F16 else (2.5 * 2 ** -8 * float(want.abs().max()) + 1e-3)
                assert err < bound, (Lk, form, op, name, err, bound)


@pytest.mark.parametrize("Lk", LENGTHS)
def test_random_operands_against_fp64_softmax(Lk):
    _random_case(Lk, 3, False)


@pytest.mark.parametrize("Lk", LDS_SWITCH)
def test_lds_switch_last_decode_length_and_first_gather_length(Lk):
    """4. 14 848 keys is the last length served by the decode kernel, 14 849 the first on the gather fallback (whose V^T tile tail is zero,
    the engine's invariant for that kernel).  The counting half is test_counting_causal_indicator_bit_exact at these lengths."""
    _random_case(Lk, 1, True)


# ================================================================================================ Part 2: the engine
STEPS = 14
STARTS = [505, 1017, 1529, 2032]


class _Model:
    def __init__(self, d, sd, max_seq, seed):
        self.d, self.V = d, d.vocab
        self.m = util.build_showo(d, sd, max_batch=1, max_seq=max_seq)
        self.eng = self.m.engine()
        g = torch.Generator().manual_seed(seed)
        self.ids = torch.randint(0, d.vocab - 20, (1, 2048), generator=g).to(torch.int64).cuda().contiguous()  # prompts and teacher-forced tokens
        self.side = torch.cuda.Stream()  # the legacy default stream cannot be captured
        self.flag0 = torch.zeros(4, dtype=torch.int32, device="cuda")
        self.memo = {}

    def engine(self):
        self.eng = self.m.engine()
        return self.eng


@pytest.fixture(scope="module")
def tiny():
    d, sd = util.tiny_state()
    T = _Model(d, sd, 2048, 5)
    T.sdt = O.to_torch(sd)
    yield T
    L().call("showo_decode_set_impl", 0)
    L().call("showo_engine_use_intervals", T.eng, None, None)


def _state(T):
    n, p, cap, ep = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    L().call("showo_engine_cache_state", T.eng, C.byref(n), C.byref(p), C.byref(cap), C.byref(ep))
    return n.value, p.value, cap.value, ep.value


def _cache_ptrs(T):
    k, vt, kls, vls = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int64()
    L().call("showo_engine_cache_ptrs", T.eng, C.byref(k), C.byref(vt), C.byref(kls), C.byref(vls))
    return k.value, vt.value, kls.value, vls.value


def _cache(T):
    """(K [nL, nH, cap, 64], V^T [nL, nH * 64, cap]) int16 copies of the engine's decode cache"""
    d, cap = T.d, _state(T)[2]
    k, vt, kls, vls = _cache_ptrs(T)
    per = d.heads * cap * 64
    K = torch.empty((d.layers, d.heads, cap, 64), dtype=torch.int16, device="cuda")
    Vt = torch.empty((d.layers, d.heads * 64, cap), dtype=torch.int16, device="cuda")
    for li in range(d.layers):
        L().call("showo_copy_b128", k + 2 * li * kls, L().ptr(K[li]), per * 2, S())
        L().call("showo_copy_b128", vt + 2 * li * vls, L().ptr(Vt[li]), per * 2, S())
    torch.cuda.synchronize()
    return K, Vt


def _poison(T, P0, pattern):
    """NaN patterns into K rows [P0, cap) and V^T columns [64 ceil(P0 / 64), cap) of every layer, through the cache pointers"""
    K, Vt = _cache(T)
    K[:, :, P0:] = pattern
    Vt[..., _ceil64(P0):] = pattern
    k, vt, kls, vls = _cache_ptrs(T)
    per = K[0].numel()
    for li in range(T.d.layers):
        L().call("showo_copy_b128", L().ptr(K[li]), k + 2 * li * kls, per * 2, S())
        L().call("showo_copy_b128", L().ptr(Vt[li]), vt + 2 * li * vls, per * 2, S())
    torch.cuda.synchronize()


def _two_interval_rows(P0):
    """prompt rows under showo_engine_use_intervals: row r sees [0, 3) and [20, r + 1) (causal below row 40)"""
    r = torch.arange(P0)
    iv = torch.stack([torch.zeros_like(r), torch.where(r < 40, r + 1, torch.full_like(r, 3)), torch.where(r < 40, 0 * r, 0 * r + 20),
                      torch.where(r < 40, 0 * r, r + 1)], dim=1)
    return iv.to(torch.int32).cuda().contiguous()


def _prefill(T, P0, intervals=False):
    ids = T.ids[:, :P0].contiguous()
    lg = torch.empty((T.V,), dtype=torch.float32, device="cuda")
    iv = _two_interval_rows(P0) if intervals else None
    if intervals:
        L().call("showo_engine_use_intervals", T.eng, L().ptr(iv), L().ptr(T.flag0))
    try:
        L().call("showo_engine_prefill", T.eng, L().ptr(ids), None, None, P0, L().ptr(lg), S())
        torch.cuda.synchronize()
    finally:
        if intervals:
            L().call("showo_engine_use_intervals", T.eng, None, None)
    assert _state(T)[0] == P0
    return lg


def _greedy(T, P0, graph, intervals=False, poison=None):
    """prefill P0 rows, then STEPS greedy steps in ONE call (device-side position, load bound P0 + STEPS): tokens, last logits row, cache"""
    lg = _prefill(T, P0, intervals)
    if poison is not None:
        _poison(T, P0, poison)
    tok = T.ids[0, P0:P0 + 1].clone()
    out = torch.empty((STEPS,), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(T.side):
        L().call("showo_engine_decode_greedy", T.eng, L().ptr(tok), STEPS, L().ptr(out), L().ptr(lg), graph, S())
    torch.cuda.synchronize()
    assert _state(T)[0] == P0 + STEPS
    return out.tolist(), lg.clone(), _cache(T)


def _steps(T, P0, feed, intervals=False, poison=None):
    """prefill P0 rows, then one showo_engine_decode_step per token of `feed` (exact length): arg-max tokens, every logits row"""
    lg = _prefill(T, P0, intervals)
    if poison is not None:
        _poison(T, P0, poison)
    nxt = torch.empty((1,), dtype=torch.int64, device="cuda")
    toks, rows = [], []
    for t in feed:
        tok = torch.tensor([int(t)], dtype=torch.int64, device="cuda")
        L().call("showo_engine_decode_step", T.eng, L().ptr(tok), None, L().ptr(lg), S())
        L().call("showo_argmax_f32", L().ptr(lg), T.V, L().ptr(nxt), S())
        torch.cuda.synchronize()
        toks.append(int(nxt))
        rows.append(lg.clone())
    return toks, rows


def _teacher(T, P0, n, impl=0):
    """logits rows of n teacher-forced step calls from P0 (tokens = T.ids[P0 : P0 + n]) under decode layer form `impl`, computed once"""
    key = ("teacher", P0, n, impl)
    if key not in T.memo:
        L().call("showo_decode_set_impl", impl)
        try:
            T.memo[key] = _steps(T, P0, T.ids[0, P0:P0 + n].tolist())[1]
        finally:
            L().call("showo_decode_set_impl", 0)
    return T.memo[key]


def _clean_greedy(T, P0):
    """the graph-replayed greedy run of test 5 on a clean cache, computed once: (tokens, last logits row, cache)"""
    key = ("greedy", P0)
    if key not in T.memo:
        T.memo[key] = _greedy(T, P0, 1)
    return T.memo[key]


def _same_run(a, b, n, what):
    assert a[0] == b[0], what
    assert torch.isfinite(a[1]).all() and torch.equal(a[1], b[1]), (what, float((a[1] - b[1]).abs().max()))
    assert torch.equal(a[2][0][:, :, :n], b[2][0][:, :, :n]), (what, "K rows")
    assert torch.equal(a[2][1][..., :n], b[2][1][..., :n]), (what, "V^T columns")


def _three_forms(T, P0, intervals=False, poison=None):
    g = _greedy(T, P0, 1, intervals, poison) if (intervals or poison is not None) else _clean_greedy(T, P0)
    e = _greedy(T, P0, 0, intervals, poison)
    feed = [int(T.ids[0, P0])] + g[0][:-1]
    toks, rows = _steps(T, P0, feed, intervals, poison)
    s = (toks, rows[-1], _cache(T))
    return g, e, s


@pytest.mark.parametrize("P0", STARTS)
def test_hint_bound_equals_exact_bound(tiny, P0):
    """5. decode_greedy as graph replay and as eager steps (device-side position, loads bounded by Lhint = P0 + 14 and clamped onto it)
    against 14 decode_step calls fed the same tokens (exact length): equal tokens, last logits bits and cache bits over [0, P0 + 14)"""
    g, e, s = _three_forms(tiny, P0)
    _same_run(e, g, P0 + STEPS, ("eager", P0))
    _same_run(s, g, P0 + STEPS, ("step calls", P0))


def test_hint_bound_equals_exact_bound_two_interval_prompt(tiny):
    """5 under showo_engine_use_intervals: the new token's mask row has two runs, [0, 3) and [20, pos]"""
    g, e, s = _three_forms(tiny, 1017, intervals=True)
    _same_run(e, g, 1017 + STEPS, "eager")
    _same_run(s, g, 1017 + STEPS, "step calls")
    assert g[0] != _clean_greedy(tiny, 1017)[0] or not torch.equal(g[1], _clean_greedy(tiny, 1017)[1])  # the mask took effect


@pytest.mark.parametrize("P0", STARTS)
def test_fused_layer_equals_seven_launch_layer_at_every_step(tiny, P0):
    """6. the fused instance (newest key / value in LDS; from position 1024 on the newest key is the tail loop's k != pos case) against
    the plain instance behind showo_attn_fwd that Part 1 checks exactly: equal logits bits at every teacher-forced step"""
    plain = _teacher(tiny, P0, STEPS, impl=1)
    fused = _teacher(tiny, P0, STEPS, impl=0)
    for i, (a, b) in enumerate(zip(plain, fused)):
        assert torch.isfinite(b).all(), (P0, i)
        assert torch.equal(a, b), (P0, i, float((a - b).abs().max()))


@pytest.mark.parametrize("P0", STARTS)
def test_stale_cache_rows_never_reach_a_result(tiny, P0):
    """7. NaN in every K row [P0, cap) and V^T column [64 ceil(P0 / 64), cap) after the prefill: tokens and logits bits of the clean run
    in all three forms, and the slots at or beyond P0 + 14 still hold the pattern"""
    T = tiny
    clean = _clean_greedy(T, P0)
    pat = NAN_BITS[BF16]
    for name, run in zip(("graph", "eager", "step calls"), _three_forms(T, P0, poison=pat)):
        _same_run(run, clean, P0 + STEPS, (name, P0))
        K, Vt = run[2]
        assert (K[:, :, P0 + STEPS:] == pat).all(), (name, P0)
        assert (Vt[..., max(_ceil64(P0), P0 + STEPS):] == pat).all(), (name, P0)


def test_full_cache_last_position_succeeds_and_the_next_step_is_refused(tiny):
    """8. step calls from 2040 up to cache length 2048: position 2047 succeeds, the next returns 5 with the cache state unchanged"""
    T = tiny
    T.memo.pop(("teacher", 2040, 8, 0), None)  # run it here (again): the cache must hold the 2048 rows afterwards
    rows = _teacher(T, 2040, 8)
    assert len(rows) == 8 and all(torch.isfinite(r).all() for r in rows)
    before = _state(T)
    assert before[0] == 2048
    tok = T.ids[0, :1].clone()
    lg = torch.empty((T.V,), dtype=torch.float32, device="cuda")
    rc = L().load().showo_engine_decode_step(T.eng, L().ptr(tok), None, L().ptr(lg), S())
    torch.cuda.synchronize()
    assert rc == 5
    assert _state(T) == before


def test_teacher_forced_logits_against_the_fp32_oracle(tiny):
    """9. step-call logits at positions 511, 512, 1023, 1024, 1025 and 2047 against O.showo_logits of the same 2048-token sequence, at
    the gate tests/test_modules_gpu.py applies to this model's bf16 logits (REL_RMS 1e-2, REL_MAX 3e-2).
    Measured on an MI355X (rel_max / rel_rms): 511: 4.1e-3 / 3.6e-3, 512: 3.1e-3 / 3.8e-3, 1023: 4.6e-3 / 4.0e-3, 1024: 3.6e-3 / 3.8e-3,
    1025: 3.1e-3 / 3.9e-3, 2047: 3.2e-3 / 3.7e-3; the test prints them as [parity] lines."""
    T = tiny
    REL_RMS, REL_MAX = 1e-2, 3e-2
    seq = T.ids.cpu()
    n = seq.shape[1]
    cm = torch.where(torch.tril(torch.ones(n, n, dtype=torch.bool)), torch.zeros(()), torch.full((), O.NEG_MASK))[None, None]
    ref = O.showo_logits(T.sdt, T.d, seq, attention_mask=cm)[0]
    runs = {505: _teacher(T, 505, STEPS), 1017: _teacher(T, 1017, STEPS), 2040: _teacher(T, 2040, 8)}
    for pos, P0 in ((511, 505), (512, 505), (1023, 1017), (1024, 1017), (1025, 1017), (2047, 2040)):
        got = runs[P0][pos - P0].cpu()
        rmax, rrms = util.relerr(got, ref[pos])
        print(f"[parity] tiny teacher-forced decode step at position {pos} vs the fp32 oracle: rel_max={rmax:.3e} rel_rms={rrms:.3e}")
        assert rrms <= REL_RMS and rmax <= REL_MAX, (pos, rmax, rrms)


def _batch_greedy(T, begin, prompts, first, cap, graph=1):
    """prompts[slot] = ids [1, n]; first[slot] = the token fed first.  (tokens [slot][STEPS], last logits rows [slot, V])"""
    n = len(prompts)
    L().call(begin, T.eng, n, cap)
    lgs = torch.empty((n, T.V), dtype=torch.float32, device="cuda")
    for b, p in enumerate(prompts):
        L().call("showo_engine_batch_prefill", T.eng, b, L().ptr(p.contiguous()), None, None, p.shape[1], L().ptr(lgs[b]), S())
    tok = torch.tensor(first, dtype=torch.int64, device="cuda")
    out = torch.empty((n, STEPS), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(T.side):
        L().call("showo_engine_batch_decode_greedy", T.eng, L().ptr(tok), STEPS, L().ptr(out), L().ptr(lgs), graph, S())
    torch.cuda.synchronize()
    return out.tolist(), lgs.clone()


def test_batched_slots_give_the_bits_of_their_batch1_runs(tiny):
    """10a. four slots prefilled at 30, 505, 1017 and 1529 rows, 14 greedy steps: lk_max is far above the short slots' lengths, so the
    clamp and the `live` predicate carry the result -- every slot gives the tokens and last logits bits of its own batch-1 run"""
    T = tiny
    lens = [30, 505, 1017, 1529]
    single = [_clean_greedy(T, n) for n in lens]
    for graph in (1, 0):
        toks, lgs = _batch_greedy(T, "showo_engine_batch_begin", [T.ids[:, :n] for n in lens], [int(T.ids[0, n]) for n in lens], 2048, graph)
        for b, n in enumerate(lens):
            assert toks[b] == single[b][0], (graph, n)
            assert torch.equal(lgs[b], single[b][1]), (graph, n, float((lgs[b] - single[b][1]).abs().max()))


def test_wide_slots_are_slot_independent_across_lengths(tiny):
    """10b. nine wide slots (the MFMA step) at lengths on both sides of 512 / 1024 / 1536, run twice with the requests permuted over the
    slots: the wide contract is slot independence and determinism, so every request gives equal tokens and logits bits in both runs"""
    T = tiny
    lens = [30, 505, 1017, 1529, 64, 512, 1024, 1536, 777]
    reqs = [torch.roll(T.ids, 37 * r, dims=1)[:, :n].contiguous() for r, n in enumerate(lens)]
    first = [int(T.ids[0, (5 * r + 1) % 2048]) for r in range(len(lens))]
    runs = []
    for order in (list(range(9)), [4, 8, 0, 6, 2, 7, 1, 3, 5]):
        toks, lgs = _batch_greedy(T, "showo_engine_batch_begin_wide", [reqs[r] for r in order], [first[r] for r in order], 2048)
        assert torch.isfinite(lgs).all()
        runs.append({r: (toks[slot], lgs[slot]) for slot, r in enumerate(order)})
    for r in range(9):
        assert runs[0][r][0] == runs[1][r][0], (r, lens[r])
        assert torch.equal(runs[0][r][1], runs[1][r][1]), (r, lens[r])


@pytest.mark.parametrize("P0", [1017])
def test_fp16_mode_hint_bound_and_fused_layer_across_1024(tiny, P0):
    """5 and 6 once more under precision 2 (the fp16 instances of the same kernels), across the 1023 / 1024 boundary"""
    T = tiny
    T.m.set_precision(2)
    try:
        T.engine()
        g = _greedy(T, P0, 1)
        e = _greedy(T, P0, 0)
        toks, rows = _steps(T, P0, [int(T.ids[0, P0])] + g[0][:-1])
        _same_run(e, g, P0 + STEPS, "eager")
        _same_run((toks, rows[-1], _cache(T)), g, P0 + STEPS, "step calls")
        # 6: at this width the two forms end in different lm_head launches under precision 2 (engine.hip head_rows: the fused LayerNorm +
        # (hi, lo) GEMV against the [hi | hi | lo] GEMM), whose fp32 sums differ in order, so the logits are not the place to compare.
        # The caches are: layer 1's K / V^T rows of every step are functions of layer 0's attention output of that step.  (Logits bits
        # of the forms under precision 2 are compared at full width, where both heads are one product: test 11.)
        feed = T.ids[0, P0:P0 + STEPS].tolist()
        fused = _steps(T, P0, feed)[1]
        cf = _cache(T)
        L().call("showo_decode_set_impl", 1)
        plain = _steps(T, P0, feed)[1]
        cp = _cache(T)
        assert all(torch.isfinite(r).all() for r in fused + plain)
        assert torch.equal(cf[0][:, :, :P0 + STEPS], cp[0][:, :, :P0 + STEPS]) and torch.equal(cf[1][..., :P0 + STEPS], cp[1][..., :P0 + STEPS])
    finally:
        L().call("showo_decode_set_impl", 0)
        T.m.set_precision(0)
        T.engine()


# ------------------------------------------------------------------------------------------------ 11. full width
@pytest.fixture(scope="module")
def wide_model():
    """H 2048, F 8192, 2 layers, vocabulary 58 498: the smallest full-width model (tests/test_mmu_nucleus_gpu.py)"""
    d = Wt.ShowoDims(layers=2)
    sd = Wt.make_showo_state(d, seed=11)
    T = _Model(d, sd, 1152, 3)
    del sd
    yield T
    L().call("showo_decode_set_impl", 0)
    T.m.set_precision(0)


@pytest.mark.parametrize("precision", [0, 2])
def test_full_width_decode_forms_equal_bits_across_1024(wide_model, precision):
    """11. At H 2048 / F 8192 the default layer (impl 0) runs the attention inside the co-scheduled launch attn_decode_co_kernel: against
    the chain (impl 2) and the seven-launch layer (impl 1) from 1017 rows over 14 steps, as step calls and as graph replay -- equal bits.
    Then the batched co-scheduled launch (attn_decode_coB_kernel), 3 slots at 505 / 1017 / 1040 rows, against the three batch-1 runs."""
    T = wide_model
    T.m.set_precision(precision)
    T.engine()
    P0 = 1017
    feed = T.ids[0, P0:P0 + STEPS].tolist()
    runs, greedy = {}, {}
    try:
        for impl in (1, 2, 0):
            L().call("showo_decode_set_impl", impl)
            runs[impl] = _steps(T, P0, feed)[1]
            greedy[impl] = _greedy(T, P0, 1)[:2]
    finally:
        L().call("showo_decode_set_impl", 0)
    for impl in (2, 0):
        for i, (a, b) in enumerate(zip(runs[1], runs[impl])):
            assert torch.isfinite(b).all() and torch.equal(a, b), (impl, i, float((a - b).abs().max()))
        assert greedy[impl][0] == greedy[1][0], impl
        assert torch.equal(greedy[impl][1], greedy[1][1]), impl
    lens = [505, 1017, 1040]
    single = [greedy[0] if n == P0 else _greedy(T, n, 1)[:2] for n in lens]
    toks, lgs = _batch_greedy(T, "showo_engine_batch_begin", [T.ids[:, :n] for n in lens], [int(T.ids[0, n]) for n in lens], 1152)
    for b, n in enumerate(lens):
        assert toks[b] == single[b][0], n
        assert torch.equal(lgs[b], single[b][1]), (n, float((lgs[b] - single[b][1]).abs().max()))
