"""GPU tests of the logit-adjustment kernels (csrc/logit_adjust.hip: showo_logits_adjust, showo_seen_mark) against the numpy float32
reference of tests/logit_adjust_ref.py, bit for bit (uint32 view): the work is three correctly rounded fp32 operations per element."""
import ctypes as C

import numpy as np
import pytest
import torch

import util
import logit_adjust_ref as R

pytestmark = pytest.mark.gpu

THETAS = (0.5, 1.0, 1.3)
SENTINEL = np.float32(-12345.5)


def _rows(V, n, seed):
    """X fp32 [n, V]: N(0, 3) with +-0 and +-inf sprinkled in"""
    rs = np.random.RandomState(seed)
    X = (3.0 * rs.standard_normal((n, V))).astype(np.float32)
    for val in (0.0, -0.0, np.inf, -np.inf):
        hit = rs.rand(n, V) < 0.03
        X[hit] = np.float32(val)
    return X, rs


def _bias(kind, x, rs):
    """no row, a finite row, a row with -inf (never under a +inf logit: inf - inf is NaN, which is not gated)"""
    if kind == 0:
        return None
    b = rs.standard_normal(x.shape[0]).astype(np.float32)
    b[rs.rand(x.shape[0]) < 0.2] = 0.0
    if kind == 2:
        b[rs.rand(x.shape[0]) < 0.3] = -np.inf
        b[x == np.inf] = 0.5
    return b


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _adjust(L, xd, ld, n, V, seen, seen_ld, mark, pen, bias, active, out, ld_out):
    a_pen = (C.c_float * n)(*pen)
    a_bias = None if bias is None else (C.c_void_p * n)(*[None if b is None else b.data_ptr() for b in bias])
    L.call("showo_logits_adjust", L.ptr(xd), ld, n, V, L.ptr(seen), seen_ld, L.ptr(mark), C.cast(a_pen, C.c_void_p),
           None if a_bias is None else C.cast(a_bias, C.c_void_p), L.ptr(active), L.ptr(out), ld_out, L.stream())
    torch.cuda.synchronize()


def _case(V, n, seed, extra_word=0):
    """inputs of one call: rows, bitmaps with bits at 0, 31, 32, V - 1 and random ones, marks (in the set, outside it, none: -1 / V),
    a penalty and a bias kind per row so that all nine (theta, bias) pairs occur within 9 rows"""
    X, rs = _rows(V, n, seed)
    W = R.words(V) + extra_word
    seen = np.zeros((n, W), dtype=np.uint32)
    marks = np.zeros(n, dtype=np.int64)
    pen, bias = [], []
    for r in range(n):
        ids = [i for i in (0, 31, 32, V - 1) if i < V and (r + i) % 5 != 4] + rs.randint(0, V, size=min(V, 40)).tolist()
        seen[r] = R.bitmap_of(V, ids, W)
        marks[r] = (rs.randint(0, V), ids[0] if ids else 0, -1, V, V - 1, 0)[r % 6]
        pen.append(THETAS[(r + seed) % 3])
        bias.append(_bias(((r + seed) // 3) % 3, X[r], rs))
    return X, seen, marks, pen, bias


def _expect(V, X, seen, marks, pen, bias):
    want = np.empty_like(X)
    after = seen.copy()
    for r in range(X.shape[0]):
        mem = R.members_of(V, seen[r])
        if 0 <= marks[r] < V:
            mem[marks[r]] = True
            after[r] |= R.bitmap_of(V, [marks[r]], seen.shape[1])
        want[r] = R.adjust_ref(X[r], mem, pen[r], bias[r])
    return want, after


@pytest.mark.parametrize("n", [1, 3, 32])
@pytest.mark.parametrize("V", [1, 31, 32, 33, 63, 65, 4099, 58498])
def test_adjust_is_bit_equal_to_the_reference(V, n):
    """ld == V, so the rows alternate in alignment; seeds 0..2 rotate the (theta, bias kind) of every row"""
    L = util.lib()
    for seed in range(3 if n < 9 else 1):
        extra = seed % 2  # seen_ld > ceil(V / 32): the word behind the row's last one stays untouched
        X, seen, marks, pen, bias = _case(V, n, seed, extra)
        want, after = _expect(V, X, seen, marks, pen, bias)
        xd, sd, md = util.dev(X), _i32(seen), util.dev(marks)
        bd = [None if b is None else util.dev(b) for b in bias]
        out = torch.full((n, V), float(SENTINEL), dtype=torch.float32, device="cuda")
        _adjust(L, xd, V, n, V, sd, seen.shape[1], md, pen, bd if any(b is not None for b in bd) else None, None, out, V)
        got = out.cpu().numpy()
        fin = ~np.isnan(want)
        assert np.array_equal(R.bits(got)[fin], R.bits(want)[fin]), (V, n, seed)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(xd.cpu().numpy().view(np.uint32), X.view(np.uint32))  # the raw rows are never written
        # the bitmap afterwards: the old one with the one marked bit ORed in, nothing at positions >= V, other words unchanged
        sa = _u32(sd)
        assert np.array_equal(sa, after), (V, n, seed)
        for r in range(n):
            assert np.nonzero(R.members_of(32 * seen.shape[1], sa[r]))[0].max(initial=0) < V
        # the mark counts as seen in the output whether or not its bit was set before
        for r in range(n):
            m = int(marks[r])
            if 0 <= m < V and np.isfinite(X[r, m]) and X[r, m] != 0 and pen[r] != 1.0 and bias[r] is None:
                assert got[r, m] != X[r, m]
        util.release()


def test_more_rows_than_one_launch_carries():
    L = util.lib()
    V, n = 65, 35
    X, seen, marks, pen, bias = _case(V, n, 1)
    want, after = _expect(V, X, seen, marks, pen, bias)
    sd = _i32(seen)
    out = torch.empty((n, V), dtype=torch.float32, device="cuda")
    _adjust(L, util.dev(X), V, n, V, sd, seen.shape[1], util.dev(marks), pen, [None if b is None else util.dev(b) for b in bias], None, out, V)
    fin = ~np.isnan(want)
    assert np.array_equal(R.bits(out.cpu().numpy())[fin], R.bits(want)[fin])
    assert np.array_equal(_u32(sd), after)


def test_rows_of_another_alignment_than_the_logits():
    """out with ld_out = V + 1 and bias rows that start 1, 2 and 3 elements behind a 16-byte boundary: the element-by-element paths"""
    L = util.lib()
    V, n = 4099, 3
    X, seen, marks, pen, _ = _case(V, n, 2)
    rs = np.random.RandomState(5)
    bias = [_bias(1 + r % 2, X[r], rs) for r in range(n)]
    want, after = _expect(V, X, seen, marks, pen, bias)
    pool = torch.zeros((n, V + 8), dtype=torch.float32, device="cuda")
    bd = []
    for r in range(n):
        pool[r, r + 1:r + 1 + V] = torch.from_numpy(bias[r]).cuda()
        bd.append(pool[r, r + 1:r + 1 + V])
    sd = _i32(seen)
    out = torch.full((n, V + 1), float(SENTINEL), dtype=torch.float32, device="cuda")
    _adjust(L, util.dev(X), V, n, V, sd, seen.shape[1], util.dev(marks), pen, bd, None, out, V + 1)
    got = out.cpu().numpy()
    fin = ~np.isnan(want)
    assert np.array_equal(R.bits(got[:, :V])[fin], R.bits(want)[fin])
    assert (got[:, V] == SENTINEL).all()
    assert np.array_equal(_u32(sd), after)


def test_inactive_rows_are_neither_marked_nor_written():
    L = util.lib()
    V, n = 4099, 3
    X, seen, marks, pen, bias = _case(V, n, 0)
    marks[:] = [7, 8, 9]
    seen[:, 0] &= np.uint32(~np.uint32(0x380))  # bits 7, 8, 9 clear beforehand
    want, after = _expect(V, X, seen, marks, pen, bias)
    sd = _i32(seen)
    out = torch.full((n, V), float(SENTINEL), dtype=torch.float32, device="cuda")
    active = torch.tensor([1, 0, 5], dtype=torch.int32, device="cuda")
    _adjust(L, util.dev(X), V, n, V, sd, seen.shape[1], util.dev(marks), pen, [None if b is None else util.dev(b) for b in bias], active, out, V)
    got, sa = out.cpu().numpy(), _u32(sd)
    fin = ~np.isnan(want)
    for r in (0, 2):
        assert np.array_equal(R.bits(got[r])[fin[r]], R.bits(want[r])[fin[r]])
        assert np.array_equal(sa[r], after[r])
    assert (got[1] == SENTINEL).all() and np.array_equal(sa[1], seen[1])


@pytest.mark.parametrize("V", [33, 58498])
def test_theta_one_without_a_bias_row_is_a_copy(V):
    L = util.lib()
    n = 3
    X, seen, marks, _, _ = _case(V, n, 0)
    seen[:] = np.uint32(0xffffffff)
    seen[:, -1] = R.bitmap_of(V, range(32 * (R.words(V) - 1), V))[-1]  # every token a member, no bit >= V
    out = torch.empty((n, V), dtype=torch.float32, device="cuda")
    _adjust(L, util.dev(X), V, n, V, _i32(seen), seen.shape[1], util.dev(marks), [1.0] * n, None, None, out, V)
    assert np.array_equal(R.bits(out.cpu().numpy()), R.bits(X))


def test_the_error_cases_launch_nothing():
    L = util.lib()
    V, n = 65, 3
    X, seen, marks, pen, _ = _case(V, n, 0)
    xd, sd, md = util.dev(X), _i32(seen), util.dev(marks)
    out = torch.full((n, V), float(SENTINEL), dtype=torch.float32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == SENTINEL).all()
        assert np.array_equal(_u32(sd), seen) and np.array_equal(xd.cpu().numpy().view(np.uint32), X.view(np.uint32))

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="code 1"):
            _adjust(L, xd, V, n, V, sd, seen.shape[1], md, [1.3, bad, 1.0], None, None, out, V)
        untouched()
    with pytest.raises(RuntimeError, match="code 1"):  # out aliasing logits: the same rows, and rows that overlap
        _adjust(L, xd, V, n, V, sd, seen.shape[1], md, pen, None, None, xd, V)
    both = torch.full((2 * n - 1, V), float(SENTINEL), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="code 1"):
        _adjust(L, both[:n], V, n, V, sd, seen.shape[1], md, pen, None, None, both[n - 1:], V)
    assert (both.cpu().numpy() == SENTINEL).all()
    with pytest.raises(RuntimeError, match="code 1"):  # a bitmap row shorter than the vocabulary
        _adjust(L, xd, V, n, V, sd, R.words(V) - 1, md, pen, None, None, out, V)
    untouched()
    _adjust(L, xd, V, 0, V, sd, seen.shape[1], md, [], None, None, out, V)  # no rows: nothing to do, no error
    untouched()


@pytest.mark.parametrize("V", [1, 33, 58498])
def test_seen_mark_sets_the_bits_and_ignores_ids_outside_the_vocabulary(V):
    L = util.lib()
    rs = np.random.RandomState(V)
    ids = np.concatenate([rs.randint(0, V, size=300), [-1, V, V + 31, -100, 0, V - 1, min(31, V - 1), min(32, V - 1)]]).astype(np.int64)
    rs.shuffle(ids)
    W = R.words(V)
    before = np.stack([R.bitmap_of(V, rs.randint(0, V, size=5)), R.bitmap_of(V, [0])])
    sd, idd = _i32(before), util.dev(ids)
    L.call("showo_seen_mark", L.ptr(sd[0]), V, L.ptr(idd), len(ids), L.stream())
    L.call("showo_seen_mark", L.ptr(sd[1]), V, L.ptr(idd), 0, L.stream())  # n == 0 launches nothing
    torch.cuda.synchronize()
    sa = _u32(sd)
    assert np.array_equal(sa[0], before[0] | R.bitmap_of(V, ids)) and np.array_equal(sa[1], before[1])
    assert W == sa.shape[1] and not R.members_of(32 * W, sa[0])[V:].any()
