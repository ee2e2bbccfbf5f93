"""GPU tests of the beam kernels through the C ABI (csrc/beam.hip): showo_beam_select against the numpy restatement of
tests/beam_ref.py -- bit for bit given the device's normaliser, at every row alignment -- and showo_kv_permute_rows against the copy it
stands for, on maps an in-place copy gets wrong."""
import numpy as np
import pytest
import torch

import util
import beam_ref as R
import logprob_ref as LP

pytestmark = pytest.mark.gpu

SENT_F, SENT_I = np.float32(-777.25), -123456789


def _select(X, cum, B, base):
    """the kernel on rows placed `base` floats into a buffer with a leading dimension that is 2 (mod 4) floats: rows alternate between
    8- and 16-byte alignment, `base` = 2 swaps which is which.  Returns (norm [nb, 2], score, beam, token) with the sentinels checked."""
    L = util.lib()
    nb, V = X.shape
    ld = (V + 3) // 4 * 4 + 2
    buf = torch.full((base + nb * ld + 8,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[base:base + nb * ld].view(nb, ld)
    view[:, :V] = torch.from_numpy(X).cuda()
    assert (view.data_ptr() % 16 == 0) == (base % 4 == 0)
    cum_d = torch.from_numpy(cum).cuda()
    norm = torch.full((nb * 2 + 4,), float(SENT_F), dtype=torch.float32, device="cuda")
    cand = torch.full((2 * B * 3 + 6,), SENT_I, dtype=torch.int32, device="cuda")
    ws = torch.empty((nb * 2 * B * 2,), dtype=torch.float32, device="cuda")
    L.call("showo_beam_select", view.data_ptr(), ld, nb, V, L.ptr(cum_d), B, L.ptr(norm), L.ptr(cand), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    norm, cand = norm.cpu().numpy(), cand.cpu().numpy()
    assert (norm[nb * 2:] == SENT_F).all() and (cand[2 * B * 3:] == SENT_I).all(), "wrote behind norm / cand"
    c = cand[:2 * B * 3].reshape(2 * B, 3)
    return norm[:nb * 2].reshape(nb, 2), c[:, 0].copy().view(np.float32), c[:, 1].copy(), c[:, 2].copy()


def _norm64(X):
    X = X.astype(np.float64)
    m = X.max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return m, np.log(np.exp(X - m[:, None]).sum(axis=1))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


FAMILIES = ("normal", "plus1e4", "minus1e4", "neginf", "equal", "ties")
NB_B = (1, 2, 3, 4, 8)


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("V", [16, 63, 64, 65, 4099, 58498])
def test_select_is_select_ref_bit_for_bit_at_every_alignment(V, kind):
    rs = np.random.RandomState(V + len(kind))
    for nb in NB_B:
        X, _ = LP.make_case(kind, V, nb, seed=3)
        cum = (-4.0 * rs.rand(nb)).astype(np.float32)
        if nb > 1:  # a planted tie across beams: two beams with the same row and the same cumulative score
            X[nb - 1] = X[0]
            cum[nb - 1] = cum[0]
        m64, ls64 = _norm64(X)
        for B in NB_B:
            if 2 * B > V:
                continue
            outs = [_select(X, cum, B, base) for base in (0, 2)]
            norm, score, beam, token = outs[0]
            assert np.array_equal(norm[:, 0], X.max(axis=1)), (nb, B)
            assert LP.within_gate(norm[:, 1], ls64).all(), (nb, B, norm[:, 1], ls64)
            ws, wb, wt = R.select_ref(X, cum, norm, B)
            assert np.array_equal(_bits(score), _bits(ws)) and np.array_equal(beam, wb) and np.array_equal(token, wt), (nb, B)
            assert ((token >= 0) & (token < V)).all()
            # the other alignment: the same bits, normaliser included
            for a, b in zip(outs[0], outs[1]):
                assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
            # (score descending, beam ascending, token ascending)
            keys = [(-float(s), int(b_), int(t)) for s, b_, t in zip(score, beam, token)]
            assert keys == sorted(keys), (nb, B)
            if kind == "equal" and nb == 1:
                assert token.tolist() == list(range(2 * B)) and (beam == 0).all()
            if kind == "neginf":
                assert np.isfinite(score[0])


@pytest.mark.parametrize("V", [65536, 65537, 70001])
def test_select_on_both_sides_of_the_register_threshold(V):
    """rows of up to 65536 entries are selected from registers, longer ones are re-read per pass: the same contract on both sides"""
    for kind in ("normal", "ties"):
        X, _ = LP.make_case(kind, V, 3, seed=4)
        X[2] = X[0]
        cum = np.array([-0.25, -1.0, -0.25], dtype=np.float32)
        for B in (2, 8):
            outs = [_select(X, cum, B, base) for base in (0, 2)]
            norm, score, beam, token = outs[0]
            assert LP.within_gate(norm[:, 1], _norm64(X)[1]).all()
            ws, wb, wt = R.select_ref(X, cum, norm, B)
            assert np.array_equal(_bits(score), _bits(ws)) and np.array_equal(beam, wb) and np.array_equal(token, wt), (kind, B)
            for a, b in zip(outs[0][1:], outs[1][1:]):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_select_orders_ties_by_beam_then_token():
    V, nb, B = 64, 4, 4
    X = np.full((nb, V), np.float32(0.5))
    cum = np.zeros(nb, dtype=np.float32)
    _, score, beam, token = _select(X, cum, B, 0)
    assert (beam == 0).all() and token.tolist() == list(range(2 * B)) and len(set(_bits(score).tolist())) == 1
    X[:, 10] = X[:, 3] = 2.0  # the two best of every row tie across the rows
    _, score, beam, token = _select(X, cum, B, 2)
    assert list(zip(beam.tolist(), token.tolist())) == [(0, 3), (0, 10), (1, 3), (1, 10), (2, 3), (2, 10), (3, 3), (3, 10)]
    cum[2] = 1.0  # a better beam goes first, with all it has
    _, score, beam, token = _select(X, cum, B, 0)
    assert list(zip(beam.tolist(), token.tolist()))[:4] == [(2, 3), (2, 10), (0, 3), (0, 10)]
    # a -inf logit scores -inf and is never taken while finite ones are left
    X[:] = -np.inf
    X[:, 5:5 + 2 * B] = 1.0
    _, score, beam, token = _select(X, np.zeros(nb, dtype=np.float32), B, 0)
    assert np.isfinite(score).all() and (beam == 0).all() and token.tolist() == list(range(5, 5 + 2 * B))
    X[0, 6:] = -np.inf  # beam 0 has one finite entry left and V = 64 >= 2B: the rest of its own candidates are -inf
    _, score, beam, token = _select(X[:1], np.zeros(1, dtype=np.float32), B, 0)
    assert token[0] == 5 and np.isneginf(score[1:]).all() and token[1:].tolist() == [0, 1, 2, 3, 4, 6, 7]


@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
@pytest.mark.parametrize("V", [65, 4099])
def test_a_row_without_a_normaliser_poisons_only_its_own_candidates(V, poison):
    nb, B = 3, 2
    X, _ = LP.make_case("normal", V, nb, seed=5)
    cum = np.array([-1.0, -0.5, -2.0], dtype=np.float32)
    clean = _select(X, cum, B, 0)
    for bad in range(nb):
        Y = X.copy()
        Y[bad, V // 2] = poison
        for base in (0, 2):
            norm, score, beam, token = _select(Y, cum, B, base)
            assert np.isnan(norm[bad, 1])
            others = [b for b in range(nb) if b != bad]
            assert np.array_equal(_bits(norm[others]), _bits(clean[0][others]))
            ws, wb, wt = R.select_ref(Y, cum, norm, B)
            assert np.array_equal(_bits(score), _bits(ws)) and np.array_equal(beam, wb) and np.array_equal(token, wt)
            assert np.isfinite(score).all() and (beam != bad).all() and ((token >= 0) & (token < V)).all()
    # every row poisoned: NaN scores, token -1, never an out-of-range token
    Y = X.copy()
    Y[:, 1] = poison
    norm, score, beam, token = _select(Y, cum, B, 0)
    assert np.isnan(score).all() and (token == -1).all() and beam.tolist() == [0] * (2 * B)
    Y[:] = -np.inf  # rows of -inf alone have no normaliser either
    norm, score, beam, token = _select(Y, cum, B, 2)
    assert np.isnan(score).all() and (token == -1).all()


def test_select_refuses_bad_arguments():
    L = util.lib()
    x = torch.zeros((8, 64), dtype=torch.float32, device="cuda")
    o = torch.zeros((512,), dtype=torch.float32, device="cuda")
    for nb, V, B in ((0, 64, 1), (9, 64, 1), (1, 64, 0), (1, 64, 9), (1, 15, 8), (1, 1, 1)):
        with pytest.raises(RuntimeError):
            L.call("showo_beam_select", L.ptr(x), 64, nb, V, L.ptr(o), B, L.ptr(o), L.ptr(o), L.ptr(o), L.stream())


# ---- showo_kv_permute_rows --------------------------------------------------------------------------------------------------------------
NL, NH = 2, 2


def _maps(B, rs):
    ident = list(range(B))
    swap = ident[:]
    swap[0], swap[1] = 1, 0
    cyc = ident[:]
    if B >= 3:
        cyc[0], cyc[1], cyc[2] = 1, 2, 0
    else:
        cyc = swap[::1]
    return {"identity": ident, "swap": swap, "cycle": cyc, "all_from_last": [B - 1] * B, "random": rs.randint(0, B, size=B).tolist()}


def _slots(B, cap, r0, r1, rs):
    """K [B, NL, NH, cap, 64] and V^T [B, NL, NH, 64, cap] bit patterns: distinct per slot in [r0, r1), identical below r0 (the
    kernel's stated precondition), NaN bits (distinct per slot) from r1 on"""
    k = rs.randint(0, 0x7f00, size=(B, NL, NH, cap, 64)).astype(np.uint16)
    vt = rs.randint(0, 0x7f00, size=(B, NL, NH, 64, cap)).astype(np.uint16)
    k[:, :, :, :r0] = k[:1, :, :, :r0]
    vt[..., :r0] = vt[:1, ..., :r0]
    for b in range(B):
        k[b, :, :, r1:] = 0x7fc0 + b
        vt[b, ..., r1:] = 0x7fc0 + b
    return k, vt


def _permute(k, vt, cap, parent, r0, r1, span, r1_dev=None):
    L = util.lib()
    B = k.shape[0]
    kd, vd = torch.from_numpy(k.view(np.int16)).cuda(), torch.from_numpy(vt.view(np.int16)).cuda()
    per = NL * NH * cap * 64
    ktab = torch.tensor([kd.data_ptr() + 2 * per * b for b in range(B)], dtype=torch.int64, device="cuda")
    vtab = torch.tensor([vd.data_ptr() + 2 * per * b for b in range(B)], dtype=torch.int64, device="cuda")
    n = L.load().showo_kv_permute_stage_elems(NL, NH, B, span)
    assert n == B * NL * NH * 64 * (8 * ((span + 7) // 8) + 8)
    stage = [torch.full((n + 64,), 0x5a5a, dtype=torch.int16, device="cuda") for _ in range(2)]
    pd = torch.tensor(parent, dtype=torch.int32, device="cuda")
    rd = torch.tensor([r1 if r1_dev is None else r1_dev], dtype=torch.int32, device="cuda")
    ls = NH * cap * 64
    L.call("showo_kv_permute_rows", L.ptr(ktab), L.ptr(vtab), cap, ls, ls, NL, NH, B, L.ptr(pd), r0, L.ptr(rd), L.ptr(stage[0]),
           L.ptr(stage[1]), span, L.stream())
    torch.cuda.synchronize()
    for s in stage:
        assert (s[n:] == 0x5a5a).all(), "wrote behind the staging buffer"
    return kd.cpu().numpy().view(np.uint16), vd.cpu().numpy().view(np.uint16)


def _check_permuted(k0, vt0, k1, vt1, parent, r0, r1, what):
    B, cap = k0.shape[0], k0.shape[3]
    c0, c1 = 8 * (r0 // 8), min(cap, 8 * ((r1 + 7) // 8))  # the V^T chunks a moved beam may take whole
    for c, p in enumerate(parent):
        assert np.array_equal(k1[c, :, :, r0:r1], k0[p, :, :, r0:r1]), (what, "K rows", c)
        assert np.array_equal(k1[c, :, :, :r0], k0[c, :, :, :r0]) and np.array_equal(k1[c, :, :, r1:], k0[c, :, :, r1:]), (what, "K outside", c)
        assert np.array_equal(vt1[c, ..., r0:r1], vt0[p, ..., r0:r1]), (what, "V^T columns", c)
        assert np.array_equal(vt1[c, ..., :c0], vt0[c, ..., :c0]) and np.array_equal(vt1[c, ..., c1:], vt0[c, ..., c1:]), (what, "V^T outside", c)
        for lo, hi in ((c0, r0), (r1, c1)):  # inside the chunks, outside the range: the beam's own bits or its parent's
            got = vt1[c, ..., lo:hi]
            assert ((got == vt0[c, ..., lo:hi]) | (got == vt0[p, ..., lo:hi])).all(), (what, "V^T chunk slack", c)


@pytest.mark.parametrize("B", [2, 4, 8])
@pytest.mark.parametrize("cap", [64, 192])
def test_permute_rows_serves_every_parent_map(cap, B):
    rs = np.random.RandomState(cap + B)
    ran = 0
    for r0 in (1, 63, 64, 65):
        for n in (1, 7, 64, 70):
            r1 = r0 + n
            if r1 > cap:
                continue
            k0, vt0 = _slots(B, cap, r0, r1, rs)
            for name, parent in _maps(B, rs).items():
                k1, vt1 = _permute(k0.copy(), vt0.copy(), cap, parent, r0, r1, span=n if (r0 + n) % 2 else n + 9)
                _check_permuted(k0, vt0, k1, vt1, parent, r0, r1, (name, r0, n))
                if name == "identity":
                    assert np.array_equal(k1, k0) and np.array_equal(vt1, vt0)
                ran += 1
    assert ran == (15 if cap == 64 else 80)  # (capacity 64 holds r0 = 1 with 1 or 7 rows and r0 = 63 with 1)


def test_permute_rows_clips_r1_and_ignores_parents_out_of_range():
    rs = np.random.RandomState(9)
    B, cap, r0 = 4, 64, 10
    k0, vt0 = _slots(B, cap, r0, 30, rs)
    # r1 on the device beyond r0 + span: rows [r0, r0 + span) move, nothing behind them
    k1, vt1 = _permute(k0.copy(), vt0.copy(), cap, [1, 0, 3, 2], r0, r0 + 8, span=8, r1_dev=1000)
    _check_permuted(k0, vt0, k1, vt1, [1, 0, 3, 2], r0, r0 + 8, "clip to span")
    # r1 <= r0: nothing moves; a parent outside [0, B) counts as the beam itself
    k1, vt1 = _permute(k0.copy(), vt0.copy(), cap, [1, 0, 3, 2], r0, r0, span=8)
    assert np.array_equal(k1, k0) and np.array_equal(vt1, vt0)
    k1, vt1 = _permute(k0.copy(), vt0.copy(), cap, [7, -1, 2, 100], r0, 30, span=20)
    assert np.array_equal(k1, k0) and np.array_equal(vt1, vt0)
