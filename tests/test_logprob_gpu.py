"""GPU tests of showo_logprob_rows (csrc/sample_row.h logprob_row): values against the fp64 reference of tests/logprob_ref.py at the
derived gate, exact ranks, the special targets, every row alignment and stride, and the bits (run to run, and whatever the row's
place in the call and in memory)."""
import numpy as np
import pytest
import torch

import util
import logprob_ref as R

pytestmark = pytest.mark.gpu

POISON = 3.0e38  # what lies between the rows (ld > V) and around the block: a read beyond a row would move the max and the rank


def _run(X, T, ld, off, want_rank=True):
    """the kernel on rows X [n, V] laid out with stride ld at `off` floats behind a 16-byte boundary -> (lp fp32 [n], rank int32 [n])"""
    L = util.lib()
    n, V = X.shape
    buf = torch.full((off + n * ld + 8,), POISON, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    rows = buf[off:off + n * ld].view(n, ld)
    rows[:, :V] = torch.from_numpy(X).cuda()
    t = torch.from_numpy(T).cuda()
    lp = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    rk = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    L.call("showo_logprob_rows", L.ptr(buf[off:]), ld, n, V, L.ptr(t), L.ptr(lp), L.ptr(rk) if want_rank else None, L.stream())
    torch.cuda.synchronize()
    return lp.cpu().numpy(), rk.cpu().numpy()


@pytest.mark.parametrize("V", R.SHAPES_V)
def test_values_ranks_and_special_targets_at_every_layout(V):
    worst = 0.0
    for n in R.SHAPES_N:
        for kind in R.KINDS:
            X, T = R.make_case(kind, V, n)
            lp64, rk64 = R.logprob_rows_ref(X, T)
            first = None
            for ld in (V, V + 3):
                for off in (0, 1):  # off = 1 with ld = V = 58498: rows at 4 and 12 bytes behind a boundary, none aligned
                    lp, rk = _run(X, T, ld, off)
                    assert np.array_equal(rk, rk64.astype(np.int32)), (kind, n, ld, off, rk, rk64)
                    ok = R.within_gate(lp, lp64)
                    assert ok.all(), (kind, n, ld, off, lp[~ok], lp64[~ok])
                    fin = np.isfinite(lp64)
                    if fin.any():
                        worst = max(worst, float(np.max(np.abs(lp[fin] - lp64[fin]) / (R.ABS + R.REL * np.abs(lp64[fin])))))
                    # the bits do not depend on where the rows lie
                    if first is None:
                        first = lp
                    assert np.array_equal(first.view(np.int32), lp.view(np.int32)), (kind, n, ld, off)
            if kind == "ignore":
                assert (lp == 0.0).all() and (rk == -1).all()
            if kind == "beyond":
                assert np.isnan(lp).all() and (rk == -1).all()
            if kind == "equal":
                assert (rk == 0).all()
    print(f"[logprob] V={V}: the kernel uses {worst:.3f} of the gate")


def test_rank_pointer_is_optional_and_no_rows_launch_nothing():
    X, T = R.make_case("normal", 4099, 3)
    lp, rk = _run(X, T, 4099, 0, want_rank=False)
    assert (rk == 7).all() and R.within_gate(lp, R.logprob_rows_ref(X, T)[0]).all()
    L = util.lib()
    L.call("showo_logprob_rows", None, 8, 0, 8, None, None, None, L.stream())
    with pytest.raises(RuntimeError):
        L.call("showo_logprob_rows", L.ptr(torch.zeros(8, device="cuda")), 4, 1, 8, L.ptr(torch.zeros(1, dtype=torch.int64, device="cuda")),
               L.ptr(torch.zeros(1, device="cuda")), None, L.stream())  # ld < V


@pytest.mark.parametrize("V", [65, 4099, 58498])
def test_bits_repeat_and_do_not_depend_on_the_row_s_place_in_the_call(V):
    for kind in ("normal", "plus1e4", "neginf"):
        X, T = R.make_case(kind, V, 37, seed=3)
        a, ra = _run(X, T, V + 3, 1)
        b, rb = _run(X, T, V + 3, 1)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(ra, rb), kind
        for off in (0, 1, 2, 3):  # row 17 scored alone, at every alignment
            c, rc = _run(X[17:18], T[17:18], V, off)
            assert c.view(np.int32)[0] == a.view(np.int32)[17] and rc[0] == ra[17], (kind, off)
