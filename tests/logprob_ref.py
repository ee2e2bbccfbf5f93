"""fp64 numpy reference of the token log-probability kernel (csrc/sample_row.h logprob_row, include/showo_hip.h showo_logprob_rows) and
the input families its tests share.

    lp   = x[t] - max(x) - log sum exp(x - max(x))      the log-softmax of the raw logits at the target
    rank = #{ i : x[i] > x[t] }                         strict
    t < 0: (0.0, -1)        t >= V: (NaN, -1)           -inf entries add 0 to the sum; a row of -inf alone gives NaN
"""
import numpy as np

# the kernel's gate: |lp - lp64| <= ABS + REL |lp64|.  Derived, not measured: one fp32 rounding on x[t] - max (6e-8 relative), a sum of up
# to 58 498 non-negative terms with relative error about (log2 V + 2) 2^-24 = 1.1e-6 for a float tree (the kernel's integer sum: V 2^-40 =
# 5e-8), one fp32 log: roughly five times headroom
ABS, REL = 1e-5, 1e-6


def logprob_ref(x, t):
    """(lp, rank) of target t under the logits row x, computed in float64"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    V, t = x.shape[0], int(t)
    if t < 0:
        return 0.0, -1
    if t >= V:
        return float("nan"), -1
    m = x.max()
    rank = int((x > x[t]).sum())
    if not np.isfinite(m):
        return float("nan"), rank
    with np.errstate(divide="ignore"):
        return float(x[t] - m - np.log(np.exp(x - m).sum())), rank


def logprob_rows_ref(X, T):
    """rows X [n, V], targets T [n] -> (lp float64 [n], rank int64 [n])"""
    out = [logprob_ref(x, t) for x, t in zip(np.asarray(X), np.asarray(T))]
    return np.array([o[0] for o in out], dtype=np.float64), np.array([o[1] for o in out], dtype=np.int64)


def within_gate(got, want):
    """elementwise: got (fp32 results) meets want (fp64 reference) at the kernel's gate; -inf and NaN must be reproduced as such"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    ok = np.zeros(want.shape, dtype=bool)
    nan, ninf = np.isnan(want), np.isneginf(want)
    fin = ~(nan | ninf)
    ok[nan] = np.isnan(got[nan])
    ok[ninf] = np.isneginf(got[ninf])
    ok[fin] = np.abs(got[fin] - want[fin]) <= ABS + REL * np.abs(want[fin])
    return ok


SHAPES_V = (1, 7, 63, 64, 65, 1023, 4099, 58498)
SHAPES_N = (1, 3, 37)
KINDS = ("normal", "plus1e4", "minus1e4", "neginf", "equal", "ties", "ignore", "beyond")


def make_case(kind, V, n, seed=0):
    """(X fp32 [n, V], T int64 [n]) of one input family.
    normal: N(0, 3) rows, targets 0, V - 1, then random; plus1e4 / minus1e4: the same rows shifted (targets V - 1, 0, then random);
    neginf: a third of the entries -inf (entry 0 stays finite), every second target one of them; equal: an all-equal row (lp = -log V,
    rank 0); ties: the target's value present three times; ignore: every target -100; beyond: every target V."""
    rs = np.random.RandomState(1000 * seed + 7 * V + n)
    X = (3.0 * rs.standard_normal((n, V))).astype(np.float32)
    T = rs.randint(0, V, size=n).astype(np.int64)
    ends = [0, V - 1]
    if kind in ("plus1e4", "minus1e4"):
        X = (X + np.float32(1e4 if kind == "plus1e4" else -1e4)).astype(np.float32)
        ends = ends[::-1]
    for r in range(min(n, 2)):
        T[r] = ends[r]
    if kind == "neginf":
        hole = rs.rand(n, V) < 1.0 / 3.0
        hole[:, 0] = False
        X[hole] = -np.inf
        for r in range(n):
            idx = np.nonzero(hole[r] if r % 2 == 0 else ~hole[r])[0]
            if idx.size:
                T[r] = idx[rs.randint(idx.size)]
    elif kind == "equal":
        X[:] = np.float32(1.25)
    elif kind == "ties" and V >= 3:
        for r in range(n):
            others = rs.permutation(np.delete(np.arange(V), T[r]))[:2]
            X[r, others] = X[r, T[r]]
    elif kind == "ignore":
        T[:] = -100
    elif kind == "beyond":
        T[:] = V
    return X, T
