"""EMA of the weights, restated in numpy, independent of the package and of torch (reference models/training_utils.py:141-177).

    decay_t    get_decay(t, ...)                                  Python floats, as the reference computes them
    one step   d = s - p;  t = omd * d;  s' = s - t               three float32 operations, omd = float32(1 - decay_t)
               s' = p  for a parameter that does not train
numpy rounds every float32 operation on its own, which is what the package's kernels must do as well.  `step_contracted` is the WRONG
form on purpose -- s - omd * d with the product unrounded, what a fused multiply-add computes -- for the test that shows the
difference is visible."""
import numpy as np


def get_decay(optimization_step, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3):
    step = max(0, optimization_step - update_after_step - 1)
    if step <= 0:
        return 0.0
    if use_ema_warmup:
        cur = 1 - (1 + step / inv_gamma) ** -power
    else:
        cur = (1 + step) / (10 + step)
    return max(min(cur, decay), min_decay)


def omd32(decay):
    """the Python float 1 - decay, rounded to float32 once"""
    return np.float32(1 - decay)


def step(s, p, decay, trains=True):
    """one step of a float32 shadow array against a float32 parameter array; returns the new shadow"""
    s = np.asarray(s, dtype=np.float32)
    p = np.asarray(p, dtype=np.float32)
    if not trains:
        return p.copy()
    with np.errstate(all="ignore"):
        d = (s - p).astype(np.float32)
        t = (omd32(decay) * d).astype(np.float32)
        return (s - t).astype(np.float32)


def step_contracted(s, p, decay):
    """s - omd * (s - p) with d rounded to float32 but the product and the last subtraction done exactly and rounded ONCE: the fma.
    (float64 holds the product of two float32 values exactly; its sum with a float32 is rounded to float64 first, which can differ
    from the exact fma only in a double-rounding corner that does not matter for counting differences.)"""
    s = np.asarray(s, dtype=np.float32)
    p = np.asarray(p, dtype=np.float32)
    d = (s - p).astype(np.float32)
    return (s.astype(np.float64) - np.float64(omd32(decay)) * d.astype(np.float64)).astype(np.float32)


def run(shadows, params_per_step, trains, start_step=0, **schedule):
    """shadows: list of float32 arrays; params_per_step: one list of arrays per optimization step; trains: list of bools.
    Returns (shadows after the last step, decay of the last step, optimization_step)."""
    sh = [np.array(s, dtype=np.float32, copy=True) for s in shadows]
    t, decay = start_step, None
    for params in params_per_step:
        t += 1
        decay = get_decay(t, **schedule)
        sh = [step(s, p, decay, tr) for s, p, tr in zip(sh, params, trains)]
    return sh, decay, t


# Inputs on which contraction shows.  With p = s + 1e-3 * N(0, 1) and decay 0.9999 the product t is ~1e-7 next to s ~ 1: its own
# rounding error (~1e-15) almost never moves s - t across a float32 rounding boundary, and the contracted form differs on 0.0015 %
# of the elements.  The difference is frequent when t is of the size of s, i.e. when |s - p| ~ |s| / omd = 1e4: measured on this draw,
# 29 % of the elements (10 % at 1e3, 1.7 % at 1e2).
CONTRACTION_SCALE = 1e4


def contraction_draw(n=65537, seed=0, scale=CONTRACTION_SCALE):
    rs = np.random.RandomState(seed)
    s = rs.randn(n).astype(np.float32)
    p = (s + scale * rs.randn(n)).astype(np.float32)
    return s, p
