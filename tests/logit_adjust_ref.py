"""numpy float32 restatement of the logit adjustment ("Logit adjustment"; csrc/logit_adjust.hip; include/showo_hip.h
showo_logits_adjust) and the bitmap helpers its tests share.

    r_i = x_i                                  i not in S
    r_i = x_i * theta  if x_i < 0,  else  x_i / theta     i in S     (fp32 multiply, fp32 IEEE division)
    y_i = r_i + beta_i                         (no bias row: y_i = r_i)

-0.0 and 0.0 are "not < 0"; -inf stays -inf; beta_i = -inf bans token i.  Every operation is one correctly rounded fp32 operation
(numpy's float32 multiply, divide and add are), so the kernel is held to these bits exactly.
"""
import numpy as np


def adjust_ref(x, members, theta, beta=None):
    """y fp32 [V] of one row: x fp32 [V], members any iterable of token ids (ids outside [0, V) are ignored) or a bool [V] array"""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    V = x.shape[0]
    m = np.asarray(members)
    if m.dtype == np.bool_:
        in_set = m.reshape(-1)
    else:
        in_set = np.zeros(V, dtype=bool)
        ids = m.astype(np.int64).reshape(-1)
        in_set[ids[(ids >= 0) & (ids < V)]] = True
    th = np.float32(theta)
    with np.errstate(all="ignore"):
        pen = np.where(x < 0, (x * th).astype(np.float32), (x / th).astype(np.float32)).astype(np.float32)
        r = np.where(in_set, pen, x).astype(np.float32)
        if beta is not None:
            r = (r + np.asarray(beta, dtype=np.float32).reshape(-1)).astype(np.float32)
    return r


def words(V):
    return (V + 31) // 32


def bitmap_of(V, ids, ld=None):
    """uint32 [ld] (ld >= ceil(V / 32)): bit i & 31 of word i >> 5 for every id in [0, V)"""
    w = np.zeros(words(V) if ld is None else ld, dtype=np.uint32)
    for i in ids:
        if 0 <= int(i) < V:
            w[int(i) >> 5] |= np.uint32(1) << np.uint32(int(i) & 31)
    return w


def members_of(V, bitmap):
    """bool [V] from a bitmap row"""
    w = np.asarray(bitmap, dtype=np.uint32).reshape(-1)
    i = np.arange(V)
    return ((w[i >> 5] >> (i & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def bits(a):
    """the uint32 view fp32 results are compared in"""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)
