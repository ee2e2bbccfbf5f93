"""Reference of the nucleus (top-p) draw of the mmu decode (csrc/sample_row.h sample_topk_topp_row), shared by the CPU and GPU tests.

The contract, restated in plain torch.  x_i = logits[i] / T in fp32, then
  1. top-k as showo_sample_topk: keep x >= (top_k-th largest x), ties with the k-th value stay, top_k None / <= 0 / >= V: no filter;
     the survivors are the candidates;
  2. p = softmax over the candidates (here in fp64);
  3. token i is kept iff the probability mass of the candidates with STRICTLY larger x is <= top_p (top_p as the fp32 value the C ABI
     receives);
  token = argmax_i p'_i / E_i with p' = p renormalised over the kept set.

`device_rule` is a host emulation of the arithmetic the kernel decides with: fp32 exp, fixed-point weights
w_i = trunc(exp(x_i - max) * 2^40), exact integer sums, kept(i) <=> (double)A_i <= (double)top_p * (double)S.

Case selection happens here, on the CPU, independent of the code under test: a family is (V, scale, top_k, top_p, T) over
logits = randn(V, seed) * scale, and its cases are the first 6 seeds whose reference margin -- min_i |mass_above(i) - top_p| over the
candidates -- is >= MARGIN = 1e-5.  That is about 50x the worst disagreement between the device's mass and the reference's: one ulp of
expf (6e-8 per term), the fp32 rounding of x - max (<= 2.4e-7 per term for the terms within 8 of the max, which carry the mass) and
the fixed-point truncation (< 5e-8 in total for V = 58498): a few 1e-7 (test_nucleus_ref_cpu.py measures it)."""
import functools

import numpy as np
import torch

MARGIN = 1e-5
V_FULL = 58498

# (V, scale, top_k, top_p, T); no top_p >= 0.999 at V >= 8192: the cut token's own mass is below MARGIN there
FAMILIES = [(V, scale, k, p, T)
            for V, scale in ((439, 1.0), (439, 3.0), (1030, 3.0), (V_FULL, 3.0))
            for k, p, T in ((None, 0.9, 1.0), (None, 0.5, 0.7), (50, 0.95, 1.3))] + [(439, 1.0, None, 0.999, 1.0)]


def _f32(v):
    return float(np.float32(v))


def family_logits(V, scale, seed, halves=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(V, generator=g) * scale
    return (x * 2).round() / 2 if halves else x


def _candidates(x, top_k):
    V = x.numel()
    if top_k is None or top_k <= 0 or top_k >= V:
        return torch.ones(V, dtype=torch.bool)
    return x >= torch.topk(x, top_k).values[-1]


def _above(x, cand, w):
    """per token: the sum of w over the candidates with strictly larger x (w: float64 or int64, zero outside the candidates)"""
    vals, inv = torch.unique(x, return_inverse=True)  # ascending
    gm = torch.zeros(vals.numel(), dtype=w.dtype).scatter_add_(0, inv, torch.where(cand, w, torch.zeros_like(w)))
    s = gm.flip(0).cumsum(0).flip(0)  # mass of the groups >= each value
    return torch.cat([s[1:], torch.zeros(1, dtype=w.dtype)])[inv]


def ref_nucleus(logits, top_k, top_p, T):
    """(kept mask [V] bool, p' [V] float64, margin) of the contract above"""
    x = logits.float() / _f32(T)
    cand = _candidates(x, top_k)
    p = torch.where(cand, x.double(), torch.tensor(-float("inf"), dtype=torch.float64)).softmax(-1)
    above = _above(x, cand, p)
    keep = cand & (above <= _f32(top_p))
    margin = float((above[cand] - _f32(top_p)).abs().min())
    pk = torch.where(keep, p, torch.zeros_like(p))
    return keep, pk / pk.sum(), margin


def device_rule(logits, top_k, top_p, T):
    """(kept mask, A / S per token as float64) by the kernel's arithmetic: fp32 exp, 2^40 fixed point, the double compare"""
    x = logits.float() / _f32(T)
    cand = _candidates(x, top_k)
    mx = x[cand].max()
    w = (torch.exp(x - mx) * float(2 ** 40)).to(torch.int64)  # exact scaling, truncating conversion
    w = torch.where(cand, w, torch.zeros_like(w))
    A, S = _above(x, cand, w), int(w.sum())
    keep = cand & (A.double() <= torch.tensor(_f32(top_p), dtype=torch.float64) * float(S)) & (w > 0)
    return keep, A.double() / float(S)


def draw_reference(logits, top_k, top_p, T, e):
    """(token, p', keep) of argmax p' / E in fp32, lowest index among ties, as test_kernels_gpu's _topk_reference does for top-k"""
    keep, pk, _ = ref_nucleus(logits, top_k, top_p, T)
    return int(torch.argmax(pk.float() / e)), pk, keep


@functools.lru_cache(maxsize=None)
def cases(family, count=6, halves=False):
    """the first `count` seeds of the family whose reference margin is >= MARGIN"""
    V, scale, k, p, T = family
    out, seed = [], 0
    while len(out) < count:
        if ref_nucleus(family_logits(V, scale, seed, halves), k, p, T)[2] >= MARGIN:
            out.append(seed)
        seed += 1
        assert seed < 200, family
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tie_case(V=439, scale=3.0, top_p=0.9, T=1.0):
    """the first seed of logits rounded to halves whose cut falls INSIDE a tied group: the lowest kept value is shared by several
    tokens, and a cut along a sorted order (the reference project's) would keep only some of them; margin >= MARGIN"""
    for seed in range(200):
        lg = family_logits(V, scale, seed, halves=True)
        keep, pk, margin = ref_nucleus(lg, None, top_p, T)
        x = lg.float() / _f32(T)
        grp = x == x[keep].min()
        n = int(grp.sum())
        p = torch.softmax(x.double(), -1)
        p1, above = float(p[grp][0]), float(p[x > x[keep].min()].sum())
        if margin >= MARGIN and n >= 3 and above + (n - 1) * p1 > _f32(top_p) + MARGIN:
            return seed
    raise AssertionError("no tie case")
