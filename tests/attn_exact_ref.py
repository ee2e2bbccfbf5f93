"""Generators and exact expectations for the multi-row (prefill) attention kernels: csrc/attention.hip attn_fwd_kernel / attn_lds_body and
csrc/attention_bwd.hip.  CPU only (numpy / torch); imports neither the package nor a GPU.  tests/test_attn_exact_ref_cpu.py checks
everything here on the CPU, so that a failure of tests/test_attn_prefill_exact_gpu.py can only mean the kernel.

The kernels decide per query row which keys are seen from four ints (lo1, hi1, lo2, hi2): visible(c) = lo1 <= c < hi1 or lo2 <= c < hi2.
The schemes here make one key too many or too few change the output bits:
  counting     Q = 0, so every visible p is 1; V integers in {-2 .. 2}; every row sees a power-of-two number n of keys: the fp32 sums are
               exact integers below 2^24, 1 / n is exact, O = round(sum / n) bit for bit
  dominating   K[k] = 16 e_{(k + s) mod 32} + 16 e_{32 + (k div 32 + s) mod 32}, q_r the code of a target key k*_r: the target scores
               512, every other key at most 256 (codes repeat every 1024 keys), exp2 of a gap of 256 natural-log units is exactly 0 in
               fp32, so O[r] is row k*_r of V bit for bit
  indicator    causal rows see r + 1 + Lk - Lq keys (no power of two): V is 1 at one key in one dimension, O there is round(1 / n) on
               the rows where 1 / n and its two fp32 neighbours round to the same 16-bit value, and exactly 0 where the key is hidden
  backward     one-hot dO / Q rows (probe rows at wave and block edges, one head dimension each): column d_j of dV / dK is the
               probability row / dS row of probe r*_j, exactly 0 on every hidden key
"""
import functools

import numpy as np
import torch

BF16, F16 = 0, 1  # SHOWO_OP_BF16 / SHOWO_OP_F16
NEG_MASK = float(torch.iinfo(torch.int64).min)  # the reference's "masked" value (oracle/showo_oracle.py NEG_MASK)
LAYOUTS = ("mixed", "wave_uniform", "block_gap")
WPB = 4  # waves (32-row query tiles) per block of the LDS-tiled forward


def ceil64(n):
    return (n + 63) // 64 * 64


def _dt(op):
    return torch.float16 if op == F16 else torch.bfloat16


def rnd(t, op):
    """fp32 -> the operand type and back"""
    return t.to(_dt(op)).to(torch.float32)


def bits(t, op):
    return t.to(_dt(op)).view(torch.int16)


def vals(b, op):
    return b.view(_dt(op)).to(torch.float32)


def pow2_le(n):
    return 1 << (int(n).bit_length() - 1)


def pow2s(n):
    return [1 << i for i in range(int(n).bit_length())]


def edges(Lk):
    """{0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 129, ..., Lk - 1, Lk} clipped to Lk"""
    e = {0, 1, Lk - 1, Lk}
    for m in range(32, Lk + 32, 32):
        e.update((m - 1, m))
        if m % 64 == 0 or m == 32:
            e.add(m + 1)
    return sorted(x for x in e if 0 <= x <= Lk)


def _valid(t, Lk):
    lo1, hi1, lo2, hi2 = t
    if not 0 <= lo1 < hi1 <= Lk:
        return False
    if lo2 == 0 and hi2 == 0:
        n = hi1 - lo1
    else:
        if not hi1 < lo2 < hi2 <= Lk:  # a gap of at least one key: two real runs
            return False
        n = hi1 - lo1 + hi2 - lo2
    return n & (n - 1) == 0


_SPLITS = [(1, 1), (1, 3), (3, 1), (2, 2), (5, 3), (1, 7), (4, 4), (16, 16), (31, 33), (33, 31), (32, 32), (1, 63), (63, 65), (64, 64),
           (127, 129), (1, 255)]


def _one_run(rs, Lk, E, P):
    for _ in range(1000):
        e, n = E[rs.randint(len(E))], P[rs.randint(len(P))]
        c = (e, e + n, 0, 0) if rs.randint(2) else (e - n, e, 0, 0)
        if _valid(c, Lk):
            return c
    raise AssertionError(Lk)


def _two_run(rs, Lk, E):
    for _ in range(200):
        a, b = E[rs.randint(len(E))], E[rs.randint(len(E))]
        n1, n2 = _SPLITS[rs.randint(len(_SPLITS))]
        c = (a, a + n1, b - n2, b) if rs.randint(2) else (a - n1, a, b, b + n2)
        if _valid(c, Lk):
            return c
    return None


def _wave_quads(Lk):
    """interval quads for the four waves of a block, every interval with a power-of-two count.  q0: the low edges (both one-interval
    fast paths, the inner sub-tile, a hull that ends one key after a 64-key tile starts); q1: hulls from key 64 on (kt0 > 0); q2: runs
    that end at Lk (the clamped loads at Lk - 1); q3: two runs shared by the whole wave; q4 / q5: mid-range edges and long runs."""
    P = pow2_le(Lk)
    m = Lk // 128 * 64
    quads = [
        [(1, 65, 0, 0), (0, 32, 0, 0), (31, 63, 0, 0), (33, 65, 0, 0)],
        [(64, 128, 0, 0), (65, 129, 0, 0), (95, 127, 0, 0), (127, 129, 0, 0)],
        [(Lk - P, Lk, 0, 0), (Lk - 1, Lk, 0, 0), (Lk - 32, Lk, 0, 0), (Lk - 64, Lk, 0, 0)],
        [(0, 1, Lk - 1, Lk), (0, 32, 64, 96), (1, 33, 65, 97), (31, 32, Lk - 3, Lk)],
        [(m - 1, m + 63, 0, 0), (m + 1, m + 65, 0, 0), (m - 32, m + 32, 0, 0), (m, m + 1, 0, 0)],
        [(0, P, 0, 0), (1, 1 + P // 2, 0, 0), (Lk - P // 2, Lk, 0, 0), (Lk - P // 2 - 1, Lk - 1, 0, 0)],
        [(0, 1, 0, 0), (0, 2, 0, 0), (Lk - 2, Lk, 0, 0), (1, 2, 0, 0)],
    ]
    out = []
    for q in quads:
        ok = [c for c in q if _valid(c, Lk)]
        if ok:
            out.append([c if _valid(c, Lk) else ok[0] for c in q])
    return out


_REGION_ORDER = (2, 0, 3, 1)


def _block_gap_row(r, Lk, phase):
    blk, wave = r // (32 * WPB), (r // 32) % WPB
    reg = _REGION_ORDER[(wave + blk + phase) % 4]
    width = Lk // 4
    base = min(reg * Lk // 4, Lk - 1)
    end = Lk if reg == 3 else max(base + 1, (reg + 1) * Lk // 4)
    off = r % 3 if width >= 4 else 0
    lo = min(base + off, end - 1)
    ns = [n for n in pow2s(max(1, width // 2)) if lo + n <= end] or [1]
    n = ns[(r // 3) % len(ns)]
    if r % 4 == 3 and n >= 2 and lo + n + 1 <= end:  # two runs inside the wave's region: n / 2 keys, one hidden, n / 2 keys
        return (lo, lo + n // 2, lo + n // 2 + 1, lo + n + 1)
    return (lo, lo + n, 0, 0)


@functools.lru_cache(maxsize=None)
def _interval_rows(Lq, Lk, layout, phase):
    E = edges(Lk)
    P = pow2s(Lk)
    rows = []
    if layout == "mixed":
        rs = np.random.RandomState(1000 * phase + Lk)  # a fixed pseudo-random walk through the (edge, count) candidates
        for r in range(Lq):
            c = _two_run(rs, Lk, E) if r % 2 else None
            rows.append(c or _one_run(rs, Lk, E, P))
    elif layout == "wave_uniform":
        Q = _wave_quads(Lk)
        for r in range(Lq):
            w = r // 32
            rows.append(Q[(w // WPB + phase) % len(Q)][w % WPB])
    elif layout == "block_gap":
        rows = [_block_gap_row(r, Lk, phase) for r in range(Lq)]
    else:
        raise ValueError(layout)
    return tuple(rows)


def interval_table(Lq, Lk, layout, phase=0):
    """int32 [Lq, 4] rows (lo1, hi1, lo2, hi2) in the kernel's canonical form (an absent second run is (0, 0), lo1 < hi1 < lo2 < hi2 <= Lk
    otherwise), every row with a power-of-two number of visible keys and its anchoring edges drawn from edges(Lk).  phase: another
    walk through the same candidates (batch b of a test uses phase b).
      "mixed"         consecutive rows cycle through different edge pairs, one-run and two-run rows interleaved
      "wave_uniform"  the 32 rows of a wave share one interval; successive waves walk _wave_quads
      "block_gap"     the four waves of a 128-row block see disjoint key ranges a quarter of Lk apart"""
    return torch.tensor(_interval_rows(Lq, Lk, layout, phase), dtype=torch.int32).reshape(Lq, 4)


def batch_table(B, Lq, Lk, layout, empty=False):
    """[B, Lq, 4]: batch b walks with phase b.  empty: one row per wave, at wave position 0 (even waves) or 31 (odd waves), sees nothing."""
    iv = torch.stack([interval_table(Lq, Lk, layout, b) for b in range(B)])
    if empty:
        iv = iv.clone()
        iv[:, empty_rows(Lq)] = 0
    return iv


def empty_rows(Lq):
    return [r for r in range(Lq) if r % 64 == 0 or r % 64 == 63]


def vis_of(iv, Lk):
    """bool [..., Lk] visibility of interval rows [..., 4]"""
    c = torch.arange(Lk)
    t = iv.to(torch.int64)[..., None, :]
    c = c.reshape((1,) * (iv.dim() - 1) + (Lk, ))
    return ((c >= t[..., 0]) & (c < t[..., 1])) | ((c >= t[..., 2]) & (c < t[..., 3]))


def dense_of(vis):
    """additive fp32 mask: 0 on the visible keys, NEG_MASK elsewhere"""
    return torch.where(vis, torch.zeros((), dtype=torch.float32), torch.full((), NEG_MASK, dtype=torch.float32))


def causal_table(B, Lq, Lk):
    """the intervals the kernels use when no table is given: row r sees keys [0, r + 1 + Lk - Lq)"""
    iv = torch.zeros((B, Lq, 4), dtype=torch.int32)
    iv[..., 1] = (torch.arange(Lq) + 1 + Lk - Lq).to(torch.int32)
    return iv


# ------------------------------------------------------------------------------------------------ the tiled kernel's control flow
def path_census(iv, Lk):
    """Which branches of attn_lds_body a [Lq, 4] table takes (WPB = 4, 32-key sub-tiles of 64-key tiles), by transcription of its
    wave-uniform decisions.  Returns a dict of counters."""
    t = iv.to(torch.int64).numpy()
    Lq = t.shape[0]
    t = t.copy()
    t[:, 1] = np.minimum(t[:, 1], Lk)
    t[:, 3] = np.minimum(t[:, 3], Lk)
    big = 0x7fffffff
    out = dict.fromkeys(("skip", "inner", "fast_tail", "fast_head", "general", "general_one_iv", "kt0_gt0", "mixed_runs_wave",
                         "hull_ends_1_after_tile", "tile_skipped_by_wave", "fast_tail_clipped", "fast_head_clipped",
                         "clamped_tile", "inner_second_run"), 0)
    nwaves = (Lq + 31) // 32
    for blk in range((nwaves + WPB - 1) // WPB):
        hulls = []
        for w in range(blk * WPB, min(nwaves, (blk + 1) * WPB)):
            rows = t[32 * w:min(Lq, 32 * w + 32)]
            h1, h2 = rows[:, 0] < rows[:, 1], rows[:, 2] < rows[:, 3]
            wmin = min(np.where(h1, rows[:, 0], big).min(), np.where(h2, rows[:, 2], big).min())
            wmax = max(np.where(h1, rows[:, 1], 0).max(), np.where(h2, rows[:, 3], 0).max())
            hulls.append((rows, int(wmin), int(wmax), bool((~h2).all())))
            out["mixed_runs_wave"] += int(h2.any() and not h2.all())
            out["hull_ends_1_after_tile"] += int(wmax % 64 == 1)
        bmin, bmax = min(h[1] for h in hulls), max(h[2] for h in hulls)
        kt0 = 0 if bmin >= big else bmin & ~63
        out["kt0_gt0"] += int(kt0 > 0)
        for kt in range(kt0, bmax, 64):
            out["clamped_tile"] += int(kt + 64 > Lk)
            for rows, wmin, wmax, one_iv in hulls:
                skipped = 0
                for ks in (kt, kt + 32):
                    lo1, hi1, lo2, hi2 = rows.T
                    if ks >= wmax or ks + 32 <= wmin:
                        out["skip"] += 1
                        skipped += 1
                    elif (((lo1 <= ks) & (ks + 32 <= hi1)) | ((lo2 <= ks) & (ks + 32 <= hi2))).all():
                        out["inner"] += 1
                        out["inner_second_run"] += int(((lo2 <= ks) & (ks + 32 <= hi2)).any())
                    elif one_iv and (lo1 <= ks).all():
                        out["fast_tail"] += 1
                        out["fast_tail_clipped"] += int((hi1 < ks + 32).any())
                    elif one_iv and (hi1 >= ks + 32).all():
                        out["fast_head"] += 1
                        out["fast_head_clipped"] += int((lo1 > ks).any())
                    else:
                        out["general"] += 1
                        out["general_one_iv"] += int(one_iv)
                out["tile_skipped_by_wave"] += int(skipped == 2)
    return out


# ------------------------------------------------------------------------------------------------ counting
@functools.lru_cache(maxsize=None)
def int_v(B, nH, Lk):
    """deterministic integers in {-2 .. 2} that depend on key, dimension, head and sequence (the pattern of
    test_decode_attn_lengths_gpu.py _int_v)"""
    k = torch.arange(Lk)[None, None, :, None]
    d = torch.arange(64)[None, None, None, :]
    h = torch.arange(nH)[None, :, None, None]
    b = torch.arange(B)[:, None, None, None]
    return (((k * 31 + d * 17 + (k >> 3) * 7 + (k >> 9) * 3 + h * 11 + b * 13 + k * d) % 5) - 2).to(torch.float32)


def counting_mean(v, iv):
    """fp32 [B, Lq, nH * 64]: the exact mean of the visible rows of integer v [B, nH, Lk, 64] under iv [B, Lq, 4] (every count a power of
    two, every sum an integer below 2^24: exact in fp32 in any order of summation)"""
    B, nH, Lk, _ = v.shape
    vis = vis_of(iv, Lk)  # [B, Lq, Lk]
    n = vis.sum(-1)
    assert bool(((n > 0) & ((n & (n - 1)) == 0)).all()), "a row without a power-of-two number of visible keys"
    s = torch.einsum("bqk,bhkd->bqhd", vis.double(), v.double())
    assert float(s.abs().max()) < 2 ** 24 and bool((s == s.round()).all())
    return (s / n[..., None, None].double()).to(torch.float32).reshape(B, iv.shape[1], nH * 64)


def counting_expectation(v, iv, op):
    """the mean rounded to the operand type (as fp32 values)"""
    return rnd(counting_mean(v, iv), op)


def split_of(x):
    """fp32 -> (hi, lo) bf16 pair as fp32 values: hi = bf16(x), lo = bf16(x - hi)"""
    hi = rnd(x, BF16)
    return hi, rnd(x - hi, BF16)


# ------------------------------------------------------------------------------------------------ dominating key
def kstar_table(iv, phase=0):
    """int64 [Lq]: a target key per row inside its intervals, walked through lo1, hi1 - 1, lo2, hi2 - 1 and the interior"""
    t = iv.to(torch.int64)
    lo1, hi1, lo2, hi2 = t.unbind(-1)
    two = lo2 < hi2
    lo2 = torch.where(two, lo2, lo1)
    hi2 = torch.where(two, hi2, hi1)
    mid = torch.where(hi2 - lo2 > hi1 - lo1, (lo2 + hi2) // 2, (lo1 + hi1) // 2)
    cand = torch.stack([lo1, hi1 - 1, lo2, hi2 - 1, mid], -1)
    r = torch.arange(t.shape[0])
    return cand[r, (r // 2 + phase) % 5]


def _code(k, shift):
    """the two hot dimensions of key index k [...]: (k + s) mod 32 and 32 + (k div 32 + s) mod 32"""
    return (k + shift) % 32, 32 + (k // 32 + shift) % 32


def dominating_qk(iv, Lk, nH):
    """iv [B, Lq, 4] (rows without a visible key get the code of key 0: their output is not defined).  Returns q [B, nH, Lq, 64] (the
    pre-scaled Q the kernel takes), k [B, nH, Lk, 64], kstar [B, Lq].  Values are 0 and 16: exact in bf16 and fp16.  The code shift
    depends on batch and head, so a wrong block-to-(batch, head) map pairs a query with the wrong code."""
    B, Lq, _ = iv.shape
    assert Lk <= 1024, "codes repeat every 1024 keys"
    ks = torch.stack([kstar_table(iv[b], b) for b in range(B)]).clamp(min=0)
    shift = (5 * torch.arange(nH)[None, :, None] + 11 * torch.arange(B)[:, None, None]) % 32  # [B, nH, 1]
    q = torch.zeros(B, nH, Lq, 64)
    k = torch.zeros(B, nH, Lk, 64)
    for x, idx in ((k, torch.arange(Lk)[None, None, :].expand(B, nH, Lk)), (q, ks[:, None, :].expand(B, nH, Lq))):
        for c in _code(idx, shift):
            x.scatter_(-1, c[..., None], 16.0)
    return q, k, ks


def gather_rows(v, ks):
    """v [B, nH, Lk, 64], ks [B, Lq] -> [B, Lq, nH * 64]: row ks[b, r] of every head"""
    B, nH, _, _ = v.shape
    Lq = ks.shape[1]
    g = torch.gather(v, 2, ks[:, None, :, None].expand(B, nH, Lq, 64))
    return g.transpose(1, 2).reshape(B, Lq, nH * 64)


def split_v(B, nH, Lk, seed):
    """random V as a (hi, lo) bf16 pair with |lo| <= ulp(hi) / 2 and bf16(hi + lo) == hi (pairs that a rounding of lo pushed onto a tie
    get lo = 0), so that a kernel that returns bf16(hi + lo) and the remainder returns the pair itself"""
    g = torch.Generator().manual_seed(seed)
    hi, lo = split_of(torch.randn(B, nH, Lk, 64, generator=g))
    s = hi + lo  # exact in fp32: both lie inside the 24 bits of the value they were split from
    keep = (rnd(s, BF16) == hi) & (rnd(s - hi, BF16) == lo)
    return hi, torch.where(keep, lo, torch.zeros(()))


# ------------------------------------------------------------------------------------------------ causal indicator
def one_over_is_unambiguous(n, op):
    """bool per entry of int tensor n: 1 / n and its two fp32 neighbours round to the same 16-bit value (a reciprocal that is one ulp off
    cannot change the expectation) -- the rule of test_decode_attn_lengths_gpu.py _one_over_is_unambiguous, vectorised"""
    f = (np.float32(1) / n.numpy().astype(np.float32)).astype(np.float32)
    c = [f, np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(1))]
    r = [rnd(torch.from_numpy(np.ascontiguousarray(x)), op) for x in c]
    return (r[0] == r[1]) & (r[0] == r[2])


def indicator_case(B, nH, Lq, Lk, op):
    """V [B, nH, Lk, 64] with a single 1 per (head, dimension) at a key that walks the edges; want [B, Lq, nH * 64] = round(1 / n_r) where
    that key is visible to causal row r (n_r = r + 1 + Lk - Lq keys) and 0 where it is hidden; check [Lq] bool: rows whose 1 / n_r is
    unambiguous (the zeros hold on every row)."""
    n = torch.arange(Lq) + 1 + Lk - Lq
    E = [e for e in edges(Lk) if e < Lk]
    E += [int(x) for x in (n - 1).tolist() + n.tolist() if 0 <= x < Lk and x not in E][:64]
    v = torch.zeros(B, nH, Lk, 64)
    key = torch.zeros(B, nH, 64, dtype=torch.int64)
    for b in range(B):
        for h in range(nH):
            for d in range(64):
                key[b, h, d] = E[(d * 7 + 3 * h + 5 * b) % len(E)]
    v.scatter_(2, key[:, :, None, :], 1.0)
    seen = key[:, None, :, :] < n[None, :, None, None]  # [B, Lq, nH, 64]
    one = rnd(1.0 / n.to(torch.float32), op)
    want = torch.where(seen, one[None, :, None, None], torch.zeros(())).reshape(B, Lq, nH * 64)
    return v, want, one_over_is_unambiguous(n, op)


# ------------------------------------------------------------------------------------------------ backward probes
def probe_rows(L):
    """up to 64 query rows at wave (32) and block (128) edges, first and last row included"""
    return [e for e in edges(L) if e < L][:64]


def probe_dims(nprobe, b, h):
    """distinct head dimensions for the probes of (batch b, head h)"""
    return [(5 * j + 3 * h + 7 * b) % 64 for j in range(nprobe)]


def sign_v(B, nH, L):
    """V = +-1, alternating along the keys (any two neighbouring keys differ), shifted by dimension, head and batch"""
    k = torch.arange(L)[None, None, :, None]
    d = torch.arange(64)[None, None, None, :]
    h = torch.arange(nH)[None, :, None, None]
    b = torch.arange(B)[:, None, None, None]
    return (1 - 2 * ((k + d + h + b) % 2)).to(torch.float32)


def backward_case(B, nH, L, layout, which):
    """Operands of the backward visibility tests, all exact in bf16.  which = "dv": Q = 0, K random; "dk": K = 0, Q[r*_j] = e_{d_j}.
    In both dO[r*_j] = e_{d_j} (head by head), V = sign_v with one sign flipped where a probe's visible keys all had the same one.
    Returns a dict with q, k, v [B, nH, L, 64], do [B, L, nH * 64], iv [B, L, 4], rows (probe rows), dims [B][nH] (their dimensions)
    and usable [B, nH, nprobe]: the probe sees at least two keys, so the visible mean of V in its dimension is neither +1 nor -1 and
    dP - D is nonzero on every visible key (the dK pattern needs it)."""
    iv = batch_table(B, L, L, layout)
    rows = probe_rows(L)
    v = sign_v(B, nH, L)
    g = torch.Generator().manual_seed(7 * L + B + nH)
    k = rnd(torch.randn(B, nH, L, 64, generator=g), BF16) if which == "dv" else torch.zeros(B, nH, L, 64)
    q = torch.zeros(B, nH, L, 64)
    do = torch.zeros(B, L, nH, 64)
    dims = [[probe_dims(len(rows), b, h) for h in range(nH)] for b in range(B)]
    vis = vis_of(iv, L)  # [B, L, L]
    usable = torch.zeros(B, nH, len(rows), dtype=torch.bool)
    for b in range(B):
        for h in range(nH):
            for j, (r, d) in enumerate(zip(rows, dims[b][h])):
                do[b, r, h, d] = 1.0
                if which == "dk":
                    q[b, h, r, d] = 1.0
                seen = vis[b, r].nonzero().flatten()
                if len(seen) >= 2 and float(v[b, h, seen, d].mean().abs()) == 1:
                    v[b, h, seen[0], d] *= -1  # all visible keys of one sign (two runs of equal parity): flip the first one
                usable[b, h, j] = len(seen) >= 2  # a row that sees one key has P = 1 and dS = 0 there by arithmetic
    return dict(q=q, k=k, v=v, do=do.reshape(B, L, nH * 64), iv=iv, rows=rows, dims=dims, usable=usable, vis=vis)


def backward_reference(c):
    """fp64 autograd of softmax(Q K^T + mask) V on the operands of backward_case: (o, lse, dq, dk, dv), head-major [B, nH, L, 64]"""
    B, nH, L, _ = c["q"].shape
    q, k, v = (c[n].double().requires_grad_(True) for n in ("q", "k", "v"))
    s = q @ k.transpose(-1, -2) + dense_of(c["vis"])[:, None].double()
    o = torch.softmax(s, -1) @ v
    o.backward(c["do"].double().reshape(B, L, nH, 64).transpose(1, 2))
    return o.detach(), torch.logsumexp(s.detach(), -1), q.grad, k.grad, v.grad
