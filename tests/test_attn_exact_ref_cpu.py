"""CPU checks of tests/attn_exact_ref.py, the generators and expectations behind tests/test_attn_prefill_exact_gpu.py: a failure of the
GPU file can then only mean the kernel.  For every (Lq, Lk, layout) the GPU tests use: the interval tables are canonical, in range and
power-of-two counted; each layout really contains the situations it is named for (path_census transcribes the wave-uniform decisions
of the LDS-tiled forward); the counting expectation equals the rounded fp64 soft-max; the dominating-key operands are exact in both
16-bit types and the fp64 soft-max puts all but e^-256 of its weight on the target key."""
import numpy as np
import pytest
import torch

import attn_exact_ref as R
from attn_exact_ref import BF16, F16

SQUARE = [2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 258, 387]
COUNT_ONLY = [1155]
APPENDED = [(5, 45), (70, 200), (130, 517)]
BACKWARD = [64, 129, 387]
GRIDS = [(1, 3), (2, 5)]


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("L", SQUARE + COUNT_ONLY)
def test_tables_are_canonical_in_range_and_power_of_two_counted(L, layout):
    E = set(R.edges(L))
    for phase in (0, 1):
        t = R.interval_table(L, L, layout, phase)
        assert t.dtype == torch.int32 and tuple(t.shape) == (L, 4)
        lo1, hi1, lo2, hi2 = t.to(torch.int64).unbind(-1)
        two = lo2 < hi2
        assert bool(((lo1 >= 0) & (lo1 < hi1) & (hi1 <= L)).all()), "first run"
        assert bool((two | ((lo2 == 0) & (hi2 == 0))).all()), "an absent second run is (0, 0)"
        assert bool((~two | ((hi1 <= lo2) & (hi2 <= L))).all()), "runs ascend and end inside Lk"
        n = (hi1 - lo1) + (hi2 - lo2)
        assert bool(((n >= 1) & ((n & (n - 1)) == 0)).all()), "no empty row, power-of-two counts"
        assert bool((R.vis_of(t, L).sum(-1) == n).all())
        if layout != "block_gap":  # every row is anchored on the edge list (block_gap places its runs by region)
            anch = [(int(a) in E) or (int(b) in E) or (int(c) in E) or (int(d) in E) for a, b, c, d in t.tolist()]
            assert all(anch)
    # the edge list itself
    want = [e for e in (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 129, L - 1, L) if 0 <= e <= L]
    assert set(want) <= E and max(E) == L and min(E) == 0


def _census(L, layout):
    c = [R.path_census(R.interval_table(L, L, layout, p), L) for p in (0, 1)]
    return {k: c[0][k] + c[1][k] for k in c[0]}


@pytest.mark.parametrize("L", [31, 33, 65, 129, 258, 387, 1155])
def test_mixed_layout_rows_of_a_wave_disagree(L):
    """a wave with rows of one and of two runs (one_iv false), so every sub-tile that is not skipped takes the general two-interval test;
    in every full wave the rows disagree about lo1 <= ks and about hi1 >= ks + 32 at some sub-tile of the wave's hull"""
    c = _census(L, "mixed")
    assert c["mixed_runs_wave"] >= 2 and c["general"] >= 2
    for p in (0, 1):
        t = R.interval_table(L, L, "mixed", p).to(torch.int64)
        for w in range(L // 32):
            rows = t[32 * w:32 * w + 32]
            ks = torch.arange(0, R.ceil64(L), 32)[:, None]
            a, b = rows[None, :, 0] <= ks, rows[None, :, 1] >= ks + 32
            assert bool((a.any(1) & ~a.all(1)).any()), (L, p, w)
            assert L < 65 or bool((b.any(1) & ~b.all(1)).any()), (L, p, w)  # below 65 keys few power-of-two runs reach a sub-tile's end
            assert len({tuple(r) for r in rows.tolist()}) >= 16, "consecutive rows cycle through different edge pairs"


@pytest.mark.parametrize("L", [65, 127, 128, 129, 258, 387, 1155])
def test_wave_uniform_layout_takes_every_wave_uniform_path(L):
    """the inner sub-tile, the one-interval fast path over a clipped tail (lo1 <= ks, some hi1 < ks + 32) and over a clipped head
    (hi1 >= ks + 32, some lo1 > ks), a skipped sub-tile; from 127 keys on a block whose first tile is not tile 0 (kt0 > 0); a hull that
    ends one key after a 64-key tile starts"""
    for p in (0, 1):
        t = R.interval_table(L, L, "wave_uniform", p)
        for w in range((L + 31) // 32):
            assert len({tuple(r) for r in t[32 * w:32 * w + 32].tolist()}) == 1, "the rows of a wave share one interval"
    c = _census(L, "wave_uniform")
    for name in ("inner", "fast_tail_clipped", "fast_head_clipped", "skip", "hull_ends_1_after_tile"):
        assert c[name] >= 1, (L, name, c)
    if L >= 127:
        assert c["kt0_gt0"] >= 1, (L, c)
    if L >= 258:
        assert c["general"] >= 1 and c["tile_skipped_by_wave"] >= 1 and c["clamped_tile"] >= 1, (L, c)
    if L >= 387:
        assert c["inner_second_run"] >= 1, (L, c)


@pytest.mark.parametrize("L", [127, 128, 129, 258, 387, 1155])
def test_block_gap_layout_waves_of_a_block_are_disjoint(L):
    """the four waves of a block see disjoint key ranges; the block hull spans 64-key tiles that some wave skips entirely"""
    for p in (0, 1):
        t = R.interval_table(L, L, "block_gap", p)
        vis = R.vis_of(t, L)
        for blk in range((L + 127) // 128):
            hull = [vis[r0:r0 + 32].any(0) for r0 in range(128 * blk, min(L, 128 * blk + 128), 32)]
            for i in range(len(hull)):
                for j in range(i + 1, len(hull)):
                    assert not bool((hull[i] & hull[j]).any()), (L, p, blk, i, j)
    c = _census(L, "block_gap")
    assert c["tile_skipped_by_wave"] >= 2 and c["skip"] >= 4 and c["mixed_runs_wave"] >= 2, (L, c)


def _fp64_softmax_out(q, k, v, add):
    s = q.double() @ k.double().transpose(-1, -2) + add[:, None].double()
    p = torch.softmax(s, -1)
    B, nH, Lq, _ = q.shape
    return p, (p @ v.double()).transpose(1, 2).reshape(B, Lq, nH * 64)


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("L", SQUARE + COUNT_ONLY)
def test_counting_expectation_is_the_rounded_fp64_softmax(L, layout):
    B, nH = (1, 3) if L > 1000 else (2, 5)
    iv = R.batch_table(B, L, L, layout)
    v = R.int_v(B, nH, L)
    assert set(v.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert not torch.equal(v[0, 0], v[0, 1]) and (B == 1 or not torch.equal(v[0, 0], v[1, 0])), "values depend on head and batch"
    _, want = _fp64_softmax_out(torch.zeros(B, nH, L, 64), torch.randn(B, nH, L, 64), v, R.dense_of(R.vis_of(iv, L)))
    for op in (BF16, F16):
        got = R.counting_expectation(v, iv, op)
        assert torch.equal(got, R.rnd(want.to(torch.float32), op)), (L, layout, op)
        assert torch.equal(got.double(), want.to(R._dt(op)).double()), "the fp32 mean is exact, so one rounding from fp64 agrees"
    hi = R.counting_expectation(v, iv, BF16)
    lo = R.rnd(R.counting_mean(v, iv) - hi, BF16)
    assert torch.equal((hi.double() + lo.double()), want) or float((hi.double() + lo.double() - want).abs().max()) < 2 ** -15


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("L", SQUARE)
def test_dominating_key_operands_are_exact_and_dominate(L, layout):
    B, nH = 2, 5
    for empty in (False, True):
        iv = R.batch_table(B, L, L, layout, empty=empty and layout == "mixed")
        q, k, ks = R.dominating_qk(iv, L, nH)
        for op in (BF16, F16):
            assert torch.equal(R.rnd(q, op), q) and torch.equal(R.rnd(k, op), k), "operands round-trip through the 16-bit type"
        vis = R.vis_of(iv, L)
        live = vis.any(-1)
        assert bool(vis.gather(-1, ks[..., None])[live].all()), "the target key is visible"
        t = iv.to(torch.int64)
        for b in range(B):  # the targets walk the four interval edges and the interior
            hit = [(ks[b] == t[b, :, 0]), (ks[b] == t[b, :, 1] - 1), (ks[b] == t[b, :, 2]) & (t[b, :, 2] < t[b, :, 3]),
                   (ks[b] == t[b, :, 3] - 1) & (t[b, :, 2] < t[b, :, 3])]
            assert L < 31 or all(bool(h.any()) for h in hit[:2]), (L, layout, b)
            assert L < 65 or layout != "mixed" or all(bool(h.any()) for h in hit), (L, layout, b)
        p, _ = _fp64_softmax_out(q, k, torch.zeros(B, nH, L, 64), R.dense_of(vis))
        s = q.double() @ k.double().transpose(-1, -2)
        top = s.gather(-1, ks[:, None, :, None].expand(B, nH, L, 1))[..., 0]
        assert bool((top == 512)[live[:, None].expand_as(top)].all())
        others = s.masked_fill(~vis[:, None], -1).scatter(-1, ks[:, None, :, None].expand(B, nH, L, 1), -1)
        assert float(others.max()) <= 256, "every other visible key scores at most 256"
        w = p.gather(-1, ks[:, None, :, None].expand(B, nH, L, 1))[..., 0]
        assert bool((1 - w[live[:, None].expand_as(w)] <= L * np.exp(-256.0)).all()), "weight 1 - O(e^-256) on the target"
        assert np.exp2(np.float32(-256.0 * 1.4426950408889634)) == 0, "exp2 of the gap is exactly 0 in fp32"
        assert not torch.equal(k[0, 0], k[0, 1]) and not torch.equal(k[0, 0], k[1, 0]), "codes depend on head and batch"


def test_split_v_pairs_are_fixed_points():
    hi, lo = R.split_v(2, 3, 130, 5)
    assert torch.equal(R.rnd(hi, BF16), hi) and torch.equal(R.rnd(lo, BF16), lo)
    s = hi + lo
    assert torch.equal(s.double(), hi.double() + lo.double()), "hi + lo is exact in fp32"
    assert torch.equal(R.rnd(s, BF16), hi) and torch.equal(R.rnd(s - hi, BF16), lo)
    assert float((lo != 0).float().mean()) > 0.9


@pytest.mark.parametrize("Lq,Lk", APPENDED)
def test_causal_indicator_expectation(Lq, Lk):
    for B, nH in GRIDS:
        for op in (BF16, F16):
            v, want, check = R.indicator_case(B, nH, Lq, Lk, op)
            assert int(v.sum()) == B * nH * 64 and bool((v.sum(2) == 1).all()), "one key per (head, dimension)"
            iv = R.causal_table(B, Lq, Lk)
            n = R.vis_of(iv, Lk).sum(-1)
            assert torch.equal(n[0], torch.arange(Lq) + 1 + Lk - Lq)
            _, ref = _fp64_softmax_out(torch.zeros(B, nH, Lq, 64), torch.zeros(B, nH, Lk, 64), v, R.dense_of(R.vis_of(iv, Lk)))
            assert torch.equal(want.double(), ref.to(R._dt(op)).double())
            assert int(check.sum()) >= min(Lq, 4), "rows with an unambiguous reciprocal exist"
            assert bool(((want != 0).any(-1)).all()) and bool((want == 0).any()), "every row sees some indicator and misses another"


@pytest.mark.parametrize("layout", ["mixed", "block_gap"])
@pytest.mark.parametrize("L", BACKWARD)
def test_backward_probes(L, layout):
    """the probes sit at wave and block edges, their dimensions are distinct per head, and enough of them have a visible mean of V
    strictly inside (-1, 1) (the dK pattern needs dP - D != 0 on every visible key); the fp64 dV / dK show the claimed patterns"""
    rows = R.probe_rows(L)
    assert len(rows) <= 64 and {0, 31, 32, L - 1} <= set(rows) and (L < 129 or {127, 128} <= set(rows))
    for B, nH in GRIDS:
        for which in ("dv", "dk"):
            c = R.backward_case(B, nH, L, layout, which)
            for t in ("q", "k", "v", "do"):
                assert torch.equal(R.rnd(c[t], BF16), c[t])
            assert all(len(set(d)) == len(rows) for per_b in c["dims"] for d in per_b)
            assert float(c["usable"].float().mean()) >= 0.5
            pos = {rows[j] % 32 for j in c["usable"].any(0).any(0).nonzero().flatten().tolist()}
            assert {0, 31} <= pos, "usable probes at both ends of a wave"
            o, lse, dq, dk, dv = R.backward_reference(c)
            n = c["vis"].sum(-1).double()
            for b in range(B):
                for h in range(nH):
                    for j, (r, d) in enumerate(zip(rows, c["dims"][b][h])):
                        if which == "dv":
                            want = c["vis"][b, r].double() / n[b, r]
                            assert float((dv[b, h, :, d] - want).abs().max()) < 1e-12
                        elif bool(c["usable"][b, h, j]):
                            assert torch.equal(dk[b, h, :, d] != 0, c["vis"][b, r]), (b, h, r)
            if which == "dv":
                assert float((lse - n.log()[:, None]).abs().max()) < 1e-12


def test_empty_rows_positions():
    rows = R.empty_rows(387)
    assert {r % 32 for r in rows} == {0, 31} and len(rows) == len({r // 32 for r in rows}), "one row per wave, at position 0 or 31"
    iv = R.batch_table(2, 387, 387, "mixed", empty=True)
    assert bool((iv[:, rows] == 0).all()) and int((R.vis_of(iv, 387).sum(-1) == 0).sum()) == 2 * len(rows)
