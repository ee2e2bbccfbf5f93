"""GPU parity tests of the BATCHED KV-cached decode (csrc/decode_batch.hip; BASELINE cfg4 "batch=4 images").

The reference's Showo.mmu_generate is batch-1 (models/modeling_showo.py:204,229) and inference_mmu.py:87-177 walks the images one by
one, so the specification of `mmu_generate_batch` is: n calls of `mmu_generate`.  Every sequence of a batch runs the arithmetic of its
batch-1 run (same lane split, accumulation order and epilogue expressions per sequence), so the bar is BIT-EXACT: equal tokens, and equal
logits bits at the C ABI."""
import numpy as np
import pytest
import torch

import util
from util import O, dev

pytestmark = pytest.mark.gpu


def _prompts(d, g, n):
    """n mmu prompts of different lengths derived from the golden one: [<mmu>, <soi>, image tokens, <eoi>, text ...]"""
    rs = np.random.RandomState(7)
    base = g["ids"][0].tolist()
    out = []
    for b in range(n):
        extra = rs.randint(5, 200, size=3 * b + (b % 2)).tolist()
        row = base[:len(base) - (b % 4 if b % 2 else 0)] + extra  # the text tail behind <eoi> is 6 tokens long
        out.append(torch.tensor([row], dtype=torch.int64))
    return out


@pytest.mark.parametrize("precision", [0, 2])  # 2 (round 6): fp16 instances of the batched kernels + the fused split-bf16 head
@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_tiny_mmu_generate_batch_equals_n_single_calls(n, precision):
    g = util.golden("showo_tiny_mmu.npz")
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd)
    m.set_precision(precision)
    ids = _prompts(d, g, n)
    assert len({t.shape[1] for t in ids}) > 1  # ragged: every sequence has its own length, position and mask row
    masks = [O.mask_mmu(t, d.eoi_id).cuda() for t in ids]
    ids = [t.cuda() for t in ids]
    single = [[int(t) for t in m.mmu_generate(ids[b], attention_mask=masks[b], max_new_tokens=40, top_k=1)] for b in range(n)]
    assert single[0][:len(g["tokens"])] == g["tokens"].tolist()  # sequence 0 is the reference's own prompt
    for graph in (0, 1):  # eager steps == hipGraph replay, across the 16-step chunk boundaries
        m.decode_graph = graph
        got = m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=40, top_k=1)
        assert [[int(t) for t in r] for r in got] == single, graph
    # on-device visibility intervals instead of dense masks
    P = util.pkg().prompting_utils
    ivs = [P.intervals_for_mmu(t, eoi_id=d.eoi_id) for t in ids]
    got = m.mmu_generate_batch(idx=ids, attention_mask=ivs, max_new_tokens=40, top_k=1)
    assert [[int(t) for t in r] for r in got] == single
    # <eot>: every sequence stops right after ITS first <eot> (like n separate calls), the others keep going
    eot = single[1][5]
    want = [m.mmu_generate(ids[b], attention_mask=masks[b], max_new_tokens=40, top_k=1, eot_token=eot) for b in range(n)]
    got = m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=40, top_k=1, eot_token=eot)
    assert [[int(t) for t in r] for r in got] == [[int(t) for t in r] for r in want]
    assert len(got[1]) == single[1].index(eot) + 1
    # sampling / accuracy mode fall back to n sequential calls (same results as calling mmu_generate)
    m.set_precision(1)
    gp = m.mmu_generate_batch(idx=ids[:2], attention_mask=masks[:2], max_new_tokens=6, top_k=1)
    assert [[int(t) for t in r] for r in gp] == [[int(t) for t in m.mmu_generate(ids[b], attention_mask=masks[b], max_new_tokens=6, top_k=1)] for b in range(2)]


@pytest.mark.parametrize("precision", [0, 2])
def test_batch_decode_logits_are_the_bits_of_the_batch1_run(precision):
    """C ABI: showo_engine_batch_prefill / _batch_decode_greedy against showo_engine_prefill / _decode_greedy, logits workspace compared
    bit for bit after the same number of steps; capacity / order errors are refused"""
    g = util.golden("showo_tiny_mmu.npz")
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd)
    m.set_precision(precision)
    L = util.lib()
    eng = m.engine()
    n, steps = 3, 5
    ids = [t.cuda() for t in _prompts(d, g, n)]
    masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda().float().contiguous() for t in ids]
    V = d.vocab
    side = torch.cuda.Stream()
    ref_logits, ref_tokens = [], []
    for b in range(n):
        lg = torch.empty((V,), dtype=torch.float32, device="cuda")
        L.call("showo_engine_prefill", eng, L.ptr(ids[b]), None, L.ptr(masks[b]), ids[b].shape[1], L.ptr(lg), L.stream())
        tok = lg.argmax().reshape(1).to(torch.int64)
        out = torch.empty((steps,), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            L.call("showo_engine_decode_greedy", eng, L.ptr(tok), steps, L.ptr(out), L.ptr(lg), 1, L.stream())
        torch.cuda.synchronize()
        ref_logits.append(lg.clone()), ref_tokens.append(out.tolist())
    with pytest.raises(RuntimeError):  # no batch yet
        L.call("showo_engine_batch_prefill", eng, 0, L.ptr(ids[0]), None, L.ptr(masks[0]), ids[0].shape[1], None, L.stream())
    cap = max(t.shape[1] for t in ids) + steps + 1
    L.call("showo_engine_batch_begin", eng, n, cap)
    lgs = torch.empty((n, V), dtype=torch.float32, device="cuda")
    tok = torch.empty((n,), dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError):  # decode before every sequence has a prefill
        L.call("showo_engine_batch_decode_greedy", eng, L.ptr(tok), 1, L.ptr(tok), L.ptr(lgs), 0, L.stream())
    for b in range(n):
        L.call("showo_engine_batch_prefill", eng, b, L.ptr(ids[b]), None, L.ptr(masks[b]), ids[b].shape[1], L.ptr(lgs[b]), L.stream())
    tok.copy_(lgs.argmax(dim=1))
    out = torch.empty((n, steps), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        L.call("showo_engine_batch_decode_greedy", eng, L.ptr(tok), steps, L.ptr(out), L.ptr(lgs), 1, L.stream())
    torch.cuda.synchronize()
    assert out.tolist() == ref_tokens
    for b in range(n):
        assert torch.equal(lgs[b], ref_logits[b]), (b, float((lgs[b] - ref_logits[b]).abs().max()))
    big = torch.empty((n, 4096), dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError):  # more steps than the caches hold
        L.call("showo_engine_batch_decode_greedy", eng, L.ptr(tok), 4096, L.ptr(big), L.ptr(lgs), 0, L.stream())
    with pytest.raises(RuntimeError):
        L.call("showo_engine_batch_begin", eng, 9, 64)


# ---- a geometry between the tiny and the full-size one ------------------------------------------------------------------------------
# hidden 576 (9 heads): a weight row ends inside sub-span u = 1 (lanes 0..7); ffn 4672 = 2 * 2048 + 576: a third chunk that ends there
# too, so the out kernels run at C = 1 + 3 = 4 chunks.  (showo_engine_create takes hidden and ffn in multiples of 64 only: 4672 is the
# nearest such ffn that, like 4624, ends inside a sub-span; 4608 would end on a sub-span boundary.)
MID = dict(util.Wt.TINY, hidden=576, heads=9, ffn=4672)


def _mid_model(precision=0):
    d = util.Wt.ShowoDims(**MID)
    sd = util.Wt.make_showo_state(d, seed=11)
    m = util.build_showo(d, sd)
    m.set_precision(precision)
    return d, sd, m


def _mid_impl_runs(precision, impls):
    """logits after a prefill and after each of 4 decode steps, per showo_decode_set_impl setting"""
    g = util.golden("showo_tiny_mmu.npz")
    d, _, m = _mid_model(precision)
    L = util.lib()
    eng = m.engine()
    ids = dev(g["ids"]).to(torch.int64).contiguous()
    mask = dev(g["mask"]).float().reshape(1, 1, ids.shape[1], ids.shape[1]).contiguous()
    runs = []
    try:
        for impl in impls:
            L.call("showo_decode_set_impl", impl)
            logits = torch.empty((d.vocab,), dtype=torch.float32, device="cuda")
            L.call("showo_engine_prefill", eng, L.ptr(ids), None, L.ptr(mask), ids.shape[1], L.ptr(logits), L.stream())
            torch.cuda.synchronize()
            seq = [(-1, logits.clone())]
            for _ in range(4):
                tok = logits.argmax().reshape(1).to(torch.int64)
                L.call("showo_engine_decode_step", eng, L.ptr(tok), None, L.ptr(logits), L.stream())
                torch.cuda.synchronize()
                seq.append((int(tok), logits.clone()))
            runs.append(seq)
    finally:
        L.call("showo_decode_set_impl", 0)
    return runs


def test_mid_geometry_decode_layer_forms_equal_bits():
    """showo_decode_set_impl 1 (general seven-launch layer), 2 (plain chain) and 0 (default) give the same logits bits over a prefill and 4
    decode steps at H 576 / F 4672"""
    for a, b, c in zip(*_mid_impl_runs(0, (1, 2, 0))):
        assert a[0] == b[0] == c[0]
        assert torch.isfinite(c[1]).all()
        assert torch.equal(a[1], b[1]) and torch.equal(a[1], c[1]), (float((a[1] - c[1]).abs().max()), float((a[1] - b[1]).abs().max()))


def test_mid_geometry_fp16_decode_layer_forms():
    """precision 2 at the same geometry: the plain chain and the default layer agree bit for bit.  The general layer (impl 1) is NOT held
    to their bits here: its lm_head is the GEMV over the [hi | lo | hi] x [Whi | Whi | Wlo] image of 3 H columns, whose lane split
    (k' -> lane (k' % 512) / 8) puts the segments' products into the lanes' chains in ln_gemvB_kernel<.., HEAD3>'s grouping only where
    H is a multiple of 2048, Phi-1.5's width (tests/test_modules_gpu.py holds the three forms to equal bits there).  At H = 576 the
    same 3 H products are summed in another grouping: measured on an MI355X, the logits differ by at most 2.4e-7 (one fp32 ulp at their
    size); the figure is printed, the split head's values are bounded in tests/test_decode_narrow_kernels_gpu.py."""
    runs = _mid_impl_runs(2, (1, 2, 0))
    worst = 0.0
    for a, b, c in zip(*runs):
        assert torch.isfinite(a[1]).all() and torch.isfinite(c[1]).all()
        assert b[0] == c[0] and torch.equal(b[1], c[1]), float((b[1] - c[1]).abs().max())
        worst = max(worst, float((a[1] - c[1]).abs().max()))
    print(f"[parity] H 576 / F 4672 precision 2: general layer vs fused layer, worst |logit difference| over prefill + 4 steps {worst:.3e}")


@pytest.mark.parametrize("n", [3, 5, 8])
def test_mid_geometry_mmu_generate_batch_equals_n_single_calls(n):
    g = util.golden("showo_tiny_mmu.npz")
    d, _, m = _mid_model()
    ids = _prompts(d, g, n)
    masks = [O.mask_mmu(t, d.eoi_id).cuda() for t in ids]
    ids = [t.cuda() for t in ids]
    single = [[int(t) for t in m.mmu_generate(ids[b], attention_mask=masks[b], max_new_tokens=12, top_k=1)] for b in range(n)]
    for graph in (0, 1):
        m.decode_graph = graph
        got = m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=12, top_k=1)
        assert [[int(t) for t in r] for r in got] == single, graph


def test_mid_geometry_int8_kernels_give_the_bits_of_the_bf16_kernels_on_pow2_scaled_weights():
    """precision 3 at H 576 / F 4672 with power-of-two scales against the bf16 kernels on q * s: batch-1 (default layer, plain chain,
    general layer) and 2 / 3 / 4 / 8 slots, eager and graph (tests/test_int8_decode_gpu.py _bit_exact_case)"""
    from test_int8_decode_gpu import _bit_exact_case
    g = util.golden("showo_tiny_mmu.npz")
    d = util.Wt.ShowoDims(**MID)
    sd = util.Wt.make_showo_state(d, seed=11)
    ids = dev(g["ids"]).to(torch.int64).contiguous()
    mask = dev(g["mask"]).float().reshape(1, 1, ids.shape[1], ids.shape[1]).contiguous()
    batch = [(t.cuda().contiguous(), O.mask_mmu(t, d.eoi_id).cuda().float().contiguous()) for t in _prompts(d, g, 8)]
    _bit_exact_case(d, sd, ids, mask, 128, (0, 2, 1), batch)
