"""Reduced step 0 of `Showo.t2i_generate` (prefix reuse): step 0 skips the leading rows that no later row can see and runs the
identical unconditional sequences of a CFG call once.  Everything here is an exact property: token ids (and the step-0 logits) with
the reduction on must EQUAL those with it off (`reduce_step0=False`) and those of the path without prefix reuse
(`reuse_prefix=False`) -- same arithmetic per row, same K-summation order (the reduced GEMMs keep the split count of the full shape).
`showo_engine_t2i_step0` reports what step 0 ran, so no test passes with the reduction silently off; the expected trim is computed
here on the host from the dense mask.  Full-size random-init weights throughout: the shapes and branches of the benchmark."""
import ctypes as C

import numpy as np
import pytest
import torch

import util

pytestmark = pytest.mark.gpu

B8, N, TEXT = 8, 256, 128
PREFIX = TEXT + 1          # position of <soi>
SEQ = TEXT + 1 + N + 2     # 387


@pytest.fixture(scope="module")
def env():
    P = util.pkg()
    torch.manual_seed(0)
    m = P.synthetic.random_init_showo(max_batch=16, max_seq=SEQ, ln_jitter=True).eval()
    uni = P.synthetic.prompting(TEXT)
    yield P, m, uni
    m.set_precision(0)


def _run(P, m, ic, iu, mask, steps=18, w=5.0, seed=5, **kw):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return m.t2i_generate(input_ids=ic.clone(), uncond_input_ids=iu, attention_mask=mask, temperature=1.0, timesteps=steps,
                          guidance_scale=w, generator=gen, config=P.gen_config(), **kw)


def _step0(m):
    out = (C.c_int * 4)()
    util.lib().call("showo_engine_t2i_step0", m.engine(), out)
    return [int(v) for v in out[:3]]


def _host_trim(mask, seqs):
    """per sequence the largest p <= PREFIX such that no row >= p sees a column < p (dense mask: 0 = visible); the uniform trim
    is the smallest of them"""
    ps = []
    for s in seqs:
        vis = (mask[s, 0] == 0).cpu().numpy()
        L = vis.shape[0]
        first = np.where(vis.any(1), vis.argmax(1), L)
        sufmin = np.minimum.accumulate(first[::-1])[::-1]
        ps.append(max(p for p in range(PREFIX + 1) if sufmin[p] >= p))
    return min(ps)


def _pads(uni, ids):
    return (ids == int(uni.sptids_dict['<|pad|>'])).sum(1).tolist()


def _mask(P, uni, ic, iu):
    sp = uni.sptids_dict
    both = torch.cat([ic, iu], dim=0) if iu is not None else ic
    return P.prompting_utils.create_attention_mask_predict_next(both, pad_id=int(sp['<|pad|>']), soi_id=int(sp['<|soi|>']),
                                                                eoi_id=int(sp['<|eoi|>']), rm_pad_in_image=True)


def _all_equal(P, m, ic, iu, mask, **kw):
    """default (graph, reduced) == eager reduced == reduction off == no prefix reuse; returns the default run's tokens and what
    its step 0 ran"""
    a = _run(P, m, ic, iu, mask, **kw)
    s0 = _step0(m)
    for sw in (dict(use_graph=0), dict(reduce_step0=False), dict(reuse_prefix=False)):
        b = _run(P, m, ic, iu, mask, **sw, **kw)
        assert torch.equal(a, b), (sw, float((a == b).float().mean()))
    return a, s0


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("batch", [8, 1])
def test_bench_batch_tokens_equal_and_step0_is_reduced(env, precision, batch):
    """the benchmark's inputs (batch 8) and batch 1 (the reduced residual GEMM would split K 10 ways, the full shape 8: pinned)"""
    P, m, uni = env
    ic, iu, mask = P.synthetic.t2i_inputs(uni, batch, N, m.mask_token_id)
    m.set_precision(precision)
    try:
        toks, s0 = _all_equal(P, m, ic, iu, mask)
    finally:
        m.set_precision(0)
    assert tuple(toks.shape) == (batch, N) and int(toks.min()) >= 0 and int(toks.max()) < 8192
    nseq0 = batch + 1 if batch > 1 else 2  # the unconditional sequences are one sequence
    p = _host_trim(mask, range(nseq0))
    pads = _pads(uni, torch.cat([ic, iu[:1]]))
    print(f"[parity] t2i step 0, batch {batch}, precision {precision}: ran {s0[0]} sequences x rows [{s0[1]}, {SEQ}) = {s0[2]} of "
          f"{2 * batch * SEQ} rows; tokens equal with the reduction off and without prefix reuse")
    assert p == min(pads) and p >= 64
    assert s0 == [nseq0, p, nseq0 * (SEQ - p)]


@pytest.mark.parametrize("case", ["batch1-p0", "batch1-p1", "batch1-p2", "batch8-nocfg"])
def test_small_batches_equal_the_path_without_prefix_reuse(env, case):
    """reduced step 0 vs `reuse_prefix=False` where fewer than 16 sequences run.  There the residual GEMM splits K and the split count
    follows M (2 sequences: 10 parts at the 516 active rows, 8 at the full 774; 8 sequences: 3 and 2).  Step 0 AND the active-rows
    steps 1..17 are pinned to the full shape's count, so the default path and the path without reuse sum in one order.  Before the
    pin of the later steps these cases disagreed, with the reduction on or off alike (token agreement 0.8789 at batch 1 precision 0,
    0.9961 at precision 2, 0.9829 at batch 8 without CFG)."""
    P, m, uni = env
    batch, precision, kw = (8, 0, dict(steps=6, w=0.0)) if case == "batch8-nocfg" else (1, int(case[-1]), dict())
    ic, iu, mask = P.synthetic.t2i_inputs(uni, batch, N, m.mask_token_id)
    if case == "batch8-nocfg":
        iu, mask = None, mask[:B8].contiguous()
    m.set_precision(precision)
    try:
        on = _run(P, m, ic, iu, mask, **kw)
        off = _run(P, m, ic, iu, mask, reduce_step0=False, **kw)
        full = _run(P, m, ic, iu, mask, reuse_prefix=False, **kw)
    finally:
        m.set_precision(0)
    print(f"[parity] t2i {case}: token agreement with reuse_prefix=False: reduced step 0 {float((on == full).float().mean()):.4f}, "
          f"full step 0 {float((off == full).float().mean()):.4f}")
    assert torch.equal(on, off)
    assert torch.equal(on, full)


def test_inpainting_batch_trims_but_does_not_share(env):
    """known image tokens that differ per sample (the 512x512 inpainting workload's shape of input): the unconditional sequences
    differ, every one of them runs; the pad trim still applies"""
    P, m, uni = env
    ic, iu, mask = P.synthetic.t2i_inputs(uni, B8, N, m.mask_token_id)
    cfg = P.gen_config()
    off = cfg.model.showo.llm_vocab_size + cfg.model.showo.num_new_special_tokens
    g = torch.Generator(device="cuda").manual_seed(3)
    known = torch.rand((B8, N), device="cuda", generator=g) < 0.5
    codes = torch.randint(0, 8192, (B8, N), device="cuda", generator=g) + off
    img0 = SEQ - (N + 1)
    for t in (ic, iu):
        t[:, img0:img0 + N] = torch.where(known, codes, t[:, img0:img0 + N])
    toks, s0 = _all_equal(P, m, ic, iu, mask, steps=6)
    assert torch.equal(toks[known], (codes - off)[known])  # known tokens come back untouched
    p = _host_trim(mask, range(2 * B8))
    assert p > 0 and s0 == [2 * B8, p, 2 * B8 * (SEQ - p)]


def test_unconditional_rows_that_differ_are_not_shared(env):
    P, m, uni = env
    ic, iu, mask = P.synthetic.t2i_inputs(uni, B8, N, m.mask_token_id)
    p = _host_trim(mask, range(2 * B8))
    # one id of one unconditional prompt
    iu2 = iu.clone()
    iu2[3, TEXT - 1] = ic[0, TEXT - 1]
    assert not torch.equal(iu2, iu)
    _, s0 = _all_equal(P, m, ic, iu2, mask, steps=4)
    assert s0 == [2 * B8, p, 2 * B8 * (SEQ - p)]
    # one interval row of one unconditional sequence (a pad row that sees one column less: still two runs at most per row)
    mask2 = mask.clone()
    mask2[B8 + 5, 0, 10, 0] = mask[0, 0, 0, SEQ - 1]  # the "masked" value
    assert float(mask[0, 0, 0, SEQ - 1]) != 0.0
    _, s0 = _all_equal(P, m, ic, iu, mask2, steps=4)
    assert s0[0] == 2 * B8 and s0[2] == s0[0] * (SEQ - s0[1])
    assert s0[1] == _host_trim(mask2, range(2 * B8))


def test_pad_free_batch_is_not_trimmed(env):
    P, m, uni = env
    ic, iu, _ = P.synthetic.t2i_inputs(uni, B8, N, m.mask_token_id)
    pad = int(uni.sptids_dict['<|pad|>'])
    g = torch.Generator(device="cuda").manual_seed(4)
    fill = torch.randint(0, 50000, (1, SEQ), device="cuda", generator=g)
    ic = torch.where(ic == pad, fill.expand_as(ic), ic).contiguous()
    iu = torch.where(iu == pad, fill.expand_as(iu), iu).contiguous()
    mask = _mask(P, uni, ic, iu)
    assert _host_trim(mask, range(2 * B8)) == 0
    _, s0 = _all_equal(P, m, ic, iu, mask, steps=4)
    assert s0 == [B8 + 1, 0, (B8 + 1) * SEQ]  # no trim; the unconditional sequences are still one sequence


def test_masks_that_rule_out_prefix_reuse_run_the_full_step(env):
    """a dense mask that is not an interval mask, and the all-visible mask (text rows see image columns): no reuse, no reduction,
    the tokens of the eager loop without reuse"""
    P, m, uni = env
    ic, iu, mask = P.synthetic.t2i_inputs(uni, B8, N, m.mask_token_id)
    holes = mask.clone()
    holes[0, 0, 300, 150] = mask[0, 0, 0, SEQ - 1]
    holes[0, 0, 300, 200] = mask[0, 0, 0, SEQ - 1]  # an image row with three visible runs
    for am in (holes, torch.zeros_like(mask)):
        a = _run(P, m, ic, iu, am, steps=4)
        assert _step0(m) == [2 * B8, 0, 2 * B8 * SEQ]
        b = _run(P, m, ic, iu, am, steps=4, use_graph=0, reuse_prefix=False)
        assert torch.equal(a, b)


def test_without_cfg_nothing_is_shared_and_the_trim_is_exact(env):
    P, m, uni = env
    ic, iu, mask = P.synthetic.t2i_inputs(uni, B8, N, m.mask_token_id)
    mask = mask[:B8].contiguous()
    _, s0 = _all_equal(P, m, ic, None, mask, steps=6, w=0.0)
    p = _host_trim(mask, range(B8))
    assert p == min(_pads(uni, ic)) and s0 == [B8, p, B8 * (SEQ - p)]


def test_poisoned_cache_rows_never_reach_a_result(env):
    """step 0 never writes the K cache rows before the trim: with the whole K cache set to NaN bit patterns at the start of the
    call the tokens are those of the full step"""
    P, m, uni = env
    ic, iu, mask = P.synthetic.t2i_inputs(uni, B8, N, m.mask_token_id)
    ref = _run(P, m, ic, iu, mask, reduce_step0=False)
    L = util.lib()
    for precision in (0, 1):
        m.set_precision(precision)
        if precision:
            ref = _run(P, m, ic, iu, mask, reduce_step0=False)
        L.call("showo_engine_t2i_debug", m.engine(), None, 1)
        try:
            got = _run(P, m, ic, iu, mask)
            s0 = _step0(m)
            got_eager = _run(P, m, ic, iu, mask, use_graph=0)
        finally:
            L.call("showo_engine_t2i_debug", m.engine(), None, 0)
            m.set_precision(0)
        assert s0[0] == B8 + 1 and s0[1] >= 64
        assert torch.equal(got, ref) and torch.equal(got_eager, ref)


def test_step0_logits_are_bit_equal(env):
    """not only the tokens: the logit rows that step 0 hands to the sampler, bit for bit, reduced vs full vs no reuse"""
    P, m, uni = env
    ic, iu, mask = P.synthetic.t2i_inputs(uni, B8, N, m.mask_token_id)
    g = torch.Generator(device="cuda").manual_seed(7)
    en = -torch.log1p(-torch.rand((2, B8 * N, 8192), device="cuda", generator=g))  # Exp(1)
    un = torch.rand((2, B8, N), device="cuda", generator=g)
    buf = torch.zeros((2 * B8 * N, 8192), dtype=torch.float32, device="cuda")
    L = util.lib()
    L.call("showo_engine_t2i_debug", m.engine(), L.ptr(buf), 0)
    try:
        got = []
        for kw in (dict(), dict(reduce_step0=False), dict(reuse_prefix=False)):
            buf.zero_()
            toks = _run(P, m, ic, iu, mask, steps=2, _exp_noise=en, _uniform=un, **kw)
            if not kw:
                assert _step0(m)[0] == B8 + 1 and _step0(m)[1] >= 64
            torch.cuda.synchronize()
            got.append((toks, buf.clone()))
    finally:
        L.call("showo_engine_t2i_debug", m.engine(), None, 0)
    assert bool(torch.isfinite(got[0][1]).all()) and float(got[0][1].abs().max()) > 0
    for toks, lg in got[1:]:
        assert torch.equal(lg.view(torch.int32), got[0][1].view(torch.int32))
        assert torch.equal(toks, got[0][0])
