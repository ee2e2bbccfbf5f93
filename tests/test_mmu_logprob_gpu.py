"""GPU tests of token log-probabilities on the mmu paths (tiny model): return_logprobs on mmu_generate / mmu_generate_batch /
MmuSession.generate / generate_batch, the C entries behind them (showo_engine_decode_sample_lp, showo_engine_batch_decode_sample_lp),
and scoring of given tokens (Showo.score, MmuSession.score) against the CPU oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import util
import logprob_ref as R
from util import O, Wt, dev

pytestmark = pytest.mark.gpu

REL_MAX = 3e-2      # bf16 operands against the fp32 oracle: the relative-max logit gate of tests/test_modules_gpu.py
PRECISE_TOL = 1e-3  # precision 1 there


def _tiny(precision=0):
    g = util.golden("showo_tiny_mmu.npz")
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd)
    m.set_precision(precision)
    return g, d, sd, m


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _ints(toks):
    return [int(t) for t in toks]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).tolist()


def _configs(g):
    """greedy; top-k 5 / T 0.7 under the fixture's injected noise; top-k 20 + top_p 0.9 from a seeded generator"""
    return (("greedy", dict(top_k=1), None),
            ("top-k 5", dict(top_k=5, temperature=0.7, _exp_noise=dev(g["exp_noise_topk5"])), None),
            ("top-k 20 + top-p", dict(top_k=20, top_p=0.9), 11))


# ---- off is off ----------------------------------------------------------------------------------------------------------------------------
def test_return_logprobs_changes_no_token_and_off_returns_what_it_did():
    g, d, sd, m = _tiny()
    ids, mask = dev(g["ids"]), dev(g["mask"])
    for graph in (1, 0):
        m.decode_graph = graph
        for name, kw, seed in _configs(g):
            plain = m.mmu_generate(ids, attention_mask=mask, max_new_tokens=8, generator=None if seed is None else _gen(seed), **kw)
            assert isinstance(plain, list) and all(isinstance(t, torch.Tensor) and t.dim() == 0 for t in plain), name
            out = m.mmu_generate(ids, attention_mask=mask, max_new_tokens=8, generator=None if seed is None else _gen(seed),
                                 return_logprobs=True, **kw)
            assert isinstance(out, tuple) and len(out) == 2, name
            toks, lps = out
            assert _ints(toks) == _ints(plain), (name, graph)
            assert lps.dtype == torch.float32 and lps.is_cuda and tuple(lps.shape) == (len(toks),), name
            assert bool(torch.isfinite(lps).all()) and bool((lps <= 0).all()), name
            if name == "greedy":
                assert _ints(plain)[:6] == g["tokens"].tolist()
    m.decode_graph = 1


# ---- values: every step's log-probability is the reference's on that step's own logits row -------------------------------------------------
DRAWS = ((1, 1.0, 1.0), (5, 1.0, 0.7), (20, 0.9, 1.0))  # (top_k, top_p, temperature): greedy, plain top-k, nucleus


def _values_case(m, V, ids, mask, steps=6):
    L = util.lib()
    eng = m.engine()
    Lp = ids.shape[1]
    side = torch.cuda.Stream()
    for k, p, T in DRAWS:
        lg = torch.empty((V,), dtype=torch.float32, device="cuda")
        tok = torch.empty((1,), dtype=torch.int64, device="cuda")
        L.call("showo_engine_prefill", eng, L.ptr(ids), None, L.ptr(mask), Lp, L.ptr(lg), L.stream())
        if k == 1:
            L.call("showo_argmax_f32", L.ptr(lg), V, L.ptr(tok), L.stream())
        else:
            L.call("showo_sample_topk_topp", L.ptr(lg), V, k, p, T, None, 4242, 0, L.ptr(tok), L.stream())
        first = tok.clone()
        one_t, one_lp, one_rk = [], [], []
        for j in range(steps):
            out = torch.empty((1,), dtype=torch.int64, device="cuda")
            lp = torch.full((1,), 7.0, dtype=torch.float32, device="cuda")
            rk = torch.full((1,), 7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                L.call("showo_engine_decode_sample_lp", eng, L.ptr(tok), 1, L.ptr(out), L.ptr(lg), k, p, T, None, 4242, 1 + j, L.ptr(lp),
                       L.ptr(rk), 0, L.stream())
            torch.cuda.synchronize()
            assert int(out.item()) == int(tok.item())
            want_lp, want_rk = R.logprob_ref(lg.cpu().numpy(), int(out.item()))  # logits_ws holds this step's row
            print(f"[logprob] draw {(k, p, T)} step {j}: token {int(out.item())} lp {float(lp.item()):.6f} (fp64 {want_lp:.6f}) rank {int(rk.item())}")
            assert int(rk.item()) == want_rk and R.within_gate(lp.cpu().numpy(), np.array([want_lp])).all(), (k, p, T, j)
            if k == 1:
                assert want_rk == 0
            one_t.append(int(out.item())); one_lp.append(lp.clone()); one_rk.append(int(rk.item()))
        L.call("showo_engine_cache_rewind", eng, Lp, L.stream())
        tok.copy_(first)
        out = torch.empty((steps,), dtype=torch.int64, device="cuda")
        lp = torch.full((steps,), 7.0, dtype=torch.float32, device="cuda")
        rk = torch.full((steps,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            L.call("showo_engine_decode_sample_lp", eng, L.ptr(tok), steps, L.ptr(out), L.ptr(lg), k, p, T, None, 4242, 1, L.ptr(lp), L.ptr(rk), 1,
                   L.stream())
        torch.cuda.synchronize()
        assert out.tolist() == one_t, (k, p, T)
        assert _bits(lp) == _bits(torch.cat(one_lp)) and rk.tolist() == one_rk, (k, p, T)
        # logprobs == NULL is the call without: the same tokens
        L.call("showo_engine_cache_rewind", eng, Lp, L.stream())
        tok.copy_(first)
        out2 = torch.empty((steps,), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            L.call("showo_engine_decode_sample_lp", eng, L.ptr(tok), steps, L.ptr(out2), L.ptr(lg), k, p, T, None, 4242, 1, None, None, 1, L.stream())
        torch.cuda.synchronize()
        assert out2.tolist() == one_t


@pytest.mark.parametrize("precision", [0, 2, 3])
def test_loop_logprobs_are_the_reference_on_each_step_row_and_graph_equals_single_steps(precision):
    g, d, sd, m = _tiny(precision)
    ids = dev(g["ids"]).to(torch.int64).contiguous()
    mask = dev(g["mask"]).float().reshape(1, 1, ids.shape[1], ids.shape[1]).contiguous()
    _values_case(m, d.vocab, ids, mask)


def test_greedy_token_seam_form_indexes_with_the_advanced_position():
    """the greedy step of vocabularies >= 16384 ends in the token-seam launch, which advances the position itself: the tiny geometry with a
    16 639-token vocabulary takes it"""
    d = Wt.ShowoDims(**dict(Wt.TINY, vocab=16639, llm_vocab=16500))
    m = util.build_showo(d, Wt.make_showo_state(d, seed=5), max_batch=1, max_seq=64)
    ids = torch.randint(0, d.llm_vocab, (1, 19), generator=torch.Generator().manual_seed(1)).cuda().to(torch.int64).contiguous()
    mask = torch.zeros((1, 1, 19, 19), dtype=torch.float32)
    mask.masked_fill_(torch.triu(torch.ones(19, 19, dtype=torch.bool), 1), torch.finfo(torch.float32).min)
    _values_case(m, d.vocab, ids, mask.cuda().contiguous())


# ---- chunks and stops ------------------------------------------------------------------------------------------------------------------------
def test_logprobs_cross_chunk_boundaries_and_are_cut_with_the_tokens():
    g, d, sd, m = _tiny()
    ids, mask = dev(g["ids"]), dev(g["mask"])
    for kw, seed in ((dict(top_k=1), None), (dict(top_k=20, top_p=0.9, temperature=1.2), 5)):
        gen = (lambda: None) if seed is None else (lambda: _gen(seed))
        toks, lps = m.mmu_generate(ids, attention_mask=mask, max_new_tokens=40, generator=gen(), return_logprobs=True, **kw)
        assert len(toks) == 40 and tuple(lps.shape) == (40,)
        t = _ints(toks)
        stop = t.index(t[3])  # its 4th token, at its first appearance
        cut_t, cut_lp = m.mmu_generate(ids, attention_mask=mask, max_new_tokens=40, generator=gen(), eot_token=t[3], return_logprobs=True, **kw)
        assert _ints(cut_t) == t[:stop + 1] and _bits(cut_lp) == _bits(lps[:stop + 1])
        # max_new_tokens cuts both as well, inside a chunk
        few_t, few_lp = m.mmu_generate(ids, attention_mask=mask, max_new_tokens=21, generator=gen(), return_logprobs=True, **kw)
        assert _ints(few_t) == t[:21] and _bits(few_lp) == _bits(lps[:21])
        assert bool((lps <= 0).all()) and bool(torch.isfinite(lps).all())


# ---- batched equals batch-1 ----------------------------------------------------------------------------------------------------------------
def _uneven_eot(free, limit):
    """an <eot> among the tokens of the unstopped runs that ends them at different lengths (so that a slot idles while others decode)"""
    for cand in free[1] + free[0] + free[2]:
        if any(r[0] == cand for r in free):
            continue  # (a first token that is <eot> ends its sequence before it takes a slot)
        lens = [(r.index(cand) + 1 if cand in r else limit) for r in free]
        if min(lens) < max(lens):
            return cand
    raise AssertionError("no token stops the sequences at different lengths")


def _three_prompts(g, d):
    base = g["ids"][0].tolist()
    ids = [torch.tensor([base[:len(base) - c]], dtype=torch.int64).cuda() for c in (0, 2, 5)]
    masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda() for t in ids]
    return ids, masks


@pytest.mark.parametrize("precision", [0, 2])
def test_mmu_generate_batch_logprobs_are_the_batch1_bits(precision):
    g, d, sd, m = _tiny(precision)
    ids, masks = _three_prompts(g, d)
    for kw, seed in ((dict(top_k=1), None), (dict(top_k=[5, 20, None], temperature=[0.7, 1.0, 1.3], top_p=[None, 0.9, 0.8]), 9)):
        def one(b, gen, eot):
            a = {k: (v[b] if isinstance(v, list) else v) for k, v in kw.items()}
            return m.mmu_generate(ids[b], attention_mask=masks[b], max_new_tokens=20, generator=gen, eot_token=eot, return_logprobs=True, **a)
        gen = None if seed is None else _gen(seed)
        free = [_ints(one(b, gen, None)[0]) for b in range(3)]
        eot = _uneven_eot(free, 20)
        gen = None if seed is None else _gen(seed)
        want = [one(b, gen, eot) for b in range(3)]
        lens = [len(w[0]) for w in want]
        assert min(lens) < max(lens), lens
        for graph in (1, 0):
            m.decode_graph = graph
            toks, lps = m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=20, eot_token=eot,
                                             generator=None if seed is None else _gen(seed), return_logprobs=True, **kw)
            plain = m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=20, eot_token=eot,
                                         generator=None if seed is None else _gen(seed), **kw)
            assert isinstance(plain, list) and [_ints(r) for r in plain] == [_ints(r) for r in toks]
            for b in range(3):
                assert _ints(toks[b]) == _ints(want[b][0]), (b, graph)
                assert lps[b].dtype == torch.float32 and _bits(lps[b]) == _bits(want[b][1]), (b, graph)
        m.decode_graph = 1


def test_greedy_batch_with_logprobs_survives_a_first_token_that_is_eot():
    """the all-greedy batch with return_logprobs runs on the slot scheduler: a sequence whose FIRST token is <eot> never takes its
    slot, which then idles through the batched steps"""
    g, d, sd, m = _tiny()
    ids, masks = _three_prompts(g, d)
    firsts = [_ints(m.mmu_generate(ids[b], attention_mask=masks[b], max_new_tokens=1, top_k=1))[0] for b in range(3)]
    eot = firsts[2]
    want = [m.mmu_generate(ids[b], attention_mask=masks[b], max_new_tokens=9, top_k=1, eot_token=eot, return_logprobs=True) for b in range(3)]
    assert len(want[2][0]) == 1
    toks, lps = m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=9, top_k=1, eot_token=eot, return_logprobs=True)
    for b in range(3):
        assert _ints(toks[b]) == _ints(want[b][0]) and _bits(lps[b]) == _bits(want[b][1]), b


def test_session_generate_batch_logprobs_are_the_bits_of_generate_plus_rewind():
    g, d, sd, m = _tiny()
    ids = torch.from_numpy(g["ids"]).to(torch.int64)
    rs = np.random.RandomState(5)
    qs = [dev(torch.tensor([rs.randint(5, 200, size=n).tolist()], dtype=torch.int64)) for n in (1, 4, 7)]
    sess = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(O.mask_mmu(ids[:, :20], d.eoi_id)))
    sess.generate(dev(ids[:, 20:]), max_new_tokens=3, top_k=1)
    state = sess.mark()
    kw = dict(top_k=[1, 5, 20], temperature=[1.0, 0.7, 1.0], top_p=[None, None, 0.9])
    gen = _gen(5)
    want = []
    for b, q in enumerate(qs):
        mark = sess.mark()
        want.append(sess.generate(q, max_new_tokens=12, generator=gen, return_logprobs=True, **{k: v[b] for k, v in kw.items()}))
        sess.rewind(mark)
    eot = _uneven_eot([_ints(w[0]) for w in want], 12)
    gen = _gen(5)
    want = []
    for b, q in enumerate(qs):
        mark = sess.mark()
        want.append(sess.generate(q, max_new_tokens=12, generator=gen, eot_token=eot, return_logprobs=True, **{k: v[b] for k, v in kw.items()}))
        sess.rewind(mark)
    toks, lps = sess.generate_batch(idx=qs, max_new_tokens=12, generator=_gen(5), eot_token=eot, return_logprobs=True, **kw)
    assert sess.mark() == state
    for b in range(3):
        assert _ints(toks[b]) == _ints(want[b][0]) and _bits(lps[b]) == _bits(want[b][1]), b
    plain = sess.generate_batch(idx=qs, max_new_tokens=12, generator=_gen(5), eot_token=eot, **kw)
    assert [_ints(r) for r in plain] == [_ints(r) for r in toks]


# ---- scoring against the oracle --------------------------------------------------------------------------------------------------------------
def _oracle_scores(logits, labels, shift):
    """fp64 log-softmax of the oracle's fp32 logits [B, L, V] at labels [B, L] -> (lp [B, L], rank [B, L], logits used per entry)"""
    B, Lq, V = logits.shape
    lp = np.zeros((B, Lq))
    rk = np.full((B, Lq), -1, dtype=np.int64)
    for b in range(B):
        for r in range(1 if shift else 0, Lq):
            if labels[b, r] >= 0:
                lp[b, r], rk[b, r] = R.logprob_ref(logits[b, r - 1 if shift else r], labels[b, r])
    return lp, rk


def _check_scores(got, logits, labels, shift, g_rel, what):
    """|d lp| <= 2 g max|logit_ref| (|d lp| <= |d x_t| + |d lse| <= 2 max|d x|); a rank may differ only by entries the oracle itself holds
    within that distance of the target"""
    tol = 2.0 * g_rel * float(np.abs(logits).max())
    lp, rk = _oracle_scores(logits, labels, shift)
    glp, grk = got.logprobs.cpu().numpy().astype(np.float64), got.ranks.cpu().numpy().astype(np.int64)
    assert got.logprobs.dtype == torch.float32 and got.ranks.dtype == torch.int32 and glp.shape == lp.shape
    scored = rk >= 0
    assert scored.any() and np.array_equal(grk >= 0, scored)
    assert (glp[~scored] == 0.0).all() and (grk[~scored] == -1).all()
    err = np.abs(glp - lp)[scored].max()
    print(f"[logprob] {what}: max |d lp| {err:.3e} (gate {tol:.3e}), ranks differing {int((grk != rk).sum())} of {int(scored.sum())}")
    assert err <= tol, (what, err, tol)
    B, Lq, V = logits.shape
    for b, r in zip(*np.nonzero(grk != rk)):
        x = logits[b, r - 1 if shift else r].astype(np.float64)
        t = labels[b, r]
        near = int((np.abs(x - x[t]) < tol).sum()) - 1
        assert abs(int(grk[b, r]) - int(rk[b, r])) <= near, (what, b, r, grk[b, r], rk[b, r], near)


@pytest.mark.parametrize("precision", [0, 1])
def test_score_matches_the_oracle_on_mmu_and_t2i_rows(precision):
    g, d, sd, m = _tiny(precision)
    g_rel = PRECISE_TOL if precision == 1 else REL_MAX
    # shift=True: the mmu prompt and its six greedy tokens, twice; the second sequence scores every other label only
    seq = torch.cat([torch.from_numpy(g["ids"]), torch.from_numpy(g["tokens"])[None]], dim=1).to(torch.int64).repeat(2, 1)
    labels = seq.clone()
    labels[1, ::2] = -100
    mask = O.mask_mmu(seq, d.eoi_id)
    ref = O.showo_logits(O.to_torch(sd), d, seq, attention_mask=mask).numpy()
    got = m.score(dev(seq), attention_mask=dev(mask), labels=dev(labels))
    _check_scores(got, ref, labels.numpy(), True, g_rel, f"precision {precision} mmu rows, shift=True")
    assert bool((got.ranks[:, 0] == -1).all())  # column 0 is never scored
    n = int((got.ranks >= 0).sum())
    # chunks: n - 1 rows per chunk give the bits of one chunk of n
    a = m.score(dev(seq), attention_mask=dev(mask), labels=dev(labels), chunk_rows=n)
    b = m.score(dev(seq), attention_mask=dev(mask), labels=dev(labels), chunk_rows=n - 1)
    assert _bits(a.logprobs) == _bits(b.logprobs) == _bits(got.logprobs) and torch.equal(a.ranks, b.ranks)
    # the sequence log-likelihood is the sum
    assert abs(float(got.logprobs.sum(-1)[0]) - _oracle_scores(ref, labels.numpy(), True)[0][0].sum()) <= 30 * 2 * g_rel * np.abs(ref).max()
    # input_embeddings score like ids
    emb = m.showo.model.embed_tokens.weight.detach().float()[dev(seq)]
    e = m.score(input_embeddings=emb, attention_mask=dev(mask), labels=dev(labels))
    assert _bits(e.logprobs) == _bits(got.logprobs)
    # shift=False: the masked image rows of the t2i sequence, under the dense mask and under an IntervalMask
    t = util.golden("showo_tiny_t2i.npz")
    ids = torch.from_numpy(t["ids_cond"]).to(torch.int64)
    lab = torch.where(ids == d.mask_token_id, torch.from_numpy(t["final_input_ids"]).to(torch.int64), torch.full_like(ids, -100))
    tmask = O.mask_t2i(ids, d.pad_id, d.soi_id, d.eoi_id)
    tref = O.showo_logits(O.to_torch(sd), d, ids, attention_mask=tmask).numpy()
    got2 = m.score(dev(ids), attention_mask=dev(tmask), labels=dev(lab), shift=False)
    _check_scores(got2, tref, lab.numpy(), False, g_rel, f"precision {precision} t2i masked rows, shift=False")
    iv = util.pkg().prompting_utils.intervals_predict_next(dev(ids), pad_id=d.pad_id, soi_id=d.soi_id, eoi_id=d.eoi_id, rm_pad_in_image=True)
    got3 = m.score(dev(ids), attention_mask=iv, labels=dev(lab), shift=False)
    _check_scores(got3, tref, lab.numpy(), False, g_rel, f"precision {precision} t2i masked rows, IntervalMask")
    assert _bits(got3.logprobs) == _bits(got2.logprobs)
    # nothing to score: zeros and -1
    none = m.score(dev(ids), attention_mask=dev(tmask), labels=torch.full_like(ids, -100).cuda(), shift=False)
    assert bool((none.logprobs == 0).all()) and bool((none.ranks == -1).all()) and tuple(none.logprobs.shape) == tuple(ids.shape)
    with pytest.raises(ValueError):
        m.score(dev(ids), labels=dev(lab)[:, :5])


# ---- session scoring -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 1])
def test_session_score_agrees_with_generate_and_leaves_the_session_alone(precision):
    g, d, sd, m = _tiny(precision)
    L = util.lib()
    g_rel = PRECISE_TOL if precision == 1 else REL_MAX
    ids = torch.from_numpy(g["ids"]).to(torch.int64)
    pm = O.mask_mmu(ids[:, :20], d.eoi_id)
    q = dev(ids[:, 20:])
    sess = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(pm))
    start = sess.mark()
    toks, lps = sess.generate(q, max_new_tokens=6, top_k=1, return_logprobs=True)
    t = _ints(toks)
    sess.rewind(start)
    cont = torch.cat([ids[:, 20:], torch.tensor([t], dtype=torch.int64)], dim=1)
    before = sess._be.cached_rows()
    sc = sess.score(dev(cont))
    assert sess._be.cached_rows() == before == 20 and sess.mark() == start
    assert tuple(sc.logprobs.shape) == (cont.shape[1],) and sc.ranks.dtype == torch.int32
    # both within the oracle gate of the oracle on the full sequence, hence within twice the gate of each other (NOT bit-equal: append
    # rows and decode steps are different kernels)
    full = torch.cat([ids, torch.tensor([t], dtype=torch.int64)], dim=1)
    ref = O.showo_logits(O.to_torch(sd), d, full, attention_mask=O.mask_mmu(full, d.eoi_id)).numpy()[0]
    tol = 2.0 * g_rel * float(np.abs(ref).max())
    want = np.array([R.logprob_ref(ref[19 + j], int(cont[0, j]))[0] for j in range(cont.shape[1])])
    got = sc.logprobs.cpu().numpy().astype(np.float64)
    gen = lps.cpu().numpy().astype(np.float64)
    print(f"[logprob] precision {precision} session: score vs oracle {np.abs(got - want).max():.3e}, generate vs oracle "
          f"{np.abs(gen - want[-6:]).max():.3e}, score vs generate {np.abs(got[-6:] - gen).max():.3e} (gate {tol:.3e})")
    assert np.abs(got - want).max() <= tol and np.abs(gen - want[-6:]).max() <= tol and np.abs(got[-6:] - gen).max() <= 2 * tol
    assert bool((sc.ranks[-6:] >= 0).all())
    # the next generate returns the bits of a run without the score
    again_t, again_lp = sess.generate(q, max_new_tokens=6, top_k=1, return_logprobs=True)
    assert _ints(again_t) == t and _bits(again_lp) == _bits(lps)
    # behind a pending token: the pending token is fed first; a list is scored against the same state, one after the other
    state = sess.mark()
    c1 = dev(torch.tensor([[7, 204, 113]], dtype=torch.int64))
    c2 = dev(torch.tensor([[80, 27, 5, 9, 11]], dtype=torch.int64))
    both = sess.score([c1, c2])
    assert sess.mark() == state and sess._be.cached_rows() == state[0]
    s1, s2 = sess.score(c1), sess.score(c2)
    assert _bits(both[0].logprobs) == _bits(s1.logprobs) and _bits(both[1].logprobs) == _bits(s2.logprobs)
    assert torch.equal(both[0].ranks, s1.ranks) and torch.equal(both[1].ranks, s2.ranks)
    assert tuple(s2.logprobs.shape) == (5,) and bool(torch.isfinite(s2.logprobs).all())
    assert int(s2.ranks.min()) >= 0
    if precision == 0:  # (precision 1 at the tiny shape keeps no KV cache: the recompute session)
        n = C.c_int()
        L.call("showo_engine_cache_state", m.engine(), C.byref(n), None, None, None)
        assert n.value == state[0]
