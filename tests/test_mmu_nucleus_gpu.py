"""GPU tests of nucleus (top-p) sampling on the mmu decode paths: the graph-captured loop (showo_engine_decode_sample_p), the batched
slots (showo_engine_batch_decode_sample_p) and the Python entry points (mmu_generate, mmu_generate_batch, MmuSession, the precision-1
recompute path).  Every path calls the one row function of csrc/sample_row.h, so a path equals another in tokens, bit for bit; the
draw itself is held to the reference in tests/test_nucleus_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import util
import nucleus_ref as N
from util import O, Wt, dev

pytestmark = pytest.mark.gpu


def _prompts(d, g, n):
    """n mmu prompts of different lengths derived from the golden one (as tests/test_mmu_batch_sample_gpu.py builds them)"""
    rs = np.random.RandomState(7)
    base = g["ids"][0].tolist()
    out = []
    for b in range(n):
        extra = rs.randint(5, 200, size=3 * b + (b % 2)).tolist()
        out.append(torch.tensor([base[:len(base) - (b % 4 if b % 2 else 0)] + extra], dtype=torch.int64))
    return out


def _tiny(precision):
    g = util.golden("showo_tiny_mmu.npz")
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd)
    m.set_precision(precision)
    return g, d, m


def _ints(rows):
    return [[int(t) for t in r] for r in rows]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _draw(L, lg, V, k, p, T, noise, seed, step, tok):
    """one token from a logits row with slot settings (k, p, T): the arg-max for k == 1"""
    if k == 1:
        L.call("showo_argmax_f32", L.ptr(lg), V, L.ptr(tok), L.stream())
    else:
        L.call("showo_sample_topk_topp", L.ptr(lg), V, k, p, T, L.ptr(noise), seed, step, L.ptr(tok), L.stream())


# ---- 7. the loop equals the steps ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("graph", [0, 1])
def test_decode_sample_p_equals_decode_step_plus_the_draw_by_hand(precision, graph):
    g, d, m = _tiny(precision)
    L = util.lib()
    eng, V, steps = m.engine(), d.vocab, 12
    ids = dev(g["ids"]).to(torch.int64).contiguous()
    mask = dev(g["mask"]).float().reshape(1, 1, ids.shape[1], ids.shape[1]).contiguous()
    E = dev(np.random.RandomState(2).exponential(size=(1 + steps, V)).astype(np.float32))
    side = torch.cuda.Stream()
    for k, p, T in ((20, 0.8, 0.9), (0, 0.6, 1.0)):
        for noise in (E, None):
            lg = torch.empty((V,), dtype=torch.float32, device="cuda")
            tok = torch.empty((1,), dtype=torch.int64, device="cuda")
            L.call("showo_engine_prefill", eng, L.ptr(ids), None, L.ptr(mask), ids.shape[1], L.ptr(lg), L.stream())
            _draw(L, lg, V, k, p, T, noise, 31337, 0, tok)
            hand = [int(tok.item())]
            for j in range(1, steps + 1):
                L.call("showo_engine_decode_step", eng, L.ptr(tok), None, L.ptr(lg), L.stream())
                _draw(L, lg, V, k, p, T, noise, 31337, j, tok)
                hand.append(int(tok.item()))
            L.call("showo_engine_prefill", eng, L.ptr(ids), None, L.ptr(mask), ids.shape[1], L.ptr(lg), L.stream())
            _draw(L, lg, V, k, p, T, noise, 31337, 0, tok)
            out = torch.empty((steps,), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                L.call("showo_engine_decode_sample_p", eng, L.ptr(tok), steps, L.ptr(out), L.ptr(lg), k, p, T, L.ptr(noise), 31337, 1, graph,
                       L.stream())
            torch.cuda.synchronize()
            assert [hand[0]] + out.tolist() == hand, (k, p, T, noise is None)
            assert len(set(hand)) > 2


# ---- 8. a batched slot draws the bits of its batch-1 run ---------------------------------------------------------------------------------
# per-slot (top_k, top_p, temperature): greedy, top-k only, top-p only, top-k + top-p
SLOTS = [(1, 0.5, 1.0), (5, 1.0, 0.7), (0, 0.8, 1.3), (20, 0.7, 1.0)]


@pytest.mark.parametrize("precision", [0, 2, 3])
@pytest.mark.parametrize("graph", [0, 1])
def test_batch_decode_sample_p_is_the_tokens_of_the_batch1_runs(precision, graph):
    """two consecutive calls (draw indices continue across the chunk boundary); slot 2 draws from an injected Exp(1) table; in the second
    call slot 3's budget ends early"""
    g, d, m = _tiny(precision)
    L = util.lib()
    eng = m.engine()
    V, n, s1, s2 = d.vocab, len(SLOTS), 5, 6
    steps = s1 + s2
    ids = [t.cuda() for t in _prompts(d, g, n)]
    masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda().float().contiguous() for t in ids]
    seeds = [7654321 + 1000 * b for b in range(n)]
    noise = [None, None, dev(np.random.RandomState(3).exponential(size=(1 + steps, V)).astype(np.float32)), None]
    side = torch.cuda.Stream()
    ref = []
    for b, (k, p, T) in enumerate(SLOTS):
        lg = torch.empty((V,), dtype=torch.float32, device="cuda")
        tok = torch.empty((1,), dtype=torch.int64, device="cuda")
        L.call("showo_engine_prefill", eng, L.ptr(ids[b]), None, L.ptr(masks[b]), ids[b].shape[1], L.ptr(lg), L.stream())
        _draw(L, lg, V, k, p, T, noise[b], seeds[b], 0, tok)
        out = torch.empty((steps,), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            L.call("showo_engine_decode_sample_p", eng, L.ptr(tok), steps, L.ptr(out), L.ptr(lg), k, p, T, L.ptr(noise[b]), seeds[b], 1, graph,
                   L.stream())
        torch.cuda.synchronize()
        ref.append(out.tolist())
    L.call("showo_engine_batch_begin", eng, n, max(t.shape[1] for t in ids) + steps + 1)
    lgs = torch.empty((n, V), dtype=torch.float32, device="cuda")
    tok = torch.empty((n,), dtype=torch.int64, device="cuda")
    for b, (k, p, T) in enumerate(SLOTS):
        L.call("showo_engine_batch_prefill", eng, b, L.ptr(ids[b]), None, L.ptr(masks[b]), ids[b].shape[1], L.ptr(lgs[b]), L.stream())
        _draw(L, lgs[b], V, k, p, T, noise[b], seeds[b], 0, tok[b:b + 1])
    arr = lambda t, v: C.cast((t * n)(*v), C.c_void_p)
    got = [[] for _ in range(n)]
    for cnt, d0, budget in ((s1, 1, [s1] * n), (s2, 1 + s1, [s2, s2, s2, 3])):
        out = torch.empty((n, cnt), dtype=torch.int64, device="cuda")
        prod = (C.c_int * n)()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            L.call("showo_engine_batch_decode_sample_p", eng, L.ptr(tok), cnt, L.ptr(out), L.ptr(lgs), arr(C.c_int, [s[0] for s in SLOTS]),
                   arr(C.c_float, [s[1] for s in SLOTS]), arr(C.c_float, [s[2] for s in SLOTS]), arr(C.c_uint64, seeds), arr(C.c_int, [d0] * n),
                   arr(C.c_void_p, [L.ptr(z) for z in noise]), arr(C.c_int, budget), -1, C.cast(prod, C.c_void_p), graph, L.stream())
        torch.cuda.synchronize()
        assert list(prod) == budget
        rows = out.tolist()
        for b in range(n):
            assert rows[b][budget[b]:] == [-1] * (cnt - budget[b])
            got[b] += rows[b][:budget[b]]
    for b in range(n):
        assert got[b] == ref[b][:len(got[b])], (b, SLOTS[b])
    assert [len(r) for r in got] == [steps, steps, steps, s1 + 3]


# ---- 9. the Python paths agree -------------------------------------------------------------------------------------------------------------
def _single(m, ids, masks, gen=None, **kw):
    out = []
    for b in range(len(ids)):
        a = {k: (v[b] if isinstance(v, list) else v) for k, v in kw.items()}
        out.append([int(t) for t in m.mmu_generate(ids[b], attention_mask=masks[b], generator=gen, **a)])
    return out


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("n", [3, 12])
def test_mmu_generate_batch_with_top_p_draws_like_sequential_calls(n, precision):
    """per-sequence top_p (None, >= 1 and inside (0, 1)) next to greedy and top-k sequences; n = 12 refills the 8 slots"""
    g, d, m = _tiny(precision)
    ids = [t.cuda() for t in _prompts(d, g, n)]
    masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda() for t in ids]
    ks, ts, ps = [5, None, 1, 20], [0.7, 1.3, 1.0, 1.0], [0.8, 0.6, 0.5, None]
    mixed = dict(top_k=[ks[b % 4] for b in range(n)], temperature=[ts[b % 4] for b in range(n)], top_p=[ps[b % 4] for b in range(n)])
    for kw in (dict(top_k=None, temperature=0.9, top_p=0.7), mixed):
        want = _single(m, ids, masks, _gen(5), max_new_tokens=24, **kw)
        for graph in (0, 1):
            m.decode_graph = graph
            got = _ints(m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=24, generator=_gen(5), **kw))
            assert got == want, graph
    m.decode_graph = 1
    # the nucleus is not a no-op here: without top_p the same seeds draw other tokens
    kw = dict(top_k=None, temperature=0.9)
    assert _single(m, ids, masks, _gen(5), max_new_tokens=24, **kw) != _single(m, ids, masks, _gen(5), max_new_tokens=24, top_p=0.7, **kw)


def test_session_generate_with_top_p_equals_mmu_generate_on_the_full_prompt():
    """prefix = the first 20 ids, question = the last 5 (the split of test_mmu_session_gpu's token-equality test, precision 0), with the
    fixture's recorded Exp(1) draws and with Philox draws"""
    g, d, m = _tiny(0)
    ids = torch.from_numpy(g["ids"]).to(torch.int64)
    pm = O.mask_mmu(ids[:, :20], d.eoi_id)
    for graph in (0, 1):
        m.decode_graph = graph
        for kw in (dict(top_k=5, temperature=0.7, top_p=0.8, _exp_noise=dev(g["exp_noise_topk5"])),
                   dict(top_k=None, temperature=1.3, top_p=0.6, _exp_noise=dev(g["exp_noise_full"])),
                   dict(top_k=20, temperature=1.0, top_p=0.7)):
            want = [int(t) for t in m.mmu_generate(dev(ids), attention_mask=dev(g["mask"]), max_new_tokens=8, generator=_gen(3), **kw)]
            sess = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(pm))
            got = [int(t) for t in sess.generate(dev(ids[:, 20:]), max_new_tokens=8, generator=_gen(3), **kw)]
            assert got == want, (graph, kw.get("top_p"))
    m.decode_graph = 1


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("n", [3, 11])
def test_session_generate_batch_with_top_p_equals_generate_plus_rewind(n, precision):
    g, d, m = _tiny(precision)
    ids = torch.from_numpy(g["ids"]).to(torch.int64)
    rs = np.random.RandomState(5)
    qs = [dev(torch.tensor([rs.randint(5, 200, size=1 + (3 * b + b % 2) % 9).tolist()], dtype=torch.int64)) for b in range(n)]
    sess = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(O.mask_mmu(ids[:, :20], d.eoi_id)))
    sess.generate(dev(ids[:, 20:]), max_new_tokens=3, top_k=1)
    state = sess.mark()
    ks, ts, ps = [5, None, 1, 20], [0.7, 1.3, 1.0, 1.0], [0.8, 0.6, 0.5, None]
    kw = dict(top_k=[ks[b % 4] for b in range(n)], temperature=[ts[b % 4] for b in range(n)], top_p=[ps[b % 4] for b in range(n)])
    gen = _gen(5)
    want = []
    for b, q in enumerate(qs):
        mark = sess.mark()
        want.append([int(t) for t in sess.generate(q, max_new_tokens=20, generator=gen, **{k: v[b] for k, v in kw.items()})])
        sess.rewind(mark)
    for graph in (0, 1):
        m.decode_graph = graph
        got = _ints(sess.generate_batch(idx=qs, max_new_tokens=20, generator=_gen(5), **kw))
        assert got == want, graph
        assert sess.mark() == state
    m.decode_graph = 1


def test_precision_1_recompute_path_takes_top_p():
    """accuracy mode at the tiny shape runs the reference's no-cache algorithm (_mmu_generate_recompute): with injected noise its tokens
    are what a host loop draws by nucleus_ref from the same engine logits (showo_engine_forward_rows on the grown sequence and mask)"""
    g, d, m = _tiny(1)
    L = util.lib()
    eng, V, steps = m.engine(), d.vocab, 8
    ids = dev(g["ids"]).to(torch.int64)
    k, p, T = None, 0.8, 1.0
    E = np.random.RandomState(4).exponential(size=(steps, V)).astype(np.float32)
    got = [int(t) for t in m.mmu_generate(ids, attention_mask=dev(g["mask"]), max_new_tokens=steps, top_k=k, temperature=T, top_p=p,
                                          _exp_noise=dev(E))]
    tab = m.showo.model.embed_tokens.weight.detach().float()
    emb = tab[ids].contiguous()
    Lq = emb.shape[1]
    mask = dev(g["mask"]).float().reshape(1, 1, Lq, Lq).contiguous()
    neg = float(torch.finfo(torch.float32).min)
    row = torch.empty((1,), dtype=torch.int32, device="cuda")
    lg = torch.empty((V,), dtype=torch.float32, device="cuda")
    want = []
    for step in range(steps):
        row.fill_(Lq - 1)
        L.call("showo_engine_forward_rows", eng, None, L.ptr(emb), L.ptr(mask), 1, Lq, L.ptr(row), 1, 0, V, L.ptr(lg), L.stream())
        t, pk, keep = N.draw_reference(lg.cpu(), k, p, T, torch.from_numpy(E[step]))
        assert N.ref_nucleus(lg.cpu(), k, p, T)[2] >= N.MARGIN, step
        want.append(t)
        grown = torch.full((1, 1, Lq + 1, Lq + 1), neg, dtype=torch.float32, device="cuda")
        grown[0, 0, :Lq, :Lq] = mask[0, 0]
        grown[0, 0, Lq, :Lq] = mask[0, 0, Lq - 1]
        grown[0, 0, Lq, Lq] = 0.0
        mask = grown
        emb = torch.cat([emb, tab[t].reshape(1, 1, -1)], dim=1).contiguous()
        Lq += 1
    assert got == want
    # the session's recompute engine passes it on as well
    sess = m.mmu_session(ids, attention_mask=dev(g["mask"]))
    assert [int(t) for t in sess.generate(max_new_tokens=steps, top_k=k, temperature=T, top_p=p, _exp_noise=dev(E))] == want


# ---- 10. the full vocabulary once --------------------------------------------------------------------------------------------------------
def test_full_vocabulary_tokens_lie_in_the_reference_nucleus():
    """H 2048, 2 layers, vocabulary 58 498 (the smallest full-width model of the sampled decode tests): 8 tokens with top_p = 0.9 behind
    top_k = 50 (over all 58 498 tokens of a randomly initialised model no single token carries 1e-5 of mass, so no cut could be MARGIN
    clear), graph == eager, and every token inside the reference's kept set of the logits of a teacher-forced forward over the grown
    sequence.  A step whose reference margin is below MARGIN is skipped; at most one may be."""
    d = Wt.ShowoDims(layers=2)
    sd = Wt.make_showo_state(d, seed=11)
    m = util.build_showo(d, sd, max_batch=1, max_seq=128)
    del sd
    Lp, steps, k, p, T = 40, 8, 50, 0.9, 1.0
    ids = torch.randint(0, d.vocab - 20, (1, Lp), generator=torch.Generator().manual_seed(3)).cuda().to(torch.int64).contiguous()
    mask = torch.zeros((1, 1, Lp, Lp), dtype=torch.float32)
    mask.masked_fill_(torch.triu(torch.ones(Lp, Lp, dtype=torch.bool), 1), torch.finfo(torch.float32).min)
    runs = []
    for graph in (1, 0):
        m.decode_graph = graph
        runs.append([int(t) for t in m.mmu_generate(ids, attention_mask=mask.cuda(), max_new_tokens=steps, top_k=k, temperature=T, top_p=p,
                                                    generator=_gen(12))])
    m.decode_graph = 1
    assert runs[0] == runs[1] and len(runs[0]) == steps
    seq = torch.cat([ids, torch.tensor([runs[0][:-1]], dtype=torch.int64, device="cuda")], dim=1)
    Ls = seq.shape[1]
    full = torch.zeros((1, 1, Ls, Ls), dtype=torch.float32)
    full.masked_fill_(torch.triu(torch.ones(Ls, Ls, dtype=torch.bool), 1), torch.finfo(torch.float32).min)
    with torch.no_grad():
        logits = m(seq, attention_mask=full.cuda())[0, Lp - 1:].float().cpu()
    skipped = 0
    for j, t in enumerate(runs[0]):
        keep, _, margin = N.ref_nucleus(logits[j], k, p, T)
        print(f"[nucleus] full vocabulary step {j}: token {t}, kept {int(keep.sum())}, margin {margin:.2e}")
        if margin < N.MARGIN:
            skipped += 1
            continue
        assert bool(keep[t]), (j, t, margin)
    assert skipped <= 1, skipped
