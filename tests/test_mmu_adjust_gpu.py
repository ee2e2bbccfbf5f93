"""GPU tests of the logit adjustment (repetition penalty, logit bias, allowed / banned tokens) on the mmu decode paths: the batch-1
loop (showo_engine_decode_sample_adj), the batched slots (showo_engine_batch_decode_sample_adj: <= 8 slots, wide slots, shared-prefix
slots) and the Python entry points.  The loop is held to a by-hand decode -- showo_engine_decode_step, the numpy adjustment of
tests/logit_adjust_ref.py, the existing stand-alone pick -- token for token; every other path is held to the loop."""
import ctypes as C

import numpy as np
import pytest
import torch

import util
import logit_adjust_ref as R
import logprob_ref as LP
from util import O, dev

pytestmark = pytest.mark.gpu


def _tiny(precision):
    g = util.golden("showo_tiny_mmu.npz")
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd)
    m.set_precision(precision)
    return g, d, m


def _prompts(d, g, n):
    """n mmu prompts of different lengths derived from the golden one (as tests/test_mmu_nucleus_gpu.py builds them)"""
    rs = np.random.RandomState(7)
    base = g["ids"][0].tolist()
    out = []
    for b in range(n):
        extra = rs.randint(5, 200, size=3 * b + (b % 2)).tolist()
        out.append(torch.tensor([base[:len(base) - (b % 4 if b % 2 else 0)] + extra], dtype=torch.int64))
    return out


def _ints(rows):
    return [[int(t) for t in r] for r in rows]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def _pick(L, row, V, k, p, T, noise, seed, step, tok):
    """the existing stand-alone picks: the arg-max for k == 1, else showo_sample_topk_topp (p >= 1: the plain top-k draw)"""
    if k == 1:
        L.call("showo_argmax_f32", L.ptr(row), V, L.ptr(tok), L.stream())
    else:
        L.call("showo_sample_topk_topp", L.ptr(row), V, k, p, T, L.ptr(noise), seed, step, L.ptr(tok), L.stream())


def _prefill(L, eng, ids, mask, lg):
    L.call("showo_engine_prefill", eng, L.ptr(ids), None, L.ptr(mask), ids.shape[1], L.ptr(lg), L.stream())


def _by_hand(L, eng, V, ids, mask, steps, draw, theta, beta, context):
    """1 + steps tokens and their raw logits rows: decode_step, the numpy adjustment on the host, the stand-alone pick on its result"""
    k, p, T, noise, seed = draw
    lg = torch.empty((V,), dtype=torch.float32, device="cuda")
    tok = torch.empty((1,), dtype=torch.int64, device="cuda")
    seen, toks, raws = list(context), [], []
    _prefill(L, eng, ids, mask, lg)
    for j in range(steps + 1):
        if j:
            L.call("showo_engine_decode_step", eng, L.ptr(tok), None, L.ptr(lg), L.stream())
            seen.append(toks[-1])  # the token this step fed joins the set
        raw = lg.cpu().numpy().copy()
        y = torch.from_numpy(R.adjust_ref(raw, seen, theta, beta)).cuda()
        _pick(L, y, V, k, p, T, noise, seed, j, tok)
        toks.append(int(tok.item()))
        raws.append(raw)
    return toks, raws


def _adj_args(seen, pen, bias, ws):
    """(arguments, what must stay alive) of the adjustment part of the _adj entries"""
    n = len(pen)
    a_pen = (C.c_float * n)(*pen)
    a_bias = (C.c_void_p * n)(*[None if b is None else b.data_ptr() for b in bias])
    L = util.lib()
    return (L.ptr(seen), seen.shape[-1], C.cast(a_pen, C.c_void_p), C.cast(a_bias, C.c_void_p), L.ptr(ws)), (a_pen, a_bias)


def _loop_adj(L, eng, V, ids, mask, steps, draw, theta, beta, context, graph, side, want_lp=False):
    """the same tokens from the device: first token by the stand-alone launches, then showo_engine_decode_sample_adj"""
    k, p, T, noise, seed = draw
    lg = torch.empty((V,), dtype=torch.float32, device="cuda")
    tok = torch.empty((1,), dtype=torch.int64, device="cuda")
    seen = _i32(R.bitmap_of(V, context)[None])
    ws = torch.empty((1, V), dtype=torch.float32, device="cuda")
    bd = None if beta is None else dev(beta)
    args, keep = _adj_args(seen, [theta], [bd], ws)
    _prefill(L, eng, ids, mask, lg)
    L.call("showo_logits_adjust", L.ptr(lg), V, 1, V, args[0], args[1], None, args[2], args[3], None, args[4], V, L.stream())
    _pick(L, ws, V, k, p, T, noise, seed, 0, tok)
    first = int(tok.item())
    out = torch.empty((steps,), dtype=torch.int64, device="cuda")
    lps = torch.empty((steps,), dtype=torch.float32, device="cuda") if want_lp else None
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        L.call("showo_engine_decode_sample_adj", eng, L.ptr(tok), steps, L.ptr(out), L.ptr(lg), k, p, T, L.ptr(noise), seed, 1, L.ptr(lps), None,
               *args, graph, L.stream())
    torch.cuda.synchronize()
    del keep
    return [first] + out.tolist(), lps, seen


def _bias_for(V, ban, seed):
    rs = np.random.RandomState(seed)
    b = (0.5 * rs.standard_normal(V)).astype(np.float32)
    b[rs.rand(V) < 0.5] = 0.0
    b[np.array(list(ban), dtype=np.int64)] = -np.inf
    return b


# ---- 1. the loop equals the steps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("graph", [0, 1])
def test_decode_sample_adj_equals_decode_step_plus_the_adjustment_by_hand(precision, graph):
    g, d, m = _tiny(precision)
    L = util.lib()
    eng, V, steps = m.engine(), d.vocab, 10
    ids = dev(g["ids"]).to(torch.int64).contiguous()
    mask = dev(g["mask"]).float().reshape(1, 1, ids.shape[1], ids.shape[1]).contiguous()
    E = dev(np.random.RandomState(2).exponential(size=(1 + steps, V)).astype(np.float32))
    side = torch.cuda.Stream()
    context = g["ids"][0].tolist()
    plain, _ = _by_hand(L, eng, V, ids, mask, steps, (1, 1.0, 1.0, None, 0), 1.0, None, [])
    draws = {"greedy": (1, 1.0, 1.0, None, 0), "topk+noise": (20, 1.0, 0.9, E, 31337), "nucleus": (0, 0.6, 1.0, None, 31337)}
    for name, draw in draws.items():
        for theta, beta in ((1.7, None), (1.3, _bias_for(V, plain[:2], 3)), (1.0, _bias_for(V, plain[:1], 4))):
            hand, raws = _by_hand(L, eng, V, ids, mask, steps, draw, theta, beta, context)
            got, lps, seen = _loop_adj(L, eng, V, ids, mask, steps, draw, theta, beta, context, graph, side, want_lp=True)
            assert got == hand, (name, theta, beta is None)
            # the bitmap afterwards: the context and every token the loop fed (all but the last one it produced)
            assert np.array_equal(seen.cpu().numpy().view(np.uint32)[0], R.bitmap_of(V, context + hand[:-1]))
            # log-probabilities: the log-softmax of the RAW rows
            want = np.array([LP.logprob_ref(raws[j], hand[j])[0] for j in range(1, steps + 1)])
            assert LP.within_gate(lps.cpu().numpy(), want).all(), (name, theta)
            if name == "greedy":
                assert hand != plain  # the adjustment is not a no-op here
                if beta is not None:
                    assert not set(hand) & set(plain[:1])
    # without log-probabilities the tokens are the same
    got, _, _ = _loop_adj(L, eng, V, ids, mask, steps, draws["nucleus"], 1.7, None, context, graph, side)
    assert got == _by_hand(L, eng, V, ids, mask, steps, draws["nucleus"], 1.7, None, context)[0]


# ---- 2. a batched slot gives the tokens of its batch-1 run --------------------------------------------------------------------------------
# per slot: (top_k, top_p, temperature, theta, bias seed or None, context from the prompt?)
SLOTS = [(1, 1.0, 1.0, 1.5, None, True), (5, 1.0, 0.7, 1.0, 5, False), (0, 0.8, 1.3, 1.0, None, False), (1, 1.0, 1.0, 1.2, None, True),
         (1, 1.0, 1.0, 3.0, 6, True)]
REFILL = (20, 0.7, 1.0, 0.5, 7, True)  # what slot 4 serves in the second call


@pytest.mark.parametrize("precision", [0, 2, 3])
@pytest.mark.parametrize("graph", [0, 1])
def test_batch_decode_sample_adj_is_the_tokens_of_the_batch1_adj_runs(precision, graph):
    """two consecutive calls.  Slot 2 is unadjusted (penalty 1, no bias row) and draws from an injected Exp(1) table; slot 3 idles from
    the start; slot 4 is stopped by <eot> in the first call and refilled with another request (a fresh bitmap row) before the second"""
    g, d, m = _tiny(precision)
    L = util.lib()
    eng = m.engine()
    V, n, s1, s2 = d.vocab, len(SLOTS), 5, 6
    steps = s1 + s2
    ids = [t.cuda() for t in _prompts(d, g, n + 1)]
    masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda().float().contiguous() for t in ids]
    side = torch.cuda.Stream()
    noise2 = dev(np.random.RandomState(3).exponential(size=(1 + steps, V)).astype(np.float32))

    def request(b, cfg, prompt):
        k, p, T, theta, bseed, ctx = cfg
        beta = None if bseed is None else _bias_for(V, [11, 12, 13], bseed)
        return (k, p, T, noise2 if b == 2 else None, 7654321 + 1000 * b), theta, beta, (ids[prompt][0].tolist() if ctx else [])

    reqs = [request(b, SLOTS[b], b) for b in range(n)]
    refill = request(4, REFILL, n)
    ref = [_loop_adj(L, eng, V, ids[b], masks[b], steps, *reqs[b], graph, side)[0] for b in range(n)]
    ref_refill = _loop_adj(L, eng, V, ids[n], masks[n], s2, *refill, graph, side)[0]
    # <eot>: a token slot 4 emits in the middle of the first call and not before
    stop = next(j for j in range(2, s1) if ref[4][j] not in ref[4][:j])
    eot = ref[4][stop]
    cut = lambda r: r[:r.index(eot) + 1] if eot in r else r

    L.call("showo_engine_batch_begin", eng, n, max(t.shape[1] for t in ids) + steps + 1)
    lgs = torch.empty((n, V), dtype=torch.float32, device="cuda")
    tok = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    seen = torch.zeros((n, R.words(V)), dtype=torch.int32, device="cuda")
    ws = torch.empty((n, V), dtype=torch.float32, device="cuda")
    pen, bias, draws = [1.0] * n, [None] * n, [None] * n

    def fill(b, req, prompt):
        """request `req` into slot b: prefill, a cleared and re-seeded bitmap row, the first token from the adjusted prefill logits"""
        draw, theta, beta, context = req
        L.call("showo_engine_batch_prefill", eng, b, L.ptr(ids[prompt]), None, L.ptr(masks[prompt]), ids[prompt].shape[1], L.ptr(lgs[b]), L.stream())
        seen[b].zero_()
        if context:
            L.call("showo_seen_mark", L.ptr(seen[b]), V, L.ptr(dev(np.array(context, dtype=np.int64))), len(context), L.stream())
        pen[b], bias[b], draws[b] = theta, None if beta is None else dev(beta), draw
        args, keep = _adj_args(seen[b:b + 1], [theta], [bias[b]], ws[b:b + 1])
        L.call("showo_logits_adjust", L.ptr(lgs[b]), V, 1, V, args[0], args[1], None, args[2], args[3], None, args[4], V, L.stream())
        _pick(L, ws[b], V, draw[0], draw[1], draw[2], draw[3], draw[4], 0, tok[b:b + 1])
        torch.cuda.synchronize()
        return int(tok[b].item())

    got = [[fill(b, reqs[b], b)] for b in range(n) if b != 3]
    got.insert(3, [])
    L.call("showo_engine_batch_prefill", eng, 3, L.ptr(ids[3]), None, L.ptr(masks[3]), ids[3].shape[1], L.ptr(lgs[3]), L.stream())
    arr = lambda t, v: C.cast((t * n)(*v), C.c_void_p)
    alive = [b != 3 and got[b][0] != eot for b in range(n)]

    def call(cnt, d0, budget, want_lp):
        out = torch.empty((n, cnt), dtype=torch.int64, device="cuda")
        lps = torch.empty((n, cnt), dtype=torch.float32, device="cuda") if want_lp else None
        prod = (C.c_int * n)()
        args, keep = _adj_args(seen, pen, bias, ws)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            L.call("showo_engine_batch_decode_sample_adj", eng, L.ptr(tok), cnt, L.ptr(out), L.ptr(lgs), arr(C.c_int, [q[0][0] for q in reqs]),
                   arr(C.c_float, [dr[1] if dr else 1.0 for dr in draws]), arr(C.c_float, [dr[2] if dr else 1.0 for dr in draws]),
                   arr(C.c_uint64, [dr[4] if dr else 0 for dr in draws]), arr(C.c_int, d0),
                   arr(C.c_void_p, [L.ptr(dr[3]) if dr else None for dr in draws]), arr(C.c_int, budget), eot, C.cast(prod, C.c_void_p),
                   L.ptr(lps), None, *args, graph, L.stream())
        torch.cuda.synchronize()
        del keep
        return out.tolist(), list(prod), lps

    budget = [s1 if alive[b] else 0 for b in range(n)]
    rows, prod, lps = call(s1, [1] * n, budget, True)
    for b in range(n):
        got[b] += rows[b][:prod[b]]
        assert rows[b][prod[b]:] == [-1] * (s1 - prod[b])
        if got[b] and got[b][-1] == eot:
            alive[b] = False
    assert prod[3] == 0 and prod[4] == stop and got[4][-1] == eot  # idle from the start; stopped by <eot> mid-call
    assert not seen[3].any() and int(tok[3]) == -7  # the idle slot was neither marked nor given a token
    assert torch.isfinite(lps[0, :prod[0]]).all() and (lps[3] == 0).all()
    for b in (0, 1, 2):
        assert got[b] == cut(ref[b])[:len(got[b])], (b, SLOTS[b])
    assert got[4] == ref[4][:stop + 1]
    # slot 4 takes another request: its draws come from another top_k, so the slot's settings change with it
    first_call = [list(t) for t in got]
    got[4] = [fill(4, refill, n)]
    reqs[4] = refill
    alive[4] = got[4][0] != eot
    budget = [s2 if alive[b] else 0 for b in range(n)]
    rows, prod, _ = call(s2, [1 + s1, 1 + s1, 1 + s1, 0, 1], budget, False)
    for b in range(n):
        got[b] += rows[b][:prod[b]]
    for b in (0, 1, 2):
        assert got[b] == cut(ref[b]), (b, SLOTS[b])
    assert got[4] == cut(ref_refill) and first_call[4] == ref[4][:stop + 1]
    assert len(got[0]) > s1 + 1 or eot in got[0]
    assert not seen[3].any()
    # slot 0's bitmap row: its context and every token it fed
    fed = got[0][:-1]
    assert np.array_equal(seen[0].cpu().numpy().view(np.uint32), R.bitmap_of(V, reqs[0][3] + fed))


# ---- 3. wide and shared-prefix slots ---------------------------------------------------------------------------------------------------------
def _per_request_kw(n):
    ths, bans, ctxs = [1.4, None, 1.0, 0.7], [None, [21, 22], [30], None], [[5, 6, 7], None, None, [40, 41]]
    return dict(repetition_penalty=[ths[b % 4] for b in range(n)], banned_tokens=[bans[b % 4] for b in range(n)],
                repetition_context=[ctxs[b % 4] for b in range(n)], top_k=[1] * n)


def _pick_kw(kw, order):
    return {k: ([v[r] for r in order] if isinstance(v, list) else v) for k, v in kw.items()}


def test_wide_slots_give_tokens_independent_of_slots_order_and_neighbours():
    g, d, m = _tiny(0)
    n, new = 12, 10
    ids = [t.cuda() for t in _prompts(d, g, n)]
    masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda() for t in ids]
    kw = _per_request_kw(n)
    kw.update(top_k=[1, 5, None, 20] * 3, temperature=[1.0, 0.7, 1.1, 1.0] * 3)
    noise = [torch.empty((new, d.vocab), device="cuda").exponential_(1.0, generator=_gen(5 + b)) for b in range(n)]

    def run(S, order, graph=1):
        m.decode_graph = graph
        out = m.mmu_generate_batch(idx=[ids[r] for r in order], attention_mask=[masks[r] for r in order], max_new_tokens=new, slots=S,
                                   _exp_noise=[noise[r] for r in order], **_pick_kw(kw, order))
        m.decode_graph = 1
        return dict(zip(order, _ints(out)))

    ref = run(9, list(range(n)))
    order2 = [7, 0, 11, 3, 9, 1, 5, 10, 2, 8, 4, 6]
    assert run(32, list(range(n))) == ref and run(9, order2, graph=0) == ref and run(16, order2) == ref
    some = run(9, order2[:10])  # other neighbours
    assert all(some[r] == ref[r] for r in some)
    assert all(not set(ref[b]) & {21, 22} for b in range(1, n, 4)) and all(30 not in ref[b] for b in range(2, n, 4))
    plain = m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=new, slots=9, _exp_noise=noise, top_k=kw["top_k"],
                                 temperature=kw["temperature"])
    assert _ints(plain) != [ref[b] for b in range(n)]  # the adjustment is not a no-op here


def test_shared_prefix_slots_give_tokens_independent_of_slots_order_and_neighbours():
    g, d, m = _tiny(0)
    n, new, P = 12, 10, 20
    full = torch.from_numpy(g["ids"]).to(torch.int64)
    sess = m.mmu_session(dev(full[:, :P]), attention_mask=dev(O.mask_mmu(full[:, :P], d.eoi_id)))
    rs = np.random.RandomState(3)
    qs = [dev(torch.cat([full[:, P:P + 1 + b % 5], torch.from_numpy(rs.randint(5, 200, size=(1, b))).to(torch.int64)], dim=1)) for b in range(n)]
    kw = _per_request_kw(n)
    kw["top_k"] = 1

    def run(S, order, share=True):
        out = sess.generate_batch(idx=[qs[r] for r in order], max_new_tokens=new, slots=S, share_prefix=share, **_pick_kw(kw, order))
        return dict(zip(order, _ints(out)))

    ref = run(9, list(range(n)))
    order2 = [7, 0, 11, 3, 9, 1, 5, 10, 2, 8, 4, 6]
    assert run(32, list(range(n))) == ref and run(16, order2) == ref
    some = run(9, order2[:10])
    assert all(some[r] == ref[r] for r in some)
    assert sess.length == P
    assert all(not set(ref[b]) & {21, 22} for b in range(1, n, 4))


# ---- 4. the public API ---------------------------------------------------------------------------------------------------------------------
def test_banned_allowed_and_penalty_through_mmu_generate():
    g, d, m = _tiny(0)
    L = util.lib()
    eng, V, new = m.engine(), d.vocab, 12
    ids = dev(g["ids"]).to(torch.int64).contiguous()
    mask = dev(g["mask"])
    kw = dict(attention_mask=mask, max_new_tokens=new, top_k=1)
    plain = [int(t) for t in m.mmu_generate(ids, **kw)]
    assert [int(t) for t in m.mmu_generate(ids, repetition_penalty=1.0, **kw)] == plain  # penalty 1, no bias: the call without
    lg = torch.empty((V,), dtype=torch.float32, device="cuda")
    _prefill(L, eng, ids, mask.float().reshape(1, 1, ids.shape[1], ids.shape[1]).contiguous(), lg)
    top2 = torch.topk(lg, 2).indices.tolist()
    assert top2[0] == plain[0]
    for graph in (0, 1):
        m.decode_graph = graph
        # banned: the plain call's first token never appears, and the first token is the row's runner-up
        got = [int(t) for t in m.mmu_generate(ids, banned_tokens=[plain[0]], **kw)]
        assert plain[0] not in got and got[0] == top2[1] and len(got) == new
        # allowed: every token lies in the set (<eot> is not in it: the call runs to its budget)
        allowed = [17, 99, 250, plain[0], 301]
        got = [int(t) for t in m.mmu_generate(ids, allowed_tokens=allowed, eot_token=5, **kw)]
        assert set(got) <= set(allowed) and len(got) == new
        got_lp = m.mmu_generate(ids, allowed_tokens=allowed, eot_token=5, return_logprobs=True, **kw)
        assert [int(t) for t in got_lp[0]] == got and torch.isfinite(got_lp[1]).all() and float(got_lp[1].max()) <= 0.0
        # the penalty with Hugging Face's set (the prompt's ids) equals the by-hand reference, greedy and sampled
        E = np.random.RandomState(2).exponential(size=(new, V)).astype(np.float32)
        for k, T, noise in ((1, 1.0, None), (5, 0.7, E)):
            hand, _ = _by_hand(L, eng, V, ids, mask.float().reshape(1, 1, ids.shape[1], ids.shape[1]).contiguous(), new - 1,
                               (k, 1.0, T, None if noise is None else dev(noise), 0), 1.6, _bias_for(V, [], 9), g["ids"][0].tolist())
            call = lambda: [int(t) for t in m.mmu_generate(ids, attention_mask=mask, max_new_tokens=new, top_k=k, temperature=T,
                                                           _exp_noise=None if noise is None else dev(noise), repetition_penalty=1.6,
                                                           repetition_context=ids[0], logit_bias=torch.from_numpy(_bias_for(V, [], 9)))]
            got = call()
            assert got == hand, (graph, k)
            assert call() == got  # nothing persists: a second identical call gives identical tokens
        assert hand != plain
    m.decode_graph = 1


def test_session_generate_equals_mmu_generate_and_generate_batch_equals_generate_plus_rewind():
    g, d, m = _tiny(0)
    ids = torch.from_numpy(g["ids"]).to(torch.int64)
    pm = O.mask_mmu(ids[:, :20], d.eoi_id)
    adj = dict(repetition_penalty=1.5, repetition_context=ids[0], banned_tokens=[33, 34], logit_bias={50: 0.75})
    for kw in (dict(top_k=1), dict(top_k=5, temperature=0.7, _exp_noise=dev(g["exp_noise_topk5"]))):
        want = [int(t) for t in m.mmu_generate(dev(ids), attention_mask=dev(g["mask"]), max_new_tokens=8, **kw, **adj)]
        sess = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(pm))
        assert [int(t) for t in sess.generate(dev(ids[:, 20:]), max_new_tokens=8, **kw, **adj)] == want
    # generate_batch: per-request keywords, 3 requests on <= 8 slots and 11 with a refill, against generate + rewind
    sess = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(pm))
    sess.generate(dev(ids[:, 20:]), max_new_tokens=3, top_k=1)
    state = sess.mark()
    rs = np.random.RandomState(5)
    for n in (3, 11):
        qs = [dev(torch.tensor([rs.randint(5, 200, size=1 + (3 * b + b % 2) % 9).tolist()], dtype=torch.int64)) for b in range(n)]
        kw = _per_request_kw(n)
        kw.update(top_k=[[1, 5, None, 20][b % 4] for b in range(n)], temperature=[[1.0, 0.7, 1.3, 1.0][b % 4] for b in range(n)])
        gen, want = _gen(5), []
        for b, q in enumerate(qs):
            mark = sess.mark()
            want.append([int(t) for t in sess.generate(q, max_new_tokens=12, generator=gen, **{k: v[b] for k, v in kw.items()})])
            sess.rewind(mark)
        n0, K0, V0 = _cache_bits(m, sess.length)
        for graph in (0, 1):
            m.decode_graph = graph
            got, lps = sess.generate_batch(idx=qs, max_new_tokens=12, generator=_gen(5), return_logprobs=True, **kw)
            assert _ints(got) == want, (n, graph)
            assert all(torch.isfinite(l).all() for l in lps)
            assert sess.mark() == state
        n1, K1, V1 = _cache_bits(m, sess.length)
        assert n1 == n0 and torch.equal(K1, K0) and torch.equal(V1, V0)
    m.decode_graph = 1


def _cache_bits(m, P):
    """bits of the engine's decode cache below row P: K rows [0, P) and V^T columns [0, P) of every layer"""
    L = util.lib()
    eng = m.engine()
    k, vt, ks, vs = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int64()
    n, pl, cap, ep = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    L.call("showo_engine_cache_ptrs", eng, C.byref(k), C.byref(vt), C.byref(ks), C.byref(vs))
    L.call("showo_engine_cache_state", eng, C.byref(n), C.byref(pl), C.byref(cap), C.byref(ep))
    d = util.tiny_dims()
    nL, nH, cp = d.layers, d.heads, cap.value

    def snap(ptr, nelems):
        out = torch.empty((nelems,), dtype=torch.int16, device="cuda")
        L.call("showo_copy_b128", ptr, L.ptr(out), nelems * 2, L.stream())
        torch.cuda.synchronize()
        return out.cpu()

    K = snap(k.value, nL * nH * cp * 64).reshape(nL, nH, cp, 64)[:, :, :P].clone()
    Vt = snap(vt.value, nL * nH * 64 * cp).reshape(nL, nH, 64, cp)[:, :, :, :P].clone()
    return n.value, K, Vt


def test_precision_1_recompute_path_takes_the_adjustment():
    """accuracy mode at the tiny shape runs the reference's no-cache algorithm (_mmu_generate_recompute): greedy tokens are what a host
    loop picks from the numpy adjustment of the same engine logits (showo_engine_forward_rows on the grown sequence and mask)"""
    g, d, m = _tiny(1)
    L = util.lib()
    eng, V, steps = m.engine(), d.vocab, 8
    ids = dev(g["ids"]).to(torch.int64)
    theta, beta, context = 1.6, _bias_for(V, [60, 61], 2), g["ids"][0].tolist()
    kw = dict(attention_mask=dev(g["mask"]), max_new_tokens=steps, top_k=1, repetition_penalty=theta, repetition_context=context,
              logit_bias=torch.from_numpy(beta))
    got = [int(t) for t in m.mmu_generate(ids, **kw)]
    tab = m.showo.model.embed_tokens.weight.detach().float()
    emb = tab[ids].contiguous()
    Lq = emb.shape[1]
    mask = dev(g["mask"]).float().reshape(1, 1, Lq, Lq).contiguous()
    neg = float(torch.finfo(torch.float32).min)
    row = torch.empty((1,), dtype=torch.int32, device="cuda")
    lg = torch.empty((V,), dtype=torch.float32, device="cuda")
    want, seen = [], list(context)
    for step in range(steps):
        row.fill_(Lq - 1)
        L.call("showo_engine_forward_rows", eng, None, L.ptr(emb), L.ptr(mask), 1, Lq, L.ptr(row), 1, 0, V, L.ptr(lg), L.stream())
        y = R.adjust_ref(lg.cpu().numpy(), seen, theta, beta)
        t = int(np.argmax(y))
        want.append(t)
        seen.append(t)
        grown = torch.full((1, 1, Lq + 1, Lq + 1), neg, dtype=torch.float32, device="cuda")
        grown[0, 0, :Lq, :Lq] = mask[0, 0]
        grown[0, 0, Lq, :Lq] = mask[0, 0, Lq - 1]
        grown[0, 0, Lq, Lq] = 0.0
        mask = grown
        emb = torch.cat([emb, tab[t].reshape(1, 1, -1)], dim=1).contiguous()
        Lq += 1
    assert got == want
    plain = [int(t) for t in m.mmu_generate(ids, attention_mask=dev(g["mask"]), max_new_tokens=steps, top_k=1)]
    assert got != plain
    sess = m.mmu_session(ids, attention_mask=dev(g["mask"]))
    kw.pop("attention_mask")
    assert [int(t) for t in sess.generate(**kw)] == want


# ---- 5. the full vocabulary once -------------------------------------------------------------------------------------------------------
def test_full_vocabulary_greedy_with_a_penalty_and_a_ban():
    """H 2048, 2 layers, vocabulary 58 498 (the smallest full-width model of the sampled decode tests): here the plain greedy loop runs
    the fused token seam, which an adjusted call leaves.  Graph == eager == the by-hand decode (decode_step, numpy adjustment,
    stand-alone arg-max); the banned token never appears and the first token is the prefill row's runner-up."""
    from util import Wt
    d = Wt.ShowoDims(layers=2)
    sd = Wt.make_showo_state(d, seed=11)
    m = util.build_showo(d, sd, max_batch=1, max_seq=128)
    del sd
    L = util.lib()
    eng, V = m.engine(), d.vocab
    Lp, steps, theta = 40, 8, 1.5
    ids = torch.randint(0, V - 20, (1, Lp), generator=torch.Generator().manual_seed(3)).cuda().to(torch.int64).contiguous()
    mask = torch.zeros((1, 1, Lp, Lp), dtype=torch.float32)
    mask.masked_fill_(torch.triu(torch.ones(Lp, Lp, dtype=torch.bool), 1), torch.finfo(torch.float32).min)
    mask = mask.cuda().contiguous()
    kw = dict(attention_mask=mask, max_new_tokens=steps, top_k=1)
    plain = [int(t) for t in m.mmu_generate(ids, **kw)]
    lg = torch.empty((V,), dtype=torch.float32, device="cuda")
    _prefill(L, eng, ids, mask, lg)
    top2 = torch.topk(lg, 2).indices.tolist()
    assert top2[0] == plain[0]
    beta = np.zeros(V, dtype=np.float32)
    beta[plain[0]] = -np.inf
    hand, _ = _by_hand(L, eng, V, ids, mask, steps - 1, (1, 1.0, 1.0, None, 0), theta, beta, ids[0].tolist())
    for graph in (1, 0):
        m.decode_graph = graph
        got = [int(t) for t in m.mmu_generate(ids, banned_tokens=[plain[0]], repetition_penalty=theta, repetition_context=ids[0], **kw)]
        assert got == hand, graph
    m.decode_graph = 1
    assert plain[0] not in hand and len(hand) == steps and hand != plain
    banned = [int(t) for t in m.mmu_generate(ids, banned_tokens=[plain[0]], **kw)]
    assert plain[0] not in banned and banned[0] == top2[1]
