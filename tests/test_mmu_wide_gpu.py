"""GPU tests of wide decode batches on the tiny model: showo_engine_batch_begin_wide (9..32 slots on the MFMA kernels of
csrc/decode_wide.hip) behind Showo.mmu_generate_batch(..., slots=S) and MmuSession.generate_batch(..., slots=S).

The contract of a wide call is NOT "the bits of the batch-1 run" (an MFMA's summation order is the hardware's): it is (1) determinism,
(2) independence of a request's tokens and log-probabilities from S, n, its slot and its neighbours, and (3) the bf16 arithmetic class
of the existing step, held against the fp32 oracle next to the batch-1 step's own figures."""
import numpy as np
import pytest
import torch

import util
from util import O, dev

pytestmark = pytest.mark.gpu

NEW = 40


def _prompts(d, g, n):
    """n mmu prompts of different lengths derived from the golden one (as tests/test_decode_batch_gpu.py builds them)"""
    rs = np.random.RandomState(7)
    base = g["ids"][0].tolist()
    out = []
    for b in range(n):
        extra = rs.randint(5, 200, size=3 * b + (b % 2)).tolist()
        row = base[:len(base) - (b % 4 if b % 2 else 0)] + extra
        out.append(torch.tensor([row], dtype=torch.int64))
    return out


def _tiny(precision=0):
    g = util.golden("showo_tiny_mmu.npz")
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd, max_batch=8, max_seq=128)
    m.set_precision(precision)
    return g, d, sd, m


def _ints(rows):
    return [[int(t) for t in r] for r in rows]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _noise(n, V, seed):
    """per-request Exp(1) tables: a request's draws follow the request, wherever it stands in the list"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.empty((NEW, V), device="cuda").exponential_(1.0, generator=g) for _ in range(n)]


# ---- 5. slot and neighbour independence -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["greedy", "topk5", "topp0.9"])
def test_wide_results_do_not_depend_on_slots_order_or_replay(mode):
    g, d, sd, m = _tiny()
    n = 12
    ids = [t.cuda() for t in _prompts(d, g, n)]
    masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda() for t in ids]
    kw = {"greedy": dict(top_k=1), "topk5": dict(top_k=5, temperature=0.7), "topp0.9": dict(top_k=None, top_p=0.9, temperature=0.9)}[mode]
    noise = None if mode == "greedy" else _noise(n, d.vocab, 5)
    order2 = [7, 0, 11, 3, 9, 1, 5, 10, 2, 8, 4, 6]

    def run(S, order, graph):
        m.decode_graph = graph
        toks, lps = m.mmu_generate_batch(idx=[ids[r] for r in order], attention_mask=[masks[r] for r in order], max_new_tokens=NEW,
                                         _exp_noise=None if noise is None else [noise[r] for r in order], return_logprobs=True, slots=S, **kw)
        back = {r: i for i, r in enumerate(order)}
        return _ints([toks[back[r]] for r in range(n)]), [lps[back[r]].clone() for r in range(n)]

    ref_t, ref_l = run(16, list(range(n)), 1)
    assert all(len(t) == NEW for t in ref_t) and all(torch.isfinite(l).all() for l in ref_l)
    for S in (9, 16, 32):
        for order in (list(range(n)), order2):
            for graph in (0, 1):
                t, l = run(S, order, graph)
                assert t == ref_t, (mode, S, order, graph)
                for r in range(n):
                    assert torch.equal(l[r], ref_l[r]), (mode, S, order, graph, r)
    if mode != "greedy":  # seeds drawn from a generator: two identical calls, and another slot count
        m.decode_graph = 1
        a = m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=NEW, generator=_gen(3), return_logprobs=True, slots=16, **kw)
        b = m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=NEW, generator=_gen(3), return_logprobs=True, slots=16, **kw)
        c = m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=NEW, generator=_gen(3), return_logprobs=True, slots=9, **kw)
        assert _ints(a[0]) == _ints(b[0]) == _ints(c[0])
        assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a[1], b[1], c[1]))


# ---- 6. against the oracle, teacher-forced --------------------------------------------------------------------------------------
def test_wide_step_logits_vs_oracle_next_to_the_batch1_step():
    """Request 0 (the fixture's prompt) in slot 11 of a 12-slot wide batch, other prompts around it, 40 teacher-forced steps: the
    logits of every step against the fp32 oracle, and the batch-1 showo_engine_decode_step's figures measured the same way.  Both
    paths round the same tensors to bf16 and differ only in fp32 summation order: the wide figures may exceed the batch-1 ones by 10 %.

    Measured on an MI355X (rel_max / rel_rms over the 40 steps' logits): see the [parity] line; DESIGN.md "Wide decode batches"."""
    g, d, sd, m = _tiny()
    sdt = O.to_torch(sd)
    ids_c = torch.from_numpy(g["ids"]).to(torch.int64)
    toks_ref = [int(t) for t in O.mmu_generate(sdt, d, ids_c, attention_mask=torch.from_numpy(g["mask"]), max_new_tokens=NEW, top_k=1)]
    seq = torch.cat([ids_c, torch.tensor([toks_ref[:-1]], dtype=torch.int64)], dim=1)
    ref = O.showo_logits(sdt, d, seq, attention_mask=O.mask_mmu(seq, d.eoi_id))[0, ids_c.shape[1] - 1:]
    assert [int(r.argmax()) for r in ref] == toks_ref
    L = util.lib()
    eng = m.engine()
    V = d.vocab
    # batch-1 step of the parent
    ids = dev(g["ids"]).to(torch.int64).contiguous()
    mask = dev(g["mask"]).float().reshape(1, 1, ids.shape[1], ids.shape[1]).contiguous()
    logits = torch.empty((V,), dtype=torch.float32, device="cuda")
    L.call("showo_engine_prefill", eng, L.ptr(ids), None, L.ptr(mask), ids.shape[1], L.ptr(logits), L.stream())
    one = []
    for j, t in enumerate(toks_ref):
        torch.cuda.synchronize()
        one.append(logits.cpu().clone())
        if j + 1 < NEW:
            tok = torch.tensor([t], dtype=torch.int64, device="cuda")
            L.call("showo_engine_decode_step", eng, L.ptr(tok), None, L.ptr(logits), L.stream())
    # wide batch: request 0 in slot 11, prompts 1..11 in slots 0..10
    S, slot = 12, 11
    others = [t.cuda() for t in _prompts(d, g, S)][1:]
    prompts = others + [ids]
    cap = max(t.shape[1] for t in prompts) + NEW + 1
    L.call("showo_engine_batch_begin_wide", eng, S, cap)
    lgs = torch.empty((S, V), dtype=torch.float32, device="cuda")
    for b, p in enumerate(prompts):
        mk = O.mask_mmu(p.cpu(), d.eoi_id).cuda().float().reshape(1, 1, p.shape[1], p.shape[1]).contiguous()
        L.call("showo_engine_batch_prefill", eng, b, L.ptr(p.contiguous()), None, L.ptr(mk), p.shape[1], L.ptr(lgs[b]), L.stream())
    tok = lgs.argmax(dim=1).to(torch.int64).contiguous()
    out = torch.empty((S, 1), dtype=torch.int64, device="cuda")
    wide = []
    for j, t in enumerate(toks_ref):
        torch.cuda.synchronize()
        wide.append(lgs[slot].cpu().clone())
        if j + 1 < NEW:
            tok[slot] = t  # teacher-forced; the other slots feed their own arg-max
            L.call("showo_engine_batch_decode_greedy", eng, L.ptr(tok), 1, L.ptr(out), L.ptr(lgs), 0, L.stream())
    one, wide = torch.stack(one), torch.stack(wide)
    assert torch.isfinite(wide).all()
    max1, rms1 = util.relerr(one, ref)
    maxw, rmsw = util.relerr(wide, ref)
    print(f"[parity] tiny teacher-forced decode vs oracle, {NEW} steps: wide (slot 11 of 12) rel_max={maxw:.3e} rel_rms={rmsw:.3e}; "
          f"batch-1 step rel_max={max1:.3e} rel_rms={rms1:.3e}; ratio {maxw / max1:.3f} / {rmsw / rms1:.3f}")
    assert maxw <= 1.10 * max1 and rmsw <= 1.10 * rms1, (maxw, max1, rmsw, rms1)
    # greedy tokens: wherever the oracle's top-2 gap exceeds twice that step's max logit error, the wide arg-max is the oracle's
    top2 = ref.topk(2, dim=1).values
    gaps = (top2[:, 0] - top2[:, 1]).tolist()
    errs = (wide - ref).abs().max(dim=1).values.tolist()
    decided = 0
    for j in range(NEW):
        if gaps[j] > 2.0 * errs[j]:
            decided += 1
            assert int(wide[j].argmax()) == toks_ref[j], (j, gaps[j], errs[j])
    print(f"[parity] tiny wide greedy tokens vs oracle: steps decided by the gap rule {decided}/{NEW}")
    assert decided * 4 >= NEW * 3, decided


# ---- 7. scheduler ---------------------------------------------------------------------------------------------------------------
def test_wide_scheduler_refills_slots_and_stops_each_request_at_its_eot(monkeypatch):
    g, d, sd, m = _tiny()
    n, S, new = 20, 9, 30
    ids = [t.cuda() for t in _prompts(d, g, n)]
    masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda() for t in ids]
    free = _ints(m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=new, top_k=1, slots=S))
    assert [len(r) for r in free] == [new] * n
    eot = free[2][4]
    want = [r[:r.index(eot) + 1] if eot in r else r for r in free]  # (neighbour independence: the same tokens, cut at the first <eot>)
    assert any(len(r) < new for r in want) and any(len(r) == new for r in want)
    L = util.lib()
    calls = {"prefill": 0, "wide": 0, "narrow": 0}
    real = L.call

    def counting(name, *a):
        if name == "showo_engine_batch_prefill":
            calls["prefill"] += 1
        elif name == "showo_engine_batch_begin_wide":
            calls["wide"] += 1
        elif name == "showo_engine_batch_begin":
            calls["narrow"] += 1
        return real(name, *a)

    monkeypatch.setattr(L, "call", counting)

    def refuse(*a, **k):
        raise AssertionError("mmu_generate_batch fell back to sequential mmu_generate calls")

    monkeypatch.setattr(util.pkg().Showo, "mmu_generate", refuse)
    got = _ints(m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=new, top_k=1, eot_token=eot, slots=S))
    assert got == want
    assert calls == {"prefill": n, "wide": 1, "narrow": 0}  # 20 prefills on 9 slots: 11 of them are refills


# ---- 8. session -----------------------------------------------------------------------------------------------------------------
def test_session_generate_batch_on_wide_slots_leaves_the_session_unchanged():
    g, d, sd, m = _tiny()
    ids = torch.from_numpy(g["ids"]).to(torch.int64)
    sess = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(O.mask_mmu(ids[:, :20], d.eoi_id)))
    mark = sess.mark()
    before = [int(t) for t in sess.generate(dev(ids[:, 20:]), max_new_tokens=12, top_k=1)]
    sess.rewind(mark)
    rs = np.random.RandomState(3)
    qs = [dev(torch.cat([ids[:, 20:20 + 1 + b % 5], torch.from_numpy(rs.randint(5, 200, size=(1, b))).to(torch.int64)], dim=1)) for b in range(12)]
    kw = dict(max_new_tokens=20, top_k=[1, 5, None] * 4, temperature=[1.0, 0.7, 1.1] * 4, top_p=[None, None, 0.9] * 4, return_logprobs=True)
    t16, l16 = sess.generate_batch(idx=qs, generator=_gen(9), slots=16, **kw)
    assert sess.length == 20
    t32, l32 = sess.generate_batch(idx=qs, generator=_gen(9), slots=32, **kw)
    assert _ints(t16) == _ints(t32) and all(torch.equal(a, b) for a, b in zip(l16, l32))
    assert all(len(t) == 20 for t in t16)
    after = [int(t) for t in sess.generate(dev(ids[:, 20:]), max_new_tokens=12, top_k=1)]
    assert after == before


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------
def test_wide_refusals_and_the_narrow_call_for_few_requests():
    g, d, sd, m = _tiny()
    n = 10
    ids = [t.cuda() for t in _prompts(d, g, n)]
    masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda() for t in ids]
    for bad in (8, 33, 0, 16.0, True):
        with pytest.raises(ValueError):
            m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=4, top_k=1, slots=bad)
    # n = 4: the call without `slots`, bit for bit
    kw = dict(max_new_tokens=12, top_k=5, temperature=0.7, return_logprobs=True)
    a = m.mmu_generate_batch(idx=ids[:4], attention_mask=masks[:4], generator=_gen(2), **kw)
    b = m.mmu_generate_batch(idx=ids[:4], attention_mask=masks[:4], generator=_gen(2), slots=16, **kw)
    assert _ints(a[0]) == _ints(b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    L = util.lib()
    eng = m.engine()
    with pytest.raises(RuntimeError):
        L.call("showo_engine_batch_begin_wide", eng, 33, 64)
    with pytest.raises(RuntimeError):
        L.call("showo_engine_batch_begin_wide", eng, 0, 64)
    # a wide batch prefilled at precision 0, then the engine switched to precision 2: the decode refuses
    S = 9
    L.call("showo_engine_batch_begin_wide", eng, S, max(t.shape[1] for t in ids) + 8)
    lgs = torch.empty((S, d.vocab), dtype=torch.float32, device="cuda")
    for s in range(S):
        mk = masks[s].float().reshape(1, 1, ids[s].shape[1], ids[s].shape[1]).contiguous()
        L.call("showo_engine_batch_prefill", eng, s, L.ptr(ids[s].contiguous()), None, L.ptr(mk), ids[s].shape[1], L.ptr(lgs[s]), L.stream())
    tok = lgs.argmax(dim=1).to(torch.int64).contiguous()
    out = torch.empty((S, 2), dtype=torch.int64, device="cuda")
    L.call("showo_engine_batch_decode_greedy", eng, L.ptr(tok), 2, L.ptr(out), L.ptr(lgs), 0, L.stream())
    torch.cuda.synchronize()
    for precision in (2, 3):
        m.set_precision(precision)
        with pytest.raises(ValueError):
            m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=4, top_k=1, slots=16)
    m.set_precision(2)
    eng = m.engine()
    with pytest.raises(RuntimeError):
        L.call("showo_engine_batch_decode_greedy", eng, L.ptr(tok), 2, L.ptr(out), L.ptr(lgs), 0, L.stream())
    with pytest.raises(RuntimeError):
        L.call("showo_engine_batch_begin_wide", eng, 9, 64)
    m.set_precision(0)
