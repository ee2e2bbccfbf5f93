"""GPU tests of shared-prefix slots on the tiny model: MmuSession.generate_batch(..., slots=S, share_prefix=True) on
showo_engine_batch_begin_shared / _batch_attach_append (csrc/decode_batch.hip) and the two attention launches of csrc/attn_shared.hip.

Every test runs at a prefix of 20 rows (base 0: the suffix caches start with 20 dead rows) and of 70 rows (base 64, two prefix splits).
The contract: deterministic; a request's tokens and log-probabilities independent of S, n, slot, order and neighbours; first logits
bit-equal to `generate`'s; later steps in the bf16 class of the forked wide path, held against the fp32 oracle next to that path's own
figures; the session unchanged afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

import util
from util import O, dev

pytestmark = pytest.mark.gpu

NEW = 24
PREFIXES = (20, 70)


def _tiny():
    g = util.golden("showo_tiny_mmu.npz")
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd, max_batch=8, max_seq=128)
    m.set_precision(0)
    return g, d, sd, m


def _full_prompt(g, P):
    """the golden mmu prompt, extended with text tokens to P + 5 rows: rows [0, P) are the session's prefix, the last 5 a question"""
    ids = torch.from_numpy(g["ids"]).to(torch.int64)
    extra = P + 5 - ids.shape[1]
    if extra > 0:
        rs = np.random.RandomState(P)
        ids = torch.cat([ids[:, :20], torch.from_numpy(rs.randint(5, 200, size=(1, extra))).to(torch.int64), ids[:, 20:]], dim=1)
    return ids


def _session(m, d, full, P):
    pre = full[:, :P]
    return m.mmu_session(dev(pre), attention_mask=dev(O.mask_mmu(pre, d.eoi_id)))


def _questions(full, P, n):
    """n questions of different lengths (1 .. 5 + n rows); question 0 is the prompt's own"""
    rs = np.random.RandomState(3)
    qs = [full[:, P:]]
    for b in range(1, n):
        qs.append(torch.cat([full[:, P:P + 1 + b % 5], torch.from_numpy(rs.randint(5, 200, size=(1, b))).to(torch.int64)], dim=1))
    return [dev(q) for q in qs]


def _ints(rows):
    return [[int(t) for t in r] for r in rows]


def _noise(n, V, seed, rows=NEW):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.empty((rows, V), device="cuda").exponential_(1.0, generator=g) for _ in range(n)]


def _cache_snapshot(m, P):
    """bits of the engine's decode cache that a session owns: K rows [0, P) and V^T columns [0, 64 ceil(P / 64)) of every layer"""
    L = util.lib()
    eng = m.engine()
    k, vt, ks, vs = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int64()
    n, pl, cap, ep = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    L.call("showo_engine_cache_ptrs", eng, C.byref(k), C.byref(vt), C.byref(ks), C.byref(vs))
    L.call("showo_engine_cache_state", eng, C.byref(n), C.byref(pl), C.byref(cap), C.byref(ep))
    d = util.tiny_dims()
    nL, nH, cp = d.layers, d.heads, cap.value
    assert ks.value == nH * cp * 64 and vs.value == nH * 64 * cp  # the layers lie back to back

    def snap(ptr, nelems):
        out = torch.empty((nelems,), dtype=torch.int16, device="cuda")
        L.call("showo_copy_b128", ptr, L.ptr(out), nelems * 2, L.stream())
        torch.cuda.synchronize()
        return out.cpu()

    K = snap(k.value, nL * nH * cp * 64).reshape(nL, nH, cp, 64)[:, :, :P].clone()
    V = snap(vt.value, nL * nH * 64 * cp).reshape(nL, nH, 64, cp)[:, :, :, :(P + 63) // 64 * 64].clone()
    return n.value, ep.value, K, V


# ---- independence of slots, order and replay ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["greedy", "topk5", "topp0.9"])
@pytest.mark.parametrize("P", PREFIXES)
def test_shared_results_do_not_depend_on_slots_order_or_replay(P, mode):
    g, d, sd, m = _tiny()
    full = _full_prompt(g, P)
    sess = _session(m, d, full, P)
    n = 12
    qs = _questions(full, P, n)
    kw = {"greedy": dict(top_k=1), "topk5": dict(top_k=5, temperature=0.7), "topp0.9": dict(top_k=None, top_p=0.9, temperature=0.9)}[mode]
    noise = None if mode == "greedy" else _noise(n, d.vocab, 5)
    order2 = [7, 0, 11, 3, 9, 1, 5, 10, 2, 8, 4, 6]

    def run(S, order, graph):
        m.decode_graph = graph
        toks, lps = sess.generate_batch(idx=[qs[r] for r in order], max_new_tokens=NEW, return_logprobs=True, slots=S, share_prefix=True,
                                        _exp_noise=None if noise is None else [noise[r] for r in order], **kw)
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
    assert sess.length == P


# ---- first logits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PREFIXES)
def test_first_logits_of_every_request_are_those_of_generate(P):
    g, d, sd, m = _tiny()
    full = _full_prompt(g, P)
    sess = _session(m, d, full, P)
    qs = _questions(full, P, 12)
    L = util.lib()
    eng = m.engine()
    be = sess._be
    want = []
    for q in qs:  # what sess.generate computes its first token from: the append on the session's cache, then a rewind
        be.append(q, None, q.shape[1])
        torch.cuda.synchronize()
        want.append(be.logits.clone())
        be.rewind(P)
    S = 12
    L.call("showo_engine_batch_begin_shared", eng, S, (P & 63) + max(q.shape[1] for q in qs) + 2)
    lgs = torch.full((S, d.vocab), float("nan"), dtype=torch.float32, device="cuda")
    for b, q in enumerate(qs):
        L.call("showo_engine_batch_attach_append", eng, b, L.ptr(q), None, q.shape[1], L.ptr(lgs[b]), L.stream())
    torch.cuda.synchronize()
    for b in range(S):
        assert torch.equal(lgs[b], want[b]), (P, b)
    p_, b_, c_ = C.c_int(), C.c_int(), C.c_int()
    L.call("showo_engine_batch_shared_state", eng, C.byref(p_), C.byref(b_), C.byref(c_))
    assert (p_.value, b_.value) == (P, P & ~63) and c_.value % 64 == 0
    cap = C.c_int()
    L.call("showo_engine_batch_slot_ptrs", eng, 3, None, None, None, None, C.byref(cap))
    assert cap.value == c_.value
    assert be.cached_rows() == P  # the engine's cache is back at the prefix


# ---- session unchanged ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PREFIXES)
def test_the_session_and_its_cache_bits_are_unchanged(P):
    g, d, sd, m = _tiny()
    full = _full_prompt(g, P)
    sess = _session(m, d, full, P)
    mark = sess.mark()
    before = [int(t) for t in sess.generate(dev(full[:, P:]), max_new_tokens=12, top_k=1)]
    sess.rewind(mark)
    n0, ep0, K0, V0 = _cache_snapshot(m, P)
    qs = _questions(full, P, 12)
    kw = dict(max_new_tokens=20, top_k=[1, 5, None] * 4, temperature=[1.0, 0.7, 1.1] * 4, top_p=[None, None, 0.9] * 4, return_logprobs=True)
    gen = lambda: torch.Generator(device="cuda").manual_seed(9)
    t16, l16 = sess.generate_batch(idx=qs, generator=gen(), slots=16, share_prefix=True, **kw)
    assert sess.length == P
    n1, ep1, K1, V1 = _cache_snapshot(m, P)
    assert (n1, ep1) == (n0, ep0) and torch.equal(K1, K0) and torch.equal(V1, V0)
    assert bool((V1[:, :, :, P:] == 0).all())  # the zero tail behind the prefix
    t32, l32 = sess.generate_batch(idx=qs, generator=gen(), slots=32, share_prefix=True, **kw)
    assert _ints(t16) == _ints(t32) and all(torch.equal(a, b) for a, b in zip(l16, l32))
    assert all(len(t) == 20 for t in t16)
    after = [int(t) for t in sess.generate(dev(full[:, P:]), max_new_tokens=12, top_k=1)]
    assert after == before


# ---- against the oracle, teacher-forced, next to the forked wide path ---------------------------------------------------------------
@pytest.mark.parametrize("P", PREFIXES)
def test_shared_step_logits_vs_oracle_next_to_the_forked_wide_step(P):
    """The prompt's own question in slot 11 of 12, other questions around it, 40 teacher-forced steps: the logits of every step against
    the fp32 oracle on the shared path and, measured the same way in the same test, on the forked wide path (showo_engine_batch_fork +
    _batch_prefill_append on showo_engine_batch_begin_wide).  Both round the same tensors to bf16; the shared attention rounds P
    relative to its key segment's max and splits the fp32 sums: it may exceed the forked figures by 10 % (the margin
    test_wide_step_logits_vs_oracle_next_to_the_batch1_step gives a path with the same rounding classes in another order).
    Figures: the [parity] lines; DESIGN.md "Shared-prefix slots"."""
    steps = 40
    g, d, sd, m = _tiny()
    sdt = O.to_torch(sd)
    full = _full_prompt(g, P)
    fmask = O.mask_mmu(full, d.eoi_id)
    toks_ref = [int(t) for t in O.mmu_generate(sdt, d, full, attention_mask=fmask, max_new_tokens=steps, top_k=1)]
    seq = torch.cat([full, torch.tensor([toks_ref[:-1]], dtype=torch.int64)], dim=1)
    ref = O.showo_logits(sdt, d, seq, attention_mask=O.mask_mmu(seq, d.eoi_id))[0, full.shape[1] - 1:]
    assert [int(r.argmax()) for r in ref] == toks_ref
    sess = _session(m, d, full, P)
    L = util.lib()
    eng = m.engine()
    V = d.vocab
    S, slot = 12, 11
    qs = _questions(full, P, S)
    rows = qs[1:] + qs[:1]  # the prompt's question in slot 11
    longest = max(q.shape[1] for q in rows)

    def teacher_forced(shared):
        if shared:
            L.call("showo_engine_batch_begin_shared", eng, S, (P & 63) + longest + steps + 1)
        else:
            L.call("showo_engine_batch_begin_wide", eng, S, P + longest + steps + 1)
        lgs = torch.empty((S, V), dtype=torch.float32, device="cuda")
        for b, q in enumerate(rows):
            if shared:
                L.call("showo_engine_batch_attach_append", eng, b, L.ptr(q), None, q.shape[1], L.ptr(lgs[b]), L.stream())
            else:
                L.call("showo_engine_batch_fork", eng, b, L.stream())
                L.call("showo_engine_batch_prefill_append", eng, b, L.ptr(q), None, q.shape[1], L.ptr(lgs[b]), L.stream())
        tok = lgs.argmax(dim=1).to(torch.int64).contiguous()
        out = torch.empty((S, 1), dtype=torch.int64, device="cuda")
        got = []
        for j, t in enumerate(toks_ref):
            torch.cuda.synchronize()
            got.append(lgs[slot].cpu().clone())
            if j + 1 < steps:
                tok[slot] = t  # teacher-forced; the other slots feed their own arg-max
                L.call("showo_engine_batch_decode_greedy", eng, L.ptr(tok), 1, L.ptr(out), L.ptr(lgs), 0, L.stream())
        return torch.stack(got)

    forked = teacher_forced(False)
    shared = teacher_forced(True)
    assert torch.isfinite(shared).all()
    assert torch.equal(shared[0], forked[0])  # the first logits come from the same append
    maxf, rmsf = util.relerr(forked, ref)
    maxs, rmss = util.relerr(shared, ref)
    print(f"[parity] tiny teacher-forced decode vs oracle, prefix {P}, {steps} steps: shared (slot 11 of 12) rel_max={maxs:.3e} "
          f"rel_rms={rmss:.3e}; forked wide rel_max={maxf:.3e} rel_rms={rmsf:.3e}; ratio {maxs / maxf:.3f} / {rmss / rmsf:.3f}")
    assert maxs <= 1.10 * maxf and rmss <= 1.10 * rmsf, (maxs, maxf, rmss, rmsf)
    top2 = ref.topk(2, dim=1).values
    gaps = (top2[:, 0] - top2[:, 1]).tolist()
    errs = (shared - ref).abs().max(dim=1).values.tolist()
    decided = 0
    for j in range(steps):
        if gaps[j] > 2.0 * errs[j]:
            decided += 1
            assert int(shared[j].argmax()) == toks_ref[j], (j, gaps[j], errs[j])
    print(f"[parity] tiny shared greedy tokens vs oracle, prefix {P}: steps decided by the gap rule {decided}/{steps}")
    assert decided * 4 >= steps * 3, decided


# ---- scheduler -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PREFIXES)
def test_shared_scheduler_refills_slots_and_stops_each_request_at_its_eot(P, monkeypatch):
    g, d, sd, m = _tiny()
    full = _full_prompt(g, P)
    sess = _session(m, d, full, P)
    n, S, new = 20, 9, 30
    qs = _questions(full, P, n)
    free = _ints(sess.generate_batch(idx=qs, max_new_tokens=new, top_k=1, slots=S, share_prefix=True))
    assert [len(r) for r in free] == [new] * n
    # an <eot> that stops the requests at different places (the tiny model's continuations share most of their tokens): the first
    # token of the free runs whose first occurrence cuts them to at least three different lengths
    def cut(t):
        return [r[:r.index(t) + 1] if t in r else r for r in free]

    eot = next(t for r in free for t in r[1:] if len({len(c) for c in cut(t)}) >= 3)
    want = cut(eot)
    assert any(len(r) < new for r in want) and len({len(r) for r in want}) >= 3
    L = util.lib()
    calls = {"attach": 0, "fork": 0, "append": 0, "shared": 0, "wide": 0, "narrow": 0}
    names = {"showo_engine_batch_attach_append": "attach", "showo_engine_batch_fork": "fork", "showo_engine_batch_prefill_append": "append",
             "showo_engine_batch_begin_shared": "shared", "showo_engine_batch_begin_wide": "wide", "showo_engine_batch_begin": "narrow"}
    real = L.call

    def counting(name, *a):
        if name in names:
            calls[names[name]] += 1
        return real(name, *a)

    monkeypatch.setattr(L, "call", counting)

    def refuse(*a, **k):
        raise AssertionError("generate_batch fell back to sequential generate calls")

    monkeypatch.setattr(type(sess), "generate", refuse)
    got = _ints(sess.generate_batch(idx=qs, max_new_tokens=new, top_k=1, eot_token=eot, slots=S, share_prefix=True))
    assert got == want
    assert calls == {"attach": n, "fork": 0, "append": 0, "shared": 1, "wide": 0, "narrow": 0}  # 20 attaches on 9 slots: 11 are refills
    assert sess.length == P


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PREFIXES)
def test_refusals_change_no_state(P):
    g, d, sd, m = _tiny()
    L = util.lib()
    lib = L.load()
    assert lib.showo_engine_batch_begin_shared(m.engine(), 9, 64) == 1  # no prefill yet
    full = _full_prompt(g, P)
    sess = _session(m, d, full, P)
    qs = _questions(full, P, 12)
    eng = m.engine()
    state0 = sess._be.state()
    with pytest.raises(ValueError, match="slots"):
        sess.generate_batch(idx=qs, max_new_tokens=4, top_k=1, share_prefix=True)
    with pytest.raises(ValueError):
        sess.generate_batch(idx=qs[:4], max_new_tokens=4, top_k=1, share_prefix=True)
    assert sess._be.state() == state0 and sess.length == P
    assert lib.showo_engine_batch_begin_shared(eng, 33, 64) == 1 and lib.showo_engine_batch_begin_shared(eng, 0, 64) == 1
    assert lib.showo_engine_batch_begin_shared(eng, 9, (P & 63) + 1) == 5  # no room behind the prefix
    # a running shared batch refuses to decode once the engine's cache moved
    S, V = 9, d.vocab
    lgs = torch.empty((S, V), dtype=torch.float32, device="cuda")
    tok = torch.zeros((S,), dtype=torch.int64, device="cuda")
    out = torch.empty((S, 2), dtype=torch.int64, device="cuda")

    def begin_and_fill():
        L.call("showo_engine_batch_begin_shared", eng, S, (P & 63) + 16 + 8)
        for b in range(S):
            L.call("showo_engine_batch_attach_append", eng, b, L.ptr(qs[b]), None, qs[b].shape[1], L.ptr(lgs[b]), L.stream())
        tok.copy_(lgs.argmax(dim=1))

    def decode():
        return lib.showo_engine_batch_decode_greedy(eng, L.ptr(tok), 2, L.ptr(out), L.ptr(lgs), 0, L.stream())

    begin_and_fill()
    assert lib.showo_engine_batch_fork(eng, 0, L.stream()) == 1  # the fork family refuses a shared batch
    assert lib.showo_engine_batch_attach_append(eng, S, L.ptr(qs[0]), None, qs[0].shape[1], L.ptr(lgs[0]), L.stream()) == 1
    cap_s = C.c_int()
    L.call("showo_engine_batch_shared_state", eng, None, None, C.byref(cap_s))
    long_q = dev(torch.full((1, cap_s.value - (P & 63)), 7, dtype=torch.int64))  # with the row behind it, one more than the suffix cache holds
    assert lib.showo_engine_batch_attach_append(eng, 0, L.ptr(long_q), None, long_q.shape[1], L.ptr(lgs[0]), L.stream()) == 5
    assert decode() == 0
    one = torch.empty((V,), dtype=torch.float32, device="cuda")
    L.call("showo_engine_prefill_append", eng, L.ptr(qs[0]), None, qs[0].shape[1], L.ptr(one), L.stream())  # an append left in place
    assert decode() == 1
    assert lib.showo_engine_batch_attach_append(eng, 0, L.ptr(qs[0]), None, qs[0].shape[1], L.ptr(lgs[0]), L.stream()) == 1
    L.call("showo_engine_cache_rewind", eng, P, L.stream())
    begin_and_fill()
    assert decode() == 0
    pre = dev(full[:, :P])
    mask = dev(O.mask_mmu(full[:, :P], d.eoi_id)).float().reshape(1, 1, P, P).contiguous()
    L.call("showo_engine_prefill", eng, L.ptr(pre), None, L.ptr(mask), P, L.ptr(one), L.stream())  # a new prefill: another epoch
    assert decode() == 1
    torch.cuda.synchronize()
    # the precision changes under a running shared batch: its decode and attach entries refuse
    begin_and_fill()
    assert decode() == 0
    torch.cuda.synchronize()
    m.set_precision(2)
    assert m.engine() is eng  # the same engine, now at precision 2

    def batch_record():
        p_, b_, c_ = C.c_int(), C.c_int(), C.c_int()
        L.call("showo_engine_batch_shared_state", eng, C.byref(p_), C.byref(b_), C.byref(c_))
        return p_.value, b_.value, c_.value

    record = batch_record()
    assert decode() == 1
    assert lib.showo_engine_batch_attach_append(eng, 0, L.ptr(qs[0]), None, qs[0].shape[1], L.ptr(lgs[0]), L.stream()) == 1
    assert lib.showo_engine_batch_begin_shared(eng, 9, 64) == 1  # (the cache was prefilled at precision 0)
    assert batch_record() == record  # a refused begin leaves the batch on record as it was
    # a session opened AT precision 2: share_prefix is refused by its own check, and nothing moves
    sess2 = _session(m, d, full, P)
    eng2 = m.engine()
    state2 = sess2._be.state()
    assert state2[0] == P
    with pytest.raises(ValueError, match="share_prefix needs precision 0"):
        sess2.generate_batch(idx=qs, max_new_tokens=4, top_k=1, slots=16, share_prefix=True)
    with pytest.raises(ValueError, match="share_prefix needs precision 0"):
        sess2.generate_batch(idx=qs[:4], max_new_tokens=4, top_k=1, slots=16, share_prefix=True)
    assert sess2._be.state() == state2 and sess2.length == P
    assert lib.showo_engine_batch_begin_shared(eng2, 9, 64) == 1  # a cache of precision 2: a shared batch is a wide batch, precision 0 only
    assert eng2 is eng and batch_record() == record and decode() == 1
    assert sess2._be.state() == state2 and sess2.length == P
    after = [int(t) for t in sess2.generate(qs[0], max_new_tokens=4, top_k=1)]  # the session still answers
    assert len(after) == 4
    m.set_precision(0)
