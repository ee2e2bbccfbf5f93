"""GPU tests of the sampled, slot-scheduled batched decode (csrc/decode_batch.hip sample_seam_rows_kernel,
showo_engine_batch_decode_sample, Showo.mmu_generate_batch's slot scheduler).

The specification is unchanged from the greedy batch: `mmu_generate_batch` returns, bit for bit, what n sequential `mmu_generate`
calls return -- now for sampled and mixed batches (per-slot top_k / temperature / seed, seeds drawn from `generator` as the sequential
calls draw them) and for any n >= 2 (at most 8 slots, refilled as sequences finish).  At the C ABI every slot's tokens AND logits bits
equal its batch-1 run."""
import numpy as np
import pytest
import torch

import util
from util import O, Wt, dev

pytestmark = pytest.mark.gpu


def _prompts(d, g, n):
    """n mmu prompts of different lengths derived from the golden one: [<mmu>, <soi>, image tokens, <eoi>, text ...]"""
    rs = np.random.RandomState(7)
    base = g["ids"][0].tolist()
    out = []
    for b in range(n):
        extra = rs.randint(5, 200, size=3 * b + (b % 2)).tolist()
        row = base[:len(base) - (b % 4 if b % 2 else 0)] + extra
        out.append(torch.tensor([row], dtype=torch.int64))
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


def _single(m, ids, masks, gen=None, **kw):
    """n sequential mmu_generate calls; top_k / temperature / _exp_noise may be per-sequence lists"""
    out = []
    for b in range(len(ids)):
        a = {k: (v[b] if isinstance(v, list) else v) for k, v in kw.items()}
        out.append([int(t) for t in m.mmu_generate(ids[b], attention_mask=masks[b], generator=gen, **a)])
    return out


# per-slot (top_k, temperature) of the C ABI test: top-k, unfiltered (None -> 0), greedy, wide top-k
SLOTS = [(5, 0.7), (0, 1.3), (1, 1.0), (50, 1.0)]


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("graph", [0, 1])
def test_batch_decode_sample_is_the_bits_of_the_batch1_runs(precision, graph):
    """showo_engine_batch_decode_sample against showo_engine_decode_sample / _decode_greedy: equal tokens and equal logits bits per slot,
    over two consecutive calls (draw indices continue across the chunk boundary); slot 1 draws from an injected Exp(1) table"""
    g, d, m = _tiny(precision)
    L = util.lib()
    eng = m.engine()
    V, n, s1, s2 = d.vocab, len(SLOTS), 5, 6
    steps = s1 + s2
    ids = [t.cuda() for t in _prompts(d, g, n)]
    masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda().float().contiguous() for t in ids]
    seeds = [1234567 + 1000 * b for b in range(n)]
    noise = [None, dev(np.random.RandomState(3).exponential(size=(1 + steps, V)).astype(np.float32)), None, None]
    side = torch.cuda.Stream()

    def first(lg, b, tok):
        k, T = SLOTS[b]
        if k == 1:
            L.call("showo_argmax_f32", L.ptr(lg), V, L.ptr(tok), L.stream())
        else:
            L.call("showo_sample_topk", L.ptr(lg), V, k, T, L.ptr(noise[b]), seeds[b], 0, L.ptr(tok), L.stream())

    ref_logits, ref_tokens = [], []
    for b in range(n):
        lg = torch.empty((V,), dtype=torch.float32, device="cuda")
        tok = torch.empty((1,), dtype=torch.int64, device="cuda")
        L.call("showo_engine_prefill", eng, L.ptr(ids[b]), None, L.ptr(masks[b]), ids[b].shape[1], L.ptr(lg), L.stream())
        first(lg, b, tok)
        out = torch.empty((steps,), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        k, T = SLOTS[b]
        with torch.cuda.stream(side):
            if k == 1:
                L.call("showo_engine_decode_greedy", eng, L.ptr(tok), steps, L.ptr(out), L.ptr(lg), graph, L.stream())
            else:
                L.call("showo_engine_decode_sample", eng, L.ptr(tok), steps, L.ptr(out), L.ptr(lg), k, T, L.ptr(noise[b]), seeds[b], 1,
                       graph, L.stream())
        torch.cuda.synchronize()
        ref_logits.append(lg.clone()), ref_tokens.append(out.tolist())

    import ctypes as C
    cap = max(t.shape[1] for t in ids) + steps + 1
    L.call("showo_engine_batch_begin", eng, n, cap)
    lgs = torch.empty((n, V), dtype=torch.float32, device="cuda")
    tok = torch.empty((n,), dtype=torch.int64, device="cuda")
    for b in range(n):
        L.call("showo_engine_batch_prefill", eng, b, L.ptr(ids[b]), None, L.ptr(masks[b]), ids[b].shape[1], L.ptr(lgs[b]), L.stream())
        first(lgs[b], b, tok[b:b + 1])
    a_k = (C.c_int * n)(*[k for k, _ in SLOTS])
    a_t = (C.c_float * n)(*[T for _, T in SLOTS])
    a_s = (C.c_uint64 * n)(*seeds)
    a_n = (C.c_void_p * n)(*[L.ptr(z) for z in noise])
    got = []
    for cnt, d0 in ((s1, 1), (s2, 1 + s1)):
        out = torch.empty((n, cnt), dtype=torch.int64, device="cuda")
        prod = (C.c_int * n)()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            L.call("showo_engine_batch_decode_sample", eng, L.ptr(tok), cnt, L.ptr(out), L.ptr(lgs), C.cast(a_k, C.c_void_p),
                   C.cast(a_t, C.c_void_p), C.cast(a_s, C.c_void_p), C.cast((C.c_int * n)(*[d0] * n), C.c_void_p), C.cast(a_n, C.c_void_p),
                   C.cast((C.c_int * n)(*[cnt] * n), C.c_void_p), -1, C.cast(prod, C.c_void_p), graph, L.stream())
        torch.cuda.synchronize()
        assert list(prod) == [cnt] * n
        got.append(out.tolist())
    assert [got[0][b] + got[1][b] for b in range(n)] == ref_tokens
    for b in range(n):
        assert torch.equal(lgs[b], ref_logits[b]), (b, float((lgs[b] - ref_logits[b]).abs().max()))
    # a budget above what the cache still holds is refused
    big = torch.empty((n, 4096), dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError):
        L.call("showo_engine_batch_decode_sample", eng, L.ptr(tok), 4096, L.ptr(big), L.ptr(lgs), C.cast(a_k, C.c_void_p), C.cast(a_t, C.c_void_p),
               C.cast(a_s, C.c_void_p), C.cast((C.c_int * n)(*[0] * n), C.c_void_p), None, C.cast((C.c_int * n)(*[4096] * n), C.c_void_p), -1,
               C.cast((C.c_int * n)(), C.c_void_p), 0, L.stream())


@pytest.mark.parametrize("precision", [0, 2])
def test_batch_decode_sample_idle_slot_at_the_capacity_stays_inside(precision):
    """slot 0 spends its budget exactly at the cache capacity while slot 1 keeps decoding: the idle slot keeps its last position (inside
    the cache), writes -1, and slot 1's tokens and logits stay the bits of its batch-1 run; slot 0's tokens are its batch-1 tokens"""
    g, d, m = _tiny(precision)
    L = util.lib()
    eng = m.engine()
    V = d.vocab
    ids = [t.cuda() for t in _prompts(d, g, 8)]
    ids = [ids[7], ids[0]]  # long, short
    masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda().float().contiguous() for t in ids]
    cap = 128
    budgets = [cap - ids[0].shape[1], cap - ids[1].shape[1]]
    steps = budgets[1]
    assert budgets[0] < steps
    side = torch.cuda.Stream()
    ref = []
    for b in range(2):
        lg = torch.empty((V,), dtype=torch.float32, device="cuda")
        tok = torch.empty((1,), dtype=torch.int64, device="cuda")
        L.call("showo_engine_prefill", eng, L.ptr(ids[b]), None, L.ptr(masks[b]), ids[b].shape[1], L.ptr(lg), L.stream())
        L.call("showo_argmax_f32", L.ptr(lg), V, L.ptr(tok), L.stream())
        out = torch.empty((budgets[b],), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            L.call("showo_engine_decode_greedy", eng, L.ptr(tok), budgets[b], L.ptr(out), L.ptr(lg), 1, L.stream())
        torch.cuda.synchronize()
        ref.append((out.tolist(), lg.clone()))
    import ctypes as C
    L.call("showo_engine_batch_begin", eng, 2, cap)
    lgs = torch.empty((2, V), dtype=torch.float32, device="cuda")
    tok = torch.empty((2,), dtype=torch.int64, device="cuda")
    for b in range(2):
        L.call("showo_engine_batch_prefill", eng, b, L.ptr(ids[b]), None, L.ptr(masks[b]), ids[b].shape[1], L.ptr(lgs[b]), L.stream())
        L.call("showo_argmax_f32", L.ptr(lgs[b]), V, L.ptr(tok[b:b + 1]), L.stream())
    out = torch.empty((2, steps), dtype=torch.int64, device="cuda")
    prod = (C.c_int * 2)()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        L.call("showo_engine_batch_decode_sample", eng, L.ptr(tok), steps, L.ptr(out), L.ptr(lgs), C.cast((C.c_int * 2)(1, 1), C.c_void_p),
               C.cast((C.c_float * 2)(1.0, 1.0), C.c_void_p), C.cast((C.c_uint64 * 2)(0, 0), C.c_void_p), C.cast((C.c_int * 2)(1, 1), C.c_void_p),
               None, C.cast((C.c_int * 2)(*budgets), C.c_void_p), -1, C.cast(prod, C.c_void_p), 1, L.stream())
    torch.cuda.synchronize()
    assert list(prod) == budgets
    rows = out.tolist()
    assert rows[0] == ref[0][0] + [-1] * (steps - budgets[0])
    assert rows[1] == ref[1][0]
    assert torch.equal(lgs[1], ref[1][1])
    assert torch.isfinite(lgs[0]).all()  # the idle slot's row stayed bounded


@pytest.mark.parametrize("precision", [0, 2])
def test_mmu_generate_batch_reproduces_the_reference_draws(precision):
    """sequence 0 is the golden prompt with the reference's recorded Exp(1) draws injected: its tokens are the reference's
    (tokens_topk5 / tokens_full); the other sequences (greedy and sampled) equal their single calls"""
    g, d, m = _tiny(precision)
    ids = [dev(g["ids"])] + [t.cuda() for t in _prompts(d, g, 3)[1:]]
    masks = [dev(g["mask"])] + [O.mask_mmu(t.cpu(), d.eoi_id).cuda() for t in ids[1:]]
    for tag, k0, t0 in (("topk5", 5, 0.7), ("full", None, 1.3)):
        kw = dict(max_new_tokens=8, top_k=[k0, 1, 5], temperature=[t0, 1.0, 0.9], _exp_noise=[dev(g[f"exp_noise_{tag}"]), None, None])
        want = _single(m, ids, masks, _gen(17), **kw)
        for graph in (0, 1):
            m.decode_graph = graph
            got = _ints(m.mmu_generate_batch(idx=ids, attention_mask=masks, generator=_gen(17), **kw))
            assert got[0] == g[f"tokens_{tag}"].tolist(), (tag, graph)
            assert got == want, (tag, graph)
    m.decode_graph = 1


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_mmu_generate_batch_draws_like_sequential_calls(n, precision):
    """seeded torch.Generator and torch.manual_seed + generator=None: the batch equals n sequential mmu_generate calls from an identically
    seeded generator -- for a scalar top-k batch and a mixed greedy / top-k / unfiltered batch, with and without an <eot> that stops
    some sequences early"""
    g, d, m = _tiny(precision)
    ids = [t.cuda() for t in _prompts(d, g, n)]
    masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda() for t in ids]
    ks, ts = [1, 5, None, 1], [1.0, 0.7, 1.3, 1.0]
    mixed = dict(top_k=[ks[b % 4] for b in range(n)], temperature=[ts[b % 4] for b in range(n)])
    for kw in (dict(top_k=5, temperature=0.7), mixed):
        want = _single(m, ids, masks, _gen(5), max_new_tokens=40, **kw)
        got = _ints(m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=40, generator=_gen(5), **kw))
        assert got == want
        torch.manual_seed(21)
        want = _single(m, ids, masks, None, max_new_tokens=40, **kw)
        torch.manual_seed(21)
        got = _ints(m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=40, **kw))
        assert got == want
        eot = _single(m, ids, masks, _gen(9), max_new_tokens=40, **kw)[1][3]  # sequence 1 (and any other that draws it) stops early
        want = _single(m, ids, masks, _gen(9), max_new_tokens=40, eot_token=eot, **kw)
        got = _ints(m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=40, eot_token=eot, generator=_gen(9), **kw))
        assert got == want and len(got[1]) <= 4


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("n", [12, 20])
def test_mmu_generate_batch_refills_slots_without_falling_back(n, precision, monkeypatch):
    """more sequences than slots: long prompts first (each slot gets a shorter successor), some sequences ending at <eot> after a few
    tokens; with Showo.mmu_generate disabled the batched call still returns what n sequential calls return"""
    g, d, m = _tiny(precision)
    ids = [t.cuda() for t in _prompts(d, g, n)][::-1]
    masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda() for t in ids]
    cases = []
    for kw in (dict(top_k=1), dict(top_k=5, temperature=0.8), dict(top_k=[1, 5, None] * (n // 3) + [1] * (n % 3),
                                                                    temperature=[1.0, 0.7, 1.2] * (n // 3) + [1.0] * (n % 3))):
        free = _single(m, ids, masks, _gen(3), max_new_tokens=30, **kw)
        eot = free[2][4]
        want = _single(m, ids, masks, _gen(3), max_new_tokens=30, eot_token=eot, **kw)
        assert any(len(r) < 30 for r in want)
        cases.append((kw, eot, want))

    def refuse(*a, **k):
        raise AssertionError("mmu_generate_batch fell back to sequential mmu_generate calls")

    monkeypatch.setattr(util.pkg().Showo, "mmu_generate", refuse)
    for kw, eot, want in cases:
        got = _ints(m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=30, eot_token=eot, generator=_gen(3), **kw))
        assert got == want


@pytest.mark.parametrize("precision", [0, 2])
def test_mmu_generate_batch_fills_the_capacity_exactly(precision):
    """longest prompt + max_new_tokens + 1 is exactly the (64-aligned) batch capacity; one sequence stops at <eot> early and nothing is
    pending: the call succeeds and matches the single calls"""
    g, d, m = _tiny(precision)
    ids = [t.cuda() for t in _prompts(d, g, 3)]
    Lmax = max(t.shape[1] for t in ids)
    max_new = 128 - Lmax - 1
    masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda() for t in ids]
    kw = dict(top_k=[5, 1, None], temperature=[0.7, 1.0, 1.1])
    free = _single(m, ids, masks, _gen(8), max_new_tokens=max_new, **kw)
    eot = free[1][2]
    want = _single(m, ids, masks, _gen(8), max_new_tokens=max_new, eot_token=eot, **kw)
    assert len(want[1]) <= 3
    got = _ints(m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=max_new, eot_token=eot, generator=_gen(8), **kw))
    assert got == want


def test_full_size_cfg4_sampled_batch_equals_sequential_calls():
    """BASELINE cfg4 shape (631-embedding w_clip_vit prompts, full-size seeded weights): 4 sequences with top_k=5, temperature=0.7,
    24 tokens, decoded together == 4 sequential calls from the same generator"""
    g = util.golden("showo_full_cfg4.npz")
    d = Wt.ShowoDims(w_clip_vit=True)
    sd = Wt.make_showo_state(d, seed=int(g["seed"]))
    m = util.build_showo(d, sd, max_batch=1, max_seq=768)
    del sd
    feats = torch.from_numpy(np.random.RandomState(int(g["feat_seed"])).standard_normal((1, 576, 1024)).astype(np.float32)).cuda()
    ids_llava = torch.from_numpy(g["ids_llava"].astype(np.int64)).cuda()
    tab = m.showo.model.embed_tokens.weight
    with torch.no_grad():
        img = m.mm_projector(feats)
        txt = tab[ids_llava]
        emb = torch.cat([txt[:, :30], img, txt[:, 30:]], dim=1).contiguous()
    assert emb.shape[1] == 631
    P = util.pkg().prompting_utils
    embs = [emb, emb[:, :620].contiguous(), torch.cat([emb, emb[:, 600:612]], dim=1).contiguous(), emb[:, :600].contiguous()]
    ams = [P.create_attention_mask_for_mmu_vit(e_, system_prompt_len=28)[0] for e_ in embs]
    gen = _gen(4)
    single = [[int(t) for t in m.mmu_generate(input_embeddings=e_, attention_mask=k_, max_new_tokens=24, top_k=5, temperature=0.7,
                                              generator=gen)] for e_, k_ in zip(embs, ams)]
    got = _ints(m.mmu_generate_batch(input_embeddings=embs, attention_mask=ams, max_new_tokens=24, top_k=5, temperature=0.7,
                                     generator=_gen(4)))
    print(f"[parity] full-size cfg4, 4 sampled sequences decoded together == 4 batch-1 calls: {got == single}")
    assert got == single
