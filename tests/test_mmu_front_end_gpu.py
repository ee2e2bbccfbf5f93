"""Call traces of the mmu decode front end (show-o_amd/modeling_showo.py, Showo.mmu_generate .. MmuSession) on the tiny model.

Every test wraps `_lib.call` with a recorder that passes each call through and asserts the ORDERED list of (C entry, selected scalar
arguments) for the decode-related entries: which entry a combination of greedy / top_p / return_logprobs reaches, with which chunk
sizes, draw indices, slot counts and capacities, and how many seeds a generator gives up.  The expectations describe what the front
end asks of the engine, so a change of its host code that reaches another entry, another argument or another order fails here even
where the tokens stay the same.

Shape: the 25-token prompt of tests/golden/showo_tiny_mmu.npz (20 + 5 for a session), 19 new tokens -- the first one from the prefill
logits, then a chunk of 16 steps and a chunk of 2 -- at precision 0."""
import pytest
import torch

import util
from util import O, dev

pytestmark = pytest.mark.gpu

NEW = 19
CHUNKS = ((16, 1), (2, 17))  # (steps, first draw index) of the chunks behind the first token

# entry -> the scalar arguments kept in the trace (positions behind the entry name)
_WATCH = {
    "showo_engine_prefill": lambda a: (a[4],),                                    # L
    "showo_engine_prefill_append": lambda a: (a[3],),                             # Ln
    "showo_engine_cache_rewind": lambda a: (a[1],),                               # length
    "showo_engine_use_intervals": lambda a: ("reset" if a[1] is None else "set",),
    "showo_argmax_f32": lambda a: (a[1],),                                        # V
    "showo_sample_topk": lambda a: (a[2], a[3], a[5], a[6]),                      # k, temperature, seed, step
    "showo_sample_topk_topp": lambda a: (a[2], a[3], a[4], a[6], a[7]),           # k, p, temperature, seed, step
    "showo_logprob_rows": lambda a: (a[2],),                                      # rows
    "showo_engine_decode_greedy": lambda a: (a[2],),                              # n
    "showo_engine_decode_sample": lambda a: (a[2], a[5], a[6], a[8], a[9]),       # n, k, temperature, seed, step0
    "showo_engine_decode_sample_p": lambda a: (a[2], a[5], a[6], a[7], a[9], a[10]),      # n, k, p, temperature, seed, step0
    "showo_engine_decode_sample_lp": lambda a: (a[2], a[5], a[6], a[7], a[9], a[10]),     # n, k, p, temperature, seed, step0
    "showo_engine_batch_begin": lambda a: (a[1], a[2]),                           # slots, capacity
    "showo_engine_batch_begin_wide": lambda a: (a[1], a[2]),
    "showo_engine_batch_prefill": lambda a: (a[1], a[5]),                         # slot, L
    "showo_engine_batch_fork": lambda a: (a[1],),                                 # slot
    "showo_engine_batch_prefill_append": lambda a: (a[1], a[4]),                  # slot, Ln
    "showo_engine_batch_decode_greedy": lambda a: (a[2],),                        # m
    "showo_engine_batch_decode_sample": lambda a: (a[2],),
    "showo_engine_batch_decode_sample_p": lambda a: (a[2],),
    "showo_engine_batch_decode_sample_lp": lambda a: (a[2],),
}
RESET = ("showo_engine_use_intervals", "reset")


@pytest.fixture(scope="module")
def tiny():
    g = util.golden("showo_tiny_mmu.npz")
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd, max_batch=8, max_seq=128)
    m.set_precision(0)
    ids = torch.from_numpy(g["ids"]).to(torch.int64)
    assert ids.shape == (1, 25)
    return d, m, ids


def _trace(monkeypatch, fn):
    """(what fn() returns, the watched calls it made in order); every call goes through to the library"""
    L = util.lib()
    real, seen = L.call, []

    def recording(name, *a):
        if name in _WATCH:
            seen.append((name,) + tuple(_WATCH[name](a)))
        return real(name, *a)

    with monkeypatch.context() as mp:
        mp.setattr(L, "call", recording)
        out = fn()
    return out, seen


def _gen(seed=3):
    return torch.Generator(device="cuda").manual_seed(seed)


def _seeds(n, seed=3):
    """the first n Philox seeds a front end draws from _gen(seed), and the generator behind them"""
    g = _gen(seed)
    return [int(torch.randint(0, 2 ** 62, (1,), generator=g, device=g.device).item()) for _ in range(n)], g


def _ints(toks):
    return [int(t) for t in toks]


def _prompt(ids, d):
    return dev(ids), dev(O.mask_mmu(ids, d.eoi_id))


def _prompts(ids, n):
    """n prompts of different lengths from the golden one: request b carries b more tokens"""
    return [torch.cat([ids, torch.arange(30, 30 + b, dtype=torch.int64).reshape(1, b)], dim=1) for b in range(n)]


def _names(seen):
    return [c[0] for c in seen]


# ---- Showo.mmu_generate ---------------------------------------------------------------------------------------------------------
# mode -> (keywords, first pick, chunk entry and its arguments between n and step0); SEED stands for the one seed drawn
SEED = object()
_MODES = {
    "greedy": (dict(top_k=1), lambda V: ("showo_argmax_f32", V), lambda n, s0: ("showo_engine_decode_greedy", n),
               lambda n, s0: ("showo_engine_decode_sample_lp", n, 1, 1.0, 1.0, 0, s0)),
    "topk5": (dict(top_k=5, temperature=0.7), lambda V: ("showo_sample_topk", 5, 0.7, SEED, 0),
              lambda n, s0: ("showo_engine_decode_sample", n, 5, 0.7, SEED, s0),
              lambda n, s0: ("showo_engine_decode_sample_lp", n, 5, 1.0, 0.7, SEED, s0)),
    "topk5_topp0.9": (dict(top_k=5, temperature=0.7, top_p=0.9), lambda V: ("showo_sample_topk_topp", 5, 0.9, 0.7, SEED, 0),
                      lambda n, s0: ("showo_engine_decode_sample_p", n, 5, 0.9, 0.7, SEED, s0),
                      lambda n, s0: ("showo_engine_decode_sample_lp", n, 5, 0.9, 0.7, SEED, s0)),
}


def _batch1_trace(mode, V, logprobs, seed, chunks=CHUNKS):
    """the calls of one batch-1 decode behind its prefill: first pick, its log-probability, the chunks"""
    kw, first, chunk, chunk_lp = _MODES[mode]
    want = [first(V)] + ([("showo_logprob_rows", 1)] if logprobs else [])
    want += [(chunk_lp if logprobs else chunk)(n, s0) for n, s0 in chunks]
    return [tuple(seed if x is SEED else x for x in c) for c in want]


@pytest.mark.parametrize("mode", list(_MODES))
def test_mmu_generate_reaches_one_entry_family_per_mode_and_log_probabilities_change_no_token(tiny, monkeypatch, mode):
    d, m, ids = tiny
    x, mask = _prompt(ids, d)
    kw = _MODES[mode][0]
    (seed,), _ = _seeds(1)
    head = [("showo_engine_prefill", 25), RESET]
    toks, seen = _trace(monkeypatch, lambda: m.mmu_generate(x, attention_mask=mask, max_new_tokens=NEW, generator=_gen(), **kw))
    assert seen == head + _batch1_trace(mode, d.vocab, False, seed)
    assert len(toks) == NEW and all(isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 0 for t in toks)
    (toks_lp, lps), seen = _trace(monkeypatch, lambda: m.mmu_generate(x, attention_mask=mask, max_new_tokens=NEW, generator=_gen(),
                                                                      return_logprobs=True, **kw))
    assert seen == head + _batch1_trace(mode, d.vocab, True, seed)
    assert _ints(toks_lp) == _ints(toks)
    assert tuple(lps.shape) == (NEW,) and lps.dtype == torch.float32 and bool(torch.isfinite(lps).all()) and float(lps.max()) <= 0.0


def test_mmu_generate_stops_at_eot_after_one_chunk_and_draws_one_seed_per_sampled_call(tiny, monkeypatch):
    d, m, ids = tiny
    x, mask = _prompt(ids, d)
    free = _ints(m.mmu_generate(x, attention_mask=mask, max_new_tokens=NEW, top_k=1))
    eot = free[4]
    at = free.index(eot)
    assert at >= 1  # (the first token is not the <eot>: the run reaches the device loop)
    toks, seen = _trace(monkeypatch, lambda: m.mmu_generate(x, attention_mask=mask, max_new_tokens=NEW, top_k=1, eot_token=eot))
    assert seen == [("showo_engine_prefill", 25), RESET, ("showo_argmax_f32", d.vocab), ("showo_engine_decode_greedy", 16)]
    assert _ints(toks) == free[:at + 1]
    # max_new_tokens = 0: the prefill and the first pick run, the result is empty
    toks, seen = _trace(monkeypatch, lambda: m.mmu_generate(x, attention_mask=mask, max_new_tokens=0, top_k=1))
    assert toks == [] and seen == [("showo_engine_prefill", 25), RESET, ("showo_argmax_f32", d.vocab)]
    # one seed per sampled call, none per greedy call
    _, want = _seeds(1)
    g = _gen()
    m.mmu_generate(x, attention_mask=mask, max_new_tokens=3, top_k=1, generator=g)
    m.mmu_generate(x, attention_mask=mask, max_new_tokens=3, top_k=5, generator=g)
    assert torch.equal(g.get_state(), want.get_state())


# ---- Showo.mmu_generate_batch ---------------------------------------------------------------------------------------------------
def _batch(tiny, n):
    d, m, ids = tiny
    ps = _prompts(ids, n)
    return [dev(p) for p in ps], [dev(O.mask_mmu(p, d.eoi_id)) for p in ps], [int(p.shape[1]) for p in ps]


def _refuse(*a, **k):
    raise AssertionError("the batch fell back to sequential mmu_generate calls")


def test_batch_of_three_greedy_requests_runs_the_greedy_batch_loop(tiny, monkeypatch):
    d, m, ids = tiny
    xs, masks, lens = _batch(tiny, 3)
    monkeypatch.setattr(util.pkg().Showo, "mmu_generate", _refuse)
    out, seen = _trace(monkeypatch, lambda: m.mmu_generate_batch(idx=xs, attention_mask=masks, max_new_tokens=NEW, top_k=1))
    want = [("showo_engine_batch_begin", 3, max(lens) + NEW + 1)]
    for b in range(3):
        want += [("showo_engine_batch_prefill", b, lens[b]), RESET, ("showo_argmax_f32", d.vocab)]
    want += [("showo_engine_batch_decode_greedy", 16), ("showo_engine_batch_decode_greedy", 2)]
    assert seen == want
    assert [len(r) for r in out] == [NEW] * 3


@pytest.mark.parametrize("case", ["mixed", "mixed_topp", "greedy_logprobs"])
def test_batch_of_three_on_slots_takes_the_p_and_lp_entries_only_when_asked(tiny, monkeypatch, case):
    d, m, ids = tiny
    V = d.vocab
    xs, masks, lens = _batch(tiny, 3)
    monkeypatch.setattr(util.pkg().Showo, "mmu_generate", _refuse)
    (s1, s2), _ = _seeds(2)
    if case == "greedy_logprobs":
        kw = dict(top_k=1, return_logprobs=True)
        picks = [[("showo_argmax_f32", V), ("showo_logprob_rows", 1)]] * 3
        entry = "showo_engine_batch_decode_sample_lp"
    else:
        topp = case == "mixed_topp"
        kw = dict(top_k=[1, 5, None], temperature=[1.0, 0.7, 1.1], generator=_gen(), **(dict(top_p=[None, None, 0.9]) if topp else {}))
        last = ("showo_sample_topk_topp", 0, 0.9, 1.1, s2, 0) if topp else ("showo_sample_topk", 0, 1.1, s2, 0)
        picks = [[("showo_argmax_f32", V)], [("showo_sample_topk", 5, 0.7, s1, 0)], [last]]
        entry = "showo_engine_batch_decode_sample_p" if topp else "showo_engine_batch_decode_sample"
    out, seen = _trace(monkeypatch, lambda: m.mmu_generate_batch(idx=xs, attention_mask=masks, max_new_tokens=NEW, **kw))
    want = [("showo_engine_batch_begin", 3, max(lens) + NEW + 1)]
    for s in range(3):
        want += [("showo_engine_batch_prefill", s, lens[s]), RESET] + picks[s]
    want += [(entry, 16), (entry, 2)]
    assert seen == want
    toks = out[0] if case == "greedy_logprobs" else out
    assert [len(r) for r in toks] == [NEW] * 3
    if case == "greedy_logprobs":
        assert [tuple(l.shape) for l in out[1]] == [(NEW,)] * 3


def test_batch_of_ten_without_slots_runs_on_eight_narrow_slots(tiny, monkeypatch):
    d, m, ids = tiny
    xs, masks, lens = _batch(tiny, 10)
    monkeypatch.setattr(util.pkg().Showo, "mmu_generate", _refuse)
    out, seen = _trace(monkeypatch, lambda: m.mmu_generate_batch(idx=xs, attention_mask=masks, max_new_tokens=NEW, top_k=1))
    names = _names(seen)
    assert seen[0] == ("showo_engine_batch_begin", 8, max(lens) + NEW + 1) and names.count("showo_engine_batch_begin") == 1
    assert "showo_engine_batch_begin_wide" not in names
    prefills = [c for c in seen if c[0] == "showo_engine_batch_prefill"]
    assert [c[2] for c in prefills] == lens                           # ten prefills, in request order
    assert [c[1] for c in prefills] == list(range(8)) + [0, 1]        # the two refills take the first free slots
    assert [c[1] for c in seen if c[0] == "showo_engine_batch_decode_sample"] == [16, 2, 16, 2]
    assert not [nm for nm in names if nm.startswith("showo_engine_batch_decode") and nm != "showo_engine_batch_decode_sample"]
    assert [len(r) for r in out] == [NEW] * 10


def test_batch_draws_one_seed_per_sampled_request(tiny):
    d, m, ids = tiny
    xs, masks, lens = _batch(tiny, 3)
    _, want = _seeds(2)
    g = _gen()
    m.mmu_generate_batch(idx=xs, attention_mask=masks, max_new_tokens=3, top_k=[5, 1, 5], generator=g)
    assert torch.equal(g.get_state(), want.get_state())


# ---- MmuSession -----------------------------------------------------------------------------------------------------------------
def _session(tiny):
    d, m, ids = tiny
    return m.mmu_session(dev(ids[:, :20]), attention_mask=dev(O.mask_mmu(ids[:, :20], d.eoi_id)))


def test_session_generate_appends_decodes_like_mmu_generate_and_rewinds_behind_the_fed_tokens(tiny, monkeypatch):
    d, m, ids = tiny
    sess, seen = _trace(monkeypatch, lambda: _session(tiny))
    assert seen == [("showo_engine_prefill", 20), RESET]
    assert type(sess._be).__name__ == "_SessionEngine"
    # at the prefix without rows: no append
    mark = sess.mark()
    toks, seen = _trace(monkeypatch, lambda: sess.generate(max_new_tokens=NEW, top_k=1))
    assert seen == _batch1_trace("greedy", d.vocab, False, None) + [("showo_engine_cache_rewind", 20 + NEW - 1)]
    assert len(toks) == NEW and sess.length == 20 + NEW - 1
    _, seen = _trace(monkeypatch, lambda: sess.rewind(mark))
    assert seen == [("showo_engine_cache_rewind", 20)]
    # with rows, every mode, with and without log-probabilities
    (seed,), _ = _seeds(1)
    for mode in _MODES:
        kw = _MODES[mode][0]
        for logprobs in (False, True):
            out, seen = _trace(monkeypatch, lambda: sess.generate(dev(ids[:, 20:]), max_new_tokens=NEW, generator=_gen(),
                                                                  **kw, **({"return_logprobs": True} if logprobs else {})))
            toks = out[0] if logprobs else out
            assert len(toks) == NEW and all(t.is_cuda for t in toks)
            assert seen == ([("showo_engine_prefill_append", 5)] + _batch1_trace(mode, d.vocab, logprobs, seed)
                            + [("showo_engine_cache_rewind", 25 + len(toks) - 1)]), (mode, logprobs)
            assert sess.length == 25 + NEW - 1
            sess.rewind(mark)


def test_session_generate_batch_forks_one_slot_per_request_and_leaves_the_session_unchanged(tiny, monkeypatch):
    d, m, ids = tiny
    V = d.vocab
    sess = _session(tiny)
    qs = [dev(torch.cat([ids[:, 20:], torch.arange(30, 30 + b, dtype=torch.int64).reshape(1, b)], dim=1)) for b in range(3)]
    lens = [5, 6, 7]
    (s0, s2), want_gen = _seeds(2)
    g = _gen()
    monkeypatch.setattr(sess, "generate", _refuse)
    out, seen = _trace(monkeypatch, lambda: sess.generate_batch(idx=qs, max_new_tokens=NEW, top_k=[5, 1, 5], temperature=0.7, generator=g))
    picks = [("showo_sample_topk", 5, 0.7, s0, 0), ("showo_argmax_f32", V), ("showo_sample_topk", 5, 0.7, s2, 0)]
    want = [("showo_engine_batch_begin", 3, 20 + max(lens) + NEW + 1)]
    for s in range(3):
        want += [("showo_engine_batch_fork", s), ("showo_engine_batch_prefill_append", s, lens[s]), picks[s]]
    want += [("showo_engine_batch_decode_sample", 16), ("showo_engine_batch_decode_sample", 2)]
    assert seen == want
    assert [len(r) for r in out] == [NEW] * 3
    assert sess.length == sess.prefix_length == 20
    assert torch.equal(g.get_state(), want_gen.get_state())
