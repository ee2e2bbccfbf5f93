"""CPU tests of the sequence rules' surface (no_repeat_ngram_size, bad_words_ids, min_new_tokens, stop_sequences): the C ABI
declarations and bindings, the keywords of the four entry points and their checks (which need no GPU), that a call with every keyword
at None makes exactly the C calls of a call without them, and the slot scheduler's stop sequences on a fake engine."""
import contextlib
import inspect
import os
import re

import pytest
import torch

import util
import seq_rules_ref as R

NEW_ENTRY_POINTS = ("showo_seq_ban", "showo_engine_decode_sample_seq", "showo_engine_batch_decode_sample_seq")
KEYWORDS = ("no_repeat_ngram_size", "bad_words_ids", "min_new_tokens", "stop_sequences")
V = 439


def _mod():
    return util.pkg().modeling_showo


def test_entry_points_are_declared_bound_and_exported():
    flat = re.sub(r"\s+", " ", open(os.path.join(util.ROOT, "include", "showo_hip.h")).read())
    L = util.lib()
    lib = L.load()
    for name in NEW_ENTRY_POINTS:
        args = re.search(r"int " + name + r"\(([^)]*)\);", flat)
        assert args, name
        assert name in L.EXPORTED_SYMBOLS and name in L._PROTOS and hasattr(lib, name), name
        assert len(args.group(1).split(",")) == len(L._PROTOS[name]), name
    # the _seq loops take everything the _adj forms take, in their order, plus the rules in front of use_graph
    for seq, adj in (("showo_engine_decode_sample_seq", "showo_engine_decode_sample_adj"),
                     ("showo_engine_batch_decode_sample_seq", "showo_engine_batch_decode_sample_adj")):
        a, b = L._PROTOS[seq], L._PROTOS[adj]
        assert a[:len(b) - 2] == b[:-2] and a[-2:] == b[-2:] and a[len(b) - 2:-2] == [L.c_p]
        assert re.sub(r"\s+", " ", re.search(r"int " + adj + r"\(([^)]*)\);", flat).group(1)).replace(", int use_graph", "") in \
            re.search(r"int " + seq + r"\(([^)]*)\);", flat).group(1).replace(", const showo_seq_rules* rules, int use_graph", "")
    # the structure of the header and its ctypes image: same fields, same order
    body = re.search(r"typedef struct showo_seq_rules \{(.*?)\} showo_seq_rules;", flat).group(1)
    names = [re.search(r"(\w+)$", f.strip()).group(1) for f in body.split(";") if f.strip()]
    assert names == [f[0] for f in L.SeqRules._fields_]
    assert "Sequence rules" in open(os.path.join(util.ROOT, "DESIGN.md")).read()
    assert "seq_rules" in open(os.path.join(util.ROOT, "show-o_amd", "csrc", "build.sh")).read()


def test_the_keywords_exist_and_default_to_none():
    S, M = util.pkg().Showo, _mod().MmuSession
    for fn in (S.mmu_generate, S.mmu_generate_batch, M.generate, M.generate_batch):
        p = inspect.signature(fn).parameters
        for k in KEYWORDS:
            assert k in p and p[k].default is None, (fn, k)
            assert k in (fn.__doc__ or ""), (fn, k)
    assert _mod()._SEQ_KEYS == KEYWORDS


# ---- the request builder -----------------------------------------------------------------------------------------------------------------
def test_all_none_is_no_request_and_rules_alone_are_a_bit_copy_adjustment():
    f = _mod()._adjust_of
    assert f(V, no_repeat_ngram_size=None, bad_words_ids=None, min_new_tokens=None, stop_sequences=None) is None
    assert f(V, bad_words_ids=[], stop_sequences=[]) is None
    a = f(V, no_repeat_ngram_size=3, repetition_context=[5, 7])
    assert a.theta == 1.0 and a.bias is None and a.context == [5, 7] and a.rules.ngram == 3 and a.rules.device
    a = f(V, bad_words_ids=[[4], [1, 2], torch.tensor([3, 4, 5]), (9,)], min_new_tokens=2, eot_token=7)
    assert a.rules.bad == [(1, 2), (3, 4, 5)] and a.rules.min_new == 2
    assert a.bias[4] == float("-inf") and a.bias[9] == float("-inf") and int(torch.isinf(a.bias).sum()) == 2  # one-token bad words
    assert a.rules.table.dtype == torch.int32 and a.rules.table.tolist() == R.table_of([[1, 2], [3, 4, 5]])
    a = f(V, stop_sequences=[[1, 2]], banned_tokens=[3])
    assert a.rules.stops == [(1, 2)] and not a.rules.device and a.rules.table is None
    assert f(V, bad_words_ids=[[6]]).rules is None  # only a banned token
    assert f(V, min_new_tokens=0, eot_token=3) is None


BAD = (dict(no_repeat_ngram_size=0), dict(no_repeat_ngram_size=-2), dict(no_repeat_ngram_size=2.0), dict(no_repeat_ngram_size=True),
       dict(no_repeat_ngram_size=17), dict(bad_words_ids=[[]]), dict(bad_words_ids=[[1, 2], []]), dict(bad_words_ids=[[1, V]]),
       dict(bad_words_ids=[[-1, 2]]), dict(bad_words_ids=[[1.5, 2]]), dict(bad_words_ids=[3, 4]), dict(bad_words_ids=[[1] * 65]),
       dict(bad_words_ids=[[1, 2]] * 1025), dict(stop_sequences=[[]]), dict(stop_sequences=[[V]]), dict(stop_sequences=[[0, -1]]),
       dict(min_new_tokens=-1, eot_token=5), dict(min_new_tokens=2), dict(min_new_tokens=1.5, eot_token=5))


@pytest.mark.parametrize("kw", BAD)
def test_bad_requests_are_value_errors(kw):
    with pytest.raises(ValueError):
        _mod()._adjust_of(V, **kw)


def test_per_request_values_shared_and_listed():
    f = _mod()._adjust_per_request
    assert f(3, V, no_repeat_ngram_size=None) == (None, [{}, {}, {}])
    adj, kws = f(3, V, no_repeat_ngram_size=2, bad_words_ids=[[1, 2], [3, 4]])  # shared: ONE request object
    assert adj[0] is adj[1] is adj[2] and adj[0].rules.ngram == 2 and adj[0].rules.bad == [(1, 2), (3, 4)]
    assert kws[2] == dict(no_repeat_ngram_size=2, bad_words_ids=[[1, 2], [3, 4]])
    adj, kws = f(3, V, no_repeat_ngram_size=[2, None, 4], bad_words_ids=[[[1, 2]], None, None], stop_sequences=[None, None, [[7], [8, 9]]],
                 min_new_tokens=[None, None, 3], eot_token=11)
    assert adj[1] is None and adj[0].rules.ngram == 2 and adj[0].rules.bad == [(1, 2)] and adj[0].rules.stops == []
    assert adj[2].rules.ngram == 4 and adj[2].rules.stops == [(7,), (8, 9)] and adj[2].rules.min_new == 3
    assert kws[1] == {} and set(kws[2]) == {"no_repeat_ngram_size", "stop_sequences", "min_new_tokens"}
    for bad in (dict(no_repeat_ngram_size=[2, 3]), dict(bad_words_ids=[[[1, 2]], None]), dict(min_new_tokens=[1, 1, 1])):
        with pytest.raises(ValueError):
            f(3, V, **bad)
    assert _mod()._hist_ld([None, adj[0], adj[2]], 12) == 12 and _mod()._hist_ld([None, f(1, V, stop_sequences=[[1]])[0][0]], 12) is None


# ---- the entry points refuse before they touch the engine --------------------------------------------------------------------------------
class _Model:
    """what the entry points read before they look at the keywords; engine() would touch the GPU"""
    _precision = 0
    vocab_size = V

    def engine(self):
        raise AssertionError("the engine was touched")


class _Backend:
    batched = True
    dev = torch.device("cpu")

    def stamp(self):
        return 1

    def cached_rows(self):
        return 3

    def prefill(self, idx, emb, mask):
        return 3

    def append(self, ids, emb, Ln):
        raise AssertionError("the engine was touched")

    def run_batch(self, *a, **k):
        raise AssertionError("the engine was touched")

    def run_beam(self, *a, **k):
        raise AssertionError("the engine was touched")


class _NoLib:
    """stands in for the _lib module: any C call is an error"""

    def call(self, name, *args):
        raise AssertionError(f"{name} was called")

    load = ptr = stream = call


def test_entry_points_refuse_bad_keywords_before_any_c_call(monkeypatch):
    monkeypatch.setattr(_mod(), "_lib", _NoLib())
    S = util.pkg().Showo
    ids = torch.tensor([[1, 2, 3]])
    sess = _mod().MmuSession(_Model(), idx=ids, _engine=_Backend())
    for kw in BAD:
        eot = {} if "eot_token" in kw else {"eot_token": None}
        with pytest.raises(ValueError):
            S.mmu_generate(_Model(), ids, max_new_tokens=2, top_k=1, **eot, **kw)
        with pytest.raises(ValueError):
            S.mmu_generate_batch(_Model(), idx=[ids] * 3, max_new_tokens=2, top_k=1, **eot, **kw)
        with pytest.raises(ValueError):
            sess.generate(ids, max_new_tokens=2, top_k=1, **eot, **kw)
        with pytest.raises(ValueError):
            sess.generate_batch(idx=[ids] * 3, max_new_tokens=2, top_k=1, **eot, **kw)
    with pytest.raises(ValueError):
        S.mmu_generate_batch(_Model(), idx=[ids] * 3, max_new_tokens=2, top_k=1, no_repeat_ngram_size=[2, 2])
    # beams take none of the four
    for kw in (dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[1, 2]]), dict(min_new_tokens=1, eot_token=5), dict(stop_sequences=[[1]])):
        with pytest.raises(ValueError):
            S.mmu_generate(_Model(), ids, max_new_tokens=2, num_beams=2, **kw)
        with pytest.raises(ValueError):
            sess.generate(ids, max_new_tokens=2, num_beams=2, **kw)


# ---- which C calls a decode makes -----------------------------------------------------------------------------------------------------------
class _Recorder:
    """stands in for the _lib module inside modeling_showo: records the entry names, launches nothing"""

    def __init__(self):
        self.names = []

    def call(self, name, *args):
        self.names.append(name)

    @staticmethod
    def ptr(t):
        return None if t is None else 0

    @staticmethod
    def stream():
        return 0


@contextlib.contextmanager
def _no_stream(model):
    yield


def _decode_names(monkeypatch, adjust, want_lp, greedy):
    mod = _mod()
    rec = _Recorder()
    monkeypatch.setattr(mod, "_lib", rec)
    monkeypatch.setattr(mod, "_graph_stream_of", _no_stream)
    logits, tok = torch.zeros(V), torch.zeros(1, dtype=torch.int64)
    draw = (True, 1, None, 1.0, None, 0) if greedy else (False, 5, 0.8, 0.9, None, 77)
    mod._decode_batch1(_Model(), None, logits, tok, 20, draw, None, want_lp, **({} if adjust is None else {"adjust": adjust}))
    return rec.names


@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("want_lp", [False, True])
def test_all_none_makes_exactly_the_c_calls_of_today(monkeypatch, want_lp, greedy):
    adjust = _mod()._adjust_of(V, no_repeat_ngram_size=None, bad_words_ids=None, min_new_tokens=None, stop_sequences=None)
    assert adjust is None
    names = _decode_names(monkeypatch, adjust, want_lp, greedy)
    loop = "showo_engine_decode_sample_lp" if want_lp else "showo_engine_decode_greedy" if greedy else "showo_engine_decode_sample_p"
    pick = ["showo_argmax_f32"] if greedy else ["showo_sample_topk_topp"]
    assert names == pick + (["showo_logprob_rows"] if want_lp else []) + [loop, loop]  # 19 tokens behind the first, in chunks of 16
    # an adjustment without rules keeps its calls too
    adjust = _mod()._adjust_of(V, repetition_penalty=1.3, repetition_context=[1, 2], no_repeat_ngram_size=None, stop_sequences=None)
    names = _decode_names(monkeypatch, adjust, want_lp, greedy)
    assert names == ["showo_seen_mark", "showo_logits_adjust"] + pick + (["showo_logprob_rows"] if want_lp else []) + \
        ["showo_engine_decode_sample_adj"] * 2


@pytest.mark.parametrize("greedy", [True, False])
def test_a_ruled_call_takes_the_seq_loop_and_stops_alone_keep_the_adj_loop(monkeypatch, greedy):
    pick = "showo_argmax_f32" if greedy else "showo_sample_topk_topp"
    adjust = _mod()._adjust_of(V, no_repeat_ngram_size=2, repetition_context=[1, 2])
    names = _decode_names(monkeypatch, adjust, False, greedy)
    assert names == ["showo_seen_mark", "showo_logits_adjust", "showo_seq_ban", pick] + ["showo_engine_decode_sample_seq"] * 2
    adjust = _mod()._adjust_of(V, stop_sequences=[[0]])  # the recorder's token is 0: the first token ends the answer
    assert _decode_names(monkeypatch, adjust, False, greedy) == ["showo_logits_adjust", pick]
    adjust = _mod()._adjust_of(V, stop_sequences=[[437, 438]])
    assert _decode_names(monkeypatch, adjust, False, greedy) == ["showo_logits_adjust", pick] + ["showo_engine_decode_sample_adj"] * 2


# ---- the slot scheduler's stop sequences ---------------------------------------------------------------------------------------------------
class _FakeSlots:
    """the engine side of _mmu_batch_schedule: request r's token d is rows[r][d]; a slot stops behind `eot`, as the device does"""

    def __init__(self, rows, slots, eot):
        self.rows, self.eot, self.occ, self.prefills, self.budgets = rows, eot, [None] * slots, [], []

    def prefill(self, s, r):
        self.prefills.append((s, r))
        self.occ[s] = r
        return self.rows[r][0]

    def decode(self, m, budget, draw0):
        self.budgets.append(list(budget))
        out, produced = [], []
        for s, b in enumerate(budget):
            row, k = [-1] * m, 0
            while k < b:
                row[k] = self.rows[self.occ[s]][draw0[s] + k]
                k += 1
                if row[k - 1] == self.eot:
                    break
            out.append(row)
            produced.append(k)
        return out, produced


def test_schedule_cuts_behind_a_stop_sequence_that_straddles_a_chunk_boundary_and_frees_the_slot():
    sched = _mod()._mmu_batch_schedule
    new, chunk, eot = 12, 4, 99
    rows = [[10 + d for d in range(new)],                    # 0: the stop (14, 15) straddles the chunks [1..4] and [5..8]
            [20, 21, 22, eot, 24, 25, 26, 27, 28, 29, 30, 31],  # 1: <eot> at 3, in front of its stop (24, 25)
            [40 + d for d in range(new)],                    # 2: no stop: runs to its budget
            [50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61]]   # 3: waits for a slot; its one-token stop is its first token
    stops = [[[14, 15]], [[24, 25]], None, [[50]]]
    eng = _FakeSlots(rows, 3, eot)
    out = sched(eng, 4, 3, new, eot, chunk=chunk, stops=stops)
    assert out == [R.stop_cut(rows[r], stops[r] or [], eot) for r in range(4)]
    assert out[0] == [10, 11, 12, 13, 14, 15] and out[1] == [20, 21, 22, eot] and len(out[2]) == new and out[3] == [50]
    # request 1 frees slot 1 at the first boundary: request 3 takes it, ends on its first token and leaves it free again
    assert eng.prefills == [(0, 0), (1, 1), (2, 2), (1, 3)]
    # request 0 retires at the second boundary: only slot 2 decodes in the third call
    assert [[b > 0 for b in bs] for bs in eng.budgets] == [[True, True, True], [True, False, True], [False, False, True]]
    # without stops the same engine gives the uncut answers (the argument has a default)
    plain = sched(_FakeSlots(rows, 3, eot), 4, 3, new, eot, chunk=chunk)
    assert plain == [R.stop_cut(rows[r], [], eot) for r in range(4)]


def test_schedule_prefers_an_earlier_eot_and_an_earlier_stop():
    sched = _mod()._mmu_batch_schedule
    eot = 99
    rows = [[1, 2, eot, 3, 4, 5, 6, 7], [1, 2, 3, eot, 5, 6, 7, 8]]
    out = sched(_FakeSlots(rows, 2, eot), 2, 2, 8, eot, chunk=16, stops=[[[2, eot, 3], [eot]], [[2, 3], [1, 2, 3, eot]]])
    assert out == [[1, 2, eot], [1, 2, 3]]
