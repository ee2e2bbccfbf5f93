"""CPU tests of the logit adjustment's surface: the C ABI declarations and bindings, the unchanged signatures of the existing decode
entries, the keywords of Showo.mmu_generate / mmu_generate_batch / MmuSession.generate / generate_batch, their checks (which need no
GPU), the bias-row builder, and that a call without the keywords makes none of the new C calls."""
import contextlib
import inspect
import math
import os
import re

import pytest
import torch

import util

NEW_ENTRY_POINTS = ("showo_seen_mark", "showo_logits_adjust", "showo_engine_decode_sample_adj", "showo_engine_batch_decode_sample_adj")
KEYWORDS = ("repetition_penalty", "repetition_context", "logit_bias", "allowed_tokens", "banned_tokens")

# the existing decode entries, as declared before the adjustment existed (whitespace-normalised)
UNCHANGED = [
    "int showo_engine_decode_greedy(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, int use_graph, "
    "void* stream);",
    "int showo_engine_decode_sample_lp(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, int top_k, "
    "float top_p, float temperature, const float* exp_noise, uint64_t seed, int step0, float* logprobs, int32_t* ranks, int use_graph, "
    "void* stream);",
    "int showo_engine_batch_decode_sample(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, "
    "const int* top_k, const float* temperature, const uint64_t* seed, const int* draw0, const float* const* exp_noise, "
    "const int* budget, int64_t eot, int* produced, int use_graph, void* stream);",
    "int showo_engine_batch_decode_sample_p(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, "
    "const int* top_k, const float* top_p, const float* temperature, const uint64_t* seed, const int* draw0, "
    "const float* const* exp_noise, const int* budget, int64_t eot, int* produced, int use_graph, void* stream);",
    "int showo_engine_batch_decode_sample_lp(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, "
    "const int* top_k, const float* top_p, const float* temperature, const uint64_t* seed, const int* draw0, "
    "const float* const* exp_noise, const int* budget, int64_t eot, int* produced, float* logprobs, int32_t* ranks, int use_graph, "
    "void* stream);",
    "int showo_logprob_rows(const float* logits, int64_t ld, int nrows, int V, const int64_t* targets, float* logprob, int32_t* rank, "
    "void* stream);",
    "int showo_argmax_f32(const float* x, int n, int64_t* out, void* stream);",
]
OLD_PROTO_LENGTHS = {"showo_engine_decode_greedy": 7, "showo_engine_decode_sample": 12, "showo_engine_decode_sample_p": 13,
                     "showo_engine_decode_sample_lp": 15, "showo_engine_batch_decode_sample": 15, "showo_engine_batch_decode_sample_p": 16,
                     "showo_engine_batch_decode_sample_lp": 18}


def _mod():
    return util.pkg().modeling_showo


def _flat_header():
    return re.sub(r"\s+", " ", open(os.path.join(util.ROOT, "include", "showo_hip.h")).read())


def test_entry_points_are_declared_bound_and_exported():
    flat = _flat_header()
    L = util.lib()
    lib = L.load()
    for name in NEW_ENTRY_POINTS:
        args = re.search(r"int " + name + r"\(([^)]*)\);", flat)
        assert args, name
        assert name in L.EXPORTED_SYMBOLS and name in L._PROTOS, name
        assert hasattr(lib, name), name
        assert len(args.group(1).split(",")) == len(L._PROTOS[name]), name
    # the _adj loops take everything the _lp forms take, in their order, plus the five adjustment arguments in front of use_graph
    for adj, lp in (("showo_engine_decode_sample_adj", "showo_engine_decode_sample_lp"),
                    ("showo_engine_batch_decode_sample_adj", "showo_engine_batch_decode_sample_lp")):
        a, b = L._PROTOS[adj], L._PROTOS[lp]
        assert a[:len(b) - 2] == b[:-2] and a[-2:] == b[-2:] and len(a) == len(b) + 5
        assert a[len(b) - 2:-2] == [L.c_p, L.c_i64, L.c_p, L.c_p, L.c_p]
    assert "Logit adjustment" in open(os.path.join(util.ROOT, "DESIGN.md")).read()


def test_existing_entries_keep_their_signatures():
    flat = _flat_header()
    for decl in UNCHANGED:
        assert re.sub(r"\s+", " ", decl) in flat, decl
    for name, n in OLD_PROTO_LENGTHS.items():
        assert len(util.lib()._PROTOS[name]) == n, name


def test_the_keywords_exist_and_default_to_none():
    S, M = util.pkg().Showo, _mod().MmuSession
    for fn in (S.mmu_generate, S.mmu_generate_batch, M.generate, M.generate_batch):
        p = inspect.signature(fn).parameters
        for k in KEYWORDS:
            assert k in p and p[k].default is None, (fn, k)
            assert k in (fn.__doc__ or ""), (fn, k)
    assert _mod()._ADJUST_KEYS == KEYWORDS


# ---- the request builder -----------------------------------------------------------------------------------------------------------------
V = 439
NEG = float("-inf")


def test_all_none_and_penalty_one_are_no_adjustment():
    f = _mod()._adjust_of
    assert f(V) is None
    assert f(V, repetition_penalty=1.0) is None and f(V, repetition_penalty=1, repetition_context=[1, 2]) is None
    assert f(V, logit_bias={}) is None and f(V, logit_bias={3: 0.0}, banned_tokens=[]) is None
    a = f(V, repetition_penalty=1.3, repetition_context=torch.tensor([[5, 7, 5]]))
    assert a.theta == 1.3 and a.bias is None and a.context == [5, 7, 5]
    assert f(V, repetition_penalty=1.0, banned_tokens=[4]).theta == 1.0


def test_bias_row_combines_dict_allowed_and_banned():
    f = _mod()._bias_row
    assert f(V) is None
    row = f(V, logit_bias={3: 1.5, 7: -2.0, 9: NEG})
    assert row.dtype == torch.float32 and tuple(row.shape) == (V,)
    assert row[3] == 1.5 and row[7] == -2.0 and row[9] == NEG and int((row != 0).sum()) == 3
    row = f(V, logit_bias={3: 1.5, 20: 0.25}, allowed_tokens=(3, 4, 5, 9), banned_tokens={4})
    want = torch.full((V,), NEG)
    want[3], want[5], want[9] = 1.5, 0.0, 0.0
    assert torch.equal(row, want)  # 20 is outside the allowed set: its bias is gone; 4 is allowed and banned: banned
    t = torch.zeros(V)
    t[11] = NEG
    t[12] = 3.0
    row = f(V, logit_bias=t, banned_tokens=torch.tensor([12]))
    assert row[11] == NEG and row[12] == NEG and int(torch.isinf(row).sum()) == 2 and t[12] == 3.0  # the caller's tensor is not written
    assert f(V, logit_bias=torch.zeros(V, dtype=torch.float64), allowed_tokens=range(V)) is None  # changes nothing


@pytest.mark.parametrize("kw", [
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1.3), dict(repetition_penalty=float("nan")),
    dict(repetition_penalty=float("inf")), dict(repetition_penalty=1.2, repetition_context=[V]),
    dict(repetition_penalty=1.2, repetition_context=[-1]), dict(repetition_context=[1.5], repetition_penalty=1.2),
    dict(logit_bias={V: 1.0}), dict(logit_bias={-1: 1.0}), dict(logit_bias={3: float("inf")}), dict(logit_bias={3: float("nan")}),
    dict(logit_bias=torch.zeros(V + 1)), dict(logit_bias=torch.full((V,), float("inf"))), dict(banned_tokens=[V]),
    dict(allowed_tokens=[-2]), dict(allowed_tokens=[]), dict(allowed_tokens=[3], banned_tokens=[3]),
    dict(allowed_tokens=[3, 4], logit_bias={3: NEG, 4: NEG}), dict(banned_tokens=list(range(V))),
])
def test_bad_requests_are_value_errors(kw):
    with pytest.raises(ValueError):
        _mod()._adjust_of(V, **kw)


def test_per_request_values_shared_and_listed():
    f = _mod()._adjust_per_request
    assert f(3, V) == (None, [{}, {}, {}])
    assert f(3, V, repetition_penalty=1.0)[0] is None
    adj, kws = f(3, V, repetition_penalty=1.2, banned_tokens=[4, 5])  # shared: ONE request object, one dense row
    assert adj[0] is adj[1] is adj[2] and adj[0].theta == 1.2 and adj[0].bias[4] == NEG
    assert kws[1] == dict(repetition_penalty=1.2, banned_tokens=[4, 5])
    ctx = [[1, 2], None, torch.tensor([7])]
    adj, kws = f(3, V, repetition_penalty=[1.2, 1.0, 0.5], repetition_context=ctx, allowed_tokens=[None, None, (7, 8)])
    assert adj[1] is None and adj[0].context == [1, 2] and adj[0].bias is None
    assert adj[2].theta == 0.5 and adj[2].context == [7] and int(torch.isfinite(adj[2].bias).sum()) == 2
    assert kws[1] == dict(repetition_penalty=1.0) and set(kws[2]) == {"repetition_penalty", "repetition_context", "allowed_tokens"}
    adj, _ = f(2, V, logit_bias=[{3: 1.0}, None])
    assert adj[0].bias[3] == 1.0 and adj[1] is None
    for bad in (dict(repetition_penalty=[1.2, 1.3]), dict(repetition_context=[[1], [2]], repetition_penalty=1.2), dict(logit_bias=[{}])):
        with pytest.raises(ValueError):
            f(3, V, **bad)


# ---- the entry points refuse before they touch the engine --------------------------------------------------------------------------------
class _Model:
    """what the entry points read before they look at the adjustment keywords; engine() would touch the GPU"""
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


BAD = (dict(repetition_penalty=0.0), dict(repetition_penalty=float("nan")), dict(banned_tokens=[V]), dict(logit_bias={1: float("inf")}),
       dict(allowed_tokens=[]), dict(repetition_penalty=1.1, repetition_context=[-1]))


def test_entry_points_refuse_bad_keywords_before_touching_the_engine():
    S = util.pkg().Showo
    ids = torch.tensor([[1, 2, 3]])
    sess = _mod().MmuSession(_Model(), idx=ids, _engine=_Backend())
    for kw in BAD:
        with pytest.raises(ValueError):
            S.mmu_generate(_Model(), ids, max_new_tokens=2, top_k=1, **kw)
        with pytest.raises(ValueError):
            S.mmu_generate_batch(_Model(), idx=[ids] * 3, max_new_tokens=2, top_k=1, **kw)
        with pytest.raises(ValueError):
            sess.generate(ids, max_new_tokens=2, top_k=1, **kw)
        with pytest.raises(ValueError):
            sess.generate_batch(idx=[ids] * 3, max_new_tokens=2, top_k=1, **kw)
    with pytest.raises(ValueError):
        S.mmu_generate_batch(_Model(), idx=[ids] * 3, max_new_tokens=2, top_k=1, repetition_penalty=[1.1, 1.2])


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


NEW_CALLS = set(NEW_ENTRY_POINTS)


@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("want_lp", [False, True])
def test_a_call_without_the_keywords_makes_no_new_c_call(monkeypatch, want_lp, greedy):
    names = _decode_names(monkeypatch, None, want_lp, greedy)
    assert names and not (set(names) & NEW_CALLS)
    loop = "showo_engine_decode_sample_lp" if want_lp else "showo_engine_decode_greedy" if greedy else "showo_engine_decode_sample_p"
    assert names.count(loop) == 2  # 19 tokens behind the first one, in chunks of 16


@pytest.mark.parametrize("greedy", [True, False])
def test_an_adjusted_call_takes_the_adj_loop(monkeypatch, greedy):
    adj = _mod()._adjust_of(V, repetition_penalty=1.3, repetition_context=[1, 2], banned_tokens=[5])
    names = _decode_names(monkeypatch, adj, False, greedy)
    assert names[0] == "showo_seen_mark" and names[1] == "showo_logits_adjust"  # the context, then the prefill logits
    assert names.count("showo_engine_decode_sample_adj") == 2
    assert not {"showo_engine_decode_greedy", "showo_engine_decode_sample", "showo_engine_decode_sample_p", "showo_engine_decode_sample_lp"} & set(names)


def test_session_passes_the_request_on_only_when_there_is_one():
    seen = []

    class Backend(_Backend):
        def append(self, ids, emb, Ln):
            pass

        def rewind(self, length):
            pass

        def settle(self, length, toks):
            pass

        def run(self, max_new_tokens, greedy, k, temperature, noise, seed, eot_token, **kw):
            seen.append(kw)
            return [4, 5]

    ids = torch.tensor([[1, 2, 3]])
    for kw in ({}, dict(repetition_penalty=1.0), dict(repetition_penalty=1.3, repetition_context=[4])):
        sess = _mod().MmuSession(_Model(), idx=ids, _engine=Backend())
        assert [int(t) for t in sess.generate(ids, max_new_tokens=2, top_k=1, **kw)] == [4, 5]
    assert seen[0] == {} and seen[1] == {}
    assert set(seen[2]) == {"adjust"} and math.isclose(seen[2]["adjust"].theta, 1.3) and seen[2]["adjust"].context == [4]
