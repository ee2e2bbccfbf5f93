"""CPU tests of the beam search's host side: the fp64 reference of tests/beam_ref.py against the installed transformers' beam search on
a tiny random GPT-2, the numpy restatement of the selection against a plain sort, the declarations of the new entry points and the
keyword validation of `mmu_generate` / `MmuSession.generate` (ValueError before the engine is touched)."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

import util
import beam_ref as R

NEW_ENTRY_POINTS = ("showo_beam_select", "showo_kv_permute_rows", "showo_engine_batch_beam_begin", "showo_engine_batch_decode_beam")
KEYWORDS = {"num_beams": None, "length_penalty": 1.0, "early_stopping": False, "num_return_sequences": 1, "return_beam_scores": False}


def _mod():
    return util.pkg().modeling_showo


# ---- declarations ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    flat = re.sub(r"\s+", " ", open(os.path.join(util.ROOT, "include", "showo_hip.h")).read())
    L = util.lib()
    lib = L.load()
    for name in NEW_ENTRY_POINTS:
        args = re.search(r"int " + name + r"\(([^)]*)\);", flat)
        assert args, name
        assert name in L.EXPORTED_SYMBOLS and name in L._PROTOS, name
        assert hasattr(lib, name), name
        assert len(args.group(1).split(",")) == len(L._PROTOS[name]), name
    assert "showo_kv_permute_stage_elems" in L._I64 and hasattr(lib, "showo_kv_permute_stage_elems")
    assert "beam" in open(os.path.join(util.ROOT, "show-o_amd", "csrc", "build.sh")).read().split()
    assert "## Beam search" in open(os.path.join(util.ROOT, "DESIGN.md")).read()


def test_the_keywords_exist_with_their_defaults():
    S, M = util.pkg().Showo, _mod().MmuSession
    for fn in (S.mmu_generate, M.generate):
        p = inspect.signature(fn).parameters
        for k, default in KEYWORDS.items():
            assert k in p and p[k].default == default and type(p[k].default) is type(default), (fn, k)
            assert k in (fn.__doc__ or ""), (fn, k)
    for fn in (S.mmu_generate_batch, M.generate_batch):  # beams on the batch entries are out of scope
        assert "num_beams" not in inspect.signature(fn).parameters


# ---- keyword validation ---------------------------------------------------------------------------------------------------------------------
V = 439


class _Model:
    """what the entry points read before they look at the beam keywords; engine() would touch the GPU"""
    _precision = 0
    vocab_size = V

    def engine(self):
        raise AssertionError("the engine was touched")


class _Precise(_Model):
    _precision = 1


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

    def run_beam(self, *a, **k):
        raise AssertionError("the engine was touched")

    def run(self, *a, **k):
        raise AssertionError("the engine was touched")


BAD = (dict(num_beams=0), dict(num_beams=9), dict(num_beams=-2), dict(num_beams=2.0), dict(num_beams=True),
       dict(num_beams=3, num_return_sequences=4), dict(num_return_sequences=2), dict(num_beams=1, num_return_sequences=2),
       dict(num_beams=2, num_return_sequences=0),
       dict(num_beams=2, length_penalty=float("nan")), dict(num_beams=2, length_penalty=float("inf")), dict(length_penalty=float("-inf")),
       dict(num_beams=2, early_stopping="never"), dict(num_beams=2, early_stopping=1), dict(early_stopping=None),
       dict(num_beams=2, top_k=5), dict(num_beams=2, top_k=0), dict(num_beams=2, top_p=0.9), dict(num_beams=2, top_p=1.0),
       dict(num_beams=2, temperature=0.7), dict(num_beams=2, generator=torch.Generator()), dict(num_beams=2, _exp_noise=torch.ones(2, V)),
       dict(num_beams=2, repetition_penalty=1.2), dict(num_beams=2, logit_bias={1: 0.5}), dict(num_beams=2, allowed_tokens=[1, 2, 3, 4]),
       dict(num_beams=2, banned_tokens=[1]), dict(num_beams=2, repetition_context=[1]),
       dict(return_beam_scores=True), dict(num_beams=1, return_beam_scores=True))


def _kw_id(kw):
    """a test id that is the same in every process: a tensor is 'T', a generator 'G' (its repr holds its address)"""
    show = lambda v: "T" if torch.is_tensor(v) else "G" if isinstance(v, torch.Generator) else v
    return ",".join(f"{k}={show(v)}" for k, v in kw.items())


@pytest.mark.parametrize("kw", BAD, ids=_kw_id)
def test_bad_beam_keywords_are_value_errors_before_the_engine_is_touched(kw):
    S = util.pkg().Showo
    ids = torch.tensor([[1, 2, 3]])
    sess = _mod().MmuSession(_Model(), idx=ids, _engine=_Backend())
    with pytest.raises(ValueError):
        S.mmu_generate(_Model(), ids, max_new_tokens=2, **kw)
    with pytest.raises(ValueError):
        sess.generate(ids, max_new_tokens=2, **kw)


def test_precision_one_and_an_empty_budget_have_no_beams():
    S = util.pkg().Showo
    ids = torch.tensor([[1, 2, 3]])
    with pytest.raises(ValueError):
        S.mmu_generate(_Precise(), ids, max_new_tokens=2, num_beams=2)
    with pytest.raises(ValueError):
        _mod().MmuSession(_Precise(), idx=ids, _engine=_Backend()).generate(ids, max_new_tokens=2, num_beams=2)
    with pytest.raises(ValueError):
        S.mmu_generate(_Model(), ids, max_new_tokens=0, num_beams=2)


def test_a_request_without_beams_is_none_and_with_beams_the_count():
    f = _mod()._beam_request
    rest = (4, 1.0, None, None, None, None, False)  # max_new_tokens, temperature, top_k, top_p, generator, noise, adjusted
    assert f(_Model(), None, 1.0, False, 1, False, *rest) is None
    assert f(_Model(), 1, 2.0, True, 1, False, *rest) is None
    assert f(_Model(), 8, 0, True, 8, True, 4, 1.0, 1, None, None, None, False) == 8
    assert f(_Model(), 2, -0.5, False, 1, False, *rest) == 2


# ---- the back-pointers ---------------------------------------------------------------------------------------------------------------------
def test_hypotheses_are_rebuilt_from_the_back_pointers():
    parent = np.array([[0, 0], [1, 0], [0, 0]], dtype=np.int32)
    token = np.array([[5, 6], [7, 8], [9, 10]], dtype=np.int32)
    lp = -np.arange(6, dtype=np.float32).reshape(3, 2)
    hyp = np.zeros((2, 8), dtype=np.int32)
    f = hyp.view(np.float32)
    hyp[0, :3] = (2, 1, 1); hyp[0, 4] = 3   # live beam 1 of row 2: 10 <- beam 0 of row 1 (7) <- beam 1 of row 0 (6)
    hyp[1, :3] = (2, 0, 0); hyp[1, 4] = 3   # <eot> behind live beam 0 of row 1: 7 <- 6
    f[1, 7] = -9.5
    out = _mod()._beam_hypotheses(2, parent, token, lp, hyp, 77)
    assert out[0]["tokens"] == [6, 7, 10] and out[0]["lps"].tolist() == [-1.0, -2.0, -5.0]
    assert out[1]["tokens"] == [6, 7, 77] and out[1]["lps"].tolist() == [-1.0, -2.0, -9.5]


# ---- select_ref against a plain sort ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,B,V", [(1, 1, 7), (3, 2, 16), (4, 4, 65), (8, 8, 300)])
def test_select_ref_is_the_sorted_head_of_all_scores(nb, B, V):
    rs = np.random.RandomState(nb * 100 + V)
    X = rs.standard_normal((nb, V)).astype(np.float32)
    X[0, :3] = X[0, 3]  # ties inside a row
    if nb > 1:
        X[1] = X[0]      # and across rows
    cum = np.zeros(nb, dtype=np.float32) if nb > 1 else np.array([-1.5], dtype=np.float32)
    norm = np.stack([X.max(1), np.log(np.exp(X - X.max(1, keepdims=True)).sum(1))], axis=1).astype(np.float32)
    s, b, t = R.select_ref(X, cum, norm, B)
    S = (cum[:, None] + ((X - norm[:, :1]) - norm[:, 1:])).astype(np.float32)
    want = sorted(((-float(S[i, j]), i, j) for i in range(nb) for j in range(V)))[:2 * B]
    assert [(-float(x), int(y), int(z)) for x, y, z in zip(s, b, t)] == want
    # a row without a normaliser comes last and poisons only itself
    norm[0, 1] = np.nan
    s2, b2, t2 = R.select_ref(X, cum, norm, B)
    if nb == 1:
        assert np.isnan(s2).all() and (t2 == -1).all()
    else:
        s3, b3, t3 = R.select_ref(X[1:], cum[1:], norm[1:], B)
        assert np.array_equal(s2, s3) and np.array_equal(b2, b3 + 1) and np.array_equal(t2, t3)


# ---- the fp64 reference against transformers --------------------------------------------------------------------------------------------------
HF_V, HF_PROMPT, HF_NEW, HF_SCALE = 40, [3, 17, 5, 29], 8, 4.0
# (model seed, eos): eos among the tokens the seed's beams emit (None: nothing finishes early), chosen so that over B x length_penalty x
# early_stopping hypotheses finish at rank < B, <eot> candidates are dropped at rank >= B, searches end on done before max_new -- and so
# that no <eot> of rank < B falls into the step that reaches max_new, where transformers adds that step's best B candidates to the
# finished set at once and the rule of DESIGN.md ("Beam search") lets early_stopping end the search first
HF_CASES = [(1, None), (1, 32), (2, 24), (2, 23), (3, 9)]
_HF = {}


def _hf_model(seed):
    if seed not in _HF:
        from transformers import GPT2Config, GPT2LMHeadModel

        def make():
            torch.manual_seed(seed)
            m = GPT2LMHeadModel(GPT2Config(vocab_size=HF_V, n_positions=32, n_embd=32, n_layer=2, n_head=2, bos_token_id=0,
                                           eos_token_id=None)).eval()
            with torch.no_grad():
                for p in m.parameters():
                    p.mul_(HF_SCALE)  # (the initialisation's logits are flat)
            return m

        _HF[seed] = (make(), make().double(), {})
    return _HF[seed]


@pytest.mark.parametrize("seed,eos", HF_CASES)
def test_beam_search_ref_is_transformers_beam_search(seed, eos):
    m32, m64, memo = _hf_model(seed)

    def logits_of(prefix):
        if prefix not in memo:
            with torch.no_grad():
                memo[prefix] = m64(torch.tensor([HF_PROMPT + list(prefix)])).logits[0, -1].numpy()
        return memo[prefix]

    early = dropped = before_max = 0
    for B, lp, es in itertools.product((2, 3, 4), (0, 1, 2), (True, False)):
        ref = R.beam_search_ref(logits_of, B, HF_NEW, eos, lp, es)
        finals = [h["final"] for h in ref["hyps"]]
        assert len(finals) == B and finals == sorted(finals, reverse=True)
        assert ref["gap"] > 1e-4, (B, lp, es, ref["gap"])
        assert finals[0] - finals[1] > 1e-4, (B, lp, es, finals)
        assert not ref["last_step_eot"], (B, lp, es)
        with torch.no_grad():
            out = m32.generate(torch.tensor([HF_PROMPT]), num_beams=B, do_sample=False, max_new_tokens=HF_NEW, length_penalty=float(lp),
                               early_stopping=es, eos_token_id=eos, pad_token_id=HF_V - 1, num_return_sequences=B,
                               return_dict_in_generate=True, output_scores=True)
        seqs = [s[len(HF_PROMPT):].tolist() for s in out.sequences]
        scores = out.sequences_scores.tolist()
        # sequences: all B where the finals are apart, the best one always
        for i, h in enumerate(ref["hyps"]):
            apart = all(abs(h["final"] - o["final"]) > 1e-4 for o in ref["hyps"] if o is not h)
            if i == 0 or apart:
                assert seqs[i][:h["len"]] == h["tokens"], (B, lp, es, i, seqs, ref["hyps"])
            assert abs(scores[i] - h["final"]) <= 1e-5, (B, lp, es, i, scores, finals)
        early += ref["finished_early"]
        dropped += ref["dropped"]
        before_max += ref["done_step"] < HF_NEW
    if eos is None:
        assert early == 0 and dropped == 0 and before_max == 0
    else:
        assert early > 0


def test_the_cases_cover_every_way_a_candidate_can_end():
    tot = {"finished_early": 0, "dropped": 0, "before_max": 0}
    for seed, eos in HF_CASES:
        if eos is None:
            continue
        _, m64, memo = _hf_model(seed)

        def logits_of(prefix):
            if prefix not in memo:
                with torch.no_grad():
                    memo[prefix] = m64(torch.tensor([HF_PROMPT + list(prefix)])).logits[0, -1].numpy()
            return memo[prefix]

        for B, es in itertools.product((2, 3, 4), (True, False)):
            ref = R.beam_search_ref(logits_of, B, HF_NEW, eos, 1.0, es)
            tot["finished_early"] += ref["finished_early"]
            tot["dropped"] += ref["dropped"]
            tot["before_max"] += ref["done_step"] < HF_NEW
    assert all(v > 0 for v in tot.values()), tot
