"""GPU tests of the sequence rules (no_repeat_ngram_size, bad_words_ids, min_new_tokens, stop_sequences) on the mmu decode paths: the
batch-1 loop (showo_engine_decode_sample_seq), the batched slots (showo_engine_batch_decode_sample_seq: <= 8 slots, wide slots,
shared-prefix slots), the sessions and the precision-1 recompute path.  A bias of +3000 / +2000 / +1000 on three text ids makes the
answers model-independent: they are the hand-worked table of tests/test_seq_rules_ref_cpu.py.  Without the bias the loop is held token
for token to a by-hand decode (showo_engine_decode_step, the numpy adjustment, the reference bans, the stand-alone pick)."""
import numpy as np
import pytest
import torch

import util
import logit_adjust_ref as A
import seq_rules_ref as R
from util import O, dev

pytestmark = pytest.mark.gpu

TA, TB, TC, TE = 17, 99, 250, 5  # the three text ids of the table and its <eot>
BIG = {TA: 3000.0, TB: 2000.0, TC: 1000.0}
NEW = 8

# (keywords, tokens, expected answer): the table
TABLE = [
    (dict(logit_bias=BIG, no_repeat_ngram_size=2), 6, [TA, TA, TB, TA, TC, TA]),
    (dict(logit_bias=BIG, no_repeat_ngram_size=2, repetition_context=[TA, TB]), 4, [TA, TA, TC, TA]),
    (dict(logit_bias=BIG, no_repeat_ngram_size=1), 3, [TA, TB, TC]),
    (dict(logit_bias=BIG, no_repeat_ngram_size=3), 7, [TA, TA, TA, TB, TA, TA, TC]),
    (dict(logit_bias=BIG, bad_words_ids=[[TA, TA]]), 4, [TA, TB, TA, TB]),
    (dict(logit_bias=BIG, bad_words_ids=[[TA, TA]], stop_sequences=[[TB, TA]]), 4, [TA, TB, TA]),
    (dict(logit_bias={TE: 3000.0, TB: 2000.0}, min_new_tokens=3), 8, [TB, TB, TB, TE]),
]
KEYS = ("logit_bias", "no_repeat_ngram_size", "repetition_context", "bad_words_ids", "stop_sequences", "min_new_tokens")


def _want(row, steps):
    """the answer of table row `row` for `steps` tokens: the reference's greedy answer under the bias alone"""
    kw = TABLE[row][0]
    return R.greedy(kw["logit_bias"], steps, 10 ** 6, n=kw.get("no_repeat_ngram_size", 0), bad=kw.get("bad_words_ids", ()),
                    context=kw.get("repetition_context", ()), min_new=kw.get("min_new_tokens", 0), eot=TE,
                    stops=kw.get("stop_sequences", ()))


def _check(got, row, where):
    """a request that took table row `row` for NEW tokens: the reference's answer -- all of it where the answer ends on <eot> or a stop
    sequence or fills the budget, else (every biased id is banned from there on: the model's own logits decide) its beginning"""
    want = _want(row, NEW)
    stops = TABLE[row][0].get("stop_sequences", ())
    if len(want) == NEW or want[-1] == TE or any(want[-len(s):] == s for s in stops):
        assert got == want, where
    else:
        assert got[:len(want)] == want and len(got) > len(want), where
    assert got[:TABLE[row][1]] == TABLE[row][2], where


def test_the_table_is_the_references_answer():
    for row, (kw, steps, want) in enumerate(TABLE):
        assert _want(row, steps) == want


def _tiny(precision):
    g = util.golden("showo_tiny_mmu.npz")
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd)
    m.set_precision(precision)
    return g, d, m


def _prompts(g, n):
    rs = np.random.RandomState(7)
    base = g["ids"][0].tolist()
    out = []
    for b in range(n):
        extra = rs.randint(5, 200, size=3 * b + (b % 2)).tolist()
        out.append(torch.tensor([base[:len(base) - (b % 4 if b % 2 else 0)] + extra], dtype=torch.int64))
    return out


def _ints(rows):
    return [[int(t) for t in r] for r in rows]


def _per_request(rows):
    """the per-request keyword lists of a batch whose request i takes table row rows[i] (None: no keyword at all)"""
    return {k: [None if r is None else TABLE[r][0].get(k) for r in rows] for k in KEYS}


# ---- 1. the table on every path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,recompute", [(0, False), (2, False), (3, False), (1, False), (1, True)])
def test_table_through_mmu_generate_and_a_session(precision, recompute):
    g, d, m = _tiny(precision)
    m.precise_recompute = recompute
    ids = dev(g["ids"]).to(torch.int64).contiguous()
    mask = dev(g["mask"])
    full = torch.from_numpy(g["ids"]).to(torch.int64)
    for graph in ((1, 0) if precision != 1 else (1,)):
        m.decode_graph = graph
        for row, (kw, steps, want) in enumerate(TABLE):
            call = lambda: [int(t) for t in m.mmu_generate(ids, attention_mask=mask, max_new_tokens=steps, top_k=1, eot_token=TE, **kw)]
            got = call()
            assert got == want, (precision, graph, row)
            assert call() == got  # nothing persists: a second identical call gives identical tokens
    m.decode_graph = 1
    for row, (kw, steps, want) in enumerate(TABLE):
        sess = m.mmu_session(dev(full[:, :20]), attention_mask=dev(O.mask_mmu(full[:, :20], d.eoi_id)))
        got, lps = sess.generate(dev(full[:, 20:]), max_new_tokens=steps, top_k=1, eot_token=TE, return_logprobs=True, **kw)
        assert [int(t) for t in got] == want and lps.shape[0] == len(want), (precision, row)
        assert sess.length == full.shape[1] + len(want) - 1  # settled on the cut answer, as behind an <eot>


@pytest.mark.parametrize("precision", [0, 2, 3])
def test_table_through_mmu_generate_batch_with_rules_that_differ_per_request(precision):
    """n = 3 on <= 8 slots (three batches cover the table) and, at precision 0, n = 10 on wide slots.  One request of every batch has no
    keyword: it gives the tokens of a batch without the keywords."""
    g, d, m = _tiny(precision)
    batches = [([0, None, 1], None), ([2, 3, 4], None), ([5, 6, None], None)]
    if precision == 0:
        batches.append(([0, 1, 2, 3, 4, 5, 6, None, 1, 5], 16))
    for rows, slots in batches:
        n = len(rows)
        ids = [t.cuda() for t in _prompts(g, n)]
        masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda() for t in ids]
        base = dict(idx=ids, attention_mask=masks, max_new_tokens=NEW, top_k=1, eot_token=TE, **({} if slots is None else {"slots": slots}))
        plain = _ints(m.mmu_generate_batch(**base))
        for graph in (1, 0):
            m.decode_graph = graph
            got, lps = m.mmu_generate_batch(return_logprobs=True, **base, **_per_request(rows))
            got = _ints(got)
            for b, r in enumerate(rows):
                assert lps[b].shape[0] == len(got[b])
                if r is None:
                    assert got[b] == plain[b], (precision, rows, graph, b)
                else:
                    _check(got[b], r, (precision, rows, graph, b))
        m.decode_graph = 1


def test_table_through_session_generate_batch_with_and_without_share_prefix():
    g, d, m = _tiny(0)
    P = 20
    full = torch.from_numpy(g["ids"]).to(torch.int64)
    sess = m.mmu_session(dev(full[:, :P]), attention_mask=dev(O.mask_mmu(full[:, :P], d.eoi_id)))
    rs = np.random.RandomState(3)
    for rows, variants in (([3, None, 5], [{}]), ([0, 1, 2, 3, 4, 5, 6, None, 6, 4], [dict(slots=16), dict(slots=16, share_prefix=True)])):
        n = len(rows)
        qs = [dev(torch.cat([full[:, P:P + 1 + b % 5], torch.from_numpy(rs.randint(5, 200, size=(1, b))).to(torch.int64)], dim=1)) for b in range(n)]
        for var in variants:
            plain = _ints(sess.generate_batch(idx=qs, max_new_tokens=NEW, top_k=1, eot_token=TE, **var))
            got = _ints(sess.generate_batch(idx=qs, max_new_tokens=NEW, top_k=1, eot_token=TE, **var, **_per_request(rows)))
            for b, r in enumerate(rows):
                if r is None:
                    assert got[b] == plain[b], (rows, var, b)
                else:
                    _check(got[b], r, (rows, var, b))
            assert sess.length == P


# ---- 2. the loop equals the steps, without the bias -----------------------------------------------------------------------------------------
def _pick(L, row, V, k, T, noise, step, tok):
    if k == 1:
        L.call("showo_argmax_f32", L.ptr(row), V, L.ptr(tok), L.stream())
    else:
        L.call("showo_sample_topk_topp", L.ptr(row), V, k, 1.0, T, L.ptr(noise), 0, step, L.ptr(tok), L.stream())
    return int(tok.item())


def _by_hand(m, V, ids, mask, steps, k, T, noise, beta, n, context=()):
    """`steps` tokens, their raw logits rows and how many picks the bans changed: decode_step, the numpy adjustment, the reference
    bans on the host, the stand-alone pick on the result.  None where the bans leave a row without a finite entry (no test goes there)"""
    L = util.lib()
    eng = m.engine()
    lg = torch.empty((V,), dtype=torch.float32, device="cuda")
    tok = torch.empty((1,), dtype=torch.int64, device="cuda")
    probe = torch.empty((1,), dtype=torch.int64, device="cuda")
    L.call("showo_engine_prefill", eng, L.ptr(ids), None, L.ptr(mask), ids.shape[1], L.ptr(lg), L.stream())
    hist, toks, raws, changed = list(context), [], [], 0
    for j in range(steps):
        if j:
            L.call("showo_engine_decode_step", eng, L.ptr(tok), None, L.ptr(lg), L.stream())
            hist.append(toks[-1])  # the token this step fed joins the history
        raw = lg.clone()
        y = np.array(A.adjust_ref(raw.cpu().numpy(), [], 1.0, beta))
        free = _pick(L, torch.from_numpy(y).cuda(), V, k, T, noise, j, probe)
        ban = R.banned(hist, V, n, (), len(context), 0, -1)
        if not np.isfinite(np.delete(y, sorted(ban))).any():
            return None
        y[np.array(sorted(ban), dtype=np.int64)] = -np.inf
        toks.append(_pick(L, torch.from_numpy(y).cuda(), V, k, T, noise, j, tok))
        changed += toks[-1] != free
        raws.append(raw)
    return toks, raws, changed


@pytest.mark.parametrize("precision", [0, 2])
def test_seq_loop_equals_decode_step_plus_the_reference_bans_by_hand(precision):
    g, d, m = _tiny(precision)
    L = util.lib()
    V, steps = d.vocab, 12
    ids = dev(g["ids"]).to(torch.int64).contiguous()
    mask4 = dev(g["mask"]).float().reshape(1, 1, ids.shape[1], ids.shape[1]).contiguous()
    allowed = [17, 99, 250, 201]
    beta = np.full(V, -np.inf, dtype=np.float32)
    beta[allowed] = 0.0
    for k, T in ((1, 1.0), (3, 0.9)):
        # a condition on the inputs, found with the by-hand decode alone: the bans change a pick and never use up all four ids (12
        # tokens over 4 ids can run into a token whose four successors are all taken); the sampled case looks for such a noise table
        for seed in range(2, 3 if k == 1 else 34):
            noise = None if k == 1 else dev(np.random.RandomState(seed).exponential(size=(steps, V)).astype(np.float32))
            out = _by_hand(m, V, ids, mask4, steps, k, T, noise, beta, 2)
            if out is not None and out[2] >= 1:
                break
        assert out is not None and out[2] >= 1, (precision, k)
        hand, raws, changed = out
        assert all(hand[j:j + 2] not in [hand[i:i + 2] for i in range(j)] for j in range(1, steps - 1))  # no bigram twice
        for graph in (1, 0):
            m.decode_graph = graph
            got, lps = m.mmu_generate(ids, attention_mask=dev(g["mask"]), max_new_tokens=steps, top_k=k, temperature=T, _exp_noise=noise,
                                      allowed_tokens=allowed, no_repeat_ngram_size=2, return_logprobs=True)
            assert [int(t) for t in got] == hand, (precision, k, graph)
            # log-probabilities: those of the RAW rows (showo_logprob_rows), banned or not
            want = torch.empty((steps,), dtype=torch.float32, device="cuda")
            for j in range(steps):
                L.call("showo_logprob_rows", L.ptr(raws[j]), V, 1, V, L.ptr(dev(np.array([hand[j]], dtype=np.int64))), L.ptr(want[j:j + 1]), None,
                       L.stream())
            torch.cuda.synchronize()
            assert torch.equal(lps.view(torch.int32), want.view(torch.int32)), (precision, k, graph)
        m.decode_graph = 1


# ---- 3. a batched slot gives the tokens of its batch-1 run ---------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 2, 3])
def test_a_batched_slot_gives_the_tokens_and_logprobs_of_its_batch1_seq_run(precision):
    g, d, m = _tiny(precision)
    n, V, new = 4, d.vocab, 12
    ids = [t.cuda() for t in _prompts(g, n)]
    masks = [O.mask_mmu(t.cpu(), d.eoi_id).cuda() for t in ids]
    allowed = [17, 99, 250, 201, 202, 210, 211]  # 7 ids: 12 tokens cannot use up every successor of one of them
    noise = [torch.empty((new, V), device="cuda").exponential_(1.0, generator=torch.Generator(device="cuda").manual_seed(5 + b)) for b in range(n)]
    kw = dict(allowed_tokens=[allowed, allowed, None, None], no_repeat_ngram_size=[2, 3, None, 1],
              bad_words_ids=[None, [[17, 99], [99, 17, 250]], None, None], repetition_context=[None, [17, 99], None, [201]],
              min_new_tokens=[None, None, None, 2], stop_sequences=[[[250, 17], [201, 201, 17]], None, None, None],
              top_k=[1, 3, 1, 1], temperature=[1.0, 0.8, 1.0, 1.0])
    single = []
    for b in range(n):
        one = {k: v[b] for k, v in kw.items()}
        single.append(m.mmu_generate(ids[b], attention_mask=masks[b], max_new_tokens=new, eot_token=202, _exp_noise=noise[b] if b == 1 else None,
                                     return_logprobs=True, **one))
    assert len(set(_ints([single[3][0]])[0])) == len(single[3][0])  # n = 1: no token twice
    for graph in (1, 0):
        m.decode_graph = graph
        got, lps = m.mmu_generate_batch(idx=ids, attention_mask=masks, max_new_tokens=new, eot_token=202, _exp_noise=noise,
                                        return_logprobs=True, **kw)
        for b in range(n):
            assert _ints([got[b]]) == _ints([single[b][0]]), (precision, graph, b)
            assert torch.equal(lps[b].view(torch.int32), single[b][1].view(torch.int32)), (precision, graph, b)
    m.decode_graph = 1


# ---- 4. sessions: nothing of the rules stays behind -----------------------------------------------------------------------------------------
def test_session_mark_rewind_around_a_ruled_generate_leaves_no_trace():
    g, d, m = _tiny(0)
    full = torch.from_numpy(g["ids"]).to(torch.int64)
    P = 20

    def session():
        return m.mmu_session(dev(full[:, :P]), attention_mask=dev(O.mask_mmu(full[:, :P], d.eoi_id)))

    q = dev(full[:, P:])
    fresh = session().generate(q, max_new_tokens=NEW, top_k=1, return_logprobs=True)
    sess = session()
    mark = sess.mark()
    ruled = sess.generate(q, max_new_tokens=NEW, top_k=1, no_repeat_ngram_size=1, bad_words_ids=[[int(fresh[0][0]), int(fresh[0][1])]],
                          stop_sequences=[[TA, TB]], min_new_tokens=2, eot_token=int(fresh[0][1]))
    assert [int(t) for t in ruled] != [int(t) for t in fresh[0]] and len(set(int(t) for t in ruled)) == len(ruled)
    sess.rewind(mark)
    again = sess.generate(q, max_new_tokens=NEW, top_k=1, return_logprobs=True)
    assert [int(t) for t in again[0]] == [int(t) for t in fresh[0]]
    assert torch.equal(again[1].view(torch.int32), fresh[1].view(torch.int32))
