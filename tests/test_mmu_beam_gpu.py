"""GPU tests of beam search on the mmu decode (showo_engine_batch_beam_begin / _batch_decode_beam, Showo.mmu_generate(num_beams=...),
MmuSession.generate(num_beams=...)).

The engine loop is held to a by-hand search, bit for bit: the bookkeeping of tests/beam_ref.py on the host, every logits row from the
BATCH-1 path (showo_engine_prefill + showo_engine_decode_step, each hypothesis prefix replayed, memoised) and the stand-alone
showo_beam_select as the pick.  That the batched slots reproduce those rows is the batch-1-bits contract of the batched step; that the
parent copies hand every beam its parent's rows is what makes the loop's scores equal the replayed ones."""
import numpy as np
import pytest
import torch

import util
import beam_ref as R
from util import O, dev

pytestmark = pytest.mark.gpu


def _tiny(precision):
    g = util.golden("showo_tiny_mmu.npz")
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd)
    m.set_precision(precision)
    return g, d, m


def _ints(toks):
    return [int(t) for t in toks]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Hand:
    """the batch-1 logits row behind prompt + prefix, for any prefix: prefill, then one decode step per token; memoised"""

    def __init__(self, eng, V, ids, mask):
        self.L, self.eng, self.V, self.ids, self.mask = util.lib(), eng, V, ids, mask
        self.memo = {}
        self.lg = torch.empty((V,), dtype=torch.float32, device="cuda")
        self.tok = torch.empty((1,), dtype=torch.int64, device="cuda")

    def prefill(self, lg):
        L = self.L
        L.call("showo_engine_prefill", self.eng, L.ptr(self.ids), None, L.ptr(self.mask), self.ids.shape[1], L.ptr(lg), L.stream())

    def row(self, prefix):
        prefix = tuple(int(t) for t in prefix)
        if prefix not in self.memo:
            L = self.L
            self.prefill(self.lg)
            self.memo.setdefault((), self.lg.clone())
            for j, tk in enumerate(prefix):
                self.tok.fill_(tk)
                L.call("showo_engine_decode_step", self.eng, L.ptr(self.tok), None, L.ptr(self.lg), L.stream())
                self.memo.setdefault(prefix[:j + 1], self.lg.clone())
        return self.memo[prefix]

    def search(self, B, max_new, eot, length_penalty, early_stopping):
        """beam_bookkeeping over these rows with showo_beam_select as the pick, everything in fp32; adds `lp` (per step, per live beam)"""
        L, V = self.L, self.V
        lps = []

        def pick(t, prefixes, cum):
            nb = len(prefixes)
            X = torch.stack([self.row(p) for p in prefixes]).contiguous()
            cum_d = torch.from_numpy(np.array(cum, dtype=np.float32)).cuda()
            norm = torch.empty((nb, 2), dtype=torch.float32, device="cuda")
            cand = torch.empty((2 * B, 3), dtype=torch.int32, device="cuda")
            ws = torch.empty((nb * 2 * B * 2,), dtype=torch.float32, device="cuda")
            L.call("showo_beam_select", L.ptr(X), V, nb, V, L.ptr(cum_d), B, L.ptr(norm), L.ptr(cand), L.ptr(ws), L.stream())
            c, n, x = cand.cpu().numpy(), norm.cpu().numpy(), X.cpu().numpy()
            score = c[:, 0].copy().view(np.float32)
            lps.append({(int(b), int(tk)): np.float32(np.float32(x[b, tk] - n[b, 0]) - n[b, 1]) for b, tk in zip(c[:, 1], c[:, 2])})
            return [(score[r], int(c[r, 1]), int(c[r, 2])) for r in range(2 * B)]

        def final_of(s, n):
            return np.float32(s) / np.float32(float(n) ** float(np.float32(length_penalty)))

        out = R.beam_bookkeeping(pick, B, max_new, eot, final_of, early_stopping)
        out["lp"] = [[lps[t][(b, tk)] for b, tk in zip(out["parent"][t], out["token"][t])] for t in range(len(out["parent"]))]
        out["eot_lp"] = lps
        return out


def _loop(m, hand, B, max_new, eot, length_penalty, early_stopping, graph, chunk):
    """the engine loop behind a fresh prefill, through the package's driver: (hypotheses, raw device tables)"""
    mod = util.pkg().modeling_showo
    m.decode_graph, m.beam_chunk = graph, chunk
    lg = torch.empty((hand.V,), dtype=torch.float32, device="cuda")
    hand.prefill(lg)
    tr = {}
    hyps = mod._beam_search(m, hand.eng, lg, hand.ids.shape[1], B, max_new, eot, float(length_penalty), early_stopping, lg.device, trace=tr)
    torch.cuda.synchronize()
    return hyps, tr


def _assert_loop_is_hand(hyps, tr, ref, B, max_new, what):
    n = len(ref["parent"])  # steps taken
    assert n == ref["done_step"]
    st = tr["state"]
    assert (int(st[0]), int(st[1]), int(st[2]), int(st[4]), int(st[5])) == (n, 1, B, max_new, B), (what, st[:8])
    assert np.array_equal(tr["parent"][:n], np.array(ref["parent"], dtype=np.int32)), what
    assert np.array_equal(tr["token"][:n], np.array(ref["token"], dtype=np.int32)), what
    assert np.array_equal(_bits(tr["cum"][:n]), _bits(np.array(ref["cum"], dtype=np.float32))), what
    assert np.array_equal(_bits(tr["lp"][:n]), _bits(np.array(ref["lp"], dtype=np.float32))), what
    for name in ("parent", "token", "cum", "lp"):  # behind done nothing was written (the tables start as zeros)
        assert not tr[name][n:].any(), (what, name)
    assert len(ref["hyps"]) == B and len(hyps) == B
    hyp_f = tr["hyp"].view(np.float32)
    for i, h in enumerate(ref["hyps"]):
        rec = tr["hyp"][i]
        assert (int(rec[0]), int(rec[1]), int(rec[2]), int(rec[4]), int(rec[6])) == (h["step"], h["beam"], h["kind"], h["len"], h["order"]), (what, i)
        assert _bits(hyp_f[i, 3]) == _bits(h["final"]) and _bits(hyp_f[i, 5]) == _bits(h["sumlp"]), (what, i)
        assert hyps[i]["tokens"] == [int(t) for t in h["tokens"]], (what, i)
    assert _bits(st[3:4].view(np.float32)) == _bits(ref["hyps"][-1]["final"])


def _pick_eot(hand, B, max_new):
    """a token that lets a hypothesis finish early AND ends an early-stopping search before max_new, by the by-hand search"""
    free = hand.search(B, max_new, None, 1.0, False)
    seen = []
    for row in free["token"]:
        for tk in row:
            if tk not in seen:
                seen.append(tk)
    for e in seen:
        ref = hand.search(B, max_new, e, 1.0, True)
        if ref["finished_early"] >= 1 and ref["done_step"] < max_new and ref["done_step"] >= 2:
            return e, free
    raise AssertionError("no token of the free search ends an early-stopping search before max_new")


def _setup(precision):
    g, d, m = _tiny(precision)
    ids = dev(g["ids"]).to(torch.int64).contiguous()
    mask = dev(g["mask"]).float().reshape(1, 1, ids.shape[1], ids.shape[1]).contiguous()
    return g, d, m, _Hand(m.engine(), d.vocab, ids, mask)


# ---- 1. the loop is the by-hand search ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,B,graph", [(p, B, gr) for p in (0, 2) for B in (2, 4, 8) for gr in (0, 1)] + [(3, 4, 1)])
def test_the_engine_loop_is_the_by_hand_search_bit_for_bit(precision, B, graph):
    g, d, m, hand = _setup(precision)
    T = 12
    eot, free = _pick_eot(hand, B, T)
    print(f"[beam] precision {precision} B {B}: eot {eot}")
    # (eot, length_penalty, early_stopping, max_new, chunk): chunk boundaries inside the search (3: 1 + 3 + 3 + 3 ends a 10-token search
    # on a boundary; 4: 4 + 4 + 1), one call for everything (16), done in the middle of a chunk and idle steps behind it (eot cases)
    cases = [(None, 1.0, False, 10, 3), (None, 0.0, False, 10, 4), (None, 2.0, True, 12, 16), (eot, 1.0, True, T, 16), (eot, 1.0, True, T, 2),
             (eot, 2.0, False, T, 5), (eot, 0.0, False, T, 16)]
    moved = shared = 0
    for case in cases:
        e, lp, es, max_new, chunk = case
        ref = hand.search(B, max_new, e, lp, es)
        hyps, tr = _loop(m, hand, B, max_new, e, lp, es, graph, chunk)
        _assert_loop_is_hand(hyps, tr, ref, B, max_new, case)
        if e is None:
            assert ref["done_step"] == max_new and all(h["kind"] == 1 for h in ref["hyps"])
        maps = [tuple(p) for p in ref["parent"][1:]]
        moved += sum(p != tuple(range(B)) for p in maps)
        shared += sum(len(set(p)) < B for p in maps)
    # the searches reorder their beams, and several beams take one parent: the parent copies were at work
    print(f"[beam] parent maps other than the identity: {moved}, with a shared parent: {shared}")
    assert moved >= 3 and shared >= 1
    ref = hand.search(B, T, eot, 1.0, True)
    assert ref["finished_early"] >= 1 and ref["done_step"] < T


# ---- 2. scores are the batch-1 log-probabilities -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 2])
def test_a_hypothesis_replays_through_the_batch1_path_bit_for_bit(precision):
    g, d, m, hand = _setup(precision)
    L, V, B, T = util.lib(), d.vocab, 4, 10
    eot, _ = _pick_eot(hand, B, T)
    for e, lpen in ((None, 1.0), (eot, 2.0)):
        hyps, tr = _loop(m, hand, B, T, e, lpen, False, 1, 4)
        for h in hyps:
            toks, lps = h["tokens"], h["lps"]
            assert len(toks) == h["len"] == len(lps) >= 1
            total = np.float32(0)
            for j, tk in enumerate(toks):
                row = hand.row(toks[:j])
                t1 = torch.tensor([tk], dtype=torch.int64, device="cuda")
                out = torch.empty((1,), dtype=torch.float32, device="cuda")
                L.call("showo_logprob_rows", L.ptr(row), V, 1, V, L.ptr(t1), L.ptr(out), None, L.stream())
                assert _bits(out.cpu().numpy()) == _bits(lps[j:j + 1]), (e, j)
                total = np.float32(total + lps[j])
            assert _bits(total) == _bits(np.float32(h["sumlp"]))
            assert _bits(np.float32(h["final"])) == _bits(total / np.float32(float(len(toks)) ** float(np.float32(lpen))))


# ---- 3. the Python entry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 2])
def test_mmu_generate_with_beams(precision):
    g, d, m, hand = _setup(precision)
    ids, mask = hand.ids, dev(g["mask"])
    B, T = 4, 10
    greedy = _ints(m.mmu_generate(ids, attention_mask=mask, max_new_tokens=T, top_k=1))
    for nb in (None, 1):  # no beams: the greedy call
        assert _ints(m.mmu_generate(ids, attention_mask=mask, max_new_tokens=T, top_k=1, num_beams=nb)) == greedy
    eot, _ = _pick_eot(hand, B, T)
    m.decode_graph, m.beam_chunk = 1, 16
    for e, lpen, es in ((None, 1.0, False), (eot, 1.0, True), (eot, 0.5, False)):
        ref = hand.search(B, T, e, lpen, es)
        best = m.mmu_generate(ids, attention_mask=mask, max_new_tokens=T, num_beams=B, eot_token=e, length_penalty=lpen, early_stopping=es)
        assert _ints(best) == [int(t) for t in ref["hyps"][0]["tokens"]]
        assert all(t.is_cuda for t in best)
        toks, lps, scores = m.mmu_generate(ids, attention_mask=mask, max_new_tokens=T, num_beams=B, eot_token=e, length_penalty=lpen,
                                           early_stopping=es, num_return_sequences=3, return_logprobs=True, return_beam_scores=True)
        assert [_ints(t) for t in toks] == [[int(t) for t in h["tokens"]] for h in ref["hyps"][:3]]
        assert np.array_equal(_bits(scores.cpu().numpy()), _bits(np.array([h["final"] for h in ref["hyps"][:3]], dtype=np.float32)))
        assert [len(x) for x in lps] == [len(t) for t in toks]
        s = scores.tolist()
        assert s == sorted(s, reverse=True)
        if e is not None and es:
            assert toks[0][-1].item() == e or ref["hyps"][0]["kind"] == 1
        toks1, sc1 = m.mmu_generate(ids, attention_mask=mask, max_new_tokens=T, num_beams=B, eot_token=e, length_penalty=lpen,
                                    early_stopping=es, return_beam_scores=True)
        assert _ints(toks1) == _ints(toks[0]) and sc1.shape == (1,) and sc1.item() == s[0]
    # a plain call afterwards has its usual bits
    assert _ints(m.mmu_generate(ids, attention_mask=mask, max_new_tokens=T, top_k=1)) == greedy


# ---- 4. sessions -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 2])
def test_a_session_after_a_beam_generate(precision):
    from test_mmu_session_gpu import _cache
    g, d, m = _tiny(precision)
    ids = torch.from_numpy(g["ids"]).to(torch.int64)
    pre, q = ids[:, :20], ids[:, 20:]
    sess = m.mmu_session(dev(pre), attention_mask=dev(O.mask_mmu(pre, d.eoi_id)))
    eng, P = m.engine(), sess.length
    mk = sess.mark()
    before = _ints(sess.generate(dev(q), max_new_tokens=8, top_k=1))
    sess.rewind(mk)
    k0, v0 = _cache(eng, d)
    toks, scores = sess.generate(dev(q), max_new_tokens=8, num_beams=4, return_beam_scores=True)
    toks = _ints(toks)
    assert len(toks) == 8 and scores.shape == (1,)
    assert sess.length == P + q.shape[1] + len(toks) - 1 and sess._pending == toks[-1]
    k1, v1 = _cache(eng, d)
    assert torch.equal(k1[:, :, :P], k0[:, :, :P]) and torch.equal(v1[:, :, :P], v0[:, :, :P]), "the search touched the session's prefix"
    follow = _ints(sess.generate(dev(q[:, :3]), max_new_tokens=4, top_k=1))  # a follow-up turn runs on the appended answer rows
    assert len(follow) == 4
    assert sess.length == P + q.shape[1] + len(toks) + 3 + len(follow) - 1
    s3 = m.mmu_session(dev(pre), attention_mask=dev(O.mask_mmu(pre, d.eoi_id)))
    mk3 = s3.mark()
    again = _ints(s3.generate(dev(q), max_new_tokens=8, num_beams=4))
    assert again == toks  # the same search from the same state
    s3.rewind(mk3)
    assert _ints(s3.generate(dev(q), max_new_tokens=8, top_k=1)) == before  # rewind + greedy: the bits from before
    s3.rewind(mk3)
    first = before[0]  # an <eot> the search meets at once: short answers, down to one token that appends nothing
    one = _ints(s3.generate(dev(q), max_new_tokens=8, num_beams=2, eot_token=first, early_stopping=True, num_return_sequences=1))
    assert s3.length == P + q.shape[1] + len(one) - 1 and s3._pending == one[-1]


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_state_change():
    g, d, m, hand = _setup(0)
    L, eng, V = util.lib(), hand.eng, d.vocab
    P, B = hand.ids.shape[1], 4
    ref, _ = _loop(m, hand, B, 6, None, 1.0, False, 1, 16)
    lg = torch.empty((V,), dtype=torch.float32, device="cuda")
    hand.prefill(lg)

    def tables(T):
        state = torch.zeros((64 + T + 1,), dtype=torch.int32, device="cuda")
        tr = [torch.zeros((T, B), dtype=torch.int32, device="cuda") for _ in range(4)]
        hyp = torch.zeros((B, 8), dtype=torch.int32, device="cuda")
        return state, [L.ptr(t) for t in tr] + [L.ptr(hyp)], (tr, hyp)

    def begin(T, state, tail, lp=1.0):
        L.call("showo_engine_batch_beam_begin", eng, L.ptr(state), T, L.ptr(lg), -1, lp, 0, *tail, L.stream())

    def forks(n):
        for b in range(n):
            L.call("showo_engine_batch_fork", eng, b, L.stream())

    # a wide batch
    L.call("showo_engine_batch_begin_wide", eng, B, P + 8)
    forks(B)
    state, tail, keep = tables(6)
    with pytest.raises(RuntimeError, match="code 1.*wide"):
        begin(6, state, tail)
    # slots of unequal length
    L.call("showo_engine_batch_begin", eng, B, P + 8)
    forks(B)
    one = torch.tensor([[5]], dtype=torch.int64, device="cuda")
    L.call("showo_engine_batch_prefill_append", eng, 1, L.ptr(one), None, 1, L.ptr(torch.empty_like(lg)), L.stream())
    with pytest.raises(RuntimeError, match="code 1.*unequal"):
        begin(6, state, tail)
    # capacity: more tokens than the batch's caches hold; a non-finite length penalty; a decode call on a state that was never begun
    L.call("showo_engine_batch_begin", eng, B, P + 8)
    forks(B)
    cap = (P + 8 + 63) // 64 * 64
    big = cap - P + 2
    sb, tb, kb = tables(big)
    with pytest.raises(RuntimeError, match="code 5"):
        begin(big, sb, tb)
    with pytest.raises(RuntimeError, match="code 1"):
        begin(6, state, tail, lp=float("nan"))
    ws = torch.empty((B, V), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="code 1"):
        L.call("showo_engine_batch_decode_beam", eng, L.ptr(state), 2, -1, 1.0, 0, L.ptr(ws), *tail, 1, L.stream())
    torch.cuda.synchronize()
    assert not state.any() and not sb.any() and not any(t.any() for t in keep[0]), "a refused call wrote its tables"
    # the batch still serves a search, and it is the one from before
    again, _ = _loop(m, hand, B, 6, None, 1.0, False, 1, 16)
    assert [h["tokens"] for h in again] == [h["tokens"] for h in ref] and [h["final"] for h in again] == [h["final"] for h in ref]
