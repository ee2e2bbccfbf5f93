"""CPU tests of nucleus (top-p) sampling: the reference restatement (tests/nucleus_ref.py) against the reference project's own
top_k_top_p_filtering and against a host emulation of the on-device arithmetic, and the Python plumbing of `top_p` on stand-in engines."""
import contextlib
import ctypes as C
import os
import types

import pytest
import torch

import util
import nucleus_ref as N
import ref_loader


def _mod():
    return util.pkg().modeling_showo


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not ref_loader.reference_available(), reason="the reference project is not on this host")
def test_kept_set_is_the_support_of_the_reference_filter():
    """inputs without a tie at the cut: ref_nucleus keeps exactly what models/sampling.py top_k_top_p_filtering leaves finite"""
    filt = ref_loader.load_reference().sampling.top_k_top_p_filtering
    for fam in N.FAMILIES:
        V, scale, k, p, T = fam
        for seed in N.cases(fam, count=3 if V > 8192 else 6):
            lg = N.family_logits(V, scale, seed)
            x = lg.float() / N._f32(T)
            keep, pk, margin = N.ref_nucleus(lg, k, p, T)
            assert int((x == x[keep].min()).sum()) == 1  # no tie at the cut (58498 normal draws do repeat a value here and there)
            out = filt(x[None].clone(), top_k=0 if k is None else k, top_p=p)
            assert torch.equal(torch.isfinite(out[0]), keep), (fam, seed, margin)
            assert abs(float(pk.sum()) - 1) < 1e-12 and bool((pk[~keep] == 0).all()) and bool(keep[x.argmax()])


def test_rule_properties_ties_top_token_and_top_k():
    """tie-inclusive at the cut, the largest token always stays, top_k first, independent of the order of the tokens"""
    lg = torch.tensor([2.0, 1.0, 1.0, 1.0, 0.0, -1.0])
    p = torch.softmax(lg.double(), -1)
    keep, pk, _ = N.ref_nucleus(lg, None, float(p[0]) + 0.01, 1.0)  # the mass above the 1.0 group is within top_p: the whole group stays
    assert keep.tolist() == [True, True, True, True, False, False]
    keep, _, _ = N.ref_nucleus(lg, None, 1e-6, 1.0)
    assert keep.tolist() == [True] + [False] * 5
    keep, _, _ = N.ref_nucleus(lg, 2, 0.999999, 1.0)  # top-2 with a tie at the 2nd value: four candidates
    assert keep.tolist() == [True, True, True, True, False, False]
    perm = torch.randperm(6, generator=torch.Generator().manual_seed(0))
    k2, _, _ = N.ref_nucleus(lg[perm], None, float(p[0]) + 0.01, 1.0)
    assert torch.equal(k2, torch.tensor([True, True, True, True, False, False])[perm])
    seed = N.tie_case()
    tl = N.family_logits(439, 3.0, seed, halves=True)
    keep, _, _ = N.ref_nucleus(tl, None, 0.9, 1.0)
    cut = tl[keep].min()
    assert int((tl == cut).sum()) >= 3 and bool(keep[tl == cut].all()) and not bool(keep[tl < cut].any())


def test_device_arithmetic_agrees_with_the_reference_above_the_margin():
    """fp32 exp + 2^40 fixed point + the double compare against the fp64 reference: the masses differ by a few 1e-7 at most (printed; the
    bound on it here is MARGIN / 10), so every case with margin >= MARGIN has the same kept set"""
    worst = 0.0
    for fam in N.FAMILIES:
        V, scale, k, p, T = fam
        for halves in (False, True):
            for seed in range(4 if V > 8192 else 24):
                lg = N.family_logits(V, scale, seed, halves)
                keep, pk, margin = N.ref_nucleus(lg, k, p, T)
                dkeep, frac = N.device_rule(lg, k, p, T)
                x = lg.float() / N._f32(T)
                cand = N._candidates(x, k)
                above = N._above(x, cand, torch.where(cand, x.double(), torch.tensor(-float("inf"), dtype=torch.float64)).softmax(-1))
                worst = max(worst, float((frac - above)[cand].abs().max()))
                if margin >= N.MARGIN:
                    assert torch.equal(keep, dkeep), (fam, halves, seed, margin)
    print(f"[nucleus] worst |device mass - reference mass| = {worst:.2e} (margin bound {N.MARGIN:.0e})")
    assert worst <= N.MARGIN / 10, worst


def test_case_selection_is_fixed_and_clear_of_the_cut():
    for fam in N.FAMILIES:
        seeds = N.cases(fam)
        assert len(seeds) == 6 and list(seeds) == sorted(seeds)
        V, scale, k, p, T = fam
        assert all(N.ref_nucleus(N.family_logits(V, scale, s), k, p, T)[2] >= N.MARGIN for s in seeds[:2])


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared():
    hdr = open(os.path.join(util.ROOT, "include", "showo_hip.h")).read()
    for name in ("showo_sample_topk_topp", "showo_engine_decode_sample_p", "showo_engine_batch_decode_sample_p"):
        assert f"int {name}(" in hdr and name in util.lib().EXPORTED_SYMBOLS
        assert hasattr(util.lib().load(), name)


def test_top_p_domain():
    M = _mod()
    assert M._nucleus_p(None) is None and M._nucleus_p(1.0) is None and M._nucleus_p(7) is None
    assert M._nucleus_p(0.25) == 0.25
    for bad in (0, 0.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            M._nucleus_p(bad)
    t = torch.zeros((1, 4), dtype=torch.int64)
    for bad in (0, -0.1, float("nan")):
        with pytest.raises(ValueError):  # raised before the engine is touched
            M.Showo.mmu_generate(object(), idx=t, top_p=bad)
        with pytest.raises(ValueError):
            M.mmu_generate_batch(object(), idx=[t, t], top_p=[0.5, bad])
    with pytest.raises(ValueError):
        M.mmu_generate_batch(object(), idx=[t, t], top_p=[0.5])
    with pytest.raises(ValueError):
        M.mmu_generate_batch(object(), idx=[t, t], top_p=[0.5, 0.6, 0.7])


class _Backend:
    """stand-in of _SessionEngine that records what `run` receives"""
    batched = False
    dev = torch.device("cpu")

    def __init__(self):
        self.rows, self.runs = 0, []

    def stamp(self):
        return ()

    def cached_rows(self):
        return self.rows

    def prefill(self, idx, input_embeddings, attention_mask):
        self.rows = idx.shape[1]
        return self.rows

    def append(self, ids, emb, Ln):
        self.rows += Ln

    def rewind(self, length):
        self.rows = length

    def use_prefix_logits(self):
        pass

    def settle(self, length, toks):
        self.rows = length + len(toks) - 1

    def run(self, max_new_tokens, greedy, k, temperature, noise, seed, eot_token, **kw):
        self.runs.append((greedy, k, seed, kw))
        return [5] * max_new_tokens


def test_session_passes_top_p_and_draws_the_same_seed():
    M = _mod()
    be = _Backend()
    s = M.MmuSession(object(), idx=torch.tensor([[1, 2, 3]]), _engine=be)
    q = torch.tensor([[9]])
    g = torch.Generator().manual_seed(3)
    s.generate(idx=q, max_new_tokens=2, top_k=5, generator=g)
    g = torch.Generator().manual_seed(3)
    s.generate(idx=q, max_new_tokens=2, top_k=5, generator=g, top_p=0.5)
    g = torch.Generator().manual_seed(3)
    s.generate(idx=q, max_new_tokens=2, top_k=5, generator=g, top_p=1.0)
    s.generate(idx=q, max_new_tokens=2, top_k=1, top_p=0.5)
    assert [r[3] for r in be.runs] == [{}, {"top_p": 0.5}, {}, {"top_p": 0.5}]
    assert be.runs[0][2] == be.runs[1][2] == be.runs[2][2]  # top_p changes no seed
    assert be.runs[3][0] is True  # top_k == 1 stays greedy
    for bad in (0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            s.generate(idx=q, max_new_tokens=2, top_p=bad)
    with pytest.raises(ValueError):
        s.generate_batch(idx=[q, q], max_new_tokens=2, top_p=[0.5])
    outs = s.generate_batch(idx=[q, q], max_new_tokens=2, top_k=5, top_p=[None, 0.25])  # not batched: generate + rewind per request
    assert len(outs) == 2 and [r[3] for r in be.runs[-2:]] == [{}, {"top_p": 0.25}]


class _FakeLib:
    """plays _lib behind _MmuSlotEngine: records the draws; a decode call emits every slot's whole budget"""

    def __init__(self):
        self.first, self.decodes = [], []

    def ptr(self, t):
        return t

    def stream(self):
        return None

    def call(self, name, *a):
        if name == "showo_argmax_f32":
            self.first.append((name, None, None))
            a[2].fill_(3)
        elif name == "showo_sample_topk":
            self.first.append((name, a[3], None))  # temperature identifies the request
            a[7].fill_(3)
        elif name == "showo_sample_topk_topp":
            self.first.append((name, a[4], a[3]))
            a[8].fill_(3)
        elif name in ("showo_engine_batch_decode_sample", "showo_engine_batch_decode_sample_p"):
            nucleus = name.endswith("_p")
            out, rest = a[3], list(a[5:])
            S = out.shape[0]
            arr = lambda v, t: [C.cast(v, C.POINTER(t))[i] for i in range(S)]
            k = arr(rest.pop(0), C.c_int)
            p = arr(rest.pop(0), C.c_float) if nucleus else [1.0] * S
            temp = arr(rest.pop(0), C.c_float)
            budget = arr(rest[3], C.c_int)
            prod = C.cast(rest[5], C.POINTER(C.c_int))
            out.fill_(-1)
            for s in range(S):
                out[s, :budget[s]] = 3
                prod[s] = budget[s]
            self.decodes.append((name, k, p, temp, budget))
        else:
            raise AssertionError(name)


class _Stream:
    def wait_stream(self, other):
        pass


def test_per_request_top_p_reaches_the_right_slot_across_refills(monkeypatch):
    M = _mod()
    fake = _FakeLib()
    monkeypatch.setattr(M, "_lib", fake)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: _Stream())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    n, slots = 11, 4
    # request r: temperature 1 + r / 64 (exact in fp32) names it; a third greedy, a third top-k only, a third with top_p
    temps = [1.0 + r / 64 for r in range(n)]
    top_ks = [1 if r % 3 == 0 else (5 if r % 3 == 1 else None) for r in range(n)]
    top_ps = [M._nucleus_p(0.5 if r % 3 == 0 else (None if r % 3 == 1 else 0.25 + r / 64)) for r in range(n)]
    seeds = [None if k == 1 else 100 + r for r, k in enumerate(top_ks)]

    class Engine(M._MmuSlotEngine):
        def fill(self, s, r):
            pass

    model = types.SimpleNamespace(vocab_size=16, decode_graph=0, _graph_stream=_Stream())
    se = Engine(model, None, None, None, None, [4] * n, slots, temps, top_ks, seeds, [None] * n, None, torch.device("cpu"), top_ps)
    # n > slots: the later requests are refilled into slots that earlier ones leave
    out = M._mmu_batch_schedule(se, n, slots, 20, None)
    assert [len(r) for r in out] == [20] * n
    by_temp = {float(torch.tensor(t, dtype=torch.float32)): r for r, t in enumerate(temps)}
    # first tokens: greedy requests take the arg-max, top_p requests the nucleus draw with their own p, the others the old call
    sampled = [r for r in range(n) if top_ks[r] != 1]
    firsts = [f for f in fake.first if f[0] != "showo_argmax_f32"]
    assert len(fake.first) == n and [by_temp[f[1]] for f in firsts] == sampled
    for name, t, p in firsts:
        r = by_temp[t]
        assert (name == "showo_sample_topk_topp") == (top_ps[r] is not None)
        if top_ps[r] is not None:
            assert p == top_ps[r]
    # decode calls: every decoding slot carries its occupant's top_p (1.0 where unset or where the slot is greedy), across the refills
    seen = set()
    for name, k, p, temp, budget in fake.decodes:
        live = [s for s in range(slots) if budget[s] > 0]
        occ = [by_temp[temp[s]] for s in live]
        want = [1.0 if top_ps[r] is None or top_ks[r] == 1 else top_ps[r] for r in occ]
        assert [p[s] for s in live] == [float(torch.tensor(w, dtype=torch.float32)) for w in want]
        assert (name == "showo_engine_batch_decode_sample_p") == any(w < 1.0 for w in want)
        assert all(p[s] == 1.0 for s in range(slots) if budget[s] == 0)
        seen.update(by_temp[temp[s]] for s in live)
    assert seen == set(range(n)) and len(fake.decodes) > 2
