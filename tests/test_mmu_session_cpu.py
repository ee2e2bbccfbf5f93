"""CPU tests of mmu sessions (Showo.mmu_session): the split condition, the interval rule of appended rows, and the session's host-side
bookkeeping (pending token, mark / rewind, staleness) on a stand-in of the engine side, in the style of test_mmu_batch_sched_cpu.py."""
import os
import re

import numpy as np
import pytest
import torch

import util
from util import O


def _P():
    return util.pkg().prompting_utils


def _mod():
    return util.pkg().modeling_showo


# ---- mmu_prefix_is_exact ----------------------------------------------------------------------------------------------------------------
def test_prefix_is_exact_for_the_mmu_vit_mask_behind_the_image():
    mask = O.mask_mmu_vit(1, 631, system_prompt_len=28)
    f = _P().mmu_prefix_is_exact
    assert f(mask, 607) and f(mask, 620)
    assert f(mask == 0, 607)            # bool form (return_inverse_mask=False)
    assert f(mask, 606)                 # the first split the issue's arithmetic allows
    assert not f(mask, 605) and not f(mask, 300)   # inside the image: later image columns are visible to the prefix
    assert not f(mask, 0) and not f(mask, 631)


def test_prefix_is_exact_for_the_mmu_mask_behind_eoi_only():
    g = util.golden("showo_tiny_mmu.npz")
    d = util.tiny_dims()
    ids = torch.from_numpy(g["ids"]).to(torch.int64)
    assert ids.shape[1] == 25 and int((ids[0] == d.eoi_id).nonzero()[0]) == 18
    mask = O.mask_mmu(ids, d.eoi_id)
    assert torch.equal(mask, torch.from_numpy(g["mask"]).to(mask.dtype).reshape(mask.shape))
    f = _P().mmu_prefix_is_exact
    assert f(mask, 19) and f(mask, 20) and f(mask, 22)
    assert not f(mask, 18)  # the split is inside the image: row 17 sees <eoi> at column 18


def test_prefix_is_not_exact_for_a_t2i_mask_split_in_the_text():
    d = util.tiny_dims()
    T = d.max_text_len + 1
    row = [d.pad_id] * (T - 6) + [d.t2i_id] + list(range(10, 14)) + [d.soi_id] + [d.mask_token_id] * d.num_vq_tokens + [d.eoi_id]
    mask = O.mask_t2i(torch.tensor([row]), d.pad_id, d.soi_id, d.eoi_id)
    f = _P().mmu_prefix_is_exact
    for P in (T - 4, T - 2):
        assert not f(mask, P)


# ---- the interval rule of appended rows -------------------------------------------------------------------------------------------------
def append_rows_np(last_iv, L0, P, Ln):
    """the rule of showo_mask_append_rows: row j = the decode row of position P + j"""
    out = np.zeros((Ln, 4), dtype=np.int32)
    for j in range(Ln):
        a, b, c, d = (int(v) for v in last_iv)
        if b == L0 and a < b:
            b = P + j + 1
        elif d == L0 and c < d:
            d = P + j + 1
        elif not c < d:
            c, d = L0, P + j + 1
        elif not a < b:
            a, b = L0, P + j + 1
        else:
            raise ValueError("more than two intervals")
        out[j] = (a, b, c, d)
    return out


def _runs(vis_row):
    """(lo1, hi1, lo2, hi2) of a boolean row with at most two runs"""
    idx = np.flatnonzero(vis_row)
    cuts = np.flatnonzero(np.diff(idx) > 1)
    assert len(cuts) <= 1
    if len(cuts) == 0:
        return (int(idx[0]), int(idx[-1]) + 1, 0, 0)
    return (int(idx[0]), int(idx[cuts[0]]) + 1, int(idx[cuts[0] + 1]), int(idx[-1]) + 1)


def _dense_of(iv, L):
    col = np.arange(L)[None, :]
    return ((col >= iv[:, 0:1]) & (col < iv[:, 1:2])) | ((col >= iv[:, 2:3]) & (col < iv[:, 3:4]))


@pytest.mark.parametrize("family,L0,L", [("vit", 607, 631), ("vit", 620, 631), ("gap", 10, 29), ("mmu", 19, 25), ("mmu", 22, 25)])
def test_append_rule_reproduces_the_dense_rows(family, L0, L):
    """prefix of L0 rows, everything behind it appended in one or in two blocks: the rule gives the dense rows L0 .. L-1 of the full
    mask.  "gap": causal rows that do not see the columns [3, 7) (a hidden pad block) -- the last prefix row has two runs, [0, 3) and
    [7, L0), and the rule extends the second."""
    if family == "vit":
        full = (O.mask_mmu_vit(1, 631, system_prompt_len=28)[0, 0] == 0).numpy()
    elif family == "gap":
        full = np.tril(np.ones((L, L), dtype=bool))
        full[7:, 3:7] = False
        assert _P().mmu_prefix_is_exact(torch.from_numpy(full), L0)
    else:
        g = util.golden("showo_tiny_mmu.npz")
        full = (O.mask_mmu(torch.from_numpy(g["ids"]).to(torch.int64), util.tiny_dims().eoi_id)[0, 0] == 0).numpy()
    width = full.shape[1]
    last = _runs(full[L0 - 1, :L0])  # what the prefill of the prefix alone leaves as its last row
    if family == "gap":
        assert last == (0, 3, 7, L0)
    rows = append_rows_np(last, L0, L0, L - L0)
    assert np.array_equal(_dense_of(rows, width)[:, :L], full[L0:L, :L])
    a = (L - L0) // 2
    two = np.concatenate([append_rows_np(last, L0, L0, a), append_rows_np(last, L0, L0 + a, L - L0 - a)]) if a else rows
    assert np.array_equal(two, rows)
    with pytest.raises(ValueError):
        append_rows_np((0, 3, 5, 9), 12, 12, 1)


# ---- the session's bookkeeping on a stand-in engine ------------------------------------------------------------------------------------
class FakeBackend:
    """plays _SessionEngine: the 'cache' is the list of token ids fed so far, the next token a deterministic function of it"""
    batched = False
    dev = torch.device("cpu")

    def __init__(self, eot=None, stop_after=None):
        self.cache, self.epoch, self.eot, self.stop_after = [], 0, eot, stop_after
        self.appended, self.rewinds = [], []

    def stamp(self):
        return ("engine", self.epoch)

    def cached_rows(self):
        return len(self.cache)

    def prefill(self, idx, input_embeddings, attention_mask):
        self.cache = idx[0].tolist()
        self.epoch += 1
        return len(self.cache)

    def embed(self, token):
        return torch.full((1, 1, 4), float(token))

    def use_prefix_logits(self):
        pass

    def append(self, ids, emb, Ln):
        rows = ids[0].tolist() if ids is not None else [int(v) for v in emb[0, :, 0].tolist()]
        assert len(rows) == Ln
        self.appended.append(rows)
        self.cache += rows

    def rewind(self, length):
        assert length <= len(self.cache)
        self.rewinds.append(length)
        del self.cache[length:]

    def next(self, cache):
        return (sum(cache) * 7 + len(cache)) % 1000 + 1000

    def run(self, max_new_tokens, greedy, k, temperature, noise, seed, eot_token):
        out = [self.next(self.cache)]
        while len(out) < max_new_tokens and not (eot_token is not None and out[-1] == eot_token):
            self.cache.append(out[-1])
            out.append(self.next(self.cache))
        # like the device loop, a chunk may run past the <eot>: the cache then holds rows the session must drop
        if eot_token is not None and out[-1] == eot_token:
            self.cache += [out[-1], 1, 2]
        return out

    def settle(self, length, toks):
        self.rewind(length + len(toks) - 1)


def _session(prefix, **kw):
    be = FakeBackend(**kw)
    s = _mod().MmuSession(object(), idx=torch.tensor([prefix]), _engine=be)
    return s, be


def _ints(toks):
    return [int(t) for t in toks]


def test_pending_token_is_fed_in_front_of_the_next_rows():
    s, be = _session([1, 2, 3, 4, 5])
    assert s.length == s.prefix_length == 5 and s.mark() == (5, None)
    a1 = _ints(s.generate(idx=torch.tensor([[10, 11]]), max_new_tokens=4, top_k=1))
    assert len(a1) == 4
    assert be.appended == [[10, 11]]
    assert be.cache == [1, 2, 3, 4, 5, 10, 11] + a1[:-1] and s.length == 7 + 3
    assert s.mark() == (10, a1[-1])
    # next call: pending token first, then the caller's rows
    a2 = _ints(s.generate(idx=torch.tensor([[20]]), max_new_tokens=2, top_k=1))
    assert be.appended[-1] == [a1[-1], 20]
    assert be.cache == [1, 2, 3, 4, 5, 10, 11] + a1 + [20] + a2[:-1] and s.length == len(be.cache)
    # embeddings: the pending token goes through embed() first
    a3 = _ints(s.generate(input_embeddings=torch.full((1, 2, 4), 33.0), max_new_tokens=1, top_k=1))
    assert be.appended[-1] == [a2[-1], 33, 33] and len(a3) == 1
    # no rows: the pending token alone continues the answer
    n = s.length
    a4 = _ints(s.generate(max_new_tokens=3, top_k=1))
    assert be.appended[-1] == [a3[-1]] and s.length == n + 1 + 2 and len(a4) == 3


def test_continuing_equals_one_longer_answer():
    s, _ = _session([1, 2, 3])
    whole = _ints(s.generate(idx=torch.tensor([[9]]), max_new_tokens=7, top_k=1))
    s, _ = _session([1, 2, 3])
    parts = _ints(s.generate(idx=torch.tensor([[9]]), max_new_tokens=3, top_k=1))
    parts += _ints(s.generate(max_new_tokens=4, top_k=1))
    assert parts == whole


def test_mark_and_rewind_restore_length_and_pending_token():
    s, be = _session([1, 2, 3, 4])
    m0 = s.mark()
    a = _ints(s.generate(idx=torch.tensor([[7, 8]]), max_new_tokens=3, top_k=1))
    m1 = s.mark()
    assert m1 == (4 + 2 + 2, a[-1])
    b = _ints(s.generate(idx=torch.tensor([[5]]), max_new_tokens=5, top_k=1))
    s.rewind(m1)
    assert s.mark() == m1 and be.cache == [1, 2, 3, 4, 7, 8] + a[:-1]
    assert _ints(s.generate(idx=torch.tensor([[5]]), max_new_tokens=5, top_k=1)) == b  # the same continuation again
    s.rewind(m0)
    assert s.length == 4 and be.cache == [1, 2, 3, 4]
    assert _ints(s.generate(idx=torch.tensor([[7, 8]]), max_new_tokens=3, top_k=1)) == a
    # refused, state unchanged: below the prefix, above the length, a non-prefix state without its pending token
    before = (s.mark(), list(be.cache))
    for bad in ((3, None), (s.length + 1, 5), (s.length, None)):
        with pytest.raises(ValueError):
            s.rewind(bad)
        assert (s.mark(), list(be.cache)) == before


def test_eot_cut_drops_what_the_device_loop_ran_past_it():
    s, be = _session([1, 2, 3])
    free = _ints(s.generate(idx=torch.tensor([[4]]), max_new_tokens=6, top_k=1))
    eot = free[2]
    s, be = _session([1, 2, 3])
    got = _ints(s.generate(idx=torch.tensor([[4]]), max_new_tokens=6, top_k=1, eot_token=eot))
    assert got == free[:3]
    assert be.cache == [1, 2, 3, 4] + got[:-1] and s.length == 6 and s.mark() == (6, eot)


def test_generate_batch_without_batched_engine_is_generate_plus_rewind_and_leaves_the_session_alone():
    s, be = _session([1, 2, 3])
    a = _ints(s.generate(idx=torch.tensor([[4]]), max_new_tokens=2, top_k=1))
    state = (s.mark(), list(be.cache))
    qs = [torch.tensor([[5, 6]]), torch.tensor([[7]]), torch.tensor([[8, 9, 10]])]
    outs = [_ints(r) for r in s.generate_batch(idx=qs, max_new_tokens=4, top_k=1)]
    assert (s.mark(), list(be.cache)) == state
    want = []
    for q in qs:
        mk = s.mark()
        want.append(_ints(s.generate(idx=q, max_new_tokens=4, top_k=1)))
        s.rewind(mk)
    assert outs == want and be.appended[-1][0] == a[-1]


def test_a_stale_session_raises_and_does_not_touch_the_cache():
    s, be = _session([1, 2, 3])
    s.generate(idx=torch.tensor([[4]]), max_new_tokens=2, top_k=1)
    mk = s.mark()
    be.epoch += 1  # somebody else prefilled the engine's decode cache (mmu_generate, a newer session)
    cache = list(be.cache)
    for call in (lambda: s.generate(idx=torch.tensor([[5]]), max_new_tokens=2, top_k=1),
                 lambda: s.generate_batch(idx=[torch.tensor([[5]]), torch.tensor([[6]])], max_new_tokens=2, top_k=1),
                 lambda: s.rewind(mk)):
        with pytest.raises(RuntimeError, match="stale"):
            call()
    assert be.cache == cache


def test_a_generate_that_fails_midway_is_undone_and_a_cache_out_of_step_is_refused():
    s, be = _session([1, 2, 3])
    s.generate(idx=torch.tensor([[4]]), max_new_tokens=2, top_k=1)
    state = (s.mark(), list(be.cache))
    run = be.run

    def failing(*a, **kw):
        be.cache += [7, 7, 7]  # the device loop wrote rows, then ran into the end of the cache
        raise RuntimeError("cache full")
    be.run = failing
    with pytest.raises(RuntimeError, match="cache full"):
        s.generate(idx=torch.tensor([[5, 6]]), max_new_tokens=4, top_k=1)
    assert (s.mark(), list(be.cache)) == state  # the appended rows and the loop's rows are gone, the pending token is kept
    be.run = run
    a = _ints(s.generate(idx=torch.tensor([[5, 6]]), max_new_tokens=4, top_k=1))
    s2, be2 = _session([1, 2, 3])
    s2.generate(idx=torch.tensor([[4]]), max_new_tokens=2, top_k=1)
    assert _ints(s2.generate(idx=torch.tensor([[5, 6]]), max_new_tokens=4, top_k=1)) == a
    # a cache that moved without the session (the undo itself failed) is never appended to at the wrong position
    be.cache.append(9)
    with pytest.raises(RuntimeError, match="out of step"):
        s.generate(idx=torch.tensor([[5]]), max_new_tokens=2, top_k=1)
    assert be.cache[-1] == 9


def test_a_backend_that_lost_its_engine_reports_stale():
    s, be = _session([1, 2, 3])
    be.stamp = lambda: None  # _SessionEngine.stamp() once the model dropped the engine
    with pytest.raises(RuntimeError, match="stale"):
        s.generate(idx=torch.tensor([[5]]), max_new_tokens=2, top_k=1)


def test_argument_checks():
    s, _ = _session([1, 2, 3])
    with pytest.raises(ValueError):
        s.generate(idx=torch.tensor([[4]]), input_embeddings=torch.zeros(1, 1, 4))
    with pytest.raises(ValueError):
        s.generate(idx=torch.tensor([[4]]), max_new_tokens=0)
    with pytest.raises(ValueError):
        s.generate(idx=torch.tensor([[4]]), temperature=0.0, top_k=5)
    with pytest.raises(ValueError):
        _mod().MmuSession(object(), idx=torch.tensor([[1, 2], [3, 4]]), _engine=FakeBackend())
    with pytest.raises(ValueError):
        _mod().MmuSession(object(), _engine=FakeBackend())


# ---- C ABI surface ------------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = ("showo_mask_append_rows", "showo_kv_fork", "showo_engine_prefill_append", "showo_engine_cache_rewind",
                    "showo_engine_cache_state", "showo_engine_cache_ptrs", "showo_engine_batch_slot_ptrs", "showo_engine_batch_fork",
                    "showo_engine_batch_prefill_append")


def test_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(util.ROOT, "include", "showo_hip.h")).read()
    declared = set(re.findall(r"\b(showo_[a-z0-9_]+)\s*\(", hdr))
    L = util.lib()
    lib = L.load()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert name in L.EXPORTED_SYMBOLS and name in L._PROTOS, name
        assert hasattr(lib, name), name
    assert re.search(r"int showo_engine_prefill_append\(showo_engine\* e, const int64_t\* ids, const float\* embeds, int Ln, float\* logits_last,\s*void\* stream\);", hdr)
    assert re.search(r"int showo_engine_cache_rewind\(showo_engine\* e, int len, void\* stream\);", hdr)
    assert hasattr(util.pkg().Showo, "mmu_session") and hasattr(_mod().MmuSession, "generate_batch")
    assert "mmu_prefix_is_exact" in (util.pkg().Showo.mmu_session.__doc__ or "")


def test_host_side_refusals_need_no_gpu():
    """null handles and bad arguments are refused with an error code and a message before anything is launched"""
    import ctypes as C
    L = util.lib()
    lib = L.load()
    assert lib.showo_engine_prefill_append(None, None, None, 1, None, None) == 1
    assert lib.showo_engine_cache_rewind(None, 0, None) == 1
    assert lib.showo_engine_batch_fork(None, 0, None) == 1
    assert lib.showo_engine_batch_prefill_append(None, 0, None, None, 1, None, None) == 1
    iv = (C.c_int32 * 4)(0, 3, 5, 9)
    assert lib.showo_mask_append_rows(C.cast(iv, C.c_void_p), 12, 12, 1, C.c_void_p(16), None) == 6
    assert b"two intervals" in lib.showo_last_error()
    assert lib.showo_kv_fork(C.c_void_p(16), C.c_void_p(16), 100, 0, 0, C.c_void_p(16), C.c_void_p(16), 64, 0, 0, 1, 1, 1, None) == 1
    assert lib.showo_kv_fork(C.c_void_p(16), C.c_void_p(16), 128, 128 * 64, 128 * 64, C.c_void_p(16), C.c_void_p(16), 64, 64 * 64, 64 * 64,
                             1, 1, 65, None) == 5
