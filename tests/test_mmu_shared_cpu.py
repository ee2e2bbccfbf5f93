"""CPU tests of shared-prefix slots' surface: the C ABI declarations and bindings, the `share_prefix` argument of
MmuSession.generate_batch (its ValueErrors and its routing to the engine side), the suffix-capacity formula, and the slot engine's
fill issuing showo_engine_batch_attach_append instead of fork + append.  The engine is a stand-in: nothing here needs a GPU."""
import inspect
import os
import re

import pytest
import torch

import util

NEW_ENTRY_POINTS = ("showo_engine_batch_begin_shared", "showo_engine_batch_attach_append", "showo_engine_batch_shared_state",
                    "showo_attn_decode_shared", "showo_attn_shared_ws_elems", "showo_kv_copy_rows")


def _mod():
    return util.pkg().modeling_showo


def test_shared_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(util.ROOT, "include", "showo_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    L = util.lib()
    lib = L.load()
    for name in NEW_ENTRY_POINTS:
        assert name in L.EXPORTED_SYMBOLS and name in L._PROTOS and hasattr(lib, name), name
        args = re.search(r"int " + name + r"\(([^)]*)\);", flat).group(1)
        assert len(args.split(",")) == len(L._PROTOS[name]), name
    assert L._PROTOS["showo_engine_batch_begin_shared"] == L._PROTOS["showo_engine_batch_begin_wide"]
    assert L._PROTOS["showo_engine_batch_attach_append"] == L._PROTOS["showo_engine_batch_prefill_append"]
    # the copy takes the fork's arguments with (r0, r1, base) in place of P
    assert len(L._PROTOS["showo_kv_copy_rows"]) == len(L._PROTOS["showo_kv_fork"]) + 2
    # the workspace size needs no GPU: 68 floats per (64-key split, head, 32 slots)
    assert lib.showo_attn_shared_ws_elems(32, 607) == 10 * 32 * 32 * 68
    assert lib.showo_attn_shared_ws_elems(2, 64) == 1 * 2 * 32 * 68 and lib.showo_attn_shared_ws_elems(2, 65) == 2 * 2 * 32 * 68
    assert lib.showo_attn_shared_ws_elems(0, 5) == 0


def test_share_prefix_argument_exists_and_defaults_to_false():
    fn = _mod().MmuSession.generate_batch
    p = inspect.signature(fn).parameters
    assert "share_prefix" in p and p["share_prefix"].default is False
    assert "share_prefix" in (fn.__doc__ or "")
    assert "share_prefix" not in inspect.signature(util.pkg().Showo.mmu_generate_batch).parameters  # unrelated prompts: out of scope
    assert _mod()._MMU_BATCH_SLOTS == 8 and (_mod()._MMU_WIDE_MIN, _mod()._MMU_WIDE_MAX) == (9, 32)


def test_suffix_capacity_formula():
    f = _mod()._shared_suffix_capacity
    # (P - base) + longest request + new tokens + 1, base = P & ~63
    assert f(607, [24, 3], 100) == (607 - 576) + 24 + 100 + 1
    assert f(64, [5], 10) == 0 + 5 + 10 + 1
    assert f(63, [5], 10) == 63 + 5 + 10 + 1
    assert f(20, [1, 9, 4], 40) == 20 + 9 + 40 + 1


class _Model:
    _precision = 0
    vocab_size = 439
    decode_graph = 1


class _Backend:
    """what MmuSession asks of its engine side, recording run_batch's arguments"""
    batched = True
    dev = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def stamp(self):
        return 1

    def cached_rows(self):
        return 70

    def prefill(self, idx, emb, mask):
        return 70

    def embed(self, token):
        raise AssertionError

    def run_batch(self, length, rows, lens, max_new_tokens, *a, **kw):
        self.calls.append((length, list(lens), max_new_tokens, dict(kw)))
        return [[1] * max_new_tokens for _ in rows]


def _session(model=None):
    be = _Backend()
    sess = _mod().MmuSession(model or _Model(), idx=torch.zeros((1, 70), dtype=torch.int64), _engine=be)
    return sess, be


def test_share_prefix_is_routed_to_the_engine_side_only_with_wide_slots():
    ids = [torch.tensor([[1, 2, 3]])] * 10
    sess, be = _session()
    sess.generate_batch(idx=ids, max_new_tokens=2, top_k=1, slots=16, share_prefix=True)
    assert be.calls[-1][3].get("slots") == 10 and be.calls[-1][3].get("share_prefix") is True
    sess.generate_batch(idx=ids, max_new_tokens=2, top_k=1, slots=16)
    assert be.calls[-1][3].get("slots") == 10 and "share_prefix" not in be.calls[-1][3]
    sess.generate_batch(idx=ids, max_new_tokens=2, top_k=1)
    assert "slots" not in be.calls[-1][3] and "share_prefix" not in be.calls[-1][3]
    # n <= 8: the call without slots / share_prefix
    sess.generate_batch(idx=ids[:8], max_new_tokens=2, top_k=1, slots=16, share_prefix=True)
    assert "slots" not in be.calls[-1][3] and "share_prefix" not in be.calls[-1][3]


def test_share_prefix_value_errors_come_before_the_engine():
    ids = [torch.tensor([[1, 2, 3]])] * 10
    sess, be = _session()
    with pytest.raises(ValueError, match="slots"):
        sess.generate_batch(idx=ids, max_new_tokens=2, top_k=1, share_prefix=True)
    with pytest.raises(ValueError, match="slots"):
        sess.generate_batch(idx=ids[:3], max_new_tokens=2, top_k=1, share_prefix=True)
    for bad in (8, 33):
        with pytest.raises(ValueError):
            sess.generate_batch(idx=ids, max_new_tokens=2, top_k=1, slots=bad, share_prefix=True)
    m = _Model()
    sess, be = _session(m)
    for precision in (1, 2, 3):
        m._precision = precision
        with pytest.raises(ValueError, match="share_prefix needs precision 0"):  # its own check, not the one `slots` makes
            sess.generate_batch(idx=ids, max_new_tokens=2, top_k=1, slots=16, share_prefix=True)
        with pytest.raises(ValueError, match="share_prefix needs precision 0"):  # also where n <= 8 would drop `slots`
            sess.generate_batch(idx=ids[:4], max_new_tokens=2, top_k=1, slots=16, share_prefix=True)
    assert be.calls == []


class _Recorder:
    """stands in for _lib.call: the names and leading integer arguments of the engine calls"""

    def __init__(self):
        self.calls = []

    def __call__(self, name, *a):
        self.calls.append((name,) + tuple(x for x in a[:4] if isinstance(x, int) and not isinstance(x, bool)))


def test_run_batch_opens_a_shared_batch_with_the_suffix_capacity_and_fill_attaches(monkeypatch):
    mod = _mod()
    rec = _Recorder()
    monkeypatch.setattr(mod._lib, "call", rec)
    monkeypatch.setattr(mod._lib, "ptr", lambda t: 0)
    monkeypatch.setattr(mod._lib, "stream", lambda: 0)
    seen = {}

    def schedule(se, n, slots, max_new_tokens, eot_token):
        seen["se"], seen["slots"] = se, slots
        for s in range(slots):
            se.fill(s, s)
        return [[7] for _ in range(n)]

    monkeypatch.setattr(mod, "_mmu_batch_schedule", schedule)
    be = mod._SessionEngine.__new__(mod._SessionEngine)
    be.model, be.eng, be.dev = _Model(), 1234, torch.device("cpu")
    n, lens = 12, [1 + b % 5 for b in range(12)]
    rows = [(torch.zeros((1, ln), dtype=torch.int64), None) for ln in lens]
    args = (70, rows, lens, 40, [1.0] * n, [1] * n, [None] * n, [None] * n, None)
    out = be.run_batch(*args, slots=12, share_prefix=True)
    assert out == [[7]] * n
    assert rec.calls[0] == ("showo_engine_batch_begin_shared", 1234, 12, (70 - 64) + 5 + 40 + 1)
    fills = rec.calls[1:]
    assert [c[0] for c in fills] == ["showo_engine_batch_attach_append"] * 12
    assert [c[2] for c in fills] == list(range(12))  # (engine, slot, ...)
    assert seen["se"].share_prefix is True
    # without share_prefix: the wide batch of whole caches, fork + append per slot
    rec.calls.clear()
    be.run_batch(*args, slots=12)
    assert rec.calls[0] == ("showo_engine_batch_begin_wide", 1234, 12, 70 + 5 + 40 + 1)
    assert [c[0] for c in rec.calls[1:]] == ["showo_engine_batch_fork", "showo_engine_batch_prefill_append"] * 12
    # share_prefix without wide slots is the narrow call
    rec.calls.clear()
    be.run_batch(*args[:1] + (rows[:4], lens[:4]) + args[3:4] + tuple(x[:4] for x in args[4:8]) + (None,), share_prefix=True)
    assert rec.calls[0][0] == "showo_engine_batch_begin"
