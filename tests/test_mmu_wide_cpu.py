"""CPU tests of the wide decode batch's surface: the C ABI declarations and bindings, the unchanged signatures of the existing
showo_engine_batch_* entries, and the `slots` argument of Showo.mmu_generate_batch / MmuSession.generate_batch (the checks that need
no GPU)."""
import inspect
import os
import re

import pytest
import torch

import util

NEW_ENTRY_POINTS = ("showo_engine_batch_begin_wide", "showo_decode_wide_ln_gemm", "showo_decode_wide_out_gemm")

# the existing batch entries, as declared before wide batches existed (whitespace-normalised)
UNCHANGED = [
    "int showo_engine_batch_begin(showo_engine* e, int nb, int cap_tokens);",
    "int showo_engine_batch_prefill(showo_engine* e, int b, const int64_t* ids, const float* embeds, const float* mask, int L, "
    "float* logits_last, void* stream);",
    "int showo_engine_batch_decode_greedy(showo_engine* e, int64_t* tok, int n_steps, int64_t* out_tokens, float* logits_ws, int use_graph, "
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
    "int showo_engine_batch_slot_ptrs(showo_engine* e, int b, uint16_t** k, uint16_t** vt, int64_t* k_lstride, int64_t* v_lstride, int* cap);",
    "int showo_engine_batch_fork(showo_engine* e, int b, void* stream);",
    "int showo_engine_batch_prefill_append(showo_engine* e, int b, const int64_t* ids, const float* embeds, int Ln, float* logits_last, "
    "void* stream);",
]


def _mod():
    return util.pkg().modeling_showo


def _header():
    return open(os.path.join(util.ROOT, "include", "showo_hip.h")).read()


def test_wide_entry_points_are_declared_bound_and_exported():
    hdr = _header()
    declared = set(re.findall(r"\b(showo_[a-z0-9_]+)\s*\(", hdr))
    L = util.lib()
    lib = L.load()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert name in L.EXPORTED_SYMBOLS and name in L._PROTOS, name
        assert hasattr(lib, name), name
    flat = re.sub(r"\s+", " ", hdr)
    assert "int showo_engine_batch_begin_wide(showo_engine* e, int nb, int cap_tokens);" in flat
    # argument counts of the bindings = those of the declarations
    for name in NEW_ENTRY_POINTS:
        args = re.search(r"int " + name + r"\(([^)]*)\);", flat).group(1)
        assert len(args.split(",")) == len(L._PROTOS[name]), name
    assert L._PROTOS["showo_engine_batch_begin_wide"] == L._PROTOS["showo_engine_batch_begin"]


def test_existing_batch_entries_keep_their_signatures():
    flat = re.sub(r"\s+", " ", _header())
    for decl in UNCHANGED:
        assert re.sub(r"\s+", " ", decl) in flat, decl


def test_slots_argument_exists_and_defaults_to_none():
    for fn in (util.pkg().Showo.mmu_generate_batch, _mod().MmuSession.generate_batch):
        p = inspect.signature(fn).parameters
        assert "slots" in p and p["slots"].default is None, fn
        assert "slots" in (fn.__doc__ or "")
    assert _mod()._MMU_BATCH_SLOTS == 8  # the narrow path's slot count is not touched


def test_slots_values_that_are_refused_or_ignored():
    f = _mod()._mmu_wide_slots
    assert f(None, 20, 0) is None and f(None, 20, 2) is None
    assert f(16, 20, 0) == 16 and f(32, 20, 0) == 20 and f(9, 9, 0) == 9
    assert f(16, 8, 0) is None and f(16, 1, 0) is None  # n <= 8: the call without `slots`
    for bad in (8, 33, 0, -1, 16.0, "16", True):
        with pytest.raises(ValueError):
            f(bad, 20, 0)
    for precision in (1, 2, 3):
        with pytest.raises(ValueError):
            f(16, 20, precision)
        with pytest.raises(ValueError):
            f(16, 4, precision)


class _Model:
    """what mmu_generate_batch reads before it looks at the slots argument"""
    _precision = 0
    vocab_size = 439


def test_entry_points_refuse_bad_slots_before_touching_the_engine():
    ids = [torch.tensor([[1, 2, 3]])] * 10
    for bad in (8, 33):
        with pytest.raises(ValueError, match="slots"):
            util.pkg().Showo.mmu_generate_batch(_Model(), idx=ids, max_new_tokens=2, top_k=1, slots=bad)
    m = _Model()
    m._precision = 2
    with pytest.raises(ValueError, match="precision 0"):
        util.pkg().Showo.mmu_generate_batch(m, idx=ids, max_new_tokens=2, top_k=1, slots=16)

    class Backend:
        batched = True
        dev = torch.device("cpu")

        def stamp(self):
            return 1

        def cached_rows(self):
            return 3

        def prefill(self, idx, emb, mask):
            return 3

        def embed(self, token):
            raise AssertionError

    sess = _mod().MmuSession(m, idx=torch.tensor([[1, 2, 3]]), _engine=Backend())
    for bad, prec in ((8, 0), (33, 0), (16, 3)):
        m._precision = prec
        with pytest.raises(ValueError):
            sess.generate_batch(idx=ids, max_new_tokens=2, top_k=1, slots=bad)
