"""CPU: the fp64 reference of the log-probability kernel (tests/logprob_ref.py) against torch, the gate's headroom, and the host-side
surface of the feature (exports, prototypes, Python signatures)."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

import util
import logprob_ref as R


@pytest.mark.parametrize("V", R.SHAPES_V)
def test_reference_equals_torch_log_softmax_and_a_brute_force_rank(V):
    for kind in ("normal", "plus1e4", "minus1e4", "neginf", "equal", "ties"):
        X, T = R.make_case(kind, V, 3, seed=1)
        lp, rk = R.logprob_rows_ref(X, T)
        want = torch.log_softmax(torch.from_numpy(X).double(), -1).gather(1, torch.from_numpy(T)[:, None])[:, 0].numpy()
        for r in range(3):
            brute = sum(1 for i in range(V) if X[r, i] > X[r, T[r]]) if V <= 4099 else int((X[r] > X[r, T[r]]).sum())
            assert rk[r] == brute, (kind, r)
            if np.isneginf(want[r]):
                assert np.isneginf(lp[r]), (kind, r)
            else:
                assert abs(lp[r] - want[r]) <= 1e-12 * max(1.0, abs(want[r])), (kind, r, lp[r], want[r])
        if kind == "equal":
            assert np.allclose(lp, -math.log(V), rtol=0, atol=1e-12) and (rk == 0).all()
        if kind == "ties" and V >= 3:
            for r in range(3):  # the two copies of the target's value are not counted: the rank is that of the value
                assert (X[r] == X[r, T[r]]).sum() >= 3 and rk[r] == int((X[r] > X[r, T[r]]).sum())
        if kind == "neginf" and V >= 7:
            assert np.isneginf(lp).any() and np.isfinite(lp).any()


def test_special_targets():
    x = np.array([0.5, -1.0, 2.0], dtype=np.float32)
    assert R.logprob_ref(x, -100) == (0.0, -1) and R.logprob_ref(x, -1) == (0.0, -1)
    lp, rk = R.logprob_ref(x, 3)
    assert math.isnan(lp) and rk == -1
    lp, rk = R.logprob_ref(np.full(4, -np.inf), 1)
    assert math.isnan(lp)
    assert R.logprob_ref(x, 2)[1] == 0 and R.logprob_ref(x, 1)[1] == 2
    X, T = R.make_case("ignore", 7, 3)
    assert (T == -100).all()
    X, T = R.make_case("beyond", 7, 3)
    assert (T == 7).all()
    got = np.array([0.0, np.nan, -np.inf, 1.0], dtype=np.float32)
    assert R.within_gate(got, np.array([0.0, np.nan, -np.inf, 1.0])).all()
    assert not R.within_gate(got, np.array([1e-3, 0.0, 0.0, np.nan])).any()


@pytest.mark.parametrize("V", R.SHAPES_V)
def test_fp32_log_softmax_stays_inside_the_kernel_gate(V):
    """the gate is derived from fp32 rounding: the fp32 reference itself (torch.log_softmax on the CPU) must meet it on these inputs"""
    worst = 0.0
    for kind in ("normal", "plus1e4", "minus1e4", "neginf", "equal", "ties"):
        X, T = R.make_case(kind, V, 37, seed=2)
        lp64, _ = R.logprob_rows_ref(X, T)
        lp32 = torch.log_softmax(torch.from_numpy(X), -1).gather(1, torch.from_numpy(T)[:, None])[:, 0].numpy()
        fin = np.isfinite(lp64)
        if fin.any():
            worst = max(worst, float(np.max(np.abs(lp32[fin] - lp64[fin]) / (R.ABS + R.REL * np.abs(lp64[fin])))))
        assert R.within_gate(lp32, lp64).all(), (kind, V)
    print(f"[logprob] V={V}: fp32 log_softmax uses {worst:.3f} of the gate")


NEW = ("showo_logprob_rows", "showo_engine_decode_sample_lp", "showo_engine_batch_decode_sample_lp", "showo_engine_score",
       "showo_engine_prefill_append_score")


def test_new_entry_points_are_declared_bound_and_exported():
    L = util.lib()
    lib = L.load()
    hdr = open(os.path.join(util.ROOT, "include", "showo_hip.h")).read()
    for name in NEW:
        assert f"int {name}(" in hdr and name in L.EXPORTED_SYMBOLS and name in L._PROTOS and hasattr(lib, name), name
    # bad arguments are refused on the host: an error code and a message, nothing launched
    assert lib.showo_logprob_rows(None, 8, 1, 8, None, None, None, None) != 0 and b"logprob_rows" in lib.showo_last_error()
    assert lib.showo_logprob_rows(None, 8, 0, 8, None, None, None, None) == 0  # no rows: nothing to do
    assert lib.showo_engine_score(None, None, None, None, 1, 1, None, None, 1, 0, None, None, None) != 0
    assert lib.showo_engine_prefill_append_score(None, None, 1, None, None, None, None, None) != 0
    assert lib.showo_engine_decode_sample_lp(None, None, 1, None, None, 1, 1.0, 1.0, None, 0, 0, None, None, 0, None) != 0


def test_python_surface_has_the_new_arguments_with_off_defaults():
    M = util.pkg().modeling_showo
    for fn in (M.Showo.mmu_generate, M.Showo.mmu_generate_batch, M.MmuSession.generate, M.MmuSession.generate_batch):
        assert inspect.signature(fn).parameters["return_logprobs"].default is False, fn
    sig = inspect.signature(M.Showo.score).parameters
    assert list(sig)[1:] == ["input_ids", "input_embeddings", "attention_mask", "labels", "shift", "chunk_rows"]
    assert sig["shift"].default is True and sig["chunk_rows"].default is None
    assert list(inspect.signature(M.MmuSession.score).parameters) == ["self", "idx"]
    assert util.pkg().TokenScores._fields == ("logprobs", "ranks")


def test_session_stand_in_without_the_keyword_still_serves_calls_without_logprobs():
    """MmuSession passes return_logprobs to its engine side only when it is set (as it does for top_p)"""
    M = util.pkg().modeling_showo

    class Eng:
        dev, batched = "cpu", False

        def prefill(self, idx, emb, mask):
            return idx.shape[1]

        def stamp(self):
            return ()

        def cached_rows(self):
            return self.rows

        def append(self, ids, emb, Ln):
            self.rows += Ln

        def rewind(self, n):
            self.rows = n

        def settle(self, length, toks):
            self.rows = length + len(toks) - 1

        def use_prefix_logits(self):
            pass

        def run(self, max_new_tokens, greedy, k, temperature, noise, seed, eot_token):
            return [4, 5, 6][:max_new_tokens]

    e = Eng()
    e.rows = 3
    s = M.MmuSession(None, idx=torch.zeros((1, 3), dtype=torch.int64), _engine=e)
    out = s.generate(torch.ones((1, 2), dtype=torch.int64), max_new_tokens=3, top_k=1)
    assert [int(t) for t in out] == [4, 5, 6] and isinstance(out, list) and s.length == 3 + 2 + 2
    with pytest.raises(TypeError):
        s.generate(torch.ones((1, 2), dtype=torch.int64), max_new_tokens=3, top_k=1, return_logprobs=True)
    assert s.length == 7 and e.rows == 7  # the failed call left the session where it was
