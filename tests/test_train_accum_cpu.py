"""Gradient accumulation over micro-batches, the parts that need no GPU: the window bookkeeping of Trainer.step (reference:
`accelerator.accumulate(model)`, training/train.py:589-631, `training.gradient_accumulation_steps`) and the C ABI it rests on."""
import inspect
import os
import re

import pytest

import util

NEW_ENTRY_POINTS = ("showo_train_set_accumulate", "showo_dgelu_colsum_bf16_acc", "showo_qkln_rope_bwd_acc", "showo_ln_bwd_acc",
                    "showo_ln_bwd_colsum_acc", "showo_embed_bwd_acc")


@pytest.mark.parametrize("k", [1, 3, 4])
def test_window_flags_and_loss_scale_over_two_windows(k):
    w = util.pkg().AccumulationWindow(k)
    assert w.steps == k and w.loss_scale == 1.0 / k and not w.is_open
    coeffs = (1.0, 0.1, 1.0)
    for window in range(2):
        for j in range(k):
            assert w.position == j
            assert w.is_first == (j == 0)
            assert w.closes == (j == k - 1)
            assert w.is_open == (j != 0)  # a partial sum sits in the gradient buffer
            got = w.scaled(coeffs)
            if k == 1:
                assert got == coeffs  # the plain step's own values, untouched
            else:
                assert got == tuple(c / k for c in coeffs)
            closed = w.advance()
            assert closed == (j == k - 1)
        assert w.windows_closed == window + 1 and w.position == 0 and not w.is_open
    # k micro-batch losses, each scaled by 1 / k, sum to the mean of the micro-batch means
    assert abs(sum(w.loss_scale for _ in range(k)) - 1.0) < 1e-12


def test_window_reset_and_bad_sizes():
    W = util.pkg().AccumulationWindow
    w = W(3)
    w.advance()
    assert w.is_open
    w.reset()
    assert w.position == 0 and w.is_first and not w.is_open
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            W(bad)


def test_trainer_takes_gradient_accumulation_steps_and_keeps_the_step_signature():
    T = util.pkg().Trainer
    p = inspect.signature(T.__init__).parameters
    assert p["gradient_accumulation_steps"].default == 1
    assert list(inspect.signature(T.step).parameters) == ["self", "input_ids", "attention_mask", "labels", "batch_size_t2i",
                                                          "batch_size_lm", "batch_size_mmu", "max_seq_length"]
    assert callable(T.window_losses)


def test_header_declares_the_accumulating_entry_points():
    hdr = open(os.path.join(util.ROOT, "include", "showo_hip.h")).read()
    declared = set(re.findall(r"\b(showo_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert name in util.lib().EXPORTED_SYMBOLS, name
    # the existing signatures keep their argument lists: the accumulating forms are additions
    assert re.search(r"int showo_embed_bwd\(const int64_t\* ids, const float\* dx, float\* dE, int\* order_ws, int T, int H, int V, void\* stream\);",
                     hdr)
    assert re.search(r"int showo_train_set_accumulate\(showo_trainer\* t, int on\);", hdr)
