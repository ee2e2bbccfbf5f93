"""Loss head on the labelled rows only (`Trainer(loss_rows="labelled")`), the parts that need no GPU: the C ABI, the public
switch, and `training_utils.labelled_rows` -- the row rule of `Showo.forward`'s three losses (reference models/modeling_showo.py:83-98)
in plain torch, which is the yardstick of the device census (showo_ce_rows_compact) in test_train_loss_rows_gpu.py."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import util

NEW_ENTRY_POINTS = ("showo_ce_rows_compact", "showo_train_set_loss_rows", "showo_train_loss_rows")


def census_by_loops(labels, bt, bl, bm, msl):
    """the reference's three slices written out row by row: (ascending labelled rows, number of targets per labelled row)"""
    B, L = labels.shape
    rows, targets = [], []
    for b in range(B):
        for l in range(L):
            n = 0
            if b < bt and l >= msl + 1 and labels[b, l] != -100:  # logits[:bt, msl + 1:] against labels[:bt, msl + 1:]
                n += 1
            if l < L - 1 and labels[b, l + 1] != -100:  # logits[.., :-1] against labels[.., 1:]
                in_lm = bt <= b < bt + bl
                in_mmu = True if bm == 0 else b >= B - bm  # logits[-0:] is the whole batch
                if in_lm or in_mmu:
                    n += 1
            if n:
                rows.append(b * L + l)
                targets.append(n)
    return np.asarray(rows, dtype=np.int64), np.asarray(targets)


def cases():
    """(name, labels int64 [B, L], split, max_seq_length, labelled rows, total rows)"""
    gs = util.golden("showo_small_train.npz")
    gt = util.golden("showo_tiny_forward.npz")
    small = torch.from_numpy(gs["labels"]).long()
    tiny = torch.from_numpy(gt["train_labels"]).long()
    d = util.tiny_dims()
    bt, bl, bm = (int(x) for x in gs["b"])
    assert (bt, bl, bm) == (6, 2, 4)
    lm_only = tiny[2:3].repeat(3, 1).clone()
    lm_only[lm_only == -100] = 7  # every position carries a label: B * (L - 1) rows predict one
    return [
        ("small", small, (6, 2, 4), 8, 151, 324),
        ("tiny", tiny, (2, 1, 2), d.max_text_len, 67, 135),
        ("tiny, b_mmu = 0", tiny, (2, 3, 0), d.max_text_len, 89, 135),
        ("all ignored", torch.full_like(tiny, -100), (2, 1, 2), d.max_text_len, 0, 135),
        ("lm only", lm_only, (0, 3, 0), d.max_text_len, 3 * (tiny.shape[1] - 1), 3 * tiny.shape[1]),
    ]


def test_header_and_bindings_carry_the_new_entry_points():
    hdr = open(os.path.join(util.ROOT, "include", "showo_hip.h")).read()
    declared = set(re.findall(r"\b(showo_[a-z0-9_]+)\s*\(", hdr))
    L = util.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert name in L._PROTOS, name
    assert re.search(r"int showo_train_set_loss_rows\(showo_trainer\* t, int mode\);", hdr)
    assert re.search(r"int showo_train_loss_rows\(showo_trainer\* t, int\* rows, int\* total\);", hdr)
    # existing signatures keep their argument lists
    assert re.search(r"int showo_train_set_accumulate\(showo_trainer\* t, int on\);", hdr)
    assert len(L._PROTOS["showo_train_forward"]) == 13 and len(L._PROTOS["showo_ce_loss"]) == 20


def test_trainer_takes_loss_rows_and_refuses_bad_values_before_any_gpu_use():
    P = util.pkg()
    T = P.Trainer
    p = inspect.signature(T.__init__).parameters
    assert p["loss_rows"].default == "all"
    assert list(inspect.signature(T.step).parameters) == ["self", "input_ids", "attention_mask", "labels", "batch_size_t2i",
                                                          "batch_size_lm", "batch_size_mmu", "max_seq_length"]
    assert isinstance(T.loss_rows_count, property)
    mode = P.training.loss_rows_mode
    assert mode("all") == 0 and mode("labelled") == 1
    for bad in ("labeled", "", None, 1, "ALL"):
        with pytest.raises(ValueError):
            mode(bad)
    # the constructor validates first: a bad value raises ValueError although the "model" is not a model at all
    with pytest.raises(ValueError, match="loss_rows"):
        T(object(), loss_rows="some")


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_labelled_rows_is_the_references_row_rule(case):
    name, labels, (bt, bl, bm), msl, want_n, want_total = case
    got = util.pkg().training_utils.labelled_rows(labels, bt, bl, bm, msl)
    rows, targets = census_by_loops(labels.numpy(), bt, bl, bm, msl)
    assert got.dtype == torch.int64 and got.dim() == 1
    assert labels.numel() == want_total
    assert len(rows) == want_n, (name, len(rows))
    assert np.array_equal(got.numpy(), rows), name
    assert bool((got[1:] > got[:-1]).all())
    if name == "tiny, b_mmu = 0":
        assert int((targets == 2).sum()) == 17  # t2i rows that the whole-batch mmu slice labels a second time
