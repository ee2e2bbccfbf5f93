"""Native step for the CLIP-ViT model (`Trainer(projector=True).step_clip_vit`), the parts that need no GPU: the C ABI, the public
signatures, and `training_utils.splice_image_columns` against the reference's concatenations (training/train_w_clip_vit.py:520-549
for llava_pretrain, :561-589 for llava_tuning)."""
import inspect
import os
import re

import pytest
import torch

import util

NEW_ENTRY_POINTS = ("showo_embed_splice_f32", "showo_gather_splice_rows_f32", "showo_embed_bwd_splice", "showo_train_forward_spliced",
                    "showo_train_image_grad", "showo_projector_backward_acc", "showo_grad_clip_norm2")


def test_header_and_bindings_carry_the_new_entry_points():
    hdr = open(os.path.join(util.ROOT, "include", "showo_hip.h")).read()
    declared = set(re.findall(r"\b(showo_[a-z0-9_]+)\s*\(", hdr))
    L = util.lib()
    lib = L.load()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert name in L._PROTOS, name
        assert hasattr(lib, name), name
    assert re.search(r"int showo_embed_splice_f32\(const int64_t\* ids, const float\* table, const float\* rows, const int32_t\* start, "
                     r"float\* x, int B, int L,\s+int n, int P, int H, int V, void\* stream\);", hdr)
    assert re.search(r"int showo_train_image_grad\(showo_trainer\* t, float\* out, int64_t n_elems, void\* stream\);", hdr)
    assert len(L._PROTOS["showo_train_forward_spliced"]) == 17
    # existing signatures keep their argument lists
    assert len(L._PROTOS["showo_train_forward"]) == 13
    assert len(L._PROTOS["showo_projector_backward"]) == 9 and len(L._PROTOS["showo_grad_clip_norm"]) == 6
    assert len(L._PROTOS["showo_embed_bwd_acc"]) == 9


def test_host_side_argument_checks_refuse_bad_layouts_without_a_launch():
    """n outside [0, B], P > L, H % 4 != 0 and a missing start are refused on the host (error code 1): nothing is launched, no GPU needed"""
    lib = util.lib().load()
    one = 4096  # never dereferenced on the host
    ok = dict(B=3, L=40, n=2, P=24, H=128)
    for bad in (dict(n=4), dict(n=-1), dict(P=41), dict(H=126), dict(B=0)):
        a = dict(ok, **bad)
        assert lib.showo_embed_splice_f32(one, one, one, one, one, a["B"], a["L"], a["n"], a["P"], a["H"], 37, None) == 1, bad
        assert lib.showo_gather_splice_rows_f32(one, one, one, a["B"], a["L"], a["n"], a["P"], a["H"], None) == 1, bad
        assert lib.showo_embed_bwd_splice(one, one, one, one, one, 0, a["B"], a["L"], a["n"], a["P"], a["H"], 37, None) == 1, bad
    assert lib.showo_embed_splice_f32(one, one, one, None, one, 3, 40, 2, 24, 128, 37, None) == 1  # rows without their starts
    assert b"spliced rows" in lib.showo_last_error()
    assert lib.showo_train_image_grad(None, one, 0, None) == 1


def test_trainer_signatures():
    P = util.pkg()
    T = P.Trainer
    p = inspect.signature(T.__init__).parameters
    assert p["projector"].default is False
    assert list(p)[-1] == "projector"  # appended: positional callers of the earlier arguments keep working
    assert list(inspect.signature(T.step).parameters) == ["self", "input_ids", "attention_mask", "labels", "batch_size_t2i",
                                                          "batch_size_lm", "batch_size_mmu", "max_seq_length"]
    assert list(inspect.signature(T.step_clip_vit).parameters) == ["self", "input_ids", "image_features", "image_start", "attention_mask",
                                                                   "labels", "batch_size_t2i", "batch_size_lm", "batch_size_mmu",
                                                                   "max_seq_length"]
    assert callable(T.projector_grads)
    assert P.training.PROJECTOR_KEYS == ("mm_projector.0.weight", "mm_projector.0.bias", "mm_projector.2.weight", "mm_projector.2.bias")


def _reference_pretrain(input_ids_mmu, labels_mmu, P, mmu, soi, eoi, ignore):
    """training/train_w_clip_vit.py:520-549: ids = [mmu, soi, eoi, text]; embeddings are cut at column 2 around the image rows;
    labels = [ignore, ignore, ignore x P, ignore, labels]"""
    n = input_ids_mmu.shape[0]
    one = torch.ones(n, 1)
    ids = torch.cat([one * mmu, one * soi, one * eoi, input_ids_mmu], dim=1).long()
    labels = torch.cat([one * ignore, one * ignore, torch.ones(n, P) * ignore, one * ignore, labels_mmu], dim=1).long()
    return ids, labels, 2


def _reference_tuning(input_ids_mmu, labels_mmu, input_ids_system, P, mmu, soi, eoi, ignore):
    """training/train_w_clip_vit.py:561-589: ids = [mmu, system, soi, eoi, text], cut at 2 + SYSTEM_PROMPT_LEN"""
    n = input_ids_mmu.shape[0]
    one = torch.ones(n, 1)
    ids = torch.cat([one * mmu, input_ids_system, one * soi, one * eoi, input_ids_mmu], dim=1).long()
    labels = torch.cat([one * ignore, torch.ones_like(input_ids_system) * ignore, one * ignore, torch.ones(n, P) * ignore, one * ignore,
                        labels_mmu], dim=1).long()
    return ids, labels, 2 + input_ids_system.shape[1]


@pytest.mark.parametrize("branch", ["llava_pretrain", "llava_tuning"])
def test_splice_image_columns_is_the_references_concatenation(branch):
    splice = util.pkg().training_utils.splice_image_columns
    g = torch.Generator().manual_seed(3)
    n, Lt, P, H = 4, 13, 6, 8
    mmu, soi, eoi, ignore, fill = 901, 902, 903, -100, 0
    text = torch.randint(0, 900, (n, Lt), generator=g)
    lab = torch.where(torch.rand(n, Lt, generator=g) < 0.4, torch.full((n, Lt), ignore), text)
    if branch == "llava_pretrain":
        ids, labels_ref, cut = _reference_pretrain(text, lab, P, mmu, soi, eoi, ignore)
        labels_text = torch.cat([torch.full((n, 3), ignore), lab], dim=1)  # the labels of the id columns themselves
    else:
        system = torch.randint(0, 900, (n, 5), generator=g)
        ids, labels_ref, cut = _reference_tuning(text, lab, system, P, mmu, soi, eoi, ignore)
        labels_text = torch.cat([torch.full((n, 3 + 5), ignore), lab], dim=1)
    got_ids, got_labels = splice(ids, labels_text, cut, P, fill, ignore)
    assert got_ids.dtype == torch.int64 and got_labels.dtype == torch.int64
    assert torch.equal(got_labels, labels_ref)
    # the ids: an embedding of the spliced ids, with the image rows put at the placeholder columns, is the reference's torch.cat
    table = torch.randn(1000, H, generator=g)
    images = torch.randn(n, P, H, generator=g)
    emb = torch.nn.functional.embedding(ids, table)
    want = torch.cat((emb[:, :cut], images, emb[:, cut:]), dim=1)
    got = torch.nn.functional.embedding(got_ids, table)
    assert bool((got_ids[:, cut:cut + P] == fill).all())
    got[:, cut:cut + P] = images
    assert torch.equal(got, want)


def test_splice_image_columns_per_sequence_starts():
    splice = util.pkg().training_utils.splice_image_columns
    g = torch.Generator().manual_seed(5)
    n, Lt, P = 3, 9, 4
    ids = torch.randint(0, 50, (n, Lt), generator=g)
    lab = torch.randint(0, 50, (n, Lt), generator=g)
    starts = [0, 5, Lt]  # at the front, inside, at the very end (start + P == L)
    got_ids, got_lab = splice(ids, lab, starts, P, 7, -100)
    for j, st in enumerate(starts):
        assert torch.equal(got_ids[j], torch.cat([ids[j, :st], torch.full((P,), 7), ids[j, st:]]))
        assert torch.equal(got_lab[j], torch.cat([lab[j, :st], torch.full((P,), -100), lab[j, st:]]))
    a, b = splice(ids, lab, 5, P, 7)  # scalar start, default ignore id
    c, d = splice(ids, lab, [5, 5, 5], P, 7, -100)
    assert torch.equal(a, c) and torch.equal(b, d)
    # a numpy integer, a 0-d tensor and a 1-d tensor of starts are starts too
    import numpy as np
    for one in (np.int64(5), torch.tensor(5), torch.tensor([5, 5, 5]), np.array([5, 5, 5])):
        e, f = splice(ids, lab, one, P, 7)
        assert torch.equal(a, e) and torch.equal(b, f)
    starts_of = util.pkg().training_utils.image_starts
    assert starts_of(np.int32(3), 2) == [3, 3] and starts_of(torch.tensor([1, 2]), 2) == [1, 2]
    for bad in (-1, Lt + 1, [0, 1]):
        with pytest.raises(ValueError):
            splice(ids, lab, bad, P, 7)
