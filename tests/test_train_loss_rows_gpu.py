"""Loss head on the labelled rows only (showo_train_set_loss_rows 1 / `Trainer(loss_rows="labelled")`): the ordered row census, the
compact cross-entropy, the row-slot final-LayerNorm backward and the engine / Trainer plumbing, against the dense mode and the
reference's own values.

Contract: the values one row gets (logits, loss, d logits, d hidden) do not depend on the mode when both launches take the production
GEMM family with the split pinned, so every gradient below lm_head is `torch.equal` between the modes; lm_head.weight / .bias differ
only in the grouping of their fp32 sums over the token rows (gate: rel. rms 1e-4 -- regrouping n = 302 random-sign products moves
a sum by about n 2^-24 = 2e-5 of its norm, one dropped or doubled row by about n^-1/2 = 6e-2); the losses in the last fp32 bit.

State of this file: written against the kernels' stated contract and collected on a CPU box; it has NOT yet run on an MI355X, so no measured
figure is quoted here."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import util
from util import Wt, dev

import test_train_accum_gpu as A
import test_train_loss_rows_cpu as cpu

pytestmark = pytest.mark.gpu

W = (1.0, 0.1, 1.0)
HEAD = ("showo.lm_head.weight", "showo.lm_head.bias")
EMBED = "showo.model.embed_tokens.weight"


def L():
    return util.lib()


# ---------------------------------------------------------------- drivers

def _run(m, batch, split, msl, mode, w=W, accumulate=0, announce=False, head_dev=False):
    """forward + full backward of one batch through the C ABI in loss-rows mode `mode`; returns the three losses"""
    P = util.pkg()
    ids, mask, labels = batch
    tr = m.trainer()
    P.modeling_showo.sync_trainable(m, tr, {n: bool(p.requires_grad) for n, p in m.named_parameters()}, False)
    dm = P.training.train_mask(tr, mask)
    B, Lq = ids.shape
    losses = torch.empty(3, dtype=torch.float32, device="cuda")
    s = L().stream()
    L().call("showo_train_set_accumulate", tr, int(accumulate))
    L().call("showo_train_set_loss_rows", tr, mode)
    if announce:
        L().call("showo_train_set_loss_weights", tr, w[0], w[1], w[2], 1)
    try:
        try:
            L().call("showo_train_forward", tr, L().ptr(ids), L().ptr(dm), L().ptr(labels), B, Lq, split[0], split[1], split[2], msl,
                     None, L().ptr(losses), s)
        finally:
            L().call("showo_trainer_use_intervals", tr, None, None)
        if head_dev:
            g3 = dev(torch.tensor(w, dtype=torch.float32))
            L().call("showo_train_backward_head_dev", tr, L().ptr(labels), split[0], split[1], split[2], msl, L().ptr(g3), s)
            for i in range(m.arch["num_hidden_layers"] - 1, -1, -1):
                L().call("showo_train_backward_layer", tr, i, s)
            L().call("showo_train_backward_embed", tr, s)
        else:
            L().call("showo_train_backward", tr, L().ptr(labels), split[0], split[1], split[2], msl, w[0], w[1], w[2], s)
    finally:
        L().call("showo_train_set_accumulate", tr, 0)
        L().call("showo_train_set_loss_rows", tr, 0)
        L().call("showo_train_set_loss_weights", tr, 0.0, 0.0, 0.0, 0)
    return losses


def _loss_rows(m):
    rows, total = C.c_int(), C.c_int()
    L().call("showo_train_loss_rows", m._trainer, C.byref(rows), C.byref(total))
    return rows.value, total.value


def _rel_rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt() / b.double().pow(2).mean().sqrt())


def _ulp_apart(a, b):
    """the two fp32 values differ by at most one unit in the last place"""
    a, b = np.float32(a), np.float32(b)
    return abs(float(a) - float(b)) <= float(np.spacing(max(abs(a), abs(b))))


_SMALL = {}


def _small2():
    """the small fixture with each group doubled (t2i, t2i, lm, lm, mmu, mmu): split 12/4/8, 24 x 27 = 648 rows, 302 labelled.  Every
    group mean -- so every loss and gradient -- is mathematically that of the fixture."""
    if not _SMALL:
        g = util.golden("showo_small_train.npz")
        d = Wt.ShowoDims(**Wt.SMALL)
        order = torch.tensor(list(range(0, 6)) * 2 + [6, 7] * 2 + list(range(8, 12)) * 2)

        def dbl(x):
            return torch.from_numpy(x)[order].contiguous()
        _SMALL.update(g=g, d=d, sd=Wt.make_showo_state(d, seed=13), host=(dbl(g["ids"]).long(), dbl(g["mask"]), dbl(g["labels"]).long()))
    s = _SMALL
    return s["g"], s["d"], s["sd"], s["host"]


SPLIT2 = (12, 4, 8)


def _small2_model():
    g, d, sd, host = _small2()
    m = util.build_showo(d, sd, max_batch=24, max_seq=32).train()
    return g, d, m, tuple(dev(x) for x in host)


def _both_modes(m, batch, split, msl, **kw):
    la = _run(m, batch, split, msl, 0, **kw)
    ga = A._snapshot(m)
    ll = _run(m, batch, split, msl, 1, **kw)
    gl = A._snapshot(m)
    return la.cpu(), ga, ll.cpu(), gl


def _redraw_small2(d, ids, labels, seed):
    """a second micro-batch with the layout of the doubled small batch (A._redraw for its 12 t2i and 8 mmu rows)"""
    rs = np.random.RandomState(seed)
    N = d.num_vq_tokens
    ids, labels = ids.clone(), labels.clone()
    img = torch.from_numpy(rs.randint(0, d.codebook, size=(12, N)) + d.image_offset)
    masked = torch.from_numpy(rs.rand(12, N) < 0.6)
    ids[:12, -(N + 1):-1] = torch.where(masked, torch.full_like(img, d.mask_token_id), img)
    labels[:12, -(N + 1):-1] = torch.where(masked, img, torch.full_like(img, -100))
    ids[16:, 2:2 + N] = torch.from_numpy(rs.randint(0, d.codebook, size=(8, N)) + d.image_offset)
    return ids, labels


# ---------------------------------------------------------------- 1. the census kernel

def _census(labels, split, msl):
    B, Lq = labels.shape
    T = B * Lq
    lab = dev(labels)
    i32 = dict(dtype=torch.int32, device="cuda")
    rows, rows_c = torch.full((3 * T,), -7, **i32), torch.full((3 * T,), -7, **i32)
    counts, n = torch.full((3,), -7, **i32), torch.full((1,), -7, **i32)
    index, slot = torch.full((T,), -7, **i32), torch.full((T,), -7, **i32)
    ws = torch.zeros(L().load().showo_ce_rows_compact_ws(T), **i32)
    L().call("showo_ce_rows_compact", L().ptr(lab), B, Lq, split[0], split[1], split[2], msl, L().ptr(rows), L().ptr(rows_c), L().ptr(counts),
             L().ptr(index), L().ptr(slot), L().ptr(n), L().ptr(ws), L().stream())
    torch.cuda.synchronize()
    return [x.cpu() for x in (rows.view(T, 3), rows_c.view(T, 3), counts, index, slot, n)], ws.numel()


def _check_census(labels, split, msl):
    (rows, rows_c, counts, index, slot, n), nblk = _census(labels, split, msl)
    want = util.pkg().training_utils.labelled_rows(labels, *split, msl)
    T, Tc = labels.numel(), int(n)
    assert Tc == want.numel()
    assert torch.equal(index[:Tc].long(), want)
    inv = torch.full((T,), -1, dtype=torch.int32)
    inv[want] = torch.arange(Tc, dtype=torch.int32)
    assert torch.equal(slot, inv)
    bt, bl, bm = split
    valid = labels != -100
    c = [int(valid[:bt, msl + 1:].sum()), int(valid[bt:bt + bl, 1:].sum()), int(valid[labels.shape[0] - bm if bm else 0:, 1:].sum())]
    assert counts.tolist() == c
    assert torch.equal(rows_c[:Tc], rows[want])  # the compact table is the table's labelled entries, in order
    assert bool((rows[:, 2] != 0).sum() == Tc) and bool((rows_c[:Tc, 2] != 0).all())
    return (rows, rows_c[:Tc], counts, index[:Tc], slot, n), nblk


@pytest.mark.parametrize("case", cpu.cases(), ids=lambda c: c[0])
def test_census_kernel_equals_labelled_rows(case):
    name, labels, split, msl, want_n, total = case
    out, _ = _check_census(labels, split, msl)
    assert int(out[5]) == want_n and labels.numel() == total


def test_census_kernel_over_several_scan_blocks_is_ordered_and_reproducible():
    small = torch.from_numpy(util.golden("showo_small_train.npz")["labels"]).long()
    labels = small.repeat(3, 1)  # 36 x 27 = 972 rows
    a, nblk = _check_census(labels, (18, 6, 12), 8)
    assert nblk >= 3, nblk
    b, _ = _check_census(labels, (18, 6, 12), 8)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------- 2. the modes agree (production family)

def test_modes_agree_on_the_doubled_small_batch_and_meet_the_reference():
    g, d, m, batch = _small2_model()
    la, ga, ll, gl = _both_modes(m, batch, SPLIT2, d.max_text_len)
    assert _loss_rows(m) == (302, 648)
    print(f"[loss rows] losses dense {la.tolist()} labelled {ll.tolist()}")
    for k in range(3):
        assert _ulp_apart(la[k], ll[k]), (k, float(la[k]), float(ll[k]))
    for n in A._names(m):
        if n in HEAD:
            r = _rel_rms(gl[n], ga[n])
            print(f"[loss rows] {n}: rel_rms(labelled, dense) = {r:.3e}")
            assert r <= 1e-4, (n, r)
        else:
            assert torch.equal(gl[n], ga[n]), n
    # doubling leaves every group mean unchanged: the labelled run meets the fixture's reference values (the gates of
    # test_small_training_step_production_path_vs_reference_golden)
    for a, b in zip(ll.tolist(), g["losses"]):
        assert abs(a - b) < 5e-3 * abs(b)
    named = dict(m.named_parameters())
    n = 0
    for k in g.files:
        if not k.startswith("grad::showo"):
            continue
        name = k[len("grad::"):]
        want = torch.from_numpy(g[k])
        rmax, rrms = util.relerr(gl[name].view(want.shape), want)
        assert rrms < 3e-2 and rmax < 8e-2, (name, rmax, rrms)
        n += 1
    assert n >= 30
    for tab, key in ((EMBED, "embed"), ("showo.lm_head.weight", "lm_head")):
        rows = torch.from_numpy(g[f"grad::{key}_row_ids"])
        rmax, rrms = util.relerr(gl[tab].view(named[tab].shape)[rows.cuda()], torch.from_numpy(g[f"grad::{key}_rows"]))
        assert rrms < 3e-2, (tab, rrms)
    # the announced form (the forward's pass writes d logits, the backward reuses it) gives the same bits
    l2 = _run(m, batch, SPLIT2, d.max_text_len, 1, announce=True).cpu()
    g2 = A._snapshot(m)
    assert torch.equal(l2, ll)
    for n in A._names(m):
        assert torch.equal(g2[n], gl[n]), n


# ---------------------------------------------------------------- 3. tiny fixture (below the production threshold)

def _tiny():
    g = util.golden("showo_tiny_forward.npz")
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd).train()
    host = (torch.from_numpy(g["train_ids"]).long(), torch.from_numpy(g["train_mask"]), torch.from_numpy(g["train_labels"]).long())
    return g, d, m, host


def _close_to_dense(ga, gl, names):
    num = sum(float((gl[n].double() - ga[n].double()).pow(2).sum()) for n in names)
    den = sum(float(ga[n].double().pow(2).sum()) for n in names)
    print(f"[loss rows] sum |g_l - g_a|^2 / sum |g_a|^2 = {num / den:.3e}")
    assert num <= (1e-5) ** 2 * den, (num, den)


def test_tiny_fixture_losses_and_gradients():
    g, d, m, host = _tiny()
    batch = tuple(dev(x) for x in host)
    la, ga, ll, gl = _both_modes(m, batch, (2, 1, 2), d.max_text_len)
    assert _loss_rows(m) == (67, 135)
    for a, b in zip(ll.tolist(), g["train_losses"]):
        assert abs(a - b) < 5e-3 * abs(b)
    _close_to_dense(ga, gl, A._names(m))


def test_tiny_fixture_transpose_branch_in_a_child_process():
    """SHOWO_TRAIN_TN=0 (read once per process): the compact head on the transpose + NT-GEMM weight-gradient form -- the R-row
    transposes of d(logits) / hf (67 labelled rows of 135) and the slot LayerNorm backward without column sums"""
    env = dict(os.environ, SHOWO_TRAIN_TN="0")
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); import test_train_loss_rows_gpu as t; t.test_tiny_fixture_losses_and_gradients(); "
            "print('CHILD_OK')" % here)
    r = subprocess.run([sys.executable, "-s", "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------- 4. edges (tiny model)

def test_edges_quirk_split_empty_batch_bad_label_and_refusals():
    g, d, m, host = _tiny()
    ids, mask, labels = host
    msl = d.max_text_len
    batch = tuple(dev(x) for x in host)
    # b_mmu = 0: logits[-0:] labels the whole batch, 17 rows carry two targets
    la, ga, ll, gl = _both_modes(m, batch, (2, 3, 0), msl)
    assert _loss_rows(m) == (89, 135)
    for k in range(3):
        assert abs(float(la[k]) - float(ll[k])) <= 1e-5 * abs(float(la[k]))
    _close_to_dense(ga, gl, A._names(m))
    # a normal step, an empty step (every label -100), the normal step again
    l0 = _run(m, batch, (2, 1, 2), msl, 1).cpu()
    g0 = A._snapshot(m)
    empty = (batch[0], batch[1], dev(torch.full_like(labels, -100)))
    le = _run(m, empty, (2, 1, 2), msl, 1).cpu()
    ge = A._snapshot(m)
    assert _loss_rows(m) == (0, 135)
    assert bool(torch.isnan(le).all())
    for n in A._names(m):
        assert int(torch.count_nonzero(ge[n])) == 0, n
    l1 = _run(m, batch, (2, 1, 2), msl, 1).cpu()
    g1 = A._snapshot(m)
    assert torch.equal(l0, l1)
    for n in A._names(m):
        assert torch.equal(g0[n], g1[n]), n
    # a label >= V in a labelled row of the lm sequence: that group's loss and the lm_head gradient are poisoned, as in the dense mode
    bad = labels.clone()
    pos = int(torch.nonzero(bad[2] != -100)[2])
    bad[2, pos] = d.vocab + 5
    lb = _run(m, (batch[0], batch[1], dev(bad)), (2, 1, 2), msl, 1).cpu()
    gb = A._snapshot(m)
    assert math.isnan(float(lb[1])) and math.isfinite(float(lb[0])) and math.isfinite(float(lb[2]))
    assert not bool(torch.isfinite(gb["showo.lm_head.weight"]).all())
    # mode 1 with logits_out: refused with a message, nothing launched
    tr = m.trainer()
    out = torch.empty(ids.numel() * d.vocab, device="cuda")
    losses = torch.empty(3, device="cuda")
    L().call("showo_train_set_loss_rows", tr, 1)
    try:
        dm = util.pkg().training.train_mask(tr, batch[1])
        before = A._gemm_counters()
        with pytest.raises(RuntimeError, match="not materialise"):
            L().call("showo_train_forward", tr, L().ptr(batch[0]), L().ptr(dm), L().ptr(batch[2]), 5, ids.shape[1], 2, 1, 2, msl,
                     L().ptr(out), L().ptr(losses), L().stream())
        assert A._gemm_counters() == before
        with pytest.raises(RuntimeError, match="mode must be"):
            L().call("showo_train_set_loss_rows", tr, 2)
    finally:
        L().call("showo_train_set_loss_rows", tr, 0)
    # the trainer is still usable, in either mode
    l2 = _run(m, batch, (2, 1, 2), msl, 1).cpu()
    assert torch.equal(l2, l0)


# ---------------------------------------------------------------- 5. with the other switches (doubled small batch)

def test_accumulation_window_in_labelled_mode_is_the_sum_of_its_micro_batches():
    g, d, m, batch = _small2_model()
    _, _, _, host = _small2()
    ids2, lab2 = _redraw_small2(d, host[0], host[2], 101)
    assert not torch.equal(ids2, host[0]) and not torch.equal(lab2, host[2])
    batches = [batch, (dev(ids2), batch[1], dev(lab2))]
    w = tuple(c / 2 for c in W)
    vs = []
    for b in batches:
        _run(m, b, SPLIT2, d.max_text_len, 1, w=w)
        vs.append(A._snapshot(m))
    assert not torch.equal(vs[0][EMBED], vs[1][EMBED])
    for j, b in enumerate(batches):
        _run(m, b, SPLIT2, d.max_text_len, 1, w=w, accumulate=j > 0)
    A._gate_sum(A._snapshot(m), vs, A._names(m), "labelled rows k=2")


def test_frozen_lm_head_runs_no_head_wgrad_and_keeps_the_rest_bit_equal():
    g, d, m, batch = _small2_model()
    m.showo.lm_head.requires_grad_(False)
    m.trainer()
    la, ga, _, _ = _both_modes(m, batch, SPLIT2, d.max_text_len)
    A._counters(m, reset=True)
    ll = _run(m, batch, SPLIT2, d.max_text_len, 1).cpu()
    cnt = A._counters(m)
    gl = A._snapshot(m)
    assert cnt["wgrad"] == 4 * d.layers, cnt  # the blocks' weight gradients only
    for n in A._names(m):
        assert torch.equal(gl[n], ga[n]), n
    for n in HEAD:
        assert int(torch.count_nonzero(gl[n])) == 0


def test_only_lm_head_trainable_runs_no_dgrad():
    g, d, m, batch = _small2_model()
    for n, p in m.named_parameters():
        p.requires_grad_(n in HEAD)
    m.trainer()
    _run(m, batch, SPLIT2, d.max_text_len, 0)
    ga = A._snapshot(m)
    A._counters(m, reset=True)
    _run(m, batch, SPLIT2, d.max_text_len, 1)
    cnt = A._counters(m)
    gl = A._snapshot(m)
    assert cnt["dgrad"] == 0 and cnt["phases"] == 0 and cnt["wgrad"] == 1, cnt
    for n in HEAD:
        r = _rel_rms(gl[n], ga[n])
        print(f"[loss rows] only lm_head trains, {n}: rel_rms = {r:.3e}")
        assert r <= 1e-4, (n, r)
    for n in A._names(m):
        if n not in HEAD:
            assert int(torch.count_nonzero(gl[n])) == 0, n


def test_device_weight_head_backward_equals_the_host_weight_form():
    g, d, m, batch = _small2_model()
    lh = _run(m, batch, SPLIT2, d.max_text_len, 1).cpu()
    gh = A._snapshot(m)
    ld = _run(m, batch, SPLIT2, d.max_text_len, 1, head_dev=True).cpu()
    gd = A._snapshot(m)
    assert torch.equal(lh, ld)
    for n in A._names(m):
        assert torch.equal(gh[n], gd[n]), n


# ---------------------------------------------------------------- 6. Trainer

def test_trainer_in_labelled_mode_trains_and_leaves_the_autograd_path_dense():
    P = util.pkg()
    g, d, ml, batch = _small2_model()
    _, _, md, _ = _small2_model()
    ids, mask, labels = batch
    kw = dict(batch_size_t2i=SPLIT2[0], batch_size_lm=SPLIT2[1], batch_size_mmu=SPLIT2[2], max_seq_length=d.max_text_len)
    saved = {k: v.detach().clone() for k, v in ml.state_dict().items()}
    logits0 = ml(ids, attention_mask=mask, labels=labels, **kw)[0].detach().clone()
    assert tuple(logits0.shape) == (24, 27, d.vocab)
    tl = P.Trainer(ml, lr=1e-3, loss_rows="labelled")
    td = P.Trainer(md, lr=1e-3)
    first_l = tl.step(ids, mask, labels, *SPLIT2, d.max_text_len)
    first_d = td.step(ids, mask, labels, *SPLIT2, d.max_text_len)
    assert tl.loss_rows_count == (302, 648) and td.loss_rows_count == (648, 648)
    assert torch.allclose(first_l.cpu(), first_d.cpu(), rtol=1e-4, atol=0)
    # the module's forward between two labelled steps runs all rows and returns the full logits
    ml.load_state_dict(saved)
    logits1 = ml(ids, attention_mask=mask, labels=labels, **kw)[0].detach()
    assert torch.equal(logits0, logits1)
    again = tl.step(ids, mask, labels, *SPLIT2, d.max_text_len)
    assert tl.loss_rows_count == (302, 648)
    assert bool(torch.isfinite(again).all())
    for _ in range(3):
        last = tl.step(ids, mask, labels, *SPLIT2, d.max_text_len)
    assert float(last.sum()) < float(first_l.sum())
