"""`Trainer(model, ema=...)` on the tiny model: the EMA rides on the native AdamW launch without changing a bit of the training run,
the shadows follow the restated recurrence (tests/ema_ref.py) over the per-step parameters, `ema_weights()` evaluates on the averaged
weights through the normal engine and puts every bit back, and checkpoints carry the shadows.

The golden tiny batch of test_train_accum_gpu.py (split 2 + 1 + 2) and its two seeded re-draws are the micro-batches."""
import numpy as np
import pytest
import torch

import ema_ref
import util

pytestmark = pytest.mark.gpu

SPLIT = (2, 1, 2)
WARM = {"decay": 0.999, "use_ema_warmup": True, "update_after_step": 1}


def _batches(k=3):
    import test_train_accum_gpu as A
    d, sd, batches, _ = A._tiny_micro_batches(k)
    return d, sd, batches


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _snap(tr):
    torch.cuda.synchronize()
    return [p.detach().cpu().numpy().copy() for _, p in tr.params + tr.pparams]


def _shadows(tr):
    torch.cuda.synchronize()
    return [s.cpu().numpy().copy() for s in tr.ema.shadow_params]


def _schedule(ema):
    return dict(ema) if isinstance(ema, dict) else {"decay": float(ema)}


def _step(tr, d, b):
    return tr.step(b[0], b[1], b[2], *SPLIT, d.max_text_len)


def _same_lists(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("ema", [WARM, 0.9], ids=["warmup", "float"])
def test_five_steps_keep_the_training_bits_and_follow_the_recurrence(ema):
    P = util.pkg()
    d, sd, batches = _batches()
    a = util.build_showo(d, sd).train()
    b = util.build_showo(d, sd).train()
    ta = P.Trainer(a, lr=1e-3)
    tb = P.Trainer(b, lr=1e-3, ema=ema)
    assert ta.ema is None and isinstance(tb.ema, P.training_utils.EMA)
    assert [tuple(s.shape) for s in tb.ema.shadow_params] == [tuple(p.shape) for _, p in tb.params + tb.pparams]
    start, snaps = _shadows(tb), []
    assert _same_lists(start, _snap(tb))  # clones of the parameters
    for i in range(5):
        la, lb = _step(ta, d, batches[i % 3]), _step(tb, d, batches[i % 3])
        assert torch.equal(la, lb), i
        snaps.append(_snap(tb))
        assert tb.ema.optimization_step == i + 1
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q), n
    for n in ta.m:
        assert torch.equal(ta.m[n], tb.m[n]) and torch.equal(ta.v[n], tb.v[n]), n
    want, decay, steps = ema_ref.run(start, snaps, [True] * len(start), **_schedule(ema))
    assert tb.ema.optimization_step == steps == 5 and tb.ema.cur_decay_value == decay == ema_ref.get_decay(5, **_schedule(ema))
    assert _same_lists(want, _shadows(tb))
    assert not _same_lists(_shadows(tb), snaps[-1])  # an average, not a copy


def test_one_ema_step_per_accumulation_window():
    P = util.pkg()
    d, sd, batches = _batches()
    m = util.build_showo(d, sd).train()
    tr = P.Trainer(m, lr=1e-3, gradient_accumulation_steps=2, ema=0.5)
    start, snaps = _shadows(tr), []
    for call in range(4):
        before = _shadows(tr)
        _step(tr, d, batches[call % 3])
        if call % 2 == 0:
            assert _same_lists(before, _shadows(tr)) and not tr.sync_gradients, call  # calls 1 and 3: no optimizer step, no EMA step
        else:
            snaps.append(_snap(tr))
            assert tr.sync_gradients
    assert tr.ema.optimization_step == 2 == tr.step_count
    want, decay, _ = ema_ref.run(start, snaps, [True] * len(start), decay=0.5)
    assert _same_lists(want, _shadows(tr)) and tr.ema.cur_decay_value == decay


def test_frozen_tensors_keep_shadows_equal_to_the_parameters():
    P = util.pkg()
    d, sd, batches = _batches()
    m = util.build_showo(d, sd).train()
    m.showo.model.embed_tokens.requires_grad_(False)
    m.showo.model.layers[0].requires_grad_(False)
    tr = P.Trainer(m, lr=1e-3, ema=0.5)
    trains = [tr.trainable[n] for n, _ in tr.params]
    assert not all(trains) and any(trains)
    start, snaps = _shadows(tr), []
    for i in range(4):
        _step(tr, d, batches[i % 3])
        snaps.append(_snap(tr))
    got = _shadows(tr)
    for i, on in enumerate(trains):
        if not on:
            assert np.array_equal(_bits(got[i]), _bits(snaps[-1][i])) and np.array_equal(_bits(got[i]), _bits(start[i])), tr.params[i][0]
    want, _, _ = ema_ref.run(start, snaps, trains, decay=0.5)  # (a frozen one "copies" in the restatement: the same statement)
    assert _same_lists(want, got)
    assert any(not np.array_equal(_bits(got[i]), _bits(snaps[-1][i])) for i, on in enumerate(trains) if on)


def test_projector_shadows_follow_the_recurrence():
    import test_train_clip_vit_gpu as V
    P = util.pkg()
    m = V._model("tiny")
    bt = V._batch("tiny")
    tr = P.Trainer(m, lr=1e-3, coeffs=V.W, projector=True, ema=0.5)
    assert len(tr.pparams) == 4 and len(tr.ema.shadow_params) == len(tr.params) + 4
    start, snaps = _shadows(tr), []
    for _ in range(3):  # decay is 0 at the first step, 2 / 11 and 3 / 12 after it, capped by 0.5
        V._native_step(tr, bt)
        snaps.append(_snap(tr))
    want, decay, _ = ema_ref.run(start, snaps, [True] * len(start), decay=0.5)
    got = _shadows(tr)
    assert decay == 0.25 and _same_lists(want, got)
    k = len(tr.params)
    assert all(not np.array_equal(_bits(got[i]), _bits(snaps[-1][i])) for i in (k, k + 2))  # the projector's weights did average
    # the averaged projector is what the model runs inside the context
    feats = bt["feats"]
    raw = m.mm_projector(feats).clone()
    with tr.ema_weights():
        avg = m.mm_projector(feats).clone()
        for (n, p), s in zip(tr.pparams, got[k:]):
            assert np.array_equal(_bits(p.detach().cpu().numpy()), _bits(s)), n
    assert not torch.equal(raw, avg) and torch.equal(raw, m.mm_projector(feats))


def _logits(m, b):
    return m(b[0], attention_mask=b[1]).clone()


def test_ema_weights_context():
    P = util.pkg()
    d, sd, batches = _batches()
    a = util.build_showo(d, sd).train()
    b = util.build_showo(d, sd).train()
    ta = P.Trainer(a, lr=1e-3, ema=0.5)
    tb = P.Trainer(b, lr=1e-3, ema=0.5)
    for i in range(3):
        _step(ta, d, batches[i])
        _step(tb, d, batches[i])
    before, shadows = _snap(tb), _shadows(tb)
    raw = _logits(b, batches[0])
    # a second model loaded with the shadows as its weights
    c = util.build_showo(d, sd)
    c.load_state_dict({n: torch.from_numpy(s).view(p.shape) for (n, p), s in zip(tb.params, shadows)}, strict=True)
    want = _logits(c, batches[0])
    with tb.ema_weights():
        got = _logits(b, batches[0])
        assert _same_lists(_snap(tb), shadows) and _same_lists(_shadows(tb), before)  # exchanged in place
        with pytest.raises(RuntimeError, match="ema_weights"):
            _step(tb, d, batches[0])
        with pytest.raises(RuntimeError, match="ema_weights"):
            tb.state_dict()
        with pytest.raises(RuntimeError, match="ema_weights"):
            with tb.ema_weights():
                pass
        assert tb._in_ema  # the refusals left the context as it was
    assert torch.equal(got, want) and not torch.equal(got, raw)
    assert _same_lists(_snap(tb), before) and _same_lists(_shadows(tb), shadows)
    assert torch.equal(_logits(b, batches[0]), raw)
    # an exception raised inside still restores
    with pytest.raises(KeyError):
        with tb.ema_weights():
            raise KeyError("boom")
    assert not tb._in_ema and _same_lists(_snap(tb), before) and _same_lists(_shadows(tb), shadows)
    assert torch.equal(_logits(b, batches[0]), raw)
    # one more step: the twin that never entered the context gets the same bits
    la, lb = _step(ta, d, batches[1]), _step(tb, d, batches[1])
    assert torch.equal(la, lb)
    assert _same_lists(_snap(ta), _snap(tb)) and _same_lists(_shadows(ta), _shadows(tb))
    assert ta.ema.optimization_step == tb.ema.optimization_step == 4
    with pytest.raises(RuntimeError, match="ema="):
        with P.Trainer(c.train(), lr=1e-3).ema_weights():
            pass


def test_checkpoint_carries_the_shadows():
    P = util.pkg()
    d, sd, batches = _batches()
    a = util.build_showo(d, sd).train()
    ta = P.Trainer(a, lr=1e-3, ema=WARM)
    for i in range(5):
        _step(ta, d, batches[i % 3])
    b = util.build_showo(d, sd).train()
    tb = P.Trainer(b, lr=1e-3, ema=WARM)
    for i in range(3):
        _step(tb, d, batches[i % 3])
    st = tb.state_dict()
    assert list(st["ema"]) == ["decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power",
                               "shadow_params"]
    assert st["ema"]["optimization_step"] == 3
    assert all(x.data_ptr() != y.data_ptr() for x, y in zip(st["ema"]["shadow_params"], tb.ema.shadow_params))  # cloned
    weights = {n: p.detach().clone() for n, p in b.state_dict().items()}
    c = util.build_showo(d, sd).train()
    c.load_state_dict(weights, strict=True)
    tc = P.Trainer(c, lr=5e-4, ema={"decay": 0.1})
    tc.load_state_dict(st)
    assert tc.ema.optimization_step == 3 and tc.ema.decay == 0.999 and tc.ema.use_ema_warmup is True and tc.ema.update_after_step == 1
    assert _same_lists(_shadows(tc), _shadows(tb))
    for i in range(3, 5):
        _step(tc, d, batches[i % 3])
    assert _same_lists(_snap(tc), _snap(ta)) and _same_lists(_shadows(tc), _shadows(ta))
    assert tc.ema.optimization_step == ta.ema.optimization_step == 5 and tc.ema.cur_decay_value == ta.ema.cur_decay_value
    # a file without "ema": the shadows start over from the current parameters, the count from 0
    plain = {k: v for k, v in st.items() if k != "ema"}
    tc.load_state_dict(plain)
    assert tc.ema.optimization_step == 0 and tc.ema.cur_decay_value is None and tc.step_count == 3
    assert _same_lists(_shadows(tc), _snap(tc))
    # a trainer without EMA ignores the entry
    e = util.build_showo(d, sd).train()
    te = P.Trainer(e, lr=1e-3)
    te.load_state_dict(st)
    assert te.ema is None and te.step_count == 3 and "ema" not in te.state_dict()
