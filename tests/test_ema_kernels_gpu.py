"""EMA of the weights on the device (csrc/ema.hip and the EMA instance of the multi-tensor AdamW), bit for bit against the numpy
restatement tests/ema_ref.py: the segment-table update, the in-place swap with its engine destinations, and the fused AdamW + EMA
launch through the trainer handle on the tiny model.

Every comparison here is exact: the update is three float32 operations per element with fixed rounding points, the swap moves bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ema_ref
import util
from util import dev

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 65535, 65536, 65537, 131075]  # tails of every length mod 4, one chunk exactly, chunk + 1, two chunks + 3
OFFSETS = [(0, 0), (1, 0), (0, 1), (1, 1)]  # element offsets of (shadow, parameter) from a 16-byte boundary: (0, 0) alone moves float4s
GUARD = 8  # elements between segments, never written


def L():
    return util.lib()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _layout(shift):
    """segment i: its shadow at s_at[i], its parameter at p_at[i] inside ONE float32 buffer, OFFSETS[(i + shift) % 4] elements past a
    16-byte boundary, guard words around every range"""
    at, s_at, p_at = GUARD + 4, [], []
    for i, n in enumerate(SIZES):
        so, po = OFFSETS[(i + shift) % 4]
        at = (at + 3) // 4 * 4
        s_at.append(at + so)
        at = (s_at[-1] + n + GUARD + 3) // 4 * 4
        p_at.append(at + po)
        at = p_at[-1] + n + GUARD
    return s_at, p_at, at + GUARD


def _fill(shift, seed):
    s_at, p_at, total = _layout(shift)
    rs = np.random.RandomState(seed)
    host = (1000.0 + np.arange(total)).astype(np.float32)  # guard words: every one its own value
    for i, n in enumerate(SIZES):
        s = rs.randn(n).astype(np.float32)
        host[s_at[i]:s_at[i] + n] = s
        host[p_at[i]:p_at[i] + n] = (s + 0.05 * rs.randn(n)).astype(np.float32)
    # a NaN and an inf in p, in an averaging segment and in a copying one, on the float4 path and on the scalar one
    for i in (3, 4, 6, 7):
        host[p_at[i] + SIZES[i] // 2] = np.nan
        host[p_at[i] + SIZES[i] - 1] = np.inf if i % 2 else -np.inf
    return host, s_at, p_at


MODES = [0, 1, 0, 0, 1, 0, 0, 1]


def _want(host, s_at, p_at, decay):
    want = host.copy()
    for i, n in enumerate(SIZES):
        want[s_at[i]:s_at[i] + n] = ema_ref.step(host[s_at[i]:s_at[i] + n], host[p_at[i]:p_at[i] + n], decay, trains=not MODES[i])
    return want


def _same(got, want):
    """equal bits, except that a NaN need only be a NaN (its payload is the hardware's)"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_table_update_matches_the_restatement(shift):
    T = util.pkg().training_utils.EmaTable
    host, s_at, p_at = _fill(shift, seed=shift)
    assert all((s_at[i] % 4, p_at[i] % 4) == OFFSETS[(i + shift) % 4] for i in range(len(SIZES)))
    for decay in (0.0, 0.5, 0.9999, 1.0):
        runs = []
        for _ in range(2):
            buf = dev(host)
            assert buf.data_ptr() % 16 == 0
            tab = T([buf[a:a + n] for a, n in zip(s_at, SIZES)], [buf[a:a + n] for a, n in zip(p_at, SIZES)])
            tab.update(1 - decay, MODES)
            torch.cuda.synchronize()
            runs.append(buf.cpu().numpy())
            tab.close()
        want = _want(host, s_at, p_at, decay)
        assert _same(runs[0], want), (shift, decay)  # shadows as restated; parameters and guard words untouched
        assert np.array_equal(_bits(runs[0]), _bits(runs[1])), (shift, decay)
        for i in (3, 4, 6, 7):  # the special values did reach the shadows
            assert not np.isfinite(want[s_at[i] + SIZES[i] - 1])
    # modes NULL = every segment averages; a second call with other modes re-uploads them
    buf = dev(host)
    tab = T([buf[a:a + n] for a, n in zip(s_at, SIZES)], [buf[a:a + n] for a, n in zip(p_at, SIZES)])
    tab.update(0.5)
    tab.update(0.5, [1] * len(SIZES))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    for i, n in enumerate(SIZES):
        assert _same(got[s_at[i]:s_at[i] + n], host[p_at[i]:p_at[i] + n]), i


@pytest.mark.parametrize("offsets", OFFSETS)
def test_update_keeps_three_roundings_where_an_fma_would_show(offsets):
    T = util.pkg().training_utils.EmaTable
    s, p = ema_ref.contraction_draw()
    n = s.size
    want, fused = ema_ref.step(s, p, 0.9999), ema_ref.step_contracted(s, p, 0.9999)
    frac = float((_bits(want) != _bits(fused)).mean())
    print(f"[ema] an fma would change {100 * frac:.2f} % of {n} elements")
    assert frac >= 0.01
    buf = dev(np.zeros(2 * n + 64, dtype=np.float32))
    a, b = 4 + offsets[0], (4 + n + 8 + 3) // 4 * 4 + offsets[1]
    buf[a:a + n].copy_(torch.from_numpy(s))
    buf[b:b + n].copy_(torch.from_numpy(p))
    T([buf[a:a + n]], [buf[b:b + n]]).update(1 - 0.9999)
    torch.cuda.synchronize()
    got = buf[a:a + n].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())


@pytest.mark.parametrize("shift", [0, 1])
def test_swap_exchanges_in_place_and_writes_the_images(shift):
    T = util.pkg().training_utils.EmaTable
    s_at, p_at, total = _layout(shift)
    rs = np.random.RandomState(7 + shift)
    host = (1000.0 + np.arange(total)).astype(np.float32)
    for i, n in enumerate(SIZES):
        host[s_at[i]:s_at[i] + n] = rs.randn(n)
        host[p_at[i]:p_at[i] + n] = rs.randn(n)
    buf = dev(host)
    # destinations: bf16 for segments 0, 3, 6 (8-byte aligned or not), fp32 for 1, 4, 7 (16-byte aligned or not), none for 2, 5
    d16 = dev(np.full(sum(SIZES) + 64, 0x7F7F, dtype=np.int16))
    d32 = dev(np.full(sum(SIZES) + 64, -7.0, dtype=np.float32))
    dst16, dst32, at16, at32 = [], [], 4, 4
    for i, n in enumerate(SIZES):
        k = i % 3
        o = (i + shift) % 2
        dst16.append(d16[at16 + o:at16 + o + n] if k == 0 else None)
        dst32.append(d32[at32 + o:at32 + o + n] if k == 1 else None)
        at16 += (n + 12) // 4 * 4 if k == 0 else 0
        at32 += (n + 12) // 4 * 4 if k == 1 else 0
    tab = T([buf[a:a + n] for a, n in zip(s_at, SIZES)], [buf[a:a + n] for a, n in zip(p_at, SIZES)], dst16, dst32)
    d16_0, d32_0 = d16.cpu().numpy().copy(), d32.cpu().numpy().copy()

    def check(cur, p_src, s_src):
        want = host.copy()
        w16, w32 = d16_0.copy(), d32_0.copy()
        for i, n in enumerate(SIZES):
            newp = host[p_src[i]:p_src[i] + n]
            want[p_at[i]:p_at[i] + n] = newp
            want[s_at[i]:s_at[i] + n] = host[s_src[i]:s_src[i] + n]
            if dst16[i] is not None:
                o = (dst16[i].data_ptr() - d16.data_ptr()) // 2
                w16[o:o + n] = util.to_bf16_bits(torch.from_numpy(newp.copy())).numpy()
            if dst32[i] is not None:
                o = (dst32[i].data_ptr() - d32.data_ptr()) // 4
                w32[o:o + n] = newp
        assert np.array_equal(_bits(cur), _bits(want))  # guard words included
        assert np.array_equal(d16.cpu().numpy(), w16) and np.array_equal(_bits(d32.cpu().numpy()), _bits(w32))

    tab.swap()
    torch.cuda.synchronize()
    check(buf.cpu().numpy(), s_at, p_at)  # p holds the old s and the other way round; every image is the cast of the new p
    tab.swap()
    torch.cuda.synchronize()
    check(buf.cpu().numpy(), p_at, s_at)  # every bit restored, images of the restored p


# ---------------------------------------------------------------- fused AdamW + EMA through the trainer handle

SPLIT = (2, 1, 2)
HP = (1e-3, 0.9, 0.999, 1e-8, 0.01)
DECAYS = (0.5, 0.9999)


def _tiny_batch():
    g = util.golden("showo_tiny_forward.npz")
    return dev(torch.from_numpy(g["train_ids"]).long()), dev(g["train_mask"]), dev(torch.from_numpy(g["train_labels"]).long())


def _backward(m, batch, msl):
    P = util.pkg()
    ids, mask, labels = batch
    tr = m.trainer()
    P.modeling_showo.sync_trainable(m, tr, {n: bool(p.requires_grad) for n, p in m.named_parameters()}, False)
    dm = P.training.train_mask(tr, mask)
    B, Lq = ids.shape
    losses = torch.empty(3, dtype=torch.float32, device="cuda")
    try:
        L().call("showo_train_forward", tr, L().ptr(ids), L().ptr(dm), L().ptr(labels), B, Lq, *SPLIT, msl, None, L().ptr(losses), L().stream())
    finally:
        L().call("showo_trainer_use_intervals", tr, None, None)
    L().call("showo_train_backward", tr, L().ptr(labels), *SPLIT, msl, 1.0, 0.1, 1.0, L().stream())
    return tr


def _optimizer_steps(with_ema):
    """two forward / backward / showo_train_adamw_step rounds on a fresh tiny model through the C ABI; with_ema: shadows bound and
    1 - decay announced before each step.  Returns CPU copies: parameters, moments, shadows, the logits of the final engine images,
    and the parameters after each step."""
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd).train()
    batch = _tiny_batch()
    named = list(m.named_parameters())
    mom = {n: (torch.zeros_like(p), torch.zeros_like(p)) for n, p in named}
    gen = torch.Generator(device="cuda").manual_seed(3)
    shadows = {n: (p.detach() + 0.01 * torch.randn(p.shape, device="cuda", generator=gen)) for n, p in named}
    start = {n: s.cpu().numpy().copy() for n, s in shadows.items()}
    per_step = []
    for step, decay in enumerate(DECAYS, 1):
        tr = _backward(m, batch, d.max_text_len)
        if step == 1:
            for n, p in named:
                L().call("showo_train_bind_param", tr, n.encode(), p.data_ptr(), mom[n][0].data_ptr(), mom[n][1].data_ptr(), p.numel())
                if with_ema:
                    L().call("showo_train_bind_ema", tr, n.encode(), shadows[n].data_ptr(), p.numel())
        if with_ema:
            L().call("showo_train_set_ema", tr, 1 - decay)
        L().call("showo_train_adamw_step", tr, *HP, step, L().stream())
        torch.cuda.synchronize()
        per_step.append({n: p.detach().cpu().numpy().copy() for n, p in named})
    if with_ema:  # the announcement is for one step: a third step without one leaves the shadows alone
        keep = {n: s.clone() for n, s in shadows.items()}
        _backward(m, batch, d.max_text_len)
        L().call("showo_train_adamw_step", m.trainer(), *HP, 3, L().stream())
        torch.cuda.synchronize()
        assert all(torch.equal(keep[n], shadows[n]) for n in keep)
        assert any(not np.array_equal(per_step[-1][n], p.detach().cpu().numpy()) for n, p in named)
    else:
        _backward(m, batch, d.max_text_len)
        L().call("showo_train_adamw_step", m.trainer(), *HP, 3, L().stream())
    logits = m.eval()(batch[0], attention_mask=batch[1]).float().cpu()
    return dict(params={n: p.detach().cpu() for n, p in named}, m={n: mom[n][0].cpu() for n in mom}, v={n: mom[n][1].cpu() for n in mom},
                shadows={n: s.cpu() for n, s in shadows.items()}, start=start, per_step=per_step, logits=logits)


def test_fused_adamw_ema_keeps_adamw_bits_and_updates_the_shadows():
    plain, fused = _optimizer_steps(False), _optimizer_steps(True)
    for n in plain["params"]:
        assert torch.equal(plain["params"][n], fused["params"][n]), n
        assert torch.equal(plain["m"][n], fused["m"][n]) and torch.equal(plain["v"][n], fused["v"][n]), n
    assert torch.equal(plain["logits"], fused["logits"])  # the engine's weight images carry the same bits
    # shadows: the plain step followed by the table update (the restatement, over the parameters after each step) ...
    for n, s0 in fused["start"].items():
        want = s0
        for decay, params in zip(DECAYS, plain["per_step"]):
            want = ema_ref.step(want, params[n], decay)
        assert np.array_equal(_bits(want), _bits(fused["shadows"][n].numpy())), n
    # ... and the table kernel itself says the same
    T = util.pkg().training_utils.EmaTable
    names = list(fused["start"])
    sh = [dev(fused["start"][n]) for n in names]
    for decay, params in zip(DECAYS, plain["per_step"]):
        ps = [dev(params[n]) for n in names]
        T(sh, ps).update(1 - decay)
        torch.cuda.synchronize()
    for n, s in zip(names, sh):
        assert torch.equal(s.cpu(), fused["shadows"][n]), n


def test_trainer_handle_refuses_an_ema_step_without_shadows_and_swaps_back():
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd).train()
    batch = _tiny_batch()
    tr = _backward(m, batch, d.max_text_len)
    named = list(m.named_parameters())
    mom = {n: (torch.zeros_like(p), torch.zeros_like(p)) for n, p in named}
    for n, p in named:
        L().call("showo_train_bind_param", tr, n.encode(), p.data_ptr(), mom[n][0].data_ptr(), mom[n][1].data_ptr(), p.numel())
    with pytest.raises(RuntimeError, match="no shadow bound"):
        L().call("showo_train_ema_swap", tr, L().stream())
    L().call("showo_train_set_ema", tr, 0.5)
    with pytest.raises(RuntimeError, match="no shadow bound"):
        L().call("showo_train_adamw_step", tr, *HP, 1, L().stream())
    with pytest.raises(RuntimeError):
        L().call("showo_train_set_ema", tr, 1.5)
    with pytest.raises(RuntimeError, match="no bound parameter"):
        L().call("showo_train_bind_ema", tr, b"showo.nope", named[0][1].data_ptr(), 1)
    # shadows = 2 x the parameters: the swap doubles every weight, the logits change, the second swap restores both
    shadows = {n: (2 * p.detach()).contiguous() for n, p in named}
    for n, p in named:
        L().call("showo_train_bind_ema", tr, n.encode(), shadows[n].data_ptr(), p.numel())
    before = {n: p.detach().clone() for n, p in named}
    m.eval()
    l0 = m(batch[0], attention_mask=batch[1]).clone()
    L().call("showo_train_ema_swap", tr, L().stream())
    l1 = m(batch[0], attention_mask=batch[1]).clone()
    for n, p in named:
        assert torch.equal(p.detach(), 2 * before[n]) and torch.equal(shadows[n], before[n]), n
    assert not torch.equal(l0, l1)
    L().call("showo_train_ema_swap", tr, L().stream())
    l2 = m(batch[0], attention_mask=batch[1])
    for n, p in named:
        assert torch.equal(p.detach(), before[n]) and torch.equal(shadows[n], 2 * before[n]), n
    assert torch.equal(l0, l2)


def _child_shadows(path):
    out = _optimizer_steps(True)
    torch.save({"shadows": out["shadows"], "params": out["params"]}, path)


def test_per_tensor_fallback_gives_the_same_shadows_in_a_child_process(tmp_path):
    """SHOWO_TRAIN_ADAMW_MULTI=0 (read once per process): per-tensor AdamW, then the table update over the trainable tensors.
    The per-tensor kernel is the one whose text this feature did not touch, so equal parameters here also pin both instances of the
    multi-tensor kernel (the test above holds them equal to each other) to the bits from before AdamSeg grew its shadow field."""
    env = dict(os.environ, SHOWO_TRAIN_ADAMW_MULTI="0")
    here = os.path.dirname(os.path.abspath(__file__))
    path = str(tmp_path / "fallback.pt")
    code = ("import sys; sys.path.insert(0, %r); import test_ema_kernels_gpu as t; t._child_shadows(%r); print('CHILD_OK')" % (here, path))
    r = subprocess.run([sys.executable, "-s", "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    child = torch.load(path, weights_only=True)
    fused = _optimizer_steps(True)
    for n in fused["shadows"]:
        assert torch.equal(child["params"][n], fused["params"][n]), n
        assert torch.equal(child["shadows"][n], fused["shadows"][n]), n
