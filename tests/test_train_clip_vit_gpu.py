"""Native training step of the CLIP-ViT model (reference training/train_w_clip_vit.py:598-639): `Trainer(projector=True).step_clip_vit`.

Kernel level: the splice (layer 0's input in one launch), the gather of the placeholder rows of the layer-0 data gradient and the table
scatter that leaves the placeholder positions out, against torch constructions and against showo_embed_f32 / showo_embed_bwd[_acc] on
the compacted token list, bit for bit.

Trainer level: the yardstick is the autograd path on the same model and batch -- embed_tokens + mm_projector + cat ->
Showo.forward(input_embeddings=..., labels=...) -> backward -- which tests/test_train_gpu.py pins to the oracle.  It is run ONCE per
geometry (`_case`) and shared, unchanged, by the tests that need it."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import util
from util import O, Wt, dev

pytestmark = pytest.mark.gpu

W = (1.0, 0.1, 1.0)  # the reference's loss weights
EMBED = "showo.model.embed_tokens.weight"
IMG_START = 2  # llava_pretrain: the image rows follow <|mmu|> <|soi|> (training/train_w_clip_vit.py:538-541)


def L():
    return util.lib()


def S():
    return util.lib().stream()


def _same_bits(a, b):
    """torch.equal that also holds for NaN (an empty loss group is 0 / 0 on both sides)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ================================================================ kernel level

KB, KL, KP, KV = 3, 40, 24, 37
SPLICE_CASES = {
    "n=0": (0, []),
    "n=B, a start at 0, a start with start+P == L": (3, [3, 0, KL - KP]),
    "n=2, different starts": (2, [5, 11]),
}


def _kernel_batch(H, n, starts, seed=0):
    g = torch.Generator().manual_seed(seed + H)
    ids = torch.randint(0, KV - 5, (KB, KL), generator=g)  # the last five table rows are named by no id
    ids.view(-1)[::3] = 7  # a heavily repeated id: runs beyond the scatter's 8-row unrolled loop and its tail
    live = torch.ones(KB, KL, dtype=torch.bool)
    for j, st in enumerate(starts):
        b = KB - n + j
        live[b, st:st + KP] = False
        ids[b, st:st + KP:2] = -1  # placeholder ids are never read: out-of-range values on purpose
        ids[b, st + 1:st + KP:2] = KV + 5
    table = torch.randn(KV, H, generator=g)
    rows = torch.randn(max(n, 1) * KP, H, generator=g)
    dx = torch.randn(KB * KL, H, generator=g)
    assert int(torch.bincount(ids[live]).max()) > 8
    return ids, live, table, rows, dx


@pytest.mark.parametrize("H", [128, 2048])
@pytest.mark.parametrize("case", list(SPLICE_CASES))
def test_splice_gather_scatter_kernels(case, H):
    n, starts = SPLICE_CASES[case]
    ids, live, table, rows, dx = _kernel_batch(H, n, starts)
    T = KB * KL
    d_ids, d_table, d_rows, d_dx = dev(ids), dev(table), dev(rows), dev(dx)
    d_start = dev(torch.tensor(starts + [0] * (1 if n == 0 else 0), dtype=torch.int32))
    # ---- splice = embedding + cat, bit for bit
    x = torch.full((T, H), float("nan"), device="cuda")
    L().call("showo_embed_splice_f32", L().ptr(d_ids), L().ptr(d_table), L().ptr(d_rows), L().ptr(d_start), L().ptr(x), KB, KL, n, KP, H, KV, S())
    emb = torch.nn.functional.embedding(d_ids.clamp(0, KV - 1), d_table)
    want = []
    for b in range(KB):
        j = b - (KB - n)
        if j < 0:
            want.append(emb[b])
        else:
            st = starts[j]
            want.append(torch.cat([emb[b, :st], d_rows[j * KP:(j + 1) * KP], emb[b, st + KP:]], dim=0))
    want = torch.stack(want).view(T, H)
    assert torch.isfinite(x).all()
    assert torch.equal(x, want)
    if n == 0:  # ... and showo_embed_f32 on every bit, its NaN rows for out-of-range ids included
        bad = d_ids.clone()
        bad[1, 4], bad[2, 39] = -3, KV
        x0, x1 = torch.zeros((T, H), device="cuda"), torch.ones((T, H), device="cuda")
        L().call("showo_embed_f32", L().ptr(bad), L().ptr(d_table), L().ptr(x0), T, H, KV, S())
        L().call("showo_embed_splice_f32", L().ptr(bad), L().ptr(d_table), None, None, L().ptr(x1), KB, KL, 0, KP, H, KV, S())
        assert _same_bits(x0, x1) and int(torch.isnan(x1).any(1).sum()) == 2
    # ---- gather = torch indexing
    if n:
        out = torch.full((n * KP, H), float("nan"), device="cuda")
        L().call("showo_gather_splice_rows_f32", L().ptr(d_dx), L().ptr(d_start), L().ptr(out), KB, KL, n, KP, H, S())
        want_rows = torch.cat([d_dx.view(KB, KL, H)[KB - n + j, st:st + KP] for j, st in enumerate(starts)], dim=0)
        assert torch.equal(out, want_rows)
    # ---- scatter = showo_embed_bwd[_acc] on the compacted token list, in both accumulate modes
    keep = live.view(-1).cuda()
    c_ids, c_dx = d_ids.view(-1)[keep].contiguous(), d_dx[keep].contiguous()
    M = int(keep.sum())
    assert M == T - n * KP
    ws, ws_c = torch.zeros(2 * T, dtype=torch.int32, device="cuda"), torch.zeros(2 * T, dtype=torch.int32, device="cuda")
    named = torch.zeros(KV, dtype=torch.bool)
    named[ids[live]] = True
    assert int((~named).sum()) >= 5
    old = torch.randn(KV, H, device="cuda")
    for accumulate in (0, 1):
        got, ref = old.clone(), old.clone()
        L().call("showo_embed_bwd_acc", L().ptr(c_ids), L().ptr(c_dx), L().ptr(ref), L().ptr(ws_c), accumulate, M, H, KV, S())
        L().call("showo_embed_bwd_splice", L().ptr(d_ids), L().ptr(d_dx), L().ptr(got), L().ptr(ws), L().ptr(d_start), accumulate, KB, KL, n, KP,
                 H, KV, S())
        assert torch.isfinite(got).all()
        assert torch.equal(got, ref), accumulate
        assert torch.equal(got[~named.cuda()], old[~named.cuda()])  # rows no live id names keep their previous contents
        assert not torch.equal(got[named.cuda()], old[named.cuda()])
    zero, ref0 = torch.zeros(KV, H, device="cuda"), torch.zeros(KV, H, device="cuda")
    L().call("showo_embed_bwd", L().ptr(c_ids), L().ptr(c_dx), L().ptr(ref0), L().ptr(ws_c), M, H, KV, S())
    L().call("showo_embed_bwd_splice", L().ptr(d_ids), L().ptr(d_dx), L().ptr(zero), L().ptr(ws), L().ptr(d_start), 0, KB, KL, n, KP, H, KV, S())
    assert torch.equal(zero, ref0)
    util.release()


def test_two_range_clip_norm_is_one_norm():
    """showo_grad_clip_norm2: one norm over both ranges (fp64 reference), both scaled by the one coefficient; an empty second range
    gives showo_grad_clip_norm's bits"""
    torch.manual_seed(2)
    a, b = torch.randn(100003 + 1, device="cuda")[:100003], torch.randn(4099, device="cuda")
    nws = L().load().showo_grad_clip_ws_doubles()
    ws = torch.empty(2 * nws, dtype=torch.float64, device="cuda")
    want = float(torch.sqrt((a.double() ** 2).sum() + (b.double() ** 2).sum()))
    a2, b2, out2 = a.clone(), b.clone(), torch.zeros(2, device="cuda")
    L().call("showo_grad_clip_norm2", a2.data_ptr(), a2.numel(), b2.data_ptr(), b2.numel(), 1.0, L().ptr(ws), L().ptr(out2), S())
    assert abs(float(out2[0]) - want) <= 1e-6 * want
    c = out2[1]
    assert torch.equal(a2, a * c) and torch.equal(b2, b * c) and float(c) < 1.0
    a3, a4, o3, o4 = a.clone(), a.clone(), torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda")
    L().call("showo_grad_clip_norm", a3.data_ptr(), a3.numel(), 1.0, L().ptr(ws), L().ptr(o3), S())
    L().call("showo_grad_clip_norm2", a4.data_ptr(), a4.numel(), None, 0, 1.0, L().ptr(ws), L().ptr(o4), S())
    assert torch.equal(o3, o4) and torch.equal(a3, a4)


# ================================================================ trainer level

GEOMETRIES = {
    # T < 256: the trainer's fallback kernels
    "tiny": dict(dims=Wt.TINY, B=3, n_img=16, n_txt=11, split=(0, 1, 2), max_batch=8, max_seq=128),
    # T = 12 x 40 = 480 >= 256: the production branch (fused save-form projection, gemm2p / gemm3w)
    "small": dict(dims=Wt.SMALL, B=12, n_img=24, n_txt=16, split=(2, 2, 8), max_batch=12, max_seq=40),
}


def _state(geo):
    d = Wt.ShowoDims(**dict(GEOMETRIES[geo]["dims"], w_clip_vit=True))
    sd = Wt.make_showo_state(d, seed=11)
    for k, v in Wt.make_projector_state(1024, d.hidden, seed=5).items():
        sd["mm_projector." + k] = v
    return d, sd


def _model(geo):
    d, sd = _state(geo)
    g = GEOMETRIES[geo]
    return util.build_showo(d, sd, max_batch=g["max_batch"], max_seq=g["max_seq"]).train()


def _batch(geo, seed=4):
    """the image rows sit on the mmu sequences only: the first B - n sequences are plain ids at full length"""
    g = GEOMETRIES[geo]
    d, _ = _state(geo)
    B, P, n_txt, n = g["B"], g["n_img"], g["n_txt"], g["split"][2]
    Lq = P + n_txt
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, d.llm_vocab, (B, Lq), generator=gen)
    labels = torch.where(torch.rand(B, Lq, generator=gen) < 0.3, torch.full((B, Lq), -100), torch.randint(0, d.llm_vocab, (B, Lq), generator=gen))
    txt = torch.randint(0, d.llm_vocab, (n, n_txt), generator=gen)
    lab = torch.cat([torch.full((n, IMG_START), -100), torch.randint(0, d.llm_vocab, (n, n_txt - IMG_START), generator=gen)], dim=1)
    ids[B - n:], labels[B - n:] = util.pkg().training_utils.splice_image_columns(txt, lab, IMG_START, P, 0)
    feats = torch.randn(n, P, 1024, generator=gen)
    mask = O.mask_mmu_vit(B, Lq, system_prompt_len=0)
    return dict(ids=ids.cuda(), labels=labels.cuda(), feats=feats.cuda(), mask=mask.cuda(), n=n, P=P, split=g["split"], msl=d.max_text_len)


def _autograd_step(m, bt):
    """the parent path: embed_tokens + mm_projector + cat -> Showo.forward(input_embeddings=..., labels=...) -> backward"""
    m.zero_grad(set_to_none=True)
    n, P, B = bt["n"], bt["P"], bt["ids"].shape[0]
    txt = m.showo.model.embed_tokens(bt["ids"])
    img = m.mm_projector(bt["feats"])
    e = torch.cat([txt[:B - n], torch.cat([txt[B - n:, :IMG_START], img, txt[B - n:, IMG_START + P:]], dim=1)], dim=0)
    e.retain_grad()
    s = bt["split"]
    losses = m(None, input_embeddings=e, attention_mask=bt["mask"], labels=bt["labels"], batch_size_t2i=s[0], batch_size_lm=s[1],
               batch_size_mmu=s[2], max_seq_length=bt["msl"])[1:]
    sum(w * l for w, l in zip(W, losses)).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    return torch.stack([l.detach() for l in losses]), grads, e.grad.detach().clone()


@functools.lru_cache(maxsize=None)
def _case(geo):
    """(batch, losses, gradients by state-dict key, input gradient) of the autograd path: computed once, never written"""
    bt = _batch(geo)
    m = _model(geo)
    losses, grads, ge = _autograd_step(m, bt)
    del m
    return bt, losses, grads, ge


def _native_step(tr, bt):
    s = bt["split"]
    return tr.step_clip_vit(bt["ids"], bt["feats"], IMG_START, bt["mask"], bt["labels"], s[0], s[1], s[2], bt["msl"])


def _grad_view(m, name):
    ptr, n = C.c_void_p(), C.c_int64()
    L().call("showo_train_grad", m._trainer, name.encode(), C.byref(ptr), C.byref(n))
    return util.pkg().training.device_view(ptr.value, n.value, "cuda")


def _native_grads(m, tr):
    torch.cuda.synchronize()
    out = {k: _grad_view(m, k).clone().view(p.shape) for k, p in m.named_parameters() if k.startswith("showo.")}
    out.update({k: v.clone() for k, v in tr.projector_grads().items()})
    return out


def _counters(m, reset=False):
    out = (C.c_int64 * 6)()
    L().call("showo_train_counters", m._trainer, C.cast(out, C.c_void_p), int(reset))
    return dict(zip(("wgrad", "dgrad", "phases", "embed", "transposes", "fused"), list(out)))


@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_step_clip_vit_gradients_are_the_autograd_paths(geo):
    P = util.pkg()
    bt, losses, grads, ge = _case(geo)
    m = _model(geo)
    tr = P.Trainer(m, lr=1e-3, coeffs=W, projector=True)
    got_losses = _native_step(tr, bt)
    assert tr.sync_gradients
    got = _native_grads(m, tr)
    assert _same_bits(got_losses, losses), (got_losses, losses)
    assert set(got) == set(grads)
    for k in grads:  # the same kernels on the same bits
        if k != EMBED:
            assert torch.equal(got[k], grads[k]), k
    # the table: bit-equal to showo_embed_bwd on the compacted token list of the returned input gradient ...
    B, Lq = bt["ids"].shape
    live = torch.ones(B, Lq, dtype=torch.bool, device="cuda")
    live[B - bt["n"]:, IMG_START:IMG_START + bt["P"]] = False
    c_ids = bt["ids"][live].contiguous()
    c_dx = ge.float().view(B * Lq, -1)[live.view(-1)].contiguous()
    dE = torch.zeros_like(got[EMBED])
    ws = torch.zeros(2 * c_ids.numel(), dtype=torch.int32, device="cuda")
    L().call("showo_embed_bwd", L().ptr(c_ids), L().ptr(c_dx), L().ptr(dE), L().ptr(ws), c_ids.numel(), dE.shape[1], dE.shape[0], S())
    assert torch.equal(got[EMBED], dE)
    # ... and against the autograd path's (torch's embedding backward: same fp32 terms, another summation order) at the bound of
    # test_training_from_input_embeddings_equals_training_from_ids
    err = float((got[EMBED] - grads[EMBED]).abs().max())
    print(f"[clip_vit] {geo}: table gradient vs autograd max err {err:.3e}, scale {float(grads[EMBED].abs().max()):.3e}")
    assert err <= 1e-5 * float(grads[EMBED].abs().max()) + 1e-9
    for k, p in m.named_parameters():  # the closing call updated everything, projector included
        assert not torch.equal(p, O.to_torch(_state(geo)[1])[k].cuda()), k


def test_step_clip_vit_transpose_branch_in_a_child_process():
    """SHOWO_TRAIN_TN=0 (read once per process): the spliced forward and backward on the transpose + NT-GEMM weight-gradient form
    (tiny, T = 81 < 256); the native step and the autograd path share the trainer and stay bit-equal"""
    env = dict(os.environ, SHOWO_TRAIN_TN="0")
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); import test_train_clip_vit_gpu as t; "
            "t.test_step_clip_vit_gradients_are_the_autograd_paths('tiny'); print('CHILD_OK')" % here)
    r = subprocess.run([sys.executable, "-s", "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_projector_only_llava_pretrain(geo):
    P = util.pkg()
    bt, losses, grads, _ = _case(geo)
    m = _model(geo)
    m.showo.requires_grad_(False)  # training/train_w_clip_vit.py:201-214
    with pytest.raises(ValueError):
        P.Trainer(m)  # nothing of model.showo trains and the projector was not asked for
    tr = P.Trainer(m, lr=1e-3, coeffs=W, projector=True)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    _counters(m, reset=True)
    got_losses = _native_step(tr, bt)
    cnt = _counters(m)
    assert _same_bits(got_losses, losses)
    pg = tr.projector_grads()
    for k in P.training.PROJECTOR_KEYS:
        assert torch.equal(pg[k], grads[k]), k
    assert cnt["wgrad"] == 0 and cnt["embed"] == 0 and cnt["phases"] == m.arch["num_hidden_layers"], cnt
    for b in range(L().load().showo_train_num_buckets(m._trainer)):  # every Show-o slot of the flat buffer reads zero
        ptr, n = C.c_void_p(), C.c_int64()
        L().call("showo_train_bucket", m._trainer, b, C.byref(ptr), C.byref(n))
        assert int(torch.count_nonzero(P.training.device_view(ptr.value, n.value, "cuda"))) == 0, b
    for k, p in m.named_parameters():
        assert torch.equal(p, before[k]) == k.startswith("showo."), k


def test_projector_adamw_matches_torch():
    """one step against torch.optim.AdamW on the handed-out gradients with the reference's two groups (no decay for `bias`,
    training/train_w_clip_vit.py:226-239), at the 2e-6 of test_adamw_matches_torch"""
    P = util.pkg()
    bt = _case("tiny")[0]
    m = _model("tiny")
    hp = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
    ref = {k: p.detach().clone().requires_grad_(True) for k, p in m.named_parameters() if k.startswith("mm_projector.")}
    opt = torch.optim.AdamW([{"params": [p for k, p in ref.items() if "bias" not in k], "weight_decay": 0.01},
                             {"params": [p for k, p in ref.items() if "bias" in k], "weight_decay": 0.0}], **hp)
    tr = P.Trainer(m, weight_decay=0.01, coeffs=W, projector=True, **hp)
    _native_step(tr, bt)
    for k, g in tr.projector_grads().items():
        ref[k].grad = g.clone()
    opt.step()
    for k, p in m.named_parameters():
        if k in ref:
            err = float((p.detach() - ref[k].detach()).abs().max())
            assert err < 2e-6, k
            assert err < float((p.detach() - O.to_torch(_state("tiny")[1])[k].cuda()).abs().max())
    # the updated projector is what the next forward runs on: the HIP images follow the masters
    want = torch.nn.Sequential(torch.nn.Linear(1024, 128), torch.nn.GELU(), torch.nn.Linear(128, 128)).cuda()
    want.load_state_dict({k[len("mm_projector."):]: p.detach() for k, p in m.named_parameters() if k in ref})
    with torch.no_grad():
        a, b = m.mm_projector(bt["feats"]), want(bt["feats"])
    assert float((a - b).abs().max()) <= 3e-2 * float(b.abs().max())


def test_accumulation_window_k2():
    """a k = 2 window against its two micro-batches alone (loss weights W / 2, overwriting): the projector and table gradients (and
    every other one) at the gate of tests/test_train_accum_gpu.py, |r - (v0 + v1)| <= (k - 1) 2^-23 (|v0| + |v1|): each accumulating
    form adds ONE fp32 rounding per added micro-batch, at most 2^-24 of a magnitude of at most |v0| + |v1|; the gate is that doubled"""
    P = util.pkg()
    b0, b1 = _case("tiny")[0], _batch("tiny", seed=9)
    assert not torch.equal(b0["ids"], b1["ids"]) and not torch.equal(b0["feats"], b1["feats"])
    a = _model("tiny")
    ta = P.Trainer(a, lr=0.0, coeffs=tuple(c / 2 for c in W), projector=True)  # lr = 0: the parameters keep their bits
    start = {k: p.detach().clone() for k, p in a.named_parameters()}
    vs = []
    for bt in (b0, b1):
        _native_step(ta, bt)
        vs.append(_native_grads(a, ta))
    for k, p in a.named_parameters():
        assert torch.equal(p, start[k]), k
    b = _model("tiny")
    tb = P.Trainer(b, lr=1e-3, coeffs=W, projector=True, gradient_accumulation_steps=2)
    l0 = _native_step(tb, b0)
    assert not tb.sync_gradients
    for k, p in b.named_parameters():  # no update, of the projector or anything else, before the closing call
        assert torch.equal(p, start[k]), k
    l1 = _native_step(tb, b1)
    assert tb.sync_gradients
    r = _native_grads(b, tb)
    for k, p in b.named_parameters():
        assert not torch.equal(p, start[k]), k
    assert torch.allclose(tb.window_losses()[1:], ((l0 + l1) / 2)[1:], rtol=0, atol=1e-6)
    for k in r:
        s = vs[0][k].double() + vs[1][k].double()
        mag = vs[0][k].double().abs() + vs[1][k].double().abs()
        err = (r[k].double() - s).abs()
        bound = 2.0 ** -23 * mag
        if k == EMBED or k.startswith("mm_projector."):
            print(f"[clip_vit] accum {k}: max err / bound = {float((err / bound.clamp(min=1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), k


def test_loss_rows_labelled_keeps_projector_and_block_gradients():
    P = util.pkg()
    bt, _, grads, _ = _case("tiny")
    m = _model("tiny")
    tr = P.Trainer(m, lr=1e-3, coeffs=W, projector=True, loss_rows="labelled")
    _native_step(tr, bt)
    rows, total = tr.loss_rows_count
    assert 0 < rows < total
    got = _native_grads(m, tr)
    for k in grads:
        if k.startswith("mm_projector.") or ".layers." in k:
            assert torch.equal(got[k], grads[k]), k


def _one_rank_group():
    import os
    import socket
    import torch.distributed as dist
    if dist.is_initialized():
        return dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    return dist


def test_exchange_fp32_single_rank_keeps_every_bit():
    """force_exchange in the 1-rank RCCL group, fp32 wire: the projector's bucket goes on the wire behind the head's and the blocks';
    parameters (projector included) equal the trainer without an exchange (the pattern of test_trainer_exchange_over_rccl_single_rank)"""
    _one_rank_group()
    P = util.pkg()
    bt = _case("tiny")[0]
    a, b = _model("tiny"), _model("tiny")
    ta = P.Trainer(a, lr=1e-3, coeffs=W, projector=True)
    tb = P.Trainer(b, lr=1e-3, coeffs=W, projector=True, wire="fp32", force_exchange=True)
    assert ta.exchange is None and tb.exchange is not None and tb.exchange.world == 1
    assert len(tb.buckets) == a.arch["num_hidden_layers"] + 3 and tb.buckets[-1].numel() >= sum(p.numel() for p in a.mm_projector.parameters())
    for _ in range(2):
        la, lb = _native_step(ta, bt), _native_step(tb, bt)
    assert _same_bits(la, lb)
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q), k


def test_clipping_takes_one_norm_over_showo_and_projector():
    """max_grad_norm: grad_norm = the fp64 norm over ALL gradients of the (unclipped) autograd path, projector included, at the 1e-3
    of test_trainer_gradient_clipping_matches_torch; both ranges come out scaled by the same coefficient c = max / (norm + 1e-6):
    elementwise clipped / unclipped = c (1 + e), |e| <= 2^-22 -- one fp32 rounding of the product (2^-24), of the sum norm + 1e-6
    (2^-24) and of the quotient (up to 2^-23 where the division is not correctly rounded)"""
    P = util.pkg()
    bt, _, grads, _ = _case("tiny")
    want = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))
    mx = float(np.float32(want / 2))  # exactly representable: the library takes max_norm as a float
    m = _model("tiny")
    tr = P.Trainer(m, lr=1e-3, coeffs=W, projector=True, max_grad_norm=mx)
    _native_step(tr, bt)
    total = float(tr.grad_norm)
    print(f"[clip_vit] grad_norm {total:.6e}, fp64 norm over all gradients {want:.6e}")
    assert abs(total - want) <= 1e-3 * want
    showo_only = float(torch.sqrt(sum((g.double() ** 2).sum() for k, g in grads.items() if k.startswith("showo."))))
    print(f"[clip_vit] norm over the Show-o gradients alone {showo_only:.6e}")
    assert abs(total - want) < abs(total - showo_only)  # the norm found is the one that includes the projector's gradients
    got = _native_grads(m, tr)
    after = float(torch.sqrt(sum((b.double() ** 2).sum() for b in tr.buckets)))
    assert abs(after - mx) <= 1e-3 * mx
    c = mx / (total + 1e-6)
    for k in grads:
        if k == EMBED:
            continue  # (bit-equal to the autograd path's only up to the summation order: checked through the norm above)
        big = grads[k].abs() > 1e-20
        ratio = got[k][big].double() / grads[k][big].double()
        assert float((ratio / c - 1).abs().max()) <= 2.0 ** -22, k


def test_frozen_projector_tensor_stays_zero_through_a_window_and_out_of_the_norm():
    """one projector tensor frozen, k = 2, max_grad_norm set: the frozen slot reads zero after every micro-batch (it is part of the
    exchange bucket and of the clipping norm), grad_norm is the fp64 norm over the TRAINABLE gradients of the window -- the sum of the
    two micro-batches' gradients at loss weights W / 2, taken alone from an all-trainable trainer at lr = 0 -- at the 1e-3 of
    test_trainer_gradient_clipping_matches_torch, the trainable projector gradients of a micro-batch keep their bits, and the frozen
    tensor is not updated"""
    P = util.pkg()
    frozen = "mm_projector.0.weight"
    b0, b1 = _case("tiny")[0], _batch("tiny", seed=9)
    a = _model("tiny")
    ta = P.Trainer(a, lr=0.0, coeffs=tuple(c / 2 for c in W), projector=True)
    vs = []
    for bt in (b0, b1):
        _native_step(ta, bt)
        vs.append(_native_grads(a, ta))
    want = float(torch.sqrt(sum(((vs[0][k].double() + vs[1][k].double()) ** 2).sum() for k in vs[0] if k != frozen)))
    with_frozen = float(torch.sqrt(sum(((vs[0][k].double() + vs[1][k].double()) ** 2).sum() for k in vs[0])))
    mx = float(np.float32(want / 2))
    b = _model("tiny")
    b.mm_projector[0].weight.requires_grad_(False)
    start = {k: p.detach().clone() for k, p in b.named_parameters()}
    tb = P.Trainer(b, lr=1e-3, coeffs=W, projector=True, gradient_accumulation_steps=2, max_grad_norm=mx)
    _native_step(tb, b0)
    torch.cuda.synchronize()
    pg = tb.projector_grads()
    assert int(torch.count_nonzero(pg[frozen])) == 0
    for k in P.training.PROJECTOR_KEYS:  # the first micro-batch alone: the trainable tensors' bits do not depend on what is frozen
        if k != frozen:
            assert torch.equal(pg[k], vs[0][k]), k
    _native_step(tb, b1)
    assert tb.sync_gradients
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(tb.projector_grads()[frozen])) == 0
    total = float(tb.grad_norm)
    print(f"[clip_vit] frozen {frozen}: grad_norm {total:.6e}, fp64 norm over the trainable gradients {want:.6e}, with the frozen "
          f"tensor's {with_frozen:.6e}")
    assert abs(total - want) <= 1e-3 * want
    after = float(torch.sqrt(sum((x.double() ** 2).sum() for x in tb.buckets)))
    assert abs(after - mx) <= 1e-3 * mx
    for k, p in b.named_parameters():
        assert torch.equal(p, start[k]) == (k == frozen), k


def test_checkpoint_resume_continues_bit_for_bit():
    P = util.pkg()
    b0, b1 = _case("tiny")[0], _batch("tiny", seed=9)
    a = _model("tiny")
    ta = P.Trainer(a, lr=1e-3, coeffs=W, projector=True)
    _native_step(ta, b0)
    model_sd = {k: v.detach().clone() for k, v in a.state_dict().items()}
    opt_sd = ta.state_dict()
    names = opt_sd["param_names"]
    assert tuple(names[-4:]) == P.training.PROJECTOR_KEYS and all(n.startswith("showo.") for n in names[:-4])
    assert names == [k for k, _ in a.named_parameters()]
    l2 = _native_step(ta, b1).clone()
    b = _model("tiny")
    b.load_state_dict(model_sd)
    tb = P.Trainer(b, lr=1e-3, coeffs=W, projector=True)
    tb.load_state_dict(opt_sd)
    assert tb.step_count == 1
    assert _same_bits(_native_step(tb, b1), l2)
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q), k
    # a file written without the projector does not resume a projector=True trainer (and keeps loading into a plain one)
    c = _model("tiny")
    plain = P.Trainer(c, lr=1e-3).state_dict()
    assert len(plain["param_names"]) == len(names) - 4
    with pytest.raises(ValueError):
        tb.load_state_dict(plain)
    P.Trainer(c, lr=1e-3).load_state_dict(plain)


def test_default_trainer_ignores_the_projector_as_before():
    """Trainer(m) on a w_clip_vit model with plain step(): the projector is untouched, and model.showo ends where the same step on a
    model without a projector ends"""
    P = util.pkg()
    d, sd = _state("tiny")
    g = GEOMETRIES["tiny"]
    m0, m1 = _model("tiny"), _model("tiny")
    d2 = Wt.ShowoDims(**Wt.TINY)
    m2 = util.build_showo(d2, {k: v for k, v in sd.items() if k.startswith("showo.")}, max_batch=g["max_batch"], max_seq=g["max_seq"]).train()
    bt = _case("tiny")[0]
    ids = bt["ids"].clone()
    ids[:, IMG_START:IMG_START + bt["P"]] = 5  # a plain id batch
    t1, t2 = P.Trainer(m1, lr=1e-3, coeffs=W), P.Trainer(m2, lr=1e-3, coeffs=W)
    assert t1.projector is False and t1.projector_grads() == {} and len(t1.buckets) == d.layers + 2
    s = bt["split"]
    la = t1.step(ids, bt["mask"], bt["labels"], s[0], s[1], s[2], bt["msl"])
    lb = t2.step(ids, bt["mask"], bt["labels"], s[0], s[1], s[2], bt["msl"])
    assert _same_bits(la, lb)
    p2 = dict(m2.named_parameters())
    for (k, p), (_, q) in zip(m1.named_parameters(), m0.named_parameters()):
        if k.startswith("mm_projector."):
            assert torch.equal(p, q), k
        else:
            assert not torch.equal(p, q) and torch.equal(p, p2[k]), k
    with pytest.raises(RuntimeError):
        t1.step_clip_vit(bt["ids"], bt["feats"], IMG_START, bt["mask"], bt["labels"], s[0], s[1], s[2], bt["msl"])
