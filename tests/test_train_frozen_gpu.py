"""Training with frozen parameters (reference: AdamW over the `requires_grad` parameters only, training/train.py:210-223; the
LLaVA-pretrain stage trains mm_projector alone, training/train_w_clip_vit.py:200-214): a frozen tensor gets no weight-gradient launch,
no hand-out, no exchange and no optimizer update, every trainable gradient keeps its bits, and the launch counters show the skipped
work.  Comparisons use ONE model and the same batch run twice (all trainable, then with requires_grad changed); Trainer comparisons
start two models from the same state dict."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import util
from util import O, Wt, dev

pytestmark = pytest.mark.gpu

W = (1.0, 0.1, 1.0)  # the reference's loss weights (training/train.py:600 with the stage-1 coefficients)
NO_DECAY = ["bias", "layer_norm.weight", "mlm_ln.weight", "embeddings.weight"]  # reference training/train.py:211
FULL = dict(hidden=2048, layers=24, heads=32, ffn=8192)  # Phi-1.5 (ShowoDims defaults)


def _loss(losses):
    return sum(w * l for w, l in zip(W, losses))


def _counters(m, reset=False):
    """{wgrad, dgrad, phases, embed, transposes, fused} of the model's trainer (showo_train_counters)"""
    out = (C.c_int64 * 6)()
    util.lib().call("showo_train_counters", m._trainer, C.cast(out, C.c_void_p), int(reset))
    return dict(zip(("wgrad", "dgrad", "phases", "embed", "transposes", "fused"), list(out)))


def _reset(m):
    if m._trainer is not None:
        _counters(m, reset=True)


def _want_wgrad(m):
    """weight-gradient GEMMs a backward launches for the model's requires_grad: Wqkv (any of q / k / v), Wd, W1, W2 per block, lm_head"""
    n = int(m.showo.lm_head.weight.requires_grad)
    for layer in m.showo.model.layers:
        a, f = layer.self_attn, layer.mlp
        n += int(a.q_proj.weight.requires_grad or a.k_proj.weight.requires_grad or a.v_proj.weight.requires_grad)
        n += int(a.dense.weight.requires_grad) + int(f.fc1.weight.requires_grad) + int(f.fc2.weight.requires_grad)
    return n


# ---------------------------------------------------------------- projector-only (LLaVA-pretrain) w_clip_vit flow

def _projector_case(dims, B, n_img, n_txt, split, max_batch, max_seq):
    d = Wt.ShowoDims(**dict(dims, w_clip_vit=True))
    sd = Wt.make_showo_state(d, seed=11)
    for k, v in Wt.make_projector_state(1024, d.hidden, seed=5).items():
        sd["mm_projector." + k] = v
    m = util.build_showo(d, sd, max_batch=max_batch, max_seq=max_seq).train()
    torch.manual_seed(4)
    feats = torch.randn(B, n_img, 1024).cuda()
    ids = torch.randint(0, d.llm_vocab, (B, n_txt)).cuda()
    Lq = n_img + n_txt
    labels = torch.cat([torch.full((B, n_img + 2), -100), torch.randint(0, d.llm_vocab, (B, n_txt - 2))], dim=1).cuda()
    mask = O.mask_mmu_vit(B, Lq, system_prompt_len=0).cuda()

    def run():
        m.zero_grad(set_to_none=True)
        txt = m.showo.model.embed_tokens(ids)
        e = torch.cat([txt[:, :2], m.mm_projector(feats), txt[:, 2:]], dim=1)
        e.retain_grad()
        _reset(m)
        losses = m(None, input_embeddings=e, attention_mask=mask, labels=labels, batch_size_t2i=split[0], batch_size_lm=split[1],
                   batch_size_mmu=split[2], max_seq_length=d.max_text_len)[1:]
        _loss(losses).backward()
        torch.cuda.synchronize()
        return e.grad.clone(), {n: p.grad.clone() for n, p in m.mm_projector.named_parameters()}

    g_all, p_all = run()
    m.showo.requires_grad_(False)  # training/train_w_clip_vit.py:200-214, und_type "llava_pretrain"
    g_fr, p_fr = run()
    cnt = _counters(m)
    assert torch.equal(g_fr, g_all)
    for n in p_all:
        assert torch.equal(p_fr[n], p_all[n]), n
    for n, p in m.showo.named_parameters():
        assert p.grad is None, n
    assert cnt["wgrad"] == 0 and cnt["embed"] == 0 and cnt["phases"] == d.layers, cnt
    # zero contract: every frozen slot of the flat gradient buffer reads as zeros
    for b in range(util.lib().load().showo_train_num_buckets(m._trainer)):
        ptr, n = C.c_void_p(), C.c_int64()
        util.lib().call("showo_train_bucket", m._trainer, b, C.byref(ptr), C.byref(n))
        assert int(torch.count_nonzero(util.pkg().training.device_view(ptr.value, n.value, "cuda"))) == 0, b


def test_projector_only_tiny():
    _projector_case(Wt.TINY, B=3, n_img=16, n_txt=11, split=(0, 1, 2), max_batch=8, max_seq=128)


def test_projector_only_small_production_kernels():
    # T = 12 x 40 = 480 >= 256: the trainer's production branch (fused save-form projection, gemm2p / gemm3w)
    _projector_case(Wt.SMALL, B=12, n_img=24, n_txt=16, split=(2, 2, 8), max_batch=12, max_seq=40)


def test_projector_only_full_size_llava_pretrain_geometry():
    # Phi-1.5, split (2, 2, 10), 576 projector rows + 195 text positions = 771 (max_seq_length 512 + the 576 image
    # rows in place of the 256 VQ tokens + the mmu prompt's special tokens)
    _projector_case(FULL, B=14, n_img=576, n_txt=195, split=(2, 2, 10), max_batch=14, max_seq=771)


# ---------------------------------------------------------------- partial freezing, ids flow

def _freeze(m, name, nL):
    """apply a named frozen set to model m (requires_grad False); returns the expected number of block phases"""
    ph = m.showo
    if name == "lower":  # the embedding plus blocks 0 .. k-1
        k = nL // 2
        ph.model.embed_tokens.requires_grad_(False)
        for i in range(k):
            ph.model.layers[i].requires_grad_(False)
        return nL - k
    if name == "coupling":  # block 1 frozen while block 0 trains: block 0's dense / fc2 bias gradients come from block 1's LN backward
        ph.model.layers[1].requires_grad_(False)
        ph.model.embed_tokens.requires_grad_(False)
        return nL
    if name == "head":  # final LayerNorm + lm_head frozen, the top block trains
        ph.model.final_layernorm.requires_grad_(False)
        ph.lm_head.requires_grad_(False)
        return nL
    if name == "singles":  # single tensors inside training blocks
        l0, l1 = ph.model.layers[0], ph.model.layers[nL - 1]
        for p in (l0.mlp.fc2.bias, l1.self_attn.dense.bias, l0.self_attn.q_layernorm.weight, l0.self_attn.k_layernorm.bias,
                  l1.self_attn.k_proj.weight, l0.self_attn.v_proj.bias, l0.input_layernorm.bias, l1.mlp.fc1.weight,
                  ph.model.final_layernorm.weight):
            p.requires_grad_(False)
        return nL
    if name == "probe":  # linear probe: lm_head only
        ph.requires_grad_(False)
        ph.lm_head.requires_grad_(True)
        return 0
    raise ValueError(name)


def _ids_batch(geom):
    if geom == "tiny":
        d = Wt.ShowoDims(**Wt.TINY)
        sd = Wt.make_showo_state(d, seed=11)
        g = util.golden("showo_tiny_forward.npz")
        return d, sd, (dev(g["train_ids"]), dev(g["train_mask"]), dev(g["train_labels"])), (2, 1, 2), dict(max_batch=8, max_seq=128)
    if geom == "small":
        d = Wt.ShowoDims(**Wt.SMALL)
        sd = Wt.make_showo_state(d, seed=13)
        g = util.golden("showo_small_train.npz")
        return d, sd, (dev(g["ids"]), dev(g["mask"]), dev(g["labels"])), tuple(int(x) for x in g["b"]), dict(max_batch=12, max_seq=32)
    d = Wt.ShowoDims(**FULL)
    sd = Wt.make_showo_state(d, seed=0)
    torch.manual_seed(7)
    B, L = 4, 96
    ids = torch.randint(0, d.vocab, (B, L)).cuda()
    labels = ids.clone()
    labels[:, :8] = -100
    return d, sd, (ids, None, labels), (1, 1, 2), dict(max_batch=4, max_seq=96)


def _partial_case(geom, names, m=None, batch=None):
    d, sd, (ids, mask, labels), split, ws = batch if batch is not None else _ids_batch(geom)
    m = m if m is not None else util.build_showo(d, sd, **ws).train()
    kw = dict(attention_mask=mask, labels=labels, batch_size_t2i=split[0], batch_size_lm=split[1], batch_size_mmu=split[2],
              max_seq_length=d.max_text_len)

    def run():
        m.zero_grad(set_to_none=True)
        _reset(m)
        _loss(m(ids, **kw)[1:]).backward()
        torch.cuda.synchronize()
        return {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}

    m.requires_grad_(True)
    full = run()
    c_full = _counters(m)
    assert c_full["wgrad"] == 4 * d.layers + 1 and c_full["phases"] == d.layers and c_full["embed"] == 2, c_full
    for name in names:
        m.requires_grad_(True)
        phases = _freeze(m, name, d.layers)
        got = run()
        cnt = _counters(m)
        for n, p in m.named_parameters():
            if p.requires_grad:
                assert got[n] is not None and torch.equal(got[n], full[n]), (name, n)
            else:
                assert got[n] is None, (name, n)
        assert cnt["phases"] == phases, (name, cnt)
        assert cnt["wgrad"] == _want_wgrad(m), (name, cnt)
        assert cnt["embed"] == (2 if m.showo.model.embed_tokens.weight.requires_grad else 0), (name, cnt)
        if name == "probe":
            assert cnt["dgrad"] == 0, cnt  # no lm_head dgrad, no final-LayerNorm backward
    m.requires_grad_(True)
    return m


SETS = ["lower", "coupling", "head", "singles", "probe"]


@pytest.mark.parametrize("geom", ["tiny", "small"])
def test_partial_freezing_gradients_bit_identical(geom):
    _partial_case(geom, SETS)


def test_partial_freezing_full_size():
    _partial_case("full", ["lower", "coupling", "probe"])


def test_partial_freezing_transpose_branch_in_a_child_process():
    """SHOWO_TRAIN_TN=0 (read once per process): the transpose + NT-GEMM weight-gradient branch skips the same launches"""
    env = dict(os.environ, SHOWO_TRAIN_TN="0")
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); import test_train_frozen_gpu as t; t._partial_case('tiny', t.SETS); print('CHILD_OK')"
            % here)
    r = subprocess.run([sys.executable, "-s", "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------- Trainer

def _trainer_batch(geom):
    d, sd, (ids, mask, labels), split, ws = _ids_batch(geom)
    return d, sd, ids, mask, labels, split, ws


def _freeze_lower(m):
    """the embedding, block 0 and one bias of block 1 frozen (a partly frozen bucket)"""
    m.showo.model.embed_tokens.requires_grad_(False)
    m.showo.model.layers[0].requires_grad_(False)
    m.showo.model.layers[1].mlp.fc1.bias.requires_grad_(False)


@pytest.mark.parametrize("geom", ["tiny", "small"])
def test_trainer_frozen_masters_unchanged_and_trainable_match(geom):
    P = util.pkg()
    d, sd, ids, mask, labels, split, ws = _trainer_batch(geom)
    a = util.build_showo(d, sd, **ws).train()
    b = util.build_showo(d, sd, **ws).train()
    _freeze_lower(b)
    ta = P.Trainer(a, lr=1e-3)
    tb = P.Trainer(b, lr=1e-3)
    init = {n: p.detach().clone() for n, p in b.named_parameters()}
    ta.step(ids, mask, labels, *split, d.max_text_len)
    tb.step(ids, mask, labels, *split, d.max_text_len)
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        if q.requires_grad:  # the same gradients in: the same AdamW update, bit for bit
            assert torch.equal(p, q), n
        else:
            assert torch.equal(q, init[n]), n
    # images: only what the step changed is rebuilt by the next forward (4 transposed images per trainable block + lm_head)
    _reset(b)
    tb.step(ids, mask, labels, *split, d.max_text_len)
    cnt = _counters(b)
    assert cnt["transposes"] == 4 * (d.layers - 1) + 1, cnt
    assert cnt["phases"] == d.layers - 1 and cnt["embed"] == 0 and cnt["wgrad"] == 4 * (d.layers - 1) + 1, cnt
    if ids.numel() >= 256:  # the inference forward's fused block images: after a step only the trainable blocks are rebuilt
        with torch.no_grad():
            b(ids, attention_mask=mask)
        tb.step(ids, mask, labels, *split, d.max_text_len)
        _reset(b)
        with torch.no_grad():
            b(ids, attention_mask=mask)
        torch.cuda.synchronize()
        assert _counters(b)["fused"] == d.layers - 1, _counters(b)
    for _ in range(2):
        tb.step(ids, mask, labels, *split, d.max_text_len)
    for n, q in b.named_parameters():
        if not q.requires_grad:
            assert torch.equal(q, init[n]), n
    # the optimizer state keeps its format; frozen entries carry their untouched (zero) moments
    st = tb.state_dict()
    assert len(st["state"]) == len(list(b.named_parameters()))
    for i, (n, q) in enumerate(b.named_parameters()):
        if not q.requires_grad:
            assert int(torch.count_nonzero(st["state"][i]["exp_avg"])) == 0, n


def test_trainer_frozen_tracks_autograd_plus_torch_adamw():
    """Trainer.step with a frozen set == autograd + torch.optim.AdamW built over the trainable parameters with the reference's two
    groups (training/train.py:210-223), within the tolerance of test_trainer_step_matches_autograd_plus_torch_adamw"""
    P = util.pkg()
    d, sd, ids, mask, labels, split, ws = _trainer_batch("tiny")
    ref = util.build_showo(d, sd, **ws).train()
    m = util.build_showo(d, sd, **ws).train()
    _freeze_lower(ref)
    _freeze_lower(m)
    named = [(n, p) for n, p in ref.named_parameters() if p.requires_grad]
    opt = torch.optim.AdamW([{"params": [p for n, p in named if not any(x in n for x in NO_DECAY)], "weight_decay": 0.01},
                             {"params": [p for n, p in named if any(x in n for x in NO_DECAY)], "weight_decay": 0.0}],
                            lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    tr = P.Trainer(m, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, coeffs=W)
    kw = dict(attention_mask=mask, labels=labels, batch_size_t2i=split[0], batch_size_lm=split[1], batch_size_mmu=split[2],
              max_seq_length=d.max_text_len)
    for step in range(3):
        before = {n: p.detach().clone() for n, p in ref.named_parameters()}
        opt.zero_grad()
        _loss(ref(ids, **kw)[1:]).backward()
        opt.step()
        tr.step(ids, mask, labels, *split, d.max_text_len)
        for (n, p), (_, q) in zip(ref.named_parameters(), m.named_parameters()):
            if not p.requires_grad:
                assert torch.equal(p, q) and torch.equal(q, before[n]), (step, n)
            elif step == 0:
                assert (p - q).abs().max() <= 1e-6 + 1e-5 * float(p.abs().max()), (step, n)
            elif "k_layernorm.bias" not in n:
                # (k_layernorm.bias shifts every key of a head alike: its gradient is ~0 by construction and Adam turns it into
                # rounding noise once the weights differ by rounding, as in test_trainer_exchange_over_rccl_single_rank)
                upd = (p - before[n]).double()
                assert float((p - q).double().norm()) <= 3e-2 * float(upd.norm()) + 1e-9, (step, n)


def test_trainer_frozen_gradient_clipping_matches_torch():
    """max_grad_norm: the flat buffer's norm is the norm over the trainable tensors (frozen slots read as zeros)"""
    P = util.pkg()
    d, sd, ids, mask, labels, split, ws = _trainer_batch("tiny")
    ref = util.build_showo(d, sd, **ws).train()
    _freeze_lower(ref)
    kw = dict(attention_mask=mask, labels=labels, batch_size_t2i=split[0], batch_size_lm=split[1], batch_size_mmu=split[2],
              max_seq_length=d.max_text_len)
    _loss(ref(ids, **kw)[1:]).backward()
    trainable = [p for p in ref.parameters() if p.requires_grad]
    want = {n: p.grad.clone() for n, p in ref.named_parameters() if p.requires_grad}
    total = float(torch.nn.utils.clip_grad_norm_(trainable, 0.05))
    assert total > 0.05
    m = util.build_showo(d, sd, **ws).train()
    _freeze_lower(m)
    tr = P.Trainer(m, lr=1e-3, max_grad_norm=0.05)
    tr.step(ids, mask, labels, *split, d.max_text_len)
    gn = float(torch.sqrt(sum((b.double() ** 2).sum() for b in tr.buckets)))
    assert abs(gn - 0.05) < 1e-3 * 0.05
    coef = 0.05 / (total + 1e-6)
    for n, p in m.named_parameters():
        ptr, k = C.c_void_p(), C.c_int64()
        util.lib().call("showo_train_grad", m._trainer, n.encode(), C.byref(ptr), C.byref(k))
        g = util.pkg().training.device_view(ptr.value, k.value, "cuda")
        if n in want:  # the clipped gradient = torch's gradient x torch's coefficient (to the trainer's bf16-GEMM accuracy)
            assert float((g - want[n].reshape(-1) * coef).norm()) <= 2e-2 * float((want[n] * coef).norm()) + 1e-9, n
        else:
            assert int(torch.count_nonzero(g)) == 0, n


def _one_rank_group():
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


def test_trainer_wholly_frozen_buckets_are_not_exchanged():
    _one_rank_group()
    P = util.pkg()
    d, sd, ids, mask, labels, split, ws = _trainer_batch("tiny")
    a = util.build_showo(d, sd, **ws).train()
    b = util.build_showo(d, sd, **ws).train()
    _freeze_lower(a)
    _freeze_lower(b)
    ta = P.Trainer(a, lr=1e-3, wire="fp32")
    tb = P.Trainer(b, lr=1e-3, wire="fp32", force_exchange=True)
    launched = []
    real = tb.exchange.launch
    tb.exchange.launch = lambda k: (launched.append(k), real(k))
    for _ in range(2):
        ta.step(ids, mask, labels, *split, d.max_text_len)
        tb.step(ids, mask, labels, *split, d.max_text_len)
    nL = d.layers
    # head, then blocks 1 .. nL-1 (block 1's bucket is partly frozen: it goes on the wire with its zeros); never block 0 or the embedding
    assert launched == 2 * ([nL + 1] + list(range(nL, 1, -1))), launched
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q), n


def test_trainer_refuses_a_changed_or_empty_trainable_set():
    P = util.pkg()
    d, sd, ids, mask, labels, split, ws = _trainer_batch("tiny")
    m = util.build_showo(d, sd, **ws).train()
    tr = P.Trainer(m, lr=1e-3)
    tr.step(ids, mask, labels, *split, d.max_text_len)
    m.showo.lm_head.bias.requires_grad_(False)
    with pytest.raises(RuntimeError, match="requires_grad"):
        tr.step(ids, mask, labels, *split, d.max_text_len)
    m.showo.requires_grad_(False)
    with pytest.raises(ValueError, match="nothing to train"):
        P.Trainer(m, lr=1e-3)
