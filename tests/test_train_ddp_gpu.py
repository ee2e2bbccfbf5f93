"""The labelled Showo.forward as a chain of autograd nodes, one per gradient bucket (embedding -> blocks -> head): every bucket's
gradients reach autograd -- and DDP's bucket hooks (accelerator.prepare, reference training/train.py:449) -- as soon as its backward
phase is queued, with no host synchronisation, bit-identical to the one-call C backward, never aliasing trainer memory, and refusing
to differentiate a forward whose activations a later forward replaced."""
import os

import pytest
import torch

import util
from util import O, Wt, dev

pytestmark = pytest.mark.gpu

W = (1.0, 0.1, 1.0)  # the reference's loss weights (training/train.py:600 with the stage-1 coefficients)
NO_DECAY = ["bias", "layer_norm.weight", "mlm_ln.weight", "embeddings.weight"]  # reference training/train.py:211


def _golden_batch():
    g = util.golden("showo_tiny_forward.npz")
    ids, mask, labels = dev(g["train_ids"]), dev(g["train_mask"]), dev(g["train_labels"])
    return ids, mask, labels


def _kw(d, mask, labels):
    return dict(attention_mask=mask, labels=labels, batch_size_t2i=2, batch_size_lm=1, batch_size_mmu=2, max_seq_length=d.max_text_len)


def _loss(losses, w=W):
    """w_t2i * loss_t2i + w_lm * loss_lm + w_mmu * loss_mmu; a weight of None leaves that loss out of the graph"""
    return sum(wi * li for wi, li in zip(w, losses) if wi is not None)


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


class _CallLog:
    """logs every C entry point called through showo_amd._lib.call (with the layer of showo_train_backward_layer) and, through
    post-accumulate-grad hooks, every parameter whose .grad autograd has just written -- in one list, in order"""

    def __init__(self, monkeypatch, model):
        self.log = []
        L = util.lib()
        real = L.call

        def call(name, *args):
            self.log.append(("call", name, args[1] if name == "showo_train_backward_layer" else None))
            return real(name, *args)

        monkeypatch.setattr(L, "call", call)
        for n, p in model.named_parameters():
            p.register_post_accumulate_grad_hook(lambda p, n=n: self.log.append(("grad", n, None)))

    def index(self, kind, name, arg=None):
        for k, e in enumerate(self.log):
            if e == (kind, name, arg):
                return k
        raise AssertionError(f"{kind} {name} {arg} never logged; log: {[e[1:] for e in self.log if e[0] == 'call'][-8:]}")

    def grads(self, pred):
        return [k for k, e in enumerate(self.log) if e[0] == "grad" and pred(e[1])]


def _assert_interleaved(cl, nL):
    """every gradient of the head is accumulated before block nL-1's backward is queued, every gradient of block nL-1 before block
    0's backward is queued, and the embedding's after showo_train_backward_embed"""
    top = f"showo.model.layers.{nL - 1}."
    head = cl.grads(lambda n: n.startswith("showo.lm_head.") or n.startswith("showo.model.final_layernorm."))
    block = cl.grads(lambda n: n.startswith(top))
    emb = cl.grads(lambda n: n == "showo.model.embed_tokens.weight")
    assert len(head) == 4 and len(block) == 18 and len(emb) == 1, (len(head), len(block), len(emb))
    first_top, first_0 = cl.index("call", "showo_train_backward_layer", nL - 1), cl.index("call", "showo_train_backward_layer", 0)
    assert max(head) < first_top, (max(head), first_top)
    assert max(block) < first_0, (max(block), first_0)
    assert min(emb) > cl.index("call", "showo_train_backward_embed")


def test_bucket_gradients_are_accumulated_between_the_backward_phases(monkeypatch):
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd).train()
    ids, mask, labels = _golden_batch()
    losses = m(ids, **_kw(d, mask, labels))[1:]
    cl = _CallLog(monkeypatch, m)
    _loss(losses).backward()
    _assert_interleaved(cl, d.layers)


def _adamw(model):
    named = list(model.named_parameters())
    return torch.optim.AdamW([{"params": [p for n, p in named if not any(x in n for x in NO_DECAY)], "weight_decay": 0.01},
                              {"params": [p for n, p in named if any(x in n for x in NO_DECAY)], "weight_decay": 0.0}],
                             lr=1e-3, betas=(0.9, 0.999), eps=1e-8)


def test_ddp_comm_hook_runs_before_the_last_block_backward_and_adamw_matches(monkeypatch):
    """DistributedDataParallel in a one-rank RCCL group: after DDP's first iteration (one bucket, rebuilt from the observed gradient
    order) the first bucket's comm hook is called before showo_train_backward_layer(0) is queued; AdamW with the reference's two
    parameter groups gives parameters bit-identical to the same steps without DDP"""
    from torch.distributed.algorithms.ddp_comm_hooks import default_hooks
    from torch.nn.parallel import DistributedDataParallel
    _one_rank_group()
    d, sd = util.tiny_state()
    ids, mask, labels = _golden_batch()
    a = util.build_showo(d, sd).train()
    b = util.build_showo(d, sd).train()
    ddp = DistributedDataParallel(a, device_ids=[0], bucket_cap_mb=0.05)
    cl = _CallLog(monkeypatch, a)
    hooks = []

    def hook(state, bucket):
        cl.log.append(("hook", bucket.index(), None))
        hooks.append(len(cl.log) - 1)
        return default_hooks.allreduce_hook(state, bucket)

    ddp.register_comm_hook(None, hook)
    oa, ob = _adamw(a), _adamw(b)
    for step in range(3):
        del cl.log[:]
        hooks.clear()
        la = ddp(ids, **_kw(d, mask, labels))[1:]
        oa.zero_grad()
        _loss(la).backward()
        oa.step()
        lb = b(ids, **_kw(d, mask, labels))[1:]
        ob.zero_grad()
        _loss(lb).backward()
        ob.step()
        for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            assert torch.equal(p, q), (step, n)
        if step >= 1:  # DDP buckets by observed gradient order from its second iteration on
            assert len(hooks) > 1, hooks
            assert hooks[0] < cl.index("call", "showo_train_backward_layer", 0), (hooks, cl.log)


def test_backward_does_not_synchronise_with_the_host():
    """no host synchronisation inside loss.backward(): the three loss weights reach the head's cross-entropy pass in device memory
    (showo_train_backward_head_dev) instead of through float(g)"""
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd).train()
    ids, mask, labels = _golden_batch()
    loss = _loss(m(ids, **_kw(d, mask, labels))[1:])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            loss.detach().item()  # the detector is live in this build: a device -> host read raises
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(p.grad is not None for p in m.parameters())


def _c_api_reference(model, ids, emb, mask, labels, split, msl, w):
    """showo_train_forward[_embeds] + showo_train_backward (host loss weights) + showo_train_grad_copy: {name: grad}, d/d(emb)"""
    L = util.lib()
    tr = model.trainer()
    lab = labels.to(torch.int64).contiguous()
    B, Lq = lab.shape
    maskf = mask.float().contiguous()
    losses = torch.empty(3, device="cuda")
    if emb is None:
        L.call("showo_train_forward", tr, L.ptr(ids), L.ptr(maskf), L.ptr(lab), B, Lq, *split, msl, None, L.ptr(losses), L.stream())
    else:
        e = emb.detach().float().contiguous()
        L.call("showo_train_forward_embeds", tr, L.ptr(e), L.ptr(maskf), L.ptr(lab), B, Lq, *split, msl, None, L.ptr(losses), L.stream())
    L.call("showo_train_backward", tr, L.ptr(lab), *split, msl, *[0.0 if x is None else x for x in w], L.stream())
    grads = {}
    for n, p in model.showo.named_parameters():
        t = torch.empty_like(p)
        L.call("showo_train_grad_copy", tr, ("showo." + n).encode(), L.ptr(t), t.numel(), L.stream())
        grads["showo." + n] = t
    g_emb = None
    if emb is not None:
        g_emb = torch.empty(tuple(emb.shape), device="cuda")
        L.call("showo_train_input_grad", tr, L.ptr(g_emb), g_emb.numel(), L.stream())
    torch.cuda.synchronize()
    return grads, g_emb


@pytest.mark.parametrize("w", [W, (0.5, None, 1.0), (1.0, 0.0, 0.25)], ids=["w1", "lm-unused", "lm-zero"])
def test_gradients_bit_identical_to_the_one_call_c_backward_ids(w):
    d, sd = util.tiny_state()
    a = util.build_showo(d, sd).train()
    b = util.build_showo(d, sd).train()
    ids, mask, labels = _golden_batch()
    _loss(a(ids, **_kw(d, mask, labels))[1:], w).backward()
    want, _ = _c_api_reference(b, ids, None, mask, labels, (2, 1, 2), d.max_text_len, w)
    for n, p in a.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, want[n]), n


def test_gradients_bit_identical_to_the_one_call_c_backward_projector_flow():
    """the w_clip_vit flow (training/train_w_clip_vit.py:530-613): mm_projector rows spliced between embedded text ids ->
    Showo.forward(input_embeddings=..., labels=...).  Every Show-o gradient, d(loss)/d(input_embeddings), and the projector and
    embedding-table gradients behind it equal the C-API backward pushed through the same torch graph, bit for bit"""
    d = Wt.ShowoDims(**dict(Wt.TINY, w_clip_vit=True))
    sd = Wt.make_showo_state(d, seed=11)
    for k, v in Wt.make_projector_state(1024, d.hidden, seed=5).items():
        sd["mm_projector." + k] = v
    a = util.build_showo(d, sd).train()
    b = util.build_showo(d, sd).train()
    torch.manual_seed(4)
    B, n_img, n_txt = 3, 16, 11
    feats = torch.randn(B, n_img, 1024).cuda()
    ids = torch.randint(0, d.llm_vocab, (B, n_txt)).cuda()
    Lq = n_img + n_txt
    labels = torch.cat([torch.full((B, n_img + 2), -100), torch.randint(0, d.llm_vocab, (B, n_txt - 2))], dim=1).cuda()
    mask = O.mask_mmu_vit(B, Lq, system_prompt_len=0).cuda()
    split = (0, 1, 2)

    def embeds(m):
        txt = m.showo.model.embed_tokens(ids)
        return torch.cat([txt[:, :2], m.mm_projector(feats), txt[:, 2:]], dim=1)

    ea = embeds(a)
    ea.retain_grad()
    losses = a(None, input_embeddings=ea, attention_mask=mask, labels=labels, batch_size_t2i=split[0], batch_size_lm=split[1],
               batch_size_mmu=split[2], max_seq_length=d.max_text_len)[1:]
    _loss(losses).backward()
    eb = embeds(b)
    want, g_emb = _c_api_reference(b, None, eb, mask, labels, split, d.max_text_len, W)
    assert torch.equal(ea.grad, g_emb)
    for n, p in b.showo.named_parameters():  # what the old single node handed autograd, then the caller's graph behind the embeddings
        p.grad = want["showo." + n]
    eb.backward(g_emb)
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), n


def _second_batch(labels):
    """a different loss on the same rows: every other valid label ignored"""
    l2 = labels.clone()
    idx = (l2 != -100).nonzero()
    l2[idx[::2, 0], idx[::2, 1]] = -100
    return l2


def test_accumulation_without_zero_grad_sums_and_never_aliases_trainer_memory():
    """two backward passes without zero_grad (the first under ddp.no_sync(), as accelerator.accumulate does) leave .grad = g(batch 1)
    + g(batch 2) bit for bit: no handed-out gradient is trainer memory that the second backward overwrites"""
    from torch.nn.parallel import DistributedDataParallel
    _one_rank_group()
    d, sd = util.tiny_state()
    ids, mask, labels = _golden_batch()
    lab2 = _second_batch(labels)
    m = util.build_showo(d, sd).train()
    single = []
    for lab in (labels, lab2):
        m.zero_grad()
        _loss(m(ids, **_kw(d, mask, lab))[1:]).backward()
        single.append({n: p.grad.clone() for n, p in m.named_parameters()})
    m.zero_grad()
    _loss(m(ids, **_kw(d, mask, labels))[1:]).backward()
    _loss(m(ids, **_kw(d, mask, lab2))[1:]).backward()
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, single[0][n] + single[1][n]), n
    a = util.build_showo(d, sd).train()
    ddp = DistributedDataParallel(a, device_ids=[0])
    with ddp.no_sync():
        _loss(ddp(ids, **_kw(d, mask, labels))[1:]).backward()
    _loss(ddp(ids, **_kw(d, mask, lab2))[1:]).backward()
    for n, p in a.named_parameters():
        assert torch.equal(p.grad, single[0][n] + single[1][n]), n


def test_backward_of_a_replaced_forward_raises():
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd).train()
    ids, mask, labels = _golden_batch()
    la = _loss(m(ids, **_kw(d, mask, labels))[1:])
    lb = _loss(m(ids, **_kw(d, mask, _second_batch(labels)))[1:])
    with pytest.raises(RuntimeError, match="another training forward"):
        la.backward()
    assert all(p.grad is None for p in m.parameters())
    lb.backward()  # the current forward still differentiates, and gives what a fresh model gives
    ref = util.build_showo(d, sd).train()
    _loss(ref(ids, **_kw(d, mask, _second_batch(labels)))[1:]).backward()
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    # Trainer.step's forward replaces the activations as well
    lc = _loss(m(ids, **_kw(d, mask, labels))[1:])
    util.pkg().Trainer(m, lr=0.0).step(ids, mask, labels, 2, 1, 2, d.max_text_len)
    with pytest.raises(RuntimeError, match="another training forward"):
        lc.backward()


def test_full_size_24_layer_bucket_gradients_interleave_with_the_backward(monkeypatch):
    """the ordering of the first test on the full 24-block model (1.45 B parameters) at one small batch"""
    from showo_amd import synthetic
    d = Wt.ShowoDims()
    torch.manual_seed(0)
    m = synthetic.random_init_showo(max_batch=2, max_seq=128).train()
    assert m.arch["num_hidden_layers"] == d.layers and m.vocab_size == d.vocab
    gen = torch.Generator(device="cuda").manual_seed(0)
    B, Lq = 2, 128
    ids = torch.randint(0, d.llm_vocab, (B, Lq), device="cuda", generator=gen)
    losses = m(ids, labels=ids, batch_size_t2i=0, batch_size_lm=1, batch_size_mmu=1, max_seq_length=d.max_text_len)[1:]
    cl = _CallLog(monkeypatch, m)
    _loss(losses).backward()
    torch.cuda.synchronize()
    _assert_interleaved(cl, d.layers)
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
