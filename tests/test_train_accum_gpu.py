"""Gradient accumulation over micro-batches on the native training path (reference: `accelerator.accumulate(model)` with
`training.gradient_accumulation_steps` = k, training/train.py:92, 589-631): the accumulating kernel forms add each micro-batch's
gradient into the flat buffer, `Trainer.step` runs the exchange, clipping, AdamW and the image refresh once per window of k calls.

The elementwise gate of the "accumulate is the sum" tests, r = the window's buffer, v_j = micro-batch j alone in overwriting mode:
    |r - sum_j v_j| <= (k - 1) * 2^-23 * sum_j |v_j|        (sum_j v_j in fp64)
Every accumulating form adds ONE fp32 rounding per micro-batch after the first, each at most 2^-24 of a magnitude that is at most
sum_j |v_j|; the gate is that bound doubled."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import util
from util import O, Wt, dev

pytestmark = pytest.mark.gpu

W = (1.0, 0.1, 1.0)  # the reference's loss weights (training/train.py:600 with the stage-1 coefficients)
NO_DECAY = ["bias", "layer_norm.weight", "mlm_ln.weight", "embeddings.weight"]  # reference training/train.py:211
SPLIT = (2, 1, 2)  # the tiny golden batch: 2 t2i + 1 lm + 2 mmu sequences
EMBED = "showo.model.embed_tokens.weight"


def L():
    return util.lib()


# ---------------------------------------------------------------- micro-batches

def _redraw(d, ids, labels, seed):
    """a micro-batch with the golden batch's layout (so its attention mask stays valid) and a seeded re-draw of the image tokens of
    the t2i and mmu rows and of the masked positions of the t2i rows (oracle/make_golden.py builds the golden batch the same way)"""
    rs = np.random.RandomState(seed)
    N = d.num_vq_tokens
    ids, labels = ids.clone(), labels.clone()
    img = torch.from_numpy(rs.randint(0, d.codebook, size=(2, N)) + d.image_offset)
    masked = torch.from_numpy(rs.rand(2, N) < 0.6)
    ids[:2, -(N + 1):-1] = torch.where(masked, torch.full_like(img, d.mask_token_id), img)
    labels[:2, -(N + 1):-1] = torch.where(masked, img, torch.full_like(img, -100))
    ids[3:, 2:2 + N] = torch.from_numpy(rs.randint(0, d.codebook, size=(2, N)) + d.image_offset)
    return ids, labels


def _tiny_micro_batches(k=3):
    g = util.golden("showo_tiny_forward.npz")
    d, sd = util.tiny_state()
    ids0, lab0 = torch.from_numpy(g["train_ids"]).long(), torch.from_numpy(g["train_labels"]).long()
    mask = dev(g["train_mask"])
    host = [(ids0, lab0)] + [_redraw(d, ids0, lab0, 100 + j) for j in range(1, k)]
    for j in range(1, k):
        assert not torch.equal(host[j][0], host[0][0]) and not torch.equal(host[j][1], host[0][1])
    batches = [(dev(i), mask, dev(l)) for i, l in host]
    return d, sd, batches, host


def _rows_touched(host_ids, V):
    """[k, V] bool: embedding rows each micro-batch reads"""
    t = torch.zeros(len(host_ids), V, dtype=torch.bool)
    for j, ids in enumerate(host_ids):
        t[j, ids.reshape(-1)] = True
    return t


# ---------------------------------------------------------------- C ABI drivers

def _names(m):
    return [n for n, _ in m.named_parameters()]


def _grad_view(m, name):
    ptr, n = C.c_void_p(), C.c_int64()
    L().call("showo_train_grad", m._trainer, name.encode(), C.byref(ptr), C.byref(n))
    return util.pkg().training.device_view(ptr.value, n.value, "cuda")


def _snapshot(m):
    torch.cuda.synchronize()
    return {n: _grad_view(m, n).clone() for n in _names(m)}


def _micro(m, batch, split, msl, w, accumulate):
    """forward + full backward of one micro-batch through the C ABI with loss weights w; returns its three losses"""
    P = util.pkg()
    ids, mask, labels = batch
    tr = m.trainer()
    P.modeling_showo.sync_trainable(m, tr, {n: bool(p.requires_grad) for n, p in m.named_parameters()}, False)
    dm = P.training.train_mask(tr, mask)
    B, Lq = ids.shape
    losses = torch.empty(3, dtype=torch.float32, device="cuda")
    s = L().stream()
    L().call("showo_train_set_accumulate", tr, int(accumulate))
    try:
        try:
            L().call("showo_train_forward", tr, L().ptr(ids), L().ptr(dm), L().ptr(labels), B, Lq, split[0], split[1], split[2], msl,
                     None, L().ptr(losses), s)
        finally:
            L().call("showo_trainer_use_intervals", tr, None, None)
        L().call("showo_train_backward", tr, L().ptr(labels), split[0], split[1], split[2], msl, w[0], w[1], w[2], s)
    finally:
        L().call("showo_train_set_accumulate", tr, 0)
    return losses


def _alone_and_window(m, batches, split, msl):
    """v_j = every micro-batch alone in overwriting mode, r = the window (first overwriting, the rest accumulating), loss weights W / k"""
    k = len(batches)
    w = tuple(c / k for c in W)
    vs = []
    for b in batches:
        _micro(m, b, split, msl, w, 0)
        vs.append(_snapshot(m))
    for j, b in enumerate(batches):
        _micro(m, b, split, msl, w, j > 0)
    return vs, _snapshot(m)


def _gate_sum(r, vs, names, tag):
    k = len(vs)
    for n in names:
        s = sum(v[n].double() for v in vs)
        a = sum(v[n].double().abs() for v in vs)
        err = (r[n].double() - s).abs()
        bound = (k - 1) * 2.0 ** -23 * a
        ratio = float((err / bound.clamp(min=1e-300)).max()) if float(a.max()) > 0 else 0.0
        print(f"[accum] {tag} {n}: max |r - sum v_j| / ((k-1) 2^-23 sum|v_j|) = {ratio:.3f} (scale {float(a.max()):.3e})")
        assert bool((err <= bound).all()), (tag, n, ratio)


def _counters(m, reset=False):
    out = (C.c_int64 * 6)()
    L().call("showo_train_counters", m._trainer, C.cast(out, C.c_void_p), int(reset))
    return dict(zip(("wgrad", "dgrad", "phases", "embed", "transposes", "fused"), list(out)))


def _gemm_counters(reset=False):
    out = (C.c_int64 * 3)()
    L().call("showo_gemm_counters", C.cast(out, C.c_void_p), 1 if reset else 0)
    return [int(v) for v in out]


# ---------------------------------------------------------------- 1. accumulate is the sum (tiny, k = 3)

def test_window_is_the_sum_of_its_micro_batches_tiny():
    d, sd, batches, host = _tiny_micro_batches(3)
    touched = _rows_touched([h[0] for h in host], d.vocab)
    once = touched.sum(0) == 1
    assert int(once.sum()) > 0, "some embedding rows must be touched by exactly one micro-batch"
    m = util.build_showo(d, sd).train()
    vs, r = _alone_and_window(m, batches, SPLIT, d.max_text_len)
    for j in range(3):  # the micro-batches really differ
        assert not torch.equal(vs[j][EMBED], vs[(j + 1) % 3][EMBED])
    _gate_sum(r, vs, _names(m), "tiny k=3")
    # a second run of the window: identical bits (fixed-order reductions, one add of the old value)
    _, r2 = _alone_and_window(m, batches, SPLIT, d.max_text_len)
    for n in _names(m):
        assert torch.equal(r[n], r2[n]), n
    # embedding rows no micro-batch touches stay exactly zero (no memset ran in accumulating mode, nothing else wrote them)
    ge = r[EMBED].view(d.vocab, d.hidden)
    never = ~touched.any(0)
    assert int(never.sum()) > 0
    assert int(torch.count_nonzero(ge[never.cuda()])) == 0
    # rows touched by one micro-batch only carry exactly that micro-batch's value (old value 0 or + 0)
    for j in range(3):
        rows = (once & touched[j]).cuda()
        assert torch.equal(ge[rows], vs[j][EMBED].view(d.vocab, d.hidden)[rows]), j


# ---------------------------------------------------------------- 2. the same at production width

def _full_width_case():
    """full-width 2-layer model, the stage-1 batch of test_full_width_two_layer_stage1_batch_gradients_vs_oracle_autograd
    (15 t2i + 4 lm + 10 mmu x 387 = 11 223 token rows) and a seeded re-draw of it, k = 2"""
    from stub_tokenizer import StubTokenizer
    import random
    P = util.pkg()
    d = Wt.ShowoDims(hidden=2048, layers=2, heads=32, ffn=8192, vocab=1000 + 10 + 512 + 1, llm_vocab=1000, codebook=512,
                     num_vq_tokens=256, max_text_len=128)
    sd_np = Wt.make_showo_state(d, seed=19)
    bt, bl, bm = 15, 4, 10
    m = util.build_showo(d, sd_np, max_batch=bt + bl + bm, max_seq=387).train()
    up = P.UniversalPrompting(StubTokenizer(vocab=d.llm_vocab, bos=d.llm_vocab - 10, eos=d.llm_vocab - 10), max_text_len=d.max_text_len,
                              cond_dropout_prob=0.1)
    rs = np.random.RandomState(23)
    words = [f"w{i}" for i in range(400)]

    def text(n):
        return " ".join(words[j] for j in rs.randint(0, len(words), size=n))

    N = d.num_vq_tokens
    texts_t2i = [text(int(k)) for k in rs.randint(3, 60, size=bt)]
    texts_lm = [text(int(k)) for k in rs.randint(100, 500, size=bl)]
    texts_mmu = [text(int(k)) for k in rs.randint(5, 110, size=bm)]
    cfg = type("Cfg", (), {"training": type("S", (dict,), {"__getattr__": dict.__getitem__})(min_masking_rate=0.0)})
    batches = []
    for seed in (5, 6):  # seed 5 = the batch of the oracle test; seed 6 = the re-draw (image tokens, masked positions, dropped captions)
        torch.manual_seed(seed)
        random.seed(seed)
        img_t2i = torch.randint(0, d.codebook, (bt, N), device="cuda") + d.image_offset
        img_mmu = torch.randint(0, d.codebook, (bm, N), device="cuda") + d.image_offset
        ids, labels, imask, _, (b1, b2, b3) = P.training_utils.build_training_batch(
            up, cfg, d.mask_token_id, P.cosine_schedule, img_t2i, list(texts_t2i), list(texts_lm), img_mmu, list(texts_mmu))
        assert (b1, b2, b3) == (bt, bl, bm) and tuple(ids.shape) == (29, 387)
        batches.append((ids.to(torch.int64).contiguous(), imask, labels.to(torch.int64).contiguous()))
    assert not torch.equal(batches[0][0], batches[1][0])
    _gemm_counters(reset=True)
    vs, r = _alone_and_window(m, batches, (bt, bl, bm), d.max_text_len)
    cnt = _gemm_counters()
    assert cnt[2] > 0, cnt  # split-K launches ran (the weight gradients contract over 11 223 token rows)
    _gate_sum(r, vs, _names(m), f"full-width k=2 TN={os.environ.get('SHOWO_TRAIN_TN', '1')}")
    touched = _rows_touched([b[0].cpu() for b in batches], d.vocab)
    never = ~touched.any(0)
    if int(never.sum()):
        assert int(torch.count_nonzero(r[EMBED].view(d.vocab, d.hidden)[never.cuda()])) == 0


def test_window_is_the_sum_full_width_stage1_batch():
    _full_width_case()


# ---------------------------------------------------------------- 3. against the oracle

def test_window_gradients_vs_oracle_autograd_of_the_mean_loss():
    """oracle autograd (fp32, CPU) of sum_j (W . losses_j) / k over the three tiny micro-batches vs the window's buffer; the gates of
    test_tiny_training_step_vs_reference_golden: fp32 sums of bf16-operand gradients stay in their error class"""
    k = 3
    d, sd_np, batches, host = _tiny_micro_batches(k)
    m = util.build_showo(d, sd_np).train()
    w = tuple(c / k for c in W)
    for j, b in enumerate(batches):
        _micro(m, b, SPLIT, d.max_text_len, w, j > 0)
    r = _snapshot(m)
    sd = {n: v.clone().requires_grad_(True) for n, v in O.to_torch(sd_np).items()}
    mask = batches[0][1].cpu()
    total = 0.0
    for ids, labels in host:
        _, l1, l2, l3 = O.showo_forward(sd, d, ids, attention_mask=mask, labels=labels, batch_size_t2i=SPLIT[0], batch_size_lm=SPLIT[1],
                                        batch_size_mmu=SPLIT[2], max_seq_length=d.max_text_len)
        total = total + (W[0] * l1 + W[1] * l2 + W[2] * l3) / k
    total.backward()
    for n, p in m.named_parameters():
        want = sd[n].grad
        assert want is not None, n
        rmax, rrms = util.relerr(r[n].view(want.shape), want)
        print(f"[parity] accumulated grad {n}: rel_max={rmax:.3e} rel_rms={rrms:.3e}")
        assert rrms < 3e-2 and rmax < 8e-2, n


# ---------------------------------------------------------------- 4. k = 1 is today's step

def test_k1_is_the_plain_step_bit_for_bit():
    P = util.pkg()
    d, sd, batches, _ = _tiny_micro_batches(2)
    a = util.build_showo(d, sd).train()
    b = util.build_showo(d, sd).train()
    ta = P.Trainer(a, lr=1e-3)
    tb = P.Trainer(b, lr=1e-3, gradient_accumulation_steps=1)
    for batch in batches:
        la = ta.step(batch[0], batch[1], batch[2], *SPLIT, d.max_text_len)
        lb = tb.step(batch[0], batch[1], batch[2], *SPLIT, d.max_text_len)
        assert torch.equal(la, lb)
        assert tb.sync_gradients and torch.equal(tb.window_losses(), lb)
    assert ta.step_count == tb.step_count == 2
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q), n
    for n in ta.m:
        assert torch.equal(ta.m[n], tb.m[n]) and torch.equal(ta.v[n], tb.v[n]), n


# ---------------------------------------------------------------- 5. window semantics

def test_window_semantics_k3():
    P = util.pkg()
    k = 3
    d, sd, batches, _ = _tiny_micro_batches(k)
    # the reference value of the clipped norm: fp64 norm of sum_j v_j (each v_j already carries the 1 / k), test 1's quantities
    m0 = util.build_showo(d, sd).train()
    w = tuple(c / k for c in W)
    tot = None
    for b in batches:
        _micro(m0, b, SPLIT, d.max_text_len, w, 0)
        v = _snapshot(m0)
        tot = {n: v[n].double() for n in v} if tot is None else {n: tot[n] + v[n].double() for n in v}
    want_norm = float(torch.sqrt(sum((t ** 2).sum() for t in tot.values())))
    del m0
    m = util.build_showo(d, sd).train()
    tr = P.Trainer(m, lr=1e-3, gradient_accumulation_steps=k, max_grad_norm=1e6)
    assert tr.sync_gradients is False and tr.step_count == 0
    counts, syncs, norms, seen = [], [], [], []
    for call in range(2 * k):
        b = batches[call % k]
        before = {n: p.detach().clone() for n, p in m.named_parameters()}
        if m._trainer is not None:
            _counters(m, reset=True)
        losses = tr.step(b[0], b[1], b[2], *SPLIT, d.max_text_len)
        torch.cuda.synchronize()
        closes = call % k == k - 1
        counts.append(tr.step_count)
        syncs.append(tr.sync_gradients)
        changed = any(not torch.equal(p, before[n]) for n, p in m.named_parameters())
        assert changed == closes, call
        # the transposed weight images follow the masters: rebuilt by the first forward and by the forward after a closing call only
        rebuilt = _counters(m)["transposes"]
        assert (rebuilt > 0) == (call % k == 0), (call, rebuilt)
        if call < k:
            seen.append(losses.clone())
        if not closes:
            with pytest.raises(RuntimeError, match="accumulation window"):
                tr.state_dict()
        else:
            norms.append(float(tr.grad_norm))
            if call == k - 1:
                assert torch.allclose(tr.window_losses(), torch.stack(seen).mean(0), rtol=0, atol=1e-6)
                assert abs(norms[0] - want_norm) <= 1e-5 * want_norm, (norms[0], want_norm)
    assert counts == [0, 0, 1, 1, 1, 2], counts
    assert syncs == [False, False, True, False, False, True], syncs
    # after a closed window the optimizer state round-trips
    st = tr.state_dict()
    m2 = util.build_showo(d, sd).train()
    tr2 = P.Trainer(m2, lr=5e-4, gradient_accumulation_steps=k)
    tr2.load_state_dict(st)
    assert tr2.step_count == 2 and tr2.lr == 1e-3
    for n in tr.m:
        assert torch.equal(tr.m[n], tr2.m[n]) and torch.equal(tr.v[n], tr2.v[n]), n
    # requires_grad changes are still refused
    m.showo.lm_head.bias.requires_grad_(False)
    with pytest.raises(RuntimeError, match="requires_grad"):
        tr.step(batches[0][0], batches[0][1], batches[0][2], *SPLIT, d.max_text_len)


# ---------------------------------------------------------------- 6. against the accumulating autograd path

def test_window_matches_the_accumulating_autograd_path():
    """the unchanged-train.py path ((loss / k).backward() k times into param.grad, one torch AdamW step) vs one native window:
    the flat gradient buffer per tensor (not the weights: a gradient that is ~0 by construction, k_layernorm.bias, turns Adam's
    update into +-lr noise) and the micro-batch losses"""
    P = util.pkg()
    k = 3
    d, sd, batches, _ = _tiny_micro_batches(k)
    ref = util.build_showo(d, sd).train()
    m = util.build_showo(d, sd).train()
    named = list(ref.named_parameters())
    opt = torch.optim.AdamW([{"params": [p for n, p in named if not any(x in n for x in NO_DECAY)], "weight_decay": 0.01},
                             {"params": [p for n, p in named if any(x in n for x in NO_DECAY)], "weight_decay": 0.0}],
                            lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    tr = P.Trainer(m, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, coeffs=W, gradient_accumulation_steps=k)
    kw = dict(batch_size_t2i=SPLIT[0], batch_size_lm=SPLIT[1], batch_size_mmu=SPLIT[2], max_seq_length=d.max_text_len)
    opt.zero_grad()
    for ids, mask, labels in batches:
        _, l1, l2, l3 = ref(ids, attention_mask=mask, labels=labels, **kw)
        ((W[0] * l1 + W[1] * l2 + W[2] * l3) / k).backward()
        losses = tr.step(ids, mask, labels, *SPLIT, d.max_text_len)
        assert torch.allclose(losses.cpu(), torch.stack([l1, l2, l3]).detach().cpu(), rtol=1e-4, atol=1e-5)
    want = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    opt.step()
    assert tr.sync_gradients and tr.step_count == 1
    for n in _names(m):
        g = _grad_view(m, n).double()
        dn = float((g - want[n].reshape(-1).double()).norm())
        gn = float(want[n].double().norm())
        print(f"[accum] native window vs autograd accumulation {n}: |d| = {dn:.3e}, |g| = {gn:.3e}")
        assert dn <= 1e-5 * gn + 1e-9, n


# ---------------------------------------------------------------- 7. exchange once per window

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


def test_exchange_runs_once_per_window_inside_the_closing_call():
    _one_rank_group()
    P = util.pkg()
    k = 3
    d, sd, batches, _ = _tiny_micro_batches(k)
    a = util.build_showo(d, sd).train()
    b = util.build_showo(d, sd).train()
    ta = P.Trainer(a, lr=1e-3, wire="fp32", gradient_accumulation_steps=k)
    tb = P.Trainer(b, lr=1e-3, wire="fp32", force_exchange=True, gradient_accumulation_steps=k)
    assert ta.exchange is None and tb.exchange is not None
    log = []
    real = tb.exchange.launch
    call = [0]
    tb.exchange.launch = lambda bucket: (log.append((call[0], bucket)), real(bucket))
    for j, (ids, mask, labels) in enumerate(batches):
        call[0] = j
        la = ta.step(ids, mask, labels, *SPLIT, d.max_text_len)
        lb = tb.step(ids, mask, labels, *SPLIT, d.max_text_len)
        assert torch.equal(la, lb)
    nL = d.layers
    # one launch per trainable bucket, all inside the third call: head -> blocks last to first -> embedding
    assert log == [(k - 1, x) for x in [nL + 1] + list(range(nL, 0, -1)) + [0]], log
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q), n


# ---------------------------------------------------------------- 8. frozen buckets

def test_frozen_buckets_stay_zero_in_a_window():
    k = 2
    d, sd, batches, _ = _tiny_micro_batches(k)
    m = util.build_showo(d, sd).train()
    m.showo.model.embed_tokens.requires_grad_(False)
    m.showo.model.layers[0].requires_grad_(False)
    m.trainer()
    _counters(m, reset=True)
    vs, r = _alone_and_window(m, batches, SPLIT, d.max_text_len)
    cnt = _counters(m)
    assert cnt["embed"] == 0, cnt  # no embedding-phase launch: neither a clear nor a scatter
    assert cnt["phases"] == 2 * k * (d.layers - 1), cnt
    trainable = [n for n, p in m.named_parameters() if p.requires_grad]
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    assert EMBED in frozen and any(".layers.0." in n for n in frozen) and len(trainable) > 0
    for n in frozen:
        assert int(torch.count_nonzero(r[n])) == 0, n
    _gate_sum(r, vs, trainable, "frozen k=2")
    for n in trainable:
        if "k_layernorm.bias" not in n:
            assert int(torch.count_nonzero(r[n])) > 0, n


# ---------------------------------------------------------------- 2b. production width, SHOWO_TRAIN_TN=0 (a child process: last)

def test_window_is_the_sum_full_width_transpose_branch_in_a_child_process():
    """SHOWO_TRAIN_TN=0 (read once per process): the transpose + NT-GEMM weight-gradient branch accumulates through the residual
    epilogue and the transpose's accumulating column sums"""
    env = dict(os.environ, SHOWO_TRAIN_TN="0")
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); import test_train_accum_gpu as t; t._full_width_case(); print('CHILD_OK')" % here)
    r = subprocess.run([sys.executable, "-s", "-c", code], env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
