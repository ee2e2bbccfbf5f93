"""`Showo` — drop-in replacement of the reference class `models.modeling_showo.Showo`
(reference models/modeling_showo.py:23-240) backed by the gfx950 engine in libshowo_hip.so.

Same constructor arguments, attributes (`config.mask_token_id`, `mask_token_id`, `vocab_size`,
`output_size`, `showo.model.embed_tokens`, `showo.resize_token_embeddings`, `mm_projector`) and state-dict
keys as the reference, so `inference_t2i.py` / `inference_mmu.py` call it unchanged.
The torch modules below are *parameter containers only* (they give `state_dict()` / `load_state_dict()`
the reference's names and shapes); all arithmetic runs in HIP kernels through the C ABI.  There is no
PyTorch fallback: without a GPU or without the built library every compute entry point raises.
"""
import collections
import contextlib
import math
import numbers
import types

import torch
import torch.nn as nn

from . import _lib
from .persistence import PretrainedMixin
from .sampling import cosine_schedule, t2i_step_constants

# microsoft/phi-1_5 architecture numbers (what AutoConfig.from_pretrained(llm_model_path) yields in the
# reference, models/modeling_showo.py:42; PhiConfig defaults)
PHI_1_5 = dict(hidden_size=2048, intermediate_size=8192, num_hidden_layers=24, num_attention_heads=32,
               max_position_embeddings=2048, layer_norm_eps=1e-5, rope_theta=10000.0, partial_rotary_factor=0.5)


# what `Showo.score` / `MmuSession.score` return: log-probabilities (fp32) and ranks (int32; -1 = not scored) of the given tokens
TokenScores = collections.namedtuple("TokenScores", ["logprobs", "ranks"])


class _Cfg(dict):
    """attribute-style config like the reference's diffusers FrozenDict (`model.config.mask_token_id`)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def get(self, k, default=None):
        return dict.get(self, k, default)


class _PhiAttentionParams(nn.Module):
    def __init__(self, hidden, head_dim, eps):
        super().__init__()
        self.q_proj = nn.Linear(hidden, hidden, bias=True)
        self.k_proj = nn.Linear(hidden, hidden, bias=True)
        self.v_proj = nn.Linear(hidden, hidden, bias=True)
        self.dense = nn.Linear(hidden, hidden, bias=True)
        self.q_layernorm = nn.LayerNorm(head_dim, eps=eps)  # forced on by PhiForCausalLM (reference models/phi.py:1088)
        self.k_layernorm = nn.LayerNorm(head_dim, eps=eps)


class _PhiMLPParams(nn.Module):
    def __init__(self, hidden, ffn):
        super().__init__()
        self.fc1 = nn.Linear(hidden, ffn)
        self.fc2 = nn.Linear(ffn, hidden)


class _PhiLayerParams(nn.Module):
    def __init__(self, hidden, ffn, head_dim, eps):
        super().__init__()
        self.self_attn = _PhiAttentionParams(hidden, head_dim, eps)
        self.mlp = _PhiMLPParams(hidden, ffn)
        self.input_layernorm = nn.LayerNorm(hidden, eps=eps)


class _PhiModelParams(nn.Module):
    def __init__(self, vocab, hidden, ffn, layers, head_dim, eps):
        super().__init__()
        self.embed_tokens = nn.Embedding(vocab, hidden)
        self.layers = nn.ModuleList([_PhiLayerParams(hidden, ffn, head_dim, eps) for _ in range(layers)])
        self.final_layernorm = nn.LayerNorm(hidden, eps=eps)


class _PhiForCausalLMParams(nn.Module):
    """Names mirror reference models/phi.py:1084-1095 (`model`, untied biased `lm_head`)."""

    def __init__(self, vocab, hidden, ffn, layers, head_dim, eps):
        super().__init__()
        self.model = _PhiModelParams(vocab, hidden, ffn, layers, head_dim, eps)
        self.lm_head = nn.Linear(hidden, vocab, bias=True)
        self.vocab_size = vocab
        for m in self.modules():  # Phi init: N(0, 0.02), zero biases (reference models/phi.py:833-842)
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Embedding):
                nn.init.normal_(m.weight, std=0.02)

    def resize_token_embeddings(self, new_vocab):
        """reference: PreTrainedModel.resize_token_embeddings called at models/modeling_showo.py:46."""
        old = self.model.embed_tokens.weight.shape[0]
        if new_vocab == old:
            return self.model.embed_tokens
        hidden = self.model.embed_tokens.weight.shape[1]
        dev = self.model.embed_tokens.weight.device
        emb = nn.Embedding(new_vocab, hidden, device=dev)
        head = nn.Linear(hidden, new_vocab, bias=True, device=dev)
        nn.init.normal_(emb.weight, std=0.02)
        nn.init.normal_(head.weight, std=0.02)
        nn.init.zeros_(head.bias)
        n = min(old, new_vocab)
        with torch.no_grad():
            emb.weight[:n] = self.model.embed_tokens.weight[:n]
            head.weight[:n] = self.lm_head.weight[:n]
            head.bias[:n] = self.lm_head.bias[:n]
        self.model.embed_tokens, self.lm_head, self.vocab_size = emb, head, new_vocab
        return emb

    def get_input_embeddings(self):
        return self.model.embed_tokens


class _TrainRun:
    """What the autograd nodes of ONE labelled Showo.forward share: the model, the trainer handle and generation of the HIP forward
    they belong to (showo_train_generation), the arguments of the backward and the gradient layout of the trainer's buckets."""

    def __init__(self, model):
        self.model, self.tr, self.gen = model, None, None

    def check(self, node):
        """the trainer still holds this forward's activations: no other training forward ran since (a labelled forward, Trainer.step)"""
        tr = self.model.__dict__.get("_trainer")
        if self.gen is None or tr is not self.tr or _lib.load().showo_train_generation(tr) != self.gen:
            raise RuntimeError(f"Showo backward ({node}): another training forward ran on this model after the one this loss comes from, "
                               "so its saved activations are gone; call backward() before the next labelled forward")

    def hand_out(self, bucket, needs):
        """the gradients of bucket `bucket` that autograd asks for (`needs`, one flag per parameter in the order of _train_param_groups;
        None for the others) in fresh tensors: ONE device copy of the whole bucket when every parameter needs its gradient, else one
        copy per needed tensor.  Autograd / DDP may keep them, the next backward overwrites only the trainer's own buffer."""
        n, src, parts = self.layout[bucket]
        needs = list(needs)
        if all(needs):
            buf = torch.empty(n, dtype=torch.float32, device=src.device)
            buf.copy_(src)
            return [buf[o:o + k].view(shape) for o, k, shape in parts]
        return [src[o:o + k].clone().view(shape) if need else None for (o, k, shape), need in zip(parts, needs)]


def _train_param_groups(model):
    """model.showo's parameters per gradient bucket of the trainer (include/showo_hip.h showo_train_bucket): 0 = embedding, 1 + i = block i,
    nL + 1 = final LayerNorm + lm_head; (state-dict key, parameter) pairs"""
    ph = model.showo
    groups = [[("showo.model.embed_tokens.weight", ph.model.embed_tokens.weight)]]
    for i, layer in enumerate(ph.model.layers):
        groups.append([(f"showo.model.layers.{i}.{n}", p) for n, p in layer.named_parameters()])
    groups.append([("showo.model.final_layernorm." + n, p) for n, p in ph.model.final_layernorm.named_parameters()] +
                  [("showo.lm_head." + n, p) for n, p in ph.lm_head.named_parameters()])
    return groups


def sync_trainable(model, tr, flags, input_grad):
    """hand the trainable set {state-dict key: trains} and the input-gradient flag to the native trainer (showo_train_set_trainable /
    showo_train_set_input_grad): only what differs from what that trainer handle was last told"""
    st = model.__dict__.get("_trainable_state")
    if st is None or st[0] is not tr:
        st = (tr, {}, True)  # a new trainer: everything trainable, input gradient on
    known, inp = st[1], st[2]
    for k, on in flags.items():
        if known.get(k, True) != bool(on):
            _lib.call("showo_train_set_trainable", tr, k.encode(), int(bool(on)))
            known[k] = bool(on)
    if inp != bool(input_grad):
        _lib.call("showo_train_set_input_grad", tr, int(bool(input_grad)))
    model.__dict__["_trainable_state"] = (tr, known, bool(input_grad))


def _grad_layout(model, tr, groups, device):
    """per bucket: (element count, zero-copy view of the trainer's bucket, [(offset, numel, shape) of each parameter's gradient]) --
    offsets from showo_train_grad; cached for the lifetime of the trainer handle"""
    cached = model.__dict__.get("_grad_layout_cache")
    if cached is not None and cached[0] is tr:
        return cached[1]
    import ctypes as C
    from .training import device_view
    lib = _lib.load()
    if lib.showo_train_num_buckets(tr) != len(groups):
        raise RuntimeError("trainer buckets do not match the model's parameter groups")
    layout = []
    for b, group in enumerate(groups):
        bp, bn = C.c_void_p(), C.c_int64()
        _lib.check(lib.showo_train_bucket(tr, b, C.byref(bp), C.byref(bn)), "showo_train_bucket")
        parts = []
        for name, p in group:
            gp, gn = C.c_void_p(), C.c_int64()
            _lib.check(lib.showo_train_grad(tr, name.encode(), C.byref(gp), C.byref(gn)), "showo_train_grad")
            off = (gp.value - bp.value) // 4
            if gn.value != p.numel() or off < 0 or off + gn.value > bn.value:
                raise RuntimeError(f"{name}: gradient outside its bucket {b}")
            parts.append((off, gn.value, tuple(p.shape)))
        layout.append((bn.value, device_view(bp.value, bn.value, device), parts))
    model.__dict__["_grad_layout_cache"] = (tr, layout)
    return layout


class _EmbedNode(torch.autograd.Function):
    """bucket 0 of the chain Showo.forward(labels=...) builds (embedding -> block 0 .. nL-1 -> head): launches nothing forward; its
    backward, last of the chain, runs the embedding phase of the HIP backward and hands out the embedding-table gradient and, for the
    `input_embeddings` flow (reference modeling_showo.py:77-78), d(loss)/d(input_embeddings) to the caller's graph (`anchor`)."""

    @staticmethod
    def forward(ctx, run, anchor, embed_w):
        ctx.run = run
        return embed_w.new_empty(0)

    @staticmethod
    def backward(ctx, g_tok):
        run = ctx.run
        run.check("embedding")
        _lib.call("showo_train_backward_embed", run.tr, _lib.stream())
        (g_w,) = run.hand_out(0, ctx.needs_input_grad[2:3])
        g_emb = None
        if run.emb_shape is not None and ctx.needs_input_grad[1]:
            g_emb = torch.empty(run.emb_shape[0], dtype=torch.float32, device=run.lab.device)
            _lib.call("showo_train_input_grad", run.tr, _lib.ptr(g_emb), g_emb.numel(), _lib.stream())
            g_emb = g_emb.to(run.emb_shape[1])
        return None, g_emb, g_w


class _BlockNode(torch.autograd.Function):
    """block i (bucket 1 + i): no forward work; the backward runs showo_train_backward_layer(i) and hands out the block's gradients, so
    their AccumulateGrad hooks (DDP's bucket readiness) fire while the blocks below are still to be queued."""

    @staticmethod
    def forward(ctx, run, i, tok, *params):
        ctx.run, ctx.i = run, i
        return tok.new_empty(0)

    @staticmethod
    def backward(ctx, g_tok):
        run = ctx.run
        run.check(f"block {ctx.i}")
        _lib.call("showo_train_backward_layer", run.tr, ctx.i, _lib.stream())
        return (None, None, g_tok.new_empty(0)) + tuple(run.hand_out(1 + ctx.i, ctx.needs_input_grad[3:]))


class _HeadNode(torch.autograd.Function):
    """Showo.forward with labels (reference models/modeling_showo.py:80-102): the forward runs the whole HIP training forward (ONE call;
    activations stay in the trainer) and returns logits + the three losses; the backward -- first of the chain -- runs the loss + head
    phase for the incoming loss gradients read on the device (no host synchronisation) and hands out the final LayerNorm and lm_head
    gradients (bucket nL + 1)."""

    @staticmethod
    def forward(ctx, run, input_ids, attention_mask, labels, b_t2i, b_lm, b_mmu, max_seq_length, tok, *params):
        model = run.model
        tr = model.trainer()
        lab = labels.to(torch.int64).contiguous()
        B, L = lab.shape
        if attention_mask is not None and tuple(attention_mask.shape) != (B, 1, L, L):
            raise ValueError(f"Attention mask should be of size {(B, 1, L, L)}, but is {tuple(attention_mask.shape)}")
        from .training import train_mask
        # the trainable set of this forward's backward: requires_grad of every parameter, and of the input embeddings
        sync_trainable(model, tr, {k: p.requires_grad for g in run.groups for k, p in g}, run.emb_grad)
        mask = train_mask(tr, attention_mask)  # dense fp32 mask, or an IntervalMask registered with the trainer
        logits = torch.empty((B, L, model.vocab_size), dtype=torch.float32, device=lab.device)
        losses = torch.empty(3, dtype=torch.float32, device=lab.device)
        try:
            if run.emb is None:
                ids = input_ids.to(torch.int64).contiguous()
                _lib.call("showo_train_forward", tr, _lib.ptr(ids), _lib.ptr(mask), _lib.ptr(lab), B, L, b_t2i, b_lm, b_mmu,
                          max_seq_length, _lib.ptr(logits), _lib.ptr(losses), _lib.stream())
            else:  # `inputs_embeds` flow of the w_clip_vit trainer (reference modeling_showo.py:77-78)
                emb = run.emb.float().contiguous()
                if tuple(emb.shape) != (B, L, model.arch["hidden_size"]):
                    raise ValueError(f"input_embeddings should be {(B, L, model.arch['hidden_size'])}, got {tuple(emb.shape)}")
                _lib.call("showo_train_forward_embeds", tr, _lib.ptr(emb), _lib.ptr(mask), _lib.ptr(lab), B, L, b_t2i, b_lm, b_mmu,
                          max_seq_length, _lib.ptr(logits), _lib.ptr(losses), _lib.stream())
        finally:
            _lib.call("showo_trainer_use_intervals", tr, None, None)
        run.tr, run.gen = tr, _lib.load().showo_train_generation(tr)
        run.layout = _grad_layout(model, tr, run.groups, lab.device)
        run.lab, run.meta = lab, (b_t2i, b_lm, b_mmu, max_seq_length)
        ctx.run = run
        ctx.mark_non_differentiable(logits)
        ctx.set_materialize_grads(False)  # no [B, L, V] zeros for the logits; an unused loss arrives as None (weight 0)
        return logits, losses[0].clone(), losses[1].clone(), losses[2].clone()

    @staticmethod
    def backward(ctx, g_logits, g_t2i, g_lm, g_mmu):
        run = ctx.run
        run.check("head")
        dev = run.lab.device
        g3 = torch.stack([torch.zeros((), dtype=torch.float32, device=dev) if g is None else g.detach().reshape(()).float()
                          for g in (g_t2i, g_lm, g_mmu)])  # the loss weights stay on the device (training/train.py:600)
        b_t2i, b_lm, b_mmu, msl = run.meta
        _lib.call("showo_train_backward_head_dev", run.tr, _lib.ptr(run.lab), b_t2i, b_lm, b_mmu, msl, _lib.ptr(g3), _lib.stream())
        return ((None,) * 8 + (torch.empty(0, device=dev),) + tuple(run.hand_out(len(run.groups) - 1, ctx.needs_input_grad[9:])))


def _train_forward(model, input_ids, input_embeddings, attention_mask, labels, b_t2i, b_lm, b_mmu, max_seq_length):
    """Showo.forward with labels as a chain of autograd nodes, one per gradient bucket (embedding -> blocks -> head): autograd
    runs their backwards head -> block nL-1 .. 0 -> embedding and accumulates every bucket's gradients as soon as its phase is queued,
    which is when DDP (accelerator.prepare, training/train.py:449) starts that bucket's all-reduce.  The tok tensors are empty: they
    only carry the graph edges."""
    run = _TrainRun(model)
    run.groups = _train_param_groups(model)
    run.emb = None if input_embeddings is None else input_embeddings.detach()
    run.emb_shape = None if input_embeddings is None else (tuple(input_embeddings.shape), input_embeddings.dtype)
    run.emb_grad = input_embeddings is not None and input_embeddings.requires_grad
    (embed_w,) = [p for _, p in run.groups[0]]
    tok = _EmbedNode.apply(run, input_embeddings, embed_w)
    for i, group in enumerate(run.groups[1:-1]):
        tok = _BlockNode.apply(run, i, tok, *[p for _, p in group])
    return _HeadNode.apply(run, input_ids, attention_mask, labels, b_t2i, b_lm, b_mmu, max_seq_length, tok,
                           *[p for _, p in run.groups[-1]])


class _ProjectorFn(torch.autograd.Function):
    """mm_projector as one autograd node: HIP forward, HIP backward (csrc/clip_engine.hip: showo_projector_backward).  The
    backward re-runs the (two small GEMMs of the) forward on the saved input, so interleaved calls cannot mix up saved state."""

    @staticmethod
    def forward(ctx, mod, x, w0, b0, w1, b1):
        ctx.mod = mod
        ctx.save_for_backward(x)
        return mod._hip_forward(x)

    @staticmethod
    def backward(ctx, g):
        mod, (x,) = ctx.mod, ctx.saved_tensors
        din, dout_dim = mod._dims
        mod._hip_forward(x)  # restores the engine's saved activations for exactly these rows
        gout = g.detach().float().contiguous()
        T = gout.numel() // dout_dim
        dev = gout.device
        gw0 = torch.empty((dout_dim, din), dtype=torch.float32, device=dev)
        gb0 = torch.empty((dout_dim,), dtype=torch.float32, device=dev)
        gw1 = torch.empty((dout_dim, dout_dim), dtype=torch.float32, device=dev)
        gb1 = torch.empty((dout_dim,), dtype=torch.float32, device=dev)
        dx = torch.empty(tuple(x.shape), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        _lib.call("showo_projector_backward", mod._proj, _lib.ptr(gout), T, _lib.ptr(dx), _lib.ptr(gw0), _lib.ptr(gb0), _lib.ptr(gw1),
                  _lib.ptr(gb1), _lib.stream())
        return None, (None if dx is None else dx.to(x.dtype)), gw0, gb0, gw1, gb1


class _MMProjector(nn.Sequential):
    """`model.mm_projector` (reference modeling_showo.py:48-53): same parameters and state-dict keys (mm_projector.0.*,
    mm_projector.2.*).  Forward and backward run on the HIP projector (two MFMA GEMMs + exact GELU and their autograd,
    csrc/clip_engine.hip): inference_mmu.py:134 as well as the w_clip_vit trainer that fine-tunes these 6 M parameters."""

    def __init__(self, din, dout):
        super().__init__(nn.Linear(din, dout), nn.GELU(), nn.Linear(dout, dout))
        self._dims = (din, dout)
        self._proj, self._rows, self._versions = None, 0, None

    def set_precision(self, precision):
        """0 (default): bf16 GEMM operands.  1: accuracy mode of the projector -- split-bf16 (hi + lo) MFMA GEMMs and the exact GELU in
        fp32 (csrc/clip_engine.hip showo_projector_set_precision): nn.Sequential(Linear, GELU, Linear) in fp32 to ~1e-5.  Inference
        only (the backward differentiates the bf16-operand forward).  `Showo.set_precision` forwards here."""
        if int(precision) not in (0, 1):
            raise ValueError("precision must be 0 (bf16 operands) or 1 (split-bf16, fp32-class)")
        self._precision = int(precision)
        if getattr(self, "_proj", None) is not None:
            _lib.call("showo_projector_set_precision", self._proj, self._precision)
            if self._precision == 1 and not _lib.load().showo_projector_precise_ready(self._proj):
                self._versions = {}  # the low halves are made by the loader (allocated on first use): upload the weights again
        return self

    def mark_weights_dirty(self):
        """re-upload the projector's parameters at the next call (updates through `.data` do not bump tensor versions)"""
        if getattr(self, "_proj", None) is not None:
            self._versions = {}

    def _drop(self):
        if getattr(self, "_proj", None) is not None:
            _lib.load().showo_projector_destroy(self._proj)
        self._proj, self._versions = None, None

    def __del__(self):
        try:
            self._drop()
        except Exception:
            pass

    def _hip_forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("show-o_amd runs the projector on the GPU (no CPU path exists)")
        import ctypes as C
        din, dout = self._dims
        xin = x.detach().float().contiguous()
        T = xin.numel() // din
        if self._proj is None or T > self._rows:
            self._drop()
            h = C.c_void_p()
            self._rows = max(T, 576)
            _lib.check(_lib.load().showo_projector_create(din, dout, self._rows, C.byref(h)), "showo_projector_create")
            self._proj, self._versions = h, {}
            _lib.call("showo_projector_set_precision", self._proj, int(getattr(self, "_precision", 0)))
        for k, v in self.state_dict().items():
            ver = (v.data_ptr(), v._version)
            if self._versions.get(k) != ver:
                src = v.detach().float().contiguous()
                _lib.call("showo_projector_load", self._proj, k.encode(), _lib.ptr(src), src.numel(), _lib.stream())
                self._versions[k] = ver
                torch.cuda.current_stream().synchronize()
        out = torch.empty(tuple(x.shape[:-1]) + (dout,), dtype=torch.float32, device=x.device)
        _lib.call("showo_projector_forward", self._proj, _lib.ptr(xin), T, _lib.ptr(out), _lib.stream())
        return out.to(x.dtype)

    def forward(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return _ProjectorFn.apply(self, x, self[0].weight, self[0].bias, self[2].weight, self[2].bias)
        return self._hip_forward(x)


class Showo(PretrainedMixin, nn.Module):
    _supports_gradient_checkpointing = True
    # the reference's @register_to_config arguments (models/modeling_showo.py:26-37) = the keys of its config.json
    _config_keys = ("w_clip_vit", "vocab_size", "llm_vocab_size", "llm_model_path", "codebook_size", "num_vq_tokens", "load_from_showo")

    def _extra_config(self):
        return {k: v for k, v in self.arch.items() if PHI_1_5.get(k) != v}

    def __init__(self, w_clip_vit, vocab_size, llm_vocab_size, llm_model_path='', codebook_size=8192,
                 num_vq_tokens=256, load_from_showo=True, **kwargs):
        super().__init__()
        arch = dict(PHI_1_5)
        arch.update({k: kwargs[k] for k in PHI_1_5 if k in kwargs})
        self.arch = arch
        self.config = _Cfg(w_clip_vit=w_clip_vit, vocab_size=vocab_size, llm_vocab_size=llm_vocab_size,
                           llm_model_path=llm_model_path, codebook_size=codebook_size, num_vq_tokens=num_vq_tokens,
                           load_from_showo=load_from_showo, mask_token_id=vocab_size - 1)
        self.vocab_size = vocab_size
        hidden, heads = arch["hidden_size"], arch["num_attention_heads"]
        if hidden // heads != 64:
            raise ValueError("the gfx950 attention kernel is built for head_dim 64 (Phi-1.5)")
        # the reference builds Phi with its native vocabulary and then resizes (modeling_showo.py:43-46); the
        # end state (embed + untied lm_head of `vocab_size` rows) is what we allocate directly.
        self.showo = _PhiForCausalLMParams(vocab_size, hidden, arch["intermediate_size"], arch["num_hidden_layers"],
                                           64, arch["layer_norm_eps"])
        if not load_from_showo:
            # reference models/modeling_showo.py:45-46: PhiForCausalLM.from_pretrained(llm_model_path) then
            # resize_token_embeddings(vocab_size) -- stage-1 training starts from the HF Phi-1.5 weights (training/train.py:203)
            self._init_from_phi_checkpoint(llm_model_path)
        self.output_size = self.vocab_size
        if w_clip_vit:
            self.mm_projector = _MMProjector(1024, hidden)  # reference: nn.Sequential(Linear(1024, 2048), GELU(), Linear(2048, 2048))
        self._engine = None
        self._engine_key = None
        self._engine_versions = None
        self._trainer = None
        self.max_batch = int(kwargs.get("max_batch", 32))
        self.max_seq = int(kwargs.get("max_seq", 1280))
        self._precision = 0

    def _init_from_phi_checkpoint(self, llm_model_path):
        """`load_from_showo=False`: start from a Hugging Face Phi checkpoint in the local directory `llm_model_path`
        (config.json + model.safetensors | pytorch_model.bin | a sharded index; keys `model.*`, `lm_head.*`).  What the reference does
        (models/modeling_showo.py:45-46; transformers `from_pretrained` + `resize_token_embeddings`):
          * every checkpoint tensor is loaded under the `showo.` prefix; tensors the checkpoint lacks keep their fresh
            initialisation -- for microsoft/phi-1_5 those are the q/k LayerNorms that PhiForCausalLM forces on (models/phi.py:1088):
            weight 1, bias 0;
          * the embedding and the untied, biased lm_head grow from the checkpoint's vocabulary to `vocab_size`: the first
            min(old, new) rows (and bias entries) are the checkpoint's, the new rows are N(0, 0.02) / zero bias (`_init_weights`).
        There is no hub access here: anything but a local directory raises."""
        import json
        import os
        from .persistence import _load_file
        if self.showo.lm_head.weight.is_meta:
            return  # from_pretrained() builds on the meta device and overwrites every tensor from the Show-o checkpoint itself
        d = llm_model_path
        if not d or not os.path.isdir(d):
            raise EnvironmentError(f"load_from_showo=False needs a local Hugging Face Phi checkpoint directory as llm_model_path "
                                   f"(got {llm_model_path!r}); hub downloads are not supported")
        cfg_path = os.path.join(d, "config.json")
        if os.path.isfile(cfg_path):
            with open(cfg_path, encoding="utf-8") as f:
                hf = json.load(f)
            for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads"):
                if k in hf and hf[k] != self.arch[k]:
                    raise ValueError(f"{cfg_path}: {k} = {hf[k]} but the model was built with {self.arch[k]} "
                                     f"(pass {k}=... to Showo for a non-Phi-1.5 geometry)")
        files = None
        for name in ("model.safetensors", "pytorch_model.safetensors", "pytorch_model.bin"):
            if os.path.isfile(os.path.join(d, name)):
                files = [os.path.join(d, name)]
                break
            idx = os.path.join(d, name + ".index.json")
            if os.path.isfile(idx):
                with open(idx, encoding="utf-8") as f:
                    files = [os.path.join(d, fn) for fn in sorted(set(json.load(f)["weight_map"].values()))]
                break
        if files is None:
            raise EnvironmentError(f"no model.safetensors / pytorch_model.bin (or sharded index) in {d}")
        want = self.showo.state_dict()
        for k, v in want.items():  # fresh initialisation of what a Phi-1.5 checkpoint does not hold
            if k.endswith("_layernorm.weight") and ("q_layernorm" in k or "k_layernorm" in k):
                v.data.fill_(1.0)
            elif k.endswith("_layernorm.bias") and ("q_layernorm" in k or "k_layernorm" in k):
                v.data.zero_()
        seen = set()
        resized = ("model.embed_tokens.weight", "lm_head.weight", "lm_head.bias")
        with torch.no_grad():
            for path in files:
                part = _load_file(path, "cpu")
                for k, v in part.items():
                    if k not in want:
                        continue
                    dst = want[k]
                    if k in resized:
                        n = min(v.shape[0], dst.shape[0])
                        if tuple(v.shape[1:]) != tuple(dst.shape[1:]):
                            raise ValueError(f"{k}: checkpoint shape {tuple(v.shape)} does not match {tuple(dst.shape)} beyond the vocabulary")
                        dst[:n].copy_(v[:n])
                    else:
                        if tuple(v.shape) != tuple(dst.shape):
                            raise ValueError(f"{k}: checkpoint shape {tuple(v.shape)} != model shape {tuple(dst.shape)}")
                        dst.copy_(v)
                    seen.add(k)
                del part
        allowed_missing = [k for k in want if "q_layernorm" in k or "k_layernorm" in k]
        missing = [k for k in want if k not in seen and k not in allowed_missing]
        if missing:
            raise KeyError(f"Phi checkpoint {d} lacks {len(missing)} tensors, e.g. {missing[:5]}")

    def set_precision(self, precision):
        """0 (default): bf16 GEMM / attention operands with fp32 accumulation -- the timed path.  1: accuracy mode, the reference's
        fp32 inference (inference_t2i.py:67, models/phi.py:1182-1183) to ~1e-4 end to end: split-bf16 (hi + lo) MFMA GEMMs, fp32
        LayerNorm / RoPE / attention / gelu_new.  At Phi-1.5's shape this mode runs on the PRODUCTION kernels (K-concatenated split
        images, csrc/engine.hip run_layers_precise_fast): same launches as precision 0 with three MFMAs per product, prefix reuse,
        hipGraph replay and the KV-cached decode included; tiny test shapes use the fp32 reference kernels of csrc/precise.hip (and
        mmu_generate then runs the reference's own no-cache algorithm).  Applies to forward() without labels, t2i_generate() and
        mmu_generate(); training keeps bf16 operands.  Costs 4x the bf16 weight memory.  With w_clip_vit the mm_projector follows.
        2: fp16 (IEEE half) operands on the SAME kernels, launches, prefix reuse and hipGraph replay as precision 0 -- the MFMA rate is
        the same, operand rounding is 2^-12 instead of 2^-9 -- with the final LayerNorm + lm_head as the split-bf16 product of
        precision 1: logits within 1e-3 of the reference's fp32 inference (rel_rms ~8e-4 at model scale where bf16 operands give
        7e-3) at the speed of the default path.  Converts saturate at +-65504 (`range_check()` counts saturated activations);
        the KV-cached decode steps run the fp16 instances of the fused three-launch layer and of the batched layer (csrc/decode.hip, decode_batch.hip; the lm_head of a decode step is one fused LayerNorm + (hi, lo) GEMV launch), the
        mm_projector runs in its fp32-class mode (it is one small MLP).  Switching to / from 2 re-uploads the weight images.
        3: int8 decode -- the one mode that trades accuracy for speed, so it is opt-in.  Every GEMM weight (q/k/v_proj, dense, fc1,
        fc2 of the blocks, lm_head) is quantised per output row to int8 with an fp32 scale amax / 127 (`showo_amd.quantization`); the
        model IS that quantised model on every entry point (prefill, forward, t2i_generate run bf16 operands on bf16(q * scale)), and
        the KV-cached decode steps of mmu_generate stream the int8 images: half the weight bytes per token (csrc/decode.hip, Q8
        instances; int8 converts exactly to bf16, one extra fp32 multiply by the row scale per output).  Cost in accuracy: logits
        rel_rms ~2.6e-2 against the unquantised fp32 model on seeded full-size weights (bf16 operands alone: 5e-3), see README.
        Cost in memory: + 1 byte per GEMM weight (1.45 GB at model scale) next to the bf16 images.  mmu_generate_batch runs the int8
        instances of the batched kernels (every sequence bit-identical to its batch-1 run).  Needs hidden <= 2048 and ffn <= 8192, multiples of 16 (the
        engine refuses other shapes).  Training maps 3 to 0 like 2; switching to / from 3 re-uploads (re-quantises) the weights."""
        if int(precision) not in (0, 1, 2, 3):
            raise ValueError("precision must be 0 (bf16 operands), 1 (split-bf16, fp32-class), 2 (fp16 operands) or 3 (int8 decode weights)")
        self._precision = int(precision)
        if self.__dict__.get("_modules", {}).get("mm_projector") is not None:
            self.mm_projector.set_precision(1 if int(precision) else 0)
        return self

    def range_check(self, fn):
        """Precision-2 diagnostic: run `fn()` (any forward / generate call of this model) with the engine's range check on and
        return the number of fp16 activation elements that left a convert saturated (|x| = 65504) or non-finite (csrc/engine.hip
        range_check; extra launches, not for timed runs).  0 on random-init weights; a deployment on a real checkpoint runs this once."""
        eng = self.engine()
        cnt = torch.zeros(1, dtype=torch.int64, device=self.showo.lm_head.weight.device)
        _lib.call("showo_engine_set_range_check", eng, _lib.ptr(cnt))
        try:
            fn()
        finally:
            _lib.call("showo_engine_set_range_check", self._engine, None)
        return int(cnt.item())

    def mark_weights_dirty(self):
        """Re-upload every parameter to the HIP engine at the next call.  The engine notices parameter changes by
        (data_ptr, tensor._version); updates made through `.data` (p.data.copy_(), DeepSpeed ZeRO flat-buffer updates, EMA swaps)
        do not bump the version counter, so an optimizer of that kind must call this after `optimizer.step()`."""
        self._engine_versions = {} if self._engine is not None else None
        if getattr(self, "mm_projector", None) is not None:
            self.mm_projector.mark_weights_dirty()

    # ---- reference attribute passthrough (`model.mask_token_id`, reference models/modeling_utils.py:139-155)
    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            cfg = self.__dict__.get("config")
            if cfg is not None and name in cfg:
                return cfg[name]
            raise

    def _set_gradient_checkpointing(self, module, value=False):
        self.gradient_checkpointing = True

    @classmethod
    def from_state_dict(cls, state_dict, device="cuda", **ctor):
        m = cls(**ctor)
        m.load_state_dict(state_dict, strict=True)
        return m.to(device)

    # ---- engine management -------------------------------------------------------------------------
    def configure_workspace(self, max_batch, max_seq):
        """Size the engine's HBM workspaces (tokens = max_batch * max_seq).  Re-creates the engine."""
        self.max_batch, self.max_seq = int(max_batch), int(max_seq)
        self._drop_engine()

    def _drop_engine(self):
        if getattr(self, "_trainer", None) is not None:
            _lib.load().showo_train_destroy(self._trainer)
            self._trainer = None
        if self._engine is not None:
            _lib.load().showo_engine_destroy(self._engine)
        self._engine, self._engine_versions = None, None

    def trainer(self):
        """HIP training state (saved activations, transposed weight images, fp32 gradient buffers); created lazily."""
        eng = self.engine(for_training=True)
        if self._trainer is None:
            import ctypes as C
            h = C.c_void_p()
            _lib.check(_lib.load().showo_train_create(eng, self.max_batch, self.max_seq, C.byref(h)), "showo_train_create")
            self._trainer = h
        # no invalidation here: every upload engine() makes stamps the tensor's version, and the trainer rebuilds the images of the
        # tensors that changed (include/showo_hip.h showo_train_invalidate_weights)
        return self._trainer

    def __del__(self):
        try:
            self._drop_engine()
        except Exception:
            pass

    def _engine_params(self):
        return [(k, v) for k, v in self.showo.state_dict(prefix="showo.").items()]

    def _rope_tables(self, device):
        # exactly PhiRotaryEmbedding._set_cos_sin_cache (reference models/phi.py:86-102), fp32, on the host
        a = self.arch
        dim = int(a["partial_rotary_factor"] * 64)
        inv_freq = 1.0 / (a["rope_theta"] ** (torch.arange(0, dim, 2, dtype=torch.int64).float() / dim))
        t = torch.arange(a["max_position_embeddings"], dtype=torch.int64).type_as(inv_freq)
        freqs = torch.outer(t, inv_freq)
        emb = torch.cat((freqs, freqs), dim=-1)
        return emb.cos().contiguous().to(device), emb.sin().contiguous().to(device)

    def engine(self, for_training=False):
        """Create the HIP engine if needed and (re)upload weights whose version changed.  for_training: the trainer works on bf16
        weight images, so a model in precision 2 (fp16 images) or 3 (images of the int8-dequantised weights) trains on a precision-0
        engine (and re-uploads on the way back)."""
        _lib.require_gpu()
        lib = _lib.load()
        dev = self.showo.lm_head.weight.device
        if dev.type != "cuda":
            raise RuntimeError("Showo parameters must live on the GPU (model.to('cuda')); no CPU path exists")
        a = self.arch
        if self._engine is None:
            import ctypes as C
            cfg = _lib.EngineConfig(hidden=a["hidden_size"], layers=a["num_hidden_layers"], heads=a["num_attention_heads"],
                                    ffn=a["intermediate_size"], vocab=self.vocab_size,
                                    rotary_dim=int(a["partial_rotary_factor"] * 64), max_pos=a["max_position_embeddings"],
                                    ln_eps=a["layer_norm_eps"], rope_theta=a["rope_theta"],
                                    max_batch=self.max_batch, max_seq=self.max_seq)
            h = C.c_void_p()
            _lib.check(lib.showo_engine_create(C.byref(cfg), C.byref(h)), "showo_engine_create")
            self._engine = h
            self._engine_versions = {}
            cos, sin = self._rope_tables(dev)
            _lib.call("showo_engine_load", self._engine, b"rope.cos", _lib.ptr(cos), cos.numel(), _lib.stream())
            _lib.call("showo_engine_load", self._engine, b"rope.sin", _lib.ptr(sin), sin.numel(), _lib.stream())
            torch.cuda.current_stream().synchronize()
        want = int(getattr(self, "_precision", 0))
        if for_training and want in (2, 3):  # the trainer works on the bf16 images of the fp32 masters
            want = 0
        if lib.showo_engine_get_precision(self._engine) != want:
            _lib.call("showo_engine_set_precision", self._engine, want)
        if want == 1 and not lib.showo_engine_precise_ready(self._engine):
            self._engine_versions = {}  # the low halves of the weights are made by the loader: upload everything again
        if lib.showo_engine_missing(self._engine):
            self._engine_versions = {}  # first use, or the weight images changed their element type / values (precision 2 or 3 <-> others)
        for k, v in self._engine_params():
            ver = (v.data_ptr(), v._version)
            if self._engine_versions.get(k) != ver:
                src = v.detach()
                if src.dtype != torch.float32 or not src.is_contiguous():
                    src = src.float().contiguous()
                _lib.call("showo_engine_load", self._engine, k.encode(), _lib.ptr(src), src.numel(), _lib.stream())
                self._engine_versions[k] = ver
                if src is not v:
                    torch.cuda.current_stream().synchronize()  # keep the temporary alive until consumed
        missing = lib.showo_engine_missing(self._engine)
        if missing:
            raise RuntimeError(f"engine is missing {missing} tensors")
        return self._engine

    def _use_mask(self, eng, attention_mask):
        """dense additive mask -> contiguous fp32 tensor; IntervalMask (prompting_utils.intervals_*) -> registered with the
        engine, returns None (the call then passes no dense mask)"""
        from .prompting_utils import IntervalMask
        if isinstance(attention_mask, IntervalMask):
            attention_mask.check()
            _lib.call("showo_engine_use_intervals", eng, _lib.ptr(attention_mask.iv), _lib.ptr(attention_mask.flag))
            return None
        return attention_mask.detach().float().contiguous()

    # ---- Showo.forward (reference models/modeling_showo.py:59-102) -------------------------------------
    def forward(self, input_ids, input_embeddings=None, attention_mask=None, labels=None, label_smoothing=0.0,
                batch_size_t2i=0, batch_size_lm=0, batch_size_mmu=0, max_seq_length=128, labels_mask_text=None,
                labels_mask_image=None, **kwargs):
        if labels is not None:
            return _train_forward(self, input_ids, input_embeddings, attention_mask, labels, int(batch_size_t2i), int(batch_size_lm),
                                  int(batch_size_mmu), int(max_seq_length))
        eng = self.engine()
        if input_embeddings is None:
            B, L = input_ids.shape
            ids = input_ids.to(torch.int64).contiguous()
            emb = None
            dev = ids.device
        else:
            B, L = input_embeddings.shape[:2]
            ids = None
            emb = input_embeddings.detach().float().contiguous()
            dev = emb.device
        mask = None
        if attention_mask is not None:
            if tuple(attention_mask.shape) != (B, 1, L, L):  # same check as the eager path, reference models/phi.py:368-372
                raise ValueError(f"Attention mask should be of size {(B, 1, L, L)}, but is {tuple(attention_mask.shape)}")
            mask = self._use_mask(eng, attention_mask)
        logits = torch.empty((B, L, self.vocab_size), dtype=torch.float32, device=dev)
        try:
            _lib.call("showo_engine_forward", eng, _lib.ptr(ids), _lib.ptr(emb), _lib.ptr(mask), B, L, _lib.ptr(logits),
                      _lib.stream())
        finally:
            _lib.call("showo_engine_use_intervals", eng, None, None)
        if labels is None:
            return logits
        raise AssertionError("unreachable")

    # ---- Showo.score: log-probabilities of given tokens, without [B, L, vocab] logits --------------------------------------
    def _score_rows(self, ids, emb, mask, B, L, rows, targets, chunk_rows):
        """(log-probabilities fp32 [n], ranks int32 [n]) of targets int64 [n] under the logits of the residual rows int32 [n] of one
        forward (showo_engine_score); the caller has registered an IntervalMask, if any"""
        n = int(rows.numel())
        lp = torch.empty((n,), dtype=torch.float32, device=rows.device)
        rk = torch.empty((n,), dtype=torch.int32, device=rows.device)
        try:
            _lib.call("showo_engine_score", self.engine(), _lib.ptr(ids), _lib.ptr(emb), _lib.ptr(mask), B, L, _lib.ptr(rows), _lib.ptr(targets), n,
                      0 if chunk_rows is None else int(chunk_rows), _lib.ptr(lp), _lib.ptr(rk), _lib.stream())
        finally:
            _lib.call("showo_engine_use_intervals", self.engine(), None, None)
        return lp, rk

    @torch.no_grad()
    def score(self, input_ids=None, input_embeddings=None, attention_mask=None, labels=None, shift=True, chunk_rows=None):
        """How probable the tokens `labels` (int64 [B, L], -100 = not scored) are: `TokenScores(logprobs, ranks)`, fp32 / int32 [B, L].
        shift=True (autoregressive rows): entry [b, r] scores labels[b, r] from the logits of row r - 1, column 0 is never scored;
        shift=False (the t2i mask-prediction form, reference modeling_showo.py:83-86): entry [b, r] is scored from row r.  logprobs
        are the log-softmax of the raw logits at the label, ranks the number of strictly larger logits; unscored entries are 0.0 / -1,
        so `logprobs.sum(-1)` is the sequence log-likelihood.  Inputs and masks (dense or IntervalMask) as in `forward`.  One forward,
        then the head on the scored rows alone in chunks of `chunk_rows` rows (default: 256 MB of logits at most): no [B, L, vocab]
        tensor exists at any time."""
        if (input_ids is None) == (input_embeddings is None):
            raise ValueError("exactly one of input_ids / input_embeddings must be given")
        if labels is None:
            raise ValueError("score needs labels")
        eng = self.engine()
        if input_embeddings is None:
            B, L = input_ids.shape
            ids, emb = input_ids.to(torch.int64).contiguous(), None
            dev = ids.device
        else:
            B, L = input_embeddings.shape[:2]
            ids, emb = None, input_embeddings.detach().float().contiguous()
            dev = emb.device
        if tuple(labels.shape) != (B, L):
            raise ValueError(f"labels should be of size {(B, L)}, but is {tuple(labels.shape)}")
        if chunk_rows is not None and int(chunk_rows) < 1:
            raise ValueError("chunk_rows must be >= 1")
        lab = labels.to(torch.int64).to(dev).reshape(-1)
        sel = (lab >= 0).reshape(B, L).clone()
        if shift:
            sel[:, 0] = False
        at = sel.reshape(-1).nonzero().reshape(-1)
        lp = torch.zeros((B * L,), dtype=torch.float32, device=dev)
        rk = torch.full((B * L,), -1, dtype=torch.int32, device=dev)
        if at.numel():
            mask = None
            if attention_mask is not None:
                if tuple(attention_mask.shape) != (B, 1, L, L):
                    raise ValueError(f"Attention mask should be of size {(B, 1, L, L)}, but is {tuple(attention_mask.shape)}")
                mask = self._use_mask(eng, attention_mask)
            rows = (at - 1 if shift else at).to(torch.int32).contiguous()
            a, b = self._score_rows(ids, emb, mask, B, L, rows, lab[at].contiguous(), chunk_rows)
            lp[at], rk[at] = a, b
        return TokenScores(lp.reshape(B, L), rk.reshape(B, L))

    # ---- Showo.t2i_generate (reference models/modeling_showo.py:104-181) -----------------------------------
    def t2i_generate(self, input_ids=None, uncond_input_ids=None, attention_mask=None, temperature=1.0, timesteps=18,
                     guidance_scale=0, noise_schedule=cosine_schedule, generator=None, config=None,
                     _exp_noise=None, _uniform=None, **kwargs):
        eng = self.engine()
        N = config.model.showo.num_vq_tokens
        offset = config.model.showo.llm_vocab_size + config.model.showo.num_new_special_tokens
        text_len = config.dataset.preprocessing.max_seq_length
        B, L = input_ids.shape
        if input_ids.dtype != torch.int64 or not input_ids.is_contiguous():
            raise ValueError("input_ids must be a contiguous int64 tensor (it is updated in place like the reference)")
        codebook = self.vocab_size - 1 - offset  # logits[..., offset:-1] (reference :144)
        unc = None
        if uncond_input_ids is not None and guidance_scale > 0:
            unc = uncond_input_ids.to(torch.int64).contiguous()
        mask = None if attention_mask is None else self._use_mask(eng, attention_mask)
        import ctypes as C
        ml, tp = t2i_step_constants(timesteps, N, temperature, noise_schedule)
        ml_a = (C.c_float * timesteps)(*ml)
        tp_a = (C.c_float * timesteps)(*tp)
        seed = _draw_seed(generator)
        out = torch.empty((B, N), dtype=torch.int64, device=input_ids.device)
        # the denoise steps run as replays of ONE captured hipGraph (cached on the engine across calls) unless use_graph=0 is
        # passed or per-launch event timing is on (the engine then runs the steps eagerly)
        use_graph = int(kwargs.get("use_graph", 1))
        # bit 0: hipGraph replay of the denoise step; bit 1: recompute the step-invariant text rows every step (A/B switch);
        # bit 2: run every row of every sequence in step 0 (reduce_step0=False; A/B switch)
        flags = (1 if use_graph else 0) | (0 if kwargs.get("reuse_prefix", True) else 2) | (0 if kwargs.get("reduce_step0", True) else 4)

        def run():
            _lib.call("showo_engine_t2i_generate", eng, _lib.ptr(input_ids), _lib.ptr(unc), _lib.ptr(mask), B, L, N, text_len,
                      self.config.mask_token_id, offset, codebook, float(guidance_scale), timesteps,
                      C.cast(ml_a, C.c_void_p), C.cast(tp_a, C.c_void_p), seed, _lib.ptr(_exp_noise), _lib.ptr(_uniform),
                      flags, _lib.ptr(out), _lib.stream())

        if use_graph:
            with _graph_stream_of(self):  # hipGraph replay of the denoise step: stream capture needs a non-default stream
                run()
        else:
            run()
        _lib.call("showo_engine_use_intervals", eng, None, None)
        return out

    # ---- Showo.mmu_generate (reference models/modeling_showo.py:183-240) -----------------------------------
    @torch.no_grad()
    def mmu_generate(self, idx=None, input_embeddings=None, attention_mask=None, max_new_tokens=100, temperature=1.0,
                     top_k=None, eot_token=None, generator=None, _exp_noise=None, top_p=None, return_logprobs=False,
                     repetition_penalty=None, repetition_context=None, logit_bias=None, allowed_tokens=None, banned_tokens=None,
                     num_beams=None, length_penalty=1.0, early_stopping=False, num_return_sequences=1, return_beam_scores=False,
                     no_repeat_ngram_size=None, bad_words_ids=None, min_new_tokens=None, stop_sequences=None):
        """reference signature + `generator` (seeds the on-device Philox stream of the multinomial draws; default: torch's
        global generator), `_exp_noise` fp32 [max_new_tokens, vocab] (parity tests inject the reference's Exp(1) draws) and `top_p`
        (nucleus sampling on the device behind the top-k filter, the reference's top_k_top_p_filtering: a token stays iff the mass of
        the strictly more probable candidates is <= top_p; None or >= 1: off, <= 0: ValueError; top_k == 1 stays the arg-max).
        `return_logprobs=True` returns `(tokens, logprobs)`: logprobs fp32 [len(tokens)] on the device, entry j the log-softmax of the
        RAW logits (temperature 1, no filter) at token j -- one more launch per decode step (showo_engine_decode_sample_lp); the
        tokens are those of the call without it.

        Logit adjustment ("Logit adjustment"; all None: exactly the calls above, no bit changes), applied on the device in
        front of the pick, in Hugging Face's order (repetition penalty, then bias, then temperature / top-k / top-p):
        `repetition_penalty` theta (finite, > 0): a token of the set S has its logit x replaced by x * theta if x < 0, else x / theta.
        S is per call: it starts as the ids of `repetition_context` (a tensor or list of ids; None: empty) and every token this call
        produces joins it as it is fed back; nothing persists across calls.  Hugging Face's set is the whole `input_ids`, which
        an `input_embeddings` prompt does not have: pass `repetition_context=idx[0]` for that behaviour.
        `logit_bias` ({id: float} or an fp32 [vocab] tensor; -inf bans, +inf / NaN: ValueError) is added to the penalised logits;
        `banned_tokens` puts -inf on the listed ids, `allowed_tokens` puts -inf everywhere else -- if it leaves out `eot_token` the
        call runs to `max_new_tokens`.  A row without a finite token, ids outside the vocabulary, theta <= 0 / NaN / inf: ValueError
        before the engine is touched.  `return_logprobs` stays the log-softmax of the RAW logits, adjusted or not.

        Sequence rules ("Sequence rules"; all None: exactly the calls above, no bit changes).  The history of a call is the ids
        of `repetition_context` followed by every token the call has produced.  `no_repeat_ngram_size` n (an int in 1..16): no n-gram of
        the history may occur twice (Hugging Face's NoRepeatNGramLogitsProcessor); `bad_words_ids` (a list of id sequences): a sequence
        is never completed (NoBadWordsLogitsProcessor; a one-token sequence is a banned token); `min_new_tokens` m (needs `eot_token`):
        `eot_token` is banned while fewer than m tokens have been produced; all three put -inf on the banned tokens on the device,
        behind the repetition penalty and the bias and in front of temperature / top-k / top-p.  `stop_sequences` (a list of id
        sequences): the answer ends behind the first position at which the produced tokens end with one of them (it is part of the
        answer, as <eot> is; whichever of <eot>, a stop sequence and max_new_tokens comes first wins).  Nothing persists across calls.
        An empty sequence, ids outside the vocabulary, n outside 1..16, min_new_tokens < 0 or without eot_token, any of the four with
        beams: ValueError before the engine is touched.

        Beam search ("Beam search"; `num_beams` None or 1: exactly the calls above, no bit changes): `num_beams` 2..8 runs
        Hugging Face's beam search (do_sample=False, no processors) on the device, the beams as the slots of a decode batch forked
        from the prompt's cache.  A hypothesis that ends on `eot_token` scores sum of log-probabilities / len ** `length_penalty`;
        `early_stopping` (a bool) stops once `num_beams` hypotheses are finished.  The best hypothesis comes back in the return type
        above (it includes its `eot_token`); `num_return_sequences` > 1 returns a list of them, best first;
        `return_logprobs=True` adds the per-token log-probabilities of each, `return_beam_scores=True` their final scores (fp32
        [num_return_sequences], last).  Beams take top_k None / 1 only, and no `top_p`, `temperature` != 1, `generator`, noise or
        logit-adjustment keyword; precision 1 has no beams: ValueError before the engine is touched."""
        adj_kw = {k_: v for k_, v in zip(_ADJUST_KEYS, (repetition_penalty, repetition_context, logit_bias, allowed_tokens, banned_tokens))
                  if v is not None}
        adj_kw.update({k_: v for k_, v in zip(_SEQ_KEYS, (no_repeat_ngram_size, bad_words_ids, min_new_tokens, stop_sequences)) if v is not None})
        beams = _beam_request(self, num_beams, length_penalty, early_stopping, num_return_sequences, return_beam_scores, max_new_tokens,
                              temperature, top_k, top_p, generator, _exp_noise, bool(adj_kw))
        if beams is not None:
            if (idx if input_embeddings is None else input_embeddings).shape[0] != 1:
                raise ValueError("mmu_generate has batch-1 semantics (reference modeling_showo.py:204,229)")
            eng = self.engine()
            dev = idx.device if input_embeddings is None else input_embeddings.device
            logits = torch.empty((self.vocab_size,), dtype=torch.float32, device=dev)
            L = _prefill(eng, *_prompt_args(self, eng, None if input_embeddings is not None else idx, input_embeddings, attention_mask), logits)
            hyps = _beam_search(self, eng, logits, L, beams, max_new_tokens, eot_token, float(length_penalty), early_stopping, dev)
            return _beam_result(hyps, num_return_sequences, return_logprobs, return_beam_scores, dev)
        adjust = _adjust_of(self.vocab_size, eot_token=eot_token, **adj_kw) if adj_kw else None
        adj_kw = {} if adjust is None else {"adjust": adjust}  # (None: the calls below are those of a call without the keywords)
        # greedy (top_k == 1) is the reference caller's setting (inference_mmu.py:81): multinomial of a one-hot = arg-max
        greedy, k, noise, seed, p = _draw_params(self, max_new_tokens, temperature, top_k, top_p, generator, _exp_noise)
        eng = self.engine()
        dev = idx.device if idx is not None else input_embeddings.device
        # accuracy mode: KV-cached like precision 0 when the engine runs it on the production kernels (Phi-1.5's shape); otherwise -- or
        # with `self.precise_recompute = True` -- the reference's own no-cache algorithm on the fp32-class path
        if int(getattr(self, "_precision", 0)) == 1 and (getattr(self, "precise_recompute", False) or
                                                         not _lib.load().showo_engine_precise_fast(eng)):
            return self._mmu_generate_recompute(idx, input_embeddings, attention_mask, max_new_tokens, temperature, top_k, eot_token,
                                                greedy, None if greedy else (k, seed, noise), top_p=p, return_logprobs=return_logprobs,
                                                **adj_kw)
        if input_embeddings is not None:
            idx = None
        if (idx if idx is not None else input_embeddings).shape[0] != 1:
            raise ValueError("mmu_generate has batch-1 semantics (reference modeling_showo.py:204,229)")
        logits = torch.empty((self.vocab_size,), dtype=torch.float32, device=dev)
        tok = torch.empty((1,), dtype=torch.int64, device=dev)
        # (an IntervalMask, prompting_utils.intervals_for_mmu / _mmu_vit: no [1,1,L,L] tensor at all)
        _prefill(eng, *_prompt_args(self, eng, idx, input_embeddings, attention_mask), logits)
        out = _decode_batch1(self, eng, logits, tok, max_new_tokens, (greedy, k, p, temperature, noise, seed), eot_token, return_logprobs,
                             **adj_kw)
        toks, lps = out if return_logprobs else (out, None)
        toks = [torch.tensor(t, device=dev) for t in toks]
        return (toks, lps) if return_logprobs else toks


def _nucleus_p(top_p):
    """the `top_p` of the mmu decode paths: None (off) for None and for top_p >= 1, the float inside (0, 1), ValueError for top_p <= 0
    or NaN.  None takes the calls of a decode without nucleus sampling, so an unset top_p changes no bit."""
    if top_p is None:
        return None
    p = float(top_p)
    if not p > 0:
        raise ValueError("top_p must be > 0 (>= 1 or None: no nucleus filter)")
    return None if p >= 1 else p


# ---- logit adjustment: repetition penalty, logit bias, allowed / banned tokens ("Logit adjustment") ----------------------------
class _Adjust:
    """one request's logit adjustment: `theta` (the repetition penalty, 1.0: none), `bias` (None or the dense fp32 [V] row on the CPU:
    logit_bias, allowed_tokens and banned_tokens combined) and `context` (the ids the set of seen tokens starts with)"""
    __slots__ = ("theta", "bias", "context", "rules")

    def __init__(self, theta, bias, context, rules=None):
        self.theta, self.bias, self.context, self.rules = theta, bias, context, rules  # rules: None or the request's _SeqRules


def _token_ids(V, ids, what):
    """`ids` (None, a tensor, any iterable of ints) as a list of ints inside [0, V); ValueError for anything else"""
    if ids is None:
        return []
    if isinstance(ids, torch.Tensor):
        ids = ids.detach().reshape(-1).tolist()
    out = []
    for t in ids:
        if isinstance(t, bool) or not isinstance(t, numbers.Integral):
            raise ValueError(f"{what}: token ids must be integers, got {t!r}")
        if not 0 <= int(t) < V:
            raise ValueError(f"{what}: token id {int(t)} outside [0, {V})")
        out.append(int(t))
    return out


def _bias_row(V, logit_bias=None, allowed_tokens=None, banned_tokens=None):
    """the dense fp32 [V] bias row (CPU) of one request, or None when it would change nothing: `logit_bias` ({id: float} or an fp32
    [V] tensor), -inf everywhere outside `allowed_tokens`, -inf on `banned_tokens`.  ValueError: ids out of range, +inf or NaN in the
    bias, a row that leaves no finite token."""
    if logit_bias is None and allowed_tokens is None and banned_tokens is None:
        return None
    if isinstance(logit_bias, torch.Tensor):
        if logit_bias.numel() != V:
            raise ValueError(f"logit_bias: a tensor must hold vocab_size = {V} values")
        row = logit_bias.detach().to(torch.float32).cpu().reshape(-1).clone()
    else:
        row = torch.zeros((V,), dtype=torch.float32)
        for t, v in (dict(logit_bias).items() if logit_bias is not None else ()):
            row[_token_ids(V, [t], "logit_bias")[0]] = float(v)
    if bool(torch.isnan(row).any()) or bool((row == float("inf")).any()):
        raise ValueError("logit_bias: +inf and NaN are refused (-inf bans a token)")
    if allowed_tokens is not None:
        keep = torch.zeros((V,), dtype=torch.bool)
        keep[torch.tensor(_token_ids(V, allowed_tokens, "allowed_tokens"), dtype=torch.int64)] = True
        row[~keep] = float("-inf")
    if banned_tokens is not None:
        row[torch.tensor(_token_ids(V, banned_tokens, "banned_tokens"), dtype=torch.int64)] = float("-inf")
    if not bool(torch.isfinite(row).any()):
        raise ValueError("logit_bias / allowed_tokens / banned_tokens leave no finite token")
    return row if bool((row != 0).any()) else None


def _adjust_of(V, repetition_penalty=None, repetition_context=None, logit_bias=None, allowed_tokens=None, banned_tokens=None,
               no_repeat_ngram_size=None, bad_words_ids=None, min_new_tokens=None, stop_sequences=None, eot_token=None):
    """the _Adjust of one request, or None when the keywords change nothing (all None, or a penalty of 1 without a bias row and no
    sequence rule): such a request takes exactly the calls of one without the keywords.  ValueError for a penalty <= 0, NaN or inf and
    for what _bias_row, _token_ids and _seq_rules_of refuse -- before anything touches the engine.  A request with sequence rules
    alone is a penalty of 1 without a bias row: its adjust launch is a bit copy."""
    theta = 1.0 if repetition_penalty is None else float(repetition_penalty)
    if not (theta > 0 and math.isfinite(theta)):
        raise ValueError("repetition_penalty must be finite and > 0 (1: none)")
    context = _token_ids(V, repetition_context, "repetition_context")
    rules, single = _seq_rules_of(V, no_repeat_ngram_size, bad_words_ids, min_new_tokens, stop_sequences, eot_token)
    if single:  # bad words of one token are banned tokens: they live in the bias row
        banned_tokens = _token_ids(V, banned_tokens, "banned_tokens") + single
    row = _bias_row(V, logit_bias, allowed_tokens, banned_tokens)
    if theta == 1.0 and row is None and rules is None:
        return None
    return _Adjust(theta, row, context, rules)


_ADJUST_KEYS = ("repetition_penalty", "repetition_context", "logit_bias", "allowed_tokens", "banned_tokens")
_SEQ_KEYS = ("no_repeat_ngram_size", "bad_words_ids", "min_new_tokens", "stop_sequences")

# ---- sequence rules: no-repeat n-grams, multi-token bad words, minimum length, stop sequences ("Sequence rules") ---------------
_SEQ_NGRAM_MAX = 16     # csrc/seq_rules.h SEQ_NGRAM_MAX
_SEQ_BAD_MAX = 1024     # bad-word sequences per request (the kernel walks any number: this bounds the table a request may upload)
_SEQ_BAD_LEN_MAX = 64   # tokens per bad-word sequence
_SEQ_STOP_MAX = 256     # stop sequences per request, each of at most _SEQ_BAD_LEN_MAX tokens (host work)


class _SeqRules:
    """one request's sequence rules: `ngram` (0: off), `bad` (the bad-word sequences of two tokens and more, tuples of ints), `min_new`
    (0: off) and `stops` (the stop sequences, host work).  `table`: the flat int32 bad-word table of include/showo_hip.h (CPU) or None."""
    __slots__ = ("ngram", "bad", "min_new", "stops", "table")

    def __init__(self, ngram, bad, min_new, stops):
        self.ngram, self.bad, self.min_new, self.stops = ngram, bad, min_new, stops
        self.table = None
        if bad:
            off = [0]
            for q in bad:
                off.append(off[-1] + len(q))
            self.table = torch.tensor([len(bad)] + off + [t for q in bad for t in q], dtype=torch.int32)

    @property
    def device(self):
        """the request has a rule the device computes (stop sequences alone are host work)"""
        return bool(self.ngram or self.bad or self.min_new)


def _token_seqs(V, seqs, what, limit):
    """`seqs` (a list / tuple of id collections, or a 2-D tensor) as a list of tuples of ints inside [0, V); ValueError for an empty
    sequence, ids outside the vocabulary, more than `limit` sequences or more than _SEQ_BAD_LEN_MAX tokens in one"""
    if isinstance(seqs, torch.Tensor):
        if seqs.dim() != 2:
            raise ValueError(f"{what}: a tensor must be 2-D (one sequence per row)")
        seqs = seqs.tolist()
    if not isinstance(seqs, (list, tuple)):
        raise ValueError(f"{what}: a list of token-id sequences")
    if len(seqs) > limit:
        raise ValueError(f"{what}: at most {limit} sequences")
    out = []
    for q in seqs:
        if not isinstance(q, (list, tuple, torch.Tensor)):
            raise ValueError(f"{what}: every entry is a sequence of token ids, got {q!r}")
        ids = _token_ids(V, q, what)
        if not ids:
            raise ValueError(f"{what}: an empty sequence")
        if len(ids) > _SEQ_BAD_LEN_MAX:
            raise ValueError(f"{what}: at most {_SEQ_BAD_LEN_MAX} tokens per sequence")
        out.append(tuple(ids))
    return out


def _seq_rules_of(V, no_repeat_ngram_size=None, bad_words_ids=None, min_new_tokens=None, stop_sequences=None, eot_token=None):
    """(the _SeqRules of one request or None when the keywords change nothing, the ids of its one-token bad words).  ValueError: a
    no_repeat_ngram_size that is not an int in 1.._SEQ_NGRAM_MAX, an empty or over-long sequence, ids outside the vocabulary, a
    min_new_tokens that is not an int >= 0 or comes without an eot_token."""
    n = 0
    if no_repeat_ngram_size is not None:
        n = no_repeat_ngram_size
        if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 1 <= int(n) <= _SEQ_NGRAM_MAX:
            raise ValueError(f"no_repeat_ngram_size must be an int in 1..{_SEQ_NGRAM_MAX}")
        n = int(n)
    m = 0
    if min_new_tokens is not None:
        m = min_new_tokens
        if isinstance(m, bool) or not isinstance(m, numbers.Integral) or int(m) < 0:
            raise ValueError("min_new_tokens must be an int >= 0")
        if eot_token is None:
            raise ValueError("min_new_tokens needs an eot_token (it is the token the rule holds back)")
        m = int(m)
    bad = [] if bad_words_ids is None else _token_seqs(V, bad_words_ids, "bad_words_ids", _SEQ_BAD_MAX)
    stops = [] if stop_sequences is None else _token_seqs(V, stop_sequences, "stop_sequences", _SEQ_STOP_MAX)
    single = [q[0] for q in bad if len(q) == 1]
    bad = [q for q in bad if len(q) > 1]
    if not (n or m or bad or stops):
        return None, single
    return _SeqRules(n, bad, m, stops), single


def _stop_len(tokens, stops, eot_token, start=0):
    """the length of the answer `tokens` cut behind the first position i >= start at which it ends: tokens[i] is the eot_token, or
    tokens[:i + 1] ends with one of the stop sequences (a match may begin in front of `start`); None when it does not end"""
    for i in range(start, len(tokens)):
        if eot_token is not None and tokens[i] == eot_token:
            return i + 1
        for q in stops or ():
            if len(q) <= i + 1 and tuple(tokens[i + 1 - len(q):i + 1]) == tuple(q):
                return i + 1
    return None


def _adjust_per_request(n, V, repetition_penalty=None, repetition_context=None, logit_bias=None, allowed_tokens=None, banned_tokens=None,
                        no_repeat_ngram_size=None, bad_words_ids=None, min_new_tokens=None, stop_sequences=None, eot_token=None):
    """(adjusts, kws) of a batch call, the convention of _per_request: every keyword is one value shared by all n requests or a
    list / tuple of n per-request values.  A penalty, bias, no_repeat_ngram_size or min_new_tokens list is always per request; an id
    keyword (context, allowed, banned) is per request when it is a list / tuple whose entries are None or id collections themselves,
    else one shared collection of ids; a sequence keyword (bad_words_ids, stop_sequences) is per request when its entries are None or
    lists of sequences themselves, else one shared list of sequences.
    adjusts: None when no request adjusts, else n entries (None | _Adjust), ONE _Adjust (one dense row) per distinct request;
    kws[b]: the keywords of the single call of request b."""
    groups = (list, tuple, set, frozenset, range, torch.Tensor)

    def nested(t):  # a list of sequences, not a sequence of ids
        if isinstance(t, torch.Tensor):
            return t.dim() == 2
        return isinstance(t, (list, tuple)) and all(isinstance(q, (list, tuple, torch.Tensor)) for q in t)

    def spread(v, kind):
        per = isinstance(v, (list, tuple)) and (kind == 0 or (len(v) > 0 and all(
            t is None or (isinstance(t, groups) if kind == 1 else nested(t)) for t in v)))
        if per and len(v) != n:
            raise ValueError("repetition_penalty / repetition_context / logit_bias / allowed_tokens / banned_tokens / no_repeat_ngram_size / "
                             "bad_words_ids / min_new_tokens / stop_sequences lists need one entry per sequence")
        return list(v) if per else [v] * n

    cols = [spread(v, kind) for v, kind in ((repetition_penalty, 0), (repetition_context, 1), (logit_bias, 0), (allowed_tokens, 1),
                                            (banned_tokens, 1), (no_repeat_ngram_size, 0), (bad_words_ids, 2), (min_new_tokens, 0),
                                            (stop_sequences, 2))]
    made, adjusts, kws = {}, [], []
    for b in range(n):
        vals = [c[b] for c in cols]
        key = (None if vals[0] is None else float(vals[0]),) + tuple(v if isinstance(v, int) else id(v) for v in vals[1:])
        if key not in made:
            made[key] = _adjust_of(V, *vals, eot_token=eot_token)
        adjusts.append(made[key])
        kws.append({k: v for k, v in zip(_ADJUST_KEYS + _SEQ_KEYS, vals) if v is not None})
    return (None if all(a is None for a in adjusts) else adjusts), kws


def _hist_ld(adjusts, max_new_tokens):
    """columns of the device history a call needs: the longest context plus max_new_tokens; None when no request has a device rule"""
    ruled = [a for a in adjusts if a is not None and a.rules is not None and a.rules.device]
    return max(len(a.context) for a in ruled) + max(int(max_new_tokens), 1) if ruled else None


class _AdjustState:
    """device side of the adjustment of `rows` logits rows (one decode slot each): the bitmap of seen tokens [rows, ceil(V / 32)], the
    adjusted rows [rows, V] the picks read, and the bias rows, uploaded once per distinct request.  `hist_ld` (not None: some request
    has a sequence rule the device computes): also the token histories int32 [rows, hist_ld] with their lengths [rows], seeded with the
    context when a row is (re)filled, and the bad-word tables, uploaded once per distinct request; `eot`: the token the minimum-length
    rule holds back.  Nothing here outlives the call."""

    def __init__(self, V, rows, dev, hist_ld=None, eot=None):
        self.V, self.W, self.dev = V, (V + 31) // 32, dev
        self.seen = torch.zeros((rows, self.W), dtype=torch.int32, device=dev)
        self.ws = torch.empty((rows, V), dtype=torch.float32, device=dev)
        self.adj = [None] * rows  # the _Adjust of the request each row serves (None: unadjusted)
        self._bias = {}
        self.ruled = hist_ld is not None
        if self.ruled:
            self.hist_ld, self.eot = int(hist_ld), -1 if eot is None else int(eot)
            self.hist = torch.zeros((rows, self.hist_ld), dtype=torch.int32, device=dev)
            self.hist_len = torch.zeros((rows,), dtype=torch.int32, device=dev)
            self._bad = {}

    def bad(self, a):
        if a is None or a.rules is None or a.rules.table is None:
            return None
        if id(a) not in self._bad:
            self._bad[id(a)] = a.rules.table.to(self.dev).contiguous()
        return self._bad[id(a)]

    def rules_args(self, s=None):
        """(pointer to the showo_seq_rules of all rows, or of row s alone; what must stay alive over the call)"""
        import ctypes as C
        rows = list(range(len(self.adj))) if s is None else [s]
        rl = [None if self.adj[r] is None or self.adj[r].rules is None or not self.adj[r].rules.device else self.adj[r].rules for r in rows]
        n = len(rows)
        ngram = (C.c_int32 * n)(*[0 if q is None else q.ngram for q in rl])
        ctx = (C.c_int32 * n)(*[0 if q is None else len(self.adj[r].context) for r, q in zip(rows, rl)])  # (what seed() put there)
        mnew = (C.c_int32 * n)(*[0 if q is None else q.min_new for q in rl])
        bad = (C.c_void_p * n)(*[_lib.ptr(self.bad(self.adj[r])) for r in rows])
        r0 = rows[0]
        from ._lib import SeqRules
        st = SeqRules(_lib.ptr(self.hist[r0]), self.hist_ld, _lib.ptr(self.hist_len[r0:]), C.cast(ngram, C.c_void_p),
                           C.cast(ctx, C.c_void_p), C.cast(mnew, C.c_void_p), self.eot, C.cast(bad, C.c_void_p))
        return C.c_void_p(C.addressof(st)), (st, ngram, ctx, mnew, bad)

    def ban(self, s, mark=None):
        """the stand-alone ban on the adjusted row of slot s, in place; mark: None, or the one-element int64 device view of the token
        that joins row s's history in front of the rules"""
        if not self.ruled or self.adj[s] is None or self.adj[s].rules is None or not self.adj[s].rules.device:
            return
        args, keep = self.rules_args(s)
        _lib.call("showo_seq_ban", _lib.ptr(self.ws[s]), self.V, 1, self.V, args, _lib.ptr(mark), None, _lib.stream())
        del keep

    def bias(self, a):
        if a is None or a.bias is None:
            return None
        if id(a) not in self._bias:
            self._bias[id(a)] = a.bias.to(self.dev).contiguous()
        return self._bias[id(a)]

    def seed(self, s, a):
        """row s serves a new request: a cleared bitmap row, re-seeded with the request's context ids"""
        self.seen[s].zero_()
        self.adj[s] = a
        if a is not None and a.context:
            ids = torch.tensor(a.context, dtype=torch.int64, device=self.dev)
            _lib.call("showo_seen_mark", _lib.ptr(self.seen[s]), self.V, _lib.ptr(ids), len(a.context), _lib.stream())
        if self.ruled:  # the history starts as the context (only a request with a device rule reads it)
            c = len(a.context) if a is not None and a.rules is not None and a.rules.device else 0
            if c:
                self.hist[s, :c].copy_(torch.tensor(a.context, dtype=torch.int32))
            self.hist_len[s:s + 1].fill_(c)

    def mark(self, s, tok):
        """the one-element int64 device view `tok` joins row s's set"""
        _lib.call("showo_seen_mark", _lib.ptr(self.seen[s]), self.V, _lib.ptr(tok), 1, _lib.stream())

    def host_args(self):
        """(penalty, bias) host arrays with one entry per row, as the C entries take them (keep them alive over the call)"""
        import ctypes as C
        n = len(self.adj)
        pen = (C.c_float * n)(*[1.0 if a is None else a.theta for a in self.adj])
        rows = (C.c_void_p * n)(*[_lib.ptr(self.bias(a)) for a in self.adj])
        return pen, rows

    def adjust(self, s, logits):
        """the stand-alone launch on one row: logits fp32 [V] -> the adjusted row of slot s (a view of self.ws), nothing marked"""
        import ctypes as C
        pen, rows = self.host_args()
        _lib.call("showo_logits_adjust", _lib.ptr(logits), self.V, 1, self.V, _lib.ptr(self.seen[s]), self.W, None,
                  C.c_void_p(C.addressof(pen) + C.sizeof(C.c_float) * s), C.c_void_p(C.addressof(rows) + C.sizeof(C.c_void_p) * s), None,
                  _lib.ptr(self.ws[s]), self.V, _lib.stream())
        return self.ws[s]

    def loop_args(self):
        """the adjustment arguments of showo_engine_decode_sample_adj / _batch_decode_sample_adj, and what must stay alive over the call"""
        import ctypes as C
        pen, rows = self.host_args()
        args, keep = (_lib.ptr(self.seen), self.W, C.cast(pen, C.c_void_p), C.cast(rows, C.c_void_p), _lib.ptr(self.ws)), (pen, rows)
        if self.ruled:  # the _seq entries: the rules behind adj_ws
            q, keep_q = self.rules_args()
            args, keep = args + (q,), keep + keep_q
        return args, keep

    def entry(self, adj_name):
        """the loop entry: `adj_name` (an _adj entry), or its _seq form when some request has a device rule"""
        return adj_name[:-4] + "_seq" if self.ruled else adj_name


def _draw_seed(generator):
    """one Philox seed for the on-device draws, from `generator` (on its device) or from torch's global generator"""
    kw = {} if generator is None else {"generator": generator, "device": generator.device}
    return int(torch.randint(0, 2 ** 62, (1,), **kw).item())


def _draw_params(model, max_new_tokens, temperature, top_k, top_p, generator, noise):
    """(greedy, k, noise, seed, p) of one mmu_generate call: greedy for top_k == 1 (k 1, no noise, seed 0: what the arg-max entries and
    showo_engine_decode_sample_lp take), else k (0: no top-k filter), the fp32 `_exp_noise` [max_new_tokens, vocab] and ONE seed drawn
    from the generator; p: None or the nucleus top_p inside (0, 1).  Checks in this order: top_p, temperature, (seed draw), noise shape."""
    p = _nucleus_p(top_p)
    if top_k == 1:
        return True, 1, None, 0, p
    if not temperature > 0:
        raise ValueError("temperature must be > 0")
    seed = _draw_seed(generator)
    if noise is not None:
        noise = noise.detach().float().contiguous()
        if tuple(noise.shape) != (max_new_tokens, model.vocab_size):
            raise ValueError("_exp_noise must be [max_new_tokens, vocab_size]")
    return False, 0 if top_k is None else int(top_k), noise, seed, p


@contextlib.contextmanager
def _graph_stream_of(model):
    """the body runs on the model's side stream (hipGraph capture and replay need a non-default stream), behind the work queued on the
    current stream; the current stream then waits for it.  The stream is made on first use and kept on the model."""
    gs = getattr(model, "_graph_stream", None)
    if gs is None:
        gs = model._graph_stream = torch.cuda.Stream()
    cur = torch.cuda.current_stream()
    gs.wait_stream(cur)
    with torch.cuda.stream(gs):
        yield
    cur.wait_stream(gs)


def _prompt_args(model, eng, idx, input_embeddings, attention_mask):
    """(ids, emb, mask, L) of one batch-1 prompt as the prefill entries take it: int64 ids [1, L] or fp32 embeddings [1, L, H], and the
    dense mask as fp32 [1, 1, L, L].  An IntervalMask is registered with the engine instead (mask None) until _prefill resets it."""
    from .prompting_utils import IntervalMask
    ids = None if idx is None else idx.to(torch.int64).contiguous()
    emb = None if input_embeddings is None else input_embeddings.detach().float().contiguous()
    L = (ids if ids is not None else emb).shape[1]
    if isinstance(attention_mask, IntervalMask):
        mask = model._use_mask(eng, attention_mask)
    else:
        mask = None if attention_mask is None else attention_mask.detach().float().reshape(1, 1, L, L).contiguous()
    return ids, emb, mask, L


def _prefill(eng, ids, emb, mask, L, logits, slot=None):
    """the prompt into the engine's decode cache (showo_engine_prefill) or into `slot` of the running batch (showo_engine_batch_prefill),
    its last row's logits into `logits`; the engine forgets the registered IntervalMask whether or not the call succeeds.  Returns L."""
    entry, head = ("showo_engine_prefill", (eng,)) if slot is None else ("showo_engine_batch_prefill", (eng, slot))
    try:
        _lib.call(entry, *head, _lib.ptr(ids), _lib.ptr(emb), _lib.ptr(mask), L, _lib.ptr(logits), _lib.stream())
    finally:
        _lib.call("showo_engine_use_intervals", eng, None, None)
    return L


def _sample_call(logits, V, k, p, temperature, noise, seed, step, tok):
    """one draw from a logits row: showo_sample_topk, or showo_sample_topk_topp behind the nucleus filter p"""
    if p is None:
        _lib.call("showo_sample_topk", _lib.ptr(logits), V, k, float(temperature), _lib.ptr(noise), seed, step, _lib.ptr(tok), _lib.stream())
    else:
        _lib.call("showo_sample_topk_topp", _lib.ptr(logits), V, k, p, float(temperature), _lib.ptr(noise), seed, step, _lib.ptr(tok),
                  _lib.stream())


def _logprob_of(logits, V, tok):
    """fp32 [1]: the log-probability of token tok[0] under the logits row (showo_logprob_rows)"""
    lp = torch.empty((1,), dtype=torch.float32, device=logits.device)
    _lib.call("showo_logprob_rows", _lib.ptr(logits), V, 1, V, _lib.ptr(tok), _lib.ptr(lp), None, _lib.stream())
    return lp


_GREEDY_DRAW = (True, 1, None, 1.0, None, 0)  # a draw (greedy, k, p, temperature, noise, seed) that is the arg-max


def _first_token(logits, V, tok, draw, want_lp=False, pick=None):
    """launch the pick of a sequence's first token from its prefill logits into the one-element view `tok`: the arg-max, or draw 0 of
    `draw` (logits / temperature -> top-k filter -> softmax -> multinomial, reference :220-228, one kernel).  want_lp: also launch its
    log-probability and return it (fp32 [1]).  Nothing is read back: the caller decides when to synchronise.  `pick`: the adjusted
    row the pick reads instead (_AdjustState.adjust); the log-probability stays that of the raw `logits`."""
    greedy, k, p, temperature, noise, seed = draw
    row = logits if pick is None else pick
    if greedy:
        _lib.call("showo_argmax_f32", _lib.ptr(row), V, _lib.ptr(tok), _lib.stream())
    else:
        _sample_call(row, V, k, p, temperature, noise, seed, 0, tok)
    return _logprob_of(logits, V, tok) if want_lp else None


def _decode_batch1(model, eng, logits, tok, max_new_tokens, draw, eot_token, want_lp, adjust=None):
    """One sequence behind its prefill (`logits`: its last row's): the int tokens, cut behind <eot>; want_lp: (tokens, their
    log-probabilities fp32 [len(tokens)]).  logits / temperature does not change the arg-max for temperature > 0 and top_k=1 makes the
    reference's multinomial a deterministic arg-max.  The first token comes from the prefill logits; the continuation
    runs in chunks of `chunk` steps entirely on the device (embed -> 24 layers on the KV cache -> lm_head -> pick), one hipGraph
    replay per step, and the host looks at the tokens (for <eot>) once per chunk.
    `adjust` (an _Adjust): the first token is picked from the adjusted prefill logits (the stand-alone launch, the context ids marked)
    and every chunk runs on showo_engine_decode_sample_adj, whose steps mark the token they feed; None: the calls of a call without.
    With sequence rules the device computes (adjust.rules) the first token also takes the stand-alone ban on the history = context and
    the chunks run on showo_engine_decode_sample_seq; stop sequences cut the answer where the host looks at the tokens, as <eot> does."""
    greedy, k, p, temperature, noise, seed = draw
    st, pick, stops = None, None, None
    if adjust is not None:
        st = _AdjustState(model.vocab_size, 1, tok.device, _hist_ld([adjust], max_new_tokens), eot_token)
        st.seed(0, adjust)
        pick = st.adjust(0, logits)
        st.ban(0)  # (sequence rules: the history is the context, nothing marked)
        stops = adjust.rules.stops if adjust.rules is not None else None
    lps = [_first_token(logits, model.vocab_size, tok, draw, want_lp, pick)]

    def done(result):
        return (result, torch.cat(lps)[:len(result)]) if want_lp else result

    result = [int(tok.item())]
    if (eot_token is not None and result[0] == eot_token) or max_new_tokens <= 1 or (stops and _stop_len(result, stops, None) is not None):
        return done(result[:max_new_tokens])
    use_graph, chunk = int(getattr(model, "decode_graph", 1)), 16
    remaining = max_new_tokens - 1
    while remaining > 0:
        n, step0 = min(chunk, remaining), max_new_tokens - remaining
        outc = torch.empty((n,), dtype=torch.int64, device=tok.device)
        if want_lp:
            lps.append(torch.empty((n,), dtype=torch.float32, device=tok.device))
        head = (eng, _lib.ptr(tok), n, _lib.ptr(outc), _lib.ptr(logits))
        with _graph_stream_of(model):
            if st is not None:
                args, keep = st.loop_args()
                _lib.call(st.entry("showo_engine_decode_sample_adj"), *head, k, 1.0 if (greedy or p is None) else p,
                          1.0 if greedy else float(temperature), _lib.ptr(noise), seed, step0, _lib.ptr(lps[-1]) if want_lp else None, None,
                          *args, use_graph, _lib.stream())
                del keep
            elif want_lp:  # one entry: it takes the greedy step for top_k == 1 and the plain top-k draw for top_p >= 1
                _lib.call("showo_engine_decode_sample_lp", *head, k, 1.0 if (greedy or p is None) else p,
                          1.0 if greedy else float(temperature), _lib.ptr(noise), seed, step0, _lib.ptr(lps[-1]), None, use_graph, _lib.stream())
            elif greedy:
                _lib.call("showo_engine_decode_greedy", *head, use_graph, _lib.stream())
            elif p is None:
                _lib.call("showo_engine_decode_sample", *head, k, float(temperature), _lib.ptr(noise), seed, step0, use_graph, _lib.stream())
            else:
                _lib.call("showo_engine_decode_sample_p", *head, k, p, float(temperature), _lib.ptr(noise), seed, step0, use_graph,
                          _lib.stream())
        for t in outc.tolist():
            result.append(t)
            if (eot_token is not None and t == eot_token) or (stops and _stop_len(result, stops, None, len(result) - 1) is not None):
                return done(result)
        remaining -= n
    return done(result)


# ---- beam search ("Beam search") ----------------------------------------------------------------------------------------------
_BEAM_MAX = 8         # beams: the slots of a regular decode batch
_BEAM_STATE_HEAD = 64  # words of a state block in front of its length-penalty table (csrc/beam.h)
_BEAM_CHUNK = 16      # steps per showo_engine_batch_decode_beam call (`model.beam_chunk` overrides it)


def _beam_request(model, num_beams, length_penalty, early_stopping, num_return_sequences, return_beam_scores, max_new_tokens, temperature,
                  top_k, top_p, generator, noise, adjusted):
    """the beam keywords of mmu_generate / MmuSession.generate, checked before the engine is touched: None for `num_beams` None or 1
    (the call is the one without the keywords), else the number of beams 2..8.  ValueError: num_beams outside 1..8,
    num_return_sequences outside 1..num_beams, a non-finite length_penalty, an early_stopping that is not a bool ("never" is not
    served), return_beam_scores without beams; with beams: top_k other than None / 1, any top_p, temperature != 1, a generator or
    noise, a logit-adjustment keyword, max_new_tokens < 1, precision 1."""
    B = 1 if num_beams is None else num_beams
    if isinstance(B, bool) or not isinstance(B, int) or not 1 <= B <= _BEAM_MAX:
        raise ValueError(f"num_beams must be an int in 1..{_BEAM_MAX}")
    n = num_return_sequences
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= B:
        raise ValueError("num_return_sequences must be an int in 1..num_beams")
    if isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float)) or not math.isfinite(length_penalty):
        raise ValueError("length_penalty must be a finite number")
    if not isinstance(early_stopping, bool):
        raise ValueError('early_stopping must be a bool (early_stopping="never" is not served)')
    if B == 1:
        if return_beam_scores:
            raise ValueError("return_beam_scores needs num_beams >= 2")
        return None
    if top_k not in (None, 1):
        raise ValueError("beam search takes top_k None or 1 (beam sampling is not served)")
    if top_p is not None or temperature != 1 or generator is not None or noise is not None:
        raise ValueError("beam search takes no top_p, temperature != 1, generator or noise (beam sampling is not served)")
    if adjusted:
        raise ValueError("beam search takes no logit-adjustment keyword (logits processors with beams are not served)")
    if max_new_tokens < 1:
        raise ValueError("max_new_tokens must be >= 1")
    if int(getattr(model, "_precision", 0)) == 1:
        raise ValueError("beam search runs at precision 0, 2 or 3 (the batched decode step)")
    return B


def _beam_hypotheses(n_hyp, tr_parent, tr_token, tr_lp, hyp, eot_token):
    """the finished hypotheses of a search, best first, rebuilt on the host from the back-pointers: dicts with `tokens` (ints, the
    <eot> included), `final`, `sumlp`, `len` and `lps` (fp32 numpy, one per token).  tr_* [T, B] and hyp int32 [B, 8] as numpy."""
    import numpy as np
    out = []
    for rec in hyp[:n_hyp]:
        step, beam, kind, length = int(rec[0]), int(rec[1]), int(rec[2]), int(rec[4])
        f = rec.view(np.float32)
        toks, lps = [], []
        s, b = (step - 1, beam) if kind == 0 else (step, beam)
        while s >= 0:
            toks.append(int(tr_token[s, b]))
            lps.append(tr_lp[s, b])
            b = int(tr_parent[s, b])
            s -= 1
        toks.reverse()
        lps.reverse()
        if kind == 0:
            toks.append(int(eot_token))
            lps.append(f[7])
        assert len(toks) == length
        out.append({"tokens": toks, "final": float(f[3]), "sumlp": float(f[5]), "len": length, "lps": np.array(lps, dtype=np.float32),
                    "step": step, "beam": beam, "kind": kind})
    return out


def _beam_search(model, eng, logits, length, B, max_new_tokens, eot_token, length_penalty, early_stopping, dev, trace=None):
    """Beam search behind a prefill or append (`logits`: its last row's; `length`: rows in the engine's decode cache): a batch of B
    slots, each a fork of that cache, showo_engine_batch_beam_begin for the first step and showo_engine_batch_decode_beam in chunks;
    the host reads the done flag once per chunk and the tables once at the end.  The engine's own cache is left as it is.  Returns
    _beam_hypotheses' list (B entries).  `trace`: a dict that receives the raw device tables (tests)."""
    V, T = model.vocab_size, int(max_new_tokens)
    if not _batch_begin(eng, B, length + T + 1):
        raise RuntimeError("beam search: prompt + max_new_tokens does not fit the engine's decode batch (max_position_embeddings, "
                           "the single-block decode attention)")
    for b in range(B):
        _lib.call("showo_engine_batch_fork", eng, b, _lib.stream())
    state = torch.zeros((_BEAM_STATE_HEAD + T + 1,), dtype=torch.int32, device=dev)
    tr_parent, tr_token = (torch.zeros((T, B), dtype=torch.int32, device=dev) for _ in range(2))
    tr_cum, tr_lp = (torch.zeros((T, B), dtype=torch.float32, device=dev) for _ in range(2))
    hyp = torch.zeros((B, 8), dtype=torch.int32, device=dev)
    ws = torch.empty((B, V), dtype=torch.float32, device=dev)
    eot = -1 if eot_token is None else int(eot_token)
    tail = (_lib.ptr(tr_parent), _lib.ptr(tr_token), _lib.ptr(tr_cum), _lib.ptr(tr_lp), _lib.ptr(hyp))
    _lib.call("showo_engine_batch_beam_begin", eng, _lib.ptr(state), T, _lib.ptr(logits), eot, length_penalty, int(early_stopping), *tail,
              _lib.stream())
    use_graph, chunk = int(getattr(model, "decode_graph", 1)), int(getattr(model, "beam_chunk", _BEAM_CHUNK))
    while True:
        t, done = state[:2].tolist()
        if done or t >= T:
            break
        with _graph_stream_of(model):
            _lib.call("showo_engine_batch_decode_beam", eng, _lib.ptr(state), min(chunk, T - t), eot, length_penalty, int(early_stopping),
                      _lib.ptr(ws), *tail, use_graph, _lib.stream())
    head = state[:_BEAM_STATE_HEAD].cpu().numpy()
    tables = [x.cpu().numpy() for x in (tr_parent, tr_token, tr_cum, tr_lp, hyp)]
    if trace is not None:
        trace.update(state=head, parent=tables[0], token=tables[1], cum=tables[2], lp=tables[3], hyp=tables[4])
    return _beam_hypotheses(int(head[2]), tables[0], tables[1], tables[3], tables[4], eot_token)


def _beam_result(hyps, num_return_sequences, return_logprobs, return_beam_scores, dev):
    """what a beam call returns: the best hypothesis' token list (num_return_sequences > 1: a list of them, best first), then, if
    asked for, the per-token log-probabilities (fp32 tensors, likewise) and the final scores (fp32 [num_return_sequences])"""
    hyps = hyps[:num_return_sequences]
    toks = [[torch.tensor(t, device=dev) for t in h["tokens"]] for h in hyps]
    lps = [torch.from_numpy(h["lps"]).to(dev) for h in hyps]
    one = num_return_sequences == 1
    out = [toks[0] if one else toks]
    if return_logprobs:
        out.append(lps[0] if one else lps)
    if return_beam_scores:
        out.append(torch.tensor([h["final"] for h in hyps], dtype=torch.float32, device=dev))
    return out[0] if len(out) == 1 else tuple(out)


# Slot scheduler of mmu_generate_batch (n >= 2 sequences at precision 0 / 2 beyond the all-greedy 2..8 case).  Slot count for more
# than _MMU_BATCH_MAX sequences: 5..8 slots run the plain three-launch batched layer, 2..4 the co-scheduled one (decode_batch.hip).
# tools/mmu_batch_bench.py at the cfg4 shape: 8 slots lead 4 by 2.5-3.4 % on top-k sampled batches of 16 / 32 and trail by 1.3-1.5 % on
# greedy ones ("Sampled batches and slot refill").
_MMU_BATCH_MAX = 8
_MMU_BATCH_SLOTS = 8
_MMU_BATCH_CHUNK = 16


def _mmu_batch_slots(n):
    return n if n <= _MMU_BATCH_MAX else _MMU_BATCH_SLOTS


# Wide decode batches (opt-in, `slots=S`): 9..32 slots of showo_engine_batch_begin_wide (csrc/decode_wide.hip, precision 0)
_MMU_WIDE_MIN, _MMU_WIDE_MAX = 9, 32


def _mmu_wide_slots(slots, n, precision):
    """the `slots` argument of mmu_generate_batch / MmuSession.generate_batch: None (the call without it: slots is None, or n <= 8
    requests) or the slot count min(slots, n) of a wide batch; ValueError for anything but None or an int in 9..32, and for a
    precision other than 0"""
    if slots is None:
        return None
    if isinstance(slots, bool) or not isinstance(slots, int) or not _MMU_WIDE_MIN <= slots <= _MMU_WIDE_MAX:
        raise ValueError(f"slots must be None or an int in {_MMU_WIDE_MIN}..{_MMU_WIDE_MAX} (a wide decode batch)")
    if int(precision) != 0:
        raise ValueError("slots (a wide decode batch) needs precision 0 (bf16 operands)")
    return None if n <= _MMU_BATCH_MAX else min(slots, n)


def _mmu_batch_seeds(top_ks, generator):
    """the Philox seed of every sampled sequence, drawn as n sequential mmu_generate calls draw them: one draw per sequence with
    top_k != 1, in sequence order, none for greedy ones (None)"""
    seeds = []
    for k in top_ks:
        seeds.append(None if k == 1 else _draw_seed(generator))
    return seeds


def _mmu_batch_schedule(eng, n, slots, max_new_tokens, eot_token, chunk=_MMU_BATCH_CHUNK, stops=None):
    """Serve requests 0..n-1 on `slots` decode slots; returns their token lists in input order.

    `eng` is the engine side: `prefill(slot, r)` puts request r into a free slot and returns its first token (drawn from the prefill
    logits); `decode(m, budget, draw0)` runs m steps of every slot -- slot s emits at most budget[s] tokens (0: idle) with draw indices
    draw0[s], draw0[s] + 1, ..., stopping early after <eot> -- and returns (rows, produced): the tokens of each slot and how many it
    emitted.  Free slots are refilled in slot order with the pending requests in input order, at chunk boundaries.
    `stops`: None, or per request None | its stop sequences (lists of ids): the answer ends behind the first position at which it ends
    with one of them -- the match may straddle chunks; the slot is retired at the chunk boundary, the tokens behind the match dropped."""
    results = [None] * n

    def stopped(r, start):
        """cut request r's answer behind the first stop match that ends at or behind position `start`; True when there was one"""
        cut = None if stops is None or not stops[r] else _stop_len(results[r], stops[r], None, start)
        if cut is not None:
            del results[r][cut:]
        return cut is not None

    pending = list(range(n))[::-1]
    occupant = [None] * slots
    remaining = [0] * slots
    while True:
        for s in range(slots):
            while occupant[s] is None and pending:
                r = pending.pop()
                first = eng.prefill(s, r)
                results[r] = [first][:max_new_tokens]
                if not ((eot_token is not None and first == eot_token) or max_new_tokens <= 1 or stopped(r, 0)):
                    occupant[s], remaining[s] = r, max_new_tokens - 1
        live = [s for s in range(slots) if occupant[s] is not None]
        if not live:
            return results
        m = min(chunk, max(remaining[s] for s in live))
        budget = [min(remaining[s], m) if occupant[s] is not None else 0 for s in range(slots)]
        draw0 = [max_new_tokens - remaining[s] if occupant[s] is not None else 0 for s in range(slots)]
        rows, produced = eng.decode(m, budget, draw0)
        for s in live:
            toks = list(rows[s][:produced[s]])
            had = len(results[occupant[s]])
            results[occupant[s]].extend(toks)
            remaining[s] -= produced[s]
            if stopped(occupant[s], had) or remaining[s] <= 0 or (eot_token is not None and toks and toks[-1] == eot_token):
                occupant[s] = None


class _MmuSlotEngine:
    """engine side of _mmu_batch_schedule: `slots` KV caches of showo_engine_batch_*, one request per slot"""

    def __init__(self, model, eng, idx, input_embeddings, masks, lens, slots, temps, top_ks, seeds, noises, eot_token, dev, top_ps=None,
                 want_lp=False, adjusts=None, max_new_tokens=0):
        self.model, self.eng, self.idx, self.emb, self.masks, self.lens = model, eng, idx, input_embeddings, masks, lens
        # adjusts: None, or per request None | _Adjust -- every decode call then goes through showo_engine_batch_decode_sample_adj (an
        # unadjusted request's slot runs with penalty 1 and no bias row: a bit copy of its logits); a slot's bitmap row is cleared and
        # re-seeded with its request's context whenever the scheduler refills it
        # sequence rules travel in the _Adjust: with a device rule in the batch every decode call is the _seq entry (one ban launch
        # behind the adjust launch; a slot's history is re-seeded with its request's context); stop sequences are the scheduler's
        self.adjusts = adjusts
        self.adj = None if adjusts is None else _AdjustState(model.vocab_size, slots, dev, _hist_ld(adjusts, max_new_tokens), eot_token)
        self.stops = None
        if adjusts is not None and any(a is not None and a.rules is not None and a.rules.stops for a in adjusts):
            self.stops = [a.rules.stops if a is not None and a.rules is not None else None for a in adjusts]
        # want_lp: every decode call goes through showo_engine_batch_decode_sample_lp; lps[r] collects request r's log-probabilities
        self.lps = {} if want_lp else None
        self.slots, self.temps, self.top_ks, self.seeds, self.noises = slots, temps, top_ks, seeds, noises
        self.top_ps = [None] * len(top_ks) if top_ps is None else top_ps  # per request: None or the nucleus p inside (0, 1)
        self.eot = -1 if eot_token is None else int(eot_token)
        self.dev = dev
        V = model.vocab_size
        self.logits = torch.empty((slots, V), dtype=torch.float32, device=dev)
        self.tok = torch.empty((slots,), dtype=torch.int64, device=dev)
        self.occ = [None] * slots
        self.use_graph = int(getattr(model, "decode_graph", 1))

    def prefill(self, s, r):
        self.fill(s, r)
        return self.first(s, r)

    def fill(self, s, r):
        """request r into slot s: its K / V^T in the slot's cache, its last row's logits in self.logits[s]"""
        ids, emb = (self.idx[r], None) if self.idx is not None else (None, self.emb[r])
        _prefill(self.eng, *_prompt_args(self.model, self.eng, ids, emb, self.masks[r]), self.logits[s], slot=s)

    def first(self, s, r):
        """request r's first token, drawn from self.logits[s]"""
        k = self.top_ks[r]
        draw = (k == 1, 0 if k is None else int(k), self.top_ps[r], self.temps[r], self.noises[r], self.seeds[r])
        pick = None
        if self.adj is not None:
            self.adj.seed(s, self.adjusts[r])
            if self.adjusts[r] is not None:
                pick = self.adj.adjust(s, self.logits[s])
                self.adj.ban(s)
        lp = _first_token(self.logits[s], self.model.vocab_size, self.tok[s:s + 1], draw, self.lps is not None, pick)
        self.occ[s] = r
        if self.lps is not None:
            self.lps[r] = [lp]
        return int(self.tok[s].item())

    def logprobs(self, r, n):
        """request r's log-probabilities, cut to its n tokens"""
        return torch.cat(self.lps[r])[:n]

    def decode(self, m, budget, draw0):
        import ctypes as C
        S = self.slots
        for s in range(S):
            # a slot no request ever took (first tokens that were <eot> ended their sequences before they needed one) still has to hold
            # a prefill for the batched step: it idles on a copy of request 0
            if self.occ[s] is None and (self.lps is not None or self.adj is not None):
                self.fill(s, 0)
                self.occ[s] = 0
        occ = [r if budget[s] > 0 else None for s, r in enumerate(self.occ)]
        k = [1 if r is None else (0 if self.top_ks[r] is None else int(self.top_ks[r])) for r in occ]
        temp = [1.0 if r is None else float(self.temps[r]) for r in occ]
        seed = [0 if r is None or self.seeds[r] is None else self.seeds[r] for r in occ]
        noise = [None if r is None or self.noises[r] is None else _lib.ptr(self.noises[r]) for r in occ]
        a_k, a_t, a_s = (C.c_int * S)(*k), (C.c_float * S)(*temp), (C.c_uint64 * S)(*seed)
        a_d, a_n, a_b, prod = (C.c_int * S)(*draw0), (C.c_void_p * S)(*noise), (C.c_int * S)(*budget), (C.c_int * S)()
        top_p = [1.0 if r is None or self.top_ps[r] is None or self.top_ks[r] == 1 else self.top_ps[r] for r in occ]
        nucleus = any(q < 1.0 for q in top_p)  # no slot filters: the call of a batch without nucleus sampling
        a_p = (C.c_float * S)(*top_p)
        out = torch.empty((S, m), dtype=torch.int64, device=self.dev)
        lp = None if self.lps is None else torch.empty((S, m), dtype=torch.float32, device=self.dev)
        with _graph_stream_of(self.model):
            if self.adj is not None:
                args, keep = self.adj.loop_args()
                _lib.call(self.adj.entry("showo_engine_batch_decode_sample_adj"), self.eng, _lib.ptr(self.tok), m, _lib.ptr(out), _lib.ptr(self.logits),
                          *(C.cast(a, C.c_void_p) for a in (a_k, a_p, a_t, a_s, a_d, a_n, a_b)), self.eot, C.cast(prod, C.c_void_p),
                          _lib.ptr(lp), None, *args, self.use_graph, _lib.stream())
                del keep
            elif lp is not None:
                _lib.call("showo_engine_batch_decode_sample_lp", self.eng, _lib.ptr(self.tok), m, _lib.ptr(out), _lib.ptr(self.logits),
                          *(C.cast(a, C.c_void_p) for a in (a_k, a_p, a_t, a_s, a_d, a_n, a_b)), self.eot, C.cast(prod, C.c_void_p),
                          _lib.ptr(lp), None, self.use_graph, _lib.stream())
            else:
                _lib.call("showo_engine_batch_decode_sample_p" if nucleus else "showo_engine_batch_decode_sample", self.eng,
                          _lib.ptr(self.tok), m, _lib.ptr(out), _lib.ptr(self.logits),
                          *(C.cast(a, C.c_void_p) for a in ((a_k, a_p, a_t, a_s, a_d, a_n, a_b) if nucleus else (a_k, a_t, a_s, a_d, a_n, a_b))),
                          self.eot, C.cast(prod, C.c_void_p), self.use_graph, _lib.stream())
        if lp is not None:
            for s, r in enumerate(occ):
                if r is not None:
                    self.lps[r].append(lp[s, :prod[s]])
        return out.tolist(), list(prod)


def _per_request(n, temperature, top_k, top_p, exp_noise, attention_mask=None):
    """(temps, top_ks, top_ps, noises, masks) of a batch call: every scalar-or-list argument as a list with one entry per request (a
    scalar serves all n, `_exp_noise` None is no table for anyone), top_ps through _nucleus_p; ValueError for a list of another length"""
    def spread(v):
        return list(v) if isinstance(v, (list, tuple)) else [v] * n

    temps, top_ks, top_ps, masks = spread(temperature), spread(top_k), spread(top_p), spread(attention_mask)
    noises = list(exp_noise) if exp_noise is not None else [None] * n
    if not (len(masks) == len(temps) == len(top_ks) == len(noises) == len(top_ps) == n):
        raise ValueError("attention_mask / temperature / top_k / top_p / _exp_noise lists need one entry per sequence")
    return temps, top_ks, [_nucleus_p(q) for q in top_ps], noises, masks


def _check_request(model, max_new_tokens, temperature, top_k, noise):
    """the checks mmu_generate makes on one sampled request's temperature and `_exp_noise`, made before a batch starts"""
    if top_k != 1 and not temperature > 0:
        raise ValueError("temperature must be > 0")
    if top_k != 1 and noise is not None and tuple(noise.shape) != (max_new_tokens, model.vocab_size):
        raise ValueError("_exp_noise must be [max_new_tokens, vocab_size]")


def _batch_noises(top_ks, noises, dev):
    """the `_exp_noise` tables of the sampled requests as contiguous fp32 tensors on the device (None: greedy, or no table)"""
    return [None if (k == 1 or z is None) else z.detach().float().contiguous().to(dev) for k, z in zip(top_ks, noises)]


def _singles(single, n, return_logprobs):
    """the sequential form of a batch call: single(0), ..., single(n - 1) in order; return_logprobs: (token lists, log-probabilities)"""
    outs = [single(b) for b in range(n)]
    return ([o[0] for o in outs], [o[1] for o in outs]) if return_logprobs else outs


def _batch_begin(eng, slots, capacity, wide=False, shared=False):
    """open a decode batch of `slots` KV caches of `capacity` rows (showo_engine_batch_begin / _begin_wide; `shared`: _begin_shared,
    whose slots are suffix caches over the engine's decode cache and whose capacity counts suffix rows).  False: the batch's common
    capacity (longest prompt + max_new_tokens) does not fit the engine (max_position_embeddings, the single-block decode attention) --
    the caller then makes n sequential calls, which fail only if a sequence actually reaches the limit before <eot>"""
    try:
        _lib.call("showo_engine_batch_begin_shared" if shared else "showo_engine_batch_begin_wide" if wide else "showo_engine_batch_begin",
                  eng, slots, capacity)
    except RuntimeError:
        return False
    return True


def _run_on_slots(eng, n, wide, capacity, slot_engine, max_new_tokens, eot_token, want_lp, shared=False):
    """n requests on the slots of a decode batch (`wide`: the slot count of a wide one, else up to 8; `shared`: a wide one of suffix
    caches, `capacity` in suffix rows): begin, `slot_engine(slots)` as the engine side of _mmu_batch_schedule, the schedule.  The int
    token lists in request order, want_lp: (token lists, log-probability tensors); None when the batch does not fit the engine (nothing
    but the begin has happened then)."""
    slots = wide if wide else _mmu_batch_slots(n)
    if not _batch_begin(eng, slots, capacity, bool(wide), bool(wide) and shared):
        return None
    se = slot_engine(slots)
    stops = getattr(se, "stops", None)
    out = _mmu_batch_schedule(se, n, slots, max_new_tokens, eot_token, **({} if stops is None else {"stops": stops}))
    return (out, [se.logprobs(b, len(out[b])) for b in range(n)]) if want_lp else out


@torch.no_grad()
def mmu_generate_batch(self, idx=None, input_embeddings=None, attention_mask=None, max_new_tokens=100, temperature=1.0, top_k=None,
                       eot_token=None, generator=None, _exp_noise=None, top_p=None, return_logprobs=False, slots=None,
                       repetition_penalty=None, repetition_context=None, logit_bias=None, allowed_tokens=None, banned_tokens=None,
                       no_repeat_ngram_size=None, bad_words_ids=None, min_new_tokens=None, stop_sequences=None):
    """n independent `mmu_generate` calls served together (BASELINE cfg4: "batch=4 images"; the reference's mmu_generate is batch-1 and
    inference_mmu.py:87-177 walks the images one by one).  `idx` / `input_embeddings` / `attention_mask` are LISTS (one entry per
    sequence, each what a single `mmu_generate` call takes: [1, L_b] ids or [1, L_b, H] embeddings, its own mask or IntervalMask);
    `temperature` / `top_k` / `top_p` are scalars or lists of n values, `_exp_noise` None or a list of n entries (None or
    [max_new_tokens, vocab]).

    Returns a list of n token lists: result[b] is what `mmu_generate(<sequence b>, attention_mask=masks[b], max_new_tokens,
    temperature[b], top_k[b], eot_token, generator=generator, _exp_noise=_exp_noise[b], top_p=top_p[b])` returns when those calls are made in order
    b = 0, 1, ..., n-1 (the same seeds are drawn from `generator`, or torch's global generator, in the same order).  At precision 0, 2 and 3
    every n >= 2 runs on the batched engine path (csrc/decode_batch.hip: one weight stream per token step for all slots, every sequence
    bit-identical to its batch-1 run): all-greedy batches of 2..8 on showo_engine_batch_decode_greedy, anything else on up to 8 slots
    of showo_engine_batch_decode_sample that are refilled as sequences finish.  Precision 1 and n < 2 make the sequential calls.
    `return_logprobs=True` returns `(tokens, logprobs)`, logprobs a list of n fp32 device tensors (result[b]'s log-probabilities, the
    bits of the batch-1 call's); every batch, the all-greedy one included, then runs on the slots of showo_engine_batch_decode_sample_lp.

    `slots=S` (an int in 9..32, precision 0 only; anything else but None: ValueError) opts in to a WIDE decode batch for n > 8 requests:
    the same slot scheduler on min(S, n) slots of showo_engine_batch_begin_wide, whose steps run MFMA skinny GEMMs (csrc/decode_wide.hip:
    16 slots per instruction instead of one dot2 chain per slot).  Contract of a wide call: results are deterministic run to run; a
    request's tokens and log-probabilities do not depend on S, on n, on the slot it lands in or on what the other slots hold (an MFMA
    output column reads only its own sequence, the K order is fixed); they are NOT promised to equal the batch-1 bits -- same bf16
    rounding points, another fp32 summation order, so a near-tie may resolve differently.  With n <= 8 the call is the one without `slots`.

    `repetition_penalty` / `repetition_context` / `logit_bias` / `allowed_tokens` / `banned_tokens` (`mmu_generate` states them): each is
    one value shared by all n requests or a list of n per-request values (an id keyword is per request when its entries are None or id
    collections themselves); one dense bias row is built per distinct request.  Any adjusted request puts the whole batch on the slots
    of showo_engine_batch_decode_sample_adj (one adjust launch per step for all slots; an unadjusted request's slot gets a bit copy of
    its logits, so its tokens are those of a batch without); every slot keeps its own set, cleared and re-seeded when it is refilled.
    All None, or penalty 1 without a bias: exactly the calls of a batch without the keywords.

    `no_repeat_ngram_size` / `bad_words_ids` / `min_new_tokens` / `stop_sequences` (`mmu_generate` states them): one value shared by all n
    requests or a list of n per-request values (a sequence keyword is per request when its entries are None or lists of sequences
    themselves).  Any request with one of them puts the whole batch on the slot scheduler, as an adjustment does; with a rule the
    device computes the slots run on showo_engine_batch_decode_sample_seq (one ban launch per step behind the adjust launch; every slot
    keeps its own token history, re-seeded with the context when it is refilled); a request without rules gets the tokens of a batch
    without the keywords.  A stop sequence retires its slot at the next chunk boundary.  All None: exactly the calls of today."""
    seqs = idx if idx is not None else input_embeddings
    n = len(seqs)
    wide = _mmu_wide_slots(slots, n, getattr(self, "_precision", 0))
    temps, top_ks, top_ps, noises, masks = _per_request(n, temperature, top_k, top_p, _exp_noise, attention_mask)
    adjusts, adj_kws = None, [{}] * n
    if any(v is not None for v in (repetition_penalty, repetition_context, logit_bias, allowed_tokens, banned_tokens, no_repeat_ngram_size,
                                   bad_words_ids, min_new_tokens, stop_sequences)):
        adjusts, adj_kws = _adjust_per_request(n, self.vocab_size, repetition_penalty, repetition_context, logit_bias, allowed_tokens,
                                               banned_tokens, no_repeat_ngram_size, bad_words_ids, min_new_tokens, stop_sequences, eot_token)

    def single(b):
        return self.mmu_generate(idx=None if idx is None else idx[b], input_embeddings=None if input_embeddings is None else input_embeddings[b],
                                 attention_mask=masks[b], max_new_tokens=max_new_tokens, temperature=temps[b], top_k=top_ks[b],
                                 eot_token=eot_token, generator=generator, _exp_noise=noises[b], top_p=top_ps[b],
                                 **({"return_logprobs": True} if return_logprobs else {}), **adj_kws[b])

    if int(getattr(self, "_precision", 0)) == 1 or n < 2:
        return _singles(single, n, return_logprobs)
    if n <= _MMU_BATCH_MAX and all(k == 1 for k in top_ks) and not return_logprobs and adjusts is None:
        return self._mmu_generate_batch_greedy(idx, input_embeddings, masks, max_new_tokens, eot_token, single)
    for b in range(n):
        if seqs[b].shape[0] != 1:
            raise ValueError("every sequence of mmu_generate_batch is one batch-1 mmu_generate call (reference modeling_showo.py:204,229)")
        _check_request(self, max_new_tokens, temps[b], top_ks[b], noises[b])
    eng = self.engine()
    dev = seqs[0].device
    lens = [int(t.shape[1]) for t in seqs]

    def slot_engine(slots):  # (the seeds are drawn behind a begin that succeeded: the sequential calls draw their own)
        return _MmuSlotEngine(self, eng, idx, input_embeddings, masks, lens, slots, temps, top_ks, _mmu_batch_seeds(top_ks, generator),
                              _batch_noises(top_ks, noises, dev), eot_token, dev, top_ps, want_lp=return_logprobs,
                              **({} if adjusts is None else {"adjusts": adjusts, "max_new_tokens": max_new_tokens}))

    out = _run_on_slots(eng, n, wide, max(lens) + max_new_tokens + 1, slot_engine, max_new_tokens, eot_token, return_logprobs)
    if out is None:
        return _singles(single, n, return_logprobs)
    out, lps = out if return_logprobs else (out, None)
    toks = [[torch.tensor(t, device=dev) for t in r] for r in out]
    return (toks, lps) if return_logprobs else toks


Showo.mmu_generate_batch = mmu_generate_batch


@torch.no_grad()
def _mmu_generate_batch_greedy(self, idx, input_embeddings, masks, max_new_tokens, eot_token, single):
    """all-greedy batch of 2..8 sequences: one slot per sequence on showo_engine_batch_decode_greedy (the cfg4 bench leg)"""
    seqs = idx if idx is not None else input_embeddings
    n = len(seqs)
    eng = self.engine()
    dev = seqs[0].device
    if not _batch_begin(eng, n, max(int(t.shape[1]) for t in seqs) + max_new_tokens + 1):
        return [single(b) for b in range(n)]
    logits = torch.empty((n, self.vocab_size), dtype=torch.float32, device=dev)
    tok = torch.empty((n,), dtype=torch.int64, device=dev)
    for b in range(n):
        if seqs[b].shape[0] != 1:
            raise ValueError("every sequence of mmu_generate_batch is one batch-1 mmu_generate call (reference modeling_showo.py:204,229)")
        ids, emb = (idx[b], None) if idx is not None else (None, input_embeddings[b])
        _prefill(eng, *_prompt_args(self, eng, ids, emb, masks[b]), logits[b], slot=b)
        _first_token(logits[b], self.vocab_size, tok[b:b + 1], _GREEDY_DRAW)
    first = tok.tolist()  # one read for all n first tokens
    results = [[torch.tensor(t, device=dev)] for t in first]
    done = [(eot_token is not None and t == eot_token) or max_new_tokens <= 1 for t in first]
    use_graph, chunk = int(getattr(self, "decode_graph", 1)), 16
    remaining = max_new_tokens - 1
    while remaining > 0 and not all(done):
        m = min(chunk, remaining)
        outc = torch.empty((n, m), dtype=torch.int64, device=dev)
        with _graph_stream_of(self):
            _lib.call("showo_engine_batch_decode_greedy", eng, _lib.ptr(tok), m, _lib.ptr(outc), _lib.ptr(logits), use_graph, _lib.stream())
        rows = outc.tolist()
        for b in range(n):
            for t in rows[b]:
                if done[b]:
                    break
                results[b].append(torch.tensor(t, device=dev))
                if (eot_token is not None and t == eot_token) or len(results[b]) >= max_new_tokens:
                    done[b] = True
        remaining -= m
    return [r[:max_new_tokens] for r in results]


Showo._mmu_generate_batch_greedy = _mmu_generate_batch_greedy


# ---- mmu sessions: one prefill of the question-invariant prefix, questions appended to its KV cache ("mmu sessions") -------
def _shared_suffix_capacity(length, lens, max_new_tokens):
    """rows a slot of a shared-prefix batch needs behind the prefix [0, length): the dead rows below the prefix's last 64-row tile
    boundary, the longest request, the new tokens and the row an idle slot keeps rewriting"""
    return (length - (length & ~63)) + max(lens) + max_new_tokens + 1


class _SessionSlotEngine(_MmuSlotEngine):
    """engine side of _mmu_batch_schedule for MmuSession.generate_batch: a slot is filled by a fork of the session's cache plus an
    append of the request's rows instead of a prefill of a whole prompt; `share_prefix`: by showo_engine_batch_attach_append -- the
    rows are appended to the session's own cache, copied into the slot's suffix cache, and the session's cache is rewound"""

    def __init__(self, model, eng, rows, lens, slots, temps, top_ks, seeds, noises, eot_token, dev, top_ps=None, want_lp=False,
                 share_prefix=False, adjusts=None, max_new_tokens=0):
        super().__init__(model, eng, None, None, None, lens, slots, temps, top_ks, seeds, noises, eot_token, dev, top_ps, want_lp, adjusts,
                         max_new_tokens)
        self.rows = rows
        self.share_prefix = share_prefix

    def fill(self, s, r):
        ids, emb = self.rows[r]
        if self.share_prefix:
            _lib.call("showo_engine_batch_attach_append", self.eng, s, _lib.ptr(ids), _lib.ptr(emb), self.lens[r], _lib.ptr(self.logits[s]),
                      _lib.stream())
            return
        _lib.call("showo_engine_batch_fork", self.eng, s, _lib.stream())
        _lib.call("showo_engine_batch_prefill_append", self.eng, s, _lib.ptr(ids), _lib.ptr(emb), self.lens[r], _lib.ptr(self.logits[s]),
                  _lib.stream())


class _SessionEngine:
    """engine side of MmuSession: the model's decode cache behind showo_engine_prefill / _prefill_append / _cache_rewind / _batch_fork
    and the device loops of mmu_generate / mmu_generate_batch.  (Tests drive MmuSession with a stand-in of this class.)"""

    def __init__(self, model):
        self.model = model
        self.eng = model.engine()
        # the batched decode serves precision 0, 2 and 3 (showo_engine_batch_fork refuses 1): a precision-1 session answers
        # generate_batch with the sequential calls, as mmu_generate_batch does
        self.batched = int(getattr(model, "_precision", 0)) != 1
        self.dev = model.showo.lm_head.weight.device
        self.logits = torch.empty((model.vocab_size,), dtype=torch.float32, device=self.dev)
        self.logits0 = None
        self.tok = torch.empty((1,), dtype=torch.int64, device=self.dev)

    def state(self):
        """(cache length, prompt length, capacity, epoch) of the engine's decode cache"""
        import ctypes as C
        n, p, cap, ep = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
        _lib.call("showo_engine_cache_state", self.eng, C.byref(n), C.byref(p), C.byref(cap), C.byref(ep))
        return n.value, p.value, cap.value, ep.value

    def stamp(self):
        """what must not change under a live session: the engine, its weights and precision, and the prompt in its decode cache.
        None once the model dropped the engine this session was opened on (configure_workspace): `self.eng` is then a destroyed
        handle and nothing may be asked of it, so the handle OBJECT is compared first (a later engine may reuse the address)."""
        m = self.model
        if m._engine is not self.eng:
            return None
        m.engine()
        return (self.state()[3], int(getattr(m, "_precision", 0)), dict(m._engine_versions))

    def cached_rows(self):
        """rows the engine itself counts in its decode cache (MmuSession holds its own `length` against it)"""
        return self.state()[0]

    def prefill(self, idx, input_embeddings, attention_mask):
        L = _prefill(self.eng, *_prompt_args(self.model, self.eng, idx, input_embeddings, attention_mask), self.logits)
        self.logits0 = self.logits.clone()
        return L

    def embed(self, token):
        return self.model.showo.model.embed_tokens.weight.detach()[int(token)].float().reshape(1, 1, -1)

    def use_prefix_logits(self):
        self.logits.copy_(self.logits0)

    def append(self, ids, emb, Ln):
        _lib.call("showo_engine_prefill_append", self.eng, _lib.ptr(ids), _lib.ptr(emb), Ln, _lib.ptr(self.logits), _lib.stream())

    def rewind(self, length):
        _lib.call("showo_engine_cache_rewind", self.eng, int(length), _lib.stream())

    def settle(self, length, toks):
        """after run(): the cache keeps the rows below `length` and the fed tokens toks[:-1] (a chunk of the device loop may have run
        past an <eot>)"""
        self.rewind(length + len(toks) - 1)

    def run(self, max_new_tokens, greedy, k, temperature, noise, seed, eot_token, top_p=None, return_logprobs=False, adjust=None):
        """Showo.mmu_generate behind its prefill: the first token from the current logits, the rest from the device loop in chunks;
        return_logprobs: (tokens, their log-probabilities fp32 [len(tokens)]); adjust: the call's _Adjust"""
        return _decode_batch1(self.model, self.eng, self.logits, self.tok, max_new_tokens, (greedy, k, top_p, temperature, noise, seed),
                              eot_token, return_logprobs, adjust)

    def run_beam(self, length, B, max_new_tokens, eot_token, length_penalty, early_stopping):
        """beam search behind the current logits on B forks of the cache [0, length): _beam_search's hypotheses, best first.  The
        session's own cache is only read."""
        return _beam_search(self.model, self.eng, self.logits, length, B, max_new_tokens, eot_token, length_penalty, early_stopping, self.dev)

    def score(self, ids, Ln, use_prefix_logits):
        """log-probabilities / ranks [Ln] of the rows ids [1, Ln] appended to the cache (showo_engine_prefill_append_score): row j from
        the logits of row j - 1, row 0 from the prefill's logits (use_prefix_logits) or NaN / -1.  The rows stay in the cache: the
        caller rewinds."""
        lp = torch.empty((Ln,), dtype=torch.float32, device=self.dev)
        rk = torch.empty((Ln,), dtype=torch.int32, device=self.dev)
        last = torch.empty_like(self.logits)  # (self.logits keeps what the last append / decode step left)
        _lib.call("showo_engine_prefill_append_score", self.eng, _lib.ptr(ids), Ln, _lib.ptr(self.logits0) if use_prefix_logits else None,
                  _lib.ptr(lp), _lib.ptr(rk), _lib.ptr(last), _lib.stream())
        return lp, rk

    def run_batch(self, length, rows, lens, max_new_tokens, temps, top_ks, seeds, noises, eot_token, top_ps=None, return_logprobs=False,
                  slots=None, share_prefix=False, adjusts=None):
        """n continuations of the cache [0, length) on the slots of a decode batch; None when the batch does not fit the engine;
        return_logprobs: (token lists, log-probability tensors); slots: the slot count of a wide batch (_mmu_wide_slots);
        share_prefix (with slots): the slots are suffix caches that read [0, length) in the session's cache"""
        shared = bool(share_prefix and slots)

        def slot_engine(slots):
            return _SessionSlotEngine(self.model, self.eng, rows, lens, slots, temps, top_ks, seeds, noises, eot_token, self.dev, top_ps,
                                      want_lp=return_logprobs, share_prefix=shared, adjusts=adjusts, max_new_tokens=max_new_tokens)

        capacity = _shared_suffix_capacity(length, lens, max_new_tokens) if shared else length + max(lens) + max_new_tokens + 1
        return _run_on_slots(self.eng, len(rows), slots, capacity, slot_engine, max_new_tokens, eot_token, return_logprobs, shared=shared)


class _SessionRecompute:
    """engine side of MmuSession in accuracy mode without the production-kernel form (tiny test shapes): no KV cache, the session
    keeps the embeddings and the dense mask and every generate runs the reference's own algorithm on them (_mmu_generate_recompute)"""
    batched = False

    def __init__(self, model):
        self.model = model
        self.dev = model.showo.lm_head.weight.device
        self.emb = self.mask = None

    def stamp(self):
        return ()

    def cached_rows(self):
        return self.emb.shape[1]

    embed = _SessionEngine.embed

    def prefill(self, idx, input_embeddings, attention_mask):
        if input_embeddings is not None:
            self.emb = input_embeddings.detach().float().contiguous()
        else:
            self.emb = self.model.showo.model.embed_tokens.weight.detach().float()[idx.to(torch.int64)].contiguous()
        L = self.emb.shape[1]
        self.mask = _dense_mask_of(attention_mask, L, self.dev)
        return L

    def use_prefix_logits(self):
        pass

    def append(self, ids, emb, Ln):
        if emb is None:
            emb = self.model.showo.model.embed_tokens.weight.detach().float()[ids]
        grown = _grow_mask(self.mask, self.emb.shape[1], Ln)
        self.emb, self.mask = torch.cat([self.emb, emb.reshape(1, Ln, -1)], dim=1).contiguous(), grown

    def rewind(self, length):
        self.emb, self.mask = self.emb[:, :length].contiguous(), self.mask[:, :, :length, :length].contiguous()

    def settle(self, length, toks):
        if len(toks) > 1:
            self.append(torch.tensor([toks[:-1]], dtype=torch.int64, device=self.dev), None, len(toks) - 1)

    def run(self, max_new_tokens, greedy, k, temperature, noise, seed, eot_token, top_p=None, return_logprobs=False, adjust=None):
        out = self.model._mmu_generate_recompute(None, self.emb, self.mask, max_new_tokens, temperature, 1 if greedy else k, eot_token,
                                                 greedy, None if greedy else (k, seed, noise), top_p=top_p, return_logprobs=return_logprobs,
                                                 **({} if adjust is None else {"adjust": adjust}))
        if return_logprobs:
            return [int(t) for t in out[0]], out[1]
        return [int(t) for t in out]

    def score(self, ids, Ln, use_prefix_logits):
        """_SessionEngine.score on the recompute path: the rows join the kept embeddings and mask, one forward scores them"""
        L = self.emb.shape[1]
        self.append(ids, None, Ln)
        j0 = 0 if use_prefix_logits else 1
        lp = torch.full((Ln,), float("nan"), dtype=torch.float32, device=self.dev)
        rk = torch.full((Ln,), -1, dtype=torch.int32, device=self.dev)
        if Ln > j0:
            rows = torch.arange(L + j0 - 1, L + Ln - 1, dtype=torch.int32, device=self.dev)
            a, b = self.model._score_rows(None, self.emb, self.mask, 1, L + Ln, rows, ids.reshape(-1)[j0:].contiguous(), None)
            lp[j0:], rk[j0:] = a, b
        return lp, rk


class MmuSession:
    """A conversation about one prefix (`Showo.mmu_session`): the prefix is prefilled once, every `generate` appends its rows to the
    KV cache and decodes, `mark` / `rewind` go back to an earlier state, `generate_batch` answers n questions about the current state
    together.  `length`: rows in the cache; `prefix_length`: rows of the prefill (the floor of `rewind`)."""

    def __init__(self, model, idx=None, input_embeddings=None, attention_mask=None, _engine=None):
        if (idx is None) == (input_embeddings is None):
            raise ValueError("exactly one of idx / input_embeddings must be given")
        if (idx if idx is not None else input_embeddings).shape[0] != 1:
            raise ValueError("an mmu session has batch-1 semantics, like mmu_generate (reference modeling_showo.py:204,229)")
        self.model = model
        if _engine is not None:
            self._be = _engine
        elif int(getattr(model, "_precision", 0)) == 1 and (getattr(model, "precise_recompute", False) or
                                                            not _lib.load().showo_engine_precise_fast(model.engine())):
            self._be = _SessionRecompute(model)
        else:
            self._be = _SessionEngine(model)
        self.prefix_length = self.length = int(self._be.prefill(idx, input_embeddings, attention_mask))
        self._pending = None  # the last token handed out: not in the cache yet, fed in front of the next rows
        self._stamp = self._be.stamp()

    def _check(self):
        stamp = self._be.stamp()
        if stamp is None or stamp != self._stamp:
            raise RuntimeError("this mmu session is stale: the engine's decode cache, weights or precision changed since it was opened "
                               "(mmu_generate, a newer mmu_session, set_precision, configure_workspace or a weight update); open a new "
                               "session")
        if self._be.cached_rows() != self.length:
            raise RuntimeError(f"this mmu session is out of step with its cache ({self._be.cached_rows()} rows cached, {self.length} "
                               "expected: an earlier call failed midway and could not be undone); open a new session")

    def mark(self):
        """the current state (rows in the cache, pending token) for a later `rewind`"""
        return (self.length, self._pending)

    def rewind(self, mark):
        """back to a state `mark()` returned earlier in THIS session (its length is between the prefix length and the current one)"""
        length, pending = mark
        if not self.prefix_length <= int(length) <= self.length:
            raise ValueError(f"rewind: length {length} outside [{self.prefix_length}, {self.length}]")
        if pending is None and int(length) != self.prefix_length:
            raise ValueError("rewind: a state behind the prefix needs its pending token (pass what mark() returned)")
        self._check()
        self._be.rewind(int(length))
        self.length, self._pending = int(length), pending

    def _rows(self, idx, input_embeddings):
        """the caller's [1, Ln] ids or [1, Ln, H] embeddings with the pending token in front: (ids, emb, Ln), all None / 0 for no rows"""
        if idx is not None and input_embeddings is not None:
            raise ValueError("at most one of idx / input_embeddings")
        dev, p = self._be.dev, self._pending
        if input_embeddings is not None:
            if input_embeddings.shape[0] != 1:
                raise ValueError("an mmu session has batch-1 semantics")
            emb = input_embeddings.detach().float().to(dev)
            if p is not None:
                emb = torch.cat([self._be.embed(p).to(dev), emb], dim=1)
            return None, emb.contiguous(), int(emb.shape[1])
        ids = None if idx is None else idx.to(torch.int64).to(dev).reshape(1, -1)
        if p is not None:
            head = torch.tensor([[int(p)]], dtype=torch.int64, device=dev)
            ids = head if ids is None else torch.cat([head, ids], dim=1)
        if ids is None or ids.shape[1] == 0:
            return None, None, 0
        return ids.contiguous(), None, int(ids.shape[1])

    def _draw_args(self, max_new_tokens, temperature, top_k, generator, noise, top_p=None):
        """mmu_generate's _draw_params, with the session's own check (a session call emits at least one token) between the top_p
        check and the others; a checked p passes _nucleus_p unchanged"""
        p = _nucleus_p(top_p)
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        return _draw_params(self.model, max_new_tokens, temperature, top_k, p, generator, noise)

    @torch.no_grad()
    def generate(self, idx=None, input_embeddings=None, max_new_tokens=100, temperature=1.0, top_k=None, eot_token=None, generator=None,
                 _exp_noise=None, top_p=None, return_logprobs=False, repetition_penalty=None, repetition_context=None, logit_bias=None,
                 allowed_tokens=None, banned_tokens=None, num_beams=None, length_penalty=1.0, early_stopping=False,
                 num_return_sequences=1, return_beam_scores=False, no_repeat_ngram_size=None, bad_words_ids=None, min_new_tokens=None,
                 stop_sequences=None):
        """Append the rows (ids [1, Ln] or embeddings [1, Ln, H]; none: continue where the last call stopped), then decode like
        `mmu_generate`: same return type, `eot_token` cut, greedy pick for top_k == 1 and sampled draws (`top_p`: nucleus).  Afterwards the cache holds the
        prefix, the rows and the answer up to its last token but one; the last token is pending and is fed first by the next call.
        `return_logprobs=True`: `(tokens, logprobs)` as `mmu_generate` returns them.
        `repetition_penalty` / `repetition_context` / `logit_bias` / `allowed_tokens` / `banned_tokens`: as `mmu_generate` takes them.  The
        set of seen tokens belongs to THIS call (the context ids, then the tokens it produces): it does not live in the session, `mark`
        / `rewind` and the cache do not know it, and an identical call from the same state gives identical tokens.
        `no_repeat_ngram_size` / `bad_words_ids` / `min_new_tokens` / `stop_sequences`: as `mmu_generate` takes them.  The token history
        belongs to THIS call as the set does; the session settles on an answer cut by a stop sequence as it does behind an <eot>.
        `num_beams` / `length_penalty` / `early_stopping` / `num_return_sequences` / `return_beam_scores`: as `mmu_generate` takes them
        (None or 1: the call without them).  The search runs on forks of the cache and leaves the session's rows as they are; afterwards
        the BEST hypothesis is the answer: its tokens but the last are appended with one showo_engine_prefill_append of ids and its
        last token is pending, the state shape a greedy `generate` leaves.  These answer rows carry the bits of the append path, not
        those of the decode steps that scored them (both are the rows of the same tokens; a follow-up turn reads the appended ones)."""
        adj_vals = (repetition_penalty, repetition_context, logit_bias, allowed_tokens, banned_tokens, no_repeat_ngram_size, bad_words_ids,
                    min_new_tokens, stop_sequences)
        beams = _beam_request(self.model, num_beams, length_penalty, early_stopping, num_return_sequences, return_beam_scores, max_new_tokens,
                              temperature, top_k, top_p, generator, _exp_noise, any(v is not None for v in adj_vals))
        if beams is not None and not hasattr(self._be, "run_beam"):
            raise ValueError("beam search needs the KV-cached engine (precision 0, 2 or 3)")
        adjust = _adjust_of(self.model.vocab_size, *adj_vals, eot_token=eot_token) if any(v is not None for v in adj_vals) else None
        self._check()
        ids, emb, Ln = self._rows(idx, input_embeddings)
        if Ln == 0 and self.length != self.prefix_length:
            raise ValueError("generate: no rows and no pending token to continue from")
        # (a beam call draws nothing: no seed is taken from the generator)
        greedy, k, noise, seed, p = self._draw_args(max_new_tokens, temperature, 1 if beams is not None else top_k, generator, _exp_noise, top_p)
        nucleus = {} if p is None else {"top_p": p}  # an engine stand-in without the keyword still serves every call without top_p
        if return_logprobs:
            nucleus["return_logprobs"] = True
        if adjust is not None:
            nucleus["adjust"] = adjust
        lps = None
        start = self.length
        try:
            if Ln:
                self._be.append(ids, emb, Ln)
                self.length += Ln
            else:
                self._be.use_prefix_logits()
            if beams is not None:
                hyps = self._be.run_beam(self.length, beams, max_new_tokens, eot_token, float(length_penalty), early_stopping)
                toks = hyps[0]["tokens"]
                if len(toks) > 1:
                    fed = torch.tensor([toks[:-1]], dtype=torch.int64, device=self._be.dev)
                    self._be.append(fed, None, len(toks) - 1)
            else:
                toks = self._be.run(max_new_tokens, greedy, k, temperature, noise, seed, eot_token, **nucleus)
                if return_logprobs:
                    toks, lps = toks
                self._be.settle(self.length, toks)
        except BaseException:
            # a call that fails midway (a full cache inside the decode loop) leaves the session where it was: the rows it wrote are
            # dropped; if even that fails, _check finds the cache out of step on the next call
            self.length = start
            if self._be.cached_rows() != start:
                self._be.rewind(start)
            raise
        self.length += len(toks) - 1
        self._pending = toks[-1]
        if beams is not None:
            return _beam_result(hyps, num_return_sequences, return_logprobs, return_beam_scores, self._be.dev)
        out = [torch.tensor(t, device=self._be.dev) for t in toks]
        return (out, lps) if return_logprobs else out

    @torch.no_grad()
    def score(self, idx):
        """How probable the continuation `idx` (int64 [1, Ln]) is here: `TokenScores(logprobs, ranks)`, both [Ln], entry j the
        log-probability / rank of idx[0, j] given the conversation so far and idx[0, :j] -- the pending token is fed first, as
        `generate` feeds it.  A list of continuations is scored one after the other against the same state and returns a list.  The
        session is left as it was (same length, same pending token): a following `generate` returns what it would have returned.
        The rows run as an append (`showo_engine_prefill_append_score`), so the values agree with `generate(..., return_logprobs=True)`
        to the precision's gate, not bit for bit, and a short append costs what DESIGN.md's "mmu sessions" records for it;
        `Showo.score` on full prompts is the bulk path."""
        self._check()
        many = isinstance(idx, (list, tuple))
        out = []
        for t in (idx if many else [idx]):
            if t.dim() != 2 or t.shape[0] != 1 or t.shape[1] < 1:
                raise ValueError("score: a continuation is an int64 [1, Ln] tensor with Ln >= 1")
            if self._pending is None and self.length != self.prefix_length:
                raise ValueError("score: no pending token to continue from")
            ids, _, Ln = self._rows(t, None)
            j0 = 0 if self._pending is None else 1
            try:
                lp, rk = self._be.score(ids, Ln, self._pending is None)
            finally:
                if self._be.cached_rows() != self.length:
                    self._be.rewind(self.length)
            out.append(TokenScores(lp[j0:], rk[j0:]))
        return out if many else out[0]

    @torch.no_grad()
    def generate_batch(self, idx=None, input_embeddings=None, max_new_tokens=100, temperature=1.0, top_k=None, eot_token=None,
                       generator=None, _exp_noise=None, top_p=None, return_logprobs=False, slots=None, share_prefix=False,
                       repetition_penalty=None, repetition_context=None, logit_bias=None, allowed_tokens=None, banned_tokens=None,
                       no_repeat_ngram_size=None, bad_words_ids=None, min_new_tokens=None, stop_sequences=None):
        """n continuations of the CURRENT state: `idx` / `input_embeddings` is a list of n row blocks ([1, Ln_i] ids or [1, Ln_i, H]
        embeddings), `temperature` / `top_k` / `top_p` scalars or lists, `_exp_noise` None or a list.  result[i] is what `generate(<block i>)`
        followed by a rewind returns when those calls are made in order (same seeds from `generator`); the session is left unchanged.
        n >= 2 at precision 0, 2, 3 runs on the slots of a decode batch, each slot a fork of this cache.
        `return_logprobs=True`: `(tokens, logprobs)`, logprobs a list of n fp32 device tensors.
        `slots=S` (an int in 9..32, precision 0; else ValueError): n > 8 continuations run on min(S, n) slots of a WIDE decode batch
        (`Showo.mmu_generate_batch` states its contract: deterministic, independent of S / n / slot / neighbours, bf16-class and not
        the batch-1 bits); n <= 8 is the call without `slots`.
        `share_prefix=True` (needs `slots=S` and precision 0; else ValueError): the slots of that wide batch keep only the rows BEHIND
        the session's cache and attend to [0, length) in place (showo_engine_batch_begin_shared, csrc/attn_shared.hip): no fork copy,
        a quarter of the slot memory, the prefix read once per head and step.  Contract: deterministic run to run; a request's tokens
        and log-probabilities do not depend on S, n, its slot, the request order or its neighbours; the first token of every request
        comes from logits bit-equal to `generate`'s; later tokens are bf16-class and NOT the bits of the forked wide path (P is
        rounded relative to its key segment's max, not the row's, and the fp32 sums are split); the session, including its cache
        bits, is unchanged afterwards.  n <= 8 is the call without `slots` / `share_prefix`.
        `repetition_penalty` / `repetition_context` / `logit_bias` / `allowed_tokens` / `banned_tokens`: shared values or per-request lists
        as `Showo.mmu_generate_batch` takes them; every request has its own set of seen tokens, none of it stays in the session.
        `no_repeat_ngram_size` / `bad_words_ids` / `min_new_tokens` / `stop_sequences`: shared values or per-request lists as
        `Showo.mmu_generate_batch` takes them; every request has its own token history, none of it stays in the session."""
        seqs = idx if idx is not None else input_embeddings
        n = len(seqs)
        adjusts, adj_kws = None, [{}] * n
        if any(v is not None for v in (repetition_penalty, repetition_context, logit_bias, allowed_tokens, banned_tokens, no_repeat_ngram_size,
                                       bad_words_ids, min_new_tokens, stop_sequences)):
            adjusts, adj_kws = _adjust_per_request(n, self.model.vocab_size, repetition_penalty, repetition_context, logit_bias,
                                                   allowed_tokens, banned_tokens, no_repeat_ngram_size, bad_words_ids, min_new_tokens,
                                                   stop_sequences, eot_token)
        self._check()
        if share_prefix and slots is None:
            raise ValueError("share_prefix needs slots=S (the slots of a wide decode batch share the prefix)")
        if share_prefix and int(getattr(self.model, "_precision", 0)) != 0:
            raise ValueError("share_prefix needs precision 0 (bf16 operands)")
        wide = _mmu_wide_slots(slots, n, getattr(self.model, "_precision", 0))
        temps, top_ks, top_ps, noises, _ = _per_request(n, temperature, top_k, top_p, _exp_noise)

        def single(b):
            mark = self.mark()
            try:
                return self.generate(idx=None if idx is None else idx[b], input_embeddings=None if input_embeddings is None else input_embeddings[b],
                                     max_new_tokens=max_new_tokens, temperature=temps[b], top_k=top_ks[b], eot_token=eot_token,
                                     generator=generator, _exp_noise=noises[b], top_p=top_ps[b],
                                     **({"return_logprobs": True} if return_logprobs else {}), **adj_kws[b])
            finally:
                self.rewind(mark)

        if n < 2 or not self._be.batched:
            return _singles(single, n, return_logprobs)
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        rows, lens = [], []
        for b in range(n):
            ids, emb, Ln = self._rows(idx[b] if idx is not None else None, input_embeddings[b] if input_embeddings is not None else None)
            if Ln == 0:
                raise ValueError("generate_batch: every sequence needs rows (or the session a pending token)")
            _check_request(self.model, max_new_tokens, temps[b], top_ks[b], noises[b])
            rows.append((ids, emb))
            lens.append(Ln)
        gen_state = None if generator is None else generator.get_state()
        seeds = _mmu_batch_seeds(top_ks, generator)
        dev = self._be.dev
        noises = _batch_noises(top_ks, noises, dev)
        nucleus = {} if all(q is None for q in top_ps) else {"top_ps": top_ps}
        if return_logprobs:
            nucleus["return_logprobs"] = True
        if wide:
            nucleus["slots"] = wide
            if share_prefix:
                nucleus["share_prefix"] = True
        if adjusts is not None:
            nucleus["adjusts"] = adjusts
        out = self._be.run_batch(self.length, rows, lens, max_new_tokens, temps, top_ks, seeds, noises, eot_token, **nucleus)
        if out is None:  # the batch's common capacity does not fit the engine: the sequential calls, drawing the same seeds again
            if gen_state is not None:
                generator.set_state(gen_state)
            return _singles(single, n, return_logprobs)
        out, lps = out if return_logprobs else (out, None)
        toks = [[torch.tensor(t, device=dev) for t in r] for r in out]
        return (toks, lps) if return_logprobs else toks


def mmu_session(self, idx=None, input_embeddings=None, attention_mask=None):
    """Open an `MmuSession`: prefill `idx` [1, L] or `input_embeddings` [1, L, H] under `attention_mask` (dense or IntervalMask) ONCE and
    keep its KV cache for any number of questions -- the question loop of the reference's inference_mmu.py:99-176 prefills the whole
    prompt (631 rows with the CLIP tower, 607 of them question-invariant) per question.

        sess = model.mmu_session(input_embeddings=prefix, attention_mask=prefix_mask)
        a1 = sess.generate(input_embeddings=q1, max_new_tokens=100, top_k=1, eot_token=eot)   # rows appended, then decoded
        a2 = sess.generate(idx=q2_ids, ...)                       # follow-up: the cache holds prefix, q1 and a1
        sess.rewind(mark)                                          # ... or back to `mark = sess.mark()` and ask something else
        outs = sess.generate_batch(input_embeddings=[q1, q2, q3], ...)   # n questions about the current state, decoded together

    Prefix + appended rows equal the full prompt (in exact arithmetic; on the GPU to the bf16 gates, since a 24-row and a 631-row
    GEMM round differently) exactly when `prompting_utils.mmu_prefix_is_exact(full_mask, P)` holds for the full prompt's mask at
    the split P: no prefix row sees a later column and every later row sees what row P - 1 sees plus the columns up to itself.  Both
    mmu mask families satisfy it at every split behind <|eoi|>.  Appended rows attend as decode rows (last prefill row + causal).
    The engine owns ONE decode cache: `mmu_generate`, another `mmu_session`, `set_precision` or a weight update make this session
    stale, and its next call raises RuntimeError."""
    return MmuSession(self, idx, input_embeddings, attention_mask)


Showo.mmu_session = mmu_session


def _dense_mask_of(attention_mask, L, device):
    """[1,1,L,L] additive fp32 mask from whatever mmu_generate accepts (dense tensor, IntervalMask, None = causal)"""
    from .prompting_utils import IntervalMask
    neg = float(torch.iinfo(torch.int64).min)
    if attention_mask is None:
        m = torch.zeros((L, L), dtype=torch.float32, device=device)
        m.masked_fill_(torch.ones((L, L), dtype=torch.bool, device=device).triu(1), neg)
        return m.reshape(1, 1, L, L)
    if isinstance(attention_mask, IntervalMask):
        iv = attention_mask.check().iv.reshape(-1, L, 4)[:1].to(torch.int64)
        col = torch.arange(L, device=iv.device)[None, None, :]
        vis = ((col >= iv[..., 0:1]) & (col < iv[..., 1:2])) | ((col >= iv[..., 2:3]) & (col < iv[..., 3:4]))
        return torch.where(vis, 0.0, neg).to(torch.float32).reshape(1, 1, L, L).to(device)
    return attention_mask.detach().float().reshape(1, 1, L, L).to(device)


def _grow_mask(mask, L, Ln):
    """the dense [1, 1, L, L] mask grown by Ln decode rows: the new columns hidden from the old rows (the reference pads them with
    finfo(dtype).min, :206-209), every new row = the last row + causal among the new ones (:203-217)"""
    neg = float(torch.finfo(torch.float32).min)
    grown = torch.full((1, 1, L + Ln, L + Ln), neg, dtype=torch.float32, device=mask.device)
    grown[0, 0, :L, :L] = mask[0, 0]
    grown[0, 0, L:, :L] = mask[0, 0, L - 1]
    grown[0, 0, L:, L:].masked_fill_(torch.ones((Ln, Ln), dtype=torch.bool, device=mask.device).tril(), 0.0)
    return grown


def _mmu_generate_recompute(self, idx, input_embeddings, attention_mask, max_new_tokens, temperature, top_k, eot_token, greedy, sampling,
                            top_p=None, return_logprobs=False, adjust=None):
    """Accuracy mode (`set_precision(1)`): the reference's OWN algorithm (models/modeling_showo.py:190-240) -- no KV cache, the whole
    sequence is run again for every token on the grown mask (new column hidden from the old rows, new row = last row + itself,
    :203-217) -- on the fp32-class engine path.  O(tokens x forward): a parity mode, not a serving mode.
    `adjust` (an _Adjust): every step's pick reads the row the stand-alone showo_logits_adjust writes, and the picked token is marked."""
    eng = self.engine()
    dev = idx.device if idx is not None else input_embeddings.device
    if (input_embeddings if input_embeddings is not None else idx).shape[0] != 1:
        raise ValueError("mmu_generate has batch-1 semantics (reference modeling_showo.py:204,229)")
    if input_embeddings is not None:
        emb = input_embeddings.detach().float().contiguous()
    else:
        emb = self.showo.model.embed_tokens.weight.detach().float()[idx.to(torch.int64)].contiguous()
    L = emb.shape[1]
    mask = _dense_mask_of(attention_mask, L, dev)
    row = torch.empty((1,), dtype=torch.int32, device=dev)
    logits = torch.empty((self.vocab_size,), dtype=torch.float32, device=dev)
    tok = torch.empty((1,), dtype=torch.int64, device=dev)
    result, lps = [], []
    st, stops, ints = None, None, []
    if adjust is not None:
        st = _AdjustState(self.vocab_size, 1, dev, _hist_ld([adjust], max_new_tokens), eot_token)
        st.seed(0, adjust)
        stops = adjust.rules.stops if adjust.rules is not None else None
    for step in range(max_new_tokens):
        row.fill_(L - 1)
        _lib.call("showo_engine_forward_rows", eng, None, _lib.ptr(emb), _lib.ptr(mask), 1, L, _lib.ptr(row), 1, 0, self.vocab_size,
                  _lib.ptr(logits), _lib.stream())
        pick = logits if st is None else st.adjust(0, logits)
        if st is not None:  # (sequence rules: the stand-alone ban; the token of the last step joins the history in front of it)
            st.ban(0, tok if step else None)
        if greedy:
            _lib.call("showo_argmax_f32", _lib.ptr(pick), self.vocab_size, _lib.ptr(tok), _lib.stream())
        else:
            k, seed, noise = sampling
            _sample_call(pick, self.vocab_size, k, top_p, temperature, noise, seed, step, tok)
        if st is not None:
            st.mark(0, tok)
        if return_logprobs:
            lps.append(_logprob_of(logits, self.vocab_size, tok))
        t = int(tok.item())
        result.append(torch.tensor(t, device=dev))
        ints.append(t)
        if (eot_token is not None and t == eot_token) or (stops and _stop_len(ints, stops, None, step) is not None):
            break
        mask = _grow_mask(mask, L, 1)
        emb = torch.cat([emb, self.showo.model.embed_tokens.weight.detach().float()[tok].reshape(1, 1, -1)], dim=1).contiguous()
        L += 1
    if return_logprobs:
        return result, (torch.cat(lps) if lps else torch.empty((0,), dtype=torch.float32, device=dev))
    return result


Showo._mmu_generate_recompute = _mmu_generate_recompute


def gen_config(llm_vocab_size=50295, num_new_special_tokens=10, num_vq_tokens=256, max_seq_length=128):
    """The subset of the OmegaConf config that t2i_generate reads (reference modeling_showo.py:123-133)."""
    ns = types.SimpleNamespace
    return ns(model=ns(showo=ns(num_vq_tokens=num_vq_tokens, num_new_special_tokens=num_new_special_tokens,
                                llm_vocab_size=llm_vocab_size)),
              dataset=ns(preprocessing=ns(max_seq_length=max_seq_length)))
