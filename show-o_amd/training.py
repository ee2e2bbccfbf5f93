"""Data-parallel training step on the HIP path (reference training/train.py:510-628 + accelerate/DeepSpeed gradient
exchange, accelerate_configs/*.yaml).

`Trainer.step()` = Showo.forward with labels -> backward -> gradient exchange -> AdamW, all on HIP kernels; the only
collective of the step is the gradient average (RCCL through torch.distributed, one all-reduce per gradient bucket:
head, then transformer blocks last to first, then the embedding), issued as soon as the bucket's backward kernels are
queued so that it overlaps the backward of the next block.  One process per GPU; every rank draws its own batch and the
three losses are per-rank means, averaged across ranks by the gradient average exactly as DDP does.
"""
import ctypes as C
from typing import Any, NamedTuple

import torch

from . import _lib

NO_DECAY = ("bias", "layer_norm.weight", "mlm_ln.weight", "embeddings.weight")  # reference training/train.py:211
PROJECTOR_KEYS = ("mm_projector.0.weight", "mm_projector.0.bias", "mm_projector.2.weight", "mm_projector.2.bias")


class _DevView:
    """zero-copy torch view of a raw device buffer owned by the HIP library (__cuda_array_interface__ v2)"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f4", "data": (int(ptr), False), "version": 2}


def device_view(ptr, n, device):
    return torch.as_tensor(_DevView(ptr, n), device=device)


class HipWireOps:
    """staging of the gradient wire on the device: HIP kernels on the current stream (include/showo_hip.h)"""

    @staticmethod
    def pack(grad, wire, scale):
        _lib.call("showo_grad_wire_pack", grad.data_ptr(), wire.data_ptr(), grad.numel(), float(scale), _lib.stream())

    @staticmethod
    def unpack(wire, grad):
        _lib.call("showo_grad_wire_unpack", wire.data_ptr(), grad.data_ptr(), grad.numel(), _lib.stream())

    @staticmethod
    def scale(grad, s):
        _lib.call("showo_scale_f32", grad.data_ptr(), grad.numel(), float(s), _lib.stream())


class GradientExchange:
    """The ONE exchange step of a data-parallel iteration (reference: accelerate / DeepSpeed around
    `accelerator.backward`, training/train.py:449,612): every gradient bucket is averaged over the process group with one
    all-reduce, launched as soon as the bucket's backward kernels are queued (`launch(b)`), and all of them are completed before the
    optimizer runs (`finish()`).

    wire = "bf16" (default, the reference's `mixed_precision: bf16` wire, 2 bytes per gradient): the bucket is scaled by 1/world
    and rounded to a bf16 staging buffer, the staging buffer is summed by the collective and widened back into the fp32 bucket.
    wire = "fp32": the fp32 bucket itself is summed and then scaled (twice the volume, no rounding).
    `ops` supplies pack / unpack / scale for the device the buckets live on (HipWireOps for the GPU path)."""

    def __init__(self, buckets, dist, group=None, wire="bf16", ops=HipWireOps):
        if wire not in ("bf16", "fp32"):
            raise ValueError("wire must be 'bf16' or 'fp32'")
        self.buckets, self.dist, self.group, self.wire, self.ops = buckets, dist, group, wire, ops
        self.world = dist.get_world_size(group)
        self.stage = [torch.empty(b.numel(), dtype=torch.bfloat16, device=b.device) for b in buckets] if wire == "bf16" else None
        self.works = []
        self._measure, self._spans, self._bspans = False, [], []

    def measure(self, on=True):
        """record the GPU time of every finish() (device events on the compute stream) from now on; exposed_ms() reads the mean,
        exposed_ms_per_bucket() the same split by bucket (wait for that bucket's collective + widening its wire)"""
        self._measure, self._spans, self._bspans = bool(on), [], []

    def exposed_ms_per_bucket(self):
        """{bucket index: mean GPU ms per step the compute stream spent waiting for / unpacking that bucket inside finish()}: buckets
        whose all-reduce hid behind the backward show only their unpack time; None when nothing was measured"""
        if not self._bspans:
            return None
        torch.cuda.synchronize()
        acc, cnt = {}, {}
        for b, e0, e1 in self._bspans:
            acc[b] = acc.get(b, 0.0) + e0.elapsed_time(e1)
            cnt[b] = cnt.get(b, 0) + 1
        return {b: acc[b] / cnt[b] for b in sorted(acc)}

    def exposed_ms(self):
        """mean GPU time per step that the compute stream spent in finish(): waiting for collectives that did not hide behind the
        backward, plus widening / scaling the wire.  None when nothing was measured (CPU buckets, measure() off)."""
        if not self._spans:
            return None
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in self._spans) / len(self._spans)

    def wire_bytes(self):
        """bytes every rank hands to the collective per step"""
        return sum(b.numel() for b in self.buckets) * (2 if self.wire == "bf16" else 4)

    def launch(self, b):
        if self.wire == "bf16":
            self.ops.pack(self.buckets[b], self.stage[b], 1.0 / self.world)
            t = self.stage[b]
        else:
            t = self.buckets[b]
        self.works.append((self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True), b))

    def finish(self):
        span = None
        if self._measure and self.buckets and self.buckets[0].is_cuda:
            span = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            span[0].record()
        self._finish()
        if span is not None:
            span[1].record()
            self._spans.append(span)

    def _finish(self):
        timed = self._measure and self.buckets and self.buckets[0].is_cuda
        for w, b in self.works:
            if timed:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            if w is not None:
                w.wait()
            if self.wire == "bf16":
                self.ops.unpack(self.stage[b], self.buckets[b])
            else:
                self.ops.scale(self.buckets[b], 1.0 / self.world)
            if timed:
                e1.record()
                self._bspans.append((b, e0, e1))
        self.works = []


def train_mask(tr, attention_mask):
    """dense additive [B,1,L,L] mask -> contiguous fp32 tensor; IntervalMask (prompting_utils.intervals_* /
    training_utils.build_training_batch) -> registered with the trainer, returns None (no dense mask is passed)"""
    from .prompting_utils import IntervalMask
    if attention_mask is None:
        return None
    if isinstance(attention_mask, IntervalMask):
        # no host-side check(): a mask the intervals cannot represent turns the losses into NaN on the device
        _lib.call("showo_trainer_use_intervals", tr, _lib.ptr(attention_mask.iv.contiguous()), _lib.ptr(attention_mask.flag))
        return None
    return attention_mask.detach().float().contiguous()


class AccumulationWindow:
    """Bookkeeping of gradient accumulation (reference: `accelerator.accumulate(model)` around the step body,
    training/train.py:589-631, with `training.gradient_accumulation_steps` = k): a window is k consecutive micro-batches that feed
    ONE optimizer step.  Pure Python, no device state: `position` is the index of the NEXT micro-batch inside its window,
    `is_first` says that it overwrites the gradient buffer (the others add into it), `closes` that it is followed by the exchange,
    clipping and the optimizer, and `loss_scale` = 1 / k is what accelerate multiplies every micro-batch loss by -- the window's
    gradient is the mean of the micro-batch gradients (a mean of per-micro-batch means, not a global token mean)."""

    def __init__(self, steps=1):
        if int(steps) != steps or int(steps) < 1:
            raise ValueError("gradient_accumulation_steps must be an integer >= 1")
        self.steps = int(steps)
        self.position = 0
        self.windows_closed = 0

    @property
    def is_first(self):
        return self.position == 0

    @property
    def closes(self):
        return self.position == self.steps - 1

    @property
    def is_open(self):
        """some micro-batch of the current window has run and its optimizer step has not: the gradient buffer holds a partial sum"""
        return self.position != 0

    @property
    def loss_scale(self):
        return 1.0 / self.steps

    def scaled(self, coeffs):
        """the loss weights of one micro-batch; k = 1 hands the caller's values through untouched"""
        return tuple(coeffs) if self.steps == 1 else tuple(c / self.steps for c in coeffs)

    def advance(self):
        """one micro-batch done; returns True when it closed its window"""
        closed = self.closes
        self.position = 0 if closed else self.position + 1
        self.windows_closed += int(closed)
        return closed

    def reset(self):
        self.position = 0


LOSS_ROWS = ("all", "labelled")


def loss_rows_mode(loss_rows):
    """`Trainer(loss_rows=...)` -> the mode of showo_train_set_loss_rows: "all" = 0 (the head runs on every token row),
    "labelled" = 1 (on the rows that carry a label).  Anything else is a ValueError (no device is touched)."""
    if not isinstance(loss_rows, str) or loss_rows not in LOSS_ROWS:
        raise ValueError(f"loss_rows must be one of {LOSS_ROWS}, got {loss_rows!r}")
    return LOSS_ROWS.index(loss_rows)


class MicroBatch(NamedTuple):
    """one micro-batch as the native calls take it: contiguous int64 ids / labels [B, L], the dense fp32 mask or None (train_mask),
    split = (batch_size_t2i, batch_size_lm, batch_size_mmu, max_seq_length), w = the three loss weights of this micro-batch"""
    ids: Any
    mask: Any
    labels: Any
    B: int
    L: int
    split: tuple
    w: tuple


class SplicedImage(NamedTuple):
    """the image rows of step_clip_vit: the projector module, its output rows fp32 [n * P, H] and the int32 start columns on the device
    (both None when n * P == 0), n image sequences of P placeholder columns"""
    projector: Any
    rows: Any
    start: Any
    n: int
    P: int


class Trainer:
    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, coeffs=(1.0, 0.1, 1.0), group=None,
                 wire="bf16", max_grad_norm=None, force_exchange=False, reserve_cus=None, gradient_accumulation_steps=1,
                 loss_rows="all", *, ema=None, projector=False):
        """gradient_accumulation_steps = k (every training YAML of the reference carries it): one step() call is one micro-batch;
        the first of a window overwrites the native gradient buffer, the others add into it (the accumulating kernel forms,
        showo_train_set_accumulate) with loss weights coeffs / k, and only the k-th runs the exchange, clipping, AdamW and the image
        refresh.  `sync_gradients` (accelerate's name) is True exactly after a call that closed a window.  k = 1 is the plain step.
        wire: "bf16" | "fp32" gradient wire of the exchange (GradientExchange).  max_grad_norm: global-norm clipping before the
        optimizer (training/train.py:614-615; null in the shipped stage-1 YAMLs).  force_exchange: run the exchange even in a
        process group of one rank (tests: drives the RCCL path on a single GPU).  reserve_cus: while an exchange is active the step's
        kernels run on a stream that keeps this many CUs free for RCCL's channel kernels (showo_stream_create_cu_mask; None = the
        SHOWO_RESERVE_CUS environment variable, default 0 = no mask: profiles/r4_exchange_contention.txt).
        loss_rows: "all" (default) runs the loss head -- final LayerNorm, lm_head, cross-entropy and their backward -- on every token
        row; "labelled" on the rows that enter a loss (masked image tokens of the t2i rows, text rows of the lm rows, answer tokens of
        the mmu rows: training_utils.labelled_rows).  Same gradients below lm_head, lm_head's own differ in the grouping of their fp32
        row sums; the forward waits once on the host for the row count (DESIGN.md "Loss head on labelled rows").
        projector: False (default) trains model.showo alone, whatever else the model holds.  True (the w_clip_vit model, reference
        training/train_w_clip_vit.py): the `requires_grad` parameters of model.mm_projector join the trainable set -- their four
        gradients are one more exchange bucket, clipping takes ONE norm over the Show-o and projector gradients, the native AdamW
        updates them (no decay for names containing "bias"), checkpoints carry their moments after the showo.* entries -- and
        step_clip_vit() runs the micro-batch with the projector's rows spliced in (DESIGN.md "CLIP-ViT training step").  A model
        whose showo is wholly frozen (LLaVA-pretrain) is accepted when the projector trains.
        ema: None (default, off), a float decay, or a dict of `training_utils.EMA` keyword arguments (decay, min_decay,
        update_after_step, use_ema_warmup, inv_gamma, power).  `self.ema` is then an EMA whose `shadow_params` follow
        `self.params + self.pparams`, initialised as clones of the parameters.  Every call that closes an accumulation window counts one
        EMA step (the reference idiom `if accelerator.sync_gradients: ema.step(...)`) and the native AdamW launch updates the shadows of
        the trainable Show-o tensors from the new master values it holds in registers; the projector's shadows take one table launch
        behind their AdamW.  Frozen tensors get no update: their shadows are set equal to the parameters whenever the binding is
        (re)built, so a hand edit of a frozen tensor needs `model.mark_weights_dirty()` and a new binding, as it does today.  Ranks
        exchange nothing for it: identical parameters give identical shadows.  `with trainer.ema_weights():` evaluates on the averaged
        weights; do not call `self.ema.step()` yourself (DESIGN.md "EMA of the weights")."""
        import os
        self._loss_rows_mode = loss_rows_mode(loss_rows)  # before anything touches the device
        self.loss_rows = loss_rows
        self.reserve_cus = int(os.environ.get("SHOWO_RESERVE_CUS", "0")) if reserve_cus is None else int(reserve_cus)
        self._masked_stream = None
        self.model, self.lr, self.betas, self.eps, self.wd, self.coeffs, self.group = model, lr, betas, eps, weight_decay, coeffs, group
        self.max_grad_norm = max_grad_norm
        self.step_count = 0
        self.window = AccumulationWindow(gradient_accumulation_steps)
        self.sync_gradients = False
        self.grad_norm = None  # total norm (device scalar) found by the clipping of the last closed window; None without max_grad_norm
        self._win_sum, self._win_n = None, 0
        self.params = [("showo." + n, p) for n, p in model.showo.named_parameters()]
        # the trainable set is read once, as the reference builds its optimizer once over the `requires_grad` parameters
        # (training/train.py:210-223): frozen tensors get no gradient, no exchange of a wholly frozen bucket and no update
        self.trainable = {n: bool(p.requires_grad) for n, p in self.params}
        self.projector = bool(projector)
        self.pparams, self.ptrainable = [], {}
        if self.projector:
            mm = getattr(model, "mm_projector", None)
            if mm is None:
                raise ValueError("Trainer(projector=True): the model has no mm_projector (build it with w_clip_vit=True)")
            self.pparams = [("mm_projector." + n, p) for n, p in mm.named_parameters()]
            if tuple(n for n, _ in self.pparams) != PROJECTOR_KEYS:
                raise ValueError(f"Trainer(projector=True): mm_projector's parameters are {[n for n, _ in self.pparams]}, expected {PROJECTOR_KEYS}")
            self.ptrainable = {n: bool(p.requires_grad) for n, p in self.pparams}
        self._ptrains = any(self.ptrainable.values())
        self._showo_trains = any(self.trainable.values())
        if not self._showo_trains and not self._ptrains:
            raise ValueError("Trainer: no parameter of model.showo requires grad; nothing to train" if not self.projector else
                             "Trainer: no parameter of model.showo or model.mm_projector requires grad; nothing to train")
        from .modeling_showo import _train_param_groups
        self._bucket_trains = [any(self.trainable[k] for k, _ in g) for g in _train_param_groups(model)]
        self._pbucket = None  # index of the projector's bucket (set by _bind when a projector parameter trains)
        self.m = {n: torch.zeros_like(p) for n, p in self.params + self.pparams}
        self.v = {n: torch.zeros_like(p) for n, p in self.params + self.pparams}
        # the projector's four gradients: one flat fp32 buffer of 256-byte aligned slots = the exchange bucket behind the head's
        self._pgrad, self._pviews = None, {}
        if self._ptrains:
            offs, cur = [], 0
            for _, p in self.pparams:
                offs.append(cur)
                cur += (p.numel() + 63) // 64 * 64
            self._pgrad = torch.zeros(cur, dtype=torch.float32, device=self.pparams[0][1].device)
            self._pviews = {n: self._pgrad[o:o + p.numel()].view(p.shape) for o, (n, p) in zip(offs, self.pparams)}
        self._wire, self._force_exchange = wire, force_exchange
        self.ema = self._make_ema(ema)
        self._pema = None      # segment table of the projector's shadows (training_utils.EmaTable)
        self._in_ema = False   # inside `with self.ema_weights()`: parameters and shadows are exchanged
        self._bound = None
        self._bind()

    def _make_ema(self, ema):
        if ema is None:
            return None
        from .training_utils import EMA
        if isinstance(ema, bool) or not isinstance(ema, (float, int, dict)):
            raise TypeError(f"Trainer(ema=...) takes None, a float decay or a dict of EMA keyword arguments, got {ema!r}")
        kw = dict(ema) if isinstance(ema, dict) else {"decay": float(ema)}
        if "parameters" in kw:
            raise TypeError("Trainer(ema={...}): the parameters are the trainer's own")
        if not 0.0 <= kw.get("decay", 0.9999) <= 1.0:
            raise ValueError("Trainer(ema=...): decay must be between 0 and 1")
        kw.setdefault("model_cls", type(self.model))
        if "model_config" not in kw and hasattr(self.model, "config") and hasattr(self.model, "arch"):
            kw["model_config"] = dict(self.model.config, **self.model.arch)
        return EMA([p for _, p in self.params + self.pparams], **kw)

    def _binding_key(self, params=None, pparams=None):
        params = self.params if params is None else params
        pparams = self.pparams if pparams is None else pparams
        shadows = tuple(s.data_ptr() for s in self.ema.shadow_params) if self.ema is not None else ()
        return (self.tr.value if hasattr(self.tr, "value") else int(self.tr),) + tuple(p.data_ptr() for _, p in params + pparams) + shadows

    def _bind(self):
        """(Re)create everything that holds raw pointers into the native trainer or the parameters: the gradient-bucket views, the
        exchange's staging buffers and the optimizer's parameter table.  Called by __init__ and by step() whenever the trainer
        handle changed (configure_workspace / _drop_engine re-create it) or a parameter's storage moved (load_state_dict(assign=True),
        .to(), ...): a stale handle would have no parameters bound and the native AdamW would write through dangling pointers."""
        self.tr = self.model.trainer()
        dev = self.params[0][1].device
        for n, p in self.params + self.pparams:
            if self.m[n].device != p.device or self.m[n].shape != p.shape:
                self.m[n] = torch.zeros_like(p)
                self.v[n] = torch.zeros_like(p)
        lib = _lib.load()
        self.buckets = []
        for b in range(lib.showo_train_num_buckets(self.tr)):
            ptr, n = C.c_void_p(), C.c_int64()
            _lib.check(lib.showo_train_bucket(self.tr, b, C.byref(ptr), C.byref(n)), "showo_train_bucket")
            self.buckets.append(device_view(ptr.value, n.value, dev))
        for n, p in self.params:  # master weights + moments are registered once per binding; the step is one C call
            if not p.is_contiguous() or p.dtype != torch.float32:
                raise ValueError(f"{n}: the native optimizer updates contiguous fp32 master parameters in place")
            _lib.call("showo_train_bind_param", self.tr, n.encode(), p.data_ptr(), self.m[n].data_ptr(), self.v[n].data_ptr(), p.numel())
        for n, p in self.pparams:
            if not p.is_contiguous() or p.dtype != torch.float32:
                raise ValueError(f"{n}: the native optimizer updates contiguous fp32 master parameters in place")
        if self._ptrains:  # the projector's gradients: one more bucket, behind the head's
            self._pbucket = len(self.buckets)
            self.buckets.append(self._pgrad)
        if self.ema is not None:
            self._bind_ema()
        import torch.distributed as dist
        group = self.group
        active = dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or self._force_exchange)
        self.exchange = GradientExchange(self.buckets, dist, group, wire=self._wire) if active else None
        self._bound = self._binding_key()

    # ---- EMA of the weights (DESIGN.md "EMA of the weights")
    def _bind_ema(self):
        """shadows -> the native trainer (Show-o tensors, next to showo_train_bind_param) and one stand-alone table (projector tensors).
        A shadow that no longer matches its parameter's device / shape is re-made as a clone; a frozen tensor's shadow is set equal to
        the parameter, here and nowhere else."""
        from .training_utils import EmaTable
        named = self.params + self.pparams
        sh = self.ema.shadow_params
        if len(sh) != len(named):
            raise ValueError(f"Trainer: the EMA holds {len(sh)} shadows, the trainer has {len(named)} parameters")
        trains = dict(self.trainable, **self.ptrainable)
        with torch.no_grad():
            for i, (n, p) in enumerate(named):
                s = sh[i]
                if s.device != p.device or s.shape != p.shape or s.dtype != torch.float32 or not s.is_contiguous():
                    sh[i] = p.detach().clone()
                elif not trains[n]:
                    s.copy_(p)
        for (n, p), s in zip(self.params, sh):
            _lib.call("showo_train_bind_ema", self.tr, n.encode(), s.data_ptr(), p.numel())
        if self._pema is not None:
            torch.cuda.synchronize(self._pema.device)  # a launch over the old table may still be in flight
            self._pema.close()
            self._pema = None
        if self.pparams:
            self._pema = EmaTable(sh[len(self.params):], [p.detach() for _, p in self.pparams])
            self._pmodes = [not self.ptrainable[n] for n, _ in self.pparams]

    def _ema_swap(self):
        """exchange parameters and shadows in place on the step's compute stream; the engine's and the projector's images follow"""
        ms = self.compute_stream()
        cur = torch.cuda.current_stream()
        if ms is not None:
            ms.wait_stream(cur)
        with torch.cuda.stream(ms if ms is not None else cur):
            _lib.call("showo_train_ema_swap", self.tr, _lib.stream())
            if self._pema is not None:
                self._pema.swap()
                self._projector_refresh([n for n, _ in self.pparams])
        if ms is not None:
            cur.wait_stream(ms)

    def ema_weights(self):
        """`with trainer.ema_weights():` -- inside, the model's parameters ARE the averaged weights (and the shadows hold the raw
        ones): `model.forward`, `t2i_generate`, `mmu_generate` and `score` run on them through the normal engine, whose weight images
        the swap kernel rewrote.  No third copy of the weights exists at any time.  The exit swaps back, exceptions included, and
        restores every bit.  Inside, step(), state_dict() and a nested ema_weights() raise RuntimeError."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            if self.ema is None:
                raise RuntimeError("Trainer.ema_weights needs Trainer(model, ema=...)")
            if self._in_ema:
                raise RuntimeError("Trainer.ema_weights: already inside ema_weights(); the parameters hold the averaged weights")
            self.tr = self.model.trainer()
            if self._binding_key() != self._bound:
                if self.window.is_open:
                    raise RuntimeError("Trainer.ema_weights: the native trainer or a tensor's storage changed inside an open accumulation window")
                self.params = [("showo." + n, p) for n, p in self.model.showo.named_parameters()]
                self.pparams = [("mm_projector." + n, p) for n, p in self.model.mm_projector.named_parameters()] if self.projector else []
                self._bind()
            self._ema_swap()
            self._in_ema = True
            try:
                yield self
            finally:
                self._in_ema = False
                self._ema_swap()
        return scope()

    def _refuse_inside_ema(self, what):
        if self._in_ema:
            raise RuntimeError(f"Trainer.{what} inside ema_weights(): the parameters hold the averaged weights; leave the context first")

    # ---- checkpoint / resume of the optimizer (reference: accelerator.save_state / load_state, training/train.py:851-889, 429-443)
    def state_dict(self):
        """torch.optim.AdamW layout: {'state': {i: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [...]} with the parameters
        numbered in `model.showo.named_parameters()` order, so the file is interchangeable with an AdamW built over that list.
        A projector=True trainer appends mm_projector.0.weight, .0.bias, .2.weight, .2.bias (the `model.named_parameters()` order).
        Refused inside an open accumulation window: the partial gradient sum is not part of the file.
        With EMA on, an "ema" entry holds `EMA.state_dict()` with the shadows cloned."""
        self._refuse_inside_ema("state_dict")
        if self.window.is_open:
            raise RuntimeError(f"Trainer.state_dict inside an open accumulation window (micro-batch {self.window.position} of "
                               f"{self.window.steps}): the partial gradient sum is not saved; checkpoint when sync_gradients is True")
        state = {i: {"step": torch.tensor(float(self.step_count)), "exp_avg": self.m[n].detach().clone(),
                     "exp_avg_sq": self.v[n].detach().clone()} for i, (n, _) in enumerate(self.params + self.pparams)}
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.wd,
                 "params": list(range(len(self.params) + len(self.pparams)))}
        out = {"state": state, "param_groups": [group], "param_names": [n for n, _ in self.params + self.pparams]}
        if self.ema is not None:
            out["ema"] = dict(self.ema.state_dict(), shadow_params=[s.detach().clone() for s in self.ema.shadow_params])
        return out

    def load_state_dict(self, sd):
        """moments are copied INTO the tensors bound to the native optimizer (showo_train_bind_param); lr / betas / eps / weight
        decay / step count are taken from the file.  An open accumulation window is dropped: the next step() starts a new one.
        EMA: a file with an "ema" entry restores the scalars and copies the shadows into the bound tensors; a file without one, loaded
        into an EMA trainer, resets the shadows to the current parameters and `optimization_step` to 0 (the averaging starts over);
        a trainer without EMA ignores the entry."""
        self._refuse_inside_ema("load_state_dict")
        self.window.reset()
        self.sync_gradients = False
        names = [n for n, _ in self.params + self.pparams]
        if "param_names" in sd and list(sd["param_names"]) != names:
            raise ValueError("optimizer state was saved for a different parameter list" +
                             (" (a file without mm_projector entries does not resume a projector=True trainer)" if self.projector else ""))
        if len(sd["state"]) not in (0, len(names)):
            raise ValueError(f"optimizer state has {len(sd['state'])} entries, the model has {len(names)} parameters")
        steps = set()
        with torch.no_grad():
            for i, n in enumerate(names):
                if i not in sd["state"]:
                    continue
                st = sd["state"][i]
                if tuple(st["exp_avg"].shape) != tuple(self.m[n].shape):
                    raise ValueError(f"{n}: moment shape {tuple(st['exp_avg'].shape)} != {tuple(self.m[n].shape)}")
                self.m[n].copy_(st["exp_avg"])
                self.v[n].copy_(st["exp_avg_sq"])
                steps.add(int(st["step"]))
        if len(steps) > 1:
            raise ValueError("per-parameter step counts differ: not an optimizer state this trainer can resume")
        g = sd["param_groups"][0]
        self.lr, self.betas, self.eps, self.wd = float(g["lr"]), tuple(g["betas"]), float(g["eps"]), float(g["weight_decay"])
        self.step_count = steps.pop() if steps else 0
        self._load_ema(sd.get("ema"))

    def _load_ema(self, esd):
        if self.ema is None:
            return
        sh = self.ema.shadow_params
        with torch.no_grad():
            if esd is None:
                for s, (_, p) in zip(sh, self.params + self.pparams):
                    s.copy_(p)
                self.ema.optimization_step, self.ema.cur_decay_value = 0, None
                return
            src = esd.get("shadow_params")
            if src is not None:
                if len(src) != len(sh) or any(tuple(a.shape) != tuple(b.shape) for a, b in zip(src, sh)):
                    raise ValueError("EMA state was saved for a different parameter list")
            self.ema.load_state_dict({k: v for k, v in esd.items() if k != "shadow_params"})
            if src is not None:
                for s, a in zip(sh, src):  # INTO the tensors bound to the native trainer
                    s.copy_(a)
        self.ema.cur_decay_value = self.ema.get_decay(self.ema.optimization_step) if self.ema.optimization_step > 0 else None

    def set_lr(self, lr):
        """learning-rate schedulers (training/train.py:303-310 `get_scheduler`) call this between steps; inside an accumulation
        window the value at the closing call is the one the optimizer uses"""
        self.lr = float(lr)

    def compute_stream(self):
        """the CU-masked stream the step runs on while a gradient exchange is active (None: the caller's current stream)"""
        if self.exchange is None or self.reserve_cus <= 0:
            return None
        if self._masked_stream is None:
            h = C.c_void_p()
            _lib.check(_lib.load().showo_stream_create_cu_mask(self.reserve_cus, C.byref(h)), "showo_stream_create_cu_mask")
            self._masked_handle = h
            self._masked_stream = torch.cuda.ExternalStream(h.value)
        return self._masked_stream

    def logging_means(self, losses, mask_prob=None):
        """The reference gathers four tensors per step for logging (training/train.py:603-610: accelerator.gather of the three losses
        and the masking rate, each repeated batch-size times, then .mean() = the mean over ranks).  Here that is ONE all-reduce of a
        4-vector, issued next to the gradient buckets; returns a device tensor [loss_t2i, loss_lm, loss_mmu, masking_rate] averaged
        over the ranks (no host sync).  Without a process group the inputs come back unchanged."""
        v = torch.cat([losses.detach().float().reshape(3), (mask_prob.detach().float().mean().reshape(1) if mask_prob is not None
                                                             else torch.zeros(1, device=losses.device))])
        ex = self.exchange
        if ex is None or ex.world == 1:
            return v
        ex.dist.all_reduce(v, op=ex.dist.ReduceOp.SUM, group=ex.group)
        return v / ex.world

    def set_loss_rows(self, loss_rows):
        """switch the loss head between "all" and "labelled" rows for the following step() calls (same validation as the constructor)"""
        self._loss_rows_mode = loss_rows_mode(loss_rows)
        self.loss_rows = loss_rows

    @property
    def loss_rows_count(self):
        """(rows the loss head of the last step ran on, token rows of its batch); host ints the forward already holds"""
        rows, total = C.c_int(), C.c_int()
        _lib.check(_lib.load().showo_train_loss_rows(self.tr, C.byref(rows), C.byref(total)), "showo_train_loss_rows")
        return rows.value, total.value

    def window_losses(self):
        """device tensor [3]: the mean of the three losses over the micro-batches of the window that closed last (of the open window's
        micro-batches so far while one is open); what the reference logs per optimizer step.  No host synchronisation."""
        if self._win_sum is None:
            raise RuntimeError("Trainer.window_losses: no step has run")
        return self._win_sum if self._win_n == 1 else self._win_sum / self._win_n

    def close(self):
        """release the CU-masked compute stream (one HIP stream per Trainer that ran with reserve_cus > 0)"""
        h = getattr(self, "_masked_handle", None)
        if h is not None:
            self._masked_stream = None
            self._masked_handle = None
            try:
                _lib.call("showo_stream_destroy", h)
            except Exception:
                pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, input_ids, attention_mask, labels, batch_size_t2i, batch_size_lm, batch_size_mmu, max_seq_length):
        """one micro-batch (with gradient_accumulation_steps = 1: one optimisation step); returns its three losses, unscaled (fp32
        device tensor [3])"""
        return self._on_compute_stream(input_ids, attention_mask, labels, batch_size_t2i, batch_size_lm, batch_size_mmu, max_seq_length)

    def step_clip_vit(self, input_ids, image_features, image_start, attention_mask, labels, batch_size_t2i, batch_size_lm, batch_size_mmu,
                      max_seq_length):
        """one micro-batch of the w_clip_vit model (reference training/train_w_clip_vit.py:598-639) on the native path; needs
        Trainer(projector=True).  input_ids / labels [B, L] at full length: the last n = image_features.shape[0] sequences hold P
        placeholder columns from image_start (an int, or n ints) whose ids are never read and whose labels are the ignore id
        (training_utils.splice_image_columns builds both).  image_features [n, P, in_dim]: the frozen tower's output, no gradient.
        Order of the call: projector forward on bf16 operands (whatever inference precision the module is set to, restored afterwards)
        -> spliced forward -> head -> blocks -> image-gradient gather -> projector backward -> projector bucket -> embedding phase.
        Window, loss_rows, reserve_cus, max_grad_norm and sync_gradients behave as in step().  Returns the three unscaled losses."""
        if not self.projector:
            raise RuntimeError("Trainer.step_clip_vit needs Trainer(model, projector=True)")
        B, L = input_ids.shape
        if image_features.dim() != 3 or image_features.shape[2] != self.model.mm_projector._dims[0]:
            raise ValueError(f"image_features should be [n, P, {self.model.mm_projector._dims[0]}], got {tuple(image_features.shape)}")
        n, P = int(image_features.shape[0]), int(image_features.shape[1])
        from .training_utils import image_starts
        starts = image_starts(image_start, n)
        if n > B or any(v < 0 or v + P > L for v in starts):
            raise ValueError(f"step_clip_vit: {n} image sequences of {P} rows from columns {starts} do not fit a [{B}, {L}] batch")
        return self._on_compute_stream(input_ids, attention_mask, labels, batch_size_t2i, batch_size_lm, batch_size_mmu, max_seq_length,
                                       image=(image_features, starts))

    def projector_grads(self):
        """{state-dict key: gradient} of the four projector tensors: views of the projector's bucket (tests, logging); a frozen
        tensor's reads zero.  Empty when no projector parameter trains."""
        return dict(self._pviews)

    def _on_compute_stream(self, *args, **kw):
        ms = None
        if getattr(self, "exchange", None) is not None and self.reserve_cus > 0:
            ms = self.compute_stream()
        if ms is None:
            return self._step(*args, **kw)
        cur = torch.cuda.current_stream()
        ms.wait_stream(cur)
        with torch.cuda.stream(ms):
            out = self._step(*args, **kw)
        cur.wait_stream(ms)
        out.record_stream(cur)  # allocated on the masked stream's pool, consumed on the caller's stream
        if self._win_sum is not None:
            self._win_sum.record_stream(cur)
        return out

    def _step(self, input_ids, attention_mask, labels, batch_size_t2i, batch_size_lm, batch_size_mmu, max_seq_length, image=None):
        self._refuse_inside_ema("step")
        # model.trainer() re-uploads parameters whose (data_ptr, version) changed since the last call (load_state_dict, resume,
        # manual edits); the native AdamW below updates them through raw pointers and refreshes the engine images itself
        self.tr = self.model.trainer()
        cur = [("showo." + n, p) for n, p in self.model.showo.named_parameters()]  # assign=True loads replace the Parameter objects
        if any(bool(p.requires_grad) != self.trainable.get(n) for n, p in cur):
            raise RuntimeError("Trainer: requires_grad of model.showo's parameters changed after the Trainer was built; build a new "
                               "Trainer for the new trainable set")
        pcur = [("mm_projector." + n, p) for n, p in self.model.mm_projector.named_parameters()] if self.projector else []
        if any(bool(p.requires_grad) != self.ptrainable.get(n) for n, p in pcur):
            raise RuntimeError("Trainer: requires_grad of model.mm_projector's parameters changed after the Trainer was built; build a "
                               "new Trainer for the new trainable set")
        win = self.window
        if self._binding_key(cur, pcur) != self._bound:  # new native trainer, or a parameter's storage moved: rebuild every raw-pointer binding
            if win.is_open:
                raise RuntimeError("Trainer: the native trainer or a parameter's storage changed inside an open accumulation window; "
                                   "the partial gradient sum belongs to the old binding")
            self.params, self.pparams = cur, pcur
            self._bind()
        from .modeling_showo import sync_trainable
        # only what the native trainer was not told yet; block 0 hands its data gradient down when the projector consumes it
        sync_trainable(self.model, self.tr, self.trainable, image is not None and self._ptrains)
        tr = self.tr
        B, L = input_ids.shape
        ids = input_ids.to(torch.int64).contiguous()
        lab = labels.to(torch.int64).contiguous()
        mask = train_mask(tr, attention_mask)
        losses = torch.empty(3, dtype=torch.float32, device=ids.device)
        # the weights of the three losses are known up front here (training/train.py:600): the forward's cross-entropy pass also
        # writes d(loss)/d(logits), so the backward does not read the [B*L, V] logits again
        ex = self.exchange
        # accumulation window: the first micro-batch overwrites the gradient buffer, the others add into it; accelerate's 1 / k on the
        # micro-batch loss goes down as the loss weights, so the announced d(logits) of the forward's pass is still the one reused
        mb = MicroBatch(ids, mask, lab, B, L, (batch_size_t2i, batch_size_lm, batch_size_mmu, max_seq_length), win.scaled(self.coeffs))
        closes = win.closes
        self.sync_gradients = False
        if not win.is_first:
            _lib.call("showo_train_set_accumulate", tr, 1)
        if self._loss_rows_mode:
            _lib.call("showo_train_set_loss_rows", tr, self._loss_rows_mode)
        try:
            self._micro_backward(mb, losses, ex if closes else None, image)
        finally:
            # per call, like the announcement of the loss weights: the module's autograd path shares this native trainer and overwrites
            # (and must return the full logits: it never runs the head on the labelled rows only)
            if not win.is_first:
                _lib.call("showo_train_set_accumulate", tr, 0)
            if self._loss_rows_mode:
                _lib.call("showo_train_set_loss_rows", tr, 0)
        if win.steps == 1:
            self._win_sum, self._win_n = losses, 1
        elif win.is_first:
            self._win_sum, self._win_n = losses.clone(), 1
        else:
            self._win_sum += losses
            self._win_n += 1
        win.advance()
        if not closes:
            return losses
        if ex is not None:
            ex.finish()
        self.grad_norm = self.clip_grad_norm_(self.max_grad_norm) if self.max_grad_norm is not None else None
        self.step_count += 1
        omd = None
        if self.ema is not None:  # one EMA step per optimizer step, not per micro-batch
            omd = self.ema.advance()[1]
        if self._showo_trains:
            if omd is not None:  # announced for this launch alone: the shadows are updated from the new master values in registers
                _lib.call("showo_train_set_ema", tr, omd)
            _lib.call("showo_train_adamw_step", tr, self.lr, self.betas[0], self.betas[1], self.eps, self.wd, self.step_count, _lib.stream())
        if self._ptrains:
            self._projector_adamw()
        if omd is not None and self._pema is not None:
            self._pema.update(omd, self._pmodes)
        self.sync_gradients = True
        return losses

    def _projector_adamw(self):
        """torch.optim.AdamW on the projector's trainable tensors (reference training/train_w_clip_vit.py:226-239: names containing
        `bias` take no decay), then their bf16 images go to the HIP projector from the updated masters -- what mark_weights_dirty()
        would make the next forward do, without its host wait"""
        for n, p in self.pparams:
            if not self.ptrainable[n]:
                continue
            _lib.call("showo_adamw", p.data_ptr(), self._pviews[n].data_ptr(), self.m[n].data_ptr(), self.v[n].data_ptr(), p.numel(),
                      self.lr, self.betas[0], self.betas[1], self.eps, 0.0 if "bias" in n else self.wd, self.step_count, _lib.stream())
            self._projector_refresh([n])

    def _projector_refresh(self, names):
        """the HIP projector's images of these tensors, from masters that were rewritten through raw pointers"""
        mm = self.model.mm_projector
        for n, p in self.pparams:
            if n not in names:
                continue
            if getattr(mm, "_proj", None) is not None and mm._versions is not None:
                k = n[len("mm_projector."):]
                _lib.call("showo_projector_load", mm._proj, k.encode(), p.data_ptr(), p.numel(), _lib.stream())
                mm._versions[k] = (p.data_ptr(), p._version)
            else:
                mm.mark_weights_dirty()

    def _projector_backward(self, tr, mm, n, P, ex):
        """image-gradient gather -> projector backward into the projector's bucket (adding inside a window) -> its collective"""
        acc = 0 if self.window.is_first else 1
        if n * P > 0:
            numel = n * P * mm._dims[1]
            g = getattr(self, "_img_grad", None)
            if g is None or g.numel() != numel or g.device != self._pgrad.device:  # kept between steps: the batch geometry rarely changes
                g = self._img_grad = torch.empty(numel, dtype=torch.float32, device=self._pgrad.device)
            _lib.call("showo_train_image_grad", tr, _lib.ptr(g), numel, _lib.stream())
            # a frozen tensor passes NULL: its gradient is neither computed nor written, in or outside a window, so its slot -- part of
            # the exchange bucket and of the clipping norm -- reads zero from the buffer's creation on
            v = [self._pviews[k].data_ptr() if self.ptrainable[k] else None for k in PROJECTOR_KEYS]
            _lib.call("showo_projector_backward_acc", mm._proj, _lib.ptr(g), n * P, None, v[0], v[1], v[2], v[3], acc, _lib.stream())
        elif not acc:
            self._pgrad.zero_()  # a micro-batch without image rows opens the window: the projector's gradient starts from zero
        if ex is not None:
            ex.launch(self._pbucket)

    def _micro_backward(self, mb, losses, ex, image=None):
        """forward + backward of one MicroBatch; ex: the exchange whose bucket collectives are launched as the buckets finish (None:
        no exchange -- no process group, or a micro-batch that does not close its window).  image: (features [n, P, in_dim], starts)
        of step_clip_vit -- the projector's rows are spliced into layer 0's input"""
        if image is None:
            return self._forward_backward(mb, losses, ex, None)
        mm = self.model.mm_projector
        feats, starts = image
        n, P = int(feats.shape[0]), int(feats.shape[1])
        prev = int(getattr(mm, "_precision", 0))
        if prev:
            mm.set_precision(0)  # training differentiates the bf16-operand forward
        try:
            rows = start = None
            if n * P > 0:
                rows = mm._hip_forward(feats.detach().float()).contiguous()
                start = torch.tensor(starts, dtype=torch.int32).to(mb.ids.device, non_blocking=True)
            return self._forward_backward(mb, losses, ex, SplicedImage(mm, rows, start, n, P))
        finally:
            if prev:
                mm.set_precision(prev)

    def _forward_backward(self, mb, losses, ex, sp):
        """the native calls of one micro-batch, in order; sp: the SplicedImage of step_clip_vit, or None"""
        tr, s = self.tr, _lib.stream
        nL = self.model.arch["num_hidden_layers"]
        ids, mask, lab = _lib.ptr(mb.ids), _lib.ptr(mb.mask), _lib.ptr(mb.labels)
        _lib.call("showo_train_set_loss_weights", tr, *mb.w, 1)
        try:  # ONE scope for the announcement: a forward that raises must withdraw it too
            try:
                if sp is None:
                    _lib.call("showo_train_forward", tr, ids, mask, lab, mb.B, mb.L, *mb.split, None, _lib.ptr(losses), s())
                else:
                    _lib.call("showo_train_forward_spliced", tr, ids, _lib.ptr(sp.rows), _lib.ptr(sp.start), sp.n, sp.P, mask, lab, mb.B, mb.L,
                              *mb.split, None, _lib.ptr(losses), s())
            finally:
                _lib.call("showo_trainer_use_intervals", tr, None, None)
            # mb.labels is this step's own contiguous copy / view and is not written between the forward above and this call: the d(logits)
            # of the forward's cross-entropy pass is reused only for the SAME forward (every forward invalidates it), pointer, split and weights.
            _lib.call("showo_train_backward_head", tr, lab, *mb.split, *mb.w, s())
        finally:
            # the announcement is per step: a later forward with labels outside Trainer.step (the module's autograd path, an eval loop)
            # must not write the T x Vp d(logits) tensor (1.3 GB at the stage-1 batch) for a backward that never comes
            _lib.call("showo_train_set_loss_weights", tr, 0.0, 0.0, 0.0, 0)
        # frozen tensors: a wholly frozen bucket is not exchanged (a partly frozen one goes on the wire with its zeros), and the
        # backward stops at the lowest phase anything needs
        bt = self._bucket_trains
        lo = 0 if bt[0] else next((i for i in range(nL) if bt[1 + i]), nL)
        through = sp is not None and self._ptrains and sp.n * sp.P > 0  # the projector consumes block 0's data gradient
        if through:
            lo = 0
        if ex is not None and bt[nL + 1]:
            ex.launch(nL + 1)
        for i in range(nL - 1, lo - 1, -1):
            _lib.call("showo_train_backward_layer", tr, i, s())
            if ex is not None and bt[i + 1]:
                ex.launch(i + 1)  # the collective of block i overlaps the backward of block i - 1
        if self._ptrains:  # (a micro-batch without image rows contributes nothing; its bucket still goes on the wire)
            self._projector_backward(tr, sp.projector if sp is not None else None, sp.n if through else 0, sp.P if through else 0, ex)
        if bt[0]:
            _lib.call("showo_train_backward_embed", tr, s())
            if ex is not None:
                ex.launch(0)

    def clip_grad_norm_(self, max_norm):
        """torch.nn.utils.clip_grad_norm_ over the flat gradient buffer (reference training/train.py:614-615
        `accelerator.clip_grad_norm_(model.parameters(), max_grad_norm)`): g *= max_norm / (||g||_2 + 1e-6) when that is < 1.
        ONE fixed-order HIP reduction over the library's flat gradient buffer + a scale pass that reads the coefficient from device
        memory (csrc/train_kernels.hip showo_grad_clip_norm): no ATen arithmetic, no host synchronisation, bit-reproducible.
        Returns the total norm (device scalar)."""
        flat = self.buckets if self._pbucket is None else self.buckets[:self._pbucket]  # the library's flat buffer
        b0, bl = flat[0], flat[-1]
        n = (bl.data_ptr() + bl.numel() * 4 - b0.data_ptr()) // 4
        if sum(b.numel() for b in flat) != n:
            raise RuntimeError("gradient buckets are not one contiguous range")
        if getattr(self, "_clip_ws", None) is None:
            self._clip_ws = torch.empty(2 * _lib.load().showo_grad_clip_ws_doubles(), dtype=torch.float64, device=b0.device)
        out2 = torch.empty(2, dtype=torch.float32, device=b0.device)
        if self._pbucket is not None:  # ONE norm over the Show-o and projector gradients (the reference clips model.parameters())
            _lib.call("showo_grad_clip_norm2", b0.data_ptr(), n, self._pgrad.data_ptr(), self._pgrad.numel(), float(max_norm),
                      _lib.ptr(self._clip_ws), _lib.ptr(out2), _lib.stream())
            return out2[0]
        _lib.call("showo_grad_clip_norm", b0.data_ptr(), n, float(max_norm), _lib.ptr(self._clip_ws), _lib.ptr(out2), _lib.stream())
        return out2[0]
