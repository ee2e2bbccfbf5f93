"""Training-step input construction on the device -- the hot-path half of the reference's `training/utils.py`
(`mask_or_random_replace_tokens` :77-154, `get_loss_weight` :73-74) and the batch assembly of `training/train.py:466-585`
(`prepare_inputs_and_labels` + the three task flows), SURVEY.md §8a row T1.

Same names, arguments and return values as the reference.  The masking itself is ONE HIP kernel (`showo_mask_tokens`:
rank-select of the noise row out of LDS) instead of rand -> argsort -> compare -> two torch.where; torch is used for the
random draws (so a seeded run consumes the device generator exactly like the reference: `rand(B)` then `rand(B, N)`) and
for evaluating the caller's `mask_schedule` callable.  `build_training_batch` returns the per-row visibility intervals
(`IntervalMask`) instead of the [B,1,L,L] fp32 masks: the training engine and `Showo.forward` consume them directly.
"""
import math
import random

import torch

from . import _lib
from . import prompting_utils as _pu


def _cfg_get(section, key, default=None):
    """`config.training.get(key, default)` for OmegaConf nodes, dicts and plain namespaces alike"""
    if hasattr(section, "get"):
        return section.get(key, default)
    return getattr(section, key, default)


def get_loss_weight(t, mask, min_val=0.3):
    return 1 - (1 - mask) * ((1 - t) * (1 - min_val))[:, None]


def mask_or_random_replace_tokens(image_tokens, mask_id, config, mask_schedule, is_train=True, noise=None):
    """reference training/utils.py:77-154.  `noise=(timesteps [B], rand [B, N])` injects the two random draws (parity tests);
    by default they are drawn from the device generator in the reference's order."""
    if not image_tokens.is_cuda:
        raise RuntimeError("show-o_amd masks tokens on the GPU: move image_tokens to the device (no CPU path exists)")
    tr = config.training
    batch_size, seq_len = image_tokens.shape
    dev = image_tokens.device
    tokens = image_tokens.to(torch.int64).contiguous()
    ratios = _cfg_get(tr, "eval_mask_ratios", None)
    if not is_train and ratios:
        mask_prob = torch.tensor(random.choices(list(ratios), k=batch_size), device=dev)
    else:
        timesteps = noise[0].to(dev) if noise is not None else torch.rand(batch_size, device=dev)
        mask_prob = mask_schedule(timesteps)
        mask_prob = mask_prob.clip(tr.min_masking_rate)
    num_token_masked = (seq_len * mask_prob).round().clamp(min=1)

    region_prob = _cfg_get(tr, "mask_contiguous_region_prob", None)
    contiguous = False if region_prob is None else random.random() < region_prob

    input_ids = torch.empty_like(tokens)
    labels = torch.empty_like(tokens)
    mask = torch.empty((batch_size, seq_len), dtype=torch.uint8, device=dev)
    # `config.training.get("noise_type", "mask")` is truthy for every non-empty string, so the reference always takes the
    # mask-token branch for the inputs (:132-133); "random_replace" only changes the labels / loss weights (:143-147)
    noise_type = _cfg_get(tr, "noise_type", "mask")
    if not noise_type:
        raise ValueError(f"noise_type {noise_type} not supported")
    predict_all = bool(_cfg_get(tr, "predict_all_tokens", False)) or noise_type == "random_replace"
    if not contiguous:
        u = noise[1].to(dev) if noise is not None else torch.rand(batch_size, seq_len, device=dev)
        u = u.to(torch.float32).contiguous()
        n = num_token_masked.to(torch.int32).contiguous()
        _lib.call("showo_mask_tokens", _lib.ptr(tokens), _lib.ptr(u), _lib.ptr(n), None, 0, batch_size, seq_len, int(mask_id), -100,
                  int(predict_all), _lib.ptr(input_ids), _lib.ptr(labels), _lib.ptr(mask), _lib.stream())
    else:
        resolution = int(seq_len ** 0.5)
        rects = []
        for k in num_token_masked.tolist():  # same host RNG calls, in the same order, as the reference loop (:109-122)
            k = int(k)
            h = random.randint(math.ceil(k / resolution), min(resolution, k))
            h = min(h, resolution)
            w = min(math.ceil(k / h), resolution)
            y0 = random.randint(0, resolution - h)
            x0 = random.randint(0, resolution - w)
            rects.append([y0, y0 + h, x0, x0 + w])
        rect = torch.tensor(rects, dtype=torch.int32, device=dev)
        _lib.call("showo_mask_tokens", _lib.ptr(tokens), None, None, _lib.ptr(rect), resolution, batch_size, seq_len, int(mask_id),
                  -100, int(predict_all), _lib.ptr(input_ids), _lib.ptr(labels), _lib.ptr(mask), _lib.stream())
    loss_weight = get_loss_weight(mask_prob, mask.long()) if predict_all else None
    return input_ids, labels, loss_weight, mask_prob


def build_training_batch(uni_prompting, config, mask_id, mask_schedule, image_tokens_t2i, texts_t2i, texts_lm, image_tokens_mmu,
                         texts_mmu, is_train=True, noise=None):
    """The mixed batch of one optimisation step (reference training/train.py:466-585): t2i rows (MLM-corrupted image tokens
    behind the caption), lm rows padded to the same length, mmu rows (image prefix + caption).

    image_tokens_* are `vq_model.get_code(...)` outputs ALREADY offset by len(tokenizer) (train.py:475-476, 555-556).
    Returns input_ids [B,L], labels [B,L], ONE IntervalMask for the whole batch (t2i rows with rm_pad_in_image, lm rows,
    mmu rows, in that order -- what the reference concatenates as dense masks, train.py:522-577), mask_prob [b_t2i], and
    the batch sizes (b_t2i, b_lm, b_mmu) `Showo.forward` / `Trainer.step` need."""
    sp = uni_prompting.sptids_dict
    pad, soi, eoi = int(sp['<|pad|>']), int(sp['<|soi|>']), int(sp['<|eoi|>'])
    ids_img, lab_img, _, mask_prob = mask_or_random_replace_tokens(image_tokens_t2i, mask_id, config, mask_schedule, is_train, noise)
    ids_t2i, _, lab_t2i = uni_prompting((texts_t2i, ids_img, lab_img), 't2i')
    iv_t2i = _pu.intervals_predict_next(ids_t2i, pad_id=pad, soi_id=soi, eoi_id=eoi, rm_pad_in_image=True)
    dev = ids_t2i.device
    ids_lm, _, lab_lm = uni_prompting((texts_lm, ids_t2i.shape[-1]), 'lm')
    ids_lm, lab_lm = ids_lm.to(dev), lab_lm.to(dev)
    iv_lm = _pu.intervals_predict_next(ids_lm, pad_id=pad, soi_id=soi, eoi_id=eoi)
    ids_mmu, _, lab_mmu = uni_prompting((image_tokens_mmu, texts_mmu), 'mmu')
    iv_mmu = _pu.intervals_for_mmu(ids_mmu, eoi_id=eoi)
    input_ids = torch.cat([ids_t2i, ids_lm, ids_mmu], dim=0)
    labels = torch.cat([lab_t2i, lab_lm, lab_mmu], dim=0)
    flag = iv_t2i.flag | iv_lm.flag  # "needs more than two runs" of either predict-next block (mmu rows never do)
    mask = _pu.IntervalMask(torch.cat([iv_t2i.iv, iv_lm.iv, iv_mmu.iv], dim=0), flag)
    return input_ids, labels, mask, mask_prob, (ids_t2i.shape[0], ids_lm.shape[0], ids_mmu.shape[0])


def image_starts(image_start, n):
    """`image_start` of splice_image_columns / Trainer.step_clip_vit as n host ints: one integer (a Python or numpy integer, a 0-d
    tensor) for every sequence, or n of them (a sequence or a 1-d tensor: read back with one `.tolist()`)"""
    import numbers
    if torch.is_tensor(image_start):
        image_start = image_start.tolist()
    if isinstance(image_start, numbers.Integral):
        return [int(image_start)] * n
    starts = [int(v) for v in image_start]
    if len(starts) != n:
        raise ValueError(f"image_start: {len(starts)} starts for {n} image sequences")
    return starts


def splice_image_columns(input_ids_mmu, labels_mmu, image_start, P, fill_id, ignore_id=-100):
    """Full-length ids and labels of the mmu sequences for Trainer.step_clip_vit: P columns inserted at column `image_start` (an int,
    or one int per sequence), ids filled with `fill_id` (never read: the projector's rows stand there), labels with `ignore_id`.
    The layout the reference gets by concatenating embeddings and labels around the image rows (training/train_w_clip_vit.py:538-549
    for llava_pretrain, image_start = 2; :577-589 for llava_tuning, image_start = 2 + SYSTEM_PROMPT_LEN).
    input_ids_mmu, labels_mmu: [n, Lt] without the image columns.  Returns (ids [n, Lt + P], labels [n, Lt + P]), int64."""
    ids, lab = input_ids_mmu.long(), labels_mmu.long()
    if ids.dim() != 2 or ids.shape != lab.shape:
        raise ValueError(f"splice_image_columns: ids {tuple(ids.shape)} and labels {tuple(lab.shape)} must be the same [n, Lt]")
    n, Lt = ids.shape
    P = int(P)
    starts = image_starts(image_start, n)
    if P < 0 or any(v < 0 or v > Lt for v in starts):
        raise ValueError(f"splice_image_columns: image_start {image_start!r} does not fit {n} sequences of {Lt} columns")
    st = torch.tensor(starts, dtype=torch.long, device=ids.device).view(n, 1)
    col = torch.arange(Lt + P, device=ids.device).view(1, Lt + P)
    image = (col >= st) & (col < st + P)
    src = (col - P * (col >= st + P).long()).clamp(0, max(Lt - 1, 0))  # the text column a non-image column comes from
    if Lt == 0:
        return ids.new_full((n, P), fill_id), lab.new_full((n, P), ignore_id)
    return (torch.where(image, ids.new_full((), fill_id), ids.gather(1, src.expand(n, -1))),
            torch.where(image, lab.new_full((), ignore_id), lab.gather(1, src.expand(n, -1))))


def labelled_rows(labels, batch_size_t2i, batch_size_lm, batch_size_mmu, max_seq_length):
    """The logits rows that enter one of the three losses of `Showo.forward` (reference models/modeling_showo.py:83-98), as
    ascending int64 indices into the flattened [B * L] rows.  Plain torch, works on CPU tensors: the stated rule of the row census
    that `Trainer(loss_rows="labelled")` runs on the device (showo_ce_rows_compact).

    Row (b, l) is labelled when
      * b < batch_size_t2i, l > max_seq_length and labels[b, l] != -100         (loss_t2i: logits[:b_t2i, max_seq_length + 1:]), or
      * l < L - 1, labels[b, l + 1] != -100 and b is an lm row                    (loss_lm: logits[b_t2i:b_t2i + b_lm, :-1]), or
      * l < L - 1, labels[b, l + 1] != -100 and b is one of the last batch_size_mmu rows (loss_mmu: logits[-b_mmu:, :-1]);
        batch_size_mmu == 0 selects the WHOLE batch there (`logits[-0:]`), as the reference's slicing does."""
    B, L = labels.shape
    valid = labels != -100
    b = torch.arange(B, device=labels.device)[:, None]
    l = torch.arange(L, device=labels.device)[None, :]
    t2i = (b < batch_size_t2i) & (l >= max_seq_length + 1) & valid
    nxt = torch.zeros_like(valid)
    nxt[:, :-1] = valid[:, 1:]
    in_lm = (b >= batch_size_t2i) & (b < batch_size_t2i + batch_size_lm)
    in_mmu = torch.ones_like(in_lm) if batch_size_mmu == 0 else (b >= B - batch_size_mmu)
    live = t2i | (nxt & (in_lm | in_mmu))
    return torch.nonzero(live.reshape(-1)).reshape(-1).to(torch.int64)


# ---------------------------------------------------------------------------------------------------------------
# EMA of the weights (reference models/training_utils.py:61-296, itself adapted from torch-ema)
# ---------------------------------------------------------------------------------------------------------------
EMA_SCALAR_KEYS = ("decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power")


def _ema_native_pairs(shadows, params):
    """True when every (shadow, parameter) pair can go through the segment-table kernel: contiguous fp32 CUDA tensors of one
    device and equal element counts"""
    if not shadows or len(shadows) != len(params):
        return False
    dev = shadows[0].device
    if dev.type != "cuda":
        return False
    for s, p in zip(shadows, params):
        if s.device != dev or p.device != dev or s.dtype != torch.float32 or p.dtype != torch.float32:
            return False
        if not s.is_contiguous() or not p.is_contiguous() or s.numel() != p.numel():
            return False
    return True


class EmaTable:
    """showo_ema_table (include/showo_hip.h): one update / swap launch over pairs of contiguous fp32 CUDA tensors.  The table holds raw
    pointers: the caller keeps the tensors alive and builds a new table when storage moves.  dst16 / dst32: optional lists of tensors
    (or None entries) that swap() also writes the bf16 cast / fp32 copy of the new parameter values to."""

    def __init__(self, shadows, params, dst16=None, dst32=None):
        import ctypes as C
        k = len(shadows)
        arr = lambda ts: (C.c_void_p * k)(*[(t.data_ptr() if t is not None and t.numel() else None) for t in ts])
        self.count = k
        self.device = shadows[0].device
        h = C.c_void_p()
        _lib.call("showo_ema_table_create", arr(shadows), arr(params), (C.c_int64 * k)(*[int(s.numel()) for s in shadows]), k,
                  arr(dst16) if dst16 is not None else None, arr(dst32) if dst32 is not None else None, C.byref(h))
        self._h = h

    def update(self, one_minus_decay, modes=None):
        import ctypes as C
        m = (C.c_int * self.count)(*[int(bool(v)) for v in modes]) if modes is not None else None
        with torch.cuda.device(self.device):
            _lib.call("showo_ema_table_update", self._h, m, float(one_minus_decay), _lib.stream())

    def swap(self):
        with torch.cuda.device(self.device):
            _lib.call("showo_ema_table_swap", self._h, _lib.stream())

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            _lib.load().showo_ema_table_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EMA:
    """Exponential moving average of a model's weights; the reference class's constructor, attributes, methods and `state_dict`
    keys.  `shadow_params[i]` follows `parameters[i]`:  shadow -= (1 - decay_t) * (shadow - parameter)  once per `step()`, with the
    decay of `get_decay`; a parameter that does not require grad is copied instead.

    `Trainer(model, ema=...)` owns one of these and updates it inside its AdamW launch; this class alone serves any list of tensors."""

    def __init__(self, parameters, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3,
                 model_cls=None, model_config=None, **kwargs):
        """decay: the ceiling of the decay factor; min_decay: its floor; update_after_step: steps before averaging starts (the shadows
        copy the parameters until then: decay 0); use_ema_warmup / inv_gamma / power: decay_t = 1 - (1 + t / inv_gamma) ** -power
        instead of (1 + t) / (10 + t).  model_cls / model_config: what `save_pretrained` rebuilds the model from
        (`model_cls.from_config(model_config)`; for a Showo, `dict(model.config, **model.arch)`)."""
        self.shadow_params = [p.clone().detach() for p in parameters]
        self.temp_stored_params = None
        self.decay, self.min_decay, self.update_after_step = decay, min_decay, update_after_step
        self.use_ema_warmup, self.inv_gamma, self.power = use_ema_warmup, inv_gamma, power
        self.optimization_step = 0
        self.cur_decay_value = None  # set by step()
        self.model_cls, self.model_config = model_cls, model_config
        self._table, self._table_key = None, None

    # ---- the decay schedule
    def get_decay(self, optimization_step):
        t = optimization_step - self.update_after_step - 1
        if t <= 0:
            return 0.0
        warm = 1 - (1 + t / self.inv_gamma) ** -self.power if self.use_ema_warmup else (1 + t) / (10 + t)
        return max(min(warm, self.decay), self.min_decay)

    def advance(self):
        """count one optimization step and return (decay, 1 - decay) of it: the bookkeeping half of step(), for a caller that
        updates the shadows itself (the Trainer's fused AdamW launch)"""
        self.optimization_step += 1
        self.cur_decay_value = self.get_decay(self.optimization_step)
        return self.cur_decay_value, 1 - self.cur_decay_value

    # ---- the update
    @torch.no_grad()
    def step(self, parameters):
        """One EMA step of every shadow against `parameters` (same order as at construction).

        When every shadow / parameter pair is a contiguous fp32 CUDA tensor this is ONE launch over a segment table (cached on the
        data pointers and `requires_grad` flags; csrc/ema.hip), with the reference's three fp32 roundings per element.  Anything else
        (CPU tensors, other dtypes after `to(dtype=...)`, non-contiguous tensors) runs the same expression in torch.
        Unlike the reference this does not call `torch.cuda.empty_cache()`: that is a device-wide stall with no effect on results."""
        parameters = list(parameters)
        _, one_minus_decay = self.advance()
        if _ema_native_pairs(self.shadow_params, parameters):
            flags = tuple(not p.requires_grad for p in parameters)
            self._native_table(parameters).update(one_minus_decay, flags)
            return
        for s, p in zip(self.shadow_params, parameters):
            if p.requires_grad:
                s.sub_(one_minus_decay * (s - p))
            else:
                s.copy_(p)

    def _native_table(self, parameters):
        key = tuple((s.data_ptr(), p.data_ptr(), s.numel(), bool(p.requires_grad)) for s, p in zip(self.shadow_params, parameters))
        if self._table is None or self._table_key != key:
            if self._table is not None:
                torch.cuda.synchronize(self._table.device)  # a launch over the old table may still be in flight
                self._table.close()
            self._table = EmaTable(self.shadow_params, [p.detach() for p in parameters])
            self._table_key = key
        return self._table

    # ---- moving the averages around
    def copy_to(self, parameters):
        """write the averaged weights into `parameters`.  On the parameters of a `Showo` follow it with `model.mark_weights_dirty()`:
        a write through `.data` does not bump the version counter the engine watches (the rule for every manual edit)."""
        for s, p in zip(self.shadow_params, list(parameters)):
            p.data.copy_(s.to(p.device).data)

    def to(self, device=None, dtype=None):
        """move the shadows; `dtype` applies to floating-point shadows only.  Shadows that are not fp32 CUDA tensors afterwards take
        the torch path of step()."""
        self.shadow_params = [s.to(device=device, dtype=dtype) if s.is_floating_point() else s.to(device=device) for s in self.shadow_params]

    def store(self, parameters):
        """keep a CPU copy of `parameters` for restore() (validate with copy_to() in between)"""
        self.temp_stored_params = [p.detach().cpu().clone() for p in parameters]

    def restore(self, parameters):
        if self.temp_stored_params is None:
            raise RuntimeError("This ExponentialMovingAverage has no `store()`ed weights to `restore()`")
        for c, p in zip(self.temp_stored_params, parameters):
            p.data.copy_(c.data)
        self.temp_stored_params = None

    # ---- state
    def state_dict(self):
        """references, not copies (the torch convention)"""
        sd = {k: getattr(self, k) for k in EMA_SCALAR_KEYS}
        sd["shadow_params"] = self.shadow_params
        return sd

    def load_state_dict(self, state_dict):
        import copy
        sd = copy.deepcopy(state_dict)
        self.decay = sd.get("decay", self.decay)
        if self.decay < 0.0 or self.decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        checks = (("min_decay", float), ("optimization_step", int), ("update_after_step", int), ("use_ema_warmup", bool),
                  ("inv_gamma", (float, int)), ("power", (float, int)))
        for k, kind in checks:
            setattr(self, k, sd.get(k, getattr(self, k)))
            if not isinstance(getattr(self, k), kind):
                raise ValueError(f"Invalid {k}")
        shadows = sd.get("shadow_params", None)
        if shadows is not None:
            self.shadow_params = shadows
            if not isinstance(shadows, list):
                raise ValueError("shadow_params must be a list")
            if not all(isinstance(s, torch.Tensor) for s in shadows):
                raise ValueError("shadow_params must all be Tensors")

    # ---- a model directory with the averaged weights
    def save_pretrained(self, path):
        """writes a directory that `model_cls.from_pretrained(path)` loads with the shadows as its weights; the EMA scalars go into its
        config.json under their state_dict names"""
        if self.model_cls is None:
            raise ValueError("`save_pretrained` can only be used if `model_cls` was defined at __init__.")
        if self.model_config is None:
            raise ValueError("`save_pretrained` can only be used if `model_config` was defined at __init__.")
        dev = self.shadow_params[0].device if self.shadow_params else "cpu"
        model = self.model_cls.from_config(self.model_config, device=dev)
        model.register_to_config(**{k: getattr(self, k) for k in EMA_SCALAR_KEYS})
        self.copy_to(model.parameters())
        model.save_pretrained(path)

    @classmethod
    def from_pretrained(cls, path, model_cls):
        _, scalars = model_cls.load_config(path, return_unused_kwargs=True)
        model = model_cls.from_pretrained(path)
        config = {k: v for k, v in model._config_dict().items() if k not in scalars}
        ema = cls(model.parameters(), model_cls=model_cls, model_config=config)
        ema.load_state_dict(scalars)
        return ema
