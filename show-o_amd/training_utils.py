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
