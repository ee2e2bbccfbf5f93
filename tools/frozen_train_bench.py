"""What does training with frozen parameters cost, against training everything?  Three pairs, each timed with device events after a
warm-up, the two forms of a pair alternating step by step in one process (so clocks and the allocator's state are shared):

  (a) llava_pretrain: the LLaVA-pretrain stage of the reference (training/train_w_clip_vit.py:200-214, und_type "llava_pretrain")
      as its unchanged loop runs it: Showo.forward(input_embeddings=..., labels=...) -> w_t2i loss_t2i + w_lm loss_lm + w_mmu
      loss_mmu -> backward -> torch.optim.AdamW built over the `requires_grad` parameters with the reference's two groups
      (train_w_clip_vit.py:226-239).  Split (2, 2, 10); an mmu row is [<|mmu|>, <|soi|>] + 576 projector rows + [<|eoi|>] + 192
      text ids (max_seq_length 512 - (576 - 256), :348), so L = 771, the length of a t2i row (512 text + 256 image + 3 specials) too.
      All trainable against mm_projector only.  The CLIP tower stays outside the timed region (random features).
  (b) stage1_lower_frozen: Trainer.step at the stage-1 batch of bench_train.py (15 t2i + 4 lm + 10 mmu, VQ codes fixed), all
      trainable against the embedding + blocks 0-11 frozen.
  (c) linear_probe: the same Trainer.step batch, all trainable against lm_head.weight / lm_head.bias only.

Prints one JSON line: per pair the mean GPU ms per step of both forms and the saving.

    python tools/frozen_train_bench.py [--steps 4] [--warmup 2] [--pairs a,b,c]"""
import argparse
import gc
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

NO_DECAY = ["bias", "layer_norm.weight", "mlm_ln.weight", "embeddings.weight"]  # reference training/train.py:211
COEFFS = (1.0, 0.1, 1.0)


def _adamw(model, lr):
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    return torch.optim.AdamW([{"params": [p for n, p in named if not any(x in n for x in NO_DECAY)], "weight_decay": 0.01},
                              {"params": [p for n, p in named if any(x in n for x in NO_DECAY)], "weight_decay": 0.0}],
                             lr=lr, betas=(0.9, 0.999), eps=1e-8)


def _alternate(steps, warmup, fa, fb):
    """mean GPU ms per call of fa and fb, called alternately (warm-up calls untimed)"""
    for _ in range(warmup):
        fa()
        fb()
    ev = {k: [] for k in "ab"}
    for _ in range(steps):
        for k, f in (("a", fa), ("b", fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    return [sum(e0.elapsed_time(e1) for e0, e1 in ev[k]) / steps for k in "ab"]


def _pair(name, ms_all, ms_frozen, what):
    return {"pair": name, "frozen": what, "ms_all_trainable": round(ms_all, 2), "ms_frozen": round(ms_frozen, 2),
            "saving_frac": round(1.0 - ms_frozen / ms_all, 4)}


def pair_llava(steps, warmup):
    from showo_amd import synthetic
    from showo_amd.prompting_utils import create_attention_mask_for_mmu_vit
    bt, bl, bm, L, n_img = 2, 2, 10, 771, 576
    B = bt + bl + bm
    torch.manual_seed(0)
    models = []
    for frozen in (False, True):
        m = synthetic.random_init_showo(max_batch=B, max_seq=L, w_clip_vit=True).train()
        if frozen:
            m.showo.requires_grad_(False)  # train_w_clip_vit.py:200-214: only mm_projector trains
        models.append((m, _adamw(m, 2e-3 if frozen else 1e-4)))
    uni_vocab = synthetic.SHOWO_DEMO["llm_vocab_size"]
    ids_t = torch.randint(0, uni_vocab, (bt + bl, L), device="cuda")  # t2i / lm rows: embedded ids
    ids_m = torch.randint(0, uni_vocab, (bm, L - n_img), device="cuda")  # mmu rows: 3 specials + 192 text ids around the image
    feats = torch.randn(bm, n_img, 1024, device="cuda")  # CLIP ViT penultimate features (outside the timed region)
    labels = torch.randint(0, uni_vocab, (B, L), device="cuda")
    labels[bt + bl:, :n_img + 3] = -100
    mask = create_attention_mask_for_mmu_vit(torch.zeros(B, L, device="cuda"))

    def step(m, opt):
        def f():
            opt.zero_grad(set_to_none=True)
            te = m.showo.model.embed_tokens(ids_m)
            mmu = torch.cat([te[:, :2], m.mm_projector(feats), te[:, 2:]], dim=1)
            emb = torch.cat([m.showo.model.embed_tokens(ids_t), mmu], dim=0)
            _, l1, l2, l3 = m(None, input_embeddings=emb, attention_mask=mask, labels=labels, batch_size_t2i=bt, batch_size_lm=bl,
                              batch_size_mmu=bm, max_seq_length=512)
            (COEFFS[0] * l1 + COEFFS[1] * l2 + COEFFS[2] * l3).backward()
            opt.step()
        return f

    ms = _alternate(steps, warmup, step(*models[0]), step(*models[1]))
    del models
    return _pair("llava_pretrain", ms[0], ms[1], "all of model.showo (mm_projector trains)")


def _stage1_batch():
    from showo_amd import synthetic
    from showo_amd.training_utils import build_training_batch
    from bench_train import synthetic_texts
    bt, bl, bm = 15, 4, 10
    uni = synthetic.prompting(max_text_len=128, cond_dropout_prob=0.1)
    off = len(uni.text_tokenizer)
    N, codebook = synthetic.SHOWO_DEMO["num_vq_tokens"], synthetic.SHOWO_DEMO["codebook_size"]
    cfg = type("Cfg", (), {"training": type("Training", (dict,), {"__getattr__": dict.__getitem__})(min_masking_rate=0.0)})
    rs = np.random.RandomState(4)
    torch.manual_seed(4)
    random.seed(4)
    texts_t2i, texts_lm, texts_mmu = synthetic_texts(rs, bt, bl, bm)
    codes = torch.randint(0, codebook, (bt + bm, N), device="cuda") + off
    return uni, cfg, codes, (bt, bl, bm), (texts_t2i, texts_lm, texts_mmu), build_training_batch


def pair_trainer(steps, warmup, name, freeze, what, keep=None):
    import showo_amd
    from showo_amd import synthetic
    uni, cfg, codes, (bt, bl, bm), (tt, tl, tm), build = _stage1_batch()
    torch.manual_seed(0)
    if keep is None:
        a = synthetic.random_init_showo(max_batch=bt + bl + bm, max_seq=387).train()
        ta = showo_amd.Trainer(a, lr=1e-4, coeffs=COEFFS)
    else:
        a, ta = keep
    b = synthetic.random_init_showo(max_batch=bt + bl + bm, max_seq=387).train()
    freeze(b)
    tb = showo_amd.Trainer(b, lr=1e-4, coeffs=COEFFS)
    ids, labels, mask, _, (b1, b2, b3) = build(uni, cfg, a.mask_token_id, showo_amd.cosine_schedule, codes[:bt], list(tt), list(tl),
                                               codes[bt:], list(tm))
    ms = _alternate(steps, warmup, lambda: ta.step(ids, mask, labels, b1, b2, b3, 128),
                    lambda: tb.step(ids, mask, labels, b1, b2, b3, 128))
    del tb, b
    return _pair(name, ms[0], ms[1], what), (a, ta)


def _freeze_lower(m):
    m.showo.model.embed_tokens.requires_grad_(False)
    for i in range(12):
        m.showo.model.layers[i].requires_grad_(False)


def _probe(m):
    m.showo.requires_grad_(False)
    m.showo.lm_head.requires_grad_(True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", default="a,b,c")
    a = ap.parse_args(argv)
    want = set(a.pairs.split(","))
    out = []
    if "a" in want:
        out.append(pair_llava(a.steps, a.warmup))
        gc.collect()
        torch.cuda.empty_cache()
    keep = None
    if "b" in want:
        r, keep = pair_trainer(a.steps, a.warmup, "stage1_lower_frozen", _freeze_lower, "embedding + blocks 0-11")
        out.append(r)
        gc.collect()
        torch.cuda.empty_cache()
    if "c" in want:
        r, keep = pair_trainer(a.steps, a.warmup, "linear_probe", _probe, "everything but lm_head", keep)
        out.append(r)
    print(json.dumps({"tool": "frozen_train_bench", "steps": a.steps, "warmup": a.warmup, "pairs": out}))


if __name__ == "__main__":
    main()
