"""The training step of the CLIP-ViT model (reference training/train_w_clip_vit.py:598-639), two ways, at the LLaVA-tuning geometry:
Phi-1.5, split (2, 2, 10), an mmu row = [<|mmu|>, <|soi|>] + 576 projector rows + [<|eoi|>] + 192 text ids, L = 576 + 195 = 771.

  (a) autograd: embed_tokens + mm_projector + torch.cat -> Showo.forward(input_embeddings=..., labels=...) -> weighted loss ->
      backward -> torch.optim.AdamW over the `requires_grad` parameters with the reference's two groups (train_w_clip_vit.py:226-239)
  (b) native:   Trainer(model, projector=True).step_clip_vit(...) -- splice kernel, phased backward, leave-out table scatter,
      projector backward, fused AdamW

Both run all-trainable and projector-only (und_type "llava_pretrain", train_w_clip_vit.py:201-214).  The two paths of a pair
alternate call by call in ONE process, the order swapping every round; every call is timed with device events after a warm-up;
reported: median, min and max GPU ms per step and the ratio of the medians.  The CLIP tower stays outside the timed region (random
features).  Writes profiles/clip_vit_train_bench.json and prints the same JSON line.

    python tools/clip_vit_train_bench.py [--steps 6] [--warmup 2] [--modes all,projector] [--out profiles/clip_vit_train_bench.json]"""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

NO_DECAY = ["bias", "layer_norm.weight", "mlm_ln.weight", "embeddings.weight"]  # reference training/train_w_clip_vit.py:227
COEFFS = (1.0, 0.1, 1.0)
BT, BL, BM, L, N_IMG, IMG_START = 2, 2, 10, 771, 576, 2


def _adamw(model, lr):
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    return torch.optim.AdamW([{"params": [p for n, p in named if not any(x in n for x in NO_DECAY)], "weight_decay": 0.01},
                              {"params": [p for n, p in named if any(x in n for x in NO_DECAY)], "weight_decay": 0.0}],
                             lr=lr, betas=(0.9, 0.999), eps=1e-8)


def _alternate(steps, warmup, fa, fb):
    """GPU ms of every timed call of fa and fb: warm-up calls untimed, then `steps` rounds, (a, b) on even rounds and (b, a) on odd"""
    for _ in range(warmup):
        fa()
        fb()
    ev = {"a": [], "b": []}
    for r in range(steps):
        order = (("a", fa), ("b", fb)) if r % 2 == 0 else (("b", fb), ("a", fa))
        for k, f in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ev.items()}


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 2), "min_ms": round(min(ms), 2), "max_ms": round(max(ms), 2), "calls": len(ms)}


def run_mode(mode, steps, warmup):
    import showo_amd
    from showo_amd import synthetic
    from showo_amd.prompting_utils import create_attention_mask_for_mmu_vit
    from showo_amd.training_utils import splice_image_columns
    B = BT + BL + BM
    lr = 2e-3 if mode == "projector" else 1e-4
    torch.manual_seed(0)
    models = []
    for _ in range(2):
        m = synthetic.random_init_showo(max_batch=B, max_seq=L, w_clip_vit=True).train()
        if mode == "projector":
            m.showo.requires_grad_(False)
        models.append(m)
    ma, mb = models
    opt = _adamw(ma, lr)
    tr = showo_amd.Trainer(mb, lr=lr, coeffs=COEFFS, projector=True)
    vocab = synthetic.SHOWO_DEMO["llm_vocab_size"]
    ids_t = torch.randint(0, vocab, (BT + BL, L), device="cuda")
    ids_m = torch.randint(0, vocab, (BM, L - N_IMG), device="cuda")
    feats = torch.randn(BM, N_IMG, 1024, device="cuda")
    lab_t = torch.randint(0, vocab, (BT + BL, L), device="cuda")
    lab_m = torch.randint(0, vocab, (BM, L - N_IMG), device="cuda")
    lab_m[:, :3] = -100
    full_ids_m, full_lab_m = splice_image_columns(ids_m, lab_m, IMG_START, N_IMG, 0)
    ids = torch.cat([ids_t, full_ids_m], dim=0)
    labels = torch.cat([lab_t, full_lab_m], dim=0)
    mask = create_attention_mask_for_mmu_vit(torch.zeros(B, L, device="cuda"))

    def autograd_step():
        opt.zero_grad(set_to_none=True)
        te = ma.showo.model.embed_tokens(ids_m)
        mmu = torch.cat([te[:, :IMG_START], ma.mm_projector(feats), te[:, IMG_START:]], dim=1)
        emb = torch.cat([ma.showo.model.embed_tokens(ids_t), mmu], dim=0)
        _, l1, l2, l3 = ma(None, input_embeddings=emb, attention_mask=mask, labels=labels, batch_size_t2i=BT, batch_size_lm=BL,
                           batch_size_mmu=BM, max_seq_length=512)
        (COEFFS[0] * l1 + COEFFS[1] * l2 + COEFFS[2] * l3).backward()
        opt.step()

    def native_step():
        tr.step_clip_vit(ids, feats, IMG_START, mask, labels, BT, BL, BM, 512)

    ms = _alternate(steps, warmup, autograd_step, native_step)
    a, b = _stats(ms["a"]), _stats(ms["b"])
    del opt, tr, models, ma, mb
    return {"mode": "all trainable" if mode == "all" else "projector only (llava_pretrain)", "autograd": a, "native": b,
            "native_over_autograd": round(b["median_ms"] / a["median_ms"], 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--modes", default="all,projector")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_vit_train_bench.json"))
    a = ap.parse_args(argv)
    out = []
    for mode in a.modes.split(","):
        if mode not in ("all", "projector"):
            raise SystemExit(f"unknown mode {mode!r}: all | projector")
        out.append(run_mode(mode, a.steps, a.warmup))
        gc.collect()
        torch.cuda.empty_cache()
    res = {"tool": "clip_vit_train_bench", "device": torch.cuda.get_device_name(0), "geometry": {"split": [BT, BL, BM], "L": L, "image_rows": N_IMG,
           "model": "Phi-1.5 Show-o, w_clip_vit"}, "steps": a.steps, "warmup": a.warmup, "results": out}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
