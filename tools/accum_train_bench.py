"""What does a micro-batch cost inside an accumulation window, against a plain optimizer step?  Stage-1 batch of bench_train.py
(15 t2i + 4 lm + 10 mmu sequences x 387 tokens, VQ codes fixed), one MI355X, ONE process, two trainers on two models started from
the same seed.  A round is

  (A) k plain steps of Trainer(gradient_accumulation_steps=1): k forwards, backwards, AdamW steps and image refreshes;
  (B) one window of Trainer(gradient_accumulation_steps=k): k forwards and backwards (the first overwrites the gradient buffer, the
      others add into it through the accumulating kernel forms), ONE AdamW step and image refresh.

Both see the same k micro-batches.  The rounds alternate (A)(B)(A)(B)... so that clocks and the allocator's state are shared; every
leg of a round is bracketed by device events.  Reported: ms per micro-batch of both with the spread (max - min) and the standard
deviation over the timed rounds, and what (B) saves per window = the k - 1 AdamW steps + image refreshes it skips, net of what
the accumulating forms cost.  Prints one JSON line and writes it to --out.

    python tools/accum_train_bench.py [--k 4] [--rounds 4] [--warmup 2] [--out profiles/accum_train_bench.json]"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

COEFFS = (1.0, 0.1, 1.0)


def _micro_batches(k, mask_token_id):
    import showo_amd
    from showo_amd import synthetic
    from showo_amd.training_utils import build_training_batch
    from bench_train import synthetic_texts
    bt, bl, bm = 15, 4, 10
    uni = synthetic.prompting(max_text_len=128, cond_dropout_prob=0.1)
    off = len(uni.text_tokenizer)
    N, codebook = synthetic.SHOWO_DEMO["num_vq_tokens"], synthetic.SHOWO_DEMO["codebook_size"]
    cfg = type("Cfg", (), {"training": type("Training", (dict,), {"__getattr__": dict.__getitem__})(min_masking_rate=0.0)})
    out = []
    for j in range(k):  # every micro-batch draws its own texts, codes and masking, as consecutive batches of a loader do
        rs = np.random.RandomState(4 + j)
        torch.manual_seed(4 + j)
        random.seed(4 + j)
        tt, tl, tm = synthetic_texts(rs, bt, bl, bm)
        codes = torch.randint(0, codebook, (bt + bm, N), device="cuda") + off
        ids, labels, mask, _, split = build_training_batch(uni, cfg, mask_token_id, showo_amd.cosine_schedule, codes[:bt], list(tt), list(tl),
                                                           codes[bt:], list(tm))
        out.append((ids, mask, labels, tuple(split)))
    return out


def _stats(ms, k):
    per = [x / k for x in ms]
    return {"ms_per_micro_batch": round(float(np.mean(per)), 3), "spread_ms": round(float(max(per) - min(per)), 3),
            "std_ms": round(float(np.std(per)), 3), "rounds_ms_per_micro_batch": [round(x, 3) for x in per]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_train_bench.json"))
    a = ap.parse_args(argv)
    if a.k < 2 or a.rounds < 4 or a.warmup < 2:
        ap.error("--k >= 2, --rounds >= 4 and --warmup >= 2")
    import showo_amd
    from showo_amd import synthetic
    k = a.k
    models, trainers = [], []
    for steps in (1, k):
        torch.manual_seed(0)
        m = synthetic.random_init_showo(max_batch=29, max_seq=387).train()
        models.append(m)
        trainers.append(showo_amd.Trainer(m, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, coeffs=COEFFS,
                                          gradient_accumulation_steps=steps))
    batches = _micro_batches(k, models[0].mask_token_id)

    def leg(tr):
        for ids, mask, labels, (b1, b2, b3) in batches:
            tr.step(ids, mask, labels, b1, b2, b3, 128)
        assert tr.sync_gradients

    for _ in range(a.warmup):
        for tr in trainers:
            leg(tr)
    ev = [[], []]
    for _ in range(a.rounds):
        for i, tr in enumerate(trainers):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            leg(tr)
            e1.record()
            ev[i].append((e0, e1))
    torch.cuda.synchronize()
    ms = [[e0.elapsed_time(e1) for e0, e1 in ev[i]] for i in (0, 1)]
    plain, window = _stats(ms[0], k), _stats(ms[1], k)
    assert trainers[0].step_count == k * (a.warmup + a.rounds) and trainers[1].step_count == a.warmup + a.rounds
    saved = float(np.mean(ms[0]) - np.mean(ms[1]))
    out = {"tool": "accum_train_bench", "k": k, "rounds": a.rounds, "warmup": a.warmup,
           "batch": "stage-1: 15 t2i + 4 lm + 10 mmu x 387 tokens per micro-batch, VQ codes fixed, 1 GPU, no exchange",
           "plain_steps": plain, "window": window, "plain_step_ms": plain["ms_per_micro_batch"],
           "saved_ms_per_window": round(saved, 3), "saved_ms_per_skipped_optimizer_step": round(saved / (k - 1), 3),
           "saved_frac_per_micro_batch": round(1.0 - window["ms_per_micro_batch"] / plain["ms_per_micro_batch"], 4),
           "note": "saved = (k - 1) x (AdamW + bf16 image refresh + the next forward's transposed-image rebuild), net of the accumulating "
                   "forms' reads of the old gradient and minus the 479 MB embedding-table clear they skip"}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
