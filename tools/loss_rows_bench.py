"""What does the loss head cost on rows nobody reads?  `Trainer(loss_rows="all")` against `loss_rows="labelled"` on the stage-1 batch
of bench_train.py (15 t2i + 4 lm + 10 mmu sequences x 387 tokens, VQ codes fixed) and on an lm-only batch of the same size, one
MI355X, ONE process, one model and one Trainer whose mode is toggled step by step after the warm-up, so both modes share clocks,
allocator state and the weights' trajectory.  Every step is a wall-clock interval between two device synchronisations: the labelled
mode's one host wait (for the row count) is inside it.

On the stage-1 batch about half the rows carry a label, so the labelled head does about half the work.  On the lm-only batch every
row but the last of each sequence carries one (Tc = T - B when the texts fill the sequence): the mode can only cost there -- the
census plus the host wait -- and that cost is what the second pair of numbers reports.

    python tools/loss_rows_bench.py [--steps 12] [--warmup 3] [--batches 4] [--out profiles/loss_rows_bench.json]

`--only all|labelled` runs the stage-1 steps in that one mode and writes nothing: the program to put behind
`rocprofv3 --kernel-trace --stats --` for a kernel table per mode (profiles/loss_rows_kernel_stats_{all,labelled}.csv)."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

COEFFS = (1.0, 0.1, 1.0)
MODES = ("all", "labelled")


def stage1_batches(n, mask_token_id):
    """n draws of the mixed batch, built the way bench_train.py's step() builds it (texts once, masking re-drawn per batch)"""
    import showo_amd
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
    tt, tl, tm = synthetic_texts(rs, bt, bl, bm)
    codes = torch.randint(0, codebook, (bt + bm, N), device="cuda") + off
    out = []
    for _ in range(n):
        ids, labels, mask, _, split = build_training_batch(uni, cfg, mask_token_id, showo_amd.cosine_schedule, codes[:bt], list(tt), list(tl),
                                                           codes[bt:], list(tm))
        out.append((ids, mask, labels, tuple(split)))
    return out, uni


def lm_only_batch(uni, L, n_seq=29):
    from showo_amd import prompting_utils as pu
    from bench_train import synthetic_texts
    sp = uni.sptids_dict
    _, texts, _ = synthetic_texts(np.random.RandomState(9), 0, n_seq, 0)
    ids, _, labels = uni((list(texts), L), 'lm')
    ids, labels = ids.cuda(), labels.cuda()
    iv = pu.intervals_predict_next(ids, pad_id=int(sp['<|pad|>']), soi_id=int(sp['<|soi|>']), eoi_id=int(sp['<|eoi|>']))
    return [(ids, iv, labels, (0, n_seq, 0))]


def timed(tr, batches, steps, warmup):
    """alternate the modes step by step on the same batch; ms per step of each mode and (Tc, T) per batch"""
    ms = {m: [] for m in MODES}
    rows = []
    for i in range(warmup + steps):
        ids, mask, labels, (b1, b2, b3) = batches[i % len(batches)]
        order = MODES if i % 2 == 0 else MODES[::-1]  # neither mode always runs second
        for mode in order:
            tr.set_loss_rows(mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.step(ids, mask, labels, b1, b2, b3, 128)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= warmup:
                ms[mode].append(dt)
            if mode == "labelled" and i < len(batches):
                rows.append(list(tr.loss_rows_count))
    out = {}
    for mode in MODES:
        v = np.asarray(ms[mode])
        out[mode] = {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(v.min()), 3), "max_ms": round(float(v.max()), 3),
                     "std_ms": round(float(v.std()), 3), "steps_ms": [round(float(x), 3) for x in v]}
    pair = np.asarray(ms["all"]) - np.asarray(ms["labelled"])  # same batch, back to back
    out["saved_ms_median_of_pairs"] = round(float(np.median(pair)), 3)
    out["saved_ms_pairs_min_max"] = [round(float(pair.min()), 3), round(float(pair.max()), 3)]
    out["rows_labelled_total"] = rows
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_rows_bench.json"))
    ap.add_argument("--only", choices=MODES, default=None, help="one mode only, stage-1 batch, nothing written (for a profiler)")
    a = ap.parse_args(argv)
    import showo_amd
    from showo_amd import synthetic
    torch.manual_seed(0)
    model = synthetic.random_init_showo(max_batch=29, max_seq=387).train()
    tr = showo_amd.Trainer(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, coeffs=COEFFS)
    batches, uni = stage1_batches(a.batches, model.mask_token_id)
    # every distinct labelled-row count is a new GEMM shape (tile candidates are timed once per shape): the warm-up must meet them all
    warm = max(a.warmup, len(batches))
    if a.only:
        tr.set_loss_rows(a.only)
        for i in range(warm + a.steps):
            ids, mask, labels, (b1, b2, b3) = batches[i % len(batches)]
            tr.step(ids, mask, labels, b1, b2, b3, 128)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "loss_rows_bench", "only": a.only, "steps": warm + a.steps, "rows_labelled_total": list(tr.loss_rows_count)}))
        return
    stage1 = timed(tr, batches, a.steps, warm)
    lm = timed(tr, lm_only_batch(uni, batches[0][0].shape[1]), a.steps, a.warmup)
    out = {"tool": "loss_rows_bench", "steps": a.steps, "warmup": warm,
           "batch": "stage-1: 15 t2i + 4 lm + 10 mmu x 387 tokens, VQ codes fixed, masking re-drawn per batch, 1 GPU, no exchange",
           "timing": "wall clock between device synchronisations around Trainer.step; modes alternate on the same batch",
           "stage1": stage1, "lm_only": lm}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
