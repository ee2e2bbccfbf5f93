"""What does an EMA of the weights cost per training step, in its three forms?  Stage-1 batch of bench_train.py (15 t2i + 4 lm + 10
mmu sequences x 387 tokens, VQ codes fixed), one MI355X, ONE process, two models started from the same seed: a plain Trainer and a
Trainer(ema=0.9999).  A round runs every leg once, the rounds repeat, so that clocks and the allocator's state are shared; every leg
is bracketed by device events.  Step legs (one Trainer.step each):

  (a) step             Trainer.step without EMA: the parent's step
  (b) step_fused       Trainer(ema=...).step: the shadows are updated inside the AdamW launch
  (c) step_table       (a) + one stand-alone segment-table launch over the 437 tensors (training_utils.EMA.step)
  (d) step_torch       (a) + the reference-form torch loop  s.sub_(omd * (s - p))  per tensor; step_torch_empty_cache adds the
                       reference's torch.cuda.empty_cache()
  (e) ema_weights      one `with trainer.ema_weights(): pass` -- two swaps with their image refresh (no step)

Optimizer legs (the launches alone, through the C ABI, gradients of the last backward): adamw, adamw_fused, table, torch_loop.
Reported per leg: the median of --rounds timed rounds, min and max; and the differences against (a) / adamw.  Prints one JSON line
and writes it to --out.

    python tools/ema_train_bench.py [--rounds 7] [--warmup 2] [--out profiles/ema_bench.json]"""
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
DECAY = 0.9999


def _batch(mask_token_id):
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
    ids, labels, mask, _, split = build_training_batch(uni, cfg, mask_token_id, showo_amd.cosine_schedule, codes[:bt], list(tt), list(tl),
                                                       codes[bt:], list(tm))
    return ids, mask, labels, tuple(split)


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(min(ms)), 3), "max_ms": round(float(max(ms)), 3),
            "spread_ms": round(float(max(ms) - min(ms)), 3), "rounds_ms": [round(float(x), 3) for x in ms]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    a = ap.parse_args(argv)
    if a.rounds < 3 or a.warmup < 1:
        ap.error("--rounds >= 3 and --warmup >= 1")
    import showo_amd
    from showo_amd import _lib, synthetic
    from showo_amd.training_utils import EMA
    models, trainers = [], []
    for ema in (None, DECAY):
        torch.manual_seed(0)
        m = synthetic.random_init_showo(max_batch=29, max_seq=387).train()
        models.append(m)
        trainers.append(showo_amd.Trainer(m, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, coeffs=COEFFS, ema=ema))
    ta, tb = trainers
    ids, mask, labels, (b1, b2, b3) = _batch(models[0].mask_token_id)
    params = [p for _, p in ta.params]
    side = EMA(params, decay=DECAY)                                  # the stand-alone table over the plain trainer's parameters
    loop_shadows = [p.detach().clone() for p in params]              # the torch loop's own shadows
    omd = 1 - DECAY
    n_elems = sum(p.numel() for p in params)

    def step(tr):
        tr.step(ids, mask, labels, b1, b2, b3, 128)

    def torch_loop(empty):
        with torch.no_grad():
            for s, p in zip(loop_shadows, params):
                s.sub_(omd * (s - p))
        if empty:
            torch.cuda.empty_cache()

    def ctx():
        with tb.ema_weights():
            pass

    def adamw(tr, fused):
        if fused:
            _lib.call("showo_train_set_ema", tr.tr, omd)
        _lib.call("showo_train_adamw_step", tr.tr, tr.lr, tr.betas[0], tr.betas[1], tr.eps, tr.wd, max(tr.step_count, 1), _lib.stream())

    legs = [
        ("step", lambda: step(ta)),
        ("step_fused", lambda: step(tb)),
        ("step_table", lambda: (step(ta), side.step(params))),
        ("step_torch", lambda: (step(ta), torch_loop(False))),
        ("step_torch_empty_cache", lambda: (step(ta), torch_loop(True))),
        ("ema_weights", ctx),
        ("adamw", lambda: adamw(ta, False)),
        ("adamw_fused", lambda: adamw(tb, True)),
        ("table", lambda: side.step(params)),
        ("torch_loop", lambda: torch_loop(False)),
    ]
    for _ in range(a.warmup):
        for _, f in legs:
            f()
    ev = {k: [] for k, _ in legs}
    for _ in range(a.rounds):
        for k, f in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    res = {k: _stats([e0.elapsed_time(e1) for e0, e1 in ev[k]]) for k, _ in legs}
    med = {k: res[k]["median_ms"] for k in res}
    gb = n_elems / 1e9
    out = {"tool": "ema_train_bench", "rounds": a.rounds, "warmup": a.warmup, "decay": DECAY, "tensors": len(params), "elements": n_elems,
           "batch": "stage-1: 15 t2i + 4 lm + 10 mmu x 387 tokens, VQ codes fixed, 1 GPU, no exchange",
           "legs": res,
           "added_ms_per_step_vs_plain": {k: round(med[k] - med["step"], 3) for k in ("step_fused", "step_table", "step_torch",
                                                                                      "step_torch_empty_cache")},
           "added_ms_optimizer_only": {"fused": round(med["adamw_fused"] - med["adamw"], 3), "table": med["table"], "torch_loop": med["torch_loop"]},
           "fused_added_frac_of_adamw": round((med["adamw_fused"] - med["adamw"]) / med["adamw"], 4),
           "bytes_per_element": {"adamw": 30, "fused_adds": 8, "table_adds": 12},
           "effective_GBps": {"adamw": round(30 * gb / (med["adamw"] * 1e-3), 1), "adamw_fused": round(38 * gb / (med["adamw_fused"] * 1e-3), 1),
                              "table": round(12 * gb / (med["table"] * 1e-3), 1)},
           "ema_weights_enter_exit_ms": med["ema_weights"]}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
