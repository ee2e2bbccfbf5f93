"""Precision 3 (int8 decode weights) against precision 0 on the KV-cached decode, BASELINE cfg4 shape, ONE process.

Inputs as in tools/mmu_batch_bench.py: full-size seeded weights (w_clip_vit), 631-embedding prompts, 100 new tokens, eot_token=None;
every time is a whole call, device-synchronised, after a warm-up call of the same shape.  The two precisions ALTERNATE (a switch
re-uploads the weights; the warm-up call absorbs that), `--rounds` rounds each (default 5), for three legs: mmu_generate (batch 1,
greedy) and mmu_generate_batch with n = 4 and n = 8 (greedy: the batched kernels, one weight stream per token step for all n, bf16
or int8 instances).  Per leg and precision: median tokens/s, spread (max - min over the rounds), and the weight bytes of the token
steps over the decode-only time (whole call minus a 1-token call of the same prompt) as GB/s; per leg the ratio of the medians.

  python tools/mmu_int8_bench.py              # one JSON line
  python tools/mmu_int8_bench.py --profile    # one call per leg and precision, for a kernel trace
                                              # (rocprofv3 --kernel-trace --stats -- python tools/mmu_int8_bench.py --profile)"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mmu_batch_bench import NEW, build  # noqa: E402

GREEDY = dict(top_k=1)


def weight_bytes(model):
    """bytes of GEMM weights one token step streams: bf16 = 2 x weights; int8 = 1 x weights + 4 x rows (the fp32 scales)"""
    a = model.arch
    H, F, nL, V = a["hidden_size"], a["intermediate_size"], a["num_hidden_layers"], model.vocab_size
    weights = nL * (3 * H * H + H * H + F * H + H * F) + V * H
    rows = nL * (3 * H + H + F + H) + V
    return {0: 2 * weights, 3: weights + 4 * rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    _, model, embs, masks = build(8)

    def leg(n, new):
        if n == 1:
            return lambda: [model.mmu_generate(input_embeddings=embs[0], attention_mask=masks[0], max_new_tokens=new, **GREEDY)]
        return lambda: model.mmu_generate_batch(input_embeddings=embs[:n], attention_mask=masks[:n], max_new_tokens=new, **GREEDY)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, [[int(t) for t in r] for r in out]

    legs = (("batch1", 1), ("n4", 4), ("n8", 8))
    if a.profile:
        for prec in (0, 3):
            model.set_precision(prec)
            for _, n in legs[:2]:
                leg(n, NEW)()
        torch.cuda.synchronize()
        print(json.dumps({"profiled": "precision 0 then 3: mmu_generate (batch 1) and mmu_generate_batch n=4, greedy, 100 tokens"}))
        return
    wb = weight_bytes(model)
    times = {(name, p): [] for name, _ in legs for p in (0, 3)}
    pre = {(name, p): [] for name, _ in legs for p in (0, 3)}
    tokens = {}
    for r in range(a.rounds):
        for prec in (0, 3):
            model.set_precision(prec)
            for name, n in legs:
                leg(n, NEW)()  # warm-up call of the same shape (after a switch: the weight upload too)
                t, out = timed(leg(n, NEW))
                assert tokens.setdefault((name, prec), out) == out  # every round decodes the same tokens
                times[(name, prec)].append(t)
                pre[(name, prec)].append(timed(leg(n, 1))[0])
            print(f"round {r} precision {prec}: " + ", ".join(f"{name} {n * NEW / times[(name, prec)][-1]:.1f} tok/s" for name, n in legs),
                  file=sys.stderr, flush=True)
    res = {"shape": "cfg4: 631-embedding w_clip_vit prompts, 100 new tokens each, full-size seeded weights, greedy", "rounds": a.rounds,
           "unit": "tokens/s (whole call)", "weight_bytes_per_step": {"precision0": wb[0], "precision3": wb[3]}}
    for name, n in legs:
        row = {}
        for prec in (0, 3):
            tps = [n * NEW / t for t in times[(name, prec)]]
            streams = 1  # the batched engine path streams the weights once per token step for all n sequences
            dec = [t - p for t, p in zip(times[(name, prec)], pre[(name, prec)])]
            gbs = [wb[prec] * streams * (NEW - 1) / t / 1e9 for t in dec]
            row[f"precision{prec}"] = {"median": statistics.median(tps), "spread": max(tps) - min(tps), "rounds": tps,
                                       "weight_GBps_decode_only_median": statistics.median(gbs), "weight_streams_per_step": streams}
        row["ratio_3_over_0"] = row["precision3"]["median"] / row["precision0"]["median"]
        row["faster_beyond_spreads"] = bool(row["precision3"]["median"] - row["precision0"]["median"] >
                                            row["precision3"]["spread"] + row["precision0"]["spread"])
        a0, a3 = tokens[(name, 0)], tokens[(name, 3)]
        row["tokens_equal_to_precision0"] = sum(int(x == y) for s0, s3 in zip(a0, a3) for x, y in zip(s0, s3)) / float(n * NEW)
        res[name] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
