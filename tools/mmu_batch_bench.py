"""Whole-call throughput of Showo.mmu_generate_batch vs n sequential mmu_generate calls at the BASELINE cfg4 shape.

Inputs are built like bench_configs.py's mmu leg: full-size seeded weights (w_clip_vit), 631-embedding prompts (mm_projector of 576
synthetic CLIP features spliced between 30 system / 25 question token embeddings), 100 new tokens, eot_token=None.  Every figure is
tokens / s of a whole call, device-synchronised, after one warm-up call of the same shape; the batched call's tokens are checked
against the sequential calls' (same generator seed).

  python tools/mmu_batch_bench.py              # the JSON below (n = 4, 16, 32; greedy and top_k=5 / temperature=0.7)
  python tools/mmu_batch_bench.py --profile    # one batched greedy and one batched sampled n = 4 call, for a kernel trace
                                               # (rocprofv3 --kernel-trace --stats -- python tools/mmu_batch_bench.py --profile)
  python tools/mmu_batch_bench.py --top-p 0.9  # cost of nucleus sampling: a sampled leg and the same leg with top_p, alternating in
                                               # this process, at batch 1 and n = 4 / 16: median and min / max tokens/s over --reps calls
  python tools/mmu_batch_bench.py --logprobs   # cost of return_logprobs=True: every leg with and without it, alternating in this
                                               # process, at batch 1 and n = 4 / 16, greedy and top_k=5: medians over --reps calls
  python tools/mmu_batch_bench.py --slots 16,32   # wide decode batches (slots=S, csrc/decode_wide.hip) against the call without
                                               # `slots`, alternating in this process, n = 16 / 32 / 64, greedy and top_k=5: medians over
                                               # --reps calls, and the time of one decode step; writes profiles/wide_decode_bench.json
  python tools/mmu_batch_bench.py --profile-wide 32   # one wide greedy n = S call of 17 tokens, for a kernel trace of the wide step
  python tools/mmu_batch_bench.py --repetition-penalty 1.2   # cost of the logit adjustment (csrc/logit_adjust.hip): every leg with and
                                               # without repetition_penalty, alternating in this process, at batch 1 and n = 4 / 16,
                                               # greedy and top_k=5, and (with --slots 32) on 32 wide slots at n = 32: medians over
                                               # --reps calls; writes profiles/logit_adjust_bench.json
  python tools/mmu_batch_bench.py --no-repeat-ngram 4,16   # cost of the sequence rules (csrc/seq_rules.hip): every leg without a keyword,
                                               # with an adjustment alone and with no_repeat_ngram_size, alternating in this process,
                                               # at batch 1 and n = 4 / 16, greedy and top_k=5, and (with --slots 32) on 32 wide slots
                                               # at n = 32: medians over --reps calls; writes profiles/seq_rules_bench.json
  python tools/mmu_batch_bench.py --num-beams 4,8   # beam search (csrc/beam.hip) against mmu_generate_batch of as many greedy
                                               # sequences, alternating in this process: tokens/s of the best hypothesis, ms per step
                                               # of both legs and their difference; writes profiles/beam_bench.json
  python tools/mmu_batch_bench.py --profile-beam 4   # one beam call of 17 tokens, twice, for a kernel trace of the beam step

The slot count for n > 8 is set through modeling_showo._MMU_BATCH_SLOTS for this run only."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NEW = 100
SAMPLED = dict(top_k=5, temperature=0.7)
GREEDY = dict(top_k=1)


def build(n_prompts):
    import showo_amd
    from showo_amd import synthetic
    from showo_amd.prompting_utils import create_attention_mask_for_mmu_vit
    torch.manual_seed(0)
    model = synthetic.random_init_showo(max_batch=1, max_seq=768, w_clip_vit=True).eval()
    tab = model.showo.model.embed_tokens.weight
    embs, masks = [], []
    for b in range(n_prompts):
        gg = torch.Generator(device="cuda").manual_seed(100 + b)
        feats = torch.randn(1, 576, 1024, device="cuda", generator=gg)
        ids = torch.randint(0, 50256, (1, 55), device="cuda", generator=gg)
        with torch.no_grad():
            img = model.mm_projector(feats)
            txt = tab[ids]
            embs.append(torch.cat([txt[:, :30], img, txt[:, 30:]], dim=1).contiguous())
        masks.append(create_attention_mask_for_mmu_vit(embs[-1], system_prompt_len=28)[0])
    assert embs[0].shape[1] == 631
    return showo_amd, model, embs, masks


def timed(fn):
    fn()  # warm-up call of the same shape
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, [[int(t) for t in r] for r in out]


def nucleus_legs(model, embs, masks, top_p, reps):
    """tokens/s of a sampled leg and of the same leg behind the nucleus filter, measured alternately (base, top-p, base, top-p, ...) so
    that both see the same clocks; per leg the median and the min / max of `reps` whole calls after one warm-up call each"""
    gen = lambda: torch.Generator(device="cuda").manual_seed(7)  # noqa: E731

    def call(n, kw):
        if n == 1:
            return lambda: model.mmu_generate(input_embeddings=embs[0], attention_mask=masks[0], max_new_tokens=NEW, generator=gen(), **kw)
        return lambda: model.mmu_generate_batch(input_embeddings=embs[:n], attention_mask=masks[:n], max_new_tokens=NEW, generator=gen(), **kw)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    res = {"shape": "cfg4: 631-embedding w_clip_vit prompts, 100 new tokens each, full-size seeded weights",
           "unit": "tokens/s (whole call)", "top_p": top_p, "reps": reps}
    for n in (1, 4, 16):
        for name, kw in (("topk5_t0.7", SAMPLED), ("unfiltered_t1.0", dict(top_k=None, temperature=1.0))):
            legs = {"base": call(n, kw), "top_p": call(n, dict(kw, top_p=top_p))}
            for fn in legs.values():
                fn()  # warm-up
            times = {k: [] for k in legs}
            for _ in range(reps):
                for k, fn in legs.items():
                    times[k].append(once(fn))
            row = {}
            for k, ts in times.items():
                rate = sorted(n * NEW / t for t in ts)
                row[k] = {"median": float(np.median(rate)), "min": rate[0], "max": rate[-1]}
            row["top_p_overhead_percent"] = 100.0 * (row["base"]["median"] / row["top_p"]["median"] - 1.0)
            res[f"n{n}_{name}"] = row
            print(f"n={n} {name}: {row}", file=sys.stderr, flush=True)
    return res


def logprob_legs(model, embs, masks, reps):
    """tokens/s of every leg without and with return_logprobs=True, measured alternately (off, on, off, on, ...) so that both see the
    same clocks; per leg the median and the min / max of `reps` whole calls after one warm-up call each.  The tokens of the two legs
    are checked to be equal.  per_token_us: the difference of the median call times over the tokens of the call (one scoring launch
    per decode step and slot row; at n = 4 greedy the "on" leg also trades the all-greedy loop for the slot scheduler's)."""
    gen = lambda: torch.Generator(device="cuda").manual_seed(7)  # noqa: E731

    def call(n, kw):
        if n == 1:
            return lambda: model.mmu_generate(input_embeddings=embs[0], attention_mask=masks[0], max_new_tokens=NEW, generator=gen(), **kw)
        return lambda: model.mmu_generate_batch(input_embeddings=embs[:n], attention_mask=masks[:n], max_new_tokens=NEW, generator=gen(), **kw)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def ints(out, n):
        return [int(t) for t in out] if n == 1 else [[int(t) for t in r] for r in out]

    res = {"shape": "cfg4: 631-embedding w_clip_vit prompts, 100 new tokens each, full-size seeded weights",
           "unit": "tokens/s (whole call)", "reps": reps}
    for n in (1, 4, 16):
        for name, kw in (("greedy", GREEDY), ("topk5_t0.7", SAMPLED)):
            legs = {"off": call(n, kw), "on": call(n, dict(kw, return_logprobs=True))}
            off, on = legs["off"](), legs["on"]()  # warm-up, and the feature changes no token
            assert ints(off, n) == ints(on[0], n), (n, name)
            times = {k: [] for k in legs}
            for _ in range(reps):
                for k, fn in legs.items():
                    times[k].append(once(fn))
            row = {}
            for k, ts in times.items():
                rate = sorted(n * NEW / t for t in ts)
                row[k] = {"median": float(np.median(rate)), "min": rate[0], "max": rate[-1]}
            row["logprobs_overhead_percent"] = 100.0 * (row["off"]["median"] / row["on"]["median"] - 1.0)
            row["per_token_us"] = 1e6 * (float(np.median(times["on"])) - float(np.median(times["off"]))) / (n * NEW)
            res[f"n{n}_{name}"] = row
            print(f"n={n} {name}: {row}", file=sys.stderr, flush=True)
    return res


def penalty_legs(model, embs, masks, theta, reps, wide_slots=None):
    """tokens/s of every leg without and with repetition_penalty=theta, measured alternately (off, on, off, on, ...) so that both see the
    same clocks; per leg the median and the min / max of `reps` whole calls after one warm-up call each.  eot_token is None, so both
    legs emit the same number of tokens (the tokens themselves differ: that is the feature).  per_token_us: the difference of the
    median call times over the tokens of the call.  What "on" adds per decode step: one adjust launch for all slots; the batch-1 greedy
    leg (reported on its own as n1_greedy) ALSO trades the fused token seam for arg-max + store + increment launches, the top-k 5 legs
    keep their token boundary, so n1_topk5 is the launch alone; at n = 4 the greedy "on" leg trades the all-greedy loop for the slot
    scheduler's as return_logprobs does.  wide_slots: one more pair of legs at n = 32 on that many wide slots."""
    gen = lambda: torch.Generator(device="cuda").manual_seed(7)  # noqa: E731

    def call(n, kw):
        if n == 1:
            return lambda: model.mmu_generate(input_embeddings=embs[0], attention_mask=masks[0], max_new_tokens=NEW, generator=gen(), **kw)
        return lambda: model.mmu_generate_batch(input_embeddings=embs[:n], attention_mask=masks[:n], max_new_tokens=NEW, generator=gen(), **kw)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    res = {"shape": "cfg4: 631-embedding w_clip_vit prompts, 100 new tokens each, full-size seeded weights",
           "unit": "tokens/s (whole call)", "reps": reps, "repetition_penalty": theta}
    shapes = [(1, {}), (4, {}), (16, {})] + ([(32, {"slots": wide_slots})] if wide_slots else [])
    for n, extra in shapes:
        for name, kw in (("greedy", GREEDY), ("topk5_t0.7", SAMPLED)):
            kw = dict(kw, **extra)
            legs = {"off": call(n, kw), "on": call(n, dict(kw, repetition_penalty=theta))}
            for fn in legs.values():
                fn()  # warm-up
            times = {k: [] for k in legs}
            for _ in range(reps):
                for k, fn in legs.items():
                    times[k].append(once(fn))
            row = {}
            for k, ts in times.items():
                rate = sorted(n * NEW / t for t in ts)
                row[k] = {"median": float(np.median(rate)), "min": rate[0], "max": rate[-1]}
            row["adjust_overhead_percent"] = 100.0 * (row["off"]["median"] / row["on"]["median"] - 1.0)
            row["per_token_us"] = 1e6 * (float(np.median(times["on"])) - float(np.median(times["off"]))) / (n * NEW)
            res[f"n{n}_{name}" + (f"_slots{wide_slots}" if extra else "")] = row
            print(f"n={n} {name}: {row}", file=sys.stderr, flush=True)
    return res


def seq_rule_legs(model, embs, masks, ngram, reps, wide_slots=None):
    """tokens/s of every leg without a keyword ("off"), with banned_tokens alone ("adjust": the adjust launch the rules ride behind) and
    with no_repeat_ngram_size=ngram ("on": the adjust launch as a bit copy plus the ban launch of csrc/seq_rules.hip), measured
    alternately (off, adjust, on, off, ...) so that all see the same clocks; per leg the median and the min / max of `reps` whole calls
    after one warm-up call each.  eot_token is None, so every leg emits the same number of tokens.  per_token_us: the difference of
    the median call times of "on" and "off" over the tokens of the call; ban_per_token_us: that of "on" and "adjust", the ban launch
    alone.  As with --repetition-penalty the batch-1 greedy "on" leg also trades the fused token seam for separate launches and the
    n = 4 greedy one the all-greedy loop for the slot scheduler's; "adjust" makes the same trades."""
    gen = lambda: torch.Generator(device="cuda").manual_seed(7)  # noqa: E731

    def call(n, kw):
        if n == 1:
            return lambda: model.mmu_generate(input_embeddings=embs[0], attention_mask=masks[0], max_new_tokens=NEW, generator=gen(), **kw)
        return lambda: model.mmu_generate_batch(input_embeddings=embs[:n], attention_mask=masks[:n], max_new_tokens=NEW, generator=gen(), **kw)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    res = {"shape": "cfg4: 631-embedding w_clip_vit prompts, 100 new tokens each, full-size seeded weights",
           "unit": "tokens/s (whole call)", "reps": reps, "no_repeat_ngram_size": ngram}
    shapes = [(1, {}), (4, {}), (16, {})] + ([(32, {"slots": wide_slots})] if wide_slots else [])
    for n, extra in shapes:
        for name, kw in (("greedy", GREEDY), ("topk5_t0.7", SAMPLED)):
            kw = dict(kw, **extra)
            legs = {"off": call(n, kw), "adjust": call(n, dict(kw, banned_tokens=[model.vocab_size - 1])),
                    "on": call(n, dict(kw, no_repeat_ngram_size=ngram))}
            for fn in legs.values():
                fn()  # warm-up
            times = {k: [] for k in legs}
            for _ in range(reps):
                for k, fn in legs.items():
                    times[k].append(once(fn))
            row = {}
            for k, ts in times.items():
                rate = sorted(n * NEW / t for t in ts)
                row[k] = {"median": float(np.median(rate)), "min": rate[0], "max": rate[-1]}
            med = {k: float(np.median(ts)) for k, ts in times.items()}
            row["rules_overhead_percent"] = 100.0 * (med["on"] / med["off"] - 1.0)
            row["per_token_us"] = 1e6 * (med["on"] - med["off"]) / (n * NEW)
            row["ban_per_token_us"] = 1e6 * (med["on"] - med["adjust"]) / (n * NEW)
            res[f"n{n}_{name}" + (f"_slots{wide_slots}" if extra else "")] = row
            print(f"n={n} {name}: {row}", file=sys.stderr, flush=True)
    return res


def wide_legs(model, embs, masks, slot_counts, reps):
    """tokens/s of mmu_generate_batch without `slots` (the baseline: 8 slots of the dot2 kernels) and with slots=S for every S, measured
    alternately (None, S1, S2, None, ...) so that all legs see the same clocks; per leg the median and min / max of `reps` whole calls
    after one warm-up call each, and ratio = median / the baseline's median.  step_ms: the time of one decode step of S = n slots,
    from the difference of a 100-token and a 36-token greedy call (64 steps, the prefills cancel).  A wide call is not the baseline's
    bits (another fp32 summation order), so tokens are compared only between the wide legs: they must agree with each other."""
    gen = lambda: torch.Generator(device="cuda").manual_seed(7)  # noqa: E731

    def call(n, kw, S, new=NEW):
        extra = {} if S is None else {"slots": S}
        return lambda: model.mmu_generate_batch(input_embeddings=embs[:n], attention_mask=masks[:n], max_new_tokens=new, generator=gen(),
                                                **kw, **extra)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    res = {"shape": "cfg4: 631-embedding w_clip_vit prompts, 100 new tokens each, full-size seeded weights",
           "unit": "tokens/s (whole call)", "reps": reps, "slots": slot_counts}
    for n in (16, 32, 64):
        for name, kw in (("greedy", GREEDY), ("topk5_t0.7", SAMPLED)):
            legs = {"none": call(n, kw, None)}
            for S in slot_counts:
                legs[f"slots{S}"] = call(n, kw, S)
            first = {k: [[int(t) for t in r] for r in fn()] for k, fn in legs.items()}  # warm-up
            wide = [first[f"slots{S}"] for S in slot_counts]
            assert all(w == wide[0] for w in wide), (n, name, "the wide legs disagree")
            agree = sum(a == b for a, b in zip(first["none"], wide[0]))
            times = {k: [] for k in legs}
            for _ in range(reps):
                for k, fn in legs.items():
                    times[k].append(once(fn))
            row = {"requests_with_the_baseline_tokens": f"{agree}/{n}"}
            for k, ts in times.items():
                rate = sorted(n * NEW / t for t in ts)
                row[k] = {"median": float(np.median(rate)), "min": rate[0], "max": rate[-1]}
            for S in slot_counts:
                row[f"slots{S}"]["ratio"] = row[f"slots{S}"]["median"] / row["none"]["median"]
            res[f"n{n}_{name}"] = row
            print(f"n={n} {name}: {row}", file=sys.stderr, flush=True)
    steps = {}
    for S in [8] + list(slot_counts):
        n = S
        extra = None if S == 8 else S
        long_, short = call(n, GREEDY, extra, 100), call(n, GREEDY, extra, 36)
        long_(), short()
        tl, ts = [], []
        for _ in range(3):
            tl.append(once(long_))
            ts.append(once(short))
        steps[f"slots{S}_n{n}"] = 1e3 * (float(np.median(tl)) - float(np.median(ts))) / 64
    res["step_ms"] = steps
    print(f"step_ms: {steps}", file=sys.stderr, flush=True)
    return res


def beam_legs(model, embs, masks, B, reps):
    """Beam search with B beams against mmu_generate_batch of n = B greedy sequences (the same weight stream per step without the
    selection, the seam and the parent copies), measured alternately in this process at two lengths (SHORT and NEW new tokens): per
    leg the medians of `reps` whole calls, tokens/s of the best hypothesis, and the time of one step as the difference of the two
    lengths' medians over the difference in steps (prefill, forks and the first pick drop out).  eot_token=None: every call runs to its
    length."""
    SHORT = 20

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def beam(T):
        return lambda: model.mmu_generate(input_embeddings=embs[0], attention_mask=masks[0], max_new_tokens=T, num_beams=B)

    def greedy(T):
        return lambda: model.mmu_generate_batch(input_embeddings=embs[:B], attention_mask=masks[:B], max_new_tokens=T, top_k=1)

    legs = {"beam_short": beam(SHORT), "greedy_short": greedy(SHORT), "beam": beam(NEW), "greedy": greedy(NEW)}
    for fn in legs.values():
        fn()  # warm-up
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(once(fn))
    med = {k: float(np.median(v)) for k, v in times.items()}
    step = {k: 1e3 * (med[k] - med[k + "_short"]) / (NEW - SHORT) for k in ("beam", "greedy")}
    res = {"shape": "cfg4: 631-embedding w_clip_vit prompts, full-size seeded weights", "num_beams": B, "new_tokens": NEW, "reps": reps,
           "call_ms": {k: 1e3 * v for k, v in med.items()},
           "call_ms_min_max": {k: [1e3 * min(v), 1e3 * max(v)] for k, v in times.items()},
           "best_hypothesis_tokens_per_s": NEW / med["beam"], "greedy_batch_tokens_per_s": B * NEW / med["greedy"],
           "step_ms": step, "step_ms_added_by_beams": step["beam"] - step["greedy"]}
    print(f"num_beams={B}: {res}", file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--num-beams", default=None, help="comma-separated beam counts (2..8): beam search against mmu_generate_batch of as many "
                                                      "greedy sequences, alternating in this process; writes profiles/beam_bench.json")
    ap.add_argument("--profile-beam", type=int, default=None, help="one beam call of 17 tokens with this many beams, twice, for a kernel trace")
    ap.add_argument("--top-p", type=float, default=None, help="measure nucleus sampling against the same sampled leg without it")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--logprobs", action="store_true", help="measure return_logprobs=True against the same legs without it")
    ap.add_argument("--out", default=None, help="also write the JSON of --top-p / --logprobs to this file")
    ap.add_argument("--slots", default=None, help="comma-separated wide slot counts (9..32) to measure against the call without `slots`")
    ap.add_argument("--profile-wide", type=int, default=None, help="one wide greedy call of 17 tokens on this many slots, for a kernel trace")
    ap.add_argument("--repetition-penalty", type=float, default=None,
                    help="measure repetition_penalty=THETA against the same legs without it (with --slots S: also n = 32 on S wide slots)")
    ap.add_argument("--no-repeat-ngram", default=None,
                    help="comma-separated sizes N (1..16): measure no_repeat_ngram_size=N against the same legs without it and with an adjustment alone (with --slots S: also "
                         "n = 32 on S wide slots); writes profiles/seq_rules_bench.json")
    a = ap.parse_args()
    if a.no_repeat_ngram is not None:
        wide = int(a.slots.split(",")[0]) if a.slots else None
        pkg, model, embs, masks = build(32 if wide else 16)
        res = {f"no_repeat_ngram_{N}": seq_rule_legs(model, embs, masks, N, a.reps, wide) for N in (int(t) for t in a.no_repeat_ngram.split(","))}
        out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "seq_rules_bench.json")
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    if a.profile_beam is not None:
        pkg, model, embs, masks = build(1)
        for _ in range(2):
            model.mmu_generate(input_embeddings=embs[0], attention_mask=masks[0], max_new_tokens=17, num_beams=a.profile_beam)
        torch.cuda.synchronize()
        print(json.dumps({"profiled": f"mmu_generate num_beams={a.profile_beam}, 17 tokens, twice"}))
        return
    if a.num_beams is not None:
        pkg, model, embs, masks = build(8)
        res = {f"num_beams_{B}": beam_legs(model, embs, masks, B, a.reps) for B in (int(t) for t in a.num_beams.split(","))}
        out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "beam_bench.json")
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    if a.repetition_penalty is not None:
        wide = int(a.slots.split(",")[0]) if a.slots else None
        pkg, model, embs, masks = build(32 if wide else 16)
        res = penalty_legs(model, embs, masks, a.repetition_penalty, a.reps, wide)
        out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "logit_adjust_bench.json")
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    if a.profile_wide is not None:
        S = a.profile_wide
        pkg, model, embs, masks = build(S)
        for _ in range(2):
            model.mmu_generate_batch(input_embeddings=embs[:S], attention_mask=masks[:S], max_new_tokens=17, top_k=1, slots=S)
        torch.cuda.synchronize()
        print(json.dumps({"profiled": f"mmu_generate_batch n={S} greedy slots={S}, 17 tokens, twice"}))
        return
    if a.slots is not None:
        pkg, model, embs, masks = build(64)
        res = wide_legs(model, embs, masks, [int(t) for t in a.slots.split(",")], a.reps)
        out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wide_decode_bench.json")
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    pkg, model, embs, masks = build(4 if a.profile else (16 if (a.top_p is not None or a.logprobs) else 32))
    if a.logprobs:
        res = logprob_legs(model, embs, masks, a.reps)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    if a.top_p is not None:
        res = nucleus_legs(model, embs, masks, a.top_p, a.reps)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    M = pkg.modeling_showo
    gen = lambda: torch.Generator(device="cuda").manual_seed(7)  # noqa: E731

    def batched(n, kw):
        return lambda: model.mmu_generate_batch(input_embeddings=embs[:n], attention_mask=masks[:n], max_new_tokens=NEW, generator=gen(), **kw)

    def sequential(n, kw):
        def run():
            g = gen()
            return [model.mmu_generate(input_embeddings=embs[b], attention_mask=masks[b], max_new_tokens=NEW, generator=g, **kw)
                    for b in range(n)]
        return run

    if a.profile:
        for kw in (GREEDY, SAMPLED):
            batched(4, kw)()
        torch.cuda.synchronize()
        print(json.dumps({"profiled": "mmu_generate_batch n=4 greedy, then n=4 top_k=5 temperature=0.7"}))
        return
    res = {"shape": "cfg4: 631-embedding w_clip_vit prompts, 100 new tokens each, full-size seeded weights", "unit": "tokens/s (whole call)"}
    for n in (4, 16, 32):
        for name, kw in (("greedy", GREEDY), ("sampled_topk5_t0.7", SAMPLED)):
            row = {}
            ts, want = timed(sequential(n, kw))
            row["sequential"] = n * NEW / ts
            slot_choices = [None] if n <= 8 else [4, 8]
            for slots in slot_choices:
                keep = M._MMU_BATCH_SLOTS
                if slots is not None:
                    M._MMU_BATCH_SLOTS = slots
                try:
                    tb, got = timed(batched(n, kw))
                finally:
                    M._MMU_BATCH_SLOTS = keep
                assert got == want, (n, name, slots)
                row["batched" if slots is None else f"batched_{slots}_slots"] = n * NEW / tb
            res[f"n{n}_{name}"] = row
            print(f"n={n} {name}: {row}", file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
