"""What an mmu session saves at the BASELINE cfg4 shape: one prefill of the question-invariant prefix instead of one per question.

Inputs are built like bench_configs.py's mmu leg: full-size seeded weights (w_clip_vit), one image = 576 synthetic CLIP features through
the mm_projector, spliced behind 30 system-prompt embeddings (prefix: 607 rows incl. <|eoi|>), questions of 24 token embeddings each
(631 rows per full prompt), greedy decode, eot_token=None.  One process; after a warm-up of every variant the variants ALTERNATE and
every figure is the median of >= 5 wall-clock intervals taken between device synchronisations.

  first comparison   k = 4 questions about one image: 4 x mmu_generate(full prompt)  vs  one mmu_session + 4 x (generate, rewind);
                     per question: time to first token (max_new_tokens = 1) and the whole call (100 new tokens)
  second comparison  n = 4 / 8 questions decoded together: mmu_generate_batch on n full prompts  vs  sess.generate_batch
  fork               showo_kv_fork of the 607-row prefix into one slot next to showo_copy_b128 on the same byte count (GB/s, read + write;
                     an interval is 50 calls queued between two synchronisations)

The baseline is the full-prompt path of the same build in the same process.  Writes profiles/mmu_prefix_bench.json.

  python tools/mmu_prefix_bench.py [--reps 5] [--new 100] [--out profiles/mmu_prefix_bench.json]
  python tools/mmu_prefix_bench.py --share-prefix [--reps 7]   # shared-prefix slots (share_prefix=True, csrc/attn_shared.hip): n = 32 / 64
                                               # questions about one image on 32 wide slots, greedy and top_k=5; legs alternating in
                                               # this process: sess.generate_batch(slots=32) forked, the same call with share_prefix=True,
                                               # mmu_generate_batch(slots=32) on full prompts (behind them: it replaces the decode cache);
                                               # tokens/s of the whole call, one decode step
                                               # by the 100-vs-36-token difference, token agreement forked / shared -> profiles/shared_prefix_bench.json
  python tools/mmu_prefix_bench.py --profile-shared 32   # one shared greedy n = S call of 17 tokens, twice, for a kernel trace"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, LQ = 607, 24


def build(n_questions):
    import showo_amd
    from showo_amd import synthetic
    from showo_amd.prompting_utils import create_attention_mask_for_mmu_vit, mmu_prefix_is_exact
    torch.manual_seed(0)
    model = synthetic.random_init_showo(max_batch=1, max_seq=768, w_clip_vit=True).eval()
    tab = model.showo.model.embed_tokens.weight
    gg = torch.Generator(device="cuda").manual_seed(100)
    feats = torch.randn(1, 576, 1024, device="cuda", generator=gg)
    sys_ids = torch.randint(0, 50256, (1, 31), device="cuda", generator=gg)  # 30 rows in front of the image, <|eoi|> behind it
    with torch.no_grad():
        img = model.mm_projector(feats)
        txt = tab[sys_ids]
        prefix = torch.cat([txt[:, :30], img, txt[:, 30:]], dim=1).float().contiguous()
        questions = [tab[torch.randint(0, 50256, (1, LQ), device="cuda", generator=gg)].float().contiguous() for _ in range(n_questions)]
    assert prefix.shape[1] == P
    fulls = [torch.cat([prefix, q], dim=1).contiguous() for q in questions]
    fmask = create_attention_mask_for_mmu_vit(fulls[0], system_prompt_len=28)
    assert mmu_prefix_is_exact(fmask, P)
    pmask = create_attention_mask_for_mmu_vit(prefix, system_prompt_len=28)[0]
    return showo_amd, model, prefix, pmask, questions, fulls, fmask[0]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def alternate(variants, reps):
    """variants: name -> fn.  One warm-up of each, then reps rounds in which the variants take turns; name -> (median s, last output)"""
    for fn in variants.values():
        fn()
    ts, outs = {k: [] for k in variants}, {}
    for _ in range(reps):
        for k, fn in variants.items():
            t, outs[k] = wall(fn)
            ts[k].append(t)
    return {k: (statistics.median(v), outs[k]) for k, v in ts.items()}


def ints(rows):
    return [[int(t) for t in r] for r in rows]


def shared_legs(reps, new, short, out, ns=(32, 64), S=32):
    """forked / shared / full-prompt legs at n questions about one image on S wide slots; see the module docstring"""
    pkg, model, prefix, pmask, questions, fulls, fmask = build(max(ns))
    sess = model.mmu_session(input_embeddings=prefix, attention_mask=pmask)
    arch = model.arch
    nL, nH = arch["num_hidden_layers"], arch["num_attention_heads"]
    base = P & ~63
    res = {"shape": f"cfg4: prefix {P} rows, questions of {LQ} rows, {new} new tokens, {S} wide slots, full-size seeded weights",
           "reps": reps, "unit": "tokens/s of the whole call (appends / prefills included), median of reps; step_ms: (t(new) - t(short)) / "
                                 f"(new - short) per n / {S}-slot round", "short": short,
           "from_shapes": {"slot_cache_bytes_forked": 4 * nL * nH * 64 * ((P + LQ + new + 1 + 63) // 64 * 64),
                           "slot_cache_bytes_shared": 4 * nL * nH * 64 * ((P - base + LQ + new + 1 + 63) // 64 * 64),
                           "fork_copy_bytes_each_way_per_request": 4 * nL * nH * 64 * P,
                           "shared_copy_bytes_each_way_per_request": 4 * nL * nH * 64 * LQ}}
    for mode, kw in (("greedy", dict(top_k=1)), ("topk5", dict(top_k=5, temperature=0.7))):
        for n in ns:
            def legs(nt):
                gen = lambda: torch.Generator(device="cuda").manual_seed(11)
                return {"forked": lambda: sess.generate_batch(input_embeddings=questions[:n], max_new_tokens=nt, generator=gen(), slots=S, **kw),
                        "shared": lambda: sess.generate_batch(input_embeddings=questions[:n], max_new_tokens=nt, generator=gen(), slots=S,
                                                              share_prefix=True, **kw)}
            r = alternate(legs(new), reps)
            r_short = alternate(legs(short), reps)
            row = {}
            for k in ("forked", "shared"):
                row[k] = {"seconds": r[k][0], "tokens_per_s": n * new / r[k][0],
                          "step_ms": 1e3 * (r[k][0] - r_short[k][0]) / (new - short) / ((n + S - 1) // S)}
            a_, b_ = ints(r["forked"][1]), ints(r["shared"][1])
            row["requests_with_equal_tokens"] = sum(x == y for x, y in zip(a_, b_))
            row["common_prefix_tokens_mean"] = sum(next((i for i, (u, v) in enumerate(zip(x, y)) if u != v), len(x)) for x, y in zip(a_, b_)) / n
            row["shared_over_forked"] = row["shared"]["tokens_per_s"] / row["forked"]["tokens_per_s"]
            res[f"{mode}_n{n}"] = row
            print(mode, n, row, file=sys.stderr, flush=True)
    # the full-prompt leg replaces the engine's decode cache, which would make the session stale: it runs BEHIND the session legs, on its
    # own (its long and short calls alternating with each other), not in their alternation -- the result says so
    res["full_prompts_leg"] = "measured behind the alternating session legs in the same process, not alternating with them"
    for mode, kw in (("greedy", dict(top_k=1)), ("topk5", dict(top_k=5, temperature=0.7))):
        for n in ns:
            gen = lambda: torch.Generator(device="cuda").manual_seed(11)

            def full(nt):
                return lambda: model.mmu_generate_batch(input_embeddings=fulls[:n], attention_mask=[fmask] * n, max_new_tokens=nt,
                                                        generator=gen(), slots=S, **kw)
            r = alternate({"long": full(new), "short": full(short)}, reps)
            t, ts = r["long"][0], r["short"][0]
            res[f"{mode}_n{n}"]["full_prompts"] = {"seconds": t, "tokens_per_s": n * new / t,
                                                   "step_ms": 1e3 * (t - ts) / (new - short) / ((n + S - 1) // S)}
            print(mode, n, "full prompts", res[f"{mode}_n{n}"]["full_prompts"], file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--new", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--share-prefix", action="store_true", help="measure shared-prefix slots against forked slots and full prompts")
    ap.add_argument("--profile-shared", type=int, default=None, help="one shared greedy call of 17 tokens on this many slots, twice")
    a = ap.parse_args()
    if a.profile_shared is not None:
        S = a.profile_shared
        pkg, model, prefix, pmask, questions, fulls, fmask = build(S)
        sess = model.mmu_session(input_embeddings=prefix, attention_mask=pmask)
        for _ in range(2):
            sess.generate_batch(input_embeddings=questions, max_new_tokens=17, top_k=1, slots=S, share_prefix=True)
        torch.cuda.synchronize()
        print(json.dumps({"profiled": f"sess.generate_batch n={S} greedy slots={S} share_prefix=True, 17 tokens, twice"}))
        return
    if a.share_prefix:
        shared_legs(a.reps or 7, a.new, 36, a.out or os.path.join(ROOT, "profiles", "shared_prefix_bench.json"))
        return
    a.reps = a.reps or 5
    a.out = a.out or os.path.join(ROOT, "profiles", "mmu_prefix_bench.json")
    reps = max(5, a.reps)
    pkg, model, prefix, pmask, questions, fulls, fmask = build(8)
    L = pkg._lib
    res = {"shape": f"cfg4: prefix {P} rows (30 system + 576 image + <|eoi|>), questions of {LQ} rows, full prompt {P + LQ}, greedy, "
                    f"{a.new} new tokens, full-size seeded weights", "reps": reps, "unit": "seconds, median of reps, wall clock between device syncs"}

    # ---- first comparison: k = 4 questions about one image, one after the other
    k = 4

    def full_calls(new):
        return lambda: [model.mmu_generate(input_embeddings=fulls[i], attention_mask=fmask, max_new_tokens=new, top_k=1) for i in range(k)]

    box = {}

    def session_calls(new, with_prefill):
        def run():
            if with_prefill:
                box["s"] = model.mmu_session(input_embeddings=prefix, attention_mask=pmask)
            s, out = box["s"], []
            mark = s.mark()
            for i in range(k):
                out.append(s.generate(input_embeddings=questions[i], max_new_tokens=new, top_k=1))
                s.rewind(mark)
            return out
        return run

    for tag, new in (("first_token", 1), ("whole_call", a.new)):
        # all three take turns in every round; "questions only" comes right behind the variant that opened the session, whose cache
        # it continues (an mmu_generate in between would replace the engine's decode cache and make the session stale)
        r = alternate({"mmu_generate_x4": full_calls(new), "session_prefill_plus_x4": session_calls(new, True),
                       "session_x4_questions_only": session_calls(new, False)}, reps)
        same = ints(r["mmu_generate_x4"][1]) == ints(r["session_prefill_plus_x4"][1])
        res[f"k4_{tag}"] = {"mmu_generate_per_question": r["mmu_generate_x4"][0] / k,
                            "session_per_question_incl_one_prefill": r["session_prefill_plus_x4"][0] / k,
                            "session_per_question_after_the_prefill": r["session_x4_questions_only"][0] / k,
                            "tokens_equal_the_full_prompt_path": same}
        print(tag, res[f"k4_{tag}"], file=sys.stderr, flush=True)

    # ---- second comparison: n questions decoded together
    for n in (4, 8):
        sess = {}

        def batch_full():
            return model.mmu_generate_batch(input_embeddings=fulls[:n], attention_mask=[fmask] * n, max_new_tokens=a.new, top_k=1)

        def batch_sess():
            sess["s"] = model.mmu_session(input_embeddings=prefix, attention_mask=pmask)
            return sess["s"].generate_batch(input_embeddings=questions[:n], max_new_tokens=a.new, top_k=1)

        r = alternate({"mmu_generate_batch": batch_full, "session_generate_batch": batch_sess}, reps)
        res[f"n{n}_batch"] = {"mmu_generate_batch": r["mmu_generate_batch"][0], "session_generate_batch_incl_prefill": r["session_generate_batch"][0],
                              "tokens_equal_the_full_prompt_path": ints(r["mmu_generate_batch"][1]) == ints(r["session_generate_batch"][1])}
        print(f"n={n}", res[f"n{n}_batch"], file=sys.stderr, flush=True)

    # ---- the fork next to the copy kernel on the same byte count
    eng = model.engine()
    model.mmu_session(input_embeddings=prefix, attention_mask=pmask)
    L.call("showo_engine_batch_begin", eng, 1, P + LQ + a.new + 1)
    arch = model.arch
    nbytes = arch["num_hidden_layers"] * arch["num_attention_heads"] * P * 64 * 2 * 2
    src = torch.empty((nbytes,), dtype=torch.uint8, device="cuda").random_()
    dst = torch.empty_like(src)
    # one call is ~100 us, the size of a launch plus a host synchronisation: an interval is CALLS calls queued back to back between
    # two synchronisations, so their overhead is spread over CALLS copies (the same for both kernels)
    CALLS = 50

    def many(fn):
        def run():
            for _ in range(CALLS):
                fn()
        return run

    r = alternate({"kv_fork": many(lambda: L.call("showo_engine_batch_fork", eng, 0, L.stream())),
                   "copy_b128": many(lambda: L.call("showo_copy_b128", L.ptr(src), L.ptr(dst), nbytes, L.stream()))}, max(reps, 9))
    t_fork, t_copy = r["kv_fork"][0] / CALLS, r["copy_b128"][0] / CALLS
    res["fork"] = {"bytes_each_way": nbytes, "calls_per_interval": CALLS, "kv_fork_s": t_fork, "kv_fork_GBps": 2 * nbytes / t_fork / 1e9,
                   "copy_b128_s": t_copy, "copy_b128_GBps": 2 * nbytes / t_copy / 1e9}
    print("fork", res["fork"], file=sys.stderr, flush=True)
    n_, p_, cap_, ep_ = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    L.call("showo_engine_cache_state", eng, C.byref(n_), C.byref(p_), C.byref(cap_), C.byref(ep_))
    assert n_.value == P
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
