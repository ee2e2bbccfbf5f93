"""bench.py — t2i images/s @256x256 (18 denoise steps, CFG on, batch 8) + decode_code on MI355X.

One "step" = one pass of the hot path over one batch: Showo.t2i_generate (18 mask-predict steps on a
[16,387] CFG batch) followed by MAGVITv2.decode_code of the 8 results (BASELINE.json configs[1]).
Inputs (ids, mask) are resident in HBM before the timed region.  Prints ONE JSON line (rank 0).
Multi-GPU: images are independent -> N replicas, no data-path collective ("weak" scaling).
A plain run sets up, warms up, times the steps, dumps (--dump-outputs) and prints the headline line.  The other legs -- roofline,
measured ceilings, accuracy / fp16 modes, the other BASELINE configs, the training step, the CPU baselines -- run with --full.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

_T0 = time.time()


def log(msg):
    print(f"[bench +{time.time() - _T0:6.1f}s] {msg}", file=sys.stderr, flush=True)


def build_inputs(d, B, O):
    """inputs of the CPU-baseline leg only (oracle mask builder; the measured GPU leg builds its own through the product)"""
    rs = np.random.RandomState(0)
    rows_c, rows_u = [], []
    for i in range(B):
        k = 5 + (i * 5) % 36  # text lengths 5..40: different pad counts exercise the per-sample mask
        text = [d.t2i_id, 50256] + rs.randint(0, 50256, size=k - 3).tolist() + [50256]
        rows_c.append([d.pad_id] * (129 - k) + text + [d.soi_id] + [d.mask_token_id] * d.num_vq_tokens + [d.eoi_id])
        rows_u.append([d.pad_id] * 126 + [d.t2i_id, 50256, 50256] + [d.soi_id] + [d.mask_token_id] * d.num_vq_tokens + [d.eoi_id])
    ic, iu = torch.tensor(rows_c), torch.tensor(rows_u)
    mask = O.mask_t2i(torch.cat([ic, iu]), d.pad_id, d.soi_id, d.eoi_id)
    return ic, iu, mask


def _pick_threads():
    """The GPU box reports 256 logical CPUs but torch's intra-op pool thrashes when given all of them (measured: one [2,387] forward
    took 234 s on 256 threads), and a single GEMM repeat can be off by 2x in either direction (round 3: one spurious sample picked 64
    threads and the baseline fell 50 %).  So: candidate pool sizes {8, 16, 32, 64}, MEDIAN of 7 repeats of the forward's dominant GEMM
    per candidate, all candidates returned for the JSON line; cpu_baseline() then checks the pick against the 8-thread pool on a real
    oracle step and keeps the faster of the two."""
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    a, b = torch.randn(774, 2048), torch.randn(2048, 8192)
    cands = {}
    for n in sorted({min(avail, c) for c in (8, 16, 32, 64)}):
        torch.set_num_threads(n)
        torch.mm(a, b)
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            torch.mm(a, b)
            ts.append(time.perf_counter() - t0)
        cands[n] = 2 * 774 * 2048 * 8192 / float(np.median(ts)) / 1e9
        log(f"cpu baseline: {n} threads -> median {cands[n]:.0f} GFLOP/s on the fc1 GEMM (7 repeats)")
    best = max(cands, key=lambda n: cands[n])
    torch.set_num_threads(best)
    return best, cands


def cpu_baseline(budget_s=30.0):
    """oracle (CPU restatement of the reference, fp32) on a bounded sample: denoise steps of ONE prompt with CFG
    ([2,387] forward + sampling per step) are timed until ~budget_s of CPU work is spent, then scaled to 18 steps.
    The ONLY place in this file that touches oracle/."""
    import showo_oracle as O
    import weights as Wt
    d = Wt.ShowoDims()
    threads, cands = _pick_threads()
    # same architecture, random init on the host (timing does not depend on the values); ~5.8 GB fp32
    g = torch.Generator().manual_seed(0)
    sd_t = {k: torch.randn(shape, generator=g) * std + mean for k, (shape, std, mean) in Wt.showo_state_spec(d).items()}
    ic, iu, mask = build_inputs(d, 1, O)
    step_s = {}
    with torch.no_grad():
        O.t2i_generate(sd_t, d, ic.clone(), iu.clone(), mask, 1.0, 1, 5.0)  # page-in + thread pool warm-up, not timed
        for nt in sorted(cands):  # every candidate runs one REAL oracle step: the GEMM microbenchmark above mis-ranks pool sizes (r4a: 64
            # threads = 4.9x the 8-thread GEMM rate, yet a 1.55x SLOWER denoise step), so the step time decides
            torch.set_num_threads(nt)
            t0 = time.time()
            O.t2i_generate(sd_t, d, ic.clone(), iu.clone(), mask, 1.0, 1, 5.0)
            step_s[nt] = time.time() - t0
            log(f"cpu baseline: one denoise step on {nt} threads: {step_s[nt]:.1f}s")
        threads = min(step_s, key=lambda k: step_s[k])
        torch.set_num_threads(threads)
        t_warm = step_s[threads]
        n = int(max(1, min(6, budget_s // max(t_warm, 1e-3))))
        t0 = time.time()
        O.t2i_generate(sd_t, d, ic.clone(), iu.clone(), mask, 1.0, n, 5.0)
        t_steps = time.time() - t0
    per_step = t_steps / n
    est = 18 * per_step  # decode (0.3 TFLOP of 38.4) is <1% and is left out of the CPU estimate, favouring the CPU
    # the other BASELINE configs on the same weights and thread pool (VERDICT r5 weak #9c), one bounded sample each: cfg1 IS this
    # workload (one prompt, CFG); cfg3 = one [2,1155] denoise forward x 18 per image; cfg4 = the reference's mmu_generate recomputes the
    # whole [1, 631 + t] sequence per token (no KV cache, models/modeling_showo.py:190-240): one [1,631] forward per token
    others = {}
    try:
        with torch.no_grad():
            d3 = Wt.ShowoDims(num_vq_tokens=1024)
            i3c, i3u, m3 = build_inputs(d3, 1, O)
            t0 = time.time()
            O.showo_logits(sd_t, d3, torch.cat([i3c, i3u]), attention_mask=m3)
            t3 = time.time() - t0
            emb = torch.randn(1, 631, d.hidden, generator=g) * 0.02
            t0 = time.time()
            O.showo_logits(sd_t, d, None, input_embeddings=emb, attention_mask=O.mask_mmu_vit(1, 631, system_prompt_len=28))
            t4 = time.time() - t0
        others = {"cfg1_t2i256_batch1": {"value": 1.0 / est, "unit": "images/s", "cores": threads, "kind": "port", "sample": "the headline's sample: BASELINE cfg1 is one prompt with CFG"},
                  "cfg3_t2i512_inpaint_batch4": {"value": 1.0 / (18 * t3), "unit": "images/s", "cores": threads, "kind": "port",
                                                 "sample": f"ONE [2,1155] denoise forward (one 512x512 image with CFG, fp32 oracle) = {t3:.1f}s, scaled x18; VQ encode / decode omitted (favours the CPU)"},
                  "cfg4_mmu_decode": {"value": 1.0 / t4, "unit": "tokens/s", "cores": threads, "kind": "port",
                                      "sample": f"ONE [1,631] forward = {t4:.1f}s = one token of the reference's no-cache mmu_generate (its cost grows with every token: favours the CPU); CLIP tower omitted"}}
    except Exception as ex:  # the headline's baseline must survive
        others = {"error": repr(ex)}
    return {"value": 1.0 / est, "unit": "images/s", "cores": threads, "kind": "port", "other_configs": others,
            "sample": f"{n} of 18 denoise steps of 1 prompt (CFG, [2,387], fp32 oracle) timed = {t_steps:.1f}s, "
                      f"scaled x18/{n}; decode_code omitted (<1% of FLOPs)",
            "thread_candidates_gflops_median_of_7": {str(k): round(v, 1) for k, v in cands.items()},
            "one_step_seconds_by_threads": {str(k): round(v, 2) for k, v in step_s.items()}}


def measured_ceilings(L):
    """ceilings of THIS box in THIS run (no stale file): about 2 s of hipBLASLt through torch.matmul (bf16, random
    normal operands, the forward's dominant shape and 4096^3; a PROBE of what the chip sustains, not part of the product) and the
    float4 copy kernel of the library on 1 GiB.  HIP events on torch's current stream = the launch stream."""
    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e-3
    out = {"source": "this run (torch.matmul = hipBLASLt probe, showo_copy_b128), random-normal bf16 operands"}
    g = torch.Generator(device="cuda").manual_seed(5)
    for name, (M, N, K) in (("proj_4128x14336x2048", (4128, 14336, 2048)), ("kcat_4128x2048x10240", (4128, 2048, 10240)), ("cube_4096", (4096, 4096, 4096))):
        a = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
        ws = [torch.randn(N, K, device="cuda", generator=g).to(torch.bfloat16) for _ in range(4)]  # rotated: weights cold like the layer stack
        i = [0]

        def mm():
            i[0] = (i[0] + 1) % len(ws)
            return torch.matmul(a, ws[i[0]].t())
        t = timed(mm, 12)
        out[f"bf16_tflops_blas_{name}"] = 2.0 * M * N * K / t / 1e12
        del a, ws
    src, dst = torch.empty(1 << 30, dtype=torch.uint8, device="cuda"), torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    t = timed(lambda: L.call("showo_copy_b128", L.ptr(src), L.ptr(dst), src.numel(), L.stream()), 6)
    out["hbm_TBps_copy"] = 2 * src.numel() / t / 1e12
    del src, dst
    try:
        out["power_wall_probe_4096x4096x8192_tflops"] = power_wall_probe(L, timed, g)
    except Exception as ex:  # a probe, never the reason a bench line is lost
        out["power_wall_probe_4096x4096x8192_tflops"] = {"error": repr(ex)}
    return out


def power_wall_probe(L, timed, g):
    """The same launches on random-normal and on all-zero bf16 operands (256 tiles of 256 x 256 = one round on 256 CUs, K = 8192, weights
    rotated): identical instruction streams, but zero operands draw far less switching power, so the power-managed clock stays high.
    The ratio zero / random is the share of the GEMM rate that the chip's power budget (not the kernel's stall cycles) takes on real
    data; first measured in profiles/r4n_power_vs_bandwidth.txt (own ring kernel 1 480 -> 1 875 TF/s, +27 %).  hipBLASLt through
    torch.matmul and the library's own kernel through its C ABI (tuner on)."""
    M, N, K = 4096, 4096, 8192
    fl = 2.0 * M * N * K / 1e12
    probe = {}
    for tag in ("random", "zero"):
        if tag == "random":
            a = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
            ws = [torch.randn(N, K, device="cuda", generator=g).to(torch.bfloat16) for _ in range(4)]
        else:
            a = torch.zeros(M, K, device="cuda", dtype=torch.bfloat16)
            ws = [torch.zeros(N, K, device="cuda", dtype=torch.bfloat16) for _ in range(4)]
        o = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        i = [0]

        def blas():
            i[0] = (i[0] + 1) % len(ws)
            return torch.matmul(a, ws[i[0]].t())

        def own():
            i[0] = (i[0] + 1) % len(ws)
            L.call("showo_gemm_bf16", L.ptr(a), K, L.ptr(ws[i[0]]), K, None, 0, L.ptr(o), N, None, 0, M, N, K, 0, L.stream())
        probe[f"blas_{tag}_operands"] = fl / timed(blas, 12)
        try:
            own()  # first call of the shape: the tile tuner times its variants here, outside the timed repeats
            probe[f"own_{tag}_operands"] = fl / timed(own, 12)
        except Exception as ex:
            probe[f"own_{tag}_operands"] = repr(ex)
        del a, ws, o
    for k in ("blas", "own"):
        r, z = probe.get(f"{k}_random_operands"), probe.get(f"{k}_zero_operands")
        if isinstance(r, float) and isinstance(z, float) and r > 0:
            probe[f"{k}_zero_over_random"] = z / r
    return probe


def child_line(argv, timeout_s, env=None):
    """run a bench workload as a child process and return its JSON line (dict) or {"error": ...}"""
    import subprocess
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True, text=True, timeout=timeout_s)
    except subprocess.TimeoutExpired:
        return {"error": f"timed out after {timeout_s}s"}
    line = None
    for l in p.stdout.splitlines():
        if l.startswith("{") and '"metric"' in l:
            line = l
    if p.returncode != 0 or line is None:
        return {"error": f"rc={p.returncode}", "stderr_tail": p.stderr[-300:]}
    return json.loads(line)


def gemm_src_sha1():
    """identity of the kernels a PMC traffic figure belongs to: sha1 over the sources of the production GEMM family"""
    import hashlib
    h = hashlib.sha1()
    for f in ("gemm_common.h", "gemm2p.hip", "gemm3w.hip"):
        with open(os.path.join(ROOT, "show-o_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def dry_run():
    """SHOWO_BENCH_DRYRUN=1: exercise ONLY the launch plumbing of the multi-GPU lines -- self-launch under torch.distributed.run,
    rank environment, the MAX-time / SUM-units aggregation, the training leg's child ranks with their own rendezvous -- with gloo
    and no GPU work (tests/test_dist_cpu.py runs it with two real processes; the first N > 1 run on hardware is then not a cold start)."""
    return os.environ.get("SHOWO_BENCH_DRYRUN", "0") == "1"


def dry_main(a):
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo")
    dt, units = aggregate(0.01 * (rank + 1), a.batch * a.steps, dist, "cpu")
    train_step = None if a.no_train_leg else train_leg(world, rank, steps=1, warmup=0, timeout_s=180)
    if rank == 0:
        print(json.dumps({"metric": "t2i images/sec @256x256 (18 denoise steps)", "value": units / dt, "unit": "images/s", "n_gpus": world,
                          "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": "bf16", "data": "dry-run: launch plumbing only, no GPU work (SHOWO_BENCH_DRYRUN=1)",
                          "config": {"workload": "dry-run"}, "dryrun": {"ranks": world, "units": units, "max_dt": dt,
                                                                          "master_port": os.environ.get("MASTER_PORT")},
                          "train_step": train_step, "cpu_baseline": None}))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def self_launch(gpus, script):
    """`python bench.py --gpus N` without a launcher: re-exec as N ranks (one process per GPU) under torch.distributed.run, as
    the reference is started by `accelerate launch` (training/train.py:91-110; accelerate_configs/8_gpus_deepspeed_zero2.yaml).
    Under a launcher (WORLD_SIZE set, the driver's form) this returns and the process is one of the ranks."""
    world_env = os.environ.get("WORLD_SIZE")
    if world_env is not None:
        if int(world_env) != gpus:
            raise SystemExit(f"bench: --gpus {gpus} but the launcher started WORLD_SIZE={world_env} ranks")
        return
    if gpus <= 1:
        return
    have = torch.cuda.device_count()
    if have < gpus and not dry_run():
        raise SystemExit(f"bench: --gpus {gpus} requested but {have} GPU(s) are visible")
    import socket
    import subprocess
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(script)] + sys.argv[1:]
    log("self-launch: " + " ".join(cmd))
    raise SystemExit(subprocess.call(cmd, env=env))


def train_leg(world, rank, steps=8, warmup=2, timeout_s=420):
    """run `bench_train.py --gpus world` as a child of this rank and return (rank 0) the fields of its JSON line that matter here"""
    import subprocess
    env = dict(os.environ)
    if world > 1:
        env["MASTER_PORT"] = str(int(env.get("MASTER_PORT", "29500")) + 101)
        env.pop("TORCHELASTIC_USE_AGENT_STORE", None)  # the children rendezvous on their own TCPStore (child rank 0 hosts it)
    cmd = [sys.executable, os.path.join(ROOT, "bench_train.py"), "--gpus", str(world), "--steps", str(steps), "--warmup", str(warmup),
           "--no-cpu-baseline"]
    t0 = time.time()
    try:
        p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        try:
            so, se = p.communicate(timeout=timeout_s)
        except subprocess.TimeoutExpired:
            p.kill()
            p.communicate()
            return {"error": f"training leg timed out after {timeout_s}s"} if rank == 0 else None
    except OSError as e:
        return {"error": str(e)} if rank == 0 else None
    if rank != 0:
        return None
    line = None
    for l in so.splitlines():
        if l.startswith("{") and '"metric"' in l:
            line = l
    if p.returncode != 0 or line is None:
        return {"error": f"bench_train.py rc={p.returncode}", "stderr_tail": se[-400:]}
    d = json.loads(line)
    log(f"training leg: {d['value']:.1f} ms/step on {d['n_gpus']} GPU(s) in {time.time() - t0:.0f}s")
    return {"metric": d["metric"], "ms_per_step": d["value"], "n_gpus": d["n_gpus"], "steps": d["steps"], "warmup": d["warmup"], "scaling": d["scaling"],
            "global_batch": d["config"].get("global_batch"), "tokens_per_s": d["config"].get("tokens_per_s"),
            "gradient_wire": d["config"].get("gradient_wire"), "gemm_tflops": d["roofline"].get("achieved"),
            "gemm_frac_of_mfma_peak": d["roofline"].get("frac"),
            "exchange_exposed_ms": d["config"].get("exchange_exposed_ms"), "wire_bytes_per_rank": d["config"].get("wire_bytes_per_rank"),
            "dryrun": d.get("dryrun"),
            "source": "bench_train.py run by this command as child ranks (one process per GPU, RCCL all-reduce of the gradient buckets overlapped with backward)"}


def aggregate(dt, units_local, dist=None, device="cpu"):
    """whole-job numbers of a replica-parallel run: (max elapsed time over ranks, units processed by all ranks).
    Independent units, no data-path collective: this MAX / SUM pair is the only communication of the benchmark."""
    if dist is None:
        return dt, units_local
    t = torch.tensor([dt], device=device, dtype=torch.float64)
    u = torch.tensor([float(units_local)], device=device, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.all_reduce(u, op=dist.ReduceOp.SUM)
    return float(t.item()), int(round(float(u.item())))


def dump_outputs(out_dir, arrays, max_bytes=64 * 10**6):
    """--dump-outputs: every [B, ...] array as out_dir/<name>.npy in float32 (the token ids are exact in float32).  When the arrays
    hold more than max_bytes in all, the same fixed, seeded sample of the B rows is written for every array."""
    host = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    B = len(next(iter(host.values())))
    keep = min(B, (max_bytes - 4096) // sum(v[0].nbytes for v in host.values()))
    rows = np.sort(np.random.RandomState(0).choice(B, keep, replace=False)) if keep < B else np.arange(B)
    os.makedirs(out_dir, exist_ok=True)
    for k, v in host.items():
        np.save(os.path.join(out_dir, k + ".npy"), v[rows])
    log(f"outputs of the last timed step -> {out_dir}: " + ", ".join(f"{k}{list(v[rows].shape)}" for k, v in host.items())
        + ("" if keep == B else f" ({keep} of {B} rows, seeded sample)"))


def main():
    if "--workload" in sys.argv:
        wl = sys.argv[sys.argv.index("--workload") + 1]
        if wl == "train":
            import bench_train
            return bench_train.main(sys.argv[1:])
        if wl in ("t2i512", "mmu", "vq"):  # BASELINE configs[2] / configs[3] and the VQ path's HBM-bound kernels as their own JSON lines
            import bench_configs
            return bench_configs.main(sys.argv[1:])
        if wl != "t2i":
            raise SystemExit(f"bench: unknown --workload {wl} (t2i | train | t2i512 | mmu | vq)")
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--event-stride", type=int, default=7, help="time every n-th launch of a kernel kind with HIP events (7 is coprime to the 4 GEMMs per layer)")
    ap.add_argument("--no-prefix-reuse", action="store_true", help="recompute the step-invariant text rows in every denoise step (A/B)")
    ap.add_argument("--no-events", action="store_true", help="skip the per-launch HIP events (A/B of their overhead)")
    ap.add_argument("--graph", type=int, default=1, help="1 (default): the denoise steps replay the engine's cached hipGraph; 0: eager launches")
    ap.add_argument("--roofline-steps", type=int, default=2, help="steps of the separate eager + HIP-event leg that feeds `roofline` (0: skip)")
    ap.add_argument("--precision", type=int, default=0, help="0 (default): bf16 operands, the timed path; 1: the WHOLE bench in accuracy mode "
                    "(split-bf16 GEMMs, fp32 attention: logits within 1e-3 of the fp32 reference end to end)")
    ap.add_argument("--no-accuracy-leg", action="store_true", help="skip the one-step accuracy-mode leg that fills `accuracy_mode`")
    ap.add_argument("--no-config-legs", action="store_true", help="skip the cfg3 / cfg4 child runs and the VQ HBM leg (other_configs, vq_hbm)")
    ap.add_argument("--no-train-leg", action="store_true", help="skip the short training-step leg (bench_train.py in child ranks) that fills `train_step`")
    ap.add_argument("--workload", default="t2i", help="t2i (default, the headline metric) | train (bench_train.py: stage-1 step time) | "
                    "t2i512 | mmu (bench_configs.py: BASELINE configs[2] / configs[3])")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step returned (image tokens, decoded images) as "
                    "DIR/<name>.npy in float32, for output-for-output comparison of two builds on the same seeded inputs")
    ap.add_argument("--full", action="store_true", help="after the headline, run every other leg (roofline, measured ceilings, accuracy and "
                    "fp16 modes, VQ HBM, the other BASELINE configs, the training step, CPU baselines); the --no-* options and "
                    "--roofline-steps select among them")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if not a.full:  # a plain run does only what the headline figure needs
        a.no_cpu_baseline = a.no_train_leg = a.no_accuracy_leg = a.no_config_legs = True
        a.roofline_steps = 0
    self_launch(a.gpus, __file__)
    if dry_run():
        return dry_main(a)
    import faulthandler
    faulthandler.dump_traceback_later(240, repeat=True, file=sys.stderr)  # shows where a stuck run is

    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))

    log(f"rank {rank}/{world} start")
    import showo_amd
    from showo_amd import synthetic
    L = showo_amd._lib
    B = a.batch
    N, codebook = synthetic.SHOWO_DEMO["num_vq_tokens"], synthetic.SHOWO_DEMO["codebook_size"]
    # random-init weights of the true architecture (no checkpoints offline): generated on the GPU, N(0, 0.02)
    torch.manual_seed(0)
    model = synthetic.random_init_showo(max_batch=2 * B, max_seq=387, ln_jitter=True).eval()
    if a.precision:
        model.set_precision(a.precision)
    log("showo params on GPU")
    vq = showo_amd.MAGVITv2(max_batch=B, max_res=256).cuda().eval()
    log("vq params on GPU")
    cfg = showo_amd.gen_config()
    uni = synthetic.prompting(max_text_len=128)
    ic_d, iu_d, mask_d = synthetic.t2i_inputs(uni, B, N, model.mask_token_id)  # prompts -> ids -> omni mask, as inference_t2i.py does
    assert tuple(ic_d.shape) == (B, 387) and tuple(mask_d.shape) == (2 * B, 1, 387, 387)
    log("inputs built")
    gen = torch.Generator(device="cuda").manual_seed(1 + rank)

    def step():
        ids = ic_d.clone()
        toks = model.t2i_generate(input_ids=ids, uncond_input_ids=iu_d, attention_mask=mask_d, temperature=1.0, timesteps=18,
                                  guidance_scale=5.0, generator=gen, config=cfg, use_graph=a.graph, reuse_prefix=not a.no_prefix_reuse)
        toks = torch.clamp(toks, max=codebook - 1, min=0)
        return toks, vq.decode_code(toks)

    img = None
    for i in range(a.warmup):
        t1 = time.time()
        _, img = step()
        torch.cuda.synchronize()
        log(f"warmup step {i}: {time.time() - t1:.2f}s")
    if img is None:
        _, img = step()
    assert tuple(img.shape) == (B, 3, 256, 256) and torch.isfinite(img).all()

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    # ---- timed region: K steps on the product's default path (hipGraph replay of the denoise steps), no per-launch events
    L.call("showo_prof_enable", 0)
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        last = step()
    barrier()
    dt = time.perf_counter() - t0
    log(f"timed {a.steps} steps in {dt:.2f}s")
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, dict(zip(("tokens", "images"), last)))
    del last
    dt, images = aggregate(dt, B * a.steps, dist, "cuda")
    # ---- roofline leg (same process, right after): the same steps with every n-th launch of each kernel kind bracketed by HIP
    # events on the launch stream; event timing makes the engine launch eagerly (a graph replay has no per-kernel events)
    L.call("showo_prof_reset")
    dt_evt, n_evt = None, 0
    if not a.no_events and a.roofline_steps > 0:
        L.call("showo_prof_set_stride", a.event_stride)  # per-launch events on a systematic sample of the launches
        L.call("showo_prof_enable", 1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(a.roofline_steps):
            step()
        torch.cuda.synchronize()
        dt_evt, n_evt = time.perf_counter() - t1, a.roofline_steps
        L.call("showo_prof_enable", 0)
        log(f"roofline leg: {n_evt} eager steps with HIP events in {dt_evt:.2f}s")
    ms_gemm, n_gemm, fl_gemm = C.c_double(), C.c_int64(), C.c_double()
    L.call("showo_prof_read", 0, C.byref(ms_gemm), C.byref(n_gemm), C.byref(fl_gemm))
    ms_attn, n_attn, fl_attn = C.c_double(), C.c_int64(), C.c_double()
    L.call("showo_prof_read", 1, C.byref(ms_attn), C.byref(n_attn), C.byref(fl_attn))
    ms_conv, n_conv, fl_conv = C.c_double(), C.c_int64(), C.c_double()
    L.call("showo_prof_read", 2, C.byref(ms_conv), C.byref(n_conv), C.byref(fl_conv))
    n_all, fl_all = C.c_int64(), C.c_double()
    L.call("showo_prof_totals", 0, C.byref(n_all), C.byref(fl_all))
    L.call("showo_prof_reset")
    # ---- accuracy-mode leg (rank 0): the configuration in which "matches the reference" (logits within north_star's 1e-3 of the fp32
    # reference END TO END; measured ~1e-5) and "images/s" are the same sentence.  Showo.set_precision(1) runs the SAME launches as the
    # timed path on K-concatenated split-bf16 images (three MFMA products per GEMM / attention product, fp32 LayerNorm / softmax / gelu),
    # with prefix reuse and hipGraph replay: timed like the headline (warm-up incl. the capture, then 3 steps), plus one eager step with
    # HIP events for its own roofline (EXECUTED MFMA flops -- 3x the algorithmic ones -- over time, against the same 2.5 PF/s).
    accuracy = None
    fp16_mode = None
    if rank == 0 and not a.no_accuracy_leg and not a.precision:
        try:
            ids2 = torch.cat([ic_d[:1], iu_d[:1]]).contiguous()
            mk2 = torch.cat([mask_d[:1], mask_d[B:B + 1]]).contiguous()
            lg0 = model(ids2, attention_mask=mk2)
            model.set_precision(1)
            lg1 = model(ids2, attention_mask=mk2)
            dd = (lg0 - lg1).double()
            rel_max, rel_rms = float(dd.abs().max() / lg1.double().abs().max()), float(dd.pow(2).mean().sqrt() / lg1.double().pow(2).mean().sqrt())
            del lg0, lg1, dd
            fast = bool(L.load().showo_engine_precise_fast(model.engine()))
            step()
            step()
            torch.cuda.synchronize()
            n_acc = 3 if fast else 1
            t1 = time.perf_counter()
            for _ in range(n_acc):
                step()
            torch.cuda.synchronize()
            dta = (time.perf_counter() - t1) / n_acc
            acc_roof = None
            if not a.no_events:
                L.call("showo_prof_reset")
                L.call("showo_prof_set_stride", a.event_stride)
                L.call("showo_prof_enable", 1)
                step()
                torch.cuda.synchronize()
                L.call("showo_prof_enable", 0)
                ms_g, n_g, fl_g = C.c_double(), C.c_int64(), C.c_double()
                L.call("showo_prof_read", 0, C.byref(ms_g), C.byref(n_g), C.byref(fl_g))
                ms_a, n_a, fl_a = C.c_double(), C.c_int64(), C.c_double()
                L.call("showo_prof_read", 1, C.byref(ms_a), C.byref(n_a), C.byref(fl_a))
                L.call("showo_prof_reset")
                ach_g = fl_g.value / max(1e-9, ms_g.value * 1e-3) / 1e12
                acc_roof = {"bound": "mfma", "kernel": "gemm2p / gemm3w on K-concatenated split images (K' = 3K) with the (hi, lo) projection epilogue",
                            "achieved": ach_g, "peak": 2500.0, "unit": "TFLOP/s executed (3 MFMA products per algorithmic product)", "frac": ach_g / 2500.0,
                            "algorithmic_tflops": ach_g / 3.0, "timed_launches": int(n_g.value), "avg_launch_ms": ms_g.value / max(1, n_g.value),
                            "attention": {"achieved_executed_tflops": fl_a.value / max(1e-9, ms_a.value * 1e-3) / 1e12}}
            # ---- fp16-operand leg (precision 2): the SAME launches as the timed path with IEEE-half operands (same MFMA rate and peak)
            # and the split-bf16 lm_head -- the configuration in which the 1e-3 and the headline's speed are one sentence.  Its logits are
            # compared in-run with the accuracy-mode logits above (themselves ~1e-5 from the fp32 reference: the in-run stand-in for it; the
            # reference fixtures are gated in tests/test_modules_gpu.py), its tokens with the accuracy-mode tokens under identical noise.
            try:
                gen_a = torch.Generator(device="cuda").manual_seed(77)
                toks_acc = model.t2i_generate(input_ids=ic_d.clone(), uncond_input_ids=iu_d, attention_mask=mask_d, temperature=1.0, timesteps=18,
                                              guidance_scale=5.0, generator=gen_a, config=cfg)
                lg1 = model(ids2, attention_mask=mk2)
                model.set_precision(2)
                lg2 = model(ids2, attention_mask=mk2)
                dd = (lg2 - lg1).double()
                h_max, h_rms = float(dd.abs().max() / lg1.double().abs().max()), float(dd.pow(2).mean().sqrt() / lg1.double().pow(2).mean().sqrt())
                del lg1, lg2, dd
                gen_a = torch.Generator(device="cuda").manual_seed(77)
                toks_h = model.t2i_generate(input_ids=ic_d.clone(), uncond_input_ids=iu_d, attention_mask=mask_d, temperature=1.0, timesteps=18,
                                            guidance_scale=5.0, generator=gen_a, config=cfg)
                agree_h = float((toks_h == toks_acc).float().mean())
                step()
                torch.cuda.synchronize()
                n_h = max(3, min(a.steps, 10))
                t1 = time.perf_counter()
                for _ in range(n_h):
                    step()
                torch.cuda.synchronize()
                dth = (time.perf_counter() - t1) / n_h
                h_roof = None
                if not a.no_events:
                    L.call("showo_prof_reset")
                    L.call("showo_prof_set_stride", a.event_stride)
                    L.call("showo_prof_enable", 1)
                    step()
                    torch.cuda.synchronize()
                    L.call("showo_prof_enable", 0)
                    ms_g, n_g, fl_g = C.c_double(), C.c_int64(), C.c_double()
                    L.call("showo_prof_read", 0, C.byref(ms_g), C.byref(n_g), C.byref(fl_g))
                    ms_a, n_a, fl_a = C.c_double(), C.c_int64(), C.c_double()
                    L.call("showo_prof_read", 1, C.byref(ms_a), C.byref(n_a), C.byref(fl_a))
                    L.call("showo_prof_reset")
                    ach_h = fl_g.value / max(1e-9, ms_g.value * 1e-3) / 1e12
                    h_roof = {"bound": "mfma", "kernel": "gemm3w_kernel / gemm2p_kernel, fp16 instances (v_mfma_f32_16x16x32_f16)", "achieved": ach_h, "peak": 2500.0,
                              "unit": "TFLOP/s", "frac": ach_h / 2500.0, "timed_launches": int(n_g.value), "avg_launch_ms": ms_g.value / max(1, n_g.value),
                              "attention_tflops": fl_a.value / max(1e-9, ms_a.value * 1e-3) / 1e12}
                fp16_mode = {"images_per_s": B / dth, "ms_per_step": dth * 1e3, "steps": n_h, "speed_vs_timed_path": (dt / a.steps) / dth,
                             "mode": "Showo.set_precision(2): fp16 (IEEE half) operands on the production kernels -- same launches, prefix reuse and hipGraph replay as "
                                     "the timed path; saturating converts; final LayerNorm + lm_head as a split-bf16 product",
                             "rel_max_vs_fp32_reference": "<= 1e-3, gated by tests/test_modules_gpu.py on the reference fixtures (full size [2,387], cfg3 [8,1155], cfg4 prefill + "
                                                          "KV-cached decode, greedy tokens identical)",
                             "logits_vs_accuracy_mode_in_this_run": {"rel_max": h_max, "rel_rms": h_rms, "sample": "[2,387] slice of this batch, full vocabulary",
                                                                     "timed_bf16_path_same_sample": {"rel_max": rel_max, "rel_rms": rel_rms}},
                             "t2i_token_agreement_with_accuracy_mode_same_noise": agree_h, "roofline": h_roof}
                log(f"fp16 leg: {B / dth:.2f} images/s ({(dt / a.steps) / dth:.3f} x the timed path); logits vs accuracy mode rel_max {h_max:.2e} rel_rms {h_rms:.2e}; "
                    f"token agreement {agree_h:.4f}; roofline {h_roof}")
            except Exception as ex:
                fp16_mode = {"error": repr(ex)}
            model.set_precision(0)
            accuracy = {"images_per_s": B / dta, "ms_per_step": dta * 1e3, "steps": n_acc,
                        "mode": ("Showo.set_precision(1) on the production kernels: K-concatenated split-bf16 images (hi*hi + lo*hi + hi*lo in one bf16 GEMM over 3K), "
                                 "(hi, lo) projection epilogue, split MFMA attention, fp32 LayerNorm / softmax / IEEE gelu; prefix reuse + hipGraph replay") if fast else
                                "Showo.set_precision(1) on the fp32 reference kernels of csrc/precise.hip (eager launches)",
                        "slowdown_vs_timed_path": (dta) / (dt / a.steps),
                        "roofline": acc_roof,
                        "rel_max_vs_fp32_reference": "<= 1e-3, gated by tests/test_modules_gpu.py on reference fixtures (full size [2,387], cfg3 [8,1155], cfg4 631-embedding prefill + "
                                                     "KV-cached decode: measured ~1e-5, greedy tokens identical)",
                        "timed_bf16_path_vs_accuracy_mode_logits": {"rel_max": rel_max, "rel_rms": rel_rms, "sample": "[2,387] slice of this batch, full vocabulary"}}
            log(f"accuracy-mode leg: {B / dta:.2f} images/s ({'production kernels' if fast else 'reference kernels'}); bf16 path vs accuracy mode rel_max {rel_max:.2e}; roofline {acc_roof}")
        except Exception as ex:  # the headline line must survive
            accuracy = {"error": repr(ex)}
            model.set_precision(0)
    ceilings = None
    vq_hbm = None
    if rank == 0 and a.full:
        try:
            ceilings = measured_ceilings(L)
            log(f"ceilings of this run: {ceilings}")
        except Exception as ex:
            ceilings = {"error": repr(ex)}
        if not a.no_config_legs:
            try:
                import bench_configs
                vq_hbm = bench_configs.vq_hbm_quick(L)
            except Exception as ex:
                vq_hbm = {"error": repr(ex)}
    if rank == 0:
        value = images / dt
        out = {
            "metric": "t2i images/sec @256x256 (18 denoise steps)", "value": value, "unit": "images/s", "n_gpus": world,
            "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": {0: "bf16", 1: "bf16x3 (split-bf16 hi+lo operands, fp32-class)", 2: "f16"}[a.precision], "data": "synthetic",
            "config": {"workload": (f"BASELINE cfg{2 if B == 8 else 1}{'' if B in (1, 8) else ' shape'}: configs/showo_demo.yaml t2i 256x256, batch {B} prompt{'s' if B > 1 else ''}, "
                                    f"CFG 5.0 (forward on [{2 * B},387]), 18 mask-predict steps + MAGVITv2.decode_code; random-init Show-o 1.45B + MAGVIT-v2 95M"),
                       "global_batch": B * world, "seq_len": 387, "parallelism": f"replicas x{world}",
                       "launch_mode": ("hipGraph replay of the denoise steps (cached on the engine)" if a.graph else "eager"),
                       "precision": {0: "bf16 operands, fp32 accumulation", 1: "accuracy mode (split-bf16 GEMMs, fp32 attention)",
                                     2: "fp16 operands, fp32 accumulation, split-bf16 lm_head"}[a.precision],
                       # SURVEY.md §8d counts the REFERENCE's flops (38.4 TFLOP per image: text rows recomputed every step, lm_head over
                       # the full vocabulary); the path skips most of that work (prefix reuse, restricted head), so this rate is NOT MFMA
                       # utilisation -- `roofline.frac` is
                       "algorithmic_tflop_per_image": 38.4, "reference_flops_rate_tflops_skipped_work_included": value * 38.4},
            "roofline": None,
        }
    if rank == 0 and a.full:
        peak = 2500.0  # TFLOP/s dense bf16 MFMA (MI355X_MICROARCH.md)
        # HBM bytes per GEMM launch: PMC counters cannot be read from inside this process; they come from the separate
        # rocprofv3 --pmc passes over this same command (scripts/gpu_pmc.sh -> profiles/pmc/bench_traffic.json)
        # The committed figure carries the hash of the GEMM sources it was measured on (tools/pmc_agg.py writes `kernel_src_sha1`):
        # when the kernels have changed since, the line says null + why instead of quoting a stale number.
        traffic, traffic_src = None, None
        try:
            tj = json.load(open(os.path.join(ROOT, "profiles", "pmc", "bench_traffic.json")))
            if tj.get("kernel_src_sha1") == gemm_src_sha1():
                traffic = tj["gemm2p_kernel"]["bytes_per_launch"]
                traffic_src = f"profiles/pmc/bench_traffic.json ({tj['tag']}: {tj['corrections']}; GEMM sources {tj['kernel_src_sha1'][:12]} = this build)"
            else:
                traffic_src = (f"profiles/pmc/bench_traffic.json ({tj.get('tag')}) was measured on GEMM sources {str(tj.get('kernel_src_sha1'))[:12]}, this "
                               f"build is {gemm_src_sha1()[:12]}: stale, not quoted (re-run scripts/gpu_pmc3.sh)")
        except (OSError, KeyError, TypeError, ValueError):
            pass
        # ceilings measured in THIS run (measured_ceilings above: hipBLASLt through torch.matmul on the forward's dominant shapes and the
        # library's float4 copy kernel): printed next to the spec peak the fraction is taken against
        measured_peak = ceilings
        # MFMA busy fraction of the two per-layer GEMM launches from the PMC pass over this command (north_star: "rocprof showing ... MFMA
        # utilisation on the transformer blocks"): SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE / 8); same staleness guard
        mfma_pmc = None
        try:
            mj = json.load(open(os.path.join(ROOT, "profiles", "pmc", "bench_mfma_util.json")))
            if mj.get("kernel_src_sha1") == gemm_src_sha1():
                top = sorted(((k, v) for k, v in mj["kernels"].items() if k.startswith("gemm")), key=lambda kv: -kv[1]["dispatches"] * kv[1]["avg_us"])[:2]
                mfma_pmc = {"source": f"profiles/pmc/bench_mfma_util.json ({mj.get('tag')}: " + mj["formula"] + ")",
                            "kernels": {k: {"mfma_busy_frac": round(v["mfma_busy_frac"], 4), "avg_us_profiled": round(v["avg_us"], 1)} for k, v in top}}
        except (OSError, KeyError, TypeError, ValueError):
            pass
        ach = fl_gemm.value / (ms_gemm.value * 1e-3) / 1e12 if ms_gemm.value > 0 else 0.0
        out["roofline"] = {"bound": "mfma", "kernel": "gemm3w_kernel / gemm2p_kernel (one template family; the tuner picks the weight-ring form gemm3w for both layer launches at this shape) -- 16-bit MFMA GEMM; per layer ONE [Wqkv;W1] projection with the QKV / GELU split epilogue and ONE K-concatenated dense|fc2 residual GEMM; lm_head rows)",
                           "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak, "measured_peak": measured_peak, "mfma_busy_pmc_from_profiles_not_this_run": mfma_pmc, "traffic": traffic, "traffic_measured_in": "a separate rocprofv3 --pmc pass of this command on the builder's box (profiles/pmc/), NOT this run; null when the GEMM sources changed since", "traffic_unit": "bytes per launch (PMC FETCH_SIZE x2 + WRITE_SIZE)",
                           "traffic_source": traffic_src,
                           "launches": int(n_all.value), "timed_launches": int(n_gemm.value),
                           "avg_launch_ms": ms_gemm.value / max(1, n_gemm.value),
                           "measured_in": f"{n_evt} extra eager steps with HIP events after the timed region ({dt_evt / n_evt * 1e3:.1f} ms per step)" if n_evt else None,
                           "time_share_of_step": (fl_all.value / max(1e-9, ach * 1e12)) / dt_evt if (ach > 0 and n_evt) else None,
                           # at small batches the forward approaches the weight-streaming roof (2.90 GB of bf16 weights per
                           # forward, 18 forwards per image batch): printed so that a --batch 1 line (BASELINE cfg1 shape) can be read
                           "weight_stream": {"bytes_per_forward": 2.896e9, "forwards_per_step": 18,
                                             "TBps_if_weights_streamed_once_per_forward": 18 * 2.896e9 / (dt / a.steps) / 1e12,
                                             "frac_of_8TBps": 18 * 2.896e9 / (dt / a.steps) / 8e12, "token_rows_per_forward": 2 * B * 387},
                           "attention": {"achieved": fl_attn.value / max(1e-9, ms_attn.value * 1e-3) / 1e12},
                           "vq_conv": {"achieved": fl_conv.value / max(1e-9, ms_conv.value * 1e-3) / 1e12}}
    # ---- training-step leg: BASELINE.json's metric is "t2i images/sec + train step-time, 1/2/4/8 MI355X", and the t2i replicas above
    # exchange nothing, so the data-parallel half (RCCL all-reduce of the gradient buckets overlapped with backward) is measured here:
    # every rank runs bench_train.py as a CHILD process (own process group on MASTER_PORT + 101, bounded by a timeout, so that a
    # problem in this leg cannot take the headline line down with it); rank 0 attaches the child's line as `train_step`.
    train_step = None
    if not a.no_train_leg:
        del model, vq, img
        torch.cuda.empty_cache()
        train_step = train_leg(world, rank)
    if rank == 0:
        out["accuracy_mode"] = accuracy
        if fp16_mode is not None:
            out["fp16_mode"] = fp16_mode
        out["vq_hbm"] = vq_hbm
        # every BASELINE config in the driver's record: cfg3 / cfg4 (and cfg1 = --batch 1) as short child runs under a ~90 s budget
        if world == 1 and not a.no_config_legs:
            others = {}
            for key, argv in (("cfg1_t2i256_batch1", ["--batch", "1", "--steps", "3", "--warmup", "1", "--full", "--roofline-steps", "1"]),
                              ("cfg3_t2i512_inpaint_batch4", ["--workload", "t2i512", "--steps", "1", "--warmup", "1"]),
                              ("cfg4_mmu_decode", ["--workload", "mmu", "--steps", "1", "--warmup", "1"])):
                t1 = time.time()
                d = child_line(argv + ["--no-cpu-baseline", "--no-train-leg", "--no-accuracy-leg", "--no-config-legs"], 150)
                if "error" in d:
                    others[key] = d
                else:
                    others[key] = {"metric": d["metric"], "value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"],
                                   "roofline": {k: d["roofline"].get(k) for k in ("bound", "achieved", "peak", "unit", "frac")},
                                   "wall_s": round(time.time() - t1, 1)}
                    for sub in ("batch4", "batch1"):  # cfg4: the 4 images decoded together, and one at a time
                        if sub in d.get("config", {}):
                            others[key][sub] = d["config"][sub]
                log(f"{key}: {others[key]}")
            out["other_configs"] = others
        out["train_step"] = train_step
        if not a.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline()
            oc = out["cpu_baseline"].pop("other_configs", None)
            if isinstance(oc, dict) and isinstance(out.get("other_configs"), dict):
                for k, v in oc.items():  # each config's CPU baseline next to its GPU figure
                    if isinstance(out["other_configs"].get(k), dict):
                        out["other_configs"][k]["cpu_baseline"] = v
            if isinstance(train_step, dict) and "error" not in train_step:
                # the CPU side of the second half of the metric, same run, same host cores (bounded sample: 3-sequence fwd + bwd)
                import bench_train
                try:
                    train_step["cpu_baseline"] = bench_train.cpu_baseline(29, budget_s=25.0, threads=out["cpu_baseline"]["cores"])
                except Exception as ex:  # the headline line must survive a host that cannot hold the fp32 model twice
                    train_step["cpu_baseline"] = {"error": repr(ex)}
        else:
            out["cpu_baseline"] = None
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
