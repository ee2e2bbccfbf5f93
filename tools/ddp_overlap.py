"""How much of the gradient all-reduce can hide behind the backward when the UNCHANGED reference loop trains this model under
DistributedDataParallel (accelerator.prepare, reference training/train.py:449; accelerator.backward, :612)?

Runs the autograd step of the full-size model -- Showo.forward(labels=...) -> w_t2i loss_t2i + w_lm loss_lm + w_mmu loss_mmu ->
loss.backward() -> torch.optim.AdamW with the reference's two parameter groups -- wrapped in DDP, with a comm hook that records a GPU
event on the compute stream when DDP hands it a ready bucket (then returns the plain all-reduce).  A second event is recorded right
after the last backward phase (showo_train_backward_embed + the embedding gradient's hand-out, i.e. when the embedding table's
gradient is accumulated).  Per DDP bucket the tool reports:

  window_ms  GPU time between the bucket's hook and the end of the backward = how long its all-reduce can run behind compute;
  and per step: tail_ms = GPU time from the end of the backward to the end of loss.backward() (DDP waits for its collectives and
  copies the averaged buckets back: the exposed part), step ms with DDP and step ms of `Trainer.step` (phased backward, overlapped
  exchange, native AdamW) on the same batch.

One process = one rank.  Without RANK / WORLD_SIZE in the environment it runs as a one-rank RCCL group (the all-reduce moves no data:
the windows are what the backward offers); under torchrun on N GPUs the same numbers show what stays exposed.

    python tools/ddp_overlap.py [--steps 3] [--warmup 2] [--batch 15,4,10]
    torchrun --nproc-per-node 8 tools/ddp_overlap.py"""
import argparse
import json
import os
import random
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

COEFFS = (1.0, 0.1, 1.0)  # training/train.py:600 with the stage-1 coefficients
NO_DECAY = ("bias", "layer_norm.weight", "mlm_ln.weight", "embeddings.weight")  # training/train.py:211


def _group():
    import torch.distributed as dist
    if "RANK" not in os.environ:
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    return dist, local


def _bucket_label(names):
    """'head', 'block 23', 'blocks 20-23 + head', 'embed' ... from the parameter names DDP put into one bucket"""
    parts = set()
    for n in names:
        if ".layers." in n:
            parts.add(int(n.split(".layers.")[1].split(".")[0]))
        elif "embed_tokens" in n:
            parts.add("embed")
        else:
            parts.add("head")
    blocks = sorted(p for p in parts if isinstance(p, int))
    out = []
    if "head" in parts:
        out.append("head")
    if blocks:
        out.append(f"block {blocks[0]}" if len(blocks) == 1 else f"blocks {blocks[0]}-{blocks[-1]}")
    if "embed" in parts:
        out.append("embed")
    return " + ".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2, help=">= 2: DDP rebuilds its buckets from the gradient order of its first iteration")
    ap.add_argument("--batch", default="15,4,10", help="t2i,lm,mmu rows (bench_train.py's stage-1 batch by default) x 387 tokens")
    ap.add_argument("--bucket-cap-mb", type=float, default=25.0, help="DDP bucket_cap_mb (accelerate passes DDP's default, 25)")
    ap.add_argument("--wire", default="bf16", help="gradient wire of Trainer.step's exchange (world > 1)")
    a = ap.parse_args(argv)
    if a.warmup < 2:
        ap.error("--warmup must be >= 2")
    dist, local = _group()
    rank, world = dist.get_rank(), dist.get_world_size()
    import showo_amd
    from showo_amd import synthetic
    from showo_amd.training_utils import build_training_batch
    from torch.distributed.algorithms.ddp_comm_hooks import default_hooks
    from torch.nn.parallel import DistributedDataParallel
    bt, bl, bm = (int(x) for x in a.batch.split(","))
    torch.manual_seed(0)  # same initial weights on every rank
    model = synthetic.random_init_showo(max_batch=bt + bl + bm, max_seq=387).train()
    uni = synthetic.prompting(max_text_len=128, cond_dropout_prob=0.1)
    off = len(uni.text_tokenizer)
    N, codebook = synthetic.SHOWO_DEMO["num_vq_tokens"], synthetic.SHOWO_DEMO["codebook_size"]
    cfg = type("Cfg", (), {"training": type("Training", (dict,), {"__getattr__": dict.__getitem__})(min_masking_rate=0.0)})
    rs = np.random.RandomState(4 + rank)
    torch.manual_seed(4 + rank)
    random.seed(4 + rank)
    # captions of 2..37 words, LM documents longer than the sequence, 126-word answers (bench_train.py's synthetic batch)
    tx_t2i = [synthetic.random_text(rs, 2 + (i * 5) % 36) for i in range(bt)]
    tx_lm = [synthetic.random_text(rs, 400) for _ in range(bl)]
    tx_mmu = [synthetic.random_text(rs, 126) for _ in range(bm)]
    codes = torch.randint(0, codebook, (bt + bm, N), device="cuda") + off  # the frozen VQ encode is not part of this comparison

    def batch():
        return build_training_batch(uni, cfg, model.mask_token_id, showo_amd.cosine_schedule, codes[:bt], list(tx_t2i), list(tx_lm),
                                    codes[bt:], list(tx_mmu))

    def timed(fn, n):
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    # ---- Trainer.step (native path) on the same batch
    trainer = showo_amd.Trainer(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, coeffs=COEFFS, wire=a.wire)

    def trainer_step():
        ids, labels, mask, _, (b1, b2, b3) = batch()
        trainer.step(ids, mask, labels, b1, b2, b3, 128)

    for _ in range(a.warmup):
        trainer_step()
    trainer_ms = timed(trainer_step, a.steps)
    trainer.close()
    del trainer

    # ---- DDP autograd step (what the unchanged train.py runs under accelerate with N > 1 processes)
    ddp = DistributedDataParallel(model, device_ids=[local], bucket_cap_mb=a.bucket_cap_mb)
    named = list(model.named_parameters())
    name_of = {p.data_ptr(): n for n, p in named}
    opt = torch.optim.AdamW([{"params": [p for n, p in named if not any(x in n for x in NO_DECAY)], "weight_decay": 0.01},
                             {"params": [p for n, p in named if any(x in n for x in NO_DECAY)], "weight_decay": 0.0}],
                            lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
    rec = {"hooks": [], "end": None}

    def hook(state, bucket):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        rec["hooks"].append((bucket.index(), bucket.buffer().numel() * bucket.buffer().element_size(),
                             _bucket_label(name_of[p.data_ptr()] for p in bucket.parameters()), e))
        return default_hooks.allreduce_hook(state, bucket)

    def end_of_backward(p):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        rec["end"] = e

    ddp.register_comm_hook(None, hook)
    model.showo.model.embed_tokens.weight.register_post_accumulate_grad_hook(end_of_backward)

    def ddp_step(measure=None):
        ids, labels, mask, _, (b1, b2, b3) = batch()
        rec["hooks"], rec["end"] = [], None
        _, l1, l2, l3 = ddp(ids, attention_mask=mask, labels=labels, batch_size_t2i=b1, batch_size_lm=b2, batch_size_mmu=b3,
                            max_seq_length=128)
        opt.zero_grad(set_to_none=True)
        loss = COEFFS[0] * l1 + COEFFS[1] * l2 + COEFFS[2] * l3
        t0 = torch.cuda.Event(enable_timing=True)
        t0.record()
        loss.backward()
        t1 = torch.cuda.Event(enable_timing=True)
        t1.record()
        opt.step()
        if measure is not None:
            measure.append((t0, list(rec["hooks"]), rec["end"], t1))

    for _ in range(a.warmup):
        ddp_step()
    ddp_ms = timed(ddp_step, a.steps)
    samples = []
    for _ in range(a.steps):  # event leg after the timed region
        ddp_step(samples)
    torch.cuda.synchronize()

    per_bucket = {}
    tails, bwds = [], []
    for t0, hooks, end, t1 in samples:
        bwds.append(t0.elapsed_time(end))
        tails.append(end.elapsed_time(t1))
        for order, (idx, nbytes, label, e) in enumerate(hooks):
            d = per_bucket.setdefault(idx, {"bucket": idx, "order": order, "MB": nbytes / 2 ** 20, "params": label, "w": []})
            d["w"].append(e.elapsed_time(end))
    rows = sorted(per_bucket.values(), key=lambda d: d["order"])
    if rank == 0:
        print(f"ddp_overlap: world {world}, batch {bt}+{bl}+{bm} x 387, DDP bucket_cap_mb {a.bucket_cap_mb}, {a.steps} steps "
              f"(after {a.warmup} warm-up)")
        print(f"{'order':>5} {'bucket':>6} {'MB':>8}  {'window_ms (hook -> end of backward)':>36}  params")
        for d in rows:
            print(f"{d['order']:>5} {d['bucket']:>6} {d['MB']:>8.1f}  {np.mean(d['w']):>36.2f}  {d['params']}")
        print(f"backward (loss.backward() start -> last backward phase): {np.mean(bwds):.2f} ms GPU; "
              f"tail after it (DDP waits + copy-back, exposed): {np.mean(tails):.2f} ms GPU")
        print(f"step: DDP autograd + torch AdamW {ddp_ms:.1f} ms, Trainer.step {trainer_ms:.1f} ms")
        print(json.dumps({"tool": "ddp_overlap", "world": world, "batch": [bt, bl, bm], "seq": 387, "bucket_cap_mb": a.bucket_cap_mb,
                          "steps": a.steps, "ddp_step_ms": round(ddp_ms, 2), "trainer_step_ms": round(trainer_ms, 2),
                          "trainer_wire": a.wire if world > 1 else None, "backward_ms": round(float(np.mean(bwds)), 2),
                          "tail_ms": round(float(np.mean(tails)), 2),
                          "buckets": [{"order": d["order"], "bucket": d["bucket"], "MB": round(d["MB"], 1), "params": d["params"],
                                       "window_ms": round(float(np.mean(d["w"])), 2)} for d in rows]}))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
