"""Host references of the t2i sampler kernels (csrc/sampler.hip), in plain torch / numpy on the CPU.

  ref_sample        CFG combine in fp32 (separate roundings, as the kernel and the reference do), then softmax, p / E and
                    the arg-max in fp64
  ref_mask_by_topk  the expression in the header comment of showo_mask_by_topk, in fp64
  philox4x32_10     numpy replica of common.h (Philox::gen, u32_to_unit): standard Philox4x32-10; with the two builders
                    sampler_exp_noise / topk_uniform it states the kernels' documented counter layout as a contract

test_sampler_ref_cpu.py checks all of it without a GPU (published Philox vectors, the recorded reference trajectory, the
oracle); test_sampler_width_gpu.py holds the kernels against it."""
from collections import namedtuple

import numpy as np
import torch

FLT_MAX = float(np.finfo(np.float32).max)
GAP_TOL = 1e-4      # sampler: rows whose two best reference scores are closer than this (relative) may differ
CONF_TOL = 5e-4     # mask_by_topk: elements whose reference confidence is closer to the cut than this may differ
EXCUSED_CAP = 0.005  # ... but never more than this share of a case

Sample = namedtuple("Sample", "ids sel gap p")
TopK = namedtuple("TopK", "masking margin k conf")


def ref_sample(lc, lu, w, cur, mask_id, E):
    """lc, lu: fp32 [R, V] (lu may be None), cur: int64 [R], E: fp32 [R, V].  Returns ids int64 [R], sel fp64 [R]
    (= p[ids]; FLT_MAX on known rows), gap fp64 [R] (relative gap between the two best scores; inf on known rows) and the
    fp64 probabilities p [R, V] (known rows: zeros)."""
    lc = torch.as_tensor(lc, dtype=torch.float32)
    cur = torch.as_tensor(cur, dtype=torch.int64).reshape(-1)
    R, V = lc.shape
    unknown = cur == mask_id
    if lu is not None:
        z = (1 + w) * lc - w * torch.as_tensor(lu, dtype=torch.float32)  # fp32, each product and the difference rounded
    else:
        z = lc.clone()
    assert z.dtype == torch.float32
    z[~unknown] = 0.0  # the logit rows of known tokens must not matter (the tests fill them with NaN)
    p = z.double().softmax(-1)
    s = (p / torch.as_tensor(E, dtype=torch.float32).reshape(R, V).double()).numpy()
    ids = torch.from_numpy(np.argmax(s, axis=-1))  # first maximal index
    if V > 1:
        top = -np.partition(-s, 1, axis=-1)[:, :2]
        with np.errstate(invalid="ignore", divide="ignore"):
            gap = torch.from_numpy((top[:, 0] - top[:, 1]) / top[:, 0])
    else:
        gap = torch.full((R,), float("inf"), dtype=torch.float64)
    sel = torch.gather(p, -1, ids[:, None])[:, 0]
    ids = torch.where(unknown, ids, cur)
    sel = torch.where(unknown, sel, torch.tensor(FLT_MAX, dtype=torch.float64))
    gap = torch.where(unknown, gap, torch.tensor(float("inf"), dtype=torch.float64))
    p[~unknown] = 0.0
    return Sample(ids, sel, gap, p)


def ref_mask_by_topk(sel, cur, mask_len_f, temp, u, mask_id):
    """sel: fp32 [B, N], cur: int64 [B, N] (before the step), u: fp32 [B, N].
      conf = log(clamp(sel, 1e-20)) + temp * (-log(clamp(-log(clamp(u, 1e-20)), 1e-20)))        (fp64)
      k = max(1, min(#unknown - 1, mask_len_f)) as integer, clamped to N - 1;  cut = sort(conf)[k];  masking = conf < cut
    Returns masking bool [B, N], margin = |conf - cut| fp64 [B, N], k int64 [B], conf fp64 [B, N]."""
    sel = torch.as_tensor(sel, dtype=torch.float32).double()
    u = torch.as_tensor(u, dtype=torch.float32).double()
    cur = torch.as_tensor(cur, dtype=torch.int64)
    B, N = sel.shape
    g = -torch.log((-torch.log(u.clamp(min=1e-20))).clamp(min=1e-20))
    conf = torch.log(sel.clamp(min=1e-20)) + float(temp) * g
    unknown = (cur == mask_id).sum(-1).double()
    k = torch.clamp(torch.minimum(unknown - 1, torch.tensor(float(mask_len_f), dtype=torch.float64)), min=1.0).long()
    k = k.clamp(max=N - 1)
    cut = torch.gather(torch.sort(conf, dim=-1).values, 1, k[:, None])
    return TopK(conf < cut, (conf - cut).abs(), k, conf)


def topk_excused(tk):
    """elements of the random family that a kernel may mask differently: those closer to the cut than CONF_TOL -- but only in a
    sample where the cut element (margin 0) has such a neighbour.  Where it has none, every other element keeps its side of the
    cut under an error below CONF_TOL, the kernel's cut is the same element, and nothing is excused."""
    near = tk.margin <= CONF_TOL
    return near & (near.sum(-1, keepdim=True) > 1)


def apply_mask(masking, sampled, ids_row, img_start, mask_id, id_offset):
    """the write-back of one step: (new cur, new ids row) from a mask"""
    masking = torch.as_tensor(masking).bool()
    N = masking.shape[-1]
    out = ids_row.clone()
    out[:, img_start:img_start + N] = torch.where(masking, torch.tensor(mask_id), sampled + id_offset)
    return torch.where(masking, torch.tensor(mask_id), sampled), out


# ------------------------------------------------------------------------------------------------------------ Philox4x32-10
_M32 = np.uint64(0xFFFFFFFF)
_PM0, _PM1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four broadcastable unsigned arrays (words 0..3), key: (k0, k1).  Returns uint32 [..., 4]."""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in counter])]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = _PM0 * c[0], _PM1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _M32, (p0 >> _S32) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + _W0) & _M32, (k1 + _W1) & _M32
    return np.stack(c, axis=-1).astype(np.uint32)


def u32_to_unit(x):
    """((x >> 8) + 0.5) * 2^-24, every operation in fp32 like common.h"""
    n = (np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    return (n + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def _key(seed):
    return (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)


def sampler_exp_noise(seed, step, rows, V):
    """the Exp(1) draws of cfg_softmax_sample_kernel: element i of row r is lane i & 3 of the block with counter
    (i >> 2, r, step, 0x51); E = -log(u) in fp32.  fp32 [rows, V]"""
    nb = (V + 3) // 4
    r4 = philox4x32_10((np.arange(nb)[None, :], np.arange(rows)[:, None], step, 0x51), _key(seed))  # [rows, nb, 4]
    u = u32_to_unit(r4).reshape(rows, nb * 4)[:, :V]
    return -torch.log(torch.from_numpy(np.ascontiguousarray(u)))  # fp32 log, correctly rounded to within an ulp like logf


def topk_uniform(seed, step, B, N):
    """the uniform draws of mask_by_topk_kernel: element i of sample b is word 0 of the block with counter (i, b, step, 0x6b).
    fp32 [B, N]"""
    r4 = philox4x32_10((np.arange(N)[None, :], np.arange(B)[:, None], step, 0x6B), _key(seed))
    return torch.from_numpy(np.ascontiguousarray(u32_to_unit(r4[..., 0])))


# ------------------------------------------------------------------------------------------------- input families (section 2)
SAMPLER_CASES = [  # (B, N, V, ld, cfg)
    (2, 256, 8192, 8192, True),    # the cfg2 row layout: eight trips of the draw loop
    (1, 64, 1030, 1032, False),    # second trip on a ragged V, rows with a stride
    (1, 64, 4100, 4100, True),     # a partial last trip
    (1, 16, 40000, 40000, True),   # top of the supported range: the 160 000-byte LDS row
]
SAMPLER_FAMILIES = [("wide", 3.0, 5.0, True), ("narrow", 0.5, 0.0, False)]  # (name, logit scale, guidance, with lu)
TOPK_SHAPES = [(2, 256), (4, 1024), (1, 257), (1, 4096)]
TOPK_TEMPS = (4.5, 0.5)


def sampler_inputs(B, N, V, ld, cfg, scale, seed):
    """lc, lu fp32 [B*N, ld] (NaN in the pad columns and in the rows of known tokens), cur int64 [B*N] (about half known,
    mask_id = V), E fp32 [B*N, V]"""
    g = torch.Generator().manual_seed(seed)
    R = B * N
    mask_id = V
    cur = torch.where(torch.rand(R, generator=g) < 0.5, torch.full((R,), mask_id), torch.randint(0, V, (R,), generator=g))
    known = cur != mask_id

    def logits():
        t = torch.full((R, ld), float("nan"))
        t[:, :V] = torch.randn(R, V, generator=g) * scale
        t[known] = float("nan")
        return t
    lc = logits()
    lu = logits() if cfg else None
    E = torch.empty(R, V).exponential_(generator=g)
    return lc, lu, cur, mask_id, E


def mask_len_values(N):
    return (0.0, 1.0, float(int(0.3 * N)), float(N - 2), float(N + 5))


def unknown_counts(N):
    return (0, 1, 2, N // 2, N)


def topk_inputs(B, N, n_unknown, seed, mask_id=8192):
    """sel = rand^4 on unknown positions (FLT_MAX on known ones), sampled, cur, u"""
    g = torch.Generator().manual_seed(seed)
    cur = torch.randint(0, mask_id, (B, N), generator=g)
    for b in range(B):
        cur[b, torch.randperm(N, generator=g)[:n_unknown]] = mask_id
    sampled = torch.where(cur == mask_id, torch.randint(0, mask_id, (B, N), generator=g), cur)
    sel = torch.where(cur == mask_id, torch.rand(B, N, generator=g) ** 4, torch.tensor(FLT_MAX))
    u = torch.rand(B, N, generator=g)
    return sel, sampled, cur, u
