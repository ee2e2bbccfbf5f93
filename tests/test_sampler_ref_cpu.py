"""The host references that test_sampler_width_gpu.py holds the sampler kernels against (tests/sampler_ref.py), checked without
a GPU: the Philox replica against the published Random123 known-answer vectors, ref_sample / ref_mask_by_topk against every step
of the recorded reference trajectory and against the oracle, and the share of near-tie inputs in every input family of the GPU
tests (what those tests may excuse) against the caps they state."""
import numpy as np
import torch

import util
from util import O
import sampler_ref as R


def test_philox_replica_matches_the_random123_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in R.philox4x32_10(ctr, key)) == want
    # vectorised = element by element, and the counter words are not interchangeable
    c0, c1 = np.arange(5)[None, :], np.arange(3)[:, None]
    blk = R.philox4x32_10((c0, c1, 7, 0x51), (123, 9))
    assert blk.shape == (3, 5, 4) and blk.dtype == np.uint32
    for r in range(3):
        for i in range(5):
            assert np.array_equal(blk[r, i], R.philox4x32_10((i, r, 7, 0x51), (123, 9)))
    assert len({tuple(v) for v in blk.reshape(-1, 4).tolist()}) == 15
    assert not np.array_equal(R.philox4x32_10((1, 2, 7, 0x51), (123, 9)), R.philox4x32_10((2, 1, 7, 0x51), (123, 9)))


def test_unit_interval_map_and_the_draw_builders():
    x = np.array([0, 255, 256, 0x7fffffff, 0x80000000, 0xfffffeff], dtype=np.uint32)
    u = R.u32_to_unit(x)
    assert u.dtype == np.float32 and u[0] == u[1] == np.float32(2.0 ** -25) and u[2] == np.float32(1.5 * 2.0 ** -24)
    assert np.all(u > 0) and np.all(u < 1)
    # the map is common.h's, fp32 step by step: above 2^23 the "+ 0.5" is rounded away (ties to even), and the top 256 words reach
    # 1.0 (probability 2^-24 per draw; the sampler's E = -log(1) is then -0 and that column cannot win).  The replica keeps it.
    assert R.u32_to_unit(np.uint32(0xffffffff)) == np.float32(1.0) and R.u32_to_unit(np.uint32(0xfffffeff)) < np.float32(1.0)
    # seed words: low word is key 0, high word key 1 (a seed above 2^32 uses both)
    seed = (5 << 32) | 77
    E = R.sampler_exp_noise(seed, 3, 2, 10)
    assert E.dtype == torch.float32 and tuple(E.shape) == (2, 10) and bool((E > 0).all())
    r4 = R.philox4x32_10((2, 1, 3, 0x51), (77, 5))  # element 9 of row 1 = lane 1 of block 2
    assert float(E[1, 9]) == float(-torch.log(torch.tensor(R.u32_to_unit(r4[1]))))
    U = R.topk_uniform(seed, 3, 2, 10)
    assert float(U[1, 9]) == float(R.u32_to_unit(R.philox4x32_10((9, 1, 3, 0x6B), (77, 5))[0]))
    # rows, steps, seeds and the two kernels each have a stream of their own
    a = R.sampler_exp_noise(seed, 0, 4, 64)
    assert len(set(a.reshape(-1).tolist())) > 250
    assert not torch.equal(a, R.sampler_exp_noise(seed, 1, 4, 64)) and not torch.equal(a, R.sampler_exp_noise(77, 0, 4, 64))


def test_references_reproduce_the_recorded_trajectory():
    """every step of tests/golden/showo_tiny_t2i.npz from its fwd_logits, exp_noise and uniform: the multinomial draws and the
    next step's fwd_in"""
    g = util.golden("showo_tiny_t2i.npz")
    d = util.tiny_dims()
    steps, w = int(g["steps"]), float(g["guidance"])
    B, N, V = g["ids_cond"].shape[0], d.num_vq_tokens, d.codebook
    off, mask_id = d.image_offset, d.mask_token_id
    Lseq = g["ids_cond"].shape[1]
    img0 = Lseq - (N + 1)
    for s in range(steps):
        ids_in = torch.from_numpy(g["fwd_in"][s])
        lg = torch.from_numpy(g["fwd_logits"][s])[:, img0:img0 + N, off:off + V].contiguous()
        cur = ids_in[:B, img0:img0 + N].clone()
        cur = torch.where(cur == mask_id, cur, cur - off)
        smp = R.ref_sample(lg[:B].reshape(B * N, V), lg[B:].reshape(B * N, V), w, cur.reshape(-1), mask_id,
                           torch.from_numpy(g["exp_noise"][s]).reshape(B * N, V))
        unknown = (cur == mask_id).reshape(-1)
        assert torch.equal(smp.ids[unknown], torch.from_numpy(g["multinomial"][s]).reshape(-1)[unknown])
        assert torch.equal(smp.ids[~unknown], cur.reshape(-1)[~unknown]) and bool((smp.sel[~unknown] == R.FLT_MAX).all())
        assert float(smp.gap[unknown].min()) > R.GAP_TOL  # the recorded draws are no near-ties
        tk = R.ref_mask_by_topk(smp.sel.float().view(B, N), cur, float(g["mask_len"][s]), float(g["temps"][s]),
                                torch.from_numpy(g["uniform"][s]).view(B, N), mask_id)
        new_cur, ids_c = R.apply_mask(tk.masking, smp.ids.view(B, N), ids_in[:B], img0, mask_id, off)
        want = torch.from_numpy(g["fwd_in"][s + 1])[:B] if s + 1 < steps else torch.from_numpy(g["final_input_ids"])
        assert torch.equal(ids_c, want), f"step {s}"
        assert torch.equal(new_cur == mask_id, tk.masking)
    assert torch.equal(smp.ids.view(B, N), torch.from_numpy(g["result"]))


def test_ref_mask_by_topk_agrees_with_the_oracle():
    mask_id = 8192
    n = 0
    for B, N in ((2, 256), (1, 257), (3, 64)):
        for nu in R.unknown_counts(N):
            for ml in R.mask_len_values(N):
                for temp in R.TOPK_TEMPS + (0.0,):
                    sel, sampled, cur, u = R.topk_inputs(B, N, nu, seed=n, mask_id=mask_id)
                    tk = R.ref_mask_by_topk(sel, cur, ml, temp, u, mask_id)
                    unknown = (cur == mask_id).sum(-1, keepdim=True)
                    k = torch.max(torch.tensor([1]), torch.min(unknown - 1, torch.tensor([ml]))).clamp(max=N - 1)  # reference :171
                    assert torch.equal(k.long()[:, 0], tk.k)
                    want = O.mask_by_random_topk(k, sel.double(), temp, u.double())
                    assert torch.equal(tk.masking, want)
                    assert int(tk.masking.sum(-1).max()) <= int(tk.k.max())  # conf < cut is strict: at most k
                    n += 1
    # fp32 oracle = fp64 reference outside the margin
    sel, sampled, cur, u = R.topk_inputs(4, 1024, 512, seed=99)
    tk = R.ref_mask_by_topk(sel, cur, 300.0, 4.5, u, mask_id)
    want32 = O.mask_by_random_topk(tk.k[:, None], sel, 4.5, u)
    far = tk.margin > R.CONF_TOL
    assert torch.equal(tk.masking[far], want32[far])


def test_ref_sample_agrees_with_the_oracle_draw():
    """RecordedNoise.multinomial (argmax(p / E) in fp32) on the fp32 softmax = ref_sample outside the near-ties"""
    lc, lu, cur, mask_id, E = R.sampler_inputs(1, 64, 1030, 1032, True, 3.0, seed=5)
    V = 1030
    smp = R.ref_sample(lc[:, :V], lu[:, :V], 5.0, cur, mask_id, E)
    unknown = cur == mask_id
    z = (1 + 5.0) * lc[unknown, :V] - 5.0 * lu[unknown, :V]
    want = O.RecordedNoise([E[unknown]], None).multinomial(z.softmax(-1))
    ok = smp.gap[unknown] > R.GAP_TOL
    assert torch.equal(smp.ids[unknown][ok], want[ok]) and int(ok.sum()) >= 0.99 * int(unknown.sum())
    assert torch.allclose(smp.sel[unknown][ok].float(), torch.gather(z.softmax(-1), -1, want[:, None])[:, 0][ok], rtol=2e-5)
    assert torch.equal(smp.ids[~unknown], cur[~unknown])


def test_near_ties_of_the_gpu_input_families_stay_inside_the_caps():
    """what the GPU tests may excuse, measured on the reference alone: rows with a top-2 gap below GAP_TOL, elements closer to the
    cut than CONF_TOL; each at most EXCUSED_CAP of its case"""
    for ci, (B, N, V, ld, cfg) in enumerate(R.SAMPLER_CASES):
        for name, scale, w, with_lu in R.SAMPLER_FAMILIES:
            lc, lu, cur, mask_id, E = R.sampler_inputs(B, N, V, ld, cfg and with_lu, scale, seed=100 + ci)
            smp = R.ref_sample(lc[:, :V], None if lu is None else lu[:, :V], w, cur, mask_id, E)
            unknown = cur == mask_id
            near = int((smp.gap[unknown] < R.GAP_TOL).sum())
            print(f"[parity] sampler family {name} V={V}: {near} of {int(unknown.sum())} rows with top-2 gap < {R.GAP_TOL}")
            assert near <= R.EXCUSED_CAP * int(unknown.sum())
    for B, N in R.TOPK_SHAPES:
        worst = 0.0
        for nu in R.unknown_counts(N):
            for ml in R.mask_len_values(N):
                for temp in R.TOPK_TEMPS:
                    sel, sampled, cur, u = R.topk_inputs(B, N, nu, seed=N + nu)
                    tk = R.ref_mask_by_topk(sel, cur, ml, temp, u, 8192)
                    worst = max(worst, float(R.topk_excused(tk).float().mean()))
        print(f"[parity] mask_by_topk random family B={B} N={N}: worst share of elements within {R.CONF_TOL} of the cut {worst:.5f}")
        assert worst <= R.EXCUSED_CAP
