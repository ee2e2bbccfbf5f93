"""The t2i sampler kernels (csrc/sampler.hip: cfg_softmax_sample_kernel, mask_by_topk_kernel) at production width and at their
edges, against the host references of tests/sampler_ref.py (checked on their own, without a GPU, by test_sampler_ref_cpu.py).

  1. injected noise: the draw loop over several trips, ragged V, strided rows, the LDS ceiling; the rank-counting cut at
     N = 256 .. 4096 with every clamp of k; exact first-index tie-breaks across lanes, waves and trips; exact ties at the cut
  2. the on-device Philox draws against a host replica of the documented counter layout (no recorded streams)
  3. through the engine at the production head width (codebook 8192, N = 256 / 1024) on a narrow body: eager (noise offset on
     the host) and hipGraph replay (offset on the device) against the references evaluated on the GPU's own step-0 logits

Tolerances.  Sampler: ids equal the fp64 reference except on rows whose two best reference scores are closer than 1e-4 relative
(more than 20 times the largest fp32 term between kernel and reference: the rounding of z - max at |z - max| <= 64 is 2^-18
relative in exp), at most 0.5 % of a case's unknown rows; sel within rtol 2e-5.  mask_by_topk: the mask equals the reference on
every element farther than 5e-4 from the cut (10 times the fp32 budget of conf: two logf at magnitudes up to 88, a product, a
sum), at most 0.5 % of a case's elements excused.  The tie families are exact."""
import numpy as np
import pytest
import torch

import util
from util import dev
import sampler_ref as R

pytestmark = pytest.mark.gpu

FLT_MAX32 = torch.tensor(R.FLT_MAX, dtype=torch.float32)


def L():
    return util.lib()


def S():
    return util.lib().stream()


def _sample(lc, lu, ld, w, cur, mask_id, E, seed, step, B, N, V):
    """showo_cfg_softmax_sample on host tensors; returns (sampled int64 [B*N], sel fp32 [B*N]) on the host"""
    sampled = torch.full((B * N,), -7, dtype=torch.int64, device="cuda")
    sel = torch.full((B * N,), -1.0, dtype=torch.float32, device="cuda")
    L().call("showo_cfg_softmax_sample", L().ptr(dev(lc)), None if lu is None else L().ptr(dev(lu)), ld, float(w), L().ptr(dev(cur)),
             mask_id, None if E is None else L().ptr(dev(E)), seed, step, L().ptr(sampled), L().ptr(sel), B, N, V, S())
    torch.cuda.synchronize()
    return sampled.cpu(), sel.cpu()


def _check_sample(got, sel, smp, cur, mask_id, label):
    """the section-2 rules; returns the number of excused rows"""
    unknown = cur == mask_id
    assert torch.equal(got[~unknown], cur[~unknown]), f"{label}: a known row lost its id"
    assert bool((sel[~unknown] == FLT_MAX32).all()), f"{label}: a known row's confidence is not FLT_MAX"
    assert int(got[unknown].min()) >= 0
    mism = (got != smp.ids) & unknown
    near = smp.gap < R.GAP_TOL
    excused = int((mism & near).sum())
    worst = float(smp.gap[mism].min()) if bool(mism.any()) else float("inf")
    n_unknown = int(unknown.sum())
    print(f"[parity] {label}: {int(mism.sum())} of {n_unknown} unknown rows differ from the fp64 reference, {excused} excused "
          f"(top-2 gap < {R.GAP_TOL}), smallest gap among them {worst:.3e}; smallest gap of the case {float(smp.gap.min()):.3e}")
    assert int((mism & ~near).sum()) == 0, f"{label}: sampled ids differ on rows that are no near-tie"
    assert excused <= R.EXCUSED_CAP * n_unknown
    p_got = torch.gather(smp.p, -1, got.clamp(min=0, max=smp.p.shape[1] - 1)[:, None])[:, 0]
    err = ((sel.double() - p_got).abs() / p_got)[unknown]
    print(f"[parity] {label}: sel vs p_ref[sampled] rel_max={float(err.max()):.3e}")
    assert float(err.max()) <= 2e-5
    return excused


# ------------------------------------------------------------------------------------------- sampler, injected noise
@pytest.mark.parametrize("case", range(len(R.SAMPLER_CASES)), ids=["cfg2-layout", "ragged-strided", "partial-trip", "lds-ceiling"])
def test_sampler_at_width_against_fp64_reference(case):
    B, N, V, ld, cfg = R.SAMPLER_CASES[case]
    for name, scale, w, with_lu in R.SAMPLER_FAMILIES:
        lc, lu, cur, mask_id, E = R.sampler_inputs(B, N, V, ld, cfg and with_lu, scale, seed=100 + case)
        assert 0.3 < float((cur == mask_id).float().mean()) < 0.7 or B * N <= 16
        got, sel = _sample(lc, lu, ld, w, cur, mask_id, E, 0, 0, B, N, V)
        smp = R.ref_sample(lc[:, :V], None if lu is None else lu[:, :V], w, cur, mask_id, E)
        _check_sample(got, sel, smp, cur, mask_id, f"sampler {name} B={B} N={N} V={V} ld={ld} cfg={lu is not None}")


def test_sampler_refuses_a_row_beyond_the_lds_ceiling():
    V = 40001
    lc = torch.zeros(1, V)
    sampled = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    sel = torch.full((1,), -1.0, device="cuda")
    cur = dev(torch.tensor([V]))
    with pytest.raises(RuntimeError, match="V out of range"):
        L().call("showo_cfg_softmax_sample", L().ptr(dev(lc)), None, V, 0.0, L().ptr(cur), V, None, 0, 0, L().ptr(sampled), L().ptr(sel), 1, 1, V, S())
    torch.cuda.synchronize()
    assert int(sampled[0]) == -7 and float(sel[0]) == -1.0  # no launch


def test_sampler_tie_breaks_are_exact():
    """first maximal index, whichever lane, wave or loop trip holds the contenders (index i: trip i // 1024, thread (i % 1024) // 4)"""
    V = 8192
    pairs = [(5000, 77), (1023, 1024), (4095, 4096), (8191, 3)]
    g = torch.Generator().manual_seed(3)
    rows, want = [], []
    rows.append(torch.zeros(V)); want.append(0)            # flat
    rows.append(torch.full((V,), 3.5)); want.append(0)
    for a, b in pairs:
        r = torch.randn(V, generator=g)
        r[a] = r[b] = 20.0
        rows.append(r); want.append(min(a, b))
    r = torch.full((V,), float("-inf")); r[6000] = -2.5                               # one live column
    rows.append(r); want.append(6000)
    n_unknown = len(rows)
    rows.append(torch.full((V,), float("nan"))); want.append(4242)  # a known row at the end
    lc = torch.stack(rows)
    cur = torch.full((len(rows),), V, dtype=torch.int64)
    cur[-1] = 4242
    E = torch.ones(len(rows), V)
    E[n_unknown - 1] = torch.empty(V).exponential_(generator=g)  # the -inf row: whatever E is
    lu_eq = lc.clone()          # z = 6 l - 5 l: equal logits stay equal
    lu_eq[n_unknown - 1] = 0.0  # (-inf) - (-inf) would be NaN
    for label, lu, w in (("no cfg", None, 0.0), ("cfg, lu = lc", lu_eq, 5.0)):
        got, sel = _sample(lc, lu, V, w, cur, V, E, 0, 0, 1, len(rows), V)
        smp = R.ref_sample(lc, lu, w, cur, V, E)
        print(f"[parity] sampler tie-breaks ({label}): got {got.tolist()} want {want}")
        assert got.tolist() == want, label
        assert torch.equal(smp.ids, got)  # the reference's first-index arg-max says the same
        assert float(sel[-2]) == 1.0 and float(sel[-1]) == R.FLT_MAX
        assert torch.allclose(sel[:-1].double(), smp.sel[:-1], rtol=2e-5, atol=0)
    # a peaked row: lc 60 above the rest, w = 5 -> z 360 above, every other exp underflows to 0; the peak wins whatever E is
    lc = torch.randn(4, V, generator=g)
    peak = [0, 1027, 5000, 8191]
    for r, c in enumerate(peak):
        lc[r, c] += 60.0
    lu = torch.zeros(4, V)
    E = torch.full((4, V), 1e-6)
    for r, c in enumerate(peak):
        E[r, c] = 1e6
    cur = torch.full((4,), V, dtype=torch.int64)
    got, sel = _sample(lc, lu, V, 5.0, cur, V, E, 0, 0, 1, 4, V)
    assert got.tolist() == peak and bool((sel == 1.0).all())


# -------------------------------------------------------------------------------------------------- mask_by_topk
IMG0, TAIL, GUARD = 5, 3, 64
CANARY_C, CANARY_U, CANARY_CUR = -1111, -2222, -3333
OFF = 310


def _topk(sel, sampled, cur, ml, temp, u, seed, step, mask_id):
    """showo_mask_by_topk on host tensors with canaries around every output; returns the kernel's mask (bool [B, N]) after checking
    the write-back against it on every element"""
    B, N = cur.shape
    ld = IMG0 + N + TAIL
    ids_c = torch.full((B, ld), CANARY_C, dtype=torch.int64, device="cuda")
    ids_u = torch.full((B, ld), CANARY_U, dtype=torch.int64, device="cuda")
    cur_d = torch.cat([cur.reshape(-1), torch.full((GUARD,), CANARY_CUR, dtype=torch.int64)]).cuda()
    m_d = torch.full((B * N + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    L().call("showo_mask_by_topk", L().ptr(dev(sel)), L().ptr(dev(sampled)), L().ptr(cur_d), L().ptr(ids_c), L().ptr(ids_u), ld, IMG0,
             mask_id, OFF, float(ml), float(temp), None if u is None else L().ptr(dev(u)), seed, step, L().ptr(m_d), B, N, S())
    torch.cuda.synchronize()
    ids_c, ids_u, cur_d, m_d = ids_c.cpu(), ids_u.cpu(), cur_d.cpu(), m_d.cpu()
    assert bool((m_d[B * N:] == 0xAB).all()) and bool((cur_d[B * N:] == CANARY_CUR).all()), "guard band overwritten"
    assert bool((m_d[:B * N] <= 1).all())
    m = m_d[:B * N].view(B, N).bool()
    for t, can in ((ids_c, CANARY_C), (ids_u, CANARY_U)):
        assert bool((t[:, :IMG0] == can).all()) and bool((t[:, IMG0 + N:] == can).all()), "ids written outside the image columns"
        assert torch.equal(t[:, IMG0:IMG0 + N], torch.where(m, torch.tensor(mask_id), sampled + OFF))
    assert torch.equal(cur_d[:B * N].view(B, N), torch.where(m, torch.tensor(mask_id), sampled))
    return m


def _check_topk(m, tk, label):
    exc = R.topk_excused(tk)
    bad = (m != tk.masking) & ~exc
    n_exc = int(((m != tk.masking) & exc).sum())
    assert int(bad.sum()) == 0, f"{label}: {int(bad.sum())} elements outside the margin differ (k={tk.k.tolist()})"
    assert int(exc.sum()) <= R.EXCUSED_CAP * m.numel(), label
    return int(exc.sum()), n_exc


@pytest.mark.parametrize("B,N", R.TOPK_SHAPES)
def test_mask_by_topk_at_width_against_fp64_reference(B, N):
    mask_id = 8192
    inside = differ = runs = 0
    for nu in R.unknown_counts(N):
        sel, sampled, cur, u = R.topk_inputs(B, N, nu, seed=N + nu, mask_id=mask_id)
        for ml in R.mask_len_values(N):
            for temp in R.TOPK_TEMPS:
                m = _topk(sel, sampled, cur, ml, temp, u, 0, 0, mask_id)
                tk = R.ref_mask_by_topk(sel, cur, ml, temp, u, mask_id)
                a, b = _check_topk(m, tk, f"B={B} N={N} unknown={nu} mask_len={ml} temp={temp}")
                inside, differ, runs = inside + a, differ + b, runs + 1
    print(f"[parity] mask_by_topk B={B} N={N}: {runs} runs (unknown x mask_len x temp), every element farther than {R.CONF_TOL} from the "
          f"cut equal to the fp64 reference; {inside} excusable elements in all, {differ} of them differ")


def test_mask_by_topk_takes_a_real_sampler_output():
    """sel / sampled straight from the sampler kernel (known positions carry FLT_MAX), cfg2 layout"""
    B, N, V, ld, cfg = R.SAMPLER_CASES[0]
    lc, lu, cur, mask_id, E = R.sampler_inputs(B, N, V, ld, cfg, 3.0, seed=100)
    got, sel = _sample(lc, lu, ld, 5.0, cur, mask_id, E, 0, 0, B, N, V)
    u = torch.rand(B, N, generator=torch.Generator().manual_seed(8))
    for ml, temp in ((76.0, 4.5), (254.0, 0.5)):
        m = _topk(sel.view(B, N), got.view(B, N), cur.view(B, N), ml, temp, u, 0, 0, mask_id)
        _check_topk(m, R.ref_mask_by_topk(sel.view(B, N), cur.view(B, N), ml, temp, u, mask_id), f"sampler output, mask_len={ml}")


def test_mask_by_topk_refuses_more_than_4096_tokens():
    N = 4097
    cur = torch.full((1, N), 8192, dtype=torch.int64, device="cuda")
    buf = torch.zeros(N + 8, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="N <= 4096"):
        L().call("showo_mask_by_topk", L().ptr(dev(torch.ones(1, N))), L().ptr(buf), L().ptr(cur), L().ptr(buf), None, N + 8, 0, 8192, OFF, 5.0,
                 1.0, None, 0, 0, None, 1, N, S())
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0 and bool((cur == 8192).all())


@pytest.mark.parametrize("B,N", R.TOPK_SHAPES)
def test_mask_by_topk_ties_at_the_cut_are_exact(B, N):
    """temp = 0 and sel in {2^-1 .. 2^-8}: conf takes 8 values with massive ties, and `conf < cut` is strict -- with k inside a tie
    group fewer than k tokens are masked"""
    mask_id = 8192
    g = torch.Generator().manual_seed(N)
    for n_unknown in (N, N // 2):
        cur = torch.randint(0, mask_id, (B, N), generator=g)
        for b in range(B):
            cur[b, torch.randperm(N, generator=g)[:n_unknown]] = mask_id
        unknown = cur == mask_id
        sampled = torch.where(unknown, torch.randint(0, mask_id, (B, N), generator=g), cur)
        sel = torch.where(unknown, 2.0 ** -torch.randint(1, 9, (B, N), generator=g).float(), torch.tensor(R.FLT_MAX))
        u = torch.rand(B, N, generator=g)
        srt = torch.sort(sel[0]).values
        c8, c7 = int((srt == 2.0 ** -8).sum()), int((srt == 2.0 ** -7).sum())
        assert c8 >= 2 and c7 >= 3 and c8 + c7 < n_unknown - 1
        for k in (1, c8 - 1, c8, c8 + c7 // 2, c8 + c7 - 1, c8 + c7, n_unknown - 1):  # last of a group, first, inside, last, first of the next
            m = _topk(sel, sampled, cur, float(k), 0.0, u, 0, 0, mask_id)
            want = sel < torch.sort(sel, dim=-1).values[:, k:k + 1]
            tk = R.ref_mask_by_topk(sel, cur, float(k), 0.0, u, mask_id)
            assert torch.equal(tk.masking, want) and int(tk.k[0]) == k
            assert torch.equal(m, want), f"B={B} N={N} unknown={n_unknown} k={k}: {int((m != want).sum())} elements differ"
        assert int((sel[0] < srt[c8 + c7 // 2]).sum()) == c8 < c8 + c7 // 2  # fewer than k are masked inside a tie group


# ------------------------------------------------------------------------------- the Philox path against the host replica
SEEDS = (1234, (0x5EED << 32) | 99)


@pytest.mark.parametrize("seed", SEEDS, ids=["seed32", "seed64"])
def test_sampler_philox_draws_follow_the_documented_counters(seed):
    """exp_noise = NULL: element i of row r at step s draws lane i & 3 of Philox(seed; i >> 2, r, s, 0x51).  Fails if two rows, two
    steps or two loop trips share a stream, or the high seed word is dropped."""
    B, N, V = 2, 64, 8192
    for name, scale, w, with_lu in R.SAMPLER_FAMILIES:  # "narrow": nearly flat rows, where the noise alone decides the token
        lc, lu, cur, mask_id, _ = R.sampler_inputs(B, N, V, V, with_lu, scale, seed=7)
        seen = []
        for step in (0, 1, 17):
            got, sel = _sample(lc, lu, V, w, cur, mask_id, None, seed, step, B, N, V)
            smp = R.ref_sample(lc, lu, w, cur, mask_id, R.sampler_exp_noise(seed, step, B * N, V))
            _check_sample(got, sel, smp, cur, mask_id, f"sampler Philox {name} seed={seed:#x} step={step}")
            seen.append(got)
    unknown = cur == mask_id
    assert float((seen[0] != seen[1])[unknown].float().mean()) > 0.9 and float((seen[1] != seen[2])[unknown].float().mean()) > 0.9


@pytest.mark.parametrize("seed", SEEDS, ids=["seed32", "seed64"])
def test_topk_philox_draws_follow_the_documented_counters(seed):
    """uniform = NULL: element i of sample b at step s draws word 0 of Philox(seed; i, b, s, 0x6b)"""
    mask_id = 8192
    for B, N in ((2, 64), (1, 1024)):
        sel, sampled, cur, _ = R.topk_inputs(B, N, N // 2, seed=N, mask_id=mask_id)
        for step in (0, 1, 17):
            m = _topk(sel, sampled, cur, float(N // 4), 4.5, None, seed, step, mask_id)
            tk = R.ref_mask_by_topk(sel, cur, float(N // 4), 4.5, R.topk_uniform(seed, step, B, N), mask_id)
            _check_topk(m, tk, f"topk Philox seed={seed:#x} step={step} B={B} N={N}")
            if step == 0:  # ... and not the sampler's stream (counter word 3 = 0x51)
                r4 = R.philox4x32_10((np.arange(N)[None, :], np.arange(B)[:, None], step, 0x51), R._key(seed))
                other = R.ref_mask_by_topk(sel, cur, float(N // 4), 4.5, torch.from_numpy(np.ascontiguousarray(R.u32_to_unit(r4[..., 0]))), mask_id)
                assert not torch.equal(other.masking, tk.masking)
    print(f"[parity] mask_by_topk Philox seed={seed:#x}: masks of steps 0, 1, 17 at (2, 64) and (1, 1024) equal the host replica's")


def test_sampler_philox_distribution_beyond_the_first_trip():
    """20 000 rows at V = 2048 (two trips of the draw loop), logits constant inside 16 blocks of 128 columns: chi-square of the block
    counts against the blocks' softmax mass"""
    V, rows, nblk = 2048, 20000, 16
    logit = torch.randn(nblk, generator=torch.Generator().manual_seed(0)).repeat_interleave(V // nblk)
    lc = logit[None].repeat(rows, 1)
    cur = torch.full((rows,), V, dtype=torch.int64)
    got, sel = _sample(lc, None, V, 0.0, cur, V, None, 1234, 0, rows, 1, V)
    p = logit.double().softmax(-1)
    pb = p.view(nblk, -1).sum(-1)
    cnt = torch.bincount(got // (V // nblk), minlength=nblk).double()
    chi2 = float(((cnt - rows * pb) ** 2 / (rows * pb)).sum())
    print(f"[parity] sampler Philox distribution V={V}, {rows} rows, 16 column blocks: chi2={chi2:.2f} (dof 15, bound 50); "
          f"share of draws beyond column 1024: {float((got >= 1024).float().mean()):.4f} (softmax mass {float(p[1024:].sum()):.4f})")
    assert chi2 < 50.0, chi2  # dof = 15; P(chi2 > 50) ~ 1e-5
    assert torch.allclose(sel.double(), p[got], rtol=2e-5, atol=0)


# ---------------------------------------------------------------------- through the engine: production head width, narrow body
def _dims(N):
    return util.Wt.ShowoDims(hidden=256, layers=2, heads=4, ffn=512, llm_vocab=300, codebook=8192, num_vq_tokens=N,
                             vocab=300 + 10 + 8192 + 1, max_text_len=8)


_MODELS = {}


@pytest.fixture(scope="module")
def models():
    def get(N):
        if N not in _MODELS:
            d = _dims(N)
            _MODELS[N] = (d, util.build_showo(d, util.Wt.make_showo_state(d, seed=11), max_batch=4, max_seq=N + 11))
        return _MODELS[N]
    yield get
    _MODELS.clear()


def _t2i_inputs(d, B, cfg, seed, known=0.5):
    """B prompts of different lengths, a share of the image tokens known (different per sample); CFG rows with the empty prompt"""
    rs = np.random.RandomState(seed)
    N, T = d.num_vq_tokens, d.max_text_len + 1
    rows_c, rows_u = [], []
    for b in range(B):
        k = 4 + 3 * b
        img = np.where(rs.rand(N) >= known, d.mask_token_id, d.image_offset + rs.randint(0, d.codebook, size=N)).tolist()
        rows_c.append([d.pad_id] * (T - k) + [d.t2i_id] + rs.randint(0, 290, size=k - 2).tolist() + [290, d.soi_id] + img + [d.eoi_id])
        rows_u.append([d.pad_id] * (T - 3) + [d.t2i_id, 290, 290, d.soi_id] + img + [d.eoi_id])
    ic = torch.tensor(rows_c).cuda()
    iu = torch.tensor(rows_u).cuda() if cfg else None
    mask = util.pkg().prompting_utils.create_attention_mask_predict_next(ic if iu is None else torch.cat([ic, iu]), pad_id=d.pad_id,
                                                                        soi_id=d.soi_id, eoi_id=d.eoi_id, rm_pad_in_image=True)
    return ic, iu, mask


def _generate(m, d, ic, iu, mask, steps, w, en, un, use_graph):
    ids = ic.clone()
    out = m.t2i_generate(input_ids=ids, uncond_input_ids=iu, attention_mask=mask, temperature=1.0, timesteps=steps, guidance_scale=w,
                         config=util.gen_config(d), _exp_noise=en, _uniform=un, use_graph=use_graph, reduce_step0=False)
    torch.cuda.synchronize()
    return out.cpu(), ids.cpu()


def _single_step(m, d, B, cfg, seed):
    """steps = 1: sampled_out and the in-place ids against ref_sample + ref_mask_by_topk on the GPU's own step-0 logits, with the
    denoise step asked for as a graph and eagerly"""
    N, V, off, mask_id = d.num_vq_tokens, d.codebook, d.image_offset, d.mask_token_id
    w = 5.0 if cfg else 0.0
    ic, iu, mask = _t2i_inputs(d, B, cfg, seed)
    g = torch.Generator().manual_seed(seed)
    E = torch.empty(1, B * N, V).exponential_(generator=g)
    u = torch.rand(1, B, N, generator=g)
    en, un = E.cuda(), u.cuda()
    nseq = 2 * B if cfg else B
    buf = torch.zeros((nseq * N, V), dtype=torch.float32, device="cuda")
    ml, tp = util.pkg().sampling.t2i_step_constants(1, N)
    img0 = ic.shape[1] - (N + 1)
    cur = ic[:, img0:img0 + N].cpu()
    cur = torch.where(cur == mask_id, cur, cur - off)
    L().call("showo_engine_t2i_debug", m.engine(), L().ptr(buf), 0)
    try:
        for ug in (1, 0):
            buf.zero_()
            out, ids = _generate(m, d, ic, iu, mask, 1, w, en, un, ug)
            lg = buf.cpu()
            assert bool(torch.isfinite(lg).all()) and float(lg.abs().max()) > 0
            smp = R.ref_sample(lg[:B * N], lg[B * N:] if cfg else None, w, cur.reshape(-1), mask_id, E[0])
            label = f"engine step B={B} N={N} cfg={cfg} use_graph={ug}"
            unknown = (cur == mask_id).reshape(-1)
            mism = (out.reshape(-1) != smp.ids) & unknown
            near = smp.gap < R.GAP_TOL
            print(f"[parity] {label}: {int(mism.sum())} of {int(unknown.sum())} unknown rows differ from the reference on the GPU's own "
                  f"logits, {int((mism & near).sum())} excused; smallest top-2 gap {float(smp.gap.min()):.3e}")
            assert int((mism & ~near).sum()) == 0 and int((mism & near).sum()) <= R.EXCUSED_CAP * int(unknown.sum())
            assert torch.equal(out.reshape(-1)[~unknown], cur.reshape(-1)[~unknown])
            # the confidence the kernel handed on is p_ref of ITS token (equal to the reference's wherever the ids agree)
            sel = torch.where(unknown, torch.gather(smp.p, -1, out.reshape(-1, 1))[:, 0], torch.tensor(R.FLT_MAX, dtype=torch.float64))
            tk = R.ref_mask_by_topk(sel.float().view(B, N), cur, ml[0], tp[0], u[0], mask_id)
            m_got = ids[:, img0:img0 + N] == mask_id
            _check_topk(m_got, tk, label)
            assert torch.equal(ids[:, img0:img0 + N][~m_got], (out + off)[~m_got])
            assert torch.equal(ids[:, :img0], ic.cpu()[:, :img0]) and torch.equal(ids[:, img0 + N:], ic.cpu()[:, img0 + N:])
    finally:
        L().call("showo_engine_t2i_debug", m.engine(), None, 0)
    return out, E[0]


def test_engine_step_at_head_width_cfg(models):
    d, m = models(256)
    _single_step(m, d, 2, True, seed=21)


def test_engine_step_at_head_width_1024_tokens_no_cfg(models):
    d, m = models(1024)
    _single_step(m, d, 1, False, seed=22)


def test_engine_three_steps_graph_equals_eager_with_gross_noise(models):
    """eager offsets the injected noise on the host, the replayed graph on the device (step * noise_stride, mask_len and temperature
    from the schedule in device memory).  Steps 1 and 2 carry planted noise -- E = 1e8 everywhere but one column per row, another
    one per step -- so a wrong stride or step index changes tokens instead of hiding in sampling noise."""
    d, m = models(256)
    B, N, V, off, mask_id = 2, d.num_vq_tokens, d.codebook, d.image_offset, d.mask_token_id
    ic, iu, mask = _t2i_inputs(d, B, True, seed=21, known=0.1)  # ~230 unknown: k0 = 221 and k1 = 128 come from the schedule
    g = torch.Generator().manual_seed(21)
    E = torch.empty(3, B * N, V)
    E[0].exponential_(generator=g)
    u0 = torch.rand(1, B, N, generator=g)
    planted = torch.randint(0, V, (3, B * N), generator=g)
    planted[2] = (planted[1] + 1 + torch.randint(0, V - 1, (B * N,), generator=g)) % V  # never step 1's column
    for s in (1, 2):
        E[s] = 1e8
        E[s].scatter_(1, planted[s][:, None], 1e-8)
    u = torch.cat([u0, torch.rand(2, B, N, generator=g)])
    en, un = E.cuda(), u.cuda()
    out_g, ids_g = _generate(m, d, ic, iu, mask, 3, 5.0, en, un, 1)
    out_e, ids_e = _generate(m, d, ic, iu, mask, 3, 5.0, en, un, 0)
    print(f"[parity] engine 3 steps B={B} N={N} V={V}: graph vs eager token agreement {float((out_g == out_e).float().mean()):.4f}")
    assert torch.equal(out_g, out_e) and torch.equal(ids_g, ids_e)
    # every token comes from the step that drew it: the known id, step 0's draw, or the planted column of step 1 / step 2
    img0 = ic.shape[1] - (N + 1)
    cur = ic[:, img0:img0 + N].cpu()
    known = cur != mask_id
    assert torch.equal(out_g[known], (cur - off)[known])
    s0, _ = _generate(m, d, ic, iu, mask, 1, 5.0, en[:1].contiguous(), un[:1].contiguous(), 0)
    p1, p2 = planted[1].view(B, N), planted[2].view(B, N)
    src = torch.where(out_g == p2, 2, torch.where(out_g == p1, 1, torch.where(out_g == s0, 0, -1)))
    assert int((src[~known] < 0).sum()) == 0, "a token that no step's noise explains"
    ml, _ = util.pkg().sampling.t2i_step_constants(3, N)
    n_unknown = (~known).sum(-1)
    # step 0 leaves k0 tokens masked, step 1 draws exactly those (only they carry a confidence below FLT_MAX) and leaves k1 of them
    # masked, step 2 draws those: k0 - k1 tokens show step 1's planted column, k1 step 2's.  +-2 for a planted column that happens to
    # be another step's token at the same position (1 / 8192 per position, 512 positions).
    for b in range(B):
        k0 = max(1, min(int(n_unknown[b]) - 1, int(ml[0])))
        k1 = max(1, min(k0 - 1, int(ml[1])))
        n2, n1 = int((src[b][~known[b]] == 2).sum()), int((src[b][~known[b]] == 1).sum())
        print(f"[parity] engine 3 steps sample {b}: {n1} tokens from step 1's planted column (k0 - k1 = {k0 - k1}), {n2} from step 2's (k1 = {k1})")
        assert abs(n2 - k1) <= 2 and abs(n1 - (k0 - k1)) <= 2
