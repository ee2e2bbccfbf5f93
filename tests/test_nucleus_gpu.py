"""GPU tests of the nucleus (top-p) draw, showo_sample_topk_topp (csrc/sample_row.h sample_topk_topp_row), against tests/nucleus_ref.py.

The cases come from nucleus_ref.cases / tie_case: chosen on the CPU from the reference alone, every one at least MARGIN = 1e-5 of
probability mass clear of the cut (about 50x what the device's fixed-point masses can differ from the reference's), so the kept set is
compared exactly and nothing is excused.  V = 439 is below one trip of the 1024-thread block, 1030 a ragged second trip, 58498 the
production vocabulary (not a multiple of the 4-wide Philox groups)."""
import ctypes as C

import numpy as np
import pytest
import torch

import util
import nucleus_ref as N
from util import O, dev

pytestmark = pytest.mark.gpu


def L():
    return util.lib()


def S():
    return L().stream()


def _topp(ld, V, k, p, T, noise, seed, step, out_ptr):
    L().call("showo_sample_topk_topp", L().ptr(ld), V, 0 if k is None else k, p, T, L().ptr(noise), seed, step, out_ptr, S())


def _probe(logits, k, p, T, probes):
    """for every token i of `probes`: E = 1 everywhere but E_i = 1e-30; the draw is i iff i is kept, else the arg-max of p'"""
    V = logits.numel()
    keep, pk, margin = N.ref_nucleus(logits, k, p, T)
    assert margin >= N.MARGIN
    top = int(torch.argmax(pk))
    E = torch.ones((len(probes), V), dtype=torch.float32)
    E[torch.arange(len(probes)), torch.as_tensor(probes)] = 1e-30
    Ed, ld = dev(E), dev(logits)
    toks = torch.full((len(probes),), -7, dtype=torch.int64, device="cuda")
    for j in range(len(probes)):
        _topp(ld, V, k, p, T, Ed, 0, j, toks.data_ptr() + 8 * j)  # row j of the noise matrix
    got = toks.tolist()
    want = [i if bool(keep[i]) else top for i in probes]
    bad = [(i, g, bool(keep[i])) for i, g in zip(probes, got) if g != (i if bool(keep[i]) else top)]
    assert got == want, (bad[:8], len(bad), margin)
    return keep


# ---- 1. the kept set, exactly ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", [f for f in N.FAMILIES if f[0] == 439 and f[1] == 3.0], ids=str)
def test_kept_set_by_probing_every_token(fam):
    V, scale, k, p, T = fam
    keep = _probe(N.family_logits(V, scale, N.cases(fam)[0]), k, p, T, list(range(V)))
    assert 1 <= int(keep.sum()) < V


def test_kept_set_keeps_a_whole_tied_group_at_the_cut():
    """logits rounded to halves, the cut inside a tied group (a cut along a sorted order would split it): every tied token stays"""
    lg = N.family_logits(439, 3.0, N.tie_case(), halves=True)
    keep = _probe(lg, None, 0.9, 1.0, list(range(439)))
    cut = lg[keep].min()
    assert int((lg == cut).sum()) >= 3 and bool(keep[lg == cut].all())


@pytest.mark.parametrize("fam", [f for f in N.FAMILIES if f[0] == N.V_FULL], ids=str)
def test_kept_set_around_the_cut_at_the_full_vocabulary(fam):
    """the 64 tokens nearest the cut on each side, the top token, the lowest token and the last index"""
    V, scale, k, p, T = fam
    lg = N.family_logits(V, scale, N.cases(fam)[0])
    keep, _, _ = N.ref_nucleus(lg, k, p, T)
    order = torch.argsort(lg, descending=True, stable=True)
    nk = int(keep.sum())
    assert bool(keep[order[:nk]].all()) and not bool(keep[order[nk:]].any())
    probes = order[max(0, nk - 64):nk + 64].tolist() + [int(order[0]), int(order[-1]), V - 1]
    _probe(lg, k, p, T, probes)


# ---- 2. the draw -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [439, 1030, N.V_FULL])
def test_draw_equals_the_reference_expression_under_injected_noise(V):
    tok = torch.zeros(1, dtype=torch.int64, device="cuda")
    g = torch.Generator().manual_seed(V)
    for fam in [f for f in N.FAMILIES if f[0] == V]:
        _, scale, k, p, T = fam
        for seed in N.cases(fam):
            lg = N.family_logits(V, scale, seed)
            e = torch.empty(V).exponential_(1, generator=g)
            want, pk, keep = N.draw_reference(lg, k, p, T, e)
            _topp(dev(lg), V, k, p, T, dev(e), 0, 0, L().ptr(tok))
            got = int(tok.item())
            if got != want:  # only acceptable as an fp32 near-tie of p'/E between two kept tokens
                a, b = float(pk[got] / e[got]), float(pk[want] / e[want])
                assert bool(keep[got]) and abs(a - b) <= 1e-5 * abs(b), (fam, seed, got, want)
    # row `step` of a noise matrix is used
    fam = [f for f in N.FAMILIES if f[0] == V][0]
    _, scale, k, p, T = fam
    lg = N.family_logits(V, scale, N.cases(fam)[0])
    E = torch.empty(3, V).exponential_(1, generator=g)
    for step in range(3):
        _topp(dev(lg), V, k, p, T, dev(E), 0, step, L().ptr(tok))
        want, pk, keep = N.draw_reference(lg, k, p, T, E[step])
        got = int(tok.item())
        assert got == want or (bool(keep[got]) and abs(float(pk[got] / E[step][got]) - float(pk[want] / E[step][want]))
                               <= 1e-5 * float(pk[want] / E[step][want]))


# ---- 3. off means the bits of sample_topk-------------------------------------------------------------------------------------------------------
def test_top_p_off_is_the_token_of_sample_topk():
    V, steps = N.V_FULL, 64
    ld = dev(N.family_logits(V, 3.0, 5))
    for k, T in ((0, 1.0), (50, 1.3), (5, 0.7)):
        want = torch.full((steps,), -1, dtype=torch.int64, device="cuda")
        for i in range(steps):
            L().call("showo_sample_topk", L().ptr(ld), V, k, T, None, 4242, i, want.data_ptr() + 8 * i, S())
        assert len(set(want.tolist())) > 1
        for p in (1.0, 7.0):
            got = torch.full((steps,), -2, dtype=torch.int64, device="cuda")
            for i in range(steps):
                _topp(ld, V, k, p, T, None, 4242, i, got.data_ptr() + 8 * i)
            assert torch.equal(got, want), (k, T, p)


def _tiny(precision=0):
    g = util.golden("showo_tiny_mmu.npz")
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd)
    m.set_precision(precision)
    return g, d, m


def test_mmu_generate_without_top_p_is_unchanged():
    g, d, m = _tiny()
    ids, mask = dev(g["ids"]), dev(g["mask"])

    def run(**kw):
        gen = torch.Generator(device="cuda").manual_seed(11)
        return [int(t) for t in m.mmu_generate(ids, attention_mask=mask, max_new_tokens=24, top_k=20, temperature=1.1, generator=gen, **kw)]

    want = run()
    assert run(top_p=None) == want and run(top_p=1.0) == want
    assert run(top_p=0.05) != want  # the keyword is not ignored: a narrow nucleus draws other tokens


# ---- 4. run-to-run determinism -------------------------------------------------------------------------------------------------------------
def test_same_call_returns_one_token_200_times():
    """thousands of near-equal masses around the cut: any order dependence of the mass sums would move the cut between runs"""
    V, n = N.V_FULL, 200
    ld = dev(N.family_logits(V, 0.05, 1))
    toks = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    for i in range(n):
        _topp(ld, V, None, 0.5, 1.0, None, 77, 3, toks.data_ptr() + 8 * i)
    got = toks.tolist()
    assert len(set(got)) == 1 and 0 <= got[0] < V


# ---- 5. distribution and support -----------------------------------------------------------------------------------------------------------
# upper 1e-7 quantile of chi-square for 1..40 degrees of freedom
CHI2_1E7 = [28.37, 32.24, 35.41, 38.24, 40.86, 43.34, 45.7, 47.97, 50.17, 52.31, 54.39, 56.43, 58.43, 60.4, 62.33, 64.23, 66.1, 67.95,
            69.78, 71.59, 73.38, 75.15, 76.9, 78.64, 80.37, 82.08, 83.77, 85.46, 87.13, 88.79, 90.44, 92.08, 93.72, 95.34, 96.95, 98.56,
            100.15, 101.74, 103.33, 104.9]


def test_philox_draws_follow_the_renormalised_distribution_on_its_support():
    V, n, p_top = 64, 6000, 0.7
    lg = None
    for seed in range(50):  # a case clear of the cut, chosen on the reference alone
        lg = N.family_logits(V, 2.0, seed)
        keep, pk, margin = N.ref_nucleus(lg, None, p_top, 1.0)
        if margin >= N.MARGIN and int(keep.sum()) >= 4:
            break
    ld = dev(lg)
    toks = torch.zeros(n, dtype=torch.int64, device="cuda")
    for i in range(n):
        _topp(ld, V, 0, p_top, 1.0, None, 99, i, toks.data_ptr() + 8 * i)
    cnt = torch.bincount(toks.cpu(), minlength=V).double()
    assert cnt[~keep].sum() == 0
    dof = int(keep.sum()) - 1
    chi2 = float((((cnt - n * pk) ** 2)[keep] / (n * pk[keep])).sum())
    print(f"[nucleus] chi2 = {chi2:.2f}, dof = {dof}, bound {CHI2_1E7[dof - 1]}")
    assert chi2 < CHI2_1E7[dof - 1], (chi2, dof)


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------------
def test_bad_top_p_is_error_1_without_a_launch():
    g, d, m = _tiny()
    lib = L().load()
    eng = m.engine()
    V = d.vocab
    ids, mask = dev(g["ids"]), dev(g["mask"])
    lg = torch.empty((2, V), dtype=torch.float32, device="cuda")
    tok = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    out = torch.full((2, 2), -7, dtype=torch.int64, device="cuda")
    L().call("showo_engine_prefill", eng, L().ptr(ids), None, L().ptr(mask), ids.shape[1], L().ptr(lg), S())
    for bad in (0.0, -0.1, float("nan")):
        assert lib.showo_sample_topk_topp(L().ptr(lg), V, 5, bad, 1.0, None, 1, 0, L().ptr(tok), S()) == 1
        assert lib.showo_engine_decode_sample_p(eng, L().ptr(tok), 2, L().ptr(out), L().ptr(lg), 5, bad, 1.0, None, 1, 1, 0, S()) == 1
        with pytest.raises(ValueError):
            m.mmu_generate(ids, attention_mask=mask, max_new_tokens=2, top_p=bad)
        with pytest.raises(ValueError):
            m.mmu_generate_batch(idx=[ids, ids], attention_mask=[mask, mask], max_new_tokens=2, top_p=[0.5, bad])
    L().call("showo_engine_batch_begin", eng, 2, ids.shape[1] + 4)
    for b in range(2):
        L().call("showo_engine_batch_prefill", eng, b, L().ptr(ids), None, L().ptr(mask), ids.shape[1], L().ptr(lg[b]), S())
    arr = lambda t, *v: C.cast((t * 2)(*v), C.c_void_p)
    for bad in (0.0, -0.1, float("nan")):
        prod = (C.c_int * 2)(-7, -7)
        rc = lib.showo_engine_batch_decode_sample_p(eng, L().ptr(tok), 2, L().ptr(out), L().ptr(lg), arr(C.c_int, 5, 5), arr(C.c_float, 0.5, bad),
                                                    arr(C.c_float, 1.0, 1.0), arr(C.c_uint64, 1, 2), arr(C.c_int, 1, 1), None, arr(C.c_int, 2, 2), -1,
                                                    C.cast(prod, C.c_void_p), 0, S())
        assert rc == 1 and list(prod) == [-7, -7]
    torch.cuda.synchronize()
    assert tok.tolist() == [-7, -7] and out.tolist() == [[-7, -7], [-7, -7]]  # nothing was launched
