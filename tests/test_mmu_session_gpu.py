"""GPU tests of mmu sessions: showo_kv_fork / showo_mask_append_rows at kernel level, showo_engine_prefill_append / _cache_rewind /
_batch_fork / _batch_prefill_append through the C ABI, and Showo.mmu_session on top ("mmu sessions").

Contracts held here: (1) a forked slot gives the bits of the engine's own cache, so generate_batch == generate + rewind; (2) a rewind is
clean; (3) append, decode and fork never touch the prefix; (4) prefix + append against the full prompt is a TOLERANCE statement -- both
are held to the fp32 oracle at the bf16 gates of tests/test_modules_gpu.py (1e-3 at precisions 1 and 2), never to each other's bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import util
from util import O, Wt, dev
from test_mmu_session_cpu import append_rows_np

pytestmark = pytest.mark.gpu

REL_RMS, REL_MAX = 1e-2, 3e-2   # bf16 operands vs the fp32 oracle (tests/test_modules_gpu.py)
TOL_FP32_CLASS = 1e-3           # precisions 1 and 2 (PRECISE_TOL / FP16_TOL there)


def _L():
    return util.lib()


def _gate(precision):
    return (TOL_FP32_CLASS, TOL_FP32_CLASS) if precision in (1, 2) else (REL_MAX, REL_RMS)


def _check(got, ref, precision, what):
    rmax, rrms = util.relerr(got, ref)
    print(f"[parity] {what} (precision {precision}): rel_max={rmax:.3e} rel_rms={rrms:.3e}")
    gmax, grms = _gate(precision)
    assert torch.isfinite(got).all() and rmax <= gmax and rrms <= grms, (what, precision, rmax, rrms)
    return rmax


def _ints(toks):
    return [int(t) for t in toks]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _snap(ptr, nelems):
    """nelems 16-bit elements of device memory at `ptr` as an int16 tensor (a copy)"""
    out = torch.empty((nelems,), dtype=torch.int16, device="cuda")
    _L().call("showo_copy_b128", ptr, _L().ptr(out), nelems * 2, _L().stream())
    torch.cuda.synchronize()
    return out


def _cache(eng, d, cap=None, slot=None):
    """(K [nL, nH, cap, 64], V^T [nL, nH * 64, cap]) int16 copies of the engine's decode cache, or of slot `slot` of the running batch"""
    L = _L()
    k, vt, kls, vls, c = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int()
    if slot is None:
        L.call("showo_engine_cache_ptrs", eng, C.byref(k), C.byref(vt), C.byref(kls), C.byref(vls))
        n, p, c2, ep = _state(eng)
        cap = c2
    else:
        L.call("showo_engine_batch_slot_ptrs", eng, slot, C.byref(k), C.byref(vt), C.byref(kls), C.byref(vls), C.byref(c))
        cap = c.value
    per = d.heads * cap * 64
    outk, outv = [], []
    for li in range(d.layers):
        outk.append(_snap(k.value + 2 * li * kls.value, per).reshape(d.heads, cap, 64))
        outv.append(_snap(vt.value + 2 * li * vls.value, per).reshape(d.heads * 64, cap))
    return torch.stack(outk), torch.stack(outv)


def _state(eng):
    n, p, cap, ep = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    _L().call("showo_engine_cache_state", eng, C.byref(n), C.byref(p), C.byref(cap), C.byref(ep))
    return n.value, p.value, cap.value, ep.value


def _prefill(eng, V, ids=None, emb=None, mask=None):
    L = _L()
    n = (ids if ids is not None else emb).shape[1]
    logits = torch.empty((V,), dtype=torch.float32, device="cuda")
    mk = None if mask is None else dev(mask).float().reshape(1, 1, n, n).contiguous()
    L.call("showo_engine_prefill", eng, L.ptr(ids), L.ptr(emb), L.ptr(mk), n, L.ptr(logits), L.stream())
    torch.cuda.synchronize()
    return logits


def _append(eng, V, ids=None, emb=None, slot=None):
    L = _L()
    n = (ids if ids is not None else emb).shape[1]
    logits = torch.empty((V,), dtype=torch.float32, device="cuda")
    if slot is None:
        L.call("showo_engine_prefill_append", eng, L.ptr(ids), L.ptr(emb), n, L.ptr(logits), L.stream())
    else:
        L.call("showo_engine_batch_prefill_append", eng, slot, L.ptr(ids), L.ptr(emb), n, L.ptr(logits), L.stream())
    torch.cuda.synchronize()
    return logits


def _i64(x):
    return dev(torch.as_tensor(x, dtype=torch.int64).reshape(1, -1))


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap_dst", [64, 192])
def test_kv_fork_is_a_bit_copy_that_writes_nothing_else(cap_dst):
    """random 16-bit patterns (NaN / inf patterns of either 16-bit float type among them) in a source of capacity 2048 with padded layer
    strides; the destination holds a sentinel: [0, P) arrives bit for bit, V^T [P, 64 ceil(P / 64)) is zero, everything else keeps the
    sentinel, the source is unchanged"""
    L = _L()
    nL, nH, cap_src, SENT = 2, 3, 2048, 0x5A5A
    gen = torch.Generator().manual_seed(3)
    ks, vs = nH * cap_src * 64 + 64, nH * 64 * cap_src + 8     # layer strides with padding between the layers
    kd, vd = nH * cap_dst * 64 + 8, nH * 64 * cap_dst + 64
    src_k = torch.randint(-32768, 32768, (nL * ks,), generator=gen, dtype=torch.int32).to(torch.int16)
    src_v = torch.randint(-32768, 32768, (nL * vs,), generator=gen, dtype=torch.int32).to(torch.int16)
    for t in (src_k, src_v):  # quiet / signalling NaN and inf of bf16 and fp16 at known places, also in row 0 / column 0
        t[0], t[1], t[2], t[3], t[64 * 7 + 5] = 0x7FC0, 0x7F81, 0x7C00, -64, 0x7E00
    sk, sv = src_k.cuda(), src_v.cuda()
    sk0, sv0 = sk.clone(), sv.clone()
    for P in (1, 7, 8, 63, 64, 65, 130):
        if P >= cap_dst:
            continue
        dk = torch.full((nL * kd,), SENT, dtype=torch.int16, device="cuda")
        dv = torch.full((nL * vd,), SENT, dtype=torch.int16, device="cuda")
        L.call("showo_kv_fork", L.ptr(sk), L.ptr(sv), cap_src, ks, vs, L.ptr(dk), L.ptr(dv), cap_dst, kd, vd, nL, nH, P, L.stream())
        torch.cuda.synchronize()
        want_k = torch.full((nL * kd,), SENT, dtype=torch.int16)
        want_v = torch.full((nL * vd,), SENT, dtype=torch.int16)
        Z = min(cap_dst, (P + 63) // 64 * 64)
        for li in range(nL):
            a = src_k[li * ks: li * ks + nH * cap_src * 64].reshape(nH, cap_src, 64)
            want_k[li * kd: li * kd + nH * cap_dst * 64].reshape(nH, cap_dst, 64)[:, :P] = a[:, :P]
            b = src_v[li * vs: li * vs + nH * 64 * cap_src].reshape(nH * 64, cap_src)
            w = want_v[li * vd: li * vd + nH * 64 * cap_dst].reshape(nH * 64, cap_dst)
            w[:, :P] = b[:, :P]
            w[:, P:Z] = 0
        assert torch.equal(dk.cpu(), want_k), ("K", cap_dst, P)
        assert torch.equal(dv.cpu(), want_v), ("V^T", cap_dst, P)
        assert torch.equal(sk, sk0) and torch.equal(sv, sv0)
    # refused before any launch: a prefix beyond a capacity, capacities that are no multiple of 64
    dk = torch.zeros((nL * kd,), dtype=torch.int16, device="cuda")
    dv = torch.zeros((nL * vd,), dtype=torch.int16, device="cuda")
    lib = L.load()
    assert lib.showo_kv_fork(L.ptr(sk), L.ptr(sv), cap_src, ks, vs, L.ptr(dk), L.ptr(dv), cap_dst, kd, vd, nL, nH, cap_dst + 1, L.stream()) == 5
    assert lib.showo_kv_fork(L.ptr(sk), L.ptr(sv), cap_src, ks, vs, L.ptr(dk), L.ptr(dv), cap_dst - 8, kd, vd, nL, nH, 1, L.stream()) == 1


@pytest.mark.parametrize("Ln", [1, 5, 64])
def test_mask_append_rows_equals_the_python_rule(Ln):
    L = _L()
    lib = L.load()
    for last, L0, P in (((0, 40, 0, 0), 40, 40), ((0, 3, 7, 40), 40, 40), ((2, 40, 0, 0), 40, 57), ((0, 0, 0, 0), 9, 9), ((0, 0, 4, 9), 9, 300)):
        iv = torch.full((Ln + 1, 4), -7, dtype=torch.int32, device="cuda")
        arr = (C.c_int32 * 4)(*last)
        L.call("showo_mask_append_rows", C.cast(arr, C.c_void_p), L0, P, Ln, L.ptr(iv), L.stream())
        torch.cuda.synchronize()
        assert np.array_equal(iv[:Ln].cpu().numpy(), append_rows_np(last, L0, P, Ln)), (last, L0, P)
        assert bool((iv[Ln] == -7).all())  # nothing behind the Ln rows
    iv = torch.full((Ln, 4), -7, dtype=torch.int32, device="cuda")
    arr = (C.c_int32 * 4)(0, 3, 5, 9)
    assert lib.showo_mask_append_rows(C.cast(arr, C.c_void_p), 12, 12, Ln, L.ptr(iv), L.stream()) == 6
    torch.cuda.synchronize()
    assert bool((iv == -7).all())


# ---- tiny model -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture():
    g = util.golden("showo_tiny_mmu.npz")
    d, sd = util.tiny_state()
    ids = torch.from_numpy(g["ids"]).to(torch.int64)
    return g, d, sd, ids


@functools.lru_cache(maxsize=None)
def _oracle_fixture_last():
    """fp32 logits of the fixture's last prompt row (what its first token is drawn from), computed once"""
    g, d, sd, ids = _fixture()
    return O.showo_logits(O.to_torch(sd), d, ids, attention_mask=torch.from_numpy(g["mask"]))[0, -1]


def _tiny(precision=0, max_seq=128):
    g, d, sd, ids = _fixture()
    m = util.build_showo(d, sd, max_seq=max_seq)
    m.set_precision(precision)
    return g, d, m, ids


def _pm(ids, d):
    return O.mask_mmu(ids, d.eoi_id)


def test_session_answers_the_fixture_question_with_the_reference_tokens():
    """prefix = the first 20 ids, question = the last 5: the session gives the fixture's greedy tokens (eager and graph), the tokens
    drawn with the reference's recorded noise, and -- prefill of the whole prompt, no rows -- what mmu_generate gives"""
    g, d, m, ids = _tiny()
    want = g["tokens"].tolist()
    sess = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(_pm(ids[:, :20], d)))
    assert sess.length == sess.prefix_length == 20
    mark = sess.mark()
    for graph in (0, 1):
        m.decode_graph = graph
        toks = sess.generate(dev(ids[:, 20:]), max_new_tokens=len(want), top_k=1)
        assert all(isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 0 for t in toks)
        got = _ints(toks)
        print(f"[parity] tiny mmu_session greedy graph={graph}", got, "reference", want)
        assert got == want and sess.length == 25 + len(want) - 1
        sess.rewind(mark)
        for tag, kw in (("topk5", dict(top_k=5, temperature=0.7)), ("full", dict(top_k=None, temperature=1.3))):
            got = _ints(sess.generate(dev(ids[:, 20:]), max_new_tokens=8, _exp_noise=dev(g[f"exp_noise_{tag}"]), **kw))
            print(f"[parity] tiny mmu_session {tag} graph={graph}", got, "reference", g[f"tokens_{tag}"].tolist())
            assert got == g[f"tokens_{tag}"].tolist()
            sess.rewind(mark)
    long_ref = _ints(m.mmu_generate(dev(ids), attention_mask=dev(g["mask"]), max_new_tokens=40, top_k=1))
    with pytest.raises(RuntimeError, match="stale"):
        sess.generate(dev(ids[:, 20:]), max_new_tokens=2, top_k=1)
    whole = m.mmu_session(dev(ids), attention_mask=dev(g["mask"]))
    assert _ints(whole.generate(max_new_tokens=40, top_k=1)) == long_ref
    # embeddings instead of ids, interval mask instead of the dense one, and the <eot> cut
    tab = m.showo.model.embed_tokens.weight.detach().float()
    ivm = util.pkg().prompting_utils.intervals_for_mmu(dev(ids[:, :20]), eoi_id=d.eoi_id)
    se = m.mmu_session(input_embeddings=tab[dev(ids[:, :20])], attention_mask=ivm)
    eot = long_ref[3]
    got = _ints(se.generate(input_embeddings=tab[dev(ids[:, 20:])], max_new_tokens=40, top_k=1, eot_token=eot))
    assert got == long_ref[:long_ref.index(eot) + 1] and se.length == 25 + len(got) - 1
    assert _state(m.engine())[0] == se.length  # what the device loop ran past <eot> is gone from the cache


@pytest.mark.parametrize("precision", [0, 2, 3])
def test_append_logits_vs_oracle_on_the_fixture(precision):
    """logits_last of prefill(ids[:20]) + append(ids[20:]) against the fp32 oracle on the 25 ids (precision 3: the oracle on the
    dequantised weights, as tests/test_int8_decode_gpu.py does); the full-prompt prefill is held to the same oracle, not to the append.

    Precision 1 is NOT among the cases here: the tiny fixture has hidden 128, so 3 * hidden is no multiple of 256, accuracy mode has no
    production-kernel form at this shape and showo_engine_prefill refuses a KV-cached prefill under it -- there is no engine append to
    take logits from.  The precision-1 logits_last check against the oracle runs at the SMALL shape
    (test_small_dims_300_row_append_takes_the_fused_layer[1]); at this shape precision 1 is held to the fixture's tokens through the
    recompute session (test_precision_1_session_on_the_tiny_shape_recomputes_like_mmu_generate)."""
    g, d, m, ids = _tiny(precision)
    if precision == 3:
        from test_int8_decode_gpu import _dequant_state
        sd_dq, _ = _dequant_state(_fixture()[2])
        ref = O.showo_logits(O.to_torch(sd_dq), d, ids, attention_mask=torch.from_numpy(g["mask"]))[0, -1]
    else:
        ref = _oracle_fixture_last()
    eng = m.engine()
    _prefill(eng, d.vocab, ids=_i64(ids[:, :20]), mask=_pm(ids[:, :20], d))
    got = _append(eng, d.vocab, ids=_i64(ids[:, 20:]))
    _check(got.cpu(), ref, precision, "tiny prefix 20 + append 5, logits_last vs oracle")
    assert _state(eng)[:2] == (25, 20)
    full = _prefill(eng, d.vocab, ids=_i64(ids), mask=g["mask"])
    _check(full.cpu(), ref, precision, "tiny full prompt 25, logits_last vs oracle")


def test_precision_1_session_on_the_tiny_shape_recomputes_like_mmu_generate():
    """accuracy mode has no production-kernel form at the tiny shape (the engine refuses a KV-cached prefill there and mmu_generate runs
    the reference's no-cache algorithm): the session does the same on its own embeddings / mask and gives the fixture's tokens, also
    over two turns; the engine-level precision-1 append is held to the oracle at the SMALL shape below"""
    g, d, m, ids = _tiny(1)
    want = g["tokens"].tolist()
    sess = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(_pm(ids[:, :20], d)))
    mark = sess.mark()
    assert _ints(sess.generate(dev(ids[:, 20:]), max_new_tokens=len(want), top_k=1)) == want
    sess.rewind(mark)
    part = _ints(sess.generate(dev(ids[:, 20:]), max_new_tokens=3, top_k=1))
    part += _ints(sess.generate(max_new_tokens=len(want) - 3, top_k=1))
    assert part == want
    outs = sess.generate_batch(idx=[dev(ids[:, 20:]), dev(ids[:, 20:23])], max_new_tokens=2, top_k=1)
    assert len(outs) == 2 and sess.length == 25 + len(want) - 1


@functools.lru_cache(maxsize=None)
def _boundary_case(P):
    """a prompt whose prefix has P rows ([<mmu>, <soi>, image, <eoi>] + seeded random text) followed by 65 more text ids, and the
    oracle's logits of every row from P - 1 on (the rows behind <eoi> are causal, so row r is the last row of the sequence cut at r)"""
    g, d, sd, ids = _fixture()
    rs = np.random.RandomState(100 + P)
    seq = torch.tensor([ids[0, :19].tolist() + rs.randint(5, 200, size=P - 19 + 65).tolist()], dtype=torch.int64)
    ref = O.showo_logits(O.to_torch(sd), d, seq, attention_mask=_pm(seq, d))[0]
    return seq, ref


@pytest.mark.parametrize("P", [63, 64, 65])
def test_append_across_key_tile_boundaries(P):
    """prefix lengths around the 64-key tile, appended blocks of 1, 2, 63, 64, 65 rows, in one append and split in two: logits_last vs the
    oracle row; Ln = 1 gives the bits of showo_engine_decode_step"""
    L = _L()
    _, d, m, _ = _tiny()
    seq, ref = _boundary_case(P)
    eng = m.engine()
    worst = 0.0
    for Ln in (1, 2, 63, 64, 65):
        pre = _prefill(eng, d.vocab, ids=_i64(seq[:, :P]), mask=_pm(seq[:, :P], d))
        got = _append(eng, d.vocab, ids=_i64(seq[:, P:P + Ln]))
        assert _state(eng)[:2] == (P + Ln, P)
        rmax, rrms = util.relerr(got.cpu(), ref[P + Ln - 1])
        assert torch.isfinite(got).all() and rmax <= REL_MAX and rrms <= REL_RMS, (P, Ln, rmax, rrms)
        worst = max(worst, rmax)
        if Ln == 1:
            assert torch.equal(_prefill(eng, d.vocab, ids=_i64(seq[:, :P]), mask=_pm(seq[:, :P], d)), pre)
            step = torch.empty_like(got)
            tok = _i64(seq[:, P:P + 1]).reshape(1)
            L.call("showo_engine_decode_step", eng, L.ptr(tok), None, L.ptr(step), L.stream())
            torch.cuda.synchronize()
            assert torch.equal(step, got)
            continue
        a = Ln // 2
        _prefill(eng, d.vocab, ids=_i64(seq[:, :P]), mask=_pm(seq[:, :P], d))
        _append(eng, d.vocab, ids=_i64(seq[:, P:P + a]))
        two = _append(eng, d.vocab, ids=_i64(seq[:, P + a:P + Ln]))
        rmax, rrms = util.relerr(two.cpu(), ref[P + Ln - 1])
        assert torch.isfinite(two).all() and rmax <= REL_MAX and rrms <= REL_RMS, (P, Ln, "two appends", rmax, rrms)
        worst = max(worst, rmax)
    print(f"[parity] tiny append at prefix {P}, Ln in (1, 2, 63, 64, 65), one and two appends, logits_last vs oracle: worst rel_max={worst:.3e}")


def test_two_turns_vs_the_oracle_on_the_whole_conversation():
    """generate(q1, 6 tokens), then a second question: the logits its first token is drawn from are the oracle's last row on
    [prompt + q1 + answer + q2] under the grown mask; the GPU's own full forward of that sequence is held to the same row"""
    g, d, m, ids = _tiny()
    sd = _fixture()[2]
    q2 = torch.tensor([[31, 7, 150, 42]], dtype=torch.int64)
    sess = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(_pm(ids[:, :20], d)))
    a1 = _ints(sess.generate(dev(ids[:, 20:]), max_new_tokens=6, top_k=1))
    assert a1 == g["tokens"].tolist() and sess.length == 30
    seq = torch.cat([ids, torch.tensor([a1], dtype=torch.int64), q2], dim=1)
    big = _pm(seq, d)
    ref = O.showo_logits(O.to_torch(sd), d, seq, attention_mask=big)[0, -1]
    eng = m.engine()
    mark = sess.mark()
    got = _append(eng, d.vocab, ids=_i64([a1[-1]] + q2[0].tolist()))  # what the session's next generate appends
    _check(got.cpu(), ref, 0, "tiny second turn (35 rows in the cache), logits of its first token vs oracle")
    own = m(dev(seq), attention_mask=dev(big))[0, -1]
    _check(own.cpu(), ref, 0, "tiny second turn, the GPU's own full forward, last row vs oracle")
    _L().call("showo_engine_cache_rewind", eng, mark[0], _L().stream())
    a2 = _ints(sess.generate(dev(q2), max_new_tokens=4, top_k=1))
    assert a2[0] == int(got.argmax()) and len(a2) == 4 and sess.length == 30 + 5 + 3
    # continuing the answer token by token equals asking for it at once
    sess.rewind(mark)
    whole = _ints(sess.generate(dev(q2), max_new_tokens=9, top_k=1))
    sess.rewind(mark)
    parts = _ints(sess.generate(dev(q2), max_new_tokens=4, top_k=1))
    assert parts == a2
    parts += _ints(sess.generate(max_new_tokens=5, top_k=1))
    assert parts == whole


def _questions(n):
    rs = np.random.RandomState(5)
    return [torch.tensor([rs.randint(5, 200, size=1 + (3 * b + b % 2) % 9).tolist()], dtype=torch.int64) for b in range(n)]


def _sequential(sess, qs, gen=None, **kw):
    out = []
    for b, q in enumerate(qs):
        a = {k: (v[b] if isinstance(v, list) else v) for k, v in kw.items()}
        mark = sess.mark()
        out.append(_ints(sess.generate(dev(q), generator=gen, **a)))
        sess.rewind(mark)
    return out


@pytest.mark.parametrize("precision", [0, 2])
def test_forked_slot_gives_the_bits_of_the_engine_cache(precision):
    """contract 1 through the C ABI, n = 3 ragged questions: logits_last of the append is bit-identical in the engine's cache and in a
    forked slot, and so is every decode logit afterwards (4 greedy steps)"""
    L = _L()
    g, d, m, ids = _tiny(precision)
    eng = m.engine()
    qs = _questions(3)
    _prefill(eng, d.vocab, ids=_i64(ids[:, :20]), mask=_pm(ids[:, :20], d))
    want = []
    for q in qs:
        lg = _append(eng, d.vocab, ids=_i64(q))
        tok = lg.argmax().reshape(1).to(torch.int64)
        out = torch.empty((4,), dtype=torch.int64, device="cuda")
        ws = torch.empty_like(lg)
        L.call("showo_engine_decode_greedy", eng, L.ptr(tok), 4, L.ptr(out), L.ptr(ws), 0, L.stream())
        torch.cuda.synchronize()
        want.append((lg, out.tolist(), ws.clone()))
        L.call("showo_engine_cache_rewind", eng, 20, L.stream())
    L.call("showo_engine_batch_begin", eng, 3, 20 + 9 + 4 + 1)
    first = torch.empty((3,), dtype=torch.int64, device="cuda")
    for b, q in enumerate(qs):
        L.call("showo_engine_batch_fork", eng, b, L.stream())
        lg = _append(eng, d.vocab, ids=_i64(q), slot=b)
        assert torch.equal(lg, want[b][0]), ("append logits", b, float((lg - want[b][0]).abs().max()))
        first[b] = lg.argmax()
    out = torch.empty((3, 4), dtype=torch.int64, device="cuda")
    ws = torch.empty((3, d.vocab), dtype=torch.float32, device="cuda")
    L.call("showo_engine_batch_decode_greedy", eng, L.ptr(first), 4, L.ptr(out), L.ptr(ws), 0, L.stream())
    torch.cuda.synchronize()
    for b in range(3):
        assert out[b].tolist() == want[b][1]
        assert torch.equal(ws[b], want[b][2]), ("decode logits", b)
    assert _state(eng)[:2] == (20, 20)  # the engine's own cache is where the rewinds left it


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("n", [3, 11])
def test_generate_batch_equals_generate_plus_rewind(n, precision):
    """contract 1 through the session: greedy, top-k with one generator (the rule of test_mmu_generate_batch_draws_like_sequential_calls:
    the batch equals the sequential calls from an identically seeded generator), with an <eot> that stops some sequences early, eager
    and graph; n = 11 refills slots, a refill being fork + append.  The session itself is unchanged by generate_batch."""
    g, d, m, ids = _tiny(precision)
    qs = _questions(n)
    dq = [dev(q) for q in qs]
    sess = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(_pm(ids[:, :20], d)))
    sess.generate(dev(ids[:, 20:]), max_new_tokens=3, top_k=1)  # a state with a pending token: every block gets it in front
    state = sess.mark()
    before = _sequential(sess, qs[:1], max_new_tokens=5, top_k=1)[0]
    ks, ts = [1, 5, None, 1], [1.0, 0.7, 1.3, 1.0]
    mixed = dict(top_k=[ks[b % 4] for b in range(n)], temperature=[ts[b % 4] for b in range(n)])
    for graph in (0, 1):
        m.decode_graph = graph
        for kw in (dict(top_k=1), dict(top_k=5, temperature=0.7), mixed):
            want = _sequential(sess, qs, _gen(5), max_new_tokens=20, **kw)
            got = [_ints(r) for r in sess.generate_batch(idx=dq, max_new_tokens=20, generator=_gen(5), **kw)]
            assert got == want, (graph, kw)
            assert sess.mark() == state and _state(m.engine())[0] == state[0]
            eot = _sequential(sess, qs, _gen(9), max_new_tokens=20, **kw)[1][3]  # sequence 1 (and any other that draws it) stops early
            want = _sequential(sess, qs, _gen(9), max_new_tokens=20, eot_token=eot, **kw)
            got = [_ints(r) for r in sess.generate_batch(idx=dq, max_new_tokens=20, eot_token=eot, generator=_gen(9), **kw)]
            assert got == want and len(got[1]) <= 4, (graph, kw)
    # after all of it the session still continues its own conversation as if nothing had happened
    assert _ints(sess.generate(dq[0], max_new_tokens=5, top_k=1)) == before


def test_rewind_is_clean_and_the_prefix_is_never_written():
    """contract 2: generate(q), rewind, a longer different continuation, rewind, generate(q) -- the same tokens and the same append
    logits bits.  contract 3: K rows / V^T columns [0, 20) of the engine's cache are the same bytes after append, decode, rewind, fork
    and generate_batch as right after the prefill; a forked slot holds the same bytes"""
    L = _L()
    g, d, m, ids = _tiny()
    eng = m.engine()
    qs = _questions(4)
    sess = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(_pm(ids[:, :20], d)))
    k0, v0 = _cache(eng, d)
    k0, v0 = k0[:, :, :20].clone(), v0[:, :, :20].clone()
    mark = sess.mark()

    def prefix_same(what):
        k, v = _cache(eng, d)
        assert torch.equal(k[:, :, :20], k0) and torch.equal(v[:, :, :20], v0), what
        n = _state(eng)[0]
        assert bool((v[:, :, n:(n + 63) // 64 * 64] == 0).all()), (what, "V^T tail")

    lg1 = _append(eng, d.vocab, ids=_i64(qs[1]))
    prefix_same("append")
    L.call("showo_engine_cache_rewind", eng, 20, L.stream())
    first = _ints(sess.generate(dev(qs[1]), max_new_tokens=12, top_k=1))
    prefix_same("append + decode")
    sess.rewind(mark)
    prefix_same("rewind")
    other = _ints(sess.generate(dev(qs[3]), max_new_tokens=70, top_k=5, temperature=0.9, generator=_gen(1)))  # crosses the 64-key tile
    assert len(other) == 70 and sess.length > 64
    sess.rewind(mark)
    prefix_same("long continuation + rewind")
    lg2 = _append(eng, d.vocab, ids=_i64(qs[1]))
    assert torch.equal(lg1, lg2)
    L.call("showo_engine_cache_rewind", eng, 20, L.stream())
    assert _ints(sess.generate(dev(qs[1]), max_new_tokens=12, top_k=1)) == first
    sess.rewind(mark)
    sess.generate_batch(idx=[dev(q) for q in qs], max_new_tokens=6, top_k=1)
    prefix_same("generate_batch")
    ks, vs = _cache(eng, d, slot=0)
    assert torch.equal(ks[:, :, :20], k0) and torch.equal(vs[:, :, :20], v0)


def test_nan_left_in_the_cache_by_a_longer_sequence_never_reaches_an_append():
    """a 130-row prefill whose embedding row 100 is NaN leaves NaN in K rows / V^T columns [100, 130); a fresh 60-row prefix plus a
    10-row append reads the key tile [64, 128): finite logits, bit-equal to the same two calls on a newly built model"""
    g, d, m, ids = _tiny(max_seq=192)
    eng = m.engine()
    rs = np.random.RandomState(9)
    seq = torch.tensor([ids[0, :19].tolist() + rs.randint(5, 200, size=51).tolist()], dtype=torch.int64)
    emb = torch.from_numpy(rs.standard_normal((1, 130, d.hidden)).astype(np.float32) * 0.05)
    emb[0, 100] = float("nan")
    poisoned = _prefill(eng, d.vocab, emb=dev(emb))
    assert torch.isnan(poisoned).any()
    _, v = _cache(eng, d)
    assert bool(torch.isnan(v[:, :, 100:130].view(torch.bfloat16).float()).any())
    _prefill(eng, d.vocab, ids=_i64(seq[:, :60]), mask=_pm(seq[:, :60], d))
    got = _append(eng, d.vocab, ids=_i64(seq[:, 60:]))
    assert torch.isfinite(got).all()
    m2 = util.build_showo(d, _fixture()[2], max_seq=192)
    e2 = m2.engine()
    _prefill(e2, d.vocab, ids=_i64(seq[:, :60]), mask=_pm(seq[:, :60], d))
    assert torch.equal(_append(e2, d.vocab, ids=_i64(seq[:, 60:])), got)
    # the same through a slot: the batch caches are zeroed when allocated, so poison slot 0 with the NaN sequence first
    L = _L()
    L.call("showo_engine_batch_begin", eng, 2, 192)
    mk = None
    lg = torch.empty((d.vocab,), dtype=torch.float32, device="cuda")
    e = dev(emb)
    L.call("showo_engine_batch_prefill", eng, 0, None, L.ptr(e), mk, 130, L.ptr(lg), L.stream())
    L.call("showo_engine_cache_rewind", eng, 60, L.stream())
    L.call("showo_engine_batch_fork", eng, 0, L.stream())
    assert torch.equal(_append(eng, d.vocab, ids=_i64(seq[:, 60:]), slot=0), got)


def test_refusals_change_no_state():
    L = _L()
    lib = L.load()
    g, d, _, ids = _tiny()
    m = util.build_showo(d, _fixture()[2], max_batch=16, max_seq=128)  # 2048 workspace rows = the cache's capacity
    eng = m.engine()
    lg = torch.empty((d.vocab,), dtype=torch.float32, device="cuda")
    q = _i64(ids[:, 20:])
    s = L.stream()
    assert lib.showo_engine_prefill_append(eng, L.ptr(q), None, 5, L.ptr(lg), s) == 1       # append before any prefill
    assert lib.showo_engine_cache_rewind(eng, 0, s) == 1
    assert lib.showo_engine_batch_fork(eng, 0, s) == 1                                      # no batch, no prefill
    _prefill(eng, d.vocab, ids=_i64(ids[:, :20]), mask=_pm(ids[:, :20], d))
    _append(eng, d.vocab, ids=q)
    st = _state(eng)
    assert st[:2] == (25, 20) and st[3] == 1
    assert lib.showo_engine_cache_rewind(eng, 19, s) == 1 and _state(eng) == st             # below the prefix
    assert lib.showo_engine_cache_rewind(eng, 26, s) == 1 and _state(eng) == st             # above the length
    big = _i64(torch.zeros((1, 2049), dtype=torch.int64))
    assert lib.showo_engine_prefill_append(eng, L.ptr(big), None, 2023, L.ptr(lg), s) == 5 and _state(eng) == st   # 25 + 2023 + 1 > 2048
    assert b"cache full" in lib.showo_last_error()
    assert lib.showo_engine_prefill_append(eng, L.ptr(big), None, 2049, L.ptr(lg), s) == 5 and _state(eng) == st   # more rows than the workspace
    assert b"workspace" in lib.showo_last_error()
    assert lib.showo_engine_prefill_append(eng, L.ptr(q), L.ptr(lg), 5, L.ptr(lg), s) == 1 and _state(eng) == st   # ids AND embeds
    L.call("showo_engine_batch_begin", eng, 2, 25)                                          # capacity 64 > 25 + 1: fits
    L.call("showo_engine_batch_fork", eng, 1, s)
    assert lib.showo_engine_batch_prefill_append(eng, 0, L.ptr(q), None, 5, L.ptr(lg), s) == 1   # slot 0 holds nothing
    assert lib.showo_engine_batch_prefill_append(eng, 1, L.ptr(big), None, 64, L.ptr(lg), s) == 5  # past the slot's capacity
    _append(eng, d.vocab, ids=_i64(torch.zeros((1, 50), dtype=torch.int64)))
    assert _state(eng)[0] == 75
    assert lib.showo_engine_batch_fork(eng, 0, s) == 5                                      # 75 + 1 > the batch's capacity of 64
    m.set_precision(2)
    eng = m.engine()
    assert lib.showo_engine_prefill_append(eng, L.ptr(q), None, 5, L.ptr(lg), s) != 0        # weights / cache of another precision
    # a session used after mmu_generate, after another session, after a precision switch
    m.set_precision(0)
    sess = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(_pm(ids[:, :20], d)))
    m.mmu_generate(dev(ids), attention_mask=dev(g["mask"]), max_new_tokens=2, top_k=1)
    for call in (lambda: sess.generate(dev(ids[:, 20:]), max_new_tokens=2, top_k=1), lambda: sess.rewind(sess.mark()),
                 lambda: sess.generate_batch(idx=[dev(ids[:, 20:])] * 2, max_new_tokens=2, top_k=1)):
        with pytest.raises(RuntimeError, match="stale"):
            call()
    s1 = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(_pm(ids[:, :20], d)))
    s2 = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(_pm(ids[:, :20], d)))
    with pytest.raises(RuntimeError, match="stale"):
        s1.generate(dev(ids[:, 20:]), max_new_tokens=2, top_k=1)
    assert len(s2.generate(dev(ids[:, 20:]), max_new_tokens=2, top_k=1)) == 2
    m.set_precision(2)
    with pytest.raises(RuntimeError, match="stale"):
        s2.generate(max_new_tokens=2, top_k=1)
    with pytest.raises(ValueError):
        s2.rewind((19, None))


# ---- SMALL dims: the fused two-GEMM layer at pos0 > 0, and accuracy mode in its production-kernel form -------------------------------
@functools.lru_cache(maxsize=None)
def _small_case():
    d = Wt.ShowoDims(**Wt.SMALL)
    sd = Wt.make_showo_state(d, seed=11)
    ids = _fixture()[3]
    rs = np.random.RandomState(21)
    seq = torch.tensor([ids[0, :19].tolist() + rs.randint(5, 200, size=370 - 19).tolist()], dtype=torch.int64)
    ref = O.showo_logits(O.to_torch(sd), d, seq, attention_mask=_pm(seq, d))[0, -1]
    return d, sd, seq, ref


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_small_dims_300_row_append_takes_the_fused_layer(precision):
    """hidden 256, 2 layers: a 70-row prefix and a 300-row append (>= 256 rows: the fused [Wqkv ; W1] projection + K-concatenated
    residual GEMM at pos0 = 70, more rows than max_seq but within max_batch * max_seq) vs the oracle; precision 1 runs its
    production-kernel form here (3 * hidden is a multiple of 256)"""
    d, sd, seq, ref = _small_case()
    m = util.build_showo(d, sd, max_batch=4, max_seq=128)
    m.set_precision(precision)
    eng = m.engine()
    if precision == 1:
        assert _L().load().showo_engine_precise_fast(eng) == 1
    _prefill(eng, d.vocab, ids=_i64(seq[:, :70]), mask=_pm(seq[:, :70], d))
    got = _append(eng, d.vocab, ids=_i64(seq[:, 70:]))
    assert _state(eng)[:2] == (370, 70)
    _check(got.cpu(), ref, precision, "SMALL prefix 70 + append 300, logits_last vs oracle")
    _L().call("showo_engine_cache_rewind", eng, 70, _L().stream())
    two = _append(eng, d.vocab, ids=_i64(seq[:, 70:200]))
    two = _append(eng, d.vocab, ids=_i64(seq[:, 200:]))
    _check(two.cpu(), ref, precision, "SMALL prefix 70 + appends 130 + 170, logits_last vs oracle")


def test_precision_1_session_in_its_production_kernel_form_answers_generate_batch_sequentially():
    """SMALL shape under set_precision(1): the session runs on the engine's KV cache (not the recompute path), and generate_batch of
    n >= 2 -- the batched decode refuses precision 1 -- returns what generate + rewind returns per question, greedy and sampled from
    one generator, and leaves the session where it was"""
    d, sd, seq, _ = _small_case()
    m = util.build_showo(d, sd, max_batch=4, max_seq=128)
    m.set_precision(1)
    assert _L().load().showo_engine_precise_fast(m.engine()) == 1
    sess = m.mmu_session(dev(seq[:, :70]), attention_mask=dev(_pm(seq[:, :70], d)))
    assert type(sess._be).__name__ == "_SessionEngine" and sess.length == 70
    sess.generate(dev(seq[:, 70:75]), max_new_tokens=3, top_k=1)  # a state with a pending token
    state = sess.mark()
    qs = _questions(3)
    dq = [dev(q) for q in qs]
    for kw in (dict(top_k=1), dict(top_k=5, temperature=0.7)):
        want = _sequential(sess, qs, _gen(5), max_new_tokens=6, **kw)
        got = [_ints(r) for r in sess.generate_batch(idx=dq, max_new_tokens=6, generator=_gen(5), **kw)]
        print(f"[parity] SMALL precision 1 generate_batch {kw}", got, "sequential", want)
        assert got == want and all(len(r) == 6 for r in got), kw
        assert sess.mark() == state and _state(m.engine())[0] == state[0]


def test_a_session_whose_engine_was_dropped_is_stale():
    """configure_workspace destroys the engine the session was opened on: the next call reports the session stale without asking
    anything of the destroyed handle, also once the model has built a new engine"""
    g, d, m, ids = _tiny()
    sess = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(_pm(ids[:, :20], d)))
    m.configure_workspace(8, 128)
    with pytest.raises(RuntimeError, match="stale"):
        sess.generate(dev(ids[:, 20:]), max_new_tokens=2, top_k=1)
    s2 = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(_pm(ids[:, :20], d)))  # a new engine, its first prefill: epoch 1 again
    with pytest.raises(RuntimeError, match="stale"):
        sess.rewind(sess.mark())
    assert _ints(s2.generate(dev(ids[:, 20:]), max_new_tokens=6, top_k=1)) == g["tokens"].tolist()


def test_a_generate_that_fails_midway_leaves_the_session_where_it_was():
    """the decode loop runs into the end of the cache (capacity 64 rows at max_batch * max_seq = 64): the error reaches the caller, the
    rows the call wrote are dropped from the engine's cache, and the same session answers a shorter request as a fresh one does"""
    g, d, sd, ids = _fixture()
    m = util.build_showo(d, sd, max_batch=1, max_seq=64)
    sess = m.mmu_session(dev(ids[:, :20]), attention_mask=dev(_pm(ids[:, :20], d)))
    cap = _state(m.engine())[2]
    with pytest.raises(RuntimeError):
        sess.generate(dev(ids[:, 20:]), max_new_tokens=cap, top_k=1)
    assert sess.mark() == (20, None) and _state(m.engine())[0] == 20
    assert _ints(sess.generate(dev(ids[:, 20:]), max_new_tokens=6, top_k=1)) == g["tokens"].tolist()


# ---- full size: the T < 256 layer at hidden 2048 / ffn 8192 (split-K shapes the tiny model never meets) ---------------------------------
def test_full_size_cfg4_prefix_607_plus_question_24_vs_reference():
    """BASELINE cfg4 at model scale (tests/golden/showo_full_cfg4.npz): prefix = the first 607 embeddings under
    create_attention_mask_for_mmu_vit, append = the last 24.  logits_last and the 8 teacher-forced decode steps vs the reference's
    last_logits at REL_RMS / REL_MAX; free-running greedy tokens equal the reference's wherever its top-2 gap exceeds twice the measured
    error of that step; generate_batch of the same question 4 times gives 4 times the tokens of generate.

    Measured on an MI355X: see the [parity] lines of this test in the run's summary."""
    g = util.golden("showo_full_cfg4.npz")
    d = Wt.ShowoDims(w_clip_vit=True)
    sd = Wt.make_showo_state(d, seed=int(g["seed"]))
    m = util.build_showo(d, sd, max_batch=1, max_seq=768)
    del sd
    L = _L()
    feats = torch.from_numpy(np.random.RandomState(int(g["feat_seed"])).standard_normal((1, 576, 1024)).astype(np.float32)).cuda()
    ids_llava = torch.from_numpy(g["ids_llava"].astype(np.int64)).cuda()
    toks_ref = g["tokens"].tolist()
    cols = torch.from_numpy(g["cols"]).cuda()
    tab = m.showo.model.embed_tokens.weight
    with torch.no_grad():
        txt = tab[ids_llava]
        emb = torch.cat([txt[:, :30], m.mm_projector(feats), txt[:, 30:]], dim=1).float().contiguous()
    assert emb.shape[1] == 631
    P = util.pkg().prompting_utils
    full_mask = P.create_attention_mask_for_mmu_vit(emb, system_prompt_len=28)
    assert P.mmu_prefix_is_exact(full_mask, 607)
    prefix, question = emb[:, :607].contiguous(), emb[:, 607:].contiguous()
    pmask = P.create_attention_mask_for_mmu_vit(prefix, system_prompt_len=28)
    assert torch.equal(pmask[0, 0], full_mask[0, 0, :607, :607])
    eng = m.engine()
    _prefill(eng, d.vocab, emb=prefix, mask=pmask[0])
    logits = _append(eng, d.vocab, emb=question)
    assert _state(eng)[:2] == (631, 607)
    last_ref = torch.from_numpy(g["last_logits"])
    worst, errs = 0.0, []
    for j, t in enumerate(toks_ref):
        torch.cuda.synchronize()
        diff = (logits[cols].cpu() - last_ref[j]).double()
        errs.append(float(diff.abs().max()))
        rel_max, rel_rms = errs[-1] / float(g["last_absmax"][j]), float(diff.pow(2).mean().sqrt() / last_ref[j].double().pow(2).mean().sqrt())
        worst = max(worst, rel_max)
        print(f"[parity] full-size cfg4 prefix 607 + append 24, step {j}: rel_max={rel_max:.3e} rel_rms={rel_rms:.3e}")
        assert rel_rms <= REL_RMS and rel_max <= REL_MAX, (j, rel_max, rel_rms)
        if j + 1 < len(toks_ref):
            tok = torch.tensor([t], dtype=torch.int64, device="cuda")
            L.call("showo_engine_decode_step", eng, L.ptr(tok), None, L.ptr(logits), L.stream())
    print(f"[parity] full-size cfg4 prefix 607 + append 24, append logits and {len(toks_ref) - 1} teacher-forced steps: worst rel_max={worst:.3e}")
    sess = m.mmu_session(input_embeddings=prefix, attention_mask=pmask[0])
    mark = sess.mark()
    toks = _ints(sess.generate(input_embeddings=question, max_new_tokens=len(toks_ref), top_k=1))
    div = next((j for j, (a, b) in enumerate(zip(toks, toks_ref)) if a != b), None)
    print(f"[parity] full-size cfg4 session greedy tokens: {toks} vs reference {toks_ref}; first divergence: {div}; reference top-2 gaps "
          f"{np.round(g['last_top2_gap'], 4).tolist()}, measured abs logit error per step {np.round(errs, 4).tolist()}")
    for j in range(len(toks_ref)):
        if toks[j] != toks_ref[j]:
            assert float(g["last_top2_gap"][j]) <= 2.0 * errs[j], (j, toks, toks_ref)  # a flipped arg-max must be a near tie
            break
    sess.rewind(mark)
    got4 = [_ints(r) for r in sess.generate_batch(input_embeddings=[question] * 4, max_new_tokens=len(toks_ref), top_k=1)]
    assert got4 == [toks] * 4
    assert sess.mark() == mark and _state(eng)[0] == 607
