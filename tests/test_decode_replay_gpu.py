"""GPU test of the shared step-replay helper (csrc/engine.h replay_steps / capture_step) under both decode loops that call it: the batch-1
loop (csrc/decode_engine.hip, showo_engine_decode_greedy) and the batched loop (csrc/decode_batch.hip, showo_engine_batch_decode_greedy).

Five greedy steps are run three ways -- one call that captures a step and replays it (use_graph = 1), one call of eager steps
(use_graph = 0), and five calls of ONE step each (n_steps = 1: the edge where nothing is captured whatever use_graph says).  A step is
the same launches in every form, so the bar is bit-exact: equal tokens and equal bits in the final logits rows."""
import ctypes as C

import pytest
import torch

import util
from util import O

pytestmark = pytest.mark.gpu

STEPS = 5
# (use_graph, steps per call): captured replay | eager loop | the no-capture edge, call by call
FORMS = {"graph": (1, STEPS), "eager": (0, STEPS), "one_step_calls": (1, 1)}


def _cache_len(L, eng):
    n = C.c_int(0)
    L.call("showo_engine_cache_state", eng, C.byref(n), None, None, None)
    return n.value


@pytest.fixture(scope="module")
def tiny():
    g = util.golden("showo_tiny_mmu.npz")
    d, sd = util.tiny_state()
    m = util.build_showo(d, sd)
    base = g["ids"][0].tolist()
    ids = [torch.tensor([base], dtype=torch.int64), torch.tensor([base[:-2] + [11, 57, 123]], dtype=torch.int64)]  # two lengths
    masks = [O.mask_mmu(t, d.eoi_id).cuda().float().contiguous() for t in ids]
    return d, m, [t.cuda() for t in ids], masks


def test_batch1_greedy_replay_eager_and_single_step_calls_agree(tiny):
    d, m, ids, masks = tiny
    L, eng, side = util.lib(), m.engine(), torch.cuda.Stream()
    P0 = ids[0].shape[1]
    got = {}
    for name, (graph, per_call) in FORMS.items():
        lg = torch.empty((d.vocab,), dtype=torch.float32, device="cuda")
        L.call("showo_engine_prefill", eng, L.ptr(ids[0]), None, L.ptr(masks[0]), P0, L.ptr(lg), L.stream())
        assert _cache_len(L, eng) == P0
        tok = lg.argmax().reshape(1).to(torch.int64)
        out = torch.empty((STEPS,), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for done in range(0, STEPS, per_call):
                L.call("showo_engine_decode_greedy", eng, L.ptr(tok), per_call, L.ptr(out[done:]), L.ptr(lg), graph, L.stream())
                assert _cache_len(L, eng) == P0 + done + per_call, name
        torch.cuda.synchronize()
        got[name] = (out.tolist(), lg.clone())
    for name in ("eager", "one_step_calls"):
        assert got[name][0] == got["graph"][0], name
        assert torch.equal(got[name][1], got["graph"][1]), name


def test_batched_greedy_replay_eager_and_single_step_calls_agree(tiny):
    d, m, ids, masks = tiny
    L, eng, side = util.lib(), m.engine(), torch.cuda.Stream()
    n = len(ids)
    L.call("showo_engine_batch_begin", eng, n, max(t.shape[1] for t in ids) + STEPS + 1)
    got = {}
    for name, (graph, per_call) in FORMS.items():
        lgs = torch.empty((n, d.vocab), dtype=torch.float32, device="cuda")
        for b in range(n):
            L.call("showo_engine_batch_prefill", eng, b, L.ptr(ids[b]), None, L.ptr(masks[b]), ids[b].shape[1], L.ptr(lgs[b]), L.stream())
        tok = lgs.argmax(dim=1).to(torch.int64)
        outs = []
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(0, STEPS, per_call):
                out = torch.empty((n, per_call), dtype=torch.int64, device="cuda")
                L.call("showo_engine_batch_decode_greedy", eng, L.ptr(tok), per_call, L.ptr(out), L.ptr(lgs), graph, L.stream())
                outs.append(out)
        torch.cuda.synchronize()
        got[name] = (torch.cat(outs, dim=1).tolist(), lgs.clone())
    for name in ("eager", "one_step_calls"):
        assert got[name][0] == got["graph"][0], name
        assert torch.equal(got[name][1], got["graph"][1]), name
