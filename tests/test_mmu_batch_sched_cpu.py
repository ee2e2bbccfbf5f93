"""CPU tests of the slot scheduler behind Showo.mmu_generate_batch (modeling_showo._mmu_batch_schedule), driven by a fake engine.

The fake engine plays the C ABI's contract (showo_engine_batch_prefill / _batch_decode_sample): a slot emits at most its budget, stops
after <eot>, and its cache grows by what it produced.  Each request's tokens are a deterministic function of (request, draw index), so
the expected output of n sequential calls is known without a GPU."""
import pytest
import torch

import util


def _mod():
    return util.pkg().modeling_showo


class FakeEngine:
    def __init__(self, lens, max_new_tokens, slots, eot, stop_at):
        self.lens, self.max_new, self.slots, self.eot, self.stop_at = lens, max_new_tokens, slots, eot, stop_at
        self.cap = max(lens) + max_new_tokens + 1
        self.occ = [None] * slots
        self.busy = [False] * slots  # the slot's occupant has tokens left to emit
        self.pos = [0] * slots     # cache length of each slot
        self.drawn = [0] * slots   # draws made by the slot's occupant
        self.prefills = []         # (slot, request) in call order
        self.budgets = []

    def token(self, r, d):
        """draw d of request r; with an <eot> id, request r emits it at draw stop_at[r]"""
        return self.eot if self.eot is not None and d == self.stop_at.get(r) else 1000 * (r + 1) + d

    def prefill(self, s, r):
        assert not self.busy[s] and all(self.busy[:s])  # the lowest free slot: no running request is replaced
        assert self.lens[r] + 1 <= self.cap
        self.prefills.append((s, r))
        self.occ[s], self.pos[s], self.drawn[s] = r, self.lens[r], 1
        t = self.token(r, 0)
        self.busy[s] = not ((self.eot is not None and t == self.eot) or self.max_new <= 1)
        return t

    def decode(self, m, budget, draw0):
        assert len(budget) == len(draw0) == self.slots and 1 <= m <= 16
        self.budgets.append(list(budget))
        rows, produced = [], []
        for s in range(self.slots):
            r, b = self.occ[s], budget[s]
            assert 0 <= b <= m
            row, k = [-1] * m, 0
            assert (b > 0) == self.busy[s]  # every running slot decodes, no free slot does
            if b:
                assert draw0[s] == self.drawn[s]                 # draw indices continue where the slot stopped
                assert self.pos[s] + b <= self.cap               # never past the slot's capacity
                assert b <= self.max_new - self.drawn[s]         # never more than the request may still emit
                while k < b:
                    t = self.token(r, draw0[s] + k)
                    row[k] = t
                    k += 1
                    if self.eot is not None and t == self.eot:
                        break
                self.pos[s] += k
                self.drawn[s] += k
                if self.drawn[s] == self.max_new or (self.eot is not None and row[k - 1] == self.eot):
                    self.busy[s] = False
            rows.append(row)
            produced.append(k)
        return rows, produced


def _expected(eng, n, max_new, eot):
    out = []
    for r in range(n):
        toks = []
        for d in range(max_new):
            toks.append(eng.token(r, d))
            if eot is not None and toks[-1] == eot:
                break
        out.append(toks)
    return out


@pytest.mark.parametrize("n,slots,max_new", [(2, 2, 40), (5, 5, 17), (12, 8, 40), (20, 4, 33), (20, 8, 1), (9, 8, 0), (32, 8, 100)])
def test_schedule_serves_every_request_once_in_input_order(n, slots, max_new):
    M = _mod()
    eot = 7
    lens = [30 + (37 * r) % 50 for r in range(n)]
    stop_at = {r: (r * 5) % 23 for r in range(0, n, 3)}  # every third request ends at <eot> (some at the prefill token)
    eng = FakeEngine(lens, max_new, slots, eot, stop_at)
    got = M._mmu_batch_schedule(eng, n, slots, max_new, eot)
    assert got == _expected(eng, n, max_new, eot)
    # every request prefilled exactly once, in input order (the fake engine checks that each goes into the lowest free slot)
    assert [r for _, r in eng.prefills] == list(range(n))
    assert not any(eng.busy)


def test_schedule_without_eot_and_with_long_before_short():
    """long requests first: each slot gets a shorter successor; budgets follow what every slot may still emit"""
    M = _mod()
    n, slots, max_new = 12, 4, 40
    lens = [100 - 5 * r for r in range(n)]
    stop_at = {r: 40 - 3 * r for r in range(n)}  # later requests end earlier
    eng = FakeEngine(lens, max_new, slots, None, stop_at)
    got = M._mmu_batch_schedule(eng, n, slots, max_new, None)
    assert got == _expected(eng, n, max_new, None) and all(len(r) == max_new for r in got)
    eng = FakeEngine(lens, max_new, slots, 99999, stop_at)
    got = M._mmu_batch_schedule(eng, n, slots, max_new, 99999)
    assert got == _expected(eng, n, max_new, 99999) and [len(r) for r in got] == [min(max_new, stop_at[r] + 1) for r in range(n)]
    assert max(max(b) for b in eng.budgets) <= 16
    assert [r for _, r in eng.prefills] == list(range(n))


def test_seeds_are_drawn_like_sequential_calls():
    """one torch.randint(0, 2**62) per sampled sequence (top_k != 1), in sequence order; none for greedy sequences"""
    M = _mod()
    top_ks = [1, 5, None, 1, 50, 0]
    g = torch.Generator().manual_seed(1234)
    got = M._mmu_batch_seeds(top_ks, g)
    g2 = torch.Generator().manual_seed(1234)
    want = [None if k == 1 else int(torch.randint(0, 2 ** 62, (1,), generator=g2).item()) for k in top_ks]
    assert got == want and got[0] is None and got[3] is None
    assert g.get_state().equal(g2.get_state())  # the generator is left where n sequential calls leave it
    torch.manual_seed(99)
    got = M._mmu_batch_seeds(top_ks, None)
    torch.manual_seed(99)
    assert got == [None if k == 1 else int(torch.randint(0, 2 ** 62, (1,)).item()) for k in top_ks]


def test_slot_count_is_bounded_by_the_batched_kernels():
    M = _mod()
    assert [M._mmu_batch_slots(n) for n in (2, 3, 8)] == [2, 3, 8]
    for n in (9, 16, 32, 100):
        assert 2 <= M._mmu_batch_slots(n) <= 8
