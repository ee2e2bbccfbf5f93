"""GPU tests of the stand-alone sequence-rule kernel (showo_seq_ban, csrc/seq_rules.hip) against tests/seq_rules_ref.py: the uint32 view
of every logits row equals the input except 0xFF800000 at exactly the reference's set, the history and its lengths are as the header
specifies, and the guard words around every buffer are unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

import util
import seq_rules_ref as R

pytestmark = pytest.mark.gpu

NINF = np.uint32(0xFF800000)
GUARD = 8
HIST_LD = 1003
VS = (1, 33, 4099, 58498)


def _alphabet(V):
    """5 ids that include 0 and V - 1 (fewer when the vocabulary has fewer)"""
    return sorted({0, V - 1, V // 2, V // 3, min(7, V - 1)})


def _history(rs, V, ln):
    """ln ids drawn from the alphabet -- many repeats, so several matches ban one token -- with a -1 and a V strewn in"""
    al = _alphabet(V)
    h = [al[i] for i in rs.randint(0, len(al), size=ln)]
    for j in range(ln):
        if rs.rand() < 0.03:
            h[j] = -1 if rs.rand() < 0.5 else V
    return h


def _table(rs, V, h, kind):
    """kind 0: none; 1: one sequence; 2: 64 sequences of 16 tokens; 3: two sequences banning the same token (and ids outside [0, V))"""
    al = _alphabet(V)
    pick = lambda: al[rs.randint(0, len(al))]
    if kind == 0:
        return None
    if kind == 1:
        return [[h[-1] if h else pick(), pick()]]
    if kind == 2:
        seqs = [[pick() for _ in range(16)] for _ in range(64)]
        if len(h) >= 15:
            for i in (0, 31, 63):
                seqs[i] = list(h[-15:]) + [pick()]
        return seqs
    w = pick()
    return [[h[-1] if h else pick(), w], ([h[-2], h[-1]] if len(h) >= 2 else [pick(), pick()]) + [w], [h[-1] if h else pick(), V],
            [h[-1] if h else pick(), -1]]


def _run(V, rows, lens, ngram, marks, active, kinds, min_new, gs, eot, seed, hist_ld=HIST_LD):
    """one launch over `rows` rows and its check.  lens: history lengths; marks: None or per row an id; active: None or per row 0 / 1;
    kinds: per row the table kind; min_new / gs: per row the minimum length and the generated count g the row is to have"""
    L = util.lib()
    rs = np.random.RandomState(seed)
    ld = V + 3 if V % 2 == 0 else V + 4  # odd: the rows' alignments alternate
    al = _alphabet(V)
    lg = rs.standard_normal(GUARD + rows * ld + GUARD).astype(np.float32)
    lg[rs.randint(0, lg.size, size=max(1, lg.size // 50))] = -np.inf  # some entries are banned already
    hist = np.array([al[i] for i in rs.randint(0, len(al), size=GUARD + rows * hist_ld + GUARD)], dtype=np.int32)  # (the rows' stale tails too)
    hlen = np.full(GUARD + rows + GUARD, 12345, dtype=np.int32)
    want_lg, want_hist, want_len = lg.view(np.uint32).copy(), hist.copy(), hlen.copy()
    tables, ctx, keep = [], [], []
    for r in range(rows):
        h0 = _history(rs, V, lens[r])
        hist[GUARD + r * hist_ld:GUARD + r * hist_ld + lens[r]] = h0
        hlen[GUARD + r] = lens[r]
        mk = None if marks is None else marks[r]
        valid = mk is not None and 0 <= mk < V
        h = h0 + ([mk] if valid else [])
        bad = _table(rs, V, h, kinds[r])
        tables.append(None if bad is None else util.dev(np.array(R.table_of(bad), dtype=np.int32)))
        ctx.append(max(0, len(h) - gs[r]))
        on = active is None or active[r]
        if on:
            ban = R.banned(h, V, ngram[r], bad or (), ctx[r], min_new[r], eot)
            for w in ban:
                want_lg[GUARD + r * ld + w] = NINF
    want_hist[:], want_len[:] = hist, hlen
    for r in range(rows):
        mk = None if marks is None else marks[r]
        if (active is None or active[r]) and mk is not None and 0 <= mk < V and lens[r] < hist_ld:
            want_hist[GUARD + r * hist_ld + lens[r]] = mk
            want_len[GUARD + r] = lens[r] + 1
    d_lg, d_hist, d_len = util.dev(lg), util.dev(hist), util.dev(hlen)
    d_mark = None if marks is None else util.dev(np.array(marks, dtype=np.int64))
    d_act = None if active is None else util.dev(np.array(active, dtype=np.int32))
    a_n, a_c, a_m = (C.c_int32 * rows)(*ngram), (C.c_int32 * rows)(*ctx), (C.c_int32 * rows)(*min_new)
    a_b = (C.c_void_p * rows)(*[None if t is None else t.data_ptr() for t in tables])
    q = L.SeqRules(d_hist.data_ptr() + 4 * GUARD, hist_ld, d_len.data_ptr() + 4 * GUARD, C.cast(a_n, C.c_void_p), C.cast(a_c, C.c_void_p),
                   C.cast(a_m, C.c_void_p), eot, C.cast(a_b, C.c_void_p) if any(t is not None for t in tables) or seed % 2 else None)
    L.call("showo_seq_ban", d_lg.data_ptr() + 4 * GUARD, ld, rows, V, C.byref(q), L.ptr(d_mark), L.ptr(d_act), L.stream())
    torch.cuda.synchronize()
    got = d_lg.cpu().numpy().view(np.uint32)
    diff = np.nonzero(got != want_lg)[0]
    assert diff.size == 0, (V, rows, ngram, [(int(i - GUARD) // ld, int(i - GUARD) % ld) for i in diff[:8]])
    assert np.array_equal(d_hist.cpu().numpy(), want_hist) and np.array_equal(d_len.cpu().numpy(), want_len), (V, rows, ngram)
    return int((want_lg != lg.view(np.uint32)).sum())


def _lengths(n):
    return [0, 1, max(n - 2, 0), n - 1, n, 255, 256, 257, 1000, HIST_LD - 1, HIST_LD]


@pytest.mark.parametrize("V", VS)
def test_every_history_length_and_ngram_size(V):
    """n in {1, 2, 3, 4, 8} x the lengths {0, 1, n-2, n-1, n, 255, 256, 257, 1000, hist_ld-1, hist_ld}, one row each: without a mark,
    with marks (valid, -1, V) and with inactive rows; the tables and the minimum length vary from row to row"""
    al = _alphabet(V)
    fired = 0
    for n in (1, 2, 3, 4, 8):
        lens = _lengths(n)
        rows = len(lens)
        kinds = [(r + n) % 4 for r in range(rows)]
        min_new = [(3 + r) % 5 for r in range(rows)]
        gs = [max(min_new[r] - (r % 2), 0) for r in range(rows)]  # g = min_new - 1 and g = min_new alternate
        marks = [[al[(r + n) % len(al)], -1, V, al[0]][r % 4] for r in range(rows)]
        marks[-1] = marks[-2] = al[-1]  # hist_ld - 1 (the last append that fits) and hist_ld (a full row: seen, not stored)
        active = [0 if r % 5 == 2 else 1 for r in range(rows)]
        eot = al[len(al) // 2]
        fired += _run(V, rows, lens, [n] * rows, None, None, kinds, min_new, gs, eot, 10 * n)
        fired += _run(V, rows, lens, [n] * rows, marks, None, kinds, min_new, gs, eot, 10 * n + 1)
        fired += _run(V, rows, lens, [n] * rows, marks, active, kinds, min_new, gs, -1, 10 * n + 2)
    assert fired > 30  # the cases ban something


@pytest.mark.parametrize("rows", [1, 3, 32, 33])
def test_row_counts_with_rules_that_differ_per_row(rows):
    """33 rows: one more than a launch carries (the rows go 32 to a launch)"""
    for V in (33, 4099):
        rs = np.random.RandomState(rows + V)
        al = _alphabet(V)
        lens = [int(t) for t in rs.randint(0, 300, size=rows)]
        ngram = [[0, 1, 2, 3, 4, 8, 16][r % 7] for r in range(rows)]
        kinds = [r % 4 for r in range(rows)]
        min_new = [r % 3 for r in range(rows)]
        gs = [(r // 3) % 3 for r in range(rows)]
        marks = [[al[r % len(al)], -1][r % 3 == 1] for r in range(rows)]
        active = [int(r % 4 != 3) for r in range(rows)]
        _run(V, rows, lens, ngram, marks, active, kinds, min_new, gs, al[0], 7, hist_ld=301)
        _run(V, rows, lens, ngram, None, None, [0] * rows, [0] * rows, [0] * rows, -1, 8, hist_ld=301)


def test_beyond_the_limits_is_error_1_before_any_launch():
    L = util.lib()
    lib = L.load()
    V = 33
    lg = torch.zeros((V,), dtype=torch.float32, device="cuda")
    hist = torch.zeros((8,), dtype=torch.int32, device="cuda")
    hlen = torch.zeros((1,), dtype=torch.int32, device="cuda")
    one = lambda v: (C.c_int32 * 1)(v)
    for ngram, ctx, mn, ld in ((17, 0, 0, 8), (-1, 0, 0, 8), (2, -1, 0, 8), (2, 0, -1, 8), (2, 0, 0, 0)):
        a = (one(ngram), one(ctx), one(mn))
        q = L.SeqRules(hist.data_ptr(), ld, hlen.data_ptr(), *(C.cast(t, C.c_void_p) for t in a), 3, None)
        assert lib.showo_seq_ban(lg.data_ptr(), V, 1, V, C.byref(q), None, None, L.stream()) == 1
    assert lib.showo_seq_ban(lg.data_ptr(), V, 1, V, None, None, None, L.stream()) == 1
    torch.cuda.synchronize()
    assert not lg.any() and not hist.any() and not hlen.any()
