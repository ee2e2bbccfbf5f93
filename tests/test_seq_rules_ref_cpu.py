"""CPU tests of tests/seq_rules_ref.py, the restatement the GPU tests hold the sequence rules to: the hand-worked answers of the
issue's table, the rules' edges, and -- where transformers imports -- Hugging Face's three logits processors on random histories."""
import random

import pytest

import seq_rules_ref as R

A, B, C_, E = 3, 5, 6, 2  # three text ids and the <eot> of the table
BIAS = {A: 3000.0, B: 2000.0, C_: 1000.0}
V = 7

# (keywords of seq_rules_ref.greedy, expected tokens): the table of the path tests
TABLE = [
    (dict(bias=BIAS, steps=6, n=2), [A, A, B, A, C_, A]),
    (dict(bias=BIAS, steps=4, n=2, context=[A, B]), [A, A, C_, A]),
    (dict(bias=BIAS, steps=3, n=1), [A, B, C_]),
    (dict(bias=BIAS, steps=7, n=3), [A, A, A, B, A, A, C_]),
    (dict(bias=BIAS, steps=4, bad=[[A, A]]), [A, B, A, B]),
    (dict(bias=BIAS, steps=4, bad=[[A, A]], stops=[[B, A]]), [A, B, A]),
    (dict(bias={E: 3000.0, B: 2000.0}, steps=8, min_new=3, eot=E), [B, B, B, E]),
]


@pytest.mark.parametrize("case", range(len(TABLE)))
def test_hand_worked_table(case):
    kw, want = TABLE[case]
    assert R.greedy(V=V, **kw) == want


def test_ngram_edges():
    assert R.banned([], V, n=1) == set() and R.banned([4], V, n=1) == {4} and R.banned([4, 1, 4], V, n=1) == {1, 4}
    assert R.banned([4], V, n=2) == set()  # shorter than n: nothing
    assert R.banned([4, 4], V, n=2) == {4} and R.banned([1, 2, 1], V, n=2) == {2}
    assert R.banned([1, 2, 3, 1, 2], V, n=3) == {3} and R.banned([1, 2, 3, 1, 2], V, n=4) == set()
    assert R.banned([1, 2, 1, 3, 1], V, n=2) == {2, 3}  # several matches
    assert R.banned([1, 9, 1], V, n=2) == set() and R.banned([9, 1, 9], V, n=2) == {1}  # 9 >= V: compared, never banned
    assert R.banned([-1, 1, -1], V, n=2) == {1}


def test_bad_word_edges():
    assert R.banned([], V, bad=[[1, 2]]) == set() and R.banned([1], V, bad=[[1, 2]]) == {2}
    assert R.banned([3, 1], V, bad=[[1, 2], [3, 1, 4], [1, 2]]) == {2, 4}
    assert R.banned([1], V, bad=[[3, 1, 4]]) == set()  # the history is shorter than the prefix
    assert R.banned([3, 1], V, bad=[[3, 1, 4]]) == {4}  # the prefix is the WHOLE history: banned (Hugging Face skips this case)
    assert R.banned([1], V, bad=[[5]]) == set()  # one-token sequences are bias entries, not table entries
    assert R.banned([1], V, bad=[[1, 7]]) == set()


def test_min_length_edges():
    assert R.banned([1, 2], V, ctx_len=2, min_new=1, eot=E) == {E} and R.banned([1, 2, 4], V, ctx_len=2, min_new=1, eot=E) == set()
    assert R.banned([1, 2, 4], V, ctx_len=2, min_new=2, eot=E) == {E}
    assert R.banned([1, 2], V, ctx_len=2, min_new=5, eot=-1) == set()


def test_stop_cut():
    assert R.stop_cut([1, 2, 3, 4], [[2, 3]]) == [1, 2, 3] and R.stop_cut([1, 2, 3, 4], [[3, 2]]) == [1, 2, 3, 4]
    assert R.stop_cut([1, 2, 3, 4], [[2, 3]], eot=2) == [1, 2] and R.stop_cut([1, 2, 3, 4], [[2, 3]], eot=4) == [1, 2, 3]
    assert R.stop_cut([1, 2, 3, 4], [[4], [1, 2, 3]]) == [1, 2, 3] and R.stop_cut([], [[1]]) == []
    assert R.stop_cut([1, 1, 1], [[1, 1]]) == [1, 1]
    assert R.table_of([[1, 2], [3, 4, 5]]) == [2, 0, 2, 5, 1, 2, 3, 4, 5]


def test_reference_equals_the_transformers_processors():
    """random histories over an alphabet of 7 (repeats are common), lengths 1..40, n 1..4, 0..5 bad sequences of 2..4 tokens; only on
    histories longer than the longest sequence: there NoBadWordsLogitsProcessor has no whole-input prefix to skip"""
    transformers = pytest.importorskip("transformers")
    import torch
    rnd = random.Random(5)
    checked = 0
    for trial in range(600):
        ln = rnd.randint(1, 40)
        hist = [rnd.randrange(V) for _ in range(ln)]
        n = rnd.randint(1, 4)
        bad = [[rnd.randrange(V) for _ in range(rnd.randint(2, 4))] for _ in range(rnd.randint(0, 5))]
        if bad and ln <= max(len(s) for s in bad):
            continue
        ctx = rnd.randint(0, ln)
        min_new = rnd.randint(0, 6)
        ids, scores = torch.tensor([hist]), torch.zeros((1, V))
        scores = transformers.NoRepeatNGramLogitsProcessor(n)(ids, scores)
        if bad:
            scores = transformers.NoBadWordsLogitsProcessor(bad, eos_token_id=None)(ids, scores)
        if min_new:
            scores = transformers.MinNewTokensLengthLogitsProcessor(ctx, min_new, E)(ids, scores)
        want = {i for i in range(V) if scores[0, i] == float("-inf")}
        assert R.banned(hist, V, n, bad, ctx, min_new, E) == want, (hist, n, bad, ctx, min_new)
        checked += 1
    assert checked > 300
