"""The numpy reference of the logit adjustment (tests/logit_adjust_ref.py) against hand-worked rows and, where `transformers` is
installed, against Hugging Face's RepetitionPenaltyLogitsProcessor."""
import numpy as np
import pytest

import logit_adjust_ref as R

INF = np.float32(np.inf)


def test_hand_worked_row():
    x = np.array([2.0, -2.0, 0.0, -0.0, 3.0, -3.0, -np.inf, 1.5], dtype=np.float32)
    y = R.adjust_ref(x, [0, 1, 2, 3, 6], 2.0)
    #            2 / 2  -2 * 2  0 / 2  -0 / 2  (not in S)   -inf * 2  (not in S)
    want = np.array([1.0, -4.0, 0.0, -0.0, 3.0, -3.0, -np.inf, 1.5], dtype=np.float32)
    assert np.array_equal(R.bits(y), R.bits(want))  # bits: -0.0 stays -0.0 ("not < 0": divided)
    # a penalty below 1 rewards: positive logits grow, negative ones shrink in magnitude
    y = R.adjust_ref(x, [0, 1], 0.5)
    assert y[0] == 4.0 and y[1] == -1.0 and np.array_equal(R.bits(y[2:]), R.bits(x[2:]))


def test_bias_comes_after_the_penalty_and_minus_inf_bans():
    x = np.array([4.0, -1.0, 2.0, 0.5], dtype=np.float32)
    beta = np.array([1.0, 0.25, -np.inf, 0.0], dtype=np.float32)
    y = R.adjust_ref(x, [0, 1, 2], 4.0, beta)
    assert y.tolist() == [4.0 / 4.0 + 1.0, -1.0 * 4.0 + 0.25, -np.inf, 0.5]
    assert R.adjust_ref(np.array([-np.inf], dtype=np.float32), [0], 1.3, np.array([2.0], dtype=np.float32))[0] == -INF


def test_fp32_rounding_is_per_operation():
    x = np.array([1.0, 1.0], dtype=np.float32)
    th = np.float32(1.3)
    y = R.adjust_ref(x, [0, 1], 1.3, np.array([1e-3, 0.0], dtype=np.float32))
    q = np.float32(np.float32(1.0) / th)
    assert y[1] == q and y[0] == np.float32(q + np.float32(1e-3))
    assert y.dtype == np.float32


def test_theta_one_without_bias_is_a_copy():
    rs = np.random.RandomState(0)
    x = (3 * rs.standard_normal(257)).astype(np.float32)
    x[[3, 9]] = [-np.inf, -0.0]
    assert np.array_equal(R.bits(R.adjust_ref(x, np.arange(257), 1.0)), R.bits(x))


def test_ids_outside_the_vocabulary_are_ignored_and_bool_members_agree():
    x = np.array([1.0, -1.0, 2.0], dtype=np.float32)
    a = R.adjust_ref(x, [-1, 3, 1], 2.0)
    assert a.tolist() == [1.0, -2.0, 2.0]
    assert np.array_equal(a, R.adjust_ref(x, np.array([False, True, False]), 2.0))


@pytest.mark.parametrize("V", [1, 31, 32, 33, 65])
def test_bitmap_layout(V):
    ids = sorted({0, min(31, V - 1), min(32, V - 1), V - 1})
    w = R.bitmap_of(V, ids + [-1, V])
    assert w.shape == (R.words(V),) and w.dtype == np.uint32
    for i in ids:
        assert (int(w[i >> 5]) >> (i & 31)) & 1
    assert sum(bin(int(t)).count("1") for t in w) == len(ids)
    assert np.nonzero(R.members_of(V, w))[0].tolist() == ids
    assert R.bitmap_of(V, ids, ld=R.words(V) + 2)[R.words(V):].tolist() == [0, 0]


def test_against_hugging_face_when_it_is_installed():
    tr = pytest.importorskip("transformers")
    torch = pytest.importorskip("torch")
    rs = np.random.RandomState(1)
    V = 97
    x = (3 * rs.standard_normal((2, V))).astype(np.float32)
    ids = rs.randint(0, V, size=(2, 11))
    for theta in (0.5, 1.3):
        got = tr.RepetitionPenaltyLogitsProcessor(penalty=theta)(torch.from_numpy(ids), torch.from_numpy(x.copy())).numpy()
        for r in range(2):
            assert np.array_equal(R.bits(got[r]), R.bits(R.adjust_ref(x[r], ids[r], theta))), (theta, r)
