"""The host reference of the re-rank stage (tests/rerank_ref.py), checked on the CPU: its exact values are the written-out
8-lane chain's bit for bit, and its dropping, ordering and padding rules hold on a table small enough to read."""
import numpy as np
import pytest

from tests.rerank_ref import NEUTRAL, exact_chain, exact_values, rerank_reference

F = np.float32


@pytest.mark.parametrize("l2", [True, False])
@pytest.mark.parametrize("d", [16, 48, 128, 272, 1536])
def test_oracle_values_are_the_chain(d, l2):
    rng = np.random.default_rng(d)
    y = (rng.standard_normal((40, d)) * 20 + 1000).astype(F)
    x = (rng.standard_normal((6, d)) * 20 + 1000).astype(F)
    ids = np.tile(np.arange(40, dtype=np.int64), (6, 1))
    val, live = exact_values(x, y, ids, l2)
    assert live.all() and val.tobytes() == exact_chain(x, y, l2).tobytes()


@pytest.mark.parametrize("l2", [True, False])
def test_dropping_ordering_padding(l2):
    d = 16
    raw = np.zeros((8, d), F)
    raw[:, 0] = [1, 2, 3, 4, 5, np.nan, np.inf, 3e38]
    q = np.zeros((2, d), F)
    q[:, 0] = [0, 1]
    ids = np.array([[4, 9, 2, -1, 5, 0, 6, 3, 7, 1], [3, 3, 8, -1, 5, 6, 7, 0, 1, 2]], dtype=np.int64)
    sign = 1 if l2 else -1
    # wide window: NaN, the infinity (L2: (0 - 3e38)^2 too), ids -1 and beyond the rows are dropped
    D, I = rerank_reference(q, raw, ids, 7, l2, -3e38, 3e38)
    if l2:
        assert I[0].tolist() == [0, 1, 2, 3, 4, -1, -1] and D[0, :5].tolist() == [1, 4, 9, 16, 25]
        assert I[1, :3].tolist() == [0, 1, 2] and sorted(I[1, 3:5].tolist()) == [3, 3] and I[1, 5:].tolist() == [-1, -1]
        assert D[1, :5].tolist() == [0, 1, 4, 9, 9]
    else:
        # a zero query: 0 * y is 0 for the six finite rows (inside the window, all equal), NaN for the NaN and the infinity
        assert sorted(I[0, :6].tolist()) == [0, 1, 2, 3, 4, 7] and I[0, 6] == -1 and (D[0, :6] == 0).all()
        D, I = rerank_reference(q[1:], raw, ids[1:], 7, l2, -3e38, 3e38)
        assert I[0, 0] == 7 and D[0, 0] == F(3e38)   # 1 * 3e38 is an ordinary value inside the window
        assert sorted(I[0, 1:3].tolist()) == [3, 3] and I[0, 3:6].tolist() == [2, 1, 0] and I[0, 6] == -1
    assert (D[I < 0] == NEUTRAL[l2]).all() and NEUTRAL[l2] == sign * np.finfo(F).max
    # a window: both edges inclusive
    lo, hi = (4.0, 16.0) if l2 else (2.0, 4.0)
    D, I = rerank_reference(q[1:], raw, ids[1:], 4, l2, lo, hi)
    if l2:
        assert I[0, 0] == 2 and sorted(I[0, 1:3].tolist()) == [3, 3] and I[0, 3] == -1 and D[0, :3].tolist() == [4, 9, 9]
    else:
        assert sorted(I[0, :2].tolist()) == [3, 3] and I[0, 2:].tolist() == [2, 1] and D[0].tolist() == [4, 4, 3, 2]
    # k beyond the table
    D, I = rerank_reference(q[1:], raw, ids[1:, :3], 5, l2, -3e38, 3e38)
    assert I.shape == (1, 5) and (I[0, 2:] == -1).all() and (D[0, 2:] == NEUTRAL[l2]).all()
