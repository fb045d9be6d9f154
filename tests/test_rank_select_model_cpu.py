"""CPU: the planted inputs of tests/test_gpu_rank_wide.py hold what their generators claim, under the numpy model of the
select's order -- so the GPU comparison of the two forms cannot pass on a degenerate input."""
import numpy as np
import pytest

import rank_select_model as m


def test_model_order_by_hand():
    keys = np.full((1, 64), 7.0e30, np.float32)
    keys[0, :8] = [1.0, -0.0, 3.0, 0.0, -np.inf, 3.0, np.inf, -1.0]
    (rows, sc), = m.select_model(keys, 8, 6)
    assert rows.tolist() == [6, 2, 5, 0, 1, 3]  # +inf first, equal 3.0 by row, -0.0 == +0.0 by row, -inf never
    assert sc[:4].tolist() == [np.inf, 3.0, 3.0, 1.0]
    (rows, _), = m.select_model(keys, 8, 100)
    assert len(rows) == 7  # count = min(k, candidates)
    ties = np.zeros((1, 64), np.uint32)
    ties[0, :8] = [9, 8, 7, 6, 5, 4, 3, 2]
    (rows, _), = m.select_model(keys.astype(np.float64), 8, 3, ties=ties)
    assert rows.tolist() == [3, 4, 7]  # the tie words come back, the lower word wins among the 3.0s
    assert len(m.select_model(keys, 8, 5, seg_k=[0])[0][0]) == 0


def test_slices():
    assert m.slice_len(16385, 1) == 16448 and m.n_slices(16385, 1) == 1
    assert m.slice_len(100003, 7) == 14336 and m.n_slices(100003, 7) == 7
    # more slices asked for than the shortest slice allows: clamped, and the last slice is one score long
    assert m.slice_len(16385, 64) == m.MIN_SLICE and m.n_slices(16385, 64) == 5
    assert 16385 - 4 * m.MIN_SLICE == 1
    assert m.n_slices(65537, 64) == 17 and 65537 - 16 * m.MIN_SLICE == 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", sorted(m.GENERATORS))
@pytest.mark.parametrize("k", [1, 64, 12000, "cap", "n+5"])
def test_generators_hold_their_claims(kind, dtype, k):
    n = 20000
    k = {"cap": m.cap_of(dtype), "n+5": n + 5}.get(k, k)
    case = m.GENERATORS[kind](np.random.default_rng(5), 2, n, dtype, k)
    m.check_claims(case, n, k)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("parts", [2, 7, 64])
@pytest.mark.parametrize("k", [1, 64, 12000])
def test_planted_pair_straddles_a_slice_boundary(dtype, parts, k):
    n = 65537
    case = m.gen_planted_boundary(np.random.default_rng(6), 2, n, dtype, k, parts)
    m.check_claims(case, n, k)


@pytest.mark.parametrize("k", [64, 12000, m.CAP64])
@pytest.mark.parametrize("n", [13313, 20000])
def test_tie_form(n, k):
    case = m.gen_tie_form(np.random.default_rng(7), 2, n, np.float64, k)
    m.check_claims(case, n, k)
