"""CPU: a model of the summation order the fp64-query dense kernels (K1D, dense_scan_f64.hip, and the score-array
kernel dense_scores_f64_kernel) are specified to use, with exact fused multiply-adds:

  * 64 lanes per row; lane l runs ONE chain acc = fma(double(e[c]), q[c], acc) from 0.0 over c = 4l .. 4l+3, then the same
    four offsets of each following 256-float chunk, ascending; offsets past D are skipped;
  * the butterfly acc += acc[lane ^ 32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1;

an FMA being the exact product plus the accumulator, rounded ONCE (fractions.Fraction -> float is correctly rounded).
tests/test_gpu_dense_f64_scan.py holds rows of every served dimension to this model's BITS, so the order is pinned to
this text and not only to the other kernel.  Finite inputs only (NaN / inf are the GPU test's edge cases)."""
from fractions import Fraction

import numpy as np
import pytest


def fma(a: float, b: float, c: float) -> float:
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def model_score(row: np.ndarray, q: np.ndarray) -> float:
    """The fp64 score of one fp32 row and one fp64 query in the kernels' order."""
    row = np.asarray(row, dtype=np.float32)
    q = np.asarray(q, dtype=np.float64)
    d = row.size
    assert q.size == d and d % 4 == 0
    acc = [0.0] * 64
    for lane in range(64):
        a = 0.0
        for chunk in range(0, d, 256):
            for j in range(4):
                c = chunk + 4 * lane + j
                if c < d:
                    a = fma(float(row[c]), float(q[c]), a)
        acc[lane] = a
    for stride in (32, 16, 8, 4, 2, 1):
        acc = [acc[lane] + acc[lane ^ stride] for lane in range(64)]
    assert all(np.float64(a).tobytes() == np.float64(acc[0]).tobytes() for a in acc)  # every lane ends with the sum
    return acc[0]


def test_fma_rounds_once():
    # 1 + 2^-53 + 2^-106-ish: a product whose low bits decide the rounding of the sum
    a, b = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30  # a * b = 1 + 2^-29 + 2^-60 (not a double)
    assert fma(a, b, -1.0) == 2.0 ** -29 + 2.0 ** -60
    assert a * b - 1.0 == 2.0 ** -29  # the separately rounded product lost the 2^-60


@pytest.mark.parametrize("d", [8, 384, 768])
def test_model_agrees_with_numpy_inside_the_error_bound(d):
    """Both the model and np.dot are fp64 sums of the D exact products e[c] * q[c] in SOME order with one rounding per
    operation: each is within gamma_D * sum |e[c] q[c]| of the exact value (Higham, Accuracy and Stability, (3.5):
    gamma_n = n u / (1 - n u), u = 2^-53, for any order of summation; an FMA only removes roundings), so they are
    within twice that of each other -- and the model within gamma_D of the exact dot product itself."""
    rng = np.random.default_rng(100 + d)
    u = 2.0 ** -53
    gamma = d * u / (1 - d * u)
    for _ in range(3):
        row = rng.standard_normal(d, dtype=np.float32)
        row /= np.linalg.norm(row)
        q = rng.standard_normal(d)
        q /= np.linalg.norm(q)
        got = model_score(row, q)
        mag = float(np.sum(np.abs(row.astype(np.float64) * q)))
        exact = sum(Fraction(float(x)) * Fraction(float(y)) for x, y in zip(row, q))
        assert abs(Fraction(got) - exact) <= Fraction(gamma * mag)
        assert abs(got - float(np.dot(row.astype(np.float64), q))) <= 2 * gamma * mag


def test_partial_last_chunk_skips_idle_lanes():
    """D = 100: lanes 0..24 hold one float4 each, the others stay 0.0; D = 260: lane 0 has two chunks, lane 1.. one."""
    rng = np.random.default_rng(7)
    for d in (100, 260):
        row = rng.standard_normal(d, dtype=np.float32)
        q = rng.standard_normal(d)
        exact = sum(Fraction(float(x)) * Fraction(float(y)) for x, y in zip(row, q))
        mag = float(np.sum(np.abs(row.astype(np.float64) * q)))
        assert abs(Fraction(model_score(row, q)) - exact) <= Fraction(d * 2.0 ** -53 * mag * 1.01)
