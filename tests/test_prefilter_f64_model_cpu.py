"""CPU: the widened bound of the float64-query prefilter (tests/prefilter_f64_model.py, DESIGN.md §3 "K1FD") holds on
the reference formulas alone -- random planted float64 queries and an input built to use the whole widening -- and the
route's entry points exist at every layer (no compute: there is no GPU in this container)."""
import math
import os
import re

import numpy as np
import pytest

import prefilter_f64_model as fm
import prefilter_model as pm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("anrag_set_dense_f64_prefilter", "anrag_dense_f64_prefilter_stats", "anrag_debug_prefilter_f64")
N, K = 4000, 25


def _corpus(dim, seed):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((N, dim), dtype=np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    e[N // 2:] *= rng.uniform(0.5, 1.5, (N - N // 2, 1)).astype(np.float32)  # norms differ: Emax is not every row's
    return e, rng


def _planted(e, rng):
    q = e[int(rng.integers(0, e.shape[0]))].astype(np.float64) + 0.05 * rng.standard_normal(e.shape[1])
    return q / np.linalg.norm(q)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("dim", [256, 768])
def test_widened_intervals_hold_the_fp64_scores_and_the_survivors_the_fp64_top_k(form, dim):
    """np.dot of the promoted matrix is an fp64 sum of the D exact products in SOME order, one rounding per operation:
    gamma64 ||q|| ||e|| holds for it as for the list scan's order (Higham, (3.5)), so it stands for s64 here."""
    e, rng = _corpus(dim, 10 * dim + form)
    emax = fm.emax_of(e)
    shares = []
    for _ in range(4):
        q = _planted(e, rng)
        q32 = fm.q32_of(q)
        assert np.any(q32.astype(np.float64) != q)
        w = fm.required_w(q, emax)
        lo, hi = fm.intervals(form, e, q32)
        s64 = e.astype(np.float64) @ q
        assert np.all(lo - w <= s64) and np.all(s64 <= hi + w)
        T = np.sort(lo)[-K]
        top = np.lexsort((np.arange(N), -s64))[:K]
        keep = fm.survivors(hi, T, w)
        assert np.all(keep[top]), "a row of the fp64 top k is no survivor"
        # the widening changes next to nothing: 2w is far below either form's radius
        assert np.count_nonzero(keep) - np.count_nonzero(hi >= T) <= 2
        assert 2 * w < 1e-3 * np.median(hi - lo)
        shares.append(float(np.max(np.abs(s64 - e.astype(np.float64) @ q32.astype(np.float64))) / w))
    print(f"form {form} D={dim}: random queries reach {min(shares):.2f} .. {max(shares):.2f} of w = {w:.3g}")
    assert max(shares) < 1.0


@pytest.mark.parametrize("dim", pm.SERVED_DIMS)
def test_pressing_input_uses_the_widening(dim):
    """q_i = q^_i +- 0.49 ulp32 and the row e* || fl32(q - q^) with ||e*|| = Emax: |(q - q^).e*| >= 0.9 delta Emax,
    and the exact products of q and q^ with e* differ by at least 0.9 of w -- so a w that loses delta, or an Emax
    below the row's norm, no longer covers this row."""
    e, rng = _corpus(dim, 77 + dim)
    q32 = fm.q32_of(_planted(e, rng))
    q = fm.pressing_query(q32, rng)
    emax0 = fm.emax_of(e)
    star = fm.pressing_row(q, emax0)
    e[N - 1] = star
    emax = fm.emax_of(e)
    assert abs(np.linalg.norm(star.astype(np.float64)) / emax0 - 1.0) < 1e-6 and emax < emax0 * (1 + 1e-6)
    delta, w = fm.delta_of(q), fm.required_w(q, emax)
    gap = abs(fm.exact_dot(q, star) - fm.exact_dot(q32, star))
    print(f"D={dim}: delta {delta:.3g}, w {w:.3g}, |(q - q^).e*| = {gap / (delta * emax):.4f} delta Emax = {gap / w:.4f} w")
    assert gap >= 0.9 * delta * emax and 0.9 * w <= gap <= w
    for form in (1, 2):
        lo, hi = fm.intervals(form, e[N - 64:], q32)
        s = fm.exact_dot(q, star)
        assert lo[-1] - w <= s <= hi[-1] + w


def test_edge_queries():
    rng = np.random.default_rng(3)
    e = rng.standard_normal((64, 256), dtype=np.float32)
    emax = fm.emax_of(e)
    q = rng.standard_normal(256)
    big = q.copy()
    big[7] = 1e300  # outside fp32's range: q^ is infinite, w too, every row survives
    assert np.isinf(fm.q32_of(big)[7]) and not math.isfinite(fm.required_w(big, emax))
    assert np.all(fm.survivors(np.array([1.0, -np.inf, np.inf]), 5.0, fm.required_w(big, emax)))
    assert fm.survivors(np.array([np.nan, 1.0]), -np.inf, math.inf).tolist() == [False, True]
    tiny = np.full(256, 1e-60)  # q^ = 0: delta = ||q||
    assert not np.any(fm.q32_of(tiny)) and fm.delta_of(tiny) == pytest.approx(16e-60)
    assert 0 < fm.required_w(tiny, emax) < 1e-55
    bad = e.copy()
    bad[3, 5] = np.nan
    bad[4, 5] = np.inf
    bad[5] *= np.float32(2.0 ** 70)  # past the cap: an infinite radius, not Emax
    assert fm.emax_of(bad) == fm.emax_of(np.delete(e, [3, 4, 5], axis=0))
    assert fm.emax_of(np.full((2, 4), np.nan, np.float32)) == 0.0


def test_new_entry_points_are_declared_exported_and_bound():
    from anrag import _native as nat
    from anrag.index import Index, ShardGroup

    header = open(os.path.join(REPO, "include", "anrag.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = nat.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared in include/anrag.h"
        assert name in nat.EXPORTS and hasattr(lib, name), f"{name} not exported / bound"
    assert nat._SIGNATURES["anrag_dense_f64_prefilter_stats"] == nat._SIGNATURES["anrag_dense_prefilter_stats"]
    assert nat._SIGNATURES["anrag_set_dense_f64_prefilter"] == nat._SIGNATURES["anrag_set_dense_f64_scan"]
    for method in ("set_dense_f64_prefilter", "dense_f64_prefilter_stats", "debug_prefilter_f64"):
        assert callable(getattr(Index, method, None)), f"Index.{method} missing"
    assert not hasattr(ShardGroup, "hybrid_search_f64")  # a group inherits the route through its shards' dense_search_f64
