"""GPU: the shadow prefilter for float64 queries (dense_prefilter_f64.hip, DESIGN.md §3 "K1FD") -- `dense_search_f64` and
`hybrid_search_f64` while a prefilter form is built -- against K1D (`set_dense_f64_prefilter(False)`) and the score array
+ sort (`set_dense_f64_scan(False)`) in ids, counts and score BITS; its widening w, Emax and the survivor rule row by row
against tests/prefilter_f64_model.py; its pruning against the fp32 prefilter's; and its steady state without allocations."""
import ctypes as C

import numpy as np
import pytest

import prefilter_f64_model as fm

pytestmark = pytest.mark.gpu

SHAPES = [(256, 20_000), (512, 8_000), (768, 6_001), (1024, 5_000), (1536, 3_000), (2048, 3_001)]
FORMS = [1, 2]
KS = [1, 10, 25, 64]
ALLOW = np.array([1, 0, 1, 1, 0, 0, 1], dtype=np.uint8)


@pytest.fixture(scope="module")
def Index():
    from anrag.index import Index

    return Index


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def _unit(n, d, seed):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((n, d), dtype=np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    return e, rng


def _planted(e, rng):
    q = e[int(rng.integers(0, e.shape[0]))].astype(np.float64) + 0.05 * rng.standard_normal(e.shape[1])
    return q / np.linalg.norm(q)


def _assert_same(a, b, what):
    (doc_a, score_a, cnt_a), (doc_b, score_b, cnt_b) = a, b
    assert cnt_a == cnt_b, what
    assert doc_a.tolist() == doc_b.tolist(), what
    assert _bits(score_a) == _bits(score_b), what


def _routes(idx, q, k, allow=None, sort=True, what=""):
    """The prefilter's answer, held to K1D's and (sort) the score array + sort's, each checked against the counters."""
    s0, t0 = idx.dense_f64_stats()
    p0, v0 = idx.dense_f64_prefilter_stats()
    f0 = idx.dense_prefilter_stats()
    idx.set_dense_f64_prefilter(True)
    a = idx.dense_search_f64(q, k, allow)
    p1, v1 = idx.dense_f64_prefilter_stats()
    assert idx.dense_f64_stats() == (s0 + 1, t0), "a list route did not answer"
    assert p1 == p0 + 1 and a[2] <= v1 - v0 <= idx.n_rows, "the fp64 prefilter did not answer"
    assert idx.dense_prefilter_stats() == f0, "the fp32 prefilter's counters moved"
    idx.set_dense_f64_prefilter(False)
    b = idx.dense_search_f64(q, k, allow)
    assert idx.dense_f64_stats() == (s0 + 2, t0) and idx.dense_f64_prefilter_stats() == (p1, v1), "K1D did not answer"
    _assert_same(a, b, f"{what}: prefilter vs K1D")
    if sort:
        idx.set_dense_f64_scan(False)
        c = idx.dense_search_f64(q, k, allow)
        assert idx.dense_f64_stats() == (s0 + 2, t0 + 1) and idx.dense_f64_prefilter_stats() == (p1, v1)
        idx.set_dense_f64_scan(True)
        _assert_same(a, c, f"{what}: prefilter vs sort")
    idx.set_dense_f64_prefilter(True)
    return a, v1 - v0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("d,n", SHAPES)
def test_prefilter_equals_k1d_and_sort_bit_for_bit(Index, form, d, n):
    e, rng = _unit(n, d, 100 * d + form)
    sid = ((np.arange(n) * 5 + 3) % 7).astype(np.uint16)
    with Index(0) as idx:
        idx.dense_load(e, source_id=sid)
        idx.set_dense_prefilter(form)
        assert idx.debug_prefilter_read(data=False)["form"] == form
        for k in KS:
            q = _planted(e, rng)
            assert np.any(q.astype(np.float32).astype(np.float64) != q)
            for flt in (None, ALLOW):
                a, surv = _routes(idx, q, k, flt, what=f"form={form} d={d} n={n} k={k} filter={flt is not None}")
                allowed = n if flt is None else int(ALLOW[sid].sum())
                assert a[2] == min(k, allowed) and surv <= allowed
                assert np.all(a[0][a[2]:] == -1) and np.all(a[1][a[2]:] == -np.inf)
        # prefilter mode 0 keeps the built form's block but turns the route off: K1D answers
        idx.set_dense_prefilter(0)
        p0 = idx.dense_f64_prefilter_stats()
        idx.dense_search_f64(q, 10)
        assert idx.dense_f64_prefilter_stats() == p0


@pytest.mark.parametrize("form", FORMS)
def test_edges(Index, form):
    d = 256
    e, rng = _unit(3000, d, 9 + form)
    q = _planted(e, rng)

    def run(rows, query, ks, sid=None, allow=None, sort=True, what=""):
        with Index(0) as idx:
            idx.dense_load(rows, source_id=sid)
            idx.set_dense_prefilter(form)
            return [_routes(idx, query, k, allow, sort=sort, what=f"{what} k={k}") for k in ks]

    # n < k, and n = 1
    (a, _), = run(e[:40], q, [64], what="n < k")
    assert a[2] == 40 and np.all(a[0][40:] == -1)
    for (a, _), k in zip(run(e[:1], q, [1, 10, 64], what="n = 1"), [1, 10, 64]):
        assert a[2] == 1 and a[0][0] == 0
    # all rows identical: ties go by row
    same = np.repeat(e[:1], 777, axis=0)
    for (a, _), k in zip(run(same, q, [1, 10, 64], what="identical rows"), [1, 10, 64]):
        assert a[0].tolist() == list(range(k)) and len(set(_bits(a[1]))) == 1
    # every score negative: rows are negative multiples of the query
    scale = -(1.0 + np.arange(300) % 17).astype(np.float64)
    neg = (scale[:, None] * q[None, :]).astype(np.float32)
    for (a, _), k in zip(run(neg, q, [1, 10, 64], what="negative scores"), [1, 10, 64]):
        assert a[2] == k and np.all(a[1] < 0) and a[0][0] == 0
    # NaN and +-inf rows (K1D's own edge cases), and rows beyond fp16's range (an infinite radius in form 1)
    f = e.copy()
    f[2500, 5] = np.nan
    f[700, :] = np.nan
    f[1200, 9] = np.inf if q[9] > 0 else -np.inf
    f[1300, 9] = np.inf if q[9] > 0 else -np.inf
    f[1300, 10] = -np.inf if q[10] > 0 else np.inf
    f[40, 9] = -np.inf if q[9] > 0 else np.inf  # a -inf score: padding on every route
    f[50] *= np.float32(1e6)                    # elements of ~6e4 .. 3e5: past 65504
    f[51] *= np.float32(-1e6)
    f[52] *= np.float32(2.0 ** 70)              # a norm past the 2^60 cap
    for (a, _), k in zip(run(f, q, [3, 10, 64], what="non-finite rows"), [3, 10, 64]):
        first = [700, 1200, 1300, 2500]
        assert a[0][:min(k, 4)].tolist() == first[:k] and np.all(a[1][:min(k, 4)] == np.inf)
        assert 40 not in a[0].tolist()
    # a filter that allows fewer than k rows, and none
    sid = np.zeros(3000, np.uint16)
    sid[[5, 900, 2998]] = 3
    allow = np.zeros(4, np.uint8)
    allow[3] = 1
    for (a, surv), k in zip(run(e, q, [1, 10, 64], sid, allow, what="three allowed rows"), [1, 10, 64]):
        m = min(k, 3)
        assert a[2] == m and set(a[0][:m].tolist()) <= {5, 900, 2998} and surv <= 3
        assert np.all(a[0][m:] == -1) and np.all(a[1][m:] == -np.inf)
    (a, surv), = run(e, q, [10], sid, np.zeros(4, np.uint8), what="nothing allowed")
    assert a[2] == 0 and surv == 0
    # a component outside fp32's range: q^ is infinite, the whole corpus is rescored, the answer is K1D's
    big = q.copy()
    big[7] = 1e300
    (a, surv), = run(e, big, [10], what="1e300")
    assert surv == 3000 and a[2] == 10 and np.all(np.isfinite(a[1]))
    # q^ = 0: the scan sees a zero query, the widening is delta = ||q||
    (a, surv), = run(e, np.full(d, 1e-60), [10], what="1e-60")
    assert a[2] == 10 and np.all(np.abs(a[1]) < 1e-57)
    # zero scores of either sign of the products: K1D's order (the sort route ranks a -0.0 behind +0.0: anrag.h)
    z = np.zeros(d)
    z[0], z[3] = 1.0, -0.0
    rows = rng.standard_normal((500, d)).astype(np.float32)
    rows[:, 0] = np.where(np.arange(500) % 2 == 0, 0.0, -0.0)
    rows[7, 0], rows[8, 0], rows[9, 0] = 1e-30, -1e-30, 1e-30
    for (a, _), k in zip(run(rows, z, [1, 10, 64], sort=False, what="signed zeros"), [1, 10, 64]):
        assert a[0][:min(k, 2)].tolist() == [7, 9][:k]
        if k > 2:
            assert np.all(a[1][2:] == 0.0) and a[0][2:].tolist() == [r for r in range(500) if r not in (7, 8, 9)][:k - 2]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("d", [256, 768])
def test_widening_row_by_row(Index, form, d):
    """q^, Emax and w as the product route computes them, every row's hi and T from the shadow scan of q^, every row's
    s64 from the score array + sort with k = N.  Measured on an MI355X (share of w the pressed row uses): 1.00 at both
    dimensions and forms; a w of 0 and an Emax over the first half of the rows each fail here (w below the model's
    required value; Emax below the model's) while passing the bit tests."""
    n, k = 4099, 10
    e, rng = _unit(n, d, 31 * d + form)
    e[n // 2:] *= rng.uniform(0.5, 1.5, (n - n // 2, 1)).astype(np.float32)  # the largest norm lies in the second half
    q_random = _planted(e, rng)
    q_press = fm.pressing_query(fm.q32_of(_planted(e, rng)), rng)
    e[n - 1] = fm.pressing_row(q_press, fm.emax_of(e))
    model_emax = fm.emax_of(e)
    assert np.argmax(np.linalg.norm(e.astype(np.float64), axis=1)) >= n // 2
    with Index(0) as idx:
        idx.dense_load(e)
        idx.set_dense_prefilter(form)
        for name, q0 in (("random", q_random), ("pressing", q_press)):
            for q in (q0, -q0):
                q32, w, emax = idx.debug_prefilter_f64(q)
                assert q32.view(np.uint32).tolist() == q.astype(np.float32).view(np.uint32).tolist()
                assert model_emax <= emax <= model_emax * (1 + 2.0 ** -20), (emax, model_emax)
                need = fm.required_w(q, emax)
                print(f"form {form} D={d} {name}: Emax {emax:.9g} (model {model_emax:.9g}), w {w:.17g} (required {need:.17g})")
                assert need <= w <= need * (1 + 2.0 ** -40), (w, need)
                hi, T = idx.debug_prefilter_bounds(q32, k)
                hi, T = hi[0].astype(np.float64), float(T[0])
                doc, score, cnt = idx.dense_search_f64(q, n)
                assert cnt == n
                s64 = np.empty(n)
                s64[doc] = score
                assert np.all(hi + w >= s64), "a row's fp64 score lies above hi + w"
                kth = np.sort(s64)[-k]
                assert T - w <= kth, (T, w, kth)
                top = np.lexsort((np.arange(n), -s64))[:k]
                assert np.all(fm.survivors(hi, T, w)[top])
                if name == "pressing":
                    share = abs(s64[n - 1] - fm.exact_dot(q32, e[n - 1])) / w
                    print(f"  the pressed row uses {share:.4f} of w")
                    assert share >= 0.85
                # ... and the product route on these inputs
                _routes(idx, q, k, what=f"{name} form={form} d={d}")


@pytest.mark.parametrize("form", FORMS)
def test_fused_hybrid_call(Index, form):
    from anrag.bm25_index import Bm25Index

    n, d = 6001, 768
    e, rng = _unit(n, d, 5 + form)
    vocab = 600
    p = 1.0 / np.arange(1, vocab + 1) ** 1.07
    p /= p.sum()
    docs = [[f"t{j}" for j in rng.choice(vocab, size=int(rng.integers(5, 50)), p=p)] for _ in range(n)]
    bi = Bm25Index(docs, k1=1.7, b=0.83, epsilon=0.05)
    dense_src = (np.arange(n) % 5).astype(np.uint16)
    bm25_src = (np.arange(n) % 3).astype(np.uint16)
    ad = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    ab = np.array([0, 1, 1], dtype=np.uint8)
    with Index(0) as idx:
        idx.dense_load(e, source_id=dense_src)
        idx.bm25_load(bi.indptr, bi.post_doc, bi.post_tf, bi.idf, bi.doc_len, bi.avgdl, bi.k1, bi.b, source_id=bm25_src)
        idx.set_dense_prefilter(form)
        for i in range(3):
            row = int(rng.integers(0, n))
            q = e[row].astype(np.float64) + 0.05 * rng.standard_normal(d)
            q /= np.linalg.norm(q)
            terms = bi.term_ids([str(t) for t in rng.choice(docs[row], size=4)] + ["not-in-vocab"])
            for k, top_n in ((25, 10), (64, 128), (1, 2)):
                for fa, fb in ((None, None), (ad, None), (None, ab), (ad, ab)):
                    s0, t0 = idx.dense_f64_stats()
                    p0, _ = idx.dense_f64_prefilter_stats()
                    idx.set_dense_f64_prefilter(True)
                    got = idx.hybrid_search_f64(q, terms, k, 5.0, 1.0, 40.0, top_n, fa, fb)
                    assert idx.dense_f64_stats() == (s0 + 1, t0) and idx.dense_f64_prefilter_stats()[0] == p0 + 1
                    idx.set_dense_f64_prefilter(False)
                    want = idx.hybrid_search_f64(q, terms, k, 5.0, 1.0, 40.0, top_n, fa, fb)
                    assert idx.dense_f64_stats() == (s0 + 2, t0) and idx.dense_f64_prefilter_stats()[0] == p0 + 1
                    idx.set_dense_f64_prefilter(True)
                    assert got[0].tolist() == want[0].tolist() and _bits(got[1]) == _bits(want[1]), (form, k, i)
                    assert 1 <= len(got[0]) <= top_n


def test_shard_group_inherits_the_route(Index):
    from anrag import _native as nat
    from anrag.index import ShardGroup

    n, d = 6001, 768
    e, rng = _unit(n, d, 44)
    sid = ((np.arange(n) * 5 + 3) % 7).astype(np.uint16)
    lib = nat.load_library()
    with Index(0) as single, ShardGroup([0, 0]) as g:
        single.dense_load(e, source_id=sid)
        single.set_dense_prefilter(0)  # the plain index: K1D
        g.dense_load(e, source_id=sid)
        g.set_dense_prefilter(2)
        asked = 0
        for k in (1, 10, 64):
            q = _planted(e, rng)
            for flt in (None, ALLOW):
                _assert_same(g.dense_search_f64(q, k, flt), single.dense_search_f64(q, k, flt), (k, flt is not None))
                asked += 1
        assert single.dense_f64_prefilter_stats() == (0, 0)
        for i in range(2):
            pq, ps = C.c_int64(0), C.c_int64(0)
            nat.check(lib.anrag_dense_f64_prefilter_stats(g.shard(i), C.byref(pq), C.byref(ps)))
            assert pq.value == asked and ps.value >= asked


def test_pruning_matches_the_fp32_prefilter(Index):
    """The survivors of a float64 query are the rows with hi >= T - 2w, those of the same query rounded to fp32 the rows
    with hi >= T, from the same scan.  2w (5e-8 .. 1.3e-7 for unit vectors) is below 1e-5 of the int8 radius (median
    1.4e-2), so the rule admits the rows whose hi lies in a band of that relative width under T: at most 1 % more, plus
    2 rows per query for the discreteness of small counts (the CPU model shows equality)."""
    n, d, k, nq = 100_000, 256, 25, 32
    e, rng = _unit(n, d, 2024)
    qs = [_planted(e, rng) for _ in range(nq)]
    with Index(0) as idx:
        idx.dense_load(e)
        idx.set_dense_prefilter(2)
        f0 = idx.dense_prefilter_stats()
        for q in qs:
            idx.dense_search(q.astype(np.float32), k)
        f1 = idx.dense_prefilter_stats()
        assert f1[0] - f0[0] == nq, "the fp32 queries did not go through the prefilter"
        p0 = idx.dense_f64_prefilter_stats()
        for q in qs:
            idx.dense_search_f64(q, k)
        p1 = idx.dense_f64_prefilter_stats()
        assert p1[0] - p0[0] == nq and idx.dense_prefilter_stats() == f1
        mean32, mean64 = (f1[1] - f0[1]) / nq, (p1[1] - p0[1]) / nq
        print(f"survivors per query at {n} x {d}, int8, k={k}: fp32 {mean32:.1f}, float64 {mean64:.1f}")
        assert mean64 >= k and mean64 <= mean32 * 1.01 + 2


def test_steady_state_allocates_nothing(Index):
    from anrag import _native as nat

    lib = nat.load_library()

    def calls():
        c = C.c_int64(0)
        nat.check(lib.anrag_debug_alloc_calls(C.byref(c)))
        return c.value

    e, rng = _unit(6001, 768, 8)
    with Index(0) as idx:
        idx.dense_load(e)
        idx.set_dense_prefilter(2)
        q = _planted(e, rng)
        idx.dense_search_f64(q, 10)
        idx.debug_prefilter_f64(q)
        before = calls()
        for i in range(50):
            idx.dense_search_f64(_planted(e, rng), 10 if i % 2 else 64)
        idx.debug_prefilter_f64(q)
        assert calls() == before
        assert idx.dense_f64_prefilter_stats()[0] == 51
