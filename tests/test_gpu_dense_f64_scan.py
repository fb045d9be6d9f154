"""GPU: K1D, the list-keeping scan of one float64 query (`anrag_dense_search_f64`, k <= 64, dim % 4 == 0 up to 3,072),
against the route it replaces -- the fp64 score array + sort, still there behind `set_dense_f64_scan(False)` -- in ids,
counts and score BITS; against a CPU model of the specified summation order; and against numpy's fp64 dot product."""
import numpy as np
import pytest

from helpers import assert_ranking_matches, load_golden
from test_dense_f64_order_cpu import model_score

pytestmark = pytest.mark.gpu

DIMS = [8, 100, 256, 384, 512, 768, 1024, 1536, 2048, 3072]
ROWS = [1, 3, 63, 64, 65, 1000, 9609, 20011]  # fewer rows than waves, waves without rows, a partial last batch, several
KS = [1, 10, 64]                              # batches per wave on the full grid


@pytest.fixture(scope="module")
def Index():
    from anrag.index import Index

    return Index


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def _both_routes(idx, q, k, allow=None):
    """(scan answer, sort answer), each checked against the route counters."""
    s0, t0 = idx.dense_f64_stats()
    idx.set_dense_f64_scan(True)
    a = idx.dense_search_f64(q, k, allow)
    s1, t1 = idx.dense_f64_stats()
    assert (s1 - s0, t1 - t0) == (1, 0), "the list scan did not answer"
    idx.set_dense_f64_scan(False)
    b = idx.dense_search_f64(q, k, allow)
    s2, t2 = idx.dense_f64_stats()
    assert (s2 - s1, t2 - t1) == (0, 1), "the score array + sort did not answer"
    idx.set_dense_f64_scan(True)
    return a, b


def _assert_same(a, b, what):
    (doc_a, score_a, cnt_a), (doc_b, score_b, cnt_b) = a, b
    assert cnt_a == cnt_b, what
    assert doc_a.tolist() == doc_b.tolist(), what
    assert _bits(score_a) == _bits(score_b), what


@pytest.fixture(scope="module")
def corpus():
    """One matrix per dimension (its first N rows are the corpus of N rows), made once."""
    made = {}

    def get(d):
        if d not in made:
            n = 2000 if d == 3072 else max(ROWS)
            rng = np.random.default_rng(1000 + d)
            e = rng.standard_normal((n, d), dtype=np.float32)
            e /= np.linalg.norm(e, axis=1, keepdims=True)
            made.clear()  # one at a time: the 2,048-d matrix is 164 MB
            made[d] = e
        return made[d]

    return get


@pytest.mark.parametrize("d", DIMS)
def test_scan_equals_sort_route_bit_for_bit(Index, corpus, d):
    e = corpus(d)
    rng = np.random.default_rng(d)
    allow = np.array([1, 0, 1, 1, 0, 0, 1], dtype=np.uint8)
    for n in ROWS:
        if n > e.shape[0]:
            continue
        sid = ((np.arange(n) * 5 + 3) % 7).astype(np.uint16)
        q = rng.standard_normal(d)
        q /= np.linalg.norm(q)
        with Index(0) as idx:
            idx.dense_load(e[:n], source_id=sid)
            for k in KS:
                for flt in (None, allow):
                    a, b = _both_routes(idx, q, k, flt)
                    _assert_same(a, b, f"d={d} n={n} k={k} filter={flt is not None}")
                    allowed = n if flt is None else int(allow[sid].sum())
                    assert a[2] == min(k, allowed)
                    assert np.all(a[0][a[2]:] == -1) and np.all(a[1][a[2]:] == -np.inf)
                    assert not np.any(a[1][:a[2]] == 0.0)  # (signed zeros are kept out of this comparison)


@pytest.mark.parametrize("d", DIMS)
def test_four_rows_have_the_models_bits(Index, d):
    """The summation order of the kernels is the one the text states (tests/test_dense_f64_order_cpu.py), on both routes."""
    rng = np.random.default_rng(50 + d)
    e = rng.standard_normal((4, d), dtype=np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    q = rng.standard_normal(d)
    q /= np.linalg.norm(q)
    with Index(0) as idx:
        idx.dense_load(e)
        a, b = _both_routes(idx, q, 4)
        _assert_same(a, b, f"d={d}")
        doc, score, cnt = a
        assert cnt == 4 and sorted(doc.tolist()) == [0, 1, 2, 3]
        for r, s in zip(doc.tolist(), score.tolist()):
            assert _bits([s]) == _bits([model_score(e[r], q)]), (d, r)


def test_order_and_edges(Index):
    rng = np.random.default_rng(9)
    n, d = 3000, 384
    e = rng.standard_normal((n, d), dtype=np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    q = rng.standard_normal(d)
    q /= np.linalg.norm(q)
    assert np.any(q.astype(np.float32).astype(np.float64) != q)  # a float64 query that is not representable in fp32
    # duplicated rows: equal bits, row-ascending
    winner = (q / np.linalg.norm(q)).astype(np.float32)
    dups = [2999, 17, 1024, 1500]
    e[dups] = winner
    with Index(0) as idx:
        idx.dense_load(e)
        a, b = _both_routes(idx, q, 10)
        _assert_same(a, b, "duplicates")
        assert a[0][:4].tolist() == sorted(dups) and len(set(_bits(a[1][:4]))) == 1
        # ... and the fp32 entry point rounds the query: not these bits
        s32 = idx.dense_search(q.astype(np.float32), 10)[1][0]
        assert np.max(np.abs(s32 - a[1])) < 1e-4 and np.any(s32.astype(np.float64) != a[1])
        # N < k
        doc, score, cnt = idx.dense_search_f64(q, 64)
        assert cnt == 64
    with Index(0) as idx:
        idx.dense_load(e[:40])
        a, b = _both_routes(idx, q, 64)
        _assert_same(a, b, "N < k")
        assert a[2] == 40 and np.all(a[0][40:] == -1) and np.all(a[1][40:] == -np.inf)
        want = e[:40].astype(np.float64) @ q
        order = np.lexsort((np.arange(40), -want))
        assert_ranking_matches(order, want[order], a[0][:40], a[1][:40], 1e-12, want, "N < k")
    # NaN and +-inf elements: a NaN dot product ranks first and is reported +inf, like a +inf one (ties row-ascending)
    f = e.copy()
    f[2500, 5] = np.nan                       # NaN score
    f[700, :] = np.nan
    f[1200, 9] = np.inf if q[9] > 0 else -np.inf   # +inf score
    f[1300, 9] = np.inf if q[9] > 0 else -np.inf
    f[1300, 10] = -np.inf if q[10] > 0 else np.inf  # inf - inf in one lane's chain: NaN
    f[40, 9] = -np.inf if q[9] > 0 else np.inf     # -inf score: reported as padding by the sort route, and by the scan
    with Index(0) as idx:
        idx.dense_load(f)
        for k in (3, 10, 64):
            a, b = _both_routes(idx, q, k)
            _assert_same(a, b, f"non-finite k={k}")
            first = [700, 1200, 1300, 2500]
            assert a[0][:min(k, 4)].tolist() == first[:k] and np.all(a[1][:min(k, 4)] == np.inf)
            assert 40 not in a[0].tolist()
            if k > 4:
                assert a[0][4:8].tolist() == sorted(dups)
    # fewer allowed rows than k: count < k, -1 / -inf padding
    sid = np.zeros(n, np.uint16)
    sid[[5, 900, 2998]] = 3
    allow = np.zeros(4, np.uint8)
    allow[3] = 1
    with Index(0) as idx:
        idx.dense_load(e, source_id=sid)
        for k in (1, 10, 64):
            a, b = _both_routes(idx, q, k, allow)
            _assert_same(a, b, f"three allowed rows, k={k}")
            m = min(k, 3)
            assert a[2] == m and set(a[0][:m].tolist()) <= {5, 900, 2998}
            assert np.all(a[0][m:] == -1) and np.all(a[1][m:] == -np.inf)
        none = np.zeros(4, np.uint8)
        a, b = _both_routes(idx, q, 10, none)
        _assert_same(a, b, "nothing allowed")
        assert a[2] == 0


def test_unserved_requests_keep_the_sort_route(Index):
    """k = 65 and a dimension that is no multiple of 4 are answered by the score array + sort, as before."""
    rng = np.random.default_rng(3)
    for d, k in ((768, 65), (6, 10), (3076, 10)):
        e = rng.standard_normal((500, d), dtype=np.float32)
        e /= np.linalg.norm(e, axis=1, keepdims=True)
        q = rng.standard_normal(d)
        q /= np.linalg.norm(q)
        with Index(0) as idx:
            idx.dense_load(e)
            assert idx.dense_f64_scan_serves() == (d == 768)
            s0, t0 = idx.dense_f64_stats()
            doc, score, cnt = idx.dense_search_f64(q, k)
            assert idx.dense_f64_stats() == (s0, t0 + 1), (d, k)
            want = e.astype(np.float64) @ q
            order = np.lexsort((np.arange(500), -want))[:k]
            assert_ranking_matches(order, want[order], doc[:cnt], score[:cnt], 1e-12, want, f"d={d} k={k}")


def test_scan_scores_like_numpy(Index, corpus):
    """`E.astype(float64) @ q` at 1e-12, as test_fp64_query_scores_like_numpy asks of the route this one replaces (sums of
    <= 3,072 products of unit vectors: the gamma_D bound of tests/test_dense_f64_order_cpu.py is 7e-13 at most)."""
    from oracle import ref_search

    for d, n in ((768, 20011), (100, 501), (3072, 2000)):
        e = corpus(d)[:n]
        rng = np.random.default_rng(77 + d)
        sid = (np.arange(n) % 5).astype(np.uint16)
        allow = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
        with Index(0) as idx:
            idx.dense_load(e, source_id=sid)
            for t in range(2):
                q = rng.standard_normal(d)
                q /= np.linalg.norm(q)
                want = np.dot(q.reshape(1, -1), e.T).flatten()
                assert want.dtype == np.float64
                for k, flt in ((10, None), (25, allow), (64, None)):
                    s0, _ = idx.dense_f64_stats()
                    doc, score, cnt = idx.dense_search_f64(q, k, flt)
                    assert idx.dense_f64_stats()[0] == s0 + 1
                    order = ref_search.canonical_topk(want, k, None if flt is None else flt.astype(bool)[sid])
                    assert cnt == len(order)
                    assert_ranking_matches(order, want[order], doc[:cnt], score[:cnt], 1e-12, want, f"fp64 d={d} k={k}")


def test_golden_float64_cases(Index):
    """The reference's own float64-query answers (tests/golden/ref_dense.json) with k <= 64, through the list scan."""
    from oracle import ref_search
    from oracle.make_golden import synth_dense, synth_query, synth_sources

    cases = [c for c in load_golden("ref_dense.json") if "rows" in c and c.get("qdtype") == "float64" and c["k"] <= 64]
    by_corpus = {}
    for c in cases:
        by_corpus.setdefault((c["n"], c["d"], c["corpus_seed"], tuple(c.get("dups", ()))), []).append(c)
    checked = 0
    for (n, d, seed, dups), group in by_corpus.items():
        e = synth_dense(n, d, seed)
        for j in dups:
            e[j] = e[group[0]["dup_of"]]
        sources = synth_sources(n, group[0]["source_seed"])
        table = {}
        sid = np.array([table.setdefault(s, len(table)) for s in sources], dtype=np.uint16)
        distinct = list(table)
        with Index(0) as idx:
            idx.dense_load(e, source_id=sid)
            served = idx.dense_f64_scan_serves()
            for c in group:
                q = e[c["dup_of"]].copy() if dups else synth_query(e, c["query_seed"], c["query_row"])
                allow = ref_search.dense_filter_mask(distinct, c["filter"]).astype(np.uint8) if c["filter"] else None
                q64 = q.astype(np.float64)
                s0, t0 = idx.dense_f64_stats()
                d64, s64, m64 = idx.dense_search_f64(q64, c["k"], allow)
                assert idx.dense_f64_stats() == ((s0 + 1, t0) if served else (s0, t0 + 1))
                assert m64 == len(c["rows"])
                assert_ranking_matches(c["rows"], c["sims"], d64[:m64], s64[:m64], 1e-12, ref_search.dense_scores(q64, e),
                                       f"golden fp64 n={n} d={d} k={c['k']} f={c['filter']}")
                checked += served
    assert checked >= 1


def test_lists_whose_best_score_is_negative_are_kept(Index):
    """Dot products are signed: a wave's list may hold negative scores only (BM25's lists, the other users of the fp64
    merge, never do).  Rows are multiples of the query, so every score is known: waves with negative rows only, a wave
    with both signs, a corpus of negative scores only -- against the sort route and the known order."""
    rng = np.random.default_rng(12)
    d = 768
    q = rng.standard_normal(d)
    q /= np.linalg.norm(q)
    for scale in ([-1, -2, -5, -6, -7, -8, -9, -10, 3, 4], [-3, -1, -2], [-1], [-4, 2, -1, -3, -2, -6, -5]):
        e = (np.asarray(scale, np.float64)[:, None] * q[None, :]).astype(np.float32)
        want = np.argsort(-np.asarray(scale, np.float64), kind="stable")
        with Index(0) as idx:
            idx.dense_load(e)
            for k in (1, 10, 64):
                a, b = _both_routes(idx, q, k)
                _assert_same(a, b, f"scale={scale} k={k}")
                m = min(k, len(scale))
                assert a[2] == m and a[0][:m].tolist() == want[:m].tolist()
