"""GPU: lists of float64 queries through `rank_batch` -- leg kind 2 (`queries_f64`), fp64 score tiles (K1TD,
dense_tile_f64.hip) -- against `Index.dense_search_f64` per query on the score-array route in ids, counts and score BITS;
against the CPU model of the specified summation order; tile kernel against per-query passes; planted rows; the select
path past the list cap; fusion with fp32 dense and BM25 legs; and `retrieve_documents_batch` as a drop-in for the loop."""
import os

import numpy as np
import pytest

from test_dense_f64_order_cpu import model_score
from test_gpu_hybrid_f64 import e2e  # noqa: F401  (the reference-shaped world: a fixture)

pytestmark = pytest.mark.gpu

DIMS = [4, 8, 100, 256, 260, 384, 768, 1024, 2048, 3072]
ROWS = [1, 63, 64, 65, 1000, 2113]
LISTS = [1, 2, 15, 16, 17, 33]
TILED = {4, 8, 100, 256, 260, 384, 768, 1024, 2048}  # dimensions that must have a tile kernel (3,072: per-query passes)
ALLOW = np.array([1, 0, 1, 1, 0, 0, 1], dtype=np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _corpus(n, d, seed):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((n, d), dtype=np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    return e


def _queries(nq, d, seed):
    """fl32 + 1e-9 noise, in float64: a cast to fp32 changes the score bits."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nq, d), dtype=np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q.astype(np.float64) + 1e-9 * rng.standard_normal((nq, d))


def _sort_route(idx, q, k, allow=None):
    """`dense_search_f64` on the score-array route (every k, every dimension)."""
    idx.set_dense_f64_scan(False)
    try:
        return idx.dense_search_f64(q, k, allow)
    finally:
        idx.set_dense_f64_scan(True)


def _assert_rows(ids, sc, cnt, refs, what):
    for i, (doc, score, c) in enumerate(refs):
        assert cnt[i] == c, (what, i, int(cnt[i]), c)
        assert ids[i, :c].tolist() == doc[:c].tolist(), (what, i)
        assert np.array_equal(_bits(sc[i, :c]), _bits(score[:c])), (what, i)
        assert np.all(ids[i, c:] == -1) and np.all(sc[i, c:] == -np.inf), (what, i)
        assert not np.any(sc[i, :c] == 0.0)  # (signed zeros are kept out of these comparisons)


@pytest.mark.parametrize("d", DIMS)
def test_tile_bits_equal_the_per_query_route(d):
    from anrag.index import Index, rank_batch

    e_all = _corpus(max(ROWS), d, 3000 + d)
    q_all = _queries(130, d, 4000 + d)
    differs_from_fp32 = False
    for n in ROWS:
        e = e_all[:n]
        sid = ((np.arange(n) * 5 + 3) % 7).astype(np.uint16)
        lists = LISTS + ([130] if n == 65 else [])
        with Index(0) as idx:
            idx.dense_load(e, source_id=sid)
            for flt in (None, ALLOW):
                refs = [_sort_route(idx, q_all[i], n, flt) for i in range(max(lists))]  # once per (n, filter)
                allowed = n if flt is None else int(ALLOW[sid].sum())
                assert all(r[2] == allowed for r in refs)
                for nq in lists:
                    t0, p0 = idx.rank_f64_tile_stats()
                    ids, sc, cnt = rank_batch([dict(index=idx, weight=1.0, allow=flt, queries_f64=q_all[:nq])], nq, n, 60.0, n,
                                              want_scores=True)
                    t1, p1 = idx.rank_f64_tile_stats()
                    assert (t1 - t0, p1 - p0) == ((nq, 0) if d in TILED else (0, nq)), (d, n, nq)
                    _assert_rows(ids, sc, cnt, refs[:nq], f"d={d} n={n} nq={nq} filter={flt is not None}")
            if n == 1000:
                # the kind-0 leg answers the queries rounded to fp32: this leg is not that leg
                _, sc32, _ = rank_batch([dict(index=idx, weight=1.0, queries=q_all[:17])], 17, n, 60.0, n, want_scores=True)
                _, sc64, _ = rank_batch([dict(index=idx, weight=1.0, queries_f64=q_all[:17])], 17, n, 60.0, n, want_scores=True)
                differs_from_fp32 = bool(np.any(_bits(sc32) != _bits(sc64)))
            if n == 65:
                # a handful of (row, query) pairs against the stated summation order
                ids, sc, cnt = rank_batch([dict(index=idx, weight=1.0, queries_f64=q_all[:17])], 17, n, 60.0, n, want_scores=True)
                for row, qi in ((0, 0), (64, 16), (31, 7), (17, 15)):
                    at = ids[qi].tolist().index(row)
                    assert _bits([sc[qi, at]])[0] == _bits([model_score(e[row], q_all[qi])])[0], (d, row, qi)
    assert differs_from_fp32, "no score differs in bits from the fp32 leg's: the comparison shows nothing"


@pytest.mark.parametrize("d", [100, 384, 768, 1024, 2048, 3072])
def test_tile_kernel_against_per_query_passes(d):
    from anrag.index import Index, rank_batch

    n, nq = 1000, 17
    e, q = _corpus(n, d, 5000 + d), _queries(nq, d, 6000 + d)
    sid = ((np.arange(n) * 3 + 1) % 7).astype(np.uint16)
    with Index(0) as idx:
        idx.dense_load(e, source_id=sid)
        for flt in (None, ALLOW):
            legs = [dict(index=idx, weight=1.0, allow=flt, queries_f64=q)]
            t0, p0 = idx.rank_f64_tile_stats()
            a = rank_batch(legs, nq, n, 60.0, n, want_scores=True)
            t1, p1 = idx.rank_f64_tile_stats()
            os.environ["ANRAG_RANK_SCAN_TILES"] = "1"
            try:
                b = rank_batch(legs, nq, n, 60.0, n, want_scores=True)
            finally:
                del os.environ["ANRAG_RANK_SCAN_TILES"]
            t2, p2 = idx.rank_f64_tile_stats()
            assert (t1 - t0, p1 - p0) == ((nq, 0) if d in TILED else (0, nq)), d
            assert (t2 - t1, p2 - p1) == (0, nq), d
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(_bits(a[1]), _bits(b[1]))
            assert int(a[2][0]) == (n if flt is None else int(ALLOW[sid].sum()))


def test_planted_rows():
    from anrag.index import Index, rank_batch

    n, d, nq = 300, 384, 18
    rng = np.random.default_rng(77)
    e = np.abs(_corpus(n, d, 78))  # every component positive
    e[200] = e[17]                 # duplicate rows: equal scores, ties by row
    e[41, 5] = np.nan              # NaN ranks first, as +inf
    e[99, 300] = -np.inf           # against a positive query: a dot product of -inf, not a candidate
    q = np.abs(_queries(nq, d, 79)) + 1e-3
    q[1::2] *= -1.0                # odd queries: every finite score negative
    with Index(0) as idx:
        idx.dense_load(e)
        ids, sc, cnt = rank_batch([dict(index=idx, weight=1.0, queries_f64=q)], nq, n, 60.0, n, want_scores=True)
        assert idx.rank_f64_tile_stats()[0] == nq
        refs = [_sort_route(idx, q[i], n) for i in range(nq)]
        for i in range(nq):
            row = ids[i, :cnt[i]].tolist()
            assert row[0] == 41 and sc[i, 0] == np.inf
            assert row.index(200) == row.index(17) + 1 and sc[i, row.index(17)] == sc[i, row.index(200)]
            assert np.all(sc[i, 1:cnt[i]] <= sc[i, :cnt[i] - 1])
            if i % 2 == 0:  # positive query: row 99 scores -inf
                assert cnt[i] == n - 1 and 99 not in row
                assert np.all(sc[i, 1:cnt[i]] > 0)
            else:           # negative query: row 99 scores +inf like the NaN row (rows 41 and 99 tie: row ascending)
                assert cnt[i] == n and row[:2] == [41, 99] and sc[i, 1] == np.inf
                assert np.all(sc[i, 2:cnt[i]] < 0)
                # the order of negative keys, against numpy
                full = e[row[2:]].astype(np.float64) @ q[i]
                assert np.all(np.diff(full) <= 1e-12)
            doc, score, c = refs[i]
            assert c == cnt[i] and doc[:c].tolist() == row
            assert np.array_equal(_bits(score[:c]), _bits(sc[i, :c]))


def test_select_path_past_the_list_cap():
    from anrag.index import Index, rank_batch, rank_wide_stats, set_rank_wide

    n, d, k, nq = 20011, 8, 12000, 3
    e, q = _corpus(n, d, 91), _queries(nq, d, 92)
    with Index(0) as idx:
        idx.dense_load(e)
        refs = [_sort_route(idx, q[i], k) for i in range(nq)]
        legs = [dict(index=idx, weight=1.0, queries_f64=q)]
        try:
            for mode in (0, 1):
                set_rank_wide(mode)
                w0 = rank_wide_stats()[0]
                ids, sc, cnt = rank_batch(legs, nq, k, 60.0, k, want_scores=True)
                assert rank_wide_stats()[0] - w0 == (nq if mode else 0)
                _assert_rows(ids, sc, cnt, refs, f"wide={mode}")
                assert np.all(cnt == k)
        finally:
            set_rank_wide(-1)


@pytest.fixture(scope="module")
def fusion_world():
    from anrag.bm25_index import Bm25Index
    from anrag.index import Index

    n, d, vocab = 2000, 384, 600
    rng = np.random.default_rng(123)
    e = _corpus(n, d, 124)
    p = 1.0 / np.arange(1, vocab + 1) ** 1.07
    p /= p.sum()
    docs = [[f"t{j}" for j in rng.choice(vocab, size=int(rng.integers(5, 50)), p=p)] for _ in range(n)]
    bi = Bm25Index(docs, k1=1.7, b=0.83, epsilon=0.05)
    nq = 6
    rows = rng.integers(0, n, nq)
    q = e[rows].astype(np.float64) + 0.05 * rng.standard_normal((nq, d))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    terms = [bi.term_ids([str(t) for t in rng.choice(docs[int(r)], size=4)] + ["not-in-vocab"]) for r in rows]
    with Index(0) as idx:
        idx.dense_load(e)
        idx.bm25_load(bi.indptr, bi.post_doc, bi.post_tf, bi.idf, bi.doc_len, bi.avgdl, bi.k1, bi.b)
        yield dict(idx=idx, q=q, q32=np.ascontiguousarray(q[:, ::-1], dtype=np.float32), terms=terms, n=n, nq=nq)


@pytest.mark.parametrize("k", [25, 300, 2000])
@pytest.mark.parametrize("three", [False, True])
def test_fusion_with_fp32_and_bm25_legs(fusion_world, k, three):
    from anrag.index import rank_batch

    w = fusion_world
    idx, q, q32, terms, n, nq = w["idx"], w["q"], w["q32"], w["terms"], w["n"], w["nq"]
    wrrf_k, top_n = 40.0, min(2 * k, n)
    legs = [dict(index=idx, weight=5.0, queries_f64=q), dict(index=idx, weight=1.0, term_lists=terms)]
    weights = [5.0, 1.0]
    if three:
        legs.insert(0, dict(index=idx, weight=2.0, queries=q32))
        weights.insert(0, 2.0)
    ids, sc, cnt = rank_batch(legs, nq, k, wrrf_k, top_n, id_space=n, want_scores=True)
    want = []
    for i in range(nq):
        lists = []
        if three:
            doc, _, c = idx.dense_search(q32[i], k)
            lists.append(doc[0, :c[0]])
        doc, _, c = _sort_route(idx, q[i], k)
        lists.append(doc[:c])
        doc, _, c = idx.bm25_search(terms[i], k)
        lists.append(doc[:c])
        wid, wsc = idx.wrrf(lists, weights, wrrf_k, top_n)
        want.append(wid)
        assert cnt[i] == len(wid) and ids[i, :cnt[i]].tolist() == wid.tolist(), (i, k, three)
        assert np.array_equal(_bits(sc[i, :cnt[i]]), _bits(wsc)), (i, k, three)
        if k <= 64 and not three:
            hid, hsc = idx.hybrid_search_f64(q[i], terms[i], k, 5.0, 1.0, wrrf_k, top_n)[:2]
            m = int(cnt[i])
            assert np.asarray(hid)[:m].tolist() == wid.tolist() and np.array_equal(_bits(np.asarray(hsc)[:m]), _bits(wsc))
    # the rank of an expected document without the lists: its position, -1 for an id the answer does not hold
    expect = np.empty(nq, np.int64)
    for i in range(nq):
        absent = np.setdiff1d(np.arange(n), want[i])
        expect[i] = want[i][(7 * i) % len(want[i])] if i % 2 == 0 or not len(absent) else absent[i]
    none, _, cnt2, ranks = rank_batch(legs, nq, k, wrrf_k, top_n, id_space=n, expect=expect, want_ids=False)
    assert none is None and np.array_equal(cnt2, cnt)
    for i in range(nq):
        pos = np.nonzero(want[i] == expect[i])[0]
        assert ranks[i] == (pos[0] + 1 if len(pos) else -1), (i, k, three)


def test_rank_of_expected_on_one_float64_leg(fusion_world):
    """One leg and no lists wanted: a count instead of a sort (rank_count_kernel over the fp64 tile)."""
    from anrag.index import rank_batch

    w = fusion_world
    idx, q, n, nq = w["idx"], w["q"], w["n"], w["nq"]
    legs = [dict(index=idx, weight=1.0, queries_f64=q)]
    ids, _, cnt = rank_batch(legs, nq, 300, 40.0, 300)
    expect = np.array([ids[i, (11 * i) % 300] if i % 2 == 0 else ids[(i + 1) % nq, 299] for i in range(nq)], dtype=np.int64)
    _, _, cnt2, ranks = rank_batch(legs, nq, 300, 40.0, 300, expect=expect, want_ids=False)
    assert np.array_equal(cnt, cnt2)
    for i in range(nq):
        pos = np.nonzero(ids[i, :cnt[i]] == expect[i])[0]
        assert ranks[i] == (pos[0] + 1 if len(pos) else -1), i


# ------------------------------------------------------------------ the reference-shaped host layer
def _list_requests(chunks, e1, count):
    from oracle.make_golden import synth_query

    rng = np.random.default_rng(57)
    out = []
    for i in range(count):
        target = int(rng.integers(0, len(chunks)))
        q64 = synth_query(e1, 700 + i, target).astype(np.float64) + rng.standard_normal(e1.shape[1]) * 1e-9
        out.append(dict(query_embeddings={"voyage-3-large": q64}, query_tokens=chunks[target]["tokens"][:3] or ["asthma"]))
    return out


def _tiled(system):
    from anrag.database_manager import ATTR

    total = 0
    for d in system.embeddings_data.values():
        for df in d.values():
            if df is not None and not df.empty:
                total += df.attrs[ATTR].index.rank_f64_tile_stats()[0]
    return total


@pytest.mark.parametrize("hybrid", [True, False])
@pytest.mark.parametrize("similarity_k", [25, 300])
def test_retrieve_documents_batch_is_the_loop(e2e, similarity_k, hybrid):  # noqa: F811
    from anrag.query_rag_retrieval import RetrievalEvaluationSystem

    chunks, cfg, e1 = e2e
    system = RetrievalEvaluationSystem(cfg, fused=True)
    queries = _list_requests(chunks, e1, 20)
    for flt in (None, "CG,NG"):
        params = dict(similarity_k=similarity_k, common_sections_n=15, use_hybrid_search=hybrid, wrrf_k=40,
                      model_weights={"voyage-3-large": 5.0, "BM25": 1.0}, filename_type_filter=flt, use_reranker=False)
        want = [system.retrieve_documents(**q, **params) for q in queries]
        t0 = _tiled(system)
        got = system.retrieve_documents_batch(queries, **params)
        assert _tiled(system) - t0 == 20, "the list did not take the fp64 tiles"
        assert got == want and all(len(g) == 15 for g in got)
    # a short small-k list stays one by one; a single query's route does not change
    params["similarity_k"] = 25
    t0 = _tiled(system)
    assert system.retrieve_documents_batch(queries[:5], **params) == [system.retrieve_documents(**q, **params) for q in queries[:5]]
    assert _tiled(system) == t0


def test_a_shard_group_answers_float64_lists_one_by_one(e2e, monkeypatch):  # noqa: F811
    from anrag import _native as nat
    from anrag.database_manager import ATTR
    from anrag.index import ShardGroup, rank_batch_group
    from anrag.query_rag_retrieval import RetrievalEvaluationSystem

    chunks, cfg, e1 = e2e
    queries = _list_requests(chunks, e1, 20)
    params = dict(similarity_k=300, common_sections_n=15, use_hybrid_search=True, wrrf_k=40,
                  model_weights={"voyage-3-large": 5.0, "BM25": 1.0}, use_reranker=False)
    single = RetrievalEvaluationSystem(cfg, fused=True)
    want = single.retrieve_documents_batch(queries, **params)
    monkeypatch.setenv("ANRAG_DEVICES", "0,0")
    grouped = RetrievalEvaluationSystem(cfg, fused=True)
    frames = [df for d in grouped.embeddings_data.values() for df in d.values() if df is not None and not df.empty]
    assert frames and all(isinstance(df.attrs[ATTR].index, ShardGroup) for df in frames)
    assert grouped.retrieve_documents_batch(queries, **params) == want
    # the group entry point rejects the kind
    group = frames[0].attrs[ATTR].index
    q = np.stack([x["query_embeddings"]["voyage-3-large"] for x in queries])
    with pytest.raises(nat.AnragError) as err:
        rank_batch_group([dict(index=group, weight=1.0, queries_f64=q)], len(queries), 300, 40.0, 15)
    assert err.value.code == -1
