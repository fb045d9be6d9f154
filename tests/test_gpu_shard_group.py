"""GPU: a shard group (one corpus over several `anrag_index` objects in one process) against the SINGLE index loaded
with the same operands -- ids equal, counts equal, score bits equal as integers.  Shards on device 0 (the same device
several times is a supported configuration); the distinct-device cases arm themselves where two devices exist."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, TOP = 25, 10
W = (5.0, 1.0, 40.0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def make_corpus(n, d, seed, vocab=400, n_sources=7):
    """Dense rows, a BM25 corpus over the same n documents (CSR, documents ascending inside a term) and source ids."""
    rng = np.random.default_rng(seed)
    E = rng.standard_normal((n, d), dtype=np.float32)
    E /= np.linalg.norm(E, axis=1, keepdims=True)
    lens = rng.integers(4, 30, size=n)
    doc_of = np.repeat(np.arange(n, dtype=np.int64), lens)
    term_of = np.minimum((vocab * rng.random(doc_of.size) ** 2.5).astype(np.int64), vocab - 1)  # skewed: a few frequent terms
    pair, tf = np.unique(term_of * n + doc_of, return_counts=True)
    post_term, post_doc = pair // n, (pair % n).astype(np.int32)
    indptr = np.zeros(vocab + 1, np.int64)
    np.cumsum(np.bincount(post_term, minlength=vocab), out=indptr[1:])
    df = np.diff(indptr)
    idf = np.log((n - df + 0.5) / (df + 0.5))
    idf = np.where(idf < 0, 0.05 * idf[idf > 0].mean(), idf)
    src = rng.integers(0, n_sources, size=n).astype(np.uint16)
    return dict(n=n, d=d, E=E, indptr=indptr, post_doc=post_doc, post_tf=tf.astype(np.int32), idf=idf.astype(np.float64),
                doc_len=lens.astype(np.int32), avgdl=float(lens.mean()), src=src, vocab=vocab, n_sources=n_sources)


def load(ix, c, dense=True, bm25=True, bm25_doc=None, src=True):
    if dense:
        ix.dense_load(c["E"], source_id=c["src"] if src else None)
    if bm25:
        ix.bm25_load(c["indptr"], c["post_doc"], c["post_tf"], c["idf"], c["doc_len"], c["avgdl"], 1.7, 0.83,
                     source_id=c["src"] if src else None, doc_id=bm25_doc)
    return ix


def make_queries(c, nq, seed):
    rng = np.random.default_rng(seed)
    Q = c["E"][rng.integers(0, c["n"], size=nq)] + 0.3 * rng.standard_normal((nq, c["d"])).astype(np.float32)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    terms = [rng.integers(0, c["vocab"], size=rng.integers(1, 9)).astype(np.int32) for _ in range(nq)]
    return Q, terms


def assert_same(got, want, what):
    ids_g, sc_g = got
    ids_w, sc_w = want
    assert ids_g.tolist() == ids_w.tolist(), what
    assert np.array_equal(_bits(sc_g), _bits(sc_w)), what


SIZES = [(1003, 256), (9609, 384), (50_000, 768)]


@pytest.fixture(scope="module", params=SIZES, ids=lambda p: f"{p[0]}x{p[1]}")
def sized(request):
    from anrag.index import Index

    n, d = request.param
    c = make_corpus(n, d, seed=n)
    single = load(Index(0), c)
    yield c, single
    single.close()


@pytest.mark.parametrize("S", [1, 2, 3, 4, 8])
def test_hybrid_equals_single_index(sized, S):
    """1. 64 hybrid queries, k = 25, top 10: plain, without tokens, w_bm25 = 0, a source filter, a filter that empties one
    whole shard, a filter that keeps fewer than k rows in total."""
    from anrag.index import ShardGroup, group_bounds

    c, single = sized
    n = c["n"]
    Q, terms = make_queries(c, 64, seed=S)
    with ShardGroup([0] * S) as g:
        load(g, c)
        info = g.info()
        assert info["n_shards"] == S
        assert info["dense_row_lo"] == group_bounds(n, S) and info["bm25_doc_lo"] == group_bounds(n, S)
        some = np.zeros(c["n_sources"], np.uint8)
        some[[1, 3, 4]] = 1
        for i in range(64):
            t = terms[i]
            wb, allow = W[1], None
            if i % 8 == 3:
                t = np.zeros(0, np.int32)            # no tokens: the dense list is the answer
            elif i % 8 == 5:
                wb = 0.0                             # BM25 switched off by its weight
            elif i % 8 == 6:
                allow = some
            want = single.hybrid_search(Q[i], t, K, W[0], wb, W[2], TOP, allow, allow)
            got = g.hybrid_search(Q[i], t, K, W[0], wb, W[2], TOP, allow, allow)
            assert len(want[0]) == TOP and want[0].min() >= 0  # the comparison is not between two empty answers
            assert_same(got, want, (S, i))
    # filters by block: source id = a function of the row, so that a filter can empty exactly one shard / keep < k rows
    lo = group_bounds(n, max(S, 2))
    src2 = np.zeros(n, np.uint16)
    src2[lo[1]:] = 1                                  # source 0 = the first block
    src2[n - 7:] = 2                                  # source 2 = the last 7 rows
    c2 = dict(c, src=src2)
    from anrag.index import Index

    with Index(0) as s2, ShardGroup([0] * S) as g2:
        load(s2, c2)
        load(g2, c2)
        for allow in (np.array([0, 1, 1], np.uint8), np.array([0, 0, 1], np.uint8), np.array([1, 0, 0], np.uint8)):
            for i in range(6):
                want = s2.hybrid_search(Q[i], terms[i], K, W[0], W[1], W[2], TOP, allow, allow)
                got = g2.hybrid_search(Q[i], terms[i], K, W[0], W[1], W[2], TOP, allow, allow)
                assert_same(got, want, (S, allow.tolist(), i))
        want = s2.dense_search(Q[:4], K, np.array([0, 0, 1], np.uint8))
        got = g2.dense_search(Q[:4], K, np.array([0, 0, 1], np.uint8))
        assert want[2].tolist() == [7] * 4 == got[2].tolist()
        assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))


def _tie_world(seed=20261):
    """Dense rows duplicated across every shard boundary; BM25 doc ids a REVERSED permutation of the rows; queries of one
    rare term, so that the BM25 top k is cut inside the run of zero scores."""
    n, d = 4000, 256
    c = make_corpus(n, d, seed, vocab=3000)
    from anrag.index import group_bounds

    for S in (2, 3, 4, 8):
        for b in group_bounds(n, S)[1:-1]:
            c["E"][b] = c["E"][b - 1]                 # equal dense scores on both sides of the cut
    doc = (n - 1 - np.arange(n)).astype(np.int64)    # document j is chunk n-1-j: ids DEscend with rows
    df = np.diff(c["indptr"])
    rare = np.nonzero((df >= 1) & (df <= 6))[0]
    rng = np.random.default_rng(seed)
    terms = [np.array([t], np.int32) for t in rng.choice(rare, size=32, replace=False)]
    Q = np.stack([c["E"][b] for b in group_bounds(n, 8)[1:-1]] * 5)[:32].astype(np.float32)
    return c, doc, Q, terms


def test_tie_case_shard_order_is_not_doc_order():
    """2. What tells the group's tail from a doc-id merge.  On the CPU first: the oracle's per-shard BM25 lists merged by
    (score desc, doc id asc) and by (score desc, shard, position) differ for at least half of the queries -- a condition
    on the inputs.  Then group == single index for all of them."""
    from oracle import ref_bm25, ref_search
    from anrag.index import Index, ShardGroup, group_bounds

    c, doc, Q, terms = _tie_world()
    n = c["n"]
    for S in (2, 4, 8):
        lo = group_bounds(n, S)
        differ = 0
        for t in terms:
            s = ref_bm25.csr_get_scores(c["indptr"], c["post_doc"], c["post_tf"], c["idf"], c["doc_len"], c["avgdl"], 1.7,
                                        0.83, [int(x) for x in t])
            per_shard = []
            for i in range(S):
                rows = ref_search.canonical_topk(s[lo[i]:lo[i + 1]], K) + lo[i]
                per_shard.append([(float(s[r]), int(doc[r]), i, p) for p, r in enumerate(rows)])
            flat = [e for l in per_shard for e in l]
            by_doc = [e[1] for e in sorted(flat, key=lambda e: (-e[0], e[1]))[:K]]
            by_shard = [e[1] for e in sorted(flat, key=lambda e: (-e[0], e[2], e[3]))[:K]]
            whole = [int(doc[r]) for r in ref_search.canonical_topk(s, K)]
            assert by_shard == whole                  # shard order IS (score desc, global row asc)
            differ += by_doc != by_shard
        assert differ * 2 >= len(terms), f"S={S}: the inputs do not separate the two merges ({differ}/{len(terms)})"
    with Index(0) as single:
        load(single, c, bm25_doc=doc, src=False)
        for S in (2, 3, 4, 8):
            with ShardGroup([0] * S) as g:
                load(g, c, bm25_doc=doc, src=False)
                for i, t in enumerate(terms):
                    want = single.hybrid_search(Q[i], t, K, W[0], W[1], W[2], TOP)
                    got = g.hybrid_search(Q[i], t, K, W[0], W[1], W[2], TOP)
                    assert len(want[0]) == TOP
                    assert_same(got, want, (S, i))
                    wd, ws, wc = single.bm25_search(t, K)
                    assert wc == K and ws[K - 1] == 0.0  # the list is cut inside the run of zero scores
                    gd, gs, gc = g.bm25_search(t, K)
                    assert gc == wc and gd.tolist() == wd.tolist() and np.array_equal(_bits(gs), _bits(ws)), (S, i)
                    wd, ws, wc = single.dense_search(Q[i], K)
                    gd, gs, gc = g.dense_search(Q[i], K)
                    assert np.array_equal(gd, wd) and np.array_equal(_bits(gs), _bits(ws)), (S, i)


@pytest.mark.parametrize("S", [2, 4])
def test_single_leg_entries_and_cold_routes(S):
    """3. Dense-only and BM25-only, k in {1, 10, 64}; cold routes k = 300 and the fp64 query; a NaN row in the last
    shard ranks first and is reported as +inf."""
    from anrag.index import Index, ShardGroup

    c = make_corpus(9609, 384, seed=3)
    c["E"][9600, 5] = np.nan
    c["src"][9600] = 0
    Q, terms = make_queries(c, 6, seed=33)
    Q = np.nan_to_num(Q)
    allow = np.array([1, 0, 1, 1, 0, 1, 1], np.uint8)
    with Index(0) as single, ShardGroup([0] * S) as g:
        load(single, c)
        load(g, c)
        for k in (1, 10, 64, 300):
            for a in (None, allow):
                wd, ws, wc = single.dense_search(Q, k, a)
                gd, gs, gc = g.dense_search(Q, k, a)
                assert gc.tolist() == wc.tolist() and np.array_equal(gd, wd) and np.array_equal(_bits(gs), _bits(ws)), (k, a)
                if k <= 64:
                    assert gd[0, 0] == 9600 and np.isposinf(gs[0, 0])
                for t in (terms[0], terms[1], np.zeros(0, np.int32)):
                    wd, ws, wc = single.bm25_search(t, k, a)
                    gd, gs, gc = g.bm25_search(t, k, a)
                    assert gc == wc and gd[:gc].tolist() == wd[:wc].tolist(), (k, a)
                    assert np.array_equal(_bits(gs[:gc]), _bits(ws[:wc])), (k, a)
        for k in (10, 300):
            wd, ws, wc = single.dense_search_f64(Q[1].astype(np.float64), k, allow)
            gd, gs, gc = g.dense_search_f64(Q[1].astype(np.float64), k, allow)
            assert gc == wc and gd[:gc].tolist() == wd[:wc].tolist() and np.array_equal(_bits(gs[:gc]), _bits(ws[:wc]))


def test_batch_equals_single_calls():
    """4. 200 queries in one call (more than the exchange groups in flight and more than the 32 pipeline slots,
    term-less queries among them) == the single calls row by row; the same burst twice with no sync in between."""
    from anrag.index import Index, ShardGroup

    c = make_corpus(9609, 384, seed=4)
    Q, terms = make_queries(c, 200, seed=44)
    for i in range(0, 200, 7):
        terms[i] = np.zeros(0, np.int32)
    with Index(0) as single, ShardGroup([0, 0, 0]) as g:
        load(single, c)
        load(g, c)
        ids, sc, cnt = g.hybrid_search_batch(Q, terms, K, *W, TOP)
        ids2, sc2, cnt2 = g.hybrid_search_batch(Q, terms, K, *W, TOP)
        assert np.array_equal(ids, ids2) and np.array_equal(_bits(sc), _bits(sc2)) and np.array_equal(cnt, cnt2)
        for i in range(200):
            want = single.hybrid_search(Q[i], terms[i], K, *W, TOP)
            assert cnt[i] == len(want[0])
            assert_same((ids[i, :cnt[i]], sc[i, :cnt[i]]), want, i)
            assert np.all(ids[i, cnt[i]:] == -1) and np.all(np.isneginf(sc[i, cnt[i]:]))
            if i % 25 == 0:
                assert_same(g.hybrid_search(Q[i], terms[i], K, *W, TOP), want, i)


def test_prefilter_modes_same_bits():
    """5. Modes 2 and 1 on the group (768-d): the bits of mode 0; every shard answered through its prefilter."""
    from anrag.index import ShardGroup

    c = make_corpus(20_000, 768, seed=5)
    Q, terms = make_queries(c, 16, seed=55)
    with ShardGroup([0, 0, 0, 0]) as g:
        load(g, c)
        g.set_dense_prefilter(0)
        base = g.hybrid_search_batch(Q, terms, K, *W, TOP)
        base_d = g.dense_search(Q[:8], K)
        for mode in (2, 1):
            g.set_dense_prefilter(mode)
            got = g.hybrid_search_batch(Q, terms, K, *W, TOP)
            assert np.array_equal(got[0], base[0]) and np.array_equal(_bits(got[1]), _bits(base[1])), mode
            got_d = g.dense_search(Q[:8], K)
            assert np.array_equal(got_d[0], base_d[0]) and np.array_equal(_bits(got_d[1]), _bits(base_d[1])), mode
            for i in range(4):
                assert g.shard_prefilter_stats(i)[0] >= 24, (mode, i)


def test_steady_state_allocates_nothing():
    """6. `anrag_debug_alloc_calls` does not move across 200 single and 200 batched group queries after warm-up."""
    from anrag import _native as nat
    from anrag.index import ShardGroup

    def calls():
        n = C.c_int64(0)
        nat.check(nat.load_library().anrag_debug_alloc_calls(C.byref(n)))
        return n.value

    c = make_corpus(9609, 384, seed=6)
    Q, terms = make_queries(c, 200, seed=66)
    with ShardGroup([0, 0, 0, 0]) as g:
        load(g, c)
        g.hybrid_search_batch(Q, terms, K, *W, TOP)
        g.hybrid_search(Q[0], terms[0], K, *W, TOP)
        g.dense_search(Q[0], K)
        g.bm25_search(terms[0], K)
        before = calls()
        for i in range(200):
            g.hybrid_search(Q[i], terms[i], K, *W, TOP)
        g.hybrid_search_batch(Q, terms, K, *W, TOP)
        g.dense_search(Q[:40], K)
        g.bm25_search(terms[3], K)
        assert calls() == before


def test_unsupported_is_raised_not_swallowed(monkeypatch):
    """7. What a group does not serve: ANRAG_ERR_UNSUPPORTED, raised through the reference-shaped classes."""
    import pandas as pd
    from anrag import _native as nat
    from anrag.bm25_index import Bm25Index
    from anrag.database_manager import Bm25Proxy, DenseHandle
    from anrag.index import ShardGroup, rank_batch
    from anrag.search_engine import SearchEngine

    monkeypatch.setenv("ANRAG_DEVICES", "0,0")
    E = np.eye(8, dtype=np.float32)
    df = pd.DataFrame({"id": [f"c{i}" for i in range(8)], "source": ["CG1"] * 8, "embedding": list(E)})
    h = DenseHandle(E, df["source"].tolist()).bind(df)
    assert isinstance(h.index, ShardGroup)
    proxy = Bm25Proxy(Bm25Index([["a", "b"], ["b", "c"], ["c", "d"], ["d"]]), ["s"] * 4)
    assert isinstance(proxy.index, ShardGroup)
    for call in (lambda: proxy.get_scores(["a"]), lambda: h.index.dense_scores(E[0]),
                 lambda: rank_batch([dict(index=h.index, weight=1.0, queries=E[:1])], 1, 4, 60.0, 4)):
        with pytest.raises(nat.AnragError) as e:
            call()
        assert e.value.code == nat.ERR_UNSUPPORTED
    se = SearchEngine(None, None)
    assert len(se.similarity_search_with_embedding(E[2], df, similarity_k=3)) == 3  # served ...

    def refuse(*a, **k):
        raise nat.AnragError(nat.ERR_UNSUPPORTED, "not served by a shard group")

    monkeypatch.setattr(ShardGroup, "dense_search", refuse)
    with pytest.raises(nat.AnragError):  # ... and a route that is not there is not "log and return empty"
        se.similarity_search_with_embedding(E[2], df, similarity_k=3)


@pytest.fixture()
def e2e_world(tmp_path, monkeypatch):
    import pickle
    import sqlite3

    from helpers import load_golden
    from oracle.make_golden import Document, synth_dense
    from oracle.ref_bm25 import BM25Okapi
    from anrag.config import Config, InfoSource

    def _write_db(path, chunks, e):
        conn = sqlite3.connect(path)
        conn.execute("CREATE TABLE chunks (id TEXT PRIMARY KEY, content TEXT NOT NULL, source TEXT NOT NULL,"
                     " embedding BLOB NOT NULL, created_at TIMESTAMP DEFAULT CURRENT_TIMESTAMP, url TEXT)")
        for c, v in zip(chunks, e):
            conn.execute("INSERT INTO chunks (id, content, source, embedding, url) VALUES (?,?,?,?,?)",
                         (c["id"], " ".join(c["tokens"]) or "-", c["source"], np.asarray(v, np.float32).tobytes(), None))
        conn.commit()
        conn.close()

    monkeypatch.setenv("ANRAG_DEVICES", "0,0,0")
    g = load_golden("ref_end_to_end.json")
    co = g["corpus"]
    chunks = co["chunks"]
    e1 = synth_dense(co["n"], co["d"], co["e1_seed"])
    e2 = synth_dense(co["n"], co["d"], co["e2_seed"])
    db1, db2, pkl = str(tmp_path / "m1.db"), str(tmp_path / "m2.db"), str(tmp_path / "bm25.pkl")
    _write_db(db1, chunks, e1)
    _write_db(db2, chunks, e2)
    kept = [c for c in chunks if c["tokens"]]
    bm25 = BM25Okapi([c["tokens"] for c in kept], k1=1.7, b=0.83, epsilon=0.05)
    sections = [Document(" ".join(c["tokens"]), {"id": c["id"], "source": c["source"]}) for c in kept]
    with open(pkl, "wb") as f:
        pickle.dump({"bm25": bm25, "sections": sections, "section_ids": [c["id"] for c in kept], "config": {}}, f)
    cfg = Config()
    sc = cfg.SOURCE_CONFIGS[InfoSource.NICE]
    saved = dict(vars(sc))
    sc.db_path = sc.voyage_db_path = db1
    sc.openai_db_path = db2
    sc.voyage_3_5_db_path = sc.qwen_db_path = sc.local_db_path = None
    sc.bm25_path = pkl
    yield g, cfg, e1, e2
    for k, v in saved.items():
        setattr(sc, k, v)


@pytest.mark.parametrize("fused", [False, True])
def test_reference_end_to_end_on_a_group(e2e_world, fused):
    """8. The reference's own `retrieve_documents` outputs through DatabaseManager + RetrievalEvaluationSystem on three
    shards (a fresh manager: the handles are built under ANRAG_DEVICES), single calls and the list entry point; every
    case is asserted, as the single-index test asserts them; UNSUPPORTED stays fatal in the list entry point."""
    import json

    from oracle.make_golden import synth_query
    from anrag import _native as nat
    from anrag.database_manager import ATTR
    from anrag.index import ShardGroup
    from anrag.query_rag_retrieval import RetrievalEvaluationSystem

    g, cfg, e1, e2 = e2e_world
    system = RetrievalEvaluationSystem(cfg, fused=fused)
    frames = [df for d in system.embeddings_data.values() for df in d.values() if df is not None and not df.empty]
    assert frames and all(isinstance(df.attrs[ATTR].index, ShardGroup) for df in frames)
    groups = {}
    for c in g["cases"]:
        q = {"voyage-3-large": synth_query(e1, c["q1_seed"], c["target"]),
             "text-embedding-3-large": synth_query(e2, c["q2_seed"], c["target"])}
        out = system.retrieve_documents(query_embeddings=q, query_tokens=c["tokens"], use_reranker=False, **c["cfg"])
        assert out == c["ids"], (fused, c["cfg"], c["tokens"])
        groups.setdefault(json.dumps(c["cfg"], sort_keys=True), []).append((c, q))
    for key, cases in groups.items():
        params = json.loads(key)
        asks = [{"query_embeddings": q, "query_tokens": c["tokens"]} for c, q in cases]
        out = system.retrieve_documents_batch(asks * 3, use_reranker=False, **params)  # lists of 16 and more among them
        assert out == [c["ids"] for c, _ in cases] * 3, params
        assert system.rank_of_expected_batch(asks, ["x"] * len(asks), use_reranker=False, **params) is None
    if fused:
        def refuse(*a, **k):
            raise nat.AnragError(nat.ERR_UNSUPPORTED, "not served by a shard group")

        key, cases = next((k, v) for k, v in groups.items() if json.loads(k).get("use_hybrid_search")
                          and json.loads(k).get("similarity_k", 25) <= 64 and all(c["tokens"] for c, _ in v))
        asks = [{"query_embeddings": {"voyage-3-large": q["voyage-3-large"]}, "query_tokens": c["tokens"]} for c, q in cases]
        orig = ShardGroup.hybrid_search_batch
        ShardGroup.hybrid_search_batch = refuse
        try:
            with pytest.raises(nat.AnragError):
                system.retrieve_documents_batch(asks, use_reranker=False, **json.loads(key))
        finally:
            ShardGroup.hybrid_search_batch = orig


def test_full_size_1m_x768():
    """9. 1M x 768 hybrid, 8 queries, S in {2, 4, 8} on device 0 == the single index."""
    import torch
    from anrag import synth
    from anrag.index import Index, ShardGroup

    dev = torch.device("cuda", 0)
    n, d = 1_000_000, 768
    E = synth.dense_corpus(n, d, 1234, dev)
    Qd, _ = synth.dense_queries(E, 8, 4321)
    post = synth.bm25_postings(n, 200_000, 777, dev)
    idf = synth.bm25_idf(post["df"].cpu().numpy(), n)
    terms = synth.bm25_queries(post, 8, 19)
    torch.cuda.synchronize()
    c = dict(E=E.cpu().numpy(), indptr=np.asarray(post["indptr"]), post_doc=post["post_doc"].cpu().numpy(),
             post_tf=post["post_tf"].cpu().numpy(), idf=idf, doc_len=np.asarray(post["doc_len"]),
             avgdl=post["total_len"] / n, src=None)
    Q = Qd.cpu().numpy()
    del E, post
    torch.cuda.empty_cache()
    with Index(0) as single:
        load(single, c, src=False)
        want = [single.hybrid_search(Q[i], terms[i], K, *W, TOP) for i in range(8)]
    for S in (2, 4, 8):
        with ShardGroup([0] * S) as g:
            load(g, c, src=False)
            ids, sc, cnt = g.hybrid_search_batch(Q, terms, K, *W, TOP)
            assert cnt.tolist() == [TOP] * 8 and g.info()["dense_rows"] == n and g.info()["bm25_docs"] == n
            for i in range(8):
                assert_same((ids[i, :cnt[i]], sc[i, :cnt[i]]), want[i], (S, i))
            assert_same(g.hybrid_search(Q[3], terms[3], K, *W, TOP), want[3], S)


@pytest.mark.parametrize("devices", [[0, 1], [1, 0]])
@pytest.mark.parametrize("size", [(9609, 384), (50_000, 768)])
def test_distinct_devices(devices, size):
    """10. Two GPUs: the home tail reads the other device's slab over the fabric."""
    from anrag import _native as nat
    from anrag.index import Index, ShardGroup

    if nat.device_count() < 2:
        pytest.skip("needs two devices")
    c = make_corpus(*size, seed=10)
    Q, terms = make_queries(c, 40, seed=100)
    with Index(0) as single, ShardGroup(devices) as g:
        load(single, c)
        load(g, c)
        ids, sc, cnt = g.hybrid_search_batch(Q, terms, K, *W, TOP)
        for i in range(40):
            want = single.hybrid_search(Q[i], terms[i], K, *W, TOP)
            assert_same((ids[i, :cnt[i]], sc[i, :cnt[i]]), want, i)
            if i < 8:
                assert_same(g.hybrid_search(Q[i], terms[i], K, *W, TOP), want, i)
