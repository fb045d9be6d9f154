"""GPU: the wide form of the ranking select (rank_batch.hip, "K4 wide": one segment cut into slices across the device,
a ticketed pick per digit, compaction and sort) against the narrow form (one workgroup per segment) and the numpy model
of the order (tests/rank_select_model.py), on planted score arrays through `anrag_debug_rank_select`; then the routes
that reach it: `anrag_rank_batch` with the wide form forced, the auto gate at a million scores, and
`RetrievalEvaluationSystem.retrieve_documents` answering one query with ONE `anrag_rank_batch`."""
import os

import numpy as np
import pytest

import rank_select_model as m

pytestmark = pytest.mark.gpu

K_FULL = 12000


@pytest.fixture(scope="module")
def ix():
    from anrag.index import Index

    with Index(0) as i:
        yield i


def _k_of(k, n, dtype):
    return {"cap": m.cap_of(dtype), "n+5": n + 5}.get(k, k)


def _both(ix, case, n, k, parts, seg_k=None, model=True):
    """Both forms over one input: wide == narrow in rows, key bits and counts; (inputs without signed zeros) == model."""
    from anrag.index import debug_rank_select, rank_wide_stats

    keys, ties = case["keys"], case["ties"]
    n_seg = keys.shape[0]
    s0 = rank_wide_stats()
    rn, kn, cn = debug_rank_select(ix, keys, n, k, ties=ties, seg_k=seg_k, form=0)
    s1 = rank_wide_stats()
    rw, kw, cw = debug_rank_select(ix, keys, n, k, ties=ties, seg_k=seg_k, form=1, parts=parts)
    s2 = rank_wide_stats()
    assert s1 == s0, "a narrow call moved the wide counters"
    passes = 9 if keys.dtype == np.float64 else 6
    assert s2 == (s1[0] + n_seg, s1[1] + passes), (s1, s2)
    assert np.array_equal(cn, cw), (cn, cw)
    assert np.array_equal(rn, rw)
    assert np.array_equal(kn.view(np.int64), kw.view(np.int64))
    if model and not case["signed_zeros"]:
        want = m.select_model(keys, n, k, ties, seg_k)
        for s, (rows, sc) in enumerate(want):
            assert cw[s] == len(rows), (s, cw[s], len(rows))
            assert np.array_equal(rw[s, :cw[s]], rows), s
            assert np.array_equal(kw[s, :cw[s]].view(np.int64), sc.view(np.int64)), s
    for s in range(n_seg):  # nothing is written past a segment's count
        assert not rw[s, cw[s]:].any() and not kw[s, cw[s]:].any()
    return rw, kw, cw


SIZES = [(np.float32, n) for n in (16385, 20000, 65537, 100003)] + [(np.float64, n) for n in (13313, 20000, 65537)]


@pytest.mark.parametrize("parts", [0, 1, 2, 7, 64])
@pytest.mark.parametrize("dtype,n", SIZES)
def test_sizes_and_slices(ix, dtype, n, parts):
    """Every size x every slicing (0: the launcher's own; 64 at 16,385 / 13,313 / 20,000 asks for more slices than the
    shortest slice allows -- clamped to 5 / 4 / 5 -- and at 16,385 and 65,537 leaves a last slice of ONE score), three
    segments, the middle one skipped."""
    rng = np.random.default_rng(n + parts)
    case = m.gen_normal(rng, 3, n, dtype, K_FULL)
    _both(ix, case, n, K_FULL, parts, seg_k=np.array([K_FULL, 0, 777], np.int32))


@pytest.mark.parametrize("kind", sorted(m.GENERATORS))
@pytest.mark.parametrize("k", [1, 64, K_FULL, "cap", "n+5"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_inputs_and_k(ix, dtype, k, kind):
    n = 20000
    k = _k_of(k, n, dtype)
    case = m.GENERATORS[kind](np.random.default_rng(11), 1, n, dtype, k)
    m.check_claims(case, n, k)
    _both(ix, case, n, k, 7)


@pytest.mark.parametrize("n_seg", [1, 3, 17])
@pytest.mark.parametrize("dtype,n", [(np.float32, 16385), (np.float64, 13313), (np.float32, 100003)])
def test_segments_with_their_own_k(ix, dtype, n, n_seg):
    """Segments of different kinds side by side (their records, histograms and survivors must not mix), per-segment k
    with zeros in it."""
    rng = np.random.default_rng(n_seg)
    kinds = sorted(m.GENERATORS)
    parts = [m.GENERATORS[kinds[s % len(kinds)]](rng, 1, n, dtype, K_FULL) for s in range(n_seg)]
    case = dict(keys=np.concatenate([p["keys"] for p in parts]), ties=None,
                signed_zeros=any(p["signed_zeros"] for p in parts))
    seg_k = np.array([[K_FULL, 0, 5, 13000, 1][s % 5] for s in range(n_seg)], np.int32)
    if n_seg == 1:
        seg_k[0] = 900
    _both(ix, case, n, K_FULL + 1000, 0 if n_seg == 3 else 2, seg_k=seg_k, model=False)
    for s, p in enumerate(parts):  # the model per segment, where it applies
        if not p["signed_zeros"]:
            from anrag.index import debug_rank_select

            rw, kw, cw = debug_rank_select(ix, p["keys"], n, int(seg_k[s]) or 1, form=1, parts=2)
            (rows, sc), = m.select_model(p["keys"], n, int(seg_k[s]) or 1)
            assert cw[0] == len(rows) and np.array_equal(rw[0, :cw[0]], rows)


@pytest.mark.parametrize("k", [1, 64, K_FULL])
@pytest.mark.parametrize("parts", [2, 7, 64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_equal_pair_across_a_slice_boundary(ix, dtype, parts, k):
    n = 65537
    case = m.gen_planted_boundary(np.random.default_rng(k + parts), 2, n, dtype, k, parts)
    m.check_claims(case, n, k)
    rw, kw, cw = _both(ix, case, n, k, parts)
    b = case["claims"]["boundary"]
    assert np.all(cw == k) and np.all(rw[:, k - 1] == b - 1) and np.all(kw[:, k - 1] == 2.0)
    rw, kw, cw = _both(ix, case, n, k + 1, parts)
    assert np.all(rw[:, k] == b)


@pytest.mark.parametrize("k", [64, K_FULL, "cap"])
@pytest.mark.parametrize("parts", [1, 7])
@pytest.mark.parametrize("n", [13313, 20000, 65537])
def test_tie_form(ix, n, parts, k):
    k = _k_of(k, n, np.float64)
    case = m.gen_tie_form(np.random.default_rng(n), 2, n, np.float64, k)
    m.check_claims(case, n, k)
    _both(ix, case, n, k, parts)


def test_steady_state_allocates_nothing(ix):
    from anrag import _native as nat
    from anrag.index import debug_rank_select
    import ctypes as C

    def allocs():
        v = C.c_int64()
        nat.check(nat.load_library().anrag_debug_alloc_calls(C.byref(v)))
        return v.value

    case = m.gen_normal(np.random.default_rng(1), 3, 65537, np.float32, K_FULL)
    first = debug_rank_select(ix, case["keys"], 65537, K_FULL, form=1)
    a = allocs()
    again = debug_rank_select(ix, case["keys"], 65537, K_FULL, form=1)
    assert allocs() == a
    for x, y in zip(first, again):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------- the routes
@pytest.fixture
def wide_mode():
    from anrag.index import set_rank_wide

    yield set_rank_wide
    set_rank_wide(-1)


@pytest.fixture(scope="module")
def small_world():
    """20,000 x 64 dense rows + 20,000 BM25 documents, document = row: an id space past the fused ranking's LDS form."""
    from anrag.bm25_index import Bm25Index
    from anrag.index import Index

    rng = np.random.default_rng(20)
    n, d, vocab = 20000, 64, 1500
    e = rng.standard_normal((n, d), dtype=np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    e[9001] = e[44]
    p = 1.0 / np.arange(1, vocab + 1) ** 1.07
    p /= p.sum()
    docs = [[f"t{j}" for j in rng.choice(vocab, size=int(rng.integers(3, 30)), p=p)] for _ in range(n)]
    bi = Bm25Index(docs, k1=1.7, b=0.83, epsilon=0.05)
    di, bx = Index(0), Index(0)
    di.dense_load(e)
    bx.bm25_load(bi.indptr, bi.post_doc, bi.post_tf, bi.idf, bi.doc_len, bi.avgdl, bi.k1, bi.b)
    q = e[rng.integers(0, n, 2)] + 0.05 * rng.standard_normal((2, d), dtype=np.float32)
    toks = [[str(t) for t in rng.choice(docs[int(rng.integers(n))], size=4)] for _ in range(2)]
    yield dict(n=n, di=di, bx=bx, bi=bi, q=np.ascontiguousarray(q, np.float32), toks=toks)
    di.close()
    bx.close()


@pytest.mark.parametrize("nq", [1, 2])
def test_rank_batch_forced_wide_equals_narrow(small_world, wide_mode, nq):
    """Dense leg (fp32, 20,000 > 16,384), BM25 leg (fp64, > 13,312) and the fused sums (tie-word form) all through the
    wide select: same ids, fused score bits, counts and expected ranks as with the narrow one, and as the per-query
    entry points' lists fused by the reference's rule."""
    from oracle import ref_search
    from anrag.index import rank_batch, rank_wide_stats

    w = small_world
    term_lists = [w["bi"].term_ids(t) for t in w["toks"]][:nq]
    legs = [dict(index=w["di"], weight=5.0, queries=w["q"][:nq]), dict(index=w["bx"], weight=1.0, term_lists=term_lists)]
    out = {}
    for mode in (0, 1):
        wide_mode(mode)
        s0 = rank_wide_stats()
        ids, sc, cnt = rank_batch(legs, nq, K_FULL, 40, K_FULL, id_space=w["n"], want_scores=True)
        expect = np.array([ids[i, 100 + i] for i in range(nq)], dtype=np.int64)
        _, _, cnt2, ranks = rank_batch(legs, nq, K_FULL, 40, K_FULL, id_space=w["n"], expect=expect)
        s1 = rank_wide_stats()
        # per call: dense, BM25 and fused segments for every query; 6 passes for the fp32 launch, 9 + 9 for the fp64 ones
        assert s1 == ((s0[0] + 2 * 3 * nq, s0[1] + 2 * 24) if mode else s0), (mode, s0, s1)
        assert np.array_equal(cnt, cnt2)
        out[mode] = (ids, sc, cnt, ranks)
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
    ids, sc, cnt, ranks = out[1]
    assert ranks.tolist() == [101 + i for i in range(nq)]
    for i in range(nq):
        l1, _, c1 = w["di"].dense_search(w["q"][i], K_FULL)
        l3, _, c3 = w["bx"].bm25_search(term_lists[i], K_FULL)
        lists = [(l1[0, :c1[0]].tolist(), "a"), (l3[:c3].tolist(), "c")]
        fused = ref_search.weighted_reciprocal_rank_fusion(lists, {"a": 5.0, "c": 1.0}, 40)[:K_FULL]
        assert cnt[i] == len(fused) and ids[i, :cnt[i]].tolist() == [d for d, _ in fused]
        assert sc[i, :cnt[i]].tolist() == [s for _, s in fused]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_auto_at_a_million_scores(ix, wide_mode, dtype):
    """One segment of 1,000,000 scores through the production dispatch in auto: the narrow form's output, by the wide form
    exactly when the committed gate says so."""
    from anrag.index import debug_rank_select, rank_wide_gate, rank_wide_stats

    n = 1_000_000
    wide_mode(-1)
    case = m.gen_bm25_like(np.random.default_rng(3), 1, n, dtype, K_FULL) if dtype == np.float64 else \
        m.gen_normal(np.random.default_rng(3), 1, n, dtype, K_FULL)
    narrow = debug_rank_select(ix, case["keys"], n, K_FULL, form=0)
    s0 = rank_wide_stats()
    auto = debug_rank_select(ix, case["keys"], n, K_FULL, form=-1)
    took = rank_wide_stats()[0] - s0[0]
    assert took == (1 if rank_wide_gate(dtype == np.float64, 1, n) else 0)
    for a, b in zip(narrow, auto):
        assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
    (rows, sc), = m.select_model(case["keys"], n, K_FULL)
    assert auto[2][0] == len(rows) and np.array_equal(auto[0][0, :len(rows)], rows)


# ---------------------------------------------------------------------------------------------- Python: one call per query
def _count_rank_batch(monkeypatch):
    import anrag.index as index_mod

    calls = []
    real = index_mod.rank_batch

    def counted(legs, n_queries, *a, **kw):
        calls.append(n_queries)
        return real(legs, n_queries, *a, **kw)

    monkeypatch.setattr(index_mod, "rank_batch", counted)
    return calls


@pytest.fixture(scope="module")
def golden_world(tmp_path_factory):
    """The corpus of tests/golden/ref_end_to_end.json as the files a user of the reference has: two SQLite `chunks`
    databases and a BM25 pickle."""
    import pickle
    import sqlite3

    from helpers import load_golden
    from oracle.make_golden import Document, synth_dense
    from oracle.ref_bm25 import BM25Okapi
    from anrag.config import Config, InfoSource

    def write_db(path, chunks, e):
        conn = sqlite3.connect(path)
        conn.execute("CREATE TABLE chunks (id TEXT PRIMARY KEY, content TEXT NOT NULL, source TEXT NOT NULL,"
                     " embedding BLOB NOT NULL, created_at TIMESTAMP DEFAULT CURRENT_TIMESTAMP, url TEXT)")
        for c, v in zip(chunks, e):
            conn.execute("INSERT INTO chunks (id, content, source, embedding, url) VALUES (?,?,?,?,?)",
                         (c["id"], " ".join(c["tokens"]) or "-", c["source"], np.asarray(v, np.float32).tobytes(), None))
        conn.commit()
        conn.close()

    g = load_golden("ref_end_to_end.json")
    co = g["corpus"]
    tmp = tmp_path_factory.mktemp("anrag_rank_one")
    e1 = synth_dense(co["n"], co["d"], co["e1_seed"])
    e2 = synth_dense(co["n"], co["d"], co["e2_seed"])
    db1, db2, pkl = str(tmp / "m1.db"), str(tmp / "m2.db"), str(tmp / "bm25.pkl")
    write_db(db1, co["chunks"], e1)
    write_db(db2, co["chunks"], e2)
    kept = [c for c in co["chunks"] if c["tokens"]]
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


def test_golden_requests_one_call_each(golden_world, monkeypatch):
    """The reference's own `retrieve_documents` outputs (tests/golden/ref_end_to_end.json): with RANK_ONE_CALL every
    request that reaches the ids-only route costs exactly one `anrag_rank_batch` of one query and answers as the per-leg
    route and the reference do; a float64 embedding keeps the per-leg route."""
    from oracle.make_golden import synth_query
    from anrag.query_rag_retrieval import RetrievalEvaluationSystem

    g, cfg, e1, e2 = golden_world
    system = RetrievalEvaluationSystem(cfg)
    assert RetrievalEvaluationSystem.RANK_ONE_CALL is True
    calls = _count_rank_batch(monkeypatch)
    routed = 0
    for c in g["cases"]:
        q = {"voyage-3-large": synth_query(e1, c["q1_seed"], c["target"]),
             "text-embedding-3-large": synth_query(e2, c["q2_seed"], c["target"])}
        ask = dict(query_tokens=c["tokens"], use_reranker=False, **c["cfg"])
        system.RANK_ONE_CALL = False
        off = system.retrieve_documents(query_embeddings=q, **ask)
        assert not calls and off == c["ids"]
        system.RANK_ONE_CALL = True
        on = system.retrieve_documents(query_embeddings=q, **ask)
        assert on == off, c["cfg"]
        w = c["cfg"]["model_weights"]
        # one dense model + BM25 at k <= 64 with tokens is answered before the ids-only route (anrag_hybrid_search)
        fused_first = (c["cfg"]["use_hybrid_search"] and c["cfg"]["similarity_k"] <= 64 and w.get("BM25", 0) > 0
                       and sum(1 for k_, v in w.items() if k_ != "BM25" and v > 0) == 1 and c["tokens"])
        assert calls in ([1], []) if fused_first else calls == [1], (c["cfg"], calls)
        routed += len(calls)
        calls.clear()
        q64 = {k_: v.astype(np.float64) for k_, v in q.items()}
        on64 = system.retrieve_documents(query_embeddings=q64, **ask)
        system.RANK_ONE_CALL = False
        assert on64 == system.retrieve_documents(query_embeddings=q64, **ask)
        assert not calls or not any(v > 0 for k_, v in w.items() if k_ != "BM25")  # float64: the per-leg route
        calls.clear()
    assert routed >= 36


def test_full_ranking_request_on_the_standin_one_call(monkeypatch):
    """similarity_k = 12000 over the 9,609-row stand-in corpus (retrieval_eval.py's full-ranking configurations)."""
    import pandas as pd
    from anrag import niceqa
    from anrag.bm25_index import Bm25Index
    from anrag.config import Config, InfoSource, LOCAL_ENCODER_KEY
    from anrag.database_manager import Bm25Proxy, DenseHandle
    from anrag.index_io import Section
    from anrag.query_rag_retrieval import RetrievalEvaluationSystem
    from anrag.search_engine import SearchEngine

    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    data = niceqa.load_standin(os.path.join(gold, "suggested_queries_bm25_preprocessed.json.gz"),
                               os.path.join(gold, "NICEQA.csv"))
    ids, sources, emb = data["ids"], data["sources"], data["embeddings"].astype(np.float32)
    df = pd.DataFrame({"id": ids, "document": [" ".join(t) for t in data["tokens"]], "source": sources,
                       "embedding": list(emb)})
    DenseHandle(emb, sources).bind(df)
    proxy = Bm25Proxy(Bm25Index(data["tokens"], k1=1.7, b=0.83, epsilon=0.05), sources)
    sections = [Section(d, {"id": i, "source": s}) for i, s, d in zip(ids, sources, df["document"])]
    system = RetrievalEvaluationSystem.__new__(RetrievalEvaluationSystem)
    system.config, system.search_engine, system.voyage_client, system.fused = Config(), SearchEngine(None, None), None, True
    system.embeddings_data = {InfoSource.NICE: {LOCAL_ENCODER_KEY: df}}
    system.bm25_data = {InfoSource.NICE: (proxy, sections, ids)}
    qv, qt = niceqa.encode_questions(data)
    calls = _count_rank_batch(monkeypatch)
    configs = [dict(model_weights={LOCAL_ENCODER_KEY: 1.0, "BM25": 0.0}, use_hybrid_search=False),
               dict(model_weights={LOCAL_ENCODER_KEY: 0.0, "BM25": 1.0}, use_hybrid_search=True),
               dict(model_weights={LOCAL_ENCODER_KEY: 5.0, "BM25": 1.0}, use_hybrid_search=True)]
    for cfg in configs:
        for flt in (None, "CG,NG"):
            for j in range(4):
                ask = dict(query_embeddings={LOCAL_ENCODER_KEY: qv[j]}, query_tokens=qt[j] or ["asthma"], similarity_k=12000,
                           common_sections_n=12000, filename_type_filter=flt, wrrf_k=40, use_reranker=False, **cfg)
                system.RANK_ONE_CALL = False
                before = len(calls)
                off = system.retrieve_documents(**ask)
                assert len(calls) == before and len(off) > 1000
                system.RANK_ONE_CALL = True
                on = system.retrieve_documents(**ask)
                assert calls[before:] == [1], cfg
                assert on == off, (cfg, flt, j)
