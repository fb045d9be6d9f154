"""GPU: `anrag_hybrid_search_f64` -- the fused hybrid query for the float64 embedding of the reference's text path
(search_engine.py:157, :129) -- against the three calls it replaces (`dense_search_f64` + `bm25_search` + `wrrf`) in ids,
fused-score bits and count; between bursts of pipelined fp32 traffic; without allocations in steady state; and through
the reference-shaped host layer, where such a request becomes ONE library call."""
import ctypes as C
import pickle
import sqlite3

import numpy as np
import pytest

from helpers import load_golden

pytestmark = pytest.mark.gpu

WORLDS = {"9609x384": (9609, 384, 4000), "3000x768": (3000, 768, 3000)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def _make_world(n, d, n_docs, seed):
    from anrag.bm25_index import Bm25Index

    rng = np.random.default_rng(seed)
    e = rng.standard_normal((n, d), dtype=np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    vocab = 600
    p = 1.0 / np.arange(1, vocab + 1) ** 1.07
    p /= p.sum()
    docs = [[f"t{j}" for j in rng.choice(vocab, size=int(rng.integers(5, 50)), p=p)] for _ in range(n_docs)]
    bi = Bm25Index(docs, k1=1.7, b=0.83, epsilon=0.05)
    dense_src = (np.arange(n) % 5).astype(np.uint16)
    bm25_src = (np.arange(n_docs) % 3).astype(np.uint16)
    queries = []
    for i in range(4):
        row = int(rng.integers(0, min(n, n_docs)))
        q = e[row].astype(np.float64) + 0.05 * rng.standard_normal(d)
        q /= np.linalg.norm(q)
        toks = [str(t) for t in rng.choice(docs[row], size=int(rng.integers(1, 7)))] + ["not-in-vocab"]
        queries.append((q, bi.term_ids(toks)))
    return dict(e=e, bi=bi, docs=docs, dense_src=dense_src, bm25_src=bm25_src, queries=queries, rng=rng)


@pytest.fixture(scope="module", params=sorted(WORLDS))
def world(request):
    from anrag.index import Index

    n, d, n_docs = WORLDS[request.param]
    w = _make_world(n, d, n_docs, 11 + d)
    bi = w["bi"]
    with Index(0) as idx:
        idx.dense_load(w["e"], source_id=w["dense_src"])
        idx.bm25_load(bi.indptr, bi.post_doc, bi.post_tf, bi.idf, bi.doc_len, bi.avgdl, bi.k1, bi.b, source_id=w["bm25_src"])
        w["idx"] = idx
        yield w


def _composed(idx, q, terms, k, w_dense, w_bm25, wrrf_k, top_n, ad=None, ab=None, dense=True):
    """The three host-synchronous calls of the method-by-method route."""
    lists, weights = [], []
    if dense and w_dense > 0:
        doc, _, cnt = idx.dense_search_f64(q, k, ad)
        lists.append(doc[:cnt])
        weights.append(w_dense)
    if len(terms) and w_bm25 > 0:
        doc, _, cnt = idx.bm25_search(terms, k, ab)
        lists.append(doc[:cnt])
        weights.append(w_bm25)
    return idx.wrrf(lists, weights, wrrf_k, top_n)


def _assert_same(got, want, what):
    assert got[0].tolist() == want[0].tolist(), what
    assert _bits(got[1]) == _bits(want[1]), what


@pytest.mark.parametrize("k", [1, 25, 64])
def test_fused_equals_the_three_calls(world, k):
    idx = world["idx"]
    ad = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    ab = np.array([0, 1, 1], dtype=np.uint8)
    for q, terms in world["queries"]:
        for w_dense, w_bm25, wrrf_k, top_n in ((5.0, 1.0, 40.0, 10), (1.0, 2.5, 60.0, 2 * k)):
            for fa, fb in ((None, None), (ad, None), (None, ab), (ad, ab)):
                s0, t0 = idx.dense_f64_stats()
                got = idx.hybrid_search_f64(q, terms, k, w_dense, w_bm25, wrrf_k, top_n, fa, fb)
                assert idx.dense_f64_stats() == (s0 + 1, t0)
                want = _composed(idx, q, terms, k, w_dense, w_bm25, wrrf_k, top_n, fa, fb)
                _assert_same(got, want, (k, w_dense, w_bm25, fa is not None, fb is not None))
                assert 1 <= len(got[0]) <= top_n
        # a term-less query and w_bm25 = 0 skip the BM25 leg: the dense list, fused alone
        no_terms = np.zeros(0, np.int32)
        _assert_same(idx.hybrid_search_f64(q, no_terms, k, 5.0, 1.0, 40.0, 10),
                     _composed(idx, q, no_terms, k, 5.0, 1.0, 40.0, 10), "no terms")
        _assert_same(idx.hybrid_search_f64(q, terms, k, 5.0, 0.0, 40.0, 10),
                     _composed(idx, q, terms, k, 5.0, 0.0, 40.0, 10), "w_bm25 = 0")
        # w_dense = 0 skips the dense leg
        _assert_same(idx.hybrid_search_f64(q, terms, k, 0.0, 1.0, 40.0, 10),
                     _composed(idx, q, terms, k, 0.0, 1.0, 40.0, 10), "w_dense = 0")
    # the fp32 fused call answers the rounded query: the float64 call is not that call
    q, terms = world["queries"][0]
    assert np.any(q.astype(np.float32).astype(np.float64) != q)


def test_envelope_and_errors(world):
    from anrag import _native as nat
    from anrag.index import Index

    idx = world["idx"]
    q, terms = world["queries"][0]
    for bad in (dict(k=65, top_n=10), dict(k=0, top_n=10), dict(k=25, top_n=129), dict(k=25, top_n=0)):
        with pytest.raises(nat.AnragError) as err:
            idx.hybrid_search_f64(q, terms, bad["k"], 5.0, 1.0, 40.0, bad["top_n"])
        assert err.value.code == -1
    with pytest.raises(nat.AnragError):  # neither leg
        idx.hybrid_search_f64(q, np.zeros(0, np.int32), 25, 0.0, 1.0, 40.0, 10)
    bi = world["bi"]
    # an index without a dense load: the BM25 list, fused alone
    with Index(0) as only_bm25:
        only_bm25.bm25_load(bi.indptr, bi.post_doc, bi.post_tf, bi.idf, bi.doc_len, bi.avgdl, bi.k1, bi.b)
        got = only_bm25.hybrid_search_f64(q, terms, 25, 5.0, 1.0, 40.0, 10)
        want = _composed(only_bm25, q, terms, 25, 5.0, 1.0, 40.0, 10, dense=False)
        _assert_same(got, want, "no dense load")
        assert only_bm25.dense_f64_stats() == (0, 0)
    # a dimension the fp64 list scan does not serve: ANRAG_ERR_UNSUPPORTED with a message, the three calls still answer
    rng = np.random.default_rng(2)
    e6 = rng.standard_normal((300, 6), dtype=np.float32)
    with Index(0) as odd:
        odd.dense_load(e6)
        odd.bm25_load(bi.indptr, bi.post_doc, bi.post_tf, bi.idf, bi.doc_len, bi.avgdl, bi.k1, bi.b)
        assert not odd.dense_f64_scan_serves()
        with pytest.raises(nat.AnragError) as err:
            odd.hybrid_search_f64(rng.standard_normal(6), terms, 25, 5.0, 1.0, 40.0, 10)
        assert err.value.code == nat.ERR_UNSUPPORTED and "dim 6" in str(err.value)
        assert len(_composed(odd, rng.standard_normal(6), terms, 25, 5.0, 1.0, 40.0, 10)[0]) == 10


def test_float64_calls_between_unsynchronised_fp32_bursts(world):
    """fp32 fused queries and single dense lane queries enqueued back to back without a host wait, a float64 call (which
    settles the pipeline and uses list set 0 and the index's staging buffers), another burst: every answer equals the
    answer the same query gets alone."""
    import torch
    from anrag import _native as nat

    idx = world["idx"]
    lib = nat.load_library()
    dev = torch.device("cuda", 0)
    e, rng = world["e"], np.random.default_rng(5)
    nq = 24
    rows = rng.integers(0, e.shape[0], nq)
    q32 = e[rows] + 0.05 * rng.standard_normal((nq, e.shape[1]), dtype=np.float32)
    q32 /= np.linalg.norm(q32, axis=1, keepdims=True)
    terms = [world["queries"][i % 4][1] for i in range(nq)]
    fused_ref = [idx.hybrid_search(q32[i], terms[i], 25, 5.0, 1.0, 40.0, 10) for i in range(nq)]
    dense_ref = [idx.dense_search(q32[i], 10)[0][0] for i in range(nq)]
    f64_ref = [idx.hybrid_search_f64(q, t, 25, 5.0, 1.0, 40.0, 10) for q, t in world["queries"]]
    d64_ref = [idx.dense_search_f64(q, 10) for q, _ in world["queries"]]
    Q = torch.from_numpy(q32).to(dev)
    T = torch.full((nq, 16), -1, dtype=torch.int32, device=dev)
    for i, t in enumerate(terms):
        T[i, : len(t)] = torch.from_numpy(np.asarray(t, np.int32)).to(dev)
    out_f = torch.zeros((nq, 10, 2), dtype=torch.int64, device=dev)
    cnt_f = torch.zeros(nq, dtype=torch.int32, device=dev)
    out_d = torch.zeros((nq, 10, 2), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def burst(lo, hi):
        for i in range(lo, hi):
            if i % 2 == 0:
                nat.check(lib.anrag_hybrid_search_device(idx.handle, Q[i].data_ptr(), T[i].data_ptr(), len(terms[i]), 25, 5.0,
                                                         1.0, 40.0, 10, None, None, out_f[i].data_ptr(), cnt_f[i:].data_ptr()))
            else:
                idx.dense_search_device(Q[i].data_ptr(), 1, 10, 0, out_d[i].data_ptr())

    for rounds in range(2):
        out_f.zero_(); out_d.zero_(); cnt_f.zero_()
        torch.cuda.synchronize()
        burst(0, nq // 2)
        mid = [idx.hybrid_search_f64(q, t, 25, 5.0, 1.0, 40.0, 10) for q, t in world["queries"][:2]]
        burst(nq // 2, nq)
        mid_d = [idx.dense_search_f64(q, 10) for q, _ in world["queries"][2:]]
        mid += [idx.hybrid_search_f64(q, t, 25, 5.0, 1.0, 40.0, 10) for q, t in world["queries"][2:]]
        idx.sync()
        for got, want in zip(mid, f64_ref):
            _assert_same(got, want, ("float64 between bursts", rounds))
        for got, want in zip(mid_d, d64_ref[2:]):
            assert got[0].tolist() == want[0].tolist() and _bits(got[1]) == _bits(want[1]) and got[2] == want[2]
        of, cf, od = out_f.cpu().numpy(), cnt_f.cpu().numpy(), out_d.cpu().numpy()
        for i in range(nq):
            if i % 2 == 0:
                ids, scores = fused_ref[i]
                assert cf[i] == len(ids) and of[i, :cf[i], 1].tolist() == ids.tolist(), (rounds, i)
                assert of[i, :cf[i], 0].copy().view(np.float64).tolist() == scores.tolist()
            else:
                assert od[i, :, 1].tolist() == dense_ref[i].tolist(), (rounds, i)


def test_steady_state_float64_calls_do_not_allocate(world):
    from anrag import _native as nat

    def alloc_calls():
        n = C.c_int64(0)
        nat.check(nat.load_library().anrag_debug_alloc_calls(C.byref(n)))
        return n.value

    idx = world["idx"]
    allow = np.array([1, 0, 1, 1, 0], dtype=np.uint8)

    def step(i):
        q, terms = world["queries"][i % 4]
        return (idx.dense_search_f64(q, 10), idx.dense_search_f64(q, 64, allow),
                idx.hybrid_search_f64(q, terms, 25, 5.0, 1.0, 40.0, 10),
                idx.hybrid_search_f64(q, terms, 64, 5.0, 1.0, 40.0, 128, allow, None))

    first = [step(i) for i in range(4)]
    before = alloc_calls()
    for i in range(50):
        again = step(i)
        for a, b in zip(first[i % 4], again):
            for x, y in zip(a, b):
                assert np.array_equal(np.asarray(x), np.asarray(y))
    assert alloc_calls() == before, "a steady-state float64 query allocated or freed device / pinned memory"


# ------------------------------------------------------------------ the reference-shaped host layer
def _write_db(path, chunks, e):
    conn = sqlite3.connect(path)
    conn.execute("CREATE TABLE chunks (id TEXT PRIMARY KEY, content TEXT NOT NULL, source TEXT NOT NULL,"
                 " embedding BLOB NOT NULL, created_at TIMESTAMP DEFAULT CURRENT_TIMESTAMP, url TEXT)")
    for c, v in zip(chunks, e):
        conn.execute("INSERT INTO chunks (id, content, source, embedding, url) VALUES (?,?,?,?,?)",
                     (c["id"], " ".join(c["tokens"]) or "-", c["source"], np.asarray(v, np.float32).tobytes(), None))
    conn.commit()
    conn.close()


@pytest.fixture()
def e2e(tmp_path):
    from oracle.make_golden import Document, synth_dense
    from oracle.ref_bm25 import BM25Okapi
    from anrag.config import Config, InfoSource

    g = load_golden("ref_end_to_end.json")
    co = g["corpus"]
    chunks = co["chunks"]
    e1 = synth_dense(co["n"], co["d"], co["e1_seed"])
    db1, pkl = str(tmp_path / "m1.db"), str(tmp_path / "bm25.pkl")
    _write_db(db1, chunks, e1)
    kept = [c for c in chunks if c["tokens"]]
    bm25 = BM25Okapi([c["tokens"] for c in kept], k1=1.7, b=0.83, epsilon=0.05)
    sections = [Document(" ".join(c["tokens"]), {"id": c["id"], "source": c["source"]}) for c in kept]
    with open(pkl, "wb") as f:
        pickle.dump({"bm25": bm25, "sections": sections, "section_ids": [c["id"] for c in kept], "config": {}}, f)
    cfg = Config()
    sc = cfg.SOURCE_CONFIGS[InfoSource.NICE]
    saved = dict(vars(sc))
    sc.db_path = sc.voyage_db_path = db1
    sc.openai_db_path = sc.voyage_3_5_db_path = sc.qwen_db_path = sc.local_db_path = None
    sc.bm25_path = pkl
    yield chunks, cfg, e1
    for k, v in saved.items():
        setattr(sc, k, v)


def _requests(chunks, e1, count=6):
    from oracle.make_golden import synth_query

    rng = np.random.default_rng(31)
    for i in range(count):
        target = int(rng.integers(0, len(chunks)))
        q64 = synth_query(e1, 900 + i, target).astype(np.float64) + rng.standard_normal(e1.shape[1]) * 1e-9
        toks = chunks[target]["tokens"][:3] or ["asthma"]
        flt = "CG,NG" if i % 3 == 2 else None
        yield q64, dict(query_tokens=toks, similarity_k=25 if i % 2 else 64, common_sections_n=15, use_hybrid_search=True,
                        wrrf_k=40, model_weights={"voyage-3-large": 5.0, "BM25": 1.0}, filename_type_filter=flt,
                        use_reranker=False)


def test_retrieve_documents_with_a_float64_embedding_is_one_library_call(e2e, monkeypatch):
    from anrag.index import Index
    from anrag.query_rag_retrieval import RetrievalEvaluationSystem

    chunks, cfg, e1 = e2e
    calls = {"f64": 0, "other": 0}
    fused_call = Index.hybrid_search_f64

    def counted(self, *a, **kw):
        calls["f64"] += 1
        return fused_call(self, *a, **kw)

    def other(name):
        inner = getattr(Index, name)

        def wrapped(self, *a, **kw):
            calls["other"] += 1
            return inner(self, *a, **kw)

        return wrapped

    fused, plain = RetrievalEvaluationSystem(cfg, fused=True), RetrievalEvaluationSystem(cfg, fused=False)
    asked = 0
    for q64, kw in _requests(chunks, e1):
        want = plain.retrieve_documents(query_embeddings={"voyage-3-large": q64}, **kw)
        with monkeypatch.context() as m:
            m.setattr(Index, "hybrid_search_f64", counted)
            for name in ("dense_search", "dense_search_f64", "bm25_search", "wrrf", "hybrid_search", "hybrid_search_batch"):
                m.setattr(Index, name, other(name))
            calls["f64"] = calls["other"] = 0
            got = fused.retrieve_documents(query_embeddings={"voyage-3-large": q64}, **kw)
            assert (calls["f64"], calls["other"]) == (1, 0), kw
        assert got == want and len(got) == 15, kw
        asked += 1
    assert asked == 6


def test_a_shard_group_world_still_answers_by_the_old_route(e2e, monkeypatch):
    """`hybrid_search_ids` declines a float64 query on a ShardGroup (there is no group form of the fused fp64 call): the
    method-by-method route answers, with the single index's ids."""
    from anrag.database_manager import ATTR
    from anrag.index import Index, ShardGroup
    from anrag.query_rag_retrieval import RetrievalEvaluationSystem

    chunks, cfg, e1 = e2e
    single = RetrievalEvaluationSystem(cfg, fused=True)
    want = [single.retrieve_documents(query_embeddings={"voyage-3-large": q64}, **kw) for q64, kw in _requests(chunks, e1, 3)]
    monkeypatch.setenv("ANRAG_DEVICES", "0,0,0")
    grouped = RetrievalEvaluationSystem(cfg, fused=True)
    frames = [df for d in grouped.embeddings_data.values() for df in d.values() if df is not None and not df.empty]
    assert frames and all(isinstance(df.attrs[ATTR].index, ShardGroup) for df in frames)

    def never(self, *a, **kw):
        raise AssertionError("the fused fp64 call has no group form")

    monkeypatch.setattr(Index, "hybrid_search_f64", never)
    got = [grouped.retrieve_documents(query_embeddings={"voyage-3-large": q64}, **kw) for q64, kw in _requests(chunks, e1, 3)]
    assert got == want
