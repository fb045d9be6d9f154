"""GPU: ranked query lists (full ranking) across the shards of a shard group -- `rank_batch_group`
(`anrag_shard_group_rank_batch`) against `rank_batch` on ONE `Index` that holds the whole corpus: ids equal, counts
equal, ranks equal, score bits equal as integers.  All shards on device 0; the two-device case arms itself where
`anrag_device_count` reports two."""
import ctypes as C

import numpy as np
import pytest

from group_rank_model import merge_by_counting, merge_by_doc, shard_lists, whole_list
from test_gpu_shard_group import e2e_world, load, make_corpus, make_queries  # noqa: F401  (e2e_world: a fixture)

pytestmark = pytest.mark.gpu

N, D = 9609, 384
FULL = 12000  # retrieval_eval.py's "rank everything"


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same(got, want, what):
    """(ids, scores, counts[, ranks]) of the group == those of the single index."""
    assert len(got) == len(want), what
    assert np.array_equal(got[2], want[2]), (what, "counts")
    if want[0] is None:
        assert got[0] is None, what
    else:
        assert np.array_equal(got[0], want[0]), (what, "ids")
    if want[1] is None:
        assert got[1] is None, what
    else:
        assert np.array_equal(_bits(got[1]), _bits(want[1])), (what, "score bits")
    if len(want) == 4:
        assert np.array_equal(got[3], want[3]), (what, "ranks")


def dense_leg(ix, Q, w=5.0, allow=None, dmap=None):
    return dict(index=ix, weight=w, queries=Q, allow=allow, doc_of_row=dmap)


def bm25_leg(ix, terms, w=1.0, allow=None, dmap=None):
    return dict(index=ix, weight=w, term_lists=terms, allow=allow, doc_of_row=dmap)


def on(ix, leg):
    return dict(leg, index=ix)


@pytest.fixture(scope="module")
def world():
    from anrag.index import Index

    c = make_corpus(N, D, seed=81)
    single = load(Index(0), c)
    Q, terms = make_queries(c, 13, seed=82)  # 13: not a multiple of 8
    yield c, single, Q, terms
    single.close()


@pytest.mark.parametrize("S", [1, 2, 3, 4, 8])
def test_single_legs(world, S):
    """1. One dense leg and one BM25 leg: k = 12,000 (the full ranking, k_s clamped to the shard's rows), 25 and 1, with
    and without a source filter."""
    from anrag.index import ShardGroup, rank_batch, rank_batch_group

    c, single, Q, terms = world
    nq = len(Q)
    some = np.zeros(c["n_sources"], np.uint8)
    some[[1, 3, 4]] = 1
    with ShardGroup([0] * S) as g:
        load(g, c)
        for k in (FULL, 25, 1):
            for allow in (None, some):
                for leg in (dense_leg(single, Q, allow=allow), bm25_leg(single, terms, allow=allow)):
                    want = rank_batch([leg], nq, k, 60.0, k, want_scores=True)
                    got = rank_batch_group([on(g, leg)], nq, k, 60.0, k, want_scores=True)
                    assert want[2].min() >= 1 and want[0][:, 0].min() >= 0  # not a comparison of two empty answers
                    same(got, want, (S, k, allow is not None, "queries" in leg))
        want = rank_batch([dense_leg(single, Q)], nq, FULL, 60.0, FULL)
        assert want[2].tolist() == [N] * nq


@pytest.mark.parametrize("in_hbm", [False, True])
def test_fusions(world, in_hbm, monkeypatch):
    """2. Dense + BM25; two dense models + BM25 with permuted document maps, the legs on groups of DIFFERENT shard counts
    and one leg on a plain Index; fusion in LDS and in HBM (the env switch, and an id space past 13,312)."""
    from anrag.index import Index, ShardGroup, rank_batch, rank_batch_group

    c, single, Q, terms = world
    nq = len(Q)
    rng = np.random.default_rng(5)
    c2 = make_corpus(N, 256, seed=83)
    Q2, _ = make_queries(c2, nq, seed=84)
    if in_hbm:
        monkeypatch.setenv("ANRAG_RANK_FUSE_IN_HBM", "1")
    with Index(0) as single2, ShardGroup([0] * 4) as g4, ShardGroup([0] * 3) as g3, ShardGroup([0] * 2) as g2:
        load(single2, c2, bm25=False)
        load(g4, c, bm25=False)
        load(g3, c, dense=False)
        load(g2, c2, bm25=False)
        for k, top in ((FULL, FULL), (FULL, 100), (25, 40)):
            legs = [dense_leg(single, Q), bm25_leg(single, terms)]
            want = rank_batch(legs, nq, k, 40.0, top, id_space=N, want_scores=True)
            got = rank_batch_group([on(g4, legs[0]), on(g3, legs[1])], nq, k, 40.0, top, id_space=N, want_scores=True)
            assert want[2].min() >= min(top, 25)
            same(got, want, ("2 legs", k, top))
        for id_space in (N, 14000):  # 14000 > 13,312: the HBM fusion whatever the switch
            maps = [rng.permutation(id_space)[:N].astype(np.int64) for _ in range(3)]
            legs = [dense_leg(single, Q, 5.0, dmap=maps[0]), dense_leg(single2, Q2, 3.0, dmap=maps[1]),
                    bm25_leg(single, terms, 1.0, dmap=maps[2])]
            for k, top in ((FULL, FULL), (300, 50)):
                want = rank_batch(legs, nq, k, 60.0, top, id_space=id_space, want_scores=True)
                # leg 0 on four shards, leg 1 on ONE plain index, leg 2 on three shards
                got = rank_batch_group([on(g4, legs[0]), legs[1], on(g3, legs[2])], nq, k, 60.0, top, id_space=id_space,
                                       want_scores=True)
                same(got, want, ("3 legs", id_space, k, top))
                # ... and the plain index FIRST (it is the home), the second model on two shards
                got = rank_batch_group([legs[0], on(g2, legs[1]), on(g3, legs[2])], nq, k, 60.0, top, id_space=id_space,
                                       want_scores=True)
                same(got, want, ("3 legs, index home", id_space, k, top))


def test_ties_across_shard_boundaries():
    """3. What tells the merge in shard order from a doc-id merge: a BM25 corpus where far fewer than k documents score
    above zero (the cut falls inside a run of zeros spanning several shards), dense rows duplicated on both sides of
    every shard boundary, a permuted document map.  On the CPU first: a (score desc, doc id asc) merge of the shards'
    lists differs from the expected lists on these inputs."""
    from oracle import ref_bm25
    from anrag.index import Index, ShardGroup, group_bounds, rank_batch, rank_batch_group

    n, d, k = 4000, 256, 1500
    c = make_corpus(n, d, 20262, vocab=3000)
    for S in (2, 3, 4, 8):
        for b in group_bounds(n, S)[1:-1]:
            c["E"][b] = c["E"][b - 1]
    rng = np.random.default_rng(9)
    dmap = rng.permutation(n).astype(np.int64)
    df = np.diff(c["indptr"])
    rare = np.nonzero((df >= 1) & (df <= 6))[0]
    terms = [np.array([t], np.int32) for t in rng.choice(rare, size=21, replace=False)]
    Q = np.stack([c["E"][b] for b in group_bounds(n, 8)[1:-1]] * 3).astype(np.float32)
    nq = len(Q)
    assert nq == len(terms)
    for S in (2, 4, 8):
        lo = group_bounds(n, S)
        differ = 0
        for t in terms:
            s = ref_bm25.csr_get_scores(c["indptr"], c["post_doc"], c["post_tf"], c["idf"], c["doc_len"], c["avgdl"], 1.7,
                                        0.83, [int(x) for x in t])
            assert (s > 0).sum() < k // 10
            lists = shard_lists(s, lo, k)
            rows, _ = merge_by_counting(lists, lo, k)
            assert rows.tolist() == whole_list(s, k)[0].tolist()  # shard order IS (score desc, global row asc)
            by_doc, _ = merge_by_doc(lists, lo, k, dmap)
            differ += by_doc.tolist() != rows.tolist()
        assert differ == len(terms), f"S={S}: the inputs do not separate the two merges ({differ}/{len(terms)})"
    with Index(0) as single:
        load(single, c, src=False)
        for S in (2, 3, 4, 8):
            with ShardGroup([0] * S) as g:
                load(g, c, src=False)
                leg = bm25_leg(single, terms, dmap=dmap)
                want = rank_batch([leg], nq, k, 60.0, k, want_scores=True)
                assert want[2].tolist() == [k] * nq and (want[1][:, k - 1] == 0.0).all()  # cut inside the zeros
                same(rank_batch_group([on(g, leg)], nq, k, 60.0, k, want_scores=True), want, (S, "bm25"))
                leg_d = dense_leg(single, Q, dmap=dmap)
                want = rank_batch([leg_d], nq, k, 60.0, k, want_scores=True)
                assert (want[1][:, 0] == want[1][:, 1]).all()  # the duplicated rows tie at the top
                same(rank_batch_group([on(g, leg_d)], nq, k, 60.0, k, want_scores=True), want, (S, "dense"))
                legs = [leg_d, leg]
                want = rank_batch(legs, nq, k, 60.0, k, id_space=n, want_scores=True)
                same(rank_batch_group([on(g, l) for l in legs], nq, k, 60.0, k, id_space=n, want_scores=True), want,
                     (S, "fused"))


def test_edges(monkeypatch):
    """4. A filter that keeps fewer than k rows overall and none in some shard; a query without term ids; a NaN row; a
    list long enough for two chunks; one past the cap and a document named twice are ERR_INVALID."""
    from anrag import _native as nat
    from anrag.index import Index, ShardGroup, group_bounds, rank_batch, rank_batch_group

    c = make_corpus(N, D, seed=85)
    c["E"][9600, 5] = np.nan
    S = 4
    lo = group_bounds(N, S)
    src = np.zeros(N, np.uint16)
    src[lo[1]:] = 1
    src[N - 7:] = 2                                     # source 2 = the last 7 rows; source 0 = the first block
    c["src"] = src
    Q, terms = make_queries(c, 21, seed=86)
    Q = np.nan_to_num(Q)
    terms[2] = np.zeros(0, np.int32)
    terms[20] = np.zeros(0, np.int32)
    nq = len(Q)
    with Index(0) as single, ShardGroup([0] * S) as g:
        load(single, c)
        load(g, c)
        want = rank_batch([dense_leg(single, Q)], nq, FULL, 60.0, 5, want_scores=True)
        assert (want[0][:, 0] == 9600).all() and np.isposinf(want[1][:, 0]).all()  # the NaN row ranks first, as +inf
        same(rank_batch_group([dense_leg(g, Q)], nq, FULL, 60.0, 5, want_scores=True), want, "nan")
        for allow in (np.array([0, 0, 1], np.uint8), np.array([1, 0, 0], np.uint8), np.array([0, 1, 1], np.uint8)):
            legs = [dense_leg(single, Q, allow=allow), bm25_leg(single, terms, allow=allow)]
            for sub in ([legs[0]], [legs[1]], legs):
                want = rank_batch(sub, nq, FULL, 60.0, FULL, id_space=N, want_scores=True)
                got = rank_batch_group([on(g, l) for l in sub], nq, FULL, 60.0, FULL, id_space=N, want_scores=True)
                same(got, want, (allow.tolist(), len(sub)))
        want = rank_batch([dense_leg(single, Q, allow=np.array([0, 0, 1], np.uint8))], nq, FULL, 60.0, FULL)
        assert want[2].tolist() == [7] * nq
        want = rank_batch([bm25_leg(single, terms)], nq, FULL, 60.0, FULL)
        assert want[2][2] == 0 and want[2][20] == 0 and want[2][3] == N  # no term ids: no list for that query only
        # two chunks: 21 queries, a budget that holds 16 of them
        legs = [dense_leg(single, Q), bm25_leg(single, terms)]
        want = rank_batch(legs, nq, FULL, 60.0, FULL, id_space=N, want_scores=True)
        per_query = N * 12 + 2 * N * 12 * 2 + FULL * 16
        monkeypatch.setenv("ANRAG_RANK_CHUNK_BUDGET", str(17 * per_query))
        got = rank_batch_group([on(g, l) for l in legs], nq, FULL, 60.0, FULL, id_space=N, want_scores=True)
        same(got, want, "two chunks")
        monkeypatch.setenv("ANRAG_RANK_CHUNK_BUDGET", "1")  # a chunk per query
        got = rank_batch_group([on(g, l) for l in legs], nq, FULL, 60.0, FULL, id_space=N, want_scores=True)
        same(got, want, "21 chunks")
        monkeypatch.delenv("ANRAG_RANK_CHUNK_BUDGET")
        twice = np.arange(N, dtype=np.int64)
        twice[lo[2] + 3] = 5                            # document 5 named by a row of shard 0 and a row of shard 2
        with pytest.raises(nat.AnragError) as e:
            rank_batch_group([dense_leg(g, Q, dmap=twice), bm25_leg(g, terms)], nq, FULL, 60.0, FULL, id_space=N)
        assert e.value.code == -1 and "two rows" in str(e.value)
    big = make_corpus(16400, 32, seed=87)
    Qb, tb = make_queries(big, 3, seed=88)
    with ShardGroup([0, 0]) as g:
        load(g, big)
        for leg, k in ((dense_leg(g, Qb), 16385), (bm25_leg(g, tb), 13313)):
            with pytest.raises(nat.AnragError) as e:
                rank_batch_group([leg], 3, k, 60.0, 10)
            assert e.value.code == -1 and "envelope" in str(e.value)
        with pytest.raises(nat.AnragError) as e:  # the fused cut
            rank_batch_group([dense_leg(g, Qb), bm25_leg(g, tb)], 3, 13312, 60.0, 13313, id_space=16400)
        assert e.value.code == -1 and "envelope" in str(e.value)


def test_expect_and_ranks(world):
    """5. Ranks of expected documents: present, absent (outside the list) and -2 (an id no frame holds); ids not wanted,
    on fused and on single legs."""
    from anrag.index import ShardGroup, rank_batch, rank_batch_group

    c, single, Q, terms = world
    nq = len(Q)
    rng = np.random.default_rng(11)
    dmap = rng.permutation(N).astype(np.int64)
    with ShardGroup([0] * 3) as g:
        load(g, c)
        legs = [dense_leg(single, Q, dmap=dmap), bm25_leg(single, terms, dmap=dmap)]
        for sub, k, top in ((legs, FULL, FULL), (legs, 200, 50), ([legs[0]], FULL, FULL), ([legs[1]], 300, 300),
                            ([legs[0]], 40, 10)):
            ids = rank_batch(sub, nq, k, 60.0, top, id_space=N)[0]
            expect = ids[:, min(top, 7) - 1].copy()     # present, at rank 7 (or the last of a short list)
            expect[1] = -2
            expect[4] = ids[4, 0]
            if top < N:
                expect[5] = np.setdiff1d(np.arange(N), ids[5])[0]  # a document that is not in the answer
            for want_ids in (True, False):
                want = rank_batch(sub, nq, k, 60.0, top, id_space=N, expect=expect, want_ids=want_ids, want_scores=want_ids)
                got = rank_batch_group([on(g, l) for l in sub], nq, k, 60.0, top, id_space=N, expect=expect,
                                       want_ids=want_ids, want_scores=want_ids)
                assert want[3][1] == -1 and want[3][4] == 1 and want[3][0] == min(top, 7)
                same(got, want, (len(sub), k, top, want_ids))


def _alloc_calls():
    from anrag import _native as nat

    n = C.c_int64(0)
    nat.check(nat.load_library().anrag_debug_alloc_calls(C.byref(n)))
    return n.value


def test_steady_state_allocates_nothing(world):
    """6. `anrag_debug_alloc_calls` does not move over repeated calls after the first."""
    from anrag.index import ShardGroup, rank_batch_group

    c, single, Q, terms = world
    nq = len(Q)
    with ShardGroup([0] * 4) as g:
        load(g, c)
        legs = [dense_leg(g, Q), bm25_leg(g, terms)]
        first = rank_batch_group(legs, nq, FULL, 60.0, FULL, id_space=N, want_scores=True)
        rank_batch_group(legs[:1], nq, FULL, 60.0, FULL)
        before = _alloc_calls()
        for _ in range(5):
            again = rank_batch_group(legs, nq, FULL, 60.0, FULL, id_space=N, want_scores=True)
            rank_batch_group(legs[:1], nq, 25, 60.0, 10)
            rank_batch_group(legs[1:], nq, FULL, 60.0, FULL)
        assert _alloc_calls() == before
        same(again, first, "repeat")


def test_interleaved_with_the_hot_route(world):
    """7. A `hybrid_search_batch` burst on the same group directly before and after a ranked call, nothing synced in
    between: both unchanged."""
    from anrag.index import ShardGroup, rank_batch, rank_batch_group

    c, single, Q, terms = world
    Qh, th = make_queries(c, 40, seed=89)
    nq = len(Q)
    with ShardGroup([0] * 3) as g:
        load(g, c)
        legs = [dense_leg(single, Q), bm25_leg(single, terms)]
        want_r = rank_batch(legs, nq, FULL, 60.0, FULL, id_space=N, want_scores=True)
        want_h = single.hybrid_search_batch(Qh, th, 25, 5.0, 1.0, 40.0, 10)
        for _ in range(3):
            h1 = g.hybrid_search_batch(Qh, th, 25, 5.0, 1.0, 40.0, 10)
            r = rank_batch_group([on(g, l) for l in legs], nq, FULL, 60.0, FULL, id_space=N, want_scores=True)
            h2 = g.hybrid_search_batch(Qh, th, 25, 5.0, 1.0, 40.0, 10)
            same(r, want_r, "ranked between two bursts")
            for h in (h1, h2):
                assert np.array_equal(h[0], want_h[0]) and np.array_equal(_bits(h[1]), _bits(want_h[1]))
                assert np.array_equal(h[2], want_h[2])


def test_through_the_classes(e2e_world, monkeypatch):
    """8. Under ANRAG_DEVICES=0,0,0: `retrieve_documents_batch` with similarity_k = 12000 on the golden end-to-end world
    equals the per-query `retrieve_documents` lists, through `rank_batch_group`; `rank_of_expected_batch` stays None."""
    from oracle.make_golden import synth_query
    from anrag import index
    from anrag.database_manager import ATTR
    from anrag.query_rag_retrieval import RetrievalEvaluationSystem

    g, cfg, e1, e2 = e2e_world
    system = RetrievalEvaluationSystem(cfg, fused=True)
    frames = [df for d in system.embeddings_data.values() for df in d.values() if df is not None and not df.empty]
    assert frames and all(isinstance(df.attrs[ATTR].index, index.ShardGroup) for df in frames)
    calls = []
    real = index.rank_batch_group

    def spy(legs, *a, **k):
        calls.append([type(l["index"]).__name__ for l in legs])
        return real(legs, *a, **k)

    monkeypatch.setattr(index, "rank_batch_group", spy)
    asks = []
    for c in g["cases"][:20]:
        asks.append({"query_embeddings": {"voyage-3-large": synth_query(e1, c["q1_seed"], c["target"]),
                                          "text-embedding-3-large": synth_query(e2, c["q2_seed"], c["target"])},
                     "query_tokens": c["tokens"]})
    for params in (dict(similarity_k=12000, common_sections_n=12000, use_hybrid_search=True),
                   dict(similarity_k=12000, common_sections_n=12000, use_hybrid_search=False),
                   dict(similarity_k=12000, common_sections_n=30, use_hybrid_search=True,
                        model_weights={"voyage-3-large": 1.0, "text-embedding-3-large": 0.0, "BM25": 1.0})):
        n_before = len(calls)
        out = system.retrieve_documents_batch(asks, use_reranker=False, **params)
        assert len(calls) == n_before + 1 and set(calls[-1]) == {"ShardGroup"}, params
        want = [system.retrieve_documents(**q, use_reranker=False, **params) for q in asks]
        assert len(calls) == n_before + 1          # the single calls do not come through the list entry
        assert out == want and all(len(w) > 0 for w in want), params
        assert system.rank_of_expected_batch(asks, ["x"] * len(asks), use_reranker=False, **params) is None


def test_full_size_1m_x768():
    """9. 1M x 768 + 1M BM25 documents, k = 12,000, fused, S in {2, 4}, 32 queries == the single index."""
    import torch
    from anrag import synth
    from anrag.index import Index, ShardGroup, rank_batch, rank_batch_group

    dev = torch.device("cuda", 0)
    n, d, nq = 1_000_000, 768, 32
    E = synth.dense_corpus(n, d, 1234, dev)
    Qd, _ = synth.dense_queries(E, nq, 4321)
    post = synth.bm25_postings(n, 200_000, 777, dev)
    idf = synth.bm25_idf(post["df"].cpu().numpy(), n)
    terms = synth.bm25_queries(post, nq, 19)
    torch.cuda.synchronize()
    c = dict(E=E.cpu().numpy(), indptr=np.asarray(post["indptr"]), post_doc=post["post_doc"].cpu().numpy(),
             post_tf=post["post_tf"].cpu().numpy(), idf=idf, doc_len=np.asarray(post["doc_len"]),
             avgdl=post["total_len"] / n, src=None)
    Q = Qd.cpu().numpy()
    del E, post
    torch.cuda.empty_cache()
    with Index(0) as single:
        load(single, c, src=False)
        legs = [dense_leg(single, Q), bm25_leg(single, terms)]
        want = rank_batch(legs, nq, FULL, 60.0, FULL, id_space=n, want_scores=True)
        want1 = rank_batch(legs[:1], nq, FULL, 60.0, FULL, want_scores=True)
    assert want[2].tolist() == [FULL] * nq
    for S in (2, 4):
        with ShardGroup([0] * S) as g:
            load(g, c, src=False)
            glegs = [dense_leg(g, Q), bm25_leg(g, terms)]
            same(rank_batch_group(glegs, nq, FULL, 60.0, FULL, id_space=n, want_scores=True), want, S)
            same(rank_batch_group(glegs[:1], nq, FULL, 60.0, FULL, want_scores=True), want1, (S, "dense"))


@pytest.mark.parametrize("devices", [[0, 1], [1, 0]])
def test_distinct_devices(devices):
    """10. Two GPUs: the home device merges a list that lives on the other one (read over the fabric, or staged); the
    legs of one call on groups whose home devices differ."""
    from anrag import _native as nat
    from anrag.index import Index, ShardGroup, rank_batch, rank_batch_group

    if nat.device_count() < 2:
        pytest.skip("needs two devices")
    c = make_corpus(N, D, seed=90)
    Q, terms = make_queries(c, 13, seed=91)
    with Index(0) as single, ShardGroup(devices) as g, ShardGroup(devices[::-1]) as g_rev:
        load(single, c)
        load(g, c)
        load(g_rev, c)
        legs = [dense_leg(single, Q), bm25_leg(single, terms)]
        for k, top in ((FULL, FULL), (25, 10)):
            want = rank_batch(legs, 13, k, 60.0, top, id_space=N, want_scores=True)
            same(rank_batch_group([on(g, l) for l in legs], 13, k, 60.0, top, id_space=N, want_scores=True), want, (k, "one group"))
            same(rank_batch_group([on(g, legs[0]), on(g_rev, legs[1])], 13, k, 60.0, top, id_space=N, want_scores=True), want,
                 (k, "two groups"))
            want1 = rank_batch(legs[:1], 13, k, 60.0, top, want_scores=True)
            same(rank_batch_group([on(g, legs[0])], 13, k, 60.0, top, want_scores=True), want1, (k, "dense"))
