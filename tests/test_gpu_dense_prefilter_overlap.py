"""The hybrid pipeline keeps `primary` for the shadow scans alone: threshold and rescore of query i run on the tail's
stream under the scans of the following queries (api.hip, hybrid_enqueue_group).  These tests only reorder legal calls:
long bursts without a sync in between, so that pipeline slots are reused while earlier rescores may still be queued, and
bursts followed at once by whatever drains the pipeline or changes the route.  Mode 2 (int8 prefilter) must answer what
mode 0 (the fp32 scan) answers, bit for bit.

The corpus is far below the 1 GiB gate, where single fused device queries would take the one-stream lanes: caller-owned
streams keep them on the three-stream pipeline.  The candidate entry points and the host list call (with document ids,
which the ranking route does not serve) always take it.  A call that brings 16 queries is launched by the library in
groups of 8 (kScanGroup): no launch here carries more than 8 queries.

What these tests are: regression tests of the drain paths and of the results under reordering.  What they are not: a
proof of the slot-lifetime argument.  On a corpus this small a scan takes about 10 us, and a missing ordering edge (a
rescore reading hi[slot] after its next writer, say) would show only by luck of timing.  The argument itself is written
down above hybrid_enqueue_group."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, VOCAB = 60_000, 768, 300
NQ = 112  # 3.5 x kPipeSlots (32), 7 calls of 16
K, TOP_N = 25, 10


@pytest.fixture(scope="module")
def data():
    from anrag.bm25_index import Bm25Index

    rng = np.random.default_rng(61)
    e = rng.standard_normal((N, D), dtype=np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    p = 1.0 / np.arange(1, VOCAB + 1) ** 1.07
    p /= p.sum()
    corpus = [[f"t{j}" for j in rng.choice(VOCAB, size=int(rng.integers(5, 30)), p=p)] for _ in range(N)]
    bi = Bm25Index(corpus, k1=1.7, b=0.83, epsilon=0.05)
    rows = rng.choice(N, NQ, replace=False)  # distinct planted rows: distinct queries
    q = e[rows] + 0.05 * rng.standard_normal((NQ, D), dtype=np.float32)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    terms = [bi.term_ids([str(t) for t in rng.choice(corpus[r], size=int(rng.integers(1, 7)))]) for r in rows]
    return e, bi, q, terms


def _index(data, doc_ids=False):
    from anrag.index import Index

    e, bi, _, _ = data
    idx = Index(0)
    idx.dense_load(e, doc_id=np.arange(N, dtype=np.int64) if doc_ids else None)
    idx.bm25_load(bi.indptr, bi.post_doc, bi.post_tf, bi.idf, bi.doc_len, bi.avgdl, bi.k1, bi.b)
    return idx


class _Device:
    """The queries in HBM, output blocks, and the device entry points called back to back with no sync."""

    def __init__(self, data):
        import torch
        from anrag import _native as nat

        self.torch, self.nat, self.lib = torch, nat, nat.load_library()
        _, _, q, terms = data
        dev = torch.device("cuda", 0)
        self.n_terms = [len(t) for t in terms]
        self.Q = torch.from_numpy(q).to(dev)
        self.T = torch.full((NQ, 8), -1, dtype=torch.int32, device=dev)
        for i, t in enumerate(terms):
            self.T[i, : len(t)] = torch.from_numpy(np.asarray(t, dtype=np.int32)).to(dev)
        self.out_f = torch.zeros((NQ, TOP_N, 2), dtype=torch.int64, device=dev)
        self.cnt_f = torch.zeros(NQ, dtype=torch.int32, device=dev)
        self.out_c = torch.zeros((NQ, 2 * K, 2), dtype=torch.int64, device=dev)
        self.streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
        torch.cuda.synchronize()

    def own_streams(self, idx):
        idx.set_streams(*(s.cuda_stream for s in self.streams))

    def clear(self):
        self.out_f.zero_(); self.cnt_f.zero_(); self.out_c.zero_()
        self.torch.cuda.synchronize()

    def fused(self, idx, qs):
        for i in qs:
            self.nat.check(self.lib.anrag_hybrid_search_device(
                idx.handle, self.Q[i].data_ptr(), self.T[i].data_ptr(), self.n_terms[i], K, 5.0, 1.0, 40.0, TOP_N, None,
                None, self.out_f[i].data_ptr(), self.cnt_f[i:].data_ptr()))

    def candidates(self, idx, qs):
        for i in qs:
            self.nat.check(self.lib.anrag_hybrid_candidates_device(
                idx.handle, self.Q[i].data_ptr(), self.T[i].data_ptr(), self.n_terms[i], K, None, None,
                self.out_c[i].data_ptr()))

    def candidate_groups(self, idx, qs, per_call=16):
        import ctypes as C

        qs = list(qs)
        for g0 in range(0, len(qs), per_call):
            g = qs[g0:g0 + per_call]
            pq = (C.c_void_p * len(g))(*[self.Q[i].data_ptr() for i in g])
            pt = (C.c_void_p * len(g))(*[self.T[i].data_ptr() for i in g])
            nt = (C.c_int32 * len(g))(*[self.n_terms[i] for i in g])
            po = (C.c_void_p * len(g))(*[self.out_c[i].data_ptr() for i in g])
            self.nat.check(self.lib.anrag_hybrid_candidates_group_device(idx.handle, pq, pt, nt, len(g), K, None, None, po))

    def results(self, idx):
        idx.sync()
        return self.out_f.cpu().numpy().copy(), self.cnt_f.cpu().numpy().copy(), self.out_c.cpu().numpy().copy()


def _equal(a, b):
    for x, y in zip(a, b):  # int64 records: the fp64 / fp32 score bits and the ids
        assert np.array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.parametrize("shape", ["fused-single", "candidates-single", "candidates-16-per-call"])
def test_long_bursts_reuse_slots_under_queued_rescores(data, shape):
    dv = _Device(data)
    with _index(data) as idx:
        dv.own_streams(idx)
        got = {}
        for mode in (0, 2, 2):  # the second mode-2 burst starts on slots the first one has used
            idx.set_dense_prefilter(mode)
            dv.clear()
            {"fused-single": dv.fused, "candidates-single": dv.candidates,
             "candidates-16-per-call": dv.candidate_groups}[shape](idx, range(NQ))
            res = dv.results(idx)
            if shape == "fused-single":
                assert (res[1] == TOP_N).all()
            else:
                assert (res[2][:, :K, 1] >= 0).all()
            if mode in got:
                _equal(got[mode], res)
            got[mode] = res
        _equal(got[0], got[2])
        queries, survivors = idx.dense_prefilter_stats()
        assert queries == 2 * NQ and survivors >= queries * K


def test_long_fused_list_in_groups(data):
    """anrag_hybrid_search_batch: 112 fused queries enqueued in groups (one scan, one threshold, one rescore and one tail
    launch per group) with no sync between the groups."""
    _, _, q, terms = data
    with _index(data, doc_ids=True) as idx:
        idx.set_dense_prefilter(0)
        off = idx.hybrid_search_batch(q, terms, K, 5.0, 1.0, 40, TOP_N)
        idx.set_dense_prefilter(2)
        on = idx.hybrid_search_batch(q, terms, K, 5.0, 1.0, 40, TOP_N)
        assert np.array_equal(off[0], on[0]) and np.array_equal(off[2], on[2])
        assert np.array_equal(off[1].view(np.uint64), on[1].view(np.uint64))
        assert idx.dense_prefilter_stats()[0] == NQ


def test_burst_then_drain_or_mode_change_without_a_sync(data):
    """A burst, then AT ONCE (the caller does not sync) a call that frees or rebuilds the prefilter block, hands the list
    sets to the lanes, or runs the ranking route; then another burst."""
    import torch
    from anrag.index import rank_batch

    _, _, q, terms = data
    dv = _Device(data)
    a, b = range(0, 48), range(48, 96)  # each longer than kPipeSlots
    with _index(data) as idx:
        dv.own_streams(idx)
        idx.set_dense_prefilter(0)
        dv.clear()
        dv.fused(idx, range(NQ))
        dv.candidates(idx, range(NQ))
        want = dv.results(idx)
        one = torch.zeros((K, 2), dtype=torch.int64, device="cuda")
        idx.dense_search_device(dv.Q[5].data_ptr(), 1, K, None, one.data_ptr())
        idx.sync()
        one_want = one.cpu().numpy().copy()
        legs = [dict(index=idx, weight=5.0, queries=q[:4]), dict(index=idx, weight=1.0, term_lists=terms[:4])]
        rank_want = rank_batch(legs, 4, 2000, 40, 2000, id_space=N, want_scores=True)

        def between_set_fp16():
            idx.set_dense_prefilter(1)  # frees the int8 block, builds the fp16 one: the second burst runs on K1F

        def between_set_off():
            idx.set_dense_prefilter(0)  # frees the block: the second burst runs on K1

        def between_lane_query():
            # no sync of the caller's in front: dense_single_enqueue itself has to let the pipeline drain, the rescores and
            # tails still queued on the tail's stream included, before the lanes take over the list sets
            idx.dense_search_device(dv.Q[5].data_ptr(), 1, K, None, one.data_ptr())

        def between_rank_batch():
            got = rank_batch(legs, 4, 2000, 40, 2000, id_space=N, want_scores=True)
            for x, y in zip(got, rank_want):
                assert np.array_equal(x, y)

        for between in (between_set_fp16, between_set_off, between_lane_query, between_rank_batch):
            # single dense queries take the lanes on the index's own streams only, where single fused queries on a corpus
            # this small would take them too: that case bursts through the candidate entry points, single and grouped
            lanes = between is between_lane_query
            if lanes:
                idx.set_streams(0, 0, 0)
            else:
                dv.own_streams(idx)
            for burst in ((dv.candidates, dv.candidate_groups) if lanes else (dv.fused, dv.candidates)):
                idx.set_dense_prefilter(2)
                one.zero_()
                dv.clear()  # the last sync of the caller's until results()
                burst(idx, a)
                between()
                burst(idx, b)
                got = dv.results(idx)
                which = (0, 1) if burst == dv.fused else (2,)
                _equal([want[j][:96] for j in which], [got[j][:96] for j in which])
                if lanes:
                    assert np.array_equal(one.cpu().numpy(), one_want)


def test_one_query_alone_on_a_fresh_index(data):
    """Nothing of a lone query is deferred to a successor that never comes."""
    dv = _Device(data)
    got = {}
    for mode in (0, 2):
        for entry in ("fused", "candidates"):
            with _index(data) as idx:
                dv.own_streams(idx)
                idx.set_dense_prefilter(mode)
                dv.clear()
                getattr(dv, entry)(idx, [7])
                res = dv.results(idx)
                assert (res[1][7] == TOP_N) if entry == "fused" else (res[2][7, :K, 1] >= 0).all()
                got[mode, entry] = res
    _equal(got[0, "fused"], got[2, "fused"])
    _equal(got[0, "candidates"], got[2, "candidates"])
