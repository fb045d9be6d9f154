"""GPU: the global tail of the row-sharded path -- `anrag_merge_candidates_device`, `anrag_merge_fuse_device`,
`anrag_wrrf_device` (select.hip, wrrf_block.hpp) -- against the host model tests/shard_merge_model.py on the planted
inputs that tests/test_shard_merge_model_cpu.py holds to what they claim, and the tail end to end at 2, 3 and 8 shards on
one GPU against the single index.  Everything is exact: ids, score bits as int64, counts, and the sentinel records behind
a query's count.

Stream discipline: torch fills and copies on ITS stream, the library reads and writes on the index's own streams, so
`torch.cuda.synchronize()` stands between a torch fill and a library call, and `Index.sync()` before results are read."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import shard_merge_model as m

pytestmark = pytest.mark.gpu

SENT = np.array([m.bits([m.SENTINEL[0]])[0], m.SENTINEL[1]], np.int64)
REC = 16  # bytes of a record


class Gpu:
    def __init__(self):
        import torch

        from anrag import _native as nat
        from anrag.index import Index

        self.torch, self.nat, self.lib = torch, nat, nat.load_library()
        self.dev = torch.device("cuda:0")
        self.util = Index(0)  # data-less: the helper index the tail kernels run on

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def sentinel(self, *shape):
        return self.up(np.broadcast_to(SENT, shape + (2,)))

    def counts(self, n):
        return self.torch.full((n,), -99, dtype=self.torch.int32, device=self.dev)

    def merge_fuse(self, ptr, n_lists, k, stride, wd, wb, wk, top_n, nq):
        out, count = self.sentinel(nq, top_n), self.counts(nq)
        self.torch.cuda.synchronize()
        self.nat.check(self.lib.anrag_merge_fuse_device(self.util.handle, ptr, n_lists, k, stride, wd, wb, wk, top_n, nq,
                                                        out.data_ptr(), count.data_ptr()))
        self.util.sync()
        return out.cpu().numpy(), count.cpu().numpy()


@pytest.fixture(scope="module")
def gpu():
    g = Gpu()
    yield g
    g.util.close()


def expected(want, top_n):
    """The model's (ids, score bits, counts) as the output buffer has to look: sentinel records behind the count."""
    ids, sbits, counts = want
    exp = np.broadcast_to(SENT, (len(counts), top_n, 2)).copy()
    for q, c in enumerate(counts):
        exp[q, :c, 0] = sbits[q, :c]
        exp[q, :c, 1] = ids[q, :c]
    return exp


def assert_fused(got, count, want, top_n, what, names=None):
    exp = expected(want, top_n)
    assert count.tolist() == want[2].tolist(), what
    for q in range(len(count)):
        assert np.array_equal(got[q], exp[q]), (what, q, names[q] if names else None, got[q, :4].tolist(), exp[q, :4].tolist())


# --------------------------------------------------------------------------- the planted launches
@pytest.mark.parametrize("p", range(len(m.PACKS)), ids=[f"k{k}-lists{n}" for k, n in m.PACKS])
def test_merge_fuse_and_merge_on_the_planted_queries(gpu, p):
    """Every planted query of one (k, n_lists) as the queries of ONE launch, inside a buffer that is poison -- (+inf, doc 7)
    -- in front of the first slab, behind every slab's payload and nowhere else; three launches: every weight set, top_n
    rotating through {1, 10, 2k, 128}.  Then `anrag_merge_candidates_device` on single halves of the same buffer."""
    k, n_lists = m.PACKS[p]
    cases = m.cases_for(k, n_lists)
    names = [c["name"] for c in cases]
    nq = len(cases)
    buf, stride, lead = m.slab(cases, k, n_lists, m.pack_extra(p))
    assert stride > nq * 2 * k
    rec = buf[lead:]
    d_buf = gpu.up(buf)
    ptr = d_buf.data_ptr() + lead * REC
    for wd, wb, wk, top_n in m.pack_launches(p, k):
        got, count = gpu.merge_fuse(ptr, n_lists, k, stride, wd, wb, wk, top_n, nq)
        want = m.merge_fuse(rec, n_lists, k, stride, wd, wb, wk, top_n, nq)
        assert_fused(got, count, want, top_n, (k, n_lists, wd, wb, wk, top_n), names)
        assert 7 not in got[:, :, 1]
        for q, c in enumerate(cases):
            if "same_as" in c:  # the lists permuted: the same answer, bit for bit
                assert np.array_equal(got[q], got[c["same_as"]]), c["name"]
        assert count[names.index("empty")] == 0
    # n_queries in {1, 3, 8}: the first queries of the same slabs (the other blocks are then data that must not be read)
    for n in (1, 3, 8):
        wd, wb, wk = m.WEIGHTS[0]
        got, count = gpu.merge_fuse(ptr, n_lists, k, stride, wd, wb, wk, 10, n)
        assert_fused(got, count, m.merge_fuse(rec, n_lists, k, stride, wd, wb, wk, 10, n), 10, (k, n_lists, "n_queries", n), names)
    # the merge alone, on one half of one query per call
    picked = ("distinct0", "distinct_big", "ties0", "ties1_reversed", "ties2_permuted", "short0", "short1", "empty", "few", "last")
    picks = [(q, i % 2) for i, q in enumerate(q for q, c in enumerate(cases) if c["name"] in picked)]
    picks += [(names.index(name), h) for name in ("one_each", "no_bm25") for h in range(2)]
    out = gpu.sentinel(len(picks), k + 1)  # a sentinel record behind every k that are written
    gpu.torch.cuda.synchronize()
    for i, (q, h) in enumerate(picks):
        gpu.nat.check(gpu.lib.anrag_merge_candidates_device(gpu.util.handle, ptr + (q * 2 * k + h * k) * REC, n_lists, k, stride,
                                                            out[i].data_ptr()))
    gpu.util.sync()
    got = out.cpu().numpy()
    for i, (q, h) in enumerate(picks):
        want = m.merge(rec, n_lists, k, stride, q * 2 * k + h * k)
        assert np.array_equal(got[i, :k], want), (k, n_lists, names[q], h, got[i, :4].tolist(), want[:4].tolist())
        assert np.array_equal(got[i, k], SENT)


def test_merge_fuse_stride_equal_to_the_payload(gpu):
    """What the searcher passes: list_stride = group * 2k exactly, nothing between the slabs."""
    k, n_lists = 25, 3
    cases = m.cases_for(k, n_lists, seed=9)
    buf, stride, lead = m.slab(cases, k, n_lists, 0, lead=0)
    assert stride == len(cases) * 2 * k
    d_buf = gpu.up(buf)
    got, count = gpu.merge_fuse(d_buf.data_ptr(), n_lists, k, stride, 5.0, 1.0, 40.0, 10, len(cases))
    assert_fused(got, count, m.merge_fuse(buf, n_lists, k, stride, 5.0, 1.0, 40.0, 10, len(cases)), 10, "tight")


def test_wrrf_device_against_the_model(gpu):
    """anrag_wrrf_device up to its 1,024 entries: padding records in the middle of both lists, docs shared between them."""
    for i, c in enumerate(m.wrrf_device_cases()):
        nd, nb = c["n_dense"], c["n_bm25"]
        d_dense, d_bm25 = gpu.up(c["dense"]), (gpu.up(c["bm25"]) if nb else None)
        lists = [c["dense"][:, 1].tolist(), c["bm25"][:, 1].tolist()]
        for (wd, wb, wk), top_n in ((m.WEIGHTS[0], 10), (m.WEIGHTS[1], nd + nb), (m.WEIGHTS[2], 1)):
            out, count = gpu.sentinel(top_n + 1), gpu.counts(1)
            gpu.torch.cuda.synchronize()
            gpu.nat.check(gpu.lib.anrag_wrrf_device(gpu.util.handle, d_dense.data_ptr(), nd, d_bm25.data_ptr() if nb else None,
                                                    nb, wd, wb, wk, top_n, out.data_ptr(), count.data_ptr()))
            gpu.util.sync()
            ids, sbits, cnt = m.fused_out(m.wrrf_padded(lists, [wd, wb], wk), top_n)
            exp = expected((ids[None], sbits[None], np.array([cnt])), top_n + 1)[0]
            got = out.cpu().numpy()
            assert int(count.cpu()[0]) == cnt, (nd, nb, top_n)
            assert np.array_equal(got, exp), (nd, nb, top_n, got[:4].tolist(), exp[:4].tolist())
            assert (got[:cnt, 1] >= 0).all()


# --------------------------------------------------------------------------- the distributed tail on one GPU
W = (5.0, 1.0, 40.0)
GROUP = 3


def cut_postings(c, lo, hi):
    """The shard-local CSR of documents [lo, hi): the global postings inside the block, rebased."""
    term_of = np.repeat(np.arange(c["vocab"]), np.diff(c["indptr"]))
    keep = (c["post_doc"] >= lo) & (c["post_doc"] < hi)
    indptr = np.zeros(c["vocab"] + 1, np.int64)
    np.cumsum(np.bincount(term_of[keep], minlength=c["vocab"]), out=indptr[1:])
    return indptr, (c["post_doc"][keep] - lo).astype(np.int32), c["post_tf"][keep]


def load_shards(stack, c, S):
    """S indexes with contiguous row blocks, shard-local postings, GLOBAL idf / avgdl and doc_id_base = lo."""
    from anrag.index import Index
    from anrag.sharded import shard_bounds

    shards = []
    for r in range(S):
        lo, hi = shard_bounds(c["n"], S, r)
        ix = stack.enter_context(Index(0))
        ix.dense_load(c["E"][lo:hi], source_id=c["src"][lo:hi], doc_id_base=lo)
        indptr, post_doc, post_tf = cut_postings(c, lo, hi)
        ix.bm25_load(indptr, post_doc, post_tf, c["idf"], c["doc_len"][lo:hi], c["avgdl"], 1.7, 0.83,
                     source_id=c["src"][lo:hi], doc_id_base=lo)
        shards.append(ix)
    return shards


def load_single(stack, c):
    from anrag.index import Index
    from test_gpu_shard_group import load

    return load(stack.enter_context(Index(0)), c)


def allow_bitmap(gpu, allow):
    """One byte per source id -> the 2,048-word device bitmap of the *_device entry points."""
    bits = np.zeros(65536, np.uint8)
    bits[: len(allow)] = np.asarray(allow) != 0
    return gpu.up(np.packbits(bits, bitorder="little").view(np.int32).copy())


def run_tail(gpu, shards, Q, terms, k, top_n, allow=None):
    """What a rank does per exchange group, for every rank at once: each shard's legs straight into its slab of the
    [S, GROUP, 2k, 2] receive buffer (`anrag_hybrid_candidates_group_device`), then ONE `anrag_merge_fuse_device`.
    -> (receive buffers [groups, S, GROUP, 2k, 2], out [groups, GROUP, top_n, 2], counts [groups, GROUP])."""
    torch, S, nq = gpu.torch, len(shards), len(Q)
    n_groups = -(-nq // GROUP)
    d_q = gpu.up(np.ascontiguousarray(Q, dtype=np.float32))
    T = np.zeros((nq, 16), np.int32)
    for i, t in enumerate(terms):
        T[i, : len(t)] = t
    d_t = gpu.up(T)
    recv = torch.zeros((n_groups, S, GROUP, 2 * k, 2), dtype=torch.int64, device=gpu.dev)
    out, count = gpu.sentinel(n_groups, GROUP, top_n), gpu.counts(n_groups * GROUP).view(n_groups, GROUP)
    d_allow = None if allow is None else allow_bitmap(gpu, allow)
    p_allow = None if allow is None else d_allow.data_ptr()
    torch.cuda.synchronize()
    for gi in range(n_groups):
        qs = list(range(gi * GROUP, min(nq, (gi + 1) * GROUP)))
        n = len(qs)
        ptrs = lambda addrs: (C.c_void_p * n)(*addrs)
        for s, sh in enumerate(shards):
            gpu.nat.check(gpu.lib.anrag_hybrid_candidates_group_device(
                sh.handle, ptrs([d_q[i].data_ptr() for i in qs]), ptrs([d_t[i].data_ptr() for i in qs]),
                (C.c_int32 * n)(*[len(terms[i]) for i in qs]), n, k, p_allow, p_allow,
                ptrs([recv[gi, s, j].data_ptr() for j in range(n)])))
        for sh in shards:
            sh.sync()
        gpu.nat.check(gpu.lib.anrag_merge_fuse_device(gpu.util.handle, recv[gi].data_ptr(), S, k, GROUP * 2 * k, W[0], W[1], W[2],
                                                      top_n, n, out[gi].data_ptr(), count[gi].data_ptr()))
        gpu.util.sync()
    return recv.cpu().numpy(), out.cpu().numpy(), count.cpu().numpy()


def check_tail(gpu, single, shards, Q, terms, k, top_n, allow=None, what=None):
    S, nq = len(shards), len(Q)
    recv, out, count = run_tail(gpu, shards, Q, terms, k, top_n, allow)
    for gi in range(recv.shape[0]):
        n = min(GROUP, nq - gi * GROUP)
        # the legs' lists are what the merge requires, and the merge + fusion of exactly these records is the model's:
        # a wrong answer below is then a wrong leg, not a wrong merge
        m.check_contract(recv[gi], S, k, GROUP * 2 * k, [q * 2 * k + h * k for q in range(n) for h in range(2)])
        want = m.merge_fuse(recv[gi], S, k, GROUP * 2 * k, W[0], W[1], W[2], top_n, n)
        assert_fused(out[gi, :n], count[gi, :n], want, top_n, (what, S, k, "model", gi))
        assert (out[gi, n:] == SENT).all() and (count[gi, n:] == -99).all()
        for j in range(n):
            i = gi * GROUP + j
            ids, scores = single.hybrid_search(Q[i], terms[i], k, W[0], W[1], W[2], top_n, allow, allow)
            c = int(count[gi, j])
            assert c == len(ids), (what, S, k, i)
            assert out[gi, j, :c, 1].tolist() == ids.tolist(), (what, S, k, i)
            assert out[gi, j, :c, 0].tolist() == m.bits(scores).tolist(), (what, S, k, i)
    return recv, out, count


def tail_world(n, seed=20263):
    """make_corpus with dense rows duplicated across every shard cut of S = 2, 3, 8, and 13 queries: random hybrid ones,
    the duplicated rows with one rare term each (the BM25 list is cut inside the run of zero scores), one without terms."""
    from anrag.sharded import shard_bounds
    from test_gpu_shard_group import make_corpus, make_queries

    c = make_corpus(n, 128, seed, vocab=3000 if n > 500 else 400)
    cuts = sorted({shard_bounds(n, S, r)[0] for S in (2, 3, 8) for r in range(1, S)})
    for b in cuts:
        c["E"][b] = c["E"][b - 1]
    df = np.diff(c["indptr"])
    rng = np.random.default_rng(seed)
    rare = rng.choice(np.nonzero((df >= 1) & (df <= 6))[0], size=6, replace=False)
    Qr, tr = make_queries(c, 6, seed)
    Q = np.concatenate([Qr[:4], c["E"][cuts][:6], Qr[4:5], c["E"][cuts[-1:]], Qr[5:6]]).astype(np.float32)
    terms = tr[:4] + [np.array([t], np.int32) for t in rare] + [np.zeros(0, np.int32), tr[4], tr[5]]
    assert len(Q) == len(terms) == 13
    return c, Q, terms, list(range(4, 10))


@pytest.fixture(scope="module")
def world():
    c, Q, terms, rare_q = tail_world(1003)
    with contextlib.ExitStack() as stack:
        yield dict(c=c, Q=Q, terms=terms, rare_q=rare_q, single=load_single(stack, c))


@pytest.mark.parametrize("S", [2, 3, 8])
def test_tail_equals_the_single_index(gpu, world, S):
    """n = 1003, d = 128, groups of 3 (the last group partial): k = 25 / top 10, then k = 64 and k = 1."""
    c, Q, terms, single = world["c"], world["Q"], world["terms"], world["single"]
    for i in world["rare_q"]:
        doc, score, cnt = single.bm25_search(terms[i], 25)
        assert cnt == 25 and score[24] == 0.0 and score[0] > 0.0  # cut inside the run of zero scores
    with contextlib.ExitStack() as stack:
        shards = load_shards(stack, c, S)
        recv, out, count = check_tail(gpu, single, shards, Q, terms, 25, 10, what="plain")
        assert (count.reshape(-1)[:13] == 10).all()
        tied = 0  # a duplicated row on both sides of a cut of THIS S: two shards lead their dense lists with equal scores
        for i in world["rare_q"]:
            best = np.sort(recv[i // GROUP, :, i % GROUP, 0, 0].copy().view(np.float64))
            tied += best[-1] == best[-2]
        assert tied >= 1
        check_tail(gpu, single, shards, Q, terms, 64, 10, what="k64")
        check_tail(gpu, single, shards, Q, terms, 64, 128, what="k64 top 128")
        check_tail(gpu, single, shards, Q, terms, 1, 10, what="k1")


@pytest.mark.parametrize("S", [2, 3, 8])
def test_tail_with_a_filter_that_empties_a_shard(gpu, world, S):
    """Source = a function of the row block: one filter leaves shard 0 without a candidate, one leaves only shard 0."""
    from anrag.sharded import shard_bounds

    src = np.zeros(world["c"]["n"], np.uint16)
    src[shard_bounds(world["c"]["n"], S, 1)[0]:] = 1
    c = dict(world["c"], src=src, n_sources=2)
    with contextlib.ExitStack() as stack:
        single = load_single(stack, c)
        shards = load_shards(stack, c, S)
        for allow in (np.array([0, 1], np.uint8), np.array([1, 0], np.uint8)):
            _, out, count = check_tail(gpu, single, shards, world["Q"], world["terms"], 25, 10, allow, what=allow.tolist())
            docs = out[:, :, :, 1].reshape(-1, 10)[:13]
            lo1 = shard_bounds(c["n"], S, 1)[0]
            assert ((docs >= lo1) if allow[1] else (docs < lo1)).all()


def test_tail_with_every_list_short(gpu):
    """n = 150 over 8 shards: 18 or 19 rows each, fewer than k = 25, so every list of every query ends in padding."""
    c, Q, terms, _ = tail_world(150, seed=20264)
    with contextlib.ExitStack() as stack:
        single = load_single(stack, c)
        shards = load_shards(stack, c, 8)
        recv, _, _ = run_tail(gpu, shards, Q[:3], terms[:3], 25, 10)
        assert (recv[0, :, :, 19:25, 1] == -1).all() and (recv[0, :, :, 44:50, 1] == -1).all() and (recv[0, :, :, 0, 1] >= 0).all()
        check_tail(gpu, single, shards, Q, terms, 25, 10, what="short")
        check_tail(gpu, single, shards, Q, terms, 25, 50, what="short top 50")
