"""GPU: the dense prefilter (fp16 shadow scan + exact rescoring, dense_prefilter.hip) answers exactly what the fp32 scan
answers -- the same ids and the same fp32 score bits -- on ordinary and adversarial corpora, and it prunes."""
import numpy as np
import pytest

import prefilter_model as pm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Index():
    from anrag.index import Index

    return Index


def _corpus(n, d, seed=0):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((n, d), dtype=np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    return e, rng


def _planted(e, rng, nq, noise=0.05):
    rows = rng.integers(0, e.shape[0], nq)
    q = e[rows] + noise * rng.standard_normal((nq, e.shape[1]), dtype=np.float32)
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _both(idx, fn):
    idx.set_dense_prefilter(0)
    off = fn()
    idx.set_dense_prefilter(1)
    on = fn()
    return off, on


def _same(off, on):
    for a, b in zip(off, on):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype.kind == "f":
            assert np.array_equal(a.view(np.uint32 if a.itemsize == 4 else np.uint64),
                                  b.view(np.uint32 if b.itemsize == 4 else np.uint64))
        else:
            assert np.array_equal(a, b)


@pytest.mark.parametrize("d,n", [(256, 300_000), (512, 50_000), (768, 60_000), (1024, 50_000), (1536, 20_000),
                                 (2048, 20_000)])
def test_on_off_bit_identical(Index, d, n):
    e, rng = _corpus(n, d, seed=d)
    src = (np.arange(n) % 300).astype(np.uint16)
    allow = np.zeros(300, np.uint8)
    allow[45:] = 1
    with Index(0) as idx:
        idx.dense_load(e, source_id=src)
        for k in (1, 10, 25, 64):
            for nq in (1, 3, 8, 15, 16):  # 15: groups of 8 + 7 (anrag_dense_search's launches)
                q = _planted(e, rng, nq)
                _same(*_both(idx, lambda: idx.dense_search(q, k)))
                _same(*_both(idx, lambda: idx.dense_search(q, k, allow_source=allow)))
        _, survivors = idx.dense_prefilter_stats()
        assert survivors > 0


def test_groups_of_16_and_device_lanes(Index):
    import torch

    e, rng = _corpus(40_000, 768, seed=5)
    q = _planted(e, rng, 16)
    dq = torch.from_numpy(q).cuda()
    with Index(0) as idx:
        idx.dense_load(e)
        res = {}
        for mode in (0, 1, 0, 1):
            idx.set_dense_prefilter(mode)
            out = torch.zeros((16, 25, 2), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            for i in range(16):  # single queries: the lanes, each merge riding in the next launch of its lane
                idx.dense_search_device(dq[i].data_ptr(), 1, 25, None, out[i].data_ptr())
            idx.sync()
            grp = torch.zeros((16, 25, 2), dtype=torch.int64, device="cuda")
            idx.dense_search_device(dq.data_ptr(), 16, 25, None, grp.data_ptr())  # one group of 16
            idx.sync()
            got = (out.cpu().numpy(), grp.cpu().numpy())
            assert np.array_equal(got[0], got[1])
            if mode in res:
                assert np.array_equal(res[mode][0], got[0])
            res[mode] = got
        assert np.array_equal(res[0][0], res[1][0])


def test_hybrid_on_off_identical(Index):
    from anrag.bm25_index import Bm25Index

    n, d, vocab = 50_000, 768, 300
    e, rng = _corpus(n, d, seed=11)
    p = 1.0 / np.arange(1, vocab + 1) ** 1.07
    p /= p.sum()
    corpus = [[f"t{j}" for j in rng.choice(vocab, size=int(rng.integers(5, 30)), p=p)] for _ in range(n)]
    bi = Bm25Index(corpus, k1=1.7, b=0.83, epsilon=0.05)
    q = _planted(e, rng, 6)
    terms = [bi.term_ids([str(t) for t in rng.choice(corpus[i * 97], size=4)]) for i in range(6)]
    with Index(0) as idx:
        idx.dense_load(e)
        idx.bm25_load(bi.indptr, bi.post_doc, bi.post_tf, bi.idf, bi.doc_len, bi.avgdl, bi.k1, bi.b)
        single = lambda: [idx.hybrid_search(q[i], terms[i], 25, 5.0, 1.0, 40, 10) for i in range(6)]
        off, on = _both(idx, single)
        for a, b in zip(off, on):
            _same(a, b)
        _same(*_both(idx, lambda: idx.hybrid_search_batch(q, terms, 25, 5.0, 1.0, 40, 10)))


def test_adversarial_rows(Index):
    n, d, k = 50_000, 256, 25
    e, rng = _corpus(n, d, seed=3)
    q = _planted(e, rng, 1)[0]
    s = e @ q
    kth = int(np.argsort(-s)[k - 1])
    e[100:140] = e[kth]                            # many copies of the row at the k-th place
    for i in range(8):                             # rows 1 ulp apart around it
        r = e[kth].copy()
        r[i] = np.nextafter(r[i], np.float32(np.inf) if i % 2 else np.float32(-np.inf))
        e[200 + i] = r
    e[300] = e[kth] * 1e5                          # past fp16's 65504
    e[301] = e[kth] * 1e-6                         # into fp16's subnormal range
    e[302] = e[kth] * 1e-9                         # below it
    e[303, 7] = np.nan                             # a NaN row (ranks first, as +inf)
    e[304, 3] = np.inf
    e[305, 9] = -np.inf
    # rows whose fp32 score sits at an end of the interval (prefilter_model.py), k + 3 of them with fp16 values of their
    # own and the highest scores of the corpus: the k-th place falls among them, so losing one changes the answer
    q_sat = pm.sat_fp16_row(d, np.random.default_rng(d))[0]
    for i in range(k + 3):
        e[400 + i] = pm.sat_fp16_row(d, rng, side=1 if i % 2 else -1, aligned=True, sign=np.sign(q_sat))[1]
    with Index(0) as idx:
        idx.dense_load(e)
        for qq in (q, -q, np.zeros(d, np.float32), np.full(d, np.nan, np.float32), q * 1e30, q_sat, -q_sat):
            for kk in (1, k, 64):
                _same(*_both(idx, lambda: idx.dense_search(qq, kk)))
        allow = np.zeros(2, np.uint8)
        allow[1] = 1
        src = np.zeros(n, np.uint16)
        src[[5, 77, 4000]] = 1                     # fewer allowed rows than k
        idx.dense_load(e, source_id=src)
        _same(*_both(idx, lambda: idx.dense_search(q, k, allow_source=allow)))


def test_all_identical_and_tiny_corpora(Index):
    row = _corpus(1, 512, seed=9)[0]
    e = np.repeat(row, 60_000, axis=0)             # every row survives
    q = row[0] + 0.01
    with Index(0) as idx:
        idx.dense_load(e)
        _same(*_both(idx, lambda: idx.dense_search(q, 64)))
        small, rng = _corpus(10, 256, seed=2)          # n_rows < k
        idx.dense_load(small)
        qs = _planted(small, rng, 2)
        _same(*_both(idx, lambda: idx.dense_search(qs, 25)))


def test_prunes_to_a_few_rows_per_query(Index):
    n, d, k = 300_000, 768, 25
    e, rng = _corpus(n, d, seed=21)
    q = _planted(e, rng, 32)
    with Index(0) as idx:
        idx.dense_load(e)
        idx.set_dense_prefilter(1)
        q0, s0 = idx.dense_prefilter_stats()
        for i in range(32):
            idx.dense_search(q[i], k)
        q1, s1 = idx.dense_prefilter_stats()
        assert q1 - q0 == 32
        assert (s1 - s0) / 32 <= 4 * k, (s1 - s0) / 32


def test_mode_switching_memory_and_auto(Index):
    import torch

    n, d = 100_000, 512
    e, rng = _corpus(n, d, seed=4)
    q = _planted(e, rng, 4)
    with Index(0) as idx:
        idx.set_dense_prefilter(0)
        idx.dense_load(e)
        base = idx.info()["hbm_bytes"]
        ref = idx.dense_search(q, 25)
        idx.set_dense_prefilter(1)
        grown = idx.info()["hbm_bytes"] - base
        assert grown >= n * (2 * d + 4) + 32 * n * 4
        _same(ref, idx.dense_search(q, 25))
        idx.set_dense_prefilter(0)
        _same(ref, idx.dense_search(q, 25))
        idx.set_dense_prefilter(1)
        _same(ref, idx.dense_search(q, 25))
        assert idx.info()["hbm_bytes"] - base == grown
        idx.set_dense_prefilter(-1)
        idx.dense_load(e)  # a reload drops the copy; auto stays off at 200 MB
        assert idx.info()["hbm_bytes"] == base
    # auto: on past 1 GiB of fp32 corpus (1M x 768)
    big = torch.randn(1_000_000, 768, device="cuda", dtype=torch.float32)
    big /= big.norm(dim=1, keepdim=True)
    torch.cuda.synchronize()
    with Index(0) as idx:
        idx.dense_load((big.data_ptr(), 1_000_000, 768))
        qb = big[12345].cpu().numpy()
        doc, _, _ = idx.dense_search(qb, 10)
        assert doc[0, 0] == 12345
        assert idx.dense_prefilter_stats()[0] == 1
