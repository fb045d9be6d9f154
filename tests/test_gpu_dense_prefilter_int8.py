"""The int8 form of the dense prefilter (mode 2, K1F8 in dense_prefilter.hip) answers exactly what the fp32 scan answers
-- the same ids and the same fp32 score bits -- on ordinary and adversarial corpora, and it prunes.  The code-object
check at the end needs no GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import prefilter_model as pm
from test_build_resources import CSRC, LLVM, _kernels

gpu = pytest.mark.gpu


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
    idx.set_dense_prefilter(2)
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


@gpu
@pytest.mark.parametrize("d,n", [(256, 200_000), (512, 50_000), (768, 60_000), (1024, 50_000), (1536, 20_000),
                                 (2048, 20_000)])
def test_int8_matches_fp32_scan(Index, d, n):
    e, rng = _corpus(n, d, seed=d + 1)
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
        queries, survivors = idx.dense_prefilter_stats()
        assert queries > 0 and survivors > 0


@gpu
def test_int8_device_lanes_and_groups(Index):
    import torch

    e, rng = _corpus(40_000, 768, seed=6)
    q = _planted(e, rng, 16)
    dq = torch.from_numpy(q).cuda()
    with Index(0) as idx:
        idx.dense_load(e)
        res = {}
        for mode in (0, 2, 0, 2):
            idx.set_dense_prefilter(mode)
            out = torch.zeros((16, 25, 2), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            for i in range(16):  # single queries: the lanes
                idx.dense_search_device(dq[i].data_ptr(), 1, 25, None, out[i].data_ptr())
            idx.sync()
            grp = torch.zeros((16, 25, 2), dtype=torch.int64, device="cuda")
            idx.dense_search_device(dq.data_ptr(), 16, 25, None, grp.data_ptr())
            idx.sync()
            got = (out.cpu().numpy(), grp.cpu().numpy())
            assert np.array_equal(got[0], got[1])
            if mode in res:
                assert np.array_equal(res[mode][0], got[0])
            res[mode] = got
        assert np.array_equal(res[0][0], res[2][0])


@gpu
def test_int8_hybrid_single_and_batch(Index):
    from anrag.bm25_index import Bm25Index

    n, d, vocab = 50_000, 768, 300
    e, rng = _corpus(n, d, seed=12)
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


@gpu
def test_int8_adversarial_rows(Index):
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
    e[300] = e[kth] * 1e5
    e[301] = e[kth] * 1e-6
    e[302] = e[kth] * 1e-9
    e[303, 7] = np.nan                             # a NaN row (ranks first, as +inf)
    e[304, 3] = np.inf
    e[305, 9] = -np.inf
    e[306] = e[kth] * 1e-40                        # subnormal components: the scale itself is subnormal
    e[307] = e[kth]
    e[307, 0] = 1e4                                # one dominant component: a coarse scale
    e[308] = e[kth] * 0.01
    e[308, 5] = 30.0
    e[309:320] = 0.0                               # all-zero rows
    e[320] = e[kth] * 1e25                         # past the 2^60 cap of the radius
    # rows whose fp32 score sits at an end of the interval (prefilter_model.py), k + 3 of them with codes of their own
    # and the highest scores of the corpus: the k-th place falls among them, so losing one changes the answer; and the
    # pair of rows that saturates the query term of the radius
    q_sat = pm.sat_i8_row(d, np.random.default_rng(d))[0]
    for i in range(k + 3):
        e[400 + i] = pm.sat_i8_row(d, rng, side=1 if i % 2 else -1, aligned=True, sign=np.sign(q_sat))[1]
    q_qt, e_qt = pm.sat_i8_query(d, np.random.default_rng(d + 1))
    e[440], e[441] = e_qt, -e_qt
    with Index(0) as idx:
        idx.dense_load(e)
        for qq in (q, -q, np.zeros(d, np.float32), np.full(d, np.nan, np.float32), q * 1e30, q * 1e-30, q_sat, -q_sat,
                   q_qt, -q_qt):
            for kk in (1, k, 64):
                _same(*_both(idx, lambda: idx.dense_search(qq, kk)))
        spiky = q.copy()
        spiky[3] = 50.0                            # a query dominated by one component
        _same(*_both(idx, lambda: idx.dense_search(spiky, k)))
        allow = np.zeros(2, np.uint8)
        allow[1] = 1
        src = np.zeros(n, np.uint16)
        src[[5, 77, 4000]] = 1                     # fewer allowed rows than k
        idx.dense_load(e, source_id=src)
        _same(*_both(idx, lambda: idx.dense_search(q, k, allow_source=allow)))


@gpu
def test_int8_all_identical_and_tiny_corpora(Index):
    row = _corpus(1, 512, seed=9)[0]
    e = np.repeat(row, 60_000, axis=0)             # every row survives
    q = row[0] + 0.01
    with Index(0) as idx:
        idx.dense_load(e)
        _same(*_both(idx, lambda: idx.dense_search(q, 64)))
        small, rng = _corpus(10, 256, seed=2)      # n_rows < k
        idx.dense_load(small)
        qs = _planted(small, rng, 2)
        _same(*_both(idx, lambda: idx.dense_search(qs, 25)))


# Mean survivors per query on this corpus: 533 measured on MI355X (DESIGN.md "K1F8"); the bound keeps a 2x margin.
_SURVIVOR_BOUND = 1_100


@gpu
def test_int8_prunes(Index):
    n, d, k = 300_000, 768, 25
    e, rng = _corpus(n, d, seed=21)
    q = _planted(e, rng, 32)
    with Index(0) as idx:
        idx.dense_load(e)
        idx.set_dense_prefilter(2)
        q0, s0 = idx.dense_prefilter_stats()
        for i in range(32):
            idx.dense_search(q[i], k)
        q1, s1 = idx.dense_prefilter_stats()
        assert q1 - q0 == 32
        mean = (s1 - s0) / 32
        print(f"int8 prefilter: {mean:.1f} survivors per query")
        assert mean <= _SURVIVOR_BOUND, mean


@gpu
def test_int8_mode_memory_and_switching(Index):
    n, d = 100_000, 512
    e, rng = _corpus(n, d, seed=4)
    q = _planted(e, rng, 4)
    with Index(0) as idx:
        idx.set_dense_prefilter(0)
        idx.dense_load(e)
        base = idx.info()["hbm_bytes"]
        ref = idx.dense_search(q, 25)
        idx.set_dense_prefilter(2)
        grown8 = idx.info()["hbm_bytes"] - base
        assert n * (d + 16) + 32 * n * 4 <= grown8 < n * (2 * d + 4) + 32 * n * 4
        _same(ref, idx.dense_search(q, 25))
        idx.set_dense_prefilter(1)                 # the fp16 form replaces the int8 block
        grown16 = idx.info()["hbm_bytes"] - base
        assert grown16 >= n * (2 * d + 4) + 32 * n * 4
        _same(ref, idx.dense_search(q, 25))
        idx.set_dense_prefilter(2)
        assert idx.info()["hbm_bytes"] - base == grown8
        _same(ref, idx.dense_search(q, 25))
        with pytest.raises(Exception):
            idx.set_dense_prefilter(3)


def _scan_kernel_vgprs():
    objs = [os.path.join(CSRC, "dense_prefilter.o")]
    if not os.path.exists(objs[0]):
        subprocess.run(["make", "-C", CSRC, "-j", "8"], check=True, capture_output=True)
    import tempfile

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k in _kernels(objs[0], tmp):
            name = subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip() \
                if shutil.which("c++filt") else k["name"]
            if "i8_scan_kernel" in name:
                out[name] = k
    return out


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="needs the ROCm LLVM tools")
def test_int8_scan_kernels_fit_beside_k3():
    ks = _scan_kernel_vgprs()
    assert len(ks) == 12, sorted(ks)  # six dimensions, with and without the source filter
    for name, k in ks.items():
        assert int(k["vgpr_count"]) <= 128, f"{name}: {k['vgpr_count']} VGPRs"
        assert int(k.get("vgpr_spill_count", 0)) == 0, name
        assert int(k.get("private_segment_fixed_size", 0)) == 0, name
