"""CPU: the host model of the sharded path's global tail (tests/shard_merge_model.py) and the inputs planted for it.

1. The model equals the restatement `OracleShardEngine.merge_fuse` used to carry, on the gloo test's own data.
2. Every planted family is inside the kernels' input contract, and the model, the literal walk of the kernel and -- for a
   permutation of the lists -- the unpermuted case agree on it.
3. Every planted family separates the right answer from the wrong ones it is there to catch: conditions on the INPUTS, so
   that tests/test_gpu_shard_merge.py cannot pass on inputs that would not notice the fault.
4. The documented limitation (equal scores, doc ids not ascending inside a list) as an executable example.
"""
import numpy as np
import pytest

import shard_merge_model as m

A = m.WEIGHTS[0]


# --------------------------------------------------------------------------- 1. the gloo test's restatement
def _restatement(rec, n_lists, k, stride, w_dense, w_bm25, wrrf_k, top_n, n_queries):
    """What tests/test_sharded_gloo.py's OracleShardEngine.merge_fuse was before it called the model."""
    from oracle import ref_search

    rec = rec.reshape(-1, 2)
    out = []
    for q in range(n_queries):
        merged = []
        for leg in range(2):
            cands = []
            for l in range(n_lists):
                base = l * stride + q * 2 * k + leg * k
                for r in rec[base: base + k]:
                    if r[1] >= 0:
                        cands.append((float(np.int64(r[0]).view(np.float64)), int(r[1])))
            cands.sort(key=lambda c: (-c[0], c[1]))
            merged.append([c[1] for c in cands[:k]])
        fused = ref_search.weighted_reciprocal_rank_fusion(
            [(merged[0], "d"), (merged[1], "b")], {"d": w_dense, "b": w_bm25}, int(wrrf_k))[:top_n]
        out.append(([i for i, _ in fused], [s for _, s in fused]))
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_model_equals_the_gloo_restatement(world):
    import torch

    from anrag.sharded import shard_bounds
    from oracle.make_golden import synth_chunks, synth_dense, synth_query
    from oracle.ref_bm25 import CsrBM25
    from test_sharded_gloo import OracleShardEngine

    n, d, k, top_n, group = 301, 32, 25, 10, 5
    chunks = [c for c in synth_chunks(n + 20, 5) if c["tokens"]][:n]
    corpus = [c["tokens"] for c in chunks]
    e = synth_dense(n, d, 6)
    glob = CsrBM25(corpus, k1=1.7, b=0.83, epsilon=0.05)
    sid = (np.arange(n) * 7 % 5).astype(np.int64)
    rng = np.random.default_rng(11)
    recv = torch.zeros(world, group, 2 * k, 2, dtype=torch.int64)
    engines = []
    for r in range(world):
        lo, hi = shard_bounds(n, world, r)
        engines.append(OracleShardEngine(e[lo:hi], lo, glob, corpus[lo:hi], sid[lo:hi]))
    for trial in range(group):
        target = int(rng.integers(n))
        q = synth_query(e, 100 + trial, target)
        toks = [str(t) for t in rng.choice(corpus[target], size=4)] if trial != 2 else []
        terms = np.array(glob.term_ids(toks), dtype=np.int32)
        for r, eng in enumerate(engines):
            eng.legs(torch.from_numpy(q), torch.from_numpy(np.resize(terms, max(len(terms), 1))), len(terms), k, recv[r, trial])
    rec = recv.numpy()
    stride = group * 2 * k
    m.check_contract(rec, world, k, stride, [q * 2 * k + h * k for q in range(group) for h in range(2)])
    for wd, wb, wk, tn in ((5.0, 1.0, 40.0, top_n), (1.0, 1.0, 60.0, 2 * k), (5.0, 0.0, 40.0, 128)):
        want = _restatement(rec, world, k, stride, wd, wb, wk, tn, group)
        ids, sbits, counts = m.merge_fuse(rec, world, k, stride, wd, wb, wk, tn, group)
        for q in range(group):
            c = int(counts[q])
            assert c == len(want[q][0]) and ids[q, :c].tolist() == want[q][0]
            assert sbits[q, :c].tolist() == m.bits(want[q][1]).tolist()
            assert (ids[q, c:] == -1).all() and (sbits[q, c:] == m.NEG_INF_BITS).all()
        # and through the engine itself, which now calls the model
        out = torch.zeros(group, tn, 2, dtype=torch.int64)
        count = torch.zeros(group, dtype=torch.int32)
        engines[0].merge_fuse(recv, world, k, stride, wd, wb, wk, tn, group, out, count)
        assert count.tolist() == counts.tolist() and np.array_equal(out.numpy()[:, :, 1], ids)
        assert np.array_equal(out.numpy()[:, :, 0], sbits)


# --------------------------------------------------------------------------- 2. contract
def _offsets(nq, k):
    return [q * 2 * k + h * k for q in range(nq) for h in range(2)]


@pytest.mark.parametrize("k,n_lists", m.PACKS)
def test_planted_families_are_in_contract(k, n_lists):
    cases = m.cases_for(k, n_lists)
    assert {c["family"] for c in cases} == {"distinct", "ties", "short", "both", "disjoint", "no_bm25"}
    buf, stride, lead = m.slab(cases, k, n_lists, 19)
    rec = buf[lead:]
    m.check_contract(rec, n_lists, k, stride, _offsets(len(cases), k))
    merged = [[m.merge(rec, n_lists, k, stride, q * 2 * k + h * k) for h in range(2)] for q in range(len(cases))]
    for q, c in enumerate(cases):
        for h in range(2):
            # under the contract the kernel's short walk is the sort
            assert np.array_equal(m.kernel_walk(rec, n_lists, k, stride, q * 2 * k + h * k), merged[q][h]), (c["name"], h)
            assert 7 not in merged[q][h][:, 1]
            if "same_as" in c:  # the merge is keyed on the doc id, not on the position of the list
                assert np.array_equal(merged[q][h], merged[c["same_as"]][h]), c["name"]
        docs = [set(merged[q][h][:, 1].tolist()) - {-1} for h in range(2)]
        if c["family"] == "both":
            assert docs[0] & docs[1]
        if c["family"] == "disjoint":
            assert not docs[0] & docs[1] and len(docs[0]) == len(docs[1]) == k
        if c["name"] == "empty":
            assert not docs[0] and not docs[1]
        if c["name"] == "few":
            assert len(docs[0]) == len(docs[1]) == k - 1
        if c["name"] == "last":
            assert all(d >= 100 + (n_lists - 1) * m.RANGE for d in docs[0] | docs[1])
        if c["name"] == "one_each":
            w = min(k, n_lists)
            for h in range(2):
                assert sorted((d - 100) // m.RANGE for d in merged[q][h][:w, 1].tolist()) == list(range(w))
        if c["name"] == "distinct_big":
            assert min(docs[0] | docs[1]) > 2 ** 32
    if (k, n_lists) == (16, 16):
        q = [c["name"] for c in cases].index("one_each")
        assert sorted((d - 100) // m.RANGE for d in merged[q][0][:, 1].tolist()) == list(range(16))


def test_fusion_lists_are_what_they_claim():
    for c in m.wrrf_device_cases():
        for rec, n in ((c["dense"], c["n_dense"]), (c["bm25"], c["n_bm25"])):
            assert rec.shape == (n, 2)
            real = rec[rec[:, 1] >= 0, 1]
            assert len(set(real.tolist())) == real.size
            if n > 2:  # padding in the middle: a real record follows it
                first_pad = int(np.flatnonzero(rec[:, 1] < 0)[0])
                assert (rec[first_pad:, 1] >= 0).any()
        if c["n_bm25"] >= 24:
            assert set(c["dense"][:, 1].tolist()) & set(c["bm25"][:, 1].tolist()) - {-1}
    assert sorted(c["n_dense"] + c["n_bm25"] for c in m.wrrf_device_cases())[-2:] == [1024, 1024]
    for mm in (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097):
        lists = m.wrrf_switch_lists(mm)
        assert sum(len(l) for l in lists) == mm and all(len(set(l)) == len(l) for l in lists)
        if mm >= 63:
            shared = set(lists[0]) & set(lists[1]) & set(lists[2])
            assert abs(len(shared) - len(lists[0]) / 3) <= 1
    for mm in (1000, 3000, 6000):
        lists = m.wrrf_negative_lists(mm)
        assert sum(len(l) for l in lists) == mm
        assert all(min(l[:300]) < 0 and l[0] < 0 and l[150] < 0 and l[299] < 0 for l in lists)
        assert [l[:300] for l in lists] == [l[:300] for l in m.wrrf_negative_lists(1000)]


# --------------------------------------------------------------------------- 3. mutants
def _mutant(records, n_lists, k, stride, w_dense, w_bm25, wrrf_k, top_n, n_queries, merge=m.merge, bm25_at=None,
            q_step=None, fuse=None):
    """merge_fuse with one part replaced."""
    ids = np.empty((n_queries, top_n), np.int64)
    sbits = np.empty((n_queries, top_n), np.int64)
    counts = np.empty(n_queries, np.int32)
    step = 2 * k if q_step is None else q_step
    for q in range(n_queries):
        dense = merge(records, n_lists, k, stride, q * step)[:, 1].tolist()
        bm25 = merge(records, n_lists, k, stride, q * step + (k if bm25_at is None else bm25_at))[:, 1].tolist()
        fused = (m.wrrf_padded([dense, bm25], [w_dense, w_bm25], wrrf_k) if fuse is None
                 else fuse(dense, bm25, w_dense, w_bm25, wrrf_k, top_n))
        ids[q], sbits[q], counts[q] = m.fused_out(fused, top_n)
    return ids, sbits, counts


def _keyed(key):
    def merge(records, n_lists, k, stride, offset):
        cands = sorted(m.gather(records, n_lists, k, stride, offset), key=key)
        return m.pack([(c[0], c[1]) for c in cands[:k]], k)
    return merge


def _lane(delta):
    return lambda records, n_lists, k, stride, offset: m.kernel_walk(records, n_lists, k, stride, offset, thr_lane=k - 1 + delta)


def _fuse_rank0(dense, bm25, wd, wb, wk, top_n):
    rrf = {}
    for ranked, w in ((dense, wd), (bm25, wb)):
        for rank, i in enumerate(ranked):  # from 0
            if i >= 0:
                rrf[i] = rrf.get(i, 0.0) + w * (1 / (wk + rank))
    return sorted(rrf.items(), key=lambda x: x[1], reverse=True)


def _compacted(lists, weights, k):
    return m.wrrf_padded([[i for i in l if i >= 0] for l in lists], weights, k)


def _fuse_bm25_first(dense, bm25, wd, wb, wk, top_n):
    score = dict(m.wrrf_padded([dense, bm25], [wd, wb], wk))
    order = list(dict.fromkeys([i for i in bm25 if i >= 0] + [i for i in dense if i >= 0]))
    return sorted(((i, score[i]) for i in order), key=lambda x: x[1], reverse=True)


def _fuse_cut_first(dense, bm25, wd, wb, wk, top_n):
    entries = [(i, w * (1 / (wk + r))) for ranked, w in ((dense, wd), (bm25, wb)) for r, i in enumerate(ranked, 1) if i >= 0]
    entries = sorted(entries, key=lambda x: x[1], reverse=True)[:top_n]
    rrf = {}
    for i, c in entries:
        rrf[i] = rrf.get(i, 0.0) + c
    return sorted(rrf.items(), key=lambda x: x[1], reverse=True)


def _differs(a, b, q):
    c = int(a[2][q])
    return c != int(b[2][q]) or a[0][q, :c].tolist() != b[0][q, :c].tolist() or a[1][q, :c].tolist() != b[1][q, :c].tolist()


@pytest.fixture(scope="module")
def packs():
    out = []
    for p, (k, n_lists) in enumerate(m.PACKS):
        cases = m.cases_for(k, n_lists)
        buf, stride, lead = m.slab(cases, k, n_lists, m.pack_extra(p))
        out.append(dict(k=k, n_lists=n_lists, cases=cases, rec=buf[lead:], stride=stride))
    return out


def _share(packs, weights, top_n_of, which, **mut):
    """(queries on which the mutant differs from the model, queries) over the cases `which(pack, case)` selects."""
    differ = total = 0
    for pk in packs:
        qs = [q for q, c in enumerate(pk["cases"]) if which(pk, c)]
        if not qs:
            continue
        k, top_n, nq = pk["k"], top_n_of(pk["k"]), len(pk["cases"])
        args = (pk["rec"], pk["n_lists"], k, pk["stride"]) + tuple(weights) + (top_n, nq)
        want = m.merge_fuse(*args)
        got = _mutant(*args, **mut)
        differ += sum(_differs(want, got, q) for q in qs)
        total += len(qs)
    return differ, total


def test_ties_separate_list_order_from_doc_order(packs):
    all_k = lambda k: 2 * k
    permuted = lambda pk, c: c["family"] == "ties" and c.get("order") == "permuted"
    d, t = _share(packs, A, all_k, permuted, merge=_keyed(lambda c: (-c[0], c[2], c[3])))
    assert t >= 100 and 2 * d >= t, f"ties broken by list order: {d}/{t}"
    # in shard order the two are the same merge: that is why the permutations are there
    d0, t0 = _share(packs, A, all_k, lambda pk, c: c.get("order") == "shard", merge=_keyed(lambda c: (-c[0], c[2], c[3])))
    assert d0 == 0 and t0 > 0
    d, t = _share(packs, A, all_k, lambda pk, c: c["family"] == "ties", merge=_keyed(lambda c: (-c[0], -c[1])))
    assert t >= 150 and 2 * d >= t, f"ties broken doc descending: {d}/{t}"


def test_later_lists_separate_the_threshold_lane(packs):
    all_k = lambda k: 2 * k
    # lane k - 2: the record that belongs in slot k - 1 is turned away once slot k - 2 is taken.  k = 1 has no such slot
    # (lane -1 is lane 63, always empty: every record is admitted and the answer is right).
    fam = lambda pk, c: pk["k"] >= 2 and pk["n_lists"] >= 2 and (c["family"] == "distinct" or c["name"] in ("last", "one_each"))
    d, t = _share(packs, A, all_k, fam, merge=_lane(-1))
    assert t >= 80 and 2 * d >= t, f"threshold from lane k - 2: {d}/{t}"
    # lane k: for k < 64 slot k is slack behind the k that are returned -- more records are admitted, every one is put
    # in its place, the first k slots are the same: not a wrong answer, and no input can tell.  At k = 64 there is no
    # lane 64: the lane number wraps to 0, the threshold is the best record, and nearly everything is turned away.
    d, t = _share(packs, A, all_k, lambda pk, c: pk["k"] < 64, merge=_lane(+1))
    assert d == 0 and t > 0
    d, t = _share(packs, A, all_k, lambda pk, c: pk["k"] == 64 and pk["n_lists"] >= 2 and c["family"] == "distinct", merge=_lane(+1))
    assert t >= 16 and 2 * d >= t, f"threshold from lane k at k = 64: {d}/{t}"


def test_offsets_are_separated_on_every_case(packs):
    all_k = lambda k: 2 * k
    distinct = lambda pk, c: c["family"] == "distinct"
    d, t = _share(packs, A, all_k, distinct, bm25_at=0)
    assert d == t > 0, f"BM25 half read at offset 0: {d}/{t}"
    ignored = ignored_of = 0
    for pk in packs:
        assert [c["name"] for c in pk["cases"][:4]] == ["distinct0", "distinct1", "distinct2", "distinct_big"]
        k, nq = pk["k"], len(pk["cases"])
        args = (pk["rec"], pk["n_lists"], k, pk["stride"]) + A + (2 * k, nq)
        want = m.merge_fuse(*args)
        got = _mutant(*args, q_step=k)
        # query 0 has no block stride to get wrong; every later query has
        assert all(_differs(want, got, q) for q in (1, 2, 3)), ("query block stride k", k, pk["n_lists"])
        if pk["n_lists"] >= 2:  # `stride` ignored: the lists read back to back, payload after payload
            got = m.merge_fuse(pk["rec"], pk["n_lists"], k, nq * 2 * k, *A, 2 * k, nq)
            # query 0 of list 1 then starts on the poison behind list 0's payload; the later queries start on records of
            # the query before them
            assert _differs(want, got, 0), ("stride ignored", k, pk["n_lists"])
            ignored += sum(_differs(want, got, q) for q in (1, 2, 3))
            ignored_of += 3
        # poison never surfaces in the model's answer, so a 7 in the kernel's is a wrong address
        assert 7 not in want[0]
    assert ignored_of >= 60 and 2 * ignored >= ignored_of, f"stride ignored, queries after the first: {ignored}/{ignored_of}"


def test_fusion_families_separate_the_fusion_mutants(packs):
    real = lambda pk, c: bool((c["rec"][:, :, 1] >= 0).any())
    d, t = _share(packs, A, lambda k: 10, real, fuse=_fuse_rank0)
    assert d == t > 0, f"fusion rank from 0: {d}/{t}"
    d, t = _share(packs, m.WEIGHTS[1], lambda k: 2 * k, lambda pk, c: c["family"] == "disjoint", fuse=_fuse_bm25_first)
    assert d == t > 0, f"fused-score ties BM25 first: {d}/{t}"
    # ... and with the weights that differ there is no tie to resolve
    d0, _ = _share(packs, A, lambda k: 2 * k, lambda pk, c: c["family"] == "disjoint", fuse=_fuse_bm25_first)
    assert d0 == 0
    for top_n in (1, 10):
        d, t = _share(packs, A, lambda k: top_n, lambda pk, c: c["family"] == "both", fuse=_fuse_cut_first)
        assert t >= 50 and 2 * d >= t, f"top_n = {top_n} applied before duplicate ids are combined: {d}/{t}"
    # w_bm25 = 0: the BM25 ids still enter (with +0), so dropping the half is a different answer wherever it adds an id
    drop = lambda dense, bm25, wd, wb, wk, top_n: m.wrrf_padded([dense], [wd], wk)
    d, t = _share(packs, m.WEIGHTS[2], lambda k: 2 * k, lambda pk, c: c["family"] == "disjoint", fuse=drop)
    assert d == t > 0


def test_padding_inside_a_list_separates_the_rank_rule():
    """A merged list has its padding at the tail, so only the id-list entry points can tell whether a padding entry
    occupies a rank: anrag_wrrf_device's planted lists and anrag_wrrf's negative ids."""
    differ = total = 0
    for c in m.wrrf_device_cases():
        lists = [c["dense"][:, 1].tolist(), c["bm25"][:, 1].tolist()]
        differ += m.wrrf_padded(lists, [5.0, 1.0], 40.0) != _compacted(lists, [5.0, 1.0], 40.0)
        total += 1
    for mm in (1000, 3000, 6000):
        lists = m.wrrf_negative_lists(mm)
        differ += m.wrrf_padded(lists, [5.0, 1.0, 2.0], 40) != _compacted(lists, [5.0, 1.0, 2.0], 40)
        total += 1
    assert 2 * differ >= total and differ >= 7, f"{differ}/{total}"
    # without negative ids it is the oracle's fusion
    from oracle import ref_search

    lists = m.wrrf_switch_lists(1025)
    want = ref_search.weighted_reciprocal_rank_fusion(list(zip(lists, "abc")), {"a": 5.0, "b": 1.0, "c": 2.0}, 40)
    assert m.wrrf_padded(lists, [5.0, 1.0, 2.0], 40) == want


# --------------------------------------------------------------------------- 4. the limitation
def test_equal_scores_with_descending_docs_are_outside_the_contract():
    """Equal scores whose doc ids do not ascend inside a list: the kernel's walk stops at (1.0, 8), which loses to the
    threshold (1.0, 6), and never sees (1.0, 3) behind it.  Row sharding cannot produce this (doc ids ascend with rows, and
    the legs rank equal scores by row); a caller with other doc ids uses the shard group's shard-order merge."""
    k = 2
    rec = np.stack([m.pack([(1.0, 5), (1.0, 6)], k), m.pack([(1.0, 8), (1.0, 3)], k)])
    with pytest.raises(AssertionError, match="order"):
        m.check_contract(rec, 2, k, k, [0])
    assert m.kernel_walk(rec, 2, k, k, 0)[:, 1].tolist() == [5, 6]
    assert m.merge(rec, 2, k, k, 0)[:, 1].tolist() == [3, 5]
    # in contract, the same records: both give (3, 5)
    rec = np.stack([m.pack([(1.0, 5), (1.0, 6)], k), m.pack([(1.0, 3), (1.0, 8)], k)])
    m.check_contract(rec, 2, k, k, [0])
    assert m.kernel_walk(rec, 2, k, k, 0)[:, 1].tolist() == m.merge(rec, 2, k, k, 0)[:, 1].tolist() == [3, 5]
