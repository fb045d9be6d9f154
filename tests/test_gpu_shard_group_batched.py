"""GPU: dense query lists on a shard group through K2 on every shard (anrag_shard_group_dense_search past the single
index's own gate) -- the answer is the single index's, ids, counts and score bits; it is the numpy merge
(tests/group_batched_model.py) of what S independent indexes return; it is the oracle's within 1e-4.  Shards of 65,536
rows or more are what the gate asks for, so the shapes are S * 65,536 + 77 rows; all shards sit on device 0."""
import ctypes as C

import numpy as np
import pytest

from group_batched_model import merge_shard_order
from helpers import assert_ranking_matches

pytestmark = pytest.mark.gpu

BASE = 7
ALLOW = np.array([1, 0, 1, 0, 0], dtype=np.uint8)
NQS = (17, 40, 256, 300)   # 128-query geometry twice, the 256-query one, two chunks (256 + 44)
KS = (1, 10, 64)


def make_world(n, d, seed, nq=300):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((n, d), dtype=np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    rows = rng.integers(0, n, nq)
    q = e[rows] + 0.05 * rng.standard_normal((nq, d), dtype=np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[1] = rng.standard_normal(d, dtype=np.float32)  # an un-planted query
    src = (np.arange(n) % 5).astype(np.uint16)
    return e, q, src


@pytest.fixture(scope="module")
def world128():
    return make_world(4 * 65536 + 77, 128, seed=21)


def rows_for(S):
    return S * 65536 + 77


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def assert_same_answer(got, want, what):
    (d, s, c), (d0, s0, c0) = got, want
    assert np.array_equal(c, c0), f"{what}: counts differ"
    assert np.array_equal(d, d0), f"{what}: ids differ in {int(np.sum(np.any(d != d0, axis=1)))} queries"
    assert np.array_equal(bits(s), bits(s0)), f"{what}: score bits differ, max |d| {np.max(np.abs(s - s0))}"


def alloc_calls():
    from anrag import _native as nat

    n = C.c_int64(0)
    nat.check(nat.load_library().anrag_debug_alloc_calls(C.byref(n)))
    return n.value


def check_equals_single(e, q, src, S):
    """Every (nq, k, filter): the group's answer is the single index's; the stats count the queries, nothing is redone."""
    from anrag.index import Index, ShardGroup

    with Index(0) as idx, ShardGroup([0] * S) as g:
        idx.dense_load(e, source_id=src, doc_id_base=BASE)
        g.dense_load(e, source_id=src, doc_id_base=BASE)
        assert min(np.diff(g.info()["dense_row_lo"])) >= 65536
        asked = passes = 0
        for nq in NQS:
            for k in KS:
                for allow in (None, ALLOW):
                    got = g.dense_search(q[:nq], k, allow)
                    assert_same_answer(got, idx.dense_search(q[:nq], k, allow), f"S={S} nq={nq} k={k} filter={allow is not None}")
                    asked += nq
                    passes += (nq + 255) // 256
        assert g.batched_stats() == dict(passes=passes, queries=asked, redone=0)


@pytest.mark.parametrize("S", [2, 3, 4])
def test_equals_the_single_index(world128, S):
    """1. ids, counts and score bits of `Index.dense_search` on the whole corpus (K2's bits: a row's score does not depend
    on its tile, its place in the tile or the 128 / 256-query geometry)."""
    e, q, src = world128
    n = rows_for(S)
    check_equals_single(e[:n], q, src[:n], S)


def test_equals_the_single_index_768d():
    """1. at the benchmark's dimension, S = 2."""
    e, q, src = make_world(rows_for(2), 768, seed=22)
    check_equals_single(e, q, src, 2)


@pytest.mark.parametrize("S,nq", [(2, 40), (4, 40), (2, 300)])
def test_equals_the_model(world128, S, nq):
    """2. S independent indexes on the row blocks, merged by the numpy model: the group's bits.  40 queries are one
    chunk in the 128-query geometry; 300 are a 256-query chunk and a second one of 44 into the other result block.
    Every side is asked twice and must answer alike, so a failure names the side that moved."""
    from anrag.index import Index, ShardGroup, group_bounds

    e, q, src = world128
    n = rows_for(S)
    b = group_bounds(n, S)
    k = 10
    for allow in (None, ALLOW):
        parts = []
        for lo, hi in zip(b[:-1], b[1:]):
            with Index(0) as idx:
                idx.dense_load(e[lo:hi], source_id=src[lo:hi], doc_id_base=BASE + lo)
                parts.append(idx.dense_search(q[:nq], k, allow))
                assert_same_answer(idx.dense_search(q[:nq], k, allow), parts[-1], f"index on rows [{lo}, {hi}) asked again")
        with ShardGroup([0] * S) as g:
            g.dense_load(e[:n], source_id=src[:n], doc_id_base=BASE)
            d, s, c = g.dense_search(q[:nq], k, allow)
            assert_same_answer(g.dense_search(q[:nq], k, allow), (d, s, c), "the group asked again")
        for qi in range(nq):
            md, ms, mc = merge_shard_order([(pd[qi], ps[qi], int(pc[qi])) for pd, ps, pc in parts], k)
            assert mc == c[qi], f"query {qi}: count {c[qi]}, model {mc}"
            assert md.tolist() == d[qi].tolist(), f"query {qi}: ids {d[qi].tolist()}, model {md.tolist()}"
            assert np.array_equal(bits(ms), bits(s[qi])), f"query {qi}: scores {s[qi].tolist()}, model {ms.tolist()}"


def test_against_the_oracle(world128):
    """3. a sample of queries (the un-planted one among them) against the fp32 oracle at 1e-4, with and without a filter."""
    from oracle import ref_search
    from anrag.index import ShardGroup

    e, q, src = world128
    S = 3
    n = rows_for(S)
    e = e[:n]
    sample = [0, 1, 2, 16, 39, 255, 256, 299]
    with ShardGroup([0] * S) as g:
        g.dense_load(e, source_id=src[:n], doc_id_base=BASE)
        for k in (10, 64):
            for allow in (None, ALLOW):
                d, s, c = g.dense_search(q, k, allow)
                keep = None if allow is None else allow[src[:n]].astype(bool)
                for qi in sample:
                    full = ref_search.dense_scores(q[qi], e)
                    want = ref_search.canonical_topk(full, k, keep)
                    assert c[qi] == k
                    assert_ranking_matches(want + BASE, full[want], d[qi], s[qi], 1e-4, None, f"k={k} q{qi}")


def test_edges(world128):
    """4. a filter that empties one shard; one that leaves fewer than k rows in all; equal rows on both sides of every
    shard boundary (global row ascending); a NaN row in the last shard (rank 0, +inf).  Each equals the single index."""
    from anrag.index import Index, ShardGroup, group_bounds

    e, q, _ = world128
    S, nq, k = 4, 20, 10
    n = rows_for(S)
    b = group_bounds(n, S)
    q = q[:nq].copy()
    e = e[:n].copy()
    for j, lo in enumerate(b[1:-1]):  # rows lo - 1 and lo are one vector, and query j is planted on it
        e[lo] = e[lo - 1]
        q[j] = e[lo]
    # sources: shard 1 is all source 4; elsewhere i % 4, but five rows (one in shard 1) carry the rare source 5
    src = (np.arange(n) % 4).astype(np.uint16)
    src[b[1]:b[2]] = 4
    rare = np.array([3, b[1] + 9, b[2] + 1, b[3] - 1, n - 2])
    src[rare] = 5
    no_shard1 = np.array([1, 1, 1, 1, 0, 0], dtype=np.uint8)
    only_rare = np.array([0, 0, 0, 0, 0, 1], dtype=np.uint8)
    with Index(0) as idx, ShardGroup([0] * S) as g:
        idx.dense_load(e, source_id=src, doc_id_base=BASE)
        g.dense_load(e, source_id=src, doc_id_base=BASE)
        # ties across the boundaries, no filter
        d, s, c = got = g.dense_search(q, k)
        assert_same_answer(got, idx.dense_search(q, k), "ties")
        for j, lo in enumerate(b[1:-1]):
            assert d[j, :2].tolist() == [BASE + lo - 1, BASE + lo] and bits(s[j, :1]) == bits(s[j, 1:2])
        # one shard filtered away entirely
        d, s, c = got = g.dense_search(q, k, no_shard1)
        assert_same_answer(got, idx.dense_search(q, k, no_shard1), "shard 1 filtered")
        assert np.all(c == k) and not np.any((d >= BASE + b[1]) & (d < BASE + b[2]))
        # fewer than k rows pass in all
        d, s, c = got = g.dense_search(q, k, only_rare)
        assert_same_answer(got, idx.dense_search(q, k, only_rare), "five rows pass")
        assert np.all(c == 5) and np.all(d[:, 5:] == -1) and np.all(np.isneginf(s[:, 5:]))
        assert all(sorted(row[:5].tolist()) == sorted((rare + BASE).tolist()) for row in d)
        # a NaN row in the last shard
        e[n - 5, 3] = np.nan
        idx.dense_load(e, source_id=src, doc_id_base=BASE)
        g.dense_load(e, source_id=src, doc_id_base=BASE)
        d, s, c = got = g.dense_search(q, k)
        assert_same_answer(got, idx.dense_search(q, k), "NaN row")
        assert np.all(d[:, 0] == BASE + n - 5) and np.all(np.isposinf(s[:, 0]))
        assert g.batched_stats()["redone"] == 0


def test_overflowing_survivor_lists_are_redone():
    """5. every row equal: each shard's survivor lists overflow by construction (as in
    test_gpu_batched.test_overflowing_survivor_lists_fall_back), all 16 queries are redone by the batch = 1 route."""
    from anrag.index import ShardGroup

    rng = np.random.default_rng(1)
    d, n = 256, 2 * 66000
    e = np.tile(rng.standard_normal(d, dtype=np.float32), (n, 1))
    q = rng.standard_normal((16, d), dtype=np.float32)
    with ShardGroup([0, 0]) as g:
        g.dense_load(e)
        doc, score, count = g.dense_search(q, 5)
        assert np.all(count == 5)
        assert np.all(doc == np.arange(5)[None, :])
        assert g.batched_stats() == dict(passes=1, queries=16, redone=16)


def test_gate(world128, monkeypatch):
    """6. shards under 65,536 rows, fewer than 16 queries, ANRAG_GROUP_BATCHED=0: the old route, its bits (those of the
    group's single-query calls), and the stats do not move."""
    from anrag.index import ShardGroup

    e, q, src = world128
    k = 10

    def singles(g, qs):
        parts = [g.dense_search(x, k) for x in qs]
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))

    none = dict(passes=0, queries=0, redone=0)
    with ShardGroup([0] * 3) as g:
        g.dense_load(e[:140000], source_id=src[:140000], doc_id_base=BASE)
        got = g.dense_search(q[:40], k)
        assert g.batched_stats() == none
        assert_same_answer(got, singles(g, q[:40]), "small shards")
    n = rows_for(2)
    with ShardGroup([0, 0]) as g:
        g.dense_load(e[:n], source_id=src[:n], doc_id_base=BASE)
        got = g.dense_search(q[:15], k)
        assert g.batched_stats() == none
        old = singles(g, q[:40])
        assert_same_answer(got, tuple(x[:15] for x in old), "15 queries")
        g.dense_search(q[:16], k)
        assert g.batched_stats() == dict(passes=1, queries=16, redone=0)
    monkeypatch.setenv("ANRAG_GROUP_BATCHED", "0")
    with ShardGroup([0, 0]) as g:
        g.dense_load(e[:n], source_id=src[:n], doc_id_base=BASE)
        got = g.dense_search(q[:40], k)
        assert g.batched_stats() == none
        assert_same_answer(got, old, "ANRAG_GROUP_BATCHED=0")


def test_split_precision(world128):
    """7. bf16x3 on every shard: scores within 1e-4 of the oracle, more than 0.99 of the ids those of f32
    (test_gpu_batched.test_split_precision_option's bar); back on f32 the single index's bits again."""
    from oracle import ref_search
    from anrag.index import Index, ShardGroup

    e, q, src = world128
    S, nq, k = 2, 200, 10
    n = rows_for(S)
    e, q = e[:n], q[:nq]
    with Index(0) as idx, ShardGroup([0] * S) as g:
        idx.dense_load(e, source_id=src[:n], doc_id_base=BASE)
        g.dense_load(e, source_id=src[:n], doc_id_base=BASE)
        want = idx.dense_search(q, k)
        g.set_batched_precision("bf16x3")
        d3, s3, c3 = g.dense_search(q, k)
        g.set_batched_precision("f32")
        assert_same_answer(g.dense_search(q, k), want, "f32 after bf16x3")
    assert np.all(c3 == k)
    for qi in range(nq):
        full = ref_search.dense_scores(q[qi], e)
        assert np.max(np.abs(full[d3[qi] - BASE] - s3[qi])) <= 1e-4, qi
    assert (d3 == want[0]).mean() > 0.99


def test_steady_state_and_the_pipeline_beside_it(world128):
    """8. no allocation across repeated 300-query calls after one warm-up; a `hybrid_search_batch` burst directly before
    and after changes neither route's answers (the pipeline is settled, the call pool is handed back)."""
    from anrag.index import ShardGroup

    e, q, src = world128
    S, k = 2, 10
    n = rows_for(S)
    no_terms = [[]] * 40
    with ShardGroup([0] * S) as g:
        g.dense_load(e[:n], source_id=src[:n], doc_id_base=BASE)
        want = g.dense_search(q, k)
        hyb = g.hybrid_search_batch(q[:40], no_terms, k, 1.0, 0.0, 60.0, k)
        before = alloc_calls()
        for _ in range(4):
            assert_same_answer(g.dense_search(q, k), want, "repeat")
        assert alloc_calls() == before
        for _ in range(2):
            got_h = g.hybrid_search_batch(q[:40], no_terms, k, 1.0, 0.0, 60.0, k)
            got_d = g.dense_search(q, k)
            assert all(np.array_equal(a, b_) for a, b_ in zip(got_h, hyb))
            assert_same_answer(got_d, want, "after a hybrid burst")
        assert alloc_calls() == before


@pytest.mark.parametrize("devices", [[0, 1], [1, 0]])
def test_distinct_devices(world128, devices):
    """9. the shards on two GPUs, either as the home device."""
    from anrag import _native as nat
    from anrag.index import Index, ShardGroup

    if nat.device_count() < 2:
        pytest.skip("needs two GPUs")
    e, q, src = world128
    n = rows_for(2)
    with Index(devices[0]) as idx, ShardGroup(devices) as g:
        idx.dense_load(e[:n], source_id=src[:n], doc_id_base=BASE)
        g.dense_load(e[:n], source_id=src[:n], doc_id_base=BASE)
        for nq, k, allow in ((300, 10, None), (40, 64, ALLOW)):
            assert_same_answer(g.dense_search(q[:nq], k, allow), idx.dense_search(q[:nq], k, allow), f"{devices} nq={nq}")
        assert g.batched_stats()["redone"] == 0
