"""CPU: the merge rule of the shard group's batched dense route (tests/group_batched_model.py) on lists whose scores
tie across every shard boundary, under a permuted doc-id map: it is NOT a doc-id-ordered merge, and it IS the oracle's
`canonical_topk` over the whole score array by global row.  The two new entry points are declared, exported and bound."""
import numpy as np

from group_batched_model import merge_doc_order, merge_shard_order, shard_topk


def _bounds(n, S):
    base, extra = divmod(n, S)
    return [i * base + min(i, extra) for i in range(S + 1)]


def test_shard_order_merge_is_canonical_and_not_doc_order():
    from oracle import ref_search

    rng = np.random.default_rng(9)
    differed = 0
    for trial in range(40):
        S = int(rng.integers(2, 9))
        n = int(rng.integers(4 * S, 60 * S))
        k = int(rng.choice([1, 3, 10, 64]))
        b = _bounds(n, S)
        values = np.array([0.0, -0.0, 0.5, 0.5, -1.25, 2.0, np.inf], dtype=np.float32)
        scores = values[rng.integers(0, len(values), size=n)]
        for lo in b[1:-1]:  # the best score of the corpus on both sides of every boundary
            scores[lo - 1] = scores[lo] = np.float32(7.0)
        doc_of_row = rng.permutation(n).astype(np.int64) + 100
        allowed = None
        if trial % 4 == 0:
            allowed = rng.random(n) < 0.5
            allowed[b[1]:b[2]] = False  # nothing left in the second shard
        lists = [shard_topk(scores, doc_of_row, lo, hi, k, allowed) for lo, hi in zip(b[:-1], b[1:])]
        doc, sc, cnt = merge_shard_order(lists, k)
        want = ref_search.canonical_topk(scores + np.float32(0.0), k, allowed)
        assert cnt == len(want)
        assert doc[:cnt].tolist() == doc_of_row[want].tolist(), (trial, S, n, k)
        assert np.array_equal(sc[:cnt].view(np.int32), scores[want].view(np.int32))
        assert np.all(doc[cnt:] == -1) and np.all(np.isneginf(sc[cnt:]))
        d2, _, _ = merge_doc_order(lists, k)
        differed += d2.tolist() != doc[:cnt].tolist()
    assert differed >= 20, differed  # the permuted map makes a doc-id tie-break return other documents


def test_declared_exported_and_bound():
    from anrag import _native as nat
    from anrag.index import ShardGroup

    lib = nat.load_library()
    for name, n_args in (("anrag_shard_group_set_batched_precision", 2), ("anrag_shard_group_batched_stats", 4)):
        assert name in nat.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == n_args
    assert callable(ShardGroup.set_batched_precision) and callable(ShardGroup.batched_stats)
    assert lib.anrag_shard_group_batched_stats(None, None, None, None) == -1  # a NULL group is refused, not dereferenced
