"""CPU: the ranked route of the shard group -- the entry point is declared, exported and bound; it refuses malformed legs
before it touches a device; and the numpy model of its merge rule (tests/group_rank_model.py) equals a lexsort over
(-score, global row) on lists with heavy ties."""
import ctypes as C
import os
import re

import numpy as np

from group_rank_model import merge_by_counting, shard_lists, whole_list

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "anrag_shard_group_rank_batch"


def test_declared_exported_and_bound():
    from anrag import _native as nat

    text = open(os.path.join(REPO, "include", "anrag.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*const\s+anrag_group_rank_leg\s*\*", text)
    assert "typedef struct anrag_group_rank_leg" in text
    lib = nat.load_library()
    assert hasattr(lib, NAME)
    assert NAME in nat.EXPORTS
    fn = getattr(lib, NAME)
    assert fn.argtypes is not None and len(fn.argtypes) == 12
    fields = [f[0] for f in nat.GroupRankLeg._fields_]
    assert fields == ["group", "idx", "kind", "queries", "term_ids", "term_offsets", "allow_source", "n_sources",
                      "doc_of_row", "weight"]
    from anrag import index

    assert callable(index.rank_batch_group)


def test_malformed_legs_are_refused_without_a_device():
    from anrag import _native as nat

    lib = nat.load_library()
    cnt = np.zeros(1, np.int32)
    ids = np.zeros(4, np.int64)

    def call(arr, n_legs):
        return lib.anrag_shard_group_rank_batch(C.cast(arr, C.c_void_p), n_legs, 1, 4, 60.0, 4, 0, ids.ctypes.data, None,
                                                cnt.ctypes.data, None, None)

    arr = (nat.GroupRankLeg * 1)()
    arr[0].kind, arr[0].weight = nat.LEG_DENSE, 1.0
    assert call(arr, 0) == -1                       # n_legs = 0
    assert call(arr, 1) == -1                       # neither a group nor an index
    assert b"exactly one" in lib.anrag_last_error()
    arr[0].group, arr[0].idx = 0x1000, 0x2000       # both (never dereferenced)
    assert call(arr, 1) == -1
    assert b"exactly one" in lib.anrag_last_error()


def _bounds(n, S):
    base, extra = divmod(n, S)
    return [i * base + min(i, extra) for i in range(S + 1)]


def test_merge_model_is_score_desc_global_row_asc():
    rng = np.random.default_rng(7)
    for trial in range(60):
        n = int(rng.integers(8, 400))
        S = int(rng.integers(1, min(8, n) + 1))
        k = int(rng.choice([1, 3, n // 2 + 1, n, n + 50]))
        # heavy ties: a handful of values, zeros of both signs among them
        values = np.array([0.0, -0.0, 1.5, 1.5, -2.0, 3.25, np.inf])
        scores = values[rng.integers(0, len(values), size=n)]
        allowed = None
        if trial % 3 == 0:
            allowed = rng.random(n) < 0.4
            allowed[_bounds(n, S)[0]:_bounds(n, S)[1]] = False  # nothing left in the first shard
        b = _bounds(n, S)
        lists = shard_lists(scores, b, k, allowed)
        rows, sc = merge_by_counting(lists, b, k)
        all_rows = np.arange(n) if allowed is None else np.nonzero(allowed)[0]
        want = all_rows[np.lexsort((all_rows, -(scores[all_rows] + 0.0)))][:k]
        assert rows.tolist() == want.tolist(), (trial, n, S, k)
        assert np.array_equal(sc.view(np.int64), scores[want].view(np.int64))
        w_rows, w_sc = whole_list(scores, k, allowed)
        assert w_rows.tolist() == want.tolist()
