"""A numpy model of the shard group's list merge (shard_group_rank.hip: shard_list_merge_kernel): rank by counting.

Entry p of shard s, score x, gets the global rank
    p + sum over t < s of #{entries of t with score >= x} + sum over t > s of #{entries of t with score > x}
-- among equal scores the earlier shard, then the earlier position, stays ahead.  Shards are ascending contiguous row
blocks and a shard's list is (score desc, local row asc), so this is (score desc, global row asc).  -0.0 == +0.0."""
import numpy as np


def shard_lists(scores, bounds, k, allowed=None):
    """Per shard [lo, hi) of `bounds`: (local rows, scores) of its best min(k, allowed rows) by (score desc, row asc)."""
    out = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        s = np.asarray(scores[lo:hi])
        rows = np.arange(hi - lo)
        if allowed is not None:
            rows = rows[np.asarray(allowed[lo:hi], dtype=bool)]
        order = rows[np.lexsort((rows, -(s[rows] + 0.0)))][:k]
        out.append((order.astype(np.int64), s[order]))
    return out


def merge_by_counting(lists, bounds, k):
    """-> (global rows, scores) of the merged list, cut to k.  Every slot is written once."""
    total = sum(len(r) for r, _ in lists)
    n_out = min(k, total)
    out_rows = np.full(n_out, -1, np.int64)
    out_scores = np.zeros(n_out, np.float64)
    for s, (rows, sc) in enumerate(lists):
        for p in range(min(len(rows), k)):
            x = sc[p]
            r = p
            for t, (_, st) in enumerate(lists):
                if t == s:
                    continue
                neg = -(np.asarray(st, np.float64) + 0.0)  # ascending
                # entries of t ahead of mine: score >= x for an earlier shard, > x for a later one
                r += int(np.searchsorted(neg, -(x + 0.0), side="right" if t < s else "left"))
            if r < n_out:
                assert out_rows[r] == -1, "a slot written twice"
                out_rows[r] = bounds[s] + rows[p]
                out_scores[r] = x
    assert (out_rows >= 0).all()
    return out_rows, out_scores


def merge_by_doc(lists, bounds, k, doc_of_row):
    """What a (score desc, doc id asc) merge would return: the rule the group must NOT use."""
    rows = np.concatenate([bounds[s] + r for s, (r, _) in enumerate(lists)])
    sc = np.concatenate([x for _, x in lists])
    order = np.lexsort((np.asarray(doc_of_row)[rows], -(sc + 0.0)))[:k]
    return rows[order], sc[order]


def whole_list(scores, k, allowed=None):
    """The single index's list: (score desc, global row asc), filtered rows left out, cut to k."""
    s = np.asarray(scores)
    rows = np.arange(len(s))
    if allowed is not None:
        rows = rows[np.asarray(allowed, dtype=bool)]
    order = rows[np.lexsort((rows, -(s[rows] + 0.0)))][:k]
    return order.astype(np.int64), s[order]
