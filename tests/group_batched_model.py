"""A numpy model of the shard group's merge of per-shard top-k lists (shard_group.hip: group_batched_merge_kernel).

Every shard hands in, per query, up to k (doc, score) records in (score desc, local row asc) order and a count.  The
merge keeps the first k of the concatenation in SHARD ORDER under a stable sort by score: a candidate of a later shard
gets ahead of an earlier shard's only on a strictly greater score.  Shards are ascending contiguous row blocks, so this
is (score desc, global row asc) whatever documents the rows map to.  -0.0 == +0.0."""
import numpy as np


def merge_shard_order(lists, k):
    """`lists`: one (doc [k], score [k], count) per shard, in shard order -> (doc [k] int64, -1 padded; score [k] in the
    lists' dtype, -inf padded; count)."""
    docs = np.concatenate([np.asarray(d)[:c] for d, _, c in lists])
    scores = np.concatenate([np.asarray(s)[:c] for _, s, c in lists])
    order = np.argsort(-(scores.astype(np.float64) + 0.0), kind="stable")[:k]
    n = len(order)
    out_doc = np.full(k, -1, np.int64)
    out_score = np.full(k, -np.inf, scores.dtype)
    out_doc[:n] = docs[order]
    out_score[:n] = scores[order]
    return out_doc, out_score, n


def merge_doc_order(lists, k):
    """What a (score desc, doc id asc) merge would return: the rule the group must NOT use."""
    docs = np.concatenate([np.asarray(d)[:c] for d, _, c in lists])
    scores = np.concatenate([np.asarray(s)[:c] for _, s, c in lists])
    order = np.lexsort((docs, -(scores.astype(np.float64) + 0.0)))[:k]
    return docs[order], scores[order], len(order)


def shard_topk(scores, doc_of_row, lo, hi, k, allowed=None):
    """One shard's list for rows [lo, hi): its best k by (score desc, row asc) as (doc, score, count), padded."""
    rows = np.arange(lo, hi)
    if allowed is not None:
        rows = rows[np.asarray(allowed[lo:hi], dtype=bool)]
    order = rows[np.lexsort((rows, -(scores[rows].astype(np.float64) + 0.0)))][:k]
    doc = np.full(k, -1, np.int64)
    sc = np.full(k, -np.inf, scores.dtype)
    doc[: len(order)] = np.asarray(doc_of_row)[order]
    sc[: len(order)] = scores[order]
    return doc, sc, len(order)
