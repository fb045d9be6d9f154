#!/usr/bin/env python
"""Ranked query lists (full ranking) on a shard group against the plain index, ONE device: dense + BM25 fused,
similarity_k = common_sections_n = 12,000, through `rank_batch` on a plain `Index` and `rank_batch_group` on groups of
1 / 2 / 4 / 8 shards of device 0.

    python scripts/measure_group_rank.py [--rows 1000000 --dim 768 --queries 256] [--reps 5] [--only plain|S1|..] [--out FILE]
    python scripts/measure_group_rank.py --rows 9609 --dim 384 --vocab 20000 --queries 2048

Per configuration, after a warm-up call: best and median of `reps` calls as µs per query, the spread (max - min) / min,
and whether ids, counts and score bits equal the first configuration's.  `--only S4` runs one configuration alone, for a
`rocprofv3 --kernel-trace --stats -- python scripts/measure_group_rank.py --only S4` run of its own.
`--cold N`: first time what a group answered such a list with BEFORE the ranked route existed -- N queries one by one
through the cold routes of a group of 4 (each shard's host entry point with a sort of all its scores, a stable merge on
the host; the lists only, the fusion in Python is not counted).  The script also runs on a checkout without
`rank_batch_group`: then only `--cold` and the plain index are timed.
Cross-device behaviour is not measurable on one GPU: all shards sit on device 0.  Across devices a peer list is
12,000 x 12 B (row + fp64 score) per shard, leg and query, read in place or staged; nothing is claimed about it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CORPUS_SEED, QUERY_SEED, BM25_SEED, BM25_QUERY_SEED = 1234, 4321, 777, 99  # bench.py's
W_DENSE, W_BM25, WRRF_K, K = 5.0, 1.0, 60.0, 12000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--cold", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from anrag import synth
    from anrag.index import Index, ShardGroup, rank_batch

    try:
        from anrag.index import rank_batch_group
    except ImportError:  # the parent commit: only --cold means something there
        rank_batch_group = None

    dev = torch.device("cuda", 0)
    E = synth.dense_corpus(args.rows, args.dim, CORPUS_SEED, dev).cpu().numpy()
    Q = synth.dense_queries_global(args.rows, args.dim, args.queries, QUERY_SEED, CORPUS_SEED, dev)[0].cpu().numpy()
    post = synth.bm25_postings(args.rows, args.vocab, BM25_SEED, dev)
    idf = synth.bm25_idf(post["df"].cpu().numpy(), args.rows)
    terms = synth.bm25_queries_global(args.rows, args.vocab, args.queries, BM25_QUERY_SEED, BM25_SEED, dev)
    terms = [np.asarray(t, np.int32) for t in terms]
    pd, pt = post["post_doc"].cpu().numpy(), post["post_tf"].cpu().numpy()
    indptr, doc_len, avgdl = np.asarray(post["indptr"]), np.asarray(post["doc_len"]), post["total_len"] / args.rows
    del post
    torch.cuda.empty_cache()
    n, nq = args.rows, args.queries

    def load(ix):
        ix.dense_load(E)
        ix.bm25_load(indptr, pd, pt, idf, doc_len, avgdl, synth.BM25_K1, synth.BM25_B)
        return ix

    def ask(ix, entry):
        legs = [dict(index=ix, weight=W_DENSE, queries=Q), dict(index=ix, weight=W_BM25, term_lists=terms)]
        return entry(legs, nq, K, WRRF_K, K, id_space=n, want_scores=True)

    rows = []
    if args.cold:  # what a group answers such a list with WITHOUT the ranked route: query by query, shard after shard
        with ShardGroup([0] * 4) as g:
            load(g)
            m = min(args.cold, nq)
            k = min(K, n)

            def cold():
                for i in range(m):
                    g.dense_search(Q[i], k)
                    g.bm25_search(terms[i], k)

            cold()
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                cold()
                times.append(time.perf_counter() - t0)
            rows.append(dict(config="S4 cold routes, one by one (lists only, no fusion)", queries=m,
                             best_us_per_query=round(1e6 * min(times) / m, 1),
                             median_us_per_query=round(1e6 * statistics.median(times) / m, 1)))
            print(json.dumps(rows[-1]), flush=True)
    configs = [("plain", None)] + [(f"S{s}", s) for s in (1, 2, 4, 8)]
    ref = None
    for name, s in configs:
        if args.only and name != args.only:
            continue
        if s is not None and rank_batch_group is None:
            continue
        make = (lambda: Index(0)) if s is None else (lambda: ShardGroup([0] * s))
        entry = rank_batch if s is None else rank_batch_group
        with make() as ix:
            load(ix)
            out = ask(ix, entry)
            if ref is None:
                ref = out
            same = bool(np.array_equal(out[0], ref[0]) and np.array_equal(out[1].view(np.int64), ref[1].view(np.int64))
                        and np.array_equal(out[2], ref[2]))
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                ask(ix, entry)
                times.append(time.perf_counter() - t0)
            rows.append(dict(config=name, shards=s or 0, queries=nq,
                             best_us_per_query=round(1e6 * min(times) / nq, 2),
                             median_us_per_query=round(1e6 * statistics.median(times) / nq, 2),
                             spread_pct=round(100 * (max(times) - min(times)) / min(times), 2), equals_first=same))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
