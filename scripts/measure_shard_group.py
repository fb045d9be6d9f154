#!/usr/bin/env python
"""Price of the shard group on ONE device: bench.py's 1M x 768 hybrid workload (synth.py, the bench's seeds, k = 25,
top 10) through `hybrid_search_batch` on a plain `Index` and on groups of 1 / 2 / 4 / 8 shards of device 0, with the
default prefilter mode and with mode 2 forced on every shard.

    python scripts/measure_shard_group.py [--rows 1000000] [--reps 5] [--only plain|S1|S2|S4|S8] [--out FILE]

Per configuration: queries per second (best of `reps` batches of 256 queries after a warm-up batch) and, for a group,
the HOST time spent enqueuing per exchange group of 8 queries, as the library itself clocks it around every group's
enqueue (`anrag_shard_group_debug_enqueue`: all shards' launches, event records and waits and the tail launch; no
uploads, no waiting for results), averaged over the timed batches.  That clock includes the shards' host-side
back-pressure: on a corpus that keeps the GPU busy it reads the GPU's time per group; the host's own enqueue cost is what
it reads on a small corpus (`--rows 16384 --vocab 20000`), where the GPU never holds the host back.  `--only S8` runs one configuration alone, for a
`rocprofv3 --kernel-trace --stats -- python scripts/measure_shard_group.py --only S8` run of its own.
Cross-device behaviour is not measurable on one GPU: all shards here sit on device 0 and share its HBM and CUs."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CORPUS_SEED, QUERY_SEED, BM25_SEED, BM25_QUERY_SEED = 1234, 4321, 777, 99  # bench.py's
W_DENSE, W_BM25, WRRF_K, K, TOPN = 5.0, 1.0, 40.0, 25, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from anrag import synth
    from anrag.index import Index, ShardGroup

    os.environ["ANRAG_BATCH_PIPELINE"] = "1"  # the plain index on the pipelined batch = 1 kernels too, not the ranking route
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

    def load(ix):
        ix.dense_load(E)
        ix.bm25_load(indptr, pd, pt, idf, doc_len, avgdl, synth.BM25_K1, synth.BM25_B)
        return ix

    def rate(ix):
        ix.hybrid_search_batch(Q, terms, K, W_DENSE, W_BM25, WRRF_K, TOPN)
        best = float("inf")
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ix.hybrid_search_batch(Q, terms, K, W_DENSE, W_BM25, WRRF_K, TOPN)
            best = min(best, time.perf_counter() - t0)
        return best

    configs = [("plain", None)] + [(f"S{s}", s) for s in (1, 2, 4, 8)]
    rows = []
    ref = None
    for name, s in configs:
        if args.only and name != args.only:
            continue
        make = (lambda: Index(0)) if s is None else (lambda: ShardGroup([0] * s))
        with make() as ix:
            load(ix)
            for mode in (-1, 2):
                ix.set_dense_prefilter(mode)
                out = ix.hybrid_search_batch(Q, terms, K, W_DENSE, W_BM25, WRRF_K, TOPN)
                if ref is None:
                    ref = out
                same = bool(np.array_equal(out[0], ref[0]) and np.array_equal(out[1].view(np.int64), ref[1].view(np.int64)))
                g0, ns0 = ix.enqueue_stats() if s else (0, 0)
                sec = rate(ix)
                g1, ns1 = ix.enqueue_stats() if s else (0, 0)
                host = round((ns1 - ns0) / 1e3 / (g1 - g0), 1) if s else ""
                rows.append(dict(config=name, shards=s or 0, prefilter_mode=mode, qps=round(args.queries / sec, 1),
                                 us_per_query=round(1e6 * sec / args.queries, 1),
                                 enqueue_clock_us_per_group=host, equals_first=same))
                print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("config,shards,prefilter_mode,qps,us_per_query,enqueue_clock_us_per_group,equals_first\n")
            for r in rows:
                f.write(",".join(str(r[k]) for k in ("config", "shards", "prefilter_mode", "qps", "us_per_query",
                                                     "enqueue_clock_us_per_group", "equals_first")) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
