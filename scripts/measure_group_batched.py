#!/usr/bin/env python
"""Dense query lists on a shard group (K2 on every shard + one merge) against the plain index, ONE device.

    python scripts/measure_group_batched.py [--rows 1000000 --dim 768] [--queries 256,1024] [--k 10] [--reps 5]
                                            [--only plain|S1|S2|S4|S8|S4-old] [--out FILE]

Per configuration and list length, after a warm-up call: best and median of `reps` `dense_search` calls as µs per
query, the spread (max - min) / min, what `batched_stats` moved by, and whether ids, counts and score bits equal the
first configuration's.  Configurations: the plain `Index`; groups of 1 / 2 / 4 / 8 shards of device 0; and `S4-old`, a
group of 4 created under ANRAG_GROUP_BATCHED=0 -- what such a call was answered with before the route existed (every
query its own batch = 1 pass on every shard; K1's score bits, so `equals_first` is false there by design).
`--only S4` runs one configuration alone, for `rocprofv3 --kernel-trace --stats -- python
scripts/measure_group_batched.py --only S4` (the per-launch time of group_batched_merge_kernel).
Cross-device behaviour is not measurable on one GPU: all shards sit on device 0.  Across devices a shard's block is
n_queries x k x 16 B of records plus 4 B of flag per query and chunk, read in place or staged; nothing is claimed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CORPUS_SEED, QUERY_SEED = 1234, 4321  # bench.py's


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", default="256,1024")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from anrag import synth
    from anrag.index import Index, ShardGroup

    dev = torch.device("cuda", 0)
    lengths = [int(x) for x in args.queries.split(",")]
    E = synth.dense_corpus(args.rows, args.dim, CORPUS_SEED, dev).cpu().numpy()
    Q = synth.dense_queries_global(args.rows, args.dim, max(lengths), QUERY_SEED, CORPUS_SEED, dev)[0].cpu().numpy()
    torch.cuda.empty_cache()

    configs = [("plain", None, None)] + [(f"S{s}", s, None) for s in (1, 2, 4, 8)] + [("S4-old", 4, "0")]
    rows, ref = [], {}
    for name, s, env in configs:
        if args.only and name != args.only:
            continue
        if env is not None:
            os.environ["ANRAG_GROUP_BATCHED"] = env  # read at group creation
        try:
            ix = Index(0) if s is None else ShardGroup([0] * s)
        finally:
            os.environ.pop("ANRAG_GROUP_BATCHED", None)
        with ix:
            ix.dense_load(E)
            for nq in lengths:
                q = Q[:nq]
                out = ix.dense_search(q, args.k)  # warm-up
                ref.setdefault(nq, out)
                same = bool(np.array_equal(out[0], ref[nq][0]) and np.array_equal(out[2], ref[nq][2])
                            and np.array_equal(out[1].view(np.int32), ref[nq][1].view(np.int32)))
                stats0 = ix.batched_stats() if hasattr(ix, "batched_stats") else None
                times = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    ix.dense_search(q, args.k)
                    times.append(time.perf_counter() - t0)
                row = dict(config=name, shards=s or 0, queries=nq, k=args.k,
                           best_us_per_query=round(1e6 * min(times) / nq, 2),
                           median_us_per_query=round(1e6 * statistics.median(times) / nq, 2),
                           spread_pct=round(100 * (max(times) - min(times)) / min(times), 2), equals_first=same)
                if stats0 is not None:
                    stats1 = ix.batched_stats()
                    row["batched_stats_moved"] = {key: stats1[key] - stats0[key] for key in stats1}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
