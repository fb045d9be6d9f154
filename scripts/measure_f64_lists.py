#!/usr/bin/env python3
"""Lists of float64 queries, A/B inside ONE process: a library built from the parent commit (ANRAG_PARENT_LIB, or
ANRAG_LIB) against this tree's, each with its own index over the same synthetic corpus of bench.py's shape.

  * the parent answers a list of 128 float64 queries one by one: `dense_search_f64` per query (dense), and
    `hybrid_search_f64` (k <= 64) or dense_search_f64 + bm25_search + wrrf (larger k) per query (hybrid);
  * this tree answers the list with ONE `rank_batch` whose dense leg is `queries_f64` (fp64 score tiles, K1TD);
  * K1TD alone, from the library's own HIP-event brackets: achieved fp64 FMA/s and HBM bytes/s.

Per-query medians of three alternating runs (parent, change, parent, change, ...), the parent's max - min beside them.
usage: ANRAG_PARENT_LIB=/path/to/parent/libanrag.so python scripts/measure_f64_lists.py [rows] [dim] [k ...]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
parent_path = os.environ.pop("ANRAG_PARENT_LIB", None) or os.environ.pop("ANRAG_LIB", None)
import numpy as np
import torch
from anrag import _native as nat
from anrag import synth
from anrag.index import Index, rank_batch

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 768
ks = [int(a) for a in sys.argv[3:]] or [10, 12000]
NQ = 128
dev = torch.device("cuda:0")


def parent_index():
    """An Index whose calls go to the parent's library (loaded RTLD_LOCAL | RTLD_DEEPBIND: its own definitions)."""
    lib = C.CDLL(parent_path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND | os.RTLD_NOW)
    for name, args in nat._SIGNATURES.items():
        if hasattr(lib, name):
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = C.c_int
    idx = Index.__new__(Index)
    idx._lib = lib
    h = C.c_void_p()
    assert lib.anrag_index_create(0, C.byref(h)) == 0
    idx._h, idx.device, idx.n_rows, idx.dim, idx.n_docs = h, 0, 0, 0, 0
    return idx


E = synth.dense_corpus(n, d, 1234, dev)
Q, _ = synth.dense_queries(E, NQ, 4321)
post = synth.bm25_postings(n, 200_000, 777, dev)
idf = synth.bm25_idf(post["df"].cpu().numpy(), n)
terms = [np.asarray(t, np.int32) for t in synth.bm25_queries(post, NQ, 99)]
rng = np.random.default_rng(5)
q64 = Q.cpu().numpy().astype(np.float64) + 1e-9 * rng.standard_normal((NQ, d))  # not representable in fp32
torch.cuda.synchronize()


def load(idx):
    idx.dense_load((E.data_ptr(), n, d))
    idx.bm25_load(post["indptr"], (post["post_doc"].data_ptr(), post["post_doc"].numel()),
                  (post["post_tf"].data_ptr(), post["post_tf"].numel()), idf, post["doc_len"], float(post["total_len"]) / n,
                  synth.BM25_K1, synth.BM25_B)


old = parent_index() if parent_path else None  # (before this tree's library enters the global scope)
new = Index(0)
load(new)
if old is not None:
    load(old)
else:
    print("no ANRAG_PARENT_LIB: the one-by-one route is this library's", flush=True)
    old = new


def loop(idx, k, hybrid):
    """The parent's answer to the list: one host-synchronous request per query."""
    top_n = min(k, 15 if k <= 64 else k)
    out = []
    for i in range(NQ):
        if not hybrid:
            doc, sc, cnt = idx.dense_search_f64(q64[i], k)
            out.append((doc[:min(cnt, top_n)], sc[:min(cnt, top_n)]))
        elif k <= 64:
            out.append(idx.hybrid_search_f64(q64[i], terms[i], k, 5.0, 1.0, 40.0, top_n))
        else:
            doc, _, cnt = idx.dense_search_f64(q64[i], k)
            bdoc, _, bcnt = idx.bm25_search(terms[i], k)
            out.append(idx.wrrf([doc[:cnt], bdoc[:bcnt]], [5.0, 1.0], 40.0, top_n))
    return out


def listed(idx, k, hybrid):
    top_n = min(k, 15 if k <= 64 else k)
    legs = [dict(index=idx, weight=5.0, queries_f64=q64)]
    if hybrid:
        legs.append(dict(index=idx, weight=1.0, term_lists=terms))
    ids, sc, cnt = rank_batch(legs, NQ, k, 40.0, top_n, id_space=n, want_scores=True)
    return [(ids[i, :cnt[i]], sc[i, :cnt[i]]) for i in range(NQ)]


def per_query_us(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) / NQ * 1e6


print("%d x %d, lists of %d float64 queries, per query" % (n, d, NQ), flush=True)
for k in ks:
    for hybrid in (False, True):
        what = "k = %d, %s" % (k, "hybrid" if hybrid else "dense")
        a, b = loop(old, k, hybrid), listed(new, k, hybrid)  # same answers first (and the warm-up of both)
        same = all(x[0].tolist() == y[0].tolist() and np.array_equal(np.asarray(x[1]).view(np.uint64), np.asarray(y[1]).view(np.uint64))
                   for x, y in zip(a, b))
        ta, tb = [], []
        for _ in range(3):
            ta.append(per_query_us(lambda: loop(old, k, hybrid)))
            tb.append(per_query_us(lambda: listed(new, k, hybrid)))
        spread = max(ta) - min(ta)
        print("%s: parent one by one %.1f us (runs %s, max - min %.1f), list %.1f us (runs %s): %.2fx; same ids and score bits: %s;"
              " below the parent by more than its spread: %s" % (
                  what, np.median(ta), " ".join("%.1f" % x for x in ta), spread, np.median(tb), " ".join("%.1f" % x for x in tb),
                  np.median(ta) / np.median(tb), same, np.median(ta) - np.median(tb) > spread), flush=True)

# K1TD alone: the library's HIP-event brackets around its launches (one launch carries the 128 queries)
legs = [dict(index=new, weight=1.0, queries_f64=q64)]
k = min(ks[0], 64)
rank_batch(legs, NQ, k, 40.0, k)
new.profile(True, kernels=[nat.KERNEL_DENSE_SCAN])
new.profile_reset()
for _ in range(3):
    rank_batch(legs, NQ, k, 40.0, k)
new.sync()
ms, launches = new.profile_read(nat.KERNEL_DENSE_SCAN)
new.profile(False)
us = ms / max(launches, 1) * 1e3
group = 16 if d <= 1024 else 8  # queries per pass over the rows (dense_tile_f64.hip)
passes = (NQ + group - 1) // group
print("K1TD: %.1f us per launch of %d queries (%d launches) = %.1f us per query; %.2f T FMA/s fp64; %d passes over the rows: "
      "%.2f TB/s read + %.2f TB/s of scores written" % (
          us, NQ, launches, us / NQ, n * d * NQ / us / 1e6, passes, passes * n * d * 4 / us / 1e6, n * NQ * 8 / us / 1e6),
      flush=True)
print("rank_f64_tile_stats (tiled, passed):", new.rank_f64_tile_stats(), flush=True)
