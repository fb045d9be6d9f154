#!/usr/bin/env python3
"""The float64 query through the shadow prefilter (K1FD, dense_prefilter_f64.hip), A/B inside ONE process: a library built
from the parent commit (ANRAG_PARENT_LIB), whose float64 queries run K1D, against this tree's, each with its own index
over the same synthetic corpus of bench.py's shape (past 1 GiB of fp32 rows: both build the int8 shadow by themselves).

  * a float64 dense top-10 per call (`anrag_dense_search_f64`);
  * the fused float64 hybrid request per call (`anrag_hybrid_search_f64`);
  * the dense leg's kernels alone from the library's own HIP-event brackets: K1D on the parent, shadow scan + threshold +
    fp64 rescore (one bracket over the three) on this tree, with the survivors per query.

Medians of three alternating runs (parent, change, parent, change, ...), the parent's max - min beside them.  Without
ANRAG_PARENT_LIB the baseline is this library with the route switched off (`set_dense_f64_prefilter(False)`).
usage: ANRAG_PARENT_LIB=/path/to/parent/libanrag.so python scripts/measure_f64_prefilter.py [rows] [dim] [calls]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
parent_path = os.environ.pop("ANRAG_PARENT_LIB", None)
import numpy as np
import torch
from anrag import _native as nat
from anrag import synth
from anrag.index import Index

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 768
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 100
dev = torch.device("cuda:0")


def parent_index():
    """An Index whose calls go to the parent's library (RTLD_LOCAL | RTLD_DEEPBIND: its calls bind to its own code)."""
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
Q, _ = synth.dense_queries(E, 64, 4321)
post = synth.bm25_postings(n, 200_000, 777, dev)
idf = synth.bm25_idf(post["df"].cpu().numpy(), n)
terms = [np.asarray(t, np.int32) for t in synth.bm25_queries(post, 64, 99)]
rng = np.random.default_rng(5)
q64 = Q.cpu().numpy().astype(np.float64) + 1e-9 * rng.standard_normal((64, d))  # not representable in fp32
torch.cuda.synchronize()


def load(idx):
    idx.dense_load((E.data_ptr(), n, d))
    idx.bm25_load(post["indptr"], (post["post_doc"].data_ptr(), post["post_doc"].numel()),
                  (post["post_tf"].data_ptr(), post["post_tf"].numel()), idf, post["doc_len"], float(post["total_len"]) / n,
                  synth.BM25_K1, synth.BM25_B)


base = parent_index() if parent_path else None  # (before this tree's library enters the global scope)
new = Index(0)
load(new)
if base is None:
    print("no ANRAG_PARENT_LIB: the baseline is this library with the fp64 prefilter switched off", flush=True)
    base = Index(0)
    load(base)
    base.set_dense_f64_prefilter(False)
else:
    load(base)
form = new.debug_prefilter_read(data=False)["form"]
print("%d x %d, %d calls per run, prefilter form %d (0 off, 1 fp16, 2 int8)" % (n, d, calls, form), flush=True)
assert form != 0, "no prefilter form was built: force one with ANRAG_DENSE_PREFILTER=1|2"


def dense_top10(idx):
    return lambda i: idx.dense_search_f64(q64[i % 64], 10)


def fused(idx):
    return lambda i: idx.hybrid_search_f64(q64[i % 64], terms[i % 64], 25, 5.0, 1.0, 40.0, 10)


def per_call_us(ask):
    for i in range(8):
        ask(i)
    t = time.perf_counter()
    for i in range(calls):
        ask(i)
    return (time.perf_counter() - t) / calls * 1e6


def ab(what, ask_old, ask_new):
    a, b = [], []
    for _ in range(3):
        a.append(per_call_us(ask_old))
        b.append(per_call_us(ask_new))
    print("%s: parent %.1f us (runs %s, max - min %.1f), change %.1f us (runs %s): %.2fx" % (
        what, np.median(a), " ".join("%.1f" % x for x in a), max(a) - min(a), np.median(b),
        " ".join("%.1f" % x for x in b), np.median(a) / np.median(b)), flush=True)
    print("  below the parent by more than the parent's spread: %s" % (np.median(a) - np.median(b) > max(a) - min(a)),
          flush=True)


# same answers first: ids and score bits
for i in range(8):
    r0, r1 = base.dense_search_f64(q64[i], 10), new.dense_search_f64(q64[i], 10)
    assert r0[0].tolist() == r1[0].tolist() and r0[1].view(np.uint64).tolist() == r1[1].view(np.uint64).tolist()
    h0, h1 = fused(base)(i), fused(new)(i)
    assert h0[0].tolist() == h1[0].tolist() and h0[1].view(np.uint64).tolist() == h1[1].view(np.uint64).tolist()
ab("float64 dense top-10", dense_top10(base), dense_top10(new))
ab("float64 hybrid request (one fused call)", fused(base), fused(new))

# the dense leg's kernels: the library's HIP-event bracket around what it launches for one query
p0 = new.dense_f64_prefilter_stats()
for name, idx in (("parent: K1D", base), ("change: shadow scan + threshold + fp64 rescore", new)):
    idx.profile(True, kernels=[nat.KERNEL_DENSE_SCAN])
    idx.profile_reset()
    for i in range(40):
        idx.dense_search_f64(q64[i % 64], 10)
    idx.sync()
    ms, launches = idx.profile_read(nat.KERNEL_DENSE_SCAN)
    idx.profile(False)
    print("%s: %.1f us per query (%d brackets)" % (name, ms / max(launches, 1) * 1e3, launches), flush=True)
p1 = new.dense_f64_prefilter_stats()
print("survivors per float64 query (k = 10): %.1f over %d queries" % ((p1[1] - p0[1]) / max(p1[0] - p0[0], 1), p1[0] - p0[0]),
      flush=True)
print("dense_f64_stats (scanned, sorted):", new.dense_f64_stats(), " fp64 prefilter (queries, survivors):", p1, flush=True)
