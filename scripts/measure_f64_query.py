#!/usr/bin/env python3
"""The float64 query (the reference's text path, src/search_engine.py:157, :129), A/B inside ONE process: a library
built from the parent commit (ANRAG_PARENT_LIB, or ANRAG_LIB) against this tree's, each with its own index over the same
synthetic corpus of bench.py's shape.

  * a float64 dense top-10 per call (`anrag_dense_search_f64`): score array + library sort against the list scan K1D;
  * the float64 hybrid request per call: the parent's three host-synchronous calls (dense_search_f64 + bm25_search + wrrf)
    against ONE `anrag_hybrid_search_f64`;
  * K1D's kernel time from the library's own HIP-event profile, as bytes / time of the 8 TB/s peak.

Medians of three alternating pairs (parent, change, parent, change, ...), the parent's max - min beside them.
usage: ANRAG_PARENT_LIB=/path/to/parent/libanrag.so python scripts/measure_f64_query.py [rows] [dim] [calls]"""
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
from anrag.index import Index

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 768
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 100
dev = torch.device("cuda:0")


def parent_index():
    """An Index whose calls go to the parent's library.  Both libraries export the same names: the parent's is loaded
    RTLD_LOCAL | RTLD_DEEPBIND | RTLD_NOW so that its own calls bind to its own definitions, never to this tree's."""
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


old = parent_index() if parent_path else None  # (before this tree's library enters the global scope)
new = Index(0)
load(new)
if old is not None:
    load(old)
else:
    print("no ANRAG_PARENT_LIB: the parent's route is this library with the list scan switched off", flush=True)


def dense_top10(idx):
    return lambda i: idx.dense_search_f64(q64[i % 64], 10)


def three_calls(idx):
    def ask(i):
        doc, _, cnt = idx.dense_search_f64(q64[i % 64], 25)
        bdoc, _, bcnt = idx.bm25_search(terms[i % 64], 25)
        return idx.wrrf([doc[:cnt], bdoc[:bcnt]], [5.0, 1.0], 40.0, 10)
    return ask


def one_call(idx):
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
    verdict = np.median(a) - np.median(b) > max(a) - min(a)
    print("  below the parent by more than the parent's spread: %s" % verdict, flush=True)


base = old
if base is None:  # this library's own score array + sort route: a second index, list scan off
    base = Index(0)
    load(base)
    base.set_dense_f64_scan(False)
print("%d x %d, %d calls per run" % (n, d, calls), flush=True)
# same answers first
for i in range(4):
    r0, r1 = base.dense_search_f64(q64[i], 10), new.dense_search_f64(q64[i], 10)
    assert r0[0].tolist() == r1[0].tolist() and r0[1].view(np.uint64).tolist() == r1[1].view(np.uint64).tolist()
    h0, h1 = three_calls(base)(i), one_call(new)(i)
    assert h0[0].tolist() == h1[0].tolist() and h0[1].view(np.uint64).tolist() == h1[1].view(np.uint64).tolist()
ab("float64 dense top-10", dense_top10(base), dense_top10(new))
ab("float64 hybrid request (three calls -> one)", three_calls(base), one_call(new))

# kernel times: the library's HIP-event brackets, one kernel id at a time (K1 itself: the fp32 scan, no shadow prefilter)
new.set_dense_prefilter(0)
for name, idx, ask in (("K1D (list scan)", new, dense_top10(new)), ("score-array kernel", base, dense_top10(base)),
                       ("K1 (fp32 query)", new, lambda i: new.dense_search(q64[i % 64].astype(np.float32), 10))):
    idx.profile(True, kernels=[nat.KERNEL_DENSE_SCAN])
    idx.profile_reset()
    for i in range(40):
        ask(i)
    idx.sync()
    ms, launches = idx.profile_read(nat.KERNEL_DENSE_SCAN)
    idx.profile(False)
    us = ms / max(launches, 1) * 1e3
    print("%s: %.1f us per launch (%d launches), %.2f TB/s = %.1f %% of 8 TB/s" % (
        name, us, launches, n * d * 4 / us / 1e6, n * d * 4 / us / 1e6 / 8 * 100), flush=True)
print("dense_f64_stats (scanned, sorted):", new.dense_f64_stats(), flush=True)
