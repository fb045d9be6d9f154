#!/usr/bin/env python3
"""One query at full ranking (similarity_k = top_n = 12,000: retrieval_eval.py's loop, one query per call), A/B inside
ONE process: a library built from the parent commit (ANRAG_PARENT_LIB) against this tree's.

  (a) dense + BM25 + WRRF per call on a synthetic corpus of bench.py's shape: the parent's three host-synchronous calls
      (dense_search + bm25_search + wrrf), ONE `anrag_rank_batch(n_queries = 1)` on the parent (narrow select), and the
      same call here in auto mode (and, for the record, with the wide select forced);
  (b) the gate sweep: the select alone (`anrag_debug_rank_select`, device time from the library's HIP-event bracket
      around its launches), narrow against wide, fp32 and fp64, over n_seg x n at k = 12,000;
  (c) `RetrievalEvaluationSystem.retrieve_documents` per call on the 9,609-row stand-in corpus with RANK_ONE_CALL off
      and on.

Medians of three alternating runs, the baseline's max - min in brackets.
usage: ANRAG_PARENT_LIB=/path/to/parent/libanrag.so python scripts/measure_rank_one.py a|b|c [rows] [dim] [calls]"""
import ctypes as C
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
parent_path = os.environ.pop("ANRAG_PARENT_LIB", None)
import numpy as np
import torch
from anrag import _native as nat
from anrag import index as index_mod
from anrag.index import Index, debug_rank_select, rank_wide_gate, rank_wide_stats, set_rank_wide

what = sys.argv[1] if len(sys.argv) > 1 else "a"
K = 12000


def med3(runs):
    return "%.1f us [%.1f]" % (np.median(runs), max(runs) - min(runs))


def alternate(asks, calls):
    """asks: name -> callable(i).  Three alternating runs of `calls` calls each -> name -> per-call us of each run."""
    out = {name: [] for name in asks}
    for _ in range(3):
        for name, ask in asks.items():
            for i in range(3):
                ask(i)
            t = time.perf_counter()
            for i in range(calls):
                ask(i)
            out[name].append((time.perf_counter() - t) / calls * 1e6)
    return out


def part_a():
    from anrag import synth

    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    d = int(sys.argv[3]) if len(sys.argv) > 3 else 768
    calls = int(sys.argv[4]) if len(sys.argv) > 4 else 30
    dev = torch.device("cuda:0")

    def parent_index():
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
    Q, _ = synth.dense_queries(E, 16, 4321)
    Q = Q.cpu().numpy().astype(np.float32)
    post = synth.bm25_postings(n, 200_000, 777, dev)
    idf = synth.bm25_idf(post["df"].cpu().numpy(), n)
    terms = [np.asarray(t, np.int32) for t in synth.bm25_queries(post, 16, 99)]
    torch.cuda.synchronize()

    def load(idx):
        idx.dense_load((E.data_ptr(), n, d))
        idx.bm25_load(post["indptr"], (post["post_doc"].data_ptr(), post["post_doc"].numel()),
                      (post["post_tf"].data_ptr(), post["post_tf"].numel()), idf, post["doc_len"],
                      float(post["total_len"]) / n, synth.BM25_K1, synth.BM25_B)

    assert parent_path, "part a needs ANRAG_PARENT_LIB"
    old = parent_index()
    new = Index(0)
    load(new)
    load(old)
    kd, kb = min(K, n), min(K, n)

    def three_calls(idx):
        def ask(i):
            doc, _, cnt = idx.dense_search(Q[i % 16], kd)
            bdoc, _, bcnt = idx.bm25_search(terms[i % 16], kb)
            return idx.wrrf([doc[0, :cnt[0]], bdoc[:bcnt]], [5.0, 1.0], 40.0, K)
        return ask

    def one_call(idx):
        def ask(i):
            legs = [dict(index=idx, weight=5.0, queries=Q[i % 16][None, :]),
                    dict(index=idx, weight=1.0, term_lists=[terms[i % 16]])]
            arr = (nat.RankLeg * 2)()
            keep = []
            for j, leg in enumerate(legs):
                arr[j].idx = idx.handle
                index_mod._fill_leg(arr[j], leg, j, 1, keep)
            return index_mod._rank_call(idx._lib.anrag_rank_batch, arr, 2, 1, K, 40.0, K, n, True, None, True)
        return ask

    ids3, sc3 = three_calls(old)(0)[:2]
    for name, idx, mode in (("parent one call", old, None), ("auto", new, -1), ("wide", new, 1)):
        if mode is not None:
            set_rank_wide(mode)
        ids1, sc1, cnt1 = one_call(idx)(0)
        m = min(len(ids3), int(cnt1[0]))
        same = ids1[0, :m].tolist() == np.asarray(ids3)[:m].tolist()
        print("%s == parent three calls in the first %d fused ids: %s" % (name, m, same), flush=True)

    def new_mode(mode):
        ask = one_call(new)

        def f(i):
            set_rank_wide(mode)
            return ask(i)
        return f

    s0 = rank_wide_stats()
    runs = alternate({"parent three calls": three_calls(old), "parent one call (narrow)": one_call(old),
                      "this tree, one call, auto": new_mode(-1), "this tree, one call, wide forced": new_mode(1),
                      "this tree, one call, narrow forced": new_mode(0)}, calls)
    set_rank_wide(-1)
    print("(a) %d x %d + %d BM25 documents, k = top_n = %d, %d calls per run; wide segments in total %d" % (
        n, d, n, K, calls, rank_wide_stats()[0] - s0[0]), flush=True)
    base = runs["parent three calls"]
    for name, r in runs.items():
        print("  %-36s %s  runs %s  %.2fx of the three calls; beyond their spread: %s" % (
            name, med3(r), " ".join("%.1f" % x for x in r), np.median(base) / np.median(r),
            abs(np.median(base) - np.median(r)) > max(base) - min(base)), flush=True)
    p1 = runs["parent one call (narrow)"]
    for name in ("this tree, one call, auto", "this tree, one call, wide forced", "this tree, one call, narrow forced"):
        r = runs[name]
        print("  %-36s against the parent's one call: %+.1f us, parent's spread %.1f" % (
            name, np.median(r) - np.median(p1), max(p1) - min(p1)), flush=True)


def part_b():
    ix = Index(0)
    rng = np.random.default_rng(8)
    budget = 64 << 20  # scores per launch this sweep stages (host array + pool): beyond it a cell is not measured
    print("(b) select alone, device time per launch (all its segments), k = %d: narrow, wide, medians of 3 alternating runs "
          "[narrow's max - min]; gate = what auto does now" % K, flush=True)
    for dtype in (np.float32, np.float64):
        for n in (65536, 262144, 1_000_000):
            stride = (n + 63) // 64 * 64
            for n_seg in (1, 2, 4, 8, 16, 32, 64, 128, 256):
                if n_seg * n > budget:
                    print("  %s n %8d n_seg %3d: not measured (staging budget)" % (np.dtype(dtype).name, n, n_seg), flush=True)
                    continue
                keys = rng.standard_normal((n_seg, stride)).astype(dtype)
                if dtype == np.float64:  # BM25-like: a few hundred positive scores over zeros
                    keys[:] = 0
                    for s in range(n_seg):
                        keys[s, rng.integers(0, n, 300)] = rng.random(300) * 20 + 0.1
                reps = 3 if n_seg * n > (8 << 20) else 8
                res = {0: [], 1: []}
                for _ in range(3):
                    for form in (0, 1):
                        debug_rank_select(ix, keys, n, K, form=form)
                        ix.profile(True, kernels=[nat.KERNEL_SELECT])
                        ix.profile_reset()
                        for _r in range(reps):
                            debug_rank_select(ix, keys, n, K, form=form)
                        ms, launches = ix.profile_read(nat.KERNEL_SELECT)
                        ix.profile(False)
                        res[form].append(ms / max(launches, 1) * 1e3)
                a, b = res[0], res[1]
                wins = np.median(a) - np.median(b) > max(a) - min(a)
                print("  %s n %8d n_seg %3d: narrow %9.1f us [%6.1f]  wide %9.1f us [%6.1f]  %5.2fx  wide wins beyond spread: "
                      "%-5s gate: %s" % (np.dtype(dtype).name, n, n_seg, np.median(a), max(a) - min(a), np.median(b),
                                         max(b) - min(b), np.median(a) / np.median(b), wins,
                                         rank_wide_gate(dtype == np.float64, n_seg, n)), flush=True)


def part_c():
    import pandas as pd
    from anrag import niceqa
    from anrag.bm25_index import Bm25Index
    from anrag.config import Config, InfoSource, LOCAL_ENCODER_KEY
    from anrag.database_manager import Bm25Proxy, DenseHandle
    from anrag.index_io import Section
    from anrag.query_rag_retrieval import RetrievalEvaluationSystem
    from anrag.search_engine import SearchEngine

    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 70
    G = os.path.join(REPO, "tests", "golden")
    data = niceqa.load_standin(os.path.join(G, "suggested_queries_bm25_preprocessed.json.gz"), os.path.join(G, "NICEQA.csv"))
    ids, sources, emb = data["ids"], data["sources"], data["embeddings"].astype(np.float32)
    df = pd.DataFrame({"id": ids, "document": [" ".join(t) for t in data["tokens"]], "source": sources, "embedding": list(emb)})
    DenseHandle(emb, sources).bind(df)
    proxy = Bm25Proxy(Bm25Index(data["tokens"], k1=1.7, b=0.83, epsilon=0.05), sources)
    sections = [Section(d, {"id": i, "source": s}) for i, s, d in zip(ids, sources, df["document"])]
    system = RetrievalEvaluationSystem.__new__(RetrievalEvaluationSystem)
    system.config, system.search_engine, system.voyage_client, system.fused = Config(), SearchEngine(None, None), None, True
    system.embeddings_data = {InfoSource.NICE: {LOCAL_ENCODER_KEY: df}}
    system.bm25_data = {InfoSource.NICE: (proxy, sections, ids)}
    qv, qt = niceqa.encode_questions(data)
    configs = {
        "dense full ranking": dict(model_weights={LOCAL_ENCODER_KEY: 1.0, "BM25": 0.0}, use_hybrid_search=False),
        "BM25 full ranking": dict(model_weights={LOCAL_ENCODER_KEY: 0.0, "BM25": 1.0}, use_hybrid_search=True),
        "hybrid full ranking": dict(model_weights={LOCAL_ENCODER_KEY: 5.0, "BM25": 1.0}, use_hybrid_search=True),
    }
    print("(c) retrieve_documents per call, 9,609 x 384 stand-in, similarity_k = common_sections_n = 12000, filter CG,NG, "
          "%d calls per run: RANK_ONE_CALL off, on [off's max - min]" % calls, flush=True)
    for name, cfg in configs.items():
        def asker(on):
            def ask(i):
                j = i % len(qv)
                system.RANK_ONE_CALL = on
                return system.retrieve_documents(query_embeddings={LOCAL_ENCODER_KEY: qv[j]}, query_tokens=qt[j] or ["asthma"],
                                                 similarity_k=12000, common_sections_n=12000, filename_type_filter="CG,NG",
                                                 wrrf_k=40, use_reranker=False, **cfg)
            return ask
        same = all(asker(False)(i) == asker(True)(i) for i in range(4))
        runs = alternate({"off": asker(False), "on": asker(True)}, calls)
        a, b = runs["off"], runs["on"]
        print("  %-20s off %s  on %s  %.2fx  same ids: %s  beyond off's spread: %s" % (
            name, med3(a), med3(b), np.median(a) / np.median(b), same, abs(np.median(a) - np.median(b)) > max(a) - min(a)),
            flush=True)


{"a": part_a, "b": part_b, "c": part_c}[what]()
