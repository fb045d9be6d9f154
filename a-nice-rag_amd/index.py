"""`Index`: one GPU's shard (corpus rows + postings) resident in HBM, over the C ABI.

Thin, numpy-in / numpy-out; no torch types here.  The reference-shaped classes
(`database_manager.DatabaseManager`, `search_engine.SearchEngine`) sit on top.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _native as nat


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _allow_bytes(allow) -> Tuple[Optional[np.ndarray], int]:
    if allow is None:
        return None, 0
    a = np.ascontiguousarray(allow, dtype=np.uint8)
    return a, int(a.size)


def rank_caps() -> Tuple[int, int]:
    """Longest list `rank_batch` returns for a dense leg / for a BM25 leg or a fused ranking."""
    a, b = C.c_int32(), C.c_int32()
    nat.check(nat.load_library().anrag_rank_caps(C.byref(a), C.byref(b)))
    return a.value, b.value


def set_rank_wide(mode: int) -> None:
    """`anrag_set_rank_wide`: which form of the select a ranking takes for segments longer than the list cap --
    -1 auto (the measured gate), 0 never wide, 1 always wide.  Process-wide."""
    nat.check(nat.load_library().anrag_set_rank_wide(int(mode)))


def rank_wide_stats() -> Tuple[int, int]:
    """(segments sorted by the wide form, pass launches enqueued for them), cumulative and process-wide."""
    a, b = C.c_int64(), C.c_int64()
    nat.check(nat.load_library().anrag_rank_wide_stats(C.byref(a), C.byref(b)))
    return a.value, b.value


def rank_wide_gate(fp64: bool, n_seg: int, n: int) -> bool:
    """Does a launch of `n_seg` segments of `n` scores take the wide form in auto mode?"""
    w = C.c_int32()
    nat.check(nat.load_library().anrag_rank_wide_gate(int(bool(fp64)), int(n_seg), int(n), C.byref(w)))
    return bool(w.value)


def debug_rank_select(index, keys: np.ndarray, n: int, k: int, ties: Optional[np.ndarray] = None, seg_k=None,
                      form: int = -1, parts: int = 0):
    """`anrag_debug_rank_select`: the select + sort of a ranking over planted scores.  keys [n_seg, stride] float32 or
    float64 (the first n of a row count), ties (optional, float64 keys) [n_seg, stride] uint32.
    -> (rows [n_seg, kk] uint32, scores [n_seg, kk] float64, counts [n_seg] int32), kk = min(k, the list cap); entries
    past a segment's count are zero."""
    keys = np.ascontiguousarray(keys)
    assert keys.ndim == 2 and keys.dtype in (np.float32, np.float64)
    fp64 = keys.dtype == np.float64
    n_seg, stride = keys.shape
    kk = min(int(k), rank_caps()[1 if fp64 else 0])
    if ties is not None:
        ties = np.ascontiguousarray(ties, dtype=np.uint32)
        assert ties.shape == keys.shape
    if seg_k is not None:
        seg_k = np.ascontiguousarray(seg_k, dtype=np.int32)
        assert seg_k.shape == (n_seg,)
    rows = np.zeros((n_seg, kk), np.uint32)
    scores = np.zeros((n_seg, kk), np.float64)
    counts = np.zeros(n_seg, np.int32)
    nat.check(nat.load_library().anrag_debug_rank_select(
        index.handle, keys.ctypes.data, int(fp64), ties.ctypes.data if ties is not None else None, n_seg, stride, int(n),
        int(k), seg_k.ctypes.data if seg_k is not None else None, int(form), int(parts), rows.ctypes.data,
        scores.ctypes.data, counts.ctypes.data))
    return rows, scores, counts


def _fill_leg(slot, leg: dict, i: int, n_queries: int, keep: list) -> None:
    """The operands of one leg into its C struct (`RankLeg` / `GroupRankLeg`: the shared fields); `keep` holds the arrays."""
    ix = leg["index"]
    slot.weight = float(leg["weight"])
    allow, ns = _allow_bytes(leg.get("allow"))
    keep.append(allow)
    slot.allow_source = nat.ptr(allow)
    slot.n_sources = ns
    dmap = leg.get("doc_of_row")
    if dmap is not None:
        dmap = np.ascontiguousarray(dmap, dtype=np.int64)
        keep.append(dmap)
    slot.doc_of_row = nat.ptr(dmap)
    if leg.get("queries_f64") is not None:
        q = np.ascontiguousarray(leg["queries_f64"])
        assert q.dtype == np.float64, f"leg {i}: queries_f64 must be float64 (got {q.dtype}); it is never cast"
        assert leg.get("queries") is None, f"leg {i}: queries and queries_f64 are two kinds of leg"
        if q.ndim == 1:
            q = q[None, :]
        assert q.shape == (n_queries, ix.dim), f"leg {i}: queries_f64 {q.shape} != ({n_queries}, {ix.dim})"
        keep.append(q)
        slot.kind = nat.LEG_DENSE_F64
        slot.queries = q.ctypes.data
    elif leg.get("queries") is not None:
        q = _f32(leg["queries"])
        if q.ndim == 1:
            q = q[None, :]
        assert q.shape == (n_queries, ix.dim), f"leg {i}: queries {q.shape} != ({n_queries}, {ix.dim})"
        keep.append(q)
        slot.kind = nat.LEG_DENSE
        slot.queries = q.ctypes.data
    else:
        term_lists = leg["term_lists"]
        assert len(term_lists) == n_queries
        offsets = np.zeros(n_queries + 1, dtype=np.int64)
        np.cumsum(np.fromiter(map(len, term_lists), np.int64, n_queries), out=offsets[1:])
        if not offsets[-1]:
            terms = np.zeros(1, np.int32)
        elif all(type(t) is np.ndarray and t.dtype == np.int32 and t.ndim == 1 for t in term_lists):
            terms = np.concatenate(term_lists)  # (what Bm25Index.term_ids returns: no per-list conversion)
        else:
            terms = np.concatenate([np.asarray(t, dtype=np.int32).reshape(-1) for t in term_lists]).astype(np.int32)
        terms = np.ascontiguousarray(terms)
        keep += [offsets, terms]
        slot.kind = nat.LEG_BM25
        slot.term_ids = terms.ctypes.data
        slot.term_offsets = offsets.ctypes.data


def _rank_call(entry, arr, n_legs, n_queries, similarity_k, wrrf_k, top_n, id_space, want_scores, expect, want_ids):
    out_id = np.empty((n_queries, top_n), np.int64) if want_ids else None
    out_score = np.empty((n_queries, top_n), np.float64) if want_scores and want_ids else None
    count = np.zeros(n_queries, np.int32)
    exp = ranks = None
    if expect is not None:
        exp = np.ascontiguousarray(expect, dtype=np.int64)
        assert exp.shape == (n_queries,)
        ranks = np.empty(n_queries, np.int32)
    nat.check(entry(C.cast(arr, C.c_void_p), n_legs, int(n_queries), int(similarity_k), float(wrrf_k),
                    int(top_n), int(id_space), nat.ptr(out_id), nat.ptr(out_score),
                    count.ctypes.data, nat.ptr(exp), nat.ptr(ranks)))
    if expect is not None:
        return out_id, out_score, count, ranks
    return out_id, out_score, count


def rank_batch(legs: Sequence[dict], n_queries: int, similarity_k: int, wrrf_k: float, top_n: int,
               id_space: int = 0, want_scores: bool = False, expect=None, want_ids: bool = True):
    """`anrag_rank_batch`: full-ranking retrieval (large k) for a LIST of queries, every step on the device.
    `legs`: dicts in the reference's list order (dense models first, BM25 last) with
        index (Index), weight, allow (uint8 per source or None), doc_of_row (int64 per row or None), and one of
        queries (float32 [nq, dim]; any other dtype is cast to float32), queries_f64 (float64 [nq, dim], never cast
        down: scored in fp64 with the bits of `Index.dense_search_f64`) or term_lists (one int32 sequence per query; an
        empty one = no BM25 for that query).  Legs of the three kinds may be mixed.
    `expect` (int64 per query): also return the 1-based rank of that document in each answer (-1: absent);
    `want_ids=False` then skips the id lists altogether.
    -> (ids [nq, top_n] int64 (-1 padded) or None, scores [nq, top_n] float64 or None, counts [nq] int32)
       -- plus ranks [nq] int32 as a fourth element when `expect` is given."""
    lib = nat.load_library()
    arr = (nat.RankLeg * len(legs))()
    keep = []
    for i, leg in enumerate(legs):
        arr[i].idx = leg["index"].handle  # (a ShardGroup has none: ERR_UNSUPPORTED -- its entry is rank_batch_group)
        _fill_leg(arr[i], leg, i, n_queries, keep)
    return _rank_call(lib.anrag_rank_batch, arr, len(legs), n_queries, similarity_k, wrrf_k, top_n, id_space, want_scores,
                      expect, want_ids)


def rank_batch_group(legs: Sequence[dict], n_queries: int, similarity_k: int, wrrf_k: float, top_n: int,
                     id_space: int = 0, want_scores: bool = False, expect=None, want_ids: bool = True):
    """`anrag_shard_group_rank_batch`: `rank_batch` for legs that live on shard groups -- a leg's `index` is a
    `ShardGroup` or an `Index`, the legs may sit on different groups, shard counts and devices.  Same arguments, same
    return shapes, and the same ids, counts, ranks and score bits as `rank_batch` on ONE index holding the whole corpus
    (`doc_of_row` maps the leg's GLOBAL rows).  A `queries_f64` leg is not served on shard groups: `AnragError(-1)`."""
    lib = nat.load_library()
    arr = (nat.GroupRankLeg * len(legs))()
    keep = []
    for i, leg in enumerate(legs):
        ix = leg["index"]
        if isinstance(ix, ShardGroup):
            arr[i].group = ix.group
        else:
            arr[i].idx = ix.handle
        _fill_leg(arr[i], leg, i, n_queries, keep)
    return _rank_call(lib.anrag_shard_group_rank_batch, arr, len(legs), n_queries, similarity_k, wrrf_k, top_n, id_space,
                      want_scores, expect, want_ids)


def parse_devices(text: str) -> list:
    """`ANRAG_DEVICES`: "0, 1,1" -> [0, 1, 1] (repeats allowed: several shards on one GPU).  Empty, negative,
    non-numeric entries and more than 16 of them are errors."""
    parts = [p.strip() for p in str(text).split(",")]
    if not parts or any(p == "" for p in parts):
        raise ValueError(f"ANRAG_DEVICES={text!r}: expected a comma-separated list of device numbers")
    if not all(p.isdigit() for p in parts):
        raise ValueError(f"ANRAG_DEVICES={text!r}: device numbers must be non-negative integers")
    if len(parts) > nat.GROUP_MAX_SHARDS:
        raise ValueError(f"ANRAG_DEVICES={text!r}: at most {nat.GROUP_MAX_SHARDS} shards")
    return [int(p) for p in parts]


def group_bounds(n: int, n_shards: int) -> list:
    """Block bounds [lo_0, ..., lo_S] a shard group cuts `n` rows into (the rule of `sharded.shard_bounds`)."""
    base, extra = divmod(int(n), int(n_shards))
    return [i * base + min(i, extra) for i in range(n_shards + 1)]


class ShardGroup:
    """Owns an `anrag_shard_group*`: ONE corpus over several GPUs (or several shards of one GPU) in one process, with
    `Index`'s method names and return shapes for what a group serves -- every answer equals the single index's, ids,
    counts and score bits.  `dense_search` with 16 or more queries takes the matrix-core pass (K2) on every shard where
    the single index takes it (every shard >= 65,536 rows, dim % 32 == 0, k <= 64) and merges the shards' lists on the
    home device; `set_batched_precision` / `batched_stats` belong to that route.  Ranked lists of queries (full ranking)
    go through `rank_batch_group`.  `dense_scores`,
    `bm25_scores` and `rank_batch` itself (it takes `Index` legs: a group has no `handle`) raise `AnragError` with code
    `ERR_UNSUPPORTED`."""

    def __init__(self, devices: Sequence[int]):
        self._lib = nat.load_library()
        self.devices = [int(d) for d in devices]
        dev = np.ascontiguousarray(self.devices, dtype=np.int32)
        h = C.c_void_p()
        nat.check(self._lib.anrag_shard_group_create(dev.ctypes.data if dev.size else None, int(dev.size), C.byref(h)))
        self._g = h
        self.device = self.devices[0]
        self.n_shards = len(self.devices)
        self.n_rows = 0
        self.dim = 0
        self.n_docs = 0

    def close(self) -> None:
        if getattr(self, "_g", None):
            self._lib.anrag_shard_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def group(self) -> C.c_void_p:
        if not self._g:
            raise nat.AnragError(-3, "shard group is closed")
        return self._g

    @property
    def handle(self):
        raise nat.AnragError(nat.ERR_UNSUPPORTED, "a shard group has no anrag_index handle: anrag_rank_batch "
                                                  "(a group's entry is rank_batch_group) and the *_device entries take "
                                                  "one index")

    def shard(self, i: int) -> C.c_void_p:
        """Borrowed `anrag_index*` of shard i (stats, profiling, tests); it dies with the group."""
        h = C.c_void_p()
        nat.check(self._lib.anrag_shard_group_shard(self.group, int(i), C.byref(h)))
        return h

    def shard_prefilter_stats(self, i: int) -> tuple:
        q, s = C.c_int64(0), C.c_int64(0)
        nat.check(self._lib.anrag_dense_prefilter_stats(self.shard(i), C.byref(q), C.byref(s)))
        return q.value, s.value

    def sync(self) -> None:
        nat.check(self._lib.anrag_shard_group_sync(self.group))

    def set_dense_prefilter(self, mode: int = -1) -> None:
        nat.check(self._lib.anrag_shard_group_set_dense_prefilter(self.group, int(mode)))

    def set_batched_precision(self, mode: str = "f32") -> None:
        """`Index.set_batched_precision` on every shard: "f32" (default) or "bf16x3"."""
        nat.check(self._lib.anrag_shard_group_set_batched_precision(self.group, {"f32": 0, "bf16x3": 1}[mode]))

    def batched_stats(self) -> dict:
        """The batched dense route so far: `passes` (chunks of up to 256 queries), `queries` it answered, `redone` (those
        of them a shard flagged and the batch = 1 route answered)."""
        p, q, r = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        nat.check(self._lib.anrag_shard_group_batched_stats(self.group, C.byref(p), C.byref(q), C.byref(r)))
        return dict(passes=p.value, queries=q.value, redone=r.value)

    def dense_load(self, embeddings, source_id=None, doc_id=None, doc_id_base: int = 0) -> None:
        """Host operands only (a numpy matrix): the group cuts it into row blocks, one per shard."""
        if isinstance(embeddings, tuple):
            raise nat.AnragError(nat.ERR_UNSUPPORTED, "a shard group loads host arrays, not device buffers")
        keep = _f32(embeddings)
        assert keep.ndim == 2
        n, d = keep.shape
        src = None if source_id is None else np.ascontiguousarray(source_id, dtype=np.uint16)
        doc = None if doc_id is None else np.ascontiguousarray(doc_id, dtype=np.int64)
        assert src is None or src.shape == (n,)
        assert doc is None or doc.shape == (n,)
        nat.check(self._lib.anrag_shard_group_dense_load(self.group, keep.ctypes.data, n, d, nat.ptr(src), nat.ptr(doc),
                                                         int(doc_id_base)))
        self.n_rows, self.dim = int(n), int(d)

    def bm25_load(self, indptr, post_doc, post_tf, idf, doc_len, avgdl: float, k1: float, b: float,
                  source_id=None, doc_id=None, doc_id_base: int = 0) -> None:
        if isinstance(post_doc, tuple) or isinstance(post_tf, tuple):
            raise nat.AnragError(nat.ERR_UNSUPPORTED, "a shard group loads host arrays, not device buffers")
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        idf = np.ascontiguousarray(idf, dtype=np.float64)
        doc_len = np.ascontiguousarray(doc_len, dtype=np.int32)
        post_doc = np.ascontiguousarray(post_doc, dtype=np.int32)
        post_tf = np.ascontiguousarray(post_tf, dtype=np.int32)
        n_terms, n_docs = indptr.size - 1, doc_len.size
        assert idf.size == n_terms and post_doc.size == post_tf.size == int(indptr[-1])
        src = None if source_id is None else np.ascontiguousarray(source_id, dtype=np.uint16)
        doc = None if doc_id is None else np.ascontiguousarray(doc_id, dtype=np.int64)
        nat.check(self._lib.anrag_shard_group_bm25_load(self.group, indptr.ctypes.data, n_terms, post_doc.ctypes.data,
                                                        post_tf.ctypes.data, idf.ctypes.data, doc_len.ctypes.data, n_docs,
                                                        float(avgdl), float(k1), float(b), nat.ptr(src), nat.ptr(doc),
                                                        int(doc_id_base)))
        self.n_docs = int(n_docs)

    def dense_search(self, queries, k: int, allow_source=None):
        q = _f32(queries)
        if q.ndim == 1:
            q = q[None, :]
        if self.n_rows == 0:
            raise nat.AnragError(-3, "dense search before dense_load")
        assert q.shape[1] == self.dim, f"query dim {q.shape[1]} != index dim {self.dim}"
        nq = q.shape[0]
        allow, ns = _allow_bytes(allow_source)
        doc = np.empty((nq, k), np.int64)
        score = np.empty((nq, k), np.float32)
        count = np.empty(nq, np.int32)
        nat.check(self._lib.anrag_shard_group_dense_search(self.group, q.ctypes.data, nq, int(k), nat.ptr(allow), ns,
                                                           doc.ctypes.data, score.ctypes.data, count.ctypes.data))
        return doc, score, count

    def dense_search_f64(self, query, k: int, allow_source=None):
        q = np.ascontiguousarray(query, dtype=np.float64).reshape(-1)
        assert q.size == self.dim, f"query dim {q.size} != index dim {self.dim}"
        allow, ns = _allow_bytes(allow_source)
        doc = np.empty(k, np.int64)
        score = np.empty(k, np.float64)
        count = np.zeros(1, np.int32)
        nat.check(self._lib.anrag_shard_group_dense_search_f64(self.group, q.ctypes.data, int(k), nat.ptr(allow), ns,
                                                               doc.ctypes.data, score.ctypes.data, count.ctypes.data))
        return doc, score, int(count[0])

    def bm25_search(self, term_ids: Sequence[int], k: int, allow_source=None):
        t = np.ascontiguousarray(term_ids, dtype=np.int32)
        allow, ns = _allow_bytes(allow_source)
        doc = np.empty(k, np.int64)
        score = np.empty(k, np.float64)
        count = np.zeros(1, np.int32)
        nat.check(self._lib.anrag_shard_group_bm25_search(self.group, nat.ptr(t) if t.size else None, int(t.size), int(k),
                                                          nat.ptr(allow), ns, doc.ctypes.data, score.ctypes.data,
                                                          count.ctypes.data))
        return doc, score, int(count[0])

    def dense_scores(self, query) -> np.ndarray:
        """Not served by a group: raises `AnragError` (`ERR_UNSUPPORTED`)."""
        raise nat.AnragError(nat.ERR_UNSUPPORTED, "a shard group does not serve score dumps (anrag_dense_scores): use one index")

    def bm25_scores(self, term_ids: Sequence[int]) -> np.ndarray:
        """Not served by a group: raises `AnragError` (`ERR_UNSUPPORTED`)."""
        raise nat.AnragError(nat.ERR_UNSUPPORTED,
                             "a shard group does not serve score dumps (anrag_bm25_scores / get_scores): use one index")

    def enqueue_stats(self) -> tuple:
        """(exchange groups enqueued so far, host nanoseconds spent enqueuing them)."""
        n, ns = C.c_int64(0), C.c_int64(0)
        nat.check(self._lib.anrag_shard_group_debug_enqueue(self.group, C.byref(n), C.byref(ns)))
        return n.value, ns.value

    def hybrid_search(self, query, term_ids: Sequence[int], similarity_k: int, w_dense: float, w_bm25: float,
                      wrrf_k: float, top_n: int, allow_dense=None, allow_bm25=None):
        q = _f32(query).reshape(-1)
        assert q.size == self.dim
        t = np.ascontiguousarray(term_ids, dtype=np.int32)
        ad, nd = _allow_bytes(allow_dense)
        ab, nb = _allow_bytes(allow_bm25)
        out_id = np.empty(top_n, np.int64)
        out_score = np.empty(top_n, np.float64)
        count = np.zeros(1, np.int32)
        nat.check(self._lib.anrag_shard_group_hybrid_search(
            self.group, q.ctypes.data, nat.ptr(t) if t.size else None, int(t.size), int(similarity_k), float(w_dense),
            float(w_bm25), float(wrrf_k), int(top_n), nat.ptr(ad), nd, nat.ptr(ab), nb, out_id.ctypes.data,
            out_score.ctypes.data, count.ctypes.data))
        m = int(count[0])
        return out_id[:m], out_score[:m]

    def hybrid_search_batch(self, queries, term_lists: Sequence[Sequence[int]], similarity_k: int, w_dense: float,
                            w_bm25: float, wrrf_k: float, top_n: int, allow_dense=None, allow_bm25=None):
        """The pipelined batch = 1 kernels on every shard; row i equals `hybrid_search(queries[i], term_lists[i], ...)`."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        assert q.shape[1] == self.dim and len(term_lists) == nq
        offsets = np.zeros(nq + 1, dtype=np.int64)
        np.cumsum([len(t) for t in term_lists], out=offsets[1:])
        terms = (np.concatenate([np.asarray(t, dtype=np.int32).reshape(-1) for t in term_lists]).astype(np.int32)
                 if offsets[-1] else np.zeros(0, np.int32))
        terms = np.ascontiguousarray(terms)
        ad, nd = _allow_bytes(allow_dense)
        ab, nb = _allow_bytes(allow_bm25)
        out_id = np.empty((nq, top_n), np.int64)
        out_score = np.empty((nq, top_n), np.float64)
        count = np.zeros(nq, np.int32)
        nat.check(self._lib.anrag_shard_group_hybrid_search_batch(
            self.group, q.ctypes.data, nat.ptr(terms) if terms.size else None, offsets.ctypes.data, nq,
            int(similarity_k), float(w_dense), float(w_bm25), float(wrrf_k), int(top_n), nat.ptr(ad), nd, nat.ptr(ab), nb,
            out_id.ctypes.data, out_score.ctypes.data, count.ctypes.data))
        return out_id, out_score, count

    def info(self) -> dict:
        n, h = C.c_int32(), C.c_int64()
        rows = np.zeros(nat.GROUP_MAX_SHARDS + 1, np.int64)
        docs = np.zeros(nat.GROUP_MAX_SHARDS + 1, np.int64)
        nat.check(self._lib.anrag_shard_group_info(self.group, C.byref(n), rows.ctypes.data, docs.ctypes.data, C.byref(h)))
        s = n.value
        return dict(n_shards=s, dense_row_lo=rows[: s + 1].tolist(), bm25_doc_lo=docs[: s + 1].tolist(),
                    dense_rows=int(rows[s]), dense_dim=self.dim, bm25_docs=int(docs[s]), hbm_bytes=h.value)


class Index:
    """Owns an `anrag_index*`.  Not copyable; `close()` (or GC) frees the HBM."""

    def __init__(self, device: int = 0):
        self._lib = nat.load_library()
        h = C.c_void_p()
        nat.check(self._lib.anrag_index_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self.n_rows = 0
        self.dim = 0
        self.n_docs = 0

    # ------------------------------------------------------------------ lifetime
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.anrag_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self) -> C.c_void_p:
        if not self._h:
            raise nat.AnragError(-3, "index is closed")
        return self._h

    def set_streams(self, primary: int = 0, secondary: int = 0, fusion: int = 0) -> None:
        """Run on caller-owned HIP streams (e.g. torch.cuda.current_stream().cuda_stream); 0 = the index's own.
        Roles: include/anrag.h, anrag_index_set_streams."""
        nat.check(self._lib.anrag_index_set_streams(self.handle, primary or None, secondary or None, fusion or None))

    def sync(self) -> None:
        nat.check(self._lib.anrag_index_sync(self.handle))

    def wait_stream(self, stream: int = 0) -> None:
        """Order the index's streams after the work already enqueued on `stream` (e.g.
        torch.cuda.current_stream().cuda_stream): inputs produced and outputs allocated / filled there are safe to hand
        to the *_device entry points, no host sync."""
        nat.check(self._lib.anrag_index_wait_stream(self.handle, stream or None))

    def signal_stream(self, stream: int = 0) -> None:
        """Order `stream` after everything the index has enqueued: the caller's framework may read the results on
        that stream without a host sync."""
        nat.check(self._lib.anrag_index_signal_stream(self.handle, stream or None))

    # ------------------------------------------------------------------ dense
    def dense_load(self, embeddings, source_id=None, doc_id=None, doc_id_base: int = 0) -> None:
        """Upload the row-major fp32 corpus matrix (numpy array, or an (address, n, d) tuple of a
        device buffer such as a torch tensor's data_ptr()).  A device buffer must be COMPLETE when this is
        called (synchronise the stream that produced it): the library copies on its own stream."""
        if isinstance(embeddings, tuple):
            addr, n, d = embeddings
            keep = None
        else:
            keep = _f32(embeddings)
            assert keep.ndim == 2
            n, d = keep.shape
            addr = keep.ctypes.data
        src = None if source_id is None else np.ascontiguousarray(source_id, dtype=np.uint16)
        doc = None if doc_id is None else np.ascontiguousarray(doc_id, dtype=np.int64)
        assert src is None or src.shape == (n,)
        assert doc is None or doc.shape == (n,)
        nat.check(self._lib.anrag_dense_load(self.handle, addr, n, d, nat.ptr(src), nat.ptr(doc), int(doc_id_base)))
        self.n_rows, self.dim = int(n), int(d)

    def dense_search(self, queries, k: int, allow_source=None):
        """-> (doc [nq,k] int64, score [nq,k] float32, count [nq] int32); rank order, tail = -1/-inf."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q[None, :]
        if self.n_rows == 0:
            raise nat.AnragError(-3, "dense search before dense_load")
        assert q.shape[1] == self.dim, f"query dim {q.shape[1]} != index dim {self.dim}"
        nq = q.shape[0]
        allow, ns = _allow_bytes(allow_source)
        doc = np.empty((nq, k), np.int64)
        score = np.empty((nq, k), np.float32)
        count = np.empty(nq, np.int32)
        nat.check(self._lib.anrag_dense_search(self.handle, q.ctypes.data, nq, int(k), nat.ptr(allow), ns,
                                               doc.ctypes.data, score.ctypes.data, count.ctypes.data))
        return doc, score, count

    def dense_search_f64(self, query, k: int, allow_source=None):
        """One float64 query, scored in fp64 like numpy scores it (`anrag_dense_search_f64`).
        -> (doc [k] int64, score [k] float64, count)."""
        q = np.ascontiguousarray(query, dtype=np.float64).reshape(-1)
        assert q.size == self.dim, f"query dim {q.size} != index dim {self.dim}"
        allow, ns = _allow_bytes(allow_source)
        doc = np.empty(k, np.int64)
        score = np.empty(k, np.float64)
        count = np.zeros(1, np.int32)
        nat.check(self._lib.anrag_dense_search_f64(self.handle, q.ctypes.data, int(k), nat.ptr(allow), ns,
                                                   doc.ctypes.data, score.ctypes.data, count.ctypes.data))
        return doc, score, int(count[0])

    F64_SCAN_MAX_DIM = 3072

    def dense_f64_scan_serves(self) -> bool:
        """The fp64 list scan (and with it `hybrid_search_f64`) serves this index's dimension."""
        return self.n_rows > 0 and self.dim % 4 == 0 and self.dim <= self.F64_SCAN_MAX_DIM

    def set_dense_f64_scan(self, on: bool = True) -> None:
        """Route of `dense_search_f64`: the list scan where it serves (default), or the score array + sort for every k
        (`anrag_set_dense_f64_scan`).  Same ids and score bits on both."""
        nat.check(self._lib.anrag_set_dense_f64_scan(self.handle, 1 if on else 0))

    def dense_f64_stats(self) -> tuple:
        """(float64 queries answered by the list scan, by the score array + sort) since the index was created."""
        a, b = C.c_int64(0), C.c_int64(0)
        nat.check(self._lib.anrag_dense_f64_stats(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def rank_f64_tile_stats(self) -> tuple:
        """(float64 list queries of `queries_f64` legs scored by the fp64 tile kernel, by per-query score passes) since
        the index was created (`anrag_rank_f64_tile_stats`)."""
        a, b = C.c_int64(0), C.c_int64(0)
        nat.check(self._lib.anrag_rank_f64_tile_stats(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_dense_f64_prefilter(self, on: bool = True) -> None:
        """Route of the float64 dense leg while a prefilter form is built: the shadow prefilter with fp64 rescoring
        (default), or the list scan K1D (`anrag_set_dense_f64_prefilter`).  Same ids and score bits on both."""
        nat.check(self._lib.anrag_set_dense_f64_prefilter(self.handle, 1 if on else 0))

    def dense_f64_prefilter_stats(self) -> tuple:
        """(float64 queries answered through the prefilter, rows rescored for them) since the first such query after
        the last dense load."""
        q, s = C.c_int64(0), C.c_int64(0)
        nat.check(self._lib.anrag_dense_f64_prefilter_stats(self.handle, C.byref(q), C.byref(s)))
        return q.value, s.value

    def set_batched_precision(self, mode: str = "f32") -> None:
        """"f32": exact f32 MFMA (default).  "bf16x3": split-precision products on the bf16 matrix cores (scores within
        ~3e-5 of f32 for unit-norm vectors)."""
        nat.check(self._lib.anrag_set_batched_precision(self.handle, {"f32": 0, "bf16x3": 1}[mode]))

    def set_dense_prefilter(self, mode: int = -1) -> None:
        """Dense top-k route: -1 auto (the int8 prefilter past 1 GiB of fp32 corpus), 0 the fp32 scan, 1 the fp16
        prefilter + exact rescoring, 2 the int8 prefilter + exact rescoring.  Results are bit-identical in every mode."""
        nat.check(self._lib.anrag_set_dense_prefilter(self.handle, int(mode)))

    def dense_prefilter_stats(self) -> tuple:
        """(queries answered through the prefilter, rows rescored) since its current form was built."""
        q, s = C.c_int64(0), C.c_int64(0)
        nat.check(self._lib.anrag_dense_prefilter_stats(self.handle, C.byref(q), C.byref(s)))
        return q.value, s.value

    def set_scan_pairing(self, mode: int) -> None:
        """The int8 prefilter's pair pass and the pairing of single `hybrid_search_device` calls
        (`anrag_set_scan_pairing`): 0 off, 1 auto (default), 2 always hold a lone query for a partner (tests)."""
        nat.check(self._lib.anrag_set_scan_pairing(self.handle, int(mode)))

    def scan_pair_stats(self) -> tuple:
        """(pair passes, single passes, pending) of the int8 scan (`anrag_scan_pair_stats`); launches nothing."""
        a, b, p = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        nat.check(self._lib.anrag_scan_pair_stats(self.handle, C.byref(a), C.byref(b), C.byref(p)))
        return a.value, b.value, p.value

    def debug_prefilter_read(self, data: bool = True) -> dict:
        """The prefilter as built (`anrag_debug_prefilter_read`): form (0 off, 1 fp16, 2 int8), rows_per_wave and
        batch_rows of the scan and, with `data`, image ([n, d] float16 / int8) and meta ([n] / [n, 4] float32)."""
        form, rpw, rw = C.c_int32(0), C.c_int64(0), C.c_int32(0)
        nat.check(self._lib.anrag_debug_prefilter_read(self.handle, C.byref(form), C.byref(rpw), C.byref(rw), None, None))
        out = {"form": form.value, "rows_per_wave": rpw.value, "batch_rows": rw.value}
        if data and form.value:
            int8 = form.value == 2
            img = np.empty((self.n_rows, self.dim), np.int8 if int8 else np.float16)
            meta = np.empty((self.n_rows, 4) if int8 else (self.n_rows,), np.float32)
            nat.check(self._lib.anrag_debug_prefilter_read(self.handle, None, None, None, img.ctypes.data, meta.ctypes.data))
            out["image"], out["meta"] = img, meta
        return out

    PREFILTER_SENTINEL = 0x7FA5A5A5  # a NaN whose bits differ from the scan's own 0x7FC00000

    def debug_prefilter_bounds(self, queries, k: int, allow_source=None):
        """One shadow scan + threshold launch for 1..16 queries (`anrag_debug_prefilter_bounds`)
        -> (hi [nq, n_rows] float32, T [nq] float32); a row the scan did not write holds PREFILTER_SENTINEL's bits."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q[None, :]
        assert q.shape[1] == self.dim, f"query dim {q.shape[1]} != index dim {self.dim}"
        allow, ns = _allow_bytes(allow_source)
        hi = np.empty((q.shape[0], self.n_rows), np.float32)
        thr = np.empty(q.shape[0], np.float32)
        nat.check(self._lib.anrag_debug_prefilter_bounds(self.handle, q.ctypes.data, q.shape[0], int(k), nat.ptr(allow), ns,
                                                         self.PREFILTER_SENTINEL, hi.ctypes.data, thr.ctypes.data))
        return hi, thr

    def debug_prefilter_f64(self, query):
        """What the float64 prefilter route derives from `query` (`anrag_debug_prefilter_f64`)
        -> (q32 [dim] float32 as staged for the shadow scan, w, Emax)."""
        q = np.ascontiguousarray(query, dtype=np.float64).reshape(-1)
        assert q.size == self.dim, f"query dim {q.size} != index dim {self.dim}"
        q32 = np.empty(self.dim, np.float32)
        w, emax = C.c_double(0.0), C.c_double(0.0)
        nat.check(self._lib.anrag_debug_prefilter_f64(self.handle, q.ctypes.data, q32.ctypes.data, C.byref(w), C.byref(emax)))
        return q32, w.value, emax.value

    LIST_ROW_SENTINEL = 0xFFFFFFFE  # never a row (a shard holds at most 2^32 - 2), nor the empty slot's 0xFFFFFFFF

    def debug_dense_lists(self, queries, k: int, allow_source=None):
        """The per-wave lists a scan group of 1..16 queries leaves for the merge (`anrag_debug_dense_lists`)
        -> (scores [nq, n_lists, 64] float32, rows [nq, n_lists, 64] uint32); a slot no kernel wrote holds
        PREFILTER_SENTINEL's bits and LIST_ROW_SENTINEL, an empty slot (-inf, 0xFFFFFFFF)."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q[None, :]
        assert q.shape[1] == self.dim, f"query dim {q.shape[1]} != index dim {self.dim}"
        allow, ns = _allow_bytes(allow_source)
        n_lists = C.c_int32(0)
        nat.check(self._lib.anrag_debug_dense_lists(self.handle, None, 0, 0, None, 0, 0, 0, C.byref(n_lists), None, None))
        scores = np.empty((q.shape[0], n_lists.value, 64), np.float32)
        rows = np.empty((q.shape[0], n_lists.value, 64), np.uint32)
        nat.check(self._lib.anrag_debug_dense_lists(self.handle, q.ctypes.data, q.shape[0], int(k), nat.ptr(allow), ns,
                                                    self.PREFILTER_SENTINEL, self.LIST_ROW_SENTINEL, C.byref(n_lists),
                                                    scores.ctypes.data, rows.ctypes.data))
        return scores, rows

    def dense_scores(self, query) -> np.ndarray:
        q = _f32(query).reshape(-1)
        assert q.size == self.dim
        out = np.empty(self.n_rows, np.float32)
        nat.check(self._lib.anrag_dense_scores(self.handle, q.ctypes.data, out.ctypes.data))
        return out

    def dense_search_device(self, d_queries: int, n_queries: int, k: int, d_allow_bits: int, d_out: int) -> None:
        nat.check(self._lib.anrag_dense_search_device(self.handle, d_queries, n_queries, k, d_allow_bits or None, d_out))

    # ------------------------------------------------------------------ BM25
    def bm25_load(self, indptr, post_doc, post_tf, idf, doc_len, avgdl: float, k1: float, b: float,
                  source_id=None, doc_id=None, doc_id_base: int = 0) -> None:
        """Postings may be numpy arrays or (device address, count) tuples of int32 buffers already in HBM
        (e.g. torch tensors); indptr / idf / doc_len are host arrays."""
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        idf = np.ascontiguousarray(idf, dtype=np.float64)
        doc_len = np.ascontiguousarray(doc_len, dtype=np.int32)
        n_terms, n_docs = indptr.size - 1, doc_len.size

        def as_ptr(a):
            if isinstance(a, tuple):
                addr, count = a
                return None, int(addr), int(count)
            arr = np.ascontiguousarray(a, dtype=np.int32)
            return arr, arr.ctypes.data, int(arr.size)

        keep_d, pd_addr, pd_n = as_ptr(post_doc)
        keep_t, pt_addr, pt_n = as_ptr(post_tf)
        assert idf.size == n_terms and pd_n == pt_n == int(indptr[-1])
        src = None if source_id is None else np.ascontiguousarray(source_id, dtype=np.uint16)
        doc = None if doc_id is None else np.ascontiguousarray(doc_id, dtype=np.int64)
        nat.check(self._lib.anrag_bm25_load(self.handle, indptr.ctypes.data, n_terms, pd_addr or None,
                                            pt_addr or None, idf.ctypes.data, doc_len.ctypes.data, n_docs,
                                            float(avgdl), float(k1), float(b), nat.ptr(src), nat.ptr(doc),
                                            int(doc_id_base)))
        self.n_docs = int(n_docs)

    def bm25_search(self, term_ids: Sequence[int], k: int, allow_source=None):
        """-> (doc [k] int64, score [k] float64, count)."""
        t = np.ascontiguousarray(term_ids, dtype=np.int32)
        allow, ns = _allow_bytes(allow_source)
        doc = np.empty(k, np.int64)
        score = np.empty(k, np.float64)
        count = np.zeros(1, np.int32)
        nat.check(self._lib.anrag_bm25_search(self.handle, nat.ptr(t) if t.size else None, int(t.size), int(k),
                                              nat.ptr(allow), ns, doc.ctypes.data, score.ctypes.data,
                                              count.ctypes.data))
        return doc, score, int(count[0])

    def bm25_scores(self, term_ids: Sequence[int]) -> np.ndarray:
        t = np.ascontiguousarray(term_ids, dtype=np.int32)
        out = np.empty(self.n_docs, np.float64)
        nat.check(self._lib.anrag_bm25_scores(self.handle, nat.ptr(t) if t.size else None, int(t.size),
                                              out.ctypes.data))
        return out

    def bm25_geometry(self) -> dict:
        """How K3 cuts and serves the loaded corpus (`anrag_debug_bm25_geometry`): n_cus, part_docs, n_parts and the
        kernel form of a one-query launch / of a group launch (0 = 256 threads x 4 documents, 1 = 1,024 x 4 "wide",
        2 = 256 x 16 "tall").  Without BM25 data everything but n_cus is 0."""
        v = [C.c_int32() for _ in range(5)]
        nat.check(self._lib.anrag_debug_bm25_geometry(self.handle, *[C.byref(x) for x in v]))
        return dict(zip(("n_cus", "part_docs", "n_parts", "form_single", "form_group"), (x.value for x in v)))

    def bm25_search_group(self, term_lists: Sequence[Sequence[int]], k: int, allow_source=None):
        """Many BM25 queries in one call over `anrag_bm25_search_group_device` (16 queries per K3 launch, 1 <= k <= 64).
        -> (doc [nq, k] int64 (-1 padded), score [nq, k] float64 (-inf padded), count [nq] int32); row i equals
        `bm25_search(term_lists[i], k, allow_source)`.  A source filter needs the source ids given to `bm25_load`."""
        nq, k = len(term_lists), int(k)
        assert nq >= 1
        lens = np.ascontiguousarray([len(t) for t in term_lists], dtype=np.int32)
        off = np.zeros(nq + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        terms = (np.concatenate([np.asarray(t, dtype=np.int32).reshape(-1) for t in term_lists]).astype(np.int32)
                 if off[-1] else np.zeros(1, np.int32))
        bufs = []
        try:
            d_terms = self.device_alloc(terms.nbytes)
            bufs.append(d_terms)
            d_out = self.device_alloc(nq * k * nat.CANDIDATE_DTYPE.itemsize)
            bufs.append(d_out)
            self.to_device(d_terms, terms)
            d_allow = None
            if allow_source is not None:
                allow = np.flatnonzero(np.ascontiguousarray(allow_source, dtype=np.uint8))
                assert allow.size == 0 or allow[-1] < 65536
                bits = np.zeros(2048, dtype=np.uint32)  # bit s of word s / 32 = source s allowed
                np.bitwise_or.at(bits, allow >> 5, np.uint32(1) << (allow & 31).astype(np.uint32))
                d_allow = self.device_alloc(bits.nbytes)
                bufs.append(d_allow)
                self.to_device(d_allow, bits)
            p_terms = (C.c_void_p * nq)(*[d_terms + 4 * int(o) for o in off[:nq]])
            p_out = (C.c_void_p * nq)(*[d_out + i * k * nat.CANDIDATE_DTYPE.itemsize for i in range(nq)])
            nat.check(self._lib.anrag_bm25_search_group_device(self.handle, p_terms, lens.ctypes.data, nq, k, d_allow, p_out))
            self.sync()
            rec = np.empty((nq, k), dtype=nat.CANDIDATE_DTYPE)
            self.to_host(rec, d_out)
        finally:
            self.sync()
            for b in bufs:
                self.device_free(b)
        doc = np.ascontiguousarray(rec["doc"])
        return doc, np.ascontiguousarray(rec["score"]), (doc >= 0).sum(axis=1).astype(np.int32)

    # ------------------------------------------------------------------ fusion
    def wrrf(self, lists: Sequence[Sequence[int]], weights: Sequence[float], k: float, top_n: int):
        """-> (id [m] int64, score [m] float64), m = min(top_n, distinct ids)."""
        ids = np.ascontiguousarray(np.concatenate([np.asarray(l, dtype=np.int64) for l in lists])
                                   if len(lists) else np.empty(0, np.int64))
        lens = np.ascontiguousarray([len(l) for l in lists], dtype=np.int32)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        top_n = int(min(top_n, max(ids.size, 1)))
        out_id = np.empty(top_n, np.int64)
        out_score = np.empty(top_n, np.float64)
        count = np.zeros(1, np.int32)
        nat.check(self._lib.anrag_wrrf(self.handle, nat.ptr(ids) if ids.size else None, lens.ctypes.data,
                                       w.ctypes.data, len(lists), float(k), top_n, out_id.ctypes.data,
                                       out_score.ctypes.data, count.ctypes.data))
        m = int(count[0])
        return out_id[:m], out_score[:m]

    def hybrid_search(self, query, term_ids: Sequence[int], similarity_k: int, w_dense: float, w_bm25: float,
                      wrrf_k: float, top_n: int, allow_dense=None, allow_bm25=None):
        q = _f32(query).reshape(-1)
        assert q.size == self.dim
        t = np.ascontiguousarray(term_ids, dtype=np.int32)
        ad, nd = _allow_bytes(allow_dense)
        ab, nb = _allow_bytes(allow_bm25)
        out_id = np.empty(top_n, np.int64)
        out_score = np.empty(top_n, np.float64)
        count = np.zeros(1, np.int32)
        nat.check(self._lib.anrag_hybrid_search(self.handle, q.ctypes.data, nat.ptr(t) if t.size else None,
                                                int(t.size), int(similarity_k), float(w_dense), float(w_bm25),
                                                float(wrrf_k), int(top_n), nat.ptr(ad), nd, nat.ptr(ab), nb,
                                                out_id.ctypes.data, out_score.ctypes.data, count.ctypes.data))
        m = int(count[0])
        return out_id[:m], out_score[:m]

    def hybrid_search_f64(self, query, term_ids: Sequence[int], similarity_k: int, w_dense: float, w_bm25: float,
                          wrrf_k: float, top_n: int, allow_dense=None, allow_bm25=None):
        """`hybrid_search` for one float64 query, its dense leg scored in fp64 (`anrag_hybrid_search_f64`): equals
        `dense_search_f64` + `bm25_search` + `wrrf` in ids and fused-score bits.  Raises AnragError(-6) for a dimension
        the fp64 list scan does not serve (`dense_f64_scan_serves`)."""
        q = np.ascontiguousarray(query, dtype=np.float64).reshape(-1)
        assert self.n_rows == 0 or q.size == self.dim
        t = np.ascontiguousarray(term_ids, dtype=np.int32)
        ad, nd = _allow_bytes(allow_dense)
        ab, nb = _allow_bytes(allow_bm25)
        out_id = np.empty(top_n, np.int64)
        out_score = np.empty(top_n, np.float64)
        count = np.zeros(1, np.int32)
        nat.check(self._lib.anrag_hybrid_search_f64(self.handle, q.ctypes.data, nat.ptr(t) if t.size else None,
                                                    int(t.size), int(similarity_k), float(w_dense), float(w_bm25),
                                                    float(wrrf_k), int(top_n), nat.ptr(ad), nd, nat.ptr(ab), nb,
                                                    out_id.ctypes.data, out_score.ctypes.data, count.ctypes.data))
        m = int(count[0])
        return out_id[:m], out_score[:m]

    def hybrid_search_batch(self, queries, term_lists: Sequence[Sequence[int]], similarity_k: int, w_dense: float,
                            w_bm25: float, wrrf_k: float, top_n: int, allow_dense=None, allow_bm25=None):
        """Many hybrid queries in one call through the device pipeline (`anrag_hybrid_search_batch`).
        -> (ids [nq, top_n] int64 (-1 padded), fused scores [nq, top_n] float64, counts [nq] int32); row i equals
        `hybrid_search(queries[i], term_lists[i], ...)`."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        assert q.shape[1] == self.dim and len(term_lists) == nq
        offsets = np.zeros(nq + 1, dtype=np.int64)
        np.cumsum([len(t) for t in term_lists], out=offsets[1:])
        terms = (np.concatenate([np.asarray(t, dtype=np.int32).reshape(-1) for t in term_lists]).astype(np.int32)
                 if offsets[-1] else np.zeros(0, np.int32))
        terms = np.ascontiguousarray(terms)
        ad, nd = _allow_bytes(allow_dense)
        ab, nb = _allow_bytes(allow_bm25)
        out_id = np.empty((nq, top_n), np.int64)
        out_score = np.empty((nq, top_n), np.float64)
        count = np.zeros(nq, np.int32)
        nat.check(self._lib.anrag_hybrid_search_batch(
            self.handle, q.ctypes.data, nat.ptr(terms) if terms.size else None, offsets.ctypes.data, nq,
            int(similarity_k), float(w_dense), float(w_bm25), float(wrrf_k), int(top_n), nat.ptr(ad), nd, nat.ptr(ab), nb,
            out_id.ctypes.data, out_score.ctypes.data, count.ctypes.data))
        return out_id, out_score, count

    # ------------------------------------------------------------------ measurement
    def profile(self, on, kernels=None, every: int = 1) -> None:
        """Bracket launches with HIP events: on=True times every kernel id, `kernels=[ids]` only those,
        `every=n` only every n-th launch (a bracket costs ~10 us of stream time)."""
        mask = 0
        if on:
            mask = 0xFFFFFFFF if kernels is None else sum(1 << int(k) for k in kernels)
        nat.check(self._lib.anrag_profile_set_sampling(self.handle, max(1, int(every))))
        nat.check(self._lib.anrag_profile_enable(self.handle, mask))

    def profile_reset(self) -> None:
        nat.check(self._lib.anrag_profile_reset(self.handle))

    def profile_read(self, kernel_id: int) -> Tuple[float, int]:
        ms = C.c_double(0)
        n = C.c_int64(0)
        nat.check(self._lib.anrag_profile_read(self.handle, int(kernel_id), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_units(self, kernel_id: int) -> int:
        """Queries the timed launches of a kernel carried (K1 launches carry up to 8 for query groups)."""
        n = C.c_int64(0)
        nat.check(self._lib.anrag_profile_read_units(self.handle, int(kernel_id), C.byref(n)))
        return n.value

    def info(self) -> dict:
        a, d, b, p, h = C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        nat.check(self._lib.anrag_index_info(self.handle, C.byref(a), C.byref(d), C.byref(b), C.byref(p), C.byref(h)))
        return dict(dense_rows=a.value, dense_dim=d.value, bm25_docs=b.value, bm25_postings=p.value,
                    hbm_bytes=h.value)

    # raw device memory (for callers without torch)
    def device_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        nat.check(self._lib.anrag_device_alloc(self.handle, int(nbytes), C.byref(p)))
        return p.value

    def device_free(self, addr: int) -> None:
        nat.check(self._lib.anrag_device_free(self.handle, addr))

    def to_device(self, addr: int, arr: np.ndarray) -> None:
        a = np.ascontiguousarray(arr)
        nat.check(self._lib.anrag_copy_to_device(self.handle, addr, a.ctypes.data, a.nbytes))

    def to_host(self, arr: np.ndarray, addr: int) -> None:
        assert arr.flags["C_CONTIGUOUS"]
        nat.check(self._lib.anrag_copy_to_host(self.handle, arr.ctypes.data, addr, arr.nbytes))
