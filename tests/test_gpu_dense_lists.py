"""GPU: the per-wave lists of the dense top-k and their merges, with planted winners.

Every dense answer with k <= 64 is a scan that leaves one sorted 64-slot list per wave, and a merge of those lists
(merge_lists, wave_topk.hpp) that pulls four entries per list at once and walks a list further only in a loop of its
own.  On a random corpus the winners spread evenly over the lists, so the end-to-end tests never fill a list with
winners.  These tests look at the lists themselves (anrag_debug_dense_lists) and put the winners where they want them:
  a. the lists of one scan partition the allowed rows, are sorted, and hold dense_scores' bits;
  b. at k below what a wave owns, slots [0, k) of every list are the top k of the rows that wave owns;
  c. planted winners -- a whole list of them, several lists, the first and the last list, the first and the last rows,
     bit-equal duplicates, a source filter, large norms -- through every consumer of the lists.
The row -> list map (`owner`) is read from a dump, never modelled: it depends on the shape of the corpus alone.
Reference: the fp64 dot product and oracle.ref_search.canonical_topk.  Planted scores are at least 1e-3 apart and at
least 0.2 above every ordinary row, so ids are compared exactly; a score s against its fp64 value s64 by
|s - s64| <= gamma_d sum |q_i e_i|, gamma_d = d 2^-24 / (1 - d 2^-24) (a sum of d products, each term rounded at most d
times in any order of summation; Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_ROW = np.uint32(0xFFFFFFFF)
SCORE_SENTINEL = np.uint32(0x7FA5A5A5)  # Index.PREFILTER_SENTINEL
ROW_SENTINEL = np.uint32(0xFFFFFFFE)    # Index.LIST_ROW_SENTINEL
LIST_LEN = 64
LISTS = 1024  # one list per scan wave, four waves per CU: what the corpora below are sized for
U = 2.0 ** -24

# one dimension of every ScanShape of scan_dispatch (dense_scan_common.hpp), and one only the generic kernel takes
SHAPE_DIMS = (256, 512, 768, 1024, 1536, 2048, 3072, 4096, 128, 384, 640, 896, 64, 192, 320, 448)
GENERIC_DIM = 100
PREFILTER_DIMS = (256, 512, 768, 1024, 1536, 2048)  # prefilter_dispatch (dense_prefilter.hip)


@pytest.fixture(scope="module")
def Index():
    from anrag.index import Index

    return Index


def gamma(d):
    return d * U / (1.0 - d * U)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _ref_scores(e, q):
    """fp64 dot products and sum |q_i e_i| of every row, in blocks (no fp64 copy of the corpus)"""
    q64 = q.astype(np.float64)
    aq = np.abs(q64)
    s, a = np.empty(len(e)), np.empty(len(e))
    for i in range(0, len(e), 8192):
        c = e[i:i + 8192].astype(np.float64)
        s[i:i + 8192] = c @ q64
        a[i:i + 8192] = np.abs(c) @ aq
    return s, a


def _ref_planted(e, rows, q):
    """... of the planted rows, one evaluation per distinct vector: a blocked fp64 matrix product may sum equal rows in
    different orders (its last bit then depends on where a row sits), and equal rows must tie in the reference"""
    uniq, inv = np.unique(e[rows], axis=0, return_inverse=True)
    s, a = _ref_scores(uniq, q)
    inv = np.asarray(inv).reshape(-1)
    return s[inv], a[inv]


def _rows_for(dim, per_list):
    return per_list * LISTS + 3


@functools.lru_cache(maxsize=1)
def _corpus(dim, n):
    """unit rows, a unit query, and the query's fp64 scores: computed once per shape, never written to"""
    rng = np.random.default_rng(100_000 + 7 * dim + n)
    e = rng.standard_normal((n, dim), dtype=np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    q = rng.standard_normal(dim).astype(np.float32)
    q /= np.float32(np.linalg.norm(q.astype(np.float64)))
    q2 = rng.standard_normal(dim).astype(np.float32)
    q2 /= np.float32(np.linalg.norm(q2.astype(np.float64)))
    s64, a64 = _ref_scores(e, q)
    e.setflags(write=False)
    return e, q, q2, s64, a64


class Aim:
    """unit rows with a chosen score against q: t q^ + sqrt(1 - t^2) w, w a unit vector orthogonal to q.  The same t
    gives the same vector, so equal targets are bit-equal rows (bit-equal scores)."""

    def __init__(self, q, seed):
        self.q = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64))
        self.rng = np.random.default_rng(seed)
        self.made = {}

    def row(self, t):
        t = float(t)
        if t not in self.made:
            w = self.rng.standard_normal(self.q.size)
            w -= (w @ self.q) * self.q
            w /= np.linalg.norm(w)
            self.made[t] = (t * self.q + np.sqrt(1.0 - t * t) * w).astype(np.float32)
        return self.made[t]


def _dump(idx, queries, k, allow=None):
    s, r = idx.debug_dense_lists(queries, k, allow_source=allow)
    assert s.shape == r.shape and s.shape[2] == LIST_LEN
    return s, r


def _owner_of(rows, n):
    """owner[row] = the list a row sits in, from the rows of one k = 64 dump; -1: in no list"""
    owner = np.full(n, -1, np.int64)
    lists = np.broadcast_to(np.arange(rows.shape[0])[:, None], rows.shape)
    real = (rows != NO_ROW) & (rows != ROW_SENTINEL)
    r = rows[real].astype(np.int64)
    assert r.size == 0 or r.max() < n, f"a list holds row {r.max()} of a corpus of {n}"
    assert np.unique(r).size == r.size, "a row sits in two slots"
    owner[r] = lists[real]
    return owner


def _check_lists_well_formed(tag, s, r, k, n):
    """slots [0, k) of every list: written, real rows first in (score desc, row asc), then (-inf, NO_ROW)"""
    s, r = s[:, :k], r[:, :k]
    assert not (_bits(s) == SCORE_SENTINEL).any() and not (r == ROW_SENTINEL).any(), (
        f"{tag}: slots no kernel wrote in lists {np.flatnonzero(((_bits(s) == SCORE_SENTINEL) | (r == ROW_SENTINEL)).any(axis=1))[:8]}")
    empty = r == NO_ROW
    assert np.all(np.isneginf(s[empty])), f"{tag}: an empty slot with a score"
    assert np.all(r[~empty] < n), f"{tag}: a row past the corpus"
    assert not np.isnan(s).any(), f"{tag}: NaN score"
    assert np.all(empty[:, 1:] >= empty[:, :-1]), f"{tag}: an empty slot ahead of a real one"
    both = ~empty[:, 1:]
    a, b = s[:, :-1].astype(np.float64), s[:, 1:].astype(np.float64)
    in_order = (a > b) | ((a == b) & (r[:, :-1] < r[:, 1:]))
    bad = both & ~in_order
    assert not bad.any(), f"{tag}: lists {np.flatnonzero(bad.any(axis=1))[:8]} are not sorted by (score desc, row asc)"


def _expected_lists(owner, dev, n_lists, allowed=None):
    """per list the rows it owns (the allowed ones) by (device score desc, row asc), the first 64: [n_lists, 64]"""
    rows = np.flatnonzero(owner >= 0) if allowed is None else np.flatnonzero(allowed & (owner >= 0))
    order = np.lexsort((rows, -dev[rows].astype(np.float64), owner[rows]))
    r = rows[order]
    o = owner[r]
    start = np.searchsorted(o, np.arange(n_lists))
    pos = np.arange(r.size) - start[o]
    keep = pos < LIST_LEN
    exp_r = np.full((n_lists, LIST_LEN), NO_ROW, np.uint32)
    exp_s = np.full((n_lists, LIST_LEN), -np.inf, np.float32)
    exp_r[o[keep], pos[keep]] = r[keep]
    exp_s[o[keep], pos[keep]] = dev[r[keep]]
    return exp_s, exp_r


def _check_selection(tag, s, r, k, exp):
    exp_s, exp_r = exp
    wrong = (r[:, :k] != exp_r[:, :k]) | (_bits(s[:, :k]) != _bits(exp_s[:, :k]))
    if wrong.any():
        li = int(np.flatnonzero(wrong.any(axis=1))[0])
        raise AssertionError(f"{tag}: {int(wrong.any(axis=1).sum())} lists differ from the top {k} of their rows; list {li}: "
                             f"got {r[li, :k].tolist()} want {exp_r[li, :k].tolist()}")


def _allowed_rows(src, allow):
    return np.ones(src.size, bool) if allow is None else allow[src].astype(bool)


# ---------------------------------------------------------------- a. the lists partition the corpus
def _ab_rows(dim):
    # 3,072 / 4,096-d: fewer rows, every list still owns 13 (part b plants 12 duplicates in one)
    return _rows_for(dim, 13 if dim >= 3072 else 40)


@pytest.mark.parametrize("dim", SHAPE_DIMS + (GENERIC_DIM,))
def test_lists_partition_the_corpus(Index, dim):
    n = _ab_rows(dim)
    e, q, _, s64, a64 = _corpus(dim, n)
    src = ((np.arange(n) * 7 + np.arange(n) // 5) % 5).astype(np.uint16)
    allow = np.array([1, 0, 1, 1, 0], np.uint8)
    with Index(0) as idx:
        idx.set_dense_prefilter(0)
        idx.dense_load(e, source_id=src)
        dev = idx.dense_scores(q)
        owners = []
        for flt in (None, allow):
            tag = f"D={dim} n={n} filter={'off' if flt is None else 'on'}"
            s, r = _dump(idx, q, 64, flt)
            s, r = s[0], r[0]
            assert 1 <= s.shape[0] <= LISTS
            _check_lists_well_formed(tag, s, r, 64, n)
            owner = _owner_of(r, n)
            allowed = _allowed_rows(src, flt)
            per = np.bincount(owner[owner >= 0], minlength=s.shape[0])
            print(f"{tag}: {s.shape[0]} lists, rows per list {per.min()} .. {per.max()}")
            assert per.max() <= LIST_LEN, f"{tag}: this shape gives a wave more than 64 rows: the test cannot see them all"
            assert np.array_equal(owner >= 0, allowed), (
                f"{tag}: rows in no list {np.flatnonzero(allowed & (owner < 0))[:8]}, "
                f"disallowed rows in a list {np.flatnonzero(~allowed & (owner >= 0))[:8]}")
            real = r != NO_ROW
            rr = r[real].astype(np.int64)
            assert np.array_equal(_bits(s[real]), _bits(dev[rr])), f"{tag}: a list score is not dense_scores' bits"
            err = np.abs(s[real].astype(np.float64) - s64[rr])
            bound = gamma(dim) * a64[rr]
            print(f"{tag}: max |s - s64| / bound = {np.max(err / bound):.4f}")
            assert np.all(err <= bound), f"{tag}: score outside the fp64 bound"
            owners.append(owner)
        keep = owners[1] >= 0
        assert np.array_equal(owners[0][keep], owners[1][keep]), "the row -> list map changed with the filter"


# ---------------------------------------------------------------- b. per-list selection below what a wave owns
@pytest.mark.parametrize("dim", SHAPE_DIMS + (GENERIC_DIM,))
def test_per_list_selection_below_what_a_wave_owns(Index, dim):
    n = _ab_rows(dim)
    base, q, _, _, _ = _corpus(dim, n)
    with Index(0) as idx:
        idx.set_dense_prefilter(0)
        idx.dense_load(base)
        _, r = _dump(idx, q, 64)
        n_lists = r.shape[1]
        owner = _owner_of(r[0], n)
        assert (owner >= 0).all()
        # three planted lists: every arrival the new head, every arrival the new last, 12 bit-equal rows
        aim = Aim(q, dim)
        e = base.copy()
        rising, falling, dups = 1, n_lists // 2 + 3, n_lists - 2
        m = np.flatnonzero(owner == rising)
        for j, row in enumerate(m):
            e[row] = aim.row(0.5 + 1e-3 * j)
        m = np.flatnonzero(owner == falling)
        for j, row in enumerate(m):
            e[row] = aim.row(0.5 + 1e-3 * (m.size - j))
        m = np.flatnonzero(owner == dups)
        assert m.size >= 12
        for row in m[:12]:
            e[row] = aim.row(0.9)
        idx.dense_load(e)
        qs = np.stack([q, -q, q])  # for -q the rising list falls: and queries 1, 2 start behind a wrapped scan
        dev = [idx.dense_scores(x) for x in (q, -q)]
        assert np.unique(_bits(dev[0][m[:12]])).size == 1, "equal rows, different score bits"
        exp = [_expected_lists(owner, d, n_lists) for d in dev]
        for k in (1, 4, 5, 63):
            s, r = _dump(idx, qs, k)
            for i, which in enumerate((0, 1, 0)):
                tag = f"D={dim} k={k} query {i}"
                _check_lists_well_formed(tag, s[i], r[i], k, n)
                _check_selection(tag, s[i], r[i], k, exp[which])


# ---------------------------------------------------------------- c. planted winners through every consumer
C_PER_LIST = {768: 80, 384: 80, 3072: 8, GENERIC_DIM: 80}
_owner_cache = {}


def _owner_map(Index, e, q):
    """owner[row] where a wave owns more than 64 rows: one dump per source class of ~20 rows per list"""
    n, dim = e.shape
    if (n, dim) in _owner_cache:
        return _owner_cache[n, dim]
    classes = max(1, -(-n // (LISTS * 20)))
    src = np.random.default_rng(n + dim).integers(0, classes, n).astype(np.uint16)
    owner = np.full(n, -1, np.int64)
    with Index(0) as idx:
        idx.set_dense_prefilter(0)
        idx.dense_load(e, source_id=src)
        for c in range(classes):
            allow = np.zeros(classes, np.uint8)
            allow[c] = 1
            _, r = _dump(idx, q, 64, allow)
            part = _owner_of(r[0], n)
            assert np.array_equal(part >= 0, src == c), f"class {c}: the dump does not hold exactly its rows"
            owner[part >= 0] = part[part >= 0]
    assert (owner >= 0).all()
    _owner_cache[n, dim] = owner
    return owner


@functools.lru_cache(maxsize=1)
def _bm25():
    """a small BM25 leg over documents 0 .. 299 (document id = dense row) and the oracle's list for one query"""
    from anrag.bm25_index import Bm25Index
    from oracle.ref_bm25 import BM25Okapi

    rng = np.random.default_rng(44)
    corpus = [[f"t{j}" for j in rng.integers(0, 60, int(rng.integers(4, 20)))] for _ in range(300)]
    toks = ["t3", "t17", "t41"]
    return Bm25Index(corpus, k1=1.7, b=0.83, epsilon=0.05), BM25Okapi(corpus, k1=1.7, b=0.83, epsilon=0.05).get_scores(toks), toks


def _spread_lists(i):
    """13 lists that ONE lane of a 4-wave merge meets in different chunks: a lane sees lists l, l + 256, l + 512,
    l + 768 (1,024 lists hold no longer run), so 13 lists are four such runs, the last one cut"""
    return 37 + 256 * (i % 4) + i // 4


def _placement(name, owner, n, rng):
    """-> dict(k, rows, ranks (0 = the best planted score; equal ranks = bit-equal rows), reject (rows a source filter
    drops), scale)"""
    n_lists = int(owner.max()) + 1
    members = lambda l: np.flatnonzero(owner == l)
    out = dict(reject=np.zeros(0, np.int64), scale=False)
    kind, _, arg = name.partition(":")
    if kind == "one-list":            # all k winners in one list, in a scattered order of arrival
        k = int(arg)
        out.update(k=k, rows=members(417)[:k], ranks=rng.permutation(k))
    elif kind == "rising":            # k + 8 high rows in one list: every arrival the new best
        rows = members(233)[:72]
        out.update(k=64, rows=rows, ranks=np.arange(72)[::-1])
    elif kind == "falling":           # ... every arrival the new last
        out.update(k=64, rows=members(234)[:72], ranks=np.arange(72))
    elif kind in ("13-adjacent", "13-apart"):
        lists = [600 + i for i in range(13)] if kind == "13-adjacent" else [_spread_lists(i) for i in range(13)]
        rows, ranks = [], []
        for i, l in enumerate(lists):
            m = members(l)
            rows += m[[0, 7, 19, 33, m.size - 1]].tolist()
            ranks += [j * 13 + i for j in range(5)]
        out.update(k=64, rows=np.array(rows), ranks=np.array(ranks))
    elif kind == "list-0":
        out.update(k=6, rows=members(0)[[0, 1, 2, 5, 9, -1]], ranks=rng.permutation(6))
    elif kind == "last-list":
        m = members(n_lists - 1)  # (every list of these corpora owns rows: part a's partition)
        assert m.size >= 6
        out.update(k=6, rows=m[[0, 1, 2, 3, -2, -1]], ranks=rng.permutation(6))
    elif kind == "last-rows":
        out.update(k=4, rows=np.array([n - 1, n - 2, n - 3, n - 4]), ranks=np.array([2, 0, 3, 1]))
    elif kind == "first-rows":
        out.update(k=4, rows=np.array([0, 1, 2, 3]), ranks=np.array([1, 3, 0, 2]))
    elif kind == "duplicates":        # 70 bit-equal rows, 40 / 30 over two lists: the answer is the 64 lowest rows
        out.update(k=64, rows=np.concatenate([members(810)[:40], members(305)[:30]]), ranks=np.zeros(70, np.int64))
    elif kind == "filtered":          # every second planted row is rejected by the source filter
        rows = members(512)[:66]
        out.update(k=33, rows=rows, ranks=rng.permutation(66), reject=rows[1::2])
    elif kind == "scaled":            # rows of norm 30, a query of norm 5
        out.update(k=33, rows=members(417)[:33], ranks=rng.permutation(33), scale=True)
    else:
        raise KeyError(name)
    assert len(set(out["rows"].tolist())) == len(out["rows"]) == len(out["ranks"])
    return out


FULL_SET = ["one-list:1", "one-list:4", "one-list:5", "one-list:6", "one-list:33", "one-list:64", "rising", "falling",
            "13-adjacent", "13-apart", "list-0", "last-list", "last-rows", "first-rows", "duplicates", "filtered", "scaled"]
CASES = [(768, p) for p in FULL_SET] + [(384, p) for p in FULL_SET] + [(3072, "one-list:6"), (GENERIC_DIM, "one-list:64")]


def _allow_bitmap(allow):
    bits = np.zeros(2048, np.uint32)
    for s in np.flatnonzero(allow):
        bits[s >> 5] |= np.uint32(1) << np.uint32(s & 31)
    return bits


class _Device:
    """queries and result records in HBM for the device entry points"""

    def __init__(self, idx, queries, k, allow, n_out):
        from anrag import _native as nat

        self.idx, self.k, self.n_out, self.dtype = idx, k, n_out, nat.CANDIDATE_DTYPE
        self.stride = queries.shape[1] * 4
        self.q = idx.device_alloc(queries.nbytes)
        idx.to_device(self.q, queries)
        self.allow = 0
        if allow is not None:
            self.allow = idx.device_alloc(2048 * 4)
            idx.to_device(self.allow, _allow_bitmap(allow))
        self.out = idx.device_alloc(n_out * k * 16)

    def clear(self):
        self.idx.to_device(self.out, np.zeros(self.n_out * self.k, self.dtype))

    def search(self, qi, n_queries, slot):
        self.idx.dense_search_device(self.q + qi * self.stride, n_queries, self.k, self.allow, self.out + slot * self.k * 16)

    def read(self):
        self.idx.sync()
        got = np.empty((self.n_out, self.k), self.dtype)
        self.idx.to_host(got, self.out)
        return got

    def close(self):
        for p in (self.q, self.allow, self.out):
            if p:
                self.idx.device_free(p)


def _same(tag, want, doc, score, count=None):
    """ids, count and fp32 score bits of route 1"""
    w_doc, w_bits = want
    doc = np.asarray(doc).reshape(-1)
    assert doc.tolist() == w_doc.tolist(), f"{tag}: ids {doc.tolist()} != {w_doc.tolist()}"
    assert np.array_equal(_bits(np.asarray(score, np.float64).astype(np.float32)), w_bits), f"{tag}: score bits differ"
    if count is not None:
        assert int(count) == int((w_doc >= 0).sum()), f"{tag}: count {int(count)}"


@pytest.mark.parametrize("dim,name", CASES, ids=[f"{d}-{p}" for d, p in CASES])
def test_planted_winners_through_every_consumer(Index, dim, name):
    from oracle import ref_search

    n = _rows_for(dim, C_PER_LIST[dim])
    base, q, q2, s64, a64 = _corpus(dim, n)
    owner = _owner_map(Index, base, q)
    n_lists = int(owner.max()) + 1
    rng = np.random.default_rng(dim * 131 + FULL_SET.index(name))
    pl = _placement(name, owner, n, rng)
    k, rows = pl["k"], pl["rows"]
    # planted scores: 1.5e-3 apart, the lowest 0.25 above the best ordinary row
    floor = float(s64.max()) + 0.25
    targets = floor + 1.5e-3 * (pl["ranks"].max() - pl["ranks"])
    assert targets.max() < 0.97, "no room for the planted scores above this corpus"
    aim = Aim(q, dim * 1000 + FULL_SET.index(name))
    e = base.copy()
    for row, t in zip(rows, targets):
        e[row] = aim.row(t)
    qq, qq2 = q, q2
    if pl["scale"]:
        e *= np.float32(30.0)
        qq, qq2 = q * np.float32(5.0), q2 * np.float32(5.0)
        ref, ref_abs = _ref_scores(e, qq)
    else:
        ref, ref_abs = s64.copy(), a64.copy()
    ref[rows], ref_abs[rows] = _ref_planted(e, rows, qq)
    src = np.zeros(n, np.uint16)
    src[pl["reject"]] = 1
    allow = np.array([1, 0], np.uint8) if pl["reject"].size else None
    allowed = _allowed_rows(src, allow)
    ordinary = np.ones(n, bool)
    ordinary[rows] = False
    gap = 0.2 * (150.0 if pl["scale"] else 1.0)
    assert ref[rows].min() >= ref[ordinary].max() + gap
    distinct = np.unique(ref[rows])
    assert distinct.size == 1 or np.diff(distinct).min() >= 1e-3
    want_rows = ref_search.canonical_topk(ref, k, None if allow is None else allowed)
    assert want_rows.size == k and set(want_rows.tolist()) <= set(rows.tolist())
    bi, bm_scores, toks = _bm25()
    bm_list = ref_search.core_bm25_search(bm_scores, None, k, None, canonical=True).tolist()
    top_n = min(2 * k, 128)
    fused = ref_search.weighted_reciprocal_rank_fusion([(want_rows.tolist(), "d"), (bm_list, "BM25")],
                                                       {"d": 5.0, "BM25": 1.0}, 40.0)[:top_n]
    modes = (0, 1, 2) if dim in PREFILTER_DIMS else (0,)
    ran = []
    with Index(0) as idx:
        idx.set_dense_prefilter(0)
        idx.dense_load(e, source_id=src if allow is not None else None)
        idx.bm25_load(bi.indptr, bi.post_doc, bi.post_tf, bi.idf, bi.doc_len, bi.avgdl, bi.k1, bi.b)
        dev = idx.dense_scores(qq)
        exp = _expected_lists(owner, dev, n_lists, allowed)
        queries = np.stack([qq, qq2, qq])
        dv = _Device(idx, queries, k, allow, 16)
        try:
            want = other = None
            for mode in modes:
                idx.set_dense_prefilter(mode)
                tag = f"D={dim} {name} k={k} mode={mode}"
                # the lists this placement leaves
                s, r = _dump(idx, qq, k, allow)
                s, r = s[0], r[0]
                _check_lists_well_formed(tag, s, r, k, n)
                if mode == 0:
                    _check_selection(tag, s, r, k, exp)
                    held = np.isin(r[:, :k], want_rows).sum(axis=1)
                    print(f"{tag}: winners per list, max {held.max()}, lists with winners {int((held > 0).sum())}")
                else:
                    real = r[:, :k] != NO_ROW
                    rr = r[:, :k][real].astype(np.int64)
                    assert np.unique(rr).size == rr.size, f"{tag}: a row in two lists"
                    assert allowed[rr].all(), f"{tag}: a rejected row in a list"
                    assert np.array_equal(_bits(s[:, :k][real]), _bits(dev[rr])), f"{tag}: not K1's score bits"
                    assert set(want_rows.tolist()) <= set(rr.tolist()), f"{tag}: the lists miss rows of the true top k"
                # 1. one query, then sync
                doc, score, cnt = idx.dense_search(qq, k, allow)
                if want is None:
                    assert doc[0].tolist() == want_rows.tolist(), f"{tag}: route 1 ids {doc[0].tolist()} != {want_rows.tolist()}"
                    err = np.abs(score[0].astype(np.float64) - ref[want_rows])
                    bound = gamma(dim) * ref_abs[want_rows]
                    print(f"{tag}: route 1 max |s - s64| / bound = {np.max(err / bound):.4f}")
                    assert np.all(err <= bound), f"{tag}: route 1 score outside the fp64 bound"
                    assert np.array_equal(_bits(score[0]), _bits(dev[want_rows]))
                    want = (doc[0].copy(), _bits(score[0]).copy())
                    d2, s2, _ = idx.dense_search(qq2, k, allow)
                    other = (d2[0].copy(), _bits(s2[0]).copy())
                _same(f"{tag} route 1", want, doc[0], score[0], cnt[0])
                # 2. single device queries back to back: with up to four scan lanes, eight put a deferred merge into a
                #    later launch of every lane; the last merge of a lane is launched by the sync
                dv.clear()
                for i in range(8):
                    dv.search(0, 1, i)
                got = dv.read()
                for i in range(8):
                    _same(f"{tag} route 2 query {i}", want, got[i]["doc"], got[i]["score"])
                # 3. three queries in one host call
                doc, score, cnt = idx.dense_search(queries, k, allow)
                for i, w in enumerate((want, other, want)):
                    _same(f"{tag} route 3 query {i}", w, doc[i], score[i], cnt[i])
                # 4. three queries in one device call: one scan launch, one grouped tail
                dv.clear()
                dv.search(0, 3, 0)
                got = dv.read()
                for i, w in enumerate((want, other, want)):
                    _same(f"{tag} route 4 query {i}", w, got[i]["doc"], got[i]["score"])
                # 6. hybrid, against the oracle's fusion of the reference list and the oracle's BM25 list
                out_id, out_score = idx.hybrid_search(qq, bi.term_ids(toks), k, 5.0, 1.0, 40.0, top_n, allow, None)
                assert out_id.tolist() == [i for i, _ in fused], f"{tag}: route 6 ids"
                assert out_score.tolist() == [x for _, x in fused], f"{tag}: route 6 fused scores"
                ran.append(mode)
            if 2 in modes:
                # 5. the lanes again across a change of route with no sync of the caller's: the pending merges of the
                #    fp32 scans are launched by the drain, those of mode 2 ride in its rescore launches
                idx.set_dense_prefilter(0)
                dv.clear()
                for i in range(8):
                    dv.search(0, 1, i)
                idx.set_dense_prefilter(2)
                for i in range(8, 16):
                    dv.search(0, 1, i)
                got = dv.read()
                for i in range(16):
                    _same(f"D={dim} {name} k={k} route 5 query {i}", want, got[i]["doc"], got[i]["score"])
        finally:
            dv.close()
    print(f"D={dim} {name} k={k}: routes 1-4, 6 in modes {ran}" + (", route 5" if 2 in modes else ""))


@pytest.mark.parametrize("k", [6, 33])
def test_shard_group_winners_in_one_list_of_the_second_shard(Index, k):
    """7. a group of two shards on one device: every winner sits in ONE list of the second shard's scan (that shard's own
    row -> list map, read from an index loaded with its block); the group's default prefilter setting."""
    from anrag.index import ShardGroup, group_bounds
    from oracle import ref_search

    dim = 768
    n = _rows_for(dim, C_PER_LIST[dim])
    base, q, _, s64, a64 = _corpus(dim, n)
    lo = group_bounds(n, 2)[1]
    with Index(0) as half:
        half.set_dense_prefilter(0)
        half.dense_load(base[lo:])
        _, r = _dump(half, q, 64)
        owner = _owner_of(r[0], n - lo)
    assert (owner >= 0).all()
    rows = lo + np.flatnonzero(owner == 401)[:k]
    assert rows.size == k
    rng = np.random.default_rng(k)
    targets = float(s64.max()) + 0.25 + 1.5e-3 * rng.permutation(k)
    aim = Aim(q, 7000 + k)
    e = base.copy()
    for row, t in zip(rows, targets):
        e[row] = aim.row(t)
    ref = s64.copy()
    ref[rows], _ = _ref_planted(e, rows, q)
    want_rows = ref_search.canonical_topk(ref, k)
    assert set(want_rows.tolist()) == set(rows.tolist())
    with Index(0) as idx:
        idx.set_dense_prefilter(0)
        idx.dense_load(e)
        doc, score, cnt = idx.dense_search(q, k)
    assert doc[0].tolist() == want_rows.tolist()
    want = (doc[0].copy(), _bits(score[0]).copy())
    with ShardGroup([0, 0]) as g:
        g.dense_load(e)
        for nq in (1, 3):
            gd, gs, gc = g.dense_search(np.stack([q] * nq), k)
            for i in range(nq):
                _same(f"group k={k} {nq} queries [{i}]", want, gd[i], gs[i], gc[i])
    print(f"shard group [0, 0] k={k}: winners in list 401 of shard 1, 1 and 3 queries")


def test_random_corpus_spreads_its_winners(Index):
    """What the placements above are for: on test_random_dense_vs_oracle's (5000, 768) corpus no list holds more of the
    top 64 than the merge's first batch of loads covers.  The figure is printed; the lists' union is checked."""
    n, d = 5000, 768
    rng = np.random.default_rng(n * 31 + d)
    e = rng.standard_normal((n, d), dtype=np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    qs = rng.standard_normal((3, d), dtype=np.float32)
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    with Index(0) as idx:
        idx.set_dense_prefilter(0)
        idx.dense_load(e)
        s, r = _dump(idx, qs, 64)
        doc, _, _ = idx.dense_search(qs, 64)
    worst = 0
    for i in range(3):
        held = np.isin(r[i], doc[i]).sum(axis=1)
        assert held.sum() == 64, "the lists do not hold the top 64"
        worst = max(worst, int(held.max()))
    print(f"(5000, 768) random corpus, {r.shape[1]} lists: at most {worst} of the top 64 in one list (3 queries)")
