"""Host model of the sharded path's global tail (select.hip: `merge_candidates_kernel`, `merge_fuse_kernel`) and of the
id-list fusion with padding (`wrrf_in_block`, wrrf.hip, sort_select.hip), and the planted inputs both are tested on
(tests/test_shard_merge_model_cpu.py on the CPU, tests/test_gpu_shard_merge.py and tests/test_gpu_fusion.py on the GPU).

Records are what the kernels read: int64 [..., 2], word 0 the bits of the fp64 score, word 1 the doc id; doc < 0 is
padding and carries -inf.  Everything is exact: ids, score BITS and counts, no tolerance anywhere.

What the merge requires of its input is `check_contract`: inside a list the records are in (score desc, doc asc) order
and padding is a tail.  The kernels walk a list only until its first record that does not enter the running top k
(`kernel_walk` is that walk, literally); under the contract this equals the sort, outside it does not.
"""
import numpy as np

NEG_INF = float("-inf")
NEG_INF_BITS = int(np.array([NEG_INF]).view(np.int64)[0])
POISON = (float("inf"), 7)        # what lies outside the addressed blocks of a planted buffer: doc 7 must never come out
SENTINEL = (-123456.75, -4242)    # what the output buffers hold before a call
RANGE = 1000                      # doc ids of list l: [base + l * RANGE, base + (l + 1) * RANGE), as under row sharding
BIG_BASE = 3 * 10 ** 12           # doc ids above 2^32


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def pack(pairs, k: int) -> np.ndarray:
    """[(score, doc)] -> int64 [k, 2], padded with (-inf, -1)."""
    rec = np.empty((k, 2), np.int64)
    rec[:, 0] = NEG_INF_BITS
    rec[:, 1] = -1
    if len(pairs):
        rec[: len(pairs), 0] = bits([s for s, _ in pairs])
        rec[: len(pairs), 1] = [d for _, d in pairs]
    return rec


def unpack(rec) -> list:
    rec = np.ascontiguousarray(rec, dtype=np.int64).reshape(-1, 2)
    return list(zip(rec[:, 0].copy().view(np.float64).tolist(), rec[:, 1].tolist()))


# --------------------------------------------------------------------------- the operations
def gather(records, n_lists: int, k: int, stride: int, offset: int) -> list:
    """The real records (doc >= 0) among the first k of every list: [(score, doc, list, position)]."""
    flat = np.ascontiguousarray(records, dtype=np.int64).reshape(-1, 2)
    out = []
    for l in range(n_lists):
        base = l * stride + offset
        for p, (s, d) in enumerate(unpack(flat[base: base + k])):
            if d >= 0:
                out.append((s, d, l, p))
    return out


def merge(records, n_lists: int, k: int, stride: int, offset: int) -> np.ndarray:
    """Global top k by (score desc, doc asc) -> int64 [k, 2], padded with (-inf, -1)."""
    cands = gather(records, n_lists, k, stride, offset)
    cands.sort(key=lambda c: (-c[0], c[1]))
    return pack([(c[0], c[1]) for c in cands[:k]], k)


def wrrf_padded(lists, weights, k) -> list:
    """`oracle.ref_search.weighted_reciprocal_rank_fusion` for id lists in which a negative id is padding: it keeps its
    rank position and contributes nothing.  -> [(id, fused score)], stable sort by score descending."""
    rrf = {}
    for ranked, w in zip(lists, weights):
        for rank, doc_id in enumerate(ranked, start=1):
            if doc_id < 0:
                continue
            rrf[doc_id] = rrf.get(doc_id, 0.0) + w * (1 / (k + rank))
    return sorted(rrf.items(), key=lambda x: x[1], reverse=True)


def fused_out(fused: list, top_n: int):
    """-> (ids [top_n] padded with -1, score bits [top_n] padded with -inf, count = min(top_n, distinct))."""
    fused = fused[:top_n]
    rec = pack([(s, i) for i, s in fused], top_n)
    return rec[:, 1].copy(), rec[:, 0].copy(), len(fused)


def merge_fuse(records, n_lists: int, k: int, stride: int, w_dense: float, w_bm25: float, wrrf_k: float, top_n: int,
               n_queries: int):
    """-> (ids [n_queries, top_n], score bits [n_queries, top_n], counts [n_queries]); rows are padded past the count."""
    ids = np.empty((n_queries, top_n), np.int64)
    sbits = np.empty((n_queries, top_n), np.int64)
    counts = np.empty(n_queries, np.int32)
    for q in range(n_queries):
        dense = merge(records, n_lists, k, stride, q * 2 * k)[:, 1].tolist()
        bm25 = merge(records, n_lists, k, stride, q * 2 * k + k)[:, 1].tolist()
        ids[q], sbits[q], counts[q] = fused_out(wrrf_padded([dense, bm25], [w_dense, w_bm25], wrrf_k), top_n)
    return ids, sbits, counts


def check_contract(records, n_lists: int, k: int, stride: int, offsets) -> None:
    """What merge_candidates_kernel / merge_fuse_kernel require of every list they read."""
    flat = np.ascontiguousarray(records, dtype=np.int64).reshape(-1, 2)
    for offset in offsets:
        for l in range(n_lists):
            base = l * stride + offset
            rows = unpack(flat[base: base + k])
            assert len(rows) == k, (l, offset, "list runs past the buffer")
            n_real = sum(d >= 0 for _, d in rows)
            assert all(d >= 0 for _, d in rows[:n_real]), (l, offset, "padding before a real record")
            assert not any(s != s for s, _ in rows), (l, offset, "NaN score")
            keys = [(-s, d) for s, d in rows[:n_real]]
            assert all(a < b for a, b in zip(keys, keys[1:])), (l, offset, "not in (score desc, doc asc) order")


def kernel_walk(records, n_lists: int, k: int, stride: int, offset: int, thr_lane=None) -> np.ndarray:
    """DocTopK as select.hip runs it: 64 slots best first, list after list, record after record until the first that does
    not beat the slot `thr_lane` (k - 1 in the kernel; readlane takes the lane number modulo 64).  -> int64 [k, 2]."""
    flat = np.ascontiguousarray(records, dtype=np.int64).reshape(-1, 2)
    thr_lane = (k - 1 if thr_lane is None else thr_lane) % 64

    def beats(s, d, ts, td):
        if td < 0:
            return d >= 0
        if d < 0:
            return False
        return s > ts or (s == ts and d < td)

    slots = [(NEG_INF, -1)] * 64
    for l in range(n_lists):
        base = l * stride + offset
        for s, d in unpack(flat[base: base + k]):
            if not beats(s, d, *slots[thr_lane]):
                break
            at = sum(beats(ss, sd, s, d) for ss, sd in slots)  # the slots ahead of the candidate are a prefix
            slots = (slots[:at] + [(s, d)] + slots[at:])[:64]
    return pack([(s, d) for s, d in slots[:k] if d >= 0], k)


# --------------------------------------------------------------------------- planted halves
# A "half" is one modality of one query: n_lists lists of at most k (score, doc) pairs, in contract.
def _docs(rng, l: int, n: int, base: int, part=None) -> np.ndarray:
    """n distinct doc ids of list l's range; part 0 / 1 = from its lower / upper half only."""
    lo, hi = (0, RANGE) if part is None else ((0, RANGE // 2) if part == 0 else (RANGE // 2, RANGE))
    return base + l * RANGE + lo + rng.permutation(hi - lo)[:n]


def _ordered(scores, docs) -> list:
    return sorted(zip([float(s) for s in scores], [int(d) for d in docs]), key=lambda c: (-c[0], c[1]))


def half_distinct(rng, k, n_lists, base=100, part=None, lens=None):
    """Distinct random scores, disjoint doc ranges per list."""
    lens = [k] * n_lists if lens is None else lens
    scores = rng.permutation(4 * k * n_lists)[: sum(lens)] / 8.0 - k  # distinct across the whole half, exact in fp64
    out, at = [], 0
    for l, n in enumerate(lens):
        out.append(_ordered(scores[at: at + n], _docs(rng, l, n, base, part)))
        at += n
    return out


def half_ties(rng, k, n_lists, base=100):
    """Scores from {0, 0.5, 1, 2, +inf}: most of the top k is decided by the doc id.  For k <= 2 every list leads with
    +inf, or the few records that there are would seldom tie across lists."""
    levels = np.array([0.0, 0.5, 1.0, 2.0, np.inf])
    out = []
    for l in range(n_lists):
        s = levels[rng.integers(0, 5, size=k)]
        if k <= 2:
            s[0] = np.inf
        out.append(_ordered(s, _docs(rng, l, k, base)))
    return out


def half_short(rng, k, n_lists, base=100):
    """0 .. k-1 real records per list."""
    return half_distinct(rng, k, n_lists, base, lens=[int(rng.integers(0, k)) for _ in range(n_lists)])


def half_few(rng, k, n_lists, base=100):
    """Fewer than k real records in total."""
    lens = [0] * n_lists
    for _ in range(k - 1):
        lens[int(rng.integers(0, n_lists))] += 1
    return half_distinct(rng, k, n_lists, base, lens=lens)


def half_empty(rng, k, n_lists, base=100):
    return [[] for _ in range(n_lists)]


def half_last(rng, k, n_lists, base=100):
    """All winners in the last list."""
    h = half_distinct(rng, k, n_lists, base)
    h[-1] = [(s + 10.0 * k * n_lists, d) for s, d in h[-1]]
    return h


def half_one_each(rng, k, n_lists, base=100, shuffle=False):
    """Exactly one winner from each of the first k lists: list l's first record beats every list's second."""
    h = half_distinct(rng, k, n_lists, base)
    order = rng.permutation(n_lists) if shuffle else np.arange(n_lists)
    for l in range(min(k, n_lists)):
        h[l][0] = (1000.0 - float(order[l]), h[l][0][1])
    return h


def block(dense, bm25, k: int) -> np.ndarray:
    """Two halves -> one query's records on every list: int64 [n_lists, 2k, 2]."""
    return np.stack([np.concatenate([pack(d, k), pack(b, k)]) for d, b in zip(dense, bm25)])


def _case(name, family, rec, **kw):
    return dict(name=name, family=family, rec=rec, **kw)


def cases_for(k: int, n_lists: int, seed: int = 0) -> list:
    """Every planted query for one (k, n_lists): dicts with `name`, `family`, `rec` int64 [n_lists, 2k, 2] and, for a
    permutation of an earlier case's lists, `same_as` = that case's position."""
    rng = np.random.default_rng([seed, k, n_lists])
    out = []
    # distinct scores
    for i in range(3):
        out.append(_case(f"distinct{i}", "distinct", block(half_distinct(rng, k, n_lists), half_distinct(rng, k, n_lists), k)))
    out.append(_case("distinct_big", "distinct",
                     block(half_distinct(rng, k, n_lists, BIG_BASE), half_distinct(rng, k, n_lists, BIG_BASE), k)))
    # heavy ties: shard order, then two permutations of the lists
    for i in range(3):
        rec = block(half_ties(rng, k, n_lists), half_ties(rng, k, n_lists), k)
        first = len(out)
        out.append(_case(f"ties{i}", "ties", rec, order="shard"))
        if n_lists > 1:
            out.append(_case(f"ties{i}_reversed", "ties", rec[::-1].copy(), same_as=first, order="permuted"))
            perm = np.roll(np.arange(n_lists), 1) if n_lists == 2 else rng.permutation(n_lists)
            while n_lists > 2 and (np.array_equal(perm, np.arange(n_lists)) or np.array_equal(perm, np.arange(n_lists)[::-1])):
                perm = rng.permutation(n_lists)
            out.append(_case(f"ties{i}_permuted", "ties", rec[perm].copy(), same_as=first, order="permuted"))
    # short and empty lists
    out.append(_case("short0", "short", block(half_short(rng, k, n_lists), half_short(rng, k, n_lists), k)))
    out.append(_case("short1", "short", block(half_short(rng, k, n_lists), half_distinct(rng, k, n_lists), k)))
    out.append(_case("empty", "short", block(half_empty(rng, k, n_lists), half_empty(rng, k, n_lists), k)))
    out.append(_case("few", "short", block(half_few(rng, k, n_lists), half_few(rng, k, n_lists), k)))
    out.append(_case("last", "short", block(half_last(rng, k, n_lists), half_last(rng, k, n_lists), k)))
    out.append(_case("one_each", "short", block(half_one_each(rng, k, n_lists), half_one_each(rng, k, n_lists, shuffle=True), k)))
    # fusion
    for i in range(2):
        dense = half_distinct(rng, k, n_lists)
        # the first half of every dense list is in the BM25 list too, ahead of the rest; the lists' leaders keep their order,
        # so that the two merged lists share their first doc even at k = 1
        both = [[(200.0 + s, d) if j == 0 else (100.0 + float(rng.integers(0, 4)), d)
                 for j, (s, d) in enumerate(lst[: (len(lst) + 1) // 2])] for lst in dense]
        extra = half_distinct(rng, k, n_lists, lens=[k // 2] * n_lists)
        bm25 = []
        for b, e in zip(both, extra):
            seen = {d for _, d in b}
            bm25.append(_ordered(*zip(*(b + [(s, d) for s, d in e if d not in seen]))) if b or e else [])
        out.append(_case(f"both{i}", "both", block(dense, bm25, k)))
    for i in range(2):
        out.append(_case(f"disjoint{i}", "disjoint",
                         block(half_distinct(rng, k, n_lists, part=0), half_distinct(rng, k, n_lists, part=1), k)))
    out.append(_case("no_bm25", "no_bm25", block(half_distinct(rng, k, n_lists), half_empty(rng, k, n_lists), k)))
    return out


def slab(cases: list, k: int, n_lists: int, extra: int, lead: int = 5):
    """The cases as the queries of one launch inside a poisoned buffer -> (int64 [lead + n_lists * stride, 2], stride, lead):
    list l's slab starts `lead + l * stride` records in and holds len(cases) blocks of 2k, then `extra` records of poison."""
    nq = len(cases)
    stride = nq * 2 * k + extra
    buf = np.empty((lead + n_lists * stride, 2), np.int64)
    buf[:, 0] = bits([POISON[0]])[0]
    buf[:, 1] = POISON[1]
    for q, c in enumerate(cases):
        for l in range(n_lists):
            at = lead + l * stride + q * 2 * k
            buf[at: at + 2 * k] = c["rec"][l]
    return buf, stride, lead


# Shapes of the packed launches.  (16, 16) is there for "one winner from each of k lists".
PACK_K = (1, 2, 25, 63, 64)
PACK_LISTS = (1, 2, 3, 8, 16)
PACKS = [(k, n) for k in PACK_K for n in PACK_LISTS] + [(16, 16)]
WEIGHTS = ((5.0, 1.0, 40.0), (1.0, 1.0, 60.0), (5.0, 0.0, 40.0))  # (w_dense, w_bm25, wrrf_k)


def top_ns(k: int) -> tuple:
    return (1, 10, 2 * k, 128)


def pack_extra(p: int) -> int:
    """Records of poison behind the payload of every list's slab in pack p."""
    return (19, 38, 7)[p % 3]


def pack_launches(p: int, k: int) -> list:
    """The three (w_dense, w_bm25, wrrf_k, top_n) a pack is launched with: every weight set, top_n rotating."""
    t = top_ns(k)
    return [WEIGHTS[j] + (t[(p + j) % 4],) for j in range(3)]


# --------------------------------------------------------------------------- planted inputs of the list fusion
def wrrf_device_cases(seed: int = 3) -> list:
    """anrag_wrrf_device: dicts with dense / bm25 records (int64 [n, 2]); padding records sit in the MIDDLE of both lists
    and about a third of the BM25 docs are dense docs."""
    rng = np.random.default_rng(seed)
    out = []
    for n_dense, n_bm25 in ((1, 0), (25, 25), (64, 64), (40, 0), (512, 512), (1000, 24)):
        dd = (10 + rng.permutation(4 * n_dense)[:n_dense]).astype(np.int64)
        bd = (10 + 4 * n_dense + rng.permutation(4 * max(n_bm25, 1))[:n_bm25]).astype(np.int64)
        shared = np.flatnonzero(rng.random(n_bm25) < 0.33)[:n_dense]
        bd[shared] = rng.permutation(dd)[: shared.size]
        for ids in (dd, bd):
            if ids.size > 2:
                ids[rng.random(ids.size) < 0.2] = -1
                ids[ids.size // 2] = -1
        mk = lambda ids: np.stack([bits(np.where(ids < 0, NEG_INF, rng.random(ids.size))), ids], axis=1)
        out.append(dict(n_dense=n_dense, n_bm25=n_bm25, dense=mk(dd), bm25=mk(bd)))
    return out


def split3(m: int) -> tuple:
    a = m // 3
    return a, a, m - 2 * a


def wrrf_switch_lists(m: int, seed: int = 0, base: int = 0) -> list:
    """M ids over 3 lists, distinct inside a list, about a third of every list shared with the others."""
    rng = np.random.default_rng([seed, m])
    pool = base + rng.permutation(2 * m + 8)
    lens = split3(m)
    common = pool[: max(lens) // 3]
    lists, at = [], len(common)
    for n in lens:
        own = pool[at: at + n]
        at += n
        ids = np.concatenate([common[: n // 3], own[: n - n // 3]])
        lists.append([int(x) for x in rng.permutation(ids)])
    assert [len(l) for l in lists] == list(lens)
    return lists


def wrrf_negative_lists(m: int, seed: int = 5) -> list:
    """The same 3 x 300 entries (negative ids scattered through them), the last list then filled up with neutral ids
    to M entries in total: the content's fused scores do not depend on M."""
    rng = np.random.default_rng(seed)
    lists = []
    for l in range(3):
        ids = rng.permutation(700)[:300].astype(np.int64)
        ids[rng.random(300) < 0.25] = -1 - l
        ids[[0, 150, 299]] = -7
        lists.append(ids.tolist())
    lists[2] = lists[2] + list(range(10 ** 6, 10 ** 6 + m - 900))
    return lists
