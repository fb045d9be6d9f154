"""Numpy model of K3's partitioning and per-partition selection (bm25.hip), and the planted corpora its three kernel
forms are tested on (tests/test_gpu_bm25_forms.py).

The kernel cuts the documents into partitions, deals a partition's documents to 64 groups, takes the group best of rank
k - 1 as a bound tau, keeps the documents not behind tau ("survivors") and picks one of three paths by their number: at
most 64 are ranked by counting, up to `surv_cap` go through wave 0's insertion / merge network, more take the general
path (every wave selects, `block_merge` combines).  The tail merges the partitions' lists.  Random scores never leave
the first two paths, so the corpora here PLANT what reaches each path; every builder records what it aims at in its
case, and tests/test_k3_select_model_cpu.py holds each case to it under this model, so that the GPU test cannot pass on
an input that misses its path.

A corpus is raw CSR (indptr, post_doc, post_tf, idf, doc_len, source_id): a few dozen terms over mostly empty documents.
"""
import numpy as np

# bm25.hip's geometry, read back from the source by tests/test_k3_select_model_cpu.py
K_FREQUENT_DF = 1024   # kFrequentDf: terms with at least this many postings carry a per-partition offset table
K_TERM_BATCH = 128     # kTermBatch: query terms per term table
K_ROUND_TERMS = 16     # kRoundTerms: terms per gather round at most
K_MAX_PART_DOCS = 4096  # kMaxPartDocs
FORMS = {"small": (256, 4), "wide": (1024, 4), "tall": (256, 16)}  # name -> (threads, documents per thread)
FORM_ID = {"small": 0, "wide": 1, "tall": 2}                       # as anrag_debug_bm25_geometry reports them
K1, B = 1.7, 0.83


def round_slots(threads: int, dpt: int) -> int:
    return 24 if (threads, dpt) == (256, 16) else 16


def surv_cap(threads: int) -> int:
    return 1024 if threads == 1024 else 512


def rot(threads: int) -> int:
    return 4 if threads == 1024 else 16


def partitioning(n_docs: int, n_cus: int, per_cu: int = 1):
    """bm25_load's rule -> (part_docs, n_parts)."""
    pd = -(-n_docs // (n_cus * per_cu))
    pd = (pd + 255) // 256 * 256
    pd = max(256, min(K_MAX_PART_DOCS, pd))
    return pd, -(-n_docs // pd)


def forms_of(part_docs: int) -> dict:
    """The form a launch of one query / of a group of queries takes."""
    if part_docs <= 1024:
        return dict(single="small", group="small")
    return dict(single="wide", group="tall")


def group_of(i, threads: int):
    """The group of document i of a partition's slice."""
    i = np.asarray(i)
    return ((i & 63) - rot(threads) * (i >> 6)) & 63


def path_of(n_surv: int, threads: int) -> str:
    return "count" if n_surv <= 64 else ("network" if n_surv <= surv_cap(threads) else "general")


def select_model(scores, k: int, threads: int, allowed=None, row0: int = 0) -> dict:
    """One partition: group bests, tau, survivors, path and the sorted list (its first k entries)."""
    s = np.asarray(scores, dtype=np.float64)
    i = np.arange(len(s))
    if allowed is not None:
        i = i[np.asarray(allowed, dtype=bool)]
    order = i[np.lexsort((i, -s[i]))]  # (score descending, row ascending): the kernel's `beats`
    g = group_of(order, threads)
    first = np.sort(np.unique(g, return_index=True)[1])  # a group's best is its first document in that order
    bests = order[first]                                 # ... and the bests are in rank order already
    if len(bests) >= k:
        tau = int(bests[k - 1])
        n_surv = int(np.flatnonzero(order == tau)[0]) + 1  # the documents tau does not beat
    else:
        tau = None  # fewer than k groups hold a document: no bound, everything allowed survives
        n_surv = len(order)
    top = order[:min(k, n_surv)]
    return dict(tau=None if tau is None else (float(s[tau]), row0 + tau), group_bests=row0 + bests, n_surv=n_surv,
                path=path_of(n_surv, threads), rows=row0 + top, scores=s[top])


def merge_model(lists, k: int):
    """The tail: the partitions' lists under (score descending, row ascending) -> rows."""
    rows = np.concatenate([np.asarray(l["rows"], dtype=np.int64) for l in lists])
    sc = np.concatenate([l["scores"] for l in lists])
    return rows[np.lexsort((rows, -sc))][:k]


def topk_model(scores, k: int, part_docs: int, threads: int, allowed=None):
    """Every partition selected, the lists merged -> (rows, per-partition results)."""
    n = len(scores)
    parts = []
    for lo in range(0, n, part_docs):
        hi = min(n, lo + part_docs)
        parts.append(select_model(scores[lo:hi], k, threads, None if allowed is None else allowed[lo:hi], lo))
    return merge_model(parts, k), parts


# ---------------------------------------------------------------------------------------------------- corpora
SRC_NONE, SRC_SPRINKLE, SRC_FEW, SRC_FIRST_CASE = 0, 1, 2, 3  # source ids of the filter cases


class Corpus:
    """Raw CSR under construction: n_docs = (n_cus - 1) * part_docs + last, i.e. n_cus partitions of part_docs documents,
    the last one `last` long."""

    def __init__(self, n_cus: int, part_docs: int, last: int, seed: int):
        assert 1 <= last <= part_docs
        self.n_cus, self.part_docs, self.last = n_cus, part_docs, last
        self.n_docs = (n_cus - 1) * part_docs + last
        self.n_parts = n_cus
        self.rng = np.random.default_rng(seed)
        self.doc_len = self.rng.integers(1, 200, self.n_docs).astype(np.int32)
        self.source_id = np.zeros(self.n_docs, dtype=np.uint16)
        self._terms = []
        self.cases = []
        self.arrays = None

    def part_len(self, p: int) -> int:
        return self.last if p == self.n_parts - 1 else self.part_docs

    def add_term(self, docs, tf, idf=None) -> int:
        docs = np.asarray(docs, dtype=np.int64).reshape(-1)
        tf = np.broadcast_to(np.asarray(tf, dtype=np.int32), docs.shape)
        assert len(np.unique(docs)) == len(docs) and (docs >= 0).all() and (docs < self.n_docs).all()
        o = np.argsort(docs, kind="stable")
        self._terms.append((docs[o].astype(np.int32), tf[o].astype(np.int32),
                            float(self.rng.uniform(0.5, 3.0)) if idf is None else float(idf)))
        return len(self._terms) - 1

    def random_tf(self, n: int):
        return self.rng.integers(1, 60, n).astype(np.int32)

    def finish(self):
        df = np.array([len(t[0]) for t in self._terms], dtype=np.int64)
        self.arrays = dict(indptr=np.concatenate([[0], np.cumsum(df)]).astype(np.int64),
                           post_doc=np.concatenate([t[0] for t in self._terms]).astype(np.int32),
                           post_tf=np.concatenate([t[1] for t in self._terms]).astype(np.int32),
                           idf=np.array([t[2] for t in self._terms], dtype=np.float64), doc_len=self.doc_len,
                           avgdl=float(self.doc_len.mean()), k1=K1, b=B)
        self.df = df
        self.n_vocab = len(df)
        return self

    def allow_vector(self, sources):
        """uint8 [n_sources] for a tuple of allowed source ids (None: no filter)."""
        if sources is None:
            return None
        a = np.zeros(int(self.source_id.max()) + 2, dtype=np.uint8)
        a[list(sources)] = 1
        return a

    def known_terms(self, terms):
        """The query as the oracle's CSR scorer takes it: ids outside the vocabulary are unknown tokens (-1)."""
        return [int(t) if 0 <= t < self.n_vocab else -1 for t in terms]

    def allowed_docs(self, sources):
        return None if sources is None else self.allow_vector(sources).astype(bool)[self.source_id]


def _pick(c: Corpus, part: int, threads: int, groups, min_stripe: int, count: int):
    """`count` documents of partition `part` in the given groups, on stripes (64 consecutive rows) >= min_stripe."""
    i = np.arange(64 * min_stripe, c.part_len(part))
    i = i[np.isin(group_of(i, threads), np.asarray(list(groups)))]
    assert len(i) >= count, (len(i), count)
    return part * c.part_docs + np.sort(c.rng.choice(i, size=count, replace=False))


def slots_for(length: int, threads: int, k: int, min_stripe: int) -> int:
    """Documents of a `length`-long partition in groups 0 .. k-2 on stripes >= min_stripe."""
    i = np.arange(64 * min_stripe, length)
    return int((group_of(i, threads) < k - 1).sum())


def selection_grid(length: int, threads: int, ks=(10, 25, 64)):
    """(k, survivors) a partition of `length` documents can hold with the planting of `plant_selection`: survivor counts
    on both sides of the boundaries 64 | 65 and surv_cap | surv_cap + 1."""
    cap = surv_cap(threads)
    return [(k, n) for k in ks for n in (64, 65, cap, cap + 1) if 1 <= n - k <= slots_for(length, threads, k, 1)]


def plant_selection(c: Corpus, form: str, k: int, n_surv: int, part: int, variant: str) -> dict:
    """One marker term held by P = n_surv - k documents of partition `part`, in groups 0 .. k-2 on stripes >= 1; everything
    else scores 0.  The k - 1 planted group bests lead, group k - 1's best is row k - 1 with score 0, so tau = (0, row
    k - 1) and the survivors are the P planted documents and rows 0 .. k-1.  variant "equal": one tf and one doc_len, so
    that the row rule decides everything; "distinct": every planted document its own tf.
    k = 1: tau is the best document itself and it alone survives."""
    threads = FORMS[form][0]
    if k == 1:
        docs, n_surv = _pick(c, part, threads, range(64), 1, 30), 1
    else:
        docs = _pick(c, part, threads, range(k - 1), 1, n_surv - k)
    if variant == "equal":
        c.doc_len[docs] = 17
        tf = np.full(len(docs), 3, dtype=np.int32)
    else:
        tf = (c.rng.permutation(len(docs)) + 1).astype(np.int32)
    case = dict(kind="select", name=f"{form}-k{k}-s{n_surv}-p{part}-{variant}", form=form, k=k, n_surv=n_surv, part=part,
                path=path_of(n_surv, threads), variant=variant, terms=[c.add_term(docs, tf)], allow=None)
    c.cases.append(case)
    return case


def filter_grid(length: int, threads: int, ks=(10, 25, 64)):
    cap = surv_cap(threads)
    return [(k, n) for k in ks for n in (64, 65, cap, cap + 1) if n <= slots_for(length, threads, k, 0)]


def plant_filters(c: Corpus, specs) -> None:
    """specs: (form, k, n_allowed).  Each case gets a partition and a source id of its own: n_allowed documents of the
    partition, all in groups 0 .. k-2, carry the source, so that under the filter fewer than k groups hold a document, tau
    stays unset and all n_allowed survive.  A random half of them holds the case's marker term.  Source SRC_SPRINKLE: two
    documents in each of up to 60 other partitions, in every marker term (the merge has other lists to weigh); source
    SRC_FEW: 7 documents in the whole corpus, 4 of them in every marker term."""
    n = c.n_parts
    assert n >= len(specs) + 8, "too few partitions for one per filter case"
    mid = n // 2
    order = [0, n - 1] + [p for d in range(1, n) for p in (mid - d, mid + d - 1) if 0 < p < n - 1]
    seen, parts = set(), []
    for p in order:
        if p not in seen:
            seen.add(p)
            parts.append(p)
    case_parts, rest = parts[:len(specs)], sorted(parts[len(specs):])
    sprinkle = np.concatenate([p * c.part_docs + c.rng.choice(c.part_len(p), size=2, replace=False) for p in rest[3:63]])
    few = np.concatenate([p * c.part_docs + c.rng.choice(c.part_len(p), size=m, replace=False)
                          for p, m in zip(rest[:3], (3, 3, 1))])
    c.source_id[sprinkle] = SRC_SPRINKLE
    c.source_id[few] = SRC_FEW
    c.few_docs = np.sort(few)
    extra = np.concatenate([sprinkle, few[:4]])
    for j, ((form, k, n_allowed), part) in enumerate(zip(specs, case_parts)):
        threads = FORMS[form][0]
        docs = _pick(c, part, threads, range(k - 1), 0, n_allowed)
        c.source_id[docs] = SRC_FIRST_CASE + j
        holders = np.sort(c.rng.choice(docs, size=max(1, n_allowed // 2), replace=False))
        term = c.add_term(np.concatenate([holders, extra]), c.random_tf(len(holders) + len(extra)))
        c.cases.append(dict(kind="filter", name=f"{form}-k{k}-allowed{n_allowed}-p{part}", form=form, k=k, n_surv=n_allowed,
                            part=part, path=path_of(n_allowed, threads), terms=[term],
                            allow=(SRC_FIRST_CASE + j, SRC_SPRINKLE)))


def plant_tail(c: Corpus) -> None:
    """Marker terms for the tail's merge (k = 64): every winner in one partition (one list feeds rounds 4 .. 63); one
    winner in each of 64 or more partitions; winners only in the last list of a wave's chunk of 64 lists."""
    n, pd = c.n_parts, c.part_docs
    p = n // 3
    docs = p * pd + c.rng.choice(c.part_len(p), size=80, replace=False)
    c.cases.append(dict(kind="tail", name="one-partition", k=64, parts=[p], terms=[c.add_term(docs, np.arange(1, 81))],
                        allow=None))
    parts = np.arange(min(n, 80))
    docs = parts * pd + c.rng.integers(0, [c.part_len(int(q)) for q in parts])
    c.cases.append(dict(kind="tail", name="one-per-partition", k=64, parts=parts.tolist(),
                        terms=[c.add_term(docs, c.rng.permutation(len(docs)) + 1)], allow=None))
    parts = [q for q in (63, 127, 191, 255) if q < n]
    if parts:
        docs = np.concatenate([q * pd + c.rng.choice(c.part_len(q), size=20, replace=False) for q in parts])
        c.cases.append(dict(kind="tail", name="last-list-of-a-chunk", k=64, parts=parts,
                            terms=[c.add_term(docs, c.rng.permutation(len(docs)) + 1)], allow=None))


def plant_short_last(c: Corpus) -> None:
    """Winners inside the last (short) partition, and straddling the last two."""
    n, pd, last = c.n_parts, c.part_docs, c.last
    lo = (n - 1) * pd
    inside = lo + c.rng.choice(last, size=min(last, 40), replace=False)
    weak = c.rng.choice(lo, size=100, replace=False)  # elsewhere, tf 1 against tf >= 5
    c.cases.append(dict(kind="short", name="inside-last", parts=[n - 1],
                        terms=[c.add_term(np.concatenate([inside, weak]),
                                          np.concatenate([c.rng.integers(5, 60, len(inside)), np.ones(100, np.int64)]))],
                        allow=None))
    straddle = np.arange(lo - 40, lo + min(last, 40))
    c.cases.append(dict(kind="short", name="straddle-last-two", parts=[n - 2, n - 1],
                        terms=[c.add_term(straddle, c.random_tf(len(straddle)))], allow=None))


def plant_scoring(c: Corpus, part: int) -> dict:
    """Terms on the edges of the gather rounds, around partition `part` (tf and doc_len vary everywhere):
    whole: three terms held by every document of the partition; df1023 / df1024: either side of the partition-table
    threshold; run<r>: r consecutive postings inside the partition plus 1,100 elsewhere (table terms); rare<r>: r postings
    in the partition and nothing else (scanned whole), for r < K_FREQUENT_DF; zero: idf 0; one_slot: 20 terms of 30 .. 60
    postings.  -> the term ids by name; the queries are in `scoring_queries`."""
    pd, n = c.part_docs, c.n_docs
    lo, ln = part * pd, c.part_len(part)
    t = {}
    t["whole"] = [c.add_term(lo + np.arange(ln), c.random_tf(ln)) for _ in range(3)]
    outside = np.setdiff1d(np.arange(n), lo + np.arange(ln))
    for df in (K_FREQUENT_DF - 1, K_FREQUENT_DF):  # half of the postings in the partition, half elsewhere
        docs = np.concatenate([lo + c.rng.choice(ln, size=df // 2, replace=False),
                               c.rng.choice(outside, size=df - df // 2, replace=False)])
        t[f"df{df}"] = c.add_term(docs, c.random_tf(df))
    for r in (256, 257, 1024, 1025):
        if r > ln:
            continue
        start = int(c.rng.integers(0, ln - r + 1))
        run = lo + start + np.arange(r)
        far = c.rng.choice(outside, size=1100, replace=False)
        t[f"run{r}"] = c.add_term(np.concatenate([run, far]), c.random_tf(r + 1100))
        if r < K_FREQUENT_DF:
            t[f"rare{r}"] = c.add_term(lo + c.rng.choice(ln, size=r, replace=False), c.random_tf(r))
    zdocs = np.concatenate([lo + c.rng.choice(ln, size=200, replace=False), c.rng.choice(outside, size=1500, replace=False)])
    t["zero"] = c.add_term(zdocs, c.random_tf(len(zdocs)), idf=0.0)
    t["one_slot"] = []
    for _ in range(20):
        m = int(c.rng.integers(30, 61))
        docs = np.concatenate([lo + c.rng.choice(ln, size=m // 2, replace=False), c.rng.choice(outside, size=m - m // 2, replace=False)])
        t["one_slot"].append(c.add_term(docs, c.random_tf(m)))
    c.scoring_terms, c.scoring_part = t, part
    return t


def scoring_queries(c: Corpus) -> dict:
    """name -> term ids (after `finish`: the unknown id n_vocab is only known then)."""
    t = c.scoring_terms
    w, one = t["whole"], t["one_slot"]
    runs = [t[key] for key in sorted(t) if key.startswith(("run", "rare"))]
    long_q = [(w + one + runs + [t["zero"], t["df1023"], t["df1024"]])[i % (23 + len(runs) + 3)] for i in range(134)]
    long_q[127] = long_q[128] = w[1]  # a duplicate pair across the term batches [0, 128) and [128, ...)
    return {
        "whole-twice": [w[0], w[0]],
        "whole-three": [w[0], w[1], w[2], w[1]],
        "whole-rare-alternating": [x for pair in zip(w + w, one[:6]) for x in pair],
        "table-threshold": [t["df1023"], t["df1024"], t["df1023"]],
        "slot-boundaries": runs + [w[2]] + runs[::-1],
        "zero-idf-and-unknown": [w[0], t["zero"], -1, one[0], c.n_vocab, t["zero"], w[0]],
        "seventeen-one-slot": one[:17],
        "over-a-term-batch": long_q,
    }


# ---------------------------------------------------------------------------------------------------- the test corpora
PART_DOCS = (256, 1024, 1280, 4096)
SHORT_LASTS = (1, 63, 64, 65, -1)  # -1: part_docs - 1


def aimed_forms(part_docs: int):
    return ("small",) if part_docs <= 1024 else ("wide", "tall")


def selection_corpus(n_cus: int, part_docs: int, seed: int = 11) -> Corpus:
    """Sections a, b and d of the grid on one corpus: the last partition is part_docs - 1 long; the selection cases go
    round the first, a middle and the last partition."""
    c = Corpus(n_cus, part_docs, part_docs - 1, seed + part_docs)
    targets = (0, n_cus // 2, n_cus - 1)
    j = 0
    for form in aimed_forms(part_docs):
        threads = FORMS[form][0]
        for k, n_surv in selection_grid(part_docs - 1, threads):
            for variant in ("equal", "distinct"):
                plant_selection(c, form, k, n_surv, targets[j % 3], variant)
                j += 1
        for variant in ("equal", "distinct"):
            plant_selection(c, form, 1, 1, targets[j % 3], variant)
            j += 1
    plant_filters(c, [(form, k, n) for form in aimed_forms(part_docs)
                      for k, n in filter_grid(part_docs - 1, FORMS[form][0])])
    plant_tail(c)
    return c.finish()


def short_last_corpus(n_cus: int, part_docs: int, last: int, seed: int = 23) -> Corpus:
    c = Corpus(n_cus, part_docs, part_docs - 1 if last < 0 else last, seed + part_docs + last)
    plant_short_last(c)
    return c.finish()


def scoring_corpus(n_cus: int, part_docs: int, seed: int = 37) -> Corpus:
    c = Corpus(n_cus, part_docs, part_docs - 1, seed + part_docs)
    plant_scoring(c, n_cus // 2)
    return c.finish()


def many_parts_corpus(n_cus: int, seed: int = 41) -> Corpus:
    """n_cus * 4096 + 1 documents: n_cus + 1 partitions, the last one document long, and that document a winner."""
    c = Corpus(n_cus + 1, K_MAX_PART_DOCS, 1, seed)
    others = c.rng.choice(c.n_docs - 1, size=300, replace=False)
    docs = np.concatenate([others, [c.n_docs - 1]])
    tf = np.concatenate([c.rng.integers(1, 30, 300), [45]])
    c.doc_len[c.n_docs - 1] = 20
    c.cases.append(dict(kind="tail", name="list-256-alone-in-the-second-chunk", k=64, parts=[c.n_parts - 1],
                        terms=[c.add_term(docs, tf)], allow=None))
    return c.finish()
