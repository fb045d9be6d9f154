"""GPU parity: K3's three kernel forms x the three paths of its selection, on planted corpora, against the oracle.

Forms (bm25.hip): <256,4> for partitions of at most 1,024 documents; above that <1024,4> ("wide") for a launch of one
query -- `bm25_search`, `bm25_scores` -- and <256,16> ("tall") for a group launch -- `bm25_search_group`.  Paths: at most
64 survivors of the bound tau are ranked by counting, up to surv_cap go through wave 0's network, more take the general
path.  Random corpora stay on the first path (and touch the second by luck), so every corpus here is planted
(tests/k3_select_model.py; tests/test_k3_select_model_cpu.py holds each case to the path it names).  Each corpus is
n_docs = (n_cus - 1) * part_docs + last documents for the device's own n_cus, and the geometry and the forms are read
back and asserted before anything else.

Oracle: oracle.ref_bm25.csr_get_scores, then ref_search.canonical_topk.  Bar: ids, counts, -1 padding and fp64 score
bits all equal, on the single-query route and on the group route."""
import numpy as np
import pytest

import k3_select_model as m

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def n_cus():
    from anrag.index import Index

    with Index(0) as idx:
        g = idx.bm25_geometry()
    assert g["n_cus"] >= 1
    assert {key: v for key, v in g.items() if key != "n_cus"} == dict(part_docs=0, n_parts=0, form_single=0, form_group=0)
    assert g["n_cus"] >= 64, "the filter cases take a partition each"
    return g["n_cus"]


def load(c, n_cus):
    """The corpus on the device; the geometry and the forms it is aimed at, asserted."""
    from anrag.index import Index

    idx = Index(0)
    a = c.arrays
    idx.bm25_load(a["indptr"], a["post_doc"], a["post_tf"], a["idf"], a["doc_len"], a["avgdl"], a["k1"], a["b"],
                  source_id=c.source_id)
    g = idx.bm25_geometry()
    forms = m.forms_of(c.part_docs)
    assert g == dict(n_cus=n_cus, part_docs=c.part_docs, n_parts=c.n_parts, form_single=m.FORM_ID[forms["single"]],
                     form_group=m.FORM_ID[forms["group"]]), g
    c.oracle_cache = {}
    return idx


def oracle(c, terms, k, allow):
    """-> (scores of every document, the k best rows): computed once per query and corpus, never modified."""
    from oracle import ref_bm25, ref_search

    key = tuple(terms)
    if key not in c.oracle_cache:
        a = c.arrays
        s = ref_bm25.csr_get_scores(a["indptr"], a["post_doc"], a["post_tf"], a["idf"], a["doc_len"], a["avgdl"], a["k1"],
                                    a["b"], c.known_terms(terms))
        s.setflags(write=False)
        c.oracle_cache[key] = s
    scores = c.oracle_cache[key]
    key = (key, k, allow)
    if key not in c.oracle_cache:
        c.oracle_cache[key] = ref_search.canonical_topk(scores, k, c.allowed_docs(allow))
    return scores, c.oracle_cache[key]


def assert_answer(doc, sc, cnt, scores, order, tag):
    assert cnt == len(order), (tag, cnt, len(order))
    assert doc[:cnt].tolist() == order.tolist(), tag
    assert np.array_equal(sc[:cnt].view(np.uint64), scores[order].view(np.uint64)), tag
    assert np.all(doc[cnt:] == -1), tag


def group_answers(idx, term_lists, k, allow):
    """`bm25_search_group`, with no launch of a single query in it (16 queries go per launch: a remainder of one would
    take the single-query form): a copy of the first query is added then, and has to come back as the first did."""
    n = len(term_lists)
    lists = list(term_lists) + ([term_lists[0]] if n % 16 == 1 else [])
    doc, sc, cnt = idx.bm25_search_group(lists, k, allow)
    assert doc.shape == sc.shape == (len(lists), k) and cnt.shape == (len(lists),)
    if len(lists) > n:
        assert cnt[n] == cnt[0] and np.array_equal(doc[n], doc[0])
        assert np.array_equal(sc[n, :cnt[n]].view(np.uint64), sc[0, :cnt[0]].view(np.uint64))
    return doc[:n], sc[:n], cnt[:n]


def check_both_routes(idx, c, queries):
    """queries: (terms, k, allowed sources or None, tag).  Each goes through `bm25_search` alone; those that share k and
    filter go through `bm25_search_group` together; both answers are held to the oracle (and so to each other)."""
    batches = {}
    for terms, k, allow, tag in queries:
        scores, order = oracle(c, terms, k, allow)
        doc, sc, cnt = idx.bm25_search(terms, k, c.allow_vector(allow))
        assert_answer(doc, sc, cnt, scores, order, ("single", tag))
        batches.setdefault((k, allow), []).append((terms, tag, scores, order))
    for (k, allow), batch in batches.items():
        doc, sc, cnt = group_answers(idx, [b[0] for b in batch], k, c.allow_vector(allow))
        for j, (_, tag, scores, order) in enumerate(batch):
            assert_answer(doc[j], sc[j], int(cnt[j]), scores, order, ("group", tag))


# ---------------------------------------------------------------------------------------------------- a, b, d
@pytest.fixture(scope="module", params=m.PART_DOCS)
def planted(request, n_cus):
    c = m.selection_corpus(n_cus, request.param)
    idx = load(c, n_cus)
    yield c, idx
    idx.close()


@pytest.mark.parametrize("k", [1, 10, 25, 64])
def test_selection_paths(planted, k):
    """P planted documents in groups 0 .. k-2 of the first, a middle or the last partition: P + k survivors, on both
    sides of 64 | 65 and of surv_cap | surv_cap + 1, once with equal planted scores (the row rule decides) and once with
    distinct ones; k = 1."""
    c, idx = planted
    cases = [x for x in c.cases if x["kind"] == "select" and x["k"] == k]
    assert cases or (k == 10 and c.part_docs == 256)  # (256-document partitions hold 64 / 65 survivors for k >= 25 only)
    check_both_routes(idx, c, [(x["terms"], k, None, x["name"]) for x in cases])


@pytest.mark.parametrize("k", [10, 25, 64])
def test_general_path_under_a_filter(planted, k):
    """The filter allows documents of fewer than k groups in the target partition: tau stays unset and every allowed
    document survives -- 64, 65, surv_cap and surv_cap + 1 of them."""
    c, idx = planted
    cases = [x for x in c.cases if x["kind"] == "filter" and x["k"] == k]
    assert cases or (k == 10 and c.part_docs == 256)  # (nine groups of a 256-document partition hold 36 documents)
    check_both_routes(idx, c, [(x["terms"], k, x["allow"], x["name"]) for x in cases])


def test_filters_that_leave_little(planted):
    """A filter that allows 7 documents in the whole corpus (count < k, the rest padding), and one that allows nothing in
    the partition that holds the query's best documents (every group of it empty)."""
    c, idx = planted
    cases = [x for x in c.cases if x["kind"] == "filter"]
    queries = []
    for x in (cases[0], cases[-1]):
        for k in (10, 64):
            queries.append((x["terms"], k, (m.SRC_FEW,), ("few", x["name"], k)))
            _, order = oracle(c, x["terms"], k, (m.SRC_FEW,))
            assert len(order) == 7 < k
            queries.append((x["terms"], k, (m.SRC_SPRINKLE,), ("nothing-in-target", x["name"], k)))
            queries.append((x["terms"], k, (), ("nothing-anywhere", x["name"], k)))
    check_both_routes(idx, c, queries)


def test_tail_merge(planted):
    """k = 64: every winner in one partition (its list feeds rounds 4 .. 63 of the merge), one winner in each of 64
    partitions, winners only in the last list of a wave's chunk of 64 lists."""
    c, idx = planted
    cases = [x for x in c.cases if x["kind"] == "tail"]
    assert len(cases) == (3 if c.n_parts > 63 else 2)
    check_both_routes(idx, c, [(x["terms"], k, None, (x["name"], k)) for x in cases for k in (64, 5)])


def test_group_of_seventeen(planted):
    """17 queries in one call: a launch of 16 in the grouped form (tall above 1,024 documents per partition), then a
    launch of 1 in the single-query form (wide); both answers are checked."""
    c, idx = planted
    cases = [x for x in c.cases if x["kind"] in ("select", "tail")]
    cases = (cases * 17)[:17]
    lists = [x["terms"] for x in cases]
    doc, sc, cnt = idx.bm25_search_group(lists, 25)
    for j, x in enumerate(cases):
        scores, order = oracle(c, x["terms"], 25, None)
        assert_answer(doc[j], sc[j], int(cnt[j]), scores, order, (j, x["name"]))


# ---------------------------------------------------------------------------------------------------- c
@pytest.mark.parametrize("last", m.SHORT_LASTS)
@pytest.mark.parametrize("part_docs", m.PART_DOCS)
def test_short_last_partition(n_cus, part_docs, last):
    """A last partition of 1, 63, 64, 65 and part_docs - 1 documents (groups left empty; fewer than k groups with a
    document), the winners inside it and straddling the last two."""
    c = m.short_last_corpus(n_cus, part_docs, last)
    idx = load(c, n_cus)
    try:
        check_both_routes(idx, c, [(x["terms"], k, None, (x["name"], k)) for x in c.cases for k in (10, 64)])
    finally:
        idx.close()


# ---------------------------------------------------------------------------------------------------- d: 257 partitions
def test_second_chunk_of_lists(n_cus):
    """n_cus * 4,096 + 1 documents: one partition more than CUs, and with more than 256 of them the tail's first wave
    takes a second chunk of lists, which holds one live list: a 1-document partition whose document is a winner."""
    c = m.many_parts_corpus(n_cus)
    idx = load(c, n_cus)
    try:
        if c.n_parts <= 256:
            pytest.skip("fewer than 257 partitions on this device")
        case, = c.cases
        _, order = oracle(c, case["terms"], 64, None)
        assert c.n_docs - 1 in order.tolist()
        check_both_routes(idx, c, [(case["terms"], k, None, k) for k in (64, 1)])
    finally:
        idx.close()


# ---------------------------------------------------------------------------------------------------- e
@pytest.fixture(scope="module", params=[1024, 4096])
def scoring(request, n_cus):
    c = m.scoring_corpus(n_cus, request.param)
    idx = load(c, n_cus)
    yield c, idx
    idx.close()


@pytest.mark.parametrize("name", ["whole-twice", "whole-three", "whole-rare-alternating", "table-threshold",
                                  "slot-boundaries", "zero-idf-and-unknown", "seventeen-one-slot", "over-a-term-batch"])
def test_scoring_rounds(scoring, name):
    """Terms on the edges of the gather rounds (a whole partition = 16 slots in the tall form and 4 in the wide one, the
    partition-table threshold, runs of 256 | 257 and 1,024 | 1,025 postings, idf 0, unknown ids, 17 one-slot terms, more
    than a term batch with a duplicate across its edge): every score of the single-query form, the top-k of both."""
    c, idx = scoring
    terms = m.scoring_queries(c)[name]
    scores, _ = oracle(c, terms, 25, None)
    got = idx.bm25_scores(terms)
    assert np.array_equal(got.view(np.uint64), scores.view(np.uint64)), name
    check_both_routes(idx, c, [(terms, k, None, (name, k)) for k in (25, 64)])
