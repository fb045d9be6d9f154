"""CPU: the numpy model of K3's selection (tests/k3_select_model.py) agrees with the oracle's order, follows the
kernel's geometry as written in bm25.hip, and every planted case of tests/test_gpu_bm25_forms.py lands on the selection
path it is meant for -- a case that misses its path fails here, so the GPU test cannot pass on a degenerate input."""
import os
import re

import numpy as np
import pytest

import k3_select_model as m
from oracle import ref_bm25, ref_search

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CUS = 64  # enough partitions for one per filter case; the GPU test reads the device's own number


def oracle_scores(c, terms):
    a = c.arrays
    return ref_bm25.csr_get_scores(a["indptr"], a["post_doc"], a["post_tf"], a["idf"], a["doc_len"], a["avgdl"], a["k1"],
                                   a["b"], c.known_terms(terms))


def test_constants_follow_the_kernel_source():
    src = open(os.path.join(REPO, "a-nice-rag_amd", "csrc", "bm25.hip")).read()

    def const(name):
        return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))

    threads, small, per_thread = const("kBm25Threads"), const("kBm25ThreadsSmall"), const("kPostPerThread")
    assert m.FORMS == {"small": (small, per_thread), "wide": (threads, per_thread), "tall": (small, threads * per_thread // small)}
    assert re.search(r"constexpr int kMaxPartDocs = kPostPerThread \* kBm25Threads;", src)
    assert re.search(r"constexpr int kDocsPerThreadTall = kMaxPartDocs / kBm25ThreadsSmall;", src)
    assert m.K_MAX_PART_DOCS == per_thread * threads
    assert m.K_FREQUENT_DF == const("kFrequentDf") and m.K_TERM_BATCH == const("kTermBatch")
    assert m.K_ROUND_TERMS == const("kRoundTerms")
    rs = re.search(r"constexpr int round_slots\(int threads, int dpt\) \{ return threads == kBm25ThreadsSmall && "
                   r"dpt == kDocsPerThreadTall \? (\d+) : (\d+); \}", src)
    sc = re.search(r"constexpr int surv_cap\(int threads\) \{ return threads == kBm25Threads \? (\d+) : (\d+); \}", src)
    ro = re.search(r"constexpr int ROT = LPG == 16 \? (\d+) : (\d+);", src)
    for name, (t, d) in m.FORMS.items():
        assert m.round_slots(t, d) == int(rs.group(1 if name == "tall" else 2)), name
        assert m.surv_cap(t) == int(sc.group(1 if t == threads else 2)), name
        assert m.rot(t) == int(ro.group(1 if t // 64 == 16 else 2)), name
    assert re.search(r"const int i = 64 \* j \+ \(\(g \+ ROT \* j\) & 63\);", src), "the dealing of documents to groups"
    assert re.search(r"pd = \(\(pd \+ 255\) / 256\) \* 256;\s*pd = std::max<int64_t>\(256, std::min<int64_t>\(kMaxPartDocs, pd\)\);", src)


@pytest.mark.parametrize("n_cus", [16, 64, 256, 304])
def test_partitioning_of_the_test_geometry(n_cus):
    for pd in m.PART_DOCS:
        for last in (1, 63, 64, 65, pd - 1, pd):
            assert m.partitioning((n_cus - 1) * pd + last, n_cus) == (pd, n_cus), (pd, last)
        assert m.forms_of(pd) == (dict(single="small", group="small") if pd <= 1024 else dict(single="wide", group="tall"))
    assert m.partitioning(n_cus * 4096 + 1, n_cus) == (4096, n_cus + 1)
    assert m.partitioning(600_123, 256) == (2560, 235) and m.partitioning(30000, 256) == (256, 118)


@pytest.mark.parametrize("threads", [256, 1024])
def test_group_dealing(threads):
    i = np.arange(m.K_MAX_PART_DOCS if threads == 1024 else 4096)
    g = m.group_of(i, threads)
    rot = m.rot(threads)
    for grp in (0, 1, 37, 63):  # group g holds rows g, 64 + (g + ROT) % 64, 128 + (g + 2 ROT) % 64, ...
        rows = [64 * j + (grp + rot * j) % 64 for j in range(len(i) // 64)]
        assert np.flatnonzero(g == grp).tolist() == rows
    assert g[:64].tolist() == list(range(64))  # the groups' lowest rows are rows 0 .. 63
    assert (np.bincount(g, minlength=64) == len(i) // 64).all()


def _random_slices(rng, n):
    cont = rng.random(n)
    sparse = np.where(rng.random(n) < 0.02, rng.random(n), 0.0)
    two = rng.choice([0.0, 1.5], size=n, p=[0.7, 0.3])
    three = rng.choice([0.0, 1.5, 2.5], size=n)
    return dict(continuous=cont, sparse=sparse, two_valued=two, three_valued=three, zeros=np.zeros(n))


@pytest.mark.parametrize("threads,pd", [(256, 256), (256, 1024), (1024, 1280), (1024, 4096), (256, 4096)])
def test_model_equals_canonical_topk_on_random_slices(threads, pd):
    rng = np.random.default_rng(pd + threads)
    n = 5 * pd + 77
    peak = 0
    for name, s in _random_slices(rng, n).items():
        for k in (1, 2, 10, 25, 63, 64):
            for allowed in (None, rng.random(n) < 0.3):
                rows, parts = m.topk_model(s, k, pd, threads, allowed)
                assert rows.tolist() == ref_search.canonical_topk(s, k, allowed).tolist(), (name, k)
                peak = max(peak, max(p["n_surv"] for p in parts))
                for p in parts:  # the bound never cuts a winner, and the survivors are what the path is chosen by
                    assert len(p["rows"]) == min(k, p["n_surv"])
    assert peak <= m.surv_cap(threads), "random data reached the general path: the premise of the planted cases changed"


def test_grids_hold_the_cases_the_issue_lists():
    want = {(256, "small"): [(25, 64), (25, 65), (64, 65)],
            (1024, "small"): [(10, 64), (10, 65), (25, 64), (25, 65), (64, 512), (64, 513)],
            (1280, "tall"): [(10, 64), (10, 65), (25, 64), (25, 65), (64, 512), (64, 513)],
            (1280, "wide"): [(64, 1024), (64, 1025)],
            (4096, "wide"): [(25, 1024), (25, 1025), (64, 1024), (64, 1025)],
            (4096, "tall"): [(10, 512), (10, 513), (25, 512), (25, 513), (64, 512), (64, 513)]}
    for (pd, form), cases in want.items():
        grid = m.selection_grid(pd - 1, m.FORMS[form][0])
        assert set(cases) <= set(grid), (pd, form, sorted(set(cases) - set(grid)))
        assert form in m.aimed_forms(pd)


@pytest.fixture(scope="module", params=m.PART_DOCS)
def planted(request):
    return m.selection_corpus(N_CUS, request.param)


def _slice(c, part):
    lo = part * c.part_docs
    return lo, lo + c.part_len(part)


def test_selection_and_filter_cases_land_on_their_paths(planted):
    c = planted
    assert m.partitioning(c.n_docs, N_CUS) == (c.part_docs, N_CUS)
    paths = set()
    for case in [x for x in c.cases if x["kind"] in ("select", "filter")]:
        threads = m.FORMS[case["form"]][0]
        scores = oracle_scores(c, case["terms"])
        allowed = c.allowed_docs(case["allow"])
        lo, hi = _slice(c, case["part"])
        got = m.select_model(scores[lo:hi], case["k"], threads, None if allowed is None else allowed[lo:hi], lo)
        assert got["n_surv"] == case["n_surv"] and got["path"] == case["path"], (case["name"], got["n_surv"], got["path"])
        paths.add((case["form"], case["path"]))
        if case["kind"] == "select" and case["k"] > 1:
            assert got["tau"] == (0.0, lo + case["k"] - 1), case["name"]
            planted_scores = scores[lo:hi][scores[lo:hi] > 0]
            assert len(planted_scores) == case["n_surv"] - case["k"]
            assert len(np.unique(planted_scores)) == (1 if case["variant"] == "equal" else len(planted_scores)), case["name"]
        if case["kind"] == "filter":
            assert got["tau"] is None and allowed[lo:hi].sum() == case["n_surv"], case["name"]
            assert (scores[lo:hi][allowed[lo:hi]] > 0).sum() >= case["n_surv"] // 2
        rows, _ = m.topk_model(scores, case["k"], c.part_docs, threads, allowed)
        assert rows.tolist() == ref_search.canonical_topk(scores, case["k"], allowed).tolist(), case["name"]
    # every path each form can hold at this partition size is aimed at, from both sides of its boundaries
    for form in m.aimed_forms(c.part_docs):
        want = {"count", "network"} if c.part_docs == 256 else {"count", "network", "general"}
        assert {p for f, p in paths if f == form} == want, (form, paths)
    by_count = {(x["form"], x["n_surv"]) for x in c.cases if x["kind"] in ("select", "filter")}
    for form in m.aimed_forms(c.part_docs):
        cap = m.surv_cap(m.FORMS[form][0])
        assert {(form, 64), (form, 65)} <= by_count
        if c.part_docs > 256:
            assert {(form, cap), (form, cap + 1)} <= by_count


def test_filter_extras(planted):
    c = planted
    assert len(c.few_docs) == 7 and (c.source_id[c.few_docs] == m.SRC_FEW).all()
    assert (c.source_id == m.SRC_FEW).sum() == 7  # fewer than k = 10 documents in the whole corpus
    for case in [x for x in c.cases if x["kind"] == "filter"]:
        lo, hi = _slice(c, case["part"])
        assert not (c.source_id[lo:hi] == m.SRC_SPRINKLE).any()  # "nothing allowed in the target partition"
        scores = oracle_scores(c, case["terms"])
        assert (scores[c.few_docs] > 0).sum() == 4


def test_tail_cases(planted):
    c = planted
    for case in [x for x in c.cases if x["kind"] == "tail"]:
        scores = oracle_scores(c, case["terms"])
        top = ref_search.canonical_topk(scores, case["k"])
        for form in m.aimed_forms(c.part_docs):
            rows, _ = m.topk_model(scores, case["k"], c.part_docs, m.FORMS[form][0])
            assert rows.tolist() == top.tolist()
        win_parts = top[scores[top] > 0] // c.part_docs
        assert set(win_parts.tolist()) <= set(case["parts"])
        if case["name"] == "one-partition":
            assert len(win_parts) == 64  # one list feeds every round of the merge
        if case["name"] == "one-per-partition":
            assert len(set(win_parts.tolist())) == len(win_parts) == min(64, c.n_parts)
    assert {"one-partition", "one-per-partition"} <= {x["name"] for x in c.cases if x["kind"] == "tail"}
    c = m.selection_corpus(256, 256)
    assert [x["parts"] for x in c.cases if x["name"] == "last-list-of-a-chunk"] == [[63, 127, 191, 255]]


@pytest.mark.parametrize("pd", m.PART_DOCS)
@pytest.mark.parametrize("last", m.SHORT_LASTS)
def test_short_last_partitions(pd, last):
    c = m.short_last_corpus(16, pd, last)
    want_last = pd - 1 if last < 0 else last
    assert c.part_len(c.n_parts - 1) == want_last and m.partitioning(c.n_docs, 16) == (pd, 16)
    for case in c.cases:
        scores = oracle_scores(c, case["terms"])
        for k in (10, 64):
            top = ref_search.canonical_topk(scores, k)
            assert int(top[0]) // pd in case["parts"]  # the best document is a planted one
            if case["name"] == "straddle-last-two" and k == 64:
                assert set((top[scores[top] > 0] // pd).tolist()) == {c.n_parts - 2, c.n_parts - 1}
            for form in m.aimed_forms(pd):
                rows, parts = m.topk_model(scores, k, pd, m.FORMS[form][0])
                assert rows.tolist() == top.tolist()
                if want_last < k:  # fewer than k groups hold a document: no bound
                    assert parts[-1]["tau"] is None and parts[-1]["n_surv"] == want_last


@pytest.mark.parametrize("pd", [1024, 4096])
def test_scoring_terms_and_queries(pd):
    c = m.scoring_corpus(16, pd)
    t, q = c.scoring_terms, m.scoring_queries(c)
    a = c.arrays
    lo, hi = _slice(c, c.scoring_part)

    def run(term):  # the term's postings inside the partition
        d = a["post_doc"][a["indptr"][term]:a["indptr"][term + 1]]
        return int(((d >= lo) & (d < hi)).sum())

    for w in t["whole"]:
        assert run(w) == hi - lo == pd  # a whole partition: pd / 256 slots in the 256-thread forms, pd / 1,024 in the wide one
    assert c.df[t["df1023"]] == m.K_FREQUENT_DF - 1 and c.df[t["df1024"]] == m.K_FREQUENT_DF
    for r in (256, 257, 1024, 1025):
        if r <= pd:
            assert run(t[f"run{r}"]) == r and c.df[t[f"run{r}"]] >= m.K_FREQUENT_DF
            if r < m.K_FREQUENT_DF:
                assert c.df[t[f"rare{r}"]] == r == run(t[f"rare{r}"])
        else:
            assert f"run{r}" not in t
    assert a["idf"][t["zero"]] == 0.0 and (a["idf"][np.arange(c.n_vocab) != t["zero"]] > 0).all()
    assert all(c.df[x] <= 256 for x in t["one_slot"])
    assert len(q["seventeen-one-slot"]) == 17 > m.K_ROUND_TERMS and len(set(q["seventeen-one-slot"])) == 17
    long_q = q["over-a-term-batch"]
    assert len(long_q) >= 130 and long_q[m.K_TERM_BATCH - 1] == long_q[m.K_TERM_BATCH] == t["whole"][1]
    assert q["whole-twice"][0] == q["whole-twice"][1] == t["whole"][0]
    assert -1 in q["zero-idf-and-unknown"] and c.n_vocab in q["zero-idf-and-unknown"]
    # tf and doc_len vary: the partition's scores under the three whole-partition terms are (all but) all distinct
    s = oracle_scores(c, q["whole-three"])[lo:hi]
    assert len(np.unique(s)) > 0.95 * pd and len(np.unique(a["doc_len"][lo:hi])) > 50
    for name, terms in q.items():  # every query's order survives the model in both forms
        scores = oracle_scores(c, terms)
        for form in m.aimed_forms(pd):
            rows, _ = m.topk_model(scores, 25, pd, m.FORMS[form][0])
            assert rows.tolist() == ref_search.canonical_topk(scores, 25).tolist(), name


def test_many_partitions_corpus():
    c = m.many_parts_corpus(256)
    assert m.partitioning(c.n_docs, 256) == (4096, 257) and c.n_docs == 256 * 4096 + 1
    case, = c.cases
    scores = oracle_scores(c, case["terms"])
    top = ref_search.canonical_topk(scores, 64)
    assert c.n_docs - 1 in top.tolist() and scores[c.n_docs - 1] > 0  # the document of list 256 is a winner
