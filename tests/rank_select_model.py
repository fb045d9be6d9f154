"""Numpy model of the ranking select's order, and the planted inputs the wide form is tested on.

The order (rank_batch.hip): score descending with -0.0 == +0.0, then the tie word ascending (the row, unless tie words
are given); -inf is "not a candidate"; count = min(k, candidates), k cut to the list cap.  `select_model` restates it as a
stable lexsort.  The generators say what they plant in `claims`; tests/test_rank_select_model_cpu.py checks each claim
against the model, so the GPU test cannot pass on a degenerate input.
"""
import numpy as np

CAP32, CAP64 = 16384, 13312  # anrag_rank_caps
MIN_SLICE = 4096             # the wide form's shortest slice (include/anrag.h, anrag_debug_rank_select)


def cap_of(dtype) -> int:
    return CAP64 if np.dtype(dtype) == np.float64 else CAP32


def stride_of(n: int) -> int:
    return (n + 63) // 64 * 64


def slice_len(n: int, parts: int) -> int:
    """Scores per slice when P = parts is asked for: a multiple of 64, never below MIN_SLICE."""
    per = -(-n // parts)
    return max(MIN_SLICE, (per + 63) // 64 * 64)


def n_slices(n: int, parts: int) -> int:
    return -(-n // slice_len(n, parts))


def select_model(keys, n, k, ties=None, seg_k=None):
    """-> per segment (rows uint32, scores float64); rows are tie words where `ties` is given."""
    keys = np.asarray(keys)
    cap = cap_of(keys.dtype)
    out = []
    for s in range(keys.shape[0]):
        ks = min(k, cap)
        if seg_k is not None:
            ks = min(ks, int(seg_k[s]))
        v = keys[s, :n].astype(np.float64) + 0.0  # -0.0 + 0.0 = +0.0: signed zeros merged
        t = np.arange(n, dtype=np.uint32) if ties is None else np.asarray(ties[s, :n], dtype=np.uint32)
        cand = np.flatnonzero(v != -np.inf)
        order = cand[np.lexsort((t[cand], -v[cand]))]
        order = order[:max(ks, 0)]
        out.append((t[order].astype(np.uint32), keys[s, :n][order].astype(np.float64)))
    return out


def _pad(rows, n, dtype):
    """[n_seg][n] -> [n_seg, stride]; the padding holds finite garbage that must never be read as a score."""
    a = np.full((len(rows), stride_of(n)), 7.0e30, dtype=dtype)
    for s, r in enumerate(rows):
        a[s, :n] = r
    return a


def gen_normal(rng, n_seg, n, dtype, k):
    keys = _pad([rng.standard_normal(n).astype(dtype) for _ in range(n_seg)], n, dtype)
    return dict(keys=keys, ties=None, signed_zeros=False, claims=dict(kind="normal", min_distinct=n // 2))


def gen_all_equal(rng, n_seg, n, dtype, k):
    keys = _pad([np.full(n, 0.25, dtype) for _ in range(n_seg)], n, dtype)
    return dict(keys=keys, ties=None, signed_zeros=False, claims=dict(kind="all_equal"))


def gen_two_values(rng, n_seg, n, dtype, k):
    """30 % of the rows score 1.0, the rest 0.5: the k-th best lies inside the larger group whenever k exceeds the
    smaller one (claims['boundary_in_larger'] says whether it does)."""
    rows = []
    hi = int(n * 0.3)
    for _ in range(n_seg):
        r = np.full(n, 0.5, dtype)
        r[rng.permutation(n)[:hi]] = 1.0
        rows.append(r)
    kk = min(k, cap_of(dtype))
    return dict(keys=_pad(rows, n, dtype), ties=None, signed_zeros=False,
                claims=dict(kind="two_values", n_hi=hi, boundary_in_larger=hi < kk))


def gen_bm25_like(rng, n_seg, n, dtype, k):
    """Fewer than k positive scores over a sea of +0.0 (a BM25 leg: most documents share no term with the query)."""
    kk = min(k, cap_of(dtype))
    pos = min(max(kk - 1, 0), 300)
    rows = []
    for _ in range(n_seg):
        r = np.zeros(n, dtype)
        r[rng.permutation(n)[:pos]] = (rng.random(pos) * 20 + 0.1).astype(dtype)
        rows.append(r)
    return dict(keys=_pad(rows, n, dtype), ties=None, signed_zeros=False, claims=dict(kind="bm25_like", positives=pos))


def gen_neg_inf(rng, n_seg, n, dtype, k):
    rows = []
    for _ in range(n_seg):
        r = rng.standard_normal(n).astype(dtype)
        r[rng.random(n) < 0.4] = -np.inf
        rows.append(r)
    return dict(keys=_pad(rows, n, dtype), ties=None, signed_zeros=False, claims=dict(kind="neg_inf"))


def gen_all_neg_inf(rng, n_seg, n, dtype, k):
    keys = _pad([np.full(n, -np.inf, dtype) for _ in range(n_seg)], n, dtype)
    return dict(keys=keys, ties=None, signed_zeros=False, claims=dict(kind="all_neg_inf"))


def gen_signed_zeros(rng, n_seg, n, dtype, k):
    rows = []
    for _ in range(n_seg):
        r = np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(dtype)
        some = rng.permutation(n)[:n // 8]
        r[some] = rng.standard_normal(some.size).astype(dtype)
        rows.append(r)
    return dict(keys=_pad(rows, n, dtype), ties=None, signed_zeros=True, claims=dict(kind="signed_zeros"))


def gen_inf_denormals(rng, n_seg, n, dtype, k):
    tiny = np.finfo(dtype).smallest_subnormal
    rows = []
    for _ in range(n_seg):
        r = rng.standard_normal(n).astype(dtype)
        p = rng.permutation(n)
        r[p[:5]] = np.inf
        m = n // 4
        r[p[5:5 + m]] = (tiny * rng.integers(1, 1000, m)).astype(dtype)
        r[p[5 + m:5 + 2 * m]] = (-tiny * rng.integers(1, 1000, m)).astype(dtype)
        rows.append(r)
    return dict(keys=_pad(rows, n, dtype), ties=None, signed_zeros=False, claims=dict(kind="inf_denormals", n_inf=5))


def gen_planted_boundary(rng, n_seg, n, dtype, k, parts):
    """Two equal keys on either side of the first slice boundary, at ranks k and k + 1 (1-based): k - 1 rows score
    above them, everything else below; the row before the boundary takes rank k."""
    b = slice_len(n, parts)
    if not (b < n and 1 <= k <= min(cap_of(dtype) - 1, n - 2)):
        raise ValueError("no room for the planted pair")
    rows = []
    for _ in range(n_seg):
        r = rng.random(n).astype(dtype)  # [0, 1)
        free = np.setdiff1d(np.arange(n), [b - 1, b])
        top = rng.permutation(free)[:k - 1]
        r[top] = (3.0 + rng.random(k - 1)).astype(dtype)
        r[b - 1] = r[b] = 2.0
        rows.append(r)
    return dict(keys=_pad(rows, n, dtype), ties=None, signed_zeros=False,
                claims=dict(kind="planted_boundary", boundary=b, k=k))


def gen_tie_form(rng, n_seg, n, dtype, k):
    """The fused-sums form: fp64 keys from a handful of equal and adjacent values, a random permutation as tie words,
    a quarter of the entries unnamed (-inf)."""
    assert np.dtype(dtype) == np.float64
    vals = np.array([1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 0.5, 1.0 / 61 + 1.0 / 62, 1.0 / 62 + 1.0 / 61])
    rows, ties = [], []
    for _ in range(n_seg):
        r = vals[rng.integers(0, vals.size, n)]
        r[rng.random(n) < 0.25] = -np.inf
        rows.append(r)
        ties.append(rng.permutation(n).astype(np.uint32))
    t = np.zeros((n_seg, stride_of(n)), np.uint32)
    for s in range(n_seg):
        t[s, :n] = ties[s]
    return dict(keys=_pad(rows, n, dtype), ties=t, signed_zeros=False, claims=dict(kind="tie_form"))


GENERATORS = dict(normal=gen_normal, all_equal=gen_all_equal, two_values=gen_two_values, bm25_like=gen_bm25_like,
                  neg_inf=gen_neg_inf, all_neg_inf=gen_all_neg_inf, signed_zeros=gen_signed_zeros,
                  inf_denormals=gen_inf_denormals)


def check_claims(case, n, k):
    """Assert that the input holds what its generator claims (raises AssertionError)."""
    keys, ties, c = case["keys"], case["ties"], case["claims"]
    cap = cap_of(keys.dtype)
    kk = min(k, cap)
    assert keys.shape[1] == stride_of(n) and keys.shape[1] % 64 == 0
    model = select_model(keys, n, k, ties)
    for s in range(keys.shape[0]):
        v = keys[s, :n]
        rows, sc = model[s]
        cand = int((v != -np.inf).sum())
        assert len(rows) == min(kk, cand)
        assert len(np.unique(rows)) == len(rows)
        assert np.all(sc[1:] <= sc[:-1])
        kind = c["kind"]
        if kind == "normal":
            assert np.unique(v).size >= c["min_distinct"] and cand == n
        elif kind == "all_equal":
            assert np.unique(v).size == 1 and n > cap  # equal keys outnumber the cap: rows decide everything
            assert np.array_equal(rows, np.arange(len(rows)))
        elif kind == "two_values":
            assert np.unique(v).size == 2 and (v == 1.0).sum() == c["n_hi"] and (v == 0.5).sum() > c["n_hi"]
            if c["boundary_in_larger"] and kk < n:
                assert sc[kk - 1] == 0.5 and (v == 0.5).sum() > kk - c["n_hi"]  # cut inside the larger group
        elif kind == "bm25_like":
            assert (v > 0).sum() == c["positives"] < max(kk, 1) and (v == 0).sum() > cap
            assert not np.signbit(v).any()
            if kk > c["positives"]:
                assert sc[c["positives"]] == 0.0  # the cut falls among the zeros
        elif kind == "neg_inf":
            assert 0 < cand < n and n - cand > n // 4
        elif kind == "all_neg_inf":
            assert cand == 0 and len(rows) == 0
        elif kind == "signed_zeros":
            z = v == 0
            assert (z & np.signbit(v)).sum() > n // 8 and (z & ~np.signbit(v)).sum() > n // 8
        elif kind == "inf_denormals":
            assert np.isposinf(v).sum() == c["n_inf"] and np.all(np.isposinf(sc[:min(c["n_inf"], len(sc))]))
            tiny = np.finfo(v.dtype).tiny
            assert ((v != 0) & (np.abs(v) < tiny)).sum() > n // 4
        elif kind == "planted_boundary":
            b = c["boundary"]
            assert b % 64 == 0 and b >= MIN_SLICE and b < n
            full = select_model(keys[s:s + 1], n, c["k"] + 1)[0]
            assert full[0][c["k"] - 1] == b - 1 and full[0][c["k"]] == b  # ranks k and k + 1 straddle the boundary
            assert full[1][c["k"] - 1] == full[1][c["k"]] == 2.0
        elif kind == "tie_form":
            t = ties[s, :n]
            assert np.array_equal(np.sort(t), np.arange(n))  # a permutation: unique tie words
            assert np.unique(v[v != -np.inf]).size <= 6 and cand > cap // 2
            pos = np.argsort(t)[rows]  # where the winners sit: among equal keys NOT in position order
            assert len(rows) < 8 or not np.array_equal(pos, np.sort(pos))  # the tie words, not the positions, decide
        else:
            raise AssertionError(kind)
