"""GPU: the dense prefilter's score intervals, row by row (dense_prefilter.hip; DESIGN.md §3 "K1F", "K1F8").

Every mode of the dense top-k returns the fp32 scan's ids and score bits because, for every allowed row,
lo <= s <= hi, and T (the k-th largest lo) <= K1's k-th score.  The end-to-end tests only notice a wrong interval when
a row of the true top k is dropped; these look at the intervals themselves (anrag_debug_prefilter_read / _bounds)
against the fp64 model of tests/prefilter_model.py, on rows built to sit at the ends of the interval:
  a. the load-time kernels: image and per-row radii against the reference;
  b. containment of K1's score in [-hi(-q), hi(q)] for every row, and T against K1's k-th score;
  c. the saturating rows really press on the device's interval (so that a radius too small shows in b);
  d. the interval is not looser than the documented outward roundings allow.
Every figure asserted on is printed first."""
import numpy as np
import pytest

import prefilter_model as pm

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x7FA5A5A5)
N_ROWS = 20_011  # odd: every wave's last batch is partial, and loads past the end are clamped


@pytest.fixture(scope="module")
def Index():
    from anrag.index import Index

    return Index


def _gauss(n, d, rng):
    e = rng.standard_normal((n, d), dtype=np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    return e


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


class Stored:
    """the model evaluated on the image and per-row data the device built"""

    def __init__(self, mode, dbg):
        self.mode, self.meta = mode, dbg["meta"].astype(np.float64)
        self.img = dbg["image"].astype(np.float64)
        self.img_norm = np.sqrt(np.sum(self.img * self.img, axis=1))
        # per row: the fp16 form's per-row data is one radius ([n]), the int8 form's {s_e, m1, m2, 0} ([n, 4])
        self.finite_row = np.isfinite(self.meta.reshape(len(self.meta), -1)).all(axis=1) & np.isfinite(self.img_norm)
        self.abs_img = np.abs(self.img) if mode == 1 else None
        self.cache = {}

    def interval(self, q):
        """(a, r, R) per row, R the widest radius a correct device may show around the model's fp64 a:
        `prefilter_model.outward` (the outward roundings of r and of a +- r, derived there from the kernel's comments)
        and, for the fp16 form only, `prefilter_model.k1f_a_slack`: the int8 a is an exact integer times two scales,
        but the fp16 a is an fp32 sum of D products, and the model's a is the fp64 one.  That slack is the rounding
        bound of the scan's own reduction (a chain of D / G FMAs per lane and a log2 G tree), gamma_(D/G + log2 G)
        sum |q_i e~_i|: 13 .. 38 roundings, not the D of DESIGN.md's worst case, and measured on |q|.|e~|, not on
        ||q|| ||e~||.  It still leaves part d weaker for fp16 than for int8: on a row whose terms cancel (|a| far
        below sum |q_i e~_i|) hi may exceed a + r by up to that slack unnoticed -- at most 38 u sum |q_i e~_i|,
        i.e. below 38 / (2 D) of r's own gamma term, 1 % of r at D = 2048."""
        key = q.tobytes()
        if key in self.cache:
            return self.cache[key]
        with np.errstate(invalid="ignore", over="ignore"):
            if self.mode == 1:
                a, r = pm.k1f_interval(self.img, self.meta, q)
                R = pm.outward(a, r) + pm.k1f_a_slack(self.abs_img, q)
            else:
                a, r, _ = pm.k1f8_interval(self.img, self.meta, q)
                R = pm.outward(a, r)
        self.cache[key] = (a, r, R)
        return a, r, R


# ---------------------------------------------------------------- a. load-time kernels
def _special_rows(e, rng):
    """rows 2 .. 12 of a corpus of >= 63 rows: the ranges that take a branch of their own in the convert kernels"""
    d = e.shape[1]
    e[2, 5] = np.nan
    e[3, 0] = np.inf
    e[4, d - 1] = -np.inf
    e[5] = e[5] * 2.0 ** 62          # norm past the 2^60 cap
    e[6] = e[6] * 1e6                # past fp16's 65504 (finite for int8)
    e[7] = 0.0                       # all zero: scale 1
    e[8] = e[8] * 1e-40              # subnormal components: int8 scale subnormal -> 1 only if it vanishes
    e[9] = 0.0
    e[9, 3] = 1e-45                  # the smallest subnormal: max / 127 vanishes, scale 1
    e[10] = e[10] * 1e-6             # fp16 subnormal range
    e[11] = e[11] * 2.0 ** 20
    e[12] = e[12] * 2.0 ** -20
    return {"inf_radius": [2, 3, 4, 5], "fp16_overflow": [6], "zero": [7], "scale_one": [7, 9]}


def _check_load(mode, e, dbg):
    n, d = e.shape
    img, meta = dbg["image"], dbg["meta"]
    e64 = e.astype(np.float64)
    if mode == 1:
        ref = pm.k1f_image(e)
        ok = np.isfinite(e) & (np.abs(e) <= 65504.0)
        assert np.array_equal(img.view(np.uint16)[ok], ref.view(np.uint16)[ok]), "fp16 image != round-to-nearest-even"
        need = pm.k1f_required_m(e, img)
        stored = meta.astype(np.float64)
    else:
        s_e = meta[:, 0].astype(np.float64)
        assert np.all(np.isfinite(s_e) & (s_e > 0)), "int8 scale not positive finite"
        assert img.min() >= -127 and img.max() <= 127
        assert np.all(meta[:, 3] == 0)
        with np.errstate(invalid="ignore"):
            mx = np.max(np.abs(e), axis=1)
        normal = np.isfinite(e).all(axis=1) & (mx >= np.finfo(np.float32).tiny)
        err = np.abs(e64[normal] - s_e[normal, None] * img[normal].astype(np.float64))
        assert np.all(err <= s_e[normal, None] * (0.5 + 2.0 ** -14)), "an int8 code is not a nearest one"
        need, need2 = pm.k1f8_required(e, img, s_e)
        stored, stored2 = meta[:, 1].astype(np.float64), meta[:, 2].astype(np.float64)
        fin2 = np.isfinite(need2)
        assert np.all(stored2[fin2] >= need2[fin2]), "m2 below ||e~||"
        assert np.all(stored2[fin2] <= need2[fin2] * pm.LOAD_WIDENING + 2.0 ** -149), "m2 looser than specified"
    fin = np.isfinite(need)
    assert np.all(np.isposinf(stored[~fin])), "a non-finite / capped row must have an infinite radius"
    short = stored[fin] < need[fin]
    assert not short.any(), f"radius below the required value on rows {np.flatnonzero(fin)[short][:8]}"
    # rounded up to fp32: at most 2^-23 relative, or one subnormal step (2^-149) absolute
    assert np.all(stored[fin] <= need[fin] * pm.LOAD_WIDENING + 2.0 ** -149), "radius looser than specified"
    return stored


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("dim", pm.SERVED_DIMS)
def test_load_time_kernels_against_reference(Index, mode, dim):
    rng = np.random.default_rng(1000 * mode + dim)
    with Index(0) as idx:
        idx.set_dense_prefilter(mode)
        idx.dense_load(_gauss(300, dim, rng))
        rw = idx.debug_prefilter_read(data=False)["batch_rows"]
        assert rw >= 1
        counts = [1, 63, 64, 65, 4 * rw - 1, 4 * rw + 1, 4 * 64 * 3 - 1, 4 * 64 * 3 + 1, N_ROWS]
        for n in counts:
            e = _gauss(n, dim, rng)
            e[rng.integers(0, n, max(1, n // 10))] *= np.float32(37.5)
            kinds = _special_rows(e, rng) if n >= 63 else {}
            idx.dense_load(e)
            dbg = idx.debug_prefilter_read()
            assert dbg["form"] == mode and dbg["image"].shape == (n, dim)
            stored = _check_load(mode, e, dbg)
            if kinds:
                assert np.all(np.isposinf(stored[kinds["inf_radius"]]))
                assert np.all(np.isfinite(stored[[7, 8, 9, 10, 12]]))
                assert np.isfinite(stored[11]) == (mode == 2)  # 2^20 x a unit row: past fp16's range
                assert stored[7] == 0.0
                if mode == 1:
                    assert np.isposinf(stored[6])
                else:
                    assert np.isfinite(stored[6])
                    assert np.all(dbg["meta"][kinds["scale_one"], 0] == 1.0)
                    assert not dbg["image"][kinds["zero"]].any()


# ---------------------------------------------------------------- b, c, d: the intervals
def _plant(mode, dim, n, rpw, rng, variant=0):
    """A corpus with rows that press on both ends of the interval at three scales, each at the first and the last row
    of a wave's block, one at row 0 and one at row n - 1.  -> e, queries {name: q}, pressed {query name: rows}"""
    e = _gauss(n, dim, rng)
    pressed = {"row": [], "-row": [], "query": [], "-query": []}
    blocks = iter(range(1, n // rpw - 1))

    cands = []

    def put(row_vec, key):
        cands.append((key, row_vec))
        w = next(blocks)
        for at in (w * rpw, (w + 1) * rpw - 1):
            e[at] = row_vec
            pressed[key].append(at)

    if mode == 2:
        q_row, _ = pm.sat_i8_row(dim, np.random.default_rng(dim), norm=1.0)
        sign = np.sign(q_row)
        q_qt, e_qt = pm.sat_i8_query(dim, np.random.default_rng(dim + 1), norm=1.0)
        for norm in (2.0 ** -20, 1.0, 2.0 ** 20):
            for side, key in ((1, "row"), (-1, "-row")):
                put(pm.sat_i8_row(dim, rng, side=side, norm=norm, sign=sign)[1], key)
            c = pm.sat_i8_query(dim, np.random.default_rng(dim + 1), norm=norm)[1]
            put(c, "query")
            put(-c, "-query")
    else:
        q_row, _ = pm.sat_fp16_row(dim, np.random.default_rng(dim))
        sign = np.sign(q_row)
        q_qt = _gauss(1, dim, rng)[0]  # the fp16 form has no query term: an ordinary query in that place
        for scale in ("tiny", "unit", "large"):
            for side, key in ((1, "row"), (-1, "-row")):
                put(pm.sat_fp16_row(dim, rng, side=side, scale=scale, sign=sign)[1], key)
    # row 0 and row n - 1: one planted variant each, another one for every (dimension, filter) case, so that over the
    # cases of a form every variant (term, side, scale) has been the first and the last row of the corpus
    for at, (key, vec) in ((0, cands[variant % len(cands)]), (n - 1, cands[(variant + 5) % len(cands)])):
        e[at] = vec
        pressed[key].append(at)
    special = range(10_000, 10_006)
    taken = {at for rows in pressed.values() for at in rows}
    assert taken.isdisjoint(special) and max(taken - {n - 1}) < 10_000, "planted rows and range rows overlap"
    # ranges: NaN, inf, huge, zero, subnormal rows
    e[10_000, 7] = np.nan
    e[10_001, 3] = np.inf
    e[10_002] = e[10_002] * 2.0 ** 62
    e[10_003] = 0.0
    e[10_004] = e[10_004] * 1e-40
    e[10_005] = e[10_005] * 1e5
    plain = e[rng.integers(12_000, n - 100)]
    spiky = plain.copy()
    spiky[3] = 50.0
    base = {"row": q_row, "query": q_qt, "planted": plain + 0.05 * _gauss(1, dim, rng)[0], "random": _gauss(1, dim, rng)[0],
            "spiky": spiky, "zero": np.zeros(dim, np.float32), "huge": plain * np.float32(1e30),
            "tiny": plain * np.float32(1e-30)}
    queries = {}
    for name, q in base.items():
        if mode == 2 and name in ("planted", "random", "spiky", "huge", "tiny"):
            q = pm.k1f8_off_ties(q)
        queries[name] = q.astype(np.float32)
        queries["-" + name] = -q.astype(np.float32)
    queries["nan"] = np.full(dim, np.nan, np.float32)
    return e, queries, pressed


def _kth_largest(s_allowed, k):
    """K1's k-th score over the allowed rows: NaN ranks first (as +inf); -inf when fewer than k rows are allowed"""
    v = np.where(np.isnan(s_allowed), np.inf, s_allowed.astype(np.float64))
    return -np.inf if v.size < k else np.partition(v, v.size - k)[v.size - k]


def _check_query(tag, stored, q, s, hi, T, k, allowed, press_rows, floor):
    """b, c, d for one query of a scan launch"""
    n = s.size
    assert not (_bits(hi) == SENTINEL).any(), f"{tag}: rows the scan never wrote: {np.flatnonzero(_bits(hi) == SENTINEL)[:8]}"
    assert _bits(T) != SENTINEL, f"{tag}: no threshold written"
    assert np.all(np.isnan(hi[~allowed])), f"{tag}: a disallowed row has a bound"
    ha, sa = hi[allowed].astype(np.float64), s[allowed]
    assert not np.isnan(ha).any(), f"{tag}: an allowed row without a bound"
    nan_s = np.isnan(sa)
    assert np.all(np.isposinf(ha[nan_s])), f"{tag}: a NaN score (ranks first) needs hi = +inf"
    below = ha[~nan_s] < sa[~nan_s].astype(np.float64)
    assert not below.any(), (f"{tag}: hi < K1's score on {int(below.sum())} rows, first "
                             f"{np.flatnonzero(allowed)[~nan_s][below][:5]}")
    kth = _kth_largest(sa, k)
    print(f"{tag}: T={float(T):.9g} k-th s={kth:.9g}")
    assert float(T) <= kth, f"{tag}: T {float(T)!r} above K1's k-th score {kth!r}"
    if allowed.sum() < k:
        assert np.isneginf(T)
    finite_q = np.isfinite(q).all() and np.linalg.norm(q.astype(np.float64)) <= pm.RADIUS_CAP
    if not finite_q:
        return
    a, r, R = stored.interval(q)
    fin = allowed & stored.finite_row & np.isfinite(a)
    # the corpus holds six rows of infinite radius at most: d and the lower bound of T must look at all the others
    assert fin.sum() >= allowed.sum() - 6, f"{tag}: only {int(fin.sum())} of {int(allowed.sum())} rows are checked"
    # d. not looser than specified
    loose = hi[fin].astype(np.float64) > a[fin] + R[fin]
    assert not loose.any(), f"{tag}: hi above a + R on rows {np.flatnonzero(fin)[loose][:5]}"
    # b. T from below: each of the k rows with the largest s has lo >= s - 2R
    if fin.sum() >= k and np.isfinite(kth):
        top = np.flatnonzero(fin)[np.argsort(-s[fin].astype(np.float64), kind="stable")[:k]]
        if np.isfinite(s[top]).all() and float(s[top][-1]) == kth:
            assert float(T) >= kth - 2.0 * float(np.max(R[top])), f"{tag}: T far below K1's k-th score"
    # c. the saturating rows press on the device's interval
    rows = np.asarray([i for i in press_rows if allowed[i]], dtype=np.int64)
    if rows.size:
        share = (s[rows].astype(np.float64) - a[rows]) / (hi[rows].astype(np.float64) - a[rows])
        print(f"{tag}: pressure on hi, min {share.min():.4f} over {rows.size} rows")
        assert np.all(share >= floor), f"{tag}: saturating rows use only {share.min():.4f} of the device's radius"


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("dim", pm.SERVED_DIMS)
def test_every_row_interval_holds_k1_score(Index, dim, mode, filtered):
    n = N_ROWS
    rng = np.random.default_rng(7 * dim + mode)
    floor = 0.85 if mode == 2 else 0.45
    with Index(0) as idx:
        idx.set_dense_prefilter(mode)
        idx.dense_load(_gauss(n, dim, rng))
        geo = idx.debug_prefilter_read(data=False)
        rpw = geo["rows_per_wave"]
        assert geo["form"] == mode and rpw % geo["batch_rows"] == 0 and n // rpw > 16
        e, queries, pressed = _plant(mode, dim, n, rpw, rng, variant=2 * pm.SERVED_DIMS.index(dim) + int(filtered))
        src = (np.arange(n) % 5).astype(np.uint16)
        src[[50, 5000, n - 2]] = 5
        idx.dense_load(e, source_id=src)
        assert idx.debug_prefilter_read(data=False)["rows_per_wave"] == rpw
        stored = Stored(mode, idx.debug_prefilter_read())
        for name, q in queries.items():
            if mode == 2 and np.isfinite(q).all() and q.any():
                assert pm.k1f8_tie_margin(q) > 1e-3, f"query {name} sits on a rounding tie of its int8 codes"
        allow_most = np.array([1, 1, 0, 1, 1, 1], np.uint8)
        allow_few = np.array([0, 0, 0, 0, 0, 1], np.uint8)
        # K1's fp32 score of every row, and proof that it is what the list-keeping scan ranks with
        idx.set_dense_prefilter(0)
        scores = {name: idx.dense_scores(q) for name, q in queries.items()}
        for name in ("row", "-query", "planted"):
            doc, sc, cnt = idx.dense_search(queries[name], 25)
            assert cnt[0] == 25 and np.array_equal(_bits(sc[0]), _bits(np.where(np.isnan(scores[name][doc[0]]), np.inf,
                                                                               scores[name][doc[0]])))
        idx.set_dense_prefilter(mode)
        names = list(queries)
        others = [x for x in names if x not in ("row", "-row", "query", "-query")]
        sat = ["row", "-row", "query", "-query"]
        groups = [(["row"], 25), (["-query"], 1),
                  (sat + others[:4], 64),                        # 8: the saturating queries first
                  (others[:6] + sat + others[6:11], 25),         # 15: in the middle
                  (others[:12] + sat, 1),                        # 16: last
                  (sat + others[:12], 25),                       # 16: first
                  (sat[:2] + others[1:13] + sat[2:], 64)]        # 16: at both ends, the NaN query among them
        for members, k in groups:
            assert 1 <= len(members) <= 16
            for allow in ([allow_most, allow_few] if filtered else [None]):
                allowed = np.ones(n, bool) if allow is None else allow[src].astype(bool)
                hi, thr = idx.debug_prefilter_bounds(np.stack([queries[m] for m in members]), k, allow_source=allow)
                for i, m in enumerate(members):
                    tag = f"D={dim} mode={mode} k={k} group={len(members)}[{i}] q={m} allowed={int(allowed.sum())}"
                    _check_query(tag, stored, queries[m], scores[m], hi[i], thr[i], k, allowed,
                                 pressed.get(m, ()), floor)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("dim", pm.SERVED_DIMS)
def test_threshold_under_rows_pressed_from_below(Index, dim, mode):
    """The top k rows are saturating rows (codes of their own) whose K1 score sits at the LOWER end of the interval:
    T is the k-th lo of rows whose s is next to lo, so a lo that is too high shows as T > K1's k-th score."""
    n, kmax = N_ROWS, 64
    rng = np.random.default_rng(11 * dim + mode)
    floor = 0.85 if mode == 2 else 0.45
    if mode == 2:
        q = pm.sat_i8_row(dim, np.random.default_rng(dim))[0]
        make = lambda: pm.sat_i8_row(dim, rng, side=-1, aligned=True, sign=np.sign(q))[1]
    else:
        q = pm.sat_fp16_row(dim, np.random.default_rng(dim))[0]
        make = lambda: pm.sat_fp16_row(dim, rng, side=-1, aligned=True, sign=np.sign(q))[1]
    e = _gauss(n, dim, rng)
    rows = rng.choice(n, kmax, replace=False)
    for at in rows:
        e[at] = make()
    with Index(0) as idx:
        idx.set_dense_prefilter(0)
        idx.dense_load(e)
        s = idx.dense_scores(q)
        idx.set_dense_prefilter(mode)
        stored = Stored(mode, idx.debug_prefilter_read())
        a, r, R = stored.interval(q)
        assert set(np.argsort(-s.astype(np.float64))[:kmax].tolist()) == set(rows.tolist())  # they are the top 64
        share = (a[rows] - s[rows].astype(np.float64)) / r[rows]
        print(f"D={dim} mode={mode}: pressure on lo, min {share.min():.4f}")
        assert np.all(share >= floor)
        for k in (1, 25, 64):
            _, thr = idx.debug_prefilter_bounds(q, k)
            kth = _kth_largest(s, k)
            print(f"D={dim} mode={mode} k={k}: T={float(thr[0]):.9g} k-th s={kth:.9g} gap/r={(kth - float(thr[0])) / r[rows].max():.4f}")
            assert float(thr[0]) <= kth, "T above K1's k-th score: lo is too high"
            assert float(thr[0]) >= kth - 2.0 * float(np.max(R[rows]))
            # and the answer is K1's
            idx.set_dense_prefilter(0)
            off = idx.dense_search(q, k)
            idx.set_dense_prefilter(mode)
            on = idx.dense_search(q, k)
            assert np.array_equal(off[0], on[0]) and np.array_equal(_bits(off[1]), _bits(on[1]))
