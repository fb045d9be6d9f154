"""A plain fp64 model of the dense prefilter's score intervals ("K1F" and "K1F8"), and inputs that
press on them.  numpy only: tests/test_prefilter_model.py checks the inputs against these formulas without a GPU,
tests/test_gpu_dense_prefilter_bounds.py checks the kernels of dense_prefilter.hip against them.

The interval of a row with approximate score a is [a - r, a + r]:
  K1F   a = q . fp16(e),          r = ||q|| m + eta,                                m >= ||e - e~|| + gamma (||e|| + ||e~||)
  K1F8  a = (v . u) s_q s_e,      r = ||q|| m1 + ||q - q~|| m2 + 2^-22 |a| + eta,   m1 >= ||e - e~|| + gamma ||e||, m2 >= ||e~||
with gamma = D u / (1 - D u), u = 2^-24, eta = D 2^-120, e~ the stored image of the row, q~ = s_q v the query codes.
Everything here is evaluated in fp64 from the image and the per-row data AS STORED by the load-time kernels; the
`required_*` functions compute, from the fp32 rows, what those per-row data must at least be."""
import numpy as np

U = 2.0 ** -24
SERVED_DIMS = (256, 512, 768, 1024, 1536, 2048)
RADIUS_CAP = 2.0 ** 60          # ||e|| or ||q|| past this: infinite radius
LOAD_WIDENING = 1.0 + 2.0 ** -20  # stored radii <= required * this (kernel: (1 + 2^-30), then rounded up to fp32: 2^-23)


def gamma(dim):
    return dim * U / (1.0 - dim * U)


def eta(dim):
    return dim * 2.0 ** -120


def _norm(x):
    return np.sqrt(np.sum(np.square(np.asarray(x, np.float64)), axis=-1))


def outward(a, r):
    """R: the widest radius the device's fp32 evaluation may give around the model's a (finite rows and queries).
    r is widened by (1 + 2^-22) (K1F) or (1 + 2^-21) (K1F8) after one to three FMAs each within 2^-24, from fp32
    norms and radii rounded up by at most 2^-23 each (a product of two: 2^-22): below r (1 + 2^-19) in all.  a +- r is
    rounded once (2^-24) and pushed out by (1 + 2^-22): below 2^-21 (|a| + r); that also holds the 3 x 2^-24 |a| by
    which K1F8's fp32 a = fl(fl(S) fl(s_q s_e)) may differ from the exact product.  K1F's a is an fp32 SUM: the fp16
    form adds `k1f_a_slack` to this."""
    return r * (1.0 + 2.0 ** -19) + 2.0 ** -21 * (np.abs(a) + r)


# ---------------------------------------------------------------- K1F
def k1f_image(e):
    with np.errstate(over="ignore"):
        return np.asarray(e, np.float32).astype(np.float16)  # round to nearest even


def k1f_required_m(e, image):
    """||e - e~|| + gamma (||e|| + ||e~||) per row, fp64; +inf where the row is non-finite or past the cap."""
    e64, h64 = np.asarray(e, np.float64), np.asarray(image, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ne, nh = _norm(e64), _norm(h64)
        m = _norm(e64 - h64) + gamma(e64.shape[-1]) * (ne + nh)
    bad = ~np.isfinite(m) | ~(ne <= RADIUS_CAP) | ~(nh <= RADIUS_CAP)
    return np.where(bad, np.inf, m)


def k1f_interval(image, m, q):
    """(a, r) per row from the stored image and radii."""
    q64 = np.asarray(q, np.float64)
    a = np.asarray(image, np.float64) @ q64
    r = _norm(q64) * np.asarray(m, np.float64) + eta(q64.size)
    return a, r


# lanes that share a row in the fp16 scan (the Half column of prefilter_dispatch in dense_prefilter.hip)
K1F_SCAN_G = {256: 32, 512: 32, 768: 32, 1024: 64, 1536: 64, 2048: 64}


def k1f_a_slack(abs_image, q):
    """By how much the device's fp32 a may differ from the fp64 a: each lane sums its D / G products with one FMA
    chain (one rounding per FMA), a tree of log2 G additions sums the lanes, so every product passes through at most
    n = D / G + log2 G roundings: |a_fp32 - a| <= gamma_n sum |q_i e~_i| (Higham, Accuracy and Stability of Numerical
    Algorithms, section 3.1).  abs_image: |e~| per row."""
    dim = np.asarray(q).size
    g = K1F_SCAN_G[dim]
    n = dim // g + int(np.log2(g))
    return n * U / (1.0 - n * U) * (np.asarray(abs_image, np.float64) @ np.abs(np.asarray(q, np.float64)))


# ---------------------------------------------------------------- K1F8
def i8_scale(mx):
    """fp32 max|x| / 127; a zero, vanished or non-finite quotient takes 1."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.float32(mx) / np.float32(127.0)
    return s if (s > 0 and np.isfinite(s)) else np.float32(1.0)


def i8_quantise(x, s):
    """codes of x at scale s, in the device's fp32 steps: rint(x * (1 / s)) clamped to +-127."""
    x = np.asarray(x, np.float32)
    inv = np.float32(1.0) / np.float32(s)
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.rint(x * inv)
    return np.clip(np.nan_to_num(y, nan=-127.0, posinf=127.0, neginf=-127.0), -127, 127).astype(np.int32)


def k1f8_query(q):
    """(s_q, v): the query's scale and codes."""
    q = np.asarray(q, np.float32)
    with np.errstate(invalid="ignore"):
        s = i8_scale(np.max(np.abs(q)))
    return s, i8_quantise(q, s)


def k1f8_tie_margin(q):
    """distance of the nearest q_i / s_q from a rounding tie (k + 1/2), in steps"""
    q = np.asarray(q, np.float32)
    s, _ = k1f8_query(q)
    t = q.astype(np.float64) / float(s)
    t = t[np.abs(t) < 127.0]
    return float(np.min(np.abs(np.abs(t - np.floor(t)) - 0.5))) if t.size else 0.5


def k1f8_off_ties(q, margin=2e-3):
    """q with every component that lies within `margin` steps of a rounding tie of its int8 code moved 3 margins away
    (the largest component, which sets the scale, is never near one): the model's codes are then the device's,
    whatever the last bit of x * (1 / s_q) does."""
    q = np.array(q, np.float32)
    s = float(k1f8_query(q)[0])
    t = q.astype(np.float64) / s
    near = (np.abs(np.abs(t - np.floor(t)) - 0.5) < margin) & (np.abs(t) < 126.0)
    q[near] = ((np.floor(t[near]) + 0.5 + 3 * margin) * s).astype(np.float32)
    return q


def k1f8_required(e, codes, s_e):
    """(m1, m2) per row: ||e - e~|| + gamma ||e|| and ||e~||, e~ = s_e u, fp64; m1 = +inf for non-finite / capped rows."""
    e64 = np.asarray(e, np.float64)
    t = np.asarray(codes, np.float64) * np.asarray(s_e, np.float64)[..., None]
    with np.errstate(invalid="ignore", over="ignore"):
        ne, nt = _norm(e64), _norm(t)
        m1 = _norm(e64 - t) + gamma(e64.shape[-1]) * ne
    bad = ~np.isfinite(m1) | ~(ne <= RADIUS_CAP) | ~(nt <= RADIUS_CAP)
    return np.where(bad, np.inf, m1), nt


def k1f8_interval(codes, meta, q):
    """(a, r, terms) per row from the stored codes and {s_e, m1, m2, 0}; terms = the summands of r, one per key."""
    q32 = np.asarray(q, np.float32)
    q64 = q32.astype(np.float64)
    s_q, v = k1f8_query(q32)
    meta = np.asarray(meta, np.float64)
    S = np.asarray(codes, np.float64) @ v.astype(np.float64)  # integers below 2^25: exact
    a = S * float(s_q) * meta[..., 0]
    terms = {"row": _norm(q64) * meta[..., 1], "query": _norm(q64 - float(s_q) * v) * meta[..., 2],
             "product": 2.0 ** -22 * np.abs(a), "eta": np.full(a.shape, eta(q64.size))}
    return a, terms["row"] + terms["query"] + terms["product"] + terms["eta"], terms


# ---------------------------------------------------------------- inputs that saturate the bound
# Each builder returns (q, e): fp32 vectors such that K1's score q . e sits at (nearly) a + side * r.  The perturbation
# is 0.49 of a step, not 0.5: no value sits on a rounding tie.  Scales are powers of two, so that the device's
# max / 127 reproduces them exactly.
PERTURB = 0.49


def _pow2_near(x):
    return 2.0 ** np.round(np.log2(x))


def _codes(rng, dim, sign, aligned, lo, hi):
    mag = rng.integers(lo, hi + 1, dim)
    return (sign * mag if aligned else rng.choice([-1, 1], dim) * mag).astype(np.int64)


def sat_i8_row(dim, rng, side=1, norm=1.0, aligned=False, sign=None):
    """The row term ||q|| ||e - e~||: q_i = +-c (its codes are +-127 exactly), e_i = s_e (u_i + side 0.49 sign q_i),
    one code pinned at 127 so that the row's scale is s_e.  aligned: u_i has q_i's sign (a high score).  sign: the signs
    of q (drawn when None), so that many rows with codes of their own press on one query."""
    sign = rng.choice([-1, 1], dim) if sign is None else np.asarray(sign)
    q = (127.0 * 2.0 ** -11 * sign).astype(np.float32)
    u = _codes(rng, dim, sign, aligned, 40, 126)
    s_e = _pow2_near(norm / (86.0 * np.sqrt(dim)))
    e = s_e * (u + side * PERTURB * sign)
    e[0] = s_e * 127.0 * (sign[0] if aligned else 1.0)
    return q, e.astype(np.float32)


def sat_i8_query(dim, rng, side=1, norm=1.0):
    """The query term ||q - q~|| ||e~||: e_i = +-c (codes +-127 exactly), q_i = s_q (v_i + 0.49 sign e_i) with one code
    pinned at 127.  side = -1: the row -e, whose score sits at the lower end."""
    sign = rng.choice([-1, 1], dim)
    c = 127.0 * _pow2_near(norm / (127.0 * np.sqrt(dim)))
    v = _codes(rng, dim, sign, False, 40, 126)
    q = 2.0 ** -11 * (v + PERTURB * sign)
    q[0] = 2.0 ** -11 * 127.0
    return q.astype(np.float32), (side * c * sign).astype(np.float32)


def sat_fp16_row(dim, rng, side=1, scale="unit", aligned=False, sign=None):
    """K1F's row term: q_i = +-c, every |e_i| on the fp16 grid of ONE binade (mantissas 1025 .. 2046 of 2048, clear of
    the binade's ends) plus side 0.49 ulp sign q_i.  scale: "unit" (row norm ~1), "tiny" (~2^-19: fp16 subnormals,
    grid 2^-24, mantissas 1 .. 2) or "large" (the top binades fp16 holds, norm 2^18.6 .. 2^20)."""
    sign = rng.choice([-1, 1], dim) if sign is None else np.asarray(sign)
    q = (2.0 ** -4 * sign).astype(np.float32)
    if scale == "tiny":
        ulp, n = 2.0 ** -24, _codes(rng, dim, sign, aligned, 1, 2)
    else:
        top = 2.0 ** 14 if scale == "large" else _pow2_near(1.0 / (1.5 * np.sqrt(dim)))
        ulp, n = top * 2.0 ** -10, _codes(rng, dim, sign, aligned, 1025, 2046)
    e = ulp * (n + side * PERTURB * sign)
    return q, e.astype(np.float32)


def pressure(q, e, a, r):
    """|q . e - a| / r with the exact (fp64) dot product: the share of the radius these inputs use."""
    return abs(float(np.asarray(q, np.float64) @ np.asarray(e, np.float64)) - float(a)) / float(r)
