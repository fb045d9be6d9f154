"""A plain fp64 model of the widened bound of the float64-query prefilter ("K1FD"), on top of
prefilter_model.py's intervals, and an input that presses on the widening.  numpy only:
tests/test_prefilter_f64_model_cpu.py checks the argument without a GPU, tests/test_gpu_dense_prefilter_f64.py checks
dense_prefilter_f64.hip and the host route against it.

q is the float64 query, q^ = fl32(q) what the shadow scan reads, [lo, hi] the scan's interval of a row for q^.  The
fp64 list scan's score s64 of the row (D FMAs and a 6-step butterfly on exactly converted values, any order) satisfies
    |s64 - q^.e| <= (gamma64 ||q|| + delta) ||e||,    gamma64 = D 2^-53 / (1 - D 2^-53),  delta = ||q - q^||,
so with Emax = max ||e|| over the rows whose norm is finite and <= 2^60 (the others have an infinite radius)
    w = (delta + gamma64 ||q||) Emax + D 2^-1000,     lo - w <= s64 <= hi + w,
and the survivors hi >= T - 2w (T the k-th largest lo) hold the fp64 top k."""
import math

import numpy as np

import prefilter_model as pm

U64 = 2.0 ** -53


def gamma64(dim):
    return dim * U64 / (1.0 - dim * U64)


def q32_of(q):
    """fl32(q), component by component, round to nearest even; out of range -> +-inf."""
    with np.errstate(over="ignore"):
        return np.asarray(q, np.float64).astype(np.float32)


def emax_of(e):
    """The largest fp64 row norm over rows whose norm is finite and at most 2^60 (0.0 when there is none)."""
    with np.errstate(invalid="ignore", over="ignore"):
        ne = np.sqrt(np.sum(np.square(np.asarray(e, np.float64)), axis=-1))
    ok = np.isfinite(ne) & (ne <= pm.RADIUS_CAP)
    return float(ne[ok].max()) if ok.any() else 0.0


def delta_of(q):
    """||q - q^||: every component difference is exact in fp64, its square too (<= 29 significant bits)."""
    q = np.asarray(q, np.float64)
    d = q - q32_of(q).astype(np.float64)
    return math.sqrt(math.fsum((d * d).tolist()))


def required_w(q, emax):
    """The widening the argument needs, in fp64 to nearest (math.fsum: the sums are rounded once): a device value may
    not lie below it.  Non-finite (a component outside fp32's range, a NaN): every row is a survivor."""
    q = np.asarray(q, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        qn = math.sqrt(math.fsum((q * q).tolist())) if np.all(np.isfinite(q)) else math.inf
        delta = delta_of(q) if np.all(np.isfinite(q32_of(q))) else math.inf
    return (delta + gamma64(q.size) * qn) * emax + q.size * 2.0 ** -1000


def survivors(hi, T, w):
    """Rows with hi >= T - 2w (NaN: rows the filter rejects, never); a non-finite w keeps every row with a non-NaN hi."""
    hi = np.asarray(hi, np.float64)
    if not math.isfinite(w):
        return ~np.isnan(hi)
    with np.errstate(invalid="ignore"):
        return hi >= float(T) - 2.0 * w


def intervals(form, e, q32):
    """(lo, hi) per row in fp64 from the image and the per-row data the load would at least store (prefilter_model's
    required_* values: the tightest intervals the design allows), for the fp32 query q32.  form 1: fp16, 2: int8."""
    e = np.asarray(e, np.float32)
    if form == 1:
        img = pm.k1f_image(e)
        a, r = pm.k1f_interval(img, pm.k1f_required_m(e, img), q32)
    else:
        with np.errstate(invalid="ignore"):
            s_e = np.array([pm.i8_scale(np.max(np.abs(row))) for row in e], np.float32)
        codes = np.stack([pm.i8_quantise(row, s) for row, s in zip(e, s_e)])
        m1, m2 = pm.k1f8_required(e, codes, s_e)
        meta = np.stack([s_e.astype(np.float64), m1, m2, np.zeros_like(m1)], axis=1)
        a, r, _ = pm.k1f8_interval(codes, meta, q32)
    return a - r, a + r


# ---------------------------------------------------------------- an input that saturates the widening
def pressing_query(q32, rng):
    """q_i = q^_i +- 0.49 ulp32(q^_i): a float64 query as far from its fp32 rounding as one gets without a tie."""
    q32 = np.asarray(q32, np.float32)
    step = np.spacing(np.abs(q32)).astype(np.float64)  # the gap above |q^_i|; half of it below a power of two
    assert not np.any(np.frexp(q32)[0] == 0.5), "a component on a binade's edge: its lower gap is half as wide"
    q = q32.astype(np.float64) + rng.choice([-1.0, 1.0], q32.size) * pm.PERTURB * step
    assert np.array_equal(q32_of(q), q32)
    return q


def pressing_row(q, norm):
    """e* proportional to fl32(q - q^) with ||e*|| = norm: (q - q^).e* = delta ||e*|| up to fp32 rounding of e*."""
    q = np.asarray(q, np.float64)
    d = q - q32_of(q).astype(np.float64)
    return (d * (norm / np.linalg.norm(d))).astype(np.float32)


def exact_dot(a, b):
    """The real product of two vectors of doubles, rounded once."""
    from fractions import Fraction

    return float(sum(Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b)))
