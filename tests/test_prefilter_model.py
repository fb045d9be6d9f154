"""CPU: the bound-saturating inputs of tests/prefilter_model.py do what they are for.  Measured against the reference
formulas of DESIGN.md §3 alone (no kernel runs here): the exact dot product sits at >= 0.9 of the radius from the
approximate score for the int8 constructions and >= 0.5 for the fp16 one, at all six served dimensions -- so a radius
that loses a term, or a fifth of its size, no longer contains K1's score on these rows."""
import numpy as np
import pytest

import prefilter_model as pm


def _i8_row(q, e):
    """the model's image and per-row data of one row, from the reference formulas"""
    s_e = pm.i8_scale(np.max(np.abs(e)))
    u = pm.i8_quantise(e, s_e)
    m1, m2 = pm.k1f8_required(e[None], u[None], np.array([s_e]))
    a, r, terms = pm.k1f8_interval(u[None], np.array([[s_e, m1[0], m2[0], 0.0]]), q)
    return u, s_e, a[0], r[0], {k: v[0] for k, v in terms.items()}


@pytest.mark.parametrize("dim", pm.SERVED_DIMS)
@pytest.mark.parametrize("norm", [2.0 ** -20, 1.0, 2.0 ** 20])
@pytest.mark.parametrize("aligned", [False, True])
def test_int8_row_term_is_saturated(dim, norm, aligned):
    for side in (1, -1):
        q, e = pm.sat_i8_row(dim, np.random.default_rng(dim + side), side=side, norm=norm, aligned=aligned)
        u, s_e, a, r, terms = _i8_row(q, e)
        assert np.max(np.abs(u)) == 127 and 0.4 * norm < np.linalg.norm(e.astype(np.float64)) < 2.5 * norm
        assert np.array_equal(np.abs(pm.k1f8_query(q)[1]), np.full(dim, 127))  # the query quantises exactly
        assert terms["query"] == 0.0
        assert pm.k1f8_tie_margin(q) > 1e-3
        exact = q.astype(np.float64) @ e.astype(np.float64)
        assert np.sign(exact - a) == side
        p = pm.pressure(q, e, a, r)
        print(f"int8 row term D={dim} norm={norm:g} side={side:+d} aligned={aligned}: {p:.4f}")
        assert 0.9 <= p <= 1.0
        # ... and the same with -q: the other side of the same row
        a2, r2, _ = pm.k1f8_interval(u[None], np.array([[s_e, 0, 0, 0]]), -q)
        assert a2[0] == -a and np.sign(-exact - a2[0]) == -side


@pytest.mark.parametrize("dim", pm.SERVED_DIMS)
@pytest.mark.parametrize("norm", [2.0 ** -20, 1.0, 2.0 ** 20])
def test_int8_query_term_is_saturated(dim, norm):
    for side in (1, -1):
        q, e = pm.sat_i8_query(dim, np.random.default_rng(dim + 7 + side), side=side, norm=norm)
        u, s_e, a, r, terms = _i8_row(q, e)
        assert np.array_equal(np.abs(u), np.full(dim, 127))  # the row quantises exactly
        assert float(s_e) * 127.0 == abs(float(e[0])) and 0.4 * norm < np.linalg.norm(e.astype(np.float64)) < 2.5 * norm
        assert np.max(pm.k1f8_query(q)[1]) == 127 and pm.k1f8_tie_margin(q) > 1e-3
        assert terms["query"] > 10 * terms["row"]  # the row term is gamma ||q|| ||e|| alone here
        exact = q.astype(np.float64) @ e.astype(np.float64)
        assert np.sign(exact - a) == side
        p = pm.pressure(q, e, a, r)
        print(f"int8 query term D={dim} norm={norm:g} side={side:+d}: {p:.4f}")
        assert 0.9 <= p <= 1.0


@pytest.mark.parametrize("dim", pm.SERVED_DIMS)
@pytest.mark.parametrize("scale", ["tiny", "unit", "large"])
@pytest.mark.parametrize("aligned", [False, True])
def test_fp16_row_term_is_saturated(dim, scale, aligned):
    for side in (1, -1):
        q, e = pm.sat_fp16_row(dim, np.random.default_rng(dim + 3 + side), side=side, scale=scale, aligned=aligned)
        h = pm.k1f_image(e)
        assert np.all(np.isfinite(h.astype(np.float64)))
        mant, expo = np.frexp(np.abs(h.astype(np.float64)))
        if scale == "tiny":
            assert np.all(np.abs(h.astype(np.float64)) < 2.0 ** -14)  # fp16 subnormals: one grid
        else:
            assert len(set(expo.tolist())) == 1  # one binade
        nrm = np.linalg.norm(e.astype(np.float64))
        lo, hi = {"tiny": (2.0 ** -21, 2.0 ** -17), "unit": (0.4, 2.5), "large": (2.0 ** 18, 2.0 ** 21)}[scale]
        assert lo < nrm < hi
        m = pm.k1f_required_m(e[None], h[None])
        a, r = pm.k1f_interval(h[None], m, q)
        exact = q.astype(np.float64) @ e.astype(np.float64)
        assert np.sign(exact - a[0]) == side
        p = pm.pressure(q, e, a[0], r[0])
        print(f"fp16 row term D={dim} scale={scale} side={side:+d} aligned={aligned}: {p:.4f}")
        assert 0.5 <= p <= 1.0


def test_ordinary_rows_do_not_press():
    """the gap the saturating inputs close: unit-norm Gaussian rows use a small share of the int8 radius"""
    rng = np.random.default_rng(0)
    for dim, share in ((256, 0.15), (768, 0.09), (2048, 0.06)):
        e = rng.standard_normal((2000, dim)).astype(np.float32)
        e /= np.linalg.norm(e, axis=1, keepdims=True)
        q = e[0] + 0.05 * rng.standard_normal(dim).astype(np.float32)
        s_e = np.array([pm.i8_scale(np.max(np.abs(row))) for row in e])
        u = np.stack([pm.i8_quantise(row, s) for row, s in zip(e, s_e)])
        m1, m2 = pm.k1f8_required(e, u, s_e)
        a, r, _ = pm.k1f8_interval(u, np.stack([s_e, m1, m2, 0 * m1], axis=1), q)
        used = np.max(np.abs(e.astype(np.float64) @ q.astype(np.float64) - a) / r)
        print(f"ordinary rows D={dim}: {used:.3f} of the radius")
        assert used <= 2 * share


def test_outward_radius_and_required_radii_edges():
    e = np.zeros((5, 256), np.float32)
    e[1, 3] = np.nan
    e[2, 3] = np.inf
    e[3] = 1e19                                     # norm past 2^60
    e[4] = 1e5                                      # past fp16's 65504
    h = pm.k1f_image(e)
    m = pm.k1f_required_m(e, h)
    assert m[0] == 0.0 and np.all(np.isinf(m[1:]))
    s_e = np.array([pm.i8_scale(np.nanmax(np.abs(row))) if np.isfinite(row).all() else 1.0 for row in e])
    u = np.stack([pm.i8_quantise(row, s) for row, s in zip(e, s_e)])
    m1, m2 = pm.k1f8_required(e, u, s_e)
    assert m1[0] == 0.0 and s_e[0] == 1.0 and np.all(np.isinf(m1[1:4])) and np.isfinite(m1[4])
    assert pm.outward(1.0, 1.0) > 1.0 and pm.gamma(2048) > 2048 * pm.U


def test_build_keeps_fp32_division_correctly_rounded():
    """the model's 1 / s_q and max / 127 are numpy's correctly rounded fp32 quotients; hipcc's default is the same
    unless the build asks for fast or approximate division.  This only reads the Makefile's text, not what the compiler
    was given in the end: what makes the model's codes the device's is that every int8 test query is kept more than
    1e-3 steps from a rounding tie (`k1f8_tie_margin`), far more than a reciprocal one ulp off could move it."""
    import os

    mk = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "a-nice-rag_amd", "csrc",
                           "Makefile")).read()
    for flag in ("-ffast-math", "-Ofast", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-freciprocal-math",
                 "-funsafe-math-optimizations", "-cl-fast-relaxed-math"):
        assert flag not in mk, flag
