"""tests/wave_model.py against brute force, its generators against their own promises, and the hidden entry it drives.  No GPU."""
import math
import os
from fractions import Fraction

import mpmath
import numpy as np

import wave_model as wm


def test_fma_model_rounds_once():
    rng = np.random.default_rng(1)
    # a * b + c where the two-rounding result differs from the fused one
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30
    assert a * b - 1.0 == 0.0 and wm.fma(a, b, -1.0) == -(2.0 ** -60)
    for _ in range(2000):
        a, b, c = (float(v) for v in rng.normal(size=3) * 10.0 ** rng.integers(-30, 30, 3))
        exact = Fraction(a) * Fraction(b) + Fraction(c)
        r = wm.fma(a, b, c)
        assert abs(Fraction(r) - exact) <= Fraction(math.ulp(r)) / 2
        # brute force: no neighbour is closer
        for nb in (math.nextafter(r, math.inf), math.nextafter(r, -math.inf)):
            assert abs(Fraction(nb) - exact) >= abs(Fraction(r) - exact)
    assert math.isnan(wm.fma(math.inf, 0.0, 1.0)) and wm.fma(math.inf, 1.0, 1.0) == math.inf and math.isnan(wm.fma(1.0, math.nan, 0.0))
    assert math.copysign(1.0, wm.fma(1.0, -0.0, -0.0)) == -1.0 and math.copysign(1.0, wm.fma(2.0, 3.0, -6.0)) == 1.0
    assert wm.fma_chain(1.0, [2.0, 3.0], [4.0, 5.0]) == 24.0 and wm.exact_dot(1.0, [2.0, 3.0], [4.0, 5.0]) == 24


def test_ulp_error():
    assert wm.ulp_error(1.0, Fraction(1)) == 0.0
    assert wm.ulp_error(1.0 + 2.0 ** -52, Fraction(1)) == 1.0
    assert wm.ulp_error(1.0 - 2.0 ** -53, Fraction(1)) == 0.5               # in ulps of the correctly rounded RESULT (1.0), not of got
    assert abs(wm.ulp_error(1 / 3.0, Fraction(1, 3)) - 1 / 3.0) < 1e-9      # 0x1.5555555555555p-2 is 1/3 ulp short
    with mpmath.workprec(wm.MP_BITS):
        third = mpmath.mpf(1) / 3
    assert abs(wm.ulp_error(1 / 3.0, third) - 1 / 3.0) < 1e-9
    assert wm.ulp_error(5e-324, Fraction(0) + Fraction(5e-324) * 2) == 1.0  # subnormal spacing
    assert wm.as_ld_significand_bits() >= 64
    x = np.array([3.0, 7.0, 1e-200, 1.0 + 2.0 ** -52])
    got = 1.0 / x
    ld = wm.ulp_error_ld(got, np.longdouble(1) / x.astype(np.longdouble))
    ex = [wm.ulp_error(g, Fraction(1) / Fraction(float(v))) for g, v in zip(got, x)]
    assert np.abs(ld - ex).max() < 1e-3 and ld.max() <= 0.5


def test_wrap_models():
    assert wm.wrap_above_ref(7.5, 2.0) == 1.5 and wm.wrap_above_ref(2.0, 2.0) == 2.0 and wm.wrap_above_ref(-1.0, 2.0) == -1.0
    assert wm.wrap_below_ref(-7.5, 2.0) == 0.5 and wm.wrap_below_ref(0.0, 2.0) == 0.0 and wm.wrap_below_ref(3.0, 2.0) == 3.0
    assert wm.wrap_below_ref(-1e-20, 2.0) == 2.0                            # the closed end the header documents


def test_exact_sets_sum_exactly_in_any_order():
    rng = np.random.default_rng(2)
    for spike in (None, 0, 17, 63):
        for x in wm.gen_exact_sum_sets(rng, 12, spike_lane=spike):
            ex = wm.exact_sum(x)
            assert Fraction(math.fsum(x)) == ex
            for _ in range(6):
                p = rng.permutation(x)
                s = 0.0
                for v in p:
                    s += float(v)
                    assert math.isfinite(s)
                assert Fraction(s) == ex
                t = p.copy()                                               # a tree association
                while t.size > 1:
                    t = t[0::2] + t[1::2]
                assert Fraction(float(t[0])) == ex
    for g in (wm.gen_exact_dot(rng, (50, 20)),):
        for row in g:
            acc, ms, xs = row[0], row[1:10], row[10:19]
            ex = wm.exact_dot(acc, ms, xs)
            assert Fraction(wm.fma_chain(acc, ms, xs)) == ex
            assert Fraction(float(acc + np.sum((ms * xs)[rng.permutation(9)]))) == ex


def test_wide_sets_stay_in_range():
    rng = np.random.default_rng(3)
    x = wm.gen_wide_sum_sets(rng, 100)
    assert np.isfinite(x).all() and np.abs(x).sum(axis=1).max() < 1e152 and np.abs(x).min() > 1e-151 and np.abs(x).max() > 1e100
    # heavy cancellation: the exact sum is many orders below the sum of magnitudes
    assert np.median([abs(float(wm.exact_sum(r))) / np.abs(r).sum() for r in x[:20]]) < 1e-10
    p = wm.gen_prod_sets(rng, 100)
    lg = np.log2(np.abs(p))
    assert np.where(lg > 0, lg, 0).sum(axis=1).max() < 1000 and np.where(lg < 0, lg, 0).sum(axis=1).min() > -1000     # any subset product is normal
    w = wm.gen_wide_dot(rng, (100, 64))
    assert np.isfinite(w).all() and (np.abs(w) >= 2.0 ** -40).all() and (np.abs(w) < 2.0 ** 41).all()


def test_recip_generators_stay_in_contract():
    rng = np.random.default_rng(4)
    tiny = np.finfo(np.float64).tiny
    for x in (wm.gen_recip_inputs(rng, per_binade=40), wm.gen_recip_edges()):
        assert np.isfinite(x).all() and (np.abs(x) >= tiny).all() and (x > 0).any() and (x < 0).any()
        with np.errstate(all="raise"):
            r = 1.0 / x
        assert np.isfinite(r).all() and (np.abs(r) >= tiny).all()
    e = np.frexp(wm.gen_recip_inputs(rng, per_binade=2))[1]
    assert e.min() == -1021 and e.max() == 1022 and np.unique(e).size == 2044          # every binade (frexp's exponent is one above)
    assert wm.gen_recip_inputs(rng).size + wm.gen_recip_edges().size >= 1000000
    for x in (wm.gen_rsqrt_inputs(rng, per_binade=40), wm.gen_rsqrt_edges()):
        assert np.isfinite(x).all() and (x >= tiny).all()
        r = 1.0 / np.sqrt(x)
        assert np.isfinite(r).all() and (r >= tiny).all()
    assert wm.gen_rsqrt_inputs(rng).size + wm.gen_rsqrt_edges().size >= 1000000
    lg = wm.gen_log2_inputs(rng)
    e = np.frexp(lg)[1]
    assert (lg > 0).all() and np.isfinite(lg).all() and lg.min() == 5e-324 and e.max() == 1024 and np.unique(e).size == 2098


def test_spd_generator_hits_its_condition_number():
    rng = np.random.default_rng(5)
    for n in (2, 5, 16, 48):
        for cond in (1.0, 1e6, 1e12):
            A = wm.gen_spd(rng, n, cond)
            ev = np.linalg.eigvalsh(A)
            assert np.array_equal(A, A.T) and ev.min() > 0 and 0.9 * cond <= ev.max() / ev.min() <= 1.1 * cond, (n, cond, ev.max() / ev.min())


def test_mp_linear_algebra():
    rng = np.random.default_rng(6)
    A = wm.gen_spd(rng, 6, 1e8)
    Lm = wm.mp_cholesky(A)
    with mpmath.workprec(wm.MP_BITS):
        for i in range(6):
            for j in range(6):
                assert abs(sum(Lm[i, k] * Lm[j, k] for k in range(6)) - mpmath.mpf(float(A[i, j]))) < mpmath.mpf(2) ** -200
        B = rng.normal(size=(6, 2))
        for r in range(2):
            X = wm.mp_solve(A, B[:, r])
            for i in range(6):
                assert abs(sum(mpmath.mpf(float(A[i, k])) * X[k] for k in range(6)) - mpmath.mpf(float(B[i, r]))) < mpmath.mpf(2) ** -180


def test_debug_entry_is_exported_and_checks_its_arguments():
    """crx_debug_wave_prim is hidden (not in include/crx.h) but exported; bad launch parameters are refused before any device call."""
    import ctypes

    import crx
    L = crx.lib()
    f = L.crx_debug_wave_prim
    root = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    assert "crx_debug_wave_prim" not in open(os.path.join(root, "include", "crx.h")).read()
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    buf = np.zeros(8192)
    p = buf.ctypes.data

    def call(op, n, in_stride, out_stride, *ia):
        arr = (ctypes.c_int * 8)(*(list(ia) + [0] * (8 - len(ia))))
        return f(op, n, p, in_stride, p, out_stride, ctypes.addressof(arr))

    assert call(0, 1, 64, 64) == -1 and call(11, 1, 64, 64) == -1 and call(6, 0, 64, 128) == -1 and f(6, 1, None, 64, p, 128, None) == -1
    assert call(6, 1, 63, 128) == -1 and call(6, 1, 64, 127) == -1                     # strides shorter than the op's layout
    assert call(4, 1, 832, 64, 12, 0, 0) == -1 and call(4, 1, 832, 64, 0, 0, 3) == -1  # instantiation, mode
    assert call(4, 1, 832, 64, 4, 14, 0) == -1                                         # <7, 8> reads lane 14: not inside `lane < 14`
    assert call(8, 1, 448, 192, 7) == -1
    for ia in ((0, 0, 2, 0, 60, 1, 100, 1), (65, 0, 70, 0, 5000, 1, 6000, 1), (8, 57, 9, 0, 600, 1, 700, 1), (8, 0, 8, 0, 90, 1, 100, 1),
               (8, 0, 9, 0, 90, 1, 7000, 1), (8, 0, 9, 30, 90, 1, 100, 1), (8, 0, 9, 0, 95, 1, 100, 1), (8, 0, 9, 0, 90, 1, 100, 3),
               (8, 0, 9, 0, 50, 9, 100, 1)):
        assert call(10, 1, ia[6] + 128, ia[6] + 192, *ia) == -1, ia
