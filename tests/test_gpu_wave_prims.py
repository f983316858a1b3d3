"""Every primitive of car-racing_amd/csrc/crx_wave.h against exact references (tests/wave_model.py), one by one, through the hidden
crx_debug_wave_prim (csrc/crx_debug_wave.hip: one 64-lane workgroup per case, the header that ships).  Every bound below comes from
the algorithm or from the header's own contract (u = 2^-53); each test prints the maximum it measured before it asserts.  All data
from fixed seeds; every assertion runs over all generated cases."""
import math
import os
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import wave_model as wm
from wave_model import U

pytestmark = pytest.mark.gpu
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
LANES = np.arange(64)
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    import crx

    crx.init()
    return crx.lib()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def uniform_lanes(block):
    """all 64 lanes of a wave-uniform result hold the same bits"""
    return same_bits(block, np.repeat(block[..., :1], 64, axis=-1)).all()


# ---- lane moves ------------------------------------------------------------------------------------------------------------------
def test_lane_moves(lib):
    """lane_f64, dpp_f64 (through ROW_REDUCE), swap32_f64, swap16_f64 on lane-identifying data: lane l holds (l + 1) * 2^k (x) and
    -(l + 65) * 2^k (y), so a result names its source lane; the row reduction runs on 2^l, whose sums name the lanes that contributed."""
    k = np.arange(64) - 32
    x = (LANES[None, :] + 1.0) * 2.0 ** k[:, None]
    y = -(LANES[None, :] + 65.0) * 2.0 ** k[:, None]
    out = wm.prim(lib, wm.OP_LANES, np.concatenate([x, y], axis=1), 384)
    for c in range(64):
        assert same_bits(out[c, :64], np.full(64, x[c, c])).all(), c          # case c reads lane c
    # swap32(a, b): a' = (a.lo32, b.lo32), b' = (a.hi32, b.hi32);  swap16(s1, s2): s1' = rows [s1.0 s2.0 s1.2 s2.2], s2' = rows [s1.1 s2.1 s1.3 s2.3]
    r = [slice(0, 16), slice(16, 32), slice(32, 48), slice(48, 64)]
    a32 = np.concatenate([x[:, :32], y[:, :32]], axis=1)
    b32 = np.concatenate([x[:, 32:], y[:, 32:]], axis=1)
    a16 = np.concatenate([x[:, r[0]], y[:, r[0]], x[:, r[2]], y[:, r[2]]], axis=1)
    b16 = np.concatenate([x[:, r[1]], y[:, r[1]], x[:, r[3]], y[:, r[3]]], axis=1)
    for name, got, want in (("swap32 x'", out[:, 128:192], a32), ("swap32 y'", out[:, 192:256], b32), ("swap16 x'", out[:, 256:320], a16),
                            ("swap16 y'", out[:, 320:384], b16)):
        assert same_bits(got, want).all(), name
    p = np.tile(2.0 ** LANES, (4, 1)) * np.array([[1.0], [3.0], [2.0 ** -600], [-5.0 * 2.0 ** 500]])
    out = wm.prim(lib, wm.OP_LANES, np.concatenate([p, p], axis=1), 384)
    want = np.repeat(p.reshape(4, 4, 16).sum(axis=2), 16, axis=1)            # 2^l: the sum of a row is exact and names its 16 lanes
    assert same_bits(out[:, 64:128], want).all()


# ---- reductions ------------------------------------------------------------------------------------------------------------------
SUM_SLOTS = (("wave_sum", 0, 0), ("wave_sum2.a", 128, 0), ("wave_sum2.b", 192, 1), ("wave_sum4.a", 256, 0), ("wave_sum4.b", 320, 1),
             ("wave_sum4.c", 384, 2), ("wave_sum4.d", 448, 3))      # name, output offset, input it reduces
MAX_SLOTS = (("wave_max", 0, 0, np.fmax), ("wave_min", 64, 1, np.fmin), ("wave_max2.c", 128, 2, np.fmax), ("wave_max2.d", 192, 3, np.fmax),
             ("wave_max4.a", 256, 0, np.fmax), ("wave_max4.b", 320, 1, np.fmax), ("wave_max4.c", 384, 2, np.fmax), ("wave_max4.d", 448, 3, np.fmax))


def test_wave_sums_exact_sets(lib):
    """(a) integers times powers of two whose sums are exact in any association, a 2^40 spike in each of the 64 lanes in turn, four
    independent sets per case (disjoint sums: a value in the wrong slot of a packed reduction is a different number): bit-equal in
    all 64 lanes."""
    rng = np.random.default_rng(101)
    x = np.stack([np.concatenate([wm.gen_exact_sum_sets(rng, 1, spike_lane=l)[0] for _ in range(4)]) for l in range(64)])
    out = wm.prim(lib, wm.OP_SUMS, x, 512)
    xs = x.reshape(64, 4, 64)
    want = np.array([[float(wm.exact_sum(xs[c, q])) for q in range(4)] for c in range(64)])
    assert len({float(v) for v in want.ravel()}) == want.size
    for name, off, q in SUM_SLOTS:
        assert same_bits(out[:, off:off + 64], np.repeat(want[:, q:q + 1], 64, axis=1)).all(), name
    # products: +-2^k and two odd integers per set, in each pair of lanes (l, 63 - l): exact
    b = 2.0 ** rng.integers(-14, 15, (64, 64)) * rng.choice([-1.0, 1.0], (64, 64))
    for l in range(64):
        b[l, l] *= 2 * rng.integers(1, 1 << 19) + 1
        b[l, 63 - l] *= 2 * rng.integers(1, 1 << 19) + 1
    x[:, 64:128] = b
    out = wm.prim(lib, wm.OP_SUMS, x, 512)
    want = np.array([float(math.prod(Fraction(float(v)) for v in b[c])) for c in range(64)])
    assert same_bits(out[:, 64:128], np.repeat(want[:, None], 64, axis=1)).all()


def test_wave_sums_wide_range(lib):
    """(b) magnitudes 1e-150 .. 1e150 with heavy cancellation: |err| <= 63 u sum|x| (any association of 63 additions); products of
    2^-14 .. 2^15 factors: relative 63 u.  Every lane returns the same value."""
    rng = np.random.default_rng(102)
    n = 200
    x = np.concatenate([wm.gen_wide_sum_sets(rng, n) for _ in range(4)], axis=1)
    out = wm.prim(lib, wm.OP_SUMS, x, 512)
    xs = x.reshape(n, 4, 64)
    exact = [[wm.exact_sum(xs[c, q]) for q in range(4)] for c in range(n)]
    worst = 0.0
    for name, off, q in SUM_SLOTS:
        assert uniform_lanes(out[:, off:off + 64]), name
        for c in range(n):
            bound = 63 * Fraction(U) * sum(Fraction(float(abs(v))) for v in xs[c, q])
            err = abs(Fraction(float(out[c, off])) - exact[c][q])
            worst = max(worst, float(err / bound))
            assert err <= bound, (name, c, float(err), float(bound))
    b = wm.gen_prod_sets(rng, n)
    x[:, 64:128] = b
    out = wm.prim(lib, wm.OP_SUMS, x, 512)
    assert uniform_lanes(out[:, 64:128])
    wp = 0.0
    for c in range(n):
        ex = math.prod(Fraction(float(v)) for v in b[c])
        rel = abs(Fraction(float(out[c, 64])) / ex - 1)
        wp = max(wp, float(rel / Fraction(U)))
        assert rel <= 63 * Fraction(U), (c, float(rel))
    print("wave sums: worst |err| / (63 u sum|x|) = %.3f; wave_prod: worst relative error %.2f u (bound 63 u)" % (worst, wp))


def test_wave_sums_specials(lib):
    """(c) one inf -> inf, one NaN -> NaN, +inf and -inf together -> NaN, wherever they sit."""
    rng = np.random.default_rng(103)
    cases, want = [], []
    for l in (0, 15, 16, 31, 32, 47, 48, 63):
        for kind in range(3):
            x = rng.normal(size=(4, 64))
            if kind == 0:
                x[:, l] = np.inf
            elif kind == 1:
                x[:, l] = NAN
            else:
                x[:, l] = np.inf
                x[:, (l + 21) % 64] = -np.inf
            cases.append(x.ravel())
            want.append(np.inf if kind == 0 else NAN)
    out = wm.prim(lib, wm.OP_SUMS, np.array(cases), 512)
    for name, off, q in SUM_SLOTS:
        assert same_bits(np.abs(out[:, off:off + 64]), np.repeat(np.array(want)[:, None], 64, axis=1)).all(), name


def test_wave_max_min(lib):
    """wave_max / wave_min / wave_max2 / wave_max4: random, ties, signed zeros, the extremum in each lane in turn, NaN in some lanes and
    in all: equal AS VALUES in every lane (the sign of a zero result is not asserted), fmax / fmin semantics for NaN."""
    rng = np.random.default_rng(104)
    cases = [rng.normal(size=(4, 64)) * 10.0 ** rng.integers(-200, 200) for _ in range(40)]
    cases += [rng.integers(-2, 3, (4, 64)).astype(np.float64) for _ in range(20)]                     # ties
    cases += [rng.choice([0.0, -0.0], (4, 64)) for _ in range(8)]                                     # -0.0 vs +0.0
    for l in range(64):                                                                               # the extremum in lane l
        x = rng.normal(size=(4, 64))
        x[:, l] = [7.0, -7.0, 8.0, 9.0]          # max of inputs 0, 2, 3; min of input 1
        x[0, (l + 1) % 64] = -9.0                # a larger |value| of the other sign must not win
        cases.append(x)
    for cnt in (1, 5, 32, 63):                                                                        # NaN in some lanes
        for _ in range(6):
            x = rng.normal(size=(4, 64))
            for q in range(4):
                x[q, rng.choice(64, cnt, replace=False)] = NAN
            cases.append(x)
    cases.append(np.full((4, 64), NAN))
    x = np.array(cases)
    out = wm.prim(lib, wm.OP_MAXS, x.reshape(len(cases), 256), 512)
    with np.errstate(invalid="ignore"):
        for name, off, q, op in MAX_SLOTS:
            want = op.reduce(x[:, q, :], axis=1)
            got = out[:, off:off + 64]
            ok = (got == want[:, None]) | (np.isnan(got) & np.isnan(want)[:, None])
            assert ok.all(), (name, np.argwhere(~ok)[:4])


# ---- dot products ------------------------------------------------------------------------------------------------------------------
def _dot_data(rng, n_m, n_each):
    """[cases, 64] arrays x, x2, acc, m[n_m]: exact sets, wide-range sets, large accumulators against cancelling terms; every lane and
    every term its own value (all four 16-lane rows differ)."""
    X, X2, ACC, M = [], [], [], []
    for kind in ("exact", "wide", "cancel"):
        g = wm.gen_exact_dot if kind == "exact" else wm.gen_wide_dot
        x, x2, acc, m = g(rng, (n_each, 64)), g(rng, (n_each, 64)), g(rng, (n_each, 64)), g(rng, (n_m, n_each, 64))
        if kind == "cancel":
            m = rng.uniform(1, 2, m.shape) * rng.choice([-1.0, 1.0], m.shape)
            x = rng.uniform(1, 2, x.shape) * 2.0 ** 30
            x2 = rng.uniform(-1, 1, x.shape)
            acc = -np.sum(m[:6], axis=0) * 1.5 * 2.0 ** 30 * (1 + 1e-9 * rng.normal(size=acc.shape))
        X.append(x); X2.append(x2); ACC.append(acc); M.append(m)
    return np.concatenate(X), np.concatenate(X2), np.concatenate(ACC), np.concatenate(M, axis=1)


def _check_dot(name, got, lanes, model, exact_terms, cnt, bad_bits, bad_bound):
    """got / model per (case, lane); exact_terms(case, lane) -> (acc, ms, xs) of the LAST fma chain, for the weaker bound
    |err| <= CNT u (|acc| + sum |m_i x_i|), reported separately from the bit comparison."""
    for c in range(got.shape[0]):
        for l in lanes:
            if not same_bits(got[c, l], model[c][l]):
                bad_bits.append((name, c, l, float(got[c, l]), model[c][l]))
                acc, ms, xs = exact_terms(c, l)
                if all(math.isfinite(v) for v in (acc, *ms, *xs)):
                    scale = abs(Fraction(acc)) + sum(abs(Fraction(m) * Fraction(x)) for m, x in zip(ms, xs))
                    if abs(Fraction(float(got[c, l])) - wm.exact_dot(acc, ms, xs)) > cnt * Fraction(U) * scale:
                        bad_bound.append((name, c, l))


@pytest.mark.parametrize("inst", range(len(wm.ROW_DOT)), ids=["row_dot<%d,%d>" % p for p in wm.ROW_DOT])
def test_row_dot(lib, inst):
    """row_dot<CNT, FIRST>: acc += m[i] * (lane FIRST + i of the reader's 16-lane row), i ascending, one fused rounding per term --
    BIT-EQUAL to the sequential-fma model, in all four rows, under full EXEC and inside `if (lane < NZ)` (NZ = 8, 10, 12, 14 where the
    region holds the lanes read; the other lanes keep their sentinel), with x loaded, produced by a VALU add right in front of the
    call, and chained (x = acc = what the previous dot product has just written).  The weaker error bound is evaluated for every
    mismatch so that a failure says which of the two claims broke."""
    cnt, first = wm.ROW_DOT[inst]
    rng = np.random.default_rng(200 + inst)
    n_each = 6
    x, x2, acc, m = _dot_data(rng, 9, n_each)
    nc = x.shape[0]
    sent = -12345.0 - LANES[None, :] + np.zeros((nc, 1))
    inp = np.concatenate([x, x2, acc] + [m[i] for i in range(9)] + [sent], axis=1)
    bad_bits, bad_bound = [], []
    for nz in (0, 8, 10, 12, 14):
        if nz and first + cnt > nz:
            continue
        lanes = range(64) if nz == 0 else range(nz)
        for mode in (0, 1, 2):
            out = wm.prim(lib, wm.OP_ROWDOT, inp, 64, (inst, nz, mode))
            xe = x + x2 if mode == 1 else x
            src = lambda l, i: 16 * (l // 16) + first + i
            stage1 = [{l: wm.fma_chain(acc[c, l], [m[i, c, l] for i in range(cnt)], [xe[c, src(l, i)] for i in range(cnt)]) for l in lanes}
                      for c in range(nc)]
            if mode < 2:
                model = stage1
                terms = lambda c, l: (float(acc[c, l]), [float(m[i, c, l]) for i in range(cnt)], [float(xe[c, src(l, i)]) for i in range(cnt)])
            else:
                model = [{l: wm.fma_chain(stage1[c][l], [m[i, c, l] for i in range(cnt)], [stage1[c][src(l, i)] for i in range(cnt)])
                          for l in lanes} for c in range(nc)]
                terms = lambda c, l: (stage1[c][l], [float(m[i, c, l]) for i in range(cnt)], [stage1[c][src(l, i)] for i in range(cnt)])
            _check_dot("nz=%d mode=%d" % (nz, mode), out, lanes, model, terms, cnt, bad_bits, bad_bound)
            if nz:
                assert same_bits(out[:, nz:], sent[:, nz:]).all(), ("sentinel", nz, mode)
    assert not bad_bound, ("error bound CNT u (|acc| + sum|m x|) broken", bad_bound[:5])
    assert not bad_bits, ("not the bits of the sequential fma chain (the error bound holds)", len(bad_bits), bad_bits[:5])


def test_halfrow_dot6(lib):
    """halfrow_dot6: lane 8 g + c returns sum_{j < 6} m[j] * x(lane 8 g + j) as an fma chain from 0, j ascending -- bit-equal in all
    eight half-rows, each with its own data; lanes 6 and 7 of every half-row hold NaN / inf in x (not among the six read: must not
    leak); m[j] NaN in one half-row must stay in that half-row."""
    rng = np.random.default_rng(300)
    x, x2, _, m = _dot_data(rng, 6, 16)
    nc = x.shape[0]
    x[:, 6::8] = NAN
    x[:, 7::8] = np.inf
    x2[:, 6::8] = 0.0
    x2[:, 7::8] = 0.0
    nan_half = {}
    for c in range(0, nc, 2):                       # every second case: one term of one half-row is NaN
        h, j = (c // 2) % 8, (c // 16) % 6
        m[j, c, 8 * h:8 * h + 8] = NAN
        nan_half[c] = h
    inp = np.concatenate([x, x2] + [m[j] for j in range(6)], axis=1)
    bad_bits, bad_bound = [], []
    for mode in (0, 1):
        out = wm.prim(lib, wm.OP_HALFROW, inp, 64, (0, 0, mode))
        xe = x + x2 if mode == 1 else x
        model = [{l: wm.fma_chain(0.0, [m[j, c, l] for j in range(6)], [xe[c, 8 * (l // 8) + j] for j in range(6)]) for l in range(64)}
                 for c in range(nc)]
        terms = lambda c, l: (0.0, [float(m[j, c, l]) for j in range(6)], [float(xe[c, 8 * (l // 8) + j]) for j in range(6)])
        _check_dot("mode=%d" % mode, out, range(64), model, terms, 6, bad_bits, bad_bound)
        for c, h in nan_half.items():
            isn = np.isnan(out[c])
            assert isn[8 * h:8 * h + 8].all() and not np.delete(isn, np.s_[8 * h:8 * h + 8]).any(), (c, h)
    assert not bad_bound, bad_bound[:5]
    assert not bad_bits, (len(bad_bits), bad_bits[:5])


# ---- scans -------------------------------------------------------------------------------------------------------------------------
def _scan_check(out, x, exact_only):
    worst = 0.0
    for c in range(x.shape[0]):
        fx = [Fraction(float(v)) for v in x[c]]
        for name, off in (("prefix", 0), ("suffix", 64)):
            for i in range(64):
                summed = fx[:i] if name == "prefix" else fx[i + 1:]
                ex = sum(summed, Fraction(0))
                got = float(out[c, off + i])
                if exact_only:
                    assert same_bits(got, float(ex)), (name, c, i, got, float(ex))
                else:
                    bound = 63 * Fraction(U) * sum(abs(v) for v in summed)
                    err = abs(Fraction(got) - ex)
                    assert err <= bound, (name, c, i, float(err), float(bound))
                    if bound:
                        worst = max(worst, float(err / bound))
    return worst


def test_excl_scans(lib):
    """excl_prefix / excl_suffix: lane i = sum of the lanes before / after it.  Exact sets bit-equal in all 64 lanes; wide-range random
    to 63 u * sum|x| over the summed lanes; a 1e300 spike in lane i among values of order 1: lane i itself returns the sum of the OTHERS
    to that bound (no cancellation: inclusive-minus-own would be off by 1e284); a NaN in lane j reaches exactly the lanes that sum it;
    lane 0 (prefix) / 63 (suffix) is exactly 0."""
    rng = np.random.default_rng(400)
    xe = wm.gen_exact_sum_sets(rng, 24)
    out = wm.prim(lib, wm.OP_SCANS, xe, 128)
    _scan_check(out, xe, True)
    assert (out[:, 0] == 0).all() and (out[:, 127] == 0).all()
    xw = np.concatenate([wm.gen_wide_sum_sets(rng, 24), rng.normal(size=(24, 64))])
    spikes = (0, 15, 16, 31, 32, 47, 48, 63)
    xs = rng.uniform(0.5, 2.0, (len(spikes), 64)) * rng.choice([-1.0, 1.0], (len(spikes), 64))
    for r, i in enumerate(spikes):
        xs[r, i] = 1e300
    xa = np.concatenate([xw, xs])
    out = wm.prim(lib, wm.OP_SCANS, xa, 128)
    worst = _scan_check(out, xa, False)
    assert (out[:, 0] == 0).all() and (out[:, 127] == 0).all()
    print("excl_prefix / excl_suffix: worst |err| / (63 u sum|x|) = %.3f" % worst)
    nan_lanes = list(range(64))
    xn = rng.normal(size=(64, 64))
    clean = wm.prim(lib, wm.OP_SCANS, xn, 128)
    for j in nan_lanes:
        xn[j, j] = NAN
    out = wm.prim(lib, wm.OP_SCANS, xn, 128)
    for j in nan_lanes:
        assert same_bits(out[j, :j + 1], clean[j, :j + 1]).all() and np.isnan(out[j, j + 1:64]).all(), ("prefix", j)
        assert same_bits(out[j, 64 + j:], clean[j, 64 + j:]).all() and np.isnan(out[j, 64:64 + j]).all(), ("suffix", j)


# ---- frcp / frsqrt / log2_fast -------------------------------------------------------------------------------------------------------
def _pad64(v, fill=1.0):
    n = (len(v) + 63) // 64 * 64
    return np.concatenate([v, np.full(n - len(v), fill)]).reshape(-1, 64), len(v)


def _recip_run(lib, v, col):
    a, n = _pad64(np.asarray(v, dtype=np.float64))
    return wm.prim(lib, wm.OP_RECIP, a, 192)[:, 64 * col:64 * col + 64].ravel()[:n]


def _mp_recip(x):
    with mpmath.workprec(wm.MP_BITS):
        return 1 / mpmath.mpf(float(x))


def _mp_rsqrt(x):
    with mpmath.workprec(wm.MP_BITS):
        return 1 / mpmath.sqrt(mpmath.mpf(float(x)))


def _ulp_judged(x, got, ref_ld, mp_ref, edges):
    """ulp errors: bulk against longdouble, everything above 0.75 ulp and all `edges` re-judged with mpmath."""
    err = wm.ulp_error_ld(got, ref_ld)
    for i in np.flatnonzero((err > 0.75) | edges):
        err[i] = wm.ulp_error(got[i], mp_ref(x[i]))
    return err


def test_frcp(lib):
    """frcp: >= 1e6 values -- random mantissas in every binade where x and 1/x are both normal, both signs; mantissas within 4 ulp of
    1 and 2; odd integers scaled.  Error <= 1 ulp of the correctly rounded 1/x: the last Newton step is ONE fma rounding of a value
    that differs from 1/x by O(delta1^2), i.e. half an ulp plus that term; 1 ulp is the header's contract."""
    assert wm.as_ld_significand_bits() >= 64
    rng = np.random.default_rng(500)
    bulk, edge = wm.gen_recip_inputs(rng), wm.gen_recip_edges()
    x = np.concatenate([bulk, edge])
    assert x.size >= 1000000
    got = _recip_run(lib, x, 0)
    assert np.isfinite(got).all()
    err = _ulp_judged(x, got, np.longdouble(1) / x.astype(np.longdouble), _mp_recip, np.arange(x.size) >= bulk.size)
    i = int(np.argmax(err))
    print("frcp: max error %.4f ulp at x = %r over %d values; not correctly rounded: %.3f %%" % (err[i], x[i], x.size, 100.0 * np.mean(err > 0.5)))
    assert err.max() <= 1.0, (err[i], x[i])


def test_frsqrt(lib):
    """frsqrt: every binade of the normal range, mantissas around 1, 2 and 4 (both exponent parities).  Error <= 2 ulp: the last step
    r * fma(hx r, r, 1.5) rounds three times (hx r enters halved, the fma, the product): 0.5 u + u + u = 2.5 u = 1.25 ulp at the
    bottom of a binade, plus the Newton remainder 1.5 delta1^2."""
    rng = np.random.default_rng(501)
    bulk, edge = wm.gen_rsqrt_inputs(rng), wm.gen_rsqrt_edges()
    x = np.concatenate([bulk, edge])
    assert x.size >= 1000000
    got = _recip_run(lib, x, 1)
    assert np.isfinite(got).all()
    err = _ulp_judged(x, got, np.longdouble(1) / np.sqrt(x.astype(np.longdouble)), _mp_rsqrt, np.arange(x.size) >= bulk.size)
    i = int(np.argmax(err))
    print("frsqrt: max error %.4f ulp at x = %r over %d values; above 1 ulp: %.4f %%" % (err[i], x[i], x.size, 100.0 * np.mean(err > 1.0)))
    assert err.max() <= 2.0, (err[i], x[i])


OFF_CONTRACT = [0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.0 ** -1023, 1.5 * 2.0 ** -1023, 2.0 ** -1022 * (1 - 2.0 ** -52), math.inf, -math.inf, NAN,
                1.25 * 2.0 ** 1022, 2.0 ** 1023, 1.5 * 2.0 ** 1023, -1.75 * 2.0 ** 1023, 1.7976931348623157e308, -1.0, -2.5e-300, -1e300]


def test_frcp_frsqrt_off_contract(lib):
    """Outside the contract (zeros, subnormals, inf, NaN, subnormal results, frsqrt of negatives) there is no accuracy claim, only
    safety: the result is the IEEE value to the bound of the contract (1 ulp / 2 ulp, in ulps of the possibly subnormal result), or it
    is not finite -- never a finite wrong number.  Prints the table that the header documents."""
    x = np.array(OFF_CONTRACT)
    rc, rs = _recip_run(lib, x, 0), _recip_run(lib, x, 1)
    print("%-24s %-24s %-24s" % ("x", "frcp(x)", "frsqrt(x)"))
    for xi, a, b in zip(x, rc, rs):
        print("%-24r %-24r %-24r" % (float(xi), float(a), float(b)))
    for xi, a, b in zip(x, rc, rs):
        xi, a, b = float(xi), float(a), float(b)
        if math.isfinite(a):
            assert math.isfinite(xi) and xi != 0.0, (xi, a)                   # 1/0 and 1/NaN have no finite value; 1/inf = 0:
            assert wm.ulp_error(a, _mp_recip(xi)) <= 1.0, ("frcp", xi, a)
        if math.isinf(xi) and math.isfinite(a):
            assert a == 0.0
        if math.isfinite(b):
            assert xi > 0.0 and math.isfinite(xi), ("frsqrt", xi, b)
            assert wm.ulp_error(b, _mp_rsqrt(xi)) <= 2.0, ("frsqrt", xi, b)


def _mp_log2(v):
    with mpmath.workprec(96):
        return [float(mpmath.log(mpmath.mpf(float(t)), 2)) for t in v]


def test_log2_fast(lib):
    """log2_fast over every binary exponent -1074 .. 1023: |err| <= 2e-7 against mpmath -- 2^-24 / ln 2 = 8.6e-8 from rounding the
    mantissa to float, one float ulp at magnitude <= 1 (6e-8) from the hardware log, margin for the final double add.
    log2_fast(0) = -inf.  The switching test of the filter, log2(al) + 2.3 log2(-Dphi) - 1.1 log2(theta), keeps its sign wherever the
    exact gap exceeds (1 + 2.3 + 1.1) * 2e-7."""
    rng = np.random.default_rng(600)
    x = wm.gen_log2_inputs(rng)
    got = _recip_run(lib, x, 2)
    err = np.abs(got - np.array(_mp_log2(x)))
    i = int(np.argmax(err))
    print("log2_fast: max |err| = %.3e at x = %r over %d values" % (err[i], x[i], x.size))
    assert err.max() <= 2e-7, (err[i], x[i])
    assert (_recip_run(lib, np.array([0.0, -0.0]), 2) == -np.inf).all()
    n = 20000
    al, dphi, th = 10.0 ** rng.uniform(-10, 0, n), 10.0 ** rng.uniform(-20, 12, n), 10.0 ** rng.uniform(-20, 12, n)
    # half of the cases sit close to the switching surface: al chosen so that the exact gap is within ~1e-5 of zero
    k = n // 2
    th[:k] = 10.0 ** rng.uniform(-12, 4, k)
    dphi[:k] = 10.0 ** rng.uniform(-8, 2, k)
    al[:k] = 2.0 ** (1.1 * np.log2(th[:k]) - 2.3 * np.log2(dphi[:k]) + rng.normal(0, 1e-5, k))
    keep = (al > 1e-300) & (al < 1e300)
    al, dphi, th = al[keep], dphi[keep], th[keep]
    lg = _recip_run(lib, np.concatenate([al, dphi, th]), 2).reshape(3, -1)
    gap = lg[0] + 2.3 * lg[1] - 1.1 * lg[2]
    ex = np.array(_mp_log2(al)) + 2.3 * np.array(_mp_log2(dphi)) - 1.1 * np.array(_mp_log2(th))
    decided = np.abs(ex) > 4.4 * 2e-7
    print("switching expression: %d of %d cases decided (|gap| > 8.8e-7), %d within 1e-4 of the surface; max |gap error| %.3e" % (
        decided.sum(), decided.size, (np.abs(ex) < 1e-4).sum(), np.abs(gap - ex).max()))
    assert decided.sum() > n // 2 and (np.abs(ex) < 1e-4).sum() > n // 4
    assert ((gap > 0) == (ex > 0))[decided].all()


def test_logacc(lib):
    """LogAcc::wave_total / wave_total_with: sum over the wave of log v for k = 1 .. 6 factors per lane in 1e-20 .. 1e12 (the slacks'
    range), all ones, powers of two only: |err| <= (64 k + 8) u (1 + |total|) against mpmath (64 k mantissa products rounded once
    each, one log, an exact exponent sum).  `other` of wave_total_with obeys the wave_sum rule."""
    rng = np.random.default_rng(700)
    worst = 0.0
    for k in range(1, 7):
        v = np.ones((30, 7, 64))
        v[:10, :6] = 10.0 ** rng.uniform(-20, 12, (10, 6, 64))
        v[20:, :6] = 2.0 ** rng.integers(-66, 40, (10, 6, 64))            # rows 10 .. 19: all ones
        v[:, 6] = rng.normal(size=(30, 64)) * 10.0 ** rng.uniform(-3, 3, (30, 1))
        out = wm.prim(lib, wm.OP_LOGACC, v.reshape(30, 448), 192, (k,))
        assert uniform_lanes(out[:, :64]) and uniform_lanes(out[:, 64:128]) and uniform_lanes(out[:, 128:])
        for c in range(30):
            with mpmath.workprec(wm.MP_BITS):
                tot = mpmath.fsum(mpmath.log(mpmath.mpf(float(t))) for t in v[c, :k].ravel())
                bound = (64 * k + 8) * U * (1 + abs(tot))
                for name, got in (("wave_total", out[c, 0]), ("wave_total_with", out[c, 64])):
                    err = abs(mpmath.mpf(float(got)) - tot)
                    worst = max(worst, float(err / bound))
                    assert err <= bound, (name, k, c, float(got), float(tot), float(err), float(bound))
            so = [Fraction(float(t)) for t in v[c, 6]]
            assert abs(Fraction(float(out[c, 128])) - sum(so)) <= 63 * Fraction(U) * sum(abs(t) for t in so), ("other", k, c)
    print("LogAcc: worst |err| / ((64 k + 8) u (1 + |total|)) = %.3f" % worst)


# ---- lap wraps -----------------------------------------------------------------------------------------------------------------------
def _lap_lengths():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "car-racing_amd"))
    from utils import racing_env
    track = racing_env.ClosedTrack(np.genfromtxt(os.path.join(ROOT, "data/track_layout/l_shape.csv"), delimiter=","), track_width=1.0)
    return [float(track.lap_length), 1.0]


def _wrap_run(lib, s, L):
    a, n = _pad64(np.asarray(s, dtype=np.float64))
    b, _ = _pad64(np.asarray(L, dtype=np.float64))
    out = wm.prim(lib, wm.OP_WRAPS, np.concatenate([a, b], axis=1), 128)
    return out[:, :64].ravel()[:n], out[:, 64:].ravel()[:n]


def test_lap_wraps(lib):
    """wrap_above / wrap_below.  Within four laps (s in (-4 L, 5 L), exact multiples of L, s == L, s == 0): bit-equal to the
    reference's `while s > L: s -= L` / `while s < 0: s += L`.  Beyond (5 .. 1e6 laps, 1e15 laps): the result lies in (0, L]
    (above) / [0, L] (below: `s += L` rounds to L itself when -s is below half an ulp of L, in the reference's loop as well), and
    its distance ON THE CIRCLE from the exact representative of s mod L is <= 4 u |s| (one rounded quotient-times-L product and two
    subtractions; on the circle because a residue within that distance of an end point may come out at the other end).  Garbage
    (L <= 0, L = NaN, s = NaN / +-inf / +-1e301) is returned unchanged."""
    rng = np.random.default_rng(800)
    for L in _lap_lengths():
        s = np.concatenate([rng.uniform(-4, 5, 4000) * L, np.arange(-4, 6) * L, [L, 0.0, -0.0, np.nextafter(L, 9e9), np.nextafter(L, 0), -5e-324, 5e-324],
                            np.nextafter(np.arange(-4, 6) * L, 9e9), np.nextafter(np.arange(-4, 6) * L, -9e9)])
        s = s[(s > -4 * L) & (s < 5 * L)]
        up, dn = _wrap_run(lib, s, np.full(s.size, L))
        assert same_bits(up, [wm.wrap_above_ref(float(v), L) for v in s]).all()
        assert same_bits(dn, [wm.wrap_below_ref(float(v), L) for v in s]).all()
        laps = np.concatenate([rng.uniform(5, 1e6, 3000), 10.0 ** rng.uniform(0.7, 6, 3000), np.arange(5, 40), rng.uniform(0.99e15, 1.01e15, 500),
                               np.full(8, 1e15)])
        for sign in (1.0, -1.0):
            s = sign * laps * L
            up, dn = _wrap_run(lib, s, np.full(s.size, L))
            got = up if sign > 0 else dn
            assert ((got > 0) & (got <= L)).all() if sign > 0 else ((got >= 0) & (got <= L)).all(), (sign, got.min(), got.max())
            fl, worst = Fraction(L), 0.0
            for v, g in zip(s, got):
                fs = Fraction(float(v))
                d = (Fraction(float(g)) - fs) % fl            # the exact residue differs from the result by a whole number of laps ...
                d = min(d, fl - d)                            # ... up to this distance on the circle
                worst = max(worst, float(d / (4 * Fraction(U) * abs(fs))))
                assert d <= 4 * Fraction(U) * abs(fs), (float(v), float(g), float(d))
            print("wrap_%s, L = %r: worst circle distance / (4 u |s|) = %.3f" % ("above" if sign > 0 else "below", L, worst))
            other = dn if sign > 0 else up                    # the other wrap has nothing to do
            assert same_bits(other, s).all()
    g = [(3.0, -1.0), (-3.0, -1.0), (3.0, 0.0), (-3.0, 0.0), (3.0, -0.0), (3.0, NAN), (-3.0, NAN), (NAN, 2.0), (math.inf, 2.0), (-math.inf, 2.0),
         (1e301, 2.0), (-1e301, 2.0), (1e301, -2.0), (-1e301, -2.0), (math.inf, -2.0), (-math.inf, NAN), (NAN, NAN), (-7.5, -math.inf), (7.5, -math.inf)]
    s, Lg = np.array([a for a, _ in g]), np.array([b for _, b in g])
    up, dn = _wrap_run(lib, s, Lg)
    assert same_bits(up, s).all(), (up, s)
    assert same_bits(dn, s).all(), (dn, s)


# ---- Cholesky and back-substitution in LDS -----------------------------------------------------------------------------------------------
def _chol_layout(n, extra, LD, base, inv_mode):
    """LDS image: `base` doubles of padding, 4 * ceil(n / 4) rows at least (the panel loop READS rows and columns up to n + 2), the
    inverse pivots either in their own array behind it (inv_st = 1) or in the padding column from row 1 on (inv_st = LD, the LMPC form)."""
    rows = max(n + extra, (n + 3) // 4 * 4)
    end = base + rows * LD + 4
    if isinstance(inv_mode, int):                           # an array of its own at a given offset
        inv, inv_st = inv_mode, 1
        assert inv >= end
        total = inv + n + 5
    elif inv_mode == "own":
        inv, inv_st = end + 3, 1
        total = inv + n + 5
    else:
        inv, inv_st = base + LD + LD - 1, LD            # last column of row 1, then down that column: rows 1 .. n
        total = max(end, inv + (n - 1) * LD + 1) + 5
    return rows, inv, inv_st, total


def _chol_run(lib, A_list, E_list, B_list, n, extra, LD, base, inv_mode, nr):
    rows, inv, inv_st, total = _chol_layout(n, extra, LD, base, inv_mode)
    rng = np.random.default_rng(n * 1000 + extra * 10 + LD)
    imgs = []
    for A, E, B in zip(A_list, E_list, B_list):
        img = rng.normal(size=total) * 1e3 + 7e5            # canary: every double the factorisation has no business with
        for i in range(n):
            img[base + i * LD: base + i * LD + i + 1] = A[i, :i + 1]
        for r in range(extra):
            img[base + (n + r) * LD: base + (n + r) * LD + n] = E[r]
        b = np.zeros((2, 64))
        b[:, :n] = B.T
        imgs.append(np.concatenate([img, b.ravel()]))
    inp = np.array(imgs)
    out = wm.prim(lib, wm.OP_CHOL, inp, total + 192, (n, extra, LD, base, inv, inv_st, total, nr))
    written = np.zeros(total, dtype=bool)
    for i in range(n):
        written[base + i * LD: base + i * LD + i + 1] = True
    for r in range(extra):
        written[base + (n + r) * LD: base + (n + r) * LD + n] = True
    written[inv + np.arange(n) * inv_st] = True
    written[base + LD - 1] = True                           # the one documented sink of the masked stores
    return inp, out, written, (rows, inv, inv_st, total)


def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def _chol_check(inp, out, written, lay, A_list, E_list, B_list, n, extra, LD, base, nr, stats):
    rows, inv, inv_st, total = lay
    for c, (A, E, B) in enumerate(zip(A_list, E_list, B_list)):
        img = out[c, :total]
        assert out[c, total + 128] == 1.0 and uniform_lanes(out[c:c + 1, total + 128:total + 192]), "l_chol returned 0 on an SPD matrix"
        assert same_bits(img[~written], inp[c, :total][~written]).all(), ("canary", n, extra, LD, base, np.flatnonzero(~same_bits(img, inp[c, :total]) & ~written)[:6])
        Lf = np.zeros((n + extra, n))
        for i in range(n + extra):
            w = min(i + 1, n)
            Lf[i, :w] = img[base + i * LD: base + i * LD + w]
        full = np.vstack([A, E]) if extra else A
        # |A - L L'| <= (n + 12) u |L||L'|: Higham's gamma_(n+1) for Cholesky plus 2 * 5 u, every entry being s * rinv with rinv within 2 ulp (4 u)
        # and one product rounding.  longdouble residual (11 more bits than the bound needs), re-judged exactly when above half of it.
        Ll = _ld(Lf)
        res = np.abs(_ld(full) - Ll @ Ll[:n].T)
        bnd = (n + 12) * U * (np.abs(Ll) @ np.abs(Ll[:n]).T)
        mask = np.tril(np.ones((n + extra, n), dtype=bool))
        mask[n:] = True
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(mask, np.where(bnd > 0, res / np.where(bnd > 0, bnd, 1), np.where(res > 0, np.inf, 0)), 0).astype(np.float64)
        if ratio.max() > 0.5:
            for i, j in np.argwhere(ratio > 0.5):
                ex = abs(Fraction(float(full[i, j])) - sum(Fraction(float(Lf[i, k])) * Fraction(float(Lf[j, k])) for k in range(n)))
                bx = (n + 12) * Fraction(U) * sum(abs(Fraction(float(Lf[i, k])) * Fraction(float(Lf[j, k]))) for k in range(n))
                ratio[i, j] = float(ex / bx)
        stats["factor"] = max(stats["factor"], float(ratio.max()))
        assert ratio.max() <= 1.0, ("factor", n, extra, LD, base, c, float(ratio.max()))
        # inverse pivots: sm[inv + j inv_st] = frsqrt(d_j) with L_jj = fl(d_j * rinv): within 2 ulp of 1 / sqrt(L_jj / rinv), plus the u / 2
        # relative that the rounding of that diagonal product leaves open (d_j itself is not stored)
        for j in range(n):
            rinv = float(img[inv + j * inv_st])
            with mpmath.workprec(wm.MP_BITS):
                ref = 1 / mpmath.sqrt(mpmath.mpf(float(Lf[j, j])) / mpmath.mpf(rinv))
                e = float(abs(mpmath.mpf(rinv) - ref) / mpmath.mpf(math.ulp(rinv)))
            stats["rinv"] = max(stats["rinv"], e)
            assert e <= 2.0 + 0.5 * U * rinv / math.ulp(rinv), ("rinv", n, j, e)
        # x = L^-T b: residual |L' x - b| <= (n + 6) u |L'||x|; forward error <= 8 n u cond against mpmath as a cross-check
        for r in range(nr):
            x = out[c, total + 64 * r: total + 64 * r + n]
            Lt = _ld(Lf[:n]).T
            rs = np.abs(Lt @ _ld(x) - _ld(B[:, r]))
            rb = (n + 6) * U * (np.abs(Lt) @ np.abs(_ld(x)))
            rr = float(np.max(np.where(rb > 0, rs / np.where(rb > 0, rb, 1), np.where(rs > 0, np.inf, 0))))
            stats["solve"] = max(stats["solve"], rr)
            assert rr <= 1.0, ("backsub residual", n, extra, LD, c, r, rr)
            xm = wm.mp_solve(Lf[:n].T, B[:, r])
            with mpmath.workprec(wm.MP_BITS):
                fe = max(abs(mpmath.mpf(float(x[i])) - xm[i]) for i in range(n)) / max(abs(xm[i]) for i in range(n))
            cond = np.linalg.cond(Lf[:n].T, np.inf)      # (n + 6) u cond_inf bounds the relative forward error in the max norm; n + 6 <= 8 n
            stats["forward"] = max(stats["forward"], float(fe) / (8 * n * U * cond))
            assert fe <= 8 * n * U * cond, ("backsub forward error", n, c, float(fe), cond)
        if nr == 1:                                          # the second right-hand side is not touched
            assert same_bits(out[c, total + 64: total + 128], inp[c, total + 64: total + 128]).all()
        assert same_bits(out[c, total + n: total + 64], inp[c, total + n: total + 64]).all()        # lanes >= n keep their entry


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 24, 31, 32, 48])
def test_l_chol_backsub(lib, n):
    """l_chol + l_backsub<1>, <2> on SPD matrices of condition 1, 1e6, 1e12: extra = 0, 1, 7 carried rows, LD = n + 1 and a padded one,
    base = 0 and != 0, the inverse pivots in their own array (inv_st = 1) and down the padding column (inv_st = LD).  Factor against the
    exact input, inverse pivots, solve residual, forward error and the canary of the untouched LDS: bounds in _chol_check."""
    rng = np.random.default_rng(900 + n)
    stats = dict(factor=0.0, rinv=0.0, solve=0.0, forward=0.0)
    combo = 0
    for extra in (0, 1, 7):
        for LD in (n + 1, n + 6):
            base, inv_mode, nr = (0, 5)[combo % 2], ("own", "column")[(combo // 2) % 2], 1 + (combo + combo // 3) % 2
            combo += 1
            conds = (1.0, 1e6, 1e12) if n > 1 else (1.0,)
            A_list = [wm.gen_spd(rng, n, cd) * 10.0 ** rng.integers(-3, 4) for cd in conds]
            E_list = [rng.normal(size=(extra, n)) for _ in conds]
            B_list = [rng.normal(size=(n, 2)) for _ in conds]
            inp, out, written, lay = _chol_run(lib, A_list, E_list, B_list, n, extra, LD, base, inv_mode, nr)
            _chol_check(inp, out, written, lay, A_list, E_list, B_list, n, extra, LD, base, nr, stats)
    print("l_chol n = %d: worst factor residual / bound %.3f, inverse pivot %.3f ulp, solve residual / bound %.3f, forward error / bound %.3g" % (
        n, stats["factor"], stats["rinv"], stats["solve"], stats["forward"]))


def test_l_chol_shipped_shapes(lib):
    """The two shapes the kernels call.  Learning MPC (crx_lmpc.hip, NMAX = 12): nv = 24 or 30 unknowns in an image of LDK = 31 columns, 7
    carried rows, the inverse pivots down the padding column from row 1 on (ik = K + LDK + 30, IKS = LDK).  Path planner (crx_prep.hip): a
    tridiagonal system of n unknowns with the right-hand side as ONE carried row, PATH_LD = 25, the pivots in an array of their own behind the image (IK = 28 * 25)."""
    rng = np.random.default_rng(950)
    stats = dict(factor=0.0, rinv=0.0, solve=0.0, forward=0.0)
    for n, extra, LD, mode in ((30, 7, 31, "column"), (24, 7, 31, "column"), (12, 1, 25, 700), (24, 1, 25, 700)):
        A_list = [wm.gen_spd(rng, n, cd) for cd in (1e2, 1e8)]
        if mode == 700:                                      # tridiagonal, as the path planner's Hessian
            A_list = [np.diag(rng.uniform(4, 6, n)) + np.diag(rng.uniform(-2, 0, n - 1), -1) for _ in A_list]
            A_list = [a + np.tril(a, -1).T for a in A_list]
        E_list = [rng.normal(size=(extra, n)) for _ in A_list]
        B_list = [rng.normal(size=(n, 2)) for _ in A_list]
        inp, out, written, lay = _chol_run(lib, A_list, E_list, B_list, n, extra, LD, 0, mode, 1)
        _chol_check(inp, out, written, lay, A_list, E_list, B_list, n, extra, LD, 0, 1, stats)
    print("l_chol shipped shapes: worst factor residual / bound %.3f, inverse pivot %.3f ulp, solve residual / bound %.3f" % (
        stats["factor"], stats["rinv"], stats["solve"]))


@pytest.mark.parametrize("n", [5, 8, 13])
def test_l_chol_bad_pivot(lib, n):
    """A pivot that is 0, negative or NaN -- in each position of a 4-column panel and in the last, partial panel -- makes l_chol return 0
    (every lane); the same matrix with the pivot repaired returns 1."""
    rng = np.random.default_rng(980 + n)
    A_list, want = [], []
    for j in range(n):
        for kind in ("zero", "negative", "nan", "good"):
            Lt = np.tril(rng.uniform(0.5, 1.5, (n, n)) * rng.choice([-1.0, 1.0], (n, n)))
            Lt = np.round(Lt * 8) / 8                       # multiples of 1/8: A = L L' and every pivot are exact in float64
            np.fill_diagonal(Lt, np.abs(np.diag(Lt)) + 1)
            Lt[j, :j] = 0.0                                 # row j starts with zeros: pivot j is A[j, j] itself, whatever the columns before it rounded to
            A = Lt @ Lt.T
            if kind == "zero":
                A[j, j] -= Lt[j, j] ** 2                    # pivot j becomes exactly 0
            elif kind == "negative":
                A[j, j] -= Lt[j, j] ** 2 + 0.125
            elif kind == "nan":
                A[j, j] = NAN
            A_list.append(A)
            want.append(1.0 if kind == "good" else 0.0)
    E_list = [np.zeros((1, n)) for _ in A_list]
    B_list = [np.ones((n, 2)) for _ in A_list]
    inp, out, written, (rows, inv, inv_st, total) = _chol_run(lib, A_list, E_list, B_list, n, 1, n + 1, 0, "own", 1)
    ok = out[:, total + 128: total + 192]
    assert same_bits(ok, np.repeat(np.array(want)[:, None], 64, axis=1)).all(), np.flatnonzero(ok[:, 0] != np.array(want))
    for c in range(len(A_list)):                            # bad pivot or not: nothing outside the documented footprint is touched
        assert same_bits(out[c, :total][~written], inp[c, :total][~written]).all(), c
