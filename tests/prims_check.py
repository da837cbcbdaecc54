"""The checks of the device primitives, written once against the `Prims` interface (tests/prims_probe.py):
tests/test_gpu_prims.py runs them on the probe library (the shipped headers on the GPU), tests/test_prims_host.py on the CPU
emulation and on its mutants, each of which must be rejected.  Every check asserts the bound the code's own comment
states (or one derived in its docstring) and returns the figures it measured.

References: tests/prims_ref.py.  Inputs are seeded; nothing here depends on what the code under test returns."""
import math

import numpy as np

import prims_ref as R
from prims_probe import mass_column_capacity

LN2 = math.log(2.0)
NOFLUX = 99.999          # B9_MAG_NOFLUX (include/base9_hip.h)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------------
# transcendentals and division
# ------------------------------------------------------------------------------------------------------------------
def log_inputs(seed=11):
    rng = np.random.default_rng(seed)
    e = np.repeat(np.arange(-1022, 1024), 128)                         # every binary exponent of the normal range
    e = np.concatenate([e, rng.integers(-1022, 1024, (1 << 18) - e.size)])
    binades = np.ldexp(1.0 + rng.random(e.size), e)
    near = rng.uniform(0.5, 2.0, 1 << 16)
    dense = []
    for c in (math.sqrt(0.5), math.sqrt(2.0), 1.0):                    # where the `lt` branch switches, and x -> 1
        steps = np.arange(-2048, 2049)
        dense.append(c + steps * math.ulp(c) * 0.5)
        dense.append(c * (1.0 + rng.uniform(-1e-9, 1e-9, 4096)))
        dense.append(c * (1.0 + rng.uniform(-1e-3, 1e-3, 4096)))
    pm = np.array([1.0 + s * 2.0 ** -j for j in range(1, 53) for s in (1, -1)])
    return dict(binades=binades, near_one=np.concatenate([near] + dense), one_pm=pm)


def check_log(P):
    """log_ge1 / log_pos <= 1 ulp (the comment's "error < 1 ulp" / "1 ulp" for any positive normal x)."""
    fig = {}
    worst = 0.0
    for name, x in log_inputs().items():
        for fn in ("log_pos", "log_ge1"):
            xx = x if fn == "log_pos" else x[x >= 1.0]
            got = P.map1(fn, xx)
            err, k = R.screened_max(got, [xx], np.log, R.mp_log, R.spacing_np, 1.0)
            fig[f"{fn} {name}"] = err
            assert err <= 1.0, f"{fn}({xx[k]!r}) = {got[k]!r}: {err:.3f} ulp from log"
            worst = max(worst, err)
    # the production call log_ge1(mant + mant), mant in [0.5, 1) (mix_wave_total)
    mant = np.concatenate([0.5 + 0.5 * np.random.default_rng(12).random(1 << 16), [0.5, np.nextafter(1.0, 0.0), np.nextafter(0.5, 1.0)]])
    got = P.map1("log_ge1", mant + mant)
    err, k = R.screened_max(got, [mant + mant], np.log, R.mp_log, R.spacing_np, 1.0)
    fig["log_ge1(mant + mant)"] = err
    assert err <= 1.0, f"log_ge1(2 * {mant[k]!r}): {err:.3f} ulp"
    sp = P.map1("log_ge1", [1.0, math.inf, math.nan])
    assert sp[0] == 0.0 and not np.signbit(sp[0]), "log_ge1(1) must be exactly +0"
    assert np.isnan(sp[1]) and np.isnan(sp[2]), "+inf and NaN in, NaN out (documented)"
    # recorded, not asserted (the comment promises nothing here): the largest and smallest subnormal, and 0
    odd = P.map1("log_pos", [2.0 ** -1023, 5e-324, 0.0])
    fig["log_pos(2^-1023), (5e-324), (0) [recorded]"] = tuple(float(v) for v in odd)
    fig["log max ulp"] = max(worst, err)
    return fig


def check_exp(P):
    """exp_fast: <= 1 ulp on [-700, 700] (the comment's "to 1 ulp"); <= 2 spacings for results below 2^-1000 (the polynomial's
    error, < 0.9 spacing, plus at most 1/2 from ldexp's rounding into the coarser subnormal grid); 0 at and below -750, +inf
    from 710 up, NaN for NaN."""
    rng = np.random.default_rng(21)
    fig = {}
    x = np.concatenate([rng.uniform(-700.0, 700.0, 1 << 18), rng.uniform(-1.0, 1.0, 1 << 14), [-700.0, 700.0, 0.0, -0.0, 5e-324, -5e-324]])
    got = P.map1("exp_fast", x)
    err, k = R.screened_max(got, [x], np.exp, R.mp_exp, R.spacing_np, 1.0)
    fig["exp_fast [-700, 700] ulp"] = err
    assert err <= 1.0, f"exp_fast({x[k]!r}) = {got[k]!r}: {err:.3f} ulp"
    # r at the edges of the reduction interval: x within a few ulp of (k + 1/2) ln 2
    ks = np.arange(-1009, 1009)
    c = (ks + 0.5) * LN2
    xe = np.concatenate([c + j * np.spacing(np.abs(c)) for j in range(-4, 5)])
    xe = xe[np.abs(xe) <= 700.0]
    got = P.map1("exp_fast", xe)
    err, k = R.screened_max(got, [xe], np.exp, R.mp_exp, R.spacing_np, 1.0)
    fig["exp_fast at (k + 1/2) ln 2 ulp"] = err
    assert err <= 1.0, f"exp_fast({xe[k]!r}) = {got[k]!r}: {err:.3f} ulp at a reduction edge"
    # results below 2^-1000, down through the subnormals to where they round to 0
    xs = np.concatenate([rng.uniform(-749.999, -1000 * LN2, 1 << 14), -LN2 * np.arange(1000, 1080), -LN2 * (np.arange(1000, 1080) + 0.5)])
    xs = xs[xs > -750.0]
    got = P.map1("exp_fast", xs)
    err, k = R.screened_max(got, [xs], np.exp, R.mp_exp, R.spacing_np, 2.0)
    fig["exp_fast below 2^-1000 spacings"] = err
    assert err <= 2.0, f"exp_fast({xs[k]!r}) = {got[k]!r}: {err:.3f} spacings"
    lo = P.map1("exp_fast", [-750.0, -750.0000001, -1e3, -1e300, -math.inf])
    assert np.all(lo == 0.0) and not np.any(np.signbit(lo)), f"x <= -750 must give exactly 0: {lo}"
    hi = P.map1("exp_fast", [710.0, 749.0, 750.0, 1e300, math.inf])
    assert np.all(hi == math.inf), f"x >= 710 must give +inf: {hi}"
    assert np.isnan(P.map1("exp_fast", [math.nan])[0])
    return fig


def check_log1pexp(P):
    """log1pexp(x), x <= 0: absolute error <= 4e-16 -- 1 ulp of e^x <= 1 through 1 / (1 + e^x): 1.1e-16; the rounding of 1 + e^x:
    1.1e-16; 1 ulp of a result <= ln 2: 1.1e-16; rounded up.  0 < x <= 700: <= 2 ulp of the result.  x = -inf: 0.
    Beyond x = 709.78 exp_fast overflows and log_ge1(+inf) is NaN: recorded here, not asserted.  The call sites that could
    reach it: hot_star / star_ll_lanes / chi2_system pass (-0.4 ln 10)(s - p), with magnitudes at most B9_MAG_NOFLUX apart from
    -4: |x| < 96; logaddexp passes lo - hi <= 0.  None reaches 709."""
    rng = np.random.default_rng(31)
    fig = {}
    x = -np.concatenate([rng.uniform(0.0, 50.0, 1 << 16), 10.0 ** rng.uniform(-300, np.log10(745.0), 1 << 15), rng.uniform(0.0, 1e-3, 1 << 12),
                         [0.0, 36.0, 36.7, 37.0, 40.0, 745.0, 750.0, 800.0, 1e6, 1e300]])
    got = P.map1("log1pexp", x)
    err, k = R.screened_max(got, [x], lambda v: np.log1p(np.exp(v)), R.mp_log1pexp, R.ones, 4e-16)
    fig["log1pexp x <= 0 abs"] = err
    assert err <= 4e-16, f"log1pexp({x[k]!r}) = {got[k]!r}: off by {err:.3e}"
    assert P.map1("log1pexp", [-math.inf])[0] == 0.0
    xp = np.concatenate([rng.uniform(0.0, 700.0, 1 << 15), 10.0 ** rng.uniform(-300, 0, 1 << 12), [700.0]])
    got = P.map1("log1pexp", xp)
    err, k = R.screened_max(got, [xp], lambda v: np.log1p(np.exp(v)), R.mp_log1pexp, R.spacing_np, 2.0)
    fig["log1pexp 0 < x <= 700 ulp"] = err
    assert err <= 2.0, f"log1pexp({xp[k]!r}) = {got[k]!r}: {err:.3f} ulp"
    big = P.map1("log1pexp", [709.7, 709.79, 710.0, 750.0, math.inf])
    fig["log1pexp(709.7, 709.79, 710, 750, inf) [recorded]"] = tuple(float(v) for v in big)
    return fig


def check_logaddexp(P):
    """logaddexp(a, b) against the mpmath log-sum-exp: |error| <= 4e-16 + 1 ulp(max(a, b)) (log1pexp's bound plus the rounding of
    the final sum; the sum's magnitude is max(a, b)'s to within ln 2)."""
    rng = np.random.default_rng(41)
    base = np.concatenate([rng.uniform(-1e6, 1e6, 200), rng.uniform(-50, 50, 200), 10.0 ** rng.uniform(-300, 6, 100) * rng.choice([-1, 1], 100), [0.0, 1e6, -1e6]])
    a_all, b_all = [], []
    for d in (0.0, 1e-300, -1e-300, 40.0, -40.0, 800.0, -800.0):
        a_all.append(base); b_all.append(base + d)
    a_all.append(base); b_all.append(base + rng.normal(0, 3, base.size))
    a = np.concatenate(a_all); b = np.concatenate(b_all)
    got = P.map2("logaddexp", a, b)
    worst = 0.0
    for ai, bi, g in zip(a, b, got):
        want = R.mp_logaddexp(float(ai), float(bi))
        bound = 4e-16 + math.ulp(max(ai, bi))
        err = float(abs(R.mpf(float(g)) - want))
        assert err <= bound, f"logaddexp({ai!r}, {bi!r}) = {g!r}: off by {err:.3e}, bound {bound:.3e}"
        worst = max(worst, err / bound)
    # either side -inf returns the other bit for bit; both -inf: -inf
    v = np.concatenate([base, [-0.0, 5e-324, math.inf]])
    ninf = np.full(v.size, -math.inf)
    assert same_bits(P.map2("logaddexp", v, ninf), v) and same_bits(P.map2("logaddexp", ninf, v), v)
    assert P.map2("logaddexp", [-math.inf], [-math.inf])[0] == -math.inf
    return {"logaddexp error / bound": worst}


def fdiv_inputs(seed=51):
    rng = np.random.default_rng(seed)
    n = 1 << 15
    den = np.ldexp(1.0 + rng.random(n), rng.integers(-500, 500, n)) * rng.choice([-1.0, 1.0], n)
    quo = np.ldexp(1.0 + rng.random(n), rng.integers(-500, 500, n)) * rng.choice([-1.0, 1.0], n)
    with np.errstate(all="ignore"):
        num = den * quo
    ok = np.isfinite(num) & (np.abs(num) >= 2.0 ** -1000)
    # ... and the interpolation case 0 <= num <= den, ordinary magnitudes
    d2 = 10.0 ** rng.uniform(-12, 3, n)
    n2 = d2 * rng.random(n)
    return np.concatenate([num[ok], n2]), np.concatenate([den[ok], d2])


def check_fdiv(P):
    """fdiv within 1 ulp of the exactly rounded quotient (its comment), |den| and |num / den| in [2^-500, 2^500], both signs; and
    find_bracket's t, which is the same sequence written out: within 1 ulp, in [0, 1] for a query inside its bracket, 0 for
    duplicate nodes."""
    fig = {}
    num, den = fdiv_inputs()
    got = P.map2("fdiv", num, den)
    err, k = R.screened_max(got, [num, den], lambda a, b: a / b, lambda a, b: R.mpf(a) / R.mpf(b), R.spacing_np, 1.0)
    fig["fdiv ulp"] = err
    assert err <= 1.0, f"fdiv({num[k]!r}, {den[k]!r}) = {got[k]!r}: {err:.3f} ulp"
    assert R.quotient_ulp_error(float(got[0]), float(num[0]), float(den[0])) <= 1.0          # (the exact-quotient form of the same statement)
    inside = (num >= 0) & (den > 0) & (num <= den)
    assert np.all((got[inside] >= 0.0) & (got[inside] <= 1.0)), "0 <= num <= den must give a weight in [0, 1]"
    # num == den: is the quotient exactly 1?  (recorded either way)
    d = np.concatenate([den, 10.0 ** np.random.default_rng(52).uniform(-12, 3, 1 << 14)])
    one = P.map2("fdiv", d, d)
    off = np.abs(one - 1.0)
    fig["fdiv(d, d) == 1 for every d"] = bool(np.all(off == 0.0))
    fig["fdiv(d, d): largest |t - 1| in ulp(1)"] = float(off.max() / 2.0 ** -52)
    assert off.max() <= 2.0 ** -52
    # find_bracket's t on a column with spacings over 15 orders of magnitude, queries inside every bracket and AT every node
    rng = np.random.default_rng(53)
    n = 200
    ax = np.cumsum(10.0 ** rng.uniform(-12, 3, n))
    ax[50:53] = ax[50]; ax[-1] = ax[-2]                                        # duplicate nodes (a run's LAST node is the bracket's: d == 0 only at the column's end)
    col = np.full(mass_column_capacity(n), np.nan); col[:n] = ax
    q = np.concatenate([ax[:-1] + (ax[1:] - ax[:-1]) * rng.random(n - 1), ax[:-1] + (ax[1:] - ax[:-1]) * rng.random(n - 1) * 1e-9, ax, [ax[-1] + 1.0]])
    for lds in (False, True):
        lo, t = P.search("find_bracket", col, n, q, lds=lds)
        assert np.array_equal(lo, R.bracket_ref(ax, q))
        a = ax[lo]; dd = ax[lo + 1] - a; nn = q - a                              # (IEEE subtractions: the device's own operands)
        dup = dd == 0.0
        assert np.all(t[dup] == 0.0), "duplicate nodes (d == 0) must give t == 0"
        assert np.any(dup)
        ins = ~dup & (q <= ax[-1])
        assert np.all((t[ins] >= 0.0) & (t[ins] <= 1.0)), "a query inside its bracket must have t in [0, 1]"
        err, k = R.screened_max(t[~dup], [nn[~dup], dd[~dup]], lambda x, y: x / y, lambda x, y: R.mpf(x) / R.mpf(y), R.spacing_np, 1.0)
        fig[f"find_bracket t ulp ({'LDS' if lds else 'global'})"] = err
        assert err <= 1.0, f"find_bracket's t is {err:.3f} ulp from the quotient"
    return fig


# ------------------------------------------------------------------------------------------------------------------
# searches
# ------------------------------------------------------------------------------------------------------------------
SEARCH_LENGTHS = list(range(2, 81)) + [127, 128, 129, 511, 512, 513, 2000]


def search_axes(n, rng):
    strict = np.sort(rng.uniform(-3.0, 7.0, n)) + np.arange(n) * 1e-9
    dup = strict.copy()
    for _ in range(max(1, n // 6)):
        i = int(rng.integers(0, n)); j = min(n, i + int(rng.integers(2, 5)))
        dup[i:j] = dup[i]
    wide = np.cumsum(10.0 ** rng.uniform(-12, 3, n)) - 50.0
    return dict(strict=strict, dup=dup, wide=wide)


def search_queries(ax):
    return np.concatenate([ax, np.nextafter(ax, -np.inf), np.nextafter(ax, np.inf), [ax[0] - 1.0, ax[0] - 1e300, ax[-1] + 1.0, ax[-1] + 1e300, -np.inf, np.inf]])


def check_searches(P, lengths=SEARCH_LENGTHS):
    """bracket, bracket8<false / true>, find_bracket (global and LDS, padding NaN and 1e300) and bracket8_lockstep<2> against
    np.searchsorted: the largest i <= n - 2 with ax[i] <= x (descending: >= x), clamped to 0 -- bit-exact integers."""
    rng = np.random.default_rng(61)
    prev = None
    n_cmp = 0
    nan_rec = {}
    for n in lengths:
        for kind, ax in search_axes(n, rng).items():
            q = search_queries(ax)
            want = R.bracket_ref(ax, q)
            tag = f"n = {n}, {kind} axis"
            b = P.search("bracket", ax, n, q)[0]
            b8 = P.search("bracket8", ax, n, q)[0]
            assert np.array_equal(b, want), f"bracket, {tag}: {q[np.flatnonzero(b != want)[:3]]}"
            assert np.array_equal(b8, want), f"bracket8<false>, {tag}: {q[np.flatnonzero(b8 != want)[:3]]}"
            assert np.array_equal(b8, b)
            dax = ax[::-1].copy()
            d8 = P.search("bracket8_desc", dax, n, q)[0]
            wd = R.bracket_ref(dax, q, desc=True)
            assert np.array_equal(d8, wd), f"bracket8<true>, {tag}: {q[np.flatnonzero(d8 != wd)[:3]]}"
            cap = mass_column_capacity(n)
            res = []
            for pad in (np.nan, 1e300):
                col = np.full(cap, pad); col[:n] = ax
                for lds in (False, True):
                    lo, t = P.search("find_bracket", col, n, q, lds=lds)
                    assert np.array_equal(lo, want), f"find_bracket ({'LDS' if lds else 'global'}, padding {pad}), {tag}: {q[np.flatnonzero(lo != want)[:3]]}"
                    res.append((lo, t))
            for lo, t in res[1:]:                                              # the over-read never decides anything
                assert np.array_equal(lo, res[0][0]) and same_bits(t, res[0][1]), f"find_bracket depends on its padding or address space, {tag}"
            if prev is not None:
                l0, l1 = P.lockstep2(ax, prev, q)
                assert np.array_equal(l0, want) and np.array_equal(l1, R.bracket_ref(prev, q)), f"bracket8_lockstep<2>, {tag}"
            n_cmp += q.size * 8
            if n in (9, 128) and kind == "strict":                             # NaN queries: recorded, not asserted
                col = np.full(cap, np.nan); col[:n] = ax
                nan_rec[n] = (int(P.search("bracket", ax, n, [np.nan])[0][0]), int(P.search("bracket8", ax, n, [np.nan])[0][0]),
                              int(P.search("find_bracket", col, n, [np.nan])[0][0]))
            prev = ax
    return {"search comparisons": n_cmp, "NaN query -> (bracket, bracket8, find_bracket) [recorded]": nan_rec}


# ------------------------------------------------------------------------------------------------------------------
# wave primitives, random numbers
# ------------------------------------------------------------------------------------------------------------------
def wave_inputs(n_waves, seed):
    """magnitudes over 1e-300 .. 1e300 with heavy cancellation: the order of the additions decides the bits"""
    rng = np.random.default_rng(seed)
    v = 10.0 ** rng.uniform(-300, 300, (n_waves, 64)) * rng.choice([-1.0, 1.0], (n_waves, 64))
    mid = 10.0 ** rng.uniform(-3, 3, (n_waves, 64)) * rng.choice([-1.0, 1.0], (n_waves, 64))
    v[::2] = mid[::2]
    for w in range(0, n_waves, 3):                                              # cancelling pairs at every tree distance
        o = (32, 16, 8, 4, 2, 1)[(w // 3) % 6]
        l = rng.integers(0, 64 - o, 8)
        v[w, l + o] = -v[w, l] * (1.0 + rng.choice([0.0, 2.0 ** -52, -2.0 ** -53], 8))
    return v


def check_lane_down(P):
    rng = np.random.default_rng(71)
    v = rng.standard_normal((8, 64)); vi = rng.integers(-2 ** 31, 2 ** 31 - 1, (8, 64)).astype(np.int32)
    for o in (1, 2, 4, 8, 16, 32):
        lanes = np.flatnonzero(R.lane_down_lanes(o))
        assert lanes.size and np.all(lanes + o < 64)
        assert same_bits(P.lane_down(o, v)[:, lanes], v[:, lanes + o]), f"lane_down<{o}>(double)"
        assert np.array_equal(P.lane_down(o, vi)[:, lanes], vi[:, lanes + o]), f"lane_down<{o}>(int)"
    return {}


def check_wave_sum(P):
    """wave_sum: lane 0 = the stated tree, bit for bit; IEEE propagation of inf / -0 / NaN; and a sanity check against math.fsum
    (64 positive terms: the tree's 6 levels of rounding are within 64 ulp -- in fact within 3)."""
    v = wave_inputs(96, 72)
    got = P.wave1("wave_sum", v)[:, 0]
    want = R.tree_sum(v)[:, 0]
    assert same_bits(got, want), f"wave_sum is not the stated tree in waves {np.flatnonzero(bits(got) != bits(want))[:5]}"
    assert len(np.unique(bits(want))) > 48
    sp = np.zeros((6, 64))
    sp[0, 5] = np.inf; sp[1, 5] = np.inf; sp[1, 40] = -np.inf; sp[2, :] = -0.0; sp[3, 63] = np.nan; sp[4, :] = -0.0; sp[4, 17] = 0.0; sp[5, 9] = -np.inf
    got = P.wave1("wave_sum", sp)[:, 0]
    want = R.tree_sum(sp)[:, 0]
    assert got[0] == np.inf and np.isnan(got[1]) and np.isnan(got[3]) and got[5] == -np.inf
    assert got[2] == 0.0 and np.signbit(got[2]) and got[4] == 0.0 and not np.signbit(got[4])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and same_bits(got[~np.isnan(got)], want[~np.isnan(want)])
    pos = np.random.default_rng(73).uniform(0.5, 2.0, (32, 64))
    got = P.wave1("wave_sum", pos)[:, 0]
    worst = max(abs(g - math.fsum(r)) / math.ulp(math.fsum(r)) for g, r in zip(got, pos))
    assert worst <= 64
    return {"wave_sum vs fsum ulp": worst}


def check_wave_sum7(P):
    v = wave_inputs(7 * 24, 74).reshape(24, 7, 64)
    one = np.zeros((7, 7, 64))
    for k in range(7):                                                          # only one vector non-zero: a mixed-up row shows
        one[k, k] = wave_inputs(1, 75 + k)[0]
    x = np.concatenate([v, one])
    got = P.wave_sum7(x)
    want = P.wave1("wave_sum", x.reshape(-1, 64))[:, 0].reshape(-1, 7)
    tree = R.tree_sum(x)[..., 0]
    assert same_bits(want, tree)
    for l in range(64):
        assert same_bits(got[:, :, l], want), f"wave_sum7: S[n] in lane {l} is not wave_sum(a[n])"
    return {}


def check_wave_max_bcast(P):
    rng = np.random.default_rng(76)
    v = np.concatenate([rng.standard_normal((8, 64)) * 1e3, np.full((1, 64), -np.inf), np.zeros((1, 64)), -np.zeros((1, 64))])
    single = np.full((64, 64), -np.inf); single[np.arange(64), np.arange(64)] = rng.standard_normal(64)
    pz = np.full((2, 64), -0.0); pz[0, 33] = 0.0; pz[1, 0] = 0.0
    v = np.concatenate([v, single, pz])
    got = P.wave1("wave_max_all", v)
    assert np.array_equal(got, np.repeat(v.max(axis=1)[:, None], 64, axis=1)), "wave_max_all is not the maximum in every lane"      # (by value: +0 == -0)
    b = wave_inputs(16, 77); b[3, 0] = -0.0; b[4, 0] = np.inf; b[5, 0] = 5e-324
    for op in ("wave_bcast0", "wave_uniform"):
        assert same_bits(P.wave1(op, b), np.repeat(b[:, :1], 64, axis=1)), op
    nanw = np.zeros((1, 64)); nanw[0, 0] = np.nan
    assert np.all(np.isnan(P.wave1("wave_bcast0", nanw))) and np.all(np.isnan(P.wave1("wave_uniform", nanw)))
    return {}


PHILOX_KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
              ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
              ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def check_rng(P):
    """philox4x32 on the device against the Random123 known-answer vectors (tests/test_mcmc.py's) and the numpy twin; u01 at
    its corners and on 2^16 random pairs: strictly inside (0, 1), the twin's bits, a finite log."""
    from base_amd import mcmc
    got = P.philox([k[0] for k in PHILOX_KAT], [k[1] for k in PHILOX_KAT])
    assert [tuple(int(x) for x in r) for r in got] == [k[2] for k in PHILOX_KAT]
    rng = np.random.default_rng(81)
    ctr = rng.integers(0, 2 ** 32, (4096, 4), dtype=np.uint64).astype(np.uint32)
    key = np.repeat(rng.integers(0, 2 ** 32, (1, 2), dtype=np.uint64).astype(np.uint32), 4096, axis=0)
    twin = np.stack(mcmc.philox4x32(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[0, 0], key[0, 1]), axis=1)
    assert np.array_equal(P.philox(ctr, key), twin)
    hi = np.concatenate([[0, 0xffffffff, 0, 0xffffffff], rng.integers(0, 2 ** 32, 1 << 16, dtype=np.uint64)]).astype(np.uint32)
    lo = np.concatenate([[0, 0xffffffff, 0xffffffff, 0], rng.integers(0, 2 ** 32, 1 << 16, dtype=np.uint64)]).astype(np.uint32)
    u, lg = P.u01(hi, lo)
    assert np.all((u > 0.0) & (u < 1.0)) and same_bits(u, mcmc._u01(hi, lo)) and np.all(np.isfinite(lg)) and np.all(lg < 0.0)
    # (0xffffffff, 0xffffffff): x + 0.5 = 2^53 - 0.5 is a tie that rounds to 2^53 -- u01 returned exactly 1 there until it was held
    # at the largest double below 1 (found by this check; gumbel()'s -log(-log 1) is +inf)
    assert u[0] == 2.0 ** -54 and u[1] == 1.0 - 2.0 ** -53
    return {}


# ------------------------------------------------------------------------------------------------------------------
# accumulators
# ------------------------------------------------------------------------------------------------------------------
def mix_cases(k, seed):
    """[(name, ea [k][64], l [k][64])]"""
    rng = np.random.default_rng(seed)
    sh = (k, 64)
    cases = []
    ea = 10.0 ** rng.uniform(-300, 300, sh); l = rng.uniform(-700, 600, sh)
    cases.append(("A over 1e-300 .. 1e300, l to 600", ea, l))
    cases.append(("l = -1e14: u = A", 10.0 ** rng.uniform(-30, 30, sh), np.full(sh, -1e14)))
    l = np.where(rng.random(sh) < 0.5, rng.uniform(600.0, 601.0, sh), np.nextafter(600.0, 700.0)); ea = np.where(rng.random(sh) < 0.5, 0.0, 10.0 ** rng.uniform(-5, 5, sh))
    cases.append(("l just above 600 / A = 0: additive", ea, l))
    cases.append(("all additive, A = 0", np.zeros(sh), rng.uniform(-50.0, 0.0, sh)))              # (one sign: no partial sum above |want|)
    cases.append(("tiny factors: the plain product underflows", np.full(sh, 1e-300), np.full(sh, -1e14)))
    cases.append(("huge factors: the plain product overflows", np.full(sh, 1e300), rng.uniform(500, 600, sh)))
    cases.append(("ordinary stars", 10.0 ** rng.uniform(-12, -2, sh), rng.uniform(-60, 5, sh)))
    return cases


def mix_want(ea, l):
    tot = R.mpf(0)
    for a, x in zip(ea.ravel(), l.ravel()):
        tot += R.mpf(float(x)) if (a == 0.0 or x > 600.0) else R.mp_mix_term(a, x)
    return tot


def check_mix(P, ks=(1, 7, 100)):
    """mix_add then mix_wave_total against mpmath sum_i log(A_i + e^{l_i}) over 64 lanes x k stars:
    |got - want| <= 64 k 4 2^-53 + 4 ulp(|want|) -- per factor one exp_fast at <= 1 ulp, one add and one multiply at 1/2 ulp each
    (relative errors of a factor are absolute errors of its logarithm), then the final log_ge1 and the additive sum.
    A star with A = 0 or l > 600 contributes exactly l (the same term in the reference)."""
    worst = 0.0
    for k in ks:
        cases = mix_cases(k, 90 + k)
        if k == 100:
            cases = cases[:1] + cases[4:]
        ea = np.stack([c[1] for c in cases]); l = np.stack([c[2] for c in cases])
        got = P.mix(ea, l)
        for (name, a, x), g in zip(cases, got):
            want = mix_want(a, x)
            bound = 64 * k * 4 * 2.0 ** -53 + 4 * R.spacing(want)
            err = float(abs(R.mpf(float(g)) - want))
            assert err <= bound, f"mix, k = {k}, {name}: {g!r} is {err:.3e} from {float(want)!r}, bound {bound:.3e}"
            worst = max(worst, err / bound)
    fig = {"mix error / bound": worst}
    # an additive-only lane contributes l EXACTLY: one star per lane, every other factor 1
    l1 = np.random.default_rng(91).uniform(600.0, 1e6, (1, 1, 64)); l1[0, 0, 1:] = 0.0
    assert P.mix(np.zeros((1, 1, 64)), l1)[0] == l1[0, 0, 0]
    # mix_value, the per-star diagnostic: the same quantity per star at 2 ulp
    rng = np.random.default_rng(92)
    ea = np.concatenate([10.0 ** rng.uniform(-300, 300, 3000), np.zeros(50), 10.0 ** rng.uniform(-5, 5, 50)])
    l = np.concatenate([rng.uniform(-700, 600, 3000), rng.uniform(-1e3, 1e3, 50), rng.uniform(600.0001, 700, 50)])
    got = P.map2("mix_value", ea, l)
    w = w_small = 0.0
    for a, x, g in zip(ea, l, got):
        if a == 0.0 or x > 600.0:
            assert g == x
            continue
        want = R.mp_mix_term(a, x)
        e = R.ulp_error(float(g), want)
        if abs(want) >= 1.0:
            assert e <= 2.0, f"mix_value({a!r}, {x!r}) = {g!r}: {e:.3f} ulp"
            w = max(w, e)
        else:       # a value inside (-1, 1): 2 ulp OF 1 -- an exp followed by a log carries e^l's rounding as an ABSOLUTE error of the
            #         logarithm (1.1e-16 / u), which is any number of ulp of a value near 0 (measured: 4 ulp at -0.11)
            ea_ = float(abs(R.mpf(float(g)) - want))
            assert ea_ <= 2 * 2.0 ** -52, f"mix_value({a!r}, {x!r}) = {g!r}: off by {ea_:.3e}"
            w_small = max(w_small, e)
    fig["mix_value ulp (|value| >= 1)"] = w
    fig["mix_value ulp (|value| < 1) [recorded; 2 ulp of 1 asserted]"] = w_small
    return fig


def mix_subnormal_record(P):
    """Subnormal A (1e-310, 5e-324) with l = -inf: mant * u is a subnormal product, and frexp_mant / frexp_exp of a subnormal are
    where an error could enter.  Recorded (error and bound); b9_load_stars cannot produce such an A -- see the caller."""
    out = {}
    for a in (1e-310, 5e-324):
        ea = np.full((1, 3, 64), a); l = np.full((1, 3, 64), -math.inf)
        got = float(P.mix(ea, l)[0])
        want = 192 * R.mp_log(a)
        out[a] = (got, float(abs(R.mpf(got) - want)) if math.isfinite(got) else math.inf, 64 * 3 * 4 * 2.0 ** -53 + 4 * R.spacing(want))
    return out


def lse_sequences(seed=95):
    rng = np.random.default_rng(seed)
    seqs = []
    for span in (1.0, 40.0, 800.0, 1e6):
        for n in (1, 2, 37, 256):
            t = rng.uniform(-span, 0.0, n) + rng.uniform(-1e3, 1e3)
            t[rng.random(n) < 0.15] = -np.inf                                   # -inf terms in between
            if n > 1:
                t[0] = rng.uniform(-span, 0.0)
            seqs.append(t)
    return seqs


def check_lse(P):
    """The online log-sum-exp (lse_add) and its merge (lse_merge) against the mpmath log-sum-exp of the same terms, fed ascending,
    descending and shuffled, and split over 2 .. 64 partial accumulators merged in a tree:
    |mx + log(sm) - want| <= n 4 2^-53 + 2 ulp(|want|) -- per term one exp_fast at 1 ulp, one multiply-add when the maximum moves,
    one add: relative errors of sm, absolute ones of its logarithm; then the rounding of the log and of the sum.
    An accumulator that has only seen -inf merges as the identity."""
    worst = 0.0
    for t in lse_sequences():
        want = R.mp_logsumexp(t)
        n = t.size
        rng = np.random.default_rng(n)
        orders = [np.sort(t), np.sort(t)[::-1], rng.permutation(t)]
        for parts in (1, 2, 3, 8, 64):
            mx, sm = P.lse(np.stack(orders), parts)
            for m, s in zip(mx, sm):
                if want == R.mpf("-inf"):
                    assert m == -math.inf and s == 0.0
                    continue
                got = R.mpf(float(m)) + R.mp_log(float(s))
                bound = n * 4 * 2.0 ** -53 + 2 * R.spacing(want)
                err = float(abs(got - want))
                assert err <= bound, f"lse of {n} terms over {parts} accumulators: off by {err:.3e}, bound {bound:.3e}"
                worst = max(worst, err / bound)
    # only -inf on one side: the identity, bit for bit (64 accumulators of which 63 saw nothing but -inf)
    t = np.full((1, 64), -math.inf); t[0, 40] = 1.2345
    mx, sm = P.lse(t, 64)
    assert mx[0] == 1.2345 and sm[0] == 1.0
    mx, sm = P.lse(np.full((1, 64), -math.inf), 64)
    assert mx[0] == -math.inf and sm[0] == 0.0
    return {"lse error / bound": worst}


# ------------------------------------------------------------------------------------------------------------------
# box pruning
# ------------------------------------------------------------------------------------------------------------------
BOX_FAMILIES = ("far", "few_sigma", "micro", "zero_width", "contains", "empty", "noflux", "near_zero_obs", "graze")
SLACK_FACTOR = 2100.0 * 2.0 ** -44
XCUT = 80.0                  # 2 x B9_MARG_CUT: 40 e-folds, in the units of X = nb + chi^2


def box_inputs(nfp, n_box=1024, seed=100):
    """n_box boxes x 64 stars (a wave tests one box).  Family of box b: BOX_FAMILIES[b % 9].  "graze": every filter of the box
    at a relative distance 1e-5 .. 1e-2.5 of a star's magnitude -- around 2^-12, where the fp32 rounding of the distance
    (2^-22 |so|) is largest against what B9_BOX_INV takes off the squared distance: the pairs that come closest to the slack."""
    rng = np.random.default_rng(seed + nfp)
    fam = np.arange(n_box) % len(BOX_FAMILIES)
    sh = (n_box, 64, nfp)
    ref = rng.uniform(-5.0, 30.0, (n_box, 1, nfp))                              # the wave's region of the magnitude space
    ref[fam == 7] = rng.uniform(-0.01, 0.01, (int((fam == 7).sum()), 1, nfp))
    obs = ref + rng.normal(0.0, 0.3, sh) * (fam != 7)[:, None, None] + rng.uniform(-0.01, 0.01, sh) * (fam == 7)[:, None, None]
    sigma = 10.0 ** rng.uniform(-4, 1, sh)
    sw = 1.0 / sigma
    sw[rng.random(sh) < 0.05] = 0.0                                             # unused filters (w = 0)
    so = sw * obs
    c = ref[:, 0, :]
    sgn = rng.choice([-1.0, 1.0], (n_box, nfp))
    width = 10.0 ** rng.uniform(-3, 0.5, (n_box, nfp))
    lo = np.empty((n_box, nfp)); hi = np.empty((n_box, nfp))
    for b in range(n_box):
        f = BOX_FAMILIES[fam[b]]
        if f == "far":
            d = sgn[b] * 10.0 ** rng.uniform(-1.5, 1.3, nfp); lo[b] = c[b] + d; hi[b] = lo[b] + width[b]
        elif f == "few_sigma":
            d = sgn[b] * rng.uniform(0.5, 8.0, nfp) * 10.0 ** rng.uniform(-4, 0, nfp); lo[b] = c[b] + d; hi[b] = lo[b] + width[b] * 0.01
        elif f == "micro":
            s = obs[b, int(rng.integers(0, 64))]; lo[b] = s + 1e-6; hi[b] = lo[b] + width[b]
        elif f == "zero_width":
            lo[b] = c[b] + sgn[b] * 10.0 ** rng.uniform(-6, 1, nfp); hi[b] = lo[b]
        elif f == "contains":
            lo[b] = obs[b].min(axis=0) - width[b]; hi[b] = obs[b].max(axis=0) + width[b]
        elif f == "empty":
            lo[b] = c[b] + 1.0; hi[b] = c[b] - 1.0
        elif f == "graze":
            s = obs[b, int(rng.integers(0, 64))]; lo[b] = s * (1.0 + sgn[b, 0] * 10.0 ** rng.uniform(-5, -2.5)); hi[b] = lo[b]
        elif f == "noflux":
            lo[b] = np.where(rng.random(nfp) < 0.5, NOFLUX, c[b] + 0.5); hi[b] = NOFLUX
        else:
            lo[b] = sgn[b] * 10.0 ** rng.uniform(-6, -1, nfp); hi[b] = lo[b] + width[b] * 1e-3
    huge = np.zeros(n_box, dtype=bool); huge[5::64] = True                       # stars with sum so^2 >= 1e30: the slack is +inf
    so[huge, ::7, 0] = 1e15 * 1.0001
    nbm = rng.uniform(0.0, 30.0, n_box); nbm[fam == 0] = 0.0
    return dict(fam=fam, so=so, sw=sw, lo=lo, hi=hi, nbm=nbm, xcut=np.full(n_box, XCUT))


def check_box(P, nfp):
    """The box pruning as a property, 2^16 (star, box) pairs per filter width:
      1. f32_below(x) <= x <= f32_above(x) for every stored bound; an empty box is stored as [0, 0];
      2. box_bound64 <= lb (1 + 2^-50), lb the exact bound from the double inputs;
      3. box_bound32 (which includes B9_BOX_INV) <= lb + slack, slack as box_stage returned it and no larger than the stated
         2100 x 2^-44 sum so^2 -- the code's own claim, for EVERY pair, no tolerance;
      4. sum so^2 >= 1e30: the slack is +inf and the box passes;
      5. box_pass<true> wherever box_pass<false>, and both are the ballot of the per-lane tests their comments state;
      6. on the far family the fp32 test excludes >= 99 % of what the fp64 test excludes at 40 e-folds."""
    inp = box_inputs(nfp)
    so, sw, lo, hi, fam = inp["so"], inp["sw"], inp["lo"], inp["hi"], inp["fam"]
    box, box_f = P.box_store(lo, hi)
    empty = (lo > hi)
    assert np.all(box[:, 0][empty] == 0.0) and np.all(box[:, 1][empty] == 0.0) and np.all(box_f[:, 0][empty] == 0.0) and np.all(box_f[:, 1][empty] == 0.0)
    assert same_bits(box[:, 0][~empty], lo[~empty]) and same_bits(box[:, 1][~empty], hi[~empty])
    bf = box_f.astype(np.float64)
    assert np.all(bf[:, 0] <= box[:, 0]), f"f32_below(x) > x at x = {box[:, 0][bf[:, 0] > box[:, 0]][:3]}"
    assert np.all(bf[:, 1] >= box[:, 1]), f"f32_above(x) < x at x = {box[:, 1][bf[:, 1] < box[:, 1]][:3]}"
    assert np.all(np.abs(bf - box) <= np.abs(box) * 2.0 ** -21 + 1e-29), "the float box is looser than the comment says (6e-6 mag at 25)"
    r = P.box_bound(so, sw, box, box_f, inp["nbm"], inp["xcut"])
    lb64, lb32, slack = r["lb64"], r["lb32"], r["slack"]
    blo = np.repeat(box[:, None, 0, :], 64, axis=1); bhi = np.repeat(box[:, None, 1, :], 64, axis=1)
    s2 = (so.astype(R.LD) ** 2).sum(axis=-1).astype(np.float64)
    huge = s2 >= 1e30
    assert huge.any() and np.all(slack[huge] == np.inf) and np.all(r["pass32"][huge.any(axis=1)] == 1)
    fin = ~huge
    # (the slack IS the stated 2100 x 2^-44 sum so^2, both ways: a larger one would make 3. vacuous, a smaller one is not what the
    #  proof in the comment covers -- on these families the outward rounding of the box alone keeps box_bound32 below lb)
    assert np.all(np.isfinite(slack[fin])) and np.all(np.abs(slack[fin] - SLACK_FACTOR * s2[fin]) <= SLACK_FACTOR * s2[fin] * 1e-12), "the slack is not the stated 2100 x 2^-44 sum so^2"
    with np.errstate(all="ignore"):
        lb = R.box_lb_screen(so, sw, blo, bhi)
    lbd = lb.astype(np.float64)
    idx = np.argwhere(fin)
    # 2. fp64
    close64 = np.argwhere(fin & (lb64.astype(R.LD) > lb * (1 + R.LD(2.0) ** -51)))
    # 3. fp32: what the screen puts within a quarter of the slack of the bound is decided exactly
    margin = (lb32.astype(R.LD) - lb).astype(np.float64)
    close32 = np.argwhere(fin & (margin > 0.25 * slack))
    rng = np.random.default_rng(7)
    sample = idx[rng.choice(len(idx), size=min(len(idx), 400), replace=False)]
    worst_frac = float(np.max(np.where(fin & (slack > 0), margin / np.where(slack > 0, slack, 1.0), -np.inf)))
    n_exact = 0
    for b, l in np.concatenate([close64, close32, sample]):
        ex = R.box_lb_exact(so[b, l], sw[b, l], box[b, 0], box[b, 1])
        F = R.Fraction
        assert abs(F(float(lbd[b, l])) - ex) <= ex * F(1, 2 ** 52) + F(1, 10 ** 300), "the long-double screen of the exact bound is off"
        assert F(float(lb64[b, l])) <= ex * (1 + F(1, 2 ** 50)), f"box_bound64 = {lb64[b, l]!r} exceeds the exact bound {float(ex)!r} (nfp {nfp}, box {b}, lane {l}, family {BOX_FAMILIES[fam[b]]})"
        assert F(float(lb32[b, l])) <= ex + F(float(slack[b, l])), (
            f"box_bound32 = {lb32[b, l]!r} > lb + slack = {float(ex)!r} + {slack[b, l]!r} (nfp {nfp}, box {b}, lane {l}, family {BOX_FAMILIES[fam[b]]})")
        n_exact += 1
    # 5. the ballots, from the per-lane quantities (IEEE additions: exact restatements of the two comparisons)
    nbm = inp["nbm"][:, None]; xc = inp["xcut"][:, None]
    lane64 = lb64 + nbm < xc
    lane32 = lb32 + nbm <= xc + slack
    assert np.array_equal(r["pass64"] != 0, lane64.any(axis=1)), "box_pass<false> is not the ballot of lb64 + nbm < xcut"
    assert np.array_equal(r["pass32"] != 0, lane32.any(axis=1)), "box_pass<true> is not the ballot of lb32 + nbm <= xcut + slack"
    assert np.all(lane32[lane64]), "the fp32 test drops a box the fp64 test keeps"
    assert np.all((r["pass32"] != 0)[r["pass64"] != 0])
    # 6. usefulness on the far family
    far = (fam == 0)[:, None] & fin
    ex64n = far & ~lane64
    ratio = float((ex64n & ~lane32).sum() / max(1, ex64n.sum()))
    assert ex64n.sum() > 1000
    assert ratio >= 0.99, f"the fp32 bound excludes only {ratio:.4f} of what the fp64 bound excludes (nfp {nfp})"
    return {"nfp": nfp, "largest (box_bound32 - lb) / slack": worst_frac, "fp32 / fp64 exclusion ratio (far family)": ratio,
            "largest box_bound64 / lb - 1": float(np.max(np.where(fin & (lbd > 0), lb64 / np.where(lbd > 0, lbd, 1.0) - 1.0, -1.0))),
            "pairs decided exactly": n_exact}
