"""Plain, slow, high-precision references for the device primitives (tests/prims_check.py uses them): mpmath at 120 bits
for the transcendentals, fractions.Fraction for exact quotients and exact box bounds, np.searchsorted for the brackets and a
numpy restatement of the wave reduction tree.

Large arrays are SCREENED with numpy's extended precision (x87 long double, 64-bit mantissa) and every point the screen
puts near the bound is measured again with mpmath, which alone decides; the screen's own error is measured against mpmath
on a sample of the same points in the same call (screened_max).  A platform without an extended long double measures
every point with mpmath."""
import math
from fractions import Fraction

import mpmath
import numpy as np

mpmath.mp.prec = 120
mpf = mpmath.mpf
LD = np.longdouble
HAVE_LD = np.finfo(LD).nmant >= 63


def spacing(want) -> float:
    """Spacing of the doubles at the correctly rounded value of `want` (mpf or float); 2^-1074 for subnormal results."""
    r = abs(float(want))
    if r == 0.0 or not math.isfinite(r):
        return 2.0 ** -1074
    return math.ulp(r)


def ulp_error(got: float, want_mp) -> float:
    """|got - want| in units of the spacing of doubles at the correctly rounded `want`."""
    return float(abs(mpf(got) - want_mp) / mpf(spacing(want_mp)))


def spacing_np(want) -> np.ndarray:
    r = np.abs(np.asarray(want).astype(np.float64))
    return np.maximum(np.spacing(r), 2.0 ** -1074)


def screened_max(got, args, fn_ld, fn_mp, unit, bound, sample=1500, seed=1):
    """max over the points of |got - f(args)| / unit(f(args)) (unit: spacing_np for ulp, or ones for absolute error).
    fn_ld(*arrays of longdouble) screens; fn_mp(*floats) -> mpf decides every point the screen puts above bound / 2 and a
    random sample, on which the screen itself must agree with mpmath to bound / 64.  -> (max, index of the max)"""
    got = np.asarray(got, dtype=np.float64)
    args = [np.asarray(a, dtype=np.float64) for a in args]
    n = got.size
    if HAVE_LD:
        with np.errstate(all="ignore"):
            want = fn_ld(*[a.astype(LD) for a in args])
            err = np.abs(got.astype(LD) - want) / unit(want).astype(LD)
        err = np.where(np.isfinite(err), err, np.inf).astype(np.float64)          # (a non-finite result is measured by mpmath)
        rng = np.random.default_rng(seed)
        check = np.union1d(np.flatnonzero(err > bound / 2), rng.choice(n, size=min(n, sample), replace=False))
    else:
        err = np.zeros(n); check = np.arange(n)
    check = check[np.argsort(-err[check], kind="stable")]                          # the screen's worst first: a failure is confirmed at once
    for i in check:
        want_mp = fn_mp(*[float(a[i]) for a in args])
        u = float(unit(np.array([float(want_mp)]))[0])
        e = float(abs(mpf(float(got[i])) - want_mp) / u) if math.isfinite(got[i]) else math.inf
        if HAVE_LD and math.isfinite(err[i]):
            assert abs(e - err[i]) <= bound / 64, f"the long-double screen is off at point {i}: {err[i]} against mpmath's {e}"
        err[i] = e
        if e > bound:
            return e, int(i)
    k = int(np.argmax(err))
    return float(err[k]), k


def ones(want):
    return np.ones(np.shape(want))


def mp_log(x):
    return mpmath.log(mpf(x))


def mp_exp(x):
    return mpmath.exp(mpf(x))


def mp_log1pexp(x):
    return mpmath.log1p(mpmath.exp(mpf(x)))


def mp_logaddexp(a, b):
    a, b = mpf(a), mpf(b)
    hi = max(a, b)
    return hi + mpmath.log(mpmath.exp(a - hi) + mpmath.exp(b - hi))


def mp_logsumexp(terms):
    t = [mpf(float(x)) for x in terms if x != -math.inf]
    if not t:
        return mpf("-inf")
    hi = max(t)
    return hi + mpmath.log(mpmath.fsum(mpmath.exp(x - hi) for x in t))


def mp_mix_term(ea, l):
    """log(A + e^l)"""
    return mpmath.log(mpf(float(ea)) + mpmath.exp(mpf(float(l))))


def exact_quotient(num: float, den: float) -> Fraction:
    return Fraction(num) / Fraction(den)


def quotient_ulp_error(got: float, num: float, den: float) -> float:
    q = exact_quotient(num, den)
    return float(abs(Fraction(got) - q) / Fraction(spacing(float(q))))


def bracket_ref(ax, x, desc=False):
    """largest i <= n - 2 with ax[i] <= x (desc: >= x), clamped to 0"""
    ax = np.asarray(ax, dtype=np.float64); x = np.asarray(x, dtype=np.float64)
    i = np.searchsorted(-ax, -x, side="right") - 1 if desc else np.searchsorted(ax, x, side="right") - 1
    return np.clip(i, 0, len(ax) - 2).astype(np.int32)


def tree_sum(v):
    """The stated tree on [..., 64]: v[l] += v[l + 32], then + 16, ... + 1, for the lanes whose partner exists, all lanes of a
    level at once.  Lane 0 holds the wave's sum."""
    v = np.array(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            nv = v.copy()
            nv[..., :64 - o] = v[..., :64 - o] + v[..., o:]
            v = nv
    return v


def lane_down_lanes(o):
    """the lanes in which lane_down<O> is specified"""
    l = np.arange(64)
    return (l % 16) + o < 16 if o < 16 else ((l // 16) % 2 == 0 if o == 16 else l < 32)


def box_lb_exact(so, sw, lo, hi) -> Fraction:
    """sum_f max(sw lo - so, so - sw hi, 0)^2 from the double inputs, exactly"""
    tot = Fraction(0)
    for o, w, a, b in zip(so, sw, lo, hi):
        o, w = Fraction(float(o)), Fraction(float(w))
        m = max(w * Fraction(float(a)) - o, o - w * Fraction(float(b)), Fraction(0))
        tot += m * m
    return tot


def _two_prod(a, b):
    """a * b = p + e exactly (Veltkamp / Dekker; no fma in numpy), for magnitudes far from over- and underflow"""
    p = a * b
    ca = 134217729.0 * a; ah = ca - (ca - a); al = a - ah
    cb = 134217729.0 * b; bh = cb - (cb - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def box_lb_screen(so, sw, lo, hi):
    """the same over [..., nfp], to ~2^-60 relative: the products exactly as (p, e) pairs, the differences and the sum in long
    double (sw lo - so cancels to 1e-7 of its operands when a box is 1e-6 mag from the star: a plain long-double product
    would leave the screen LESS accurate than the fp64 bound it is to judge).  The callers re-measure what is close."""
    so, sw, lo, hi = (np.asarray(a, dtype=np.float64) for a in (so, sw, lo, hi))
    p1, e1 = _two_prod(sw, lo)
    p2, e2 = _two_prod(sw, hi)
    a = (p1.astype(LD) - so.astype(LD)) + e1.astype(LD)
    b = (so.astype(LD) - p2.astype(LD)) - e2.astype(LD)
    m = np.maximum(np.maximum(a, b), 0)
    return (m * m).sum(axis=-1)
