"""The forward model of DESIGN.md section 2 for ONE stellar system, stated once over an arithmetic `B` and evaluated

  * in mpmath at 50 digits with a running first-order error bound (`RefArith`): the reference and its error budget;
  * in correctly rounded fp64 (`F64Arith`): an emulation of what the oracle and the device compute, which can carry one
    MUTANT at a time (tests/test_wd_seams_host.py shows that the checker rejects each of them).

The inputs are the pack's and the row's fp64 numbers, taken exactly.  CPU only; nothing here knows about the device.

Error budget.  Every value of the reference is a pair (v, e): v the exact value of the stated formula, e a first-order bound on
|fp64 result - v| under these rules: u = 2^-53 per fp64 operation (one rounding: +, -, *, fma); a division 3u (fdiv is within
1 ulp of the correctly rounded quotient, the bound tests/prims_check.py :: check_fdiv pins: 2u + u; a plain `/` is inside it);
exp10 and log10 3 ulp = 6u (the OpenCL full-profile double requirement the device library targets); log1pexp(x) 4e-16 absolute
for x <= 0 and 2 ulp above (prims_check.check_log1pexp).  The host-side star constants (the mass prior, the Gaussian constants)
and the closing mixtures (field star, two populations, the node sum of the marginalised mode) are NOT followed operation by
operation: they take a flat allowance of 16u (64u for the node sum) on the magnitude of their result and constants (each term's own
budget enters a log-sum-exp with its share of the sum), several times
what their dozen operations and 1-ulp library calls can lose, and orders below the chi^2 term they stand next to.  Input errors are
carried through each operation with the operation's own partial derivatives at the reference's values, so the bound follows
the chain cell by cell (it is piecewise linear inside a cell).  Decisions (branches, bracket indices) are taken on the exact
values; a case whose decision the fp64 rounding could turn is not a case of the catalogue (tests/wd_seams.py keeps the
deciding quantities exact or at a distance).  Nothing here is derived from what a device returns.

kappa is the amplification of the one ill-conditioned step, log10(10^logAge - 10^prec): 10^logAge / (10^logAge - 10^prec).
"""
import bisect
import math
from fractions import Fraction

import mpmath
import numpy as np

from base_amd import abi

M = mpmath.MPContext()
M.dps = 50
U = M.mpf(2) ** -53
LOG_G_PLUS_LOG_MSUN = 26.12302173752
MF_MU, MF_SIGMA = -1.02, 0.67729
NOFLUX = abi.MAG_NOFLUX

# branch tags of a component
DNE, BELOW_FIRST, MSRGB, WD_NOMODELS, WD_NOTYET, WD, NSBH = "DNE", "below_first_mass", "MS/RGB", "WD_no_models", "WD_not_yet_dead", "WD", "NS/BH"


class V:
    """(value, first-order bound on the fp64 result's distance from it)"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0):
        self.v, self.e = M.mpf(v), M.mpf(e)


class RefArith:
    """50-digit values with the running error bound of the module's docstring."""
    name = "ref"

    def c(self, x):                       # an input: exact
        return V(x)

    def val(self, a):
        return a.v

    def _r(self, v, e, k=1):              # k roundings of size u on the result
        return V(v, e + k * U * abs(v))

    def add(self, a, b): return self._r(a.v + b.v, a.e + b.e)
    def sub(self, a, b): return self._r(a.v - b.v, a.e + b.e)
    def mul(self, a, b): return self._r(a.v * b.v, abs(a.v) * b.e + abs(b.v) * a.e)
    def neg(self, a): return V(-a.v, a.e)

    def div(self, a, b):
        q = a.v / b.v
        return self._r(q, (a.e + abs(q) * b.e) / abs(b.v), 3)

    def fma(self, t, d, a): return self._r(t.v * d.v + a.v, abs(t.v) * d.e + abs(d.v) * t.e + a.e)

    def log10(self, a):
        if not a.v > 0:
            return V(M.nan, M.inf)
        return self._r(M.log10(a.v), a.e / (a.v * M.ln(10)), 6)

    def exp10(self, a):
        v = M.power(10, a.v)
        return self._r(v, v * M.ln(10) * a.e, 6)

    def log(self, a):
        return self._r(M.ln(a.v), a.e / a.v, 2)

    def log1pexp(self, x):
        ex = M.exp(x.v)
        v = M.log1p(ex)
        own = M.mpf("4e-16") if x.v <= 0 else 4 * U * abs(v)
        return V(v, ex / (1 + ex) * x.e + own)

    def isfinite(self, a):
        return M.isfinite(a.v)


def _fma(t, d, a):
    if not (math.isfinite(t) and math.isfinite(d) and math.isfinite(a)):
        return t * d + a
    return float(Fraction(t) * Fraction(d) + Fraction(a))


class F64Arith:
    """Correctly rounded fp64 with the library's log10 / pow: what the oracle computes, up to the transcendentals' last bits."""
    name = "f64"

    def c(self, x): return float(x)
    def val(self, a): return a
    def add(self, a, b): return a + b
    def sub(self, a, b): return a - b
    def mul(self, a, b): return a * b
    def neg(self, a): return -a

    def div(self, a, b):
        if b == 0.0:
            return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
        return a / b

    def fma(self, t, d, a): return _fma(t, d, a)

    def log10(self, a):
        if a != a or a < 0.0:
            return math.nan
        return -math.inf if a == 0.0 else math.log10(a)

    def exp10(self, a): return float(np.power(10.0, a))
    def log(self, a): return math.log(a) if a > 0 else (-math.inf if a == 0 else math.nan)

    def log1pexp(self, x):
        if x != x:
            return x
        return x + math.log1p(math.exp(-x)) if x > 0 else math.log1p(math.exp(x))

    def isfinite(self, a): return math.isfinite(a)


REF, F64 = RefArith(), F64Arith()

#: the mutants of the power test (one at a time, F64Arith only)
MUTANTS = ("tip_lt", "wdup_lt", "notyet_gt", "clamp_cool_age", "clamp_at_teff", "clamp_at_logg", "weidemann_clamped",
           "heavy_dropped", "light_ignored", "carb_swapped", "db_no_fallback", "log_cool_64ulp")


def lerp(B, a, b, t):
    return B.fma(t, B.sub(b, a), a)


def _kind(ax, xv):
    if xv < ax[0]: return "below"
    if xv > ax[-1]: return "above"
    j = bisect.bisect_left(ax, xv)
    return "node" if j < len(ax) and ax[j] == xv else "interior"


def lookup(B, ax, x, name, tags, clamp=False, near=None):
    """Bracket of x on the ascending axis ax (floats): the largest i <= n-2 with ax[i] <= x, and the extrapolating weight.
    near: a distance inside which a computed x counts as being on a node (its own tolerance)."""
    xv = B.val(x)
    if xv != xv:                                  # NaN: every comparison is false, the searches end at 0
        i = 0
    else:
        i = max(0, min(len(ax) - 2, bisect.bisect_right(ax, xv) - 1))
    kind = _kind(ax, xv) if xv == xv else "nan"
    if near is not None and kind != "node" and xv == xv and any(abs(xv - a) <= near for a in ax):
        kind = "node"
    tags.add(f"{name}:{kind}")
    t = B.div(B.sub(x, B.c(ax[i])), B.sub(B.c(ax[i + 1]), B.c(ax[i])))
    if clamp:
        t = min(max(t, 0.0), 1.0)
    return i, t


class Model:
    """A pack (dict of numpy arrays, base_amd.synth's keys) at one parameter row and population, under arithmetic B."""

    def __init__(self, B, pack, par, pop=0, mut=None):
        self.B, self.pack, self.mut = B, pack, mut
        self.par = [float(x) for x in par]
        if pop:
            self.par[abi.P_Y] = self.par[abi.P_Y2]
        self.nf = int(pack["n_filt"])
        la, fe, yy = (list(map(float, pack[k])) for k in ("log_age", "feh", "y"))
        self.la, self.nA, self.nY = la, len(la), len(yy)
        p = self.par
        self.valid = la[0] <= p[abi.P_LOGAGE] <= la[-1] and fe[0] <= p[abi.P_FEH] <= fe[-1] and \
            (len(yy) == 1 or yy[0] <= p[abi.P_Y] <= yy[-1])
        if not self.valid:
            return
        t = set()
        self.ia, self.ta = lookup(B, la, B.c(p[abi.P_LOGAGE]), "grid_age", t)
        self.i_f, self.tf = lookup(B, fe, B.c(p[abi.P_FEH]), "grid_feh", t)
        self.iy, self.ty = lookup(B, yy, B.c(p[abi.P_Y]), "grid_y", t) if self.nY > 1 else (0, B.c(0.0))
        self.ny = 2 if self.nY > 1 else 1
        first, cnt, off = pack["iso_first_eep"], pack["iso_n_eep"], pack["iso_offset"]
        ks = [((self.i_f + df) * self.nY + self.iy + dy) * self.nA + self.ia + da
              for df in range(2) for dy in range(self.ny) for da in range(2)]
        self.lo = max(int(first[k]) for k in ks)
        self.n = min(int(first[k] + cnt[k]) for k in ks) - self.lo
        self.valid = self.n >= 2
        if not self.valid:
            return
        self._pt = lambda df, dy, da, e: int(off[k := ((self.i_f + df) * self.nY + self.iy + dy) * self.nA + self.ia + da]) + self.lo + e - int(first[k])
        self.mass = [self._derive(e, None) for e in range(self.n)]
        self.massv = [B.val(m) for m in self.mass]
        self.tip = self.mass[-1]
        tips_all = np.asarray(pack["mass"])[np.asarray(off) + np.asarray(cnt) - 1]
        self.tips = {(df, dy): [float(x) for x in tips_all[((self.i_f + df) * self.nY + self.iy + dy) * self.nA:][:self.nA]]
                     for df in range(2) for dy in range(self.ny)}
        self.has_wd = len(pack.get("wc_mass", [])) >= 2 and len(pack.get("at_log_teff", [])) >= 2
        if self.has_wd:
            from base_amd import synth
            self.tracks = [tuple(list(map(float, a)) for a in tr) for tr in synth.wd_cooling_tracks(pack)]
            self.nG, self.nTe = len(pack["at_logg"]), len(pack["at_log_teff"])
            self.at = np.asarray(pack["at_mags"], dtype=np.float64).reshape(-1, self.nG, self.nTe, self.nf)
            self.n_at_type = int(pack.get("n_at_type", self.at.shape[0]))

    def _derive(self, e, f):
        """derived isochrone, EEP e: the mass (f None) or filter f's magnitude -- lerp in age, then Y, then FeH"""
        B, col = self.B, (np.asarray(self.pack["mass"]) if f is None else np.asarray(self.pack["mags"]).reshape(-1, self.nf)[:, f])
        vf = []
        for df in range(2):
            vy = [lerp(B, B.c(col[self._pt(df, dy, 0, e)]), B.c(col[self._pt(df, dy, 1, e)]), self.ta) for dy in range(self.ny)]
            vf.append(lerp(B, vy[0], vy[1], self.ty) if self.ny == 2 else vy[0])
        return lerp(B, vf[0], vf[1], self.tf)

    # ---- the WD chain --------------------------------------------------------------------------------------------------
    def ifmr(self, m, tags):
        B, p, i = self.B, self.par, int(self.pack.get("ifmr_id", abi.IFMR_WILLIAMS))
        c, mm = B.c, B.c(m)
        if i == abi.IFMR_WEIDEMANN:
            mf = [0.55, 0.60, 0.68, 0.79, 0.88, 0.95, 1.02]
            k, t = lookup(B, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], mm, "weidemann", tags, clamp=self.mut == "weidemann_clamped")
            return lerp(B, c(mf[k]), c(mf[k + 1]), t)
        if i == abi.IFMR_WILLIAMS: return B.add(c(0.339), B.mul(c(0.129), mm))
        if i == abi.IFMR_SALARIS_LIN: return B.add(c(0.466), B.mul(c(0.084), mm))
        if i == abi.IFMR_SALARIS_PW:
            tags.add("salaris_pw:" + ("low" if m < 4.0 else "high"))
            return B.add(B.mul(c(0.134), mm), c(0.331)) if m < 4.0 else B.add(B.mul(c(0.047), mm), c(0.679))
        d = B.sub(mm, c(3.0))
        r = B.add(c(p[abi.P_IFMR_INTERCEPT]), B.mul(c(p[abi.P_IFMR_SLOPE]), d))
        if i == abi.IFMR_LINEAR: return r
        return B.add(r, B.mul(B.mul(c(p[abi.P_IFMR_QUAD]), d), d))

    def prec_corner(self, tips, m, tags):
        B, la, na = self.B, self.la, self.nA
        for j, nm in ((0, "0"), (1, "1"), (na - 2, "na-2"), (na - 1, "na-1")):
            if m == tips[j]: tags.add("corner:on_tip[" + nm + "]")
        if m > tips[0] and self.mut != "heavy_dropped":
            tags.add("corner:heavy")
            return B.sub(B.c(la[0]), B.mul(B.c(2.7), B.log10(B.div(B.c(m), B.c(tips[0])))))
        if m > tips[0]:
            return B.c(la[0])
        if m <= tips[na - 1] and self.mut != "light_ignored":
            tags.add("corner:light")
            return B.c(la[na - 1])
        lo = 0                                     # descending column: the largest i <= na-2 with tips[i] >= m
        for i in range(na - 1):
            if tips[i] >= m: lo = i
        a, b = tips[lo], tips[lo + 1]
        if b == a or (lo > 0 and tips[lo - 1] == a) or (tips[lo + 1] == m and lo + 2 < na and tips[lo + 2] == m):
            tags.add("corner:equal_tips")
        tags.add("corner:inside")
        t = B.div(B.sub(B.c(m), B.c(a)), B.sub(B.c(b), B.c(a))) if b != a else B.c(0.0)
        return lerp(B, B.c(la[lo]), B.c(la[lo + 1]), t)

    def wd_chain(self, m, tags, out, stop=None):
        """status (WD_NOMODELS / WD_NOTYET / WD); fills out[...] with the intermediates.  stop="log_cool": no further."""
        B, p = self.B, self.par
        if not self.has_wd:
            return WD_NOMODELS
        pc = {}
        for k in self.tips:
            ct = set()
            pc[k] = self.prec_corner(self.tips[k], m, ct)
            tags |= ct
            out.setdefault("corner_kind", {})[k] = "heavy" if "corner:heavy" in ct else ("light" if "corner:light" in ct else "inside")
        out["prec_corner"] = pc
        kinds = set(out["corner_kind"].values())
        if len(kinds) > 1:
            tags.add("corners:mixed(" + "+".join(sorted(kinds)) + ")")
        elif kinds == {"heavy"}:
            tags.add("corners:all_heavy")
        vf = [lerp(B, pc[(df, 0)], pc[(df, 1)], self.ty) if self.ny == 2 else pc[(df, 0)] for df in range(2)]
        prec = out["prec"] = lerp(B, vf[0], vf[1], self.tf)
        log_age = p[abi.P_LOGAGE]
        wd_mass = out["wd_mass"] = self.ifmr(m, tags)
        dead = B.val(prec) > log_age if self.mut == "notyet_gt" else B.val(prec) >= log_age
        if dead:
            return WD_NOTYET
        A, P = B.exp10(B.c(log_age)), B.exp10(prec)
        diff = B.sub(A, P)
        out["kappa"] = B.val(A) / B.val(diff) if B.val(diff) > 0 else math.inf
        log_cool = B.log10(diff)
        if self.mut == "log_cool_64ulp":
            log_cool = log_cool + 64 * math.ulp(log_cool)
        out["log_cool"] = log_cool
        if stop == "log_cool":
            return WD
        # cooling tracks
        wm, wc = list(map(float, self.pack["wc_mass"])), list(map(float, self.pack["wc_carb"]))
        mv = B.val(wd_mass)
        tags.add("wd_mass:" + ("nonpositive" if not mv > 0 else ("tiny" if mv < 1e-6 else "positive")))
        im, tm = lookup(B, wm, wd_mass, "wc_mass", tags)
        nc = 2 if len(wc) > 1 else 1
        ic, tc = lookup(B, wc, B.c(p[abi.P_CARBONICITY]), "wc_carb", tags) if nc == 2 else (0, B.c(0.0))
        if self.mut == "carb_swapped" and nc == 2:
            tc = B.sub(B.c(1.0), tc)
        near = self._near(log_cool)
        res = []
        for q in (1, 2):
            vc = []
            for dc in range(nc):
                vm = []
                for dm in range(2):
                    age, tab = self.tracks[(ic + dc) * len(wm) + im + dm][0], self.tracks[(ic + dc) * len(wm) + im + dm][q]
                    tt = set()
                    ia, ta = lookup(B, age, log_cool, "wc_age", tt, clamp=self.mut == "clamp_cool_age", near=near)
                    if q == 1:
                        tags |= tt
                        out.setdefault("age_kinds", []).append((len(age), next(iter(tt)).split(":")[1]))
                    vm.append(lerp(B, B.c(tab[ia]), B.c(tab[ia + 1]), ta))
                vc.append(lerp(B, vm[0], vm[1], tm))
            res.append(lerp(B, vc[0], vc[1], tc) if nc == 2 else vc[0])
        ak = [k for _, k in out["age_kinds"]]
        if len(set(ak)) > 1:
            tags.add("wc_age:mixed(" + "+".join(sorted(set(ak))) + ")")
        if any(n == 2 for n, _ in out["age_kinds"]):
            tags.add("wc_age:two_point_track")
        out["log_teff"], out["log_radius"] = res
        out["logg"] = B.sub(B.add(B.c(LOG_G_PLUS_LOG_MSUN), B.log10(wd_mass)), B.mul(B.c(2.0), res[1]))
        return WD

    def _near(self, x):
        """the distance inside which a computed value counts as on a node: its own tolerance (reference arithmetic only)"""
        return float(2 * x.e + 2 * U * abs(x.v)) if isinstance(x, V) else None

    def atmosphere(self, ch, wd_type, tags):
        B = self.B
        ty = 1 if (wd_type > 0 and (self.n_at_type > 1 or self.mut == "db_no_fallback")) else 0
        if wd_type > 0:
            tags.add("atm:DB" if self.n_at_type > 1 else "atm:DB_falls_back_to_DA")
        ty = min(ty, self.at.shape[0] - 1) if self.mut != "db_no_fallback" else ty
        it, tt = lookup(B, list(map(float, self.pack["at_log_teff"])), ch["log_teff"], "at_teff", tags,
                        clamp=self.mut == "clamp_at_teff", near=self._near(ch["log_teff"]))
        ig, tg = lookup(B, list(map(float, self.pack["at_logg"])), ch["logg"], "at_logg", tags,
                        clamp=self.mut == "clamp_at_logg", near=self._near(ch["logg"]))
        if ty >= self.at.shape[0]:                 # the mutant reads a table that is not there: any wrong number will do
            return [B.c(0.0)] * self.nf
        out = []
        for f in range(self.nf):
            v = [lerp(B, B.c(self.at[ty, ig + dg, it, f]), B.c(self.at[ty, ig + dg, it + 1, f]), tt) for dg in range(2)]
            out.append(lerp(B, v[0], v[1], tg))
        return out

    def component(self, m, wd_type, tags, out):
        """Absolute magnitudes of one component (a list, or None for "no flux") and its branch tag."""
        B = self.B
        m = float(m)
        if not m > 0.0:
            return None, DNE
        tipv = B.val(self.tip)
        if (m < tipv) if self.mut == "tip_lt" else (m <= tipv):
            if m < self.massv[0]:
                return None, BELOW_FIRST
            lo = max(0, min(self.n - 2, bisect.bisect_right(self.massv, m) - 1))
            tags.add("iso_mass:" + _kind(self.massv, m))
            a, d = self.mass[lo], B.sub(self.mass[lo + 1], self.mass[lo])
            t = B.div(B.sub(B.c(m), a), d) if B.val(d) > 0 else B.c(0.0)
            return [lerp(B, self._derive(lo, f), self._derive(lo + 1, f), t) for f in range(self.nf)], MSRGB
        if not ((m < self.pack["m_wd_up"]) if self.mut == "wdup_lt" else (m <= self.pack["m_wd_up"])):
            return None, NSBH
        st = self.wd_chain(m, tags, out)
        if st == WD_NOMODELS:
            return None, st
        if st == WD_NOTYET:
            return [B.c(-4.0)] * self.nf, st
        return self.atmosphere(out, wd_type, tags), st


def log_mass_norm(m_wd_up):
    Phi = lambda x: M.erfc(-x / M.sqrt(2)) / 2
    zup, zlo = (M.log10(M.mpf(m_wd_up)) - M.mpf(MF_MU)) / M.mpf(MF_SIGMA), (M.mpf(-1) - M.mpf(MF_MU)) / M.mpf(MF_SIGMA)
    return M.ln(1 / (M.mpf(MF_SIGMA) * M.sqrt(2 * M.pi) * (Phi(zup) - Phi(zlo))))


def log_prior_mass(m, m_wd_up):
    """(value, budget): log c - z^2/2 - log m - log ln 10, about ten fp64 operations and two library calls on the host"""
    m = M.mpf(m)
    z = (M.log10(m) - M.mpf(MF_MU)) / M.mpf(MF_SIGMA)
    terms = [log_mass_norm(m_wd_up), -z * z / 2, -M.ln(m), -M.ln(M.ln(M.mpf(10)))]
    v = sum(terms)
    return v, 16 * U * sum(abs(t) for t in terms) + 16 * U * abs(z) * (abs(z) + 1)


def evaluate(pack, par, pop, m1, q, wd_type, obs=None, sigma=None, prior=1.0, log_fs=None, B=REF, mut=None, model=None):
    """The whole system under arithmetic B.  Returns a dict: tags (set), branch (per component), the primary's intermediates,
    abs_mags / app_mags (lists; None = exactly B9_MAG_NOFLUX, "nan" = not a number) and, with obs and sigma, ll (the
    population's log-likelihood), value (the per-star mixture value) -- under REF each a V with its budget."""
    md = model if model is not None else Model(B, pack, par, pop, mut)
    r = dict(tags=set(), branch=[], model=md)
    if not md.valid:
        r["branch"] = ["row_outside_grid"]
        return r
    B, nf, p = md.B, md.nf, md.par
    inter = {}
    c1, b1 = md.component(m1, wd_type, r["tags"], inter)
    r["branch"].append(b1)
    r.update({k: inter.get(k) for k in ("prec_corner", "corner_kind", "prec", "wd_mass", "log_cool", "log_teff", "log_radius", "logg", "kappa")})
    c2 = None
    if q > 0.0:
        i2 = {}
        c2, b2 = md.component(float(np.float64(q) * np.float64(m1)), wd_type, r["tags"], i2)
        r["branch"].append(b2)
        r["kappa"] = max(x for x in (r["kappa"], i2.get("kappa")) if x is not None) if (r["kappa"] or i2.get("kappa")) else None
    if c1 is None and (c2 is None):
        r["tags"].add("system:no_flux")
    nanv = lambda x: B.val(x) != B.val(x) or not B.isfinite(x)
    ab, ap, lk = [], [], []                        # lk: what the likelihood sees (a dark component counts as B9_MAG_NOFLUX there)
    k1, k2 = B.c(2.5 / 2.302585092994045684), B.c(-0.4 * 2.302585092994045684)
    for f in range(nf):
        a, b = (c1[f] if c1 is not None else None), (c2[f] if c2 is not None else None)
        dark = a is None and (b is None or not q > 0.0)
        a = a if a is not None else B.c(NOFLUX)
        if q > 0.0 and not nanv(a):
            b = b if b is not None else B.c(NOFLUX)
            a = B.sub(a, B.mul(k1, B.log1pexp(B.mul(k2, B.sub(b, a))))) if not nanv(b) else b
        if nanv(a):
            ab.append("nan"); ap.append("nan"); lk.append("nan"); continue
        shift = B.add(B.c(p[abi.P_MOD]), B.mul(B.c(float(np.float64(pack["abs_coeff"][f]) - 1.0)), B.c(p[abi.P_ABS])))
        lk.append(B.add(a, shift))
        ab.append(None if dark else a); ap.append(None if dark else lk[-1])
    r["like_mags"] = lk
    r["abs_mags"], r["app_mags"] = ab, ap
    if obs is not None:
        r.update(loglike(B, pack, r, m1, obs, sigma, prior, log_fs))
    return r


def loglike(B, pack, r, m1, obs, sigma, prior, log_fs):
    """ll = logPriorMass(m1) + sum_f -1/2 [log(2 pi sigma^2) + (pred - obs)^2 / sigma^2]; value = the field-star mixture.
    A filter without flux predicts B9_MAG_NOFLUX; a non-finite prediction makes the star impossible."""
    nf = len(obs)
    impossible = any(a == "nan" for a in r["app_mags"])
    if B is REF:
        lpm, e = log_prior_mass(m1, pack["m_wd_up"])
        c0 = V(lpm, e)
    else:
        lpm, _ = log_prior_mass(m1, pack["m_wd_up"])
        c0 = float(lpm)
    chi2 = B.c(0.0)
    for f in range(nf):
        if not sigma[f] > 0.0:
            continue
        var = float(sigma[f]) * float(sigma[f])
        g = -0.5 * M.ln(2 * M.pi * M.mpf(var))
        c0 = V(c0.v + g, c0.e + 4 * U * abs(g) + U * abs(c0.v + g)) if B is REF else float(M.mpf(c0) + g)
        if impossible:
            continue
        pr = r["like_mags"][f]
        d = B.sub(pr, B.c(float(obs[f])))
        w = B.div(B.c(1.0), B.c(var))
        chi2 = B.add(chi2, B.mul(B.mul(w, d), d))
    out = dict(c0=c0)
    if impossible:
        out["ll"] = None                           # -inf
        out["value"] = None if prior >= 1.0 else (V(M.ln(1 - M.mpf(prior)) + M.mpf(log_fs), 8 * U * abs(log_fs)) if B is REF
                                                  else math.log1p(-prior) + log_fs)
        return out
    ll = B.sub(c0, B.mul(B.c(0.5), chi2))
    out["ll"] = ll
    if prior >= 1.0:
        out["value"] = ll
    elif B is REF:
        a, b = M.ln(1 - M.mpf(prior)) + M.mpf(log_fs), M.ln(M.mpf(prior)) + ll.v
        v = max(a, b) + M.log1p(M.exp(-abs(a - b)))
        out["value"] = V(v, ll.e + 8 * U * (abs(a) + abs(b)) + M.mpf("4e-16") + 2 * U * abs(v))
    else:
        a, b = math.log1p(-prior) + log_fs, math.log(prior) + ll
        out["value"] = max(a, b) + math.log1p(math.exp(-abs(a - b)))
    return out


def tolerance(x):
    """2 x budget + 1 ulp of the value (the factor 2 covers the second-order terms)"""
    return float(2 * x.e) + math.ulp(float(x.v))
