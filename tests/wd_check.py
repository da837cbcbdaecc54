"""numpy restatement of the WD chain up to the atmosphere lookup, following oracle/b9_oracle.c :: wd_mags line by line
(precursor age per corner -> interpolation in Y and FeH -> IFMR -> cooling age -> cooling tracks -> log g), and the
atmosphere lookup on its own.  What b9_sample_wd_mass reports as derived values is checked against this; the helper itself
is tied to synth.forward_mags (a forward model the GPU is already tested against) by tests/test_wdmass_host.py."""
import numpy as np

from base_amd import abi, synth

LOG_G_PLUS_LOG_MSUN = 26.12302173752
ZAMS_RTOL = 1e-12         # a drawn ZAMS mass against the node it names (tests/test_gpu_wdmass.py, tests/ragged_chain.py)


def ifmr(pack, par, m):
    """The initial-final mass relation as oracle/b9_oracle.c :: ifmr states it.  synth._ifmr is the same except for
    Weidemann's table, which the oracle (and the device) extrapolates along its end segments where np.interp clamps."""
    m = np.asarray(m, dtype=np.float64)
    if pack.get("ifmr_id", abi.IFMR_WILLIAMS) == abi.IFMR_WEIDEMANN:
        mf = np.array([0.55, 0.60, 0.68, 0.79, 0.88, 0.95, 1.02])
        i = np.clip(np.floor(m).astype(int) - 1, 0, 5)
        return mf[i] + (m - (i + 1.0)) * (mf[i + 1] - mf[i])
    return synth._ifmr(pack, par, m) * np.ones_like(m)


def wd_chain(pack, par, m, pop=0):
    """(wd_mass, prec_log_age, log_cool_age, log_teff, logg) of WD progenitors of ZAMS mass m (array) at parameter row par,
    population pop (1: B9_P_Y2 takes the place of B9_P_Y).  Where the precursor has not died yet (prec >= logAge) the last
    three are 0, as b9_sample_wd_mass reports them."""
    par = np.asarray(par, dtype=np.float64).copy()
    if pop:
        par[abi.P_Y] = par[abi.P_Y2]
    m = np.atleast_1d(np.asarray(m, dtype=np.float64))
    la, fe, yy = pack["log_age"], pack["feh"], pack["y"]
    nA, nY = len(la), len(yy)
    i_f, tf = synth._bracket(fe, par[abi.P_FEH])
    iy, ty = synth._bracket(yy, par[abi.P_Y]) if nY > 1 else (0, 0.0)
    tips_all = pack["mass"][pack["iso_offset"] + pack["iso_n_eep"] - 1]

    def corner(ifeh, iyy):                      # prec_log_age_corner: invert the AGB-tip-mass(age) curve
        tips = tips_all[(ifeh * nY + iyy) * nA:(ifeh * nY + iyy) * nA + nA]
        out = np.interp(-m, -tips, la)
        return np.where(m > tips[0], la[0] - 2.7 * np.log10(np.maximum(m, 1e-30) / tips[0]), out)

    vf = []
    for df in range(2):                         # wd_prec_log_age: Y, then FeH
        vy = [corner(i_f + df, iy + dy) for dy in range(2 if nY > 1 else 1)]
        vf.append(vy[0] + ty * (vy[1] - vy[0]) if nY > 1 else vy[0])
    prec = vf[0] + tf * (vf[1] - vf[0])
    log_age = par[abi.P_LOGAGE]
    not_yet = prec >= log_age
    wdm = ifmr(pack, par, m)
    with np.errstate(invalid="ignore", divide="ignore"):
        cool = np.log10(np.maximum(10.0 ** log_age - 10.0 ** prec, 1e-300))
    nC, nM = len(pack["wc_carb"]), len(pack["wc_mass"])
    tracks = synth.wd_cooling_tracks(pack)
    im, tm = synth._lin(pack["wc_mass"], wdm)
    if nC > 1:
        ic, tc = synth._lin(pack["wc_carb"], np.full_like(m, par[abi.P_CARBONICITY]))
    else:
        ic, tc = np.zeros_like(im), np.zeros_like(tm)

    def along(q, t_idx):                        # a quantity along each star's track, at its cooling age (own axis per track)
        out = np.empty(len(m))
        for t in np.unique(t_idx):
            sel = t_idx == t
            age, tab = tracks[t][0], tracks[t][q]
            ia, ta = synth._lin(age, cool[sel])
            out[sel] = tab[ia] + ta * (tab[ia + 1] - tab[ia])
        return out

    def tri(q):                                 # across mass, then across carbonicity
        def at_c(icc):
            a0, a1 = along(q, icc * nM + im), along(q, icc * nM + im + 1)
            return a0 + tm * (a1 - a0)
        if nC > 1:
            c0, c1 = at_c(ic), at_c(ic + 1)
            return c0 + tc * (c1 - c0)
        return at_c(ic)

    lteff, lrad = tri(1), tri(2)
    logg = LOG_G_PLUS_LOG_MSUN + np.log10(wdm) - 2.0 * lrad
    cool, lteff, logg = (np.where(not_yet, 0.0, x) for x in (cool, lteff, logg))
    return wdm, prec, cool, lteff, logg


def atmosphere_mags(pack, log_teff, logg, wd_type):
    """Absolute magnitudes [n, n_filt] of the atmosphere table at (log Teff, log g): the last step of wd_mags."""
    nf = pack["n_filt"]
    log_teff, logg = np.atleast_1d(log_teff), np.atleast_1d(logg)
    nG, nTe = len(pack["at_logg"]), len(pack["at_log_teff"])
    at = pack["at_mags"].reshape(-1, nG, nTe, nf)
    tyv = np.where((np.asarray(wd_type) > 0) & (at.shape[0] > 1), 1, 0) * np.ones(len(log_teff), dtype=int)
    it, tt = synth._lin(pack["at_log_teff"], log_teff)
    ig, tg = synth._lin(pack["at_logg"], logg)
    g0 = at[tyv, ig, it] + tt[:, None] * (at[tyv, ig, it + 1] - at[tyv, ig, it])
    g1 = at[tyv, ig + 1, it] + tt[:, None] * (at[tyv, ig + 1, it + 1] - at[tyv, ig + 1, it])
    return g0 + tg[:, None] * (g1 - g0)


def apparent(pack, par, mags):
    return mags + par[abi.P_MOD] + (np.asarray(pack["abs_coeff"])[None, :] - 1.0) * par[abi.P_ABS]
