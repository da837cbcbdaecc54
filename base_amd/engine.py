"""Python front-end over the C ABI (include/base9_hip.h) -- used by tests, bench and the
walker-parallel driver.  Everything numeric happens in libbase9hip.so on the GPU; this class
only pins buffers and forwards calls.  It raises if the library or a GPU is missing: the hot
path has no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np

from . import abi

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class B9Error(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"base9_hip error {code}: {msg}")
        self.code = code


class Engine:
    """One context on one GPU: `Engine(pack, stars, priors, options).logpost(params)`."""

    def __init__(self, pack: Optional[abi.Pinned] = None, stars: Optional[abi.Pinned] = None,
                 priors: Optional[abi.b9_priors] = None, options: Optional[abi.b9_options] = None,
                 device: int = -1, lib: Optional[C.CDLL] = None):
        self.lib = lib or abi.load_hip_library()
        self._ctx = C.c_void_p()
        rc = self.lib.b9_ctx_create(int(device), C.byref(self._ctx))
        if rc != abi.B9_OK:
            msg = self.lib.b9_last_error(None).decode()
            self._ctx = C.c_void_p()
            raise B9Error(rc, msg)
        self.n_stars = 0
        self.n_filt = 0
        if pack is not None:
            self.load_pack(pack)
        if stars is not None:
            self.load_stars(stars)
        if priors is not None:
            self.set_priors(priors)
        self.options = abi.make_options()                # the context's defaults
        if options is not None:
            self.set_options(options)

    # -- plumbing -------------------------------------------------------------------------
    def _check(self, rc: int) -> None:
        if rc != abi.B9_OK:
            raise B9Error(rc, self.lib.b9_last_error(self._ctx).decode())

    def close(self) -> None:
        if getattr(self, "_ctx", None) and self._ctx.value:
            self.lib.b9_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- staging --------------------------------------------------------------------------
    def load_pack(self, pack: abi.Pinned) -> None:
        self._check(self.lib.b9_load_pack(self._ctx, pack.byref()))
        self.n_filt = pack.struct.n_filt
        # the largest mass a node can take: the isochrones' and the WD-stage steps' (hostlib.star_intervals' first edges)
        self.max_mass = max(float(np.ctypeslib.as_array(pack.struct.mass, (int(pack.struct.n_points),)).max()), float(pack.struct.m_wd_up))

    def load_stars(self, stars: abi.Pinned) -> None:
        self._check(self.lib.b9_load_stars(self._ctx, stars.byref()))
        self.n_stars = stars.struct.n_stars
        self.wd_index = np.flatnonzero(np.asarray(stars.keep["stage"]) == abi.STAGE_WD)

    def set_priors(self, priors: abi.b9_priors) -> None:
        self._check(self.lib.b9_set_priors(self._ctx, C.byref(priors)))

    def set_options(self, options: abi.b9_options) -> None:
        self._check(self.lib.b9_set_options(self._ctx, C.byref(options)))
        self.options = options

    def set_tuning(self, **fields) -> None:
        """b9_set_tuning: launch-plan fields of abi.b9_tuning by name (tiles_per_block=3, ...); no argument = automatic."""
        t = abi.b9_tuning()
        for k, v in fields.items():
            if not hasattr(t, k):
                raise AttributeError(f"b9_tuning has no field {k}")
            setattr(t, k, int(v))
        self._check(self.lib.b9_set_tuning(self._ctx, C.byref(t)))

    def update_tuning(self, **fields) -> None:
        """b9_get_tuning + b9_set_tuning: change the named fields only (the environment's overrides and earlier settings stay)."""
        t = abi.b9_tuning()
        self._check(self.lib.b9_get_tuning(self._ctx, C.byref(t)))
        for k, v in fields.items():
            if not hasattr(t, k):
                raise AttributeError(f"b9_tuning has no field {k}")
            setattr(t, k, int(v))
        self._check(self.lib.b9_set_tuning(self._ctx, C.byref(t)))

    # -- hot path -------------------------------------------------------------------------
    def logpost(self, params: np.ndarray, perstar: bool = False):
        params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
        nw = params.shape[0]
        out = np.empty(nw)
        ps = np.empty((nw, self.n_stars)) if perstar else None
        self._check(self.lib.b9_logpost(self._ctx, params.ctypes.data_as(_dp), nw, out.ctypes.data_as(_dp),
                                        ps.ctypes.data_as(_dp) if perstar else None))
        return (out, ps) if perstar else out

    def logpost_device(self, d_params: int, n_walkers: int, d_logpost: int, d_perstar: int = 0,
                       stream: int = 0) -> None:
        """Asynchronous, device pointers (ints, e.g. torch.Tensor.data_ptr())."""
        self._check(self.lib.b9_logpost_device(self._ctx, C.c_void_p(d_params), int(n_walkers),
                                               C.c_void_p(d_logpost), C.c_void_p(d_perstar or None),
                                               C.c_void_p(stream or None)))

    def mcmc_run_block(self, params, logpost, walker_ids, free, chol, seed, step0, n_steps, record=True):
        """Device-resident Metropolis block (b9_mcmc_run_block).  Same contract as
        mcmc.HostBlockRunner.run: returns (params, logpost, samples, lps, n_accept)."""
        return self.mcmc_collect(self.mcmc_submit(params, logpost, walker_ids, free, chol, seed, step0, n_steps, record,
                                                  cont=False, asynchronous=False))

    def mcmc_submit(self, params, logpost, walker_ids, free, chol, seed, step0, n_steps, record=True, cont=False,
                    asynchronous=True, row_origin=None, rows_event=False):
        """Enqueue a block (B9_BLOCK_ASYNC) -- with cont=True from the state the previous block left on the device
        (B9_BLOCK_CONTINUE; params / logpost then only give the shapes).  Returns a handle for mcmc_collect; at
        most two handles may be outstanding and they are collected in submission order.  With `row_origin` the
        handle's "rows" receive the block's per-walker summary rows (b9_mcmc_block::rows); rows_event adds
        B9_BLOCK_ROWS_EVENT (the block's rows_ready event is recorded behind its last kernel)."""
        params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, abi.B9_NPARAM).copy()
        W, d = params.shape[0], len(free)
        logpost = np.ascontiguousarray(logpost, dtype=np.float64).copy()
        keep = dict(params=params, logpost=logpost, free=np.ascontiguousarray(free, dtype=np.int32),
                    ids=np.ascontiguousarray(walker_ids, dtype=np.int32), chol=np.ascontiguousarray(chol, dtype=np.float64),
                    samples=np.empty((n_steps, W, d)) if record else None, lps=np.empty((n_steps, W)) if record else None)
        blk = abi.b9_mcmc_block()
        blk.n_walkers, blk.n_free = W, d
        blk.free_idx = keep["free"].ctypes.data_as(_ip)
        blk.chol = keep["chol"].ctypes.data_as(_dp)
        blk.walker_ids = keep["ids"].ctypes.data_as(_ip)
        blk.seed, blk.step0, blk.n_steps = int(seed), int(step0), int(n_steps)
        blk.flags = (abi.BLOCK_CONTINUE if cont else 0) | (abi.BLOCK_ASYNC if asynchronous else 0) | (abi.BLOCK_ROWS_EVENT if rows_event else 0)
        blk.params = params.ctypes.data_as(_dp)
        blk.logpost = logpost.ctypes.data_as(_dp)
        blk.samples = keep["samples"].ctypes.data_as(_dp) if record else None
        blk.lps = keep["lps"].ctypes.data_as(_dp) if record else None
        if row_origin is not None:      # the block's last launch also condenses every walker's chain into a summary row
            keep["origin"] = np.ascontiguousarray(row_origin, dtype=np.float64)
            keep["rows"] = np.empty((W, abi.row_doubles(d)))
            blk.row_origin = keep["origin"].ctypes.data_as(_dp)
            blk.rows = keep["rows"].ctypes.data_as(_dp)
        self._check(self.lib.b9_mcmc_run_block(self._ctx, C.byref(blk)))
        keep["blk"], keep["pending"] = blk, bool(asynchronous and n_steps > 0)
        return keep

    def mcmc_collect(self, h):
        if h["pending"]:
            self._check(self.lib.b9_mcmc_wait(self._ctx, C.byref(h["blk"])))
            h["pending"] = False
        return h["params"], h["logpost"], h["samples"], h["lps"], int(h["blk"].n_accept)

    def sample_mass(self, params: np.ndarray, seed: int = 1, row0: int = 0):
        """b9_sample_mass: per (row, star) one Gumbel-max draw of (primary mass, mass ratio, population) on the
        marginalisation grid + the membership probability.  Returns (mass, ratio, member, pop), each [rows, n_stars]."""
        params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
        nr = params.shape[0]
        mass, ratio, member = (np.empty((nr, self.n_stars)) for _ in range(3))
        pop = np.empty((nr, self.n_stars), dtype=np.int32)
        self._check(self.lib.b9_sample_mass(self._ctx, params.ctypes.data_as(_dp), nr, int(seed), int(row0),
                                            mass.ctypes.data_as(_dp), ratio.ctypes.data_as(_dp), member.ctypes.data_as(_dp),
                                            pop.ctypes.data_as(C.POINTER(C.c_int32))))
        return mass, ratio, member, pop

    WD_DERIVED = ("wd_mass", "prec_log_age", "log_cool_age", "log_teff", "logg")

    def n_wd_stars(self) -> int:
        r = int(self.lib.b9_n_wd_stars(self._ctx))
        if r < 0:
            self._check(r)
        return r

    def sample_wd_mass(self, params: np.ndarray, n_nodes: int, seed: int = 1, row0: int = 0, derived=WD_DERIVED):
        """b9_sample_wd_mass: per (row, WD-stage star) one Gumbel-max draw of the ZAMS mass on n_nodes equal steps above the
        AGB tip, the membership probability and the quantities that follow from the drawn mass.  Returns a dict of
        [rows, n_wd] arrays -- zams, member, pop and the `derived` ones (any subset of WD_DERIVED; the others are not
        computed) -- plus star_index, the WD-stage stars' indices in the catalogue."""
        params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
        nr, n_wd = params.shape[0], self.n_wd_stars()
        names = ("zams",) + self.WD_DERIVED + ("member",)
        out = {k: (np.zeros((nr, n_wd)) if k in ("zams", "member") or k in derived else None) for k in names}
        pop = np.zeros((nr, n_wd), dtype=np.int32)
        ptr = [out[k].ctypes.data_as(_dp) if out[k] is not None else None for k in names]
        self._check(self.lib.b9_sample_wd_mass(self._ctx, params.ctypes.data_as(_dp), nr, int(n_nodes), int(seed), int(row0),
                                               *ptr, pop.ctypes.data_as(_ip)))
        res = {k: v for k, v in out.items() if v is not None}
        res["pop"] = pop
        res["star_index"] = self.wd_index.copy()
        return res

    def wd_moments(self, params: np.ndarray, n_nodes: int, acc: Optional[np.ndarray] = None):
        """b9_wd_moments: the WD-stage stars' posterior moments of the ZAMS mass and the five derived values over `params`'
        rows on b9_sample_wd_mass's grid of n_nodes steps, exactly (no draws).  Returns (acc [n_wd, abi.WDM_N], star_index):
        the accumulators in the order of sample_wd_mass's columns and those stars' indices in the catalogue.  acc=None starts
        from zeros; else the call continues `acc` (B9_WDM_CONTINUE) and returns a new array."""
        params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
        n_wd = self.n_wd_stars()
        if acc is None:
            out, flags = np.zeros((n_wd, abi.WDM_N)), 0
        else:
            out, flags = np.array(acc, dtype=np.float64, order="C").reshape(n_wd, abi.WDM_N), abi.WDM_CONTINUE
        self._check(self.lib.b9_wd_moments(self._ctx, params.ctypes.data_as(_dp), params.shape[0], int(n_nodes), flags, out.ctypes.data_as(_dp)))
        return out, self.wd_index.copy()

    def wd_bins(self, rows: np.ndarray, n_nodes: int, edges: np.ndarray, quantities: int = abi.WQ_ALL, acc: Optional[np.ndarray] = None):
        """b9_wd_bins: the WD-stage stars' node weights over `rows` on b9_wd_moments' grid of n_nodes steps, binned on every line's
        OWN edges `edges` [n_wd, n_sel, n_bins + 1] -- a line is (WD-stage star, selected quantity of the mask `quantities`, bit
        abi.WQ_*, ascending).  Returns (acc [n_wd, n_sel, n_bins + 3] -- below, the bins, at or above, the total (membership) --,
        star_index).  acc=None starts from zeros; else the call continues `acc` (B9_WBIN_CONTINUE) and returns a new array."""
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
        n_wd, n_sel = self.n_wd_stars(), bin(int(quantities) & 0xffffffff).count("1")
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        n_bins = edges.shape[-1] - 1
        edges = edges.reshape(n_wd, max(n_sel, 1), n_bins + 1)
        if acc is None:
            out, flags = np.zeros((n_wd, max(n_sel, 1), n_bins + 3)), 0
        else:
            out, flags = np.array(acc, dtype=np.float64, order="C").reshape(n_wd, max(n_sel, 1), n_bins + 3), abi.WBIN_CONTINUE
        self._check(self.lib.b9_wd_bins(self._ctx, rows.ctypes.data_as(_dp), rows.shape[0], int(n_nodes), int(quantities), edges.ctypes.data_as(_dp),
                                        n_bins, flags, out.ctypes.data_as(_dp)))
        return out, self.wd_index.copy()

    def star_moments(self, rows: np.ndarray, acc: Optional[np.ndarray] = None) -> np.ndarray:
        """b9_star_moments: the per-star posterior moments [n_stars, abi.MOM_N] summed over `rows`, exactly (no draws).
        acc=None starts from zeros; else the call continues `acc` (B9_MOM_CONTINUE) and returns a new array."""
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
        if acc is None:
            out, flags = np.zeros((self.n_stars, abi.MOM_N)), 0
        else:
            out, flags = np.array(acc, dtype=np.float64, order="C").reshape(self.n_stars, abi.MOM_N), abi.MOM_CONTINUE
        self._check(self.lib.b9_star_moments(self._ctx, rows.ctypes.data_as(_dp), rows.shape[0], flags, out.ctypes.data_as(_dp)))
        return out

    def mass_hist(self, rows: np.ndarray, edges: np.ndarray, quantity: int = abi.HQ_PRIMARY, star_hist: Optional[np.ndarray] = None,
                  want_star: bool = True, want_rows: bool = True) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
        """b9_mass_hist: the exact binned mass posteriors over `rows` for the bins `edges` [n_bins + 1] of `quantity`
        (abi.HQ_*): (star_hist [n_stars, n_bins + 1] summed over the rows, row_hist [n_rows, n_bins + 1] summed over the
        stars); the last column is the total (membership).  star_hist=None starts from zeros; else the call continues it
        (B9_HIST_CONTINUE) and returns a new array.  want_star / want_rows = False passes NULL for that output (None back)."""
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
        edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        n_bins = len(edges) - 1
        flags = 0
        sh = rh = None
        if want_star:
            if star_hist is None:
                sh = np.zeros((self.n_stars, n_bins + 1))
            else:
                sh, flags = np.array(star_hist, dtype=np.float64, order="C").reshape(self.n_stars, n_bins + 1), abi.HIST_CONTINUE
        if want_rows:
            rh = np.zeros((rows.shape[0], n_bins + 1))
        ptr = lambda a: a.ctypes.data_as(_dp) if a is not None else None      # noqa: E731
        self._check(self.lib.b9_mass_hist(self._ctx, rows.ctypes.data_as(_dp), rows.shape[0], int(quantity), edges.ctypes.data_as(_dp), n_bins, flags,
                                          ptr(sh), ptr(rh)))
        return sh, rh

    def ratio_hist(self, rows: np.ndarray, mass_edges: np.ndarray, star_cells: Optional[np.ndarray] = None, want_star: bool = True,
                   want_rows: bool = True) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
        """b9_ratio_hist: the exact mass-ratio posteriors by primary mass over `rows` for the mass bins `mass_edges`
        [n_mbins + 1]: (star_cells [n_stars, n_mbins Q + 1] summed over the rows, row_cells [n_rows, n_mbins Q + 1] summed over
        the stars), Q = max(1, options.marg_n_q); column b Q + j is (mass bin b, ratio node j), the last column the total (membership).
        star_cells=None starts from zeros; else the call continues it (B9_RH_CONTINUE) and returns a new array.  want_star /
        want_rows = False passes NULL for that output (None back)."""
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
        edges = np.ascontiguousarray(mass_edges, dtype=np.float64).reshape(-1)
        n_mbins = len(edges) - 1
        ncol = max(n_mbins, 0) * max(1, int(self.options.marg_n_q)) + 1
        flags = 0
        sc = rc = None
        if want_star:
            if star_cells is None:
                sc = np.zeros((self.n_stars, ncol))
            else:
                sc, flags = np.array(star_cells, dtype=np.float64, order="C").reshape(self.n_stars, ncol), abi.RH_CONTINUE
        if want_rows:
            rc = np.zeros((rows.shape[0], ncol))
        ptr = lambda a: a.ctypes.data_as(_dp) if a is not None else None      # noqa: E731
        self._check(self.lib.b9_ratio_hist(self._ctx, rows.ctypes.data_as(_dp), rows.shape[0], edges.ctypes.data_as(_dp), n_mbins, flags, ptr(sc), ptr(rc)))
        return sc, rc

    def star_bins(self, rows: np.ndarray, edges: np.ndarray, quantity: int = abi.HQ_PRIMARY, acc: Optional[np.ndarray] = None) -> np.ndarray:
        """b9_star_bins: every star's node weights over `rows` binned on that star's OWN edges `edges` [n_stars, n_bins + 1] of
        `quantity` (abi.HQ_*): acc [n_stars, n_bins + 3] -- below, the bins, at or above, the total (membership).  acc=None
        starts from zeros; else the call continues `acc` (B9_SBIN_CONTINUE) and returns a new array."""
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
        edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(self.n_stars, -1)
        n_bins = edges.shape[1] - 1
        if acc is None:
            out, flags = np.zeros((self.n_stars, n_bins + 3)), 0
        else:
            out, flags = np.array(acc, dtype=np.float64, order="C").reshape(self.n_stars, n_bins + 3), abi.SBIN_CONTINUE
        self._check(self.lib.b9_star_bins(self._ctx, rows.ctypes.data_as(_dp), rows.shape[0], int(quantity), edges.ctypes.data_as(_dp), n_bins, flags,
                                          out.ctypes.data_as(_dp)))
        return out

    def phot_resid(self, rows: np.ndarray, star_resid: Optional[np.ndarray] = None, want_star: bool = True,
                   want_rows: bool = True) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
        """b9_phot_resid: the exact posterior-predictive residuals over `rows`: (star_resid [n_stars, 2 + 2 n_filt] summed over
        the rows -- ROWS, MEMBER, then per filter p sum w d and p sum w d^2 about the star's pivot --, row_resid
        [n_rows, 1 + 5 n_filt] -- sum p, then per filter N, R, C, W, D over the stars that have the filter).  star_resid=None
        starts from zeros; else the call continues it (B9_RESID_CONTINUE) and returns a new array.  want_star / want_rows =
        False passes NULL for that output (None back)."""
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
        nf = self.n_filt
        flags = 0
        sr = rr = None
        if want_star:
            if star_resid is None:
                sr = np.zeros((self.n_stars, 2 + 2 * nf))
            else:
                sr, flags = np.array(star_resid, dtype=np.float64, order="C").reshape(self.n_stars, 2 + 2 * nf), abi.RESID_CONTINUE
        if want_rows:
            rr = np.zeros((rows.shape[0], 1 + 5 * nf))
        ptr = lambda a: a.ctypes.data_as(_dp) if a is not None else None      # noqa: E731
        self._check(self.lib.b9_phot_resid(self._ctx, rows.ctypes.data_as(_dp), rows.shape[0], flags, ptr(sr), ptr(rr)))
        return sr, rr

    def filter_loo(self, rows: np.ndarray, acc: Optional[np.ndarray] = None, want_star: bool = True,
                   want_rows: bool = True) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
        """b9_filter_loo: the exact leave-one-filter-out predictions over `rows`: (star_loo [n_stars, 2 + 3 n_filt] summed over
        the rows -- ROWS, MEMBER, then per filter p sum w^f d, p sum w^f d^2 about the star's pivot and p l_f, the log density of
        the observation under what the other filters predict --, row_loo [n_rows, 1 + 6 n_filt] -- sum p, then per filter N, R,
        C, W, D, E over the stars that have the filter).  acc=None starts from zeros; else the call continues it
        (B9_LOO_CONTINUE) and returns a new array.  want_star / want_rows = False passes NULL for that output (None back)."""
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
        nf = self.n_filt
        flags = 0
        sl = rl = None
        if want_star:
            if acc is None:
                sl = np.zeros((self.n_stars, 2 + 3 * nf))
            else:
                sl, flags = np.array(acc, dtype=np.float64, order="C").reshape(self.n_stars, 2 + 3 * nf), abi.LOO_CONTINUE
        if want_rows:
            rl = np.zeros((rows.shape[0], 1 + 6 * nf))
        ptr = lambda a: a.ctypes.data_as(_dp) if a is not None else None      # noqa: E731
        self._check(self.lib.b9_filter_loo(self._ctx, rows.ctypes.data_as(_dp), rows.shape[0], flags, ptr(sl), ptr(rl)))
        return sl, rl

    def star_offset(self, rows: np.ndarray, k, tau, acc: Optional[np.ndarray] = None, want_star: bool = True,
                    want_rows: bool = True) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
        """b9_star_offset: the exact per-star offsets over `rows` along the directions k [n_dir, n_filt] (mag per unit offset)
        with the prior widths tau [n_dir] (mag; a scalar serves every direction): (star_off [n_stars, 2 + 3 n_dir] summed over
        the rows -- ROWS, MEMBER, then per direction p E[delta], p E[mu^2] and p times the log Bayes factor of the star having an
        offset of its own --, row_off [n_rows, 1 + 4 n_dir] -- sum p, then per direction N, M1, M2, E over the stars the
        direction touches).  acc=None starts from zeros; else the call continues it (B9_OFF_CONTINUE) and returns a new array.
        want_star / want_rows = False passes NULL for that output (None back)."""
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
        k = np.ascontiguousarray(k, dtype=np.float64).reshape(-1, self.n_filt)
        nd = k.shape[0]
        tau = np.ascontiguousarray(np.broadcast_to(np.asarray(tau, dtype=np.float64), (nd,)))
        flags = 0
        so = ro = None
        if want_star:
            if acc is None:
                so = np.zeros((self.n_stars, 2 + 3 * nd))
            else:
                so, flags = np.array(acc, dtype=np.float64, order="C").reshape(self.n_stars, 2 + 3 * nd), abi.OFF_CONTINUE
        if want_rows:
            ro = np.zeros((rows.shape[0], 1 + 4 * nd))
        ptr = lambda a: a.ctypes.data_as(_dp) if a is not None else None      # noqa: E731
        self._check(self.lib.b9_star_offset(self._ctx, rows.ctypes.data_as(_dp), rows.shape[0], flags, nd, ptr(k), ptr(tau), ptr(so), ptr(ro)))
        return so, ro

    def pointwise(self, rows: np.ndarray, tail_len: int = 0, acc: Optional[np.ndarray] = None, tail: Optional[np.ndarray] = None,
                  want_rows: bool = True) -> Tuple[np.ndarray, Optional[np.ndarray], Optional[np.ndarray]]:
        """b9_pointwise: every star's marginal log-likelihood v over `rows`, reduced: (acc [n_stars, 8] -- abi.PW_ROWS .. PW_M2 --,
        tail [n_stars, tail_len] -- the largest -v, descending, padded with -inf; None for tail_len = 0 --, row_lpd [n_rows] --
        the rows' sums over the stars; None for want_rows = False).  acc=None starts from zeros (and the tail from -inf); else the
        call continues acc and tail (B9_PW_CONTINUE) and returns new arrays."""
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
        flags = 0
        if acc is None:
            a = np.zeros((self.n_stars, abi.PW_N))
            t = np.full((self.n_stars, tail_len), -np.inf) if tail_len > 0 else None
        else:
            flags = abi.PW_CONTINUE
            a = np.array(acc, dtype=np.float64, order="C").reshape(self.n_stars, abi.PW_N)
            t = None
            if tail_len > 0:
                if tail is None:
                    raise ValueError("continuing with tail_len > 0 needs the tail of the calls before")
                t = np.array(tail, dtype=np.float64, order="C").reshape(self.n_stars, tail_len)
        rl = np.zeros(rows.shape[0]) if want_rows else None
        ptr = lambda x: x.ctypes.data_as(_dp) if x is not None else None      # noqa: E731
        self._check(self.lib.b9_pointwise(self._ctx, rows.ctypes.data_as(_dp), rows.shape[0], flags, int(tail_len), ptr(a), ptr(t), ptr(rl)))
        return a, t, rl

    def star_influence(self, rows: np.ndarray, q=None, tail_len: int = 0, groups=None, n_groups: int = 0,
                       state=None) -> Tuple[Optional[np.ndarray], Optional[np.ndarray], Optional[np.ndarray]]:
        """b9_star_influence: the leave-one-star-out state of the per-row quantities q [n_rows, n_q] and the groups' sums of v
        over `rows`: (acc [n_stars, 6 + 4 n_q] -- abi.INF_ROWS .. INF_MEANV, then WQ, WQ2, MQ, CVQ per quantity; None for
        q = None --, tail [n_stars, tail_len] -- as Engine.pointwise's; None for tail_len = 0 --, group_lpd [n_rows, n_groups] --
        the sum of v over the stars i with groups[i] == g; None for groups = None).  state=None starts from zeros (the tail
        from -inf); else state = (acc, tail) of the calls before is continued (B9_INF_CONTINUE) and new arrays come back."""
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
        flags, nq = 0, 0
        a = t = gl = g = None
        if q is not None:
            q = np.ascontiguousarray(q, dtype=np.float64).reshape(rows.shape[0], -1)
            nq = q.shape[1]
            if state is None:
                a = np.zeros((self.n_stars, abi.INF_N(nq)))
                t = np.full((self.n_stars, tail_len), -np.inf) if tail_len > 0 else None
            else:
                flags = abi.INF_CONTINUE
                a = np.array(state[0], dtype=np.float64, order="C").reshape(self.n_stars, abi.INF_N(nq))
                if tail_len > 0:
                    if state[1] is None:
                        raise ValueError("continuing with tail_len > 0 needs the tail of the calls before")
                    t = np.array(state[1], dtype=np.float64, order="C").reshape(self.n_stars, tail_len)
        if groups is not None:
            g = np.ascontiguousarray(groups, dtype=np.int32).reshape(self.n_stars)
            gl = np.zeros((rows.shape[0], max(int(n_groups), 0)))
        ptr = lambda x: x.ctypes.data_as(_dp) if x is not None else None      # noqa: E731
        gp = g.ctypes.data_as(C.POINTER(C.c_int32)) if g is not None else None
        self._check(self.lib.b9_star_influence(self._ctx, rows.ctypes.data_as(_dp), rows.shape[0], flags, nq, ptr(q), ptr(a), int(tail_len), ptr(t),
                                               int(n_groups), gp, ptr(gl)))
        return a, t, gl

    def derive_isochrone(self, param_row: np.ndarray, pop: int = 0, cap: int = 4096) -> Tuple[int, np.ndarray, np.ndarray, float]:
        row = np.ascontiguousarray(param_row, dtype=np.float64)
        mass = np.empty(cap)
        mags = np.empty(cap * self.n_filt)
        first, n, tip = C.c_int32(0), C.c_int32(0), C.c_double(0)
        self._check(self.lib.b9_derive_isochrone(self._ctx, row.ctypes.data_as(_dp), pop, cap,
                                                 mass.ctypes.data_as(_dp), mags.ctypes.data_as(_dp),
                                                 C.byref(first), C.byref(n), C.byref(tip)))
        k = n.value
        return first.value, mass[:k].copy(), mags[:k * self.n_filt].reshape(k, self.n_filt).copy(), tip.value

    def predict_mags(self, param_row: np.ndarray, mass1, mass_ratio, wd_type=None, pop=None) -> Tuple[np.ndarray, np.ndarray]:
        """b9_predict_mags: predicted apparent magnitudes [n, n_filt] and stages [n] of n systems at one parameter row
        (B9_MAG_NOFLUX / B9_STAGE_DNE where the row lies outside the grid).  wd_type / pop: None = all DA / all population 0."""
        row = np.ascontiguousarray(param_row, dtype=np.float64).reshape(abi.B9_NPARAM)
        m1 = np.ascontiguousarray(mass1, dtype=np.float64).ravel()
        q = np.ascontiguousarray(mass_ratio, dtype=np.float64).ravel()
        n = m1.size
        if q.size != n:
            raise ValueError("mass1 and mass_ratio differ in length")
        wt = None if wd_type is None else np.ascontiguousarray(wd_type, dtype=np.int32).ravel()
        pp = None if pop is None else np.ascontiguousarray(pop, dtype=np.int32).ravel()
        for a in (wt, pp):
            if a is not None and a.size != n:
                raise ValueError("wd_type / pop differ in length from mass1")
        mags = np.empty((n, self.n_filt))
        stage = np.empty(n, dtype=np.int32)
        self._check(self.lib.b9_predict_mags(self._ctx, row.ctypes.data_as(_dp), n, m1.ctypes.data_as(_dp), q.ctypes.data_as(_dp),
                                             wt.ctypes.data_as(_ip) if wt is not None else None,
                                             pp.ctypes.data_as(_ip) if pp is not None else None,
                                             mags.ctypes.data_as(_dp), stage.ctypes.data_as(_ip)))
        return mags, stage

    def cmd_band(self, rows: np.ndarray, spec, pivot=None, mom=None, edges=None, bins=None, want_mom: bool = True,
                 want_bins: Optional[bool] = None) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
        """b9_cmd_band: the isochrone and WD-sequence lines `spec` (abi.make_band_spec) selects, reduced over `rows`: (mom
        [n_lines, abi.BAND_NMOM] -- N, SUM and SUMSQ about `pivot` [n_lines] (None: 0), MIN, MAX --, bins [n_lines, n_bins + 3] on the
        lines' own `edges` [n_lines, n_bins + 1] -- below, the bins, at or above, the total).  Needs a pack, no stars.  mom / bins
        given: the call continues them (B9_BAND_CONTINUE; both must be given where both are wanted) and returns new arrays.
        want_mom = False passes NULL for the moments; bins are wanted when edges are given (want_bins overrides)."""
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
        st = spec.struct if isinstance(spec, abi.Pinned) else spec
        n_lines = abi.band_shape(st, self.n_filt, 2 if self.options.n_pops == 2 else 1)[2]
        if want_bins is None:
            want_bins = edges is not None
        cont = mom is not None or bins is not None
        if cont and ((want_mom and mom is None) or (want_bins and bins is None)):
            raise ValueError("cmd_band: a continued call takes every output it asks for")
        n_bins = 0
        e = None
        if edges is not None:
            e = np.ascontiguousarray(edges, dtype=np.float64).reshape(max(n_lines, 1), -1)
            n_bins = e.shape[1] - 1
        piv = None if pivot is None else np.ascontiguousarray(pivot, dtype=np.float64).reshape(n_lines)
        m = b = None
        if want_mom:
            m = np.array(mom, dtype=np.float64, order="C").reshape(n_lines, abi.BAND_NMOM) if cont else np.zeros((n_lines, abi.BAND_NMOM))
        if want_bins:
            b = np.array(bins, dtype=np.float64, order="C").reshape(n_lines, n_bins + 3) if cont else np.zeros((n_lines, max(n_bins, 0) + 3))
        ptr = lambda a: a.ctypes.data_as(_dp) if a is not None else None
        self._check(self.lib.b9_cmd_band(self._ctx, rows.ctypes.data_as(_dp), rows.shape[0], C.byref(st), abi.BAND_CONTINUE if cont else 0, ptr(piv), ptr(m),
                                         ptr(e), n_bins, ptr(b)))
        return m, b

    # -- introspection --------------------------------------------------------------------
    def bytes_per_star_eval(self) -> int:
        return int(self.lib.b9_bytes_per_star_eval(self._ctx))

    def step_tiles_per_block(self, n_walkers: int) -> int:
        r = int(self.lib.b9_step_tiles_per_block(self._ctx, int(n_walkers)))
        if r < 0:
            self._check(r)
        return r

    def step_depth(self, n_walkers: int) -> int:
        r = int(self.lib.b9_step_depth(self._ctx, int(n_walkers)))
        if r < 0:
            self._check(r)
        return r

    def device_id(self) -> int:
        return int(self.lib.b9_device_id(self._ctx))

    def max_eep(self) -> int:
        return int(self.lib.b9_max_eep(self._ctx))

    def enable_timing(self, every: int = 1) -> None:
        """0/False: off; n: bracket every n-th launch of the dominant kernel with HIP events."""
        self._check(self.lib.b9_enable_timing(self._ctx, int(every)))

    def calibrate_timing(self) -> float:
        """ms an event bracket adds to a kernel's own duration (measured on an empty kernel)."""
        ms = C.c_double(0)
        self._check(self.lib.b9_calibrate_timing(self._ctx, C.byref(ms)))
        return ms.value

    def clock_stamp(self, which: int) -> None:
        """Enqueue the opening (0) / closing (1) shader-clock stamp on the context's stream."""
        self._check(self.lib.b9_clock_stamp(self._ctx, int(which)))

    def clock_mhz(self) -> Dict:
        """Shader clock between the two stamps: median over the compute units, extremes, length of the stretch (reference clock)."""
        m, lo, hi, sec = C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0)
        self._check(self.lib.b9_clock_mhz(self._ctx, C.byref(m), C.byref(lo), C.byref(hi), C.byref(sec)))
        return {"mhz": m.value, "mhz_min_cu": lo.value, "mhz_max_cu": hi.value, "ref_seconds": sec.value}

    def kernel_time_ms(self, reset: bool = True) -> Tuple[float, int]:
        ms, n = C.c_double(0), C.c_int32(0)
        self._check(self.lib.b9_kernel_time_ms(self._ctx, 1 if reset else 0, C.byref(ms), C.byref(n)))
        return ms.value, n.value


def make_problem(pack_dict: Dict, cluster: Dict, n_pops: int = 1, mode: int = abi.MODE_GIVEN_MASS,
                 marg_iso_increm: int = 8, marg_n_q: int = 8):
    """Pin a synthetic pack + cluster into ABI structs: (pack, stars, priors, options)."""
    from . import synth
    pack = abi.make_pack(pack_dict)
    stars = abi.make_stars(cluster)
    priors = synth.default_priors(pack_dict, cluster["truth"], n_pops)
    options = abi.make_options(mode, n_pops, marg_iso_increm, marg_n_q)
    return pack, stars, priors, options


def star_table(acc: np.ndarray) -> np.ndarray:
    """The derived columns of b9_star_moments' accumulators (hostlib.STAR_TABLE_COLUMNS: rows, member, mass, massSd,
    massRatio, massRatioSd, pBinary, pPop2), [n_stars, 8] -- host arithmetic (b9h_star_table)."""
    from . import hostlib
    return hostlib.star_table(acc)


def wd_table(acc: np.ndarray) -> np.ndarray:
    """The derived columns of b9_wd_moments' accumulators (hostlib.WD_TABLE_COLUMNS: rows, member, pCooled, zamsMass,
    zamsMassSd, then a mean and an sd of wdMass, precLogAge, logCoolAge, logTeff, logg, and pPop2), [n_wd, 16] -- host
    arithmetic (b9h_wd_table)."""
    from . import hostlib
    return hostlib.wd_table(acc)
